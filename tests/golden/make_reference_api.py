"""Writes tests/golden/reference_api.json, the reference's public ABI as tests/test_abi.py compares the product with it: the function names its
public headers declare (the regex of test_abi) and the struct sizes, offsets and constants a C compiler sees through those headers (test_abi.C_PROBE).
Run where a checkout of the reference exists; the output is committed, so the tests need no reference.
    python tests/golden/make_reference_api.py <reference checkout>"""
import json
import os
import pathlib
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_abi  # noqa: E402


def main(ref):
    inc = os.path.join(ref, "libgpujpeg")
    names = set()
    for f in sorted(os.listdir(inc)):
        if f.endswith(".h"):
            names |= set(re.findall(r"\b(gpujpeg_[a-z0-9_]+)\s*\(", open(os.path.join(inc, f)).read()))
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        gen = tmp / "gen" / "libgpujpeg"
        gen.mkdir(parents=True)
        (gen / "gpujpeg_version.h").write_text("#define GPUJPEG_VERSION_MAJOR 0\n#define GPUJPEG_VERSION_MINOR 27\n#define GPUJPEG_VERSION_PATCH 13\n")
        layout = test_abi.probe(ref, tmp, "ref", extra=["-I", str(tmp / "gen")])
    with open(os.path.join(HERE, "reference_api.json"), "w") as f:
        json.dump({"functions": sorted(names), "layout": layout}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
