#!/usr/bin/env python3
"""Progressive (SOF2) decode against the baseline twin of the same picture (dec_opt_progressive = on), on the GPU.

Public API only. One picture per size -- smooth structure plus noise, the kind that compresses like a photograph -- saved by libjpeg (through PIL) at
quality 75, 4:2:0, once progressive (libjpeg's ten-scan script) and once baseline (optimize=False): the same quantised coefficients, so the
baseline file is the twin and both decode to the same bytes (checked here before anything is timed). Streams and pixels are device buffers. The
points are measured in ALTERNATION (each round gives every point a slice of calls), wall clock around calls that end in a synchronise; the figure
of a point is the MEDIAN of its five rounds, with the rounds' minimum and maximum beside it:

    prog     gpujpeg_decoder_decode of the progressive file
    base     the same call on the twin (no restart markers: the single-frame route of any libjpeg file)
    prog2    prog once more: the difference to prog is the spread every other difference has to beat
    pil      PIL (libjpeg-turbo, one CPU thread) decoding the progressive file from memory: what a caller without the option falls back to

and, from one call with perf_stats: the scans, levels (= entropy launches) and segments (= waves) of the progressive frame and its kernel-times
slot [0] (the clear of the planes and the launches of the levels) next to the twin's slot [0].

    python tools/progressive_times.py --out profiles/progressive.json [--calls 20] [--sizes 640x368,1920x1080,3840x2160]

writes the JSON and, beside it, the same figures as a table (.md)."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime per process)

from gpujpeg_amd import libgpujpeg as G  # noqa: E402

ROUNDS = 5


def picture(w, h, seed=7):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    chans = [128 + 90 * np.sin(xx / (37.0 + 11 * c) + c) * np.cos(yy / (53.0 - 7 * c)) + 30 * np.sin((xx + yy) / 9.0 + c) for c in range(3)]
    img = np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def saved(rgb, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=75, subsampling=2, **kw)
    return np.frombuffer(b.getvalue(), np.uint8).copy()


def decoder(lib, perf):
    dec = G.Decoder(lib)
    p, pi = lib.default_parameters(), lib.default_image_parameters()
    p.perf_stats, p.verbose, pi.width, pi.height = int(perf), -1, 0, 0
    assert dec.init(p, pi) == 0
    dec.set_output_format(G.CS_DEFAULT, G.PIXFMT_AUTODETECT)
    assert dec.set_option(G.DEC_OPT_PROGRESSIVE, G.PROGRESSIVE_ON) == 0
    return dec


def measure(lib, w, h, calls):
    from PIL import Image
    rgb = picture(w, h)
    prog, base = saved(rgb, progressive=True), saved(rgb, optimize=False)
    dev = torch.device("cuda:0")
    d_prog, d_base = torch.from_numpy(prog).to(dev), torch.from_numpy(base).to(dev)
    out = torch.empty(w * h * 3 + 64, dtype=torch.uint8, device=dev)
    # the contract first: both files decode to the same bytes
    dec = decoder(lib, True)
    a, _ = dec.decode(prog)
    stats = dec.progressive_stats()
    ms_prog = dec.kernel_times()[0]
    b, _ = dec.decode(base)
    ms_base = dec.kernel_times()[0]
    assert np.array_equal(a, b), "the progressive file and its twin decode to different bytes"
    dec.close()
    dec = decoder(lib, False)
    host = prog.tobytes()

    def device_call(stream):
        def go():
            o = G.DecoderOutput()
            o.type, o.data = G.DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, out.data_ptr()
            assert lib.L.gpujpeg_decoder_decode(dec.h, stream.data_ptr(), stream.numel(), C.byref(o)) == 0
        return go

    points = {"prog": device_call(d_prog), "base": device_call(d_base), "prog2": device_call(d_prog),
              "pil": lambda: np.asarray(Image.open(io.BytesIO(host)))}
    for f in points.values():
        f()
    rounds = {k: [] for k in points}
    for _ in range(ROUNDS):
        for k, f in points.items():
            n = max(2, calls // 4) if k == "pil" else calls
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            torch.cuda.synchronize()
            rounds[k].append((time.perf_counter() - t0) / n * 1e3)
    dec.close()
    res = {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rounds.items()}
    return {"width": w, "height": h, "bytes_progressive": int(prog.size), "bytes_baseline": int(base.size), "scans": stats[2], "levels": stats[3],
            "segments": stats[4], "entropy_ms_progressive": float(ms_prog), "entropy_ms_baseline": float(ms_base), "points": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/progressive.json")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="640x368,1920x1080,3840x2160")
    a = ap.parse_args()
    lib = G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    results = [measure(lib, *[int(v) for v in s.split("x")], a.calls) for s in a.sizes.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "calls_per_round": a.calls, "rounds": ROUNDS, "quality": 75, "sampling": "4:2:0", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    lines = ["# Progressive decode against the baseline twin (tools/progressive_times.py)", "",
             f"{doc['device']}; libjpeg files at quality 75, 4:2:0; device buffers; ms per call, median of {ROUNDS} alternating rounds of {a.calls} calls [min - max].", "",
             "| size | bytes prog / base | scans / levels / waves | prog | base | prog2 | PIL on the host | entropy stage prog / base (ms) |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        p = r["points"]
        cell = lambda k: f"{p[k]['ms']:.3f} [{p[k]['min']:.3f} - {p[k]['max']:.3f}]"  # noqa: E731
        lines.append(f"| {r['width']}x{r['height']} | {r['bytes_progressive']} / {r['bytes_baseline']} | {r['scans']} / {r['levels']} / {r['segments']} | {cell('prog')} | "
                     f"{cell('base')} | {cell('prog2')} | {cell('pil')} | {r['entropy_ms_progressive']:.3f} / {r['entropy_ms_baseline']:.3f} |")
    with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
