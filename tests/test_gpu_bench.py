"""-m gpu: bench.py's plain run and --dump-outputs. The plain line carries the headline and nothing that takes runs of its own (those come with
--full); two runs with the same arguments write the same files (seeded inputs, whole turns of the frame rotation per step), within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "hd", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(gpu_lib, tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for d in (a, b):
        assert d["value"] > 0 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["config"]["frames_per_step_per_pipeline"] % 3 == 0
        assert not {"roofline", "workloads", "full_api", "cpu_baseline"} & set(d)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y), f"{n} differs between two runs with the same arguments"
        total += x.nbytes
    assert total <= 64 << 20
    load = lambda n: np.load(tmp_path / "a" / f"{n}.npy")  # noqa: E731
    sizes = load("jpeg_bytes")
    pipelines = a["config"]["streams_per_gpu"]
    assert sizes.shape == (pipelines,)
    for i in range(pipelines):  # an HD stream is written whole: a JPEG from SOI to EOI
        jpeg = load(f"jpeg_{i}")
        assert jpeg.size == sizes[i] and list(jpeg[:2]) == [0xFF, 0xD8] and list(jpeg[-2:]) == [0xFF, 0xD9]
        for k in range(3):  # every pipeline codes the same three frames
            assert np.array_equal(load(f"decoded_{i}_{k}"), load(f"decoded_0_{k}"))
    assert not np.array_equal(load("decoded_0_0"), load("decoded_0_1"))
