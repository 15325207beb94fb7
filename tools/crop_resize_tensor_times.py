#!/usr/bin/env python3
"""Crop-and-resize with tensor output (gpujpeg_amd_decoder_decode_batch_crop_resize_tensor): frames per second against the u8 call followed by the
pass every caller otherwise writes, on the GPU.

Public API only. Workloads as in tools/crop_resize_times.py: 256 x HD and 256 x 4K frames of one header, one RandomResizedCrop rectangle per frame
(fixed seed) resampled to 224 x 224, every other frame mirrored; streams and results are device buffers. Element types and layouts: F16 / CHW and
F32 / CHW, the ImageNet recipe (scale = 1 / (255 std), bias = -mean / std). The points are measured in ALTERNATION -- each round gives every point a
slice of calls --, wall clock around calls that end in a synchronise; a point's figure is the MEDIAN of its rounds, and all rounds are in the report:

    a            the u8 call alone (packed RGB bytes): what the tensor call adds to is seen against it
    b_<dtype>    the u8 call followed by the torch pass that makes the same tensor from its bytes:
                     x = u8.view(n, 224, 224, 3).permute(0, 3, 1, 2).to(dtype, memory_format=torch.contiguous_format); x.mul_(scale).add_(bias)
                 -- permute, to(dtype), mul, add in the cheapest form that leaves the same contiguous CHW tensor: one converting copy into a tensor
                 allocated once, outside the timing, and two in-place element-wise kernels. What a caller writes costs this or more.
    c_<dtype>    the tensor call
    a2           a once more: the difference to a is the spread every other difference has to beat

    python tools/crop_resize_tensor_times.py --out profiles/crop_resize_tensor.json [--calls 15] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/crop_resize_tensor_times.py --trace      (256 x HD, a few calls of a and of
                                                                                     both c points: the durations of the two resampling kernels)

A "call" is one pass over the 256 frames; rates are frames per second."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (before the library: one HIP runtime per process)

from gpujpeg_amd import libgpujpeg as G  # noqa: E402
from crop_resize_times import OUT, random_resized_crops  # noqa: E402
from region_batch_times import FRAMES, WORKLOADS, encode_frames  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE, BIAS = [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)]
DTYPES = {"f16": (G.TENSOR_F16, torch.float16), "f32": (G.TENSOR_F32, torch.float32)}


class Point:
    """one decoder and one way to get the tensors; run(n) times n passes over the frames as one round"""

    def __init__(self, name, kind, lib, d_in, stride, sizes, rects, mirror, dtype=None):
        self.name, self.kind = name, kind
        self.dec = G.Decoder(lib)
        self.d_in, self.stride, self.sizes, self.rects, self.mirror = d_in, stride, sizes, rects, mirror
        self.raw = OUT * OUT * 3
        self.rounds = []
        if kind != "c":
            self.u8 = torch.empty(self.raw * FRAMES, dtype=torch.uint8, device=d_in.device)
        if kind != "a":
            self.code, tdtype = DTYPES[dtype]
            self.x = torch.empty((FRAMES, 3, OUT, OUT), dtype=tdtype, device=d_in.device)
            self.scale = torch.tensor(SCALE, dtype=tdtype, device=d_in.device).view(1, 3, 1, 1)
            self.bias = torch.tensor(BIAS, dtype=tdtype, device=d_in.device).view(1, 3, 1, 1)

    def call(self):
        if self.kind == "c":
            self.dec.decode_batch_crop_resize_tensor(None, self.rects, OUT, OUT, self.code, G.TENSOR_CHW, SCALE, BIAS, mirror=self.mirror, out=self.x,
                                                     device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)
            return
        self.dec.decode_batch_crop_resize(None, self.rects, OUT, OUT, mirror=self.mirror, device_out=self.u8.data_ptr(), out_stride=self.raw,
                                          device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)
        if self.kind == "b":  # (the call has waited for the decoder's stream; the pass runs on torch's)
            self.x.copy_(self.u8.view(FRAMES, OUT, OUT, 3).permute(0, 3, 1, 2))  # = .to(dtype, memory_format=contiguous_format) into the tensor kept
            self.x.mul_(self.scale).add_(self.bias)

    def run(self, n, timed=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.call()
        torch.cuda.synchronize()
        if timed:
            self.rounds.append((time.perf_counter() - t0) / n)

    def result(self):
        ms = [t * 1000.0 for t in self.rounds]
        med = statistics.median(ms)
        return {"rounds_ms_per_call": [round(t, 4) for t in ms], "median_ms_per_call": round(med, 4), "frames_per_s": round(FRAMES / med * 1000.0, 1),
                "last_batch": list(self.dec.last_batch())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="hd,4k")
    ap.add_argument("--trace", action="store_true", help="256 x HD, a few calls of a and of the c points and no report -- for a kernel trace")
    ap.add_argument("--lib", default=None, help="another build of the library")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library(args.lib)
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": FRAMES, "streams": "RGB 4:4:4 q75 non-interleaved, restart auto", "output": [OUT, OUT], "layout": "CHW", "calls_per_point": args.calls,
              "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(",") or (args.trace and wname != "hd"):
            continue
        d_in, stride, sizes = encode_frames(lib, w, h, device)
        rects = random_resized_crops(w, h, FRAMES, w + OUT)
        mirror = [f & 1 for f in range(FRAMES)]
        mk = lambda name, kind, dtype=None: Point(name, kind, lib, d_in, stride, sizes, rects, mirror, dtype)  # noqa: E731
        pts = [mk("a_u8_call", "a")]
        for d in DTYPES:
            if not args.trace:
                pts.append(mk(f"b_u8_call_then_torch_{d}", "b", d))
            pts.append(mk(f"c_tensor_call_{d}", "c", d))
        if not args.trace:
            pts.append(mk("a2_u8_call_again", "a"))
        out = {"size": [w, h], "stream_bytes_mean": int(np.mean(sizes))}
        if args.trace:
            for p in pts:
                p.run(3, timed=False)
        else:
            for p in pts:
                p.run(args.warmup, timed=False)
            # the two ways make the same tensor, up to the pass's own rounding (it multiplies and adds in the tensor's type)
            by = {p.name: p for p in pts}
            for d in DTYPES:
                diff = (by[f"b_u8_call_then_torch_{d}"].x.float() - by[f"c_tensor_call_{d}"].x.float()).abs().max().item()
                out[f"max_abs_difference_b_c_{d}"] = diff
                print(wname, d, "largest |b - c| =", diff, flush=True)
            per = max(1, args.calls // args.rounds)
            for _ in range(args.rounds):
                for p in pts:
                    p.run(per)
            out["points"] = {p.name: p.result() for p in pts}
            for k, v in out["points"].items():
                print(wname, k, json.dumps(v), flush=True)
        for p in pts:
            p.dec.close()
        del pts
        report["workloads"][wname] = out
        del d_in
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
