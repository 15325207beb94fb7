#!/usr/bin/env python3
"""Crop-and-resize with dec_opt_resize_filter=antialias against the same call with the default bilinear filter, on the GPU.

Public API only. The workloads, rectangles and output of tools/crop_resize_times.py -- 256 x HD and 256 x 4K frames of one header (q75, restart auto), one
RandomResizedCrop rectangle per frame (same seeds), 224 x 224 packed RGB, every other frame mirrored, device buffers -- once with 4:4:4 streams
(non-interleaved, as there) and once with 4:2:0 streams (interleaved), which dec_opt_resize_prescale leaves alone. Points, measured in ALTERNATION, wall
clock around calls that end in a synchronise, a point's figure the MEDIAN of its rounds:

    a        the call with the default filter (bilinear)
    f        the call with dec_opt_resize_filter=antialias
    a2       a once more: the difference to a is the spread every other difference has to beat

    python tools/crop_resize_antialias_times.py --out profiles/crop_resize_antialias.json [--calls 9] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/crop_resize_antialias_times.py --trace f [--sampling 420]   (kernel durations of ONE
                                                                                                     point; 256 x HD, three calls)
    python tools/crop_resize_antialias_times.py --lib OTHER/libgpujpeg.so --points a,a2    (another build of the library -- the parent commit's has no f)

A "call" is one pass over the 256 frames; rates are frames per second."""
import argparse
import ctypes as C
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
from region_batch_times import FRAMES, WORKLOADS, natural_frame  # noqa: E402


def encode_frames(lib, w, h, device, sampling):
    """FRAMES streams with one header in one device buffer -> (tensor, stride, sizes); sampling: "444" (non-interleaved) or "420" (interleaved)"""
    base = natural_frame(w, h, 1, device)
    frames = torch.stack([torch.roll(base, (37 * f, 101 * f), (0, 1)) for f in range(FRAMES)]).contiguous()
    p = lib.default_parameters()
    p.quality, p.restart_interval, p.verbose = 75, G.RESTART_AUTO, -1
    if sampling == "420":
        lib.L.gpujpeg_parameters_chroma_subsampling(C.byref(p), G.SUBSAMPLING_420)
        p.interleaved = 1
    pi = lib.default_image_parameters()
    pi.width, pi.height = w, h
    enc = G.Encoder(lib)
    ptrs, sizes = enc.encode_batch_noclone(p, pi, frames.data_ptr(), FRAMES, gpu=True)
    stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(stride * FRAMES, np.uint8)
    for f, (ptr, n) in enumerate(zip(ptrs, sizes)):
        host[f * stride:f * stride + n] = np.frombuffer((C.c_uint8 * n).from_address(ptr), np.uint8)
    enc.close()
    del frames
    return torch.from_numpy(host).to(device), stride, sizes


class Point:
    """one decoder with one filter; run(n) times n passes over the frames as one round"""

    def __init__(self, name, lib, d_in, stride, sizes, rects, mirror, filt):
        self.name, self.lib = name, lib
        self.dec = G.Decoder(lib)
        self.dec.set_output_format(1, 1)  # (packed RGB, whatever the stream's sampling)
        if filt:
            assert self.dec.set_option("dec_opt_resize_filter", filt) == 0
        self.d_in, self.stride, self.sizes, self.rects, self.mirror = d_in, stride, sizes, rects, mirror
        self.raw = OUT * OUT * 3
        self.d_out = torch.empty(self.raw * FRAMES, dtype=torch.uint8, device=d_in.device)
        self.rounds = []

    def call(self):
        self.dec.decode_batch_crop_resize(None, self.rects, OUT, OUT, mirror=self.mirror, device_out=self.d_out.data_ptr(), out_stride=self.raw,
                                          device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)

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
                "last_batch": list(self.dec.last_batch()), "region_stats": list(self.dec.region_stats())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=9, help="timed calls per point, spread over the rounds")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="hd,4k")
    ap.add_argument("--sampling", default="444,420")
    ap.add_argument("--points", default="a,f,a2")
    ap.add_argument("--trace", default=None, metavar="POINT", help="a or f: 256 x HD, three calls of that point alone and no report -- for a kernel trace")
    ap.add_argument("--lib", default=None, help="another build of the library (A/B runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library(args.lib)
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    which = [args.trace] if args.trace else args.points.split(",")
    filters = {"a": ("a_bilinear", None), "f": ("f_antialias", "antialias"), "a2": ("a2_bilinear_again", None)}
    report = {"frames": FRAMES, "output": [OUT, OUT], "calls_per_point": args.calls, "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(",") or (args.trace and wname != "hd"):
            continue
        for sampling in args.sampling.split(",")[:1 if args.trace else None]:
            d_in, stride, sizes = encode_frames(lib, w, h, device, sampling)
            rects = random_resized_crops(w, h, FRAMES, w + OUT)
            mirror = [f & 1 for f in range(FRAMES)]
            pts = [Point(filters[k][0], lib, d_in, stride, sizes, rects, mirror, filters[k][1]) for k in ("a", "f", "a2") if k in which]
            key = f"{wname}_{sampling}"
            out = {"size": [w, h], "sampling": sampling, "stream_bytes_mean": int(np.mean(sizes))}
            if args.trace:
                for p in pts:
                    p.run(3, timed=False)
            else:
                for p in pts:
                    p.run(args.warmup, timed=False)
                per = max(1, args.calls // args.rounds)
                for _ in range(args.rounds):
                    for p in pts:
                        p.run(per)
                out["points"] = {p.name: p.result() for p in pts}
                for k, v in out["points"].items():
                    print(key, k, json.dumps(v), flush=True)
            for p in pts:
                p.dec.close()
            del pts, d_in
            report["workloads"][key] = out
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
