#!/usr/bin/env python3
"""Batched reduced-size decode (dec_opt_scale together with gpujpeg_amd_decoder_decode_batch): frames per second against the alternatives, on the GPU.

Public API only. Workloads, 256 frames of one header each (a seeded photograph-like frame shifted per frame, q75, restart auto), streams and pixels
in device memory:

    hd       1920 x 1080, RGB 4:4:4, non-interleaved scans     (the token route: k_huffman_decode_tok + k_idct_tok_scaled_rgb444)
    4k       3840 x 2160, the same
    hd420    1920 x 1080, 4:2:0, one interleaved scan, decoded to packed RGB   (the plane route: k_huffman_decode_par + k_idct_scaled + k_postprocess)

at dec_opt_scale = 1/2, 1/4 and 1/8. The points of a table are measured in ALTERNATION (each round gives every point a slice of calls), wall clock
around calls that end in a synchronise:

    a        decode_batch with the scale
    b        the same call through --baseline-lib (a build of the commit before the batched reduced-size kernels: the loop of single calls inside
             the batch call); only when that library is given
    c        the full-size decode_batch of the same streams
    a2       a once more: the difference to a is the spread every other difference has to beat

    python tools/scaled_batch_times.py --out profiles/scaled_batch.json [--calls 20] [--baseline-lib PATH/libgpujpeg.so]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/scaled_batch_times.py --trace      (kernel names; hd and hd420 at 1/4, a few calls)

A "call" is one pass over the 256 frames; rates are frames per second."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime per process)

from gpujpeg_amd import libgpujpeg as G  # noqa: E402
from tools.region_batch_times import natural_frame  # noqa: E402

FRAMES = 256
WORKLOADS = (("hd", 1920, 1080, False), ("4k", 3840, 2160, False), ("hd420", 1920, 1080, True))
SCALES = (2, 4, 8)


def encode_frames(lib, w, h, il420, device):
    """FRAMES streams with one header in one device buffer -> (tensor, stride, sizes)"""
    base = natural_frame(w, h, 1, device)
    frames = torch.stack([torch.roll(base, (37 * f, 101 * f), (0, 1)) for f in range(FRAMES)]).contiguous()
    p = lib.default_parameters()
    p.quality, p.restart_interval, p.verbose = 75, G.RESTART_AUTO, -1
    if il420:
        p.interleaved = 1
        lib.L.gpujpeg_parameters_chroma_subsampling(C.byref(p), G.SUBSAMPLING_420)
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
    """one decoder at one scale; run(n) adds n passes over the frames to its time"""

    def __init__(self, name, lib, d_in, stride, sizes, w, h, s):
        self.name, self.lib, self.s = name, lib, s
        self.dec = G.Decoder(lib)
        assert self.dec.set_option("dec_opt_scale", "1" if s == 1 else "1/%d" % s) == 0
        self.d_in, self.stride, self.sizes = d_in, stride, sizes
        self.raw = -(-w // s) * -(-h // s) * 3
        self.d_out = torch.empty(self.raw * FRAMES, dtype=torch.uint8, device=d_in.device)
        self.wall_s, self.calls = 0.0, 0

    def call(self):
        self.dec.decode_batch(None, device_out=self.d_out.data_ptr(), out_stride=self.raw, device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)

    def run(self, n, timed=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.call()
        torch.cuda.synchronize()
        if timed:
            self.wall_s += time.perf_counter() - t0
            self.calls += n

    def result(self):
        return {"calls": self.calls, "ms_per_call": round(self.wall_s / self.calls * 1000.0, 4), "frames_per_s": round(FRAMES * self.calls / self.wall_s, 1),
                "last_batch": list(self.dec.last_batch())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="hd,4k,hd420")
    ap.add_argument("--baseline-lib", default=None, help="libgpujpeg.so of the commit to compare with: point b")
    ap.add_argument("--trace", action="store_true", help="hd and hd420 at 1/4, a few calls per point and no report: for a kernel trace")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    base = None
    if args.baseline_lib and not args.trace:
        base = G.Library(os.path.abspath(args.baseline_lib))
        assert base.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": FRAMES, "streams": "q75, restart auto; hd / 4k: RGB 4:4:4 non-interleaved, hd420: 4:2:0 interleaved", "calls_per_point": args.calls,
              "rounds": args.rounds, "baseline_lib": bool(base), "workloads": {}}
    for wname, w, h, il420 in WORKLOADS:
        if wname not in args.workloads.split(",") or (args.trace and wname == "4k"):
            continue
        d_in, stride, sizes = encode_frames(lib, w, h, il420, device)
        out = {"size": [w, h], "stream_bytes_mean": int(np.mean(sizes))}
        full = Point("c_full_size_decode_batch", lib, d_in, stride, sizes, w, h, 1)
        full.run(2 if args.trace else args.warmup, timed=False)
        for s in (4,) if args.trace else SCALES:
            pts = [Point("a_scaled_decode_batch", lib, d_in, stride, sizes, w, h, s)]
            if base:
                pts.append(Point("b_baseline_lib_scaled_decode_batch", base, d_in, stride, sizes, w, h, s))
            pts.append(Point("a2_scaled_decode_batch_again", lib, d_in, stride, sizes, w, h, s))
            for p in pts:
                p.run(2 if args.trace else args.warmup, timed=False)
            if not args.trace:
                full.wall_s, full.calls = 0.0, 0
                per = max(1, args.calls // args.rounds)
                for _ in range(args.rounds):
                    for p in pts + [full]:
                        p.run(per)
                out["scale_1_%d" % s] = {p.name: p.result() for p in pts + [full]}
                for k, v in out["scale_1_%d" % s].items():
                    print(wname, "1/%d" % s, k, json.dumps(v), flush=True)
            for p in pts:
                p.dec.close()
            del pts
        full.dec.close()
        report["workloads"][wname] = out
        del d_in, full
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
