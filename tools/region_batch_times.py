#!/usr/bin/env python3
"""Batched region decode (gpujpeg_amd_decoder_decode_batch_regions): crops per second against today's alternatives, on the GPU.

Public API only. Workloads: 256 x HD and 256 x 4K frames of one header (a seeded photograph-like frame shifted per frame; q75, non-interleaved
4:4:4, restart auto), one crop per frame -- 224 x 224 and 512 x 512 at seeded uniformly random origins. Streams and pixels are device buffers.
The points of a table are measured in ALTERNATION (each round gives every point a slice of calls), wall clock around calls that end in a
synchronise:

    a        the batch of regions
    b        a loop of set_option(dec_opt_region) + gpujpeg_decoder_decode over the same rectangles: the only way before this call existed
    c        the full-frame gpujpeg_amd_decoder_decode_batch: what a caller decodes before it crops
    d        the batch of regions with every origin equal: against a, the price of per-frame covers and of the padded selection
    a2       a once more: the difference to a is the spread every other difference has to beat

    python tools/region_batch_times.py --out profiles/region_batch.json [--calls 20]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/region_batch_times.py --trace      (kernel names; 256 x HD, 224 x 224, a few calls)

A "call" is one pass over the 256 frames; rates are crops (= frames) per second."""
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

FRAMES = 256
WORKLOADS = (("hd", 1920, 1080), ("4k", 3840, 2160))
CROPS = (224, 512)


def natural_frame(w, h, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    yy = torch.arange(h, device=device, dtype=torch.float32).view(-1, 1)
    xx = torch.arange(w, device=device, dtype=torch.float32).view(1, -1)
    chans = []
    for k, (fx, fy, ph) in enumerate([(1 / 97.0, 1 / 61.0, 0.3), (1 / 53.0, 1 / 131.0, 1.1), (1 / 211.0, 1 / 89.0, 2.0)]):
        base = 128 + 70 * torch.sin(xx * fx + ph) * torch.cos(yy * fy) + 30 * torch.sin((xx + yy) * fx * 3.1 + k)
        tex = 12 * torch.sin(xx * 0.9 + yy * 0.35 + k) * torch.sin(yy * 0.7 - xx * 0.11)
        nz = 3.0 * torch.randn((h, w), device=device, generator=g)
        chans.append((base + tex + nz).clamp(0, 255).to(torch.uint8))
    return torch.stack(chans, -1).contiguous()


def encode_frames(lib, w, h, device, sampling="444"):
    """FRAMES streams with one header in one device buffer -> (tensor, stride, sizes); sampling "420": interleaved 4:2:0 streams, what photographs are"""
    base = natural_frame(w, h, 1, device)
    frames = torch.stack([torch.roll(base, (37 * f, 101 * f), (0, 1)) for f in range(FRAMES)]).contiguous()
    p = lib.default_parameters()
    p.quality, p.restart_interval, p.verbose = 75, G.RESTART_AUTO, -1
    if sampling == "420":
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
    """one decoder and one way to get the crops; run(n) adds n passes over the frames to its time"""

    def __init__(self, name, kind, lib, d_in, stride, sizes, w, h, crop, origins):
        self.name, self.kind, self.lib = name, kind, lib
        self.dec = G.Decoder(lib)
        self.d_in, self.stride, self.sizes = d_in, stride, sizes
        self.crop, self.origins = crop, origins
        self.raw = (w * h if kind == "c" else crop * crop) * 3
        self.d_out = torch.empty(self.raw * FRAMES, dtype=torch.uint8, device=d_in.device)
        self.out = G.DecoderOutput()
        self.wall_s, self.calls = 0.0, 0

    def call(self):
        if self.kind == "c":
            self.dec.decode_batch(None, device_out=self.d_out.data_ptr(), out_stride=self.raw, device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)
        elif self.kind == "b":
            o = self.out
            for f, (x, y) in enumerate(self.origins):
                assert self.dec.set_option("dec_opt_region", "%d,%d,%d,%d" % (x, y, self.crop, self.crop)) == 0
                o.type, o.data = G.DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, self.d_out.data_ptr() + f * self.raw
                assert self.lib.L.gpujpeg_decoder_decode(self.dec.h, self.d_in.data_ptr() + f * self.stride, self.sizes[f], C.byref(o)) == 0
        else:
            self.dec.decode_batch_regions(None, self.origins, self.crop, self.crop, device_out=self.d_out.data_ptr(), out_stride=self.raw,
                                          device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)

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
        r = {"calls": self.calls, "ms_per_call": round(self.wall_s / self.calls * 1000.0, 4), "crops_per_s": round(FRAMES * self.calls / self.wall_s, 1)}
        if self.kind != "b":
            r["last_batch"] = list(self.dec.last_batch())
        if self.kind in ("a", "d"):
            r["region_stats"] = list(self.dec.region_stats())
        return r


def points_for(lib, d_in, stride, sizes, w, h, crop, seed):
    rng = np.random.default_rng(seed)
    origins = [(int(rng.integers(0, w - crop + 1)), int(rng.integers(0, h - crop + 1))) for _ in range(FRAMES)]
    same = [origins[0]] * FRAMES
    mk = lambda name, kind, org: Point(name, kind, lib, d_in, stride, sizes, w, h, crop, org)  # noqa: E731
    return [mk("a_batch_regions", "a", origins), mk("b_single_region_calls", "b", origins), mk("c_full_decode_batch", "c", origins),
            mk("d_batch_regions_equal_origins", "d", same), mk("a2_batch_regions_again", "a", origins)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="hd,4k")
    ap.add_argument("--trace", action="store_true", help="256 x HD, 224 x 224, a few calls per point and no report: for a kernel trace")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": FRAMES, "streams": "RGB 4:4:4 q75 non-interleaved, restart auto", "calls_per_point": args.calls, "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(",") or (args.trace and wname != "hd"):
            continue
        d_in, stride, sizes = encode_frames(lib, w, h, device)
        out = {"size": [w, h], "stream_bytes_mean": int(np.mean(sizes))}
        for crop in CROPS[:1] if args.trace else CROPS:
            pts = points_for(lib, d_in, stride, sizes, w, h, crop, seed=w + crop)
            for p in pts:
                p.run(2 if args.trace else args.warmup, timed=False)
            if not args.trace:
                per = max(1, args.calls // args.rounds)
                for _ in range(args.rounds):
                    for p in pts:
                        p.run(per)
                out[f"crop_{crop}"] = {p.name: p.result() for p in pts}
                for k, v in out[f"crop_{crop}"].items():
                    print(wname, crop, k, json.dumps(v), flush=True)
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
