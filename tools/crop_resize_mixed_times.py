#!/usr/bin/env python3
"""Crop-and-resize over streams of different image sizes (dec_opt_batch_sizes = mixed): frames per second against the alternatives, on the GPU.

Public API only. 256 streams of ONE family -- one encoder configuration (q75, non-interleaved 4:4:4) with an EXPLICIT restart interval, so that their
headers differ in SOF0's dimensions alone -- whose widths and heights are drawn independently and uniformly from 0.75 .. 1.25 of the workload's nominal
size (HD, 4K; fixed seed), rounded to even. One rectangle per frame drawn the way RandomResizedCrop draws it against that frame's own image
(tools/crop_resize_times.py), resampled to 224 x 224 packed RGB, every other frame mirrored. Streams and pixels are device buffers. The points are
measured in ALTERNATION (each round gives every point a slice of calls), wall clock around calls that end in a synchronise; the figure of a point
is the MEDIAN of its rounds:

    a        the "mixed" call on the 256 streams of different sizes
    b        the loop of single-frame crop-and-resize calls (a batch of one) on the same streams: the only way without the option
    c        the "same" call on 256 equal-size streams of the mean area, same content and rectangles drawn the same way
    d        the "mixed" call on c's streams: against c, the price of the per-frame geometry record and of reading the headers
    a2, c2   a and c once more: the differences to a and c are the spread every other difference has to beat

    python tools/crop_resize_mixed_times.py --out profiles/crop_resize_mixed.json [--calls 20] [--workloads hd,4k] [--restart 16]

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
from region_batch_times import FRAMES, WORKLOADS, natural_frame  # noqa: E402


def encode_family(lib, dims, restart, device):
    """one stream per (w, h) of dims, all from one encoder configuration, in one device buffer -> (tensor, stride, sizes)"""
    wmax, hmax = max(w for w, _ in dims), max(h for _, h in dims)
    base = natural_frame(wmax, hmax, 1, device)
    p = lib.default_parameters()
    p.quality, p.restart_interval, p.verbose = 75, restart, -1
    enc = G.Encoder(lib)
    streams = []
    for f, (w, h) in enumerate(dims):
        frame = torch.roll(base, (37 * f, 101 * f), (0, 1))[:h, :w].contiguous()
        pi = lib.default_image_parameters()
        pi.width, pi.height = w, h
        streams.append(enc.encode(p, pi, frame.data_ptr(), gpu=True))
    enc.close()
    sizes = [int(s.size) for s in streams]
    stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(stride * len(streams), np.uint8)
    for f, s in enumerate(streams):
        host[f * stride:f * stride + s.size] = s
    return torch.from_numpy(host).to(device), stride, sizes


class Point:
    """one decoder and one way to get the frames; run(n) times n passes over the frames as one round"""

    def __init__(self, name, kind, lib, d_in, stride, sizes, rects, mirror, mixed):
        self.name, self.kind = name, kind
        self.dec = G.Decoder(lib)
        assert self.dec.set_option(G.DEC_OPT_BATCH_SIZES, G.BATCH_SIZES_MIXED if mixed else G.BATCH_SIZES_SAME) == 0
        self.d_in, self.stride, self.sizes, self.rects, self.mirror = d_in, stride, sizes, rects, mirror
        self.raw = OUT * OUT * 3
        self.d_out = torch.empty(self.raw * FRAMES, dtype=torch.uint8, device=d_in.device)
        self.rounds = []

    def call(self):
        if self.kind == "b":
            for f, r in enumerate(self.rects):
                self.dec.decode_batch_crop_resize(None, [r], OUT, OUT, mirror=[self.mirror[f]], device_out=self.d_out.data_ptr() + f * self.raw, out_stride=self.raw,
                                                  device_in=self.d_in.data_ptr() + f * self.stride, in_stride=self.stride, sizes=self.sizes[f:f + 1])
        else:
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
        r = {"rounds_ms_per_call": [round(t, 4) for t in ms], "median_ms_per_call": round(med, 4), "frames_per_s": round(FRAMES / med * 1000.0, 1)}
        if self.kind != "b":
            r["last_batch"] = list(self.dec.last_batch())
        return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="hd")
    ap.add_argument("--restart", type=int, default=16, help="the explicit restart interval of every stream, in MCUs (RESTART_AUTO depends on the image size)")
    ap.add_argument("--check", action="store_true", help="compare a's frames with b's once, byte for byte, before the rounds")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": FRAMES, "streams": "RGB 4:4:4 q75 non-interleaved, restart interval %d" % args.restart, "output": [OUT, OUT], "calls_per_point": args.calls,
              "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(","):
            continue
        rng = np.random.default_rng(w + h)
        dims = [(int(rng.uniform(0.75, 1.25) * w) & ~1, int(rng.uniform(0.75, 1.25) * h) & ~1) for _ in range(FRAMES)]
        area = float(np.mean([a * b for a, b in dims]))
        we = int(round((area * w / h) ** 0.5)) & ~1
        he = int(round(area / we)) & ~1
        mirror = [f & 1 for f in range(FRAMES)]
        rects = [random_resized_crops(a, b, 1, w + OUT + f)[0] for f, (a, b) in enumerate(dims)]
        eq_rects = random_resized_crops(we, he, FRAMES, w + OUT)
        d_mix, s_mix, z_mix = encode_family(lib, dims, args.restart, device)
        d_eq, s_eq, z_eq = encode_family(lib, [(we, he)] * FRAMES, args.restart, device)
        mk = lambda name, kind, mixed, eq=False: Point(name, kind, lib, d_eq if eq else d_mix, s_eq if eq else s_mix, z_eq if eq else z_mix,  # noqa: E731
                                                       eq_rects if eq else rects, mirror, mixed)
        pts = [mk("a_mixed_call", "a", True), mk("b_single_frame_calls", "b", True), mk("c_same_call_equal_sizes", "c", False, True),
               mk("d_mixed_call_equal_sizes", "d", True, True), mk("a2_mixed_call_again", "a", True), mk("c2_same_call_again", "c", False, True)]
        out = {"nominal": [w, h], "sizes_min_max": [[min(a for a, _ in dims), min(b for _, b in dims)], [max(a for a, _ in dims), max(b for _, b in dims)]],
               "distinct_sizes": len(set(dims)), "equal_size": [we, he], "stream_bytes_mean": int(np.mean(z_mix)), "stream_bytes_mean_equal": int(np.mean(z_eq))}
        for p in pts:
            p.run(args.warmup, timed=False)
        if args.check:
            torch.cuda.synchronize()
            out["a_equals_b"] = bool(torch.equal(pts[0].d_out, pts[1].d_out))
            print(wname, "a_equals_b", out["a_equals_b"], flush=True)
        per = max(1, args.calls // args.rounds)
        for _ in range(args.rounds):
            for p in pts:
                p.run(per if p.kind != "b" else max(1, per // 4))  # (the loop of single calls takes tens of ms a pass)
        out["points"] = {p.name: p.result() for p in pts}
        for k, v in out["points"].items():
            print(wname, k, json.dumps(v), flush=True)
        for p in pts:
            p.dec.close()
        del pts, d_mix, d_eq
        report["workloads"][wname] = out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
