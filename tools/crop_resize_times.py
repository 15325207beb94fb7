#!/usr/bin/env python3
"""Batched crop-and-resize (gpujpeg_amd_decoder_decode_batch_crop_resize): frames per second against the alternatives, on the GPU.

Public API only. Workloads: 256 x HD and 256 x 4K frames of one header (a seeded photograph-like frame shifted per frame; q75, non-interleaved
4:4:4, restart auto), one rectangle per frame drawn the way RandomResizedCrop draws it -- area 8 .. 100 % of the image, aspect 3/4 .. 4/3
(log-uniform), ten tries, then the centre crop; fixed seed -- and resampled to 224 x 224 packed RGB, every other frame mirrored. Streams and pixels are
device buffers. The points are measured in ALTERNATION (each round gives every point a slice of calls), wall clock around calls that end in a
synchronise; the figure of a point is the MEDIAN of its rounds:

    a        the crop-and-resize call
    b        a loop of set_option(dec_opt_region) + gpujpeg_decoder_decode over the same rectangles: the only way before this call existed; the
             resize the caller would still have to launch per image is NOT counted, which favours the loop
    c        gpujpeg_amd_decoder_decode_batch_regions with 224 x 224 crops of the same streams: the fixed-size ceiling
    d        the crop-and-resize call with every rectangle 224 x 224 (c's rectangles): against c, the resample stage, the plane route and per-frame covers
    e        a with dec_opt_resize_prescale=1/8: the reduced-size IDCT ahead of the resample wherever the rectangle is at least twice the output
             (the share of frames per scale that the seed draws is in the report: scale_share)
    f        e with dec_opt_resize_prescale_subsampled=on: on 4:2:0 streams (--sampling 420) the prescale per component; on 4:4:4 streams it is e
    g        a with dec_opt_resize_filter=antialias, for reference
    a2       a once more: the difference to a is the spread every other difference has to beat
             (--sampling 420: e is a as well -- the prescale leaves 4:2:0 streams alone without f's option --, so a, e and a2 are three repeats of today's call)

    python tools/crop_resize_times.py --out profiles/crop_resize.json [--calls 20]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/crop_resize_times.py --trace a      (kernel durations of ONE point; 256 x HD, a few calls)
    python tools/crop_resize_times.py --sampling 420 --points a,e,f,g,a2 --out profiles/crop_resize_420.json      (interleaved 4:2:0 streams)
    python tools/crop_resize_times.py --lib OTHER/libgpujpeg.so --points a,a2 --workloads hd          (another build of the library, some points: A/B runs
                                                                                                     alternate two such processes)

A "call" is one pass over the 256 frames; rates are frames per second."""
import argparse
import ctypes as C
import json
import math
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
from region_batch_times import FRAMES, WORKLOADS, encode_frames  # noqa: E402

OUT = 224


def random_resized_crops(w, h, n, seed, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """n rectangles (x, y, w, h) as torchvision's RandomResizedCrop.get_params draws them, from a seeded numpy generator"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        for _ in range(10):
            area = w * h * rng.uniform(scale[0], scale[1])
            aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
            cw, ch = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < cw <= w and 0 < ch <= h:
                out.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
                break
        else:  # the centre crop of the closest legal aspect
            in_ratio = w / h
            cw, ch = (w, int(round(w / ratio[0]))) if in_ratio < ratio[0] else (int(round(h * ratio[1])), h) if in_ratio > ratio[1] else (w, h)
            out.append(((w - cw) // 2, (h - ch) // 2, cw, ch))
    return out


class Point:
    """one decoder and one way to get the frames; run(n) times n passes over the frames as one round"""

    def __init__(self, name, kind, lib, d_in, stride, sizes, rects, mirror, prescale=None, options=()):
        self.name, self.kind, self.lib = name, kind, lib
        self.dec = G.Decoder(lib)
        if prescale:
            assert self.dec.set_option("dec_opt_resize_prescale", prescale) == 0
        for opt, val in options:
            assert self.dec.set_option(opt, val) == 0, (opt, val)
        self.d_in, self.stride, self.sizes = d_in, stride, sizes
        self.rects, self.mirror = rects, mirror
        self.raw = OUT * OUT * 3
        room = max(r[2] * r[3] for r in rects) * 3 if kind == "b" else self.raw * FRAMES
        self.d_out = torch.empty(room, dtype=torch.uint8, device=d_in.device)
        self.out = G.DecoderOutput()
        self.rounds = []

    def call(self):
        if self.kind == "b":
            o = self.out
            for f, r in enumerate(self.rects):
                assert self.dec.set_option("dec_opt_region", "%d,%d,%d,%d" % r) == 0
                o.type, o.data = G.DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, self.d_out.data_ptr()
                assert self.lib.L.gpujpeg_decoder_decode(self.dec.h, self.d_in.data_ptr() + f * self.stride, self.sizes[f], C.byref(o)) == 0
        elif self.kind == "c":
            self.dec.decode_batch_regions(None, [r[:2] for r in self.rects], OUT, OUT, device_out=self.d_out.data_ptr(), out_stride=self.raw,
                                          device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)
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
            r["region_stats"] = list(self.dec.region_stats())
        if self.kind in ("e", "f"):
            r["idct_side"] = self.dec.idct_path()
            r["prescaled_frames"] = sum(1 for s in self.dec.prescales() if s > 1)
        return r


def points_for(lib, d_in, stride, sizes, w, h, seed, which):
    rects = random_resized_crops(w, h, FRAMES, seed)
    rng = np.random.default_rng(seed + 1)
    fixed = [(int(rng.integers(0, w - OUT + 1)), int(rng.integers(0, h - OUT + 1)), OUT, OUT) for _ in range(FRAMES)]
    mirror = [f & 1 for f in range(FRAMES)]
    mk = lambda name, kind, rc, mir, pre=None, opts=(): Point(name, kind, lib, d_in, stride, sizes, rc, mir, pre, opts)  # noqa: E731
    makers = {"a": lambda: mk("a_crop_resize", "a", rects, mirror), "b": lambda: mk("b_single_region_calls", "b", rects, None),
              "c": lambda: mk("c_batch_regions_224", "c", fixed, None), "d": lambda: mk("d_crop_resize_224_rectangles", "d", fixed, None),
              "e": lambda: mk("e_crop_resize_prescale_8", "e", rects, mirror, "1/8"), "a2": lambda: mk("a2_crop_resize_again", "a", rects, mirror),
              "f": lambda: mk("f_crop_resize_prescale_8_subsampled", "f", rects, mirror, "1/8", (("dec_opt_resize_prescale_subsampled", "on"),)),
              "g": lambda: mk("g_crop_resize_antialias", "g", rects, mirror, None, (("dec_opt_resize_filter", "antialias"),))}
    return [makers[k]() for k in ("a", "b", "c", "d", "e", "f", "g", "a2") if k in which], rects


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="hd,4k")
    ap.add_argument("--trace", default=None, metavar="POINT", help="a, b, c, d, e, f or g: 256 x HD, a few calls of that point alone and no report -- for a kernel trace")
    ap.add_argument("--points", default="a,b,c,d,e,a2", help="the points to measure (a library without dec_opt_resize_prescale: leave e out)")
    ap.add_argument("--sampling", default="444", choices=["444", "420"], help="the streams: non-interleaved 4:4:4, or interleaved 4:2:0")
    ap.add_argument("--lib", default=None, help="another build of the library (A/B runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library(args.lib)
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": FRAMES, "streams": "RGB 4:4:4 q75 non-interleaved, restart auto" if args.sampling == "444" else "RGB 4:2:0 q75 interleaved, restart auto", "output": [OUT, OUT], "calls_per_point": args.calls,
              "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(",") or (args.trace and wname != "hd"):
            continue
        d_in, stride, sizes = encode_frames(lib, w, h, device, args.sampling)
        pts, rects = points_for(lib, d_in, stride, sizes, w, h, w + OUT, [args.trace] if args.trace else args.points.split(","))
        out = {"size": [w, h], "stream_bytes_mean": int(np.mean(sizes)), "rectangle_area_share_mean": round(float(np.mean([r[2] * r[3] for r in rects])) / (w * h), 4)}
        if hasattr(lib.L, "gpujpeg_amd_host_crop_resize_plan"):  # (frames per scale that dec_opt_resize_prescale=1/8 gives these rectangles)
            scales = [G.crop_resize_plan(lib, w, h, True, r, OUT, OUT, 8)[0] for r in rects]
            out["scale_share"] = {str(s): round(scales.count(s) / len(scales), 4) for s in (1, 2, 4, 8)}
        if args.trace:
            for p in pts:
                p.run(3, timed=False)
        else:
            print(wname, "scale_share", json.dumps(out.get("scale_share")), flush=True)
            for p in pts:
                p.run(args.warmup, timed=False)
            per = max(1, args.calls // args.rounds)
            for _ in range(args.rounds):
                for p in pts:
                    p.run(per if p.kind != "b" else max(1, per // 4))  # (the loop of single calls takes 20 .. 40 ms a pass)
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
