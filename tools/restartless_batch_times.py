#!/usr/bin/env python3
"""Crop-and-resize over streams WITHOUT restart markers (dec_opt_batch_restartless): frames per second with the option on and off, on the GPU.

Public API only. 256 interleaved 4:2:0 streams at q75 of ONE family whose widths and heights are drawn independently and uniformly from 0.75 .. 1.25 of
the workload's nominal size (HD, 4K; fixed seed), rounded to even -- once with restart interval 0 (what libjpeg, PIL and OpenCV write) and once, the
same images, with an explicit restart interval. Both go through the mixed-size call (dec_opt_batch_sizes = mixed). Two kinds of rectangle per frame,
resampled to 224 x 224 packed RGB: drawn the way RandomResizedCrop draws them against the frame's own image (tools/crop_resize_times.py), and fixed
224 x 224 crops at random origins. Streams and pixels are device buffers. The points are measured in ALTERNATION (each round gives every point a
slice of calls), wall clock around calls that end in a synchronise; the figure of a point is the MEDIAN of its rounds, the spread their minimum and
maximum:

    on          restart-less streams, option on: the batched launches, scans left behind the cover
    off         restart-less streams, option off: every frame through the single-frame route inside the call (the only route before the option).
                Its streams are handed over in HOST memory (one packed buffer, copied by the call): the single-frame route launches a device-resident
                stream on the previous frame's header before it has read the stream's own, and refuses a rectangle that does not fit THAT image --
                which streams of different sizes run into. The copies are a few per cent of this point's time.
    on_to_end   as `on` with the developer setting GJ_DEC_NO_EARLY_STOP=1: every scan decoded to its end (what the early stop is worth)
    ri_off      the same images with a restart interval, option off: the batch as it was -- the ceiling
    ri_on       the same, option on: must be within the spread of ri_off

    python tools/restartless_batch_times.py --out profiles/restartless_batch.json [--calls 10] [--workloads hd,4k] [--restart 16]

A "call" is one pass over the 256 frames; rates are frames per second. `entropy_bytes` is gpujpeg_amd_decoder_get_entropy_bytes of the last call."""
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


def encode_family(lib, dims, restart, device):
    """one interleaved 4:2:0 stream per (w, h) of dims, all from one encoder configuration, in one device buffer -> (tensor, stride, sizes)"""
    wmax, hmax = max(w for w, _ in dims), max(h for _, h in dims)
    base = natural_frame(wmax, hmax, 1, device)
    p = lib.default_parameters()
    p.quality, p.restart_interval, p.verbose, p.interleaved = 75, restart, -1, 1
    lib.L.gpujpeg_parameters_chroma_subsampling(C.byref(p), G.SUBSAMPLING_420)
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
    return torch.from_numpy(host).to(device), stride, sizes, host


class Point:
    """one decoder and one set of streams and rectangles; run(n) times n passes over the frames as one round"""

    def __init__(self, name, lib, family, rects, on, to_end=False, host=False):
        self.name, self.lib, self.host = name, lib, host
        if to_end:
            assert lib.tuning("GJ_DEC_NO_EARLY_STOP=1")
        self.dec = G.Decoder(lib)
        if to_end:
            lib.tuning(None)
        assert self.dec.set_option(G.DEC_OPT_BATCH_SIZES, G.BATCH_SIZES_MIXED) == 0
        assert self.dec.set_option(G.DEC_OPT_BATCH_RESTARTLESS, G.BATCH_RESTARTLESS_ON if on else G.BATCH_RESTARTLESS_OFF) == 0
        self.d_in, self.stride, self.sizes, self.h_in = family
        self.rects = rects
        self.raw = OUT * OUT * 3
        self.d_out = torch.empty(self.raw * FRAMES, dtype=torch.uint8, device=self.d_in.device)
        self.rounds = []

    def call(self):
        if self.host:  # (the C call itself: the packed host buffer as it is)
            n = len(self.sizes)
            csz = (C.c_size_t * n)(*self.sizes)
            rc4 = (C.c_int * (4 * n))(*[int(v) for r in self.rects for v in r])
            pi = G.ImageParameters()
            rc = self.lib.L.gpujpeg_amd_decoder_decode_batch_crop_resize(self.dec.h, self.h_in.ctypes.data, self.stride, csz, n, rc4, None, OUT, OUT,
                                                                          self.d_out.data_ptr(), self.raw, C.byref(pi))
            assert rc == 0, rc
            return
        self.dec.decode_batch_crop_resize(None, self.rects, OUT, OUT, device_out=self.d_out.data_ptr(), out_stride=self.raw, device_in=self.d_in.data_ptr(),
                                          in_stride=self.stride, sizes=self.sizes)

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
        rc, handed, read = self.dec.entropy_bytes()
        return {"rounds_ms_per_call": [round(t, 3) for t in ms], "median_ms_per_call": round(med, 3), "frames_per_s": round(FRAMES / med * 1000.0, 1),
                "frames_per_s_min_max": [round(FRAMES / max(ms) * 1000.0, 1), round(FRAMES / min(ms) * 1000.0, 1)], "last_batch": list(self.dec.last_batch()),
                "entropy_bytes": [handed, read] if rc == 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="hd")
    ap.add_argument("--restart", type=int, default=16, help="the explicit restart interval of the ceiling's streams, in MCUs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": FRAMES, "streams": "4:2:0 q75 interleaved, restart interval 0 / %d" % args.restart, "output": [OUT, OUT], "calls_per_point": args.calls,
              "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(","):
            continue
        rng = np.random.default_rng(w + h)
        dims = [(int(rng.uniform(0.75, 1.25) * w) & ~1, int(rng.uniform(0.75, 1.25) * h) & ~1) for _ in range(FRAMES)]
        fam0 = encode_family(lib, dims, 0, device)
        fam1 = encode_family(lib, dims, args.restart, device)
        out = {"nominal": [w, h], "stream_bytes_mean": [int(np.mean(fam0[2])), int(np.mean(fam1[2]))], "rectangles": {}}
        org = np.random.default_rng(w + OUT + 1)
        kinds = {"random_resized_crop": [random_resized_crops(a, b, 1, w + OUT + f)[0] for f, (a, b) in enumerate(dims)],
                 "fixed_224": [(int(org.integers(0, a - OUT + 1)), int(org.integers(0, b - OUT + 1)), OUT, OUT) for a, b in dims]}
        for kname, rects in kinds.items():
            pts = [Point("on", lib, fam0, rects, True), Point("off", lib, fam0, rects, False, host=True), Point("on_to_end", lib, fam0, rects, True, to_end=True),
                   Point("ri_off", lib, fam1, rects, False), Point("ri_on", lib, fam1, rects, True)]
            for p in pts:
                p.run(1 if p.name == "off" else args.warmup, timed=False)
            torch.cuda.synchronize()
            same = bool(torch.equal(pts[0].d_out, pts[1].d_out) and torch.equal(pts[0].d_out, pts[2].d_out))
            per = max(1, args.calls // args.rounds)
            for _ in range(args.rounds):
                for p in pts:
                    p.run(1 if p.name == "off" else per)  # (the single-frame route takes milliseconds per frame)
            res = {p.name: p.result() for p in pts}
            res["on_equals_off_equals_to_end"] = same
            for k, v in res.items():
                print(wname, kname, k, json.dumps(v), flush=True)
            out["rectangles"][kname] = res
            for p in pts:
                p.dec.close()
            del pts
        report["workloads"][wname] = out
        del fam0, fam1
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
