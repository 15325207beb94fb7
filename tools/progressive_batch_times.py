#!/usr/bin/env python3
"""Progressive files through the batch call (dec_opt_batch_progressive): frames per second with the option on and off, on the GPU.

Public API only. The streams are what a folder of web pictures holds: N different pictures of ONE size saved by libjpeg (through PIL) at quality 75,
4:2:0, progressive=True -- ten scans, optimised Huffman tables of their own, no restart markers -- and, the same pictures, saved as baseline files
(optimize=False): the twins, which share one header. Streams and pixels are device buffers; the call is gpujpeg_amd_decoder_decode_batch to packed RGB.
The points are measured in ALTERNATION (each round gives every point a slice of calls), wall clock around calls that end in a synchronise; the figure
of a point is the MEDIAN of its rounds, the spread their minimum and maximum:

    off         progressive files, dec_opt_progressive = on, dec_opt_batch_progressive = off: every frame through the single-frame route inside the
                call (the only route before the option; one call per round: it takes seconds)
    on          the same, dec_opt_batch_progressive = on: frame 0 ahead (single), the others as one group through the batched launches
    twins       the baseline saves through the same call with dec_opt_batch_restartless = on: what the same pictures cost as baseline files
    host_parse  NOT a decode: gpujpeg_amd_host_stream_info over the N progressive files in host memory, one after the other -- the reader's two
                parses (headers, then every scan), which is the host's walk inside the `on` call (that call also builds the decode tables and
                the work lists)

    python tools/progressive_batch_times.py --out profiles/progressive_batch.json [--calls 10] [--workloads small,hd,4k] [--frames-4k 64] [--lib OTHER.so]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/progressive_batch_times.py --workloads small --only on --rounds 1
    python tools/progressive_batch_times.py --levels-from DIR --workloads small --out profiles/progressive_batch_levels.json

The second form runs the `on` point alone under the profiler; the third reads the kernel trace it wrote and reports the time of the entropy launches
per level (the launches of a call come in level order) -- kernel times come from the trace, never from the host clock.
A "call" is one pass over the N frames; rates are frames per second."""
import argparse
import csv
import glob
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("small", 640, 368), ("hd", 1920, 1080), ("4k", 3840, 2160))
FRAMES = 256
KERNEL = "k_huffman_decode_prog_batch"


def picture(w, h, seed):
    """a natural-looking base picture, larger than the frames by what the per-frame shifts need"""
    rng = np.random.default_rng(seed)
    yy = np.arange(h, dtype=np.float32)[:, None]
    xx = np.arange(w, dtype=np.float32)[None, :]
    chans = []
    for k, (fx, fy, ph) in enumerate([(1 / 97.0, 1 / 61.0, 0.3), (1 / 53.0, 1 / 131.0, 1.1), (1 / 211.0, 1 / 89.0, 2.0)]):
        base = 128 + 70 * np.sin(xx * fx + ph) * np.cos(yy * fy) + 30 * np.sin((xx + yy) * fx * 3.1 + k)
        tex = 12 * np.sin(xx * 0.9 + yy * 0.35 + k) * np.sin(yy * 0.7 - xx * 0.11)
        chans.append(np.clip(base + tex + 3.0 * rng.standard_normal((h, w), dtype=np.float32), 0, 255).astype(np.uint8))
    return np.stack(chans, -1)


def save_files(w, h, n):
    """n different w x h pictures -> ([progressive files], [baseline files]) as numpy uint8 arrays, by libjpeg through PIL"""
    from PIL import Image
    base = picture(w, h, w + h)
    prog, twin = [], []
    for f in range(n):
        im = Image.fromarray(np.ascontiguousarray(np.roll(base, (37 * f, 101 * f), (0, 1))))
        for out, kw in ((prog, {"progressive": True}), (twin, {"optimize": False})):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=75, subsampling=2, **kw)
            out.append(np.frombuffer(b.getvalue(), np.uint8).copy())
    return prog, twin


def packed(streams, torch, device):
    sizes = [int(s.size) for s in streams]
    stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(stride * len(streams), np.uint8)
    for f, s in enumerate(streams):
        host[f * stride:f * stride + s.size] = s
    return torch.from_numpy(host).to(device), stride, sizes


class Point:
    """one decoder and one set of streams; run(n) times n passes over the frames as one round"""

    def __init__(self, name, G, lib, torch, family, raw, options, stats=False):
        self.name, self.torch, self.stats = name, torch, stats
        self.dec = G.Decoder(lib)
        self.dec.set_output_format(G.RGB, G.P012_444)
        for k, v in options:
            assert self.dec.set_option(k, v) == 0, (k, v)
        self.d_in, self.stride, self.sizes = family
        self.raw = raw
        self.d_out = torch.empty(raw * len(self.sizes), dtype=torch.uint8, device=self.d_in.device)
        self.rounds = []

    def call(self):
        self.dec.decode_batch(None, device_out=self.d_out.data_ptr(), out_stride=self.raw, device_in=self.d_in.data_ptr(), in_stride=self.stride, sizes=self.sizes)

    def run(self, n, timed=True):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.call()
        self.torch.cuda.synchronize()
        if timed:
            self.rounds.append((time.perf_counter() - t0) / n)

    def result(self):
        ms = [t * 1000.0 for t in self.rounds]
        med = statistics.median(ms)
        n = len(self.sizes)
        out = {"rounds_ms_per_call": [round(t, 3) for t in ms], "median_ms_per_call": round(med, 3), "frames_per_s": round(n / med * 1000.0, 1),
               "frames_per_s_min_max": [round(n / max(ms) * 1000.0, 1), round(n / min(ms) * 1000.0, 1)], "last_batch": list(self.dec.last_batch())}
        if self.stats:
            out["progressive_batch_stats"] = list(self.dec.progressive_batch_stats())
        return out


def levels_from(directory, names):
    """the kernel trace of a run of the `on` point alone over the workloads `names` (as many calls each) -> per workload and level of the entropy
    stage: launches, waves, median, minimum and maximum time"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if KERNEL in r.get("Kernel_Name", ""):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)))
    rows.sort()
    assert rows, "no " + KERNEL + " launches in the trace"
    # a call's launches come in level order; a new call starts where the grid grows again (level 0 is the widest)
    calls = []
    for i, (t0, t1, grid) in enumerate(rows):
        if i == 0 or grid > rows[i - 1][2]:
            calls.append([])
        calls[-1].append(((t1 - t0) / 1000.0, grid // 64))
    assert len(calls) % len(names) == 0, (len(calls), names)
    per = len(calls) // len(names)
    out = {"kernel": KERNEL, "workloads": {}}
    for k, name in enumerate(names):
        mine = calls[k * per:(k + 1) * per]
        levels = []
        for level in range(max(len(c) for c in mine)):
            v = [c[level] for c in mine if level < len(c)]
            levels.append({"level": level, "launches": len(v), "waves": v[0][1], "median_us": round(statistics.median(t for t, _ in v), 1),
                           "min_us": round(min(t for t, _ in v), 1), "max_us": round(max(t for t, _ in v), 1)})
        out["workloads"][name] = levels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="small")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--frames-4k", type=int, default=64, help="frames of the 4k workload (memory and the time of the off point)")
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's: the off point must equal it)")
    ap.add_argument("--only", default=None, help="one point alone (profiler runs)")
    ap.add_argument("--levels-from", default=None, help="a directory with the kernel trace of an `--only on` run: report the entropy launches per level")
    args = ap.parse_args()
    if args.levels_from:
        rep = levels_from(args.levels_from, args.workloads.split(","))
        print(json.dumps(rep), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    import torch  # (before the library: one HIP runtime per process)
    from gpujpeg_amd import libgpujpeg as G
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library(args.lib) if args.lib else G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    has_option = hasattr(lib.L, "gpujpeg_amd_decoder_get_progressive_batch_stats")  # (a library from before the option: the off point alone)
    report = {"streams": "libjpeg (PIL) q75 4:2:0, progressive=True / baseline optimize=False, no restart markers", "output": "packed RGB, device buffers",
              "calls_per_point": args.calls, "rounds": args.rounds, "workloads": {}}
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(","):
            continue
        n = args.frames_4k if wname == "4k" else args.frames
        prog, twin = save_files(w, h, n)
        raw = w * h * 3
        fam_p, fam_t = packed(prog, torch, device), packed(twin, torch, device)
        pts = [Point("off", G, lib, torch, fam_p, raw, (("dec_opt_progressive", "on"),))]
        if has_option:
            pts.append(Point("on", G, lib, torch, fam_p, raw, (("dec_opt_progressive", "on"), ("dec_opt_batch_progressive", "on")), stats=True))
        pts.append(Point("twins", G, lib, torch, fam_t, raw, (("dec_opt_batch_restartless", "on"),)))
        if args.only:
            pts = [p for p in pts if p.name == args.only]
        for p in pts:
            p.run(1 if p.name == "off" else args.warmup, timed=False)
        torch.cuda.synchronize()
        same = bool(all(torch.equal(pts[0].d_out, p.d_out) for p in pts[1:]))
        per = max(1, args.calls // args.rounds)
        parse = []
        for rnd in range(args.rounds):
            for p in pts:
                p.run(1 if p.name == "off" else per)
            print(wname, "round", rnd, {p.name: round(p.rounds[-1] * 1000.0, 3) for p in pts}, flush=True)
            t0 = time.perf_counter()
            for s in prog:
                assert G.stream_info(lib, s) is not None
            parse.append((time.perf_counter() - t0) * 1000.0)
        res = {p.name: p.result() for p in pts}
        res["host_parse"] = {"rounds_ms": [round(t, 3) for t in parse], "median_ms": round(statistics.median(parse), 3)}
        res["all_points_give_the_same_pixels"] = same
        if "on" in res and "off" in res:
            res["on_over_off"] = round(res["off"]["median_ms_per_call"] / res["on"]["median_ms_per_call"], 2)
        for k, v in res.items():
            print(wname, k, json.dumps(v), flush=True)
        report["workloads"][wname] = {"size": [w, h], "frames": n, "stream_bytes_mean": [int(np.mean(fam_p[2])), int(np.mean(fam_t[2]))], "points": res}
        for p in pts:
            p.dec.close()
        del pts, fam_p, fam_t
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
