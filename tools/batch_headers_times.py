#!/usr/bin/env python3
"""Crop-and-resize over streams with different headers in one family (dec_opt_batch_headers = any): frames per second against the alternatives, on the GPU.

Public API only. 256 interleaved 4:2:0 streams whose widths and heights are drawn independently and uniformly from 0.75 .. 1.25 of the workload's
nominal size (HD, 4K; fixed seed), rounded to even, as tools/restartless_batch_times.py draws them. Two sets of the same pictures:

    heterogeneous  every stream at its own quality (60 .. 95, fixed seed), every other stream with optimal Huffman tables of its own
                   (enc_opt_huffman = optimal), and a COM segment of 0 .. 30 KB behind SOI in three streams of four: no two headers are byte-equal
    family         one quality (75), the Annex K tables, no comment: the byte-equal family of profiles/crop_resize_mixed.md / restartless_batch.md

once with an explicit restart interval and once without restart markers (dec_opt_batch_restartless = on). One RandomResizedCrop rectangle per frame
against that frame's own image, to 224 x 224 packed RGB, every other frame mirrored. Streams and pixels are device buffers. The points are measured
in ALTERNATION (each round gives every point a slice of calls), wall clock around calls that end in a synchronise; the figure of a point is the
MEDIAN of its rounds, the spread their minimum and maximum:

    het_any      the heterogeneous set, dec_opt_batch_sizes = mixed and dec_opt_batch_headers = any
    het_same     the heterogeneous set, mixed alone: today's route -- the frames go the single-frame route inside the call (one call per round).
                 With device-resident streams that route plans a stranger's rectangle against the image of the frame decoded before it (its
                 speculative launch on the cached header) and refuses one that does not fit: the point is then reported as failing
    het_any_host, het_same_host   the same two with the streams in host memory (pixels still to device memory), where today's route works
    fam_same     the family, mixed alone
    fam_any      the family with `any`: against fam_same, what the option costs where it is not needed
    fam_same2    fam_same once more: the spread every difference has to beat
    fam_parent   fam_same through ANOTHER build of the library (--parent-lib: the parent commit's), taking turns in the same run

The host's share of the `any` call comes from gpujpeg_amd_decoder_get_batch_header_times (the last call of every point): bringing the headers to the
host, the reader's parse, and the family rule with table keys, table sets and geometries. --sets 16 / 256 gives the heterogeneous streams that many
distinct table sets.

    python tools/batch_headers_times.py --out profiles/batch_headers.json [--calls 20] [--workloads hd,4k] [--restart 16] [--parent-lib OTHER.so]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/batch_headers_times.py --workloads hd --only het_any --rounds 1

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


def with_comment(jpeg, n):
    """the stream with a COM segment of n payload bytes behind SOI (n = 0: unchanged)"""
    if n == 0:
        return jpeg
    seg = np.frombuffer(b"\xff\xfe" + (n + 2).to_bytes(2, "big") + b"c" * (n - 1) + b"\0", np.uint8)
    return np.concatenate([jpeg[:2], seg, jpeg[2:]])


def encode_set(lib, dims, restart, device, heterogeneous, seed, sets=0):
    """one interleaved 4:2:0 stream per (w, h) of dims in one device buffer -> (tensor, stride, sizes, the streams, the same buffer in host memory)"""
    wmax, hmax = max(w for w, _ in dims), max(h for _, h in dims)
    base = natural_frame(wmax, hmax, 1, device)
    rng = np.random.default_rng(seed)
    encs = {}
    streams = []
    for f, (w, h) in enumerate(dims):
        # (sets: 0 = every other stream with optimal tables, qualities 60 .. 95; 16 = Annex K tables at 16 qualities: 16 table sets; 256 = every
        # stream with optimal tables of its own: as many sets as streams)
        optimal = heterogeneous and (f % 2 == 1 if sets == 0 else sets >= len(dims))
        if optimal not in encs:
            encs[optimal] = G.Encoder(lib)
            assert encs[optimal].set_option(G.ENC_OPT_HUFFMAN, G.ENC_HUFFMAN_OPTIMAL if optimal else G.ENC_HUFFMAN_STANDARD) == 0
        p = lib.default_parameters()
        quality = int(rng.integers(60, 96))
        if 0 < sets < len(dims):
            quality = 60 + 2 * (f % sets)
        p.quality, p.restart_interval, p.verbose, p.interleaved = (quality if heterogeneous else 75), restart, -1, 1
        lib.L.gpujpeg_parameters_chroma_subsampling(C.byref(p), G.SUBSAMPLING_420)
        frame = torch.roll(base, (37 * f, 101 * f), (0, 1))[:h, :w].contiguous()
        pi = lib.default_image_parameters()
        pi.width, pi.height = w, h
        s = encs[optimal].encode(p, pi, frame.data_ptr(), gpu=True)
        if heterogeneous and f % 4:
            s = with_comment(s, int(rng.integers(1, 30001)) if f % 4 == 3 else int(rng.integers(1, 600)))
        streams.append(s)
    for e in encs.values():
        e.close()
    sizes = [int(s.size) for s in streams]
    stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(stride * len(streams), np.uint8)
    for f, s in enumerate(streams):
        host[f * stride:f * stride + s.size] = s
    return torch.from_numpy(host).to(device), stride, sizes, streams, host


class Point:
    """one decoder and one set of streams; run(n) times n passes over the frames as one round"""

    def __init__(self, name, lib, data, rects, mirror, options, slow=False, host=False):
        self.name, self.slow = name, slow
        self.base = data[4].ctypes.data if host else data[0].data_ptr()  # (streams in host memory: the same buffer, not copied by this tool)
        self.dec = G.Decoder(lib)
        for k, v in options:
            assert self.dec.set_option(k, v) == 0, (k, v)
        self.d_in, self.stride, self.sizes = data[:3]
        self.rects, self.mirror = rects, mirror
        self.raw = OUT * OUT * 3
        self.d_out = torch.empty(self.raw * len(self.sizes), dtype=torch.uint8, device=self.d_in.device)
        self.rounds = []

    def call(self):
        self.dec.decode_batch_crop_resize(None, self.rects, OUT, OUT, mirror=self.mirror, device_out=self.d_out.data_ptr(), out_stride=self.raw,
                                          device_in=self.base, in_stride=self.stride, sizes=self.sizes)

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
        n = len(self.sizes)
        r = {"rounds_ms_per_call": [round(t, 4) for t in ms], "median_ms_per_call": round(med, 4), "frames_per_s": round(n / med * 1000.0, 1),
             "frames_per_s_min_max": [round(n / max(ms) * 1000.0, 1), round(n / min(ms) * 1000.0, 1)], "last_batch": list(self.dec.last_batch())}
        if hasattr(self.dec, "batch_header_stats") and hasattr(self.dec.lib.L, "gpujpeg_amd_decoder_get_batch_header_stats"):
            r["batch_header_stats"] = list(self.dec.batch_header_stats())
            r["batch_header_times_ms"] = [round(x, 4) for x in self.dec.batch_header_times()[1:]]  # (gather, parse, rule + table sets + geometries: of the last call)
        return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="hd")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--restart", type=int, default=16, help="the explicit restart interval of the streams with restart markers, in MCUs")
    ap.add_argument("--modes", default="restart,restartless")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's) for the fam_parent point")
    ap.add_argument("--sets", type=int, default=0, help="distinct table sets of the heterogeneous streams: 0 = as drawn (every other stream optimal tables), 16, or 256 (one per stream)")
    ap.add_argument("--only", default=None, help="one point alone (profiler runs)")
    ap.add_argument("--points", default=None, help="these points alone, in this order inside a round (the position inside a round is worth 1 - 2 %%)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library()
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    parent = G.Library(args.parent_lib) if args.parent_lib else None
    if parent is not None:
        assert parent.L.gpujpeg_init_device(0, 0) == 0
    report = {"frames": args.frames, "streams": "4:2:0 interleaved; heterogeneous: q60-95, every other stream optimal tables, COM of 0 .. 30 KB; family: q75, Annex K tables",
              "output": [OUT, OUT], "calls_per_point": args.calls, "rounds": args.rounds, "workloads": {}}
    MIXED, ANY = (G.DEC_OPT_BATCH_SIZES, G.BATCH_SIZES_MIXED), (G.DEC_OPT_BATCH_HEADERS, G.BATCH_HEADERS_ANY)
    for wname, w, h in WORKLOADS:
        if wname not in args.workloads.split(","):
            continue
        rng = np.random.default_rng(w + h)
        dims = [(int(rng.uniform(0.75, 1.25) * w) & ~1, int(rng.uniform(0.75, 1.25) * h) & ~1) for _ in range(args.frames)]
        mirror = [f & 1 for f in range(args.frames)]
        rects = [random_resized_crops(a, b, 1, w + OUT + f)[0] for f, (a, b) in enumerate(dims)]
        for mode in args.modes.split(","):
            restart = args.restart if mode == "restart" else 0
            more = () if restart else ((G.DEC_OPT_BATCH_RESTARTLESS, G.BATCH_RESTARTLESS_ON),)
            het = encode_set(lib, dims, restart, device, True, w + 1, args.sets)
            fam = encode_set(lib, dims, restart, device, False, w + 2)
            pts = [Point("het_any", lib, het, rects, mirror, (MIXED, ANY) + more), Point("het_same", lib, het, rects, mirror, (MIXED,) + more, slow=True),
                   Point("het_any_host", lib, het, rects, mirror, (MIXED, ANY) + more, host=True),
                   Point("het_same_host", lib, het, rects, mirror, (MIXED,) + more, slow=True, host=True),
                   Point("fam_same", lib, fam, rects, mirror, (MIXED,) + more), Point("fam_any", lib, fam, rects, mirror, (MIXED, ANY) + more),
                   Point("fam_same2", lib, fam, rects, mirror, (MIXED,) + more)]
            if parent is not None:
                pts.append(Point("fam_parent", parent, fam, rects, mirror, (MIXED,) + more))
            if args.only:
                pts = [p for p in pts if p.name == args.only]
            if args.points:
                pts = [p for name in args.points.split(",") for p in pts if p.name == name]
            failed = {}
            for p in list(pts):
                try:
                    p.run(1 if p.slow else args.warmup, timed=False)
                except RuntimeError as e:  # (today's route on device-resident strangers, see above)
                    failed[p.name] = str(e)
                    pts.remove(p)
            torch.cuda.synchronize()
            by = {p.name: p for p in pts}
            out = {"nominal": [w, h], "restart_interval": restart, "stream_bytes_mean": [int(np.mean(het[2])), int(np.mean(fam[2]))],
                   "header_bytes_max": int(max(bytes(s).index(b"\xff\xda") for s in het[3]))}
            out["points_that_fail"] = failed
            for a, b in (("het_any", "het_same"), ("het_any", "het_any_host"), ("het_any_host", "het_same_host")):
                if a in by and b in by:
                    out[a + "_equals_" + b] = bool(torch.equal(by[a].d_out, by[b].d_out))
            if "fam_any" in by and "fam_same" in by:
                out["fam_any_equals_fam_same"] = bool(torch.equal(by["fam_any"].d_out, by["fam_same"].d_out))
            per = max(1, args.calls // args.rounds)
            parse = []
            for rnd in range(args.rounds):
                for p in pts:
                    p.run(1 if p.slow else per)
                print(wname, mode, "round", rnd, {p.name: round(p.rounds[-1] * 1000.0, 3) for p in pts}, flush=True)
                t0 = time.perf_counter()
                for s in het[3]:
                    assert G.stream_info(lib, s) is not None
                parse.append((time.perf_counter() - t0) * 1000.0)
            out["points"] = {p.name: p.result() for p in pts}
            out["host_parse_of_the_heterogeneous_streams_ms"] = {"rounds": [round(t, 3) for t in parse], "median": round(statistics.median(parse), 3)}
            for k, v in out["points"].items():
                print(wname, mode, k, json.dumps(v), flush=True)
            for p in pts:
                p.dec.close()
            del pts, by, het, fam
            report["workloads"][wname + "_" + mode] = out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
