#!/usr/bin/env python3
"""Region decode (dec_opt_region): kernel times and decode-only rates per region, on the GPU.

Public API only (gpujpeg_decoder_decode, gpujpeg_amd_decoder_get_kernel_times, _get_region_stats). Frames: the two 8K frames of
tools/scaled_decode_times.py (seeded photograph-like frame, camera fixture tiled to 8K; q75, non-interleaved 4:4:4, restart auto). The stream
lies in device memory and the pixels go to a device buffer (first two tables) or both are host buffers (third table). The points of a table --
no option, the whole image as a region, three centred rectangles, a strip and a column, on the default path and on the generic kernels
(set_fused(0)) and, with --parent-lib, no option on another build of the library, twice -- are measured in ALTERNATION: each round gives every
point a slice of calls, so drifting clocks and neighbours hit all points alike. The two parent points are the same code measured twice: their
difference is the spread every other difference has to beat.

    python tools/region_decode_times.py --out profiles/region_decode.json [--parent-lib libgpujpeg_parent.so] [--calls 200]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/region_decode_times.py --trace      (kernel names; a few calls per point)

Rates count INPUT pixels (the stream's 7680 x 4320) per second of wall clock around calls that end in a stream synchronise."""
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
import torch  # noqa: E402  (before the library: one HIP runtime per process)

from gpujpeg_amd import libgpujpeg as G  # noqa: E402

W, H = 7680, 4320
CAMERA_FIXTURE = os.path.join(ROOT, "tests", "golden", "camera_bt709_422_q95.jpg")
# (name, region): None = no option
REGIONS = (("full", None), ("whole", (0, 0, W, H)), ("3840x2160", (1920, 1080, 3840, 2160)), ("1920x1080", (2880, 1620, 1920, 1080)),
           ("512x512", (3583, 1903, 512, 512)), ("strip_7680x64", (0, 2128, 7680, 64)), ("column_64x4320", (3808, 0, 64, 4320)))


def natural_frame(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    yy = torch.arange(H, device=device, dtype=torch.float32).view(-1, 1)
    xx = torch.arange(W, device=device, dtype=torch.float32).view(1, -1)
    chans = []
    for k, (fx, fy, ph) in enumerate([(1 / 97.0, 1 / 61.0, 0.3), (1 / 53.0, 1 / 131.0, 1.1), (1 / 211.0, 1 / 89.0, 2.0)]):
        base = 128 + 70 * torch.sin(xx * fx + ph) * torch.cos(yy * fy) + 30 * torch.sin((xx + yy) * fx * 3.1 + k)
        tex = 12 * torch.sin(xx * 0.9 + yy * 0.35 + k) * torch.sin(yy * 0.7 - xx * 0.11)
        nz = 3.0 * torch.randn((H, W), device=device, generator=g)
        chans.append((base + tex + nz).clamp(0, 255).to(torch.uint8))
    return torch.stack(chans, -1).contiguous()


def camera_frame(lib, device):
    d = G.Decoder(lib)
    px, pi = d.decode(np.fromfile(CAMERA_FIXTURE, np.uint8))
    d.close()
    tile = torch.from_numpy(px.reshape(pi.height, pi.width, 3).copy()).to(device)
    return tile.repeat(-(-H // pi.height), -(-W // pi.width), 1)[:H, :W].contiguous()


def encode(lib, frame):
    p = lib.default_parameters()
    p.quality, p.restart_interval, p.verbose = 75, G.RESTART_AUTO, -1
    pi = lib.default_image_parameters()
    pi.width, pi.height = W, H
    enc = G.Encoder(lib)
    jpeg = enc.encode(p, pi, frame.data_ptr(), gpu=True)
    enc.close()
    return jpeg


class Point:
    """one decoder in one configuration; run(n) adds n calls to its samples"""

    def __init__(self, name, lib, region, fused, perf, d_jpeg, jpeg, host_out):
        self.name, self.lib, self.region, self.host_out = name, lib, region, host_out
        self.dec = G.Decoder(lib)
        if perf:
            p, pi = lib.default_parameters(), lib.default_image_parameters()
            p.perf_stats, p.verbose, pi.width, pi.height = 1, -1, 0, 0
            assert self.dec.init(p, pi) == 0
            self.dec.set_output_format(G.CS_DEFAULT, G.PIXFMT_AUTODETECT)
        if not fused:
            self.dec.set_fused(0)
        if region is not None:
            assert self.dec.set_option("dec_opt_region", "%d,%d,%d,%d" % region) == 0
        self.perf = perf
        self.src = jpeg.ctypes.data if host_out else d_jpeg.data_ptr()
        self.size = int(jpeg.size)
        self.d_out = None if host_out else torch.empty(W * H * 3, dtype=torch.uint8, device=d_jpeg.device)
        self.out = G.DecoderOutput()
        self.kernel_ms, self.wall_s, self.calls, self.path = [], 0.0, 0, None

    def call(self):
        o = self.out
        if self.host_out:
            o.type, o.data = G.DECODER_OUTPUT_INTERNAL_BUFFER, None
        else:
            o.type, o.data = G.DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, self.d_out.data_ptr()
        rc = self.lib.L.gpujpeg_decoder_decode(self.dec.h, self.src, self.size, C.byref(o))
        assert rc == 0, (self.name, rc)

    def run(self, n, timed=True):
        t0 = time.perf_counter()
        for _ in range(n):
            self.call()
            if self.perf and timed:
                ms = (C.c_float * 8)()
                assert self.lib.L.gpujpeg_amd_decoder_get_kernel_times(self.dec.h, ms) == 0
                self.kernel_ms.append(list(ms)[:5])
        if timed:
            self.wall_s += time.perf_counter() - t0
            self.calls += n

    def result(self):
        r = {"calls": self.calls, "out_pixels": list(self.region[2:]) if self.region else [W, H]}
        if self.region is not None:
            r["region_stats"] = list(self.dec.region_stats())
        if self.perf:
            med = [statistics.median(k[i] for k in self.kernel_ms) * 1000.0 for i in range(4)]
            r.update(entropy_us=round(med[0], 2), idct_us=round(med[1], 2), postprocess_us=round(med[2], 2), marker_scan_us=round(med[3], 2),
                     idct_side_us=round(med[1] + med[2], 2), idct_path=int(self.kernel_ms[-1][4]))
        else:
            r.update(ms_per_call=round(self.wall_s / self.calls * 1000.0, 4), mpix_s_input=round(W * H * self.calls / self.wall_s / 1e6, 1))
        return r


def measure(points, calls, warmup, rounds):
    for p in points:
        p.run(warmup, timed=False)
    per = max(1, calls // rounds)
    for _ in range(rounds):
        for p in points:
            p.run(per)
    return {p.name: p.result() for p in points}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's: `make variant NAME=parent`), measured without the option")
    ap.add_argument("--lib", default=None, help="the build under test when it is not the product library (a variant build beside --parent-lib's)")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames", default="natural,camera")
    ap.add_argument("--trace", action="store_true", help="a few calls per point and no report: for a kernel trace")
    ap.add_argument("--trace-lib", default=None, help="with --trace: only this library, no option")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda:0")
    lib = G.Library(args.lib)
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    parent = None
    if args.parent_lib:
        parent = G.Library(args.parent_lib)
        assert parent.L.gpujpeg_init_device(0, 0) == 0
    report = {"frame": f"{W}x{H} RGB 4:4:4 q75 non-interleaved, restart auto", "calls_per_point": args.calls, "rounds": args.rounds, "frames": {}}
    for fname in args.frames.split(","):
        frame = natural_frame(1, device) if fname == "natural" else camera_frame(lib, device)
        jpeg = encode(lib, frame)
        del frame
        d_jpeg = torch.from_numpy(jpeg).to(device)
        torch.cuda.synchronize()
        if args.trace:
            if args.trace_lib:
                tl = G.Library(args.trace_lib)
                assert tl.L.gpujpeg_init_device(0, 0) == 0
                pts = [Point("trace", tl, None, True, False, d_jpeg, jpeg, False)]
            else:
                pts = [Point(f"{n}{'' if f else '_generic'}", lib, r, f, False, d_jpeg, jpeg, False) for f in (True, False) for n, r in REGIONS]
            for p in pts:
                p.run(5, timed=False)
            continue
        out = {"jpeg_bytes": int(jpeg.size)}
        for table, perf, host in (("kernel_times_device_io", True, False), ("rate_device_io", False, False), ("rate_host_io", False, True)):
            pts = []
            if parent is not None and not host:
                pts.append(Point("parent_full_a", parent, None, True, perf, d_jpeg, jpeg, host))
            for n, r in REGIONS:
                pts.append(Point(f"default_{n}", lib, r, True, perf, d_jpeg, jpeg, host))
            if parent is not None and not host:
                pts.append(Point("parent_full_b", parent, None, True, perf, d_jpeg, jpeg, host))
            if not host:
                for n, r in REGIONS:
                    pts.append(Point(f"generic_{n}", lib, r, False, perf, d_jpeg, jpeg, host))
            out[table] = measure(pts, args.calls, args.warmup, args.rounds)
            for p in pts:
                p.dec.close()
            del pts
            for k, v in out[table].items():
                print(fname, table, k, json.dumps(v), flush=True)
        report["frames"][fname] = out
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
