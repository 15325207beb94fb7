"""Batched region decode with one crop per frame (gpujpeg_amd_decoder_decode_batch_regions; gpujpeg_amd_ext.h).

The definition of frame f's result is the single-frame region call: what gpujpeg_decoder_decode returns for stream f with
dec_opt_region = "X_f,Y_f,W,H". Expected pixels are the cropped oracle decode (oracle.decode + a numpy crop, no product code) and the same
library's single region calls; nothing is compared with the batched path itself. Every comparison is byte for byte.

Two tiers with the same bodies, like test_region_decode.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Damaged streams run on the CPU tier only. One test re-runs the CPU tier on the AddressSanitizer + UBSan build."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import CASES, make_raw, natural_image, oracle_image, random_case, random_raw
from test_region_decode import GRID, OPT, case_named, case_stream, crop, damaged_restart_markers, opt_value, perf_decoder

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")
ASAN_DIR = os.path.join(EMU_DIR, "_build_asan")
ASAN_LIB = os.path.join(ASAN_DIR, "libgpujpeg_emu.so")
CLANG_RT = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"


@pytest.fixture(scope="session")
def emu(G):
    """The product's host C and .hip files on the CPU execution model (built like test_emu_parity.py's emu_lib)."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None:
        pytest.skip("hipemu needs ROCm's clang++ (host compilation of the .hip files)")
    import fcntl
    with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-j8", "-C", EMU_DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = G.Library(os.environ.get("GJ_EMU_LIB") or EMU_LIB)
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    return lib


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dlib(request):
    """the library of the tier: the CPU execution model, or the product on the GPU (lib.tier says which)"""
    lib = request.getfixturevalue("emu" if request.param == "emu" else "gpu_lib")
    lib.tier = request.param
    return lib


# ================================================================================================ helpers
def frames_of(O, case, n, seed=20):
    """n streams of one configuration (one header) with different content"""
    name, w, h, pf = case[:4]
    comps = {0: 1, 1: 3, 6: 4}.get(pf)
    out = []
    for f in range(n):
        raw = natural_image(w, h, comps, seed=seed + f) if comps and f % 2 == 0 else O.noise(O.raw_size(w, h, pf), seed=seed + f)
        out.append(O.encode(oracle_image(O, case), raw))
    return out


def new_decoder(G, lib, pf=None, cs=None, align=None):
    dec = G.Decoder(lib)
    if pf is not None:
        dec.set_output_format(cs, pf)
    if align:
        assert dec.set_option("dec_opt_alignment_bytes", str(align)) == 0
    return dec


def single_calls(G, lib, streams, origins, W, H, pf=None, cs=None, align=None):
    """the definition: one decoder of the same kind, dec_opt_region + gpujpeg_decoder_decode per frame -> (pixels, ImageParameters, stats) per frame"""
    dec = new_decoder(G, lib, pf, cs, align)
    out = []
    for jpeg, (x, y) in zip(streams, origins):
        assert dec.set_option(OPT, opt_value((x, y, W, H))) == 0
        px, pi = dec.decode(jpeg)
        out.append((px, pi, dec.region_stats()))
    dec.close()
    return out


def oracle_crops(O, streams, origins, W, H, pf=None, cs=None, pad_r=0):
    out = []
    for jpeg, (x, y) in zip(streams, origins):
        raw, img = O.decode(jpeg, -1 if pf is None else pf, -1 if cs is None else cs)
        out.append(crop(raw, img.width, img.height, img.pixel_format, (x, y, W, H), pad_r=pad_r))
    return out


def same(got, want):
    return len(got) == len(want) and all(a.size == b.size and np.array_equal(a, b) for a, b in zip(got, want))


def raw_call(G, lib, dec, streams, origins, W, H, out, stride):
    """the C call with a caller-owned host output buffer -> return code"""
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    buf = np.zeros(in_stride * len(sizes), np.uint8)
    for i, x in enumerate(streams):
        buf[i * in_stride:i * in_stride + x.size] = x
    n = len(sizes)
    csz = (C.c_size_t * n)(*sizes)
    org = (C.c_int * (2 * n))(*[int(v) for xy in origins for v in xy])
    pi = G.ImageParameters()
    return lib.L.gpujpeg_amd_decoder_decode_batch_regions(dec.h, buf.ctypes.data, in_stride, csz, n, org, W, H, out.ctypes.data, stride, C.byref(pi))


# six frames of rgb_hdlike_r24 (480 x 272, 60 blocks per row, restart interval 24: segments wrap rows), W x H = 100 x 45:
# covers 13 (X mod 8 <= 4) and 14 (>= 5) blocks wide, 6 (Y mod 8 <= 3) and 7 (>= 4) blocks high, (0, 0), and (380, 227) that ends at both image edges
HD_CASE = "rgb_hdlike_r24"
HD_W, HD_H = 100, 45
HD_ORIGINS = [(0, 0), (380, 227), (13, 20), (100, 3), (205, 100), (64, 68)]


@pytest.fixture(scope="module")
def hd(O):
    """the streams of tests 1 and 2 and their cropped oracle decodes, made once"""
    case = case_named(HD_CASE)
    streams = frames_of(O, case, len(HD_ORIGINS))
    assert {((x % 8 + HD_W - 1) // 8 + 1, (y % 8 + HD_H - 1) // 8 + 1) for x, y in HD_ORIGINS} == {(13, 6), (14, 7), (13, 7)}
    return streams, oracle_crops(O, streams, HD_ORIGINS, HD_W, HD_H)


# ================================================================================================ 1. crops differ per frame, both routes
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("mode", ["GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS"])
def test_crops_differ_per_frame(O, G, dlib, hd, mode, chunk, monkeypatch):
    streams, want = hd
    monkeypatch.setenv(mode, "1")
    singles = single_calls(G, dlib, streams, HD_ORIGINS, HD_W, HD_H)
    assert same([s[0] for s in singles], want)
    dec = perf_decoder(G, dlib)
    if chunk:
        dec.set_batch_chunk(chunk)
    n = len(streams)
    for rep in range(2):
        got, pi = dec.decode_batch_regions(streams, HD_ORIGINS, HD_W, HD_H)
        assert (pi.width, pi.height, pi.pixel_format, pi.color_space) == (HD_W, HD_H, 1, 1) and dlib.image_size(pi) == want[0].size
        assert same(got, want), (rep, [int(np.count_nonzero(a != b)) for a, b in zip(got, want)])
        batched, single = dec.last_batch()
        assert batched + single == n and single <= 1, (batched, single)
        st = dec.region_stats()
        assert st[0] == 1
        assert st[1] == sum(s[2][1] for s in singles) < n * singles[0][2][3], st
        assert st[2] == sum(s[2][2] for s in singles) and st[3] == sum(s[2][3] for s in singles), st
        assert dec.idct_path() == (4 if mode == "GJ_DEC_TOKENS" else 3), "the route of the batched launches"
    dec.close()


# ================================================================================================ 2. padding is exercised, not assumed
@pytest.mark.parametrize("mode", ["GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS"])
def test_null_entries_fill_whole_batches(O, G, dlib, hd, mode, monkeypatch):
    """GJ_DEC_G=1: one table entry per batch of the entropy decoders, so the null entries behind a frame's own selection are batches of their own"""
    streams, want = hd
    monkeypatch.setenv(mode, "1")
    monkeypatch.setenv("GJ_DEC_G", "1")
    singles = single_calls(G, dlib, streams, HD_ORIGINS, HD_W, HD_H)
    assert len({s[2][1] for s in singles}) > 1, "the origins give every frame the same number of selected segments: the test shows nothing"
    dec = new_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_regions(streams, HD_ORIGINS, HD_W, HD_H)
        assert same(got, want), rep
        assert dec.last_batch()[1] <= 1 and dec.region_stats()[1] == sum(s[2][1] for s in singles)
    dec.close()


# ================================================================================================ 3. other configurations on the plane route
# (case, output pixel format / colour space or None = the stream's, W, H, line alignment)
PLANE_CONFIGS = [("rgb_interleaved", None, None, 51, 29, 64), ("rgb_to_420_il", 5, 3, 50, 30, 0), ("rgb_to_422_nonil", None, None, 37, 21, 0),
                 ("uyvy_422_il_q90", None, None, 50, 30, 0), ("gray", None, None, 45, 23, 0), ("rgba_4444", None, None, 33, 19, 0),
                 ("planar444_in", None, None, 41, 27, 0)]


@pytest.mark.parametrize("name,pf,cs,W,H,align", PLANE_CONFIGS, ids=[c[0] for c in PLANE_CONFIGS])
def test_plane_route_configurations(O, G, dlib, name, pf, cs, W, H, align):
    case = case_named(name)
    w, h = case[1], case[2]
    pf, cs = (case[3], case[4]) if pf is None else (pf, cs)  # (the requested output: the stream's own format, or another one)
    out_pf = pf
    ah, av = GRID.get(out_pf, (1, 1))
    origins = [(0, 0), (w - W, h - H), ((w // 3) // ah * ah, min(h // 2 + 3, h - H) // av * av), ((w // 2 + 5) // ah * ah, 0)]
    assert all(x % ah == 0 and y % av == 0 and x + W <= w and y + H <= h for x, y in origins)
    streams = frames_of(O, case, 4, seed=40)
    singles = single_calls(G, dlib, streams, origins, W, H, pf, cs, align)
    pad = singles[0][1].width_padding
    assert (pad != 0) == bool(align)
    want = oracle_crops(O, streams, origins, W, H, pf, cs)

    def pixels(frames):  # (dec_opt_alignment_bytes pads the region's lines: what lies in the padding is nobody's)
        if not pad:
            return frames
        pitch = W * 3 + pad
        return [px[:H * pitch].reshape(H, pitch)[:, :W * 3].reshape(-1) for px in frames]

    assert same(pixels([s[0] for s in singles]), want)
    dec = new_decoder(G, dlib, pf, cs, align)
    for rep in range(2):
        got, pi = dec.decode_batch_regions(streams, origins, W, H)
        assert (pi.width, pi.height, pi.pixel_format, pi.width_padding) == (W, H, out_pf, pad)
        assert all(a.size == s[0].size == dlib.image_size(pi) for a, s in zip(got, singles))
        assert same(pixels(got), want), (rep, [int(np.count_nonzero(a != b)) for a, b in zip(pixels(got), want)])
        assert dec.last_batch()[1] <= 1, dec.last_batch()
        st = dec.region_stats()
        assert st[0] == 1 and st[1:] == tuple(sum(s[2][i] for s in singles) for i in (1, 2, 3)), st
    dec.close()


# ================================================================================================ 4. fallbacks
def test_restart_interval_0_goes_frame_by_frame(O, G, dlib):
    case = case_named("rgb_restart0")
    streams = frames_of(O, case, 3, seed=60)
    origins = [(0, 0), (100 - 40, 60 - 25), (33, 17)]
    want = oracle_crops(O, streams, origins, 40, 25)
    dec = new_decoder(G, dlib)
    for rep in range(2):
        got, pi = dec.decode_batch_regions(streams, origins, 40, 25)
        assert same(got, want) and (pi.width, pi.height) == (40, 25)
        assert dec.last_batch() == (0, 3)
        st = dec.region_stats()
        assert st[0] == 2 and st[1] == st[3] == 9, st
    dec.close()


def test_a_stream_of_another_size_fails_the_call(O, G, dlib):
    streams = frames_of(O, case_named(HD_CASE), 3)
    other = case_stream(O, case_named("rgb_natural_auto"))  # 640 x 368: the rectangles below lie inside it as well
    origins = [(0, 0), (8, 8), (16, 16)]
    dec = new_decoder(G, dlib)
    with pytest.raises(RuntimeError):
        dec.decode_batch([streams[0], other, streams[2]])
    for rep in range(2):
        with pytest.raises(RuntimeError):
            dec.decode_batch_regions([streams[0], other, streams[2]], origins, 64, 40)
        got, _ = dec.decode_batch_regions(streams, origins, 64, 40)  # (and with a header to launch on the second time)
        assert same(got, oracle_crops(O, streams, origins, 64, 40))
    # the decoder's own region option across a call that fails part-way: the batch's rectangles travel in its calls' requests, never in the option
    own, full0 = (5, 7, 50, 40), O.decode(streams[0])[0]
    assert dec.set_option(OPT, opt_value(own)) == 0
    with pytest.raises(RuntimeError):
        dec.decode_batch_regions([streams[0], other, streams[2]], origins, 64, 40)
    px, pi = dec.decode(streams[0])
    assert (pi.width, pi.height) == (50, 40) and np.array_equal(px, crop(full0, 480, 272, 1, own))
    got, _ = dec.decode_batch_regions(streams, origins, 64, 40)
    assert same(got, oracle_crops(O, streams, origins, 64, 40))
    assert dec.set_option(OPT, "full") == 0
    px, pi = dec.decode(streams[0])
    assert (pi.width, pi.height) == (480, 272) and np.array_equal(px, full0) and dec.region_stats()[0] == 0
    dec.close()


def test_damaged_restart_markers_in_one_frame(O, G, emu):
    """(CPU tier and sanitizer build only) frame 2's restart markers are damaged: its bytes are what the single region call returns for that stream,
    its neighbours stay in the batched launches"""
    streams, origins = frames_of(O, case_named(HD_CASE), 5), HD_ORIGINS[:5]
    good = oracle_crops(O, streams, origins, HD_W, HD_H)
    for kind, bad, _ in damaged_restart_markers(streams[2]):
        ref = new_decoder(G, emu)
        assert ref.set_option(OPT, opt_value(origins[0] + (HD_W, HD_H))) == 0
        ref.decode(streams[0])  # (a header to launch on, as the batch call has when it reaches frame 2)
        assert ref.set_option(OPT, opt_value(origins[2] + (HD_W, HD_H))) == 0
        try:
            want2 = ref.decode(bad)[0]
        except RuntimeError:
            want2 = None
        ref.close()
        mixed = streams[:2] + [bad] + streams[3:]
        dec = new_decoder(G, emu)
        for rep in range(2):
            if want2 is None:
                with pytest.raises(RuntimeError):
                    dec.decode_batch_regions(mixed, origins, HD_W, HD_H)
                continue
            got, _ = dec.decode_batch_regions(mixed, origins, HD_W, HD_H)
            assert np.array_equal(got[2], want2), (kind, rep)
            assert same(got[:2] + got[3:], good[:2] + good[3:]), (kind, rep)
            batched, single = dec.last_batch()
            assert single <= 2 and batched >= 3, (kind, batched, single)
        got, _ = dec.decode_batch_regions(streams, origins, HD_W, HD_H)  # the decoder decodes the intact streams as ever
        assert same(got, good), kind
        dec.close()


# ================================================================================================ 5. refusals
def test_refusals_write_nothing_and_leave_the_decoder_usable(O, G, dlib):
    streams = frames_of(O, case_named(HD_CASE), 4)
    ok = HD_ORIGINS[:4]
    want = oracle_crops(O, streams, ok, HD_W, HD_H)
    stride = want[0].size + 32

    def refused(dec, origins, W, H):
        out = np.full(stride * 4, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, origins, W, H, out, stride) == -1, (origins, W, H)
        assert np.all(out == 0xA5), "a refused call wrote to the output"

    def accepted(dec, wanted=want):
        out = np.full(stride * 4, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, ok, HD_W, HD_H, out, stride) == 0
        rows = out.reshape(4, stride)
        assert all(np.array_equal(rows[f, :wanted[f].size], wanted[f]) for f in range(4)) and np.all(rows[:, wanted[0].size:] == 0xA5)

    bad_sets = [(ok[:2] + [(480, 0)] + ok[3:], HD_W, HD_H), (ok[:3] + [(0, 272)], HD_W, HD_H), (ok[:1] + [(381, 0)] + ok[2:], HD_W, HD_H),
                (ok[:3] + [(10, 228)], HD_W, HD_H), ([(-1, 0)] + ok[1:], HD_W, HD_H), (ok, 0, HD_H), (ok, HD_W, 0), (ok, -3, -3), (ok, 481, 10), (ok, 10, 273)]
    for cold in (True, False):  # (without a header to launch on: frame 0 goes ahead; with one: the rectangles meet the cached header's geometry)
        dec = new_decoder(G, dlib)
        if not cold:
            accepted(dec)
        for origins, W, H in bad_sets:
            refused(dec, origins, W, H)
            if cold:
                accepted(dec)
                dec.close()
                dec = new_decoder(G, dlib)
        accepted(dec)
        # a scale, a flip
        assert dec.set_option("dec_opt_scale", "1/2") == 0
        refused(dec, ok, HD_W, HD_H)
        assert dec.set_option("dec_opt_scale", "1") == 0
        accepted(dec)
        assert dec.set_option("dec_opt_flipped", "1") == 0
        refused(dec, ok, HD_W, HD_H)
        assert dec.set_option("dec_opt_flipped", "0") == 0
        accepted(dec)
        dec.close()
    # off the sampling grid of planar 4:2:0 output: odd X, odd Y, odd W away from the right edge
    dec = new_decoder(G, dlib, 5, 3)
    want420 = oracle_crops(O, streams, [(x & ~1, y & ~1) for x, y in ok], 100, 44, 5, 3)
    for origins, W, H in (([(1, 0)] + ok[1:], 100, 44), ([(0, 0), (2, 1), (4, 4), (6, 6)], 100, 44), ([(0, 0), (2, 2), (4, 4), (6, 6)], 99, 44)):
        out = np.full(stride * 4, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, origins, W, H, out, stride) == -1 and np.all(out == 0xA5), (origins, W, H)
        got, _ = dec.decode_batch_regions(streams, [(x & ~1, y & ~1) for x, y in ok], 100, 44)
        assert same(got, want420)
    dec.close()


# ================================================================================================ 6. state
def test_the_decoders_own_region_option_is_untouched(O, G, dlib):
    streams, origins = frames_of(O, case_named(HD_CASE), 3), HD_ORIGINS[2:5]
    want = oracle_crops(O, streams, origins, HD_W, HD_H)
    full0 = O.decode(streams[0])[0]
    dec = new_decoder(G, dlib)
    own = (5, 7, 50, 40)
    assert dec.set_option(OPT, opt_value(own)) == 0
    for rep in range(2):
        got, pi = dec.decode_batch_regions(streams, origins, HD_W, HD_H)
        assert same(got, want) and (pi.width, pi.height) == (HD_W, HD_H)
        px, pi = dec.decode(streams[0])  # the option is in force as before ...
        assert (pi.width, pi.height) == (50, 40) and np.array_equal(px, crop(full0, 480, 272, 1, own))
        got, pi = dec.decode_batch(streams)  # ... and decode_batch with it goes frame by frame, as ever
        assert dec.last_batch() == (0, 3) and (pi.width, pi.height) == (50, 40)
        assert same(got, [crop(O.decode(x)[0], 480, 272, 1, own) for x in streams])
    assert dec.set_option(OPT, "full") == 0
    got, _ = dec.decode_batch_regions(streams, origins, HD_W, HD_H)
    assert same(got, want)
    px, pi = dec.decode(streams[0])
    assert (pi.width, pi.height) == (480, 272) and np.array_equal(px, full0) and dec.region_stats()[0] == 0
    dec.close()


@pytest.mark.parametrize("mode", ["GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS"])
def test_state_between_calls(O, G, dlib, mode, monkeypatch):
    """a batch of regions leaves coefficients of uncovered blocks and stale block records in the batch buffers: the full-frame batch, the single
    calls and another batch of regions that follow on the same decoder do not trust them"""
    monkeypatch.setenv(mode, "1")
    case = case_named(HD_CASE)
    streams = frames_of(O, case, 4)
    others = frames_of(O, case, 4, seed=90)
    full, full_o = [O.decode(x)[0] for x in streams], [O.decode(x)[0] for x in others]
    A, B = HD_ORIGINS[:4], [(300, 200), (7, 90), (230, 11), (111, 111)]
    want_a, want_b = oracle_crops(O, streams, A, HD_W, HD_H), oracle_crops(O, others, B, 150, 60)
    dec = new_decoder(G, dlib)
    bad_want = None
    if dlib.tier == "emu":  # (damaged streams: CPU tier only) what a decoder of its own makes of the damaged stream
        kind, bad, _ = damaged_restart_markers(others[1])[0]
        ref = new_decoder(G, dlib)
        ref.decode(others[0])
        bad_want = ref.decode(bad)[0]
        ref.close()
    for rep in range(2):
        got, _ = dec.decode_batch_regions(streams, A, HD_W, HD_H)
        assert same(got, want_a), rep
        if bad_want is not None:  # a damaged full-frame stream right after the batch of regions
            got, _ = dec.decode_batch([others[0], bad, others[2]])
            assert np.array_equal(got[0], full_o[0]) and np.array_equal(got[2], full_o[2]) and np.array_equal(got[1], bad_want), rep
        got, pi = dec.decode_batch(others)
        assert same(got, full_o) and (pi.width, pi.height) == (480, 272), rep
        got, _ = dec.decode_batch_regions(others, B, 150, 60)
        assert same(got, want_b), rep
        px, _ = dec.decode(streams[3])
        assert np.array_equal(px, full[3]), rep
        got, _ = dec.decode_batch(streams)
        assert same(got, full), rep
    dec.close()


# ================================================================================================ 7. device buffers
@pytest.mark.gpu
def test_device_streams_and_device_output(O, G, gpu_lib):
    import torch
    streams, want = frames_of(O, case_named(HD_CASE), len(HD_ORIGINS)), None
    want = oracle_crops(O, streams, HD_ORIGINS, HD_W, HD_H)
    n, raw = len(streams), want[0].size
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    d_in = torch.from_numpy(host).cuda()
    out_stride = raw + 61
    d_out = torch.full((out_stride * n,), 0xA5, dtype=torch.uint8, device="cuda")
    dec = new_decoder(G, gpu_lib)
    # a refusal leaves the device buffer as it was
    with pytest.raises(RuntimeError):
        dec.decode_batch_regions(None, HD_ORIGINS[:5] + [(400, 250)], HD_W, HD_H, device_out=d_out.data_ptr(), out_stride=out_stride, device_in=d_in.data_ptr(),
                                 in_stride=in_stride, sizes=sizes)
    torch.cuda.synchronize()
    assert bool(torch.all(d_out == 0xA5))
    for rep in range(2):
        d_out.fill_(0xA5)
        _, pi = dec.decode_batch_regions(None, HD_ORIGINS, HD_W, HD_H, device_out=d_out.data_ptr(), out_stride=out_stride, device_in=d_in.data_ptr(),
                                         in_stride=in_stride, sizes=sizes)
        torch.cuda.synchronize()
        rows = d_out.cpu().numpy().reshape(n, out_stride)
        assert (pi.width, pi.height) == (HD_W, HD_H)
        assert all(np.array_equal(rows[f, :raw], want[f]) for f in range(n)) and np.all(rows[:, raw:] == 0xA5), rep
        assert dec.region_stats()[0] == 1
    assert dec.last_batch() == (n, 0), "the second call has a header to launch on: every frame through the batched launches"
    dec.close()


# ================================================================================================ 8. random differential
def random_origins(rng, w, h, pf, n):
    """a random W x H and n legal origins for it in a w x h image of output format pf"""
    ah, av = GRID.get(pf, (1, 1))
    W = ah * int(rng.integers(1, w // ah + 1)) if w >= ah else w
    H = av * int(rng.integers(1, h // av + 1)) if h >= av else h
    return W, H, [(int(rng.integers(0, (w - W) // ah + 1)) * ah, int(rng.integers(0, (h - H) // av + 1)) * av) for _ in range(n)]


@pytest.mark.parametrize("seed", range(20))
def test_random_configurations(O, G, emu, seed):
    case = random_case(seed)
    streams = [O.encode(oracle_image(O, case), random_raw(O, case, seed + 100 * f)) for f in range(3)]
    rng = np.random.default_rng(7000 + seed)
    dec = new_decoder(G, emu, case[3], case[4])
    for _ in range(2):
        W, H, origins = random_origins(rng, case[1], case[2], case[3], 3)
        singles = single_calls(G, emu, streams, origins, W, H, case[3], case[4])
        got, pi = dec.decode_batch_regions(streams, origins, W, H)
        assert (pi.width, pi.height) == (W, H)
        assert same(got, [s[0] for s in singles]), (case, W, H, origins)
        st = dec.region_stats()
        assert st[1:] == tuple(sum(s[2][i] for s in singles) for i in (1, 2, 3)) and st[0] == max(s[2][0] for s in singles), (st, case)
    dec.close()


# ================================================================================================ 10. larger frames
@pytest.mark.gpu
def test_hd_frames_take_the_token_route_by_themselves(O, G, gpu_lib):
    """16 x 1920 x 1080, 224 x 224 crops at seeded random origins: the token gate opens for the batch without a setting"""
    w, h, n, W = 1920, 1080, 16, 224
    base = natural_image(w, h, 3, seed=3).reshape(h, w, 3)
    p, pi = gpu_lib.default_parameters(), gpu_lib.default_image_parameters()
    p.quality, p.restart_interval, p.interleaved, p.verbose = 75, -1, 0, -1
    pi.width, pi.height, pi.pixel_format, pi.color_space = w, h, 1, 1
    enc = G.Encoder(gpu_lib)
    streams = [enc.encode(p, pi, np.ascontiguousarray(np.roll(base, (37 * f, 101 * f), (0, 1))).reshape(-1)) for f in range(n)]
    enc.close()
    rng = np.random.default_rng(16)
    origins = [(int(rng.integers(0, w - W + 1)), int(rng.integers(0, h - W + 1))) for _ in range(n)]
    want = oracle_crops(O, streams[:4], origins[:4], W, W) + [s[0] for s in single_calls(G, gpu_lib, streams[4:], origins[4:], W, W)]
    dec = perf_decoder(G, gpu_lib)
    for rep in range(2):
        got, pi2 = dec.decode_batch_regions(streams, origins, W, W)
        assert (pi2.width, pi2.height) == (W, W) and same(got, want), rep
        batched, single = dec.last_batch()
        assert single <= 1 and batched >= n - 1
        assert dec.idct_path() == 4 and dec.region_stats()[0] == 1
    dec.close()


# ================================================================================================ 9. sanitizers
@pytest.fixture(scope="session")
def asan_env():
    if not os.path.exists(CLANG_RT) or shutil.which("make") is None:
        pytest.skip("needs ROCm's clang with its AddressSanitizer runtime")
    import fcntl
    with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-j8", "-C", EMU_DIR, "SAN=1", "OPT=-O1", f"OUT={ASAN_DIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return dict(os.environ, LD_PRELOAD=CLANG_RT, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0:abort_on_error=1",
                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_cpu_tier_under_sanitizers(asan_env):
    """this file's CPU-tier tests once more on the AddressSanitizer + UBSan build of the execution model (the per-frame records, the padded
    compacted tables, the planes of the largest cover, the damaged frame inside a batch)"""
    env = dict(asan_env, GJ_EMU_LIB=ASAN_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-n", "4", "-m", "not gpu", "-p", "no:faulthandler",
                        "-p", "no:cacheprovider", "-k", "not under_sanitizers"], capture_output=True, text=True, errors="replace",
                       timeout=1500, env=env, cwd=ROOT)
    tail = (r.stdout[-1500:] + "\n" + "\n".join(ln for ln in r.stderr.splitlines() if not ln.startswith("[GPUJPEG]"))[-3000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1500:]
