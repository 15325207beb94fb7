"""Region-of-interest decode (decoder option dec_opt_region = X,Y,W,H; gpujpeg_amd_ext.h).

The definition is the crop of the full decode: pixel (i, j) of the result is pixel (X + i, Y + j) of what the decoder returns without the
option. Expected pixels use no product code: oracle.decode(jpeg, pf, cs) -- pinned to the reference by the other suites -- cropped in numpy
(per plane for planar formats, per pixel pair for packed 4:2:2). Every comparison is byte for byte. What a call skipped is read from
gpujpeg_amd_decoder_get_region_stats and compared with counts a plain Python loop over the geometry's blocks gives.

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on the MI355X.
One test re-runs the CPU tier on the AddressSanitizer + UBSan build of the execution model."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import CASES, make_raw, natural_image, oracle_image, random_case, random_raw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")
ASAN_DIR = os.path.join(EMU_DIR, "_build_asan")
ASAN_LIB = os.path.join(ASAN_DIR, "libgpujpeg_emu.so")
CLANG_RT = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"
OPT = "dec_opt_region"
# output formats whose pixels share samples: (horizontal, vertical) grid the region has to lie on
GRID = {3: (2, 1), 4: (2, 1), 5: (2, 2)}
# chroma planes of the planar formats: (horizontal, vertical) subsampling
PLANAR = {2: (1, 1), 4: (2, 1), 5: (2, 2)}
BPP = {0: 1, 1: 3, 6: 4}


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
    """the library of the tier: the CPU execution model, or the product on the GPU"""
    return request.getfixturevalue("emu" if request.param == "emu" else "gpu_lib")


# ================================================================================================ the definition: a crop, in numpy
def crop(full, w, h, pf, reg, pad=0, pad_r=0):
    """the W x H image at (X, Y) of the w x h image `full` of pixel format pf (line paddings of packed formats: pad in, pad_r out)"""
    X, Y, W, H = reg
    if pf in BPP:
        b = BPP[pf]
        rows = full[:h * (w * b + pad)].reshape(h, w * b + pad)[Y:Y + H, X * b:(X + W) * b]
        return np.concatenate([rows, np.zeros((H, pad_r), np.uint8)], 1).reshape(-1) if pad_r else rows.reshape(-1)
    if pf == 3:  # packed 4:2:2: pixel pairs of 4 bytes
        assert w % 2 == 0 and X % 2 == 0
        return full.reshape(h, w * 2)[Y:Y + H, X * 2:(X + ((W + 1) & ~1)) * 2].reshape(-1)
    hs, vs = PLANAR[pf]
    cw, ch = -(-w // hs), -(-h // vs)
    assert X % hs == 0 and Y % vs == 0
    y = full[:w * h].reshape(h, w)[Y:Y + H, X:X + W]
    out = [y.reshape(-1)]
    for c in range(2):
        p = full[w * h + c * cw * ch:w * h + (c + 1) * cw * ch].reshape(ch, cw)
        out.append(p[Y // vs:Y // vs + -(-H // vs), X // hs:X // hs + -(-W // hs)].reshape(-1))
    return np.concatenate(out)


def regions(w, h, pf):
    """the issue's regions for a w x h image of output format pf: whole image, interior rectangle (all four numbers odd where the format allows),
    a single pixel (pixel pair / quad), the bottom-right corner up to both edges, a full-width strip lower than a block, a full-height strip
    narrower than a block"""
    ah, av = GRID.get(pf, (1, 1))

    def fit(x, y, W, H):
        x, y = min(x, w - 1) // ah * ah, min(y, h - 1) // av * av
        W, H = max(1, min(W, w - x)), max(1, min(H, h - y))
        if W % ah and x + W != w:
            W = W + 1 if x + W + 1 <= w else W - 1
        if H % av and y + H != h:
            H = H + 1 if y + H + 1 <= h else H - 1
        return (x, y, W, H) if W >= 1 and H >= 1 else None

    want = [(0, 0, w, h), fit((w // 3) | 1, (h // 3) | 1, (w // 4) | 1, (h // 4) | 1), fit(w // 2, h // 2, ah, av), fit(max(0, w - 13), max(0, h - 11), w, h),
            fit(0, (h // 2) | 1, w, 5), fit((w // 2) | 1, 0, 5, h)]
    out = []
    for r in want:
        if r is not None and r not in out:
            out.append(r)
    return out


def opt_value(reg):
    return "%d,%d,%d,%d" % tuple(reg)


def decode_region(G, lib, jpeg, pf, cs, reg, dec=None):
    own = dec is None
    if own:
        dec = G.Decoder(lib)
    try:
        if pf is not None and getattr(dec, "_fmt", None) != (cs, pf):  # (setting the format drops the header cache: once per decoder)
            dec.set_output_format(cs, pf)
            dec._fmt = (cs, pf)
        assert dec.set_option(OPT, "full" if reg is None else opt_value(reg)) == 0
        return dec.decode(jpeg)
    finally:
        if own:
            dec.close()


def check(O, G, lib, jpeg, pf, cs, reg, dec=None, full=None):
    """the contract of one region decode: pixels, returned parameters and size"""
    if full is None:
        full = O.decode(jpeg, -1 if pf is None else pf, -1 if cs is None else cs)
    raw, img = full
    want = crop(raw, img.width, img.height, img.pixel_format, reg)
    px, pi = decode_region(G, lib, jpeg, pf, cs, reg, dec)
    assert (pi.width, pi.height, pi.pixel_format) == (reg[2], reg[3], img.pixel_format), (pi.width, pi.height, pi.pixel_format)
    assert px.size == want.size == O.raw_size(reg[2], reg[3], img.pixel_format) == lib.image_size(pi), (px.size, want.size)
    assert np.array_equal(px, want), (reg, int(np.count_nonzero(px != want)))
    return px


def case_named(name):
    return [c for c in CASES if c[0] == name][0]


def case_stream(O, case):
    return O.encode(oracle_image(O, case), make_raw(O, case))


# ================================================================================================ what a call may skip, counted in plain Python
def stream_geometry(G, lib, jpeg):
    """numbers of gpujpeg_amd_host_geometry for the stream's own parameters + its sampling factors"""
    pi, p = G.ImageParameters(), G.Parameters()
    assert lib.L.gpujpeg_decoder_get_image_info(jpeg.ctypes.data_as(C.c_void_p), jpeg.size, C.byref(pi), C.byref(p), None) == 0
    geo = (C.c_int * 20)()
    lib.L.gpujpeg_amd_host_geometry.argtypes = [C.POINTER(G.Parameters), C.POINTER(G.ImageParameters), C.POINTER(C.c_int)]
    assert lib.L.gpujpeg_amd_host_geometry(C.byref(p), C.byref(pi), geo) == 0
    n = p.comp_count
    samp = [(p.sampling_factor[c].horizontal, p.sampling_factor[c].vertical) for c in range(n)]
    return dict(segments=geo[0], ri=geo[2], interleaved=bool(p.interleaved) and n > 1, samp=samp,
                blocks=[(geo[4 + 4 * c] // 8, geo[5 + 4 * c] // 8) for c in range(n)], scan_segments=[geo[6 + 4 * c] for c in range(n)])


def expected_work(geo, reg, out_pf):
    """(segments with a block / an MCU in the cover per scan, blocks of the cover) -- by walking every block of every segment"""
    X, Y, W, H = reg
    Wr = (W + 1) & ~1 if out_pf == 3 else W  # (packed 4:2:2 reads the samples of whole pixel pairs)
    mh, mv = max(s[0] for s in geo["samp"]), max(s[1] for s in geo["samp"])
    cover = []
    for (sh, sv), (bx, by) in zip(geo["samp"], geo["blocks"]):
        if geo["interleaved"]:
            x0, x1 = X // (8 * mh) * sh, ((X + Wr - 1) // (8 * mh) + 1) * sh
            y0, y1 = Y // (8 * mv) * sv, ((Y + H - 1) // (8 * mv) + 1) * sv
        else:
            x0, x1 = X // (mh // sh) // 8, (X + Wr - 1) // (mh // sh) // 8 + 1
            y0, y1 = Y // (mv // sv) // 8, (Y + H - 1) // (mv // sv) // 8 + 1
        cover.append((x0, min(x1, bx), y0, min(y1, by)))
    blocks = sum((x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in cover)
    ri = geo["ri"]
    per_scan = []
    if geo["interleaved"]:  # one scan of MCUs; an MCU is in the cover when its first component's blocks are
        sh, sv = geo["samp"][0]
        mx, my = geo["blocks"][0][0] // sh, geo["blocks"][0][1] // sv
        x0, x1, y0, y1 = cover[0]
        inside = [x0 <= (m % mx) * sh < x1 and y0 <= (m // mx) * sv < y1 for m in range(mx * my)]
        per_scan.append(sum(any(inside[a:a + ri]) for a in range(0, mx * my, ri)) if ri > 0 else 1)
    else:
        for (bx, by), (x0, x1, y0, y1) in zip(geo["blocks"], cover):
            inside = [x0 <= k % bx < x1 and y0 <= k // bx < y1 for k in range(bx * by)]
            per_scan.append(sum(any(inside[a:a + ri]) for a in range(0, bx * by, ri)) if ri > 0 else 1)
    return per_scan, blocks


def check_stats(G, lib, dec, jpeg, reg, out_pf, mode=1):
    geo = stream_geometry(G, lib, jpeg)
    per_scan, blocks = expected_work(geo, reg, out_pf)
    st = dec.region_stats()
    if geo["ri"] <= 0:
        mode = 2
    assert st[0] == mode and st[2] == blocks and st[3] == geo["segments"], (st, per_scan, blocks, geo["segments"])
    assert st[1] == (sum(per_scan) if mode == 1 else geo["segments"]), (st, per_scan)
    return per_scan, geo


# ================================================================================================ 1. the option
def test_option_values(O, G, dlib):
    jpeg = case_stream(O, CASES[0])
    full = O.decode(jpeg)
    dec = G.Decoder(dlib)
    for good in ("0,0,64,64", "5,7,9,11", "full", "63,63,1,1", "3,1,8,8"):
        assert dec.set_option(OPT, good) == 0, good
    for bad in ("", "1,2,3", "1,2,3,4,5", "-1,0,4,4", "0,0,0,4", "0,0,4,0", "a,b,c,d", "1, 2,3,4", "1,2,3,4 ", "0x1,0,4,4", "1.5,0,4,4", "Full", "1,2,,4", ",1,2,3",
                "99999999999,0,1,1"):
        assert dec.set_option(OPT, bad) != 0, bad
    px, pi = dec.decode(jpeg)  # the refused values left 3,1,8,8 in force
    assert (pi.width, pi.height) == (8, 8) and np.array_equal(px, crop(full[0], 64, 64, 1, (3, 1, 8, 8)))
    assert dec.region_stats()[0] == 1
    assert dec.set_option(OPT, "full") == 0
    px, pi = dec.decode(jpeg)
    assert (pi.width, pi.height) == (64, 64) and np.array_equal(px, full[0]) and dec.region_stats()[0] == 0
    dec.close()


def test_image_info_keeps_the_streams_size(O, G, dlib):
    jpeg = case_stream(O, CASES[1])
    dec = G.Decoder(dlib)
    assert dec.set_option(OPT, "8,8,16,16") == 0
    dec.decode(jpeg)
    pi, p = G.ImageParameters(), G.Parameters()
    assert dlib.L.gpujpeg_decoder_get_image_info(jpeg.ctypes.data_as(C.c_void_p), jpeg.size, C.byref(pi), C.byref(p), None) == 0
    assert (pi.width, pi.height) == (640, 368)
    dec.close()


# ================================================================================================ 2. every configuration
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cases_and_regions(O, G, dlib, case):
    """every configuration x the issue's regions, on ONE decoder (the calls after the first launch on the cached header where the stream allows):
    pixels, parameters, sizes, and the work the call reports"""
    jpeg = case_stream(O, case)
    full = O.decode(jpeg, case[3], case[4])
    dec = G.Decoder(dlib)
    for reg in regions(case[1], case[2], case[3]):
        check(O, G, dlib, jpeg, case[3], case[4], reg, dec, full)
        check_stats(G, dlib, dec, jpeg, reg, case[3])
    dec.close()


@pytest.mark.parametrize("name,pf,cs", [("rgb_to_420_il", 2, 3), ("rgb_to_420_il", 0, 3), ("rgb_to_422_nonil", 6, 1), ("uyvy_422_il_q90", 1, 1),
                                        ("planar420_in", 1, 1), ("rgb_natural_auto", 5, 3), ("rgb_natural_auto", 3, 3), ("rgb_natural_auto", 4, 3),
                                        ("gray", 1, 1)])
def test_requested_output_formats(O, G, dlib, name, pf, cs):
    """formats with independent pixels take odd rectangles of subsampled / interleaved streams; subsampled output of 4:4:4 streams on its grid"""
    case = case_named(name)
    jpeg = case_stream(O, case)
    full = O.decode(jpeg, pf, cs)
    dec = G.Decoder(dlib)
    for reg in regions(case[1], case[2], pf):
        check(O, G, dlib, jpeg, pf, cs, reg, dec, full)
        check_stats(G, dlib, dec, jpeg, reg, pf)
    dec.close()


def test_custom_host_buffer_and_alignment(O, G, dlib):
    jpeg = case_stream(O, case_named("rgb_odd_noise"))
    raw, img = O.decode(jpeg)
    reg = (31, 17, 45, 23)
    want = crop(raw, 119, 61, 1, reg)
    dec = G.Decoder(dlib)
    assert dec.set_option(OPT, opt_value(reg)) == 0
    buf = np.full(want.size + 64, 0xA5, np.uint8)
    out = G.DecoderOutput()
    out.type, out.data = G.DECODER_OUTPUT_CUSTOM_BUFFER, buf.ctypes.data
    assert dlib.L.gpujpeg_decoder_decode(dec.h, jpeg.ctypes.data, jpeg.size, C.byref(out)) == 0
    assert out.data_size == want.size and (out.param_image.width, out.param_image.height) == (45, 23)
    assert np.array_equal(buf[:want.size], want) and np.all(buf[want.size:] == 0xA5)
    # dec_opt_alignment_bytes pads the REGION's line
    assert dec.set_option("dec_opt_alignment_bytes", "64") == 0
    px, pi = dec.decode(jpeg)
    pitch = 45 * 3 + pi.width_padding
    assert pi.width_padding == -(45 * 3) % 64 and pitch % 64 == 0 and px.size == dlib.image_size(pi) == O.raw_size(45, 23, 1, pi.width_padding)
    assert np.array_equal(px[:23 * pitch].reshape(23, pitch)[:, :45 * 3].reshape(-1), want)
    dec.close()


@pytest.mark.gpu
def test_custom_device_buffer_and_device_stream(O, G, gpu_lib):
    import torch
    jpeg = case_stream(O, case_named("rgb_natural_auto"))
    raw, img = O.decode(jpeg)
    dj = torch.from_numpy(jpeg).cuda()
    for reg in regions(640, 368, 1):
        want = crop(raw, 640, 368, 1, reg)
        d_out = torch.full((want.size + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        dec = G.Decoder(gpu_lib)
        assert dec.set_option(OPT, opt_value(reg)) == 0
        out = G.DecoderOutput()
        out.type, out.data = G.DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, d_out.data_ptr()
        for _ in range(3):  # (a device-resident stream; the later calls launch on the cached header)
            assert gpu_lib.L.gpujpeg_decoder_decode(dec.h, dj.data_ptr(), jpeg.size, C.byref(out)) == 0
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert out.data_size == want.size and np.array_equal(got[:want.size], want) and np.all(got[want.size:] == 0xA5), reg
            check_stats(G, gpu_lib, dec, jpeg, reg, 1)
        assert dec.path_counters()[0] >= 1
        dec.close()


# ================================================================================================ 3. every kernel path
PATH_CASES = ["rgb_natural_auto", "rgb_hdlike_r24", "uyvy_422_il_q90", "rgb_to_420_il"]
PATHS = ["default", "GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS", "GJ_DEC_SEQ", "serial", "unfused", "keep_coefficients", "GPUJPEG_HOST_SCAN", "GJ_DEC_NO_SPEC"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", PATH_CASES)
def test_kernel_paths(O, G, dlib, name, path, monkeypatch):
    """the selection feeds every entropy decoder, on the first call and on the cached header; results are equal across the paths because every
    one of them equals the cropped oracle decode"""
    case = case_named(name)
    jpeg = case_stream(O, case)
    full = O.decode(jpeg, case[3], case[4])
    if path == "serial":
        monkeypatch.setenv("GJ_DEC_ENTROPY", "serial")
    elif path.startswith("G"):
        monkeypatch.setenv(path, "1")
    dec = G.Decoder(dlib)
    if path == "unfused":
        dec.set_fused(0)
    if path == "keep_coefficients":
        dec.keep_coefficients(True)
    regs = regions(case[1], case[2], case[3])
    for rep in range(3):  # (second and third call of one decoder on the same header)
        for reg in regs[:4] if rep else regs:
            check(O, G, dlib, jpeg, case[3], case[4], reg, dec, full)
            check_stats(G, dlib, dec, jpeg, reg, case[3])
    spec = dec.path_counters()[0]
    if path in ("GPUJPEG_HOST_SCAN", "GJ_DEC_NO_SPEC"):
        assert spec == 0
    else:
        assert spec >= 2, "the calls after the first launch on the cached header"
    assert dec.path_counters()[2] == 0
    dec.close()


def perf_decoder(G, lib):
    """a decoder whose calls keep their kernel times (and with them which IDCT side ran: Decoder.idct_path)"""
    dec = G.Decoder(lib)
    p, pi = lib.default_parameters(), lib.default_image_parameters()
    p.perf_stats, p.verbose, pi.width, pi.height = 1, -1, 0, 0
    assert dec.init(p, pi) == 0
    dec.set_output_format(G.CS_DEFAULT, G.PIXFMT_AUTODETECT)
    return dec


@pytest.mark.parametrize("name", ["rgb_natural_auto", "rgb_hdlike_r24", "rgb_odd_noise", "rgb_big_restart", "rgb_bt709", "rgb_internal_rgb"])
def test_token_fed_and_generic_region_kernels_agree(O, G, dlib, name, monkeypatch):
    """three components 4:4:4, non-interleaved scans, packed output: in token mode the region's pixels come from the records and tokens of the
    cover's blocks (k_idct_tok_region_rgb444, IDCT side 4), in plane mode and with set_fused(0) from the cover-sized planes (side 3) -- the same
    bytes, which are the cropped oracle decode; the selection feeds the token decoder as it feeds the others"""
    case = case_named(name)
    jpeg = case_stream(O, case)
    full = O.decode(jpeg)
    monkeypatch.setenv("GJ_DEC_TOKENS", "1")
    tok = perf_decoder(G, dlib)
    monkeypatch.delenv("GJ_DEC_TOKENS")
    monkeypatch.setenv("GJ_DEC_NO_TOKENS", "1")
    pla = perf_decoder(G, dlib)
    monkeypatch.delenv("GJ_DEC_NO_TOKENS")
    gen = perf_decoder(G, dlib)
    gen.set_fused(0)
    w, h = case[1], case[2]
    regs = regions(w, h, 1) + [(5, 3, w - 5, h - 3), (0, 0, w - 3, h - 1)]
    interleaved = bool(case[7])
    for rep in range(2):  # (the second round launches on the cached header)
        for reg in regs:
            a = check(O, G, dlib, jpeg, None, None, reg, tok, full)
            assert tok.idct_path() == (3 if interleaved else 4), "the token-fed region kernel did not run"
            check_stats(G, dlib, tok, jpeg, reg, 1)
            b = check(O, G, dlib, jpeg, None, None, reg, pla, full)
            c = check(O, G, dlib, jpeg, None, None, reg, gen, full)
            assert pla.idct_path() == 3 and gen.idct_path() == 3
            assert np.array_equal(a, b) and np.array_equal(a, c), (rep, reg)
    # token mode, region, then the full frame in token mode: every record the full call reads is its own
    px, _ = decode_region(G, dlib, jpeg, None, None, None, tok)
    assert np.array_equal(px, full[0]) and tok.idct_path() == 0
    for d in (tok, pla, gen):
        d.close()


# ================================================================================================ 4. work actually skipped
def test_interior_rectangle_selects_fewer_segments_in_every_scan(O, G, dlib):
    """rgb_natural_auto: 640 x 368, 12 blocks per segment, 307 segments per scan -- selection by column as well as by row"""
    jpeg = case_stream(O, case_named("rgb_natural_auto"))
    full = O.decode(jpeg)
    dec = G.Decoder(dlib)
    reg = (213, 123, 161, 93)
    check(O, G, dlib, jpeg, None, None, reg, dec, full)
    per_scan, geo = check_stats(G, dlib, dec, jpeg, reg, 1)
    assert geo["ri"] == 12 and geo["scan_segments"] == [307, 307, 307]
    assert all(0 < n < 307 for n in per_scan), per_scan
    rows = (123 + 93 - 1) // 8 - 123 // 8 + 1
    assert all(n < rows * 7 for n in per_scan), "a row-only selection would take the rows' 80 blocks = 7 segments each"
    dec.close()


def test_restart_interval_0_decodes_every_segment(O, G, dlib):
    case = case_named("rgb_restart0")
    jpeg = case_stream(O, case)
    full = O.decode(jpeg)
    dec = G.Decoder(dlib)
    for reg in regions(100, 60, 1):
        check(O, G, dlib, jpeg, None, None, reg, dec, full)
        st = dec.region_stats()
        assert st[0] == 2 and st[1] == st[3] == 3, st
        check_stats(G, dlib, dec, jpeg, reg, 1)
    dec.close()


@pytest.mark.parametrize("name", ["rgb_big_restart", "rgb_hdlike_r24"])
def test_alternating_regions_are_counted_per_call(O, G, dlib, name):
    """one decoder, two regions in turn (A, B, A, B): every call's statistics are its own region's brute-force count -- nothing of the call before
    is kept. rgb_big_restart: 512 x 256, interval 300, a segment spans more than four block rows; rgb_hdlike_r24: segments wrap row ends.
    A: an interior rectangle, all four numbers odd; B: a full-height strip narrower than a block -- their selections differ in every scan"""
    case = case_named(name)
    jpeg = case_stream(O, case)
    full = O.decode(jpeg)
    w, h = case[1], case[2]
    a, b = ((w // 3) | 1, (h // 3) | 1, (w // 4) | 1, (h // 4) | 1), ((w // 2) | 1, 0, 5, h)
    assert all(v % 2 == 1 for v in a) and b[2] < 8 and b[3] == h
    geo = stream_geometry(G, dlib, jpeg)
    scans_a, scans_b = expected_work(geo, a, 1)[0], expected_work(geo, b, 1)[0]
    assert geo["ri"] > 0 and len(scans_a) == 3 and all(x != y for x, y in zip(scans_a, scans_b)), (scans_a, scans_b)
    dec = G.Decoder(dlib)
    for reg in (a, b, a, b):
        check(O, G, dlib, jpeg, None, None, reg, dec, full)
        per_scan, _ = check_stats(G, dlib, dec, jpeg, reg, 1)  # (mode 1, the sum of the brute-force count, the cover's blocks)
        assert per_scan == (scans_a if reg == a else scans_b)
    dec.close()


def test_cover_planes_after_a_region_call(O, G, dlib):
    """gpujpeg_amd_decoder_read_planes after a region call: the cover-sized component planes = the crop of the oracle's planes at the cover"""
    jpeg = case_stream(O, case_named("rgb_to_422_nonil"))
    st = O.parse(jpeg)
    planes = O.idct(st, O.huffman_decode(st, jpeg))
    O.lib().gjo_stream_free(C.byref(st))
    dec = G.Decoder(dlib)
    reg = (37, 21, 50, 30)
    check(O, G, dlib, jpeg, None, None, reg, dec)
    geo = stream_geometry(G, dlib, jpeg)
    want, off = [], 0
    for (sh, sv), (bx, by) in zip(geo["samp"], geo["blocks"]):
        sub = 2 // sh
        x0, x1, y0, y1 = 37 // sub // 8, (37 + 49) // sub // 8 + 1, 21 // 8, (21 + 29) // 8 + 1
        want.append(planes[off:off + bx * by * 64].reshape(by * 8, bx * 8)[y0 * 8:y1 * 8, x0 * 8:x1 * 8].reshape(-1))
        off += bx * by * 64
    want = np.concatenate(want)
    assert np.array_equal(dec.planes(want.size), want)
    dec.close()


# ================================================================================================ 5. state between calls
def sequence_body(O, G, lib, keep_switch=False):
    a = case_named("rgb_natural_auto")
    b = case_named("rgb_hdlike_r24")
    ja, jb = case_stream(O, a), case_stream(O, b)
    ja2 = O.encode(oracle_image(O, a), natural_image(640, 368, 3, seed=77))  # (another frame with the same header)
    fa, fa2, fb = O.decode(ja), O.decode(ja2), O.decode(jb)
    A, B = (40, 24, 100, 60), (401, 201, 199, 131)
    dec = G.Decoder(lib)
    steps = [(ja, fa, A), (ja2, fa2, None), (ja, fa, B), (jb, fb, None), (ja2, fa2, A), (ja, fa, None), (jb, fb, (100, 50, 33, 21)), (jb, fb, None)]
    for i, (jpeg, full, reg) in enumerate(steps):
        if keep_switch:
            dec.keep_coefficients(i % 2 == 1)
        if reg is None:
            px, pi = decode_region(G, lib, jpeg, None, None, None, dec)
            assert np.array_equal(px, full[0]) and (pi.width, pi.height) == (full[1].width, full[1].height), i
            assert dec.region_stats()[0] == 0
        else:
            check(O, G, lib, jpeg, None, None, reg, dec, full)
            check_stats(G, lib, dec, jpeg, reg, 1)
    dec.close()


@pytest.mark.parametrize("mode", ["GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS", "GJ_DEC_SEQ", "serial", "keep_switch"])
def test_state_between_calls(O, G, dlib, mode, monkeypatch):
    """region A, full frame, region B elsewhere, another stream of another size full, region A again, ...: no call trusts the coefficient planes or
    the block records an earlier region call left outside its selection"""
    if mode == "serial":
        monkeypatch.setenv("GJ_DEC_ENTROPY", "serial")
    elif mode != "keep_switch":
        monkeypatch.setenv(mode, "1")
    sequence_body(O, G, dlib, keep_switch=mode == "keep_switch")


@pytest.mark.parametrize("name", ["rgb_hdlike_r24", "gray", "rgba_4444", "planar444_in"])
def test_channel_remap_on_the_region(O, G, dlib, name):
    case = case_named(name)
    jpeg = case_stream(O, case)
    raw, img = O.decode(jpeg, case[3], case[4])
    mapping = {0: "0", 6: "2103"}.get(case[3], "210")
    remapped = O.channel_remap(img, raw, mapping)
    dec = G.Decoder(dlib)
    assert dec.set_option("dec_opt_channel_remap", mapping) == 0
    for reg in regions(case[1], case[2], case[3])[:4]:
        check(O, G, dlib, jpeg, case[3], case[4], reg, dec, (remapped, img))
    dec.close()


# ================================================================================================ 6. damaged streams
def damaged_restart_markers(jpeg, seed=8):
    """one damaged restart marker per stream, made the way kind 8 of tools/fuzz_decoder.py makes them: renumbered, removed, doubled.
    -> [(kind, stream, ordinal of the marker among the stream's restart markers)]"""
    rng = np.random.default_rng(seed)
    r = np.nonzero((jpeg[:-1] == 0xFF) & (jpeg[1:] >= 0xD0) & (jpeg[1:] <= 0xD7))[0]
    out = []
    for op, kind in enumerate(("renumbered", "removed", "doubled")):
        bad = jpeg.copy()
        n = int(rng.integers(r.size // 4, r.size // 2))
        i = int(r[n])
        if op == 0:
            bad[i + 1] = 0xD0 + (int(bad[i + 1]) - 0xD0 + 1 + int(rng.integers(0, 7))) % 8
        elif op == 1:
            bad[i], bad[i + 1] = 0x12, 0x34
        else:
            bad[i + 2:i + 4] = bad[i:i + 2]
        out.append((kind, bad, n))
    return out


def raw_call(G, lib, dec, data):
    out = G.DecoderOutput()
    out.type = G.DECODER_OUTPUT_INTERNAL_BUFFER
    data = np.ascontiguousarray(data)
    rc = lib.L.gpujpeg_decoder_decode(dec.h, data.ctypes.data, data.size, C.byref(out))
    px = np.frombuffer((C.c_uint8 * out.data_size).from_address(out.data), np.uint8).copy() if rc == 0 else None
    return rc, px


def test_damaged_restart_markers(O, G, dlib):
    """the region call returns what the full call returns; where that is 0, its pixels are the crop of the product's own full decode of the damaged
    stream outside the blocks of the two restart segments next to the damaged marker (what a decoder emits once a segment's data has run out is
    garbage in every decoder); afterwards the decoder decodes the intact stream as ever"""
    jpeg = case_stream(O, case_named("rgb_natural_auto"))
    good = O.decode(jpeg)[0]
    reg = (160, 40, 320, 280)  # 40 x 35 block positions
    good_crop = crop(good, 640, 368, 1, reg)
    for kind, bad, n in damaged_restart_markers(jpeg):
        fd, rd = G.Decoder(dlib), G.Decoder(dlib)
        rc_full, px_full = raw_call(G, dlib, fd, bad)
        assert rd.set_option(OPT, opt_value(reg)) == 0
        rc, px = raw_call(G, dlib, rd, bad)
        assert (rc == 0) == (rc_full == 0), (kind, rc_full, rc)
        if rc == 0:
            st = rd.region_stats()
            # the rule: a table with fewer entries than the geometry has segments (a removed marker: the host walk merged two segments) -> every
            # segment is entropy-decoded; a host walk that found every segment still selects -- each entry is judged by its own geometric index
            assert st[0] == (1 if st[3] == 921 else 2), (kind, st)
            if kind == "removed":
                assert st[3] < 921 and st[0] == 2, (kind, st)
            # restart marker n of the stream ends segment n_in_scan of scan n // 306 (307 segments, 306 markers per scan)
            k = n % 306
            mask = np.ones((368 // 8, 640 // 8), bool)
            for b in range(k * 12, min((k + 2) * 12, 80 * 46)):
                mask[b // 80, b % 80] = False
            inside = mask[reg[1] // 8:(reg[1] + reg[3]) // 8, reg[0] // 8:(reg[0] + reg[2]) // 8]
            assert np.count_nonzero(inside) >= 10 * np.count_nonzero(~inside)
            pm = np.repeat(np.repeat(mask, 8, 0), 8, 1)[reg[1]:reg[1] + reg[3], reg[0]:reg[0] + reg[2]]
            want = crop(px_full, 640, 368, 1, reg).reshape(reg[3], reg[2], 3)
            got = px.reshape(reg[3], reg[2], 3)
            assert np.array_equal(got[pm], want[pm]), (kind, int(np.count_nonzero(got[pm] != want[pm])))
        px2, _ = rd.decode(jpeg)
        assert np.array_equal(px2, good_crop), kind
        for d in (fd, rd):
            d.close()


def test_truncated_and_flipped_streams_do_not_fault(O, G, dlib):
    jpeg = case_stream(O, case_named("rgb_natural_auto"))
    good = crop(O.decode(jpeg)[0], 640, 368, 1, (213, 123, 161, 93))
    flipped = jpeg.copy()
    i = jpeg.size // 2
    while flipped[i] == 0xFF or flipped[i - 1] == 0xFF or flipped[i + 1] == 0xFF:
        i += 1
    flipped[i] ^= 0x5A
    if flipped[i] == 0xFF:
        flipped[i] = 0x11
    for bad in (jpeg[:jpeg.size * 2 // 3].copy(), flipped):
        fd, rd = G.Decoder(dlib), G.Decoder(dlib)
        assert rd.set_option(OPT, "213,123,161,93") == 0
        rc_full, _ = raw_call(G, dlib, fd, bad)
        rc, _ = raw_call(G, dlib, rd, bad)
        assert (rc == 0) == (rc_full == 0)
        assert np.array_equal(rd.decode(jpeg)[0], good)
        fd.close()
        rd.close()


# ================================================================================================ 7. refusals
def test_refusals_leave_the_decoder_usable(O, G, dlib):
    jpeg = case_stream(O, case_named("rgb_natural_auto"))
    raw, img = O.decode(jpeg)
    dec = G.Decoder(dlib)
    ok = (11, 13, 37, 41)
    for bad in ((640, 0, 1, 1), (0, 368, 1, 1), (600, 0, 41, 8), (0, 360, 8, 9), (0, 0, 641, 368), (100000, 5, 5, 5)):
        assert dec.set_option(OPT, opt_value(bad)) == 0
        with pytest.raises(RuntimeError):
            dec.decode(jpeg)
        check(O, G, dlib, jpeg, None, None, ok, dec, (raw, img))
    dec.close()
    # misaligned on the three subsampled output formats; the edge exemption
    for pf, bads, goods in ((3, [(1, 0, 8, 8), (0, 0, 7, 8)], [(0, 1, 8, 7), (632, 3, 8, 5)]),
                            (4, [(3, 0, 8, 8), (2, 0, 5, 8)], [(2, 1, 6, 7)]),
                            (5, [(1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 7, 8), (0, 0, 8, 7)], [(2, 2, 6, 6), (630, 360, 10, 8)])):
        full = O.decode(jpeg, pf, 3)
        dec = G.Decoder(dlib)
        for bad in bads:
            dec.set_output_format(3, pf)
            assert dec.set_option(OPT, opt_value(bad)) == 0
            with pytest.raises(RuntimeError):
                dec.decode(jpeg)
            check(O, G, dlib, jpeg, pf, 3, goods[0], dec, full)
        for good in goods:
            check(O, G, dlib, jpeg, pf, 3, good, dec, full)
        dec.close()
    # odd image: a region that ends at the right / bottom edge may have an odd size
    case = case_named("planar420_in")
    j2 = case_stream(O, case)
    jo = O.encode(oracle_image(O, ("odd420", 161, 121, 5, 3, 75, 6, 0, None, 3)), O.noise(O.raw_size(161, 121, 5), seed=5))
    check(O, G, dlib, jo, 5, 3, (150, 110, 11, 11))
    check(O, G, dlib, j2, 5, 3, (150, 110, 12, 12))
    # with a flip, with a scale
    dec = G.Decoder(dlib)
    assert dec.set_option(OPT, opt_value(ok)) == 0
    assert dec.set_option("dec_opt_flipped", "1") == 0
    with pytest.raises(RuntimeError):
        dec.decode(jpeg)
    assert dec.set_option("dec_opt_flipped", "0") == 0
    check(O, G, dlib, jpeg, None, None, ok, dec, (raw, img))
    assert dec.set_option("dec_opt_scale", "1/2") == 0
    with pytest.raises(RuntimeError):
        dec.decode(jpeg)
    assert dec.set_option("dec_opt_scale", "1") == 0
    check(O, G, dlib, jpeg, None, None, ok, dec, (raw, img))
    dec.close()


# ================================================================================================ 8. batch calls and the tool
def test_batch_calls_equal_frame_at_a_time(O, G, dlib):
    case = case_named("rgb_hdlike_r24")
    w, h = case[1], case[2]
    streams = [O.encode(oracle_image(O, case), natural_image(w, h, 3, seed=20 + f)) for f in range(5)]
    reg = (101, 33, 211, 97)
    want = [crop(O.decode(x)[0], w, h, 1, reg) for x in streams]
    dec = G.Decoder(dlib)
    dec.set_batch_chunk(2)
    assert dec.set_option(OPT, opt_value(reg)) == 0
    for rep in range(2):
        got, pi = dec.decode_batch(streams)
        assert (pi.width, pi.height) == (211, 97) and dec.last_batch() == (0, 5)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), rep
    got, pi = dec.decode_batch_ptrs(streams, want[0].size)  # room for exactly a region image
    assert (pi.width, pi.height) == (211, 97) and all(np.array_equal(a, b) for a, b in zip(got, want)) and dec.last_batch() == (0, 5)
    assert dec.set_option(OPT, "full") == 0  # and back: the batched launches
    got, pi = dec.decode_batch(streams)
    assert (pi.width, pi.height) == (w, h) and all(np.array_equal(a, O.decode(x)[0]) for a, x in zip(got, streams))
    dec.close()


@pytest.mark.gpu
def test_cli_region_decode(O, G, gpu_lib, tmp_path):
    tool = os.path.join(os.path.dirname(G.PRODUCT_LIB), "gpujpegtool")
    jpeg = case_stream(O, case_named("rgb_odd_noise"))
    src, dst = tmp_path / "in.jpg", tmp_path / "out.pnm"
    jpeg.tofile(src)
    r = subprocess.run([tool, "-d", "-O", "dec_opt_region=31,17,45,23", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = dst.read_bytes()
    m = re.match(rb"P6\s+(\d+)\s+(\d+)\s+(\d+)\s", data)
    assert m and tuple(int(x) for x in m.groups()) == (45, 23, 255), data[:32]
    assert np.array_equal(np.frombuffer(data[m.end():], np.uint8), crop(O.decode(jpeg)[0], 119, 61, 1, (31, 17, 45, 23)))
    assert OPT in subprocess.run([tool, "-O", "help"], capture_output=True, text=True, timeout=60).stdout


# ================================================================================================ 9. random differential
def random_region(rng, w, h, pf):
    ah, av = GRID.get(pf, (1, 1))
    x, y = int(rng.integers(0, w)) // ah * ah, int(rng.integers(0, h)) // av * av
    W, H = int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))
    if W % ah and x + W != w:
        W += 1
    if H % av and y + H != h:
        H += 1
    return (x, y, W, H)


@pytest.mark.parametrize("seed", range(40))
def test_random_configurations(O, G, emu, seed):
    case = random_case(seed)
    jpeg = O.encode(oracle_image(O, case), random_raw(O, case, seed))
    full = O.decode(jpeg, case[3], case[4])
    rng = np.random.default_rng(6000 + seed)
    dec = G.Decoder(emu)
    for _ in range(3):
        reg = random_region(rng, case[1], case[2], case[3])
        check(O, G, emu, jpeg, case[3], case[4], reg, dec, full)
        check_stats(G, emu, dec, jpeg, reg, case[3])
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(3840, 2160), (7680, 4320)])
def test_large_natural_frames(O, G, gpu_lib, w, h):
    """frames for which token mode opens by itself without the option: five regions each, and the full frame in between"""
    jpeg = O.encode(oracle_image(O, ("rgb_large", w, h, 1, 1, 75, -1, 0, None, 3)), natural_image(w, h, 3, seed=9))
    full = O.decode(jpeg)
    rng = np.random.default_rng(w)
    dec = perf_decoder(G, gpu_lib)
    regs = [(w // 2 - 256 - 1, h // 2 - 256 - 1, 512, 512), (0, h // 2, w, 64), (w // 2, 0, 64, h)] + [random_region(rng, w, h, 1) for _ in range(2)]
    for i, reg in enumerate(regs):
        check(O, G, gpu_lib, jpeg, None, None, reg, dec, full)
        per_scan, geo = check_stats(G, gpu_lib, dec, jpeg, reg, 1)
        assert dec.idct_path() == 4, "the token gate opens by itself for a frame of this size: the token-fed region kernel"
        if i == 0:  # selection by column: 66 block columns cross at most ceil(66 / ri) + 1 segments in each of the cover's 65 or 66 block rows
            ri, bx = geo["ri"], geo["blocks"][0][0]
            assert all(n <= 66 * (-(-66 // ri) + 1) < 65 * (bx // ri) for n in per_scan), (per_scan, ri, bx)
        if i == 2:
            px, _ = decode_region(G, gpu_lib, jpeg, None, None, None, dec)
            assert np.array_equal(px, full[0])
    dec.close()


# ================================================================================================ sanitizers
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
    """this file's CPU-tier tests once more on the AddressSanitizer + UBSan build of the execution model (every geometry and the damaged streams
    through the selection, the cover-sized planes and the region buffers)"""
    env = dict(asan_env, GJ_EMU_LIB=ASAN_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-n", "4", "-m", "not gpu", "-p", "no:faulthandler",
                        "-p", "no:cacheprovider", "-k", "not under_sanitizers"], capture_output=True, text=True, errors="replace",
                       timeout=1500, env=env, cwd=ROOT)
    tail = (r.stdout[-1500:] + "\n" + "\n".join(ln for ln in r.stderr.splitlines() if not ln.startswith("[GPUJPEG]"))[-3000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1500:]
