"""Reduced-size decode (decoder option dec_opt_scale = 1/2, 1/4, 1/8; gpujpeg_amd_ext.h).

The reference has no reduced decode, so the mode is outside reference parity by construction. It is pinned by a restatement that uses no
product code: the oracle (pinned to the reference by the other suites) parses the stream and decodes its coefficients; the definition -- an
integer N-point inverse DCT of every block's N x N low-frequency corner, N = 8 / s, restated below in numpy -- gives the reduced component
planes; the oracle's postprocessor makes the pixels of the ceil(W / s) x ceil(H / s) image out of them. Expected and decoded buffers are
compared byte for byte.

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu (own fixture, as tests/test_huffman_optimal.py), the
-m gpu tier the product library on the MI355X. One test re-runs the CPU tier on the AddressSanitizer + UBSan build of the execution model."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import CASES, make_raw, natural_image, oracle_image, psnr, random_case, random_raw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")
ASAN_DIR = os.path.join(EMU_DIR, "_build_asan")
ASAN_LIB = os.path.join(ASAN_DIR, "libgpujpeg_emu.so")
CLANG_RT = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"
CAMERA = os.path.join(HERE, "golden", "camera_bt709_422_q95.jpg")
OPT = "dec_opt_scale"
SCALES = [2, 4, 8]
PF_UYVY = 3


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


# ================================================================================================ restatement: the definition
def k_matrix(N):
    """K[x][u] = k(u) cos((2x + 1) u pi / 2N), k(0) = sqrt(1/8), k(u > 0) = 1/2: the N-point inverse DCT of the corner, a flat block keeps its value"""
    return np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / (2 * N)) for u in range(N)] for x in range(N)])


def m_matrix(N):
    return np.rint(k_matrix(N) * 8192).astype(np.int64)


def test_definition_matrices():
    """the tables as the documents print them"""
    assert m_matrix(1).tolist() == [[2896]]
    assert m_matrix(2).tolist() == [[2896, 2896], [2896, -2896]]
    assert m_matrix(4).tolist() == [[2896, 3784, 2896, 1567], [2896, 1567, -2896, -3784], [2896, -1567, -2896, 3784], [2896, -3784, 2896, -1567]]
    # nothing overflows 32 bits
    row = int(np.abs(m_matrix(4)).sum(1).max())
    assert row == 11143 and row * 32768 < 2 ** 31 and row * ((row * 32768 + 1024) >> 11) + 16384 < 2 ** 31


ZIGZAG = []
for _sd in range(15):
    _cells = [(i, _sd - i) for i in range(_sd + 1) if i < 8 and _sd - i < 8]
    ZIGZAG += _cells if _sd % 2 else _cells[::-1]
NATURAL_FROM_ZIGZAG = np.zeros((8, 8), int)  # [row][column] -> index in zig-zag order
for _i, (_r, _c) in enumerate(ZIGZAG):
    NATURAL_FROM_ZIGZAG[_r, _c] = _i


def corner_blocks(s, coefs, c, N):
    """clamped dequantised corner D[by][bx][v][u] of component c (int64)"""
    k = s.img.comp[c]
    dw, dh, off = k.data_width, k.data_height, k.data_offset
    q = np.array(list(s.qraw[s.qmap[c]]), np.int64)[NATURAL_FROM_ZIGZAG]
    B = np.asarray(coefs[off:off + dw * dh]).reshape(dh // 8, dw // 8, 8, 8).astype(np.int64)
    return np.clip(B * q, -32768, 32767)[:, :, :N, :N]


def reduced_planes(s, coefs, N):
    """the definition, integer: one (data_height * N / 8) x (data_width * N / 8) plane per component"""
    out, m = [], m_matrix(N)
    for c in range(s.img.comp_count):
        D = corner_blocks(s, coefs, c, N)
        T = (np.einsum("yv,abvu->abyu", m, D) + 1024) >> 11
        S = (np.einsum("abyu,xu->abyx", T, m) + 16384) >> 15
        nby, nbx = D.shape[:2]
        out.append(np.clip(S + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(nby * N, nbx * N))
    return out


def reduced_planes_float(s, coefs, N):
    """the same transform in float64, rounded once at the end"""
    out, K = [], k_matrix(N)
    for c in range(s.img.comp_count):
        D = corner_blocks(s, coefs, c, N).astype(np.float64)
        S = np.einsum("yv,abvu,xu->abyx", K, D, K)
        nby, nbx = D.shape[:2]
        out.append(np.clip(np.rint(S + 128), 0, 255).transpose(0, 2, 1, 3).reshape(nby * N, nbx * N))
    return out


def dims(w, h, s):
    return -(-w // s), -(-h // s)


def expected_from_coefs(O, stream, coefs, s):
    """(pixels, Image) of the reduced image, or (None, None) where the output format has none (packed 4:2:2 of odd width)"""
    N = 8 // s
    W, H = dims(stream.img.width, stream.img.height, s)
    if stream.img.pixel_format == PF_UYVY and W % 2:
        return None, None
    im2 = O.Image.from_buffer_copy(stream.img)
    im2.width, im2.height = W, H
    assert O.lib().gjo_image_init(C.byref(im2)) == 0
    red = reduced_planes(stream, coefs, N)
    planes = np.zeros(im2.data_size, np.uint8)
    for c in range(im2.comp_count):
        k2, r = im2.comp[c], red[c]
        hh, ww = min(k2.data_height, r.shape[0]), min(k2.data_width, r.shape[1])
        assert ww >= k2.width and hh >= k2.height, (c, ww, k2.width, hh, k2.height)  # every sample the pixels ask for is there
        P = np.zeros((k2.data_height, k2.data_width), np.uint8)
        P[:hh, :ww] = r[:hh, :ww]
        planes[k2.data_offset:k2.data_offset + P.size] = P.reshape(-1)
    return O.postprocess(im2, planes), im2


def expected(O, jpeg, pf, cs, s):
    st = O.parse(jpeg, pf, cs)
    try:
        return expected_from_coefs(O, st, O.huffman_decode(st, jpeg), s)
    finally:
        O.lib().gjo_stream_free(C.byref(st))


def decode_scaled(G, lib, jpeg, pf, cs, s, dec=None, **kw):
    """one decode at 1/s with the output format (pf, cs) (None: the decoder's default) -> (pixels, ImageParameters)"""
    own = dec is None
    if own:
        dec = G.Decoder(lib)
    try:
        if pf is not None:
            dec.set_output_format(cs, pf)
        assert dec.set_option(OPT, "1" if s == 1 else f"1/{s}") == 0
        return dec.decode(jpeg, **kw)
    finally:
        if own:
            dec.close()


def check(O, G, lib, jpeg, pf, cs, s, dec=None):
    """the contract of one reduced decode: pixels, returned parameters and size -- or the refusal"""
    want, im2 = expected(O, jpeg, -1 if pf is None else pf, -1 if cs is None else cs, s)
    if want is None:
        with pytest.raises(RuntimeError):
            decode_scaled(G, lib, jpeg, pf, cs, s, dec)
        return None
    px, pi = decode_scaled(G, lib, jpeg, pf, cs, s, dec)
    assert (pi.width, pi.height, pi.pixel_format) == (im2.width, im2.height, im2.pixel_format), (pi.width, pi.height, pi.pixel_format)
    assert px.size == want.size == O.raw_size(im2.width, im2.height, im2.pixel_format) == lib.image_size(pi)
    assert np.array_equal(px, want), (s, int(np.count_nonzero(px != want)), int(np.abs(px.astype(int) - want.astype(int)).max()))
    return px


def case_stream(O, case):
    return O.encode(oracle_image(O, case), make_raw(O, case))


# ================================================================================================ the definition itself (no library)
def test_definition_integer_against_float(O):
    """max |integer - round(float64)| <= 1 level over all CASES at every scale: the first pass keeps two fraction bits and the table entries are
    off by < 0.5 / 8192, so with legal coefficients the integer result stays within half a level of the exact one before its own final rounding"""
    worst = 0
    for case in CASES:
        jpeg = case_stream(O, case)
        st = O.parse(jpeg, case[3], case[4])
        coefs = O.huffman_decode(st, jpeg)
        for s in SCALES:
            for a, b in zip(reduced_planes(st, coefs, 8 // s), reduced_planes_float(st, coefs, 8 // s)):
                worst = max(worst, int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()))
        O.lib().gjo_stream_free(C.byref(st))
    print("max |integer - round(float64)| =", worst)
    assert worst <= 1


PSNR_CASES = [c for c in CASES if c[0] in ("rgb_natural_auto", "rgb_hdlike_r24", "rgb_big_restart")] + [("gray_natural", 640, 368, 0, 3, 75, -1, 0, None, 3)]


@pytest.mark.parametrize("case", PSNR_CASES, ids=[c[0] for c in PSNR_CASES])
def test_definition_orientation_psnr(O, case):
    """The reduced image is the box average of the ORACLE's full-size decode to >= 40 dB at every scale (natural images, q75). 40 lies between the
    46.6 dB minimum the definition reaches and the <= 35 dB a transposed or zig-zag-ordered corner gives: it guards the definition's orientation."""
    name, w, h, pf, cs = case[:5]
    comps = 1 if pf == 0 else 3
    raw = natural_image(w, h, comps, seed=len(name)) if name == "gray_natural" else make_raw(O, case)
    jpeg = O.encode(oracle_image(O, case), raw)
    full = O.decode(jpeg, pf, cs)[0].reshape(h, w, comps).astype(np.float64)
    for s in SCALES:
        W, H = dims(w, h, s)
        assert W * s == w and H * s == h
        want, _ = expected(O, jpeg, pf, cs, s)
        box = full.reshape(H, s, W, s, comps).mean((1, 3))
        p = psnr(want.reshape(H, W, comps), box)
        print(name, f"1/{s}", f"{p:.1f} dB")
        assert p >= 40.0, (name, s, p)


# ================================================================================================ every case x every scale
UYVY_EVEN = ("uyvy_even_320x48", 320, 48, 3, 3, 90, -1, 1, None, 3)  # packed 4:2:2 with an even reduced width at every scale (CASES has odd ones only)


@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
@pytest.mark.parametrize("case", CASES + [UYVY_EVEN], ids=[c[0] for c in CASES + [UYVY_EVEN]])
def test_cases_at_every_scale(O, G, dlib, case, s):
    """output format = the case's own pixel format and colour space, as in the parity suites; packed 4:2:2 of odd reduced width is refused"""
    name, w, h, pf, cs = case[:5]
    jpeg = case_stream(O, case)
    W, _ = dims(w, h, s)
    got = check(O, G, dlib, jpeg, pf, cs, s)
    assert (got is None) == (pf == PF_UYVY and W % 2 == 1)


@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
def test_default_output_format_and_camera_fixture(O, G, dlib, s):
    """the decoder's default output (RGB) of a 4:2:0 stream, a gray stream and the camera fixture (BT.709 4:2:2, q95)"""
    for case in [c for c in CASES if c[0] in ("rgb_to_420_il", "gray", "rgb_natural_auto")]:
        check(O, G, dlib, case_stream(O, case), None, None, s)
    check(O, G, dlib, np.fromfile(CAMERA, np.uint8), None, None, s)


@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
def test_requested_output_formats(O, G, dlib, s):
    """a 4:2:0 stream as packed RGB, planar 4:2:0, planar 4:4:4 and luma only; a gray stream as RGB"""
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_to_420_il"][0])
    for pf, cs in ((1, 1), (5, 3), (2, 3), (0, 3)):
        check(O, G, dlib, jpeg, pf, cs, s)
    check(O, G, dlib, case_stream(O, [c for c in CASES if c[0] == "gray"][0]), 1, 1, s)


@pytest.mark.parametrize("seed", range(40))
def test_random_configurations(O, G, dlib, seed):
    case = random_case(seed)
    s = int(np.random.default_rng(4000 + seed).choice(SCALES))
    jpeg = O.encode(oracle_image(O, case), random_raw(O, case, seed))
    check(O, G, dlib, jpeg, case[3], case[4], s)


# ================================================================================================ the two IDCT sides give the same bytes
def perf_decoder(G, lib):
    """a decoder whose calls keep their kernel times (and with them which IDCT side ran)"""
    dec = G.Decoder(lib)
    p, pi = lib.default_parameters(), lib.default_image_parameters()
    p.perf_stats, p.verbose, pi.width, pi.height = 1, -1, 0, 0
    assert dec.init(p, pi) == 0
    dec.set_output_format(G.CS_DEFAULT, G.PIXFMT_AUTODETECT)
    return dec


def paths_body(O, G, lib, jpeg, monkeypatch, gate_opens=False):
    want = {s: expected(O, jpeg, -1, -1, s)[0] for s in SCALES}
    for k in ("GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS"):
        monkeypatch.delenv(k, raising=False)
    st = O.parse(jpeg)
    coefs = O.huffman_decode(st, jpeg)
    # default path and generic kernels
    dec, gen = perf_decoder(G, lib), perf_decoder(G, lib)
    gen.set_fused(0)
    for s in SCALES:
        a = decode_scaled(G, lib, jpeg, None, None, s, dec)[0]
        if gate_opens:
            assert dec.idct_path() == 2, "the token gate opens by itself for a frame of this size"
        b = decode_scaled(G, lib, jpeg, None, None, s, gen)[0]
        assert gen.idct_path() == 1
        assert np.array_equal(a, want[s]) and np.array_equal(b, want[s]), s
        # the reduced component planes of the generic path, component after component
        red = np.concatenate([p.reshape(-1) for p in reduced_planes(st, coefs, 8 // s)])
        assert np.array_equal(gen.planes(red.size), red), s
    dec.close()
    gen.close()
    O.lib().gjo_stream_free(C.byref(st))
    # token-fed kernel forced / forbidden (the settings are taken when a decoder is created)
    monkeypatch.setenv("GJ_DEC_TOKENS", "1")
    tok = perf_decoder(G, lib)
    monkeypatch.delenv("GJ_DEC_TOKENS")
    monkeypatch.setenv("GJ_DEC_NO_TOKENS", "1")
    pla = perf_decoder(G, lib)
    monkeypatch.delenv("GJ_DEC_NO_TOKENS")
    for rep in range(2):  # (the second round launches on the cached header)
        for s in SCALES:
            a = decode_scaled(G, lib, jpeg, None, None, s, tok)[0]
            assert tok.idct_path() == 2, "the token-fed reduced-size kernel did not run"
            b = decode_scaled(G, lib, jpeg, None, None, s, pla)[0]
            assert pla.idct_path() == 1
            assert np.array_equal(a, b) and np.array_equal(a, want[s]), (rep, s)
    tok.close()
    pla.close()


@pytest.mark.parametrize("name", ["rgb_natural_auto", "rgb_big_restart"])
def test_generic_and_token_fed_kernels_agree(O, G, dlib, name, monkeypatch):
    """set_fused(0) == default path, GJ_DEC_TOKENS=1 == GJ_DEC_NO_TOKENS, byte for byte; the forced case really ran the token-fed kernel"""
    paths_body(O, G, dlib, case_stream(O, [c for c in CASES if c[0] == name][0]), monkeypatch)


@pytest.mark.gpu
def test_generic_and_token_fed_kernels_agree_4k(O, G, gpu_lib, monkeypatch):
    """a 4:4:4 frame of 388 800 blocks: the token gate opens by itself"""
    w, h = 3840, 2160
    jpeg = O.encode(oracle_image(O, ("rgb_4k", w, h, 1, 1, 75, -1, 0, None, 3)), natural_image(w, h, 3, seed=9))
    paths_body(O, G, gpu_lib, jpeg, monkeypatch, gate_opens=True)


def test_odd_sizes_through_the_token_fed_kernel(O, G, dlib, monkeypatch):
    """block rows that are no multiple of a wave, partial blocks on both edges, width padding: the dword stores and the byte-wise edges"""
    monkeypatch.setenv("GJ_DEC_TOKENS", "1")
    for w, h, q, ri in ((1119, 77, 90, 12), (517, 40, 75, 3), (8, 8, 75, 4), (1031, 17, 50, -1)):
        jpeg = O.encode(oracle_image(O, ("odd", w, h, 1, 1, q, ri, 0, None, 3)), natural_image(w, h, 3, seed=w))
        dec = perf_decoder(G, dlib)
        for s in SCALES:
            check(O, G, dlib, jpeg, None, None, s, dec)
            assert dec.idct_path() == 2
        dec.close()


# ================================================================================================ the option
def test_scale_changes_between_calls_of_one_decoder(O, G, dlib):
    """scale 1 -> 1/4 -> 1 -> 1/8 on one decoder and one stream: neither the header cache nor the speculative launch keeps a stale scale"""
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_natural_auto"][0])
    fresh = G.Decoder(dlib)
    full = fresh.decode(jpeg)[0]
    fresh.close()
    assert np.array_equal(full, O.decode(jpeg)[0])
    dec = G.Decoder(dlib)
    for s in (1, 4, 1, 8):
        if s == 1:
            px, pi = decode_scaled(G, dlib, jpeg, None, None, 1, dec)
            assert np.array_equal(px, full) and (pi.width, pi.height) == (640, 368)
        else:
            check(O, G, dlib, jpeg, None, None, s, dec)
    assert dec.path_counters()[0] >= 1  # (calls on the cached header took part)
    dec.close()


def test_invalid_values_leave_the_scale_unchanged(O, G, dlib):
    jpeg = case_stream(O, CASES[0])
    dec = G.Decoder(dlib)
    assert dec.set_option(OPT, "1/4") == 0
    for bad in ("1/3", "0", "2", ""):
        assert dec.set_option(OPT, bad) != 0, bad
    px, pi = dec.decode(jpeg)
    assert (pi.width, pi.height) == (16, 16) and np.array_equal(px, expected(O, jpeg, -1, -1, 4)[0])
    assert dec.set_option(OPT, "1") == 0
    assert np.array_equal(dec.decode(jpeg)[0], O.decode(jpeg)[0])
    dec.close()


def test_image_info_keeps_the_streams_size(O, G, dlib):
    jpeg = case_stream(O, CASES[1])
    dec = G.Decoder(dlib)
    assert dec.set_option(OPT, "1/8") == 0
    dec.decode(jpeg)
    pi, p = G.ImageParameters(), G.Parameters()
    assert dlib.L.gpujpeg_decoder_get_image_info(jpeg.ctypes.data_as(C.c_void_p), jpeg.size, C.byref(pi), C.byref(p), None) == 0
    assert (pi.width, pi.height) == (640, 368)
    dec.close()


def test_channel_remap_and_flip(O, G, dlib):
    """dec_opt_channel_remap works on the reduced image; dec_opt_flipped together with a scale is refused by the decode call"""
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_hdlike_r24"][0])
    for fused in (1, 0):
        dec = G.Decoder(dlib)
        dec.set_fused(fused)
        assert dec.set_option("dec_opt_channel_remap", "210") == 0
        for s in SCALES:
            want, im2 = expected(O, jpeg, -1, -1, s)
            assert np.array_equal(decode_scaled(G, dlib, jpeg, None, None, s, dec)[0], O.channel_remap(im2, want, "210")), (fused, s)
        dec.close()
    dec = G.Decoder(dlib)
    assert dec.set_option("dec_opt_flipped", "1") == 0
    with pytest.raises(RuntimeError):
        decode_scaled(G, dlib, jpeg, None, None, 2, dec)
    assert dec.set_option(OPT, "1") == 0  # (full size: the flip works as ever)
    assert dec.decode(jpeg)[0].size == 480 * 272 * 3
    dec.close()


@pytest.mark.parametrize("tokens", [False, True], ids=["planes", "tokens"])
def test_line_alignment_applies_to_the_reduced_line(O, G, dlib, tokens, monkeypatch):
    """dec_opt_alignment_bytes pads the lines of the reduced image (both IDCT sides)"""
    monkeypatch.setenv("GJ_DEC_TOKENS" if tokens else "GJ_DEC_NO_TOKENS", "1")
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_odd_noise"][0])
    st = O.parse(jpeg)
    coefs = O.huffman_decode(st, jpeg)
    dec = G.Decoder(dlib)
    assert dec.set_option("dec_opt_alignment_bytes", "64") == 0
    for s in SCALES:
        W, H = dims(119, 61, s)
        st.img.width_padding = -(W * 3) % 64
        want, im2 = expected_from_coefs(O, st, coefs, s)
        px, pi = decode_scaled(G, dlib, jpeg, None, None, s, dec)
        pitch = W * 3 + pi.width_padding
        assert pi.width_padding == im2.width_padding == -(W * 3) % 64 and pitch % 64 == 0 and px.size == dlib.image_size(pi) == want.size
        assert np.array_equal(px[:H * pitch].reshape(H, pitch)[:, :W * 3], want[:H * pitch].reshape(H, pitch)[:, :W * 3]), s
    dec.close()
    O.lib().gjo_stream_free(C.byref(st))


def test_custom_host_buffer(O, G, dlib):
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_odd_noise"][0])
    dec = G.Decoder(dlib)
    assert dec.set_option(OPT, "1/2") == 0
    want = expected(O, jpeg, -1, -1, 2)[0]
    buf = np.full(want.size + 64, 0xA5, np.uint8)
    out = G.DecoderOutput()
    out.type, out.data = G.DECODER_OUTPUT_CUSTOM_BUFFER, buf.ctypes.data
    assert dlib.L.gpujpeg_decoder_decode(dec.h, jpeg.ctypes.data, jpeg.size, C.byref(out)) == 0
    assert out.data_size == want.size and (out.param_image.width, out.param_image.height) == (60, 31)
    assert np.array_equal(buf[:want.size], want) and np.all(buf[want.size:] == 0xA5)
    dec.close()


@pytest.mark.gpu
def test_custom_device_buffer(O, G, gpu_lib):
    import torch
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_natural_auto"][0])
    dj = torch.from_numpy(jpeg).cuda()
    for s in SCALES:
        want = expected(O, jpeg, -1, -1, s)[0]
        d_out = torch.full((want.size + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        dec = G.Decoder(gpu_lib)
        assert dec.set_option(OPT, f"1/{s}") == 0
        out = G.DecoderOutput()
        out.type, out.data = G.DECODER_OUTPUT_CUSTOM_CUDA_BUFFER, d_out.data_ptr()
        for _ in range(2):  # (a device-resident stream; the second call launches on the cached header)
            assert gpu_lib.L.gpujpeg_decoder_decode(dec.h, dj.data_ptr(), jpeg.size, C.byref(out)) == 0
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert out.data_size == want.size and np.array_equal(got[:want.size], want) and np.all(got[want.size:] == 0xA5), s
        dec.close()


# ================================================================================================ batches
def test_batch_calls_equal_frame_at_a_time(O, G, dlib):
    """5 HD-like frames at 1/2, chunk size 2: the batch calls return the reduced frames of the single calls, strides counted in reduced frames"""
    case = [c for c in CASES if c[0] == "rgb_hdlike_r24"][0]
    w, h = case[1], case[2]
    streams = [O.encode(oracle_image(O, case), natural_image(w, h, 3, seed=20 + f)) for f in range(5)]
    single = G.Decoder(dlib)
    assert single.set_option(OPT, "1/2") == 0
    want = [single.decode(x)[0] for x in streams]
    single.close()
    for f, x in enumerate(streams):
        assert np.array_equal(want[f], expected(O, x, -1, -1, 2)[0]), f
    dec = G.Decoder(dlib)
    dec.set_batch_chunk(2)
    assert dec.set_option(OPT, "1/2") == 0
    for rep in range(2):
        got, pi = dec.decode_batch(streams)
        assert (pi.width, pi.height) == (w // 2, h // 2)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), rep
    got, pi = dec.decode_batch_ptrs(streams, want[0].size)  # room for exactly a reduced frame
    assert (pi.width, pi.height) == (w // 2, h // 2) and all(np.array_equal(a, b) for a, b in zip(got, want))
    # and back to full size: the batched launches
    assert dec.set_option(OPT, "1") == 0
    got, pi = dec.decode_batch(streams)
    assert (pi.width, pi.height) == (w, h) and all(np.array_equal(a, O.decode(x)[0]) for a, x in zip(got, streams))
    dec.close()


# ================================================================================================ damaged streams
def damaged_streams(jpeg):
    """the fuzz tests' three kinds: truncated, a flipped byte in a scan, a missing restart marker"""
    d = jpeg.copy()
    sos = int(np.nonzero((d[:-1] == 0xFF) & (d[1:] == 0xDA))[0][0])
    rst = [int(i) for i in np.nonzero((d[:-1] == 0xFF) & (d[1:] >= 0xD0) & (d[1:] <= 0xD7))[0] if i > sos]
    out = [("truncated", d[: d.size * 2 // 3].copy())]
    flipped = d.copy()
    i = sos + 40 + (d.size - sos) // 3
    while flipped[i] == 0xFF or flipped[i - 1] == 0xFF or flipped[i + 1] == 0xFF:
        i += 1
    flipped[i] ^= 0x5A
    if flipped[i] == 0xFF:
        flipped[i] = 0x11
    out.append(("flipped_byte", flipped))
    m = rst[len(rst) // 2]
    out.append(("missing_restart_marker", np.concatenate([d[:m], d[m + 2:]])))
    return out


def raw_call(G, lib, dec, data):
    out = G.DecoderOutput()
    out.type = G.DECODER_OUTPUT_INTERNAL_BUFFER
    data = np.ascontiguousarray(data)
    rc = lib.L.gpujpeg_decoder_decode(dec.h, data.ctypes.data, data.size, C.byref(out))
    px = np.frombuffer((C.c_uint8 * out.data_size).from_address(out.data), np.uint8).copy() if rc == 0 else None
    return rc, px


@pytest.mark.parametrize("tokens", [False, True], ids=["planes", "tokens"])
def test_damaged_streams(O, G, dlib, tokens, monkeypatch):
    """A damaged stream at 1/4 returns like the full-size call on the same bytes; when that succeeds, the reduced pixels are the definition applied
    to the coefficients the call decoded (read_coefficients). Token mode decodes the same pixels without the planes. Out-of-bounds accesses are
    what the sanitizer build of this file's CPU tier is for."""
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_natural_auto"][0])
    st = O.parse(jpeg)
    monkeypatch.setenv("GJ_DEC_TOKENS" if tokens else "GJ_DEC_NO_TOKENS", "1")
    good = expected(O, jpeg, -1, -1, 4)[0]
    for kind, bad in damaged_streams(jpeg):
        ref_dec, keep, dec = G.Decoder(dlib), G.Decoder(dlib), G.Decoder(dlib)
        rc_full, _ = raw_call(G, dlib, ref_dec, bad)
        keep.keep_coefficients(True)
        for d in (keep, dec):
            assert d.set_option(OPT, "1/4") == 0
        rc_keep, px_keep = raw_call(G, dlib, keep, bad)
        rc, px = raw_call(G, dlib, dec, bad)
        assert (rc == 0) == (rc_full == 0) == (rc_keep == 0), (kind, rc_full, rc_keep, rc)
        if rc_keep == 0:
            coefs = keep.coefficients(st.img.data_size)
            assert coefs.size == st.img.data_size
            want = expected_from_coefs(O, st, coefs, 4)[0]
            assert np.array_equal(px_keep, want), kind
            if kind == "flipped_byte" or not tokens:  # (the marker structure is intact: token mode and plane mode decode the same samples)
                assert np.array_equal(px, want), kind
        assert np.array_equal(dec.decode(jpeg)[0], good), kind  # the decoder is intact afterwards
        for d in (ref_dec, keep, dec):
            d.close()
    O.lib().gjo_stream_free(C.byref(st))


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


def _run(env, args, timeout=900):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, errors="replace", timeout=timeout, env=env, cwd=ROOT)
    tail = (r.stdout[-1500:] + "\n" + "\n".join(ln for ln in r.stderr.splitlines() if not ln.startswith("[GPUJPEG]"))[-3000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    return r.stdout


def test_cpu_tier_under_sanitizers(asan_env):
    """this file's CPU-tier tests once more on the AddressSanitizer + UBSan build of the execution model (every geometry and the damaged streams
    through the new kernels and the reduced buffers)"""
    env = dict(asan_env, GJ_EMU_LIB=ASAN_LIB)
    out = _run(env, ["-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-n", "4", "-m", "not gpu", "-p", "no:faulthandler", "-p", "no:cacheprovider",
                     "-k", "emu and not under_sanitizers"], timeout=1500)
    assert " passed" in out and "failed" not in out, out[-1500:]


# ================================================================================================ command line
@pytest.mark.gpu
def test_cli_reduced_decode(O, G, gpu_lib, tmp_path):
    """gpujpegtool -d -O dec_opt_scale=1/4 writes a PNM of the reduced size whose pixels are the API's"""
    tool = os.path.join(os.path.dirname(G.PRODUCT_LIB), "gpujpegtool")
    jpeg = case_stream(O, [c for c in CASES if c[0] == "rgb_odd_noise"][0])
    src, dst = tmp_path / "in.jpg", tmp_path / "out.pnm"
    jpeg.tofile(src)
    r = subprocess.run([tool, "-d", "-O", "dec_opt_scale=1/4", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    import re
    data = dst.read_bytes()
    m = re.match(rb"P6\s+(\d+)\s+(\d+)\s+(\d+)\s", data)
    assert m and tuple(int(x) for x in m.groups()) == (30, 16, 255), data[:32]
    px = decode_scaled(G, gpu_lib, jpeg, None, None, 4)[0]
    assert np.array_equal(np.frombuffer(data[m.end():], np.uint8), px) and np.array_equal(px, expected(O, jpeg, -1, -1, 4)[0])
    assert "dec_opt_scale" in subprocess.run([tool, "-O", "help"], capture_output=True, text=True, timeout=60).stdout
