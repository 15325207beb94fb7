"""Decoder and encoder on streams built from CHOSEN coefficients, Huffman tables, table slots and table maps (tests/synth_streams.py).

The streams of the other suites are images pushed through an encoder: |AC| stays below 232 there, the tables are Annex K's (or the product's own
fit-limited ones) in slots 0 and 1 with the standard component -> table map. The decoder's fallbacks for everything else -- a value beyond a
token's 10 bits (gj_dec_entropy_tok.hip: `mx >= 10u`, the batch goes through the planes and its block records say 0xFFFF), tables in slots 2 and 3
or with more second-level tables than the two-level layout holds (gj_decoder.c dec_tables: tab2_ok; gj_tables.c gj_huffman_decoder_table2 returns 1),
the +-32768 clamp of the reduced-size decode (gj_dec_idct_scaled.hip gj_dequant_clamp) -- and the encoder's AC symbols of size 9 and 10 are reached
here on purpose; each test asserts in Python the property of its INPUT that forces the path.

Ground truth, in this order: (a) the coefficients are the chosen ones; (b) oracle.huffman_decode of the synthetic stream returns them -- this pins
the Python writer without any product code; (c) pixels are oracle.decode (reduced images: the definition restated in tests/test_scaled_decode.py,
regions: a numpy crop); (d) CPU tier only, where oracle/_ref is built: the reference's own library decodes every synthetic stream to the oracle's
pixels. Every comparison of a decode is byte for byte.

The encoder's own limit, the size of its output buffer, is the last section but one: thin frames whose stream the reference's sizing rule does not
hold, frames of 65535 pixels in one dimension, and the assembly kernels' overflow guard on both sides of its boundary (GJ_ENC_OUT_CAP).

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on the MI355X. One test
re-runs the CPU tier on the AddressSanitizer + UBSan build of the execution model. tests/MUTATIONS.md records which of these tests fail for which
deliberate defect of the decoder and of the encoder's output limit.

Times: the CPU tier of this file takes about 95 s on 8 cores (pytest -n 8), its slowest test 29 s (test_mixed_batches_in_token_mode); the sanitizer
re-run 7 min 20 s. The -m gpu tier had not been timed on an MI355X when this file was written. With the output-limit section: the CPU tier without
the sanitizer re-run about 3 min on 8 cores (the 65535-pixel frames take 15 .. 45 s each on the execution model, eight decoder paths twice), the
sanitizer re-run 12 min 20 s of its 25 min limit with other work on the machine."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import synth_streams as S
import test_scaled_decode as SD
from conftest import api_params, oracle_image
from synth_streams import Spec
from test_huffman_optimal import OPT as ENC_OPT, OPTIMAL, subtables, transcode
from test_region_decode import crop, opt_value

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")
ASAN_DIR = os.path.join(EMU_DIR, "_build_asan")
ASAN_LIB = os.path.join(ASAN_DIR, "libgpujpeg_emu.so")
CLANG_RT = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"
MAIN = "rgb_640x368_r12"  # the smallest frame with several token batches per scan: 3 x 307 restart segments of 12 blocks
TOK_GMAX = 64             # segments per batch of the token decoder at most (gj_dec_internal.h GJ_TOK_GMAX)
SCALES = SD.SCALES
REGIONS = [(0, 0, 640, 368), (213, 123, 161, 93), (627, 357, 13, 11)]  # the whole image, an interior rectangle, the bottom-right corner


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


# ================================================================================================ decoders of every path
PATHS = {"default": {}, "tokens": {"GJ_DEC_TOKENS": "1"}, "no_tokens": {"GJ_DEC_NO_TOKENS": "1"}, "seq": {"GJ_DEC_SEQ": "1"},
         "tokens_seq": {"GJ_DEC_TOKENS": "1", "GJ_DEC_SEQ": "1"}, "serial": {"GJ_DEC_ENTROPY": "serial"}, "unfused": {}, "keep_coefficients": {}}
SETTINGS = ("GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS", "GJ_DEC_SEQ", "GJ_DEC_ENTROPY", "GPUJPEG_NO_FUSED", "GPUJPEG_HOST_SCAN", "GJ_DEC_NO_SPEC")


def make_decoder(G, lib, monkeypatch, path, geometry=None, perf=False):
    """a decoder of one of PATHS (the developer settings are taken when a decoder is created), set to the geometry's output format"""
    with monkeypatch.context() as mp:
        for k in SETTINGS:
            mp.delenv(k, raising=False)
        for k, v in PATHS[path].items():
            mp.setenv(k, v)
        dec = SD.perf_decoder(G, lib) if perf else G.Decoder(lib)
    if path == "unfused":
        dec.set_fused(0)
    if path == "keep_coefficients":
        dec.keep_coefficients(True)
    fmt = S.output_format(geometry) if geometry else None
    if fmt:
        dec.set_output_format(fmt[1], fmt[0])
    return dec


def check_paths(G, lib, monkeypatch, spec, paths=PATHS):
    """the stream of `spec` through the decoders of `paths`, two calls each (the second one runs on the cached header): the oracle's pixels, and the
    chosen coefficients where the decoder keeps them"""
    jpeg, coefs = S.get(spec)
    want = S.pixels(spec)[0]
    for path in paths:
        dec = make_decoder(G, lib, monkeypatch, path, spec.geometry)
        for rep in range(2):
            px = dec.decode(jpeg)[0]
            assert px.size == want.size and np.array_equal(px, want), (S.spec_id(spec), path, rep, int(np.count_nonzero(px != want)))
        if path == "keep_coefficients":
            got = dec.coefficients(coefs.size)
            assert got.size == coefs.size and np.array_equal(got, coefs), (S.spec_id(spec), int(np.count_nonzero(got != coefs)))
        dec.close()


@functools.lru_cache(maxsize=None)
def reduced(spec, s):
    """the reduced image of the Spec's stream at 1/s by the definition (tests/test_scaled_decode.py), read-only"""
    pf, cs = S.output_format(spec.geometry) or (-1, -1)
    px = SD.expected(S.O, S.get(spec)[0], pf, cs, s)[0]
    px.setflags(write=False)
    return px


def decode_at(G, lib, dec, jpeg, scale=1, region=None):
    """one call of `dec` at a scale or on a region (the two options exclude each other)"""
    assert dec.set_option("dec_opt_region", "full" if region is None else opt_value(region)) == 0
    assert dec.set_option("dec_opt_scale", "1" if scale == 1 else f"1/{scale}") == 0
    return dec.decode(jpeg)[0]


def segments_with_big(coefs, geometry, quality, restart):
    """per scan of a non-interleaved frame: one flag per restart segment -- does it hold a coefficient beyond a token's 10 value bits (|v| >= 512)?"""
    img, out = S.image(geometry, quality), []
    for c in range(img.comp_count):
        k = img.comp[c]
        blocks = np.abs(np.asarray(coefs[k.data_offset:k.data_offset + k.data_width * k.data_height]).reshape(-1, 64)[:, :]).copy()
        blocks[:, 0] = 0  # (the DC difference has a slot of its own)
        big = blocks.max(1) >= 512
        out.append(np.array([big[a:a + restart].any() for a in range(0, big.size, restart)]))
    return out


def longest_run(flags):
    best = cur = 0
    for f in flags:
        cur = cur + 1 if f else 0
        best = max(best, cur)
    return best


# ================================================================================================ (a), (b): the streams themselves
GENERATORS = ["sparse", "big_1", "big_5", "big_dense", "shapes", "every_symbol", "dc_extremes"]
QUALITIES = (100, 75, 1)  # all steps 1, the usual tables, all steps 255 (|coefficient x step| reaches 1023 x 255)
PATH_SPECS = [Spec(geo, gen, QUALITIES[(gi + ki) % 3]) for gi, geo in enumerate(S.GEOMETRIES) for ki, gen in enumerate(GENERATORS)]

EVERY_SYMBOL_DEEP = Spec(MAIN, "every_symbol", 100, "unrestricted")
MAP_MIXED = ((1, 0), (0, 1), (1, 1))     # luminance with the "chrominance" DC table; Cb and Cr differ from each other
MAP_FOUR = ((3, 2), (0, 1), (2, 3))      # slots 0..3, every component its own pair
NOT_TAKEN_SPECS = [EVERY_SYMBOL_DEEP,
                   Spec(MAIN, "shapes", 75, slots=((0, 2), (1, 3))), Spec("420_il_322x242_r3", "big_5", 75, slots=((0, 2), (1, 3))),
                   Spec("grey_333x111", "shapes", 75, slots=((0, 3),)),
                   Spec(MAIN, "big_5", 100, "fitted", table_map=MAP_FOUR), Spec("420_il_322x242_r3", "shapes", 75, table_map=MAP_FOUR, dht_layout="single"),
                   Spec("uyvy_il_322x50", "every_symbol", 75, "unrestricted", table_map=MAP_FOUR)]
TAKEN_SPECS = [Spec(MAIN, "sparse", 75, "fixed_length"), Spec("420_il_322x242_r3", "shapes", 75, "fixed_length", dht_layout="single"),
               Spec(MAIN, "few_symbols", 100, "skewed"), Spec("uyvy_il_322x50", "few_symbols", 75, "skewed", table_map=MAP_MIXED, dht_layout="single"),
               Spec(MAIN, "every_symbol", 100, "fitted"), Spec("grey_333x111", "every_symbol", 75, "fitted", dht_layout="single"),
               Spec(MAIN, "shapes", 75, table_map=MAP_MIXED), Spec(MAIN, "big_5", 75, "fitted", table_map=MAP_MIXED, dht_layout="single"),
               Spec("420_il_322x242_r3", "shapes", 75, table_map=MAP_MIXED), Spec("420_il_322x242_r3", "every_symbol", 100, "fitted", table_map=MAP_MIXED, dht_layout="single"),
               Spec("rgb_320x64_r1", "few_symbols", 100, "skewed", table_map=MAP_MIXED), Spec("rgb_200x120_r0", "every_symbol", 1, "fitted", table_map=MAP_MIXED)]
QUANT_SPECS = [Spec(geo, "big_5", 100, quant=q) for geo in (MAIN, "420_il_322x242_r3") for q in ("all_255", "mixed_1_255", "slots_1_2_3")] + \
              [Spec("grey_333x111", "shapes", 100, quant="slots_1_2_3")]
MIXED_SPECS = [Spec(MAIN, g, 75) for g in ("big_1", "big_5", "big_dense")]
CLAMP_SPECS = [Spec(MAIN, "low_frequency_extremes", 1), Spec(MAIN, "low_frequency_511", 1)]
STATE_SPECS = [Spec(MAIN, "big_5", 75), Spec(MAIN, "sparse_other", 75)]
BATCH_SPECS = [[Spec(MAIN, g, 75, slots=((0, 2), (1, 3))) for g in ("sparse", "shapes", "sparse_other")],
               [EVERY_SYMBOL_DEEP, Spec(MAIN, "every_symbol_other", 100, "unrestricted"), EVERY_SYMBOL_DEEP]]
ALL_SPECS = list(dict.fromkeys(PATH_SPECS + NOT_TAKEN_SPECS + TAKEN_SPECS + QUANT_SPECS + MIXED_SPECS + CLAMP_SPECS + STATE_SPECS + [s for b in BATCH_SPECS for s in b]))


def ids(specs):
    return [S.spec_id(s) for s in specs]


@pytest.mark.parametrize("spec", ALL_SPECS, ids=ids(ALL_SPECS))
def test_streams_hold_the_chosen_coefficients(O, spec):
    """(a) the chosen coefficients are baseline-legal; (b) the oracle's Huffman decoder returns exactly them from the synthetic stream, whatever its
    tables, slots, table map and DHT layout -- and the stream says what the Spec says. No product code."""
    jpeg, coefs = S.get(spec)
    Z = S.zigzag_blocks(coefs)
    assert np.abs(Z[:, 1:]).max() <= 1023 and -1024 <= Z[:, 0].min() and Z[:, 0].max() <= 1016
    pf, cs = S.output_format(spec.geometry) or (-1, -1)
    st = O.parse(jpeg, pf, cs)
    try:
        back = O.huffman_decode(st, jpeg)
        assert back.size == coefs.size and np.array_equal(back, coefs), int(np.count_nonzero(back != coefs))
        n = st.img.comp_count
        tables, segments = S.dht_tables(jpeg)
        if spec.table_map:
            assert [tuple(st.hmap[c]) for c in range(n)] == [tuple(x) for x in spec.table_map[:n]]
        if spec.slots:
            assert {st.hmap[c][k] for c in range(n) for k in range(2)} <= {new for _, new in spec.slots}
        if spec.quant == "slots_1_2_3":
            assert [st.qmap[c] for c in range(n)] == [1, 2, 3][:n]
        if spec[3:] != Spec("", "")[3:]:  # (re-coded: exactly the tables the scans use, in the layout asked for)
            assert segments == (1 if spec.dht_layout == "single" else len(tables))
            assert {(cls, tid) for cls, tid, _, _ in tables} == {(k, st.hmap[c][k]) for c in range(n) for k in range(2)}
    finally:
        O.lib().gjo_stream_free(C.byref(st))


def test_generators_reach_what_they_are_for(O):
    """the properties of the INPUT the tests below rely on, on the main geometry"""
    Z = {g: S.zigzag_blocks(S.coefficients(MAIN, g, 100)) for g in S.GENERATORS}
    assert np.abs(Z["sparse"][:, 1:]).max() < 512 and 0.06 < np.count_nonzero(Z["sparse"][:, 1:]) / Z["sparse"][:, 1:].size < 0.10
    assert np.count_nonzero(np.abs(Z["big_1"][:, 1:]) > 7) == 1 and np.count_nonzero(np.abs(Z["big_5"][:, 1:]) > 7) == 5
    assert np.all(np.abs(Z["big_dense"][:, 1:]).max(1) >= 511)
    sh = Z["shapes"]
    nz = sh[:, 1:] != 0
    assert np.count_nonzero(nz.all(1)) >= 4, "blocks without EOB"
    assert np.count_nonzero(nz[:, 62] & (nz.sum(1) == 1)) >= 2 and np.count_nonzero(nz[:, 0] & (nz.sum(1) == 1)) >= 2 and np.count_nonzero(~nz.any(1)) >= 2
    assert np.any(~nz[:-1].any(1) & nz[1:].all(1)), "an empty block in front of a full one"
    ac, dc = S.symbol_sizes(S.stream(MAIN, "shapes", 100)[0])
    assert {0xF0, 0x00} <= ac[0] and any(s >> 4 == 15 and s & 15 for s in ac[0]), "ZRL, EOB and a run of exactly 15"
    ac, dc = S.symbol_sizes(S.stream(MAIN, "every_symbol", 100)[0])
    assert ac[0] == {0x00, 0xF0} | {(r << 4) | s for r in range(16) for s in range(1, 11)} and dc[0] == set(range(12))
    ac, dc = S.symbol_sizes(S.stream(MAIN, "dc_extremes", 100)[0])
    assert 11 in dc[0] and 11 in dc[1]
    ac, dc = S.symbol_sizes(S.stream(MAIN, "few_symbols", 100)[0])
    assert all(len(v) == 16 for v in ac.values())


# ================================================================================================ every entropy decoder path
@pytest.mark.parametrize("spec", PATH_SPECS, ids=ids(PATH_SPECS))
def test_every_entropy_decoder_path(O, G, dlib, spec, monkeypatch):
    """every generator x every geometry (qualities 100, 75 and 1 in turn) through the default path, token mode, plane mode, the lane-per-segment
    kernel with and without tokens, the serial decoder, the generic kernels and a decoder that keeps its coefficients"""
    check_paths(G, dlib, monkeypatch, spec)


# ================================================================================================ mixed batches in token mode
@pytest.mark.parametrize("spec", MIXED_SPECS, ids=ids(MIXED_SPECS))
def test_mixed_batches_in_token_mode(O, G, dlib, spec, monkeypatch):
    """A token-mode frame whose batches are of both kinds: a batch with a |v| >= 512 goes through the planes inside the token decoder and its blocks'
    records say so (gj_dec_entropy_tok.hip: `mx >= 10u`), the others stay tokens -- the token-fed full-size, reduced-size and region kernels read
    both kinds in one frame. big_1 / big_5: some batches; big_dense: every batch. Plane mode gives the same bytes."""
    jpeg, coefs = S.get(spec)
    flags = segments_with_big(coefs, MAIN, spec.quality, 12)
    assert [f.size for f in flags] == [307, 307, 307]
    if spec.generator == "big_dense":
        assert all(f.all() for f in flags), "every restart segment, so every batch, holds a value beyond a token"
    else:  # a batch is <= 64 consecutive segments of one scan, counted from the scan's first: 127 segments in a row hold a whole one
        assert any(f.any() for f in flags) and max(longest_run(~f) for f in flags) >= 2 * TOK_GMAX - 1
    full = S.pixels(spec)
    for path, sides in (("tokens", (0, 2, 4)), ("no_tokens", (0, 1, 3))):
        dec = make_decoder(G, dlib, monkeypatch, path, perf=True)
        for rep in range(2):  # (the second round launches on the cached header)
            px = decode_at(G, dlib, dec, jpeg)
            assert dec.idct_path() == sides[0] and np.array_equal(px, full[0]), (path, rep)
            for s in SCALES:
                px = decode_at(G, dlib, dec, jpeg, scale=s)
                assert dec.idct_path() == sides[1] and np.array_equal(px, reduced(spec, s)), (path, rep, s)
            for reg in REGIONS:
                px = decode_at(G, dlib, dec, jpeg, region=reg)
                assert dec.idct_path() == sides[2] and np.array_equal(px, crop(full[0], 640, 368, 1, reg)), (path, rep, reg)
        dec.close()


def test_state_between_calls_in_token_mode(O, G, dlib, monkeypatch):
    """one token-mode decoder: a frame with big values, a frame of the same header without any, the first again, a region of it, the second at full
    size -- block records that say "through the planes" (0xFFFF) left by an earlier call are never trusted"""
    a, b = STATE_SPECS
    assert S.get(a)[0].size != S.get(b)[0].size
    assert any(f.any() for f in segments_with_big(S.get(a)[1], MAIN, 75, 12)) and not any(f.any() for f in segments_with_big(S.get(b)[1], MAIN, 75, 12))
    first = min(int(np.argmax(f)) for f in segments_with_big(S.get(a)[1], MAIN, 75, 12) if f.any())  # a segment of 12 blocks with a big value, 80 blocks per row
    reg = (min(560, max(0, first * 12 % 80 * 8 - 20)), min(308, max(0, first * 12 // 80 * 8 - 20)), 80, 60)
    dec = make_decoder(G, dlib, monkeypatch, "tokens", perf=True)
    for i, (spec, region) in enumerate([(a, None), (b, None), (a, None), (a, reg), (b, None), (b, reg), (a, None)]):
        px = decode_at(G, dlib, dec, S.get(spec)[0], region=region)
        want = S.pixels(spec)[0] if region is None else crop(S.pixels(spec)[0], 640, 368, 1, region)
        assert dec.idct_path() == (0 if region is None else 4) and np.array_equal(px, want), (i, int(np.count_nonzero(px != want)))
    dec.close()


# ================================================================================================ the reduced decode's clamp
def unclamped_corners(O, spec, N):
    """per component: dequantised corners [by][bx][v][u] WITHOUT the definition's clamp"""
    jpeg, coefs = S.get(spec)
    st = O.parse(jpeg)
    out = []
    for c in range(st.img.comp_count):
        k = st.img.comp[c]
        q = np.array(list(st.qraw[st.qmap[c]]), np.int64)[SD.NATURAL_FROM_ZIGZAG]
        B = np.asarray(coefs[k.data_offset:k.data_offset + k.data_width * k.data_height]).reshape(k.data_height // 8, k.data_width // 8, 8, 8).astype(np.int64)
        out.append((B * q)[:, :, :N, :N])
    O.lib().gjo_stream_free(C.byref(st))
    return out


@pytest.mark.parametrize("spec", CLAMP_SPECS, ids=ids(CLAMP_SPECS))
def test_reduced_decode_clamps_the_dequantised_coefficients(O, G, dlib, spec, monkeypatch):
    """Quality 1 (steps of 255) and |AC| up to 1023 (low_frequency_511: up to 511, so that every batch of the token-mode frame stays tokens) at the
    low-frequency positions: the 8x8, 4x4 and 2x2 corners and the DC alone hold products beyond +-32767, which the definition clamps to
    [-32768, 32767] (gj_dec_idct_scaled.hip gj_dequant_clamp). All three scales on both IDCT sides, the generic side's planes included
    (test_scaled_decode.paths_body, imported)."""
    for N in (8, 4, 2, 1):
        D = unclamped_corners(O, spec, N)
        beyond = [np.abs(d).max((2, 3)) > 32767 for d in D]
        assert all(b.any() for b in beyond), N
    D8 = unclamped_corners(O, spec, 8)
    dc_only = [(np.abs(d[:, :, 0, 0]) > 32767) & (np.count_nonzero(d, (2, 3)) == 1) for d in D8]
    assert all(b.sum() >= 10 for b in dc_only), "blocks whose only coefficient is a DC beyond the clamp"
    big = segments_with_big(S.get(spec)[1], MAIN, 1, 12)
    assert any(f.any() for f in big) == (spec.generator == "low_frequency_extremes")
    SD.paths_body(O, G, dlib, S.get(spec)[0], monkeypatch)


def test_definition_with_clamped_inputs(O):
    """What the reduced-size definition promises once the clamp acts. test_scaled_decode.test_definition_integer_against_float argues
    |integer - round(float64)| <= 1 level for "legal" coefficients, whose dequantised values stay near the sample range; a clamped value is 32768
    and the argument's terms scale with it. Restated per sample, for inputs D (clamped, as in both restatements), table entries off by at most
    0.5 / 8192 and the two fraction bits of the first pass:
        |integer - exact| <= sum_u |K[x][u]| * (sum_v |D[v][u]| * 0.5 / 8192 + 1 / 8)  +  sum_u |T[y][u]| / 4 * 0.5 / 8192  +  1 / 2
    before the final clamp to 0..255, which cannot widen a difference. The bound is computed from the data and asserted for every sample; the float
    restatement clamps its inputs like the integer one (both take test_scaled_decode.corner_blocks), without that the two differ by up to 255.
    Measured here (CPU, numpy): max |integer - round(float64)| = 2 levels at 1/2 (23 samples of the two frames), 0 at 1/4 and 1/8; the bound at
    those samples is between 3.99 and 7.95 levels; a float64 transform of UNclamped inputs leaves the bound at 30670 samples. The integer definition is unchanged."""
    worst, over_one, differ_without_clamp = 0, 0, 0
    for spec in (Spec(MAIN, "low_frequency_extremes", 1), Spec("420_il_322x242_r3", "low_frequency_extremes", 1)):
        jpeg, coefs = S.get(spec)
        st = O.parse(jpeg)
        for s in SCALES:
            N = 8 // s
            K, m = SD.k_matrix(N), SD.m_matrix(N)
            got = SD.reduced_planes(st, coefs, N)
            for c in range(st.img.comp_count):
                D = SD.corner_blocks(st, coefs, c, N)
                assert D.min() == -32768 and D.max() == 32767, "the clamp acts on both sides"
                T = (np.einsum("yv,abvu->abyu", m, D) + 1024) >> 11
                exact = np.einsum("yv,abvu,xu->abyx", K, D.astype(np.float64), K)
                first = np.einsum("yv,abvu->abyu", np.ones((N, N)), np.abs(D)) * (0.5 / 8192) + 0.125  # (the same for every y)
                bound = np.einsum("xu,abyu->abyx", np.abs(K) + 0.5 / 8192, first) + np.einsum("xu,abyu->abyx", np.ones((N, N)), np.abs(T) / 4.0) * (0.5 / 8192) + 0.5
                nby, nbx = D.shape[:2]
                unrounded = np.clip(exact + 128, 0, 255).transpose(0, 2, 1, 3).reshape(nby * N, nbx * N)
                bound = bound.transpose(0, 2, 1, 3).reshape(nby * N, nbx * N)
                diff = np.abs(got[c].astype(np.float64) - unrounded)
                assert np.all(diff <= bound + 1e-6), (S.spec_id(spec), s, c, float((diff - bound).max()))
                d = np.abs(got[c].astype(np.int64) - np.rint(unrounded).astype(np.int64))
                worst, over_one = max(worst, int(d.max())), over_one + int(np.count_nonzero(d > 1))
                if (d > 1).any():
                    print(S.spec_id(spec), f"1/{s}", "component", c, "bound where |integer - round(float64)| > 1:", float(bound[d > 1].min()), "..", float(bound[d > 1].max()))
                raw = unclamped_corners(O, spec, N)[c].astype(np.float64)
                loose = np.clip(np.rint(np.einsum("yv,abvu,xu->abyx", K, raw, K) + 128), 0, 255).transpose(0, 2, 1, 3).reshape(nby * N, nbx * N)
                differ_without_clamp += int(np.count_nonzero(np.abs(loose - got[c]) > np.ceil(bound)))
        O.lib().gjo_stream_free(C.byref(st))
    print("max |integer - round(float64)| with clamped inputs =", worst, "levels;", over_one, "samples beyond 1 level;", differ_without_clamp,
          "samples where a transform of unclamped inputs leaves the bound")
    assert differ_without_clamp > 1000, "the streams tell a decode without the clamp from the definition"


# ================================================================================================ Huffman tables
def table_check(lib, bits, vals, is_ac):
    fn = lib.L.gpujpeg_amd_host_huffman_table_check
    fn.argtypes = [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int]
    return fn((C.c_uint8 * 17)(*bits), (C.c_uint8 * 256)(*(list(vals) + [0] * (256 - len(vals)))), is_ac)


@pytest.mark.parametrize("spec", NOT_TAKEN_SPECS, ids=ids(NOT_TAKEN_SPECS))
def test_tables_the_two_level_layout_does_not_take(O, G, dlib, spec, monkeypatch):
    """Streams for which dec_tables (gj_decoder.c) leaves tab2_ok false -- a table in slot 2 or 3 (`dc_table > 1 || ac_table > 1`), or one that needs
    more than GJ_DEC2_SUBTABLES = 6 second-level tables (gj_tables.c gj_huffman_decoder_table2 `return 1`) -- are decoded by the lane-per-segment
    kernel whatever the settings ask for. Every table is a valid one (gpujpeg_amd_host_huffman_table_check)."""
    tables, _ = S.dht_tables(S.get(spec)[0])
    assert any(tid > 1 for _, tid, _, _ in tables) or any(cls == 1 and subtables(bits) > 6 for cls, _, bits, _ in tables)
    if spec == EVERY_SYMBOL_DEEP:
        assert any(cls == 1 and subtables(bits) > 6 and max(L for L in range(17) if bits[L]) >= 14 for cls, _, bits, _ in tables)
    if spec.table_map == MAP_FOUR:
        assert {tid for _, tid, _, _ in tables} == {0, 1, 2, 3}
    for cls, tid, bits, vals in tables:
        assert table_check(dlib, bits, vals, cls) == 0, (cls, tid, bits)
    check_paths(G, dlib, monkeypatch, spec)


@pytest.mark.parametrize("specs", BATCH_SPECS, ids=["slots_2_3", "deep_tables"])
def test_tables_not_taken_in_the_batch_call(O, G, dlib, specs):
    """decode_batch, chunk size 2, 3 frames: Annex K tables in slots 2 and 3 (one header), and frames with deep tables of their own (the second
    frame's tables differ from its neighbours')"""
    streams = [S.get(s)[0] for s in specs]
    dec = G.Decoder(dlib)
    dec.set_batch_chunk(2)
    for rep in range(2):
        got, pi = dec.decode_batch(streams)
        assert (pi.width, pi.height) == (640, 368)
        for f, (px, s) in enumerate(zip(got, specs)):
            assert np.array_equal(px, S.pixels(s)[0]), (rep, f)
    dec.close()


@pytest.mark.parametrize("spec", TAKEN_SPECS, ids=ids(TAKEN_SPECS))
def test_tables_of_unusual_shape(O, G, dlib, spec, monkeypatch):
    """Tables the two-level layout takes, of shapes no encoder here writes: every symbol at 8 bits (DC: 4), one code of every length 1..16 (all six
    second-level code lengths behind ONE 10-bit prefix), the optimal table under the fit rule of a frame that uses every symbol; luminance with
    the second DC table and Cb / Cr with different tables -- in non-interleaved scans and in interleaved ones, where the table changes from
    block to block inside an MCU; one DHT segment per table or one for all."""
    tables, _ = S.dht_tables(S.get(spec)[0])
    assert all(tid <= 1 and subtables(bits) <= 6 for _, tid, bits, _ in tables)
    if spec.tables == "skewed":
        assert all(bits[1:] == [1] * 16 for cls, _, bits, _ in tables if cls == 1)
    if spec.tables == "fixed_length":
        assert all(sum(bits) == bits[8 if cls else 4] for cls, _, bits, _ in tables)
    for cls, tid, bits, vals in tables:
        assert table_check(dlib, bits, vals, cls) == 0, (cls, tid, bits)
    check_paths(G, dlib, monkeypatch, spec)


# ================================================================================================ quantisation tables
@pytest.mark.parametrize("spec", QUANT_SPECS, ids=ids(QUANT_SPECS))
def test_quantisation_variants(O, G, dlib, spec, monkeypatch):
    """every step 255, steps 1 and 255 mixed inside one table, three tables in slots 1..3 (SOF0 maps the components to them): full size and the three
    scales, default path, token mode and generic kernels"""
    jpeg = S.get(spec)[0]
    for path in ("default", "tokens", "unfused"):
        dec = make_decoder(G, dlib, monkeypatch, path, spec.geometry)
        for s in (1,) + tuple(SCALES) + (1,):
            px = decode_at(G, dlib, dec, jpeg, scale=s)
            want = S.pixels(spec)[0] if s == 1 else reduced(spec, s)
            assert np.array_equal(px, want), (path, s, int(np.count_nonzero(px != want)))
        dec.close()


# ================================================================================================ (d) the reference's own library
def test_reference_decodes_every_synthetic_stream(O, G, ref):
    """(d) CPU tier, where oracle/_ref is built: the reference's host code and kernels (contraction off, like the oracle under this fixture) decode
    every synthetic stream of this file to the oracle's pixels -- the oracle had not been pinned to the reference at these coefficient magnitudes,
    table shapes, slots and maps."""
    for spec in ALL_SPECS:
        jpeg = S.get(spec)[0]
        pf, cs = S.output_format(spec.geometry) or (-1, -1)
        want = O.decode(jpeg, pf, cs)[0]  # (not the cached pixels: the oracle runs without contraction under this fixture)
        dec = G.Decoder(ref)
        if pf >= 0:
            dec.set_output_format(cs, pf)
        px = dec.decode(jpeg)[0]
        dec.close()
        assert px.size == want.size and np.array_equal(px, want), (S.spec_id(spec), int(np.count_nonzero(px != want)))


# ================================================================================================ encoder
# name, width, height, restart, interleaved, subsampling
ENC_SIZES = [("rgb_320x200_r12", 320, 200, 12, 0, None), ("420_il_322x122_r3", 322, 122, 3, 1, [(2, 2), (1, 1), (1, 1)]), ("rgb_200x104_r0", 200, 104, 0, 0, None)]
PATTERNS = ["basis", "checkerboard", "stripes", "blocks", "noise"]
ENC_CASES = [(p, size, q) for size in ENC_SIZES for q in (100, 97) for p in PATTERNS]


def enc_case(pattern, size, q):
    name, w, h, ri, il, ss = size
    return (f"{pattern}_{name}_q{q}", w, h, 1, 1, q, ri, il, ss, 3)


@functools.lru_cache(maxsize=None)
def enc_expected(pattern, size_name, q):
    """(raw image, the oracle's stream, its coefficients) -- read-only"""
    size = [s for s in ENC_SIZES if s[0] == size_name][0]
    case = enc_case(pattern, size, q)
    raw = S.pattern(pattern, case[1], case[2])
    img = oracle_image(S.O, case)
    coefs = S.O.fdct_quant(img, S.O.preprocess(img, raw))
    jpeg = S.O.encode_from_coefs(img, coefs)
    for a in (coefs, jpeg):
        a.setflags(write=False)
    return raw, jpeg, coefs


def test_encoder_patterns_reach_the_extremes(O):
    """the oracle's own coefficients of the patterns: AC of size 10 (|AC| >= 512) and DC differences of size 11 at every size and quality"""
    for size in ENC_SIZES:
        for q in (100, 97):
            ac, dc = set(), set()
            for p in PATTERNS:
                a, d = S.symbol_sizes(enc_expected(p, size[0], q)[1])
                ac |= {s & 15 for v in a.values() for s in v}
                dc |= {s for v in d.values() for s in v}
            assert {9, 10} <= ac and 11 in dc, (size[0], q, sorted(ac), sorted(dc))
    Z = S.zigzag_blocks(enc_expected("basis", ENC_SIZES[0][0], 100)[2])
    assert np.abs(Z[:, 1:]).max() >= 1000 and Z[:, 0].min() == -1024 and Z[:, 0].max() == 1016


@pytest.mark.parametrize("pattern,size,q", ENC_CASES, ids=[f"{p}-{s[0]}-q{q}" for p, s, q in ENC_CASES])
def test_encoder_codes_the_extremes(O, G, dlib, pattern, size, q):
    """the product's stream is the oracle's: fused kernels, the kernels that go through the coefficient planes (whose content is the oracle's), generic"""
    case = enc_case(pattern, size, q)
    raw, want, coefs = enc_expected(pattern, size[0], q)
    p, pi = api_params(dlib, G, case)
    enc = G.Encoder(dlib)
    got = enc.encode(p, pi, raw)
    assert got.size == want.size and np.array_equal(got, want), "fused"
    enc.keep_coefficients()
    got = enc.encode(p, pi, raw)
    assert got.size == want.size and np.array_equal(got, want), "coefficient planes"
    assert np.array_equal(enc.coefficients(coefs.size), coefs)
    enc.set_fused(False)
    got = enc.encode(p, pi, raw)
    assert got.size == want.size and np.array_equal(got, want), "generic"
    enc.close()


@pytest.mark.parametrize("size", ENC_SIZES, ids=[s[0] for s in ENC_SIZES])
def test_encoder_optimal_tables_at_the_extremes(O, G, dlib, size):
    """enc_opt_huffman=optimal on frames with AC symbols of size 9 and 10 and DC size 11: the transcoded default stream, byte for byte"""
    for pattern in ("basis", "noise"):
        case = enc_case(pattern, size, 100)
        raw, default, _ = enc_expected(pattern, size[0], 100)
        p, pi = api_params(dlib, G, case)
        for fused in (True, False):
            enc = G.Encoder(dlib)
            enc.set_fused(fused)
            assert enc.set_option(ENC_OPT, OPTIMAL) == 0
            got = enc.encode(p, pi, raw)
            enc.close()
            want = enc_transcoded(pattern, size[0])
            assert got.size == want.size and np.array_equal(got, want), (pattern, fused)


@functools.lru_cache(maxsize=None)
def enc_transcoded(pattern, size_name):
    return transcode(enc_expected(pattern, size_name, 100)[1])


@pytest.mark.parametrize("size", ENC_SIZES, ids=[s[0] for s in ENC_SIZES])
def test_encoder_batch_at_the_extremes(O, G, dlib, size):
    """the batch encode call on 3 such frames"""
    patterns = ["basis", "noise", "stripes"]
    case = enc_case("batch", size, 100)
    p, pi = api_params(dlib, G, case)
    raws = [enc_expected(x, size[0], 100)[0] for x in patterns]
    enc = G.Encoder(dlib)
    got = enc.encode_batch(p, pi, np.concatenate(raws), 3, dlib.image_size(pi))
    for x, g in zip(patterns, got):
        want = enc_expected(x, size[0], 100)[1]
        assert g.size == want.size and np.array_equal(g, want), x
    got = enc.encode_batch_ptrs(p, pi, [np.array(r) for r in raws])
    assert all(np.array_equal(g, enc_expected(x, size[0], 100)[1]) for x, g in zip(patterns, got))
    enc.close()


# ================================================================================================ encoder: the output-buffer limit
# The encoder's stream buffer holds 1000 + scan headers + 2 bytes per CODED sample (whole padded blocks; gj_encoder.c encoder_configure) + 4096 bytes.
# The reference counts the image's own samples, which a thin image exceeds with ordinary content (65535x1 codes eight rows of blocks for one of
# pixels): those frames are the first seven LIMIT_CASES. With the padded count a frame has about 2 bytes per coded sample of room and 0/255 noise at
# quality 100 needs 1.6, so no image reaches the assembly kernels' guard (k_gather; k_scan_segments + k_assemble + k_segment_info) and the host
# checks behind it through the public API any more: the developer setting GJ_ENC_OUT_CAP=<bytes> lowers the capacity they are told.
# tests/MUTATIONS.md ("encoder output limit") records which of these tests fail for which deliberate defect.
OUT_CAP = "GJ_ENC_OUT_CAP"
S420 = ((2, 2), (1, 1), (1, 1))
BYTES_PER_PIXEL = {0: 1, 1: 3, 3: 2}  # grey, packed RGB, packed 4:2:2
# name, width, height, pixel format, quality, restart, interleaved, subsampling, content, the route of gj_tile_kernel (gj_encode.hip) it takes
LIMIT_CASES = [
    # streams beyond the reference's sizing rule (asserted below)
    ("rgb_65535x1_q90_r8", 65535, 1, 1, 90, 8, 0, None, "ramp", "rgb444"),
    ("rgb_il_1x65535_q90_r8", 1, 65535, 1, 90, 8, 1, None, "ramp", "blocks"),
    ("rgb_65535x1_q100_r1", 65535, 1, 1, 100, 1, 0, None, "ramp", "planes"),
    ("rgb_512x1_q100_r8", 512, 1, 1, 100, 8, 0, None, "noise", "rgb444"),
    ("rgb_1025x9_q100", 1025, 9, 1, 100, -1, 0, None, "noise", "rgb444"),
    ("rgb_9x1025_q100", 9, 1025, 1, 100, -1, 0, None, "noise", "rgb444"),
    ("uyvy_il_1024x1_q100_r4", 1024, 1, 3, 100, 4, 1, None, "noise", "uyvy422"),
    # the largest dimension a frame can have (the other suites stop at 15 360)
    ("rgb_65535x8_auto", 65535, 8, 1, 90, -1, 0, None, "ramp", "rgb444"),
    ("rgb_8x65535_auto", 8, 65535, 1, 90, -1, 0, None, "ramp", "rgb444"),
    ("420_il_65535x9_r3", 65535, 9, 1, 90, 3, 1, S420, "ramp", "blocks"),
    ("420_il_9x65535_r3", 9, 65535, 1, 90, 3, 1, S420, "ramp", "blocks"),
    ("uyvy_il_65534x3_auto", 65534, 3, 3, 90, -1, 1, None, "ramp", "uyvy422"),
    ("uyvy_2x65535_auto", 2, 65535, 3, 90, -1, 0, None, "ramp", "planes"),
    ("grey_65535x5_r5", 65535, 5, 0, 90, 5, 0, None, "ramp", "blocks"),
    ("grey_5x65535_r0", 5, 65535, 0, 90, 0, 0, None, "ramp", "planes"),
]
BEYOND_THE_REFERENCE_RULE = 7  # the first so many of LIMIT_CASES


def limit_case(name, w, h, pf, q, ri, il, ss):
    """the case tuple of conftest.oracle_image / api_params: enc_case's, with the pixel format (and YCbCr input for the formats that are not RGB)"""
    c = enc_case("x", (name, w, h, ri, il, tuple(map(tuple, ss)) if ss else None), q)  # (tuples: the cases are keys of limit_expected's cache)
    return (name,) + c[1:] if pf == 1 else (name,) + c[1:3] + (pf, 3) + c[5:]


def limit_raw(content, w, h, pf, seed=0):
    """0/255 noise (S.pattern), a ramp over the bytes with noise of 0 .. 23 on it, or one value -- in the byte count of the pixel format"""
    n = w * h * BYTES_PER_PIXEL[pf]
    if content == "noise":
        raw = np.array(S.pattern("noise", w, h, seed)[:n])
    elif content == "flat":
        raw = np.full(n, 77, np.uint8)
    else:
        raw = ((np.arange(n, dtype=np.int64) * 3 // 11 + S.O.noise(n, seed=11 + seed) % 24) % 256).astype(np.uint8)  # (conftest.random_raw's ramp)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def limit_expected(case, content, segment_info=0, seed=0):
    """(raw image, the oracle's stream, the oracle's Image) -- read-only"""
    raw = limit_raw(content, case[1], case[2], case[3], seed)
    img = oracle_image(S.O, case, segment_info=segment_info)
    jpeg = S.O.encode(img, raw)
    jpeg.setflags(write=False)
    return raw, jpeg, img


def segment_blocks(img):
    """blocks per restart segment (0: no restart markers)"""
    per_mcu = sum(img.samp_h[c] * img.samp_v[c] for c in range(img.comp_count)) if img.interleaved else 1
    return img.restart_interval * per_mcu


def expected_route(case, img):
    """gj_tile_kernel (gj_encode.hip) restated for the configurations of these tests: a kernel from pixels to tile streams needs restart segments
    of 4 .. 256 blocks; k_encode_rgb444 takes packed RGB 4:4:4 in one scan per component, k_encode_uyvy422 packed 4:2:2 in an interleaved scan,
    k_encode_blocks the other RGB layouts and grey; everything else goes through the coefficient planes and k_huffman"""
    pf, il = case[3], case[7]
    if not 4 <= segment_blocks(img) <= 256 or (pf == 3 and not il):
        return "planes"
    if pf == 3:
        return "uyvy422"
    return "rgb444" if pf == 1 and not il and case[8] is None else "blocks"


def assert_route(G, lib, enc, p, pi, raw, want, route):
    """what the binding can tell: a batch call codes its frames by batched launches where a tile kernel takes the configuration, one by one otherwise"""
    got = enc.encode_batch(p, pi, np.array(raw), 1, lib.image_size(pi))
    assert got[0].size == want.size and np.array_equal(got[0], want), "batch of one"
    assert enc.last_batch() == ((0, 1) if route == "planes" else (1, 0)), (route, enc.last_batch())


def decode_paths(G, lib, monkeypatch, jpeg, want, fmt, paths=PATHS):
    """the stream through the decoders of `paths`, two calls each (the second one runs on the cached header): the oracle's pixels"""
    for path in paths:
        dec = make_decoder(G, lib, monkeypatch, path)
        if fmt:
            dec.set_output_format(fmt[1], fmt[0])
        for rep in range(2):
            px = dec.decode(jpeg)[0]
            assert px.size == want.size and np.array_equal(px, want), (path, rep, int(np.count_nonzero(px != want)))
        dec.close()


@pytest.mark.parametrize("tc", LIMIT_CASES, ids=[c[0] for c in LIMIT_CASES])
def test_thin_and_extreme_geometries(O, G, dlib, tc, monkeypatch):
    """Frames of one row or column of blocks and frames at the 65535 limit of a dimension, default settings: the fused kernels, the kernels that go
    through the coefficient planes and the generic ones write the oracle's stream, every decoder path returns the oracle's pixels from it. The
    first seven have streams that the reference's sizing rule (2 bytes per sample of the IMAGE) does not hold: refused before the buffer was
    sized by the coded samples. Between them the cases take all four routes of gj_tile_kernel."""
    name, w, h, pf, q, ri, il, ss, content, route = tc
    case = limit_case(name, w, h, pf, q, ri, il, ss)
    raw, want, img = limit_expected(case, content)
    scan_headers = img.scan_count * 10 if not img.interleaved else 8 + 2 * img.comp_count  # SOS: marker, length, count, 2 per component, Ss Se AhAl
    reference_rule = 1000 + scan_headers + w * h * img.comp_count * 2 + 4096
    print(name, "oracle stream", want.size, "B; the reference's rule", reference_rule, "B; coded samples", int(img.data_size))
    if LIMIT_CASES.index(tc) < BEYOND_THE_REFERENCE_RULE:
        assert want.size > reference_rule, (want.size, reference_rule)
    assert want.size <= 1000 + scan_headers + 2 * max(w * h * img.comp_count, int(img.data_size)) + 4096
    assert expected_route(case, img) == route, (segment_blocks(img), route)
    monkeypatch.delenv(OUT_CAP, raising=False)
    p, pi = api_params(dlib, G, case)
    enc = G.Encoder(dlib)
    got = enc.encode(p, pi, raw)
    assert got.size == want.size and np.array_equal(got, want), "fused"
    assert_route(G, dlib, enc, p, pi, raw, want, route)
    enc.keep_coefficients()
    got = enc.encode(p, pi, raw)
    assert got.size == want.size and np.array_equal(got, want), "coefficient planes"
    enc.set_fused(False)
    got = enc.encode(p, pi, raw)
    assert got.size == want.size and np.array_equal(got, want), "generic"
    enc.close()
    fmt = (3, 3) if pf == 3 else None
    want_px = O.decode(want, *(fmt or (-1, -1)))[0]
    decode_paths(G, dlib, monkeypatch, want, want_px, fmt)
    if name in ("rgb_65535x8_auto", "rgb_8x65535_auto"):  # a region that ends at the far edge, and the smallest reduced image
        reg = (65000, 2, 535, 6) if w > h else (2, 65000, 6, 535)
        dec = make_decoder(G, dlib, monkeypatch, "default")
        for rep in range(2):
            px = decode_at(G, dlib, dec, want, region=reg)
            assert np.array_equal(px, crop(want_px, w, h, 1, reg)), (rep, reg)
            px = decode_at(G, dlib, dec, want, scale=8)
            small = SD.expected(O, want, -1, -1, 8)[0]
            assert px.size == small.size and np.array_equal(px, small), (rep, "1/8")
        dec.close()


# ---- the guard: GJ_ENC_OUT_CAP on both sides of the boundary
# route, size (ENC_SIZES' columns), pixel format, what the encoder is set to
GUARD_SIZES = {"rgb444": (ENC_SIZES[0], 1), "blocks": (ENC_SIZES[1], 1), "uyvy422": (("uyvy_il_320x200_r4", 320, 200, 4, 1, None), 3),
               "restart0": (("rgb_320x200_r0", 320, 200, 0, 0, None), 1), "keep": (ENC_SIZES[0], 1), "generic": (ENC_SIZES[1], 1)}
# route, segment_info, enc_opt_huffman=optimal
GUARD_ROUTES = [(r, 0, False) for r in GUARD_SIZES] + [(r, 1, False) for r in GUARD_SIZES if r != "restart0"] + [("rgb444", 0, True), ("generic", 0, True)]


def guard_case(route):
    size, pf = GUARD_SIZES[route]
    return limit_case(size[0], size[1], size[2], pf, 100, size[3], size[4], size[5])


def capped_encoder(G, lib, monkeypatch, cap, route="rgb444", optimal=False, out=None):
    """an encoder created under GJ_ENC_OUT_CAP=<cap> (None: without the setting; the settings are taken when a coder is created), set to a route"""
    with monkeypatch.context() as mp:
        mp.delenv(OUT_CAP, raising=False)
        if cap is not None:
            mp.setenv(OUT_CAP, str(cap))
        enc = G.Encoder(lib)
    if route == "keep":
        enc.keep_coefficients()
    if route == "generic":
        enc.set_fused(False)
    if optimal:
        assert enc.set_option(ENC_OPT, OPTIMAL) == 0
    if out:
        assert enc.set_option("enc_opt_out", out) == 0
    return enc


def encode_to_host(lib, enc, p, pi, raw, device_out):
    """one encode call -> the stream as a numpy copy, whether the encoder leaves it in host or in device memory"""
    ptr, n = enc.encode_noclone(p, pi, raw)
    if not device_out:
        return np.ctypeslib.as_array(ptr, shape=(n,)).copy()
    L = lib.L
    L.gj_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.gj_hip_stream_sync.argtypes = [C.c_void_p]
    got = np.empty(n, np.uint8)
    assert L.gj_hip_memcpy_d2h(got.ctypes.data, C.cast(ptr, C.c_void_p), n, None) == 0 and L.gj_hip_stream_sync(None) == 0
    return got


def refusal(size, cap):
    return f"Compressed stream ({size} B) does not fit the output buffer ({cap} B)"


@pytest.mark.parametrize("route,segment_info,optimal", GUARD_ROUTES, ids=[f"{r}{'-segment_info' * si}{'-optimal' * o}" for r, si, o in GUARD_ROUTES])
def test_encoder_output_guard_both_sides(O, G, dlib, route, segment_info, optimal, monkeypatch, capfd):
    """S = the oracle's size of a dense frame (0/255 noise, quality 100). An encoder told a capacity of S bytes returns the oracle's bytes (the
    comparison is `total > capacity`), one told S - 1 returns -1 and its message names S bytes and the capacity in force -- through k_gather behind
    each of the three tile kernels, through k_scan_segments + k_assemble (no restart markers, kept coefficients, generic kernels), with the
    APP13 segment index (k_segment_info behind both), with the frame's own Huffman tables, into host and into device memory."""
    case = guard_case(route)
    raw, want, img = limit_expected(case, "noise", segment_info)
    if optimal:
        want = transcode(want)
    S_ = int(want.size)
    # (keep_coefficients() and set_fused(False) take a geometry of the tile kernels through the coefficient planes; without restart markers the geometry does)
    assert expected_route(case, img) == {"restart0": "planes", "keep": "rgb444", "generic": "blocks"}.get(route, route)
    tile_route = "planes" if route in ("restart0", "keep", "generic") else route
    assert S_ - 1 < 2 * int(img.data_size), "both capacities are below the stream buffer's size: the setting is the capacity in force"
    p, pi = api_params(dlib, G, case, segment_info=segment_info)
    for device_out in (False, True):
        out = "enc_out_val_device" if device_out else None
        enc = capped_encoder(G, dlib, monkeypatch, S_, route, optimal, out)
        if not optimal and not segment_info and not device_out:
            assert_route(G, dlib, enc, p, pi, raw, want, tile_route)
        for rep in range(2):
            got = encode_to_host(dlib, enc, p, pi, raw, device_out)
            assert got.size == S_ and np.array_equal(got, want), (device_out, rep, "capacity S")
        enc.close()
        enc = capped_encoder(G, dlib, monkeypatch, S_ - 1, route, optimal, out)
        capfd.readouterr()
        with pytest.raises(RuntimeError, match="gpujpeg_encoder_encode failed"):
            enc.encode_noclone(p, pi, raw)
        assert refusal(S_, S_ - 1) in capfd.readouterr().err, (device_out, "capacity S - 1")
        enc.close()


STATE_ROUTES = ["rgb444", "blocks", "keep"]


@pytest.mark.parametrize("route", STATE_ROUTES)
def test_encoder_state_after_a_refusal(O, G, dlib, route, monkeypatch, capfd):
    """one encoder under a capacity between the sizes of a flat and a dense frame of one geometry: dense (refused), flat, dense (refused), flat --
    the flat frames are the oracle's byte for byte. k_gather's two sets of group totals (the one a refused call leaves and the one it clears),
    the set the host picks for the next call and the epoch of k_scan_segments' partial sums survive the early return."""
    case = guard_case(route)
    dense, dense_jpeg, _ = limit_expected(case, "noise")
    flat, flat_jpeg, _ = limit_expected(case, "flat")
    cap = (int(flat_jpeg.size) + int(dense_jpeg.size)) // 2
    assert flat_jpeg.size < cap < dense_jpeg.size
    p, pi = api_params(dlib, G, case)
    enc = capped_encoder(G, dlib, monkeypatch, cap, route)
    for step in range(2):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            enc.encode(p, pi, dense)
        assert refusal(int(dense_jpeg.size), cap) in capfd.readouterr().err, step
        got = enc.encode(p, pi, flat)
        assert got.size == flat_jpeg.size and np.array_equal(got, flat_jpeg), (step, got.size, int(flat_jpeg.size))
    enc.close()


BATCH_ROUTES = [("rgb444", (3, 0)), ("blocks", (3, 0)), ("restart0", (0, 3))]


@pytest.mark.parametrize("route,how", BATCH_ROUTES, ids=[r for r, _ in BATCH_ROUTES])
def test_encoder_batches_at_the_output_limit(O, G, dlib, route, how, monkeypatch, capfd):
    """encode_batch and encode_batch_ptrs (the latter in chunks of two frames) on [flat, dense, flat] under a capacity between the two sizes return
    -1 and name the frame; the next batch of three flat frames on the same encoder is the oracle's; under a capacity of the dense frame's size all
    three frames are the oracle's. Batched launches (a result pair per frame) and a configuration the batch call codes frame by frame."""
    case = guard_case(route)
    dense, dense_jpeg, _ = limit_expected(case, "noise")
    flat, flat_jpeg, _ = limit_expected(case, "flat")
    other, other_jpeg, _ = limit_expected(case, "ramp")
    cap = (int(max(flat_jpeg.size, other_jpeg.size)) + int(dense_jpeg.size)) // 2
    assert max(flat_jpeg.size, other_jpeg.size) < cap < dense_jpeg.size
    p, pi = api_params(dlib, G, case)
    frame = dlib.image_size(pi)
    mixed, calm = [flat, dense, other], [flat, other, flat]
    calm_want = [flat_jpeg, other_jpeg, flat_jpeg]
    enc = capped_encoder(G, dlib, monkeypatch, cap, route)
    for ptrs in (False, True):
        enc.set_batch_chunk(2 if ptrs else 0)
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            enc.encode_batch_ptrs(p, pi, [np.array(r) for r in mixed]) if ptrs else enc.encode_batch(p, pi, np.concatenate(mixed), 3, frame)
        err = capfd.readouterr().err
        assert f"({int(dense_jpeg.size)} B)" in err and f"does not fit the output buffer ({cap} B)" in err, ptrs
        if how == (3, 0):
            assert "of frame 1 " in err
        got = enc.encode_batch_ptrs(p, pi, [np.array(r) for r in calm]) if ptrs else enc.encode_batch(p, pi, np.concatenate(calm), 3, frame)
        assert enc.last_batch() == how
        for f, (g, want) in enumerate(zip(got, calm_want)):
            assert g.size == want.size and np.array_equal(g, want), (ptrs, f)
    enc.close()
    enc = capped_encoder(G, dlib, monkeypatch, int(dense_jpeg.size), route)
    for ptrs in (False, True):
        enc.set_batch_chunk(2 if ptrs else 0)
        got = enc.encode_batch_ptrs(p, pi, [np.array(r) for r in mixed]) if ptrs else enc.encode_batch(p, pi, np.concatenate(mixed), 3, frame)
        assert enc.last_batch() == how
        for f, (g, want) in enumerate(zip(got, [flat_jpeg, dense_jpeg, other_jpeg])):
            assert g.size == want.size and np.array_equal(g, want), (ptrs, f)
    enc.close()


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
    """this file's CPU-tier tests once more on the AddressSanitizer + UBSan build of the execution model (the lane-per-segment kernel over stream
    windows with deep tables, the plane batches inside the token decoder, the clamp's arithmetic)"""
    env = dict(asan_env, GJ_EMU_LIB=ASAN_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-n", "4", "-m", "not gpu", "-p", "no:faulthandler",
                        "-p", "no:cacheprovider", "-k", "emu and not under_sanitizers"], capture_output=True, text=True, errors="replace",
                       timeout=1500, env=env, cwd=ROOT)
    tail = (r.stdout[-1500:] + "\n" + "\n".join(ln for ln in r.stderr.splitlines() if not ln.startswith("[GPUJPEG]"))[-3000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1500:]
