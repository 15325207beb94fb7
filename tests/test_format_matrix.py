"""The format-conversion matrix: every input pixel format against every coded sampling on the way in, every coded sampling against every requested
output on the way out, at sizes with partial MCUs on both edges -- the sampling and layout arithmetic of k_preprocess, k_encode_blocks<PLANAR / !PLANAR>,
k_postprocess / gj_pixel_store, k_copy_planes_out and the reduced-size, region and batch routes that share gj_pixel_store / gj_region_sample.

Every expectation is bit-exact against oracle/ (pinned to the reference for these cells by tests/test_oracle_vs_ref.py): stream bytes for encode; decoded
bytes, data_size and the reported ImageParameters for decode. No tolerances. Content is noise at q85 with a restart interval of 3 (and of 8 where only a
longer segment reaches a kernel: one scan per component has one block per MCU, and the tile kernels start at 4 blocks per segment).

Two observable differences from the reference are pinned here:
  * packed 4:2:2 (422-u8-p1020) of odd width is refused by encoder, decoder (full-size, region, batch) and oracle alike: the pixel kernels run over the
    width rounded up to a whole pixel pair while the image buffer holds width * height * 2 bytes (the note at CASES in tests/conftest.py says the same
    of the reference's input side);
  * planar 4:2:2 output through the per-pixel store indexes its chroma planes by row, W*H + y*((W+1)/2) + x/2 -- the layout raw_size, k_copy_planes_out
    and the fused PLANAR encoder use, byte-identical to the reference's W*H + pos/2 for even W. For odd W the reference's index makes pixel (W-1, y) of
    an even row and pixel (0, y+1) share a byte: a write-write race in its kernel (established from the index arithmetic and from the differing samples
    on the CPU execution model, not by watching a GPU disagree with itself).

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on the MI355X."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import api_params, oracle_image
from test_region_decode import check as region_check, perf_decoder, regions as region_regions
from test_scaled_decode import check as scaled_check

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")

Q, RI = 85, 3
RI_TILES = 8  # one scan per component: a segment of 8 blocks, which the kernels from pixels to tile streams take (4 .. 256)
SAMPLINGS = {
    "444": ((1, 1), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "420": ((2, 2), (1, 1), (1, 1)), "440": ((1, 2), (1, 1), (1, 1)),
    "411": ((4, 1), (1, 1), (1, 1)), "410": ((4, 2), (1, 1), (1, 1)), "mixed": ((2, 2), (2, 1), (1, 2)),
}
# four components (packed 4:4:4:4 input): the plain one, and the three samplings above that no kernel is specialised for with a fourth component
# (of the first one's factors, or 1x1 where an interleaved MCU would otherwise pass 16 blocks) -- in the reference these run its dynamic-sampling kernel with every factor set (tests/test_oracle_vs_ref.py)
SAMPLINGS4 = {"4444": ((1, 1),) * 4, "4114": ((4, 1), (1, 1), (1, 1), (4, 1)), "4101": ((4, 2), (1, 1), (1, 1), (1, 1)), "mixed4": ((2, 2), (2, 1), (1, 2), (2, 2))}
# partial MCUs on both edges for every sampling up to the 32x16 MCU of (4, 2); one pixel; one frame of whole MCUs of every sampling
SIZES = [(33, 35), (50, 21), (17, 9), (1, 1), (64, 32)]
EVEN_SIZES = [(34, 35), (50, 21), (18, 9), (2, 1), (64, 32)]  # packed 4:2:2 input: the next even width
OUTPUTS = [(0, 3), (1, 1), (1, 3), (2, 3), (2, 1), (3, 3), (3, 4), (4, 3), (5, 3), (5, 1), (6, 1), (-5, 0)]  # (pixel format, colour space); -5, 0: native, none
PF_NAME = {0: "u8", 1: "444p012", 2: "444p0p1p2", 3: "422p1020", 4: "422p0p1p2", 5: "420p0p1p2", 6: "4444", -5: "native"}


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


# ================================================================================================ the cells
@pytest.fixture
def OO(O):
    """the oracle (the name the tests of this file know it by)"""
    return O


def encode_case(w, h, pf, cs, il, sampling, csi=3, ri=RI):
    """a case in the form of conftest.CASES; sampling: a name of SAMPLINGS, or None for the format's own"""
    ss = None if sampling is None else tuple(SAMPLINGS4[sampling] if sampling in SAMPLINGS4 else SAMPLINGS[sampling])
    return (f"m_{w}x{h}_pf{pf}_cs{cs}_{sampling}_il{il}_csi{csi}_r{ri}", w, h, pf, cs, Q, ri, il, ss, csi)


def encode_cells():
    """(case, width_padding) of the encode matrix"""
    cells = []
    for il in (0, 1):
        for i, (w, h) in enumerate(SIZES):
            we = EVEN_SIZES[i][0]
            for pad in (0, 3):
                if il == 0:  # (grey has one scan)
                    cells.append((encode_case(w, h, 0, 3, 0, None), pad))
                cells.append((encode_case(w, h, 6, 1, il, None), pad))  # by default the encoder codes three components of the four
                for name in SAMPLINGS4:
                    cells.append((encode_case(w, h, 6, 1, il, name), pad))
            for name in SAMPLINGS:
                for cs in (1, 3):  # packed 4:4:4 holding RGB or YCbCr
                    for pad in (0, 3):
                        cells.append((encode_case(w, h, 1, cs, il, name), pad))
                for pf in (2, 4, 5):  # (no padding: the size of a planar image has none, gpujpeg_image_calculate_size)
                    cells.append((encode_case(w, h, pf, 3, il, name), 0))
                for pad in (0, 4):  # (a pixel pair is four bytes: the reference tells U from V by the byte offset modulo 4, so only whole pairs of padding)
                    cells.append((encode_case(we, h, 3, 3, il, name), pad))
            cells.append((encode_case(w, h, 1, 4, il, "444"), 0))  # a source that is not RGB, cs 4 -> internal 3: the fused kernels do not take it
            cells.append((encode_case(w, h, 1, 4, il, "420"), 3))
    # one scan per component at a restart interval the tile kernels take
    for w, h in SIZES[:2]:
        for pad in (0, 3):
            cells.append((encode_case(w, h, 1, 1, 0, None, ri=RI_TILES), pad))
            cells.append((encode_case(w, h, 1, 1, 0, "420", ri=RI_TILES), pad))
            cells.append((encode_case(w, h, 0, 3, 0, None, ri=RI_TILES), pad))
        for pf in (2, 4, 5):
            cells.append((encode_case(w, h, pf, 3, 0, None, ri=RI_TILES), 0))
    return cells


ENCODE_CELLS = encode_cells()


def make_cell(O, case, pad):
    """(raw image, the oracle's Image, the oracle's stream) of an encode cell -- read-only"""
    img = oracle_image(O, case, width_padding=pad)
    raw = O.noise(int(img.raw_size), seed=1000 + case[1] * 7 + case[2] * 3 + case[3])
    jpeg = O.encode(img, raw)
    raw.setflags(write=False)
    jpeg.setflags(write=False)
    return raw, img, jpeg


@functools.lru_cache(maxsize=None)
def cell_expected(O, case, pad):
    """make_cell, made once (the oracle in its default mode, which the product's tiers compare with)"""
    return make_cell(O, case, pad)


def encode_route(case, img, pad):
    """the default path of a cell: gj_tile_kernel and the kernels behind the coefficient planes (gj_encode.hip) restated from the geometry"""
    pf, cs = case[3], case[4]
    il, csi, n = img.interleaved, img.color_space_internal, img.comp_count
    samp = tuple((img.samp_h[c], img.samp_v[c]) for c in range(n))
    blocks = img.restart_interval * (sum(h * v for h, v in samp) if il else 1)
    segs_ok = img.restart_interval > 0 and 4 <= blocks <= 256
    same = cs == csi or 0 in (cs, csi)
    own = {0: ((1, 1),), 2: SAMPLINGS["444"], 4: SAMPLINGS["422"], 5: SAMPLINGS["420"]}.get(pf)
    copy = own is not None and samp == own and (n != 3 or cs == csi)  # gj_geom::no_transform for the encoder
    uyvy = (pf == 3 and n == 3 and same and samp == SAMPLINGS["422"] and img.comp[0].data_width == 2 * img.comp[1].data_width and
            img.comp[0].data_height == img.comp[1].data_height)
    rgb444 = pf == 1 and n == 3 and samp == SAMPLINGS["444"] and (same or (cs, csi) in ((1, 3), (1, 2), (1, 4), (3, 1)))
    blocks_mode = 1 if copy else 0 if pf == 1 and n == 3 and (same or (cs == 1 and csi in (2, 3, 4))) else -1
    if uyvy and il and segs_ok:
        return "uyvy422"
    if rgb444 and not il and segs_ok:
        return "rgb444"
    if segs_ok and blocks_mode >= 0:
        return "blocks_planar" if blocks_mode else "blocks"
    return "fused_uyvy422" if uyvy else "fused_rgb444" if rgb444 else "copy_planes" if copy else "preprocess"


TILE_ROUTES = ("uyvy422", "rgb444", "blocks", "blocks_planar")
ALL_ROUTES = set(TILE_ROUTES) | {"fused_uyvy422", "fused_rgb444", "copy_planes", "preprocess"}


def block_branches(img, w, h, pad, planar):
    """the branches of k_encode_blocks<planar> the blocks of an image take (gj_enc_tiles.hip; the image starts on a multiple of 4 bytes)"""
    seen = set()
    src_off = 0
    for c in range(img.comp_count):
        k = img.comp[c]
        sh, sv = img.max_h // k.h, img.max_v // k.v
        for by in range(k.data_height // 8):
            for bx in range(k.data_width // 8):
                if planar:  # a plane of the component's own samples, pitch = its width + padding
                    pitch = k.width + pad
                    interior = bx * 8 + 8 <= k.width and by * 8 + 8 <= k.height
                    aligned = (pitch | (src_off + by * 8 * pitch + bx * 8)) & 3 == 0
                    seen.add("partial" if not interior else "fast" if aligned else "unaligned")
                else:  # the pixels (x * sub_h, y * sub_v) of the packed image
                    pitch = w * 3 + pad
                    interior = bx * 8 * sh + 8 * sh <= w and (by * 8 + 7) * sv < h
                    seen.add("sub_h>2" if sh > 2 else "partial" if not interior else "fast" if pitch % 4 == 0 else "unaligned")
        src_off += (k.width + pad) * k.height
    return seen


# ================================================================================================ 1. the encode matrix
def test_the_matrix_reaches_what_it_is_for(OO):
    """From the geometry alone: the cells whose default path is k_encode_blocks put at least one block into each of its branches, in both
    instantiations -- a block that leaves the image (partial MCU), a component with sub_h > 2 (the slow branch), a block fetched by aligned loads
    (the fast branch) and one inside the image whose pitch or start is no multiple of 4 (width_padding = 3, an odd width) -- and every route of
    gj_tile_kernel and of the kernels behind the coefficient planes is the default path of at least one cell."""
    seen = {False: set(), True: set()}
    routes = set()
    for case, pad in ENCODE_CELLS:
        img = oracle_image(OO, case, width_padding=pad)
        route = encode_route(case, img, pad)
        routes.add(route)
        if route in ("blocks", "blocks_planar"):
            seen[route == "blocks_planar"] |= block_branches(img, case[1], case[2], pad, route == "blocks_planar")
    assert seen[True] == {"partial", "fast", "unaligned"}, seen[True]
    assert seen[False] == {"partial", "sub_h>2", "fast", "unaligned"}, seen[False]
    assert routes == ALL_ROUTES, routes


@pytest.mark.parametrize("il", [0, 1], ids=["scans", "interleaved"])
@pytest.mark.parametrize("pf", [0, 1, 2, 3, 4, 5, 6])
def test_encode_matrix(OO, G, dlib, pf, il):
    """Every cell of the encode matrix on the default path, with keep_coefficients() and with set_fused(False): the oracle's bytes. The route of the
    default path is restated from the geometry (encode_route) and checked against what the batch call reports: batched launches where a kernel from
    pixels to tile streams takes the cell, frame by frame through the coefficient planes otherwise -- so no cell goes the generic way unseen.
    (Grey is coded in one scan: that row's interleaved half is empty.)"""
    cells = [(case, pad) for case, pad in ENCODE_CELLS if case[3] == pf and case[7] == il]
    assert cells or (pf, il) == (0, 1)
    if pf == 6:  # the default drops the alpha channel; with four sampling factors all four components are coded
        assert {cell_expected(OO, case, pad)[1].comp_count for case, pad in cells} == {3, 4}
    encoders = {"default": G.Encoder(dlib), "keep": G.Encoder(dlib), "generic": G.Encoder(dlib)}
    encoders["keep"].keep_coefficients()
    encoders["generic"].set_fused(False)
    for case, pad in cells:
        raw, img, want = cell_expected(OO, case, pad)
        p, pi = api_params(dlib, G, case)
        pi.width_padding = pad
        assert dlib.image_size(pi) == raw.size == img.raw_size
        route = encode_route(case, img, pad)
        for how, e in encoders.items():
            got = e.encode(p, pi, raw)
            assert got.size == want.size and np.array_equal(got, want), (case[0], pad, how, route, got.size, want.size)
            got = e.encode_batch(p, pi, np.array(raw), 1, raw.size)
            assert got[0].size == want.size and np.array_equal(got[0], want), (case[0], pad, how, route, "batch of one")
            tiles = how == "default" and route in TILE_ROUTES  # (keep_coefficients() and set_fused(False) take no kernel from pixels to tile streams)
            assert e.last_batch() == ((1, 0) if tiles else (0, 1)), (case[0], pad, how, route, e.last_batch())
    for e in encoders.values():
        e.close()


# ================================================================================================ 2. the decode matrix
STREAM_KINDS = [(name, il) for name in SAMPLINGS for il in (0, 1)] + [("grey", 0), ("4444", 1), ("4444", 0)]


def make_stream(O, kind, il, w, h, seed=0, ri=RI):
    """the oracle's stream of a w x h noise image coded with the sampling `kind` -- read-only"""
    if kind == "grey":
        case = encode_case(w, h, 0, 3, 0, None, ri=ri)
    elif kind == "4444":
        case = encode_case(w, h, 6, 1, il, None, ri=ri)
        case = case[:8] + (((1, 1),) * 4,) + case[9:]
    else:
        case = encode_case(w, h, 1, 1, il, kind, ri=ri)
    img = oracle_image(O, case)
    jpeg = O.encode(img, O.noise(int(img.raw_size), seed=77 + seed + w + 3 * h))
    jpeg.setflags(write=False)
    return jpeg


@functools.lru_cache(maxsize=None)
def stream(O, kind, il, w, h, seed=0, ri=RI):
    """make_stream, made once (the oracle in its default mode)"""
    return make_stream(O, kind, il, w, h, seed, ri)


@functools.lru_cache(maxsize=None)
def stream_planes(O, kind, il, w, h, seed=0):
    """(coefficients, component planes) of a stream by the oracle: what the decoder's coefficient and sample planes hold once its kernels wrote them"""
    jpeg = stream(O, kind, il, w, h, seed)
    st = O.parse(jpeg)
    try:
        coefs = O.huffman_decode(st, jpeg)
        return coefs, O.idct(st, coefs).copy()
    finally:
        O.lib().gjo_stream_free(C.byref(st))


def native_format(kind, il):
    """the decoder's native output of a stream (gj_reader.c native_pixel_format, src/gpujpeg_reader.c:1494-1618): resolved at the frame header, before a
    scan header has said whether the scans are interleaved, so the planar layout of the three standard samplings and planar 4:4:4 for the others"""
    if kind == "grey":
        return 0
    if kind == "4444":
        return 6
    return {"444": 2, "422": 4, "420": 5}.get(kind, 2)


def oracle_decode(O, jpeg, pf, cs, kind, il):
    """(pixels, Image) of the oracle for the request, or None where it refuses"""
    if pf == -5:
        pf = native_format(kind, il)
    try:
        return O.decode(jpeg, pf, cs)
    except ValueError:
        return None


def decode_route(img, fused=True):
    """the IDCT side of a full-size decode restated (gj_launch_idct, gj_hip_decode_uses_planes): which kernel makes the pixels"""
    samp = tuple((img.comp[c].h, img.comp[c].v) for c in range(img.comp_count))
    same = img.color_space == img.color_space_internal or 0 in (img.color_space, img.color_space_internal)
    pair = same or (img.color_space_internal, img.color_space) in ((3, 1), (2, 1), (4, 1), (1, 3))
    if (fused and img.pixel_format == 3 and samp == SAMPLINGS["422"] and same and img.comp[0].data_width == 2 * img.comp[1].data_width and
            img.comp[0].data_height == img.comp[1].data_height):  # (gj_is_uyvy422: whole pixel pairs of blocks, which one scan per component need not have)
        return "uyvy422"
    if fused and img.pixel_format == 1 and samp == SAMPLINGS["444"] and pair:
        return "rgb444"
    planar = img.pixel_format in (0, 2, 4, 5)
    own = {0: ((1, 1),), 2: SAMPLINGS["444"], 4: SAMPLINGS["422"], 5: SAMPLINGS["420"]}.get(img.pixel_format)
    if planar and samp == own and not (img.comp_count >= 3 and img.color_space != img.color_space_internal):
        return "copy_planes"
    return "postprocess"


def check_decode(O, G, lib, dec, jpeg, pf, cs, kind, il):
    """one cell: the oracle's bytes, size and parameters -- or the refusal of both"""
    want = oracle_decode(O, jpeg, pf, cs, kind, il)
    dec.set_output_format(cs, pf)
    if want is None:
        with pytest.raises(RuntimeError):
            dec.decode(jpeg)
        return None
    raw, img = want
    px, pi = dec.decode(jpeg)
    assert (pi.width, pi.height, pi.pixel_format, pi.color_space) == (img.width, img.height, img.pixel_format, img.color_space), \
        (pf, cs, pi.width, pi.height, pi.pixel_format, pi.color_space)
    assert px.size == raw.size == img.raw_size == lib.image_size(pi), (pf, cs, px.size, raw.size)
    diff = np.flatnonzero(px != raw)
    assert diff.size == 0, (PF_NAME[pf], cs, int(diff.size), diff[:8].tolist())
    return img


def marker_seed(O, kind, il, w, h):
    """a second stream of the geometry whose coefficients and samples both differ from those of stream 0"""
    c0, p0 = stream_planes(O, kind, il, w, h)
    for seed in range(1, 20):
        c, p = stream_planes(O, kind, il, w, h, seed)
        if not np.array_equal(c, c0) and not np.array_equal(p, p0):
            return seed
    raise AssertionError("no second stream")


def observed_route(O, dec, kind, il, w, h, seed):
    """Which buffers the last decode (of stream 0) wrote, after the marker stream `seed` had gone through the generic kernels of the same decoder and
    left ITS coefficients and samples in them: the entropy decoder stores coefficient planes or hands tokens to the IDCT, and the IDCT side stores
    component planes for the generic pixel kernels (k_copy_planes_out, k_postprocess) or goes straight to pixels (the fused kernels).
    -> ("planes" | "tokens", "generic" | "fused"). What these buffers cannot tell apart is k_copy_planes_out from k_postprocess: that part of
    decode_route stays a restatement (gj_geom::no_transform)."""
    (c0, p0), (cm, pm) = stream_planes(O, kind, il, w, h), stream_planes(O, kind, il, w, h, seed)
    c, p = dec.coefficients(c0.size), dec.planes(p0.size)
    entropy = "planes" if np.array_equal(c, c0) else "tokens" if np.array_equal(c, cm) else "?"
    pixels = "generic" if np.array_equal(p, p0) else "fused" if np.array_equal(p, pm) else "?"
    return entropy, pixels


def expected_buffers(img, fused, env, il):
    """decode_route, and gj_hip_decode's choice of token mode under the developer settings `env` (forced token mode takes the token-fed IDCT where
    there is one: one scan per component of the fused 4:4:4 configuration; the interleaved packed 4:2:2 one through the lane-per-segment decoder)"""
    route = decode_route(img, fused)
    tokens = fused and env.get("GJ_DEC_TOKENS") == "1" and ((route == "rgb444" and not il) or (route == "uyvy422" and il and env.get("GJ_DEC_SEQ") == "1"))
    return ("tokens" if tokens else "planes", "fused" if route in ("rgb444", "uyvy422") else "generic"), ("tok_" if tokens else "") + route


DECODE_PATHS = [("fused", True, {}), ("generic", False, {})]
TOKEN_PATHS = {("444", 0): ("tokens", True, {"GJ_DEC_TOKENS": "1"}), ("422", 1): ("tokens_seq", True, {"GJ_DEC_TOKENS": "1", "GJ_DEC_SEQ": "1"})}


def decode_cells(O, G, dlib, monkeypatch, kind, il, size):
    """every cell of one stream; -> the routes its cells were SEEN to take (observed_route agreed with the restatement)"""
    w, h = size
    jpeg = stream(O, kind, il, w, h)
    seed = marker_seed(O, kind, il, w, h)
    marker = stream(O, kind, il, w, h, seed)
    seen = set()
    for name, fused, env in DECODE_PATHS + ([TOKEN_PATHS[(kind, il)]] if (kind, il) in TOKEN_PATHS else []):
        for var in ("GJ_DEC_TOKENS", "GJ_DEC_SEQ"):
            monkeypatch.delenv(var, raising=False)
        for var, value in env.items():
            monkeypatch.setenv(var, value)
        dec = G.Decoder(dlib)
        refused = 0
        for pf, cs in OUTPUTS:
            if oracle_decode(O, jpeg, pf, cs, kind, il) is not None:  # the marker through the generic kernels, in the cell's own format
                dec.set_fused(False)
                check_decode(O, G, dlib, dec, marker, pf, cs, kind, il)
                assert observed_route(O, dec, kind, il, w, h, seed) == ("tokens", "fused"), "the marker's own values are in both buffers"
            dec.set_fused(fused)
            img = check_decode(O, G, dlib, dec, jpeg, pf, cs, kind, il)
            if img is None:
                refused += 1
                # the decoder decodes the next stream correctly
                check_decode(O, G, dlib, dec, stream(O, "420", 1, 50, 21), 1, 1, "420", 1)
                continue
            buffers, route = expected_buffers(img, fused, env, il)
            assert observed_route(O, dec, kind, il, w, h, seed) == buffers, (name, PF_NAME[pf], cs, route)
            seen.add(route)
        assert refused == (2 if w % 2 else 0), (name, refused)  # (packed 4:2:2 in two colour spaces, of the odd widths: nothing else is refused)
        dec.close()
    return seen


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("kind,il", STREAM_KINDS, ids=["%s_%s" % (k, "il" if i else "scans") for k, i in STREAM_KINDS])
def test_decode_matrix(OO, G, dlib, kind, il, size, monkeypatch):
    """Every requested output of every stream through the fused and the generic kernels, and with token mode forced where a token-fed IDCT exists: the
    4:4:4 stream in one scan per component (k_idct_tok_rgb444) and the interleaved 4:2:2 stream (k_idct_tok_uyvy422, through the lane-per-segment
    decoder). Every cell's route, restated from the geometry, is checked against what the decoder's buffers show (observed_route), so a cell cannot
    go another way unseen."""
    assert decode_cells(OO, G, dlib, monkeypatch, kind, il, size)


def test_decode_matrix_reaches_every_pixel_kernel(OO, G, dlib, monkeypatch):
    """The cells of two streams of the matrix are seen to take the token-fed and the fused 4:4:4 kernel, both packed 4:2:2 kernels and the generic
    chain, which by gj_geom::no_transform ends in k_copy_planes_out (the 4:2:2 stream's own planar layout) or in k_postprocess."""
    seen = decode_cells(OO, G, dlib, monkeypatch, "444", 0, (50, 21)) | decode_cells(OO, G, dlib, monkeypatch, "422", 1, (50, 21))
    assert seen == {"rgb444", "tok_rgb444", "uyvy422", "tok_uyvy422", "copy_planes", "postprocess"}, seen


# ================================================================================================ 3. the same outputs through the other pixel stages
THREE_STREAMS = [("444", 0), ("420", 1), ("411", 0)]
THREE_IDS = ["444_scans", "420_il", "411_scans"]


@pytest.mark.parametrize("kind,il", THREE_STREAMS, ids=THREE_IDS)
@pytest.mark.parametrize("s", [2, 8])
def test_reduced_size_outputs(OO, G, dlib, kind, il, s):
    """Reduced-size decode of a 66x35 stream: 33x18 at 1/2 and 9x5 at 1/8, an odd width out of an even one. Expected: the oracle's coefficients
    through the definition of tests/test_scaled_decode.py and the oracle's postprocessor; packed 4:2:2 of the odd reduced width is refused."""
    jpeg = stream(OO, kind, il, 66, 35)
    for fused in (True, False):
        dec = G.Decoder(dlib)
        dec.set_fused(fused)
        for pf, cs in OUTPUTS:
            if pf == -5:
                pf = native_format(kind, il)
            got = scaled_check(OO, G, dlib, jpeg, pf, cs, s, dec)
            assert (got is None) == (pf == 3), (pf, cs)
        dec.close()


@pytest.mark.parametrize("kind,il", THREE_STREAMS, ids=THREE_IDS)
@pytest.mark.parametrize("size", SIZES[:2], ids=["33x35", "50x21"])
def test_region_outputs(OO, G, dlib, kind, il, size):
    """Region decode of one interior odd rectangle and of the bottom-right corner (tests/test_region_decode.py: regions): the crop of the oracle's full
    decode. Packed 4:2:2 from the even width only (the odd one: test_decoder_refuses_odd_width_packed_422)."""
    w, h = size
    jpeg = stream(OO, kind, il, w, h)
    for fused in (True, False):
        dec = G.Decoder(dlib)
        dec.set_fused(fused)
        for pf, cs in OUTPUTS:
            if pf == -5:
                pf = native_format(kind, il)
            if pf == 3 and w % 2:
                continue
            full = OO.decode(jpeg, pf, cs)
            rs = region_regions(w, h, pf)
            assert rs[0] == (0, 0, w, h) and len(rs) >= 4
            interior, corner = rs[1], rs[3]
            assert corner[0] + corner[2] == w and corner[1] + corner[3] == h and 0 < interior[0] and interior[0] + interior[2] < w
            for reg in (interior, corner):
                region_check(OO, G, dlib, jpeg, pf, cs, reg, dec, full)
        dec.close()


BATCH_SIZES = ((129, 67), (130, 67))  # (odd for the formats that take it, even for packed 4:2:2)


@pytest.mark.parametrize("kind,il", THREE_STREAMS, ids=THREE_IDS)
def test_batch_outputs(OO, G, dlib, kind, il):
    """decode_batch of three frames to packed and planar 4:4:4, planar 4:2:2 and 4:2:0 at 129x67 and to packed 4:2:2 at 130x67: every frame is the
    oracle's decode of its stream, and the call reports that frames 1 and 2 went through the batched launches (frame blockIdx.z of the pixel kernels;
    with host output frame 0 goes the ordinary way first and leaves the header to launch on). The frames are larger than the matrix's: the batched
    launches run on the device's marker scan, which takes a stream whose scans' markers lie in different chunks of it -- one scan per component of
    33x35 or 50x21 is too short for that, and such a batch is decoded frame by frame, which test_decode_matrix covers."""
    for (w, h), outs in zip(BATCH_SIZES, ([(1, 1), (2, 3), (4, 3), (5, 3)], [(3, 3)])):
        streams = [stream(OO, kind, il, w, h, seed=f) for f in range(3)]
        for pf, cs in outs:
            dec = G.Decoder(dlib)
            dec.set_output_format(cs, pf)
            for rep in range(2):  # (the second call has a cached header from the start)
                frames, pi = dec.decode_batch(streams)
                assert dec.last_batch() == (2, 1), (w, h, pf, cs, rep, dec.last_batch())
                for f, px in enumerate(frames):
                    raw, img = OO.decode(streams[f], pf, cs)
                    assert (pi.width, pi.height, pi.pixel_format, pi.color_space) == (w, h, pf, cs)
                    assert px.size == raw.size and np.array_equal(px, raw), (pf, cs, rep, f, int(np.count_nonzero(px != raw)))
            dec.close()


# ================================================================================================ 4. packed 4:2:2 of odd width
REFUSAL = "needs an even width"


def test_oracle_refuses_odd_width_packed_422(OO):
    """the restatement refuses what the product refuses (it used to run its pixel loops past raw_size)"""
    with pytest.raises(ValueError):
        OO.make_image(33, 35, pixel_format=3, color_space=3)
    with pytest.raises(ValueError):
        OO.parse(stream(OO, "422", 1, 33, 35), 3, 3)
    assert OO.make_image(34, 35, pixel_format=3, color_space=3).raw_size == 34 * 35 * 2
    assert OO.parse(stream(OO, "422", 1, 33, 35), 4, 3).img.raw_size == 33 * 35 + 2 * 17 * 35


def test_encoder_refuses_odd_width_packed_422(OO, G, dlib, capfd):
    """One message naming the size, nothing launched (the kernel times of the call before are still the ones reported), and the same encoder
    then codes a valid image. The call never reaches a kernel: by gj_geom_init's raw_width the kernels would read 2 * height bytes past the image."""
    good = encode_case(34, 35, 3, 3, 1, None)
    raw, img, want = cell_expected(OO, good, 0)
    for how in ("default", "generic"):
        enc = G.Encoder(dlib)
        enc.set_fused(how == "default")
        p, pi = api_params(dlib, G, good)
        p.perf_stats = 1
        assert np.array_equal(enc.encode(p, pi, raw), want)
        times = enc.kernel_times()
        for w, h in ((33, 35), (1, 1)):
            bad_p, bad_pi = api_params(dlib, G, encode_case(w, h, 3, 3, 1, None))
            bad_p.perf_stats = 1
            bad_raw = np.zeros((w + 1) * h * 2, np.uint8)  # (room for the rounded-up width, whatever the call does)
            capfd.readouterr()
            with pytest.raises(RuntimeError):
                enc.encode(bad_p, bad_pi, bad_raw)
            err = capfd.readouterr().err
            assert err.count("[Error]") >= 1 and err.count(REFUSAL) == 1 and f"{w}x{h}" in err, err
            with pytest.raises(RuntimeError):
                enc.encode_batch(bad_p, bad_pi, np.concatenate([bad_raw, bad_raw]), 2, bad_raw.size)
            assert REFUSAL in capfd.readouterr().err
            assert enc.kernel_times() == times
            assert np.array_equal(enc.encode(p, pi, raw), want)
            times = enc.kernel_times()
        enc.close()


def raw_decode(G, lib, dec, jpeg):
    """the decode call itself: (return code, the output structure, whose data_size held a sentinel going in)"""
    out = G.DecoderOutput()
    out.type = G.DECODER_OUTPUT_INTERNAL_BUFFER
    out.data_size = 0xA5A5
    jpeg = np.ascontiguousarray(jpeg)
    return lib.L.gpujpeg_decoder_decode(dec.h, jpeg.ctypes.data, jpeg.size, C.byref(out)), out


@pytest.mark.parametrize("kind,il", [("444", 0), ("422", 1), ("420", 1)], ids=["444_scans", "422_il", "420_il"])
def test_decoder_refuses_odd_width_packed_422(OO, G, dlib, kind, il, capfd):
    """Full-size call, region call (a rectangle that ends at the right edge of the odd image) and decode_batch, cold and with a header to launch on:
    one message naming the size, the output's data_size untouched, the kernel times and region statistics of the call before still the ones
    reported, and the same decoder then decodes. These calls never reach a kernel:
    by gj_geom_init's raw_width a 33x35 image would be stored up to byte 2379 of 2310."""
    odd = [stream(OO, kind, il, 33, 35, seed=f) for f in range(3)]
    even = stream(OO, kind, il, 50, 21)
    want_even = OO.decode(even, 3, 3)[0]
    want_odd = OO.decode(odd[0], 4, 3)[0]
    for fused in (True, False):
        dec = perf_decoder(G, dlib)
        dec.set_fused(fused)
        dec.set_output_format(3, 3)
        for warm in (False, True):
            if warm:
                rc, out = raw_decode(G, dlib, dec, even)
                assert rc == 0 and out.data_size == want_even.size
            before = (dec.kernel_times(), dec.region_stats())
            assert warm == (before[0] is not None)
            # the full-size call
            capfd.readouterr()
            rc, out = raw_decode(G, dlib, dec, odd[0])
            err = capfd.readouterr().err
            assert rc != 0 and out.data_size == 0xA5A5 and err.count(REFUSAL) == 1 and "33x35" in err, (rc, out.data_size, err)
            # the region call: up to the right edge of the odd image the rectangle is odd
            assert dec.set_option("dec_opt_region", "16,3,17,9") == 0
            rc, out = raw_decode(G, dlib, dec, odd[0])
            err = capfd.readouterr().err
            assert rc != 0 and out.data_size == 0xA5A5 and err.count(REFUSAL) == 1 and "17x9" in err, (rc, out.data_size, err)
            assert dec.set_option("dec_opt_region", "full") == 0
            # decode_batch, and a batch of regions
            with pytest.raises(RuntimeError):
                dec.decode_batch(odd)
            err = capfd.readouterr().err
            assert err.count(REFUSAL) == 1 and "33x35" in err, err
            with pytest.raises(RuntimeError):
                dec.decode_batch_regions(odd, [(16, 3)] * 3, 17, 9)
            assert REFUSAL in capfd.readouterr().err
            assert (dec.kernel_times(), dec.region_stats()) == before
            # the same decoder, valid requests
            px, pi = dec.decode(even)
            assert (pi.width, pi.height, pi.pixel_format) == (50, 21, 3) and np.array_equal(px, want_even)
        dec.set_output_format(3, 4)
        px, pi = dec.decode(odd[0])
        assert (pi.width, pi.height, pi.pixel_format) == (33, 35, 4) and np.array_equal(px, want_odd)
        dec.close()
