"""Crop-and-resize with the antialiased resample (dec_opt_resize_filter = antialias; gpujpeg_amd_ext.h).

The definition of a frame's result is the triangle filter stated in the header -- half-pixel centres, support stretched by w / OW when reducing, exact
rational weights renormalised by their sum, one rounding -- over what the single-frame region call returns for the frame's rectangle. Expected bytes are
a numpy restatement of that definition (aa_image below, int64 throughout: 2 S + U V < 2^62) applied to the cropped ORACLE decode (oracle.decode + a numpy
crop, no product code), never the product's own bilinear output; every comparison with the library is byte for byte.

Two tiers with the same bodies, like test_crop_resize.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on
the MI355X. The damaged stream runs on the CPU tier only."""
import ctypes as C

import numpy as np
import pytest

from conftest import natural_image, oracle_image
from test_crop_resize import BPP, diffs, raw_call, resize_image
from test_crop_resize_tensor import BF16, CHW, F16, F32, FORMAT_IDS, FORMATS, HWC, IMAGENET, tensor_raw_call, tensors_equal
from test_region_batch import dlib, emu, frames_of, new_decoder, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import OPT, case_named, crop, damaged_restart_markers, opt_value, perf_decoder

FILTER, PRESCALE = "dec_opt_resize_filter", "dec_opt_resize_prescale"

# streams of this file: small, every one with a restart interval (the batched launches take them)
#        name             w    h    pf cs q   ri il subsampling                    internal
A444 = ("aa_444", 200, 120, 1, 1, 75, 5, 0, None, 3)
A420 = ("aa_420_il_odd", 161, 97, 1, 1, 75, 3, 1, [(2, 2), (1, 1), (1, 1)], 3)
AGRAY = ("aa_gray", 48, 40, 0, 3, 75, 2, 0, None, 3)
AWIDE = ("aa_444_wide", 272, 256, 1, 1, 75, 8, 0, None, 3)
ANAT = ("aa_420_il_natural", 640, 368, 1, 1, 75, 20, 1, [(2, 2), (1, 1), (1, 1)], 3)
A422 = case_named("rgb_to_422_nonil")  # 200 x 100, restart interval 5


# ================================================================================================ the definition, in numpy
def aa_weights(n_src, n_out):
    """u_i(k) for every output sample i and source sample k of one axis: (n_out, n_src) int64"""
    d = max(n_src, n_out)
    i = np.arange(n_out, dtype=np.int64)[:, None]
    k = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, 2 * d - np.abs((2 * k + 1) * n_out - (2 * i + 1) * n_src))


def aa_channels(c, ow, oh):
    """c: (h, w, channels) uint8 -> (oh, ow, channels) uint8 by the definition"""
    h, w = c.shape[:2]
    u, v = aa_weights(w, ow), aa_weights(h, oh)
    U, V = u.sum(1), v.sum(1)
    assert U.min() >= max(w, ow) and V.min() >= max(h, oh)
    rows = np.tensordot(c.astype(np.int64), u, axes=([1], [1]))  # (h, channels, ow): sum_k u_i(k) C[l][k]
    S = np.tensordot(v, rows, axes=([1], [0])).transpose(0, 2, 1)  # (oh, ow, channels)
    uv = (V[:, None] * U[None, :])[:, :, None]
    assert float(uv.max()) * 511 < 2.0 ** 63
    return ((2 * S + uv) // (2 * uv)).astype(np.uint8)


def aa_image(c, w, h, pf, ow, oh, mirror=False):
    """the w x h image c of pixel format pf (no line padding) -> the ow x oh image of the same format, mirrored horizontally on request"""
    if pf in BPP:
        r = aa_channels(c.reshape(h, w, BPP[pf]), ow, oh)
        return np.ascontiguousarray(r[:, ::-1] if mirror else r).reshape(-1)
    assert pf == 2
    r = aa_channels(c.reshape(3, h, w).transpose(1, 2, 0), ow, oh)
    return np.ascontiguousarray((r[:, ::-1] if mirror else r).transpose(2, 0, 1)).reshape(-1)


def aa_expected(O, streams, rects, ow, oh, pf=None, cs=None, mirror=None):
    """the restatement over the cropped oracle decodes -> one array per frame"""
    out = []
    for f, (jpeg, rect) in enumerate(zip(streams, rects)):
        raw, img = O.decode(jpeg, -1 if pf is None else pf, -1 if cs is None else cs)
        c = crop(raw, img.width, img.height, img.pixel_format, rect)
        out.append(aa_image(c, rect[2], rect[3], img.pixel_format, ow, oh, bool(mirror and mirror[f])))
    return out


def aa_decoder(G, lib, pf=None, cs=None, align=None, perf=False):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib)
    if pf is not None:
        dec.set_output_format(cs, pf)
    if align:
        assert dec.set_option("dec_opt_alignment_bytes", str(align)) == 0
    assert dec.set_option(FILTER, "antialias") == 0
    return dec


# ================================================================================================ 1. the definition alone
def test_definition_is_the_identity_at_equal_size():
    rng = np.random.default_rng(1)
    for w, h in ((1, 1), (7, 5), (64, 48), (100, 3)):
        c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(aa_channels(c, w, h), c)
        assert np.array_equal(aa_image(c.reshape(-1), w, h, 1, w, h), c.reshape(-1))
        assert np.array_equal(aa_image(c.reshape(-1), w, h, 1, w, h, True), c[:, ::-1].reshape(-1))


def test_definition_keeps_a_constant():
    for value in (0, 1, 127, 254, 255):
        for (w, h), (ow, oh) in (((100, 45), (32, 24)), ((9, 7), (64, 48)), ((301, 9), (7, 5)), ((1, 33), (1, 1)), ((256, 256), (1, 1)), ((5, 300), (13, 2))):
            assert np.all(aa_channels(np.full((h, w, 2), value, np.uint8), ow, oh) == value), (value, w, h, ow, oh)


def test_definition_against_torch_antialias():
    """<= 0.501 levels from float64 torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True) -- the same rational value
    rounded once -- over the shapes of test_crop_resize.test_definition_against_float_and_torch"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(2)
    crops = []
    for w, h in ((100, 45), (37, 150), (9, 7), (1, 1), (1, 33), (41, 1), (301, 9)):
        crops.append(natural_image(w, h, 3, seed=w + h).reshape(h, w, 3))
        crops.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    worst = 0.0
    for c in crops:
        for ow, oh in ((32, 24), (64, 48), (7, 5), (1, 1), (13, 5), (149, 211)):
            r = aa_channels(c, ow, oh).astype(np.float64)
            t = F.interpolate(torch.from_numpy(c.astype(np.float64)).permute(2, 0, 1)[None], size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
            worst = max(worst, float(np.max(np.abs(r - t[0].permute(1, 2, 0).numpy()))))
    print(f"largest difference from torch's antialiased bilinear filter in float64: {worst} levels")
    assert worst <= 0.501


def exact_bilinear(c, ow, oh):
    """bilinear interpolation with half-pixel centres and edge clamp, exact rational weights, rounded once (half up): for w <= ow and h <= oh"""
    h, w = c.shape[:2]

    def axis(n_src, n_out):
        n = np.clip((2 * np.arange(n_out, dtype=np.int64) + 1) * n_src - n_out, 0, (n_src - 1) * 2 * n_out)
        p0 = n // (2 * n_out)
        return p0, np.minimum(p0 + 1, n_src - 1), n - p0 * 2 * n_out

    x0, x1, fx = axis(w, ow)
    y0, y1, fy = axis(h, oh)
    c = c.astype(np.int64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = c[y0][:, x0] * (2 * ow - fx) + c[y0][:, x1] * fx
    bot = c[y1][:, x0] * (2 * ow - fx) + c[y1][:, x1] * fx
    den = 4 * ow * oh
    return ((2 * (top * (2 * oh - fy) + bot * fy) + den) // (2 * den)).astype(np.uint8)


def test_definition_is_exact_bilinear_when_enlarging():
    rng = np.random.default_rng(3)
    for (w, h), (ow, oh) in (((9, 7), (64, 48)), ((1, 1), (7, 5)), ((5, 7), (5, 20)), ((31, 24), (32, 24)), ((2, 3), (149, 211)), ((1, 9), (9, 9))):
        c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(aa_channels(c, ow, oh), exact_bilinear(c, ow, oh)), (w, h, ow, oh)


# ================================================================================================ 2. the host helper
@pytest.mark.parametrize("n_src,n_out", [(7, 5), (5, 7), (1, 9), (9, 1), (301, 32), (100, 100), (256, 1), (65535, 256), (40000, 157)])
def test_host_helper_equals_the_dense_formula(G, emu, n_src, n_out):
    big = n_src > 1000
    d = max(n_src, n_out)
    k = np.arange(n_src, dtype=np.int64)
    most = 0
    for i in ((0, n_out // 2, n_out - 1) if big else range(n_out)):
        u = np.maximum(0, 2 * d - np.abs((2 * k + 1) * n_out - (2 * i + 1) * n_src))
        nz = np.flatnonzero(u)
        first, weights, total = G.resize_weights(emu, n_src, n_out, i)
        assert first == nz[0] and len(weights) == nz[-1] - nz[0] + 1 == nz.size, (i, first, len(weights), nz[0], nz[-1])  # (tight, and a run without holes)
        assert weights == [int(x) for x in u[nz]] and total == int(u.sum()) and total >= d, i
        with pytest.raises(ValueError):
            G.resize_weights(emu, n_src, n_out, i, capacity=len(weights) - 1)
        most = max(most, total)
    if (n_src, n_out) == (40000, 157):
        assert 255 * most > 2 ** 32, "the row sums of this pair were meant to pass 32 bits"
    assert G.resize_weights(emu, n_src, n_out, n_out) is None and G.resize_weights(emu, n_src, n_out, -1) is None


def test_host_helper_refuses_what_the_call_refuses(G, emu):
    assert G.resize_weights(emu, 257, 1, 0) is None and G.resize_weights(emu, 256, 1, 0) is not None
    assert G.resize_weights(emu, 0, 4, 0) is None and G.resize_weights(emu, 4, 0, 0) is None
    assert G.resize_weights(emu, 65536, 256, 0) is None and G.resize_weights(emu, 100, 16385, 0) is None


# ================================================================================================ 3. rectangles, formats, samplings
def breaking_rects(w, h, ow, oh):
    """the whole image; one pixel; one pixel wide and full height; an odd origin ending at the bottom-right corner; narrower than the output and higher
    than it (where the output is wider than a pixel); equal to the output; a ratio that is no integer"""
    return [(0, 0, w, h), (w // 2 | 1, h // 2 | 1, 1, 1), (w // 3 | 1, 0, 1, h), ((w - 41) | 1, (h - 29) | 1, w - ((w - 41) | 1), h - ((h - 29) | 1)),
            (5, 3, max(1, ow - 3), min(h - 3, 2 * oh + 5)), (8, 9, ow, oh), (3, 2, min(157, w - 3), min(93, h - 2))]


MIRROR = [1, 0, 1, 0, 0, 1, 1]
# (id, case, output pixel format, colour space, OW, OH, line alignment)
CONFIGS = [("444_to_rgb", A444, 1, 1, 32, 24, 0), ("422_nonil_to_planar_ycbcr", A422, 2, 3, 7, 5, 0), ("420_il_odd_to_rgb", A420, 1, 1, 64, 40, 0),
           ("420_il_odd_to_rgba_1x1", A420, 6, 1, 1, 1, 0), ("gray_to_u8_aligned", AGRAY, 0, 3, 7, 5, 16), ("gray_to_rgb", AGRAY, 1, 1, 32, 24, 0),
           ("planar444_no_transform", case_named("planar444_in"), 2, 3, 32, 24, 0)]


@pytest.mark.parametrize("ident,case,pf,cs,ow,oh,align", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_rectangles_formats_samplings(O, G, dlib, ident, case, pf, cs, ow, oh, align):
    w, h = case[1], case[2]
    rects = breaking_rects(w, h, ow, oh)
    assert all(x >= 0 and y >= 0 and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h for x, y, rw, rh in rects), rects
    assert rects[3][0] & 1 and rects[3][1] & 1 and rects[3][0] + rects[3][2] == w and rects[3][1] + rects[3][3] == h
    assert ow == 1 or (rects[4][2] < ow and rects[4][3] > oh)
    streams = frames_of(O, case, 7, seed=300)
    want = aa_expected(O, streams, rects, ow, oh, pf, cs, MIRROR)
    # the rectangle equal to the output: the bytes of the single region call (mirrored here), which are the cropped oracle decode
    raw5, img5 = O.decode(streams[5], pf, cs)
    assert np.array_equal(want[5], resize_image(crop(raw5, w, h, pf, rects[5]), ow, oh, pf, ow, oh, True))
    single = new_decoder(G, dlib, pf, cs)
    assert single.set_option(OPT, opt_value(rects[5])) == 0
    assert np.array_equal(resize_image(single.decode(streams[5])[0], ow, oh, pf, ow, oh, True), want[5])
    single.close()
    bpp = BPP.get(pf)
    pad = (-(ow * bpp)) % align if align else 0

    def pixels(frames):  # (dec_opt_alignment_bytes pads the output's lines: what lies in the padding is nobody's)
        return [px[:oh * (ow * bpp + pad)].reshape(oh, ow * bpp + pad)[:, :ow * bpp].reshape(-1) for px in frames] if pad else frames

    dec = aa_decoder(G, dlib, pf, cs, align, perf=True)
    dec.set_batch_chunk(3)
    for rep in range(2):  # (the first call: frame 0 through the single-frame route; the second: every frame through the batched launches, three at a time)
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
        assert (pi.width, pi.height, pi.pixel_format, pi.width_padding) == (ow, oh, pf, pad) and (pad != 0) == bool(align)
        assert same(pixels(got), want), (rep, diffs(pixels(got), want))
        batched, single_n = dec.last_batch()
        assert batched + single_n == 7 and single_n <= 1, (batched, single_n)
        assert dec.idct_path() == 7 and dec.prescales() == [1] * 7 and dec.region_stats()[0] == 1
    dec.close()


# ================================================================================================ 4. the 64-bit path, the ratio's limit
def test_ratio_256_and_the_64_bit_products(O, G, dlib, capfd):
    streams = frames_of(O, AWIDE, 3, seed=310)
    rects = [(7, 0, 256, 256), (16, 100, 256, 16), (3, 5, 100, 50)]
    _, _, U = G.resize_weights(dlib, 256, 1, 0)
    assert U * U > 2 ** 32, "U V of the first frame was meant to need 64 bits"
    want = aa_expected(O, streams, rects, 1, 1)
    dec = aa_decoder(G, dlib)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, 1, 1, mirror=[0, 1, 0])
        assert (pi.width, pi.height) == (1, 1) and same(got, want), (rep, got, want)
    for cold in (False, True):
        if cold:
            dec.close()
            dec = aa_decoder(G, dlib)
        out = np.full(3 * 16, 0xA5, np.uint8)
        capfd.readouterr()
        assert raw_call(G, dlib, dec, streams, [rects[0], (15, 100, 257, 16), rects[2]], 1, 1, out, 16) == -1
        err = capfd.readouterr().err
        assert np.all(out == 0xA5) and "Frame 1 " in err, err
        assert raw_call(G, dlib, dec, streams, [rects[0], (15, 0, 16, 257 - 1), (0, 0, 16, 256)], 1, 1, out, 16) == 0  # (256 along the other axis)
        assert np.all(out.reshape(3, 16)[:, 3:] == 0xA5)
    got, _ = dec.decode_batch_crop_resize(streams, rects, 1, 1, mirror=[0, 1, 0])
    assert same(got, want)
    dec.close()


def test_row_sums_beyond_32_bits(O, G, dlib):
    """a 40 000 x 8 grey image of bright pixels resampled to 157 columns: U_i is about 20 million, the weighted sum of a row about 5 * 10^9 -- the
    kernel has to take its 64-bit row sums for this frame, and takes the 32-bit ones for its narrow neighbour in the same launch"""
    case = ("aa_gray_40000", 40000, 8, 0, 3, 90, 100, 0, None, 3)
    raws = [(255 - O.noise(40000 * 8, seed=380 + f) % 16).astype(np.uint8) for f in range(3)]
    streams = [O.encode(oracle_image(O, case), raw) for raw in raws]
    rects = [(0, 0, 40000, 8), (17, 1, 39983, 7), (20000, 2, 300, 5)]
    _, weights, U = G.resize_weights(dlib, 40000, 157, 78)
    assert U * 240 > 2 ** 32 and len(weights) > 500
    want = aa_expected(O, streams, rects, 157, 2, mirror=[0, 1, 0])
    assert min(int(w.min()) for w in want) >= 200
    dec = aa_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, 157, 2, mirror=[0, 1, 0])
        assert same(got, want), (rep, diffs(got, want))
    dec.close()


# ================================================================================================ 5. fallbacks
def both_filters(G, lib, streams, rects, ow, oh, mirror=None, reps=2):
    """the call under both filters on two decoders of the same age -> the antialiased frames, after asserting that the routing was the same"""
    a, b = aa_decoder(G, lib, perf=True), perf_decoder(G, lib)
    for rep in range(reps):
        got, _ = a.decode_batch_crop_resize(streams, rects, ow, oh, mirror=mirror)
        b.decode_batch_crop_resize(streams, rects, ow, oh, mirror=mirror)
        assert a.last_batch() == b.last_batch() and a.region_stats() == b.region_stats(), (rep, a.last_batch(), b.last_batch())
        assert (a.idct_path(), b.idct_path()) == (7, 5)
        yield rep, got, a.last_batch()
    a.close()
    b.close()


def test_restart_interval_0_goes_frame_by_frame(O, G, dlib):
    streams = frames_of(O, case_named("rgb_restart0"), 3, seed=60)
    rects = [(0, 0, 100, 60), (60, 35, 40, 25), (33, 17, 11, 30)]
    want = aa_expected(O, streams, rects, 20, 16, mirror=[0, 1, 0])
    for rep, got, counts in both_filters(G, dlib, streams, rects, 20, 16, mirror=[0, 1, 0]):
        assert same(got, want), (rep, diffs(got, want))
        assert counts == (0, 3)


def test_another_header_and_the_first_frame_of_a_decoders_life(O, G, dlib):
    """frame 2 has other quantisation tables (another header: the single-frame route inside the call); the first call of each decoder is its first
    frame ever and writes to host memory (frame 0 ahead of the batched launches)"""
    streams = frames_of(O, A444, 4, seed=320)
    other = frames_of(O, A444[:5] + (40,) + A444[6:], 1, seed=321)[0]
    mixed = streams[:2] + [other] + streams[3:]
    rects = [(0, 0, 200, 120), (31, 17, 157, 93), (100, 3, 99, 9), (5, 5, 64, 40)]
    want = aa_expected(O, mixed, rects, 32, 24)
    singles = []
    for rep, got, counts in both_filters(G, dlib, mixed, rects, 32, 24):
        assert same(got, want), (rep, diffs(got, want))
        singles.append(counts[1])
        assert counts[0] + counts[1] == 4
    assert singles[0] >= 1 and singles[1] >= 1, singles


def test_damaged_restart_markers_in_one_frame(O, G, emu):
    """(CPU tier only) frame 2's restart markers are damaged: its bytes are the restatement over what the single region call returns for that stream,
    its neighbours equal the restatement over the oracle"""
    streams = frames_of(O, A444, 4, seed=330)
    rects = [(0, 0, 200, 120), (31, 17, 157, 93), (13, 20, 37, 90), (100, 3, 99, 9)]
    good = aa_expected(O, streams, rects, 32, 24)
    kind, bad, _ = next(iter(damaged_restart_markers(streams[2])))
    ref = new_decoder(G, emu)
    assert ref.set_option(OPT, opt_value(rects[0])) == 0
    ref.decode(streams[0])
    assert ref.set_option(OPT, opt_value(rects[2])) == 0
    try:
        want2 = aa_image(ref.decode(bad)[0], rects[2][2], rects[2][3], 1, 32, 24)
    except RuntimeError:
        want2 = None
    ref.close()
    mixed = streams[:2] + [bad] + streams[3:]
    dec = aa_decoder(G, emu)
    for rep in range(2):
        if want2 is None:
            with pytest.raises(RuntimeError):
                dec.decode_batch_crop_resize(mixed, rects, 32, 24)
            continue
        got, _ = dec.decode_batch_crop_resize(mixed, rects, 32, 24)
        assert same(got[:2] + got[3:], good[:2] + good[3:]) and np.array_equal(got[2], want2), (kind, rep)
    got, _ = dec.decode_batch_crop_resize(streams, rects, 32, 24)
    assert same(got, good), kind
    dec.close()


# ================================================================================================ 6. the tensor call
@pytest.mark.parametrize("dtype,layout", FORMATS, ids=FORMAT_IDS)
def test_tensor_call(O, G, dlib, dtype, layout):
    scale, bias = IMAGENET
    ow, oh = 32, 24
    streams = frames_of(O, A420, 4, seed=340)
    rects = [(0, 0, 161, 97), (121, 69, 40, 28), (3, 2, 157, 93), (8, 9, 20, 31)]
    mirror = [0, 1, 1, 0]
    want = aa_expected(O, streams, rects, ow, oh, mirror=mirror)
    a, b = aa_decoder(G, dlib, perf=True), aa_decoder(G, dlib, perf=True)
    for rep in range(2):
        u8, _ = a.decode_batch_crop_resize(streams, rects, ow, oh, mirror=mirror)
        assert same(u8, want), (rep, diffs(u8, want))
        got, pi = b.decode_batch_crop_resize_tensor(streams, rects, ow, oh, dtype, layout, scale, bias, mirror=mirror)
        assert got.shape == ((4, 3, oh, ow) if layout == CHW else (4, oh, ow, 3)) and (pi.width, pi.height, pi.pixel_format) == (ow, oh, 1)
        d = tensors_equal(got, u8, 1, ow, oh, dtype, layout, scale, bias)
        assert d == [0] * 4, (rep, d)
        assert a.last_batch() == b.last_batch() and a.region_stats() == b.region_stats() and a.idct_path() == b.idct_path() == 7
    a.close()
    b.close()


def test_tensor_call_single_channel(O, G, dlib):
    streams = frames_of(O, AGRAY, 3, seed=341)
    rects = [(0, 0, 48, 40), (1, 1, 45, 37), (20, 3, 5, 30)]
    want = aa_expected(O, streams, rects, 7, 5)
    scale, bias = [1.0 / 255.0] * 3, [-0.5] * 3
    dec = aa_decoder(G, dlib)
    for rep, (dtype, layout) in enumerate(((F16, HWC), (BF16, CHW), (F32, CHW))):
        got, pi = dec.decode_batch_crop_resize_tensor(streams, rects, 7, 5, dtype, layout, scale, bias)
        assert pi.pixel_format == 0 and tensors_equal(got, want, 0, 7, 5, dtype, layout, scale, bias) == [0] * 3, rep
    dec.close()


# ================================================================================================ 7. refusals
def test_refusals_write_nothing_and_leave_the_decoder_usable(O, G, dlib, capfd):
    streams = frames_of(O, AWIDE, 4, seed=350)
    ok = [(0, 0, 272, 256), (131, 127, 141, 129), (13, 20, 37, 150), (100, 3, 157, 93)]
    ow, oh = 32, 24
    want = aa_expected(O, streams, ok, ow, oh)
    stride = want[0].size + 32

    def refused(dec, rects, w=ow, h=oh, names=None):
        out = np.full(stride * 4, 0xA5, np.uint8)
        capfd.readouterr()
        assert raw_call(G, dlib, dec, streams, rects, w, h, out, stride) == -1, (rects, w, h)
        err = capfd.readouterr().err
        assert np.all(out == 0xA5), "a refused call wrote to the output"
        assert "[Error]" in err, "a refusal without a message"
        if names is not None:
            assert f"Frame {names} " in err, err

    def accepted(dec):
        out = np.full(stride * 4, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, ok, ow, oh, out, stride) == 0
        rows = out.reshape(4, stride)
        assert all(np.array_equal(rows[f, :want[f].size], want[f]) for f in range(4)) and np.all(rows[:, want[0].size:] == 0xA5)

    bad_rects = [(2, ok[:2] + [(272, 0, 10, 10)] + ok[3:]), (3, ok[:3] + [(0, 256, 5, 5)]), (1, ok[:1] + [(132, 0, 141, 45)] + ok[2:]), (0, [(-1, 0, 10, 10)] + ok[1:]),
                 (2, ok[:2] + [(5, 5, 0, 10)] + ok[3:]), (3, ok[:3] + [(0, 0, 10, 257)])]
    for cold in (True, False):
        dec = aa_decoder(G, dlib)
        if not cold:
            accepted(dec)
        # an unknown value: refused by set_option, the setting stays
        capfd.readouterr()
        for value in ("lanczos", "", "Antialias", "1"):
            assert dec.set_option(FILTER, value) != 0
        assert "[Error]" in capfd.readouterr().err
        for frame, rects in bad_rects:
            refused(dec, rects, names=frame)
            if cold:
                accepted(dec)
                dec.close()
                dec = aa_decoder(G, dlib)
        # the ratio: 272 > 256 x 1 along x, 256 = 256 x 1 along y
        small = [(0, 0, 100, 50), (5, 5, 64, 64), (1, 1, 30, 30), (9, 9, 256, 10)]
        refused(dec, small[:2] + [(0, 0, 272, 256)] + small[3:], 1, 1, names=2)
        refused(dec, small[:3] + [(9, 9, 257, 10)], 1, 1, names=3)
        refused(dec, [(0, 0, 257, 1)] + small[1:], 1, 1, names=0)
        for w, h in ((0, oh), (ow, 0), (-3, -3), (16385, oh), (ow, 16385)):
            refused(dec, ok, w, h)
        accepted(dec)
        # the prescale: refused on the option, whatever the rectangles would take
        for value in ("1/2", "1/8"):
            assert dec.set_option(PRESCALE, value) == 0
            refused(dec, ok)
        assert dec.set_option(PRESCALE, "1") == 0
        accepted(dec)
        for opt, on, off in (("dec_opt_scale", "1/2", "1"), ("dec_opt_flipped", "1", "0"), ("dec_opt_channel_remap", "210", "")):
            assert dec.set_option(opt, on) == 0
            refused(dec, ok)
            assert dec.set_option(opt, off) == 0
            accepted(dec)
        dec.close()
    for pf in (3, 4, 5):  # output formats whose pixels share samples
        dec = aa_decoder(G, dlib, pf, 3)
        refused(dec, [(0, 0, 272, 256), (130, 126, 142, 130), (12, 20, 38, 150), (100, 2, 156, 94)])
        dec.set_output_format(1, 1)
        accepted(dec)
        dec.close()
    # the tensor call makes the same refusals
    dec = aa_decoder(G, dlib)
    fmt = G.tensor_format(F32, CHW, *IMAGENET)
    out = np.full(4 * ow * oh * 3 * 4 + 64, 0xA5, np.uint8)
    assert tensor_raw_call(G, dlib, dec, streams, [(0, 0, 100, 50), (5, 5, 64, 64), (1, 1, 30, 30), (0, 0, 272, 256)], 1, 1, fmt, out, 16) == -1 and np.all(out == 0xA5)
    assert dec.set_option(PRESCALE, "1/4") == 0
    assert tensor_raw_call(G, dlib, dec, streams, ok, ow, oh, fmt, out, ow * oh * 12) == -1 and np.all(out == 0xA5)
    assert dec.set_option(PRESCALE, "1") == 0
    accepted(dec)
    dec.close()


# ================================================================================================ 8. nothing else moved
def test_nothing_else_moved(O, G, dlib):
    streams = frames_of(O, A444, 4, seed=360)
    rects = [(0, 0, 200, 120), (31, 17, 157, 93), (13, 20, 37, 90), (100, 3, 99, 9)]
    origins = [(100, 50), (7, 9), (130, 11), (111, 60)]
    ow, oh = 32, 24
    plain = perf_decoder(G, dlib)
    explicit = perf_decoder(G, dlib)
    assert explicit.set_option(FILTER, "bilinear") == 0
    moving = perf_decoder(G, dlib)
    want_aa = aa_expected(O, streams, rects, ow, oh)
    full = [O.decode(x)[0] for x in streams]
    for rep in range(2):
        base, _ = plain.decode_batch_crop_resize(streams, rects, ow, oh)
        got, _ = explicit.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, base) and explicit.idct_path() == plain.idct_path() == 5 and explicit.last_batch() == plain.last_batch()
        assert moving.set_option(FILTER, "antialias") == 0
        got, _ = moving.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, want_aa) and moving.idct_path() == 7, (rep, diffs(got, want_aa))
        assert not same(got, base), "the two filters gave the same bytes: the test shows nothing"
        # the other calls of a decoder that holds the filter
        got, _ = moving.decode_batch_regions(streams, origins, 70, 60)
        assert same(got, [crop(full[f], 200, 120, 1, origins[f] + (70, 60)) for f in range(4)]) and moving.idct_path() in (3, 4), rep
        px, pi = moving.decode(streams[3])
        assert (pi.width, pi.height) == (200, 120) and np.array_equal(px, full[3]) and moving.idct_path() == 0, rep
        got, _ = moving.decode_batch(streams)
        assert same(got, full), rep
        assert moving.set_option(FILTER, "bilinear") == 0
        got, _ = moving.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, base) and moving.idct_path() == 5, rep
    for dec in (plain, explicit, moving):
        dec.close()


# ================================================================================================ 9. what it is for
def area_average(c, ow, oh):
    """the exact area average of the (h, w, channels) image over the ow x oh grid of equal cells (fractional coverage at the cells' borders), float64"""
    def cover(n_src, n_out):
        k = np.arange(n_src, dtype=np.float64)[None, :]
        lo = np.arange(n_out, dtype=np.float64)[:, None] * n_src / n_out
        return np.clip(np.minimum(k + 1, lo + n_src / n_out) - np.maximum(k, lo), 0, None) * n_out / n_src
    h, w = c.shape[:2]
    return np.tensordot(cover(h, oh), np.tensordot(c.astype(np.float64), cover(w, ow), axes=([1], [1])), axes=([1], [0])).transpose(0, 2, 1)


def test_less_aliasing_than_bilinear(O, G, dlib):
    stream = frames_of(O, ANAT, 1, seed=370)[0]
    rect, ow, oh = (21, 9, 600, 350), 64, 40
    raw, img = O.decode(stream)
    ideal = area_average(crop(raw, 640, 368, 1, rect).reshape(350, 600, 3), ow, oh)
    mse = {}
    for name, options in (("bilinear", ()), ("bilinear + prescale 1/8", ((PRESCALE, "1/8"),)), ("antialias", ((FILTER, "antialias"),))):
        dec = new_decoder(G, dlib)
        for opt, value in options:
            assert dec.set_option(opt, value) == 0
        got, _ = dec.decode_batch_crop_resize([stream], [rect], ow, oh)
        if name != "antialias":
            assert dec.prescales() == [1], "the prescale leaves a 4:2:0 stream alone"
        mse[name] = float(np.mean((got[0].reshape(oh, ow, 3).astype(np.float64) - ideal) ** 2))
        dec.close()
    print("mean squared error against the exact area average: " + ", ".join(f"{k}: {v:.3f}" for k, v in mse.items()))
    assert mse["antialias"] < mse["bilinear"] and mse["antialias"] < mse["bilinear + prescale 1/8"]
