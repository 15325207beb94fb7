"""dec_opt_resize_prescale_subsampled: the prescale of crop-and-resize on 4:2:0 streams, each component at its own N (gpujpeg_amd_ext.h).

With the option on, a frame of an eligible stream (every component sub_h == sub_v in {1, 2}, at least one 2) takes its scale s by the rule of the
all-1x1 streams, and the image the resample reads is built per component: component c's blocks leave N_c x N_c samples, N_c = 8 sub_h / s -- N_c = 8 is
the full-size plane, N_c <= 4 the transform of dec_opt_scale --, so every plane has one sample per reduced pixel and the pixels are made like those of
an all-1x1 stream. per_component_reduced below restates that in numpy over the oracle (parse, huffman_decode, idct, postprocess) and the two lines of
test_scaled_decode.reduced_planes; plan, pre_resize_image and the frames of scale 1 are test_crop_resize_prescale's. Every comparison with the library
is byte for byte.

Two tiers with the same bodies, like test_crop_resize_prescale.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Every test sets the new option, so none passes on a library without it."""
import ctypes as C

import numpy as np
import pytest

import test_crop_resize_prescale as pre
from conftest import natural_image, oracle_image
from test_crop_resize import BPP, diffs, raw_call, region_stats_of
from test_crop_resize_prescale import NAME, PRE, area_average, expanded, plan, pre_resize_image
from test_region_batch import dlib, emu, frames_of, new_decoder, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import case_named, crop, damaged_restart_markers, perf_decoder
from test_scaled_decode import corner_blocks, m_matrix

SUB = "dec_opt_resize_prescale_subsampled"
plain_expected = pre.plain_expected
S420 = [(2, 2), (1, 1), (1, 1)]
IL = case_named("rgb_to_420_il")        # 322 x 242, interleaved: 20 MCUs and 2 pixels wide, 15 MCUs and 2 pixels high
PLANAR = case_named("planar420_in")     # 162 x 122, non-interleaved, planar 4:2:0 in
ODD = ("sub_420_il_odd", 161, 97, 1, 1, 75, 3, 1, S420, 3)  # interleaved, restart interval 3, 11 x 7 MCUs: an odd number
R0 = ("sub_420_restart0", 100, 60, 1, 1, 75, 0, 1, S420, 3)
C422 = case_named("rgb_to_422_nonil")


# ================================================================================================ the definition, in numpy
_reduced = {}  # (stream, pf, cs, s) -> the image reduced per component: made once, shared by the tests, never written to


def per_component_reduced(O, jpeg, pf, cs, s):
    """Rs of the definition -> (pixels, width, height, pixel format)"""
    key = (jpeg.tobytes(), pf, cs, s)
    if key in _reduced:
        return _reduced[key]
    st = O.parse(jpeg, -1 if pf is None else pf, -1 if cs is None else cs)
    try:
        coefs = O.huffman_decode(st, jpeg)
        full = O.idct(st, coefs)
        img = st.img
        red = []
        for c in range(img.comp_count):
            k = img.comp[c]
            t = img.max_h // k.h
            assert t == img.max_v // k.v and t in (1, 2) and t * k.h == img.max_h
            N = 8 * t // s
            assert N in (1, 2, 4, 8)
            if N == 8:
                red.append(full[k.data_offset:k.data_offset + k.data_width * k.data_height].reshape(k.data_height, k.data_width))
                continue
            D, m = corner_blocks(st, coefs, c, N), m_matrix(N)
            T = (np.einsum("yv,abvu->abyu", m, D) + 1024) >> 11
            S = (np.einsum("abyu,xu->abyx", T, m) + 16384) >> 15
            red.append(np.clip(S + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(D.shape[0] * N, D.shape[1] * N))
        im2 = O.Image.from_buffer_copy(img)
        im2.width, im2.height = -(-img.width // s), -(-img.height // s)
        for i in range(img.comp_count):
            im2.samp_h[i] = im2.samp_v[i] = 1
        assert O.lib().gjo_image_init(C.byref(im2)) == 0
        planes = np.zeros(im2.data_size, np.uint8)
        for c in range(im2.comp_count):
            k2, r = im2.comp[c], red[c]
            assert (k2.width, k2.height) == (im2.width, im2.height) and r.shape[1] >= k2.width and r.shape[0] >= k2.height, (c, r.shape, k2.width, k2.height)
            hh, ww = min(k2.data_height, r.shape[0]), min(k2.data_width, r.shape[1])
            P = np.zeros((k2.data_height, k2.data_width), np.uint8)
            P[:hh, :ww] = r[:hh, :ww]
            planes[k2.data_offset:k2.data_offset + P.size] = P.reshape(-1)
        _reduced[key] = (O.postprocess(im2, planes), im2.width, im2.height, im2.pixel_format)
    finally:
        O.lib().gjo_stream_free(C.byref(st))
    return _reduced[key]


def expected(O, streams, rects, ow, oh, S, pf=None, cs=None, mirror=None):
    """the restatement -> (one array per frame, the plans)"""
    out, plans = [], []
    for f, (jpeg, rect) in enumerate(zip(streams, rects)):
        img = O.parse(jpeg).img
        p = plan(img.width, img.height, True, rect, ow, oh, S)
        plans.append(p)
        m = bool(mirror and mirror[f])
        if p[0] == 1:
            out.append(plain_expected(O, [jpeg], [rect], ow, oh, pf, cs, [1] if m else None)[0])
            continue
        px, rw, rh, rpf = per_component_reduced(O, jpeg, pf, cs, p[0])
        assert p[1] + p[3] <= rw and p[2] + p[4] <= rh
        out.append(pre_resize_image(crop(px, rw, rh, rpf, p[1:]), rpf, rect, p, ow, oh, m))
    return out, plans


def sub_decoder(G, lib, S, pf=None, cs=None, align=None, perf=False, value="on"):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib, pf, cs, align)
    if perf and pf is not None:
        dec.set_output_format(cs, pf)
    assert dec.set_option(PRE, NAME[S]) == 0
    if value is not None:
        assert dec.set_option(SUB, value) == 0
    return dec


# ================================================================================================ 1. the host plan
def option_exists(G, lib):
    """the tests that run no call of the library are this option's too"""
    dec = G.Decoder(lib)
    assert dec.set_option(SUB, "on") == 0 and dec.set_option(SUB, "off") == 0
    dec.close()


def test_host_plan_takes_the_flag_for_an_eligible_stream(G, emu):
    """what the decoder passes for a 4:2:0 stream under the option: a non-zero flag, any non-zero value, gives the plan of the all-1x1 streams"""
    option_exists(G, emu)
    lib = emu
    for W, rect, ow, S in pre.sweep():
        want = plan(W, 61, True, rect, ow, 1, S)
        assert G.crop_resize_plan(lib, W, 61, 1, rect, ow, 1, S) == G.crop_resize_plan(lib, W, 61, 7, rect, ow, 1, S) == want, (W, rect, ow, S)
    assert G.crop_resize_plan(lib, 322, 242, 1, (3, 50, 300, 40), 24, 16, 8) == plan(322, 242, True, (3, 50, 300, 40), 24, 16, 8) == (2, 1, 25, 151, 20)


# ================================================================================================ 2. every scale in one batch, per stream
SCALES = [1, 2, 4, 8, 2, 8, 8, 4]
MIRROR = [f & 1 for f in range(8)]
# scale 1 (too narrow), 2, 4, 8, h as the limit (2), the whole image (8), a rectangle that ends at both edges (8), 4 at odd origins
SMALL = [(13, 21, 20, 15), (7, 9, 30, 20), (33, 5, 50, 35), (51, 13, 100, 66), (3, 50, 150, 20), None, None, (75, 49, 49, 33)]
# (the planar 4:2:0 stream goes to planar 4:4:4 YCbCr: the call refuses its own format, whose pixels share samples)
BATCHES = {  # id -> (case, output format / colour space, rectangles, output size)
    "420_il": (IL, None, None, [(13, 21, 40, 30), (7, 9, 60, 40), (33, 5, 100, 70), (101, 43, 200, 130), (3, 50, 300, 40), (0, 0, 322, 242),
                                (121, 111, 201, 131), (151, 99, 97, 65)], 24, 16),
    "planar420_nonil": (PLANAR, 2, 3, SMALL[:5] + [(0, 0, 162, 122), (61, 57, 101, 65)] + SMALL[7:], 12, 8),
    "420_il_odd_r3": (ODD, None, None, SMALL[:5] + [(0, 0, 161, 97), (60, 32, 101, 65)] + SMALL[7:], 12, 8),
}
_batches = {}


def batch_of(O, ident):
    """streams and expected frames at every S of one of BATCHES, made once"""
    if ident not in _batches:
        case, pf, cs, rects, ow, oh = BATCHES[ident]
        streams = frames_of(O, case, len(rects))
        want = {S: expected(O, streams, rects, ow, oh, S, pf, cs, mirror=MIRROR) for S in (2, 4, 8)}
        assert [p[0] for p in want[8][1]] == SCALES
        assert any(r[0] % 16 and r[1] % 16 and r[0] % 2 and r[1] % 2 for r in rects) and rects[6][0] + rects[6][2] == case[1] and rects[6][1] + rects[6][3] == case[2]
        _batches[ident] = (streams, want)
    return _batches[ident]


@pytest.mark.parametrize("ident", list(BATCHES))
def test_every_scale_in_one_batch(O, G, dlib, ident):
    case, pf, cs, rects, ow, oh = BATCHES[ident]
    streams, want = batch_of(O, ident)
    want, plans = want[8]
    n = len(streams)
    singles = region_stats_of(G, dlib, streams, [expanded(case[1], case[2], p) for p in plans], pf, cs)
    for chunk in (3, 0):
        dec = sub_decoder(G, dlib, 8, pf, cs, perf=True)
        if chunk:
            dec.set_batch_chunk(chunk)
        for rep in range(2):
            got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
            assert (pi.width, pi.height) == (ow, oh) and dlib.image_size(pi) == ow * oh * 3
            assert same(got, want), (chunk, rep, diffs(got, want))
            assert dec.prescales() == SCALES
            assert dec.idct_path() == 8
            batched, single = dec.last_batch()
            assert batched + single == n and single <= 1, (batched, single)
            st = dec.region_stats()
            assert st[0] == 1 and st[1:] == tuple(sum(s[i] for s in singles) for i in (1, 2, 3)), (st, singles)
        dec.close()


# ================================================================================================ 3. every N_c
@pytest.mark.parametrize("S", [2, 4, 8])
def test_option_caps_the_scale_and_every_n_occurs(O, G, dlib, S):
    case, pf, cs, rects, ow, oh = BATCHES["420_il"]
    streams, want = batch_of(O, "420_il")
    want, plans = want[S]
    assert max(p[0] for p in plans) == S and (8 // S, 16 // S) in {(8 // p[0], 16 // p[0]) for p in plans if p[0] > 1}  # (luma, chroma) = (4, 8), (2, 4), (1, 2)
    dec = sub_decoder(G, dlib, S, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.prescales() == [min(s, S) for s in SCALES] == [p[0] for p in plans] and dec.idct_path() == 8
    dec.close()


# ================================================================================================ 4. edges
# the whole image to 1 x 1 (8), a rectangle of 1 x 1 (1), a cover of one MCU (8: pixels 16 .. 31 both ways), the last MCU row and column (2: 306 .. 321, 240 .. 241);
# rectangles of exactly s OW x s OH (8, 4, 2) beside the whole image
EDGES = [("to_1x1", [(0, 0, 322, 242), (100, 100, 1, 1), (17, 18, 9, 9), (306, 240, 16, 2)], 1, 1, [8, 1, 8, 2]),
         ("exactly_s_times_the_output", [(5, 7, 56, 24), (9, 17, 28, 12), (301, 235, 14, 6), (0, 0, 322, 242)], 7, 3, [8, 4, 2, 8])]


@pytest.mark.parametrize("ident,rects,ow,oh,scales", EDGES, ids=[e[0] for e in EDGES])
def test_edges(O, G, dlib, ident, rects, ow, oh, scales):
    streams = frames_of(O, IL, len(rects), seed=50)
    want, plans = expected(O, streams, rects, ow, oh, 8)
    assert [p[0] for p in plans] == scales
    if ident == "to_1x1":
        assert expanded(322, 242, plans[2]) == (16, 16, 16, 16) and expanded(322, 242, plans[3]) == (306, 240, 16, 2)
    dec = sub_decoder(G, dlib, 8)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert (pi.width, pi.height) == (ow, oh) and same(got, want), (rep, diffs(got, want))
        assert dec.prescales() == scales
    dec.close()


# ================================================================================================ 5. configurations
# (id, case, output pixel format, colour space, line alignment)
CONFIGS = [("rgb", IL, 1, 1, 0), ("planar444_ycbcr", PLANAR, 2, 3, 0), ("rgba_4444", IL, 6, 1, 0), ("u8", IL, 0, 3, 0), ("rgb_aligned_64", IL, 1, 1, 64)]


def config_rects(w, h, ow, oh):
    """the whole image, odd origins at scales 2 and 4, the far corner, a rectangle smaller than the output"""
    return [(0, 0, w, h), (1, 3, 2 * ow + 3, 2 * oh + 1), (w - 4 * ow - 1, h - 4 * oh - 2, 4 * ow + 1, 4 * oh + 2), (w // 3 | 1, h // 2 | 1, 5, 3)]


@pytest.mark.parametrize("ident,case,pf,cs,align", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_configurations(O, G, dlib, ident, case, pf, cs, align):
    w, h = case[1], case[2]
    ow, oh = 7, 5
    rects = config_rects(w, h, ow, oh)
    streams = frames_of(O, case, 4, seed=40)
    want, plans = expected(O, streams, rects, ow, oh, 8, pf, cs)
    assert [p[0] for p in plans] == [8, 2, 4, 1], plans
    bpp = BPP.get(pf)
    pad = (-(ow * bpp)) % align if align else 0

    def pixels(frames):  # (dec_opt_alignment_bytes pads the output's lines: what lies in the padding is nobody's)
        return [px[:oh * (ow * bpp + pad)].reshape(oh, ow * bpp + pad)[:, :ow * bpp].reshape(-1) for px in frames] if pad else frames

    dec = sub_decoder(G, dlib, 8, pf, cs, align)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert (pi.width, pi.height, pi.pixel_format, pi.width_padding) == (ow, oh, pf, pad)
        assert (pad != 0) == bool(align) and all(a.size == dlib.image_size(pi) for a in got)
        assert same(pixels(got), want), (rep, diffs(pixels(got), want))
        assert dec.prescales() == [p[0] for p in plans] and dec.last_batch()[1] <= 1
    dec.close()


@pytest.mark.parametrize("dtype,layout", [(1, 0), (0, 1)], ids=["f16_chw", "f32_hwc"])
def test_tensor_call_is_the_host_element_of_the_u8_bytes(O, G, dlib, dtype, layout):
    ow, oh = 7, 5
    rects = config_rects(322, 242, ow, oh)
    streams = frames_of(O, IL, 4, seed=40)
    scale, bias = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)], [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    fmt = G.tensor_format(dtype, layout, scale, bias)
    lut = np.array([[G.tensor_element(dlib, fmt, c, v) for v in range(256)] for c in range(3)], np.uint32)
    a, b = sub_decoder(G, dlib, 8, 1, 1), sub_decoder(G, dlib, 8, 1, 1)
    for rep in range(2):
        u8, _ = a.decode_batch_crop_resize(streams, rects, ow, oh, mirror=[0, 1, 0, 1])
        got, _ = b.decode_batch_crop_resize_tensor(streams, rects, ow, oh, dtype, layout, scale, bias, mirror=[0, 1, 0, 1])
        assert a.prescales() == b.prescales() == [8, 2, 4, 1] and a.region_stats() == b.region_stats()
        for f in range(4):
            hwc = u8[f].reshape(oh, ow, 3)
            want = np.stack([lut[c][hwc[:, :, c]] for c in range(3)], -1)
            want = want if layout == 1 else want.transpose(2, 0, 1)
            bits = np.ascontiguousarray(got[f]).view(np.uint32 if dtype == 0 else np.uint16)
            assert bits.shape == want.shape and np.array_equal(bits.astype(np.uint32), want), (rep, f)
    a.close()
    b.close()


# ================================================================================================ 6. the option off is today's call
def test_option_off_is_the_call_without_it(O, G, dlib):
    case, pf, cs, rects, ow, oh = BATCHES["420_il"]
    streams, want = batch_of(O, "420_il")
    n = len(streams)
    plain = perf_decoder(G, dlib)  # (a decoder that saw neither option)
    ref, _ = plain.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
    ref_stats = plain.region_stats()
    plain.close()
    assert same(ref, plain_expected(O, streams, rects, ow, oh, mirror=MIRROR))
    for value in (None, "off"):  # never set, set to off
        dec = sub_decoder(G, dlib, 8, perf=True, value=value)
        if value is None:
            assert dec.set_option(SUB, "on") == 0 and dec.set_option(SUB, "off") == 0  # (the option exists; off again before any call)
        for rep in range(2):
            got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
            assert same(got, ref), (value, rep, diffs(got, ref))
            assert dec.prescales() == [1] * n and dec.idct_path() == 5 and dec.region_stats() == ref_stats
        # on, and off again, between the calls of one decoder
        assert dec.set_option(SUB, "on") == 0
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
        assert same(got, want[8][0]) and dec.prescales() == SCALES and dec.idct_path() == 8
        assert dec.set_option(SUB, "off") == 0
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
        assert same(got, ref) and dec.prescales() == [1] * n and dec.idct_path() == 5 and dec.region_stats() == ref_stats
        # without a prescale the option has no effect
        assert dec.set_option(SUB, "on") == 0 and dec.set_option(PRE, "1") == 0
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
        assert same(got, ref) and dec.prescales() == [1] * n and dec.idct_path() == 5 and dec.region_stats() == ref_stats
        dec.close()


# ================================================================================================ 7. streams the option does not reach
def test_422_keeps_scale_1(O, G, dlib):
    w, h = C422[1], C422[2]
    rects = [(0, 0, w, h), (1, 3, w - 2, h - 5), (w // 2, h // 2, w // 2, h // 2)]
    streams = frames_of(O, C422, 3, seed=44)
    assert all(plan(w, h, True, r, 8, 6, 8)[0] >= 4 for r in rects), "an eligible stream would be prescaled here"
    plain = new_decoder(G, dlib, 1, 1)
    ref, _ = plain.decode_batch_crop_resize(streams, rects, 8, 6)
    plain.close()
    assert same(ref, plain_expected(O, streams, rects, 8, 6, 1, 1))
    dec = sub_decoder(G, dlib, 8, 1, 1, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, 8, 6)
        assert same(got, ref), (rep, diffs(got, ref))
        assert dec.prescales() == [1, 1, 1] and dec.idct_path() == 5
    dec.close()


def test_444_takes_the_whole_prescale(O, G, dlib):
    streams = frames_of(O, case_named(pre.HD_CASE), len(pre.HD_RECTS))
    want, plans = pre.expected(O, streams, pre.HD_RECTS, pre.OW, pre.OH, 8, mirror=pre.HD_MIRROR)
    dec = sub_decoder(G, dlib, 8, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, pre.HD_RECTS, pre.OW, pre.OH, mirror=pre.HD_MIRROR)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.prescales() == pre.HD_SCALES and dec.idct_path() == 6
    dec.close()


# ================================================================================================ 8. frame-by-frame routes
def test_restart_interval_0_goes_frame_by_frame(O, G, dlib):
    streams = frames_of(O, R0, 3, seed=60)
    rects = [(0, 0, 100, 60), (59, 35, 41, 25), (33, 17, 11, 30)]
    want, plans = expected(O, streams, rects, 6, 4, 8, mirror=[0, 1, 0])
    assert [p[0] for p in plans] == [8, 4, 1]
    dec = sub_decoder(G, dlib, 8, perf=True)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, 6, 4, mirror=[0, 1, 0])
        assert same(got, want) and (pi.width, pi.height) == (6, 4), (rep, diffs(got, want))
        assert dec.last_batch() == (0, 3) and dec.idct_path() == 8 and dec.prescales() == [8, 4, 1]
        assert dec.region_stats()[0] == 2
    dec.close()


def test_single_frame_route_gives_the_batched_bytes(O, G, dlib):
    """host output: frame 0 of every call goes through the single-frame region call, on a fresh decoder (its first call) and on one with a header to
    launch on; every frame of the batch takes that place once and gives the bytes it gives inside the batched launches"""
    case, pf, cs, rects, ow, oh = BATCHES["420_il_odd_r3"]
    streams, want = batch_of(O, "420_il_odd_r3")
    want = want[8][0]
    n = len(streams)
    for first in range(n):
        order = [first] + [f for f in range(n) if f != first][:2]
        dec = sub_decoder(G, dlib, 8)
        for rep in range(2):
            got, _ = dec.decode_batch_crop_resize([streams[f] for f in order], [rects[f] for f in order], ow, oh, mirror=[MIRROR[f] for f in order])
            assert same(got, [want[f] for f in order]), (first, rep)
            assert dec.prescales() == [SCALES[f] for f in order] and dec.last_batch()[1] >= 1
        dec.close()


def test_damaged_restart_markers_in_one_frame(O, G, emu):
    """(CPU tier only) frame 3's restart markers are damaged (scale 8): it goes through the single-frame route, its neighbours stay in the batched
    launches and equal the restatement; what the damaged frame gives is what that route gives it alone, on a decoder of the same state"""
    case, pf, cs, rects, ow, oh = BATCHES["420_il_odd_r3"]
    streams, want = batch_of(O, "420_il_odd_r3")
    want = want[8][0][:5]
    streams, rects, flags = streams[:5], rects[:5], MIRROR[:5]
    for kind, bad, _ in damaged_restart_markers(streams[3]):
        ref = sub_decoder(G, emu, 8)
        try:
            ref.decode_batch_crop_resize([streams[0]], [rects[0]], ow, oh)  # (a header to launch on, as the batch call has when it reaches frame 3)
            want3 = ref.decode_batch_crop_resize([bad], [rects[3]], ow, oh, mirror=[flags[3]])[0][0]
        except RuntimeError:
            want3 = None
        ref.close()
        mixed = streams[:3] + [bad] + streams[4:]
        dec = sub_decoder(G, emu, 8)
        for rep in range(2):
            if want3 is None:
                with pytest.raises(RuntimeError):
                    dec.decode_batch_crop_resize(mixed, rects, ow, oh, mirror=flags)
                continue
            got, _ = dec.decode_batch_crop_resize(mixed, rects, ow, oh, mirror=flags)
            assert same(got[:3] + got[4:], want[:3] + want[4:]), (kind, rep)
            assert np.array_equal(got[3], want3), (kind, rep)
            batched, single = dec.last_batch()
            assert 1 <= single <= 2 and batched >= 3, (kind, batched, single)
            assert dec.prescales() == SCALES[:5]
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=flags)  # the decoder decodes the intact streams as ever
        assert same(got, want), kind
        dec.close()


# ================================================================================================ 9. refusals
def test_bad_option_values_are_refused_and_the_setting_is_kept(O, G, dlib, capfd):
    case, pf, cs, rects, ow, oh = BATCHES["420_il"]
    streams, want = batch_of(O, "420_il")
    for kept, frames, scales in (("on", want[8][0], SCALES), ("off", plain_expected(O, streams, rects, ow, oh, mirror=MIRROR), [1] * 8)):
        dec = sub_decoder(G, dlib, 8, value=kept)
        for bad in ("1", "0", "", "On", "on ", "true", "1/8", "yes"):
            capfd.readouterr()
            assert dec.set_option(SUB, bad) != 0, bad
            assert "[Error]" in capfd.readouterr().err
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
        assert same(got, frames) and dec.prescales() == scales, kept
        dec.close()


def test_refusals_write_nothing_and_leave_the_decoder_usable(O, G, dlib, capfd):
    case, pf, cs, rects, ow, oh = BATCHES["420_il"]
    streams, want = batch_of(O, "420_il")
    n, raw = len(streams), ow * oh * 3
    dec = sub_decoder(G, dlib, 8)

    def refused(rects_, words):
        out = np.full(raw * n + 64, 0xA5, np.uint8)
        capfd.readouterr()
        assert raw_call(G, dlib, dec, streams, rects_, ow, oh, out, raw, mirror=MIRROR) != 0
        err = capfd.readouterr().err
        assert all(w in err for w in words), err
        assert np.all(out == 0xA5) and dec.prescales() == []

    # the antialiased filter together with a prescale: still refused
    assert dec.set_option("dec_opt_resize_filter", "antialias") == 0
    refused(rects, ["dec_opt_resize_filter", "dec_opt_resize_prescale"])
    assert dec.set_option("dec_opt_resize_filter", "bilinear") == 0
    got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
    assert same(got, want[8][0])  # (a header to launch on from here: the rectangles are checked ahead of the launches)
    # a rectangle outside the image names its frame
    refused(rects[:5] + [(123, 43, 200, 130)] + rects[6:], ["Frame 5", "123,43,200,130"])
    got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=MIRROR)
    assert same(got, want[8][0]) and dec.prescales() == SCALES
    dec.close()


# ================================================================================================ 10. quality (no library)
Q_IL = ("sub_q_420_il", 640, 368, 1, 1, 75, -1, 1, S420, 3)
Q_NONIL = ("sub_q_420_nonil", 322, 242, 1, 1, 75, -1, 0, S420, 3)
QUALITY = [(Q_IL, (17, 9, 600, 350), 64, 40, 8), (Q_IL, (3, 5, 520, 330), 120, 80, 4), (Q_IL, (33, 21, 300, 200), 120, 80, 2),
           (Q_NONIL, (1, 3, 319, 237), 24, 16, 8), (Q_NONIL, (5, 7, 100, 70), 40, 30, 2)]


@pytest.mark.parametrize("case,rect,ow,oh,s", QUALITY, ids=[f"{q[0][0]}_to_{q[2]}x{q[3]}" for q in QUALITY])
def test_per_component_definition_is_nearer_the_area_average(O, G, emu, case, rect, ow, oh, s):
    """natural 4:2:0 content at q75: mean squared error against the exact area average of the full-size oracle crop, all channels -- the restatement with
    the per-component prescale strictly below the unprescaled definition (6.98 / 4.23 / 1.39 / 9.31 / 1.56 against 0.80 / 0.70 / 0.50 / 0.78 / 0.46
    when the option was proposed)"""
    option_exists(G, emu)
    jpeg = O.encode(oracle_image(O, case), natural_image(case[1], case[2], 3, seed=5))
    full, img = O.decode(jpeg)
    ideal = area_average(crop(full, img.width, img.height, 1, rect).reshape(rect[3], rect[2], 3), ow, oh)
    (sub,), (p,) = expected(O, [jpeg], [rect], ow, oh, 8)
    assert p[0] == s
    (today,) = plain_expected(O, [jpeg], [rect], ow, oh)
    mse_sub = float(np.mean((sub.reshape(oh, ow, 3) - ideal) ** 2))
    mse_today = float(np.mean((today.reshape(oh, ow, 3) - ideal) ** 2))
    print(f"{case[0]} {rect} -> {ow}x{oh}, s = {s}: MSE today {mse_today:.2f}, per component {mse_sub:.2f}")
    assert mse_sub < mse_today
