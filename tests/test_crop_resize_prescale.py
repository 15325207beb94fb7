"""dec_opt_resize_prescale: crop-and-resize with the reduced-size IDCT of dec_opt_scale ahead of the resample (gpujpeg_amd_ext.h).

Frame f of a call with the option at 1/S takes the scale s_f -- the largest of 1, 2, 4, 8 with s <= S, w >= s OW and h >= s OH; 1 for a subsampled
stream -- and is the bilinear resample, at the taps of the REDUCED image, of the covering rectangle's crop of what dec_opt_scale = 1/s_f decodes.
Expected bytes are the numpy restatement of that definition (plan, pre_taps, pre_resize below) over test_scaled_decode.expected -- itself numpy over
the oracle's coefficients --, and test_crop_resize.expected for the frames of scale 1; every comparison with the library is byte for byte.

Two tiers with the same bodies, like test_crop_resize.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Every test needs the option, so none passes on a library without it."""
import numpy as np
import pytest

import test_crop_resize as base
from test_crop_resize import BPP, diffs, raw_call, region_stats_of, taps
from test_region_batch import dlib, emu, frames_of, new_decoder, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import OPT, case_named, case_stream, crop, damaged_restart_markers, opt_value, perf_decoder
from test_scaled_decode import expected as scaled_expected

PRE = "dec_opt_resize_prescale"
plain_expected = base.expected  # (the restatement without a prescale; test 8 replaces the name in that module)
NAME = {1: "1", 2: "1/2", 4: "1/4", 8: "1/8"}


# ================================================================================================ the definition, in numpy
def plan(W, H, all_1x1, rect, ow, oh, S):
    """(s, x', y', w', h') of one frame"""
    x, y, w, h = rect
    s = 1
    if all_1x1:
        for t in (2, 4, 8):
            if t <= S and w >= t * ow and h >= t * oh:
                s = t
    xr, yr = x // s, y // s
    return s, xr, yr, -(-(x + w) // s) - xr, -(-(y + h) // s) - yr


def expanded(W, H, p):
    """the full-size rectangle whose cover a frame of plan p decodes"""
    s, xr, yr, wr, hr = p
    return xr * s, yr * s, min(wr * s, W - xr * s), min(hr * s, H - yr * s)


def pre_taps(n_src, n_out, off, s, n_red):
    """the generalised taps: n_out output samples of an n_src-sample crop that starts `off` full-size samples behind the first of n_red reduced ones"""
    i = np.arange(n_out, dtype=np.int64)
    d = 2 * n_out * s
    n = np.maximum((2 * i + 1) * n_src + 2 * n_out * off - n_out * s, 0)
    p0 = n // d
    f = ((n - p0 * d) * 256) // d
    return p0, np.minimum(p0 + 1, n_red - 1), f


def pre_resize_channels(c, rect, p, ow, oh):
    """c: the (h', w', channels) crop of the reduced image at (x', y') -> (oh, ow, channels) by the definition"""
    x, y, w, h = rect
    s, xr, yr, wr, hr = p
    assert c.shape[:2] == (hr, wr)
    x0, x1, fx = pre_taps(w, ow, x - s * xr, s, wr)
    y0, y1, fy = pre_taps(h, oh, y - s * yr, s, hr)
    assert x0.max() <= wr - 1 and y0.max() <= hr - 1
    c = c.astype(np.int64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = c[y0][:, x0] * (256 - fx) + c[y0][:, x1] * fx
    bot = c[y1][:, x0] * (256 - fx) + c[y1][:, x1] * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)


def pre_resize_image(c, pf, rect, p, ow, oh, mirror=False):
    wr, hr = p[3], p[4]
    if pf in BPP:
        r = pre_resize_channels(c.reshape(hr, wr, BPP[pf]), rect, p, ow, oh)
        return (r[:, ::-1] if mirror else r).reshape(-1)
    assert pf == 2
    r = pre_resize_channels(c.reshape(3, hr, wr).transpose(1, 2, 0), rect, p, ow, oh)
    return (r[:, ::-1] if mirror else r).transpose(2, 0, 1).reshape(-1)


_reduced = {}  # (stream, pf, cs, s) -> the reduced decode: made once, shared by the tests, never written to


def reduced(O, jpeg, pf, cs, s):
    key = (jpeg.tobytes(), pf, cs, s)
    if key not in _reduced:
        px, img = scaled_expected(O, jpeg, -1 if pf is None else pf, -1 if cs is None else cs, s)
        _reduced[key] = (px, img.width, img.height, img.pixel_format)
    return _reduced[key]


def expected(O, streams, rects, ow, oh, S, pf=None, cs=None, mirror=None, all_1x1=True):
    """the restatement -> (one array per frame, the plans)"""
    out, plans = [], []
    for f, (jpeg, rect) in enumerate(zip(streams, rects)):
        img = O.parse(jpeg).img
        p = plan(img.width, img.height, all_1x1, rect, ow, oh, S)
        plans.append(p)
        m = bool(mirror and mirror[f])
        if p[0] == 1:
            out.append(plain_expected(O, [jpeg], [rect], ow, oh, pf, cs, [1] if m else None)[0])
            continue
        px, rw, rh, rpf = reduced(O, jpeg, pf, cs, p[0])
        assert (rw, rh) == (-(-img.width // p[0]), -(-img.height // p[0])) and p[1] + p[3] <= rw and p[2] + p[4] <= rh
        out.append(pre_resize_image(crop(px, rw, rh, rpf, p[1:]), rpf, rect, p, ow, oh, m))
    return out, plans


def pre_decoder(G, lib, S, pf=None, cs=None, align=None, perf=False):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib, pf, cs, align)
    if perf and pf is not None:
        dec.set_output_format(cs, pf)
    assert dec.set_option(PRE, NAME[S]) == 0
    return dec


# ================================================================================================ 1. the definition alone
def test_taps_at_scale_1_are_the_unprescaled_taps():
    for n_src, n_out in ((1, 1), (7, 5), (5, 7), (480, 24), (100, 100), (65535, 16384), (3, 16384)):
        for a, b in zip(pre_taps(n_src, n_out, 0, 1, n_src), taps(n_src, n_out)):
            assert np.array_equal(a, b), (n_src, n_out)


SWEEP_W = (119, 120, 333, 1)


def sweep():
    """(W, rect, OW, S): origins and widths around the multiples of s, rectangles that end at the edge of a W that is no multiple of s"""
    rng = np.random.default_rng(5)
    for W in SWEEP_W:
        for S in (1, 2, 4, 8):
            for _ in range(60):
                x = int(rng.integers(0, W))
                w = int(rng.integers(1, W - x + 1))
                if rng.integers(0, 3) == 0:
                    w = W - x
                yield W, (x, 0, w, 61), int(rng.integers(1, max(w // max(int(rng.integers(1, 9)), 1), 1) + 1)), S


def test_first_tap_lies_inside_the_covering_rectangle():
    seen = set()
    for W, rect, ow, S in sweep():
        s, xr, _, wr, _ = plan(W, 61, True, rect, ow, 1, S)
        seen.add(s)
        x0, x1, f = pre_taps(rect[2], ow, rect[0] - s * xr, s, wr)
        assert 0 <= x0.min() and x0.max() <= wr - 1 and x1.max() <= wr - 1 and 0 <= f.min() and f.max() <= 255, (W, rect, ow, S)
        assert (xr + wr) <= -(-W // s) and 0 <= rect[0] - s * xr < s
    assert seen == {1, 2, 4, 8}


def test_host_plan_equals_the_numpy_plan(G, lib):
    for W, rect, ow, S in sweep():
        for ok in (True, False):
            assert G.crop_resize_plan(lib, W, 61, ok, rect, ow, 1, S) == plan(W, 61, ok, rect, ow, 1, S), (W, rect, ow, S, ok)
    # both axes, and h as the limit
    assert G.crop_resize_plan(lib, 480, 272, 1, (3, 50, 400, 40), 24, 16, 8) == plan(480, 272, True, (3, 50, 400, 40), 24, 16, 8) == (2, 1, 25, 201, 20)
    # what the call refuses
    for args in ((480, 272, 1, (0, 0, 481, 10), 8, 8, 8), (480, 272, 1, (-1, 0, 10, 10), 8, 8, 8), (480, 272, 1, (0, 0, 10, 0), 8, 8, 8),
                 (480, 272, 1, (0, 270, 10, 3), 8, 8, 8), (480, 272, 1, (0, 0, 10, 10), 0, 8, 8), (480, 272, 1, (0, 0, 10, 10), 8, 16385, 8),
                 (480, 272, 1, (0, 0, 10, 10), 8, 8, 3), (480, 272, 1, (0, 0, 10, 10), 8, 8, 16)):
        assert G.crop_resize_plan(lib, *args) is None, args


def area_average(c, ow, oh):
    """the exact area average of c (h, w, channels) over the ow x oh grid, float64"""
    def weights(n_src, n_out):
        e = np.arange(n_out + 1) * n_src / n_out
        p = np.arange(n_src)
        return np.clip(np.minimum(e[1:, None], p[None, :] + 1) - np.maximum(e[:-1, None], p[None, :]), 0, None) * n_out / n_src
    h, w = c.shape[:2]
    return np.einsum("jy,yxc,ix->jic", weights(h, oh), c.astype(np.float64), weights(w, ow))


QUALITY = [("rgb_natural_auto", (17, 9, 600, 350), 64, 40, 8), ("rgb_natural_auto", (3, 5, 520, 330), 120, 80, 4), ("rgb_hdlike_r24", (0, 0, 480, 272), 56, 32, 8)]


@pytest.mark.parametrize("name,rect,ow,oh,s", QUALITY, ids=[f"{q[0]}_to_{q[2]}x{q[3]}" for q in QUALITY])
def test_prescaled_definition_is_nearer_the_area_average(O, name, rect, ow, oh, s):
    """natural content, s >= 4: mean squared error against the exact area average of the full-size oracle crop, all channels -- the restatement with the
    prescale strictly below the unprescaled definition (7.36 / 4.47 / 6.92 against 0.60 / 0.98 / 0.64 when the option was proposed)"""
    case = case_named(name)
    jpeg = case_stream(O, case)
    full, img = O.decode(jpeg)
    ideal = area_average(crop(full, img.width, img.height, 1, rect).reshape(rect[3], rect[2], 3), ow, oh)
    (pre,), (p,) = expected(O, [jpeg], [rect], ow, oh, 8)
    assert p[0] == s
    (today,) = plain_expected(O, [jpeg], [rect], ow, oh)
    mse_pre = float(np.mean((pre.reshape(oh, ow, 3) - ideal) ** 2))
    mse_today = float(np.mean((today.reshape(oh, ow, 3) - ideal) ** 2))
    print(f"{name} {rect} -> {ow}x{oh}, s = {s}: MSE today {mse_today:.2f}, prescaled {mse_pre:.2f}")
    assert mse_pre < mse_today


# ================================================================================================ 2. every scale in one batch
HD_CASE = "rgb_hdlike_r24"
OW, OH = 24, 16
# scale 1 (too narrow), 2, 4, 8, h as the limit (2), the whole image (8), a rectangle that ends at both edges (8), 4 at odd origins
HD_RECTS = [(13, 21, 40, 30), (7, 9, 60, 40), (33, 5, 100, 70), (101, 43, 200, 130), (3, 50, 400, 40), (0, 0, 480, 272), (279, 141, 201, 131), (251, 99, 97, 65)]
HD_SCALES = [1, 2, 4, 8, 2, 8, 8, 4]
HD_MIRROR = [f & 1 for f in range(8)]


@pytest.fixture(scope="module")
def hd(O):
    """the streams of tests 2, 3 and 8 and their expected frames at every S, made once"""
    streams = frames_of(O, case_named(HD_CASE), len(HD_RECTS))
    want = {S: expected(O, streams, HD_RECTS, OW, OH, S, mirror=HD_MIRROR) for S in (1, 2, 4, 8)}
    assert [p[0] for p in want[8][1]] == HD_SCALES
    assert any(r[0] % 8 and r[1] % 8 for r in HD_RECTS) and any(p[0] > 1 and (r[0] % p[0] or r[1] % p[0]) for r, p in zip(HD_RECTS, want[8][1]))
    return streams, want


def test_every_scale_in_one_batch(O, G, dlib, hd):
    streams, want = hd
    want, plans = want[8]
    n = len(streams)
    singles = region_stats_of(G, dlib, streams, [expanded(480, 272, p) for p in plans])
    for chunk in (3, 0):
        dec = pre_decoder(G, dlib, 8, perf=True)
        if chunk:
            dec.set_batch_chunk(chunk)
        for rep in range(2):
            got, pi = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
            assert (pi.width, pi.height, pi.pixel_format) == (OW, OH, 1) and dlib.image_size(pi) == OW * OH * 3
            assert same(got, want), (chunk, rep, diffs(got, want))
            assert dec.prescales() == HD_SCALES
            assert dec.idct_path() == 6
            batched, single = dec.last_batch()
            assert batched + single == n and single <= 1, (batched, single)
            st = dec.region_stats()
            assert st[0] == 1 and st[1:] == tuple(sum(s[i] for s in singles) for i in (1, 2, 3)), (st, singles)
        dec.close()


# ================================================================================================ 3. S caps the scale
@pytest.mark.parametrize("S", [2, 4])
def test_option_caps_the_scale(O, G, dlib, hd, S):
    streams, want = hd
    want, plans = want[S]
    assert max(p[0] for p in plans) == S
    dec = pre_decoder(G, dlib, S, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.prescales() == [min(s, S) for s in HD_SCALES] == [p[0] for p in plans] and dec.idct_path() == 6
    dec.close()


def test_option_at_1_is_the_call_without_it(O, G, dlib, hd):
    streams, want = hd
    plain = perf_decoder(G, dlib)  # (a decoder that never saw the option)
    ref, _ = plain.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
    ref_stats = plain.region_stats()
    plain.close()
    assert same(ref, want[1][0])
    dec = pre_decoder(G, dlib, 8, perf=True)
    got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
    assert same(got, want[8][0]) and dec.idct_path() == 6
    assert dec.set_option(PRE, "1") == 0
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
        assert same(got, ref), (rep, diffs(got, ref))
        assert dec.prescales() == [1] * len(streams) and dec.idct_path() == 5 and dec.region_stats() == ref_stats
    dec.close()


# ================================================================================================ 4. edges
EDGES = [("odd_noise", "rgb_odd_noise", [(0, 0, 119, 61), (63, 37, 56, 24), (1, 1, 117, 59)], 7, 3, [8, 8, 8]),
         ("interleaved_mcu_covers", "rgb_interleaved", [(200, 60, 133, 63), (5, 7, 100, 50), (301, 101, 32, 22), (0, 0, 333, 123)], 7, 3, [8, 8, 4, 8]),
         ("to_1x1", HD_CASE, [(0, 0, 480, 272), (10, 10, 5, 3), (100, 100, 1, 1), (473, 265, 7, 7)], 1, 1, [8, 2, 1, 4])]


@pytest.mark.parametrize("ident,name,rects,ow,oh,scales", EDGES, ids=[e[0] for e in EDGES])
def test_edges(O, G, dlib, ident, name, rects, ow, oh, scales):
    streams = frames_of(O, case_named(name), len(rects), seed=50)
    want, plans = expected(O, streams, rects, ow, oh, 8)
    assert [p[0] for p in plans] == scales
    dec = pre_decoder(G, dlib, 8)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert (pi.width, pi.height) == (ow, oh) and same(got, want), (rep, diffs(got, want))
        assert dec.prescales() == scales  # (rgb_odd_noise goes frame by frame, with or without the option: one restart segment per scan)
    dec.close()


# ================================================================================================ 5. configurations
# (id, case, output pixel format / colour space or None = the stream's, line alignment)
CONFIGS = [("gray_to_u8", "gray", None, None, 0), ("gray_to_rgb", "gray", 1, 1, 0), ("rgba_4444", "rgba_4444", None, None, 0),
           ("planar444_no_transform", "planar444_in", None, None, 0), ("rgb_bt709", "rgb_bt709", None, None, 0), ("rgb_interleaved_aligned", "rgb_interleaved", None, None, 64)]


@pytest.mark.parametrize("ident,name,pf,cs,align", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_configurations(O, G, dlib, ident, name, pf, cs, align):
    case = case_named(name)
    w, h = case[1], case[2]
    pf, cs = (case[3], case[4]) if pf is None else (pf, cs)
    ow, oh = 7, 5
    # the whole image, odd origins at scales 2 and 4 (where the image has room), the far corner, a rectangle smaller than the output
    rects = [(0, 0, w, h), (1, 3, min(2 * ow + 3, w - 1), min(2 * oh + 1, h - 3)), (w - min(4 * ow + 1, w), h - min(4 * oh + 2, h), min(4 * ow + 1, w), min(4 * oh + 2, h)),
             (w // 3 | 1, h // 2 | 1, 5, 3)]
    streams = frames_of(O, case, 4, seed=40)
    want, plans = expected(O, streams, rects, ow, oh, 8, pf, cs)
    assert len({p[0] for p in plans}) >= 3, plans
    bpp = BPP.get(pf)
    pad = (-(ow * bpp)) % align if align else 0

    def pixels(frames):  # (dec_opt_alignment_bytes pads the output's lines: what lies in the padding is nobody's)
        return [px[:oh * (ow * bpp + pad)].reshape(oh, ow * bpp + pad)[:, :ow * bpp].reshape(-1) for px in frames] if pad else frames

    dec = pre_decoder(G, dlib, 8, pf, cs, align)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert (pi.width, pi.height, pi.pixel_format, pi.width_padding) == (ow, oh, pf, pad)
        assert (pad != 0) == bool(align) and all(a.size == dlib.image_size(pi) for a in got)
        assert same(pixels(got), want), (rep, diffs(pixels(got), want))
        assert dec.prescales() == [p[0] for p in plans] and dec.last_batch()[1] <= 1
    dec.close()


# ================================================================================================ 6. subsampled streams are left alone
@pytest.mark.parametrize("name", ["rgb_to_420_il", "rgb_to_422_nonil"])
def test_subsampled_streams_take_no_prescale(O, G, dlib, name):
    case = case_named(name)
    w, h = case[1], case[2]
    rects = [(0, 0, w, h), (1, 3, w - 2, h - 5), (w // 2, h // 2, w // 2, h // 2)]
    streams = frames_of(O, case, 3, seed=44)
    assert all(plan(w, h, True, r, 8, 6, 8)[0] >= 4 for r in rects), "a 4:4:4 stream would be prescaled here"
    plain = new_decoder(G, dlib, 1, 1)
    ref, _ = plain.decode_batch_crop_resize(streams, rects, 8, 6)
    plain.close()
    assert same(ref, expected(O, streams, rects, 8, 6, 8, 1, 1, all_1x1=False)[0])
    dec = pre_decoder(G, dlib, 8, 1, 1, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, 8, 6)
        assert same(got, ref), (rep, diffs(got, ref))
        assert dec.prescales() == [1, 1, 1] and dec.idct_path() == 5
    dec.close()


# ================================================================================================ 7. frame-by-frame routes
def test_restart_interval_0_goes_frame_by_frame(O, G, dlib):
    streams = frames_of(O, case_named("rgb_restart0"), 3, seed=60)
    rects = [(0, 0, 100, 60), (59, 35, 41, 25), (33, 17, 11, 30)]
    want, plans = expected(O, streams, rects, 6, 4, 8, mirror=[0, 1, 0])
    assert [p[0] for p in plans] == [8, 4, 1]
    dec = pre_decoder(G, dlib, 8, perf=True)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, 6, 4, mirror=[0, 1, 0])
        assert same(got, want) and (pi.width, pi.height) == (6, 4), (rep, diffs(got, want))
        assert dec.last_batch() == (0, 3) and dec.idct_path() == 6 and dec.prescales() == [8, 4, 1]
        st = dec.region_stats()
        assert st[0] == 2 and st[1] == st[3] == 9, st
    dec.close()


def test_single_frame_route_gives_the_batched_bytes(O, G, dlib, hd):
    """host output: frame 0 of every call goes through the single-frame region call, on a fresh decoder (its first call) and on one with a header to
    launch on; every frame of the batch takes that place once and gives the bytes it gives inside the batched launches"""
    streams, want = hd
    want = want[8][0]
    n = len(streams)
    for first in range(n):
        order = [first] + [f for f in range(n) if f != first][:2]
        dec = pre_decoder(G, dlib, 8)
        for rep in range(2):
            got, _ = dec.decode_batch_crop_resize([streams[f] for f in order], [HD_RECTS[f] for f in order], OW, OH, mirror=[HD_MIRROR[f] for f in order])
            assert same(got, [want[f] for f in order]), (first, rep)
            assert dec.prescales() == [HD_SCALES[f] for f in order] and dec.last_batch()[1] >= 1
        dec.close()


def test_damaged_restart_markers_in_one_frame(O, G, emu, hd):
    """(CPU tier only) frame 3's restart markers are damaged (scale 8): it goes through the single-frame route, its neighbours stay in the batched
    launches and equal the restatement; what the damaged frame gives is what that route gives it alone, on a decoder of the same state"""
    streams, want = hd
    want = want[8][0][:5]
    streams, rects, flags = streams[:5], HD_RECTS[:5], HD_MIRROR[:5]
    for kind, bad, _ in damaged_restart_markers(streams[3]):
        ref = pre_decoder(G, emu, 8)
        try:
            ref.decode_batch_crop_resize([streams[0]], [rects[0]], OW, OH)  # (a header to launch on, as the batch call has when it reaches frame 3)
            want3 = ref.decode_batch_crop_resize([bad], [rects[3]], OW, OH, mirror=[flags[3]])[0][0]
        except RuntimeError:
            want3 = None
        ref.close()
        mixed = streams[:3] + [bad] + streams[4:]
        dec = pre_decoder(G, emu, 8)
        for rep in range(2):
            if want3 is None:
                with pytest.raises(RuntimeError):
                    dec.decode_batch_crop_resize(mixed, rects, OW, OH, mirror=flags)
                continue
            got, _ = dec.decode_batch_crop_resize(mixed, rects, OW, OH, mirror=flags)
            assert same(got[:3] + got[4:], want[:3] + want[4:]), (kind, rep)
            assert np.array_equal(got[3], want3), (kind, rep)
            batched, single = dec.last_batch()
            assert 1 <= single <= 2 and batched >= 3, (kind, batched, single)
            assert dec.prescales() == HD_SCALES[:5]
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH, mirror=flags)  # the decoder decodes the intact streams as ever
        assert same(got, want), kind
        dec.close()


# ================================================================================================ 8. refusals and state
def test_refusals_with_the_option_set(O, G, dlib, capfd, monkeypatch):
    """every refusal of the call without the option, dec_opt_scale = 1/2 among them, on decoders that have dec_opt_resize_prescale = 1/8: the body of
    test_crop_resize's test with its decoders and its expected frames replaced"""
    def with_option(G_, lib, *a):
        dec = new_decoder(G_, lib, *a)
        assert dec.set_option(PRE, "1/8") == 0
        return dec

    def want(O_, streams, rects, ow, oh, *a, **kw):
        frames, plans = expected(O_, streams, rects, ow, oh, 8, *a, **kw)
        assert max(p[0] for p in plans) == 8
        return frames

    monkeypatch.setattr(base, "new_decoder", with_option)
    monkeypatch.setattr(base, "expected", want)
    base.test_refusals_write_nothing_and_leave_the_decoder_usable(O, G, dlib, capfd)


def test_bad_option_values_are_refused_and_the_setting_is_kept(O, G, dlib, hd, capfd):
    streams, want = hd
    dec = pre_decoder(G, dlib, 4)
    for bad in ("1/3", "2", "", "1/16", "8", "1/8 ", "full", "0"):
        capfd.readouterr()
        assert dec.set_option(PRE, bad) != 0, bad
        assert "[Error]" in capfd.readouterr().err
    got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
    assert same(got, want[4][0]) and dec.prescales() == [min(s, 4) for s in HD_SCALES]
    dec.close()


def test_guard_bytes(O, G, dlib, hd):
    """an output stride larger than a frame and a frame size (13 x 5 x 3 = 195 bytes) that is no multiple of 4: the bytes between the slots and behind
    the last one are untouched"""
    streams, _ = hd
    ow, oh = 13, 5
    want, plans = expected(O, streams, HD_RECTS, ow, oh, 8, mirror=HD_MIRROR)
    assert {p[0] for p in plans} == {2, 4, 8}
    n, raw = len(streams), ow * oh * 3
    stride = raw + 29
    dec = pre_decoder(G, dlib, 8)
    for rep in range(2):
        out = np.full(stride * n + 64, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, HD_RECTS, ow, oh, out, stride, mirror=HD_MIRROR) == 0
        rows = out[:stride * n].reshape(n, stride)
        assert all(np.array_equal(rows[f, :raw], want[f]) for f in range(n)), (rep, [int(np.count_nonzero(rows[f, :raw] != want[f])) for f in range(n)])
        assert np.all(rows[:, raw:] == 0xA5) and np.all(out[stride * n:] == 0xA5), rep
    dec.close()


@pytest.mark.parametrize("mode", ["GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS"])
def test_state_between_calls(O, G, dlib, hd, mode, monkeypatch):
    """prescaled and unprescaled calls, a plain decode, a region decode and a dec_opt_scale decode on one decoder: each equals its own expectation, and
    the option touches none of the others"""
    monkeypatch.setenv(mode, "1")
    streams, want = hd
    region = (101, 43, 200, 130)
    full3 = O.decode(streams[3])[0]
    half3 = scaled_expected(O, streams[3], -1, -1, 2)[0]
    dec = pre_decoder(G, dlib, 8, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
        assert same(got, want[8][0]) and dec.idct_path() == 6, (rep, diffs(got, want[8][0]))
        px, pi = dec.decode(streams[3])
        assert (pi.width, pi.height) == (480, 272) and np.array_equal(px, full3), rep
        assert dec.set_option(PRE, "1") == 0
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=HD_MIRROR)
        assert same(got, want[1][0]) and dec.idct_path() == 5, (rep, diffs(got, want[1][0]))
        assert dec.set_option(PRE, "1/8") == 0
        assert dec.set_option(OPT, opt_value(region)) == 0
        px, pi = dec.decode(streams[3])
        assert (pi.width, pi.height) == (200, 130) and np.array_equal(px, crop(full3, 480, 272, 1, region)), rep
        got, _ = dec.decode_batch_crop_resize(streams[:4], HD_RECTS[:4], OW, OH)  # (the decoder's own region is neither read nor changed)
        assert same(got, expected(O, streams[:4], HD_RECTS[:4], OW, OH, 8)[0]), rep
        assert dec.set_option(OPT, "full") == 0
        assert dec.set_option("dec_opt_scale", "1/2") == 0
        px, pi = dec.decode(streams[3])
        assert (pi.width, pi.height) == (240, 136) and np.array_equal(px, half3), rep
        with pytest.raises(RuntimeError):
            dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH)
        assert dec.prescales() == []
        assert dec.set_option("dec_opt_scale", "1") == 0
    dec.close()


# ================================================================================================ 9. GPU only
@pytest.mark.gpu
def test_device_streams_and_device_output(O, G, gpu_lib):
    import torch
    case = case_named("rgb_natural_auto")  # 640 x 368
    ow = oh = 32
    rects = [(0, 0, 640, 368), (13, 7, 300, 260), (301, 55, 140, 135), (77, 101, 70, 66), (5, 3, 60, 33), (383, 111, 257, 257), (9, 300, 600, 64), (555, 299, 85, 69)]
    flags = [0, 1, 0, 0, 1, 1, 0, 1]
    streams = frames_of(O, case, len(rects), seed=70)
    want, plans = expected(O, streams, rects, ow, oh, 8, mirror=flags)
    scales = [p[0] for p in plans]
    assert set(scales) == {1, 2, 4, 8}
    n, raw = len(streams), ow * oh * 3
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    d_in = torch.from_numpy(host).cuda()
    out_stride = raw + 61
    d_out = torch.full((out_stride * n,), 0xA5, dtype=torch.uint8, device="cuda")
    dec = pre_decoder(G, gpu_lib, 8, perf=True)
    for rep in range(2):
        d_out.fill_(0xA5)
        _, pi = dec.decode_batch_crop_resize(None, rects, ow, oh, mirror=flags, device_out=d_out.data_ptr(), out_stride=out_stride,
                                             device_in=d_in.data_ptr(), in_stride=in_stride, sizes=sizes)
        torch.cuda.synchronize()
        rows = d_out.cpu().numpy().reshape(n, out_stride)
        assert (pi.width, pi.height) == (ow, oh)
        assert all(np.array_equal(rows[f, :raw], want[f]) for f in range(n)), (rep, [int(np.count_nonzero(rows[f, :raw] != want[f])) for f in range(n)])
        assert np.all(rows[:, raw:] == 0xA5), rep
        assert dec.prescales() == scales and dec.idct_path() == 6 and dec.region_stats()[0] == 1
    assert dec.last_batch() == (n, 0), "the second call has a header to launch on: every frame through the batched launches"
    dec.close()
