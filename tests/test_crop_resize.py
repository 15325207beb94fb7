"""Batched crop-and-resize, one rectangle per frame (gpujpeg_amd_decoder_decode_batch_crop_resize; gpujpeg_amd_ext.h).

The definition of frame f's result is the bilinear resize -- half-pixel centres, 8-bit weights, integer arithmetic, stated in the header -- of what
the single-frame region call returns for rectangle f. Expected bytes are a numpy restatement of that definition (resize_image below) applied to the
cropped ORACLE decode (oracle.decode + a numpy crop, no product code); every comparison with the library is byte for byte.

Two tiers with the same bodies, like test_region_batch.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Damaged streams and the random configurations run on the CPU tier only."""
import ctypes as C

import numpy as np
import pytest

from conftest import natural_image, oracle_image, random_case, random_raw
from test_region_batch import dlib, emu, frames_of, new_decoder, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import OPT, case_named, case_stream, crop, damaged_restart_markers, opt_value, perf_decoder

BPP = {0: 1, 1: 3, 6: 4}  # packed formats; 2 = planar 4:4:4 (three planes)
ALLOWED = [0, 1, 2, 6]    # output formats whose pixels share no samples


# ================================================================================================ the definition, in numpy
def taps(n_src, n_out):
    """source positions and 8-bit weight of the n_out output samples along one axis of an n_src-sample crop"""
    i = np.arange(n_out, dtype=np.int64)
    n = np.maximum((2 * i + 1) * n_src - n_out, 0)
    p0 = n // (2 * n_out)
    f = ((n - p0 * 2 * n_out) * 256) // (2 * n_out)
    return p0, np.minimum(p0 + 1, n_src - 1), f


def resize_channels(c, ow, oh):
    """c: (h, w, channels) uint8 -> (oh, ow, channels) uint8 by the definition"""
    h, w = c.shape[:2]
    x0, x1, fx = taps(w, ow)
    y0, y1, fy = taps(h, oh)
    c = c.astype(np.int64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = c[y0][:, x0] * (256 - fx) + c[y0][:, x1] * fx
    bot = c[y1][:, x0] * (256 - fx) + c[y1][:, x1] * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)


def resize_image(c, w, h, pf, ow, oh, mirror=False):
    """the w x h image c of pixel format pf (no line padding) -> the ow x oh image of the same format, mirrored horizontally on request"""
    if pf in BPP:
        r = resize_channels(c.reshape(h, w, BPP[pf]), ow, oh)
        return (r[:, ::-1] if mirror else r).reshape(-1)
    assert pf == 2
    r = resize_channels(c.reshape(3, h, w).transpose(1, 2, 0), ow, oh)
    return (r[:, ::-1] if mirror else r).transpose(2, 0, 1).reshape(-1)


def expected(O, streams, rects, ow, oh, pf=None, cs=None, mirror=None):
    """the restatement over the cropped oracle decodes -> one array per frame"""
    out = []
    for f, (jpeg, rect) in enumerate(zip(streams, rects)):
        raw, img = O.decode(jpeg, -1 if pf is None else pf, -1 if cs is None else cs)
        c = crop(raw, img.width, img.height, img.pixel_format, rect)
        out.append(resize_image(c, rect[2], rect[3], img.pixel_format, ow, oh, bool(mirror and mirror[f])))
    return out


def region_stats_of(G, lib, streams, rects, pf=None, cs=None):
    """gpujpeg_amd_decoder_get_region_stats of the single-frame region call of every rectangle"""
    dec = new_decoder(G, lib, pf, cs)
    out = []
    for jpeg, rect in zip(streams, rects):
        assert dec.set_option(OPT, opt_value(rect)) == 0
        dec.decode(jpeg)
        out.append(dec.region_stats())
    dec.close()
    return out


def raw_call(G, lib, dec, streams, rects, ow, oh, out, stride, mirror=None):
    """the C call with a caller-owned host output buffer -> return code"""
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    buf = np.zeros(in_stride * len(sizes), np.uint8)
    for i, x in enumerate(streams):
        buf[i * in_stride:i * in_stride + x.size] = x
    n = len(sizes)
    csz = (C.c_size_t * n)(*sizes)
    rc4 = (C.c_int * (4 * n))(*[int(v) for r in rects for v in r])
    mir = None if mirror is None else (C.c_uint8 * n)(*mirror)
    pi = G.ImageParameters()
    return lib.L.gpujpeg_amd_decoder_decode_batch_crop_resize(dec.h, buf.ctypes.data, in_stride, csz, n, rc4, mir, ow, oh, out.ctypes.data, stride, C.byref(pi))


def diffs(got, want):
    return [int(np.count_nonzero(a != b)) if a.size == b.size else -1 for a, b in zip(got, want)]


# ================================================================================================ 1. the definition alone
def float_resize(c, ow, oh):
    """the same interpolation in float64, rounded once"""
    h, w = c.shape[:2]
    sx = np.maximum((np.arange(ow) + 0.5) * w / ow - 0.5, 0.0)
    sy = np.maximum((np.arange(oh) + 0.5) * h / oh - 0.5, 0.0)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (sx - x0)[None, :, None], (sy - y0)[:, None, None]
    c = c.astype(np.float64)
    top = c[y0][:, x0] * (1 - fx) + c[y0][:, x1] * fx
    bot = c[y1][:, x0] * (1 - fx) + c[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def test_definition_is_the_identity_at_equal_size():
    rng = np.random.default_rng(1)
    for w, h in ((1, 1), (7, 5), (64, 48), (100, 3)):
        c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(resize_channels(c, w, h), c)
        assert np.array_equal(resize_image(c.reshape(-1), w, h, 1, w, h), c.reshape(-1))
        assert np.array_equal(resize_image(c.reshape(-1), w, h, 1, w, h, True), c[:, ::-1].reshape(-1))


def test_definition_against_float_and_torch():
    """<= 2 levels from the float64 interpolation rounded once and from torch's bilinear (align_corners=False, no antialiasing): each 8-bit weight is
    truncated by less than 1/256, which moves a value by less than one level per axis, plus the two roundings"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(2)
    crops = []
    for w, h in ((100, 45), (37, 150), (9, 7), (1, 1), (1, 33), (41, 1), (301, 9)):
        crops.append(natural_image(w, h, 3, seed=w + h).reshape(h, w, 3))
        crops.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    worst_f = worst_t = 0.0
    for c in crops:
        for ow, oh in ((32, 24), (64, 48), (7, 5), (1, 1), (13, 5), (149, 211)):
            r = resize_channels(c, ow, oh).astype(np.float64)
            worst_f = max(worst_f, float(np.max(np.abs(r - np.rint(float_resize(c, ow, oh))))))
            t = F.interpolate(torch.from_numpy(c.astype(np.float64)).permute(2, 0, 1)[None], size=(oh, ow), mode="bilinear", align_corners=False)
            worst_t = max(worst_t, float(np.max(np.abs(r - np.rint(t[0].permute(1, 2, 0).numpy())))))
    print(f"largest difference: {worst_f} levels from float64, {worst_t} levels from torch.nn.functional.interpolate")
    assert worst_f <= 2 and worst_t <= 2


# ================================================================================================ 2. rectangles differ per frame
# six frames of rgb_hdlike_r24 (480 x 272, 60 blocks per row, restart interval 24: segments wrap rows) resampled to 32 x 24: the whole image, a
# rectangle that ends at both edges, a tall one, a flat one, one pixel, the identity
HD_CASE = "rgb_hdlike_r24"
HD_RECTS = [(0, 0, 480, 272), (380, 227, 100, 45), (13, 20, 37, 150), (100, 3, 301, 9), (205, 100, 1, 1), (64, 68, 32, 24)]
OW, OH = 32, 24


@pytest.fixture(scope="module")
def hd(O):
    """the streams of tests 2, 3, 4 and their expected frames, made once"""
    streams = frames_of(O, case_named(HD_CASE), len(HD_RECTS))
    covers = {((x % 8 + w - 1) // 8 + 1, (y % 8 + h - 1) // 8 + 1) for x, y, w, h in HD_RECTS}
    assert len(covers) >= 3, "the rectangles give covers of fewer than three block sizes: the test shows nothing"
    return streams, expected(O, streams, HD_RECTS, OW, OH)


def rectangles_body(O, G, lib, hd):
    streams, want = hd
    n = len(streams)
    singles = region_stats_of(G, lib, streams, HD_RECTS)
    assert len({s[1] for s in singles}) >= 3, "the rectangles select the same number of segments in every frame: the test shows nothing"
    for chunk in (0, 2):
        dec = perf_decoder(G, lib)
        if chunk:
            dec.set_batch_chunk(chunk)
        for rep in range(2):
            got, pi = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH)
            assert (pi.width, pi.height, pi.pixel_format, pi.color_space) == (OW, OH, 1, 1) and lib.image_size(pi) == OW * OH * 3
            assert same(got, want), (chunk, rep, diffs(got, want))
            batched, single = dec.last_batch()
            assert batched + single == n and single <= 1, (batched, single)
            assert dec.idct_path() == 5
            st = dec.region_stats()
            assert st[0] == 1 and st[1] == sum(s[1] for s in singles) < n * singles[0][3], st
            assert st[2] == sum(s[2] for s in singles) and st[3] == sum(s[3] for s in singles), st
        dec.close()


def test_rectangles_differ_per_frame(O, G, dlib, hd):
    rectangles_body(O, G, dlib, hd)


# ================================================================================================ 3. null entries as whole batches
def test_null_entries_fill_whole_batches(O, G, dlib, hd, monkeypatch):
    """GJ_DEC_G=1: one table entry per batch of the entropy decoder, so the null entries behind a frame's own selection -- the one-pixel rectangle's
    table is padded to the whole image's -- are batches of their own"""
    monkeypatch.setenv("GJ_DEC_G", "1")
    rectangles_body(O, G, dlib, hd)


# ================================================================================================ 4. mirror
def test_mirror(O, G, dlib, hd):
    streams, want = hd
    flags = [1, 0, 1, 0, 1, 0]
    mirrored = [w.reshape(OH, OW, 3)[:, ::-1].reshape(-1) if m else w for w, m in zip(want, flags)]
    assert same(mirrored, expected(O, streams[:2], HD_RECTS[:2], OW, OH, mirror=flags[:2]) + mirrored[2:])
    dec = new_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=flags)
        assert same(got, mirrored), (rep, diffs(got, mirrored))
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=[0] * 6)
        assert same(got, want), rep
        got, _ = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=None)
        assert same(got, want), rep
    dec.close()


# ================================================================================================ 5. configurations
# (id, case, output pixel format / colour space or None = the stream's, line alignment)
CONFIGS = [("420_il_to_rgb", "rgb_to_420_il", 1, 1, 0), ("420_il_to_planar444", "rgb_to_420_il", 2, 3, 0), ("422_nonil_to_rgb", "rgb_to_422_nonil", None, None, 0),
           ("rgb_interleaved_aligned", "rgb_interleaved", None, None, 64), ("gray_to_u8", "gray", None, None, 0), ("gray_to_rgb", "gray", 1, 1, 0),
           ("rgba_4444", "rgba_4444", None, None, 0), ("planar444_no_transform", "planar444_in", None, None, 0)]


@pytest.mark.parametrize("ident,name,pf,cs,align", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_configurations(O, G, dlib, ident, name, pf, cs, align):
    case = case_named(name)
    w, h = case[1], case[2]
    pf, cs = (case[3], case[4]) if pf is None else (pf, cs)
    ow, oh = 21, 13
    # odd origins and odd sizes (chroma samples shared between neighbours), the far corner, a rectangle smaller than the output
    rects = [(1, 3, 37, 29), (w - 45, h - 31, 45, 31), (w // 3 | 1, h // 2 | 1, 9, 5), (0, 0, w, h)]
    assert all(x >= 0 and y >= 0 and x + rw <= w and y + rh <= h for x, y, rw, rh in rects)
    streams = frames_of(O, case, 4, seed=40)
    want = expected(O, streams, rects, ow, oh, pf, cs)
    bpp = BPP.get(pf)
    pad = (-(ow * bpp)) % align if align else 0

    def pixels(frames):  # (dec_opt_alignment_bytes pads the output's lines: what lies in the padding is nobody's)
        return [px[:oh * (ow * bpp + pad)].reshape(oh, ow * bpp + pad)[:, :ow * bpp].reshape(-1) for px in frames] if pad else frames

    singles = region_stats_of(G, dlib, streams, rects, pf, cs)
    dec = new_decoder(G, dlib, pf, cs, align)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert (pi.width, pi.height, pi.pixel_format, pi.width_padding) == (ow, oh, pf, pad)
        assert (pad != 0) == bool(align) and all(a.size == dlib.image_size(pi) for a in got)
        assert same(pixels(got), want), (rep, diffs(pixels(got), want))
        assert dec.last_batch()[1] <= 1, dec.last_batch()
        st = dec.region_stats()
        assert st[0] == 1 and st[1:] == tuple(sum(s[i] for s in singles) for i in (1, 2, 3)), st
    dec.close()


# ================================================================================================ 6. up as well as down
@pytest.mark.parametrize("rect,ow,oh", [((203, 101, 9, 7), 64, 48), ((0, 0, 480, 272), 7, 5), ((0, 0, 480, 272), 1, 1)], ids=["up", "down", "to_1x1"])
def test_up_and_down(O, G, dlib, rect, ow, oh):
    streams = frames_of(O, case_named(HD_CASE), 3, seed=33)
    rects = [rect, (rect[0] + (1 if rect[2] < 480 else 0), rect[1], rect[2] - (0 if rect[2] < 480 else 1), rect[3]), rect]
    want = expected(O, streams, rects, ow, oh)
    dec = new_decoder(G, dlib)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert (pi.width, pi.height) == (ow, oh) and same(got, want), (rep, diffs(got, want))
    dec.close()


# ================================================================================================ 7. fallbacks
def test_restart_interval_0_goes_frame_by_frame(O, G, dlib):
    streams = frames_of(O, case_named("rgb_restart0"), 3, seed=60)
    rects = [(0, 0, 100, 60), (60, 35, 40, 25), (33, 17, 11, 30)]
    want = expected(O, streams, rects, 20, 16)
    dec = perf_decoder(G, dlib)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, 20, 16, mirror=[0, 1, 0])
        assert same(got, [want[0], want[1].reshape(16, 20, 3)[:, ::-1].reshape(-1), want[2]]) and (pi.width, pi.height) == (20, 16)
        assert dec.last_batch() == (0, 3) and dec.idct_path() == 5
        st = dec.region_stats()
        assert st[0] == 2 and st[1] == st[3] == 9, st
    dec.close()


def test_damaged_restart_markers_in_one_frame(O, G, emu):
    """(CPU tier only) frame 2's restart markers are damaged: it goes through the single-frame route -- its bytes are the restatement over what the
    single region call returns for that stream --, its neighbours stay in the batched launches and equal the restatement over the oracle"""
    streams, rects = frames_of(O, case_named(HD_CASE), 4), HD_RECTS[:4]
    good = expected(O, streams, rects, OW, OH)
    for kind, bad, _ in damaged_restart_markers(streams[2]):
        ref = new_decoder(G, emu)
        assert ref.set_option(OPT, opt_value(rects[0])) == 0
        ref.decode(streams[0])  # (a header to launch on, as the batch call has when it reaches frame 2)
        assert ref.set_option(OPT, opt_value(rects[2])) == 0
        try:
            want2 = resize_image(ref.decode(bad)[0], rects[2][2], rects[2][3], 1, OW, OH)
        except RuntimeError:
            want2 = None
        ref.close()
        mixed = streams[:2] + [bad] + streams[3:]
        dec = new_decoder(G, emu)
        for rep in range(2):
            if want2 is None:
                with pytest.raises(RuntimeError):
                    dec.decode_batch_crop_resize(mixed, rects, OW, OH)
                continue
            got, _ = dec.decode_batch_crop_resize(mixed, rects, OW, OH)
            assert same(got[:2] + got[3:], good[:2] + good[3:]), (kind, rep)
            assert np.array_equal(got[2], want2), (kind, rep)
            batched, single = dec.last_batch()
            assert 1 <= single <= 2 and batched >= 2, (kind, batched, single)
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)  # the decoder decodes the intact streams as ever
        assert same(got, good), kind
        dec.close()


def test_a_stream_of_another_size_fails_the_call(O, G, dlib):
    streams = frames_of(O, case_named(HD_CASE), 3)
    other = case_stream(O, case_named("rgb_natural_auto"))  # 640 x 368: the rectangles below lie inside it as well
    rects = [(0, 0, 64, 40), (8, 8, 30, 50), (16, 16, 100, 20)]
    dec = new_decoder(G, dlib)
    for rep in range(2):
        with pytest.raises(RuntimeError):
            dec.decode_batch_crop_resize([streams[0], other, streams[2]], rects, 16, 16)
        got, _ = dec.decode_batch_crop_resize(streams, rects, 16, 16)  # (and with a header to launch on the second time)
        assert same(got, expected(O, streams, rects, 16, 16))
    # the decoder's own region option across a call that fails part-way: the batch's rectangles travel in its calls' requests, never in the option
    own, full0 = (5, 7, 50, 40), O.decode(streams[0])[0]
    assert dec.set_option(OPT, opt_value(own)) == 0
    with pytest.raises(RuntimeError):
        dec.decode_batch_crop_resize([streams[0], other, streams[2]], rects, 16, 16)
    px, pi = dec.decode(streams[0])
    assert (pi.width, pi.height) == (50, 40) and np.array_equal(px, crop(full0, 480, 272, 1, own))
    got, _ = dec.decode_batch_crop_resize(streams, rects, 16, 16)
    assert same(got, expected(O, streams, rects, 16, 16))
    assert dec.set_option(OPT, "full") == 0
    px, pi = dec.decode(streams[0])
    assert (pi.width, pi.height) == (480, 272) and np.array_equal(px, full0) and dec.region_stats()[0] == 0
    dec.close()


# ================================================================================================ 8. refusals
def test_refusals_write_nothing_and_leave_the_decoder_usable(O, G, dlib, capfd):
    streams = frames_of(O, case_named(HD_CASE), 4)
    ok = HD_RECTS[:4]
    want = expected(O, streams, ok, OW, OH)
    stride = want[0].size + 32

    def refused(dec, rects, ow=OW, oh=OH, names=None):
        out = np.full(stride * 4, 0xA5, np.uint8)
        capfd.readouterr()
        assert raw_call(G, dlib, dec, streams, rects, ow, oh, out, stride) == -1, (rects, ow, oh)
        err = capfd.readouterr().err
        assert np.all(out == 0xA5), "a refused call wrote to the output"
        assert "[Error]" in err, "a refusal without a message"
        if names is not None:
            assert f"Frame {names} " in err, err

    def accepted(dec):
        out = np.full(stride * 4, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, ok, OW, OH, out, stride) == 0
        rows = out.reshape(4, stride)
        assert all(np.array_equal(rows[f, :want[f].size], want[f]) for f in range(4)) and np.all(rows[:, want[0].size:] == 0xA5)

    bad_rects = [(2, ok[:2] + [(480, 0, 10, 10)] + ok[3:]), (3, ok[:3] + [(0, 272, 5, 5)]), (1, ok[:1] + [(381, 0, 100, 45)] + ok[2:]), (3, ok[:3] + [(10, 228, 20, 45)]),
                 (0, [(-1, 0, 10, 10)] + ok[1:]), (2, ok[:2] + [(5, 5, 0, 10)] + ok[3:]), (1, ok[:1] + [(5, 5, 10, -2)] + ok[2:]), (0, [(0, 0, 481, 10)] + ok[1:]),
                 (3, ok[:3] + [(0, 0, 10, 273)])]
    for cold in (True, False):  # (without a header to launch on: frame 0 goes ahead; with one: the rectangles meet the cached header's geometry)
        dec = new_decoder(G, dlib)
        if not cold:
            accepted(dec)
        for frame, rects in bad_rects:
            refused(dec, rects, names=frame)
            if cold:
                accepted(dec)
                dec.close()
                dec = new_decoder(G, dlib)
        for ow, oh in ((0, OH), (OW, 0), (-3, -3), (16385, OH), (OW, 16385)):
            refused(dec, ok, ow, oh)
        accepted(dec)
        # a scale, a flip, a channel remap
        for opt, on, off in (("dec_opt_scale", "1/2", "1"), ("dec_opt_flipped", "1", "0"), ("dec_opt_channel_remap", "210", "")):
            assert dec.set_option(opt, on) == 0
            refused(dec, ok)
            assert dec.set_option(opt, off) == 0
            accepted(dec)
        # the decoder's own region, set beforehand, is still in force for a following single decode
        own = (5, 7, 50, 40)
        assert dec.set_option(OPT, opt_value(own)) == 0
        refused(dec, bad_rects[0][1], names=2)
        accepted(dec)
        px, pi = dec.decode(streams[0])
        assert (pi.width, pi.height) == (50, 40) and np.array_equal(px, crop(O.decode(streams[0])[0], 480, 272, 1, own))
        dec.close()
    # an output format the STREAM decides (the native one of a 4:2:0 stream: planar 4:2:0) -- refused with the stream's header in hand
    s420 = frames_of(O, case_named("planar420_in"), 2, seed=70)
    dec = new_decoder(G, dlib, G.PIXFMT_NATIVE, G.CS_DEFAULT)
    for rep in range(2):
        out = np.full(4096, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, s420, [(0, 0, 40, 40), (2, 2, 20, 20)], 16, 16, out, 2048) == -1 and np.all(out == 0xA5)
        assert dec.decode(s420[0])[1].pixel_format == 5
    dec.close()
    # output formats whose pixels share samples: packed 4:2:2, planar 4:2:2, planar 4:2:0
    even = [(0, 0, 480, 272), (380, 226, 100, 46), (12, 20, 38, 150), (100, 2, 300, 10)]
    for pf in (3, 4, 5):
        for cold in (True, False):
            dec = new_decoder(G, dlib, pf, 3)
            if not cold:
                dec.decode(streams[0])
            refused(dec, even)
            dec.set_output_format(1, 1)
            accepted(dec)
            dec.close()


# ================================================================================================ 9. state between calls
@pytest.mark.parametrize("mode", ["GJ_DEC_TOKENS", "GJ_DEC_NO_TOKENS"])
def test_state_between_calls(O, G, dlib, mode, monkeypatch):
    """crop-resize, a full-frame batch, a batch of regions, crop-resize with other rectangles on one decoder: the other calls may take the token
    route, this one takes the planes whatever the setting, and no call trusts what an earlier one left in the batch buffers"""
    monkeypatch.setenv(mode, "1")
    case = case_named(HD_CASE)
    streams, others = frames_of(O, case, 4), frames_of(O, case, 4, seed=90)
    A, B = HD_RECTS[:4], [(300, 200, 150, 60), (7, 90, 64, 48), (230, 11, 21, 200), (0, 0, 480, 272)]
    origins = [(300, 200), (7, 90), (230, 11), (111, 111)]
    want_a, want_b = expected(O, streams, A, OW, OH), expected(O, others, B, 48, 40, mirror=[0, 1, 1, 0])
    full_o = [O.decode(x)[0] for x in others]
    want_r = [crop(full_o[f], 480, 272, 1, origins[f] + (150, 60)) for f in range(4)]
    dec = perf_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, A, OW, OH)
        assert same(got, want_a) and dec.idct_path() == 5, (rep, diffs(got, want_a))
        got, pi = dec.decode_batch(others)
        assert same(got, full_o) and (pi.width, pi.height) == (480, 272), rep
        got, _ = dec.decode_batch_regions(others, origins, 150, 60)
        assert same(got, want_r) and dec.idct_path() == (4 if mode == "GJ_DEC_TOKENS" else 3), rep
        got, _ = dec.decode_batch_crop_resize(others, B, 48, 40, mirror=[0, 1, 1, 0])
        assert same(got, want_b) and dec.idct_path() == 5, (rep, diffs(got, want_b))
        px, _ = dec.decode(streams[3])
        assert np.array_equal(px, O.decode(streams[3])[0]), rep
    dec.close()


# ================================================================================================ 10. guard bytes
def test_guard_bytes(O, G, dlib):
    """an output stride larger than a frame, and a frame size (13 x 5 x 3 = 195 bytes) that is no multiple of 4: the bytes between the slots and behind
    the last one are untouched"""
    streams = frames_of(O, case_named(HD_CASE), 4)
    rects, ow, oh = HD_RECTS[:4], 13, 5
    want = expected(O, streams, rects, ow, oh)
    raw = ow * oh * 3
    stride = raw + 29
    dec = new_decoder(G, dlib)
    for rep in range(2):
        out = np.full(stride * 4 + 64, 0xA5, np.uint8)
        assert raw_call(G, dlib, dec, streams, rects, ow, oh, out, stride, mirror=[0, 0, 1, 0]) == 0
        rows = out[:stride * 4].reshape(4, stride)
        want_m = [want[0], want[1], want[2].reshape(oh, ow, 3)[:, ::-1].reshape(-1), want[3]]
        assert all(np.array_equal(rows[f, :raw], want_m[f]) for f in range(4)), rep
        assert np.all(rows[:, raw:] == 0xA5) and np.all(out[stride * 4:] == 0xA5), rep
    dec.close()


# ================================================================================================ 11. random configurations
SEEDS = range(24)


def random_call(seed):
    """a random configuration, an output format from the four allowed (every stream decodes to every one of them: none of these calls is one the
    library must refuse), three random rectangles, an output size of up to 48 x 48, a random mirror"""
    case = random_case(seed)
    rng = np.random.default_rng(8000 + seed)
    w, h = case[1], case[2]
    pf = int(rng.choice(ALLOWED))
    rects = []
    for _ in range(3):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        rects.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
    return case, pf, case[4], rects, int(rng.integers(1, 49)), int(rng.integers(1, 49)), [int(v) for v in rng.integers(0, 2, 3)]


def test_random_seeds_reach_every_output_format():
    """(no seed ends in a refusal -- the rectangles lie inside the image, the formats are the allowed ones --, so all of them check pixels)"""
    calls = [random_call(seed) for seed in SEEDS]
    assert {c[1] for c in calls} == set(ALLOWED)
    assert all(x + w <= c[0][1] and y + h <= c[0][2] and w >= 1 and h >= 1 for c in calls for x, y, w, h in c[3])


@pytest.mark.parametrize("seed", SEEDS)
def test_random_configurations(O, G, emu, seed):
    case, pf, cs, rects, ow, oh, mirror = random_call(seed)
    streams = [O.encode(oracle_image(O, case), random_raw(O, case, seed + 100 * f)) for f in range(3)]
    want = expected(O, streams, rects, ow, oh, pf, cs, mirror)
    dec = new_decoder(G, emu, pf, cs)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=mirror)
        assert (pi.width, pi.height, pi.pixel_format) == (ow, oh, pf)
        assert same(got, want), (case, pf, cs, rects, ow, oh, mirror, rep, diffs(got, want))
    dec.close()


# ================================================================================================ 12. GPU only
@pytest.mark.gpu
def test_device_streams_and_device_output(O, G, gpu_lib, hd):
    import torch
    streams, want = hd
    flags = [0, 1, 0, 0, 1, 1]
    want = [w.reshape(OH, OW, 3)[:, ::-1].reshape(-1) if m else w for w, m in zip(want, flags)]
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
        dec.decode_batch_crop_resize(None, HD_RECTS[:5] + [(400, 250, 100, 10)], OW, OH, device_out=d_out.data_ptr(), out_stride=out_stride,
                                     device_in=d_in.data_ptr(), in_stride=in_stride, sizes=sizes)
    torch.cuda.synchronize()
    assert bool(torch.all(d_out == 0xA5))
    for rep in range(2):
        d_out.fill_(0xA5)
        _, pi = dec.decode_batch_crop_resize(None, HD_RECTS, OW, OH, mirror=flags, device_out=d_out.data_ptr(), out_stride=out_stride,
                                             device_in=d_in.data_ptr(), in_stride=in_stride, sizes=sizes)
        torch.cuda.synchronize()
        rows = d_out.cpu().numpy().reshape(n, out_stride)
        assert (pi.width, pi.height) == (OW, OH)
        assert all(np.array_equal(rows[f, :raw], want[f]) for f in range(n)) and np.all(rows[:, raw:] == 0xA5), rep
        assert dec.region_stats()[0] == 1
    assert dec.last_batch() == (n, 0), "the second call has a header to launch on: every frame through the batched launches"
    dec.close()


@pytest.mark.gpu
def test_hd_frames(O, G, gpu_lib):
    """8 x 1920 x 1080, rectangles up to the whole frame -> 224 x 224: the grids for the largest cover and the chunking at a real size"""
    w, h, n, S = 1920, 1080, 8, 224
    base = natural_image(w, h, 3, seed=3).reshape(h, w, 3)
    p, pi = gpu_lib.default_parameters(), gpu_lib.default_image_parameters()
    p.quality, p.restart_interval, p.interleaved, p.verbose = 75, -1, 0, -1
    pi.width, pi.height, pi.pixel_format, pi.color_space = w, h, 1, 1
    enc = G.Encoder(gpu_lib)
    streams = [enc.encode(p, pi, np.ascontiguousarray(np.roll(base, (37 * f, 101 * f), (0, 1))).reshape(-1)) for f in range(n)]
    enc.close()
    rng = np.random.default_rng(16)
    rects = [(0, 0, w, h), (w - 224, h - 224, 224, 224)]
    for _ in range(n - 2):
        rw, rh = int(rng.integers(100, w + 1)), int(rng.integers(100, h + 1))
        rects.append((int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))
    flags = [f & 1 for f in range(n)]
    want = expected(O, streams, rects, S, S, mirror=flags)
    dec = perf_decoder(G, gpu_lib)
    dec.set_batch_chunk(3)
    for rep in range(2):
        got, pi2 = dec.decode_batch_crop_resize(streams, rects, S, S, mirror=flags)
        assert (pi2.width, pi2.height) == (S, S) and same(got, want), (rep, diffs(got, want))
        batched, single = dec.last_batch()
        assert single <= 1 and batched >= n - 1
        assert dec.idct_path() == 5 and dec.region_stats()[0] == 1
    dec.close()
