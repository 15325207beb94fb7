"""Crop-and-resize with a normalised float tensor as its result (gpujpeg_amd_decoder_decode_batch_crop_resize_tensor; gpujpeg_amd_ext.h).

The definition of the tensor is an element-wise function of the bytes the u8 call returns: float32(byte) * float32(scale[c]) + float32(bias[c]) as two
rounded binary32 operations, then the conversion to the element type (round to nearest even), laid out CHW or HWC. tensor_of below restates it in numpy;
the bytes it is applied to are test_crop_resize.expected's, the restatement of the resample over the cropped ORACLE decode (no product code). Every
comparison with the library is between BIT PATTERNS, so -0, infinities and binary16 subnormals count.

Two tiers with the same bodies, like test_crop_resize.py: the CPU tier runs the product's kernels on tests/hipemu (the conversions in their portable
integer form), the -m gpu tier the product library on the MI355X (the hardware's conversions)."""
import ctypes as C

import numpy as np
import pytest

from test_crop_resize import HD_CASE, HD_RECTS, expected, resize_image
from test_region_batch import dlib, emu, frames_of, new_decoder  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import OPT, case_named, case_stream, crop, damaged_restart_markers, opt_value

F32, F16, BF16 = 0, 1, 2
CHW, HWC = 0, 1
ELSIZE = {F32: 4, F16: 2, BF16: 2}
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
FORMATS = [(d, l) for d in (F32, F16, BF16) for l in (CHW, HWC)]
FORMAT_IDS = [f"{'f32 f16 bf16'.split()[d]}_{'chw hwc'.split()[l]}" for d, l in FORMATS]

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMAGENET = ([1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
# (scale, bias) per channel: the ImageNet recipe; binary16 subnormals; binary16 overflow; a tie of binary16 at every odd value up to 2047 / 2^k; a tie of
# bfloat16 likewise; a negative scale with a positive bias, which crosses zero (128 -> +0)
PAIRS = [IMAGENET, ([2.0 ** -20] * 3, [0.0] * 3), ([300.0] * 3, [0.0] * 3), ([1.0 + 2.0 ** -11] * 3, [0.0] * 3), ([1.0 + 2.0 ** -8] * 3, [0.0] * 3),
         ([-1.0 / 128.0] * 3, [1.0] * 3)]
PAIR_IDS = ["imagenet", "f16_subnormals", "f16_overflow", "f16_ties", "bf16_ties", "crosses_zero"]


# ================================================================================================ the definition, in numpy
def tensor_of(u8, dtype, scale, bias):
    """u8: (..., C) bytes -> the bit patterns (uint32 for F32, uint16 for F16 / BF16) of the elements, same shape"""
    ch = u8.shape[-1]
    with np.errstate(over="ignore"):
        f = u8.astype(np.float32) * np.asarray(scale[:ch], np.float32)
        f = f + np.asarray(bias[:ch], np.float32)
        assert f.dtype == np.float32
        if dtype == F32:
            return f.view(np.uint32)
        if dtype == F16:
            return f.astype(np.float16).view(np.uint16)
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def frame_tensor(u8, pf, ow, oh, dtype, layout, scale, bias):
    """one frame of the u8 call (pixel format pf: 0 grey, 1 packed, 2 planar 4:4:4) -> the bit patterns of its tensor, in the tensor's own shape"""
    hwc = u8.reshape(3, oh, ow).transpose(1, 2, 0) if pf == 2 else u8.reshape(oh, ow, -1)
    t = tensor_of(hwc, dtype, scale, bias)
    return np.ascontiguousarray(t if layout == HWC else t.transpose(2, 0, 1))


def bits(a, dtype):
    return np.ascontiguousarray(a).view(BITS[dtype])


def tensors_equal(got, want_u8, pf, ow, oh, dtype, layout, scale, bias):
    """got: the array the wrapper returns; want_u8: one array of bytes per frame -> the number of differing elements per frame"""
    out = []
    for f, u8 in enumerate(want_u8):
        w = frame_tensor(u8, pf, ow, oh, dtype, layout, scale, bias)
        g = bits(got[f], dtype)
        out.append(int(np.count_nonzero(g != w)) if g.shape == w.shape else -1)
    return out


def tensor_raw_call(G, lib, dec, streams, rects, ow, oh, fmt, out, stride, mirror=None, offset=0):
    """the C call with a caller-owned host output buffer (fmt: a TensorFormat or None) -> return code"""
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
    return lib.L.gpujpeg_amd_decoder_decode_batch_crop_resize_tensor(dec.h, buf.ctypes.data, in_stride, csz, n, rc4, mir, ow, oh,
                                                                     None if fmt is None else C.byref(fmt), out.ctypes.data + offset, stride, C.byref(pi))


# ================================================================================================ 1. the restatement against torch on the CPU
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_restatement_against_torch(pair):
    import torch
    scale, bias = pair
    v = np.arange(256, dtype=np.uint8).reshape(256, 1).repeat(3, 1)
    t = torch.from_numpy(v).to(torch.float32) * torch.tensor(scale, dtype=torch.float32)
    t = t + torch.tensor(bias, dtype=torch.float32)
    assert np.array_equal(tensor_of(v, F32, scale, bias), t.numpy().view(np.uint32))
    assert np.array_equal(tensor_of(v, F16, scale, bias), t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(tensor_of(v, BF16, scale, bias), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_pairs_reach_what_they_are_for():
    v = np.arange(256, dtype=np.uint8).reshape(256, 1)
    sub = tensor_of(v, F16, *PAIRS[1])
    assert np.any((sub & 0x7C00) == 0) and np.any((sub & 0x7FFF) != 0) and len(np.unique(sub)) > 100, "no binary16 subnormals"
    assert np.any(tensor_of(v, F16, *PAIRS[2]) == 0x7C00) and not np.any(tensor_of(v, BF16, *PAIRS[2]) == 0x7F80), "no binary16 overflow"
    for dtype, pair, drop in ((F16, PAIRS[3], 13), (BF16, PAIRS[4], 16)):  # ties: the dropped bits of the float are 1000...0 for some values
        f = tensor_of(v, F32, *pair)
        assert np.any((f & ((1 << drop) - 1)) == (1 << (drop - 1))), (dtype, "no ties")
    z = tensor_of(v, F32, *PAIRS[5]).view(np.float32)
    assert np.any(z > 0) and np.any(z < 0) and np.any(z == 0)


# ================================================================================================ 2. the host helper
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_host_helper_equals_the_restatement(G, emu, pair):
    scale, bias = pair
    scale = [scale[0], scale[1] * 0.75, scale[2] * 1.5]  # (another scale per channel: the helper reads its channel's)
    v = np.arange(256, dtype=np.uint8).reshape(256, 1).repeat(3, 1)
    for dtype in (F32, F16, BF16):
        fmt = G.tensor_format(dtype, CHW, scale, bias)
        want = tensor_of(v, dtype, scale, bias)
        got = np.array([[G.tensor_element(emu, fmt, c, i) for c in range(3)] for i in range(256)], dtype=np.uint32)
        assert np.array_equal(got, want.astype(np.uint32)), (dtype, np.argwhere(got != want)[:5])


# ================================================================================================ 3. bytes
OW, OH = 64, 40
MIRROR = [0, 1, 0, 0, 1, 0]


@pytest.fixture(scope="module")
def hd(O):
    """the streams of tests 3, 4, 6, 8 and 10 and the frames the u8 call is defined to return for them, made once"""
    streams = frames_of(O, case_named(HD_CASE), len(HD_RECTS))
    want = expected(O, streams, HD_RECTS, OW, OH, mirror=MIRROR)
    distinct = len(np.unique(np.concatenate(want)))
    assert distinct >= 200, f"the expected frames hold {distinct} distinct byte values: too few to check the conversions"
    return streams, want


@pytest.mark.parametrize("dtype,layout", FORMATS, ids=FORMAT_IDS)
def test_bytes(O, G, dlib, hd, dtype, layout):
    streams, want = hd
    scale, bias = IMAGENET
    dec = new_decoder(G, dlib)
    for rep in range(2):  # (the first call: frame 0 through the single-frame route; the second: every frame through the batched launches)
        got, pi = dec.decode_batch_crop_resize_tensor(streams, HD_RECTS, OW, OH, dtype, layout, scale, bias, mirror=MIRROR)
        assert got.shape == ((6, 3, OH, OW) if layout == CHW else (6, OH, OW, 3)) and got.dtype == {F32: np.float32, F16: np.float16, BF16: np.uint16}[dtype]
        assert (pi.width, pi.height, pi.pixel_format) == (OW, OH, 1)
        d = tensors_equal(got, want, 1, OW, OH, dtype, layout, scale, bias)
        assert d == [0] * 6, (rep, d)
    dec.close()


@pytest.mark.parametrize("pair", PAIRS[1:], ids=PAIR_IDS[1:])
def test_bytes_at_the_edges_of_the_element_types(O, G, dlib, hd, pair):
    """the same frames with the scales of test 1: binary16 subnormals, overflow to infinity, ties of both 16-bit types and the zero crossing come out of
    the KERNEL's conversions (on the GPU tier the hardware's) as the restatement has them"""
    streams, want = hd
    scale, bias = pair
    dec = new_decoder(G, dlib)
    for dtype, layout in ((F16, CHW), (BF16, CHW), (F32, HWC)):
        got, _ = dec.decode_batch_crop_resize_tensor(streams[:3], HD_RECTS[:3], OW, OH, dtype, layout, scale, bias, mirror=MIRROR[:3])
        d = tensors_equal(got, want[:3], 1, OW, OH, dtype, layout, scale, bias)
        assert d == [0] * 3, (dtype, d)
    dec.close()


# ================================================================================================ 4. against the library's own u8 call
@pytest.mark.parametrize("prescale", ["1", "1/8"], ids=["no_prescale", "prescale_8"])
def test_against_the_u8_call(O, G, dlib, hd, prescale):
    streams, _ = hd
    scale, bias = IMAGENET
    if prescale != "1":
        plans = [G.crop_resize_plan(dlib, 480, 272, 1, r, OW, OH, 8) for r in HD_RECTS]
        assert any(p[0] > 1 for p in plans), "no frame takes a prescale: the test shows nothing"
    a, b = new_decoder(G, dlib), new_decoder(G, dlib)
    for dec in (a, b):
        assert dec.set_option("dec_opt_resize_prescale", prescale) == 0
    for rep, (dtype, layout) in enumerate(((F16, CHW), (BF16, HWC), (F32, CHW))):
        u8, pi_u = a.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=MIRROR)
        got, pi_t = b.decode_batch_crop_resize_tensor(streams, HD_RECTS, OW, OH, dtype, layout, scale, bias, mirror=MIRROR)
        d = tensors_equal(got, u8, 1, OW, OH, dtype, layout, scale, bias)
        assert d == [0] * 6, (rep, d)
        assert a.prescales() == b.prescales() and a.last_batch() == b.last_batch() and a.region_stats() == b.region_stats(), rep
        assert a.idct_path() == b.idct_path()
        assert (pi_u.width, pi_u.height, pi_u.pixel_format, pi_u.color_space, pi_u.width_padding) == \
               (pi_t.width, pi_t.height, pi_t.pixel_format, pi_t.color_space, pi_t.width_padding)
        if prescale != "1":
            assert b.prescales() == [p[0] for p in plans]
    a.close()
    b.close()


# ================================================================================================ 5. configurations
# (id, case, output pixel format, colour space, channels)
CONFIGS = [("420_il_to_rgb", "rgb_to_420_il", 1, 1, 3), ("420_il_to_planar444", "rgb_to_420_il", 2, 1, 3), ("420_il_to_ycbcr", "rgb_to_420_il", 1, 3, 3),
           ("gray", "gray", None, None, 1), ("planar444_no_transform", "planar444_in", None, None, 3)]


@pytest.mark.parametrize("ident,name,pf,cs,ch", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_configurations(O, G, dlib, ident, name, pf, cs, ch):
    case = case_named(name)
    w, h = case[1], case[2]
    pf, cs = (case[3], case[4]) if pf is None else (pf, cs)
    ow, oh = 21, 13
    rects = [(1, 3, 37, 29), (w - 45, h - 31, 45, 31), (w // 3 | 1, h // 2 | 1, 9, 5), (0, 0, w, h)]
    streams = frames_of(O, case, 4, seed=40)
    want = expected(O, streams, rects, ow, oh, pf, cs, mirror=[0, 0, 1, 1])
    if ident == "420_il_to_planar444":  # the planar format gives the tensor of the packed one
        packed = expected(O, streams, rects, ow, oh, 1, cs, mirror=[0, 0, 1, 1])
        assert all(np.array_equal(p.reshape(oh, ow, 3), q.reshape(3, oh, ow).transpose(1, 2, 0)) for p, q in zip(packed, want))
    if ident == "420_il_to_ycbcr":  # the colour space is honoured: other bytes than RGB's
        assert not np.array_equal(want[0], expected(O, streams[:1], rects[:1], ow, oh, 1, 1)[0])
    scale, bias = IMAGENET
    dec = new_decoder(G, dlib, pf, cs)
    for rep, (dtype, layout) in enumerate(((F32, CHW), (F16, HWC))):
        got, pi = dec.decode_batch_crop_resize_tensor(streams, rects, ow, oh, dtype, layout, scale, bias, mirror=[0, 0, 1, 1])
        assert got.shape == ((4, ch, oh, ow) if layout == CHW else (4, oh, ow, ch)) and pi.pixel_format == pf
        d = tensors_equal(got, want, pf, ow, oh, dtype, layout, scale, bias)
        assert d == [0] * 4, (rep, d)
        assert dec.last_batch()[1] <= 1
    dec.close()


# ================================================================================================ 6. routes
def test_restart_interval_0_goes_frame_by_frame(O, G, dlib):
    streams = frames_of(O, case_named("rgb_restart0"), 3, seed=60)
    rects = [(0, 0, 100, 60), (60, 35, 40, 25), (33, 17, 11, 30)]
    want = expected(O, streams, rects, 20, 16, mirror=[0, 1, 0])
    dec = new_decoder(G, dlib)
    for rep, (dtype, layout) in enumerate(((F16, CHW), (F32, HWC))):
        got, _ = dec.decode_batch_crop_resize_tensor(streams, rects, 20, 16, dtype, layout, *IMAGENET, mirror=[0, 1, 0])
        assert tensors_equal(got, want, 1, 20, 16, dtype, layout, *IMAGENET) == [0] * 3, rep
        assert dec.last_batch() == (0, 3)
        assert dec.region_stats()[0] == 2
    dec.close()


def test_damaged_restart_markers_in_one_frame(O, G, emu):
    """(CPU tier only) frame 2's restart markers are damaged: it goes through the single-frame route -- its tensor is the restatement over what the
    single region call returns for that stream --, its neighbours stay in the batched launches"""
    streams, rects = frames_of(O, case_named(HD_CASE), 4), HD_RECTS[:4]
    good = expected(O, streams, rects, OW, OH)
    checked = 0
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
                    dec.decode_batch_crop_resize_tensor(mixed, rects, OW, OH, F16, CHW, *IMAGENET)
                continue
            got, _ = dec.decode_batch_crop_resize_tensor(mixed, rects, OW, OH, F16, CHW, *IMAGENET)
            assert tensors_equal(got, good[:2] + [want2] + good[3:], 1, OW, OH, F16, CHW, *IMAGENET) == [0] * 4, (kind, rep)
            batched, single = dec.last_batch()
            assert 1 <= single <= 2 and batched >= 2, (kind, batched, single)
            checked += 1
        dec.close()
    assert checked > 0, "every damaged stream was refused: the single-frame route was not reached"


def test_first_call_chunks_and_host_output(O, G, dlib, hd):
    """the first call of a fresh decoder (frame 0 ahead, through the single-frame kernel), then five frames in chunks of two, with host output"""
    streams, want = hd
    dec = new_decoder(G, dlib)
    got, _ = dec.decode_batch_crop_resize_tensor(streams[:5], HD_RECTS[:5], OW, OH, BF16, CHW, *IMAGENET, mirror=MIRROR[:5])
    assert tensors_equal(got, want[:5], 1, OW, OH, BF16, CHW, *IMAGENET) == [0] * 5
    assert dec.last_batch()[1] >= 1, "the first frame of a decoder's life goes the single-frame way"
    dec.set_batch_chunk(2)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize_tensor(streams[:5], HD_RECTS[:5], OW, OH, F32, HWC, *IMAGENET, mirror=MIRROR[:5])
        assert tensors_equal(got, want[:5], 1, OW, OH, F32, HWC, *IMAGENET) == [0] * 5, rep
        batched, single = dec.last_batch()
        assert batched + single == 5 and single <= 1  # (host output: frame 0 goes ahead)
    dec.close()


@pytest.mark.gpu
def test_device_output(O, G, gpu_lib, hd):
    """device streams and device output through an integer pointer: every frame through the batched launches from the second call on"""
    import torch
    streams, want = hd
    n = len(streams)
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    d_in = torch.from_numpy(host).cuda()
    raw = 3 * OW * OH * 2
    stride = raw + 6
    d_out = torch.full((stride * n,), 0xA5, dtype=torch.uint8, device="cuda")
    dec = new_decoder(G, gpu_lib)
    for rep in range(2):
        d_out.fill_(0xA5)
        dec.decode_batch_crop_resize_tensor(None, HD_RECTS, OW, OH, F16, CHW, *IMAGENET, mirror=MIRROR, out=d_out.data_ptr(), out_stride=stride,
                                            device_in=d_in.data_ptr(), in_stride=in_stride, sizes=sizes)
        torch.cuda.synchronize()
        rows = d_out.cpu().numpy().reshape(n, stride)
        for f in range(n):
            assert np.array_equal(rows[f, :raw].view(np.uint16).reshape(3, OH, OW), frame_tensor(want[f], 1, OW, OH, F16, CHW, *IMAGENET)), (rep, f)
        assert np.all(rows[:, raw:] == 0xA5), rep
    assert dec.last_batch() == (n, 0)
    dec.close()


# ================================================================================================ 7. state
def test_state_between_calls(O, G, dlib, hd):
    """a tensor call, the u8 call, a tensor call of another type and layout, a plain decode: each equals what a fresh decoder gives (the expectation
    from the oracle), so no call sees the tensor state of an earlier one"""
    streams, want = hd
    full = O.decode(streams[3])[0]
    dec = new_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize_tensor(streams, HD_RECTS, OW, OH, F16, CHW, *IMAGENET, mirror=MIRROR)
        assert tensors_equal(got, want, 1, OW, OH, F16, CHW, *IMAGENET) == [0] * 6, rep
        u8, pi = dec.decode_batch_crop_resize(streams, HD_RECTS, OW, OH, mirror=MIRROR)
        assert all(np.array_equal(a, b) for a, b in zip(u8, want)) and dlib.image_size(pi) == OW * OH * 3, rep
        got, _ = dec.decode_batch_crop_resize_tensor(streams, HD_RECTS, OW, OH, F32, HWC, *PAIRS[5], mirror=MIRROR)
        assert tensors_equal(got, want, 1, OW, OH, F32, HWC, *PAIRS[5]) == [0] * 6, rep
        px, pi = dec.decode(streams[3])
        assert (pi.width, pi.height) == (480, 272) and np.array_equal(px, full), rep
        assert dec.set_option(OPT, opt_value((5, 7, 50, 40))) == 0
        px, pi = dec.decode(streams[3])
        assert (pi.width, pi.height) == (50, 40) and np.array_equal(px, crop(full, 480, 272, 1, (5, 7, 50, 40))), rep
        assert dec.set_option(OPT, "full") == 0
    dec.close()


def test_a_stream_of_another_size_fails_the_call(O, G, dlib):
    """a tensor call that fails part-way leaves nothing of itself in the decoder: its own region option holds for the single decode that follows, the
    next tensor call is correct, and a plain decode returns the u8 pixels of the full frame -- no tensor, no resize, no rectangle seen"""
    streams = frames_of(O, case_named(HD_CASE), 3)
    other = case_stream(O, case_named("rgb_natural_auto"))  # 640 x 368: the rectangles below lie inside it as well
    rects = [(0, 0, 64, 40), (8, 8, 30, 50), (16, 16, 100, 20)]
    want = expected(O, streams, rects, 16, 16)
    own, full0 = (5, 7, 50, 40), O.decode(streams[0])[0]
    dec = new_decoder(G, dlib)
    assert dec.set_option(OPT, opt_value(own)) == 0
    for rep in range(2):
        with pytest.raises(RuntimeError):
            dec.decode_batch_crop_resize_tensor([streams[0], other, streams[2]], rects, 16, 16, F16, CHW, *IMAGENET)
        px, pi = dec.decode(streams[0])
        assert (pi.width, pi.height) == (50, 40) and px.dtype == np.uint8 and np.array_equal(px, crop(full0, 480, 272, 1, own)), rep
        got, _ = dec.decode_batch_crop_resize_tensor(streams, rects, 16, 16, F16, CHW, *IMAGENET)  # (and with a header to launch on the second time)
        assert tensors_equal(got, want, 1, 16, 16, F16, CHW, *IMAGENET) == [0] * 3, rep
    assert dec.set_option(OPT, "full") == 0
    px, pi = dec.decode(streams[0])
    assert (pi.width, pi.height) == (480, 272) and px.dtype == np.uint8 and np.array_equal(px, full0) and dec.region_stats()[0] == 0
    dec.close()


# ================================================================================================ 8. guard bytes and stride
@pytest.mark.parametrize("dtype,layout,extra", [(F16, CHW, 22), (BF16, HWC, 2), (F32, CHW, 28), (F32, HWC, 12)], ids=["f16_chw", "bf16_hwc", "f32_chw", "f32_hwc"])
def test_guard_bytes_and_stride(O, G, dlib, dtype, layout, extra):
    """slots larger than a frame, pre-filled: only the first C OW OH elsize bytes of each change; the stride is a multiple of the element size and not of
    16, and the frame (13 x 5 pixels) is no multiple of a wave"""
    streams = frames_of(O, case_named(HD_CASE), 4)
    rects, ow, oh = HD_RECTS[:4], 13, 5
    want = expected(O, streams, rects, ow, oh, mirror=[0, 0, 1, 0])
    raw = ow * oh * 3 * ELSIZE[dtype]
    stride = raw + extra
    assert stride % 16 != 0 and stride % ELSIZE[dtype] == 0
    fmt = G.tensor_format(dtype, layout, *IMAGENET)
    dec = new_decoder(G, dlib)
    for rep in range(2):
        out = np.full(stride * 4 + 64, 0xA5, np.uint8)
        assert tensor_raw_call(G, dlib, dec, streams, rects, ow, oh, fmt, out, stride, mirror=[0, 0, 1, 0]) == 0
        rows = out[:stride * 4].reshape(4, stride)
        for f in range(4):
            assert np.array_equal(rows[f, :raw].view(BITS[dtype]), frame_tensor(want[f], 1, ow, oh, dtype, layout, *IMAGENET).reshape(-1)), (rep, f)
        assert np.all(rows[:, raw:] == 0xA5) and np.all(out[stride * 4:] == 0xA5), rep
    dec.close()


# ================================================================================================ 9. refusals
def test_refusals_write_nothing_and_leave_the_decoder_usable(O, G, dlib, capfd):
    streams = frames_of(O, case_named(HD_CASE), 2)
    ok = HD_RECTS[1:3]  # (two frames and small rectangles: the valid call that follows every refusal stays cheap)
    ow, oh = 32, 24
    want = expected(O, streams, ok, ow, oh)
    good = G.tensor_format(F16, CHW, *IMAGENET)
    raw = ow * oh * 3 * 2
    stride = raw + 32

    def refused(dec, fmt=good, rects=ok, w=ow, h=oh, stride=stride, offset=0, what="", option=False):
        """one refusal: -1, a message, nothing written -- and the next valid call on the same decoder is correct (option: the refusal comes from a
        setting of the decoder, so the valid call follows once the caller has taken the setting back)"""
        out = np.full(stride * 2 + 64, 0xA5, np.uint8)
        capfd.readouterr()
        assert tensor_raw_call(G, dlib, dec, streams, rects, w, h, fmt, out, stride, offset=offset) == -1, what
        err = capfd.readouterr().err
        assert np.all(out == 0xA5), f"a refused call wrote to the output ({what})"
        assert "[Error]" in err, f"a refusal without a message ({what})"
        if not option:
            accepted(dec, what)

    want_bits = [frame_tensor(want[f], 1, ow, oh, F16, CHW, *IMAGENET).reshape(-1) for f in range(2)]

    def accepted(dec, after=""):
        out = np.full(stride * 2, 0xA5, np.uint8)
        assert tensor_raw_call(G, dlib, dec, streams, ok, ow, oh, good, out, stride) == 0, after
        rows = out.reshape(2, stride)
        for f in range(2):
            assert np.array_equal(rows[f, :raw].view(np.uint16), want_bits[f]), (after, f)
        assert np.all(rows[:, raw:] == 0xA5), after

    def fmt_with(dtype=F16, layout=CHW, scale=IMAGENET[0], bias=IMAGENET[1]):
        return G.tensor_format(dtype, layout, scale, bias)

    inf, nan = float("inf"), float("nan")
    for cold in (True, False):
        # cold: every case on a decoder of its own, without a header to launch on -- frame 0 goes ahead through the single-frame route and the refusal
        # is made there or before; warm: all cases on ONE decoder that has a header -- the batched launches are planned first
        state = {"dec": None}

        def nxt():
            if cold or state["dec"] is None:
                if state["dec"] is not None:
                    state["dec"].close()
                state["dec"] = new_decoder(G, dlib)
                if not cold:
                    accepted(state["dec"], "warm-up")
            return state["dec"]

        refused(nxt(), fmt=None, what="format == NULL")
        for dtype, layout in ((3, CHW), (-1, CHW), (F16, 2), (F32, -1)):
            refused(nxt(), fmt=fmt_with(dtype, layout), what=f"dtype {dtype}, layout {layout}")
        for c in range(3):
            for bad in ((nan,) if cold else (inf, -inf, nan)):  # (cold: one value per channel, each on a decoder of its own)
                s, b = list(IMAGENET[0]), list(IMAGENET[1])
                s[c] = bad
                refused(nxt(), fmt=fmt_with(scale=s), what=f"scale[{c}] = {bad}")
                b[c] = bad
                refused(nxt(), fmt=fmt_with(bias=b), what=f"bias[{c}] = {bad}")
        refused(nxt(), offset=1, what="output not aligned to the element size")
        refused(nxt(), stride=stride + 1, what="stride not a multiple of the element size")
        refused(nxt(), fmt=fmt_with(F32), stride=raw * 2 + 2, what="f32: stride a multiple of 2, not of 4")
        refused(nxt(), stride=raw - 2, what="stride smaller than a frame")
        refused(nxt(), fmt=fmt_with(F32), stride=raw, what="f32: stride of an f16 frame")
        # what the u8 call refuses: rectangles, output sizes, a scale, a flip, a channel remap
        refused(nxt(), rects=ok[:1] + [(480, 0, 10, 10)], what="rectangle outside the image")
        refused(nxt(), rects=ok[:1] + [(5, 5, 0, 10)], what="empty rectangle")
        for w, h in ((0, oh), (ow, 0), (16385, oh)):
            refused(nxt(), w=w, h=h, what=f"output {w} x {h}")
        for opt, on, off in (("dec_opt_scale", "1/2", "1"), ("dec_opt_flipped", "1", "0"), ("dec_opt_channel_remap", "210", "")):
            dec = nxt()
            assert dec.set_option(opt, on) == 0
            refused(dec, what=opt, option=True)
            assert dec.set_option(opt, off) == 0
            accepted(dec, opt)
        for align, back in ((2, "1"), (64, "0")):
            dec = nxt()
            assert dec.set_option("dec_opt_alignment_bytes", str(align)) == 0
            refused(dec, what=f"dec_opt_alignment_bytes = {align}", option=True)
            assert dec.set_option("dec_opt_alignment_bytes", back) == 0
            accepted(dec, f"dec_opt_alignment_bytes = {align}")
        # pixel formats: the four-channel one, and those the u8 call refuses
        for pf, cs in ((6, 1), (3, 3), (4, 3), (5, 3)):
            dec = nxt()
            dec.set_output_format(cs, pf)
            refused(dec, what=f"pixel format {pf}", option=True)
            dec.set_output_format(1, 1)
            accepted(dec, f"pixel format {pf}")
        state["dec"].close()
    # a format the STREAM decides: four channels
    s4 = frames_of(O, case_named("rgba_4444"), 2, seed=70)
    dec = new_decoder(G, dlib)
    for rep in range(2):
        out = np.full(8192, 0xA5, np.uint8)
        capfd.readouterr()
        assert tensor_raw_call(G, dlib, dec, s4, [(0, 0, 40, 40), (2, 2, 20, 20)], 16, 16, good, out, 4096) == -1 and np.all(out == 0xA5)
        assert "[Error]" in capfd.readouterr().err
        assert dec.decode(s4[0])[1].pixel_format == 6
    dec.close()
    # a non-finite scale of a channel a single-channel tensor does not have is nobody's
    sg = frames_of(O, case_named("gray"), 2, seed=71)
    rects = [(0, 0, 100, 60), (7, 9, 33, 41)]
    want_g = expected(O, sg, rects, 16, 16)
    dec = new_decoder(G, dlib)
    got, _ = dec.decode_batch_crop_resize_tensor(sg, rects, 16, 16, F32, CHW, [0.5, inf, nan], [-1.0, nan, inf])
    assert tensors_equal(got, want_g, 0, 16, 16, F32, CHW, [0.5], [-1.0]) == [0, 0]
    with pytest.raises(RuntimeError):
        dec.decode_batch_crop_resize_tensor(sg, rects, 16, 16, F32, CHW, [inf, 1.0, 1.0], [0.0] * 3)
    dec.close()


# ================================================================================================ 10. sanity against the float pipeline
def test_f32_is_within_one_rounding_per_operation_of_exact_arithmetic(O, G, dlib, hd):
    """a derived bound: the product is rounded once (relative 2^-24 of |R scale|), the sum once more (2^-24 of the result, itself at most
    |R scale| (1 + 2^-24) + |bias|): together below 2^-23 (|R scale| + |bias|), with scale and bias taken as the binary32 values the call receives"""
    streams, want = hd
    scale, bias = IMAGENET
    dec = new_decoder(G, dlib)
    got, _ = dec.decode_batch_crop_resize_tensor(streams, HD_RECTS, OW, OH, F32, HWC, scale, bias, mirror=MIRROR)
    dec.close()
    s64, b64 = np.asarray(scale, np.float32).astype(np.float64), np.asarray(bias, np.float32).astype(np.float64)
    for f in range(6):
        r = want[f].reshape(OH, OW, 3).astype(np.float64)
        err = np.abs(got[f].astype(np.float64) - (r * s64 + b64))
        bound = 2.0 ** -23 * (np.abs(r * s64) + np.abs(b64))
        print(f"frame {f}: largest error / bound = {float(np.max(err / bound)):.3f}")
        assert np.all(err <= bound), f


# ================================================================================================ 11. GPU only
@pytest.fixture(scope="module")
def hd4(O, gpu_lib, G):
    """four 1920 x 1080 streams, random-resized-crop rectangles to 224 x 224 and the expected bytes, made once"""
    from conftest import natural_image
    w, h, n, S = 1920, 1080, 4, 224
    base = natural_image(w, h, 3, seed=3).reshape(h, w, 3)
    p, pi = gpu_lib.default_parameters(), gpu_lib.default_image_parameters()
    p.quality, p.restart_interval, p.interleaved, p.verbose = 75, -1, 0, -1
    pi.width, pi.height, pi.pixel_format, pi.color_space = w, h, 1, 1
    enc = G.Encoder(gpu_lib)
    streams = [enc.encode(p, pi, np.ascontiguousarray(np.roll(base, (37 * f, 101 * f), (0, 1))).reshape(-1)) for f in range(n)]
    enc.close()
    rng = np.random.default_rng(17)
    rects = []
    for _ in range(n):  # area 8 .. 100 % of the frame, aspect 3/4 .. 4/3, as RandomResizedCrop draws them
        while True:
            area, ratio = rng.uniform(0.08, 1.0) * w * h, np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            rw, rh = int(round(np.sqrt(area * ratio))), int(round(np.sqrt(area / ratio)))
            if 0 < rw <= w and 0 < rh <= h:
                break
        rects.append((int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))
    flags = [0, 1, 0, 1]
    return streams, rects, flags, expected(O, streams, rects, S, S, mirror=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [(F16, CHW), (BF16, HWC)], ids=["f16_chw", "bf16_hwc"])
def test_torch_tensor_out(O, G, gpu_lib, hd4, dtype, layout):
    import torch
    streams, rects, flags, want = hd4
    n, S = len(streams), 224
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    d_in = torch.from_numpy(host).cuda()
    shape = (n, 3, S, S) if layout == CHW else (n, S, S, 3)
    out = torch.empty(shape, dtype=torch.float16 if dtype == F16 else torch.bfloat16, device="cuda")
    dec = new_decoder(G, gpu_lib)
    for rep in range(2):
        out.zero_()
        res, pi = dec.decode_batch_crop_resize_tensor(None, rects, S, S, dtype, layout, *IMAGENET, mirror=flags, out=out, device_in=d_in.data_ptr(),
                                                      in_stride=in_stride, sizes=sizes)
        torch.cuda.synchronize()
        assert res is None and (pi.width, pi.height) == (S, S)
        got = out.cpu().view(torch.int16).numpy().view(np.uint16)
        for f in range(n):
            assert np.array_equal(got[f], frame_tensor(want[f], 1, S, S, dtype, layout, *IMAGENET)), (rep, f)
    assert dec.last_batch() == (n, 0)
    # an out of the wrong element size, a non-contiguous one and one with another frame count never reach the library
    for bad in (torch.empty(shape, dtype=torch.float32, device="cuda"), out.transpose(1, 2), out[:2]):
        with pytest.raises(ValueError):
            dec.decode_batch_crop_resize_tensor(None, rects, S, S, dtype, layout, *IMAGENET, out=bad, device_in=d_in.data_ptr(), in_stride=in_stride, sizes=sizes)
    dec.close()


def test_cpu_torch_tensor_out(O, G, emu, hd):
    """a torch tensor in host memory takes the same way (the wrapper asks it for its pointer, element size and contiguity only)"""
    import torch
    streams, want = hd
    out = torch.zeros((6, OH, OW, 3), dtype=torch.bfloat16)
    dec = new_decoder(G, emu)
    res, _ = dec.decode_batch_crop_resize_tensor(streams, HD_RECTS, OW, OH, BF16, HWC, *IMAGENET, mirror=MIRROR, out=out)
    dec.close()
    got = out.view(torch.int16).numpy().view(np.uint16)
    assert res is None and all(np.array_equal(got[f], frame_tensor(want[f], 1, OW, OH, BF16, HWC, *IMAGENET)) for f in range(6))


# ================================================================================================ 12. ABI
def test_abi(G, emu):
    assert C.sizeof(G.TensorFormat) == 40
    assert G.TensorFormat.scale.offset == 8 and G.TensorFormat.bias.offset == 24
    for name in ("gpujpeg_amd_decoder_decode_batch_crop_resize_tensor", "gpujpeg_amd_host_tensor_element"):
        assert hasattr(emu.L, name), name
    assert (G.TENSOR_F32, G.TENSOR_F16, G.TENSOR_BF16, G.TENSOR_CHW, G.TENSOR_HWC) == (0, 1, 2, 0, 1)


def test_product_library_exports_the_symbols(G, lib):
    for name in ("gpujpeg_amd_decoder_decode_batch_crop_resize_tensor", "gpujpeg_amd_host_tensor_element"):
        assert hasattr(lib.L, name), name
    fmt = G.tensor_format(G.TENSOR_F16, G.TENSOR_CHW, 1.0 + 2.0 ** -11, 0.0)  # (host code of the product library: the tie goes to even)
    assert [G.tensor_element(lib, fmt, 0, v) for v in (0, 1, 3)] == [0x0000, 0x3C00, 0x4201]
