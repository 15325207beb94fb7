"""Crop-and-resize over streams of DIFFERENT image sizes in one batch (dec_opt_batch_sizes = mixed; gpujpeg_amd_ext.h).

Frame f of a "mixed" call is what the same call returns for the one stream f: the definition over the single-frame region call, as ever. Expected
bytes are expected() of test_crop_resize.py -- the numpy restatement over the ORACLE decode of every stream at that stream's own size, no product
code -- and the numpy restatements of the prescale, antialias and tensor tests; every comparison is byte for byte.

The streams of a batch are one FAMILY: one encoder configuration with an explicit restart interval of 2 to 4 MCUs, so that their headers differ in
the four dimension bytes of SOF0 alone. The sizes make every per-frame field of the geometry differ: a single MCU (8 x 8, 16 x 16: one segment, fewer
MCUs than the restart interval), sides that are no multiple of the MCU (67 x 35, 129 x 50), the largest frame (200 x 97) neither first nor last, and
33 x 130, taller than wide, so that the widest and the highest cover -- and the largest segment and sample counts -- come from different frames.

Two tiers with the same bodies, like test_crop_resize.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Damaged streams run on the CPU tier only."""
import numpy as np
import pytest

from conftest import natural_image, oracle_image
from test_crop_resize import diffs, expected, raw_call, region_stats_of
from test_region_batch import dlib, emu, new_decoder, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import damaged_restart_markers, perf_decoder

MIXED = ("dec_opt_batch_sizes", "mixed")
SIZES = [(16, 16), (40, 24), (67, 35), (200, 97), (33, 130), (129, 50), (8, 8)]
OW, OH = 24, 16

# (id, pixel format of the input, colour space, quality, restart interval, interleaved, sampling, internal colour space): one family each
FAMILIES = {
    "444_il": (1, 1, 75, 3, 1, None, 3),
    "420_il": (1, 1, 75, 2, 1, [(2, 2), (1, 1), (1, 1)], 3),
    "444_nonil": (1, 1, 95, 4, 0, None, 3),
    "gray": (0, 3, 75, 3, 0, None, 3),
}
# Three non-interleaved scans: the marker scan's record of a 4 KB part of the stream holds two markers that are no restart markers, so a stream whose
# two SOS markers and EOI fall into one part is walked on the host -- the single-frame route, with or without this option. The frames of this
# family are large enough (quality 95) to stay in the batched launches; its smallest sides are no multiple of the MCU either.
FAMILY_SIZES = {"444_nonil": [(72, 56), (88, 40), (67, 75), (200, 97), (33, 130), (129, 50), (61, 64)]}


def family_case(fam, w, h, **over):
    pf, cs, q, ri, il, ss, csi = FAMILIES[fam]
    q, ri = over.get("q", q), over.get("ri", ri)
    return (f"{fam}_{w}x{h}", w, h, pf, cs, q, ri, il, ss, csi)


def stream_of(O, fam, w, h, seed, **over):
    case = family_case(fam, w, h, **over)
    comps = {0: 1, 1: 3}[case[3]]
    raw = natural_image(w, h, comps, seed=seed) if seed % 2 == 0 and fam not in FAMILY_SIZES else O.noise(O.raw_size(w, h, case[3]), seed=seed)
    return O.encode(oracle_image(O, case), raw)


def rects_of(sizes):
    """per frame, in turn: the whole image, a rectangle that touches the right and bottom edges, one pixel, an inner rectangle"""
    out = []
    for f, (w, h) in enumerate(sizes):
        kind = f % 4
        if kind == 0 or w < 6 or h < 6:
            out.append((0, 0, w, h))
        elif kind == 1:
            out.append((w // 3, h // 4, w - w // 3, h - h // 4))
        elif kind == 2:
            out.append((w - 1, h - 1, 1, 1))
        else:
            out.append((1, 2, w // 2, h // 2))
    return out


_made = {}


def family(O, fam, seed=300):
    """(streams, rectangles, expected frames at OW x OH) of a family at its sizes, made once per session"""
    sizes = FAMILY_SIZES.get(fam, SIZES)
    key = (fam, seed)
    if key not in _made:
        streams = [stream_of(O, fam, w, h, seed + f) for f, (w, h) in enumerate(sizes)]
        rects = rects_of(sizes)
        _made[key] = (streams, rects, expected(O, streams, rects, OW, OH))
    return _made[key]


def mixed_decoder(G, lib, perf=False, pf=None, cs=None):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib, pf, cs)
    assert dec.set_option(*MIXED) == 0
    return dec


def family_headers_differ_in_dimensions_only(streams):
    """the premise of the tests: SOI .. first SOS header of every stream is byte-identical except for four bytes"""
    def header(s):
        b = bytes(s)
        return b[:b.index(b"\xff\xda") + 2 + int.from_bytes(b[b.index(b"\xff\xda") + 2:b.index(b"\xff\xda") + 4], "big")]
    h0 = header(streams[0])
    at = h0.index(b"\xff\xc0") + 5
    return all(len(header(s)) == len(h0) and header(s)[:at] == h0[:at] and header(s)[at + 4:] == h0[at + 4:] for s in streams)


# ================================================================================================ 1. the feature
@pytest.mark.parametrize("order", ["given", "reversed_halves"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_mixed_sizes_in_one_batch(O, G, dlib, fam, order):
    streams, rects, want = family(O, fam)
    assert family_headers_differ_in_dimensions_only(streams)
    idx = list(range(len(streams)))
    if order != "given":  # a second order of the same streams: the same per-frame bytes (the largest frame still neither first nor last)
        idx = idx[2:] + idx[:2]
        assert idx.index(3) not in (0, len(idx) - 1)
    streams, rects, want = [streams[i] for i in idx], [rects[i] for i in idx], [want[i] for i in idx]
    n = len(streams)
    singles = region_stats_of(G, dlib, streams, rects)
    dec = mixed_decoder(G, dlib, perf=True)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert (pi.width, pi.height) == (OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        batched, single = dec.last_batch()
        assert batched + single == n and batched >= n - 1, (batched, single)
        assert dec.idct_path() == 5
        st = dec.region_stats()
        assert st[1:] == tuple(sum(s[i] for s in singles) for i in (1, 2, 3)), (st, singles)
    dec.close()


# ================================================================================================ 2. chunks
@pytest.mark.parametrize("fam", ["444_il", "444_nonil"])
def test_chunks_take_their_maxima_from_different_frames(O, G, dlib, fam):
    streams, rects, want = family(O, fam)
    dec = mixed_decoder(G, dlib)
    dec.set_batch_chunk(3)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


# ================================================================================================ 3. composition
def test_mirror(O, G, dlib):
    streams, rects, want = family(O, "444_il")
    flags = [1, 0, 1, 1, 0, 1, 0]
    mirrored = [w.reshape(OH, OW, 3)[:, ::-1].reshape(-1) if m else w for w, m in zip(want, flags)]
    dec = mixed_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH, mirror=flags)
        assert same(got, mirrored), (rep, diffs(got, mirrored))
    dec.close()


@pytest.mark.parametrize("fam,pf,cs", [("444_il", 1, 1), ("420_il", 2, 3), ("gray", 0, 3), ("444_nonil", 6, 1)], ids=["rgb", "planar444", "u8", "rgbx"])
def test_output_formats(O, G, dlib, fam, pf, cs):
    streams, rects, _ = family(O, fam)
    want = expected(O, streams, rects, OW, OH, pf, cs)
    dec = mixed_decoder(G, dlib, pf=pf, cs=cs)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert pi.pixel_format == pf and same(got, want), (rep, diffs(got, want))
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


PRESCALE_SIZES = [(40, 24), (129, 50), (200, 97), (33, 130), (67, 35), (16, 16)]


def test_prescale_444(O, G, dlib):
    """dec_opt_resize_prescale = 1/8 on 4:4:4: whole-image rectangles to 12 x 8, so that s_f differs between the frames (8 for 200 x 97, 1 for 16 x 16)"""
    import test_crop_resize_prescale as pre
    ow, oh = 12, 8
    streams = [stream_of(O, "444_il", w, h, 340 + f) for f, (w, h) in enumerate(PRESCALE_SIZES)]
    rects = [(0, 0, w, h) for w, h in PRESCALE_SIZES]
    want, plans = pre.expected(O, streams, rects, ow, oh, 8)
    scales = [p[0] for p in plans]
    assert len(set(scales)) >= 3, scales
    dec = mixed_decoder(G, dlib, perf=True)
    assert dec.set_option("dec_opt_resize_prescale", "1/8") == 0
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, want), (rep, diffs(got, want))
        assert list(dec.prescales()) == scales and dec.idct_path() == 6
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


def test_prescale_subsampled_420(O, G, dlib):
    """dec_opt_resize_prescale_subsampled = on on 4:2:0: every frame reduced per component at its own s_f"""
    import test_crop_resize_prescale_subsampled as sub
    ow, oh = 12, 8
    streams = [stream_of(O, "420_il", w, h, 350 + f) for f, (w, h) in enumerate(PRESCALE_SIZES)]
    rects = [(0, 0, w, h) for w, h in PRESCALE_SIZES]
    want, plans = sub.expected(O, streams, rects, ow, oh, 8)
    scales = [p[0] for p in plans]
    assert len(set(scales)) >= 3, scales
    dec = mixed_decoder(G, dlib, perf=True)
    assert dec.set_option("dec_opt_resize_prescale", "1/8") == 0 and dec.set_option("dec_opt_resize_prescale_subsampled", "on") == 0
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, want), (rep, diffs(got, want))
        assert list(dec.prescales()) == scales and dec.idct_path() == 8
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


def test_antialias(O, G, dlib):
    from test_crop_resize_antialias import aa_expected
    streams, rects, _ = family(O, "444_nonil")
    want = aa_expected(O, streams, rects, OW, OH)
    dec = mixed_decoder(G, dlib, perf=True)
    assert dec.set_option("dec_opt_resize_filter", "antialias") == 0
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.idct_path() == 7 and dec.last_batch()[0] >= len(streams) - 1
    dec.close()


def test_tensor_call(O, G, dlib):
    from test_crop_resize_tensor import CHW, F16, F32, HWC, IMAGENET, tensors_equal
    scale, bias = IMAGENET
    streams, rects, want = family(O, "444_il")
    n = len(streams)
    for dtype, layout in ((F16, CHW), (F32, HWC)):
        dec = mixed_decoder(G, dlib)
        for rep in range(2):
            got, pi = dec.decode_batch_crop_resize_tensor(streams, rects, OW, OH, dtype, layout, scale, bias)
            assert got.shape == ((n, 3, OH, OW) if layout == CHW else (n, OH, OW, 3)) and (pi.width, pi.height) == (OW, OH)
            d = tensors_equal(got, want, 1, OW, OH, dtype, layout, scale, bias)
            assert d == [0] * n, (dtype, layout, rep, d)
            assert dec.last_batch()[0] >= n - 1
        dec.close()


# ================================================================================================ 4. outside the family
def with_comment(jpeg, text=b"not of the family\0"):
    """the stream with a COM segment behind SOI"""
    seg = np.frombuffer(b"\xff\xfe" + (len(text) + 2).to_bytes(2, "big") + text, np.uint8)
    return np.concatenate([jpeg[:2], seg, jpeg[2:]])


def test_frames_outside_the_family_go_the_single_frame_route(O, G, dlib):
    """another quality (other DQT), restart interval 0 and an added COM segment in the middle of the batch: the same bytes, and exactly those frames
    (and frame 0, where it goes ahead of the launches: a fresh decoder, pixels to host memory) counted as single"""
    streams, rects, want = family(O, "444_il")
    streams, rects = list(streams), list(rects)
    strangers = {2: stream_of(O, "444_il", *SIZES[2], 402, q=40), 3: stream_of(O, "444_il", *SIZES[3], 403, ri=0), 5: with_comment(streams[5])}
    for f, s in strangers.items():
        streams[f] = s
    want = expected(O, streams, rects, OW, OH)
    n = len(streams)
    dec = mixed_decoder(G, dlib, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        batched, single = dec.last_batch()
        assert batched + single == n and len(strangers) <= single <= len(strangers) + 1, (rep, batched, single)
    dec.close()


# ================================================================================================ 5. refusals
def test_refusals(O, G, dlib, capfd):
    streams, rects, want = family(O, "444_il")
    n, raw = len(streams), OW * OH * 3

    def call(dec, rr):
        out = np.full(raw * n + 64, 0xA5, np.uint8)
        return raw_call(G, dlib, dec, streams, rr, OW, OH, out, raw), out

    # a rectangle inside frame 0's image (16 x 16) but outside frame 6's (8 x 8), and one inside the largest image but outside frame 4's (33 x 130)
    for f, rect in ((6, (4, 4, 10, 10)), (4, (30, 10, 100, 50))):
        bad = list(rects)
        bad[f] = rect
        for fresh in (True, False):
            dec = mixed_decoder(G, dlib)
            if not fresh:
                assert same(dec.decode_batch_crop_resize(streams, rects, OW, OH)[0], want)
            capfd.readouterr()
            rc, out = call(dec, bad)
            assert rc == -1 and np.all(out == 0xA5), (f, fresh)
            assert f"Frame {f} of the batch" in capfd.readouterr().err
            rc, out = call(dec, rects)  # the decoder is usable afterwards
            assert rc == 0 and same([out[i * raw:(i + 1) * raw] for i in range(n)], want) and np.all(out[n * raw:] == 0xA5), (f, fresh)
            dec.close()
    # "same": the batch of different sizes is refused as it is without the option
    for value in (None, "same"):
        dec = new_decoder(G, dlib)
        if value:
            assert dec.set_option("dec_opt_batch_sizes", value) == 0
        for rep in range(2):
            rc, out = call(dec, [(0, 0, 8, 8)] * n)
            assert rc == -1, (value, rep)
        dec.close()
    # a bad value is refused and the setting is kept
    dec = mixed_decoder(G, dlib)
    for value in ("both", "", "Mixed", "1"):
        assert dec.set_option("dec_opt_batch_sizes", value) != 0
    assert same(dec.decode_batch_crop_resize(streams, rects, OW, OH)[0], want)
    assert dec.set_option("dec_opt_batch_sizes", "same") == 0
    assert dec.set_option("dec_opt_batch_sizes", "mixed ") != 0
    with pytest.raises(RuntimeError):
        dec.decode_batch_crop_resize(streams, rects, OW, OH)
    dec.close()


# ================================================================================================ 6. state
def test_state_after_a_mixed_call(O, G, dlib):
    """a "same" call on equal-size streams, a plain decode and a decode_batch after a "mixed" call: the bytes of a fresh decoder (the oracle's)"""
    streams, rects, want = family(O, "444_il")
    w, h = SIZES[2]
    equal = [stream_of(O, "444_il", w, h, 500 + f) for f in range(3)]
    eq_rects = [(0, 0, w, h), (w - 20, h - 11, 20, 11), (3, 5, 31, 17)]
    eq_want = expected(O, equal, eq_rects, OW, OH)
    full = [O.decode(s)[0] for s in equal]
    dec = mixed_decoder(G, dlib)
    for rep in range(2):
        assert dec.set_option(*MIXED) == 0
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.set_option("dec_opt_batch_sizes", "same") == 0
        got, _ = dec.decode_batch_crop_resize(equal, eq_rects, OW, OH)
        assert same(got, eq_want), (rep, diffs(got, eq_want))
        assert dec.set_option(*MIXED) == 0
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        px, pi = dec.decode(streams[3])
        assert (pi.width, pi.height) == SIZES[3] and np.array_equal(px, O.decode(streams[3])[0])
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        got, pi = dec.decode_batch(equal)
        assert (pi.width, pi.height) == (w, h) and same(got, full)
    dec.close()


# ================================================================================================ 7. damaged family frames (CPU tier only)
def rewrite_dimensions(jpeg, w, h):
    bad = jpeg.copy()
    at = bytes(jpeg).index(b"\xff\xc0") + 5
    bad[at:at + 4] = [h >> 8, h & 255, w >> 8, w & 255]
    return bad


def test_damaged_family_frames(O, G, emu):
    """frame 3 (the largest) of the family is damaged -- scan data truncated, restart markers damaged, SOF0's dimensions rewritten to a larger and to a
    smaller image than the data encodes --: the call's outcome for it is the outcome of the call on that stream alone (the same bytes, or both fail),
    the neighbours' slots equal the restatement over the oracle, the bytes behind the output are untouched"""
    streams, rects, want = family(O, "444_il")
    n, raw, f = len(streams), OW * OH * 3, 3
    w, h = SIZES[f]
    cases = [("truncated", streams[f][:streams[f].size * 2 // 3].copy()), ("larger", rewrite_dimensions(streams[f], w + 24, h + 16)),
             ("smaller", rewrite_dimensions(streams[f], w - 40, h - 30))]
    cases += [(kind, bad) for kind, bad, _ in damaged_restart_markers(streams[f])]
    for kind, bad in cases:
        rect = (0, 0, w - 40, h - 30)  # (inside every version of the frame)
        rr = list(rects)
        rr[f] = rect
        good = expected(O, [s for i, s in enumerate(streams) if i != f], [r for i, r in enumerate(rr) if i != f], OW, OH)
        ref = mixed_decoder(G, emu)
        ref.decode_batch_crop_resize(streams[:1], rects[:1], OW, OH)  # (a header to launch on, as the batch call has when it reaches the frame)
        try:
            alone = ref.decode_batch_crop_resize([bad], [rect], OW, OH)[0][0]
        except RuntimeError:
            alone = None
        ref.close()
        batch = streams[:f] + [bad] + streams[f + 1:]
        dec = mixed_decoder(G, emu)
        for rep in range(2):
            out = np.full(raw * n + 256, 0xA5, np.uint8)
            rc = raw_call(G, emu, dec, batch, rr, OW, OH, out, raw)
            assert np.all(out[raw * n:] == 0xA5), (kind, rep)
            assert (rc == 0) == (alone is not None), (kind, rep, rc)
            if rc != 0:
                continue
            got = [out[i * raw:(i + 1) * raw] for i in range(n)]
            assert same(got[:f] + got[f + 1:], good), (kind, rep, diffs(got[:f] + got[f + 1:], good))
            assert np.array_equal(got[f], alone), (kind, rep)
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)  # the decoder decodes the intact streams as ever
        assert same(got, want), kind
        dec.close()


# ================================================================================================ 8. GPU only: device-resident streams
@pytest.mark.gpu
def test_device_streams_and_device_output(O, G, gpu_lib):
    """streams and pixels in device memory: the headers come to the host by the gather launch, every frame goes through the batched launches from the
    second call on, the bytes between the slots are untouched"""
    import torch
    streams, rects, want = family(O, "420_il")
    n, raw = len(streams), OW * OH * 3
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    d_in = torch.from_numpy(host).cuda()
    out_stride = raw + 61
    d_out = torch.full((out_stride * n,), 0xA5, dtype=torch.uint8, device="cuda")
    dec = mixed_decoder(G, gpu_lib, perf=True)
    for chunk in (0, 3):
        dec.set_batch_chunk(chunk)
        for rep in range(2):
            d_out.fill_(0xA5)
            _, pi = dec.decode_batch_crop_resize(None, rects, OW, OH, device_out=d_out.data_ptr(), out_stride=out_stride, device_in=d_in.data_ptr(),
                                                 in_stride=in_stride, sizes=sizes)
            torch.cuda.synchronize()
            rows = d_out.cpu().numpy().reshape(n, out_stride)
            assert (pi.width, pi.height) == (OW, OH)
            assert all(np.array_equal(rows[f, :raw], want[f]) for f in range(n)), (chunk, rep, [int(np.count_nonzero(rows[f, :raw] != want[f])) for f in range(n)])
            assert np.all(rows[:, raw:] == 0xA5), (chunk, rep)
    assert dec.last_batch() == (n, 0), "a header to launch on: every frame through the batched launches"
    dec.close()
