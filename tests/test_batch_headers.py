"""Crop-and-resize over streams with DIFFERENT HEADERS in one family (dec_opt_batch_headers = any next to dec_opt_batch_sizes = mixed; gpujpeg_amd_ext.h).

The definition does not change: frame f is what the same call returns for the one stream f. Expected bytes never come from the product: expected() of
test_crop_resize.py over the ORACLE decode of every stream, and the numpy restatements of the prescale, subsampled-prescale, antialias and tensor
tests; every comparison is byte for byte.

The streams are oracle-encoded streams of test_crop_resize_mixed.py's families at its sizes (8 x 8 to 200 x 97, the single MCU and 33 x 130 included),
changed per frame: another quality (other DQT), written again by synth_streams.recode() with tables of their own, other slots, other DHT segments,
and with COM / APP1 segments behind SOI. What the tests rely on is asserted from the bytes: the headers differ, the first scan bytes take many
residues mod 16, the distinct table contents are counted by a restatement of the rule (table_key).

Two tiers with the same bodies, like test_crop_resize_mixed.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Damaged streams run on the CPU tier only."""
import numpy as np
import pytest

import synth_streams as S
from test_crop_resize import diffs, expected, raw_call, region_stats_of
from test_crop_resize_mixed import FAMILIES, FAMILY_SIZES, MIXED, OH, OW, SIZES, family, rects_of, stream_of, with_comment
from test_huffman_optimal import optimal_table, segments_of, subtables
from test_region_batch import dlib, emu, new_decoder, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import perf_decoder

OPT = "dec_opt_batch_headers"
ANY = (OPT, "any")
HDR_WINDOW = 65536   # GJ_HDR_WINDOW: the longest header a family frame may have
GATHER = 4096        # GJ_HDR_GATHER: the first window of every device-resident stream
QUALITIES = [35, 50, 75, 90, 95, 100, 75]
QUALITIES_NONIL = [90, 95, 100, 92, 97, 95, 100]  # (three scans: SOS / SOS / EOI stay out of one 4 KB part, FAMILY_SIZES of test_crop_resize_mixed.py)
# (the last comment puts that frame's first scan byte into a LATER 4 KB part of the marker scan than the others': the parts are cut from the smallest
# first scan byte of the call, ~0.6 KB, so 700 bytes would stay in part 0 -- 4300 do not; test 1 asserts the part index from the bytes)
COMMENTS = [0, 1, 5, 14, 15, 16, 4300]


# ================================================================================================ helpers
def any_decoder(G, lib, perf=False, pf=None, cs=None, more=()):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib, pf, cs)
    for k, v in (MIXED, ANY) + tuple(more):
        assert dec.set_option(k, v) == 0
    return dec


def mixed_decoder(G, lib, perf=False, pf=None, cs=None, more=()):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib, pf, cs)
    for k, v in (MIXED,) + tuple(more):
        assert dec.set_option(k, v) == 0
    return dec


def with_segment(jpeg, marker, payload):
    """the stream with one more marker segment behind SOI"""
    seg = np.frombuffer(bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload), np.uint8)
    return np.concatenate([jpeg[:2], seg, jpeg[2:]])


def scan_begin(jpeg):
    """the first byte behind the first SOS header"""
    at = 2
    b = bytes(jpeg)
    while True:
        assert b[at] == 0xFF
        n = int.from_bytes(b[at + 2:at + 4], "big")
        if b[at + 1] == 0xDA:
            return at + 2 + n
        at += 2 + n


def header_of(jpeg):
    return bytes(jpeg)[:scan_begin(jpeg)]


def table_key(jpeg):
    """what a table set is deduplicated by, restated: the contents of the tables the components reference, numbered in the order of their first use"""
    q, h, comps, sel = {}, {}, [], {}
    for m, pl, _ in segments_of(jpeg):
        if m == 0xDB:
            for o in range(0, len(pl), 65):
                q[pl[o] & 15] = bytes(pl[o + 1:o + 65])
        elif m == 0xC4:
            p = 0
            while p < len(pl):
                n = sum(pl[p + 1:p + 17])
                h[(pl[p] >> 4, pl[p] & 15)] = bytes(pl[p + 1:p + 17 + n])
                p += 17 + n
        elif m == 0xC0:
            comps = [(pl[6 + 3 * k], pl[8 + 3 * k]) for k in range(pl[5])]
        elif m == 0xDA:
            for k in range(pl[0]):
                sel[pl[1 + 2 * k]] = (pl[2 + 2 * k] >> 4, pl[2 + 2 * k] & 15)
    qs, dcs, acs = [], [], []
    for cid, tq in comps:
        for lst, slot in ((qs, tq), (dcs, sel[cid][0]), (acs, sel[cid][1])):
            if slot not in lst:
                lst.append(slot)
    return (tuple(q[s] for s in qs), tuple(h[(0, s)] for s in dcs), tuple(h[(1, s)] for s in acs))


def varied(O, fam, seed=900):
    """(streams, rectangles, sizes) of the family at its sizes, every frame with a header of its own: quality, tables, slots, DHT segments, comment"""
    sizes = FAMILY_SIZES.get(fam, SIZES)
    qualities = QUALITIES_NONIL if fam in FAMILY_SIZES else QUALITIES
    ncomp = 1 if fam == "gray" else 3
    streams = []
    for f, (w, h) in enumerate(sizes):
        s = stream_of(O, fam, w, h, seed + f, q=qualities[f])
        if f == 1:      # tables of its own (the optimal ones of its symbols)
            s = S.recode(s, tables=S.fitted)
        elif f == 2:    # every component on slot 0
            s = S.recode(s, tables=S.fitted, table_map=[(0, 0)] * ncomp)
        elif f == 3:    # the tables of slot 0 in slot 1 and the other way round
            s = S.recode(s, tables=S.fitted, slots={0: 1, 1: 0})
        elif f == 4:    # the same tables in the other DHT layout: one segment instead of one per table, or the other way round
            s = S.recode(s, dht_layout="single" if S.dht_tables(s)[1] > 1 else "separate")
        elif f == 5:
            s = S.recode(s, tables=S.unrestricted if fam == "gray" else S.fitted, dht_layout="single")
        if COMMENTS[f]:
            s = with_comment(s, b"c" * (COMMENTS[f] - 1) + b"\0")
        streams.append(s)
    return streams, rects_of(sizes), sizes


_made = {}


def varied_family(O, fam):
    if fam not in _made:
        streams, rects, sizes = varied(O, fam)
        _made[fam] = (streams, rects, expected(O, streams, rects, OW, OH))
    return _made[fam]


def thumbnail(O):
    """a complete small JPEG for an APP1 payload: SOI, DQT, SOF0, DHT, SOS, entropy bytes with FF 00 and FF D0 .. FF D7, EOI"""
    t = bytes(stream_of(O, "444_il", 24, 24, 77, q=95, ri=1))
    assert t[:2] == b"\xff\xd8" and t[-2:] == b"\xff\xd9" and b"\xff\x00" in t and all(bytes([0xFF, 0xD0 + k]) in t for k in range(8))
    assert all(m in t for m in (b"\xff\xdb", b"\xff\xc0", b"\xff\xc4", b"\xff\xda"))
    return t


# ================================================================================================ 1. the feature
@pytest.mark.parametrize("order", ["given", "reversed_halves"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_different_headers_in_one_family(O, G, dlib, fam, order):
    streams, rects, want = varied_family(O, fam)
    equal, eq_rects, eq_want = family(O, fam)  # (the byte-equal family of the same sizes: what the counts are compared with)
    n = len(streams)
    headers = [header_of(s) for s in streams]
    assert len(set(headers)) == n and len({len(x) for x in headers}) >= 6
    assert len({scan_begin(s) % 16 for s in streams}) >= 5, [scan_begin(s) % 16 for s in streams]
    part0 = min(scan_begin(s) for s in streams) & ~15
    parts = [(scan_begin(s) - part0) // 4096 for s in streams]
    assert parts[:6] == [0] * 6 and parts[6] >= 1, parts  # (one begin in a later 4 KB part than the others)
    assert len({table_key(s) for s in streams}) >= 5
    assert S.dht_tables(streams[4])[1] != S.dht_tables(streams[0])[1]
    if fam == "444_nonil":  # (SOS / SOS / EOI of a frame not inside one 4 KB part of the marker scan, cut from the smallest first scan byte)
        a0 = min(scan_begin(s) for s in streams) & ~15
        for s in streams:
            b = bytes(s)
            marks = [b.rindex(b"\xff\xda", 0, b.rindex(b"\xff\xda")), b.rindex(b"\xff\xda"), len(b) - 2]
            assert len({(m - a0) // 4096 for m in marks}) > 1, marks
    idx = list(range(n))
    if order != "given":
        idx = idx[2:] + idx[:2]
    streams, rects, want = [streams[i] for i in idx], [rects[i] for i in idx], [want[i] for i in idx]
    equal, eq_rects = [equal[i] for i in idx], [eq_rects[i] for i in idx]
    singles = region_stats_of(G, dlib, streams, rects)
    ref = mixed_decoder(G, dlib, perf=True)
    dec = any_decoder(G, dlib, perf=True)  # (on the parent commit: set_option fails here)
    for rep in range(2):
        ref.decode_batch_crop_resize(equal, eq_rects, OW, OH)
        got, pi = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert (pi.width, pi.height) == (OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch() == ref.last_batch(), (rep, dec.last_batch(), ref.last_batch())
        batched, single = dec.last_batch()
        assert batched + single == n and batched >= n - 1
        assert dec.idct_path() == 5
        st = dec.region_stats()
        assert st[1:] == tuple(sum(s[i] for s in singles) for i in (1, 2, 3)), (st, singles)
        assert dec.batch_header_stats() == (0, batched, len({table_key(s) for s in streams}), 0, 0), (rep, dec.batch_header_stats())
    ref.close()
    dec.close()


# ================================================================================================ 2. header bytes that look like scan data
def test_header_bytes_that_look_like_scan_data(O, G, dlib):
    """APP1 segments whose payload is a complete JPEG -- inside the first 4 KB part of the marker scan, across a part boundary, 20 KB long, and in a
    header beyond 64 KB -- among plain frames, so that the launch begins early and these frames' own scans late"""
    plain, rects, _ = family(O, "444_il")
    thumb = thumbnail(O)
    streams = list(plain)
    begin0 = min(scan_begin(s) for s in plain)
    a0 = begin0 & ~15
    streams[1] = with_segment(plain[1], 0xE1, thumb)                                     # inside the first part
    assert scan_begin(streams[1]) < a0 + 4096
    pad = a0 + 4096 - 4 - len(thumb) // 2 - 8                                            # the thumbnail's middle on the part boundary
    streams[2] = with_comment(with_segment(plain[2], 0xE1, thumb), b"p" * (pad - 5) + b"\0")
    at = bytes(streams[2]).index(thumb)
    assert at < a0 + 4096 < at + len(thumb)
    streams[4] = with_segment(plain[4], 0xE1, (thumb * 40)[:20000])                      # a 20 KB segment
    assert GATHER < scan_begin(streams[4]) < HDR_WINDOW
    streams[5] = with_segment(with_segment(plain[5], 0xE1, (thumb * 90)[:40000]), 0xE2, (thumb * 90)[:40000])  # a header beyond the window
    assert scan_begin(streams[5]) > HDR_WINDOW
    want = expected(O, streams, rects, OW, OH)
    n = len(streams)
    singles = region_stats_of(G, dlib, streams, rects)
    dec = any_decoder(G, dlib, perf=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch() == (n - 2, 2), (rep, dec.last_batch())  # (frame 0 ahead -- pixels to host memory -- and the long header)
        st = dec.region_stats()
        assert st[1:] == tuple(sum(s[i] for s in singles) for i in (1, 2, 3)), (st, singles)
        assert dec.batch_header_stats() == (0, n - 2, 1, 0, 0), rep
    dec.close()


# ================================================================================================ 3. one table set per distinct content
def test_table_sets_are_deduplicated_by_content(O, G, dlib):
    sizes = SIZES[1:7]
    rects = rects_of(sizes)
    contents = [dict(q=75), dict(q=50), dict(q=75), dict(q=90), dict(q=50), dict(q=90)]
    streams = [with_comment(stream_of(O, "444_il", w, h, 930 + f, **contents[f]), b"n" * f + b"\0") for f, (w, h) in enumerate(sizes)]
    assert len({header_of(s) for s in streams}) == 6 and len({table_key(s) for s in streams}) == 3
    want = expected(O, streams, rects, OW, OH)
    dec = any_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.batch_header_stats()[:3] == (0, 5, 3), dec.batch_header_stats()
    one = [with_comment(stream_of(O, "444_il", w, h, 940 + f), b"m" * (3 * f) + b"\0") for f, (w, h) in enumerate(sizes)]
    assert len({header_of(s) for s in one}) == 6 and len({table_key(s) for s in one}) == 1
    got, _ = dec.decode_batch_crop_resize(one, rects, OW, OH)
    assert same(got, expected(O, one, rects, OW, OH))
    assert dec.batch_header_stats()[:3] == (0, 5, 1), dec.batch_header_stats()
    dec.close()


# ================================================================================================ 4. chunks
@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("fam", ["444_il", "444_nonil"])
def test_chunks_index_the_records_by_frame(O, G, dlib, fam, chunk):
    streams, rects, want = varied_family(O, fam)
    begins = [scan_begin(s) for s in streams]
    sizes = FAMILY_SIZES.get(fam, SIZES)
    assert len({begins.index(min(begins)), begins.index(max(begins)), max(range(7), key=lambda f: sizes[f][0] * sizes[f][1])}) == 3
    dec = any_decoder(G, dlib)
    dec.set_batch_chunk(chunk)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


# ================================================================================================ 5. all three IDCT kernels read the frame's tables
PRESCALE_SIZES = [(40, 24), (129, 50), (200, 97), (33, 130), (67, 35), (16, 16)]
PRESCALE_Q = [35, 90, 50, 100, 75, 95]


def prescale_streams(O, fam, seed):
    out = []
    for f, (w, h) in enumerate(PRESCALE_SIZES):
        s = stream_of(O, fam, w, h, seed + f, q=PRESCALE_Q[f])
        out.append(with_comment(S.recode(s, tables=S.fitted) if f % 2 else s, b"k" * (f * 3) + b"\0"))
    assert len({table_key(s) for s in out}) == len(out)
    return out, [(0, 0, w, h) for w, h in PRESCALE_SIZES]


def test_idct_region_reads_the_frames_float_tables(O, G, dlib):
    streams, rects, want = varied_family(O, "420_il")  # (s_f = 1: k_idct_region_batch)
    dec = any_decoder(G, dlib, perf=True)
    got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
    assert same(got, want) and dec.idct_path() == 5 and list(dec.prescales()) == [1] * len(streams)
    dec.close()


def test_idct_region_scaled_reads_the_frames_uint16_tables(O, G, dlib):
    import test_crop_resize_prescale as pre
    ow, oh = 12, 8
    streams, rects = prescale_streams(O, "444_il", 950)
    want, plans = pre.expected(O, streams, rects, ow, oh, 8)
    scales = [p[0] for p in plans]
    assert len(set(scales)) >= 3, scales
    dec = any_decoder(G, dlib, perf=True, more=(("dec_opt_resize_prescale", "1/8"),))
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, want), (rep, diffs(got, want))
        assert list(dec.prescales()) == scales and dec.idct_path() == 6
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


def test_idct_region_scaled_comp_reads_both_tables(O, G, dlib):
    import test_crop_resize_prescale_subsampled as sub
    ow, oh = 12, 8
    streams, rects = prescale_streams(O, "420_il", 960)
    want, plans = sub.expected(O, streams, rects, ow, oh, 8)
    scales = [p[0] for p in plans]
    assert len(set(scales)) >= 3, scales
    dec = any_decoder(G, dlib, perf=True, more=(("dec_opt_resize_prescale", "1/8"), ("dec_opt_resize_prescale_subsampled", "on")))
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, want), (rep, diffs(got, want))
        assert list(dec.prescales()) == scales and dec.idct_path() == 8
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


# ================================================================================================ 6. composition
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_restartless_streams_of_different_quality_and_tables(O, G, dlib, fam):
    """dec_opt_batch_restartless = on: the stage / pieces / blocks kinds of test_batch_restartless.py at its shapes, every frame at its own quality, two
    with tables of their own"""
    import test_batch_restartless as R
    small, large, _, tall = R.SHAPES[fam]
    sizes = [small, large, large, tall]
    base, _ = R.mixed_set(O, fam)
    kinds = [R.kind_of(fam, s, w, h) for s, (w, h) in zip(base, sizes)]
    assert kinds[:3] == ["stage", "pieces", "blocks"]
    streams = [with_comment(base[0], b"a\0"), S.recode(base[1], dht_layout="single" if S.dht_tables(base[1])[1] > 1 else "separate"),
               with_comment(S.recode(base[2], tables=S.fitted), b"bcd\0"),
               S.recode(R.stream_of(O, fam, *tall, "natural", 731, q=92 if fam == "444_nonil" else 60), tables=S.fitted)]
    assert [R.kind_of(fam, s, w, h) for s, (w, h) in zip(streams[:2], sizes[:2])] == kinds[:2]
    assert len({header_of(s) for s in streams}) == 4 and len({table_key(s) for s in streams}) >= 3
    rects = R.rects_of(sizes)
    want = expected(O, streams, rects, OW, OH)
    n = len(streams)
    dec = any_decoder(G, dlib, more=((R.OPT, "on"),))
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch() == (n - 1, 1), (rep, dec.last_batch())
        rc, handed, read = dec.entropy_bytes()
        assert rc == 0 and handed == sum(b for s in streams[1:] for _, b in R.scans_of(s)) and 0 < read <= handed, (rep, handed, read)
    dec.close()


def test_antialias(O, G, dlib):
    from test_crop_resize_antialias import aa_expected
    streams, rects, _ = varied_family(O, "444_nonil")
    want = aa_expected(O, streams, rects, OW, OH)
    dec = any_decoder(G, dlib, perf=True, more=(("dec_opt_resize_filter", "antialias"),))
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.idct_path() == 7 and dec.last_batch()[0] >= len(streams) - 1
    dec.close()


def test_mirror(O, G, dlib):
    streams, rects, want = varied_family(O, "444_il")
    flags = [1, 0, 1, 1, 0, 1, 0]
    mirrored = [w.reshape(OH, OW, 3)[:, ::-1].reshape(-1) if m else w for w, m in zip(want, flags)]
    dec = any_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH, mirror=flags)
        assert same(got, mirrored), (rep, diffs(got, mirrored))
    dec.close()


@pytest.mark.parametrize("fam,pf,cs", [("444_il", 1, 1), ("420_il", 2, 3), ("gray", 0, 3), ("444_nonil", 6, 1)], ids=["rgb", "planar444", "u8", "rgbx"])
def test_output_formats(O, G, dlib, fam, pf, cs):
    streams, rects, _ = varied_family(O, fam)
    want = expected(O, streams, rects, OW, OH, pf, cs)
    dec = any_decoder(G, dlib, pf=pf, cs=cs)
    for rep in range(2):
        got, pi = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert pi.pixel_format == pf and same(got, want), (rep, diffs(got, want))
        assert dec.last_batch()[0] >= len(streams) - 1
    dec.close()


def test_tensor_call(O, G, dlib):
    from test_crop_resize_tensor import CHW, F16, F32, HWC, IMAGENET, tensors_equal
    scale, bias = IMAGENET
    streams, rects, want = varied_family(O, "444_il")
    n = len(streams)
    for dtype, layout in ((F16, CHW), (F32, HWC)):
        dec = any_decoder(G, dlib)
        for rep in range(2):
            got, pi = dec.decode_batch_crop_resize_tensor(streams, rects, OW, OH, dtype, layout, scale, bias)
            assert got.shape == ((n, 3, OH, OW) if layout == CHW else (n, OH, OW, 3)) and (pi.width, pi.height) == (OW, OH)
            d = tensors_equal(got, want, 1, OW, OH, dtype, layout, scale, bias)
            assert d == [0] * n, (dtype, layout, rep, d)
            assert dec.last_batch()[0] >= n - 1
        dec.close()


def test_a_folder_as_it_lies_on_disk(O, G, dlib):
    """files written by PIL (libjpeg): 4:2:0, no restart markers, different sizes and qualities, optimize=True, an Exif blob -- in one call"""
    Image = pytest.importorskip("PIL.Image")
    import io
    import test_batch_restartless as R
    rng = np.random.default_rng(5)
    spec = [((64, 48), dict(quality=75)), ((97, 61), dict(quality=90, optimize=True)), ((40, 72), dict(quality=60)),
            ((120, 80), dict(quality=85, optimize=True, exif=b"Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0")), ((33, 33), dict(quality=95)), ((80, 56), dict(quality=75, comment=b"a folder"))]
    streams = []
    for (w, h), kw in spec:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([xx * 255 // w, yy * 255 // h, (xx + yy) % 256], -1) + rng.integers(-20, 21, (h, w, 3))
        buf = io.BytesIO()
        Image.fromarray(img.clip(0, 255).astype(np.uint8), "RGB").save(buf, "JPEG", subsampling="4:2:0", **kw)
        streams.append(np.frombuffer(buf.getvalue(), np.uint8))
    assert len({header_of(s) for s in streams}) == len(streams) and all(b"\xff\xdd" not in header_of(s) for s in streams)
    sizes = [s for s, _ in spec]
    rects = rects_of(sizes)
    want = expected(O, streams, rects, OW, OH)
    dec = any_decoder(G, dlib, more=((R.OPT, "on"),))
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch() == (len(streams) - 1, 1), (rep, dec.last_batch())
        assert dec.batch_header_stats()[2] == len({table_key(s) for s in streams})
    dec.close()


# ================================================================================================ 7. routing
def unfitting_ac(cls, tid, freq):
    """tables for recode(): the AC tables with five dominant and 150 equally rare symbols (test_host_tables_fit_rule_picks_10) -- too deep for the
    two-level layout --, the DC tables optimal"""
    if cls == 0:
        return optimal_table(freq)[:2]
    f = np.zeros(256, np.int64)
    f[[0x00, 0x01, 0x02, 0x11, 0x03]] = 1_000_000
    f[[s for s in range(256) if s not in (0x00, 0x01, 0x02, 0x11, 0x03)][:150]] = 1
    f[(np.asarray(freq) > 0) & (f == 0)] = 1
    bits, vals = optimal_table(f, 16)[:2]
    assert subtables(bits) > 6
    return bits, vals


def test_routing(O, G, dlib, capfd):
    import progressive_streams as P
    plain, rects, _ = family(O, "444_il")
    rects = list(rects)

    def strangers():
        out = {1: stream_of(O, "gray", *SIZES[1], 971), 3: stream_of(O, "444_il", *SIZES[3], 973, ri=5),
               4: S.recode(plain[4], slots={1: 2}), 5: S.recode(plain[5], tables=unfitting_ac)}
        pf, cs, q, ri, il, ss, csi = FAMILIES["444_il"]
        w, h = SIZES[2]
        case = ("422", w, h, pf, cs, q, ri, il, [(2, 1), (1, 1), (1, 1)], csi)
        from conftest import oracle_image
        out[2] = O.encode(oracle_image(O, case), O.noise(O.raw_size(w, h, pf), seed=972))
        return out

    streams = list(plain)
    for f, s in strangers().items():
        streams[f] = s
    assert any(t[1] == 2 for t in S.dht_tables(streams[4])[0])
    # two more family frames with headers of their own (another quality and a comment; tables of its own), so that a heterogeneous family shares
    # the launches with the strangers' slots
    streams[6] = with_comment(stream_of(O, "444_il", *SIZES[6], 976, q=50), b"family\0")
    streams += [S.recode(stream_of(O, "444_il", *SIZES[2], 977, q=90), tables=S.fitted), with_comment(stream_of(O, "444_il", *SIZES[1], 978, q=35), b"xy\0")]
    rects += [rects[2], rects[1]]
    assert len({table_key(s) for s in streams[6:]}) == 3 and len({header_of(s) for s in [streams[0]] + streams[6:]}) == 4
    n = len(streams)
    want = expected(O, streams, rects, OW, OH, 0, 3)  # (single-channel output asked for: the grey stream decodes to the size of the others' slots)
    dec = any_decoder(G, dlib, pf=0, cs=3)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        assert dec.last_batch() == (3, n - 3), (rep, dec.last_batch())  # (frames 6, 7, 8: frame 0 goes ahead, five strangers)
        assert dec.batch_header_stats()[:3] == (0, 3, 4), dec.batch_header_stats()  # (frame 0's set is built too: every header is looked at)
    # a progressive stream, with and without the two progressive options
    from test_progressive_batch import BH, BW, progressive
    prog, twin = progressive(4, P.LIBJPEG_COLOUR)[:2]  # (a 4:2:0 frame; the oracle decodes its baseline twin)
    streams2, rects2 = list(plain), list(rects[:len(plain)])
    streams2[3], rects2[3] = prog, (3, 2, BW - 7, BH - 5)
    want2 = expected(O, streams2[:3] + [twin] + streams2[4:], rects2, OW, OH)
    for options in ((), (("dec_opt_progressive", "on"),), (("dec_opt_progressive", "on"), ("dec_opt_batch_progressive", "on"))):
        d2 = any_decoder(G, dlib, more=options)
        for rep in range(2):
            if not options:  # (the reader refuses SOF2: the call fails as ever)
                with pytest.raises(RuntimeError):
                    d2.decode_batch_crop_resize(streams2, rects2, OW, OH)
            else:
                got, _ = d2.decode_batch_crop_resize(streams2, rects2, OW, OH)
                assert same(got, want2), (options, rep, diffs(got, want2))
                assert d2.last_batch() == (len(streams2) - 2, 2), (options, rep, d2.last_batch())
        d2.close()
    # a refused rectangle names its frame and writes nothing
    raw = OW * OH
    bad = list(rects)
    bad[4] = (30, 10, 100, 50)  # (outside frame 4's 33 x 130 image)
    for fresh in (True, False):
        d3 = any_decoder(G, dlib, pf=0, cs=3)
        if not fresh:
            d3.decode_batch_crop_resize(streams, rects, OW, OH)
        capfd.readouterr()
        out = np.full(raw * n + 64, 0xA5, np.uint8)
        assert raw_call(G, dlib, d3, streams, bad, OW, OH, out, raw) == -1 and np.all(out == 0xA5), fresh
        assert "Frame 4 of the batch" in capfd.readouterr().err
        d3.close()
    dec.close()


# ================================================================================================ 8. the option
def test_option_semantics(O, G, dlib, capfd):
    streams, rects, want = varied_family(O, "444_il")
    equal, eq_rects, eq_want = family(O, "444_il")
    n = len(streams)
    assert G.DEC_OPT_BATCH_HEADERS == OPT and (G.BATCH_HEADERS_SAME, G.BATCH_HEADERS_ANY) == ("same", "any")
    # bad values are refused and leave the setting as it was
    dec = any_decoder(G, dlib)
    for value in ("both", "", "Any", "1", "any "):
        assert dec.set_option(OPT, value) != 0
    assert "Unknown value both for dec_opt_batch_headers" in capfd.readouterr().err
    got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
    assert same(got, want) and dec.last_batch() == (n - 1, 1) and dec.batch_header_stats()[0] == 0
    # "same" after "any": the routing of a mixed call -- the heterogeneous set goes frame by frame
    ref = mixed_decoder(G, dlib)
    ref.decode_batch_crop_resize(streams, rects, OW, OH)
    assert dec.set_option(OPT, "same") == 0
    for rep in range(2):
        a, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        b, _ = ref.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(a, want) and same(b, want)
        assert dec.last_batch() == ref.last_batch() and dec.last_batch()[0] <= 1, (dec.last_batch(), ref.last_batch())
        assert dec.batch_header_stats() == (-1, 0, 0, 0, 0)
    # a byte-equal family: identical bytes and counters under "same" and "any", and the state afterwards is the one a mixed call leaves
    for rep in range(2):
        assert dec.set_option(OPT, "any") == 0
        a, _ = dec.decode_batch_crop_resize(equal, eq_rects, OW, OH)
        b, _ = ref.decode_batch_crop_resize(equal, eq_rects, OW, OH)
        assert same(a, eq_want) and same(b, eq_want)
        assert (dec.last_batch(), dec.region_stats(), dec.path_counters()[1:]) == (ref.last_batch(), ref.region_stats(), ref.path_counters()[1:]), rep
        assert dec.batch_header_stats()[:3] == (0, n - 1, 1)
        assert dec.set_option(OPT, "same") == 0
        a, _ = dec.decode_batch_crop_resize(equal, eq_rects, OW, OH)
        b, _ = ref.decode_batch_crop_resize(equal, eq_rects, OW, OH)
        assert same(a, eq_want) and dec.last_batch() == ref.last_batch() == (n - 1, 1)
        assert dec.batch_header_stats() == (-1, 0, 0, 0, 0)
    ref.close()
    dec.close()
    # "any" without "mixed" changes nothing: the batch of different sizes is refused as ever, a batch of one size is what it is without the option
    w, h = SIZES[2]
    one_size = [stream_of(O, "444_il", w, h, 500 + f) for f in range(3)]
    one_rects = [(0, 0, w, h), (w - 20, h - 11, 20, 11), (3, 5, 31, 17)]
    outs = []
    for value in (None, "any"):
        d2 = new_decoder(G, dlib)
        if value:
            assert d2.set_option(OPT, value) == 0
        with pytest.raises(RuntimeError):
            d2.decode_batch_crop_resize(streams, rects, OW, OH)
        got, _ = d2.decode_batch_crop_resize(one_size, one_rects, OW, OH)
        outs.append((got, d2.last_batch(), d2.region_stats(), d2.batch_header_stats()))
        d2.close()
    assert same(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:] and outs[1][3] == (-1, 0, 0, 0, 0)
    assert same(outs[0][0], expected(O, one_size, one_rects, OW, OH))


# ================================================================================================ 9. damaged family frames (CPU tier only)
def test_damaged_family_frames(O, G, emu, capfd):
    """frame 3 of the family is damaged -- an over-subscribed DHT, a DQT that is referenced but missing, a header cut inside a segment (and at 100 bytes: streams
    shorter than the first scan byte their slot is launched with), a scan damaged behind a valid header --: the call returns what it returns with the option off, with the same message; the other frames are right; nothing is
    written outside any frame's slot"""
    streams, rects, want = family(O, "444_il")  # (byte-equal headers: the neighbours go through the batched launches with the option off too)
    n, raw, f = len(streams), OW * OH * 3, 3
    good = bytes(streams[f])
    dht = good.index(b"\xff\xc4")
    over = bytearray(good)
    over[dht + 5] = 3  # (three codes of one bit)
    dqt = good.index(b"\xff\xdb")
    no_dqt = good[:dqt] + good[dqt + 2 + int.from_bytes(good[dqt + 2:dqt + 4], "big"):]
    cut = good[:dht + 20]
    begin = scan_begin(streams[f])
    scan = bytearray(good)
    scan[begin + 40:begin + 48] = b"\xff\xd3\xff\xd9\x00\xff\xd1\x12"
    assert len(cut) < scan_begin(streams[0]) and 100 < min(scan_begin(s) for s in streams)  # (streams shorter than every family frame's header)
    for kind, bad in (("over_subscribed_dht", bytes(over)), ("missing_dqt", no_dqt), ("cut_header", cut), ("cut_at_100_bytes", good[:100]),
                      ("damaged_scan", bytes(scan))):
        batch = streams[:f] + [np.frombuffer(bad, np.uint8)] + streams[f + 1:]
        seen = []
        for maker in (mixed_decoder, any_decoder):
            dec = maker(G, emu)
            dec.decode_batch_crop_resize(streams[:1], rects[:1], OW, OH)  # (a header to launch on)
            for rep in range(2):
                capfd.readouterr()
                out = np.full(raw * n + 256, 0xA5, np.uint8)
                rc = raw_call(G, emu, dec, batch, rects, OW, OH, out, raw)
                # (the whole of stderr but for ONE note: "[Info] Reinitializing decoder." says that the coder was set up for another image size, and how
                # often that happens is routing -- with the option off a stream shorter than the cached header sends EVERY frame of the call down the
                # single-frame route, one set-up per size; with `any` the neighbours stay in the batched launches)
                err = "".join(x for x in capfd.readouterr().err.splitlines(True) if x.strip() != "[GPUJPEG] [Info] Reinitializing decoder.")
                assert np.all(out[raw * n:] == 0xA5), (kind, rep)
                seen.append((rc, err, out.copy()))
                if rc == 0:
                    got = [out[i * raw:(i + 1) * raw] for i in range(n)]
                    assert same(got[:f] + got[f + 1:], want[:f] + want[f + 1:]), (kind, rep)
            got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)  # the decoder decodes the intact streams as ever
            assert same(got, want), kind
            dec.close()
        for a, b in zip(seen[:2], seen[2:]):
            assert a[0] == b[0] and a[1] == b[1], (kind, a[:2], b[:2])
            if a[0] == 0:
                assert np.array_equal(a[2], b[2]), kind


# ================================================================================================ 10. GPU only: device-resident streams
@pytest.mark.gpu
def test_device_streams_and_device_output(O, G, gpu_lib):
    """streams and pixels in device memory: the headers come to the host by the gather launch -- one of them, 20 KB long, on its own --, every frame
    goes through the batched launches from the first call on once a header is cached, the bytes between the slots are untouched"""
    import torch
    streams, rects, _ = varied_family(O, "420_il")
    streams = list(streams)
    streams[4] = with_segment(streams[4], 0xE1, (thumbnail(O) * 40)[:20000])
    want = expected(O, streams, rects, OW, OH)
    n, raw = len(streams), OW * OH * 3
    sizes = [int(x.size) for x in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    d_in = torch.from_numpy(host).cuda()
    out_stride = raw + 61
    d_out = torch.full((out_stride * n,), 0xA5, dtype=torch.uint8, device="cuda")
    dec = any_decoder(G, gpu_lib, perf=True)
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
    rc, fam, sets, nbytes, fetched = dec.batch_header_stats()
    long_ones = [f for f in range(n) if scan_begin(streams[f]) > GATHER]  # (the 20 KB segment, and the comment that reaches a later part)
    assert long_ones == [4, 6]
    assert (rc, fam, sets, fetched) == (0, n, len({table_key(s) for s in streams}), len(long_ones))
    assert nbytes == n * GATHER + sum(min(sizes[f], HDR_WINDOW) for f in long_ones)
    dec.close()
