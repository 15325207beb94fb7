"""The orientation a stream carries, for callers of the crop-and-resize calls: gpujpeg_amd_host_stream_orientation and
gpujpeg_amd_host_orientation_plan (host only; gpujpeg_amd_ext.h).

The batch calls return pixels in stored orientation. The two functions give a caller (rot, flip) of a stream as the reader parses it from Exif APP1 /
SPIFF, and, for a rectangle of the stream's DISPLAY image D = orient(I), the rectangle's pre-image rect' in I, the output size (OW', OH') to ask the call
for and the three bits that turn the returned frame R' into mirror(orient(R')).

Nothing expected comes from the product: orient() is np.rot90 and a column reversal; rect' is read off the oriented INDEX image arange(W H), not
computed by formula (pre_image); the bits are checked by what they mean, on an index image of R'. The last test puts the pieces together on the CPU tier
(tests/hipemu): planner, the crop-and-resize call as it is, the bits applied in numpy, against expected() of test_crop_resize.py over the ORACLE decode.

The streams are oracle-encoded streams of test_crop_resize_mixed.py's families with an Exif APP1 segment (IFD0 with tag 0x0112, values 1 to 8, II and MM)
spliced in behind SOI; one variant carries the orientation in a SPIFF directory entry, one carries none. On the parent commit every test that touches
the library fails: it lacks the exports."""
import struct

import numpy as np
import pytest

from test_batch_headers import thumbnail, with_segment
from test_crop_resize import BPP, diffs, expected
from test_crop_resize_mixed import MIXED, SIZES, rects_of, stream_of
from test_region_batch import emu, new_decoder, same  # noqa: F401  (emu: the fixture of the CPU tier)

ANY = ("dec_opt_batch_headers", "any")
EXIF = {1: (0, 0), 2: (0, 1), 3: (2, 0), 4: (2, 1), 5: (1, 1), 6: (1, 0), 7: (3, 1), 8: (3, 0)}  # Exif value -> (quarter turns clockwise, then mirrored)
ALL8 = [EXIF[v] for v in range(1, 9)]
OUTS = [(37, 21), (5, 3), (1, 7), (1, 1)]  # OW != OH


# ================================================================================================ the definition, in numpy
def orient(a, rot, flip):
    """the display image of the stored image a (rows, columns, ...): rot quarter turns clockwise, then mirrored left-right if flip"""
    a = np.rot90(a, k=-rot)
    return a[:, ::-1] if flip else a


def display_size(w, h, rot):
    return (h, w) if rot & 1 else (w, h)


def pre_image(w, h, rot, flip, rect):
    """the rectangle of the stored w x h image whose pixels the rectangle `rect` of the display image shows, from the index image"""
    x, y, rw, rh = rect
    idx = orient(np.arange(w * h).reshape(h, w), rot, flip)[y:y + rh, x:x + rw]
    assert idx.shape == (rh, rw), "the rectangle is not inside the display image"
    sx, sy = idx % w, idx // w
    out = (int(sx.min()), int(sy.min()), int(sx.max() - sx.min() + 1), int(sy.max() - sy.min() + 1))
    assert out[2] * out[3] == rw * rh
    return out


def orient_frame(flat, pf, owp, ohp, rot, flip, mirror=False):
    """frame R' (owp x ohp, pixel format pf, no padding) -> mirror(orient(R')) in the same format"""
    if pf == 2:
        a = flat.reshape(3, ohp, owp).transpose(1, 2, 0)
    else:
        a = flat.reshape(ohp, owp, BPP[pf])
    a = orient(a, rot, flip)
    if mirror:
        a = a[:, ::-1]
    return np.ascontiguousarray(a.transpose(2, 0, 1) if pf == 2 else a).reshape(-1)


def oriented_expected(O, streams, rects, orients, ow, oh, fn=expected, pf=None, cs=None, mirror=None, extra=(), pick=None):
    """mirror_f(orient(fn(stream f, rect', OW', OH'))) per frame; fn: one of the restatements of the call without the option"""
    out = []
    for f, (jpeg, rect, (rot, flip)) in enumerate(zip(streams, rects, orients)):
        img = O.decode(jpeg, -1 if pf is None else pf, -1 if cs is None else cs)[1]
        rp = pre_image(img.width, img.height, rot, flip, rect)
        owp, ohp = display_size(ow, oh, rot)
        r = fn(O, [jpeg], [rp], owp, ohp, *extra, pf, cs)
        r = r[0] if pick is None else pick(r)[0]
        out.append(orient_frame(r, img.pixel_format, owp, ohp, rot, flip, bool(mirror and mirror[f])))
    return out


# ================================================================================================ streams
def exif_app1(value, order="II", count=1, typ=3, magic=0x2A, ifd1_value=None, thumb=b"", entries_claimed=None, cut=None):
    """the payload of an Exif APP1 segment: TIFF header, IFD0 with tag 0x0112 = value (and tag 0x010F ahead of it, so that it is not the first entry);
    ifd1_value: an IFD1 with an orientation of its own and a JPEG thumbnail behind it"""
    e = "<" if order == "II" else ">"
    short = struct.pack(e + "H", value) + b"\0\0"  # (a SHORT sits in the first two bytes of the value field in either byte order)
    entries = [struct.pack(e + "HHI", 0x010F, 2, 4) + b"abc\0", struct.pack(e + "HHI", 0x0112, typ, count) + short]
    n = len(entries) if entries_claimed is None else entries_claimed
    ifd0 = struct.pack(e + "H", n) + b"".join(entries)
    next_at = 8 + len(ifd0) + 4
    tiff = order.encode() + struct.pack(e + "HI", magic, 8) + ifd0 + struct.pack(e + "I", next_at if ifd1_value is not None else 0)
    if ifd1_value is not None:
        at = next_at + 2 + 3 * 12 + 4
        tiff += struct.pack(e + "H", 3) + struct.pack(e + "HHI", 0x0112, 3, 1) + struct.pack(e + "H", ifd1_value) + b"\0\0" + \
            struct.pack(e + "HHII", 0x0201, 4, 1, at) + struct.pack(e + "HHII", 0x0202, 4, 1, len(thumb)) + struct.pack(e + "I", 0) + thumb
    payload = b"Exif\0\0" + tiff
    return payload if cut is None else payload[:cut]


def with_exif(jpeg, value, order="II", **kw):
    return with_segment(jpeg, 0xE1, exif_app1(value, order, **kw))


def spiff_stream(O, w, h, seed, rot, flip):
    """an oracle stream with a SPIFF header (4:4:4, BT.709 inside) and an orientation entry in its directory"""
    import oracle
    img = oracle.make_image(w, h, pixel_format=1, color_space=1, quality=75, restart_interval=3, interleaved=1, color_space_internal=oracle.CS_BT709)
    jpeg = O.encode(img, O.noise(O.raw_size(w, h, 1), seed=seed))
    b = bytes(jpeg)
    assert b[2:4] == b"\xff\xe8" and b[6:12] == b"SPIFF\0", "the oracle did not write a SPIFF header"
    at = 4 + int.from_bytes(b[4:6], "big")  # the end-of-directory entry
    assert b[at:at + 2] == b"\xff\xe8"
    entry = b"\xff\xe8" + (10).to_bytes(2, "big") + (4).to_bytes(4, "big") + bytes([rot, flip, 0, 0])
    return np.frombuffer(b[:at] + entry + b[at:], np.uint8)


def oriented_family(O, fam, sizes, orients, seed=500, orders=("II", "MM"), **over):
    """one stream per size with the Exif value of its orientation, byte orders in turn"""
    value = {v: k for k, v in EXIF.items()}
    return [with_exif(stream_of(O, fam, w, h, seed + f, **over), value[orients[f]], orders[f % len(orders)]) for f, (w, h) in enumerate(sizes)]


def display_rects(sizes, orients):
    """rects_of() over the DISPLAY sizes: the whole image, a rectangle that touches the right and bottom edges, one pixel, an inner one"""
    return rects_of([display_size(w, h, rot) for (w, h), (rot, _) in zip(sizes, orients)])


SIZES8 = SIZES + [(97, 40)]


# ================================================================================================ 0. the definition alone
def test_orient_is_exif():
    """Exif 1 .. 8 by their meaning: 2 mirrored, 3 upside down, 4 flipped vertically, 5 transposed, 6 to be turned clockwise, 7 transverse, 8 anticlockwise"""
    a = np.arange(12).reshape(3, 4)
    want = {1: a, 2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1], 5: a.T, 6: a.T[:, ::-1], 7: a[::-1, ::-1].T, 8: a.T[::-1]}
    for v, (rot, flip) in EXIF.items():
        assert np.array_equal(orient(a, rot, flip), want[v]), v
        assert orient(a, rot, flip).shape == display_size(4, 3, rot)[::-1]


def test_orient_against_pil():
    ImageOps = pytest.importorskip("PIL.ImageOps")
    from PIL import Image
    a = (np.arange(15 * 22 * 3) % 251).astype(np.uint8).reshape(15, 22, 3)
    for v, (rot, flip) in EXIF.items():
        im = Image.fromarray(a)
        im.getexif()[0x0112] = v
        got = np.asarray(ImageOps.exif_transpose(im))
        assert np.array_equal(got, orient(a, rot, flip)), v


# ================================================================================================ 1. host only
def test_stream_orientation_host_only(O, G, lib):
    base = stream_of(O, "444_il", 40, 24, 7)
    assert G.stream_orientation(lib, base) == (0, 0, 0, 40, 24)
    for v, (rot, flip) in EXIF.items():
        for order in ("II", "MM"):
            dw, dh = display_size(40, 24, rot)
            assert G.stream_orientation(lib, with_exif(base, v, order)) == (1, rot, flip, dw, dh), (v, order)
    # flawed tags count as not set, as the reader decides: values 0 and 9, an IFD that claims more entries than the segment holds, a segment cut inside
    # the IFD, a wrong TIFF magic, a wrong byte-order mark
    for bad in (with_exif(base, 0), with_exif(base, 9), with_exif(base, 9, "MM"), with_exif(base, 6, entries_claimed=40), with_exif(base, 6, cut=30),
                with_exif(base, 6, magic=0x2B), with_exif(base, 6, "MM", magic=0x2B),
                with_segment(base, 0xE1, exif_app1(6).replace(b"II", b"XI", 1))):
        assert G.stream_orientation(lib, bad) == (0, 0, 0, 40, 24)
    # an IFD1 with an orientation of its own behind a thumbnail: IFD0's holds
    assert G.stream_orientation(lib, with_exif(base, 6, "MM", ifd1_value=3, thumb=thumbnail(O))) == (1, 1, 0, 24, 40)
    assert G.stream_orientation(lib, spiff_stream(O, 40, 24, 3, 3, 1)) == (1, 3, 1, 24, 40)
    assert G.stream_orientation(lib, base[:40]) is None and G.stream_orientation(lib, np.zeros(64, np.uint8)) is None


def test_orientation_plan_host_only(G, lib):
    """the planner against the index image: random rectangles, rectangles at every edge, all eight orientations, both mirror flags"""
    rng = np.random.default_rng(8)
    for w, h in ((33, 130), (8, 8), (200, 97), (1, 5)):
        for rot, flip in ALL8:
            dw, dh = display_size(w, h, rot)
            rects = [(0, 0, dw, dh), (0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (0, dh - 1, dw, 1), (dw - 1, 0, 1, dh), (0, 0, 1, dh), (0, 0, dw, 1)]
            for _ in range(12):
                x, y = int(rng.integers(0, dw)), int(rng.integers(0, dh))
                rects.append((x, y, int(rng.integers(1, dw - x + 1)), int(rng.integers(1, dh - y + 1))))
            for rect in rects:
                for mirror in (0, 1):
                    for ow, oh in ((37, 21), (1, 7)):
                        got = G.orientation_plan(lib, w, h, rot, flip, rect, ow, oh, mirror)
                        assert got is not None and got[:4] == pre_image(w, h, rot, flip, rect), (w, h, rot, flip, rect)
                        assert got[4:6] == display_size(ow, oh, rot)
                        # the bits, from what they mean: output pixel (i, j) is pixel (i', j') of R'
                        owp, ohp = got[4:6]
                        rp = np.arange(owp * ohp).reshape(ohp, owp)
                        want = orient(rp, rot, flip)
                        want = want[:, ::-1] if mirror else want
                        T, FX, FY = got[6] & 4, got[6] & 1, got[6] & 2
                        jj, ii = np.mgrid[0:oh, 0:ow]
                        a, b = (jj, ii) if T else (ii, jj)
                        ip, jp = (owp - 1 - a if FX else a), (ohp - 1 - b if FY else b)
                        assert np.array_equal(rp[jp, ip], want), (rot, flip, mirror, got)
                        if not (rot or flip):
                            assert got[6] == mirror
            for bad in ((0, 0, dw + 1, 1), (0, 0, 1, dh + 1), (dw, 0, 1, 1), (-1, 0, 1, 1), (0, 0, 0, 1), (1, 1, dw, dh)):
                assert G.orientation_plan(lib, w, h, rot, flip, bad, 4, 4) is None, (w, h, rot, bad)
    assert G.orientation_plan(lib, 8, 8, 4, 0, (0, 0, 1, 1), 4, 4) is None and G.orientation_plan(lib, 8, 8, 0, 0, (0, 0, 1, 1), 0, 4) is None
    assert G.orientation_plan(lib, 8, 8, 1, 0, (0, 0, 1, 1), 16385, 4) is None


# ================================================================================================ 2. the pieces together, on the CPU tier
def turned(flat, pf, owp, ohp, ow, oh, bits):
    """frame R' -> the ow x oh frame whose pixel (i, j) is pixel (i', j') of R', by the bits"""
    a = flat.reshape(ohp, owp, BPP[pf])
    jj, ii = np.mgrid[0:oh, 0:ow]
    u, v = (jj, ii) if bits & 4 else (ii, jj)
    ip, jp = (owp - 1 - u if bits & 1 else u), (ohp - 1 - v if bits & 2 else v)
    return np.ascontiguousarray(a[jp, ip]).reshape(-1)


@pytest.mark.parametrize("ow,oh", OUTS[:2])
def test_planner_with_the_call_gives_the_display_orientation(O, G, emu, ow, oh):
    """eight streams, one Exif value each: stream_orientation, then the planner, then ONE crop-and-resize call per output size (OW', OH') on the
    pre-images, then the bits -- equal to mirror(orient(R')) with R' from the numpy restatement over the oracle decode"""
    streams = oriented_family(O, "444_il", SIZES8, ALL8, seed=520)
    rects = display_rects(SIZES8, ALL8)
    mirror = [1, 0, 0, 1, 1, 0, 1, 0]
    want = oriented_expected(O, streams, rects, ALL8, ow, oh, mirror=mirror)
    plans = []
    for jpeg, rect, (w, h), m in zip(streams, rects, SIZES8, mirror):
        is_set, rot, flip, dw, dh = G.stream_orientation(emu, jpeg)
        assert (dw, dh) == display_size(w, h, rot)
        plans.append(G.orientation_plan(emu, w, h, rot, flip, rect, ow, oh, m))
    assert [tuple(p[4:6]) for p in plans] == [display_size(ow, oh, rot) for rot, _ in ALL8]
    got = [None] * 8
    dec = new_decoder(G, emu)
    for k, v in (MIXED, ANY):
        assert dec.set_option(k, v) == 0
    for size in sorted({tuple(p[4:6]) for p in plans}):
        idx = [f for f in range(8) if tuple(plans[f][4:6]) == size]
        frames, pi = dec.decode_batch_crop_resize([streams[f] for f in idx], [plans[f][:4] for f in idx], *size)
        assert (pi.width, pi.height, pi.pixel_format) == size + (1,)
        for f, px in zip(idx, frames):
            got[f] = turned(px, 1, size[0], size[1], ow, oh, plans[f][6])
    dec.close()
    assert same(got, want), diffs(got, want)

