"""Streams WITHOUT restart markers through the batched launches of the batch calls (dec_opt_batch_restartless = on; gpujpeg_amd_ext.h).

Frame f of every batch call stays what the single-frame call returns for stream f. Expected bytes never come from the product: the oracle decode
(full frames), expected() of test_scaled_decode.py (dec_opt_scale), the cropped oracle decode of test_region_batch.py (regions), expected() of
test_crop_resize.py and the prescale / subsampled / antialias / tensor restatements (crop-and-resize). Every comparison is byte for byte.

The streams are oracle-encoded with restart interval 0, one FAMILY (one header but for SOF0's dimensions) per scan kind. Every family has the three
kinds of frame the sub-sequence decoder tells apart (k_huffman_decode_par: a stage of 8192 bytes and 1280 blocks, pieces of 8192 - 64 bytes):
    stage   every scan fits the stage: <= 8192 - 11 bytes and <= 1280 blocks;
    blocks  a scan over the block limit but within the byte limit (smooth content at a size of more than 1280 blocks per scan);
    pieces  every scan is longer than three pieces (noise).
`blocks` and `pieces` frames have the family's LARGE size, so that the calls that need equal sizes see them in one batch; the mixed-size call sees all
three kinds plus a frame taller than wide. No large size is a multiple of the MCU except 4:4:4's 176 x 168 (the issue's example of 1386 blocks).

Two tiers with the same bodies, like test_crop_resize_mixed.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Damaged streams run on the CPU tier only."""
import numpy as np
import pytest

from conftest import natural_image, oracle_image
from test_crop_resize import diffs, expected, raw_call
from test_crop_resize_mixed import FAMILIES, family_case, family_headers_differ_in_dimensions_only, with_comment
from test_region_batch import dlib, emu, new_decoder, oracle_crops, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_region_decode import perf_decoder

OPT = "dec_opt_batch_restartless"
STAGE_BYTES, STAGE_BLOCKS, PIECE = 8192 - 11, 1280, 8192 - 64
OW, OH = 24, 16

# family -> (small size, large size, amplitude of the smooth frame's noise, a size taller than wide)
SHAPES = {
    "444_il": ((40, 24), (176, 168), 4, (35, 67)),
    "420_il": ((40, 24), (250, 215), 4, (51, 67)),  # (whole images to 12 x 8: s_f = 2, 8, 8, 4)
    # (three scans: the small frames are noise at quality 95, so that SOS / SOS / EOI do not share one 4 KB part of the marker scan -- FAMILY_SIZES of
    # test_crop_resize_mixed.py; the smooth frame's chrominance scans are the ones over the block limit, its luminance scan is two pieces)
    "444_nonil": ((72, 56), (300, 310), 1, (61, 88)),
    "gray": ((40, 24), (300, 290), 4, (35, 67)),
}


def smooth_image(w, h, comps, amp, seed):
    """gradients plus +-amp of noise: a few bytes per block"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200 // w + 20, yy * 200 // h + 20, (xx + yy) * 100 // (w + h) + 60][:comps], -1)
    return (base + rng.integers(-amp, amp + 1, base.shape)).clip(0, 255).astype(np.uint8).reshape(-1)


def stream_of(O, fam, w, h, kind, seed, **over):
    over.setdefault("ri", 0)
    case = family_case(fam, w, h, **over)
    comps = {0: 1, 1: 3}[case[3]]
    if kind == "smooth":
        raw = smooth_image(w, h, comps, SHAPES[fam][2], seed)
    elif kind == "natural" and fam != "444_nonil":
        raw = natural_image(w, h, comps, seed=seed)
    else:
        raw = O.noise(O.raw_size(w, h, case[3]), seed=seed)
    return O.encode(oracle_image(O, case), raw)


def scans_of(jpeg):
    """[(first byte, bytes)] of the entropy-coded data of every scan"""
    b, out, at = bytes(jpeg), [], 0
    while True:
        i = b.find(b"\xff\xda", at)
        if i < 0:
            return out
        start = i + 2 + int.from_bytes(b[i + 2:i + 4], "big")
        j = start
        while True:
            j = b.index(b"\xff", j)
            if b[j + 1] != 0 and not 0xD0 <= b[j + 1] <= 0xD7:
                break
            j += 2
        out.append((start, j - start))
        at = j


def blocks_per_scan(fam, w, h):
    if fam == "420_il":
        return [((w + 15) // 16) * ((h + 15) // 16) * 6]
    per = ((w + 7) // 8) * ((h + 7) // 8)
    return {"444_il": [3 * per], "444_nonil": [per] * 3, "gray": [per]}[fam]


def kind_of(fam, jpeg, w, h):
    """which of the three kinds a stream is, from its bytes and geometry"""
    lens, blocks = [n for _, n in scans_of(jpeg)], blocks_per_scan(fam, w, h)
    assert len(lens) == len(blocks) and b"\xff\xd0" not in bytes(jpeg)[scans_of(jpeg)[0][0]:]
    if all(n <= STAGE_BYTES and k <= STAGE_BLOCKS for n, k in zip(lens, blocks)):
        return "stage"
    if all(n > 3 * PIECE for n in lens):
        return "pieces"
    if any(n <= STAGE_BYTES and k > STAGE_BLOCKS for n, k in zip(lens, blocks)):
        return "blocks"
    return "other"


_made = {}


def equal_set(O, fam, which):
    """(streams, size) of one image size: the family's large one -- smooth, noise, smooth, noise -- or its small one (three frames that fit the stage)"""
    key = (fam, which)
    if key not in _made:
        small, large = SHAPES[fam][:2]
        if which == "large":
            w, h = large
            streams = [stream_of(O, fam, w, h, kind, 700 + f) for f, kind in enumerate(["smooth", "noise", "smooth", "noise"])]
            assert [kind_of(fam, s, w, h) for s in streams] == ["blocks", "pieces", "blocks", "pieces"], [scans_of(s) for s in streams]
        else:
            w, h = small
            streams = [stream_of(O, fam, w, h, "natural", 720 + f) for f in range(3)]
            assert [kind_of(fam, s, w, h) for s in streams] == ["stage"] * 3
        _made[key] = (streams, (w, h))
    return _made[key]


def mixed_set(O, fam):
    """(streams, sizes) of different image sizes: stage, pieces, blocks, and a frame taller than wide -- the long frame neither first nor last"""
    key = (fam, "mixed")
    if key not in _made:
        small, large, _, tall = SHAPES[fam]
        sizes = [small, large, large, tall]
        streams = [equal_set(O, fam, "small")[0][0], equal_set(O, fam, "large")[0][1], equal_set(O, fam, "large")[0][0],
                   stream_of(O, fam, *tall, "natural", 730)]
        assert [kind_of(fam, s, w, h) for s, (w, h) in zip(streams, sizes)][:3] == ["stage", "pieces", "blocks"] and tall[1] > tall[0]
        assert family_headers_differ_in_dimensions_only(streams)
        _made[key] = (streams, sizes)
    return _made[key]


def rects_of(sizes):
    """per frame, in turn: the whole image, a rectangle that touches the right and bottom edges, an inner rectangle, one pixel"""
    out = []
    for f, (w, h) in enumerate(sizes):
        out.append([(0, 0, w, h), (w // 3, h // 4, w - w // 3, h - h // 4), (1, 2, w // 2, h // 2), (w - 1, h - 1, 1, 1)][f % 4])
    return out


def origins_of(w, h, rw, rh, n):
    """the top left corner, the rectangle that ends at both edges, and two inner ones (inside the image for every rw <= w - 13, rh <= h - 9, or rw == w)"""
    return [[(0, 0), (w - rw, h - rh), (min(13, w - rw), min(9, h - rh)), ((w - rw) // 2, min(1, h - rh))][f % 4] for f in range(n)]


def the_decoder(G, lib, value="on", perf=False, pf=None, cs=None, mixed=False):
    dec = perf_decoder(G, lib) if perf else new_decoder(G, lib, pf, cs)
    if value is not None:
        assert dec.set_option(OPT, value) == 0
    if mixed:
        assert dec.set_option("dec_opt_batch_sizes", "mixed") == 0
    return dec


def counted(dec, n, restartless_batched=True):
    batched, single = dec.last_batch()
    assert batched + single == n, (batched, single)
    if restartless_batched:
        assert batched >= n - 1, (batched, single)
    else:
        assert batched == 0, (batched, single)


def every_call(O, G, lib, fam, value, chunk=0):
    """the calls of case 1 on one decoder each, twice: bytes against the oracle's, frames counted"""
    from test_scaled_batch import set_scale, wanted
    from test_crop_resize_tensor import CHW, F16, IMAGENET, tensors_equal
    on = value == "on"
    for which in ("large", "small"):
        streams, (w, h) = equal_set(O, fam, which)
        n = len(streams)
        full = [O.decode(s)[0] for s in streams]
        dec = the_decoder(G, lib, value)
        dec.set_batch_chunk(chunk)
        for s in (1, 2, 8):  # decode_batch at full size and with dec_opt_scale
            set_scale(dec, s)
            want = full if s == 1 else wanted(O, streams, s)
            for rep in range(2):
                got, _ = dec.decode_batch(streams)
                assert same(got, want), (which, s, rep, diffs(got, want))
                counted(dec, n, on)
        set_scale(dec, 1)
        rw, rh = min(w, 100), min(h, 45)
        origins = origins_of(w, h, rw, rh, n)
        want = oracle_crops(O, streams, origins, rw, rh)
        for rep in range(2):
            got, pi = dec.decode_batch_regions(streams, origins, rw, rh)
            assert (pi.width, pi.height) == (rw, rh) and same(got, want), (which, rep, diffs(got, want))
            counted(dec, n, on)
        rects = rects_of([(w, h)] * n)
        want = expected(O, streams, rects, OW, OH)
        for rep in range(2):
            got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
            assert same(got, want), (which, rep, diffs(got, want))
            counted(dec, n, on)
        dec.close()
    streams, sizes = mixed_set(O, fam)
    n, rects = len(streams), rects_of(sizes)
    want = expected(O, streams, rects, OW, OH)
    dec = the_decoder(G, lib, value, mixed=True)
    dec.set_batch_chunk(chunk)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        counted(dec, n, on)
    if fam != "gray":
        scale, bias = IMAGENET
        for rep in range(2):
            got, _ = dec.decode_batch_crop_resize_tensor(streams, rects, OW, OH, F16, CHW, scale, bias)
            assert tensors_equal(got, want, 1, OW, OH, F16, CHW, scale, bias) == [0] * n, rep
            counted(dec, n, on)
    dec.close()


# ================================================================================================ 1. every call, option on
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_every_call_with_the_option_on(O, G, dlib, fam):
    every_call(O, G, dlib, fam, "on")


# ================================================================================================ 2. option off / absent
@pytest.mark.parametrize("value", ["off", None])
def test_option_off_or_absent(O, G, dlib, value):
    """the same calls, the same bytes, and no restart-less frame counted as batched: the route of every earlier release"""
    every_call(O, G, dlib, "420_il", value)


# ================================================================================================ 3. chunks
@pytest.mark.parametrize("fam", ["444_il", "444_nonil"])
def test_chunks(O, G, dlib, fam):
    every_call(O, G, dlib, fam, "on", chunk=2)


# ================================================================================================ 4. composition
def test_composition_on_420(O, G, dlib):
    """4:2:0, whole-image rectangles to 12 x 8 so that s_f differs between the frames: prescale, prescale per component, antialias with the mirror,
    and the other output formats"""
    import test_crop_resize_prescale as pre
    import test_crop_resize_prescale_subsampled as sub
    from test_crop_resize_antialias import aa_expected
    streams, sizes = mixed_set(O, "420_il")
    n, ow, oh = len(streams), 12, 8
    rects = [(0, 0, w, h) for w, h in sizes]
    for name, opts, idct in (("prescale", (("dec_opt_resize_prescale", "1/8"),), 5),
                             ("subsampled", (("dec_opt_resize_prescale", "1/8"), ("dec_opt_resize_prescale_subsampled", "on")), 8)):
        # (without the subsampled option a 4:2:0 stream keeps s_f = 1: the plan of streams whose components are not all 1 x 1)
        want, plans = pre.expected(O, streams, rects, ow, oh, 8, all_1x1=False) if name == "prescale" else sub.expected(O, streams, rects, ow, oh, 8)
        scales = [p[0] for p in plans]
        assert scales == [1] * n if name == "prescale" else len(set(scales)) >= 3, scales
        dec = the_decoder(G, dlib, perf=True, mixed=True)
        for o in opts:
            assert dec.set_option(*o) == 0
        for rep in range(2):
            got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
            assert same(got, want), (name, rep, diffs(got, want))
            assert list(dec.prescales()) == scales and dec.idct_path() == idct, (name, dec.prescales(), dec.idct_path())
            counted(dec, n)
        dec.close()
    flags = [1, 0, 1, 1]
    want = aa_expected(O, streams, rects, ow, oh)
    want = [x.reshape(oh, ow, 3)[:, ::-1].reshape(-1) if m else x for x, m in zip(want, flags)]
    dec = the_decoder(G, dlib, perf=True, mixed=True)
    assert dec.set_option("dec_opt_resize_filter", "antialias") == 0
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh, mirror=flags)
        assert same(got, want), ("antialias", rep, diffs(got, want))
        assert dec.idct_path() == 7
        counted(dec, n)
    dec.close()
    for pf, cs in ((0, 3), (2, 3), (6, 1)):
        want = expected(O, streams, rects, ow, oh, pf, cs)
        dec = the_decoder(G, dlib, pf=pf, cs=cs, mixed=True)
        for rep in range(2):
            got, pi = dec.decode_batch_crop_resize(streams, rects, ow, oh)
            assert pi.pixel_format == pf and same(got, want), (pf, rep, diffs(got, want))
            counted(dec, n)
        dec.close()


# ================================================================================================ 5. leaving a scan early
def prefix_bytes(O, fam, jpeg_raw, w, h, rows):
    """per scan, the entropy-coded bytes up to the end of the first `rows` pixel rows (whole MCU rows): those of the stream of the image's top rows
    alone, which codes the same blocks with the same predictors in the same order, padded to a whole byte"""
    top = jpeg_raw.reshape(h, -1)[:rows].reshape(-1)
    return [n for _, n in scans_of(O.encode(oracle_image(O, family_case(fam, w, rows, ri=0)), top))]


@pytest.mark.parametrize("fam", ["444_il", "420_il", "444_nonil"])
def test_a_scan_is_left_behind_the_cover(O, G, dlib, fam):
    """three `pieces` frames of one size. A rectangle in the top 8 rows: the cover ends with the first row of MCUs, whose last block is complete after
    p bytes of the scan, so the workgroup stops at the first piece boundary at or behind p -- ceil(p / PIECE) pieces of PIECE = 8192 - 64 bytes --
    and out[1] is at most the sum of those over the scans of the frames the batched launches took. A rectangle that touches the last pixel, and the
    last pixel alone: everything is read. Then whole images with the option on and off and a full-frame batch: nothing the stop left behind shows."""
    w, h = SHAPES[fam][1]
    case = family_case(fam, w, h, ri=0)
    raws = [O.noise(O.raw_size(w, h, case[3]), seed=760 + f) for f in range(3)]
    streams = [O.encode(oracle_image(O, case), r) for r in raws]
    assert all(kind_of(fam, s, w, h) == "pieces" for s in streams)
    n, mcu_rows = len(streams), 16 if fam == "420_il" else 8
    lens = [[k for _, k in scans_of(s)] for s in streams]
    tops = [prefix_bytes(O, fam, r, w, h, mcu_rows) for r in raws]
    dec = the_decoder(G, dlib)

    def call(rects, on=True):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        want = expected(O, streams, rects, OW, OH)
        assert same(got, want), (rects[0], diffs(got, want))
        batched, single = dec.last_batch()
        assert batched + single == n and (batched >= n - 1 if on else batched == 0), (on, batched, single)
        return list(range(n - batched, n)), dec.entropy_bytes()  # (a frame that goes ahead of the launches is frame 0)

    for rep in range(2):
        took, (rc, handed, read) = call([(5, 2, w - 9, 6)] * n)
        bound = sum(min(k, -(-p // PIECE) * PIECE) for f in took for k, p in zip(lens[f], tops[f]))
        print(f"{fam}: handed {handed} B, read {read} B, bound {bound} B")
        assert rc == 0 and handed == sum(sum(lens[f]) for f in took), (handed, lens)
        assert read < handed and read <= bound and read % PIECE == 0, (read, handed, bound)
        for rects in ([(w - 30, h - 20, 30, 20)] * n, [(w - 1, h - 1, 1, 1)] * n):
            took, (rc, handed, read) = call(rects)
            assert rc == 0 and read == handed == sum(sum(lens[f]) for f in took), (rects[0], handed, read)
        whole = [(0, 0, w, h)] * n
        took, (rc, handed, read) = call(whole)
        assert rc == 0 and read == handed
        assert dec.set_option(OPT, "off") == 0
        assert call(whole, on=False)[1] == (-1, 0, 0)
        got, _ = dec.decode_batch(streams)
        assert same(got, [O.decode(s)[0] for s in streams]) and dec.entropy_bytes() == (-1, 0, 0)
        assert dec.set_option(OPT, "on") == 0
        got, _ = dec.decode_batch(streams)
        assert same(got, [O.decode(s)[0] for s in streams])
        rc, handed, read = dec.entropy_bytes()
        assert rc == 0 and handed == read and handed > 0
        dec.decode(streams[0])
        assert dec.entropy_bytes() == (-1, 0, 0)
    dec.close()


def test_the_early_stop_can_be_switched_off_for_measurements(O, G, emu, monkeypatch):
    """GJ_DEC_NO_EARLY_STOP=1 (the A/B setting of tools/restartless_batch_times.py): the same bytes, everything read"""
    fam = "444_il"
    streams, (w, h) = equal_set(O, fam, "large")
    rects = [(5, 2, w - 9, 6)] * len(streams)
    monkeypatch.setenv("GJ_DEC_NO_EARLY_STOP", "1")
    dec = the_decoder(G, emu)
    got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
    assert same(got, expected(O, streams, rects, OW, OH))
    rc, handed, read = dec.entropy_bytes()
    assert rc == 0 and read == handed > 0
    dec.close()


# ================================================================================================ 6. strangers
def test_strangers_inside_a_restartless_family(O, G, dlib):
    """another quality, an added COM segment and a frame WITH a restart interval: the same bytes; exactly those frames -- and frame 0 where it goes
    ahead of the launches -- are counted single"""
    fam = "444_il"
    streams, sizes = mixed_set(O, fam)
    streams, sizes = list(streams) + [equal_set(O, fam, "small")[0][1], equal_set(O, fam, "small")[0][2]], list(sizes) + [SHAPES[fam][0]] * 2
    strangers = {2: stream_of(O, fam, *sizes[2], "smooth", 781, q=40), 3: stream_of(O, fam, *sizes[3], "natural", 782, ri=3), 4: with_comment(streams[4])}
    for f, s in strangers.items():
        streams[f] = s
    n, rects = len(streams), rects_of(sizes)
    want = expected(O, streams, rects, OW, OH)
    dec = the_decoder(G, dlib, mixed=True)
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), (rep, diffs(got, want))
        batched, single = dec.last_batch()
        assert batched + single == n and len(strangers) <= single <= len(strangers) + 1, (rep, batched, single)
    dec.close()


# ================================================================================================ 7. damaged streams (CPU tier only)
def test_damaged_restartless_streams(O, G, emu):
    """a restart-less stream truncated in the middle of its scan, and one with a stray RST0 in its scan, inside a batch: the call's return code and
    the other frames' bytes are those of the call with the option off; the bytes behind the output are untouched"""
    fam = "444_il"
    streams, sizes = mixed_set(O, fam)
    n, raw, f = len(streams), OW * OH * 3, 1
    rects = rects_of(sizes)
    start, length = scans_of(streams[f])[0]
    stray = streams[f].copy()
    at = start + length // 2
    while stray[at - 1] == 0xFF or stray[at + 2] == 0:  # (not behind a 0xFF, and not in front of a byte that would read as stuffing)
        at += 1
    stray[at:at + 2] = [0xFF, 0xD0]
    for kind, bad in (("truncated", streams[f][:start + length // 2].copy()), ("stray RST0", stray)):
        batch = streams[:f] + [bad] + streams[f + 1:]
        results = {}
        for value in ("off", "on"):
            dec = the_decoder(G, emu, value, mixed=True)
            for rep in range(2):
                out = np.full(raw * n + 256, 0xA5, np.uint8)
                rc = raw_call(G, emu, dec, batch, rects, OW, OH, out, raw)
                assert np.all(out[raw * n:] == 0xA5), (kind, value, rep)
                results[value, rep] = (rc, [out[i * raw:(i + 1) * raw].copy() for i in range(n) if i != f])
            if results[value, 1][0] == 0:
                got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)  # the decoder decodes the intact streams as ever
                assert same(got, expected(O, streams, rects, OW, OH)), (kind, value)
            dec.close()
        for rep in range(2):
            assert results["on", rep][0] == results["off", rep][0], (kind, rep)
            if results["on", rep][0] == 0:
                assert same(results["on", rep][1], results["off", rep][1]), (kind, rep)


# ================================================================================================ 8. refusals
def test_refusals(O, G, dlib, capfd):
    fam = "444_il"
    streams, sizes = mixed_set(O, fam)
    n, raw, rects = len(streams), OW * OH * 3, rects_of(sizes)
    want = expected(O, streams, rects, OW, OH)
    dec = the_decoder(G, dlib, mixed=True)
    for value in ("both", "", "On", "1", "on "):  # a bad value is refused and the setting is kept
        assert dec.set_option(OPT, value) != 0
    got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
    assert same(got, want) and dec.last_batch()[0] >= n - 1 and dec.entropy_bytes()[0] == 0
    # a rectangle outside its frame's image: refused before anything is written, the message names the frame
    bad = list(rects)
    bad[3] = (20, 40, 30, 40)  # (inside the large frames, outside frame 3's 35 x 67)
    capfd.readouterr()
    out = np.full(raw * n + 64, 0xA5, np.uint8)
    assert raw_call(G, dlib, dec, streams, bad, OW, OH, out, raw) == -1 and np.all(out == 0xA5)
    assert "Frame 3 of the batch" in capfd.readouterr().err
    assert dec.entropy_bytes() == (-1, 0, 0)
    # dec_opt_flipped: refused by the call as without the option
    assert dec.set_option("dec_opt_flipped", "1") == 0
    assert raw_call(G, dlib, dec, streams, rects, OW, OH, out, raw) == -1 and np.all(out == 0xA5)
    assert dec.set_option("dec_opt_flipped", "0") == 0
    assert raw_call(G, dlib, dec, streams, rects, OW, OH, out, raw) == 0
    assert same([out[i * raw:(i + 1) * raw] for i in range(n)], want) and np.all(out[n * raw:] == 0xA5)
    dec.close()
    # streams of different sizes without dec_opt_batch_sizes = mixed stay refused
    dec = the_decoder(G, dlib)
    with pytest.raises(RuntimeError):
        dec.decode_batch_crop_resize(streams, [(0, 0, 8, 8)] * n, OW, OH)
    dec.close()
