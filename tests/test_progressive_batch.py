"""dec_opt_batch_progressive = on (gpujpeg_amd_ext.h): the progressive frames of a batch call that form a GROUP -- same size, sampling, quantisation
tables and colour decisions -- go through batched launches, and frame f stays what the single-frame call returns for stream f: the image of its
baseline twin.

Streams, twins and expected bytes are those of test_progressive_decode.py: the Python writer of progressive_streams.py (chosen coefficients, scan
script, tables, restart interval; the twin is O.encode_from_coefs of the same coefficients) and files written by libjpeg through PIL
(tests/golden/progressive_batch/, make_progressive_batch_fixtures.py: the baseline save is the twin). Expected bytes never come from the product:
pixels are the oracle's decode of the twin, reduced images expected() of test_scaled_decode.py, regions the cropped oracle decode of
test_region_batch.py, crop-and-resize expected() of test_crop_resize.py and, for the options of that call, of the tests that define them. Every
comparison is byte for byte.

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on the MI355X. Damaged
streams run on the CPU tier only: nothing damaged is sent to a GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import progressive_streams as P
import synth_streams as SS
from test_crop_resize import expected as resized
from test_progressive_decode import BH, BW, S420, case, device_copy, image_of, prog_decoder
from test_region_batch import dlib, emu, oracle_crops, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_scaled_decode import expected as reduced

OPT = "dec_opt_batch_progressive"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive_batch")


def batch_decoder(G, lib, pf=None, cs=None):
    dec = prog_decoder(G, lib, pf, cs)
    assert dec.set_option(OPT, "on") == 0
    return dec


def image(w=BW, h=BH, quality=90, restart=0):
    import oracle as O
    return O.make_image(w, h, pixel_format=1, color_space=1, quality=quality, restart_interval=restart, interleaved=1, subsampling=S420)


def progressive(seed, script, restart=0, tables="per_scan", upto=None, w=BW, h=BH, quality=90):
    """-> (progressive stream, twin, script as written, restart interval) of a w x h 4:2:0 image with seeded coefficients"""
    import oracle as O
    from test_progressive_decode import prefix_coefficients
    img = image(w, h, quality)
    coefs = P.legal(img, SS.with_big(SS.sparse(img, seed=seed, density=0.3), 20, seed=seed), script)
    jpeg = P.write(img, coefs, script, restart=restart, tables=tables, upto=upto)
    shown = coefs if upto is None else prefix_coefficients(img, coefs, script[:upto])
    return jpeg, O.encode_from_coefs(img, shown), list(script)[:upto], restart


def baseline(seed, w=BW, h=BH):
    import oracle as O
    img = image(w, h, restart=2)
    return O.encode_from_coefs(img, P.legal(img, SS.sparse(img, seed=seed, density=0.3)))


@functools.lru_cache(maxsize=None)
def mixed_set(first_progressive):
    """three baseline streams of one header (restart interval 2: the batched launches take them) and five progressive streams of the same 64 x 48
    geometry between them -- libjpeg's script, deep approximation, chroma first, spectral selection only, a DC scan per component; restart intervals
    0, 1 and 2; tables per scan and up front; one stream that ends after its sixth scan -> (streams, twins, progressive flags, (script, restart) or None)"""
    B = [baseline(s) for s in (1, 2, 3)]
    Pg = [progressive(4, P.LIBJPEG_COLOUR, restart=1, upto=6), progressive(5, P.deep_approximation(3), restart=2, tables="up_front"),
          progressive(6, P.chroma_first(), restart=0), progressive(7, P.spectral_only(3), restart=0, tables="up_front"),
          progressive(8, P.dc_per_component(3), restart=2)]
    order = [("P", 0), ("B", 0), ("P", 1), ("P", 2), ("B", 1), ("P", 3), ("B", 2), ("P", 4)] if first_progressive else \
            [("B", 0), ("P", 0), ("B", 1), ("P", 1), ("P", 2), ("B", 2), ("P", 3), ("P", 4)]
    streams = [B[i] if k == "B" else Pg[i][0] for k, i in order]
    twins = [B[i] if k == "B" else Pg[i][1] for k, i in order]
    plans = [None if k == "B" else Pg[i][2:] for k, i in order]
    for a in streams + twins:
        a.setflags(write=False)
    return streams, twins, [k == "P" for k, _ in order], plans


@functools.lru_cache(maxsize=None)
def wanted(first_progressive):
    import oracle as O
    return [O.decode(t)[0] for t in mixed_set(first_progressive)[1]]


def group_of(prog, rep, first_progressive):
    """the frames of the call that are candidates of the progressive pass and progressive: with pixels wanted in host memory frame 0 goes ahead of
    everything (single whatever it is)"""
    return [f for f, p in enumerate(prog) if p and f > 0]


def stats_of(plans, frames, chunk):
    """(frames, groups = 1, launches, records) of one group of `frames` cut into chunks of `chunk`"""
    img = image()
    chunk = chunk or len(frames)
    launches = sum(max(max(P.levels_of(plans[f][0])) + 1 for f in frames[a:a + chunk]) for a in range(0, len(frames), chunk))
    records = sum(P.segment_count(img, plans[f][0], plans[f][1]) for f in frames)
    return (0, len(frames), 1, launches, records)


# ================================================================================================ 1. a call that mixes both kinds
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("first_progressive", [False, True])
def test_mixed_batch(O, G, dlib, first_progressive, chunk):
    streams, twins, prog, plans = mixed_set(first_progressive)
    dec = batch_decoder(G, dlib)
    dec.set_batch_chunk(chunk)
    n, nprog = len(prog), sum(prog)
    for rep in range(3):
        got, _ = dec.decode_batch(streams)
        assert same(got, wanted(first_progressive)), rep
        group = group_of(prog, rep, first_progressive)
        batched, single = dec.last_batch()
        if first_progressive and rep == 0:  # (a progressive frame 0 leaves no header to launch on: the baseline frames go single, the group is batched)
            assert (batched, single) == (len(group), n - len(group)), (rep, batched, single)
        else:  # (frame 0 ahead, single; every other baseline frame and the group batched)
            assert (batched, single) == (n - 1, 1), (rep, batched, single)
        assert len(group) == nprog - (1 if first_progressive else 0)
        assert dec.progressive_batch_stats() == stats_of(plans, group, chunk), rep
    dec.close()


def test_device_buffers_take_frame_0_into_the_group(O, G, dlib):
    """streams and pixels in device memory, a decoder that has a header cached: in a call with baseline frames no frame goes ahead and a progressive
    frame 0 is of the group; the group's frames of an all-progressive call lie a constant distance apart in the output (no staging)"""
    L = dlib.L
    L.gj_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.gj_hip_free.argtypes = [C.c_void_p]
    for first_progressive, only in ((True, False), (True, True)):
        streams, twins, prog, plans = mixed_set(first_progressive)
        want = wanted(first_progressive)
        if only:
            keep = [f for f, p in enumerate(prog) if p]
            streams, want, plans, prog = [streams[f] for f in keep], [want[f] for f in keep], [plans[f] for f in keep], [True] * len(keep)
        n, raw = len(streams), want[0].size
        sizes = [int(s.size) for s in streams]
        in_stride = (max(sizes) + 64 + 15) & ~15
        buf = np.zeros(in_stride * n, np.uint8)
        for i, s in enumerate(streams):
            buf[i * in_stride:i * in_stride + s.size] = s
        d_in, d_out = device_copy(dlib, buf), device_copy(dlib, np.zeros(raw * n, np.uint8))
        dec = batch_decoder(G, dlib)
        base = mixed_set(False)[0][0]
        assert np.array_equal(dec.decode(base)[0], O.decode(base)[0])  # (caches the baseline header)
        for rep in range(2):
            dec.decode_batch(None, device_out=d_out, out_stride=raw, device_in=d_in, in_stride=in_stride, sizes=sizes)
            out = np.empty(raw * n, np.uint8)
            assert L.gj_hip_memcpy_d2h(out.ctypes.data, d_out, out.size, None) == 0 and L.gj_hip_stream_sync(None) == 0
            assert same([out[f * raw:(f + 1) * raw] for f in range(n)], want), (only, rep)
            # (not one frame of an all-progressive call passes the launches on the cached header: a stale cache, frame 0 goes ahead as ever)
            assert dec.last_batch() == ((n - 1, 1) if only else (n, 0)), (only, rep)
            group = [f for f, p in enumerate(prog) if p and not (only and f == 0)]
            assert dec.progressive_batch_stats() == stats_of(plans, group, 0), (only, rep)
        dec.close()
        L.gj_hip_free(d_in)
        L.gj_hip_free(d_out)


# ================================================================================================ 2. several groups
def test_two_groups_in_one_call(O, G, dlib):
    """quality 90 and quality 50 differ in their quantisation tables: two groups of two; a 4:4:4 stream of the same size is alone and goes single"""
    import oracle as O2
    a = [progressive(s, P.LIBJPEG_COLOUR, restart=s % 2) for s in (11, 12)]
    b = [progressive(s, P.deep_approximation(3), quality=50) for s in (13, 14)]
    img = O2.make_image(BW, BH, pixel_format=1, color_space=1, quality=90, restart_interval=0, interleaved=1, subsampling=None)
    coefs = P.legal(img, SS.sparse(img, seed=15, density=0.3), P.LIBJPEG_COLOUR)
    lone = (P.write(img, coefs, P.LIBJPEG_COLOUR), O2.encode_from_coefs(img, coefs))
    order = [baseline(1), a[0], b[0], lone, a[1], b[1]]
    streams = [x if isinstance(x, np.ndarray) else x[0] for x in order]
    twins = [x if isinstance(x, np.ndarray) else x[1] for x in order]
    want = [O.decode(t)[0] for t in twins]
    dec = batch_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch(streams)
        assert same(got, want), rep
        assert dec.last_batch() == (4, 2), rep  # (frame 0 ahead and the lone 4:4:4 stream)
        rc, frames, groups, launches, records = dec.progressive_batch_stats()
        levels = max(P.levels_of(P.LIBJPEG_COLOUR)) + 1 + max(P.levels_of(P.deep_approximation(3))) + 1
        assert (rc, frames, groups, launches) == (0, 4, 2, levels), rep
        assert records == sum(P.segment_count(image(), x[2], x[3]) for x in a + b), rep
        assert dec.progressive_stats()[1:3] == (1, 10)  # (the last single-frame decode inside the call: the lone stream, ten scans)
    dec.close()


# ================================================================================================ 3. long scans
@pytest.mark.parametrize("chunk", [1, 0])
def test_refill_and_look_ahead(O, G, dlib, chunk):
    """322 x 242 without restart markers: every scan is one segment of several KB (the 1 KiB stage is refilled), a DC scan stores more than 64 blocks
    and the refinement scans load several 32-block look-aheads"""
    cases = [case("420_322x242", kind="refinement_runs"), case("420_322x242", kind="with_big")]
    assert all(max(n for _, n in P.scan_data_ranges(c[0])) > 1024 for c in cases)
    streams = [baseline(1, 322, 242)] + [c[0] for c in cases]
    want = [O.decode(t)[0] for t in [streams[0]] + [c[1] for c in cases]]
    dec = batch_decoder(G, dlib)
    dec.set_batch_chunk(chunk)
    got, _ = dec.decode_batch(streams)
    assert same(got, want)
    assert dec.last_batch() == (2, 1)
    levels = max(P.levels_of(cases[0][3])) + 1
    assert dec.progressive_batch_stats() == (0, 2, 1, levels * (2 if chunk == 1 else 1), 2 * len(cases[0][3]))
    dec.close()


# ================================================================================================ 4. every call form
RECTS = [(1, 2, 40, 31), (0, 0, BW, BH), (7, 3, 19, 29), (3, 1, 36, 36), (13, 6, 50, 40), (2, 2, 8, 8), (21, 9, 33, 17), (5, 5, 58, 42)]
ORIGINS = [(1, 3), (39, 33), (7, 5), (13, 1), (40, 34), (3, 17), (21, 9), (0, 0)]
MIRROR = [0, 1, 1, 0, 1, 0, 0, 1]
OW, OH = 12, 8


def both_ways(G, dlib, call, options=()):
    """the call on a decoder with the option on and on one with it off -> ((result, region_stats, last_batch) of each, progressive_batch_stats of `on`)"""
    out = []
    for setting in ("on", "off"):
        dec = prog_decoder(G, dlib)
        assert dec.set_option(OPT, setting) == 0
        for k, v in options:
            assert dec.set_option(k, v) == 0
        call(dec)  # (the first call of a decoder: its frame 0 caches the header the later ones launch on)
        got = call(dec)
        out.append((got, dec.region_stats(), dec.last_batch(), dec.progressive_batch_stats()))
        dec.close()
    return out


@pytest.mark.parametrize("form", ["scale", "regions", "crop_resize", "prescale", "antialias"])
def test_call_forms(O, G, dlib, form):
    streams, twins, prog, plans = mixed_set(False)
    n = len(streams)
    options = ()
    if form == "scale":
        options = (("dec_opt_scale", "1/2"),)
        call = lambda dec: dec.decode_batch(streams)[0]  # noqa: E731
        want = [reduced(O, t, -1, -1, 2)[0] for t in twins]
    elif form == "regions":
        call = lambda dec: dec.decode_batch_regions(streams, ORIGINS, 24, 14)[0]  # noqa: E731
        want = oracle_crops(O, twins, ORIGINS, 24, 14)
    else:
        call = lambda dec: dec.decode_batch_crop_resize(streams, RECTS, OW, OH, mirror=MIRROR)[0]  # noqa: E731
        if form == "crop_resize":
            want = resized(O, twins, RECTS, OW, OH, mirror=MIRROR)
        elif form == "prescale":
            from test_crop_resize_prescale_subsampled import expected as prescaled
            options = (("dec_opt_resize_prescale", "1/2"), ("dec_opt_resize_prescale_subsampled", "on"))
            want = prescaled(O, twins, RECTS, OW, OH, 2, mirror=MIRROR)[0]
        else:
            from test_crop_resize_antialias import aa_expected as antialiased
            options = (("dec_opt_resize_filter", "antialias"),)
            want = antialiased(O, twins, RECTS, OW, OH, mirror=MIRROR)
    on, off = both_ways(G, dlib, call, options)
    assert same(on[0], off[0]) and same(on[0], want), form
    if form != "scale":  # (gpujpeg_amd_decoder_get_region_stats after a call with rectangles: the same four numbers, mode 2 with a progressive frame)
        assert on[1] == off[1] and on[1][0] == 2, (form, on[1], off[1])
    assert off[2] == (n - sum(prog) - 1, sum(prog) + 1) and on[2] == (n - 1, 1), (form, on[2], off[2])
    assert on[3] == stats_of(plans, group_of(prog, 1, False), 0) and off[3] == (-1, 0, 0, 0, 0), (form, on[3])


def test_tensor_call(O, G, dlib):
    """frame f of the batched tensor call is, bit for bit, the single call on stream f and on its twin"""
    streams, twins, prog, plans = mixed_set(False)
    scale, bias = [1 / 255.0] * 3, [-0.5, 0.0, 0.25]
    dec = batch_decoder(G, dlib)
    for rep in range(2):
        ten, _ = dec.decode_batch_crop_resize_tensor(streams, RECTS, OW, OH, G.TENSOR_F16, G.TENSOR_CHW, scale, bias, mirror=MIRROR)
        assert dec.last_batch() == (len(streams) - 1, 1), rep
        assert dec.progressive_batch_stats() == stats_of(plans, group_of(prog, rep, False), 0), rep
    one = prog_decoder(G, dlib)
    for f in range(len(streams)):
        a, _ = one.decode_batch_crop_resize_tensor([streams[f]], [RECTS[f]], OW, OH, G.TENSOR_F16, G.TENSOR_CHW, scale, bias, mirror=[MIRROR[f]])
        b, _ = one.decode_batch_crop_resize_tensor([twins[f]], [RECTS[f]], OW, OH, G.TENSOR_F16, G.TENSOR_CHW, scale, bias, mirror=[MIRROR[f]])
        assert np.array_equal(np.asarray(ten[f]).view(np.uint16), np.asarray(a[0]).view(np.uint16)), f
        assert np.array_equal(np.asarray(a[0]).view(np.uint16), np.asarray(b[0]).view(np.uint16)), f
    assert one.progressive_batch_stats() == (-1, 0, 0, 0, 0)
    one.close()
    dec.close()


def test_a_refused_rectangle_names_its_frame_and_writes_nothing(O, G, dlib, capfd):
    streams, twins, prog, _ = mixed_set(False)
    dec = batch_decoder(G, dlib)
    dec.decode_batch_regions(streams, ORIGINS, 24, 14)
    bad = list(ORIGINS)
    bad[4] = (BW - 10, 3)  # (frame 4 is progressive: 24 pixels from x = 54 leave the 64 x 48 image)
    with pytest.raises(RuntimeError):
        dec.decode_batch_regions(streams, bad, 24, 14)
    assert "Frame 4 of the batch" in capfd.readouterr().err
    got, _ = dec.decode_batch_regions(streams, ORIGINS, 24, 14)
    assert same(got, oracle_crops(O, twins, ORIGINS, 24, 14))
    dec.close()


# ================================================================================================ 5. dec_opt_batch_sizes = mixed
def test_mixed_sizes_group_by_size(O, G, dlib):
    """progressive streams of two sizes, two of each: two groups; a third size alone goes single (per-frame geometry inside one set of progressive
    launches is not built)"""
    a = [progressive(s, P.LIBJPEG_COLOUR, restart=s % 3) for s in (21, 22)]
    b = [progressive(s, P.chroma_first(), w=40, h=56) for s in (23, 24)]
    lone = progressive(25, P.LIBJPEG_COLOUR, w=56, h=24)
    order = [baseline(1), a[0], b[0], lone, b[1], a[1], baseline(2, 48, 32)]
    streams = [x if isinstance(x, np.ndarray) else x[0] for x in order]
    twins = [x if isinstance(x, np.ndarray) else x[1] for x in order]
    rects = [(1, 2, 40, 31), (0, 0, BW, BH), (7, 3, 19, 29), (3, 1, 36, 20), (13, 6, 25, 40), (2, 2, 8, 8), (2, 1, 40, 30)]
    want = resized(O, twins, rects, OW, OH)
    dec = batch_decoder(G, dlib)
    assert dec.set_option("dec_opt_batch_sizes", "mixed") == 0
    for rep in range(2):
        got, _ = dec.decode_batch_crop_resize(streams, rects, OW, OH)
        assert same(got, want), rep
        assert dec.last_batch() == (5, 2), rep  # (frame 0 ahead and the lone size single; the other baseline frame is of frame 0's family)
        rc, frames, groups, launches, records = dec.progressive_batch_stats()
        assert (rc, frames, groups) == (0, 4, 2), rep
        assert launches == max(P.levels_of(P.LIBJPEG_COLOUR)) + 1 + max(P.levels_of(P.chroma_first())) + 1
    dec.close()


# ================================================================================================ 6. files written by libjpeg
NAMES = ["gradient", "rings", "blocks"]


def test_libjpeg_files_form_one_group(O, G, dlib):
    prog = [np.fromfile(os.path.join(GOLDEN, n + "_progressive.jpg"), np.uint8) for n in NAMES]
    twin = [np.fromfile(os.path.join(GOLDEN, n + "_baseline.jpg"), np.uint8) for n in NAMES]
    assert all(p.size < 8192 for p in prog + twin)
    heads = [bytes(p[:bytes(p).index(b"\xff\xda")]) for p in prog]
    assert len(set(heads)) == 3  # (optimised tables: no two headers are byte-equal)
    infos = [G.stream_info(dlib, p) for p in prog]
    assert all(i[:6] == (83, 131, 3, 1, 10, 3) and i[7] == 0 for i in infos)
    want = [O.decode(t)[0] for t in twin]
    dec = batch_decoder(G, dlib)
    got, _ = dec.decode_batch([twin[0]] + prog)  # (a baseline frame 0 goes ahead: the three files are the candidates)
    assert same(got, [want[0]] + want)
    assert dec.last_batch() == (3, 1)
    assert dec.progressive_batch_stats() == (0, 3, 1, 3, 30)  # (ten scans each without restart markers: 30 waves in 3 launches)
    got, _ = dec.decode_batch(prog)  # (a progressive frame 0 ahead: a group of two)
    assert same(got, want)
    assert dec.last_batch() == (2, 1) and dec.progressive_batch_stats() == (0, 2, 1, 3, 20)
    dec.close()


# ================================================================================================ 7. the option and the routing
def test_option_off_and_routing(O, G, dlib, capfd):
    streams, twins, prog, plans = mixed_set(False)
    n, nprog = len(prog), sum(prog)
    want = wanted(False)
    dec = prog_decoder(G, dlib)
    assert dec.progressive_batch_stats() == (-1, 0, 0, 0, 0)
    for setting in (None, "off"):  # what test_progressive_decode.py pins: the progressive frames are single
        if setting:
            assert dec.set_option(OPT, setting) == 0
        for rep in range(2):
            got, _ = dec.decode_batch(streams)
            assert same(got, want)
            assert dec.last_batch() == (n - nprog - 1, nprog + 1)
            assert dec.progressive_batch_stats() == (-1, 0, 0, 0, 0)
    assert dec.set_option(OPT, "on") == 0
    assert dec.set_option(OPT, "maybe") != 0 and dec.set_option(OPT, "ON") != 0  # refused, and the setting stays
    assert "Unknown value maybe for dec_opt_batch_progressive" in capfd.readouterr().err
    got, _ = dec.decode_batch(streams)
    assert same(got, want) and dec.last_batch() == (n - 1, 1)
    assert dec.progressive_batch_stats() == stats_of(plans, group_of(prog, 1, False), 0)
    px, _ = dec.decode(streams[1])  # (any other call: the getter says so)
    assert np.array_equal(px, want[1]) and dec.progressive_batch_stats() == (-1, 0, 0, 0, 0)
    dec.keep_coefficients(True)  # (a state in which the batched launches decline: every frame single)
    got, _ = dec.decode_batch(streams)
    assert same(got, want) and dec.last_batch() == (0, n)
    assert dec.progressive_batch_stats() == (0, 0, 0, 0, 0)
    dec.keep_coefficients(False)
    got, _ = dec.decode_batch(streams)
    assert same(got, want) and dec.last_batch() == (n - 1, 1)
    assert dec.set_option("dec_opt_progressive", "off") == 0  # (the reader refuses SOF2 again: the call fails as ever)
    capfd.readouterr()
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        dec.decode_batch(streams)
    assert "Marker SOF2 (Progressive with Huffman coding) is not supported!" in capfd.readouterr().err
    assert dec.progressive_batch_stats() == (-1, 0, 0, 0, 0)
    dec.close()
    assert G.DEC_OPT_BATCH_PROGRESSIVE == OPT and (G.BATCH_PROGRESSIVE_OFF, G.BATCH_PROGRESSIVE_ON) == ("off", "on")


def test_a_group_of_one_goes_single(O, G, dlib):
    streams, twins = [baseline(1), progressive(4, P.LIBJPEG_COLOUR)[0], baseline(2)], None
    twins = [streams[0], progressive(4, P.LIBJPEG_COLOUR)[1], streams[2]]
    dec = batch_decoder(G, dlib)
    for rep in range(2):
        got, _ = dec.decode_batch(streams)
        assert same(got, [O.decode(t)[0] for t in twins])
        assert dec.last_batch() == (1, 2) and dec.progressive_batch_stats() == (0, 0, 0, 0, 0)
        assert dec.progressive_stats()[1] == 1
    dec.close()


# ================================================================================================ 8. what the pass leaves behind
def test_the_header_cache_survives_a_group_call(O, G, dlib):
    """a progressive-group call, a baseline batch call, the group call again: the baseline call launches on its cached header -- path counters and
    counts as in the same sequence without the group calls --, and every byte is right throughout"""
    base = [baseline(s) for s in (1, 2, 3, 4)]
    streams, twins, prog, plans = mixed_set(False)
    want_base, want = [O.decode(b)[0] for b in base], wanted(False)

    def run(with_groups):
        dec = batch_decoder(G, dlib)
        seen = []
        for rep in range(2):
            if with_groups:
                got, _ = dec.decode_batch(streams)
                assert same(got, want), rep
                assert dec.progressive_batch_stats()[1] == sum(prog)
            else:  # (the same call without its progressive frames: what it leaves cached is what the group call must leave)
                got, _ = dec.decode_batch([s for s, p in zip(streams, prog) if not p])
            got, _ = dec.decode_batch(base)
            assert same(got, want_base), rep
            seen.append((dec.last_batch(), dec.path_counters()))
        dec.close()
        return seen

    a, b = run(True), run(False)
    assert a == b, (a, b)
    assert a[-1][0] == (3, 1)  # (frame 0 ahead on the cached header, the three others batched)


# ================================================================================================ 9. damaged streams (CPU tier only)
def damaged(kind):
    good = progressive(31, P.LIBJPEG_COLOUR, restart=0)[0]
    d = bytearray(good.tobytes())
    ranges = P.scan_data_ranges(good)
    if kind == "flip":
        start, length = ranges[4]
        at = start + length // 2
        d[at] = (d[at] ^ 0x5A) if (d[at] ^ 0x5A) != 0xFF and d[at - 1] != 0xFF else d[at] ^ 0x12
    elif kind == "truncated":
        start, length = ranges[3]
        d = d[:start + length // 2]
    else:  # an SOS with an illegal Ah / Al: the refinement scan 5 says Ah = 3 where the coefficients were last coded with Al = 2
        sos = [i for i in range(len(d) - 1) if d[i] == 0xFF and d[i + 1] == 0xDA and any(abs(i + 2 + ((d[i + 2] << 8) | d[i + 3]) - s) == 0 for s, _ in ranges)]
        at = sos[5]
        n = (d[at + 2] << 8) | d[at + 3]
        d[at + 2 + n - 1] = 0x32
    return np.frombuffer(bytes(d), np.uint8).copy()


@pytest.mark.parametrize("kind", ["flip", "truncated", "sos"])
def test_a_damaged_stream_in_a_group_of_three(O, G, emu, kind):
    """pixels wanted in DEVICE memory, every slot followed by a guard band: the call returns what the option-off call returns; where it succeeds every
    frame's bytes -- the damaged frame's too -- are the option-off call's and the good frames are their twins' images; and whatever the call returns,
    the guard bands behind the slots, read back from the device, are untouched: no stage of the batched launches writes past its frame's slot"""
    L = emu.L
    L.gj_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.gj_hip_free.argtypes = [C.c_void_p]
    good = [progressive(s, P.LIBJPEG_COLOUR, restart=s % 2) for s in (32, 33)]
    streams = [baseline(1), good[0][0], damaged(kind), good[1][0]]
    want = [O.decode(t)[0] for t in (streams[0], good[0][1], good[1][1])]
    raw, n = want[0].size, len(streams)
    sizes = [int(s.size) for s in streams]
    in_stride = (max(sizes) + 64 + 15) & ~15
    buf = np.zeros(in_stride * n, np.uint8)
    for i, s in enumerate(streams):
        buf[i * in_stride:i * in_stride + s.size] = s
    GUARD = 512
    slot = raw + GUARD
    results = []
    for setting in ("on", "off"):
        dec = prog_decoder(G, emu)
        assert dec.set_option(OPT, setting) == 0
        assert np.array_equal(dec.decode(streams[0])[0], want[0])  # (caches the baseline header: no frame goes ahead)
        d_out = device_copy(emu, np.full(slot * n, 0x5A, np.uint8))
        pi = G.ImageParameters()
        rc = L.gpujpeg_amd_decoder_decode_batch(dec.h, buf.ctypes.data, in_stride, (C.c_size_t * n)(*sizes), n, C.c_void_p(d_out), slot, C.byref(pi))
        out = np.empty(slot * n, np.uint8)
        assert L.gj_hip_memcpy_d2h(out.ctypes.data, d_out, out.size, None) == 0 and L.gj_hip_stream_sync(None) == 0
        L.gj_hip_free(d_out)
        frames = [out[f * slot:f * slot + raw].copy() for f in range(n)]
        assert all(np.all(out[f * slot + raw:(f + 1) * slot] == 0x5A) for f in range(n)), "the guard bands behind the slots, in device memory"
        results.append((rc, frames, dec.last_batch()))
        got, _ = dec.decode_batch([streams[0], good[0][0], good[1][0]])  # (the decoder goes on)
        assert same(got, want), (kind, setting)
        dec.close()
    (rc_on, on, count_on), (rc_off, off, count_off) = results
    assert rc_on == rc_off, (kind, rc_on, rc_off)
    if rc_on == 0:
        assert same(on, off), kind
        assert same([on[0], on[1], on[3]], want), kind
        assert count_on[0] >= 3 and count_off == (1, 3), (kind, count_on, count_off)  # (frame 0 on its cached header; with the option, the group too)
    else:  # (a failed call: the baseline launches have run over every slot, as ever, and only what was accepted before the failure is an image)
        assert np.array_equal(on[0], want[0]) and np.array_equal(off[0], want[0]), kind
