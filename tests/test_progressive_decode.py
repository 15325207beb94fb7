"""Progressive (SOF2) streams, dec_opt_progressive = on (gpujpeg_amd_ext.h): the decoder returns the image of the stream's BASELINE TWIN.

The streams come from the Python writer of progressive_streams.py -- chosen coefficients, chosen scan script, tables and slots -- whose twin is
O.encode_from_coefs of the same coefficients, and from libjpeg (tests/golden/progressive/, written through PIL by make_progressive_fixtures.py: the
baseline save of the same picture is the twin), so that the writer and the kernel cannot share one misreading of ITU T.81 Annex G. Expected bytes
never come from the product: pixels are the oracle's decode of the twin, coefficients the ones put in, reduced images expected() of
test_scaled_decode.py, regions the cropped oracle decode of test_region_batch.py, crop-and-resize expected() of test_crop_resize.py. Every
comparison is byte for byte.

Two tiers with the same bodies, like test_batch_restartless.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. Damaged streams run on the CPU tier only: nothing damaged is sent to a GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import progressive_streams as P
import synth_streams as SS
from test_crop_resize import expected as resized
from test_region_batch import dlib, emu, new_decoder, oracle_crops, same  # noqa: F401  (emu, dlib: the fixtures of the two tiers)
from test_scaled_decode import expected as reduced

OPT = "dec_opt_progressive"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive")
S420, S422 = [(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)]
# name: (width, height, oracle pixel format, colour space, subsampling) -- the smallest that reach each rule of the geometry
GEOMS = {
    "grey_8x8": (8, 8, 0, 3, None),             # one block
    "grey_17x9": (17, 9, 0, 3, None),
    "444_24x16": (24, 16, 1, 1, None),
    "420_33x17": (33, 17, 1, 1, S420),          # luminance: 5 x 3 coded blocks in a 6 x 4 plane; chrominance 17 x 9 samples: 3 x 2 coded blocks
    "422_35x13": (35, 13, 1, 1, S422),
    "4444_16x16": (16, 16, 6, 1, [(1, 1)] * 4),
    "420_322x242": (322, 242, 1, 1, S420),      # several restart segments per scan
    "grey_2048x1032": (2048, 1032, 0, 3, None),  # 33024 blocks: an EOB run of 32767 is followed by another
}
PF_RGB, PF_420, PF_U8 = 1, 5, 0
FORMATS = {1: ((PF_RGB, 1), (PF_420, 3), (PF_U8, 3)), 3: ((PF_RGB, 1), (PF_420, 3), (PF_U8, 3)), 4: ((PF_RGB, 1), (PF_420, 3), (PF_U8, 3))}


@functools.lru_cache(maxsize=None)
def image_of(geom):
    import oracle as O
    w, h, pf, cs, ss = GEOMS[geom]
    return O.make_image(w, h, pixel_format=pf, color_space=cs, quality=90, restart_interval=0, interleaved=1 if pf else 0, subsampling=ss)


def refinement_runs(img, seed=0):
    """coefficients that make the refinement scans pass non-zero-history coefficients inside runs of 16 and more: large values (history after the first
    scans) at every third position, +-1 (new in the last scan) only at position 60"""
    rng = np.random.default_rng(seed)
    n = int(img.data_size) // 64
    Z = np.zeros((n, 64), np.int16)
    Z[:, 0] = rng.integers(-200, 200, n)
    Z[:, 3:58:3] = rng.integers(4, 40, (n, 19)) * rng.choice([-1, 1], (n, 19))
    Z[::2, 60] = rng.choice([-1, 1], (n + 1) // 2)
    Z[1::4, 3:58:3] = 0  # (and blocks where the run is free of history)
    return SS.to_planes(Z)


def coefficients(geom, kind, seed=0):
    img = image_of(geom)
    n = int(img.data_size)
    if kind == "sparse":
        return SS.sparse(img, seed=seed)
    if kind == "with_big":
        return SS.dc_extremes(SS.with_big(SS.sparse(img, seed=seed, density=0.2), max(8, n // 256), seed=seed))
    if kind == "dense":
        rng = np.random.default_rng(seed)
        return (rng.integers(1, 90, n) * rng.choice([-1, 1], n)).astype(np.int16)
    if kind == "zero":
        return np.zeros(n, np.int16)
    if kind == "zero_ac":
        Z = np.zeros((n // 64, 64), np.int16)
        Z[:, 0] = np.random.default_rng(seed).integers(-300, 300, n // 64)
        return SS.to_planes(Z)
    if kind == "refinement_runs":
        return refinement_runs(img, seed)
    raise KeyError(kind)


def script_of(name, n):
    return {"default": P.default_script, "spectral": P.spectral_only, "one_ac": P.one_ac_scan, "deep": P.deep_approximation, "dc_each": P.dc_per_component,
            "dc_chroma": lambda _: P.dc_chroma_together(), "chroma_first": lambda _: P.chroma_first(), "band63": P.single_coefficient_band}[name](n)


@functools.lru_cache(maxsize=None)
def case(geom, script="default", kind="sparse", restart=0, tables="per_scan", slots="by_scan", upto=None):
    """-> (progressive stream, twin, coefficients, script as written, restart interval); read-only arrays, one per process for both tiers"""
    import oracle as O
    img = image_of(geom)
    sc = script_of(script, img.comp_count)
    coefs = P.legal(img, coefficients(geom, kind), sc)
    jpeg = P.write(img, coefs, sc, restart=restart, tables=tables, slots=slots, upto=upto)
    shown = coefs
    if upto is not None:  # a prefix of the script is an image: the coefficients as far as its scans have told them
        shown = prefix_coefficients(img, coefs, sc[:upto])
    twin = O.encode_from_coefs(img, shown)
    for a in (jpeg, twin, shown):
        a.setflags(write=False)
    return jpeg, twin, shown, sc[:upto], restart


def prefix_coefficients(img, coefs, scans):
    """what a decoder holds after `scans`: per coefficient the bits down to the lowest Al coded so far (magnitudes for AC, the value for DC)"""
    Z = SS.zigzag_blocks(coefs).astype(np.int32)
    out = np.zeros_like(Z)
    for comps, ss, se, ah, al in scans:
        for c in comps:
            h, v, bx, by, cbx, cby, first = P.frame_of(img)[0][c]
            rows = np.arange(first, first + bx * by).reshape(by, bx)
            rows = (rows if len(comps) > 1 else rows[:cby, :cbx]).reshape(-1)
            band = Z[rows, ss:se + 1]
            out[rows, ss:se + 1] = (band >> al) << al if ss == 0 else np.sign(band) * ((np.abs(band) >> al) << al)
    return SS.to_planes(out.astype(np.int16))


def prog_decoder(G, lib, pf=None, cs=None, align=None):
    dec = new_decoder(G, lib, pf, cs, align)
    assert dec.set_option(OPT, "on") == 0
    return dec


def check(O, G, lib, geom, **kw):
    """the contract of one stream: coefficients, pixels in every format asked for, the two stats calls"""
    jpeg, twin, coefs, script, restart = case(geom, **kw)
    img = image_of(geom)
    dec = prog_decoder(G, lib)
    dec.keep_coefficients(True)
    px, pi = dec.decode(jpeg)
    assert np.array_equal(dec.coefficients(int(img.data_size)), coefs), (geom, kw)
    want, wimg = O.decode(twin)
    assert px.size == want.size and np.array_equal(px, want), (geom, kw)
    assert (pi.width, pi.height, pi.pixel_format) == (wimg.width, wimg.height, wimg.pixel_format)
    levels = max(P.levels_of(script)) + 1
    segments = P.segment_count(img, script, restart)
    assert dec.progressive_stats() == (0, 1, len(script), levels, segments), (geom, kw)
    assert G.stream_info(lib, jpeg) == (img.width, img.height, img.comp_count, 1, len(script), levels, restart, 0), (geom, kw)
    dec.close()
    for pf, cs in FORMATS[img.comp_count]:  # packed RGB, planar 4:2:0 and grey
        dec = prog_decoder(G, lib, pf, cs)
        px, _ = dec.decode(jpeg)
        want, _ = O.decode(twin, pf, cs)
        assert px.size == want.size and np.array_equal(px, want), (geom, kw, pf, cs)
        dec.close()


# ================================================================================================ 1. scripts and geometries
@pytest.mark.parametrize("geom", ["grey_8x8", "grey_17x9", "444_24x16", "420_33x17", "422_35x13", "4444_16x16", "420_322x242"])
def test_libjpeg_script_on_every_geometry(O, G, dlib, geom):
    n = image_of(geom).comp_count
    if n == 3:
        assert script_of("default", 3) is P.LIBJPEG_COLOUR and P.levels_of(P.LIBJPEG_COLOUR) == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]
    if n == 1:
        assert script_of("default", 1) == P.LIBJPEG_GREY and max(P.levels_of(P.LIBJPEG_GREY)) == 2
    check(O, G, dlib, geom, kind="with_big")


@pytest.mark.parametrize("geom", ["grey_17x9", "420_33x17", "4444_16x16"])
@pytest.mark.parametrize("script", ["spectral", "one_ac", "deep", "dc_each", "band63"])
def test_scripts(O, G, dlib, geom, script):
    check(O, G, dlib, geom, script=script, kind="with_big")


@pytest.mark.parametrize("geom", ["444_24x16", "420_33x17", "422_35x13"])
@pytest.mark.parametrize("script", ["dc_chroma", "chroma_first"])
def test_component_subsets_and_orders(O, G, dlib, geom, script):
    check(O, G, dlib, geom, script=script, kind="with_big")


@pytest.mark.parametrize("geom", ["grey_17x9", "420_33x17"])
@pytest.mark.parametrize("kind", ["sparse", "dense", "zero", "refinement_runs"])
def test_coefficient_patterns(O, G, dlib, geom, kind):
    check(O, G, dlib, geom, kind=kind)
    check(O, G, dlib, geom, kind=kind, script="deep")


def test_zrl_inside_refinement_is_what_the_pattern_reaches():
    """the pattern's last scan does code runs of 16 and more that pass coefficients with history (symbol 0xF0 in a refinement scan)"""
    img = image_of("grey_17x9")
    sc = P.LIBJPEG_GREY
    Z = SS.zigzag_blocks(P.legal(img, coefficients("grey_17x9", "refinement_runs"), sc))
    segs = P.scan_symbols_of(img, Z, sc[-1], 0)
    assert any(b < 0 and a == 0xF0 for seg in segs for a, b in seg)


def test_one_eob_run_follows_another(O, G, dlib):
    """grey 2048 x 1032 with zero AC: 33024 blocks, an EOB run of 32767 and the next"""
    check(O, G, dlib, "grey_2048x1032", kind="zero_ac")


@pytest.mark.parametrize("restart", [1, 3])
@pytest.mark.parametrize("script", ["default", "dc_each"])
def test_restart_intervals_count_mcus_or_blocks(O, G, dlib, restart, script):
    check(O, G, dlib, "420_33x17", script=script, kind="with_big", restart=restart)


def test_several_restart_segments_per_scan(O, G, dlib):
    check(O, G, dlib, "420_322x242", kind="with_big", restart=7)


@pytest.mark.parametrize("upto", range(1, 10))
def test_a_prefix_of_the_script_is_an_image(O, G, dlib, upto):
    check(O, G, dlib, "420_33x17", kind="with_big", upto=upto)


@pytest.mark.parametrize("tables,slots", [("up_front", "by_scan"), ("per_scan", 0), ("per_scan", 3), ("up_front", 2)])
def test_tables_and_slots(O, G, dlib, tables, slots):
    check(O, G, dlib, "420_33x17", kind="with_big", tables=tables, slots=slots)
    check(O, G, dlib, "grey_17x9", kind="dense", tables=tables, slots=slots)


# ================================================================================================ 2. the options behind the planes
@pytest.mark.parametrize("geom", ["420_33x17", "444_24x16"])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_scale(O, G, dlib, geom, s):
    jpeg, twin = case(geom, kind="with_big")[:2]
    want, _ = reduced(O, twin, -1, -1, s)
    dec = prog_decoder(G, dlib)
    assert dec.set_option("dec_opt_scale", f"1/{s}") == 0
    px, _ = dec.decode(jpeg)
    assert px.size == want.size and np.array_equal(px, want)
    dec.close()


@pytest.mark.parametrize("geom", ["420_33x17", "444_24x16"])
def test_region(O, G, dlib, geom):
    jpeg, twin = case(geom, kind="with_big")[:2]
    w, h = GEOMS[geom][:2]
    dec = prog_decoder(G, dlib)
    for x, y, rw, rh in ((5, 3, 11, 7), (w - 9, h - 6, 9, 6), (w // 2, h // 2, 1, 1)):
        assert dec.set_option("dec_opt_region", f"{x},{y},{rw},{rh}") == 0
        px, _ = dec.decode(jpeg)
        assert same([px], oracle_crops(O, [twin], [(x, y)], rw, rh)), (x, y, rw, rh)
        assert dec.region_stats()[0] == 2
    dec.close()


# ================================================================================================ 3. batch calls
BW, BH = 64, 48


@functools.lru_cache(maxsize=None)
def batch_set(first_progressive=False, mixed=False):
    """-> (streams, the streams whose oracle decode is expected, progressive flags). Baseline streams of ONE header WITH a restart interval (2 MCUs), so
    that the batched launches take them, and progressive streams of the same geometry between them; mixed: also a baseline stream of the family at
    another size and a progressive stream of another size"""
    import oracle as O

    def baseline(w, h, seed):
        img = O.make_image(w, h, pixel_format=1, color_space=1, quality=90, restart_interval=2, interleaved=1, subsampling=S420)
        return O.encode_from_coefs(img, P.legal(img, SS.sparse(img, seed=seed, density=0.3)))

    def progressive(w, h, seed, script):
        img = O.make_image(w, h, pixel_format=1, color_space=1, quality=90, restart_interval=0, interleaved=1, subsampling=S420)
        coefs = P.legal(img, SS.with_big(SS.sparse(img, seed=seed, density=0.3), 20, seed=seed), script)
        return P.write(img, coefs, script, restart=seed % 3), O.encode_from_coefs(img, coefs)

    B = [baseline(BW, BH, s) for s in (1, 2, 3)]
    Pg = [progressive(BW, BH, 4, P.LIBJPEG_COLOUR), progressive(BW, BH, 5, P.deep_approximation(3)), progressive(BW, BH, 6, P.chroma_first())]
    order = [("P", 0), ("B", 0), ("B", 1), ("P", 1), ("B", 2), ("P", 2)] if first_progressive else [("B", 0), ("P", 0), ("B", 1), ("P", 1), ("P", 2), ("B", 2)]
    streams = [B[i] if k == "B" else Pg[i][0] for k, i in order]
    twins = [B[i] if k == "B" else Pg[i][1] for k, i in order]
    prog = [k == "P" for k, _ in order]
    if mixed:
        other = progressive(40, 56, 7, P.LIBJPEG_COLOUR)
        streams, twins, prog = streams + [baseline(48, 32, 8), other[0]], twins + [baseline(48, 32, 8), other[1]], prog + [False, True]
    return streams, twins, prog


def counted(dec, prog, rep, first_progressive):
    """the batched launches took the baseline frames, the progressive ones went the single-frame route: with pixels wanted in host memory frame 0 goes
    ahead of the launches (single whatever it is), and a progressive frame 0 leaves no header to launch on in the first call"""
    batched, single = dec.last_batch()
    nprog, n = sum(prog), len(prog)
    if first_progressive and rep == 0:
        assert (batched, single) == (0, n), (rep, batched, single)
    else:
        ahead = 0 if prog[0] else 1
        assert batched > 0 and single == nprog + ahead and batched == n - nprog - ahead, (rep, batched, single)


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("first_progressive", [False, True])
def test_decode_batch_mixes_baseline_and_progressive(O, G, dlib, first_progressive, chunk):
    """(chunk 2: the baseline frames behind the progressive ones take several sets of launches)"""
    streams, twins, prog = batch_set(first_progressive)
    dec = prog_decoder(G, dlib)
    dec.set_batch_chunk(chunk)
    for rep in range(3):
        got, _ = dec.decode_batch(streams)
        assert same(got, [O.decode(t)[0] for t in twins]), rep
        counted(dec, prog, rep, first_progressive)
    dec.close()


@pytest.mark.parametrize("first_progressive", [False, True])
@pytest.mark.parametrize("mixed", [False, True])
def test_crop_resize_mixes_baseline_and_progressive(O, G, dlib, mixed, first_progressive):
    streams, twins, prog = batch_set(first_progressive, mixed)
    rects = [(1, 2, 40, 31), (0, 0, BW, BH), (7, 3, 19, 29), (3, 1, 36, 36), (13, 6, 50, 40), (2, 2, 8, 8)] + ([(2, 1, 40, 30), (5, 6, 33, 47)] if mixed else [])
    ow, oh = 12, 8
    dec = prog_decoder(G, dlib)
    if mixed:
        assert dec.set_option("dec_opt_batch_sizes", "mixed") == 0
    for rep in range(3):
        got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
        assert same(got, resized(O, twins, rects, ow, oh)), rep
        counted(dec, prog, rep, first_progressive)
    # the tensor call: the same routes, and frame f is, bit for bit, the single call on stream f and on its twin
    scale, bias = [1 / 255.0] * 3, [-0.5, 0.0, 0.25]
    ten, _ = dec.decode_batch_crop_resize_tensor(streams, rects, ow, oh, G.TENSOR_F16, G.TENSOR_CHW, scale, bias)
    counted(dec, prog, 3, first_progressive)
    for f in range(len(streams)):
        one, _ = dec.decode_batch_crop_resize_tensor([streams[f]], [rects[f]], ow, oh, G.TENSOR_F16, G.TENSOR_CHW, scale, bias)
        two, _ = dec.decode_batch_crop_resize_tensor([twins[f]], [rects[f]], ow, oh, G.TENSOR_F16, G.TENSOR_CHW, scale, bias)
        assert np.array_equal(np.asarray(ten[f]).view(np.uint16), np.asarray(one[0]).view(np.uint16)), f
        assert np.array_equal(np.asarray(one[0]).view(np.uint16), np.asarray(two[0]).view(np.uint16)), f
    dec.close()


@pytest.mark.parametrize("call", ["regions", "crop_resize", "tensor"])
def test_progressive_frame_0_behind_a_stale_header_cache(O, G, dlib, call):
    """a decoder that last decoded ANOTHER size (its header cache: a 32 x 32 stream), then a batch whose frame 0 is progressive and whose rectangles lie
    outside that older image: nothing vouches for the cached header, so nothing is launched on it and every frame goes its own way -- the call does
    not fail --, and the next call launches on the header the baseline frames left"""
    import oracle as O2
    small = O2.make_image(32, 32, pixel_format=1, color_space=1, quality=90, restart_interval=2, interleaved=1, subsampling=S420)
    stale = O2.encode_from_coefs(small, P.legal(small, SS.sparse(small, seed=9, density=0.3)))
    streams, twins, prog = batch_set(True)
    streams, twins, prog = streams[:3], twins[:3], prog[:3]  # progressive, baseline, baseline: 64 x 48
    rects = [(20, 10, 40, 30), (33, 17, 31, 31), (40, 34, 24, 14)]
    ow, oh = 12, 8
    scale, bias = [1 / 255.0] * 3, [-0.5, 0.0, 0.25]
    dec = prog_decoder(G, dlib)
    for _ in range(2):
        assert np.array_equal(dec.decode(stale)[0], O.decode(stale)[0])
    assert dec.path_counters()[0] == 1  # (the second of them launched on the cached header: there is one)
    for rep in range(2):
        if call == "regions":
            got, _ = dec.decode_batch_regions(streams, [r[:2] for r in rects], 24, 14)
            assert same(got, oracle_crops(O, twins, [r[:2] for r in rects], 24, 14)), rep
        elif call == "crop_resize":
            got, _ = dec.decode_batch_crop_resize(streams, rects, ow, oh)
            assert same(got, resized(O, twins, rects, ow, oh)), rep
        else:
            got, _ = dec.decode_batch_crop_resize_tensor(streams, rects, ow, oh, G.TENSOR_F16, G.TENSOR_CHW, scale, bias)
        counts = dec.last_batch()
        assert counts == ((0, 3) if rep == 0 else (2, 1)), (rep, counts)
        if call == "tensor":  # (frame f is, bit for bit, the single call on its twin; the last of these leaves the baseline frames' header cached)
            for f in range(3):
                one, _ = dec.decode_batch_crop_resize_tensor([twins[f]], [rects[f]], ow, oh, G.TENSOR_F16, G.TENSOR_CHW, scale, bias)
                assert np.array_equal(np.asarray(got[f]).view(np.uint16), np.asarray(one[0]).view(np.uint16)), (rep, f)
    dec.close()


# ================================================================================================ 4. one decoder, both kinds of frame
ENTROPY = [{}, {"GJ_DEC_ENTROPY": "serial"}, {"GJ_DEC_SEQ": "1"}, {"GJ_DEC_NO_TOKENS": "1"}]


def device_copy(lib, data):
    """the bytes in device memory (the library's own allocator, on either tier) -> pointer"""
    L = lib.L
    L.gj_hip_malloc.restype = C.c_void_p
    L.gj_hip_malloc.argtypes = [C.c_size_t]
    L.gj_hip_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.gj_hip_stream_sync.argtypes = [C.c_void_p]
    ptr = L.gj_hip_malloc(data.size + 64)
    assert ptr and L.gj_hip_memcpy_h2d(ptr, data.ctypes.data, data.size, None) == 0 and L.gj_hip_stream_sync(None) == 0
    return ptr


def decode_at(G, lib, dec, where, size):
    """gpujpeg_decoder_decode on a stream given by address (host or device memory) -> pixels"""
    out = G.DecoderOutput()
    out.type = G.DECODER_OUTPUT_INTERNAL_BUFFER
    rc = lib.L.gpujpeg_decoder_decode(dec.h, where, size, C.byref(out))
    assert rc == 0, rc
    return np.frombuffer((C.c_uint8 * out.data_size).from_address(out.data), np.uint8).copy()


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("env", ENTROPY, ids=lambda e: "_".join(e) or "default")
def test_alternating_frames_keep_planes_and_header_cache(O, G, dlib, monkeypatch, env, memory):
    """baseline full frame, progressive REGION call, baseline full frame (through the plane-route entropy decoder the setting forces), progressive full
    frame, and again: every result right, and the baseline frames' path counters -- launches on the cached header, launches without the table
    kernel, frames decoded again -- those of the same sequence without the progressive frames. Streams in host memory and in device memory (where
    the header of a speculative launch is otherwise compared on the device, behind the launch)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    import oracle as O2
    w, h = 64, 48
    img = O2.make_image(w, h, pixel_format=1, color_space=1, quality=90, restart_interval=2, interleaved=1, subsampling=S420)
    base = [O2.encode_from_coefs(img, P.legal(img, SS.sparse(img, seed=s, density=0.3))) for s in (1, 2)]
    pimg = O2.make_image(w, h, pixel_format=1, color_space=1, quality=90, restart_interval=0, interleaved=1, subsampling=S420)
    pc = P.legal(pimg, SS.with_big(SS.sparse(pimg, seed=5, density=0.3), 20))
    prog, ptwin = P.write(pimg, pc, P.LIBJPEG_COLOUR, restart=2), O2.encode_from_coefs(pimg, pc)
    at = {id(x): (device_copy(dlib, x) if memory == "device" else x.ctypes.data) for x in base + [prog]}
    want_base = [O.decode(b)[0] for b in base]

    def run(with_progressive):
        dec = prog_decoder(G, dlib)

        def frame(stream, region):
            assert dec.set_option("dec_opt_region", region) == 0
            return decode_at(G, dlib, dec, at[id(stream)], stream.size)

        for rep in range(3):
            assert np.array_equal(frame(base[0], "full"), want_base[0]), (rep, "baseline")
            if with_progressive:
                assert same([frame(prog, "9,5,30,20")], oracle_crops(O, [ptwin], [(9, 5)], 30, 20)), (rep, "progressive region")
                assert dec.progressive_stats()[1] == 1 and dec.region_stats()[0] == 2
            assert np.array_equal(frame(base[1], "full"), want_base[1]), (rep, "baseline behind the progressive region")
            assert dec.progressive_stats()[1] == 0
            if with_progressive:
                assert np.array_equal(frame(prog, "full"), O.decode(ptwin)[0]), (rep, "progressive")
        counters = dec.path_counters()
        dec.close()
        return counters

    with_p, without = run(True), run(False)
    assert with_p == without and with_p[2] == 0, (with_p, without)
    if not env:
        assert with_p[0] > 0  # (the baseline frames do launch on the cached header: the comparison is not one of zeros)
    if memory == "device":
        dlib.L.gj_hip_free.argtypes = [C.c_void_p]
        for ptr in at.values():
            dlib.L.gj_hip_free(ptr)


# ================================================================================================ 5. the option, and what is refused
def test_option_off_refuses_sof2_as_ever(O, G, dlib, capfd):
    jpeg, twin = case("420_33x17", kind="with_big")[:2]
    for setting in (None, "off"):
        dec = G.Decoder(dlib)
        if setting:
            assert dec.set_option(OPT, setting) == 0
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            dec.decode(jpeg)
        assert "Marker SOF2 (Progressive with Huffman coding) is not supported!" in capfd.readouterr().err
        px, _ = dec.decode(twin)
        assert np.array_equal(px, O.decode(twin)[0])
        assert dec.progressive_stats() == (0, 0, 0, 0, 0)
        dec.close()
    dec = G.Decoder(dlib)
    assert dec.progressive_stats() == (-1, 0, 0, 0, 0)
    assert dec.set_option(OPT, "on") == 0
    assert dec.set_option(OPT, "maybe") != 0  # refused, and the setting stays
    px, _ = dec.decode(jpeg)
    assert np.array_equal(px, O.decode(twin)[0])
    assert dec.set_option(OPT, "off") == 0 and dec.set_option(OPT, "ON") != 0
    with pytest.raises(RuntimeError):
        dec.decode(jpeg)
    dec.close()
    assert G.PROGRESSIVE_MAX_SCANS == 64 and G.DEC_OPT_PROGRESSIVE == OPT
    assert G.stream_info(dlib, twin)[:4] == (33, 17, 3, 0) and G.stream_info(dlib, twin[:10]) is None


def refused_streams():
    img = image_of("420_33x17")
    coefs = P.legal(img, coefficients("420_33x17", "sparse"))
    sc = P.LIBJPEG_COLOUR
    out = {}
    out["refinement with the wrong Ah"] = (P.write(img, coefs, sc, raw_sos={5: ((0,), 1, 63, 3, 2)}), 6)
    out["AC before DC"] = (P.write(img, coefs, [sc[1], sc[0]] + sc[2:]), 1)
    out["an AC scan with two components"] = (P.write(img, coefs, sc, raw_sos={2: ((1, 2), 1, 63, 0, 1)}), 3)
    many = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(3) for k in range(1, 23)]
    out["65 scans"] = (P.write(img, coefs, many[:65]), 65)
    slot = bytearray(P.write(img, coefs, sc, slots=0).tobytes())
    at = bytes(slot).index(b"\xff\xda", bytes(slot).index(b"\xff\xda") + 2)  # the second SOS: the luminance AC scan asks for AC slot 2
    slot[at + 6] = 0x22
    out["an undefined table slot"] = (np.frombuffer(bytes(slot), np.uint8).copy(), 2)
    return out


@pytest.mark.parametrize("what", ["refinement with the wrong Ah", "AC before DC", "an AC scan with two components", "65 scans", "an undefined table slot"])
def test_refusals_leave_the_decoder_usable(O, G, dlib, capfd, what):
    bad, offender = refused_streams()[what]
    good, twin = case("420_33x17", kind="with_big")[:2]
    dec = prog_decoder(G, dlib)
    for rep in range(2):
        with pytest.raises(RuntimeError):
            dec.decode(bad)
        err = capfd.readouterr().err
        assert ("more than 64 scans" in err) if offender == 65 else (f"Progressive scan {offender - 1}:" in err), err
        px, _ = dec.decode(good)
        assert np.array_equal(px, O.decode(twin)[0]), (what, rep)
    dec.close()
    assert G.stream_info(dlib, bad)[7] == offender


def test_an_sos_without_payload_at_the_end_of_the_data(O, G, dlib):
    """a stream that ends in an SOS segment of length 2 (no payload: not even the component count) is refused, by both parses, and the decoder goes on"""
    good, twin = case("420_33x17", kind="with_big")[:2]
    d = good.tobytes()
    second = d.index(b"\xff\xda", d.index(b"\xff\xda") + 2)
    for at in (d.index(b"\xff\xda"), second):
        bad = np.frombuffer(d[:at] + b"\xff\xda\x00\x02", np.uint8).copy()
        assert G.stream_info(dlib, bad) is None
        dec = prog_decoder(G, dlib)
        with pytest.raises(RuntimeError):
            dec.decode(bad)
        assert np.array_equal(dec.decode(good)[0], O.decode(twin)[0])
        dec.close()


# ================================================================================================ 6. files written by libjpeg
FILES = ["444_q75", "422_q75", "420_q75", "420_q30", "420_q95", "grey_q75"]


@pytest.mark.parametrize("name", FILES)
def test_libjpeg_files_decode_to_their_baseline_twins(O, G, dlib, name):
    prog = np.fromfile(os.path.join(GOLDEN, name + "_progressive.jpg"), np.uint8)
    twin = np.fromfile(os.path.join(GOLDEN, name + "_baseline.jpg"), np.uint8)
    assert prog.size < 8192 and twin.size < 8192
    st = O.parse(twin)
    try:
        want_coefs = O.huffman_decode(st, twin)
    finally:
        O.lib().gjo_stream_free(C.byref(st))
    dec = prog_decoder(G, dlib)
    dec.keep_coefficients(True)
    px, _ = dec.decode(prog)
    got = dec.coefficients(want_coefs.size)
    assert np.array_equal(px, O.decode(twin)[0]), name
    info = G.stream_info(dlib, prog)
    assert info[3] == 1 and info[4] == (6 if name.startswith("grey") else 10) and info[5] == 3 and info[7] == 0
    assert np.array_equal(got, want_coefs), name
    one, _ = dec.decode(twin)
    assert np.array_equal(one, px)
    dec.close()


@pytest.mark.gpu
def test_gpujpegtool_passes_the_option_through(O, G, gpu_lib, tmp_path):
    """the tool has no flag of its own: -O dec_opt_progressive=on reaches gpujpeg_decoder_set_option, and the file decodes to its twin's image"""
    import subprocess
    exe = os.path.join(os.path.dirname(G.PRODUCT_LIB), "gpujpegtool")
    src = os.path.join(GOLDEN, "420_q75_progressive.jpg")
    twin = np.fromfile(os.path.join(GOLDEN, "420_q75_baseline.jpg"), np.uint8)
    r = subprocess.run([exe, "-d", "-O", OPT + "=on", src, "out.rgb"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(tmp_path / "out.rgb", np.uint8), O.decode(twin, PF_RGB, 1)[0])
    r = subprocess.run([exe, "-d", src, "off.rgb"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp_path, timeout=120)
    assert r.returncode != 0 and b"SOF2" in r.stderr


def test_pil_reads_the_writers_streams_as_their_twins(O):
    PIL = pytest.importorskip("PIL.Image")
    import io
    for geom, script, kind, restart in (("420_33x17", "default", "with_big", 0), ("420_33x17", "deep", "dense", 3), ("grey_17x9", "default", "refinement_runs", 0),
                                        ("444_24x16", "chroma_first", "sparse", 1), ("422_35x13", "dc_chroma", "with_big", 0), ("420_33x17", "dc_each", "sparse", 2)):
        jpeg, twin = case(geom, script=script, kind=kind, restart=restart)[:2]
        a = np.asarray(PIL.open(io.BytesIO(jpeg.tobytes())))
        b = np.asarray(PIL.open(io.BytesIO(twin.tobytes())))
        assert np.array_equal(a, b), (geom, script, kind, restart)


# ================================================================================================ 7. damaged streams (CPU tier only)
@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("geom,restart", [("420_33x17", 0), ("420_322x242", 7)])
def test_damaged_progressive_streams(O, G, emu, geom, restart, part):
    """200 seeded single-byte and burst mutations inside the entropy-coded data, and truncations at every 97th byte (a quarter of both per case): the
    call returns, the guard bands around the stream and around the output are untouched, and the decoder then decodes a good stream correctly"""
    jpeg, twin = case(geom, kind="with_big", restart=restart)[:2]
    want = O.decode(twin)[0]
    ranges = P.scan_data_ranges(jpeg)
    rng = np.random.default_rng(97)
    GUARD = 4096
    dec = prog_decoder(G, emu)
    raw = want.size

    def attempt(data):
        buf = np.full(GUARD + data.size + GUARD, 0xA5, np.uint8)
        buf[GUARD:GUARD + data.size] = data
        out = np.full(GUARD + raw + GUARD, 0x5A, np.uint8)
        o = G.DecoderOutput()
        o.type, o.data = G.DECODER_OUTPUT_CUSTOM_BUFFER, out.ctypes.data + GUARD
        rc = emu.L.gpujpeg_decoder_decode(dec.h, buf.ctypes.data + GUARD, data.size, C.byref(o))
        assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + data.size:] == 0xA5), "the stream's guard bands"
        assert np.all(out[:GUARD] == 0x5A) and np.all(out[GUARD + raw:] == 0x5A), "the output's guard bands"
        return rc

    mutated = []
    for i in range(200):
        start, length = ranges[int(rng.integers(len(ranges)))]
        bad = jpeg.copy()
        at = start + int(rng.integers(max(1, length)))
        n = 1 if i % 2 == 0 else int(rng.integers(2, 9))
        bad[at:min(at + n, start + length)] = rng.integers(0, 256, min(at + n, start + length) - at)
        mutated.append(bad)
    for bad in mutated[part::4]:
        attempt(bad)
    for cut in list(range(97, jpeg.size, 97))[part::4]:
        attempt(jpeg[:cut].copy())
    px, _ = dec.decode(jpeg)
    assert np.array_equal(px, want)
    dec.close()
