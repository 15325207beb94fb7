"""Batched reduced-size decode: dec_opt_scale = 1/2, 1/4, 1/8 together with gpujpeg_amd_decoder_decode_batch / _decode_batch_ptrs (gpujpeg_amd_ext.h).

Expected pixels are always test_scaled_decode.expected(): the numpy restatement of the integer definition over the oracle's coefficients (no product
code); where stated, also the same library's single calls with the option. Nothing is compared with the batched path itself. Every comparison is
byte for byte.

Two tiers with the same bodies, like test_region_batch.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product
library on the MI355X. One test re-runs the CPU tier on the AddressSanitizer + UBSan build of the execution model.

"Every frame through the batched launches", last_batch() == (n, 0), needs the pixels to go to DEVICE memory: with host output frame 0 of every
batch call goes the ordinary way first (it tells the size of the staging area), so the most a host-output call can report is (n - 1, 1). The tests
that ask for (n, 0) therefore hand over device buffers (gj_hip_malloc, which both tiers have); test 2 checks both."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import CASES, natural_image, oracle_image
from test_region_batch import frames_of, new_decoder, same
from test_region_decode import damaged_restart_markers
from test_scaled_decode import OPT, SCALES, UYVY_EVEN, damaged_streams, dims, expected, perf_decoder

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")
ASAN_DIR = os.path.join(EMU_DIR, "_build_asan")
ASAN_LIB = os.path.join(ASAN_DIR, "libgpujpeg_emu.so")
CLANG_RT = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"
ROUTES = {"tokens": ("GJ_DEC_TOKENS", 2), "planes": ("GJ_DEC_NO_TOKENS", 1)}  # route -> (setting, idct_path of the reduced-size kernel)


@pytest.fixture(scope="session")
def emu(G):
    """The product's host C and .hip files on the CPU execution model (built like test_emu_parity.py's emu_lib)."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("make") is None:
        pytest.skip("hipemu needs ROCm's clang++ (host compilation of the .hip files)")
    import fcntl
    with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-j8", "-C", EMU_DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = G.Library(os.environ.get("GJ_EMU_LIB") or EMU_LIB)
    assert lib.L.gpujpeg_init_device(0, 0) == 0
    return lib


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dlib(request):
    """the library of the tier: the CPU execution model, or the product on the GPU (lib.tier says which)"""
    lib = request.getfixturevalue("emu" if request.param == "emu" else "gpu_lib")
    lib.tier = request.param
    return lib


# ================================================================================================ helpers
def case_named(name):
    return [c for c in CASES if c[0] == name][0]


def set_scale(dec, s):
    assert dec.set_option(OPT, "1" if s == 1 else f"1/{s}") == 0


def wanted(O, streams, s, pf=None, cs=None):
    return [expected(O, x, -1 if pf is None else pf, -1 if cs is None else cs, s)[0] for x in streams]


def diffs(got, want):
    return [int(np.count_nonzero(a != b)) if a.size == b.size else (a.size, b.size) for a, b in zip(got, want)]


def device_batch(lib, dec, streams, frame, slack=0):
    """decode_batch with streams and pixels in device memory: streams at a 16-byte stride, output slots of frame + slack bytes pre-filled with 0xA5
    -> (frames, the slack bytes behind every frame [n][slack], ImageParameters)"""
    L = lib.L
    L.gj_hip_malloc.restype = C.c_void_p
    L.gj_hip_malloc.argtypes = [C.c_size_t]
    L.gj_hip_free.argtypes = [C.c_void_p]
    L.gj_hip_memcpy_h2d.argtypes = L.gj_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.gj_hip_stream_sync.argtypes = [C.c_void_p]
    n, sizes = len(streams), [int(x.size) for x in streams]
    in_stride, out_stride = (max(sizes) + 64 + 15) & ~15, frame + slack
    host = np.zeros(in_stride * n, np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride:i * in_stride + x.size] = x
    out = np.full(out_stride * n, 0xA5, np.uint8)
    d_in, d_out = L.gj_hip_malloc(host.size), L.gj_hip_malloc(out.size)
    assert d_in and d_out
    try:
        assert L.gj_hip_memcpy_h2d(d_in, host.ctypes.data, host.size, None) == 0 and L.gj_hip_memcpy_h2d(d_out, out.ctypes.data, out.size, None) == 0
        assert L.gj_hip_stream_sync(None) == 0
        _, pi = dec.decode_batch(None, device_out=d_out, out_stride=out_stride, device_in=d_in, in_stride=in_stride, sizes=sizes)
        assert L.gj_hip_memcpy_d2h(out.ctypes.data, d_out, out.size, None) == 0 and L.gj_hip_stream_sync(None) == 0
    finally:
        L.gj_hip_free(d_in)
        L.gj_hip_free(d_out)
    rows = out.reshape(n, out_stride)
    return [rows[f, :frame].copy() for f in range(n)], rows[:, frame:].copy(), pi


# six frames of rgb_hdlike_r24 (480 x 272: 60 blocks per row, so the waves of the token-fed kernel straddle block rows; 2040 block positions, so
# the last workgroup of both kernels is partial), natural and noise content in alternation
HD_CASE = "rgb_hdlike_r24"


@pytest.fixture(scope="module")
def hd(O):
    """the streams of tests 1, 4, 5, 7 and 8 and their expected reduced images at every scale (and the full-size oracle decode), made once"""
    streams = frames_of(O, case_named(HD_CASE), 6)
    want = {s: wanted(O, streams, s) for s in SCALES}
    want[1] = [O.decode(x)[0] for x in streams]
    return streams, want


# frames whose reduced size is no multiple of 4 while whole waves take the dense store path: 1031 x 17 (129 blocks per row; 258 x 5 pixels x 3 =
# 3870 bytes at 1/4, 129 x 3 x 3 = 1161 at 1/8) and 517 x 40 (65 blocks per row; 65 x 5 x 3 = 975 bytes at 1/8). The other scales give multiples
# of 4: test 2 also runs them with slots of one byte more.
ODD_CASES = [("odd_1031x17", 1031, 17, 1, 1, 50, -1, 0, None, 3), ("odd_517x40", 517, 40, 1, 1, 75, 3, 0, None, 3)]


@pytest.fixture(scope="module")
def odd(O):
    out = {}
    for case in ODD_CASES:
        streams = [O.encode(oracle_image(O, case), natural_image(case[1], case[2], 3, seed=case[1] + f)) for f in range(3)]
        out[case[0]] = (streams, {s: wanted(O, streams, s) for s in SCALES})
    sizes = {(name, s): out[name][1][s][0].size for name in out for s in SCALES}
    assert sizes[("odd_1031x17", 4)] == 3870 and sizes[("odd_1031x17", 8)] == 1161 and sizes[("odd_517x40", 8)] == 975
    return out


# ================================================================================================ 1. batched, both routes, chunks
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
def test_batched_both_routes(O, G, dlib, hd, s, route, chunk, monkeypatch):
    """the second call has a header to launch on: every frame goes through the batched launches and the reduced-size kernel of the route"""
    streams, want = hd
    monkeypatch.setenv(ROUTES[route][0], "1")
    dec = perf_decoder(G, dlib)
    if chunk:
        dec.set_batch_chunk(chunk)
    set_scale(dec, s)
    W, H = dims(480, 272, s)
    for rep in range(2):
        got, guard, pi = device_batch(dlib, dec, streams, want[s][0].size)
        assert (pi.width, pi.height, pi.pixel_format) == (W, H, 1) and dlib.image_size(pi) == want[s][0].size
        assert same(got, want[s]), (rep, diffs(got, want[s]))
    print("last_batch", dec.last_batch(), "idct_path", dec.idct_path())
    assert dec.last_batch() == (6, 0)
    assert dec.idct_path() == ROUTES[route][1], "the route of the batched launches"
    got, pi = dec.decode_batch(streams)  # (pixels to host memory: frame 0 goes ahead, the others are batched)
    assert same(got, want[s]) and dec.last_batch() == (5, 1)
    dec.close()


# ================================================================================================ 2. dense stores at unaligned frame bases
@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
@pytest.mark.parametrize("name", [c[0] for c in ODD_CASES])
def test_dense_stores_at_unaligned_frame_bases(O, G, dlib, odd, name, s, monkeypatch):
    """token route: frames 1 and 2 start off the dword grid (frames packed back to back, in the staging area of a host-output call and in a device
    buffer alike), so the alignment of the dense rows has to come from the frame's own base and the byte-wise head and tail must stay in its slot"""
    streams, want = odd[name]
    raw = want[s][0].size
    monkeypatch.setenv("GJ_DEC_TOKENS", "1")
    dec = perf_decoder(G, dlib)
    set_scale(dec, s)
    for rep in range(2):
        got, pi = dec.decode_batch(streams)  # host output
        assert dlib.image_size(pi) == raw and same(got, want[s]), (rep, diffs(got, want[s]))
    print("host output: last_batch", dec.last_batch(), "idct_path", dec.idct_path())
    assert dec.last_batch() == (2, 1), "host output: frame 0 goes ahead, the others through the batched launches"
    assert dec.idct_path() == 2
    for rep in range(2):
        got, guard, _ = device_batch(dlib, dec, streams, raw, slack=1 if rep else 0)  # (slots of raw and of raw + 1 bytes)
        assert same(got, want[s]) and np.all(guard == 0xA5), (rep, diffs(got, want[s]))
        print("device output: last_batch", dec.last_batch(), "idct_path", dec.idct_path())
        assert dec.last_batch() == (3, 0) and dec.idct_path() == 2
    dec.close()


# ================================================================================================ 3. plane-route configurations
PLANE_CASES = [case_named(n) for n in ("rgb_to_420_il", "rgb_to_422_nonil", "planar420_in", "gray", "rgba_4444")] + [UYVY_EVEN]


@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
@pytest.mark.parametrize("case", PLANE_CASES, ids=[c[0] for c in PLANE_CASES])
def test_plane_route_configurations(O, G, dlib, case, s):
    pf, cs = case[3], case[4]
    streams = frames_of(O, case, 3, seed=40)
    want = wanted(O, streams, s, pf, cs)
    W, H = dims(case[1], case[2], s)
    # what a decoder of the same settings without the scale reports for its second call
    full = new_decoder(G, dlib, pf, cs)
    for rep in range(2):
        full.decode_batch(streams)
    unscaled = full.last_batch()
    full.close()
    dec = new_decoder(G, dlib, pf, cs)
    set_scale(dec, s)
    for rep in range(2):
        got, pi = dec.decode_batch(streams)
        assert (pi.width, pi.height, pi.pixel_format) == (W, H, pf) and dlib.image_size(pi) == want[0].size
        assert same(got, want), (rep, diffs(got, want))
    print("last_batch", dec.last_batch(), "without the scale", unscaled)
    assert dec.last_batch() == unscaled
    dec.close()


# ================================================================================================ 4. strangers inside a scaled batch
def test_strangers_inside_a_scaled_batch(O, G, dlib, hd):
    """frame 2 has another header (another quality), frame 3 a misnumbered restart marker (CPU tier: also one with a missing marker): they go the
    ordinary way with the decoder's scale, their neighbours stay in the batched launches"""
    streams, want = hd
    case = case_named(HD_CASE)
    other = O.encode(oracle_image(O, case[:5] + (90,) + case[6:]), natural_image(480, 272, 3, seed=77))
    bads = [bad for kind, bad, _ in damaged_restart_markers(streams[3]) if kind == "renumbered"]
    if dlib.tier == "emu":
        bads += [bad for kind, bad in damaged_streams(streams[3]) if kind == "missing_restart_marker"]
    for bad in bads:
        mixed = [streams[0], streams[1], other, bad, streams[4]]
        ref = new_decoder(G, dlib)  # the definition: the single scaled call on every stream
        set_scale(ref, 2)
        singles = []
        for x in mixed:
            try:
                singles.append(ref.decode(x)[0])
            except RuntimeError:
                singles.append(None)
        ref.close()
        assert same([singles[i] for i in (0, 1, 4)], [want[2][i] for i in (0, 1, 4)]) and np.array_equal(singles[2], expected(O, other, -1, -1, 2)[0])
        dec = new_decoder(G, dlib)
        set_scale(dec, 2)
        for rep in range(2):
            if singles[3] is None:
                with pytest.raises(RuntimeError):
                    dec.decode_batch(mixed)
                continue
            got, pi = dec.decode_batch(mixed)
            assert (pi.width, pi.height) == (240, 136) and same(got, singles), (rep, diffs(got, singles))
            batched, single = dec.last_batch()
            print("last_batch", batched, single)
            assert single >= 2 and batched >= 1, (batched, single)
        got, _ = dec.decode_batch(streams)  # the decoder decodes the intact streams as ever
        assert same(got, want[2])
        dec.close()


# ================================================================================================ 5. option changes on one decoder
def test_option_changes_on_one_decoder(O, G, dlib, hd):
    streams, want = hd
    dec = new_decoder(G, dlib)
    for s in (1, 4, 1, 8):
        set_scale(dec, s)
        W, H = dims(480, 272, s)
        got, pi = dec.decode_batch(streams)
        assert (pi.width, pi.height) == (W, H) and dlib.image_size(pi) == want[s][0].size and same(got, want[s]), (s, diffs(got, want[s]))
        got, _, pi = device_batch(dlib, dec, streams, want[s][0].size)
        assert (pi.width, pi.height) == (W, H) and same(got, want[s]) and dec.last_batch() == (6, 0), (s, dec.last_batch())
        set_scale(dec, 2)  # one single call at 1/2 in between
        px, pi = dec.decode(streams[1])
        assert (pi.width, pi.height) == (240, 136) and np.array_equal(px, want[2][1])
    # the decoder saw another geometry last (its cached header is a 640 x 368 sequence's): a scaled batch of 480 x 272 frames
    big = O.encode(oracle_image(O, case_named("rgb_natural_auto")), natural_image(640, 368, 3, seed=5))
    for device in (False, True):
        set_scale(dec, 1)
        px, pi = dec.decode(big)
        assert (pi.width, pi.height) == (640, 368) and np.array_equal(px, O.decode(big)[0])
        set_scale(dec, 4)
        got, pi = device_batch(dlib, dec, streams, want[4][0].size)[::2] if device else dec.decode_batch(streams)
        assert (pi.width, pi.height) == (120, 68) and same(got, want[4]), (device, diffs(got, want[4]))
    dec.close()


# ================================================================================================ 6. refusals keep their shape
def test_refusals_keep_their_shape(O, G, dlib, hd):
    streams, want = hd
    # packed 4:2:2 output of odd reduced width: 322 x 50 is 161, 81 and 41 pixels wide
    case = case_named("uyvy_422_il_q90")
    uyvy = frames_of(O, case, 3, seed=60)
    full = [O.decode(x, 3, 3)[0] for x in uyvy]
    for warm in (False, True):  # (without / with a header to launch on when the refused call comes)
        for s in SCALES:
            dec = new_decoder(G, dlib, 3, 3)
            if warm:
                assert same(dec.decode_batch(uyvy)[0], full)
            set_scale(dec, s)
            with pytest.raises(RuntimeError):
                dec.decode(uyvy[0])
            with pytest.raises(RuntimeError):
                dec.decode_batch(uyvy)
            with pytest.raises(RuntimeError):
                device_batch(dlib, dec, uyvy, full[0].size)
            set_scale(dec, 1)
            assert same(dec.decode_batch(uyvy)[0], full), (warm, s)
            dec.close()
        # a flip together with a scale
        dec = new_decoder(G, dlib)
        if warm:
            assert same(dec.decode_batch(streams)[0], want[1])
        set_scale(dec, 2)
        assert dec.set_option("dec_opt_flipped", "1") == 0
        with pytest.raises(RuntimeError):
            dec.decode(streams[0])
        with pytest.raises(RuntimeError):
            dec.decode_batch(streams)
        with pytest.raises(RuntimeError):
            device_batch(dlib, dec, streams, want[2][0].size)
        assert dec.set_option("dec_opt_flipped", "0") == 0
        assert same(dec.decode_batch(streams)[0], want[2]), warm
        dec.close()
    # a batch of regions with a scale set stays refused
    dec = new_decoder(G, dlib)
    set_scale(dec, 2)
    origins = [(0, 0)] * len(streams)
    for rep in range(2):
        with pytest.raises(RuntimeError):
            dec.decode_batch_regions(streams, origins, 64, 40)
        assert same(dec.decode_batch(streams)[0], want[2])
    dec.close()


# ================================================================================================ 7. separate buffers
@pytest.mark.parametrize("s", SCALES, ids=[f"1_{s}" for s in SCALES])
def test_decode_batch_ptrs_with_room_for_exactly_a_reduced_frame(O, G, dlib, hd, s):
    streams, want = hd
    dec = new_decoder(G, dlib)
    set_scale(dec, s)
    W, H = dims(480, 272, s)
    for rep in range(2):
        got, pi = dec.decode_batch_ptrs(streams, want[s][0].size)
        assert (pi.width, pi.height) == (W, H) and same(got, want[s]), (rep, diffs(got, want[s]))
    batched, single = dec.last_batch()
    print("last_batch", batched, single)
    assert batched >= 5 and single <= 1, "(single = 1: numpy happened to put the destinations a constant distance apart, which makes them one host buffer)"
    dec.close()


# ================================================================================================ 8. device-resident in and out
@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("s", [4, 8], ids=["1_4", "1_8"])
def test_device_streams_and_device_output(O, G, gpu_lib, hd, odd, s, route, monkeypatch):
    """streams in device memory at a 16-byte stride, output slots of raw + 64 bytes pre-filled with 0xA5: every frame, and every guard byte behind it"""
    monkeypatch.setenv(ROUTES[route][0], "1")
    for streams, want in (hd, odd["odd_1031x17"]):
        dec = perf_decoder(G, gpu_lib)
        set_scale(dec, s)
        for rep in range(2):
            got, guard, pi = device_batch(gpu_lib, dec, streams, want[s][0].size, slack=64)
            assert gpu_lib.image_size(pi) == want[s][0].size and same(got, want[s]), (rep, diffs(got, want[s]))
            assert guard.shape == (len(streams), 64) and np.all(guard == 0xA5), rep
        assert dec.last_batch() == (len(streams), 0) and dec.idct_path() == ROUTES[route][1]
        dec.close()


# ================================================================================================ 9. sanitizers
@pytest.fixture(scope="session")
def asan_env():
    if not os.path.exists(CLANG_RT) or shutil.which("make") is None:
        pytest.skip("needs ROCm's clang with its AddressSanitizer runtime")
    import fcntl
    with open(os.path.join(EMU_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-j8", "-C", EMU_DIR, "SAN=1", "OPT=-O1", f"OUT={ASAN_DIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return dict(os.environ, LD_PRELOAD=CLANG_RT, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0:abort_on_error=1",
                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_cpu_tier_under_sanitizers(asan_env):
    """this file's CPU-tier tests once more on the AddressSanitizer + UBSan build of the execution model (the reduced planes and pixels of every
    frame of a batch, the unaligned frame bases, the strangers inside a batch)"""
    env = dict(asan_env, GJ_EMU_LIB=ASAN_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-n", "4", "-m", "not gpu", "-p", "no:faulthandler",
                        "-p", "no:cacheprovider", "-k", "not under_sanitizers"], capture_output=True, text=True, errors="replace",
                       timeout=1500, env=env, cwd=ROOT)
    tail = (r.stdout[-1500:] + "\n" + "\n".join(ln for ln in r.stderr.splitlines() if not ln.startswith("[GPUJPEG]"))[-3000:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1500:]
