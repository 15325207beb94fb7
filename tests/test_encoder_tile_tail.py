"""The tail of the fused encoders' coder (gj_code_tile, gpujpeg_amd/csrc/gj_enc_tiles.hip): the merge of the lanes' private streams into the LDS
window (a wave none of whose blocks has completed a dword merges the 64-bit register tails alone), the drain of the window to the tile's stream as
one run of dwords (a dword with 0xFF bytes looks up its segment and adds its count there), and the tile's finished size taken by the first wave.

Every case compares the product's JPEG bytes with the oracle's, like tests/test_gpu_parity.py::test_encoder_tiles_and_gather: the file holds every
stream byte, and k_gather places and stuffs the segments by seg_bytes[] / seg_ff[] and the tile sizes, so a wrong count moves or damages the bytes.
Every case is encoded without and with the APP13 segment index: inside a tile k_gather needs only the SUM of its segments' 0xFF counts, the index
needs every single one (a 0xFF byte counted for the neighbouring segment shows there and nowhere else).

The shapes are the ones at which this code can go wrong. Segment geometry: restart intervals that give 1, 7 and 64 segments per 256-lane tile, a
last tile with fewer segments, a last segment shorter than the interval, segments that straddle two waves (36 blocks) and segments that end on lane
63 (4 blocks), frames whose tile slack is not a multiple of 64 blocks. Content: all-grey, in frames of whole MCUs (every block is DC + EOB: no lane completes a dword, in
any component), the natural pattern at q75, noise at q100 (blocks that continue in d_temp, tiles that need several windows, many 0xFF bytes: each noise
case with more than one segment per tile is asserted to hold a tile with 0xFF bytes in two of its segments). Kernel shapes: k_encode_rgb444 whole,
its one-component form, its split tail (developer settings GJ_ENC_SPLIT / GJ_ENC_TAIL), k_encode_uyvy422, k_encode_blocks (planar 4:2:0, RGB ->
4:2:0 interleaved), and a 3-frame encode_batch.

On the CPU tier the execution model's build counts the waves per side of the merge (gj_emu_enc_merge_waves, under GJ_HIPEMU only): all-grey must
take the tails-only side in every wave that holds a block, noise at q100 in none -- "equal bytes" cannot mean "the short merge never ran".

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on the MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import api_params, natural_image, oracle_image
from test_synthetic_streams import emu  # noqa: F401  (the fixture)

S420 = ((2, 2), (1, 1), (1, 1))
WHOLE, ONE, TAIL = {"GJ_ENC_SPLIT": "0"}, {"GJ_ENC_SPLIT": "100000"}, {"GJ_ENC_SPLIT": "0", "GJ_ENC_TAIL": "2"}
SETTINGS = ("GJ_ENC_SPLIT", "GJ_ENC_TAIL")

# id: (w, h, pixel format, colour space, quality, restart interval, interleaved, subsampling, content, developer settings)
CASES = {
    # ---- k_encode_rgb444, all three components per workgroup. 296x16: 74 blocks; 640x368 and 636x364: 3680 blocks
    "grey_296x16_r36": (296, 16, 1, 1, 75, 36, 0, None, "grey", WHOLE),         # 7 per tile; the one tile has 3 segments, the last of 2 blocks
    "grey_640x368_r4": (640, 368, 1, 1, 75, 4, 0, None, "grey", WHOLE),          # 64 per tile, every 16th segment ends on lane 63; last tile: 24 segments
    "grey_640x368_r200": (640, 368, 1, 1, 75, 200, 0, None, "grey", WHOLE),      # 1 per tile, the last one of 80 blocks
    "natural_640x368_r36": (640, 368, 1, 1, 75, 36, 0, None, "natural", WHOLE),  # 15 tiles of 252 blocks, the last of 5 segments, the last segment of 8 blocks
    "natural_636x364_r4": (636, 364, 1, 1, 75, 4, 0, None, "natural", WHOLE),
    "natural_640x368_r200": (640, 368, 1, 1, 75, 200, 0, None, "natural", WHOLE),
    "noise_512x264_r36": (512, 264, 1, 1, 100, 36, 0, None, "noise", WHOLE),     # 2112 blocks: tiles of ~25 KB, several windows; last tile 3 segments, last segment 24 blocks
    "noise_296x16_r4": (296, 16, 1, 1, 100, 4, 0, None, "noise", WHOLE),         # 19 segments in one tile, the last of 2 blocks; SEEDS: 0xFF bytes at segment ends
    "noise_296x16_r200": (296, 16, 1, 1, 100, 200, 0, None, "noise", WHOLE),     # one segment over two waves, several windows
    # ---- its one-component form (three workgroups per tile) and its split tail (the last two tiles as three workgroups each)
    "one_grey_296x16_r36": (296, 16, 1, 1, 75, 36, 0, None, "grey", ONE),
    "one_natural_636x364_r36": (636, 364, 1, 1, 75, 36, 0, None, "natural", ONE),
    "one_noise_296x16_r36": (296, 16, 1, 1, 100, 36, 0, None, "noise", ONE),
    "tail_grey_640x368_r36": (640, 368, 1, 1, 75, 36, 0, None, "grey", TAIL),
    "tail_natural_640x368_r36": (640, 368, 1, 1, 75, 36, 0, None, "natural", TAIL),
    "tail_noise_512x264_r36": (512, 264, 1, 1, 100, 36, 0, None, "noise", TAIL),
    # ---- k_encode_uyvy422: interleaved packed 4:2:2 at q90, 4 blocks per MCU: intervals of 9, 1 and 64 MCUs = 7, 64 and 1 segments per tile
    "uyvy_grey_640x48_r9": (640, 48, 3, 3, 90, 9, 1, None, "grey", {}),
    "uyvy_noise_648x50_r9": (648, 50, 3, 3, 90, 9, 1, None, "noise", {}),        # 41 x 7 MCUs = 287: 32 segments, the last of 8 MCUs; last tile 4 segments
    "uyvy_noise_296x16_r1": (296, 16, 3, 3, 90, 1, 1, None, "noise", {}),
    "uyvy_noise_648x50_r64": (648, 50, 3, 3, 90, 64, 1, None, "noise", {}),
    "uyvy_noise_q100_296x16_r9": (296, 16, 3, 3, 100, 9, 1, None, "noise", {}),
    # ---- k_encode_blocks: planar 4:2:0 (three scans of different sizes) and RGB -> 4:2:0 interleaved (6 blocks per MCU: 6 MCUs = 36 blocks)
    "planar420_grey_320x112_r36": (320, 112, 5, 3, 75, 36, 0, None, "grey", {}),
    "planar420_noise_322x114_r36": (322, 114, 5, 3, 100, 36, 0, None, "noise", {}),
    "planar420_noise_322x114_r4": (322, 114, 5, 3, 100, 4, 0, None, "noise", {}),
    "rgb420il_grey_320x112_r6": (320, 112, 1, 1, 75, 6, 1, S420, "grey", {}),
    "rgb420il_natural_322x114_r6": (322, 114, 1, 1, 75, 6, 1, S420, "natural", {}),
    "rgb420il_noise_322x114_r6": (322, 114, 1, 1, 100, 6, 1, S420, "noise", {}),
    "rgb420il_noise_322x114_r42": (322, 114, 1, 1, 100, 42, 1, S420, "noise", {}),  # 252 blocks per segment: one per tile
}


# noise seeds chosen for what the stream then holds (test_tile_tail_ff_bytes_at_segment_boundaries); the others follow from the size
SEEDS = {"noise_296x16_r4": 2}


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request):
    """(the library of the tier, is it the CPU execution model)"""
    return request.getfixturevalue("emu" if request.param == "emu" else "gpu_lib"), request.param == "emu"


def case_of(name):
    w, h, pf, cs, q, ri, il, sub, _, _ = CASES[name]
    return (name, w, h, pf, cs, q, ri, il, [tuple(s) for s in sub] if sub else None, 3)


def pixels(O, content, w, h, pf, seed):
    n = O.raw_size(w, h, pf)
    if content == "grey":
        return np.full(n, 128, np.uint8)
    if content == "natural":
        assert pf == 1
        return natural_image(w, h, 3, seed=seed)
    return O.noise(n, seed=seed)  # the reference's test-image noise (src/utils/image.c .tst files), oracle.noise


@functools.lru_cache(maxsize=None)
def reference(name):
    """(raw pixels, the oracle's JPEG, the oracle's JPEG with the APP13 segment index) of a case, computed once, read-only"""
    import oracle as O
    w, h, pf, cs, q, ri, il, sub, content, _ = CASES[name]
    raw = pixels(O, content, w, h, pf, seed=SEEDS.get(name, w * 7 + h + ri))
    want = [O.encode(oracle_image(O, case_of(name), segment_info=si), raw) for si in (0, 1)]
    for a in [raw] + want:
        a.setflags(write=False)
    return raw, want[0], want[1]


def scan_segments(jpeg):
    """per scan of a baseline JPEG, for every restart segment in stream order: (the offsets of its 0xFF bytes in the UNSTUFFED segment, one per
    FF 00 pair; the unstuffed segment's bytes)"""
    b = bytes(jpeg)
    assert b[:2] == b"\xff\xd8"
    scans, p = [], 2
    while p < len(b):
        assert b[p] == 0xFF, p
        m = b[p + 1]
        if m == 0xD9:
            break
        n = (b[p + 2] << 8) | b[p + 3]
        p += 2 + n
        if m != 0xDA:
            continue
        segs, ff, start = [], [], p
        while True:
            q = b.index(b"\xff", p)
            nxt = b[q + 1]
            p = q + 2
            if nxt == 0x00:
                ff.append(q - start - len(ff))
            elif 0xD0 <= nxt <= 0xD7:
                segs.append((ff, q - start - len(ff)))
                ff, start = [], p
            else:  # the next marker: the scan is over
                segs.append((ff, q - start - len(ff)))
                p = q
                break
        scans.append(segs)
    return scans


def segments_per_tile(name):
    """restart segments per 256-lane tile of the fused encoders: 256 / blocks per segment"""
    w, h, pf, cs, q, ri, il, sub, _, _ = CASES[name]
    per_mcu = 1 if not il else (4 if pf == 3 else sum(a * b for a, b in sub) if sub else 3)
    return 256 // (ri * per_mcu)


def merge_waves(lib):
    """[waves through gj_merge_stream, waves through gj_merge_tail_only] so far (the execution model's build only)"""
    return np.array(list((C.c_ulonglong * 2).in_dll(lib.L, "gj_emu_enc_merge_waves")), np.int64)


def rgb444_waves(name):
    """waves of k_encode_rgb444 that hold a block, over the three components (each component of each tile is coded by one workgroup, whatever the
    shape of the launch)"""
    w, h, _, _, _, ri, _, _, _, _ = CASES[name]
    nb = ((w + 7) // 8) * ((h + 7) // 8)
    tile = (256 // ri) * ri
    return 3 * sum((min(tile, nb - t) + 63) // 64 for t in range(0, nb, tile))


def encoder(G, lib, monkeypatch, settings):
    """an encoder created under the developer settings (they are taken when a coder is created)"""
    with monkeypatch.context() as mp:
        for k in SETTINGS:
            mp.delenv(k, raising=False)
        for k, v in settings.items():
            mp.setenv(k, v)
        return G.Encoder(lib)


def check_merge_sides(name, content, quality, delta):
    general, tails = int(delta[0]), int(delta[1])
    assert general + tails > 0, name
    if content == "grey":
        assert general == 0, (name, general, tails)
    if content == "noise" and quality == 100:
        assert tails == 0, (name, general, tails)
    if CASES[name][2] == 1 and not CASES[name][6]:  # k_encode_rgb444: the waves are known
        assert general + tails == rgb444_waves(name), (name, general, tails, rgb444_waves(name))


@pytest.mark.parametrize("name", list(CASES))
def test_tile_tail_bytes(O, G, tier, name, monkeypatch):
    """the product's file equals the oracle's, without and with the APP13 segment index (the index holds every segment's position in the file: the
    tile sizes alone place the tiles, seg_bytes[] + seg_ff[] of every single segment place the index entries), on one coder (the second call runs on
    warm buffers); the noise fixtures hold what they are there for; on the execution model the merge took the side the content prescribes"""
    lib, is_emu = tier
    w, h, pf, cs, q, ri, il, sub, content, settings = CASES[name]
    raw, want, want_index = reference(name)
    spt = segments_per_tile(name)
    assert spt in (1, 7, 64), (name, spt)
    scans = scan_segments(want)
    if content == "noise" and spt > 1:
        tiles = [s[t:t + spt] for s in scans for t in range(0, len(s), spt)]
        assert any(sum(1 for ff, _ in t if ff) >= 2 for t in tiles), "the fixture needs a tile with 0xFF bytes in two of its segments"
    enc = encoder(G, lib, monkeypatch, settings)
    for seg_info, expect in ((0, want), (1, want_index)):
        p, pi = api_params(lib, G, case_of(name), segment_info=seg_info)
        before = merge_waves(lib) if is_emu else None
        got = enc.encode(p, pi, raw)
        assert got.size == expect.size and np.array_equal(got, expect), (name, seg_info, got.size, expect.size)
        if is_emu:
            check_merge_sides(name, content, q, merge_waves(lib) - before)
    enc.close()


def test_tile_tail_ff_bytes_at_segment_boundaries():
    """the drain finds the segment of a dword with 0xFF bytes by bisection in the segments' first dwords: the fixture that is there for the two ends
    of that search holds a 0xFF byte in the FIRST dword of a segment that is not its tile's first, and one in the LAST dword of a segment that is not
    its tile's last (test_tile_tail_bytes compares its bytes)"""
    name = "noise_296x16_r4"
    spt = segments_per_tile(name)
    first = last = False
    for scan in scan_segments(reference(name)[1]):
        for t in range(0, len(scan), spt):
            tile = scan[t:t + spt]
            for k, (ff, nbytes) in enumerate(tile):
                first |= k > 0 and any(o < 4 for o in ff)
                last |= k < len(tile) - 1 and any(o >= 4 * ((nbytes - 1) // 4) for o in ff)
    assert first and last


def test_tile_tail_geometry_of_the_cases():
    """the segment geometry the cases are there for, restated from their sizes"""
    def geo(name):
        w, h, _, _, _, ri, _, _, _, _ = CASES[name]
        nb = ((w + 7) // 8) * ((h + 7) // 8)
        spt = 256 // ri
        segs = (nb + ri - 1) // ri
        return nb, spt, segs, segs % spt, nb - (segs - 1) * ri
    assert geo("grey_296x16_r36") == (74, 7, 3, 3, 2)          # a last tile of 3 segments, a last segment of 2 blocks; segment 1 = lanes 36 .. 71
    assert geo("natural_640x368_r36") == (3680, 7, 103, 5, 8)  # tile slack 4 blocks, 5 segments in the last tile
    assert geo("grey_640x368_r4") == (3680, 64, 920, 24, 4)    # segments end on lane 63; the last tile holds 96 blocks
    assert geo("grey_640x368_r200") == (3680, 1, 19, 0, 80)    # tile slack 56 blocks
    assert geo("noise_512x264_r36") == (2112, 7, 59, 3, 24)
    assert geo("noise_296x16_r4") == (74, 64, 19, 19, 2)


def test_tile_tail_batch_of_three(O, G, tier, monkeypatch):
    """encode_batch of three 640x368 frames behind one set of launches (blockIdx.z = frame): a grey, a natural and a noise frame, each equal to the
    oracle's stream; on the execution model the grey frame's waves are the ones on the tails-only side at the least"""
    lib, is_emu = tier
    case = ("batch", 640, 368, 1, 1, 75, 36, 0, None, 3)
    frames = np.stack([pixels(O, c, 640, 368, 1, seed=5) for c in ("grey", "natural", "noise")])
    img = oracle_image(O, case)
    want = [O.encode(img, f) for f in frames]
    p, pi = api_params(lib, G, case)
    enc = encoder(G, lib, monkeypatch, {})
    before = merge_waves(lib) if is_emu else None
    got = enc.encode_batch(p, pi, frames.reshape(-1), 3)
    assert enc.last_batch() == (3, 0)
    for f in range(3):
        assert got[f].size == want[f].size and np.array_equal(got[f], want[f]), f
    if is_emu:
        delta = merge_waves(lib) - before
        per_frame = 3 * (14 * 4 + 3)  # 14 tiles of 252 blocks and one of 152, three components
        assert int(delta.sum()) == 3 * per_frame and int(delta[1]) >= per_frame, list(delta)
    enc.close()
