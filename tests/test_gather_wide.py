"""k_gather (gpujpeg_amd/csrc/gj_enc_assemble.hip): a wave takes one tile stream on its own (scalar set-up, two wave reductions for its place in the
file, no workgroup barrier), and a lane takes FOUR consecutive dwords of the stream a round: one 16-byte load, the four bytes LDS holds for them (a
segment notes at its last dword the bytes that do not count and its restart marker), one wave prefix sum of the lanes' output bytes, one 16-byte store
for a lane whose dwords are whole and free of 0xFF, dword stores and byte-by-byte turns for the others.

Every case compares the product's JPEG bytes with the oracle's: the file holds every stream byte, every stuffed zero, every RSTn, the scan headers
and the EOI, and the returned size is the result word. The shapes are the ones at which this kernel can go wrong; test_gather_wide_shapes_occur ASSERTS
from the oracle's streams that each of them occurs in the case that is there for it (the segment parser of tests/test_encoder_tile_tail.py restated,
the tile / round / lane geometry of the kernel restated from the sizes): "equal bytes" cannot mean "the shape never came up". The noise seeds follow
from the cases' sizes (reference()); which case holds which shape was found with the oracle on the CPU and is written down in SHAPES.

Two tiers with the same bodies: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the product library on the MI355X."""
import functools

import numpy as np
import pytest

from conftest import api_params, natural_image, oracle_image
from test_synthetic_streams import emu  # noqa: F401  (the fixture)

S420 = ((2, 2), (1, 1), (1, 1))
WHOLE, ONE, TAIL = {"GJ_ENC_SPLIT": "0"}, {"GJ_ENC_SPLIT": "100000"}, {"GJ_ENC_SPLIT": "0", "GJ_ENC_TAIL": "2"}
SETTINGS = ("GJ_ENC_SPLIT", "GJ_ENC_TAIL")
ROUND_DW, LANE_DW, MARK_DW = 256, 4, 2048  # dwords a wave takes a round, a lane takes a round, LDS holds notes for at a time

# id: (w, h, pixel format, colour space, quality, restart interval, interleaved, subsampling, content, developer settings)
CASES = {
    # ---- behind k_encode_rgb444 (three scans: the second and third begin with a header copy)
    "grey_64x16_r36": (64, 16, 1, 1, 75, 36, 0, None, "grey", WHOLE),            # 16 blocks, one segment: a tile stream of 3 (Y) and 2 (Cb, Cr) dwords
    "grey_296x16_r36": (296, 16, 1, 1, 75, 36, 0, None, "grey", WHOLE),          # one tile of 3 segments a scan (the issue names it for "at most 4 dwords": it has 15 and 11)
    "grey_640x368_r4": (640, 368, 1, 1, 75, 4, 0, None, "grey", WHOLE),          # tiles of 64 one-dword segments: every dword is followed by RSTn; last tile 24 segments
    "natural_640x368_r36": (640, 368, 1, 1, 75, 36, 0, None, "natural", WHOLE),  # 15 tiles a scan (45: a workgroup with one wave), the ordinary case
    "natural_q95_640x368_r36": (640, 368, 1, 1, 95, 36, 0, None, "natural", WHOLE),  # tile streams of more than 512 dwords
    "noise_512x264_r36": (512, 264, 1, 1, 100, 36, 0, None, "noise", WHOLE),     # tile streams of ~6000 dwords: three passes of the LDS notes; 27 tiles
    "noise_296x16_r4": (296, 16, 1, 1, 100, 4, 0, None, "noise", WHOLE),         # 19 segments in one tile, many 0xFF bytes
    "noise_296x16_r200": (296, 16, 1, 1, 100, 200, 0, None, "noise", WHOLE),     # one segment a tile
    # ---- its one-component launch shape and its split tail
    "one_noise_296x16_r36": (296, 16, 1, 1, 100, 36, 0, None, "noise", ONE),
    "one_natural_636x364_r36": (636, 364, 1, 1, 75, 36, 0, None, "natural", ONE),
    "tail_natural_640x368_r36": (640, 368, 1, 1, 75, 36, 0, None, "natural", TAIL),
    "tail_noise_512x264_r36": (512, 264, 1, 1, 100, 36, 0, None, "noise", TAIL),
    # ---- behind k_encode_uyvy422: one interleaved scan
    "uyvy_noise_264x50_r9": (264, 50, 3, 3, 90, 9, 1, None, "noise", {}),        # 14 segments: two tiles (a workgroup with two waves)
    "uyvy_noise_q100_296x16_r9": (296, 16, 3, 3, 100, 9, 1, None, "noise", {}),
    # ---- behind k_encode_blocks: planar 4:2:0, three scans of different sizes
    "planar420_noise_322x114_r36": (322, 114, 5, 3, 100, 36, 0, None, "noise", {}),  # 3 + 1 + 1 tiles
    "planar420_noise_322x114_r4": (322, 114, 5, 3, 100, 4, 0, None, "noise", {}),
    "planar420_grey_320x112_r36": (320, 112, 5, 3, 75, 36, 0, None, "grey", {}),
}

# noise seeds: the rule below (they follow from the size) gave every shape with the oracle on the CPU, so no case needs a seed of its own; one
# that does is written down here
SEEDS = {}

# what each case is there for: asserted from the oracle's stream of that case
SHAPES = {
    "grey_64x16_r36": {"tile of at most 4 dwords"},
    "grey_640x368_r4": {"tile of 64 one-dword segments", "segment ends inside a lane's four dwords"},
    "natural_640x368_r36": {"tile dwords a multiple of 4", "tile dwords no multiple of 4", "tile of more than 256 dwords", "tiles % 4 == 1",
                            "segment ends inside a lane's four dwords", "three scans"},
    "natural_q95_640x368_r36": {"tile of more than 512 dwords", "round without 0xFF next to a round with one"},
    "noise_512x264_r36": {"tile of more than 2048 dwords", "tiles % 4 == 3", "two 0xFF in one dword", "0xFF in a lane's fourth dword"},
    "noise_296x16_r4": {"0xFF in a segment's last byte, RSTn behind it", "two 0xFF in one dword",
                        "0xFF in a lane's fourth dword", "segment ends inside a lane's four dwords", "tiles % 4 == 3"},
    "uyvy_noise_264x50_r9": {"tiles % 4 == 2", "one scan"},
    "planar420_noise_322x114_r36": {"three scans", "tiles % 4 == 1", "scans of different tile counts"},
    "planar420_noise_322x114_r4": {"0xFF in a segment's first byte", "0xFF in a segment's last byte, RSTn behind it", "tile of more than 2048 dwords"},
}


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request):
    """the library of the tier"""
    return request.getfixturevalue("emu" if request.param == "emu" else "gpu_lib")


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
    return O.noise(n, seed=seed)  # the reference's test-image noise, oracle.noise


@functools.lru_cache(maxsize=None)
def reference(name):
    """(raw pixels, the oracle's JPEG) of a case, computed once, read-only"""
    import oracle as O
    w, h, pf, cs, q, ri, il, sub, content, _ = CASES[name]
    raw = pixels(O, content, w, h, pf, seed=SEEDS.get(name, w * 7 + h + ri))
    want = O.encode(oracle_image(O, case_of(name)), raw)
    raw.setflags(write=False)
    want.setflags(write=False)
    return raw, want


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


def shapes(name):
    """what k_gather meets in the oracle's stream of a case: a tile stream is the segments of a tile back to back, each on a dword boundary; dword d
    of it is taken in round d // 256 by lane d % 256 // 4 as its dword d % 4"""
    spt = segments_per_tile(name)
    scans = scan_segments(reference(name)[1])
    tiles = [(si, s[t:t + spt], t + spt >= len(s)) for si, s in enumerate(scans) for t in range(0, len(s), spt)]
    found = {"one scan" if len(scans) == 1 else "three scans" if len(scans) == 3 else "?"}
    found.add("tiles %% 4 == %d" % (len(tiles) % 4))
    if len({(len(s) + spt - 1) // spt for s in scans}) > 1:
        found.add("scans of different tile counts")
    for _, tile, scan_ends in tiles:
        ndw = [(nbytes + 3) // 4 for _, nbytes in tile]
        total = sum(ndw)
        found.add("tile dwords a multiple of 4" if total % LANE_DW == 0 else "tile dwords no multiple of 4")
        for limit in (ROUND_DW, 2 * ROUND_DW, MARK_DW):
            if total > limit:
                found.add("tile of more than %d dwords" % limit)
        if total <= LANE_DW:
            found.add("tile of at most 4 dwords")
        if len(tile) == 64 and all(n == 1 for n in ndw):
            found.add("tile of 64 one-dword segments")
        round_ff = [0] * ((total + ROUND_DW - 1) // ROUND_DW)
        base = 0
        for k, ((ff, nbytes), n) in enumerate(zip(tile, ndw)):
            rst_follows = not (scan_ends and k == len(tile) - 1)
            if k < len(tile) - 1 and (base + n) % LANE_DW != 0:
                found.add("segment ends inside a lane's four dwords")
            if ff and ff[-1] == nbytes - 1 and rst_follows:
                found.add("0xFF in a segment's last byte, RSTn behind it")
            if ff and ff[0] == 0:
                found.add("0xFF in a segment's first byte")
            dws = [base + o // 4 for o in ff]
            if len(dws) != len(set(dws)):
                found.add("two 0xFF in one dword")
            for d in dws:
                round_ff[d // ROUND_DW] += 1
                if d % LANE_DW == 3 and d % ROUND_DW != ROUND_DW - 1 and d + 1 < total:
                    found.add("0xFF in a lane's fourth dword")
            base += n
        if any((a == 0) != (b == 0) for a, b in zip(round_ff, round_ff[1:])):
            found.add("round without 0xFF next to a round with one")
    return found


def encoder(G, lib, monkeypatch, settings):
    """an encoder created under the developer settings (they are taken when a coder is created)"""
    with monkeypatch.context() as mp:
        for k in SETTINGS:
            mp.delenv(k, raising=False)
        for k, v in settings.items():
            mp.setenv(k, v)
        return G.Encoder(lib)


@pytest.mark.parametrize("name", list(CASES))
def test_gather_wide_bytes(O, G, tier, name, monkeypatch):
    """the product's file equals the oracle's, twice on one coder (the second call runs on warm buffers and on the other set of group totals)"""
    raw, want = reference(name)
    enc = encoder(G, tier, monkeypatch, CASES[name][9])
    p, pi = api_params(tier, G, case_of(name))
    for call in range(2):
        got = enc.encode(p, pi, raw)
        assert got.size == want.size and np.array_equal(got, want), (name, call, got.size, want.size)
    enc.close()


def test_gather_wide_batch_of_three(O, G, tier, monkeypatch):
    """encode_batch of three 640x368 frames behind one set of launches (blockIdx.z = frame): a grey, a natural and a noise frame, each equal to the
    oracle's stream"""
    case = ("batch", 640, 368, 1, 1, 75, 36, 0, None, 3)
    frames = np.stack([pixels(O, c, 640, 368, 1, seed=5) for c in ("grey", "natural", "noise")])
    img = oracle_image(O, case)
    want = [O.encode(img, f) for f in frames]
    p, pi = api_params(tier, G, case)
    enc = encoder(G, tier, monkeypatch, {})
    got = enc.encode_batch(p, pi, frames.reshape(-1), 3)
    assert enc.last_batch() == (3, 0)
    for f in range(3):
        assert got[f].size == want[f].size and np.array_equal(got[f], want[f]), f
    enc.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_gather_wide_shapes_occur(name):
    """the oracle's stream of the case holds the shapes the case is there for (test_gather_wide_bytes compares its bytes)"""
    found = shapes(name)
    assert SHAPES[name] <= found, (name, sorted(SHAPES[name] - found))


def test_gather_wide_every_shape_has_a_case():
    """the list of the shapes this kernel can go wrong at, against what the cases claim (each claim is asserted above); the feeders and launch shapes
    follow from the cases' formats and developer settings"""
    claimed = set().union(*SHAPES.values())
    wanted = {"tile of at most 4 dwords", "tile of 64 one-dword segments", "tile dwords a multiple of 4", "tile dwords no multiple of 4",
              "tile of more than 256 dwords", "tile of more than 512 dwords", "tile of more than 2048 dwords", "segment ends inside a lane's four dwords",
              "0xFF in a segment's last byte, RSTn behind it", "0xFF in a segment's first byte", "two 0xFF in one dword", "0xFF in a lane's fourth dword",
              "round without 0xFF next to a round with one", "three scans", "one scan", "tiles % 4 == 1", "tiles % 4 == 2", "tiles % 4 == 3",
              "scans of different tile counts"}
    assert wanted <= claimed, sorted(wanted - claimed)
    formats = {(CASES[n][2], CASES[n][6]) for n in CASES}
    assert {(1, 0), (3, 1), (5, 0)} <= formats  # k_encode_rgb444, k_encode_uyvy422, k_encode_blocks on planar 4:2:0
    assert any(CASES[n][9] == ONE for n in CASES) and any(CASES[n][9] == TAIL for n in CASES)
