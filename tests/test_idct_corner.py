"""k_idct_tok_rgb444's corner path: a wave whose Cb and Cr blocks have no coefficient outside natural rows 0 .. 3 x columns 0 .. 3 transforms them
with gj_idct_pk_corner4 (gj_device.h) over half a slot; every other wave, and every wave under GJ_IDCT_DENSE=1, with the full transform. Same bytes.

Streams are built from CHOSEN coefficients (tests/synth_streams.py, oracle.encode_from_coefs) and decoded in token mode (GJ_DEC_TOKENS=1: small
frames take the token path too). Expected output: the oracle's pixels, byte for byte, and the same bytes again under GJ_IDCT_DENSE=1.

Which waves take which side is restated here in Python (corner_waves) from the coefficients alone, and every fixture is asserted to contain the
kinds of waves it is there for. On the CPU tier the execution model's build counts the waves per side (gj_emu_idct_tok_waves, gj_dec_idct.hip,
under GJ_HIPEMU only) and the count must equal the restatement's: "equal bytes" cannot mean "the corner path never ran".

The restatement needs to know where the token decoder's batches end (a wave that holds blocks of two batches has two token ranges and goes the dense
way): GJ_DEC_G=<segments per batch> fixes the plan, with values that put the batch ends on wave boundaries. A batch is decoded as one group as long as
its bytes fit the decoder's stage; the chrominance scans here have a few bytes per block, far below that.

Two tiers with the same bodies, like tests/test_synthetic_streams.py: the CPU tier runs the product's kernels on tests/hipemu, the -m gpu tier the
product library on the MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import synth_streams as S
import test_scaled_decode as SD
from test_region_decode import crop, opt_value
from test_synthetic_streams import SETTINGS, emu  # noqa: F401  (emu: the fixture)

# name: (S.GEOMETRIES' tuple, segments per token batch for GJ_DEC_G, restart interval): blocks per batch = a multiple of the 64 of a wave
GEOS = {
    "rgb_512x16_r8": ((512, 16, 1, 1, 8, 0, None, None), 8, 8),        # 128 block positions: two waves with blocks, two without
    "rgb_640x368_r12": (S.GEOMETRIES["rgb_640x368_r12"], 16, 12),    # 3680 positions: 15 workgroups, a partial last wave, 20 batches per scan
    "rgb_636x364_r12": ((636, 364, 1, 1, 12, 0, None, None), 16, 12),  # the same blocks, edge stores on the right and at the bottom
}
MAIN = "rgb_640x368_r12"
QUALITIES = (100, 75, 1)  # all steps 1, the usual tables, all steps 255
OUTSIDE = (4, 32, 36, 7, 56, 63)  # natural positions just outside the corner, and the far ends of row 0, column 0 and the block
WAVE = 7  # the wave of MAIN that the single coefficients go into (blocks 448 .. 511: inside batch 2 = blocks 384 .. 575)
TOK_STAGE = 832  # GJ_TOK_STAGE (gj_dec_internal.h)
CORNER = np.array([r * 8 + c for r in range(4) for c in range(4)][1:])  # the 15 AC positions of the corner, natural order
SETTINGS_HERE = tuple(SETTINGS) + ("GJ_IDCT_DENSE", "GJ_DEC_G")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def tier(request):
    """(the library of the tier, is it the CPU execution model)"""
    return request.getfixturevalue("emu" if request.param == "emu" else "gpu_lib"), request.param == "emu"


# ================================================================================================ coefficients
def image(geo, quality):
    return S.image(GEOS[geo][0], quality)


def component_blocks(img, coefs, c):
    """[block][natural position] of component c: a VIEW of coefs"""
    k = img.comp[c]
    return coefs[k.data_offset:k.data_offset + k.data_width * k.data_height].reshape(-1, 64)


@functools.lru_cache(maxsize=None)
def corner_only(geo, quality, seed=0, chroma="corner"):
    """Y dense (about 10 AC per block anywhere in the block), Cb and Cr: about 4 AC per block inside the corner, both signs, mostly small, every
    16th value +-511 (the largest a token holds); the corner's edge positions 3, 24 and 27 in every 5th block; every 7th block DC only; blocks 100 .. 109
    without AC in all three components. chroma="anywhere": Cb and Cr like Y (a frame whose waves go the dense way). Read-only."""
    img = image(geo, quality)
    rng = np.random.default_rng(4400 + seed)
    coefs = np.zeros(int(img.data_size), np.int16)
    for c in range(3):
        B = component_blocks(img, coefs, c)
        n = B.shape[0]
        if c == 0 or chroma == "anywhere":
            B[:, 1:] = np.where(rng.random((n, 63)) < 0.16, rng.integers(1, 8, (n, 63)) * rng.choice([-1, 1], (n, 63)), 0)
        else:
            v = rng.integers(1, 8, (n, 15)) * rng.choice([-1, 1], (n, 15))
            v = np.where(rng.random((n, 15)) < 1 / 16, 511 * rng.choice([-1, 1], (n, 15)), v)
            B[:, CORNER] = np.where(rng.random((n, 15)) < 0.27, v, 0)
            B[c::5, 3], B[c::5, 24], B[c::5, 27] = 511, -511, 37
            B[c + 2::7, 1:] = 0
        B[100:110, 1:] = 0
        B[:, 0] = rng.integers(-60, 61, n)
    coefs.setflags(write=False)
    return coefs


@functools.lru_cache(maxsize=None)
def built(geo, quality, key=("corner_only",)):
    """(jpeg, coefficients, the oracle's pixels) of a fixture, read-only. key: ("corner_only",), ("anywhere",),
    ("one", component, block, natural position, value): corner_only with that one coefficient set"""
    if key[0] == "anywhere":
        coefs = corner_only(geo, quality, 1, "anywhere")
    else:
        coefs = corner_only(geo, quality)
        if key[0] == "one":
            coefs = coefs.copy()
            component_blocks(image(geo, quality), coefs, key[1])[key[2], key[3]] = key[4]
            coefs.setflags(write=False)
    jpeg = S.O.encode_from_coefs(image(geo, quality), coefs.copy())
    px = S.O.decode(jpeg)[0]
    for a in (jpeg, px):
        a.setflags(write=False)
    return jpeg, coefs, px


# ================================================================================================ the decision, restated
def corner_waves(geo, quality, coefs):
    """One flag per wave of k_idct_tok_rgb444's grid (workgroups of 256 lanes over the block positions; a wave = 64 consecutive positions,
    lb = 256 x workgroup + thread): does it take the corner side? Per chrominance component the wave's token range must be `fast` (gj_tok_fetch:
    every lane's tokens follow the previous lane's, at most GJ_TOK_STAGE from the 16-byte piece the first one lies in), no block may be in the
    planes (a batch with an |AC| >= 512 goes there as a whole) and no AC coefficient of its blocks may lie in rows 4 .. 7 or columns 4 .. 7.
    Lanes behind the last block carry an empty range at token 0: a wave with blocks and such lanes has a break, a wave of such lanes only has none."""
    img = image(geo, quality)
    _, segs, restart = GEOS[geo]
    nb = (img.comp[0].data_width // 8) * (img.comp[0].data_height // 8)
    waves = 4 * ((nb + 255) // 256)
    flags = np.ones(waves, bool)
    for c in (1, 2):
        A = np.array(component_blocks(img, coefs, c)).reshape(-1, 8, 8)
        assert A.shape[0] == nb
        A[:, 0, 0] = 0
        count = np.count_nonzero(A, (1, 2))
        outside = (A[:, 4:, :] != 0).any((1, 2)) | (A[:, :, 4:] != 0).any((1, 2))
        batch = np.arange(nb) // (segs * restart)
        big = np.abs(A).max((1, 2)) >= 512
        in_planes = np.isin(batch, np.unique(batch[big]))
        for w in range(waves):
            a, b = 64 * w, min(64 * w + 64, nb)
            if a >= nb:
                continue  # no block: 64 empty ranges, nothing outside the corner
            tokens = int(count[a:b][~in_planes[a:b]].sum())
            assert tokens <= TOK_STAGE - 7 or tokens > TOK_STAGE, "the fixture leaves `fast` to the alignment of the wave's first token"
            fast = b - a == 64 and batch[a] == batch[b - 1] and tokens <= TOK_STAGE
            if not fast or in_planes[a:b].any() or outside[a:b].any():
                flags[w] = False
    return flags


# ================================================================================================ decoding
def decoder(G, lib, monkeypatch, geo, dense=False, perf=False):
    """a token-mode decoder with the geometry's batch plan (the developer settings are taken when a decoder is created)"""
    with monkeypatch.context() as mp:
        for k in SETTINGS_HERE:
            mp.delenv(k, raising=False)
        mp.setenv("GJ_DEC_TOKENS", "1")
        mp.setenv("GJ_DEC_G", str(GEOS[geo][1]))
        if dense:
            mp.setenv("GJ_IDCT_DENSE", "1")
        return SD.perf_decoder(G, lib) if perf else G.Decoder(lib)


def wave_counts(lib):
    """[dense, corner] waves of k_idct_tok_rgb444 so far (the execution model's build only)"""
    return np.array(list((C.c_ulonglong * 2).in_dll(lib.L, "gj_emu_idct_tok_waves")), np.int64)


def check(G, tier, monkeypatch, geo, quality, key=("corner_only",), flags=None):
    """the fixture through a decoder that may take the corner side and through one that may not: the oracle's pixels from both, two calls each (the
    second runs on the cached header); on the execution model the first call's waves per side are the restatement's"""
    lib, is_emu = tier
    jpeg, coefs, want = built(geo, quality, key)
    flags = corner_waves(geo, quality, coefs) if flags is None else flags
    for dense in (False, True):
        dec = decoder(G, lib, monkeypatch, geo, dense)
        for rep in range(2):
            before = wave_counts(lib) if is_emu else None
            px = dec.decode(jpeg)[0]
            assert px.size == want.size and np.array_equal(px, want), (geo, quality, key, dense, rep, int(np.count_nonzero(px != want)))
            if is_emu and rep == 0:
                n = int(flags.sum())
                assert list(wave_counts(lib) - before) == ([flags.size, 0] if dense else [flags.size - n, n]), (geo, quality, key, dense)
        dec.close()
    return flags


# ================================================================================================ corner-only chrominance
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("geo", list(GEOS))
def test_corner_only_chroma(O, G, tier, geo, quality, monkeypatch):
    """Chrominance confined to the corner with values of both signs up to +-511, the corner's edge positions 3, 24 and 27, DC-only blocks and blocks
    without AC in any component; luminance dense. Every wave whose 64 positions all hold a block takes the corner side, the partial last wave
    (640x368, 636x364: 32 blocks) the dense one, the waves without a block the corner side."""
    img = image(geo, quality)
    coefs = built(geo, quality)[1]
    for c in (1, 2):
        B = component_blocks(img, coefs, c).reshape(-1, 8, 8)
        assert not B[:, 4:, :].any() and not B[:, :, 4:].any() and B.min() == -511 and B.max() == 511
        flat = B.reshape(-1, 64)
        assert flat[:, 3].any() and flat[:, 24].any() and flat[:, 27].any()
        assert np.count_nonzero(~flat[:, 1:].any(1) & (flat[:, 0] != 0)) >= 10, "DC-only blocks"
    Y = component_blocks(img, coefs, 0).reshape(-1, 8, 8)
    assert Y[:, 4:, 4:].any() and np.count_nonzero(Y) / Y.shape[0] > 8
    assert not any(component_blocks(img, coefs, c)[100:110, 1:].any() for c in range(3))
    flags = check(G, tier, monkeypatch, geo, quality)
    nb = Y.shape[0]
    assert flags[:nb // 64].all() and flags[(nb + 63) // 64:].all() and flags.size > (nb + 63) // 64
    if nb % 64:
        assert not flags[nb // 64]


# ================================================================================================ one coefficient outside the corner
@pytest.mark.parametrize("component", (1, 2), ids=("cb", "cr"))
@pytest.mark.parametrize("position", OUTSIDE)
def test_one_coefficient_outside_the_corner(O, G, tier, position, component, monkeypatch):
    """exactly one chrominance coefficient outside the corner, in the block at lane 0, at lane 63 and in the middle of one wave: that wave goes the
    dense way, its neighbours do not (the entry test must not miss a token of the wave's own blocks, in whichever 16-byte piece it arrives)"""
    quality = QUALITIES[(OUTSIDE.index(position) + component) % 3]
    base = corner_waves(MAIN, quality, built(MAIN, quality)[1])
    assert base[WAVE - 1:WAVE + 2].all()
    for lane in (0, 63, 29):
        key = ("one", component, 64 * WAVE + lane, position, -3 if lane == 29 else 5)
        coefs = built(MAIN, quality, key)[1]
        assert np.count_nonzero(coefs != built(MAIN, quality)[1]) == 1
        flags = corner_waves(MAIN, quality, coefs)
        assert not flags[WAVE] and np.array_equal(np.delete(flags, WAVE), np.delete(base, WAVE))
        check(G, tier, monkeypatch, MAIN, quality, key, flags)


# ================================================================================================ a block through the planes
@pytest.mark.parametrize("component,value", [(1, 700), (2, -512)], ids=("cb", "cr"))
def test_block_through_the_planes(O, G, tier, component, value, monkeypatch):
    """a chrominance coefficient beyond a token's 10 value bits at a corner position of an otherwise corner-only wave: its batch (blocks 384 .. 575,
    waves 6 .. 8) goes through the coefficient planes, the records say so, and those waves take the dense side whatever their tokens say"""
    key = ("one", component, 64 * WAVE + 17, 9, value)
    flags = corner_waves(MAIN, 75, built(MAIN, 75, key)[1])
    base = corner_waves(MAIN, 75, built(MAIN, 75)[1])
    assert list(np.flatnonzero(base & ~flags)) == [WAVE - 1, WAVE, WAVE + 1] and not (flags & ~base).any()
    check(G, tier, monkeypatch, MAIN, 75, key, flags)


# ================================================================================================ batch call, partial last wave
def test_partial_last_wave_in_a_batch_call(O, G, tier, monkeypatch):
    """decode_batch of 640x368 frames with one header, corner-only ones and one whose chrominance lies anywhere in the block; 3680 positions = 57
    whole waves, one of 32 blocks and two without any per frame. Three frames, because the call decodes frame 0 by itself ahead of the batched
    launches: the last two, one of each kind, are the 2-frame batch (blockIdx.z = frame)."""
    lib, is_emu = tier
    frames = [built(MAIN, 75), built(MAIN, 75, ("anywhere",)), built(MAIN, 75)]
    flags = [corner_waves(MAIN, 75, f[1]) for f in frames]
    assert flags[0][:57].all() and not flags[0][57] and flags[0][58:].all() and flags[0].size == 60
    assert not flags[1][:58].any() and flags[1][58:].all()
    for dense in (False, True):
        dec = decoder(G, lib, monkeypatch, MAIN, dense)
        for rep in range(2):
            before = wave_counts(lib) if is_emu else None
            got, pi = dec.decode_batch([f[0] for f in frames])
            assert (pi.width, pi.height) == (640, 368) and dec.last_batch() == (2, 1)
            for i, (px, f) in enumerate(zip(got, frames)):
                assert np.array_equal(px, f[2]), (dense, rep, i, int(np.count_nonzero(px != f[2])))
            if is_emu:
                n = int(sum(f.sum() for f in flags))
                assert list(wave_counts(lib) - before) == ([180, 0] if dense else [180 - n, n]), (dense, rep)
        dec.close()


# ================================================================================================ region and reduced-size calls
def test_region_and_reduced_size_calls_stay_dense(O, G, tier, monkeypatch):
    """the corner-only stream through the token-fed region kernel and the token-fed reduced-size kernels: their existing definitions (a crop of the
    oracle's pixels; tests/test_scaled_decode.py's reduced image), and no wave of k_idct_tok_rgb444 is counted for them"""
    lib, is_emu = tier
    jpeg, _, full = built(MAIN, 75)
    dec = decoder(G, lib, monkeypatch, MAIN, perf=True)
    before = wave_counts(lib) if is_emu else None
    for reg in [(0, 0, 640, 368), (213, 123, 161, 93), (627, 357, 13, 11)]:
        assert dec.set_option("dec_opt_region", opt_value(reg)) == 0
        px = dec.decode(jpeg)[0]
        assert dec.idct_path() == 4 and np.array_equal(px, crop(full, 640, 368, 1, reg)), reg
    assert dec.set_option("dec_opt_region", "full") == 0
    for s in SD.SCALES:
        assert dec.set_option("dec_opt_scale", f"1/{s}") == 0
        px = dec.decode(jpeg)[0]
        assert dec.idct_path() == 2 and np.array_equal(px, SD.expected(O, jpeg, -1, -1, s)[0]), s
    if is_emu:
        assert list(wave_counts(lib) - before) == [0, 0]
    assert dec.set_option("dec_opt_scale", "1") == 0
    px = dec.decode(jpeg)[0]
    assert dec.idct_path() == 0 and np.array_equal(px, full)
    if is_emu:
        assert list(wave_counts(lib) - before) == [1, 59]
    dec.close()
