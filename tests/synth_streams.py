"""Baseline streams built from CHOSEN coefficients, tables and table maps (helper module of tests/test_synthetic_streams.py; no fixtures here).

Almost every stream the other suites decode is an image pushed through the oracle's encoder, so the coefficients, the Huffman tables, the table
slots and the component -> table maps are the ones that construction happens to give. Here they are chosen:
  - coefficient generators (seeded; int16 arrays in the oracle's plane layout: component after component, block after block in raster order,
    64 coefficients per block in natural [row][column] order) that stay inside the baseline-legal domain -- |AC| <= 1023, DC in [-1024, 1016]
    so that DC differences reach size 11 -- and that oracle.encode_from_coefs turns into a stream with the Annex K tables;
  - recode(): a Python re-coder that parses the symbols of such a stream (scan_symbols of tests/test_huffman_optimal.py) and writes them again
    with other Huffman tables, table slots, component -> table maps, DHT layouts and quantisation tables. The coefficients do not change.
No product code is used, and nothing of the reference tree. The generated streams are cached per process (both tiers decode the same ones) and
returned read-only."""
import collections
import functools

import numpy as np

import oracle as O
from test_huffman_optimal import canonical, optimal_table, scan_symbols, segments_of, subtables  # noqa: F401  (subtables: re-exported)

ZIGZAG = []  # (row, column) of zig-zag position k
for _sd in range(15):
    _cells = [(i, _sd - i) for i in range(_sd + 1) if i < 8 and _sd - i < 8]
    ZIGZAG += _cells if _sd % 2 else _cells[::-1]
NATURAL_OF_ZIGZAG = np.array([r * 8 + c for r, c in ZIGZAG])  # index inside a block of the planes of zig-zag position k

BIG = (512, -512, 1023, -1023, 511, -511, 700)  # both sides of the token decoder's 10 value bits (|v| >= 512 does not fit) and the largest legal AC


def zigzag_blocks(coefs):
    """planes -> [block][zig-zag position] (a copy)"""
    return np.asarray(coefs, np.int16).reshape(-1, 64)[:, NATURAL_OF_ZIGZAG].copy()


def to_planes(Z):
    c = np.empty_like(Z)
    c[:, NATURAL_OF_ZIGZAG] = Z
    return c.reshape(-1)


# ================================================================================================ geometries
# name: (width, height, pixel format, colour space, restart interval, interleaved, subsampling, output (pixel format, colour space) or None)
GEOMETRIES = {
    "rgb_640x368_r12": (640, 368, 1, 1, 12, 0, None, None),     # 3 x 307 segments: several token batches per scan, the token-fed kernels
    "rgb_320x64_r1": (320, 64, 1, 1, 1, 0, None, None),
    "rgb_200x120_r0": (200, 120, 1, 1, 0, 0, None, None),
    "420_il_322x242_r3": (322, 242, 1, 1, 3, 1, ((2, 2), (1, 1), (1, 1)), None),
    "uyvy_il_322x50": (322, 50, 3, 3, 2, 1, None, (3, 3)),
    "grey_333x111": (333, 111, 0, 3, 5, 0, None, None),
    "rgb_8x8": (8, 8, 1, 1, 4, 0, None, None),
}


def image(geometry, quality):
    w, h, pf, cs, ri, il, ss, _ = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    return O.make_image(w, h, pixel_format=pf, color_space=cs, quality=quality, restart_interval=ri, interleaved=il,
                        subsampling=None if ss is None else [tuple(x) for x in ss])


def output_format(geometry):
    """(pixel format, colour space) the tests ask the decoders for: None = the decoder's default"""
    return GEOMETRIES[geometry][7]


# ================================================================================================ coefficient generators
def _blocks(img):
    return int(img.data_size) // 64


def sparse(img, seed=0, density=0.08, dc=60):
    """the background: about 8 % non-zero small AC coefficients, a moderate DC"""
    rng = np.random.default_rng(seed)
    n = _blocks(img)
    Z = np.zeros((n, 64), np.int16)
    vals = rng.integers(1, 8, (n, 63)) * rng.choice([-1, 1], (n, 63))
    Z[:, 1:] = np.where(rng.random((n, 63)) < density, vals, 0)
    Z[:, 0] = rng.integers(-dc, dc + 1, n)
    return to_planes(Z)


def with_big(coefs, n, values=BIG, seed=0):
    """plants n coefficients of `values` at random blocks and AC positions (n >= the number of blocks: one in every block)"""
    rng = np.random.default_rng(1000 + seed)
    Z = zigzag_blocks(coefs)
    nb = Z.shape[0]
    blocks = np.arange(nb) if n >= nb else rng.choice(nb, n, replace=False)
    Z[blocks, rng.integers(1, 64, blocks.size)] = rng.choice(values, blocks.size)
    return to_planes(Z)


def shapes(coefs, seed=0):
    """a handful of blocks of each kind: all 63 AC non-zero (no EOB), only position 63 (three ZRL), only position 1, an empty block next to a
    full one, runs of exactly 15 (symbols 0xF1..) and of exactly 16 (ZRL + run 0)"""
    rng = np.random.default_rng(2000 + seed)
    Z = zigzag_blocks(coefs)
    nb = Z.shape[0]

    def value():
        return int(rng.integers(1, 40)) * int(rng.choice([-1, 1]))

    def full(b):
        Z[b, 1:] = rng.integers(1, 6, 63) * rng.choice([-1, 1], 63)

    def only(b, positions):
        Z[b, 1:] = 0
        for p in positions:
            Z[b, p] = value()

    for anchor in range(4):
        b = nb * anchor // 4
        kinds = [full, lambda b: only(b, [63]), lambda b: only(b, [1]), lambda b: only(b, []), full, lambda b: only(b, [1, 17, 33, 49]),
                 lambda b: only(b, [1, 18, 35, 52]), lambda b: only(b, [16]), lambda b: only(b, [17])]
        for i, kind in enumerate(kinds):
            kind((b + i) % nb)
    return to_planes(Z)


def _magnitude(rng, size):
    v = int(rng.integers(1 << (size - 1), 1 << size))
    return v if rng.random() < 0.5 else -v


def _dc_walk(rng, sizes):
    """DC values whose differences (in plane order, from 0) have the given sizes wherever a value of [-1024, 1016] allows it"""
    out, cur = [], 0
    for s in sizes:
        d = int(rng.integers(1 << (s - 1), 1 << s)) if s else 0
        order = (d, -d) if rng.random() < 0.5 else (-d, d)
        for step in order + ((1 << s) >> 1, -((1 << s) >> 1)):  # (then the smallest difference of the size)
            if -1024 <= cur + step <= 1016:
                cur += step
                break
        out.append(cur)
    return out


def every_symbol(img, seed=0):
    """every AC symbol (run 0..15 x size 1..10, ZRL, EOB) and every DC size 0..11, with strongly skewed frequencies (geometric run / size draw): an
    optimal table without the decoder-fit rule is deep"""
    rng = np.random.default_rng(3000 + seed)
    n = _blocks(img)
    Z = np.zeros((n, 64), np.int16)
    b, k = 0, 1
    for r in range(16):  # once each, packed into the first blocks
        for s in range(1, 11):
            if k + r > 63:
                b, k = b + 1, 1
            Z[b % n, k + r] = _magnitude(rng, s)
            k += r + 1
    Z[(b + 1) % n, 40] = _magnitude(rng, 3)  # two ZRL
    pr = 0.5 ** np.arange(16)
    ps = 0.5 ** np.arange(10)
    R = rng.choice(16, n * 24 + 64, p=pr / pr.sum())
    S = 1 + rng.choice(10, n * 24 + 64, p=ps / ps.sum())
    stop = rng.random(n * 24 + 64) < 0.06
    i = 0
    for b in range(b + 2, n):
        k = 1
        for _ in range(24):
            r = int(R[i])
            if k + r > 63 or stop[i]:
                i += 1
                break
            Z[b, k + r] = _magnitude(rng, int(S[i]))
            k += r + 1
            i += 1
    pd = 0.5 ** np.arange(12)
    sizes = list(range(11, -1, -1)) + [int(x) for x in rng.choice(12, max(0, n - 12), p=pd / pd.sum())]  # (every size once, from a difference of -1024)
    Z[:, 0] = _dc_walk(rng, sizes[:n])
    return to_planes(Z)


FEW = [(0, 1), (0, 2), (1, 1), (0, 3), (2, 1), (0, 10), (1, 2), (0, 9), (3, 1), (15, 1), (0, 4), (5, 2), (0, 5), (0, 6)]  # + EOB + ZRL = 16 AC symbols


def few_symbols(img, seed=0):
    """at most 16 different AC symbols (FEW, EOB, ZRL), skewed: a code with one word of every length 1..16 can hold them"""
    rng = np.random.default_rng(4000 + seed)
    n = _blocks(img)
    Z = np.zeros((n, 64), np.int16)
    p = 0.6 ** np.arange(len(FEW))
    P = rng.choice(len(FEW), n * 12, p=p / p.sum())
    i = 0
    for b in range(n):
        k = 1
        if b % 97 == 5:  # ZRL: two of them, then (0, 1)
            Z[b, 33] = 1
            continue
        if b < 2 * len(FEW):  # every symbol at least once
            r, s = FEW[b % len(FEW)]
            Z[b, 1 + r] = _magnitude(rng, s)
            continue
        for _ in range(int(rng.integers(0, 12))):
            r, s = FEW[int(P[i])]
            i += 1
            if k + r > 63:
                break
            Z[b, k + r] = _magnitude(rng, s)
            k += r + 1
    Z[:, 0] = rng.integers(-30, 31, n)
    return to_planes(Z)


def dc_extremes(coefs):
    """DC alternating -1024 / +1016 from block to block: differences of size 11"""
    Z = zigzag_blocks(coefs)
    Z[:, 0] = np.where(np.arange(Z.shape[0]) % 2 == 0, -1024, 1016)
    return to_planes(Z)


def low_frequency_extremes(img, seed=0, top=1023):
    """|AC| = top at the low-frequency positions and extreme DC values: with steps of 255 (quality 1) every corner the reduced-size decode uses
    -- 8x8, 4x4, 2x2 and the DC alone -- holds products beyond +-32767"""
    rng = np.random.default_rng(5000 + seed)
    n = _blocks(img)
    c = np.zeros((n, 8, 8), np.int16)
    dc = rng.choice([-1024, 1016, 300, -300, 129, -129, 128, -128, 5], n)  # (128 x 255 = 32640 stays inside, 129 x 255 = 32895 does not)
    for b in range(n):
        kind = b % 4
        if kind == 3:
            continue  # the DC alone
        m = (2, 4, 8)[kind]
        k = int(rng.integers(1, 6))
        c[b, rng.integers(0, m, k), rng.integers(0, m, k)] = rng.choice([top, -top, 129, -128, min(top, 640)], k)
    c[:, 0, 0] = dc
    return c.reshape(-1)


GENERATORS = {
    "sparse": lambda img: sparse(img),
    "big_1": lambda img: with_big(sparse(img), 1),
    "big_5": lambda img: with_big(sparse(img), 5),
    "big_dense": lambda img: with_big(sparse(img), 1 << 30),
    "shapes": lambda img: shapes(sparse(img)),
    "every_symbol": lambda img: every_symbol(img),
    "dc_extremes": lambda img: dc_extremes(sparse(img)),
    "few_symbols": lambda img: few_symbols(img),
    "low_frequency_extremes": lambda img: low_frequency_extremes(img),
    "low_frequency_511": lambda img: low_frequency_extremes(img, top=511),  # (every value fits a token: no batch of a token-mode frame leaves it)
    "every_symbol_other": lambda img: every_symbol(img, seed=1),
    "sparse_other": lambda img: sparse(img, seed=77),  # another frame of the same header without any big value
}


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def coefficients(geometry, generator, quality=100):
    return _frozen(GENERATORS[generator](image(geometry, quality)))


@functools.lru_cache(maxsize=None)
def stream(geometry, generator, quality=100):
    """the oracle's stream (Annex K tables) of the generator's coefficients -> (jpeg, coefficients), both read-only"""
    coefs = coefficients(geometry, generator, quality)
    return _frozen(O.encode_from_coefs(image(geometry, quality), coefs.copy())), coefs


# ================================================================================================ tables for recode()
def unrestricted(cls, tid, freq):
    """the optimal table of the counts, code lengths limited to 16 only (no decoder-fit rule)"""
    return optimal_table(freq, 16)[:2]


def fitted(cls, tid, freq):
    """the optimal table under the decoder-fit rule (what enc_opt_huffman=optimal writes)"""
    return optimal_table(freq)[:2]


def fixed_length(cls, tid, freq):
    """every used symbol at 8 bits (DC: 4 bits)"""
    used = [s for s in range(256) if freq[s]]
    bits = [0] * 17
    bits[4 if cls == 0 else 8] = len(used)
    assert len(used) < (16 if cls == 0 else 256)
    return bits, used


def skewed(cls, tid, freq):
    """one code of every length 1, 2, 3, ...: the most frequent symbol first; 16 symbols end with the one 16-bit code 1111111111111110"""
    used = sorted((s for s in range(256) if freq[s]), key=lambda s: (-int(freq[s]), s))
    assert len(used) <= 16, len(used)
    return [0] + [1] * len(used) + [0] * (16 - len(used)), used


ANNEX_K = None  # tables=: the stream's own tables unchanged (id parity picks luminance / chrominance)

QUANT_ALL_255 = {"tables": {0: [255] * 64, 1: [255] * 64}, "map": None}
QUANT_MIXED = {"tables": {0: [1 if (i * 7) % 3 else 255 for i in range(64)], 1: [255 if (i * 5) % 4 else 1 for i in range(64)]}, "map": None}
QUANT_SLOTS_123 = {"tables": {1: [1 + (i % 5) for i in range(64)], 2: [255 - 3 * i for i in range(64)], 3: [2] * 64}, "map": [1, 2, 3]}


# ================================================================================================ the re-coder
def recode(jpeg, tables=ANNEX_K, slots=None, table_map=None, dht_layout="separate", quant=None):
    """The baseline stream `jpeg` with the same symbols in the same order, written again:
      tables      callable (class, id, counts[256]) -> (BITS[0..16], HUFFVAL) that makes the table of a slot from the counts of the symbols coded
                  with it; ANNEX_K keeps the stream's tables (slot id & 1 picks the luminance or the chrominance one)
      slots       {old id: new id}: moves DHT ids and SOS selectors
      table_map   [(dc id, ac id)] per component of the frame, replaces the selectors altogether
      dht_layout  "separate": one DHT segment per table; "single": all tables in one segment
      quant       {"tables": {slot: 64 steps in DQT order}, "map": [slot per component] or None}: rewrites the DQT payloads and SOF0's Tq
    Every DHT goes where the first one was. The APP13 index is dropped; byte stuffing, restart markers and 1-padding as the encoder writes them."""
    segs = segments_of(jpeg)
    syms = scan_symbols(jpeg)
    comps, orig, scans = [], {}, []
    for m, pl, _ in segs:
        if m == 0xC0:
            comps = [(pl[6 + 3 * k], pl[7 + 3 * k] >> 4, pl[7 + 3 * k] & 15) for k in range(pl[5])]
        elif m == 0xC4:
            p = 0
            while p < len(pl):
                bits = [0] + list(pl[p + 1:p + 17])
                orig[(pl[p] >> 4, pl[p] & 15)] = (bits, list(pl[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDA:
            scans.append([(pl[1 + 2 * k], pl[2 + 2 * k] >> 4, pl[2 + 2 * k] & 15) for k in range(pl[0])])
    index = {cid: i for i, (cid, _, _) in enumerate(comps)}
    sel = {}
    for sc in scans:
        for cid, td, ta in sc:
            sel[index[cid]] = ((slots or {}).get(td, td), (slots or {}).get(ta, ta))
    if table_map is not None:
        sel = {i: tuple(table_map[i]) for i in sel}
    # every symbol's new table: a DC symbol opens a block, the blocks of a segment cycle through the scan's MCU layout
    freq, assigned = {}, []
    for sc, scan_syms in zip(scans, syms):
        layout = [index[cid] for cid, _, _ in sc for _ in range(comps[index[cid]][1] * comps[index[cid]][2] if len(sc) > 1 else 1)]
        scan_out = []
        for seg in scan_syms:
            blk, out = -1, []
            for (cls, _), s, v, n in seg:
                blk += cls == 0
                key = (cls, sel[layout[blk % len(layout)]][cls])
                freq.setdefault(key, np.zeros(256, np.int64))[s] += 1
                out.append((key, s, v, n))
            scan_out.append(out)
        assigned.append(scan_out)
    new = {}
    for key in sorted(freq):
        if tables is ANNEX_K:
            new[key] = orig.get((key[0], key[1] & 1)) or orig[(key[0], 0)]
        else:
            bits, vals = tables(key[0], key[1], freq[key])
            new[key] = ([int(b) for b in bits], [int(v) for v in vals])
    words = {key: {s: format(c, f"0{L}b") for s, (c, L) in canonical(*t).items()} for key, t in new.items()}

    def segment(m, pl):
        return bytes([0xFF, m, (len(pl) + 2) >> 8, (len(pl) + 2) & 255]) + bytes(pl)

    out, si, dht_done, dqt_done = bytearray(), 0, False, False
    for m, pl, _ in segs:
        if m == 0xED:
            continue
        if pl is None:
            out += bytes([0xFF, m])
            continue
        if m == 0xC4:
            if not dht_done:
                payloads = [bytes([(cls << 4) | tid] + new[(cls, tid)][0][1:17] + new[(cls, tid)][1]) for cls, tid in sorted(new, key=lambda k: (k[1], k[0]))]
                for pl2 in ([b"".join(payloads)] if dht_layout == "single" else payloads):
                    out += segment(0xC4, pl2)
                dht_done = True
            continue
        if m == 0xDB and quant is not None:
            if not dqt_done:
                for slot, steps in sorted(quant["tables"].items()):
                    assert len(steps) == 64 and all(1 <= x <= 255 for x in steps)
                    out += segment(0xDB, bytes([slot] + list(steps)))
                dqt_done = True
            continue
        if m == 0xC0 and quant is not None and quant["map"] is not None:
            pl = bytearray(pl)
            for k, slot in enumerate(quant["map"][:pl[5]]):
                pl[8 + 3 * k] = slot
        if m == 0xDA:
            ns = pl[0]
            pl = bytes([ns] + [x for k in range(ns) for x in (pl[1 + 2 * k], (sel[index[pl[1 + 2 * k]]][0] << 4) | sel[index[pl[1 + 2 * k]]][1])]) + pl[1 + 2 * ns:]
        out += segment(m, pl)
        if m == 0xDA:
            for k, seg in enumerate(assigned[si]):
                if k:
                    out += bytes([0xFF, 0xD0 + (k - 1) % 8])
                s = "".join(words[key][sym] + (format(v, "b").zfill(n) if n else "") for key, sym, v, n in seg)
                s += "1" * (-len(s) % 8)
                out += int(s, 2).to_bytes(len(s) // 8, "big").replace(b"\xff", b"\xff\x00") if s else b""
            si += 1
    return np.frombuffer(bytes(out), np.uint8)


def dht_tables(jpeg):
    """[(class, id, BITS, HUFFVAL)] of every table of the stream, and the number of DHT segments"""
    out, n = [], 0
    for m, pl, _ in segments_of(jpeg):
        if m == 0xC4:
            n += 1
            p = 0
            while p < len(pl):
                bits = [0] + list(pl[p + 1:p + 17])
                out.append((pl[p] >> 4, pl[p] & 15, bits, list(pl[p + 17:p + 17 + sum(bits)])))
                p += 17 + sum(bits)
    return out, n


def symbol_sizes(jpeg):
    """({AC symbols}, {DC symbols}) per table id that the stream's scans use: {id: set}"""
    ac, dc = {}, {}
    for scan in scan_symbols(jpeg):
        for seg in scan:
            for (cls, tid), s, _, _ in seg:
                (ac if cls else dc).setdefault(tid, set()).add(s)
    return ac, dc


TABLES = {"annex_k": ANNEX_K, "unrestricted": unrestricted, "fitted": fitted, "fixed_length": fixed_length, "skewed": skewed}
QUANTS = {None: None, "all_255": QUANT_ALL_255, "mixed_1_255": QUANT_MIXED, "slots_1_2_3": QUANT_SLOTS_123}


@functools.lru_cache(maxsize=None)
def recoded(geometry, generator, quality=100, tables="annex_k", slots=None, table_map=None, dht_layout="separate", quant=None):
    """recode() of stream(geometry, generator, quality) with hashable arguments (tables / quant by name, slots as ((old, new), ...), table_map
    as ((dc, ac), ...)) -> (jpeg, coefficients), both read-only"""
    jpeg, coefs = stream(geometry, generator, quality)
    q = QUANTS[quant]
    if q is not None and q["map"] is not None and GEOMETRIES[geometry][2] == 0:
        q = {"tables": q["tables"], "map": q["map"][:1]}
    return _frozen(recode(jpeg, TABLES[tables], dict(slots) if slots else None, table_map, dht_layout, q)), coefs


# ================================================================================================ one name for every stream the tests use
Spec = collections.namedtuple("Spec", "geometry generator quality tables slots table_map dht_layout quant",
                              defaults=(100, "annex_k", None, None, "separate", None))


def spec_id(spec):
    parts = [spec.generator, spec.geometry, f"q{spec.quality}"]
    if spec.tables != "annex_k":
        parts.append(spec.tables)
    if spec.slots:
        parts.append("slots" + "".join(f"{a}{b}" for a, b in spec.slots))
    if spec.table_map:
        parts.append("map" + "".join(f"{a}{b}" for a, b in spec.table_map))
    if spec.dht_layout != "separate":
        parts.append("one_dht")
    if spec.quant:
        parts.append(spec.quant)
    return "-".join(parts)


def get(spec):
    """(jpeg, coefficients) of a Spec: the oracle's stream, re-coded where the Spec asks for anything but the Annex K tables in their slots"""
    if spec[3:] == Spec("", "")[3:]:
        return stream(spec.geometry, spec.generator, spec.quality)
    return recoded(*spec)


@functools.lru_cache(maxsize=None)
def pixels(spec):
    """the oracle's decode of the Spec's stream to the geometry's output format -> (pixels, read-only; Image)"""
    pf, cs = output_format(spec.geometry) or (-1, -1)
    px, img = O.decode(get(spec)[0], pf, cs)
    return _frozen(px), img


# ================================================================================================ images for the encoder
def pattern(name, w, h, seed=0):
    """packed RGB images (flat uint8) whose quantised coefficients reach the extremes at quality 100: AC of size 10, DC differences of size 11"""
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "basis":  # every block a DCT basis function thresholded to 0 / 255, (u, v) changing from block to block, inverted now and then
        i = (yy // 8) * ((w + 7) // 8) + xx // 8
        on = np.cos((2 * (xx % 8) + 1) * (i % 8) * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * ((i // 8) % 8) * np.pi / 16) > 0
        g = np.where(on ^ ((i // 64) % 2 == 1), 255, 0)
        img = np.stack([g, g, np.where((yy // 8) % 2 == 1, 255 - g, g)], -1)  # (odd block rows: blue against red and green -- chrominance swings too)
    elif name == "noise":
        img = np.random.default_rng(6000 + seed).integers(0, 2, (h, w, 3)) * 255
    else:
        g = {"checkerboard": (xx + yy) % 2, "stripes": xx % 2, "blocks": (xx // 8 + yy // 8) % 2}[name] * 255
        img = np.stack([g, g, g], -1)
    return _frozen(img.astype(np.uint8).reshape(-1))
