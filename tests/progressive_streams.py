"""Progressive (SOF2) streams built from CHOSEN coefficients and a CHOSEN scan script (helper module of tests/test_progressive_decode.py; no
fixtures here, no product code, nothing of the reference tree).

write(img, coefs, script, ...) is a Python progressive WRITER: it takes an oracle image description, coefficient planes in the oracle's layout
(component after component, block after block in raster order of the padded plane, 64 coefficients per block in natural order) and a scan script
-- a list of (components, Ss, Se, Ah, Al) -- and emits a SOF2 stream. The header segments of O.encode_from_coefs(img, coefs) are kept as they
are, except that SOF0's marker byte becomes C2, the DHTs are dropped and DRI is the writer's own; then every scan is DHT + SOS + entropy-coded data by
the encoding procedures of ITU T.81 G.1.2 (DC first and refinement, AC first with EOB runs, AC refinement with buffered correction bits), with a
restart interval per scan (MCUs in a scan of several components, blocks in a scan of one).

The TWIN of such a stream is O.encode_from_coefs(img, coefs) itself: expected pixels are O.decode(twin, ...), expected coefficients the ones put in.
A scan of one component codes only the ceil(w_c / 8) x ceil(h_c / 8) blocks of its component: legal() zeroes the AC coefficients of the padded blocks
around them, which no progressive stream can carry."""
import numpy as np

import oracle as O
from synth_streams import to_planes, zigzag_blocks
from test_huffman_optimal import canonical, optimal_table, segments_of

# ================================================================================================ scan scripts: (components, Ss, Se, Ah, Al)
# libjpeg's jpeg_simple_progression (jcparam.c), byte for byte the lists it makes: three-component YCbCr, and everything else (here: one component)
LIBJPEG_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                  ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
LIBJPEG_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


def default_script(n):
    return LIBJPEG_COLOUR if n == 3 else libjpeg_any(n)


def libjpeg_any(n):
    """jpeg_simple_progression's all-purpose script for n components (n = 1: LIBJPEG_GREY)"""
    comps = tuple(range(n))
    each = lambda ss, se, ah, al: [((c,), ss, se, ah, al) for c in comps]  # noqa: E731
    return [(comps, 0, 0, 0, 1)] + each(1, 5, 0, 2) + each(6, 63, 0, 2) + each(1, 63, 2, 1) + [(comps, 0, 0, 1, 0)] + each(1, 63, 1, 0)


def spectral_only(n):
    comps = tuple(range(n))
    return [(comps, 0, 0, 0, 0)] + [((c,), ss, se, 0, 0) for ss, se in ((1, 5), (6, 63)) for c in comps]


def one_ac_scan(n):
    comps = tuple(range(n))
    return [(comps, 0, 0, 0, 0)] + [((c,), 1, 63, 0, 0) for c in comps]


def deep_approximation(n):
    """AC Al 3 -> 2 -> 1 -> 0, DC Al 2 -> 1 -> 0"""
    comps = tuple(range(n))
    out = [(comps, 0, 0, 0, 2)] + [((c,), 1, 63, 0, 3) for c in comps] + [(comps, 0, 0, 2, 1)]
    for ah in (3, 2, 1):
        out += [((c,), 1, 63, ah, ah - 1) for c in comps]
        if ah == 2:
            out += [(comps, 0, 0, 1, 0)]
    return out


def dc_per_component(n):
    return [((c,), 0, 0, 0, 0) for c in range(n)] + [((c,), 1, 63, 0, 0) for c in range(n)]


def dc_chroma_together():
    return [((0,), 0, 0, 0, 1), ((1, 2), 0, 0, 0, 1), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((1, 2), 0, 0, 1, 0), ((0,), 0, 0, 1, 0)]


def chroma_first():
    return [((1, 2), 0, 0, 0, 0), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 0, 0, 0, 0), ((2,), 1, 63, 1, 0), ((0,), 1, 63, 0, 1), ((1,), 1, 63, 1, 0),
            ((0,), 1, 63, 1, 0)]


def single_coefficient_band(n):
    comps = tuple(range(n))
    return [(comps, 0, 0, 0, 0)] + [((c,), 1, 62, 0, 1) for c in comps] + [((c,), 63, 63, 0, 1) for c in comps] + [((c,), 63, 63, 1, 0) for c in comps] + \
           [((c,), 1, 62, 1, 0) for c in comps]


def levels_of(script):
    """the dependency levels by the rule of the decoder's plan: 0, or 1 + the highest level of an earlier scan that shares a component and a coefficient"""
    lv = []
    for i, (comps, ss, se, _, _) in enumerate(script):
        deps = [lv[j] for j, (c2, s2, e2, _, _) in enumerate(script[:i]) if set(comps) & set(c2) and s2 <= se and ss <= e2]
        lv.append(1 + max(deps) if deps else 0)
    return lv


# ================================================================================================ geometry
def frame_of(img):
    """per component: (h, v, blocks_x of the padded plane, blocks_y, coded blocks per row, coded block rows, first block of the plane), and the MCU grid"""
    n = img.comp_count
    hmax, vmax = max(img.samp_h[c] for c in range(n)), max(img.samp_v[c] for c in range(n))
    comps = []
    for c in range(n):
        k = img.comp[c]
        h, v = img.samp_h[c], img.samp_v[c]
        wc, hc = -(-img.width * h // hmax), -(-img.height * v // vmax)
        comps.append((h, v, k.data_width // 8, k.data_height // 8, -(-wc // 8), -(-hc // 8), int(k.data_offset) // 64))
    mx, my = -(-img.width // (8 * hmax)), -(-img.height // (8 * vmax))
    if n > 1:
        for h, v, bx, by, _, _, _ in comps:
            assert bx == mx * h and by == my * v, "progressive frames have whole-MCU planes: make the oracle image with interleaved=1"
    return comps, mx, my


def legal(img, coefs, script=None):
    """the coefficients with zero AC in the padded blocks no scan of one component codes (a copy) -- and zero DC there too for the components whose DC
    comes in a scan of their own in `script`"""
    Z = zigzag_blocks(coefs)
    alone = {s[0][0] for s in script or [] if s[1] == 0 and len(s[0]) == 1}
    for c, (h, v, bx, by, cbx, cby, first) in enumerate(frame_of(img)[0]):
        P = Z[first:first + bx * by].reshape(by, bx, 64)
        lo = 0 if c in alone else 1
        P[cby:, :, lo:] = 0
        P[:, cbx:, lo:] = 0
    return to_planes(Z)


def scan_blocks(img, comps):
    """the blocks a scan of `comps` codes, in coding order: [unit][block of the unit] -> (index into the planes' blocks, place in comps)"""
    fr, mx, my = frame_of(img)
    if len(comps) == 1:
        h, v, bx, by, cbx, cby, first = fr[comps[0]]
        return [[(first + y * bx + x, 0)] for y in range(cby) for x in range(cbx)]
    out = []
    for y in range(my):
        for x in range(mx):
            unit = []
            for i, c in enumerate(comps):
                h, v, bx, _, _, _, first = fr[c]
                unit += [(first + (y * v + j) * bx + x * h + k, i) for j in range(v) for k in range(h)]
            out.append(unit)
    return out


# ================================================================================================ the encoding procedures (G.1.2)
def _size(v):
    return int(v).bit_length()


class _Scan:
    """the symbols and bits of one scan, segment by segment: [(symbol, -1) | (bits, count)]"""

    def __init__(self):
        self.segments, self.cur = [], []
        self.eobrun, self.be = 0, []

    def sym(self, s):
        self.cur.append((s, -1))

    def bits(self, v, n):
        if n:
            self.cur.append((int(v) & ((1 << n) - 1), n))

    def flush_eobrun(self):
        if self.eobrun > 0:
            n = self.eobrun.bit_length() - 1
            self.sym(n << 4)
            self.bits(self.eobrun, n)
            self.eobrun = 0
        for b in self.be:
            self.bits(b, 1)
        self.be = []

    def restart(self):
        self.flush_eobrun()
        self.segments.append(self.cur)
        self.cur = []


def _dc_first(S, Z, unit, pred, al):
    for b, i in unit:
        v = int(Z[b, 0]) >> al
        d = v - pred[i]
        pred[i] = v
        n = _size(abs(d))
        S.sym(n)
        S.bits(d if d >= 0 else d - 1, n)


def _dc_refine(S, Z, unit, al):
    for b, _ in unit:
        S.bits((int(Z[b, 0]) >> al) & 1, 1)


def _ac_first(S, row, ss, se, al):
    band = (np.abs(row[ss:se + 1].astype(np.int32)) >> al)
    prev = -1
    for i in np.flatnonzero(band):
        i = int(i)
        r = i - prev - 1
        prev = i
        S.flush_eobrun()
        while r > 15:
            S.sym(0xF0)
            r -= 16
        t = int(band[i])
        n = _size(t)
        S.sym((r << 4) | n)
        S.bits(t if row[ss + i] >= 0 else ~t, n)
    if prev != se - ss:
        S.eobrun += 1
        if S.eobrun == 0x7FFF:
            S.flush_eobrun()


def _ac_refine(S, row, ss, se, al):
    absv = (np.abs(row[ss:se + 1].astype(np.int32)) >> al)
    nz = [int(i) for i in np.flatnonzero(absv)]
    eob = max([i for i in nz if absv[i] == 1], default=-1)
    r, br, prev = 0, [], -1
    for i in nz:
        r += i - prev - 1
        prev = i
        while r > 15 and i <= eob:
            S.flush_eobrun()
            S.sym(0xF0)
            r -= 16
            for b in br:
                S.bits(b, 1)
            br = []
        t = int(absv[i])
        if t > 1:
            br.append(t & 1)
            continue
        S.flush_eobrun()
        S.sym((r << 4) | 1)
        S.bits(0 if row[ss + i] < 0 else 1, 1)
        for b in br:
            S.bits(b, 1)
        br, r = [], 0
    r += (se - ss) - prev
    if r > 0 or br:
        S.eobrun += 1
        S.be += br
        if S.eobrun == 0x7FFF or len(S.be) > 937:
            S.flush_eobrun()


def scan_symbols_of(img, Z, scan, restart):
    comps, ss, se, ah, al = scan
    units = scan_blocks(img, comps)
    S = _Scan()
    pred = [0] * len(comps)
    for u, unit in enumerate(units):
        if restart and u and u % restart == 0:
            S.restart()
            pred = [0] * len(comps)
        if ss == 0:
            _dc_first(S, Z, unit, pred, al) if ah == 0 else _dc_refine(S, Z, unit, al)
        else:
            (_ac_first if ah == 0 else _ac_refine)(S, Z[unit[0][0]], ss, se, al)
    S.restart()
    return S.segments


def _pack(segment, codes):
    acc, n = 0, 0
    for a, b in segment:
        if b < 0:
            a, b = codes[a]
        acc = (acc << b) | a
        n += b
    pad = -n % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((n + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


def _counts(segments):
    f = [0] * 256
    for seg in segments:
        for a, b in seg:
            if b < 0:
                f[a] += 1
    return f


def _dht(tc, slot, table):
    bits, vals = table[0], table[1]
    body = bytes([(tc << 4) | slot]) + bytes(int(x) for x in bits[1:17]) + bytes(int(x) for x in vals)
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


# ================================================================================================ the writer
def write(img, coefs, script, restart=0, tables="per_scan", slots="by_scan", upto=None, raw_sos=None):
    """-> numpy uint8 SOF2 stream.
    restart: the restart interval, applied to every scan in its own unit; tables: "per_scan" (every scan gets the optimal table of its own symbol
    counts, defined in front of it) or "up_front" (one DC and one AC table from the counts of all scans, defined once); slots: "by_scan" (scan i uses
    slot i mod 4) or an int (every scan redefines and uses that slot); upto: only the first `upto` scans (a prefix is an image);
    raw_sos: {scan index: (components, Ss, Se, Ah, Al)} written into that scan's SOS instead of what the data was coded with (refusal tests)"""
    twin = O.encode_from_coefs(img, coefs)
    Z = zigzag_blocks(coefs)
    head = segments_of(twin)
    first_sos = next(i for i, s in enumerate(head) if s[0] == 0xDA)
    out, ids = [b"\xff\xd8"], None
    for m, payload, _ in head[1:first_sos]:
        if m in (0xC4, 0xDD):
            continue
        if m == 0xC0:
            m = 0xC2
            ids = [payload[6 + 3 * c] for c in range(payload[5])]
        out.append(bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + payload)
    if restart:
        out.append(b"\xff\xdd\x00\x04" + int(restart).to_bytes(2, "big"))
    script = list(script)[:upto]
    coded = [scan_symbols_of(img, Z, scan, restart) for scan in script]
    shared = {}
    if tables == "up_front":
        for tc in (0, 1):
            f = [0] * 256
            for scan, segs in zip(script, coded):
                if (scan[1] > 0) == bool(tc) and not (scan[1] == 0 and scan[3]):
                    f = [a + b for a, b in zip(f, _counts(segs))]
            shared[tc] = optimal_table(f)
            if shared[tc] is not None:
                out.append(_dht(tc, slots if isinstance(slots, int) else 0, shared[tc]))
    for i, (scan, segs) in enumerate(zip(script, coded)):
        comps, ss, se, ah, al = scan
        tc = 1 if ss else 0
        slot = slots if isinstance(slots, int) else (0 if tables == "up_front" else i % 4)
        codes = None
        if not (ss == 0 and ah):
            table = shared[tc] if tables == "up_front" else optimal_table(_counts(segs))
            codes = canonical(table[0], table[1])
            if tables != "up_front":
                out.append(_dht(tc, slot, table))
        hc, s0, s1, a0, a1 = raw_sos[i] if raw_sos and i in raw_sos else scan
        sos = bytes([len(hc)]) + b"".join(bytes([ids[c], (slot << 4) | slot]) for c in hc) + bytes([s0, s1, (a0 << 4) | a1])
        out.append(b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos)
        for j, seg in enumerate(segs):
            if j:
                out.append(bytes([0xFF, 0xD0 + (j - 1) % 8]))
            out.append(_pack(seg, codes))
    out.append(b"\xff\xd9")
    return np.frombuffer(b"".join(out), np.uint8).copy()


def scan_data_ranges(jpeg):
    """[(first byte, length)] of the entropy-coded data of every scan"""
    d = bytes(jpeg)
    out, pos = [], 2
    while pos < len(d) and d[pos + 1] != 0xD9:
        m = d[pos + 1]
        n = (d[pos + 2] << 8) | d[pos + 3]
        pos += 2 + n
        if m == 0xDA:
            end = pos
            while True:
                end = d.index(b"\xff", end)
                if d[end + 1] == 0 or 0xD0 <= d[end + 1] <= 0xD7:
                    end += 2
                    continue
                break
            out.append((pos, end - pos))
            pos = end
    return out


def segment_count(img, script, restart):
    return sum(-(-len(scan_blocks(img, s[0])) // restart) if restart else 1 for s in script)
