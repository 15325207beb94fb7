"""Per-frame optimal Huffman tables (encoder option enc_opt_huffman=optimal, gpujpeg_amd_ext.h).

The option is outside reference parity by construction, so it is pinned by a restatement that is independent of the product:
  - the table build of ITU T.81 Annex K.2 (Figures K.1, K.3, K.4; ties of equal counts go to the larger symbol value, as libjpeg's
    table generator does) plus the decoder-fit rule (the largest code-length limit L of 16 .. 10 whose table needs at most 6 second-level
    tables of the two-level decoder), in Python below;
  - a small transcoder, a Python `jpegtran -optimize`: it parses the product's DEFAULT stream (itself pinned to the reference), counts the
    symbols, builds the tables and re-emits every symbol -- byte stuffing, restart markers, 1-bit padding and the APP13 index included.
Its output is the expected optimized file, byte for byte.

Two tiers: the CPU tier runs the product's kernels on tests/hipemu (the execution model of tests/test_emu_parity.py, own fixture), the
-m gpu tier the product library on the MI355X."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import CASES, api_params, make_raw, natural_image, oracle_image

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "hipemu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libgpujpeg_emu.so")
CAMERA = os.path.join(HERE, "golden", "camera_bt709_422_q95.jpg")
OPT, OPTIMAL, STANDARD = "enc_opt_huffman", "optimal", "standard"


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


# ================================================================================================ restatement: tables
def optimal_table(freq, limit=None):
    """BITS[0..16], HUFFVAL, L for the counts freq[256] (None when every count is 0). limit=None applies the decoder-fit rule."""
    f = [int(x) for x in freq] + [1]  # K.1: reserved code point 256, count 1 (no code of all ones)
    if not any(f[:256]):
        return None
    size, others = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if f[i]]
        if len(live) < 2:
            break
        # the smallest count; of equal counts the LARGER symbol value
        c1 = max(live, key=lambda i: (-f[i], i))
        c2 = max((i for i in live if i != c1), key=lambda i: (-f[i], i))
        f[c1] += f[c2]
        f[c2] = 0
        for c in (c1, c2):
            size[c] += 1
            while others[c] >= 0:
                c = others[c]
                size[c] += 1
        c = c1
        while others[c] >= 0:
            c = others[c]
        others[c] = c2
    counts = [0] * 260
    for s in size:
        if s:
            counts[s] += 1
    vals = [j for s in range(1, 258) for j in range(256) if size[j] == s]  # K.4: unadjusted size, then value
    for L in ([limit] if limit else range(16, 9, -1)):
        b = list(counts)
        for i in range(259, L, -1):  # K.3
            while b[i] > 0:
                j = i - 2
                while b[j] == 0:
                    j -= 1
                b[i] -= 2
                b[i - 1] += 1
                b[j + 1] += 2
                b[j] -= 1
        i = L
        while b[i] == 0:
            i -= 1
        b[i] -= 1
        bits = [0] + b[1:17]
        if limit or subtables(bits) <= 6:
            return bits, vals, L
    raise AssertionError("no limit fits")


def subtables(bits):
    """second-level tables of the two-level decoder: canonical codes put every code longer than 10 bits behind one 10-bit prefix boundary"""
    return -(-sum(bits[L] << (16 - L) for L in range(11, 17)) // 64)


def canonical(bits, vals):
    code, out, p = 0, {}, 0
    for L in range(1, 17):
        for _ in range(bits[L]):
            out[vals[p]] = (code, L)
            code += 1
            p += 1
        code <<= 1
    return out


# ================================================================================================ restatement: transcoder
def segments_of(jpeg):
    """[(marker, payload bytes or None, entropy bytes following an SOS or b"")] of a baseline stream"""
    d = bytes(jpeg)
    assert d[:2] == b"\xff\xd8"
    out, pos = [(0xD8, None, b"")], 2
    while pos < len(d):
        assert d[pos] == 0xFF, pos
        m = d[pos + 1]
        pos += 2
        if m == 0xD9:
            out.append((m, None, b""))
            break
        n = (d[pos] << 8) | d[pos + 1]
        payload = d[pos + 2:pos + n]
        pos += n
        ecs = b""
        if m == 0xDA:  # entropy-coded data up to the first marker that is not RSTn
            end = pos
            while True:
                end = d.index(b"\xff", end)
                if d[end + 1] == 0x00 or 0xD0 <= d[end + 1] <= 0xD7:
                    end += 2
                    continue
                break
            ecs = d[pos:end]
            pos = end
        out.append((m, payload, ecs))
    return out


def _split_restart(ecs):
    """entropy-coded data -> unstuffed segments (split at RSTn)"""
    segs, cur, i = [], bytearray(), 0
    while i < len(ecs):
        b = ecs[i]
        if b == 0xFF:
            nxt = ecs[i + 1]
            if nxt == 0x00:
                cur.append(0xFF)
            else:
                assert 0xD0 <= nxt <= 0xD7
                segs.append(bytes(cur))
                cur = bytearray()
            i += 2
            continue
        cur.append(b)
        i += 1
    segs.append(bytes(cur))
    return segs


class _Bits:
    def __init__(self, data):
        self.s = "".join(format(b, "08b") for b in data) + "1" * 32
        self.p = 0

    def peek16(self):
        return int(self.s[self.p:self.p + 16], 2)

    def take(self, n):
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v


def _decode_lut(bits, vals):
    lut = [None] * 65536
    for sym, (code, L) in canonical(bits, vals).items():
        base = code << (16 - L)
        for x in range(base, base + (1 << (16 - L))):
            lut[x] = (L, sym)
    return lut


def scan_symbols(jpeg):
    """Every symbol of every scan of a baseline stream in coding order, per restart segment: [scan][segment] = [(table key, symbol,
    magnitude bits, their count)]; table key = (class, id)."""
    segs = segments_of(jpeg)
    tables, comps, ri, W, H, scans = {}, {}, 0, 0, 0, []
    for m, pl, ecs in segs:
        if m == 0xC4:
            p = 0
            while p < len(pl):
                tc, bits = pl[p], [0] + list(pl[p + 1:p + 17])
                n = sum(bits)
                tables[(tc >> 4, tc & 15)] = (bits, list(pl[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xC0:
            H, W = (pl[1] << 8) | pl[2], (pl[3] << 8) | pl[4]
            for k in range(pl[5]):
                cid, hv = pl[6 + 3 * k], pl[7 + 3 * k]
                comps[cid] = (hv >> 4, hv & 15)
        elif m == 0xDD:
            ri = (pl[0] << 8) | pl[1]
        elif m == 0xDA:
            sc = [(pl[1 + 2 * k], pl[2 + 2 * k] >> 4, pl[2 + 2 * k] & 15) for k in range(pl[0])]
            scans.append((sc, ecs))
    hmax = max(h for h, v in comps.values())
    vmax = max(v for h, v in comps.values())
    luts = {k: _decode_lut(*t) for k, t in tables.items()}
    out = []
    for sc, ecs in scans:
        if len(sc) > 1:
            mcus = -(-W // (8 * hmax)) * -(-H // (8 * vmax))
            layout = [(cid, td, ta) for cid, td, ta in sc for _ in range(comps[cid][0] * comps[cid][1])]
        else:
            cid, td, ta = sc[0]
            h, v = comps[cid]
            mcus = -(-(-(-W * h // hmax)) // 8) * -(-(-(-H * v // vmax)) // 8)
            layout = [sc[0]]
        per = ri if ri else mcus
        scan_out = []
        for si, data in enumerate(_split_restart(ecs)):
            n = min(per, mcus - si * per)
            br, syms = _Bits(data), []
            for _ in range(n):
                for cid, td, ta in layout:
                    L, s = luts[(0, td)][br.peek16()]
                    br.take(L)
                    syms.append(((0, td), s, br.take(s), s))
                    lut, k = luts[(1, ta)], 1
                    while k < 64:
                        L, s = lut[br.peek16()]
                        br.take(L)
                        r, z = s >> 4, s & 15
                        syms.append(((1, ta), s, br.take(z), z))
                        if z == 0 and r != 15:
                            break
                        k += r + 1
            scan_out.append(syms)
        assert len(scan_out) == -(-mcus // per)
        out.append(scan_out)
    return out


def transcode(jpeg):
    """The expected enc_opt_huffman=optimal stream of a frame from its default stream: same symbols, the frame's own tables."""
    segs = segments_of(jpeg)
    syms = scan_symbols(jpeg)
    freq = {}
    for scan in syms:
        for seg in scan:
            for key, s, _, _ in seg:
                freq.setdefault(key, np.zeros(256, np.int64))[s] += 1
    new = {key: optimal_table(f)[:2] for key, f in freq.items()}
    codes = {key: canonical(*t) for key, t in new.items()}
    out, pending_app13, si = bytearray(), [], 0
    for m, pl, ecs in segs:
        if m == 0xED and si < len(syms):  # APP13 index of the next scan: rebuilt behind it
            pending_app13.append((len(out), pl))
            out += bytes([0xFF, m, (len(pl) + 2) >> 8, (len(pl) + 2) & 255]) + pl
            continue
        if pl is None:
            out += bytes([0xFF, m])
            continue
        if m == 0xC4:
            tc = pl[0]
            bits, vals = new[(tc >> 4, tc & 15)]
            pl = bytes([tc] + bits[1:17] + vals)
        out += bytes([0xFF, m, (len(pl) + 2) >> 8, (len(pl) + 2) & 255]) + pl
        if m == 0xDA:
            start, offsets = len(out), []
            for k, seg in enumerate(syms[si]):
                if k:
                    out += bytes([0xFF, 0xD0 + (k - 1) % 8])
                offsets.append(len(out) - start)
                s = "".join(format(codes[key][sym][0], f"0{codes[key][sym][1]}b") + (format(v, f"0{n}b") if n else "")
                            for key, sym, v, n in seg)
                s += "1" * (-len(s) % 8)
                for i in range(0, len(s), 8):
                    b = int(s[i:i + 8], 2)
                    out.append(b)
                    if b == 0xFF:
                        out.append(0)
            offsets.append(len(out) - start)
            if pending_app13:
                data = b"".join(int(o).to_bytes(4, "big") for o in offsets)
                for at, old in pending_app13:
                    chunk, data = data[:len(old) - 1], data[len(old) - 1:]
                    out[at + 5:at + 4 + len(old)] = chunk
                assert not data
            pending_app13 = []
            si += 1
    return np.frombuffer(bytes(out), np.uint8)


def frame_without_entropy(jpeg, keep_app13=True):
    return [(m, pl) for m, pl, _ in segments_of(jpeg) if m != 0xC4 and (keep_app13 or m != 0xED)]


def dht_tables(jpeg):
    out = []
    for m, pl, _ in segments_of(jpeg):
        if m == 0xC4:
            p = 0
            while p < len(pl):
                bits = [0] + list(pl[p + 1:p + 17])
                out.append((pl[p], bits, list(pl[p + 17:p + 17 + sum(bits)])))
                p += 17 + sum(bits)
    return out


# ================================================================================================ helpers on the libraries
def encode_pair(lib, G, case, raw, segment_info=0, options=(), fused=True):
    """(default stream, optimal stream) of one frame; both from fresh encoders with the same options"""
    p, pi = api_params(lib, G, case, segment_info)
    res = []
    for mode in (STANDARD, OPTIMAL):
        enc = G.Encoder(lib)
        enc.set_fused(fused)
        for k, v in options:
            assert enc.set_option(k, v) == 0
        assert enc.set_option(OPT, mode) == 0
        res.append(enc.encode(p, pi, raw))
        enc.close()
    return res


def check_bytes(O, d, o, segment_info=False):
    want = transcode(d)
    assert o.size == want.size and np.array_equal(o, want), "optimized stream differs from the transcoded default stream"
    assert frame_without_entropy(o, not segment_info) == frame_without_entropy(d, not segment_info), "bytes outside DHT / entropy data differ"
    for tc, bits, vals in dht_tables(o):
        assert subtables(bits) <= 6, (tc, bits)
        assert prefix_code_ok(bits, vals)
    s, s2 = O.parse(o), O.parse(d)
    assert np.array_equal(O.huffman_decode(s, o), O.huffman_decode(s2, d)), "coefficients differ"
    O.lib().gjo_stream_free(C.byref(s))
    O.lib().gjo_stream_free(C.byref(s2))


def prefix_code_ok(bits, vals):
    """a valid prefix code: Kraft sum <= 1 and no code of all ones"""
    kraft = sum(bits[L] << (16 - L) for L in range(1, 17))
    return kraft < (1 << 16) and len(vals) == len(set(vals)) == sum(bits)


def host_optimal(lib, freq):
    f = np.ascontiguousarray(freq, np.uint32)
    bits, vals = np.zeros(17, np.uint8), np.zeros(256, np.uint8)
    fn = lib.L.gpujpeg_amd_host_huffman_optimal
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L = fn(f.ctypes.data, bits.ctypes.data, vals.ctypes.data)
    return L, [int(b) for b in bits], [int(v) for v in vals[:int(bits.sum())]]


# ================================================================================================ CPU tier: host tables
@pytest.mark.parametrize("seed", range(12))
def test_host_tables_equal_the_restatement(lib, seed):
    rng = np.random.default_rng(seed)
    freq = np.zeros(256, np.uint32)
    n = int(rng.integers(1, 257))
    syms = rng.choice(256, n, replace=False)
    freq[syms] = rng.integers(1, [2, 10, 1000, 1 << 20][seed % 4], n)
    L, bits, vals = host_optimal(lib, freq)
    want_bits, want_vals, want_L = optimal_table(freq)
    assert (L, bits, vals) == (want_L, want_bits, want_vals)
    assert subtables(bits) <= 6 and sum(bits) == n


def test_host_tables_fit_rule_picks_10(lib):
    freq = np.zeros(256, np.uint32)
    freq[[0x00, 0x01, 0x02, 0x11, 0x03]] = 1_000_000  # 5 dominant symbols, 150 equally rare ones
    rare = [s for s in range(256) if s not in (0x00, 0x01, 0x02, 0x11, 0x03)][:150]
    freq[rare] = 1
    assert subtables(optimal_table(freq, 16)[0]) == 23
    L, bits, vals = host_optimal(lib, freq)
    assert L == 10 and subtables(bits) == 0 and max(i for i in range(17) if bits[i]) == 10
    assert (bits, vals) == optimal_table(freq)[:2]


def test_host_tables_small_and_full_and_deep(lib):
    for sym in (0x00, 0x37, 0xFF):  # one symbol: one 1-bit code
        freq = np.zeros(256, np.uint32)
        freq[sym] = 12345
        assert host_optimal(lib, freq) == (16, [0, 1] + [0] * 15, [sym])
    freq = np.zeros(256, np.uint32)  # every AC symbol of baseline coding
    ac = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    freq[ac] = np.arange(1, 163) * 7 % 101 + 1
    L, bits, vals = host_optimal(lib, freq)
    assert sum(bits) == 162 and sorted(vals) == sorted(ac) and (L, bits, vals) == (optimal_table(freq)[2], *optimal_table(freq)[:2])
    fib = [1, 1]  # Fibonacci-like counts: unlimited code lengths far beyond 16, K.3 folds them
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    freq = np.zeros(256, np.uint32)
    freq[:40] = fib
    L, bits, vals = host_optimal(lib, freq)
    assert sum(bits) == 40 and max(i for i in range(17) if bits[i]) <= 16
    assert (bits, vals, L) == optimal_table(freq)
    assert host_optimal(lib, np.zeros(256, np.uint32))[0] == -1


def test_restated_table_build_ties_and_reserved_code():
    """The restatement's own invariants: a tie goes to the larger symbol value, no code is all ones, K.4 order is by unadjusted size."""
    freq = np.zeros(256, np.uint32)
    freq[[1, 2, 3, 4]] = 10
    bits, vals, L = optimal_table(freq)
    assert vals == [1, 2, 3, 4] and bits[2] == 3 and bits[3] == 1  # 5 leaves (4 + reserved): the larger symbols merge first
    code = canonical(bits, vals)
    assert all(c != (1 << n) - 1 for c, n in code.values())


# ================================================================================================ CPU tier: the product on hipemu
def test_emu_option_values(G, emu):
    enc = G.Encoder(emu)
    for v in (STANDARD, OPTIMAL, STANDARD):
        assert enc.set_option(OPT, v) == 0
    for bad in ("", "Optimal", "optimized", "1"):
        assert enc.set_option(OPT, bad) != 0
    assert G.ENC_OPT_HUFFMAN == OPT and (G.ENC_HUFFMAN_STANDARD, G.ENC_HUFFMAN_OPTIMAL) == (STANDARD, OPTIMAL)
    enc.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_emu_optimal_bytes_equal_the_transcoder(O, G, emu, case):
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw)
    img = oracle_image(O, case)
    assert np.array_equal(d, O.encode(img, raw)), "default stream is not the reference's"
    check_bytes(O, d, o)
    s = O.parse(o)
    assert np.array_equal(O.huffman_decode(s, o), O.fdct_quant(img, O.preprocess(img, raw)))
    O.lib().gjo_stream_free(C.byref(s))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("rgb_tiny_r4", "rgb_interleaved", "rgb_to_422_nonil", "planar420_in", "gray", "rgb_restart0")],
                         ids=lambda c: c[0])
def test_emu_optimal_generic_path(O, G, emu, case):
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw, fused=False)
    check_bytes(O, d, o)


@pytest.mark.parametrize("case", [c for c in CASES if c[6] != 0][:4], ids=lambda c: c[0])
def test_emu_optimal_segment_info(O, G, emu, case):
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw, segment_info=1)
    check_bytes(O, d, o, segment_info=True)
    dec = G.Decoder(emu)  # consumes the APP13 index instead of scanning for RSTn
    assert np.array_equal(dec.decode(o)[0], O.decode(d)[0])


@pytest.mark.parametrize("options", [("enc_hdr", "JFIF"), ("enc_hdr", "Adobe"), ("enc_hdr", "SPIFF"), ("enc_hdr", "Exif"),
                                     ("enc_opt_flipped", "1"), ("enc_opt_channel_remap", "210"), ("enc_metadata", "orientation=90")],
                         ids=lambda o: f"{o[0]}={o[1]}")
def test_emu_optimal_with_options(O, G, emu, options):
    case = ("opts", 120, 90, 1, 1, 75, 6, 0, None, 3)
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw, options=[options])
    check_bytes(O, d, o)


def test_emu_optimal_outputs_inputs_and_determinism(O, G, emu):
    case = ("io", 200, 120, 1, 1, 80, 5, 1, None, 3)
    raw = make_raw(O, case)
    d, want = encode_pair(emu, G, case, raw)
    check_bytes(O, d, want)
    run_outputs_inputs_and_isolation(emu, G, case, raw, d, want)


def run_outputs_inputs_and_isolation(lib, G, case, raw, d, want):
    p, pi = api_params(lib, G, case)
    L = lib.L
    L.gj_hip_malloc.restype = C.c_void_p
    L.gj_hip_malloc.argtypes = [C.c_size_t]
    L.gj_hip_free.argtypes = [C.c_void_p]
    L.gj_hip_memcpy_h2d.argtypes = L.gj_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.gj_hip_stream_sync.argtypes = [C.c_void_p]
    d_raw = L.gj_hip_malloc(raw.size)
    assert d_raw and L.gj_hip_memcpy_h2d(d_raw, raw.ctypes.data, raw.size, None) == 0 and L.gj_hip_stream_sync(None) == 0
    try:
        for out in ("enc_out_val_pageable", "enc_out_val_pinned", "enc_out_val_device"):
            enc = G.Encoder(lib)
            assert enc.set_option("enc_opt_out", out) == 0 and enc.set_option(OPT, OPTIMAL) == 0
            for gpu in (False, True):
                ptr, n = enc.encode_noclone(p, pi, d_raw if gpu else raw, gpu=gpu)
                got = np.empty(n, np.uint8)
                if out == "enc_out_val_device":
                    assert L.gj_hip_memcpy_d2h(got.ctypes.data, C.cast(ptr, C.c_void_p), n, None) == 0 and L.gj_hip_stream_sync(None) == 0
                else:
                    got[:] = np.ctypeslib.as_array(ptr, shape=(n,))
                assert np.array_equal(got, want), (out, gpu)
            enc.close()
    finally:
        L.gj_hip_free(d_raw)
    enc = G.Encoder(lib)  # determinism, and the option off again on the same encoder
    assert enc.set_option(OPT, OPTIMAL) == 0
    assert np.array_equal(enc.encode(p, pi, raw), want) and np.array_equal(enc.encode(p, pi, raw), want)
    assert enc.set_option(OPT, STANDARD) == 0
    assert np.array_equal(enc.encode(p, pi, raw), d)
    assert enc.set_option(OPT, OPTIMAL) == 0
    assert np.array_equal(enc.encode(p, pi, raw), want)
    enc.close()


def run_batches(O, G, lib, case, frames=3):
    p, pi = api_params(lib, G, case)
    n = lib.image_size(pi)
    raws = [natural_image(case[1], case[2], 3, seed=40 + f) for f in range(frames)]
    one = G.Encoder(lib)
    assert one.set_option(OPT, OPTIMAL) == 0
    want = [one.encode(p, pi, r) for r in raws]
    for w, r in zip(want, raws):
        assert np.array_equal(w, transcode(one_default(lib, G, p, pi, r)))
    enc = G.Encoder(lib)
    assert enc.set_option(OPT, OPTIMAL) == 0
    got = enc.encode_batch(p, pi, np.concatenate(raws), frames, n)
    assert enc.last_batch() == (0, frames)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    got = enc.encode_batch_ptrs(p, pi, raws)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert enc.set_option(OPT, STANDARD) == 0
    got = enc.encode_batch(p, pi, np.concatenate(raws), frames, n)
    assert enc.last_batch()[0] == frames  # (the default configuration takes the batched launches again)
    assert all(np.array_equal(a, one_default(lib, G, p, pi, r)) for a, r in zip(got, raws))


def one_default(lib, G, p, pi, raw):
    enc = G.Encoder(lib)
    out = enc.encode(p, pi, raw)
    enc.close()
    return out


def test_emu_optimal_frame_batches(O, G, emu):
    run_batches(O, G, emu, ("batch", 256, 64, 1, 1, 75, 8, 0, None, 3))


def decoders_agree(G, lib, d, o, monkeypatch, O=None):
    modes = [{}, {"GJ_DEC_TOKENS": "1"}, {"GJ_DEC_NO_TOKENS": "1"}, {"GJ_DEC_ENTROPY": "serial"}, {"GJ_DEC_SEQ": "1"}, {"GJ_DEC_SEQ": "0"},
             {"GPUJPEG_HOST_SCAN": "1"}]
    base = None
    for env in modes:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            dec = G.Decoder(lib)
            a = dec.decode(d)[0]
            b = dec.decode(o)[0]  # (after d: the header cache of d does not match o)
            c = dec.decode(o)[0]
            dec.close()
        assert np.array_equal(a, b) and np.array_equal(b, c), env
        base = a if base is None else base
        assert np.array_equal(base, a)
    if O is not None:
        assert np.array_equal(base, O.decode(d)[0])


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("rgb_natural_auto", "uyvy_422_il_q90", "rgb_to_420_il", "gray", "rgb_restart0")],
                         ids=lambda c: c[0])
def test_emu_decoders_agree(O, G, emu, case, monkeypatch):
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw)
    decoders_agree(G, emu, d, o, monkeypatch, O)


def test_emu_reference_decodes_the_optimized_stream(O, G, emu, _ref_lib):
    case = ("ref", 320, 200, 1, 1, 75, 6, 0, None, 3)
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw)
    dec = G.Decoder(_ref_lib)
    assert np.array_equal(dec.decode(o)[0], dec.decode(d)[0])
    dec.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("rgb_natural_auto", "rgb_to_420_il", "gray")], ids=lambda c: c[0])
def test_emu_pil_decodes_the_optimized_stream(O, G, emu, case):
    Image = pytest.importorskip("PIL.Image")
    import io
    raw = make_raw(O, case)
    d, o = encode_pair(emu, G, case, raw)
    a = np.asarray(Image.open(io.BytesIO(d.tobytes())).convert("RGB"))
    b = np.asarray(Image.open(io.BytesIO(o.tobytes())).convert("RGB"))
    assert np.array_equal(a, b)


def camera_rgb(O):
    jpeg = np.fromfile(CAMERA, np.uint8)
    px, _ = O.decode(jpeg, 1, 1)  # 4:4:4 RGB, packed
    return px.reshape(-1)


@pytest.mark.parametrize("q", [50, 75, 90])
def test_emu_optimal_is_smaller(O, G, emu, q):
    for name, w, h, raw in (("natural", 640, 480, natural_image(640, 480)), ):
        case = (name, w, h, 1, 1, q, -1, 0, None, 3)
        d, o = encode_pair(emu, G, case, raw)
        assert o.size < d.size, (name, q, d.size, o.size)


# ================================================================================================ -m gpu tier: the product on the MI355X
HD_CASES = [("hd_rgb_q75", 1920, 1080, 1, 1, 75, -1, 0, None, 3),
            ("hd_uyvy422_il_q90", 1920, 1080, 3, 3, 90, -1, 1, None, 3),
            ("hd_rgb_420_il", 1920, 1080, 1, 1, 60, -1, 1, [(2, 2), (1, 1), (1, 1)], 3),
            ("hd_rgb_restart0", 1920, 1080, 1, 1, 75, 0, 0, None, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_optimal_bytes_equal_the_transcoder(O, G, gpu_lib, case):
    raw = make_raw(O, case)
    d, o = encode_pair(gpu_lib, G, case, raw)
    check_bytes(O, d, o)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HD_CASES, ids=[c[0] for c in HD_CASES])
def test_gpu_optimal_hd(O, G, gpu_lib, case, monkeypatch):
    raw = natural_image(1920, 1080) if case[3] == 1 else O.noise(O.raw_size(1920, 1080, case[3]), seed=5)
    d, o = encode_pair(gpu_lib, G, case, raw)
    check_bytes(O, d, o)
    decoders_agree(G, gpu_lib, d, o, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[6] != 0][:4], ids=lambda c: c[0])
def test_gpu_optimal_segment_info(O, G, gpu_lib, case):
    raw = make_raw(O, case)
    d, o = encode_pair(gpu_lib, G, case, raw, segment_info=1)
    check_bytes(O, d, o, segment_info=True)
    assert np.array_equal(G.Decoder(gpu_lib).decode(o)[0], O.decode(d)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,pf,q,il,ss", [("8k_rgb_q75", 7680, 4320, 1, 75, 0, None), ("4k_rgb_q75", 3840, 2160, 1, 75, 0, None),
                                                 ("8k_uyvy422_q90", 7680, 4320, 3, 90, 1, None)])
def test_gpu_optimal_coefficients_full_size(O, G, gpu_lib, name, w, h, pf, q, il, ss):
    case = (name, w, h, pf, 3 if pf == 3 else 1, q, -1, il, ss, 3)
    raw = natural_image(w, h) if pf == 1 else O.noise(O.raw_size(w, h, pf), seed=9)
    d, o = encode_pair(gpu_lib, G, case, raw)
    img = oracle_image(O, case)
    coefs = O.fdct_quant(img, O.preprocess(img, raw))
    for j in (d, o):
        s = O.parse(j)
        assert np.array_equal(O.huffman_decode(s, j), coefs), name
        O.lib().gjo_stream_free(C.byref(s))
    for tc, bits, vals in dht_tables(o):
        assert subtables(bits) <= 6
    assert o.size < d.size


@pytest.mark.gpu
def test_gpu_optimal_outputs_inputs_batches_and_stats(O, G, gpu_lib):
    case = ("io", 640, 360, 1, 1, 80, 5, 1, None, 3)
    raw = make_raw(O, case)
    d, want = encode_pair(gpu_lib, G, case, raw)
    check_bytes(O, d, want)
    run_outputs_inputs_and_isolation(gpu_lib, G, case, raw, d, want)
    run_batches(O, G, gpu_lib, ("batch", 1920, 1080, 1, 1, 75, -1, 0, None, 3))
    p, pi = api_params(gpu_lib, G, case)
    p.perf_stats = 1
    enc = G.Encoder(gpu_lib)
    assert enc.set_option(OPT, OPTIMAL) == 0
    assert np.array_equal(enc.encode(p, pi, raw), want)
    kt = enc.kernel_times(6)
    assert kt is not None and kt[5] > 0 and kt[2] > 0, kt  # [5] k_huffman_count, [2] k_huffman
    assert enc.set_option(OPT, STANDARD) == 0
    enc.encode(p, pi, raw)
    assert enc.kernel_times(6)[5] == 0
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", [50, 75, 90])
def test_gpu_optimal_is_smaller(O, G, gpu_lib, q):
    for name, raw in (("natural", natural_image(1920, 1080)), ("camera", camera_rgb(O))):
        case = (name, 1920, 1080, 1, 1, q, -1, 0, None, 3)
        d, o = encode_pair(gpu_lib, G, case, raw)
        assert o.size < d.size, (name, q, d.size, o.size)


@pytest.mark.gpu
def test_gpu_cli_writes_the_api_bytes(O, G, gpu_lib, tmp_path):
    exe = os.path.join(os.path.dirname(G.PRODUCT_LIB), "gpujpegtool")
    raw = natural_image(640, 368)
    src = tmp_path / "in.rgb"
    raw.tofile(src)
    got = {}
    for mode in (STANDARD, OPTIMAL):
        out = tmp_path / f"{mode}.jpg"
        r = subprocess.run([exe, "-e", "-s", "640x368", "-f", "444-u8-p012", "-q", "75", "-r", "8", "-O", f"{OPT}={mode}", str(src), str(out)],
                           capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-400:]
        got[mode] = np.fromfile(out, np.uint8)
    case = ("cli", 640, 368, 1, 1, 75, 8, 0, None, 3)
    d, o = encode_pair(gpu_lib, G, case, raw)
    assert np.array_equal(got[STANDARD], d)
    assert np.array_equal(got[OPTIMAL], o)
