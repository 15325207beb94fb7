"""Pins the CPU restatement (oracle/gj_oracle.c) against the reference's own code.

oracle/_ref/libgpujpeg_ref.so is the reference's host C files (driver, geometry, tables, JFIF writer/reader,
CPU Huffman coders) AND all five of its CUDA modules (colour / sampling, fDCT + quantiser, dequantiser + IDCT, and since round 6 the two
Huffman GPU modules) compiled unmodified from /root/reference against a host-memory CUDA stub and run under the cudaemu execution
model (oracle/cudaemu; contraction off). So for identical parameters and pixels:
  * complete JPEG bytes must match  -> geometry, tables, header bytes, Huffman, stuffing, RSTn, stitching
  * the reference's CPU Huffman coder re-encoding the same coefficients must give the same file
  * decode through reference reader + reference CPU Huffman decoder must match the restated parser/decoder
"""
import ctypes as C

import numpy as np
import pytest

from conftest import CASES, api_params, make_raw, oracle_image


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_encode_bytes_and_decode_pixels(O, G, ref, case):
    raw = make_raw(O, case)
    p, pi = api_params(ref, G, case)
    enc = G.Encoder(ref)
    jpeg = enc.encode(p, pi, raw)
    want = O.encode(oracle_image(O, case), raw)
    assert np.array_equal(jpeg, want)

    # the reference CPU Huffman coder (src/gpujpeg_huffman_cpu_encoder.c:297) on the same coefficients
    out, size = C.POINTER(C.c_uint8)(), C.c_size_t()
    ref.L.gjref_reencode_cpu_huffman.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    assert ref.L.gjref_reencode_cpu_huffman(enc.h, C.byref(out), C.byref(size)) == 0
    cpu = np.ctypeslib.as_array(out, shape=(size.value,)).copy()
    if case[8] is None or True:
        assert np.array_equal(cpu, jpeg), "GPU-path segment stitching differs from the reference CPU Huffman stream"

    # decode: default output format, then the native one
    dec = G.Decoder(ref)
    px, info = dec.decode(jpeg)
    opx, oinfo = O.decode(want)
    assert (info.width, info.height, info.pixel_format, info.color_space) == (oinfo.width, oinfo.height, oinfo.pixel_format, oinfo.color_space)
    assert np.array_equal(px, opx)


def _warp_stats(ref):
    st = (C.c_ulong * 4)()
    ref.L.cudaemu_warp_stats(st)
    return list(st)


@pytest.mark.parametrize("blocks", [1, 3, 70])
def test_cudaemu_warp_mode_known_answers(ref, blocks):
    """The execution model itself, apart from the reference: four small kernels written for this repository in the reference encoder's warp-synchronous style
    (oracle/cudaemu/selftest/warp_selftest.cu: a prefix sum that hands values from lane to lane through shared memory with no barrier, compaction by vote,
    partial exit + rotation + __syncthreads, room reserved with atomicAdd and read by the other lanes without a barrier) against closed forms. Every one of them
    is wrong under a model that runs the lanes one after the other (the prefix sum in 120 of 128 lanes, tried with cudaemu's plain mode). 70 blocks: the grid
    is spread over host threads."""
    rng = np.random.default_rng(blocks)
    n = blocks * 128
    vin = rng.integers(0, 1 << 20, n, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p)
    # 1. prefix sum per warp
    out = np.zeros(n, np.uint32)
    ref.L.cudaemu_selftest_scan.argtypes = [u32p, u32p, C.c_int]
    ref.L.cudaemu_selftest_scan(ptr(vin), ptr(out), blocks)
    assert np.array_equal(out.reshape(-1, 32), np.cumsum(vin.reshape(-1, 32), axis=1, dtype=np.uint32))
    # 2. compaction by vote
    out = np.full(n, 0xFFFFFFFF, np.uint32)
    cnt = np.zeros(n // 32, np.uint32)
    ref.L.cudaemu_selftest_compact.argtypes = [u32p, u32p, u32p, C.c_int]
    ref.L.cudaemu_selftest_compact(ptr(vin), ptr(out), ptr(cnt), blocks)
    for w, row in enumerate(vin.reshape(-1, 32)):
        odd = row[row & 1 == 1]
        assert cnt[w] == odd.size and np.array_equal(out[w * 32:w * 32 + odd.size], odd) and np.all(out[w * 32 + odd.size:(w + 1) * 32] == 0xFFFFFFFF)
    # 3. exits, rotation, block barrier, votes of the live lanes
    out = np.zeros(n, np.uint32)
    sums, votes = np.zeros(blocks, np.uint32), np.zeros(blocks * 4, np.uint32)
    ref.L.cudaemu_selftest_rotate.argtypes = [u32p, u32p, u32p, u32p, C.c_int]
    ref.L.cudaemu_selftest_rotate(ptr(vin), ptr(out), ptr(sums), ptr(votes), blocks)
    for b in range(blocks):
        live = 24 if b == 1 else 32
        first = []
        for w in range(4):
            row, got = vin[b * 128 + w * 32:b * 128 + w * 32 + 32], out[b * 128 + w * 32:b * 128 + w * 32 + 32]
            if w & 1:
                assert np.all(got == 0xDEAD)
                continue
            assert np.array_equal(got[:live], np.roll(row[:live], -1)) and np.all(got[live:] == 0xBEEF)
            assert votes[b * 4 + w] == (1 << live) - 1
            first.append(int(row[1]))
        assert sums[b] == (first[0] + first[1]) & 0xFFFFFFFF
    # 4. room reserved with an atomic, its result handed to the warp through shared memory
    out = np.zeros(n, np.uint32)
    total = np.zeros(1, np.uint32)
    ref.L.cudaemu_selftest_reserve.argtypes = [u32p, u32p, u32p, C.c_int]
    ref.L.cudaemu_selftest_reserve(ptr(vin), ptr(out), ptr(total), blocks)
    odd_all = vin[vin & 1 == 1]
    assert total[0] == odd_all.size and np.array_equal(np.sort(out[:odd_all.size]), np.sort(odd_all))
    runs = {tuple(row[row & 1 == 1]) for row in vin.reshape(-1, 32)}  # every warp's odd values lie together, in lane order, wherever its reservation landed
    at = 0
    while at < odd_all.size:
        hit = [r for r in runs if len(r) and tuple(out[at:at + len(r)]) == r]
        assert hit, at
        runs.discard(hit[0])
        at += len(hit[0])


HUFF_GPU_CASES = CASES + [("huff_many_segments_r2", 400, 304, 1, 1, 90, 2, 0, None, 3), ("huff_il_420_r3", 322, 242, 1, 1, 60, 3, 1, [(2, 2), (1, 1), (1, 1)], 3),
                          ("huff_q100_noise_r5", 128, 96, 1, 1, 100, 5, 0, None, 3)]


@pytest.mark.parametrize("case", HUFF_GPU_CASES, ids=[c[0] for c in HUFF_GPU_CASES])
def test_reference_huffman_gpu_kernels_run_and_agree(O, G, ref, case):
    """ The reference's two Huffman GPU modules -- src/gpujpeg_huffman_gpu_encoder.cu (encode_kernel_warp :304-404, serialization :417-503,
    compaction :563-613) and gpujpeg_huffman_gpu_decoder.cu (table kernel :546-610, decode_kernel :397-495) -- compiled where they lie and run under
    cudaemu's warp mode (32 lanes in lock step: votes, code words exchanged through shared memory). For every configuration:
    reference GPU Huffman encoder bytes == reference CPU Huffman encoder bytes == oracle, reference GPU Huffman decoder coefficients == oracle,
    and the counters prove the kernels ran (the reference takes its CPU coders for restart interval 0 / fewer than 32 segments)."""
    raw = make_raw(O, case)
    p, pi = api_params(ref, G, case)
    img = oracle_image(O, case)
    enc = G.Encoder(ref)
    before = _warp_stats(ref)
    jpeg = enc.encode(p, pi, raw)
    after = _warp_stats(ref)
    want = O.encode(img, raw)
    assert np.array_equal(jpeg, want), "reference GPU Huffman encoder stream != oracle"
    if case[6] != 0:  # src/gpujpeg_encoder.c:510-533: restart interval 0 is coded by the CPU Huffman coder
        # encode_kernel_warp + serialization + compaction (the decomposition-table kernel ran when the encoder was created)
        assert after[0] - before[0] == 3 and after[2] > before[2] and after[3] > before[3], (before, after)
    else:
        assert after[0] == before[0]
    out, size = C.POINTER(C.c_uint8)(), C.c_size_t()
    ref.L.gjref_reencode_cpu_huffman.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    assert ref.L.gjref_reencode_cpu_huffman(enc.h, C.byref(out), C.byref(size)) == 0
    assert np.array_equal(np.ctypeslib.as_array(out, shape=(size.value,)), jpeg), "reference GPU Huffman encoder != reference CPU Huffman encoder"

    dec = G.Decoder(ref)
    before = _warp_stats(ref)
    px, _ = dec.decode(jpeg)
    after = _warp_stats(ref)
    n = C.c_size_t()
    ref.L.gjref_decoder_coefficients.restype = C.POINTER(C.c_int16)
    ref.L.gjref_decoder_coefficients.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    got = np.ctypeslib.as_array(ref.L.gjref_decoder_coefficients(dec.h, C.byref(n)), shape=(n.value,)).copy()
    st = O.parse(want)
    assert np.array_equal(got, O.huffman_decode(st, want)), "reference GPU Huffman decoder coefficients != oracle"
    assert np.array_equal(px, O.decode(want)[0])
    segments = img.segment_count
    if segments >= 32:  # src/gpujpeg_decoder.c:255-268: fewer than 32 segments go to the CPU Huffman decoder
        assert after[0] - before[0] == 2 and after[1] > before[1], (segments, before, after)  # table kernel + decode kernel


@pytest.mark.parametrize("seed", range(160))
def test_random_configurations(O, G, ref, seed):
    """The restatement against the reference (its host C + its CUDA kernels on the CPU, contraction off) on random configurations: pixel
    formats, colour spaces, chroma samplings, odd sizes, qualities, restart intervals, interleaving. tests/test_gpu_parity.py runs the
    product against the restatement on the same cases."""
    from conftest import random_case, random_raw
    case = random_case(seed)
    if case[8] and case[8][0][0] == 4:
        pytest.skip("4:1:1 takes the reference's dynamic-sampling kernel, which divides by the zero sampling factor of the unused fourth "
                    "component (src/gpujpeg_preprocessor.cu:53-63): ignored by a GPU, a trap on the CPU; covered on the GPU by test_gpu_refhip.py")
    raw = random_raw(O, case, seed)
    p, pi = api_params(ref, G, case)
    enc = G.Encoder(ref)
    jpeg = enc.encode(p, pi, raw)
    want = O.encode(oracle_image(O, case), raw)
    assert jpeg.size == want.size and np.array_equal(jpeg, want), (case, "stream differs")
    # (round 6: `jpeg` comes out of the reference's Huffman GPU kernels under cudaemu's warp mode; the same coefficients through its CPU Huffman coder)
    out, size = C.POINTER(C.c_uint8)(), C.c_size_t()
    ref.L.gjref_reencode_cpu_huffman.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    assert ref.L.gjref_reencode_cpu_huffman(enc.h, C.byref(out), C.byref(size)) == 0
    assert np.array_equal(np.ctypeslib.as_array(out, shape=(size.value,)), jpeg), (case, "reference GPU Huffman encoder != reference CPU Huffman encoder")
    px, info = G.Decoder(ref).decode(jpeg)
    opx, oinfo = O.decode(want)
    assert (info.width, info.height, info.pixel_format, info.color_space) == (oinfo.width, oinfo.height, oinfo.pixel_format, oinfo.color_space)
    assert np.array_equal(px, opx), (case, "decoded samples differ")


@pytest.mark.parametrize("case", [c for c in CASES if c[6] != 0][:8], ids=lambda c: c[0])
def test_segment_info_index(O, G, ref, case):
    """APP13 segment index (src/gpujpeg_writer.c:522-623) written and consumed."""
    raw = make_raw(O, case)
    p, pi = api_params(ref, G, case, segment_info=1)
    jpeg = G.Encoder(ref).encode(p, pi, raw)
    want = O.encode(oracle_image(O, case, segment_info=1), raw)
    assert np.array_equal(jpeg, want)
    px, _ = G.Decoder(ref).decode(jpeg)
    assert np.array_equal(px, O.decode(want)[0])


@pytest.mark.parametrize("quality", [1, 10, 25, 49, 50, 51, 75, 90, 99, 100])
def test_quantisation_tables(O, ref, quality):
    ref.L.gjref_quant_tables.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_uint16)]
    for t in (0, 1):
        raw, fwd, inv = (C.c_uint8 * 64)(), (C.c_float * 64)(), (C.c_uint16 * 64)()
        ref.L.gjref_quant_tables(t, quality, raw, fwd, inv)
        oraw, ofwd, oinv = (C.c_uint8 * 64)(), (C.c_float * 64)(), (C.c_uint16 * 64)()
        O.lib().gjo_quant_table(t, quality, oraw, ofwd, oinv)
        assert bytes(raw) == bytes(oraw)
        assert np.array_equal(np.array(fwd[:], np.float32).view(np.uint32), np.array(ofwd[:], np.float32).view(np.uint32)), "forward table must be bit-identical"
        assert list(inv) == list(oinv)


@pytest.mark.parametrize("pf,w,h", [(1, 641, 481), (3, 322, 77), (5, 33, 35), (4, 33, 35), (2, 10, 10), (0, 99, 3), (6, 17, 9)])
def test_output_format_requests(O, G, ref, pf, w, h):
    """Decoder output formats other than the default: native planar / packed layouts and colour spaces."""
    cs = 1 if pf in (1, 6) else 3
    raw = O.noise(O.raw_size(w, h, pf), seed=pf + w)
    case = ("x", w, h, pf, cs, 80, 4, 1 if pf != 0 else 0, None, 3)
    p, pi = api_params(ref, G, case)
    jpeg = G.Encoder(ref).encode(p, pi, raw)
    for opf, ocs in [(pf, cs), (1, 1), (G.PIXFMT_NATIVE, G.NONE)]:
        dec = G.Decoder(ref)
        dec.set_output_format(ocs, opf)
        px, info = dec.decode(jpeg)
        opx, oinfo = O.decode(jpeg, info.pixel_format, info.color_space)
        assert np.array_equal(px, opx), (opf, ocs)


# ---- the format-conversion matrix (tests/test_format_matrix.py): the restatement pinned to the reference for every cell the product is compared on
def test_format_matrix_encode_cells(O, G, ref):
    """Every cell of the encode matrix: the reference's bytes are the restatement's. This includes the generic load of an odd-width planar 4:2:2
    image (W*H + pos/2, src/gpujpeg_preprocessor.cu:88-159), which is deterministic and stays as the reference has it. The matrix holds packed
    4:2:2 input at even widths only.
    One kind of cell cannot be run: three components in a sampling the reference has no specialised kernel for (4:1:1, 4:1:0, mixed) take its
    dynamic-sampling kernel, which divides by the zero factor of the unused fourth component (src/gpujpeg_preprocessor.cu:53-63) -- a trap on the
    CPU, a fault when compiled for gfx950 (tests/test_gpu_refhip.py), so the reference shows no behaviour for them anywhere. The same kernel and the
    same three samplings ARE pinned here by the matrix's four-component cells (SAMPLINGS4: every factor set), and what the reference's decoder makes
    of the restatement's 4:1:1, 4:1:0 and mixed streams by test_format_matrix_decode_cells."""
    import test_format_matrix as M
    dynamic3 = (M.SAMPLINGS["411"], M.SAMPLINGS["410"], M.SAMPLINGS["mixed"])
    not_run, dynamic4 = set(), set()
    for case, pad in M.ENCODE_CELLS:
        assert not (case[3] == 3 and case[1] % 2)  # odd-width packed 4:2:2: the reference reads past the caller's buffer -- never run
        if case[8] in dynamic3:
            not_run.add(case[8])  # the dynamic-sampling kernel with three components divides by zero: see above
            continue
        raw, img, want = M.make_cell(O, case, pad)
        p, pi = api_params(ref, G, case)
        pi.width_padding = pad
        enc = G.Encoder(ref)  # (a fresh one per cell, as the tests above have it)
        got = enc.encode(p, pi, raw)
        enc.close()
        assert got.size == want.size and np.array_equal(got, want), (case[0], pad)
        if img.comp_count == 4:
            dynamic4.add(case[8])
    assert not_run == set(dynamic3)
    assert dynamic4 == set(M.SAMPLINGS4.values())  # (plain 4:4:4:4, and 4:1:1, 4:1:0 and mixed with a fourth component)


@pytest.mark.parametrize("kind,il", [(k, i) for k in ("444", "422", "420", "440", "411", "410", "mixed") for i in (0, 1)] + [("grey", 0), ("4444", 1), ("4444", 0)])
def test_format_matrix_decode_cells(O, G, ref, kind, il):
    """Every cell of the decode matrix: the reference's pixels, size and reported parameters are the restatement's -- but for the two kinds of cell
    the restatement leaves the reference on purpose, which are not run."""
    import test_format_matrix as M
    skipped = set()
    for w, h in M.SIZES:
        jpeg = M.make_stream(O, kind, il, w, h)
        for pf, cs in M.OUTPUTS:
            want = M.oracle_decode(O, jpeg, pf, cs, kind, il)
            if want is None:
                assert pf == 3 and w % 2
                skipped.add("packed")  # odd-width packed 4:2:2: the reference stores past the end of its output buffer -- no behaviour to match
                continue
            raw, img = want
            if img.pixel_format == 4 and w % 2 and h > 1 and M.decode_route(img, False) == "postprocess":
                skipped.add("planar")  # odd-width planar 4:2:2 through the per-pixel store: two pixels of the reference share a byte -- a race
                continue  # (1x1 has no second row to collide with and is run)
            dec = G.Decoder(ref)
            dec.set_output_format(cs, pf)
            px, info = dec.decode(jpeg)
            dec.close()
            assert (info.width, info.height, info.pixel_format, info.color_space) == (img.width, img.height, img.pixel_format, img.color_space), (w, h, pf, cs)
            assert px.size == raw.size and np.array_equal(px, raw), (w, h, pf, cs, int(np.count_nonzero(px != raw)))
    # (a 4:2:2 stream's planar 4:2:2 output is its own layout: k_copy_planes_out's side, the reference's memcpy -- pinned above at odd widths too)
    assert skipped == ({"packed"} if kind == "422" else {"packed", "planar"})


@pytest.mark.parametrize("pf,mapping,flip", [(1, "210", False), (1, "F0Z", True), (6, "1230", True), (1, "012", True)])
def test_channel_remap_and_flip_options(O, G, ref, pf, mapping, flip):
    """The reference's own option parsing, call order (src/gpujpeg_encoder.c:661-699,767-771, src/gpujpeg_decoder.c:499-503) and
    kernels (channel_remap_kernel, vertical_flip_kernel: src/gpujpeg_preprocessor.cu:455-559) against the restated in-place channel
    permutation and plane flip. Packed formats only: for a planar format the reference computes the row pitch as
    width * component count (src/gpujpeg_preprocessor.cu:520-523) and its kernel then reads and writes past the end of the image
    (offset up to 3 * w * h in a plane of w * h bytes), so there is no reference behaviour to match; the product and the
    restatement permute the planes (tests/test_gpu_parity.py)."""
    w, h = 88, 52
    cs = 1 if pf in (1, 6) else 3
    raw = O.noise(O.raw_size(w, h, pf), seed=3 * pf + len(mapping))
    case = ("x", w, h, pf, cs, 85, 5, 1 if pf == 6 else 0, [(1, 1)] * 4 if pf == 6 else None, 3)
    img = oracle_image(O, case)
    planes = O.preprocess(img, O.channel_remap(img, raw, mapping))
    if flip:
        planes = O.flip_planes(img, planes)
    want = O.encode_from_coefs(img, O.fdct_quant(img, planes))
    p, pi = api_params(ref, G, case)
    enc = G.Encoder(ref)
    assert enc.set_option("enc_opt_channel_remap", mapping) == 0
    assert enc.set_option("enc_opt_flipped", "1" if flip else "0") == 0
    assert np.array_equal(enc.encode(p, pi, raw), want)
    s = O.parse(want)
    dplanes = O.idct(s, O.huffman_decode(s, want))
    if flip:
        dplanes = O.flip_planes(s.img, dplanes)
    want_px = O.channel_remap(s.img, O.postprocess(s.img, dplanes), mapping)
    O.lib().gjo_stream_free(C.byref(s))
    dec = G.Decoder(ref)
    assert ref.L.gpujpeg_decoder_set_option(dec.h, b"dec_opt_channel_remap", mapping.encode()) == 0
    assert ref.L.gpujpeg_decoder_set_option(dec.h, b"dec_opt_flipped", b"1" if flip else b"0") == 0
    px, _ = dec.decode(want)
    assert np.array_equal(px, want_px)


@pytest.mark.parametrize("orientation", [None, "90", "180-"])
def test_exif_header_bytes(O, G, ref, lib, orientation):
    """enc_hdr=Exif: the APP1 segment of our writer against the reference's (src/gpujpeg_exif.c:172-450) byte by byte,
    except the DateTime value (wall clock). Host-only on our side (gpujpeg_amd_host_headers), full encode on the reference side."""
    w, h = 64, 48
    case = ("e", w, h, 1, 1, 75, -1, 0, None, 3)
    p, pi = api_params(ref, G, case)
    enc = G.Encoder(ref)
    assert enc.set_option("enc_hdr", "Exif") == 0
    if orientation:
        assert enc.set_option("enc_metadata", "orientation=" + orientation) == 0
    jpeg = bytes(enc.encode(p, pi, O.noise(w * h * 3)))
    assert jpeg[2:4] == b"\xff\xe1"
    n = 4 + int.from_bytes(jpeg[4:6], "big")
    want = bytearray(jpeg[2:n])
    # ours: header type 8 = GPUJPEG_HEADER_EXIF; orientation goes in through the metadata argument of the host helper
    import ctypes as C
    buf = (C.c_uint8 * 4096)()
    main = C.c_size_t()
    p2, pi2 = api_params(lib, G, case)
    fn = lib.L.gpujpeg_amd_host_headers_md
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]
    rot, flip = {None: (-1, 0), "90": (1, 0), "180-": (2, 1)}[orientation]
    got_n = fn(C.byref(p2), C.byref(pi2), 8, rot, flip, buf, 4096, C.byref(main))
    got = bytearray(bytes(buf[2:n]))
    assert got_n > 0 and len(got) == len(want)
    i = got.find(b"\x01\x32")  # DateTime tag id 0x0132: its 20-byte value sits at the offset stored in the entry
    off = int.from_bytes(got[i + 8:i + 12], "big") + 2 + 2 + 6  # marker(2)+len(2)+"Exif\0\0"(6) relative to the sliced buffer start
    # ... and the value of the Exif IFD pointer: the reference takes it from a compound literal that is out of scope when it is
    # read (src/gpujpeg_exif.c:297-300), so this gcc build of it emits stack garbage there; ours stores the real offset
    j = got.find(b"\x87\x69")
    assert int.from_bytes(got[j + 8:j + 12], "big") + 10 == got.find(b"\x90\x00") - 2  # points at the entry count before ExifVersion
    for b in (got, want):
        b[off:off + 20] = b"x" * 20
        b[j + 8:j + 12] = b"PPPP"
    assert got == want


EXIF_TAG_SETS = [
    ["0x010F:ASCII=MI355X build"],                                   # Make: a new tag in the 0th IFD, value behind the IFD
    ["Orientation=6", "0x9003:ASCII=2026:09:26 10:00:00"],           # replaces a built-in tag; private tag with a long value
    ["XResolution=300/1", "YResolution=300/1", "0x829A:RATIONAL=1/250", "0x8827:SHORT=400", "0xA405:SHORT=35"],
    ["WhitePoint=313/1000,329/1000", "0x0100:LONG=640", "0x9286:UNDEFINED=raw comment"],
    ["PixelXDimension=77"],                                          # replaced private tag: the reference keeps a stale copy of the last built-in one
    ["0x9204:SRATIONAL=-1/3", "0x0101:BYTE=1,2,3", "0x0102:BYTE=1,2,3,4,5"],
]


@pytest.mark.parametrize("tags", EXIF_TAG_SETS, ids=[str(i) for i in range(len(EXIF_TAG_SETS))])
def test_custom_exif_tags(O, G, ref, lib, tags):
    """enc_exif_tag: user tags in either IFD, replacing built-in ones, sorted by id, long values behind their IFD
    (src/gpujpeg_exif.c:172-600) -- the APP1 segment equals the reference's except DateTime and the Exif IFD pointer
    (see test_exif_header_bytes)."""
    import ctypes as C
    w, h = 64, 48
    case = ("e", w, h, 1, 1, 75, -1, 0, None, 3)
    p, pi = api_params(ref, G, case)
    enc = G.Encoder(ref)
    for t in tags:
        assert enc.set_option("enc_exif_tag", t) == 0
    jpeg = bytes(enc.encode(p, pi, O.noise(w * h * 3)))
    enc.h = None  # the reference's gpujpeg_exif_tags_destroy (src/gpujpeg_exif.c:592-598) advances the wrong loop variable and corrupts
    #               the heap when an IFD has two or more user tags: this encoder is deliberately not destroyed
    assert jpeg[2:4] == b"\xff\xe1"
    n = 4 + int.from_bytes(jpeg[4:6], "big")
    want = bytearray(jpeg[2:n])
    buf = (C.c_uint8 * 8192)()
    main = C.c_size_t()
    p2, pi2 = api_params(lib, G, case)
    fn = lib.L.gpujpeg_amd_host_headers_exif
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_uint8), C.c_size_t,
                   C.POINTER(C.c_size_t)]
    arr = (C.c_char_p * len(tags))(*[t.encode() for t in tags])
    assert fn(C.byref(p2), C.byref(pi2), 0, -1, 0, arr, len(tags), buf, 8192, C.byref(main)) > 0
    got = bytearray(bytes(buf[2:n]))
    assert bytes(buf[n:n + 2]) == jpeg[n:n + 2], "same segment length"

    def records(b):  # 0th IFD records by tag id -> (record offset)
        base = 2 + 2 + 6  # marker, length, "Exif\0\0"
        cnt = int.from_bytes(b[base + 8:base + 10], "big")
        return {int.from_bytes(b[base + 10 + 12 * i:base + 12 + 12 * i], "big"): base + 10 + 12 * i for i in range(cnt)}
    rg, rw = records(got), records(want)
    assert sorted(rg) == sorted(rw) and list(rg) == sorted(rg), "records sorted by id"
    for b, r in ((got, rg), (want, rw)):
        if 0x132 in r and not any(t.lower().startswith("datetime") for t in tags):
            off = int.from_bytes(b[r[0x132] + 8:r[0x132] + 12], "big") + 10
            b[off:off + 20] = b"x" * 20          # DateTime: wall clock
        b[r[0x8769] + 8:r[0x8769] + 12] = b"PPPP"  # Exif IFD pointer: unspecified in the reference
    assert got == want
    # our pointer is the real offset of the Exif IFD: its first record is ExifVersion unless a smaller private id was added
    raw = bytes(buf[2:n])
    ptr = int.from_bytes(raw[rg[0x8769] + 8:rg[0x8769] + 12], "big") + 10
    cnt = int.from_bytes(raw[ptr:ptr + 2], "big")
    ids = [int.from_bytes(raw[ptr + 2 + 12 * i:ptr + 4 + 12 * i], "big") for i in range(cnt)]
    assert ids == sorted(ids) and 0x9000 in ids


def test_custom_exif_tag_errors(lib):
    import ctypes as C
    fn = lib.L.gpujpeg_amd_host_headers_exif
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_uint8), C.c_size_t,
                   C.POINTER(C.c_size_t)]
    p = lib.default_parameters()
    p.verbose = -1
    pi = lib.default_image_parameters()
    pi.width, pi.height = 64, 48
    buf = (C.c_uint8 * 8192)()
    for bad in ("NoSuchName=1", "0x10F=x", "0x10F:FLOAT=1", "0x10F:SHORT", "Orientation=6x", "0x10F:ASCII=" + "x" * 4000):
        arr = (C.c_char_p * 1)(bad.encode())
        assert fn(C.byref(p), C.byref(pi), 0, -1, 0, arr, 1, buf, 8192, None) == 0, bad


STRESS = [("natural", 704, 512, 30), ("natural", 704, 512, 75), ("natural", 704, 512, 95), ("noise", 256, 256, 100), ("noise", 256, 256, 50),
          ("flat", 256, 64, 75)]


def _stress_raw(O, kind, w, h, q):
    from conftest import natural_image
    if kind == "natural":
        return natural_image(w, h, 3, seed=q)
    if kind == "noise":
        return O.noise(w * h * 3, seed=q)
    return np.full(w * h * 3, 128 + (q % 3), np.uint8)   # tie-adjacent: every AC coefficient is an exact 0, DC sits on the table


@pytest.mark.parametrize("kind,w,h,q", STRESS, ids=[f"{k}_{q}" for k, _, _, q in STRESS])
def test_float_stages_stress(O, G, ref, kind, w, h, q):
    """Larger frames through the reference's own fDCT+quantiser and dequantiser+IDCT kernels (src/gpujpeg_dct_gpu.cu:180-295,
    :472-618, contraction off) against the restatement in the same mode: every byte of the stream, every decoded sample."""
    raw = _stress_raw(O, kind, w, h, q)
    case = ("s", w, h, 1, 1, q, -1, 0, None, 3)
    p, pi = api_params(ref, G, case)
    jpeg = G.Encoder(ref).encode(p, pi, raw)
    want = O.encode(oracle_image(O, case), raw)
    assert np.array_equal(jpeg, want)
    px, _ = G.Decoder(ref).decode(jpeg)
    assert np.array_equal(px, O.decode(want)[0])


@pytest.mark.parametrize("compiler", ["gcc", "clang"])
def test_contraction_sensitivity(O, G, compiler, capsys):
    """How far the results move when a HOST compiler chooses the fusions (g++ / clang++ -ffp-contract=fast -mfma on the reference's
    .cu files): not a parity statement, the measured size of the risk that DESIGN.md section 3 discusses. The restatement runs
    with its pinned map (the one hipcc produces for gfx950, tests/test_gpu_refhip.py). Streams must be identical (a coefficient
    changes only when a product lands within an ulp of a rounding tie); decoded samples may differ by at most 2 levels in at
    most 0.1 % of the samples."""
    import os
    path = O.REF_FMA_PATHS[compiler]
    if not os.path.exists(path):
        pytest.skip("needs /root/reference")
    lib = G.Library(path)
    differing = total = worst = files = 0
    for case in CASES:
        raw = make_raw(O, case)
        p, pi = api_params(lib, G, case)
        jpeg = G.Encoder(lib).encode(p, pi, raw)
        want = O.encode(oracle_image(O, case), raw)
        files += not np.array_equal(jpeg, want)
        px, _ = G.Decoder(lib).decode(want)
        opx, _ = O.decode(want)
        d = np.abs(px.astype(np.int16) - opx.astype(np.int16))
        differing += int((d != 0).sum())
        total += d.size
        worst = max(worst, int(d.max()))
    with capsys.disabled():
        print(f"\n[contraction sensitivity] {compiler} -ffp-contract=fast vs pinned map: {files} of {len(CASES)} streams differ, "
              f"{differing} of {total} decoded samples differ, max |diff| {worst}")
    assert files == 0
    assert differing <= total // 1000 and worst <= 2
