// gj_enc_assemble.hip -- MI355X (gfx950, wave64) JPEG encoder: the streams the coders leave -> the finished file, on the device
// (part of the encoder's device code, see gj_enc_internal.h for the map of the files)
//   k_gather              tile streams of the fused encoders -> the file: stuffing in flight, RSTn, scan headers, EOI, result words
//   k_scan_segments       prefix sum of the stuffed segment sizes -> final byte offsets   } behind k_huffman (coefficient planes),
//   k_assemble            byte stuffing + RSTn + scan headers + EOI, in stream order      } k_scan_segments also for the APP13 index
//   k_segment_info        APP13 segment index (src/gpujpeg_writer.c:522-623)
#include "gj_enc_internal.h"

// ================================================================================================
// k_gather: the tile streams -> the file. Replaces k_scan_segments + k_assemble behind the k_encode_* kernels (the reference:
// serialisation + compaction kernels and the host's stitching, src/gpujpeg_huffman_gpu_encoder.cu:417-613, src/gpujpeg_encoder.c:567-629).
//
// An encoder workgroup leaves the UNSTUFFED stream of its tile in the tile's area of d_temp (segments on dword boundaries, back to back),
// the segments' byte counts, the size the tile's stream will have in the file, and adds that size to the total of its group of
// 32 tiles (one atomic, nobody waits for it). Here ONE WAVE takes one tile stream, ~6000 waves at once for an 8K frame, on its own: the
// four waves of a workgroup share nothing and never wait for each other. Which tile a wave has is the same for its 64 lanes, and the
// compiler is told so (readfirstlane of the wave index): scan, segment range, source address, header sizes live in scalar registers.
// Everything the wave needs is asked for in one trip: the group totals and the sizes of its group's tiles in front of it (their sum
// is its place in the file: two wave reductions), its segments' byte counts, and the first 2 KB of its stream (where those are follows
// from the launch's geometry, not from loaded values).
// Then the stream is stuffed in flight, 256 dwords a round: a lane takes FOUR consecutive dwords with one 16-byte load (tile areas start
// on multiples of GJ_TEMP_BYTES_PER_BLOCK = 13 x 16 bytes) and the four bytes LDS holds for them: a segment's lane has noted at the
// segment's LAST dword how many of its bytes do not count and whether a restart marker follows, and which. The bytes a lane puts
// into the file are then 16 + its 0xFF bytes - the bytes that do not count + 2 per marker, and ONE wave prefix sum per round places
// every lane: no dword has to know its segment. A lane whose dwords are whole, unmarked and free of 0xFF leaves them as one unaligned
// 16-byte store; another lane stores its clean dwords one by one, and the few that are left (0xFF inside, a segment's end) go byte by
// byte, one such dword per lane and turn, as long as any lane has one.
// Round 3 needed a launch for the offsets (5 us), a wave per four segments with two dependent trips and byte stores (16 us), and
// 19 MB of traffic for the same; up to round 6 a lane took one dword a round, found its segment with a second prefix sum and two
// ds_bpermute, and the workgroup's waves met at four barriers for two workgroup scans of which only the totals were used.
// ================================================================================================
#define GJ_GATHER_PRELOAD 2 // rounds of 256 dwords whose loads are issued before anything is known about the tile stream
#define GJ_GATHER_MARK_DW 2048 // dwords of a tile stream whose segment ends are noted in LDS at a time
#ifndef GJ_GATHER_STORE16
#define GJ_GATHER_STORE16 1 // 1: a clean lane leaves with one unaligned 16-byte store, 0: with four unaligned dword stores (profiles/gather_wide.md)
#endif
// -DGJ_TRACE_PHASES (the `trace` target of the Makefile, tools/gather_valu_budget.py): gj_hip_trace_stop_gather(n) ends every wave at stamp n, so
// that SQ_INSTS_VALU of the launch counts the vector instructions in front of that stamp (as gj_hip_trace_stop_encoder in gj_enc_tiles.hip)
#ifdef GJ_TRACE_PHASES
static __device__ int gj_trace_stop_g = 1 << 30;
extern "C" GJ_HIP_API int gj_hip_trace_stop_gather(int n) { return hipMemcpyToSymbol(HIP_SYMBOL(gj_trace_stop_g), &n, sizeof n) == hipSuccess ? 0 : -1; }
#define GJ_TRACE_G(slot) do { if ((slot) >= gj_trace_stop_g) __builtin_amdgcn_endpgm(); } while (0)
#else
#define GJ_TRACE_G(slot) ((void)0)
#endif
// what a segment notes at its last dword: bits 0-2 one bit per byte of the dword that does not count (0 .. 3 of them), bits 3-4 both set when a
// restart marker follows (popcount = its two bytes), bits 5-7 which
#define GJ_GATHER_PAD 0x07070707u
#define GJ_GATHER_RST 0x18181818u
__global__ __launch_bounds__(256) void k_gather(const GjTail T0)
{
    GjTail T = T0;
    { // frame blockIdx.z of a batch: its own tile list, group totals, tile streams, segment counts, stream buffer and result words
        const size_t fz = blockIdx.z;
        T.piece += fz * T0.f_tail; T.group += fz * T0.f_tail; T.group_other += fz * T0.f_tail;
        T.temp += fz * T0.f_temp; T.seg_bytes += fz * T0.f_seg;
        T.jpeg += fz * T0.f_jpeg; T.d_result += fz * 2;
        if (T.h_result) T.h_result += fz * 2;
    }
    __shared__ __attribute__((aligned(16))) uint8_t s_mark[4][GJ_GATHER_MARK_DW];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (the same in all lanes: what follows from it is scalar)
    const uint32_t P = T.npieces, NG = T.ngroups;
    const uint32_t p = blockIdx.x * 4u + wave;
    if (blockIdx.x == 0) // the next call's group totals
        for (uint32_t g = threadIdx.x; g < NG; g += 256) T.group_other[g] = 0;
    if (p >= P) return; // (a wave without a tile: nobody waits for it)
    // ---- this wave's tile stream: where its segments and its bytes are (no loaded value needed)
    const uint32_t scan = gj_tail_scan_of(T, p);
    const uint32_t t = p - gj_pick4(T.scan_first, scan), seg0 = t * T.spt, scan_segs = gj_pick4(T.segs, scan);
    const uint32_t nseg = min(T.spt, scan_segs - seg0);
    const uint32_t s0 = gj_pick4(T.seg_first, scan) + seg0;
    const uint64_t src_block = (uint64_t)gj_pick4(T.block_first, scan) + (uint64_t)seg0 * T.seg_blocks;
    const uint32_t* const src = reinterpret_cast<const uint32_t*>(T.temp + src_block * GJ_TEMP_BYTES_PER_BLOCK); // (a multiple of 16 bytes: gj_hip_encode asserts it)
    // dwords of the tile's area, a multiple of four: nothing is read behind them, nor behind the buffer (the area of a scan's last tile ends
    // with its last, shorter segment; found by the execution model under AddressSanitizer in round 4: the preload below read up to 35 blocks further)
    const uint64_t room = T.temp_blocks > src_block ? T.temp_blocks - src_block : 0u;
    const uint32_t src_dw = (uint32_t)min((uint64_t)nseg * T.seg_blocks, room) * (GJ_TEMP_BYTES_PER_BLOCK / 4u);
    // ---- one trip: group totals, the sizes of the tiles of the group in front of this one, the segments' byte counts, the first rounds of the stream
    const uint32_t ga = p >> 5;
    uint32_t before = 0, all = 0;
    for (uint32_t g0 = 0; g0 < NG; g0 += 256) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t g = g0 + (uint32_t)u * 64u + lane;
            v[u] = g < NG ? T.group[g] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t g = g0 + (uint32_t)u * 64u + lane;
            all += v[u];
            before += g < ga ? v[u] : 0u;
        }
    }
    if (lane < (p & 31u)) before += T.piece[(ga << 5) + lane];
    const uint32_t nb = lane < nseg ? T.seg_bytes[s0 + lane] : 0u;
    uint4 pre[GJ_GATHER_PRELOAD];
#pragma unroll
    for (int m = 0; m < GJ_GATHER_PRELOAD; m++) {
        const uint32_t d = (uint32_t)m * 256u + 4u * lane;
        pre[m] = d < src_dw ? *reinterpret_cast<const uint4*>(src + d) : make_uint4(0u, 0u, 0u, 0u);
    }
    const uint32_t done_bytes = (uint32_t)__builtin_amdgcn_readlane((int)gj_wave_incl_scan(before), 63);
    const uint32_t all_bytes = (uint32_t)__builtin_amdgcn_readlane((int)gj_wave_incl_scan(all), 63);
    const uint64_t total = (uint64_t)T.main_hdr + gj_pick4(T.hdr_end, gj_tail_scan_of(T, P - 1)) + all_bytes + 2u;
    const bool overflow = total > T.capacity;
    uint8_t* const out = T.jpeg;
    if (p == P - 1 && lane == 0) { // (the wave of the last tile stream)
        T.d_result[0] = (uint32_t)total;
        T.d_result[1] = overflow ? 1u : 0u;
        if (T.h_result) { // the host's (pinned, device-visible) copy: no copy launch behind the kernel
            T.h_result[0] = (uint32_t)total;
            T.h_result[1] = overflow ? 1u : 0u;
        }
        if (!overflow) { // EOI: the file's last two bytes
            out[(uint32_t)total - 2u] = 0xFF;
            out[(uint32_t)total - 1u] = 0xD9;
        }
    }
    if (overflow) return;
    const uint32_t F = T.main_hdr + gj_pick4(T.hdr_end, scan) + done_bytes; // the tile stream's first byte in the file
    if (t == 0) { // first tile of a scan: its header (APP13 placeholders + SOS) sits right in front
        const uint32_t h1 = gj_pick4(T.hdr_end, scan), h0 = scan == 0 ? 0u : gj_pick4(T.hdr_end, scan - 1);
        for (uint32_t b = lane; b < h1 - h0; b += 64) out[F - (h1 - h0) + b] = T.scan_hdr[h0 + b];
    }
    GJ_TRACE_G(1); // set up: the file offset is known
    // ---- lane sl keeps segment sl: its last dword in the tile stream and what it notes there
    const uint32_t last = scan_segs - seg0 - 1u; // (local index of the scan's last segment: no restart marker behind it)
    const uint32_t ndw = (nb + 3u) >> 2;
    const uint32_t dwi = gj_wave_incl_scan(ndw);
    const uint32_t total_dw = (uint32_t)__builtin_amdgcn_readlane((int)dwi, 63);
    const uint32_t note = ((1u << (4u * ndw - nb)) - 1u) | (lane != last ? 0x18u | (((seg0 + lane) & 7u) << 5) : 0u); // (RSTn: src/gpujpeg_huffman_gpu_encoder.cu:497-502)
    GJ_TRACE_G(2); // segment books
    uint8_t* const mark = s_mark[wave];
    uint32_t pos = F; // where the round's first byte goes
    for (uint32_t c0 = 0; c0 < total_dw; c0 += GJ_GATHER_MARK_DW) { // (tile streams of more dwords take several passes)
        const uint32_t c1 = min(total_dw, c0 + (uint32_t)GJ_GATHER_MARK_DW);
        gj_wave_sync();
        // (a byte per dword: a lane's 16 bytes are 16 dwords' notes; whole rounds of 256 dwords are cleared)
        static_assert(GJ_GATHER_MARK_DW == 2048, "two clearing stores of 1024 bytes");
        reinterpret_cast<uint4*>(mark)[lane] = make_uint4(0u, 0u, 0u, 0u);
        if (c1 - c0 > 1024u) reinterpret_cast<uint4*>(mark)[64u + lane] = make_uint4(0u, 0u, 0u, 0u);
        gj_wave_sync();
        if (lane < nseg && dwi - 1u >= c0 && dwi - 1u < c1) mark[dwi - 1u - c0] = (uint8_t)note;
        gj_wave_sync();
        for (uint32_t r0 = c0; r0 < c1; r0 += 256u) {
            const uint32_t d0 = r0 + 4u * lane;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (r0 < GJ_GATHER_PRELOAD * 256u) {
#pragma unroll
                for (int q = 0; q < GJ_GATHER_PRELOAD; q++)
                    if (r0 == (uint32_t)q * 256u) x = pre[q];
            } else if (d0 < total_dw && d0 < src_dw) {
                x = *reinterpret_cast<const uint4*>(src + d0);
            }
            uint32_t v[4] = {x.x, x.y, x.z, x.w};
            const uint32_t M = *reinterpret_cast<const uint32_t*>(mark + (d0 - c0));
            const uint32_t nlive = (uint32_t)min(4, max(0, (int)(total_dw - d0))); // the lane's dwords that belong to the stream
            if (r0 + 256u > total_dw) { // (the stream's last round: what lies behind it in the area is not looked at)
#pragma unroll
                for (int k = 1; k < 4; k++) v[k] = (uint32_t)k < nlive ? v[k] : 0u;
                v[0] = nlive ? v[0] : 0u;
            }
            uint32_t ffm[4], ffc = 0; // (the bytes behind a segment's end are zero)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                ffm[k] = ((v[k] & 0x7F7F7F7Fu) + 0x01010101u) & v[k] & 0x80808080u;
                ffc += (uint32_t)__builtin_popcount(ffm[k]);
            }
            const uint32_t bytes = 4u * nlive + ffc + (uint32_t)__builtin_popcount(M & GJ_GATHER_RST) - (uint32_t)__builtin_popcount(M & GJ_GATHER_PAD);
            const uint32_t bi = gj_wave_incl_scan(bytes);
            uint32_t q = pos + bi - bytes;
            pos += (uint32_t)__builtin_amdgcn_readlane((int)bi, 63);
            uint32_t dirty = 0, qk[4]; // the lane's dwords that go byte by byte, and where each dword's bytes go
            if ((M | ffm[0] | ffm[1] | ffm[2] | ffm[3]) == 0 && nlive == 4) {
#if GJ_GATHER_STORE16
                __builtin_memcpy(out + q, v, 16);
#else
#pragma unroll
                for (int k = 0; k < 4; k++) *reinterpret_cast<gj_u32_unaligned*>(out + q + 4 * k) = v[k];
#endif
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t mk = (M >> (8 * k)) & 0xFFu;
                    qk[k] = q;
                    if ((uint32_t)k < nlive) {
                        if ((mk | ffm[k]) == 0) *reinterpret_cast<gj_u32_unaligned*>(out + q) = v[k];
                        else dirty |= 1u << k;
                    }
                    q += 4u + (uint32_t)__builtin_popcount(ffm[k]) + (uint32_t)__builtin_popcount(mk & 0x18u) - (uint32_t)__builtin_popcount(mk & 0x07u);
                }
            }
            while (__ballot(dirty != 0)) { // a turn: every lane that has one writes one such dword
                if (dirty) {
                    const uint32_t k = (uint32_t)__builtin_ctz(dirty);
                    dirty &= dirty - 1u;
                    const uint32_t w = k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
                    uint32_t o = k == 0 ? qk[0] : k == 1 ? qk[1] : k == 2 ? qk[2] : qk[3];
                    const uint32_t mk = (M >> (8u * k)) & 0xFFu;
                    const int vb = 4 - __builtin_popcount(mk & 0x07u);
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (b < vb) {
                            const uint32_t byte = (w >> (8 * b)) & 0xFFu;
                            out[o++] = (uint8_t)byte;
                            if (byte == 0xFFu) out[o++] = 0;
                        }
                    if (mk & 0x08u) { // RSTn behind the segment's last dword
                        out[o] = 0xFF;
                        out[o + 1] = (uint8_t)(0xD0u + (mk >> 5));
                    }
                }
            }
        }
    }
    GJ_TRACE_G(3); // rounds (what follows is the kernel's end)
}

// the workgroup's Huffman tables in the layout of GjCoderLds::lut: the host has them ready behind its (code << 8 | size) tables
// (gj_enc_job::d_huff_lut + GJ_CODER_LUT_OFFSET, gj_huffman_coder_lut; worked out in the kernel they cost every wave ~60 vector instructions, round 5)
// ================================================================================================
// Final offsets: exclusive prefix sum over stuffed segment sizes (+2 for RSTn except at the end of a scan) and over
// the scan headers that precede each scan. One launch of ceil(S/1024) workgroups (k_scan_segments below): per-workgroup totals
// published with an epoch tag, every workgroup adds the totals of its predecessors (at most a few hundred values) to its local scan.
// ================================================================================================
__device__ __forceinline__ uint32_t gj_segment_out_size(const gj_enc_job& J, int s, uint32_t* hdr)
{
    const GjSeg sg = gj_segment(J.g, s);
    *hdr = 0;
    if (sg.first_in_scan) {
        const int scan = J.g.interleaved ? 0 : sg.comp;
        *hdr = J.scan_hdr_offset[scan + 1] - J.scan_hdr_offset[scan];
    }
    return J.d_seg_bytes[s] + J.d_seg_ff[s] + (sg.last_in_scan ? 0u : 2u);
}

// inclusive scan over a 1024-thread workgroup; s_w needs 16 words
__device__ __forceinline__ uint32_t gj_wg1024_incl_scan(uint32_t v, uint32_t* s_w, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = gj_wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        const uint32_t x = s_w[w];
        if (w < wave) off += x;
        all += x;
    }
    if (total) *total = all;
    return inc + off;
}

// One launch: every workgroup scans its 1024 segments, publishes its total tagged with the call's epoch, then adds up the
// totals of its predecessors as soon as they appear (all workgroups of a frame are resident at once and are dispatched
// in index order, so a predecessor never waits for a successor). The epoch tag makes clearing the slots unnecessary.
__global__ __launch_bounds__(1024) void k_scan_segments(const gj_enc_job J, unsigned long long* __restrict__ partial, const uint32_t epoch)
{
    __shared__ uint32_t s_w[16];
    const int S = J.g.segment_count;
    const int s = blockIdx.x * 1024 + threadIdx.x;
    uint32_t hdr = 0, v = 0;
    if (s < S) v = gj_segment_out_size(J, s, &hdr);
    uint32_t total;
    const uint32_t inc = gj_wg1024_incl_scan(v + hdr, s_w, &total);
    if (threadIdx.x == 0)
        __hip_atomic_store(&partial[blockIdx.x], ((unsigned long long)epoch << 32) | total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t pre = 0;
    for (unsigned t = threadIdx.x; t < blockIdx.x; t += 1024) {
        unsigned long long p;
        do {
            p = __hip_atomic_load(&partial[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        } while ((uint32_t)(p >> 32) != epoch);
        pre += (uint32_t)p;
    }
    uint32_t base;
    gj_wg1024_incl_scan(pre, s_w, &base);
    base += J.main_hdr_size;
    if (s < S) J.d_seg_out[s] = base + inc - v; // segment data start (its scan header sits right before)
    if (s == S - 1) {
        const uint32_t end = base + inc;
        const uint32_t size = end + 2; // EOI
        J.d_seg_out[S] = end;
        J.d_result[0] = size;
        J.d_result[1] = (uint64_t)size > J.jpeg_capacity ? 1u : 0u;
        if (J.h_result) { // the host's (pinned, device-visible) copy: no copy launch behind the kernels
            J.h_result[0] = size;
            J.h_result[1] = (uint64_t)size > J.jpeg_capacity ? 1u : 0u;
        }
    }
}

// ================================================================================================
// Stream assembly: one WAVE per segment. Reads the unstuffed bytes, inserts 0x00 after every 0xFF
// (ballot-free: per-lane counts + wave prefix sum), appends RSTn, and the first / last segment of a scan
// also writes the scan header / EOI. Replaces the reference's serialisation + compaction kernels and the
// host-side stitching loop (src/gpujpeg_huffman_gpu_encoder.cu:417-613, src/gpujpeg_encoder.c:567-629).
// ================================================================================================
                      // instead of four; 43 200 waves of one short segment each spent their time waiting)
__global__ __launch_bounds__(256) void k_assemble(const gj_enc_job J)
{
    const gj_geom& g = J.g;
    const int s0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * GJ_ASM_SEGS;
    const int lane = threadIdx.x & 63;
    if (s0 >= g.segment_count || J.d_result[1]) return;
    uint8_t* out = J.d_jpeg;
    uint32_t raw4[GJ_ASM_SEGS], o4[GJ_ASM_SEGS], w4[GJ_ASM_SEGS];
    const uint8_t* src4[GJ_ASM_SEGS];
#pragma unroll
    for (int q = 0; q < GJ_ASM_SEGS; q++) {
        const int s = min(s0 + q, g.segment_count - 1);
        raw4[q] = s0 + q < g.segment_count ? J.d_seg_bytes[s] : 0u;
        o4[q] = J.d_seg_out[s];
        src4[q] = J.d_temp + gj_segment(g, s).first_block * GJ_TEMP_BYTES_PER_BLOCK;
    }
#pragma unroll
    for (int q = 0; q < GJ_ASM_SEGS; q++) w4[q] = (uint32_t)lane * 4u < raw4[q] ? *reinterpret_cast<const uint32_t*>(src4[q] + lane * 4) : 0u;
#pragma unroll
    for (int q = 0; q < GJ_ASM_SEGS; q++) {
        const int s = s0 + q;
        if (s >= g.segment_count) break;
        const GjSeg sg = gj_segment(g, s);
        const uint32_t raw = raw4[q];
        const uint8_t* src = src4[q];
        uint32_t o = o4[q];
        if (sg.first_in_scan) { // scan header (APP13 placeholders + SOS) right before the first segment
            const int scan = g.interleaved ? 0 : sg.comp;
            const uint32_t h0 = J.scan_hdr_offset[scan], hn = J.scan_hdr_offset[scan + 1] - h0;
            for (uint32_t b = lane; b < hn; b += 64) out[o - hn + b] = J.d_scan_hdr[h0 + b];
        }
        for (uint32_t c0 = 0; c0 < raw; c0 += 256) {
            const uint32_t idx = c0 + lane * 4;
            uint32_t w = w4[q];
            int vb = 0;
            if (idx < raw) {
                if (c0) w = *reinterpret_cast<const uint32_t*>(src + idx);
                vb = (int)min(4u, raw - idx);
            }
            int cnt = vb;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (b < vb && ((w >> (8 * b)) & 0xFFu) == 0xFFu) cnt++;
            const uint32_t inc = gj_wave_incl_scan((uint32_t)cnt);
            uint32_t p = o + inc - (uint32_t)cnt;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (b < vb) {
                    const uint32_t byte = (w >> (8 * b)) & 0xFFu;
                    out[p++] = (uint8_t)byte;
                    if (byte == 0xFFu) out[p++] = 0;
                }
            }
            o += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        if (lane == 0) {
            if (!sg.last_in_scan) {
                out[o] = 0xFF;
                out[o + 1] = (uint8_t)(0xD0 + (sg.index_in_scan & 7));
            }
            if (s == g.segment_count - 1) {
                out[o] = 0xFF;
                out[o + 1] = 0xD9;
            }
        }
    }
}

// APP13 segment index (src/gpujpeg_writer.c:522-547): big-endian u32 start of every segment relative to
// the first one of its scan, plus the end position (after the dropped final RSTn).
#define GJ_MAX_HEADER_SIZE (65536 - 100)
__global__ __launch_bounds__(256) void k_segment_info(const gj_enc_job J)
{
    const gj_geom& g = J.g;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= g.segment_count || J.d_result[1]) return;
    const GjSeg sg = gj_segment(g, s);
    const int scan = g.interleaved ? 0 : sg.comp;
    const int first = g.interleaved ? 0 : g.comp[scan].first_segment;
    const int segs = g.interleaved ? g.segment_count : g.comp[scan].segment_count;
    const uint32_t data0 = J.d_seg_out[first];
    const uint32_t hdr_begin = data0 - (J.scan_hdr_offset[scan + 1] - J.scan_hdr_offset[scan]);
    for (int e = sg.index_in_scan; e <= (sg.last_in_scan ? segs : sg.index_in_scan); e++) {
        uint32_t pos;
        if (e < segs) pos = J.d_seg_out[first + e] - data0;
        else pos = J.d_seg_out[first + segs - 1] + J.d_seg_bytes[first + segs - 1] + J.d_seg_ff[first + segs - 1] - data0;
        // payload chunks of GJ_MAX_HEADER_SIZE bytes, each preceded by marker(2)+length(2)+scan(1)
        const uint32_t byte = (uint32_t)e * 4u;
        const uint32_t chunk = byte / GJ_MAX_HEADER_SIZE, within = byte % GJ_MAX_HEADER_SIZE;
        uint8_t* p = J.d_jpeg + hdr_begin + J.scan_info_payload[scan] + chunk * (GJ_MAX_HEADER_SIZE + 5u) + within;
        p[0] = (uint8_t)(pos >> 24); p[1] = (uint8_t)(pos >> 16); p[2] = (uint8_t)(pos >> 8); p[3] = (uint8_t)pos;
    }
}

