// gj_dec_entropy_prog.hip -- MI355X (gfx950, wave64) JPEG decoder: entropy decoding of PROGRESSIVE streams (SOF2, ITU T.81 Annex G) into the
// coefficient planes, one wave per restart segment of a scan.
// (part of the decoder's device code, see gj_dec_internal.h for the map of the files)
#include "gj_dec_internal.h"
#include "gj_bitreader.h"

// ================================================================================================
// k_huffman_decode_prog: ONE WAVE PER RECORD of the work list (gj_hip.h: gj_prog_rec -- a restart segment of one scan; nothing in here knows of
// frames). The scans of a progressive frame refine the same blocks again and again, so the planes are cleared once per frame and every scan
// stores only ITS coefficients, as 16-bit stores: the scans of one level (gj_prog_plan) run in the same launch and write other coefficients of
// the same 128-byte blocks.
//
// Huffman decoding inside a segment is serial. The wave does it in wave-uniform control flow -- every lane computes the same symbol from the
// same LDS words (broadcast reads) -- and spends its 64 lanes on what is parallel in a block: LANE k IS ZIG-ZAG POSITION k.
//   AC, first scan      a symbol's value lands in lane k = its position; at the end of the block the lanes of [Ss, Se] that got a value store it.
//                       An EOB run skips whole blocks without a store.
//   AC, refinement      the lanes load the block (one 128-byte line), __ballot(coefficient != 0) is the history mask. A symbol with run r passes
//                       the stretch up to the (r + 1)-th zero of the mask behind the cursor; every non-zero lane of the stretch takes ITS
//                       correction bit, number popcount(mask below it), from the stream: all at once. An EOB run corrects the rest of the band
//                       in one step per block. Lanes whose value changed store it. No lane waits for a load per coefficient.
//   DC, first scan      decoded serially; lane (ordinal & 63) keeps the block's value, 64 blocks are stored at a time.
//   DC, refinement      64 blocks per step: lane j takes bit j and ORs 1 << Al into its block's DC.
// The stream comes through an LDS stage of 1 KiB that the wave refills together (coalesced dwords, stuffed zeros dropped: gj_unstuff_round), so a
// segment may have any length -- a progressive scan without restart markers is ONE segment.
//
// On any byte sequence: positions are clamped to 63, an EOB run to the blocks that are left, bits behind the segment's end are zero, every loop is
// bounded by the segment's blocks (a symbol moves the position by one at least). A corrupt scan gives wrong coefficients, inside the planes.
// ================================================================================================
#define GJ_PROG_STAGE_BYTES 1024u
#define GJ_PROG_STAGE_DW (GJ_PROG_STAGE_BYTES / 4u + 4u) // + the zero padding behind the last byte
#define GJ_PROG_AHEAD 32u                               // blocks a refinement scan loads ahead of the one it decodes (see there)
#define GJ_PROG_NEED_BITS 128u                          // a symbol (16) + its extra bits (15) + the correction bits of a stretch (63), rounded up

// A value that is the same in every lane, said so: what is read from LDS is a vector value to the compiler, and everything computed from it -- the
// whole serial decode -- would run on the vector unit, four cycles an instruction for a lone wave, with branches on execution masks. Behind this it
// runs on the scalar unit. (The CPU execution model runs a lane at a time: there the value is taken as it is, no exchange between the lanes.)
__device__ __forceinline__ uint32_t gj_prog_uniform(const uint32_t v)
{
#ifdef GJ_HIPEMU
    return v;
#else
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#endif
}

// the wave's view of its segment: the same values in every lane
struct GjProgBits {
    const uint32_t* src;  // aligned source of the segment
    const uint32_t* end;  // behind the last dword of the stream buffer
    uint32_t ndw, c0;     // source dwords of the segment, the next one to take
    int lead;             // bytes in front of the segment inside its first dword
    uint32_t len;
    uint32_t carry;       // gj_unstuff_round
    uint32_t sbytes;      // bytes in the stage
    uint32_t bitpos;      // the cursor, bits from the start of the stage
    uint64_t acc;         // the n bits at the cursor, left aligned, in registers: a symbol costs one table look-up in LDS, not five round trips
    uint32_t n;           // (bitpos + n is a multiple of 32: the window grows by whole dwords of the stage)
};

// all 64 lanes call: drops what has been read, takes rounds of 64 source dwords while they fit
__device__ __forceinline__ void gj_prog_refill(GjProgBits& B, uint32_t* s_stage, const int lane)
{
    uint8_t* U8 = reinterpret_cast<uint8_t*>(s_stage);
    const uint32_t have = (B.sbytes + 3u) >> 2;
    const uint32_t keep = min(B.bitpos >> 5, have); // first dword that is still needed
    const uint32_t tail = have - keep;              // (a few dwords: the refill comes when fewer than GJ_PROG_NEED_BITS bits are left)
    uint32_t t = 0;
    gj_wave_sync();
    if ((uint32_t)lane < tail) t = s_stage[keep + (uint32_t)lane];
    gj_wave_sync();
    if ((uint32_t)lane < tail) s_stage[lane] = t;
    gj_wave_sync();
    B.bitpos -= keep * 32u;
    B.sbytes -= min(keep * 4u, B.sbytes);
    while (B.c0 < B.ndw && B.sbytes + 256u <= GJ_PROG_STAGE_BYTES) {
        const uint32_t idx = B.c0 + (uint32_t)lane;
        uint32_t w = 0;
        if (idx < B.ndw && B.src + idx < B.end) w = B.src[idx];
        B.sbytes += gj_unstuff_round(U8, B.sbytes, idx, B.lead, B.len, w, B.carry, lane);
        B.c0 += 64u;
    }
    for (uint32_t b = B.sbytes + (uint32_t)lane; b < ((B.sbytes + 3u) & ~3u) + 8u; b += 64u) U8[b ^ 3u] = 0;
    gj_wave_sync();
}

__device__ __forceinline__ uint32_t gj_prog_dword(const GjProgBits& B, const uint32_t* s_stage, const uint32_t dw)
{
    return dw < ((B.sbytes + 3u) >> 2) + 2u ? s_stage[dw] : 0u;
}

// the window again from the stage, after the cursor has moved by more than the window held
__device__ __forceinline__ void gj_prog_sync(GjProgBits& B, const uint32_t* s_stage)
{
    const uint32_t r = B.bitpos & 31u;
    B.acc = (uint64_t)gj_prog_uniform(gj_prog_dword(B, s_stage, B.bitpos >> 5)) << (32u + r);
    B.n = 32u - r;
}

// before a symbol: enough bits in the stage, or the source is used up (zero bits follow then). The window never holds bits the stage has not
// got yet: it reaches 64 bits ahead of the cursor at most, and GJ_PROG_NEED_BITS were there when it was filled.
__device__ __forceinline__ void gj_prog_need(GjProgBits& B, uint32_t* s_stage, const int lane)
{
    // (rounds of 256 source bytes: a round may bring fewer bytes than it needs; the loop ends with the source)
    while (B.c0 < B.ndw && B.bitpos + GJ_PROG_NEED_BITS > B.sbytes * 8u) gj_prog_refill(B, s_stage, lane);
    if (B.bitpos > B.sbytes * 8u + 64u) { // (behind the end: zeros, wherever the cursor is)
        B.bitpos = B.sbytes * 8u + 64u;
        gj_prog_sync(B, s_stage);
    }
}

// at least 32 bits in the window
__device__ __forceinline__ void gj_prog_fill(GjProgBits& B, const uint32_t* s_stage)
{
    if (B.n <= 32u) {
        B.acc |= (uint64_t)gj_prog_uniform(gj_prog_dword(B, s_stage, (B.bitpos + B.n) >> 5)) << (32u - B.n);
        B.n += 32u;
    }
}

// the cursor k < 64 bits on
__device__ __forceinline__ void gj_prog_skip(GjProgBits& B, const uint32_t* s_stage, const uint32_t k)
{
    B.bitpos += k;
    if (k >= B.n) {
        gj_prog_sync(B, s_stage);
    } else {
        B.acc <<= k;
        B.n -= k;
    }
}

__device__ __forceinline__ uint32_t gj_prog_bit(const GjProgBits& B, const uint32_t* s_stage, const uint32_t p)
{
    return (gj_prog_dword(B, s_stage, p >> 5) >> (31u - (p & 31u))) & 1u;
}

// n <= 16 bits at the cursor
__device__ __forceinline__ uint32_t gj_prog_get(GjProgBits& B, const uint32_t* s_stage, const uint32_t n)
{
    if (n == 0) return 0u;
    gj_prog_fill(B, s_stage);
    const uint32_t v = (uint32_t)(B.acc >> 32) >> (32u - n);
    gj_prog_skip(B, s_stage, n);
    return v;
}

// one Huffman symbol with table t (GJ_DEC_TAB_WORDS layout, in LDS)
__device__ __forceinline__ uint32_t gj_prog_symbol(GjProgBits& B, const uint32_t* s_stage, const uint16_t* t)
{
    gj_prog_fill(B, s_stage);
    const uint32_t hi = (uint32_t)(B.acc >> 32);
    uint32_t ent = gj_prog_uniform(t[hi >> (32 - GJ_DEC_FAST_BITS)]);
    if (ent == 0) ent = gj_prog_uniform(gj_decode_slow(hi, t));
    gj_prog_skip(B, s_stage, ent >> 8);
    return ent & 0xFFu;
}

// block number `o` of the segment in coding order: its index in the planes (64 coefficients per block) and the scan component it belongs to
__device__ __forceinline__ uint32_t gj_prog_block(const gj_prog_rec& R, const uint32_t per_mcu, const uint32_t o, int& ci)
{
    const uint32_t m = R.first + o / per_mcu;
    uint32_t p = o % per_mcu;
    ci = 0;
    while (ci + 1 < (int)R.ncomp && p >= (uint32_t)R.c[ci].h * R.c[ci].v) { p -= (uint32_t)R.c[ci].h * R.c[ci].v; ci++; }
    const gj_prog_comp& k = R.c[ci];
    const uint32_t my = m / R.across, mx = m - my * R.across;
    const uint32_t h = max((uint32_t)k.h, 1u);
    return k.base + (my * k.v + p / h) * k.pitch + mx * h + p % h;
}

__global__ __launch_bounds__(64) void k_huffman_decode_prog(const uint8_t* __restrict__ jpeg, const uint64_t jpeg_size, const gj_prog_rec* __restrict__ recs,
                                                            const uint32_t rec_count, const uint16_t* __restrict__ tabs, const uint32_t tab_count,
                                                            int16_t* __restrict__ coefs, const uint64_t coef_blocks)
{
    if (blockIdx.x >= rec_count) return;
#define GJ_PROG_TABLE(t) ((uint32_t)(t))
#include "gj_dec_entropy_prog_body.h"
#undef GJ_PROG_TABLE
}

// The same for the frames of a chunk (gj_prog_plan::d_frames): the record names its frame (gj_prog_rec::frame, clamped to the chunk), the frame's entry
// says where its stream lies behind the chunk's streams, where its tables begin in the pool and where its planes begin in the chunk's planes. Everything
// the wave reads or writes is clamped PER FRAME -- pos / len to the frame's own stream, block numbers to the frame's own coef_blocks blocks --, so that a
// corrupt scan gives wrong coefficients inside its own frame's planes and never in a neighbour's.
__global__ __launch_bounds__(64) void k_huffman_decode_prog_batch(const uint8_t* __restrict__ streams, const gj_prog_frame* __restrict__ frames, const uint32_t frame_count,
                                                                  const gj_prog_rec* __restrict__ recs, const uint32_t rec_count, const uint16_t* __restrict__ tabs,
                                                                  const uint32_t tab_count, int16_t* __restrict__ planes, const uint64_t coef_blocks)
{
    if (blockIdx.x >= rec_count || frame_count == 0u) return;
    const gj_prog_frame& F = frames[min((uint32_t)recs[blockIdx.x].frame, frame_count - 1u)];
    const uint8_t* __restrict__ jpeg = streams + F.stream;
    const uint64_t jpeg_size = F.size;
    int16_t* __restrict__ coefs = planes + F.coef_block * 64u;
    const uint32_t tab_first = F.tab_first;
#define GJ_PROG_TABLE(t) (tab_first + (uint32_t)(t))
#include "gj_dec_entropy_prog_body.h"
#undef GJ_PROG_TABLE
}

// the entropy stage of a progressive frame: the planes cleared, then one launch per level. A chunk of frames (gj_prog_plan::d_frames): ONE clear of the
// chunk's planes, then level l of all its frames in one launch -- as many launches as its deepest frame has levels
void gj_launch_huffman_prog(const gj_dec_job* job, hipStream_t st)
{
    const gj_prog_plan* P = job->prog;
    const gj_geom& g = job->g;
    if (P->d_frames != nullptr) {
        const uint32_t frames = job->batch.count > 1 ? job->batch.count : 1u;
        GJ_HIP_CHECK(hipMemsetAsync(job->d_coefs, 0, (size_t)frames * g.fb.coefs * sizeof(int16_t), st));
        for (int l = 0; l < P->levels && l < GJ_PROG_MAX_SCANS; l++) {
            if (P->level_count[l] == 0) continue;
            hipLaunchKernelGGL(k_huffman_decode_prog_batch, dim3(P->level_count[l]), dim3(64), 0, st, job->d_jpeg, P->d_frames, frames, P->d_recs + P->level_first[l],
                               P->level_count[l], P->d_tabs, P->tab_count, job->d_coefs, (uint64_t)(g.data_size / 64));
        }
        return;
    }
    GJ_HIP_CHECK(hipMemsetAsync(job->d_coefs, 0, g.data_size * sizeof(int16_t), st));
    for (int l = 0; l < P->levels && l < GJ_PROG_MAX_SCANS; l++) {
        if (P->level_count[l] == 0) continue;
        hipLaunchKernelGGL(k_huffman_decode_prog, dim3(P->level_count[l]), dim3(64), 0, st, job->d_jpeg, job->jpeg_size, P->d_recs + P->level_first[l],
                           P->level_count[l], P->d_tabs, P->tab_count, job->d_coefs, (uint64_t)(g.data_size / 64));
    }
}
