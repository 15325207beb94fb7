// gj_dec_internal.h -- what the files of the decoder's device code share.
//
//   gj_decode.hip               gj_hip_decode: picks the kernels of a frame and launches them
//   gj_dec_markers.hip          k_marker_scan, k_marker_segments: segment table built on the device, summary for the host in pinned memory
//                               k_gather_headers: the headers of a batch's streams to the host in one launch (dec_opt_batch_sizes = mixed)
//   gj_dec_entropy_tok.hip      k_huffman_decode_tok: sub-sequence parallel entropy decoding into 16-bit TOKENS + one record per block
//                               (the default for large non-interleaved frames)
//   gj_dec_entropy_par.hip      k_huffman_decode_par: sub-sequence parallel entropy decoding into the coefficient planes (segments of any length)
//   gj_dec_entropy_seq.hip      one lane per restart segment (interleaved scans with many short segments): k_huffman_decode_win over a ring the
//                               lane refills itself (token mode), k_huffman_decode_seq over an LDS stage (plane mode)
//   gj_dec_entropy_serial.hip   k_huffman_decode: one lane per restart segment, stream windows (Huffman tables that do not fit the two-level layout)
//   gj_dec_entropy_prog.hip     k_huffman_decode_prog: progressive streams (SOF2), one wave per restart segment of a scan, lane k = zig-zag position k;
//                               k_huffman_decode_prog_batch: the same over a chunk of frames (both are gj_dec_entropy_prog_body.h, included once each)
//   gj_dec_idct.hip             k_idct_fused_* (from the planes), k_idct_tok_* (from tokens; the full-size and the region kernel around one core:
//                               gj_tok_tables, gj_tok_idct3), k_idct / k_postprocess / k_copy_planes_out (generic); gj_launch_idct: the IDCT side of
//                               every kind of call and its one tail (debug stage, channel remap, gj_dec_job::idct_path)
//   gj_dec_idct_scaled.hip      reduced-size output (dec_opt_scale): k_idct_scaled (from the planes), k_idct_tok_scaled_rgb444 (from tokens)
//   gj_dec_region.hip           region decode (dec_opt_region): k_segment_select (table -> the entries that touch the region's cover), k_idct_region,
//                               k_postprocess_region / k_copy_planes_region (cover blocks -> cover planes -> the region's pixels),
//                               k_resize_region (crop-and-resize: the rectangle resampled to the call's output size instead of copied),
//                               k_idct_region_scaled (dec_opt_resize_prescale: the cover's blocks through the reduced-size IDCT ahead of it),
//                               k_idct_region_scaled_comp (dec_opt_resize_prescale_subsampled: the same on 4:2:0 streams, N per component),
//                               k_resize_region_aa (dec_opt_resize_filter = antialias: the resample with the triangle filter, tiled through LDS)
//   this header                 what those share: the 4:4:4 configuration and its colour pairs (gj_is_rgb444, GJ_COLOR_PAIRS), gj_block_of, the block
//                               records of the token-fed kernels (gj_rec_pack, gj_tok_record) and their token ranges (gj_tok_fetch), the N-point IDCT of a
//                               block's corner (gj_idct_corner)
//   gj_bitreader.h              unstuffing of a restart segment into an LDS stage, two-level table look-up
//
// Restates src/gpujpeg_huffman_gpu_decoder.cu:135-495 (entropy decoding semantics; identical results to
// src/gpujpeg_huffman_cpu_decoder.c:245-372), src/gpujpeg_dct_gpu.cu:312-366,472-618 and src/gpujpeg_postprocessor.cu:49-217.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "gj_device.h"
#include "gj_hip.h"

// developer aid (gj_tuning::debug_sync): waits after every launch and names the stage on stderr (which kernel faulted?)
static inline void gj_debug_stage(const bool on, hipStream_t st, const char* what)
{
    if (!on) return;
    const hipError_t e = hipStreamSynchronize(st);
    fprintf(stderr, "[GPUJPEG] [Debug] %s: %s\n", what, hipGetErrorString(e));
}

// ---- the marker scan's second launch when it was left to gj_hip_decode (gj_dec_job::scan)
void gj_launch_marker_table_deferred(const gj_dec_job* job, hipStream_t st);
// does gj_launch_huffman_tok derive its batches' table entries from the scan's records itself (no k_marker_table launch)?
bool gj_tok_folds_table(const gj_dec_job* job);
bool gj_par_folds_table(const gj_dec_job* job); // the same for gj_launch_huffman_par

// ---- entropy decoders: each launches its kernel for the whole segment table of the job
void gj_launch_huffman_serial(const gj_dec_job* job, hipStream_t st);
void gj_launch_huffman_par(const gj_dec_job* job, hipStream_t st);
void gj_launch_huffman_seq(const gj_dec_job* job, hipStream_t st, bool tokens);
void gj_launch_huffman_tok(const gj_dec_job* job, hipStream_t st);
// ... and the entropy stage of a progressive frame (gj_dec_job::prog): the planes cleared, one launch per level of its plan
void gj_launch_huffman_prog(const gj_dec_job* job, hipStream_t st);

// Batches of the sub-sequence decoders: consecutive table entries, cut per scan -- the luminance segments of a photograph carry two to
// three times the bytes of the chrominance ones, and a batch is sized to fill the LDS stage (one batch size for the whole stream
// gave luminance batches that had to be decoded as two groups, and chrominance batches that left half of the lanes idle).
struct GjBatchPlan {
    int n;                       // ranges (scans)
    int first[GJ_MAX_COMP];      // first table entry of range c
    int count[GJ_MAX_COMP];      // entries
    int g[GJ_MAX_COMP];          // segments per batch
    int batch0[GJ_MAX_COMP + 1]; // first batch of range c; [n] = number of batches
};
// cap_u: bytes of the kernel's LDS stage, max_blocks / gmax: blocks / segments a batch may have; resident (0: no preference): the workgroups
// of the kernel the GPU holds at once -- fuller batches are preferred when they keep the launch within one such generation
GjBatchPlan gj_plan_batches(const gj_dec_job* job, unsigned cap_u, unsigned max_blocks, unsigned gmax, unsigned resident);

// k_huffman_decode_tok (shared with the launcher's choice of the kernel)
#define GJ_TOK_CAP_U 10752     // bytes of unstuffed stream per group, incl. 8 B of zero padding per segment
#define GJ_TOK_MAX_BLOCKS 2304 // blocks per batch
#define GJ_TOK_RESIDENT ((unsigned)gj_hip_cu_count() * 4u)  // workgroups of the token decoder the GPU holds at once (MI355X: 256 CUs x 4)
#define GJ_TOK_GMAX 64         // segments per batch

// ---- what k_marker_scan leaves per scanning workgroup (gj_dec_markers.hip), read by k_marker_table and -- when the table launch is folded into it --
// by k_huffman_decode_tok
#define GJ_SCAN_LIST 2048    // restart markers a workgroup may hold (beyond that the host walks the stream)
#define GJ_SCAN_REC_WORDS 16 // 32-bit words of a record (layout: gj_dec_markers.hip)
struct GjOther { uint32_t pos, code, after, b03, b47; }; // a marker that is no restart marker: position, code, restart markers of its workgroup behind it, the 8 bytes behind the code
// other marker q (0, 1) of a record whose words 4 .. 15 are r1, r2, r3
__device__ __forceinline__ GjOther gj_rec_other(const uint4& r1, const uint4& r2, const uint4& r3, const uint32_t q)
{
    return q == 0 ? GjOther{r1.x, r1.y, r1.z, r1.w, r2.x} : GjOther{r2.z, r2.w, r3.x, r3.y, r3.z};
}
// the 16 bits behind the code: the length of the marker's segment (big-endian in the stream)
__device__ __forceinline__ uint32_t gj_other_len(const GjOther& o) { return ((o.b03 & 0xFFu) << 8) | ((o.b03 >> 8) & 0xFFu); }

// ---- The segment table without its launch (round 5). k_marker_table turns the scanning workgroups' records and marker lists into table entries --
// 11 us and a launch gap in front of every decoded frame, at every size -- and all a batch needs of that table is the positions of its own G + 1
// markers. On the speculative path (the same header as the previous frame: the only outcome the host accepts is a COMPLETE, REGULAR stream --
// every scan with all its segments, restart markers numbered in sequence, SOS headers between the scans, EOI) the structure is known from the
// geometry: restart marker number r of the stream ends segment r - (scans in front) ... so a workgroup reads the <= 256 records (one per lane, one
// trip), checks that every scan has exactly the restart markers it should have (prefix sums), finds the scanning workgroups that hold its
// markers (binary search in LDS) and reads them from their lists (second trip). Anything else -- a marker too many or too few, a number out of
// sequence, an unexpected marker code -- raises rst_irregular in the host's summary and the workgroup leaves: the host decodes the frame again
// the careful way, through k_marker_table (gj_decoder.c). Workgroup 0 also writes the summary the host validates (scan boundaries, SOS bytes, EOI).
struct GjFold {
    const uint32_t* recs;  // nullptr: the table has been written (seg_pos / seg_len / seg_index)
    const uint32_t* lists;
    uint32_t nwg, part_bytes;
    uint64_t begin;
    gj_scan_summary* hsum; // host memory
    uint32_t* h_maxlen;    // host memory: one word per batch
};


// LDS words gj_fold_batch needs for a kernel whose batches hold up to GMAX segments
#define GJ_FOLD_SCRATCH_WORDS(GMAX) (256 + GJ_SCAN_MAX_OTHER * 6 + 2 * ((GMAX) + 1) + 3)

// The table entries of ONE batch -- segments si0 .. si0 + nseg - 1 of the plan's range pc, nseg <= GMAX <= 255 -- from the scan's records: lane j < nseg
// gets its segment's geometric index, position and length (ld_s, ld_p, ld_l). All 256 threads call; `scratch` = GJ_FOLD_SCRATCH_WORDS(GMAX) words
// of LDS nobody else uses meanwhile, s_tmp = the 4 words of gj_wg256_incl_scan. Returns false (in every thread) when the stream is not the
// regular one the geometry describes: rst_irregular is raised in the host's summary and the workgroup must leave. Workgroup 0 writes the summary.
// (IL: the stream is ONE interleaved scan -- a template parameter: asked at run time it cost the 8K frame's token decoder 1.3 us, profiles/r5_13)
template <int GMAX, bool IL = false>
__device__ __forceinline__ bool gj_fold_batch(const GjFold& F, const gj_geom& g, const uint8_t* __restrict__ jpeg, const uint64_t jpeg_size, const GjBatchPlan& plan,
                                              const int pc, const int si0, const int nseg, uint32_t* const scratch, uint32_t* const s_tmp, uint32_t& ld_s,
                                              uint32_t& ld_p, uint32_t& ld_l)
{
    const int tid = threadIdx.x;
    uint32_t* const f_rinc = scratch;                         // [256] restart markers up to and including scanning workgroup t
    uint32_t* const f_o = f_rinc + 256;                       // [GJ_SCAN_MAX_OTHER][6] the other markers in stream order: position, code, restart markers in front, bytes 0..3, 4..7 behind the code, restart markers of its workgroup behind it
    uint32_t* const f_mpos = f_o + GJ_SCAN_MAX_OTHER * 6;     // [GMAX + 1] the batch's restart markers: entry j ends segment k0 - 1 + j of the scan
    uint32_t* const f_mnum = f_mpos + GMAX + 1;               // ... their numbers (RSTn & 7)
    uint32_t* const f_max = f_mnum + GMAX + 1;                // [0] longest segment of the batch, [1], [2] flags (a workgroup-wide "or" without __syncthreads_or, which takes LDS of its own)
    // scans of the stream: one per component in component order, or ONE interleaved scan that holds every segment (plan range 0)
    const int S = IL ? 1 : g.comp_count;
    auto segs_of = [&](const int c) { return IL ? (uint32_t)g.segment_count : (uint32_t)g.comp[c].segment_count; };
    const uint32_t base0 = (uint32_t)(((reinterpret_cast<uintptr_t>(jpeg) + F.begin) & ~(uintptr_t)15) - reinterpret_cast<uintptr_t>(jpeg)); // where the scanning workgroups' parts begin
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0, r2 = r0, r3 = r0;
    if ((uint32_t)tid < F.nwg) {
        const uint4* r4 = reinterpret_cast<const uint4*>(F.recs + (size_t)tid * GJ_SCAN_REC_WORDS);
        r0 = r4[0]; r1 = r4[1]; r2 = r4[2]; r3 = r4[3];
    }
    const uint32_t n = r0.x, no = min(r0.z, 2u);
    const bool bad = r0.w != 0 || n > (uint32_t)GJ_SCAN_LIST || r0.z > 2u;
    if (tid < 3) f_max[tid] = 0; // (visible behind the barriers of the prefix sum)
    uint32_t tot;
    // (two sums in one scan: restart markers in the low 22 bits -- 256 workgroups x GJ_SCAN_LIST = 2^19 at most --, other markers above them: up to 2 per
    // workgroup = 512, which an 8-bit field let wrap around to a small count on a malformed stream)
    const uint32_t inc = gj_wg256_incl_scan((n & 0x3FFFFFu) | (no << 22), s_tmp, &tot);
    const uint32_t rinc = inc & 0x3FFFFFu, oinc = inc >> 22;
    f_rinc[tid] = rinc;
    for (uint32_t q = 0; q < no; q++) {
        const uint32_t slot = oinc - no + q;
        if (slot < (uint32_t)GJ_SCAN_MAX_OTHER) {
            const GjOther o = gj_rec_other(r1, r2, r3, q);
            uint32_t* const fo = f_o + slot * 6;
            fo[0] = o.pos; fo[1] = o.code & 0xFFu; fo[2] = rinc - o.after; fo[3] = o.b03; fo[4] = o.b47; fo[5] = o.after;
        }
    }
    if (bad) f_max[1] = 1;
    __syncthreads(); // (the scratch is written)
    const bool bad_any = f_max[1] != 0;
    const uint32_t total_rst = tot & 0x3FFFFFu, total_other = tot >> 22;
    // is this the stream the geometry describes? scan c: segs_c - 1 restart markers, then the SOS of scan c + 1 (EOI behind the last one)
    bool regular = !bad_any && total_other == (uint32_t)S && plan.n == S;
    uint32_t exp_rst = 0, sstart = (uint32_t)F.begin, my_start = 0, my_end = 0, my_first = 0;
    for (int c = 0; c < S && regular; c++) {
        const uint32_t* const fo = f_o + c * 6;
        const uint32_t first_rank = exp_rst;
        exp_rst += segs_of(c) - 1u;
        regular = fo[1] == (c == S - 1 ? 0xD9u : 0xDAu) && fo[2] == exp_rst && fo[0] >= sstart && (uint64_t)fo[0] + 2u <= jpeg_size;
        if (c == pc) { my_start = sstart; my_end = fo[0]; my_first = first_rank; }
        sstart = fo[0] + 2u + (((fo[3] & 0xFFu) << 8) | ((fo[3] >> 8) & 0xFFu)); // behind the SOS header
    }
    regular = regular && total_rst == exp_rst;
    const uint32_t segs_pc = segs_of(pc);
    const int k0 = si0 - plan.first[pc]; // the batch's first segment inside its scan
    bool irregular = false;
    if (regular && tid <= nseg) { // the restart marker that ends segment k0 - 1 + tid of the scan
        const int kk = k0 - 1 + tid;
        uint32_t pos = 0, num = 0xFFu;
        if (kk >= 0 && (uint32_t)kk + 1u < segs_pc) {
            const uint32_t q = my_first + (uint32_t)kk; // its rank among the stream's restart markers (< total_rst)
            int lo = 0, hi = (int)F.nwg - 1;            // the first scanning workgroup with more than q markers up to and including its own
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (f_rinc[mid] > q) hi = mid; else lo = mid + 1;
            }
            const uint32_t idx = q - (lo ? f_rinc[lo - 1] : 0u);
            if (idx < (uint32_t)GJ_SCAN_LIST) {
                const uint32_t ent = F.lists[(size_t)lo * GJ_SCAN_LIST + idx];
                pos = base0 + (uint32_t)lo * F.part_bytes + (ent & 0xFFFFFFu);
                num = ent >> 24;
            } else {
                irregular = true;
            }
        }
        f_mpos[tid] = pos;
        f_mnum[tid] = num;
    }
    __syncthreads();
    if (regular && tid < nseg) {
        const uint32_t k = (uint32_t)(k0 + tid);
        const bool last = k + 1u == segs_pc;
        const uint32_t from = k == 0 ? my_start : f_mpos[tid] + 2u, to = last ? my_end : f_mpos[tid + 1];
        if (!last && f_mnum[tid + 1] != (k & 7u)) irregular = true; // RSTn out of sequence: the reference reader treats it specially, the host walk reproduces that
        if (last && to <= from && segs_pc > 1u) irregular = true;   // an empty segment in front of the end of a scan
        if (to > jpeg_size) irregular = true;
        ld_s = (IL ? 0u : (uint32_t)g.comp[pc].first_segment) + k;
        ld_p = from;
        ld_l = to > from ? to - from : 0u;
        atomicMax(f_max, ld_l);
    }
    if (!regular || irregular) f_max[2] = 1;
    __syncthreads();
    const bool give_up = f_max[2] != 0;
    if (blockIdx.x == 0) { // what the host validates (the table kernel's summary, gj_dec_markers.hip)
        gj_scan_summary* const hs = F.hsum;
        if (tid < (int)min(total_other, (uint32_t)GJ_SCAN_MAX_OTHER)) {
            const uint32_t* const fo = f_o + tid * 6;
            hs->other_pos[tid] = fo[0];
            hs->other_code[tid] = (uint8_t)fo[1];
            const uint32_t ob[4] = {fo[3], fo[4], 0, 0};
            for (int q = 0; q < 4; q++) reinterpret_cast<uint32_t*>(hs->other_bytes[tid])[q] = ob[q];
            hs->other_after[tid] = fo[5];
        }
        if (tid == 0) {
            hs->rst_count = total_rst;
            hs->other_count = total_other;
            hs->scan_count = regular ? (uint32_t)S : 0u;
            hs->status = regular ? 1u : 2u;
            hs->segment_count = regular ? total_rst + (uint32_t)S : 0u;
        }
        if (regular && tid < S) { // scan boundaries: behind the SOS header in front (scan 0: the start of the data) .. the marker that ends it
            uint32_t st = (uint32_t)F.begin;
            if (tid > 0) {
                const uint32_t* const fp = f_o + (tid - 1) * 6;
                st = fp[0] + 2u + (((fp[3] & 0xFFu) << 8) | ((fp[3] >> 8) & 0xFFu));
            }
            hs->scan_start[tid] = st;
            hs->scan_end[tid] = f_o[tid * 6];
        }
    }
    if (tid == 0) {
        F.h_maxlen[blockIdx.x] = give_up ? 0u : *f_max;
        if (give_up) F.hsum->rst_irregular = 1u;
    }
    __syncthreads(); // (the scratch may be reused)
    return !give_up;
}

// ---- IDCT side
// Three components, 4:4:4, packed 3-byte pixels: the configuration of every k_idct_*_rgb444 kernel
static inline bool gj_is_rgb444(const gj_geom& g)
{
    if (g.pixel_format != GJ_PF_444_P012 || g.comp_count != 3) return false;
    for (int c = 0; c < 3; c++)
        if (g.comp[c].samp_h != 1 || g.comp[c].samp_v != 1) return false;
    return true;
}
// ... and the (color_space_internal, color_space) pairs those kernels are instantiated for, the first one for "no transform". A launcher makes its
// array of instantiations from this list and takes entry gj_color_pair(g), the geometry's place in it (-1: not in the list).
#define GJ_COLOR_PAIRS(X) \
    X(GJ_CS_NONE, GJ_CS_NONE) X(GJ_CS_BT601_256, GJ_CS_RGB) X(GJ_CS_BT601, GJ_CS_RGB) X(GJ_CS_BT709, GJ_CS_RGB) X(GJ_CS_RGB, GJ_CS_BT601_256)
static inline int gj_color_pair(const gj_geom& g)
{
    const int from = g.color_space_internal, to = g.color_space;
    if (from == to || from == GJ_CS_NONE || to == GJ_CS_NONE) return 0;
    int i = 0;
#define GJ_X(F, T) \
    if (from == F && to == T) return i; \
    i++;
    GJ_COLOR_PAIRS(GJ_X)
#undef GJ_X
    return -1;
}

// block gb of a geometry's planes (blocks of component 0 in raster order, then component 1's ...): its component, and its place in that component's grid
__device__ __forceinline__ int gj_block_of(const gj_geom& g, const unsigned gb, unsigned& bx, unsigned& by)
{
    int c = 0;
#pragma unroll
    for (int i = 1; i < GJ_MAX_COMP; i++)
        if (i < g.comp_count && (uint64_t)gb * 64 >= g.comp[i].data_offset) c = i;
    const gj_comp_geom& k = g.comp[c];
    const unsigned lb = gb - (unsigned)(k.data_offset / 64);
    by = lb / (unsigned)k.blocks_x;
    bx = lb - by * (unsigned)k.blocks_x;
    return c;
}

typedef void (*gj_idct_tok_t)(const gj_geom, const int16_t*, const uint2*, const uint16_t*, uint32_t, const float*, uint8_t*, int /* gj_tuning::idct_dense */);
gj_idct_tok_t gj_idct_tok_for(const gj_geom& g); // the token-fed IDCT kernel for this configuration, or nullptr
bool gj_is_uyvy422(const gj_geom& g);
// dequantisation + IDCT + postprocessing of the frame, whichever kind of call it is (full size, reduced size, region); channel remap; the one place
// that reports gj_dec_job::idct_path. ev (may be null): events 2 and 3 of gj_hip_decode
void gj_launch_idct(const gj_dec_job* job, hipStream_t st, gj_idct_tok_t idct_tok, gj_event_t* ev);
// reduced-size decode (gj_dec_idct_scaled.hip): is there a token-fed kernel for this configuration; the IDCT side of the frame -- true: the pixels
// are in d_raw, false: the reduced component planes are in d_planes and the pixel kernels follow with job->gs
bool gj_idct_tok_scaled_for(const gj_geom& g);
bool gj_launch_idct_scaled(const gj_dec_job* job, hipStream_t st, bool tokens);

// the generic pixel kernels' second half (k_postprocess, k_postprocess_region): the samples v of pixel (x, y) = number `pos` of a W x H image ->
// colour transform -> the stores of the pixel format (src/gpujpeg_postprocessor.cu:193-217, src/gpujpeg_preprocessor_common.cuh:118-203)
// (in two halves: k_resize_region blends the transformed values of four source pixels before the stores)
__device__ __forceinline__ void gj_pixel_transform(const gj_geom& g, int (&v)[4])
{
    if (g.comp_count == 1) { // single channel expanded for the colour transform (:127-170)
        if (g.color_space_internal == GJ_CS_RGB) v[1] = v[2] = v[0];
        else v[1] = v[2] = 128;
    }
    gj_color_transform(g.color_space_internal, g.color_space, v[0], v[1], v[2]);
}

__device__ __forceinline__ void gj_pixel_store(const gj_geom& g, uint8_t* __restrict__ raw, const unsigned W, const unsigned H, const unsigned x,
                                               const unsigned y, const unsigned pos, const int (&v)[4])
{
    switch (g.pixel_format) {
    case GJ_PF_U8: raw[(size_t)pos + (size_t)g.width_padding * y] = (uint8_t)v[0]; break;
    case GJ_PF_444_P012: {
        uint8_t* p = raw + (size_t)pos * 3 + (size_t)g.width_padding * y;
        p[0] = (uint8_t)v[0]; p[1] = (uint8_t)v[1]; p[2] = (uint8_t)v[2];
        break; }
    case GJ_PF_4444_P0123: {
        uint8_t* p = raw + (size_t)pos * 4 + (size_t)g.width_padding * y;
        p[0] = (uint8_t)v[0]; p[1] = (uint8_t)v[1]; p[2] = (uint8_t)v[2]; p[3] = (uint8_t)v[3];
        break; }
    case GJ_PF_444_P0P1P2:
        raw[pos] = (uint8_t)v[0]; raw[(size_t)W * H + pos] = (uint8_t)v[1]; raw[(size_t)2 * W * H + pos] = (uint8_t)v[2];
        break;
    case GJ_PF_422_P0P1P2:
        raw[pos] = (uint8_t)v[0];
        if ((x & 1) == 0) { // chroma by row, the layout of raw_size and k_copy_planes_out (the reference's pos / 2 makes rows of odd W share a byte: DESIGN 1)
            const size_t cpos = (size_t)y * ((W + 1) / 2) + x / 2;
            raw[(size_t)W * H + cpos] = (uint8_t)v[1];
            raw[(size_t)W * H + (size_t)H * ((W + 1) / 2) + cpos] = (uint8_t)v[2];
        }
        break;
    case GJ_PF_422_P1020: {
        const size_t off = (size_t)pos * 2 + (size_t)g.width_padding * y;
        raw[off + 1] = (uint8_t)v[0];
        raw[off] = (uint8_t)((x & 1) == 0 ? v[1] : v[2]);
        break; }
    case GJ_PF_420_P0P1P2:
        raw[pos] = (uint8_t)v[0];
        if ((pos & 1) == 0 && (y & 1) == 0) {
            raw[(size_t)W * H + (size_t)(y / 2) * ((W + 1) / 2) + x / 2] = (uint8_t)v[1];
            raw[(size_t)W * H + (size_t)((H + 1) / 2 + y / 2) * ((W + 1) / 2) + x / 2] = (uint8_t)v[2];
        }
        break;
    default: break;
    }
}

__device__ __forceinline__ void gj_store_pixel(const gj_geom& g, uint8_t* __restrict__ raw, const unsigned W, const unsigned H, const unsigned x,
                                               const unsigned y, const unsigned pos, int (&v)[4])
{
    gj_pixel_transform(g, v);
    gj_pixel_store(g, raw, W, H, x, y, pos, v);
}

// ---- reduced-size IDCT (the definition: gj_dec_idct_scaled.hip), shared by k_idct_scaled, k_idct_tok_scaled_rgb444 and k_idct_region_scaled
// M_N[x][u]
template <int N>
__device__ __forceinline__ constexpr int gj_mn(const int x, const int u)
{
    constexpr int M4[4][4] = {{2896, 3784, 2896, 1567}, {2896, 1567, -2896, -3784}, {2896, -1567, -2896, 3784}, {2896, -3784, 2896, -1567}};
    return N == 1 ? 2896 : N == 2 ? ((x & u) ? -2896 : 2896) : M4[x & 3][u & 3];
}

__device__ __forceinline__ int gj_dequant_clamp(const int f, const int q) { return min(max(f * q, -32768), 32767); }

// D[v * N + u] (dequantised, clamped) -> row y of the block's N x N samples in byte x of out[y]
template <int N>
__device__ __forceinline__ void gj_idct_corner(const int (&D)[N * N], uint32_t (&out)[N])
{
    int T[N * N];
#pragma unroll
    for (int y = 0; y < N; y++)
#pragma unroll
        for (int u = 0; u < N; u++) {
            int s = 1024;
#pragma unroll
            for (int v = 0; v < N; v++) s += gj_mn<N>(y, v) * D[v * N + u];
            T[y * N + u] = s >> 11;
        }
#pragma unroll
    for (int y = 0; y < N; y++) {
        uint32_t row = 0;
#pragma unroll
        for (int x = 0; x < N; x++) {
            int s = 16384;
#pragma unroll
            for (int u = 0; u < N; u++) s += gj_mn<N>(x, u) * T[y * N + u];
            row |= (uint32_t)min(max((s >> 15) + 128, 0), 255) << (8 * x);
        }
        out[y] = row;
    }
}

// the N x N corner of a block of the coefficient planes (rows of 8 int16)
template <int N>
__device__ __forceinline__ void gj_corner_from_plane(const int16_t* __restrict__ blk, int (&F)[N * N])
{
    if constexpr (N == 4) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint2 w = *reinterpret_cast<const uint2*>(blk + v * 8);
            F[v * 4 + 0] = (int16_t)w.x; F[v * 4 + 1] = (int32_t)w.x >> 16;
            F[v * 4 + 2] = (int16_t)w.y; F[v * 4 + 3] = (int32_t)w.y >> 16;
        }
    } else if constexpr (N == 2) {
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(blk + v * 8);
            F[v * 2 + 0] = (int16_t)w; F[v * 2 + 1] = (int32_t)w >> 16;
        }
    } else {
        F[0] = blk[0];
    }
}

// region decode (gj_dec_region.hip): the compacted segment table of job->region (from job's table, which has been written), and the IDCT side
// up to the region's pixels (gj_launch_idct goes on from there)
void gj_launch_segment_select(const gj_dec_job* job, hipStream_t st);
void gj_launch_segment_select_batch(const gj_dec_job* job, hipStream_t st); // (a batch of regions: every frame's table against its own cover)
void gj_launch_idct_region(const gj_dec_job* job, hipStream_t st, bool tokens, gj_event_t* ev);
void gj_launch_idct_tok_region(const gj_dec_job* job, hipStream_t st); // (gj_dec_idct.hip: beside k_idct_tok_rgb444, whose LDS helpers it shares)

// ---- token-fed IDCT kernels (gj_dec_idct.hip, gj_dec_idct_scaled.hip): the wave's tokens on their way into LDS
#define GJ_TOK_STAGE 832 // tokens per wave in LDS (with the 32 KiB tile: four workgroups per CU)

// the wave's token range of one component: dense and small enough for the stage (the normal case), with the two 16-byte
// loads per lane that fetch it
struct GjTokRange {
    uint32_t S, E;
    bool fast;
    uint4 t0, t1;
};

__device__ __forceinline__ GjTokRange gj_tok_fetch(const uint16_t* __restrict__ d_tok, const uint32_t start, const uint32_t cnt, const int lane)
{
    GjTokRange r;
    const uint32_t end = start + cnt;
    const uint32_t prev_end = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)end, 0x138, 0xF, 0xF, false); // wave_shr:1
    const unsigned long long breaks = __ballot(lane != 0 && start != prev_end);
    r.S = (uint32_t)__builtin_amdgcn_readlane((int)start, 0) & ~7u; // (16-byte pieces of 8 tokens)
    r.E = (uint32_t)__builtin_amdgcn_readlane((int)end, 63);
    r.fast = breaks == 0 && r.E - r.S <= GJ_TOK_STAGE;
    r.t0 = r.t1 = make_uint4(0, 0, 0, 0);
    if (r.fast) {
        const uint32_t i0 = (uint32_t)lane * 8u, i1 = i0 + 512u;
        if (r.S + i0 < r.E) r.t0 = *reinterpret_cast<const uint4*>(d_tok + r.S + i0);
        if (i1 < GJ_TOK_STAGE && r.S + i1 < r.E) r.t1 = *reinterpret_cast<const uint4*>(d_tok + r.S + i1);
    }
    return r;
}

// A block's record as the token-fed kernels keep it: start = first token, cd = count << 16 | DC term, bit 31: "the block is in the coefficient
// planes" (count 0xFFFF in the record) -- packed until the block is worked on (k_idct_tok_rgb444 has no register to spare, profiles/r5_11);
// gj_rec_count takes the count out. The guards are for damaged streams: a record nobody wrote, a range that leaves the token array -- count 0.
__device__ __forceinline__ uint32_t gj_rec_count(const uint32_t cd) { return (cd >> 16) & 0x7FFFu; }

// a record as the array holds it -> its cd word: the ONE place with the guards
__device__ __forceinline__ uint32_t gj_rec_pack(const uint2 r, const uint32_t tok_cap)
{
    uint32_t n = r.y >> 16;
    const bool planes = n == 0xFFFFu;
    if (planes || n > 63u || r.x > tok_cap || n > tok_cap - r.x) n = 0;
    return (r.y & 0xFFFFu) | (n << 16) | (planes ? 0x80000000u : 0u);
}

// Component c's record of block position lb (4:4:4, non-interleaved scans: plane order == coding order); a lane without a block gets an empty range.
// One call per component from the kernel's own unrolled loop: a helper that loads all three lets the compiler put the loads into one branch, which
// costs k_idct_tok_scaled_rgb444<1> four registers.
__device__ __forceinline__ void gj_tok_record(const gj_geom& g, const uint2* d_rec, const uint32_t tok_cap, const bool has_block, const unsigned lb,
                                              const int c, uint32_t& start, uint32_t& cd)
{
    start = cd = 0;
    if (has_block) {
        const uint2 r = d_rec[g.comp[c].data_offset / 64 + lb];
        start = r.x;
        cd = gj_rec_pack(r, tok_cap);
    }
}
