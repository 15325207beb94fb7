// gj_dec_region.hip -- MI355X (gfx950, wave64) JPEG decoder: region-of-interest decode (dec_opt_region = X,Y,W,H). The result is the crop of
// the full decode, byte for byte; what a region call saves is work:
//
//   k_segment_select        segment table -> compacted table of the entries whose restart segment touches the region's cover
//                           (gj_segment_in_cover, gj_device.h), in stream order, and their number per scan in pinned host memory. Every entropy
//                           decoder reads the table, so every one of them decodes the selection without a change to its symbol loop.
//   k_idct_region           dequantisation + IDCT of the cover's blocks from the coefficient planes into COVER-SIZED component planes
//                           (one lane per block like k_idct, the same arithmetic: gj_idct_pk)
//   k_postprocess_region    the region's pixels from those planes: k_postprocess with the region's origin inside the cover
//   k_copy_planes_region    the same for planar output whose layout equals the component layout (k_copy_planes_out)
//   k_resize_region         crop-and-resize (gpujpeg_amd_decoder_decode_batch_crop_resize): in place of the two above, the rectangle resampled
//                           bilinearly to the call's output size, with an optional horizontal mirror
//   k_resize_region_tensor  the same pixels stored as a normalised float tensor (gpujpeg_amd_decoder_decode_batch_crop_resize_tensor: f32 / f16 / bf16,
//                           CHW / HWC, element = byte * scale[c] + bias[c]) -- k_resize_region up to and including the blend, another store
//   k_resize_region_aa      both of them with the antialiased triangle filter in place of the four-tap blend (dec_opt_resize_filter = antialias:
//   (.._aa_tensor)          gj_resize_aa_taps, exact rational weights over a footprint that grows with the reduction, one rounding)
//   k_idct_region_scaled    in front of k_resize_region for the frames dec_opt_resize_prescale reduces (gj_region_frame::scale = s > 1): the
//                           cover's blocks through the N-point IDCT of their N x N corner, N = 8 / s (k_idct_scaled's arithmetic: gj_idct_corner),
//                           into REDUCED cover planes
//   k_idct_region_scaled_comp  the same for the frames dec_opt_resize_prescale_subsampled reduces PER COMPONENT (gj_region_frame::per_comp: 4:2:0):
//                           component c's blocks through N_c = 8 sub_h / s -- N_c = 8 is k_idct_region's transform --, one sample per reduced pixel in every plane
//
// Every configuration can go this way; three-component 4:4:4 streams with non-interleaved scans and packed 3-byte output in token mode go
// through k_idct_tok_region_rgb444 (gj_dec_idct.hip, beside k_idct_tok_rgb444 whose LDS helpers it shares) instead of the last three: same bytes.
//
// A BATCH of regions (gj_region::d_frames: one rectangle per frame, gpujpeg_amd_decoder_decode_batch_regions) runs the same code with blockIdx.z =
// frame: k_segment_select_batch, k_idct_region_batch, k_postprocess_region_batch, k_copy_planes_region_batch, k_resize_region_batch, k_resize_region_tensor_batch, k_idct_region_scaled_batch, k_idct_region_scaled_comp_batch and the batched instantiation of
// k_idct_tok_region_rgb444 read their frame's rectangle and cover from device memory and share the bodies of the single-frame kernels.
// (part of the decoder's device code, see gj_dec_internal.h for the map of the files)
#include "gj_dec_internal.h"

extern "C" int gj_hip_segment_in_cover(const gj_geom* g, const gj_region* r, int s) { return gj_segment_in_cover(*g, r->frame, s) ? 1 : 0; }
extern "C" uint32_t gj_hip_tensor_element(const gj_tensor* t, int c, int v) { return gj_tensor_element(*t, c, v); }
extern "C" int gj_hip_resize_aa_weights(int n_src, int n_out, int i, int* first, int* count, uint32_t* weights, int capacity, uint64_t* sum)
{
    if (n_src < 1 || n_out < 1 || n_src > 65535 || n_out > GJ_RESIZE_MAX_OUT || i < 0 || i >= n_out || n_src > GJ_RESIZE_AA_MAX_RATIO * n_out) return -1;
    int k0, n;
    uint32_t U;
    gj_resize_aa_taps(n_src, n_out, i, k0, n, U);
    if (first) *first = k0;
    if (count) *count = n;
    if (sum) *sum = U;
    if (weights) {
        if (capacity < n) return -2;
        for (int k = 0; k < n; k++) weights[k] = gj_resize_aa_weight(n_src, n_out, i, k0 + k);
    }
    return 0;
}

// ================================================================================================
// Selection
// ================================================================================================
#define GJ_SEL_CHUNK 1024 // table entries per workgroup = its lanes

// scan of the stream a geometric segment index belongs to (0 for an interleaved scan)
__device__ __forceinline__ int gj_segment_scan(const gj_geom& g, const uint32_t s)
{
    int c = 0;
    if (!g.interleaved)
        for (int i = 1; i < GJ_MAX_COMP; i++)
            if (i < g.comp_count && (int)s >= g.comp[i].first_segment) c = i;
    return c;
}

// One launch, no ordering between workgroups: workgroup w takes entries [w * 1024, (w + 1) * 1024) of the table, one per lane, and finds where its
// selected entries go by counting the selected ones in front of its chunk itself -- reads of 4-byte indices that stay in L2 and a predicate of two
// 32-bit divisions each; the table of an 8K frame has 43 200 entries, the last workgroup evaluates all of them, 43 trips of its 1024 lanes. Counting is a ballot
// per wave and trip (every lane of a wave holds the wave's count), the order of the table (stream order) is kept: the batch plan's and the token
// decoder's arguments need batches in increasing stream position.
// The last workgroup has counted everything: it leaves the totals, per scan too, for the entropy decoders (device word) and for the host (pinned).
__global__ __launch_bounds__(GJ_SEL_CHUNK) void k_segment_select(const gj_geom g, const gj_region r, const uint32_t* __restrict__ seg_pos,
                                                                 const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ seg_index,
                                                                 const int seg_count_max, const uint32_t* __restrict__ seg_count_ptr,
                                                                 uint32_t* __restrict__ out, const uint32_t out_stride, uint32_t* __restrict__ d_count,
                                                                 uint32_t* __restrict__ h_count)
{
    __shared__ uint32_t s_before, s_scan[GJ_MAX_COMP], s_wave[GJ_SEL_CHUNK / GJ_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = seg_count_ptr ? min((int)*seg_count_ptr, seg_count_max) : seg_count_max;
    const int begin = (int)blockIdx.x * GJ_SEL_CHUNK;
    const bool last_wg = blockIdx.x == gridDim.x - 1;
    if (begin >= n && !last_wg) return;
    if (tid == 0) s_before = 0;
    if (tid < GJ_MAX_COMP) s_scan[tid] = 0;
    __syncthreads();
    // selected entries in front of the chunk (the last workgroup: per scan as well); every lane makes every trip
    uint32_t before = 0, per[GJ_MAX_COMP] = {0, 0, 0, 0};
    const int front = min(begin, n);
    for (int base = 0; base < front; base += GJ_SEL_CHUNK) {
        const int i = base + tid;
        const uint32_t s = i < front ? seg_index[i] : 0xFFFFFFFFu;
        const bool in = i < front && gj_segment_in_cover(g, r.frame, (int)s);
        before += (uint32_t)__popcll(__ballot(in));
        if (last_wg) {
            const int sc = in ? gj_segment_scan(g, s) : -1;
#pragma unroll
            for (int c = 0; c < GJ_MAX_COMP; c++) per[c] += (uint32_t)__popcll(__ballot(sc == c));
        }
    }
    // the chunk
    const int i = begin + tid;
    const uint32_t s = i < n ? seg_index[i] : 0xFFFFFFFFu;
    const bool in = i < n && gj_segment_in_cover(g, r.frame, (int)s);
    const unsigned long long b = __ballot(in);
    if (last_wg) {
        const int sc = in ? gj_segment_scan(g, s) : -1;
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++) per[c] += (uint32_t)__popcll(__ballot(sc == c));
    }
    if (lane == 0) {
        s_wave[wave] = (uint32_t)__popcll(b);
        if (before) atomicAdd(&s_before, before);
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++)
            if (last_wg && per[c]) atomicAdd(&s_scan[c], per[c]);
    }
    __syncthreads();
    uint32_t at = s_before, total = s_before;
    for (int w = 0; w < GJ_SEL_CHUNK / GJ_WAVE; w++) {
        if (w < wave) at += s_wave[w];
        total += s_wave[w];
    }
    at += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (in && at < out_stride) { // (cannot fail: the compacted table has room for every entry of the table)
        out[at] = seg_pos[i];
        out[out_stride + at] = seg_len[i];
        out[2 * out_stride + at] = s;
    }
    if (last_wg) {
        if (tid == 0) {
            *d_count = total;
            h_count[0] = total;
        }
        if (tid < GJ_MAX_COMP) h_count[1 + tid] = s_scan[tid];
    }
}

// the table of this job behind the selection: what the entropy decoders are launched with (gj_hip_decode)
void gj_launch_segment_select(const gj_dec_job* job, hipStream_t st)
{
    const gj_geom& g = job->g;
    const gj_region& r = job->region;
    const uint32_t stride = (uint32_t)g.segment_count + GJ_MAX_COMP;
    const unsigned wgs = ((unsigned)max(job->seg_count, 1) + GJ_SEL_CHUNK - 1) / GJ_SEL_CHUNK;
    hipLaunchKernelGGL(k_segment_select, dim3(wgs), dim3(GJ_SEL_CHUNK), 0, st, g, r, job->d_seg_pos, job->d_seg_len, job->d_seg_index, job->seg_count,
                       job->d_seg_count, r.d_sel, stride, r.d_sel_count, r.h_sel_count);
}

// The selection of a batch of regions: frame blockIdx.z's table (at gj_frame_strides::seg words, entries counted by its marker scan) against ITS
// cover. All frames are decoded behind ONE batch plan, which the host makes for the largest selection of every scan among them (r.sel_count): the
// entries of scan c go to the fixed offset sum(sel_count[0 .. c)) of the frame's compacted table in stream order, and what the frame's own
// selection leaves of the range is filled with null entries -- index 0xFFFFFFFF, length 0: a segment without blocks for both batchable entropy
// decoders. One workgroup per frame walks the table in trips of its 1024 lanes and keeps the running count per scan (a ballot per scan and wave,
// the waves' counts through LDS); what it found per scan goes to pinned host memory, where the host compares it with the frame's plan.
// (MIXED: frames of different image sizes, gj_frame_geom -- the predicate, the scans and the bound of the table are the frame's own)
template <bool MIXED>
__global__ __launch_bounds__(GJ_SEL_CHUNK) void k_segment_select_batch(const gj_geom g_launch, const gj_region rb, const uint32_t* __restrict__ seg_pos,
                                                                       const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ seg_index,
                                                                       const int seg_count_max, const uint32_t* __restrict__ seg_count_ptr,
                                                                       uint32_t* __restrict__ out, const uint32_t out_stride, uint32_t* __restrict__ h_found,
                                                                       uint32_t* __restrict__ h_bytes /* may be null: gj_region::h_sel_bytes */)
{
    __shared__ uint32_t s_wave[GJ_MAX_COMP][GJ_SEL_CHUNK / GJ_WAVE];
    const size_t z = blockIdx.z;
    const gj_geom& g = gj_frame_geom<MIXED>(g_launch);
    seg_pos += z * g_launch.fb.seg; seg_len += z * g_launch.fb.seg; seg_index += z * g_launch.fb.seg;
    out += z * g_launch.fb.seg;
    h_found += z * GJ_MAX_COMP;
    const gj_region_frame& r = rb.d_frames[z]; // (read where it lies: a copy indexed by component would live in scratch memory)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min((int)seg_count_ptr[z * (sizeof(gj_scan_summary) / 4)], MIXED ? min(seg_count_max, g.segment_count) : seg_count_max);
    uint32_t first[GJ_MAX_COMP], run[GJ_MAX_COMP], bytes = 0; // (bytes: the lengths of the entries this lane selected)
    {
        uint32_t at = 0;
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++) { first[c] = at; run[c] = 0; at += (uint32_t)rb.sel_count[c]; }
    }
    for (int base = 0; base < n; base += GJ_SEL_CHUNK) { // (n is the same in every lane: every lane makes every trip)
        const int i = base + tid;
        const uint32_t s = i < n ? seg_index[i] : 0xFFFFFFFFu;
        const bool in = i < n && gj_segment_in_cover(g, r, (int)s);
        const int sc = in ? gj_segment_scan(g, s) : -1;
        if (in) bytes += seg_len[i];
        uint32_t below = 0; // selected entries of this lane's scan in front of it inside its wave
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++) {
            const unsigned long long b = __ballot(sc == c);
            if (lane == 0) s_wave[c][wave] = (uint32_t)__popcll(b);
            if (sc == c) below = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++) {
            uint32_t front = 0, all = 0;
            for (int w = 0; w < GJ_SEL_CHUNK / GJ_WAVE; w++) {
                if (w < wave) front += s_wave[c][w];
                all += s_wave[c][w];
            }
            if (sc == c) {
                const uint32_t k = run[c] + front + below;
                if (k < (uint32_t)rb.sel_count[c] && first[c] + k < out_stride) { // (more than planned: another stream than the geometry's -- the host sees the count)
                    out[first[c] + k] = seg_pos[i];
                    out[out_stride + first[c] + k] = seg_len[i];
                    out[2 * out_stride + first[c] + k] = s;
                }
            }
            run[c] += all;
        }
        __syncthreads(); // (s_wave is rewritten by the next trip)
    }
#pragma unroll
    for (int c = 0; c < GJ_MAX_COMP; c++)
        for (uint32_t k = run[c] + (uint32_t)tid; k < (uint32_t)rb.sel_count[c] && first[c] + k < out_stride; k += GJ_SEL_CHUNK) {
            out[first[c] + k] = 0u;
            out[out_stride + first[c] + k] = 0u;
            out[2 * out_stride + first[c] + k] = 0xFFFFFFFFu;
        }
#pragma unroll
    for (int c = 0; c < GJ_MAX_COMP; c++)
        if (tid == c) h_found[c] = run[c];
    if (h_bytes != nullptr) { // (what the entropy decoder is handed of this frame: the waves' sums through LDS, one store)
        const uint32_t inc = gj_wave_incl_scan(bytes);
        if (lane == 63) s_wave[0][wave] = inc;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
            for (int w = 0; w < GJ_SEL_CHUNK / GJ_WAVE; w++) all += s_wave[0][w];
            h_bytes[z] = all;
        }
    }
}

void gj_launch_segment_select_batch(const gj_dec_job* job, hipStream_t st)
{
    const gj_geom& g = job->g;
    const gj_region& r = job->region;
    const uint32_t stride = (uint32_t)g.segment_count + GJ_MAX_COMP;
    auto kern = g.fb.geoms != nullptr ? k_segment_select_batch<true> : k_segment_select_batch<false>;
    hipLaunchKernelGGL(kern, dim3(1, 1, job->batch.count), dim3(GJ_SEL_CHUNK), 0, st, g, r, job->d_seg_pos, job->d_seg_len, job->d_seg_index,
                       job->seg_count, job->d_seg_count, r.d_sel, stride, r.h_sel_count, r.h_sel_bytes);
}

// ================================================================================================
// IDCT side
// ================================================================================================
// gr: the region image's geometry whose component planes are the COVER (gj_geom_init_region): blocks_x / blocks_y, data_width / data_height and
// data_offset of every component describe the cover-sized planes. One lane per block of the cover; a block of the cover is block
// (bx0 + bx, by0 + by) of the component's coefficient plane, which holds its blocks in raster order for every kind of scan.
// (BATCH: gr holds the planes of the largest cover of the batch, r is the frame's: lanes beyond the frame's own cover leave)
// (r: gj_region::frame, or the frame's record where it lies in device memory)
// one block: its 64 coefficients at blk (float table qf of its component) -> its 8 x 8 samples at dst, rows `pitch` bytes apart
__device__ __forceinline__ void gj_idct_region_block(const int16_t* __restrict__ blk, const float* __restrict__ qf, uint8_t* __restrict__ dst, const size_t pitch)
{
    uint32_t w[32];
    {
        const uint4* p = reinterpret_cast<const uint4*>(blk);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint4 v = p[q];
            w[q * 4] = v.x; w[q * 4 + 1] = v.y; w[q * 4 + 2] = v.z; w[q * 4 + 3] = v.w;
        }
    }
    uint32_t px[16];
    gj_idct_pk(w, qf, px);
#pragma unroll
    for (int q = 0; q < 8; q++) *reinterpret_cast<uint2*>(dst + (size_t)q * pitch) = make_uint2(px[2 * q], px[2 * q + 1]);
}

template <bool BATCH>
__device__ __forceinline__ void gj_idct_region_body(const gj_geom& g, const gj_geom& gr, const gj_region_frame& r, const int16_t* __restrict__ coefs,
                                                    const float* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    const unsigned gb = blockIdx.x * 256u + threadIdx.x;
    if (gb >= (unsigned)gr.block_count) return;
    if (r.scale > 1) return; // (a prescaled frame of a crop-and-resize call: k_idct_region_scaled, k_idct_region_scaled_comp -- whole or per component)
    unsigned bx, by;
    const int c = gj_block_of(gr, gb, bx, by);
    const gj_comp_geom& k = gr.comp[c];
    if (BATCH && (bx >= (unsigned)(r.bx1[c] - r.bx0[c]) || by >= (unsigned)(r.by1[c] - r.by0[c]))) return;
    const gj_comp_geom& kf = g.comp[c];
    const unsigned fbx = (unsigned)r.bx0[c] + bx, fby = (unsigned)r.by0[c] + by;
    if (fbx >= (unsigned)kf.blocks_x || fby >= (unsigned)kf.blocks_y) return; // (cannot happen: the cover lies inside the component's grid)
    gj_idct_region_block(coefs + kf.data_offset + ((size_t)fby * kf.blocks_x + fbx) * 64, qtab + kf.q_table * 64,
                         planes + k.data_offset + (size_t)by * 8 * k.data_width + bx * 8, (size_t)k.data_width);
}

__global__ __launch_bounds__(256) void k_idct_region(const gj_geom g, const gj_geom gr, const gj_region r, const int16_t* __restrict__ coefs,
                                                     const float* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    gj_idct_region_body<false>(g, gr, r.frame, coefs, qtab, planes);
}

// frame blockIdx.z of a batch of regions (the planes of a frame take as many bytes as its coefficients take elements at most)
// (MIXED: frames of different image sizes -- the coefficient planes of frame z are laid out by ITS geometry, gj_frame_geom; the cover planes by gr)
// (HDRS: frames with headers of their own, gj_batch::own_headers -- frame z's quantisation tables are its table set's, gj_frame_tabset_words; an
// instantiation of its own, so that the batches without such records keep their code)
template <bool MIXED, bool HDRS = false>
__global__ __launch_bounds__(256) void k_idct_region_batch(const gj_geom g, const gj_geom gr, const gj_region rb, const int16_t* __restrict__ coefs,
                                                           const float* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    const size_t z = blockIdx.z;
    gj_idct_region_body<true>(gj_frame_geom<MIXED>(g), gr, rb.d_frames[z], coefs + z * g.fb.coefs, qtab + gj_frame_tabset_words<HDRS>(g) / 2, planes + z * g.fb.coefs);
}

// The same for a frame dec_opt_resize_prescale reduces by s = 8 / N: block (bx, by) of the cover leaves the N x N samples of k_idct_scaled -- the
// corner of the block, gj_dequant_clamp with the uint16 table, gj_idct_corner<N> -- at (bx N, by N) of the component's REDUCED cover plane, laid out
// like k_idct_scaled's reduced planes inside the slot of the full-size ones: pitch data_width N / 8, offset data_offset N N / 64 (data_offset is a
// multiple of 64, data_width of 8, the slot's base of 64: rows of N bytes are N-byte aligned). Reads and writes stay inside the frame's own cover.
// one block: the N x N corner of its coefficients at blk (uint16 table q of its component) -> block (bx, by) of component k's reduced cover plane
template <int N>
__device__ __forceinline__ void gj_idct_region_scaled_block(const gj_comp_geom& k, const unsigned bx, const unsigned by, const int16_t* __restrict__ blk,
                                                            const uint16_t* __restrict__ q, uint8_t* __restrict__ planes)
{
    int D[N * N];
    gj_corner_from_plane<N>(blk, D);
#pragma unroll
    for (int v = 0; v < N; v++)
#pragma unroll
        for (int u = 0; u < N; u++) D[v * N + u] = gj_dequant_clamp(D[v * N + u], (int)q[v * 8 + u]);
    uint32_t px[N];
    gj_idct_corner<N>(D, px);
    const size_t pitch = (size_t)k.data_width * N / 8;
    uint8_t* dst = planes + k.data_offset * (N * N) / 64 + (size_t)by * N * pitch + (size_t)bx * N;
#pragma unroll
    for (int y = 0; y < N; y++) {
        if (N == 4) *reinterpret_cast<uint32_t*>(dst + y * pitch) = px[y];
        else if (N == 2) *reinterpret_cast<uint16_t*>(dst + y * pitch) = (uint16_t)px[y];
        else dst[0] = (uint8_t)px[0];
    }
}

template <int N, bool BATCH>
__device__ __forceinline__ void gj_idct_region_scaled_body(const gj_geom& g, const gj_geom& gr, const gj_region_frame& r, const int16_t* __restrict__ coefs,
                                                           const uint16_t* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    const unsigned gb = blockIdx.x * 256u + threadIdx.x;
    if (gb >= (unsigned)gr.block_count) return;
    unsigned bx, by;
    const int c = gj_block_of(gr, gb, bx, by);
    const gj_comp_geom& k = gr.comp[c];
    if (BATCH && (bx >= (unsigned)(r.bx1[c] - r.bx0[c]) || by >= (unsigned)(r.by1[c] - r.by0[c]))) return;
    const gj_comp_geom& kf = g.comp[c];
    const unsigned fbx = (unsigned)r.bx0[c] + bx, fby = (unsigned)r.by0[c] + by;
    if (fbx >= (unsigned)kf.blocks_x || fby >= (unsigned)kf.blocks_y) return; // (cannot happen: the cover lies inside the component's grid)
    gj_idct_region_scaled_block<N>(k, bx, by, coefs + kf.data_offset + ((size_t)fby * kf.blocks_x + fbx) * 64, qtab + kf.q_table * 64, planes);
}

// ONE launch for every scale: the frame's scale is the same in all lanes of a workgroup (blockIdx.z = frame), so the switch does not diverge; a
// frame of scale 1 leaves (k_idct_region_batch transforms it). The figures of this choice: profiles/idct_side_resources.md.
template <bool BATCH>
__device__ __forceinline__ void gj_idct_region_scaled_switch(const gj_geom& g, const gj_geom& gr, const gj_region_frame& r, const int16_t* __restrict__ coefs,
                                                             const uint16_t* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    if (r.per_comp) return; // (reduced per component: k_idct_region_scaled_comp)
    switch (r.scale) {
    case 2: gj_idct_region_scaled_body<4, BATCH>(g, gr, r, coefs, qtab, planes); break;
    case 4: gj_idct_region_scaled_body<2, BATCH>(g, gr, r, coefs, qtab, planes); break;
    case 8: gj_idct_region_scaled_body<1, BATCH>(g, gr, r, coefs, qtab, planes); break;
    default: break;
    }
}

__global__ __launch_bounds__(256) void k_idct_region_scaled(const gj_geom g, const gj_geom gr, const gj_region r, const int16_t* __restrict__ coefs,
                                                            const uint16_t* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    gj_idct_region_scaled_switch<false>(g, gr, r.frame, coefs, qtab, planes);
}

template <bool MIXED, bool HDRS = false>
__global__ __launch_bounds__(256) void k_idct_region_scaled_batch(const gj_geom g, const gj_geom gr, const gj_region rb, const int16_t* __restrict__ coefs,
                                                                  const uint16_t* __restrict__ qtab, uint8_t* __restrict__ planes)
{
    const size_t z = blockIdx.z;
    gj_idct_region_scaled_switch<true>(gj_frame_geom<MIXED>(g), gr, rb.d_frames[z], coefs + z * g.fb.coefs, qtab + gj_frame_tabset_words<HDRS>(g), planes + z * g.fb.coefs);
}

// The same for a frame that is reduced PER COMPONENT (gj_region_frame::per_comp, dec_opt_resize_prescale_subsampled: a 4:2:0-like stream, sub_h == sub_v
// in {1, 2}): component c's blocks leave N_c x N_c samples, N_c = 8 sub_h / scale -- at scale 2 luma 4 and chroma 8, at 4 luma 2 and chroma 4, at 8
// luma 1 and chroma 2 --, so that every reduced plane has one sample per reduced pixel. N_c <= 4: the arithmetic above; N_c = 8: k_idct_region's
// (gj_idct_pk with the float table), into the same place the full-size kernel writes. The planes lie where the formulas above put them with N_c for N;
// the host admits only streams whose sub_h does not fall from one component to the next, for which those ranges do not overlap.
// One lane per block of the cover, the blocks of a component one after the other (gj_block_of): N_c is the same in all lanes of a wave except in the
// waves that hold the last blocks of one component and the first of the next -- at most comp_count - 1 = 2 waves per frame, which run two arms.
// Every other frame leaves at entry (the same decision in all lanes of a workgroup: blockIdx.z = frame).
template <bool BATCH>
__device__ __forceinline__ void gj_idct_region_scaled_comp_body(const gj_geom& g, const gj_geom& gr, const gj_region_frame& r, const int16_t* __restrict__ coefs,
                                                                const uint16_t* __restrict__ qtab, const float* __restrict__ qtabf, uint8_t* __restrict__ planes)
{
    if (!r.per_comp || r.scale < 2) return;
    const unsigned gb = blockIdx.x * 256u + threadIdx.x;
    if (gb >= (unsigned)gr.block_count) return;
    unsigned bx, by;
    const int c = gj_block_of(gr, gb, bx, by);
    const gj_comp_geom& k = gr.comp[c];
    if (BATCH && (bx >= (unsigned)(r.bx1[c] - r.bx0[c]) || by >= (unsigned)(r.by1[c] - r.by0[c]))) return;
    const gj_comp_geom& kf = g.comp[c];
    const unsigned fbx = (unsigned)r.bx0[c] + bx, fby = (unsigned)r.by0[c] + by;
    if (fbx >= (unsigned)kf.blocks_x || fby >= (unsigned)kf.blocks_y) return; // (cannot happen: the cover lies inside the component's grid)
    const int16_t* blk = coefs + kf.data_offset + ((size_t)fby * kf.blocks_x + fbx) * 64;
    const uint16_t* q = qtab + kf.q_table * 64;
    switch (8u * (unsigned)kf.sub_h / (unsigned)r.scale) { // N_c
    case 8: gj_idct_region_block(blk, qtabf + kf.q_table * 64, planes + k.data_offset + (size_t)by * 8 * k.data_width + bx * 8, (size_t)k.data_width); break;
    case 4: gj_idct_region_scaled_block<4>(k, bx, by, blk, q, planes); break;
    case 2: gj_idct_region_scaled_block<2>(k, bx, by, blk, q, planes); break;
    case 1: gj_idct_region_scaled_block<1>(k, bx, by, blk, q, planes); break;
    default: break; // (cannot happen: sub_h is 1 or 2, scale 2, 4 or 8, and sub_h 2 comes with every scale)
    }
}

__global__ __launch_bounds__(256) void k_idct_region_scaled_comp(const gj_geom g, const gj_geom gr, const gj_region r, const int16_t* __restrict__ coefs,
                                                                 const uint16_t* __restrict__ qtab, const float* __restrict__ qtabf, uint8_t* __restrict__ planes)
{
    gj_idct_region_scaled_comp_body<false>(g, gr, r.frame, coefs, qtab, qtabf, planes);
}

template <bool MIXED, bool HDRS = false>
__global__ __launch_bounds__(256) void k_idct_region_scaled_comp_batch(const gj_geom g, const gj_geom gr, const gj_region rb, const int16_t* __restrict__ coefs,
                                                                       const uint16_t* __restrict__ qtab, const float* __restrict__ qtabf, uint8_t* __restrict__ planes)
{
    const size_t z = blockIdx.z;
    const size_t set = gj_frame_tabset_words<HDRS>(g);
    gj_idct_region_scaled_comp_body<true>(gj_frame_geom<MIXED>(g), gr, rb.d_frames[z], coefs + z * g.fb.coefs, qtab + set, qtabf + set / 2, planes + z * g.fb.coefs);
}

// sample of component c that pixel (x, y) of the REGION needs, in the cover-sized plane: pixel (r.x + x, r.y + y) of the stream's image
// (N = 8, or with a prescale N = 8 / gj_region_frame::scale: the reduced cover plane of k_idct_region_scaled and pixel (x' + x, y' + y) of the reduced image)
// (PER_COMP, a frame reduced per component: N = N_c, and the component's reduced plane has ONE sample per reduced pixel -- sample (x' + x, y' + y), no
// division by sub_h / sub_v)
template <bool PER_COMP = false>
__device__ __forceinline__ size_t gj_region_sample(const gj_comp_geom& k, const gj_region_frame& r, const int c, const unsigned x, const unsigned y,
                                                   const unsigned N = 8u)
{
    const unsigned sx = (PER_COMP ? (unsigned)r.x + x : ((unsigned)r.x + x) / (unsigned)k.sub_h) - (unsigned)r.bx0[c] * N;
    const unsigned sy = (PER_COMP ? (unsigned)r.y + y : ((unsigned)r.y + y) / (unsigned)k.sub_v) - (unsigned)r.by0[c] * N;
    // (the cover holds them; its own size bounds them -- the planes of a frame of a batch are laid out for the largest cover, the frame's own may be smaller)
    const unsigned cw = (unsigned)(r.bx1[c] - r.bx0[c]) * N, ch = (unsigned)(r.by1[c] - r.by0[c]) * N;
    const size_t offset = N == 8u ? (size_t)k.data_offset : (size_t)(k.data_offset * (N * N) / 64), pitch = N == 8u ? (size_t)k.data_width : (size_t)k.data_width * N / 8;
    return offset + (size_t)min(sy, ch - 1u) * pitch + min(sx, cw - 1u);
}

// k_postprocess for a region: one lane per pixel of the W x H image (raw_width x height of gr)
__device__ __forceinline__ void gj_postprocess_region_body(const gj_geom& gr, const gj_region_frame& r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const unsigned W = (unsigned)gr.raw_width, H = (unsigned)gr.height;
    const unsigned pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= W * H) return;
    const unsigned y = pos / W, x = pos - y * W;
    int v[4] = {0, 0, 0, gr.pixel_format == GJ_PF_4444_P0123 ? 0xFF : 0};
#pragma unroll
    for (int c = 0; c < GJ_MAX_COMP; c++) {
        if (c >= gr.comp_count) break;
        v[c] = planes[gj_region_sample(gr.comp[c], r, c, x, y)];
    }
    gj_store_pixel(gr, raw, W, H, x, y, pos, v);
}

__global__ __launch_bounds__(256) void k_postprocess_region(const gj_geom gr, const gj_region r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    gj_postprocess_region_body(gr, r.frame, planes, raw);
}

// frame blockIdx.z of a batch of regions: its rectangle, its cover planes (laid out for the largest cover: gr), its pixels
__global__ __launch_bounds__(256) void k_postprocess_region_batch(const gj_geom gr, const gj_region rb, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const size_t z = blockIdx.z;
    gj_postprocess_region_body(gr, rb.d_frames[z], planes + z * gr.fb.coefs, raw + z * gr.fb.raw);
}

// k_copy_planes_out for a region: plane c of the result is the crop of plane c at (r.x / sub_h, r.y / sub_v), k.width x k.height samples
__device__ __forceinline__ void gj_copy_planes_region_body(const gj_geom& gr, const gj_region_frame& r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    size_t dst_off = 0;
    for (int c = 0; c < gr.comp_count; c++) {
        const gj_comp_geom& k = gr.comp[c];
        const size_t dpitch = (size_t)k.width + gr.width_padding;
        const size_t n = (size_t)k.width * k.height;
        const size_t ox = (size_t)(r.x / k.sub_h - r.bx0[c] * 8), oy = (size_t)(r.y / k.sub_v - r.by0[c] * 8);
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
            const size_t y = i / k.width, x = i - y * k.width;
            raw[dst_off + y * dpitch + x] = planes[k.data_offset + (oy + y) * k.data_width + ox + x];
        }
        dst_off += dpitch * k.height;
    }
}

__global__ __launch_bounds__(256) void k_copy_planes_region(const gj_geom gr, const gj_region r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    gj_copy_planes_region_body(gr, r.frame, planes, raw);
}

__global__ __launch_bounds__(256) void k_copy_planes_region_batch(const gj_geom gr, const gj_region rb, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const size_t z = blockIdx.z;
    gj_copy_planes_region_body(gr, rb.d_frames[z], planes + z * gr.fb.coefs, raw + z * gr.fb.raw);
}

// The store of a tensor call's pixel stage: channel c of output pixel `pos` (of `plane` = OW x OH) -> element pos of plane c (CHW) or element
// pos x channels + c (HWC) of the frame's tensor `out`, as gj_tensor_element makes it. One lane per pixel: a wave's stores to a plane of a CHW frame are
// 64 consecutive elements, to an HWC frame 64 x channels consecutive elements. dtype and layout are the same in every lane (kernel arguments).
__device__ __forceinline__ void gj_tensor_store(const gj_tensor& t, uint8_t* __restrict__ out, const unsigned plane, const unsigned pos, const int (&v)[4])
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c >= t.channels) break;
        const size_t at = t.layout == GJ_TENSOR_HWC ? (size_t)pos * (unsigned)t.channels + c : (size_t)c * plane + pos;
        const uint32_t e = gj_tensor_element(t, c, v[c]);
        if (t.dtype == GJ_TENSOR_F32) reinterpret_cast<uint32_t*>(out)[at] = e;
        else reinterpret_cast<uint16_t*>(out)[at] = (uint16_t)e;
    }
}

// Crop-and-resize (gj_region::resize): the pixel stage of a call whose rectangle -- r.w x r.h, every frame's own -- is resampled to ONE output size,
// gr.width x gr.height (gr: the geometry of the OUTPUT image over the cover's planes). One lane per output pixel: its four source pixels of the
// rectangle (gj_resize_taps; a mirrored frame reads column OW - 1 - i), each made like k_postprocess_region makes a pixel -- the components' samples
// inside the cover, the expansion of a single component, the colour transform --, blended per channel with 8-bit weights (gj_resize_blend) and
// stored in the output format. A frame with a prescale (gj_region_frame::scale > 1) reads the reduced cover planes at the taps of the reduced image.
// The result is the resize of what the region call returns, which is why a no_transform configuration
// (k_copy_planes_region: no colour stage) blends the samples as they are. Output formats whose pixels share no samples only (the host refuses the others).
// TENSOR (gj_region::tensor, gpujpeg_amd_decoder_decode_batch_crop_resize_tensor): the same up to and including the blend; the channels of the blended pixel
// then go to the frame's tensor as float(byte) * scale + bias in the call's element type and layout (gj_tensor_store) instead of to the pixel format's bytes.
// PER_COMP: a frame that is reduced per component (gj_region_frame::per_comp) -- the taps are the prescaled frame's, in reduced pixels with s; the sample
// of component c comes from ITS reduced plane, N_c = N sub_h (gj_region_sample<true>). Behind a template parameter so that every other frame runs the
// instructions it ran without it; the choice is the frame's, the same in every lane of a workgroup (gj_resize_region_body).
template <bool TENSOR, bool PER_COMP>
__device__ __forceinline__ void gj_resize_region_pixel(const gj_geom& gr, const gj_region_frame& r, const gj_tensor& t, const uint8_t* __restrict__ planes,
                                                       uint8_t* __restrict__ raw)
{
    const unsigned OW = (unsigned)gr.width, OH = (unsigned)gr.height;
    const unsigned pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= OW * OH) return;
    const unsigned j = pos / OW, i = pos - j * OW;
    int sx[2], sy[2], fx, fy;
    const int s = r.scale > 1 ? r.scale : 1; // (a prescaled frame: the taps in the reduced image, the samples in the reduced cover planes)
    const unsigned N = 8u / (unsigned)s;
    gj_resize_taps(r.mirror ? (int)(OW - 1u - i) : (int)i, r.src_w, (int)OW, r.off_x, s, r.w, sx[0], sx[1], fx);
    gj_resize_taps((int)j, r.src_h, (int)OH, r.off_y, s, r.h, sy[0], sy[1], fy);
    int v[4][4]; // [source pixel: top left, top right, bottom left, bottom right][channel]
#pragma unroll
    for (int q = 0; q < 4; q++) {
        v[q][0] = v[q][1] = v[q][2] = 0;
        v[q][3] = gr.pixel_format == GJ_PF_4444_P0123 ? 0xFF : 0;
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++) {
            if (c >= gr.comp_count) break;
            if (PER_COMP) v[q][c] = planes[gj_region_sample<true>(gr.comp[c], r, c, (unsigned)sx[q & 1], (unsigned)sy[q >> 1], N * (unsigned)gr.comp[c].sub_h)];
            else v[q][c] = planes[gj_region_sample(gr.comp[c], r, c, (unsigned)sx[q & 1], (unsigned)sy[q >> 1], N)];
        }
        if (!gr.no_transform) gj_pixel_transform(gr, v[q]);
    }
    int o[4];
#pragma unroll
    for (int ch = 0; ch < 4; ch++) o[ch] = gj_resize_blend(v[0][ch], v[1][ch], v[2][ch], v[3][ch], fx, fy);
    if (TENSOR) gj_tensor_store(t, raw, OW * OH, pos, o);
    else gj_pixel_store(gr, raw, OW, OH, i, j, pos, o);
}

template <bool TENSOR>
__device__ __forceinline__ void gj_resize_region_body(const gj_geom& gr, const gj_region_frame& r, const gj_tensor& t, const uint8_t* __restrict__ planes,
                                                      uint8_t* __restrict__ raw)
{
    if (r.per_comp) gj_resize_region_pixel<TENSOR, true>(gr, r, t, planes, raw);
    else gj_resize_region_pixel<TENSOR, false>(gr, r, t, planes, raw);
}

__global__ __launch_bounds__(256) void k_resize_region(const gj_geom gr, const gj_region r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    gj_resize_region_body<false>(gr, r.frame, r.tensor, planes, raw);
}

__global__ __launch_bounds__(256) void k_resize_region_tensor(const gj_geom gr, const gj_region r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    gj_resize_region_body<true>(gr, r.frame, r.tensor, planes, raw);
}

// frame blockIdx.z of a batch: its rectangle and mirror flag, its cover planes (laid out for the largest cover: gr), its slot of the output
__global__ __launch_bounds__(256) void k_resize_region_batch(const gj_geom gr, const gj_region rb, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const size_t z = blockIdx.z;
    gj_resize_region_body<false>(gr, rb.d_frames[z], rb.tensor, planes + z * gr.fb.coefs, raw + z * gr.fb.raw);
}

// ... and its slot of the output as a tensor (gr.fb.raw: bytes between two frames, a multiple of the element size)
__global__ __launch_bounds__(256) void k_resize_region_tensor_batch(const gj_geom gr, const gj_region rb, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const size_t z = blockIdx.z;
    gj_resize_region_body<true>(gr, rb.d_frames[z], rb.tensor, planes + z * gr.fb.coefs, raw + z * gr.fb.raw);
}

// Crop-and-resize with the antialiased filter (gj_region::filter, dec_opt_resize_filter = antialias): the pixel stage above with the triangle filter
// of gj_resize_aa_taps in place of the four-tap blend, separably -- along the rows with u_i(k), down the columns with v_j(l) -- and exactly: one 64-bit
// multiply-add per row and channel, one 64-bit division per channel (gj_resize_aa_round). No prescale under this filter: N = 8 throughout.
// WIDE: the row's sums in 64 bits, for a frame whose rectangle is so wide that 255 U_i may pass 2^32 (gj_resize_aa_row_fits_32: w above ~32 900);
// every other frame keeps them in 32. The choice is the frame's, the same in every lane of a workgroup.
// The fourth channel of GJ_PF_4444_P0123 is 0xFF in every source pixel and a constant stays a constant under the filter: it is stored as that.
template <bool WIDE> struct gj_aa_row_sum { typedef uint32_t type; };
template <> struct gj_aa_row_sum<true> { typedef uint64_t type; };

// acc[ch] = sum over the taps k = kx .. kx + nx - 1 of output column ii of u_ii(k) P[y][k][ch], P[y][k] = pixel (k, y) of the rectangle made as
// gj_resize_region_body makes it: the components' samples (gj_region_sample), gj_pixel_transform unless no_transform.
// gj_region_sample -- two divisions per component -- is asked for the row's FIRST tap only. Along a row the sample of component c moves on by one
// where (r.x + k) reaches a multiple of sub_h, and stays at the last column of the frame's cover (the clamp of gj_region_sample, which no tap of
// a rectangle inside the image meets): `rem` counts the pixels into the sample, `room` the columns left.
template <bool WIDE>
__device__ __forceinline__ void gj_resize_aa_row(const gj_geom& gr, const gj_region_frame& r, const uint8_t* __restrict__ planes, const int ii, const int kx,
                                                 const int nx, const unsigned y, typename gj_aa_row_sum<WIDE>::type (&acc)[3])
{
    typedef typename gj_aa_row_sum<WIDE>::type row_t;
    const uint8_t* at[GJ_MAX_COMP] = {planes, planes, planes, planes};
    unsigned rem[GJ_MAX_COMP] = {0, 0, 0, 0}, room[GJ_MAX_COMP] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < GJ_MAX_COMP; c++) {
        if (c >= gr.comp_count) break;
        const gj_comp_geom& k = gr.comp[c];
        const unsigned X = (unsigned)r.x + (unsigned)kx, q = X / (unsigned)k.sub_h;
        const unsigned sx = q - (unsigned)r.bx0[c] * 8u, last = (unsigned)(r.bx1[c] - r.bx0[c]) * 8u - 1u;
        at[c] = planes + gj_region_sample(k, r, c, (unsigned)kx, y);
        rem[c] = X - q * (unsigned)k.sub_h;
        room[c] = sx < last ? last - sx : 0u;
    }
    acc[0] = acc[1] = acc[2] = 0;
    for (int k = 0; k < nx; k++) {
        const uint32_t u = gj_resize_aa_weight(r.w, gr.width, ii, kx + k);
        int v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < GJ_MAX_COMP; c++) {
            if (c >= gr.comp_count) break;
            v[c] = *at[c];
            if (++rem[c] == (unsigned)gr.comp[c].sub_h) {
                rem[c] = 0;
                if (room[c]) { room[c]--; at[c]++; }
            }
        }
        if (!gr.no_transform) gj_pixel_transform(gr, v);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) acc[ch] += (row_t)u * (uint32_t)v[ch];
    }
}

// A workgroup per tile of GJ_AA_TX x GJ_AA_TY output pixels (blockIdx.x, blockIdx.y; 256 lanes), one lane per pixel of the tile. The rows of the
// rectangle the tile's pixels weigh -- from the first tap of its first row to the last tap of its last -- are taken GJ_AA_TY at a time: lane
// (ti, tj) leaves the sums of row base + tj for ITS column in LDS (gj_resize_aa_row), and after the barrier adds, of those GJ_AA_TY rows, the ones
// inside its own pixel's taps, each times v_j(l). Neighbouring output rows share half of their source rows when reducing: a source pixel is made
// and weighted along its row about once per output column that holds it (twice when reducing) instead of once per output PIXEL (four times) --
// the figures of this shape and of the two it was measured against: profiles/crop_resize_antialias.md. Every lane reaches every barrier (lanes outside the image carry no work).
#define GJ_AA_TX 32
#define GJ_AA_TY 8
template <bool TENSOR, bool WIDE>
__device__ __forceinline__ void gj_resize_region_aa_tile(const gj_geom& gr, const gj_region_frame& r, const gj_tensor& t, const uint8_t* __restrict__ planes,
                                                         uint8_t* __restrict__ raw)
{
    typedef typename gj_aa_row_sum<WIDE>::type row_t;
    __shared__ row_t H[GJ_AA_TY][GJ_AA_TX][3];
    const unsigned OW = (unsigned)gr.width, OH = (unsigned)gr.height;
    const unsigned ti = threadIdx.x % GJ_AA_TX, tj = threadIdx.x / GJ_AA_TX;
    const unsigned i = blockIdx.x * GJ_AA_TX + ti, j0 = blockIdx.y * GJ_AA_TY, j = j0 + tj;
    const bool col = i < OW, pix = col && j < OH;
    const int ii = r.mirror ? (int)(OW - 1u - (col ? i : 0u)) : (int)(col ? i : 0u);
    int kx, nx, ky = 0, ny = 0;
    uint32_t U, V = 1;
    gj_resize_aa_taps(r.w, (int)OW, ii, kx, nx, U);
    if (pix) gj_resize_aa_taps(r.h, (int)OH, (int)j, ky, ny, V);
    // the tile's rows of the rectangle (j0 < OH: the grid has no tile below the image)
    int row_lo, row_hi, n;
    gj_resize_aa_range(r.h, (int)OH, (int)j0, row_lo, n);
    gj_resize_aa_range(r.h, (int)OH, (int)min(j0 + GJ_AA_TY - 1u, OH - 1u), row_hi, n);
    row_hi += n - 1;
    uint64_t S[3] = {0, 0, 0};
    for (int base = row_lo; base <= row_hi; base += GJ_AA_TY) {
        if (col && base + (int)tj <= row_hi) {
            row_t acc[3];
            gj_resize_aa_row<WIDE>(gr, r, planes, ii, kx, nx, (unsigned)(base + (int)tj), acc);
            H[tj][ti][0] = acc[0]; H[tj][ti][1] = acc[1]; H[tj][ti][2] = acc[2];
        }
        __syncthreads();
        const int from = max(base, ky), to = min(base + GJ_AA_TY, ky + ny); // (a pixel outside the image: ny = 0, no row)
        for (int l = from; l < to; l++) {
            const uint32_t vw = gj_resize_aa_weight(r.h, (int)OH, (int)j, l);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) S[ch] += (uint64_t)vw * H[l - base][ti][ch];
        }
        __syncthreads(); // (H is rewritten by the next trip)
    }
    if (!pix) return;
    int o[4];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch] = gj_resize_aa_round(S[ch], U, V);
    o[3] = gr.pixel_format == GJ_PF_4444_P0123 ? 0xFF : 0;
    const unsigned pos = j * OW + i;
    if (TENSOR) gj_tensor_store(t, raw, OW * OH, pos, o);
    else gj_pixel_store(gr, raw, OW, OH, i, j, pos, o);
}
static dim3 gj_resize_aa_grid(const gj_geom& gr, const unsigned frames)
{
    return dim3(((unsigned)gr.width + GJ_AA_TX - 1) / GJ_AA_TX, ((unsigned)gr.height + GJ_AA_TY - 1) / GJ_AA_TY, frames);
}

template <bool TENSOR>
__device__ __forceinline__ void gj_resize_region_aa_body(const gj_geom& gr, const gj_region_frame& r, const gj_tensor& t, const uint8_t* __restrict__ planes,
                                                         uint8_t* __restrict__ raw)
{
    if (gj_resize_aa_row_fits_32(r.w, gr.width)) gj_resize_region_aa_tile<TENSOR, false>(gr, r, t, planes, raw);
    else gj_resize_region_aa_tile<TENSOR, true>(gr, r, t, planes, raw);
}

__global__ __launch_bounds__(256) void k_resize_region_aa(const gj_geom gr, const gj_region r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    gj_resize_region_aa_body<false>(gr, r.frame, r.tensor, planes, raw);
}

__global__ __launch_bounds__(256) void k_resize_region_aa_tensor(const gj_geom gr, const gj_region r, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    gj_resize_region_aa_body<true>(gr, r.frame, r.tensor, planes, raw);
}

// frame blockIdx.z of a batch, as for k_resize_region_batch
__global__ __launch_bounds__(256) void k_resize_region_aa_batch(const gj_geom gr, const gj_region rb, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const size_t z = blockIdx.z;
    gj_resize_region_aa_body<false>(gr, rb.d_frames[z], rb.tensor, planes + z * gr.fb.coefs, raw + z * gr.fb.raw);
}

__global__ __launch_bounds__(256) void k_resize_region_aa_tensor_batch(const gj_geom gr, const gj_region rb, const uint8_t* __restrict__ planes, uint8_t* __restrict__ raw)
{
    const size_t z = blockIdx.z;
    gj_resize_region_aa_body<true>(gr, rb.d_frames[z], rb.tensor, planes + z * gr.fb.coefs, raw + z * gr.fb.raw);
}

// The IDCT side of a region call: cover blocks -> cover planes -> region pixels. A batch of regions (d_frames) runs the same stages through the
// _batch kernels with blockIdx.z = frame and grids for the largest cover (gr).
void gj_launch_idct_region(const gj_dec_job* job, hipStream_t st, const bool tokens, gj_event_t* ev)
{
    const gj_geom& gr = job->gs;
    const gj_region& r = job->region;
    const bool batch = r.d_frames != nullptr;
    const unsigned frames = batch ? job->batch.count : 1u;
    if (tokens) { // token mode: records and tokens of the cover's blocks -> region pixels (k_idct_tok_region_rgb444)
        gj_launch_idct_tok_region(job, st);
        if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[2], st));
        return;
    }
    // (crop-and-resize with a prescale: the frames of scale 1 through the full-size kernel, the others through the reduced-size one -- each launch
    // only where the chunk has such frames, gj_region::scale_mask; the frames that are reduced per component through the kernel of their own,
    // gj_region::comp_mask; every other region call: scale 1 alone)
    const dim3 grid(((unsigned)gr.block_count + 255) / 256, 1, frames);
    const unsigned comp = r.resize ? r.comp_mask : 0u;
    const unsigned scales = r.resize && (r.scale_mask || comp) ? r.scale_mask : 1u;
    const bool mixed = batch && job->g.fb.geoms != nullptr; // (frames of different image sizes: the instantiations that read every frame's own geometry)
    const bool hdrs = mixed && job->batch.own_headers != 0;    // (... with headers of their own: and every frame's own table set)
    auto idct_batch = hdrs ? k_idct_region_batch<true, true> : mixed ? k_idct_region_batch<true> : k_idct_region_batch<false>;
    auto scaled_batch = hdrs ? k_idct_region_scaled_batch<true, true> : mixed ? k_idct_region_scaled_batch<true> : k_idct_region_scaled_batch<false>;
    auto comp_batch = hdrs ? k_idct_region_scaled_comp_batch<true, true> : mixed ? k_idct_region_scaled_comp_batch<true> : k_idct_region_scaled_comp_batch<false>;
    if (scales & 1u) hipLaunchKernelGGL(batch ? idct_batch : k_idct_region, grid, dim3(256), 0, st, job->g, gr, r, job->d_coefs, job->d_qtabf, job->d_planes);
    if (scales & ~1u)
        hipLaunchKernelGGL(batch ? scaled_batch : k_idct_region_scaled, grid, dim3(256), 0, st, job->g, gr, r, job->d_coefs, job->d_qtab, job->d_planes);
    if (comp)
        hipLaunchKernelGGL(batch ? comp_batch : k_idct_region_scaled_comp, grid, dim3(256), 0, st, job->g, gr, r, job->d_coefs, job->d_qtab,
                           job->d_qtabf, job->d_planes);
    if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[2], st));
    if (r.resize) { // crop-and-resize: gr is the output image's geometry
        const unsigned n = (unsigned)gr.width * (unsigned)gr.height;
        if (r.filter == GJ_RESIZE_FILTER_ANTIALIAS) { // (dec_opt_resize_filter = antialias: the triangle filter's kernels on their own grid)
            if (r.tensor.on)
                hipLaunchKernelGGL(batch ? k_resize_region_aa_tensor_batch : k_resize_region_aa_tensor, gj_resize_aa_grid(gr, frames), dim3(256), 0, st, gr, r, job->d_planes, job->d_raw);
            else
                hipLaunchKernelGGL(batch ? k_resize_region_aa_batch : k_resize_region_aa, gj_resize_aa_grid(gr, frames), dim3(256), 0, st, gr, r, job->d_planes, job->d_raw);
        } else if (r.tensor.on) // (gpujpeg_amd_decoder_decode_batch_crop_resize_tensor: the same pixels, stored as the call's tensor)
            hipLaunchKernelGGL(batch ? k_resize_region_tensor_batch : k_resize_region_tensor, dim3((n + 255) / 256, 1, frames), dim3(256), 0, st, gr, r, job->d_planes, job->d_raw);
        else
            hipLaunchKernelGGL(batch ? k_resize_region_batch : k_resize_region, dim3((n + 255) / 256, 1, frames), dim3(256), 0, st, gr, r, job->d_planes, job->d_raw);
    } else if (gr.no_transform) {
        const size_t n = (size_t)gr.comp[0].width * gr.comp[0].height;
        hipLaunchKernelGGL(batch ? k_copy_planes_region_batch : k_copy_planes_region, dim3((unsigned)min((n + 255) / 256, (size_t)2048), 1, frames), dim3(256), 0, st,
                           gr, r, job->d_planes, job->d_raw);
    } else {
        const unsigned n = (unsigned)gr.raw_width * (unsigned)gr.height;
        hipLaunchKernelGGL(batch ? k_postprocess_region_batch : k_postprocess_region, dim3((n + 255) / 256, 1, frames), dim3(256), 0, st, gr, r, job->d_planes,
                           job->d_raw);
    }
}
