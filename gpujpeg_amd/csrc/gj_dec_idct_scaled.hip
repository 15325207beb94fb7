// gj_dec_idct_scaled.hip -- MI355X (gfx950, wave64) JPEG decoder: reduced-size output (dec_opt_scale = 1/2, 1/4, 1/8). Every 8x8 block leaves
// N x N samples (N = 4, 2, 1): the N-point inverse DCT of its low-frequency N x N corner, in integer arithmetic (DESIGN "Reduced-size decode"):
//
//     D[v][u] = clamp(F[v][u] * Q[v][u], -32768, 32767)                    u, v < N   (F, Q in natural order, v = vertical frequency)
//     T[y][u] = (sum_v M_N[y][v] * D[v][u] + 1024)  >> 11                  columns
//     S[y][x] = (sum_u M_N[x][u] * T[y][u] + 16384) >> 15                  rows
//     out     = clamp(S + 128, 0, 255)
//
// with M_N[x][u] = round(8192 k(u) cos((2x + 1) u pi / 2N)), k(0) = sqrt(1/8), k(u > 0) = 1/2. Nothing overflows 32 bits: the largest row of |M_4|
// sums to 11 143, so |sum| <= 11 143 * 32 768 in the first pass, |T| <= 178 288, and 11 143 * 178 288 + 16 384 < 2^31 in the second.
// The reference has no reduced decode: the mode is pinned by the numpy restatement of these four lines in tests/test_scaled_decode.py.
//
//   k_idct_scaled<N>                   from the coefficient planes into the REDUCED component planes, one lane per block; every configuration.
//                                      The pixel kernels of the full-size path (k_postprocess, k_copy_planes_out, k_channel_remap) follow with the
//                                      reduced geometry (gj_dec_job::gs).
//   k_idct_tok_scaled_rgb444<N, ..>    from the entropy decoder's tokens and block records to packed 3-byte pixels, one lane per block position
//                                      (the configuration of k_idct_tok_rgb444: three components 4:4:4, non-interleaved scans). N = 1 reads the
//                                      records only: the DC term is in them.
// Both know the frame dimension of a batch (blockIdx.z, gj_frame_strides): frame z's reduced planes lie z x gj_frame_strides::coefs bytes into
// d_planes -- where k_postprocess / k_copy_planes_out look for them with gs.fb = g.fb --, its pixels z x gj_frame_strides::raw bytes into d_raw.
// (part of the decoder's device code, see gj_dec_internal.h for the map of the files)
#include "gj_dec_internal.h"

// (gj_mn, gj_dequant_clamp, gj_idct_corner, gj_corner_from_plane: gj_dec_internal.h -- k_idct_region_scaled shares them)

// ================================================================================================
// (a) generic: coefficient planes -> reduced component planes, one lane per block like k_idct
// ================================================================================================
// A lane reads N rows of N coefficients out of its 128-byte block (N = 1: 2 bytes of every 128-byte line the wave touches -- the loads of this
// kernel are as uncoalesced as k_idct's and fetch the whole frame's lines for a fraction of their bytes; the token-fed kernel below is the fast
// path) and writes N rows of N bytes. `zero`: the whole block is cleared once it has been read, as k_idct does.
template <int N>
__global__ __launch_bounds__(256) void k_idct_scaled(const gj_geom g, int16_t* __restrict__ coefs, const uint16_t* __restrict__ qtab,
                                                     uint8_t* __restrict__ planes, const int zero)
{
    if (g.fb.sizes != nullptr) { // frame blockIdx.z of a batch (the reduced planes of a frame lie as far apart as the full-size ones: k_postprocess)
        coefs += (size_t)blockIdx.z * g.fb.coefs;
        planes += (size_t)blockIdx.z * g.fb.coefs;
    }
    const unsigned gb = blockIdx.x * 256u + threadIdx.x;
    if (gb >= (unsigned)g.block_count) return;
    unsigned bx, by;
    const gj_comp_geom& k = g.comp[gj_block_of(g, gb, bx, by)];
    int16_t* blk = coefs + (size_t)gb * 64;
    int D[N * N];
    gj_corner_from_plane<N>(blk, D);
    if (zero) {
        uint4* p = reinterpret_cast<uint4*>(blk);
#pragma unroll
        for (int r = 0; r < 8; r++) p[r] = make_uint4(0, 0, 0, 0);
    }
    const uint16_t* q = qtab + k.q_table * 64;
#pragma unroll
    for (int v = 0; v < N; v++)
#pragma unroll
        for (int u = 0; u < N; u++) D[v * N + u] = gj_dequant_clamp(D[v * N + u], (int)q[v * 8 + u]);
    uint32_t px[N];
    gj_idct_corner<N>(D, px);
    // the reduced plane: data_width * N / 8 samples per row, data_offset * N * N / 64 behind the first plane (data_offset is a multiple of 64,
    // data_width of 8: rows of N bytes are N-byte aligned)
    const size_t pitch = (size_t)k.data_width * N / 8;
    uint8_t* dst = planes + k.data_offset * (N * N) / 64 + (size_t)by * N * pitch + (size_t)bx * N;
#pragma unroll
    for (int y = 0; y < N; y++) {
        if (N == 4) *reinterpret_cast<uint32_t*>(dst + y * pitch) = px[y];
        else if (N == 2) *reinterpret_cast<uint16_t*>(dst + y * pitch) = (uint16_t)px[y];
        else dst[0] = (uint8_t)px[0];
    }
}

// ================================================================================================
// (b) token-fed, three components 4:4:4, non-interleaved scans, packed 3-byte pixels
// ================================================================================================
// One lane per block position, the three components' records as in k_idct_tok_rgb444 (with its guards for records nobody wrote and for blocks
// that arrive through the coefficient planes). N = 1 needs nothing else. N = 2, 4: the tokens of the wave's 64 blocks go through the wave's LDS
// stage (gj_tok_fetch's rule: one dense range that fits) and every lane keeps those of its block whose natural position lies in the N x N
// corner -- in registers, by compare-and-select, never through an indexed array (no scratch). A token on position 0 never replaces the record's DC
// term (damaged streams, see gj_tok_to_slot in gj_dec_idct.hip). Waves whose tokens are not one dense range read them from HBM lane by lane.
//
// Output: a wave's 64 blocks of one block row are 64 x 3N contiguous bytes in each of their N pixel rows. The lanes put their bytes into an LDS
// tile and the wave stores it as aligned dwords (the first and the last few bytes of a row that does not start on a dword: byte stores); waves that
// straddle two block rows, or the image's right / bottom edge, store byte by byte with bounds checks.
template <int N>
__device__ __forceinline__ void gj_corner_put(int (&F)[N * N], const uint32_t tok)
{
    const int pos = (int)(tok & 63u), v = pos >> 3, u = pos & 7;
    const int val = (int)(int16_t)tok >> 6;
    const int idx = (v < N && u < N) ? v * N + u : 0; // (0: outside the corner, or the DC position -- dropped either way)
#pragma unroll
    for (int i = 1; i < N * N; i++) F[i] = idx == i ? val : F[i];
}

template <int N, int CS_FROM, int CS_TO>
__global__ __launch_bounds__(256, 4) void k_idct_tok_scaled_rgb444(const gj_geom g, const int16_t* __restrict__ coefs, const uint2* __restrict__ d_rec,
                                                                    const uint16_t* __restrict__ d_tok, const uint32_t tok_cap,
                                                                    const uint16_t* __restrict__ qtab, uint8_t* __restrict__ raw, const int out_w,
                                                                    const int out_h, const int out_padding)
{
    if (g.fb.sizes != nullptr) { // frame blockIdx.z of a batch (tok_cap is a frame's; a reduced frame need not end on a dword: the stores below take
                                 // their alignment from the row's address, so from the frame's own base)
        const size_t z = blockIdx.z;
        coefs += z * g.fb.coefs; d_rec += z * g.fb.rec; d_tok += z * g.fb.tok;
        raw += z * g.fb.raw;
    }
    constexpr int ROWB = 64 * 3 * N;                                               // bytes of a wave's blocks in one pixel row
    __shared__ __attribute__((aligned(16))) uint16_t s_stage[4][N > 1 ? GJ_TOK_STAGE : 8];
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[4][N][ROWB / 4 + 1];   // (+ 1: the dword past the end that the shifted read touches)
    __shared__ int s_q[3][N * N];
    if (threadIdx.x < 3 * N * N) {
        const int c = threadIdx.x / (N * N), i = threadIdx.x % (N * N);
        s_q[c][i] = (int)qtab[g.comp[c].q_table * 64 + (i / N) * 8 + (i % N)];
    }
    const gj_comp_geom& k0 = g.comp[0];
    const unsigned nb = (unsigned)(k0.blocks_x * k0.blocks_y);
    const unsigned lb = blockIdx.x * 256u + threadIdx.x;
    const unsigned by = lb / (unsigned)k0.blocks_x, bx = lb - by * (unsigned)k0.blocks_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t* stage = s_stage[wave];

    // ---- 1. the three block records
    uint32_t start[3], cd[3]; // count << 16 | DC, bit 31: the block is in the coefficient planes
#pragma unroll
    for (int c = 0; c < 3; c++) gj_tok_record(g, d_rec, tok_cap, lb < nb, lb, c, start[c], cd[c]);
    __syncthreads(); // (s_q; everything below is private to a wave)

    // ---- 2. per component: corner coefficients -> samples
    uint32_t px[3][N];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t cnt = gj_rec_count(cd[c]);
        const bool in_plane = (int32_t)cd[c] < 0;
        int F[N * N];
#pragma unroll
        for (int i = 0; i < N * N; i++) F[i] = 0;
        if (in_plane) gj_corner_from_plane<N>(coefs + g.comp[c].data_offset + (size_t)lb * 64, F);
        else F[0] = (int)(int16_t)(cd[c] & 0xFFFFu);
        if constexpr (N > 1) {
            const GjTokRange tr = gj_tok_fetch(d_tok, start[c], cnt, lane);
            if (tr.fast) {
                gj_wave_sync(); // (the previous component's tokens have been read)
                *reinterpret_cast<uint4*>(stage + lane * 8) = tr.t0;
                if (lane * 8 + 512 < GJ_TOK_STAGE) *reinterpret_cast<uint4*>(stage + lane * 8 + 512) = tr.t1;
                gj_wave_sync();
                for (uint32_t a = start[c] - tr.S, b = a + cnt; a < b; a++) gj_corner_put<N>(F, stage[a]);
            } else {
                for (uint32_t a = start[c], b = a + cnt; a < b; a++) gj_corner_put<N>(F, d_tok[a]); // (a + cnt <= tok_cap, checked above)
            }
        }
#pragma unroll
        for (int i = 0; i < N * N; i++) F[i] = gj_dequant_clamp(F[i], s_q[c][i]);
        gj_idct_corner<N>(F, px[c]);
    }

    // ---- 3. colour transform, the lane's N rows of 3N bytes into the wave's tile
    uint8_t* tile = reinterpret_cast<uint8_t*>(s_tile[wave]);
    constexpr int TROW = (ROWB / 4 + 1) * 4;
    uint32_t packed[N][(3 * N + 3) / 4];
#pragma unroll
    for (int y = 0; y < N; y++) {
#pragma unroll
        for (int w = 0; w < (3 * N + 3) / 4; w++) packed[y][w] = 0;
#pragma unroll
        for (int x = 0; x < N; x++) {
            int a = (int)((px[0][y] >> (8 * x)) & 0xFFu), b = (int)((px[1][y] >> (8 * x)) & 0xFFu), cc = (int)((px[2][y] >> (8 * x)) & 0xFFu);
            gj_color_transform(CS_FROM, CS_TO, a, b, cc);
            const int v3[3] = {a, b, cc};
#pragma unroll
            for (int j = 0; j < 3; j++) packed[y][(3 * x + j) >> 2] |= (uint32_t)(v3[j] & 0xFF) << (8 * ((3 * x + j) & 3));
        }
        uint8_t* t = tile + y * TROW + lane * 3 * N;
        if (N == 4) {
            uint32_t* t4 = reinterpret_cast<uint32_t*>(t);
            t4[0] = packed[y][0]; t4[1] = packed[y][1]; t4[2] = packed[y][2];
        } else if (N == 2) {
            uint16_t* t2 = reinterpret_cast<uint16_t*>(t);
            t2[0] = (uint16_t)packed[y][0]; t2[1] = (uint16_t)(packed[y][0] >> 16); t2[2] = (uint16_t)packed[y][1];
        } else {
            t[0] = (uint8_t)packed[y][0]; t[1] = (uint8_t)(packed[y][0] >> 8); t[2] = (uint8_t)(packed[y][0] >> 16);
        }
    }
    gj_wave_sync();

    // ---- 4. store
    const size_t pitch = (size_t)out_w * 3 + out_padding;
    const unsigned lb_first = lb - (unsigned)lane, lb_last = lb_first + 63u;
    const unsigned by_first = lb_first / (unsigned)k0.blocks_x, bx_first = lb_first - by_first * (unsigned)k0.blocks_x;
    // the wave's 64 blocks: all there, in one block row, inside the image
    const bool dense = lb_last < nb && bx_first + 63u < (unsigned)k0.blocks_x && (bx_first + 64u) * N <= (unsigned)out_w && (by_first + 1u) * N <= (unsigned)out_h;
    if (dense) {
#pragma unroll
        for (int y = 0; y < N; y++) {
            uint8_t* G = raw + (size_t)(by_first * N + y) * pitch + (size_t)bx_first * 3 * N; // the row's ROWB bytes
            const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(G) & 3u);               // ... start `a` bytes behind a dword
            const uint32_t* trow = reinterpret_cast<const uint32_t*>(tile + y * TROW);
            // dword j of the aligned run holds the tile's bytes 4j - a .. 4j - a + 3
            for (uint32_t j = (uint32_t)lane; j * 4u < a + ROWB; j += 64u) {
                const int off = (int)(j * 4u) - (int)a;
                uint32_t w;
                if (a == 0) w = trow[j];
                else w = __builtin_amdgcn_alignbyte(trow[j], j ? trow[j - 1] : 0u, 4u - a);
                if (off >= 0 && off + 4 <= ROWB) {
                    *reinterpret_cast<uint32_t*>(G + off) = w;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (off + b >= 0 && off + b < ROWB) G[off + b] = (uint8_t)(w >> (8 * b));
                }
            }
        }
    } else if (lb < nb) {
#pragma unroll
        for (int y = 0; y < N; y++) {
            const unsigned py = by * N + y;
#pragma unroll
            for (int x = 0; x < N; x++) {
                const unsigned pxx = bx * N + x;
                if (py < (unsigned)out_h && pxx < (unsigned)out_w) {
                    uint8_t* p = raw + (size_t)py * pitch + (size_t)pxx * 3;
#pragma unroll
                    for (int j = 0; j < 3; j++) p[j] = (uint8_t)(packed[y][(3 * x + j) >> 2] >> (8 * ((3 * x + j) & 3)));
                }
            }
        }
    }
}

// ================================================================================================
// Kernel selection and launch
// ================================================================================================
typedef void (*gj_idct_tok_scaled_t)(const gj_geom, const int16_t*, const uint2*, const uint16_t*, uint32_t, const uint16_t*, uint8_t*, int, int, int);

// the instantiation for the geometry's colour pair (GJ_COLOR_PAIRS), or nullptr
template <int N>
static gj_idct_tok_scaled_t gj_idct_tok_scaled_kernel(const gj_geom& g)
{
#define GJ_X(F, T) k_idct_tok_scaled_rgb444<N, F, T>,
    static const gj_idct_tok_scaled_t k[] = {GJ_COLOR_PAIRS(GJ_X)};
#undef GJ_X
    const int pair = gj_color_pair(g);
    return pair >= 0 ? k[pair] : nullptr;
}

// does a token-fed reduced-size kernel exist for this configuration? (what gj_idct_tok_for serves with k_idct_tok_rgb444)
bool gj_idct_tok_scaled_for(const gj_geom& g)
{
    return !g.interleaved && gj_is_rgb444(g) && gj_color_pair(g) >= 0;
}

// The IDCT side of a reduced-size decode. Returns true when the pixels are in d_raw (token-fed kernel), false when the reduced component planes
// are in d_planes and the pixel kernels have to follow with job->gs.
bool gj_launch_idct_scaled(const gj_dec_job* job, hipStream_t st, const bool tokens)
{
    const gj_geom& g = job->g;
    const int N = 8 / job->scale;
    const unsigned frames = job->batch.count > 1 ? job->batch.count : 1u; // (a batch: blockIdx.z = frame)
    if (tokens) {
        const gj_idct_tok_scaled_t k = N == 4 ? gj_idct_tok_scaled_kernel<4>(g) : N == 2 ? gj_idct_tok_scaled_kernel<2>(g) : gj_idct_tok_scaled_kernel<1>(g);
        const unsigned nb = (unsigned)(g.comp[0].blocks_x * g.comp[0].blocks_y);
        hipLaunchKernelGGL(k, dim3((nb + 255) / 256, 1, frames), dim3(256), 0, st, g, job->d_coefs, (const uint2*)job->d_blkrec, (const uint16_t*)job->d_tok,
                           job->tok_cap, job->d_qtab, job->d_raw, job->gs.width, job->gs.height, job->gs.width_padding);
        return true;
    }
    const dim3 grid(((unsigned)g.block_count + 255) / 256, 1, frames);
    if (N == 4) hipLaunchKernelGGL(k_idct_scaled<4>, grid, dim3(256), 0, st, g, job->d_coefs, job->d_qtab, job->d_planes, job->zero_coefs);
    else if (N == 2) hipLaunchKernelGGL(k_idct_scaled<2>, grid, dim3(256), 0, st, g, job->d_coefs, job->d_qtab, job->d_planes, job->zero_coefs);
    else hipLaunchKernelGGL(k_idct_scaled<1>, grid, dim3(256), 0, st, g, job->d_coefs, job->d_qtab, job->d_planes, job->zero_coefs);
    return false;
}
