/*
 * gj_hip.h -- the thin C-ABI seam between the host C library (encoder/decoder drivers, JFIF writer and
 * reader, tables) and the hand-written gfx950 HIP code. Plain pointers and sizes only; the host side
 * never includes a HIP header.
 *
 * It replaces the reference's internal seam: the CUDA runtime subset the host C uses
 * (cudaMalloc/cudaMemcpyAsync/cudaEvent*, enumerated over the files of src/) and the five CUDA module groups
 *   gpujpeg_preprocessor_encode      src/gpujpeg_preprocessor.h:84-98
 *   gpujpeg_dct_gpu / gpujpeg_idct_gpu  src/gpujpeg_dct_gpu.h:46-55
 *   gpujpeg_huffman_gpu_encoder_*    src/gpujpeg_huffman_gpu_encoder.h:48-68
 *   gpujpeg_huffman_gpu_decoder_*    src/gpujpeg_huffman_gpu_decoder.h:47-60
 *   gpujpeg_postprocessor_decode     src/gpujpeg_postprocessor.h:46-59
 * coarsened into one launcher per direction (gj_hip_encode / gj_hip_decode), because on MI355X the
 * stages are fused and the stream is assembled on the device.
 */
#ifndef GJ_HIP_H
#define GJ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GJ_HIP_API __attribute__((visibility("default")))

typedef void* gj_stream_t; /* hipStream_t */
typedef void* gj_event_t;  /* hipEvent_t */

/* ------------------------------------------------------------------ runtime subset */
GJ_HIP_API int gj_hip_device_count(void);
GJ_HIP_API int gj_hip_get_device(int* device);
GJ_HIP_API int gj_hip_set_device(int device);
GJ_HIP_API int gj_hip_device_reset(void);
GJ_HIP_API int gj_hip_device_props(int device, char name[256], int* major, int* minor, size_t* global_mem, size_t* shared_mem,
                        int* regs_per_block, int* cu_count);
/* compute units of the current device (cached): what "the workgroups the device holds at once" is derived from */
GJ_HIP_API int gj_hip_cu_count(void);
GJ_HIP_API int gj_hip_runtime_version(int* driver, int* runtime);
GJ_HIP_API const char* gj_hip_last_error(void);

GJ_HIP_API void* gj_hip_malloc(size_t size);
GJ_HIP_API void gj_hip_free(void* p);
GJ_HIP_API void* gj_hip_host_alloc(size_t size); /* pinned */
GJ_HIP_API void gj_hip_host_free(void* p);
GJ_HIP_API int gj_hip_memcpy_h2d(void* dst, const void* src, size_t n, gj_stream_t s); /* async on s */
GJ_HIP_API int gj_hip_memcpy_d2h(void* dst, const void* src, size_t n, gj_stream_t s);
GJ_HIP_API int gj_hip_memcpy_d2d(void* dst, const void* src, size_t n, gj_stream_t s);
/* Copies of whole images between host and device. Large ones go through the process's one stream per direction and device ("copy lanes",
 * gj_runtime.hip: the host link carries both directions at once only that way) and are COMPLETE when the call returns: the thread waits for the
 * copy on `done`, an event of the caller that no other call in flight uses; gj_hip_download waits for the work on s first. Small copies,
 * done == NULL and the developer setting GJ_COPY_LANES=0: asynchronous on s, exactly gj_hip_memcpy_h2d / _d2h. */
GJ_HIP_API int gj_hip_upload(void* dst, const void* src, size_t n, gj_stream_t s, gj_event_t done);
GJ_HIP_API int gj_hip_download(void* dst, const void* src, size_t n, gj_stream_t s, gj_event_t done);
/* several such copies of one direction: copy with gj_hip_memcpy_h2d / _d2h on the stream gj_hip_lane_begin returns (the lane -- behind the work on s
 * when `download` -- or s itself), then gj_hip_lane_end: complete on return when that was a lane, asynchronous on s otherwise */
GJ_HIP_API gj_stream_t gj_hip_lane_begin(int download, size_t bytes_each, gj_stream_t s);
GJ_HIP_API int gj_hip_lane_end(gj_stream_t lane, gj_stream_t s, gj_event_t done);
GJ_HIP_API int gj_hip_memset(void* dst, int value, size_t n, gj_stream_t s);
GJ_HIP_API int gj_hip_stream_sync(gj_stream_t s);
/* 1 if p points to device (HBM) memory, 0 for host memory (reference: test/unit/run_tests.c:40-78) */
GJ_HIP_API int gj_hip_is_device_ptr(const void* p);

GJ_HIP_API gj_event_t gj_hip_event_create(void);
GJ_HIP_API void gj_hip_event_destroy(gj_event_t e);
GJ_HIP_API int gj_hip_event_record(gj_event_t e, gj_stream_t s);
GJ_HIP_API float gj_hip_event_elapsed_ms(gj_event_t start, gj_event_t stop); /* synchronises on stop */

/* ------------------------------------------------------------------ geometry shared by host and kernels */
#define GJ_MAX_COMP 4
#define GJ_MAX_MCU_BLOCKS 16     /* blocks per interleaved MCU we accept (JPEG itself allows 10) */
#define GJ_TEMP_BYTES_PER_BLOCK 208 /* >= worst case 1658 bits of an 8x8 block before byte stuffing, 16 B multiple */
/* gj_enc_job.d_tail (k_encode_* -> k_gather): two sets of GJ_TAIL_GROUPS_CAP(segments) group totals, used alternately, then the tile list
 * (one word per tile stream, at most one stream per segment) */
#define GJ_TAIL_GROUPS_CAP(segments) (((unsigned)(segments) + 32u) / 32u + 1u)
#define GJ_TAIL_WORDS(segments) (2u * GJ_TAIL_GROUPS_CAP(segments) + ((unsigned)(segments) + 1u))

enum { GJ_PF_U8 = 0, GJ_PF_444_P012 = 1, GJ_PF_444_P0P1P2 = 2, GJ_PF_422_P1020 = 3, GJ_PF_422_P0P1P2 = 4,
       GJ_PF_420_P0P1P2 = 5, GJ_PF_4444_P0123 = 6 };

typedef struct gj_comp_geom {
    int type;                  /* 0 luminance tables, 1 chrominance tables (encoder) */
    int samp_h, samp_v;
    int sub_h, sub_v;          /* max_h / samp_h, max_v / samp_v */
    int width, height;         /* real size */
    int data_width, data_height;
    int blocks_x, blocks_y;
    int mcu_count_x, mcu_count;
    int segment_count;         /* non-interleaved: segments of this component's scan */
    int first_segment;         /* non-interleaved: global index of its first segment */
    int q_table, dc_table, ac_table; /* decoder: table slots */
    int reserved;
    uint64_t data_offset;      /* offset in samples of the plane / coefficient plane */
} gj_comp_geom;

/* Decoder kernels of a frame batch (gj_dec_job::batch, blockIdx.z = frame): what lies between the buffers of two frames. It travels with
 * the geometry because every decoder kernel takes the geometry by value; sizes == NULL (everything zero) for a single frame. */
struct gj_geom;
typedef struct gj_frame_strides {
    const uint32_t* sizes;    /* [frames] bytes of every frame's stream, device memory */
    uint64_t jpeg, raw;       /* bytes */
    uint64_t coefs, tok, rec; /* int16 coefficients, tokens, block records */
    uint32_t seg;             /* words between the frames' seg_pos (and seg_len, seg_index) */
    uint32_t frames;          /* frames of the launch (what fills the device is the batch, not the frame: gj_hip_decode_wants_tokens) */
    /* frames of DIFFERENT image sizes (dec_opt_batch_sizes = mixed, crop-and-resize alone): [frames] the geometry of every frame, device memory; NULL:
     * all frames share the geometry this record travels in. The record of a frame is a whole gj_geom that the kernels read where it lies
     * (gj_device.h: gj_frame_geom) -- they index its components at run time, and a copy patched in registers would live in scratch memory. Its
     * own fb is not read as strides: in a batch whose frames have headers of their OWN (dec_opt_batch_headers = any, gj_batch::own_headers) it is where
     * the frame's header record lies (GJ_REC_BEGIN, GJ_REC_TABSET, GJ_REC_TABSETS below), so that neither the geometry that every decoder kernel
     * takes by value nor the per-frame record grows by a byte for it. */
    const struct gj_geom* geoms;
} gj_frame_strides;
/* The header record of a frame of such a batch, in the fb of ITS geometry record `rec` (geoms[z]):
 *   GJ_REC_BEGIN    the first byte behind the frame's first SOS header: what lies in front of it is no 0xFF and follows none for the marker scan
 *   GJ_REC_TABSET   which table set of the launch's pool (GJ_TABSET_WORDS) the frame is decoded with -- set s lies s x GJ_TABSET_WORDS words behind
 *                   the job's table pointers
 *   GJ_REC_TABSETS  the sets in the pool; the kernels clamp the index to it */
#define GJ_REC_BEGIN(rec) ((rec).fb.jpeg)
#define GJ_REC_TABSET(rec) ((rec).fb.frames)
#define GJ_REC_TABSETS(rec) ((rec).fb.seg)

typedef struct gj_geom {
    int width, height, width_padding;
    int pixel_format, color_space, color_space_internal;
    int comp_count, interleaved, restart_interval;
    int max_h, max_v;
    int mcu_count;             /* interleaved: MCUs in the scan */
    int mcu_count_x;           /* interleaved */
    int segment_count;         /* all scans */
    int scan_count;
    int blocks_per_mcu;        /* 1 when not interleaved */
    int seg_blocks;            /* blocks in a full segment (restart_interval * blocks_per_mcu; whole scan if 0) */
    int block_count;
    int raw_width;             /* width used by the pixel kernels (even for 4:2:2 packed) */
    int no_transform;          /* planar copy path: raw layout equals component layout */
    uint64_t data_size;        /* samples in all planes */
    uint64_t raw_size;
    gj_comp_geom comp[GJ_MAX_COMP];
    uint8_t mcu_comp[GJ_MAX_MCU_BLOCKS]; /* interleaved MCU layout: component of block p */
    uint8_t mcu_bx[GJ_MAX_MCU_BLOCKS];   /* block x inside the MCU */
    uint8_t mcu_by[GJ_MAX_MCU_BLOCKS];
    uint8_t mcu_prev[GJ_MAX_MCU_BLOCKS]; /* distance (in scan order) to the previous block of the same component */
    gj_frame_strides fb;       /* decoder kernels of a frame batch; all zero for a single frame */
} gj_geom;

/* ------------------------------------------------------------------ encoder */
#define GJ_CODER_LUT_OFFSET 1024 /* words of gj_enc_job::d_huff_lut in front of the coder's tables */
#define GJ_CODER_LUT_WORDS 544
/* Developer settings (A/B measurements, forced modes of the tests): process-wide values set through gj_hip_tuning_setting("NAME=VALUE") -- the names
 * in the comments below, public as gpujpeg_amd_tuning (gpujpeg_amd_ext.h) --, copied into a coder ONCE, when it is created (gj_hip_tuning_defaults);
 * the launchers see the coder's copy only. The release library does not read the environment; builds with -DGJ_TUNING_ENV (`make trace`, `make variant`,
 * the CPU execution model of tests/hipemu) also take the settings whose names are in the environment at that moment. */
typedef struct gj_tuning {
    int no_fused;        /* GPUJPEG_NO_FUSED: generic kernels only */
    int enc_split;       /* GJ_ENC_SPLIT=<tiles>: frames of up to so many tiles are coded one component per workgroup (-1: the default limit) */
    int enc_tail;        /* GJ_ENC_TAIL=<tiles>: so many of the last tiles of a frame larger than the GPU are coded one component per workgroup (-1: default 32, 0: none) */
    int dec_balance;     /* GJ_DEC_BALANCE=1: sparse frames' batches cut by estimated time so that they fill one generation (latency of a lone decode) */
    int host_timing;     /* GJ_HOST_TIMING=1: the coder prints where the host's time of its calls went when it is destroyed */
    int host_scan;       /* GPUJPEG_HOST_SCAN: the decoder walks the stream on the host like the reference */
    int enc_no_whole422; /* GJ_ENC_NO_WHOLE422: packed 4:2:2 through k_fused_uyvy422 + k_huffman instead of k_encode_uyvy422 */
    int dec_tokens;      /* GJ_DEC_TOKENS=1 -> 1 (token mode wherever a token-fed IDCT exists), GJ_DEC_NO_TOKENS -> 0, else -1 = by frame */
    int dec_serial;      /* GJ_DEC_ENTROPY=serial: lane-per-segment entropy decoder */
    int dec_batch;       /* GJ_DEC_G: segments per batch of the sub-sequence decoder, 0 = automatic */
    int dec_sub;         /* GJ_DEC_SUB: bytes per sub-sequence, 0 = automatic */
    int dec_no_spec;     /* GJ_DEC_NO_SPEC: no speculative launch on a cached header */
    int dec_seq;         /* GJ_DEC_SEQ: 1 = always the lane-per-segment entropy decoder in plane mode, 2 (GJ_DEC_SEQ=0) = never, 0 = by the frame */
    int debug_sync;      /* GJ_DEC_DEBUG_SYNC=1: wait after every decoder stage and name it on stderr */
    int scan_shape;      /* GJ_SCAN_SHAPE=<pieces * 100 + rounds>: 4 KB pieces per round (1, 2, 4, 8, 16) and rounds (1 .. 4) of a workgroup of the marker scan
                            instead of the choice by the stream's size (tests: every shape on small streams) */
    int dec_tok_nocoop;  /* GJ_DEC_TOK_NOCOOP=1: the token-mode entropy decoder copies its batch segment by segment instead of as one piece (A/B) */
    int enc_by_blocks;   /* GJ_ENC_BLOCKS: packed RGB 4:4:4 through k_encode_blocks (a workgroup codes one component of its tile: three times the
                            workgroups, a third of the work each) 1 = always, -1 = never, 0 = small frames only */
    int dec_fill;        /* GJ_DEC_FILL=<32nds>: how full the sub-sequence decoders' LDS stage is planned on average (default 23, up to 27 when that keeps
                            a single frame within one generation of workgroups); A/B runs of the batch plan */
    int enc_out_cap;     /* GJ_ENC_OUT_CAP=<bytes>: the assembly kernels and the host's checks take min(the stream buffer's size, bytes) as the output
                            capacity (0: the buffer's size); tests of the overflow guard, which no image reaches through the public API */
    int idct_dense;      /* GJ_IDCT_DENSE=1: every wave of k_idct_tok_rgb444 takes the dense body (full 8x8 transform of the chrominance blocks too); A/B
                            runs on one build, tests of the corner path */
    int dec_no_early_stop; /* GJ_DEC_NO_EARLY_STOP=1: a batch of regions on restart-less streams (dec_opt_batch_restartless) entropy-decodes every scan to its
                            end instead of leaving it behind the cover's last block (A/B runs; the bytes are the same) */
    int dec_careful;     /* set by the host for ONE call, never from the environment: a kernel that takes whole segments into LDS met one that
                            does not fit (overflow flag) -- this call uses the kernels without that limit */
} gj_tuning;
GJ_HIP_API void gj_hip_tuning_defaults(gj_tuning* t);
GJ_HIP_API int gj_hip_tuning_setting(const char* setting);          /* "NAME=VALUE" or "NAME"; NULL: back to the defaults. 0, or -1 for an unknown name */
GJ_HIP_API const char* const* gj_hip_tuning_names(int* count); /* the names gj_hip_tuning_setting knows */

/* Frame batch (MI355X extension, gpujpeg_amd_{encoder_encode,decoder_decode}_batch): `count` frames of ONE geometry, tables and header behind
 * one set of launches (blockIdx.z = frame) -- an HD frame has 135 encoder tiles for the 1024 workgroup places of the device, a batch fills
 * them. Frame f's buffers lie f x stride behind the job's pointers. count <= 1: a single frame, the strides are ignored. */
typedef struct gj_batch {
    uint32_t count;
    uint64_t raw;            /* bytes between the frames' pixels (d_raw) */
    uint64_t jpeg;           /* bytes between the frames' streams (d_jpeg) */
    uint64_t temp;           /* encoder: bytes between the frames' tile areas (d_temp) */
    uint64_t coefs;          /* decoder: int16 elements between the frames' coefficient planes */
    uint64_t tok;            /* decoder: tokens between the frames' token arrays */
    uint64_t rec;            /* decoder: block records between the frames' record arrays */
    uint32_t seg;            /* words between the frames' per-segment arrays (encoder: seg_bytes, seg_ff; decoder: each of seg_pos, seg_len, seg_index) */
    uint32_t tail;           /* encoder: words between the frames' d_tail */
    uint32_t scratch;        /* decoder: words between the frames' marker-scan scratch */
    uint32_t maxlen;         /* decoder: words between the frames' longest-segment words in pinned host memory */
    const uint32_t* d_sizes; /* decoder: [count] bytes of every frame's stream, in device memory */
    const struct gj_geom* d_geoms; /* decoder: NULL, or [count] the geometry of every frame (gj_frame_strides::geoms), in device memory */
    uint32_t own_headers;          /* decoder: 1 = every frame's geometry record carries its header record (GJ_REC_BEGIN ...; dec_opt_batch_headers = any); with d_geoms alone */
} gj_batch;

typedef struct gj_enc_job {
    gj_geom g;
    const uint8_t* d_raw;          /* input pixels in HBM */
    uint8_t* d_planes;             /* padded planar components (generic path only) */
    int16_t* d_coefs;              /* quantised coefficients, 64 per block */
    const float* d_fwd_q[2];       /* forward tables, luminance / chrominance (src/gpujpeg_table.c:103-123 layout) */
    const uint32_t* d_huff_lut;    /* [4][256]: (code << 8) | size ; order lumaDC, lumaAC, chromaDC, chromaAC; behind them, at GJ_CODER_LUT_OFFSET, the
                                      GJ_CODER_LUT_WORDS words of the fused encoders' coder: per table type AC[(run << 4) | ((16 - nbits) & 15)] (256) then DC[nbits] (16),
                                      entry = (code bits + nbits) << 26 | code << nbits (gj_huffman_coder_lut) */
    uint8_t* d_temp;               /* per-segment unstuffed bitstreams */
    uint32_t* d_seg_bytes;         /* [segment_count] unstuffed byte count */
    uint32_t* d_seg_ff;            /* [segment_count] number of 0xFF bytes */
    uint32_t* d_seg_out;           /* [segment_count + 1] final byte offset of each segment in the JPEG */
    uint8_t* d_jpeg;               /* finished stream */
    uint64_t jpeg_capacity;
    uint32_t* d_result;            /* [0] total JPEG size, [1] overflow flag */
    uint32_t* h_result;            /* optional: the same two words in pinned host memory, written by the kernel that computes them */
    uint32_t* d_tail;              /* k_encode_* -> k_gather: GJ_TAIL_WORDS(segment_count) words, see there; the group totals are zero at allocation
                                      and after every call (two sets, used alternately) */
    int tail_set;                  /* which of d_tail's two sets of group totals this call uses: alternates from call to call */
    uint64_t* d_scan_partial;      /* [ceil(segment_count / 1024)] epoch-tagged workgroup totals of the offset scan; zero at allocation */
    uint32_t epoch;                /* differs from the previous call's (and is never 0) */
    gj_tuning tune;
    const uint8_t* d_scan_hdr;     /* scan headers back to back (APP13 placeholders zeroed + SOS) */
    uint32_t scan_hdr_offset[GJ_MAX_COMP + 1];
    uint32_t scan_info_payload[GJ_MAX_COMP]; /* offset inside scan header of the first APP13 payload, 0 = none */
    uint32_t main_hdr_size;        /* bytes already placed at d_jpeg[0..) by the host */
    int segment_info;
    int use_fused;                 /* 1: fused kernels when the format allows (raw -> segment streams, or raw -> coefficients) */
    int keep_coefs;                /* 1: the caller wants the coefficient planes in d_coefs (tests): do not use the fully fused kernel */
    int flipped;                   /* enc_opt_flipped: flip the component planes vertically after the colour stage (generic path) */
    uint32_t channel_remap;        /* enc_opt_channel_remap: packed mapping, 0 = none; applied to d_raw IN PLACE before anything else */
    gj_batch batch;                /* count > 1: a batch of frames (fully fused 4:4:4 kernel only; d_result / h_result hold two words per frame) */
    /* Per-frame optimal Huffman tables (enc_opt_huffman=optimal) split a frame's encode in two calls, both through the coefficient planes:
     * GJ_ENC_STAGE_COUNT   pixels -> planes, then k_huffman_count adds the frame's symbol counts to d_huff_freq (zeroed first on the stream);
     * GJ_ENC_STAGE_CODE    planes -> k_huffman (with the tables d_huff_lut points to) -> k_scan_segments -> k_assemble (+ k_segment_info).
     * GJ_ENC_STAGE_ALL (0) is the one-call encode of every other frame. */
    int stage;
    uint32_t* d_huff_freq;         /* GJ_ENC_STAGE_COUNT: [2 table types][DC, AC][256] symbol counts */
} gj_enc_job;
enum { GJ_ENC_STAGE_ALL = 0, GJ_ENC_STAGE_COUNT = 1, GJ_ENC_STAGE_CODE = 2 };
/* 1 when gj_hip_encode takes a batch (gj_enc_job::batch.count > 1) of this job's configuration */
GJ_HIP_API int gj_hip_encode_batchable(const gj_enc_job* job);
/* 1 when gj_hip_encode codes this job through tile streams + k_gather (the launch that uses and clears gj_enc_job::tail_set's group totals) */
GJ_HIP_API int gj_hip_encode_tiles(const gj_enc_job* job);

/* events (may be NULL): 0 start, 1 after preprocess, 2 after DCT/quant (GJ_ENC_STAGE_CODE: its start), 3 after k_huffman, 4 after k_scan_segments,
 * 5 after k_assemble (+ segment info); GJ_ENC_STAGE_COUNT: 6 after DCT/quant, 7 after k_huffman_count (and nothing from 2 on) */
#define GJ_ENC_EVENTS 8
GJ_HIP_API int gj_hip_encode(const gj_enc_job* job, gj_stream_t stream, gj_event_t ev[GJ_ENC_EVENTS]);


/* ------------------------------------------------------------------ decoder */
/* A marker scan whose SECOND launch (k_marker_table: records -> segment table) has been left to gj_hip_decode (gj_hip_find_segments_deferred:
 * speculative single-frame launches). k_huffman_decode_tok derives the table entries of its batches from the scan's records itself and writes the
 * summary the host validates -- one launch and ~11 us less per decoded frame --; for any other entropy decoder gj_hip_decode launches k_marker_table
 * first, with the arguments kept here. valid = 0: the table has been written (gj_hip_find_segments). */
struct gj_scan_summary;
typedef struct gj_scan_deferred {
    int valid;
    uint32_t wgs, part_bytes;      /* scanning workgroups (<= 256) and the bytes of the stream each of them took */
    uint64_t begin, size;
    const uint32_t* recs;          /* [wgs] records, [wgs] marker lists (d_scratch of the scan) */
    const uint32_t* lists;
    uint32_t* d_seg_pos;           /* where k_marker_table writes, should it be launched after all */
    uint32_t* d_seg_len;
    uint32_t* d_seg_index;
    uint32_t max_segments;
    struct gj_scan_summary* d_summary;
    struct gj_scan_summary* h_summary; /* pinned host memory */
    uint32_t* h_maxlen_parts;      /* pinned host memory: the longest segment per scanning workgroup (table launch) or per entropy-decoder batch (folded) */
    uint32_t maxlen_capacity;
    uint32_t* maxlen_part_count;   /* host: how many of those words the launch that ran has written */
    int* folded;                   /* host, may be NULL: set to 1 by gj_hip_decode when the table launch was folded into the entropy decoder, to 0 otherwise */
} gj_scan_deferred;

/* Region-of-interest decode (dec_opt_region): the W x H pixels at (x, y) of the stream's image. The COVER of the region is, per component, the
 * smallest rectangle of 8x8 blocks -- whole MCUs of an interleaved scan -- that holds every sample the region's pixels need. */
/* origin and cover of ONE rectangle: what a single region call has once (gj_region::frame) and a batch of regions once per frame, in device
 * memory (gj_region::d_frames) */
typedef struct gj_region_frame {
    int x, y;                      /* pixels of the stream's image */
    int bx0[GJ_MAX_COMP], by0[GJ_MAX_COMP], bx1[GJ_MAX_COMP], by1[GJ_MAX_COMP]; /* cover: blocks [bx0, bx1) x [by0, by1) of the component's grid */
    int mx0, my0, mx1, my1;        /* interleaved scan: the cover in MCUs */
    int w, h;                      /* pixels of the rectangle (a crop-and-resize call: every frame has its own; the other region calls read gj_region::w / h) */
    int mirror;                    /* crop-and-resize: 1 = the resampled image is mirrored horizontally */
    /* crop-and-resize with dec_opt_resize_prescale: the cover's blocks leave N x N samples, N = 8 / scale, and the resample reads the
     * REDUCED cover planes. x, y, w, h above are then x', y', w', h' -- the rectangle's covering rectangle in the image reduced by `scale` --,
     * src_w / src_h the caller's w and h, off_x / off_y = x - scale x', y - scale y': what gj_resize_taps needs. Every other region call: scale 1,
     * src_w = w, src_h = h, offsets 0 (gj_geom_init_region). */
    int scale;                     /* 1, 2, 4 or 8 */
    int src_w, src_h, off_x, off_y;
    /* ... with dec_opt_resize_prescale_subsampled on a stream gj_geom_prescale_per_component accepts (4:2:0): 1 = the frame is reduced PER COMPONENT --
     * component c's blocks leave N_c x N_c samples, N_c = 8 sub_h / scale (1, 2, 4 or 8: the full-size IDCT), so that every reduced plane has one
     * sample per reduced pixel (k_idct_region_scaled_comp; k_resize_region reads sample x' + x, no division by sub_h). 0: every other frame */
    int per_comp;
} gj_region_frame;
/* Tensor output of crop-and-resize (gpujpeg_amd_decoder_decode_batch_crop_resize_tensor): the pixel stage stores, in place of the bytes of the pixel
 * format, element (c, j, i) = convert(float(byte) * scale[c] + bias[c]) -- two binary32 operations, each rounded to nearest even, never fused; the
 * conversion to binary16 / bfloat16 rounds to nearest even (gj_device.h: gj_tensor_element, the ONE statement of it) -- at (c OH + j) OW + i (CHW) or
 * (j OW + i) channels + c (HWC) of the frame. channels: 1 for single-channel output, 3 for packed or planar 4:4:4 (gj_geom_init_resized sets it). */
enum { GJ_TENSOR_F32 = 0, GJ_TENSOR_F16 = 1, GJ_TENSOR_BF16 = 2 };
enum { GJ_TENSOR_CHW = 0, GJ_TENSOR_HWC = 1 };
typedef struct gj_tensor {
    int on;                        /* 1: the call stores a tensor */
    int dtype, layout, channels;
    float scale[4], bias[4];       /* [3]: not used */
} gj_tensor;
#define GJ_TENSOR_ELSIZE(dtype) ((dtype) == GJ_TENSOR_F32 ? 4 : 2)
typedef struct gj_region {
    int on;                        /* 1: this call decodes a region */
    int select;                    /* 1: only the restart segments that touch the cover are entropy-decoded (k_segment_select compacts the table) */
    int w, h;                      /* pixels of the region */
    gj_region_frame frame;         /* where it lies in the stream's image, and its cover */
    int sel_count[GJ_MAX_COMP];    /* select: segments of every scan that touch the cover, as the geometry gives them (the batch plan) */
    uint32_t* d_sel;               /* select: the compacted table, three arrays of (g.segment_count + GJ_MAX_COMP) words: pos | len | index */
    uint32_t* d_sel_count;         /* select: device word, entries of the compacted table (what the entropy decoders bound their work with) */
    uint32_t* h_sel_count;         /* select: pinned host words written by k_segment_select: [0] entries of the compacted table, [1 + c] of scan c */
    /* a batch of regions (gj_dec_job::batch together with region.on: gpujpeg_amd_decoder_decode_batch_regions) -- one w x h for all frames, the
     * origin and with it the cover PER FRAME: `frame` above is not used, frame f's is d_frames[f]. select is 1.
     * sel_count[c] is the LARGEST selection of scan c among the frames: frame f's compacted table (d_sel + f x gj_frame_strides::seg words, laid out
     * like the frame's segment table) holds its own selection of scan c from entry sum(sel_count[0 .. c)) on and null entries (index 0xFFFFFFFF,
     * length 0: a segment without blocks for the entropy decoders) up to the next scan's, so that ONE batch plan serves every frame. d_sel_count is
     * not used (every compacted table has sum(sel_count) entries); h_sel_count holds GJ_MAX_COMP words per frame: the entries found per scan. */
    const gj_region_frame* d_frames; /* device memory, [gj_batch::count]; NULL: a single frame */
    /* crop-and-resize (gpujpeg_amd_decoder_decode_batch_crop_resize): the rectangle -- gj_region_frame::w x h, per frame -- is resampled to the
     * gs.width x gs.height image by the pixel stage (k_resize_region, bilinear: gj_resize_taps) instead of being copied. gs is then the geometry of
     * the OUTPUT image over the cover's planes, w / h above are not used, and the call goes through the component planes (no token mode). */
    int resize;
    /* ... and the scales (gj_region_frame::scale) among the frames of this launch, bit log2(scale): k_idct_region serves the frames of scale 1,
     * k_idct_region_scaled the others; a launch without frames for one of them is left out. Anything but 1 outside a resize job is refused. */
    unsigned scale_mask;
    /* ... and the scales among the frames of this launch that are reduced per component (gj_region_frame::per_comp; they are NOT in scale_mask):
     * k_idct_region_scaled_comp serves them, and is left out where there are none. Anything but 0 outside a resize job is refused. */
    unsigned comp_mask;
    /* ... and what the pixel stage of a resize job stores: tensor.on = 0 the bytes of gs's pixel format (k_resize_region), 1 the tensor
     * (k_resize_region_tensor; gs.raw_size is then the tensor's size) */
    gj_tensor tensor;
    /* ... and the filter of the resample (dec_opt_resize_filter): GJ_RESIZE_FILTER_BILINEAR the four taps of k_resize_region, GJ_RESIZE_FILTER_ANTIALIAS
     * the triangle filter of k_resize_region_aa (gj_device.h: gj_resize_aa_taps) over frames of scale 1 -- with a prescaled frame, or outside a
     * resize job, anything but BILINEAR is refused */
    int filter;
    /* ... and, a batch of regions (d_frames) launched with gj_dec_job::batch_restartless: pinned host words, or NULL. h_sel_bytes[frame]: the sum of the
     * table lengths of the entries the frame's selection found (k_segment_select_batch) -- what the entropy decoder is handed. h_left_early[frame x
     * GJ_MAX_COMP + scan]: the bytes of a restart-less scan k_huffman_decode_par did NOT read because the cover's last block had been decoded (the
     * host zeroes the words before the launch; NULL: every scan is decoded to its end) */
    uint32_t* h_sel_bytes;
    uint32_t* h_left_early;
} gj_region;
enum { GJ_RESIZE_FILTER_BILINEAR = 0, GJ_RESIZE_FILTER_ANTIALIAS = 1 };
/* the predicate of the selection (gj_device.h: gj_segment_in_cover) for host code: does restart segment s have a block / an MCU inside the cover?
 * (the decoder's own plan does not call it: gj_region_plan counts in closed form) */
GJ_HIP_API int gj_hip_segment_in_cover(const gj_geom* g, const gj_region* r, int s);
/* the bits k_resize_region_tensor stores for byte v (0 .. 255) of channel c (gj_device.h: gj_tensor_element) for host code */
GJ_HIP_API uint32_t gj_hip_tensor_element(const gj_tensor* t, int c, int v);
/* the taps k_resize_region_aa gives output sample i of n_out along an axis of n_src source samples (gj_device.h: gj_resize_aa_taps, _weight) for host
 * code: first tap, tap count, the weights (NULL: not wanted) and their sum. -1: arguments the call refuses (sizes, i, n_src > 256 n_out), -2: capacity < count */
GJ_HIP_API int gj_hip_resize_aa_weights(int n_src, int n_out, int i, int* first, int* count, uint32_t* weights, int capacity, uint64_t* sum);

/* Progressive streams (SOF2, dec_opt_progressive): the work list of k_huffman_decode_prog, ONE WAVE PER RECORD. A record is one restart segment of
 * one scan and says everything the wave needs -- no record refers to a frame: where its blocks lie is given per component as the block index of the
 * plane's first block in d_coefs and the plane's pitch in blocks, so that a chunk of frames (gj_prog_frame, below) only adds a plane base per record's frame.
 * A scan of one component (every AC scan, a DC scan of one component) codes the ceil(w_c / 8) x ceil(h_c / 8) blocks of the component in raster
 * order (`across` of them per row) inside the plane's pitch; a DC scan of several components codes whole MCUs of the FRAME's grid (`across` MCUs
 * per row), component c's h x v blocks of every MCU. first / count: blocks of the first kind of scan, MCUs of the second. */
enum { GJ_PROG_DC_FIRST = 0, GJ_PROG_DC_REFINE = 1, GJ_PROG_AC_FIRST = 2, GJ_PROG_AC_REFINE = 3 };
typedef struct gj_prog_comp {
    uint32_t base;                 /* block index (64 coefficients each) of the component plane's first block */
    uint32_t pitch;                /* blocks per row of the plane */
    uint16_t table;                /* entry of the table pool: the DC table of a first DC scan, the AC table of an AC scan */
    uint8_t h, v;                  /* blocks per MCU (scans of several components) */
} gj_prog_comp;
typedef struct gj_prog_rec {
    uint32_t pos, len;             /* the segment's entropy-coded bytes in the stream */
    uint32_t first, count;         /* first block / MCU of the segment and how many it codes */
    uint32_t across;               /* coded blocks / MCUs per row */
    uint8_t kind, ncomp, ss, se, ah, al;
    uint16_t frame;                /* a chunk of frames (gj_prog_plan::d_frames): the record's frame in the chunk; a single frame: 0, not read */
    gj_prog_comp c[GJ_MAX_COMP];
} gj_prog_rec;
/* A chunk of progressive frames behind ONE set of launches (dec_opt_batch_progressive, k_huffman_decode_prog_batch): what a record's frame number
 * stands for. pos / len of the frame's records stay relative to the frame's OWN stream -- a 32-bit offset into a staging area of 256 streams is not
 * safe --, the table numbers of its records count from tab_first, their block numbers from coef_block; the kernel clamps positions to `size`, table
 * numbers to the whole pool and block numbers to the frame's own planes. The frames of one chunk share the geometry: frames of different image sizes
 * are different launches (per-frame geometry for progressive frames is not built). */
typedef struct gj_prog_frame {
    uint64_t stream;               /* bytes from gj_dec_job::d_jpeg to the frame's stream */
    uint32_t size;                 /* bytes of the stream */
    uint32_t tab_first;            /* first entry of the frame's tables in the pool */
    uint64_t coef_block;           /* block index of the frame's planes in gj_dec_job::d_coefs: frame number in the chunk x gj_frame_strides::coefs / 64 */
} gj_prog_frame;
/* the plan of a progressive frame: scans whose coefficients do not depend on each other form a LEVEL and are launched together, the levels one
 * after the other on the stream (gj_decoder.c: the level of a scan is 1 + the highest level among the earlier scans that share a component and
 * a coefficient with it). Records of a level lie back to back. */
#define GJ_PROG_MAX_SCANS 64
typedef struct gj_prog_plan {
    const gj_prog_rec* d_recs;     /* device memory */
    const uint16_t* d_tabs;        /* device memory: the table pool, GJ_DEC_TAB_WORDS words per entry */
    uint32_t tab_count;
    int levels;
    uint32_t level_first[GJ_PROG_MAX_SCANS], level_count[GJ_PROG_MAX_SCANS];
    /* a chunk of frames: device memory, [gj_batch::count] (NULL: a single frame). Level l is then level l of ALL the chunk's frames, its records in
     * descending order of len -- the longest serial walks start first --, and `levels` the deepest frame's */
    const gj_prog_frame* d_frames;
} gj_prog_plan;

typedef struct gj_dec_job {
    gj_geom g;                     /* pixel_format / color_space describe the requested output */
    const uint8_t* d_jpeg;         /* whole file in HBM */
    uint64_t jpeg_size;
    const uint32_t* d_seg_pos;     /* [seg_count] byte offset of each segment's entropy data */
    const uint32_t* d_seg_len;     /* [seg_count] */
    const uint32_t* d_seg_index;   /* [seg_count] geometric segment index */
    int seg_count;                 /* number of table entries (upper bound when d_seg_count is set) */
    const uint32_t* d_seg_count;   /* optional: actual count in device memory (written by gj_hip_find_segments) */
    const uint16_t* d_huff_tab;    /* [4 slots][2 classes][GJ_DEC_TAB_WORDS] decode tables */
    const uint16_t* d_huff_tab2;   /* [2 slots][2 classes][GJ_DEC2_WORDS] two-level tables of the sub-sequence decoder, or NULL when the
                                      stream's tables do not fit them (then only the lane-per-segment kernel runs) */
    const uint16_t* d_qtab;        /* [4][64] natural order */
    const float* d_qtabf;          /* the same as float: what the IDCT kernels multiply with */
    int16_t* d_coefs;
    uint8_t* d_planes;
    uint8_t* d_raw;                /* output pixels */
    int use_fused;
    int flipped;                   /* dec_opt_flipped: flip the component planes before the colour stage (generic path) */
    uint32_t channel_remap;        /* dec_opt_channel_remap: applied to the finished image in d_raw */
    int clear_coefs;               /* 1: d_coefs is not known to be all zero, clear it first */
    int zero_coefs;                /* 1: the IDCT kernels zero every block after reading it (next call may skip clear_coefs) */
    gj_tuning tune;
    uint32_t max_seg_len;          /* longest restart segment of the stream when known (see scan_bytes), 0 = unknown */
    uint32_t* d_overflow;          /* one word the entropy decoders that take whole segments into LDS (k_huffman_decode_tok, _seq) set when they
                                      meet a segment they cannot stage */
    uint32_t scan_bytes[GJ_MAX_COMP]; /* entropy-coded bytes of every scan when known (this stream's, or the previous frame's on the speculative
                                         path; 0 = unknown): the entropy decoder sizes its batches per scan with them */
    /* token mode: entropy decoder -> fused IDCT without the coefficient planes (used when a token-fed IDCT kernel exists for the
     * configuration; 0 / NULL = planes) */
    int tokens;
    uint16_t* d_tok;               /* [tok_cap + 64] 16-bit tokens: value << 6 | natural position; the run of a decoder group starts at token
                                      4 x the byte offset of its first segment */
    uint32_t tok_cap;              /* >= 4 x jpeg_size (tokens) */
    void* d_blkrec;                /* [g.block_count] uint2 per block in coding order: first token, count << 16 | (uint16) DC term;
                                      count 0xFFFF = the block is in d_coefs (segment decoded piece by piece) */
    gj_scan_deferred scan;         /* valid: the segment table has not been written yet (see gj_scan_deferred) */
    gj_batch batch;                /* count > 1: a batch of frames with the same header (speculative launches only: d_seg_count and d_overflow
                                      point to frame 0's words inside arrays of gj_scan_summary) */
    /* reduced-size decode (dec_opt_scale): scale = 2, 4, 8 (0 or 1: full size). The entropy decoders work on g as ever; the IDCT side leaves
     * 8 / scale samples per block edge and the pixel kernels behind it work on gs, the geometry of the reduced image (gj_geom_init_scaled: d_planes
     * holds the reduced planes, d_raw the reduced image). No flip. A single frame, or a batch of frames (gj_dec_job::batch): frame z's reduced planes
     * lie z x gj_frame_strides::coefs bytes into d_planes -- the full-size planes' stride --, its reduced image z x gj_frame_strides::raw bytes into
     * d_raw, and gs.fb = g.fb. */
    int scale;
    gj_geom gs;
    int* idct_path;                /* host, may be NULL: which IDCT side ran -- 0 full size, 1 k_idct_scaled, 2 k_idct_tok_scaled_rgb444, 3 k_idct_region, 4 k_idct_tok_region_rgb444,
                                      5 k_idct_region + k_resize_region (crop-and-resize), 6 the same with a frame through k_idct_region_scaled (dec_opt_resize_prescale),
                                      7 k_idct_region + k_resize_region_aa (dec_opt_resize_filter = antialias),
                                      8 5 with a frame through k_idct_region_scaled_comp (dec_opt_resize_prescale_subsampled) */
    /* region decode (dec_opt_region, region.on): the entropy decoders work on g -- with region.select on the compacted table --, the IDCT side
     * transforms the cover's blocks -- from tokens straight into d_raw, or into cover-sized planes in d_planes from which the region's pixels go to d_raw --; gs is the geometry of the W x H image
     * with the cover's planes (gj_geom_init_region). No scale, no flip. A single frame, or (region.d_frames) a batch of frames with one
     * rectangle each: gs then holds the planes of the LARGEST cover of the batch -- per component the widest and the highest one --, every frame's
     * cover planes are laid out like that (gj_frame_strides::coefs bytes apart in d_planes) and gs.fb = g.fb. */
    gj_region region;
    /* dec_opt_batch_restartless: 1 = a batch (gj_dec_job::batch) of streams WITHOUT restart markers is taken -- one segment per scan, decoded piece
     * by piece by k_huffman_decode_par, plane mode -- and a batch of regions on them selects every segment. 0: gj_hip_decode_batchable says no */
    int batch_restartless;
    /* a progressive frame (host memory, NULL: a baseline frame): the coefficient planes are cleared and filled by k_huffman_decode_prog, one launch
     * per level, in place of the entropy decoders above -- no segment table, no tokens, no selection --; the IDCT side is the plane route's.
     * With gj_dec_job::batch (and gj_prog_plan::d_frames): a chunk of progressive frames of one geometry and one set of quantisation tables -- the
     * chunk's planes cleared once, one k_huffman_decode_prog_batch launch per level, then the IDCT side exactly as a baseline batch has it (full size,
     * scale, a batch of regions -- WITHOUT a selection: every segment is decoded --, crop-and-resize). Nothing but d_jpeg, d_coefs, d_planes, d_raw,
     * d_qtab / d_qtabf, g / gs with their fb, batch.count, scale and region is read. */
    const gj_prog_plan* prog;
} gj_dec_job;
/* 1 when gj_hip_decode takes a batch (gj_dec_job::batch.count > 1) of this job's configuration */
GJ_HIP_API int gj_hip_decode_batchable(const gj_dec_job* job);
/* 1 when the IDCT side of this configuration goes through the component planes (gj_dec_job::d_planes; a batch needs a set per frame,
 * gj_frame_strides::coefs bytes apart) */
GJ_HIP_API int gj_hip_decode_uses_planes(const gj_geom* g, int use_fused);

/* 1 when a frame of this geometry (requested output included) and stream size is decoded in token mode: a token-fed IDCT kernel
 * exists for it and the measured size / density rule (or the GJ_DEC_TOKENS / GJ_DEC_NO_TOKENS override) says so. The host asks
 * before it allocates d_tok / d_blkrec. */
GJ_HIP_API int gj_hip_decode_wants_tokens(const gj_geom* g, uint64_t jpeg_size, const gj_tuning* tune);

/* decode table layout per (slot, class): 1024 fast entries (len << 8 | symbol, 0 = miss) followed by
 * maxcode[18] (as u16 pairs lo/hi), valptr[17], mincode[17] and the 256 symbol values */
#define GJ_DEC_FAST_BITS 10
#define GJ_DEC_TAB_WORDS (1024 + 36 + 17 + 34 + 256 + 1)

/* two-level table of the sub-sequence decoder: 1024 first-level entries indexed by the next 10 bits, then up to
 * GJ_DEC2_SUBTABLES second-level tables of 64 entries indexed by the 6 bits after those. Entry: bits [0,5) code length +
 * magnitude bits (0 in the first level = go to the second level, whose word offset is entry >> 5), [5,9) magnitude bits,
 * [9,15) zig-zag advance (DC: 1 + high nibble; AC: run + 1, 16 for ZRL, 63 for EOB: the position inside a block is >= 1, so
 * the block is complete at >= 64), bit 15 set for a non-zero AC coefficient (what the token decoder counts and stores). */
#define GJ_DEC2_SUBTABLES 6
#define GJ_DEC2_WORDS (1024 + 64 * GJ_DEC2_SUBTABLES)

/* A table set: what the batched kernels read for ONE header, in the order the decoder's own table block holds it behind gj_dec_job::d_qtab -- the
 * four uint16 inverse quantisation tables (natural order), the four two-level Huffman tables [2 slots][2 classes], the four float quantisation
 * tables. A pool of them (gj_batch::own_headers, GJ_REC_TABSET) lies GJ_TABSET_WORDS uint16 words apart: d_qtab, d_huff_tab2 and d_qtabf of the job point
 * into set 0. A multiple of 8 words, so that every set is read with 16-byte loads. */
#define GJ_TABSET_TAB2_OFFSET (4 * 64)
#define GJ_TABSET_QF_OFFSET (GJ_TABSET_TAB2_OFFSET + 4 * GJ_DEC2_WORDS)
#define GJ_TABSET_WORDS (GJ_TABSET_QF_OFFSET + 4 * 64 * 2)

/* events (may be NULL): 0 start, 1 after Huffman, 2 after IDCT, 3 after postprocess */
#define GJ_DEC_EVENTS 4
GJ_HIP_API int gj_hip_decode(const gj_dec_job* job, gj_stream_t stream, gj_event_t ev[GJ_DEC_EVENTS]);

/* Device-side segment discovery: finds RSTn and scan boundaries in the device-resident stream [begin, size) and
 * writes the segment table (offset, length, geometric index) in stream order. The small summary is what the host
 * reads back to validate the structure (and to learn the segment count). Replaces the host memchr walk of
 * src/gpujpeg_reader.c:1039-1155. */
#define GJ_SCAN_MAX_OTHER 16
typedef struct gj_scan_summary {
    uint32_t rst_count;                       /* RSTn markers found */
    uint32_t other_count;                     /* every other marker (SOS of later scans, EOI, ...) */
    uint32_t other_pos[GJ_SCAN_MAX_OTHER];
    uint8_t other_code[GJ_SCAN_MAX_OTHER];
    uint8_t other_bytes[GJ_SCAN_MAX_OTHER][16]; /* the 16 bytes after each of them (length + start of the payload) */
    uint32_t other_after[GJ_SCAN_MAX_OTHER];  /* RSTn markers behind it inside its workgroup's part of the stream */
    uint32_t scan_count, segment_count;
    uint32_t status;                          /* 1 = clean (scans ... EOI), 2 = unexpected marker between scans, 3 = no EOI */
    uint32_t scan_start[GJ_MAX_COMP], scan_end[GJ_MAX_COMP];
    uint32_t header_differs;                  /* 1 when the stream does not start with the cached header (speculative launches) */
    uint32_t max_seg_len;                     /* longest segment of the table (filled in by the host from the per-chunk maxima) */
    uint32_t seq_overflow;                    /* set by k_huffman_decode_tok / _seq: a segment did not fit the LDS stage, decode the frame with the other kernel */
    uint32_t rst_irregular;                   /* an RSTn out of sequence, or an empty segment in front of the end of a scan: the reference reader
                                                 resynchronises / drops it (src/gpujpeg_reader.c:1074-1135), so the host walks such a stream */
} gj_scan_summary;

GJ_HIP_API size_t gj_hip_find_segments_scratch_words(uint64_t begin, uint64_t size, uint32_t max_segments);
/* d_scratch: gj_hip_find_segments_scratch_words() words (the workgroups' records and marker lists between the two launches);
 * d_summary: the device's copy, of which only segment_count is written (speculative launches read it).
 * d_hdr_ref (may be NULL): the cached header of a speculative launch; sets h_summary->header_differs = (d_jpeg[0..hdr_n) != d_hdr_ref[0..hdr_n))
 * h_summary, h_maxlen_parts: PINNED HOST memory the kernels write directly (no copy launches behind them): the summary the host validates
 * once the stream has been waited for (the host clears rst_irregular, seq_overflow and header_differs in it before the launch; max_seg_len
 * is not written by the device: the longest segment of the table is the maximum over *maxlen_part_count words of h_maxlen_parts, one per
 * workgroup) */
GJ_HIP_API int gj_hip_find_segments(const gj_geom* g, const uint8_t* d_jpeg, uint64_t begin, uint64_t size, uint32_t* d_seg_pos,
                                    uint32_t* d_seg_len, uint32_t* d_seg_index, uint32_t max_segments, uint32_t* d_scratch,
                                    gj_scan_summary* d_summary, const uint8_t* d_hdr_ref, uint32_t hdr_n, gj_scan_summary* h_summary,
                                    uint32_t* h_maxlen_parts, uint32_t maxlen_capacity, uint32_t* maxlen_part_count, gj_stream_t stream,
                                    const gj_tuning* tune);
/* The same for the frames of a batch (batch->count streams with the same header: begin, and d_hdr_ref compared with every one of them): `size` is
 * the LONGEST stream, batch->d_sizes the streams' sizes, batch->jpeg / seg / scratch / maxlen the strides of d_jpeg, the three tables, d_scratch
 * and h_maxlen_parts; d_summary and h_summary are arrays of batch->count summaries. batch->jpeg must be a multiple of 16. */
GJ_HIP_API int gj_hip_find_segments_batch(const gj_geom* g, const uint8_t* d_jpeg, uint64_t begin, uint64_t size, uint32_t* d_seg_pos,
                                          uint32_t* d_seg_len, uint32_t* d_seg_index, uint32_t max_segments, uint32_t* d_scratch,
                                          gj_scan_summary* d_summary, const uint8_t* d_hdr_ref, uint32_t hdr_n, gj_scan_summary* h_summary,
                                          uint32_t* h_maxlen_parts, uint32_t maxlen_capacity, uint32_t* maxlen_part_count, gj_stream_t stream,
                                          const gj_tuning* tune, const gj_batch* batch);
/* gj_hip_find_segments for ONE frame whose table launch may be left to gj_hip_decode: launches k_marker_scan, and k_marker_table only when the scan has
 * more than 256 workgroups (streams beyond 16 MB); otherwise *defer describes the pending launch (defer->valid = 1) for gj_dec_job::scan. The caller must
 * decode with that job on the same stream next -- nothing else writes the table. */
GJ_HIP_API int gj_hip_find_segments_deferred(const gj_geom* g, const uint8_t* d_jpeg, uint64_t begin, uint64_t size, uint32_t* d_seg_pos,
                                             uint32_t* d_seg_len, uint32_t* d_seg_index, uint32_t max_segments, uint32_t* d_scratch,
                                             gj_scan_summary* d_summary, const uint8_t* d_hdr_ref, uint32_t hdr_n, gj_scan_summary* h_summary,
                                             uint32_t* h_maxlen_parts, uint32_t maxlen_capacity, uint32_t* maxlen_part_count, gj_stream_t stream,
                                             const gj_tuning* tune, gj_scan_deferred* defer);
/* The first n bytes of each of `frames` device-resident streams (`stride` bytes apart, d_sizes: their sizes in device memory) into PINNED HOST memory,
 * stream z's at h_out + z n, zero behind a stream's end; valid once the stream has been waited for. One launch for all of them. */
GJ_HIP_API int gj_hip_gather_headers(const uint8_t* d_jpeg, uint64_t stride, const uint32_t* d_sizes, uint32_t frames, uint32_t n, uint8_t* h_out,
                                     gj_stream_t stream);
/* workgroups the marker scan cuts [begin, size) into at most (capacity of h_maxlen_parts) */
GJ_HIP_API size_t gj_hip_find_segments_max_chunks(uint64_t begin, uint64_t size);

#ifdef __cplusplus
}
#endif
#endif
