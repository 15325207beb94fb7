/*
 * gj_internal.h -- host-side state of the MI355X libgpujpeg implementation (plain C11).
 * The host never sees HIP types: everything device-related goes through include/gj_hip.h.
 */
#ifndef GJ_INTERNAL_H
#define GJ_INTERNAL_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "gj_hip.h"
#include "libgpujpeg/gpujpeg_common.h"
#include "libgpujpeg/gpujpeg_decoder.h"
#include "libgpujpeg/gpujpeg_encoder.h"
#include "libgpujpeg/gpujpeg_type.h"
#include "libgpujpeg/gpujpeg_version.h"

/* ---- logging, same prefixes as the reference (src/gpujpeg_common_internal.h:131-150) ---- */
extern const char* gj_fg_red;
extern const char* gj_fg_yellow;
extern const char* gj_term_reset;
void gj_init_term_colors(void);
#define GJ_ERROR(...) (fprintf(stderr, "%s[GPUJPEG] [Error]%s ", gj_fg_red, gj_term_reset), fprintf(stderr, __VA_ARGS__))
#define GJ_WARN(...) (fprintf(stderr, "%s[GPUJPEG] [Warning]%s ", gj_fg_yellow, gj_term_reset), fprintf(stderr, __VA_ARGS__))
#define GJ_VERBOSE(level, ...) ((level) >= GPUJPEG_LL_VERBOSE ? (void)(fprintf(stderr, "[GPUJPEG] [Verbose] "), fprintf(stderr, __VA_ARGS__)) : (void)0)
#define GJ_DEBUG(level, ...) ((level) >= GPUJPEG_LL_DEBUG ? (void)(fprintf(stderr, "[GPUJPEG] [Debug] "), fprintf(stderr, __VA_ARGS__)) : (void)0)

enum { GJ_LUMA = 0, GJ_CHROMA = 1 };

/* ---- pixel formats (src/gpujpeg_common.c:130-151) ---- */
int gj_pixfmt_unit_size(enum gpujpeg_pixel_format pf);
const struct gpujpeg_component_sampling_factor* gj_pixfmt_sampling(enum gpujpeg_pixel_format pf);
int gj_pixfmt_is_interleaved(enum gpujpeg_pixel_format pf);
gpujpeg_sampling_factor_t gj_make_sampling_factor(int comp_count, const struct gpujpeg_component_sampling_factor* sf);
int gj_parse_channel_remap(unsigned* out, const char* val, const char* optname); /* src/gpujpeg_encoder.c:661-699 */
bool gj_parameters_equal(const struct gpujpeg_parameters* a, const struct gpujpeg_parameters* b);
bool gj_image_parameters_equal(const struct gpujpeg_image_parameters* a, const struct gpujpeg_image_parameters* b);

/* ---- geometry (src/gpujpeg_common.c:675-870, 1040-1085) ---- */
int gj_geom_init(gj_geom* g, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image, bool encoder);
/* geometry and image parameters of the reduced image of a decode at scale 1/s (s = 2, 4, 8); -1 when the output format has no such image */
int gj_geom_init_scaled(gj_geom* gs, const gj_geom* full, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image, int s,
                        unsigned alignment, struct gpujpeg_image_parameters* param_image_scaled);
/* region decode (dec_opt_region): region[4] = x, y, w, h validated against the stream's image and the output format; r: the rectangle and its cover;
 * gr: the geometry of the w x h image whose component planes are the cover's; -1 (with a message) when the region is refused */
int gj_geom_init_region(gj_geom* gr, gj_region* r, const gj_geom* full, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                        const int region[4], unsigned alignment, struct gpujpeg_image_parameters* pi_region);
/* crop-and-resize: the geometry of the out_w x out_h image over the component planes of `cover` (from gj_geom_init_region; go may be cover itself);
 * -1 (with a message) for an output size outside 1 .. 16384 or an output format whose pixels share samples. tensor (NULL or on = 0: none): the call
 * stores a tensor -- its channel count is set, go->raw_size becomes the tensor's byte size, a format other than u8 / packed / planar 4:4:4 is refused */
int gj_geom_init_resized(gj_geom* go, const gj_geom* cover, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                         int out_w, int out_h, unsigned alignment, gj_tensor* tensor, struct gpujpeg_image_parameters* pi_out);
/* dec_opt_resize_prescale: the scale and covering rectangle of one crop-and-resize frame (out = s, x', y', w', h'; -1 where the call refuses), and
 * that plan applied to what gj_geom_init_region + gj_geom_init_resized made for the caller's rectangle `rect` (s > 1: the expanded cover, the frame's record;
 * r->tensor is kept and the new geometry sized with it) */
int gj_crop_resize_plan(int image_w, int image_h, int all_components_1x1, const int rect[4], int out_w, int out_h, int max_scale, int out[5]);
/* (subsampled: dec_opt_resize_prescale_subsampled -- non-zero: a stream gj_geom_prescale_per_component accepts is planned like an all-1x1 one and its
 * frames of s > 1 are reduced per component, gj_region_frame::per_comp) */
int gj_region_prescale(gj_geom* go, gj_region* r, const gj_geom* full, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                       const int rect[4], int out_w, int out_h, int max_scale, int subsampled, unsigned alignment, struct gpujpeg_image_parameters* pi_out);
/* a rectangle of a stream's DISPLAY image (the image_w x image_h image turned clockwise by `rot` quarter turns, then mirrored left-right if `flip`)
 * -> out = x', y', w', h' (its pre-image in the stored image), OW', OH' (out_w x out_h, swapped for odd rot), the bits that turn the resample of the
 * pre-image into the display-oriented result (mirror folded in), 0; -1 for a rectangle outside the display image or an output size outside 1 .. 16384 */
#define GJ_ORIENT_FX 1 /* reverse the columns of R' */
#define GJ_ORIENT_FY 2 /* reverse its rows */
#define GJ_ORIENT_T 4  /* swap the output axes */
int gj_orientation_plan(int image_w, int image_h, int rot, int flip, const int rect[4], int out_w, int out_h, int mirror, int out[8]);
/* 1 for a stream dec_opt_resize_prescale_subsampled reduces per component: every component sub_h == sub_v in {1, 2}, at least one 2, and no
 * component less subsampled than the one ahead of it (the reduced planes lie at data_offset N_c^2 / 64: they would overlap otherwise) */
int gj_geom_prescale_per_component(const gj_geom* full);
/* the ONE plan of a region call, single frame or frame f of a batch: the three steps above in that order (resize == NULL: a plain region, the first
 * step alone), r->resize / frame.mirror / tensor set, and r->sel_count[sc] = restart segments of scan sc that touch the cover (1 without a restart
 * interval: the scan's one segment, which gj_segment_in_cover always takes). -1: the rectangle was refused, -2: the resize was; either with the step's own message */
struct gj_resize { int out_w, out_h, mirror, prescale; gj_tensor tensor; int filter; int subsampled; }; /* prescale: dec_opt_resize_prescale; tensor.on = 0: the bytes of the pixel format;
                                                                                           filter: dec_opt_resize_filter (GJ_RESIZE_FILTER_*; antialias: -3 with a message
                                                                                           for a rectangle more than 256 times the output along an axis, or with a prescale);
                                                                                           subsampled: dec_opt_resize_prescale_subsampled (0 / 1) */
int gj_region_plan(gj_geom* gr, gj_region* r, const gj_geom* full, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                   const int rect[4], const struct gj_resize* resize, unsigned alignment, struct gpujpeg_image_parameters* pi_out);

/* ---- tables ---- */
extern const uint8_t gj_zigzag[64];
void gj_quant_table_raw(int type, int quality, uint8_t raw_zigzag[64]);                       /* src/gpujpeg_table.c:35-100 */
void gj_quant_table_forward(const uint8_t raw_zigzag[64], float fwd[64]);                    /* src/gpujpeg_table.c:103-123 */
void gj_quant_table_inverse(const uint8_t raw_zigzag[64], uint16_t inv[64]);                 /* src/gpujpeg_table.c:154-160 */
void gj_huffman_std_spec(int type, int is_ac, const uint8_t** bits17, const uint8_t** vals, int* count); /* :190-254 */
/* Huffman tables of an encoded frame, [table type][DC, AC]: BITS[1..16] and HUFFVAL (enc_opt_huffman=optimal; NULL where a function takes
 * one = the typical tables of Annex K.3) */
struct gj_huff_spec {
    uint8_t bits[2][2][17];
    uint8_t vals[2][2][256];
};
void gj_huffman_spec_table(const struct gj_huff_spec* spec, int type, int is_ac, const uint8_t** bits17, const uint8_t** vals, int* count);
void gj_huffman_encoder_lut(const struct gj_huff_spec* spec, uint32_t lut[GJ_CODER_LUT_OFFSET + GJ_CODER_LUT_WORDS]); /* src/gpujpeg_huffman_gpu_encoder.cu:958-969 */
int gj_huffman_optimal(const uint32_t freq[256], uint8_t bits17[17], uint8_t vals[256]); /* ITU T.81 K.2 + the decoder-fit rule; returns the length limit used */
int gj_huffman_decoder_table(const uint8_t bits17[17], const uint8_t* vals, uint16_t out[GJ_DEC_TAB_WORDS]); /* src/gpujpeg_table.c:384-449 */
int gj_huffman_decoder_table2(const uint8_t bits17[17], const uint8_t* vals, int is_ac, uint16_t out[GJ_DEC2_WORDS]);

/* ---- timers: hipEvents around the stages (src/gpujpeg_common_internal.h:156-205) ---- */
struct gj_timers {
    gj_event_t ev[GJ_ENC_EVENTS];
    /* [0] is recorded in front of every host <-> device copy of a call whether or not statistics are wanted: with an event record in front of
     * the upload AND one in front of the download the HIP runtime overlaps the copies of concurrent coders (8K, four pipelines, pinned buffers both
     * ways: 10.6 against 8.3 Gpix/s; one of the two alone changes nothing; measured in round 4, profiles/r4_08_copy_markers.txt). */
    gj_event_t copy_in[2], copy_out[2];
    /* what the calling thread waits for behind a copy through the process's copy lanes (gj_hip_upload / gj_hip_download) */
    gj_event_t lane_in, lane_out;
    bool valid;
};

/* ---- coder state shared by encoder and decoder ---- */
struct gj_coder {
    struct gpujpeg_parameters param;
    struct gpujpeg_image_parameters param_image;
    gj_geom geom;
    bool configured;
    gj_stream_t stream;
    int device;
    /* device buffers */
    uint8_t* d_raw_own; size_t d_raw_cap;
    uint8_t* d_planes; size_t d_planes_cap;
    int16_t* d_coefs; size_t d_coefs_cap;
    /* statistics (src/gpujpeg_common.c:2170-2254) */
    struct gj_timers timers;
    struct gpujpeg_duration_stats stats;
    float kernel_ms[8]; /* per-kernel durations of the last call (include/gpujpeg_amd_ext.h) */
    double start_time, init_end_time, stop_time;
    double first_frame_duration, aggregate_duration;
    long frames;
    bool encoder;
    /* GJ_HOST_TIMING=1 (developer switch): where the host's time of a call goes -- [0] entry -> first launch, [1] the launches, [2] waiting for the
     * stream, [3] behind the wait; printed when the coder is destroyed */
    bool ht_on;
    double ht[4], ht_mark;
    long ht_calls;
};
#define GJ_HT_START(c) do { if ((c)->ht_on) (c)->ht_mark = gj_now_us(); } while (0)
#define GJ_HT(c, i) do { if ((c)->ht_on) { const double t_ = gj_now_us(); (c)->ht[i] += t_ - (c)->ht_mark; (c)->ht_mark = t_; } } while (0)
double gj_now_us(void);

void gj_coder_process_stats(struct gj_coder* c, bool with_stats);
void gj_coder_process_stats_overall(struct gj_coder* c);
int gj_timers_create(struct gj_timers* t);
void gj_timers_destroy(struct gj_timers* t);
int gj_ensure_device_buffer(void** p, size_t* cap, size_t need);
int gj_ensure_pinned_buffer(void** p, size_t* cap, size_t need, size_t grow_to); /* grow_to >= need: what a buffer that has to grow is replaced by */
int gj_channel_remap_check(unsigned remap, enum gpujpeg_pixel_format pixel_format);

/* ---- writer (src/gpujpeg_writer.c) ---- */
struct gj_scan_headers {
    uint8_t* bytes;             /* all scan headers back to back */
    size_t size;
    uint32_t offset[GJ_MAX_COMP + 1];
    uint32_t info_payload[GJ_MAX_COMP];
};
struct gj_exif_tags; /* user Exif tags (enc_exif_tag), gj_writer.c */
int gj_exif_add_tag(struct gj_exif_tags** tags, const char* cfg); /* 0 = added, -1 = error or "help" */
void gj_exif_tags_destroy(struct gj_exif_tags* tags);
size_t gj_write_main_header(uint8_t* out, size_t out_cap, const gj_geom* g, const struct gpujpeg_parameters* param, enum gpujpeg_header_type header_type,
                            const uint8_t qraw[2][64], const struct gpujpeg_image_metadata* metadata, const struct gj_exif_tags* exif_tags,
                            const struct gj_huff_spec* huff /* NULL: Annex K.3 */);
int gj_write_scan_headers(struct gj_scan_headers* sh, const gj_geom* g, const struct gpujpeg_parameters* param);

/* ---- raster file formats behind gpujpeg_image_load_from_file / save_to_file (gj_image_io.c, gj_image_png.c) ---- */
struct gj_raster { int w, h, comps; uint8_t* px; }; /* top-down, tightly packed, comps interleaved 8-bit channels; px is malloc'ed */
int gj_png_decode(const uint8_t* d, size_t n, struct gj_raster* out, int want_pixels);
int gj_gif_decode(const uint8_t* d, size_t n, struct gj_raster* out, int want_pixels);
int gj_png_save(const char* filename, const uint8_t* image, int w, int h, int comps, size_t pitch);

/* ---- reader (src/gpujpeg_reader.c) ---- */
struct gj_reader_result {
    struct gpujpeg_parameters param;
    struct gpujpeg_image_parameters param_image;
    enum gpujpeg_header_type header_type;
    enum gpujpeg_color_space header_color_space;
    uint8_t comp_id[GJ_MAX_COMP];
    int quant_map[GJ_MAX_COMP];
    int huff_map[GJ_MAX_COMP][2];
    uint8_t qraw[4][64];
    bool q_present[4];
    uint8_t hbits[4][2][17];
    uint8_t hvals[4][2][256];
    bool h_present[4][2];
    const char* comment;
    struct gpujpeg_image_metadata metadata;
    /* scans: byte range of the entropy-coded data of each scan inside the file */
    int scan_count;
    size_t scan_begin[GJ_MAX_COMP], scan_end[GJ_MAX_COMP];
    /* APP13 segment info, if present: per scan, pointer to big-endian u32 offsets */
    const uint8_t* seg_info[GJ_MAX_COMP][GPUJPEG_MAX_SEGMENT_INFO_HEADER_COUNT];
    int seg_info_size[GJ_MAX_COMP][GPUJPEG_MAX_SEGMENT_INFO_HEADER_COUNT];
    int seg_info_count[GJ_MAX_COMP];
    size_t header_end; /* offset of the first SOS marker */
    size_t sof_dims;   /* offset of SOF0's height field: the four bytes height, width (big-endian u16 each) that streams of one family may differ in */
    bool eoi_seen;
    bool progressive;  /* the frame header is SOF2 (only with allow_progressive): the parse ended at the first SOS -- header_end, scan_begin[0], the tables
                          defined up to there; param.interleaved says "whole-MCU planes"; the scans are gj_reader_parse_progressive's */
};
/* parse every marker; when segments != NULL also split scans at RSTn on the host (reference behaviour) */
struct gj_host_segments {
    uint32_t* pos; uint32_t* len; uint32_t* index; /* arrays of capacity cap */
    int count, cap;
};
int gj_reader_parse(const uint8_t* image, size_t size, int verbose, bool ff_cs_itu601_is_709,
                    enum gpujpeg_pixel_format req_pixfmt, enum gpujpeg_color_space req_cs, unsigned req_alignment,
                    struct gj_reader_result* r, bool headers_only, bool allow_progressive /* SOF2 is taken (dec_opt_progressive); false: refused as ever */);
int gj_reader_split_scans(const uint8_t* image, const struct gj_reader_result* r, const gj_geom* g, struct gj_host_segments* segs, int verbose);

/* the scans of a progressive frame (gj_reader.c: gj_reader_parse_progressive) */
struct gj_prog_scan {
    int ncomp, comp[GJ_MAX_COMP];   /* components of the scan: indices into the frame's, ascending */
    int ss, se, ah, al;
    int restart_interval;           /* as DRI stood at the SOS: MCUs of a scan of several components, BLOCKS of a scan of one */
    int table[GJ_MAX_COMP];         /* per scan component, the entry of gj_prog_info::pool it decodes with: the DC table in a first DC scan, the AC table
                                       in an AC scan; -1 in a DC refinement (bits only) */
    int across, units;              /* what it codes: one component -- the ceil(w_c / 8) x ceil(h_c / 8) blocks of the component in raster order, `across`
                                       per row (NOT the padded plane's pitch); several -- the MCUs of the frame's grid */
    size_t begin, end;              /* its entropy-coded data: first byte, the marker behind */
    int seg_first, seg_count;       /* its restart segments in gj_prog_info::segs (index: the segment's number inside the scan) */
    int level;                      /* 0, or 1 + the highest level of an earlier scan that shares a component and a coefficient with it */
};
struct gj_prog_table { uint8_t bits[17]; uint8_t vals[256]; }; /* BITS / HUFFVAL in force at a scan's SOS */
struct gj_prog_info {
    int scan_count, levels;
    int bad_scan;                   /* 0: a valid script (ITU T.81 Annex G); else 1 + the first scan that breaks a rule */
    struct gj_prog_scan scan[GJ_PROG_MAX_SCANS];
    struct gj_prog_table* pool; int pool_count, pool_cap;
    struct gj_host_segments segs;
};
int gj_reader_parse_progressive(const uint8_t* image, size_t size, const struct gj_reader_result* r, struct gj_prog_info* info, bool quiet);
void gj_prog_info_free(struct gj_prog_info* info);

/* ---- image file I/O (src/utils/image_delegate.c, pam.c, y4m.c) ---- */
int gj_image_load(const char* filename, enum gpujpeg_image_file_format fmt, uint8_t** image, size_t* size);
int gj_image_save(const char* filename, enum gpujpeg_image_file_format fmt, const uint8_t* image, size_t size,
                  const struct gpujpeg_image_parameters* param_image);
int gj_image_probe(const char* filename, enum gpujpeg_image_file_format fmt, struct gpujpeg_image_parameters* param_image, int file_exists);

#endif
