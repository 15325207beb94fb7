/*
 * gj_decoder.c -- the libgpujpeg decoder API on MI355X. Host driver counterpart of
 * src/gpujpeg_decoder.c: same entry points, output types, ownership and error behaviour. The JPEG
 * bytes are uploaded once and decoded in place (no per-segment host memcpy as in
 * src/gpujpeg_reader.c:1115,1128).
 */
#define _GNU_SOURCE
#include <assert.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "gj_internal.h"
#include "gpujpeg_amd_ext.h"

/* What ONE call was asked for: made by its entry point -- gpujpeg_decoder_decode from the options, a batch call's single-frame route from the batch's
 * rectangle of that frame --, handed to decoder_decode and constant from there on, the same for every attempt. Never stored in the decoder. */
struct dec_request {
    int scale;                 /* 1, 2, 4, 8 */
    bool region; int rect[4];  /* the x, y, w, h pixels only */
    bool resize;               /* crop-and-resize: a region call whose rectangle is resampled ... */
    struct gj_resize rs;       /* ... like this */
};

/* The image a call decodes to: the stream's own (scale 1, no region), the reduced one, or the W x H one over a region's cover planes (crop-and-resize:
 * the resampled one). Written by dec_image_set alone. */
struct dec_image {
    int scale;                           /* 1, 2, 4, 8 */
    bool region, resize;                 /* (the scale and a region exclude each other; resize: a region whose image is the resampled one) */
    gj_geom geom;                        /* scale > 1 or region: geometry and parameters of that image */
    struct gpujpeg_image_parameters pi;
    gj_region rg;                        /* region: pixel rectangle, cover, planned selection */
};

struct gpujpeg_decoder {
    struct gj_coder coder;
    enum gpujpeg_pixel_format req_pixel_format;
    enum gpujpeg_color_space req_color_space;
    bool ff_cs_itu601_is_709;
    unsigned req_alignment;
    struct gpujpeg_image_metadata metadata;
    /* device */
    uint8_t* d_jpeg; size_t d_jpeg_cap;
    uint32_t* d_seg; size_t d_seg_cap; /* pos | len | index */
    uint16_t* d_huff_tab;
    uint16_t* d_qtab;
    /* host */
    uint8_t* h_raw; size_t h_raw_cap; /* pinned internal output buffer */
    uint32_t* h_seg; size_t h_seg_cap; /* pinned staging of the segment table */
    uint16_t* h_tabs;                  /* pinned staging: 8 decode tables + 4 quant tables */
    struct gj_host_segments segs;
    int use_fused;
    bool flipped;                 /* dec_opt_flipped */
    unsigned channel_remap;       /* dec_opt_channel_remap, packed; 0 = none */
    int keep_coefs;               /* 1: leave the coefficients in HBM after the call (gpujpeg_amd_decoder_keep_coefficients) */
    uint16_t* d_tok; size_t d_tok_cap;     /* token mode (gj_hip.h): non-zero AC coefficients of the frame */
    void* d_blkrec; size_t d_blkrec_cap;   /* token mode: one record per block */
    /* device-side segment discovery */
    uint8_t* h_hdr;               /* pinned: first bytes of a device-resident stream, for header parsing */
    uint32_t* d_scan_scratch; size_t d_scan_scratch_cap;
    gj_scan_summary* d_summary;   /* the device's copy: only segment_count is used (speculative launches read it) */
    bool scan_timed;              /* this call's marker scan ran on the device between events 4 and 5 */
    uint32_t last_max_seg_len;    /* longest segment of the last frame decoded with this header (speculative path) */
    uint32_t last_scan_bytes[GJ_MAX_COMP]; /* entropy-coded bytes per scan of the last frame decoded with this header (speculative path) */
    gj_scan_summary* h_summary;   /* pinned */
    uint32_t* h_maxlen; size_t h_maxlen_cap; /* pinned: per-chunk longest segments of the marker scan */
    uint32_t maxlen_parts;
    int host_scan;                /* 1: always walk the stream on the host (reference behaviour) */
    gj_tuning tune;               /* developer switches, read from the environment when the decoder is created */
    /* header cache: a stream that starts with the same bytes (SOI .. first SOS header) as the previous one has the same
     * tables and geometry, so the call goes straight to the kernels and is validated after the fact */
    uint8_t* hdr_cache; uint8_t* d_hdr_cache; size_t hdr_cache_len; bool hdr_cache_valid;
    bool need_planes; /* a frame with the cached header raised the entropy decoders' overflow flag (a segment too long for the LDS stage, a coefficient
                         too large for a token): the following frames with that header go through the kernels without those limits at once,
                         instead of being decoded twice each */
    struct gj_reader_result hdr_cache_r;
    bool tab2_ok;
    /* frame batches (gpujpeg_amd_decoder_decode_batch): per-frame words for ALL frames of a call, work buffers for one chunk of frames */
    gj_scan_summary* b_dsum; size_t b_dsum_cap;    /* device: segment counts */
    gj_scan_summary* bh_sum; size_t bh_sum_cap;    /* pinned: what the host validates */
    uint32_t* bh_maxlen; size_t bh_maxlen_cap;     /* pinned: longest segments per scanning workgroup */
    uint32_t* b_sizes; size_t b_sizes_cap;         /* device: stream sizes */
    uint32_t* bh_sizes; size_t bh_sizes_cap;       /* pinned staging of the same */
    uint32_t* b_seg; size_t b_seg_cap;
    uint32_t* b_scratch; size_t b_scratch_cap;
    int16_t* b_coefs; size_t b_coefs_cap;
    uint8_t* b_planes; size_t b_planes_cap;        /* component planes per frame (configurations whose IDCT side is the generic kernels) */
    uint16_t* b_tok; size_t b_tok_cap;
    void* b_rec; size_t b_rec_cap;
    uint8_t* b_jpeg; size_t b_jpeg_cap;            /* streams handed over in host memory */
    uint8_t* b_raw; size_t b_raw_cap;              /* pixels wanted in host memory */
    uint8_t* b_gather; size_t b_gather_cap;        /* streams given as separate buffers (decode_batch_ptrs), gathered 16-byte aligned */
    uint8_t* b_scatter; size_t b_scatter_cap;      /* ... and the frames decoded back to back before they go to separate buffers */
    int b_last_batched, b_last_single;             /* frames of the last batch call that the batched launches decoded / that went the ordinary way */
    int last_folded;                               /* the last decode call did without the k_marker_table launch (gj_scan_deferred) */
    long n_spec, n_folded, n_again;                /* calls launched on the cached header / of those without the table launch / decoded again the careful way */
    int b_chunk;                                   /* gpujpeg_amd_decoder_set_batch_chunk: frames per launch at most, 0 = the default */
    /* reduced-size decode (dec_opt_scale) and region decode (dec_opt_region): the options. A call reads them once, into its request (struct
     * dec_request); the header cache and the speculative launch hold nothing that depends on them: the parse result and the entropy side are the
     * full-size ones at every scale and for every region. */
    int scale;                                     /* 0 / 1 = full size, else 2, 4, 8 */
    bool region_on; int region[4];                 /* x, y, w, h: written by gpujpeg_decoder_set_option alone */
    struct dec_image img;                          /* what the decode call in progress (and, after it, the last one) decodes to */
    int last_idct_path;                            /* gj_dec_job::idct_path of the last call */
    uint32_t* d_sel; size_t d_sel_cap;             /* the compacted segment table of a region's selection */
    uint32_t* d_sel_count; uint32_t* h_sel_count;  /* its entry count on the device; pinned: [0] the same, [1 + c] entries of scan c */
    long region_stats[4];                          /* gpujpeg_amd_decoder_get_region_stats */
    /* batches of regions (gpujpeg_amd_decoder_decode_batch_regions): one rectangle per frame */
    uint32_t* b_sel; size_t b_sel_cap;             /* device: the compacted segment tables of one chunk of frames, laid out like b_seg */
    gj_region_frame* b_rgn; size_t b_rgn_cap;      /* device: origin and covers of every frame of a call */
    gj_region_frame* bh_rgn; size_t bh_rgn_cap;    /* pinned staging of the same */
    uint32_t* bh_found; size_t bh_found_cap;       /* pinned: [frame][GJ_MAX_COMP] entries per scan the selection found */
    /* dec_opt_resize_prescale: the largest reduction crop-and-resize may put in front of its resample (0 / 1: none, else 2, 4, 8). Read by that call alone,
     * into its rectangles' description (struct dec_rects); the scale every frame of its last call took: gpujpeg_amd_decoder_get_prescales */
    int resize_prescale;
    uint8_t* prescales; int prescales_n, prescales_cap;
    /* dec_opt_resize_filter: the filter of crop-and-resize's resample (GJ_RESIZE_FILTER_BILINEAR, the default, or _ANTIALIAS). Read by that call alone,
     * into its rectangles' description like the prescale */
    int resize_filter;
    /* dec_opt_resize_prescale_subsampled: 1 = the prescale reduces 4:2:0-like streams too, each component at its own N (gj_region_prescale). Read by that
     * call alone, into its rectangles' description like the two above; no effect without a prescale */
    int resize_prescale_subsampled;
    /* dec_opt_batch_sizes: 1 = the streams of a crop-and-resize call may differ in image size ("mixed"). Read by that call alone, into its rectangles'
     * description. The headers of the call's frames (pinned: gathered by one launch from device-resident streams) and every frame's geometry
     * (pinned staging and device copy, uploaded once per call next to b_rgn) */
    int batch_sizes_mixed;
    uint8_t* bh_hdrs; size_t bh_hdrs_cap;
    gj_geom* bh_geoms; size_t bh_geoms_cap;
    gj_geom* b_geoms; size_t b_geoms_cap;
    /* dec_opt_batch_headers: 1 = the family of such a call holds every stream of the reference's shape, whatever its tables and marker segments ("any").
     * Read by that call alone, and only next to "mixed". Every frame's header record and the pool of table sets (pinned staging and device copy,
     * uploaded once per call next to b_geoms), the headers that did not end inside the gather window (pinned), and what the last such call took
     * (gpujpeg_amd_decoder_get_batch_header_stats) */
    int batch_headers_any;
    uint16_t* bh_tabsets; size_t bh_tabsets_cap;
    uint16_t* b_tabsets; size_t b_tabsets_cap;
    uint8_t* bh_long_hdrs; size_t bh_long_hdrs_cap;
    long hdr_stats[4]; bool hdr_stats_valid;
    double hdr_ms[3];                              /* ... and where the host's look at the headers spent its time (gpujpeg_amd_decoder_get_batch_header_times) */
    /* dec_opt_batch_restartless: 1 = the batch calls take streams without restart markers through their batched launches (gj_dec_job::batch_restartless).
     * Read by every batch call, once, when it starts. What the batched launches of the last such call handed to the entropy decoders and what those
     * read of it (gpujpeg_amd_decoder_get_entropy_bytes); pinned, per frame of a call with rectangles: the bytes its selection found and, per scan,
     * the bytes of a restart-less scan that were not read (gj_region::h_sel_bytes, h_left_early) */
    int batch_restartless;
    uint64_t entropy_bytes[2]; bool entropy_valid;
    uint32_t* bh_sel_bytes; size_t bh_sel_bytes_cap;
    uint32_t* bh_left; size_t bh_left_cap;
    /* dec_opt_progressive: 1 = the reader takes SOF2 (the option alone sets the reader's flag). A progressive frame has its own route (dec_progressive):
     * its scan list, the pinned staging and the device copy of its work list -- decode tables of every table snapshot, then the records --, and its
     * OWN quantisation tables (u16, then float): d_huff_tab holds the cached header's, which such a frame must leave alone */
    int progressive;
    struct gj_prog_info prog;
    uint8_t* d_prog; size_t d_prog_cap;
    uint8_t* h_prog; size_t h_prog_cap;
    uint16_t* d_prog_q; uint16_t* h_prog_q;
    long prog_stats[4]; bool prog_stats_valid;     /* gpujpeg_amd_decoder_get_progressive_stats */
    /* dec_opt_batch_progressive: 1 = the batch calls take the progressive frames that form a group through batched launches of their own
     * (batch_progressive). Read by every batch call, once, when it starts. What those launches of the last such call took
     * (gpujpeg_amd_decoder_get_progressive_batch_stats); pinned: the device-resident streams of the call's candidates for the host's walk; device:
     * the frames of a chunk whose slots in the caller's output are not a constant distance apart, before they are copied there */
    int batch_progressive;
    long pb_stats[4]; bool pb_stats_valid;
    uint8_t* bh_pstreams; size_t bh_pstreams_cap;
    uint8_t* b_praw; size_t b_praw_cap;
};

/* what a call decodes to: the stream's image, or the reduced one */
static bool dec_reduced_or_region(const struct gpujpeg_decoder* d) { return d->img.scale > 1 || d->img.region; }
static size_t dec_raw_size(const struct gpujpeg_decoder* d) { return dec_reduced_or_region(d) ? d->img.geom.raw_size : d->coder.geom.raw_size; }
static struct gpujpeg_image_parameters dec_out_param_image(const struct gpujpeg_decoder* d)
{
    struct gpujpeg_image_parameters pi = dec_reduced_or_region(d) ? d->img.pi : d->coder.param_image;
    if (pi.color_space == GPUJPEG_NONE) pi.color_space = d->coder.param.color_space_internal;
    return pi;
}

/* the one writer of d->img. geom / pi: the reduced or the region image, NULL where there is none (the stream's own image, or a refusal: what a
 * refused call leaves describes no region image); rg: NULL unless the image is a region's */
static void dec_image_set(struct gpujpeg_decoder* d, int scale, const gj_geom* geom, const struct gpujpeg_image_parameters* pi, const gj_region* rg)
{
    struct dec_image* m = &d->img;
    m->scale = scale;
    m->region = rg != NULL;
    m->resize = rg != NULL && rg->resize != 0;
    if (geom) m->geom = *geom;
    if (pi) m->pi = *pi;
    if (rg) m->rg = *rg;
}

static struct dec_request dec_request_options(const struct gpujpeg_decoder* d)
{
    struct dec_request q = {.scale = d->scale > 1 ? d->scale : 1, .region = d->region_on};
    memcpy(q.rect, d->region, sizeof q.rect);
    return q;
}

/* The image of the call, once the coder is configured for the stream: the request checked against the stream and the decoder's other options, geometry
 * and parameters of the reduced image (gj_geom_init_scaled) or of the region's (gj_region_plan: cover, selection per scan) derived. 0 or -1 (refused,
 * with a message). */
static int dec_call_geometry(struct gpujpeg_decoder* d, const struct dec_request* q)
{
    const struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    gj_geom gs;
    struct gpujpeg_image_parameters ps;
    dec_image_set(d, q->scale, NULL, NULL, NULL);
    if (q->scale > 1) {
        if (d->flipped) {
            GJ_ERROR(GPUJPEG_DEC_OPT_FLIPPED_BOOL " is not available together with " GPUJPEG_AMD_DEC_OPT_SCALE "=1/%d!\n", q->scale);
            return -1;
        }
        if (gj_geom_init_scaled(&gs, g, &c->param, &c->param_image, q->scale, d->req_alignment, &ps) != 0) return -1;
        dec_image_set(d, q->scale, &gs, &ps, NULL);
    }
    if (!q->region) {
        if (q->scale > 1 || g->raw_width == g->width) return 0;
        /* a full-size call: packed 4:2:2 of odd width has no image -- the pixel kernels would store the whole last pixel pair, past the raw_size bytes of
         * the output. Not for a call that cuts rectangles out of the image or reduces it: those images have their own width checked
         * (gj_geom_init_region, gj_geom_init_scaled) */
        GJ_ERROR("Packed 4:2:2 output needs an even width: the image is %dx%d!\n", g->width, g->height);
        return -1;
    }
    if (q->scale > 1) {
        GJ_ERROR(GPUJPEG_AMD_DEC_OPT_REGION " is not available together with " GPUJPEG_AMD_DEC_OPT_SCALE "=1/%d!\n", q->scale);
        return -1;
    }
    if (d->flipped) {
        GJ_ERROR(GPUJPEG_AMD_DEC_OPT_REGION " is not available together with " GPUJPEG_DEC_OPT_FLIPPED_BOOL "!\n");
        return -1;
    }
    gj_region rg;
    if (gj_region_plan(&gs, &rg, g, &c->param, &c->param_image, q->rect, q->resize ? &q->rs : NULL, d->req_alignment, &ps) != 0) return -1;
    dec_image_set(d, 1, &gs, &ps, &rg);
    return 0;
}

#define GJ_HDR_WINDOW 65536

/* ------------------------------------------------------------------ output helpers (gpujpeg_decoder.h:105-143) */
void gpujpeg_decoder_output_set_default(struct gpujpeg_decoder_output* o) { o->type = GPUJPEG_DECODER_OUTPUT_INTERNAL_BUFFER; o->data = NULL; o->data_size = 0; o->texture = NULL; }
void gpujpeg_decoder_output_set_custom(struct gpujpeg_decoder_output* o, uint8_t* buf) { o->type = GPUJPEG_DECODER_OUTPUT_CUSTOM_BUFFER; o->data = buf; o->data_size = 0; o->texture = NULL; }
void gpujpeg_decoder_output_set_texture(struct gpujpeg_decoder_output* o, struct gpujpeg_opengl_texture* t) { o->type = GPUJPEG_DECODER_OUTPUT_OPENGL_TEXTURE; o->data = NULL; o->data_size = 0; o->texture = t; }
void gpujpeg_decoder_output_set_cuda_buffer(struct gpujpeg_decoder_output* o) { o->type = GPUJPEG_DECODER_OUTPUT_CUDA_BUFFER; o->data = NULL; o->data_size = 0; o->texture = NULL; }
void gpujpeg_decoder_output_set_custom_cuda(struct gpujpeg_decoder_output* o, uint8_t* d_buf) { o->type = GPUJPEG_DECODER_OUTPUT_CUSTOM_CUDA_BUFFER; o->data = d_buf; o->data_size = 0; o->texture = NULL; }

/* ------------------------------------------------------------------ create / destroy (src/gpujpeg_decoder.c:97-183, 560-584) */
#define GJ_TABS_QF_OFFSET (8 * GJ_DEC_TAB_WORDS + 4 * 64 + 4 * GJ_DEC2_WORDS) /* u16 words; 4-byte aligned */
#define GJ_TABS_WORDS (GJ_TABS_QF_OFFSET + 4 * 64 * 2)

struct gpujpeg_decoder* gpujpeg_decoder_create(cudaStream_t stream)
{
    gj_init_term_colors();
    struct gpujpeg_decoder* d = calloc(1, sizeof *d);
    if (!d) return NULL;
    d->coder.stream = (gj_stream_t)stream;
    d->req_pixel_format = GPUJPEG_PIXFMT_AUTODETECT;
    d->req_color_space = GPUJPEG_CS_DEFAULT;
    gj_hip_tuning_defaults(&d->tune);
    d->coder.ht_on = d->tune.host_timing != 0;
    d->use_fused = !d->tune.no_fused;
    gpujpeg_set_default_parameters(&d->coder.param);
    gpujpeg_image_set_default_parameters(&d->coder.param_image);
    d->coder.param.comp_count = 0;
    d->coder.param.restart_interval = 0;
    if (gj_hip_get_device(&d->coder.device) != 0) goto fail;
    if (gj_timers_create(&d->coder.timers) != 0) goto fail;
    d->d_huff_tab = gj_hip_malloc(GJ_TABS_WORDS * sizeof(uint16_t));
    d->h_tabs = gj_hip_host_alloc(GJ_TABS_WORDS * sizeof(uint16_t));
    if (!d->d_huff_tab || !d->h_tabs) goto fail;
    d->d_qtab = d->d_huff_tab + 8 * GJ_DEC_TAB_WORDS;
    d->h_hdr = gj_hip_host_alloc(GJ_HDR_WINDOW);
    d->d_summary = gj_hip_malloc(sizeof(gj_scan_summary));
    d->h_summary = gj_hip_host_alloc(sizeof(gj_scan_summary));
    d->d_sel_count = gj_hip_malloc(sizeof(uint32_t));
    d->h_sel_count = gj_hip_host_alloc((1 + GJ_MAX_COMP) * sizeof(uint32_t));
    if (!d->h_hdr || !d->d_summary || !d->h_summary || !d->d_sel_count || !d->h_sel_count) goto fail;
    if (gj_hip_memset(d->d_summary, 0, sizeof(gj_scan_summary), d->coder.stream) != 0 || gj_hip_stream_sync(d->coder.stream) != 0) goto fail;
    d->host_scan = d->tune.host_scan;
    return d;
fail:
    GJ_ERROR("Decoder initialisation failed: %s\n", gj_hip_last_error());
    gpujpeg_decoder_destroy(d);
    return NULL;
}

struct gpujpeg_decoder_init_parameters gpujpeg_decoder_default_init_parameters(void)
{
    return (struct gpujpeg_decoder_init_parameters){(cudaStream_t)0, 0, false, false};
}

struct gpujpeg_decoder* gpujpeg_decoder_create_with_params(const struct gpujpeg_decoder_init_parameters* params)
{
    struct gpujpeg_decoder* d = gpujpeg_decoder_create(params->stream);
    if (!d) return NULL;
    d->coder.param.verbose = params->verbose;
    d->coder.param.perf_stats = params->perf_stats;
    d->ff_cs_itu601_is_709 = params->ff_cs_itu601_is_709;
    return d;
}

int gpujpeg_decoder_destroy(struct gpujpeg_decoder* d)
{
    if (!d) return -1;
    gj_coder_process_stats_overall(&d->coder);
    gj_timers_destroy(&d->coder.timers);
    gj_hip_free(d->d_jpeg); gj_hip_free(d->d_seg); gj_hip_free(d->d_huff_tab);
    gj_hip_free(d->coder.d_raw_own); gj_hip_free(d->coder.d_planes); gj_hip_free(d->coder.d_coefs);
    gj_hip_free(d->d_tok); gj_hip_free(d->d_blkrec);
    gj_hip_host_free(d->h_raw); gj_hip_host_free(d->h_seg); gj_hip_host_free(d->h_tabs);
    free(d->hdr_cache); gj_hip_free(d->d_hdr_cache);
    gj_hip_host_free(d->h_hdr); gj_hip_host_free(d->h_summary); gj_hip_host_free(d->h_maxlen); gj_hip_free(d->d_summary); gj_hip_free(d->d_scan_scratch);
    free(d->segs.pos); free(d->segs.len); free(d->segs.index); free(d->prescales);
    gj_hip_free(d->d_sel); gj_hip_free(d->d_sel_count); gj_hip_host_free(d->h_sel_count);
    gj_hip_free(d->b_dsum); gj_hip_free(d->b_sizes); gj_hip_free(d->b_seg); gj_hip_free(d->b_scratch); gj_hip_free(d->b_coefs); gj_hip_free(d->b_planes); gj_hip_free(d->b_tok);
    gj_hip_free(d->b_rec); gj_hip_free(d->b_jpeg); gj_hip_free(d->b_raw); gj_hip_free(d->b_gather); gj_hip_free(d->b_scatter);
    gj_hip_host_free(d->bh_sum); gj_hip_host_free(d->bh_maxlen); gj_hip_host_free(d->bh_sizes);
    gj_hip_free(d->b_sel); gj_hip_free(d->b_rgn); gj_hip_host_free(d->bh_rgn); gj_hip_host_free(d->bh_found);
    gj_hip_host_free(d->bh_hdrs); gj_hip_host_free(d->bh_geoms); gj_hip_free(d->b_geoms);
    gj_hip_host_free(d->bh_tabsets); gj_hip_free(d->b_tabsets); gj_hip_host_free(d->bh_long_hdrs);
    gj_hip_host_free(d->bh_sel_bytes); gj_hip_host_free(d->bh_left);
    gj_hip_host_free(d->bh_pstreams); gj_hip_free(d->b_praw);
    gj_prog_info_free(&d->prog); gj_hip_free(d->d_prog); gj_hip_host_free(d->h_prog); gj_hip_free(d->d_prog_q); gj_hip_host_free(d->h_prog_q);
    free(d);
    return 0;
}

void gpujpeg_decoder_set_output_format(struct gpujpeg_decoder* d, enum gpujpeg_color_space cs, enum gpujpeg_pixel_format pf)
{
    d->req_color_space = cs;
    d->req_pixel_format = pf;
    d->hdr_cache_valid = false; /* the cached parse result embeds the requested output format */
}

/* ------------------------------------------------------------------ configuration (src/gpujpeg_decoder.c:185-233) */
static int decoder_configure(struct gpujpeg_decoder* d, const struct gpujpeg_parameters* p, const struct gpujpeg_image_parameters* pi)
{
    struct gj_coder* c = &d->coder;
    const int verbose = c->param.verbose, perf = c->param.perf_stats;
    if (c->configured && gj_parameters_equal(&c->param, p) && gj_image_parameters_equal(&c->param_image, pi)) return 0;
    if (c->configured && verbose >= GPUJPEG_LL_INFO) fprintf(stderr, "[GPUJPEG] [Info] Reinitializing decoder.\n");
    c->configured = false;
    c->param = *p;
    c->param.verbose = verbose;
    c->param.perf_stats = perf;
    c->param_image = *pi;
    gj_geom* g = &c->geom;
    if (gj_geom_init(g, p, pi, false) != 0) {
        GJ_ERROR("Failed to init coder image!\n");
        return -1;
    }
    if (gj_ensure_device_buffer((void**)&c->d_coefs, &c->d_coefs_cap, g->data_size * sizeof(int16_t)) != 0) return -1;
    if (gj_ensure_device_buffer((void**)&c->d_planes, &c->d_planes_cap, g->data_size) != 0) return -1;
    if (gj_ensure_device_buffer((void**)&d->d_seg, &d->d_seg_cap, ((size_t)g->segment_count * 3 + 4) * sizeof(uint32_t)) != 0) return -1;
    const size_t seg_bytes = (size_t)g->segment_count * 3 * sizeof(uint32_t);
    if (gj_ensure_pinned_buffer((void**)&d->h_seg, &d->h_seg_cap, seg_bytes, seg_bytes) != 0) return -1;
    c->configured = true;
    return 0;
}

int gpujpeg_decoder_init(struct gpujpeg_decoder* d, const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* pi)
{
    d->coder.param.verbose = param->verbose;
    d->coder.param.perf_stats = param->perf_stats || param->verbose >= GPUJPEG_LL_STATUS;
    if ((size_t)pi->width * pi->height * param->comp_count == 0) return 0;
    if (decoder_configure(d, param, pi) != 0) return -1;
    gpujpeg_decoder_set_output_format(d, pi->color_space, pi->pixel_format);
    return 0;
}

/* ------------------------------------------------------------------ decode (src/gpujpeg_decoder.c:235-465) */

/* Validate what the device found: scans in component order, each introduced by a well-formed SOS, EOI at the end.
 * Fills the Huffman table selectors of the later scans. Returns 0 when the device table can be used. */
static int accept_device_scan(const gj_scan_summary* su, struct gj_reader_result* r, const gj_geom* g)
{
    if (su->status != 1 || su->other_count > GJ_SCAN_MAX_OTHER || su->rst_irregular) return -1;
    const int expect_scans = g->interleaved ? 1 : g->comp_count;
    if ((int)su->scan_count != expect_scans) return -1;
    if (su->segment_count > (uint32_t)g->segment_count) return -1;
    /* order the markers by position and check them one by one */
    int order[GJ_SCAN_MAX_OTHER];
    const int n = (int)su->other_count;
    for (int i = 0; i < n; i++) {
        int j = i;
        while (j > 0 && su->other_pos[order[j - 1]] > su->other_pos[i]) { order[j] = order[j - 1]; j--; }
        order[j] = i;
    }
    int scan = 1;
    for (int i = 0; i < n; i++) {
        const int k = order[i];
        const uint8_t* b = su->other_bytes[k];
        if (su->other_code[k] == 0xD9) return (scan == expect_scans) ? 0 : -1;
        if (su->other_code[k] != 0xDA || scan >= expect_scans) return -1;
        /* SOS of a non-interleaved scan: length 8, one component, id of component `scan`, tables, 0, 63, 0 */
        if (b[0] != 0 || b[1] != 8 || b[2] != 1 || b[3] != r->comp_id[scan] || b[5] != 0 || b[6] != 63 || b[7] != 0) return -1;
        r->huff_map[scan][0] = (b[4] >> 4) & 15;
        r->huff_map[scan][1] = b[4] & 15;
        scan++;
    }
    return -1; /* no EOI */
}

/* the longest restart segment of the device's table: the maximum of the per-chunk values the marker scan left (valid once the stream has been
 * waited for) */
static void summary_take_maxlen(gj_scan_summary* su, const uint32_t* parts, uint32_t n)
{
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++)
        if (parts[i] > m) m = parts[i];
    su->max_seg_len = m;
}

/* entropy-coded bytes per scan: what the entropy decoder's batch sizes are cut to (luminance segments are 2-3 x the chrominance ones) */
static void summary_scan_bytes(const gj_scan_summary* su, uint32_t bytes[GJ_MAX_COMP])
{
    for (int sc = 0; sc < GJ_MAX_COMP; sc++) bytes[sc] = sc < (int)su->scan_count ? su->scan_end[sc] - su->scan_start[sc] : 0;
}

/* The acceptance rule of a launch on the cached header (single frames and batches): now that the summary of the stream is on the host, was
 * the stream what the launch assumed? Same header, nothing the fast kernels could not stage, the usual scan structure with the cached
 * header's table selectors, and every segment present (a stream with missing segments needs the planes cleared first). */
static bool spec_summary_ok(const struct gpujpeg_decoder* d, const gj_scan_summary* su, const gj_geom* g)
{
    const struct gj_reader_result* r = &d->hdr_cache_r;
    struct gj_reader_result chk = *r;
    if (su->header_differs != 0 || su->seq_overflow != 0 || accept_device_scan(su, &chk, g) != 0 || (int)su->segment_count != g->segment_count) return false;
    for (int i = 0; i < g->comp_count; i++)
        if (chk.huff_map[i][0] != r->huff_map[i][0] || chk.huff_map[i][1] != r->huff_map[i][1]) return false;
    return true;
}

/* what the acceptance rule reads of a header: the component ids and the Huffman selectors of every component's SOS header, as the launch assumed them */
struct hdr_sel {
    uint8_t comp_id[GJ_MAX_COMP]; uint8_t huff[GJ_MAX_COMP][2];
    uint8_t refused; /* 1: the reader did not take this frame's header -- its errors are on stderr already (the reader prints them whatever the
                        verbosity): the frame is not parsed, and so not reported, a second time */
};
/* The same rule for a frame that was launched on its OWN header (dec_opt_batch_headers = any): against that header's ids and selectors. */
static bool spec_summary_ok_own(const struct hdr_sel* s, const gj_scan_summary* su, const gj_geom* g)
{
    struct gj_reader_result chk; /* (accept_device_scan reads comp_id and writes huff_map, nothing else) */
    for (int i = 0; i < GJ_MAX_COMP; i++) {
        chk.comp_id[i] = s->comp_id[i];
        chk.huff_map[i][0] = s->huff[i][0];
        chk.huff_map[i][1] = s->huff[i][1];
    }
    if (su->header_differs != 0 || su->seq_overflow != 0 || accept_device_scan(su, &chk, g) != 0 || (int)su->segment_count != g->segment_count) return false;
    for (int i = 0; i < g->comp_count; i++)
        if (chk.huff_map[i][0] != s->huff[i][0] || chk.huff_map[i][1] != s->huff[i][1]) return false;
    return true;
}

/* what the kernels are to know about the last accepted frame of this header (speculative launches and batches plan with it) */
static void remember_summary(struct gpujpeg_decoder* d, const gj_scan_summary* su)
{
    summary_scan_bytes(su, d->last_scan_bytes);
    d->last_max_seg_len = su->max_seg_len;
}

static void geom_take_tables(gj_geom* g, const struct gj_reader_result* r)
{
    for (int i = 0; i < g->comp_count; i++) {
        g->comp[i].q_table = r->quant_map[i];
        g->comp[i].dc_table = r->huff_map[i][0];
        g->comp[i].ac_table = r->huff_map[i][1];
    }
}

/* a selection's share of every scan's bytes -- sel[sc] of the scan's segments --: an estimate, it only sizes the entropy decoders' batches */
static void selected_scan_bytes(const gj_geom* g, const int sel[GJ_MAX_COMP], uint32_t scan_bytes[GJ_MAX_COMP])
{
    for (int sc = 0; sc < g->scan_count && sc < GJ_MAX_COMP; sc++) {
        const int all = g->interleaved ? g->segment_count : g->comp[sc].segment_count;
        if (all > 0) scan_bytes[sc] = (uint32_t)((uint64_t)scan_bytes[sc] * (uint64_t)sel[sc] / (uint64_t)all);
    }
}

/* everything of a job that comes from the decoder's state and options (geometry with its table selectors included: set those first) */
static void dec_job_base(struct gpujpeg_decoder* d, bool tab2_ok, gj_dec_job* job)
{
    const struct gj_coder* c = &d->coder;
    memset(job, 0, sizeof *job);
    d->last_idct_path = 0;
    job->idct_path = &d->last_idct_path;
    job->g = c->geom;
    job->d_huff_tab = d->d_huff_tab;
    job->d_qtab = d->d_qtab;
    job->d_qtabf = (const float*)(const void*)(d->d_huff_tab + GJ_TABS_QF_OFFSET);
    job->d_huff_tab2 = tab2_ok ? d->d_qtab + 4 * 64 : NULL;
    job->d_coefs = c->d_coefs;
    job->d_planes = c->d_planes;
    job->use_fused = d->use_fused && !d->flipped;
    job->flipped = d->flipped;
    job->channel_remap = d->channel_remap;
    job->tune = d->tune;
    if (d->img.scale > 1) {
        job->scale = d->img.scale;
        job->gs = d->img.geom;
    }
    if (d->img.region) {
        job->region = d->img.rg;
        job->region.on = 1;
        job->gs = d->img.geom;
    }
}

/* One call = up to three attempts (decoder_decode). What the stages of an attempt share: */
struct dec_call {
    const struct dec_request* req;           /* what the call was asked for: the same for every attempt */
    uint8_t* image; size_t image_size;       /* the stream as the caller gave it */
    struct gpujpeg_decoder_output* output;
    bool jpeg_on_device;                     /* device-resident stream (MI355X extension) */
    bool stats; double t_read0;
    bool careful;        /* this attempt must not use the entropy decoders that take whole restart segments into LDS (a previous attempt on this
                            stream met a segment that does not fit), and it does not launch on the header cache */
    bool spec;           /* launched on the cached header, validated afterwards */
    bool device_scan;    /* the device finds the segments (decided by dec_headers; dec_segment_table may hand over to the host walk) */
    bool host_io;        /* copies from or into the caller's host memory have been queued on the coder's stream */
    const uint8_t* himage; /* host view of (at least the headers of) the stream */
    uint8_t* host_copy;    /* the whole of a device-resident stream for the host walk; freed by decoder_decode */
    const uint8_t* d_jpeg;
    uint8_t* d_raw;
    int seg_count;
    const uint32_t* d_seg_count;
    gj_scan_deferred scan_deferred;
    bool tab2_ok;
    bool no_select;      /* region call: a previous attempt's selection did not match its plan -- this one entropy-decodes every segment */
    bool select;         /* region call: this attempt entropy-decodes the segments that touch the cover only */
    struct gj_reader_result r;
};
/* what an attempt and its stages return: 0, a negative error code of the call, or DEC_AGAIN (dec_after only: another attempt, with k->careful as
 * this one left it). dec_device_scan alone uses 1 for something else: "not a stream for the device scan". */
enum { DEC_DONE = 0, DEC_FAILED = -1, DEC_AGAIN = 1 };

/* the one place that brings the whole of a device-resident stream to the host, and the full parse of the host walk; 0 or the error code of the call */
static int dec_host_view(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    if (k->jpeg_on_device && !k->host_copy) {
        k->host_copy = malloc(k->image_size);
        if (!k->host_copy || gj_hip_memcpy_d2h(k->host_copy, k->image, k->image_size, c->stream) != 0 || gj_hip_stream_sync(c->stream) != 0) return -1;
    }
    k->himage = k->jpeg_on_device ? k->host_copy : k->image;
    const int rc = gj_reader_parse(k->himage, k->image_size, c->param.verbose, d->ff_cs_itu601_is_709, d->req_pixel_format, d->req_color_space,
                                   d->req_alignment, &k->r, false, d->progressive != 0);
    if (rc != 0) GJ_ERROR("Decoder failed when decoding image data!\n");
    return rc > 0 ? -1 : rc; /* (the reader's own error code is what the call returns; a positive one would read as DEC_AGAIN) */
}

/* ---- 1. headers. A device-resident stream (MI355X extension) is parsed from a 64 KiB window. Decides who finds the segments. ---- */
static int dec_headers(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const bool may_scan = !d->host_scan;
    k->himage = k->image;
    /* speculative path: same header as last time (compared on the device for a device-resident stream) */
    k->spec = may_scan && d->hdr_cache_valid && k->image_size > d->hdr_cache_len && !d->tune.dec_no_spec && !k->careful;
    if (k->spec && !k->jpeg_on_device) k->spec = memcmp(k->image, d->hdr_cache, d->hdr_cache_len) == 0;
    /* (dec_opt_progressive = on: a device-resident stream may be a progressive one, which never launches on the cached header and leaves the cache
     * alone -- its header is looked at on the host first, where without the option the device compares it behind the launch) */
    if (k->spec && k->jpeg_on_device && d->progressive) {
        if (gj_hip_memcpy_d2h(d->h_hdr, k->image, d->hdr_cache_len, c->stream) != 0 || gj_hip_stream_sync(c->stream) != 0) return -1;
        k->spec = memcmp(d->h_hdr, d->hdr_cache, d->hdr_cache_len) == 0;
    }
    if (k->spec) {
        k->r = d->hdr_cache_r;
        k->device_scan = true;
        return 0;
    }
    size_t hsize = k->image_size;
    if (k->jpeg_on_device) {
        hsize = k->image_size < GJ_HDR_WINDOW ? k->image_size : GJ_HDR_WINDOW;
        if (gj_hip_memcpy_d2h(d->h_hdr, k->image, hsize, c->stream) != 0 || gj_hip_stream_sync(c->stream) != 0) return -1;
        k->himage = d->h_hdr;
    }
    /* an odd header, or an APP13 index that makes scanning unnecessary: the host walk */
    k->device_scan = may_scan &&
                     gj_reader_parse(k->himage, hsize, hsize < k->image_size ? GPUJPEG_LL_QUIET - 1 : c->param.verbose, d->ff_cs_itu601_is_709,
                                     d->req_pixel_format, d->req_color_space, d->req_alignment, &k->r, true, d->progressive != 0) == 0 &&
                     k->r.seg_info_count[0] == 0;
    if (k->device_scan && k->r.progressive) k->device_scan = false; /* (a progressive frame: the host walks every scan) */
    return k->device_scan ? 0 : dec_host_view(d, k);
}

/* ---- 2. stream to HBM ---- */
static int dec_upload(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    if (k->stats || !k->jpeg_on_device) gj_hip_event_record(c->timers.copy_in[0], c->stream); /* (without perf_stats too: see gj_internal.h, copy markers) */
    if (k->jpeg_on_device) {
        k->d_jpeg = k->image;
        return 0;
    }
    if (gj_ensure_device_buffer((void**)&d->d_jpeg, &d->d_jpeg_cap, k->image_size + 64) != 0) return -1;
    k->host_io = true;
    k->d_jpeg = d->d_jpeg;
    return gj_hip_memcpy_h2d(d->d_jpeg, k->image, k->image_size, c->stream); /* (on the coder's own stream, not in the upload lane behind other coders' images) */
}

/* the marker scan on the device: the plain one is waited for and judged here (-> 1 when the stream is not for it), a speculative one leaves its
 * second launch to gj_hip_decode and is judged once everything has run */
static int dec_device_scan(struct gpujpeg_decoder* d, struct dec_call* k, size_t S)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    const size_t begin = k->r.scan_begin[0];
    const size_t words = gj_hip_find_segments_scratch_words(begin, k->image_size, (uint32_t)g->segment_count);
    if (gj_ensure_device_buffer((void**)&d->d_scan_scratch, &d->d_scan_scratch_cap, words * sizeof(uint32_t)) != 0) return -1;
    /* (a speculative launch on a device-resident stream has its header compared with the cached one by the scan's first kernel) */
    const bool cmp = k->spec && k->jpeg_on_device;
    const uint8_t* d_hdr = cmp ? d->d_hdr_cache : NULL;
    const uint32_t hdr_len = cmp ? (uint32_t)d->hdr_cache_len : 0u;
    /* the kernels write what the host validates straight into pinned host memory */
    /* (a word per scanning workgroup, or -- when the table launch is folded into the token decoder -- per batch of that kernel: at most a few thousand) */
    size_t max_chunks = gj_hip_find_segments_max_chunks(begin, k->image_size);
    if (max_chunks < 4096) max_chunks = 4096;
    int frc = gj_ensure_pinned_buffer((void**)&d->h_maxlen, &d->h_maxlen_cap, max_chunks * sizeof(uint32_t), max_chunks * sizeof(uint32_t) * 2);
    const uint32_t maxlen_cap = (uint32_t)(d->h_maxlen_cap / sizeof(uint32_t));
    d->h_summary->rst_irregular = 0;
    d->h_summary->seq_overflow = 0;
    d->h_summary->header_differs = 0;
    GJ_HT(c, 0);
    if (k->stats) gj_hip_event_record(c->timers.ev[4], c->stream); /* (the marker scan is GPU time of this call: events 4 and 5 bracket it) */
    /* speculative launches leave the scan's second launch to gj_hip_decode: the token decoder does without it (gj_scan_deferred) */
    if (frc == 0 && k->spec)
        frc = gj_hip_find_segments_deferred(g, k->d_jpeg, begin, k->image_size, d->d_seg, d->d_seg + S, d->d_seg + 2 * S, (uint32_t)g->segment_count,
                                            d->d_scan_scratch, d->d_summary, d_hdr, hdr_len, d->h_summary, d->h_maxlen, maxlen_cap, &d->maxlen_parts,
                                            c->stream, &d->tune, &k->scan_deferred);
    else if (frc == 0)
        frc = gj_hip_find_segments(g, k->d_jpeg, begin, k->image_size, d->d_seg, d->d_seg + S, d->d_seg + 2 * S, (uint32_t)g->segment_count,
                                   d->d_scan_scratch, d->d_summary, d_hdr, hdr_len, d->h_summary, d->h_maxlen, maxlen_cap, &d->maxlen_parts, c->stream,
                                   &d->tune);
    if (k->stats) gj_hip_event_record(c->timers.ev[5], c->stream);
    d->scan_timed = k->stats;
    if (frc != 0 || (!k->spec && gj_hip_stream_sync(c->stream) != 0)) {
        GJ_ERROR("Marker scan failed: %s\n", gj_hip_last_error());
        return -1;
    }
    if (k->spec) { /* the kernels take the segment count from the device; the summary is checked once everything has run */
        k->seg_count = g->segment_count;
        k->d_seg_count = &d->d_summary->segment_count;
        return 0;
    }
    summary_take_maxlen(d->h_summary, d->h_maxlen, d->maxlen_parts);
    if (accept_device_scan(d->h_summary, &k->r, g) != 0) return 1;
    k->seg_count = (int)d->h_summary->segment_count;
    return 0;
}

/* the reference's way: the host walks the stream and the table is uploaded */
static int dec_host_scan(struct gpujpeg_decoder* d, struct dec_call* k, size_t S)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    if (gj_reader_split_scans(k->himage, &k->r, g, &d->segs, c->param.verbose) != 0) return -1;
    if (d->segs.count > g->segment_count) {
        GJ_ERROR("Decoder can't decode image that has segment count %d (maximum segment count for specified parameters is %d)!\n", d->segs.count, g->segment_count);
        return -1;
    }
    k->seg_count = d->segs.count;
    const size_t ns = (size_t)k->seg_count;
    if (gj_ensure_pinned_buffer((void**)&d->h_seg, &d->h_seg_cap, ns * 3 * sizeof(uint32_t), ns * 3 * sizeof(uint32_t)) != 0) return -1;
    memcpy(d->h_seg, d->segs.pos, ns * sizeof(uint32_t));
    memcpy(d->h_seg + ns, d->segs.len, ns * sizeof(uint32_t));
    memcpy(d->h_seg + 2 * ns, d->segs.index, ns * sizeof(uint32_t));
    if (gj_hip_memcpy_h2d(d->d_seg, d->h_seg, ns * sizeof(uint32_t), c->stream) != 0 ||
        gj_hip_memcpy_h2d(d->d_seg + S, d->h_seg + ns, ns * sizeof(uint32_t), c->stream) != 0 ||
        gj_hip_memcpy_h2d(d->d_seg + 2 * S, d->h_seg + 2 * ns, ns * sizeof(uint32_t), c->stream) != 0)
        return -1;
    return 0;
}

/* ---- 3. segment table ---- */
static int dec_segment_table(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    k->seg_count = 0;
    k->d_seg_count = NULL;
    memset(&k->scan_deferred, 0, sizeof k->scan_deferred);
    const size_t S = (size_t)g->segment_count + GJ_MAX_COMP;
    if (gj_ensure_device_buffer((void**)&d->d_seg, &d->d_seg_cap, (S * 4 + 8) * sizeof(uint32_t)) != 0) return -1;
    if (k->device_scan) {
        const int src = dec_device_scan(d, k, S);
        if (src < 0) return -1;
        if (src > 0) {
            /* unusual stream (markers between scans, damaged data...): the host walk decides */
            GJ_DEBUG(c->param.verbose, "device marker scan not applicable (status %u), walking the stream on the host\n", d->h_summary->status);
            k->device_scan = false;
            const int vrc = dec_host_view(d, k);
            if (vrc != 0) return vrc;
        }
    }
    if (!k->device_scan && dec_host_scan(d, k, S) != 0) return -1;
    if (k->seg_count != g->segment_count && c->param.verbose >= 0) GJ_WARN("%d segments read, expected %d. Broken JPEG?\n", k->seg_count, g->segment_count);
    c->stats.duration_stream = k->stats ? (gpujpeg_get_time() - k->t_read0) * 1000.0 : 0;
    return 0;
}

/* ---- 4. tables: decode tables for every DHT slot present, natural-order quantisation tables (on the device already for the cached header) ---- */
static int dec_tables(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    gj_geom* g = &c->geom;
    const struct gj_reader_result* r = &k->r;
    geom_take_tables(g, r);
    k->tab2_ok = d->tab2_ok;
    if (k->spec) return 0;
    memset(d->h_tabs, 0, GJ_TABS_WORDS * sizeof(uint16_t));
    for (int th = 0; th < 4; th++)
        for (int tc = 0; tc < 2; tc++)
            if (r->h_present[th][tc] && gj_huffman_decoder_table(r->hbits[th][tc], r->hvals[th][tc], d->h_tabs + (th * 2 + tc) * GJ_DEC_TAB_WORDS) != 0) {
                GJ_ERROR("Invalid Huffman table %d/%d!\n", th, tc);
                return -1;
            }
    for (int t = 0; t < 4; t++)
        if (r->q_present[t]) {
            uint16_t* qi = d->h_tabs + 8 * GJ_DEC_TAB_WORDS + t * 64;
            float* qf = (float*)(void*)(d->h_tabs + GJ_TABS_QF_OFFSET) + t * 64;
            gj_quant_table_inverse(r->qraw[t], qi);
            for (int i = 0; i < 64; i++) qf[i] = (float)qi[i];
        }
    /* two-level tables of the sub-sequence decoder: slots 0 and 1 only, every table has to fit the layout */
    k->tab2_ok = true;
    for (int i = 0; i < g->comp_count; i++)
        if (g->comp[i].dc_table > 1 || g->comp[i].ac_table > 1) k->tab2_ok = false;
    for (int th = 0; th < 2 && k->tab2_ok; th++)
        for (int tc = 0; tc < 2; tc++)
            if (r->h_present[th][tc] && gj_huffman_decoder_table2(r->hbits[th][tc], r->hvals[th][tc], tc,
                                                                   d->h_tabs + 8 * GJ_DEC_TAB_WORDS + 4 * 64 + (th * 2 + tc) * GJ_DEC2_WORDS) != 0)
                k->tab2_ok = false;
    for (int i = 0; i < g->comp_count; i++) {
        if (g->comp[i].q_table > 3 || g->comp[i].dc_table > 3 || g->comp[i].ac_table > 3 || !r->q_present[g->comp[i].q_table] ||
            !r->h_present[g->comp[i].dc_table][0] || !r->h_present[g->comp[i].ac_table][1]) {
            GJ_ERROR("Component %d refers to a table that was not defined!\n", i);
            return -1;
        }
    }
    if (gj_hip_memcpy_h2d(d->d_huff_tab, d->h_tabs, GJ_TABS_WORDS * sizeof(uint16_t), c->stream) != 0) {
        GJ_ERROR("Decoder copy compressed data failed: %s\n", gj_hip_last_error());
        return -1;
    }
    d->tab2_ok = k->tab2_ok;
    return 0;
}

/* ---- 5. destination (:336-375) ---- */
static int dec_destination(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    if (k->output->type == GPUJPEG_DECODER_OUTPUT_CUSTOM_CUDA_BUFFER) {
        k->d_raw = k->output->data;
    } else if (k->output->type == GPUJPEG_DECODER_OUTPUT_OPENGL_TEXTURE) {
        GJ_ERROR("OpenGL texture output is not supported by the MI355X build.\n");
        return -1;
    } else {
        if (gj_ensure_device_buffer((void**)&c->d_raw_own, &c->d_raw_cap, dec_raw_size(d)) != 0) return -1;
        k->d_raw = c->d_raw_own;
    }
    return 0;
}

/* ---- 6. the kernels ---- */
static int dec_launch(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    const size_t S = (size_t)g->segment_count + GJ_MAX_COMP;
    gj_dec_job job;
    dec_job_base(d, k->tab2_ok, &job);
    job.d_jpeg = k->d_jpeg;
    job.jpeg_size = k->image_size;
    job.d_seg_pos = d->d_seg;
    job.d_seg_len = d->d_seg + S;
    job.d_seg_index = d->d_seg + 2 * S;
    job.seg_count = k->seg_count;
    job.d_seg_count = k->d_seg_count;
    job.scan = k->scan_deferred;
    d->last_folded = 0;
    job.scan.folded = &d->last_folded;
    if (k->spec) d->n_spec++;
    job.d_raw = k->d_raw;
    if (gj_channel_remap_check(d->channel_remap, c->param_image.pixel_format) != 0) return -1;
    /* the sub-sequence entropy decoder zero-fills every block it decodes; a full clear is needed only when segments are missing
     * from the table (their blocks would keep the previous frame's coefficients) -- unknown before the end in the speculative path,
     * which is validated and repeated then */
    job.clear_coefs = !k->spec && k->seg_count != g->segment_count;
    job.zero_coefs = 0;
    /* region call: where the stream is (or, on the cached header, is assumed to be) the regular one of the geometry, only the segments that touch
     * the cover are entropy-decoded. The selected table has fewer entries than the geometry by design; no clear is needed for it -- every block of
     * the cover belongs to a selected segment, and the decoders zero-fill the blocks of the segments they decode. */
    k->select = d->img.region && !k->no_select && g->restart_interval > 0 && (k->spec || k->seg_count == g->segment_count);
    if (k->select) {
        if (gj_ensure_device_buffer((void**)&d->d_sel, &d->d_sel_cap, 3 * S * sizeof(uint32_t)) != 0) return -1;
        job.region.select = 1;
        job.region.d_sel = d->d_sel;
        job.region.d_sel_count = d->d_sel_count;
        job.region.h_sel_count = d->h_sel_count;
        memset(d->h_sel_count, 0xFF, (1 + GJ_MAX_COMP) * sizeof(uint32_t));
    }
    /* token mode buffers (gj_hip.h): one record per block, 4 tokens per stream byte at most */
    /* (crop-and-resize resamples from the cover planes: no token mode) */
    if (!d->keep_coefs && !d->img.resize && job.use_fused && k->tab2_ok && k->image_size < ((size_t)1 << 29) && gj_hip_decode_wants_tokens(&job.g, k->image_size, &d->tune)) {
        const size_t tok_need = (k->image_size * 4 + 64) * sizeof(uint16_t);
        if (tok_need > d->d_tok_cap) { /* (grown with headroom: frames of a sequence vary in size) */
            if (gj_ensure_device_buffer((void**)&d->d_tok, &d->d_tok_cap, tok_need + tok_need / 4) != 0) return -1;
        }
        if ((size_t)g->block_count * 8 + 64 > d->d_blkrec_cap) {
            if (gj_ensure_device_buffer((void**)&d->d_blkrec, &d->d_blkrec_cap, (size_t)g->block_count * 8 + 64) != 0) return -1;
            gj_hip_memset(d->d_blkrec, 0, d->d_blkrec_cap, c->stream);
        }
        job.tokens = 1;
        job.d_tok = d->d_tok;
        job.tok_cap = (uint32_t)(k->image_size * 4);
        job.d_blkrec = d->d_blkrec;
    }
    job.tune.dec_careful = k->careful || d->need_planes;
    /* the word the entropy decoders raise when they meet a segment they cannot stage: in the host's (pinned, device-visible) summary */
    d->h_summary->seq_overflow = 0;
    job.d_overflow = &d->h_summary->seq_overflow;
    if (k->spec) {
        memcpy(job.scan_bytes, d->last_scan_bytes, sizeof job.scan_bytes);
        job.max_seg_len = d->last_max_seg_len;
    } else if (k->device_scan) {
        job.max_seg_len = d->h_summary->max_seg_len;
        summary_scan_bytes(d->h_summary, job.scan_bytes);
    } else {
        job.max_seg_len = 0;
        for (int i = 0; i < d->segs.count; i++)
            if (d->segs.len[i] > job.max_seg_len) job.max_seg_len = d->segs.len[i];
        for (int sc = 0; sc < k->r.scan_count && sc < GJ_MAX_COMP; sc++) { /* (the others stay 0) */
            const size_t from = k->r.scan_begin[sc], to = k->r.scan_end[sc];
            if (to > from) job.scan_bytes[sc] = (uint32_t)(to - from);
        }
    }
    if (!k->spec && k->seg_count != g->segment_count) memset(job.scan_bytes, 0, sizeof job.scan_bytes); /* (table and geometry out of step: one batch size) */
    if (k->select) selected_scan_bytes(g, d->img.rg.sel_count, job.scan_bytes);
    if (gj_hip_decode(&job, c->stream, k->stats ? c->timers.ev : NULL) != 0) {
        GJ_ERROR("Decoder kernels failed: %s\n", gj_hip_last_error());
        return -1;
    }
    /* (the lane-per-segment entropy decoder may have met a segment it cannot stage: known once everything has run) */
    return 0;
}

/* ---- 7. pixels to where the caller wants them ---- */
static int dec_download(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const size_t raw_size = dec_raw_size(d);
    struct gpujpeg_decoder_output* output = k->output;
    output->data_size = raw_size;
    output->param_image = dec_out_param_image(d);
    if (output->type != GPUJPEG_DECODER_OUTPUT_INTERNAL_BUFFER && output->type != GPUJPEG_DECODER_OUTPUT_CUSTOM_BUFFER) {
        output->data = k->d_raw;
        return 0;
    }
    if (output->type == GPUJPEG_DECODER_OUTPUT_INTERNAL_BUFFER) {
        if (gj_ensure_pinned_buffer((void**)&d->h_raw, &d->h_raw_cap, raw_size, raw_size) != 0) return -1;
        output->data = d->h_raw;
    } else {
        assert(output->data != NULL);
    }
    gj_hip_event_record(c->timers.copy_out[0], c->stream);
    k->host_io = true;
    if (gj_hip_download(output->data, k->d_raw, raw_size, c->stream, k->stats ? NULL : c->timers.lane_out) != 0) return -1; /* (the process's download lane) */
    if (k->stats) gj_hip_event_record(c->timers.copy_out[1], c->stream);
    return 0;
}

/* a region's selection: did k_segment_select find in this stream's table what the plan took from the geometry? */
static bool dec_selection_ok(const struct gpujpeg_decoder* d, const struct dec_call* k)
{
    if (!k->select) return true;
    uint32_t sum = 0;
    for (int sc = 0; sc < GJ_MAX_COMP; sc++) {
        if (d->h_sel_count[1 + sc] != (uint32_t)d->img.rg.sel_count[sc]) return false;
        sum += (uint32_t)d->img.rg.sel_count[sc];
    }
    return d->h_sel_count[0] == sum;
}

/* ---- 8. everything has run: was a launch on the cached header justified? Which header do the next calls launch on? ---- */
static int dec_after(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    const gj_scan_summary* su = d->h_summary;
    if (!k->spec && !dec_selection_ok(d, k)) {
        GJ_DEBUG(c->param.verbose, "the region's selection found other segments than planned: decoding again with every segment\n");
        k->no_select = true;
        return DEC_AGAIN;
    }
    if (!k->spec && su->seq_overflow && !k->careful) { /* (a kernel forced on a stream with segments it cannot stage; or, after a host
                                                           walk, a table whose longest segment the host did not foresee) */
        GJ_DEBUG(c->param.verbose, "a restart segment did not fit the entropy decoder's LDS stage: decoding again through the coefficient planes\n");
        d->need_planes = true; /* (and so for the frames that follow with this header) */
        k->careful = true;
        return DEC_AGAIN;
    }
    if (k->spec) { /* now the summary of this stream is on the host: was it what we assumed? */
        summary_take_maxlen(d->h_summary, d->h_maxlen, d->maxlen_parts);
        if (spec_summary_ok(d, su, g) && !dec_selection_ok(d, k)) { /* (cannot happen for a stream the rule accepts: its table is the geometry's) */
            d->n_again++;
            k->no_select = true;
            return DEC_AGAIN;
        }
        if (!spec_summary_ok(d, su, g)) { /* different header or unusual scan structure: decode again the careful way */
            d->n_again++;
            if (d->last_folded) d->n_folded--; /* (counted at the launch: only accepted launches count as folded) */
            const bool overflow_only = su->seq_overflow != 0 && su->header_differs == 0;
            if (overflow_only) d->need_planes = true; /* (the header was the assumed one: it stays cached, the next frames launch on it with the other kernels) */
            else d->hdr_cache_valid = false;
            k->careful = overflow_only;
            return DEC_AGAIN;
        }
        remember_summary(d, su);
        if ((int)su->segment_count != g->segment_count && c->param.verbose >= 0)
            GJ_WARN("%d segments read, expected %d. Broken JPEG?\n", (int)su->segment_count, g->segment_count);
    } else if (k->device_scan && k->r.scan_begin[0] <= GJ_HDR_WINDOW && k->r.scan_begin[0] < k->image_size) {
        /* remember this header (SOI .. first SOS header) for the next call */
        const size_t n = k->r.scan_begin[0];
        if (!d->hdr_cache) d->hdr_cache = malloc(GJ_HDR_WINDOW);
        if (!d->d_hdr_cache) d->d_hdr_cache = gj_hip_malloc(GJ_HDR_WINDOW);
        if (d->hdr_cache && d->d_hdr_cache) {
            /* another header than the cached one: what was learnt about the old one's frames does not apply (unless this very call is the
             * second attempt that learnt it) */
            if (!k->careful && !(d->hdr_cache_len == n && memcmp(d->hdr_cache, k->himage, n) == 0)) d->need_planes = false;
            memcpy(d->hdr_cache, k->himage, n);
            if (gj_hip_memcpy_h2d(d->d_hdr_cache, d->hdr_cache, n, c->stream) == 0 && gj_hip_stream_sync(c->stream) == 0) {
                d->hdr_cache_len = n;
                d->hdr_cache_r = k->r;
                d->hdr_cache_r.comment = NULL;
                d->hdr_cache_valid = true;
                remember_summary(d, su);
            }
        }
    } else {
        d->hdr_cache_valid = false;
    }
    return DEC_DONE;
}

static void dec_stats(struct gpujpeg_decoder* d, const struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const struct gpujpeg_decoder_output* output = k->output;
    if (k->stats) {
        struct gpujpeg_duration_stats* s = &c->stats;
        s->duration_huffman_coder = gj_hip_event_elapsed_ms(c->timers.ev[0], c->timers.ev[1]);
        s->duration_dct_quantization = gj_hip_event_elapsed_ms(c->timers.ev[1], c->timers.ev[2]);
        s->duration_preprocessor = gj_hip_event_elapsed_ms(c->timers.ev[2], c->timers.ev[3]);
        s->duration_in_gpu = gj_hip_event_elapsed_ms(c->timers.ev[0], c->timers.ev[3]);
        for (int i = 0; i < GJ_DEC_EVENTS - 1; i++) c->kernel_ms[i] = gj_hip_event_elapsed_ms(c->timers.ev[i], c->timers.ev[i + 1]);
        c->kernel_ms[3] = d->scan_timed ? gj_hip_event_elapsed_ms(c->timers.ev[4], c->timers.ev[5]) : 0.0f; /* the marker scan, when the device did it */
        s->duration_in_gpu += c->kernel_ms[3];
        c->kernel_ms[4] = (float)d->last_idct_path; /* (not a duration: which IDCT side ran, gpujpeg_amd_ext.h) */
        c->timers.valid = true;
        s->duration_memory_to = gj_hip_event_elapsed_ms(c->timers.copy_in[0], c->timers.copy_in[1]);
        if (output->type == GPUJPEG_DECODER_OUTPUT_INTERNAL_BUFFER || output->type == GPUJPEG_DECODER_OUTPUT_CUSTOM_BUFFER)
            s->duration_memory_from = gj_hip_event_elapsed_ms(c->timers.copy_out[0], c->timers.copy_out[1]);
    }
    gj_coder_process_stats(c, k->stats);
    if (c->param.verbose >= GPUJPEG_LL_STATUS)
        fprintf(stderr, "Decompressed Size:%13zu bytes %dx%d %s %s\n", output->data_size, output->param_image.width, output->param_image.height,
                gpujpeg_pixel_format_get_name(output->param_image.pixel_format), gpujpeg_color_space_get_name(output->param_image.color_space));
}

/* ---- progressive frames (dec_opt_progressive) ---- */
/* The plan of a progressive frame, from its scan list (d->prog) and the coder's geometry: the decode tables of every table snapshot and one record
 * per restart segment of every scan (gj_hip.h: gj_prog_rec), the records of a level back to back, staged in pinned memory and uploaded. 0 or -1. */
/* the records of one level of one frame's scan list, back to back at `recs` (room: the frame's segment count) -> how many; frame: what the records of a
 * chunk of frames name (gj_prog_rec::frame), 0 for a single frame */
static uint32_t prog_level_records(const struct gj_prog_info* info, const gj_geom* g, int level, unsigned frame, gj_prog_rec* recs)
{
    uint32_t at = 0;
    for (int si = 0; si < info->scan_count; si++) {
        const struct gj_prog_scan* s = &info->scan[si];
        if (s->level != level) continue;
        const int ri = s->restart_interval;
        for (int j = 0; j < s->seg_count; j++) {
            const int e = s->seg_first + j;
            const uint32_t number = info->segs.index[e]; /* the segment's number inside its scan */
            const uint64_t first = ri > 0 ? (uint64_t)number * (uint64_t)ri : 0;
            if (first >= (uint64_t)s->units) continue;
            gj_prog_rec* q = &recs[at++];
            q->pos = info->segs.pos[e];
            q->len = info->segs.len[e];
            q->first = (uint32_t)first;
            q->count = ri > 0 && first + (uint64_t)ri < (uint64_t)s->units ? (uint32_t)ri : (uint32_t)((uint64_t)s->units - first);
            q->across = (uint32_t)s->across;
            q->kind = (uint8_t)(s->ss == 0 ? (s->ah == 0 ? GJ_PROG_DC_FIRST : GJ_PROG_DC_REFINE) : (s->ah == 0 ? GJ_PROG_AC_FIRST : GJ_PROG_AC_REFINE));
            q->ncomp = (uint8_t)s->ncomp;
            q->ss = (uint8_t)s->ss; q->se = (uint8_t)s->se; q->ah = (uint8_t)s->ah; q->al = (uint8_t)s->al;
            q->frame = (uint16_t)frame;
            for (int i = 0; i < s->ncomp; i++) {
                const gj_comp_geom* k = &g->comp[s->comp[i]];
                q->c[i].base = (uint32_t)(k->data_offset / 64);
                q->c[i].pitch = (uint32_t)k->blocks_x;
                q->c[i].table = (uint16_t)(s->table[i] >= 0 ? s->table[i] : 0);
                q->c[i].h = (uint8_t)(s->ncomp > 1 ? k->samp_h : 1);
                q->c[i].v = (uint8_t)(s->ncomp > 1 ? k->samp_v : 1);
            }
        }
    }
    return at;
}

static int prog_plan(struct gpujpeg_decoder* d, gj_prog_plan* plan)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    const struct gj_prog_info* info = &d->prog;
    const size_t tab_bytes = ((size_t)info->pool_count * GJ_DEC_TAB_WORDS * sizeof(uint16_t) + 15) & ~(size_t)15;
    const size_t nrec = (size_t)info->segs.count;
    const size_t bytes = tab_bytes + (nrec + 1) * sizeof(gj_prog_rec);
    if (gj_ensure_pinned_buffer((void**)&d->h_prog, &d->h_prog_cap, bytes, bytes * 2) != 0) return -1;
    if (gj_ensure_device_buffer((void**)&d->d_prog, &d->d_prog_cap, bytes) != 0) return -1;
    memset(d->h_prog, 0, bytes);
    for (int t = 0; t < info->pool_count; t++)
        if (gj_huffman_decoder_table(info->pool[t].bits, info->pool[t].vals, (uint16_t*)(void*)d->h_prog + (size_t)t * GJ_DEC_TAB_WORDS) != 0) {
            GJ_ERROR("Invalid Huffman table in a progressive scan!\n");
            return -1;
        }
    gj_prog_rec* recs = (gj_prog_rec*)(void*)(d->h_prog + tab_bytes);
    memset(plan, 0, sizeof *plan);
    uint32_t at = 0;
    for (int level = 0; level < info->levels; level++) {
        plan->level_first[level] = at;
        at += prog_level_records(info, g, level, 0, recs + at);
        plan->level_count[level] = at - plan->level_first[level];
    }
    plan->levels = info->levels;
    plan->d_tabs = (const uint16_t*)(const void*)d->d_prog;
    plan->tab_count = (uint32_t)info->pool_count;
    plan->d_recs = (const gj_prog_rec*)(const void*)(d->d_prog + tab_bytes);
    if (gj_hip_memcpy_h2d(d->d_prog, d->h_prog, tab_bytes + (size_t)at * sizeof(gj_prog_rec), c->stream) != 0) return -1;
    d->prog_stats[0] = 1;
    d->prog_stats[1] = info->scan_count;
    d->prog_stats[2] = info->levels;
    d->prog_stats[3] = (long)at;
    return 0;
}

/* the quantisation tables of a progressive frame (a group of them: any of its frames'): natural order, u16 and float, in the buffer of their own */
static int prog_quant_tables(struct gpujpeg_decoder* d, const struct gj_reader_result* r)
{
    const size_t q_bytes = 4 * 64 * (sizeof(uint16_t) + sizeof(float));
    if (!d->d_prog_q) d->d_prog_q = gj_hip_malloc(q_bytes);
    if (!d->h_prog_q) d->h_prog_q = gj_hip_host_alloc(q_bytes);
    if (!d->d_prog_q || !d->h_prog_q) return -1;
    memset(d->h_prog_q, 0, q_bytes);
    for (int t = 0; t < 4; t++)
        if (r->q_present[t]) {
            uint16_t* qi = d->h_prog_q + t * 64;
            float* qf = (float*)(void*)(d->h_prog_q + 4 * 64) + t * 64;
            gj_quant_table_inverse(r->qraw[t], qi);
            for (int i = 0; i < 64; i++) qf[i] = (float)qi[i];
        }
    return gj_hip_memcpy_h2d(d->d_prog_q, d->h_prog_q, q_bytes, d->coder.stream);
}

/* A progressive frame, once its first headers are parsed (k->r, k->himage the whole stream): the careful route only -- the host walks every scan, no
 * launch on the header cache (which is neither read nor written), no device marker scan, no tokens, no selection. The scans fill the coefficient
 * planes (gj_dec_job::prog), the IDCT side is the plane route of a baseline frame of this geometry, whatever the call asked for. */
static int dec_progressive(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    const struct gj_reader_result* r = &k->r;
    d->prog_stats_valid = true;
    memset(d->prog_stats, 0, sizeof d->prog_stats);
    k->spec = k->device_scan = k->select = false;
    if (gj_reader_parse_progressive(k->himage, k->image_size, r, &d->prog, false) != 0 || d->prog.bad_scan != 0) {
        GJ_ERROR("Decoder failed when decoding image data!\n");
        return DEC_FAILED;
    }
    for (int i = 0; i < r->param.comp_count; i++)
        if (!r->q_present[r->quant_map[i]]) {
            GJ_ERROR("Component %d refers to a table that was not defined!\n", i);
            return DEC_FAILED;
        }
    for (int i = 0; i < GPUJPEG_METADATA_COUNT; i++) d->metadata.vals[i] = r->metadata.vals[i];
    if (decoder_configure(d, &r->param, &r->param_image) != 0 || dec_call_geometry(d, k->req) != 0) return DEC_FAILED;
    c->init_end_time = k->stats ? gpujpeg_get_time() : 0;
    if (dec_upload(d, k) != 0) return DEC_FAILED;
    gj_prog_plan plan;
    if (prog_plan(d, &plan) != 0) return DEC_FAILED;
    if (prog_quant_tables(d, r) != 0) return DEC_FAILED;
    c->stats.duration_stream = k->stats ? (gpujpeg_get_time() - k->t_read0) * 1000.0 : 0;
    if (k->stats) gj_hip_event_record(c->timers.copy_in[1], c->stream);
    if (dec_destination(d, k) != 0) return DEC_FAILED;
    for (int i = 0; i < c->geom.comp_count; i++) {
        c->geom.comp[i].q_table = r->quant_map[i];
        c->geom.comp[i].dc_table = c->geom.comp[i].ac_table = 0;
    }
    gj_dec_job job;
    dec_job_base(d, false, &job);
    job.d_qtab = d->d_prog_q;
    job.d_qtabf = (const float*)(const void*)(d->d_prog_q + 4 * 64);
    job.d_jpeg = k->d_jpeg;
    job.jpeg_size = k->image_size;
    job.d_raw = k->d_raw;
    job.prog = &plan;
    d->last_folded = 0;
    d->scan_timed = false;
    if (gj_channel_remap_check(d->channel_remap, c->param_image.pixel_format) != 0) return DEC_FAILED;
    if (gj_hip_decode(&job, c->stream, k->stats ? c->timers.ev : NULL) != 0) {
        GJ_ERROR("Decoder kernels failed: %s\n", gj_hip_last_error());
        return DEC_FAILED;
    }
    if (dec_download(d, k) != 0) return DEC_FAILED;
    GJ_HT(c, 1);
    if (gj_hip_stream_sync(c->stream) != 0) {
        GJ_ERROR("Decoder failed: %s\n", gj_hip_last_error());
        return DEC_FAILED;
    }
    GJ_HT(c, 2);
    d->region_stats[0] = d->img.region ? 2 : 0;
    d->region_stats[1] = d->region_stats[3] = d->prog_stats[3];
    d->region_stats[2] = d->img.region ? (long)d->img.geom.block_count : (long)c->geom.block_count;
    dec_stats(d, k);
    k->output->metadata = &d->metadata;
    GJ_HT(c, 3);
    c->ht_calls++;
    return DEC_DONE;
}

/* one attempt: the stages in the order their work goes onto the stream */
static int dec_attempt(struct gpujpeg_decoder* d, struct dec_call* k)
{
    struct gj_coder* c = &d->coder;
    GJ_HT_START(c);
    k->stats = c->param.perf_stats != 0 || c->param.verbose >= GPUJPEG_LL_STATUS;
    c->start_time = k->stats ? gpujpeg_get_time() : 0;
    memset(&c->stats, 0, sizeof c->stats);
    k->t_read0 = k->stats ? gpujpeg_get_time() : 0;

    int rc = dec_headers(d, k);
    if (rc != 0) return rc;
    if (k->r.progressive) return dec_progressive(d, k);
    memset(d->prog_stats, 0, sizeof d->prog_stats);
    d->prog_stats_valid = true;
    for (int i = 0; i < GPUJPEG_METADATA_COUNT; i++) d->metadata.vals[i] = k->r.metadata.vals[i];
    if (decoder_configure(d, &k->r.param, &k->r.param_image) != 0 || dec_call_geometry(d, k->req) != 0) return DEC_FAILED;
    c->init_end_time = k->stats ? gpujpeg_get_time() : 0;
    if (dec_upload(d, k) != 0) return DEC_FAILED;
    if ((rc = dec_segment_table(d, k)) != 0) return rc;
    if (dec_tables(d, k) != 0) return DEC_FAILED;
    if (k->stats) gj_hip_event_record(c->timers.copy_in[1], c->stream);
    if (dec_destination(d, k) != 0 || dec_launch(d, k) != 0 || dec_download(d, k) != 0) return DEC_FAILED;
    if (d->last_folded) d->n_folded++;
    GJ_HT(c, 1);
    if (gj_hip_stream_sync(c->stream) != 0) {
        GJ_ERROR("Decoder failed: %s\n", gj_hip_last_error());
        return DEC_FAILED;
    }
    GJ_HT(c, 2);
    if (dec_after(d, k) == DEC_AGAIN) return DEC_AGAIN;
    /* what this call did (gpujpeg_amd_decoder_get_region_stats): from what was launched and what the selection found */
    const long stream_segs = k->spec ? (long)d->h_summary->segment_count : (long)k->seg_count;
    d->region_stats[0] = !d->img.region ? 0 : k->select ? 1 : 2;
    d->region_stats[1] = k->select ? (long)d->h_sel_count[0] : stream_segs;
    d->region_stats[2] = d->img.region ? (long)d->img.geom.block_count : (long)c->geom.block_count;
    d->region_stats[3] = stream_segs;
    dec_stats(d, k);
    k->output->metadata = &d->metadata;
    GJ_HT(c, 3);
    c->ht_calls++;
    return DEC_DONE;
}

/* At most three attempts: on the cached header; rejected for its header or scan structure, the plain way; and when that meets a segment too
 * long for the LDS stage, the careful way (an attempt that is careful already never asks for another). */
static int decoder_decode(struct gpujpeg_decoder* d, const struct dec_request* req, uint8_t* image, size_t image_size, struct gpujpeg_decoder_output* output)
{
    struct dec_call k; /* (not cleared as a whole: it holds a parse result of several KiB) */
    k.req = req;
    k.image = image;
    k.image_size = image_size;
    k.output = output;
    k.jpeg_on_device = gj_hip_is_device_ptr(image) != 0;
    k.careful = false;
    k.no_select = false;
    k.select = false;
    k.host_io = false;
    k.host_copy = NULL;
    int rc = DEC_AGAIN;
    for (int attempt = 0; attempt < 4 && rc == DEC_AGAIN; attempt++) { /* (the fourth: a region's selection that did not match its plan) */
        rc = dec_attempt(d, &k);
        free(k.host_copy);
        k.host_copy = NULL;
    }
    if (rc == DEC_DONE) return 0;
    if (k.host_io) gj_hip_stream_sync(d->coder.stream); /* (what this call queued on its stream must not read or write the caller's memory after the error has left; a copy stranded on a copy lane by a failing event is not covered) */
    return rc < 0 ? rc : -1;
}

int gpujpeg_decoder_decode(struct gpujpeg_decoder* d, uint8_t* image, size_t image_size, struct gpujpeg_decoder_output* output)
{
    const struct dec_request q = dec_request_options(d);
    if (d) d->entropy_valid = d->pb_stats_valid = d->hdr_stats_valid = false;
    return decoder_decode(d, &q, image, image_size, output);
}

int gpujpeg_decoder_get_stats(struct gpujpeg_decoder* d, struct gpujpeg_duration_stats* stats)
{
    if (!d || !stats) return -1;
    *stats = d->coder.stats;
    return 0;
}

/* ------------------------------------------------------------------ frame batches (MI355X extension, include/gpujpeg_amd_ext.h) */
/* Streams with ONE header (a sequence from one encoder) decoded by one set of launches per chunk of frames -- marker scan, marker table, entropy
 * decoder, IDCT, each with blockIdx.z = frame. It is the speculative path of decoder_decode (kernels launched on the cached header, the device
 * compares every stream's header with it, the host validates every frame's summary afterwards) for many frames at once; a frame whose
 * summary does not pass -- another header, an unusual scan structure, a segment the fast kernels cannot stage -- is decoded again by
 * gpujpeg_decoder_decode's own path, and so is everything the batched kernels do not cover. */
#define GJ_DEC_BATCH_CHUNK_MAX 256
#define GJ_DEC_BATCH_BYTES ((size_t)8 << 30) /* work buffers of one chunk */

/* one rectangle per frame of a batch call: a batch of regions (gpujpeg_amd_decoder_decode_batch_regions) or crop-and-resize
 * (gpujpeg_amd_decoder_decode_batch_crop_resize); neither (all NULL / 0): the decoder's own options hold for every frame */
struct dec_rects {
    const int* origins; int rw, rh;          /* a batch of regions, frame f: the rw x rh pixels at (origins[2f], origins[2f + 1]) */
    const int* rects; const uint8_t* mirror; /* crop-and-resize, frame f: the rectangle rects[4f .. 4f + 3] = x, y, w, h, each with its own size ... */
    struct gj_resize resize;                 /* ... resampled to ONE out_w x out_h image per frame (mirror: per frame, when mirror && mirror[f]) */
    bool mixed;                              /* ... of streams that may differ in image size (dec_opt_batch_sizes = mixed) */
    bool any;                                /* ... and in tables and marker segments (dec_opt_batch_headers = any; with mixed alone) */
};

/* what the parts of a batch call share */
struct dec_batch {
    const uint8_t* streams; size_t stream_stride; const size_t* sizes; int count;
    size_t output_stride;
    bool streams_on_device, out_on_device;
    uint8_t* d_out; size_t d_out_stride; /* where the pixels go on the device: the caller's buffer, or a staging area that is copied out at the end */
    size_t frame_raw;                    /* what every frame decodes to (0: not known yet) */
    int first;                           /* 1: frame 0 went the ordinary way ahead of the batched launches */
    uint8_t* frame_done;
    bool host_io;                        /* copies from or into the caller's host memory have been queued */
    struct dec_rects what;               /* the rectangles, if the call has its own */
    bool planned;                        /* the rectangles have been checked against the streams' geometry; what follows is valid then */
    int* plan;                           /* [count][GJ_MAX_COMP] restart segments of every scan that touch frame f's cover */
    int plan_max[GJ_MAX_COMP];           /* the largest of them per scan */
    gj_geom gs_max;                      /* geometry of the rw x rh (crop-and-resize: out_w x out_h) image with the planes of the largest cover (per component the widest and the highest) */
    gj_geom gs_one; gj_region rg_one;    /* the same for one of the frames, and its region (crop-and-resize: the out_w x out_h image over that frame's cover) */
    struct gpujpeg_image_parameters pi_r;
    int img_w, img_h;                    /* the streams' image, as the rectangles were checked against it */
    long stats[4];                       /* gpujpeg_amd_decoder_get_region_stats of the call: sums over the frames */
    bool unselected;                     /* a frame was entropy-decoded in full */
    /* streams of different image sizes (what.mixed): valid once `prepared` */
    bool prepared;                       /* every frame's header has been looked at: */
    uint8_t* fam;                        /* [count] 1: frame f is of the FAMILY -- its header is the cached one except for SOF0's dimensions -- and d->bh_geoms[f] is its geometry */
    int n_fam;                           /* such frames from `first` on */
    gj_geom g_max;                       /* the launch's geometry: the family's, with the segment, block and sample counts of its largest frames */
    /* ... with headers of their own (what.any): d->bh_geoms[f] carries family frame f's header record (GJ_REC_BEGIN ...), d->bh_tabsets the pool of n_sets table sets */
    struct hdr_sel* sel;                 /* [count] what the acceptance rule reads of family frame f's own header */
    int n_sets;
    size_t begin_min;                    /* the smallest first scan byte among the family's frames from `first` on */
    bool restartless;                    /* dec_opt_batch_restartless = on: streams without restart markers go through the batched launches too */
    bool ahead_progressive;              /* frame 0 went ahead and was a progressive frame: it planned no rectangles (batch_decode_one); ahead_w x ahead_h: its image */
    int ahead_w, ahead_h;
    bool prog_batch;                     /* dec_opt_batch_progressive = on and dec_opt_progressive = on: groups of progressive frames go through batched launches (batch_progressive) */
};

/* one rectangle per frame: a batch of regions, or crop-and-resize */
static bool batch_has_regions(const struct dec_batch* b) { return b->what.origins != NULL || b->what.rects != NULL; }
/* ... as the request of frame f's own call: what the single-frame route decodes and what the plan of the batched launches checks */
static struct dec_request batch_request(const struct gpujpeg_decoder* d, const struct dec_batch* b, int f)
{
    const struct dec_rects* w = &b->what;
    struct dec_request q = dec_request_options(d);
    if (w->rects) {
        q.region = q.resize = true;
        memcpy(q.rect, w->rects + 4 * (size_t)f, sizeof q.rect);
        q.rs = w->resize;
        q.rs.mirror = w->mirror && w->mirror[f] ? 1 : 0;
    } else if (w->origins) {
        q.region = true;
        q.rect[0] = w->origins[2 * f]; q.rect[1] = w->origins[2 * f + 1]; q.rect[2] = w->rw; q.rect[3] = w->rh;
    }
    return q;
}

/* the image parameters of a family frame: the cached header's with the frame's own dimensions (and the line padding that follows from the width) */
static struct gpujpeg_image_parameters mixed_param_image(const struct gpujpeg_decoder* d, int w, int h)
{
    struct gpujpeg_image_parameters pi = d->hdr_cache_r.param_image;
    pi.width = w;
    pi.height = h;
    if (d->req_alignment != 0) { /* (the reader's rule, resolve_output) */
        const unsigned linesize = (unsigned)gj_pixfmt_unit_size(pi.pixel_format) * (unsigned)w;
        pi.width_padding = (int)((linesize + d->req_alignment - 1) / d->req_alignment * d->req_alignment - linesize);
    }
    return pi;
}

/* the geometry of a family frame of w x h pixels into d->bh_geoms[f]: one gj_geom_init per distinct size of a call (slot[64], all -1 at first: the
 * frame that last had a size of this hash); the table selectors are the caller's to set. false: the geometry refuses the size */
static bool mixed_frame_geom(struct gpujpeg_decoder* d, int slot[64], int f, int w, int h, const struct gpujpeg_parameters* param)
{
    gj_geom* gf = d->bh_geoms + f;
    const int at = (int)(((unsigned)w * 31u + (unsigned)h) & 63u), same = slot[at];
    if (same >= 0 && d->bh_geoms[same].width == w && d->bh_geoms[same].height == h) {
        *gf = d->bh_geoms[same];
    } else {
        const struct gpujpeg_image_parameters pi = mixed_param_image(d, w, h);
        if (gj_geom_init(gf, param, &pi, false) != 0) return false;
    }
    slot[at] = f;
    return true;
}

/* ---- frames with headers of their own (dec_opt_batch_headers = any, gpujpeg_amd_ext.h) ---- */
/* The first window of every device-resident stream that the gather launch brings to the host: JFIF + DQT + SOF0 + DHT + SOS are ~620 bytes with the
 * Annex K tables and ~350 with optimised ones, a comment or a small Exif block (orientation, camera, date: under 1 KB) fits next to them; an Exif
 * thumbnail or an ICC profile (3 KB to 64 KB) does not, whatever window below GJ_HDR_WINDOW is chosen -- such a header is fetched on its own. 256
 * frames are 1 MB of pinned memory. */
#define GJ_HDR_GATHER 4096

/* Where the first scan's data begin, from the first n bytes of a stream alone: the offset behind the first SOS header; 0: the header does not end
 * within these bytes; -1: not a marker sequence. (The walk of gj_reader_parse without its reading: what tells a header that is cut by the window
 * from one the reader refuses.) */
static long hdr_scan_begin(const uint8_t* p, size_t n)
{
    if (n < 4) return 0;
    if (p[0] != 0xFF || p[1] != 0xD8) return -1;
    size_t o = 2;
    for (;;) {
        if (o + 4 > n) return 0;
        if (p[o] != 0xFF) return -1;
        while (o + 1 < n && p[o + 1] == 0xFF) o++; /* fill bytes */
        if (o + 4 > n) return 0;
        const int m = p[o + 1];
        if (m == 0xD8) { o += 2; continue; }
        if (m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) return -1;
        const size_t len = ((size_t)p[o + 2] << 8) | p[o + 3];
        if (len < 2) return -1;
        if (m == 0xDA) return o + 2 + len <= n ? (long)(o + 2 + len) : 0;
        o += 2 + len;
    }
}

/* The family rule: does the parse of a frame's header agree with the reference's in everything the batched launches take from the LAUNCH -- baseline,
 * component count, ids and sampling, interleaving, restart interval, and what the reader made of APPn / JFIF / Adobe and the ids (colour space,
 * pixel format)? Width, height (and the line padding that follows from the width), tables and table slots are the frame's own. */
static bool hdr_same_shape(const struct gj_reader_result* ref, const struct gj_reader_result* r)
{
    if (ref->progressive || r->progressive) return false;
    struct gpujpeg_image_parameters ia = ref->param_image, ib = r->param_image;
    ib.width = ia.width; ib.height = ia.height; ib.width_padding = ia.width_padding;
    if (!gj_parameters_equal(&ref->param, &r->param) || !gj_image_parameters_equal(&ia, &ib) || ref->header_color_space != r->header_color_space) return false;
    for (int i = 0; i < ref->param.comp_count && i < GJ_MAX_COMP; i++)
        if (ref->comp_id[i] != r->comp_id[i]) return false;
    return true;
}

/* The tables a header's components reference, numbered in the order of their first use (component 0's first): q[i], dc[i], ac[i] = component i's
 * place in a table set, *_src[k] = the header's slot that place k is filled from. Two headers that reference the same contents through different
 * slots have the same set. false: a Huffman table outside slots 0 and 1 (referenced, or merely defined), or a table that is referenced but not defined. */
struct hdr_tabs { int nq, ndc, nac; int q[GJ_MAX_COMP], dc[GJ_MAX_COMP], ac[GJ_MAX_COMP]; int q_src[4], dc_src[2], ac_src[2]; };
static bool hdr_take_tables(const struct gj_reader_result* r, struct hdr_tabs* t)
{
    memset(t, 0, sizeof *t);
    for (int tc = 0; tc < 2; tc++)
        if (r->h_present[2][tc] || r->h_present[3][tc]) return false;
    for (int i = 0; i < r->param.comp_count && i < GJ_MAX_COMP; i++) {
        const int qs = r->quant_map[i], ds = r->huff_map[i][0], as = r->huff_map[i][1];
        if (qs < 0 || qs > 3 || ds < 0 || ds > 1 || as < 0 || as > 1 || !r->q_present[qs] || !r->h_present[ds][0] || !r->h_present[as][1]) return false;
        int k;
        for (k = 0; k < t->nq && t->q_src[k] != qs; k++) {}
        if (k == t->nq) t->q_src[t->nq++] = qs;
        t->q[i] = k;
        for (k = 0; k < t->ndc && t->dc_src[k] != ds; k++) {}
        if (k == t->ndc) t->dc_src[t->ndc++] = ds;
        t->dc[i] = k;
        for (k = 0; k < t->nac && t->ac_src[k] != as; k++) {}
        if (k == t->nac) t->ac_src[t->nac++] = as;
        t->ac[i] = k;
    }
    return true;
}

/* what a table set is made from, byte for byte: the counts, the 64 values of every quantisation table, BITS and HUFFVAL of every Huffman table, in
 * the order of hdr_tabs; what sets are deduplicated by */
#define GJ_HDR_KEY_BYTES (4 + 4 * 64 + 4 * (17 + 256))
static void hdr_tabs_key(const struct gj_reader_result* r, const struct hdr_tabs* t, uint8_t key[GJ_HDR_KEY_BYTES])
{
    memset(key, 0, GJ_HDR_KEY_BYTES);
    key[0] = (uint8_t)t->nq; key[1] = (uint8_t)t->ndc; key[2] = (uint8_t)t->nac;
    uint8_t* p = key + 4;
    for (int k = 0; k < t->nq; k++, p += 64) memcpy(p, r->qraw[t->q_src[k]], 64);
    for (int k = 0; k < t->ndc; k++, p += 17 + 256) { memcpy(p, r->hbits[t->dc_src[k]][0], 17); memcpy(p + 17, r->hvals[t->dc_src[k]][0], 256); }
    for (int k = 0; k < t->nac; k++, p += 17 + 256) { memcpy(p, r->hbits[t->ac_src[k]][1], 17); memcpy(p + 17, r->hvals[t->ac_src[k]][1], 256); }
}

/* a table set (GJ_TABSET_WORDS, gj_hip.h) from its key; false: a Huffman table does not fit the two-level layout */
static bool tabset_build(const uint8_t key[GJ_HDR_KEY_BYTES], uint16_t* set)
{
    memset(set, 0, GJ_TABSET_WORDS * sizeof(uint16_t));
    const int nq = key[0], ndc = key[1], nac = key[2];
    const uint8_t* p = key + 4;
    for (int k = 0; k < nq; k++, p += 64) {
        uint16_t* qi = set + k * 64;
        float* qf = (float*)(void*)(set + GJ_TABSET_QF_OFFSET) + k * 64;
        gj_quant_table_inverse(p, qi);
        for (int i = 0; i < 64; i++) qf[i] = (float)qi[i];
    }
    for (int k = 0; k < ndc; k++, p += 17 + 256)
        if (gj_huffman_decoder_table2(p, p + 17, 0, set + GJ_TABSET_TAB2_OFFSET + (k * 2 + 0) * GJ_DEC2_WORDS) != 0) return false;
    for (int k = 0; k < nac; k++, p += 17 + 256)
        if (gj_huffman_decoder_table2(p, p + 17, 1, set + GJ_TABSET_TAB2_OFFSET + (k * 2 + 1) * GJ_DEC2_WORDS) != 0) return false;
    return true;
}

/* the distinct table sets of a call while its headers are looked at: keys and sets in ordinary memory (the sets move to the pinned pool once their
 * number is known), found through an open-addressing table of key numbers; setno[k] = the set of key k, or -1: its tables do not fit the layout --
 * its frames are no family frames, and it takes no place among the sets */
struct tabset_pool { int n, nkeys, cap, kcap; uint8_t* keys; int* setno; uint16_t* sets; int* slots; unsigned mask; };
static void tabset_pool_free(struct tabset_pool* P) { free(P->keys); free(P->sets); free(P->setno); free(P->slots); memset(P, 0, sizeof *P); }
static int tabset_pool_init(struct tabset_pool* P, int frames)
{
    memset(P, 0, sizeof *P);
    unsigned m = 16;
    while (m < 2u * (unsigned)frames) m *= 2;
    P->slots = malloc((size_t)m * sizeof(int));
    if (!P->slots) return -1;
    for (unsigned i = 0; i < m; i++) P->slots[i] = -1;
    P->mask = m - 1;
    return 0;
}
/* the number of the key's set (built when the key is new), -1: its tables do not fit, -2: out of memory */
static int tabset_pool_find(struct tabset_pool* P, const uint8_t key[GJ_HDR_KEY_BYTES])
{
    uint32_t h = 2166136261u;
    for (int i = 0; i < GJ_HDR_KEY_BYTES; i++) h = (h ^ key[i]) * 16777619u;
    unsigned at = h & P->mask;
    for (; P->slots[at] >= 0; at = (at + 1) & P->mask)
        if (memcmp(P->keys + (size_t)P->slots[at] * GJ_HDR_KEY_BYTES, key, GJ_HDR_KEY_BYTES) == 0) return P->setno[P->slots[at]];
    if (P->nkeys == P->kcap) {
        const int cap = P->kcap ? P->kcap * 2 : 4;
        uint8_t* keys = realloc(P->keys, (size_t)cap * GJ_HDR_KEY_BYTES);
        if (keys) P->keys = keys;
        int* setno = realloc(P->setno, (size_t)cap * sizeof(int));
        if (setno) P->setno = setno;
        if (!keys || !setno) return -2;
        P->kcap = cap;
    }
    if (P->n == P->cap) {
        const int cap = P->cap ? P->cap * 2 : 4;
        uint16_t* sets = realloc(P->sets, (size_t)cap * GJ_TABSET_WORDS * sizeof(uint16_t));
        if (!sets) return -2;
        P->sets = sets;
        P->cap = cap;
    }
    memcpy(P->keys + (size_t)P->nkeys * GJ_HDR_KEY_BYTES, key, GJ_HDR_KEY_BYTES);
    const int set = tabset_build(key, P->sets + (size_t)P->n * GJ_TABSET_WORDS) ? P->n++ : -1;
    P->setno[P->nkeys] = set;
    P->slots[at] = P->nkeys++;
    return set;
}

/* The family of a call whose frames may have headers of their own (dec_rects::any): every frame's header is parsed (header only, quiet) and compared
 * with the reference's parse (hdr_same_shape); a family frame gets the geometry of its own dimensions with the places of ITS tables in its table
 * set (d->bh_geoms[f]), with its header record in that record's fb (GJ_REC_BEGIN, GJ_REC_TABSET: first scan byte, set), and what the acceptance rule reads of its header (b->sel[f]); the
 * distinct sets go to the pinned pool (d->bh_tabsets, b->n_sets). b->fam[f]: 1, or 3 when the header is also byte for byte the cached one except for
 * the dimensions -- the frames a "mixed" call would have taken, whose summaries the next launch on the cached header may plan with. Device-resident
 * streams: one launch gathers the first GJ_HDR_GATHER bytes of every stream; the headers that do not end inside them are copied on their own, up to
 * GJ_HDR_WINDOW bytes each, with one wait for all of them. 0 or -1. */
static int batch_any_family(struct gpujpeg_decoder* d, struct dec_batch* b, int from, bool family)
{
    struct gj_coder* c = &d->coder;
    const int count = b->count;
    const struct gj_reader_result* ref = &d->hdr_cache_r;
    const size_t n = d->hdr_cache_len, dims = ref->sof_dims;
    const bool bytes_rule = d->hdr_cache != NULL && dims >= 2 && dims + 4 <= n;
    memset(d->hdr_stats, 0, sizeof d->hdr_stats);
    memset(d->hdr_ms, 0, sizeof d->hdr_ms);
    const double t_begin = gpujpeg_get_time();
    b->n_sets = 0;
    b->begin_min = 0;
    memset(b->sel, 0, (size_t)count * sizeof *b->sel);
    if (!family) return 0;
    int rc = -1;
    struct tabset_pool P;
    struct gj_reader_result* rr = malloc(sizeof *rr);
    int* long_at = NULL; /* device-resident streams: where frame f's header lies in d->bh_long_hdrs (slot number), -1: inside its gather window */
    if (!rr || tabset_pool_init(&P, count) != 0) { free(rr); return -1; }
    if (b->streams_on_device) {
        const size_t sizes_bytes = (size_t)count * sizeof(uint32_t);
        long_at = malloc((size_t)count * sizeof(int));
        if (!long_at) goto out;
        if (gj_ensure_device_buffer((void**)&d->b_sizes, &d->b_sizes_cap, sizes_bytes) != 0) goto out;
        if (gj_ensure_pinned_buffer((void**)&d->bh_sizes, &d->bh_sizes_cap, sizes_bytes, sizes_bytes + sizes_bytes / 2) != 0) goto out;
        if (gj_ensure_pinned_buffer((void**)&d->bh_hdrs, &d->bh_hdrs_cap, (size_t)count * GJ_HDR_GATHER, (size_t)count * GJ_HDR_GATHER * 2) != 0) goto out;
        for (int f = 0; f < count; f++) d->bh_sizes[f] = b->sizes[f] > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)b->sizes[f];
        if (gj_hip_memcpy_h2d(d->b_sizes, d->bh_sizes, sizes_bytes, c->stream) != 0 ||
            gj_hip_gather_headers(b->streams, b->stream_stride, d->b_sizes, (uint32_t)count, GJ_HDR_GATHER, d->bh_hdrs, c->stream) != 0 ||
            gj_hip_stream_sync(c->stream) != 0) {
            GJ_ERROR("Reading the headers of the batch failed: %s\n", gj_hip_last_error());
            goto out;
        }
        d->hdr_stats[2] = (long)count * GJ_HDR_GATHER;
        int n_long = 0;
        for (int f = 0; f < count; f++) {
            const size_t have = b->sizes[f] < GJ_HDR_GATHER ? b->sizes[f] : GJ_HDR_GATHER;
            long_at[f] = b->sizes[f] > GJ_HDR_GATHER && hdr_scan_begin(d->bh_hdrs + (size_t)f * GJ_HDR_GATHER, have) == 0 ? n_long++ : -1;
        }
        if (n_long > 0) {
            if (gj_ensure_pinned_buffer((void**)&d->bh_long_hdrs, &d->bh_long_hdrs_cap, (size_t)n_long * GJ_HDR_WINDOW, (size_t)n_long * GJ_HDR_WINDOW * 2) != 0) goto out;
            for (int f = 0; f < count; f++) {
                if (long_at[f] < 0) continue;
                const size_t take = b->sizes[f] < GJ_HDR_WINDOW ? b->sizes[f] : GJ_HDR_WINDOW;
                if (gj_hip_memcpy_d2h(d->bh_long_hdrs + (size_t)long_at[f] * GJ_HDR_WINDOW, b->streams + (size_t)f * b->stream_stride, take, c->stream) != 0) goto out;
                d->hdr_stats[2] += (long)take;
            }
            if (gj_hip_stream_sync(c->stream) != 0) {
                GJ_ERROR("Reading the headers of the batch failed: %s\n", gj_hip_last_error());
                goto out;
            }
            d->hdr_stats[3] = n_long;
        }
    }
    d->hdr_ms[0] = (gpujpeg_get_time() - t_begin) * 1000.0;
    int slot[64]; /* (one geometry per distinct size: the frame that last had a size of this hash) */
    for (int i = 0; i < 64; i++) slot[i] = -1;
    for (int f = 0; f < count; f++) {
        const double t_frame = gpujpeg_get_time();
        double t_parsed = t_frame;
        /* (the clock is read three times per frame, ~0.1 us of a parse of 1 to 3 us: [1] reader, [2] family rule, table key and set, geometry) */
#define GJ_HDR_FRAME_DONE() do { const double t_ = gpujpeg_get_time(); d->hdr_ms[1] += (t_parsed - t_frame) * 1000.0; d->hdr_ms[2] += (t_ - t_parsed) * 1000.0; } while (0)
        const uint8_t* hp = b->streams + (size_t)f * b->stream_stride;
        size_t hn = b->sizes[f];
        if (b->streams_on_device) {
            hp = long_at[f] < 0 ? d->bh_hdrs + (size_t)f * GJ_HDR_GATHER : d->bh_long_hdrs + (size_t)long_at[f] * GJ_HDR_WINDOW;
            const size_t cap = long_at[f] < 0 ? (size_t)GJ_HDR_GATHER : (size_t)GJ_HDR_WINDOW;
            if (hn > cap) hn = cap;
        }
        if (hn <= 4 || b->sizes[f] > 0x1FFFFFF0u) { GJ_HDR_FRAME_DONE(); continue; }
        if (gj_reader_parse(hp, hn, GPUJPEG_LL_QUIET - 1, d->ff_cs_itu601_is_709, d->req_pixel_format, d->req_color_space, d->req_alignment, rr, true, d->progressive != 0) != 0) {
            b->sel[f].refused = 1;
            t_parsed = gpujpeg_get_time();
            GJ_HDR_FRAME_DONE();
            continue;
        }
        t_parsed = gpujpeg_get_time();
        if (!hdr_same_shape(ref, rr)) { GJ_HDR_FRAME_DONE(); continue; }
        const size_t begin = rr->scan_begin[0];
        if (begin > GJ_HDR_WINDOW || b->sizes[f] <= begin + 2) { GJ_HDR_FRAME_DONE(); continue; }
        if (!rr->param.interleaved && rr->param.comp_count > 1) {
            /* the selectors of the second and later scans stand in THEIR SOS headers: a stream in host memory is walked for them; a device-resident
             * one is launched with the reference's, and the acceptance rule compares them with what the marker scan finds */
            if (!b->streams_on_device) {
                if (gj_reader_parse(hp, hn, GPUJPEG_LL_QUIET - 1, d->ff_cs_itu601_is_709, d->req_pixel_format, d->req_color_space, d->req_alignment, rr, false, d->progressive != 0) != 0 ||
                    !hdr_same_shape(ref, rr) || rr->scan_begin[0] != begin) {
                    GJ_HDR_FRAME_DONE();
                    continue;
                }
            } else {
                for (int i = 1; i < rr->param.comp_count && i < GJ_MAX_COMP; i++) { rr->huff_map[i][0] = ref->huff_map[i][0]; rr->huff_map[i][1] = ref->huff_map[i][1]; }
            }
        }
        const int w = rr->param_image.width, h = rr->param_image.height;
        struct hdr_tabs t;
        if (w < 1 || h < 1 || !hdr_take_tables(rr, &t)) { GJ_HDR_FRAME_DONE(); continue; }
        uint8_t key[GJ_HDR_KEY_BYTES];
        hdr_tabs_key(rr, &t, key);
        const int set = tabset_pool_find(&P, key);
        if (set == -2) goto out;
        if (set < 0) { GJ_HDR_FRAME_DONE(); continue; }
        gj_geom* gf = d->bh_geoms + f;
        if (!mixed_frame_geom(d, slot, f, w, h, &ref->param)) { GJ_HDR_FRAME_DONE(); continue; }
        for (int i = 0; i < gf->comp_count && i < GJ_MAX_COMP; i++) {
            gf->comp[i].q_table = t.q[i];
            gf->comp[i].dc_table = t.dc[i];
            gf->comp[i].ac_table = t.ac[i];
            b->sel[f].comp_id[i] = rr->comp_id[i];
            b->sel[f].huff[i][0] = (uint8_t)rr->huff_map[i][0];
            b->sel[f].huff[i][1] = (uint8_t)rr->huff_map[i][1];
        }
        memset(&gf->fb, 0, sizeof gf->fb); /* (the header record: the pool's count follows once it is known) */
        GJ_REC_BEGIN(*gf) = begin;
        GJ_REC_TABSET(*gf) = (uint32_t)set;
        const bool bytes = bytes_rule && begin == n && hn >= n && memcmp(hp, d->hdr_cache, dims) == 0 && memcmp(hp + dims + 4, d->hdr_cache + dims + 4, n - dims - 4) == 0;
        b->fam[f] = bytes ? 3 : 1;
        if (f >= from) {
            if (b->n_fam == 0 || begin < b->begin_min) b->begin_min = begin;
            b->n_fam++;
        }
        GJ_HDR_FRAME_DONE();
    }
#undef GJ_HDR_FRAME_DONE
    if (P.n > 0) {
        const size_t bytes = (size_t)P.n * GJ_TABSET_WORDS * sizeof(uint16_t);
        if (gj_ensure_pinned_buffer((void**)&d->bh_tabsets, &d->bh_tabsets_cap, bytes, bytes + bytes / 2) != 0) goto out;
        memcpy(d->bh_tabsets, P.sets, bytes);
    }
    b->n_sets = P.n;
    for (int f = 0; f < count; f++)
        if (b->fam[f]) GJ_REC_TABSETS(d->bh_geoms[f]) = (uint32_t)P.n;
    d->hdr_stats[0] = b->n_fam;
    d->hdr_stats[1] = P.n;
    rc = 0;
out:
    tabset_pool_free(&P);
    free(long_at);
    free(rr);
    return rc;
}

/* Streams of different image sizes (dec_opt_batch_sizes = mixed): the host looks at every frame's header before anything is planned. The FAMILY of
 * the call are the frames whose first hdr_cache_len bytes are the cached header's except for the four dimension bytes of SOF0 (where the reader found
 * them: gj_reader_result::sof_dims): same tables, sampling, restart interval and scan header, so they go through one set of launches, each with the
 * geometry of its own dimensions (d->bh_geoms[f]; gj_geom_init, one per distinct size). Device-resident streams: ONE gather launch and one wait for
 * all headers. Every other frame goes the single-frame route later; its rectangle is checked here, against its own header, so that a refusal comes
 * before anything of the output is written (a header the reader does not take is left to that route's own error). 0 or -1. */
/* (from: the first frame that has not been decoded yet -- 1 when frame 0 goes ahead of everything) */
static int batch_mixed_prepare(struct gpujpeg_decoder* d, struct dec_batch* b, int from)
{
    struct gj_coder* c = &d->coder;
    if (b->prepared) return 0;
    const int count = b->count;
    const struct gj_reader_result* r = &d->hdr_cache_r;
    const size_t n = d->hdr_cache_len, dims = r->sof_dims;
    if (gj_ensure_pinned_buffer((void**)&d->bh_geoms, &d->bh_geoms_cap, (size_t)count * sizeof(gj_geom), (size_t)count * sizeof(gj_geom) * 2) != 0) return -1;
    memset(b->fam, 0, (size_t)count);
    b->n_fam = 0;
    bool family = d->hdr_cache_valid && d->hdr_cache != NULL && dims >= 2 && dims + 4 <= n && b->what.rects != NULL;
    /* (headers of their own, dec_rects::any: the rule over the parsed headers instead of the bytes -- the reference is the cached header's parse) */
    const bool any = b->what.any;
    if (any) {
        family = d->hdr_cache_valid && b->what.rects != NULL;
        if (batch_any_family(d, b, from, family) != 0) return -1;
    }
    const uint8_t* hdrs = b->streams;
    size_t hdr_stride = b->stream_stride;
    if (!any && family && b->streams_on_device) {
        const size_t sizes_bytes = (size_t)count * sizeof(uint32_t);
        if (gj_ensure_device_buffer((void**)&d->b_sizes, &d->b_sizes_cap, sizes_bytes) != 0) return -1;
        if (gj_ensure_pinned_buffer((void**)&d->bh_sizes, &d->bh_sizes_cap, sizes_bytes, sizes_bytes + sizes_bytes / 2) != 0) return -1;
        if (gj_ensure_pinned_buffer((void**)&d->bh_hdrs, &d->bh_hdrs_cap, (size_t)count * n, (size_t)count * n * 2) != 0) return -1;
        for (int f = 0; f < count; f++) d->bh_sizes[f] = b->sizes[f] > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)b->sizes[f];
        if (gj_hip_memcpy_h2d(d->b_sizes, d->bh_sizes, sizes_bytes, c->stream) != 0 ||
            gj_hip_gather_headers(b->streams, b->stream_stride, d->b_sizes, (uint32_t)count, (uint32_t)n, d->bh_hdrs, c->stream) != 0 ||
            gj_hip_stream_sync(c->stream) != 0) {
            GJ_ERROR("Reading the headers of the batch failed: %s\n", gj_hip_last_error());
            return -1;
        }
        hdrs = d->bh_hdrs;
        hdr_stride = n;
    }
    int slot[64]; /* (one geometry per distinct size: the frame that last had a size of this hash) */
    for (int i = 0; i < 64; i++) slot[i] = -1;
    for (int f = 0; f < count && !any; f++) {
        const uint8_t* hb = hdrs + (size_t)f * hdr_stride;
        bool fam = family && b->sizes[f] > n + 2 && memcmp(hb, d->hdr_cache, dims) == 0 && memcmp(hb + dims + 4, d->hdr_cache + dims + 4, n - dims - 4) == 0;
        const int h = fam ? (int)(((unsigned)hb[dims] << 8) | hb[dims + 1]) : 0, w = fam ? (int)(((unsigned)hb[dims + 2] << 8) | hb[dims + 3]) : 0;
        if (fam && (w < 1 || h < 1)) fam = false;
        if (fam) {
            fam = mixed_frame_geom(d, slot, f, w, h, &r->param);
            if (fam) geom_take_tables(d->bh_geoms + f, r);
        }
        if (fam) {
            b->fam[f] = 1;
            if (f >= from) b->n_fam++;
        }
    }
    /* (no frame is of the cached header's family and frame 0 has not gone ahead yet: it will, its header becomes the cached one, and this runs again) */
    for (int f = from; f < count && (b->n_fam > 0 || from > 0); f++) {
        /* not of the family: its rectangle against its own header */
        if (b->fam[f]) continue;
        if (any && b->sel[f].refused) continue; /* (a header the reader has just refused: left to the single-frame route's own error, as below) */
        struct gj_reader_result* rr = malloc(sizeof *rr);
        if (!rr) return -1;
        const uint8_t* himage = b->streams + (size_t)f * b->stream_stride;
        size_t hsize = b->sizes[f];
        int ok = 1;
        if (b->streams_on_device) {
            hsize = hsize < GJ_HDR_WINDOW ? hsize : GJ_HDR_WINDOW;
            if (gj_hip_memcpy_d2h(d->h_hdr, himage, hsize, c->stream) != 0 || gj_hip_stream_sync(c->stream) != 0) { free(rr); return -1; }
            himage = d->h_hdr;
        }
        ok = hsize > 4 && gj_reader_parse(himage, hsize, GPUJPEG_LL_QUIET - 1, d->ff_cs_itu601_is_709, d->req_pixel_format, d->req_color_space, d->req_alignment, rr, true, d->progressive != 0) == 0;
        gj_geom gf, gs;
        gj_region rg;
        struct gpujpeg_image_parameters pr;
        if (ok && gj_geom_init(&gf, &rr->param, &rr->param_image, false) == 0) {
            const struct dec_request q = batch_request(d, b, f);
            const int refused = gj_region_plan(&gs, &rg, &gf, &rr->param, &rr->param_image, q.rect, q.resize ? &q.rs : NULL, d->req_alignment, &pr);
            if (refused != 0) {
                GJ_ERROR("Frame %d of the batch: the rectangle %d,%d,%d,%d was refused%s!\n", f, q.rect[0], q.rect[1], q.rect[2], q.rect[3], refused == -3 ? " by the resize filter" : "");
                free(rr);
                return -1;
            }
        }
        free(rr);
    }
    b->prepared = true;
    return 0;
}

/* The rectangles of a set of frames that share one geometry -- the frames of the baseline batched launches (batch_regions_plan), or a group of
 * progressive frames (batch_progressive) --: the image, region and parameters of the frame planned last, and per component the widest and the highest
 * cover so far */
struct cover_plan {
    gj_geom gs_one; gj_region rg_one; struct gpujpeg_image_parameters pi_r;
    int wmax[GJ_MAX_COMP], hmax[GJ_MAX_COMP];
};

/* frame f's rectangle against geometry g (gj_region_plan; a refusal names the frame): its origin and covers into *out, the scale it takes into the
 * call's prescales, its cover into the largest one. 0 or -1. */
static int batch_cover_frame(struct gpujpeg_decoder* d, const struct dec_batch* b, int f, const gj_geom* g, const struct gpujpeg_parameters* param,
                             const struct gpujpeg_image_parameters* pi_f, struct cover_plan* cp, gj_region_frame* out)
{
    const struct dec_request q = batch_request(d, b, f);
    const int refused = gj_region_plan(&cp->gs_one, &cp->rg_one, g, param, pi_f, q.rect, q.resize ? &q.rs : NULL, d->req_alignment, &cp->pi_r);
    if (refused == -1) GJ_ERROR("Frame %d of the batch: the region %d,%d,%d,%d was refused!\n", f, q.rect[0], q.rect[1], q.rect[2], q.rect[3]);
    if (refused == -3) GJ_ERROR("Frame %d of the batch: the rectangle %d,%d,%d,%d was refused by the resize filter!\n", f, q.rect[0], q.rect[1], q.rect[2], q.rect[3]);
    if (refused != 0) return -1;
    if (q.resize && f < d->prescales_n) d->prescales[f] = (uint8_t)cp->rg_one.frame.scale;
    const gj_region_frame* rf = &cp->rg_one.frame;
    *out = *rf;
    for (int i = 0; i < g->comp_count && i < GJ_MAX_COMP; i++) {
        if (rf->bx1[i] - rf->bx0[i] > cp->wmax[i]) cp->wmax[i] = rf->bx1[i] - rf->bx0[i];
        if (rf->by1[i] - rf->by0[i] > cp->hmax[i]) cp->hmax[i] = rf->by1[i] - rf->by0[i];
    }
    return 0;
}

/* the planes of the largest cover: every frame's cover planes are laid out like this (*gs_max: the image of the frame planned last over them) */
static void batch_cover_planes(const struct cover_plan* cp, const gj_geom* g, gj_geom* gs_max)
{
    *gs_max = cp->gs_one;
    uint64_t offset = 0;
    for (int i = 0; i < g->comp_count && i < GJ_MAX_COMP; i++) {
        gj_comp_geom* k = &gs_max->comp[i];
        k->blocks_x = cp->wmax[i];
        k->blocks_y = cp->hmax[i];
        k->data_width = cp->wmax[i] * 8;
        k->data_height = cp->hmax[i] * 8;
        k->data_offset = offset;
        offset += (uint64_t)k->data_width * k->data_height;
    }
    gs_max->data_size = offset;
    gs_max->block_count = (int)(offset / 64);
}

/* A batch of regions, once the coder is configured for the streams' geometry: every frame's rectangle checked against it (gj_region_plan; a
 * refusal names the frame), its origin and covers into the pinned records, its selection per scan; the largest cover and the largest selection
 * per scan of the call. 0 or -1. Nothing has been launched and nothing of the caller's output has been written when this runs. */
/* Streams of different image sizes (dec_rects::mixed; from: see batch_mixed_prepare): every frame of the family against ITS geometry; the others keep
 * the record, plan and geometry of a family frame -- the launches run over their slots too, with whatever their streams hold, and the single-frame
 * route decodes them afterwards --; g_max, the launch's geometry: the family's with the largest segment, block and sample counts among its frames. */
static int batch_regions_plan(struct gpujpeg_decoder* d, struct dec_batch* b, int from)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    const bool mixed = b->what.mixed;
    b->planned = false;
    if (mixed && batch_mixed_prepare(d, b, from) != 0) return -1;
    int ref = -1; /* mixed: a frame of the family */
    if (gj_ensure_pinned_buffer((void**)&d->bh_rgn, &d->bh_rgn_cap, (size_t)b->count * sizeof(gj_region_frame), (size_t)b->count * sizeof(gj_region_frame) * 2) != 0) return -1;
    memset(b->plan_max, 0, sizeof b->plan_max);
    struct cover_plan cp;
    memset(&cp, 0, sizeof cp);
    for (int f = 0; f < b->count; f++) {
        struct gpujpeg_image_parameters pi_f = c->param_image;
        if (mixed) {
            if (!b->fam[f]) continue;
            g = d->bh_geoms + f;
            pi_f = mixed_param_image(d, g->width, g->height);
            if (ref < 0) { ref = f; b->g_max = *g; memset(&b->g_max.fb, 0, sizeof b->g_max.fb); /* (a frame's record may carry its header record there) */ }
            if (g->segment_count > b->g_max.segment_count) b->g_max.segment_count = g->segment_count;
            if (g->block_count > b->g_max.block_count) b->g_max.block_count = g->block_count;
            if (g->data_size > b->g_max.data_size) b->g_max.data_size = g->data_size;
            for (int i = 0; i < g->comp_count && i < GJ_MAX_COMP; i++)
                if (g->comp[i].segment_count > b->g_max.comp[i].segment_count) b->g_max.comp[i].segment_count = g->comp[i].segment_count;
        }
        if (batch_cover_frame(d, b, f, g, &c->param, &pi_f, &cp, d->bh_rgn + f) != 0) return -1;
        b->gs_one = cp.gs_one; b->rg_one = cp.rg_one; b->pi_r = cp.pi_r;
        for (int sc = 0; sc < GJ_MAX_COMP; sc++) {
            const int n = b->rg_one.sel_count[sc];
            b->plan[f * GJ_MAX_COMP + sc] = n;
            if (n > b->plan_max[sc]) b->plan_max[sc] = n;
        }
    }
    if (mixed) {
        if (ref < 0) { /* (no family: nothing will be launched) */
            b->planned = true;
            return 0;
        }
        for (int f = 0; f < b->count; f++)
            if (!b->fam[f]) {
                d->bh_rgn[f] = d->bh_rgn[ref];
                d->bh_geoms[f] = d->bh_geoms[ref];
                memcpy(b->plan + (size_t)f * GJ_MAX_COMP, b->plan + (size_t)ref * GJ_MAX_COMP, GJ_MAX_COMP * sizeof(int));
            }
    }
    batch_cover_planes(&cp, g, &b->gs_max);
    b->img_w = c->param_image.width;
    b->img_h = c->param_image.height;
    b->planned = true;
    return 0;
}

/* one frame of a batch the ordinary way: into the decoder's own buffer first -- a stream that is not what the caller promised (other dimensions) must
 * not be written over the neighbours' slots --, then into its slot. `ahead`: frame 0 in front of the batched launches, which tells what every
 * frame decodes to and with that where the pixels go on the device (the output size is known once a frame has been parsed) */
static int batch_decode_one(struct gpujpeg_decoder* d, struct dec_batch* b, int f, bool ahead)
{
    struct gj_coder* c = &d->coder;
    struct gpujpeg_decoder_output o;
    gpujpeg_decoder_output_set_cuda_buffer(&o);
    /* (a batch of regions: the single-frame region call with this frame's rectangle -- the definition of the frame's result; crop-and-resize: the same
     * call with the resampling kernel as its pixel stage) */
    const struct dec_request q = batch_request(d, b, f);
    if (decoder_decode(d, &q, (uint8_t*)(uintptr_t)(b->streams + (size_t)f * b->stream_stride), b->sizes[f], &o) != 0) {
        if (q.resize) GJ_ERROR("Frame %d of the batch: crop-and-resize of the rectangle %d,%d,%d,%d failed!\n", f, q.rect[0], q.rect[1], q.rect[2], q.rect[3]);
        return -1;
    }
    if (q.resize && f < d->prescales_n) d->prescales[f] = (uint8_t)d->img.rg.frame.scale;
    if (batch_has_regions(b)) {
        if (d->region_stats[0] != 1) b->unselected = true;
        for (int i = 1; i < 4; i++) b->stats[i] += d->region_stats[i];
        /* (frame 0 ahead of everything: the streams' geometry is known now -- every rectangle is checked before a pixel goes to the caller's slots) */
        /* (a PROGRESSIVE frame 0 tells nothing of the kind about the baseline streams behind it -- its restart interval is its own, and the plan counts restart
         * segments --: the rectangles are then planned against the header the batched launches run on, batch_launches) */
        if (ahead && !b->what.mixed && d->prog_stats[0] != 0) {
            b->ahead_progressive = true;
            b->ahead_w = c->param_image.width;
            b->ahead_h = c->param_image.height;
        } else if (ahead && batch_regions_plan(d, b, 1) != 0) return -1;
        if (!ahead && b->planned && !b->what.mixed && (c->param_image.width != b->img_w || c->param_image.height != b->img_h)) {
            GJ_ERROR("Frame %d of the batch is a %dx%d image, the others %dx%d!\n", f, c->param_image.width, c->param_image.height, b->img_w, b->img_h);
            return -1;
        }
    }
    const size_t raw = dec_raw_size(d);
    if (ahead) {
        b->frame_raw = raw;
        if (b->output_stride < raw) {
            GJ_ERROR("Output stride %zu is smaller than a decoded frame (%zu B)!\n", b->output_stride, raw);
            return -1;
        }
        if (!b->out_on_device) {
            if (gj_ensure_device_buffer((void**)&d->b_raw, &d->b_raw_cap, raw * (size_t)b->count) != 0) return -1;
            b->d_out = d->b_raw;
            b->d_out_stride = raw;
        }
    } else {
        if (b->frame_raw == 0) b->frame_raw = raw;
        if (raw != b->frame_raw || raw > b->d_out_stride) {
            GJ_ERROR("A frame of the batch decodes to %zu B, the others to %zu B (output stride %zu)!\n", raw, b->frame_raw, b->d_out_stride);
            return -1;
        }
    }
    if (gj_hip_memcpy_d2d(b->d_out + (size_t)f * b->d_out_stride, o.data, raw, c->stream) != 0 || gj_hip_stream_sync(c->stream) != 0) return -1;
    return 0;
}

/* The work buffers of one chunk of frames: what a frame takes of each (into B), how many frames fit a chunk (the return value, 0 on error),
 * the buffers and the job's pointers to them. */
/* (g: the launch's geometry -- the coder's, or for streams of different image sizes the one with the family's largest counts, dec_batch::g_max;
 * min_samples: samples a frame's planes must hold at least -- the planes of the largest cover of such a batch, whose width and height come from
 * different frames, may be larger than any frame's own; planes_only: a chunk of progressive frames -- coefficient planes and, where the IDCT side wants
 * them, component planes: no segment table, no marker-scan scratch, no compacted table, no tokens, so that the memory goes to frames) */
static int batch_chunk_buffers(struct gpujpeg_decoder* d, const gj_geom* g, gj_dec_job* job, gj_batch* B, int n_all, size_t begin, size_t max_size, bool regions,
                               size_t min_samples, bool planes_only)
{
    struct gj_coder* c = &d->coder;
    const size_t S = (size_t)g->segment_count + GJ_MAX_COMP;
    const size_t seg_frame = planes_only ? 0 : (3 * S + 8 + 3) & ~(size_t)3;                                                 /* words */
    const size_t scratch_frame = planes_only ? 0 : (gj_hip_find_segments_scratch_words(begin, max_size, (uint32_t)g->segment_count) + 3) & ~(size_t)3; /* words */
    const size_t coefs_frame = ((size_t)(g->data_size > min_samples ? g->data_size : min_samples) + 63) & ~(size_t)63;   /* int16 */
    const int chunk_cap = d->b_chunk > 0 && d->b_chunk < GJ_DEC_BATCH_CHUNK_MAX ? d->b_chunk : GJ_DEC_BATCH_CHUNK_MAX;
    job->g.fb.frames = (uint32_t)(n_all < chunk_cap ? n_all : chunk_cap); /* (what the token / plane choice looks at) */
    const bool tokens = !planes_only && !d->img.resize && gj_hip_decode_wants_tokens(&job->g, max_size, &d->tune) != 0; /* (crop-and-resize: the cover planes) */
    const size_t tok_frame = tokens ? (max_size * 4 + 64 + 63) & ~(size_t)63 : 0;                                            /* tokens */
    const size_t rec_frame = tokens ? ((size_t)g->block_count + 8 + 7) & ~(size_t)7 : 0;                                    /* records */
    /* (a batch of regions: the cover planes of every configuration that does not take the token-fed region kernel, and a compacted table per frame;
     * a reduced-size batch: the reduced planes of every configuration, also of those whose full-size IDCT is fused and has none -- the token route
     * does not touch them, but whether a chunk takes it is gj_hip_decode's decision, made with the longest segment of the streams) */
    const bool planes = regions || job->scale > 1 || gj_hip_decode_uses_planes(g, job->use_fused) != 0;
    const size_t frame_bytes = seg_frame * 4 * (regions ? 2 : 1) + scratch_frame * 4 + coefs_frame * 2 + tok_frame * 2 + rec_frame * 8 + (planes ? coefs_frame : 0);
    int chunk = (int)(GJ_DEC_BATCH_BYTES / frame_bytes);
    if (chunk > chunk_cap) chunk = chunk_cap;
    if (chunk > n_all) chunk = n_all;
    if (chunk < 1) chunk = 1;
    if (!planes_only && gj_ensure_device_buffer((void**)&d->b_seg, &d->b_seg_cap, seg_frame * 4 * (size_t)chunk) != 0) return 0;
    if (!planes_only && regions && gj_ensure_device_buffer((void**)&d->b_sel, &d->b_sel_cap, seg_frame * 4 * (size_t)chunk) != 0) return 0;
    if (!planes_only && gj_ensure_device_buffer((void**)&d->b_scratch, &d->b_scratch_cap, scratch_frame * 4 * (size_t)chunk + 64) != 0) return 0;
    if (gj_ensure_device_buffer((void**)&d->b_coefs, &d->b_coefs_cap, coefs_frame * 2 * (size_t)chunk) != 0) return 0;
    if (planes && gj_ensure_device_buffer((void**)&d->b_planes, &d->b_planes_cap, coefs_frame * (size_t)chunk) != 0) return 0;
    if (planes) job->d_planes = d->b_planes;
    if (tokens) {
        if (gj_ensure_device_buffer((void**)&d->b_tok, &d->b_tok_cap, tok_frame * 2 * (size_t)chunk) != 0) return 0;
        const size_t had = d->b_rec_cap;
        if (gj_ensure_device_buffer((void**)&d->b_rec, &d->b_rec_cap, rec_frame * 8 * (size_t)chunk) != 0) return 0;
        if (d->b_rec_cap != had && gj_hip_memset(d->b_rec, 0, d->b_rec_cap, c->stream) != 0) return 0;
    }
    job->d_seg_pos = planes_only ? NULL : d->b_seg;
    job->d_seg_len = planes_only ? NULL : d->b_seg + S;
    job->d_seg_index = planes_only ? NULL : d->b_seg + 2 * S;
    job->d_coefs = d->b_coefs;
    job->tokens = tokens ? 1 : 0;
    job->d_tok = tokens ? d->b_tok : NULL;
    job->tok_cap = tokens ? (uint32_t)(max_size * 4) : 0;
    job->d_blkrec = tokens ? d->b_rec : NULL;
    B->coefs = coefs_frame;
    B->tok = tok_frame;
    B->rec = rec_frame;
    B->seg = (uint32_t)seg_frame;
    B->scratch = (uint32_t)scratch_frame;
    return chunk;
}

/* The batched launches for the frames from b->first on, if the decoder's state and the streams allow them, and every frame's verdict in
 * b->frame_done. Returns 0, -1 on error, or 1: the cached header turned out to be another sequence's -- frame 0 has to go the ordinary way
 * (which replaces the cache) and the batch is planned again (asked for only while !force_first and frame 0 has not gone ahead). */
static int batch_launches(struct gpujpeg_decoder* d, struct dec_batch* b, bool force_first)
{
    struct gj_coder* c = &d->coder;
    const gj_geom* g = &c->geom;
    const int first = b->first, count = b->count, n_all = count - first;
    const size_t* sizes = b->sizes;
    /* (the region of the decoder's own option goes frame by frame: the single-frame region kernels do not know the frame dimension; a batch of
     * regions or crop-and-resize -- batch_has_regions -- has kernels that do, and so has a reduced-size decode, dec_opt_scale) */
    const bool regions = batch_has_regions(b);
    if (regions && b->what.mixed && d->tune.dec_sub) return 0; /* (the tuning aid's sub-sequence sizes: no instantiation for frames of different sizes) */
    /* (headers of their own: every family frame brings its tables and its header's length, which batch_any_family has checked against its size) */
    const bool any = regions && b->what.mixed && b->what.any;
    bool batched = (regions || !d->region_on) && d->hdr_cache_valid && !d->need_planes && !d->host_scan && !d->tune.dec_no_spec && !d->keep_coefs && c->configured &&
                   (b->streams_on_device ? (b->stream_stride & 15u) == 0 : true) && (d->tab2_ok || any);
    size_t max_size = 0;
    for (int f = first; f < count; f++) {
        if (sizes[f] > max_size) max_size = sizes[f];
        if ((!any && sizes[f] <= d->hdr_cache_len + 2) || sizes[f] > 0x1FFFFFF0u) batched = false;
    }
    if (!batched || n_all < 1) return 0;
    dec_image_set(d, 1, NULL, NULL, NULL);
    const struct gj_reader_result* r = &d->hdr_cache_r;
    /* a scale the single call refuses for this header (a flip; packed 4:2:2 output of odd reduced width, gj_geom_init_scaled): nothing is launched,
     * the frames go the ordinary way and that call says why */
    if (d->scale > 1 && (d->flipped || (r->param_image.pixel_format == GPUJPEG_422_U8_P1020 && (GPUJPEG_AMD_SCALED_DIM(r->param_image.width, d->scale) & 1)))) return 0;
    if (decoder_configure(d, &r->param, &r->param_image) != 0) return -1; /* (the geometry of the cached header, whatever the coder was last set up for) */
    if (!regions) { /* (the image of the decoder's options -- no region among them here -- over the cached header's geometry) */
        const struct dec_request q = dec_request_options(d);
        if (dec_call_geometry(d, &q) != 0) return -1;
    }
    /* a batch of regions: the rectangles against the cached header's geometry, unless frame 0 went ahead and they have been checked against its own.
     * A rectangle the CACHED header refuses may be one the streams' own header takes (an older sequence's cache): frame 0 goes ahead and decides. */
    /* (behind a progressive frame 0 that went ahead nothing has vouched for the cached header: an older sequence's, of another size than frame 0's image
     * or with a geometry that refuses a rectangle, is no reason to fail the call -- nothing is launched, and every frame's own call decides) */
    if (regions && !b->planned && b->ahead_progressive && (r->param_image.width != b->ahead_w || r->param_image.height != b->ahead_h)) return 0;
    if (regions && !b->planned && batch_regions_plan(d, b, first) != 0) return b->ahead_progressive ? 0 : first == 0 && !force_first && !b->what.mixed ? 1 : -1;
    const bool mixed = regions && b->what.mixed;
    /* (different image sizes: no frame from here on is of the cached header's family -- an older sequence's cache: frame 0 goes ahead and decides --,
     * or nothing to launch) */
    if (mixed && b->n_fam < 1) return first == 0 && !force_first ? 1 : 0;
    /* (... or of a minority: the cached header is that of a stray frame an earlier call decoded last -- frame 0's is the better reference) */
    if (mixed && 2 * b->n_fam < n_all && first == 0 && !force_first) return 1;
    const size_t frame_raw = regions ? (size_t)b->gs_one.raw_size : dec_raw_size(d);
    if (b->output_stride < frame_raw || (b->frame_raw != 0 && b->frame_raw != frame_raw)) {
        /* the cached header is an OLDER sequence's (a larger image than the caller's slots, ADVICE r4: this used to fail the call): these
         * streams are strangers to it */
        return first == 0 && !force_first ? 1 : 0;
    }
    b->frame_raw = frame_raw;
    geom_take_tables(&c->geom, r);
    if (regions) dec_image_set(d, 1, &b->gs_one, &b->pi_r, &b->rg_one); /* (what a region call leaves: the image of one of the frames) */
    gj_dec_job job;
    dec_job_base(d, true, &job);
    if (mixed) { /* (from here on the launch's geometry: the strides of the tables and the sizes of the work buffers follow the family's largest frames) */
        g = &b->g_max;
        job.g = *g;
        memset(&job.g.fb, 0, sizeof job.g.fb); /* (a frame's record may carry its header record there: the launch's strides are set below) */
    }
    if (any) { /* (the tables: the call's pool of table sets, laid out like the decoder's own block behind d_qtab -- uploaded below, once) */
        if (b->n_sets < 1 || gj_ensure_device_buffer((void**)&d->b_tabsets, &d->b_tabsets_cap, (size_t)b->n_sets * GJ_TABSET_WORDS * sizeof(uint16_t)) != 0) return -1;
        job.d_qtab = d->b_tabsets;
        job.d_huff_tab2 = d->b_tabsets + GJ_TABSET_TAB2_OFFSET;
        job.d_qtabf = (const float*)(const void*)(d->b_tabsets + GJ_TABSET_QF_OFFSET);
    }
    job.seg_count = g->segment_count;
    job.tune.dec_careful = 0;
    job.max_seg_len = d->last_max_seg_len;
    memcpy(job.scan_bytes, d->last_scan_bytes, sizeof job.scan_bytes);
    job.jpeg_size = max_size;
    job.batch_restartless = b->restartless ? 1 : 0;
    /* (the two pointers only have to be non-null for the question; they are set per chunk below) */
    job.d_seg_count = &d->d_summary->segment_count;
    job.d_overflow = &d->h_summary->seq_overflow;
    if (!gj_hip_decode_batchable(&job)) return 0;

    /* (headers of their own: ONE part layout for the marker scan of every chunk, from the smallest first scan byte among the call's family frames -- the
     * scratch and the longest-segment words are sized for it, and every frame masks what lies in front of its own, GJ_REC_BEGIN) */
    const size_t begin = any ? b->begin_min : r->scan_begin[0];
    /* streams in host memory: one staging area, slots on 16-byte addresses */
    const uint8_t* d_streams = b->streams + (size_t)first * b->stream_stride;
    size_t d_stride = b->stream_stride;
    if (!b->streams_on_device) {
        d_stride = (max_size + 64 + 15) & ~(size_t)15;
        if (gj_ensure_device_buffer((void**)&d->b_jpeg, &d->b_jpeg_cap, d_stride * (size_t)n_all) != 0) return -1;
        gj_hip_event_record(c->timers.copy_in[0], c->stream); /* (copy marker, see gj_internal.h) */
        b->host_io = true;
        for (int f = first; f < count; f++)
            if (gj_hip_memcpy_h2d(d->b_jpeg + (size_t)(f - first) * d_stride, b->streams + (size_t)f * b->stream_stride, sizes[f], c->stream) != 0) return -1;
        d_streams = d->b_jpeg;
    }
    /* per-frame words of all frames */
    const size_t max_chunks = gj_hip_find_segments_max_chunks(begin, max_size);
    const size_t sizes_bytes = (size_t)n_all * sizeof(uint32_t), sum_bytes = (size_t)n_all * sizeof(gj_scan_summary);
    const size_t maxlen_bytes = (size_t)n_all * max_chunks * sizeof(uint32_t);
    if (gj_ensure_device_buffer((void**)&d->b_sizes, &d->b_sizes_cap, sizes_bytes) != 0) return -1;
    if (gj_ensure_pinned_buffer((void**)&d->bh_sizes, &d->bh_sizes_cap, sizes_bytes, sizes_bytes + sizes_bytes / 2) != 0) return -1;
    if (gj_ensure_pinned_buffer((void**)&d->bh_sum, &d->bh_sum_cap, sum_bytes, sum_bytes + sum_bytes / 2) != 0) return -1;
    if (gj_ensure_pinned_buffer((void**)&d->bh_maxlen, &d->bh_maxlen_cap, maxlen_bytes, maxlen_bytes + maxlen_bytes / 2) != 0) return -1;
    {
        const size_t had = d->b_dsum_cap;
        if (gj_ensure_device_buffer((void**)&d->b_dsum, &d->b_dsum_cap, sum_bytes) != 0) return -1;
        if (d->b_dsum_cap != had && gj_hip_memset(d->b_dsum, 0, d->b_dsum_cap, c->stream) != 0) return -1;
    }
    memset(d->bh_sum, 0, sum_bytes);
    for (int i = 0; i < n_all; i++) d->bh_sizes[i] = (uint32_t)sizes[first + i];
    if (gj_hip_memcpy_h2d(d->b_sizes, d->bh_sizes, sizes_bytes, c->stream) != 0) return -1;
    gj_batch B;
    memset(&B, 0, sizeof B);
    const int chunk = batch_chunk_buffers(d, g, &job, &B, n_all, begin, max_size, regions, mixed ? (size_t)b->gs_max.data_size : 0, false);
    if (chunk < 1) return -1;
    const size_t S = (size_t)g->segment_count + GJ_MAX_COMP;
    if (regions) {
        /* the per-frame records, uploaded once; ONE selection plan for all frames: the largest selection of every scan (gj_region) */
        const size_t rgn_bytes = (size_t)count * sizeof(gj_region_frame), found_bytes = (size_t)count * GJ_MAX_COMP * sizeof(uint32_t);
        if (gj_ensure_device_buffer((void**)&d->b_rgn, &d->b_rgn_cap, rgn_bytes) != 0) return -1;
        if (gj_ensure_pinned_buffer((void**)&d->bh_found, &d->bh_found_cap, found_bytes, found_bytes * 2) != 0) return -1;
        if (gj_hip_memcpy_h2d(d->b_rgn, d->bh_rgn, rgn_bytes, c->stream) != 0) return -1;
        if (mixed) { /* (every frame's geometry, once per call like the records) */
            if (gj_ensure_device_buffer((void**)&d->b_geoms, &d->b_geoms_cap, (size_t)count * sizeof(gj_geom)) != 0) return -1;
            if (gj_hip_memcpy_h2d(d->b_geoms, d->bh_geoms, (size_t)count * sizeof(gj_geom), c->stream) != 0) return -1;
        }
        if (any) { /* (the pool of table sets: one upload; every frame's header record has gone up inside its geometry record) */
            if (gj_hip_memcpy_h2d(d->b_tabsets, d->bh_tabsets, (size_t)b->n_sets * GJ_TABSET_WORDS * sizeof(uint16_t), c->stream) != 0) return -1;
        }
        memset(d->bh_found, 0xFF, found_bytes);
        if (b->restartless) { /* (what every frame's selection hands to the entropy decoder, and what that leaves unread of a restart-less scan) */
            const size_t sel_bytes = (size_t)count * sizeof(uint32_t), left_bytes = (size_t)count * GJ_MAX_COMP * sizeof(uint32_t);
            if (gj_ensure_pinned_buffer((void**)&d->bh_sel_bytes, &d->bh_sel_bytes_cap, sel_bytes, sel_bytes * 2) != 0) return -1;
            if (gj_ensure_pinned_buffer((void**)&d->bh_left, &d->bh_left_cap, left_bytes, left_bytes * 2) != 0) return -1;
            memset(d->bh_sel_bytes, 0, sel_bytes);
            memset(d->bh_left, 0, left_bytes);
        }
        job.gs = b->gs_max;
        job.region.select = 1;
        memset(&job.region.frame, 0, sizeof job.region.frame); /* (not used: d_frames) */
        memcpy(job.region.sel_count, b->plan_max, sizeof job.region.sel_count);
        job.region.d_sel = d->b_sel;
        job.region.d_sel_count = NULL;
        job.seg_count = g->segment_count; /* (entries of a frame's table at most; gj_hip_decode hands the entropy decoders the plan's) */
        selected_scan_bytes(g, b->plan_max, job.scan_bytes);
    }
    B.jpeg = d_stride;
    B.raw = b->d_out_stride;
    B.maxlen = (uint32_t)max_chunks;
    job.g.fb.jpeg = B.jpeg;
    job.g.fb.raw = B.raw;
    job.g.fb.coefs = B.coefs;
    job.g.fb.tok = B.tok;
    job.g.fb.rec = B.rec;
    job.g.fb.seg = B.seg;
    if (regions || job.scale > 1) job.gs.fb = job.g.fb; /* (the pixel kernels of a batch of regions and of a reduced-size batch take gs only) */
    for (int a = 0; a < n_all; a += chunk) {
        B.count = (uint32_t)(n_all - a < chunk ? n_all - a : chunk);
        B.d_sizes = d->b_sizes + a;
        B.d_geoms = mixed ? d->b_geoms + first + a : NULL;
        B.own_headers = any ? 1u : 0u;
        job.batch = B;
        job.g.fb.sizes = B.d_sizes;
        job.g.fb.geoms = B.d_geoms;
        if (regions || job.scale > 1) { job.gs.fb.sizes = B.d_sizes; job.gs.fb.geoms = B.d_geoms; }
        if (regions) {
            job.region.d_frames = d->b_rgn + first + a;
            job.region.scale_mask = job.region.comp_mask = 0; /* (which of the three IDCT kernels this chunk's frames need) */
            for (uint32_t i = 0; i < B.count; i++) {
                const gj_region_frame* rf = d->bh_rgn + first + a + (int)i;
                if (rf->per_comp) job.region.comp_mask |= (unsigned)rf->scale;
                else job.region.scale_mask |= (unsigned)rf->scale;
            }
            job.region.h_sel_count = d->bh_found + (size_t)(first + a) * GJ_MAX_COMP;
            job.region.h_sel_bytes = b->restartless ? d->bh_sel_bytes + first + a : NULL;
            job.region.h_left_early = b->restartless ? d->bh_left + (size_t)(first + a) * GJ_MAX_COMP : NULL;
        }
        job.d_jpeg = d_streams + (size_t)a * d_stride;
        job.d_raw = b->d_out + (size_t)(first + a) * b->d_out_stride;
        job.d_seg_count = &d->b_dsum[a].segment_count;
        job.d_overflow = &d->bh_sum[a].seq_overflow;
        uint32_t parts = 0;
        if (gj_hip_find_segments_batch(g, job.d_jpeg, begin, max_size, d->b_seg, d->b_seg + S, d->b_seg + 2 * S, (uint32_t)g->segment_count, d->b_scratch,
                                       d->b_dsum + a, mixed ? NULL : d->d_hdr_cache, mixed ? 0u : (uint32_t)d->hdr_cache_len, d->bh_sum + a, d->bh_maxlen + (size_t)a * max_chunks,
                                       (uint32_t)max_chunks, &parts, c->stream, &d->tune, &B) != 0 ||
            gj_hip_decode(&job, c->stream, NULL) != 0) {
            GJ_ERROR("Decoder kernels failed: %s\n", gj_hip_last_error());
            return -1;
        }
        d->maxlen_parts = parts;
    }
    if (gj_hip_stream_sync(c->stream) != 0) {
        GJ_ERROR("Decoder failed: %s\n", gj_hip_last_error());
        return -1;
    }
    if (regions || job.scale > 1) c->kernel_ms[4] = (float)d->last_idct_path; /* (which IDCT side the batched launches took, gpujpeg_amd_ext.h) */
    /* every frame's summary: was the stream what the launch assumed? */
    int accepted = 0;
    for (int i = 0; i < n_all; i++) {
        gj_scan_summary* su = d->bh_sum + i;
        summary_take_maxlen(su, d->bh_maxlen + (size_t)i * max_chunks, d->maxlen_parts);
        /* (different image sizes: the family's frames alone -- the host compared their headers --, each against its OWN segment count and scans) */
        if (mixed && !b->fam[first + i]) continue;
        const gj_geom* gf = mixed ? d->bh_geoms + first + i : g;
        /* (headers of their own: the rule against the frame's OWN ids and selectors) */
        if (any ? !spec_summary_ok_own(&b->sel[first + i], su, gf) : !spec_summary_ok(d, su, gf)) continue;
        if (regions) { /* did the selection find in this stream's table what the plan took from the geometry? (cannot fail for a stream the rule accepts) */
            const int f = first + i;
            if (memcmp(d->bh_found + (size_t)f * GJ_MAX_COMP, b->plan + (size_t)f * GJ_MAX_COMP, GJ_MAX_COMP * sizeof(uint32_t)) != 0) continue;
            const gj_region_frame* rf = d->bh_rgn + f;
            for (int sc = 0; sc < GJ_MAX_COMP; sc++) b->stats[1] += b->plan[f * GJ_MAX_COMP + sc];
            for (int k = 0; k < g->comp_count && k < GJ_MAX_COMP; k++) b->stats[2] += (long)(rf->bx1[k] - rf->bx0[k]) * (rf->by1[k] - rf->by0[k]);
            b->stats[3] += (long)su->segment_count;
        }
        b->frame_done[first + i] = 1;
        accepted++;
        if (b->restartless) { /* (gpujpeg_amd_decoder_get_entropy_bytes: the table lengths of the frame's segments -- its scans without their restart markers --, or of its selection) */
            uint64_t handed = 0, left = 0;
            if (regions) {
                handed = d->bh_sel_bytes[first + i];
                for (int sc = 0; sc < GJ_MAX_COMP; sc++) left += d->bh_left[(size_t)(first + i) * GJ_MAX_COMP + sc];
            } else {
                for (int sc = 0; sc < (int)su->scan_count && sc < GJ_MAX_COMP; sc++) handed += su->scan_end[sc] - su->scan_start[sc];
                handed -= 2u * (uint64_t)su->rst_count;
            }
            d->entropy_bytes[0] += handed;
            d->entropy_bytes[1] += handed - (left < handed ? left : handed);
        }
        /* (what the next launch on this header plans with: a frame of the cached header's own dimensions) */
        /* (headers of their own: and of the cached header's own bytes -- what a "mixed" call would have remembered, no more) */
        if (!mixed || (gf->width == c->geom.width && gf->height == c->geom.height && (!any || (b->fam[first + i] & 2)))) remember_summary(d, su);
    }
    /* not one frame passed: the cached header (an older sequence's, of dimensions the slots happen to hold) is not these streams' */
    return accepted == 0 && first == 0 && !force_first ? 1 : 0;
}

/* ---- groups of progressive frames through batched launches (dec_opt_batch_progressive, gpujpeg_amd_ext.h) ---- */
/* a frame of the call that is still undecoded when the pass runs */
struct prog_cand {
    int f;                         /* frame of the call */
    const uint8_t* himage;        /* its whole stream in host memory: the host walks every scan, as dec_progressive does */
    struct gj_reader_result r;
    struct gj_prog_info info;
};
/* the progressive candidates that agree in everything the stages behind the coefficient planes read (prog_same_group) */
struct prog_group {
    int n; int* member;            /* indices into the candidates, ascending frames */
    struct gpujpeg_parameters param; /* the first member's, restart interval 0: the restart intervals are the records' */
    gj_geom g;
    size_t max_size;               /* the longest stream */
    struct cover_plan cp; gj_geom gs_max; gj_region_frame* rf; /* a call with rectangles: every member's against g, the planes of the largest cover */
};

static size_t prog_align16(size_t n) { return (n + 15) & ~(size_t)15; }

/* width and height, component count, ids and sampling, what the reader made of APPn / Adobe / JFIF (its colour-space and pixel-format decisions), and
 * per component the CONTENTS of its quantisation table. Huffman tables, scan scripts and restart intervals may differ. */
static bool prog_same_group(const struct gj_reader_result* a, const struct gj_reader_result* b)
{
    struct gpujpeg_parameters pa = a->param, pb = b->param;
    pa.restart_interval = pb.restart_interval = 0;
    if (!gj_parameters_equal(&pa, &pb) || !gj_image_parameters_equal(&a->param_image, &b->param_image) || a->header_color_space != b->header_color_space) return false;
    for (int i = 0; i < a->param.comp_count && i < GJ_MAX_COMP; i++)
        if (a->comp_id[i] != b->comp_id[i] || memcmp(a->qraw[a->quant_map[i]], b->qraw[b->quant_map[i]], 64) != 0) return false;
    return true;
}

/* the frame header of a stream, from its first n bytes alone: 1 = SOF2, 0 = another one (or a scan, or the end, ahead of any), -1 = not within these
 * bytes or not a marker sequence -- what spares the pass the parse, and a device-resident stream the copy, of a frame that is not progressive */
#define GJ_PROG_SNIFF_BYTES 1024
static int prog_sniff(const uint8_t* p, size_t n)
{
    if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return -1;
    size_t at = 2;
    while (at + 4 <= n) {
        if (p[at] != 0xFF) return -1;
        const unsigned m = p[at + 1];
        if (m == 0xFF) { at++; continue; } /* (fill bytes) */
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) return m == 0xC2 ? 1 : 0;
        if (m == 0xDA || m == 0xD9) return 0;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { at += 2; continue; } /* (markers without a length) */
        at += 2 + (((size_t)p[at + 2] << 8) | p[at + 3]);
    }
    return -1;
}

/* inside a level the longest serial walks start first (ties: by frame and position, so that the order is one) */
static int prog_longest_first(const void* pa, const void* pb)
{
    const gj_prog_rec* a = pa;
    const gj_prog_rec* b = pb;
    if (a->len != b->len) return a->len > b->len ? -1 : 1;
    if (a->frame != b->frame) return a->frame < b->frame ? -1 : 1;
    return a->pos < b->pos ? -1 : a->pos > b->pos ? 1 : 0;
}

/* One group: the coder configured for its geometry, its quantisation tables, the table pools, per-frame records and work lists of all its frames in one
 * pinned buffer with one upload, its host streams staged once, then per chunk of frames one gj_hip_decode -- the chunk's planes cleared, one entropy
 * launch per level, the IDCT side of a baseline batch --, and one wait. 0 (frame_done set for the members; or nothing done: a group whose frames do not
 * fit the caller's slots goes the single-frame route, which says so) or -1. */
static int batch_progressive_group(struct gpujpeg_decoder* d, struct dec_batch* b, struct prog_cand* cand, const struct prog_group* G)
{
    struct gj_coder* c = &d->coder;
    const bool regions = batch_has_regions(b);
    const int n = G->n;
    const struct gj_reader_result* r0 = &cand[G->member[0]].r;
    if (decoder_configure(d, &G->param, &r0->param_image) != 0) return -1;
    if (regions) {
        dec_image_set(d, 1, &G->cp.gs_one, &G->cp.pi_r, &G->cp.rg_one); /* (what a region call leaves: the image of one of the frames) */
    } else {
        const struct dec_request q = dec_request_options(d);
        if (dec_call_geometry(d, &q) != 0) return -1;
    }
    const size_t frame_raw = regions ? (size_t)G->cp.gs_one.raw_size : dec_raw_size(d);
    if (b->output_stride < frame_raw || (b->frame_raw != 0 && b->frame_raw != frame_raw)) return 0;
    b->frame_raw = frame_raw;
    for (int i = 0; i < c->geom.comp_count; i++) {
        c->geom.comp[i].q_table = r0->quant_map[i];
        c->geom.comp[i].dc_table = c->geom.comp[i].ac_table = 0;
    }
    if (prog_quant_tables(d, r0) != 0) return -1;
    gj_dec_job job;
    dec_job_base(d, false, &job);
    job.d_qtab = d->d_prog_q;
    job.d_qtabf = (const float*)(const void*)(d->d_prog_q + 4 * 64);
    job.jpeg_size = G->max_size;
    gj_batch B;
    memset(&B, 0, sizeof B);
    const int chunk = batch_chunk_buffers(d, &c->geom, &job, &B, n, 0, G->max_size, regions, 0, true); /* (planes, no tokens, no segment table) */
    if (chunk < 1) return -1;
    const int chunks = (n + chunk - 1) / chunk;

    /* the one upload: table pools | per-frame records | rectangles | stream sizes | work lists */
    size_t pool_total = 0, rec_total = 0;
    for (int i = 0; i < n; i++) {
        pool_total += (size_t)cand[G->member[i]].info.pool_count;
        rec_total += (size_t)cand[G->member[i]].info.segs.count;
    }
    const size_t tab_bytes = prog_align16(pool_total * GJ_DEC_TAB_WORDS * sizeof(uint16_t)), pf_bytes = prog_align16((size_t)n * sizeof(gj_prog_frame));
    const size_t rf_bytes = regions ? prog_align16((size_t)n * sizeof(gj_region_frame)) : 0, sz_bytes = prog_align16((size_t)n * sizeof(uint32_t));
    const size_t rec_at = tab_bytes + pf_bytes + rf_bytes + sz_bytes, bytes = rec_at + (rec_total + 1) * sizeof(gj_prog_rec);
    if (gj_ensure_pinned_buffer((void**)&d->h_prog, &d->h_prog_cap, bytes, bytes + bytes / 2) != 0) return -1;
    if (gj_ensure_device_buffer((void**)&d->d_prog, &d->d_prog_cap, bytes) != 0) return -1;
    memset(d->h_prog, 0, bytes);
    gj_prog_frame* pf = (gj_prog_frame*)(void*)(d->h_prog + tab_bytes);
    uint32_t* sz = (uint32_t*)(void*)(d->h_prog + tab_bytes + pf_bytes + rf_bytes);
    gj_prog_rec* recs = (gj_prog_rec*)(void*)(d->h_prog + rec_at);
    if (regions) memcpy(d->h_prog + tab_bytes + pf_bytes, G->rf, (size_t)n * sizeof(gj_region_frame));
    /* streams in host memory: one staging area, slots on 16-byte addresses; device-resident ones are read where they lie */
    const size_t slot = prog_align16(G->max_size + 64);
    if (!b->streams_on_device) {
        if (gj_ensure_device_buffer((void**)&d->b_jpeg, &d->b_jpeg_cap, slot * (size_t)n) != 0) return -1;
        b->host_io = true;
    }
    size_t tab = 0;
    for (int i = 0; i < n; i++) {
        const struct prog_cand* k = &cand[G->member[i]];
        for (int t = 0; t < k->info.pool_count; t++)
            if (gj_huffman_decoder_table(k->info.pool[t].bits, k->info.pool[t].vals, (uint16_t*)(void*)d->h_prog + (tab + (size_t)t) * GJ_DEC_TAB_WORDS) != 0) {
                GJ_ERROR("Invalid Huffman table in a progressive scan!\n");
                return -1;
            }
        pf[i].stream = b->streams_on_device ? (uint64_t)k->f * b->stream_stride : (uint64_t)i * slot;
        pf[i].size = (uint32_t)b->sizes[k->f];
        pf[i].tab_first = (uint32_t)tab;
        pf[i].coef_block = (uint64_t)(i % chunk) * (B.coefs / 64);
        sz[i] = pf[i].size;
        tab += (size_t)k->info.pool_count;
        if (!b->streams_on_device && gj_hip_memcpy_h2d(d->b_jpeg + (size_t)i * slot, k->himage, b->sizes[k->f], c->stream) != 0) return -1;
    }
    /* the work list of every chunk: level l of ALL its frames back to back, the longest segments first */
    gj_prog_plan* plans = calloc((size_t)chunks, sizeof *plans);
    if (!plans) return -1;
    uint32_t at = 0;
    long launches = 0;
    for (int ch = 0; ch < chunks; ch++) {
        gj_prog_plan* P = &plans[ch];
        const int a = ch * chunk, m = n - a < chunk ? n - a : chunk;
        for (int i = 0; i < m; i++)
            if (cand[G->member[a + i]].info.levels > P->levels) P->levels = cand[G->member[a + i]].info.levels;
        for (int level = 0; level < P->levels && level < GJ_PROG_MAX_SCANS; level++) {
            P->level_first[level] = at;
            for (int i = 0; i < m; i++) at += prog_level_records(&cand[G->member[a + i]].info, &c->geom, level, (unsigned)i, recs + at);
            P->level_count[level] = at - P->level_first[level];
            qsort(recs + P->level_first[level], P->level_count[level], sizeof *recs, prog_longest_first);
            if (P->level_count[level] > 0) launches++;
        }
        P->d_recs = (const gj_prog_rec*)(const void*)(d->d_prog + rec_at);
        P->d_tabs = (const uint16_t*)(const void*)d->d_prog;
        P->tab_count = (uint32_t)pool_total;
        P->d_frames = (const gj_prog_frame*)(const void*)(d->d_prog + tab_bytes) + a;
    }
    int rc = gj_hip_memcpy_h2d(d->d_prog, d->h_prog, rec_at + (size_t)at * sizeof(gj_prog_rec), c->stream);
    const uint32_t* d_sizes = (const uint32_t*)(const void*)(d->d_prog + tab_bytes + pf_bytes + rf_bytes);
    const gj_region_frame* d_rf = (const gj_region_frame*)(const void*)(d->d_prog + tab_bytes + pf_bytes);
    const size_t praw = prog_align16(frame_raw);
    job.d_jpeg = b->streams_on_device ? b->streams : d->b_jpeg;
    job.g.fb.jpeg = B.jpeg = b->streams_on_device ? b->stream_stride : slot; /* (not read: every frame's record says where its stream lies) */
    job.g.fb.coefs = B.coefs;
    if (regions) {
        job.gs = G->gs_max;
        job.region.select = 0; /* (every segment of every scan is decoded) */
        job.region.d_sel = NULL;
        job.region.d_sel_count = job.region.h_sel_count = NULL;
        memset(&job.region.frame, 0, sizeof job.region.frame); /* (not used: d_frames) */
    }
    for (int ch = 0; ch < chunks && rc == 0; ch++) {
        const int a = ch * chunk, m = n - a < chunk ? n - a : chunk;
        /* where the pixels go: the caller's slots where the chunk's frames lie a constant distance apart, else back to back and copied there */
        const int f0 = cand[G->member[a]].f, step = m > 1 ? cand[G->member[a + 1]].f - f0 : 1;
        bool strided = true;
        for (int i = 1; i < m; i++) strided = strided && cand[G->member[a + i]].f - cand[G->member[a + i - 1]].f == step;
        if (!strided && gj_ensure_device_buffer((void**)&d->b_praw, &d->b_praw_cap, praw * (size_t)chunk) != 0) { rc = -1; break; }
        B.count = (uint32_t)m;
        B.raw = strided ? (uint64_t)step * b->d_out_stride : praw;
        B.d_sizes = d_sizes + a;
        job.batch = B;
        job.g.fb.sizes = B.d_sizes;
        job.g.fb.raw = B.raw;
        job.g.fb.frames = (uint32_t)m;
        if (regions || job.scale > 1) job.gs.fb = job.g.fb; /* (the pixel kernels of a batch of regions and of a reduced-size batch take gs only) */
        if (regions) {
            job.region.d_frames = d_rf + a;
            job.region.scale_mask = job.region.comp_mask = 0; /* (which of the three IDCT kernels this chunk's frames need) */
            for (int i = 0; i < m; i++) {
                if (G->rf[a + i].per_comp) job.region.comp_mask |= (unsigned)G->rf[a + i].scale;
                else job.region.scale_mask |= (unsigned)G->rf[a + i].scale;
            }
        }
        job.d_raw = strided ? b->d_out + (size_t)f0 * b->d_out_stride : d->b_praw;
        job.prog = &plans[ch];
        if (!gj_hip_decode_batchable(&job) || gj_hip_decode(&job, c->stream, NULL) != 0) {
            GJ_ERROR("Decoder kernels failed: %s\n", gj_hip_last_error());
            rc = -1;
        }
        for (int i = 0; i < m && rc == 0 && !strided; i++)
            rc = gj_hip_memcpy_d2d(b->d_out + (size_t)cand[G->member[a + i]].f * b->d_out_stride, d->b_praw + (size_t)i * praw, frame_raw, c->stream);
    }
    if (gj_hip_stream_sync(c->stream) != 0 && rc == 0) {
        GJ_ERROR("Decoder failed: %s\n", gj_hip_last_error());
        rc = -1;
    }
    free(plans);
    if (rc != 0) return -1;
    if (regions || job.scale > 1) c->kernel_ms[4] = (float)d->last_idct_path; /* (which IDCT side the batched launches took, gpujpeg_amd_ext.h) */
    for (int i = 0; i < n; i++) {
        const struct prog_cand* k = &cand[G->member[i]];
        b->frame_done[k->f] = 1;
        if (regions) { /* (gpujpeg_amd_decoder_get_region_stats: what the frame's own region call reports -- every segment decoded, its cover's blocks) */
            const gj_region_frame* rf = &G->rf[i];
            b->unselected = true;
            b->stats[1] += (long)k->info.segs.count;
            b->stats[3] += (long)k->info.segs.count;
            for (int q = 0; q < c->geom.comp_count && q < GJ_MAX_COMP; q++) b->stats[2] += (long)(rf->bx1[q] - rf->bx0[q]) * (rf->by1[q] - rf->by0[q]);
        }
    }
    d->pb_stats[0] += n;
    d->pb_stats[1] += 1;
    d->pb_stats[2] += launches;
    d->pb_stats[3] += (long)at;
    return 0;
}

/* The pass of a batch call between the baseline batched launches and the single-frame route: the candidates -- the frames still undecoded -- are brought
 * to the host whole (device-resident streams: every copy queued, ONE wait) and parsed (gj_reader_parse + gj_reader_parse_progressive); the progressive
 * ones the parser takes form groups (prog_same_group; with rectangles: every member's rectangle planned against the group's geometry, a refusal names
 * the frame and fails the call before a group has written anything), and every group of two or more runs through batch_progressive_group, one after the
 * other. Everything else stays undecoded for the single-frame route, which gives it the message and return code it always had. The header cache and
 * what the speculative launches remember (remember_summary) are neither read nor written. Frames of different image sizes are different groups:
 * per-frame geometry inside one set of progressive launches is not built. 0 or -1. */
static int batch_progressive(struct gpujpeg_decoder* d, struct dec_batch* b)
{
    struct gj_coder* c = &d->coder;
    const bool regions = batch_has_regions(b);
    /* (a decoder state in which the baseline batched launches decline too: every frame goes the single-frame route) */
    if ((!regions && d->region_on) || d->keep_coefs || !d->use_fused || d->flipped || d->channel_remap || d->host_scan || d->tune.dec_no_spec) return 0;
    int left = 0;
    for (int f = 0; f < b->count; f++)
        if (!b->frame_done[f]) {
            if (b->sizes[f] < 4 || b->sizes[f] > 0x7FFFFFF0u) return 0;
            left++;
        }
    if (left < 2) return 0;
    /* a look at the frame header first: a baseline frame that is left (a call whose progressive frame 0 left no header to launch on has many) is neither
     * copied to the host nor parsed. Device-resident streams: the first bytes of all of them by ONE gather launch */
    const uint8_t* heads = b->streams;
    size_t head_stride = b->stream_stride;
    if (b->streams_on_device) {
        const size_t sizes_bytes = (size_t)b->count * sizeof(uint32_t), hdr_bytes = (size_t)b->count * GJ_PROG_SNIFF_BYTES;
        if (gj_ensure_device_buffer((void**)&d->b_sizes, &d->b_sizes_cap, sizes_bytes) != 0) return -1;
        if (gj_ensure_pinned_buffer((void**)&d->bh_sizes, &d->bh_sizes_cap, sizes_bytes, sizes_bytes + sizes_bytes / 2) != 0) return -1;
        if (gj_ensure_pinned_buffer((void**)&d->bh_hdrs, &d->bh_hdrs_cap, hdr_bytes, hdr_bytes * 2) != 0) return -1;
        for (int f = 0; f < b->count; f++) d->bh_sizes[f] = (uint32_t)b->sizes[f];
        if (gj_hip_memcpy_h2d(d->b_sizes, d->bh_sizes, sizes_bytes, c->stream) != 0 ||
            gj_hip_gather_headers(b->streams, b->stream_stride, d->b_sizes, (uint32_t)b->count, GJ_PROG_SNIFF_BYTES, d->bh_hdrs, c->stream) != 0 ||
            gj_hip_stream_sync(c->stream) != 0) {
            GJ_ERROR("Reading the headers of the batch failed: %s\n", gj_hip_last_error());
            return -1;
        }
        heads = d->bh_hdrs;
        head_stride = GJ_PROG_SNIFF_BYTES;
    }
    struct prog_cand* cand = calloc((size_t)left, sizeof *cand);
    struct prog_group* groups = calloc((size_t)left, sizeof *groups);
    int ncand = 0, ngroups = 0, rc = -1;
    if (!cand || !groups) goto out;
    for (int f = 0; f < b->count; f++) {
        const size_t seen = b->streams_on_device && b->sizes[f] > GJ_PROG_SNIFF_BYTES ? GJ_PROG_SNIFF_BYTES : b->sizes[f];
        if (b->frame_done[f] || prog_sniff(heads + (size_t)f * head_stride, seen) == 0) continue; /* (1, or not told by these bytes: the parse decides) */
        cand[ncand].f = f;
        cand[ncand++].himage = b->streams + (size_t)f * b->stream_stride;
    }
    if (ncand < 2) { rc = 0; goto out; }
    if (b->streams_on_device) {
        /* a RUN of neighbouring candidates comes with one copy of everything from its first stream to the end of its last -- 255 frames of a dataset
         * are one submission, not 255 --, unless the gaps between the streams would more than double what is copied */
        size_t bytes = 0;
        for (int pass = 0; pass < 2; pass++) { /* (0: the size of the pinned buffer, 1: the copies) */
            size_t at = 0;
            for (int k = 0; k < ncand;) {
                int e = k + 1;
                size_t sum = b->sizes[cand[k].f];
                while (e < ncand && cand[e].f == cand[e - 1].f + 1) sum += b->sizes[cand[e++].f];
                const size_t span = (size_t)(e - 1 - k) * b->stream_stride + b->sizes[cand[e - 1].f];
                if (e - k > 1 && span > 2 * sum + 4096) e = k + 1; /* (streams far apart: one by one) */
                const size_t n = e - k > 1 ? span : b->sizes[cand[k].f];
                if (pass == 1) {
                    if (gj_hip_memcpy_d2h(d->bh_pstreams + at, b->streams + (size_t)cand[k].f * b->stream_stride, n, c->stream) != 0) goto out;
                    for (int i = k; i < e; i++) cand[i].himage = d->bh_pstreams + at + (size_t)(i - k) * b->stream_stride;
                }
                at += prog_align16(n);
                k = e;
            }
            bytes = at;
            if (pass == 0 && gj_ensure_pinned_buffer((void**)&d->bh_pstreams, &d->bh_pstreams_cap, bytes, bytes + bytes / 2) != 0) goto out;
        }
        if (gj_hip_stream_sync(c->stream) != 0) goto out;
    }
    /* the groups: a candidate joins the first group it agrees with */
    for (int k = 0; k < ncand; k++) {
        struct prog_cand* q = &cand[k];
        const size_t size = b->sizes[q->f];
        if (gj_reader_parse(q->himage, size, GPUJPEG_LL_QUIET - 1, d->ff_cs_itu601_is_709, d->req_pixel_format, d->req_color_space, d->req_alignment, &q->r, true, true) != 0 ||
            !q->r.progressive || q->r.scan_begin[0] >= size)
            continue;
        if (gj_reader_parse_progressive(q->himage, size, &q->r, &q->info, true) != 0 || q->info.bad_scan != 0 || q->info.levels > GJ_PROG_MAX_SCANS) continue;
        bool tables = true;
        for (int i = 0; i < q->r.param.comp_count; i++)
            if (q->r.quant_map[i] < 0 || q->r.quant_map[i] > 3 || !q->r.q_present[q->r.quant_map[i]]) tables = false;
        if (!tables) continue;
        int gi = 0;
        while (gi < ngroups && !prog_same_group(&cand[groups[gi].member[0]].r, &q->r)) gi++;
        struct prog_group* G = &groups[gi];
        if (gi == ngroups) {
            G->member = calloc((size_t)ncand, sizeof *G->member);
            if (!G->member) goto out;
            ngroups++;
        }
        G->member[G->n++] = k;
        if (size > G->max_size) G->max_size = size;
    }
    /* every group's geometry; a call with rectangles: every member's rectangle against it, before any group is launched */
    for (int gi = 0; gi < ngroups; gi++) {
        struct prog_group* G = &groups[gi];
        if (G->n < 2) continue;
        const struct gj_reader_result* r0 = &cand[G->member[0]].r;
        G->param = r0->param;
        G->param.restart_interval = 0;
        /* (what the single call refuses for this image: nothing is launched, the frames go the ordinary way and that call says why) */
        const int w = r0->param_image.width, s = d->scale > 1 ? d->scale : 1;
        bool refused = gj_geom_init(&G->g, &G->param, &r0->param_image, false) != 0;
        if (!refused && !regions) refused = r0->param_image.pixel_format == GPUJPEG_422_U8_P1020 && ((s > 1 ? GPUJPEG_AMD_SCALED_DIM(w, s) : w) & 1);
        /* (a call whose rectangles have been checked against the baseline frames' image: a frame of another size fails that call, as ever) */
        if (!refused && regions && b->planned && !b->what.mixed) refused = w != b->img_w || r0->param_image.height != b->img_h;
        if (refused) { G->n = 0; continue; }
        if (!regions) continue;
        G->rf = calloc((size_t)G->n, sizeof *G->rf);
        if (!G->rf) goto out;
        for (int i = 0; i < G->n; i++)
            if (batch_cover_frame(d, b, cand[G->member[i]].f, &G->g, &G->param, &r0->param_image, &G->cp, G->rf + i) != 0) goto out;
        batch_cover_planes(&G->cp, &G->g, &G->gs_max);
    }
    for (int gi = 0; gi < ngroups; gi++)
        if (groups[gi].n >= 2 && batch_progressive_group(d, b, cand, &groups[gi]) != 0) goto out;
    rc = 0;
out:
    for (int gi = 0; groups && gi < ngroups; gi++) { free(groups[gi].member); free(groups[gi].rf); }
    for (int k = 0; cand && k < ncand; k++) gj_prog_info_free(&cand[k].info);
    free(groups);
    free(cand);
    return rc;
}

/* the batch call proper; what: the rectangles of a batch of regions or of crop-and-resize, or NULL */
static int decode_batch(struct gpujpeg_decoder* d, const uint8_t* streams, size_t stream_stride, const size_t* sizes, int count, const struct dec_rects* what,
                        uint8_t* output, size_t output_stride, struct gpujpeg_image_parameters* param_image)
{
    struct gj_coder* c = &d->coder;
    struct dec_batch b = {.streams = streams, .stream_stride = stream_stride, .sizes = sizes, .count = count, .output_stride = output_stride,
                          .d_out = output, .d_out_stride = output_stride};
    if (what) b.what = *what;
    b.restartless = d->batch_restartless != 0; /* (the option as it is when the call starts) */
    d->entropy_valid = d->pb_stats_valid = d->hdr_stats_valid = false;
    d->entropy_bytes[0] = d->entropy_bytes[1] = 0;
    b.prog_batch = d->batch_progressive != 0 && d->progressive != 0; /* (both options as they are when the call starts) */
    memset(d->pb_stats, 0, sizeof d->pb_stats);
    const bool regions = batch_has_regions(&b);
    b.streams_on_device = gj_hip_is_device_ptr(streams) != 0;
    b.out_on_device = gj_hip_is_device_ptr(output) != 0;
    int rc = -1;
    b.frame_done = calloc((size_t)count, 1);
    if (regions) b.plan = calloc((size_t)count * GJ_MAX_COMP, sizeof(int));
    if (regions && b.what.mixed) b.fam = calloc((size_t)count, 1);
    if (regions && b.what.mixed && b.what.any) b.sel = calloc((size_t)count, sizeof *b.sel);
    if (!b.frame_done || (regions && !b.plan) || (regions && b.what.mixed && !b.fam) || (regions && b.what.mixed && b.what.any && !b.sel)) goto out;
    /* The header cache is what a batch launches on: frame 0 goes the ordinary way when there is none (or when it has to). A second pass, with
     * force_first, when the cached header turned out to be another sequence's: frame 0 replaces the cache, then the batch. */
    for (int pass = 0; pass < 2; pass++) {
        const bool force_first = pass == 1;
        if (b.first == 0 && (!b.out_on_device || !d->hdr_cache_valid || force_first)) {
            if (batch_decode_one(d, &b, 0, true) != 0) goto out;
            b.frame_done[0] = 1;
            b.first = 1;
        }
        const int again = batch_launches(d, &b, force_first);
        if (again < 0) goto out;
        if (again == 0) break;
        b.frame_raw = 0;
        b.planned = false;
        b.prepared = false;
    }
    /* a batch of regions none of whose rectangles has been looked at (nothing has been launched: no header to launch on that these streams share,
     * or a decoder state without batched launches): frame 0 the ordinary way tells the streams' geometry, and every rectangle is checked against it
     * before the first pixel goes to the caller's slots */
    if (regions && !b.planned && b.first == 0) {
        if (batch_decode_one(d, &b, 0, true) != 0) goto out;
        b.frame_done[0] = 1;
        b.first = 1;
    }
    /* the progressive frames among what is left, where they form groups (dec_opt_batch_progressive) */
    if (b.prog_batch && batch_progressive(d, &b) != 0) goto out;
    /* whatever is left: the ordinary call, frame by frame */
    d->b_last_batched = 0;
    for (int f = b.first; f < count; f++) d->b_last_batched += b.frame_done[f] ? 1 : 0;
    d->b_last_single = count - d->b_last_batched;
    for (int f = 0; f < count; f++)
        if (!b.frame_done[f] && batch_decode_one(d, &b, f, false) != 0) goto out;
    if (!b.out_on_device) {
        gj_hip_event_record(c->timers.copy_out[0], c->stream); /* (copy marker) */
        const gj_stream_t down = gj_hip_lane_begin(1, b.frame_raw, c->stream); /* (the process's download lane for frames of 1 MiB and more) */
        b.host_io = true;
        int copies = 0;
        for (int f = 0; f < count && copies == 0; f++)
            copies = gj_hip_memcpy_d2h(output + (size_t)f * output_stride, b.d_out + (size_t)f * b.d_out_stride, b.frame_raw, down);
        /* (a copy that could not be queued: the ones before it are still on their way INTO THE CALLER'S BUFFERS -- the lane is waited for here,
         * the coder's stream at the exit) */
        if (gj_hip_lane_end(down, c->stream, c->timers.lane_out) != 0 || copies != 0 || gj_hip_stream_sync(c->stream) != 0) goto out;
    }
    if (param_image) *param_image = dec_out_param_image(d);
    if (regions) { /* (gpujpeg_amd_decoder_get_region_stats of the call: sums over its frames) */
        b.stats[0] = b.unselected ? 2 : 1;
        memcpy(d->region_stats, b.stats, sizeof d->region_stats);
    }
    d->entropy_valid = b.restartless;
    d->pb_stats_valid = b.prog_batch;
    /* (gpujpeg_amd_decoder_get_batch_header_stats: what the last look at the call's headers found; none -- a decoder state without batched launches -- zeros) */
    d->hdr_stats_valid = regions && b.what.mixed && b.what.any;
    if (d->hdr_stats_valid && !b.prepared) { memset(d->hdr_stats, 0, sizeof d->hdr_stats); memset(d->hdr_ms, 0, sizeof d->hdr_ms); }
    rc = 0; /* (c->frames counts the frames TIMED with perf_stats, src/gpujpeg_common.c:2238-2254: a batch adds none) */
out:
    if (rc != 0 && b.host_io) gj_hip_stream_sync(c->stream); /* (what is queued on the stream must not read the caller's streams or write its frames after the error has left) */
    free(b.frame_done);
    free(b.plan);
    free(b.fam);
    free(b.sel);
    return rc;
}

int gpujpeg_amd_decoder_decode_batch(struct gpujpeg_decoder* d, const uint8_t* streams, size_t stream_stride, const size_t* sizes, int count,
                                     uint8_t* output, size_t output_stride, struct gpujpeg_image_parameters* param_image)
{
    if (!d || !streams || !sizes || count < 1 || !output) return -1;
    return decode_batch(d, streams, stream_stride, sizes, count, NULL, output, output_stride, param_image);
}

/* A batch of regions: one width x height rectangle per frame, each at its own origin. The decoder's own dec_opt_region is neither read nor changed
 * (frames that go the ordinary way have their rectangle in their call's request). */
int gpujpeg_amd_decoder_decode_batch_regions(struct gpujpeg_decoder* d, const uint8_t* streams, size_t stream_stride, const size_t* sizes, int count,
                                             const int* origins, int width, int height, uint8_t* output, size_t output_stride,
                                             struct gpujpeg_image_parameters* param_image)
{
    if (!d || !streams || !sizes || count < 1 || !output || !origins) return -1;
    d->entropy_valid = d->pb_stats_valid = d->hdr_stats_valid = false;
    if (width < 1 || height < 1) {
        GJ_ERROR("A batch of regions needs a width and a height of at least 1 (given: %d x %d)!\n", width, height);
        return -1;
    }
    if (d->scale > 1) {
        GJ_ERROR("A batch of regions is not available together with " GPUJPEG_AMD_DEC_OPT_SCALE "=1/%d!\n", d->scale);
        return -1;
    }
    if (d->flipped) {
        GJ_ERROR("A batch of regions is not available together with " GPUJPEG_DEC_OPT_FLIPPED_BOOL "!\n");
        return -1;
    }
    const struct dec_rects what = {.origins = origins, .rw = width, .rh = height};
    return decode_batch(d, streams, stream_stride, sizes, count, &what, output, output_stride, param_image);
}

/* Crop-and-resize: one rectangle per frame, each with its own size, resampled to ONE out_width x out_height image per frame (bilinear, gj_resize_taps),
 * optionally mirrored. A batch of regions whose pixel stage resamples: the same plan, selection, entropy decoders and k_idct_region_batch -- always
 * through the cover planes --, then k_resize_region_batch. As for the batch of regions, the decoder's own dec_opt_region is neither read nor changed. */
/* (tensor: NULL, or what gpujpeg_amd_decoder_decode_batch_crop_resize_tensor checked -- the same call with another store in its pixel stage) */
static int decode_batch_crop_resize(struct gpujpeg_decoder* d, const uint8_t* streams, size_t stream_stride, const size_t* sizes, int count, const int* rects,
                                    const uint8_t* mirror, int out_width, int out_height, const gj_tensor* tensor, uint8_t* output, size_t output_stride,
                                    struct gpujpeg_image_parameters* param_image)
{
    if (!d || !streams || !sizes || count < 1 || !output || !rects) return -1;
    d->entropy_valid = d->pb_stats_valid = d->hdr_stats_valid = false;
    d->prescales_n = 0;
    if (out_width < 1 || out_height < 1 || out_width > 16384 || out_height > 16384) {
        GJ_ERROR("Crop-and-resize needs an output width and height of 1 to 16384 (given: %d x %d)!\n", out_width, out_height);
        return -1;
    }
    for (int f = 0; f < count; f++)
        if (rects[4 * f + 2] < 1 || rects[4 * f + 3] < 1) {
            GJ_ERROR("Frame %d of the batch: the rectangle %d,%d,%d,%d needs a width and a height of at least 1!\n", f, rects[4 * f], rects[4 * f + 1],
                     rects[4 * f + 2], rects[4 * f + 3]);
            return -1;
        }
    if (d->scale > 1) {
        GJ_ERROR("Crop-and-resize is not available together with " GPUJPEG_AMD_DEC_OPT_SCALE "=1/%d!\n", d->scale);
        return -1;
    }
    if (d->flipped) {
        GJ_ERROR("Crop-and-resize is not available together with " GPUJPEG_DEC_OPT_FLIPPED_BOOL "!\n");
        return -1;
    }
    if (d->channel_remap) {
        GJ_ERROR("Crop-and-resize is not available together with " GPUJPEG_DEC_OPT_CHANNEL_REMAP "!\n");
        return -1;
    }
    if (d->resize_filter == GJ_RESIZE_FILTER_ANTIALIAS && d->resize_prescale > 1) { /* (the filter over the reduced cover: not built) */
        GJ_ERROR(GPUJPEG_AMD_DEC_OPT_RESIZE_FILTER "=" GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_ANTIALIAS " is not available together with " GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE "=1/%d!\n",
                 d->resize_prescale);
        return -1;
    }
    const enum gpujpeg_pixel_format pf = d->req_pixel_format;
    if (pf == GPUJPEG_422_U8_P1020 || pf == GPUJPEG_422_U8_P0P1P2 || pf == GPUJPEG_420_U8_P0P1P2) { /* (a format the stream decides: checked with its header) */
        GJ_ERROR("Crop-and-resize is implemented for pixel formats whose pixels do not share samples, not for %s!\n", gpujpeg_pixel_format_get_name(pf));
        return -1;
    }
    /* (the scale every frame takes, as launched: written by the plan of the batched launches and by the frames that go the ordinary way) */
    d->prescales_n = 0;
    if (count > d->prescales_cap) {
        uint8_t* p = realloc(d->prescales, (size_t)count);
        if (!p) return -1;
        d->prescales = p;
        d->prescales_cap = count;
    }
    memset(d->prescales, 1, (size_t)count);
    d->prescales_n = count;
    struct dec_rects what = {.rects = rects, .mirror = mirror, .resize = {.out_w = out_width, .out_h = out_height, .prescale = d->resize_prescale, .filter = d->resize_filter,
                                                                                   .subsampled = d->resize_prescale_subsampled},
                             .mixed = d->batch_sizes_mixed != 0, .any = d->batch_sizes_mixed != 0 && d->batch_headers_any != 0};
    if (tensor) what.resize.tensor = *tensor;
    int rc = decode_batch(d, streams, stream_stride, sizes, count, &what, output, output_stride, param_image);
    if (rc == 0) { /* (slot [4] of the kernel times, gpujpeg_amd_ext.h: 6 when any frame of the call was prescaled -- 8 when per component: the call's
                      streams share one header, the coder's geometry --, whichever launch came last) */
        const float path = what.resize.subsampled && gj_geom_prescale_per_component(&d->coder.geom) ? 8.0f : 6.0f;
        for (int f = 0; f < count; f++)
            if (d->prescales[f] > 1) { d->coder.kernel_ms[4] = path; break; }
    } else {
        d->prescales_n = 0;
    }
    return rc;
}

int gpujpeg_amd_decoder_decode_batch_crop_resize(struct gpujpeg_decoder* d, const uint8_t* streams, size_t stream_stride, const size_t* sizes, int count,
                                                 const int* rects, const uint8_t* mirror, int out_width, int out_height, uint8_t* output, size_t output_stride,
                                                 struct gpujpeg_image_parameters* param_image)
{
    return decode_batch_crop_resize(d, streams, stream_stride, sizes, count, rects, mirror, out_width, out_height, NULL, output, output_stride, param_image);
}

/* The same call with a normalised float tensor as its result: what is checked here is the format and what it asks of the output; everything else --
 * refusals, routing, fallbacks, statistics -- is the call above. The frame's byte size is the tensor's from gj_geom_init_resized on. */
int gpujpeg_amd_decoder_decode_batch_crop_resize_tensor(struct gpujpeg_decoder* d, const uint8_t* streams, size_t stream_stride, const size_t* sizes, int count,
                                                        const int* rects, const uint8_t* mirror, int out_width, int out_height,
                                                        const struct gpujpeg_amd_tensor_format* format, void* output, size_t output_stride,
                                                        struct gpujpeg_image_parameters* param_image)
{
    if (!d || !streams || !sizes || count < 1 || !output || !rects) return -1;
    d->entropy_valid = d->pb_stats_valid = d->hdr_stats_valid = false;
    d->prescales_n = 0;
    if (!format) {
        GJ_ERROR("Tensor output needs a format!\n");
        return -1;
    }
    if (format->dtype < GPUJPEG_AMD_TENSOR_F32 || format->dtype > GPUJPEG_AMD_TENSOR_BF16 || (format->layout != GPUJPEG_AMD_TENSOR_CHW && format->layout != GPUJPEG_AMD_TENSOR_HWC)) {
        GJ_ERROR("Tensor output: unknown element type %d or layout %d!\n", format->dtype, format->layout);
        return -1;
    }
    /* (the pixel format -- and with it the channel count -- and the scales and biases of those channels are checked where the frame's geometry is made,
     * gj_geom_init_resized: for a cold and a warm decoder alike before anything is written) */
    if (d->req_alignment > 1) {
        GJ_ERROR("Tensor output is not available together with " GPUJPEG_DEC_OPT_ALIGNMENT_BYTES_INT "=%u: its frames are dense!\n", d->req_alignment);
        return -1;
    }
    const size_t elsize = (size_t)GJ_TENSOR_ELSIZE(format->dtype);
    if ((uintptr_t)output % elsize != 0 || output_stride % elsize != 0) {
        GJ_ERROR("Tensor output: the buffer and the output stride (%zu) must be multiples of the element size (%zu B)!\n", output_stride, elsize);
        return -1;
    }
    /* (a stride smaller than a frame: the call above refuses it once the channel count is known, before anything is written) */
    gj_tensor t = {.on = 1, .dtype = format->dtype, .layout = format->layout};
    memcpy(t.scale, format->scale, sizeof t.scale);
    memcpy(t.bias, format->bias, sizeof t.bias);
    return decode_batch_crop_resize(d, streams, stream_stride, sizes, count, rects, mirror, out_width, out_height, &t, (uint8_t*)output, output_stride, param_image);
}

/* host-only: the element the tensor call stores for byte v of channel c (the code its kernels run: gj_device.h, gj_tensor_element) */
uint32_t gpujpeg_amd_host_tensor_element(const struct gpujpeg_amd_tensor_format* format, int channel, int v)
{
    if (!format || format->dtype < GPUJPEG_AMD_TENSOR_F32 || format->dtype > GPUJPEG_AMD_TENSOR_BF16 || channel < 0 || channel > 2 || v < 0 || v > 255) return 0;
    gj_tensor t = {.on = 1, .dtype = format->dtype, .layout = format->layout};
    memcpy(t.scale, format->scale, sizeof t.scale);
    memcpy(t.bias, format->bias, sizeof t.bias);
    return gj_hip_tensor_element(&t, channel, v);
}

/* The same for streams and destinations that are separate buffers (device or host memory). The streams are gathered 16 bytes aligned in a staging
 * buffer (they are small), the frames are decoded back to back and copied to their destinations; `frame_bytes` = room in every destination. */
int gpujpeg_amd_decoder_decode_batch_ptrs(struct gpujpeg_decoder* d, const uint8_t* const* streams, const size_t* sizes, int count, uint8_t* const* outputs,
                                          size_t frame_bytes, struct gpujpeg_image_parameters* param_image)
{
    if (!d || !streams || !sizes || !outputs || count < 1) return -1;
    size_t longest = 0;
    for (int f = 0; f < count; f++) {
        if (!streams[f] || !outputs[f]) return -1;
        if (sizes[f] > longest) longest = sizes[f];
    }
    struct gj_coder* c = &d->coder;
    if (frame_bytes == 0) return -1;
    /* buffers of one kind a constant distance apart (streams: a multiple of 16 bytes in device memory): used where they are */
    bool in_strided = true, out_strided = true;
    /* (addresses compared as integers: the buffers may be unrelated allocations, whose pointers C does not let us subtract) */
#define GJ_ADDR_STEP(a, b) ((ptrdiff_t)((uintptr_t)(a) - (uintptr_t)(b)))
    const ptrdiff_t in_step = count > 1 ? GJ_ADDR_STEP(streams[1], streams[0]) : (ptrdiff_t)((longest + 64 + 15) & ~(size_t)15);
    const ptrdiff_t out_step = count > 1 ? GJ_ADDR_STEP(outputs[1], outputs[0]) : (ptrdiff_t)frame_bytes;
    const int in_dev = gj_hip_is_device_ptr(streams[0]), out_dev = gj_hip_is_device_ptr(outputs[0]);
    for (int f = 1; f < count; f++) {
        in_strided = in_strided && GJ_ADDR_STEP(streams[f], streams[f - 1]) == in_step && gj_hip_is_device_ptr(streams[f]) == in_dev;
        out_strided = out_strided && GJ_ADDR_STEP(outputs[f], outputs[f - 1]) == out_step && gj_hip_is_device_ptr(outputs[f]) == out_dev;
    }
#undef GJ_ADDR_STEP
    in_strided = in_strided && in_step > 0 && (size_t)in_step >= longest && (!in_dev || (in_step & 15) == 0);
    out_strided = out_strided && out_step >= (ptrdiff_t)frame_bytes;
    const uint8_t* src = streams[0];
    size_t in_stride = (size_t)in_step;
    if (!in_strided) {
        in_stride = (longest + 64 + 15) & ~(size_t)15;
        if (gj_ensure_device_buffer((void**)&d->b_gather, &d->b_gather_cap, in_stride * (size_t)count) != 0) return -1;
        for (int f = 0; f < count; f++) {
            const int rc = gj_hip_is_device_ptr(streams[f]) ? gj_hip_memcpy_d2d(d->b_gather + (size_t)f * in_stride, streams[f], sizes[f], c->stream)
                                                            : gj_hip_memcpy_h2d(d->b_gather + (size_t)f * in_stride, streams[f], sizes[f], c->stream);
            if (rc != 0) return -1;
        }
        if (gj_hip_stream_sync(c->stream) != 0) return -1; /* (the first frame may be parsed on the host from the staged copy) */
        src = d->b_gather;
    }
    struct gpujpeg_image_parameters pi;
    if (out_strided) { /* (device or host memory: decode_batch takes both) */
        if (gpujpeg_amd_decoder_decode_batch(d, src, in_stride, sizes, count, outputs[0], (size_t)out_step, &pi) != 0) return -1;
        if (param_image) *param_image = pi;
        return 0;
    }
    if (gj_ensure_device_buffer((void**)&d->b_scatter, &d->b_scatter_cap, frame_bytes * (size_t)count) != 0) return -1;
    if (gpujpeg_amd_decoder_decode_batch(d, src, in_stride, sizes, count, d->b_scatter, frame_bytes, &pi) != 0) return -1;
    const size_t raw = dec_raw_size(d);
    for (int f = 0; f < count; f++) {
        const int rc = gj_hip_is_device_ptr(outputs[f]) ? gj_hip_memcpy_d2d(outputs[f], d->b_scatter + (size_t)f * frame_bytes, raw, c->stream)
                                                        : gj_hip_memcpy_d2h(outputs[f], d->b_scatter + (size_t)f * frame_bytes, raw, c->stream);
        if (rc != 0) return -1;
    }
    if (gj_hip_stream_sync(c->stream) != 0) return -1;
    if (param_image) *param_image = pi;
    return 0;
}

/* ------------------------------------------------------------------ image info (src/gpujpeg_reader.c:1739-1872) */
int gpujpeg_decoder_get_image_info2(uint8_t* image, size_t image_size, struct gpujpeg_image_info* info, int verbose, unsigned flags)
{
    struct gj_reader_result r;
    const bool count_segments = (flags & GPUJPEG_COUNT_SEG_COUNT_REQ) != 0;
    const int rc = gj_reader_parse(image, image_size, verbose, false, GPUJPEG_PIXFMT_NATIVE, GPUJPEG_NONE, 0, &r, !count_segments, false);
    if (rc != 0) return rc;
    memset(info, 0, sizeof *info);
    info->param_image = r.param_image;
    info->param = r.param;
    info->header_type = r.header_type;
    info->comment = r.comment;
    info->metadata = r.metadata;
    if (info->param_image.color_space == GPUJPEG_NONE) info->param_image.color_space = r.param.color_space_internal;
    if (count_segments) {
        gj_geom g;
        struct gj_host_segments segs = {0};
        if (gj_geom_init(&g, &r.param, &r.param_image, false) == 0 && gj_reader_split_scans(image, &r, &g, &segs, verbose) == 0)
            info->segment_count = segs.count;
        free(segs.pos); free(segs.len); free(segs.index);
    }
    return 0;
}

int gpujpeg_decoder_get_image_info(uint8_t* image, size_t image_size, struct gpujpeg_image_parameters* pi, struct gpujpeg_parameters* param, int* segment_count)
{
    struct gpujpeg_image_info info;
    const int rc = gpujpeg_decoder_get_image_info2(image, image_size, &info, param ? param->verbose : 0, segment_count ? GPUJPEG_COUNT_SEG_COUNT_REQ : 0);
    if (rc != 0) return rc;
    if (pi) *pi = info.param_image;
    if (param) { const int v = param->verbose, ps = param->perf_stats; *param = info.param; param->verbose = v; param->perf_stats = ps; }
    if (segment_count) *segment_count = info.segment_count;
    return 0;
}

/* ------------------------------------------------------------------ options (src/gpujpeg_decoder.c:486-558) */
int gpujpeg_decoder_set_option(struct gpujpeg_decoder* d, const char* opt, const char* val)
{
    if (d == NULL || opt == NULL || val == NULL) return GPUJPEG_ERROR;
    if (strcmp(opt, GPUJPEG_DEC_OPT_ALIGNMENT_BYTES_INT) == 0) {
        const int a = atoi(val);
        if (a < 0) { GJ_ERROR("Wrong alignment: %s\n", val); return GPUJPEG_ERROR; }
        d->req_alignment = (unsigned)a;
        d->hdr_cache_valid = false;
        return GPUJPEG_NOERR;
    }
    if (strcmp(opt, GPUJPEG_DEC_OPT_TGA_RLE_BOOL) == 0) return GPUJPEG_NOERR; /* only affects file output */
    if (strcmp(opt, GPUJPEG_DEC_OPT_FLIPPED_BOOL) == 0) { /* src/gpujpeg_decoder.c:499-501 */
        if (strcasecmp(val, GPUJPEG_VAL_TRUE) == 0 || strcmp(val, "1") == 0) d->flipped = true;
        else if (strcasecmp(val, GPUJPEG_VAL_FALSE) == 0 || strcmp(val, "0") == 0) d->flipped = false;
        else { GJ_ERROR("Unknown option %s for " GPUJPEG_DEC_OPT_FLIPPED_BOOL "\n", val); return GPUJPEG_ERROR; }
        return GPUJPEG_NOERR;
    }
    if (strcmp(opt, GPUJPEG_DEC_OPT_CHANNEL_REMAP) == 0) return gj_parse_channel_remap(&d->channel_remap, val, opt);
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_SCALE) == 0) { /* holds from the next decode call on */
        static const char* const names[4] = {"1", "1/2", "1/4", "1/8"};
        for (int i = 0; i < 4; i++)
            if (strcmp(val, names[i]) == 0) { d->scale = 1 << i; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_SCALE " (1, 1/2, 1/4 or 1/8)\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE) == 0) { /* read by gpujpeg_amd_decoder_decode_batch_crop_resize alone */
        static const char* const names[4] = {"1", "1/2", "1/4", "1/8"};
        for (int i = 0; i < 4; i++)
            if (strcmp(val, names[i]) == 0) { d->resize_prescale = 1 << i; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE " (1, 1/2, 1/4 or 1/8)\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_RESIZE_FILTER) == 0) { /* read by gpujpeg_amd_decoder_decode_batch_crop_resize (and _tensor) alone */
        if (strcmp(val, GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_BILINEAR) == 0) { d->resize_filter = GJ_RESIZE_FILTER_BILINEAR; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_ANTIALIAS) == 0) { d->resize_filter = GJ_RESIZE_FILTER_ANTIALIAS; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_RESIZE_FILTER " (" GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_BILINEAR " or " GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_ANTIALIAS ")\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE_SUBSAMPLED) == 0) { /* read by gpujpeg_amd_decoder_decode_batch_crop_resize (and _tensor) alone */
        if (strcmp(val, GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_OFF) == 0) { d->resize_prescale_subsampled = 0; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_ON) == 0) { d->resize_prescale_subsampled = 1; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE_SUBSAMPLED " (" GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_OFF " or " GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_ON ")\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_BATCH_RESTARTLESS) == 0) { /* read by every batch call when it starts */
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_OFF) == 0) { d->batch_restartless = 0; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_ON) == 0) { d->batch_restartless = 1; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_BATCH_RESTARTLESS " (" GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_OFF " or " GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_ON ")\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_BATCH_PROGRESSIVE) == 0) { /* read by every batch call when it starts */
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_OFF) == 0) { d->batch_progressive = 0; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_ON) == 0) { d->batch_progressive = 1; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_BATCH_PROGRESSIVE " (" GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_OFF " or " GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_ON ")\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_BATCH_SIZES) == 0) { /* read by gpujpeg_amd_decoder_decode_batch_crop_resize (and _tensor) alone */
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_SAME) == 0) { d->batch_sizes_mixed = 0; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_MIXED) == 0) { d->batch_sizes_mixed = 1; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_BATCH_SIZES " (" GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_SAME " or " GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_MIXED ")\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_BATCH_HEADERS) == 0) { /* read by gpujpeg_amd_decoder_decode_batch_crop_resize (and _tensor) alone, next to dec_opt_batch_sizes = mixed */
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_SAME) == 0) { d->batch_headers_any = 0; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_ANY) == 0) { d->batch_headers_any = 1; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_BATCH_HEADERS " (" GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_SAME " or " GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_ANY ")\n", val);
        return GPUJPEG_ERROR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_REGION) == 0) { /* syntax only: the decode call checks the region against its stream */
        if (strcmp(val, "full") == 0) { d->region_on = false; return GPUJPEG_NOERR; }
        long v[4];
        const char* p = val;
        bool ok = true;
        for (int i = 0; i < 4 && ok; i++) {
            int digits = 0;
            v[i] = 0;
            while (*p >= '0' && *p <= '9' && digits < 9) { v[i] = v[i] * 10 + (*p - '0'); p++; digits++; }
            ok = digits > 0 && !(*p >= '0' && *p <= '9') && *p == (i < 3 ? ',' : '\0');
            if (ok && i < 3) p++;
        }
        if (!ok || v[2] < 1 || v[3] < 1) {
            GJ_ERROR("Wrong value %s for " GPUJPEG_AMD_DEC_OPT_REGION " (X,Y,W,H in pixels with W, H >= 1, or full)\n", val);
            return GPUJPEG_ERROR;
        }
        for (int i = 0; i < 4; i++) d->region[i] = (int)v[i];
        d->region_on = true;
        return GPUJPEG_NOERR;
    }
    if (strcmp(opt, GPUJPEG_AMD_DEC_OPT_PROGRESSIVE) == 0) { /* holds from the next decode call on */
        if (strcmp(val, GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_OFF) == 0) { d->progressive = 0; return GPUJPEG_NOERR; }
        if (strcmp(val, GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_ON) == 0) { d->progressive = 1; return GPUJPEG_NOERR; }
        GJ_ERROR("Unknown value %s for " GPUJPEG_AMD_DEC_OPT_PROGRESSIVE " (" GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_OFF " or " GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_ON ")\n", val);
        return GPUJPEG_ERROR;
    }
    GJ_ERROR("Invalid decoder option: %s!\n", opt);
    return GPUJPEG_ERROR;
}

void gpujpeg_decoder_print_options(void)
{
    printf("\t" GPUJPEG_DEC_OPT_ALIGNMENT_BYTES_INT "=<n> - required line alignment of the decoded image in bytes\n");
    printf("\t" GPUJPEG_DEC_OPT_FLIPPED_BOOL "=[" GPUJPEG_VAL_TRUE "|" GPUJPEG_VAL_FALSE "] - whether the output image should be vertically flipped\n");
    printf("\t" GPUJPEG_DEC_OPT_CHANNEL_REMAP "=XYZ[W] - output channel remapping, 'help' for details\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_SCALE "=[1|1/2|1/4|1/8] - decode to a reduced-size image (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE "=[1|1/2|1/4|1/8] - largest reduced-size IDCT crop-and-resize may put ahead of its resample (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_RESIZE_FILTER "=[" GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_BILINEAR "|" GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_ANTIALIAS "] - filter of crop-and-resize's resample: four taps, or a footprint that grows with the reduction (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE_SUBSAMPLED "=[" GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_OFF "|" GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_ON "] - let that prescale reduce 4:2:0 streams too, each component at its own N (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_BATCH_RESTARTLESS "=[" GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_OFF "|" GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_ON "] - whether the batch calls take streams without restart markers through their batched launches (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_BATCH_SIZES "=[" GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_SAME "|" GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_MIXED "] - whether the streams of one crop-and-resize call may differ in image size (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_BATCH_HEADERS "=[" GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_SAME "|" GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_ANY "] - whether the streams of one such call (" GPUJPEG_AMD_DEC_OPT_BATCH_SIZES "=" GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_MIXED ") may differ in tables and marker segments and still share its batched launches (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_PROGRESSIVE "=[" GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_OFF "|" GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_ON "] - whether progressive (SOF2) streams are decoded (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_BATCH_PROGRESSIVE "=[" GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_OFF "|" GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_ON "] - whether the batch calls take groups of progressive streams through batched launches (MI355X extension)\n");
    printf("\t" GPUJPEG_AMD_DEC_OPT_REGION "=[X,Y,W,H|full] - decode the W x H pixels at (X, Y) only (MI355X extension)\n");
}

/* ------------------------------------------------------------------ MI355X extensions (include/gpujpeg_amd_ext.h) */

void gpujpeg_amd_decoder_set_batch_chunk(struct gpujpeg_decoder* d, int frames) { if (d) d->b_chunk = frames > 0 ? frames : 0; }

int gpujpeg_amd_decoder_get_path_counters(struct gpujpeg_decoder* d, long counters[3])
{
    if (!d || !counters) return -1;
    counters[0] = d->n_spec;
    counters[1] = d->n_folded;
    counters[2] = d->n_again;
    return 0;
}

int gpujpeg_amd_decoder_last_batch(struct gpujpeg_decoder* d, int* batched, int* single)
{
    if (!d) return -1;
    if (batched) *batched = d->b_last_batched;
    if (single) *single = d->b_last_single;
    return 0;
}

size_t gpujpeg_amd_decoder_read_coefficients(struct gpujpeg_decoder* d, int16_t* dst, size_t capacity)
{
    const size_t n = d->coder.geom.data_size;
    if (!d->coder.configured || capacity < n) return 0;
    if (gj_hip_memcpy_d2h(dst, d->coder.d_coefs, n * sizeof(int16_t), d->coder.stream) != 0 || gj_hip_stream_sync(d->coder.stream) != 0) return 0;
    return n;
}

size_t gpujpeg_amd_decoder_read_planes(struct gpujpeg_decoder* d, uint8_t* dst, size_t capacity)
{
    const size_t n = dec_reduced_or_region(d) ? d->img.geom.data_size : d->coder.geom.data_size; /* (the reduced planes of a reduced-size decode, the cover's of a region decode) */
    if (!d->coder.configured || capacity < n) return 0;
    if (gj_hip_memcpy_d2h(dst, d->coder.d_planes, n, d->coder.stream) != 0 || gj_hip_stream_sync(d->coder.stream) != 0) return 0;
    return n;
}

int gpujpeg_amd_host_crop_resize_plan(int image_w, int image_h, int all_components_1x1, const int rect[4], int out_w, int out_h, int max_scale, int out[5])
{
    if (!rect || !out) return -1;
    return gj_crop_resize_plan(image_w, image_h, all_components_1x1, rect, out_w, out_h, max_scale, out);
}

int gpujpeg_amd_host_resize_weights(int n_src, int n_out, int i, int* first, int* count, uint32_t* weights, int capacity, uint64_t* sum)
{
    return gj_hip_resize_aa_weights(n_src, n_out, i, first, count, weights, weights ? capacity : 0, sum);
}

int gpujpeg_amd_decoder_get_prescales(struct gpujpeg_decoder* d, uint8_t* dst, int capacity)
{
    if (!d || !dst || d->prescales_n < 1 || capacity < d->prescales_n) return 0;
    memcpy(dst, d->prescales, (size_t)d->prescales_n);
    return d->prescales_n;
}

int gpujpeg_amd_host_orientation_plan(int image_w, int image_h, int rotation, int flip, const int rect[4], int out_w, int out_h, int mirror, int out[8])
{
    if (!rect || !out || rotation < 0 || rotation > 3) return -1;
    return gj_orientation_plan(image_w, image_h, rotation, flip != 0, rect, out_w, out_h, mirror != 0, out);
}

int gpujpeg_amd_host_stream_orientation(const uint8_t* image, size_t size, int out[5])
{
    if (!image || !out) return -1;
    memset(out, 0, 5 * sizeof(int));
    struct gj_reader_result* r = malloc(sizeof *r);
    int rc = -1;
    if (r && gj_reader_parse(image, size, GPUJPEG_LL_QUIET - 1, false, GPUJPEG_PIXFMT_NATIVE, GPUJPEG_NONE, 0, r, true, true) == 0) {
        const bool set = r->metadata.vals[GPUJPEG_METADATA_ORIENTATION].set;
        out[0] = set ? 1 : 0;
        out[1] = set ? (int)r->metadata.vals[GPUJPEG_METADATA_ORIENTATION].orient.rotation : 0;
        out[2] = set ? (int)r->metadata.vals[GPUJPEG_METADATA_ORIENTATION].orient.flip : 0;
        out[3] = (out[1] & 1) ? r->param_image.height : r->param_image.width;
        out[4] = (out[1] & 1) ? r->param_image.width : r->param_image.height;
        rc = 0;
    }
    free(r);
    return rc;
}

int gpujpeg_amd_decoder_get_entropy_bytes(struct gpujpeg_decoder* d, uint64_t out[2])
{
    if (!d || !out) return -1;
    out[0] = d->entropy_valid ? d->entropy_bytes[0] : 0;
    out[1] = d->entropy_valid ? d->entropy_bytes[1] : 0;
    return d->entropy_valid ? 0 : -1;
}

int gpujpeg_amd_decoder_get_region_stats(struct gpujpeg_decoder* d, long out[4])
{
    if (!d || !out) return -1;
    memcpy(out, d->region_stats, sizeof d->region_stats);
    return 0;
}

int gpujpeg_amd_decoder_get_progressive_stats(struct gpujpeg_decoder* d, long out[4])
{
    if (!d || !out) return -1;
    for (int i = 0; i < 4; i++) out[i] = d->prog_stats_valid ? d->prog_stats[i] : 0;
    return d->prog_stats_valid ? 0 : -1;
}

int gpujpeg_amd_decoder_get_progressive_batch_stats(struct gpujpeg_decoder* d, long out[4])
{
    if (!d || !out) return -1;
    for (int i = 0; i < 4; i++) out[i] = d->pb_stats_valid ? d->pb_stats[i] : 0;
    return d->pb_stats_valid ? 0 : -1;
}

int gpujpeg_amd_decoder_get_batch_header_stats(struct gpujpeg_decoder* d, long out[4])
{
    if (!d || !out) return -1;
    for (int i = 0; i < 4; i++) out[i] = d->hdr_stats_valid ? d->hdr_stats[i] : 0;
    return d->hdr_stats_valid ? 0 : -1;
}

int gpujpeg_amd_decoder_get_batch_header_times(struct gpujpeg_decoder* d, double ms[3])
{
    if (!d || !ms) return -1;
    for (int i = 0; i < 3; i++) ms[i] = d->hdr_stats_valid ? d->hdr_ms[i] : 0.0;
    return d->hdr_stats_valid ? 0 : -1;
}

int gpujpeg_amd_host_stream_info(const uint8_t* image, size_t size, int out[8])
{
    if (!image || !out) return -1;
    memset(out, 0, 8 * sizeof(int));
    struct gj_reader_result* r = malloc(sizeof *r);
    struct gj_prog_info* info = calloc(1, sizeof *info);
    int rc = -1;
    if (r && info && gj_reader_parse(image, size, GPUJPEG_LL_QUIET - 1, false, GPUJPEG_PIXFMT_NATIVE, GPUJPEG_NONE, 0, r, false, true) == 0) {
        out[0] = r->param_image.width;
        out[1] = r->param_image.height;
        out[2] = r->param.comp_count;
        out[3] = r->progressive ? 1 : 0;
        out[4] = r->scan_count;
        out[5] = 1;
        out[6] = r->param.restart_interval;
        rc = 0;
        if (r->progressive && (rc = gj_reader_parse_progressive(image, size, r, info, true)) == 0) {
            out[4] = info->scan_count;
            out[5] = info->levels;
            out[7] = info->bad_scan;
            if (info->scan_count > 0) out[6] = info->scan[0].restart_interval;
        }
    }
    if (info) gj_prog_info_free(info);
    free(info);
    free(r);
    return rc;
}

void gpujpeg_amd_decoder_set_fused(struct gpujpeg_decoder* d, int enabled) { d->use_fused = enabled != 0; }
void gpujpeg_amd_decoder_keep_coefficients(struct gpujpeg_decoder* d, int enabled) { d->keep_coefs = enabled != 0; }

/* durations of the kernels of the last decode: [0] k_huffman_decode, [1] IDCT (fused: incl. postprocess), [2] postprocess */
int gpujpeg_amd_decoder_get_kernel_times(struct gpujpeg_decoder* d, float ms[8])
{
    if (!d->coder.timers.valid) return -1;
    memcpy(ms, d->coder.kernel_ms, 8 * sizeof(float));
    return 0;
}
