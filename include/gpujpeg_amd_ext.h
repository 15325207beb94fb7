/*
 * gpujpeg_amd_ext.h -- MI355X-specific additions next to the unchanged libgpujpeg API.
 * They expose intermediate device state for stage-level parity tests and benchmarks; production callers
 * never need them.
 */
#ifndef GPUJPEG_AMD_EXT_H
#define GPUJPEG_AMD_EXT_H

#include <stddef.h>
#include <stdint.h>

#include "libgpujpeg/gpujpeg_common.h"

#ifdef __cplusplus
extern "C" {
#endif

struct gpujpeg_encoder;
struct gpujpeg_decoder;

/* copy the quantised coefficients of the last encode/decode call (int16, 64 per 8x8 block, blocks in
 * raster order per component, components back to back = the reference's d_data_quantized layout,
 * src/gpujpeg_dct_gpu.cu:286-294) to host memory; returns the number of coefficients, 0 on error */
GPUJPEG_API size_t gpujpeg_amd_encoder_read_coefficients(struct gpujpeg_encoder* encoder, int16_t* dst, size_t capacity);
GPUJPEG_API size_t gpujpeg_amd_decoder_read_coefficients(struct gpujpeg_decoder* decoder, int16_t* dst, size_t capacity);
/* padded planar component samples (generic path only) */
GPUJPEG_API size_t gpujpeg_amd_encoder_read_planes(struct gpujpeg_encoder* encoder, uint8_t* dst, size_t capacity);
GPUJPEG_API size_t gpujpeg_amd_decoder_read_planes(struct gpujpeg_decoder* decoder, uint8_t* dst, size_t capacity);
/* 1 = use the fused fast-path kernels when the format allows (default), 0 = always take the generic path */
GPUJPEG_API void gpujpeg_amd_encoder_set_fused(struct gpujpeg_encoder* encoder, int enabled);
GPUJPEG_API void gpujpeg_amd_decoder_set_fused(struct gpujpeg_decoder* decoder, int enabled);
/* 1 = the following encode calls leave the quantised coefficients in HBM for gpujpeg_amd_encoder_read_coefficients (tests).
 * Default 0: where the format allows, pixels go to entropy-coded segments in one kernel and no coefficient planes exist. */
GPUJPEG_API void gpujpeg_amd_encoder_keep_coefficients(struct gpujpeg_encoder* encoder, int enabled);
/* 1 = leave the coefficients of the following decode calls in HBM for gpujpeg_amd_decoder_read_coefficients (tests).
 * Default 0: the IDCT clears each block once it has read it, which saves the per-frame clear of the coefficient planes. */
GPUJPEG_API void gpujpeg_amd_decoder_keep_coefficients(struct gpujpeg_decoder* decoder, int enabled);

/* Developer settings: forced kernel paths for tests and A/B measurements ("GJ_DEC_TOKENS=1", "GJ_ENC_TAIL=0", ...; the table in INTEGRATION.md).
 * Process-wide; a coder takes the values that are set when it is CREATED. `setting` is "NAME=VALUE" or "NAME"; NULL forgets every setting.
 * Returns 0, -1 for a name the library does not know. The library never reads the environment (round 6). */
GPUJPEG_API int gpujpeg_amd_tuning(const char* setting);
/* the names gpujpeg_amd_tuning knows, NULL-terminated */
GPUJPEG_API const char* const* gpujpeg_amd_tuning_names(void);

/* Host-only helper (no device access): the marker segments the encoder would emit for these parameters --
 * everything up to the first scan (SOI .. COM), followed by the scan headers back to back. Parameters are
 * adjusted exactly like gpujpeg_encoder_encode() does on a fresh encoder (comp_count 0, RESTART_AUTO).
 * Returns the number of bytes written, 0 on error. Used by the CPU test-suite to check tables, geometry
 * and the writer against the oracle without a GPU. */
GPUJPEG_API size_t gpujpeg_amd_host_headers(const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                                            int header_type, uint8_t* dst, size_t capacity, size_t* main_header_size);
/* the same with orientation metadata (rotation in quarter turns clockwise, -1 = none; flip) as set by enc_metadata */
GPUJPEG_API size_t gpujpeg_amd_host_headers_md(const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                                               int header_type, int rotation, int flip, uint8_t* dst, size_t capacity, size_t* main_header_size);
/* the same with user Exif tags in the syntax of the encoder option enc_exif_tag ("<ID>:<type>=<value>" or "<name>=<value>");
 * any tag selects the Exif header like the option does */
GPUJPEG_API size_t gpujpeg_amd_host_headers_exif(const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image,
                                                 int header_type, int rotation, int flip, const char* const* exif_tags, int exif_tag_count,
                                                 uint8_t* dst, size_t capacity, size_t* main_header_size);
/* Host-only: decode a BMP / TGA / PNG / GIF file (by extension) with the readers behind gpujpeg_image_load_from_file into caller
 * memory: interleaved 8-bit channels, top-down. dst == NULL: header only. Returns 0, -1 on error or when capacity is too small. */
GPUJPEG_API int gpujpeg_amd_read_raster_file(const char* filename, uint8_t* dst, size_t capacity, int* width, int* height, int* channels);
/* Host-only: geometry summary for the adjusted parameters: out[0] segment_count, [1] block_count, [2] restart interval,
 * [3] blocks per MCU, [4 + 4*c ..] per component data_width, data_height, segment_count, type */
GPUJPEG_API int gpujpeg_amd_host_geometry(const struct gpujpeg_parameters* param, const struct gpujpeg_image_parameters* param_image, int out[20]);

/* Host-only: builds both decode-table layouts for one DHT table (bits[1..16] = codes per length, vals = symbols) exactly as
 * gpujpeg_decoder_decode does and reports 0 = accepted, -1 = rejected (over-subscribed or more than 256 symbols). Lets the CPU
 * test-suite feed hostile tables to the builders without a GPU. */
GPUJPEG_API int gpujpeg_amd_host_huffman_table_check(const uint8_t bits[17], const uint8_t* vals, int is_ac);
/* Encoder option (gpujpeg_encoder_set_option): Huffman tables of the written streams.
 *   "standard" (default)  the typical tables of ITU T.81 Annex K.3 -- byte for byte the reference's streams;
 *   "optimal"             per frame, tables built from the frame's own symbol counts (counted on the GPU, k_huffman_count): smaller files
 *                         with the same coefficients. One more host wait per frame (the 4 KiB histogram), and the frame goes through the
 *                         coefficient planes; batch calls code such frames one by one. Outside reference parity by construction. */
#define GPUJPEG_AMD_ENC_OPT_HUFFMAN "enc_opt_huffman"
#define GPUJPEG_AMD_ENC_HUFFMAN_VAL_STANDARD "standard"
#define GPUJPEG_AMD_ENC_HUFFMAN_VAL_OPTIMAL "optimal"
/* Decoder option (gpujpeg_decoder_set_option): reduced-size output. "1" (default), "1/2", "1/4", "1/8": the decode calls return the image of
 * GPUJPEG_AMD_SCALED_DIM(width, s) x GPUJPEG_AMD_SCALED_DIM(height, s) pixels that the N x N low-frequency corner (N = 8 / s) of every block gives
 * (integer N-point inverse DCT, DESIGN "Reduced-size decode"); output->param_image, output->data_size and the buffer layout are those of an image of
 * that size, gpujpeg_decoder_get_image_info keeps reporting the stream's own size. May be changed between two calls of a decoder. Packed 4:2:2 output
 * of odd reduced width and dec_opt_flipped together with a scale are refused by the decode call. The batch calls (gpujpeg_amd_decoder_decode_batch,
 * _decode_batch_ptrs) take the scale into their batched launches -- the frame is a grid dimension of the reduced-size kernels, output_stride and
 * frame_bytes count in reduced frames --; what still goes frame by frame inside the call is what does so at full size (restart interval 0, channel
 * remap, another header, damaged markers, a segment too long for the fast entropy decoders, the first frame of a decoder's life, frame 0 of a call
 * whose pixels go to host memory). A scale together with gpujpeg_amd_decoder_decode_batch_regions is refused.
 * Outside reference parity by construction (the reference has no reduced decode). */
#define GPUJPEG_AMD_DEC_OPT_SCALE "dec_opt_scale"
#define GPUJPEG_AMD_SCALED_DIM(v, s) (((v) + (s) - 1) / (s))
/* Decoder option (gpujpeg_decoder_set_option): region-of-interest decode. "X,Y,W,H" in pixels of the stream's full-size image, or "full" (default):
 * no region. set_option checks the syntax only (four decimal integers, W, H >= 1; anything else returns GPUJPEG_ERROR and leaves the setting as it
 * was); the option holds from the next decode call on and may be changed between two calls of a decoder.
 * A decode call with a region returns the W x H image whose pixel (i, j) is pixel (X + i, Y + j) of the image the same decoder returns without
 * the option -- same pixel format, colour space and dec_opt_channel_remap; output->param_image.width / height are W and H, output->data_size and
 * the buffer layout those of a W x H image of that format (dec_opt_alignment_bytes applies to the region's line),
 * gpujpeg_decoder_get_image_info keeps reporting the stream's own size. Planar output: plane c is the crop of plane c of the full result at
 * (X / hs_c, Y / vs_c), ceil(W / hs_c) x ceil(H / vs_c) samples.
 * Grey, packed 4:4:4 / 4:4:4:4 and planar 4:4:4 output take any rectangle inside the image, whatever the stream's sampling. Packed 4:2:2, planar
 * 4:2:2 and planar 4:2:0 output need X (4:2:0: and Y) even, and W (H) even unless the region ends at the image's right (bottom) edge.
 * Refused by the DECODE CALL with a message (the decoder stays usable): a region that is not inside the stream's image, those misalignments, a
 * region together with dec_opt_flipped or with a dec_opt_scale other than 1.
 * What a region call skips: on a stream with a restart interval whose segments are all there, only the restart segments that touch the region's
 * cover (per component the smallest rectangle of 8x8 blocks, whole MCUs of an interleaved scan, that holds the samples the region needs) are
 * entropy-decoded; otherwise (restart interval 0, missing segments) all of them. Either way only the cover's blocks are transformed, only W x H pixels
 * are written and downloaded. Token mode serves a region call where it serves the full frame's packed 4:4:4 output (k_idct_tok_region_rgb444),
 * every other configuration goes through the coefficient planes and cover-sized component planes; the bytes are the same. Batch calls decode the frames
 * of a decoder that has a region one by one (one crop per frame behind batched launches: gpujpeg_amd_decoder_decode_batch_regions). After a region call gpujpeg_amd_decoder_read_planes returns the cover-sized component planes (cover
 * of component c: see DESIGN 4.2) and gpujpeg_amd_decoder_read_coefficients the full planes, of which only the blocks of the entropy-decoded
 * segments are this frame's. */
#define GPUJPEG_AMD_DEC_OPT_REGION "dec_opt_region"
/* Decoder option "dec_opt_resize_prescale" = "1" (default), "1/2", "1/4" or "1/8": the largest reduction S that
 * gpujpeg_amd_decoder_decode_batch_crop_resize may put in front of its resample -- the reduced-size IDCT of dec_opt_scale over the rectangle's cover,
 * a low-pass filter that costs less than the transform it replaces, where the bilinear resample alone would point-sample a rectangle much larger
 * than the output. Read by that call alone (its definition with a prescale: below); every other call, and that call with "1", is what it is without
 * the option. Another value is refused by gpujpeg_decoder_set_option and leaves the setting as it was. dec_opt_scale itself stays refused by the call. */
#define GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE "dec_opt_resize_prescale"
/* Decoder option "dec_opt_resize_prescale_subsampled" = "off" (default) or "on": lets that prescale reduce 4:2:0 streams too -- the streams of
 * photographs --, each component at its own N, the way libjpeg's scaled decode does. Read by gpujpeg_amd_decoder_decode_batch_crop_resize and
 * gpujpeg_amd_decoder_decode_batch_crop_resize_tensor alone; it holds from the next call on and may be changed between two calls of a decoder. Another
 * value is refused by gpujpeg_decoder_set_option (GPUJPEG_ERROR) and leaves the setting as it was. It has an effect only together with a
 * dec_opt_resize_prescale other than 1; with "off" every byte, counter, launch and kernel-times slot of every call is what it is without the option.
 * WITH "on". Take sub_h, sub_v of a component as the largest horizontal (vertical) sampling factor of the stream divided by the component's. A stream is
 * ELIGIBLE when every component has sub_h == sub_v in {1, 2}, at least one has 2, and no component has a smaller sub_h than the component ahead of
 * it: 4:2:0, and Y sampled 2 x 2 followed by further 2 x 2 components and then by 1 x 1 ones, in the stream's order (sub_h 1 ... 1 2 ... 2). [The last condition
 * is this library's: the reduced planes below lie inside the slots of the full-size ones and would overlap in another order.] A frame of an eligible
 * stream takes s_f by the rule of the streams whose components are all 1 x 1 (below; gpujpeg_amd_host_crop_resize_plan with all_components_1x1 != 0). Every
 * other subsampled stream keeps s_f = 1: 4:2:2, 4:4:0, 4:1:1, anything with a factor of 4 or sub_h != sub_v (no rectangular reduced IDCT).
 * For s = s_f > 1, Rs of the definition below is the ceil(W / s) x ceil(H / s) image built like this. Component c has t_c = sub_h and N_c = 8 t_c / s, one of
 * 1, 2, 4, 8; sample (X, Y) of its reduced plane is
 *     N_c <= 4:  sample (X mod N_c, Y mod N_c) of block (X / N_c, Y / N_c) under the transform of dec_opt_scale with N = N_c (gj_dequant_clamp with the
 *                uint16 table, then the N_c-point IDCT of the block's N_c x N_c corner: DESIGN "Reduced-size decode")
 *     N_c = 8:   sample (X, Y) of the component's plane of the full-size decode (the float IDCT of k_idct_region, with the FMA-parity caveat it carries)
 * and pixel (X, Y) of Rs is made from the components' samples at (X, Y) exactly as a pixel of a stream whose components are all 1 x 1: the same colour
 * transform, the same expansion of a single component, the same no_transform rule. Every plane has one sample per reduced pixel: at s = 2 a 4:2:0
 * stream's chroma goes through the full-size IDCT and its luma through N = 4, at s = 8 luma takes N = 1 and chroma N = 2. Blocks line up: reduced pixel
 * X covers the full-size pixels [sX, sX + s), the samples of block X / N_c of every component.
 * From there x', w', C', the taps, the blend, the mirror, the output formats and the tensor store are the text below, word for word, and so is the
 * cover: the region call's for the covering rectangle expanded to full size; reduced sample X of component c lies in block X / N_c of it.
 *   Refusals:  all unchanged.    Antialias:  dec_opt_resize_filter = antialias together with a prescale stays refused.
 *   Prescales: gpujpeg_amd_decoder_get_prescales reports s_f.
 *   Planes:    gpujpeg_amd_decoder_read_planes returns the reduced cover planes with N_c per component: component c at offset data_offset N_c^2 / 64 with
 *              pitch data_width N_c / 8 of the cover plane's.
 *   Slot [4] of gpujpeg_amd_decoder_get_kernel_times is 8 after a call in which at least one frame was reduced per component (k_idct_region_scaled_comp);
 *              it stays 6 when only frames of all-1 x 1 streams were reduced, and 5 when none was. */
#define GPUJPEG_AMD_DEC_OPT_RESIZE_PRESCALE_SUBSAMPLED "dec_opt_resize_prescale_subsampled"
#define GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_OFF "off"
#define GPUJPEG_AMD_DEC_RESIZE_PRESCALE_SUBSAMPLED_VAL_ON "on"
/* Decoder option "dec_opt_resize_filter" = "bilinear" (default) or "antialias": the filter of the resample of
 * gpujpeg_amd_decoder_decode_batch_crop_resize and gpujpeg_amd_decoder_decode_batch_crop_resize_tensor. Read by those two calls alone; it holds from the
 * next call on and may be changed between two calls of a decoder. Another value is refused by gpujpeg_decoder_set_option (GPUJPEG_ERROR) and leaves the
 * setting as it was. With "bilinear" every byte, counter and kernel of every call is what it is without the option.
 * WITH "antialias" everything in the DEFINITION of the crop-and-resize call (below) stands -- C, the mirror, the output formats, param_image, the strides,
 * the fourth byte of GPUJPEG_4444_U8_P0123 going through the same formula -- except the lines that make R. For a frame with rectangle w x h and output
 * OW x OH, channel by channel on output pixels; integers throughout, division = floor:
 *     Dx = max(w, OW);  u_i(k) = max(0, 2 Dx - |(2k + 1) OW - (2i + 1) w|)   k in [0, w),  U_i = sum_k u_i(k)        i < OW
 *     Dy = max(h, OH);  v_j(l) = max(0, 2 Dy - |(2l + 1) OH - (2j + 1) h|)   l in [0, h),  V_j = sum_l v_j(l)        j < OH
 *     S       = sum_l v_j(l) sum_k u_i(k) C[l][k]
 *     R[j][i] = (2 S + U_i V_j) / (2 U_i V_j);      out[j][i] = mirror && mirror[f] ? R[j][OW - 1 - i] : R[j][i]
 * The triangle filter with half-pixel centres whose support is stretched by w / OW when reducing and is one pixel when enlarging; taps outside the
 * rectangle are dropped and the rest renormalised by their exact sum: the antialias = True bilinear filter of torch and PIL with exact rational weights
 * and ONE rounding (half up) -- at most half a level from that filter evaluated in float64. The identity for w == OW and h == OH; a constant stays
 * that constant (0xFF stays 0xFF); U_i >= Dx > 0. Where w <= OW and h <= OH it is bilinear interpolation with exact weights, which may differ from the
 * 8-bit weights of "bilinear" by a level.
 * Refused by the call with a message, -1 returned, nothing of `output` written, the decoder usable as before: a frame with w > 256 OW or h > 256 OH (the
 * message names the frame; with image sides <= 65535 this keeps U_i, V_j < 2^26 and 2 S + U V < 2^62: every accepted frame comes out exact); the
 * filter together with a dec_opt_resize_prescale other than 1. Every other refusal, the routing, the fallbacks, gpujpeg_amd_decoder_last_batch,
 * _get_region_stats and _get_prescales (all 1) are those of the call with "bilinear"; the batched launches end in k_resize_region_aa_batch
 * (k_resize_region_aa_tensor_batch), the single-frame route in k_resize_region_aa (_tensor): the same bytes. Slot [4] of
 * gpujpeg_amd_decoder_get_kernel_times is 7 after a call that resampled with this filter. */
#define GPUJPEG_AMD_DEC_OPT_RESIZE_FILTER "dec_opt_resize_filter"
#define GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_BILINEAR "bilinear"
#define GPUJPEG_AMD_DEC_RESIZE_FILTER_VAL_ANTIALIAS "antialias"
/* Decoder option "dec_opt_batch_sizes" = "same" (default) or "mixed": whether the streams of ONE call of gpujpeg_amd_decoder_decode_batch_crop_resize or
 * gpujpeg_amd_decoder_decode_batch_crop_resize_tensor may differ in image size. Read by those two calls alone (gpujpeg_amd_decoder_decode_batch and
 * _decode_batch_regions do not read it and keep refusing streams of other dimensions); it holds from the next call on and may be changed between two
 * calls of a decoder. Another value is refused by gpujpeg_decoder_set_option (GPUJPEG_ERROR) and leaves the setting as it was. With "same" every byte,
 * counter, launch, refusal and kernel-times slot of every call is what it is without the option.
 * WITH "mixed" frame f is, byte for byte (tensor call: bit for bit), what the same call returns for a batch of the one stream f with rects[4f .. 4f + 3],
 * mirror[f] and every other argument and option the same -- the definition over the single-frame region call, as ever. The streams may differ in image
 * width and height (and in anything else); every rectangle is checked against ITS stream's image, a refusal names the frame and is made before anything of
 * `output` is written (a stream whose header the reader does not take fails in its own decode instead). param_image and the layout of the output do not
 * depend on the source sizes. All other refusals stand; dec_opt_resize_prescale, dec_opt_resize_prescale_subsampled, dec_opt_resize_filter, the mirror,
 * the output formats and the tensor formats compose with it as they do without; gpujpeg_amd_decoder_get_prescales reports every frame's s_f from its own
 * rectangle and image.
 *   Routing.   The FAMILY of a call are the frames whose header -- SOI up to and including the first SOS header -- is byte for byte the call's reference
 *              header except for the four bytes of SOF0 that hold height and width. The reference header is the one the decoder last decoded a frame
 *              with (a fresh decoder, or one that last saw another sequence: frame 0's, which goes the single-frame route first). Family frames have
 *              the same DQT, DHT, DRI, sampling, scan header and APPn / COM segments; they go through the batched launches, each with the geometry
 *              of its own dimensions. Every other frame -- another quality, restart interval 0, another comment, damaged markers, a segment too long
 *              for the fast entropy decoders, frame 0 of a call whose pixels go to host memory -- goes the single-frame route inside the call.
 *              gpujpeg_amd_decoder_last_batch counts both kinds, gpujpeg_amd_decoder_get_region_stats gives the sums over the frames (equal to the sums
 *              of the single calls); slot [4] of the kernel times is as without the option.
 *   Encoding.  GPUJPEG_ENCODER_RESTART_AUTO-style automatic restart intervals are chosen from the image size, so two images of different size get
 *              different DRI segments and are NOT of one family: encode a dataset meant for this call with one explicit restart interval (and one
 *              quality, sampling and interleaving). */
#define GPUJPEG_AMD_DEC_OPT_BATCH_SIZES "dec_opt_batch_sizes"
#define GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_SAME "same"
#define GPUJPEG_AMD_DEC_BATCH_SIZES_VAL_MIXED "mixed"
/* Decoder option "dec_opt_batch_restartless" = "off" (default) or "on": whether the batch calls -- gpujpeg_amd_decoder_decode_batch, _decode_batch_ptrs
 * (with and without dec_opt_scale), _decode_batch_regions, _decode_batch_crop_resize and _decode_batch_crop_resize_tensor (dec_opt_batch_sizes "same" and
 * "mixed", with the prescale, subsampled-prescale and antialias options) -- take streams WITHOUT restart markers (no DRI segment, restart interval 0:
 * what libjpeg, PIL, OpenCV and cameras write) through their batched launches. Read by every batch call when it starts; it holds from the next call on
 * and may be changed between two calls of a decoder. Another value is refused by gpujpeg_decoder_set_option (GPUJPEG_ERROR) and leaves the setting as it
 * was. With "off" every byte, counter, launch, refusal and kernel-times slot of every call is what it is without the option.
 * WITH "on" it overrides, in the comments of this header, every "restart interval 0" in a list of what goes frame by frame inside a batch call
 * (dec_opt_scale, dec_opt_batch_sizes "Routing", the frame-batch introduction, gpujpeg_amd_decoder_decode_batch_regions and
 * gpujpeg_amd_decoder_decode_batch_crop_resize) and the advice under "Encoding" to give a dataset an explicit restart interval: a folder of files written
 * by one tool at one quality is one family under dec_opt_batch_sizes = mixed as it is. Nothing else of those lists changes: another header, damaged
 * markers, frame 0 of a fresh decoder or of a call with host output, and a small stream of several scans whose SOS / SOS / EOI markers share one 4 KB
 * part of the marker scan still go the single-frame route. Frame f stays, byte for byte (tensor call: bit for bit), what the single-frame call
 * returns for stream f; gpujpeg_amd_decoder_last_batch counts such frames as batched. Entropy decoding is k_huffman_decode_par through the coefficient
 * planes (no token mode for these streams): a scan that does not fit the kernel's 8 KB stage is one workgroup that walks it piece by piece, so it
 * is the BATCH that fills the device, not the frame.
 *   Regions.   A scan without restart markers cannot be entered in the middle: a selection on such a stream is still every segment of every scan, and
 *              gpujpeg_amd_decoder_get_region_stats counts them so (out[0] is 1 where the batched launches took the frames; the single-frame region
 *              call, which is not changed, says 2 and decodes every scan to its end). But it can be LEFT: in a batch of regions or of crop-and-resize
 *              the workgroup stops reading a scan after the piece that completes the last block of the frame's cover (a prescaled frame: the expanded
 *              covering rectangle's). Scans that fit the stage whole are decoded whole. What lies in the batch's coefficient planes behind the
 *              cover is never read: every later call fills the blocks it decodes first.
 *   gpujpeg_amd_decoder_get_entropy_bytes: after a batch call made with "on", out[0] = the entropy-coded bytes (segment-table lengths) of the segments
 *              the batched launches handed to the entropy decoders, summed over the frames they took; out[1] = the bytes of them that were read --
 *              equal unless a scan was left early. Returns 0. After any other call: both 0, returns -1. */
#define GPUJPEG_AMD_DEC_OPT_BATCH_RESTARTLESS "dec_opt_batch_restartless"
#define GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_OFF "off"
#define GPUJPEG_AMD_DEC_BATCH_RESTARTLESS_VAL_ON "on"
/* Decoder option dec_opt_progressive = "off" (default) | "on" (gpujpeg_decoder_set_option): whether gpujpeg_decoder_decode takes PROGRESSIVE streams --
 * frame header SOF2: 8-bit samples, Huffman coding, 1 to 4 components, sampling factors 1 to 4, at most 10 blocks per MCU, 8-bit DQT (what "save for
 * the web", mozjpeg and a few percent of any scraped dataset are). It holds from the next decode call on and may be changed between two calls; another
 * value is refused (GPUJPEG_ERROR) and leaves the setting as it was. With "off" every byte, return code, message, counter, launch and kernel-times slot
 * of every call is what it is without the option, and a SOF2 stream is refused by the reader. gpujpeg_decoder_get_image_info takes no decoder and
 * refuses SOF2 always: gpujpeg_amd_host_stream_info below tells a caller the sizes.
 * WITH "on" the call returns the image the same decoder returns for the stream's BASELINE TWIN -- the SOF0 stream with the same quantisation tables,
 * component ids, sampling, APPn segments and quantised coefficients --, byte for byte, in every output pixel format, colour space and
 * dec_opt_alignment_bytes: the scans fill the quantised coefficient planes (k_huffman_decode_prog, one wave per restart segment of a scan), and
 * everything behind those planes is the plane route of any other frame. So dec_opt_scale works through the coefficient-plane kernels, dec_opt_region
 * too (every segment is decoded: gpujpeg_amd_decoder_get_region_stats reports mode 2), gpujpeg_amd_decoder_read_coefficients after
 * gpujpeg_amd_decoder_keep_coefficients returns the full planes, dec_opt_flipped and dec_opt_channel_remap behave as on any plane-route frame (what
 * that route refuses stays refused). Inside a batch call (decode_batch, _ptrs, _regions, _crop_resize, _crop_resize_tensor, every option of those) a
 * progressive frame goes the single-frame route -- "another header" --, gpujpeg_amd_decoder_last_batch counts it as single, frame f is byte for byte
 * the single call on stream f, and a call may mix baseline and progressive streams freely; with dec_opt_batch_sizes = mixed a progressive stream is
 * never of the family. A progressive frame never launches on a cached header, never takes the device marker scan or token mode (the host walks
 * the stream), and leaves the header cache as it found it -- in host memory and in device memory: while the option is "on", the header of a
 * device-resident stream is brought to the host and compared there before a single-frame call launches on the cached header (one small copy and wait
 * per such call; with "off" the device compares it behind the launch, as ever). The batched launches of a batch call do run over a progressive
 * stream's slot like over any stream with another header, and its frame is decoded again the single-frame way.
 *   Scans.     Any script that is valid under ITU T.81 Annex G: DC scans (Ss = Se = 0) over any non-empty subset of the components, two or more
 *              interleaved; AC scans of one component, 1 <= Ss <= Se <= 63; the first scan of a coefficient has Ah = 0, a refinement Ah = the
 *              Al the coefficient was last coded with and Al = Ah - 1; no AC scan of a component ahead of a DC scan that covers it; Al <= 13; at most
 *              GPUJPEG_AMD_PROGRESSIVE_MAX_SCANS scans (the library's own cap). DHT may redefine a slot in front of any scan: a scan decodes
 *              with the tables as they stand at its SOS. DRI applies to every scan: MCUs in a scan of several components, BLOCKS in a scan of one;
 *              RSTn resets the DC prediction and the EOB run. The stream may end after any whole scan: the scans that are there give the image.
 *              Inside a scan, a segment that ends early reads zero bits, as in the other decoders.
 *   Refused    by the decode call, with a message and a negative return, the decoder usable as before: a script that breaks a rule (the message
 *              names the scan and the rule), more scans than the cap, arithmetic coding (SOF10), 12-bit samples, a scan that names a table
 *              slot that was never defined.
 *   Geometry.  Every component's plane has the padded, whole-MCU layout of the interleaved geometry: pitch blocks_x. A scan of ONE component
 *              codes only ceil(w_c / 8) x ceil(h_c / 8) blocks, w_c = ceil(W H_c / Hmax) and h_c likewise, in raster order INSIDE that pitch; a DC
 *              scan of several components codes whole MCUs of the grid the FRAME's largest factors give, also when it holds a subset of the
 *              components. The padded blocks that scans of one component skip keep the DC their DC scan gave them, and zero AC.
 *   Launches.  Scans whose coefficients do not depend on each other form a LEVEL -- level 0, or 1 + the highest level among the earlier scans that
 *              share a component and a coefficient with the scan -- and are decoded by one launch, the levels one after the other (libjpeg's
 *              ten-scan colour script: 3 levels of 5 + 4 + 1 scans). Kernel-times slot [0] is the sum over those launches (with the clear of the
 *              planes in front of them), slot [4] what the IDCT side sets.
 * gpujpeg_amd_decoder_get_progressive_stats: about the last decode call -- out[0] 1 if the frame was progressive, else 0 (and the rest 0); out[1] scans
 * decoded; out[2] levels = entropy launches; out[3] restart segments of scans = waves launched. Returns 0; -1 with zeros before the first call.
 * gpujpeg_amd_host_stream_info (host only, no device): out[0..2] width, height, components; out[3] 1 for SOF2, else 0; out[4] scans; out[5] levels
 * (a baseline stream: 1); out[6] the restart interval; out[7] 0 for a valid script, else 1 + the first offending scan (more scans than the cap:
 * the cap + 1). Returns 0; -1 when the headers cannot be parsed. */
#define GPUJPEG_AMD_DEC_OPT_PROGRESSIVE "dec_opt_progressive"
#define GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_OFF "off"
#define GPUJPEG_AMD_DEC_PROGRESSIVE_VAL_ON "on"
#define GPUJPEG_AMD_PROGRESSIVE_MAX_SCANS 64
GPUJPEG_API int gpujpeg_amd_decoder_get_progressive_stats(struct gpujpeg_decoder* decoder, long out[4]);
GPUJPEG_API int gpujpeg_amd_host_stream_info(const uint8_t* image, size_t size, int out[8]);
/* Decoder option "dec_opt_batch_progressive" = "off" (default) or "on": whether the batch calls -- gpujpeg_amd_decoder_decode_batch, _decode_batch_ptrs
 * (with and without dec_opt_scale), _decode_batch_regions, _decode_batch_crop_resize and _decode_batch_crop_resize_tensor (with the prescale,
 * subsampled-prescale and antialias options, the mirror, every output and tensor format those calls take) -- take the PROGRESSIVE frames of a call
 * through batched launches of their own. Read by every batch call when it starts; it holds from the next call on and may be changed between two calls
 * of a decoder. Another value is refused by gpujpeg_decoder_set_option (GPUJPEG_ERROR) and leaves the setting as it was. With "off", or with
 * dec_opt_progressive = "off" (a SOF2 stream then fails the call as ever), every byte, counter, launch, refusal, message and kernel-times slot of every
 * call is what it is without the option: a progressive frame goes the single-frame route and gpujpeg_amd_decoder_last_batch counts it as single.
 * WITH "on" (and dec_opt_progressive = "on") it overrides, in the comment of dec_opt_progressive above, "inside a batch call a progressive frame goes
 * the single-frame route" for the progressive frames that form a GROUP. Frame f stays, byte for byte (tensor call: bit for bit), what the single-frame
 * call returns for stream f -- its baseline twin's image --, and gpujpeg_amd_decoder_last_batch counts the frames of a group as batched.
 *   Group.     The candidates are the frames of the call that are still undecoded after frame 0 has gone ahead (fresh decoder, host output, stale
 *              header cache) and the baseline batched launches have run, both exactly as without the option. Among them a group is the progressive
 *              frames that agree in everything the stages behind the coefficient planes read: image width and height; component count, ids and
 *              sampling factors; per component the CONTENTS of its quantisation table (64 values, not the slot number); and what the reader makes of
 *              APPn / Adobe / JFIF (its colour-space decisions, not the segments' bytes). Huffman tables, DHT redefinitions between scans, scan
 *              scripts, restart intervals and a stream that ends after a whole scan may differ freely inside a group: libjpeg writes optimised
 *              tables into every progressive file, so a folder of files saved by one tool at one quality and size is one group although no two of
 *              their headers are byte-equal. A group needs at least 2 frames; a call may hold several groups, which run one after the other. With
 *              dec_opt_batch_sizes = mixed every distinct image size is its own group: per-frame geometry for progressive frames of different sizes
 *              inside one set of launches is NOT built.
 *   Routing.   The single-frame route, with the same message and return code as without the option: a progressive frame in a group of one; a frame
 *              whose headers or scan script the parser refuses; every frame while the decoder is in a state in which the baseline batched launches
 *              decline too (gpujpeg_amd_decoder_keep_coefficients, gpujpeg_amd_decoder_set_fused(0), dec_opt_flipped, dec_opt_channel_remap, the
 *              decoder's own dec_opt_region, a scale the single call refuses). A rectangle the single call would refuse is refused before anything
 *              of the output is written, with the frame named.
 *   Launches.  Per chunk of a group's frames (gpujpeg_amd_decoder_set_batch_chunk) one clear of the chunk's coefficient planes, then level l of ALL
 *              the chunk's frames in ONE k_huffman_decode_prog_batch launch -- as many launches as the chunk's deepest frame has levels, one wave per
 *              restart segment of a scan as in the single-frame kernel, the longest segments of a level first --, then the IDCT side as a baseline
 *              batch has it. The host walks every scan of every candidate whose frame header is SOF2 first (device-resident streams: one
 *              launch gathers the first KB of every stream, then one copy per run of neighbouring progressive streams, one wait). The header
 *              cache is neither read nor written: a baseline batch call afterwards launches on the header it had cached.
 *   Counters.  gpujpeg_amd_decoder_get_region_stats after a batch of regions or of crop-and-resize: the four numbers of the same call with the option
 *              off (a progressive frame contributes mode 2, its scan segments, its cover's blocks). gpujpeg_amd_decoder_get_prescales and
 *              _get_entropy_bytes are unchanged (progressive frames add nothing to the latter). Kernel-times slot [4] is what the last set of batched
 *              launches took. gpujpeg_amd_decoder_get_progressive_stats keeps its meaning: the last single-frame decode inside the call.
 * gpujpeg_amd_decoder_get_progressive_batch_stats: after a batch call made with both options "on", out[0] = frames the batched progressive launches
 * took, out[1] = groups, out[2] = k_huffman_decode_prog_batch launches, out[3] = records (waves). Returns 0. After any other call: zeros, returns -1. */
#define GPUJPEG_AMD_DEC_OPT_BATCH_PROGRESSIVE "dec_opt_batch_progressive"
#define GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_OFF "off"
#define GPUJPEG_AMD_DEC_BATCH_PROGRESSIVE_VAL_ON "on"
GPUJPEG_API int gpujpeg_amd_decoder_get_progressive_batch_stats(struct gpujpeg_decoder* decoder, long out[4]);
/* Decoder option "dec_opt_batch_headers" = "same" (default) or "any": whether the FAMILY of a dec_opt_batch_sizes = mixed call (see there, "Routing")
 * holds only streams whose headers are byte-equal, or every baseline stream of the same SHAPE whatever its tables and marker segments. Read by
 * gpujpeg_amd_decoder_decode_batch_crop_resize and gpujpeg_amd_decoder_decode_batch_crop_resize_tensor alone, and only while dec_opt_batch_sizes = mixed
 * is set (without it the option has no effect); it holds from the next call on and may be changed between two calls of a decoder. Another value is
 * refused by gpujpeg_decoder_set_option (GPUJPEG_ERROR) and leaves the setting as it was. With "same" every byte, counter, launch, refusal, message
 * and kernel-times slot of every call is what it is without the option, and the batched launches run the kernel instantiations they run without it.
 * WITH "any" the definition does not change: frame f is, byte for byte (tensor call: bit for bit), what the same call returns for the one stream f.
 * Only the routing does -- two files saved at different qualities (other DQT), files with optimised Huffman tables (a DHT of their own each) and files
 * that carry Exif, ICC or a comment (other APPn / COM segments, another header length) are of ONE family.
 *   Family.    The reference is the PARSED result of the reference header, chosen as without the option (a fresh decoder: frame 0's, after frame 0
 *              went the single-frame route; the minority rule stands). A frame is of the family when the reader's parse of ITS header agrees with the
 *              reference in: frame type SOF0 with 8-bit samples; component count, component ids and sampling factors; interleaving (the later SOS
 *              headers of a non-interleaved stream are checked when the marker scan has found them); the restart interval ("absent" equals only
 *              "absent"); and everything the reader decides about colour space and pixel format from APPn / JFIF / Adobe and the component ids. Its
 *              DC and AC tables must sit in DHT slots 0 and 1 (no DHT for slot 2 or 3) and fit the two-level decode layout, and it must define every
 *              table it references. Free to differ: width and height; the 64 values of any quantisation table; the contents of any Huffman table;
 *              which slots the components use; number and order of DQT / DHT segments; APPn / COM segments; so also the length of the header, up to
 *              64 KB. A non-interleaved stream in DEVICE memory is taken with the reference's table selectors for its second and later scans (its
 *              own are not known before the launch); where they turn out to be others the frame goes the single-frame route.
 *   Routing.   The single-frame route inside the call, with the message and return code it has without the option: another sampling, component count
 *              or restart interval; a progressive stream (unless dec_opt_batch_progressive takes it); a DHT in slot 2 or 3; a table that does not fit
 *              the layout; a header longer than 64 KB; damaged markers; a segment too long for the fast entropy decoder. Every rectangle is checked
 *              against its own stream's image before anything of `output` is written.
 *   Tables.    One TABLE SET -- the uint16 and float inverse quantisation tables and the four two-level Huffman tables -- per distinct content of the
 *              DQT values and DHT bits / values the frame's components reference (a folder of files with the Annex K tables at one quality is one
 *              set whatever its comments say, and whichever slots its files use); all sets go to the device in one upload; every frame carries the
 *              index of its set and the offset of its first scan byte. The marker scan treats the bytes in front of a frame's own scan as it treats
 *              the bytes in front of the scan of a byte-equal family: an Exif thumbnail -- a complete JPEG with SOS, RSTn and EOI inside APP1 --
 *              reaches no table entry and no count. Device-resident streams: one launch gathers the first 4 KB of every stream; a header that does
 *              not end inside them is fetched on its own, one wait for all of those.
 *   State.     Family frames neither read nor write the header cache beyond what a "mixed" call does: a "same" call on a byte-equal family afterwards
 *              behaves as if the "any" call had been a "mixed" call. Everything dec_opt_batch_sizes = mixed composes with composes with "any":
 *              dec_opt_batch_restartless (files from libjpeg have no DRI), the prescales, the antialias filter, the mirror, the output and tensor
 *              formats, gpujpeg_amd_decoder_set_batch_chunk and dec_opt_batch_progressive, whose pass runs after the baseline launches.
 * gpujpeg_amd_decoder_get_batch_header_stats: after a crop-and-resize call made with "any" (and "mixed"), out[0] = frames the host admitted to the
 * family, out[1] = distinct table sets uploaded, out[2] = header bytes brought to the host, out[3] = frames whose header did not end within the first
 * gather window and was fetched on its own. Returns 0. After any other call: zeros, returns -1. */
#define GPUJPEG_AMD_DEC_OPT_BATCH_HEADERS "dec_opt_batch_headers"
#define GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_SAME "same"
#define GPUJPEG_AMD_DEC_BATCH_HEADERS_VAL_ANY "any"
GPUJPEG_API int gpujpeg_amd_decoder_get_batch_header_stats(struct gpujpeg_decoder* decoder, long out[4]);
/* Where the host's look at the headers of that call spent its time, in milliseconds of the host's clock: ms[0] = bringing the headers of
 * device-resident streams to the host (the gather launch, the copies of long headers, their waits; 0 for streams in host memory), ms[1] = the
 * reader's parse of every header, ms[2] = the family rule, the table keys, building the distinct table sets and the frames' geometries. Returns 0
 * after a call made with "any" (and "mixed"); after any other call: zeros, returns -1. */
GPUJPEG_API int gpujpeg_amd_decoder_get_batch_header_times(struct gpujpeg_decoder* decoder, double ms[3]);
/* Host-only: the table enc_opt_huffman=optimal builds for one class from symbol counts freq[256] (ITU T.81 Annex K.2: Figures K.1, K.3, K.4;
 * reserved code point, ties to the larger symbol value), code lengths limited to the largest L of 16 .. 10 whose table the library's
 * two-level decode tables take. Writes BITS (bits[1..16]) and HUFFVAL; returns L, or -1 when no count is non-zero. */
GPUJPEG_API int gpujpeg_amd_host_huffman_optimal(const uint32_t freq[256], uint8_t bits[17], uint8_t vals[256]);

/* per-kernel durations (ms, hipEvents on the coder's stream) of the last call made with perf_stats != 0:
 * encoder: [0] preprocess, [1] DCT+quant (fused path: preprocess included), [2] k_huffman or k_encode_*, [3] k_gather (behind k_huffman:
 *          k_scan_segments), [4] k_assemble (behind k_huffman only), [5] k_huffman_count (enc_opt_huffman=optimal; 0 otherwise)
 * decoder: [0] entropy decoder, [1] IDCT (fused path: postprocess included), [2] postprocess, [3] marker scan (k_markers; 0 when the host walked the stream),
 *          [4] not a duration: the IDCT side of that call -- 0 full size, 1 reduced size from the coefficient planes (k_idct_scaled), 2 reduced size from
 *          tokens (k_idct_tok_scaled_rgb444), 3 region from the coefficient planes (k_idct_region), 4 region from tokens (k_idct_tok_region_rgb444),
 *          5 region resampled from the cover planes (k_idct_region + k_resize_region: gpujpeg_amd_decoder_decode_batch_crop_resize),
 *          gpujpeg_amd_decoder_decode_batch_regions leaves the side its batched launches took here (3 or 4) and no durations, and so do
 *          6 the same with at least one frame of the call reduced ahead of the resample (k_idct_region_scaled: dec_opt_resize_prescale);
 *          gpujpeg_amd_decoder_decode_batch with a dec_opt_scale (1 or 2) and gpujpeg_amd_decoder_decode_batch_crop_resize (5, 6 or 7);
 *          7 region resampled from the cover planes with the antialiased filter (k_idct_region + k_resize_region_aa: dec_opt_resize_filter = antialias);
 *          8 as 6 with at least one frame reduced per component (k_idct_region_scaled_comp: dec_opt_resize_prescale_subsampled) */
GPUJPEG_API int gpujpeg_amd_encoder_get_kernel_times(struct gpujpeg_encoder* encoder, float ms[8]);
GPUJPEG_API int gpujpeg_amd_decoder_get_kernel_times(struct gpujpeg_decoder* decoder, float ms[8]);

/* ---- frame batches: many frames of ONE geometry behind one set of kernel launches --------------------------------------------------
 * The libgpujpeg API codes a frame per call. An HD frame is 135 workgroups of the encoder kernel on a device with 1024 places for them,
 * and a call is 2 (encode) or 4 (decode) dependent launches: frame-at-a-time calls cannot fill an MI355X with small frames however many
 * coders run side by side. These two calls take `count` frames that share parameters (encoder) or the header (decoder) and launch every
 * kernel once per chunk of frames (the frame is a grid dimension). Results are identical, byte for byte, to the frame-at-a-time calls;
 * configurations (restart interval 0, flip, channel remap, APP13 index) or streams (another header, damaged markers) the batched kernels do
 * not cover are coded frame by frame inside the call.
 *
 * gpujpeg_amd_encoder_encode_batch: frame f lies at frames + f * frame_stride (device memory = GPU_IMAGE semantics, or host memory: copied);
 *   images_compressed[f] / images_compressed_size[f] receive every frame's stream -- in device memory with enc_opt_out=device, else in
 *   pinned / pageable host memory -- owned by the encoder and valid until its next call. The streams lie a constant number of bytes apart
 *   (images_compressed[1] - images_compressed[0], a multiple of 16), so the pointers can go straight into gpujpeg_amd_decoder_decode_batch.
 *   perf_stats / get_stats are not kept for batch calls.
 * gpujpeg_amd_decoder_decode_batch: stream f lies at streams + f * stream_stride and has sizes[f] bytes (device or host memory); frame f's
 *   pixels go to output + f * output_stride (device memory) in the format set with gpujpeg_decoder_set_output_format. All streams must
 *   decode to the same image parameters; returns 0 when every frame was decoded. */
GPUJPEG_API int gpujpeg_amd_encoder_encode_batch(struct gpujpeg_encoder* encoder, const struct gpujpeg_parameters* param,
                                                 const struct gpujpeg_image_parameters* param_image, const uint8_t* frames, size_t frame_stride,
                                                 int count, uint8_t** images_compressed, size_t* images_compressed_size);
/* The same for frames / streams / destinations that are separate buffers (device or host memory, mixed if need be): buffers that lie a constant
 * distance apart are coded where they are, others are gathered into (scattered from) a staging buffer with one copy per frame on the coder's
 * stream. frame_bytes: room in every destination (>= the decoded frame). */
GPUJPEG_API int gpujpeg_amd_encoder_encode_batch_ptrs(struct gpujpeg_encoder* encoder, const struct gpujpeg_parameters* param,
                                                      const struct gpujpeg_image_parameters* param_image, const uint8_t* const* frames, int count,
                                                      uint8_t** images_compressed, size_t* images_compressed_size);
GPUJPEG_API int gpujpeg_amd_decoder_decode_batch_ptrs(struct gpujpeg_decoder* decoder, const uint8_t* const* streams, const size_t* sizes, int count,
                                                      uint8_t* const* outputs, size_t frame_bytes, struct gpujpeg_image_parameters* param_image);
/* frames per set of launches at most (0 = the default: up to 256, fewer for large frames whose work buffers would exceed 6 / 8 GB); tests use it to cut
 * small batches into several chunks */
GPUJPEG_API void gpujpeg_amd_encoder_set_batch_chunk(struct gpujpeg_encoder* encoder, int frames);
GPUJPEG_API void gpujpeg_amd_decoder_set_batch_chunk(struct gpujpeg_decoder* decoder, int frames);
/* how the frames of the last batch call were coded: by the batched launches / frame by frame inside the call (tests, benchmarks) */
GPUJPEG_API int gpujpeg_amd_encoder_last_batch(struct gpujpeg_encoder* encoder, int* batched, int* single);
GPUJPEG_API int gpujpeg_amd_decoder_last_batch(struct gpujpeg_decoder* decoder, int* batched, int* single);
/* how the decode calls of this decoder ran so far (tests, benchmarks): [0] launched speculatively on the cached header of the previous frame,
 * [1] of those, without the marker scan's second launch (the token decoder derived its segment table from the scan's records itself),
 * [2] speculative launches whose stream turned out not to be what was assumed and that were decoded again the careful way */
GPUJPEG_API int gpujpeg_amd_decoder_get_path_counters(struct gpujpeg_decoder* decoder, long counters[3]);
GPUJPEG_API int gpujpeg_amd_decoder_decode_batch(struct gpujpeg_decoder* decoder, const uint8_t* streams, size_t stream_stride, const size_t* sizes,
                                                 int count, uint8_t* output, size_t output_stride, struct gpujpeg_image_parameters* param_image);
/* what the last decode call did with dec_opt_region (taken from what was launched and from the device's selection result): out[0] mode: 0 = no
 * region, 1 = region, entropy-decoded the selected restart segments only, 2 = region, every segment entropy-decoded (fallback); out[1] restart
 * segments handed to the entropy decoder; out[2] 8x8 blocks the IDCT side transformed; out[3] segments in the stream */
GPUJPEG_API int gpujpeg_amd_decoder_get_region_stats(struct gpujpeg_decoder* decoder, long out[4]);
/* entropy-coded bytes handed to / read by the entropy decoders of the batched launches of the last batch call made with dec_opt_batch_restartless = on
 * (see there); 0, or -1 with both words 0 after any other call */
GPUJPEG_API int gpujpeg_amd_decoder_get_entropy_bytes(struct gpujpeg_decoder* decoder, uint64_t out[2]);
/* A batch of regions: gpujpeg_amd_decoder_decode_batch with one crop per frame -- frame f is the `width` x `height` pixels at
 * (origins[2f], origins[2f + 1]) of stream f's image. The bytes at output + f * output_stride are exactly what gpujpeg_decoder_decode of this decoder
 * returns for stream f with dec_opt_region = "X_f,Y_f,width,height" (every output format and colour space, dec_opt_alignment_bytes, the planar crop
 * rules); param_image and the frame size are those of a width x height image. streams, stream_stride, sizes, output (device or host memory) and
 * output_stride as for gpujpeg_amd_decoder_decode_batch. The decoder's own dec_opt_region is neither read nor changed by the call.
 * Every configuration the full-frame batch covers goes through batched launches: the frame is a grid dimension of the region kernels, every frame's
 * restart segments are selected against its own cover, and the host waits once per chunk of frames. Restart interval 0, a stream with another header
 * or with damaged markers: that frame goes through the single-frame region call inside this one.
 * Refused with a message, -1 returned, nothing of `output` written, the decoder usable as before: width or height < 1; an origin whose rectangle
 * the single-frame call would refuse (outside the image, off the output format's sampling grid: the message names the frame); a dec_opt_scale other
 * than 1; dec_opt_flipped.
 * Afterwards gpujpeg_amd_decoder_last_batch counts the frames as for decode_batch, and gpujpeg_amd_decoder_get_region_stats gives out[1..3] as sums
 * over the call's frames, out[0] = 1 when every frame was entropy-decoded from its selected segments only, else 2. */
GPUJPEG_API int gpujpeg_amd_decoder_decode_batch_regions(struct gpujpeg_decoder* decoder, const uint8_t* streams, size_t stream_stride,
                                                         const size_t* sizes, int count, const int* origins, int width, int height, uint8_t* output,
                                                         size_t output_stride, struct gpujpeg_image_parameters* param_image);
/* Crop-and-resize, one rectangle per frame: frame f is the rects[4f + 2] x rects[4f + 3] pixels at (rects[4f], rects[4f + 1]) of stream f's image,
 * resampled to out_width x out_height and, where mirror != NULL and mirror[f] != 0, mirrored horizontally -- the random-resized crop (and flip) of a
 * training pipeline in one call, every rectangle with its own size and aspect. streams, stream_stride, sizes, output (device or host memory) and
 * output_stride as for gpujpeg_amd_decoder_decode_batch_regions; pixel format and colour space are the ones set with
 * gpujpeg_decoder_set_output_format, dec_opt_alignment_bytes applies to the out_width line, param_image and the frame size are those of an
 * out_width x out_height image. The decoder's own dec_opt_region is neither read nor changed.
 * DEFINITION. Let C be the w x h image gpujpeg_decoder_decode of this decoder returns for stream f with dec_opt_region = "x,y,w,h", taken channel by
 * channel, OW = out_width, OH = out_height; integers throughout, division = floor, arithmetic shifts:
 *     nx = max((2 i + 1) w - OW, 0);  x0 = nx / (2 OW);  fx = ((nx - x0 2 OW) 256) / (2 OW);  x1 = min(x0 + 1, w - 1)          i < OW
 *     ny, y0, fy, y1 likewise from j, h, OH                                                                                  j < OH
 *     top = C[y0][x0] (256 - fx) + C[y0][x1] fx;   bot = C[y1][x0] (256 - fx) + C[y1][x1] fx
 *     R[j][i] = (top (256 - fy) + bot fy + 32768) >> 16;    out[j][i] = mirror && mirror[f] ? R[j][OW - 1 - i] : R[j][i]
 * Bilinear interpolation with half-pixel centres (align_corners = false, no antialiasing) with 8-bit weights, on output pixels -- after the colour
 * transform --, the identity for w == OW and h == OH. The fourth byte of GPUJPEG_4444_U8_P0123 goes through the same formula (0xFF stays 0xFF).
 * Output formats: those whose pixels share no samples (GPUJPEG_U8, GPUJPEG_444_U8_P012, GPUJPEG_444_U8_P0P1P2, GPUJPEG_4444_U8_P0123); they take any
 * rectangle inside the image of a stream of any sampling.
 * The frames go through the batched launches of the batch of regions on the coefficient-plane route (every frame's restart segments selected against
 * its own cover, k_idct_region) with the resampling kernel k_resize_region as the pixel stage; a frame the batched launches do not cover (restart
 * interval 0, another header, damaged markers, the first frame of a decoder's life, frame 0 of a call whose pixels go to host memory) goes through
 * the single-frame region call with the same kernel as its pixel stage: the same bytes.
 * Refused with a message, -1 returned, nothing of `output` written, the decoder usable as before: out_width or out_height outside 1 .. 16384; a
 * rectangle with w or h < 1 or not inside the stream's image (the message names the frame); an output format whose pixels share samples (packed or
 * planar 4:2:2, planar 4:2:0); a dec_opt_scale other than 1; dec_opt_flipped; a dec_opt_channel_remap.
 * Afterwards gpujpeg_amd_decoder_last_batch and gpujpeg_amd_decoder_get_region_stats count as for gpujpeg_amd_decoder_decode_batch_regions, and slot
 * [4] of gpujpeg_amd_decoder_get_kernel_times is 5.
 * WITH dec_opt_resize_prescale = 1/S. Frame f with rectangle (x, y, w, h) takes the scale s_f = the largest s of 1, 2, 4, 8 with s <= S, w >= s OW and
 * h >= s OH (the bilinear step then reduces by less than 2 per axis); s_f = 1 for a stream with a component whose sampling is not 1 x 1 (dec_opt_scale
 * reduces subsampled chroma by the same N as luma: at 1/8 one sample per 16 x 16 pixels, worse than no prescale; dec_opt_resize_prescale_subsampled = on reduces 4:2:0 per component instead: see the
 * option). With s_f = 1 the frame is as above.
 * With s = s_f > 1 let Rs be the image gpujpeg_decoder_decode of this decoder returns for stream f with dec_opt_scale = 1/s, and
 *     x' = x / s;  w' = ceil((x + w) / s) - x';  y', h' likewise;  C' = the w' x h' crop of Rs at (x', y')  (inside Rs because x + w <= W)
 *     d  = 2 OW s;  nx = max((2 i + 1) w + 2 OW (x - s x') - OW s, 0);  x0 = nx / d;  fx = ((nx - x0 d) 256) / d;  x1 = min(x0 + 1, w' - 1)
 *     ny, y0, fy, y1 likewise from j, h, y, y', h', OH;  top, bot, R and the mirror as above with C' for C.
 * The source position is ((x + (i + 1/2) w / OW) / s) - 1/2 in reduced pixels, exactly: the rectangle does not move (resizing the covering rectangle
 * with the taps above would move it by up to s - 1 pixels); x0 <= w' - 1 always; for s = 1 the lines are the ones above term for term.
 * The cover of such a frame is the one the region call has for (x' s, y' s, min(w' s, W - x' s), min(h' s, H - y' s)): selection and entropy decoding
 * as before, k_idct_region_scaled for its blocks (N = 8 / s samples per block edge), k_resize_region over the reduced cover planes; a batch mixes
 * scales freely, and the single-frame route takes the same kernels: the same bytes. Refusals are the same and are made on the caller's rectangle.
 * Afterwards gpujpeg_amd_decoder_get_prescales gives s_f of every frame, slot [4] of the kernel times is 6 when any s_f > 1 (else 5),
 * gpujpeg_amd_decoder_get_region_stats counts the covers as launched (out[2]: their 8x8 blocks), and gpujpeg_amd_decoder_read_planes returns the last
 * frame's cover-sized buffer whose first bytes are its REDUCED cover planes (component c: offset N N / 64 of the cover plane's, pitch N / 8 of its). */
GPUJPEG_API int gpujpeg_amd_decoder_decode_batch_crop_resize(struct gpujpeg_decoder* decoder, const uint8_t* streams, size_t stream_stride,
                                                             const size_t* sizes, int count, const int* rects, const uint8_t* mirror, int out_width,
                                                             int out_height, uint8_t* output, size_t output_stride,
                                                             struct gpujpeg_image_parameters* param_image);
/* Crop-and-resize with a normalised float tensor as its result: the call above with one more pixel stage -- what a training pipeline otherwise does in
 * a pass of its own over the batch (uint8 -> float, HWC -> CHW, (x / 255 - mean) / std, cast), done where the pixel is still in registers.
 * DEFINITION. Let R_f be the bytes gpujpeg_amd_decoder_decode_batch_crop_resize of this decoder returns for frame f with every other argument the same
 * (mirror, dec_opt_resize_prescale, output colour space), taken as R_f[j][i][c]; C = 1 where that call's pixel format is GPUJPEG_U8, 3 where it is
 * GPUJPEG_444_U8_P012 or GPUJPEG_444_U8_P0P1P2 (the two give the same tensor: the layout is format->layout); OW = out_width, OH = out_height. Then
 *     T_f(c, j, i) = cvt(fadd(fmul((float)R_f[j][i][c], format->scale[c]), format->bias[c]))                                  c < C, j < OH, i < OW
 * fmul and fadd each round to nearest-even in binary32 and are never fused into one operation; cvt is the identity for GPUJPEG_AMD_TENSOR_F32 and
 * round-to-nearest-even for GPUJPEG_AMD_TENSOR_F16 (subnormals are produced, not flushed; overflow gives infinity) and GPUJPEG_AMD_TENSOR_BF16.
 * The usual recipe is scale[c] = 1 / (255 std[c]), bias[c] = -mean[c] / std[c]; it differs from (x / 255 - mean) / std in the last place of some elements.
 * LAYOUT. GPUJPEG_AMD_TENSOR_CHW: element (c, j, i) at index (c OH + j) OW + i; GPUJPEG_AMD_TENSOR_HWC: at (j OW + i) C + c. Frames are dense; frame f
 * starts output_stride BYTES behind frame f - 1; output_stride is a multiple of the element size (4, 2, 2) and at least C OW OH times it. `output` is
 * device or host memory, as above. param_image is what the call above reports.
 * Routing, fallbacks, gpujpeg_amd_decoder_last_batch, _get_region_stats, _get_prescales and slot [4] of the kernel times are exactly those of the call above
 * on the same arguments: the batched launches end in k_resize_region_tensor_batch in place of k_resize_region_batch, the single-frame route in
 * k_resize_region_tensor. The decoder's own dec_opt_region is neither read nor changed, and no later call of the decoder sees anything of the format.
 * Refused with a message, -1 returned, nothing of `output` written, the decoder usable as before: everything the call above refuses, and format == NULL;
 * a dtype or layout outside the enums; a scale or bias among the first C that is not finite; a pixel format other than the three above
 * (GPUJPEG_4444_U8_P0123 included); a dec_opt_alignment_bytes greater than 1; an `output` or output_stride that is not a multiple of the element size; an
 * output_stride smaller than a frame. */
enum { GPUJPEG_AMD_TENSOR_F32 = 0, GPUJPEG_AMD_TENSOR_F16 = 1, GPUJPEG_AMD_TENSOR_BF16 = 2 };
enum { GPUJPEG_AMD_TENSOR_CHW = 0, GPUJPEG_AMD_TENSOR_HWC = 1 };
struct gpujpeg_amd_tensor_format { int dtype, layout; float scale[4], bias[4]; }; /* 40 bytes; scale / bias [3] reserved */
GPUJPEG_API int gpujpeg_amd_decoder_decode_batch_crop_resize_tensor(struct gpujpeg_decoder* decoder, const uint8_t* streams, size_t stream_stride,
                                                                    const size_t* sizes, int count, const int* rects, const uint8_t* mirror, int out_width,
                                                                    int out_height, const struct gpujpeg_amd_tensor_format* format, void* output,
                                                                    size_t output_stride, struct gpujpeg_image_parameters* param_image);
/* Host-only: the bits that call stores for the 8-bit value v (0 .. 255) of channel c (0 .. 2) -- a float's 32 bits, or the 16 bits of a binary16 /
 * bfloat16 in the low half; the code the call itself runs. 0 for arguments outside those ranges, a NULL format or a dtype outside the enum. */
GPUJPEG_API uint32_t gpujpeg_amd_host_tensor_element(const struct gpujpeg_amd_tensor_format* format, int channel, int v);
/* Host-only: scale and covering rectangle dec_opt_resize_prescale gives ONE frame of a crop-and-resize call -- rect = x, y, w, h in an
 * image_w x image_h image whose components are (all_components_1x1 != 0) or are not all sampled 1 x 1, output out_w x out_h, max_scale = S (1, 2, 4, 8).
 * Writes out = s, x', y', w', h' (the definition above; the code the call itself runs) and returns 0, or -1 where the call would refuse: a rectangle
 * with w or h < 1 or not inside the image, an output size outside 1 .. 16384, another max_scale. Callers pass all_components_1x1 != 0 as well for a
 * stream that is eligible under dec_opt_resize_prescale_subsampled = on (above): its frames take the same plan. */
GPUJPEG_API int gpujpeg_amd_host_crop_resize_plan(int image_w, int image_h, int all_components_1x1, const int rect[4], int out_w, int out_h, int max_scale,
                                                  int out[5]);
/* Host-only: the taps dec_opt_resize_filter = antialias gives output sample i (0 .. n_out - 1) along one axis of n_src source samples resampled to
 * n_out, by the code the call itself runs: *first = the first source sample with a positive weight, *count = how many follow each other from there,
 * weights[0 .. count) = u_i(first + t) of the definition above, *sum = their sum U_i. Every pointer may be NULL (not wanted); `capacity` = room in
 * `weights`. Returns 0; -1 where the call would refuse (n_src outside 1 .. 65535, n_out outside 1 .. 16384, i outside the output, n_src > 256 n_out);
 * -2 when capacity < count (first, count and sum are written, weights is not). */
GPUJPEG_API int gpujpeg_amd_host_resize_weights(int n_src, int n_out, int i, int* first, int* count, uint32_t* weights, int capacity, uint64_t* sum);
/* s_f of every frame of the decoder's last gpujpeg_amd_decoder_decode_batch_crop_resize call, as launched: dst[f], one byte per frame. Returns the
 * frame count, or 0 on error (no such call yet, the last one failed, capacity too small). */
GPUJPEG_API int gpujpeg_amd_decoder_get_prescales(struct gpujpeg_decoder* decoder, uint8_t* dst, int capacity);
/* Orientation for callers of the crop-and-resize calls. The batch calls return pixels in STORED orientation and do not look at the orientation a
 * stream carries (Exif APP1 tag 0x0112 of IFD0 in either byte order, or the SPIFF directory entry: gpujpeg_decoder_output::metadata of the single
 * call). The two host-only functions below give a caller what it takes to honour it without parsing Exif or restating the geometry:
 * (rot, flip) is what the reader's metadata holds -- rot quarter turns clockwise, then mirrored left-right if flip; (0, 0) when nothing set it; a flawed
 * tag or a truncated Exif block counts as not set, exactly as the reader decides. The DISPLAY image D of the stored W x H image I is I turned clockwise by
 * rot quarter turns, then mirrored left-right if flip (numpy: np.rot90(I, k=-rot), then [:, ::-1]); D is H x W for odd rot.
 * Out of scope here: applying the orientation inside any decode call; writing or rewriting Exif; any change to the reader's orientation parsing. */
/* Host-only, no device: the orientation the reader finds in a stream's headers. out = set (0 / 1), rotation, flip, display width, display height
 * (rotation and flip 0 when not set). Returns 0, or -1 when the headers cannot be parsed. */
GPUJPEG_API int gpujpeg_amd_host_stream_orientation(const uint8_t* image, size_t size, int out[5]);
/* Host-only: rect = x, y, w, h in the display image of an image_w x image_h stored image with `rotation` (0 .. 3) and `flip`, to be resampled to
 * out_w x out_h pixels of the display orientation and, with mirror != 0, mirrored once more. Writes out = x', y', w', h' -- the rectangle's pre-image in the
 * stored image: what to hand to gpujpeg_amd_decoder_decode_batch_crop_resize --, OW', OH' -- the output size to ask that call for: out_w x out_h, swapped
 * for odd rotations --, bits, 0, and returns 0. With R' the OW' x OH' frame that call returns (no mirror), pixel (i, j) of the display-oriented result is
 * pixel (i', j') of R':  (a, b) = bits & 4 ? (j, i) : (i, j);  i' = bits & 1 ? OW' - 1 - a : a;  j' = bits & 2 ? OH' - 1 - b : b  -- in numpy
 * np.rot90(R', -rotation), then [:, ::-1] if flip, then [:, ::-1] if mirror. With rotation = flip = 0 the rectangle and the size come back as given and
 * bits is the mirror flag. Returns -1 for a rectangle with w or h < 1 or not inside the display image, an output size outside 1 .. 16384, a rotation
 * outside 0 .. 3. */
GPUJPEG_API int gpujpeg_amd_host_orientation_plan(int image_w, int image_h, int rotation, int flip, const int rect[4], int out_w, int out_h, int mirror,
                                                  int out[8]);

#ifdef __cplusplus
}
#endif
#endif
