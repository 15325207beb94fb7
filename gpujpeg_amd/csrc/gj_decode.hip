// gj_decode.hip -- MI355X (gfx950, wave64) JPEG decoder: gj_hip_decode picks the kernels of a frame and launches them.
// The kernels live in gj_dec_*.hip (map: gj_dec_internal.h).
#include "gj_dec_internal.h"

// Does a frame of this geometry and stream size go through token mode (given fused kernels and two-level Huffman tables)? The host
// asks before it allocates the token buffers; the launcher asks again.
// Measured (8K / 16K RGB natural frames at q75, 4.75 B of stream per block: +17 % enc+dec; HD and 4K equal or slightly slower;
// 8K noise -15 %; crossover at 8K RGB near 9 B per block): tokens pay when the frame fills the GPU more than once (the token-fed IDCT has
// the longer dependency chain per workgroup) and blocks carry few coefficients (2 B per coefficient against 128 B per block).
// gj_tuning::dec_tokens forces either mode (tests, A/B runs).
extern "C" int gj_hip_decode_wants_tokens(const gj_geom* g, uint64_t jpeg_size, const gj_tuning* tune)
{
    if (tune->dec_tokens == 0 || gj_idct_tok_for(*g) == nullptr) return 0;
    if (g->seg_blocks > GJ_TOK_MAX_BLOCKS || g->restart_interval == 0) return 0; // (k_huffman_decode_tok takes whole segments into its LDS stage)
    if (tune->dec_sub) return 0; // (the tuning aid sweeps the plane-mode kernels)
    if (tune->dec_tokens == 1) return 1;
    // (interleaved scans -- packed 4:2:2, BASELINE config 4 at q90: 10.4 B per block -- go through the lane-per-segment kernel, whose plane mode
    // pays for the zero fill and the scattered stores of 128-byte blocks: tokens win up to denser streams there)
    // (round 3, k_huffman_decode_tok: a 4K RGB frame -- 389 K blocks -- gains 9 % enc+dec and 7 % decode-only, an HD frame loses 4 %)
    // (a batch of frames, gj_frame_strides: the blocks of all its frames fill the GPU, so HD frames take token mode too)
    const uint64_t blocks_in_flight = (uint64_t)g->block_count * (g->fb.frames > 1 ? g->fb.frames : 1u);
    // (round 5, k_huffman_decode_tok on denser streams: the camera frame at q100, 11.8 B per block, decodes 11 % faster through tokens than through the
    // planes -- 133.6 against 120.0 Gpix/s decode-only --; `.tst` noise at q75, 26.8 B per block, 5 % slower -- 34.7 against 36.7: the entropy stage takes
    // 0.908 ms either way, ~2.2 symbols per byte at a sub-sequence hit rate that noise's long codes halve, and the token-fed IDCT then moves as many bytes
    // as the planes would. The gate for non-interleaved scans moves from 8 to 16 B per block.)
    return blocks_in_flight >= (g->interleaved ? 900000u : 300000u) && jpeg_size <= (uint64_t)g->block_count * (g->interleaved ? 12u : 16u);
}

// A batch of frames (gj_dec_job::batch) is a speculative launch on one header through the sub-sequence entropy decoders -- tokens for non-interleaved
// 4:4:4, coefficient planes for everything else (the lane-per-segment kernels and the token-fed 4:2:2 IDCT do not know the frame dimension) -- and any
// of the IDCT-side kernels; no option that touches other buffers. Streams without restart markers -- one segment per scan, which k_huffman_decode_par
// decodes piece by piece, plane mode (gj_hip_decode_wants_tokens says no) -- where the job asks for them (gj_dec_job::batch_restartless).
extern "C" int gj_hip_decode_batchable(const gj_dec_job* job)
{
    const gj_geom& g = job->g;
    // (a chunk of progressive frames, gj_dec_job::prog with gj_prog_plan::d_frames: its own entropy stage -- no segment table, no two-level tables, no
    // overflow word, and restart intervals are the records' business --, the same IDCT-side kernels)
    if (job->prog != nullptr)
        return job->prog->d_frames != nullptr && !job->flipped && !job->channel_remap && !job->tokens && !job->scan.valid && !job->region.select && g.fb.geoms == nullptr &&
               job->batch.d_geoms == nullptr;
    return job->d_huff_tab2 != nullptr && job->d_overflow != nullptr && job->d_seg_count != nullptr && job->seg_count > 0 &&
           !job->flipped && !job->channel_remap && !job->clear_coefs && !job->tune.dec_serial && !job->tune.dec_careful && job->tune.dec_seq != 1 &&
           (g.restart_interval > 0 || job->batch_restartless);
}

extern "C" int gj_hip_decode(const gj_dec_job* job, gj_stream_t stream, gj_event_t ev[4])
{
    hipStream_t st = (hipStream_t)stream;
    const gj_geom& g = job->g;
    if (g.blocks_per_mcu > GJ_MAX_MCU_BLOCKS) return -1;
    if ((job->batch.count > 1 || g.fb.sizes != nullptr) && (!gj_hip_decode_batchable(job) || g.fb.sizes == nullptr || job->batch.count > 65535u)) return -1;
    // (a reduced-size decode: no flip; a batch: the pixel kernels find frame z's reduced planes and pixels through gs.fb, which must be g.fb)
    if (job->scale > 1 && ((job->scale != 2 && job->scale != 4 && job->scale != 8) || job->flipped ||
                           (g.fb.sizes != nullptr && (job->gs.fb.sizes != g.fb.sizes || job->gs.fb.coefs != g.fb.coefs || job->gs.fb.raw != g.fb.raw))))
        return -1;
    const gj_region& rg = job->region;
    // (a region call: no scale, no flip; with a selection, room for the compacted table and its counts. A single frame -- or a batch of regions,
    // gj_region::d_frames: always with a selection, compacted tables at the frames' table stride, the found counts of every frame)
    const bool rg_batch = rg.on && rg.d_frames != nullptr;
    // (crop-and-resize, gj_region::resize: the plane route only -- the host leaves gj_dec_job::tokens 0 --, an output size the taps' arithmetic takes,
    // no channel remap)
    if (rg.on && rg.resize && (job->tokens || job->channel_remap || job->gs.width < 1 || job->gs.height < 1 || job->gs.width > GJ_RESIZE_MAX_OUT ||
                               job->gs.height > GJ_RESIZE_MAX_OUT || job->gs.raw_width != job->gs.width))
        return -1;
    // (a tensor, gj_region::tensor: the store of a resize job alone; an element type and a layout the store knows; one channel for single-channel
    // output, three for packed or planar 4:4:4; gs.raw_size is the tensor's, and in a batch the frames lie whole elements apart)
    if (rg.on && rg.tensor.on &&
        (!rg.resize || rg.tensor.dtype < GJ_TENSOR_F32 || rg.tensor.dtype > GJ_TENSOR_BF16 || (rg.tensor.layout != GJ_TENSOR_CHW && rg.tensor.layout != GJ_TENSOR_HWC) ||
         rg.tensor.channels != (job->gs.pixel_format == GJ_PF_U8 ? 1 : 3) || (job->gs.pixel_format != GJ_PF_U8 && job->gs.pixel_format != GJ_PF_444_P012 && job->gs.pixel_format != GJ_PF_444_P0P1P2) ||
         job->gs.raw_size != (uint64_t)rg.tensor.channels * job->gs.width * job->gs.height * GJ_TENSOR_ELSIZE(rg.tensor.dtype) ||
         ((uintptr_t)job->d_raw | (g.fb.sizes != nullptr ? (uintptr_t)job->gs.fb.raw : 0)) % GJ_TENSOR_ELSIZE(rg.tensor.dtype) != 0))
        return -1;
    // (a scale per frame, gj_region_frame::scale: inside a resize job alone -- dec_opt_resize_prescale --, one of 1, 2, 4, 8; gj_dec_job::scale stays 1)
    // (... and the frames reduced per component, gj_region_frame::per_comp, in comp_mask instead: scales 2, 4, 8, inside a resize job alone; a single
    // frame is in the mask of its kind alone)
    if (rg.on && ((rg.scale_mask & ~(rg.resize ? 0xFu : 1u)) != 0 || (rg.comp_mask & ~(rg.resize ? 0xEu : 0u)) != 0 ||
                  (!rg_batch && rg.frame.scale > 1 &&
                   (!rg.resize || (rg.frame.per_comp ? rg.comp_mask : rg.scale_mask) != (unsigned)rg.frame.scale || (rg.frame.per_comp ? rg.scale_mask : rg.comp_mask) != 0u)) ||
                  (!rg_batch && rg.frame.scale <= 1 && (rg.frame.per_comp || rg.comp_mask))))
        return -1;
    // (a filter, gj_region::filter: one the pixel stage knows; the antialiased one inside a resize job alone and over frames of scale 1 alone)
    if (rg.on && rg.filter != GJ_RESIZE_FILTER_BILINEAR &&
        (rg.filter != GJ_RESIZE_FILTER_ANTIALIAS || !rg.resize || (rg.scale_mask & ~1u) != 0 || rg.comp_mask != 0 ||
         (!rg_batch && (rg.frame.scale > 1 || rg.frame.w > GJ_RESIZE_AA_MAX_RATIO * job->gs.width || rg.frame.h > GJ_RESIZE_AA_MAX_RATIO * job->gs.height))))
        return -1;
    // (a chunk of progressive frames has no selection: every segment of every scan is decoded)
    // (without restart markers a selection is every segment of every scan: a batch of regions on such streams alone, gj_dec_job::batch_restartless)
    if (rg.on && (job->scale > 1 || job->flipped || (rg.select && (!rg.d_sel || !rg.h_sel_count || (g.restart_interval <= 0 && !(rg_batch && job->batch_restartless)))) ||
                  (rg_batch ? (g.fb.sizes == nullptr || (job->prog != nullptr ? rg.select != 0 : !rg.select) || job->channel_remap) : (g.fb.sizes != nullptr || job->batch.count > 1 || (rg.select && !rg.d_sel_count)))))
        return -1;
    // (frames of different image sizes, gj_frame_strides::geoms: a batch of crop-and-resize frames alone -- the selection, the sub-sequence decoder in
    // plane mode and the region IDCT kernels are the stages that read a frame's own geometry --, the same records for g and gs, one per frame of the launch)
    if ((g.fb.geoms != nullptr || job->batch.d_geoms != nullptr) &&
        (!rg_batch || !rg.resize || job->tokens || g.fb.geoms != job->batch.d_geoms || job->gs.fb.geoms != g.fb.geoms || job->tune.dec_sub))
        return -1;
    // (... with headers of their own, gj_batch::own_headers: inside such a batch alone -- the header records lie in the frames' geometry records)
    if (job->batch.own_headers && g.fb.geoms == nullptr) return -1;
    // (a progressive frame, gj_dec_job::prog: through the coefficient planes -- its own entropy stage, then the plane route's IDCT side --, a single
    // frame, or a chunk of frames with its per-frame records, which the check of every batch above has passed)
    if (job->prog != nullptr && ((job->prog->d_frames != nullptr) != (g.fb.sizes != nullptr) || job->tokens || job->scan.valid || rg.select || job->prog->levels < 0 ||
                                 job->prog->levels > GJ_PROG_MAX_SCANS))
        return -1;
    gj_hip_note_reset();
    if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[0], st));
    if (job->prog != nullptr) {
        gj_launch_huffman_prog(job, st);
        gj_debug_stage(job->tune.debug_sync != 0, st, "entropy decoder (progressive)");
        if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[1], st));
        gj_launch_idct(job, st, nullptr, ev);
        if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[3], st));
        return (hipGetLastError() == hipSuccess && !gj_hip_noted()) ? 0 : -1;
    }
    bool par = job->d_huff_tab2 != nullptr && job->seg_count > 0;
    if (job->tune.dec_serial) par = false; // the lane-per-segment kernel (A/B measurements, tests)
    const bool fast_ok = par && !job->tune.dec_careful && job->d_overflow != nullptr; // kernels that take whole segments into LDS are allowed
    // interleaved scans with many short segments: one lane per segment (k_huffman_decode_seq); the host vouches for the longest segment
    // (this stream's, or the previous frame's on the speculative path, where `d_overflow` is checked afterwards)
    // (a batch of frames: its segments are in flight together; only the token mode of the lane-per-segment decoder -- the ring kernel -- knows the frame dimension)
    const bool batch = g.fb.sizes != nullptr;
    const uint64_t segs_in_flight = (uint64_t)job->seg_count * (batch && g.fb.frames > 1 ? g.fb.frames : 1u);
    bool seq = fast_ok && job->tune.dec_seq != 2 &&
               (job->tune.dec_seq == 1 || (g.interleaved && job->max_seg_len != 0 && job->max_seg_len <= 1024u && segs_in_flight >= 16384u));
    // token mode: the entropy decoder hands the non-zero coefficients to the fused IDCT as a dense token array plus one
    // record per block instead of through the coefficient planes: k_huffman_decode_tok for non-interleaved scans (every segment has to
    // fit its LDS stage), the lane-per-segment kernel for interleaved ones
    // (a reduced-size decode, gj_dec_job::scale: token mode where the token-fed reduced-size kernel exists -- not for the interleaved 4:2:2 scan)
    const bool tok_wanted = fast_ok && job->tokens && job->use_fused && job->d_tok && job->d_blkrec && gj_hip_decode_wants_tokens(&g, job->jpeg_size, &job->tune) &&
                            (job->scale <= 1 || gj_idct_tok_scaled_for(g)) && (!job->region.on || gj_idct_tok_scaled_for(g)); // (region: the same configuration)
    const bool tok_sub = tok_wanted && !g.interleaved && !seq && job->max_seg_len != 0 && job->max_seg_len + 12u <= (uint32_t)GJ_TOK_CAP_U;
    const bool tok_seq = tok_wanted && seq;
    gj_idct_tok_t idct_tok = (tok_sub || tok_seq) ? gj_idct_tok_for(g) : nullptr;
    const bool tokens = idct_tok != nullptr;
    if (batch && !tokens) seq = false; // (planes: the sub-sequence decoder)
    // Both entropy decoders store only non-zero coefficients. The sub-sequence kernel zero-fills the blocks of the segments it
    // decodes itself; clear_coefs asks for a full clear first (segments missing from the table, lane-per-segment kernel).
    if (tokens) {
        if (job->clear_coefs) GJ_HIP_CHECK(hipMemsetAsync(job->d_blkrec, 0, (size_t)g.block_count * sizeof(uint2), st));
    } else if (job->clear_coefs || !par) {
        GJ_HIP_CHECK(hipMemsetAsync(job->d_coefs, 0, g.data_size * sizeof(int16_t), st));
    }
    // a marker scan whose table launch was left to us (gj_scan_deferred): the token decoder reads the scan's records itself, everything else needs the table
    const bool takes_par = !(tokens && tok_sub) && !seq && par;
    // (a selection reads the table: its launch is not folded into the entropy decoder)
    const bool folded = job->scan.valid && !rg.select && ((tokens && tok_sub && gj_tok_folds_table(job)) || (takes_par && gj_par_folds_table(job)));
    if (job->scan.valid && !folded) gj_launch_marker_table_deferred(job, st);
    if (job->scan.valid && job->scan.folded) *job->scan.folded = folded ? 1 : 0;
    // region call with a selection: the entropy decoder gets the compacted table -- as many entries as the geometry says touch the cover (the plan),
    // bounded by what k_segment_select found in this stream's table
    gj_dec_job sel;
    if (rg.select) {
        if (rg_batch) gj_launch_segment_select_batch(job, st);
        else gj_launch_segment_select(job, st);
        sel = *job;
        const uint32_t stride = (uint32_t)g.segment_count + GJ_MAX_COMP;
        sel.d_seg_pos = rg.d_sel;
        sel.d_seg_len = rg.d_sel + stride;
        sel.d_seg_index = rg.d_sel + 2 * stride;
        sel.d_seg_count = rg_batch ? nullptr : rg.d_sel_count; // (a batch: every frame's compacted table is padded to the plan's entries)
        sel.seg_count = 0;
        for (int c = 0; c < g.scan_count && c < GJ_MAX_COMP; c++) sel.seg_count += rg.sel_count[c];
        sel.scan.valid = 0;
        job = &sel;
    }
    if (tokens && tok_sub) gj_launch_huffman_tok(job, st);
    else if (seq) gj_launch_huffman_seq(job, st, tokens);
    else if (par) gj_launch_huffman_par(job, st);
    else gj_launch_huffman_serial(job, st);
    gj_debug_stage(job->tune.debug_sync != 0, st, "entropy decoder");
    if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[1], st));
    gj_launch_idct(job, st, idct_tok, ev);
    if (ev) GJ_HIP_CHECK(hipEventRecord((hipEvent_t)ev[3], st));
    return (hipGetLastError() == hipSuccess && !gj_hip_noted()) ? 0 : -1;
}
