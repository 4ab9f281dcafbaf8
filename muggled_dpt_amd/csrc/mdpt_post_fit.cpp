// libmdpt: the mdpt_post_* entry points that fit maps to other data (see mdpt_post.cpp): tiles, true-depth alignment, guided upsampling, video.
#include "mdpt_post_checks.h"

extern "C" {

// ---- tiled high-resolution inference (the fit the reference's results_explainer.md describes under "Fitting to (more) known data")
MDPT_SAME_RECORD(mdpt_tile, PostTile, 32, map, h, w, x1, y1, x2, y2);

// the host table: sizes positive, boxes inside the H x W photo (H = 0: boxes only ordered and non-negative), maps aligned to their element;
// *max_chunks = the fit chunks of the largest map
static int check_tiles(const mdpt_tile* tiles, int32_t T, int32_t map_dtype, int32_t H, int32_t W, size_t* max_chunks) {
    if (!tiles) return fail(MDPT_E_INVALID, "null argument");
    if (T <= 0) return fail(MDPT_E_INVALID, "bad tile count %d", T);
    size_t most = 0;
    for (int t = 0; t < T; ++t) {
        const mdpt_tile& q = tiles[t];
        if (!q.map || !aligned_to_element(q.map, map_dtype)) return fail(MDPT_E_INVALID, "null or misaligned map (tile %d)", t);
        if (q.h <= 0 || q.w <= 0) return fail(MDPT_E_INVALID, "bad map size %dx%d (tile %d)", q.h, q.w, t);
        if (!(0 <= q.x1 && q.x1 < q.x2 && 0 <= q.y1 && q.y1 < q.y2) || (H > 0 && (q.x2 > W || q.y2 > H)))
            return fail(MDPT_E_INVALID, "box (%d, %d)-(%d, %d) of tile %d is empty or outside the %dx%d photo", q.x1, q.y1, q.x2, q.y2, t, H, W);
        most = std::max(most, tile_fit_chunks((size_t)q.h * q.w));
    }
    if (most >= ((size_t)1 << 24)) return fail(MDPT_E_INVALID, "a tile map is too large (fewer than 2^24 chunks of %d samples)", MDPT_TILE_FIT_CHUNK);
    *max_chunks = most;
    return 0;
}

int mdpt_post_tile_scratch_bytes(const mdpt_tile* tiles_host, int32_t T, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    size_t max_chunks;
    CHK(check_tiles(tiles_host, T, MDPT_DTYPE_BF16, 0, 0, &max_chunks));
    *bytes = (size_t)T * max_chunks * 6 * sizeof(double);
    return 0;
}

int mdpt_post_tile_fit(const mdpt_tile* tiles_host, const void* tiles_dev, int32_t T, int32_t map_dtype, const void* guide, int32_t guide_dtype,
                       int32_t guide_h, int32_t guide_w, int32_t H, int32_t W, void* fit_f64, void* sums_f64, void* scratch, size_t scratch_bytes,
                       void* stream) {
    if (!tiles_dev || !guide || !fit_f64 || !sums_f64 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(map_dtype) || !tensor_dtype_ok(guide_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d / %d", map_dtype, guide_dtype);
    if (H <= 0 || W <= 0 || guide_h <= 0 || guide_w <= 0) return fail(MDPT_E_INVALID, "bad size: photo %dx%d, guide %dx%d", H, W, guide_h, guide_w);
    if (T > 65535) return fail(MDPT_E_INVALID, "%d tiles: the fit takes at most 65535 per call", T);
    size_t max_chunks;
    CHK(check_tiles(tiles_host, T, map_dtype, H, W, &max_chunks));
    if ((((uintptr_t)tiles_dev | (uintptr_t)fit_f64 | (uintptr_t)sums_f64 | (uintptr_t)scratch) & 7) != 0 ||
        !aligned_to_element(guide, guide_dtype))
        return fail(MDPT_E_INVALID, "misaligned pointer (the table and the fp64 buffers need 8 bytes, the guide its element)");
    CHK(check_scratch("tile", scratch_bytes, (size_t)T * max_chunks * 6 * sizeof(double), "mdpt_post_tile_scratch_bytes"));
    CHK(mdpt_launch_post_tile_fit((const PostTile*)tiles_dev, T, (int)max_chunks, map_dtype, guide, guide_dtype, guide_h, guide_w, H, W, (double*)scratch,
                                  (double*)sums_f64, (double*)fit_f64, (hipStream_t)stream));
    return 0;
}

int mdpt_post_tile_blend(const mdpt_tile* tiles_host, const void* tiles_dev, int32_t T, int32_t map_dtype, int32_t H, int32_t W, const void* fit_f64,
                         const void* sums_f64, double feather, void* out_f32, void* stream) {
    if (!tiles_dev || !out_f32) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(map_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", map_dtype);
    if (H <= 0 || W <= 0) return fail(MDPT_E_INVALID, "bad photo size %dx%d", H, W);
    if (!(feather >= 0.0) || feather > 1e300) return fail(MDPT_E_INVALID, "the feather width must be finite and >= 0, got %g", feather);
    // 64 x 16 pixels per workgroup, one grid axis: fewer than 2^24 workgroups of 256 threads (about 17 gigapixels)
    if ((((size_t)W + 63) / 64) * (((size_t)H + 15) / 16) >= ((size_t)1 << 24)) return fail(MDPT_E_INVALID, "a photo of %dx%d is too large for one blend", H, W);
    size_t max_chunks;
    CHK(check_tiles(tiles_host, T, map_dtype, H, W, &max_chunks));
    if ((((uintptr_t)tiles_dev | (uintptr_t)fit_f64 | (uintptr_t)sums_f64) & 7) != 0 || ((uintptr_t)out_f32 & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table and the fp64 buffers need 8 bytes, the output 4)");
    CHK(mdpt_launch_post_tile_blend((const PostTile*)tiles_dev, T, map_dtype, H, W, (const double*)fit_f64, (const double*)sums_f64, feather,
                                    (float*)out_f32, (hipStream_t)stream));
    return 0;
}

// ---- true depth from ground truth (results_explainer.md "True depth from DPT result" / "Fitting to (more) known data")
MDPT_SAME_RECORD(mdpt_depth_pair, AlignPair, 40, pred, ph, pw, truth, valid, H, W);
static_assert(MDPT_ALIGN_NUM_METRICS == ALIGN_METRIC_SUMS, "the metrics of a pair are its partial sums solved in place");

// the host table: sizes positive, H W < 2^31, predictions aligned to their element, truth (need_truth) non-null and 4-byte aligned;
// *max_chunks = the chunks of the largest truth
static int check_pairs(const mdpt_depth_pair* pairs, int32_t P, int32_t pred_dtype, bool need_truth, size_t* max_chunks) {
    if (!pairs) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_count("pair", "", P));
    size_t most = 0;
    for (int p = 0; p < P; ++p) {
        const mdpt_depth_pair& q = pairs[p];
        if (!q.pred || !aligned_to_element(q.pred, pred_dtype)) return fail(MDPT_E_INVALID, "null or misaligned prediction (pair %d)", p);
        if (q.ph <= 0 || q.pw <= 0 || q.H <= 0 || q.W <= 0) return fail(MDPT_E_INVALID, "bad size: prediction %dx%d, truth %dx%d (pair %d)", q.ph, q.pw, q.H, q.W, p);
        CHK(check_below_2_31("truth", q.H, q.W, "", p));
        if (need_truth && (!q.truth || ((uintptr_t)q.truth & 3) != 0)) return fail(MDPT_E_INVALID, "null or misaligned truth (pair %d)", p);
        most = std::max(most, tile_fit_chunks((size_t)q.H * q.W));
    }
    *max_chunks = most;
    return 0;
}

static int check_align_common(int32_t pred_dtype, int32_t space, double tmin, double tmax) {
    if (!tensor_dtype_ok(pred_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", pred_dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown alignment space %d", space);
    if (!(tmin <= tmax)) return fail(MDPT_E_INVALID, "the truth range [%g, %g] is empty or NaN", tmin, tmax);
    return 0;
}

int mdpt_post_align_scratch_bytes(const mdpt_depth_pair* pairs_host, int32_t P, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    size_t max_chunks;
    CHK(check_pairs(pairs_host, P, MDPT_DTYPE_BF16, false, &max_chunks));
    *bytes = align_scratch_bytes((size_t)P, max_chunks);
    return 0;
}

int mdpt_post_align_fit(const mdpt_depth_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t pred_dtype, int32_t space, int32_t method, double tmin,
                        double tmax, void* fit_f64, void* sums_f64, void* scratch, size_t scratch_bytes, void* stream) {
    if (!pairs_dev || !fit_f64 || !sums_f64 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_align_common(pred_dtype, space, tmin, tmax));
    if (method != MDPT_ALIGN_LSTSQ && method != MDPT_ALIGN_MEDIAN) return fail(MDPT_E_INVALID, "unknown alignment method %d", method);
    size_t max_chunks;
    CHK(check_pairs(pairs_host, P, pred_dtype, true, &max_chunks));
    if ((((uintptr_t)pairs_dev | (uintptr_t)fit_f64 | (uintptr_t)sums_f64 | (uintptr_t)scratch) & 7) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the fp64 buffers and the scratch need 8 bytes)");
    CHK(check_scratch("alignment", scratch_bytes, align_scratch_bytes((size_t)P, max_chunks), "mdpt_post_align_scratch_bytes"));
    unsigned* hist = (unsigned*)((double*)scratch + align_parts_doubles((size_t)P, max_chunks));
    CHK(mdpt_launch_post_align_fit((const AlignPair*)pairs_dev, P, (int)max_chunks, pred_dtype, space == MDPT_ALIGN_INVERSE, method == MDPT_ALIGN_MEDIAN, tmin,
                                   tmax, (double*)scratch, hist, hist + (size_t)P * ALIGN_HIST_WORDS, (double*)sums_f64, (double*)fit_f64,
                                   (hipStream_t)stream));
    return 0;
}

int mdpt_post_align_metrics(const mdpt_depth_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t pred_dtype, int32_t space, double tmin,
                            double tmax, const void* fit_f64, void* metrics_f64, void* scratch, size_t scratch_bytes, void* stream) {
    if (!pairs_dev || !metrics_f64 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_align_common(pred_dtype, space, tmin, tmax));
    size_t max_chunks;
    CHK(check_pairs(pairs_host, P, pred_dtype, true, &max_chunks));
    if ((((uintptr_t)pairs_dev | (uintptr_t)fit_f64 | (uintptr_t)metrics_f64 | (uintptr_t)scratch) & 7) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the fp64 buffers and the scratch need 8 bytes)");
    CHK(check_scratch("alignment", scratch_bytes, align_scratch_bytes((size_t)P, max_chunks), "mdpt_post_align_scratch_bytes"));
    CHK(mdpt_launch_post_align_metrics((const AlignPair*)pairs_dev, P, (int)max_chunks, pred_dtype, space == MDPT_ALIGN_INVERSE, tmin, tmax,
                                       (const double*)fit_f64, (double*)scratch, (double*)metrics_f64, (hipStream_t)stream));
    return 0;
}

int mdpt_post_align_apply(const mdpt_depth_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t pred_dtype, int32_t space, const void* fit_f64,
                          const int64_t* out_offsets_host, const void* out_offsets_dev, double dmin, double dmax, void* out_f32, void* stream) {
    if (!pairs_dev || !out_offsets_host || !out_offsets_dev || !out_f32) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_align_common(pred_dtype, space, 0.0, 0.0));
    if (dmin != dmin || dmax != dmax || dmin > dmax) return fail(MDPT_E_INVALID, "the clamp [%g, %g] is empty or NaN", dmin, dmax);
    size_t max_chunks;
    CHK(check_pairs(pairs_host, P, pred_dtype, false, &max_chunks));
    for (int p = 0; p < P; ++p)
        if (out_offsets_host[p] < 0) return fail(MDPT_E_INVALID, "negative output offset (pair %d)", p);
    if ((((uintptr_t)pairs_dev | (uintptr_t)fit_f64 | (uintptr_t)out_offsets_dev) & 7) != 0 || ((uintptr_t)out_f32 & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the fit and the offsets need 8 bytes, the output 4)");
    size_t max_pixels = 0;
    for (int p = 0; p < P; ++p) max_pixels = std::max(max_pixels, (size_t)pairs_host[p].H * pairs_host[p].W);
    CHK(mdpt_launch_post_align_apply((const AlignPair*)pairs_dev, P, max_pixels, pred_dtype, space == MDPT_ALIGN_INVERSE, (const double*)fit_f64,
                                     (const long long*)out_offsets_dev, dmin, dmax, (float*)out_f32, (hipStream_t)stream));
    return 0;
}

// ---- photo-guided upsampling (the fast guided filter with the photo as guide)
MDPT_SAME_RECORD(mdpt_guided_pair, GuidedPair, 56, map, h, w, photo, pitch, H, W, out, scratch_off);

// the host table's map sizes: positive, h w < 2^31; *bytes = the scratch of the P regions laid end to end
static int check_guided_sizes(const mdpt_guided_pair* pairs, int32_t P, size_t* bytes) {
    if (!bytes || !pairs) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_count("pair", "", P));
    size_t total = 0;
    for (int p = 0; p < P; ++p) {
        const mdpt_guided_pair& q = pairs[p];
        CHK(check_map_size(q.h, q.w, p));
        total += guided_pair_scratch_bytes((size_t)q.h, (size_t)q.w);
    }
    *bytes = total;
    return 0;
}

int mdpt_post_guided_scratch_bytes(const mdpt_guided_pair* pairs_host, int32_t P, size_t* bytes) { return check_guided_sizes(pairs_host, P, bytes); }

int mdpt_post_guided_upsample(const mdpt_guided_pair* pairs_host, const void* pairs_dev, int32_t P, int32_t map_dtype, int32_t radius, double eps,
                              void* scratch, size_t scratch_bytes, void* coeffs_f64, void* stream) {
    if (!pairs_host || !pairs_dev || !scratch) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(map_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", map_dtype);
    if (radius < 0 || radius > GUIDED_MAX_RADIUS) return fail(MDPT_E_INVALID, "radius %d: the window radius must be 0 .. %d cells", radius, GUIDED_MAX_RADIUS);
    if (!(eps > 0.0) || eps > 1e300) return fail(MDPT_E_INVALID, "eps must be finite and > 0, got %g", eps);
    size_t packed;
    CHK(check_guided_sizes(pairs_host, P, &packed));
    if ((((uintptr_t)pairs_dev | (uintptr_t)scratch | (uintptr_t)coeffs_f64) & 7) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the scratch and the coefficients need 8 bytes)");
    int max_h = 0, max_w = 0, max_H = 0, max_W = 0;
    ScratchRegions regions;
    for (int p = 0; p < P; ++p) {
        const mdpt_guided_pair& q = pairs_host[p];
        if (!q.map || !q.photo || !q.out) return fail(MDPT_E_INVALID, "null map, photo or output (pair %d)", p);
        if (!aligned_to_element(q.map, map_dtype) || ((uintptr_t)q.out & 3) != 0)
            return fail(MDPT_E_INVALID, "misaligned map or output (pair %d: the map needs its element, the output 4 bytes)", p);
        if (q.H < q.h || q.W < q.w)
            return fail(MDPT_E_INVALID, "the %dx%d photo of pair %d is smaller than its %dx%d map: guided upsampling only enlarges", q.H, q.W, p, q.h, q.w);
        CHK(check_below_2_31("photo", q.H, q.W, "", p));
        CHK(check_pitch(q.pitch, q.W, p));
        CHK(regions.add(p, q.scratch_off, guided_pair_scratch_bytes((size_t)q.h, (size_t)q.w), scratch_bytes, "given (mdpt_post_guided_scratch_bytes)"));
        max_h = q.h > max_h ? q.h : max_h, max_w = q.w > max_w ? q.w : max_w;
        max_H = q.H > max_H ? q.H : max_H, max_W = q.W > max_W ? q.W : max_W;
    }
    CHK(regions.finish());
    CHK(mdpt_launch_post_guided((const GuidedPair*)pairs_dev, P, map_dtype, radius, eps, max_h, max_w, max_H, max_W, (char*)scratch, (double*)coeffs_f64,
                                (hipStream_t)stream));
    return 0;
}

// ---- temporally stable video depth (frame-to-frame fit, temporal filter, carried display range; not in the reference)
static int check_video_sizes(int32_t T, int32_t h, int32_t w) {
    CHK(check_count("frame", "", T));
    if (h <= 0 || w <= 0 || (size_t)h * w >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "bad frame size %dx%d (h w < 2^31)", h, w);
    return 0;
}

// the display's scratch: the frames' and the carried ranges' partials, the resized fp32 frames (resize only), the uint8 frames - in that order
static size_t video_display_scratch_bytes(size_t T, size_t out_px, bool resize) {
    return 2 * T * MDPT_POST_SEG_PARTS * 2 * sizeof(unsigned) + (resize ? T * out_px * sizeof(float) : 0) + T * out_px;
}

static int check_video_out(int32_t h, int32_t w, int32_t out_h, int32_t out_w, size_t* out_px) {
    if ((out_h == 0) != (out_w == 0) || out_h < 0 || out_w < 0) return fail(MDPT_E_INVALID, "bad display size %dx%d (0x0: the frames' own)", out_h, out_w);
    *out_px = out_h ? (size_t)out_h * out_w : (size_t)h * w;
    if (*out_px > (size_t)INT32_MAX) return fail(MDPT_E_INVALID, "a display frame of %dx%d is too large (fewer than 2^31 pixels)", out_h, out_w);
    return 0;
}

int mdpt_post_video_scratch_bytes(int32_t T, int32_t h, int32_t w, int32_t out_h, int32_t out_w, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_video_sizes(T, h, w));
    size_t out_px;
    CHK(check_video_out(h, w, out_h, out_w, &out_px));
    const size_t fit = video_fit_scratch_doubles((size_t)T, (size_t)h * w) * sizeof(double);
    const size_t display = video_display_scratch_bytes((size_t)T, out_px, out_h != 0);
    *bytes = ((fit > display ? fit : display) + 7) & ~(size_t)7;
    return 0;
}

int mdpt_post_video_fit(const void* frames, int32_t dtype, int32_t T, int32_t h, int32_t w, const void* prev_frame, const void* ab_in_f64, const void* started_i32,
                        int32_t rounds, double c, double cut_corr, void* table_f64, void* ab_out_f64, void* sums_f64, void* scratch, size_t scratch_bytes,
                        void* stream) {
    if (!frames || !prev_frame || !ab_in_f64 || !started_i32 || !table_f64 || !ab_out_f64 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    CHK(check_video_sizes(T, h, w));
    if (rounds < 0 || rounds > 8) return fail(MDPT_E_INVALID, "rounds must be 0 .. 8, got %d", rounds);
    if (!(c > 0.0) || c > 1e150) return fail(MDPT_E_INVALID, "c must be finite and > 0, got %g", c);
    if (!(cut_corr >= 0.0 && cut_corr <= 1.0)) return fail(MDPT_E_INVALID, "cut_corr must be in [0, 1], got %g", cut_corr);
    if ((((uintptr_t)ab_in_f64 | (uintptr_t)table_f64 | (uintptr_t)ab_out_f64 | (uintptr_t)sums_f64 | (uintptr_t)scratch) & 7) != 0 ||
        ((uintptr_t)started_i32 & 3) != 0 || !aligned_to_element(frames, dtype) || !aligned_to_element(prev_frame, dtype))
        return fail(MDPT_E_INVALID, "misaligned pointer (the fp64 buffers and the scratch need 8 bytes, the flag 4, the frames their element)");
    CHK(check_scratch("video", scratch_bytes, video_fit_scratch_doubles((size_t)T, (size_t)h * w) * sizeof(double), "mdpt_post_video_scratch_bytes"));
    CHK(mdpt_launch_post_video_fit(frames, dtype, T, (size_t)h * w, prev_frame, (const double*)ab_in_f64, (const int*)started_i32, rounds, c, cut_corr,
                                   (double*)table_f64, (double*)ab_out_f64, (double*)sums_f64, (double*)scratch, (hipStream_t)stream));
    return 0;
}

int mdpt_post_video_filter(const void* frames, int32_t dtype, int32_t T, int32_t h, int32_t w, const void* table_f64, const void* prev_out_f32, double alpha,
                           double tau, void* out_f32, void* stream) {
    if (!frames || !table_f64 || !prev_out_f32 || !out_f32) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    CHK(check_video_sizes(T, h, w));
    if (!(alpha > 0.0 && alpha <= 1.0)) return fail(MDPT_E_INVALID, "alpha must be in (0, 1], got %g", alpha);
    if (!(tau >= 0.0) || tau > 1e150) return fail(MDPT_E_INVALID, "tau must be finite and >= 0, got %g", tau);
    if (((uintptr_t)table_f64 & 7) != 0 || (((uintptr_t)prev_out_f32 | (uintptr_t)out_f32) & 3) != 0 || !aligned_to_element(frames, dtype))
        return fail(MDPT_E_INVALID, "misaligned pointer (the table needs 8 bytes, the fp32 buffers 4, the frames their element)");
    if (out_f32 == frames || out_f32 == prev_out_f32) return fail(MDPT_E_INVALID, "the output must be a buffer of its own");
    CHK(mdpt_launch_post_video_filter(frames, dtype, T, (size_t)h * w, (const double*)table_f64, (const float*)prev_out_f32, alpha, tau, (float*)out_f32,
                                      (hipStream_t)stream));
    return 0;
}

int mdpt_post_video_display(const void* stable_f32, int32_t T, int32_t h, int32_t w, const void* table_f64, const void* range_in_f32, const void* started_i32,
                            int32_t out_h, int32_t out_w, int32_t reverse, const void* cmap_bgr, double range_rate, void* out_bgr, void* ranges_f32,
                            void* range_out_f32, void* scratch, size_t scratch_bytes, void* stream) {
    if (!stable_f32 || !table_f64 || !range_in_f32 || !started_i32 || !out_bgr || !range_out_f32 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_video_sizes(T, h, w));
    size_t out_px;
    CHK(check_video_out(h, w, out_h, out_w, &out_px));
    if (!(range_rate > 0.0 && range_rate <= 1.0)) return fail(MDPT_E_INVALID, "range_rate must be in (0, 1], got %g", range_rate);
    if (((uintptr_t)table_f64 & 7) != 0 ||
        (((uintptr_t)stable_f32 | (uintptr_t)range_in_f32 | (uintptr_t)started_i32 | (uintptr_t)ranges_f32 | (uintptr_t)range_out_f32 | (uintptr_t)scratch) & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table needs 8 bytes, the fp32 buffers, the flag and the scratch 4)");
    const bool resize = out_h != 0;
    CHK(check_scratch("video", scratch_bytes, video_display_scratch_bytes((size_t)T, out_px, resize), "mdpt_post_video_scratch_bytes"));
    unsigned* parts = (unsigned*)scratch;
    unsigned* rparts = parts + (size_t)T * MDPT_POST_SEG_PARTS * 2;
    float* scaled = resize ? (float*)(rparts + (size_t)T * MDPT_POST_SEG_PARTS * 2) : nullptr;
    unsigned char* u8 = (unsigned char*)(rparts + (size_t)T * MDPT_POST_SEG_PARTS * 2) + (resize ? (size_t)T * out_px * sizeof(float) : 0);
    CHK(mdpt_launch_post_video_display((const float*)stable_f32, T, h, w, resize ? out_h : h, resize ? out_w : w, (const double*)table_f64,
                                       (const float*)range_in_f32, (const int*)started_i32, range_rate, reverse != 0, (const unsigned char*)cmap_bgr, scaled, parts,
                                       rparts, u8, (unsigned char*)out_bgr, (float*)ranges_f32, (float*)range_out_f32, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
