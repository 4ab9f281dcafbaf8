// libmdpt: the depth post-processing entry points of include/mdpt.h (mdpt_post_*). None of them takes a handle, a plan or a workspace: argument checks
// (the shared ones: mdpt_post_checks.h), the image tables of the per-image kernels, and one launcher call (postprocess.hip) each. Here: min/max, scale and normalize,
// the display tails, masking, block-norm tiles; mdpt_post_geometry.cpp: mesh, render, hole filling; _fit.cpp: tiles, alignment, guided, video; _photo.cpp: the rest.
#include "mdpt_post_checks.h"

extern "C" {

// ---- depth post-processing (demo_helpers/postprocess.py, run_3dviewer.py:576-590)
int mdpt_post_minmax(const void* in_f32, size_t count, void* minmax_out, void* scratch8, void* stream) {
    if (!in_f32 || !minmax_out || !scratch8 || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    CHK(mdpt_launch_post_minmax((const float*)in_f32, count, (float*)minmax_out, (unsigned*)scratch8, (hipStream_t)stream));
    return 0;
}

int mdpt_post_scale_prediction(const void* in_bhw_f32, int32_t B, int32_t in_h, int32_t in_w, void* out_bhw_f32, int32_t out_h,
                               int32_t out_w, void* minmax_out, void* scratch8, void* stream) {
    if (!in_bhw_f32 || !out_bhw_f32 || (minmax_out && !scratch8)) return fail(MDPT_E_INVALID, "null argument");
    if (B <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return fail(MDPT_E_INVALID, "bad size %dx%dx%d -> %dx%d", B, in_h, in_w, out_h, out_w);
    CHK(mdpt_launch_post_scale((const float*)in_bhw_f32, (float*)out_bhw_f32, B, in_h, in_w, out_h, out_w, (float*)minmax_out,
                               (unsigned*)scratch8, (hipStream_t)stream));
    return 0;
}

int mdpt_post_normalize(const void* in_f32, size_t count, const void* minmax, void* out, int32_t mode, int32_t lossy, void* stream) {
    if (!in_f32 || !out || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    if (mode < MDPT_POST_F32 || mode > MDPT_POST_U24) return fail(MDPT_E_INVALID, "unknown post-processing mode %d", mode);
    CHK(mdpt_launch_post_normalize((const float*)in_f32, (const float*)minmax, out, count, mode, lossy, (hipStream_t)stream));
    return 0;
}

// ---- per-image display tail (run_video.py:348-361 per frame, over a batch; demo_helpers/postprocess.py:107-145, toadui/colormaps.py:237-259)

int mdpt_post_minmax_seg(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t in_h, int32_t in_w, void* out_bhw_f32, int32_t out_h, int32_t out_w,
                         void* parts, void* hist_clear, void* stream) {
    if (!in_bhw || !parts) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    if (B <= 0 || B > 65535 || in_h <= 0 || in_w <= 0 || (out_bhw_f32 && (out_h <= 0 || out_w <= 0)))
        return fail(MDPT_E_INVALID, "bad size %dx%dx%d -> %dx%d", B, in_h, in_w, out_h, out_w);
    const PostRunTable t = uniform_table(in_bhw, B, in_h, in_w, out_bhw_f32 ? out_h : in_h, out_bhw_f32 ? out_w : in_w);
    CHK(mdpt_launch_post_seg_minmax(t, in_dtype, (float*)out_bhw_f32, (unsigned*)parts, (unsigned*)hist_clear, (hipStream_t)stream));
    return 0;
}

int mdpt_post_u8_hist_seg(const void* in_bhw, int32_t in_dtype, int32_t B, size_t count, const void* parts, int32_t reverse, void* out_u8, void* hist,
                          void* stream) {
    if (!in_bhw || !parts || !out_u8 || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_batch(B));
    int ih, iw;
    if (!count_as_hw(count, ih, iw)) return fail(MDPT_E_INVALID, "bad image size %zu", count);
    CHK(mdpt_launch_post_seg_u8(uniform_table(in_bhw, B, ih, iw, ih, iw), in_dtype, (const unsigned*)parts, reverse != 0, (unsigned char*)out_u8,
                                (unsigned*)hist, (hipStream_t)stream));
    return 0;
}

int mdpt_post_histogram(const void* in_u8, int32_t B, size_t count, void* hist, void* stream) {
    if (!in_u8 || !hist || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    CHK(check_batch(B));
    CHK(mdpt_launch_post_hist((const unsigned char*)in_u8, B, count, (unsigned*)hist, (hipStream_t)stream));
    return 0;
}

int mdpt_post_equalize_lut(const void* hist, int32_t B, const void* bin_of_value, int32_t min_value, int32_t max_value, void* lut_out, void* stream) {
    if (!hist || !lut_out) return fail(MDPT_E_INVALID, "null argument");
    if (B <= 0) return fail(MDPT_E_INVALID, "bad batch %d", B);
    if (bin_of_value && (min_value < 0 || max_value > 255 || max_value <= min_value))
        return fail(MDPT_E_INVALID, "bad equalization range [%d, %d]", min_value, max_value);
    CHK(mdpt_launch_post_eq_lut((const unsigned*)hist, B, (const int*)bin_of_value, min_value, max_value, (unsigned char*)lut_out, (hipStream_t)stream));
    return 0;
}

int mdpt_post_colorize(const void* in_u8, int32_t B, size_t count, const void* eq_lut, const void* cmap_bgr, int32_t channels, void* out, void* stream) {
    if (!in_u8 || !out || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    CHK(check_batch(B));
    if (channels != 1 && channels != 3) return fail(MDPT_E_INVALID, "channels must be 1 or 3, got %d", channels);
    int ih, iw;
    if (!count_as_hw(count, ih, iw)) return fail(MDPT_E_INVALID, "bad image size %zu", count);
    CHK(mdpt_launch_post_colorize(uniform_table(in_u8, B, ih, iw, ih, iw), (const unsigned char*)eq_lut, (const unsigned char*)cmap_bgr, channels,
                                  (unsigned char*)out, (hipStream_t)stream));
    return 0;
}

// ---- still-image display tail (run_image.py:185-195, 323-343, 350-358) and the viewer's edge alpha (run_3dviewer.py:455-505, 576-593)
static PlaneMap plane_map(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                          const void* vparts) {
    return PlaneMap{in_bhw, in_dtype, B, H, W, (const unsigned*)parts, (const double*)coef, factor, (const double*)vparts};
}

int mdpt_post_display_prep(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t in_h, int32_t in_w, void* out_bhw, int32_t out_h, int32_t out_w,
                           void* parts, void* hist_clear, void* stream) {
    if (!in_bhw || !out_bhw || !parts) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_batch_hw(B, in_h, in_w));
    CHK(check_batch_hw(B, out_h, out_w));
    CHK(mdpt_launch_post_display_prep(in_bhw, in_dtype, B, in_h, in_w, out_bhw, out_h, out_w, (unsigned*)parts, (unsigned*)hist_clear, (hipStream_t)stream));
    return 0;
}

int mdpt_post_plane_fit(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* sample_xy, int32_t num_samples,
                        int32_t xy_per_image, void* coef_out, void* stream) {
    if (!in_bhw || !sample_xy || !coef_out) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_batch_hw(B, H, W));
    if (num_samples <= 0) return fail(MDPT_E_INVALID, "bad sample count %d", num_samples);
    CHK(mdpt_launch_post_plane_fit(in_bhw, in_dtype, B, H, W, (const unsigned*)parts, (const int*)sample_xy, num_samples,
                                   xy_per_image ? (size_t)num_samples * 2 : 0, (double*)coef_out, (hipStream_t)stream));
    return 0;
}

int mdpt_post_plane_eval(const void* coef, int32_t B, int32_t H, int32_t W, void* out_f32, void* stream) {
    if (!coef || !out_f32) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_batch_hw(B, H, W));
    CHK(mdpt_launch_post_plane_eval((const double*)coef, B, H, W, (float*)out_f32, (hipStream_t)stream));
    return 0;
}

int mdpt_post_plane_minmax(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                           void* vparts, void* stream) {
    if (!in_bhw || !parts || !coef || !vparts) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_batch_hw(B, H, W));
    CHK(mdpt_launch_post_plane_minmax(plane_map(in_bhw, in_dtype, B, H, W, parts, coef, factor, nullptr), (double*)vparts, (hipStream_t)stream));
    return 0;
}

int mdpt_post_threshold(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                        const void* vparts, double thresh_min, double thresh_max, int32_t mode, int32_t reverse, void* out, void* hist, void* stream) {
    if (!in_bhw || !parts || !coef || !vparts || !out) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_batch_hw(B, H, W));
    if (mode != MDPT_POST_F32 && mode != MDPT_POST_U8) return fail(MDPT_E_INVALID, "threshold mode must be MDPT_POST_F32 or MDPT_POST_U8, got %d", mode);
    if (mode == MDPT_POST_U8 && reverse) return fail(MDPT_E_INVALID, "the uint8 threshold pass does not reverse (255 - x follows the equalization)");
    if (!(thresh_min <= thresh_max)) return fail(MDPT_E_INVALID, "threshold out of order: [%g, %g]", thresh_min, thresh_max);
    const double delta = thresh_max - thresh_min > 0.001 ? thresh_max - thresh_min : 0.001;  // run_image.py:329
    CHK(mdpt_launch_post_threshold(plane_map(in_bhw, in_dtype, B, H, W, parts, coef, factor, vparts), thresh_min, delta, mode, reverse != 0, out,
                                   mode == MDPT_POST_U8 ? (unsigned*)hist : nullptr, (hipStream_t)stream));
    return 0;
}

int mdpt_post_edge_mag(const void* in_bhw_f32, int32_t B, int32_t H, int32_t W, const void* parts, const float* blur_weights, int32_t blur_ksize,
                       void* mag_f32, void* mag_max, void* stream) {
    if (!in_bhw_f32 || !blur_weights || !mag_f32 || !mag_max) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_batch_hw(B, H, W));
    if (blur_ksize < 1 || blur_ksize > 15 || blur_ksize % 2 == 0) return fail(MDPT_E_INVALID, "blur kernel size must be odd, 1..15, got %d", blur_ksize);
    const int pad = blur_ksize / 2, min_side = pad + 1 > 2 ? pad + 1 : 2;  // reflect padding needs pad < side (blur pad, Sobel pad 1)
    if (H < min_side || W < min_side) return fail(MDPT_E_INVALID, "map %dx%d is too small for reflect padding (sides of at least %d)", H, W, min_side);
    CHK(mdpt_launch_post_edge_mag((const float*)in_bhw_f32, B, H, W, (const unsigned*)parts, blur_weights, blur_ksize, (float*)mag_f32, (unsigned*)mag_max,
                                  (hipStream_t)stream));
    return 0;
}

int mdpt_post_edge_mask(const void* mag_f32, const void* mag_max, int32_t B, size_t count, void* out_u8, void* stream) {
    if (!mag_f32 || !mag_max || !out_u8 || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    CHK(check_batch(B));
    CHK(mdpt_launch_post_edge_mask((const float*)mag_f32, (const unsigned*)mag_max, B, count, (unsigned char*)out_u8, (hipStream_t)stream));
    return 0;
}

int mdpt_post_pack_u24_alpha(const void* in_bhw_f32, int32_t B, size_t count, const void* parts, int32_t lossy, const void* mag_f32, const void* mag_max,
                             const void* mask_u8, int32_t mask_per_image, void* out_bgra, void* stream) {
    if (!in_bhw_f32 || !out_bgra || count == 0 || (mag_f32 && !mag_max)) return fail(MDPT_E_INVALID, "null argument / empty input");
    CHK(check_batch(B));
    if (mag_f32 && mask_u8) return fail(MDPT_E_INVALID, "alpha is either the edge mask or the caller's mask");
    CHK(mdpt_launch_post_pack_u24((const float*)in_bhw_f32, B, count, (const unsigned*)parts, lossy != 0, (const float*)mag_f32, (const unsigned*)mag_max,
                                  (const unsigned char*)mask_u8, mask_per_image ? count : 0, (unsigned char*)out_bgra, (hipStream_t)stream));
    return 0;
}

// ---- the same for images of different sizes: one run per image, MDPT_POST_RUNS images per launch; per-image buffers advance by the images before
// The image table of one launch: images [b0, b0 + MDPT_POST_RUNS) of B, one run each. Image i is in_hw[2i] x in_hw[2i+1] elements at in[i] - or,
// when `in` is NULL, at byte `off` of the packed uint8 buffer in_u8 - and its out_hw[2i] x out_hw[2i+1] output starts at element `off` of the
// packed output: `off` counts the output elements of the images before, across launches (0 before the first table, advanced here).
static PostRunTable image_table(const void* const* in, const void* in_u8, const int32_t* in_hw, const int32_t* out_hw, int b0, int B, size_t& off) {
    PostRunTable t{};
    t.n = B - b0 < MDPT_POST_RUNS ? B - b0 : MDPT_POST_RUNS;
    for (int r = 0; r < t.n; ++r) {
        const int i = b0 + r;
        t.run[r] = PostRun{in ? in[i] : (const unsigned char*)in_u8 + off, off, in_hw[2 * i], in_hw[2 * i + 1], out_hw[2 * i], out_hw[2 * i + 1], 1};
        off += (size_t)out_hw[2 * i] * out_hw[2 * i + 1];
    }
    return t;
}

int mdpt_post_minmax_images(const void* const* in, const int32_t* in_hw, int32_t in_dtype, int32_t B, void* out_f32, const int32_t* out_hw, void* parts,
                            void* hist_clear, void* stream) {
    if (!in || !in_hw || !parts || (out_f32 && !out_hw)) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_images(in, in_hw, B, "input"));
    if (out_f32) CHK(check_images(nullptr, out_hw, B, "output"));
    size_t off = 0;
    for (int b0 = 0; b0 < B; b0 += MDPT_POST_RUNS) {
        const PostRunTable t = image_table(in, nullptr, in_hw, out_f32 ? out_hw : in_hw, b0, B, off);
        CHK(mdpt_launch_post_seg_minmax(t, in_dtype, (float*)out_f32, (unsigned*)parts + (size_t)b0 * MDPT_POST_SEG_PARTS * 2,
                                        hist_clear ? (unsigned*)hist_clear + (size_t)b0 * 256 : nullptr, (hipStream_t)stream));
    }
    return 0;
}

int mdpt_post_u8_hist_images(const void* const* in, const int32_t* hw, int32_t in_dtype, int32_t B, const void* parts, int32_t reverse, void* out_u8,
                             void* hist, void* stream) {
    if (!in || !hw || !parts || !out_u8) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_images(in, hw, B, "input"));
    size_t off = 0;
    for (int b0 = 0; b0 < B; b0 += MDPT_POST_RUNS) {
        const PostRunTable t = image_table(in, nullptr, hw, hw, b0, B, off);
        CHK(mdpt_launch_post_seg_u8(t, in_dtype, (const unsigned*)parts + (size_t)b0 * MDPT_POST_SEG_PARTS * 2, reverse != 0, (unsigned char*)out_u8,
                                    hist ? (unsigned*)hist + (size_t)b0 * 256 : nullptr, (hipStream_t)stream));
    }
    return 0;
}

int mdpt_post_colorize_images(const void* in_u8, const int32_t* hw, int32_t B, const void* eq_lut, const void* cmap_bgr, int32_t channels, void* out,
                              void* stream) {
    if (!in_u8 || !hw || !out) return fail(MDPT_E_INVALID, "null argument");
    if (channels != 1 && channels != 3) return fail(MDPT_E_INVALID, "channels must be 1 or 3, got %d", channels);
    CHK(check_images(nullptr, hw, B, "input"));
    size_t off = 0;
    for (int b0 = 0; b0 < B; b0 += MDPT_POST_RUNS) {
        const PostRunTable t = image_table(nullptr, in_u8, hw, hw, b0, B, off);
        CHK(mdpt_launch_post_colorize(t, eq_lut ? (const unsigned char*)eq_lut + (size_t)b0 * 256 : nullptr, (const unsigned char*)cmap_bgr, channels,
                                      (unsigned char*)out, (hipStream_t)stream));
    }
    return 0;
}

// ---- depth masking (experiments/depth_masking.py:189-199, 314-332 display; :341-361 save)
static int check_mask_window(double thresh_min, double thresh_max) {
    if (!(0.0 <= thresh_min && thresh_min <= thresh_max && thresh_max <= 1.0))
        return fail(MDPT_E_INVALID, "threshold must be (min, max) with 0 <= min <= max <= 1, got [%g, %g]", thresh_min, thresh_max);
    return 0;
}

int mdpt_post_mask_display(const void* in_bhw, int32_t in_dtype, int32_t B, int32_t H, int32_t W, const void* parts, const void* coef, double factor,
                           const void* vparts, double thresh_min, double thresh_max, int32_t invert, const void* images_bgr, int32_t image_h, int32_t image_w,
                           void* mask_out, void* composite_out, void* stream) {
    if (!in_bhw || !parts || !coef || !vparts || !images_bgr || !mask_out || !composite_out) return fail(MDPT_E_INVALID, "null argument");
    if (!tensor_dtype_ok(in_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", in_dtype);
    CHK(check_batch_hw(B, H, W));
    CHK(check_batch_hw(B, image_h, image_w));
    CHK(check_mask_window(thresh_min, thresh_max));
    CHK(mdpt_launch_post_mask_display(plane_map(in_bhw, in_dtype, B, H, W, parts, coef, factor, vparts), thresh_min, thresh_max, invert != 0,
                                      (const unsigned char*)images_bgr, image_h, image_w, (unsigned char*)mask_out, (unsigned char*)composite_out,
                                      (hipStream_t)stream));
    return 0;
}

int mdpt_post_mask_cutout_images(const void* const* maps, const int32_t* map_hw, int32_t map_dtype, const void* const* parts, const void* const* coef,
                                 const void* const* vparts, double factor, const void* const* images, const int32_t* image_hw, const int64_t* out_offsets,
                                 int32_t B, double thresh_min, double thresh_max, int32_t invert, void* out_bgra, void* out_mask, void* stream) {
    if (!maps || !map_hw || !parts || !coef || !vparts || !images || !image_hw || !out_offsets || !out_bgra || !out_mask)
        return fail(MDPT_E_INVALID, "null argument");
    if (((uintptr_t)out_bgra & 3) != 0) return fail(MDPT_E_INVALID, "the BGRA output must be 4-byte aligned");
    if (!tensor_dtype_ok(map_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", map_dtype);
    CHK(check_mask_window(thresh_min, thresh_max));
    CHK(check_images(maps, map_hw, B, "map"));
    CHK(check_images(images, image_hw, B, "image"));
    for (int k = 0; k < B; ++k) {
        if (!parts[k] || !coef[k] || !vparts[k]) return fail(MDPT_E_INVALID, "null argument (statistics of image %d)", k);
        if (out_offsets[k] < 0) return fail(MDPT_E_INVALID, "bad output offset %lld (image %d)", (long long)out_offsets[k], k);
    }
    for (int b0 = 0; b0 < B; b0 += MDPT_MASK_IMAGES) {
        MaskTable t{};
        t.n = B - b0 < MDPT_MASK_IMAGES ? B - b0 : MDPT_MASK_IMAGES;
        t.dt = map_dtype;
        for (int r = 0; r < t.n; ++r) {
            const int k = b0 + r;
            t.im[r] = MaskImage{maps[k], (const unsigned*)parts[k], (const double*)coef[k], (const double*)vparts[k], (const unsigned char*)images[k],
                                (size_t)out_offsets[k], map_hw[2 * k], map_hw[2 * k + 1], image_hw[2 * k], image_hw[2 * k + 1]};
        }
        CHK(mdpt_launch_post_mask_cutout(t, factor, thresh_min, thresh_max, invert != 0, (unsigned char*)out_bgra, (unsigned char*)out_mask,
                                         (hipStream_t)stream));
    }
    return 0;
}

// ---- block norm tiles (experiments/block_norm_visualization.py:137-147, 207-233)
int mdpt_post_block_norm_tiles(const void* const* maps, const int32_t* map_hw, int32_t L, int32_t B, int32_t H, int32_t W, void* tiles_u8, void* minmax_f32,
                               void* stream) {
    if (!maps || !map_hw || !tiles_u8 || !minmax_f32) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_batch_hw(B, H, W));
    if (L <= 0 || (size_t)H * W > ((size_t)1 << 24)) return fail(MDPT_E_INVALID, "bad map count %d / tile size %dx%d", L, H, W);
    CHK(check_images(maps, map_hw, L, "map"));
    for (int l = 0; l < L; ++l)
        if (H % map_hw[2 * l] || W % map_hw[2 * l + 1])
            return fail(MDPT_E_INVALID, "map %d (%dx%d) does not divide the tile size %dx%d", l, map_hw[2 * l], map_hw[2 * l + 1], H, W);
    const int per_launch = 65535 / B < MDPT_POST_RUNS ? 65535 / B : MDPT_POST_RUNS;  // (maps per launch: a launch holds at most 65535 images)
    for (int l0 = 0; l0 < L; l0 += per_launch) {
        PostRunTable t{};
        t.n = L - l0 < per_launch ? L - l0 : per_launch;
        for (int r = 0; r < t.n; ++r)
            t.run[r] = PostRun{maps[l0 + r], (size_t)(l0 + r) * B * H * W, map_hw[2 * (l0 + r)], map_hw[2 * (l0 + r) + 1], H, W, B};
        CHK(mdpt_launch_post_block_norm_tiles(t, (unsigned char*)tiles_u8, (float*)minmax_f32 + (size_t)l0 * B * 2, (hipStream_t)stream));
    }
    return 0;
}

}  // extern "C"
