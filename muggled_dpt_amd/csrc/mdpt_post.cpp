// libmdpt: the depth post-processing entry points of include/mdpt.h (mdpt_post_*). None of them takes a handle, a plan or a workspace: argument
// checks, the image tables of the per-image kernels, and one launcher call (postprocess.hip) each.
#include "mdpt_internal.h"
#include <algorithm>
#include <utility>
#include <vector>

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

// a uint8 / map count as the ih x iw of one table entry (1 x count)
static bool count_as_hw(size_t count, int& ih, int& iw) {
    if (count == 0 || count > (size_t)INT32_MAX) return false;
    ih = 1;
    iw = (int)count;
    return true;
}

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
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
    int ih, iw;
    if (!count_as_hw(count, ih, iw)) return fail(MDPT_E_INVALID, "bad image size %zu", count);
    CHK(mdpt_launch_post_seg_u8(uniform_table(in_bhw, B, ih, iw, ih, iw), in_dtype, (const unsigned*)parts, reverse != 0, (unsigned char*)out_u8,
                                (unsigned*)hist, (hipStream_t)stream));
    return 0;
}

int mdpt_post_histogram(const void* in_u8, int32_t B, size_t count, void* hist, void* stream) {
    if (!in_u8 || !hist || count == 0) return fail(MDPT_E_INVALID, "null argument / empty input");
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
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
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
    if (channels != 1 && channels != 3) return fail(MDPT_E_INVALID, "channels must be 1 or 3, got %d", channels);
    int ih, iw;
    if (!count_as_hw(count, ih, iw)) return fail(MDPT_E_INVALID, "bad image size %zu", count);
    CHK(mdpt_launch_post_colorize(uniform_table(in_u8, B, ih, iw, ih, iw), (const unsigned char*)eq_lut, (const unsigned char*)cmap_bgr, channels,
                                  (unsigned char*)out, (hipStream_t)stream));
    return 0;
}

// ---- still-image display tail (run_image.py:185-195, 323-343, 350-358) and the viewer's edge alpha (run_3dviewer.py:455-505, 576-593)
static int check_batch_hw(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return fail(MDPT_E_INVALID, "bad size %dx%dx%d", B, H, W);
    return 0;
}

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
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
    CHK(mdpt_launch_post_edge_mask((const float*)mag_f32, (const unsigned*)mag_max, B, count, (unsigned char*)out_u8, (hipStream_t)stream));
    return 0;
}

int mdpt_post_pack_u24_alpha(const void* in_bhw_f32, int32_t B, size_t count, const void* parts, int32_t lossy, const void* mag_f32, const void* mag_max,
                             const void* mask_u8, int32_t mask_per_image, void* out_bgra, void* stream) {
    if (!in_bhw_f32 || !out_bgra || count == 0 || (mag_f32 && !mag_max)) return fail(MDPT_E_INVALID, "null argument / empty input");
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
    if (mag_f32 && mask_u8) return fail(MDPT_E_INVALID, "alpha is either the edge mask or the caller's mask");
    CHK(mdpt_launch_post_pack_u24((const float*)in_bhw_f32, B, count, (const unsigned*)parts, lossy != 0, (const float*)mag_f32, (const unsigned*)mag_max,
                                  (const unsigned char*)mask_u8, mask_per_image ? count : 0, (unsigned char*)out_bgra, (hipStream_t)stream));
    return 0;
}

// ---- the same for images of different sizes: one run per image, MDPT_POST_RUNS images per launch; per-image buffers advance by the images before
static int check_images(const void* const* in, const int32_t* hw, int32_t B, const char* what) {
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
    for (int i = 0; i < B; ++i) {
        if (in && !in[i]) return fail(MDPT_E_INVALID, "null argument (%s %d)", what, i);
        if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0) return fail(MDPT_E_INVALID, "bad %s size %dx%d (image %d)", what, hw[2 * i], hw[2 * i + 1], i);
    }
    return 0;
}

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

// ---- depth-to-mesh (3dviewer/mesh.js:184-200 grid, shaders.js:163-264 vertices, mesh.js:330-371 filtering, save_gltf.js:16-25 bounds)
static double js_round(double v) {  // Math.round: halves go toward +inf
    const double f = floor(v);
    return v - f >= 0.5 ? f + 1.0 : f;
}

int mdpt_post_mesh_grid(int32_t w, int32_t h, double target_faces, int32_t* nx, int32_t* ny) {
    if (!nx || !ny) return fail(MDPT_E_INVALID, "null argument");
    if (w <= 0 || h <= 0 || !(target_faces == target_faces)) return fail(MDPT_E_INVALID, "bad photo size %dx%d / face target %g", w, h, target_faces);
    const double t = target_faces > 2.0 ? target_faces : 2.0;
    const double tv = js_round(0.5 * t + sqrt(t));
    const double aspect = (double)w / (double)h;
    const double rx = sqrt(tv * aspect), ry = rx / aspect;
    const double fx = js_round(rx) > 2.0 ? js_round(rx) : 2.0, fy = js_round(ry) > 2.0 ? js_round(ry) : 2.0;
    if (fx * fy >= 2147483648.0) return fail(MDPT_E_INVALID, "a grid of %.0f x %.0f vertices is too large (the product must be below 2^31)", fx, fy);
    *nx = (int32_t)fx;
    *ny = (int32_t)fy;
    return 0;
}

// nx x ny vertices: sides of at least 2, fewer than 2^31 vertices and faces (counts are int32, face indices uint32)
static int check_mesh_grid(int32_t nx, int32_t ny) {
    if (nx < 2 || ny < 2) return fail(MDPT_E_INVALID, "a mesh grid needs sides of at least 2, got %dx%d", nx, ny);
    if ((size_t)nx * (size_t)ny >= ((size_t)1 << 31) || 2 * ((size_t)nx - 1) * ((size_t)ny - 1) >= ((size_t)1 << 31))
        return fail(MDPT_E_INVALID, "a grid of %dx%d vertices is too large (vertices and faces must each be fewer than 2^31)", nx, ny);
    return 0;
}

// the scratch of B images: the vertex map, the two lists of block counts, the ordered bounds - 4-byte words, in MeshJob's order
static size_t mesh_scratch_words(size_t B, int32_t nx, int32_t ny) {
    const size_t nv = (size_t)nx * ny, cells = ((size_t)nx - 1) * ((size_t)ny - 1);
    return B * (nv + mesh_blocks(nv) + mesh_blocks(cells) + 6);
}

int mdpt_post_mesh_scratch_bytes(int32_t B, int32_t nx, int32_t ny, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    if (B <= 0 || B > 65535) return fail(MDPT_E_INVALID, "bad batch %d", B);
    CHK(check_mesh_grid(nx, ny));
    *bytes = 4 * mesh_scratch_words((size_t)B, nx, ny);
    return 0;
}

int mdpt_post_mesh(const void* frames_bgra, int32_t B, int32_t H, int32_t W, int32_t nx, int32_t ny, const void* vertex_xy_f64, double a, double b,
                   double tan_half_fov, double x_scale, double y_scale, double edge_threshold, int32_t is_metric, int32_t mode, void* xyz_f32,
                   void* uv_f32, void* faces_u32, void* counts_i32, void* bounds_f32, void* scratch, size_t scratch_bytes, void* stream) {
    if (!frames_bgra || !xyz_f32 || !uv_f32 || !faces_u32 || !counts_i32 || !bounds_f32 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    if (((uintptr_t)frames_bgra & 3) != 0) return fail(MDPT_E_INVALID, "the BGRA frames must be 4-byte aligned");
    CHK(check_batch_hw(B, H, W));
    CHK(check_mesh_grid(nx, ny));
    if (mode != MDPT_MESH_TRIANGLES && mode != MDPT_MESH_POINTS) return fail(MDPT_E_INVALID, "unknown mesh mode %d", mode);
    if (!(edge_threshold == edge_threshold)) return fail(MDPT_E_INVALID, "the edge threshold is not a number");
    if (scratch_bytes < 4 * mesh_scratch_words((size_t)B, nx, ny))
        return fail(MDPT_E_INVALID, "mesh scratch of %zu bytes, %zu needed (mdpt_post_mesh_scratch_bytes)", scratch_bytes,
                    4 * mesh_scratch_words((size_t)B, nx, ny));
    const size_t nv = (size_t)nx * ny, cells = ((size_t)nx - 1) * ((size_t)ny - 1);
    MeshJob m{};
    m.frames = (const unsigned*)frames_bgra;
    m.vertex_xy = (const double*)vertex_xy_f64;
    m.B = B, m.H = H, m.W = W, m.nx = nx, m.ny = ny, m.is_metric = is_metric != 0, m.points = mode == MDPT_MESH_POINTS;
    m.x_step = 2.0 / (double)(nx - 1), m.y_step = 2.0 / (double)(ny - 1);  // mesh.js:198
    m.a = a, m.b = b, m.tan_half_fov = tan_half_fov, m.x_scale = x_scale, m.y_scale = y_scale;
    m.alpha_min = edge_threshold * 255.0;  // shaders.js:175
    m.vmap = (int*)scratch;
    m.vcnt = (unsigned*)scratch + (size_t)B * nv;
    m.fcnt = m.vcnt + (size_t)B * mesh_blocks(nv);
    m.bord = m.fcnt + (size_t)B * mesh_blocks(cells);
    CHK(mdpt_launch_post_mesh(m, (float*)xyz_f32, (float*)uv_f32, (unsigned*)faces_u32, (int*)counts_i32, (float*)bounds_f32, (hipStream_t)stream));
    return 0;
}

// ---- tiled high-resolution inference (the fit the reference's results_explainer.md describes under "Fitting to (more) known data")
static_assert(sizeof(mdpt_tile) == sizeof(PostTile) && sizeof(mdpt_tile) == 32, "mdpt_tile of include/mdpt.h is PostTile of mdpt_kernels.h");

static size_t dtype_bytes(int dt) { return dt == MDPT_DTYPE_F32 ? 4 : 2; }

// the host table: sizes positive, boxes inside the H x W photo (H = 0: boxes only ordered and non-negative), maps aligned to their element;
// *max_chunks = the fit chunks of the largest map
static int check_tiles(const mdpt_tile* tiles, int32_t T, int32_t map_dtype, int32_t H, int32_t W, size_t* max_chunks) {
    if (!tiles) return fail(MDPT_E_INVALID, "null argument");
    if (T <= 0) return fail(MDPT_E_INVALID, "bad tile count %d", T);
    size_t most = 0;
    for (int t = 0; t < T; ++t) {
        const mdpt_tile& q = tiles[t];
        if (!q.map || ((uintptr_t)q.map & (dtype_bytes(map_dtype) - 1)) != 0) return fail(MDPT_E_INVALID, "null or misaligned map (tile %d)", t);
        if (q.h <= 0 || q.w <= 0) return fail(MDPT_E_INVALID, "bad map size %dx%d (tile %d)", q.h, q.w, t);
        if (!(0 <= q.x1 && q.x1 < q.x2 && 0 <= q.y1 && q.y1 < q.y2) || (H > 0 && (q.x2 > W || q.y2 > H)))
            return fail(MDPT_E_INVALID, "box (%d, %d)-(%d, %d) of tile %d is empty or outside the %dx%d photo", q.x1, q.y1, q.x2, q.y2, t, H, W);
        const size_t c = tile_fit_chunks((size_t)q.h * q.w);
        most = c > most ? c : most;
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
        ((uintptr_t)guide & (dtype_bytes(guide_dtype) - 1)) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table and the fp64 buffers need 8 bytes, the guide its element)");
    const size_t need = (size_t)T * max_chunks * 6 * sizeof(double);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "tile scratch of %zu bytes, %zu needed (mdpt_post_tile_scratch_bytes)", scratch_bytes, need);
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
static_assert(sizeof(mdpt_depth_pair) == sizeof(AlignPair) && sizeof(mdpt_depth_pair) == 40, "mdpt_depth_pair of include/mdpt.h is AlignPair of mdpt_kernels.h");
static_assert(MDPT_ALIGN_NUM_METRICS == ALIGN_METRIC_SUMS, "the metrics of a pair are its partial sums solved in place");

// the host table: sizes positive, H W < 2^31, predictions aligned to their element, truth (need_truth) non-null and 4-byte aligned;
// *max_chunks = the chunks of the largest truth
static int check_pairs(const mdpt_depth_pair* pairs, int32_t P, int32_t pred_dtype, bool need_truth, size_t* max_chunks) {
    if (!pairs) return fail(MDPT_E_INVALID, "null argument");
    if (P <= 0 || P > 65535) return fail(MDPT_E_INVALID, "bad pair count %d (1 .. 65535 per call)", P);
    size_t most = 0;
    for (int p = 0; p < P; ++p) {
        const mdpt_depth_pair& q = pairs[p];
        if (!q.pred || ((uintptr_t)q.pred & (dtype_bytes(pred_dtype) - 1)) != 0) return fail(MDPT_E_INVALID, "null or misaligned prediction (pair %d)", p);
        if (q.ph <= 0 || q.pw <= 0 || q.H <= 0 || q.W <= 0) return fail(MDPT_E_INVALID, "bad size: prediction %dx%d, truth %dx%d (pair %d)", q.ph, q.pw, q.H, q.W, p);
        if ((size_t)q.H * q.W >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "a truth of %dx%d is too large (H W < 2^31, pair %d)", q.H, q.W, p);
        if (need_truth && (!q.truth || ((uintptr_t)q.truth & 3) != 0)) return fail(MDPT_E_INVALID, "null or misaligned truth (pair %d)", p);
        const size_t c = tile_fit_chunks((size_t)q.H * q.W);
        most = c > most ? c : most;
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
    const size_t need = align_scratch_bytes((size_t)P, max_chunks);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "alignment scratch of %zu bytes, %zu needed (mdpt_post_align_scratch_bytes)", scratch_bytes, need);
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
    const size_t need = align_scratch_bytes((size_t)P, max_chunks);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "alignment scratch of %zu bytes, %zu needed (mdpt_post_align_scratch_bytes)", scratch_bytes, need);
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
    for (int p = 0; p < P; ++p) {
        const size_t px = (size_t)pairs_host[p].H * pairs_host[p].W;
        max_pixels = px > max_pixels ? px : max_pixels;
    }
    CHK(mdpt_launch_post_align_apply((const AlignPair*)pairs_dev, P, max_pixels, pred_dtype, space == MDPT_ALIGN_INVERSE, (const double*)fit_f64,
                                     (const long long*)out_offsets_dev, dmin, dmax, (float*)out_f32, (hipStream_t)stream));
    return 0;
}

// ---- photo-guided upsampling (the fast guided filter with the photo as guide)
static_assert(sizeof(mdpt_guided_pair) == sizeof(GuidedPair) && sizeof(mdpt_guided_pair) == 56, "mdpt_guided_pair of include/mdpt.h is GuidedPair of mdpt_kernels.h");

// the host table's map sizes: positive, h w < 2^31; *bytes = the scratch of the P regions laid end to end
static int check_guided_sizes(const mdpt_guided_pair* pairs, int32_t P, size_t* bytes) {
    if (!pairs) return fail(MDPT_E_INVALID, "null argument");
    if (P <= 0 || P > 65535) return fail(MDPT_E_INVALID, "bad pair count %d (1 .. 65535 per call)", P);
    size_t total = 0;
    for (int p = 0; p < P; ++p) {
        const mdpt_guided_pair& q = pairs[p];
        if (q.h <= 0 || q.w <= 0 || (size_t)q.h * q.w >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "bad map size %dx%d (pair %d; h w < 2^31)", q.h, q.w, p);
        total += guided_pair_scratch_bytes((size_t)q.h, (size_t)q.w);
    }
    *bytes = total;
    return 0;
}

int mdpt_post_guided_scratch_bytes(const mdpt_guided_pair* pairs_host, int32_t P, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    return check_guided_sizes(pairs_host, P, bytes);
}

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
    std::vector<std::pair<size_t, size_t>> regions;
    for (int p = 0; p < P; ++p) {
        const mdpt_guided_pair& q = pairs_host[p];
        if (!q.map || !q.photo || !q.out) return fail(MDPT_E_INVALID, "null map, photo or output (pair %d)", p);
        if (((uintptr_t)q.map & (dtype_bytes(map_dtype) - 1)) != 0 || ((uintptr_t)q.out & 3) != 0)
            return fail(MDPT_E_INVALID, "misaligned map or output (pair %d: the map needs its element, the output 4 bytes)", p);
        if (q.H < q.h || q.W < q.w)
            return fail(MDPT_E_INVALID, "the %dx%d photo of pair %d is smaller than its %dx%d map: guided upsampling only enlarges", q.H, q.W, p, q.h, q.w);
        if ((size_t)q.H * q.W >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "a photo of %dx%d is too large (H W < 2^31, pair %d)", q.H, q.W, p);
        if (q.pitch < 3 * (int64_t)q.W) return fail(MDPT_E_INVALID, "a row pitch of %lld bytes is less than the %d pixels of a row (pair %d)", (long long)q.pitch, q.W, p);
        const size_t need = guided_pair_scratch_bytes((size_t)q.h, (size_t)q.w);
        if (q.scratch_off < 0 || (q.scratch_off & 7) != 0 || (size_t)q.scratch_off > scratch_bytes || scratch_bytes - (size_t)q.scratch_off < need)
            return fail(MDPT_E_INVALID, "the scratch region of pair %d (offset %lld, %zu bytes) is misaligned or outside the %zu bytes given "
                        "(mdpt_post_guided_scratch_bytes)", p, (long long)q.scratch_off, need, scratch_bytes);
        regions.emplace_back((size_t)q.scratch_off, (size_t)q.scratch_off + need);
        max_h = q.h > max_h ? q.h : max_h, max_w = q.w > max_w ? q.w : max_w;
        max_H = q.H > max_H ? q.H : max_H, max_W = q.W > max_W ? q.W : max_W;
    }
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); ++k)
        if (regions[k].first < regions[k - 1].second) return fail(MDPT_E_INVALID, "the scratch regions of two pairs overlap (at byte %zu)", regions[k].first);
    CHK(mdpt_launch_post_guided((const GuidedPair*)pairs_dev, P, map_dtype, radius, eps, max_h, max_w, max_H, max_W, (char*)scratch, (double*)coeffs_f64,
                                (hipStream_t)stream));
    return 0;
}

// ---- rendering of depth meshes (3dviewer/index.html:1158-1228 render_3d, shaders.js mesh shaders)
static_assert(sizeof(mdpt_texture) == sizeof(RenderTex) && sizeof(mdpt_texture) == 16, "mdpt_texture of include/mdpt.h is RenderTex of mdpt_kernels.h");

static int check_render_sizes(int32_t B, int32_t V, int32_t nv, int32_t nf, int32_t out_h, int32_t out_w) {
    if (B <= 0 || V <= 0 || (int64_t)B * V > 65535) return fail(MDPT_E_INVALID, "bad batch %d x %d views (the product must be 1 .. 65535 per call)", B, V);
    if (nv <= 0 || nf <= 0) return fail(MDPT_E_INVALID, "bad mesh capacity: %d vertices, %d faces", nv, nf);
    if (out_h <= 0 || out_w <= 0 || out_h > RENDER_MAX_SIDE || out_w > RENDER_MAX_SIDE)
        return fail(MDPT_E_INVALID, "bad output size %dx%d (sides of 1 .. %d)", out_h, out_w, RENDER_MAX_SIDE);
    return 0;
}

int mdpt_post_render_scratch_bytes(int32_t B, int32_t V, int32_t nv, int32_t nf, int32_t out_h, int32_t out_w, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_render_sizes(B, V, nv, nf, out_h, out_w));
    *bytes = render_scratch_bytes((size_t)B, (size_t)V, (size_t)nv, (size_t)out_h, (size_t)out_w);
    return 0;
}

int mdpt_post_render(const void* xyz_f32, const void* uv_f32, const void* faces_i32, const void* counts_i32, int32_t B, int32_t nv, int32_t nf,
                     int32_t mode, const mdpt_texture* tex_host, const void* tex_dev, const void* view_proj_f64, int32_t V, int32_t out_h, int32_t out_w,
                     int32_t cull_back, double point_size, void* color_bgra, void* depth_f32, void* face_id_i32, void* scratch, size_t scratch_bytes,
                     void* stream) {
    if (!xyz_f32 || !uv_f32 || !faces_i32 || !counts_i32 || !tex_host || !tex_dev || !view_proj_f64 || !color_bgra || !scratch)
        return fail(MDPT_E_INVALID, "null argument");
    CHK(check_render_sizes(B, V, nv, nf, out_h, out_w));
    if (mode != MDPT_MESH_TRIANGLES && mode != MDPT_MESH_POINTS) return fail(MDPT_E_INVALID, "unknown mesh mode %d", mode);
    if (mode == MDPT_MESH_POINTS && nf != nv) return fail(MDPT_E_INVALID, "a point list holds one face per vertex: nf %d, nv %d", nf, nv);
    if (!(point_size > 0.0 && point_size <= 1024.0)) return fail(MDPT_E_INVALID, "point_size must be in (0, 1024], got %g", point_size);
    for (int i = 0; i < B; ++i)
        if (!tex_host[i].bgr || tex_host[i].h <= 0 || tex_host[i].w <= 0)
            return fail(MDPT_E_INVALID, "null texture or bad texture size %dx%d (mesh %d)", tex_host[i].h, tex_host[i].w, i);
    if ((((uintptr_t)tex_dev | (uintptr_t)view_proj_f64 | (uintptr_t)scratch) & 7) != 0 ||
        (((uintptr_t)xyz_f32 | (uintptr_t)uv_f32 | (uintptr_t)faces_i32 | (uintptr_t)counts_i32 | (uintptr_t)color_bgra | (uintptr_t)depth_f32 |
          (uintptr_t)face_id_i32) & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the matrices and the scratch need 8 bytes, the slabs and the outputs 4)");
    const size_t need = render_scratch_bytes((size_t)B, (size_t)V, (size_t)nv, (size_t)out_h, (size_t)out_w);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "render scratch of %zu bytes, %zu needed (mdpt_post_render_scratch_bytes)", scratch_bytes, need);
    RenderJob r{};
    r.xyz = (const float*)xyz_f32, r.uv = (const float*)uv_f32, r.faces = (const int*)faces_i32, r.counts = (const int*)counts_i32;
    r.tex = (const RenderTex*)tex_dev, r.view_proj = (const double*)view_proj_f64;
    r.B = B, r.V = V, r.nv = nv, r.nf = nf, r.H = out_h, r.W = out_w, r.points = mode == MDPT_MESH_POINTS, r.cull_back = cull_back != 0;
    r.half = (int)nearbyint(point_size * 128.0);
    r.zbuf = (unsigned long long*)scratch;
    r.verts = (RenderVertex*)(r.zbuf + (size_t)B * V * out_h * out_w);
    CHK(mdpt_launch_post_render(r, (unsigned char*)color_bgra, (float*)depth_f32, (int*)face_id_i32, (hipStream_t)stream));
    return 0;
}

// ---- hole filling of rendered views (depth-banded push-pull; not in the reference)
static int check_fill_sizes(int32_t N, int32_t H, int32_t W) {
    if (N <= 0 || N > 65535) return fail(MDPT_E_INVALID, "bad image count %d (1 .. 65535 per call)", N);
    if (H <= 0 || W <= 0 || H > RENDER_MAX_SIDE || W > RENDER_MAX_SIDE) return fail(MDPT_E_INVALID, "bad image size %dx%d (sides of 1 .. %d)", H, W, RENDER_MAX_SIDE);
    return 0;
}

int mdpt_post_fill_scratch_bytes(int32_t N, int32_t H, int32_t W, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_fill_sizes(N, H, W));
    *bytes = fill_scratch_bytes((size_t)N, H, W);
    return 0;
}

int mdpt_post_fill_holes(const void* color_bgra, const void* depth_f32, int32_t N, int32_t H, int32_t W, double band, void* out_bgra, void* out_depth_f32,
                         void* scratch, size_t scratch_bytes, void* stream) {
    if (!color_bgra || !depth_f32 || !out_bgra || !scratch) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_fill_sizes(N, H, W));
    if (!(band >= 0.0 && band <= 1.0)) return fail(MDPT_E_INVALID, "band must be in [0, 1], got %g", band);
    if ((((uintptr_t)color_bgra | (uintptr_t)depth_f32 | (uintptr_t)out_bgra | (uintptr_t)out_depth_f32) & 3) != 0 || ((uintptr_t)scratch & 15) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the images and the depths need 4 bytes, the scratch 16)");
    if (out_bgra == color_bgra || (out_depth_f32 && out_depth_f32 == depth_f32))
        return fail(MDPT_E_INVALID, "the outputs must be buffers of their own, not the inputs");
    const size_t need = fill_scratch_bytes((size_t)N, H, W);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "fill scratch of %zu bytes, %zu needed (mdpt_post_fill_scratch_bytes)", scratch_bytes, need);
    FillJob j{};
    j.color = (const unsigned char*)color_bgra, j.depth = (const float*)depth_f32, j.out = (unsigned char*)out_bgra, j.out_depth = (float*)out_depth_f32;
    j.scratch = scratch, j.N = N, j.keep = 1.0 - band, j.plan = fill_plan(H, W);
    CHK(mdpt_launch_post_fill(j, (hipStream_t)stream));
    return 0;
}

// ---- temporally stable video depth (frame-to-frame fit, temporal filter, carried display range; not in the reference)
static int check_video_sizes(int32_t T, int32_t h, int32_t w) {
    if (T <= 0 || T > 65535) return fail(MDPT_E_INVALID, "bad frame count %d (1 .. 65535 per call)", T);
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
        ((uintptr_t)started_i32 & 3) != 0 || (((uintptr_t)frames | (uintptr_t)prev_frame) & (dtype_bytes(dtype) - 1)) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the fp64 buffers and the scratch need 8 bytes, the flag 4, the frames their element)");
    const size_t need = video_fit_scratch_doubles((size_t)T, (size_t)h * w) * sizeof(double);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "video scratch of %zu bytes, %zu needed (mdpt_post_video_scratch_bytes)", scratch_bytes, need);
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
    if (((uintptr_t)table_f64 & 7) != 0 || (((uintptr_t)prev_out_f32 | (uintptr_t)out_f32) & 3) != 0 || ((uintptr_t)frames & (dtype_bytes(dtype) - 1)) != 0)
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
    const size_t need = video_display_scratch_bytes((size_t)T, out_px, resize);
    if (scratch_bytes < need) return fail(MDPT_E_INVALID, "video scratch of %zu bytes, %zu needed (mdpt_post_video_scratch_bytes)", scratch_bytes, need);
    unsigned* parts = (unsigned*)scratch;
    unsigned* rparts = parts + (size_t)T * MDPT_POST_SEG_PARTS * 2;
    float* scaled = resize ? (float*)(rparts + (size_t)T * MDPT_POST_SEG_PARTS * 2) : nullptr;
    unsigned char* u8 = (unsigned char*)(rparts + (size_t)T * MDPT_POST_SEG_PARTS * 2) + (resize ? (size_t)T * out_px * sizeof(float) : 0);
    CHK(mdpt_launch_post_video_display((const float*)stable_f32, T, h, w, resize ? out_h : h, resize ? out_w : w, (const double*)table_f64,
                                       (const float*)range_in_f32, (const int*)started_i32, range_rate, reverse != 0, (const unsigned char*)cmap_bgr, scaled, parts,
                                       rparts, u8, (unsigned char*)out_bgr, (float*)ranges_f32, (float*)range_out_f32, (hipStream_t)stream));
    return 0;
}

// ---- synthetic depth of field (per-pixel defocus, occlusion-aware gather; not in the reference)
static_assert(sizeof(mdpt_refocus_pair) == sizeof(RefocusPair) && sizeof(mdpt_refocus_pair) == 64, "mdpt_refocus_pair of include/mdpt.h is RefocusPair of mdpt_kernels.h");
static_assert(offsetof(mdpt_refocus_pair, photo) == offsetof(RefocusPair, photo) && offsetof(mdpt_refocus_pair, pitch) == offsetof(RefocusPair, pitch) &&
              offsetof(mdpt_refocus_pair, H) == offsetof(RefocusPair, H) && offsetof(mdpt_refocus_pair, out) == offsetof(RefocusPair, out) &&
              offsetof(mdpt_refocus_pair, scratch_off) == offsetof(RefocusPair, scratch_off) && offsetof(mdpt_refocus_pair, tile_off) == 56 &&
              offsetof(RefocusPair, tile_off) == 56, "mdpt_refocus_pair of include/mdpt.h is RefocusPair of mdpt_kernels.h, field by field");
static_assert(MDPT_REFOCUS_MAX_RADIUS == REFOCUS_MAX_RADIUS && MDPT_REFOCUS_TILE == REFOCUS_TILE, "the refocus limits of include/mdpt.h are those of mdpt_kernels.h");

// the host table's photo sizes: positive, H W < 2^31; *bytes = the scratch of the P regions laid end to end
static int check_refocus_sizes(const mdpt_refocus_pair* pairs, int32_t P, int32_t max_radius, size_t* bytes) {
    if (!pairs) return fail(MDPT_E_INVALID, "null argument (records)");
    if (P <= 0 || P > 65535) return fail(MDPT_E_INVALID, "bad pair count n = %d (1 .. 65535 per call)", P);
    if (max_radius < 0 || max_radius > REFOCUS_MAX_RADIUS) return fail(MDPT_E_INVALID, "max_radius %d: the blur radius limit must be 0 .. %d pixels", max_radius, REFOCUS_MAX_RADIUS);
    size_t total = 0;
    for (int p = 0; p < P; ++p) {
        const mdpt_refocus_pair& q = pairs[p];
        if (q.H <= 0 || q.W <= 0) return fail(MDPT_E_INVALID, "bad photo size %dx%d (pair %d)", q.H, q.W, p);
        if ((size_t)q.H * q.W >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "a photo of %dx%d is too large (H W < 2^31 pixels, pair %d)", q.H, q.W, p);
        total += refocus_pair_scratch_bytes((size_t)q.H, (size_t)q.W);
    }
    *bytes = total;
    return 0;
}

int mdpt_post_refocus_scratch_bytes(const mdpt_refocus_pair* records_host, int32_t n, int32_t max_radius, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    return check_refocus_sizes(records_host, n, max_radius, bytes);
}

int mdpt_post_refocus(const mdpt_refocus_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double focus,
                      const double* focus_xy, double aperture, double focus_range, int32_t max_radius, void* scratch, size_t scratch_bytes, void* radius_out,
                      void* defocus_out, void* stream) {
    if (!records_host || !records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_host, records_dev or scratch)");
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown refocus space %d", space);
    size_t packed;
    CHK(check_refocus_sizes(records_host, n, max_radius, &packed));
    if (!(aperture >= 0.0) || aperture > 1e300) return fail(MDPT_E_INVALID, "aperture must be finite and >= 0 (pixels per unit of defocus), got %g", aperture);
    if (!(focus_range >= 0.0) || focus_range > 1e300) return fail(MDPT_E_INVALID, "focus_range must be finite and >= 0, got %g", focus_range);
    if (focus_xy) {
        if (!(focus_xy[0] >= 0.0 && focus_xy[0] <= 1.0 && focus_xy[1] >= 0.0 && focus_xy[1] <= 1.0))
            return fail(MDPT_E_INVALID, "focus_xy must lie in [0, 1]^2, got (%g, %g)", focus_xy[0], focus_xy[1]);
    } else if (space == MDPT_ALIGN_INVERSE ? !(focus >= 0.0 && focus <= 1.0) : (!(focus > 0.0) || focus > 1e300)) {
        return fail(MDPT_E_INVALID, "focus %g is outside its domain (inverse space: 0 .. 1 of the map's range; depth space: a finite depth > 0)", focus);
    }
    if ((((uintptr_t)records_dev | (uintptr_t)scratch) & 7) != 0 || ((uintptr_t)defocus_out & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table and the scratch need 8 bytes, defocus_out 4)");
    size_t max_pixels = 0, tiles = 0;
    int with_out = 0;
    std::vector<std::pair<size_t, size_t>> regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_refocus_pair& q = records_host[p];
        if (!q.map || !q.photo) return fail(MDPT_E_INVALID, "null map or photo (pair %d)", p);
        if (((uintptr_t)q.map & (dtype_bytes(dtype) - 1)) != 0) return fail(MDPT_E_INVALID, "misaligned map (pair %d: it needs its element)", p);
        if (q.h <= 0 || q.w <= 0 || (size_t)q.h * q.w >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "bad map size %dx%d (pair %d; h w < 2^31)", q.h, q.w, p);
        if (q.pitch < 3 * (int64_t)q.W) return fail(MDPT_E_INVALID, "a row pitch of %lld bytes is less than the %d pixels of a row (pair %d)", (long long)q.pitch, q.W, p);
        const size_t px = (size_t)q.H * q.W, need = refocus_pair_scratch_bytes((size_t)q.H, (size_t)q.W);
        if (q.scratch_off < 0 || (q.scratch_off & 7) != 0 || (size_t)q.scratch_off > scratch_bytes || scratch_bytes - (size_t)q.scratch_off < need)
            return fail(MDPT_E_INVALID, "the scratch region of pair %d (offset %lld, %zu bytes) is misaligned or outside the %zu bytes of scratch given "
                        "(mdpt_post_refocus_scratch_bytes)", p, (long long)q.scratch_off, need, scratch_bytes);
        if (q.tile_off != (int64_t)tiles)
            return fail(MDPT_E_INVALID, "tile_off %lld of pair %d is not the %zu tiles of %dx%d pixels of the pairs before it", (long long)q.tile_off, p, tiles,
                        REFOCUS_TILE, REFOCUS_TILE);
        regions.emplace_back((size_t)q.scratch_off, (size_t)q.scratch_off + need);
        tiles += refocus_pair_tiles((size_t)q.H, (size_t)q.W);
        max_pixels = px > max_pixels ? px : max_pixels;
        with_out += q.out != nullptr;
    }
    if (with_out != 0 && with_out != n) return fail(MDPT_E_INVALID, "out is null in %d of %d records: every pair has an output, or none (the preparation alone)", n - with_out, n);
    if (!with_out && !radius_out && !defocus_out) return fail(MDPT_E_INVALID, "null argument: no record has an output and neither radius_out nor defocus_out is given");
    if (tiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu tiles: a call takes fewer than 2^31", tiles);
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); ++k)
        if (regions[k].first < regions[k - 1].second) return fail(MDPT_E_INVALID, "the scratch regions of two pairs overlap (at byte %zu)", regions[k].first);
    RefocusJob j{};
    j.pairs = (const RefocusPair*)records_dev;
    j.P = n, j.dt = dtype, j.depth_space = space == MDPT_ALIGN_DEPTH, j.pointed = focus_xy != nullptr, j.max_radius = max_radius, j.gather = with_out != 0;
    j.focus = focus_xy ? 0.0 : (j.depth_space ? 1.0 / focus : focus);
    j.fx = focus_xy ? focus_xy[0] : 0.0, j.fy = focus_xy ? focus_xy[1] : 0.0;
    j.aperture = aperture, j.half_range = focus_range / 2.0;
    j.scratch = (char*)scratch, j.radius_out = (unsigned char*)radius_out, j.defocus_out = (float*)defocus_out;
    j.max_pixels = max_pixels, j.total_tiles = tiles;
    CHK(mdpt_launch_post_refocus(j, (hipStream_t)stream));
    return 0;
}

// ---- surface normals and relighting (edge-aware differences of the unprojected map, Lambert / Blinn-Phong mix; not in the reference)
static_assert(sizeof(mdpt_normals_pair) == sizeof(NormalsPair) && sizeof(mdpt_normals_pair) == 104, "mdpt_normals_pair of include/mdpt.h is NormalsPair of mdpt_kernels.h");
static_assert(offsetof(mdpt_normals_pair, photo) == offsetof(NormalsPair, photo) && offsetof(mdpt_normals_pair, pitch) == offsetof(NormalsPair, pitch) &&
              offsetof(mdpt_normals_pair, H) == offsetof(NormalsPair, H) && offsetof(mdpt_normals_pair, normals) == offsetof(NormalsPair, normals) &&
              offsetof(mdpt_normals_pair, encoded) == offsetof(NormalsPair, encoded) && offsetof(mdpt_normals_pair, relit) == offsetof(NormalsPair, relit) &&
              offsetof(mdpt_normals_pair, scratch_off) == offsetof(NormalsPair, scratch_off) && offsetof(mdpt_normals_pair, tile_off) == offsetof(NormalsPair, tile_off) &&
              offsetof(mdpt_normals_pair, kx) == offsetof(NormalsPair, kx) && offsetof(mdpt_normals_pair, ky) == offsetof(NormalsPair, ky) &&
              offsetof(mdpt_normals_pair, step) == 96 && offsetof(NormalsPair, step) == 96, "mdpt_normals_pair of include/mdpt.h is NormalsPair of mdpt_kernels.h, field by field");
static_assert(MDPT_NORMALS_MAX_STEP == NORMALS_MAX_STEP && MDPT_NORMALS_TILE == NORMALS_TILE && MDPT_NORMALS_MAX_LIGHTS == NORMALS_MAX_LIGHTS,
              "the normals limits of include/mdpt.h are those of mdpt_kernels.h");

// the host table's photo sizes: positive, H W < 2^31; *bytes = the scratch of the P regions laid end to end
static int check_normals_sizes(const mdpt_normals_pair* pairs, int32_t P, size_t* bytes) {
    if (!pairs) return fail(MDPT_E_INVALID, "null argument (records)");
    if (P <= 0 || P > 65535) return fail(MDPT_E_INVALID, "bad pair count n = %d (1 .. 65535 per call)", P);
    for (int p = 0; p < P; ++p) {
        const mdpt_normals_pair& q = pairs[p];
        if (q.H <= 0 || q.W <= 0) return fail(MDPT_E_INVALID, "bad photo size %dx%d (pair %d)", q.H, q.W, p);
        if ((size_t)q.H * q.W >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "a photo of %dx%d is too large (H W < 2^31 pixels, pair %d)", q.H, q.W, p);
    }
    *bytes = (size_t)P * NORMALS_HEADER_BYTES;
    return 0;
}

int mdpt_post_normals_scratch_bytes(const mdpt_normals_pair* records_host, int32_t n, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    return check_normals_sizes(records_host, n, bytes);
}

int mdpt_post_normals(const mdpt_normals_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double min_depth,
                      double max_depth, double edge_ratio, const void* lights_dev, int32_t num_lights, double ambient, double diffuse, double specular,
                      int32_t shininess_log2, void* scratch, size_t scratch_bytes, void* stream) {
    if (!records_host || !records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_host, records_dev or scratch)");
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown normals space %d", space);
    size_t packed;
    CHK(check_normals_sizes(records_host, n, &packed));
    if (space == MDPT_ALIGN_INVERSE && !(min_depth > 0.0 && min_depth < max_depth && max_depth <= 1e300))
        return fail(MDPT_E_INVALID, "need 0 < min_depth < max_depth, finite, in inverse space, got %g, %g", min_depth, max_depth);
    if (!(edge_ratio >= 1.0)) return fail(MDPT_E_INVALID, "edge_ratio must be >= 1 (inf: always the central difference), got %g", edge_ratio);
    if (num_lights < 0 || num_lights > NORMALS_MAX_LIGHTS) return fail(MDPT_E_INVALID, "bad light count num_lights = %d (0 .. %d per call)", num_lights, NORMALS_MAX_LIGHTS);
    if (!(ambient >= 0.0 && ambient <= 1e300 && diffuse >= 0.0 && diffuse <= 1e300 && specular >= 0.0 && specular <= 1e300))
        return fail(MDPT_E_INVALID, "ambient, diffuse and specular must be finite and >= 0, got %g, %g, %g", ambient, diffuse, specular);
    if (shininess_log2 < 0 || shininess_log2 > 10) return fail(MDPT_E_INVALID, "shininess_log2 %d: the number of squarings must be 0 .. 10", shininess_log2);
    if ((((uintptr_t)records_dev | (uintptr_t)scratch | (uintptr_t)lights_dev) & 7) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the lights and the scratch need 8 bytes)");
    size_t tiles = 0;
    int with_normals = 0, with_encoded = 0, with_relit = 0, with_photo = 0;
    std::vector<std::pair<size_t, size_t>> regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_normals_pair& q = records_host[p];
        if (!q.map) return fail(MDPT_E_INVALID, "null map (pair %d)", p);
        if (((uintptr_t)q.map & (dtype_bytes(dtype) - 1)) != 0) return fail(MDPT_E_INVALID, "misaligned map (pair %d: it needs its element)", p);
        if (q.h <= 0 || q.w <= 0 || (size_t)q.h * q.w >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "bad map size %dx%d (pair %d; h w < 2^31)", q.h, q.w, p);
        if (q.photo && q.pitch < 3 * (int64_t)q.W)
            return fail(MDPT_E_INVALID, "a row pitch of %lld bytes is less than the %d pixels of a row (pair %d)", (long long)q.pitch, q.W, p);
        if (q.step < 1 || q.step > NORMALS_MAX_STEP) return fail(MDPT_E_INVALID, "step %d of pair %d: the difference step must be 1 .. %d photo pixels", q.step, p, NORMALS_MAX_STEP);
        if (!(q.kx > 0.0 && q.kx <= 1e300 && q.ky > 0.0 && q.ky <= 1e300)) return fail(MDPT_E_INVALID, "the camera scales kx, ky of pair %d must be finite and > 0, got %g, %g", p, q.kx, q.ky);
        if (((uintptr_t)q.normals & 3) != 0) return fail(MDPT_E_INVALID, "misaligned normals output (pair %d: fp32)", p);
        if (q.scratch_off < 0 || (q.scratch_off & 7) != 0 || (size_t)q.scratch_off > scratch_bytes || scratch_bytes - (size_t)q.scratch_off < NORMALS_HEADER_BYTES)
            return fail(MDPT_E_INVALID, "the scratch region of pair %d (offset %lld, %d bytes) is misaligned or outside the %zu bytes of scratch given "
                        "(mdpt_post_normals_scratch_bytes)", p, (long long)q.scratch_off, NORMALS_HEADER_BYTES, scratch_bytes);
        if (q.tile_off != (int64_t)tiles)
            return fail(MDPT_E_INVALID, "tile_off %lld of pair %d is not the %zu tiles of %dx%d pixels of the pairs before it", (long long)q.tile_off, p, tiles,
                        NORMALS_TILE, NORMALS_TILE);
        regions.emplace_back((size_t)q.scratch_off, (size_t)q.scratch_off + NORMALS_HEADER_BYTES);
        tiles += normals_pair_tiles((size_t)q.H, (size_t)q.W);
        with_normals += q.normals != nullptr, with_encoded += q.encoded != nullptr, with_relit += q.relit != nullptr, with_photo += q.photo != nullptr;
    }
    for (int got : {with_normals, with_encoded, with_relit})
        if (got != 0 && got != n) return fail(MDPT_E_INVALID, "an output is null in %d of %d records: every pair has it, or none", n - got, n);
    if (!with_normals && !with_encoded && !with_relit) return fail(MDPT_E_INVALID, "null argument: no record has an output (normals, encoded or relit)");
    if (with_relit && (num_lights < 1 || !lights_dev)) return fail(MDPT_E_INVALID, "relit frames are asked for without lights (lights_dev null or num_lights = %d)", num_lights);
    if (with_photo != 0 && with_photo != n) return fail(MDPT_E_INVALID, "photo is null in %d of %d records: every pair has a photo, or none (white clay)", n - with_photo, n);
    if (tiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu tiles: a call takes fewer than 2^31", tiles);
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); ++k)
        if (regions[k].first < regions[k - 1].second) return fail(MDPT_E_INVALID, "the scratch regions of two pairs overlap (at byte %zu)", regions[k].first);
    NormalsJob j{};
    j.pairs = (const NormalsPair*)records_dev;
    j.P = n, j.dt = dtype, j.depth_space = space == MDPT_ALIGN_DEPTH, j.central_only = edge_ratio > 1e300, j.V = with_relit ? num_lights : 0;
    j.shininess_log2 = shininess_log2;
    if (!j.depth_space) j.depth_a = 1.0 / max_depth, j.depth_b = 1.0 / min_depth - 1.0 / max_depth;
    j.edge_ratio = edge_ratio, j.ambient = ambient, j.diffuse = diffuse, j.specular = specular;
    j.lights = (const double*)lights_dev, j.scratch = (char*)scratch, j.total_tiles = tiles;
    CHK(mdpt_launch_post_normals(j, (hipStream_t)stream));
    return 0;
}

// ---- cast shadows and ambient occlusion for the relighting (marches on a working grid, folded into the shading; not in the reference)
static_assert(sizeof(mdpt_shadows_pair) == sizeof(ShadowsPair) && sizeof(mdpt_shadows_pair) == 120, "mdpt_shadows_pair of include/mdpt.h is ShadowsPair of mdpt_kernels.h");
static_assert(offsetof(mdpt_shadows_pair, photo) == offsetof(ShadowsPair, photo) && offsetof(mdpt_shadows_pair, pitch) == offsetof(ShadowsPair, pitch) &&
              offsetof(mdpt_shadows_pair, H) == offsetof(ShadowsPair, H) && offsetof(mdpt_shadows_pair, gh) == offsetof(ShadowsPair, gh) &&
              offsetof(mdpt_shadows_pair, gw) == offsetof(ShadowsPair, gw) && offsetof(mdpt_shadows_pair, ao) == offsetof(ShadowsPair, ao) &&
              offsetof(mdpt_shadows_pair, vis) == offsetof(ShadowsPair, vis) && offsetof(mdpt_shadows_pair, relit) == offsetof(ShadowsPair, relit) &&
              offsetof(mdpt_shadows_pair, scratch_off) == offsetof(ShadowsPair, scratch_off) && offsetof(mdpt_shadows_pair, tile_off) == offsetof(ShadowsPair, tile_off) &&
              offsetof(mdpt_shadows_pair, gtile_off) == offsetof(ShadowsPair, gtile_off) && offsetof(mdpt_shadows_pair, kx) == offsetof(ShadowsPair, kx) &&
              offsetof(mdpt_shadows_pair, ky) == offsetof(ShadowsPair, ky) && offsetof(mdpt_shadows_pair, step) == 112 && offsetof(ShadowsPair, step) == 112,
              "mdpt_shadows_pair of include/mdpt.h is ShadowsPair of mdpt_kernels.h, field by field");
static_assert(MDPT_SHADOWS_MAX_REACH == SHADOWS_MAX_REACH && MDPT_SHADOWS_AO_DIRECTIONS == SHADOWS_AO_DIRECTIONS, "the shadow limits of include/mdpt.h are those of mdpt_kernels.h");

// the host table's photo and grid sizes: positive, fewer than 2^31 pixels / nodes; *bytes = the scratch of the P regions laid end to end
static int check_shadows_sizes(const mdpt_shadows_pair* pairs, int32_t P, size_t* bytes) {
    if (!pairs) return fail(MDPT_E_INVALID, "null argument (records)");
    if (P <= 0 || P > 65535) return fail(MDPT_E_INVALID, "bad pair count n = %d (1 .. 65535 per call)", P);
    for (int p = 0; p < P; ++p) {
        const mdpt_shadows_pair& q = pairs[p];
        if (q.H <= 0 || q.W <= 0) return fail(MDPT_E_INVALID, "bad photo size %dx%d (pair %d)", q.H, q.W, p);
        if ((size_t)q.H * q.W >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "a photo of %dx%d is too large (H W < 2^31 pixels, pair %d)", q.H, q.W, p);
        if (q.gh <= 0 || q.gw <= 0 || (size_t)q.gh * q.gw >= ((size_t)1 << 31))
            return fail(MDPT_E_INVALID, "bad working grid %dx%d (pair %d; positive, gh gw < 2^31 nodes)", q.gh, q.gw, p);
    }
    *bytes = (size_t)P * NORMALS_HEADER_BYTES;
    return 0;
}

int mdpt_post_shadows_scratch_bytes(const mdpt_shadows_pair* records_host, int32_t n, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    return check_shadows_sizes(records_host, n, bytes);
}

int mdpt_post_shadows(const mdpt_shadows_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double min_depth,
                      double max_depth, double edge_ratio, const void* lights_dev, int32_t num_lights, double ambient, double diffuse, double specular,
                      int32_t shininess_log2, int32_t shadow_reach, double shadow_bias, double shadow_thickness, int32_t ao_reach, double ao_radius,
                      double ao_bias, double ao_strength, void* scratch, size_t scratch_bytes, void* stream) {
    if (!records_host || !records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_host, records_dev or scratch)");
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown shadows space %d", space);
    size_t packed;
    CHK(check_shadows_sizes(records_host, n, &packed));
    if (space == MDPT_ALIGN_INVERSE && !(min_depth > 0.0 && min_depth < max_depth && max_depth <= 1e300))
        return fail(MDPT_E_INVALID, "need 0 < min_depth < max_depth, finite, in inverse space, got %g, %g", min_depth, max_depth);
    if (!(edge_ratio >= 1.0)) return fail(MDPT_E_INVALID, "edge_ratio must be >= 1 (inf: always the central difference), got %g", edge_ratio);
    if (num_lights < 0 || num_lights > NORMALS_MAX_LIGHTS) return fail(MDPT_E_INVALID, "bad light count num_lights = %d (0 .. %d per call)", num_lights, NORMALS_MAX_LIGHTS);
    if (!(ambient >= 0.0 && ambient <= 1e300 && diffuse >= 0.0 && diffuse <= 1e300 && specular >= 0.0 && specular <= 1e300))
        return fail(MDPT_E_INVALID, "ambient, diffuse and specular must be finite and >= 0, got %g, %g, %g", ambient, diffuse, specular);
    if (shininess_log2 < 0 || shininess_log2 > 10) return fail(MDPT_E_INVALID, "shininess_log2 %d: the number of squarings must be 0 .. 10", shininess_log2);
    if (shadow_reach < 0 || shadow_reach > SHADOWS_MAX_REACH) return fail(MDPT_E_INVALID, "shadow_reach %d: a shadow march takes 0 .. %d grid nodes", shadow_reach, SHADOWS_MAX_REACH);
    if (ao_reach < 0 || ao_reach > SHADOWS_MAX_REACH) return fail(MDPT_E_INVALID, "ao_reach %d: an occlusion direction takes 0 .. %d grid nodes", ao_reach, SHADOWS_MAX_REACH);
    if (!(shadow_bias >= 0.0 && shadow_bias < 1.0)) return fail(MDPT_E_INVALID, "shadow_bias must be in [0, 1), got %g", shadow_bias);
    if (!(shadow_thickness >= 0.0)) return fail(MDPT_E_INVALID, "shadow_thickness must be >= 0 (inf: an occluder of any thickness), got %g", shadow_thickness);
    if (!(ao_radius > 0.0 && ao_radius <= 1e300)) return fail(MDPT_E_INVALID, "ao_radius must be finite and > 0, got %g", ao_radius);
    if (!(ao_bias >= 0.0 && ao_bias <= 1e300 && ao_strength >= 0.0 && ao_strength <= 1e300))
        return fail(MDPT_E_INVALID, "ao_bias and ao_strength must be finite and >= 0, got %g, %g", ao_bias, ao_strength);
    if ((((uintptr_t)records_dev | (uintptr_t)scratch | (uintptr_t)lights_dev) & 7) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the lights and the scratch need 8 bytes)");
    size_t tiles = 0, gtiles = 0;
    int with_ao = 0, with_vis = 0, with_relit = 0, with_photo = 0;
    std::vector<std::pair<size_t, size_t>> regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_shadows_pair& q = records_host[p];
        if (!q.map) return fail(MDPT_E_INVALID, "null map (pair %d)", p);
        if (((uintptr_t)q.map & (dtype_bytes(dtype) - 1)) != 0) return fail(MDPT_E_INVALID, "misaligned map (pair %d: it needs its element)", p);
        if (q.h <= 0 || q.w <= 0 || (size_t)q.h * q.w >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "bad map size %dx%d (pair %d; h w < 2^31)", q.h, q.w, p);
        if (q.photo && q.pitch < 3 * (int64_t)q.W)
            return fail(MDPT_E_INVALID, "a row pitch of %lld bytes is less than the %d pixels of a row (pair %d)", (long long)q.pitch, q.W, p);
        if (q.step < 1 || q.step > NORMALS_MAX_STEP) return fail(MDPT_E_INVALID, "step %d of pair %d: the difference step must be 1 .. %d photo pixels", q.step, p, NORMALS_MAX_STEP);
        if (!(q.kx > 0.0 && q.kx <= 1e300 && q.ky > 0.0 && q.ky <= 1e300)) return fail(MDPT_E_INVALID, "the camera scales kx, ky of pair %d must be finite and > 0, got %g, %g", p, q.kx, q.ky);
        if ((((uintptr_t)q.ao | (uintptr_t)q.vis) & 3) != 0) return fail(MDPT_E_INVALID, "misaligned ao or vis plane (pair %d: fp32)", p);
        if (q.scratch_off < 0 || (q.scratch_off & 7) != 0 || (size_t)q.scratch_off > scratch_bytes || scratch_bytes - (size_t)q.scratch_off < NORMALS_HEADER_BYTES)
            return fail(MDPT_E_INVALID, "the scratch region of pair %d (offset %lld, %d bytes) is misaligned or outside the %zu bytes of scratch given "
                        "(mdpt_post_shadows_scratch_bytes)", p, (long long)q.scratch_off, NORMALS_HEADER_BYTES, scratch_bytes);
        if (q.tile_off != (int64_t)tiles)
            return fail(MDPT_E_INVALID, "tile_off %lld of pair %d is not the %zu tiles of %dx%d pixels of the pairs before it", (long long)q.tile_off, p, tiles,
                        NORMALS_TILE, NORMALS_TILE);
        if (q.gtile_off != (int64_t)gtiles)
            return fail(MDPT_E_INVALID, "gtile_off %lld of pair %d is not the %zu tiles of %dx%d grid nodes of the pairs before it", (long long)q.gtile_off, p,
                        gtiles, NORMALS_TILE, NORMALS_TILE);
        regions.emplace_back((size_t)q.scratch_off, (size_t)q.scratch_off + NORMALS_HEADER_BYTES);
        tiles += normals_pair_tiles((size_t)q.H, (size_t)q.W);
        gtiles += normals_pair_tiles((size_t)q.gh, (size_t)q.gw);
        with_ao += q.ao != nullptr, with_vis += q.vis != nullptr, with_relit += q.relit != nullptr, with_photo += q.photo != nullptr;
    }
    for (int got : {with_ao, with_vis, with_relit})
        if (got != 0 && got != n) return fail(MDPT_E_INVALID, "an output is null in %d of %d records: every pair has it, or none", n - got, n);
    if (!with_ao && !with_vis && !with_relit) return fail(MDPT_E_INVALID, "null argument: no record has an output (ao, vis or relit)");
    if ((with_relit || with_vis) && (num_lights < 1 || !lights_dev))
        return fail(MDPT_E_INVALID, "vis planes or relit frames are asked for without lights (lights_dev null or num_lights = %d)", num_lights);
    const bool use_vis = shadow_reach > 0, use_ao = ao_reach > 0 && ao_strength > 0.0;
    if (with_relit && ((use_vis && !with_vis) || (use_ao && !with_ao)))
        return fail(MDPT_E_INVALID, "the shading needs a plane that no record has (vis with shadow_reach > 0, ao with ao_reach > 0 and ao_strength > 0)");
    if (with_photo != 0 && with_photo != n) return fail(MDPT_E_INVALID, "photo is null in %d of %d records: every pair has a photo, or none (white clay)", n - with_photo, n);
    if (tiles >= ((size_t)1 << 31) || gtiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu photo tiles, %zu grid tiles: a call takes fewer than 2^31 of each", tiles, gtiles);
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); ++k)
        if (regions[k].first < regions[k - 1].second) return fail(MDPT_E_INVALID, "the scratch regions of two pairs overlap (at byte %zu)", regions[k].first);
    ShadowsJob j{};
    j.pairs = (const ShadowsPair*)records_dev;
    j.P = n, j.dt = dtype, j.depth_space = space == MDPT_ALIGN_DEPTH, j.central_only = edge_ratio > 1e300, j.V = (with_relit || with_vis) ? num_lights : 0;
    j.shininess_log2 = shininess_log2;
    if (!j.depth_space) j.depth_a = 1.0 / max_depth, j.depth_b = 1.0 / min_depth - 1.0 / max_depth;
    j.edge_ratio = edge_ratio, j.ambient = ambient, j.diffuse = diffuse, j.specular = specular;
    j.lights = (const double*)lights_dev, j.scratch = (char*)scratch, j.total_tiles = tiles, j.total_gtiles = gtiles;
    j.shadow_reach = shadow_reach, j.ao_reach = ao_reach, j.thick_inf = shadow_thickness > 1e300, j.use_vis = use_vis, j.use_ao = use_ao;
    j.planes = with_ao || with_vis, j.shade = with_relit != 0;
    j.shadow_bias = shadow_bias, j.shadow_thickness = shadow_thickness, j.ao_radius = ao_radius, j.ao_bias = ao_bias, j.ao_strength = ao_strength;
    CHK(mdpt_launch_post_shadows(j, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
