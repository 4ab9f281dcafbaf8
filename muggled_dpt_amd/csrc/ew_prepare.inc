// ---- uint8 BGR frame -> normalised model tensor through PyTorch's antialiased resize: alone (prepare_image) and fused with patchify

namespace {

// prepare_image (SURVEY §8(f) row 1; reference v2_depthanything/patch_embed.py:103-145): uint8 HxWx3 BGR ->
// [3, oh, ow] fp32, RGB order, resized with PyTorch's *antialiased* bilinear (F.interpolate(mode="bilinear",
// antialias=True, align_corners=False)) and normalised ((v/255) - mean) / std. The antialias filter is the
// separable triangle filter of aten's _upsample_bilinear2d_aa: per output index i, scale = in/out,
// support = max(scale, 1), centre = scale*(i+0.5), taps j in [floor(centre-support+0.5), floor(centre+support+0.5))
// clipped to the image, weight = max(0, 1 - |(j - centre + 0.5) / max(scale,1)|), normalised to sum 1. mode="bicubic" is the same
// machinery with the cubic filter (support 2*max(scale,1)).
// One thread per output pixel (all 3 channels): rows of weights are recomputed per pixel (<= ~2*scale+2 taps).
// INTERP 0 = bilinear (triangle filter, support 1), 1 = bicubic (Keys cubic with a = -0.5, support 2: aten's _upsample_bicubic2d_aa;
// its weights go negative, so outputs may over/undershoot the 0..255 range exactly like the reference's).
template <int INTERP>
__device__ __forceinline__ float aa_filter(float x) {
    x = fabsf(x);
    if (INTERP == 0) return fmaxf(0.0f, 1.0f - x);
    const float a = -0.5f;
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
    return 0.0f;
}

template <int INTERP>
__device__ __forceinline__ void aa_span(int i, float scale, int in_size, int& lo, int& n, float& center, float& invscale) {
    const float half_taps = INTERP == 0 ? 1.0f : 2.0f;  // interp_size / 2
    const float support = scale >= 1.0f ? half_taps * scale : half_taps;
    invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
    center = scale * ((float)i + 0.5f);
    lo = max((int)(center - support + 0.5f), 0);
    const int hi = min((int)(center + support + 0.5f), in_size);
    n = hi - lo;
}

// The output is written in the MODEL's dtype (out_dtype = MDPT_DT_*; the reference builds the tensor in the model dtype too,
// patch_embed.py:131-145 - here the filter runs in fp32 and rounds once): no cast kernel between this one and the patchify of mdpt_forward.
// One output pixel (all three channels, R G B): the arithmetic both kernels below share, so that the fused form's values equal the stand-alone one's bit for bit.
// The source is a BOX of an image read where it lies: `bgr` is the box's first pixel, ih x iw the box's size and `pitch` the bytes from one image
// row to the next (3 iw for a packed image). The taps clip at the box's edges (aa_span), as the reference's resize of the cropped array does:
// no pixel outside the box is read. A box starts at byte y1 pitch + 3 x1 of its image, which has no alignment: the loads stay byte-wise.
template <int INTERP>
__device__ __forceinline__ void aa_pixel_rgb(const unsigned char* __restrict__ bgr, size_t pitch, int ih, int iw, int oh, int ow, int oy, int ox, float m0, float m1, float m2,
                                             float s0, float s1, float s2, float& v0, float& v1, float& v2) {
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    int ylo, yn, xlo, xn;
    float yc, yinv, xc, xinv;
    aa_span<INTERP>(oy, sy, ih, ylo, yn, yc, yinv);
    aa_span<INTERP>(ox, sx, iw, xlo, xn, xc, xinv);
    float wxs = 0.0f, wys = 0.0f;
    for (int j = 0; j < xn; ++j) wxs += aa_filter<INTERP>(((float)(j + xlo) - xc + 0.5f) * xinv);
    for (int j = 0; j < yn; ++j) wys += aa_filter<INTERP>(((float)(j + ylo) - yc + 0.5f) * yinv);
    float acc_b = 0.0f, acc_g = 0.0f, acc_r = 0.0f;
    for (int a = 0; a < yn; ++a) {
        const float wy = aa_filter<INTERP>(((float)(a + ylo) - yc + 0.5f) * yinv) / wys;
        const unsigned char* row = bgr + (size_t)(ylo + a) * pitch + (size_t)xlo * 3;
        float rb = 0.0f, rg = 0.0f, rr = 0.0f;  // horizontal pass first (like the reference's separable CPU kernel)
        for (int c = 0; c < xn; ++c) {
            const float wx = aa_filter<INTERP>(((float)(c + xlo) - xc + 0.5f) * xinv) / wxs;
            rb += wx * (float)row[c * 3 + 0];
            rg += wx * (float)row[c * 3 + 1];
            rr += wx * (float)row[c * 3 + 2];
        }
        acc_b += wy * rb;
        acc_g += wy * rg;
        acc_r += wy * rr;
    }
    v0 = (acc_r / 255.0f - m0) * s0;  // channel 0 = R
    v1 = (acc_g / 255.0f - m1) * s1;  // channel 1 = G
    v2 = (acc_b / 255.0f - m2) * s2;  // channel 2 = B
}

template <int INTERP>
__global__ __launch_bounds__(256) void prepare_image_kernel(const unsigned char* __restrict__ bgr, size_t pitch, void* __restrict__ out, int out_dtype, int ih,
                                                            int iw, int oh, int ow, float m0, float m1, float m2, float s0,
                                                            float s1, float s2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= oh * ow) return;
    const int ox = idx % ow, oy = idx / ow;
    float v0, v1, v2;
    aa_pixel_rgb<INTERP>(bgr, pitch, ih, iw, oh, ow, oy, ox, m0, m1, m2, s0, s1, s2, v0, v1, v2);
    const size_t plane = (size_t)oh * ow;
    if (out_dtype == MDPT_DT_BF16) {
        __bf16* o = (__bf16*)out;
        o[idx] = (__bf16)v0; o[plane + idx] = (__bf16)v1; o[2 * plane + idx] = (__bf16)v2;
    } else if (out_dtype == MDPT_DT_F16) {
        _Float16* o = (_Float16*)out;
        o[idx] = (_Float16)v0; o[plane + idx] = (_Float16)v1; o[2 * plane + idx] = (_Float16)v2;
    } else {
        float* o = (float*)out;
        o[idx] = v0; o[plane + idx] = v1; o[2 * plane + idx] = v2;
    }
}

// prepare_image fused with patchify (SURVEY 8(f) row 1 as written; DPTModel.inference = patch_embed.py:103-145 -> :77-99): one thread = one pixel
// of the model tensor, computed from the uint8 image as above, rounded to the dtype the stand-alone kernel would have written it in (img_dt: the
// values - and so every bit behind them - equal mdpt_prepare_image + patchify_kernel) and stored straight into its three places of the patch
// embedding's im2col rows (k = c P^2 + ky P + kx). The normalised image never exists in memory. The first pixel of a patch also zeroes its
// row's padding columns [3 P^2, Kp). Batched (mdpt_forward_bgr_batch / _frames): blockIdx.y = frame b of the launch's frame table, read from its
// run's source with that run's own size, row pitch and frame stride (frame j of a run at ptr + j frame_stride), writes rows b gh gw + py gw + px, the row layout of patchify_kernel.
template <int INTERP>
__global__ __launch_bounds__(256) void prepare_patchify_kernel(const BgrRunTable t, int img_dt, op_t* out_hi, op_t* out_lo, int H, int W, int P, int Kp,
                                                               float m0, float m1, float m2, float s0, float s1, float s2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= H * W) return;
    const int b = blockIdx.y;
    int r = 0, j = b;  // frame b = frame j of run r (a block-uniform walk over the table; the grid holds exactly the table's frames)
    while (r < t.n - 1 && j >= t.run[r].count) j -= t.run[r++].count;
    const unsigned char* bgr = t.run[r].ptr;
    const int ih = t.run[r].ih, iw = t.run[r].iw;
    const int ox = idx % W, oy = idx / W;
    float v[3];
    aa_pixel_rgb<INTERP>(bgr + (size_t)j * (size_t)t.run[r].frame_stride, (size_t)t.run[r].pitch, ih, iw, H, W, oy, ox, m0, m1, m2, s0, s1, s2, v[0], v[1], v[2]);
    const int py = oy / P, ky = oy - py * P, px = ox / P, kx = ox - px * P;
    const size_t row = ((size_t)b * (H / P) * (W / P) + (size_t)py * (W / P) + px) * Kp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = img_dt == MDPT_DT_BF16 ? (float)(__bf16)v[c] : (img_dt == MDPT_DT_F16 ? (float)(_Float16)v[c] : v[c]);
        const size_t o = row + (size_t)c * P * P + ky * P + kx;
        const op_t h = to_op(r);
        out_hi[o] = h;
        if (out_lo) out_lo[o] = to_op(r - (float)h);
    }
    if (ky == 0 && kx == 0)
        for (int k = 3 * P * P; k < Kp; ++k) {
            out_hi[row + k] = to_op(0.0f);
            if (out_lo) out_lo[row + k] = to_op(0.0f);
        }
}

// INTERP as a template argument: launch(std::integral_constant<int, INTERP>)
template <typename Launch>
inline int interp_dispatch(int interp, Launch&& launch) {
    return interp == 0 ? launch(std::integral_constant<int, 0>{}) : launch(std::integral_constant<int, 1>{});
}

}  // namespace

int MDPT_FN(mdpt_launch_prepare_image)(const unsigned char* bgr, size_t pitch, void* out, int out_dtype, int ih, int iw, int oh, int ow, const float mean[3],
                              const float inv_std[3], int interp, hipStream_t stream) {
    if (pitch < (size_t)3 * (size_t)(iw > 0 ? iw : 0)) return (int)hipErrorInvalidValue;
    if (ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0 || (interp != 0 && interp != 1) || out_dtype < MDPT_DT_F32 || out_dtype > MDPT_DT_F16) return (int)hipErrorInvalidValue;
    return interp_dispatch(interp, [&](auto ip) {
        return ew_launch("prepare_image_kernel", 0.0, prepare_image_kernel<decltype(ip)::value>, dim3((oh * ow + 255) / 256), dim3(256), 0, stream, bgr, pitch, out,
                         out_dtype, ih, iw, oh, ow, mean[0], mean[1], mean[2], inv_std[0], inv_std[1], inv_std[2]);
    });
}

int MDPT_FN(mdpt_launch_prepare_patchify)(const BgrRunTable& t, int img_dtype, op_t* out_hi, op_t* out_lo, int H, int W, int P, int Kp,
                                         const float mean[3], const float inv_std[3], int interp, hipStream_t stream) {
    if (t.n <= 0 || t.n > MDPT_BGR_RUNS || H <= 0 || W <= 0 || P <= 0 || (H % P) || (W % P) || Kp < 3 * P * P || (interp != 0 && interp != 1) ||
        img_dtype < MDPT_DT_F32 || img_dtype > MDPT_DT_F16)
        return (int)hipErrorInvalidValue;
    int B = 0;
    for (int r = 0; r < t.n; ++r) {
        if (!t.run[r].ptr || t.run[r].ih <= 0 || t.run[r].iw <= 0 || t.run[r].count <= 0 || t.run[r].count > 65535 - B || t.run[r].pitch < 3ll * t.run[r].iw ||
            (t.run[r].count > 1 && t.run[r].frame_stride <= 0))
            return (int)hipErrorInvalidValue;
        B += t.run[r].count;
    }
    return interp_dispatch(interp, [&](auto ip) {
        return ew_launch("prepare_patchify_kernel", 0.0, prepare_patchify_kernel<decltype(ip)::value>, dim3((H * W + 255) / 256, B), dim3(256), 0, stream, t, img_dtype,
                         out_hi, out_lo, H, W, P, Kp, mean[0], mean[1], mean[2], inv_std[0], inv_std[1], inv_std[2]);
    });
}
