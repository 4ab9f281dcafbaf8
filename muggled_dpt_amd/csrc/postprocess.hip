// Depth post-processing on the GPU: the step immediately after the DPT forward in the reference's demos
// (muggled_dpt/demo_helpers/postprocess.py:22-29 scale_prediction, :63-74 normalize_01, :79-91 convert_to_uint8;
// run_3dviewer.py:576-590 24-bit packing). HBM-bound streaming kernels: fp32 in, fp32 / u8 out, no host round trip of the
// full-resolution fp32 map. min/max travel through a 2-float device buffer (no sync).

#include "mdpt_kernels.h"
#include "dt_io.h"
#include "mdpt_prof.h"

namespace {

// order-preserving float <-> uint mapping so that atomicMin/atomicMax on unsigned work for any sign
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ void minmax_init_kernel(unsigned* mm) {
    mm[0] = 0xffffffffu;  // running min (ordered domain)
    mm[1] = 0u;           // running max
}

// The block's (256 threads) min / max of every thread's (lo, hi), whether any thread saw a NaN and whether any holds a pixel at all: valid on
// thread 0. T = float or double. The trailing barrier lets a kernel call it (or read what a publisher below stored in LDS) more than once.
template <typename T>
struct BlockMinMax { T lo, hi; bool any_nan, any_px; };

template <typename T>
__device__ __forceinline__ BlockMinMax<T> block_minmax_reduce(T lo, T hi, bool saw_nan, bool any) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
    }
    BlockMinMax<T> r{lo, hi, __any(saw_nan) != 0, __any(any) != 0};
    __shared__ T slo[4], shi[4];
    __shared__ int snan[4], sany[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { slo[wave] = r.lo; shi[wave] = r.hi; snan[wave] = r.any_nan; sany[wave] = r.any_px; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) { r.lo = fmin(r.lo, slo[w]); r.hi = fmax(r.hi, shi[w]); r.any_nan |= snan[w] != 0; r.any_px |= sany[w] != 0; }
    __syncthreads();
    return r;
}

// torch's .min() / .max() PROPAGATE NaN (normalize_01 of a map with a NaN gives an all-NaN map) while fminf / fmaxf drop it: a thread
// that saw a NaN says so, and the block then pins its min to ordered 0 and its max to ordered ~0, both of which ord2f() maps back to NaN bit
// patterns. Three publishers of the block's result: atomics on a running ordered {min, max} ...
__device__ __forceinline__ void block_minmax(float lo, float hi, bool saw_nan, unsigned* mm) {
    const BlockMinMax<float> r = block_minmax_reduce(lo, hi, saw_nan, true);
    if (threadIdx.x == 0) {
        atomicMin(mm + 0, r.any_nan ? 0u : f2ord(r.lo));
        atomicMax(mm + 1, r.any_nan ? 0xffffffffu : f2ord(r.hi));
    }
}

// ... a store of the ordered {min, max} (the partials of the per-image kernels; a share without pixels is neutral) ...
__device__ __forceinline__ void block_minmax_part(float lo, float hi, bool saw_nan, bool any, unsigned* part) {
    const BlockMinMax<float> r = block_minmax_reduce(lo, hi, saw_nan, any);
    if (threadIdx.x == 0) {
        part[0] = r.any_nan ? 0u : (r.any_px ? f2ord(r.lo) : 0xffffffffu);
        part[1] = r.any_nan ? 0xffffffffu : (r.any_px ? f2ord(r.hi) : 0u);
    }
}

// ... and a store of the fp64 {min, max} (a NaN pins NaN, numpy's min / max propagate it; a share without pixels keeps {inf, -inf}: neutral)
__device__ __forceinline__ void block_minmax_f64(double lo, double hi, bool saw_nan, double* part) {
    const BlockMinMax<double> r = block_minmax_reduce(lo, hi, saw_nan, true);
    if (threadIdx.x == 0) {
        part[0] = r.any_nan ? NAN : r.lo;
        part[1] = r.any_nan ? NAN : r.hi;
    }
}

__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ in, size_t n, unsigned* mm) {
    float lo = INFINITY, hi = -INFINITY;
    bool saw_nan = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = in[i];
        saw_nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax(lo, hi, saw_nan, mm);
}

__global__ void minmax_finish_kernel(const unsigned* mm, float* out) {
    out[0] = ord2f(mm[0]);
    out[1] = ord2f(mm[1]);
}

// F.interpolate(x[:, None], size=(oh, ow), mode="bilinear") (align_corners=False, no antialias) of image `base` (ih x iw, dtype dt) at output pixel
// (oy, ox), sy = ih / oh, sx = iw / ow: src = max(0, s*(dst+0.5)-0.5); rounded to dt (the map scale_prediction returns).
// scale_bilinear_kernel's arithmetic as the compiler contracts it there (its gfx950 code: fma for the source position, one fma and one
// product per row, two products and an add across the rows), spelled out with _rn intrinsics so that no contraction choice here can differ
__device__ __forceinline__ float bilinear_at(const void* in, size_t base, int dt, int ih, int iw, float sy, float sx, int oy, int ox) {
    const float fy = fmaxf(__fmaf_rn(sy, (float)oy + 0.5f, -0.5f), 0.0f), fx = fmaxf(__fmaf_rn(sx, (float)ox + 0.5f, -0.5f), 0.0f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < ih - 1), x1 = x0 + (x0 < iw - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float p00 = ld_dt(in, base + (size_t)y0 * iw + x0, dt), p01 = ld_dt(in, base + (size_t)y0 * iw + x1, dt);
    const float p10 = ld_dt(in, base + (size_t)y1 * iw + x0, dt), p11 = ld_dt(in, base + (size_t)y1 * iw + x1, dt);
    const float top = __fmaf_rn(p01, lx, __fmul_rn(p00, 1.0f - lx)), bot = __fmaf_rn(p10, 1.0f - lx, __fmul_rn(p11, lx));
    return round_dt(__fadd_rn(__fmul_rn(1.0f - ly, top), __fmul_rn(ly, bot)), dt);
}

// scale_prediction of a uniform fp32 batch, left to the compiler's contraction (bilinear_at restates it; tests/test_gpu_display_tail.py keeps the
// two in step). Optionally folds the min/max reduction of the OUTPUT into the same pass (for
// convert_to_uint8(scale_prediction(x))).
__global__ __launch_bounds__(256) void scale_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int ih, int iw,
                                                             int oh, int ow, unsigned* mm) {
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    const size_t total = (size_t)B * oh * ow;
    float lo = INFINITY, hi = -INFINITY;
    bool saw_nan = false;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(idx % ow), oy = (int)((idx / ow) % oh);
        const size_t b = idx / ((size_t)ow * oh);
        const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.0f);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < ih - 1), x1 = x0 + (x0 < iw - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float* p = in + b * (size_t)ih * iw;
        const float v = (1.0f - ly) * ((1.0f - lx) * p[(size_t)y0 * iw + x0] + lx * p[(size_t)y0 * iw + x1]) +
                        ly * ((1.0f - lx) * p[(size_t)y1 * iw + x0] + lx * p[(size_t)y1 * iw + x1]);
        out[idx] = v;
        saw_nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    if (mm) block_minmax(lo, hi, saw_nan, mm);
}

// x, or (x - lo) / range with have_range: normalize_01 in fp32
__device__ __forceinline__ float norm01(float x, float lo, float range, bool have_range) { return have_range ? (x - lo) / range : x; }

// the same for an integer output: a NaN (max == min: 0 / 0; NaN anywhere in the map) becomes 0 - converting NaN to an integer is undefined in C and
// implementation-defined in torch's .byte(); values are clamped to the representable range before the conversion
__device__ __forceinline__ float norm_clamp01(float x, float lo, float range, bool have_range) {
    const float v = norm01(x, lo, range, have_range);
    return v == v ? fminf(fmaxf(v, 0.0f), 1.0f) : 0.0f;
}

// BGRA of v in [0, 1]: the 24-bit round-half-even(16777215 v) split into bytes (B = low, G = mid, R = high; lossy: high byte only), A = alpha
__device__ __forceinline__ uchar4 u24_px(float v, int lossy, unsigned char alpha) {
    const int q = (int)rintf(16777215.0f * v);
    uchar4 px;
    px.x = lossy ? 0 : (unsigned char)(q & 255);
    px.y = lossy ? 0 : (unsigned char)((q >> 8) & 255);
    px.z = (unsigned char)((q >> 16) & 255);
    px.w = alpha;
    return px;
}

// mode 0: fp32 (x - min) / (max - min); mode 1: u8 = trunc(255 * norm) (Tensor.byte()); mode 2: BGRA u8 = u24_px(norm), alpha left 0.
// minmax == null: the input is used as is (metric models skip normalize_01, run_3dviewer.py:577-578).
template <int MODE>
__global__ __launch_bounds__(256) void normalize_kernel(const float* __restrict__ in, const float* __restrict__ minmax, void* out, size_t n,
                                                        int lossy) {
    const float lo = minmax ? minmax[0] : 0.0f, hi = minmax ? minmax[1] : 1.0f;
    const float range = hi - lo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        // (mode 0: a NaN - NaN input, or max == min - propagates like the reference's fp32 result)
        if (MODE == 0) ((float*)out)[i] = norm01(in[i], lo, range, minmax != nullptr);
        else if (MODE == 1) ((unsigned char*)out)[i] = (unsigned char)(int)(255.0f * norm_clamp01(in[i], lo, range, minmax != nullptr));
        else ((uchar4*)out)[i] = u24_px(norm_clamp01(in[i], lo, range, minmax != nullptr), lossy, 0);
    }
}

// ---- per-image display tail (the per-frame loop of the reference's run_video.py:348-361 over a batch): segmented min/max, uint8 + histogram,
// equalization LUT, colormap. Every image of the batch gets its own min/max, histogram and LUT; nothing crosses from one image to another.
// Segmented min/max: grid (SEG_PARTS = MDPT_POST_SEG_PARTS, B); block (x, b) leaves the ordered {min, max} of its share of image b in parts[(b PARTS + x) 2 ..],
// the next kernel reduces the PARTS entries of its image (no atomics, no buffer to clear first). A NaN pins {0, ~0} (block_minmax_part).
// Every kernel here takes a PostRunTable (mdpt_kernels.h) by value: blockIdx.y = image b of the table, image j of run r; the uniform batch of
// the mdpt_post_*_seg / mdpt_post_colorize entry points is one run, images of different sizes (mdpt_post_*_images) one run each.
constexpr int SEG_PARTS = 64;

// image b of the launch -> its run r and its index j in that run (a block-uniform walk; the grid holds exactly the table's images)
__device__ __forceinline__ const PostRun& seg_image(const PostRunTable& t, int b, int& j) {
    int r = 0;
    j = b;
    while (r < t.n - 1 && j >= t.run[r].count) j -= t.run[r++].count;
    return t.run[r];
}

// image b's {min, max} from its SEG_PARTS partials; a block-wide call (its barrier also publishes what the caller wrote to LDS before), every
// thread gets the pair
__device__ __forceinline__ void seg_range(const unsigned* __restrict__ parts, int b, float& lo, float& hi) {
    __shared__ unsigned smm[2];
    if (threadIdx.x < SEG_PARTS) {
        unsigned mn = parts[((size_t)b * SEG_PARTS + threadIdx.x) * 2], mx = parts[((size_t)b * SEG_PARTS + threadIdx.x) * 2 + 1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
            mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        }
        if (threadIdx.x == 0) { smm[0] = mn; smm[1] = mx; }
    }
    __syncthreads();
    lo = ord2f(smm[0]);
    hi = ord2f(smm[1]);
}

// image b's fp64 {min, max - min} of its plane-removed values from its SEG_PARTS vparts (plane_minmax_kernel; a NaN partial pins NaN; one lane
// per partial); block-wide like seg_range
__device__ __forceinline__ void seg_vrange(const double* __restrict__ vparts, int b, double& vlo, double& vrange) {
    __shared__ double svr[2];
    if (threadIdx.x < SEG_PARTS) {
        double a = vparts[((size_t)b * SEG_PARTS + threadIdx.x) * 2], z = vparts[((size_t)b * SEG_PARTS + threadIdx.x) * 2 + 1];
        const bool any_nan = __any(a != a || z != z);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a = fmin(a, __shfl_xor(a, o));
            z = fmax(z, __shfl_xor(z, o));
        }
        if (threadIdx.x == 0) {
            svr[0] = any_nan ? NAN : a;
            svr[1] = any_nan ? NAN : z;
        }
    }
    __syncthreads();
    vlo = svr[0];
    vrange = svr[1] - svr[0];
}

// the block's LDS-private 256-bin histogram into hist[b, :]: one integer atomic per non-empty bin
__device__ __forceinline__ void hist_flush(const unsigned* bins, unsigned* __restrict__ hist, int b) {
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(hist + (size_t)b * 256 + threadIdx.x, bins[threadIdx.x]);
}

// Per image of the table, its min/max partials and (hist_clear != null) the zeroing of the [B,256] histogram the next kernel accumulates into.
// DISPLAY false - out == null: min/max of the input image. Otherwise scale_prediction of it to its oh x ow (bilinear_at: rounded to the input's
// dtype), stored as fp32 at its place of the packed out, min/max of that.
// DISPLAY true - remove_inf_tensor(scale_prediction(x)): the resize is an identity copy when the size does not change, as torch's upsample does (a
// bilinear tap on an inf neighbour would give NaN), +-inf -> 0, stored in the input's dtype; min/max of the result.
template <bool DISPLAY>
__global__ __launch_bounds__(256) void seg_scale_minmax_kernel(const PostRunTable t, int in_dt, void* __restrict__ out, unsigned* __restrict__ parts,
                                                               unsigned* __restrict__ hist_clear) {
    const int b = blockIdx.y;
    if (hist_clear && blockIdx.x == 0) hist_clear[(size_t)b * 256 + threadIdx.x] = 0u;
    int j;
    const PostRun& img = seg_image(t, b, j);
    const void* in = img.in;
    const int ih = img.ih, iw = img.iw, oh = img.oh, ow = img.ow;
    const bool store = DISPLAY || out != nullptr, resize = store && !(DISPLAY && ih == oh && iw == ow);
    const size_t n = store ? (size_t)oh * ow : (size_t)ih * iw;
    const size_t in_base = (size_t)j * ih * iw, out_base = img.off + (size_t)j * oh * ow;
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    float lo = INFINITY, hi = -INFINITY;
    bool saw_nan = false, any = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = resize ? bilinear_at(in, in_base, in_dt, ih, iw, sy, sx, (int)(i / ow), (int)(i % ow)) : ld_dt(in, in_base + i, in_dt);
        if (DISPLAY && isinf(v)) v = 0.0f;
        if (DISPLAY) st_dt(out, out_base + i, v, in_dt);
        else if (store) ((float*)out)[out_base + i] = v;
        any = true;
        saw_nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax_part(lo, hi, saw_nan, any, parts + ((size_t)b * SEG_PARTS + blockIdx.x) * 2);
}

// (255 * normalize_01(image b)).byte() with image b's own min/max (normalize_kernel<1>'s arithmetic), optionally 255 - x, and (hist != null) image
// b's 256-bin histogram of the result: LDS-private bins, flushed per block into hist[b, :]. Image b has ih x iw
// elements; its result goes to its place of the packed out.
__global__ __launch_bounds__(256) void seg_u8_hist_kernel(const PostRunTable t, int in_dt, const unsigned* __restrict__ parts, int reverse,
                                                          unsigned char* __restrict__ out, unsigned* __restrict__ hist) {
    const int b = blockIdx.y;
    int j;
    const PostRun& img = seg_image(t, b, j);
    const void* in = img.in;
    const size_t n = (size_t)img.ih * img.iw;
    __shared__ unsigned bins[256];
    bins[threadIdx.x] = 0u;
    float lo, hi;
    seg_range(parts, b, lo, hi);  // (publishes the zeroed bins too)
    const float range = hi - lo;
    const size_t base = (size_t)j * n, obase = img.off + (size_t)j * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        int q = (int)(255.0f * norm_clamp01(ld_dt(in, base + i, in_dt), lo, range, true));
        if (reverse) q = 255 - q;
        out[obase + i] = (unsigned char)q;
        if (hist) atomicAdd(&bins[q], 1u);
    }
    if (hist) hist_flush(bins, hist, b);
}

// 256-bin histogram per image of a uint8 batch, accumulated into hist[b, :] (same privatisation as above)
__global__ __launch_bounds__(256) void seg_hist_kernel(const unsigned char* __restrict__ in, size_t n, unsigned* __restrict__ hist) {
    const int b = blockIdx.y;
    __shared__ unsigned bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const size_t base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) atomicAdd(&bins[in[base + i]], 1u);
    hist_flush(bins, hist, b);
}

// Equalization LUT of image b (one block, thread t = entry t), the reference's histogram_equalization (demo_helpers/postprocess.py:107-145):
// bin_of == null: cv2.equalizeHist - first non-empty bin i; a single-valued image maps to i; else lut[i] = 0 and
//   lut[j] = saturate_cast<uchar>(float(hist[i+1] + ... + hist[j]) * (255.f / (total - hist[i]))), round half to even, in fp32.
// bin_of != null: the np.histogram(x, 1 + max - min, range=(min, max)) branch; bin_of[v] is the bin numpy puts value v in (-1: outside the range).
//   cdf over the bins, (cdf - cdf.min()) / float(max(cdf.max() - cdf.min(), 1)), uint8(255 * .) truncating, in fp64; lut = [0] * min, that, [255] * (255 - max).
__global__ __launch_bounds__(256) void equalize_lut_kernel(const unsigned* __restrict__ hist, const int* __restrict__ bin_of, int vmin, int vmax,
                                                           unsigned char* __restrict__ lut) {
    const int b = blockIdx.x, t = threadIdx.x;
    __shared__ unsigned h[256];
    __shared__ int sbin[256];
    __shared__ unsigned first;
    __shared__ unsigned long long total;
    h[t] = hist[(size_t)b * 256 + t];
    sbin[t] = bin_of ? bin_of[t] : 0;
    if (t == 0) { first = 256u; total = 0ull; }
    __syncthreads();
    unsigned char* out = lut + (size_t)b * 256;
    if (!bin_of) {
        if (h[t]) { atomicMin(&first, (unsigned)t); atomicAdd(&total, (unsigned long long)h[t]); }
        __syncthreads();
        const int i = (int)first;
        if (i > 255) { out[t] = 0; return; }  // (an empty image)
        if ((unsigned long long)h[i] == total) { out[t] = (unsigned char)i; return; }
        const float scale = __fdiv_rn(255.0f, (float)(total - h[i]));
        unsigned long long cum = 0;
        for (int k = i + 1; k <= t; ++k) cum += h[k];
        const float r = rintf(__fmul_rn((float)cum, scale));
        out[t] = t <= i ? 0 : (unsigned char)fminf(fmaxf(r, 0.0f), 255.0f);
        return;
    }
    if (t < vmin) { out[t] = 0; return; }
    if (t > vmax) { out[t] = 255; return; }
    const int nb = 1 + vmax - vmin, k = t - vmin;
    unsigned long long c0 = 0, ck = 0, cl = 0;  // cdf[0], cdf[k], cdf[nb - 1]
    for (int v = 0; v < 256; ++v) {
        const int bin = sbin[v];
        if (bin < 0) continue;
        c0 += bin <= 0 ? h[v] : 0u;
        ck += bin <= k ? h[v] : 0u;
        cl += bin <= nb - 1 ? h[v] : 0u;
    }
    const unsigned long long den = cl - c0 > 1ull ? cl - c0 : 1ull;
    const double norm = __ddiv_rn((double)(ck - c0), (double)den);
    out[t] = (unsigned char)(int)__dmul_rn(255.0, norm);
}

// out[b, i] = cmap[eq[b][x[b, i]]] as BGR (channels 3) or eq[b][x[b, i]] (channels 1); eq == null: identity, cmap == null: gray (cv2.cvtColor GRAY2BGR).
// Image b (ih x iw uint8 at its run's in) goes to its place of the packed out (element off + j ih iw, times channels).
__global__ __launch_bounds__(256) void colorize_kernel(const PostRunTable tab, const unsigned char* __restrict__ eq, const unsigned char* __restrict__ cmap,
                                                       int channels, unsigned char* __restrict__ out) {
    const int b = blockIdx.y, t = threadIdx.x;
    int j;
    const PostRun& img = seg_image(tab, b, j);
    const size_t n = (size_t)img.ih * img.iw;
    const unsigned char* in = (const unsigned char*)img.in + (size_t)j * n;
    __shared__ unsigned char seq[256];
    __shared__ unsigned char scm[256 * 3];
    seq[t] = eq ? eq[(size_t)b * 256 + t] : (unsigned char)t;
    for (int c = 0; c < 3; ++c) scm[t * 3 + c] = cmap ? cmap[t * 3 + c] : (unsigned char)t;
    __syncthreads();
    const size_t base = img.off + (size_t)j * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + t; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int e = seq[in[i]];
        if (channels == 1) {
            out[base + i] = (unsigned char)e;
        } else {
            unsigned char* o = out + (base + i) * 3;
            o[0] = scm[e * 3 + 0];
            o[1] = scm[e * 3 + 1];
            o[2] = scm[e * 3 + 2];
        }
    }
}

inline int grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// the x extent of a (blocks, images) grid
inline int grid_seg(size_t n) { return grid_for(n) < 256 ? grid_for(n) : 256; }

// images of a table (at most 65535, the grid's y) and the largest of their sizes (in: ih iw, out: oh ow); false: a malformed table
inline bool table_extent(const PostRunTable& t, int& B, size_t& max_in, size_t& max_out) {
    B = 0;
    max_in = max_out = 0;
    if (t.n <= 0 || t.n > MDPT_POST_RUNS) return false;
    for (int r = 0; r < t.n; ++r) {
        const PostRun& p = t.run[r];
        if (!p.in || p.ih <= 0 || p.iw <= 0 || p.oh <= 0 || p.ow <= 0 || p.count <= 0 || p.count > 65535 - B) return false;
        B += p.count;
        max_in = (size_t)p.ih * p.iw > max_in ? (size_t)p.ih * p.iw : max_in;
        max_out = (size_t)p.oh * p.ow > max_out ? (size_t)p.oh * p.ow : max_out;
    }
    return true;
}

// ---- still-image display tail (the reference's run_image.py:185-195, 323-343, 350-358) and the 3D viewer's edge alpha (run_3dviewer.py:455-505).
// Every kernel takes a uniform batch: image b is [h, w] at element b h w; grids are (parts, B) or one block per image. The prepared map comes from
// seg_scale_minmax_kernel<true> (its display form); the kernels after the plane fit take it with its statistics as one PlaneMap (mdpt_kernels.h). The arithmetic whose order the
// reference fixes (numpy's fp64, torch's per-op rounding) is written out with contraction off.

// normalize_01 of a map stored in dtype dt as torch evaluates it in that dtype: (x - min) and (max - min) each rounded to dt, then the quotient
__device__ __forceinline__ float norm01_dt(float x, float lo, float hi, int dt) {
#pragma clang fp contract(off)
    return round_dt(round_dt(x - lo, dt) / round_dt(hi - lo, dt), dt);
}

// numpy's plane image at pixel (x, y): -(d + nx x + ny y) / nz in fp64 (plane_fit.py generate_image_from_plane_normal); c = {nx, ny, nz, d}
__device__ __forceinline__ double plane_at(const double* c, int x, int y) {
#pragma clang fp contract(off)
    return -(c[3] + c[0] * (double)x + c[1] * (double)y) / c[2];
}

// d = -(nx mx + ny my + nz mz), numpy's order
__device__ __forceinline__ double plane_offset(const double* n, double mx, double my, double mz) {
#pragma clang fp contract(off)
    return -1.0 * (n[0] * mx + n[1] * my + n[2] * mz);
}

// torch's reflect padding index (no edge repeat) for offsets up to n - 1 past either end; clamped so that no index leaves the map
__device__ __forceinline__ int reflect_idx(int v, int n) {
    v = v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v);
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}

// K doubles summed over the block (256 threads); every thread gets the sums
template <int K>
__device__ __forceinline__ void block_sum_f64(double (&v)[K]) {
    __shared__ double s[4][K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) s[wave][k] = v[k];
    __syncthreads();
    for (int k = 0; k < K; ++k) v[k] = ((s[0][k] + s[1][k]) + s[2][k]) + s[3][k];
    __syncthreads();
}

// the eigenvector of the smallest eigenvalue of a symmetric 3x3 matrix, by cyclic Jacobi with a fixed number of sweeps (quadratic convergence:
// 3x3 in fp64 is converged after 4 or 5). A zero off-diagonal element is skipped, so a diagonal matrix (a constant map: z row and column zero)
// keeps its axes. Ties go to the later axis, so a degenerate fit prefers the z normal (a constant plane) over an x / y one.
__device__ void jacobi3_min_eigvec(double a[3][3], double n[3]) {
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 10; ++sweep) {
        for (int k = 0; k < 3; ++k) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int r = 0; r < 3; ++r) {
                const double arp = a[r][p], arq = a[r][q];
                a[r][p] = c * arp - s * arq;
                a[r][q] = s * arp + c * arq;
            }
            for (int r = 0; r < 3; ++r) {
                const double apr = a[p][r], aqr = a[q][r];
                a[p][r] = c * apr - s * aqr;
                a[q][r] = s * apr + c * aqr;
            }
            for (int r = 0; r < 3; ++r) {
                const double vrp = v[r][p], vrq = v[r][q];
                v[r][p] = c * vrp - s * vrq;
                v[r][q] = s * vrp + c * vrq;
            }
        }
    }
    int m = 0;
    for (int k = 1; k < 3; ++k)
        if (a[k][k] <= a[m][m]) m = k;
    for (int r = 0; r < 3; ++r) n[r] = v[r][m];
}

// plane of best fit of image b (one block per image; plane_fit.py get_xyz_samples / find_plane_normal / generate_image_from_plane_normal):
// z at the N sample points (parts != null: of normalize_01(image b) in dtype dt), the known x / y means (w-1)/2, (h-1)/2 and the sample z mean,
// the 3x3 Gram matrix of the centred samples in fp64, its smallest eigenvector (numpy's smallest right singular vector, up to sign) -> coef[b] =
// {nx, ny, nz, d}, d = -(nx mx + ny my + nz mz). Sample points are clamped into the map.
__global__ __launch_bounds__(256) void plane_fit_kernel(const void* __restrict__ in, int dt, int h, int w, const unsigned* __restrict__ parts,
                                                        const int* __restrict__ xy, int N, size_t xy_stride, double* __restrict__ coef) {
    const int b = blockIdx.x;
    float lo = 0.0f, hi = 1.0f;
    if (parts) seg_range(parts, b, lo, hi);
    const int* pts = xy + (size_t)b * xy_stride;
    const size_t base = (size_t)b * h * w;
    auto z_at = [&](int k, int& x, int& y) -> double {
        x = min(max(pts[2 * k], 0), w - 1);
        y = min(max(pts[2 * k + 1], 0), h - 1);
        const float z = ld_dt(in, base + (size_t)y * w + x, dt);
        return (double)(parts ? norm01_dt(z, lo, hi, dt) : z);
    };
    double zs[1] = {0.0};
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        int x, y;
        zs[0] += z_at(k, x, y);
    }
    block_sum_f64<1>(zs);
    const double mx = (w - 1) * 0.5, my = (h - 1) * 0.5, mz = zs[0] / N;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // xx xy xz yy yz zz
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        int x, y;
        const double cz = z_at(k, x, y) - mz, cx = x - mx, cy = y - my;
        g[0] += cx * cx; g[1] += cx * cy; g[2] += cx * cz;
        g[3] += cy * cy; g[4] += cy * cz; g[5] += cz * cz;
    }
    block_sum_f64<6>(g);
    if (threadIdx.x != 0) return;
    double a[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}}, nrm[3];
    jacobi3_min_eigvec(a, nrm);
    double* c = coef + (size_t)b * 4;
    c[0] = nrm[0];
    c[1] = nrm[1];
    c[2] = nrm[2];
    c[3] = plane_offset(nrm, mx, my, mz);
}

// the plane image of coef[b], rounded to fp32
__global__ __launch_bounds__(256) void plane_eval_kernel(const double* __restrict__ coef, int h, int w, float* __restrict__ out) {
    const int b = blockIdx.y;
    const double* c = coef + (size_t)b * 4;
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[(size_t)b * n + i] = (float)plane_at(c, (int)(i % w), (int)(i / w));
}

// v = dn - factor * plane in fp64 at pixel (x, y) of the map at element `base` (numpy: the fp32 map minus the fp64 plane), dn = normalize_01(map)
// in dtype dt; c = the map's plane
__device__ __forceinline__ double plane_removed(const void* map, size_t base, int dt, int w, int x, int y, float lo, float hi, const double* c,
                                                double factor) {
#pragma clang fp contract(off)
    return (double)norm01_dt(ld_dt(map, base + (size_t)y * w + x, dt), lo, hi, dt) - plane_at(c, x, y) * factor;
}

// n = normalize_01(v) in fp64 with v's {min, max - min}: the value the threshold display windows and the depth masks compare
__device__ __forceinline__ double plane_norm(const void* map, size_t base, int dt, int w, int x, int y, float lo, float hi, const double* c, double factor,
                                             double vlo, double vrange) {
#pragma clang fp contract(off)
    return (plane_removed(map, base, dt, w, x, y, lo, hi, c, factor) - vlo) / vrange;
}

// image b's plane in registers (the pointers of a PlaneMap carry no __restrict__: read through them after a store or a barrier, the plane is
// loaded again, per lane)
struct Plane { double c[4]; };
__device__ __forceinline__ Plane plane_of(const double* coef, int b) {
    const double* c = coef + (size_t)b * 4;
    return Plane{{c[0], c[1], c[2], c[3]}};
}

// per-image fp64 {min, max} partials of v: vparts[b][part] (block_minmax_f64)
__global__ __launch_bounds__(256) void plane_minmax_kernel(const PlaneMap m, double* __restrict__ vparts) {
    const int b = blockIdx.y;
    const Plane plane = plane_of(m.coef, b);
    float lo, hi;
    seg_range(m.parts, b, lo, hi);
    const size_t n = (size_t)m.h * m.w, base = (size_t)b * n;
    double vlo = INFINITY, vhi = -INFINITY;
    bool saw_nan = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = plane_removed(m.in, base, m.dt, m.w, (int)(i % m.w), (int)(i / m.w), lo, hi, plane.c, m.factor);
        saw_nan |= v != v;
        vlo = fmin(vlo, v);
        vhi = fmax(vhi, v);
    }
    block_minmax_f64(vlo, vhi, saw_nan, vparts + ((size_t)b * SEG_PARTS + blockIdx.x) * 2);
}

// t = clip((n - tmin) / delta, 0, 1) in fp64 (run_image.py:331-333, 355-356). Mode 1 (MDPT_POST_U8): round-half-even(255 t) -> uint8
// (a NaN -> 0), and (hist != null) its 256-bin histogram into hist[b]; mode 0 (MDPT_POST_F32): t, or 1 - t with reverse, -> fp32.
template <int MODE>
__global__ __launch_bounds__(256) void threshold_kernel(const PlaneMap m, double tmin, double delta, int reverse, void* __restrict__ out,
                                                        unsigned* __restrict__ hist) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const Plane plane = plane_of(m.coef, b);
    __shared__ unsigned bins[256];
    bins[threadIdx.x] = 0u;
    float lo, hi;
    double vlo, vrange;
    seg_range(m.parts, b, lo, hi);  // (publishes the zeroed bins too)
    seg_vrange(m.vparts, b, vlo, vrange);
    const size_t n = (size_t)m.h * m.w, base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = plane_norm(m.in, base, m.dt, m.w, (int)(i % m.w), (int)(i / m.w), lo, hi, plane.c, m.factor, vlo, vrange);
        double t = (v - tmin) / delta;
        t = t != t ? t : (t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t));
        if (MODE == 1) {
            const int q = t == t ? (int)rint(255.0 * t) : 0;
            ((unsigned char*)out)[base + i] = (unsigned char)q;
            if (hist) atomicAdd(&bins[q], 1u);
        } else {
            ((float*)out)[base + i] = (float)(reverse ? 1.0 - t : t);
        }
    }
    if (MODE == 1 && hist) hist_flush(bins, hist, b);
}

// ---- edge alpha (run_3dviewer.py:455-505): blur = conv(x, gauss, reflect pad p), (dx, dy) = conv(blur, sobel, reflect pad 1), mag = sqrt(dx^2 + dy^2)
constexpr int EDGE_TILE = 16;
constexpr int EDGE_MAX_PAD = 7;
struct EdgeBlur { float w[(2 * EDGE_MAX_PAD + 1) * (2 * EDGE_MAX_PAD + 1)]; int ksize; };

// one 16x16 tile of image b per block: the input tile with a (1 + p)-pixel halo in LDS (each LDS element the input at the reflected coordinate),
// the blurred tile with a 1-pixel halo (each at the reflected blurred coordinate, so the Sobel halo reflects on the blurred map as torch pads it),
// then the Sobel magnitude -> mag[b] (blur and Sobel in fp64: the Sobel differences neighbouring blurred values of up to ~k^2 times the map, which
// leaves fp32 sums a few 1e-3 of a byte off at 1080p; fp64 keeps the bytes off the reference's only at rounding ties), and the image's max through an atomicMax on the bits of the (non-negative) fp32 magnitudes. parts != null:
// the map is normalize_01(x) in fp32 first (norm01).
__global__ __launch_bounds__(256) void edge_mag_kernel(const float* __restrict__ in, int h, int w, const unsigned* __restrict__ parts, const EdgeBlur blur,
                                                       float* __restrict__ mag, unsigned* __restrict__ mag_max) {
    constexpr int BT = EDGE_TILE + 2, RMAX = BT + 2 * EDGE_MAX_PAD;
    __shared__ float sx[RMAX * RMAX];
    __shared__ double sb[BT * BT];
    const int b = blockIdx.z, t = threadIdx.x;
    float lo = 0.0f, hi = 1.0f;
    if (parts) seg_range(parts, b, lo, hi);
    const float range = hi - lo;
    const int ks = blur.ksize, p = ks / 2, R = BT + 2 * p;
    const int y0 = blockIdx.y * EDGE_TILE, x0 = blockIdx.x * EDGE_TILE;
    const float* img = in + (size_t)b * h * w;
    for (int e = t; e < R * R; e += 256) {
        const int vy = y0 - 1 - p + e / R, vx = x0 - 1 - p + e % R;
        const float v = img[(size_t)reflect_idx(vy, h) * w + reflect_idx(vx, w)];
        sx[e] = norm01(v, lo, range, parts != nullptr);
    }
    __syncthreads();
    for (int e = t; e < BT * BT; e += 256) {
        const int gy = y0 - 1 + e / BT, gx = x0 - 1 + e % BT;
        double acc = 0.0;
        if (gy <= h && gx <= w) {  // (rows / columns past h / w are no Sobel neighbour of a pixel of the map)
            const int ry = reflect_idx(gy, h) - y0 + 1, rx = reflect_idx(gx, w) - x0 + 1;  // in [0, BT): see the comment above
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx) acc = fma((double)blur.w[ky * ks + kx], (double)sx[(ry + ky) * R + rx + kx], acc);
        }
        sb[e] = acc;
    }
    __syncthreads();
    const int ty = t / EDGE_TILE, tx = t % EDGE_TILE, y = y0 + ty, x = x0 + tx;
    float m = 0.0f;
    if (y < h && x < w) {
        const double* s = sb + ty * BT + tx;  // s[i BT + j] = blurred at (reflect(y + i - 1), reflect(x + j - 1))
        const double dy = 3.0 * (s[0] - s[2 * BT]) + 10.0 * (s[1] - s[2 * BT + 1]) + 3.0 * (s[2] - s[2 * BT + 2]);
        const double dx = 3.0 * (s[0] - s[2]) + 10.0 * (s[BT] - s[BT + 2]) + 3.0 * (s[2 * BT] - s[2 * BT + 2]);
        m = (float)sqrt(dx * dx + dy * dy);
        mag[(size_t)b * h * w + (size_t)y * w + x] = m;
    }
    unsigned bits = m != m ? 0x7fffffffu : __float_as_uint(m);  // a NaN wins the max (torch's max propagates it)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o));
    if ((t & 63) == 0) atomicMax(mag_max + b, bits);
}

// ~round(255 mag / max) (torch: 255 * mag, then / max, round half to even, .byte(), bitwise_not); max 0 (a flat map) or NaN -> 0 before the not: 255
__device__ __forceinline__ unsigned char edge_byte(float m, float mx) {
#pragma clang fp contract(off)
    const float r = rintf((255.0f * m) / mx);
    return (unsigned char)(255 - (r == r ? (int)fminf(fmaxf(r, 0.0f), 255.0f) : 0));
}

__global__ __launch_bounds__(256) void edge_mask_kernel(const float* __restrict__ mag, const unsigned* __restrict__ mag_max, size_t n,
                                                        unsigned char* __restrict__ out) {
    const int b = blockIdx.y;
    const float mx = __uint_as_float(mag_max[b]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[(size_t)b * n + i] = edge_byte(mag[(size_t)b * n + i], mx);
}

// pack_depth_u24 per image (norm_clamp01 with image b's min/max from parts; parts == null: metric, as is; then u24_px) with the alpha byte
// in the same pass: the edge byte of mag (mag != null), the caller's mask (mask != null; per image or one for all), or 0
__global__ __launch_bounds__(256) void pack_u24_kernel(const float* __restrict__ in, size_t n, const unsigned* __restrict__ parts, int lossy,
                                                       const float* __restrict__ mag, const unsigned* __restrict__ mag_max,
                                                       const unsigned char* __restrict__ mask, size_t mask_stride, uchar4* __restrict__ out) {
    const int b = blockIdx.y;
    float lo = 0.0f, hi = 1.0f;
    if (parts) seg_range(parts, b, lo, hi);
    const float range = hi - lo;
    const float mx = mag ? __uint_as_float(mag_max[b]) : 0.0f;
    const size_t base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned char alpha = mag ? edge_byte(mag[base + i], mx) : (mask ? mask[(size_t)b * mask_stride + i] : (unsigned char)0);
        out[base + i] = u24_px(norm_clamp01(in[base + i], lo, range, parts != nullptr), lossy, alpha);
    }
}

// ---- depth masking (the reference's experiments/depth_masking.py: display :189-199, 314-332; save :341-361). n = normalize_01(normalize_01(x) - f plane)
// in fp64 (plane_norm), mask = 255 where tmin <= n <= tmax (a NaN compares false: 0), 255 - mask with invert.
// cv2.resize(INTER_LINEAR) is restated per axis: p = float((d + 0.5) scale - 0.5) with scale = 1 / (out / in) in fp64 (cv2's own form), s = floor(p),
// a = p - s in fp32; s < 0 -> s = 0, a = 0; s >= in - 1 -> s = in - 1, a = 0. CV_64F: weights (1 - a, a) in fp32, sums in fp64, rows first, then
// across them. CV_8U: weights round(2048 w), integer sums, (v + 2^21) >> 22: cv2's scalar fixed-point path (its SIMD / IPP paths may round 1 off).
constexpr int MASK_PX = 4;  // consecutive pixels per thread: 12 BGR bytes in (one dwordx3 load), 16 BGRA + 4 mask bytes out (dwordx4 + dword stores)

struct CvTap { int s0, s1; float a; };
struct alignas(4) Bytes12 { unsigned w0, w1, w2; };  // (not uint3: a 3-vector may be accessed as 16 bytes)

__device__ __forceinline__ CvTap cv_tap(int d, double scale, int n) {
#pragma clang fp contract(off)
    const float p = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(p);
    float a = p - (float)s;
    if (s < 0) { s = 0; a = 0.0f; }
    if (s >= n - 1) { s = n - 1; a = 0.0f; }
    return CvTap{s, s + (a != 0.0f), a};  // (a != 0 only where s + 1 < n)
}

// v0 (1 - a) + v1 a in fp64 with fp32 weights; a == 0: v0 (cv2's one-tap border columns)
__device__ __forceinline__ double lerp_cv64(double v0, double v1, float a) {
#pragma clang fp contract(off)
    return a == 0.0f ? v0 : v0 * (double)(1.0f - a) + v1 * (double)a;
}

__device__ __forceinline__ unsigned mask_byte(double n, double tmin, double tmax, int invert) {
    return ((n >= tmin && n <= tmax) != (invert != 0)) ? 255u : 0u;
}

// cv2.resize of a BGR uint8 image at the output pixel of taps (tx, ty), the scalar fixed-point formula -> o[0..2]
__device__ __forceinline__ void bgr_lerp_u8(const unsigned char* __restrict__ src, int iw, CvTap tx, CvTap ty, unsigned char* o) {
    const int ax1 = (int)rintf(tx.a * 2048.0f), ax0 = (int)rintf((1.0f - tx.a) * 2048.0f);
    const int ay1 = (int)rintf(ty.a * 2048.0f), ay0 = (int)rintf((1.0f - ty.a) * 2048.0f);
    const unsigned char* r0 = src + (size_t)ty.s0 * iw * 3;
    const unsigned char* r1 = src + (size_t)ty.s1 * iw * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int h0 = r0[tx.s0 * 3 + ch] * ax0 + r0[tx.s1 * 3 + ch] * ax1;
        const int h1 = r1[tx.s0 * 3 + ch] * ax0 + r1[tx.s1 * 3 + ch] * ax1;
        const int v = (h0 * ay0 + h1 * ay1 + (1 << 21)) >> 22;
        o[ch] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

// display (uniform batch, map b at the display size h x w, photo b ih x iw): the mask of n, and the composite - cv2.resize of the photo where the
// mask is 255, CheckerPattern() where it is 0: A = 169 where ((y - t) mod 64 < 32) == ((x - l) mod 64 < 32), else B = 214, t = max(h - 64, 0) / 2,
// l = max(w - 64, 0) / 2 (toadui/helpers/checker_pattern.py: 32-px tiles, BORDER_WRAP padding, cropped). MASK_PX pixels of the flat image per thread.
__global__ __launch_bounds__(256) void mask_display_kernel(const PlaneMap m, double tmin, double tmax, int invert, const unsigned char* __restrict__ img,
                                                           int ih, int iw, unsigned char* __restrict__ mask_out, unsigned char* __restrict__ comp_out) {
    const int b = blockIdx.y;
    const Plane plane = plane_of(m.coef, b);
    const int dt = m.dt, h = m.h, w = m.w;
    const void* map = m.in;
    const double factor = m.factor;
    float lo, hi;
    double vlo, vrange;
    seg_range(m.parts, b, lo, hi);
    seg_vrange(m.vparts, b, vlo, vrange);
    const size_t n = (size_t)h * w, base = (size_t)b * n;
    const unsigned char* src = img + (size_t)b * ih * iw * 3;
    const double scale_x = 1.0 / ((double)w / (double)iw), scale_y = 1.0 / ((double)h / (double)ih);
    const int top = max(h - 64, 0) / 2, left = max(w - 64, 0) / 2;
    for (size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * MASK_PX; p0 < n; p0 += (size_t)gridDim.x * blockDim.x * MASK_PX) {
        const int cnt = n - p0 < (size_t)MASK_PX ? (int)(n - p0) : MASK_PX;
        int y = (int)(p0 / w), x = (int)(p0 % w);
        CvTap ty = cv_tap(y, scale_y, ih);
        unsigned mword = 0u;
        unsigned char px[MASK_PX * 3];
#pragma unroll
        for (int k = 0; k < MASK_PX; ++k) {
            px[k * 3] = px[k * 3 + 1] = px[k * 3 + 2] = 0;
            if (k >= cnt) continue;
            const unsigned m = mask_byte(plane_norm(map, base, dt, w, x, y, lo, hi, plane.c, factor, vlo, vrange), tmin, tmax, invert);
            mword |= m << (8 * k);
            if (m) {
                bgr_lerp_u8(src, iw, cv_tap(x, scale_x, iw), ty, px + k * 3);
            } else {
                const unsigned char v = (((y - top) & 63) < 32) == (((x - left) & 63) < 32) ? 169 : 214;
                px[k * 3] = px[k * 3 + 1] = px[k * 3 + 2] = v;
            }
            if (++x == w) {
                x = 0;
                ty = cv_tap(++y, scale_y, ih);
            }
        }
        unsigned char* mo = mask_out + base + p0;
        unsigned char* co = comp_out + (base + p0) * 3;
        if (cnt == MASK_PX && ((uintptr_t)mo & 3) == 0) {
            *(unsigned*)mo = mword;
        } else {
            for (int k = 0; k < cnt; ++k) mo[k] = (unsigned char)(mword >> (8 * k));
        }
        if (cnt == MASK_PX && ((uintptr_t)co & 3) == 0) {
            unsigned wd[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                wd[q] = (unsigned)px[4 * q] | (unsigned)px[4 * q + 1] << 8 | (unsigned)px[4 * q + 2] << 16 | (unsigned)px[4 * q + 3] << 24;
            *(Bytes12*)co = Bytes12{wd[0], wd[1], wd[2]};
        } else {
            for (int k = 0; k < cnt * 3; ++k) co[k] = px[k];
        }
    }
}

// cutout (one photo per blockIdx.y, any sizes): s = cv2.resize(n, (iw, ih)) in fp64 from the 2 x 2 map taps evaluated on the fly, the mask of s,
// BGRA = (BGR AND mask, mask), both at the photo's packed offset. The taps of consecutive pixels are shared where they repeat (an enlargement).
__global__ __launch_bounds__(256) void mask_cutout_kernel(const MaskTable t, double factor, double tmin, double tmax, int invert,
                                                          unsigned char* __restrict__ out_bgra, unsigned char* __restrict__ out_mask) {
    const MaskImage& im = t.im[blockIdx.y];
    float lo, hi;
    double vlo, vrange;
    seg_range(im.parts, 0, lo, hi);
    seg_vrange(im.vparts, 0, vlo, vrange);
    const int dt = t.dt, h = im.h, w = im.w, ih = im.ih, iw = im.iw;
    const void* map = im.map;
    const double* c = im.coef;
    const unsigned char* img = im.img;
    const double scale_x = 1.0 / ((double)iw / (double)w), scale_y = 1.0 / ((double)ih / (double)h);
    const size_t n = (size_t)ih * iw;
    unsigned char* bgra = out_bgra + im.off * 4;
    unsigned char* msk = out_mask + im.off;
    for (size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * MASK_PX; p0 < n; p0 += (size_t)gridDim.x * blockDim.x * MASK_PX) {
        const int cnt = n - p0 < (size_t)MASK_PX ? (int)(n - p0) : MASK_PX;
        const unsigned char* in = img + p0 * 3;
        unsigned wd[3] = {0u, 0u, 0u};
        if (cnt == MASK_PX && ((uintptr_t)in & 3) == 0) {
            const Bytes12 v = *(const Bytes12*)in;
            wd[0] = v.w0;
            wd[1] = v.w1;
            wd[2] = v.w2;
        } else {
            for (int k = 0; k < cnt * 3; ++k) wd[k >> 2] |= (unsigned)in[k] << (8 * (k & 3));
        }
        int y = (int)(p0 / iw), x = (int)(p0 % iw);
        CvTap ty = cv_tap(y, scale_y, h);
        int key_x = -1, key_y = -1;
        double n00 = 0.0, n01 = 0.0, n10 = 0.0, n11 = 0.0;
        unsigned mword = 0u, px[MASK_PX];
#pragma unroll
        for (int k = 0; k < MASK_PX; ++k) {
            px[k] = 0u;
            if (k >= cnt) continue;
            const CvTap tx = cv_tap(x, scale_x, w);
            const bool bx = tx.s1 != tx.s0, by = ty.s1 != ty.s0;
            if (2 * tx.s0 + bx != key_x || 2 * ty.s0 + by != key_y) {
                key_x = 2 * tx.s0 + bx;
                key_y = 2 * ty.s0 + by;
                n00 = plane_norm(map, 0, dt, w, tx.s0, ty.s0, lo, hi, c, factor, vlo, vrange);
                n01 = bx ? plane_norm(map, 0, dt, w, tx.s1, ty.s0, lo, hi, c, factor, vlo, vrange) : n00;
                n10 = by ? plane_norm(map, 0, dt, w, tx.s0, ty.s1, lo, hi, c, factor, vlo, vrange) : n00;
                n11 = bx && by ? plane_norm(map, 0, dt, w, tx.s1, ty.s1, lo, hi, c, factor, vlo, vrange) : (bx ? n01 : n10);
            }
            const double s = lerp_cv64(lerp_cv64(n00, n01, tx.a), lerp_cv64(n10, n11, tx.a), ty.a);
            const unsigned m = mask_byte(s, tmin, tmax, invert);
            mword |= m << (8 * k);
            // BGR of pixel k: bytes 3k .. 3k + 2 of the loaded words
            unsigned bgr = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) bgr |= ((wd[(3 * k + ch) >> 2] >> (8 * ((3 * k + ch) & 3))) & 255u) << (8 * ch);
            px[k] = (m ? bgr : 0u) | m << 24;
            if (++x == iw) {
                x = 0;
                ty = cv_tap(++y, scale_y, h);
            }
        }
        unsigned char* bo = bgra + p0 * 4;
        unsigned char* mo = msk + p0;
        if (cnt == MASK_PX && ((uintptr_t)bo & 15) == 0) {
            *(uint4*)bo = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
            for (int k = 0; k < cnt; ++k) *(unsigned*)(bo + 4 * k) = px[k];  // (the BGRA output is 4-byte aligned: checked by the entry point)
        }
        if (cnt == MASK_PX && ((uintptr_t)mo & 3) == 0) {
            *(unsigned*)mo = mword;
        } else {
            for (int k = 0; k < cnt; ++k) mo[k] = (unsigned char)(mword >> (8 * k));
        }
    }
}

// Block norm tiles (experiments/block_norm_visualization.py:137-147 BlockData.__init__, then the nearest-neighbour enlargement of :207-233):
// one workgroup per (map, image) of the table - maps are token grids, a few thousand floats at most. Pass 1: the map's own min / max (a NaN
// pins both to NaN, as numpy's min / max do) -> minmax[(map, image)] = {min, max}. Pass 2, in fp32 as numpy computes it, one IEEE operation per
// step and nothing contracted: u8 = rint(((n - min) / (max - min)) * 255), rint rounding halves to even like np.round; written at the oh x ow
// tile's pixels (y, x) from map cell (y / fy, x / fx) for the whole factors fy = oh / ih, fx = ow / iw. A value that is not a number (a
// constant map's 0 / 0, a map holding a NaN: every value of it) gives 0, where the reference's uint8 conversion is undefined.
__global__ __launch_bounds__(256) void block_norm_tiles_kernel(const PostRunTable t, unsigned char* __restrict__ out, float* __restrict__ minmax) {
    const int b = blockIdx.x;
    int j;
    const PostRun& img = seg_image(t, b, j);
    const int ih = img.ih, iw = img.iw, oh = img.oh, ow = img.ow;
    const int n = ih * iw;
    const float* in = (const float*)img.in + (size_t)j * n;
    float lo = INFINITY, hi = -INFINITY;
    bool saw_nan = false;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = in[i];
        saw_nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    __shared__ unsigned smm[2];
    block_minmax_part(lo, hi, saw_nan, true, smm);  // (n >= 1: thread 0 always holds a value)
    __syncthreads();
    const float mn = ord2f(smm[0]), mx = ord2f(smm[1]);
    if (threadIdx.x == 0) {
        minmax[2 * (size_t)b] = mn;
        minmax[2 * (size_t)b + 1] = mx;
    }
    const float range = __fsub_rn(mx, mn);
    const int fy = oh / ih, fx = ow / iw;
    unsigned char* dst = out + img.off + (size_t)j * oh * ow;
    for (int i = threadIdx.x; i < oh * ow; i += 256) {
        const int y = i / ow, x = i - y * ow;
        const float v = __fmul_rn(__fdiv_rn(__fsub_rn(in[(y / fy) * iw + x / fx], mn), range), 255.0f);
        dst[i] = v == v ? (unsigned char)(int)rintf(v) : (unsigned char)0;
    }
}

// ---- depth-to-mesh: the client half of the reference's 3D viewer ("Save 3D Model"), which is JavaScript on the CPU there - 3dviewer/shaders.js:163-264
// run_vertex_shader_cpu (the unprojection of every plane vertex through a bilinear sample of the 24-bit depth + alpha frame), mesh.js:170-254
// _make_plane_mesh (the grid and its two triangles per cell) and mesh.js:330-371 filter_mesh_vertices (drop the vertices below the edge threshold
// and every face that touches one, keep the order, renumber). Positions, weights, the alpha comparison and the depth arithmetic are fp64 as in
// JavaScript, nothing contracted, rounded to fp32 once on output. One deviation: the 24-bit depth value is interpolated, where the JavaScript
// interpolates its three bytes separately and truncates each (garbage across a byte carry).
//
// The compaction is an order-preserving multi-launch scan, bit-deterministic: (1) alpha -> a keep flag per vertex and the kept count of every
// 256-vertex block, (2) the kept faces of every 256-cell block from the flags, (3) ONE workgroup per image and list scans the block counts in
// 256-wide chunks with a running carry (no workgroup ever waits for another), (4) the kept vertices are computed and written at block offset +
// rank in block (64-bit ballots and popcounts, wave totals through LDS) and the flag plane becomes the old -> new index map, (5) the kept faces are
// written through that map. A launch boundary separates every producer from its consumers.
//
// R is the type of the arithmetic: double. A -DMDPT_DEBUG_SWITCHES build also holds the float instances, chosen by MDPT_MESH_FP32=1, so that
// tools/probes/gpu_mesh.py can time what the fp64 costs; they do not meet the fp64 specification and no release build has them.

// the exclusive rank of this thread's k (0, 1 or 2) items among the block's 256 threads, in thread order, and the block's total
__device__ __forceinline__ unsigned block_rank(int k, unsigned& total) {
    const unsigned long long m1 = __ballot(k >= 1), m2 = __ballot(k >= 2);
    const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1;
    __shared__ unsigned swave[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) swave[wave] = __popcll(m1) + __popcll(m2);
    __syncthreads();
    unsigned rank = __popcll(m1 & below) + __popcll(m2 & below);
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) rank += swave[w];
        total += swave[w];
    }
    __syncthreads();
    return rank;
}

template <typename R>
__device__ __forceinline__ void mesh_vertex_xy(const MeshJob& m, size_t i, R& x, R& y) {
#pragma clang fp contract(off)
    if (m.vertex_xy) {
        x = (R)m.vertex_xy[2 * i];
        y = (R)m.vertex_xy[2 * i + 1];
        return;
    }
    const int r = (int)(i / (size_t)m.nx), c = (int)(i - (size_t)r * m.nx);  // mesh.js:198-200
    x = (R)c * (R)m.x_step - (R)1;
    y = (R)1 - (R)r * (R)m.y_step;
}

// shaders.js:212-252 in the viewer's vertically flipped frame (index.html:1067-1070: flipped row j = frame row H - 1 - j): the four taps as pixel
// indices of one frame and the two weights. A coordinate that is not a number clamps to 1 (fmin(1, NaN) = 1), so such a position samples the last
// column / row of the flipped frame with weight 0 on the neighbour; nothing leaves the frame.
template <typename R>
struct MeshTaps { size_t tl, tr, bl, br; R tx, ty; };

template <typename R>
__device__ __forceinline__ MeshTaps<R> mesh_taps(R x, R y, int H, int W) {
#pragma clang fp contract(off)
    const R u = (x + (R)1) * (R)0.5, v = (y + (R)1) * (R)0.5;
    const R xr = fmax((R)0, fmin((R)1, u)) * (R)(W - 1), yr = fmax((R)0, fmin((R)1, v)) * (R)(H - 1);
    const int x1 = (int)floor(xr), y1 = (int)floor(yr);
    const int x2 = x1 + 1 < W - 1 ? x1 + 1 : W - 1, y2 = y1 + 1 < H - 1 ? y1 + 1 : H - 1;
    const size_t top = (size_t)(H - 1 - y1) * W, bot = (size_t)(H - 1 - y2) * W;
    return MeshTaps<R>{top + x1, top + x2, bot + x1, bot + x2, xr - (R)x1, yr - (R)y1};
}

template <typename R>
__device__ __forceinline__ R mesh_lerp(const MeshTaps<R>& t, R tl, R tr, R bl, R br) {
#pragma clang fp contract(off)
    const R l = ((R)1 - t.ty) * tl + t.ty * bl, r = ((R)1 - t.ty) * tr + t.ty * br;  // shaders.js:232-234
    return ((R)1 - t.tx) * l + t.tx * r;
}

// (1) shaders.js:198: a vertex is kept if its interpolated alpha byte reaches edge_threshold * 255
template <typename R>
__global__ __launch_bounds__(256) void mesh_flag_kernel(const MeshJob m) {
    const int b = blockIdx.y;
    const size_t nv = (size_t)m.nx * m.ny, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < nv) {
        R x, y;
        mesh_vertex_xy(m, i, x, y);
        const MeshTaps<R> t = mesh_taps(x, y, m.H, m.W);
        const unsigned* f = m.frames + (size_t)b * m.H * m.W;
        keep = mesh_lerp(t, (R)(f[t.tl] >> 24), (R)(f[t.tr] >> 24), (R)(f[t.bl] >> 24), (R)(f[t.br] >> 24)) >= (R)m.alpha_min;
        m.vmap[(size_t)b * nv + i] = keep ? 0 : -1;
    }
    unsigned total;
    block_rank(keep ? 1 : 0, total);
    if (threadIdx.x == 0) m.vcnt[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// mesh.js:218-228 for grid cell k of image b: the map entries of its corners {v, v + 1, v + nx, v + nx + 1} and which of its two triangles
// [v, v + nx, v + nx + 1], [v, v + nx + 1, v + 1] have all their vertices kept (bit 0, bit 1)
__device__ __forceinline__ int mesh_cell(const MeshJob& m, int b, size_t k, int (&e)[4]) {
    const size_t cols = (size_t)m.nx - 1, r = k / cols, c = k - r * cols;
    const int* v = m.vmap + (size_t)b * m.nx * m.ny + c + r * m.nx;
    e[0] = v[0];
    e[1] = v[1];
    e[2] = v[m.nx];
    e[3] = v[(size_t)m.nx + 1];
    const bool diag = e[0] >= 0 && e[3] >= 0;
    return (diag && e[2] >= 0 ? 1 : 0) | (diag && e[1] >= 0 ? 2 : 0);
}

// (2) the kept faces of every block of 256 cells
__global__ __launch_bounds__(256) void mesh_face_count_kernel(const MeshJob m) {
    const size_t cells = ((size_t)m.nx - 1) * ((size_t)m.ny - 1), k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int e[4];
    const int tri = k < cells ? mesh_cell(m, blockIdx.y, k, e) : 0;
    unsigned total;
    block_rank((tri & 1) + (tri >> 1), total);
    if (threadIdx.x == 0) m.fcnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// (3) block counts -> exclusive offsets in place and the image's total -> counts; blockIdx.x = the list (0 vertices, 1 faces), blockIdx.y = image.
// The vertex list's workgroup also resets the image's running bounds.
__global__ __launch_bounds__(256) void mesh_scan_kernel(const MeshJob m, unsigned nbv, unsigned nbf, int* __restrict__ counts) {
    const int b = blockIdx.y, which = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n = which ? nbf : nbv;
    unsigned* cnt = which ? m.fcnt + (size_t)b * nbf : m.vcnt + (size_t)b * nbv;
    __shared__ unsigned swave[4];
    unsigned carry = 0;
    for (unsigned base = 0; base < n; base += 256) {
        const unsigned i = base + threadIdx.x, v = i < n ? cnt[i] : 0;
        unsigned inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) swave[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += swave[w];
            total += swave[w];
        }
        if (i < n) cnt[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[2 * (size_t)b + which] = (int)carry;
        if (m.points) counts[2 * (size_t)b + 1] = (int)carry;  // one "face" [i] per kept vertex
    }
    if (which == 0 && threadIdx.x < 6) m.bord[6 * (size_t)b + threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

// (4) shaders.js:185-205 for the kept vertices, written at their new index; the flag plane becomes the old -> new map; the image's bounds
// (save_gltf.js:16-25, of the fp32 values as written: rounding is monotonic) through ordered-uint atomics, whose result does not depend on order
template <typename R>
__global__ __launch_bounds__(256) void mesh_vertex_kernel(const MeshJob m, float* __restrict__ xyz, float* __restrict__ uv) {
    const int b = blockIdx.y;
    const size_t nv = (size_t)m.nx * m.ny, i = (size_t)blockIdx.x * 256 + threadIdx.x, slab = (size_t)b * nv;
    const bool keep = i < nv && m.vmap[slab + i] >= 0;
    unsigned total;
    const unsigned rank = block_rank(keep ? 1 : 0, total);
    if (total == 0) return;  // (uniform over the block)
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (keep) {
#pragma clang fp contract(off)
        R x, y;
        mesh_vertex_xy(m, i, x, y);
        const MeshTaps<R> t = mesh_taps(x, y, m.H, m.W);
        const unsigned* f = m.frames + (size_t)b * m.H * m.W;
        const R s = (R)(1.0 / 16777216.0);
        const R d = mesh_lerp(t, (R)(f[t.tl] & 0xffffffu) * s, (R)(f[t.tr] & 0xffffffu) * s, (R)(f[t.bl] & 0xffffffu) * s,
                              (R)(f[t.br] & 0xffffffu) * s);
        const R lin = (R)m.a + (R)m.b * d, depth = m.is_metric ? lin : (R)1 / lin;  // shaders.js:178-180
        p[0] = (float)(depth * x * (R)m.x_scale * (R)m.tan_half_fov);
        p[1] = (float)(depth * y * (R)m.y_scale * (R)m.tan_half_fov);
        p[2] = (float)(-depth);
        const size_t nw = (size_t)m.vcnt[(size_t)b * gridDim.x + blockIdx.x] + rank, o = slab + nw;
        xyz[3 * o] = p[0];
        xyz[3 * o + 1] = p[1];
        xyz[3 * o + 2] = p[2];
        uv[2 * o] = (float)((x + (R)1) * (R)0.5);
        uv[2 * o + 1] = (float)((y + (R)1) * (R)0.5);
        m.vmap[slab + i] = (int)nw;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const BlockMinMax<float> r = block_minmax_reduce(keep ? p[k] : INFINITY, keep ? p[k] : -INFINITY, false, keep);
        if (threadIdx.x == 0) {  // (most blocks improve nothing: a device-scope load first keeps them off the six contended addresses)
            unsigned* lo = m.bord + 6 * (size_t)b + k;
            if (f2ord(r.lo) < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo, f2ord(r.lo));
            if (f2ord(r.hi) > __hip_atomic_load(lo + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(lo + 3, f2ord(r.hi));
        }
    }
}

// the image's bounds once its vertices are written (the first workgroup of the launch after): save_gltf.js:16-17's initial values when nothing
// was kept; its clamp of real values to +-1e6 is not reproduced
__device__ __forceinline__ void mesh_finish_bounds(const MeshJob& m, int b, const int* counts, float* bounds) {
    if (blockIdx.x == 0 && threadIdx.x < 6)
        bounds[6 * (size_t)b + threadIdx.x] = counts[2 * (size_t)b] > 0 ? ord2f(m.bord[6 * (size_t)b + threadIdx.x]) : (threadIdx.x < 3 ? 1e6f : -1e6f);
}

// (5) mesh.js:357-368: the kept faces in cell order, first then second triangle, with the new vertex indices
__global__ __launch_bounds__(256) void mesh_face_kernel(const MeshJob m, unsigned* __restrict__ faces, const int* __restrict__ counts,
                                                        float* __restrict__ bounds) {
    const int b = blockIdx.y;
    mesh_finish_bounds(m, b, counts, bounds);
    const size_t cells = ((size_t)m.nx - 1) * ((size_t)m.ny - 1), k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int e[4];
    const int tri = k < cells ? mesh_cell(m, b, k, e) : 0;
    unsigned total;
    const unsigned rank = block_rank((tri & 1) + (tri >> 1), total);
    if (!tri) return;
    unsigned* o = faces + ((size_t)b * 2 * cells + m.fcnt[(size_t)b * gridDim.x + blockIdx.x] + rank) * 3;
    if (tri & 1) {
        o[0] = e[0];
        o[1] = e[2];
        o[2] = e[3];
        o += 3;
    }
    if (tri & 2) {
        o[0] = e[0];
        o[1] = e[3];
        o[2] = e[1];
    }
}

// (5, points) mesh.js:287-300: face [i] of every kept vertex, renumbered - the identity list of the kept count
__global__ __launch_bounds__(256) void mesh_point_kernel(const MeshJob m, unsigned* __restrict__ faces, const int* __restrict__ counts,
                                                         float* __restrict__ bounds) {
    const int b = blockIdx.y;
    mesh_finish_bounds(m, b, counts, bounds);
    const size_t nv = (size_t)m.nx * m.ny, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int nw = m.vmap[(size_t)b * nv + i];
    if (nw >= 0) faces[(size_t)b * nv + nw] = (unsigned)nw;
}

// the float instances exist in A/B builds alone
#ifdef MDPT_DEBUG_SWITCHES
void mesh_launch_flag_f32(const MeshJob& m, unsigned nbv, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_flag_kernel<float>, dim3(nbv, m.B), dim3(256), 0, stream, m);
}
void mesh_launch_vertex_f32(const MeshJob& m, unsigned nbv, float* xyz, float* uv, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_vertex_kernel<float>, dim3(nbv, m.B), dim3(256), 0, stream, m, xyz, uv);
}
#else
void mesh_launch_flag_f32(const MeshJob&, unsigned, hipStream_t) {}
void mesh_launch_vertex_f32(const MeshJob&, unsigned, float*, float*, hipStream_t) {}
#endif

// ---- tiled high-resolution inference: the maps of overlapping tiles of one photo (DPTModel.inference_regions) put together into one map at the
// photo's resolution. Every forward of a relative-depth model has its own unknown scale and shift (the reference's
// .readme_assets/results_explainer.md, "Results are scene-specific!"), and "Fitting to (more) known data" there names the cure, a least-squares fit
// of the two terms, without code for it: the whole photo inferred once at model size is the guide, every tile's map is fitted to the guide over the
// tile's own box, and the fitted tiles are feather-blended. All arithmetic is fp64, nothing contracted, rounded to fp32 once.
//
// The fit is bit-deterministic without atomics and without one workgroup waiting for or reading another: (1) workgroup (c, t) reduces chunk c of
// tile t's samples - MDPT_TILE_FIT_CHUNK of them, each thread its 8 in order, then block_sum_f64's fixed tree - into parts[t][c]; (2) in the next
// launch one workgroup per tile adds the tile's partials in chunk order and solves. A launch boundary separates the producers from the consumer.

// a map (gh x gw of dtype gdt) covering an H x W frame, at frame position (X, Y): bilinear at u = X gw / W - 0.5, v = Y gh / H - 0.5, clamped to the
// map; fp64 weights, rows first. The one resampler of the fits: the tile fit reads its guide through it (guide_at), the true-depth block its
// prediction at the centre of a ground-truth pixel (align_sample / align_apply_kernel), the guided upsampling its mean coefficients at the centre of a
// photo pixel (guided_apply_kernel, which takes the taps and the mix apart to share taps between neighbouring pixels)
struct BilinearTaps { int x0, x1, y0, y1; double ax, ay; };
__device__ __forceinline__ BilinearTaps bilinear_f64_taps(int gh, int gw, double X, double Y, int H, int W) {
#pragma clang fp contract(off)
    double u = X * (double)gw / (double)W - 0.5, v = Y * (double)gh / (double)H - 0.5;
    u = fmin(fmax(u, 0.0), (double)(gw - 1));
    v = fmin(fmax(v, 0.0), (double)(gh - 1));
    const int x0 = (int)floor(u), y0 = (int)floor(v);
    return BilinearTaps{x0, min(x0 + 1, gw - 1), y0, min(y0 + 1, gh - 1), u - (double)x0, v - (double)y0};
}
// the four taps (row y0: g00 at x0, g01 at x1; row y1: g10, g11) mixed with the fp64 weights, rows first
__device__ __forceinline__ double bilinear_f64_mix(const BilinearTaps& t, double g00, double g01, double g10, double g11) {
#pragma clang fp contract(off)
    const double top = g00 * (1.0 - t.ax) + g01 * t.ax, bot = g10 * (1.0 - t.ax) + g11 * t.ax;
    return top * (1.0 - t.ay) + bot * t.ay;
}
__device__ __forceinline__ double bilinear_f64_at(const void* g, int gdt, int gh, int gw, double X, double Y, int H, int W) {
    const BilinearTaps t = bilinear_f64_taps(gh, gw, X, Y, H, W);
    const double g00 = ld_dt(g, (size_t)t.y0 * gw + t.x0, gdt), g01 = ld_dt(g, (size_t)t.y0 * gw + t.x1, gdt);
    const double g10 = ld_dt(g, (size_t)t.y1 * gw + t.x0, gdt), g11 = ld_dt(g, (size_t)t.y1 * gw + t.x1, gdt);
    return bilinear_f64_mix(t, g00, g01, g10, g11);
}

// the guide (gh x gw of dtype gdt, covering the H x W photo) at photo position (X, Y)
__device__ __forceinline__ double guide_at(const void* g, int gdt, int gh, int gw, double X, double Y, int H, int W) {
    return bilinear_f64_at(g, gdt, gh, gw, X, Y, H, W);
}

// (1) blockIdx.y = tile, blockIdx.x = chunk. Sample (j, i) of the map: x = m[j, i], y = the guide at the pixel's centre in the photo,
// (x1 + (i + 0.5) bw / w, y1 + (j + 0.5) bh / h); a sample whose x or y is not finite is skipped. -> {n, Sx, Sy, Sxx, Sxy, Syy} of the chunk
__global__ __launch_bounds__(256) void tile_fit_partial_kernel(const PostTile* __restrict__ tiles, int dt, const void* __restrict__ guide, int gdt, int gh,
                                                               int gw, int H, int W, double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const PostTile t = tiles[blockIdx.y];
    const size_t n = (size_t)t.h * t.w, base = (size_t)blockIdx.x * MDPT_TILE_FIT_CHUNK;
    if (base >= n) return;  // (uniform over the block: the grid's x extent is that of the largest map)
    const double bw = (double)(t.x2 - t.x1), bh = (double)(t.y2 - t.y1);
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < MDPT_TILE_FIT_CHUNK / 256; ++k) {
        const size_t e = base + (size_t)k * 256 + threadIdx.x;
        if (e >= n) break;
        const int j = (int)(e / t.w), i = (int)(e - (size_t)j * t.w);
        const double x = (double)ld_dt(t.map, e, dt);
        const double X = (double)t.x1 + ((double)i + 0.5) * bw / (double)t.w, Y = (double)t.y1 + ((double)j + 0.5) * bh / (double)t.h;
        const double y = guide_at(guide, gdt, gh, gw, X, Y, H, W);
        if (isfinite(x) && isfinite(y)) {
            a[0] += 1.0; a[1] += x; a[2] += y;
            a[3] += x * x; a[4] += x * y; a[5] += y * y;
        }
    }
    block_sum_f64<6>(a);
    if (threadIdx.x == 0) {
        double* p = parts + ((size_t)blockIdx.y * max_chunks + blockIdx.x) * 6;
        for (int k = 0; k < 6; ++k) p[k] = a[k];
    }
}

// the least-squares line y = s x + t of the sums {n, Sx, Sy, Sxx, Sxy}: var = n Sxx - Sx^2, s = (n Sxy - Sx Sy) / var, t = (Sy - s Sx) / n; a
// degenerate set (n < 2, var <= 0, s not finite or <= 0) gets s = 0, t = Sy / n; n == 0: t = 0. (The tile fit's and the true-depth fit's one rule)
__device__ __forceinline__ void affine_solve(double n, double sx, double sy, double sxx, double sxy, double& scale, double& shift) {
#pragma clang fp contract(off)
    scale = 0.0, shift = 0.0;
    if (n > 0.0) {
        const double var = n * sxx - sx * sx;
        const double cand = (n * sxy - sx * sy) / var;
        if (n >= 2.0 && var > 0.0 && isfinite(cand) && cand > 0.0) {
            scale = cand;
            shift = (sy - scale * sx) / n;
        } else {
            shift = sy / n;
        }
    }
}

// (2) one workgroup per tile: lane k adds partial sum k of the tile's chunks in chunk order -> sums[t]; then var = n Sxx - Sx^2,
// s = (n Sxy - Sx Sy) / var, t = (Sy - s Sx) / n -> fit[t] = {s, t}. A degenerate tile (n < 2, var <= 0, s not finite or <= 0) gets s = 0 and the
// guide's mean t = Sy / n; n == 0: t = 0, and the blend skips the tile (sums[t][0] == 0 marks it empty)
__global__ __launch_bounds__(64) void tile_fit_solve_kernel(const PostTile* __restrict__ tiles, const double* __restrict__ parts, int max_chunks,
                                                            double* __restrict__ sums, double* __restrict__ fit) {
#pragma clang fp contract(off)
    const int t = blockIdx.x;
    __shared__ double s[6];
    if (threadIdx.x < 6) {
        const size_t chunks = tile_fit_chunks((size_t)tiles[t].h * tiles[t].w);
        const double* p = parts + (size_t)t * max_chunks * 6 + threadIdx.x;
        double acc = 0.0;
        for (size_t c = 0; c < chunks; ++c) acc += p[c * 6];
        s[threadIdx.x] = acc;
        sums[(size_t)t * 6 + threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double scale, shift;
    affine_solve(s[0], s[1], s[2], s[3], s[4], scale, shift);
    fit[2 * (size_t)t] = scale;
    fit[2 * (size_t)t + 1] = shift;
}

// Blend: out[Y, X] = (float)(sum_t w_t z_t / sum_t w_t) over the non-empty tiles whose box holds the pixel, in tile order. z_t = s_t val_t + t_t,
// val_t = cv2.resize(m_t, (bw, bh)) at (Y - y1, X - x1) as the cutout kernel evaluates it (cv_tap / lerp_cv64: fp32 weights, fp64 sums, rows
// first), with equal taps giving that tap (lerp_tile), so that constant tiles blend to exactly their constant. w_t = wx wy,
// wx = min(1, (dx + 1) / (r + 1)) with dx the distance in pixels to the nearer of the tile's left and right edge columns - an edge on the photo's
// border does not count (no ramp at the image's own border; neither counts: wx = 1) - wy likewise. No tile: NaN; a z that is
// not finite propagates.
// A workgroup owns a BLEND_BW x BLEND_BH block of the photo (16 threads x BLEND_PX pixels across, 16 rows). It walks the table 256 tiles at a time:
// the tiles that touch the block are compacted, in order (block_rank), into LDS with their fit and resize scales, and every thread loops over those
// survivors only - a 16 x 16 grid of tiles costs a pixel the 1 to 4 tiles that hold it, not 256 box tests.
constexpr int BLEND_PX = 4, BLEND_BW = 64, BLEND_BH = 16;
struct BlendTile { const void* map; double s, t, scale_x, scale_y; int h, w, x1, y1, x2, y2; };

// lerp_cv64, except that two equal taps give that tap: cv2's fp32 weights 1 - a and a need not sum to 1 where the source position lies in the
// first source interval (a < 1 carries bits below 2^-24), which would leave a flat region of the tiles one fp32 ulp off the value they all hold.
// (Two equal infinite taps give that infinity under both rules: lerp_cv64 multiplies by 0 < 1 - a and 0 < a only, its a == 0 case is one tap)
__device__ __forceinline__ double lerp_tile(double v0, double v1, float a) { return v0 == v1 ? v0 : lerp_cv64(v0, v1, a); }

// min(1, (d + 1) / (r + 1)) of edge distance d (d < 0: no edge counts), r1 = r + 1
__device__ __forceinline__ double feather_weight(int d, double r1) {
#pragma clang fp contract(off)
    return d >= 0 && (double)d + 1.0 < r1 ? ((double)d + 1.0) / r1 : 1.0;
}

// the distance of coordinate c to the nearer edge of [lo, hi) that is not the photo's border [0, n); -1: neither counts
__device__ __forceinline__ int edge_distance(int c, int lo, int hi, int n) {
    const int dl = lo > 0 ? c - lo : -1, dr = hi < n ? hi - 1 - c : -1;
    return dl < 0 ? dr : (dr < 0 ? dl : min(dl, dr));
}

__global__ __launch_bounds__(256) void tile_blend_kernel(const PostTile* __restrict__ tiles, int T, int dt, int H, int W, const double* __restrict__ fit,
                                                         const double* __restrict__ sums, double r1, float* __restrict__ out, int blocks_x) {
#pragma clang fp contract(off)
    __shared__ BlendTile live[256];
    const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
    const int bx0 = bx * BLEND_BW, by0 = by * BLEND_BH, bx1 = min(bx0 + BLEND_BW, W), by1 = min(by0 + BLEND_BH, H);
    const int Y = by0 + (int)threadIdx.x / (BLEND_BW / BLEND_PX), X0 = bx0 + ((int)threadIdx.x % (BLEND_BW / BLEND_PX)) * BLEND_PX;
    const bool active = Y < H && X0 < W;
    double num[BLEND_PX], den[BLEND_PX];
#pragma unroll
    for (int k = 0; k < BLEND_PX; ++k) num[k] = den[k] = 0.0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        PostTile ti{};
        bool keep = false;
        if (t < T) {
            ti = tiles[t];
            keep = ti.x1 < bx1 && ti.x2 > bx0 && ti.y1 < by1 && ti.y2 > by0 && !(sums && sums[6 * (size_t)t] == 0.0);
        }
        unsigned total;
        const unsigned rank = block_rank(keep ? 1 : 0, total);
        if (keep)
            live[rank] = BlendTile{ti.map, fit ? fit[2 * (size_t)t] : 1.0, fit ? fit[2 * (size_t)t + 1] : 0.0,
                                   1.0 / ((double)(ti.x2 - ti.x1) / (double)ti.w), 1.0 / ((double)(ti.y2 - ti.y1) / (double)ti.h),
                                   ti.h, ti.w, ti.x1, ti.y1, ti.x2, ti.y2};
        __syncthreads();
        if (!active) continue;  // (the barriers above and in block_rank are passed by every thread of every pass)
        for (unsigned q = 0; q < total; ++q) {
            const BlendTile& b = live[q];
            if (Y < b.y1 || Y >= b.y2 || X0 >= b.x2 || X0 + BLEND_PX <= b.x1) continue;
            const CvTap ty = cv_tap(Y - b.y1, b.scale_y, b.h);
            const double wy = feather_weight(edge_distance(Y, b.y1, b.y2, H), r1);
            const size_t row0 = (size_t)ty.s0 * b.w, row1 = (size_t)ty.s1 * b.w;
            int key = -1;
            double m00 = 0.0, m01 = 0.0, m10 = 0.0, m11 = 0.0;
#pragma unroll
            for (int k = 0; k < BLEND_PX; ++k) {
                const int X = X0 + k;
                if (X < b.x1 || X >= b.x2 || X >= W) continue;
                const CvTap tx = cv_tap(X - b.x1, b.scale_x, b.w);
                if (2 * tx.s0 + (tx.s1 != tx.s0) != key) {  // the taps of consecutive pixels repeat where the tile is enlarged
                    key = 2 * tx.s0 + (tx.s1 != tx.s0);
                    m00 = (double)ld_dt(b.map, row0 + tx.s0, dt);
                    m01 = (double)ld_dt(b.map, row0 + tx.s1, dt);
                    m10 = (double)ld_dt(b.map, row1 + tx.s0, dt);
                    m11 = (double)ld_dt(b.map, row1 + tx.s1, dt);
                }
                const double val = lerp_tile(lerp_tile(m00, m01, tx.a), lerp_tile(m10, m11, tx.a), ty.a);
                const double z = b.s * val + b.t;
                const double w = feather_weight(edge_distance(X, b.x1, b.x2, W), r1) * wy;
                num[k] += w * z;
                den[k] += w;
            }
        }
    }
    if (!active) return;
    float v[BLEND_PX];
#pragma unroll
    for (int k = 0; k < BLEND_PX; ++k) v[k] = den[k] > 0.0 ? (float)(num[k] / den[k]) : NAN;
    float* o = out + (size_t)Y * W + X0;
    if (X0 + BLEND_PX <= W && ((uintptr_t)o & 15) == 0) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < BLEND_PX && X0 + k < W; ++k) o[k] = v[k];
    }
}

// ---- true depth from ground truth: a prediction aligned to a measured depth map that is partly valid and at its own resolution, scored with the
// standard metrics, and mapped to true depth. The reference's .readme_assets/results_explainer.md gives depth = 1 / (A V + B) ("True depth from DPT
// result") and names two ways to A and B when measurements exist ("Fitting to (more) known data": least squares, or matching the median and the
// spread), with code for neither. A pair is an AlignPair (mdpt_kernels.h); the table lives in device memory and pairs may all differ in size.
// Everything follows the tile fit: fp64, nothing contracted, rounded once, fixed chunks reduced by a fixed tree and added in chunk order by the
// next launch, integer atomics only (the radix select's counts, which do not depend on order), no workgroup waits for or reads another.

struct AlignSample { double v, t, g; };

// THE sample rule of every kernel below: truth pixel e = Y W + X of pair p. g = truth[e] counts if it is finite, > 0, inside [tmin, tmax] (+-inf:
// no bound) and valid[e] != 0 (valid == null: all); v = the prediction at the pixel's centre (bilinear_f64_at) must be finite; t = 1 / g in
// inverse space, g in depth space. (truth is tested first: a pixel without a measurement costs no prediction read)
__device__ __forceinline__ bool align_sample(const AlignPair& p, int dt, int inverse, double tmin, double tmax, size_t e, AlignSample& s) {
#pragma clang fp contract(off)
    const double g = (double)p.truth[e];
    if (!(isfinite(g) && g > 0.0 && g >= tmin && g <= tmax)) return false;
    if (p.valid && p.valid[e] == 0) return false;
    const int Y = (int)(e / (size_t)p.W), X = (int)(e - (size_t)Y * p.W);
    const double v = bilinear_f64_at(p.pred, dt, p.ph, p.pw, (double)X + 0.5, (double)Y + 0.5, p.H, p.W);
    if (!isfinite(v)) return false;
    s.v = v;
    s.g = g;
    s.t = inverse ? 1.0 / g : g;
    return true;
}

// lane k < K of the block adds partial sum k of `chunks` chunks in chunk order -> s[k] (shared); the block is synchronised on return
template <int K>
__device__ __forceinline__ void chunk_order_sum(const double* __restrict__ parts, size_t chunks, double* s) {
    if (threadIdx.x < K) {
        double acc = 0.0;
        for (size_t c = 0; c < chunks; ++c) acc += parts[c * K + threadIdx.x];
        s[threadIdx.x] = acc;
    }
    __syncthreads();
}

// least squares (1): blockIdx.y = pair, blockIdx.x = chunk of MDPT_TILE_FIT_CHUNK truth pixels -> {n, Sv, St, Svv, Svt, Stt} of the chunk
__global__ __launch_bounds__(256) void align_fit_partial_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                                double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    const size_t n = (size_t)p.H * p.W, base = (size_t)blockIdx.x * MDPT_TILE_FIT_CHUNK;
    if (base >= n) return;  // (uniform over the block)
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < MDPT_TILE_FIT_CHUNK / 256; ++k) {
        const size_t e = base + (size_t)k * 256 + threadIdx.x;
        if (e >= n) break;
        AlignSample s;
        if (align_sample(p, dt, inverse, tmin, tmax, e, s)) {
            a[0] += 1.0; a[1] += s.v; a[2] += s.t;
            a[3] += s.v * s.v; a[4] += s.v * s.t; a[5] += s.t * s.t;
        }
    }
    block_sum_f64<6>(a);
    if (threadIdx.x == 0) {
        double* o = parts + ((size_t)blockIdx.y * max_chunks + blockIdx.x) * 6;
        for (int k = 0; k < 6; ++k) o[k] = a[k];
    }
}

// least squares (2): one workgroup per pair: the partials in chunk order -> sums[p], affine_solve -> fit[p] = {A, B}
__global__ __launch_bounds__(64) void align_fit_solve_kernel(const AlignPair* __restrict__ pairs, const double* __restrict__ parts, int max_chunks,
                                                             double* __restrict__ sums, double* __restrict__ fit) {
    const int p = blockIdx.x;
    __shared__ double s[6];
    chunk_order_sum<6>(parts + (size_t)p * max_chunks * 6, tile_fit_chunks((size_t)pairs[p].H * pairs[p].W), s);
    if (threadIdx.x < 6) sums[(size_t)p * 6 + threadIdx.x] = s[threadIdx.x];
    if (threadIdx.x != 0) return;
    double scale, shift;
    affine_solve(s[0], s[1], s[2], s[3], s[4], scale, shift);
    fit[2 * (size_t)p] = scale;
    fit[2 * (size_t)p + 1] = shift;
}

// ---- the median fit: exact medians of the float32 roundings v32, t32 of the samples by a radix select over order-preserving 32-bit keys, 8 bits
// a pass from the top. A pass is a histogram launch (every workgroup counts the digits of its samples in LDS and flushes the non-zero bins with
// integer atomics) and a select launch (one workgroup per pair narrows the key prefix of BOTH middle ranks, (n - 1) / 2 and n / 2, of both streams,
// and clears the pair's bins for the next pass). Bins: hist[p][2 s + r][256], s = 0 v / 1 t, r = the rank's track; while the two tracks of a stream
// share their prefix only track 0 is counted. State: state[p][0..3] the prefixes, [4..7] the ranks left inside the prefix, [8] n. The samples are
// recomputed in every pass: nothing per pixel is stored.

// float -> key whose unsigned order is the float order (-0.0 before +0.0), and back
__device__ __forceinline__ unsigned f32_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void align_select_clear_kernel(unsigned* __restrict__ hist, unsigned* __restrict__ state) {
    unsigned* h = hist + (size_t)blockIdx.x * ALIGN_HIST_WORDS;
    for (int i = threadIdx.x; i < ALIGN_HIST_WORDS; i += 256) h[i] = 0;
    if (threadIdx.x < ALIGN_STATE_WORDS) state[(size_t)blockIdx.x * ALIGN_STATE_WORDS + threadIdx.x] = 0;
}

// blockIdx.y = pair, blockIdx.x strides over the pair's truth pixels. A thread keeps the bin of its last sample per stream and adds its run length
// once the bin changes: the top digits of a depth map are nearly constant, and one LDS atomic per sample would serialise the wave on one address.
__global__ __launch_bounds__(256) void align_hist_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                         const unsigned* __restrict__ state, unsigned* __restrict__ hist, int shift) {
    __shared__ unsigned bins[ALIGN_HIST_WORDS];
    const AlignPair p = pairs[blockIdx.y];
    const size_t n = (size_t)p.H * p.W;
    if ((size_t)blockIdx.x * 256 >= n) return;  // (uniform over the block)
    for (int i = threadIdx.x; i < ALIGN_HIST_WORDS; i += 256) bins[i] = 0;
    const unsigned* st = state + (size_t)blockIdx.y * ALIGN_STATE_WORDS;
    const unsigned pre[4] = {st[0], st[1], st[2], st[3]};
    const unsigned mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    __syncthreads();
    int cur[2] = {-1, -1};
    unsigned run[2] = {0, 0};
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        AlignSample s;
        if (!align_sample(p, dt, inverse, tmin, tmax, e, s)) continue;
        const unsigned key[2] = {f32_key((float)s.v), f32_key((float)s.t)};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const unsigned top = key[q] & mask;
            const int track = top == pre[2 * q] ? 0 : (top == pre[2 * q + 1] ? 1 : -1);
            if (track < 0) continue;
            const int bin = (2 * q + track) * 256 + (int)((key[q] >> shift) & 255u);
            if (bin != cur[q]) {
                if (run[q]) atomicAdd(&bins[cur[q]], run[q]);
                cur[q] = bin;
                run[q] = 0;
            }
            ++run[q];
        }
    }
    for (int q = 0; q < 2; ++q)
        if (run[q]) atomicAdd(&bins[cur[q]], run[q]);
    __syncthreads();
    unsigned* h = hist + (size_t)blockIdx.y * ALIGN_HIST_WORDS;
    for (int i = threadIdx.x; i < ALIGN_HIST_WORDS; i += 256)
        if (bins[i]) atomicAdd(&h[i], bins[i]);
}

// one workgroup per pair; thread 2 s + r < 4 walks the 256 bins of its stream and track to the digit that holds its rank. After the last pass
// (shift == 0) the prefixes are the keys of the two middle order statistics: med = ((double)lo + (double)hi) 0.5 -> sums[p] = {n, med v, med t}
// (n == 0: zeros)
__global__ __launch_bounds__(256) void align_select_kernel(unsigned* __restrict__ hist, unsigned* __restrict__ state, int shift, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ unsigned bins[ALIGN_HIST_WORDS];
    __shared__ unsigned key[4];
    unsigned* h = hist + (size_t)blockIdx.x * ALIGN_HIST_WORDS;
    unsigned* st = state + (size_t)blockIdx.x * ALIGN_STATE_WORDS;
    for (int i = threadIdx.x; i < ALIGN_HIST_WORDS; i += 256) {
        bins[i] = h[i];
        h[i] = 0;
    }
    const int tr = threadIdx.x & 3, s2 = tr & 2;
    const unsigned pre = st[tr], pre0 = st[s2], pre1 = st[s2 + 1], rank_in = st[4 + tr];
    unsigned n = st[8];
    __syncthreads();  // (the state is read by every thread before any thread writes it)
    if (threadIdx.x < 4) {
        const unsigned* b = bins + (pre0 == pre1 ? s2 : tr) * 256;
        unsigned rank = rank_in;
        if (shift == 24) {
            n = 0;
            for (int d = 0; d < 256; ++d) n += bins[d];  // (every sample has a v key: track 0 of stream v holds them all)
            rank = n == 0 ? 0u : ((tr & 1) ? n / 2 : (n - 1) / 2);
        }
        unsigned below = 0;
        int d = 0;
        for (; d < 255; ++d) {
            if (rank < below + b[d]) break;
            below += b[d];
        }
        key[tr] = pre | ((unsigned)d << shift);
        st[tr] = key[tr];
        st[4 + tr] = rank - below;
        if (tr == 0) st[8] = n;
    }
    __syncthreads();
    if (shift == 0 && threadIdx.x < 3) {
        double out = (double)n;
        if (threadIdx.x > 0) {
            const int q = 2 * ((int)threadIdx.x - 1);
            out = n == 0 ? 0.0 : ((double)key_f32(key[q]) + (double)key_f32(key[q + 1])) * 0.5;
        }
        sums[(size_t)blockIdx.x * 6 + threadIdx.x] = out;
    }
}

// mean absolute deviation (1): as align_fit_partial_kernel, {sum |v32 - med v|, sum |t32 - med t|} of the chunk
__global__ __launch_bounds__(256) void align_mad_partial_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                                const double* __restrict__ sums, double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    const size_t n = (size_t)p.H * p.W, base = (size_t)blockIdx.x * MDPT_TILE_FIT_CHUNK;
    if (base >= n) return;
    const double mv = sums[(size_t)blockIdx.y * 6 + 1], mt = sums[(size_t)blockIdx.y * 6 + 2];
    double a[2] = {0.0, 0.0};
    for (int k = 0; k < MDPT_TILE_FIT_CHUNK / 256; ++k) {
        const size_t e = base + (size_t)k * 256 + threadIdx.x;
        if (e >= n) break;
        AlignSample s;
        if (align_sample(p, dt, inverse, tmin, tmax, e, s)) {
            a[0] += fabs((double)(float)s.v - mv);
            a[1] += fabs((double)(float)s.t - mt);
        }
    }
    block_sum_f64<2>(a);
    if (threadIdx.x == 0) {
        double* o = parts + ((size_t)blockIdx.y * max_chunks + blockIdx.x) * 2;
        o[0] = a[0];
        o[1] = a[1];
    }
}

// mean absolute deviation (2): mad = S / n -> sums[p][3..5] = {mad v, mad t, 0}; A = mad t / mad v, B = med t - A med v. mad v == 0, or an A that is
// not finite or <= 0: A = 0, B = med t (n == 0: 0), the least-squares fit's degenerate rule with the median in the mean's place
__global__ __launch_bounds__(64) void align_mad_solve_kernel(const AlignPair* __restrict__ pairs, const double* __restrict__ parts, int max_chunks,
                                                             double* __restrict__ sums, double* __restrict__ fit) {
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    __shared__ double s[2];
    chunk_order_sum<2>(parts + (size_t)p * max_chunks * 2, tile_fit_chunks((size_t)pairs[p].H * pairs[p].W), s);
    if (threadIdx.x != 0) return;
    double* o = sums + (size_t)p * 6;
    const double n = o[0], mv = o[1], mt = o[2];
    const double mad_v = n > 0.0 ? s[0] / n : 0.0, mad_t = n > 0.0 ? s[1] / n : 0.0;
    o[3] = mad_v;
    o[4] = mad_t;
    o[5] = 0.0;
    double a = 0.0, b = n > 0.0 ? mt : 0.0;
    const double cand = mad_t / mad_v;
    if (n > 0.0 && mad_v > 0.0 && isfinite(cand) && cand > 0.0) {
        a = cand;
        b = mt - a * mv;
    }
    fit[2 * (size_t)p] = a;
    fit[2 * (size_t)p + 1] = b;
}

// metrics (1): as align_fit_partial_kernel. q = A v + B (fit == null: A = 1, B = 0); a sample whose q is not > 0 is counted as bad and left out;
// d = 1 / q in inverse space, q in depth space -> {n, bad, sum |d - g| / g, sum (d - g)^2 / g, sum (d - g)^2, sum e^2, sum |log10 d - log10 g|,
// count r < 1.25, < 1.25^2, < 1.25^3, sum e}, e = ln d - ln g, r = max(d / g, g / d)
__global__ __launch_bounds__(256) void align_metrics_partial_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                                    const double* __restrict__ fit, double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    const size_t n = (size_t)p.H * p.W, base = (size_t)blockIdx.x * MDPT_TILE_FIT_CHUNK;
    if (base >= n) return;
    const double A = fit ? fit[2 * (size_t)blockIdx.y] : 1.0, B = fit ? fit[2 * (size_t)blockIdx.y + 1] : 0.0;
    double a[ALIGN_METRIC_SUMS];
#pragma unroll
    for (int k = 0; k < ALIGN_METRIC_SUMS; ++k) a[k] = 0.0;
    for (int k = 0; k < MDPT_TILE_FIT_CHUNK / 256; ++k) {
        const size_t e = base + (size_t)k * 256 + threadIdx.x;
        if (e >= n) break;
        AlignSample s;
        if (!align_sample(p, dt, inverse, tmin, tmax, e, s)) continue;
        a[0] += 1.0;
        const double q = A * s.v + B;
        if (!(q > 0.0)) {
            a[1] += 1.0;
            continue;
        }
        const double d = inverse ? 1.0 / q : q, g = s.g, diff = d - g;
        const double le = log(d) - log(g), r = fmax(d / g, g / d);
        a[2] += fabs(diff) / g;
        a[3] += diff * diff / g;
        a[4] += diff * diff;
        a[5] += le * le;
        a[6] += fabs(log10(d) - log10(g));
        a[7] += r < 1.25 ? 1.0 : 0.0;
        a[8] += r < 1.5625 ? 1.0 : 0.0;
        a[9] += r < 1.953125 ? 1.0 : 0.0;
        a[10] += le;
    }
    block_sum_f64<ALIGN_METRIC_SUMS>(a);
    if (threadIdx.x == 0) {
        double* o = parts + ((size_t)blockIdx.y * max_chunks + blockIdx.x) * ALIGN_METRIC_SUMS;
        for (int k = 0; k < ALIGN_METRIC_SUMS; ++k) o[k] = a[k];
    }
}

// metrics (2): the partials in chunk order, then over the m = n - bad scored samples: {n, bad, AbsRel, SqRel, RMSE, RMSE-log, log10, delta1, delta2,
// delta3, SILog = 100 sqrt(max(mean e^2 - (mean e)^2, 0))}; m == 0: NaN
__global__ __launch_bounds__(64) void align_metrics_solve_kernel(const AlignPair* __restrict__ pairs, const double* __restrict__ parts, int max_chunks,
                                                                 double* __restrict__ metrics) {
#pragma clang fp contract(off)
    const int p = blockIdx.x;
    __shared__ double s[ALIGN_METRIC_SUMS];
    chunk_order_sum<ALIGN_METRIC_SUMS>(parts + (size_t)p * max_chunks * ALIGN_METRIC_SUMS, tile_fit_chunks((size_t)pairs[p].H * pairs[p].W), s);
    if (threadIdx.x != 0) return;
    double* o = metrics + (size_t)p * ALIGN_METRIC_SUMS;
    const double m = s[0] - s[1];
    o[0] = s[0];
    o[1] = s[1];
    if (!(m > 0.0)) {
        for (int k = 2; k < ALIGN_METRIC_SUMS; ++k) o[k] = NAN;
        return;
    }
    const double me = s[10] / m;
    o[2] = s[2] / m;
    o[3] = s[3] / m;
    o[4] = sqrt(s[4] / m);
    o[5] = sqrt(s[5] / m);
    o[6] = s[6] / m;
    o[7] = s[7] / m;
    o[8] = s[8] / m;
    o[9] = s[9] / m;
    o[10] = 100.0 * sqrt(fmax(s[5] / m - me * me, 0.0));
}

// true depth: out pixel (Y, X) of pair p's H x W output (at out + offs[p]) = the prediction at the pixel's centre, q = A v + B, d = 1 / q in inverse
// space (q <= 0: +inf), q in depth space; then clamped to [dmin, dmax] where those are finite, rounded to fp32 once. NaN stays NaN.
__global__ __launch_bounds__(256) void align_apply_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, const double* __restrict__ fit,
                                                          const long long* __restrict__ offs, double dmin, double dmax, float* __restrict__ out) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    const size_t n = (size_t)p.H * p.W;
    const double A = fit ? fit[2 * (size_t)blockIdx.y] : 1.0, B = fit ? fit[2 * (size_t)blockIdx.y + 1] : 0.0;
    float* o = out + offs[blockIdx.y];
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int Y = (int)(e / (size_t)p.W), X = (int)(e - (size_t)Y * p.W);
        const double v = bilinear_f64_at(p.pred, dt, p.ph, p.pw, (double)X + 0.5, (double)Y + 0.5, p.H, p.W);
        const double q = A * v + B;
        double d = inverse ? (q <= 0.0 ? (double)INFINITY : 1.0 / q) : q;
        if (isfinite(dmin) && d < dmin) d = dmin;
        if (isfinite(dmax) && d > dmax) d = dmax;
        o[e] = (float)d;
    }
}

// ---- photo-guided upsampling: He & Sun's fast guided filter ("Fast Guided Filter", 2015) with the uint8 BGR photo as the guide, for the step every
// route here takes bilinearly: a map of about model size back at the photo's size. The filter is fitted at MAP resolution - the photo averaged over the
// cell of every map pixel is the low-resolution guide - and applied at photo resolution, so the photo is passed over twice and everything between
// works on h x w cells. A pair is a GuidedPair (mdpt_kernels.h); the table lives in device memory and pairs may all differ in size. Six launches:
//   (1) guided_cell_sum_kernel ... photo pixel (Y, X) belongs to cell (Y h / H, X w / W), integer division -> per cell {n, SB, SG, SR} as uint64
//   (2) guided_row_kernel<13> .... per cell g_c = (S_c / n) / 255 and p = the map; the 13 moments g, g g^T, p, g p summed over the cells within
//                                  `radius` along the row, clipped to the grid -> 13 planes of row sums
//   (3) guided_col_kernel<13> .... the row sums summed over the rows within `radius`, divided by the window's own count -> the window means; then
//                                  Sigma = mean(g g^T) - mean(g) mean(g)^T + eps I, a = Sigma^-1 (mean(g p) - mean(g) mean(p)) by Cholesky,
//                                  b = mean(p) - a . mean(g) -> 4 planes {aB, aG, aR, b}
//   (4) guided_row_kernel<4>, (5) guided_col_kernel<4>: the same window mean of the four coefficients -> [h, w, 4]
//   (6) guided_apply_kernel ...... per photo pixel the four mean coefficients resampled at the pixel's centre (bilinear_f64_taps / _mix, the geometry of
//                                  bilinear_f64_at), q = aB B / 255 + aG G / 255 + aR R / 255 + b, rounded to fp32 once
// A window sum is separable and DIRECT: 2 radius + 1 additions along the row, then 2 radius + 1 along the column, each in index order from LDS - no
// running sum (add the entering cell, subtract the leaving one), whose rounding errors would travel along the row and be amplified by Sigma^-1.
// All fp64, nothing contracted. Bit-deterministic and independent of what else is in the call: a workgroup of (1) owns whole cells and adds their
// bytes with integer LDS atomics (exact in any order), every fp64 sum has a fixed order, and a launch boundary separates every producer from its
// consumer. A NaN in a map stays inside the windows that see it, and inside its own pair.

constexpr int GUIDED_CI = 32, GUIDED_CJ = 8;  // cells of one workgroup of the cell sums: 32 across, 8 down
constexpr int GUIDED_ROW_W = 256;             // cells of one workgroup of a row pass
constexpr int GUIDED_COL_T = 32;              // a column pass workgroup owns 32 x 32 cells: 32 threads across, 8 down, 4 rows a thread
constexpr int GUIDED_PX = 4, GUIDED_BW = 64, GUIDED_BH = 16;  // apply: as the tile blend, 16 threads x 4 pixels across, 16 rows

// the first pixel of cell c along an axis of n_cells cells over N pixels: pixel X lies in cell X n_cells / N, so cell c holds [ceil(c N / n_cells),
// ceil((c + 1) N / n_cells)); N >= n_cells leaves no cell empty
__device__ __forceinline__ int guided_cell_start(int c, int n_cells, int N) { return (int)(((long long)c * N + n_cells - 1) / n_cells); }

struct GuidedScratch { unsigned long long* cells; double* ab; double* mean; double* rows; };
__device__ __forceinline__ GuidedScratch guided_scratch(const GuidedPair& p, char* scratch) {
    const size_t n = (size_t)p.h * p.w;
    double* base = (double*)(scratch + p.scratch_off);
    return GuidedScratch{(unsigned long long*)base, base + 4 * n, base + 8 * n, base + 12 * n};
}

// (1) blockIdx.y = pair, blockIdx.x = a block of 32 x 8 cells. Thread t owns the byte columns b0 + t + 256 k of the block's pixel columns (consecutive
// threads read consecutive bytes of a row, one byte each: no alignment is asked of the photo or its pitch), walks each down the rows of one cell row
// with a register sum, and adds that sum to the cell's channel in LDS. Every photo byte is read once, by the one workgroup that owns its cell.
__global__ __launch_bounds__(256) void guided_cell_sum_kernel(const GuidedPair* __restrict__ pairs, char* __restrict__ scratch) {
    const GuidedPair p = pairs[blockIdx.y];
    const int tiles_x = (p.w + GUIDED_CI - 1) / GUIDED_CI, tiles_y = (p.h + GUIDED_CJ - 1) / GUIDED_CJ;
    if (blockIdx.x >= (unsigned)(tiles_x * tiles_y)) return;  // (uniform over the block: the grid's x extent is that of the largest map)
    const int i0 = (int)(blockIdx.x % (unsigned)tiles_x) * GUIDED_CI, j0 = (int)(blockIdx.x / (unsigned)tiles_x) * GUIDED_CJ;
    const int ni = min(GUIDED_CI, p.w - i0), nj = min(GUIDED_CJ, p.h - j0);
    __shared__ unsigned long long acc[GUIDED_CJ][GUIDED_CI][3];
    __shared__ int ys[GUIDED_CJ + 1], xs[GUIDED_CI + 1];
    for (int k = threadIdx.x; k < GUIDED_CJ * GUIDED_CI * 3; k += 256) (&acc[0][0][0])[k] = 0;
    if (threadIdx.x <= (unsigned)nj) ys[threadIdx.x] = guided_cell_start(j0 + (int)threadIdx.x, p.h, p.H);
    if (threadIdx.x >= 64 && threadIdx.x - 64 <= (unsigned)ni) xs[threadIdx.x - 64] = guided_cell_start(i0 + (int)threadIdx.x - 64, p.w, p.W);
    __syncthreads();
    const long long b0 = 3LL * xs[0], b1 = 3LL * xs[ni];
    for (long long b = b0 + threadIdx.x; b < b1; b += 256) {
        const int x = (int)(b / 3), c = (int)(b - 3LL * x);
        const int li = (int)(((long long)x * p.w) / p.W) - i0;
        for (int lj = 0; lj < nj; ++lj) {
            const unsigned char* q = p.photo + (long long)ys[lj] * p.pitch + b;
            unsigned long long s = 0;
            for (int Y = ys[lj]; Y < ys[lj + 1]; ++Y, q += p.pitch) s += *q;
            atomicAdd(&acc[lj][li][c], s);
        }
    }
    __syncthreads();
    const int lj = (int)threadIdx.x / GUIDED_CI, li = (int)threadIdx.x % GUIDED_CI;
    if (lj < nj && li < ni) {
        unsigned long long* o = guided_scratch(p, scratch).cells + 4 * ((size_t)(j0 + lj) * p.w + i0 + li);
        o[0] = (unsigned long long)(ys[lj + 1] - ys[lj]) * (unsigned long long)(xs[li + 1] - xs[li]);
        o[1] = acc[lj][li][0];
        o[2] = acc[lj][li][1];
        o[3] = acc[lj][li][2];
    }
}

// (2), (4) blockIdx.y = pair, blockIdx.x = (row j, segment of 256 cells). The segment's values and `radius` cells of halo either side go to LDS, then
// thread i adds the cells max(i - radius, 0) .. min(i + radius, w - 1) in index order, plane by plane -> rows[k][j w + i]. K == 13: the values are the
// moments of the cell (from the cell sums and the map); K == 4: the coefficients of launch (3).
template <int K>
__global__ __launch_bounds__(256) void guided_row_kernel(const GuidedPair* __restrict__ pairs, int dt, int radius, char* __restrict__ scratch) {
#pragma clang fp contract(off)
    const GuidedPair p = pairs[blockIdx.y];
    const int segs = (p.w + GUIDED_ROW_W - 1) / GUIDED_ROW_W;
    if (blockIdx.x >= (unsigned)segs * (unsigned)p.h) return;  // (uniform over the block)
    const int j = (int)(blockIdx.x / (unsigned)segs), c0 = (int)(blockIdx.x % (unsigned)segs) * GUIDED_ROW_W;
    const GuidedScratch s = guided_scratch(p, scratch);
    const size_t n = (size_t)p.h * p.w, row = (size_t)j * p.w;
    __shared__ double v[K][GUIDED_ROW_W + 2 * GUIDED_MAX_RADIUS];
    const int lo = max(c0 - radius, 0), hi = min(c0 + GUIDED_ROW_W + radius, p.w);
    for (int x = lo + (int)threadIdx.x; x < hi; x += 256) {
        const int at = x - c0 + radius;
        if constexpr (K == GUIDED_MOMENTS) {
            const unsigned long long* cs = s.cells + 4 * (row + x);
            const double cnt = (double)cs[0];
            const double g0 = (double)cs[1] / cnt / 255.0, g1 = (double)cs[2] / cnt / 255.0, g2 = (double)cs[3] / cnt / 255.0;
            const double pm = (double)ld_dt(p.map, row + x, dt);
            v[0][at] = g0, v[1][at] = g1, v[2][at] = g2;
            v[3][at] = g0 * g0, v[4][at] = g0 * g1, v[5][at] = g0 * g2;
            v[6][at] = g1 * g1, v[7][at] = g1 * g2, v[8][at] = g2 * g2;
            v[9][at] = pm, v[10][at] = g0 * pm, v[11][at] = g1 * pm, v[12][at] = g2 * pm;
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k][at] = s.ab[k * n + row + x];
        }
    }
    __syncthreads();
    const int i = c0 + (int)threadIdx.x;
    if (i >= p.w) return;
    const int a = max(i - radius, 0) - c0 + radius, b = min(i + radius, p.w - 1) - c0 + radius;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double sum = 0.0;
        for (int x = a; x <= b; ++x) sum += v[k][x];
        s.rows[k * n + row + i] = sum;
    }
}

// x = Sigma^-1 c for the symmetric positive definite Sigma = {s00, s01, s02, s11, s12, s22}: Cholesky Sigma = L L^T, forward and back substitution
__device__ __forceinline__ void guided_solve3(double s00, double s01, double s02, double s11, double s12, double s22, const double (&c)[3], double (&x)[3]) {
#pragma clang fp contract(off)
    const double l00 = sqrt(s00), l10 = s01 / l00, l20 = s02 / l00;
    const double l11 = sqrt(s11 - l10 * l10), l21 = (s12 - l20 * l10) / l11;
    const double l22 = sqrt(s22 - l20 * l20 - l21 * l21);
    const double y0 = c[0] / l00, y1 = (c[1] - l10 * y0) / l11, y2 = (c[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
}

// (3), (5) blockIdx.y = pair, blockIdx.x = a block of 32 x 32 cells. Plane by plane, the block's rows and `radius` rows of halo above and below go to
// LDS and thread (tx, ty) adds, for each of its four rows j = j0 + ty + 8 q, the rows max(j - radius, 0) .. min(j + radius, h - 1) in index order. The
// 2D window sum divided by the window's own count is the window mean. K == 13: the solve -> ab planes; K == 4: -> mean [h, w, 4] (and the caller's
// coefficient buffer, where pair p starts 4 sum_{q < p} h_q w_q doubles in)
template <int K>
__global__ __launch_bounds__(256) void guided_col_kernel(const GuidedPair* __restrict__ pairs, int radius, double eps, char* __restrict__ scratch,
                                                         double* __restrict__ coeffs) {
#pragma clang fp contract(off)
    const GuidedPair p = pairs[blockIdx.y];
    const int tiles_x = (p.w + GUIDED_COL_T - 1) / GUIDED_COL_T, tiles_y = (p.h + GUIDED_COL_T - 1) / GUIDED_COL_T;
    if (blockIdx.x >= (unsigned)(tiles_x * tiles_y)) return;  // (uniform over the block)
    const int i0 = (int)(blockIdx.x % (unsigned)tiles_x) * GUIDED_COL_T, j0 = (int)(blockIdx.x / (unsigned)tiles_x) * GUIDED_COL_T;
    const GuidedScratch s = guided_scratch(p, scratch);
    const size_t n = (size_t)p.h * p.w;
    __shared__ double tile[GUIDED_COL_T + 2 * GUIDED_MAX_RADIUS][GUIDED_COL_T];
    __shared__ unsigned long long before;
    const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5, i = i0 + tx;
    const int jlo = max(j0 - radius, 0), jhi = min(j0 + GUIDED_COL_T + radius, p.h);
    if (K == 4 && coeffs) {  // the cells of the pairs before this one (an integer sum: any order)
        if (threadIdx.x == 0) before = 0;
        __syncthreads();
        unsigned long long mine = 0;
        for (unsigned q = threadIdx.x; q < blockIdx.y; q += 256) mine += (unsigned long long)pairs[q].h * (unsigned long long)pairs[q].w;
        if (mine) atomicAdd(&before, mine);
    }
    double acc[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        __syncthreads();  // (the previous plane has been read by every thread)
        if (i < p.w)
            for (int jj = jlo + ty; jj < jhi; jj += 8) tile[jj - j0 + radius][tx] = s.rows[k * n + (size_t)jj * p.w + i];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + ty + 8 * q;
            double sum = 0.0;
            if (i < p.w && j < p.h) {
                const int a = max(j - radius, 0) - j0 + radius, b = min(j + radius, p.h - 1) - j0 + radius;
                for (int jj = a; jj <= b; ++jj) sum += tile[jj][tx];
            }
            acc[k][q] = sum;
        }
    }
    if (i >= p.w) return;
    const double across = (double)(min(i + radius, p.w - 1) - max(i - radius, 0) + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + ty + 8 * q;
        if (j >= p.h) continue;
        const double count = across * (double)(min(j + radius, p.h - 1) - max(j - radius, 0) + 1);
        const size_t cell = (size_t)j * p.w + i;
        double m[K];
#pragma unroll
        for (int k = 0; k < K; ++k) m[k] = acc[k][q] / count;
        if constexpr (K == GUIDED_MOMENTS) {
            const double c[3] = {m[10] - m[0] * m[9], m[11] - m[1] * m[9], m[12] - m[2] * m[9]};
            double a3[3];
            guided_solve3(m[3] - m[0] * m[0] + eps, m[4] - m[0] * m[1], m[5] - m[0] * m[2], m[6] - m[1] * m[1] + eps, m[7] - m[1] * m[2],
                          m[8] - m[2] * m[2] + eps, c, a3);
            s.ab[cell] = a3[0];
            s.ab[n + cell] = a3[1];
            s.ab[2 * n + cell] = a3[2];
            s.ab[3 * n + cell] = m[9] - ((a3[0] * m[0] + a3[1] * m[1]) + a3[2] * m[2]);
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) s.mean[4 * cell + k] = m[k];
            if (coeffs)
                for (int k = 0; k < K; ++k) coeffs[4 * ((size_t)before + cell) + k] = m[k];
        }
    }
}

// (6) blockIdx.y = pair, blockIdx.x = a 64 x 16 block of the photo; a thread owns 4 pixels of a row. The pixel's centre (X + 0.5, Y + 0.5) in the
// h x w coefficient grid gives the taps; the 16 doubles of a tap pair are loaded again only where the pair changes (an enlargement repeats it from
// pixel to pixel). c / 255 comes from a table built with that very division. One 16-byte store where the row allows it.
__global__ __launch_bounds__(256) void guided_apply_kernel(const GuidedPair* __restrict__ pairs, char* __restrict__ scratch) {
#pragma clang fp contract(off)
    const GuidedPair p = pairs[blockIdx.y];
    const int blocks_x = (p.W + GUIDED_BW - 1) / GUIDED_BW, blocks_y = (p.H + GUIDED_BH - 1) / GUIDED_BH;
    if (blockIdx.x >= (unsigned)blocks_x * (unsigned)blocks_y) return;  // (uniform over the block)
    __shared__ double unit[256];
    unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    const int Y = (int)(blockIdx.x / (unsigned)blocks_x) * GUIDED_BH + (int)threadIdx.x / (GUIDED_BW / GUIDED_PX);
    const int X0 = (int)(blockIdx.x % (unsigned)blocks_x) * GUIDED_BW + ((int)threadIdx.x % (GUIDED_BW / GUIDED_PX)) * GUIDED_PX;
    if (Y >= p.H || X0 >= p.W) return;
    const double* mean = guided_scratch(p, scratch).mean;
    const unsigned char* px = p.photo + (long long)Y * p.pitch + 3LL * X0;
    float v[GUIDED_PX];
    int key0 = -1, key1 = -1;
    double m0[4], m1[4], m2[4], m3[4];  // the coefficients at (y0, x0), (y0, x1), (y1, x0), (y1, x1)
#pragma unroll
    for (int k = 0; k < GUIDED_PX; ++k) {
        const int X = X0 + k;
        if (X >= p.W) {
            v[k] = 0.0f;
            continue;
        }
        const BilinearTaps t = bilinear_f64_taps(p.h, p.w, (double)X + 0.5, (double)Y + 0.5, p.H, p.W);
        if (t.x0 != key0 || t.x1 != key1) {
            key0 = t.x0, key1 = t.x1;
            const double* r0 = mean + 4 * (size_t)t.y0 * p.w;
            const double* r1 = mean + 4 * (size_t)t.y1 * p.w;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                m0[c] = r0[4 * (size_t)t.x0 + c];
                m1[c] = r0[4 * (size_t)t.x1 + c];
                m2[c] = r1[4 * (size_t)t.x0 + c];
                m3[c] = r1[4 * (size_t)t.x1 + c];
            }
        }
        const double aB = bilinear_f64_mix(t, m0[0], m1[0], m2[0], m3[0]), aG = bilinear_f64_mix(t, m0[1], m1[1], m2[1], m3[1]);
        const double aR = bilinear_f64_mix(t, m0[2], m1[2], m2[2], m3[2]), bb = bilinear_f64_mix(t, m0[3], m1[3], m2[3], m3[3]);
        v[k] = (float)(((aB * unit[px[3 * k]] + aG * unit[px[3 * k + 1]]) + aR * unit[px[3 * k + 2]]) + bb);
    }
    float* o = p.out + (size_t)Y * p.W + X0;
    if (X0 + GUIDED_PX <= p.W && ((uintptr_t)o & 15) == 0) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < GUIDED_PX && X0 + k < p.W; ++k) o[k] = v[k];
    }
}

// ---- rendering of depth meshes: what the reference's 3D viewer does in a browser with WebGL (3dviewer/index.html:1158-1228 render_3d, the mesh
// shaders of shaders.js) for the slabs of the mesh kernels above, read in place, with their device-side counts. Four launches whatever B and V are:
// (1) the z-buffer cleared to all ones, (2) one thread per (mesh, view, kept vertex): clip = [x, y, z, 1] M in fp64, screen x / y snapped to 1/256
// pixel, 1/w and z01 kept in fp64, (3) one workgroup per 256 faces: int64 edge functions on the snapped coordinates at the pixel centres, top-left
// fill rule, z01 interpolated linearly in screen space, the key (fp32 bits of z01) << 32 | face merged into the uint64 z-buffer with atomicMin - an
// integer vector atomic whose result does not depend on order, so the image is bit-deterministic and ties go to the lower face index - and (4) one
// thread per pixel: the winning face's edge values again, perspective-correct barycentrics, a bilinear texture sample, one rounding to uint8.
// Nothing is contracted: tests/render_restate.py restates the arithmetic in numpy, operation by operation.

__device__ __forceinline__ long long render_edge(int ax, int ay, int bx, int by, int px, int py) {
    return ((long long)bx - ax) * ((long long)py - ay) - ((long long)by - ay) * ((long long)px - ax);
}

// a pixel centre ON an edge belongs to the face whose interior lies to its right (a > 0) or, on a horizontal edge, below it (b > 0): the top-left
// rule; (a, b) = the edge function's gradient with the interior positive
__device__ __forceinline__ bool render_edge_in(long long e, long long a, long long b) { return e > 0 || (e == 0 && (a > 0 || (a == 0 && b > 0))); }

// one face of one view, set up: its snapped vertices, s = +1 / -1 so that s x edge is positive inside, E = s x twice the area, and the pixels
// [x0, x1] x [y0, y1] whose centres its bounding box holds, clipped to the viewport. Points: i[0] alone, the square of half-size r.half.
struct RenderTri { int i[3]; int x[3], y[3]; long long s, E; int x0, y0, x1, y1; };

// false: the face does nothing (an index outside the kept vertices, an unusable vertex, no area, culled, or off the viewport)
__device__ __forceinline__ bool render_setup(const RenderJob& r, int b, const RenderVertex* __restrict__ verts, int kv, size_t f, RenderTri& t) {
    const int per = r.points ? 1 : 3;
    const int* fi = r.faces + ((size_t)b * r.nf + f) * per;
    int minx, maxx, miny, maxy;
    for (int k = 0; k < per; ++k) {
        t.i[k] = fi[k];
        if (t.i[k] < 0 || t.i[k] >= kv) return false;
        t.x[k] = verts[t.i[k]].x, t.y[k] = verts[t.i[k]].y;
        if (t.x[k] == RENDER_UNUSABLE) return false;
    }
    if (r.points) {
        t.s = 1, t.E = 1;
        minx = t.x[0] - r.half, maxx = t.x[0] + r.half - 1, miny = t.y[0] - r.half, maxy = t.y[0] + r.half - 1;
    } else {
        const long long area = render_edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
        // rows run downward here, so a triangle that is counter-clockwise with y up - the viewer's front - has a negative area
        if (area == 0 || (area > 0 && r.cull_back)) return false;
        t.s = area < 0 ? -1 : 1, t.E = t.s * area;
        minx = min(t.x[0], min(t.x[1], t.x[2])), maxx = max(t.x[0], max(t.x[1], t.x[2]));
        miny = min(t.y[0], min(t.y[1], t.y[2])), maxy = max(t.y[0], max(t.y[1], t.y[2]));
    }
    // pixel p's centre is at 256 p + 128
    t.x0 = max(0, (minx + 127) >> 8), t.x1 = min(r.W - 1, (maxx - 128) >> 8);
    t.y0 = max(0, (miny + 127) >> 8), t.y1 = min(r.H - 1, (maxy - 128) >> 8);
    return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// the three edge values of pixel (px, py), interior positive, e[k] opposite vertex k -> whether the pixel's centre is covered
__device__ __forceinline__ bool render_cover(const RenderTri& t, int px, int py, long long (&e)[3]) {
    const int X = px * 256 + 128, Y = py * 256 + 128;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = (k + 1) % 3, q = (k + 2) % 3;
        e[k] = t.s * render_edge(t.x[p], t.y[p], t.x[q], t.y[q], X, Y);
        in = in && render_edge_in(e[k], -t.s * ((long long)t.y[q] - t.y[p]), t.s * ((long long)t.x[q] - t.x[p]));
    }
    return in;
}

__device__ __forceinline__ void render_merge(unsigned long long* __restrict__ zb, double z01, unsigned face) {
    if (!(z01 >= 0.0 && z01 <= 1.0)) return;  // near / far
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)z01 + 0.0f) << 32) | face;
    if (key < *zb) atomicMin(zb, key);  // (the plain read can only be stale upward: a key that could win is never skipped)
}

// every pixel of a face's box from `first` in steps of `step`: one lane alone (0, 1) or the workgroup together (threadIdx.x, 256)
__device__ __forceinline__ void render_walk(const RenderJob& r, const RenderVertex* __restrict__ verts, unsigned long long* __restrict__ zb,
                                            const RenderTri& t, unsigned face, int first, int step) {
#pragma clang fp contract(off)
    const int bw = t.x1 - t.x0 + 1, n = bw * (t.y1 - t.y0 + 1);
    const double z0 = verts[t.i[0]].z01;
    if (r.points) {
        for (int p = first; p < n; p += step) render_merge(zb + (size_t)(t.y0 + p / bw) * r.W + (t.x0 + p % bw), z0, face);
        return;
    }
    const double z1 = verts[t.i[1]].z01, z2 = verts[t.i[2]].z01, E = (double)t.E;
    for (int p = first; p < n; p += step) {
        const int px = t.x0 + p % bw, py = t.y0 + p / bw;
        long long e[3];
        if (!render_cover(t, px, py, e)) continue;
        render_merge(zb + (size_t)py * r.W + px, ((double)e[0] * z0 + (double)e[1] * z1 + (double)e[2] * z2) / E, face);
    }
}

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long* __restrict__ zbuf, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) zbuf[i] = ~0ull;
}

__device__ __forceinline__ int render_kept(const RenderJob& r, int b, int which) {
    const int k = r.counts[2 * (size_t)b + which], cap = which ? r.nf : r.nv;
    return k < 0 ? 0 : (k > cap ? cap : k);
}

// blockIdx.y = mesh b x V + view
__global__ __launch_bounds__(256) void render_vertex_kernel(const RenderJob r) {
#pragma clang fp contract(off)
    const int bv = blockIdx.y, b = bv / r.V;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)render_kept(r, b, 0)) return;
    const float* p = r.xyz + ((size_t)b * r.nv + i) * 3;
    const double* M = r.view_proj + (size_t)bv * 16;
    const double x = p[0], y = p[1], z = p[2];
    const double cx = x * M[0] + y * M[4] + z * M[8] + M[12], cy = x * M[1] + y * M[5] + z * M[9] + M[13];
    const double cz = x * M[2] + y * M[6] + z * M[10] + M[14], cw = x * M[3] + y * M[7] + z * M[11] + M[15];
    RenderVertex o{RENDER_UNUSABLE, 0, 0.0, 0.0};
    if (cw > 0.0) {
        const double sx = rint((cx / cw + 1.0) * 0.5 * (double)r.W * 256.0), sy = rint((1.0 - cy / cw) * 0.5 * (double)r.H * 256.0);
        if (fabs(sx) < 1073741824.0 && fabs(sy) < 1073741824.0) o = RenderVertex{(int)sx, (int)sy, 1.0 / cw, (cz / cw + 1.0) * 0.5};
    }
    r.verts[(size_t)bv * r.nv + i] = o;
}

__global__ __launch_bounds__(256) void render_raster_kernel(const RenderJob r) {
    __shared__ unsigned queue[256];
    __shared__ unsigned queued;
    const int bv = blockIdx.y, b = bv / r.V;
    const int kv = render_kept(r, b, 0), kf = render_kept(r, b, 1);
    const size_t first = (size_t)blockIdx.x * 256;
    if (first >= (size_t)kf) return;  // (the whole workgroup)
    if (threadIdx.x == 0) queued = 0;
    __syncthreads();
    const RenderVertex* verts = r.verts + (size_t)bv * r.nv;
    unsigned long long* zb = r.zbuf + (size_t)bv * r.H * r.W;
    const size_t f = first + threadIdx.x;
    RenderTri t;
    if (f < (size_t)kf && render_setup(r, b, verts, kv, f, t)) {
        if ((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) <= RENDER_SMALL_BOX)
            render_walk(r, verts, zb, t, (unsigned)f, 0, 1);
        else
            queue[atomicAdd(&queued, 1u)] = threadIdx.x;  // (any order: the merge does not depend on it)
    }
    __syncthreads();
    const unsigned n = queued;
    for (unsigned j = 0; j < n; ++j) {
        const size_t g = first + queue[j];
        if (render_setup(r, b, verts, kv, g, t)) render_walk(r, verts, zb, t, (unsigned)g, (int)threadIdx.x, 256);
    }
}

// GL's LINEAR filter with CLAMP_TO_EDGE on one level: texel centres at + 0.5, v = 1 the photo's first row -> the three bytes, rounded once
__device__ __forceinline__ void render_sample(const RenderTex& tex, double u, double v, unsigned char (&bgr)[3]) {
#pragma clang fp contract(off)
    const double tx = fmin(fmax(u * (double)tex.w - 0.5, -1.0), (double)tex.w), ty = fmin(fmax((1.0 - v) * (double)tex.h - 0.5, -1.0), (double)tex.h);
    const double fx0 = floor(tx), fy0 = floor(ty), wx = tx - fx0, wy = ty - fy0;
    const int x0 = min(max((int)fx0, 0), tex.w - 1), x1 = min(max((int)fx0 + 1, 0), tex.w - 1);
    const int y0 = min(max((int)fy0, 0), tex.h - 1), y1 = min(max((int)fy0 + 1, 0), tex.h - 1);
    const unsigned char* top = tex.bgr + (size_t)y0 * tex.w * 3;
    const unsigned char* bot = tex.bgr + (size_t)y1 * tex.w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = (1.0 - wx) * (double)top[3 * x0 + c] + wx * (double)top[3 * x1 + c];
        const double d = (1.0 - wx) * (double)bot[3 * x0 + c] + wx * (double)bot[3 * x1 + c];
        const double val = floor((1.0 - wy) * a + wy * d + 0.5);
        bgr[c] = (unsigned char)(int)fmin(fmax(val, 0.0), 255.0);
    }
}

__global__ __launch_bounds__(256) void render_resolve_kernel(const RenderJob r, uchar4* __restrict__ color, float* __restrict__ depth,
                                                             int* __restrict__ ids) {
#pragma clang fp contract(off)
    const int bv = blockIdx.y, b = bv / r.V;
    const size_t hw = (size_t)r.H * r.W, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const size_t o = (size_t)bv * hw + p;
    const unsigned long long key = r.zbuf[o];
    uchar4 c = make_uchar4(0, 0, 0, 0);
    float d = INFINITY;
    int id = -1;
    const RenderVertex* verts = r.verts + (size_t)bv * r.nv;
    RenderTri t;
    if (key != ~0ull && render_setup(r, b, verts, render_kept(r, b, 0), (size_t)(unsigned)key, t)) {
        const float* uv = r.uv + (size_t)b * r.nv * 2;
        double u, v, w;
        if (r.points) {
            u = uv[2 * (size_t)t.i[0]], v = uv[2 * (size_t)t.i[0] + 1], w = 1.0 / verts[t.i[0]].invw;
        } else {
            long long e[3];
            render_cover(t, (int)(p % (size_t)r.W), (int)(p / (size_t)r.W), e);
            const double s0 = (double)e[0] * verts[t.i[0]].invw, s1 = (double)e[1] * verts[t.i[1]].invw, s2 = (double)e[2] * verts[t.i[2]].invw;
            const double S = s0 + s1 + s2, b0 = s0 / S, b1 = s1 / S, b2 = s2 / S;
            u = b0 * (double)uv[2 * (size_t)t.i[0]] + b1 * (double)uv[2 * (size_t)t.i[1]] + b2 * (double)uv[2 * (size_t)t.i[2]];
            v = b0 * (double)uv[2 * (size_t)t.i[0] + 1] + b1 * (double)uv[2 * (size_t)t.i[1] + 1] + b2 * (double)uv[2 * (size_t)t.i[2] + 1];
            w = (double)t.E / S;
        }
        unsigned char bgr[3];
        render_sample(r.tex[b], u, v, bgr);
        c = make_uchar4(bgr[0], bgr[1], bgr[2], 255);
        d = (float)w;
        id = (int)(unsigned)key;
    }
    color[o] = c;
    if (depth) depth[o] = d;
    if (ids) ids[o] = id;
}

// ---- hole filling of rendered views: hierarchical (push-pull) filling with a preference for the far side, for the pixels render_resolve_kernel
// leaves as background - the disocclusions behind depth edges and everything outside the photo's frustum (not in the reference, whose viewer shows
// the holes). Level 0 is the image (a pixel is valid iff alpha != 0 and 0 < depth < inf), level l + 1 halves level l rounding up, to the 1 x 1 level
// L; a node = {three colour channels, depth} fp32, depth 0 = invalid (FillPlan of mdpt_kernels.h). Push and pull share one selection rule: of up to
// four contributors those with (double)d >= (1 - band) x (double)dmax are kept, dmax the largest valid depth among them. Push: the mean of the kept
// children (2Y + dy, 2X + dx) in the order (0,0) (0,1) (1,0) (1,1). Pull, top down, for invalid nodes only: the kept ones of the four nearest
// parents, weights 9/16 3/16 3/16 1/16, normalised by the kept weights. Sums and the one division in fp64 in that order, rounded once to fp32 (at
// level 0: colour floor(v + 0.5) clamped, alpha 255): tests/fill_restate.py restates it in numpy, and nothing here depends on how levels are grouped
// into launches. The launches: (1) fill_push_kernel, one per FILL_PUSH_LEVELS levels below the top: a workgroup owns an aligned 32 x 32 block of its
// base level and makes the 16 x 16, 8 x 8 and 4 x 4 nodes above it through LDS; (2) fill_top_kernel: one workgroup per image holds every level of at
// most 32 x 32 nodes in LDS, finishes the push and starts the pull; (3) fill_pull_kernel, one per level below the top; the last writes the outputs.
// No atomics, no workgroup waits on another, every scratch node that is read was written by this call.

__device__ __forceinline__ float4 fill_pixel(uchar4 c, float d) {
    if (c.w == 0 || !(d > 0.0f && d < INFINITY)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4((float)c.x, (float)c.y, (float)c.z, d);
}

// the selection rule and the weighted mean of the kept contributors -> false: none is valid
__device__ __forceinline__ bool fill_mix(const float4 (&v)[4], const double (&wt)[4], double keep, double (&o)[4]) {
#pragma clang fp contract(off)
    float dmax = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) dmax = fmaxf(dmax, v[k].w);
    if (!(dmax > 0.0f)) return false;
    const double thr = keep * (double)dmax;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, sw = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k].w > 0.0f && (double)v[k].w >= thr) {
            s0 = s0 + wt[k] * (double)v[k].x, s1 = s1 + wt[k] * (double)v[k].y, s2 = s2 + wt[k] * (double)v[k].z, s3 = s3 + wt[k] * (double)v[k].w;
            sw = sw + wt[k];
        }
    o[0] = s0 / sw, o[1] = s1 / sw, o[2] = s2 / sw, o[3] = s3 / sw;
    return true;
}

// push: the node above the four children (a child that does not exist is passed as invalid)
__device__ __forceinline__ float4 fill_push_node(const float4 (&v)[4], double keep) {
    const double ones[4] = {1.0, 1.0, 1.0, 1.0};  // (1 x v and the count are exact: the mean of the kept children)
    double o[4];
    if (!fill_mix(v, ones, keep, o)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
}

// pull: node (y, x) of a level from its parents' level of hp x wp nodes
__device__ __forceinline__ bool fill_pull_node(const float4* __restrict__ parents, int hp, int wp, int y, int x, double keep, double (&o)[4]) {
    const double wt[4] = {0.5625, 0.1875, 0.1875, 0.0625};
    const int ya = y >> 1, xa = x >> 1;
    const int yb = min(max(ya + ((y & 1) ? 1 : -1), 0), hp - 1), xb = min(max(xa + ((x & 1) ? 1 : -1), 0), wp - 1);
    const float4 v[4] = {parents[(size_t)ya * wp + xa], parents[(size_t)ya * wp + xb], parents[(size_t)yb * wp + xa], parents[(size_t)yb * wp + xb]};
    return fill_mix(v, wt, keep, o);
}

__device__ __forceinline__ float fill_byte(double v) { return (float)fmin(fmax(floor(v + 0.5), 0.0), 255.0); }

__device__ __forceinline__ float4* fill_image_nodes(const FillJob& j, int n) { return (float4*)j.scratch + (size_t)n * j.plan.off[j.plan.L + 1]; }

// blockIdx.y = image, blockIdx.x = the 32 x 32 block of level `base`; levels = 1 .. FILL_PUSH_LEVELS levels to make above it
template <bool FROM_INPUT>
__global__ __launch_bounds__(256) void fill_push_kernel(const FillJob j, int base, int levels) {
    __shared__ float4 tile[16 * 16 + 8 * 8];
    const FillPlan& p = j.plan;
    const int n = blockIdx.y;
    const int hb = fill_level_side(p.H, base), wb = fill_level_side(p.W, base);
    const int across = (wb + 31) / 32, by = (int)blockIdx.x / across, bx = (int)blockIdx.x % across;
    float4* img = fill_image_nodes(j, n);
    const float4* below = img + p.off[base];  // (base >= 1)
    {
        const int h1 = fill_level_side(p.H, base + 1), w1 = fill_level_side(p.W, base + 1);
        const int Y = by * 16 + ((int)threadIdx.x >> 4), X = bx * 16 + ((int)threadIdx.x & 15);
        float4 node = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (Y < h1 && X < w1) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cy = 2 * Y + (k >> 1), cx = 2 * X + (k & 1);
                v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (cy < hb && cx < wb) {
                    const size_t c = (size_t)cy * wb + cx;
                    if (FROM_INPUT) {
                        const size_t at = (size_t)n * p.H * p.W + c;
                        v[k] = fill_pixel(((const uchar4*)j.color)[at], j.depth[at]);
                    } else {
                        v[k] = below[c];
                    }
                }
            }
            node = fill_push_node(v, j.keep);
            img[p.off[base + 1] + (size_t)Y * w1 + X] = node;
        }
        tile[threadIdx.x] = node;  // (a node outside the level is invalid: the levels above need no test of their own)
    }
    float4* src = tile;
    float4* dst = tile + 256;
    for (int s = 2, side = 16; s <= levels; ++s, side >>= 1) {
        __syncthreads();
        const int half = side >> 1;  // this level's share of the block: 8 x 8, then 4 x 4
        if ((int)threadIdx.x < half * half) {
            const int hs = fill_level_side(p.H, base + s), ws = fill_level_side(p.W, base + s);
            const int ty = (int)threadIdx.x / half, tx = (int)threadIdx.x % half, Y = by * half + ty, X = bx * half + tx;
            float4 node = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (Y < hs && X < ws) {
                const float4 v[4] = {src[(2 * ty) * side + 2 * tx], src[(2 * ty) * side + 2 * tx + 1], src[(2 * ty + 1) * side + 2 * tx],
                                     src[(2 * ty + 1) * side + 2 * tx + 1]};
                node = fill_push_node(v, j.keep);
                img[p.off[base + s] + (size_t)Y * ws + X] = node;
            }
            dst[threadIdx.x] = node;
        }
        float4* t = src;
        src = dst, dst = t;
    }
}

#define FILL_TOP_NODES (1024 + 256 + 64 + 16 + 4 + 1)

// blockIdx.x = image: the levels top .. L in LDS, pushed up and pulled down; top == 0 (an image of at most 32 x 32 pixels): the whole call
__global__ __launch_bounds__(256) void fill_top_kernel(const FillJob j) {
    __shared__ float4 lds[FILL_TOP_NODES];
    const FillPlan& p = j.plan;
    const int n = blockIdx.x, top = p.top;
    const size_t hw = (size_t)p.H * p.W;
    float4* img = fill_image_nodes(j, n);
    const uchar4* color = (const uchar4*)j.color + (size_t)n * hw;
    const float* depth = j.depth + (size_t)n * hw;
    // level l's first node in LDS: the scratch's order, from level top on (top == 0: the image, then the scratch's levels)
    auto at = [&](int l) { return top ? (int)(p.off[l] - p.off[top]) : (l ? (int)(hw + p.off[l]) : 0); };
    const int n_top = fill_level_side(p.H, top) * fill_level_side(p.W, top), n_all = at(p.L) + 1;
    for (int i = threadIdx.x; i < n_top; i += 256) lds[i] = top ? img[p.off[top] + i] : fill_pixel(color[i], depth[i]);
    for (int l = top; l < p.L; ++l) {
        __syncthreads();
        const int h = fill_level_side(p.H, l), w = fill_level_side(p.W, l), h1 = fill_level_side(p.H, l + 1), w1 = fill_level_side(p.W, l + 1);
        const float4* src = lds + at(l);
        float4* dst = lds + at(l + 1);
        for (int i = threadIdx.x; i < h1 * w1; i += 256) {
            const int Y = i / w1, X = i % w1;
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cy = 2 * Y + (k >> 1), cx = 2 * X + (k & 1);
                v[k] = cy < h && cx < w ? src[cy * w + cx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            dst[i] = fill_push_node(v, j.keep);
        }
    }
    for (int l = p.L - 1; l >= top; --l) {
        __syncthreads();
        const int h = fill_level_side(p.H, l), w = fill_level_side(p.W, l), h1 = fill_level_side(p.H, l + 1), w1 = fill_level_side(p.W, l + 1);
        float4* own = lds + at(l);
        const float4* parents = lds + at(l + 1);
        for (int i = threadIdx.x; i < h * w; i += 256) {
            if (own[i].w > 0.0f) continue;
            double o[4];
            if (!fill_pull_node(parents, h1, w1, i / w, i % w, j.keep, o)) continue;
            own[i] = l ? make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3])
                       : make_float4(fill_byte(o[0]), fill_byte(o[1]), fill_byte(o[2]), (float)o[3]);
        }
    }
    __syncthreads();
    if (top) {
        for (int i = threadIdx.x; i < n_all; i += 256) img[p.off[top] + i] = lds[i];
        return;
    }
    uchar4* out = (uchar4*)j.out + (size_t)n * hw;
    for (int i = threadIdx.x; i < n_top; i += 256) {
        const uchar4 c = color[i];
        const float d = depth[i];
        const bool valid = fill_pixel(c, d).w > 0.0f, filled = lds[i].w > 0.0f;
        const float4 f = lds[i];
        out[i] = valid ? c : (filled ? make_uchar4((unsigned char)f.x, (unsigned char)f.y, (unsigned char)f.z, 255) : make_uchar4(0, 0, 0, 0));
        if (j.out_depth) j.out_depth[(size_t)n * hw + i] = valid ? d : (filled ? f.w : INFINITY);
    }
}

// blockIdx.y = image, one thread per node of level l (below the top): an invalid node takes its value from level l + 1, in place; OUT: l == 0,
// the outputs: valid pixels copied as they are, the others filled, or background where nothing above them is valid (an image without a valid pixel)
template <bool OUT>
__global__ __launch_bounds__(256) void fill_pull_kernel(const FillJob j, int l) {
    const FillPlan& p = j.plan;
    const int n = blockIdx.y;
    const int h = fill_level_side(p.H, l), w = fill_level_side(p.W, l), h1 = fill_level_side(p.H, l + 1), w1 = fill_level_side(p.W, l + 1);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h * w) return;
    float4* img = fill_image_nodes(j, n);
    const float4* parents = img + p.off[l + 1];
    const int y = (int)(i / (size_t)w), x = (int)(i % (size_t)w);
    double o[4];
    if (OUT) {
        const size_t at = (size_t)n * h * w + i;
        uchar4 c = ((const uchar4*)j.color)[at];
        float d = j.depth[at];
        if (!(fill_pixel(c, d).w > 0.0f)) {
            c = make_uchar4(0, 0, 0, 0), d = INFINITY;
            if (fill_pull_node(parents, h1, w1, y, x, j.keep, o))
                c = make_uchar4((unsigned char)fill_byte(o[0]), (unsigned char)fill_byte(o[1]), (unsigned char)fill_byte(o[2]), 255), d = (float)o[3];
        }
        ((uchar4*)j.out)[at] = c;
        if (j.out_depth) j.out_depth[at] = d;
    } else {
        float4* own = img + p.off[l];
        if (own[i].w > 0.0f) return;
        if (fill_pull_node(parents, h1, w1, y, x, j.keep, o)) own[i] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
    }
}

}  // namespace

int mdpt_launch_post_fill(const FillJob& j, hipStream_t stream) {
    const FillPlan& p = j.plan;
    if (j.N <= 0 || j.N > 65535 || p.H <= 0 || p.W <= 0 || p.H > RENDER_MAX_SIDE || p.W > RENDER_MAX_SIDE || !(j.keep >= 0.0 && j.keep <= 1.0) ||
        p.top < 0 || p.top > p.L || p.L >= FILL_MAX_LEVELS)
        return (int)hipErrorInvalidValue;
    for (int base = 0; base < p.top; base += FILL_PUSH_LEVELS) {
        const int levels = p.top - base < FILL_PUSH_LEVELS ? p.top - base : FILL_PUSH_LEVELS;
        const size_t blocks = (((size_t)fill_level_side(p.H, base) + 31) / 32) * (((size_t)fill_level_side(p.W, base) + 31) / 32);
        MdptProfScope prof(base ? "fill_push_kernel<0>" : "fill_push_kernel<1>", 0.0, stream);
        if (base)
            hipLaunchKernelGGL(fill_push_kernel<false>, dim3((unsigned)blocks, j.N), dim3(256), 0, stream, j, base, levels);
        else
            hipLaunchKernelGGL(fill_push_kernel<true>, dim3((unsigned)blocks, j.N), dim3(256), 0, stream, j, base, levels);
    }
    {
        MdptProfScope prof("fill_top_kernel", 0.0, stream);
        hipLaunchKernelGGL(fill_top_kernel, dim3(j.N), dim3(256), 0, stream, j);
    }
    for (int l = p.top - 1; l >= 0; --l) {
        const size_t blocks = ((size_t)fill_level_side(p.H, l) * fill_level_side(p.W, l) + 255) / 256;
        MdptProfScope prof(l ? "fill_pull_kernel<0>" : "fill_pull_kernel<1>", 0.0, stream);
        if (l)
            hipLaunchKernelGGL(fill_pull_kernel<false>, dim3((unsigned)blocks, j.N), dim3(256), 0, stream, j, l);
        else
            hipLaunchKernelGGL(fill_pull_kernel<true>, dim3((unsigned)blocks, j.N), dim3(256), 0, stream, j, l);
    }
    return (int)hipGetLastError();
}

int mdpt_launch_post_render(const RenderJob& r, unsigned char* color, float* depth, int* ids, hipStream_t stream) {
    const size_t hw = (size_t)r.H * r.W, faces = (size_t)r.nf;
    if (r.B <= 0 || r.V <= 0 || (size_t)r.B * r.V > 65535 || r.nv <= 0 || r.nf <= 0 || r.H <= 0 || r.W <= 0 || r.H > RENDER_MAX_SIDE ||
        r.W > RENDER_MAX_SIDE || r.half < 0)
        return (int)hipErrorInvalidValue;
    const dim3 by((unsigned)r.B * r.V);
    const size_t cells = hw * r.B * r.V, clear_blocks = (cells + 2047) / 2048;
    {
        MdptProfScope prof("render_clear_kernel", 0.0, stream);
        hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)(clear_blocks > 65536 ? 65536 : clear_blocks)), dim3(256), 0, stream, r.zbuf, cells);
    }
    {
        MdptProfScope prof("render_vertex_kernel", 0.0, stream);
        hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)(((size_t)r.nv + 255) / 256), by.x), dim3(256), 0, stream, r);
    }
    {
        MdptProfScope prof("render_raster_kernel", 0.0, stream);
        hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)((faces + 255) / 256), by.x), dim3(256), 0, stream, r);
    }
    MdptProfScope prof("render_resolve_kernel", 0.0, stream);
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((hw + 255) / 256), by.x), dim3(256), 0, stream, r, (uchar4*)color, depth, ids);
    return (int)hipGetLastError();
}

int mdpt_launch_post_tile_fit(const PostTile* tiles, int T, int max_chunks, int dt, const void* guide, int gdt, int gh, int gw, int H, int W, double* parts,
                              double* sums, double* fit, hipStream_t stream) {
    // (a grid's x extent times the 256 threads of a block must stay below 2^32)
    if (T <= 0 || T > 65535 || max_chunks <= 0 || max_chunks >= (1 << 24) || gh <= 0 || gw <= 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
    {
        MdptProfScope prof("tile_fit_partial_kernel", 0.0, stream);
        hipLaunchKernelGGL(tile_fit_partial_kernel, dim3(max_chunks, T), dim3(256), 0, stream, tiles, dt, guide, gdt, gh, gw, H, W, parts, max_chunks);
    }
    MdptProfScope prof("tile_fit_solve_kernel", 0.0, stream);
    hipLaunchKernelGGL(tile_fit_solve_kernel, dim3(T), dim3(64), 0, stream, tiles, (const double*)parts, max_chunks, sums, fit);
    return (int)hipGetLastError();
}

int mdpt_launch_post_tile_blend(const PostTile* tiles, int T, int dt, int H, int W, const double* fit, const double* sums, double feather, float* out,
                                hipStream_t stream) {
    const size_t blocks_x = ((size_t)W + BLEND_BW - 1) / BLEND_BW, blocks_y = ((size_t)H + BLEND_BH - 1) / BLEND_BH;
    if (T <= 0 || H <= 0 || W <= 0 || !(feather >= 0.0) || blocks_x * blocks_y >= ((size_t)1 << 24)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("tile_blend_kernel", 0.0, stream);
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)(blocks_x * blocks_y)), dim3(256), 0, stream, tiles, T, dt, H, W, fit, sums, feather + 1.0, out,
                       (int)blocks_x);
    return (int)hipGetLastError();
}

int mdpt_launch_post_align_fit(const AlignPair* pairs, int P, int max_chunks, int dt, int inverse, int median, double tmin, double tmax, double* parts,
                               unsigned* hist, unsigned* state, double* sums, double* fit, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_chunks <= 0 || max_chunks >= (1 << 24)) return (int)hipErrorInvalidValue;
    if (!median) {
        {
            MdptProfScope prof("align_fit_partial_kernel", 0.0, stream);
            hipLaunchKernelGGL(align_fit_partial_kernel, dim3(max_chunks, P), dim3(256), 0, stream, pairs, dt, inverse, tmin, tmax, parts, max_chunks);
        }
        MdptProfScope prof("align_fit_solve_kernel", 0.0, stream);
        hipLaunchKernelGGL(align_fit_solve_kernel, dim3(P), dim3(64), 0, stream, pairs, (const double*)parts, max_chunks, sums, fit);
        return (int)hipGetLastError();
    }
    // 1 clear + 4 x (histogram, select) + the deviation's partial and solve = 11 launches
    {
        MdptProfScope prof("align_select_clear_kernel", 0.0, stream);
        hipLaunchKernelGGL(align_select_clear_kernel, dim3(P), dim3(256), 0, stream, hist, state);
    }
    const int hist_blocks = align_stride_blocks((size_t)max_chunks * MDPT_TILE_FIT_CHUNK);
    for (int shift = 24; shift >= 0; shift -= 8) {
        {
            MdptProfScope prof("align_hist_kernel", 0.0, stream);
            hipLaunchKernelGGL(align_hist_kernel, dim3(hist_blocks, P), dim3(256), 0, stream, pairs, dt, inverse, tmin, tmax, (const unsigned*)state, hist,
                               shift);
        }
        MdptProfScope prof("align_select_kernel", 0.0, stream);
        hipLaunchKernelGGL(align_select_kernel, dim3(P), dim3(256), 0, stream, hist, state, shift, sums);
    }
    {
        MdptProfScope prof("align_mad_partial_kernel", 0.0, stream);
        hipLaunchKernelGGL(align_mad_partial_kernel, dim3(max_chunks, P), dim3(256), 0, stream, pairs, dt, inverse, tmin, tmax, (const double*)sums, parts,
                           max_chunks);
    }
    MdptProfScope prof("align_mad_solve_kernel", 0.0, stream);
    hipLaunchKernelGGL(align_mad_solve_kernel, dim3(P), dim3(64), 0, stream, pairs, (const double*)parts, max_chunks, sums, fit);
    return (int)hipGetLastError();
}

int mdpt_launch_post_align_metrics(const AlignPair* pairs, int P, int max_chunks, int dt, int inverse, double tmin, double tmax, const double* fit,
                                   double* parts, double* metrics, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_chunks <= 0 || max_chunks >= (1 << 24)) return (int)hipErrorInvalidValue;
    {
        MdptProfScope prof("align_metrics_partial_kernel", 0.0, stream);
        hipLaunchKernelGGL(align_metrics_partial_kernel, dim3(max_chunks, P), dim3(256), 0, stream, pairs, dt, inverse, tmin, tmax, fit, parts, max_chunks);
    }
    MdptProfScope prof("align_metrics_solve_kernel", 0.0, stream);
    hipLaunchKernelGGL(align_metrics_solve_kernel, dim3(P), dim3(64), 0, stream, pairs, (const double*)parts, max_chunks, metrics);
    return (int)hipGetLastError();
}

int mdpt_launch_post_align_apply(const AlignPair* pairs, int P, size_t max_pixels, int dt, int inverse, const double* fit, const long long* offs, double dmin,
                                 double dmax, float* out, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_pixels == 0 || max_pixels >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    // (the blocks of a pair stride over its output pixels, 256 at a time: one block per 2048 pixels of the largest output, capped)
    const int blocks = align_stride_blocks(max_pixels);
    MdptProfScope prof("align_apply_kernel", 0.0, stream);
    hipLaunchKernelGGL(align_apply_kernel, dim3(blocks, P), dim3(256), 0, stream, pairs, dt, inverse, fit, offs, dmin, dmax, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_guided(const GuidedPair* pairs, int P, int dt, int radius, double eps, int max_h, int max_w, int max_H, int max_W, char* scratch,
                            double* coeffs, hipStream_t stream) {
    if (P <= 0 || P > 65535 || radius < 0 || radius > GUIDED_MAX_RADIUS || !(eps > 0.0) || max_h <= 0 || max_w <= 0 || max_H < max_h || max_W < max_w)
        return (int)hipErrorInvalidValue;
    // (every grid's x extent is that of the table's largest sizes, below 2^31; a workgroup past its own pair's extent returns at once)
    const size_t cell_blocks = (((size_t)max_w + GUIDED_CI - 1) / GUIDED_CI) * (((size_t)max_h + GUIDED_CJ - 1) / GUIDED_CJ);
    const size_t row_blocks = (((size_t)max_w + GUIDED_ROW_W - 1) / GUIDED_ROW_W) * (size_t)max_h;
    const size_t col_blocks = (((size_t)max_w + GUIDED_COL_T - 1) / GUIDED_COL_T) * (((size_t)max_h + GUIDED_COL_T - 1) / GUIDED_COL_T);
    const size_t apply_blocks = (((size_t)max_W + GUIDED_BW - 1) / GUIDED_BW) * (((size_t)max_H + GUIDED_BH - 1) / GUIDED_BH);
    if (cell_blocks >= ((size_t)1 << 31) || row_blocks >= ((size_t)1 << 31) || apply_blocks >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    {
        MdptProfScope prof("guided_cell_sum_kernel", 0.0, stream);
        hipLaunchKernelGGL(guided_cell_sum_kernel, dim3((unsigned)cell_blocks, P), dim3(256), 0, stream, pairs, scratch);
    }
    {
        MdptProfScope prof("guided_row_kernel<13>", 0.0, stream);
        hipLaunchKernelGGL(guided_row_kernel<GUIDED_MOMENTS>, dim3((unsigned)row_blocks, P), dim3(256), 0, stream, pairs, dt, radius, scratch);
    }
    {
        MdptProfScope prof("guided_col_kernel<13>", 0.0, stream);
        hipLaunchKernelGGL(guided_col_kernel<GUIDED_MOMENTS>, dim3((unsigned)col_blocks, P), dim3(256), 0, stream, pairs, radius, eps, scratch, (double*)nullptr);
    }
    {
        MdptProfScope prof("guided_row_kernel<4>", 0.0, stream);
        hipLaunchKernelGGL(guided_row_kernel<4>, dim3((unsigned)row_blocks, P), dim3(256), 0, stream, pairs, dt, radius, scratch);
    }
    {
        MdptProfScope prof("guided_col_kernel<4>", 0.0, stream);
        hipLaunchKernelGGL(guided_col_kernel<4>, dim3((unsigned)col_blocks, P), dim3(256), 0, stream, pairs, radius, eps, scratch, coeffs);
    }
    MdptProfScope prof("guided_apply_kernel", 0.0, stream);
    hipLaunchKernelGGL(guided_apply_kernel, dim3((unsigned)apply_blocks, P), dim3(256), 0, stream, pairs, scratch);
    return (int)hipGetLastError();
}

int mdpt_launch_post_mesh(const MeshJob& m, float* xyz, float* uv, unsigned* faces, int* counts, float* bounds, hipStream_t stream) {
    const size_t nv = (size_t)m.nx * m.ny, cells = ((size_t)m.nx - 1) * ((size_t)m.ny - 1);
    if (m.B <= 0 || m.B > 65535 || m.nx < 2 || m.ny < 2 || nv >= ((size_t)1 << 31) || 2 * cells >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const unsigned nbv = (unsigned)mesh_blocks(nv), nbf = (unsigned)mesh_blocks(cells);
#ifdef MDPT_DEBUG_SWITCHES  // A/B builds only (read at every call: the probe switches within one process)
    const char* fp32_env = getenv("MDPT_MESH_FP32");
    const bool fp32 = fp32_env && fp32_env[0] == '1';
#else
    const bool fp32 = false;
#endif
    {
        MdptProfScope prof(fp32 ? "mesh_flag_kernel<float>" : "mesh_flag_kernel", 0.0, stream);
        if (fp32)
            mesh_launch_flag_f32(m, nbv, stream);
        else
            hipLaunchKernelGGL(mesh_flag_kernel<double>, dim3(nbv, m.B), dim3(256), 0, stream, m);
    }
    if (!m.points) {
        MdptProfScope prof("mesh_face_count_kernel", 0.0, stream);
        hipLaunchKernelGGL(mesh_face_count_kernel, dim3(nbf, m.B), dim3(256), 0, stream, m);
    }
    {
        MdptProfScope prof("mesh_scan_kernel", 0.0, stream);
        hipLaunchKernelGGL(mesh_scan_kernel, dim3(m.points ? 1 : 2, m.B), dim3(256), 0, stream, m, nbv, nbf, counts);
    }
    {
        MdptProfScope prof(fp32 ? "mesh_vertex_kernel<float>" : "mesh_vertex_kernel", 0.0, stream);
        if (fp32)
            mesh_launch_vertex_f32(m, nbv, xyz, uv, stream);
        else
            hipLaunchKernelGGL(mesh_vertex_kernel<double>, dim3(nbv, m.B), dim3(256), 0, stream, m, xyz, uv);
    }
    MdptProfScope prof(m.points ? "mesh_point_kernel" : "mesh_face_kernel", 0.0, stream);
    if (m.points)
        hipLaunchKernelGGL(mesh_point_kernel, dim3(nbv, m.B), dim3(256), 0, stream, m, faces, counts, bounds);
    else
        hipLaunchKernelGGL(mesh_face_kernel, dim3(nbf, m.B), dim3(256), 0, stream, m, faces, counts, bounds);
    return (int)hipGetLastError();
}

int mdpt_launch_post_block_norm_tiles(const PostRunTable& t, unsigned char* out, float* minmax, hipStream_t stream) {
    int B;
    size_t max_in, max_out;
    if (!table_extent(t, B, max_in, max_out) || max_in > (1u << 24) || max_out > (1u << 24)) return (int)hipErrorInvalidValue;
    for (int r = 0; r < t.n; ++r)
        if (t.run[r].oh % t.run[r].ih || t.run[r].ow % t.run[r].iw) return (int)hipErrorInvalidValue;
    MdptProfScope prof("block_norm_tiles_kernel", 0.0, stream);
    hipLaunchKernelGGL(block_norm_tiles_kernel, dim3(B), dim3(256), 0, stream, t, out, minmax);
    return (int)hipGetLastError();
}

int mdpt_launch_post_minmax(const float* in, size_t n, float* minmax_out, unsigned* scratch2, hipStream_t stream) {
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, stream, scratch2);
    hipLaunchKernelGGL(minmax_kernel, dim3(grid_for(n)), dim3(256), 0, stream, in, n, scratch2);
    hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(1), 0, stream, scratch2, minmax_out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_scale(const float* in, float* out, int B, int ih, int iw, int oh, int ow, float* minmax_out, unsigned* scratch2,
                           hipStream_t stream) {
    MdptProfScope prof("scale_bilinear_kernel", 0.0, stream);
    if (minmax_out) hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, stream, scratch2);
    hipLaunchKernelGGL(scale_bilinear_kernel, dim3(grid_for((size_t)B * oh * ow)), dim3(256), 0, stream, in, out, B, ih, iw, oh, ow,
                       minmax_out ? scratch2 : nullptr);
    if (minmax_out) hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(1), 0, stream, scratch2, minmax_out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_normalize(const float* in, const float* minmax, void* out, size_t n, int mode, int lossy, hipStream_t stream) {
    MdptProfScope prof("normalize_kernel", 0.0, stream);
    if (mode == 0) hipLaunchKernelGGL(normalize_kernel<0>, dim3(grid_for(n)), dim3(256), 0, stream, in, minmax, out, n, lossy);
    else if (mode == 1) hipLaunchKernelGGL(normalize_kernel<1>, dim3(grid_for(n)), dim3(256), 0, stream, in, minmax, out, n, lossy);
    else if (mode == 2) hipLaunchKernelGGL(normalize_kernel<2>, dim3(grid_for(n)), dim3(256), 0, stream, in, minmax, out, n, lossy);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int mdpt_launch_post_seg_minmax(const PostRunTable& t, int in_dt, float* out, unsigned* parts, unsigned* hist_clear, hipStream_t stream) {
    int B;
    size_t max_in, max_out;
    if (!table_extent(t, B, max_in, max_out)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("seg_scale_minmax_kernel", 0.0, stream);
    hipLaunchKernelGGL(seg_scale_minmax_kernel<false>, dim3(SEG_PARTS, B), dim3(256), 0, stream, t, in_dt, (void*)out, parts, hist_clear);
    return (int)hipGetLastError();
}

int mdpt_launch_post_seg_u8(const PostRunTable& t, int in_dt, const unsigned* parts, int reverse, unsigned char* out, unsigned* hist, hipStream_t stream) {
    int B;
    size_t n, max_out;
    if (!table_extent(t, B, n, max_out)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("seg_u8_hist_kernel", 0.0, stream);
    hipLaunchKernelGGL(seg_u8_hist_kernel, dim3(grid_seg(n), B), dim3(256), 0, stream, t, in_dt, parts, reverse, out, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_hist(const unsigned char* in, int B, size_t n, unsigned* hist, hipStream_t stream) {
    MdptProfScope prof("seg_hist_kernel", 0.0, stream);
    hipLaunchKernelGGL(seg_hist_kernel, dim3(grid_seg(n), B), dim3(256), 0, stream, in, n, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_eq_lut(const unsigned* hist, int B, const int* bin_of, int vmin, int vmax, unsigned char* lut, hipStream_t stream) {
    MdptProfScope prof("equalize_lut_kernel", 0.0, stream);
    hipLaunchKernelGGL(equalize_lut_kernel, dim3(B), dim3(256), 0, stream, hist, bin_of, vmin, vmax, lut);
    return (int)hipGetLastError();
}

int mdpt_launch_post_colorize(const PostRunTable& t, const unsigned char* eq, const unsigned char* cmap, int channels, unsigned char* out,
                              hipStream_t stream) {
    int B;
    size_t n, max_out;
    if (!table_extent(t, B, n, max_out)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("colorize_kernel", 0.0, stream);
    hipLaunchKernelGGL(colorize_kernel, dim3(grid_seg(n), B), dim3(256), 0, stream, t, eq, cmap, channels, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_display_prep(const void* in, int dt, int B, int ih, int iw, void* out, int oh, int ow, unsigned* parts, unsigned* hist_clear,
                                  hipStream_t stream) {
    MdptProfScope prof("disp_prep_kernel", 0.0, stream);  // (the label the probes and profiles know the display form by)
    hipLaunchKernelGGL(seg_scale_minmax_kernel<true>, dim3(SEG_PARTS, B), dim3(256), 0, stream, uniform_table(in, B, ih, iw, oh, ow), dt, out, parts,
                       hist_clear);
    return (int)hipGetLastError();
}

int mdpt_launch_post_plane_fit(const void* in, int dt, int B, int h, int w, const unsigned* parts, const int* xy, int N, size_t xy_stride, double* coef,
                               hipStream_t stream) {
    MdptProfScope prof("plane_fit_kernel", 0.0, stream);
    hipLaunchKernelGGL(plane_fit_kernel, dim3(B), dim3(256), 0, stream, in, dt, h, w, parts, xy, N, xy_stride, coef);
    return (int)hipGetLastError();
}

int mdpt_launch_post_plane_eval(const double* coef, int B, int h, int w, float* out, hipStream_t stream) {
    const size_t n = (size_t)h * w;
    MdptProfScope prof("plane_eval_kernel", 0.0, stream);
    hipLaunchKernelGGL(plane_eval_kernel, dim3(grid_seg(n), B), dim3(256), 0, stream, coef, h, w, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_plane_minmax(const PlaneMap& m, double* vparts, hipStream_t stream) {
    MdptProfScope prof("plane_minmax_kernel", 0.0, stream);
    hipLaunchKernelGGL(plane_minmax_kernel, dim3(SEG_PARTS, m.B), dim3(256), 0, stream, m, vparts);
    return (int)hipGetLastError();
}

int mdpt_launch_post_threshold(const PlaneMap& m, double tmin, double delta, int mode, int reverse, void* out, unsigned* hist, hipStream_t stream) {
    const dim3 grid(grid_seg((size_t)m.h * m.w), m.B);
    MdptProfScope prof("threshold_kernel", 0.0, stream);
    if (mode == 1) hipLaunchKernelGGL(threshold_kernel<1>, grid, dim3(256), 0, stream, m, tmin, delta, reverse, out, hist);
    else hipLaunchKernelGGL(threshold_kernel<0>, grid, dim3(256), 0, stream, m, tmin, delta, reverse, out, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_edge_mag(const float* in, int B, int h, int w, const unsigned* parts, const float* blur_w, int ksize, float* mag, unsigned* mag_max,
                              hipStream_t stream) {
    if (ksize < 1 || ksize > 2 * EDGE_MAX_PAD + 1 || ksize % 2 == 0) return (int)hipErrorInvalidValue;
    EdgeBlur blur{};
    for (int i = 0; i < ksize * ksize; ++i) blur.w[i] = blur_w[i];
    blur.ksize = ksize;
    hipError_t e = hipMemsetAsync(mag_max, 0, sizeof(unsigned) * (size_t)B, stream);
    if (e != hipSuccess) return (int)e;
    MdptProfScope prof("edge_mag_kernel", 0.0, stream);
    hipLaunchKernelGGL(edge_mag_kernel, dim3((w + EDGE_TILE - 1) / EDGE_TILE, (h + EDGE_TILE - 1) / EDGE_TILE, B), dim3(256), 0, stream, in, h, w, parts,
                       blur, mag, mag_max);
    return (int)hipGetLastError();
}

int mdpt_launch_post_edge_mask(const float* mag, const unsigned* mag_max, int B, size_t n, unsigned char* out, hipStream_t stream) {
    MdptProfScope prof("edge_mask_kernel", 0.0, stream);
    hipLaunchKernelGGL(edge_mask_kernel, dim3(grid_seg(n), B), dim3(256), 0, stream, mag, mag_max, n, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_pack_u24(const float* in, int B, size_t n, const unsigned* parts, int lossy, const float* mag, const unsigned* mag_max,
                              const unsigned char* mask, size_t mask_stride, unsigned char* out, hipStream_t stream) {
    MdptProfScope prof("pack_u24_kernel", 0.0, stream);
    hipLaunchKernelGGL(pack_u24_kernel, dim3(grid_seg(n), B), dim3(256), 0, stream, in, n, parts, lossy, mag, mag_max, mask,
                       mask_stride, (uchar4*)out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_mask_display(const PlaneMap& m, double tmin, double tmax, int invert, const unsigned char* img, int ih, int iw, unsigned char* mask,
                                  unsigned char* comp, hipStream_t stream) {
    const size_t g = ((size_t)m.h * m.w + 256 * MASK_PX - 1) / (256 * MASK_PX);
    MdptProfScope prof("mask_display_kernel", 0.0, stream);
    hipLaunchKernelGGL(mask_display_kernel, dim3(g > 512 ? 512 : (int)g, m.B), dim3(256), 0, stream, m, tmin, tmax, invert, img, ih, iw, mask, comp);
    return (int)hipGetLastError();
}

int mdpt_launch_post_mask_cutout(const MaskTable& t, double factor, double tmin, double tmax, int invert, unsigned char* bgra, unsigned char* mask,
                                 hipStream_t stream) {
    if (t.n <= 0 || t.n > MDPT_MASK_IMAGES) return (int)hipErrorInvalidValue;
    size_t most = 0;
    for (int k = 0; k < t.n; ++k) most = (size_t)t.im[k].ih * t.im[k].iw > most ? (size_t)t.im[k].ih * t.im[k].iw : most;
    const size_t g = (most + 256 * MASK_PX - 1) / (256 * MASK_PX);
    MdptProfScope prof("mask_cutout_kernel", 0.0, stream);
    hipLaunchKernelGGL(mask_cutout_kernel, dim3(g > 2048 ? 2048 : (int)g, t.n), dim3(256), 0, stream, t, factor, tmin, tmax, invert, bgra, mask);
    return (int)hipGetLastError();
}
