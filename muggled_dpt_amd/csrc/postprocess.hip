// Depth post-processing on the GPU: the step immediately after the DPT forward in the reference's demos
// (muggled_dpt/demo_helpers/postprocess.py:22-29 scale_prediction, :63-74 normalize_01, :79-91 convert_to_uint8;
// run_3dviewer.py:576-590 24-bit packing). HBM-bound streaming kernels: fp32 in, fp32 / u8 out, no host round trip of the
// full-resolution fp32 map. min/max travel through a 2-float device buffer (no sync).

#include "mdpt_kernels.h"
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

// torch's .min() / .max() PROPAGATE NaN (normalize_01 of a map with a NaN gives an all-NaN map) while fminf / fmaxf drop it: a thread
// that saw a NaN says so, and the block then pins the running min to ordered 0 and the running max to ordered ~0, both of which
// ord2f() maps back to NaN bit patterns.
__device__ __forceinline__ void block_minmax(float lo, float hi, bool saw_nan, unsigned* mm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    const bool wave_nan = __any(saw_nan);
    __shared__ float slo[4], shi[4];
    __shared__ int snan[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { slo[wave] = lo; shi[wave] = hi; snan[wave] = wave_nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        bool any_nan = wave_nan;
        for (int w = 1; w < 4; ++w) { lo = fminf(lo, slo[w]); hi = fmaxf(hi, shi[w]); any_nan |= snan[w] != 0; }
        atomicMin(mm + 0, any_nan ? 0u : f2ord(lo));
        atomicMax(mm + 1, any_nan ? 0xffffffffu : f2ord(hi));
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

// F.interpolate(x[:, None], size=(oh, ow), mode="bilinear") (align_corners=False, no antialias): src = max(0, s*(dst+0.5)-0.5)
// Optionally folds the min/max reduction of the OUTPUT into the same pass (for convert_to_uint8(scale_prediction(x))).
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

// mode 0: fp32 (x - min) / (max - min); mode 1: u8 = trunc(255 * norm) (Tensor.byte()); mode 2: BGRA u8 = 24-bit
// round-half-even(16777215 * norm) split into bytes (B = low, G = mid, R = high; alpha left 0), lossy: high byte only.
// minmax == null: the input is used as is (metric models skip normalize_01, run_3dviewer.py:577-578).
template <int MODE>
__global__ __launch_bounds__(256) void normalize_kernel(const float* __restrict__ in, const float* __restrict__ minmax, void* out, size_t n,
                                                        int lossy) {
    const float lo = minmax ? minmax[0] : 0.0f, hi = minmax ? minmax[1] : 1.0f;
    const float range = hi - lo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = minmax ? (in[i] - lo) / range : in[i];
        if (MODE == 0) {
            ((float*)out)[i] = v;  // NaN (NaN input, or max == min) propagates like the reference's fp32 result
            continue;
        }
        // integer outputs: a NaN (max == min: 0 / 0; NaN anywhere in the map) becomes 0 - converting NaN to an integer is undefined in
        // C and implementation-defined in torch's .byte(); values are clamped to the representable range before the conversion
        v = v == v ? fminf(fmaxf(v, 0.0f), 1.0f) : 0.0f;
        if (MODE == 1) {
            ((unsigned char*)out)[i] = (unsigned char)(int)(255.0f * v);
        } else {
            const int q = (int)rintf(16777215.0f * v);
            uchar4 px;
            px.x = lossy ? 0 : (unsigned char)(q & 255);
            px.y = lossy ? 0 : (unsigned char)((q >> 8) & 255);
            px.z = (unsigned char)((q >> 16) & 255);
            px.w = 0;
            ((uchar4*)out)[i] = px;
        }
    }
}

// ---- per-image display tail (the per-frame loop of the reference's run_video.py:348-361 over a batch): segmented min/max, uint8 + histogram,
// equalization LUT, colormap. Every image of the batch gets its own min/max, histogram and LUT; nothing crosses from one image to another.
// Segmented min/max: grid (SEG_PARTS = MDPT_POST_SEG_PARTS, B); block (x, b) leaves the ordered {min, max} of its share of image b in parts[(b PARTS + x) 2 ..],
// the next kernel reduces the PARTS entries of its image (no atomics, no buffer to clear first). A NaN pins {0, ~0} like block_minmax.
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

__device__ __forceinline__ float ld_dt(const void* p, size_t i, int dt) {
    if (dt == MDPT_DT_BF16) return (float)((const __bf16*)p)[i];
    if (dt == MDPT_DT_F16) return (float)((const _Float16*)p)[i];
    return ((const float*)p)[i];
}

// the value of the map once stored in dtype dt (scale_prediction returns its map in the prediction's dtype, postprocess.py:22-29)
__device__ __forceinline__ float round_dt(float v, int dt) {
    if (dt == MDPT_DT_BF16) return (float)(__bf16)v;
    if (dt == MDPT_DT_F16) return (float)(_Float16)v;
    return v;
}

__device__ __forceinline__ void block_minmax_part(float lo, float hi, bool saw_nan, bool any, unsigned* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    const bool wave_nan = __any(saw_nan), wave_any = __any(any);
    __shared__ float slo[4], shi[4];
    __shared__ int snan[4], sany[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { slo[wave] = lo; shi[wave] = hi; snan[wave] = wave_nan; sany[wave] = wave_any; }
    __syncthreads();
    if (threadIdx.x == 0) {
        bool any_nan = wave_nan, any_px = wave_any;
        for (int w = 1; w < 4; ++w) { lo = fminf(lo, slo[w]); hi = fmaxf(hi, shi[w]); any_nan |= snan[w] != 0; any_px |= sany[w] != 0; }
        part[0] = any_nan ? 0u : (any_px ? f2ord(lo) : 0xffffffffu);  // a share without pixels is neutral
        part[1] = any_nan ? 0xffffffffu : (any_px ? f2ord(hi) : 0u);
    }
}

// out == null: min/max of each input image. Otherwise F.interpolate(bilinear) of each image to its oh x ow (the arithmetic of scale_bilinear_kernel),
// rounded to the input's dtype, stored as fp32 at its place of the packed out, min/max of that. hist_clear != null: zero the [B,256] histogram the
// next kernel accumulates into.
__global__ __launch_bounds__(256) void seg_scale_minmax_kernel(const PostRunTable t, int in_dt, float* __restrict__ out, unsigned* __restrict__ parts,
                                                               unsigned* __restrict__ hist_clear) {
    const int b = blockIdx.y;
    if (hist_clear && blockIdx.x == 0) hist_clear[(size_t)b * 256 + threadIdx.x] = 0u;
    int j;
    const PostRun& img = seg_image(t, b, j);
    const void* in = img.in;
    const int ih = img.ih, iw = img.iw, oh = img.oh, ow = img.ow;
    const bool scale = out != nullptr;
    const size_t n = scale ? (size_t)oh * ow : (size_t)ih * iw;
    const size_t in_base = (size_t)j * ih * iw, out_base = img.off + (size_t)j * oh * ow;
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    float lo = INFINITY, hi = -INFINITY;
    bool saw_nan = false, any = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v;
        if (scale) {
            const int ox = (int)(i % ow), oy = (int)(i / ow);
            // scale_bilinear_kernel's arithmetic as the compiler contracts it there (its gfx950 code: fma for the source position, one fma and one
            // product per row, two products and an add across the rows), spelled out with _rn intrinsics so that no contraction choice here can differ
            const float fy = fmaxf(__fmaf_rn(sy, (float)oy + 0.5f, -0.5f), 0.0f), fx = fmaxf(__fmaf_rn(sx, (float)ox + 0.5f, -0.5f), 0.0f);
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + (y0 < ih - 1), x1 = x0 + (x0 < iw - 1);
            const float ly = fy - (float)y0, lx = fx - (float)x0;
            const float p00 = ld_dt(in, in_base + (size_t)y0 * iw + x0, in_dt), p01 = ld_dt(in, in_base + (size_t)y0 * iw + x1, in_dt);
            const float p10 = ld_dt(in, in_base + (size_t)y1 * iw + x0, in_dt), p11 = ld_dt(in, in_base + (size_t)y1 * iw + x1, in_dt);
            const float top = __fmaf_rn(p01, lx, __fmul_rn(p00, 1.0f - lx)), bot = __fmaf_rn(p10, 1.0f - lx, __fmul_rn(p11, lx));
            v = __fadd_rn(__fmul_rn(1.0f - ly, top), __fmul_rn(ly, bot));
            v = round_dt(v, in_dt);
            out[out_base + i] = v;
        } else {
            v = ld_dt(in, in_base + i, in_dt);
        }
        any = true;
        saw_nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax_part(lo, hi, saw_nan, any, parts + ((size_t)b * SEG_PARTS + blockIdx.x) * 2);
}

// (255 * normalize_01(image b)).byte() with image b's own min/max (normalize_kernel<1>'s arithmetic), optionally 255 - x, and (hist != null) image
// b's 256-bin histogram of the result: LDS-private bins, one integer atomic per non-empty bin and block into hist[b, :]. Image b has ih x iw
// elements; its result goes to its place of the packed out.
__global__ __launch_bounds__(256) void seg_u8_hist_kernel(const PostRunTable t, int in_dt, const unsigned* __restrict__ parts, int reverse,
                                                          unsigned char* __restrict__ out, unsigned* __restrict__ hist) {
    const int b = blockIdx.y;
    int j;
    const PostRun& img = seg_image(t, b, j);
    const void* in = img.in;
    const size_t n = (size_t)img.ih * img.iw;
    __shared__ unsigned bins[256];
    __shared__ unsigned smm[2];
    bins[threadIdx.x] = 0u;
    if (threadIdx.x < 64) {
        unsigned mn = parts[((size_t)b * SEG_PARTS + threadIdx.x) * 2], mx = parts[((size_t)b * SEG_PARTS + threadIdx.x) * 2 + 1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
            mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        }
        if (threadIdx.x == 0) { smm[0] = mn; smm[1] = mx; }
    }
    __syncthreads();
    const float lo = ord2f(smm[0]), hi = ord2f(smm[1]);
    const float range = hi - lo;
    const size_t base = (size_t)j * n, obase = img.off + (size_t)j * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = (ld_dt(in, base + i, in_dt) - lo) / range;
        v = v == v ? fminf(fmaxf(v, 0.0f), 1.0f) : 0.0f;
        int q = (int)(255.0f * v);
        if (reverse) q = 255 - q;
        out[obase + i] = (unsigned char)q;
        if (hist) atomicAdd(&bins[q], 1u);
    }
    if (!hist) return;
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(hist + (size_t)b * 256 + threadIdx.x, bins[threadIdx.x]);
}

// 256-bin histogram per image of a uint8 batch, accumulated into hist[b, :] (same privatisation as above)
__global__ __launch_bounds__(256) void seg_hist_kernel(const unsigned char* __restrict__ in, size_t n, unsigned* __restrict__ hist) {
    const int b = blockIdx.y;
    __shared__ unsigned bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const size_t base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) atomicAdd(&bins[in[base + i]], 1u);
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(hist + (size_t)b * 256 + threadIdx.x, bins[threadIdx.x]);
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

}  // namespace

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
    hipLaunchKernelGGL(seg_scale_minmax_kernel, dim3(SEG_PARTS, B), dim3(256), 0, stream, t, in_dt, out, parts, hist_clear);
    return (int)hipGetLastError();
}

int mdpt_launch_post_seg_u8(const PostRunTable& t, int in_dt, const unsigned* parts, int reverse, unsigned char* out, unsigned* hist, hipStream_t stream) {
    int B;
    size_t n, max_out;
    if (!table_extent(t, B, n, max_out)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("seg_u8_hist_kernel", 0.0, stream);
    hipLaunchKernelGGL(seg_u8_hist_kernel, dim3(grid_for(n) < 256 ? grid_for(n) : 256, B), dim3(256), 0, stream, t, in_dt, parts, reverse, out, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_hist(const unsigned char* in, int B, size_t n, unsigned* hist, hipStream_t stream) {
    MdptProfScope prof("seg_hist_kernel", 0.0, stream);
    hipLaunchKernelGGL(seg_hist_kernel, dim3(grid_for(n) < 256 ? grid_for(n) : 256, B), dim3(256), 0, stream, in, n, hist);
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
    hipLaunchKernelGGL(colorize_kernel, dim3(grid_for(n) < 256 ? grid_for(n) : 256, B), dim3(256), 0, stream, t, eq, cmap, channels, out);
    return (int)hipGetLastError();
}
