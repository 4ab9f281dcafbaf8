// Depth post-processing on the GPU: the step immediately after the DPT forward in the reference's demos
// (muggled_dpt/demo_helpers/postprocess.py:22-29 scale_prediction, :63-74 normalize_01, :79-91 convert_to_uint8;
// run_3dviewer.py:576-590 24-bit packing). HBM-bound streaming kernels: fp32 in, fp32 / u8 out, no host round trip of the
// full-resolution fp32 map. min/max travel through a 2-float device buffer (no sync).

namespace {

__global__ void minmax_init_kernel(unsigned* mm) {
    mm[0] = 0xffffffffu;  // running min (ordered domain)
    mm[1] = 0u;           // running max
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
    if (mode == 0) post_launch("normalize_kernel", normalize_kernel<0>, dim3(grid_for(n)), dim3(256), stream, in, minmax, out, n, lossy);
    else if (mode == 1) post_launch("normalize_kernel", normalize_kernel<1>, dim3(grid_for(n)), dim3(256), stream, in, minmax, out, n, lossy);
    else if (mode == 2) post_launch("normalize_kernel", normalize_kernel<2>, dim3(grid_for(n)), dim3(256), stream, in, minmax, out, n, lossy);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int mdpt_launch_post_seg_minmax(const PostRunTable& t, int in_dt, float* out, unsigned* parts, unsigned* hist_clear, hipStream_t stream) {
    int B;
    size_t max_in, max_out;
    if (!table_extent(t, B, max_in, max_out)) return (int)hipErrorInvalidValue;
    post_launch("seg_scale_minmax_kernel", seg_scale_minmax_kernel<false>, dim3(SEG_PARTS, B), dim3(256), stream, t, in_dt, out, parts, hist_clear);
    return (int)hipGetLastError();
}

int mdpt_launch_post_seg_u8(const PostRunTable& t, int in_dt, const unsigned* parts, int reverse, unsigned char* out, unsigned* hist, hipStream_t stream) {
    int B;
    size_t n, max_out;
    if (!table_extent(t, B, n, max_out)) return (int)hipErrorInvalidValue;
    post_launch("seg_u8_hist_kernel", seg_u8_hist_kernel, dim3(grid_seg(n), B), dim3(256), stream, t, in_dt, parts, reverse, out, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_hist(const unsigned char* in, int B, size_t n, unsigned* hist, hipStream_t stream) {
    post_launch("seg_hist_kernel", seg_hist_kernel, dim3(grid_seg(n), B), dim3(256), stream, in, n, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_eq_lut(const unsigned* hist, int B, const int* bin_of, int vmin, int vmax, unsigned char* lut, hipStream_t stream) {
    post_launch("equalize_lut_kernel", equalize_lut_kernel, dim3(B), dim3(256), stream, hist, bin_of, vmin, vmax, lut);
    return (int)hipGetLastError();
}

int mdpt_launch_post_colorize(const PostRunTable& t, const unsigned char* eq, const unsigned char* cmap, int channels, unsigned char* out,
                              hipStream_t stream) {
    int B;
    size_t n, max_out;
    if (!table_extent(t, B, n, max_out)) return (int)hipErrorInvalidValue;
    post_launch("colorize_kernel", colorize_kernel, dim3(grid_seg(n), B), dim3(256), stream, t, eq, cmap, channels, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_display_prep(const void* in, int dt, int B, int ih, int iw, void* out, int oh, int ow, unsigned* parts, unsigned* hist_clear,
                                  hipStream_t stream) {
    post_launch("disp_prep_kernel", seg_scale_minmax_kernel<true>, dim3(SEG_PARTS, B), dim3(256), stream, uniform_table(in, B, ih, iw, oh, ow), dt, out, parts,
                hist_clear);  // (the label the probes and profiles know the display form by)
    return (int)hipGetLastError();
}

int mdpt_launch_post_block_norm_tiles(const PostRunTable& t, unsigned char* out, float* minmax, hipStream_t stream) {
    int B;
    size_t max_in, max_out;
    if (!table_extent(t, B, max_in, max_out) || max_in > (1u << 24) || max_out > (1u << 24)) return (int)hipErrorInvalidValue;
    for (int r = 0; r < t.n; ++r)
        if (t.run[r].oh % t.run[r].ih || t.run[r].ow % t.run[r].iw) return (int)hipErrorInvalidValue;
    post_launch("block_norm_tiles_kernel", block_norm_tiles_kernel, dim3(B), dim3(256), stream, t, out, minmax);
    return (int)hipGetLastError();
}
