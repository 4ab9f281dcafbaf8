// What more than one post-processing feature uses (postprocess.hip includes this file first): ordered float keys, the block reductions, the chunked
// fp64 reduction of the fits, the resamplers shared between features, and the launch helper.

namespace {

// float <-> key whose unsigned order is the float order (-0.0 before +0.0): atomicMin / atomicMax on unsigned work for any sign, and the radix
// select of the median fit walks the keys' digits from the top
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
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

// The chunked reduction of the fits, bit-deterministic without atomics: workgroup (blockIdx.x = chunk c, blockIdx.y = record) reduces samples
// [c CHUNK, (c + 1) CHUNK) of the record's n - each thread its MDPT_TILE_FIT_CHUNK / 256 = 8 strided samples in order, sample(e, a) adding sample e
// to the thread's K sums, then block_sum_f64's fixed tree - into row[c K ..], `row` being the record's parts[max_chunks][K]. A chunk past n does
// nothing (uniform over the block, before any barrier: the grid's x extent is that of the largest record). chunk_order_sum adds the chunks up.
// chunk_reduce_at: the same for a workgroup whose chunk c is not its blockIdx.x (the local fit's grid folds cell and chunk into x); `o` = where the
// chunk's K sums go.
template <int K, typename Sample>
__device__ __forceinline__ void chunk_reduce_at(size_t chunk, size_t n, double* __restrict__ o, Sample&& sample) {
    const size_t base = chunk * MDPT_TILE_FIT_CHUNK;
    if (base >= n) return;
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    for (int k = 0; k < MDPT_TILE_FIT_CHUNK / 256; ++k) {
        const size_t e = base + (size_t)k * 256 + threadIdx.x;
        if (e >= n) break;
        sample(e, a);
    }
    block_sum_f64<K>(a);
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) o[k] = a[k];
}
template <int K, typename Sample>
__device__ __forceinline__ void chunk_reduce(size_t n, double* __restrict__ row, Sample&& sample) {
    chunk_reduce_at<K>((size_t)blockIdx.x, n, row + (size_t)blockIdx.x * K, sample);
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

// the body of both least-squares solve kernels (one workgroup per record i): the record's six partial sums in chunk order -> sums[i],
// affine_solve -> fit[i] = {scale, shift}
__device__ __forceinline__ void affine_fit_solve(const double* __restrict__ row, size_t chunks, int i, double* __restrict__ sums, double* __restrict__ fit) {
    __shared__ double s[6];
    chunk_order_sum<6>(row, chunks, s);
    if (threadIdx.x < 6) sums[(size_t)i * 6 + threadIdx.x] = s[threadIdx.x];
    if (threadIdx.x != 0) return;
    double scale, shift;
    affine_solve(s[0], s[1], s[2], s[3], s[4], scale, shift);
    fit[2 * (size_t)i] = scale;
    fit[2 * (size_t)i + 1] = shift;
}

// torch's reflect padding index (no edge repeat) for offsets up to n - 1 past either end; clamped so that no index leaves the map
__device__ __forceinline__ int reflect_idx(int v, int n) {
    v = v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v);
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}

// cv2.resize(INTER_LINEAR) restated per axis (the depth masks' cutout and composite, the tile blend): p = float((d + 0.5) scale - 0.5) with
// scale = 1 / (out / in) in fp64 (cv2's own form), s = floor(p), a = p - s in fp32; s < 0 -> s = 0, a = 0; s >= in - 1 -> s = in - 1, a = 0.
// CV_64F (lerp_cv64): weights (1 - a, a) in fp32, sums in fp64, rows first, then across them.
struct CvTap { int s0, s1; float a; };
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

// a map (gh x gw of dtype gdt) covering an H x W frame, at frame position (X, Y): bilinear at u = X gw / W - 0.5, v = Y gh / H - 0.5, clamped to the
// map; fp64 weights, rows first. The one resampler of the fits: the tile fit reads its guide through it (tile_fit_partial_kernel), the true-depth block
// its prediction at the centre of a ground-truth pixel (align_pred_at), the guided upsampling its mean coefficients at the centre of a
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

// What the per-photo features over a pair table (refocus, normals) share. The map at the centre of photo pixel (Y, X) of an H x W photo: a map of the
// photo's size is read directly, so that it comes through unchanged whatever its neighbours hold
__device__ __forceinline__ double map_at_pixel_centre(const void* map, int dt, int h, int w, int H, int W, int Y, int X) {
    if (h == H && w == W) return (double)ld_dt(map, (size_t)Y * w + X, dt);
    return bilinear_f64_at(map, dt, h, w, (double)X + 0.5, (double)Y + 0.5, H, W);
}

// share `share` of `shares` (workgroups of 256 threads) of the fp32 min / max of the FINITE values of a map of n elements -> part[0..1] as ordered
// keys (a share without a finite value stores the neutral {~0, 0})
__device__ __forceinline__ void finite_minmax_part(const void* map, size_t n, int dt, unsigned share, unsigned shares, unsigned* part) {
    float lo = INFINITY, hi = -INFINITY;
    bool any = false;
    for (size_t i = (size_t)share * 256 + threadIdx.x; i < n; i += (size_t)shares * 256) {
        const float v = ld_dt(map, i, dt);
        if (isfinite(v)) {
            lo = fminf(lo, v), hi = fmaxf(hi, v);
            any = true;
        }
    }
    block_minmax_part(lo, hi, false, any, part);
}

// the reduced ordered keys of those partials -> lo, hi as fp64 (a zero takes the sign +; a map without a finite value: 0, 0) and whether hi > lo
__device__ __forceinline__ bool finite_range(unsigned lo_o, unsigned hi_o, double& lo, double& hi) {
#pragma clang fp contract(off)
    const bool any = lo_o <= hi_o;  // (a map without a finite value leaves the neutral partials {~0, 0})
    lo = any ? (double)ord2f(lo_o) + 0.0 : 0.0;
    hi = any ? (double)ord2f(hi_o) + 0.0 : 0.0;
    return any && hi > lo;
}

// the pair that owns tile `tile` of a call: the last record whose tile_off (the tiles of the pairs before it) is not beyond it; `off`: the field that
// counts them, for a record with more than one tiling
template <typename Pair>
__device__ __forceinline__ int pair_of_tile(const Pair* __restrict__ pairs, int P, long long tile, long long Pair::*off = &Pair::tile_off) {
    int a = 0, b = P - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (pairs[mid].*off <= tile) a = mid;
        else b = mid - 1;
    }
    return a;
}

inline int grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// the x extent of a (blocks, images) grid
inline int grid_seg(size_t n) { return grid_for(n) < 256 ? grid_for(n) : 256; }

// one launch under its profiler label (the scope closes after the launch; the arguments convert to the kernel's parameter types)
template <typename... Params, typename... Args>
inline void post_launch(const char* label, void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t stream, Args&&... args) {
    MdptProfScope prof(label, 0.0, stream);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<Params>(args)...);
}

}  // namespace
