// ---- true depth from ground truth: a prediction aligned to a measured depth map that is partly valid and at its own resolution, scored with the
// standard metrics, and mapped to true depth. The reference's .readme_assets/results_explainer.md gives depth = 1 / (A V + B) ("True depth from DPT
// result") and names two ways to A and B when measurements exist ("Fitting to (more) known data": least squares, or matching the median and the
// spread), with code for neither. A pair is an AlignPair (mdpt_kernels.h); the table lives in device memory and pairs may all differ in size.
// Everything follows the tile fit: fp64, nothing contracted, rounded once, fixed chunks reduced by a fixed tree and added in chunk order by the
// next launch, integer atomics only (the radix select's counts, which do not depend on order), no workgroup waits for or reads another.

namespace {

struct AlignSample { double v, t, g; };

// the prediction at the centre of truth pixel e = Y W + X of pair p (bilinear_f64_at)
__device__ __forceinline__ double align_pred_at(const AlignPair& p, int dt, size_t e) {
    const int Y = (int)(e / (size_t)p.W), X = (int)(e - (size_t)Y * p.W);
    return bilinear_f64_at(p.pred, dt, p.ph, p.pw, (double)X + 0.5, (double)Y + 0.5, p.H, p.W);
}

// THE sample rule of every kernel below: truth pixel e = Y W + X of pair p. g = truth[e] counts if it is finite, > 0, inside [tmin, tmax] (+-inf:
// no bound) and valid[e] != 0 (valid == null: all); v = the prediction at the pixel's centre (align_pred_at) must be finite; t = 1 / g in
// inverse space, g in depth space. (truth is tested first: a pixel without a measurement costs no prediction read)
__device__ __forceinline__ bool align_sample(const AlignPair& p, int dt, int inverse, double tmin, double tmax, size_t e, AlignSample& s) {
#pragma clang fp contract(off)
    const double g = (double)p.truth[e];
    if (!(isfinite(g) && g > 0.0 && g >= tmin && g <= tmax)) return false;
    if (p.valid && p.valid[e] == 0) return false;
    const double v = align_pred_at(p, dt, e);
    if (!isfinite(v)) return false;
    s.v = v;
    s.g = g;
    s.t = inverse ? 1.0 / g : g;
    return true;
}

// least squares (1): blockIdx.y = pair, blockIdx.x = chunk of MDPT_TILE_FIT_CHUNK truth pixels -> {n, Sv, St, Svv, Svt, Stt} of the chunk
__global__ __launch_bounds__(256) void align_fit_partial_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                                double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    chunk_reduce<6>((size_t)p.H * p.W, parts + (size_t)blockIdx.y * max_chunks * 6, [&](size_t e, double (&a)[6]) {
#pragma clang fp contract(off)
        AlignSample s;
        if (align_sample(p, dt, inverse, tmin, tmax, e, s)) {
            a[0] += 1.0; a[1] += s.v; a[2] += s.t;
            a[3] += s.v * s.v; a[4] += s.v * s.t; a[5] += s.t * s.t;
        }
    });
}

// least squares (2): one workgroup per pair (affine_fit_solve): the partials in chunk order -> sums[p], affine_solve -> fit[p] = {A, B}
__global__ __launch_bounds__(64) void align_fit_solve_kernel(const AlignPair* __restrict__ pairs, const double* __restrict__ parts, int max_chunks,
                                                             double* __restrict__ sums, double* __restrict__ fit) {
    const int p = blockIdx.x;
    affine_fit_solve(parts + (size_t)p * max_chunks * 6, tile_fit_chunks((size_t)pairs[p].H * pairs[p].W), p, sums, fit);
}

// ---- the median fit: exact medians of the float32 roundings v32, t32 of the samples by a radix select over the ordered 32-bit keys (f2ord), 8 bits
// a pass from the top. A pass is a histogram launch (every workgroup counts the digits of its samples in LDS and flushes the non-zero bins with
// integer atomics) and a select launch (one workgroup per pair narrows the key prefix of BOTH middle ranks, (n - 1) / 2 and n / 2, of both streams,
// and clears the pair's bins for the next pass). Bins: hist[p][2 s + r][256], s = 0 v / 1 t, r = the rank's track; while the two tracks of a stream
// share their prefix only track 0 is counted. State: state[p][0..3] the prefixes, [4..7] the ranks left inside the prefix, [8] n. The samples are
// recomputed in every pass (see DESIGN.md): nothing per pixel is stored.

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
        const unsigned key[2] = {f2ord((float)s.v), f2ord((float)s.t)};
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
            out = n == 0 ? 0.0 : ((double)ord2f(key[q]) + (double)ord2f(key[q + 1])) * 0.5;
        }
        sums[(size_t)blockIdx.x * 6 + threadIdx.x] = out;
    }
}

// mean absolute deviation (1): as align_fit_partial_kernel, {sum |v32 - med v|, sum |t32 - med t|} of the chunk
__global__ __launch_bounds__(256) void align_mad_partial_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                                const double* __restrict__ sums, double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    const double mv = sums[(size_t)blockIdx.y * 6 + 1], mt = sums[(size_t)blockIdx.y * 6 + 2];
    chunk_reduce<2>((size_t)p.H * p.W, parts + (size_t)blockIdx.y * max_chunks * 2, [&](size_t e, double (&a)[2]) {
#pragma clang fp contract(off)
        AlignSample s;
        if (align_sample(p, dt, inverse, tmin, tmax, e, s)) {
            a[0] += fabs((double)(float)s.v - mv);
            a[1] += fabs((double)(float)s.t - mt);
        }
    });
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
    const double A = fit ? fit[2 * (size_t)blockIdx.y] : 1.0, B = fit ? fit[2 * (size_t)blockIdx.y + 1] : 0.0;
    chunk_reduce<ALIGN_METRIC_SUMS>((size_t)p.H * p.W, parts + (size_t)blockIdx.y * max_chunks * ALIGN_METRIC_SUMS,
                                    [&](size_t e, double (&a)[ALIGN_METRIC_SUMS]) {
#pragma clang fp contract(off)
        AlignSample s;
        if (!align_sample(p, dt, inverse, tmin, tmax, e, s)) return;
        a[0] += 1.0;
        const double q = A * s.v + B;
        if (!(q > 0.0)) {
            a[1] += 1.0;
            return;
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
    });
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

// q = A v + B -> true depth (align_apply_kernel and the local fit's apply): d = 1 / q in inverse space (q <= 0: +inf), q in depth space; then clamped
// to [dmin, dmax] where those are finite, rounded to fp32 once. NaN stays NaN.
__device__ __forceinline__ float align_depth_of(double q, int inverse, double dmin, double dmax) {
#pragma clang fp contract(off)
    double d = inverse ? (q <= 0.0 ? (double)INFINITY : 1.0 / q) : q;
    if (isfinite(dmin) && d < dmin) d = dmin;
    if (isfinite(dmax) && d > dmax) d = dmax;
    return (float)d;
}

// true depth: out pixel (Y, X) of pair p's H x W output (at out + offs[p]) = the prediction at the pixel's centre, q = A v + B -> align_depth_of
__global__ __launch_bounds__(256) void align_apply_kernel(const AlignPair* __restrict__ pairs, int dt, int inverse, const double* __restrict__ fit,
                                                          const long long* __restrict__ offs, double dmin, double dmax, float* __restrict__ out) {
#pragma clang fp contract(off)
    const AlignPair p = pairs[blockIdx.y];
    const size_t n = (size_t)p.H * p.W;
    const double A = fit ? fit[2 * (size_t)blockIdx.y] : 1.0, B = fit ? fit[2 * (size_t)blockIdx.y + 1] : 0.0;
    float* o = out + offs[blockIdx.y];
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        o[e] = align_depth_of(A * align_pred_at(p, dt, e) + B, inverse, dmin, dmax);
    }
}

}  // namespace

int mdpt_launch_post_align_fit(const AlignPair* pairs, int P, int max_chunks, int dt, int inverse, int median, double tmin, double tmax, double* parts,
                               unsigned* hist, unsigned* state, double* sums, double* fit, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_chunks <= 0 || max_chunks >= (1 << 24)) return (int)hipErrorInvalidValue;
    if (!median) {
        post_launch("align_fit_partial_kernel", align_fit_partial_kernel, dim3(max_chunks, P), dim3(256), stream, pairs, dt, inverse, tmin, tmax, parts,
                    max_chunks);
        post_launch("align_fit_solve_kernel", align_fit_solve_kernel, dim3(P), dim3(64), stream, pairs, parts, max_chunks, sums, fit);
        return (int)hipGetLastError();
    }
    // 1 clear + 4 x (histogram, select) + the deviation's partial and solve = 11 launches
    post_launch("align_select_clear_kernel", align_select_clear_kernel, dim3(P), dim3(256), stream, hist, state);
    const int hist_blocks = align_stride_blocks((size_t)max_chunks * MDPT_TILE_FIT_CHUNK);
    for (int shift = 24; shift >= 0; shift -= 8) {
        post_launch("align_hist_kernel", align_hist_kernel, dim3(hist_blocks, P), dim3(256), stream, pairs, dt, inverse, tmin, tmax, state,
                    hist, shift);
        post_launch("align_select_kernel", align_select_kernel, dim3(P), dim3(256), stream, hist, state, shift, sums);
    }
    post_launch("align_mad_partial_kernel", align_mad_partial_kernel, dim3(max_chunks, P), dim3(256), stream, pairs, dt, inverse, tmin, tmax,
                sums, parts, max_chunks);
    post_launch("align_mad_solve_kernel", align_mad_solve_kernel, dim3(P), dim3(64), stream, pairs, parts, max_chunks, sums, fit);
    return (int)hipGetLastError();
}

int mdpt_launch_post_align_metrics(const AlignPair* pairs, int P, int max_chunks, int dt, int inverse, double tmin, double tmax, const double* fit,
                                   double* parts, double* metrics, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_chunks <= 0 || max_chunks >= (1 << 24)) return (int)hipErrorInvalidValue;
    post_launch("align_metrics_partial_kernel", align_metrics_partial_kernel, dim3(max_chunks, P), dim3(256), stream, pairs, dt, inverse, tmin, tmax, fit,
                parts, max_chunks);
    post_launch("align_metrics_solve_kernel", align_metrics_solve_kernel, dim3(P), dim3(64), stream, pairs, parts, max_chunks, metrics);
    return (int)hipGetLastError();
}

int mdpt_launch_post_align_apply(const AlignPair* pairs, int P, size_t max_pixels, int dt, int inverse, const double* fit, const long long* offs, double dmin,
                                 double dmax, float* out, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_pixels == 0 || max_pixels >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    // (the blocks of a pair stride over its output pixels, 256 at a time: one block per 2048 pixels of the largest output, capped)
    const int blocks = align_stride_blocks(max_pixels);
    post_launch("align_apply_kernel", align_apply_kernel, dim3(blocks, P), dim3(256), stream, pairs, dt, inverse, fit, offs, dmin, dmax, out);
    return (int)hipGetLastError();
}
