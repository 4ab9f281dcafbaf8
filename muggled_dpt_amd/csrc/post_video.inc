// ---- temporally stable video depth (not in the reference, whose run_video.py normalises every frame on its own): the relative-depth families return
// each map up to a scale and a shift of its own, so a clip pumps in brightness and shimmers. Three stages, all on the device, nothing read back:
// (1) a robust affine fit a_t P_t + b_t ~ P_{t-1} of every frame to its predecessor (iteratively reweighted least squares, Cauchy weights) and the
// chain (A_t, B_t) that composes the fits; (2) a temporal filter of the aligned frames that averages small differences and lets large ones through;
// (3) the display tail with a range carried from frame to frame in place of each frame's own min / max. Everything follows the tile and true-depth
// fits: fp64, nothing contracted, rounded once, fixed chunks reduced by a fixed tree and added in chunk order by the next launch, no atomics, no
// workgroup waits for or reads another.

namespace {

// the record of a pair between the rounds of its fit: {a, b, s2, status}
constexpr int VIDEO_REC = 4;
constexpr double VIDEO_RUN = 0.0, VIDEO_EXACT = 1.0, VIDEO_CUT = 2.0, VIDEO_START = 3.0;  // status: the fit goes on / is kept / the chain re-anchors

// the T frames of a call ([T, hw] of dtype dt), the raw last frame of the call before ([hw], same dtype) and whether there was one (started[0] != 0)
struct VideoClip { const void* frames; const void* prev; const int* started; int dt, T; size_t hw; };

// fit (1): blockIdx.y = frame t, blockIdx.x = chunk of MDPT_TILE_FIT_CHUNK pixels -> the chunk's weighted {n, Sx, Sy, Sxx, Sxy, Syy}, x = P_t, y = P_{t-1},
// over the pixels where both are finite. Round 0: w = 1; round k: w = 1 / (1 + r^2 / (c^2 s^2)), r = a x + b - y, {a, b, s^2} of round k - 1 (rec).
// A pair whose fit is kept (exact, cut, start) does nothing.
__global__ __launch_bounds__(256) void video_fit_partial_kernel(const VideoClip v, int round, double c2, const double* __restrict__ rec,
                                                                double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const int t = blockIdx.y;
    if (t == 0 && v.started[0] == 0) return;  // (uniform over the block, before any barrier)
    double a = 1.0, b = 0.0, c2s2 = 1.0;
    if (round > 0) {
        const double* r = rec + (size_t)t * VIDEO_REC;
        if (r[3] != VIDEO_RUN) return;
        a = r[0];
        b = r[1];
        c2s2 = c2 * r[2];
    }
    const void* y = t == 0 ? v.prev : v.frames;
    const size_t xb = (size_t)t * v.hw, yb = t == 0 ? 0 : (size_t)(t - 1) * v.hw;
    chunk_reduce<6>(v.hw, parts + (size_t)t * max_chunks * 6, [&](size_t e, double (&s)[6]) {
#pragma clang fp contract(off)
        const double px = (double)ld_dt(v.frames, xb + e, v.dt), py = (double)ld_dt(y, yb + e, v.dt);
        if (!(isfinite(px) && isfinite(py))) return;
        double w = 1.0;
        if (round > 0) {
            const double r = (a * px + b) - py;
            w = 1.0 / (1.0 + (r * r) / c2s2);
        }
        const double wx = w * px, wy = w * py;
        s[0] += w; s[1] += wx; s[2] += wy;
        s[3] += wx * px; s[4] += wx * py; s[5] += wy * py;
    });
}

// fit (2): one workgroup per frame: the partials in chunk order -> sums (where asked for: this round's [T, 6]; a kept pair repeats the sums it was
// kept with, a start has zeros), then var = n Sxx - Sx^2, cov = n Sxy - Sx Sy, a = cov / var, b = (Sy - a Sx) / n, s^2 = max(0, (Syy - a Sxy - b Sy) / n)
// -> rec. Cut: fewer than two samples (round 0, where n counts them), var <= 0, a <= 0, a result that is not finite - in any round - and, once the
// fit is final (the last round, or exact), var_y <= 0 or cov^2 < cut_corr^2 var var_y. Exact: s^2 <= 2^-40 Syy / n.
__global__ __launch_bounds__(64) void video_fit_solve_kernel(const int* __restrict__ started, const double* __restrict__ parts, size_t chunks, int max_chunks,
                                                             int round, int last, double cut_corr2, double* __restrict__ rec, double* __restrict__ sums,
                                                             const double* __restrict__ sums_before) {
#pragma clang fp contract(off)
    const int t = blockIdx.x;
    double* r = rec + (size_t)t * VIDEO_REC;
    const bool start = t == 0 && started[0] == 0;
    if (start || (round > 0 && r[3] != VIDEO_RUN)) {  // (uniform over the block)
        if (sums && threadIdx.x < 6) sums[(size_t)t * 6 + threadIdx.x] = round > 0 ? sums_before[(size_t)t * 6 + threadIdx.x] : 0.0;
        if (round == 0 && threadIdx.x == 0) { r[0] = 1.0; r[1] = 0.0; r[2] = 0.0; r[3] = VIDEO_START; }
        return;
    }
    __shared__ double s[6];
    chunk_order_sum<6>(parts + (size_t)t * max_chunks * 6, chunks, s);
    if (sums && threadIdx.x < 6) sums[(size_t)t * 6 + threadIdx.x] = s[threadIdx.x];
    if (threadIdx.x != 0) return;
    const double n = s[0], sx = s[1], sy = s[2], sxx = s[3], sxy = s[4], syy = s[5];
    const double var = n * sxx - sx * sx, cov = n * sxy - sx * sy;
    const double a = cov / var, b = (sy - a * sx) / n;
    const double s2 = fmax(0.0, (syy - a * sxy - b * sy) / n);
    double status = VIDEO_RUN;
    if ((round == 0 && !(n >= 2.0)) || !(var > 0.0) || !(a > 0.0) || !(isfinite(a) && isfinite(b) && isfinite(s2))) {
        status = VIDEO_CUT;
    } else {
        if (s2 <= 0x1p-40 * syy / n) status = VIDEO_EXACT;
        if (last || status == VIDEO_EXACT) {
            const double var_y = n * syy - sy * sy;
            if (!(var_y > 0.0) || cov * cov < cut_corr2 * (var * var_y)) status = VIDEO_CUT;
        }
    }
    r[0] = a; r[1] = b; r[2] = s2; r[3] = status;
}

// fit (3): the chain, one lane, in order from the state's (A, B): A_t = A_{t-1} a_t, B_t = A_{t-1} b_t + B_{t-1}, sigma_t = A_{t-1} s_t; a start, a cut, a
// result that is not finite or an A_t outside [2^-20, 2^20] re-anchors: {1, 0, 0, cut = 1} -> table [T, 4], ab_out = the last (A, B)
__global__ void video_chain_kernel(const double* __restrict__ rec, int T, const double* __restrict__ ab_in, const int* __restrict__ started,
                                   double* __restrict__ table, double* __restrict__ ab_out) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double A = 1.0, B = 0.0;
    if (started[0] != 0) { A = ab_in[0]; B = ab_in[1]; }
    for (int t = 0; t < T; ++t) {
        const double* r = rec + (size_t)t * VIDEO_REC;
        bool cut = r[3] >= VIDEO_CUT;
        double An = 1.0, Bn = 0.0, sg = 0.0;
        if (!cut) {
            An = A * r[0];
            Bn = A * r[1] + B;
            sg = A * sqrt(r[2]);
            cut = !(isfinite(An) && isfinite(Bn) && isfinite(sg)) || An < 0x1p-20 || An > 0x1p20;
            if (cut) { An = 1.0; Bn = 0.0; sg = 0.0; }
        }
        double* o = table + (size_t)t * 4;
        o[0] = An; o[1] = Bn; o[2] = sg; o[3] = cut ? 1.0 : 0.0;
        A = An;
        B = Bn;
    }
    ab_out[0] = A;
    ab_out[1] = B;
}

// N consecutive pixels of a frame as floats: one load of N elements where the frames allow it (vec), else N loads
template <int N>
__device__ __forceinline__ void video_load(const void* p, size_t i, int dt, bool vec, float (&v)[N]) {
    if constexpr (N == 4) if (vec) {
        if (dt == MDPT_DT_F32) {
            const float4 q = *(const float4*)((const float*)p + i);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const uint2 q = *(const uint2*)((const unsigned short*)p + i);
            const unsigned short h[4] = {(unsigned short)(q.x & 0xffffu), (unsigned short)(q.x >> 16), (unsigned short)(q.y & 0xffffu), (unsigned short)(q.y >> 16)};
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (dt == MDPT_DT_BF16) {
                    v[j] = __uint_as_float((unsigned)h[j] << 16);
                } else {
                    _Float16 f;
                    __builtin_memcpy(&f, &h[j], 2);
                    v[j] = (float)f;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = ld_dt(p, i + j, dt);
}

template <int N>
__device__ __forceinline__ void video_store(float* p, size_t i, bool vec, const float (&v)[N]) {
    if constexpr (N == 4) if (vec) {
        *(float4*)(p + i) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) p[i + j] = v[j];
}

// the filter of pixels [i, i + N) over the T frames, the previous output in registers: s = A_t p + B_t; a cut, or a previous output or a p that is not
// finite: o = s; else d = s - o_prev, g = d^2 / (d^2 + (tau sigma_t)^2) (0 / 0: 0), k = alpha + (1 - alpha) g, o = o_prev + k d (k == 1: s); fp64, rounded
// once to fp32, and that fp32 is the next o_prev
template <int N>
__device__ __forceinline__ void video_filter_pixels(const void* __restrict__ frames, int dt, int T, size_t hw, size_t i, bool vec,
                                                    const double* __restrict__ table, const float* __restrict__ prev_out, double alpha, double tau,
                                                    float* __restrict__ out) {
#pragma clang fp contract(off)
    float o[N], p[N];
    video_load<N>(prev_out, i, MDPT_DT_F32, vec, o);
    for (int t = 0; t < T; ++t) {
        const double A = table[4 * (size_t)t], B = table[4 * (size_t)t + 1], ts = tau * table[4 * (size_t)t + 2];
        const bool cut = table[4 * (size_t)t + 3] != 0.0;
        const double ts2 = ts * ts;
        video_load<N>(frames, (size_t)t * hw + i, dt, vec, p);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double s = A * (double)p[j] + B;
            float r = (float)s;
            if (!cut && isfinite(o[j]) && isfinite(p[j])) {
                const double op = (double)o[j], d = s - op, d2 = d * d, den = d2 + ts2;
                const double g = den > 0.0 ? d2 / den : 0.0;
                const double k = alpha + (1.0 - alpha) * g;
                if (k != 1.0) r = (float)(op + k * d);
            }
            o[j] = r;
        }
        video_store<N>(out, (size_t)t * hw + i, vec, o);
    }
}

// parallel over pixels, sequential over frames: a lane takes 4 consecutive pixels of the flat frame (one 16-byte load of fp32, 8 bytes of bf16 / fp16,
// one 16-byte store, where hw is a multiple of 4 and the buffers are aligned: vec), the hw % 4 pixels left over get a lane each
__global__ __launch_bounds__(256) void video_filter_kernel(const void* __restrict__ frames, int dt, int T, size_t hw, int vec,
                                                           const double* __restrict__ table, const float* __restrict__ prev_out, double alpha, double tau,
                                                           float* __restrict__ out) {
    const size_t groups = hw / 4, lanes = groups + (hw - 4 * groups);
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= lanes) return;
    if (id < groups) video_filter_pixels<4>(frames, dt, T, hw, 4 * id, vec != 0, table, prev_out, alpha, tau, out);
    else video_filter_pixels<1>(frames, dt, T, hw, 4 * groups + (id - groups), false, table, prev_out, alpha, tau, out);
}

// the carried display range, one wave, in order: {m_t, M_t} = frame t's min / max from its SEG_PARTS partials; lo_t = lo_{t-1} + rho (m_t - lo_{t-1}) in
// fp64, rounded to fp32, hi alike; the frame's own {m_t, M_t} at a cut, without a range before, with rho == 1, and where any of the four is not
// finite -> rparts [T, SEG_PARTS, 2]: every partial of frame t = the ordered {lo_t, hi_t} (a NaN pins {0, ~0} as block_minmax_part does), which
// seg_u8_hist_kernel reduces to just that pair; ranges [T, 2] (null: not wanted); range_out = the last pair
__global__ __launch_bounds__(64) void video_range_kernel(const unsigned* __restrict__ parts, int T, const double* __restrict__ table,
                                                         const float* __restrict__ range_in, const int* __restrict__ started, double rho,
                                                         unsigned* __restrict__ rparts, float* __restrict__ ranges, float* __restrict__ range_out) {
#pragma clang fp contract(off)
    float lo = range_in[0], hi = range_in[1];
    bool have = started[0] != 0;
    for (int t = 0; t < T; ++t) {
        unsigned mn = parts[((size_t)t * SEG_PARTS + threadIdx.x) * 2], mx = parts[((size_t)t * SEG_PARTS + threadIdx.x) * 2 + 1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
            mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        }
        const float m = ord2f(mn), M = ord2f(mx);
        if (!have || table[4 * (size_t)t + 3] != 0.0 || rho == 1.0 || !(isfinite(m) && isfinite(M) && isfinite(lo) && isfinite(hi))) {
            lo = m;
            hi = M;
        } else {
            lo = (float)((double)lo + rho * ((double)m - (double)lo));
            hi = (float)((double)hi + rho * ((double)M - (double)hi));
        }
        have = true;
        rparts[((size_t)t * SEG_PARTS + threadIdx.x) * 2] = lo != lo ? 0u : f2ord(lo);
        rparts[((size_t)t * SEG_PARTS + threadIdx.x) * 2 + 1] = hi != hi ? 0xffffffffu : f2ord(hi);
        if (ranges && threadIdx.x == 0) { ranges[2 * (size_t)t] = lo; ranges[2 * (size_t)t + 1] = hi; }
    }
    if (threadIdx.x == 0) { range_out[0] = lo; range_out[1] = hi; }
}

}  // namespace

// 2 (rounds + 1) + 1 launches: a partial and a solve per round, then the chain. scratch = [T, max_chunks, 6] fp64 partials, then [T, VIDEO_REC] records
int mdpt_launch_post_video_fit(const void* frames, int dt, int T, size_t hw, const void* prev, const double* ab_in, const int* started, int rounds, double c,
                               double cut_corr, double* table, double* ab_out, double* sums, double* scratch, hipStream_t stream) {
    const size_t chunks = tile_fit_chunks(hw);
    if (T <= 0 || T > 65535 || chunks == 0 || chunks >= ((size_t)1 << 24) || rounds < 0) return (int)hipErrorInvalidValue;
    const VideoClip v{frames, prev, started, dt, T, hw};
    double* parts = scratch;
    double* rec = scratch + (size_t)T * chunks * 6;
    for (int k = 0; k <= rounds; ++k) {
        double* sk = sums ? sums + (size_t)k * T * 6 : nullptr;
        post_launch("video_fit_partial_kernel", video_fit_partial_kernel, dim3((unsigned)chunks, T), dim3(256), stream, v, k, c * c, rec, parts, (int)chunks);
        post_launch("video_fit_solve_kernel", video_fit_solve_kernel, dim3(T), dim3(64), stream, started, parts, chunks, (int)chunks, k, k == rounds,
                    cut_corr * cut_corr, rec, sk, sk && k > 0 ? sk - (size_t)T * 6 : nullptr);
    }
    post_launch("video_chain_kernel", video_chain_kernel, dim3(1), dim3(64), stream, rec, T, ab_in, started, table, ab_out);
    return (int)hipGetLastError();
}

// one launch
int mdpt_launch_post_video_filter(const void* frames, int dt, int T, size_t hw, const double* table, const float* prev_out, double alpha, double tau, float* out,
                                  hipStream_t stream) {
    if (T <= 0 || hw == 0 || hw >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const size_t elt = dt == MDPT_DT_F32 ? 4 : 2;
    const bool vec = hw % 4 == 0 && ((uintptr_t)frames & (4 * elt - 1)) == 0 && (((uintptr_t)prev_out | (uintptr_t)out) & 15) == 0;
    const size_t lanes = hw / 4 + hw % 4;
    post_launch("video_filter_kernel", video_filter_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), stream, frames, dt, T, hw, (int)vec, table,
                prev_out, alpha, tau, out);
    return (int)hipGetLastError();
}

// four launches: resize + per-frame min / max, the carried range, uint8 (+ reverse), colormap; the first, third and fourth are depth_to_color's own.
// scaled = fp32 [T, oh, ow] (null: no resize, oh x ow = h x w), parts / rparts = [T, SEG_PARTS, 2], u8 = [T, oh, ow]
int mdpt_launch_post_video_display(const float* stable, int T, int h, int w, int oh, int ow, const double* table, const float* range_in, const int* started,
                                   double rho, int reverse, const unsigned char* cmap, float* scaled, unsigned* parts, unsigned* rparts, unsigned char* u8,
                                   unsigned char* out, float* ranges, float* range_out, hipStream_t stream) {
    if ((size_t)oh * ow > (size_t)INT32_MAX) return (int)hipErrorInvalidValue;
    int rc = mdpt_launch_post_seg_minmax(uniform_table(stable, T, h, w, oh, ow), MDPT_DT_F32, scaled, parts, nullptr, stream);
    if (rc) return rc;
    post_launch("video_range_kernel", video_range_kernel, dim3(1), dim3(64), stream, parts, T, table, range_in, started, rho, rparts, ranges, range_out);
    const int n = oh * ow;
    rc = mdpt_launch_post_seg_u8(uniform_table(scaled ? (const void*)scaled : (const void*)stable, T, 1, n, 1, n), MDPT_DT_F32, rparts, reverse, u8, nullptr,
                                 stream);
    if (rc) return rc;
    return mdpt_launch_post_colorize(uniform_table(u8, T, 1, n, 1, n), nullptr, cmap, 3, out, stream);
}
