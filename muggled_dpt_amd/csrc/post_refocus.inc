// ---- synthetic depth of field ("portrait mode"): a photo refocused by its depth map. A focal plane is put where the caller says, every photo pixel
// gets a blur radius from its signed defocus, and the blur is a per-pixel, occlusion-aware gather: scatter-as-gather with depth order. A pair is a
// RefocusPair (mdpt_kernels.h); the table lives in device memory and pairs may all differ in size. Four launches whatever the number of pairs:
//   (1) refocus_minmax_kernel .... the fp32 min / max of the FINITE values of every map, 64 workgroups a map -> ordered-key partials in the pair's header
//   (2) refocus_state_kernel ..... one workgroup a pair: the partials -> lo, hi (a zero takes the sign +); the focal value (given, or read at the pointed
//                                  photo pixel); whether the pair is live (else e = 0 everywhere and the photo comes back byte for byte); the pixels
//                                  of the pairs before it (where the planes are asked for)
//   (3) refocus_prepare_kernel ... per photo pixel (Y, X): s = the map at the pixel's centre (bilinear_f64_at; a map of the photo's size is read
//                                  directly, so that it comes through unchanged whatever its neighbours hold), the signed defocus
//                                  e = (s - lo) / (hi - lo) - focus (inverse space) or (s > 0 ? 1 / s : 0) - 1 / focus (depth space), e = 0 where s is
//                                  not finite, r = min(max_radius, aperture max(0, |e| - focus_range / 2)), rq = floor(4 r)
//                                  -> 8 bytes: B | G << 8 | R << 16 | rq << 24 and e32 = fp32(e)
//   (4) refocus_gather_kernel .... the hot path. One workgroup of 1024 threads owns a 32 x 32 tile of output pixels, one thread each, and stages the
//                                  tile and max_radius texels of halo into LDS once (a texel outside the photo: rq = 0, e32 = -inf, which no rule
//                                  below lets cover a pixel). k(q) = (rq rq) >> 4 is the squared radius of q's lattice disc, N(k) its number of lattice
//                                  points. For output pixel p over the taps q = p + (dy, dx), dy outer, dx inner, both ascending:
//                                  k_eff = e32(q) > e32(p) ? k(q) : min(k(q), k(p)); where dx^2 + dy^2 <= k_eff the tap adds w B, w G, w R, w with
//                                  w = 1.0 / N(k_eff) to four fp64 sums (product, then add); out = floor(sum_c / sum_w + 0.5).
//                                  The loop runs over the disc of the tile's largest k (tile and halo) only - a tap that cannot cover adds nothing,
//                                  so the window changes no bit - and a tile whose largest k is 0 copies its pixels.
// All fp64, nothing contracted. Bit-deterministic, no atomics, no workgroup waits for another, nothing read back; a launch boundary separates every
// producer from its consumer. Choices where the definition is silent: in depth space a NON-FINITE s (NaN, +-inf) gives e = 0 like everywhere else
// and a finite s <= 0 is infinitely far (u = 0); lo and hi take +0 for a zero of either sign.

namespace {

constexpr int REFOCUS_MAX_K = REFOCUS_MAX_RADIUS * REFOCUS_MAX_RADIUS;  // the largest k: rq <= 4 max_radius

// N(k), k = 0 .. 1024: the lattice points (dx, dy) with dx^2 + dy^2 <= k, counted at compile time as exact integers (N(0) = 1, N(1) = 5, N(2) = 9, N(4) = 13)
struct RefocusCounts { unsigned n[REFOCUS_MAX_K + 1]; };
constexpr RefocusCounts refocus_counts() {
    RefocusCounts c{};
    for (int dy = -REFOCUS_MAX_RADIUS; dy <= REFOCUS_MAX_RADIUS; ++dy)
        for (int dx = -REFOCUS_MAX_RADIUS; dx <= REFOCUS_MAX_RADIUS; ++dx)
            if (dx * dx + dy * dy <= REFOCUS_MAX_K) c.n[dx * dx + dy * dy] += 1;
    for (int k = 1; k <= REFOCUS_MAX_K; ++k) c.n[k] += c.n[k - 1];
    return c;
}
__constant__ RefocusCounts refocus_n = refocus_counts();
static_assert(refocus_counts().n[0] == 1 && refocus_counts().n[1] == 5 && refocus_counts().n[2] == 9 && refocus_counts().n[4] == 13 &&
              refocus_counts().n[REFOCUS_MAX_K] == 3209, "N(k) of the lattice disc");

// what launch (2) leaves for launch (3), behind the partials of launch (1) in the pair's header
struct RefocusState { double lo, hi, focus; unsigned long long before; int live, pad; };
static_assert(REFOCUS_PARTS * 2 * sizeof(unsigned) + sizeof(RefocusState) <= REFOCUS_HEADER_BYTES && REFOCUS_HEADER_BYTES % 8 == 0, "the header of a pair's scratch");

__device__ __forceinline__ unsigned* refocus_parts(const RefocusPair& p, char* scratch) { return (unsigned*)(scratch + p.scratch_off); }
__device__ __forceinline__ RefocusState* refocus_state(const RefocusPair& p, char* scratch) {
    return (RefocusState*)(scratch + p.scratch_off + REFOCUS_PARTS * 2 * sizeof(unsigned));
}
__device__ __forceinline__ uint2* refocus_plane(const RefocusPair& p, char* scratch) { return (uint2*)(scratch + p.scratch_off + REFOCUS_HEADER_BYTES); }

// the map at the centre of photo pixel (Y, X)
__device__ __forceinline__ double refocus_map_at(const RefocusPair& p, int dt, int Y, int X) {
    return map_at_pixel_centre(p.map, dt, p.h, p.w, p.H, p.W, Y, X);
}

// (1) blockIdx.y = pair, blockIdx.x = one of the 64 shares of the map (elements share + 64 k blocks of 256)
__global__ __launch_bounds__(256) void refocus_minmax_kernel(const RefocusPair* __restrict__ pairs, int dt, char* __restrict__ scratch) {
    const RefocusPair p = pairs[blockIdx.y];
    finite_minmax_part(p.map, (size_t)p.h * p.w, dt, blockIdx.x, REFOCUS_PARTS, refocus_parts(p, scratch) + 2 * blockIdx.x);
}

// (2) blockIdx.x = pair, one wave
__global__ __launch_bounds__(64) void refocus_state_kernel(RefocusJob j) {
#pragma clang fp contract(off)
    const RefocusPair p = j.pairs[blockIdx.x];
    const unsigned* parts = refocus_parts(p, j.scratch);
    unsigned lo_o = parts[2 * threadIdx.x], hi_o = parts[2 * threadIdx.x + 1];
    unsigned long long before = 0;
    if (j.radius_out || j.defocus_out)  // (an integer sum: any order)
        for (unsigned q = threadIdx.x; q < blockIdx.x; q += 64) before += (unsigned long long)j.pairs[q].H * (unsigned long long)j.pairs[q].W;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo_o = min(lo_o, __shfl_xor(lo_o, o));
        hi_o = max(hi_o, __shfl_xor(hi_o, o));
        before += __shfl_xor(before, o);
    }
    if (threadIdx.x != 0) return;
    RefocusState st{};
    const bool ranged = finite_range(lo_o, hi_o, st.lo, st.hi);
    st.before = before;
    st.live = j.depth_space || ranged;
    st.focus = j.focus;
    if (j.pointed) {
        const int Y = min(p.H - 1, (int)floor(j.fy * (double)p.H)), X = min(p.W - 1, (int)floor(j.fx * (double)p.W));
        const double s = refocus_map_at(p, j.dt, Y, X);
        if (!isfinite(s) || (j.depth_space && !(s > 0.0))) st.live = 0;
        else if (j.depth_space) st.focus = 1.0 / s;
        else st.focus = ranged ? (s - st.lo) / (st.hi - st.lo) : 0.0;
    }
    *refocus_state(p, j.scratch) = st;
}

// (3) blockIdx.y = pair, blockIdx.x = 256 photo pixels in row-major order, one a thread; the photo is read byte by byte through its pitch
__global__ __launch_bounds__(256) void refocus_prepare_kernel(RefocusJob j) {
#pragma clang fp contract(off)
    const RefocusPair p = j.pairs[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.H * p.W) return;  // (the grid's x extent is that of the largest photo)
    const RefocusState st = *refocus_state(p, j.scratch);
    const int Y = (int)(i / (unsigned)p.W), X = (int)(i - (size_t)Y * p.W);
    double e = 0.0;
    if (st.live) {
        const double s = refocus_map_at(p, j.dt, Y, X);
        if (isfinite(s)) {
            if (j.depth_space) e = (s > 0.0 ? 1.0 / s : 0.0) - st.focus;
            else e = (s - st.lo) / (st.hi - st.lo) - st.focus;
        }
    }
    const double r = fmin((double)j.max_radius, j.aperture * fmax(0.0, fabs(e) - j.half_range));
    const unsigned rq = (unsigned)(int)floor(4.0 * r);
    const float e32 = (float)e;
    const unsigned char* px = p.photo + (long long)Y * p.pitch + 3LL * X;
    refocus_plane(p, j.scratch)[i] = make_uint2((unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16 | rq << 24, __float_as_uint(e32));
    if (j.radius_out) j.radius_out[st.before + i] = (unsigned char)rq;
    if (j.defocus_out) j.defocus_out[st.before + i] = e32;
}

// floor(sqrt(v)) of a small non-negative integer
__device__ __forceinline__ int refocus_isqrt(int v) {
    int r = (int)sqrtf((float)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// (4) blockIdx.x = a tile of the call: the pair is the last whose tile_off is not beyond it. HALO >= R = max_radius sizes the LDS image (the
// launcher picks the smallest of 8, 16, 32): a texel is the 8 bytes of launch (3), a row of the image S = 32 + 2 HALO texels. A wave reads 2 rows
// of 32 consecutive texels per tap with one ds_read_b64: each half wave covers the 64 banks once, whatever S. The weights 1.0 / N(k) up to the
// tile's largest k are divided out once per workgroup into LDS.
template <int HALO>
__global__ __launch_bounds__(REFOCUS_TILE* REFOCUS_TILE) void refocus_gather_kernel(const RefocusPair* __restrict__ pairs, int P, int R,
                                                                                    char* __restrict__ scratch) {
#pragma clang fp contract(off)
    constexpr int T = REFOCUS_TILE, S = T + 2 * HALO, THREADS = T * T;
    __shared__ uint2 tex[S * S];
    __shared__ double weight[HALO * HALO + 1];
    __shared__ int wave_k[THREADS / 64];
    __shared__ int which;
    const int tid = (int)threadIdx.x;
    if (tid == 0) which = pair_of_tile(pairs, P, (long long)blockIdx.x);
    __syncthreads();
    const RefocusPair p = pairs[which];
    const int tile = (int)((long long)blockIdx.x - p.tile_off), tiles_x = (p.W + T - 1) / T;
    const int X0 = (tile % tiles_x) * T, Y0 = (tile / tiles_x) * T;
    const uint2* plane = refocus_plane(p, scratch);
    const int side = T + 2 * R;
    int kmax = 0;
    for (int idx = tid; idx < side * side; idx += THREADS) {
        const int ly = idx / side, lx = idx - ly * side;
        const int Y = Y0 - R + ly, X = X0 - R + lx;
        uint2 t = make_uint2(0u, 0xff800000u);  // outside the photo: rq = 0, e32 = -inf - no tap
        if (Y >= 0 && Y < p.H && X >= 0 && X < p.W) t = plane[(size_t)Y * p.W + X];
        tex[ly * S + lx] = t;
        const int rq = (int)(t.x >> 24);
        kmax = max(kmax, (rq * rq) >> 4);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o));
    if ((tid & 63) == 0) wave_k[tid >> 6] = kmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) kmax = max(kmax, wave_k[w]);
    kmax = min(kmax, R * R);  // (rq <= 4 R from launch (3): the window never leaves the staged halo)
    for (int k = tid; k <= kmax; k += THREADS) weight[k] = 1.0 / (double)refocus_n.n[k];
    __syncthreads();

    const int tx = tid % T, ty = tid / T, X = X0 + tx, Y = Y0 + ty;
    if (X >= p.W || Y >= p.H) return;
    const uint2* centre = tex + (ty + R) * S + tx + R;
    const uint2 me = *centre;
    unsigned char* o = p.out + ((size_t)Y * p.W + X) * 3;
    if (kmax == 0) {  // nothing in reach is blurred
        o[0] = (unsigned char)(me.x & 255u), o[1] = (unsigned char)((me.x >> 8) & 255u), o[2] = (unsigned char)((me.x >> 16) & 255u);
        return;
    }
    const float ep = __uint_as_float(me.y);
    const int rqp = (int)(me.x >> 24), kp = (rqp * rqp) >> 4;
    double sb = 0.0, sg = 0.0, sr = 0.0, sw = 0.0;
    const int rw = refocus_isqrt(kmax);
    for (int dy = -rw; dy <= rw; ++dy) {
        const int xr = refocus_isqrt(kmax - dy * dy);
        const uint2* row = centre + dy * S;
        for (int dx = -xr; dx <= xr; ++dx) {
            const uint2 q = row[dx];
            const int rqq = (int)(q.x >> 24), kq = (rqq * rqq) >> 4;
            const int k_eff = __uint_as_float(q.y) > ep ? kq : min(kq, kp);
            if (dx * dx + dy * dy <= k_eff) {
                const double w = weight[k_eff];
                const double wb = w * (double)(q.x & 255u), wg = w * (double)((q.x >> 8) & 255u), wr = w * (double)((q.x >> 16) & 255u);
                sb = sb + wb, sg = sg + wg, sr = sr + wr, sw = sw + w;
            }
        }
    }
    o[0] = (unsigned char)floor(sb / sw + 0.5), o[1] = (unsigned char)floor(sg / sw + 0.5), o[2] = (unsigned char)floor(sr / sw + 0.5);
}

}  // namespace

int mdpt_launch_post_refocus(const RefocusJob& j, hipStream_t stream) {
    if (j.P <= 0 || j.P > 65535 || j.max_radius < 0 || j.max_radius > REFOCUS_MAX_RADIUS || j.max_pixels == 0 || j.max_pixels >= ((size_t)1 << 31) ||
        (j.gather && (j.total_tiles == 0 || j.total_tiles >= ((size_t)1 << 31))))
        return (int)hipErrorInvalidValue;
    post_launch("refocus_minmax_kernel", refocus_minmax_kernel, dim3(REFOCUS_PARTS, j.P), dim3(256), stream, j.pairs, j.dt, j.scratch);
    post_launch("refocus_state_kernel", refocus_state_kernel, dim3(j.P), dim3(64), stream, j);
    post_launch("refocus_prepare_kernel", refocus_prepare_kernel, dim3((unsigned)((j.max_pixels + 255) / 256), j.P), dim3(256), stream, j);
    if (j.gather) {
        const dim3 grid((unsigned)j.total_tiles), block(REFOCUS_TILE * REFOCUS_TILE);
        if (j.max_radius <= 8) post_launch("refocus_gather_kernel<8>", refocus_gather_kernel<8>, grid, block, stream, j.pairs, j.P, j.max_radius, j.scratch);
        else if (j.max_radius <= 16) post_launch("refocus_gather_kernel<16>", refocus_gather_kernel<16>, grid, block, stream, j.pairs, j.P, j.max_radius, j.scratch);
        else post_launch("refocus_gather_kernel<32>", refocus_gather_kernel<32>, grid, block, stream, j.pairs, j.P, j.max_radius, j.scratch);
    }
    return (int)hipGetLastError();
}
