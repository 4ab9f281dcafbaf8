// ---- tiled high-resolution inference: the maps of overlapping tiles of one photo (DPTModel.inference_regions) put together into one map at the
// photo's resolution. Every forward of a relative-depth model has its own unknown scale and shift (the reference's
// .readme_assets/results_explainer.md, "Results are scene-specific!"), and "Fitting to (more) known data" there names the cure, a least-squares fit
// of the two terms, without code for it: the whole photo inferred once at model size is the guide, every tile's map is fitted to the guide over the
// tile's own box, and the fitted tiles are feather-blended. All arithmetic is fp64, nothing contracted, rounded to fp32 once.
//
// The fit is bit-deterministic without atomics and without one workgroup waiting for or reading another: (1) workgroup (c, t) reduces chunk c of
// tile t's samples - MDPT_TILE_FIT_CHUNK of them, each thread its 8 in order, then block_sum_f64's fixed tree - into parts[t][c]; (2) in the next
// launch one workgroup per tile adds the tile's partials in chunk order and solves. A launch boundary separates the producers from the consumer.

namespace {

// (1) blockIdx.y = tile, blockIdx.x = chunk. Sample (j, i) of the map: x = m[j, i], y = the guide at the pixel's centre in the photo,
// (x1 + (i + 0.5) bw / w, y1 + (j + 0.5) bh / h); a sample whose x or y is not finite is skipped. -> {n, Sx, Sy, Sxx, Sxy, Syy} of the chunk
__global__ __launch_bounds__(256) void tile_fit_partial_kernel(const PostTile* __restrict__ tiles, int dt, const void* __restrict__ guide, int gdt, int gh,
                                                               int gw, int H, int W, double* __restrict__ parts, int max_chunks) {
#pragma clang fp contract(off)
    const PostTile t = tiles[blockIdx.y];
    const double bw = (double)(t.x2 - t.x1), bh = (double)(t.y2 - t.y1);
    chunk_reduce<6>((size_t)t.h * t.w, parts + (size_t)blockIdx.y * max_chunks * 6, [&](size_t e, double (&a)[6]) {
#pragma clang fp contract(off)
        const int j = (int)(e / t.w), i = (int)(e - (size_t)j * t.w);
        const double x = (double)ld_dt(t.map, e, dt);
        const double X = (double)t.x1 + ((double)i + 0.5) * bw / (double)t.w, Y = (double)t.y1 + ((double)j + 0.5) * bh / (double)t.h;
        const double y = bilinear_f64_at(guide, gdt, gh, gw, X, Y, H, W);
        if (isfinite(x) && isfinite(y)) {
            a[0] += 1.0; a[1] += x; a[2] += y;
            a[3] += x * x; a[4] += x * y; a[5] += y * y;
        }
    });
}

// (2) one workgroup per tile (affine_fit_solve): lane k adds partial sum k of the tile's chunks in chunk order -> sums[t]; then var = n Sxx - Sx^2,
// s = (n Sxy - Sx Sy) / var, t = (Sy - s Sx) / n -> fit[t] = {s, t}. A degenerate tile (n < 2, var <= 0, s not finite or <= 0) gets s = 0 and the
// guide's mean t = Sy / n; n == 0: t = 0, and the blend skips the tile (sums[t][0] == 0 marks it empty)
__global__ __launch_bounds__(64) void tile_fit_solve_kernel(const PostTile* __restrict__ tiles, const double* __restrict__ parts, int max_chunks,
                                                            double* __restrict__ sums, double* __restrict__ fit) {
    const int t = blockIdx.x;
    affine_fit_solve(parts + (size_t)t * max_chunks * 6, tile_fit_chunks((size_t)tiles[t].h * tiles[t].w), t, sums, fit);
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

}  // namespace

int mdpt_launch_post_tile_fit(const PostTile* tiles, int T, int max_chunks, int dt, const void* guide, int gdt, int gh, int gw, int H, int W, double* parts,
                              double* sums, double* fit, hipStream_t stream) {
    // (a grid's x extent times the 256 threads of a block must stay below 2^32)
    if (T <= 0 || T > 65535 || max_chunks <= 0 || max_chunks >= (1 << 24) || gh <= 0 || gw <= 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
    post_launch("tile_fit_partial_kernel", tile_fit_partial_kernel, dim3(max_chunks, T), dim3(256), stream, tiles, dt, guide, gdt, gh, gw, H, W, parts,
                max_chunks);
    post_launch("tile_fit_solve_kernel", tile_fit_solve_kernel, dim3(T), dim3(64), stream, tiles, parts, max_chunks, sums, fit);
    return (int)hipGetLastError();
}

int mdpt_launch_post_tile_blend(const PostTile* tiles, int T, int dt, int H, int W, const double* fit, const double* sums, double feather, float* out,
                                hipStream_t stream) {
    const size_t blocks_x = ((size_t)W + BLEND_BW - 1) / BLEND_BW, blocks_y = ((size_t)H + BLEND_BH - 1) / BLEND_BH;
    if (T <= 0 || H <= 0 || W <= 0 || !(feather >= 0.0) || blocks_x * blocks_y >= ((size_t)1 << 24)) return (int)hipErrorInvalidValue;
    post_launch("tile_blend_kernel", tile_blend_kernel, dim3((unsigned)(blocks_x * blocks_y)), dim3(256), stream, tiles, T, dt, H, W, fit, sums, feather + 1.0,
                out, (int)blocks_x);
    return (int)hipGetLastError();
}
