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

namespace {

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

}  // namespace

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
    post_launch("guided_cell_sum_kernel", guided_cell_sum_kernel, dim3((unsigned)cell_blocks, P), dim3(256), stream, pairs, scratch);
    post_launch("guided_row_kernel<13>", guided_row_kernel<GUIDED_MOMENTS>, dim3((unsigned)row_blocks, P), dim3(256), stream, pairs, dt, radius, scratch);
    post_launch("guided_col_kernel<13>", guided_col_kernel<GUIDED_MOMENTS>, dim3((unsigned)col_blocks, P), dim3(256), stream, pairs, radius, eps, scratch,
                nullptr);
    post_launch("guided_row_kernel<4>", guided_row_kernel<4>, dim3((unsigned)row_blocks, P), dim3(256), stream, pairs, dt, radius, scratch);
    post_launch("guided_col_kernel<4>", guided_col_kernel<4>, dim3((unsigned)col_blocks, P), dim3(256), stream, pairs, radius, eps, scratch, coeffs);
    post_launch("guided_apply_kernel", guided_apply_kernel, dim3((unsigned)apply_blocks, P), dim3(256), stream, pairs, scratch);
    return (int)hipGetLastError();
}
