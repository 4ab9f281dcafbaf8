// ---- locally varying true-depth alignment (depth completion from sparse measurements; not in the reference): the fit of post_align.inc, t ~ A v + B, per
// cell of a gh x gw grid over the truth instead of per image, smoothed as the guided filter smooths its coefficients, and applied as a coefficient FIELD.
// A pair is a LocalFitPair (mdpt_kernels.h); the table lives in device memory and pairs may all differ in size and grid. The samples are those of
// align_sample (MDPT_ALIGN_LSTSQ), truth pixel (Y, X) belongs to cell (Y gh / H, X gw / W) (guided_cell_start gives a cell's first pixel). Five launches:
//   (1) localfit_partial_kernel ... a workgroup = (cell, chunk): the cell's pixels in row-major order INSIDE the cell, MDPT_TILE_FIT_CHUNK at a time,
//                                   chunk_reduce_at's fixed strides and tree -> {n, Sv, St, Svv, Svt, Stt} of the chunk
//   (2) localfit_cell_kernel ...... a thread = (cell, moment): the cell's chunks added in chunk order -> moments [cells, 6]
//   (3) localfit_global_kernel .... a workgroup = pair: the cells added in row-major order -> sums [P, 6], affine_solve -> fit [P, 2] = (A0, B0)
//   (4) localfit_window_kernel .... a thread = node: the moments of the cells within `radius`, clipped to the grid, one running sum with dj outer and di
//                                   inner, both ascending; + prior (G / n_G) term by term; affine_solve; a window without a sample or a degenerate
//                                   one takes (A0, B0) -> window fits (scratch)
//   (5) localfit_mean_kernel ...... a thread = node: the window fits summed over the same window in the same order, divided by its count -> coeffs
// and one for the apply: per output pixel (A, B) = the coefficients resampled at the pixel's centre (bilinear_f64_taps / _mix over the grid), v as
// align_apply_kernel reads it, q = A v + B -> align_depth_of.
// The split of a cell's samples depends on the pair's own H, W, gh, gw only: not on P, not on the other pairs, not on the grid of the launch (a workgroup
// past its pair's extent returns at once). All fp64, nothing contracted, no atomics, a launch boundary between every producer and its consumer:
// bit-deterministic, and a pair's results are those of its own call. The window sums are direct, (2 radius + 1)^2 additions a node: no running sum
// whose errors would travel (post_guided.inc); a large radius on a large grid pays for that.

namespace {

__device__ __forceinline__ AlignPair localfit_align_pair(const LocalFitPair& p) { return AlignPair{p.pred, p.ph, p.pw, p.truth, p.valid, p.H, p.W}; }

struct LocalFitScratch { double* parts; double* wfit; size_t chunks; };
__device__ __forceinline__ LocalFitScratch localfit_scratch(const LocalFitPair& p, char* scratch) {
    const size_t chunks = localfit_cell_chunks((size_t)p.H, (size_t)p.W, (size_t)p.gh, (size_t)p.gw);
    double* base = (double*)(scratch + p.scratch_off);
    return LocalFitScratch{base, base + (size_t)p.gh * p.gw * chunks * 6, chunks};
}

// the pixels [y0, y1) x [x0, x1) of cell c = j gw + i
struct LocalFitCell { int y0, y1, x0, x1; };
__device__ __forceinline__ LocalFitCell localfit_cell(const LocalFitPair& p, int cell) {
    const int j = cell / p.gw, i = cell - j * p.gw;
    return LocalFitCell{guided_cell_start(j, p.gh, p.H), guided_cell_start(j + 1, p.gh, p.H), guided_cell_start(i, p.gw, p.W), guided_cell_start(i + 1, p.gw, p.W)};
}

// (1) blockIdx.y = pair, blockIdx.x = cell * chunks + chunk (chunks = those of the pair's largest cell; a chunk past the cell's pixels does nothing)
__global__ __launch_bounds__(256) void localfit_partial_kernel(const LocalFitPair* __restrict__ pairs, int dt, int inverse, double tmin, double tmax,
                                                               char* __restrict__ scratch) {
#pragma clang fp contract(off)
    const LocalFitPair p = pairs[blockIdx.y];
    const LocalFitScratch s = localfit_scratch(p, scratch);
    if ((size_t)blockIdx.x >= (size_t)p.gh * p.gw * s.chunks) return;  // (uniform over the block: the grid's x extent is that of the largest pair)
    const int cell = (int)((size_t)blockIdx.x / s.chunks);
    const size_t chunk = (size_t)blockIdx.x - (size_t)cell * s.chunks;
    const LocalFitCell c = localfit_cell(p, cell);
    const int cw = c.x1 - c.x0;
    const AlignPair a = localfit_align_pair(p);
    chunk_reduce_at<6>(chunk, (size_t)(c.y1 - c.y0) * cw, s.parts + (size_t)blockIdx.x * 6, [&](size_t k, double (&m)[6]) {
#pragma clang fp contract(off)
        const int dy = (int)(k / (size_t)cw), dx = (int)(k - (size_t)dy * cw);
        AlignSample q;
        if (align_sample(a, dt, inverse, tmin, tmax, (size_t)(c.y0 + dy) * p.W + (c.x0 + dx), q)) {
            m[0] += 1.0; m[1] += q.v; m[2] += q.t;
            m[3] += q.v * q.v; m[4] += q.v * q.t; m[5] += q.t * q.t;
        }
    });
}

// (2) blockIdx.y = pair, thread = (cell, moment k): the chunks the cell has, in chunk order
__global__ __launch_bounds__(256) void localfit_cell_kernel(const LocalFitPair* __restrict__ pairs, char* __restrict__ scratch, double* __restrict__ moments) {
#pragma clang fp contract(off)
    const LocalFitPair p = pairs[blockIdx.y];
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)p.gh * p.gw * 6) return;
    const int cell = (int)(at / 6), k = (int)(at - (size_t)cell * 6);
    const LocalFitScratch s = localfit_scratch(p, scratch);
    const LocalFitCell c = localfit_cell(p, cell);
    const size_t chunks = tile_fit_chunks((size_t)(c.y1 - c.y0) * (c.x1 - c.x0));
    const double* row = s.parts + (size_t)cell * s.chunks * 6;
    double acc = 0.0;
    for (size_t q = 0; q < chunks; ++q) acc += row[q * 6 + k];
    moments[((size_t)p.cell_off + cell) * 6 + k] = acc;
}

// (3) one workgroup per pair (affine_fit_solve): the cells in row-major order -> sums[p] = G, affine_solve -> fit[p] = (A0, B0)
__global__ __launch_bounds__(64) void localfit_global_kernel(const LocalFitPair* __restrict__ pairs, const double* __restrict__ moments,
                                                             double* __restrict__ sums, double* __restrict__ fit) {
    const int p = blockIdx.x;
    affine_fit_solve(moments + (size_t)pairs[p].cell_off * 6, (size_t)pairs[p].gh * pairs[p].gw, p, sums, fit);
}

// the clipped window of node (j, i)
struct LocalFitWindow { int j0, j1, i0, i1; };
__device__ __forceinline__ LocalFitWindow localfit_window(const LocalFitPair& p, int cell, int radius) {
    const int j = cell / p.gw, i = cell - j * p.gw;
    return LocalFitWindow{max(j - radius, 0), min(j + radius, p.gh - 1), max(i - radius, 0), min(i + radius, p.gw - 1)};
}

// (4) blockIdx.y = pair, thread = node
__global__ __launch_bounds__(256) void localfit_window_kernel(const LocalFitPair* __restrict__ pairs, int radius, double prior, const double* __restrict__ moments,
                                                              const double* __restrict__ sums, const double* __restrict__ fit, char* __restrict__ scratch) {
#pragma clang fp contract(off)
    const LocalFitPair p = pairs[blockIdx.y];
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)p.gh * p.gw) return;
    const int cell = (int)at;
    const LocalFitWindow w = localfit_window(p, cell, radius);
    const double* m = moments + (size_t)p.cell_off * 6;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int jj = w.j0; jj <= w.j1; ++jj)
        for (int ii = w.i0; ii <= w.i1; ++ii) {
            const double* c = m + ((size_t)jj * p.gw + ii) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k] += c[k];
        }
    const double* G = sums + (size_t)blockIdx.y * 6;
    double A = fit[2 * (size_t)blockIdx.y], B = fit[2 * (size_t)blockIdx.y + 1];
    if (s[0] > 0.0) {  // (a window without a sample takes the global fit itself: what the prior alone would give, without its rounding)
        if (prior > 0.0 && G[0] > 0.0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k] += prior * (G[k] / G[0]);
        }
        double scale, shift;
        affine_solve(s[0], s[1], s[2], s[3], s[4], scale, shift);
        if (scale > 0.0) A = scale, B = shift;  // (affine_solve gives a degenerate set scale = 0, every other one scale > 0)
    }
    double* o = localfit_scratch(p, scratch).wfit + 2 * (size_t)cell;
    o[0] = A;
    o[1] = B;
}

// (5) blockIdx.y = pair, thread = node
__global__ __launch_bounds__(256) void localfit_mean_kernel(const LocalFitPair* __restrict__ pairs, int radius, char* __restrict__ scratch, double* __restrict__ coeffs) {
#pragma clang fp contract(off)
    const LocalFitPair p = pairs[blockIdx.y];
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)p.gh * p.gw) return;
    const int cell = (int)at;
    const LocalFitWindow w = localfit_window(p, cell, radius);
    const double* f = localfit_scratch(p, scratch).wfit;
    double a = 0.0, b = 0.0;
    for (int jj = w.j0; jj <= w.j1; ++jj)
        for (int ii = w.i0; ii <= w.i1; ++ii) {
            a += f[2 * ((size_t)jj * p.gw + ii)];
            b += f[2 * ((size_t)jj * p.gw + ii) + 1];
        }
    const double count = (double)(w.j1 - w.j0 + 1) * (double)(w.i1 - w.i0 + 1);
    double* o = coeffs + 2 * ((size_t)p.cell_off + cell);
    o[0] = a / count;
    o[1] = b / count;
}

// apply: blockIdx.y = pair, the blocks stride over the pair's H x W output pixels (H, W are the OUTPUT size here, as in align_apply_kernel)
__global__ __launch_bounds__(256) void localfit_apply_kernel(const LocalFitPair* __restrict__ pairs, int dt, int inverse, const double* __restrict__ coeffs,
                                                             double dmin, double dmax) {
#pragma clang fp contract(off)
    const LocalFitPair p = pairs[blockIdx.y];
    const AlignPair a = localfit_align_pair(p);
    const size_t n = (size_t)p.H * p.W;
    const double* c = coeffs + 2 * (size_t)p.cell_off;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int Y = (int)(e / (size_t)p.W), X = (int)(e - (size_t)Y * p.W);
        const BilinearTaps t = bilinear_f64_taps(p.gh, p.gw, (double)X + 0.5, (double)Y + 0.5, p.H, p.W);
        const double* c00 = c + 2 * ((size_t)t.y0 * p.gw + t.x0);
        const double* c01 = c + 2 * ((size_t)t.y0 * p.gw + t.x1);
        const double* c10 = c + 2 * ((size_t)t.y1 * p.gw + t.x0);
        const double* c11 = c + 2 * ((size_t)t.y1 * p.gw + t.x1);
        const double A = bilinear_f64_mix(t, c00[0], c01[0], c10[0], c11[0]), B = bilinear_f64_mix(t, c00[1], c01[1], c10[1], c11[1]);
        p.out[e] = align_depth_of(A * align_pred_at(a, dt, e) + B, inverse, dmin, dmax);
    }
}

}  // namespace

int mdpt_launch_localfit_fit(const LocalFitJob& j, hipStream_t stream) {
    if (j.P <= 0 || j.P > 65535 || j.radius < 0 || j.radius > LOCALFIT_MAX_RADIUS || !(j.prior >= 0.0) || j.max_blocks == 0 || j.max_blocks >= ((size_t)1 << 31) ||
        j.max_cells == 0 || j.max_cells > (size_t)LOCALFIT_MAX_GRID * LOCALFIT_MAX_GRID)
        return (int)hipErrorInvalidValue;
    // (every grid's x extent is that of the table's largest pair; a workgroup or thread past its own pair's extent returns at once)
    const unsigned node_blocks = (unsigned)((j.max_cells + 255) / 256), moment_blocks = (unsigned)((j.max_cells * 6 + 255) / 256);
    post_launch("localfit_partial_kernel", localfit_partial_kernel, dim3((unsigned)j.max_blocks, j.P), dim3(256), stream, j.pairs, j.dt, j.inverse, j.tmin, j.tmax,
                j.scratch);
    post_launch("localfit_cell_kernel", localfit_cell_kernel, dim3(moment_blocks, j.P), dim3(256), stream, j.pairs, j.scratch, j.moments);
    post_launch("localfit_global_kernel", localfit_global_kernel, dim3(j.P), dim3(64), stream, j.pairs, j.moments, j.sums, j.fit);
    post_launch("localfit_window_kernel", localfit_window_kernel, dim3(node_blocks, j.P), dim3(256), stream, j.pairs, j.radius, j.prior, j.moments, j.sums, j.fit,
                j.scratch);
    post_launch("localfit_mean_kernel", localfit_mean_kernel, dim3(node_blocks, j.P), dim3(256), stream, j.pairs, j.radius, j.scratch, j.coeffs);
    return (int)hipGetLastError();
}

int mdpt_launch_localfit_apply(const LocalFitPair* pairs, int P, size_t max_pixels, int dt, int inverse, const double* coeffs, double dmin, double dmax,
                               hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_pixels == 0 || max_pixels >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    post_launch("localfit_apply_kernel", localfit_apply_kernel, dim3(align_stride_blocks(max_pixels), P), dim3(256), stream, pairs, dt, inverse, coeffs, dmin, dmax);
    return (int)hipGetLastError();
}
