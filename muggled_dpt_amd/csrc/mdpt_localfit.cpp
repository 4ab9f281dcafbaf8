// libmdpt: the mdpt_localfit_* entry points (locally varying true-depth alignment; kernels in post_localfit.inc). Named apart from mdpt_post_* (see
// include/mdpt.h); the checks they share with those come from mdpt_post_checks.h, their own are written once below.
#include "mdpt_post_checks.h"

#include <cmath>

MDPT_SAME_RECORD(mdpt_localfit_pair, LocalFitPair, 72, pred, ph, pw, truth, valid, H, W, gh, gw, cell_off, scratch_off, out);
static_assert(MDPT_LOCALFIT_MAX_GRID == LOCALFIT_MAX_GRID && MDPT_LOCALFIT_MAX_RADIUS == LOCALFIT_MAX_RADIUS && MDPT_LOCALFIT_CHUNK == MDPT_TILE_FIT_CHUNK,
              "the limits of include/mdpt.h are those of mdpt_kernels.h");

// the table of every local-fit entry point: present, 1 .. 65535 records
static int check_localfit_table(const mdpt_localfit_pair* records, int32_t n) {
    if (!records) return fail(MDPT_E_INVALID, "null argument (records_host)");
    return check_count("pair", "n = ", n);
}
// record p's sizes: prediction and H x W positive, H W < 2^31, the grid 1 .. cap (`fits`: and no larger than H x W)
static int check_localfit_sizes(const mdpt_localfit_pair& q, int p, bool fits) {
    if (q.ph <= 0 || q.pw <= 0 || q.H <= 0 || q.W <= 0) return fail(MDPT_E_INVALID, "bad size: prediction %dx%d, truth %dx%d (pair %d)", q.ph, q.pw, q.H, q.W, p);
    CHK(check_below_2_31("truth", q.H, q.W, "", p));
    if (q.gh < 1 || q.gw < 1 || q.gh > LOCALFIT_MAX_GRID || q.gw > LOCALFIT_MAX_GRID || (fits && (q.gh > q.H || q.gw > q.W)))
        return fail(MDPT_E_INVALID, "bad grid %dx%d (pair %d: 1 .. %d cells an axis%s)", q.gh, q.gw, p, LOCALFIT_MAX_GRID, fits ? ", no more than the truth's pixels" : "");
    return 0;
}
static int check_localfit_common(int32_t pred_dtype, int32_t space) {
    if (!tensor_dtype_ok(pred_dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", pred_dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown alignment space %d", space);
    return 0;
}
// record p's prediction and its place in the cell tables
static int check_localfit_record(const mdpt_localfit_pair& q, int p, int32_t pred_dtype, size_t cells_before) {
    if (!q.pred || !aligned_to_element(q.pred, pred_dtype)) return fail(MDPT_E_INVALID, "null or misaligned prediction (pair %d)", p);
    if (q.cell_off != (int64_t)cells_before)
        return fail(MDPT_E_INVALID, "cell_off %lld of pair %d is not the %zu cells of the pairs before it", (long long)q.cell_off, p, cells_before);
    return 0;
}

extern "C" {

int mdpt_localfit_scratch_bytes(const mdpt_localfit_pair* records_host, int32_t n, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    CHK(check_localfit_table(records_host, n));
    size_t total = 0;
    for (int p = 0; p < n; ++p) {
        const mdpt_localfit_pair& q = records_host[p];
        CHK(check_localfit_sizes(q, p, true));
        total += localfit_pair_scratch_bytes((size_t)q.H, (size_t)q.W, (size_t)q.gh, (size_t)q.gw);
    }
    *bytes = total;
    return 0;
}

int mdpt_localfit_fit(const mdpt_localfit_pair* records_host, const void* records_dev, int32_t n, int32_t pred_dtype, int32_t space, int32_t radius,
                      double prior, double tmin, double tmax, void* moments_f64, void* fit_f64, void* sums_f64, void* coeffs_f64, void* scratch,
                      size_t scratch_bytes, void* stream) {
    if (!records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_dev or scratch)");
    if (!moments_f64 || !fit_f64 || !sums_f64 || !coeffs_f64) return fail(MDPT_E_INVALID, "null argument (moments_f64, fit_f64, sums_f64 or coeffs_f64)");
    CHK(check_localfit_table(records_host, n));
    CHK(check_localfit_common(pred_dtype, space));
    if (radius < 0 || radius > LOCALFIT_MAX_RADIUS) return fail(MDPT_E_INVALID, "radius %d: the window radius must be 0 .. %d cells", radius, LOCALFIT_MAX_RADIUS);
    if (!(prior >= 0.0) || !std::isfinite(prior)) return fail(MDPT_E_INVALID, "prior must be finite and >= 0 pseudo-samples, got %g", prior);
    if (!(tmin <= tmax)) return fail(MDPT_E_INVALID, "the truth range [%g, %g] is empty or NaN", tmin, tmax);
    if ((((uintptr_t)records_dev | (uintptr_t)moments_f64 | (uintptr_t)fit_f64 | (uintptr_t)sums_f64 | (uintptr_t)coeffs_f64 | (uintptr_t)scratch) & 7) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the fp64 buffers and the scratch need 8 bytes)");
    size_t cells = 0, max_blocks = 0, max_cells = 0;
    ScratchRegions regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_localfit_pair& q = records_host[p];
        CHK(check_localfit_sizes(q, p, true));
        CHK(check_localfit_record(q, p, pred_dtype, cells));
        if (!q.truth || ((uintptr_t)q.truth & 3) != 0) return fail(MDPT_E_INVALID, "null or misaligned truth (pair %d)", p);
        const size_t H = (size_t)q.H, W = (size_t)q.W, gh = (size_t)q.gh, gw = (size_t)q.gw;
        CHK(regions.add(p, q.scratch_off, localfit_pair_scratch_bytes(H, W, gh, gw), scratch_bytes, "of scratch given (mdpt_localfit_scratch_bytes)"));
        cells += gh * gw;
        max_cells = std::max(max_cells, gh * gw);
        max_blocks = std::max(max_blocks, gh * gw * localfit_cell_chunks(H, W, gh, gw));
    }
    CHK(regions.finish());
    if (max_blocks >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu chunks in one pair: a call takes fewer than 2^31", max_blocks);
    LocalFitJob j{};
    j.pairs = (const LocalFitPair*)records_dev;
    j.P = n, j.dt = pred_dtype, j.inverse = space == MDPT_ALIGN_INVERSE, j.radius = radius;
    j.prior = prior, j.tmin = tmin, j.tmax = tmax;
    j.scratch = (char*)scratch;
    j.moments = (double*)moments_f64, j.fit = (double*)fit_f64, j.sums = (double*)sums_f64, j.coeffs = (double*)coeffs_f64;
    j.max_blocks = max_blocks, j.max_cells = max_cells;
    CHK(mdpt_launch_localfit_fit(j, (hipStream_t)stream));
    return 0;
}

int mdpt_localfit_apply(const mdpt_localfit_pair* records_host, const void* records_dev, int32_t n, int32_t pred_dtype, int32_t space,
                        const void* coeffs_f64, double dmin, double dmax, void* stream) {
    if (!records_dev || !coeffs_f64) return fail(MDPT_E_INVALID, "null argument (records_dev or coeffs_f64)");
    CHK(check_localfit_table(records_host, n));
    CHK(check_localfit_common(pred_dtype, space));
    if (dmin != dmin || dmax != dmax || dmin > dmax) return fail(MDPT_E_INVALID, "the clamp [%g, %g] is empty or NaN", dmin, dmax);
    if ((((uintptr_t)records_dev | (uintptr_t)coeffs_f64) & 7) != 0) return fail(MDPT_E_INVALID, "misaligned pointer (the table and the coefficients need 8 bytes)");
    size_t cells = 0, max_pixels = 0;
    for (int p = 0; p < n; ++p) {
        const mdpt_localfit_pair& q = records_host[p];
        CHK(check_localfit_sizes(q, p, false));
        CHK(check_localfit_record(q, p, pred_dtype, cells));
        if (!q.out || ((uintptr_t)q.out & 3) != 0) return fail(MDPT_E_INVALID, "null or misaligned out (pair %d: fp32)", p);
        cells += (size_t)q.gh * q.gw;
        max_pixels = std::max(max_pixels, (size_t)q.H * q.W);
    }
    CHK(mdpt_launch_localfit_apply((const LocalFitPair*)records_dev, n, max_pixels, pred_dtype, space == MDPT_ALIGN_INVERSE, (const double*)coeffs_f64, dmin, dmax,
                                   (hipStream_t)stream));
    return 0;
}

}  // extern "C"
