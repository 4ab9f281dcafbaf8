// ---- still-image display tail (the reference's run_image.py:185-195, 323-343, 350-358) and the 3D viewer's edge alpha (run_3dviewer.py:455-505).
// Every kernel takes a uniform batch: image b is [h, w] at element b h w; grids are (parts, B) or one block per image. The prepared map comes from
// seg_scale_minmax_kernel<true> (its display form); the kernels after the plane fit take it with its statistics as one PlaneMap (mdpt_kernels.h). The arithmetic whose order the
// reference fixes (numpy's fp64, torch's per-op rounding) is written out with contraction off.

namespace {

// normalize_01 of a map stored in dtype dt as torch evaluates it in that dtype: (x - min) and (max - min) each rounded to dt, then the quotient
__device__ __forceinline__ float norm01_dt(float x, float lo, float hi, int dt) {
#pragma clang fp contract(off)
    return round_dt(round_dt(x - lo, dt) / round_dt(hi - lo, dt), dt);
}

// numpy's plane image at pixel (x, y): -(d + nx x + ny y) / nz in fp64 (plane_fit.py generate_image_from_plane_normal); c = {nx, ny, nz, d}
__device__ __forceinline__ double plane_at(const double* c, int x, int y) {
#pragma clang fp contract(off)
    return -(c[3] + c[0] * (double)x + c[1] * (double)y) / c[2];
}

// d = -(nx mx + ny my + nz mz), numpy's order
__device__ __forceinline__ double plane_offset(const double* n, double mx, double my, double mz) {
#pragma clang fp contract(off)
    return -1.0 * (n[0] * mx + n[1] * my + n[2] * mz);
}

// the eigenvector of the smallest eigenvalue of a symmetric 3x3 matrix, by cyclic Jacobi with a fixed number of sweeps (quadratic convergence:
// 3x3 in fp64 is converged after 4 or 5). A zero off-diagonal element is skipped, so a diagonal matrix (a constant map: z row and column zero)
// keeps its axes. Ties go to the later axis, so a degenerate fit prefers the z normal (a constant plane) over an x / y one.
__device__ void jacobi3_min_eigvec(double a[3][3], double n[3]) {
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 10; ++sweep) {
        for (int k = 0; k < 3; ++k) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int r = 0; r < 3; ++r) {
                const double arp = a[r][p], arq = a[r][q];
                a[r][p] = c * arp - s * arq;
                a[r][q] = s * arp + c * arq;
            }
            for (int r = 0; r < 3; ++r) {
                const double apr = a[p][r], aqr = a[q][r];
                a[p][r] = c * apr - s * aqr;
                a[q][r] = s * apr + c * aqr;
            }
            for (int r = 0; r < 3; ++r) {
                const double vrp = v[r][p], vrq = v[r][q];
                v[r][p] = c * vrp - s * vrq;
                v[r][q] = s * vrp + c * vrq;
            }
        }
    }
    int m = 0;
    for (int k = 1; k < 3; ++k)
        if (a[k][k] <= a[m][m]) m = k;
    for (int r = 0; r < 3; ++r) n[r] = v[r][m];
}

// plane of best fit of image b (one block per image; plane_fit.py get_xyz_samples / find_plane_normal / generate_image_from_plane_normal):
// z at the N sample points (parts != null: of normalize_01(image b) in dtype dt), the known x / y means (w-1)/2, (h-1)/2 and the sample z mean,
// the 3x3 Gram matrix of the centred samples in fp64, its smallest eigenvector (numpy's smallest right singular vector, up to sign) -> coef[b] =
// {nx, ny, nz, d}, d = -(nx mx + ny my + nz mz). Sample points are clamped into the map.
__global__ __launch_bounds__(256) void plane_fit_kernel(const void* __restrict__ in, int dt, int h, int w, const unsigned* __restrict__ parts,
                                                        const int* __restrict__ xy, int N, size_t xy_stride, double* __restrict__ coef) {
    const int b = blockIdx.x;
    float lo = 0.0f, hi = 1.0f;
    if (parts) seg_range(parts, b, lo, hi);
    const int* pts = xy + (size_t)b * xy_stride;
    const size_t base = (size_t)b * h * w;
    auto z_at = [&](int k, int& x, int& y) -> double {
        x = min(max(pts[2 * k], 0), w - 1);
        y = min(max(pts[2 * k + 1], 0), h - 1);
        const float z = ld_dt(in, base + (size_t)y * w + x, dt);
        return (double)(parts ? norm01_dt(z, lo, hi, dt) : z);
    };
    double zs[1] = {0.0};
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        int x, y;
        zs[0] += z_at(k, x, y);
    }
    block_sum_f64<1>(zs);
    const double mx = (w - 1) * 0.5, my = (h - 1) * 0.5, mz = zs[0] / N;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // xx xy xz yy yz zz
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        int x, y;
        const double cz = z_at(k, x, y) - mz, cx = x - mx, cy = y - my;
        g[0] += cx * cx; g[1] += cx * cy; g[2] += cx * cz;
        g[3] += cy * cy; g[4] += cy * cz; g[5] += cz * cz;
    }
    block_sum_f64<6>(g);
    if (threadIdx.x != 0) return;
    double a[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}}, nrm[3];
    jacobi3_min_eigvec(a, nrm);
    double* c = coef + (size_t)b * 4;
    c[0] = nrm[0];
    c[1] = nrm[1];
    c[2] = nrm[2];
    c[3] = plane_offset(nrm, mx, my, mz);
}

// the plane image of coef[b], rounded to fp32
__global__ __launch_bounds__(256) void plane_eval_kernel(const double* __restrict__ coef, int h, int w, float* __restrict__ out) {
    const int b = blockIdx.y;
    const double* c = coef + (size_t)b * 4;
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[(size_t)b * n + i] = (float)plane_at(c, (int)(i % w), (int)(i / w));
}

// v = dn - factor * plane in fp64 at pixel (x, y) of the map at element `base` (numpy: the fp32 map minus the fp64 plane), dn = normalize_01(map)
// in dtype dt; c = the map's plane
__device__ __forceinline__ double plane_removed(const void* map, size_t base, int dt, int w, int x, int y, float lo, float hi, const double* c,
                                                double factor) {
#pragma clang fp contract(off)
    return (double)norm01_dt(ld_dt(map, base + (size_t)y * w + x, dt), lo, hi, dt) - plane_at(c, x, y) * factor;
}

// n = normalize_01(v) in fp64 with v's {min, max - min}: the value the threshold display windows and the depth masks compare
__device__ __forceinline__ double plane_norm(const void* map, size_t base, int dt, int w, int x, int y, float lo, float hi, const double* c, double factor,
                                             double vlo, double vrange) {
#pragma clang fp contract(off)
    return (plane_removed(map, base, dt, w, x, y, lo, hi, c, factor) - vlo) / vrange;
}

// image b's plane in registers (the pointers of a PlaneMap carry no __restrict__: read through them after a store or a barrier, the plane is
// loaded again, per lane)
struct Plane { double c[4]; };
__device__ __forceinline__ Plane plane_of(const double* coef, int b) {
    const double* c = coef + (size_t)b * 4;
    return Plane{{c[0], c[1], c[2], c[3]}};
}

// per-image fp64 {min, max} partials of v: vparts[b][part] (block_minmax_f64)
__global__ __launch_bounds__(256) void plane_minmax_kernel(const PlaneMap m, double* __restrict__ vparts) {
    const int b = blockIdx.y;
    const Plane plane = plane_of(m.coef, b);
    float lo, hi;
    seg_range(m.parts, b, lo, hi);
    const size_t n = (size_t)m.h * m.w, base = (size_t)b * n;
    double vlo = INFINITY, vhi = -INFINITY;
    bool saw_nan = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = plane_removed(m.in, base, m.dt, m.w, (int)(i % m.w), (int)(i / m.w), lo, hi, plane.c, m.factor);
        saw_nan |= v != v;
        vlo = fmin(vlo, v);
        vhi = fmax(vhi, v);
    }
    block_minmax_f64(vlo, vhi, saw_nan, vparts + ((size_t)b * SEG_PARTS + blockIdx.x) * 2);
}

// t = clip((n - tmin) / delta, 0, 1) in fp64 (run_image.py:331-333, 355-356). Mode 1 (MDPT_POST_U8): round-half-even(255 t) -> uint8
// (a NaN -> 0), and (hist != null) its 256-bin histogram into hist[b]; mode 0 (MDPT_POST_F32): t, or 1 - t with reverse, -> fp32.
template <int MODE>
__global__ __launch_bounds__(256) void threshold_kernel(const PlaneMap m, double tmin, double delta, int reverse, void* __restrict__ out,
                                                        unsigned* __restrict__ hist) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const Plane plane = plane_of(m.coef, b);
    __shared__ unsigned bins[256];
    bins[threadIdx.x] = 0u;
    float lo, hi;
    double vlo, vrange;
    seg_range(m.parts, b, lo, hi);  // (publishes the zeroed bins too)
    seg_vrange(m.vparts, b, vlo, vrange);
    const size_t n = (size_t)m.h * m.w, base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = plane_norm(m.in, base, m.dt, m.w, (int)(i % m.w), (int)(i / m.w), lo, hi, plane.c, m.factor, vlo, vrange);
        double t = (v - tmin) / delta;
        t = t != t ? t : (t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t));
        if (MODE == 1) {
            const int q = t == t ? (int)rint(255.0 * t) : 0;
            ((unsigned char*)out)[base + i] = (unsigned char)q;
            if (hist) atomicAdd(&bins[q], 1u);
        } else {
            ((float*)out)[base + i] = (float)(reverse ? 1.0 - t : t);
        }
    }
    if (MODE == 1 && hist) hist_flush(bins, hist, b);
}

// ---- edge alpha (run_3dviewer.py:455-505): blur = conv(x, gauss, reflect pad p), (dx, dy) = conv(blur, sobel, reflect pad 1), mag = sqrt(dx^2 + dy^2)
constexpr int EDGE_TILE = 16;
constexpr int EDGE_MAX_PAD = 7;
struct EdgeBlur { float w[(2 * EDGE_MAX_PAD + 1) * (2 * EDGE_MAX_PAD + 1)]; int ksize; };

// one 16x16 tile of image b per block: the input tile with a (1 + p)-pixel halo in LDS (each LDS element the input at the reflected coordinate),
// the blurred tile with a 1-pixel halo (each at the reflected blurred coordinate, so the Sobel halo reflects on the blurred map as torch pads it),
// then the Sobel magnitude -> mag[b] (blur and Sobel in fp64: the Sobel differences neighbouring blurred values of up to ~k^2 times the map, which
// leaves fp32 sums a few 1e-3 of a byte off at 1080p; fp64 keeps the bytes off the reference's only at rounding ties), and the image's max through an atomicMax on the bits of the (non-negative) fp32 magnitudes. parts != null:
// the map is normalize_01(x) in fp32 first (norm01).
__global__ __launch_bounds__(256) void edge_mag_kernel(const float* __restrict__ in, int h, int w, const unsigned* __restrict__ parts, const EdgeBlur blur,
                                                       float* __restrict__ mag, unsigned* __restrict__ mag_max) {
    constexpr int BT = EDGE_TILE + 2, RMAX = BT + 2 * EDGE_MAX_PAD;
    __shared__ float sx[RMAX * RMAX];
    __shared__ double sb[BT * BT];
    const int b = blockIdx.z, t = threadIdx.x;
    float lo = 0.0f, hi = 1.0f;
    if (parts) seg_range(parts, b, lo, hi);
    const float range = hi - lo;
    const int ks = blur.ksize, p = ks / 2, R = BT + 2 * p;
    const int y0 = blockIdx.y * EDGE_TILE, x0 = blockIdx.x * EDGE_TILE;
    const float* img = in + (size_t)b * h * w;
    for (int e = t; e < R * R; e += 256) {
        const int vy = y0 - 1 - p + e / R, vx = x0 - 1 - p + e % R;
        const float v = img[(size_t)reflect_idx(vy, h) * w + reflect_idx(vx, w)];
        sx[e] = norm01(v, lo, range, parts != nullptr);
    }
    __syncthreads();
    for (int e = t; e < BT * BT; e += 256) {
        const int gy = y0 - 1 + e / BT, gx = x0 - 1 + e % BT;
        double acc = 0.0;
        if (gy <= h && gx <= w) {  // (rows / columns past h / w are no Sobel neighbour of a pixel of the map)
            const int ry = reflect_idx(gy, h) - y0 + 1, rx = reflect_idx(gx, w) - x0 + 1;  // in [0, BT): see the comment above
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx) acc = fma((double)blur.w[ky * ks + kx], (double)sx[(ry + ky) * R + rx + kx], acc);
        }
        sb[e] = acc;
    }
    __syncthreads();
    const int ty = t / EDGE_TILE, tx = t % EDGE_TILE, y = y0 + ty, x = x0 + tx;
    float m = 0.0f;
    if (y < h && x < w) {
        const double* s = sb + ty * BT + tx;  // s[i BT + j] = blurred at (reflect(y + i - 1), reflect(x + j - 1))
        const double dy = 3.0 * (s[0] - s[2 * BT]) + 10.0 * (s[1] - s[2 * BT + 1]) + 3.0 * (s[2] - s[2 * BT + 2]);
        const double dx = 3.0 * (s[0] - s[2]) + 10.0 * (s[BT] - s[BT + 2]) + 3.0 * (s[2 * BT] - s[2 * BT + 2]);
        m = (float)sqrt(dx * dx + dy * dy);
        mag[(size_t)b * h * w + (size_t)y * w + x] = m;
    }
    unsigned bits = m != m ? 0x7fffffffu : __float_as_uint(m);  // a NaN wins the max (torch's max propagates it)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o));
    if ((t & 63) == 0) atomicMax(mag_max + b, bits);
}

// ~round(255 mag / max) (torch: 255 * mag, then / max, round half to even, .byte(), bitwise_not); max 0 (a flat map) or NaN -> 0 before the not: 255
__device__ __forceinline__ unsigned char edge_byte(float m, float mx) {
#pragma clang fp contract(off)
    const float r = rintf((255.0f * m) / mx);
    return (unsigned char)(255 - (r == r ? (int)fminf(fmaxf(r, 0.0f), 255.0f) : 0));
}

__global__ __launch_bounds__(256) void edge_mask_kernel(const float* __restrict__ mag, const unsigned* __restrict__ mag_max, size_t n,
                                                        unsigned char* __restrict__ out) {
    const int b = blockIdx.y;
    const float mx = __uint_as_float(mag_max[b]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[(size_t)b * n + i] = edge_byte(mag[(size_t)b * n + i], mx);
}

// pack_depth_u24 per image (norm_clamp01 with image b's min/max from parts; parts == null: metric, as is; then u24_px) with the alpha byte
// in the same pass: the edge byte of mag (mag != null), the caller's mask (mask != null; per image or one for all), or 0
__global__ __launch_bounds__(256) void pack_u24_kernel(const float* __restrict__ in, size_t n, const unsigned* __restrict__ parts, int lossy,
                                                       const float* __restrict__ mag, const unsigned* __restrict__ mag_max,
                                                       const unsigned char* __restrict__ mask, size_t mask_stride, uchar4* __restrict__ out) {
    const int b = blockIdx.y;
    float lo = 0.0f, hi = 1.0f;
    if (parts) seg_range(parts, b, lo, hi);
    const float range = hi - lo;
    const float mx = mag ? __uint_as_float(mag_max[b]) : 0.0f;
    const size_t base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned char alpha = mag ? edge_byte(mag[base + i], mx) : (mask ? mask[(size_t)b * mask_stride + i] : (unsigned char)0);
        out[base + i] = u24_px(norm_clamp01(in[base + i], lo, range, parts != nullptr), lossy, alpha);
    }
}

// ---- depth masking (the reference's experiments/depth_masking.py: display :189-199, 314-332; save :341-361). n = normalize_01(normalize_01(x) - f plane)
// in fp64 (plane_norm), mask = 255 where tmin <= n <= tmax (a NaN compares false: 0), 255 - mask with invert.
// cv2.resize(INTER_LINEAR) is restated per axis by cv_tap (post_common.inc). CV_64F: lerp_cv64, rows first, then across them. CV_8U: weights
// round(2048 w), integer sums, (v + 2^21) >> 22: cv2's scalar fixed-point path (its SIMD / IPP paths may round 1 off).
constexpr int MASK_PX = 4;  // consecutive pixels per thread: 12 BGR bytes in (one dwordx3 load), 16 BGRA + 4 mask bytes out (dwordx4 + dword stores)

struct alignas(4) Bytes12 { unsigned w0, w1, w2; };  // (not uint3: a 3-vector may be accessed as 16 bytes)

__device__ __forceinline__ unsigned mask_byte(double n, double tmin, double tmax, int invert) {
    return ((n >= tmin && n <= tmax) != (invert != 0)) ? 255u : 0u;
}

// cv2.resize of a BGR uint8 image at the output pixel of taps (tx, ty), the scalar fixed-point formula -> o[0..2]
__device__ __forceinline__ void bgr_lerp_u8(const unsigned char* __restrict__ src, int iw, CvTap tx, CvTap ty, unsigned char* o) {
    const int ax1 = (int)rintf(tx.a * 2048.0f), ax0 = (int)rintf((1.0f - tx.a) * 2048.0f);
    const int ay1 = (int)rintf(ty.a * 2048.0f), ay0 = (int)rintf((1.0f - ty.a) * 2048.0f);
    const unsigned char* r0 = src + (size_t)ty.s0 * iw * 3;
    const unsigned char* r1 = src + (size_t)ty.s1 * iw * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int h0 = r0[tx.s0 * 3 + ch] * ax0 + r0[tx.s1 * 3 + ch] * ax1;
        const int h1 = r1[tx.s0 * 3 + ch] * ax0 + r1[tx.s1 * 3 + ch] * ax1;
        const int v = (h0 * ay0 + h1 * ay1 + (1 << 21)) >> 22;
        o[ch] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

// display (uniform batch, map b at the display size h x w, photo b ih x iw): the mask of n, and the composite - cv2.resize of the photo where the
// mask is 255, CheckerPattern() where it is 0: A = 169 where ((y - t) mod 64 < 32) == ((x - l) mod 64 < 32), else B = 214, t = max(h - 64, 0) / 2,
// l = max(w - 64, 0) / 2 (toadui/helpers/checker_pattern.py: 32-px tiles, BORDER_WRAP padding, cropped). MASK_PX pixels of the flat image per thread.
__global__ __launch_bounds__(256) void mask_display_kernel(const PlaneMap m, double tmin, double tmax, int invert, const unsigned char* __restrict__ img,
                                                           int ih, int iw, unsigned char* __restrict__ mask_out, unsigned char* __restrict__ comp_out) {
    const int b = blockIdx.y;
    const Plane plane = plane_of(m.coef, b);
    const int dt = m.dt, h = m.h, w = m.w;
    const void* map = m.in;
    const double factor = m.factor;
    float lo, hi;
    double vlo, vrange;
    seg_range(m.parts, b, lo, hi);
    seg_vrange(m.vparts, b, vlo, vrange);
    const size_t n = (size_t)h * w, base = (size_t)b * n;
    const unsigned char* src = img + (size_t)b * ih * iw * 3;
    const double scale_x = 1.0 / ((double)w / (double)iw), scale_y = 1.0 / ((double)h / (double)ih);
    const int top = max(h - 64, 0) / 2, left = max(w - 64, 0) / 2;
    for (size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * MASK_PX; p0 < n; p0 += (size_t)gridDim.x * blockDim.x * MASK_PX) {
        const int cnt = n - p0 < (size_t)MASK_PX ? (int)(n - p0) : MASK_PX;
        int y = (int)(p0 / w), x = (int)(p0 % w);
        CvTap ty = cv_tap(y, scale_y, ih);
        unsigned mword = 0u;
        unsigned char px[MASK_PX * 3];
#pragma unroll
        for (int k = 0; k < MASK_PX; ++k) {
            px[k * 3] = px[k * 3 + 1] = px[k * 3 + 2] = 0;
            if (k >= cnt) continue;
            const unsigned m = mask_byte(plane_norm(map, base, dt, w, x, y, lo, hi, plane.c, factor, vlo, vrange), tmin, tmax, invert);
            mword |= m << (8 * k);
            if (m) {
                bgr_lerp_u8(src, iw, cv_tap(x, scale_x, iw), ty, px + k * 3);
            } else {
                const unsigned char v = (((y - top) & 63) < 32) == (((x - left) & 63) < 32) ? 169 : 214;
                px[k * 3] = px[k * 3 + 1] = px[k * 3 + 2] = v;
            }
            if (++x == w) {
                x = 0;
                ty = cv_tap(++y, scale_y, ih);
            }
        }
        unsigned char* mo = mask_out + base + p0;
        unsigned char* co = comp_out + (base + p0) * 3;
        if (cnt == MASK_PX && ((uintptr_t)mo & 3) == 0) {
            *(unsigned*)mo = mword;
        } else {
            for (int k = 0; k < cnt; ++k) mo[k] = (unsigned char)(mword >> (8 * k));
        }
        if (cnt == MASK_PX && ((uintptr_t)co & 3) == 0) {
            unsigned wd[3];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                wd[q] = (unsigned)px[4 * q] | (unsigned)px[4 * q + 1] << 8 | (unsigned)px[4 * q + 2] << 16 | (unsigned)px[4 * q + 3] << 24;
            *(Bytes12*)co = Bytes12{wd[0], wd[1], wd[2]};
        } else {
            for (int k = 0; k < cnt * 3; ++k) co[k] = px[k];
        }
    }
}

// cutout (one photo per blockIdx.y, any sizes): s = cv2.resize(n, (iw, ih)) in fp64 from the 2 x 2 map taps evaluated on the fly, the mask of s,
// BGRA = (BGR AND mask, mask), both at the photo's packed offset. The taps of consecutive pixels are shared where they repeat (an enlargement).
__global__ __launch_bounds__(256) void mask_cutout_kernel(const MaskTable t, double factor, double tmin, double tmax, int invert,
                                                          unsigned char* __restrict__ out_bgra, unsigned char* __restrict__ out_mask) {
    const MaskImage& im = t.im[blockIdx.y];
    float lo, hi;
    double vlo, vrange;
    seg_range(im.parts, 0, lo, hi);
    seg_vrange(im.vparts, 0, vlo, vrange);
    const int dt = t.dt, h = im.h, w = im.w, ih = im.ih, iw = im.iw;
    const void* map = im.map;
    const double* c = im.coef;
    const unsigned char* img = im.img;
    const double scale_x = 1.0 / ((double)iw / (double)w), scale_y = 1.0 / ((double)ih / (double)h);
    const size_t n = (size_t)ih * iw;
    unsigned char* bgra = out_bgra + im.off * 4;
    unsigned char* msk = out_mask + im.off;
    for (size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * MASK_PX; p0 < n; p0 += (size_t)gridDim.x * blockDim.x * MASK_PX) {
        const int cnt = n - p0 < (size_t)MASK_PX ? (int)(n - p0) : MASK_PX;
        const unsigned char* in = img + p0 * 3;
        unsigned wd[3] = {0u, 0u, 0u};
        if (cnt == MASK_PX && ((uintptr_t)in & 3) == 0) {
            const Bytes12 v = *(const Bytes12*)in;
            wd[0] = v.w0;
            wd[1] = v.w1;
            wd[2] = v.w2;
        } else {
            for (int k = 0; k < cnt * 3; ++k) wd[k >> 2] |= (unsigned)in[k] << (8 * (k & 3));
        }
        int y = (int)(p0 / iw), x = (int)(p0 % iw);
        CvTap ty = cv_tap(y, scale_y, h);
        int key_x = -1, key_y = -1;
        double n00 = 0.0, n01 = 0.0, n10 = 0.0, n11 = 0.0;
        unsigned mword = 0u, px[MASK_PX];
#pragma unroll
        for (int k = 0; k < MASK_PX; ++k) {
            px[k] = 0u;
            if (k >= cnt) continue;
            const CvTap tx = cv_tap(x, scale_x, w);
            const bool bx = tx.s1 != tx.s0, by = ty.s1 != ty.s0;
            if (2 * tx.s0 + bx != key_x || 2 * ty.s0 + by != key_y) {
                key_x = 2 * tx.s0 + bx;
                key_y = 2 * ty.s0 + by;
                n00 = plane_norm(map, 0, dt, w, tx.s0, ty.s0, lo, hi, c, factor, vlo, vrange);
                n01 = bx ? plane_norm(map, 0, dt, w, tx.s1, ty.s0, lo, hi, c, factor, vlo, vrange) : n00;
                n10 = by ? plane_norm(map, 0, dt, w, tx.s0, ty.s1, lo, hi, c, factor, vlo, vrange) : n00;
                n11 = bx && by ? plane_norm(map, 0, dt, w, tx.s1, ty.s1, lo, hi, c, factor, vlo, vrange) : (bx ? n01 : n10);
            }
            const double s = lerp_cv64(lerp_cv64(n00, n01, tx.a), lerp_cv64(n10, n11, tx.a), ty.a);
            const unsigned m = mask_byte(s, tmin, tmax, invert);
            mword |= m << (8 * k);
            // BGR of pixel k: bytes 3k .. 3k + 2 of the loaded words
            unsigned bgr = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) bgr |= ((wd[(3 * k + ch) >> 2] >> (8 * ((3 * k + ch) & 3))) & 255u) << (8 * ch);
            px[k] = (m ? bgr : 0u) | m << 24;
            if (++x == iw) {
                x = 0;
                ty = cv_tap(++y, scale_y, h);
            }
        }
        unsigned char* bo = bgra + p0 * 4;
        unsigned char* mo = msk + p0;
        if (cnt == MASK_PX && ((uintptr_t)bo & 15) == 0) {
            *(uint4*)bo = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
            for (int k = 0; k < cnt; ++k) *(unsigned*)(bo + 4 * k) = px[k];  // (the BGRA output is 4-byte aligned: checked by the entry point)
        }
        if (cnt == MASK_PX && ((uintptr_t)mo & 3) == 0) {
            *(unsigned*)mo = mword;
        } else {
            for (int k = 0; k < cnt; ++k) mo[k] = (unsigned char)(mword >> (8 * k));
        }
    }
}

}  // namespace

int mdpt_launch_post_plane_fit(const void* in, int dt, int B, int h, int w, const unsigned* parts, const int* xy, int N, size_t xy_stride, double* coef,
                               hipStream_t stream) {
    post_launch("plane_fit_kernel", plane_fit_kernel, dim3(B), dim3(256), stream, in, dt, h, w, parts, xy, N, xy_stride, coef);
    return (int)hipGetLastError();
}

int mdpt_launch_post_plane_eval(const double* coef, int B, int h, int w, float* out, hipStream_t stream) {
    const size_t n = (size_t)h * w;
    post_launch("plane_eval_kernel", plane_eval_kernel, dim3(grid_seg(n), B), dim3(256), stream, coef, h, w, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_plane_minmax(const PlaneMap& m, double* vparts, hipStream_t stream) {
    post_launch("plane_minmax_kernel", plane_minmax_kernel, dim3(SEG_PARTS, m.B), dim3(256), stream, m, vparts);
    return (int)hipGetLastError();
}

int mdpt_launch_post_threshold(const PlaneMap& m, double tmin, double delta, int mode, int reverse, void* out, unsigned* hist, hipStream_t stream) {
    const dim3 grid(grid_seg((size_t)m.h * m.w), m.B);
    if (mode == 1) post_launch("threshold_kernel", threshold_kernel<1>, grid, dim3(256), stream, m, tmin, delta, reverse, out, hist);
    else post_launch("threshold_kernel", threshold_kernel<0>, grid, dim3(256), stream, m, tmin, delta, reverse, out, hist);
    return (int)hipGetLastError();
}

int mdpt_launch_post_edge_mag(const float* in, int B, int h, int w, const unsigned* parts, const float* blur_w, int ksize, float* mag, unsigned* mag_max,
                              hipStream_t stream) {
    if (ksize < 1 || ksize > 2 * EDGE_MAX_PAD + 1 || ksize % 2 == 0) return (int)hipErrorInvalidValue;
    EdgeBlur blur{};
    for (int i = 0; i < ksize * ksize; ++i) blur.w[i] = blur_w[i];
    blur.ksize = ksize;
    hipError_t e = hipMemsetAsync(mag_max, 0, sizeof(unsigned) * (size_t)B, stream);
    if (e != hipSuccess) return (int)e;
    post_launch("edge_mag_kernel", edge_mag_kernel, dim3((w + EDGE_TILE - 1) / EDGE_TILE, (h + EDGE_TILE - 1) / EDGE_TILE, B), dim3(256), stream, in, h, w,
                parts, blur, mag, mag_max);
    return (int)hipGetLastError();
}

int mdpt_launch_post_edge_mask(const float* mag, const unsigned* mag_max, int B, size_t n, unsigned char* out, hipStream_t stream) {
    post_launch("edge_mask_kernel", edge_mask_kernel, dim3(grid_seg(n), B), dim3(256), stream, mag, mag_max, n, out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_pack_u24(const float* in, int B, size_t n, const unsigned* parts, int lossy, const float* mag, const unsigned* mag_max,
                              const unsigned char* mask, size_t mask_stride, unsigned char* out, hipStream_t stream) {
    post_launch("pack_u24_kernel", pack_u24_kernel, dim3(grid_seg(n), B), dim3(256), stream, in, n, parts, lossy, mag, mag_max, mask, mask_stride,
                (uchar4*)out);
    return (int)hipGetLastError();
}

int mdpt_launch_post_mask_display(const PlaneMap& m, double tmin, double tmax, int invert, const unsigned char* img, int ih, int iw, unsigned char* mask,
                                  unsigned char* comp, hipStream_t stream) {
    const size_t g = ((size_t)m.h * m.w + 256 * MASK_PX - 1) / (256 * MASK_PX);
    post_launch("mask_display_kernel", mask_display_kernel, dim3(g > 512 ? 512 : (int)g, m.B), dim3(256), stream, m, tmin, tmax, invert, img, ih, iw, mask,
                comp);
    return (int)hipGetLastError();
}

int mdpt_launch_post_mask_cutout(const MaskTable& t, double factor, double tmin, double tmax, int invert, unsigned char* bgra, unsigned char* mask,
                                 hipStream_t stream) {
    if (t.n <= 0 || t.n > MDPT_MASK_IMAGES) return (int)hipErrorInvalidValue;
    size_t most = 0;
    for (int k = 0; k < t.n; ++k) most = (size_t)t.im[k].ih * t.im[k].iw > most ? (size_t)t.im[k].ih * t.im[k].iw : most;
    const size_t g = (most + 256 * MASK_PX - 1) / (256 * MASK_PX);
    post_launch("mask_cutout_kernel", mask_cutout_kernel, dim3(g > 2048 ? 2048 : (int)g, t.n), dim3(256), stream, t, factor, tmin, tmax, invert, bgra, mask);
    return (int)hipGetLastError();
}
