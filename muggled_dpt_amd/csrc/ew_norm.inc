// ---- row-wise kernels behind the GEMMs: LayerNorm (alone, and as the reduction of a K-split GEMM), the K-split finish, the per-token L2 norm,
// the SwiGLU gate, and the token-mean compensation of the weight rounding (column means + the skinny product against the residue plane)

namespace {

// LayerNorm (eps 1e-6, reference components/misc_helpers.py:190-210): one wave per row, row held in
// registers (F <= 64*4*MAXV), two-pass mean / centred variance in fp32.
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

// ViT-G SwiGLU gate (reference components/misc_helpers.py:182-185): in fp32 [rows, 2h] = (a | b) -> silu(a) * b as
// bf16 hi (+lo) [rows, hp], columns [h, hp) zero (K padding of the outer GEMM). One thread = 4 columns.
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

}  // namespace

int MDPT_FN(mdpt_launch_layernorm)(const float* x, const float* gamma, const float* beta, op_t* out_hi, op_t* out_lo, float* out_f32,
                          int rows, int F, hipStream_t stream, size_t out_f8, int out_a8) {
    if ((F & 3) || F > 64 * 4 * LN_MAXV) return (int)hipErrorInvalidValue;
    if (rows <= 0) return 0;
    return ln_dispatch(F, [&](auto nv) {
        return ew_launch("layernorm_kernel", 0.0, layernorm_kernel<decltype(nv)::value>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, gamma, beta, out_hi, out_lo,
                         out_f32, rows, F, out_f8, out_a8);
    });
}

int MDPT_FN(mdpt_launch_layernorm_addp)(float* x, const float* part, size_t part_stride, int npart, const float* gamma, const float* beta,
                                       op_t* out_hi, op_t* out_lo, float* out_f32, int rows, int F, hipStream_t stream, size_t out_f8, int out_a8) {
    if ((F & 3) || F > 64 * 4 * LN_MAXV || !part || npart < 1) return (int)hipErrorInvalidValue;
    if (rows <= 0) return 0;
    return ln_dispatch(F, [&](auto nv) {
        return ew_launch("layernorm_addp_kernel", 0.0, layernorm_addp_kernel<decltype(nv)::value>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, part, part_stride,
                         npart, gamma, beta, out_hi, out_lo, out_f32, rows, F, out_f8, out_a8);
    });
}

int MDPT_FN(mdpt_launch_ksplit_finish)(const float* part, size_t part_stride, int nparts, const float* bias, float* out_f32, op_t* out_hi, op_t* out_lo,
                                      int relu_planes, int M, int N, int ldc, hipStream_t stream, size_t out_f8, int out_a8) {
    if (!part || nparts < 1 || (N & 3) || (ldc & 3) || M <= 0) return (int)hipErrorInvalidValue;
    return ew_launch("ksplit_finish_kernel", 0.0, ksplit_finish_kernel, dim3(grid_for((size_t)M * (N / 4))), dim3(256), 0, stream, part, part_stride, nparts, bias,
                     out_f32, out_hi, out_lo, relu_planes, M, N, ldc, out_f8, out_a8);
}

int MDPT_FN(mdpt_launch_row_norm)(const float* in, float* norm_out, float* chan_out, int chan, int B, int ntok, int npad, int skip, int F,
                                  hipStream_t stream) {
    if (B <= 0 || ntok <= 0 || F <= 0 || skip < 0 || skip + ntok > npad || (chan_out && (chan < 0 || chan >= F))) return (int)hipErrorInvalidValue;
    if (!norm_out && !chan_out) return 0;
    const size_t rows = (size_t)B * ntok;
    return ew_launch("row_norm_kernel", 0.0, row_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, in, norm_out, chan_out, chan, B, ntok, npad, skip,
                     F, (F % 4 == 0 && ((uintptr_t)in & 15) == 0) ? 1 : 0);
}

int MDPT_FN(mdpt_launch_swiglu)(const float* in, op_t* out_hi, op_t* out_lo, size_t rows, int h, int hp, hipStream_t stream) {
    if ((h & 3) || (hp & 3) || hp < h) return (int)hipErrorInvalidValue;
    return ew_launch("swiglu_kernel", 0.0, swiglu_kernel, dim3(grid_for(rows * (hp / 4))), dim3(256), 0, stream, in, out_hi, out_lo, rows, h, hp);
}

int MDPT_FN(mdpt_launch_colmean)(const op_t* A, int lda, int B, int rows_per_img, int nreal, int step, int K, op_t* mean, hipStream_t stream) {
    if (B <= 0 || nreal <= 0 || nreal > rows_per_img || step <= 0 || (K & 7) || (lda & 7)) return (int)hipErrorInvalidValue;
    return ew_launch("colmean_kernel", 0.0, colmean_kernel, dim3((K + 127) / 128, B), dim3(1024), 0, stream, A, lda, rows_per_img, nreal, step, K, mean);
}

int MDPT_FN(mdpt_launch_wrc_table)(const op_t* mean, const op_t* w_lo, const float* bias, float* out, int B, int N, int K, hipStream_t stream, const float* wscale) {
    if (B <= 0 || N <= 0 || K <= 0 || (K & 31)) return (int)hipErrorInvalidValue;
    return ew_launch("wrc_table_kernel", 2.0 * B * N * K, wrc_table_kernel, dim3((N + 15) / 16), dim3(1024), 0, stream, mean, w_lo, bias, out, B, N, K, wscale);
}
