// ---- token setup and token layout: patchify (+ the NaN poison of a flagged image), the position-embedding resize, the cls / pad rows of the
// residual stream, the transposed-V pad columns, the token import / export of the stage-level API, the BEiT relative position tables

namespace {

// patchify: NCHW fp32 -> rows [B*Np][Kp] with k = c*P*P + ky*P + kx (the conv weight's own flatten
// order, patch_embed.py:56-62,92), zero padded to Kp. One thread = 4 consecutive k.
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

__global__ __launch_bounds__(256) void tokens_import_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo, int B,
                                                            int N, int npad, int F, size_t out_f8, int out_a8) {
    const size_t total = (size_t)B * npad * F;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int t = (int)((idx / F) % npad);
        const int b = (int)(idx / ((size_t)F * npad));
        const float v = t < N ? in[((size_t)b * N + t) * F + f] : 0.0f;
        plane_store1(out_hi, out_lo, idx, v, out_f8, out_a8);
    }
}

// lo_f8 != 0: in_lo is the e5m2 residue plane of an F8 consumer (plane_load1)
__global__ __launch_bounds__(256) void tokens_export_kernel(const op_t* in_hi, const op_t* in_lo, const float* in_f32,
                                                            float* __restrict__ out, int B, int N, int npad, int F, int skip_cls, size_t lo_f8) {
    const int nout = N - skip_cls;
    const size_t total = (size_t)B * nout * F;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(idx % F);
        const int t = (int)((idx / F) % nout);
        const int b = (int)(idx / ((size_t)F * nout));
        const size_t o = ((size_t)b * npad + t + skip_cls) * F + f;
        const float v = in_f32 ? in_f32[o] : plane_load1(in_hi, in_lo, o, lo_f8);
        out[idx] = v;
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

}  // namespace

int MDPT_FN(mdpt_launch_patchify)(const void* img, int img_dtype, op_t* out_hi, op_t* out_lo, int B, int H, int W, int P, int Kp, hipStream_t stream,
                                  unsigned* poison) {
    const size_t total = (size_t)B * (H / P) * (W / P) * (Kp / 4);
    return ew_launch("patchify_kernel", 0.0, patchify_kernel, dim3(grid_for(total)), dim3(256), 0, stream, img, img_dtype, out_hi, out_lo, B, H, W, P, Kp, poison);
}

int MDPT_FN(mdpt_launch_poison_depth)(void* depth, int depth_dtype, const unsigned* poison, int B, size_t hw, hipStream_t stream) {
    const unsigned gx = (unsigned)((hw + 256 * 8 - 1) / (256 * 8));
    return ew_launch("poison_depth_kernel", 0.0, poison_depth_kernel, dim3(gx < 1 ? 1 : gx, B), dim3(256), 0, stream, depth, depth_dtype, poison, hw);
}

int MDPT_FN(mdpt_launch_posembed)(const float* base, float* out, int Gh, int Gw, int gh, int gw, int F, hipStream_t stream) {
    return ew_launch("posembed_kernel", 0.0, posembed_kernel, dim3(grid_for((size_t)gh * gw * F)), dim3(256), 0, stream, base, out, Gh, Gw, gh, gw, F);
}

int MDPT_FN(mdpt_launch_init_tokens)(float* resid, const float* cls_token, const float* cls_embed, int B, int N, int npad, int F, hipStream_t stream) {
    const size_t total = (size_t)B * (1 + npad - N) * F;
    return ew_launch("init_tokens_kernel", 0.0, init_tokens_kernel, dim3(grid_for(total)), dim3(256), 0, stream, resid, cls_token, cls_embed, B, N, npad, F);
}

int MDPT_FN(mdpt_launch_zero_vt_pad)(op_t* vt_hi, op_t* vt_lo, int rows, int N, int npadv, hipStream_t stream) {
    if (npadv == N) return 0;
    return ew_launch("zero_vt_pad_kernel", 0.0, zero_vt_pad_kernel, dim3(grid_for((size_t)rows * (npadv - N))), dim3(256), 0, stream, vt_hi, vt_lo, rows, N, npadv);
}

int MDPT_FN(mdpt_launch_tokens_import)(const float* in, op_t* out_hi, op_t* out_lo, int B, int N, int npad, int F, hipStream_t stream, size_t out_f8, int out_a8) {
    return ew_launch(tokens_import_kernel, dim3(grid_for((size_t)B * npad * F)), dim3(256), 0, stream, in, out_hi, out_lo, B, N, npad, F, out_f8, out_a8);
}

int MDPT_FN(mdpt_launch_tokens_export)(const op_t* in_hi, const op_t* in_lo, const float* in_f32, float* out, int B, int N, int npad,
                              int F, int skip_cls, hipStream_t stream, size_t lo_f8) {
    return ew_launch(tokens_export_kernel, dim3(grid_for((size_t)B * (N - skip_cls) * F)), dim3(256), 0, stream, in_hi, in_lo, in_f32, out, B, N, npad, F, skip_cls, lo_f8);
}

int MDPT_FN(mdpt_launch_tokens_to_resid)(const float* tokens, const float* pos, float* resid, int B, int Np, int npad, int F, hipStream_t stream) {
    return ew_launch(tokens_to_resid_kernel, dim3(grid_for((size_t)B * Np * F)), dim3(256), 0, stream, tokens, pos, resid, B, Np, npad, F);
}

int MDPT_FN(mdpt_beit_relpos_elen)(int gh, int gw) {
    const int rw = 2 * gw - 1, R = (2 * gh - 1) * rw, T = (gh - 1) * rw + gw - 1;
    return 2 * R + 2 * T + 2;
}

// workgroups of a relpos launch: one thread per table entry of a block, and at least one per (padded) token
static int beit_relpos_grid(int heads, int gh, int gw, int ntok_pad) {
    const size_t total = (size_t)heads * MDPT_FN(mdpt_beit_relpos_elen)(gh, gw);
    return grid_for(total > (size_t)ntok_pad ? total : (size_t)ntok_pad);
}

int MDPT_FN(mdpt_launch_beit_relpos_batch)(const BeitRelposBatch& b, hipStream_t stream) {
    if (b.n < 1 || b.n > 32) return (int)hipErrorInvalidValue;
    return ew_launch(beit_relpos_batch_kernel, dim3(beit_relpos_grid(b.heads, b.gh, b.gw, b.ntok_pad), b.n), dim3(256), 0, stream, b);
}

int MDPT_FN(mdpt_launch_beit_relpos)(const float* ref_lut, float* ext_lut, int* tq, int* tk, int heads, int Gh, int Gw, int gh, int gw, int N,
                            int ntok_pad, hipStream_t stream) {
    return ew_launch(beit_relpos_kernel, dim3(beit_relpos_grid(heads, gh, gw, ntok_pad)), dim3(256), 0, stream, ref_lut, ext_lut, tq, tk, heads, Gh, Gw, gh, gw, N, ntok_pad);
}
