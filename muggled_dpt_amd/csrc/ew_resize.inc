// ---- bilinear resize, align_corners=True (components/misc_helpers.py:39-42): src = dst*(in-1)/(out-1). Three kernels, one set of source
// coordinates (up_scale / up_tap): the direct and the LDS-tiled fp32 -> operand plane forms must round identically (batch-size independent
// bits), and the bf16 -> bf16 form must give the bits conv3h.hip computes for its halo.

namespace {

// scale pair of a resize and, per output pixel (y, x), the four source taps (y0 | y1, x0 | x1) with the weights (ly, lx) of the second row / column
struct UpScale { float sy, sx; };
struct UpTap { int y0, x0, y1, x1; float ly, lx; };
__device__ __forceinline__ UpScale up_scale(int Hi, int Wi, int Ho, int Wo) {
#pragma clang fp contract(off)
    return UpScale{Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.0f, Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.0f};
}
__device__ __forceinline__ UpTap up_tap(UpScale s, int y, int x, int Hi, int Wi) {
#pragma clang fp contract(off)  // (no fma(sx, x, -x0))
    const float fy = s.sy * (float)y, fx = s.sx * (float)x;
    const int y0 = (int)fy, x0 = (int)fx;
    return UpTap{y0, x0, y0 + (y0 < Hi - 1), x0 + (x0 < Wi - 1), fy - (float)y0, fx - (float)x0};
}

// NHWC fp32 in -> bf16 hi(/lo) and/or fp32 out. One thread = CPT (4 or 8) channels of one output pixel: a CU retires
// about one store instruction per 64 cycles whatever its width, so the bf16 output wants 16-byte (8-channel) stores.
template <int CPT>
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo,
                                                       float* out_f32, int B, int Hi, int Wi, int Ho, int Wo, int C, size_t out_f8, int out_a8) {
#pragma clang fp contract(off)  // the direct and the tiled kernel must round identically (batch-size independent bits)
    const int cq = C / CPT;
    const size_t total = (size_t)B * Ho * Wo * cq;
    const UpScale s = up_scale(Hi, Wi, Ho, Wo);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % cq) * CPT;
        const size_t pix = idx / cq;
        const int x = (int)(pix % Wo);
        const int y = (int)((pix / Wo) % Ho);
        const int b = (int)(pix / ((size_t)Wo * Ho));
        const UpTap t = up_tap(s, y, x, Hi, Wi);
        const float* base = in + (size_t)b * Hi * Wi * C + c;
        const size_t o = pix * C + c;
        f32x4 v[CPT / 4];
#pragma unroll
        for (int q = 0; q < CPT / 4; ++q) {
            const f32x4 v00 = *(const f32x4*)(base + ((size_t)t.y0 * Wi + t.x0) * C + 4 * q);
            const f32x4 v01 = *(const f32x4*)(base + ((size_t)t.y0 * Wi + t.x1) * C + 4 * q);
            const f32x4 v10 = *(const f32x4*)(base + ((size_t)t.y1 * Wi + t.x0) * C + 4 * q);
            const f32x4 v11 = *(const f32x4*)(base + ((size_t)t.y1 * Wi + t.x1) * C + 4 * q);
            v[q] = (1.0f - t.ly) * ((1.0f - t.lx) * v00 + t.lx * v01) + t.ly * ((1.0f - t.lx) * v10 + t.lx * v11);
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

// LDS-tiled form for the big maps (fp32 NHWC in, bf16 hi(/lo) out): a workgroup owns an 8x8 block of OUTPUT pixels, stages the
// (at most 7x7) source patch they interpolate from once in LDS and reads its four neighbours per pixel from there. The direct
// kernel issues four 16-byte global loads per 8-byte result and tops out at ~2.5 TB/s on the vector-memory path; here the
// source is read from global once (x1.2-1.7 halo), so the kernel is limited by the unavoidable HBM bytes.
// Same arithmetic, same operation order as upsample_kernel (bit-identical results).
template <int C8>  // channels / 8 (lanes per pixel): 32 -> C = 256, 16 -> C = 128, 8 -> C = 64
__global__ __launch_bounds__(256) void upsample_tiled_kernel(const float* __restrict__ in, op_t* out_hi, op_t* out_lo, int B, int Hi,
                                                             int Wi, int Ho, int Wo, size_t out_f8, int out_a8) {
#pragma clang fp contract(off)
    constexpr int C = C8 * 8, TS = 8, PS = 7;  // tile side, max patch side
    extern __shared__ __attribute__((aligned(16))) float patch[];  // [PS*PS][C]
    const int tiles_x = (Wo + TS - 1) / TS, tiles_y = (Ho + TS - 1) / TS;
    const int bt = blockIdx.x;
    const int tx = bt % tiles_x, ty = (bt / tiles_x) % tiles_y, b = bt / (tiles_x * tiles_y);
    const UpScale s = up_scale(Hi, Wi, Ho, Wo);
    const float sy = s.sy, sx = s.sx;
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
        const UpTap t = up_tap(s, y, x, Hi, Wi);
        const float* p00 = patch + (size_t)((t.y0 - py0) * PS + (t.x0 - px0)) * C + lane_c;
        const float* p01 = patch + (size_t)((t.y0 - py0) * PS + (t.x1 - px0)) * C + lane_c;
        const float* p10 = patch + (size_t)((t.y1 - py0) * PS + (t.x0 - px0)) * C + lane_c;
        const float* p11 = patch + (size_t)((t.y1 - py0) * PS + (t.x1 - px0)) * C + lane_c;
        f32x4 v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4 v00 = *(const f32x4*)(p00 + 4 * q), v01 = *(const f32x4*)(p01 + 4 * q);
            const f32x4 v10 = *(const f32x4*)(p10 + 4 * q), v11 = *(const f32x4*)(p11 + 4 * q);
            v[q] = (1.0f - t.ly) * ((1.0f - t.lx) * v00 + t.lx * v01) + t.ly * ((1.0f - t.lx) * v10 + t.lx * v11);
        }
        const size_t o = (((size_t)b * Ho + y) * Wo + x) * C + lane_c;
        opx8 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h[e] = to_op(v[0][e]); h[e + 4] = to_op(v[1][e]); }
        *(opx8*)(out_hi + o) = h;
        if (out_lo) lo_store8(out_lo, o, out_f8, out_a8, v[0], v[1], h);
    }
}

// bf16 NHWC -> bf16 NHWC bilinear (align_corners=True) resize, 8 channels (16 bytes) per thread: the stand-alone form of the upsample in
// front of the head's first conv for launches too small for the halo-staged conv kernel that interpolates its own input (conv3h.hip).
// Same arithmetic (up_bf16.h), so both forms give the same bits.
__global__ __launch_bounds__(256) void upsample_bf16src_kernel(const op_t* __restrict__ in, op_t* __restrict__ out, int B, int Hi, int Wi, int Ho,
                                                               int Wo, int C) {
#pragma clang fp contract(off)  // the source coordinates and weights must be the bits conv3h.hip computes (no fma(sx, x, -x0))
    const int c8 = C >> 3;
    const size_t total = (size_t)B * Ho * Wo * c8;
    const UpScale s = up_scale(Hi, Wi, Ho, Wo);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % c8);
        const size_t pix = idx / c8;
        const int x = (int)(pix % Wo), y = (int)((pix / Wo) % Ho), b = (int)(pix / ((size_t)Wo * Ho));
        const UpTap t = up_tap(s, y, x, Hi, Wi);
        const op_t* base = in + (size_t)b * Hi * Wi * C + ch * 8;
        const mdpt_u32x4 v00 = *(const mdpt_u32x4*)(base + ((size_t)t.y0 * Wi + t.x0) * C), v01 = *(const mdpt_u32x4*)(base + ((size_t)t.y0 * Wi + t.x1) * C);
        const mdpt_u32x4 v10 = *(const mdpt_u32x4*)(base + ((size_t)t.y1 * Wi + t.x0) * C), v11 = *(const mdpt_u32x4*)(base + ((size_t)t.y1 * Wi + t.x1) * C);
        *(mdpt_u32x4*)(out + pix * C + ch * 8) = mdpt_up_bf16x8(v00, v01, v10, v11, t.lx, t.ly);
    }
}

}  // namespace

int MDPT_FN(mdpt_launch_upsample)(const float* in, op_t* out_hi, op_t* out_lo, float* out_f32, int B, int Hi, int Wi, int Ho, int Wo,
                         int C, hipStream_t stream, size_t out_f8, int out_a8) {
    if (C & 3) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)B * Ho * Wo * (C / 4);
    MdptProfScope prof("upsample_kernel", 0.0, stream);  // one label for the direct and the tiled form
    // big bf16 outputs with 64 / 128 / 256 channels and a source span of at most 7 pixels per 8 output pixels (scale >= ~1.2): tiled
    const bool span_ok = (long)7 * (Hi - 1) <= (long)5 * (Ho - 1) && (long)7 * (Wi - 1) <= (long)5 * (Wo - 1);
    if (out_hi && !out_f32 && (C == 256 || C == 128 || C == 64) && span_ok && (size_t)B * Ho * Wo >= 65536) {
        const dim3 tiles(B * ((Ho + 7) / 8) * ((Wo + 7) / 8));
        const size_t lds = (size_t)49 * C * 4;
        if (C == 256) {
            if (const int e = mdpt_lds_limit<upsample_tiled_kernel<32>>(64 * 1024)) return e;
            return ew_launch(upsample_tiled_kernel<32>, tiles, dim3(256), lds, stream, in, out_hi, out_lo, B, Hi, Wi, Ho, Wo, out_f8, out_a8);
        }
        if (C == 128) return ew_launch(upsample_tiled_kernel<16>, tiles, dim3(256), lds, stream, in, out_hi, out_lo, B, Hi, Wi, Ho, Wo, out_f8, out_a8);
        return ew_launch(upsample_tiled_kernel<8>, tiles, dim3(256), lds, stream, in, out_hi, out_lo, B, Hi, Wi, Ho, Wo, out_f8, out_a8);
    }
    if ((C & 7) == 0 && out_hi)
        return ew_launch(upsample_kernel<8>, dim3(grid_for(total / 2)), dim3(256), 0, stream, in, out_hi, out_lo, out_f32, B, Hi, Wi, Ho, Wo, C, out_f8, out_a8);
    return ew_launch(upsample_kernel<4>, dim3(grid_for(total)), dim3(256), 0, stream, in, out_hi, out_lo, out_f32, B, Hi, Wi, Ho, Wo, C, out_f8, out_a8);
}

int MDPT_FN(mdpt_launch_upsample_bf16)(const op_t* in, op_t* out, int B, int Hi, int Wi, int Ho, int Wo, int C, hipStream_t stream) {
    if (C & 7) return (int)hipErrorInvalidValue;
    return ew_launch("upsample_bf16src_kernel", 0.0, upsample_bf16src_kernel, dim3(grid_for((size_t)B * Ho * Wo * (C / 8))), dim3(256), 0, stream, in, out, B, Hi, Wi, Ho, Wo, C);
}
