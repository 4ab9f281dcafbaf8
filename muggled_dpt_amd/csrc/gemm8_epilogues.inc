// gemm.hip, part 4: direct (register -> global) epilogues of the 8-phase kernel.
// ------------------------------------------------------------------------------------------------------------
// Variant B ("8-phase"), 256x256 tile, 8 waves, 64-deep K tiles double-buffered in LDS (128 KiB), 16x16x32 MFMAs.
//
// Two K tiles per loop iteration, four phases per K tile; a phase is
//     { ds_read this phase's register sub-tile | issue the LDS-DMA of ONE half-tile | barrier | 16 MFMAs | barrier }.
// The two wave groups (waves 0-3 / 4-7: one wave of each group per SIMD) run the same program ONE BARRIER apart, so while
// one group issues its MFMA block the other one reads LDS and issues DMA - the matrix pipe sees back-to-back MFMA blocks.
// A wave owns four 64x32 quadrants of the tile, (qm, qn) = rows qm*128 + grp*64, cols qn*128 + wc*32: every 128-row A
// half-tile and every 128-column B half-tile of a K tile is therefore read in exactly one phase,
//     P1: B0, A0 -> MFMA(0,0)    P2: B1 -> MFMA(0,1)    P3: A1 -> MFMA(1,1)    P4: (none) -> MFMA(1,0)
// and can be re-staged early. DMA schedule (e/o = even/odd LDS buffer, t = this iteration's first K tile):
//     P1: -          P2: B0e(t+2)  P3: A0e(t+2)  P4: B1e(t+2), A1e(t+2) + vmcnt(8)
//     P5: -          P6: B0o(t+3)  P7: A0o(t+3)  P8: B1o(t+3), A1o(t+3) + vmcnt(8)
// (round 3: A1 moved out of the 12-read phases P1 / P5 into P4 / P8, which read nothing - QKV 243.9 -> 240.3 us, fc1 372.0 -> 368.0 us on
// one box, profiles/r03_gemm8_schedule_ab.txt.) vmcnt(8) (the 4 half-tiles x 2 DMA instructions issued since the last wait stay in
// flight) at P4 retires the odd buffer, which is read in P5-P7, and at P8 the even buffer, read in P1-P3 of the next iteration: the
// wait sits one phase (>= one workgroup barrier that both groups have passed) before the first read. WAR: a half-tile is re-staged two
// phases after the phase that read it; B0 and A1 are re-staged ONE phase later, which is safe because the reading phase retires those
// reads BEFORE its first barrier (P1 / P5: lgkmcnt(8) for the 4 B reads, issued first, order pinned; P3 / P7: lgkmcnt(0)).
// ------------------------------------------------------------------------------------------------------------
// Direct (register -> global) epilogues of the 8-phase kernel for tiles computed with SWAPPED MFMA operands
// (acc = mfma(B frag, A frag)): a lane then owns, for output row m = 16-row block + (lane & 15), four CONSECUTIVE columns
// n = 16-col block + 4*(lane >> 4) + r - fp32 values go out as 16-byte vectors straight from the accumulators, and a bf16
// result gets its 8-column / 16-byte vectors by one v_permlane16_swap per register pair between lanes l and l^16
// (even 16-lane rows collect block j = 0, odd rows block j = 1). No LDS round trip. Everything is unrolled over the 128
// accumulator registers, so only the three hot epilogues of the encoder get this form (small code, no per-row feature
// branches); every other combination runs the plain operand order + the LDS-strip epilogue:
//   DM_BF16  : out_hi(/lo) = act(acc + bias)                    (fc1 + GELU; plain bf16 outputs)
//   DM_RESID : out_f32 = resid + gamma * (acc + bias), fp32      (attention proj, fc2: in-place residual update)
//   DM_QK    : Q (pre-scaled) / K head-major bf16(/lo)            (QKV tiles without V columns)
//   DM_F32   : out_f32 = acc + bias, fp32                          (1x1 projections, SwinV2 QKV / proj / fc2, SwiGLU inner linear)
//   DM_RINIT : the DM_F32 epilogue behind a main loop whose accumulators were INITIALISED with the residual tile (attention proj,
//              fc2 with the layer scale folded into the packed weights and bias): out = (resid + A W'^T) + bias'. The 256 KB residual
//              read of a tile streams in under the first K tiles instead of sitting exposed in the epilogue.
//   DM_VT    : V transposed, token-contiguous (epilogue_direct_vt: PLAIN operand order, a lane owns 4 consecutive tokens)
//   DM_SWQK  : SwinV2 cosine-attention Q / K (heads of 32): L2-normalised, Q times the head's logit scale, scattered to window order
//              (QKV tiles without V columns when GemmParams::swin_tokmap is set; the V tiles of that GEMM use DM_F32)
//   DM_SWVT  : SwinV2 V columns written as the transposed window operand (4-token runs, plain operand order like DM_VT)
// Per-image bias tables in the direct epilogues exist in the fp16 build only (the bf16 build's kernels stay exactly what round 3 tuned);
// launches that carry one in the bf16 build run the strip-epilogue kernels.
constexpr bool HAVE_IMGB = MDPT_OP_IS_F16 != 0;
enum { DM_NONE = 0, DM_BF16 = 1, DM_RESID = 2, DM_QK = 3, DM_VT = 4, DM_F32 = 5, DM_RINIT = 6, DM_SWQK = 7, DM_SWVT = 8 };

// Everything that selects code is a template parameter (MODE, X3 = hi+lo output planes, ACT) and every memory access is a raw
// buffer op whose out-of-range lanes (tail rows: offset beyond num_records; tail columns: offset forced to ~0) are dropped by
// the hardware bounds check. No divergent branch means hipcc can count vmcnt: with `if (row < M) store` every store sat in its
// own basic block behind an `s_waitcnt vmcnt(0)`, i.e. each store waited for the previous one's write acknowledgement
// (measured: 520 cycles per store, 33-42k cycles for the in-place residual form whose loads waited the same way).
// Row addresses advance by uniform strides; DM_RESID reads back exactly the 16-byte groups it writes, group g+1's loads are
// issued ahead of group g's stores.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(unsigned)(bytes < 0xFFFFFFF0ull ? bytes : 0xFFFFFFF0ull), 0x00020000);
}

// IMGB: per-image bias table (GemmParams::bias_img_stride, rows of bias_img_rows >= 256 per image - the token-mean compensation of the
// weight rounding, mdpt_stages.cpp wrc_bias): a 256-row tile lies in at most two images, rows from tile-local index `bnd` on take the
// next image's bias vector. One select per value, then the SAME single add as every other form of the epilogue ((acc + bias) ...).
template <int MODE, bool X3, int ACT, bool IMGB = false>
__device__ __forceinline__ void epilogue_direct(const GemmParams& p, f32x4 (&acc)[2][2][4][2], int m0, int n0, int grp, int wc, int lane) {
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int l15 = lane & 15, lh = lane >> 4;
    const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256;  // valid rows of this tile (tail tile: fewer)
    int bnd = 1 << 30;  // tile-local row where the next image starts (IMGB)
    const float* bias0 = p.bias;
    const float* bias1 = p.bias;
    if (IMGB) {
        const int img0 = m0 / p.bias_img_rows;
        bnd = (img0 + 1) * p.bias_img_rows - m0;
        bias0 = p.bias + (size_t)img0 * p.bias_img_stride;
        bias1 = bnd < rows_here ? bias0 + p.bias_img_stride : bias0;
    }
    auto pick = [&](const f32x4& a, const f32x4& b, bool next) {  // (IMGB only) per-lane select, no arithmetic
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = next ? b[e] : a[e];
        return r;
    };

    if (MODE == DM_F32) {
        const __amdgpu_buffer_rsrc_t rs = tile_rsrc(p.out_f32 + (size_t)m0 * p.ldc, (size_t)rows_here * p.ldc * 4);
        const unsigned row_b = (unsigned)p.ldc * 4u;
        const float inv_s = (MDPT_OP_IS_F16 && p.wscale) ? p.wscale[1] : 1.0f;  // power-of-two weight scale (GemmParams::wscale): exact
#pragma unroll
        for (int qn = 0; qn < 2; ++qn) {
            f32x4 bias[2], biasn[2];
            unsigned col_off[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nc = n0 + qn * 128 + wc * 32 + j * 16 + 4 * lh;
                bias[j] = p.bias ? *(const f32x4*)(bias0 + (nc < p.N ? nc : p.N - 4)) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (IMGB) biasn[j] = *(const f32x4*)(bias1 + (nc < p.N ? nc : p.N - 4));
                col_off[j] = nc < p.N ? (unsigned)nc * 4u : OOB;
            }
#pragma unroll
            for (int qm = 0; qm < 2; ++qm)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned row = (unsigned)(qm * 128 + grp * 64 + i * 16 + l15) * row_b;
                    const bool next = IMGB && qm * 128 + grp * 64 + i * 16 + l15 >= bnd;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const f32x4 a = MDPT_OP_IS_F16 ? acc[qm][qn][i][j] * inv_s : acc[qm][qn][i][j];
                        const f32x4 v = a + (IMGB ? pick(bias[j], biasn[j], next) : bias[j]);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, col_off[j] == OOB ? OOB : row + col_off[j], 0, 0);
                    }
                }
        }
        return;
    }
    if (MODE == DM_RESID) {
        // in-place residual update; descriptor over this tile's rows (base = row m0), byte offsets inside it
        const __amdgpu_buffer_rsrc_t rs = tile_rsrc(p.out_f32 + (size_t)m0 * p.ldc, (size_t)rows_here * p.ldc * 4);
        const unsigned row_b = (unsigned)p.ldc * 4u;
        f32x4 bias[2][2], gam[2][2];
        unsigned col_off[2][2];
#pragma unroll
        for (int qn = 0; qn < 2; ++qn)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nc = n0 + qn * 128 + wc * 32 + j * 16 + 4 * lh;
                const int ncl = nc < p.N ? nc : p.N - 4;
                bias[qn][j] = *(const f32x4*)(p.bias + ncl);
                gam[qn][j] = *(const f32x4*)(p.gamma + ncl);
                col_off[qn][j] = nc < p.N ? (unsigned)nc * 4u : OOB;
            }
        auto row_off = [&](int g, int i) { return (unsigned)((g >> 1) * 128 + grp * 64 + i * 16 + l15) * row_b; };  // group g = 2 qm + qn
        // vmcnt retires in order, so a wait for loads that were issued after a store also waits for that store's write
        // acknowledgement (~2 us). Order: loads of groups 0,1 -> results 0,1 computed in registers -> loads of groups 2,3
        // (into the registers the finished accumulators free) -> stores 0,1 -> wait for loads 2,3 only -> stores 2,3.
        u32x4 old[4][4][2];
        f32x4 res[2][4][2];
        auto load_group = [&](int g) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned c = col_off[g & 1][j];
                    old[g][i][j] = __builtin_amdgcn_raw_buffer_load_b128(rs, c == OOB ? OOB : row_off(g, i) + c, 0, 0);
                }
        };
        auto value = [&](int g, int i, int j) {
            return (acc[g >> 1][g & 1][i][j] + bias[g & 1][j]) * gam[g & 1][j] + __builtin_bit_cast(f32x4, old[g][i][j]);
        };
        auto store = [&](int g, int i, int j, f32x4 v) {
            const unsigned c = col_off[g & 1][j];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, c == OOB ? OOB : row_off(g, i) + c, 0, 0);
        };
        // test hook (dbg_times): wave 0 stamps [epilogue start, loads 0,1 issued, loads 0,1 landed, loads 2,3 + stores 0,1 issued,
        // loads 2,3 landed, all stores issued] behind the 6 per-workgroup slots of every workgroup
        unsigned long long* stamp = p.dbg_times && threadIdx.x == 0 ? p.dbg_times + (size_t)gridDim.x * 6 + (size_t)blockIdx.x * 16 : nullptr;
        if (stamp) stamp[0] = memtime_now();
        load_group(0);
        load_group(1);
        if (p.dbg_times) {
            if (stamp) stamp[1] = memtime_now();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (stamp) stamp[2] = memtime_now();
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) res[g][i][j] = value(g, i, j);
        load_group(2);
        load_group(3);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) store(g, i, j, res[g][i][j]);
        if (p.dbg_times) {
            if (stamp) stamp[3] = memtime_now();
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            if (stamp) stamp[4] = memtime_now();
        }
#pragma unroll
        for (int g = 2; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) store(g, i, j, value(g, i, j));
        if (stamp) stamp[5] = memtime_now();
        return;
    }

    // ---- bf16 outputs
    __amdgpu_buffer_rsrc_t rs_hi, rs_lo;
    __amdgpu_buffer_rsrc_t rs_lo8 = tile_rsrc(p.out_hi, 0), rs_a8 = rs_lo8;
    if (MODE == DM_BF16) {
        rs_hi = tile_rsrc(p.out_hi + (size_t)m0 * p.ldc, (size_t)rows_here * p.ldc * 2);
        rs_lo = tile_rsrc(X3 ? p.out_lo + (size_t)m0 * p.ldc : p.out_hi, X3 ? (size_t)rows_here * p.ldc * 2 : 0);
        if (MDPT_HAVE_F8 && X3 && p.out_f8) {  // byte planes: the residue plane, the values' plane out_f8 bytes behind it
            rs_lo8 = tile_rsrc((const unsigned char*)p.out_lo + (size_t)m0 * p.ldc, (size_t)rows_here * p.ldc);
            rs_a8 = tile_rsrc((const unsigned char*)p.out_lo + p.out_f8 + (size_t)m0 * p.ldc, p.out_a8 ? (size_t)rows_here * p.ldc : 0);
        }
    }
    // per-column constants of this lane's 4-column groups, both column halves loaded before the first store (a wait placed
    // after a store would also wait for that store's acknowledgement)
    f32x4 bias_q[2][2], biasn_q[2][2], gam_q[2][2];
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ncol = n0 + qn * 128 + wc * 32 + j * 16 + 4 * lh;
            const int nc = ncol < p.N ? ncol : p.N - 4;  // clamped: out-of-range columns are never stored
            bias_q[qn][j] = p.bias ? *(const f32x4*)(bias0 + nc) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (IMGB) biasn_q[qn][j] = *(const f32x4*)(bias1 + nc);
            if (MODE == DM_QK && ncol < p.F) gam_q[qn][j] = f32x4{p.qscale, p.qscale, p.qscale, p.qscale};
            else if (MODE == DM_QK) gam_q[qn][j] = f32x4{1.0f, 1.0f, 1.0f, 1.0f};
        }
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
        const int nq = n0 + qn * 128 + wc * 32;
        const int n8 = nq + (lh & 1) * 16 + (lh >> 1) * 8;  // first of the 8 columns this lane stores as bf16
        const f32x4(&bias)[2] = bias_q[qn];
        const f32x4(&biasn)[2] = biasn_q[qn];
        const f32x4(&gam)[2] = gam_q[qn];
        // QKV: this wave's 32 columns lie in one of the Q / K planes (F is a multiple of 64): wave-uniform descriptor
        int qk_h = 0, qk_d = 0;
        if (MODE == DM_QK) {
            const int which = __builtin_amdgcn_readfirstlane(nq >= p.F);
            const int fcol = n8 - which * p.F;
            qk_h = fcol >> 6; qk_d = fcol & 63;
            const size_t plane = (size_t)p.M * p.F * 2;  // [B, heads, npad, 64] bf16 (M = B * npad); < 4 GiB checked by the caller
            rs_hi = tile_rsrc(which ? p.k_hi : p.q_hi, plane);
            rs_lo = tile_rsrc(X3 ? (which ? p.k_lo : p.q_lo) : p.q_hi, X3 ? plane : 0);
        }
        const bool nok = n8 < p.N;
#pragma unroll
        for (int qm = 0; qm < 2; ++qm) {
            const int rfirst = qm * 128 + grp * 64 + l15;  // tile-local row of block i is rfirst + 16 i
            int qb = 0, qt = 0;
            if (MODE == DM_QK) {
                qb = (m0 + rfirst) / p.npad;
                qt = m0 + rfirst - qb * p.npad;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 v[2];
                const bool next = IMGB && rfirst + 16 * i >= bnd;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    v[j] = acc[qm][qn][i][j] + (IMGB ? pick(bias[j], biasn[j], next) : bias[j]);
                    if (MODE == DM_QK) {
                        v[j] *= gam[j];
                    } else if (ACT == MDPT_ACT_GELU) {
#pragma unroll
                        for (int e = 0; e < 4; e += 2) {
                            const gelu_f32x2 g2 = gelu_erf2(gelu_f32x2{v[j][e], v[j][e + 1]});
                            v[j][e] = g2[0];
                            v[j][e + 1] = g2[1];
                        }
                    } else if (ACT == MDPT_ACT_RELU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[j][e] = fmaxf(v[j][e], 0.0f);
                    }
                }
                // pack pairs, exchange halves with lane ^ 16, one 16-byte store (two in x3 mode)
                unsigned hw_[2][2], lw_[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int w2 = 0; w2 < 2; ++w2) {
                        const f32x2 pp = {v[j][2 * w2], v[j][2 * w2 + 1]};
                        const opx2 hh = to_op2(pp);
                        hw_[j][w2] = __builtin_bit_cast(unsigned, hh);
                        if (X3) {
                            const f32x2 rr = pp - __builtin_convertvector(hh, f32x2);
                            lw_[j][w2] = __builtin_bit_cast(unsigned, to_op2(rr));
                        }
                    }
                unsigned ph[4], pl[4];
#pragma unroll
                for (int w2 = 0; w2 < 2; ++w2) {
                    auto r = __builtin_amdgcn_permlane16_swap(hw_[0][w2], hw_[1][w2], false, false);
                    ph[w2] = r[0];
                    ph[w2 + 2] = r[1];
                    if (X3) {
                        auto rl = __builtin_amdgcn_permlane16_swap(lw_[0][w2], lw_[1][w2], false, false);
                        pl[w2] = rl[0];
                        pl[w2 + 2] = rl[1];
                    }
                }
                unsigned off;
                if (MODE == DM_BF16) {
                    off = ((unsigned)(rfirst + 16 * i) * (unsigned)p.ldc + (unsigned)n8) * 2u;  // rows >= M lie beyond num_records
                    if (!nok) off = OOB;
                } else {
                    off = (unsigned)((((size_t)(qb * p.heads + qk_h) * p.npad + qt) * 64 + qk_d) * 2);
                    if (!nok || m0 + rfirst + 16 * i >= p.M) off = OOB;
                }
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{ph[0], ph[1], ph[2], ph[3]}, rs_hi, off, 0, 0);
#if MDPT_HAVE_F8
                if (X3 && MODE == DM_BF16 && p.out_f8) {
                    // the lo plane in the fp8 form an F8 consumer reads (f8_cross.h): this lane's 8 columns -> 8 e5m2 bytes of the residue (and
                    // of the values), from the SAME fp32 values and fp16 roundings as the 16-bit form; byte offset = element offset = off / 2
                    float hv[2][4], vv[2][4];
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int w2 = 0; w2 < 2; ++w2) {
                            const f32x2 hf = __builtin_convertvector(__builtin_bit_cast(opx2, hw_[j][w2]), f32x2);
                            hv[j][2 * w2] = hf[0]; hv[j][2 * w2 + 1] = hf[1];
                            vv[j][2 * w2] = v[j][2 * w2]; vv[j][2 * w2 + 1] = v[j][2 * w2 + 1];
                        }
                    unsigned l8[2], a8[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        l8[j] = f8_lo8x4(vv[j][0], vv[j][1], vv[j][2], vv[j][3], hv[j][0], hv[j][1], hv[j][2], hv[j][3]);
                        a8[j] = f8_a8x4(hv[j][0], hv[j][1], hv[j][2], hv[j][3]);
                    }
                    // lanes l / l ^ 16 exchange like the 16-bit words: even 16-lane rows collect column block j = 0, odd rows j = 1
                    auto rl = __builtin_amdgcn_permlane16_swap(l8[0], l8[1], false, false);
                    const unsigned off8 = off == OOB ? OOB : off >> 1;
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{rl[0], rl[1]}, rs_lo8, off8, 0, 0);
                    if (p.out_a8) {
                        auto ra = __builtin_amdgcn_permlane16_swap(a8[0], a8[1], false, false);
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{ra[0], ra[1]}, rs_a8, off8, 0, 0);
                    }
                } else
#endif
                if (X3) __builtin_amdgcn_raw_buffer_store_b128(u32x4{pl[0], pl[1], pl[2], pl[3]}, rs_lo, off, 0, 0);
                if (MODE == DM_QK) {  // next row block: token + 16, rolling over into the next image
                    qt += 16;
                    while (qt >= p.npad) { qt -= p.npad; ++qb; }
                }
            }
        }
    }
}

// SwinV2 window-attention operands straight out of a Q / K tile of the QKV GEMM (windowed_attention.py:100-123: F.normalize(q), F.normalize(k),
// q * exp(clamped logit scale)). Heads are 32 wide = the 32 columns one wave owns in a quadrant: a lane holds two 4-column groups of a row (groups
// lh and 4 + lh of the head), the four lanes lane, lane^16, lane^32, lane^48 hold the row's whole head. |.|^2 is summed in the order
// swin_qk_prep_kernel (swin.hip) uses on the fp32 QKV rows - (a^2 + b^2) + (c^2 + d^2) per group, group c with group c+4, then the neighbour
// group pair, then the other half - with unfused multiplies, so the fused and the unfused form of a block give the same bits whichever tile
// rule picks which. Rows scatter through the token map: image token t -> swin_tokmap[t] = w*heads*npad + i, + img*swin_img_rows + h*npad.
template <bool X3, bool IMGB = false>
__device__ __forceinline__ void epilogue_swin_qk(const GemmParams& p, f32x4 (&acc)[2][2][4][2], int m0, int n0, int grp, int wc, int lane) {
#pragma clang fp contract(off)
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int l15 = lane & 15, lh = lane >> 4;
    const size_t plane = (size_t)(p.M / p.swin_N) * p.swin_img_rows * 64;  // bytes of a Q / K plane (< 4 GiB: checked by the caller)
    // IMGB: per-image bias table (token-mean compensation, see epilogue_direct): >= 256 token rows per image, two bias vectors per tile
    int bnd = 1 << 30;
    const float* bias0 = p.bias;
    const float* bias1 = p.bias;
    if (IMGB) {
        const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256;
        const int img0 = m0 / p.bias_img_rows;
        bnd = (img0 + 1) * p.bias_img_rows - m0;
        bias0 = p.bias + (size_t)img0 * p.bias_img_stride;
        bias1 = bnd < rows_here ? bias0 + p.bias_img_stride : bias0;
    }
    // everything that is loaded comes before the first store (a wait after a store also waits for the store)
    f32x4 bias_q[2][2], biasn_q[2][2];
    float scale_q[2];
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
        const int nq = n0 + qn * 128 + wc * 32;
        const int which = __builtin_amdgcn_readfirstlane(nq >= p.F);
        const float ls = p.swin_logit_scale[(nq - which * p.F) >> 5];
        scale_q[qn] = which ? 1.0f : ls;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            bias_q[qn][j] = p.bias ? *(const f32x4*)(bias0 + nq + j * 16 + 4 * lh) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (IMGB) biasn_q[qn][j] = *(const f32x4*)(bias1 + nq + j * 16 + 4 * lh);
        }
    }
    int dst[2][4];
#pragma unroll
    for (int qm = 0; qm < 2; ++qm) {
        const int r0 = m0 + qm * 128 + grp * 64 + l15;
        int img = r0 / p.swin_N, t = r0 - img * p.swin_N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dst[qm][i] = r0 + 16 * i < p.M ? img * p.swin_img_rows + p.swin_tokmap[t] : -1;
            t += 16;
            while (t >= p.swin_N) { t -= p.swin_N; ++img; }
        }
    }
    const int d8 = (lh & 1) * 16 + (lh >> 1) * 8;  // first of the 8 head columns this lane stores (after the lane^16 exchange)
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
        // (Q | K plane and head recomputed here, wave-uniform scalars: kept in arrays across the loops above they became a pointer table in scratch)
        const int nq = n0 + qn * 128 + wc * 32;
        const int which = __builtin_amdgcn_readfirstlane(nq >= p.F);
        const __amdgpu_buffer_rsrc_t rs_hi = tile_rsrc(which ? p.k_hi : p.q_hi, plane);
        const __amdgpu_buffer_rsrc_t rs_lo = tile_rsrc(X3 ? (which ? p.k_lo : p.q_lo) : p.q_hi, X3 ? plane : 0);
        const int hrow = ((nq - which * p.F) >> 5) * p.npad;
#pragma unroll
        for (int qm = 0; qm < 2; ++qm)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 v[2];
                float sg[2];
                const bool next = IMGB && qm * 128 + grp * 64 + 16 * i + l15 >= bnd;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    f32x4 bj = bias_q[qn][j];
                    if (IMGB) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) bj[e] = next ? biasn_q[qn][j][e] : bj[e];
                    }
                    v[j] = acc[qm][qn][i][j] + bj;
                    sg[j] = (v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3]);
                }
                float ss = sg[0] + sg[1];
                // cross-lane sums with the swap instructions: swap(x, x) leaves [R0 R0 R2 R2] / [R1 R1 R3 R3] (rows of 16 lanes) resp.
                // [lo lo] / [hi hi] in the two registers. The results go through scalars: __builtin_bit_cast applied to an element of the
                // returned vector reads element 0 both times (DESIGN.md bug 4)
                {
                    const unsigned u = __builtin_bit_cast(unsigned, ss);
                    auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
                    const unsigned r0 = r[0], r1 = r[1];
                    ss = __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
                }
                {
                    const unsigned u = __builtin_bit_cast(unsigned, ss);
                    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                    const unsigned r0 = r[0], r1 = r[1];
                    ss = __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
                }
                float scale = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
                scale *= scale_q[qn];
                unsigned hw_[2][2], lw_[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int w2 = 0; w2 < 2; ++w2) {
                        const f32x2 pp = {v[j][2 * w2] * scale, v[j][2 * w2 + 1] * scale};
                        const opx2 hh = to_op2(pp);
                        hw_[j][w2] = __builtin_bit_cast(unsigned, hh);
                        if (X3) {
                            const f32x2 rr = pp - __builtin_convertvector(hh, f32x2);
                            lw_[j][w2] = __builtin_bit_cast(unsigned, to_op2(rr));
                        }
                    }
                unsigned ph[4], pl[4];
#pragma unroll
                for (int w2 = 0; w2 < 2; ++w2) {
                    auto r = __builtin_amdgcn_permlane16_swap(hw_[0][w2], hw_[1][w2], false, false);
                    ph[w2] = r[0];
                    ph[w2 + 2] = r[1];
                    if (X3) {
                        auto rl = __builtin_amdgcn_permlane16_swap(lw_[0][w2], lw_[1][w2], false, false);
                        pl[w2] = rl[0];
                        pl[w2 + 2] = rl[1];
                    }
                }
                const unsigned off = dst[qm][i] < 0 ? OOB : (unsigned)(((size_t)(dst[qm][i] + hrow) * 32 + d8) * 2);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{ph[0], ph[1], ph[2], ph[3]}, rs_hi, off, 0, 0);
                if (X3) __builtin_amdgcn_raw_buffer_store_b128(u32x4{pl[0], pl[1], pl[2], pl[3]}, rs_lo, off, 0, 0);
            }
    }
}

// SwinV2 V columns as the window attention's transposed operand Vt[(img*nw + w)*heads + h][d][npadv] (what swin_v_prep_kernel builds from
// fp32 rows: bf16(acc + bias), lo = bf16(v - hi) in bf16x3 mode - the same two conversions). Plain operand order: a lane owns 4 consecutive
// rows = image tokens t .. t+3 (t % 4 == 0) of one column; the caller guarantees grid width, window width and shift are multiples of 4,
// so the four tokens are consecutive positions of one window: one 8-byte store per lane, row block and column. Pad positions [wa, npadv)
// are zeroed by the caller once per stage.
template <bool X3, bool IMGB = false>
__device__ __forceinline__ void epilogue_swin_vt(const GemmParams& p, f32x4 (&acc)[2][2][4][2], int m0, int n0, int grp, int wc, int lane) {
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int l15 = lane & 15, lh = lane >> 4;
    const size_t plane = (size_t)(p.M / p.swin_N) * p.swin_img_velems * 2;  // bytes; < 4 GiB checked by the caller
    const __amdgpu_buffer_rsrc_t rs_hi = tile_rsrc(p.vt_hi, plane);
    const __amdgpu_buffer_rsrc_t rs_lo = tile_rsrc(X3 ? p.vt_lo : p.vt_hi, X3 ? plane : 0);
    int bnd = 1 << 30;  // IMGB: per-image bias table, see epilogue_direct_vt (a lane's 4 rows never straddle two images: token counts are multiples of 4)
    const float* bias0 = p.bias;
    const float* bias1 = p.bias;
    if (IMGB) {
        const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256;
        const int img0 = m0 / p.bias_img_rows;
        bnd = (img0 + 1) * p.bias_img_rows - m0;
        bias0 = p.bias + (size_t)img0 * p.bias_img_stride;
        bias1 = bnd < rows_here ? bias0 + p.bias_img_stride : bias0;
    }
    float bias_q[2][2], biasn_q[2][2];
    int col_q[2][2];
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + qn * 128 + wc * 32 + j * 16 + l15;
            bias_q[qn][j] = p.bias ? bias0[n < p.N ? n : p.N - 1] : 0.0f;
            if (IMGB) biasn_q[qn][j] = bias1[n < p.N ? n : p.N - 1];
            col_q[qn][j] = n < p.N ? (n - 2 * p.F) * p.npadv : -1;  // (h*32 + d) * npadv
        }
    int dst[2][4];
#pragma unroll
    for (int qm = 0; qm < 2; ++qm) {
        const int r0 = m0 + qm * 128 + grp * 64 + 4 * lh;
        int img = r0 / p.swin_N, t = r0 - img * p.swin_N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dst[qm][i] = r0 + 16 * i < p.M ? img * p.swin_img_velems + p.swin_vtokmap[t] : -1;
            t += 16;
            while (t >= p.swin_N) { t -= p.swin_N; ++img; }
        }
    }
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int qm = 0; qm < 2; ++qm)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bool next = IMGB && qm * 128 + grp * 64 + 16 * i + 4 * lh >= bnd;
                    const f32x4 v = acc[qm][qn][i][j] + (next ? biasn_q[qn][j] : bias_q[qn][j]);
                    unsigned hw_[2], lw_[2];
#pragma unroll
                    for (int w2 = 0; w2 < 2; ++w2) {
                        const f32x2 pp = {v[2 * w2], v[2 * w2 + 1]};
                        const opx2 hb = to_op2(pp);
                        hw_[w2] = __builtin_bit_cast(unsigned, hb);
                        if (X3) {
                            const f32x2 rr = pp - __builtin_convertvector(hb, f32x2);
                            lw_[w2] = __builtin_bit_cast(unsigned, to_op2(rr));
                        }
                    }
                    const unsigned off = dst[qm][i] < 0 || col_q[qn][j] < 0 ? OOB : (unsigned)(dst[qm][i] + col_q[qn][j]) * 2u;
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{hw_[0], hw_[1]}, rs_hi, off, 0, 0);
                    if (X3) __builtin_amdgcn_raw_buffer_store_b64(u32x2{lw_[0], lw_[1]}, rs_lo, off, 0, 0);
                }
}

// V columns of the QKV GEMM, written transposed: Vt[(b, h, d)][token]. With the PLAIN MFMA operand order a lane owns 4 consecutive
// rows (tokens 4*(lane>>4) .. +3 of a 16-row block) of one column, i.e. 8 bytes of a Vt row; v_permlane16_swap between the two
// 16-column blocks of the quadrant gives lanes (lane>>4) = 0,1 the 8 tokens 0-7 of a column of block 0 / block 1 and lanes 2,3
// the tokens 8-15: one 16-byte store per lane and row block, no LDS. Same arithmetic as the strip path (bias add, hi/lo split).
template <bool X3, bool IMGB = false>
__device__ __forceinline__ void epilogue_direct_vt(const GemmParams& p, f32x4 (&acc)[2][2][4][2], int m0, int n0, int grp, int wc, int lane) {
    constexpr unsigned OOB = 0xFFFFFFF0u;
    const int l15 = lane & 15, lh = lane >> 4;
    const size_t plane = (size_t)(p.M / p.npad) * p.F * p.npadv * 2;  // [B, heads, 64, npadv] bf16; < 4 GiB checked by the caller
    const __amdgpu_buffer_rsrc_t rs_hi = tile_rsrc(p.vt_hi, plane);
    const __amdgpu_buffer_rsrc_t rs_lo = tile_rsrc(X3 ? p.vt_lo : p.vt_hi, X3 ? plane : 0);
    // IMGB: per-image bias table, see epilogue_direct. A lane's 4 rows (tokens) start at a multiple of 4 and images at multiples of 8
    // rows: the four values of a register quad always belong to one image
    int bnd = 1 << 30;
    const float* bias0 = p.bias;
    const float* bias1 = p.bias;
    if (IMGB) {
        const int rows_here = p.M - m0 < 256 ? p.M - m0 : 256;
        const int img0 = m0 / p.bias_img_rows;
        bnd = (img0 + 1) * p.bias_img_rows - m0;
        bias0 = p.bias + (size_t)img0 * p.bias_img_stride;
        bias1 = bnd < rows_here ? bias0 + p.bias_img_stride : bias0;
    }
    float bias_q[2][2], biasn_q[2][2];
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + qn * 128 + wc * 32 + j * 16 + l15;
            bias_q[qn][j] = bias0[n < p.N ? n : p.N - 1];
            if (IMGB) biasn_q[qn][j] = bias1[n < p.N ? n : p.N - 1];
        }
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
        const int ncol = n0 + qn * 128 + wc * 32 + (lh & 1) * 16 + l15;  // the column this lane stores after the swap
        const int fcol = ncol - 2 * p.F, hh = fcol >> 6, dd = fcol & 63;
        const bool nok = ncol < p.N;
#pragma unroll
        for (int qm = 0; qm < 2; ++qm) {
            const int mfirst = m0 + qm * 128 + grp * 64 + (lh >> 1) * 8;  // first of this lane's 8 tokens in row block 0
            int qb = mfirst / p.npad, qt = mfirst - qb * p.npad;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned hw_[2][2], lw_[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // plain operand order: this lane's rows of block i are qm*128 + grp*64 + 16 i + 4 lh .. + 3
                    const bool next = IMGB && qm * 128 + grp * 64 + 16 * i + 4 * lh >= bnd;
                    const f32x4 v = acc[qm][qn][i][j] + (next ? biasn_q[qn][j] : bias_q[qn][j]);
#pragma unroll
                    for (int w2 = 0; w2 < 2; ++w2) {
                        const f32x2 pp = {v[2 * w2], v[2 * w2 + 1]};
                        const opx2 hb = to_op2(pp);
                        hw_[j][w2] = __builtin_bit_cast(unsigned, hb);
                        if (X3) {
                            const f32x2 rr = pp - __builtin_convertvector(hb, f32x2);
                            lw_[j][w2] = __builtin_bit_cast(unsigned, to_op2(rr));
                        }
                    }
                }
                unsigned ph[4], pl[4];
#pragma unroll
                for (int w2 = 0; w2 < 2; ++w2) {
                    auto r = __builtin_amdgcn_permlane16_swap(hw_[0][w2], hw_[1][w2], false, false);
                    ph[w2] = r[0];
                    ph[w2 + 2] = r[1];
                    if (X3) {
                        auto rl = __builtin_amdgcn_permlane16_swap(lw_[0][w2], lw_[1][w2], false, false);
                        pl[w2] = rl[0];
                        pl[w2 + 2] = rl[1];
                    }
                }
                unsigned off = (unsigned)((((size_t)(qb * p.heads + hh) * 64 + dd) * p.npadv + qt) * 2);
                if (!nok || mfirst + 16 * i >= p.M) off = OOB;
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{ph[0], ph[1], ph[2], ph[3]}, rs_hi, off, 0, 0);
                if (X3) __builtin_amdgcn_raw_buffer_store_b128(u32x4{pl[0], pl[1], pl[2], pl[3]}, rs_lo, off, 0, 0);
                qt += 16;
                while (qt >= p.npad) { qt -= p.npad; ++qb; }
            }
        }
    }
}
