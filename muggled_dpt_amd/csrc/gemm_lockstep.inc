// gemm.hip, part 3: the lockstep main loop (BM x BN x 64 tiles, 2- or 3-deep LDS ring) incl. the K-split forms of its 64x64 tile.
// ------------------------------------------------------------------------------------------------------------
// Variant A ("lockstep"): all waves run  wait-DMA -> barrier -> issue next DMA -> LDS reads -> MFMAs  together.
// Used for small tiles (128x128, 2 workgroups per CU) and the 32-wide head tile.
// ------------------------------------------------------------------------------------------------------------
// F8 (fp16 build, BK = 64, generic / depth-to-space epilogues): the launch runs its cross-term passes on fp8 planes (GemmParams::f8) - kernels of
// their own, so that every other launch keeps the code and the register allocation it had
template <int BM, int BN, int WM, int WN, int BK, int NST, int MINW, int AMODE, int EKIND, bool F8 = false>
__global__ __launch_bounds__(64 * WM * WN, MINW) void gemm_kernel(const GemmParams p) {
    static_assert(!F8 || (MDPT_HAVE_F8 && BK == 64), "fp8 cross terms: fp16 build, 64-element K tiles");
    constexpr int NW = WM * WN;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    using St = Stager<BM, BN, NW, BK, AMODE, F8>;
    constexpr int ROWB = St::ROWB, CPR = St::CPR, RPB = St::RPB, NLOAD = St::NLOAD, A_BYTES = St::A_BYTES, STAGE = St::SLAB;
    constexpr int KSTEPS = BK / 16;     // 32x32x16 MFMA k-steps per slab
    static_assert(BK == 32 || BK == 64, "BK");
    static_assert(NST == 2 || NST == 3, "ring depth");
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
    static_assert(32 * WTN * 4 * NW <= NST * STAGE, "epilogue strip must fit in the ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned long long t_start = 0, t_first = 0, t_loop = 0;
    if (p.dbg_times) t_start = memtime_now();

    int m0, n0;
    tile_coords((p.N + BN - 1) / BN, BM, BN, m0, n0);
    // K split (GemmParams::ksplit; the launcher sets grid.y for the 64x64 dense / generic instantiations only): range z of the K axis
    constexpr bool KSPLIT = (AMODE == MDPT_A_DENSE || AMODE == MDPT_A_CONV3) && EKIND == MDPT_E_GENERIC && BM == 64 && BN == 64 && BK == 64;
    const int kz = KSPLIT ? (int)blockIdx.y : 0;
    const int kspan = KSPLIT && p.ksplit > 1 ? p.K / p.ksplit : p.K;
    St st;
    st.init(p, m0, n0, wave, lane, kz * kspan, kspan);

    // ---- fragment read offsets: row = 32*blk + (lane&31), chunk = 2*kk + (lane>>5), swizzled with key(row)
    const int l31 = lane & 31, half = lane >> 5;
    const int sw_frag = (l31 / RPB) & (CPR - 1);
    int frag_off[KSTEPS];
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) frag_off[kk] = l31 * ROWB + (((kk * 2 + half) ^ sw_frag) << 4);
    const int wm = wave / WN, wn = wave % WN;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    if (EKIND == MDPT_E_GENERIC && p.acc_init && kz == 0) {
        // residual GEMMs (out = resid + A W^T + bias, in place): the accumulators START at the residual, the epilogue adds the bias and
        // stores - the same order of operations in every tile variant (see gemm8_body's RI form, where this hides the residual read
        // under the main loop). acc[i][j][r] = C[32 i + (r&3) + 8 (r>>2) + 4 half][32 j + (lane&31)]; out-of-range elements read 0.
        // descriptor over THIS tile's rows (base = row m0, byte offsets inside the tile: < BM * ldr * 4, so no 32-bit wrap however large M is)
        const int mw = m0 + (wave / WN) * WTM, nw = n0 + (wave % WN) * WTN;
        const size_t tile_bytes = (size_t)(p.M - m0 < BM ? p.M - m0 : BM) * p.ldr * 4;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.resid + (size_t)m0 * p.ldr), 0, (int)(unsigned)(tile_bytes < 0xFFFFFFF0ull ? tile_bytes : 0xFFFFFFF0ull), 0x00020000);
        const float s_in = (MDPT_OP_IS_F16 && p.wscale) ? p.wscale[0] : 1.0f;  // power-of-two weight scale (GemmParams::wscale): the residual enters the accumulators scaled alike
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = nw + j * 32 + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const unsigned off = (n < p.N && m < p.M) ? ((unsigned)(m - m0) * (unsigned)p.ldr + (unsigned)n) * 4u : 0xFFFFFFF0u;
                    acc[i][j][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
                    if (MDPT_OP_IS_F16) acc[i][j][r] *= s_in;
                }
            }
    }

    // ---- main loop: NST-deep LDS ring. Iteration t: wait for THIS wave's DMA of slab t (counted vmcnt: with a
    //      3-deep ring the DMA of slab t+1 stays in flight across the barrier), barrier (everybody's part of slab t
    //      has landed AND everybody finished reading slab t-1), refill the slot of slab t-1 with slab t+NST-1, compute.
    //      LDS-DMA completion is only tracked by vmcnt: the waits are explicit (hipcc does not reliably insert them).
    // GemmParams::f8 (fp16 build, BK = 64): the first T8 K tiles are fp8 tiles of the cross-term passes (f8_cross.h); a lane's two 16-byte reads of
    // k-steps (2 s, 2 s + 1) are the 32 operand bytes of one 32x32x64 MFMA. wsc / wsc_lo: the E8M0 scales of the weight rows this lane's column
    // blocks read (byte j = block j), of the W_hi plane and of the W - W_hi plane.
    constexpr bool F8C = F8;
    static_assert(!F8 || TN <= 4, "one scale byte per 32-column block of a wave");
    const int T8 = F8C ? ktiles_f8(p, kspan) : 0, T8a = F8C ? kspan / 128 : 0;
    const int total = F8C ? ktiles_total(p, kspan) : (kspan / BK) * p.npass;
    int wsc = 0, wsc_lo = 0;
    if constexpr (F8C) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            int n = n0 + wn * WTN + j * 32 + l31;
            n = n < p.N ? n : p.N - 1;
            wsc |= (int)p.S8[n] << (8 * j);
            if (p.npass == 3) wsc_lo |= (int)p.S8_lo[n] << (8 * j);
        }
    }
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < total) st.issue(p, smem + s * STAGE, wave);
    int rd = 0, wr = NST - 1;
    for (int t = 0; t < total; ++t) {
        if (NST == 3 && t + 1 < total) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLOAD) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (p.dbg_times && t == 0) t_first = memtime_now();
        if (t + NST - 1 < total) st.issue(p, smem + wr * STAGE, wave);
        const char* sA = smem + rd * STAGE + wm * WTM * ROWB;
        const char* sB = smem + rd * STAGE + A_BYTES + wn * WTN * ROWB;
        opx8 a0[TM], b0[TN], a1[TM], b1[TN];
#define LOAD_FRAGS(A_, B_, KK_)                                                                           \
    do {                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) A_[i] = *(const opx8*)(sA + i * 32 * ROWB + frag_off[KK_]); \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) B_[j] = *(const opx8*)(sB + j * 32 * ROWB + frag_off[KK_]); \
    } while (0)
#define MFMA_RANGE(A_, B_, LO_, HI_)                                                                      \
    do {                                                                                                  \
        _Pragma("unroll") for (int ij = LO_; ij < HI_; ++ij)                                              \
            acc[ij / TN][ij % TN] = MDPT_MFMA_32x32x16(A_[ij / TN], B_[ij % TN], acc[ij / TN][ij % TN], 0, 0, 0); \
    } while (0)
        // Fragment reads are double-buffered in registers and the issue order is pinned (hipcc would otherwise sink
        // every ds_read next to its MFMA: read; wait; mfma). hipcc's waits are always lgkmcnt(0), so the order is
        // chosen such that each wait sits a full MFMA block after the newest outstanding read:
        //   L0 L1 | M0 | L2 | M1 | M2[first] | L3 | M2[rest] | M3
        bool f8tile = false;
#if MDPT_HAVE_F8
        if constexpr (F8C) f8tile = t < T8;  // (wave-uniform) an fp8 K tile: L0 L1 | M(k-steps 0, 1) | L2 L3 | M(k-steps 2, 3)
        if constexpr (F8C) if (f8tile) {
            const int ws = t < T8a ? wsc : wsc_lo;
#define MFMA_F8_ALL(A0_, A1_, B0_, B1_)                                                                   \
    do {                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                  \
            f8_mfma32_a_first<0>(acc[i][0], f8_cat(A0_[i], A1_[i]), f8_cat(B0_[0], B1_[0]), F8_A_SCALE, ws);   \
            if constexpr (TN > 1) f8_mfma32_a_first<1>(acc[i][1 % TN], f8_cat(A0_[i], A1_[i]), f8_cat(B0_[1 % TN], B1_[1 % TN]), F8_A_SCALE, ws); \
            if constexpr (TN > 2) f8_mfma32_a_first<2>(acc[i][2 % TN], f8_cat(A0_[i], A1_[i]), f8_cat(B0_[2 % TN], B1_[2 % TN]), F8_A_SCALE, ws); \
            if constexpr (TN > 3) f8_mfma32_a_first<3>(acc[i][3 % TN], f8_cat(A0_[i], A1_[i]), f8_cat(B0_[3 % TN], B1_[3 % TN]), F8_A_SCALE, ws); \
        }                                                                                                 \
    } while (0)
            // All four k-steps' fragments are read into their OWN registers before the first MFMA: a 32x32x64 f8f6f4 MFMA holds 8 + 8 source VGPRs
            // per lane and runs 16 passes - with the fp16 path's pattern (reload a source register right behind the MFMA that read it) the head
            // stage showed rare wrong elements against the CPU emulation (max error 40x its mean; tools/probes/gpu_f8_lockstep_pattern.py), which the
            // halo-staged kernels (other registers reloaded, a barrier in between) never did. hipcc waits for the reads by itself (builtin MFMA).
            opx8 a2[TM], b2[TN], a3[TM], b3[TN];
            LOAD_FRAGS(a0, b0, 0);
            LOAD_FRAGS(a1, b1, 1);
            LOAD_FRAGS(a2, b2, 2);
            LOAD_FRAGS(a3, b3, 3);
            PIN();
            MFMA_F8_ALL(a0, a1, b0, b1);
            PIN();
            MFMA_F8_ALL(a2, a3, b2, b3);
            PIN();
            // hipcc (ROCm 7.2) under-counts the wait states between a 32x32x64 f8f6f4 MFMA on fp8 operands (16 passes) and a NON-MFMA reader of its
            // result: where it moved the accumulators between register sets behind the tile (v_accvgpr_mov a31, a15 after `s_nop 8`), the last
            // accumulator register - rows 27 / 31 of every 32x32 block - was copied before the second MFMA had written it. Found by
            // tools/probes/gpu_f8_h1_check.py: (block 0, tap 0, channels 64-127) missing for exactly those rows. Settle by hand behind every fp8 tile.
            f8_mfma_settle();
            PIN();
#undef MFMA_F8_ALL
        }
#endif
        if (!f8tile) {
        LOAD_FRAGS(a0, b0, 0);
        LOAD_FRAGS(a1, b1, 1);
        PIN();
        MFMA_RANGE(a0, b0, 0, TM * TN);
        PIN();
        if (KSTEPS == 4) {
            LOAD_FRAGS(a0, b0, 2);
            PIN();
        }
        MFMA_RANGE(a1, b1, 0, TM * TN);
        PIN();
        if (KSTEPS == 4) {
            MFMA_RANGE(a0, b0, 0, 1);
            PIN();
            LOAD_FRAGS(a1, b1, 3);
            PIN();
            MFMA_RANGE(a0, b0, 1, TM * TN);
            PIN();
            MFMA_RANGE(a1, b1, 0, TM * TN);
            PIN();
        }
        }
#undef LOAD_FRAGS
#undef MFMA_RANGE
        rd = rd + 1 == NST ? 0 : rd + 1;
        wr = wr + 1 == NST ? 0 : wr + 1;
    }
    if (p.dbg_times) t_loop = memtime_now();
    __syncthreads();  // every wave is done reading the ring: reuse it as epilogue staging
    if (KSPLIT && p.ksplit > 1 && p.ks_all) run_epilogue_partial<WTN, TM, TN>(p, acc, smem, wave, lane, m0 + wm * WTM, n0 + wn * WTN, p.ks_part + (size_t)kz * p.M * p.ldc);
    else if (KSPLIT && kz > 0) run_epilogue_partial<WTN, TM, TN>(p, acc, smem, wave, lane, m0 + wm * WTM, n0 + wn * WTN, p.ks_part + (size_t)(kz - 1) * p.M * p.ldc);
    else run_epilogue<WTN, TM, TN, EKIND>(p, acc, smem, wave, lane, m0 + wm * WTM, n0 + wn * WTN);
    if (p.dbg_times && tid == 0) {
        // (written out, not stamp_record(.., 4): through the shared writer the register allocation of gemm_kernel<64, 64, 2, 2, 64, 2, 1, 0, 3, f8> changes)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned long long* d = p.dbg_times + (size_t)blockIdx.x * 6;
        d[0] = t_start; d[1] = t_first; d[2] = t_loop; d[3] = memtime_now();
        d[4] = __builtin_amdgcn_s_getreg(20 << 0 | 0 << 6 | 3 << 11);  // HW_REG_XCC_ID bits [3:0]
        d[5] = __builtin_amdgcn_s_getreg(4 << 0 | 0 << 6 | 31 << 11);  // HW_REG_HW_ID
    }
}
