// What the MFMA kernel files share (gemm.hip, conv3h.hip, attention.hip, head.hip; textually included first inside the file's anonymous
// namespace): the vector types, the LDS-DMA / buffer-descriptor / clock helpers, the schedule macros of the hand-scheduled main loops, the
// XCD-contiguous block -> tile map and the writer of the per-workgroup debug stamp record. No floating-point arithmetic lives here: the
// file takes no side in the including file's fp-contract mode.

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// 64 lanes x 16 B -> lds_wave_base + lane*16 (LDS-DMA: the destination is wave-uniform base + lane*16, no register round trip)
__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ unsigned long long memtime_now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// raw buffer descriptor over `bytes` bytes at `base` (a lane offset at or beyond the size reads zeros / drops the store)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(unsigned)(bytes < 0xFFFFFFF0ull ? bytes : 0xFFFFFFF0ull), 0x00020000);
}

// schedule macros of the hand-scheduled loops: PIN = nothing moves across this point, BAR = a pinned workgroup barrier, counted waits
// (WAIT_LGKM / WAIT_VM take a literal, WAIT_VM_IMM any integral constant expression)
#define PIN() __builtin_amdgcn_sched_barrier(0)
#define BAR() do { PIN(); __builtin_amdgcn_s_barrier(); PIN(); } while (0)
#define WAIT_LGKM(N_) asm volatile("s_waitcnt lgkmcnt(" #N_ ")" ::: "memory")
#define WAIT_VM(N_) asm volatile("s_waitcnt vmcnt(" #N_ ")" ::: "memory")
#define WAIT_VM_IMM(N_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory")

// XCD-contiguous tile of this workgroup (bijective for any grid size): the dispatcher places block b on XCD b % 8; every XCD gets a
// contiguous run of tiles, so what neighbouring tiles share (operand panels, halo rows / columns) stays in that XCD's L2.
__device__ __forceinline__ int xcd_tile() {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7;
    return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
}

// The six-slot debug stamp record of this workgroup (GemmParams / Conv3hParams::dbg_times; layouts: mdpt_kernels.h), written by one thread
// once its stores are acknowledged: [start, first barrier, loop done, stores acknowledged, slot 4, slot 5]. `xcc_slot` (a constant at
// every call site) says which slot receives HW_REG_XCC_ID:
//     4: [.., XCC id, HW_REG_HW_ID]     5: [.., t_issued, XCC id]     STAMP_HW_ID: [.., t_issued, HW_REG_HW_ID]
//     STAMP_NO_ID: [.., stores acknowledged again, 0]
constexpr int STAMP_HW_ID = -1, STAMP_NO_ID = -2;
__device__ __forceinline__ void stamp_record(unsigned long long* dbg_times, unsigned long long t_start, unsigned long long t_first, unsigned long long t_loop,
                                             int xcc_slot, unsigned long long t_issued = 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long* d = dbg_times + (size_t)blockIdx.x * 6;
    d[0] = t_start; d[1] = t_first; d[2] = t_loop; d[3] = memtime_now();
    if (xcc_slot == STAMP_NO_ID) { d[4] = d[3]; d[5] = 0; return; }
    d[4] = xcc_slot == 4 ? __builtin_amdgcn_s_getreg(20 << 0 | 0 << 6 | 3 << 11) : t_issued;  // HW_REG_XCC_ID bits [3:0]
    d[5] = xcc_slot == 5 ? __builtin_amdgcn_s_getreg(20 << 0 | 0 << 6 | 3 << 11) : __builtin_amdgcn_s_getreg(4 << 0 | 0 << 6 | 31 << 11);  // ... or HW_REG_HW_ID
}
