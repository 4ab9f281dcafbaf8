// What more than one file of the HBM-bound helper kernels uses (elementwise.hip includes this file first, swin.hip takes it too): the operand
// plane stores and loads, the wave sum, the grid size of a grid-stride launch, the launch helper and the LayerNorm row-width dispatch.

#include <type_traits>
#include "mdpt_kernels.h"
#include "mdpt_prof.h"
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

// one element at a time (the stage-level entry points and the BEiT tap path: not hot). lo_f8 != 0: lo is the e5m2 residue plane of an F8
// consumer (bytes, + the a8 plane lo_f8 bytes behind it if lo_a8; f8_cross.h)
__device__ __forceinline__ void plane_store1(op_t* hi, op_t* lo, size_t idx, float v, size_t lo_f8, int lo_a8) {
    const op_t h = to_op(v);
    hi[idx] = h;
#if MDPT_HAVE_F8
    if (lo && lo_f8) {
        unsigned char* b8 = (unsigned char*)lo;
        b8[idx] = (unsigned char)(f8_pk_e5m2((v - (float)h) * F8_LO_SCALE, 0.0f, 0u, false) & 0xFF);
        if (lo_a8) b8[lo_f8 + idx] = (unsigned char)(f8_pk_e5m2((float)h, 0.0f, 0u, false) & 0xFF);
        return;
    }
#endif
    if (lo) lo[idx] = to_op(v - (float)h);
}

// ... and back: hi (+ lo); lo_f8 != 0: value = hi + e5m2(byte) * 2^-F8_LO_SHIFT (an e5m2 byte is the top byte of an fp16)
__device__ __forceinline__ float plane_load1(const op_t* hi, const op_t* lo, size_t idx, size_t lo_f8) {
    if (lo && lo_f8) {
        const unsigned short b16 = (unsigned short)(((const unsigned char*)lo)[idx] << 8);
        return (float)hi[idx] + (float)__builtin_bit_cast(_Float16, b16) * (1.0f / F8_LO_SCALE);
    }
    float v = (float)hi[idx];
    if (lo) v += (float)lo[idx];
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// workgroups of 256 threads for a grid-stride loop over `total` items, at most `cap`
inline int grid_for(size_t total, int cap = 16384) {
    size_t g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

// one launch, returning hipError_t as int (the arguments convert to the kernel's parameter types) ...
template <typename... Params, typename... Args>
inline int ew_launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<Params>(args)...);
    return (int)hipGetLastError();
}
// ... and under its profiler label (the scope closes after the launch)
template <typename... Params, typename... Args>
inline int ew_launch(const char* label, double flops, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args&&... args) {
    MdptProfScope prof(label, flops, stream);
    return ew_launch(kernel, grid, block, lds, stream, static_cast<Args&&>(args)...);
}

// the one-wave-per-row LayerNorm kernels hold a row of F floats as NV float4 per lane (F <= 256 NV): launch(std::integral_constant<int, NV>)
template <typename Launch>
inline int ln_dispatch(int F, Launch&& launch) {
    if (F <= 256) return launch(std::integral_constant<int, 1>{});
    if (F <= 512) return launch(std::integral_constant<int, 2>{});
    if (F <= 1024) return launch(std::integral_constant<int, 4>{});
    if (F <= 1536) return launch(std::integral_constant<int, 6>{});
    return launch(std::integral_constant<int, 8>{});
}

}  // namespace
