// Bilinear interpolation (align_corners=True: SpatialUpsampleLayer, v2_depthanything/components/misc_helpers.py:39-42) of EIGHT channels of a
// bf16 NHWC map from its four source pixels, result rounded to bf16. ONE definition of the arithmetic for every kernel that upsamples
// the bf16 output of the last fusion projection in front of the head's first conv (fusion_model.py:182 -> head_model.py:74-76): the
// halo-staged conv kernel that interpolates its input patch in LDS (conv3h.hip, big launches) and the stand-alone upsample kernel
// (elementwise.hip, small launches) must produce the same bits - one image's result may not depend on the batch it is part of.
//   out = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)      in fp32, no contraction
#pragma once

typedef __attribute__((ext_vector_type(4))) unsigned mdpt_u32x4;

__device__ __forceinline__ mdpt_u32x4 mdpt_up_bf16x8(mdpt_u32x4 v00, mdpt_u32x4 v01, mdpt_u32x4 v10, mdpt_u32x4 v11, float lx, float ly) {
#pragma clang fp contract(off)
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    const float wx0 = 1.0f - lx, wy0 = 1.0f - ly;
    mdpt_u32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned d00 = v00[w], d01 = v01[w], d10 = v10[w], d11 = v11[w];  // (scalar copies: bit_cast on a vector ELEMENT expression reads element 0)
        const f32x2_t a00 = op2_to_f32(d00);
        const f32x2_t a01 = op2_to_f32(d01);
        const f32x2_t a10 = op2_to_f32(d10);
        const f32x2_t a11 = op2_to_f32(d11);
        const f32x2_t r = wy0 * (wx0 * a00 + lx * a01) + ly * (wx0 * a10 + lx * a11);
        out[w] = __builtin_bit_cast(unsigned, to_op2(r));
    }
    return out;
}

// Source patch of a 16x16 output tile at (oy0, ox0) of an align_corners upsample (scales sy, sx = (source - 1) / (output - 1)): the source
// pixels that the tile's output rows oy0 - halo .. oy0 + 15 + halo (clipped to the map; columns alike) interpolate from - first row /
// column and extent. halo = 1: the tile with the one-pixel border a 3x3 conv reads; halo = 0: the tile itself.
struct mdpt_up_patch_t {
    int py0, px0, ph, pw;
};
__device__ __forceinline__ mdpt_up_patch_t mdpt_up_patch(float sy, float sx, int oy0, int ox0, int halo, int Ho, int Wo, int Hs, int Ws) {
    mdpt_up_patch_t g;
    const int oy_first = oy0 == 0 ? 0 : oy0 - halo, ox_first = ox0 == 0 ? 0 : ox0 - halo;
    const int oy_last = min(oy0 + 15 + halo, Ho - 1), ox_last = min(ox0 + 15 + halo, Wo - 1);
    g.py0 = (int)(sy * (float)oy_first); g.px0 = (int)(sx * (float)ox_first);
    g.ph = min((int)(sy * (float)oy_last) + 1, Hs - 1) - g.py0 + 1;
    g.pw = min((int)(sx * (float)ox_last) + 1, Ws - 1) - g.px0 + 1;
    return g;
}
