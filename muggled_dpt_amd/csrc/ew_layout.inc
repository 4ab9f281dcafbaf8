// ---- layout conversion NCHW fp32 <-> NHWC fp32 / operand planes (stage-level API and debug taps; not on the fused forward path)

namespace {

__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* in_f32, const op_t* in_hi, const op_t* in_lo,
                                                           float* __restrict__ out, int B, int H, int W, int C, int Cp) {
    const size_t total = (size_t)B * C * H * W;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int c = (int)((idx / ((size_t)W * H)) % C);
        const int b = (int)(idx / ((size_t)W * H * C));
        const size_t o = (((size_t)b * H + y) * W + x) * Cp + c;
        out[idx] = in_f32 ? in_f32[o] : plane_load1(in_hi, in_lo, o, 0);
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
            plane_store1(out_hi, out_lo, idx, v, out_f8, out_a8);
        }
    }
}

}  // namespace

int MDPT_FN(mdpt_launch_nhwc_to_nchw)(const float* in_f32, const op_t* in_hi, const op_t* in_lo, float* out, int B, int H, int W, int C,
                             int Cp, hipStream_t stream) {
    return ew_launch(nhwc_to_nchw_kernel, dim3(grid_for((size_t)B * C * H * W)), dim3(256), 0, stream, in_f32, in_hi, in_lo, out, B, H, W, C, Cp);
}

int MDPT_FN(mdpt_launch_nchw_to_nhwc)(const float* in, float* out_f32, op_t* out_hi, op_t* out_lo, int relu_bf16, int B, int H, int W,
                             int C, int Cp, hipStream_t stream, size_t out_f8, int out_a8) {
    return ew_launch(nchw_to_nhwc_kernel, dim3(grid_for((size_t)B * H * W * Cp)), dim3(256), 0, stream, in, out_f32, out_hi, out_lo, relu_bf16, B, H, W, C, Cp, out_f8, out_a8);
}
