// ---- hole filling of rendered views: hierarchical (push-pull) filling with a preference for the far side, for the pixels render_resolve_kernel
// leaves as background - the disocclusions behind depth edges and everything outside the photo's frustum (not in the reference, whose viewer shows
// the holes). Level 0 is the image (a pixel is valid iff alpha != 0 and 0 < depth < inf), level l + 1 halves level l rounding up, to the 1 x 1 level
// L; a node = {three colour channels, depth} fp32, depth 0 = invalid (FillPlan of mdpt_kernels.h). Push and pull share one selection rule: of up to
// four contributors those with (double)d >= (1 - band) x (double)dmax are kept, dmax the largest valid depth among them. Push: the mean of the kept
// children (2Y + dy, 2X + dx) in the order (0,0) (0,1) (1,0) (1,1). Pull, top down, for invalid nodes only: the kept ones of the four nearest
// parents, weights 9/16 3/16 3/16 1/16, normalised by the kept weights. Sums and the one division in fp64 in that order, rounded once to fp32 (at
// level 0: colour floor(v + 0.5) clamped, alpha 255): tests/fill_restate.py restates it in numpy, and nothing here depends on how levels are grouped
// into launches. The launches: (1) fill_push_kernel, one per FILL_PUSH_LEVELS levels below the top: a workgroup owns an aligned 32 x 32 block of its
// base level and makes the 16 x 16, 8 x 8 and 4 x 4 nodes above it through LDS; (2) fill_top_kernel: one workgroup per image holds every level of at
// most 32 x 32 nodes in LDS, finishes the push and starts the pull; (3) fill_pull_kernel, one per level below the top; the last writes the outputs.
// No atomics, no workgroup waits on another, every scratch node that is read was written by this call.

namespace {

__device__ __forceinline__ float4 fill_pixel(uchar4 c, float d) {
    if (c.w == 0 || !(d > 0.0f && d < INFINITY)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4((float)c.x, (float)c.y, (float)c.z, d);
}

// the selection rule and the weighted mean of the kept contributors -> false: none is valid
__device__ __forceinline__ bool fill_mix(const float4 (&v)[4], const double (&wt)[4], double keep, double (&o)[4]) {
#pragma clang fp contract(off)
    float dmax = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) dmax = fmaxf(dmax, v[k].w);
    if (!(dmax > 0.0f)) return false;
    const double thr = keep * (double)dmax;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, sw = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k].w > 0.0f && (double)v[k].w >= thr) {
            s0 = s0 + wt[k] * (double)v[k].x, s1 = s1 + wt[k] * (double)v[k].y, s2 = s2 + wt[k] * (double)v[k].z, s3 = s3 + wt[k] * (double)v[k].w;
            sw = sw + wt[k];
        }
    o[0] = s0 / sw, o[1] = s1 / sw, o[2] = s2 / sw, o[3] = s3 / sw;
    return true;
}

// push: the node above the four children (a child that does not exist is passed as invalid)
__device__ __forceinline__ float4 fill_push_node(const float4 (&v)[4], double keep) {
    const double ones[4] = {1.0, 1.0, 1.0, 1.0};  // (1 x v and the count are exact: the mean of the kept children)
    double o[4];
    if (!fill_mix(v, ones, keep, o)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
}

// pull: node (y, x) of a level from its parents' level of hp x wp nodes
__device__ __forceinline__ bool fill_pull_node(const float4* __restrict__ parents, int hp, int wp, int y, int x, double keep, double (&o)[4]) {
    const double wt[4] = {0.5625, 0.1875, 0.1875, 0.0625};
    const int ya = y >> 1, xa = x >> 1;
    const int yb = min(max(ya + ((y & 1) ? 1 : -1), 0), hp - 1), xb = min(max(xa + ((x & 1) ? 1 : -1), 0), wp - 1);
    const float4 v[4] = {parents[(size_t)ya * wp + xa], parents[(size_t)ya * wp + xb], parents[(size_t)yb * wp + xa], parents[(size_t)yb * wp + xb]};
    return fill_mix(v, wt, keep, o);
}

__device__ __forceinline__ float fill_byte(double v) { return (float)fmin(fmax(floor(v + 0.5), 0.0), 255.0); }

__device__ __forceinline__ float4* fill_image_nodes(const FillJob& j, int n) { return (float4*)j.scratch + (size_t)n * j.plan.off[j.plan.L + 1]; }

// blockIdx.y = image, blockIdx.x = the 32 x 32 block of level `base`; levels = 1 .. FILL_PUSH_LEVELS levels to make above it
template <bool FROM_INPUT>
__global__ __launch_bounds__(256) void fill_push_kernel(const FillJob j, int base, int levels) {
    __shared__ float4 tile[16 * 16 + 8 * 8];
    const FillPlan& p = j.plan;
    const int n = blockIdx.y;
    const int hb = fill_level_side(p.H, base), wb = fill_level_side(p.W, base);
    const int across = (wb + 31) / 32, by = (int)blockIdx.x / across, bx = (int)blockIdx.x % across;
    float4* img = fill_image_nodes(j, n);
    const float4* below = img + p.off[base];  // (base >= 1)
    {
        const int h1 = fill_level_side(p.H, base + 1), w1 = fill_level_side(p.W, base + 1);
        const int Y = by * 16 + ((int)threadIdx.x >> 4), X = bx * 16 + ((int)threadIdx.x & 15);
        float4 node = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (Y < h1 && X < w1) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cy = 2 * Y + (k >> 1), cx = 2 * X + (k & 1);
                v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (cy < hb && cx < wb) {
                    const size_t c = (size_t)cy * wb + cx;
                    if (FROM_INPUT) {
                        const size_t at = (size_t)n * p.H * p.W + c;
                        v[k] = fill_pixel(((const uchar4*)j.color)[at], j.depth[at]);
                    } else {
                        v[k] = below[c];
                    }
                }
            }
            node = fill_push_node(v, j.keep);
            img[p.off[base + 1] + (size_t)Y * w1 + X] = node;
        }
        tile[threadIdx.x] = node;  // (a node outside the level is invalid: the levels above need no test of their own)
    }
    float4* src = tile;
    float4* dst = tile + 256;
    for (int s = 2, side = 16; s <= levels; ++s, side >>= 1) {
        __syncthreads();
        const int half = side >> 1;  // this level's share of the block: 8 x 8, then 4 x 4
        if ((int)threadIdx.x < half * half) {
            const int hs = fill_level_side(p.H, base + s), ws = fill_level_side(p.W, base + s);
            const int ty = (int)threadIdx.x / half, tx = (int)threadIdx.x % half, Y = by * half + ty, X = bx * half + tx;
            float4 node = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (Y < hs && X < ws) {
                const float4 v[4] = {src[(2 * ty) * side + 2 * tx], src[(2 * ty) * side + 2 * tx + 1], src[(2 * ty + 1) * side + 2 * tx],
                                     src[(2 * ty + 1) * side + 2 * tx + 1]};
                node = fill_push_node(v, j.keep);
                img[p.off[base + s] + (size_t)Y * ws + X] = node;
            }
            dst[threadIdx.x] = node;
        }
        float4* t = src;
        src = dst, dst = t;
    }
}

#define FILL_TOP_NODES (1024 + 256 + 64 + 16 + 4 + 1)

// blockIdx.x = image: the levels top .. L in LDS, pushed up and pulled down; top == 0 (an image of at most 32 x 32 pixels): the whole call
__global__ __launch_bounds__(256) void fill_top_kernel(const FillJob j) {
    __shared__ float4 lds[FILL_TOP_NODES];
    const FillPlan& p = j.plan;
    const int n = blockIdx.x, top = p.top;
    const size_t hw = (size_t)p.H * p.W;
    float4* img = fill_image_nodes(j, n);
    const uchar4* color = (const uchar4*)j.color + (size_t)n * hw;
    const float* depth = j.depth + (size_t)n * hw;
    // level l's first node in LDS: the scratch's order, from level top on (top == 0: the image, then the scratch's levels)
    auto at = [&](int l) { return top ? (int)(p.off[l] - p.off[top]) : (l ? (int)(hw + p.off[l]) : 0); };
    const int n_top = fill_level_side(p.H, top) * fill_level_side(p.W, top), n_all = at(p.L) + 1;
    for (int i = threadIdx.x; i < n_top; i += 256) lds[i] = top ? img[p.off[top] + i] : fill_pixel(color[i], depth[i]);
    for (int l = top; l < p.L; ++l) {
        __syncthreads();
        const int h = fill_level_side(p.H, l), w = fill_level_side(p.W, l), h1 = fill_level_side(p.H, l + 1), w1 = fill_level_side(p.W, l + 1);
        const float4* src = lds + at(l);
        float4* dst = lds + at(l + 1);
        for (int i = threadIdx.x; i < h1 * w1; i += 256) {
            const int Y = i / w1, X = i % w1;
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cy = 2 * Y + (k >> 1), cx = 2 * X + (k & 1);
                v[k] = cy < h && cx < w ? src[cy * w + cx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            dst[i] = fill_push_node(v, j.keep);
        }
    }
    for (int l = p.L - 1; l >= top; --l) {
        __syncthreads();
        const int h = fill_level_side(p.H, l), w = fill_level_side(p.W, l), h1 = fill_level_side(p.H, l + 1), w1 = fill_level_side(p.W, l + 1);
        float4* own = lds + at(l);
        const float4* parents = lds + at(l + 1);
        for (int i = threadIdx.x; i < h * w; i += 256) {
            if (own[i].w > 0.0f) continue;
            double o[4];
            if (!fill_pull_node(parents, h1, w1, i / w, i % w, j.keep, o)) continue;
            own[i] = l ? make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3])
                       : make_float4(fill_byte(o[0]), fill_byte(o[1]), fill_byte(o[2]), (float)o[3]);
        }
    }
    __syncthreads();
    if (top) {
        for (int i = threadIdx.x; i < n_all; i += 256) img[p.off[top] + i] = lds[i];
        return;
    }
    uchar4* out = (uchar4*)j.out + (size_t)n * hw;
    for (int i = threadIdx.x; i < n_top; i += 256) {
        const uchar4 c = color[i];
        const float d = depth[i];
        const bool valid = fill_pixel(c, d).w > 0.0f, filled = lds[i].w > 0.0f;
        const float4 f = lds[i];
        out[i] = valid ? c : (filled ? make_uchar4((unsigned char)f.x, (unsigned char)f.y, (unsigned char)f.z, 255) : make_uchar4(0, 0, 0, 0));
        if (j.out_depth) j.out_depth[(size_t)n * hw + i] = valid ? d : (filled ? f.w : INFINITY);
    }
}

// blockIdx.y = image, one thread per node of level l (below the top): an invalid node takes its value from level l + 1, in place; OUT: l == 0,
// the outputs: valid pixels copied as they are, the others filled, or background where nothing above them is valid (an image without a valid pixel)
template <bool OUT>
__global__ __launch_bounds__(256) void fill_pull_kernel(const FillJob j, int l) {
    const FillPlan& p = j.plan;
    const int n = blockIdx.y;
    const int h = fill_level_side(p.H, l), w = fill_level_side(p.W, l), h1 = fill_level_side(p.H, l + 1), w1 = fill_level_side(p.W, l + 1);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h * w) return;
    float4* img = fill_image_nodes(j, n);
    const float4* parents = img + p.off[l + 1];
    const int y = (int)(i / (size_t)w), x = (int)(i % (size_t)w);
    double o[4];
    if (OUT) {
        const size_t at = (size_t)n * h * w + i;
        uchar4 c = ((const uchar4*)j.color)[at];
        float d = j.depth[at];
        if (!(fill_pixel(c, d).w > 0.0f)) {
            c = make_uchar4(0, 0, 0, 0), d = INFINITY;
            if (fill_pull_node(parents, h1, w1, y, x, j.keep, o))
                c = make_uchar4((unsigned char)fill_byte(o[0]), (unsigned char)fill_byte(o[1]), (unsigned char)fill_byte(o[2]), 255), d = (float)o[3];
        }
        ((uchar4*)j.out)[at] = c;
        if (j.out_depth) j.out_depth[at] = d;
    } else {
        float4* own = img + p.off[l];
        if (own[i].w > 0.0f) return;
        if (fill_pull_node(parents, h1, w1, y, x, j.keep, o)) own[i] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
    }
}

}  // namespace

int mdpt_launch_post_fill(const FillJob& j, hipStream_t stream) {
    const FillPlan& p = j.plan;
    if (j.N <= 0 || j.N > 65535 || p.H <= 0 || p.W <= 0 || p.H > RENDER_MAX_SIDE || p.W > RENDER_MAX_SIDE || !(j.keep >= 0.0 && j.keep <= 1.0) ||
        p.top < 0 || p.top > p.L || p.L >= FILL_MAX_LEVELS)
        return (int)hipErrorInvalidValue;
    for (int base = 0; base < p.top; base += FILL_PUSH_LEVELS) {
        const int levels = p.top - base < FILL_PUSH_LEVELS ? p.top - base : FILL_PUSH_LEVELS;
        const size_t blocks = (((size_t)fill_level_side(p.H, base) + 31) / 32) * (((size_t)fill_level_side(p.W, base) + 31) / 32);
        if (base)
            post_launch("fill_push_kernel<0>", fill_push_kernel<false>, dim3((unsigned)blocks, j.N), dim3(256), stream, j, base, levels);
        else
            post_launch("fill_push_kernel<1>", fill_push_kernel<true>, dim3((unsigned)blocks, j.N), dim3(256), stream, j, base, levels);
    }
    post_launch("fill_top_kernel", fill_top_kernel, dim3(j.N), dim3(256), stream, j);
    for (int l = p.top - 1; l >= 0; --l) {
        const size_t blocks = ((size_t)fill_level_side(p.H, l) * fill_level_side(p.W, l) + 255) / 256;
        if (l)
            post_launch("fill_pull_kernel<0>", fill_pull_kernel<false>, dim3((unsigned)blocks, j.N), dim3(256), stream, j, l);
        else
            post_launch("fill_pull_kernel<1>", fill_pull_kernel<true>, dim3((unsigned)blocks, j.N), dim3(256), stream, j, l);
    }
    return (int)hipGetLastError();
}
