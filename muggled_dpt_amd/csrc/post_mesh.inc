// ---- depth-to-mesh: the client half of the reference's 3D viewer ("Save 3D Model"), which is JavaScript on the CPU there - 3dviewer/shaders.js:163-264
// run_vertex_shader_cpu (the unprojection of every plane vertex through a bilinear sample of the 24-bit depth + alpha frame), mesh.js:170-254
// _make_plane_mesh (the grid and its two triangles per cell) and mesh.js:330-371 filter_mesh_vertices (drop the vertices below the edge threshold
// and every face that touches one, keep the order, renumber). Positions, weights, the alpha comparison and the depth arithmetic are fp64 as in
// JavaScript, nothing contracted, rounded to fp32 once on output. One deviation: the 24-bit depth value is interpolated, where the JavaScript
// interpolates its three bytes separately and truncates each (garbage across a byte carry).
//
// The compaction is an order-preserving multi-launch scan, bit-deterministic: (1) alpha -> a keep flag per vertex and the kept count of every
// 256-vertex block, (2) the kept faces of every 256-cell block from the flags, (3) ONE workgroup per image and list scans the block counts in
// 256-wide chunks with a running carry (no workgroup ever waits for another), (4) the kept vertices are computed and written at block offset +
// rank in block (64-bit ballots and popcounts, wave totals through LDS) and the flag plane becomes the old -> new index map, (5) the kept faces are
// written through that map. A launch boundary separates every producer from its consumers.
//
// R is the type of the arithmetic: double. A -DMDPT_DEBUG_SWITCHES build also holds the float instances, chosen by MDPT_MESH_FP32=1, so that
// tools/probes/gpu_mesh.py can time what the fp64 costs; they do not meet the fp64 specification and no release build has them.

namespace {

template <typename R>
__device__ __forceinline__ void mesh_vertex_xy(const MeshJob& m, size_t i, R& x, R& y) {
#pragma clang fp contract(off)
    if (m.vertex_xy) {
        x = (R)m.vertex_xy[2 * i];
        y = (R)m.vertex_xy[2 * i + 1];
        return;
    }
    const int r = (int)(i / (size_t)m.nx), c = (int)(i - (size_t)r * m.nx);  // mesh.js:198-200
    x = (R)c * (R)m.x_step - (R)1;
    y = (R)1 - (R)r * (R)m.y_step;
}

// shaders.js:212-252 in the viewer's vertically flipped frame (index.html:1067-1070: flipped row j = frame row H - 1 - j): the four taps as pixel
// indices of one frame and the two weights. A coordinate that is not a number clamps to 1 (fmin(1, NaN) = 1), so such a position samples the last
// column / row of the flipped frame with weight 0 on the neighbour; nothing leaves the frame.
template <typename R>
struct MeshTaps { size_t tl, tr, bl, br; R tx, ty; };

template <typename R>
__device__ __forceinline__ MeshTaps<R> mesh_taps(R x, R y, int H, int W) {
#pragma clang fp contract(off)
    const R u = (x + (R)1) * (R)0.5, v = (y + (R)1) * (R)0.5;
    const R xr = fmax((R)0, fmin((R)1, u)) * (R)(W - 1), yr = fmax((R)0, fmin((R)1, v)) * (R)(H - 1);
    const int x1 = (int)floor(xr), y1 = (int)floor(yr);
    const int x2 = x1 + 1 < W - 1 ? x1 + 1 : W - 1, y2 = y1 + 1 < H - 1 ? y1 + 1 : H - 1;
    const size_t top = (size_t)(H - 1 - y1) * W, bot = (size_t)(H - 1 - y2) * W;
    return MeshTaps<R>{top + x1, top + x2, bot + x1, bot + x2, xr - (R)x1, yr - (R)y1};
}

template <typename R>
__device__ __forceinline__ R mesh_lerp(const MeshTaps<R>& t, R tl, R tr, R bl, R br) {
#pragma clang fp contract(off)
    const R l = ((R)1 - t.ty) * tl + t.ty * bl, r = ((R)1 - t.ty) * tr + t.ty * br;  // shaders.js:232-234
    return ((R)1 - t.tx) * l + t.tx * r;
}

// (1) shaders.js:198: a vertex is kept if its interpolated alpha byte reaches edge_threshold * 255
template <typename R>
__global__ __launch_bounds__(256) void mesh_flag_kernel(const MeshJob m) {
    const int b = blockIdx.y;
    const size_t nv = (size_t)m.nx * m.ny, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < nv) {
        R x, y;
        mesh_vertex_xy(m, i, x, y);
        const MeshTaps<R> t = mesh_taps(x, y, m.H, m.W);
        const unsigned* f = m.frames + (size_t)b * m.H * m.W;
        keep = mesh_lerp(t, (R)(f[t.tl] >> 24), (R)(f[t.tr] >> 24), (R)(f[t.bl] >> 24), (R)(f[t.br] >> 24)) >= (R)m.alpha_min;
        m.vmap[(size_t)b * nv + i] = keep ? 0 : -1;
    }
    unsigned total;
    block_rank(keep ? 1 : 0, total);
    if (threadIdx.x == 0) m.vcnt[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// mesh.js:218-228 for grid cell k of image b: the map entries of its corners {v, v + 1, v + nx, v + nx + 1} and which of its two triangles
// [v, v + nx, v + nx + 1], [v, v + nx + 1, v + 1] have all their vertices kept (bit 0, bit 1)
__device__ __forceinline__ int mesh_cell(const MeshJob& m, int b, size_t k, int (&e)[4]) {
    const size_t cols = (size_t)m.nx - 1, r = k / cols, c = k - r * cols;
    const int* v = m.vmap + (size_t)b * m.nx * m.ny + c + r * m.nx;
    e[0] = v[0];
    e[1] = v[1];
    e[2] = v[m.nx];
    e[3] = v[(size_t)m.nx + 1];
    const bool diag = e[0] >= 0 && e[3] >= 0;
    return (diag && e[2] >= 0 ? 1 : 0) | (diag && e[1] >= 0 ? 2 : 0);
}

// (2) the kept faces of every block of 256 cells
__global__ __launch_bounds__(256) void mesh_face_count_kernel(const MeshJob m) {
    const size_t cells = ((size_t)m.nx - 1) * ((size_t)m.ny - 1), k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int e[4];
    const int tri = k < cells ? mesh_cell(m, blockIdx.y, k, e) : 0;
    unsigned total;
    block_rank((tri & 1) + (tri >> 1), total);
    if (threadIdx.x == 0) m.fcnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// (3) block counts -> exclusive offsets in place and the image's total -> counts; blockIdx.x = the list (0 vertices, 1 faces), blockIdx.y = image.
// The vertex list's workgroup also resets the image's running bounds.
__global__ __launch_bounds__(256) void mesh_scan_kernel(const MeshJob m, unsigned nbv, unsigned nbf, int* __restrict__ counts) {
    const int b = blockIdx.y, which = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n = which ? nbf : nbv;
    unsigned* cnt = which ? m.fcnt + (size_t)b * nbf : m.vcnt + (size_t)b * nbv;
    __shared__ unsigned swave[4];
    unsigned carry = 0;
    for (unsigned base = 0; base < n; base += 256) {
        const unsigned i = base + threadIdx.x, v = i < n ? cnt[i] : 0;
        unsigned inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) swave[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += swave[w];
            total += swave[w];
        }
        if (i < n) cnt[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[2 * (size_t)b + which] = (int)carry;
        if (m.points) counts[2 * (size_t)b + 1] = (int)carry;  // one "face" [i] per kept vertex
    }
    if (which == 0 && threadIdx.x < 6) m.bord[6 * (size_t)b + threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

// (4) shaders.js:185-205 for the kept vertices, written at their new index; the flag plane becomes the old -> new map; the image's bounds
// (save_gltf.js:16-25, of the fp32 values as written: rounding is monotonic) through ordered-uint atomics, whose result does not depend on order
template <typename R>
__global__ __launch_bounds__(256) void mesh_vertex_kernel(const MeshJob m, float* __restrict__ xyz, float* __restrict__ uv) {
    const int b = blockIdx.y;
    const size_t nv = (size_t)m.nx * m.ny, i = (size_t)blockIdx.x * 256 + threadIdx.x, slab = (size_t)b * nv;
    const bool keep = i < nv && m.vmap[slab + i] >= 0;
    unsigned total;
    const unsigned rank = block_rank(keep ? 1 : 0, total);
    if (total == 0) return;  // (uniform over the block)
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (keep) {
#pragma clang fp contract(off)
        R x, y;
        mesh_vertex_xy(m, i, x, y);
        const MeshTaps<R> t = mesh_taps(x, y, m.H, m.W);
        const unsigned* f = m.frames + (size_t)b * m.H * m.W;
        const R s = (R)(1.0 / 16777216.0);
        const R d = mesh_lerp(t, (R)(f[t.tl] & 0xffffffu) * s, (R)(f[t.tr] & 0xffffffu) * s, (R)(f[t.bl] & 0xffffffu) * s,
                              (R)(f[t.br] & 0xffffffu) * s);
        const R lin = (R)m.a + (R)m.b * d, depth = m.is_metric ? lin : (R)1 / lin;  // shaders.js:178-180
        p[0] = (float)(depth * x * (R)m.x_scale * (R)m.tan_half_fov);
        p[1] = (float)(depth * y * (R)m.y_scale * (R)m.tan_half_fov);
        p[2] = (float)(-depth);
        const size_t nw = (size_t)m.vcnt[(size_t)b * gridDim.x + blockIdx.x] + rank, o = slab + nw;
        xyz[3 * o] = p[0];
        xyz[3 * o + 1] = p[1];
        xyz[3 * o + 2] = p[2];
        uv[2 * o] = (float)((x + (R)1) * (R)0.5);
        uv[2 * o + 1] = (float)((y + (R)1) * (R)0.5);
        m.vmap[slab + i] = (int)nw;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const BlockMinMax<float> r = block_minmax_reduce(keep ? p[k] : INFINITY, keep ? p[k] : -INFINITY, false, keep);
        if (threadIdx.x == 0) {  // (most blocks improve nothing: a device-scope load first keeps them off the six contended addresses)
            unsigned* lo = m.bord + 6 * (size_t)b + k;
            if (f2ord(r.lo) < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo, f2ord(r.lo));
            if (f2ord(r.hi) > __hip_atomic_load(lo + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(lo + 3, f2ord(r.hi));
        }
    }
}

// the image's bounds once its vertices are written (the first workgroup of the launch after): save_gltf.js:16-17's initial values when nothing
// was kept; its clamp of real values to +-1e6 is not reproduced
__device__ __forceinline__ void mesh_finish_bounds(const MeshJob& m, int b, const int* counts, float* bounds) {
    if (blockIdx.x == 0 && threadIdx.x < 6)
        bounds[6 * (size_t)b + threadIdx.x] = counts[2 * (size_t)b] > 0 ? ord2f(m.bord[6 * (size_t)b + threadIdx.x]) : (threadIdx.x < 3 ? 1e6f : -1e6f);
}

// (5) mesh.js:357-368: the kept faces in cell order, first then second triangle, with the new vertex indices
__global__ __launch_bounds__(256) void mesh_face_kernel(const MeshJob m, unsigned* __restrict__ faces, const int* __restrict__ counts,
                                                        float* __restrict__ bounds) {
    const int b = blockIdx.y;
    mesh_finish_bounds(m, b, counts, bounds);
    const size_t cells = ((size_t)m.nx - 1) * ((size_t)m.ny - 1), k = (size_t)blockIdx.x * 256 + threadIdx.x;
    int e[4];
    const int tri = k < cells ? mesh_cell(m, b, k, e) : 0;
    unsigned total;
    const unsigned rank = block_rank((tri & 1) + (tri >> 1), total);
    if (!tri) return;
    unsigned* o = faces + ((size_t)b * 2 * cells + m.fcnt[(size_t)b * gridDim.x + blockIdx.x] + rank) * 3;
    if (tri & 1) {
        o[0] = e[0];
        o[1] = e[2];
        o[2] = e[3];
        o += 3;
    }
    if (tri & 2) {
        o[0] = e[0];
        o[1] = e[3];
        o[2] = e[1];
    }
}

// (5, points) mesh.js:287-300: face [i] of every kept vertex, renumbered - the identity list of the kept count
__global__ __launch_bounds__(256) void mesh_point_kernel(const MeshJob m, unsigned* __restrict__ faces, const int* __restrict__ counts,
                                                         float* __restrict__ bounds) {
    const int b = blockIdx.y;
    mesh_finish_bounds(m, b, counts, bounds);
    const size_t nv = (size_t)m.nx * m.ny, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int nw = m.vmap[(size_t)b * nv + i];
    if (nw >= 0) faces[(size_t)b * nv + nw] = (unsigned)nw;
}

// the float instances exist in A/B builds alone
#ifdef MDPT_DEBUG_SWITCHES
void mesh_launch_flag_f32(const MeshJob& m, unsigned nbv, hipStream_t stream) {
    post_launch("mesh_flag_kernel<float>", mesh_flag_kernel<float>, dim3(nbv, m.B), dim3(256), stream, m);
}
void mesh_launch_vertex_f32(const MeshJob& m, unsigned nbv, float* xyz, float* uv, hipStream_t stream) {
    post_launch("mesh_vertex_kernel<float>", mesh_vertex_kernel<float>, dim3(nbv, m.B), dim3(256), stream, m, xyz, uv);
}
#else
void mesh_launch_flag_f32(const MeshJob&, unsigned, hipStream_t) {}
void mesh_launch_vertex_f32(const MeshJob&, unsigned, float*, float*, hipStream_t) {}
#endif

}  // namespace

int mdpt_launch_post_mesh(const MeshJob& m, float* xyz, float* uv, unsigned* faces, int* counts, float* bounds, hipStream_t stream) {
    const size_t nv = (size_t)m.nx * m.ny, cells = ((size_t)m.nx - 1) * ((size_t)m.ny - 1);
    if (m.B <= 0 || m.B > 65535 || m.nx < 2 || m.ny < 2 || nv >= ((size_t)1 << 31) || 2 * cells >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    const unsigned nbv = (unsigned)mesh_blocks(nv), nbf = (unsigned)mesh_blocks(cells);
#ifdef MDPT_DEBUG_SWITCHES  // A/B builds only (read at every call: the probe switches within one process)
    const char* fp32_env = getenv("MDPT_MESH_FP32");
    const bool fp32 = fp32_env && fp32_env[0] == '1';
#else
    const bool fp32 = false;
#endif
    if (fp32)
        mesh_launch_flag_f32(m, nbv, stream);
    else
        post_launch("mesh_flag_kernel", mesh_flag_kernel<double>, dim3(nbv, m.B), dim3(256), stream, m);
    if (!m.points) {
        post_launch("mesh_face_count_kernel", mesh_face_count_kernel, dim3(nbf, m.B), dim3(256), stream, m);
    }
    post_launch("mesh_scan_kernel", mesh_scan_kernel, dim3(m.points ? 1 : 2, m.B), dim3(256), stream, m, nbv, nbf, counts);
    if (fp32)
        mesh_launch_vertex_f32(m, nbv, xyz, uv, stream);
    else
        post_launch("mesh_vertex_kernel", mesh_vertex_kernel<double>, dim3(nbv, m.B), dim3(256), stream, m, xyz, uv);
    if (m.points)
        post_launch("mesh_point_kernel", mesh_point_kernel, dim3(nbv, m.B), dim3(256), stream, m, faces, counts, bounds);
    else
        post_launch("mesh_face_kernel", mesh_face_kernel, dim3(nbf, m.B), dim3(256), stream, m, faces, counts, bounds);
    return (int)hipGetLastError();
}
