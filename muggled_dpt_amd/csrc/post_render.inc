// ---- rendering of depth meshes: what the reference's 3D viewer does in a browser with WebGL (3dviewer/index.html:1158-1228 render_3d, the mesh
// shaders of shaders.js) for the slabs of the mesh kernels above, read in place, with their device-side counts. Four launches whatever B and V are:
// (1) the z-buffer cleared to all ones, (2) one thread per (mesh, view, kept vertex): clip = [x, y, z, 1] M in fp64, screen x / y snapped to 1/256
// pixel, 1/w and z01 kept in fp64, (3) one workgroup per 256 faces: int64 edge functions on the snapped coordinates at the pixel centres, top-left
// fill rule, z01 interpolated linearly in screen space, the key (fp32 bits of z01) << 32 | face merged into the uint64 z-buffer with atomicMin - an
// integer vector atomic whose result does not depend on order, so the image is bit-deterministic and ties go to the lower face index - and (4) one
// thread per pixel: the winning face's edge values again, perspective-correct barycentrics, a bilinear texture sample, one rounding to uint8.
// Nothing is contracted: tests/render_restate.py restates the arithmetic in numpy, operation by operation.

namespace {

__device__ __forceinline__ long long render_edge(int ax, int ay, int bx, int by, int px, int py) {
    return ((long long)bx - ax) * ((long long)py - ay) - ((long long)by - ay) * ((long long)px - ax);
}

// a pixel centre ON an edge belongs to the face whose interior lies to its right (a > 0) or, on a horizontal edge, below it (b > 0): the top-left
// rule; (a, b) = the edge function's gradient with the interior positive
__device__ __forceinline__ bool render_edge_in(long long e, long long a, long long b) { return e > 0 || (e == 0 && (a > 0 || (a == 0 && b > 0))); }

// one face of one view, set up: its snapped vertices, s = +1 / -1 so that s x edge is positive inside, E = s x twice the area, and the pixels
// [x0, x1] x [y0, y1] whose centres its bounding box holds, clipped to the viewport. Points: i[0] alone, the square of half-size r.half.
struct RenderTri { int i[3]; int x[3], y[3]; long long s, E; int x0, y0, x1, y1; };

// false: the face does nothing (an index outside the kept vertices, an unusable vertex, no area, culled, or off the viewport)
__device__ __forceinline__ bool render_setup(const RenderJob& r, int b, const RenderVertex* __restrict__ verts, int kv, size_t f, RenderTri& t) {
    const int per = r.points ? 1 : 3;
    const int* fi = r.faces + ((size_t)b * r.nf + f) * per;
    int minx, maxx, miny, maxy;
    for (int k = 0; k < per; ++k) {
        t.i[k] = fi[k];
        if (t.i[k] < 0 || t.i[k] >= kv) return false;
        t.x[k] = verts[t.i[k]].x, t.y[k] = verts[t.i[k]].y;
        if (t.x[k] == RENDER_UNUSABLE) return false;
    }
    if (r.points) {
        t.s = 1, t.E = 1;
        minx = t.x[0] - r.half, maxx = t.x[0] + r.half - 1, miny = t.y[0] - r.half, maxy = t.y[0] + r.half - 1;
    } else {
        const long long area = render_edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
        // rows run downward here, so a triangle that is counter-clockwise with y up - the viewer's front - has a negative area
        if (area == 0 || (area > 0 && r.cull_back)) return false;
        t.s = area < 0 ? -1 : 1, t.E = t.s * area;
        minx = min(t.x[0], min(t.x[1], t.x[2])), maxx = max(t.x[0], max(t.x[1], t.x[2]));
        miny = min(t.y[0], min(t.y[1], t.y[2])), maxy = max(t.y[0], max(t.y[1], t.y[2]));
    }
    // pixel p's centre is at 256 p + 128
    t.x0 = max(0, (minx + 127) >> 8), t.x1 = min(r.W - 1, (maxx - 128) >> 8);
    t.y0 = max(0, (miny + 127) >> 8), t.y1 = min(r.H - 1, (maxy - 128) >> 8);
    return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// the three edge values of pixel (px, py), interior positive, e[k] opposite vertex k -> whether the pixel's centre is covered
__device__ __forceinline__ bool render_cover(const RenderTri& t, int px, int py, long long (&e)[3]) {
    const int X = px * 256 + 128, Y = py * 256 + 128;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = (k + 1) % 3, q = (k + 2) % 3;
        e[k] = t.s * render_edge(t.x[p], t.y[p], t.x[q], t.y[q], X, Y);
        in = in && render_edge_in(e[k], -t.s * ((long long)t.y[q] - t.y[p]), t.s * ((long long)t.x[q] - t.x[p]));
    }
    return in;
}

__device__ __forceinline__ void render_merge(unsigned long long* __restrict__ zb, double z01, unsigned face) {
    if (!(z01 >= 0.0 && z01 <= 1.0)) return;  // near / far
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)z01 + 0.0f) << 32) | face;
    if (key < *zb) atomicMin(zb, key);  // (the plain read can only be stale upward: a key that could win is never skipped)
}

// every pixel of a face's box from `first` in steps of `step`: one lane alone (0, 1) or the workgroup together (threadIdx.x, 256)
__device__ __forceinline__ void render_walk(const RenderJob& r, const RenderVertex* __restrict__ verts, unsigned long long* __restrict__ zb,
                                            const RenderTri& t, unsigned face, int first, int step) {
#pragma clang fp contract(off)
    const int bw = t.x1 - t.x0 + 1, n = bw * (t.y1 - t.y0 + 1);
    const double z0 = verts[t.i[0]].z01;
    if (r.points) {
        for (int p = first; p < n; p += step) render_merge(zb + (size_t)(t.y0 + p / bw) * r.W + (t.x0 + p % bw), z0, face);
        return;
    }
    const double z1 = verts[t.i[1]].z01, z2 = verts[t.i[2]].z01, E = (double)t.E;
    for (int p = first; p < n; p += step) {
        const int px = t.x0 + p % bw, py = t.y0 + p / bw;
        long long e[3];
        if (!render_cover(t, px, py, e)) continue;
        render_merge(zb + (size_t)py * r.W + px, ((double)e[0] * z0 + (double)e[1] * z1 + (double)e[2] * z2) / E, face);
    }
}

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long* __restrict__ zbuf, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) zbuf[i] = ~0ull;
}

__device__ __forceinline__ int render_kept(const RenderJob& r, int b, int which) {
    const int k = r.counts[2 * (size_t)b + which], cap = which ? r.nf : r.nv;
    return k < 0 ? 0 : (k > cap ? cap : k);
}

// blockIdx.y = mesh b x V + view
__global__ __launch_bounds__(256) void render_vertex_kernel(const RenderJob r) {
#pragma clang fp contract(off)
    const int bv = blockIdx.y, b = bv / r.V;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)render_kept(r, b, 0)) return;
    const float* p = r.xyz + ((size_t)b * r.nv + i) * 3;
    const double* M = r.view_proj + (size_t)bv * 16;
    const double x = p[0], y = p[1], z = p[2];
    const double cx = x * M[0] + y * M[4] + z * M[8] + M[12], cy = x * M[1] + y * M[5] + z * M[9] + M[13];
    const double cz = x * M[2] + y * M[6] + z * M[10] + M[14], cw = x * M[3] + y * M[7] + z * M[11] + M[15];
    RenderVertex o{RENDER_UNUSABLE, 0, 0.0, 0.0};
    if (cw > 0.0) {
        const double sx = rint((cx / cw + 1.0) * 0.5 * (double)r.W * 256.0), sy = rint((1.0 - cy / cw) * 0.5 * (double)r.H * 256.0);
        if (fabs(sx) < 1073741824.0 && fabs(sy) < 1073741824.0) o = RenderVertex{(int)sx, (int)sy, 1.0 / cw, (cz / cw + 1.0) * 0.5};
    }
    r.verts[(size_t)bv * r.nv + i] = o;
}

__global__ __launch_bounds__(256) void render_raster_kernel(const RenderJob r) {
    __shared__ unsigned queue[256];
    __shared__ unsigned queued;
    const int bv = blockIdx.y, b = bv / r.V;
    const int kv = render_kept(r, b, 0), kf = render_kept(r, b, 1);
    const size_t first = (size_t)blockIdx.x * 256;
    if (first >= (size_t)kf) return;  // (the whole workgroup)
    if (threadIdx.x == 0) queued = 0;
    __syncthreads();
    const RenderVertex* verts = r.verts + (size_t)bv * r.nv;
    unsigned long long* zb = r.zbuf + (size_t)bv * r.H * r.W;
    const size_t f = first + threadIdx.x;
    RenderTri t;
    if (f < (size_t)kf && render_setup(r, b, verts, kv, f, t)) {
        if ((t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) <= RENDER_SMALL_BOX)
            render_walk(r, verts, zb, t, (unsigned)f, 0, 1);
        else
            queue[atomicAdd(&queued, 1u)] = threadIdx.x;  // (any order: the merge does not depend on it)
    }
    __syncthreads();
    const unsigned n = queued;
    for (unsigned j = 0; j < n; ++j) {
        const size_t g = first + queue[j];
        if (render_setup(r, b, verts, kv, g, t)) render_walk(r, verts, zb, t, (unsigned)g, (int)threadIdx.x, 256);
    }
}

// GL's LINEAR filter with CLAMP_TO_EDGE on one level: texel centres at + 0.5, v = 1 the photo's first row -> the three bytes, rounded once
__device__ __forceinline__ void render_sample(const RenderTex& tex, double u, double v, unsigned char (&bgr)[3]) {
#pragma clang fp contract(off)
    const double tx = fmin(fmax(u * (double)tex.w - 0.5, -1.0), (double)tex.w), ty = fmin(fmax((1.0 - v) * (double)tex.h - 0.5, -1.0), (double)tex.h);
    const double fx0 = floor(tx), fy0 = floor(ty), wx = tx - fx0, wy = ty - fy0;
    const int x0 = min(max((int)fx0, 0), tex.w - 1), x1 = min(max((int)fx0 + 1, 0), tex.w - 1);
    const int y0 = min(max((int)fy0, 0), tex.h - 1), y1 = min(max((int)fy0 + 1, 0), tex.h - 1);
    const unsigned char* top = tex.bgr + (size_t)y0 * tex.w * 3;
    const unsigned char* bot = tex.bgr + (size_t)y1 * tex.w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = (1.0 - wx) * (double)top[3 * x0 + c] + wx * (double)top[3 * x1 + c];
        const double d = (1.0 - wx) * (double)bot[3 * x0 + c] + wx * (double)bot[3 * x1 + c];
        const double val = floor((1.0 - wy) * a + wy * d + 0.5);
        bgr[c] = (unsigned char)(int)fmin(fmax(val, 0.0), 255.0);
    }
}

__global__ __launch_bounds__(256) void render_resolve_kernel(const RenderJob r, uchar4* __restrict__ color, float* __restrict__ depth,
                                                             int* __restrict__ ids) {
#pragma clang fp contract(off)
    const int bv = blockIdx.y, b = bv / r.V;
    const size_t hw = (size_t)r.H * r.W, p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const size_t o = (size_t)bv * hw + p;
    const unsigned long long key = r.zbuf[o];
    uchar4 c = make_uchar4(0, 0, 0, 0);
    float d = INFINITY;
    int id = -1;
    const RenderVertex* verts = r.verts + (size_t)bv * r.nv;
    RenderTri t;
    if (key != ~0ull && render_setup(r, b, verts, render_kept(r, b, 0), (size_t)(unsigned)key, t)) {
        const float* uv = r.uv + (size_t)b * r.nv * 2;
        double u, v, w;
        if (r.points) {
            u = uv[2 * (size_t)t.i[0]], v = uv[2 * (size_t)t.i[0] + 1], w = 1.0 / verts[t.i[0]].invw;
        } else {
            long long e[3];
            render_cover(t, (int)(p % (size_t)r.W), (int)(p / (size_t)r.W), e);
            const double s0 = (double)e[0] * verts[t.i[0]].invw, s1 = (double)e[1] * verts[t.i[1]].invw, s2 = (double)e[2] * verts[t.i[2]].invw;
            const double S = s0 + s1 + s2, b0 = s0 / S, b1 = s1 / S, b2 = s2 / S;
            u = b0 * (double)uv[2 * (size_t)t.i[0]] + b1 * (double)uv[2 * (size_t)t.i[1]] + b2 * (double)uv[2 * (size_t)t.i[2]];
            v = b0 * (double)uv[2 * (size_t)t.i[0] + 1] + b1 * (double)uv[2 * (size_t)t.i[1] + 1] + b2 * (double)uv[2 * (size_t)t.i[2] + 1];
            w = (double)t.E / S;
        }
        unsigned char bgr[3];
        render_sample(r.tex[b], u, v, bgr);
        c = make_uchar4(bgr[0], bgr[1], bgr[2], 255);
        d = (float)w;
        id = (int)(unsigned)key;
    }
    color[o] = c;
    if (depth) depth[o] = d;
    if (ids) ids[o] = id;
}

}  // namespace

int mdpt_launch_post_render(const RenderJob& r, unsigned char* color, float* depth, int* ids, hipStream_t stream) {
    const size_t hw = (size_t)r.H * r.W, faces = (size_t)r.nf;
    if (r.B <= 0 || r.V <= 0 || (size_t)r.B * r.V > 65535 || r.nv <= 0 || r.nf <= 0 || r.H <= 0 || r.W <= 0 || r.H > RENDER_MAX_SIDE ||
        r.W > RENDER_MAX_SIDE || r.half < 0)
        return (int)hipErrorInvalidValue;
    const dim3 by((unsigned)r.B * r.V);
    const size_t cells = hw * r.B * r.V, clear_blocks = (cells + 2047) / 2048;
    post_launch("render_clear_kernel", render_clear_kernel, dim3((unsigned)(clear_blocks > 65536 ? 65536 : clear_blocks)), dim3(256), stream, r.zbuf, cells);
    post_launch("render_vertex_kernel", render_vertex_kernel, dim3((unsigned)(((size_t)r.nv + 255) / 256), by.x), dim3(256), stream, r);
    post_launch("render_raster_kernel", render_raster_kernel, dim3((unsigned)((faces + 255) / 256), by.x), dim3(256), stream, r);
    post_launch("render_resolve_kernel", render_resolve_kernel, dim3((unsigned)((hw + 255) / 256), by.x), dim3(256), stream, r, (uchar4*)color, depth, ids);
    return (int)hipGetLastError();
}
