// ---- surface normals and relighting from depth maps: the normal of every photo pixel under the camera of the mesh export (post_mesh.inc: x right, y up,
// the camera looks along -z), as fp32 unit vectors, as an encoded uint8 BGR normal map, and / or as V relit copies of the photo, one per light. A pair is
// a NormalsPair (mdpt_kernels.h); the table lives in device memory and pairs may all differ in size. At most three launches whatever the number of pairs
// and lights:
//   (1) normals_minmax_kernel ... inverse space only: the fp32 min / max of the FINITE values of every map, 64 workgroups a map -> ordered-key partials in
//                                 the pair's header (finite_minmax_part of post_common.inc: refocus's rule)
//   (2) normals_state_kernel .... inverse space only: one wave a pair, the partials -> lo, hi (finite_range: a zero takes the sign +)
//   (3) normals_tile_kernel ..... one workgroup of 1024 threads owns a 32 x 32 tile of output pixels, one thread each. It stages z of the tile and `step`
//                                 texels of halo into LDS once as fp64 (the four corners of the halo, which no tap reads, left out): s = the map at the
//                                 pixel's centre (map_at_pixel_centre), z = 1 / (a + b v) with v = (s - lo) / (hi - lo) or 0 for a flat map (inverse
//                                 space; valid iff s is finite) or z = s (depth space; valid iff s is finite and > 0); NaN marks an invalid texel and
//                                 everything outside the photo. P = ((z x) kx, (z y) ky, -z) is recomputed from z and the pixel's coordinates, so one
//                                 plane is staged. Each thread takes its four neighbours at +-step from LDS, picks per axis the central difference
//                                 or, across a depth edge or next to an unusable neighbour, the one-sided difference, forms the normal once and then
//                                 loops over the V lights: the normal never goes through memory and is never recomputed per light.
// All fp64, nothing contracted, every result rounded once; the arithmetic is written out in include/mdpt.h. Bit-deterministic, no atomics, no workgroup
// waits for another, nothing read back; a launch boundary separates every producer from its consumer.
// LDS: 64 x 64 x 8 bytes = 32 KiB whatever the step (row pitch 64 texels). A wave is two tile rows of 32 consecutive texels and every tap of it - the
// centre, the row taps at +-step, the column taps at rows -+step - is 32 consecutive 8-byte texels per half wave: one ds_read_b64 covers 256 contiguous
// bytes, all 64 banks once, whatever the row pitch, so neither the row nor the column taps conflict.

namespace {

// what launch (2) leaves for launch (3), behind the partials of launch (1) in the pair's header
struct NormalsState { double lo, hi; int ranged, pad; };
static_assert(NORMALS_PARTS * 2 * sizeof(unsigned) + sizeof(NormalsState) <= NORMALS_HEADER_BYTES && NORMALS_HEADER_BYTES % 8 == 0, "the header of a pair's scratch");
static_assert(NORMALS_PARTS == 64, "normals_state_kernel reduces the partials with one wave");
static_assert(NORMALS_TILE + 2 * NORMALS_MAX_STEP == 64, "the LDS image of normals_tile_kernel");

// (Pair: NormalsPair, or the ShadowsPair of post_shadows.inc, whose header is laid out alike)
template <typename Pair>
__device__ __forceinline__ unsigned* normals_parts(const Pair& p, char* scratch) { return (unsigned*)(scratch + p.scratch_off); }
template <typename Pair>
__device__ __forceinline__ NormalsState* normals_state(const Pair& p, char* scratch) {
    return (NormalsState*)(scratch + p.scratch_off + NORMALS_PARTS * 2 * sizeof(unsigned));
}

// (1) blockIdx.y = pair, blockIdx.x = one of the 64 shares of the map
__global__ __launch_bounds__(256) void normals_minmax_kernel(const NormalsPair* __restrict__ pairs, int dt, char* __restrict__ scratch) {
    const NormalsPair p = pairs[blockIdx.y];
    finite_minmax_part(p.map, (size_t)p.h * p.w, dt, blockIdx.x, NORMALS_PARTS, normals_parts(p, scratch) + 2 * blockIdx.x);
}

// the body of launch (2): one wave reduces the partials of pair p and lane 0 stores its state
template <typename Pair>
__device__ __forceinline__ void normals_state_of(const Pair& p, char* __restrict__ scratch) {
    const unsigned* parts = normals_parts(p, scratch);
    unsigned lo_o = parts[2 * threadIdx.x], hi_o = parts[2 * threadIdx.x + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo_o = min(lo_o, __shfl_xor(lo_o, o));
        hi_o = max(hi_o, __shfl_xor(hi_o, o));
    }
    if (threadIdx.x != 0) return;
    NormalsState st{};
    st.ranged = finite_range(lo_o, hi_o, st.lo, st.hi);
    *normals_state(p, scratch) = st;
}

// (2) blockIdx.x = pair, one wave
__global__ __launch_bounds__(64) void normals_state_kernel(const NormalsPair* __restrict__ pairs, char* __restrict__ scratch) {
    normals_state_of(pairs[blockIdx.x], scratch);
}

struct NormalsVec { double x, y, z; };

// the camera-space point of pixel (Y, X) of an H x W image at depth z (Cam: anything with H, W, kx, ky - a pair, or the working grid of post_shadows.inc)
struct NormalsCam { int H, W; double kx, ky; };
template <typename Cam>
__device__ __forceinline__ NormalsVec normals_point(const Cam& p, double z, int Y, int X) {
#pragma clang fp contract(off)
    const double x = 2.0 * ((double)X + 0.5) / (double)p.W - 1.0, y = 1.0 - 2.0 * ((double)Y + 0.5) / (double)p.H;
    return NormalsVec{(z * x) * p.kx, (z * y) * p.ky, -z};
}

__device__ __forceinline__ NormalsVec normals_sub(const NormalsVec& a, const NormalsVec& b) {
#pragma clang fp contract(off)
    return NormalsVec{a.x - b.x, a.y - b.y, a.z - b.z};
}

// The tangent along one axis: A = the neighbour at +step (x axis: X + step; y axis: Y - step, up), B the one at -step, a NaN depth = not usable.
// Both usable: central where the two depth differences are within edge_ratio of each other, else the side with the smaller one; one usable: that side.
// -> false where neither is.
template <typename Job, typename Cam>
__device__ __forceinline__ bool normals_tangent(const Job& j, const Cam& p, double z0, const NormalsVec& P0, double zA, int YA, int XA,
                                                double zB, int YB, int XB, NormalsVec& T) {
#pragma clang fp contract(off)
    const bool useA = zA == zA, useB = zB == zB;
    if (!useA && !useB) return false;
    bool takeA = useA, takeB = useB;
    if (useA && useB && !j.central_only) {
        const double da = fabs(zA - z0), db = fabs(z0 - zB);
        if (!(da <= j.edge_ratio * db && db <= j.edge_ratio * da)) {
            takeA = da < db;
            takeB = !takeA;
        }
    }
    const NormalsVec PA = takeA ? normals_point(p, zA, YA, XA) : P0, PB = takeB ? normals_point(p, zB, YB, XB) : P0;
    T = normals_sub(PA, PB);
    return true;
}

// the pair's depth range as the staging loops use it (inverse space: what launch (2) left; depth space: not read)
struct NormalsRange { double lo, range; bool ranged; };
template <typename Job, typename Pair>
__device__ __forceinline__ NormalsRange normals_range(const Job& j, const Pair& p) {
#pragma clang fp contract(off)
    NormalsRange r{0.0, 0.0, false};
    if (!j.depth_space) {
        const NormalsState st = *normals_state(p, j.scratch);
        r.lo = st.lo, r.range = st.hi - st.lo, r.ranged = st.ranged != 0;
    }
    return r;
}

// z of pixel (Y, X) of an H x W image over the pair's map, NaN where it lies outside the image or is invalid
template <typename Job, typename Pair>
__device__ __forceinline__ double normals_depth(const Job& j, const Pair& p, const NormalsRange& r, int H, int W, int Y, int X) {
#pragma clang fp contract(off)
    double z = NAN;
    if (Y >= 0 && Y < H && X >= 0 && X < W) {
        const double s = map_at_pixel_centre(p.map, j.dt, p.h, p.w, H, W, Y, X);
        if (j.depth_space) {
            if (isfinite(s) && s > 0.0) z = s;
        } else if (isfinite(s)) {
            const double v = r.ranged ? (s - r.lo) / r.range : 0.0;
            z = 1.0 / (j.depth_a + j.depth_b * v);
        }
    }
    return z;
}

// The normal of pixel (Y, X) from the staged depths: centre = its texel in an LDS image of row pitch S, the neighbours t texels away. -> whether it has
// one; P0 is set where the centre is valid, n where the normal is.
template <typename Job, typename Cam>
__device__ __forceinline__ bool normals_at(const Job& j, const Cam& p, const double* centre, int S, int t, int Y, int X, NormalsVec& P0, NormalsVec& n) {
#pragma clang fp contract(off)
    const double z0 = *centre;
    bool valid = z0 == z0;
    if (valid) {
        P0 = normals_point(p, z0, Y, X);
        NormalsVec Tx, Ty;
        valid = normals_tangent(j, p, z0, P0, centre[t], Y, X + t, centre[-t], Y, X - t, Tx) &&
                normals_tangent(j, p, z0, P0, centre[-t * S], Y - t, X, centre[t * S], Y + t, X, Ty);
        if (valid) {
            const double nx = Tx.y * Ty.z - Tx.z * Ty.y, ny = Tx.z * Ty.x - Tx.x * Ty.z, nz = Tx.x * Ty.y - Tx.y * Ty.x;
            const double len2 = (nx * nx + ny * ny) + nz * nz;
            valid = isfinite(len2) && len2 > 0.0;
            if (valid) {
                const double len = sqrt(len2);
                n = NormalsVec{nx / len, ny / len, nz / len};
            }
        }
    }
    return valid;
}

// The body of launch (3), blockIdx.x = a tile of the call (pair_of_tile); thread = (ty, tx) of the tile, tx fastest. OCC = false: normals_tile_kernel
// (Job = NormalsJob). OCC = true: the shade kernel of post_shadows.inc (Job = ShadowsJob), the same pixel with the two factors of its planes in the mix -
// shade = ambient a + (diffuse d) s_v, spec = 255 ((specular sp) s_v) - and no normals / encoded outputs.
template <bool OCC, typename Job>
__device__ __forceinline__ void normals_tile_body(const Job& j) {
#pragma clang fp contract(off)
    constexpr int T = NORMALS_TILE, S = T + 2 * NORMALS_MAX_STEP, THREADS = T * T;
    __shared__ double zt[S * S];
    __shared__ int which;
    const int tid = (int)threadIdx.x;
    if (tid == 0) which = pair_of_tile(j.pairs, j.P, (long long)blockIdx.x);
    __syncthreads();
    const auto p = j.pairs[which];  // (a NormalsPair, or a ShadowsPair)
    const int tile = (int)((long long)blockIdx.x - p.tile_off), tiles_x = (p.W + T - 1) / T;
    const int X0 = (tile % tiles_x) * T, Y0 = (tile / tiles_x) * T;
    const int t = p.step, side = T + 2 * t;  // (1 <= t <= NORMALS_MAX_STEP, checked on the host: side <= S)
    const NormalsRange range = normals_range(j, p);
    for (int idx = tid; idx < side * side; idx += THREADS) {
        const int ly = idx / side, lx = idx - ly * side;
        if ((ly < t || ly >= t + T) && (lx < t || lx >= t + T)) continue;  // a corner of the halo: no tap reads it
        zt[ly * S + lx] = normals_depth(j, p, range, p.H, p.W, Y0 - t + ly, X0 - t + lx);  // (NaN: outside the photo, or invalid)
    }
    __syncthreads();

    const int tx = tid % T, ty = tid / T, X = X0 + tx, Y = Y0 + ty;
    if (X >= p.W || Y >= p.H) return;
    NormalsVec P0{0.0, 0.0, 0.0}, n{0.0, 0.0, 0.0};
    const bool valid = normals_at(j, p, zt + (ty + t) * S + tx + t, S, t, Y, X, P0, n);
    const size_t i = (size_t)Y * p.W + X;
    if constexpr (!OCC) {
        if (p.normals) {
            float* o = p.normals + 3 * i;
            o[0] = (float)n.x, o[1] = (float)n.y, o[2] = (float)n.z;
        }
        if (p.encoded) {
            unsigned char* o = p.encoded + 3 * i;
            o[0] = (unsigned char)floor((n.z + 1.0) / 2.0 * 255.0 + 0.5);
            o[1] = (unsigned char)floor((n.y + 1.0) / 2.0 * 255.0 + 0.5);
            o[2] = (unsigned char)floor((n.x + 1.0) / 2.0 * 255.0 + 0.5);
        }
    }
    if (!p.relit) return;
    unsigned c0 = 255u, c1 = 255u, c2 = 255u;
    if (p.photo) {  // read byte by byte through the pitch: no alignment is asked of a photo
        const unsigned char* px = p.photo + (long long)Y * p.pitch + 3LL * X;
        c0 = px[0], c1 = px[1], c2 = px[2];
    }
    NormalsVec view{0.0, 0.0, 0.0};
    if (valid && j.specular > 0.0) {
        const double plen = sqrt((P0.x * P0.x + P0.y * P0.y) + P0.z * P0.z);
        view = NormalsVec{-P0.x / plen, -P0.y / plen, -P0.z / plen};
    }
    const size_t frame = (size_t)p.H * p.W * 3;
    unsigned char* o = p.relit + 3 * i;
    // OCC: the pair's planes at the pixel's centre, by map_at_pixel_centre's rule with the taps formed once for the 1 + V planes
    [[maybe_unused]] BilinearTaps taps{};
    [[maybe_unused]] bool direct = false;
    [[maybe_unused]] double amb = j.ambient;
    [[maybe_unused]] auto plane_at = [&](const float* g) -> double {
        if constexpr (OCC) {
            if (direct) return (double)g[(size_t)Y * p.gw + X];
            return bilinear_f64_mix(taps, (double)g[(size_t)taps.y0 * p.gw + taps.x0], (double)g[(size_t)taps.y0 * p.gw + taps.x1],
                                    (double)g[(size_t)taps.y1 * p.gw + taps.x0], (double)g[(size_t)taps.y1 * p.gw + taps.x1]);
        } else {
            return 1.0;
        }
    };
    if constexpr (OCC) {
        direct = p.gh == p.H && p.gw == p.W;
        if (valid && !direct && (j.use_ao || j.use_vis)) taps = bilinear_f64_taps(p.gh, p.gw, (double)X + 0.5, (double)Y + 0.5, p.H, p.W);
        if (valid && j.use_ao) amb = j.ambient * plane_at(p.ao);
    }
    for (int v = 0; v < j.V; ++v, o += frame) {
        if (!valid) {
            o[0] = (unsigned char)c0, o[1] = (unsigned char)c1, o[2] = (unsigned char)c2;
            continue;
        }
        const double lx = j.lights[3 * v], ly = j.lights[3 * v + 1], lz = j.lights[3 * v + 2];
        const double dot = (n.x * lx + n.y * ly) + n.z * lz;
        double shade, sv = 1.0;
        if constexpr (OCC) {
            if (j.use_vis) sv = plane_at(p.vis + (size_t)v * p.gh * p.gw);
            shade = amb + (j.diffuse * (dot > 0.0 ? dot : 0.0)) * sv;
        } else {
            shade = j.ambient + j.diffuse * (dot > 0.0 ? dot : 0.0);
        }
        double spec = 0.0;
        if (j.specular > 0.0) {
            const double hx = lx + view.x, hy = ly + view.y, hz = lz + view.z;
            const double hlen = sqrt((hx * hx + hy * hy) + hz * hz);
            const double nh = (n.x * (hx / hlen) + n.y * (hy / hlen)) + n.z * (hz / hlen);
            double sp = nh > 0.0 ? nh : 0.0;  // (a NaN - the light straight behind the view - is 0)
            for (int k = 0; k < j.shininess_log2; ++k) sp = sp * sp;
            spec = OCC ? 255.0 * ((j.specular * sp) * sv) : 255.0 * (j.specular * sp);
        }
        o[0] = (unsigned char)fmin(255.0, floor(((double)c0 * shade + spec) + 0.5));
        o[1] = (unsigned char)fmin(255.0, floor(((double)c1 * shade + spec) + 0.5));
        o[2] = (unsigned char)fmin(255.0, floor(((double)c2 * shade + spec) + 0.5));
    }
}

// (3)
__global__ __launch_bounds__(NORMALS_TILE* NORMALS_TILE) void normals_tile_kernel(NormalsJob j) { normals_tile_body<false>(j); }

}  // namespace

int mdpt_launch_post_normals(const NormalsJob& j, hipStream_t stream) {
    if (j.P <= 0 || j.P > 65535 || j.V < 0 || j.V > NORMALS_MAX_LIGHTS || j.shininess_log2 < 0 || j.shininess_log2 > 10 || j.total_tiles == 0 ||
        j.total_tiles >= ((size_t)1 << 31))
        return (int)hipErrorInvalidValue;
    if (!j.depth_space) {
        post_launch("normals_minmax_kernel", normals_minmax_kernel, dim3(NORMALS_PARTS, j.P), dim3(256), stream, j.pairs, j.dt, j.scratch);
        post_launch("normals_state_kernel", normals_state_kernel, dim3(j.P), dim3(64), stream, j.pairs, j.scratch);
    }
    post_launch("normals_tile_kernel", normals_tile_kernel, dim3((unsigned)j.total_tiles), dim3(NORMALS_TILE * NORMALS_TILE), stream, j);
    return (int)hipGetLastError();
}
