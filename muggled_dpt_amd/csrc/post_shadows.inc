// ---- cast shadows and ambient occlusion for the relighting (post_normals.inc): screen-space shadow marches and horizon occlusion on a small working grid
// of gh x gw nodes over the photo's field of view, resized to the photo and folded into the shading. A pair is a ShadowsPair (mdpt_kernels.h); the table
// lives in device memory and pairs may all differ in size. At most four launches whatever the number of pairs and lights:
//   (1) shadows_minmax_kernel ... inverse space only: normals_minmax_kernel's partials over this table (finite_minmax_part of post_common.inc)
//   (2) shadows_state_kernel .... inverse space only: one wave a pair, the partials -> lo, hi (normals_state_of)
//   (3) shadows_grid_kernel ..... one workgroup of 1024 threads owns a 32 x 32 tile of grid nodes, one thread each. It stages z of the tile and r nodes of
//                                 halo (r = the larger reach of the call, at least the normal's one node, at most 32) into LDS once as fp64, by the
//                                 rule of normals_tile_kernel (normals_depth: NaN marks an invalid node and everything outside the grid), forms the
//                                 node's normal once (normals_at, step one node), runs the eight occlusion directions and then loops over the V
//                                 lights with z0, P0 and n in registers; every tap is an LDS read. Writes ao fp32 [gh,gw] and vis fp32 [V,gh,gw].
//   (4) shadows_shade_kernel .... normals_tile_body<true>: normals_tile_kernel's pixel with the two planes, read at the pixel's centre, in the mix.
// All fp64, nothing contracted, every stored value rounded once, only + - * / sqrt floor and comparisons; the arithmetic is written out in include/mdpt.h.
// Bit-deterministic, no atomics, no workgroup waits for another, nothing read back; a launch boundary separates every producer from its consumer.
// LDS of (3): 96 x 96 x 8 bytes = 72 KiB whatever the reach (row pitch 96 nodes), so two workgroups fit the 160 KiB of a CU. Expected bank behaviour,
// NOT measured: a wave is two tile rows of 32 consecutive nodes. The normal's taps and the occlusion taps are whole-row shifts - every lane of a half
// wave adds the same (k di, k dj) - so a ds_read_b64 covers 256 contiguous bytes, all 64 banks once, as in normals_tile_kernel. The shadow taps are not:
// every lane rounds its own projected direction, which turns slowly with the node's position, so neighbouring lanes follow nearly parallel lines and read
// nearly consecutive nodes, with a repeated or skipped node where the rounding differs between two lanes (a two-way conflict there) and with lanes
// dropping out as their marches end.

namespace {

static_assert(NORMALS_TILE + 2 * SHADOWS_MAX_REACH == 96 && SHADOWS_MAX_REACH >= 1, "the LDS image of shadows_grid_kernel");
static_assert(SHADOWS_AO_DIRECTIONS == 8, "the lattice directions of shadows_grid_kernel");

// (1) blockIdx.y = pair, blockIdx.x = one of the 64 shares of the map
__global__ __launch_bounds__(256) void shadows_minmax_kernel(const ShadowsPair* __restrict__ pairs, int dt, char* __restrict__ scratch) {
    const ShadowsPair p = pairs[blockIdx.y];
    finite_minmax_part(p.map, (size_t)p.h * p.w, dt, blockIdx.x, NORMALS_PARTS, normals_parts(p, scratch) + 2 * blockIdx.x);
}

// (2) blockIdx.x = pair, one wave
__global__ __launch_bounds__(64) void shadows_state_kernel(const ShadowsPair* __restrict__ pairs, char* __restrict__ scratch) {
    normals_state_of(pairs[blockIdx.x], scratch);
}

// (3) blockIdx.x = a grid tile of the call (pair_of_tile over gtile_off); thread = (ty, tx) of the tile, tx fastest
__global__ __launch_bounds__(NORMALS_TILE* NORMALS_TILE) void shadows_grid_kernel(ShadowsJob j) {
#pragma clang fp contract(off)
    constexpr int T = NORMALS_TILE, S = T + 2 * SHADOWS_MAX_REACH, THREADS = T * T;
    __shared__ double zt[S * S];
    __shared__ int which;
    const int tid = (int)threadIdx.x;
    if (tid == 0) which = pair_of_tile(j.pairs, j.P, (long long)blockIdx.x, &ShadowsPair::gtile_off);
    __syncthreads();
    const ShadowsPair p = j.pairs[which];
    const int tile = (int)((long long)blockIdx.x - p.gtile_off), tiles_x = (p.gw + T - 1) / T;
    const int J0 = (tile % tiles_x) * T, I0 = (tile / tiles_x) * T;
    const int shadow_reach = p.vis ? j.shadow_reach : 0, ao_reach = p.ao ? j.ao_reach : 0;
    const int r = max(1, max(shadow_reach, ao_reach)), side = T + 2 * r;  // (reach <= SHADOWS_MAX_REACH, checked on the host: side <= S)
    const NormalsRange range = normals_range(j, p);
    for (int idx = tid; idx < side * side; idx += THREADS) {
        const int ly = idx / side, lx = idx - ly * side;
        zt[ly * S + lx] = normals_depth(j, p, range, p.gh, p.gw, I0 - r + ly, J0 - r + lx);  // (NaN: outside the grid, or invalid)
    }
    __syncthreads();

    const int tx = tid % T, ty = tid / T, J = J0 + tx, I = I0 + ty;
    if (J >= p.gw || I >= p.gh) return;
    const NormalsCam cam{p.gh, p.gw, p.kx, p.ky};
    const double* centre = zt + (ty + r) * S + tx + r;
    NormalsVec P0{0.0, 0.0, 0.0}, n{0.0, 0.0, 0.0};
    const bool valid = normals_at(j, cam, centre, S, 1, I, J, P0, n);
    const size_t planes = (size_t)p.gh * p.gw, node = (size_t)I * p.gw + J;
    const double z0 = *centre;

    if (p.ao) {
        double ao = 1.0;
        if (valid) {
            const double rad = j.ao_radius * z0, rad2 = rad * rad;
            double sum = 0.0;
            // counter-clockwise from the right as the camera sees it (rows grow downwards): E, NE, N, NW, W, SW, S, SE
            constexpr int DI[SHADOWS_AO_DIRECTIONS] = {0, -1, -1, -1, 0, 1, 1, 1}, DJ[SHADOWS_AO_DIRECTIONS] = {1, 1, 0, -1, -1, -1, 0, 1};
#pragma unroll
            for (int d = 0; d < SHADOWS_AO_DIRECTIONS; ++d) {
                double occ = 0.0;
                for (int k = 1; k <= ao_reach; ++k) {
                    const int di = k * DI[d], dj = k * DJ[d];
                    if (I + di < 0 || I + di >= p.gh || J + dj < 0 || J + dj >= p.gw) break;
                    const double zq = centre[di * S + dj];
                    if (!(zq == zq)) continue;
                    const NormalsVec D = normals_sub(normals_point(cam, zq, I + di, J + dj), P0);
                    const double l2 = (D.x * D.x + D.y * D.y) + D.z * D.z;
                    const double hgt = ((D.x * n.x + D.y * n.y) + D.z * n.z) / sqrt(l2);
                    const double fall = 1.0 - l2 / rad2, rise = hgt - j.ao_bias;
                    const double term = (rise > 0.0 ? rise : 0.0) * (fall > 0.0 ? fall : 0.0);
                    if (term > occ) occ = term;
                }
                sum += occ;
            }
            const double open = 1.0 - (j.ao_strength * sum) / 8.0;
            ao = open > 0.0 ? open : 0.0;
        }
        p.ao[node] = (float)ao;
    }
    if (!p.vis) return;

    const double x0 = 2.0 * ((double)J + 0.5) / (double)p.gw - 1.0, y0 = 1.0 - 2.0 * ((double)I + 0.5) / (double)p.gh;  // (normals_point's)
    const double lit_below = 1.0 - j.shadow_bias;
    float* o = p.vis + node;
    for (int v = 0; v < j.V; ++v, o += planes) {
        float vis = 1.0f;
        const double Lx = j.lights[3 * v], Ly = j.lights[3 * v + 1], Lz = j.lights[3 * v + 2];
        const double gx = (Lx / p.kx + x0 * Lz) * (double)p.gw, gy = -((Ly / p.ky + y0 * Lz) * (double)p.gh);
        if (valid && !(gx == 0.0 && gy == 0.0) && isfinite(gx) && isfinite(gy)) {
            const bool x_major = fabs(gx) >= fabs(gy);
            const double m = x_major ? fabs(gx) : fabs(gy), sx = gx / m, sy = gy / m;
            // the ray parameter on the major axis c (x or y): t = ((z0 kc) (cq - c0)) / (Lc + (Lz kc) cq)
            const double kc = x_major ? p.kx : p.ky, c0 = x_major ? x0 : y0, Lc = x_major ? Lx : Ly, zk = z0 * kc, Lk = Lz * kc;
            for (int k = 1; k <= shadow_reach; ++k) {
                const int di = (int)floor((double)k * sy + 0.5), dj = (int)floor((double)k * sx + 0.5);
                const int qi = I + di, qj = J + dj;
                if (qi < 0 || qi >= p.gh || qj < 0 || qj >= p.gw) break;
                const double cq = x_major ? 2.0 * ((double)qj + 0.5) / (double)p.gw - 1.0 : 1.0 - 2.0 * ((double)qi + 0.5) / (double)p.gh;
                const double t = (zk * (cq - c0)) / (Lc + Lk * cq), zr = z0 - t * Lz;
                if (!(t > 0.0) || !(zr > 0.0)) break;
                const double zq = centre[di * S + dj];  // (|di|, |dj| <= k <= r: inside the staged image)
                if (zq == zq && zq < zr * lit_below && (j.thick_inf || zr - zq <= j.shadow_thickness * zr)) {
                    vis = 0.0f;
                    break;
                }
            }
        }
        *o = vis;
    }
}

// (4)
__global__ __launch_bounds__(NORMALS_TILE* NORMALS_TILE) void shadows_shade_kernel(ShadowsJob j) { normals_tile_body<true>(j); }

}  // namespace

int mdpt_launch_post_shadows(const ShadowsJob& j, hipStream_t stream) {
    if (j.P <= 0 || j.P > 65535 || j.V < 0 || j.V > NORMALS_MAX_LIGHTS || j.shininess_log2 < 0 || j.shininess_log2 > 10 || j.shadow_reach < 0 ||
        j.shadow_reach > SHADOWS_MAX_REACH || j.ao_reach < 0 || j.ao_reach > SHADOWS_MAX_REACH || (!j.planes && !j.shade) ||
        (j.planes && (j.total_gtiles == 0 || j.total_gtiles >= ((size_t)1 << 31))) || (j.shade && (j.total_tiles == 0 || j.total_tiles >= ((size_t)1 << 31))))
        return (int)hipErrorInvalidValue;
    if (!j.depth_space) {
        post_launch("shadows_minmax_kernel", shadows_minmax_kernel, dim3(NORMALS_PARTS, j.P), dim3(256), stream, j.pairs, j.dt, j.scratch);
        post_launch("shadows_state_kernel", shadows_state_kernel, dim3(j.P), dim3(64), stream, j.pairs, j.scratch);
    }
    if (j.planes)
        post_launch("shadows_grid_kernel", shadows_grid_kernel, dim3((unsigned)j.total_gtiles), dim3(NORMALS_TILE * NORMALS_TILE), stream, j);
    if (j.shade)
        post_launch("shadows_shade_kernel", shadows_shade_kernel, dim3((unsigned)j.total_tiles), dim3(NORMALS_TILE * NORMALS_TILE), stream, j);
    return (int)hipGetLastError();
}
