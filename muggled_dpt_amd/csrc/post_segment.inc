// ---- depth segmentation (not in the reference): connected-component labelling of a depth map over the criterion the mesh export cuts faces by and
// the normals stop differences at - a depth discontinuity between neighbouring nodes - with a table of the regions and pick-to-cutout. An image is a
// SegmentImage (mdpt_kernels.h); the table lives in device memory and images may all differ in size. Ten launches whatever the number of images:
//   (1) segment_minmax_kernel .... the fp32 min / max of the VALID nodes of every map (finite; in depth space also > 0), 64 workgroups a map
//   (2) segment_state_kernel ..... one wave an image: the partials -> lo, hi, the link threshold step (hi - lo) of inverse space -> header and range[]
//   (3) segment_tile_kernel ...... one workgroup of 1024 threads per 32 x 32 tile, one thread a node. The values and one node of halo (left, right,
//                                  below) go to LDS, every node forms its link bits ONCE (E, S and, at 8-connectivity, SE, SW: each pair belongs to its
//                                  upper node) and the tile's components are found by a union-find in LDS (segment_union below, workgroup scope).
//                                  -> every node's parent as a linear index y w + x of the image (-1: not valid), its link bits, aux = 0
//   (4) segment_merge_kernel ..... one workgroup a tile, one thread per node of the tile's left and right columns and last row: every linked pair that
//                                  crosses a tile edge is united in global memory by the same segment_union, agent scope
//   (5) segment_flatten_kernel ... every node follows its chain to the root, stores it and adds 1 to the root's area (aux)
//   (6) segment_flag_kernel ...... the kept roots (area >= min_area) of every block of 256 nodes
//   (7) segment_scan_kernel ...... one workgroup an image scans the block counts with a running carry (the mesh export's scheme) -> counts[]
//   (8) segment_scatter_kernel ... a kept root's rank in raster order is its region: area, first, the neutral elements of the other columns; aux
//                                  becomes the old root -> region map (-1: dropped)
//   (9) segment_relabel_kernel ... labels, and bbox / vmin / vmax / sum_q through integer atomics (min, max, 64-bit add)
//  (10) segment_finish_kernel .... vmin / vmax from ordered keys to fp32
//
// segment_union(a, b): a = find(a), b = find(b); equal: done; the larger root goes under the smaller: old = atomicMin(&parent[larger], smaller); old ==
// larger: it was a root and is linked now, done; else somebody got there first - parent[larger] is min(old, smaller), whichever link that lost is made
// again by uniting old and smaller: continue from there. Lock-free: no thread waits for another, and the larger of the two indices falls with every
// round, so it ends. Visibility in launch (4): the XCDs' L2s are not coherent and a CU's L1 is never refreshed, so a find may read an OLD parent. Every
// value parent[x] ever holds is a node of x's final component, is <= x, and only falls; a stale one is therefore an older ancestor: the chain still
// descends and ends at a node of the right component, at worst one that is no longer a root. Correctness rests on the atomicMin alone, which executes
// at the memory side and returns the truth: it either links a true root (old == larger) or hands back the true parent to continue from. Linking under a
// node that has stopped being a root is harmless - it is a smaller index of the same component, so no cycle and no wrong merge. The finds of launch (4)
// are agent-scope atomic loads all the same (they bypass L1, which keeps the chains short); launch (5) is a launch of its own, so it sees everything.
// In launch (5) the in-place store of a root races with other chains walking through that node: both the old and the new value are ancestors.
// Every output is an integer or an fp32 value moved, never computed; sums are integers; nothing depends on the order of the atomics: bit-deterministic.
// No float atomics, no workgroup waits for another, nothing read back.

namespace {

struct SegmentState { double lo, hi, thr; };
static_assert(SEGMENT_PARTS * 2 * sizeof(unsigned) + sizeof(SegmentState) <= SEGMENT_HEADER_BYTES && SEGMENT_HEADER_BYTES % 8 == 0, "the header of an image's scratch");
constexpr int SEGMENT_E = 1, SEGMENT_S = 2, SEGMENT_SE = 4, SEGMENT_SW = 8;  // link bits of a node: to (x + 1, y), (x, y + 1), (x + 1, y + 1), (x - 1, y + 1)

__device__ __forceinline__ unsigned* segment_parts(const SegmentImage& p, char* scratch) { return (unsigned*)(scratch + p.scratch_off); }
__device__ __forceinline__ SegmentState* segment_state(const SegmentImage& p, char* scratch) {
    return (SegmentState*)(scratch + p.scratch_off + SEGMENT_PARTS * 2 * sizeof(unsigned));
}
__device__ __forceinline__ int* segment_aux(const SegmentImage& p, char* scratch) { return (int*)(scratch + p.scratch_off + SEGMENT_HEADER_BYTES); }
__device__ __forceinline__ unsigned char* segment_links(const SegmentImage& p, char* scratch) {
    return (unsigned char*)(scratch + p.scratch_off + SEGMENT_HEADER_BYTES + 4 * (size_t)p.h * p.w);
}
__device__ __forceinline__ unsigned* segment_bcnt(const SegmentImage& p, char* scratch) {
    const size_t n = (size_t)p.h * p.w;
    return (unsigned*)(scratch + p.scratch_off + SEGMENT_HEADER_BYTES + 4 * n + ((n + 7) & ~(size_t)7));
}

__device__ __forceinline__ bool segment_valid(float v, int depth_space) { return isfinite(v) && (!depth_space || v > 0.0f); }
// two VALID neighbours are linked: |vp - vq| <= step (hi - lo) (inverse space, the right side once per image) or <= step min(vp, vq) (depth space)
__device__ __forceinline__ bool segment_linked(float vp, float vq, int depth_space, double step, double thr) {
#pragma clang fp contract(off)
    const double a = (double)vp, b = (double)vq;
    const double bound = depth_space ? step * fmin(a, b) : thr;
    return fabs(a - b) <= bound;
}

// the union-find of the header comment; SCOPE = __HIP_MEMORY_SCOPE_WORKGROUP (LDS) or __HIP_MEMORY_SCOPE_AGENT (global memory)
template <int SCOPE>
__device__ __forceinline__ int segment_find(int* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        x = p;
    }
}
template <int SCOPE>
__device__ __forceinline__ void segment_union(int* parent, int a, int b) {
    for (;;) {
        a = segment_find<SCOPE>(parent, a);
        b = segment_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

// (1) blockIdx.y = image, blockIdx.x = one of the 64 shares of the map
__global__ __launch_bounds__(256) void segment_minmax_kernel(const SegmentImage* __restrict__ images, int dt, int depth_space, char* __restrict__ scratch) {
    const SegmentImage p = images[blockIdx.y];
    unsigned* part = segment_parts(p, scratch) + 2 * blockIdx.x;
    const size_t n = (size_t)p.h * p.w;
    if (!depth_space) {
        finite_minmax_part(p.map, n, dt, blockIdx.x, SEGMENT_PARTS, part);
        return;
    }
    float lo = INFINITY, hi = -INFINITY;  // (finite_minmax_part with depth space's rule of validity)
    bool any = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)SEGMENT_PARTS * 256) {
        const float v = ld_dt(p.map, i, dt);
        if (segment_valid(v, 1)) {
            lo = fminf(lo, v), hi = fmaxf(hi, v);
            any = true;
        }
    }
    block_minmax_part(lo, hi, false, any, part);
}

// (2) blockIdx.x = image, one wave
__global__ __launch_bounds__(64) void segment_state_kernel(SegmentJob j) {
#pragma clang fp contract(off)
    const SegmentImage p = j.images[blockIdx.x];
    const unsigned* parts = segment_parts(p, j.scratch);
    unsigned lo_o = parts[2 * threadIdx.x], hi_o = parts[2 * threadIdx.x + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo_o = min(lo_o, __shfl_xor(lo_o, o));
        hi_o = max(hi_o, __shfl_xor(hi_o, o));
    }
    if (threadIdx.x != 0) return;
    SegmentState st{};
    finite_range(lo_o, hi_o, st.lo, st.hi);
    st.thr = j.step * (st.hi - st.lo);
    *segment_state(p, j.scratch) = st;
    j.range[2 * (size_t)blockIdx.x] = st.lo, j.range[2 * (size_t)blockIdx.x + 1] = st.hi;
}

// (3) blockIdx.x = a tile of the call. LDS: rows Y0 .. Y0 + 32 of columns X0 - 1 .. X0 + 32 (outside the image: NaN, which is not valid), the parents.
__global__ __launch_bounds__(SEGMENT_TILE* SEGMENT_TILE) void segment_tile_kernel(SegmentJob j) {
    constexpr int T = SEGMENT_TILE, S = T + 2, ROWS = T + 1, THREADS = T * T;
    __shared__ float val[ROWS * S];
    __shared__ int lab[THREADS];
    __shared__ int which;
    const int tid = (int)threadIdx.x;
    if (tid == 0) which = pair_of_tile(j.images, j.P, (long long)blockIdx.x);
    __syncthreads();
    const SegmentImage p = j.images[which];
    const int tile = (int)((long long)blockIdx.x - p.tile_off), tiles_x = (p.w + T - 1) / T;
    const int X0 = (tile % tiles_x) * T, Y0 = (tile / tiles_x) * T;
    for (int idx = tid; idx < ROWS * S; idx += THREADS) {
        const int ly = idx / S, c = idx - ly * S;
        const int Y = Y0 + ly, X = X0 - 1 + c;
        val[idx] = (Y < p.h && X >= 0 && X < p.w) ? ld_dt(p.map, (size_t)Y * p.w + X, j.dt) : NAN;
    }
    const double thr = segment_state(p, j.scratch)->thr;
    __syncthreads();
    const int tx = tid % T, ty = tid / T;
    const float* at = val + ty * S + tx + 1;
    const float v = *at;
    const bool valid = segment_valid(v, j.depth_space);
    int bits = 0;
    if (valid) {
        const float e = at[1], s = at[S], se = at[S + 1], sw = at[S - 1];
        if (segment_valid(e, j.depth_space) && segment_linked(v, e, j.depth_space, j.step, thr)) bits |= SEGMENT_E;
        if (segment_valid(s, j.depth_space) && segment_linked(v, s, j.depth_space, j.step, thr)) bits |= SEGMENT_S;
        if (j.conn8) {
            if (segment_valid(se, j.depth_space) && segment_linked(v, se, j.depth_space, j.step, thr)) bits |= SEGMENT_SE;
            if (segment_valid(sw, j.depth_space) && segment_linked(v, sw, j.depth_space, j.step, thr)) bits |= SEGMENT_SW;
        }
    }
    lab[tid] = valid ? tid : -1;
    __syncthreads();
    if ((bits & SEGMENT_E) && tx < T - 1) segment_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, tid, tid + 1);
    if ((bits & SEGMENT_S) && ty < T - 1) segment_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, tid, tid + T);
    if ((bits & SEGMENT_SE) && tx < T - 1 && ty < T - 1) segment_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, tid, tid + T + 1);
    if ((bits & SEGMENT_SW) && tx > 0 && ty < T - 1) segment_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, tid, tid + T - 1);
    __syncthreads();
    const int X = X0 + tx, Y = Y0 + ty;
    if (X >= p.w || Y >= p.h) return;
    const size_t i = (size_t)Y * p.w + X;
    int parent = -1;
    if (valid) {
        const int r = segment_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, tid);  // (raster order in the tile is raster order in the image: the lowest index either way)
        parent = (Y0 + r / T) * p.w + X0 + r % T;
    }
    p.labels[i] = parent;
    segment_aux(p, j.scratch)[i] = 0;
    segment_links(p, j.scratch)[i] = (unsigned char)bits;
}

// (4) blockIdx.x = a tile of the call; threads 0 .. 31 its right column, 32 .. 63 its last row, 64 .. 95 its left column (a corner node once)
__global__ __launch_bounds__(128) void segment_merge_kernel(SegmentJob j) {
    constexpr int T = SEGMENT_TILE;
    __shared__ int which;
    const int tid = (int)threadIdx.x;
    if (tid == 0) which = pair_of_tile(j.images, j.P, (long long)blockIdx.x);
    __syncthreads();
    const SegmentImage p = j.images[which];
    const int tile = (int)((long long)blockIdx.x - p.tile_off), tiles_x = (p.w + T - 1) / T;
    const int k = tid & 31, side = tid >> 5;
    int lx, ly;
    if (side == 0) lx = T - 1, ly = k;
    else if (side == 1) lx = k, ly = T - 1;
    else lx = 0, ly = k;
    if (side == 3 || (side == 1 && lx == T - 1) || (side == 2 && ly == T - 1)) return;
    const int X = (tile % tiles_x) * T + lx, Y = (tile / tiles_x) * T + ly;
    if (X >= p.w || Y >= p.h) return;
    const int i = Y * p.w + X;
    const int bits = segment_links(p, j.scratch)[i];  // (a set bit: the neighbour is a valid node of the image)
    const bool right = lx == T - 1, below = ly == T - 1, left = lx == 0;
    if ((bits & SEGMENT_E) && right) segment_union<__HIP_MEMORY_SCOPE_AGENT>(p.labels, i, i + 1);
    if ((bits & SEGMENT_S) && below) segment_union<__HIP_MEMORY_SCOPE_AGENT>(p.labels, i, i + p.w);
    if ((bits & SEGMENT_SE) && (right || below)) segment_union<__HIP_MEMORY_SCOPE_AGENT>(p.labels, i, i + p.w + 1);
    if ((bits & SEGMENT_SW) && (left || below)) segment_union<__HIP_MEMORY_SCOPE_AGENT>(p.labels, i, i + p.w - 1);
}

// whether every lane of the wave that has a key (key >= 0) has the same one; all 64 lanes call it
__device__ __forceinline__ bool segment_wave_uniform(int key, unsigned long long& have) {
    have = __ballot(key >= 0);
    if (have == 0) return false;
    const int first = __shfl(key, __ffsll((long long)have) - 1);
    return __ballot(key >= 0 && key == first) == have;
}

// (5) blockIdx.y = image, blockIdx.x = 256 nodes in raster order. A wave whose nodes share one root adds its count once (a large region puts
// thousands of adds on one address otherwise)
__global__ __launch_bounds__(256) void segment_flatten_kernel(SegmentJob j) {
    const SegmentImage p = j.images[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (i < (size_t)p.h * p.w) {
        r = p.labels[i];
        if (r >= 0) {
            for (int q; (q = p.labels[r]) != r;) r = q;
            p.labels[i] = r;
        }
    }
    int* aux = segment_aux(p, j.scratch);
    unsigned long long have;
    if (segment_wave_uniform(r, have)) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)have) - 1) atomicAdd(aux + r, __popcll(have));
    } else if (r >= 0) {
        atomicAdd(aux + r, 1);
    }
}

__device__ __forceinline__ bool segment_kept_root(const SegmentImage& p, const int* aux, size_t i, int min_area) {
    return i < (size_t)p.h * p.w && p.labels[i] == (int)i && aux[i] >= min_area;
}

// (6) the kept roots of every block of 256 nodes (a block past the image does nothing: the grid's x extent is that of the largest image)
__global__ __launch_bounds__(256) void segment_flag_kernel(SegmentJob j) {
    const SegmentImage p = j.images[blockIdx.y];
    if ((size_t)blockIdx.x * 256 >= (size_t)p.h * p.w) return;
    unsigned total;
    block_rank(segment_kept_root(p, segment_aux(p, j.scratch), (size_t)blockIdx.x * 256 + threadIdx.x, j.min_area) ? 1 : 0, total);
    if (threadIdx.x == 0) segment_bcnt(p, j.scratch)[blockIdx.x] = total;
}

// (7) block counts -> exclusive offsets in place and the image's total -> counts; blockIdx.x = image (mesh_scan_kernel's scheme)
__global__ __launch_bounds__(256) void segment_scan_kernel(SegmentJob j) {
    const SegmentImage p = j.images[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n = (unsigned)(((size_t)p.h * p.w + 255) / 256);
    unsigned* cnt = segment_bcnt(p, j.scratch);
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
    if (threadIdx.x == 0) j.counts[blockIdx.x] = (int)carry;
}

// (8) a kept root -> its region's row (area, first, neutral bbox / vrange / sum_q); aux: old root -> region, -1 for a dropped root
__global__ __launch_bounds__(256) void segment_scatter_kernel(SegmentJob j) {
    const SegmentImage p = j.images[blockIdx.y];
    if ((size_t)blockIdx.x * 256 >= (size_t)p.h * p.w) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int* aux = segment_aux(p, j.scratch);
    const bool keep = segment_kept_root(p, aux, i, j.min_area);
    unsigned total;
    const unsigned rank = block_rank(keep ? 1 : 0, total);
    if (keep) {
        const unsigned id = segment_bcnt(p, j.scratch)[blockIdx.x] + rank;
        const size_t g = (size_t)p.region_off + id;
        j.area[g] = aux[i];
        j.first[g] = (int)i;
        j.bbox[4 * g] = 0x7fffffff, j.bbox[4 * g + 1] = 0x7fffffff, j.bbox[4 * g + 2] = -1, j.bbox[4 * g + 3] = -1;
        ((unsigned*)j.vrange)[2 * g] = 0xffffffffu, ((unsigned*)j.vrange)[2 * g + 1] = 0u;
        j.sum_q[g] = 0;
        aux[i] = (int)id;
    } else if (i < (size_t)p.h * p.w && p.labels[i] == (int)i) {
        aux[i] = -1;
    }
}

// (9) labels and the order-independent statistics. A wave whose labelled nodes share one region reduces first and issues its seven atomics once.
__global__ __launch_bounds__(256) void segment_relabel_kernel(SegmentJob j) {
#pragma clang fp contract(off)
    const SegmentImage p = j.images[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int id = -1, x = 0, y = 0;
    unsigned vo = 0;
    long long q = 0;
    if (i < (size_t)p.h * p.w) {
        const int r = p.labels[i];
        if (r >= 0) id = segment_aux(p, j.scratch)[r];
        p.labels[i] = id;
        if (id >= 0) {
            const SegmentState st = *segment_state(p, j.scratch);
            const float v = ld_dt(p.map, i, j.dt);
            y = (int)(i / (unsigned)p.w), x = (int)(i - (size_t)y * p.w);
            vo = f2ord(v);
            if (st.hi > st.lo) q = (long long)floor(((double)v - st.lo) / (st.hi - st.lo) * 16777216.0 + 0.5);
        }
    }
    const bool act = id >= 0;
    int x0 = act ? x : 0x7fffffff, y0 = act ? y : 0x7fffffff, x1 = act ? x : -1, y1 = act ? y : -1;
    unsigned vlo = act ? vo : 0xffffffffu, vhi = act ? vo : 0u;
    unsigned long long have;
    const bool uniform = segment_wave_uniform(id, have);
    bool issue = act;
    if (uniform) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            x0 = min(x0, __shfl_xor(x0, o)), y0 = min(y0, __shfl_xor(y0, o));
            x1 = max(x1, __shfl_xor(x1, o)), y1 = max(y1, __shfl_xor(y1, o));
            vlo = min(vlo, __shfl_xor(vlo, o)), vhi = max(vhi, __shfl_xor(vhi, o));
            q += __shfl_xor(q, o);
        }
        issue = (int)(threadIdx.x & 63) == __ffsll((long long)have) - 1;
    }
    if (!issue) return;
    const size_t g = (size_t)p.region_off + id;
    atomicMin(j.bbox + 4 * g, x0), atomicMin(j.bbox + 4 * g + 1, y0), atomicMax(j.bbox + 4 * g + 2, x1), atomicMax(j.bbox + 4 * g + 3, y1);
    atomicMin((unsigned*)j.vrange + 2 * g, vlo), atomicMax((unsigned*)j.vrange + 2 * g + 1, vhi);
    atomicAdd((unsigned long long*)j.sum_q + g, (unsigned long long)q);
}

// (10) blockIdx.y = image: the ordered keys of its K regions -> fp32
__global__ __launch_bounds__(256) void segment_finish_kernel(SegmentJob j) {
    const SegmentImage p = j.images[blockIdx.y];
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)j.counts[blockIdx.y]) return;
    unsigned* u = (unsigned*)j.vrange + 2 * ((size_t)p.region_off + r);
    const float lo = ord2f(u[0]), hi = ord2f(u[1]);
    u[0] = __float_as_uint(lo), u[1] = __float_as_uint(hi);
}

// label -> BGR: a fixed integer hash (two multiply-xorshift rounds), every channel at least 32 so that no region is black; -1: black
__global__ __launch_bounds__(256) void segment_colors_kernel(const SegmentImage* __restrict__ images, unsigned char* __restrict__ colors) {
    const SegmentImage p = images[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.h * p.w) return;
    const int id = p.labels[i];
    unsigned h = 0u;
    if (id >= 0) {
        h = ((unsigned)id + 1u) * 2654435761u;
        h ^= h >> 15;
        h *= 2246822519u;
        h ^= h >> 13;
        h |= 0x202020u;
    }
    unsigned char* o = colors + ((size_t)p.pixel_off + i) * 3;
    o[0] = (unsigned char)(h & 255u), o[1] = (unsigned char)((h >> 8) & 255u), o[2] = (unsigned char)((h >> 16) & 255u);
}

// pick lookup: one thread a pick {image, node or region}; anything out of range selects nothing
__global__ __launch_bounds__(256) void segment_pick_kernel(const SegmentPhoto* __restrict__ photos, int P, const int* __restrict__ picks, int num_picks, int by_label,
                                                           unsigned char* __restrict__ selected) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= num_picks) return;
    const int k = picks[2 * t], v = picks[2 * t + 1];
    if (k < 0 || k >= P || v < 0) return;
    const SegmentPhoto p = photos[k];
    int id = v;
    if (!by_label) {
        if ((long long)v >= (long long)p.h * p.w) return;
        id = p.labels[v];
    }
    if (id >= 0 && id < p.regions) selected[p.region_off + id] = 1;
}

// cutout (one photo per blockIdx.y): photo pixel (Y, X) belongs to node ((Y h) / H, (X w) / W), integers throughout; mask = 255 where the node's region
// is selected, flipped by invert; BGRA = (BGR AND mask, mask). Four consecutive pixels of a row per thread: 12 BGR bytes in (one dwordx3 load where the
// address allows), 16 BGRA + 4 mask bytes out (dwordx4 + dword stores), as mask_cutout_kernel; the photo is read through its pitch.
__global__ __launch_bounds__(256) void segment_cutout_kernel(const SegmentPhoto* __restrict__ photos, const unsigned char* __restrict__ selected, int invert) {
    const SegmentPhoto p = photos[blockIdx.y];
    const int gpr = (p.W + MASK_PX - 1) / MASK_PX;  // groups per row
    const size_t groups = (size_t)gpr * p.H;
    const unsigned char* sel = selected + p.region_off;
    for (size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (size_t)gridDim.x * 256) {
        const int Y = (int)(gi / (unsigned)gpr), X = (int)(gi - (size_t)Y * gpr) * MASK_PX;
        const int cnt = p.W - X < MASK_PX ? p.W - X : MASK_PX;
        const unsigned char* in = p.photo + (long long)Y * p.pitch + 3LL * X;
        unsigned wd[3] = {0u, 0u, 0u};
        if (cnt == MASK_PX && ((uintptr_t)in & 3) == 0) {
            const Bytes12 v = *(const Bytes12*)in;
            wd[0] = v.w0, wd[1] = v.w1, wd[2] = v.w2;
        } else {
            for (int k = 0; k < cnt * 3; ++k) wd[k >> 2] |= (unsigned)in[k] << (8 * (k & 3));
        }
        const int* row = p.labels + (size_t)(((long long)Y * p.h) / p.H) * p.w;
        unsigned mword = 0u, px[MASK_PX];
#pragma unroll
        for (int k = 0; k < MASK_PX; ++k) {
            px[k] = 0u;
            if (k >= cnt) continue;
            const int id = row[((long long)(X + k) * p.w) / p.W];
            const bool on = (id >= 0 && sel[id] != 0) != (invert != 0);
            const unsigned m = on ? 255u : 0u;
            mword |= m << (8 * k);
            unsigned bgr = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) bgr |= ((wd[(3 * k + ch) >> 2] >> (8 * ((3 * k + ch) & 3))) & 255u) << (8 * ch);
            px[k] = (on ? bgr : 0u) | m << 24;
        }
        const size_t at = (size_t)Y * p.W + X;
        unsigned char* bo = p.bgra + at * 4;
        unsigned char* mo = p.mask + at;
        if (cnt == MASK_PX && ((uintptr_t)bo & 15) == 0) {
            *(uint4*)bo = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
            for (int k = 0; k < cnt; ++k) *(unsigned*)(bo + 4 * k) = px[k];  // (the BGRA output is 4-byte aligned: checked by the entry point)
        }
        if (cnt == MASK_PX && ((uintptr_t)mo & 3) == 0) {
            *(unsigned*)mo = mword;
        } else {
            for (int k = 0; k < cnt; ++k) mo[k] = (unsigned char)(mword >> (8 * k));
        }
    }
}

}  // namespace

int mdpt_launch_segment(const SegmentJob& j, hipStream_t stream) {
    if (j.P <= 0 || j.P > 65535 || j.min_area < 1 || j.max_pixels == 0 || j.max_pixels >= ((size_t)1 << 31) || j.total_tiles == 0 || j.total_tiles >= ((size_t)1 << 31))
        return (int)hipErrorInvalidValue;
    const dim3 nodes((unsigned)((j.max_pixels + 255) / 256), j.P), tiles((unsigned)j.total_tiles);
    post_launch("segment_minmax_kernel", segment_minmax_kernel, dim3(SEGMENT_PARTS, j.P), dim3(256), stream, j.images, j.dt, j.depth_space, j.scratch);
    post_launch("segment_state_kernel", segment_state_kernel, dim3(j.P), dim3(64), stream, j);
    post_launch("segment_tile_kernel", segment_tile_kernel, tiles, dim3(SEGMENT_TILE * SEGMENT_TILE), stream, j);
    post_launch("segment_merge_kernel", segment_merge_kernel, tiles, dim3(128), stream, j);
    post_launch("segment_flatten_kernel", segment_flatten_kernel, nodes, dim3(256), stream, j);
    post_launch("segment_flag_kernel", segment_flag_kernel, nodes, dim3(256), stream, j);
    post_launch("segment_scan_kernel", segment_scan_kernel, dim3(j.P), dim3(256), stream, j);
    post_launch("segment_scatter_kernel", segment_scatter_kernel, nodes, dim3(256), stream, j);
    post_launch("segment_relabel_kernel", segment_relabel_kernel, nodes, dim3(256), stream, j);
    post_launch("segment_finish_kernel", segment_finish_kernel, dim3((unsigned)((j.max_regions + 255) / 256 > 0 ? (j.max_regions + 255) / 256 : 1), j.P), dim3(256), stream, j);
    return (int)hipGetLastError();
}

int mdpt_launch_segment_colors(const SegmentImage* images, int P, size_t max_pixels, unsigned char* colors, hipStream_t stream) {
    if (P <= 0 || P > 65535 || max_pixels == 0 || max_pixels >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
    post_launch("segment_colors_kernel", segment_colors_kernel, dim3((unsigned)((max_pixels + 255) / 256), P), dim3(256), stream, images, colors);
    return (int)hipGetLastError();
}

int mdpt_launch_segment_cutout(const SegmentPhoto* photos, int P, const int* picks, int num_picks, int by_label, unsigned char* selected, int invert,
                               size_t max_groups, hipStream_t stream) {
    if (P <= 0 || P > 65535 || num_picks < 0 || max_groups == 0) return (int)hipErrorInvalidValue;
    if (num_picks > 0)
        post_launch("segment_pick_kernel", segment_pick_kernel, dim3((unsigned)((num_picks + 255) / 256)), dim3(256), stream, photos, P, picks, num_picks, by_label, selected);
    const size_t g = (max_groups + 255) / 256;
    post_launch("segment_cutout_kernel", segment_cutout_kernel, dim3(g > 2048 ? 2048 : (unsigned)g, P), dim3(256), stream, photos, selected, invert);
    return (int)hipGetLastError();
}
