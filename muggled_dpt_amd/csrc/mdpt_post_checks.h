// libmdpt: the argument checks that the mdpt_post_*.cpp files share, each rule and its message once (words that differ between entry points are arguments).
// Plain host functions that return 0 or what fail() returned, for CHK(). tests/test_post_refusals_cpu.py pins every message and the order of the checks.
#pragma once
#include "mdpt_internal.h"
#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

// MDPT_SAME_RECORD(pub, kern, size, field...): a record of include/mdpt.h and its twin of mdpt_kernels.h have one size and every listed field at one offset
// (list them all). The recursion only walks the list: 27 rescans, enough for 27 fields.
#define MDPT_RESCAN1(...) __VA_ARGS__
#define MDPT_RESCAN3(...) MDPT_RESCAN1(MDPT_RESCAN1(MDPT_RESCAN1(__VA_ARGS__)))
#define MDPT_RESCAN27(...) MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(MDPT_RESCAN3(__VA_ARGS__)))))))))
#define MDPT_PARENS ()
#define MDPT_SAME_FIELDS(pub, kern, field, ...) &&offsetof(pub, field) == offsetof(kern, field) __VA_OPT__(MDPT_SAME_FIELDS_AGAIN MDPT_PARENS(pub, kern, __VA_ARGS__))
#define MDPT_SAME_FIELDS_AGAIN() MDPT_SAME_FIELDS
#define MDPT_SAME_RECORD(pub, kern, size, ...)                                                                         \
    static_assert(sizeof(pub) == size && sizeof(kern) == size MDPT_RESCAN27(MDPT_SAME_FIELDS(pub, kern, __VA_ARGS__)), \
                  #pub " of include/mdpt.h is " #kern " of mdpt_kernels.h, field by field")

namespace mdpt {

inline size_t dtype_bytes(int dt) { return dt == MDPT_DTYPE_F32 ? 4 : 2; }
inline bool aligned_to_element(const void* p, int dt) { return ((uintptr_t)p & (dtype_bytes(dt) - 1)) == 0; }
// a uint8 / map count as the ih x iw of one table entry (1 x count)
inline bool count_as_hw(size_t count, int& ih, int& iw) {
    if (count == 0 || count > (size_t)INT32_MAX) return false;
    ih = 1, iw = (int)count;
    return true;
}
inline int check_batch(int32_t B) { return B <= 0 || B > 65535 ? fail(MDPT_E_INVALID, "bad batch %d", B) : 0; }
inline int check_batch_hw(int32_t B, int32_t H, int32_t W) { return B <= 0 || B > 65535 || H <= 0 || W <= 0 ? fail(MDPT_E_INVALID, "bad size %dx%dx%d", B, H, W) : 0; }
inline int check_images(const void* const* in, const int32_t* hw, int32_t B, const char* what) {
    CHK(check_batch(B));
    for (int i = 0; i < B; ++i) {
        if (in && !in[i]) return fail(MDPT_E_INVALID, "null argument (%s %d)", what, i);
        if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0) return fail(MDPT_E_INVALID, "bad %s size %dx%d (image %d)", what, hw[2 * i], hw[2 * i + 1], i);
    }
    return 0;
}

// the records (pairs, frames, images) of one call: `name` = "" or the argument's name as "n = "
inline int check_count(const char* what, const char* name, int32_t n) { return n <= 0 || n > 65535 ? fail(MDPT_E_INVALID, "bad %s count %s%d (1 .. 65535 per call)", what, name, n) : 0; }
// sizes are int32 and so are pixel indices: H W < 2^31 (`unit` = "" or " pixels"); a photo, a map
inline int check_below_2_31(const char* what, int32_t H, int32_t W, const char* unit, int p) {
    return (size_t)H * W >= ((size_t)1 << 31) ? fail(MDPT_E_INVALID, "a %s of %dx%d is too large (H W < 2^31%s, pair %d)", what, H, W, unit, p) : 0;
}
inline int check_photo_size(int32_t H, int32_t W, int p) {
    if (H <= 0 || W <= 0) return fail(MDPT_E_INVALID, "bad photo size %dx%d (pair %d)", H, W, p);
    return check_below_2_31("photo", H, W, " pixels", p);
}
inline int check_map_size(int32_t h, int32_t w, int p) {
    return h <= 0 || w <= 0 || (size_t)h * w >= ((size_t)1 << 31) ? fail(MDPT_E_INVALID, "bad map size %dx%d (pair %d; h w < 2^31)", h, w, p) : 0;
}
inline int check_map_aligned(const void* map, int dt, int p) { return aligned_to_element(map, dt) ? 0 : fail(MDPT_E_INVALID, "misaligned map (pair %d: it needs its element)", p); }
inline int check_pitch(int64_t pitch, int32_t W, int p) {
    return pitch < 3 * (int64_t)W ? fail(MDPT_E_INVALID, "a row pitch of %lld bytes is less than the %d pixels of a row (pair %d)", (long long)pitch, W, p) : 0;
}

// the scratch regions of a call's records: each aligned to 8 bytes and inside the scratch_bytes (`given`: the entry point's end of the message), no two overlapping
struct ScratchRegions {
    std::vector<std::pair<size_t, size_t>> regions;
    int add(int p, int64_t off, size_t need, size_t scratch_bytes, const char* given) {
        if (off < 0 || (off & 7) != 0 || (size_t)off > scratch_bytes || scratch_bytes - (size_t)off < need)
            return fail(MDPT_E_INVALID, "the scratch region of pair %d (offset %lld, %zu bytes) is misaligned or outside the %zu bytes %s", p, (long long)off, need, scratch_bytes, given);
        regions.emplace_back((size_t)off, (size_t)off + need);
        return 0;
    }
    int finish() {
        std::sort(regions.begin(), regions.end());
        for (size_t k = 1; k < regions.size(); ++k)
            if (regions[k].first < regions[k - 1].second) return fail(MDPT_E_INVALID, "the scratch regions of two pairs overlap (at byte %zu)", regions[k].first);
        return 0;
    }
};
// tile_off / gtile_off of record p = the tiles (side x side `units`) of the records before it
inline int check_running_offset(const char* name, int64_t off, size_t running, int p, int side, const char* units) {
    if (off == (int64_t)running) return 0;
    return fail(MDPT_E_INVALID, "%s %lld of pair %d is not the %zu tiles of %dx%d %s of the pairs before it", name, (long long)off, p, running, side, side, units);
}
// an optional per-record pointer that `got` of n records have: all of them, or none
inline int check_all_or_none(int got, int n, const char* what, const char* has, const char* note) {
    return got != 0 && got != n ? fail(MDPT_E_INVALID, "%s is null in %d of %d records: every pair has %s, or none%s", what, n - got, n, has, note) : 0;
}
inline int check_scratch(const char* what, size_t have, size_t need, const char* query) {
    return have < need ? fail(MDPT_E_INVALID, "%s scratch of %zu bytes, %zu needed (%s)", what, have, need, query) : 0;
}

// ---- what mdpt_post_normals and mdpt_post_shadows share (a ShadowsPair is a NormalsPair plus the grid): the scalars, the record checks, the job's common fields
struct RelightArgs {
    int32_t n, dtype, space; double min_depth, max_depth, edge_ratio; const void* lights_dev; int32_t num_lights; double ambient, diffuse, specular; int32_t shininess_log2;
};

// the *_scratch_bytes query, and the entry point's size check: photo (and working grid) sizes positive, fewer than 2^31 pixels (nodes); *bytes = P headers
template <class Pair> int check_relight_sizes(const Pair* pairs, int32_t P, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    if (!pairs) return fail(MDPT_E_INVALID, "null argument (records)");
    CHK(check_count("pair", "n = ", P));
    for (int p = 0; p < P; ++p) {
        CHK(check_photo_size(pairs[p].H, pairs[p].W, p));
        if constexpr (std::is_same_v<Pair, mdpt_shadows_pair>)
            if (pairs[p].gh <= 0 || pairs[p].gw <= 0 || (size_t)pairs[p].gh * pairs[p].gw >= ((size_t)1 << 31))
                return fail(MDPT_E_INVALID, "bad working grid %dx%d (pair %d; positive, gh gw < 2^31 nodes)", pairs[p].gh, pairs[p].gw, p);
    }
    *bytes = (size_t)P * NORMALS_HEADER_BYTES;
    return 0;
}

// the scalars, in their order; `feature` = "normals" / "shadows"
template <class Pair> int check_relight_scalars(const char* feature, const Pair* records_host, const void* records_dev, const void* scratch, const RelightArgs& a) {
    if (!records_host || !records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_host, records_dev or scratch)");
    if (!tensor_dtype_ok(a.dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", a.dtype);
    if (a.space != MDPT_ALIGN_INVERSE && a.space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown %s space %d", feature, a.space);
    size_t packed;
    CHK(check_relight_sizes(records_host, a.n, &packed));
    if (a.space == MDPT_ALIGN_INVERSE && !(a.min_depth > 0.0 && a.min_depth < a.max_depth && a.max_depth <= 1e300))
        return fail(MDPT_E_INVALID, "need 0 < min_depth < max_depth, finite, in inverse space, got %g, %g", a.min_depth, a.max_depth);
    if (!(a.edge_ratio >= 1.0)) return fail(MDPT_E_INVALID, "edge_ratio must be >= 1 (inf: always the central difference), got %g", a.edge_ratio);
    if (a.num_lights < 0 || a.num_lights > NORMALS_MAX_LIGHTS) return fail(MDPT_E_INVALID, "bad light count num_lights = %d (0 .. %d per call)", a.num_lights, NORMALS_MAX_LIGHTS);
    if (!(a.ambient >= 0.0 && a.ambient <= 1e300 && a.diffuse >= 0.0 && a.diffuse <= 1e300 && a.specular >= 0.0 && a.specular <= 1e300))
        return fail(MDPT_E_INVALID, "ambient, diffuse and specular must be finite and >= 0, got %g, %g, %g", a.ambient, a.diffuse, a.specular);
    if (a.shininess_log2 < 0 || a.shininess_log2 > 10) return fail(MDPT_E_INVALID, "shininess_log2 %d: the number of squarings must be 0 .. 10", a.shininess_log2);
    return 0;
}
inline int check_relight_pointers(const void* records_dev, const void* scratch, const void* lights_dev) {
    if ((((uintptr_t)records_dev | (uintptr_t)scratch | (uintptr_t)lights_dev) & 7) == 0) return 0;
    return fail(MDPT_E_INVALID, "misaligned pointer (the table, the lights and the scratch need 8 bytes)");
}

// record p: its map, the photo's pitch, the difference step, the camera scales, its fp32 outputs (`outputs`: their addresses or-ed, named by `what`), its
// scratch header and its photo tiles, which it adds to `tiles`
template <class Pair>
int check_relight_record(const Pair& q, int p, int dtype, uintptr_t outputs, const char* what, size_t scratch_bytes, const char* given, ScratchRegions& regions, size_t& tiles) {
    if (!q.map) return fail(MDPT_E_INVALID, "null map (pair %d)", p);
    CHK(check_map_aligned(q.map, dtype, p));
    CHK(check_map_size(q.h, q.w, p));
    if (q.photo) CHK(check_pitch(q.pitch, q.W, p));
    if (q.step < 1 || q.step > NORMALS_MAX_STEP) return fail(MDPT_E_INVALID, "step %d of pair %d: the difference step must be 1 .. %d photo pixels", q.step, p, NORMALS_MAX_STEP);
    if (!(q.kx > 0.0 && q.kx <= 1e300 && q.ky > 0.0 && q.ky <= 1e300)) return fail(MDPT_E_INVALID, "the camera scales kx, ky of pair %d must be finite and > 0, got %g, %g", p, q.kx, q.ky);
    if ((outputs & 3) != 0) return fail(MDPT_E_INVALID, "misaligned %s (pair %d: fp32)", what, p);
    CHK(regions.add(p, q.scratch_off, NORMALS_HEADER_BYTES, scratch_bytes, given));
    CHK(check_running_offset("tile_off", q.tile_off, tiles, p, NORMALS_TILE, "pixels"));
    tiles += normals_pair_tiles((size_t)q.H, (size_t)q.W);
    return 0;
}

// the fields NormalsJob and ShadowsJob have in common (V = the lights the kernels read: 0 when nothing lit is asked for)
template <class Job> void fill_relight_job(Job& j, const void* records_dev, const RelightArgs& a, int V, void* scratch, size_t tiles) {
    j.pairs = (decltype(j.pairs))records_dev;
    j.P = a.n, j.dt = a.dtype, j.depth_space = a.space == MDPT_ALIGN_DEPTH, j.central_only = a.edge_ratio > 1e300, j.V = V;
    j.shininess_log2 = a.shininess_log2;
    if (!j.depth_space) j.depth_a = 1.0 / a.max_depth, j.depth_b = 1.0 / a.min_depth - 1.0 / a.max_depth;
    j.edge_ratio = a.edge_ratio, j.ambient = a.ambient, j.diffuse = a.diffuse, j.specular = a.specular;
    j.lights = (const double*)a.lights_dev, j.scratch = (char*)scratch, j.total_tiles = tiles;
}

}  // namespace mdpt
