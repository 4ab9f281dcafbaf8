// libmdpt: the mdpt_post_* entry points that re-render a photo by its depth (see mdpt_post.cpp): refocus, normals, shadows.
#include "mdpt_post_checks.h"

extern "C" {

// ---- synthetic depth of field (per-pixel defocus, occlusion-aware gather; not in the reference)
MDPT_SAME_RECORD(mdpt_refocus_pair, RefocusPair, 64, map, h, w, photo, pitch, H, W, out, scratch_off, tile_off);
static_assert(MDPT_REFOCUS_MAX_RADIUS == REFOCUS_MAX_RADIUS && MDPT_REFOCUS_TILE == REFOCUS_TILE, "the refocus limits of include/mdpt.h are those of mdpt_kernels.h");

// the *_scratch_bytes query, and the entry point's size check: photo sizes positive, H W < 2^31; *bytes = the scratch of the P regions laid end to end
static int check_refocus_sizes(const mdpt_refocus_pair* pairs, int32_t P, int32_t max_radius, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    if (!pairs) return fail(MDPT_E_INVALID, "null argument (records)");
    CHK(check_count("pair", "n = ", P));
    if (max_radius < 0 || max_radius > REFOCUS_MAX_RADIUS) return fail(MDPT_E_INVALID, "max_radius %d: the blur radius limit must be 0 .. %d pixels", max_radius, REFOCUS_MAX_RADIUS);
    size_t total = 0;
    for (int p = 0; p < P; ++p) {
        CHK(check_photo_size(pairs[p].H, pairs[p].W, p));
        total += refocus_pair_scratch_bytes((size_t)pairs[p].H, (size_t)pairs[p].W);
    }
    *bytes = total;
    return 0;
}

int mdpt_post_refocus_scratch_bytes(const mdpt_refocus_pair* records_host, int32_t n, int32_t max_radius, size_t* bytes) {
    return check_refocus_sizes(records_host, n, max_radius, bytes);
}

int mdpt_post_refocus(const mdpt_refocus_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double focus,
                      const double* focus_xy, double aperture, double focus_range, int32_t max_radius, void* scratch, size_t scratch_bytes, void* radius_out,
                      void* defocus_out, void* stream) {
    if (!records_host || !records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_host, records_dev or scratch)");
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown refocus space %d", space);
    size_t packed;
    CHK(check_refocus_sizes(records_host, n, max_radius, &packed));
    if (!(aperture >= 0.0) || aperture > 1e300) return fail(MDPT_E_INVALID, "aperture must be finite and >= 0 (pixels per unit of defocus), got %g", aperture);
    if (!(focus_range >= 0.0) || focus_range > 1e300) return fail(MDPT_E_INVALID, "focus_range must be finite and >= 0, got %g", focus_range);
    if (focus_xy) {
        if (!(focus_xy[0] >= 0.0 && focus_xy[0] <= 1.0 && focus_xy[1] >= 0.0 && focus_xy[1] <= 1.0))
            return fail(MDPT_E_INVALID, "focus_xy must lie in [0, 1]^2, got (%g, %g)", focus_xy[0], focus_xy[1]);
    } else if (space == MDPT_ALIGN_INVERSE ? !(focus >= 0.0 && focus <= 1.0) : (!(focus > 0.0) || focus > 1e300)) {
        return fail(MDPT_E_INVALID, "focus %g is outside its domain (inverse space: 0 .. 1 of the map's range; depth space: a finite depth > 0)", focus);
    }
    if ((((uintptr_t)records_dev | (uintptr_t)scratch) & 7) != 0 || ((uintptr_t)defocus_out & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table and the scratch need 8 bytes, defocus_out 4)");
    size_t max_pixels = 0, tiles = 0;
    int with_out = 0;
    ScratchRegions regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_refocus_pair& q = records_host[p];
        if (!q.map || !q.photo) return fail(MDPT_E_INVALID, "null map or photo (pair %d)", p);
        CHK(check_map_aligned(q.map, dtype, p));
        CHK(check_map_size(q.h, q.w, p));
        CHK(check_pitch(q.pitch, q.W, p));
        CHK(regions.add(p, q.scratch_off, refocus_pair_scratch_bytes((size_t)q.H, (size_t)q.W), scratch_bytes, "of scratch given (mdpt_post_refocus_scratch_bytes)"));
        CHK(check_running_offset("tile_off", q.tile_off, tiles, p, REFOCUS_TILE, "pixels"));
        tiles += refocus_pair_tiles((size_t)q.H, (size_t)q.W);
        max_pixels = std::max(max_pixels, (size_t)q.H * q.W);
        with_out += q.out != nullptr;
    }
    CHK(check_all_or_none(with_out, n, "out", "an output", " (the preparation alone)"));
    if (!with_out && !radius_out && !defocus_out) return fail(MDPT_E_INVALID, "null argument: no record has an output and neither radius_out nor defocus_out is given");
    if (tiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu tiles: a call takes fewer than 2^31", tiles);
    CHK(regions.finish());
    RefocusJob j{};
    j.pairs = (const RefocusPair*)records_dev;
    j.P = n, j.dt = dtype, j.depth_space = space == MDPT_ALIGN_DEPTH, j.pointed = focus_xy != nullptr, j.max_radius = max_radius, j.gather = with_out != 0;
    j.focus = focus_xy ? 0.0 : (j.depth_space ? 1.0 / focus : focus);
    j.fx = focus_xy ? focus_xy[0] : 0.0, j.fy = focus_xy ? focus_xy[1] : 0.0;
    j.aperture = aperture, j.half_range = focus_range / 2.0;
    j.scratch = (char*)scratch, j.radius_out = (unsigned char*)radius_out, j.defocus_out = (float*)defocus_out;
    j.max_pixels = max_pixels, j.total_tiles = tiles;
    CHK(mdpt_launch_post_refocus(j, (hipStream_t)stream));
    return 0;
}

// ---- surface normals and relighting (edge-aware differences of the unprojected map, Lambert / Blinn-Phong mix; not in the reference)
MDPT_SAME_RECORD(mdpt_normals_pair, NormalsPair, 104, map, h, w, photo, pitch, H, W, normals, encoded, relit, scratch_off, tile_off, kx, ky, step, pad);
static_assert(MDPT_NORMALS_MAX_STEP == NORMALS_MAX_STEP && MDPT_NORMALS_TILE == NORMALS_TILE && MDPT_NORMALS_MAX_LIGHTS == NORMALS_MAX_LIGHTS,
              "the normals limits of include/mdpt.h are those of mdpt_kernels.h");

int mdpt_post_normals_scratch_bytes(const mdpt_normals_pair* records_host, int32_t n, size_t* bytes) { return check_relight_sizes(records_host, n, bytes); }

int mdpt_post_normals(const mdpt_normals_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double min_depth,
                      double max_depth, double edge_ratio, const void* lights_dev, int32_t num_lights, double ambient, double diffuse, double specular,
                      int32_t shininess_log2, void* scratch, size_t scratch_bytes, void* stream) {
    const RelightArgs a{n, dtype, space, min_depth, max_depth, edge_ratio, lights_dev, num_lights, ambient, diffuse, specular, shininess_log2};
    CHK(check_relight_scalars("normals", records_host, records_dev, scratch, a));
    CHK(check_relight_pointers(records_dev, scratch, lights_dev));
    size_t tiles = 0;
    int with_normals = 0, with_encoded = 0, with_relit = 0, with_photo = 0;
    ScratchRegions regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_normals_pair& q = records_host[p];
        CHK(check_relight_record(q, p, dtype, (uintptr_t)q.normals, "normals output", scratch_bytes, "of scratch given (mdpt_post_normals_scratch_bytes)", regions, tiles));
        with_normals += q.normals != nullptr, with_encoded += q.encoded != nullptr, with_relit += q.relit != nullptr, with_photo += q.photo != nullptr;
    }
    for (int got : {with_normals, with_encoded, with_relit}) CHK(check_all_or_none(got, n, "an output", "it", ""));
    if (!with_normals && !with_encoded && !with_relit) return fail(MDPT_E_INVALID, "null argument: no record has an output (normals, encoded or relit)");
    if (with_relit && (num_lights < 1 || !lights_dev)) return fail(MDPT_E_INVALID, "relit frames are asked for without lights (lights_dev null or num_lights = %d)", num_lights);
    CHK(check_all_or_none(with_photo, n, "photo", "a photo", " (white clay)"));
    if (tiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu tiles: a call takes fewer than 2^31", tiles);
    CHK(regions.finish());
    NormalsJob j{};
    fill_relight_job(j, records_dev, a, with_relit ? num_lights : 0, scratch, tiles);
    CHK(mdpt_launch_post_normals(j, (hipStream_t)stream));
    return 0;
}

// ---- cast shadows and ambient occlusion for the relighting (marches on a working grid, folded into the shading; not in the reference)
MDPT_SAME_RECORD(mdpt_shadows_pair, ShadowsPair, 120, map, h, w, photo, pitch, H, W, gh, gw, ao, vis, relit, scratch_off, tile_off, gtile_off, kx, ky, step, pad);
static_assert(MDPT_SHADOWS_MAX_REACH == SHADOWS_MAX_REACH && MDPT_SHADOWS_AO_DIRECTIONS == SHADOWS_AO_DIRECTIONS, "the shadow limits of include/mdpt.h are those of mdpt_kernels.h");

int mdpt_post_shadows_scratch_bytes(const mdpt_shadows_pair* records_host, int32_t n, size_t* bytes) { return check_relight_sizes(records_host, n, bytes); }

int mdpt_post_shadows(const mdpt_shadows_pair* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double min_depth,
                      double max_depth, double edge_ratio, const void* lights_dev, int32_t num_lights, double ambient, double diffuse, double specular,
                      int32_t shininess_log2, int32_t shadow_reach, double shadow_bias, double shadow_thickness, int32_t ao_reach, double ao_radius,
                      double ao_bias, double ao_strength, void* scratch, size_t scratch_bytes, void* stream) {
    const RelightArgs a{n, dtype, space, min_depth, max_depth, edge_ratio, lights_dev, num_lights, ambient, diffuse, specular, shininess_log2};
    CHK(check_relight_scalars("shadows", records_host, records_dev, scratch, a));
    if (shadow_reach < 0 || shadow_reach > SHADOWS_MAX_REACH) return fail(MDPT_E_INVALID, "shadow_reach %d: a shadow march takes 0 .. %d grid nodes", shadow_reach, SHADOWS_MAX_REACH);
    if (ao_reach < 0 || ao_reach > SHADOWS_MAX_REACH) return fail(MDPT_E_INVALID, "ao_reach %d: an occlusion direction takes 0 .. %d grid nodes", ao_reach, SHADOWS_MAX_REACH);
    if (!(shadow_bias >= 0.0 && shadow_bias < 1.0)) return fail(MDPT_E_INVALID, "shadow_bias must be in [0, 1), got %g", shadow_bias);
    if (!(shadow_thickness >= 0.0)) return fail(MDPT_E_INVALID, "shadow_thickness must be >= 0 (inf: an occluder of any thickness), got %g", shadow_thickness);
    if (!(ao_radius > 0.0 && ao_radius <= 1e300)) return fail(MDPT_E_INVALID, "ao_radius must be finite and > 0, got %g", ao_radius);
    if (!(ao_bias >= 0.0 && ao_bias <= 1e300 && ao_strength >= 0.0 && ao_strength <= 1e300))
        return fail(MDPT_E_INVALID, "ao_bias and ao_strength must be finite and >= 0, got %g, %g", ao_bias, ao_strength);
    CHK(check_relight_pointers(records_dev, scratch, lights_dev));
    size_t tiles = 0, gtiles = 0;
    int with_ao = 0, with_vis = 0, with_relit = 0, with_photo = 0;
    ScratchRegions regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_shadows_pair& q = records_host[p];
        CHK(check_relight_record(q, p, dtype, (uintptr_t)q.ao | (uintptr_t)q.vis, "ao or vis plane", scratch_bytes, "of scratch given (mdpt_post_shadows_scratch_bytes)", regions, tiles));
        CHK(check_running_offset("gtile_off", q.gtile_off, gtiles, p, NORMALS_TILE, "grid nodes"));
        gtiles += normals_pair_tiles((size_t)q.gh, (size_t)q.gw);
        with_ao += q.ao != nullptr, with_vis += q.vis != nullptr, with_relit += q.relit != nullptr, with_photo += q.photo != nullptr;
    }
    for (int got : {with_ao, with_vis, with_relit}) CHK(check_all_or_none(got, n, "an output", "it", ""));
    if (!with_ao && !with_vis && !with_relit) return fail(MDPT_E_INVALID, "null argument: no record has an output (ao, vis or relit)");
    if ((with_relit || with_vis) && (num_lights < 1 || !lights_dev))
        return fail(MDPT_E_INVALID, "vis planes or relit frames are asked for without lights (lights_dev null or num_lights = %d)", num_lights);
    const bool use_vis = shadow_reach > 0, use_ao = ao_reach > 0 && ao_strength > 0.0;
    if (with_relit && ((use_vis && !with_vis) || (use_ao && !with_ao)))
        return fail(MDPT_E_INVALID, "the shading needs a plane that no record has (vis with shadow_reach > 0, ao with ao_reach > 0 and ao_strength > 0)");
    CHK(check_all_or_none(with_photo, n, "photo", "a photo", " (white clay)"));
    if (tiles >= ((size_t)1 << 31) || gtiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu photo tiles, %zu grid tiles: a call takes fewer than 2^31 of each", tiles, gtiles);
    CHK(regions.finish());
    ShadowsJob j{};
    fill_relight_job(j, records_dev, a, (with_relit || with_vis) ? num_lights : 0, scratch, tiles);
    j.total_gtiles = gtiles, j.shadow_reach = shadow_reach, j.ao_reach = ao_reach, j.thick_inf = shadow_thickness > 1e300, j.use_vis = use_vis, j.use_ao = use_ao;
    j.planes = with_ao || with_vis, j.shade = with_relit != 0;
    j.shadow_bias = shadow_bias, j.shadow_thickness = shadow_thickness, j.ao_radius = ao_radius, j.ao_bias = ao_bias, j.ao_strength = ao_strength;
    CHK(mdpt_launch_post_shadows(j, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
