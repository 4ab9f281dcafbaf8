// libmdpt: the mdpt_post_* entry points of the depth mesh (see mdpt_post.cpp): mesh grid, mesh, render, hole filling.
#include "mdpt_post_checks.h"

extern "C" {

// ---- depth-to-mesh (3dviewer/mesh.js:184-200 grid, shaders.js:163-264 vertices, mesh.js:330-371 filtering, save_gltf.js:16-25 bounds)
static double js_round(double v) {  // Math.round: halves go toward +inf
    const double f = floor(v);
    return v - f >= 0.5 ? f + 1.0 : f;
}

int mdpt_post_mesh_grid(int32_t w, int32_t h, double target_faces, int32_t* nx, int32_t* ny) {
    if (!nx || !ny) return fail(MDPT_E_INVALID, "null argument");
    if (w <= 0 || h <= 0 || !(target_faces == target_faces)) return fail(MDPT_E_INVALID, "bad photo size %dx%d / face target %g", w, h, target_faces);
    const double t = target_faces > 2.0 ? target_faces : 2.0;
    const double tv = js_round(0.5 * t + sqrt(t));
    const double aspect = (double)w / (double)h;
    const double rx = sqrt(tv * aspect), ry = rx / aspect;
    const double fx = js_round(rx) > 2.0 ? js_round(rx) : 2.0, fy = js_round(ry) > 2.0 ? js_round(ry) : 2.0;
    if (fx * fy >= 2147483648.0) return fail(MDPT_E_INVALID, "a grid of %.0f x %.0f vertices is too large (the product must be below 2^31)", fx, fy);
    *nx = (int32_t)fx;
    *ny = (int32_t)fy;
    return 0;
}

// nx x ny vertices: sides of at least 2, fewer than 2^31 vertices and faces (counts are int32, face indices uint32)
static int check_mesh_grid(int32_t nx, int32_t ny) {
    if (nx < 2 || ny < 2) return fail(MDPT_E_INVALID, "a mesh grid needs sides of at least 2, got %dx%d", nx, ny);
    if ((size_t)nx * (size_t)ny >= ((size_t)1 << 31) || 2 * ((size_t)nx - 1) * ((size_t)ny - 1) >= ((size_t)1 << 31))
        return fail(MDPT_E_INVALID, "a grid of %dx%d vertices is too large (vertices and faces must each be fewer than 2^31)", nx, ny);
    return 0;
}

// the scratch of B images: the vertex map, the two lists of block counts, the ordered bounds - 4-byte words, in MeshJob's order
static size_t mesh_scratch_words(size_t B, int32_t nx, int32_t ny) {
    const size_t nv = (size_t)nx * ny, cells = ((size_t)nx - 1) * ((size_t)ny - 1);
    return B * (nv + mesh_blocks(nv) + mesh_blocks(cells) + 6);
}

int mdpt_post_mesh_scratch_bytes(int32_t B, int32_t nx, int32_t ny, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_batch(B));
    CHK(check_mesh_grid(nx, ny));
    *bytes = 4 * mesh_scratch_words((size_t)B, nx, ny);
    return 0;
}

int mdpt_post_mesh(const void* frames_bgra, int32_t B, int32_t H, int32_t W, int32_t nx, int32_t ny, const void* vertex_xy_f64, double a, double b,
                   double tan_half_fov, double x_scale, double y_scale, double edge_threshold, int32_t is_metric, int32_t mode, void* xyz_f32,
                   void* uv_f32, void* faces_u32, void* counts_i32, void* bounds_f32, void* scratch, size_t scratch_bytes, void* stream) {
    if (!frames_bgra || !xyz_f32 || !uv_f32 || !faces_u32 || !counts_i32 || !bounds_f32 || !scratch) return fail(MDPT_E_INVALID, "null argument");
    if (((uintptr_t)frames_bgra & 3) != 0) return fail(MDPT_E_INVALID, "the BGRA frames must be 4-byte aligned");
    CHK(check_batch_hw(B, H, W));
    CHK(check_mesh_grid(nx, ny));
    if (mode != MDPT_MESH_TRIANGLES && mode != MDPT_MESH_POINTS) return fail(MDPT_E_INVALID, "unknown mesh mode %d", mode);
    if (!(edge_threshold == edge_threshold)) return fail(MDPT_E_INVALID, "the edge threshold is not a number");
    CHK(check_scratch("mesh", scratch_bytes, 4 * mesh_scratch_words((size_t)B, nx, ny), "mdpt_post_mesh_scratch_bytes"));
    const size_t nv = (size_t)nx * ny, cells = ((size_t)nx - 1) * ((size_t)ny - 1);
    MeshJob m{};
    m.frames = (const unsigned*)frames_bgra;
    m.vertex_xy = (const double*)vertex_xy_f64;
    m.B = B, m.H = H, m.W = W, m.nx = nx, m.ny = ny, m.is_metric = is_metric != 0, m.points = mode == MDPT_MESH_POINTS;
    m.x_step = 2.0 / (double)(nx - 1), m.y_step = 2.0 / (double)(ny - 1);  // mesh.js:198
    m.a = a, m.b = b, m.tan_half_fov = tan_half_fov, m.x_scale = x_scale, m.y_scale = y_scale;
    m.alpha_min = edge_threshold * 255.0;  // shaders.js:175
    m.vmap = (int*)scratch;
    m.vcnt = (unsigned*)scratch + (size_t)B * nv;
    m.fcnt = m.vcnt + (size_t)B * mesh_blocks(nv);
    m.bord = m.fcnt + (size_t)B * mesh_blocks(cells);
    CHK(mdpt_launch_post_mesh(m, (float*)xyz_f32, (float*)uv_f32, (unsigned*)faces_u32, (int*)counts_i32, (float*)bounds_f32, (hipStream_t)stream));
    return 0;
}

// ---- rendering of depth meshes (3dviewer/index.html:1158-1228 render_3d, shaders.js mesh shaders)
MDPT_SAME_RECORD(mdpt_texture, RenderTex, 16, bgr, h, w);

static int check_render_sizes(int32_t B, int32_t V, int32_t nv, int32_t nf, int32_t out_h, int32_t out_w) {
    if (B <= 0 || V <= 0 || (int64_t)B * V > 65535) return fail(MDPT_E_INVALID, "bad batch %d x %d views (the product must be 1 .. 65535 per call)", B, V);
    if (nv <= 0 || nf <= 0) return fail(MDPT_E_INVALID, "bad mesh capacity: %d vertices, %d faces", nv, nf);
    if (out_h <= 0 || out_w <= 0 || out_h > RENDER_MAX_SIDE || out_w > RENDER_MAX_SIDE)
        return fail(MDPT_E_INVALID, "bad output size %dx%d (sides of 1 .. %d)", out_h, out_w, RENDER_MAX_SIDE);
    return 0;
}

int mdpt_post_render_scratch_bytes(int32_t B, int32_t V, int32_t nv, int32_t nf, int32_t out_h, int32_t out_w, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_render_sizes(B, V, nv, nf, out_h, out_w));
    *bytes = render_scratch_bytes((size_t)B, (size_t)V, (size_t)nv, (size_t)out_h, (size_t)out_w);
    return 0;
}

int mdpt_post_render(const void* xyz_f32, const void* uv_f32, const void* faces_i32, const void* counts_i32, int32_t B, int32_t nv, int32_t nf,
                     int32_t mode, const mdpt_texture* tex_host, const void* tex_dev, const void* view_proj_f64, int32_t V, int32_t out_h, int32_t out_w,
                     int32_t cull_back, double point_size, void* color_bgra, void* depth_f32, void* face_id_i32, void* scratch, size_t scratch_bytes,
                     void* stream) {
    if (!xyz_f32 || !uv_f32 || !faces_i32 || !counts_i32 || !tex_host || !tex_dev || !view_proj_f64 || !color_bgra || !scratch)
        return fail(MDPT_E_INVALID, "null argument");
    CHK(check_render_sizes(B, V, nv, nf, out_h, out_w));
    if (mode != MDPT_MESH_TRIANGLES && mode != MDPT_MESH_POINTS) return fail(MDPT_E_INVALID, "unknown mesh mode %d", mode);
    if (mode == MDPT_MESH_POINTS && nf != nv) return fail(MDPT_E_INVALID, "a point list holds one face per vertex: nf %d, nv %d", nf, nv);
    if (!(point_size > 0.0 && point_size <= 1024.0)) return fail(MDPT_E_INVALID, "point_size must be in (0, 1024], got %g", point_size);
    for (int i = 0; i < B; ++i)
        if (!tex_host[i].bgr || tex_host[i].h <= 0 || tex_host[i].w <= 0)
            return fail(MDPT_E_INVALID, "null texture or bad texture size %dx%d (mesh %d)", tex_host[i].h, tex_host[i].w, i);
    if ((((uintptr_t)tex_dev | (uintptr_t)view_proj_f64 | (uintptr_t)scratch) & 7) != 0 ||
        (((uintptr_t)xyz_f32 | (uintptr_t)uv_f32 | (uintptr_t)faces_i32 | (uintptr_t)counts_i32 | (uintptr_t)color_bgra | (uintptr_t)depth_f32 |
          (uintptr_t)face_id_i32) & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the matrices and the scratch need 8 bytes, the slabs and the outputs 4)");
    CHK(check_scratch("render", scratch_bytes, render_scratch_bytes((size_t)B, (size_t)V, (size_t)nv, (size_t)out_h, (size_t)out_w), "mdpt_post_render_scratch_bytes"));
    RenderJob r{};
    r.xyz = (const float*)xyz_f32, r.uv = (const float*)uv_f32, r.faces = (const int*)faces_i32, r.counts = (const int*)counts_i32;
    r.tex = (const RenderTex*)tex_dev, r.view_proj = (const double*)view_proj_f64;
    r.B = B, r.V = V, r.nv = nv, r.nf = nf, r.H = out_h, r.W = out_w, r.points = mode == MDPT_MESH_POINTS, r.cull_back = cull_back != 0;
    r.half = (int)nearbyint(point_size * 128.0);
    r.zbuf = (unsigned long long*)scratch;
    r.verts = (RenderVertex*)(r.zbuf + (size_t)B * V * out_h * out_w);
    CHK(mdpt_launch_post_render(r, (unsigned char*)color_bgra, (float*)depth_f32, (int*)face_id_i32, (hipStream_t)stream));
    return 0;
}

// ---- hole filling of rendered views (depth-banded push-pull; not in the reference)
static int check_fill_sizes(int32_t N, int32_t H, int32_t W) {
    CHK(check_count("image", "", N));
    if (H <= 0 || W <= 0 || H > RENDER_MAX_SIDE || W > RENDER_MAX_SIDE) return fail(MDPT_E_INVALID, "bad image size %dx%d (sides of 1 .. %d)", H, W, RENDER_MAX_SIDE);
    return 0;
}

int mdpt_post_fill_scratch_bytes(int32_t N, int32_t H, int32_t W, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_fill_sizes(N, H, W));
    *bytes = fill_scratch_bytes((size_t)N, H, W);
    return 0;
}

int mdpt_post_fill_holes(const void* color_bgra, const void* depth_f32, int32_t N, int32_t H, int32_t W, double band, void* out_bgra, void* out_depth_f32,
                         void* scratch, size_t scratch_bytes, void* stream) {
    if (!color_bgra || !depth_f32 || !out_bgra || !scratch) return fail(MDPT_E_INVALID, "null argument");
    CHK(check_fill_sizes(N, H, W));
    if (!(band >= 0.0 && band <= 1.0)) return fail(MDPT_E_INVALID, "band must be in [0, 1], got %g", band);
    if ((((uintptr_t)color_bgra | (uintptr_t)depth_f32 | (uintptr_t)out_bgra | (uintptr_t)out_depth_f32) & 3) != 0 || ((uintptr_t)scratch & 15) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the images and the depths need 4 bytes, the scratch 16)");
    if (out_bgra == color_bgra || (out_depth_f32 && out_depth_f32 == depth_f32))
        return fail(MDPT_E_INVALID, "the outputs must be buffers of their own, not the inputs");
    CHK(check_scratch("fill", scratch_bytes, fill_scratch_bytes((size_t)N, H, W), "mdpt_post_fill_scratch_bytes"));
    FillJob j{};
    j.color = (const unsigned char*)color_bgra, j.depth = (const float*)depth_f32, j.out = (unsigned char*)out_bgra, j.out_depth = (float*)out_depth_f32;
    j.scratch = scratch, j.N = N, j.keep = 1.0 - band, j.plan = fill_plan(H, W);
    CHK(mdpt_launch_post_fill(j, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
