// libmdpt: the mdpt_segment_* entry points (depth segmentation: connected surfaces, region tables, pick-to-cutout; kernels in post_segment.inc). Named
// apart from mdpt_post_* (see include/mdpt.h); the checks they share with those come from mdpt_post_checks.h, their own are written once below.
#include "mdpt_post_checks.h"

MDPT_SAME_RECORD(mdpt_segment_image, SegmentImage, 56, map, h, w, labels, scratch_off, region_off, tile_off, pixel_off);
MDPT_SAME_RECORD(mdpt_segment_photo, SegmentPhoto, 72, labels, h, w, photo, pitch, H, W, bgra, mask, region_off, regions, pad);
static_assert(MDPT_SEGMENT_TILE == SEGMENT_TILE, "the tile of include/mdpt.h is that of mdpt_kernels.h");

// the table of every segment entry point: present, 1 .. 65535 records
template <class Record> static int check_segment_table(const Record* records, int32_t n, const char* what) {
    if (!records) return fail(MDPT_E_INVALID, "null argument (records_host)");
    return check_count(what, "n = ", n);
}
// a label plane of h x w nodes (record p)
static int check_segment_nodes(const void* labels, int32_t h, int32_t w, int p) {
    CHK(check_map_size(h, w, p));
    if (!labels) return fail(MDPT_E_INVALID, "null labels (image %d)", p);
    if (((uintptr_t)labels & 3) != 0) return fail(MDPT_E_INVALID, "misaligned labels (image %d: int32)", p);
    return 0;
}
// pixel_off of record p = the nodes of the images before it
static int check_pixel_off(int64_t off, size_t running, int p) {
    return off == (int64_t)running ? 0 : fail(MDPT_E_INVALID, "pixel_off %lld of image %d is not the %zu nodes of the images before it", (long long)off, p, running);
}

extern "C" {

int mdpt_segment_scratch_bytes(const mdpt_segment_image* records_host, int32_t n, size_t* bytes) {
    if (!bytes) return fail(MDPT_E_INVALID, "null argument (bytes)");
    CHK(check_segment_table(records_host, n, "image"));
    size_t total = 0;
    for (int p = 0; p < n; ++p) {
        CHK(check_map_size(records_host[p].h, records_host[p].w, p));
        total += segment_image_scratch_bytes((size_t)records_host[p].h, (size_t)records_host[p].w);
    }
    *bytes = total;
    return 0;
}

int mdpt_segment_depth(const mdpt_segment_image* records_host, const void* records_dev, int32_t n, int32_t dtype, int32_t space, double step,
                       int32_t connectivity, int32_t min_area, void* scratch, size_t scratch_bytes, void* counts, void* area, void* bbox, void* first,
                       void* vrange, void* sum_q, void* range, void* stream) {
    if (!records_dev || !scratch) return fail(MDPT_E_INVALID, "null argument (records_dev or scratch)");
    if (!counts || !area || !bbox || !first || !vrange || !sum_q || !range)
        return fail(MDPT_E_INVALID, "null argument (counts, area, bbox, first, vrange, sum_q or range)");
    CHK(check_segment_table(records_host, n, "image"));
    if (!tensor_dtype_ok(dtype)) return fail(MDPT_E_INVALID, "bad tensor dtype %d", dtype);
    if (space != MDPT_ALIGN_INVERSE && space != MDPT_ALIGN_DEPTH) return fail(MDPT_E_INVALID, "unknown segment space %d", space);
    if (!(step >= 0.0) || step > 1e300) return fail(MDPT_E_INVALID, "step must be finite and >= 0, got %g", step);
    if (connectivity != 4 && connectivity != 8) return fail(MDPT_E_INVALID, "connectivity must be 4 or 8, got %d", connectivity);
    if (min_area < 1) return fail(MDPT_E_INVALID, "min_area must be >= 1 (1 keeps every component), got %d", min_area);
    if ((((uintptr_t)records_dev | (uintptr_t)scratch | (uintptr_t)sum_q | (uintptr_t)range) & 7) != 0 ||
        (((uintptr_t)counts | (uintptr_t)area | (uintptr_t)bbox | (uintptr_t)first | (uintptr_t)vrange) & 3) != 0)
        return fail(MDPT_E_INVALID, "misaligned pointer (the table, the scratch, sum_q and range need 8 bytes, the int32 / fp32 tables 4)");
    size_t max_pixels = 0, max_regions = 0, tiles = 0, regions_before = 0, pixels = 0;
    ScratchRegions regions;
    for (int p = 0; p < n; ++p) {
        const mdpt_segment_image& q = records_host[p];
        if (!q.map) return fail(MDPT_E_INVALID, "null map (image %d)", p);
        CHK(check_segment_nodes(q.labels, q.h, q.w, p));
        CHK(check_map_aligned(q.map, dtype, p));
        CHK(regions.add(p, q.scratch_off, segment_image_scratch_bytes((size_t)q.h, (size_t)q.w), scratch_bytes, "of scratch given (mdpt_segment_scratch_bytes)"));
        if (q.region_off != (int64_t)regions_before)
            return fail(MDPT_E_INVALID, "region_off %lld of image %d is not the %zu region rows of the images before it", (long long)q.region_off, p, regions_before);
        CHK(check_running_offset("tile_off", q.tile_off, tiles, p, SEGMENT_TILE, "nodes"));
        CHK(check_pixel_off(q.pixel_off, pixels, p));
        const size_t rows = segment_image_regions((size_t)q.h, (size_t)q.w, (size_t)min_area);
        regions_before += rows, pixels += (size_t)q.h * q.w;
        tiles += segment_image_tiles((size_t)q.h, (size_t)q.w);
        max_pixels = std::max(max_pixels, (size_t)q.h * q.w), max_regions = std::max(max_regions, rows);
    }
    if (tiles >= ((size_t)1 << 31)) return fail(MDPT_E_INVALID, "%zu tiles: a call takes fewer than 2^31", tiles);
    CHK(regions.finish());
    SegmentJob j{};
    j.images = (const SegmentImage*)records_dev;
    j.P = n, j.dt = dtype, j.depth_space = space == MDPT_ALIGN_DEPTH, j.conn8 = connectivity == 8, j.min_area = min_area, j.step = step;
    j.scratch = (char*)scratch;
    j.counts = (int*)counts, j.area = (int*)area, j.bbox = (int*)bbox, j.first = (int*)first, j.vrange = (float*)vrange, j.sum_q = (long long*)sum_q;
    j.range = (double*)range;
    j.max_pixels = max_pixels, j.max_regions = max_regions, j.total_tiles = tiles;
    CHK(mdpt_launch_segment(j, (hipStream_t)stream));
    return 0;
}

int mdpt_segment_colors(const mdpt_segment_image* records_host, const void* records_dev, int32_t n, void* colors, void* stream) {
    if (!records_dev || !colors) return fail(MDPT_E_INVALID, "null argument (records_dev or colors)");
    CHK(check_segment_table(records_host, n, "image"));
    if (((uintptr_t)records_dev & 7) != 0) return fail(MDPT_E_INVALID, "misaligned pointer (the table needs 8 bytes)");
    size_t max_pixels = 0, pixels = 0;
    for (int p = 0; p < n; ++p) {
        const mdpt_segment_image& q = records_host[p];
        CHK(check_segment_nodes(q.labels, q.h, q.w, p));
        CHK(check_pixel_off(q.pixel_off, pixels, p));
        pixels += (size_t)q.h * q.w;
        max_pixels = std::max(max_pixels, (size_t)q.h * q.w);
    }
    CHK(mdpt_launch_segment_colors((const SegmentImage*)records_dev, n, max_pixels, (unsigned char*)colors, (hipStream_t)stream));
    return 0;
}

int mdpt_segment_cutout(const mdpt_segment_photo* records_host, const void* records_dev, int32_t n, const void* picks_dev, int32_t num_picks,
                        int32_t by_label, void* selected, size_t selected_bytes, int32_t invert, void* stream) {
    if (!records_dev || !selected) return fail(MDPT_E_INVALID, "null argument (records_dev or selected)");
    CHK(check_segment_table(records_host, n, "photo"));
    if (num_picks < 0 || (num_picks > 0 && !picks_dev)) return fail(MDPT_E_INVALID, "bad pick count num_picks = %d (>= 0, with picks_dev)", num_picks);
    if (((uintptr_t)records_dev & 7) != 0 || ((uintptr_t)picks_dev & 3) != 0) return fail(MDPT_E_INVALID, "misaligned pointer (the table needs 8 bytes, picks_dev 4)");
    size_t max_groups = 0;
    for (int p = 0; p < n; ++p) {
        const mdpt_segment_photo& q = records_host[p];
        CHK(check_segment_nodes(q.labels, q.h, q.w, p));
        if (!q.photo || !q.bgra || !q.mask) return fail(MDPT_E_INVALID, "null photo, bgra or mask (pair %d)", p);
        CHK(check_photo_size(q.H, q.W, p));
        CHK(check_pitch(q.pitch, q.W, p));
        if (((uintptr_t)q.bgra & 3) != 0) return fail(MDPT_E_INVALID, "misaligned bgra (pair %d: 4 bytes)", p);
        if (q.regions < 0 || q.region_off < 0 || (size_t)q.region_off > selected_bytes || selected_bytes - (size_t)q.region_off < (size_t)q.regions)
            return fail(MDPT_E_INVALID, "the %d rows at region_off %lld of pair %d are outside the %zu bytes of selected", q.regions, (long long)q.region_off, p, selected_bytes);
        max_groups = std::max(max_groups, (((size_t)q.W + 3) / 4) * (size_t)q.H);
    }
    CHK(mdpt_launch_segment_cutout((const SegmentPhoto*)records_dev, n, (const int*)picks_dev, num_picks, by_label != 0, (unsigned char*)selected, invert != 0,
                                   max_groups, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
