#!/usr/bin/env python3
"""Headless single-image run (SURVEY §8(b) "who calls it" / §8(d) config 1): load a checkpoint (or build a seeded synthetic one),
run DPTModel.inference on one BGR uint8 image and print load ms, inference ms and the output shape, like the reference's
run_image.py:204-208 does before it opens its window. No display, no OpenCV: images come from a .npy file (HxWx3 uint8, BGR) or
are synthesised; the 8-bit depth map can be saved as .npy (device-side post-processing, muggled_dpt_amd.postprocess).
Several -i files (of any sizes) run together through DPTModel.inference_images, batched per model tensor size; -o is then a directory
that receives every image's 8-bit depth map at the image's own size (postprocess.depth_to_color_images).
For one image, --display saves the still-image demo's BGR frame (postprocess.depth_to_display: --remove_plane, --threshold, --reverse,
--high_contrast as in run_image.py) and --u24 the 3D viewer's BGRA 24-bit frame with its edge alpha (postprocess.pack_depth_u24_frames).
For one image or several, --cutout DIR saves the depth masking demo's results at each image's own size (postprocess.depth_mask_images:
--mask MIN MAX, --invert_mask and --remove_plane as in experiments/depth_masking.py): <name>_mask.npy (uint8) and <name>_cutout.npy (BGRA).
For one image or several, --block_norms DIR saves the per-token L2 norms of every transformer block's output (DPTModel.block_norms, the capture step
of experiments/block_norm_visualization.py without exporting a block tensor): <name>_blocknorms.npy, fp32 [L, h, w], or an object array of L maps
when the blocks' grids differ (SwinV2).
For one image or several, --mesh DIR saves the 3D viewer's "Save 3D Model" result (postprocess.pack_depth_u24_frames -> depth_frames_to_mesh ->
mesh_io): <name>.glb with the photo as its texture, or with --mesh_obj <name>.obj plus <name>_image.png; --mesh_faces, --mesh_fov and --mesh_points
are the viewer's mesh density, FOV and point mode.
For one image or several, --tiles NY NX saves the depth at the PHOTO's resolution from an NY x NX grid of overlapping tiles (DPTModel.inference_tiled:
every tile fitted to the whole-image prediction with one scale and one shift, then feather-blended; --tile_overlap is the share of a tile side that
neighbours have in common): <name>_tiled.npy, fp32 [H, W], in the current directory.
For one image or several, --guided RADIUS EPS saves the depth at the PHOTO's resolution with the photo as the guide of the enlargement
(postprocess.guided_upsample_images, one call for the whole list; RADIUS in cells of the model's map, EPS the variance below which the photo's texture
is ignored, e.g. 8 1e-4; no photo may be smaller than the model's map of it): <name>_guided.npy, fp32 [H, W], in the current directory.
For one image or several, --refocus FOCUS APERTURE saves every photo refocused by its depth ("portrait mode": refocus.refocus_images, one call for
the whole list; FOCUS = the focal plane, 0 .. 1 of the map's range or, for a metric model, a depth; APERTURE = photo pixels of blur radius per unit of
defocus, e.g. 0.8 32): <name>_refocus.png in the current directory. --refocus_at X Y focuses on the point (X, Y) of the photo, normalised, instead of
FOCUS; --refocus_radius R is the largest blur radius (0 .. 32, default 16); --refocus_guided RADIUS EPS enlarges the depth with the photo as the guide first.
For one image or several, --normals saves every photo's encoded surface normal map (relight.depth_normals at the photo's size; B, G, R = z, y, x):
<name>_normals.png in the current directory. --relight X Y Z saves every photo shaded by its normals with a light towards (X, Y, Z) in the camera frame
(x right, y up, z towards the camera; relight.relight_images, one call for the whole list): <name>_relit000.png; --relight_sweep N instead writes N frames
<name>_relit###.png for a ring of N lights at the elevation of (X, Y, Z), starting at its azimuth; --relight_guided RADIUS EPS enlarges the depth with the
photo as the guide first (and takes the normals over one photo pixel). --shade X Y Z [--shade_sweep N] does the same with cast shadows and ambient
occlusion (relight.shade_images; --shade_reach K: the grid nodes a shadow march walks, 0 .. 32, 0 = no shadows; --shade_ao STRENGTH: the occlusion's
strength, 0 = none): <name>_shaded###.png.
For one image or several, --segments STEP saves every map's depth-connected surfaces (segment.segment_depth, one call for the whole list; STEP = the largest
step between linked neighbours, as a share of the map's range or, for a metric model, of the nearer depth, e.g. 0.02; --segments_min_area N drops smaller
regions, default 16; --segments_conn 4|8): <name>_labels.npy (int32, the model's map size, -1 = no region) and <name>_regions.json (area, bbox, first, vmin,
vmax, mean per region) in the current directory. --pick X Y (repeatable; normalised) also saves the regions under those points of every photo as
<name>_pick_mask.npy (uint8) and <name>_pick_cutout.npy (BGRA) at the photo's size (segment.region_cutouts).
With --truth DIR, --truth_local GH GW also completes every measured map (local_align.fit_true_depth_local over a GH x GW grid, true_depth_local; --truth_local_radius R
cells, default 1; --truth_local_prior K pseudo-samples, default 4): <name>_completed.npy (true depth at the truth's size, following the measurements locally) and
the completed map's metrics next to the global fit's in <name>_metrics.json (keys local_*).
--stable [ALPHA] takes the images, in order, as the frames of ONE clip (they share a size): DPTModel.inference_video aligns every frame's map to the
frame before it and filters the clip over time (muggled_dpt_amd.video; ALPHA = the filter's weight, default 0.3), video_display shows it with a
carried range: <name>_stable.npy (fp32, the model's map size) and <name>_stable.png (the photo's size) into --output (a directory; default: the
current one). Nothing else is written in that mode.
--crop X1 Y1 X2 Y2 is the reference's --crop with a stored box: normalised corners, applied to every image before it is predicted
(crop_slices_from_norm: a side under 5 px falls back to the image's full extent); every output is then that of the cropped image.

  python tools/mdpt_run_image.py --synthetic vits --size 518 --fp32
  python tools/mdpt_run_image.py -m model_weights/depth_anything_v2_vitl.pth -i image.npy -o depth_u8.npy
  python tools/mdpt_run_image.py -m model_weights/depth_anything_v2_vitl.pth -i a.npy -i b.npy -i c.npy -o depth_dir
  python tools/mdpt_run_image.py -m model_weights/depth_anything_v2_vitl.pth -i image.npy --crop 0.25 0.1 0.75 0.9 -o depth_u8.npy
  python tools/mdpt_run_image.py -m model_weights/depth_anything_v2_vitl.pth -i a.npy -i b.npy --mask 0.5 1 --remove_plane 0.5 --cutout cut_dir
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-m", "--model_path", default=None, help="checkpoint file (any of the four supported families)")
    ap.add_argument("--synthetic", default="vits", help="config name for seeded synthetic weights when no checkpoint is given")
    ap.add_argument("-i", "--image_path", action="append", default=None,
                    help=".npy file holding an HxWx3 uint8 BGR image; give it several times to run several images (any sizes) batched")
    ap.add_argument("-b", "--batch_size", type=int, default=32, help="several images: at most this many per batched forward")
    ap.add_argument("-s", "--size", type=int, default=None, help="max side length (default: the model's base size)")
    ap.add_argument("-a", "--use_aspect_ratio", action="store_true", help="keep the image aspect ratio (default: square sizing)")
    ap.add_argument("--crop", type=float, nargs=4, default=None, metavar=("X1", "Y1", "X2", "Y2"),
                    help="predict this box of every image only: normalised top-left and bottom-right corners (the reference's --crop)")
    ap.add_argument("--fp32", action="store_true", help="float32 model = split-bf16 fp32-class arithmetic (default: bfloat16)")
    ap.add_argument("-o", "--output", default=None, help="save the 8-bit depth map (.npy)")
    ap.add_argument("--remove_plane", type=float, default=0.0, metavar="F", help="single image: remove F times the plane of best fit (run_image.py)")
    ap.add_argument("--threshold", type=float, nargs=2, default=(0.0, 1.0), metavar=("MIN", "MAX"), help="single image: display threshold window")
    ap.add_argument("--reverse", action="store_true", help="single image: reverse the display values")
    ap.add_argument("--high_contrast", action="store_true", help="single image: thresholded histogram equalization")
    ap.add_argument("--display", default=None, metavar="OUT.npy", help="single image: save the still-image demo's BGR display frame (.npy)")
    ap.add_argument("--u24", default=None, metavar="OUT.npy", help="single image: save the 3D viewer's BGRA 24-bit frame with edge alpha (.npy)")
    ap.add_argument("--mask", type=float, nargs=2, default=(0.0, 1.0), metavar=("MIN", "MAX"), help="depth masking: keep pixels whose depth is in MIN..MAX")
    ap.add_argument("--invert_mask", action="store_true", help="depth masking: keep the pixels outside the --mask range instead")
    ap.add_argument("--cutout", default=None, metavar="DIR", help="save every image's depth mask and BGRA cutout (.npy) at its own size into DIR")
    ap.add_argument("--block_norms", default=None, metavar="DIR", help="save every image's per-block token norm maps (.npy) into DIR")
    ap.add_argument("--mesh", default=None, metavar="DIR", help="save every image's textured mesh (.glb) into DIR")
    ap.add_argument("--mesh_faces", type=float, default=None, metavar="N", help="mesh: target number of faces (default: the viewer's 312500)")
    ap.add_argument("--mesh_fov", type=float, default=None, metavar="DEG", help="mesh: field of view in degrees (default: the viewer's 50)")
    ap.add_argument("--mesh_obj", action="store_true", help="mesh: write <name>.obj and <name>_image.png instead of <name>.glb")
    ap.add_argument("--mesh_points", action="store_true", help="mesh: a point cloud (one vertex per face) instead of triangles")
    ap.add_argument("--tiles", type=int, nargs=2, default=None, metavar=("NY", "NX"), help="save every image's depth at its own resolution from an NY x NX tile grid")
    ap.add_argument("--tile_overlap", type=float, default=0.25, metavar="F", help="tiles: the share of a tile side that neighbouring tiles have in common")
    ap.add_argument("--guided", nargs=2, default=None, metavar=("RADIUS", "EPS"), help="save every image's depth at its own resolution, enlarged with "
                    "the photo as the guide (fast guided filter): window radius in map cells and regularisation, e.g. 8 1e-4")
    ap.add_argument("--refocus", type=float, nargs=2, default=None, metavar=("FOCUS", "APERTURE"), help="save every photo refocused by its depth: the focal "
                    "plane (0 .. 1 of the map's range; a depth for a metric model) and the blur radius in photo pixels per unit of defocus, e.g. 0.8 32")
    ap.add_argument("--refocus_at", type=float, nargs=2, default=None, metavar=("X", "Y"), help="refocus: focus on this point of the photo (normalised) instead of FOCUS")
    ap.add_argument("--refocus_radius", type=int, default=16, metavar="R", help="refocus: the largest blur radius in photo pixels, 0 .. 32")
    ap.add_argument("--refocus_guided", nargs=2, default=None, metavar=("RADIUS", "EPS"), help="refocus: enlarge the depth with the photo as the guide first")
    ap.add_argument("--normals", action="store_true", help="save every photo's encoded surface normal map, <name>_normals.png")
    ap.add_argument("--relight", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="save every photo relit from the direction (X, Y, Z) "
                    "(x right, y up, z towards the camera), e.g. -1 1 1")
    ap.add_argument("--relight_sweep", type=int, default=None, metavar="N", help="relight: N frames for a ring of lights at the elevation of (X, Y, Z)")
    ap.add_argument("--relight_guided", nargs=2, default=None, metavar=("RADIUS", "EPS"), help="normals / relight / shade: enlarge the depth with the photo as the guide first")
    ap.add_argument("--shade", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="save every photo relit from (X, Y, Z) with cast shadows "
                    "and ambient occlusion, <name>_shaded000.png")
    ap.add_argument("--shade_sweep", type=int, default=None, metavar="N", help="shade: N frames for a ring of lights at the elevation of (X, Y, Z)")
    ap.add_argument("--shade_reach", type=int, default=32, metavar="K", help="shade: grid nodes a shadow march walks (0 .. 32; 0: no shadows)")
    ap.add_argument("--shade_ao", type=float, default=1.0, metavar="STRENGTH", help="shade: strength of the ambient occlusion (0: none)")
    ap.add_argument("--segments", type=float, default=None, metavar="STEP", help="save every map's depth-connected surfaces, <name>_labels.npy and "
                    "<name>_regions.json: the largest step between linked neighbours (share of the range; of the nearer depth for a metric model), e.g. 0.02")
    ap.add_argument("--segments_min_area", type=int, default=16, metavar="N", help="segments: drop regions of fewer than N nodes")
    ap.add_argument("--segments_conn", type=int, default=4, choices=(4, 8), help="segments: neighbours along the axes, or the diagonals too")
    ap.add_argument("--pick", type=float, nargs=2, action="append", default=None, metavar=("X", "Y"), help="segments: save the region under this point of "
                    "every photo (normalised; repeatable) as <name>_pick_mask.npy and <name>_pick_cutout.npy")
    ap.add_argument("--truth", default=None, metavar="DIR", help="measured depth per image, DIR/<name>.npy (fp32, any size; zero or NaN: no measurement): "
                    "fit the prediction to it, save <name>_true.npy (true depth at the truth's size) and <name>_metrics.json")
    ap.add_argument("--truth_method", default="lstsq", choices=("lstsq", "median"), help="truth: least squares, or median and mean absolute deviation")
    ap.add_argument("--truth_local", type=int, nargs=2, default=None, metavar=("GH", "GW"), help="truth: also fit (A, B) per cell of a GH x GW grid over the "
                    "truth and save <name>_completed.npy (depth completion), its metrics beside the global fit's")
    ap.add_argument("--truth_local_radius", type=int, default=1, metavar="R", help="truth_local: window radius in cells")
    ap.add_argument("--truth_local_prior", type=float, default=4.0, metavar="K", help="truth_local: pseudo-samples that pull a window towards the global fit")
    ap.add_argument("--truth_range", type=float, nargs=2, default=None, metavar=("MIN", "MAX"), help="truth: use measurements within MIN..MAX only")
    ap.add_argument("--render", default=None, metavar="DIR", help="render every image's depth mesh from moving viewpoints (the 3D viewer's view) and "
                    "save <name>_view###.png (RGBA) into DIR; the mesh follows --mesh_faces / --mesh_fov / --mesh_points")
    ap.add_argument("--render_views", type=int, default=16, metavar="N", help="render: number of views on the swing")
    ap.add_argument("--render_swing", type=float, nargs=2, default=(8.0, 4.0), metavar=("YAW", "PITCH"), help="render: half-axes of the swing in degrees")
    ap.add_argument("--render_wh", type=int, nargs=2, default=(1280, 720), metavar=("W", "H"), help="render: output size")
    ap.add_argument("--render_stereo", type=float, default=None, metavar="BASELINE", help="render: a left / right pair BASELINE world units apart "
                    "instead of the swing (views 000 and 001)")
    ap.add_argument("--render_fill", type=float, nargs="?", const=0.1, default=None, metavar="BAND", help="render: fill the holes of every view "
                    "(depth-banded push-pull, BAND in 0..1, default 0.1): the PNGs then have alpha 255 everywhere")
    ap.add_argument("--stable", type=float, nargs="?", const=0.3, default=None, metavar="ALPHA", help="the images, in order, are the frames of one clip "
                    "(one size): save every frame's temporally stable depth <name>_stable.npy (fp32) and its display frame <name>_stable.png, "
                    "normalised by a carried range, into --output (a directory; default: the working directory); ALPHA = the filter's weight, default 0.3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mdpt_run_image needs an MI355X: no GPU visible (there is no CPU fallback)")

    from muggled_dpt_amd import make_depthanythingv2_dpt_from_original_state_dict, make_dpt_from_state_dict
    from muggled_dpt_amd.postprocess import convert_to_uint8
    t0 = time.perf_counter()
    if args.model_path:
        cfg, model = make_dpt_from_state_dict(args.model_path)
    else:
        from muggled_dpt_amd.synthetic import make_synthetic_original_state_dict
        cfg, model = make_depthanythingv2_dpt_from_original_state_dict(make_synthetic_original_state_dict(args.synthetic, 0))
    model.to("cuda", torch.float32 if args.fp32 else torch.bfloat16)
    if args.stable is not None:
        return run_clip(model, args)
    if args.image_path and len(args.image_path) > 1:
        return run_images(model, args, t0, bool(cfg.get("is_metric", False)))
    if args.image_path:
        img = np.load(args.image_path[0])
    else:
        img = np.random.default_rng(1).integers(0, 256, (518, 518, 3), dtype=np.uint8)
    crop = crop_argument(args)
    model.inference(img, args.size, not args.use_aspect_ratio, crop=crop)  # first call builds the engine (weight repack)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print(f"Loading model & first call: {round(1000 * (t1 - t0))} ms", flush=True)
    depth = model.inference(img, args.size, not args.use_aspect_ratio, crop=crop)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    img = cropped(img, crop)  # what was predicted: the display steps below work at its size
    print(f"Inference: {round(1000 * (t2 - t1), 2)} ms", f"Prediction shape: {tuple(depth.shape)}, dtype {depth.dtype}, device {depth.device}", sep="\n")
    if args.output:
        np.save(args.output, convert_to_uint8(depth).squeeze(0).cpu().numpy())
        print("saved", args.output)
    if args.display:
        from muggled_dpt_amd.postprocess import depth_to_display
        frame = depth_to_display(depth, (img.shape[1], img.shape[0]), args.remove_plane, tuple(args.threshold), args.reverse, args.high_contrast)
        np.save(args.display, frame[0].cpu().numpy())
        print("saved", args.display)
    if args.u24:
        from muggled_dpt_amd.postprocess import pack_depth_u24_frames
        np.save(args.u24, pack_depth_u24_frames(depth, is_metric=bool(cfg.get("is_metric", False)))[0].cpu().numpy())
        print("saved", args.u24)
    save_cutouts(args, args.image_path or ["synthetic.npy"], [img], [depth])
    save_block_norms(model, args, args.image_path or ["synthetic.npy"], [img])
    save_meshes(args, bool(cfg.get("is_metric", False)), args.image_path or ["synthetic.npy"], [img], [depth])
    save_renders(args, bool(cfg.get("is_metric", False)), args.image_path or ["synthetic.npy"], [img], [depth])
    save_tiled(model, args, args.image_path or ["synthetic.npy"], [img])
    save_true_depth(args, bool(cfg.get("is_metric", False)), args.image_path or ["synthetic.npy"], [depth])
    save_guided(args, args.image_path or ["synthetic.npy"], [img], [depth])
    save_refocus(args, bool(cfg.get("is_metric", False)), args.image_path or ["synthetic.npy"], [img], [depth])
    save_relight(args, bool(cfg.get("is_metric", False)), args.image_path or ["synthetic.npy"], [img], [depth])
    save_segments(args, bool(cfg.get("is_metric", False)), args.image_path or ["synthetic.npy"], [img], [depth])


def crop_argument(args):
    """--crop X1 Y1 X2 Y2 -> the ((x1, y1), (x2, y2)) box DPTModel.inference takes, or None"""
    return None if args.crop is None else ((args.crop[0], args.crop[1]), (args.crop[2], args.crop[3]))


def cropped(img, crop):
    """the box of the image that crop= makes the model predict (a packed copy, for the display steps)"""
    if crop is None:
        return img
    from muggled_dpt_amd import crop_slices_from_norm
    ys, xs = crop_slices_from_norm(img.shape, crop)
    print(f"Cropping to x {xs.start}:{xs.stop}, y {ys.start}:{ys.stop} of {img.shape[1]}x{img.shape[0]}")
    return np.ascontiguousarray(img[ys, xs])


def save_cutouts(args, paths, images, depths):
    """--cutout: the depth masking demo's save step for every image (postprocess.depth_mask_images, one call for the whole list)"""
    if not args.cutout:
        return
    from muggled_dpt_amd.postprocess import depth_mask_images
    os.makedirs(args.cutout, exist_ok=True)
    results = depth_mask_images(depths, images, args.remove_plane, tuple(args.mask), args.invert_mask)
    for path, (cutout, mask) in zip(paths, results):
        stem = os.path.join(args.cutout, os.path.splitext(os.path.basename(path))[0])
        np.save(stem + "_mask.npy", mask.cpu().numpy())
        np.save(stem + "_cutout.npy", cutout.cpu().numpy())
        print("saved", stem + "_mask.npy", stem + "_cutout.npy")


def save_meshes(args, is_metric, paths, images, depths):
    """--mesh: inference -> pack_depth_u24_frames -> depth_frames_to_mesh -> the writer, one mesh call per image (photo sizes set the grids)"""
    if not args.mesh:
        return
    from muggled_dpt_amd import mesh_io
    from muggled_dpt_amd import postprocess as pp
    os.makedirs(args.mesh, exist_ok=True)
    for path, img, depth in zip(paths, images, depths):
        frames = pp.pack_depth_u24_frames(depth, is_metric=is_metric)
        slabs = pp.depth_frames_to_mesh(frames, (img.shape[1], img.shape[0]), pp.MESH_FOV_DEG if args.mesh_fov is None else args.mesh_fov,
                                        is_metric=is_metric, target_num_faces=pp.MESH_TARGET_FACES if args.mesh_faces is None else args.mesh_faces,
                                        mode="points" if args.mesh_points else "triangles")
        xyz, uv, faces, bounds = pp.mesh_views(*slabs)[0]
        stem = os.path.join(args.mesh, os.path.splitext(os.path.basename(path))[0])
        rgb = np.ascontiguousarray(img[:, :, ::-1])  # the photo, top row first: write_glb flips it for glTF's v axis, the .obj's PNG stays upright
        if args.mesh_obj:
            mesh_io.write_obj(stem + ".obj", xyz, uv, faces)
            with open(stem + "_image.png", "wb") as fh:
                fh.write(mesh_io.encode_png(rgb))
            print("saved", stem + ".obj", stem + "_image.png", f"({xyz.shape[0]} vertices, {faces.shape[0]} faces)")
        else:
            mesh_io.write_glb(stem + ".glb", xyz, uv, faces, rgb, bounds)
            print("saved", stem + ".glb", f"({xyz.shape[0]} vertices, {faces.shape[0]} faces)")


def save_renders(args, is_metric, paths, images, depths):
    """--render: pack_depth_u24_frames -> depth_frames_to_mesh -> render_mesh per image (photo sizes set the grids), every view of an image in one
    call; the views are a closed swing around the viewer's start pose, or a stereo pair"""
    if not args.render:
        return
    from muggled_dpt_amd import mesh_io, orbit_camera
    from muggled_dpt_amd import postprocess as pp
    os.makedirs(args.render, exist_ok=True)
    w, h = args.render_wh
    if args.render_stereo is not None:
        views = orbit_camera.stereo_views(args.render_stereo, aspect=w / h)
    else:
        views = orbit_camera.swing_views(args.render_views, args.render_swing[0], args.render_swing[1], aspect=w / h)
    for path, img, depth in zip(paths, images, depths):
        frames = pp.pack_depth_u24_frames(depth, is_metric=is_metric)
        xyz, uv, faces, counts, _ = pp.depth_frames_to_mesh(frames, (img.shape[1], img.shape[0]), pp.MESH_FOV_DEG if args.mesh_fov is None else args.mesh_fov,
                                                           is_metric=is_metric,
                                                           target_num_faces=pp.MESH_TARGET_FACES if args.mesh_faces is None else args.mesh_faces,
                                                           mode="points" if args.mesh_points else "triangles")
        color = pp.render_mesh(xyz, uv, faces, counts, [img], views, (w, h), point_size=2.0, fill_holes=args.render_fill)[0]
        rgba = color[..., [2, 1, 0, 3]].cpu().numpy()
        stem = os.path.join(args.render, os.path.splitext(os.path.basename(path))[0])
        for k in range(rgba.shape[0]):
            with open(f"{stem}_view{k:03d}.png", "wb") as fh:
                fh.write(mesh_io.encode_png(rgba[k]))
        print("saved", f"{stem}_view000.png .. _view{rgba.shape[0] - 1:03d}.png", f"({w}x{h}, {float((rgba[..., 3] > 0).mean()):.3f} of the pixels covered)")


def save_tiled(model, args, paths, images):
    """--tiles: DPTModel.inference_tiled per image (one batched inference_regions call and one stitch each), the fp32 map at the image's own size"""
    if not args.tiles:
        return
    for path, img in zip(paths, images):
        tiled = model.inference_tiled(img, tiles=tuple(args.tiles), overlap=args.tile_overlap, max_side_length=args.size,
                                      use_square_sizing=not args.use_aspect_ratio, batch_size=args.batch_size)
        out = os.path.splitext(os.path.basename(path))[0] + "_tiled.npy"
        np.save(out, tiled[0].cpu().numpy())
        print("saved", out, f"({tiled.shape[2]}x{tiled.shape[1]} from {args.tiles[0]}x{args.tiles[1]} tiles)")


def save_true_depth(args, is_metric, paths, depths):
    """--truth: one fit_true_depth, one depth_metrics and one true_depth call over all images (what DPTModel.evaluate_depth runs after its
    inference), the fit and the metrics read back once for the .json files; --truth_local: fit_true_depth_local and true_depth_local as well (what
    DPTModel.inference_completed runs), the completed maps scored as they are (depth_metrics with fit=None in depth space)"""
    if not args.truth:
        if args.truth_local is not None:
            raise SystemExit("--truth_local needs --truth DIR")
        return
    import json
    from muggled_dpt_amd import postprocess as pp
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    truths = [np.load(os.path.join(args.truth, stem + ".npy")).astype(np.float32) for stem in stems]
    space = "depth" if is_metric else "inverse"
    rng = (None, None) if args.truth_range is None else tuple(args.truth_range)
    fit = pp.fit_true_depth(depths, truths, None, space, args.truth_method, rng)
    metrics = pp.depth_metrics(depths, truths, fit, None, space, rng)
    maps = pp.true_depth(depths, fit, [t.shape for t in truths], space)
    completed = local_metrics = None
    if args.truth_local is not None:
        from muggled_dpt_amd import local_align
        local = local_align.fit_true_depth_local(depths, truths, None, space=space, grid_hw=tuple(args.truth_local), radius=args.truth_local_radius,
                                                 prior=args.truth_local_prior, truth_range=rng)
        completed = local_align.true_depth_local(depths, local, [t.shape for t in truths], space)
        local_metrics = pp.depth_metrics(completed, truths, None, None, "depth", rng).cpu().tolist()
    fit, metrics = fit.cpu().tolist(), metrics.cpu().tolist()
    for k, stem in enumerate(stems):
        np.save(stem + "_true.npy", maps[k][0].cpu().numpy())
        report = {"A": fit[k][0], "B": fit[k][1], "space": space, "method": args.truth_method, **dict(zip(pp.DEPTH_METRIC_NAMES, metrics[k]))}
        if completed is not None:
            np.save(stem + "_completed.npy", completed[k][0].cpu().numpy())
            report.update({"local_grid": list(args.truth_local), "local_radius": args.truth_local_radius, "local_prior": args.truth_local_prior,
                           **{"local_" + name: value for name, value in zip(pp.DEPTH_METRIC_NAMES, local_metrics[k])}})
            print("saved", stem + "_completed.npy", f"(AbsRel {local_metrics[k][2]:.4g}, delta1 {local_metrics[k][7]:.4g})")
        with open(stem + "_metrics.json", "w") as fh:
            json.dump(report, fh, indent=1)
        print("saved", stem + "_true.npy", stem + "_metrics.json", f"(A {fit[k][0]:.6g}, B {fit[k][1]:.6g}, AbsRel {metrics[k][2]:.4g}, delta1 {metrics[k][7]:.4g})")


def save_guided(args, paths, images, depths):
    """--guided: one postprocess.guided_upsample_images call over all images, the fp32 map at each image's own size"""
    if not args.guided:
        return
    from muggled_dpt_amd.postprocess import guided_upsample_images
    maps = guided_upsample_images(depths, images, int(args.guided[0]), float(args.guided[1]))
    for path, m in zip(paths, maps):
        out = os.path.splitext(os.path.basename(path))[0] + "_guided.npy"
        np.save(out, m[0].cpu().numpy())
        print("saved", out, f"({m.shape[2]}x{m.shape[1]}, radius {int(args.guided[0])}, eps {float(args.guided[1]):g})")


def save_refocus(args, is_metric, paths, images, depths):
    """--refocus: one refocus.refocus_images call over all images (after one guided_upsample_images call with --refocus_guided), a PNG per photo"""
    if not args.refocus:
        return
    from muggled_dpt_amd import mesh_io
    from muggled_dpt_amd.refocus import refocus_images
    if args.refocus_guided:
        from muggled_dpt_amd.postprocess import guided_upsample_images
        depths = guided_upsample_images(depths, images, int(args.refocus_guided[0]), float(args.refocus_guided[1]))
    shown = refocus_images(depths, images, args.refocus[0], args.refocus_at, args.refocus[1], args.refocus_radius, 0.0, "depth" if is_metric else "inverse")
    for path, bgr in zip(paths, shown):
        out = os.path.splitext(os.path.basename(path))[0] + "_refocus.png"
        with open(out, "wb") as fh:
            fh.write(mesh_io.encode_png(np.ascontiguousarray(bgr.cpu().numpy()[:, :, ::-1])))
        where = f"at ({args.refocus_at[0]:g}, {args.refocus_at[1]:g})" if args.refocus_at else f"focus {args.refocus[0]:g}"
        print("saved", out, f"({bgr.shape[1]}x{bgr.shape[0]}, {where}, aperture {args.refocus[1]:g}, radius <= {args.refocus_radius})")


def save_segments(args, is_metric, paths, images, depths):
    """--segments / --pick: one segment.segment_depth call over all maps, the labels and the region table per image; with --pick one region_cutouts call"""
    if args.segments is None:
        if args.pick:
            raise SystemExit("--pick needs --segments STEP")
        return
    import json
    from muggled_dpt_amd.segment import region_cutouts, segment_depth
    seg = segment_depth(depths, space="depth" if is_metric else "inverse", step=args.segments, connectivity=args.segments_conn, min_area=args.segments_min_area)
    for path, labels, rows in zip(paths, seg.labels, seg.region_views()):
        stem = os.path.splitext(os.path.basename(path))[0]
        np.save(stem + "_labels.npy", labels.cpu().numpy())
        table = {name: rows[name].cpu().numpy().tolist() for name in ("area", "bbox", "first", "vmin", "vmax", "mean")}
        with open(stem + "_regions.json", "w") as fh:
            json.dump(dict(count=rows["count"], **table), fh)
        print("saved", stem + "_labels.npy", stem + "_regions.json", f"({rows['count']} regions of {labels.shape[1]}x{labels.shape[0]} nodes)")
    if args.pick:
        for path, (cutout, mask) in zip(paths, region_cutouts(seg, images, points=[[tuple(p) for p in args.pick]] * len(images))):
            stem = os.path.splitext(os.path.basename(path))[0]
            np.save(stem + "_pick_mask.npy", mask.cpu().numpy())
            np.save(stem + "_pick_cutout.npy", cutout.cpu().numpy())
            print("saved", stem + "_pick_mask.npy", stem + "_pick_cutout.npy")


def save_relight(args, is_metric, paths, images, depths):
    """--normals / --relight: one relight.depth_normals and / or one relight.relight_images call over all images (after one guided_upsample_images call with
    --relight_guided), PNGs per photo"""
    if not (args.normals or args.relight or args.shade):
        return
    import math
    from muggled_dpt_amd import mesh_io
    from muggled_dpt_amd.relight import depth_normals, light_sweep, relight_images
    step = None
    if args.relight_guided:
        from muggled_dpt_amd.postprocess import guided_upsample_images
        depths, step = guided_upsample_images(depths, images, int(args.relight_guided[0]), float(args.relight_guided[1])), 1
    space = "depth" if is_metric else "inverse"

    def save(out, bgr, note):
        with open(out, "wb") as fh:
            fh.write(mesh_io.encode_png(np.ascontiguousarray(bgr.cpu().numpy()[:, :, ::-1])))
        print("saved", out, f"({bgr.shape[1]}x{bgr.shape[0]}, {note})")

    if args.normals:
        for path, bgr in zip(paths, depth_normals(depths, None, images, space=space, step=step, encode=True)[1]):
            save(os.path.splitext(os.path.basename(path))[0] + "_normals.png", bgr, "normal map")
    def ring_of(light, sweep):
        """the light alone, or with a sweep a ring of lights at its elevation that starts at its azimuth"""
        if not sweep:
            return [light]
        x, y, z = light
        ring = light_sweep(sweep, math.degrees(math.atan2(z, math.hypot(x, y))))
        turn = math.atan2(y, x)
        return [(math.cos(turn) * lx - math.sin(turn) * ly, math.sin(turn) * lx + math.cos(turn) * ly, lz) for lx, ly, lz in ring.tolist()]

    if args.relight:
        lights = ring_of(args.relight, args.relight_sweep)
        for path, frames in zip(paths, relight_images(depths, images, lights, space=space, step=step)):
            for k, bgr in enumerate(frames):
                save(os.path.splitext(os.path.basename(path))[0] + f"_relit{k:03d}.png", bgr, f"light {tuple(round(v, 3) for v in lights[k])}")
    if args.shade:
        from muggled_dpt_amd.relight import shade_images
        lights = ring_of(args.shade, args.shade_sweep)
        for path, frames in zip(paths, shade_images(depths, images, lights, space=space, step=step, shadow_reach=args.shade_reach, ao_strength=args.shade_ao)):
            for k, bgr in enumerate(frames):
                save(os.path.splitext(os.path.basename(path))[0] + f"_shaded{k:03d}.png", bgr,
                     f"light {tuple(round(v, 3) for v in lights[k])}, shadows over {args.shade_reach} nodes, occlusion {args.shade_ao:g}")


def save_block_norms(model, args, paths, images):
    """--block_norms: one DPTModel.block_norms call per group of images that share a model tensor size"""
    if not args.block_norms:
        return
    os.makedirs(args.block_norms, exist_ok=True)
    groups = {}
    for k, img in enumerate(images):
        x = model.prepare_image_bgr(img, args.size, not args.use_aspect_ratio)
        groups.setdefault(tuple(x.shape[2:]), []).append((k, x))
    for members in groups.values():
        for at in range(0, len(members), args.batch_size):
            chunk = members[at:at + args.batch_size]
            norms, _ = model.block_norms(torch.cat([x for _, x in chunk]))
            host = [n.cpu().numpy() for n in norms]
            for row, (k, _) in enumerate(chunk):
                maps = [h[row] for h in host]
                if len({m.shape for m in maps}) == 1:
                    arr = np.stack(maps)
                else:
                    arr = np.empty(len(maps), dtype=object)
                    arr[:] = maps
                out = os.path.join(args.block_norms, os.path.splitext(os.path.basename(paths[k]))[0] + "_blocknorms.npy")
                np.save(out, arr, allow_pickle=True)
                print("saved", out)


def run_images(model, args, t0, is_metric=False):
    """several images of any sizes: DPTModel.inference_images, then every 8-bit map back at its image's own size"""
    from muggled_dpt_amd.postprocess import depth_to_color_images
    images = [np.load(p) for p in args.image_path]
    square = not args.use_aspect_ratio
    crop = crop_argument(args)
    model.inference_images(images, args.size, square, args.batch_size, crops=crop)  # first call builds the engine (weight repack)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print(f"Loading model & first call: {round(1000 * (t1 - t0))} ms", flush=True)
    depths = model.inference_images(images, args.size, square, args.batch_size, crops=crop)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    images = [cropped(img, crop) for img in images]  # what was predicted: the display steps below work at those sizes
    print(f"Inference of {len(images)} images: {round(1000 * (t2 - t1), 2)} ms ({round(1000 * (t2 - t1) / len(images), 2)} ms per image)")
    for path, img, d in zip(args.image_path, images, depths):
        print(f"  {path}: {img.shape[1]}x{img.shape[0]} -> prediction {tuple(d.shape)}, dtype {d.dtype}")
    if args.output:
        os.makedirs(args.output, exist_ok=True)
        grey = depth_to_color_images(depths, [(img.shape[1], img.shape[0]) for img in images])
        for path, g in zip(args.image_path, grey):
            out = os.path.join(args.output, os.path.splitext(os.path.basename(path))[0] + "_depth_u8.npy")
            np.save(out, g[0, :, :, 0].cpu().numpy())
            print("saved", out)
    save_cutouts(args, args.image_path, images, depths)
    save_block_norms(model, args, args.image_path, images)
    save_meshes(args, is_metric, args.image_path, images, depths)
    save_renders(args, is_metric, args.image_path, images, depths)
    save_tiled(model, args, args.image_path, images)
    save_true_depth(args, is_metric, args.image_path, depths)
    save_guided(args, args.image_path, images, depths)
    save_refocus(args, is_metric, args.image_path, images, depths)
    save_relight(args, is_metric, args.image_path, images, depths)
    save_segments(args, is_metric, args.image_path, images, depths)


def run_clip(model, args):
    """--stable: the images as the frames of one clip through DPTModel.inference_video, the display frames through video.video_display"""
    from muggled_dpt_amd import mesh_io
    from muggled_dpt_amd.video import video_display
    if not args.image_path:
        raise SystemExit("--stable needs the clip's frames: -i FRAME.npy for every frame, in order")
    frames = [np.load(p) for p in args.image_path]
    if len({f.shape for f in frames}) != 1:
        raise SystemExit(f"--stable: the frames of a clip share one size, got {sorted({f.shape for f in frames})}")
    stable, table, _ = model.inference_video(frames, None, args.batch_size, args.size, not args.use_aspect_ratio, alpha=args.stable)
    shown, _ = video_display(stable, table, None, (frames[0].shape[1], frames[0].shape[0]), args.reverse)
    out_dir = args.output or "."
    os.makedirs(out_dir, exist_ok=True)
    cuts = table[:, 3].cpu().numpy()
    for k, path in enumerate(args.image_path):
        stem = os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0] + "_stable")
        np.save(stem + ".npy", stable[k].cpu().numpy())
        with open(stem + ".png", "wb") as fh:
            fh.write(mesh_io.encode_png(shown[k].cpu().numpy()))
        print("saved", stem + ".npy", stem + ".png", "(the chain re-anchors here)" if cuts[k] and k else "")


if __name__ == "__main__":
    main()
