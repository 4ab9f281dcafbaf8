"""fp64 numpy restatement of the cast shadows and the ambient occlusion of the relighting (muggled_dpt_amd.relight.light_occlusion / shade_images,
mdpt_post_shadows), written from the definition in include/mdpt.h: whole-grid arrays, one gather per march step k over all nodes at once, a Python loop over
the lights and the directions. Nothing of the kernel's scheme (tiles, halo, LDS) is in here. The depth, the points and the normal of the working grid are
tests/normals_restate.py's, called on the grid with the photo's camera; the resize of the planes to the photo is refocus_restate.map_at_pixels.

  grid ....... node (i, j) of gh x gw = pixel (i, j) of a gh x gw image: z, P, n = normals_restate.normals at step 1 with the PHOTO's kx, ky; a node without z
               or n has ao = 1, vis = 1
  occlusion .. directions (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1) (1,0) (1,1); k = 1 .. ao_reach: q = node + k d, outside / invalid q skipped; D = P_q - P_0,
               l2 = (Dx^2 + Dy^2) + Dz^2, hgt = ((Dx nx + Dy ny) + Dz nz) / sqrt(l2), fall = 1 - l2 / (rad rad), rad = ao_radius z_0, rise = hgt - ao_bias,
               term = max0(rise) max0(fall) (max0(v) = v if v > 0 else 0); occ_d = the largest term > 0; sum in order from 0; open = 1 - (ao_strength sum) / 8,
               ao = fp32(max0(open))
  shadow ..... gx = (Lx / kx + x0 Lz) gw, gy = -((Ly / ky + y0 Lz) gh); both 0 or either not finite: lit; major axis c = x if |gx| >= |gy| else y, m = |g_c|,
               sx = gx / m, sy = gy / m; k = 1 .. shadow_reach: q = (i + floor(k sy + 0.5), j + floor(k sx + 0.5)), off the grid: lit;
               t = ((z_0 k_c) (cq - c_0)) / (L_c + (Lz k_c) cq), zr = z_0 - t Lz, t or zr not > 0: lit; z_q valid, z_q < zr (1 - bias) and
               (thickness inf or zr - z_q <= thickness zr): vis = 0
  shading .... relight's pixel with a, s_v = the planes at the pixel's centre: shade = ambient a + (diffuse max0(d)) s_v, spec = 255 ((specular sp) s_v)"""
from unittest import mock

import numpy as np

from tests import normals_restate as nr
from tests import refocus_restate as rr

MAX_REACH = 32
AO_DIRECTIONS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))
DEFAULTS = dict(shadow_reach=32, shadow_bias=0.02, shadow_thickness=float("inf"), ao_reach=8, ao_radius=0.25, ao_bias=0.05, ao_strength=1.0)


def grid_geometry(p, gh: int, gw: int, kx: float, ky: float, space="inverse", min_depth=50.0, max_depth=100.0, edge_ratio=2.0):
    """-> (z [gh,gw] NaN where invalid, P [gh,gw,3], n [gh,gw,3], valid [gh,gw]): normals_restate.normals on the grid, at a step of one node, under the
    photo's camera scales instead of the grid's own aspect"""
    with mock.patch.object(nr, "camera_scales", lambda H, W, fov_deg: (kx, ky)):
        n, valid, P = nr.normals(p, gh, gw, space=space, min_depth=min_depth, max_depth=max_depth, step=1, edge_ratio=edge_ratio)
    return -P[..., 2], P, n, valid


def ambient_occlusion(z, P, n, valid, ao_reach=8, ao_radius=0.25, ao_bias=0.05, ao_strength=1.0) -> np.ndarray:
    """-> ao fp32 [gh,gw]"""
    total = np.zeros(z.shape)
    with np.errstate(all="ignore"):
        rad = np.float64(ao_radius) * z
        rad2 = rad * rad
        for di, dj in AO_DIRECTIONS:
            occ = np.zeros(z.shape)
            for k in range(1, int(ao_reach) + 1):
                zq = nr.shifted(z, k * di, k * dj)
                D = [nr.shifted(P[..., c], k * di, k * dj) - P[..., c] for c in range(3)]
                l2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
                hgt = ((D[0] * n[..., 0] + D[1] * n[..., 1]) + D[2] * n[..., 2]) / np.sqrt(l2)
                fall, rise = 1.0 - l2 / rad2, hgt - np.float64(ao_bias)
                term = np.where(rise > 0.0, rise, 0.0) * np.where(fall > 0.0, fall, 0.0)
                occ = np.where(~np.isnan(zq) & (term > occ), term, occ)
            total = total + occ
        opened = 1.0 - (np.float64(ao_strength) * total) / 8.0
    return np.where(valid, np.where(opened > 0.0, opened, 0.0), 1.0).astype(np.float32)


def cast_shadows(z, valid, kx: float, ky: float, light_dirs, shadow_reach=32, shadow_bias=0.02, shadow_thickness=float("inf")) -> np.ndarray:
    """-> vis fp32 [V,gh,gw] of 0.0 / 1.0"""
    gh, gw = z.shape
    I, J = np.mgrid[0:gh, 0:gw]
    x0, y0 = 2.0 * (J + 0.5) / np.float64(gw) - 1.0, 1.0 - 2.0 * (I + 0.5) / np.float64(gh)
    kx, ky, bias, thick = np.float64(kx), np.float64(ky), np.float64(shadow_bias), np.float64(shadow_thickness)
    planes = []
    with np.errstate(all="ignore"):
        for L in nr.unit_lights(light_dirs):
            gx, gy = (L[0] / kx + x0 * L[2]) * np.float64(gw), -((L[1] / ky + y0 * L[2]) * np.float64(gh))
            active = valid & ~((gx == 0.0) & (gy == 0.0)) & np.isfinite(gx) & np.isfinite(gy)
            x_major = np.abs(gx) >= np.abs(gy)
            m = np.where(x_major, np.abs(gx), np.abs(gy))
            sx, sy = gx / m, gy / m
            kc, c0, Lc = np.where(x_major, kx, ky), np.where(x_major, x0, y0), np.where(x_major, L[0], L[1])
            zk, Lk = z * kc, L[2] * kc
            vis = np.ones(z.shape, np.float32)
            for k in range(1, int(shadow_reach) + 1):
                di = np.where(active, np.floor(np.float64(k) * sy + 0.5), 0.0).astype(np.int64)
                dj = np.where(active, np.floor(np.float64(k) * sx + 0.5), 0.0).astype(np.int64)
                qi, qj = I + di, J + dj
                active = active & (qi >= 0) & (qi < gh) & (qj >= 0) & (qj < gw)
                cq = np.where(x_major, 2.0 * (qj + 0.5) / np.float64(gw) - 1.0, 1.0 - 2.0 * (qi + 0.5) / np.float64(gh))
                t = (zk * (cq - c0)) / (Lc + Lk * cq)
                zr = z - t * L[2]
                active = active & (t > 0.0) & (zr > 0.0)
                zq = z[np.clip(qi, 0, gh - 1), np.clip(qj, 0, gw - 1)]
                hit = active & ~np.isnan(zq) & (zq < zr * (1.0 - bias)) & (np.isinf(thick) | (zr - zq <= thick * zr))
                vis[hit] = 0.0
                active = active & ~hit
            planes.append(vis)
    return np.stack(planes)


def occlusion(p, H: int, W: int, light_dirs=None, grid_hw=None, space="inverse", fov_deg=50.0, min_depth=50.0, max_depth=100.0, edge_ratio=2.0, shadow_reach=32,
              shadow_bias=0.02, shadow_thickness=float("inf"), ao_reach=8, ao_radius=0.25, ao_bias=0.05, ao_strength=1.0):
    """map [h,w] under an H x W photo -> (ao fp32 [gh,gw], vis fp32 [V,gh,gw] or None, valid nodes [gh,gw])"""
    p = np.asarray(p)
    gh, gw = p.shape if grid_hw is None else grid_hw
    kx, ky = nr.camera_scales(H, W, fov_deg)
    z, P, n, valid = grid_geometry(p, gh, gw, kx, ky, space, min_depth, max_depth, edge_ratio)
    ao = ambient_occlusion(z, P, n, valid, ao_reach, ao_radius, ao_bias, ao_strength)
    vis = None if light_dirs is None else cast_shadows(z, valid, kx, ky, light_dirs, shadow_reach, shadow_bias, shadow_thickness)
    return ao, vis, valid


def shade(photo: np.ndarray, n, valid, P, light_dirs, ao=None, vis=None, ambient=0.35, diffuse=0.9, specular=0.0, shininess_log2=4) -> np.ndarray:
    """uint8 BGR [H,W,3], normals_restate.normals()'s results at the photo's size and the planes (None: the constant 1) -> uint8 [V,H,W,3]"""
    H, W = photo.shape[:2]
    colour = photo.astype(np.float64)
    frames = []
    with np.errstate(all="ignore"):
        amb = np.float64(ambient) if ao is None else np.float64(ambient) * rr.map_at_pixels(ao, H, W)
        if specular > 0.0:
            plen = np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])
            view = [-P[..., c] / plen for c in range(3)]
        for v, l in enumerate(nr.unit_lights(light_dirs)):
            s = np.float64(1.0) if vis is None else rr.map_at_pixels(vis[v], H, W)
            dot = (n[..., 0] * l[0] + n[..., 1] * l[1]) + n[..., 2] * l[2]
            sh = amb + (np.float64(diffuse) * np.where(dot > 0.0, dot, 0.0)) * s
            spec = np.zeros_like(sh)
            if specular > 0.0:
                hv = [l[c] + view[c] for c in range(3)]
                hlen = np.sqrt((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2])
                nh = (n[..., 0] * (hv[0] / hlen) + n[..., 1] * (hv[1] / hlen)) + n[..., 2] * (hv[2] / hlen)
                sp = np.where(nh > 0.0, nh, 0.0)
                for _ in range(int(shininess_log2)):
                    sp = sp * sp
                spec = 255.0 * ((np.float64(specular) * sp) * s)
            out = np.minimum(255.0, np.floor((colour * sh[..., None] + spec[..., None]) + 0.5))
            frames.append(np.where(valid[..., None], out, colour).astype(np.uint8))
    return np.stack(frames)


def shade_images(p, photo: np.ndarray, light_dirs, ambient=0.35, diffuse=0.9, specular=0.0, shininess_log2=4, grid_hw=None, step=None, space="inverse",
                 fov_deg=50.0, min_depth=50.0, max_depth=100.0, edge_ratio=2.0, **occl):
    """map [h,w] and uint8 BGR photo [H,W,3] -> (frames uint8 [V,H,W,3], ao fp32 [gh,gw], vis fp32 [V,gh,gw]); a plane whose factor is off is not used"""
    H, W = photo.shape[:2]
    camera = dict(space=space, fov_deg=fov_deg, min_depth=min_depth, max_depth=max_depth, edge_ratio=edge_ratio)
    occl = {**DEFAULTS, **occl}
    ao, vis, _ = occlusion(p, H, W, light_dirs, grid_hw, **camera, **occl)
    n, valid, P = nr.normals(p, H, W, step=step, **camera)
    use_ao, use_vis = occl["ao_reach"] > 0 and occl["ao_strength"] > 0.0, occl["shadow_reach"] > 0
    return shade(photo, n, valid, P, light_dirs, ao if use_ao else None, vis if use_vis else None, ambient, diffuse, specular, shininess_log2), ao, vis
