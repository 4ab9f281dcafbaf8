"""The camera of the reference's 3D viewer on the host, in fp64 numpy: Orbit_Camera (demo_helpers/3dviewer/orbitcam.js) and the MAT4 pieces it uses
(linalg.js), restated, and the view-projection matrix render_3d builds from them (index.html:1190-1202). Matrices are the reference's: 16 numbers,
row-major, applied as row vector times matrix (clip = [x, y, z, 1] M) - what postprocess.render_mesh / mdpt_post_render take.

On top of it, two ways to make several views at once: swing_views (a closed ellipse around a pose: the looping "3D photo" clip) and stereo_views
(a left / right pair). Nothing here touches the device."""

from __future__ import annotations

import math

import numpy as np

# orbitcam.js:28-34, :184-185 and index.html:397, :463
ZOOM_SENSITIVITY, ZOOM_MIN, ZOOM_MAX, ORBIT_SENSITIVITY, SHIFT_SENSITIVITY = 0.95, 0.05, 500.0, 0.005, 0.005
NEAR_DIST, FAR_DIST = ZOOM_MIN * 0.25, ZOOM_MAX * 2
VIEWER_DISTANCE, VIEWER_VIEW_FOV_DEG = 50.0, 60.0


def _vec(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float64).reshape(3).copy()


def _norm(v: np.ndarray) -> np.ndarray:
    """VEC3.norm: vectors shorter than 1e-5 become zero"""
    length = math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    return v / length if length > 0.00001 else np.zeros(3)


def _norm_cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return _norm(np.cross(a, b))


def rotate_axis_angle(point, axis, angle_rad: float) -> np.ndarray:
    """Rodrigues' formula as linalg.js:44-70 adds its three terms"""
    point, axis = _vec(point), _vec(axis)
    cos, sin = math.cos(angle_rad), math.sin(angle_rad)
    return cos * point + sin * np.cross(axis, point) + ((1.0 - cos) * float(axis @ point)) * axis


def look_at(camera_xyz, target_xyz, up_axis) -> np.ndarray:
    """MAT4.look_at (linalg.js:126-137): rows x, y, z axes and the camera position -> [4,4]"""
    camera_xyz = _vec(camera_xyz)
    z_axis = _norm(camera_xyz - _vec(target_xyz))
    x_axis = _norm_cross(_vec(up_axis), z_axis)
    y_axis = _norm_cross(z_axis, x_axis)
    m = np.zeros((4, 4))
    m[0, :3], m[1, :3], m[2, :3], m[3, :3], m[3, 3] = x_axis, y_axis, z_axis, camera_xyz, 1.0
    return m


def perspective(fov_rad: float, aspect: float, near: float = NEAR_DIST, far: float = FAR_DIST) -> np.ndarray:
    """MAT4.perspective (linalg.js:89-99)"""
    f = math.tan(0.5 * (math.pi - fov_rad))
    range_inv = 1.0 / (near - far)
    return np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (near + far) * range_inv, -1], [0, 0, near * far * range_inv * 2, 0]], dtype=np.float64)


def orthographic(left: float, right: float, bottom: float, top: float, near: float, far: float) -> np.ndarray:
    """MAT4.orthographic (linalg.js:76-87)"""
    return np.array([[2 / (right - left), 0, 0, 0], [0, 2 / (top - bottom), 0, 0], [0, 0, 2 / (near - far), 0],
                     [(left + right) / (left - right), (bottom + top) / (bottom - top), (near + far) / (near - far), 1]], dtype=np.float64)


def rotate_x(angle_rad: float) -> np.ndarray:
    """MAT4.rotate_x (linalg.js:101-111)"""
    cos, sin = math.cos(angle_rad), math.sin(angle_rad)
    return np.array([[1, 0, 0, 0], [0, cos, sin, 0], [0, -sin, cos, 0], [0, 0, 0, 1]], dtype=np.float64)


class OrbitCamera:
    """Orbit_Camera without its canvas: the pose (distance, origin, origin_offset, position_norm, up, right) and the moves of the viewer's mouse
    handlers. rotate / translate take the pixels of a drag, zoom the sign of a wheel step, as the JavaScript does."""

    def __init__(self, initial_distance: float = VIEWER_DISTANCE, world_up=(0, 1, 0), world_right=(1, 0, 0)):
        self._initial_distance = float(initial_distance)
        self.distance = float(initial_distance)
        self.world_up, self.world_right = _norm(_vec(world_up)), _norm(_vec(world_right))
        self.reset()

    def reset(self) -> None:
        """orbitcam.js:44-58: panning and orientation back to the start (the distance stays, as there)"""
        self.origin, self.origin_offset = np.zeros(3), np.zeros(3)
        self.up, self.right = self.world_up.copy(), self.world_right.copy()
        self.position_norm = (self.origin + self.origin_offset) - _norm_cross(self.up, self.right)

    def copy(self) -> "OrbitCamera":
        other = OrbitCamera(self._initial_distance, self.world_up, self.world_right)
        other.distance = self.distance
        for name in ("origin", "origin_offset", "up", "right", "position_norm"):
            setattr(other, name, getattr(self, name).copy())
        return other

    def set_origin_offset(self, camera_offset: float, tilt_rad: float) -> None:
        self.origin_offset[1] = -camera_offset * math.sin(tilt_rad)
        self.origin_offset[2] = -camera_offset * math.cos(tilt_rad)

    def snap_to_axis(self, snap_x: bool = False, snap_y: bool = False, snap_z: bool = False, invert: bool = False) -> None:
        value = -1.0 if invert else 1.0
        if snap_x:
            self.position_norm, self.up, self.right = _vec([value, 0, 0]), _vec([0, 1, 0]), _vec([0, 0, -value])
        elif snap_y:
            self.position_norm, self.up, self.right = _vec([0, value, 0]), _vec([0, 0, -value]), _vec([1, 0, 0])
        elif snap_z:
            self.position_norm, self.up, self.right = _vec([0, 0, value]), _vec([0, 1, 0]), _vec([value, 0, 0])

    def translate(self, dx: float, dy: float, dz: float = 0.0) -> None:
        """orbitcam.js:96-116: the origin moves along the camera's own axes"""
        self.origin = self.origin + (self.up * (dy * SHIFT_SENSITIVITY) + self.right * (-dx * SHIFT_SENSITIVITY)) + self.position_norm * (-dz * SHIFT_SENSITIVITY)

    def rotate(self, dx: float, dy: float) -> None:
        """orbitcam.js:120-146: up / down about the camera's right axis, then left / right about the world's up axis"""
        angle_x, angle_y = -dx * ORBIT_SENSITIVITY, -dy * ORBIT_SENSITIVITY
        pos = rotate_axis_angle(self.position_norm, self.right, angle_y)
        pos = rotate_axis_angle(pos, self.world_up, angle_x)
        new_right = rotate_axis_angle(self.right, self.world_up, angle_x)
        self.position_norm = _norm(pos)
        self.right = _norm(new_right)
        self.up = _norm_cross(new_right, -pos)

    def zoom(self, zoom_delta: float) -> None:
        self.distance *= ZOOM_SENSITIVITY if zoom_delta > 0 else 1.0 / ZOOM_SENSITIVITY
        self.distance = max(ZOOM_MIN, min(ZOOM_MAX, self.distance))

    def world_to_view(self) -> np.ndarray:
        """get_world_to_view_mat4 (orbitcam.js:162-175): the inverse of the look-at matrix from the camera's position to the origin"""
        real_origin = self.origin + self.origin_offset
        return np.linalg.inv(look_at(self.position_norm * self.distance + real_origin, real_origin, self.up))

    def view_to_clip(self, fov_rad: float, aspect: float = 1.0, orthographic_camera: bool = False) -> np.ndarray:
        """get_view_to_clipspace_mat4 (orbitcam.js:179-203)"""
        if not orthographic_camera:
            return perspective(fov_rad, aspect, NEAR_DIST, FAR_DIST)
        zoom = (self.distance + (self.origin + self.origin_offset)[2] * 0.5) * 0.5
        return orthographic(-zoom * aspect, zoom * aspect, -zoom, zoom, -FAR_DIST, FAR_DIST)


def viewer_view_proj(camera: OrbitCamera | None = None, tilt_deg: float = 0.0, view_offset: float = 0.5, min_depth: float = 50.0, max_depth: float = 100.0,
                     view_fov_deg: float = VIEWER_VIEW_FOV_DEG, aspect: float = 1.0, orthographic: bool = False) -> np.ndarray:
    """index.html:1190-1202 -> float64 [16]: tilt . (view . proj), after the origin offset rule of :1191-1195 has been applied to `camera` (as
    render_3d applies it on every frame; None: a camera in the viewer's start pose). Defaults are the viewer's controls as it starts; min_depth /
    max_depth are the mesh's (postprocess.MESH_MIN_DEPTH / MESH_MAX_DEPTH), aspect the output's width / height."""
    camera = OrbitCamera() if camera is None else camera
    tilt_rad = float(tilt_deg) * (math.pi / 180.0)
    near_offset = min_depth * (view_offset * 2.0)
    far_offset = min_depth + ((max_depth - min_depth) * (view_offset * 2 - 1))
    camera.set_origin_offset(far_offset if view_offset > 0.5 else near_offset, tilt_rad)
    view = camera.world_to_view()
    proj = camera.view_to_clip(float(view_fov_deg) * (math.pi / 180.0), float(aspect), bool(orthographic))
    return (rotate_x(-tilt_rad) @ (view @ proj)).reshape(16)


def swing_views(n: int, yaw_deg: float = 8.0, pitch_deg: float = 4.0, camera: OrbitCamera | None = None, **viewer) -> np.ndarray:
    """n matrices [n,16] on a closed ellipse around `camera`'s pose (None: the start pose): view k orbits by (yaw_deg cos t, pitch_deg sin t),
    t = 2 pi k / n, so the clip loops. **viewer goes to viewer_view_proj."""
    n = int(n)
    if n < 1:
        raise ValueError(f"swing_views: need at least one view, got {n}")
    base = OrbitCamera() if camera is None else camera
    out = np.empty((n, 16))
    for k in range(n):
        cam = base.copy()
        t = 2.0 * math.pi * k / n
        cam.rotate(math.radians(yaw_deg) * math.cos(t) / ORBIT_SENSITIVITY, math.radians(pitch_deg) * math.sin(t) / ORBIT_SENSITIVITY)
        out[k] = viewer_view_proj(cam, **viewer)
    return out


def stereo_views(baseline: float, camera: OrbitCamera | None = None, **viewer) -> np.ndarray:
    """the left and the right eye [2,16]: `camera`'s pose moved by -/+ baseline / 2 (world units) along its right axis, looking the same way"""
    base = OrbitCamera() if camera is None else camera
    out = np.empty((2, 16))
    for k, side in enumerate((-0.5, 0.5)):
        cam = base.copy()
        cam.origin = cam.origin + cam.right * (side * float(baseline))
        out[k] = viewer_view_proj(cam, **viewer)
    return out
