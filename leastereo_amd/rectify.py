"""The host side of rectification: camera models, Bouguet's stereo rectification, the
calibration block of ``kernels.rectify_u8`` (lea_rectify_pair_u8) and calibration files.
Float64 numpy throughout; the images themselves are rectified on the device.

Conventions: a point in the left camera's frame X_l is X_r = R X_l + T in the right one's;
``size`` and ``out_size`` are (height, width); pixel (0, 0) is the centre of the top-left pixel,
as in OpenCV."""
from __future__ import annotations

import json
import os

import numpy as np

CALIB_FLOATS = 24
MODELS = ("pinhole", "fisheye")


class CameraModel:
    """A raw camera: ``K`` 3 x 3 (no skew) and ``dist`` in OpenCV's order -- pinhole:
    k1 k2 p1 p2 [k3 [k4 k5 k6]] (4, 5 or 8 coefficients, the rational model); fisheye:
    k1 k2 k3 k4 (the equidistant model)."""

    def __init__(self, K, dist=(0.0, 0.0, 0.0, 0.0), model: str = "pinhole"):
        K = np.asarray(K, np.float64)
        dist = np.asarray(dist, np.float64).reshape(-1)
        if model not in MODELS:
            raise ValueError(f"CameraModel: model {model!r} is not one of {MODELS}")
        if K.shape != (3, 3) or not np.isfinite(K).all():
            raise ValueError(f"CameraModel: K must be a finite 3 x 3 matrix, got shape {K.shape}")
        if K[0, 1] != 0.0:
            raise ValueError(f"CameraModel: skew {K[0, 1]} is not supported (K[0, 1] must be 0)")
        if K[1, 0] != 0.0 or tuple(K[2]) != (0.0, 0.0, 1.0) or not (K[0, 0] > 0 and K[1, 1] > 0):
            raise ValueError("CameraModel: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with fx, fy > 0")
        want = (4, 5, 8) if model == "pinhole" else (4,)
        if dist.size not in want or not np.isfinite(dist).all():
            raise ValueError(f"CameraModel: a {model} camera takes {' or '.join(map(str, want))} finite distortion "
                             f"coefficients, got {dist.size}")
        self.K, self.dist, self.model = K, dist, model

    fx = property(lambda self: float(self.K[0, 0]))
    fy = property(lambda self: float(self.K[1, 1]))
    cx = property(lambda self: float(self.K[0, 2]))
    cy = property(lambda self: float(self.K[1, 2]))

    def coefficients(self) -> np.ndarray:
        """The eight floats k[8] of the calibration block (zeros where the model has none)."""
        k = np.zeros(8, np.float64)
        k[:self.dist.size] = self.dist
        return k


def rodrigues(om) -> np.ndarray:
    """The rotation matrix of the rotation vector ``om`` (axis times angle)."""
    om = np.asarray(om, np.float64).reshape(3)
    th = float(np.linalg.norm(om))
    Kx = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if th < 1e-8:  # sin(th) / th and (1 - cos(th)) / th^2 to second order
        return np.eye(3) + Kx + 0.5 * (Kx @ Kx)
    return np.eye(3) + (np.sin(th) / th) * Kx + ((1.0 - np.cos(th)) / (th * th)) * (Kx @ Kx)


def rodrigues_inv(R) -> np.ndarray:
    """The rotation vector of a rotation matrix (angles below pi)."""
    R = np.asarray(R, np.float64)
    if R.shape != (3, 3) or not np.allclose(R @ R.T, np.eye(3), atol=1e-6) or np.linalg.det(R) < 0:
        raise ValueError("rodrigues_inv: not a rotation matrix")
    u, _, vt = np.linalg.svd(R)  # the nearest rotation: a calibration file holds rounded numbers
    R = u @ vt
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * float(np.linalg.norm(v)), 0.5 * (float(np.trace(R)) - 1.0)
    th = float(np.arctan2(s, c))
    if s < 1e-8:
        if c < 0:
            raise ValueError("rodrigues_inv: a rotation by pi has no unique half rotation")
        return 0.5 * v
    return v * (th / (2.0 * s))


class Rectification:
    """What ``stereo_rectify`` returns: ``R1``, ``R2`` (raw camera frame to rectified frame),
    ``focal`` (pixels), ``baseline``, the new principal point (``cx``, ``cy``) of the left view
    and ``cx_right`` of the right one, ``size`` and ``out_size`` (height, width), and the two
    cameras."""

    def __init__(self, cam_l, cam_r, R1, R2, focal, baseline, cx, cy, cx_right, size, out_size):
        self.cam_l, self.cam_r = cam_l, cam_r
        self.R1, self.R2 = R1, R2
        self.focal, self.baseline = float(focal), float(baseline)
        self.cx, self.cy, self.cx_right = float(cx), float(cy), float(cx_right)
        self.size, self.out_size = tuple(int(v) for v in size), tuple(int(v) for v in out_size)

    def new_camera_matrices(self):
        """(K_new,left, K_new,right)."""
        f = self.focal
        return (np.array([[f, 0.0, self.cx], [0.0, f, self.cy], [0.0, 0.0, 1.0]]),
                np.array([[f, 0.0, self.cx_right], [0.0, f, self.cy], [0.0, 0.0, 1.0]]))

    def calib64(self) -> np.ndarray:
        """The calibration block in float64, [2, 24]: per view M[9] = R_k^T K_new,k^-1, fx, fy,
        cx, cy of the raw camera, model (0 pinhole, 1 fisheye), k[8], two zeros."""
        out = np.zeros((2, CALIB_FLOATS), np.float64)
        for v, (cam, Rk, Kn) in enumerate(zip((self.cam_l, self.cam_r), (self.R1, self.R2),
                                              self.new_camera_matrices())):
            out[v, :9] = (Rk.T @ np.linalg.inv(Kn)).reshape(-1)
            out[v, 9:13] = cam.fx, cam.fy, cam.cx, cam.cy
            out[v, 13] = float(MODELS.index(cam.model))
            out[v, 14:22] = cam.coefficients()
        return out

    def calib(self) -> np.ndarray:
        """float32 [1, 2, 24]: what ``kernels.rectify_u8(calib=...)`` takes."""
        return self.calib64().astype(np.float32)[None]

    def q(self, origin=(0, 0)) -> np.ndarray:
        """The reprojection matrix of the rectified pair (``pointcloud.q_matrix``) for a map
        whose pixel (0, 0) lies at ``origin`` = (x0, y0) of the rectified left image."""
        from .pointcloud import q_matrix
        return q_matrix(self.focal, self.baseline, self.cx, self.cy, self.cx_right, origin)

    def projections(self):
        """(P1, P2), 3 x 4: rectified-frame points of the left camera to the two rectified images."""
        K1, K2 = self.new_camera_matrices()
        P1 = np.hstack([K1, np.zeros((3, 1))])
        P2 = np.hstack([K2, K2 @ np.array([[-self.baseline], [0.0], [0.0]])])
        return P1, P2


def stereo_rectify(cam_l: CameraModel, cam_r: CameraModel, R, T, size, out_size=None, focal: float = None,
                   zero_disparity: bool = True) -> Rectification:
    """Bouguet's rectification of a horizontal rig (the algorithm of OpenCV's stereoRectify,
    without its ``alpha`` zoom): both cameras are turned by half of ``R`` each, then together so
    that the baseline lies along -x.  ``focal`` (default min(fy_l, fy_r) scaled by Ho / H) and
    ``out_size`` (default ``size``) are the tools to shrink or grow the border."""
    R = np.asarray(R, np.float64)
    T = np.asarray(T, np.float64).reshape(-1)
    if T.shape != (3,) or not np.isfinite(T).all() or not np.linalg.norm(T) > 0:
        raise ValueError("stereo_rectify: T must be a finite non-zero 3-vector")
    H, W = (int(v) for v in size)
    Ho, Wo = (H, W) if out_size is None else (int(v) for v in out_size)
    if min(H, W, Ho, Wo) < 1:
        raise ValueError(f"stereo_rectify: bad size {size} or out_size {out_size}")
    om = rodrigues_inv(R)
    r_r = rodrigues(-0.5 * om)
    t = r_r @ T
    if abs(t[1]) > abs(t[0]):
        raise ValueError(f"stereo_rectify: a vertical rig (|t_y| = {abs(t[1]):g} > |t_x| = {abs(t[0]):g}) is not "
                         f"supported")
    if t[0] > 0:
        raise ValueError(f"stereo_rectify: t_x = {t[0]:g} > 0 after the half rotation: the views are swapped "
                         f"(X_r = R X_l + T puts the right camera at -R^T T)")
    nt = float(np.linalg.norm(t))
    uu = np.array([np.sign(t[0]), 0.0, 0.0])
    ww = np.cross(t, uu)
    nw = float(np.linalg.norm(ww))
    if nw > 0.0:
        ww = ww * (np.arccos(min(abs(t[0]) / nt, 1.0)) / nw)
    wR = rodrigues(ww)
    R1, R2 = wR @ r_r.T, wR @ r_r
    if focal is None:
        focal = min(cam_l.fy, cam_r.fy) * Ho / H
    focal = float(focal)
    if not (np.isfinite(focal) and focal > 0):
        raise ValueError(f"stereo_rectify: focal {focal} must be a finite number > 0")
    c = []
    for cam, Rk in ((cam_l, R1), (cam_r, R2)):
        z = Rk @ np.array([0.0, 0.0, 1.0])
        if not z[2] > 0:
            raise ValueError("stereo_rectify: a camera looks away from the rectified axis")
        c.append(np.array([Wo / W * cam.cx, Ho / H * cam.cy]) - focal * z[:2] / z[2])
    cy = 0.5 * (c[0][1] + c[1][1])
    cx_l, cx_r = c[0][0], c[1][0]
    if zero_disparity:
        cx_l = cx_r = 0.5 * (cx_l + cx_r)
    return Rectification(cam_l, cam_r, R1, R2, focal, nt, cx_l, cy, cx_r, (H, W), (Ho, Wo))


def save_calibration(path, cam_l: CameraModel, cam_r: CameraModel, R, T, size) -> None:
    """``.json`` or ``.npz`` with the keys K1, D1, K2, D2, R, T, size (height, width), model."""
    if cam_l.model != cam_r.model:
        raise ValueError("save_calibration: one file holds one lens model")
    d = dict(K1=cam_l.K, D1=cam_l.dist, K2=cam_r.K, D2=cam_r.dist, R=np.asarray(R, np.float64),
             T=np.asarray(T, np.float64).reshape(3), size=np.asarray(size, np.int64), model=cam_l.model)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".json":
        with open(path, "w") as f:
            json.dump({k: (v if isinstance(v, str) else v.tolist()) for k, v in d.items()}, f, indent=1)
    elif ext == ".npz":
        with open(path, "wb") as f:
            np.savez(f, **d)
    else:
        raise ValueError(f"save_calibration: {path}: .json or .npz")


def load_calibration(path):
    """(cam_l, cam_r, R, T, size) of a file ``save_calibration`` wrote (``model`` may be absent:
    pinhole)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".json":
        with open(path) as f:
            d = json.load(f)
    elif ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
    else:
        raise ValueError(f"load_calibration: {path}: .json or .npz")
    missing = [k for k in ("K1", "D1", "K2", "D2", "R", "T", "size") if k not in d]
    if missing:
        raise ValueError(f"load_calibration: {path} lacks {', '.join(missing)}")
    model = str(np.asarray(d.get("model", "pinhole")).reshape(-1)[0])
    size = tuple(int(v) for v in np.asarray(d["size"]).reshape(-1))
    if len(size) != 2:
        raise ValueError(f"load_calibration: {path}: size must be (height, width)")
    return (CameraModel(d["K1"], d["D1"], model), CameraModel(d["K2"], d["D2"], model),
            np.asarray(d["R"], np.float64).reshape(3, 3), np.asarray(d["T"], np.float64).reshape(3), size)


class Rectifier:
    """A ``Rectification`` on the device: the calibration block lives in device memory, so a
    captured call replays with whatever ``update`` last wrote there."""

    def __init__(self, rect: Rectification, device="cuda", fill: int = 0, want_valid: bool = True):
        import torch
        self.rect, self.device, self.fill, self.want_valid = rect, device, int(fill), bool(want_valid)
        self.calib = torch.from_numpy(rect.calib()).to(device)

    def update(self, rect: Rectification) -> None:
        """Overwrite the device block in place (same sizes): the next call and the next replay use it."""
        import torch
        if rect.size != self.rect.size or rect.out_size != self.rect.out_size:
            raise ValueError(f"Rectifier.update: sizes {rect.size} -> {rect.out_size} differ from "
                             f"{self.rect.size} -> {self.rect.out_size}")
        self.calib.copy_(torch.from_numpy(rect.calib()).to(self.device, non_blocking=False))
        self.rect = rect

    def _images(self, left_u8, right_u8):
        import torch
        out = []
        for a in (left_u8, right_u8):
            if not isinstance(a, torch.Tensor):
                a = np.asarray(a)  # a decoded image is read-only: torch wants a buffer it may write to
                a = torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else np.array(a))
            out.append(a.to(self.device))
        if tuple(out[0].shape[-3:-1]) != self.rect.size:
            raise ValueError(f"Rectifier: images of {tuple(out[0].shape[-3:-1])}, calibrated for {self.rect.size}")
        return out

    def __call__(self, left_u8, right_u8, want_maps: bool = False):
        """``kernels.rectify_u8`` of a pair (numpy or tensors, [H, W, ps] or [B, H, W, ps])."""
        from . import kernels
        left, right = self._images(left_u8, right_u8)
        return kernels.rectify_u8(left, right, calib=self.calib, size=self.rect.out_size, fill=self.fill,
                                  want_valid=self.want_valid, want_maps=want_maps)

    def maps(self):
        """The map stage run once: float32 [2, 2, Ho, Wo] on the device (view, then x / y), the
        coordinates every call with this calibration uses."""
        import torch
        from . import kernels
        px = torch.zeros((1, 1, 1, 3), device=self.device, dtype=torch.uint8)
        return kernels.rectify_u8(px, px.clone(), calib=self.calib, size=self.rect.out_size, want_valid=False,
                                  want_maps=True).maps[0]
