"""The host side of the point cloud: the reprojection matrix of a rectified rig and the PLY
file.  The cloud itself is made on the device by ``kernels.reproject``
(lea_disparity_pointcloud_f32)."""
from __future__ import annotations

import numpy as np


def q_matrix(focal: float, baseline: float, cx: float, cy: float, cx_right: float = None, origin=(0, 0)) -> np.ndarray:
    """The float64 4 x 4 reprojection matrix of a rectified pair, for a disparity map whose
    pixel (0, 0) lies at ``origin`` = (x0, y0) of the calibrated left image (a crop or a pad
    keeps the camera's own calibration this way):

        Z = f B / (d - (cx - cx_right)),   X = (x + x0 - cx) Z / f,   Y = (y + y0 - cy) Z / f

    ``focal`` f in pixels, ``baseline`` B in the unit of the cloud, (``cx``, ``cy``) the left
    principal point, ``cx_right`` the right one's x (None: the same as ``cx``).  With
    h = Q (x, y, d, 1) the point is (h0, h1, h2) / h3."""
    focal, baseline = float(focal), float(baseline)
    if not (np.isfinite(focal) and focal > 0 and np.isfinite(baseline) and baseline > 0):
        raise ValueError(f"q_matrix: focal {focal} and baseline {baseline} must be finite numbers > 0")
    x0, y0 = (float(v) for v in origin)
    shift = 0.0 if cx_right is None else float(cx) - float(cx_right)
    Q = np.zeros((4, 4), np.float64)
    Q[0, 0], Q[0, 3] = 1.0, x0 - float(cx)
    Q[1, 1], Q[1, 3] = 1.0, y0 - float(cy)
    Q[2, 3] = focal
    Q[3, 2], Q[3, 3] = 1.0 / baseline, -shift / baseline
    return Q


_PLY_TYPES = {"float": "<f4", "uchar": "u1"}


def _ply_dtype(rgb: bool, normals: bool) -> np.dtype:
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields)


def ply_header(n: int, rgb: bool, normals: bool) -> str:
    """The header ``write_ply`` writes for ``n`` vertices."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    for name, t in _ply_dtype(rgb, normals).descr:
        lines.append(f"property {'float' if t == '<f4' else 'uchar'} {name}")
    return "\n".join(lines + ["end_header"]) + "\n"


def write_ply(path, xyz, rgb=None, normals=None) -> int:
    """Binary little-endian PLY of the points ``xyz`` [N, 3] float32: ``float x y z``, then
    ``float nx ny nz`` with ``normals`` [N, 3] float32, then ``uchar red green blue`` with
    ``rgb`` [N, 3] uint8.  The floats are written bit for bit.  Returns the bytes written."""
    xyz = np.asarray(xyz)
    n = xyz.shape[0] if xyz.ndim == 2 else -1
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.dtype != np.float32:
        raise ValueError(f"write_ply: xyz must be float32 [N, 3], got {xyz.dtype} {xyz.shape}")
    if normals is not None:
        normals = np.asarray(normals)
        if normals.shape != (n, 3) or normals.dtype != np.float32:
            raise ValueError(f"write_ply: normals must be float32 [{n}, 3], got {normals.dtype} {normals.shape}")
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.shape != (n, 3) or rgb.dtype != np.uint8:
            raise ValueError(f"write_ply: rgb must be uint8 [{n}, 3], got {rgb.dtype} {rgb.shape}")
    rec = np.empty(n, _ply_dtype(rgb is not None, normals is not None))
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = xyz[:, k]
    if normals is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            rec[name] = normals[:, k]
    if rgb is not None:
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = rgb[:, k]
    data = ply_header(n, rgb is not None, normals is not None).encode("ascii") + rec.tobytes()
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read_ply(path):
    """Reads what ``write_ply`` writes (binary little-endian, one vertex element of float and
    uchar properties): (xyz, rgb, normals), ``None`` for what the file does not hold."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_ply: {path} has no PLY header")
    lines = data[:end].decode("ascii").split("\n")[1:]
    body = data[end + len(b"end_header\n"):]
    if not lines or lines[0] != "format binary_little_endian 1.0":
        raise ValueError(f"read_ply: {path}: only binary_little_endian 1.0 is read")
    n, fields = None, []
    for line in lines[1:]:
        word = line.split()
        if not word or word[0] == "comment":
            continue
        if word[0] == "element":
            if n is not None or word[1] != "vertex":
                raise ValueError(f"read_ply: {path}: one vertex element only, got '{line}'")
            n = int(word[2])
        elif word[0] == "property" and n is not None and len(word) == 3 and word[1] in _PLY_TYPES:
            fields.append((word[2], _PLY_TYPES[word[1]]))
        else:
            raise ValueError(f"read_ply: {path}: cannot read '{line}'")
    dt = np.dtype(fields)
    if n is None or len(body) != n * dt.itemsize:
        raise ValueError(f"read_ply: {path}: {len(body)} bytes of data for {n} vertices of {dt.itemsize} bytes")
    rec = np.frombuffer(body, dt, n)
    take = lambda names, t: (np.stack([rec[k] for k in names], 1).astype(t, copy=False)  # noqa: E731
                             if all(k in rec.dtype.names for k in names) else None)
    xyz = take(("x", "y", "z"), np.float32)
    if xyz is None:
        raise ValueError(f"read_ply: {path} has no x, y, z")
    return xyz, take(("red", "green", "blue"), np.uint8), take(("nx", "ny", "nz"), np.float32)
