"""Surface models on the device: point clouds rasterised into a z-buffered ground grid (a
digital surface model) with the colour or the row of the surface seen in each cell (an
orthophoto), mosaicked over any number of clouds.  The kernels are csrc/dsm.hip, the
definition is at lea_dsm_splat_f32 in include/leastereo_hip.h.

The host side here: the 3 x 4 grid matrix of a ground grid (``grid_matrix``), the bounding grid of
a view (``grid_from_view``), and ``Surface``, which owns the persistent keys and launches on the
current stream through ``kernels._launch``: nothing is copied to the host, nothing synchronises,
``add`` and ``resolve`` are capturable.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from . import _lib, kernels
from .kernels import _as_f32, _launch, _number, _ptr

MAX_RADIUS = 2  # LEA_DSM_MAX_RADIUS
STAGING = {"auto": 0, "global": 1, "lds": 2}  # LEA_DSM_STAGING_*
MAX_FILL = 1024

SurfaceMaps = collections.namedtuple("SurfaceMaps", "height rgb source state hits")
SurfaceMaps.__doc__ = """What ``Surface.resolve`` returns, on the device, each [B, GH, GW] ([GH, GW] for a surface
without a batch): ``height`` float32 (``nodata`` in an empty cell), ``rgb`` uint8 [..., 3] of a surface that took
colours or ``source`` int32 (the row of the winning point, -1 in an empty cell) of one that did not (``None`` for the
other), ``state`` uint8 (0 measured, 1 filled, 2 empty) and ``hits`` (the surface's int32 counts, not a copy; ``None``
for a surface without them)."""


def _vec3(who, name, v):
    a = np.asarray(v, dtype=np.float64)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: {name} must be three finite numbers, got {v!r}")
    return a


def _pose(who, pose):
    if pose is None:
        return np.eye(4)
    p = np.asarray(pose, dtype=np.float64)
    if p.shape != (4, 4) or not np.all(np.isfinite(p)):
        raise ValueError(f"{who}: pose must be a finite 4 x 4 camera-to-world matrix, got shape {p.shape}")
    return p


def grid_matrix64(origin, cell, u_axis=(1, 0, 0), v_axis=(0, 1, 0), z_axis=(0, 0, -1), z0=0.0, pose=None) -> np.ndarray:
    """``grid_matrix`` before its one rounding: float64 [3, 4]."""
    who = "grid_matrix"
    o, ua, va, za = (_vec3(who, n, v) for n, v in (("origin", origin), ("u_axis", u_axis), ("v_axis", v_axis),
                                                   ("z_axis", z_axis)))
    cell, z0 = float(cell), float(z0)
    if not (math.isfinite(cell) and cell > 0 and math.isfinite(z0)):
        raise ValueError(f"grid_matrix: cell {cell} must be a finite number > 0 and z0 {z0} finite")
    p = _pose(who, pose)
    R, t = p[:3, :3], p[:3, 3]
    G = np.empty((3, 4), np.float64)
    for r, (axis, scale, add) in enumerate(((ua, 1.0 / cell, 0.0), (va, 1.0 / cell, 0.0), (za, 1.0, z0))):
        G[r, :3] = (axis @ R) * scale
        G[r, 3] = float(axis @ (t - o)) * scale + add
    return G


def grid_matrix(origin, cell, u_axis=(1, 0, 0), v_axis=(0, 1, 0), z_axis=(0, 0, -1), z0=0.0, pose=None) -> np.ndarray:
    """The float32 [3, 4] matrix G that takes a camera-frame point P to grid coordinates: with
    P_w = pose P (``pose`` a 4 x 4 camera-to-world matrix, the identity by default),

        u = u_axis . (P_w - origin) / cell,  v = v_axis . (P_w - origin) / cell,
        z = z_axis . (P_w - origin) + z0

    u is the column and v the row of the cell (cell i has its centre at the integer i), z the
    height that is kept.  Composed in float64 and rounded once.  The defaults suit a nadir
    camera, x right, y down, looking along +z: the height is z0 - Z."""
    return grid_matrix64(origin, cell, u_axis, v_axis, z_axis, z0, pose).astype(np.float32)


def grid_from_view(Q, h: int, w: int, disp_range, cell: float = None, pose=None):
    """(G, GH, GW): the bounding grid of the frustum of an h x w view with reprojection matrix
    ``Q`` (``pointcloud.q_matrix``) between the two disparities ``disp_range`` = (far, near), with
    the default axes of ``grid_matrix`` and the origin at the frustum's smallest world x and y
    (and z = 0).  ``cell`` None is the ground sample distance at the far disparity: the distance
    between the points of two neighbouring pixels there.  Float64 on the host; G is float32."""
    who = "grid_from_view"
    Q = np.asarray(Q, dtype=np.float64)
    if Q.shape != (4, 4) or not np.all(np.isfinite(Q)):
        raise ValueError(f"{who}: Q must be a finite 4 x 4 matrix, got shape {Q.shape}")
    _number(who, "h", h, "an integer >= 1", lo=1, integer=True)
    _number(who, "w", w, "an integer >= 1", lo=1, integer=True)
    d = np.asarray(disp_range, dtype=np.float64)
    if d.shape != (2,) or not np.all(np.isfinite(d)) or d[0] == d[1]:
        raise ValueError(f"{who}: disp_range must be two different finite disparities, got {disp_range!r}")
    p = _pose(who, pose)

    def point(x, y, dd):
        hh = Q @ np.array([x, y, dd, 1.0])
        if hh[3] == 0:
            raise ValueError(f"{who}: disparity {dd} is at infinity under this Q")
        return hh[:3] / hh[3]

    far = d[0] if abs(point(0, 0, d[0])[2]) >= abs(point(0, 0, d[1])[2]) else d[1]
    if cell is None:
        cell = float(np.linalg.norm(point(1, 0, far) - point(0, 0, far)))
    cell = float(cell)
    if not (math.isfinite(cell) and cell > 0):
        raise ValueError(f"{who}: cell {cell} must be a finite number > 0")
    corners = np.array([point(x, y, dd) for dd in d for y in (0, h - 1) for x in (0, w - 1)])
    world = corners @ p[:3, :3].T + p[:3, 3]
    lo, hi = world.min(0), world.max(0)
    gw = int(math.floor((hi[0] - lo[0]) / cell + 0.5)) + 1
    gh = int(math.floor((hi[1] - lo[1]) / cell + 0.5)) + 1
    if gh * gw > 2 ** 31 - 1:
        raise ValueError(f"{who}: a grid of {gh} x {gw} cells is above 2^31 - 1; choose a larger cell")
    return grid_matrix((lo[0], lo[1], 0.0), cell, pose=p), gh, gw


class Surface:
    """A ground grid of ``gh`` x ``gw`` cells on ``device`` (``batch`` of them, or one without a
    batch axis): ``keys`` int64 [B, GH, GW] holding the uint64 keys of lea_dsm_splat_f32 bit for
    bit (0 = empty), and with ``hits=True`` the int32 counts ``hits``.  The grid persists between
    calls: ``add`` any number of clouds in any order (the result is the same bits), ``resolve``
    to read it out, ``clear`` to start again."""

    def __init__(self, gh: int, gw: int, device, batch: int = None, hits: bool = False):
        who = "Surface"
        _number(who, "gh", gh, "an integer >= 1", lo=1, integer=True)
        _number(who, "gw", gw, "an integer >= 1", lo=1, integer=True)
        if batch is not None:
            _number(who, "batch", batch, "an integer in 1 .. 65535, or None", lo=1, hi=65535, integer=True)
        self.batch = batch
        self.b = 1 if batch is None else batch
        if self.b * gh * gw > 2 ** 31 - 1:
            raise ValueError(f"Surface: B * GH * GW = {self.b * gh * gw} is above 2^31 - 1")
        self.gh, self.gw = gh, gw
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipKernelError(f"Surface: the grid lives on a ROCm device, got {self.device}")
        lead = () if batch is None else (batch,)
        self.keys = torch.empty(lead + (gh, gw), device=self.device, dtype=torch.int64)
        self.hits = torch.empty(lead + (gh, gw), device=self.device, dtype=torch.int32) if hits else None
        self.kind = None  # the payload of the hits since the last clear: None, "rgb" or "source"
        self.clear()

    def clear(self) -> "Surface":
        """``lea_dsm_clear``: every cell empty, every count 0.  One launch."""
        _launch("lea_dsm_clear", self.keys.data_ptr(), _ptr(self.hits), self.b, self.gh, self.gw)
        self.kind = None
        return self

    def _g(self, G) -> torch.Tensor:
        shape = tuple(G.shape) if isinstance(G, torch.Tensor) else np.shape(G)
        if shape not in ((3, 4), (self.b, 3, 4)):
            raise ValueError(f"Surface.add: G must be [3, 4] or [{self.b}, 3, 4], got {shape}")
        return _as_f32(G, self.device, "Surface.add: G must be a floating-point matrix")

    def add(self, points: torch.Tensor, G, count: torch.Tensor = None, colours: torch.Tensor = None,
            radius: float = 0.0, staging: str = "auto", row_width: int = 0) -> "Surface":
        """``lea_dsm_splat_f32``: the rows of ``points`` (float32 on the device, [B, rows, 3] or an
        organised [B, H, W, 3]; without the B for a surface without a batch) through ``G``
        ([3, 4] or [B, 3, 4], ``grid_matrix``; a float32 device tensor is read in place at every
        launch and replay) into the grid, each covering the cells within ``radius`` cells
        (0 .. 2) of where it lands; the highest wins a cell.  ``count`` int32 [B] on the device:
        the rows of each item that are read (``PointCloud.count``).  ``colours`` uint8 like
        ``points``: the surface then carries colours, else rows; one surface cannot mix the two
        between clears.  ``staging`` "auto", "global" or "lds" and ``row_width`` (the width of the
        image the rows are the pixels of, or 0) choose how the scatter runs, never what it
        gives.  One launch."""
        who = "Surface.add"
        if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32:
            raise ValueError(f"{who}: points must be a float32 tensor on the device")
        lead = 0 if self.batch is None else 1
        if points.dim() not in (lead + 2, lead + 3) or points.shape[-1] != 3 or 0 in points.shape or (
                lead and points.shape[0] != self.b):
            raise ValueError(f"{who}: points must be {'[B, ' if lead else '['}rows, 3] or "
                             f"{'[B, ' if lead else '['}H, W, 3]{f' with B = {self.b}' if lead else ''}, got "
                             f"{tuple(points.shape)}")
        rows = math.prod(points.shape[lead:-1])
        if self.b * rows > 2 ** 31 - 1:
            raise ValueError(f"{who}: B * rows = {self.b * rows} is above 2^31 - 1")
        if colours is not None:
            if (not isinstance(colours, torch.Tensor) or not colours.is_cuda or colours.dtype != torch.uint8
                    or colours.shape != points.shape):
                raise ValueError(f"{who}: colours must be a uint8 {tuple(points.shape)} tensor on the device")
        if count is not None:
            if (not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int32
                    or count.numel() != self.b or count.dim() != lead):
                raise ValueError(f"{who}: count must be an int32 {'[B]' if lead else 'scalar'} tensor on the device")
        _number(who, "radius", radius, f"in 0 .. {MAX_RADIUS}", lo=0, hi=MAX_RADIUS)
        if staging not in STAGING:
            raise ValueError(f"{who}: staging {staging!r}: one of {', '.join(STAGING)}")
        _number(who, "row_width", row_width, "an integer in 0 .. rows", lo=0, hi=rows, integer=True)
        kind = "source" if colours is None else "rgb"
        if self.kind not in (None, kind):
            raise ValueError(f"{who}: this surface holds {self.kind} payloads since its last clear; one with "
                             f"{'colours' if kind == 'rgb' else 'no colours'} cannot be mixed in")
        g = self._g(G)
        p = points.contiguous()
        c = None if colours is None else colours.contiguous()
        n = None if count is None else count.contiguous()
        _launch("lea_dsm_splat_f32", p.data_ptr(), _ptr(n), _ptr(c), g.data_ptr(), 12 if g.dim() == 3 else 0, self.b,
                rows, int(row_width), float(radius), STAGING[staging], self.gh, self.gw, self.keys.data_ptr(),
                _ptr(self.hits))
        self.kind = kind
        return self

    def add_cloud(self, pc, G, radius: float = 0.0, staging: str = "auto", row_width: int = None) -> "Surface":
        """``add`` of a ``kernels.PointCloud``: its compact ``xyz`` with ``count`` and ``rgb``
        where it has them, else its organised ``points`` (NaN where not valid: those rows are
        skipped), whose width is then the ``row_width`` unless one is given."""
        if not isinstance(pc, kernels.PointCloud):
            raise ValueError(f"Surface.add_cloud: a kernels.PointCloud, got {type(pc).__name__}")
        if pc.xyz is not None:
            return self.add(pc.xyz, G, pc.count, pc.rgb, radius, staging, 0 if row_width is None else row_width)
        if pc.points is None:
            raise ValueError("Surface.add_cloud: the cloud has neither xyz nor points")
        return self.add(pc.points, G, None, None, radius, staging,
                        pc.points.shape[-2] if row_width is None else row_width)

    def resolve(self, fill_iterations: int = 0, min_neighbours: int = 3, nodata: float = float("nan")) -> SurfaceMaps:
        """``lea_dsm_resolve_f32``: the grid read out as ``SurfaceMaps``, after ``fill_iterations``
        passes in which an empty cell with at least ``min_neighbours`` (1 .. 8) non-empty
        8-neighbours takes the lowest of them (the background).  The keys themselves are not
        changed: more clouds can be added afterwards.  ``fill_iterations`` + 1 launches."""
        who = "Surface.resolve"
        _number(who, "fill_iterations", fill_iterations, f"an integer in 0 .. {MAX_FILL}", lo=0, hi=MAX_FILL,
                integer=True)
        _number(who, "min_neighbours", min_neighbours, "an integer in 1 .. 8", lo=1, hi=8, integer=True)
        _number(who, "nodata", nodata, "a number", bools=False)
        shape, dev = tuple(self.keys.shape), self.device
        ws = None
        if fill_iterations:
            ws = torch.empty(_lib.load().lea_dsm_resolve_workspace_bytes(self.b, self.gh, self.gw) // 8, device=dev,
                             dtype=torch.int64)
        height = torch.empty(shape, device=dev, dtype=torch.float32)
        state = torch.empty(shape, device=dev, dtype=torch.uint8)
        rgb = torch.empty(shape + (3,), device=dev, dtype=torch.uint8) if self.kind == "rgb" else None
        source = torch.empty(shape, device=dev, dtype=torch.int32) if self.kind != "rgb" else None
        _launch("lea_dsm_resolve_f32", self.keys.data_ptr(), _ptr(self.hits), self.b, self.gh, self.gw,
                int(fill_iterations), int(min_neighbours), float(nodata), _ptr(ws), height.data_ptr(), _ptr(rgb),
                _ptr(source), state.data_ptr())
        return SurfaceMaps(height, rgb, source, state, self.hits)
