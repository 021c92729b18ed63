"""Whole-scene inference: a disparity map for an image pair larger than one forward.

The scene is cut into overlapping tiles on the device (``kernels.standardize_tiles_u8``: one
gather, every tile standardised with the whole scene's statistics, as the reference
standardises before it crops), the tiles go through the captured forward in batches, and each
output map is blended back on the device (``kernels.blend_tiles``).  Nothing is copied to the
host and nothing synchronises.

Stereo makes the overlap one-sided: a tile cut at column x0 > 0 sees no right-image pixel left
of x0, so its first ``maxdisp`` columns were matched against a truncated search range.  They
are a guard band of weight 0 (plus ``context`` columns on every cut side for the network's
receptive field), then the weight ramps up over ``ramp`` pixels.  A side that touches the
scene's border has neither guard nor ramp.  DESIGN.md §4, "Whole-scene inference", has the
rule and its reasons; ``plan_tiles`` and ``TilePlan.weights`` state it exactly.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

MAX_AXIS_TILES = 64  # lea_tile_blend_f32 stages the origins of one axis in LDS
MAX_RAMP = 256       # a weight product is then <= 65536: exact in float32

SceneResult = collections.namedtuple(
    "SceneResult", "disp entropy peak disp_local disp_right state disp_filled",
    defaults=(None,) * 6)


def _axis_origins(S: int, L: int, guards: int, ramp: int, name: str):
    """Origins of the tiles of length L along an axis of length S whose two guards sum to
    ``guards``: one tile at S - L (<= 0: the scene at the tile's far end, zeros before it, as
    the reference pads) when it fits, else evenly spread tiles no more than
    L - guards - ramp apart."""
    if S <= L:
        return [S - L]
    smax = L - guards - ramp
    if smax < 1:
        raise ValueError(f"plan_tiles: a tile of {L} along {name} is too short for guards of {guards} "
                         f"and a ramp of {ramp} (needs at least {guards + ramp + 1})")
    n = -(-(S - L) // smax) + 1
    if n > MAX_AXIS_TILES:
        raise ValueError(f"plan_tiles: {n} tiles along {name} (at most {MAX_AXIS_TILES}); use a larger tile")
    return [(k * (S - L)) // (n - 1) for k in range(n)]


def _axis_weights(o: int, L: int, S: int, g0: int, g1: int, ramp: int) -> np.ndarray:
    """The integer weights of tile coordinates 0 .. L-1 of a tile at origin o."""
    lo, hi = o > 0, o + L < S
    a, b = (g0 if lo else 0), (g1 if hi else 0)
    i = np.arange(L, dtype=np.int64)
    w = np.full(L, ramp, dtype=np.int64)
    if lo:
        w = np.minimum(w, i - a + 1)
    if hi:
        w = np.minimum(w, (L - b) - i)
    w[(i < a) | (i >= L - b)] = 0
    return w


class TilePlan:
    """A separable tile plan: tile k = ky * nx + kx has its origin at (ys[ky], xs[kx]).
    ``plan_tiles`` makes one; a plan may also be built from origins handed in directly
    (nothing then promises coverage: ``covers()`` tells)."""

    def __init__(self, height, width, tile_h, tile_w, maxdisp, context, ramp, ys, xs):
        if not 1 <= ramp <= MAX_RAMP:
            raise ValueError(f"ramp {ramp}: 1..{MAX_RAMP}")
        if context < 0 or maxdisp < 0:
            raise ValueError(f"context {context} and maxdisp {maxdisp} must not be negative")
        if min(height, width, tile_h, tile_w) < 1:
            raise ValueError(f"bad scene {height}x{width} or tile {tile_h}x{tile_w}")
        if not (1 <= len(ys) <= MAX_AXIS_TILES and 1 <= len(xs) <= MAX_AXIS_TILES):
            raise ValueError(f"{len(ys)} x {len(xs)} tiles: 1..{MAX_AXIS_TILES} per axis")
        self.height, self.width = int(height), int(width)
        self.tile_h, self.tile_w = int(tile_h), int(tile_w)
        self.maxdisp, self.context, self.ramp = int(maxdisp), int(context), int(ramp)
        self.ys, self.xs = [int(v) for v in ys], [int(v) for v in xs]
        self._device = {}

    ny = property(lambda self: len(self.ys))
    nx = property(lambda self: len(self.xs))

    def __len__(self):
        return self.ny * self.nx

    @property
    def origins(self) -> np.ndarray:
        """int32 [N, 2]: (y, x) of every tile, in tile order."""
        return np.array([(y, x) for y in self.ys for x in self.xs], dtype=np.int32).reshape(-1, 2)

    def guards(self, view: str = "left"):
        """((y low, y high), (x low, x high)) guard widths of a view's maps."""
        c, d = self.context, self.maxdisp
        if view == "left":
            return (c, c), (d + c, c)
        if view == "right":
            return (c, c), (c, d + c)
        raise ValueError(f"view {view!r}: 'left' or 'right'")

    def axis_weights(self, view: str = "left"):
        """(wy [ny, tile_h], wx [nx, tile_w]) int64: the per-axis weights of every tile row
        and column of the plan."""
        (gy0, gy1), (gx0, gx1) = self.guards(view)
        wy = np.stack([_axis_weights(o, self.tile_h, self.height, gy0, gy1, self.ramp) for o in self.ys])
        wx = np.stack([_axis_weights(o, self.tile_w, self.width, gx0, gx1, self.ramp) for o in self.xs])
        return wy, wx

    def weights(self, k: int, view: str = "left") -> np.ndarray:
        """int64 [tile_h, tile_w]: tile k's weights, the product of its two axes'."""
        wy, wx = self.axis_weights(view)
        return wy[k // self.nx][:, None] * wx[k % self.nx][None, :]

    def cover_count(self, view: str = "left") -> np.ndarray:
        """int64 [H, W]: how many tiles weigh on each scene pixel."""
        wy, wx = self.axis_weights(view)

        def axis(w, origins, L, S):
            n = np.zeros(S, dtype=np.int64)
            for row, o in zip(w, origins):
                lo, hi = max(o, 0), min(o + L, S)
                if lo < hi:
                    n[lo:hi] += row[lo - o:hi - o] > 0
            return n
        return axis(wy, self.ys, self.tile_h, self.height)[:, None] * \
            axis(wx, self.xs, self.tile_w, self.width)[None, :]

    def covers(self) -> bool:
        """Every scene pixel has a tile of positive weight, in both views."""
        return all(bool((self.cover_count(v) > 0).all()) for v in ("left", "right"))

    def device_axes(self, device):
        """(ys, xs) as int32 tensors on ``device`` (made once per device)."""
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.tensor(self.ys, dtype=torch.int32, device=device),
                                 torch.tensor(self.xs, dtype=torch.int32, device=device))
        return self._device[key]


def plan_tiles(height: int, width: int, tile_h: int, tile_w: int, maxdisp: int, context: int = 16,
               ramp: int = 32) -> TilePlan:
    """The tile plan of a ``height`` x ``width`` scene for ``tile_h`` x ``tile_w`` forwards.
    The x guards sum to maxdisp + 2 * context, the y guards to 2 * context."""
    if not 1 <= ramp <= MAX_RAMP:
        raise ValueError(f"ramp {ramp}: 1..{MAX_RAMP}")
    if context < 0:
        raise ValueError(f"context {context} must not be negative")
    ys = _axis_origins(height, tile_h, 2 * context, ramp, "y")
    xs = _axis_origins(width, tile_w, maxdisp + 2 * context, ramp, "x")
    return TilePlan(height, width, tile_h, tile_w, maxdisp, context, ramp, ys, xs)


# an origin no scene reaches: the gather writes such a tile as zeros
_PAD_ORIGIN = -(1 << 30)


class SceneRunner:
    """``runner(left_u8, right_u8) -> SceneResult`` for uint8 scenes [H, W, 3|4] of any size,
    on the host (numpy or tensor) or the device.  Keeps one captured forward per mode
    (``model.graphed(tile_batch, tile_h, tile_w, ...)``; ``graph=False`` calls the model
    directly) and one ``TilePlan`` per scene size.

    ``confidence=True`` also blends the entropy, peak mass and winner-window disparity;
    ``lr_threshold`` blends the tiles' right-view disparity with the right view's guards and
    runs ``kernels.lr_check`` once on the two scene maps (a per-tile state cannot be blended).
    Asking for both runs two forwards per batch (one capture holds one of them).
    Inference only, like ``forward_lr``."""

    def __init__(self, model, tile_h: int, tile_w: int, tile_batch: int = 1, context: int = 16, ramp: int = 32,
                 confidence: bool = False, radius: int = 4, lr_threshold=None, graph: bool = True):
        if tile_batch < 1:
            raise ValueError(f"tile_batch {tile_batch}: at least 1")
        if not 1 <= ramp <= MAX_RAMP:
            raise ValueError(f"ramp {ramp}: 1..{MAX_RAMP}")
        if lr_threshold is not None and not lr_threshold > 0:
            raise ValueError(f"lr_threshold {lr_threshold}: a threshold in pixels > 0, or None")
        model.check_shape(tile_h, tile_w)
        self.model = model
        self.tile_h, self.tile_w, self.tile_batch = int(tile_h), int(tile_w), int(tile_batch)
        self.context, self.ramp = int(context), int(ramp)
        self.confidence, self.radius, self.lr_threshold, self.graph = bool(confidence), radius, lr_threshold, graph
        self.captures = 0  # graphs captured so far
        self._graphs = {}
        self._plans = {}

    # ------------------------------------------------------------------ planning
    def plan(self, height: int, width: int) -> TilePlan:
        key = (int(height), int(width))
        if key not in self._plans:
            self._plans[key] = plan_tiles(key[0], key[1], self.tile_h, self.tile_w, self.model.maxdisp,
                                          self.context, self.ramp)
        return self._plans[key]

    def batches(self, plan: TilePlan):
        """The batches one call forwards: lists of ``tile_batch`` tile indices in tile order,
        -1 for the zero tiles that pad the last one (forwarded, never blended)."""
        n, b = len(plan), self.tile_batch
        idx = list(range(n)) + [-1] * (-n % b)
        return [idx[i:i + b] for i in range(0, len(idx), b)]

    def tiles(self, left_u8, right_u8, plan: TilePlan = None):
        """The network inputs of one call: (left, right) float32 [nb * tile_batch, 3, tile_h,
        tile_w], batch i being rows i * tile_batch .. (i + 1) * tile_batch - 1."""
        from . import kernels
        left, right = self._scenes(left_u8, right_u8)
        plan = plan or self.plan(left.shape[0], left.shape[1])
        return kernels.standardize_tiles_u8(left, right, self._origins(plan, left.device), self.tile_h,
                                            self.tile_w)

    def _origins(self, plan, device):
        key = "origins:" + str(device)
        if key not in plan._device:
            o = np.full((len(self.batches(plan)) * self.tile_batch, 2), _PAD_ORIGIN, dtype=np.int32)
            o[:len(plan)] = plan.origins
            plan._device[key] = torch.from_numpy(o).to(device)
        return plan._device[key]

    def _scenes(self, left, right):
        dev = next(self.model.parameters()).device
        out = []
        for t in (left, right):
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(np.ascontiguousarray(t))
            if t.requires_grad:
                raise RuntimeError("SceneRunner is inference only: pass inputs that do not require grad")
            if t.dtype != torch.uint8:
                raise ValueError(f"SceneRunner takes decoded uint8 scenes, got {t.dtype}")
            if t.dim() == 4 and t.shape[0] == 1:
                t = t[0]
            out.append(t.to(dev, non_blocking=True))
        if out[0].shape != out[1].shape or out[0].dim() != 3 or out[0].shape[-1] not in (3, 4):
            raise ValueError(f"left/right must both be [H, W, 3|4] uint8, got {tuple(out[0].shape)} and "
                             f"{tuple(out[1].shape)}")
        return out

    # ------------------------------------------------------------------ forwards
    def _modes(self):
        modes = (["confidence"] if self.confidence else []) + (["lr"] if self.lr_threshold is not None else [])
        return modes or ["plain"]

    def _forward(self, mode, x, y):
        """One batch through the model: a tuple of [tile_batch, tile_h, tile_w] maps (static
        buffers under ``graph``: overwritten by the next call)."""
        if self.graph:
            # a capture holds the packed weights of its day: drop it when they have changed
            version = (self.model.feature._weights_version(), self.model.matching._weights_version(),
                       self.model.precision)
            if version != getattr(self, "_version", None):
                self._graphs, self._version = {}, version
            if mode not in self._graphs:
                self._graphs[mode] = self.model.graphed(
                    self.tile_batch, self.tile_h, self.tile_w, confidence=mode == "confidence", radius=self.radius,
                    lr_threshold=self.lr_threshold if mode == "lr" else None)
                self.captures += 1
            out = self._graphs[mode](x, y)
        elif mode == "confidence":
            out = self.model.forward_with_confidence(x, y, self.radius)
        elif mode == "lr":
            out = self.model.forward_lr(x, y, self.lr_threshold)
        else:
            out = self.model(x, y)
        if mode == "confidence":
            return {"disp": out.disp, "entropy": out.entropy, "peak": out.peak, "disp_local": out.disp_local}
        if mode == "lr":
            return {"disp": out.disp, "disp_right": out.disp_right}
        return {"disp": out}

    @torch.no_grad()
    def __call__(self, left_u8, right_u8) -> SceneResult:
        from . import kernels
        if self.model.training:
            raise RuntimeError("SceneRunner is inference only (its outputs have no backward): "
                               "call model.eval() first")
        left, right = self._scenes(left_u8, right_u8)
        plan = self.plan(left.shape[0], left.shape[1])
        xl, xr = kernels.standardize_tiles_u8(left, right, self._origins(plan, left.device), self.tile_h,
                                              self.tile_w)
        n, b = len(plan), self.tile_batch
        maps = {}
        for i in range(len(self.batches(plan))):
            rows = slice(i * b, (i + 1) * b)
            for mode in self._modes():
                for name, t in self._forward(mode, xl[rows], xr[rows]).items():
                    if name == "disp" and mode == "lr" and self.confidence:
                        continue  # the confidence forward's disparity is the same, bit for bit
                    if name not in maps:
                        maps[name] = torch.empty((xl.shape[0], self.tile_h, self.tile_w), device=xl.device,
                                                 dtype=torch.float32)
                    maps[name][rows].copy_(t)
        out = {name: kernels.blend_tiles(t[:n], plan, "right" if name == "disp_right" else "left")
               for name, t in maps.items()}
        if self.lr_threshold is not None:
            lr = kernels.lr_check(out["disp"][None], out["disp_right"][None], self.lr_threshold)
            out["state"], out["disp_filled"] = lr.state[0], lr.disp_filled[0]
        return SceneResult(**out)


@torch.no_grad()
def refine_scene(result: SceneResult, left_u8, lam: float = None, sigma: float = None, iterations: int = None,
                 return_support: bool = False, speckle: dict = None):
    """``kernels.fgs_refine`` of a ``SceneResult``, once, at scene size, after the blend (never
    per tile: a tile's solve stops at its cut).  The guide is the uint8 scene ``left_u8``
    [H, W, 3|4] standardised with the whole scene's statistics (what the tiles were cut from),
    ``conf`` is ``result.peak`` if the runner blended it, ``exclude`` is ``result.state`` if it
    ran the left-right check.  Returns the refined disparity [H, W], with ``return_support``
    (refined, support).  ``None`` for a parameter takes the default of ``kernels.fgs_refine``.
    ``speckle=dict(max_size=..., max_diff=...)`` (an empty dict for the defaults) runs
    ``speckle_scene`` first, and the refinement excludes what it removed; ``None``: no such
    call."""
    from . import kernels
    if speckle is not None:
        if not isinstance(speckle, dict) or set(speckle) - {"max_size", "max_diff"}:
            raise ValueError(f"refine_scene: speckle must be None or a dict of max_size / max_diff, got {speckle!r}")
        result = result._replace(state=speckle_scene(result, **speckle).state)
    disp = result.disp
    left = left_u8
    if isinstance(left, np.ndarray):
        left = torch.from_numpy(np.ascontiguousarray(left))
    if left.dtype != torch.uint8:
        raise ValueError(f"refine_scene takes the decoded uint8 scene, got {left.dtype}")
    if left.dim() == 4 and left.shape[0] == 1:
        left = left[0]
    if left.dim() != 3 or tuple(left.shape[:2]) != tuple(disp.shape):
        raise ValueError(f"left_u8 must be [H, W, 3|4] of the result's size {tuple(disp.shape)}, got "
                         f"{tuple(left.shape)}")
    left = left.to(disp.device, non_blocking=True)
    h, w = disp.shape
    origin = torch.zeros((1, 2), dtype=torch.int32, device=disp.device)
    guide = kernels.standardize_tiles_u8(left, left, origin, h, w)[0]  # one tile: the whole scene
    out = kernels.fgs_refine(guide, disp[None], None if result.peak is None else result.peak[None],
                             None if result.state is None else result.state[None],
                             kernels.REFINE_LAMBDA if lam is None else lam,
                             kernels.REFINE_SIGMA if sigma is None else sigma,
                             kernels.REFINE_ITERATIONS if iterations is None else iterations, return_support=True)
    return (out[0][0], out[1][0]) if return_support else out[0][0]


@torch.no_grad()
def speckle_scene(result: SceneResult, max_size: int = None, max_diff: float = None, fill: float = 0.0):
    """``kernels.speckle_filter`` of a ``SceneResult``, once, at scene size, after the blend:
    the blended disparity, with ``result.state`` as walls if the runner ran the left-right
    check.  Never run the filter per tile: a component cut by a tile's edge looks small there
    and would be removed, while at scene size it is judged at its whole size.  Returns
    ``kernels.DisparitySpeckle`` with [H, W] maps (state, size, filtered).  ``None`` for a
    parameter takes the (untuned) default of ``kernels.speckle_filter``."""
    from . import kernels
    return kernels.speckle_filter(result.disp, result.state,
                                  kernels.SPECKLE_MAX_SIZE if max_size is None else max_size,
                                  kernels.SPECKLE_MAX_DIFF if max_diff is None else max_diff, fill)


@torch.no_grad()
def points_scene(result: SceneResult, Q, left_u8=None, use: str = "refined", refined: torch.Tensor = None,
                 refine: dict = None, **kw):
    """``kernels.reproject`` of a ``SceneResult``, once, at scene size, after the blend (never
    per tile: the overlaps would give their points twice, and a tile's normals stop at its
    cut), with ``exclude`` = ``result.state`` when the runner ran the left-right check (or
    ``speckle_scene`` put its state there).  ``use`` names the map: "disp" (the blended
    disparity), "filled" (``result.disp_filled``) or "refined" (``refined``, what
    ``refine_scene`` returned for this result; None: it is called here, with the keywords in
    ``refine``).  ``Q`` is the scene's matrix (``pointcloud.q_matrix``, origin (0, 0));
    ``left_u8`` the uint8 scene [H, W, 3|4] for the colours, or None.  ``kw``: the other
    keywords of ``reproject``.  Returns ``kernels.PointCloud`` without a batch axis."""
    from . import kernels
    if use not in ("refined", "filled", "disp"):
        raise ValueError(f"points_scene: use {use!r}: one of refined, filled, disp")
    if use == "refined" and refined is None:
        if left_u8 is None:
            raise ValueError("points_scene: use='refined' needs the scene left_u8 as the guide, or refined=")
        refined = refine_scene(result, left_u8, **({} if refine is None else refine))
    disp = {"refined": refined, "filled": result.disp_filled, "disp": result.disp}[use]
    if disp is None:
        raise ValueError("points_scene: use='filled', but the result holds no filled disparity (the runner ran no "
                         "left-right check)")
    if tuple(disp.shape) != tuple(result.disp.shape):
        raise ValueError(f"points_scene: the map is {tuple(disp.shape)}, the scene {tuple(result.disp.shape)}")
    image = left_u8
    if image is not None:
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        image = image.to(disp.device, non_blocking=True)
    return kernels.reproject(disp, Q, image, result.state, **kw)


@torch.no_grad()
def dsm_scene(result: SceneResult, Q, left_u8=None, grid=None, cell: float = None, radius: float = 0.5,
              use: str = "refined", fill_iterations: int = 0, min_neighbours: int = 3, disp_range=None,
              pose=None, surface=None, **kw):
    """The surface model of a ``SceneResult`` (``dsm.Surface``), once, at scene size, after the
    blend, through ``points_scene`` (never per tile, for the reason given there: the overlaps
    would give their points twice).  ``grid`` is (G, GH, GW); None: ``dsm.grid_from_view`` of the
    scene between the disparities ``disp_range`` = (far, near), with ``cell`` and ``pose``.
    ``radius``: the footprint of a point in cells.  ``surface``: a ``dsm.Surface`` of the grid's
    size to add the scene to (a mosaic of several scenes; it is not cleared), None: a new one.
    ``kw``: the other keywords of ``points_scene``.  Returns ``dsm.SurfaceMaps`` (``rgb`` with
    ``left_u8``, else ``source``: rows of the scene's compact cloud)."""
    from . import dsm
    if grid is None:
        if disp_range is None:
            raise ValueError("dsm_scene: without a grid the two disparities disp_range = (far, near) that bound it "
                             "are needed")
        h, w = result.disp.shape
        grid = dsm.grid_from_view(Q.cpu().numpy() if isinstance(Q, torch.Tensor) else Q, h, w, disp_range, cell, pose)
    G, gh, gw = grid
    cloud = points_scene(result, Q, left_u8, use=use, **kw)
    if surface is None:
        surface = dsm.Surface(gh, gw, result.disp.device)
    elif (surface.gh, surface.gw, surface.batch) != (gh, gw, None):
        raise ValueError(f"dsm_scene: the surface is {surface.gh} x {surface.gw} (batch {surface.batch}), the grid "
                         f"{gh} x {gw} without a batch")
    return surface.add_cloud(cloud, G, radius=radius).resolve(fill_iterations, min_neighbours)


@torch.no_grad()
def view_scene(result: SceneResult, left_u8, s: float = 1.0, use: str = "refined", refined: torch.Tensor = None,
               refine: dict = None, **kw):
    """``kernels.forward_warp`` of a ``SceneResult``, once, at scene size, after the blend: the
    uint8 scene ``left_u8`` [H, W, 3|4] as seen from baseline fraction ``s`` (0 = the left camera,
    1 = the right one) through the map ``use`` names, chosen as ``points_scene`` chooses it, with
    ``exclude`` = ``result.state`` when the runner ran the left-right check (or ``speckle_scene``
    put its state there) and the map is not the refined one, which has no flagged pixels left.
    The image is converted to float32 with torch ops (the kernel takes no uint8), so the view's
    colours are on the 0 .. 255 scale.  ``kw``: the other keywords of ``forward_warp``.  Returns
    ``kernels.WarpedView`` without a batch axis (image [3, H, W]).  Refuses a scene wider than
    ``kernels.FORWARD_WARP_MAX_W``."""
    from . import kernels
    if use not in ("refined", "filled", "disp"):
        raise ValueError(f"view_scene: use {use!r}: one of refined, filled, disp")
    if result.disp.shape[-1] > kernels.FORWARD_WARP_MAX_W:
        raise ValueError(f"view_scene: the scene is {result.disp.shape[-1]} wide, the warp's limit is "
                         f"{kernels.FORWARD_WARP_MAX_W}")
    if use == "refined" and refined is None:
        refined = refine_scene(result, left_u8, **({} if refine is None else refine))
    disp = {"refined": refined, "filled": result.disp_filled, "disp": result.disp}[use]
    if disp is None:
        raise ValueError("view_scene: use='filled', but the result holds no filled disparity (the runner ran no "
                         "left-right check)")
    if tuple(disp.shape) != tuple(result.disp.shape):
        raise ValueError(f"view_scene: the map is {tuple(disp.shape)}, the scene {tuple(result.disp.shape)}")
    image = left_u8
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dim() == 4 and image.shape[0] == 1:
        image = image[0]
    if image.dtype != torch.uint8 or image.dim() != 3 or tuple(image.shape[:2]) != tuple(disp.shape):
        raise ValueError(f"view_scene: left_u8 must be uint8 [H, W, 3|4] of the result's size {tuple(disp.shape)}, got "
                         f"{image.dtype} {tuple(image.shape)}")
    image = image.to(disp.device, non_blocking=True)[..., :3].permute(2, 0, 1).to(torch.float32).contiguous()
    exclude = None if use != "disp" else result.state
    out = kernels.forward_warp(image[None], disp[None].contiguous(), float(s),
                               None if exclude is None else exclude[None], **kw)
    return kernels.WarpedView(*(None if t is None else t[0] for t in out))
