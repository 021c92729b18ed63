"""Cell-graph executors: run the searched networks on the HIP kernels.

``MatchingExecutor`` runs newMatching.forward (retrain/skip_model_3d.py:140-174),
``FeatureExecutor`` runs newFeature.forward (retrain/new_model_2d.py:140-165).
Both are prepared once per weight load (``NewMatching.executor()`` /
``NewFeature.executor()``): every ConvBR's weight is re-laid out for its kernel
and its BN folded into fp32 scale/shift.  ``run`` then issues only C-ABI launches
on the current stream (no host syncs), so a whole forward can be captured in a
HIP graph.

An executor is put together in three steps ("How an executor is put together"):

* plan: ``_plan`` makes one ``ConvParams`` entry per ConvBR, then one planning method per route
  (``_plan_s1_group``, ``_plan_s0_pair``, ``_plan_pair_steps``, ``_plan_share``, ``_plan_fanout``,
  each behind its class switch) adds the stacked entries.  An entry records the ConvBRs whose
  weights it stacks and along which axis (``_plan_entry``), so nothing later reads that out of its
  name;
* pack once: ``_pack`` gives every planned entry the weight of the format that runs, from
  ``_source_weights`` of its record -- f32 executors ``packed`` (+ ``wino``), bf16 executors their
  bf16 fragments only;
* run with the carry: ``cell`` allocates the cell output ``cat([s1, s2, s3, s4])`` once and every
  producer writes its channel slice directly (preprocess -> s1 slot, first DAG op -> s_k slot, the
  second accumulates through the conv epilogue, a skip_connect term enters as the epilogue's
  residual: neither the ``cat`` nor the ``sum`` moves data).  What the next cell needs beyond the
  two states -- a level-down copy of the output, its own s0 already computed -- is returned in
  ``CellOut`` and handed to the next ``cell`` call; nothing of a forward stays on the executor.

A new route adds: a planning method and its call in ``_plan``, its launch in the part of ``cell``
it replaces (``_preprocess_s0``, ``_preprocess_s1``, ``_paired_steps``, ``_steps``), and, where it
hands something to the next cell, a field of ``CellOut``.  The packers need no edit.

Feature-net activations are [B, C, 1, H, W] views: a 2D map is the one-plane case of the 3D
kernels (1x1 convs, bilinear = trilinear on one plane), and the 3x3 convs run on the 2D entry of
the same MFMA engine.
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import kernels
from .arch import scale_dimension


def _stacked(fl: torch.Tensor, fr: torch.Tensor) -> torch.Tensor:
    """[fl; fr] along the batch: a view when fr directly follows fl in one buffer (the
    forward's stacked feature batch, LEAStereo.forward), else a copy (torch.cat) -- the
    r05 C4 forward's two copyBuffer launches were this cat of adjacent views.  One buffer
    means one storage: two separate tensors that the caching allocator happened to place
    back to back have adjacent addresses too, and a view of the first cannot span both."""
    if (fl.is_contiguous() and fr.is_contiguous() and fl.shape == fr.shape and fl.dtype == fr.dtype
            and fl.device == fr.device
            and fl.untyped_storage().data_ptr() == fr.untyped_storage().data_ptr()
            and fr.data_ptr() == fl.data_ptr() + fl.numel() * fl.element_size()):
        return fl.as_strided((2 * fl.shape[0],) + tuple(fl.shape[1:]), fl.stride())
    return torch.cat((fl, fr), 0)


@dataclass
class ConvParams:
    packed: torch.Tensor | None  # packed weights ("s3": the raw [cout, cin, 3, 3] weight); None until _pack
    scale: torch.Tensor | None
    shift: torch.Tensor | None
    cin: int
    cout: int
    k: int
    relu: bool
    kind: str = "3d"          # "3d" (k 1/3), "2d" (3x3 s1), "s3" (3x3 stride 3); bf16 packs: "bf16", "bf16_2d"
    wino: torch.Tensor | None = None  # Winograd-packed weight (f32 3D k=3 layers)
    # the record of what the entry holds: the ConvBR modules whose weights it stacks, in order, along
    # ``axis`` (0: cout -- sibling groups, share, fanout, s0_pair; 1: cin -- the pair steps); ``taps``:
    # the one source's 27 taps as the output channels of a 1x1 (last_3.taps)
    sources: tuple = ()
    axis: int = 0
    taps: bool = False


class CellOut(NamedTuple):
    """What cell() returns and the next cell() takes."""
    s0: torch.Tensor                  # the next cell's s0 (this cell's s1 input)
    out: torch.Tensor                 # this cell's output
    down: torch.Tensor | None = None  # the output one level down too, where its producers wrote it
    memo: tuple | None = None         # the next cell's s0 already computed: (source tensor, size, value)


# f32 3x3x3 layers run on the Winograd F(2,3)-along-W engine (2/3 of the direct
# engine's MFMA work); LEASTEREO_WINOGRAD=0 keeps them on the direct engine.
WINOGRAD = os.environ.get("LEASTEREO_WINOGRAD", "1") != "0"
# stem0 over the cost volume through 2D maps (csrc/cv_stem.hip); LEASTEREO_CV_STEM=0
# runs the 3D conv on the in-place cost volume instead.
CV_STEM = os.environ.get("LEASTEREO_CV_STEM", "1") != "0"


def _cat(ts, axis=0):
    return ts[0] if len(ts) == 1 else torch.cat(ts, axis)


def _plan_entry(convs, sources, axis=0, bn=True):
    """The (not yet packed) ConvParams of the ConvBR ``sources[0]``, or of several stacked along
    ``axis`` with their folded BN concatenated in the same order; ReLU and kind are the first's.
    ``bn=False``: the bare conv (no BN, no ReLU).  ``convs``: the net's ConvBR modules by name."""
    mods = [convs[s] for s in sources]
    mod, ws = mods[0], [m.conv.weight for m in mods]
    cout, cin, k = ws[0].shape[0], ws[0].shape[1], ws[0].shape[-1]
    if axis == 0:
        cout = sum(w.shape[0] for w in ws)
    else:
        cin = sum(w.shape[1] for w in ws)
    folded = [m.folded_bn() if bn else (None, None) for m in mods]
    scale, shift = folded[0] if len(mods) == 1 or not bn else (
        torch.cat([f[j] for f in folded]).contiguous() for j in (0, 1))
    if ws[0].dim() == 5 or k == 1:  # (1x1 Conv2d = 1x1x1 Conv3d on one plane)
        kind = "3d"
    elif mod.stride == 3:
        kind = "s3"
    elif mod.stride != 1 or mod.padding != 1:
        raise ValueError(f"unsupported Conv2d stride={mod.stride} padding={mod.padding}")
    else:
        kind = "2d"
    return ConvParams(None, scale, shift, cin, cout, k, bn and mod.relu, kind, sources=tuple(sources), axis=axis)


def _source_weights(convs, p):
    """The f32 weights that entry ``p`` stacks, in its record's order: what every packer reads.  A 2D
    1x1 comes in its one-plane 3D form.  ``taps``: the 3x3x3 weight's taps as rows co * 27 + tap of a
    1x1 weight, with zero rows up to the entry's cout (c8: channels in blocks of 8)."""
    ws = [convs[s].conv.weight for s in p.sources]
    if p.taps:
        taps = ws[0].permute(0, 2, 3, 4, 1).reshape(-1, ws[0].shape[1], 1, 1, 1)
        pad = p.cout - taps.shape[0]
        return [torch.cat([taps, taps.new_zeros((pad,) + tuple(taps.shape[1:]))], 0) if pad else taps]
    return [w.reshape(*w.shape[:2], 1, 1, 1) if w.dim() == 4 and w.shape[-1] == 1 else w for w in ws]


class CellGraphExecutor:
    """Shared machinery: parameter packing, ConvBR dispatch, the searched cell."""

    # stage capture for the per-stage parity checks (tests): tap(name, f32 NCDHW copy) at
    # the stages oracle/torch_ref.matching_forward names; None (the default) costs nothing
    tap = None

    def _emit(self, name, t):
        if self.tap is not None:
            self.tap(name, self._as_f32(t))

    @staticmethod
    def _as_f32(t):
        return t.detach().clone()

    # fp32: a down-sampled s1 that the next cell reads again as its s0 (same tensor, same
    # size) feeds one stacked 1x1 conv for both cells (the bf16 executors memoise every
    # resample instead); LEASTEREO_SHARE_DOWNSAMPLE=0 keeps two passes
    SHARE_DOWNSAMPLE = os.environ.get("LEASTEREO_SHARE_DOWNSAMPLE", "1") != "0"
    # where no cell resamples down: cell i's preprocess and cell i + 1's pre_preprocess, two 1x1
    # convs at the level of the tensor both read, as one two-head launch (lea_conv1x1_heads);
    # the f32 matching executor only
    FANOUT_1X1 = False
    # a three-op sibling group of 16-channel 3D ops (the L1 cells: 16 -> 48) as a 32-cout
    # launch on the pipelined W x D kernel plus a 16-cout one (r03: 66 + 43 us vs 124 us on
    # the 1-D 48-row engine); the f32 Winograd matching executor only.  Split as step 0's op
    # (head, 16 couts) + steps 1, 2 (the 32-cout group).  (r04: running op0 (s0 -> step 0)
    # on a side stream beside s1's preprocess and this group, the head accumulating after
    # the join, measured 140.6 -> 138.1 pairs/s at C2 in graph replay: not kept)
    SPLIT_S1_GROUP48 = False
    # the feature net's 2D cells: their two conv ops on s0 (op0 -> step 0 with the skip term as
    # its residual, op4 -> step 2 before op5 accumulates) as one launch writing two slots
    # (lea_conv2d_bnrelu_pair; r04).  The f32 feature executor only; LEASTEREO_PAIR_S0=0: two launches
    PAIR_S0 = False
    # a 3D cell whose every step sums two conv ops (the shipped matching genotype): each step
    # as ONE LEA_PAIR_SUM launch, y = relu(BN_a(conv_a(s_ja))) + relu(BN_b(conv_b(s_jb))),
    # reading the two states and writing the step's slot once (r05) -- instead of the s1
    # sibling group plus an accumulating launch per remaining op (a read-modify-write of the
    # slot each).  Executors whose engine takes LEA_PAIR_SUM set it
    PAIR_STEPS = False
    # the cells' channel counts that take the pair launches (A/B: LEASTEREO_PAIR_C=16,32 ...)
    PAIR_C = tuple(int(c) for c in os.environ.get("LEASTEREO_PAIR_C", "8,16,32").split(",") if c)

    # activations in the c8 layout ([B, C/8, D, H, W, 8] bfloat16; _C8Layout sets it): the f32-only
    # routes and operands stay out
    C8 = False

    def __init__(self, net):
        self.m = net
        with torch.no_grad():
            self._plan()
            for name, p in self.p.items():
                self._pack(name, p)

    def _plan(self):
        """``p``: one entry per ConvBR, then each route's stacked entries (and ``s1_group``,
        ``s1_split``, ``s0_pair``, ``pair_steps``: what cell() runs from)."""
        from .model import ConvBR
        self._convs = {name: mod for name, mod in self.m.named_modules() if isinstance(mod, ConvBR)}
        self.p = {name: _plan_entry(self._convs, (name,)) for name in self._convs}
        self.s1_group, self.s1_split, self.s0_pair, self.pair_steps = {}, set(), {}, {}
        cells = list(self.m.cells)
        for i, cell in enumerate(cells):
            self._plan_s1_group(i, cell)
        for i, cell in enumerate(cells) if self.PAIR_S0 else ():
            self._plan_s0_pair(i, cell)
        for i, cell in enumerate(cells) if self.PAIR_STEPS else ():
            self._plan_pair_steps(i, cell)
        for i, (cell, nxt) in enumerate(zip(cells, cells[1:])) if self.SHARE_DOWNSAMPLE else ():
            self._plan_share(i, cell, nxt)
        for i, (cell, nxt) in enumerate(zip(cells, cells[1:])) if self.FANOUT_1X1 else ():
            self._plan_fanout(i, cell, nxt)

    @staticmethod
    def _first_cat_state(cell):
        """The first state that is part of the cell's output (states: s0, s1, then one per step)."""
        return 2 + cell.steps - cell.block_multiplier

    def _plan_s1_group(self, i, cell):
        """Sibling ops: the DAG ops that read s1 (one per step: ops 1, 2, 4 of the matching
        genotype) write consecutive cat slots, so they run as ONE conv with cout = n*C over
        channels [.., ..) of the cell output (their weights and folded BN stacked along cout).
        The remaining ops accumulate."""
        group = []
        for k, terms in enumerate(cell.plan):
            for op, j in terms:
                if j == 1 and cell.op_kinds[op] == "conv":
                    group.append((k, op))
                    break
        steps = [k for k, _ in group]
        if (len(group) < 2 or steps != list(range(steps[0], steps[0] + len(steps)))
                or 2 + steps[0] < self._first_cat_state(cell)):
            return
        names = [f"cells.{i}._ops.{op}" for _, op in group]
        w0 = cell._ops[group[0][1]].conv.weight
        split = (self.SPLIT_S1_GROUP48 and WINOGRAD and len(names) == 3 and cell.c_out == 16
                 and w0.dim() == 5 and w0.shape[2] == 3)
        for key, part in ((("s1_group_head", names[:1]), ("s1_group", names[1:])) if split
                          else (("s1_group", names),)):
            self.p[f"cells.{i}.{key}"] = _plan_entry(self._convs, part)
        self.s1_group[i] = group
        if split:
            self.s1_split.add(i)

    def _plan_s0_pair(self, i, cell):
        """A 2D cell's two conv ops on s0 as one launch writing two slots (PAIR_S0)."""
        pair = [(k, op) for k, terms in enumerate(cell.plan) for op, j in terms
                if j == 0 and cell.op_kinds[op] == "conv"]
        if (len(pair) != 2 or cell.dims != 2 or 2 + pair[0][0] < self._first_cat_state(cell)
                or cell.c_out % 8 or 2 * cell.c_out > 32):
            return
        (k0, op0), (k1, op1) = pair
        m0, m1 = cell._ops[op0], cell._ops[op1]
        other = [(o, j) for o, j in cell.plan[k1] if o != op1]
        # the s1 sibling group writes its steps' slots without accumulating, after
        # the pair: a step both of them write would lose the pair's term
        if {k for k, _ in self.s1_group.get(i, [])} & {k0, k1}:
            return
        # op1 writes its step first (the other term a conv that accumulates after it)
        if (m0.relu != m1.relu or m0.conv.weight.dim() != 4 or m0.conv.weight.shape[-1] != 3
                or m0.stride != 1 or m1.stride != 1 or cell.plan[k1][0][0] != op1
                or not other or cell.op_kinds[other[0][0]] != "conv"):
            return
        self.p[f"cells.{i}.s0_pair"] = _plan_entry(self._convs, [f"cells.{i}._ops.{op0}", f"cells.{i}._ops.{op1}"])
        self.s0_pair[i] = pair

    def _plan_pair_steps(self, i, cell):
        """A 3D cell whose every step sums two 3x3x3 conv ops: one entry per step (PAIR_STEPS)."""
        terms = [[(op, j) for op, j in t] for t in cell.plan]
        if (cell.dims != 3 or not terms or cell.c_out not in self.PAIR_C
                or any(len(t) != 2 or any(cell.op_kinds[op] != "conv" for op, _ in t) for t in terms)):
            return
        if any(cell._ops[op].conv.weight.shape[-1] != 3 or not cell._ops[op].relu for t in terms for op, _ in t):
            return
        for k, t in enumerate(terms):
            # a LEA_PAIR_SUM step: [W_a | W_b] along cin, BN (a's, then b's)
            self.p[f"cells.{i}.pair{k}"] = _plan_entry(self._convs, [f"cells.{i}._ops.{op}" for op, _ in t], axis=1)
        self.pair_steps[i] = terms

    def _plan_share(self, i, cell, nxt):
        """A cell that resamples s1, followed by a same-level cell: the next cell's s0 is this s1
        (Cell.forward returns prev_input, skip_model_3d.py:75) at the same size, so both 1x1 convs
        run as one stacked conv over one read of it (down: interpolation in the conv's staging;
        up: one low-resolution conv and one up-sampling with the stacked BN)."""
        if (cell.downup_sample != 0 and nxt.downup_sample == 0
                and nxt.c_out == cell.c_out and self._first_cat_state(cell) == 1
                and cell.preprocess.conv.weight.shape[1] == nxt.pre_preprocess.conv.weight.shape[1]
                # the next cell applies pre_preprocess only when s0's channels differ
                # from its C_out (skip_model_3d.py:52); the memo path assumes it does
                and cell.preprocess.conv.weight.shape[1] != nxt.c_out):
            self.p[f"cells.{i}.share"] = _plan_entry(
                self._convs, [f"cells.{i + 1}.pre_preprocess", f"cells.{i}.preprocess"])

    def _plan_fanout(self, i, cell, nxt):
        """The same pair of readers where cell i does not resample down (no `share`): cell i's
        `preprocess` and cell i + 1's `pre_preprocess` both run a 1x1 at the source's own level --
        plain, or the raw conv of the commuted up-sampling (conv()) -- so one two-head launch reads
        the source once (cells.{i}.fanout: [this preprocess ; next pre_preprocess], each head
        keeping its own folded BN; which form each head takes is settled from the sizes at run
        time, _fanout_forms)."""
        wa, wb = cell.preprocess.conv.weight, nxt.pre_preprocess.conv.weight
        if (f"cells.{i}.share" in self.p or cell.dims != 3
                or wa.dim() != 5 or wa.shape[-1] != 1 or wb.shape[-1] != 1 or wa.shape[1] != wb.shape[1]
                or cell.downup_sample < 0 or cell.downup_sample + nxt.downup_sample < 0
                or wb.shape[1] == nxt.c_out):  # the next cell skips pre_preprocess
            return
        # (each head's BN / ReLU are its own ConvBR's)
        self.p[f"cells.{i}.fanout"] = _plan_entry(
            self._convs, [f"cells.{i}.preprocess", f"cells.{i + 1}.pre_preprocess"], bn=False)

    def _takes_winograd(self, p):
        """f32 3x3x3 layers the Winograd engine takes get its packed weight as well."""
        return WINOGRAD and p.kind == "3d" and kernels.wino_eligible(p.cout, p.cin, p.k)

    def _pack(self, name, p):
        """The f32 engines' operands of a planned entry: ``packed`` (the pair steps' weight
        concatenated along cin), and ``wino`` of the same weight where _takes_winograd."""
        w = _cat(_source_weights(self._convs, p), p.axis)
        if p.kind == "s3":
            p.packed = w.detach().contiguous()
        elif p.kind == "2d":
            p.packed = kernels.pack_conv2d_weight(w)
        else:
            p.packed = kernels.pack_conv_weight(w)
        if self._takes_winograd(p):
            p.wino = kernels.pack_conv_weight_wino(w)


    def _fanout_takes(self, x):
        """The two-head 1x1 (lea_conv1x1_heads) is an f32 device kernel."""
        return x.is_cuda and x.dtype == torch.float32

    def _fanout_forms(self, i, src, size):
        """For a planned cells.{i}.fanout on a source of volume ``src``: (next cell's size, this
        head commuted up-sampling?, next head commuted up-sampling?), or None where a head would
        not run at the source's own level (sizes that round to a down-sampling)."""
        nxt = self.m.cells[i + 1]
        sc = {0: None, -1: 0.5, 1: 2}[nxt.downup_sample]
        nsize = tuple(size) if sc is None else tuple(scale_dimension(n, sc) for n in size)
        ups = []
        for s in (tuple(size), nsize):
            if s != tuple(src) and not all(o >= n for o, n in zip(s, src)):
                return None
            ups.append(s != tuple(src))
        return nsize, ups[0], ups[1]

    def _fanout(self, i, x, size, forms, out, dn_out):
        """Cell i's s1 preprocess and cell i + 1's s0 pre_preprocess of the same source ``x`` as
        one two-head launch.  This cell's head goes where conv() puts it (``out``, or the raw z
        that the up-sampling reads; ``dn_out``: that up-sampling's level-down side output); the
        next cell's is handed on as the memo, keyed by the source and its size.  Returns
        (s1, memo)."""
        nsize, up_a, up_b = forms
        pa, pb = self.p[f"cells.{i}.preprocess"], self.p[f"cells.{i + 1}.pre_preprocess"]
        b, src = x.shape[0], self._volume(x)
        za = self._empty(b, pa.cout, src, x) if up_a or out is None else out
        zb = self._empty(b, pb.cout, src, x)
        fold = lambda p, up: (None, None, False) if up else (p.scale, p.shift, p.relu)
        kernels.conv1x1_heads(x, self.p[f"cells.{i}.fanout"].packed, pa.cout, *fold(pa, up_a),
                              pb.cout, *fold(pb, up_b), out_a=za, out_b=zb)
        if up_b:
            zb = kernels.resample_trilinear(zb, nsize, True, None, pb.scale, pb.shift, pb.relu)
        memo = (x, nsize, zb)
        if not up_a:
            return za, memo
        if dn_out is not None:
            return kernels.resample_trilinear_down2(za, size, out, dn_out, pa.scale, pa.shift, pa.relu)[0], memo
        return kernels.resample_trilinear(za, size, True, out, pa.scale, pa.shift, pa.relu), memo

    def conv(self, name, x, out=None, accumulate=False, x2=None, size=None, residual=None, down=None,
             down_only=False):
        """ConvBR ``name`` on x (or cat(x, x2)); with ``size`` != x's volume the input
        is trilinearly resampled (align_corners=True) inside the conv.  ``down``: the launch also
        writes the output's trilinear resample to half its volume there (``down_only``: and leaves
        ``out``, read as the residual, unfinished) -- the commuted up-sampling 1x1 and the
        depth-paired Winograd tiles have that form; anywhere else it is an error."""
        p = self.p[name]
        cin = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
        if cin != p.cin:
            raise ValueError(f"{name}: expected {p.cin} input channels, got {cin}")
        resized = size is not None and tuple(size) != tuple(x.shape[2:5])
        if p.kind == "s3":
            return kernels.conv2d_s3_bnrelu(x, p.packed, p.scale, p.shift, p.relu)
        if p.kind == "2d":
            if resized or x2 is not None:
                raise ValueError(f"{name}: 2D 3x3 conv takes one input at its own size")
            return kernels.conv2d_bnrelu(x, p.packed, p.cout, p.scale, p.shift, p.relu, out,
                                         accumulate, residual)
        if resized:
            if x2 is not None or residual is not None:
                raise ValueError("resampled conv takes one input and no residual")
            up = all(int(o) >= int(i) for o, i in zip(size, x.shape[2:]))
            if p.k == 1 and up and not accumulate:
                # interp and the 1x1 conv commute: conv at the low resolution, then
                # resample the narrow result with the BN/ReLU epilogue into `out`
                z = kernels.conv3d_bnrelu(x, p.packed, p.cout, 1, None, None, relu=False)
                if down is not None:  # the level-down copy from the same launch
                    return kernels.resample_trilinear_down2(z, size, out, down, p.scale, p.shift, p.relu)[0]
                return kernels.resample_trilinear(z, size, True, out, p.scale, p.shift, p.relu)
            if down is not None:
                raise ValueError(f"{name}: no down-sampling form of this resampled conv")
            return kernels.conv3d_bnrelu_resampled(x, size, p.packed, p.cout, p.k, p.scale,
                                                   p.shift, p.relu, out, accumulate)
        if p.wino is not None and kernels.wino_preferred(x.shape[0], p.cout, p.cin, *x.shape[2:5]):
            if down is not None:
                if x2 is not None:
                    raise ValueError(f"{name}: the down-sampling epilogue takes one input")
                kernels.conv3d_bnrelu_wino_dp_down2(x, p.wino, p.cout, p.scale, p.shift, p.relu, out, down,
                                                    accumulate, residual, only=down_only)
                return out
            return kernels.conv3d_bnrelu_wino(x, p.wino, p.cout, p.scale, p.shift, p.relu, out,
                                              accumulate, x2, residual)
        if down is not None:
            raise ValueError(f"{name}: no down-sampling epilogue on this conv's engine")
        return kernels.conv3d_bnrelu(x, p.packed, p.cout, p.k, p.scale, p.shift, p.relu, out,
                                     accumulate, x2, residual)

    def _pair_ok(self, x, x2, out):
        """The f32 pair launch's shape / alignment rule (lea_conv3d_bnrelu_wino, LEA_PAIR_SUM:
        the F(2,3) x F(2,3) tile, conv3d_wino22.hip)."""
        return kernels.pair_sum_supported(x, x2, out)

    def pair_conv(self, name, x, x2, out):
        p = self.p[name]
        return kernels.conv3d_bnrelu_wino(x, p.wino, p.cout, p.scale, p.shift, True, out, x2=x2, pair_sum=True)

    # activation layout hooks (f32 NCDHW here; the bf16 executor overrides them)
    def _empty(self, b, c, size, like):
        return torch.empty((b, c) + tuple(size), device=like.device, dtype=like.dtype)

    @staticmethod
    def _channels(t, c0, c1):
        return t[:, c0:c1]

    @staticmethod
    def _nchannels(t):
        return t.shape[1]

    @staticmethod
    def _volume(t):
        return tuple(t.shape[2:5])

    @staticmethod
    def _resample(x, size):
        return kernels.resample_trilinear(x, size)

    @staticmethod
    def _maps(t):
        """A one-plane result as the 2D maps its reader takes."""
        return t.squeeze(2)

    def _cell_output_takes_down(self, i, size):
        """Whether cell i's producers also write its output (at ``size``) one level down
        (MatchingExecutor)."""
        return False

    def cell(self, i, s0, s1, down=None, memo=None):
        """Cell.forward (skip_model_3d.py:41-75 / new_model_2d.py:41-75).  The level
        change of s1 (:44-48) and the size match of s0 (:49-51) are fused into the
        1x1 preprocess convs (:52-53) that consume them.  ``down`` = (s0, s1) already at
        this cell's size (either may be None), written by their producers' down-sampling
        epilogues: the preprocess convs then run at this level on them.  ``memo``: the previous
        cell's CellOut.memo.  Where this cell's own output is read only one level down
        (_cell_output_takes_down) that copy is the result's ``down`` (None otherwise)."""
        cell = self.m.cells[i]
        c, bm = cell.c_out, cell.block_multiplier
        s0_down, s1_down = down or (None, None)
        if s0_down is not None:
            s0 = s0_down
        if s1_down is not None:
            s1 = s1_down
        prev_input = s1
        size = self._cell_size(cell, s1, s1_down is not None)
        b = s1.shape[0]
        big = None
        if f"cells.{i}.share" in self.p:
            # this cell's s1 preprocess and the next cell's s0 pre_preprocess read the
            # same down-sampled tensor: one stacked 1x1 conv writes [next s0 | this s1]
            # into the channels just before and at the start of this cell's output
            big = self._empty(b, c + bm * c, size, s1)
            out = self._channels(big, c, c + bm * c)
        else:
            out = self._empty(b, bm * c, size, s1)
        first = self._first_cat_state(cell)
        slot = {first + k: self._channels(out, k * c, (k + 1) * c) for k in range(bm)}
        # the output's only reader is the next cell's down-sampling preprocess: its producers write
        # that level too (dslot, the same channel order), the last state nothing else
        dn = None
        if self._cell_output_takes_down(i, size) and self._down_kernels_take(s1, c, self._volume(s1), size):
            dn = self._empty(b, bm * c, tuple(n // 2 for n in size), s1)
        dslot = {} if dn is None else {idx: self._channels(dn, k * c, (k + 1) * c) for k, idx in enumerate(slot)}
        s0 = self._preprocess_s0(i, s0, size, slot.get(0), memo)
        s1, memo = self._preprocess_s1(i, s1, size, big, slot.get(1), dslot.get(1), s1_down is not None)
        if not self._paired_steps(i, s0, s1, slot):
            self._steps(i, s0, s1, size, out, slot, dslot)
        return CellOut(prev_input, out, dn, memo)

    def _cell_size(self, cell, s1, s1_down):
        """The cell's volume: s1's after its level change (unless its producer made it already)."""
        size = self._volume(s1)
        if cell.downup_sample != 0 and not s1_down:
            sc = 0.5 if cell.downup_sample < 0 else 2
            # the D axis of a 2D map stays 1 (bilinear on H, W only)
            size = tuple(n if (cell.dims == 2 and ax == 0) else scale_dimension(n, sc)
                         for ax, n in enumerate(size))
        return size

    def _preprocess_s0(self, i, s0, size, out, memo):
        """s0 at this cell's channels and size, copied or written into ``out`` (its slot) if it is
        part of the output."""
        if memo is not None and memo[0] is s0 and memo[1] == size:
            s0 = memo[2]  # computed by the previous cell's stacked conv
        elif self._nchannels(s0) != self.m.cells[i].c_out:
            return self.conv(f"cells.{i}.pre_preprocess", s0, out=out, size=size)
        elif self._volume(s0) != size:
            s0 = self._resample(s0, size)
        if out is not None:
            out.copy_(s0)
        return s0

    def _preprocess_s1(self, i, s1, size, big, out, dn_out, s1_down):
        """s1's preprocess into ``out`` (its slot): stacked with the next cell's pre_preprocess into
        ``big`` (share), as the two-head launch, or plain; ``dn_out``: its level-down side output.
        Returns (s1, the next cell's memo or None)."""
        c = self.m.cells[i].c_out
        if big is not None:
            self.conv(f"cells.{i}.share", s1, out=self._channels(big, 0, 2 * c), size=size)
            return self._channels(big, c, 2 * c), (s1, size, self._channels(big, 0, c))
        forms = None
        if (self.FANOUT_1X1 and f"cells.{i}.fanout" in self.p and not s1_down
                and not self.C8 and self._fanout_takes(s1)):
            forms = self._fanout_forms(i, self._volume(s1), size)
        if forms is not None and (dn_out is None or forms[1]):
            return self._fanout(i, s1, size, forms, out, dn_out)
        return self.conv(f"cells.{i}.preprocess", s1, out=out, size=size,
                         **({} if dn_out is None else {"down": dn_out})), None

    def _paired_steps(self, i, s0, s1, slot):
        """Every step as one LEA_PAIR_SUM launch, where the cell is planned so and the engine takes
        the operands; False where the generic steps have to run."""
        pairs = self.pair_steps.get(i)
        if pairs is None:
            return False
        states = [s0, s1]
        dsts = [slot.get(2 + k) for k in range(len(pairs))]
        if not (all(d is not None for d in dsts) and all(
                self._pair_ok(states[t[0][1]] if t[0][1] < 2 else dsts[t[0][1] - 2],
                              states[t[1][1]] if t[1][1] < 2 else dsts[t[1][1] - 2], dsts[k])
                for k, t in enumerate(pairs))):
            return False
        for k, ((_, ja), (_, jb)) in enumerate(pairs):
            self.pair_conv(f"cells.{i}.pair{k}", states[ja], states[jb], dsts[k])
            states.append(dsts[k])
        return True

    def _steps(self, i, s0, s1, size, out, slot, dslot):
        """The steps of the DAG: the s0 pair and the s1 sibling group first (one launch each, straight
        into their slots), then per step the remaining conv ops (a skip term as the first one's
        residual, accumulating once the slot is written) and the skip terms left.  ``dslot``: the
        launch that finishes a state writes it one level down there too."""
        cell = self.m.cells[i]
        c, b, n_states = cell.c_out, s1.shape[0], 2 + cell.steps
        states = [s0, s1]
        group = self.s1_group.get(i, [])
        written = set()
        done = set(group)
        consumed = set()  # steps whose skip term went in as an epilogue residual already
        pair = self.s0_pair.get(i)
        if pair is not None and self._nchannels(s0) == c and self._volume(s0) == size:
            (k0, op0), (k1, op1) = pair
            skips0 = [states[j] for o, j in cell.plan[k0] if cell.op_kinds[o] != "conv"]
            p = self.p[f"cells.{i}.s0_pair"]
            kernels.conv2d_bnrelu_pair(s0, p.packed, c, 2 * c, p.scale, p.shift, p.relu,
                                       slot[2 + k0], slot[2 + k1], skips0[-1] if skips0 else None)
            done |= {(k0, op0), (k1, op1)}
            written |= {k0, k1}
            if skips0:
                consumed.add(k0)
        if group:  # ops on s1 of every step, one launch, straight into their slots
            k0 = 2 + group[0][0] - self._first_cat_state(cell)
            if i in self.s1_split:
                self.conv(f"cells.{i}.s1_group", s1, out=self._channels(out, (k0 + 1) * c, (k0 + 3) * c))
                self.conv(f"cells.{i}.s1_group_head", s1, out=self._channels(out, k0 * c, (k0 + 1) * c))
            else:
                self.conv(f"cells.{i}.s1_group", s1, out=self._channels(out, k0 * c, (k0 + len(group)) * c))
            written |= {k for k, _ in group}
        for step, terms in enumerate(cell.plan):
            dst = slot.get(len(states))
            if dst is None:
                dst = self._empty(b, c, size, s1)
            skips = [states[j] for k, j in terms if cell.op_kinds[k] != "conv"]
            if step in consumed:
                skips.pop()
            todo = [k for k, _ in terms if (step, k) not in done and cell.op_kinds[k] == "conv"]
            for k, j in terms:
                if (step, k) in done or cell.op_kinds[k] != "conv":
                    continue
                residual = None
                if step not in written and skips:  # skip_connect term -> epilogue residual
                    residual = skips.pop()
                kw = {}
                if dslot and k == todo[-1]:  # the launch that finishes this state
                    kw = {"down": dslot[len(states)], "down_only": len(states) == n_states - 1}
                self.conv(f"cells.{i}._ops.{k}", states[j], out=dst, accumulate=step in written,
                          residual=residual, **kw)
                written.add(step)
            for t in skips:
                if step in written:
                    dst.add_(t)
                else:
                    dst.copy_(t)
                written.add(step)
            states.append(dst)



class MatchingExecutor(CellGraphExecutor):
    SPLIT_S1_GROUP48 = os.environ.get("LEASTEREO_SPLIT_GROUP48", "1") != "0"
    # the matching cells' steps as LEA_PAIR_SUM launches (LEASTEREO_PAIR_STEPS=0: the s1 group
    # + accumulating launches); the f32 pair runs on the Winograd F(2,3) x F(2,3) tile
    PAIR_STEPS = WINOGRAD and os.environ.get("LEASTEREO_PAIR_STEPS", "0") != "0"
    # the stems write cell 0's level themselves (the L0 -> L1 down-sampling as an epilogue): stem0's
    # factored kernel as a side output (lea_cv_stem_combine_down2), stem1 instead of its
    # full-resolution output (lea_conv3d_bnrelu_wino_down2), so cell 0's two 1x1 preprocess convs run
    # at L1 instead of each re-reading a whole L0 volume; LEASTEREO_FUSED_DOWN=0: the separate
    # resampling launches
    FUSED_DOWN = os.environ.get("LEASTEREO_FUSED_DOWN", "1") != "0"
    # the same inside the cell chain, a switch of its own: conv1's only reader is cell 5's stacked
    # 1x1 one level down (cells.5.share), so its epilogue writes that level and its own output never
    # exists (lea_conv3d_bnrelu_wino_down2_cat); and cell 10's output, read only by the last cell's
    # preprocess one level down: its producers write that level too (s1's up-sampling through
    # lea_resample3d_trilinear_down2, each step's finishing launch through
    # lea_conv3d_bnrelu_wino_dp_down2) and the last state's full-resolution values never exist;
    # LEASTEREO_FUSED_DOWN_CELLS=0: the resampling 1x1s
    FUSED_DOWN_CELLS = os.environ.get("LEASTEREO_FUSED_DOWN_CELLS", "1") != "0"
    # stem0's 2D maps that the combine kernels read on a few columns only (the masked left maps,
    # the K2 maps) computed on those columns alone (lea_conv2d_bnrelu_windowed); f32 device
    # tensors only; LEASTEREO_WINDOWED_MAPS=0: every map on every column
    WINDOWED_MAPS = os.environ.get("LEASTEREO_WINDOWED_MAPS", "1") != "0"
    # LEASTEREO_FANOUT_1X1=0: every 1x1 preprocess as a launch of its own
    FANOUT_1X1 = os.environ.get("LEASTEREO_FANOUT_1X1", "1") != "0"

    def run(self, x):
        """newMatching.forward (skip_model_3d.py:140-174): [B,64,D3,H3,W3] -> [B,1,D3,H3,W3]."""
        return self._from_stem0(self.conv("stem0", x))

    def run_features(self, fl, fr, maxdisp):
        """build_cost_volume + newMatching.forward (LEAStereo.py:34-50) with the cost
        volume read in place by stem0's conv (never materialised)."""
        p = self.p["stem0"]
        if fl.shape[1] * 2 != p.cin:
            raise ValueError(f"stem0 expects {p.cin} cost-volume channels, got 2*{fl.shape[1]}")
        d3 = int(maxdisp / 3)
        if self.cv is not None and kernels.cv_stem_supported(p.cout, d3, fl.shape[3], False):
            return self._from_stem0(*self._cv_stem(fl.unsqueeze(2), fr.unsqueeze(2), d3))
        if p.wino is not None and kernels.wino_preferred(fl.shape[0], p.cout, p.cin, int(maxdisp / 3),
                                                         *fl.shape[2:4]):
            stem0 = kernels.conv3d_bnrelu_costvolume_wino(fl, fr, maxdisp, p.wino, p.cout, p.scale,
                                                          p.shift, p.relu)
        else:
            stem0 = kernels.conv3d_bnrelu_costvolume(fl, fr, maxdisp, p.packed, p.cout, p.scale,
                                                     p.shift, p.relu)
        return self._from_stem0(stem0)

    def _cv_stem(self, fl5, fr5, d3):
        """stem0 = ConvBR3d(cost volume) (LEAStereo.py:34-48, skip_model_3d.py:141) as
        2D maps of each feature map + lea_cv_stem_combine (csrc/cv_stem.hip)."""
        p, (wl, wr) = self.p["stem0"], self.cv
        windowed = (self.WINDOWED_MAPS and self.cv_win is not None and fl5.is_cuda
                    and fl5.dtype == torch.float32)
        if windowed:
            # the masked left maps and the K2 maps only on the columns the combine kernels read
            # (kernels.cv_stem_map_windows); the left maps t-major, so the full-width ones lead
            lwin, rwin = kernels.cv_stem_map_windows(d3, fl5.shape[4])
            lm = kernels.conv2d_bnrelu_windowed(fl5, self.cv_win[0], 9 * p.cout, 3 * p.cout, (lwin,))
            rm = kernels.conv2d_bnrelu_windowed(fr5, self.cv_win[1], 6 * p.cout, 3 * p.cout, rwin)
        else:
            lm = kernels.conv2d_bnrelu(fl5, wl, 9 * p.cout, None, None, relu=False)
            rm = kernels.conv2d_bnrelu(fr5, wr, 6 * p.cout, None, None, relu=False)
        if self._cell0_takes_down((d3,) + tuple(lm.shape[3:5])) and kernels.cv_stem_down2_supported(lm, p.cout, d3):
            # (stem0, stem0 at cell 0's level): the side output of the same launch
            return kernels.cv_stem_combine_down2(lm, rm, p.cout, d3, p.scale, p.shift, p.relu, tmajor=windowed)
        return kernels.cv_stem_combine(lm, rm, p.cout, d3, p.scale, p.shift, p.relu, tmajor=windowed), None

    def _down_route(self, switch):
        """The part every *_takes_down predicate starts with: its switch on, no tap installed (the
        per-stage checks see today's launches), not the c8 layout."""
        return switch and self.tap is None and not self.C8

    @staticmethod
    def _halves(vol):
        """One level down is exactly half of ``vol``, an aligned 2 x 2 x 2 reduction."""
        return all(n % 2 == 0 and scale_dimension(n, 0.5) == n // 2 for n in vol)

    def _cell0_takes_down(self, vol):
        """Cell 0 reads the stems one level down, at exactly half of ``vol``: their producers may
        write that level themselves."""
        cells = self.m.cells
        return (self._down_route(self.FUSED_DOWN) and len(cells) > 0
                and cells[0].downup_sample < 0 and cells[0].dims == 3 and self._halves(vol))

    def _conv1_takes_down(self, vol):
        """conv1 (cat(outs[1], outs[4]) -> cell 5's s1) has one reader, cell 5's stacked 1x1
        (cells.5.share: cell 5's s1 and, through the share memo, cell 6's s0), which reads it at
        exactly half of ``vol``: conv1 may write that level itself."""
        cells = self.m.cells
        return (self._down_route(self.FUSED_DOWN_CELLS) and len(cells) == 12 and "cells.5.share" in self.p
                and cells[5].downup_sample < 0 and cells[5].dims == 3 and self._halves(vol))

    def _cell_output_takes_down(self, i, size):
        """Cell i's output (at ``size``) has one reader, the down-sampling ``preprocess`` of the
        next cell, at exactly half of an even volume: cell i + 1 is the last cell (no cell i + 2
        reads the output as its s0), takes its s1 alone (no ``share``), and neither conv1 nor conv2
        reads cell i.  The producers that have a down-sampling form must be the ones that run: s1
        from the commuted up-sampling 1x1, every step finished by a conv launch (no skip term left
        to add), the step launches not paired."""
        cells = self.m.cells
        n = len(cells)
        if not (self._down_route(self.FUSED_DOWN_CELLS) and 0 <= i and i + 2 == n
                and not (n == 12 and i in (1, 4, 8))):
            return False
        cell, nxt = cells[i], cells[i + 1]
        pre = self.p.get(f"cells.{i}.preprocess")
        return (cell.dims == 3 and nxt.dims == 3
                and nxt.downup_sample < 0 and f"cells.{i + 1}.share" not in self.p
                and cell.downup_sample > 0 and f"cells.{i}.share" not in self.p
                and pre is not None and pre.k == 1
                and self._first_cat_state(cell) == 1
                and self.pair_steps.get(i) is None and self.s0_pair.get(i) is None
                and all(cell.op_kinds[op] == "conv" for terms in cell.plan for op, _ in terms)
                and all(self._finishing_op(i, step) is not None for step in range(len(cell.plan)))
                and self._halves(size) and size[2] % 4 == 0)

    def _finishing_op(self, i, step):
        """The op whose launch writes step ``step``'s state last (the s1 sibling group runs first),
        where that launch is a Winograd conv; else None."""
        group = self.s1_group.get(i, [])
        rest = [op for op, _ in self.m.cells[i].plan[step] if (step, op) not in group]
        if not rest or self.p[f"cells.{i}._ops.{rest[-1]}"].wino is None:
            return None
        return rest[-1]

    def _down_kernels_take(self, like, c, in_size, size):
        """The *_supported queries of the launches _cell_output_takes_down's route runs, for f32
        device tensors like ``like`` (the cell's s1)."""
        b = like.shape[0]
        return (like.is_cuda and like.dtype == torch.float32
                and kernels.wino_preferred(b, c, c, *size)
                and kernels.wino_dp_down2_kernel_name(b, c, c, *size) is not None
                and kernels.resample_down2_shape_supported(in_size, size))

    def _cv_stem_pack(self, wl, wr):
        return kernels.pack_conv2d_weight(wl), kernels.pack_conv2d_weight(wr)

    def _from_stem0(self, stem0, stem0_down=None):
        out = self._matching_body(stem0, stem0_down)
        if self.tap is not None:  # the head's output is f32 NCDHW in every executor
            self.tap("matching", out.detach().clone())
        return out

    def _matching_body(self, stem0, stem0_down=None):
        d, h, w = self._volume(stem0)
        self._emit("stem0", stem0)
        stem1 = stem1_down = None
        p1 = self.p["stem1"]
        if ("cells.0.share" in self.p and self._cell0_takes_down((d, h, w)) and p1.wino is not None
                and kernels.wino_preferred(stem0.shape[0], p1.cout, p1.cin, d, h, w)
                and kernels.conv3d_wino_down2_supported(stem0, p1.cout)):
            # stem1's only readers are cell 0's s1 and cell 1's s0 (the share memo), both one
            # level down: its epilogue writes that level and the full-resolution output never
            # exists (lea_conv3d_bnrelu_wino_down2)
            stem1_down = kernels.conv3d_bnrelu_wino_down2(stem0, p1.wino, p1.cout, p1.scale, p1.shift, p1.relu)
        else:
            stem1 = self.conv("stem1", stem0)
            self._emit("stem1", stem1)
        outs = []
        # the carry: the next cell's (s0, s1), either of them already at its level (down), its memo
        s0, s1, down, memo = stem0, stem1, (stem0_down, stem1_down), None
        n = len(self.m.cells)
        for i in range(n):
            if i == 5 and n == 12:   # :150-151, cat read in place by the conv
                pc, xa, xb = self.p["conv1"], outs[1].out, outs[4].out
                if (self._conv1_takes_down(self._volume(xa)) and pc.wino is not None
                        and kernels.wino_preferred(xa.shape[0], pc.cout, pc.cin, *xa.shape[2:5])
                        and kernels.conv3d_wino_down2_cat_supported(xa, xb, pc.cout)):
                    down = (None, kernels.conv3d_bnrelu_wino_down2_cat(xa, xb, pc.wino, pc.cout, pc.scale,
                                                                       pc.shift, pc.relu))
                    s0, s1 = outs[4].s0, None
                else:
                    s0, s1 = outs[4].s0, self.conv("conv1", xa, x2=xb)
                    self._emit("conv1", s1)
            elif i == 9 and n == 12:  # :155-156
                s0, s1 = outs[8].s0, self.conv("conv2", outs[4].out, x2=outs[8].out)
                self._emit("conv2", s1)
            o = self.cell(i, s0, s1, down=down, memo=memo)
            self._emit(f"cell{i}", o.out)
            outs.append(o)
            # (down: where cell i wrote its output at the next cell's level as well)
            s0, s1, down, memo = o.s0, o.out, (None, o.down), o.memo
        last = outs[-1].out
        lh = self._volume(last)[1]
        full, half, quarter = (d, h, w), (d // 2, h // 2, w // 2), (d // 4, h // 4, w // 4)
        # head (:161-173): the 1x1 Upsample pairs run commuted (see conv()); the final
        # Upsample + last_3 run as per-tap partial sums at the low resolution, then one
        # 27-sample interpolating sum per output voxel (no full-resolution 32-ch tensor)
        if lh == h:
            return self._last3_same_size(last)
        if lh == h // 2:
            y = self.conv("last_6", last)
        elif lh == h // 4:
            y = self.conv("last_6", self.conv("last_12", last), size=half)
        elif lh == h // 8:
            y = self.conv("last_12", self.conv("last_24", last), size=quarter)
            y = self.conv("last_6", y, size=half)
        else:
            raise ValueError(f"matching-net output size {tuple(last.shape[2:])} has no head")
        p3 = self.p["last_3"]
        q = self.conv("last_3.taps", y)
        return self._tapsum(q, p3, full)

    @staticmethod
    def _tapsum(q, p3, full):
        return kernels.tapsum_upsample(q, p3.cout, full, p3.scale, p3.shift, p3.relu)

    def _last3_same_size(self, last):
        return self.conv("last_3", last)

    def __init__(self, matching):
        super().__init__(matching)
        self.cv = self.cv_win = None
        if CV_STEM:
            with torch.no_grad():
                self._factor_stem0()

    def _plan(self):
        super()._plan()
        # Head: last_3(Upsample(y)) = sum over taps of upsampled per-tap partial
        # sums (lea_tapsum_upsample); the taps run as a 1x1 conv with 27*cout outputs
        # (c8: 27*cout channels padded to a block)
        co, ci = self.m.last_3.conv.weight.shape[:2]
        cout = co * 27 + ((-co * 27) % 8 if self.C8 else 0)
        self.p["last_3.taps"] = ConvParams(None, None, None, ci, cout, 1, False, sources=("last_3",), taps=True)

    def _factor_stem0(self):
        """The factored stem0's operands: ``cv``, the 2D map weights of each feature map, and
        ``cv_win``, the windowed route's own (f32 only)."""
        wl, wr = kernels.cv_stem_split_weights(self.m.stem0.conv.weight)
        self.cv = self._cv_stem_pack(wl, wr)
        if self.WINDOWED_MAPS and not self.C8:
            # the windowed route's own operands: left rows (3 kd + t) cout + o -> t-major,
            # both packed as [full-width rows ; windowed rows]
            co = wl.shape[0] // 9
            wlt = wl.view(3, 3, co, *wl.shape[1:]).transpose(0, 1).reshape(wl.shape)
            self.cv_win = (kernels.pack_conv2d_weight_windowed(wlt, 3 * co),
                           kernels.pack_conv2d_weight_windowed(wr, 3 * co))


class MatchingExecutorDirect(MatchingExecutor):
    """newMatching.forward on the direct implicit-GEMM engine only: stem0 reads the
    cost volume in place (no factored 2D maps) and no layer runs Winograd.  An
    independent algorithm for the same f32 arithmetic, used by bench.py as the
    per-pair cross-check of every rank's shard (precision "f32_direct")."""

    SPLIT_S1_GROUP48 = False
    PAIR_STEPS = False
    FANOUT_1X1 = False  # the cross-check keeps the single launches

    def _factor_stem0(self):
        """No factored stem."""

    def _takes_winograd(self, p):
        """Direct engine only."""
        return False


class FeatureExecutor(CellGraphExecutor):
    # stems 0 and 1 as one kernel (csrc/feature_stem.hip); LEASTEREO_FEATURE_STEM=0 runs
    # them as two convs
    FUSED_STEM = os.environ.get("LEASTEREO_FEATURE_STEM", "1") != "0"
    PAIR_S0 = os.environ.get("LEASTEREO_PAIR_S0", "1") != "0"

    def _stems(self, x, c8=False, x2=None):
        """new_model_2d.py:93-94 (stem1(stem0(x))), fused where the kernel is instantiated;
        with x2 the images of x then x2 as one batch (the fused stem reads both sources,
        no concatenated copy)."""
        p0, p1 = self.p["stem0"], self.p["stem1"]
        if (self.FUSED_STEM and p0.relu and p1.relu and (p0.cin, p0.cout, p1.cout) == (3, 16, 32)
                and p1.kind == "s3"):
            return kernels.feature_stem(x, self.m.stem0.conv.weight, p0.scale, p0.shift, p1.packed,
                                        p1.scale, p1.shift, c8, x2)
        if x2 is not None:
            x = torch.cat((x, x2), 0)
        stem1 = self.conv("stem1", self.conv("stem0", x.unsqueeze(2)))
        return kernels.to_c8(stem1) if c8 else stem1

    def run(self, x, x2=None):
        """newFeature.forward (new_model_2d.py:140-165): [N,3,H,W] -> [N,32,H/3,W/3]
        (with x2: the stacked features of x then x2).  One graph for both layouts, through the
        layout hooks (bf16: c8 maps [N, 32/8, 1, H/3, W/3, 8])."""
        stem1 = self._stems(x, c8=self.C8, x2=x2)
        stem2 = self.conv("stem2", stem1)
        o = CellOut(stem1, stem2)
        for i in range(len(self.m.cells)):
            o = self.cell(i, o.s0, o.out, memo=o.memo)
        last = o.out
        h, w = self._volume(stem2)[1:]
        lh = self._volume(last)[1]
        full, half, quarter = (1, h, w), (1, h // 2, w // 2), (1, h // 4, w // 4)
        # head (:156-163): ConvBR at the low level, then nn.Upsample; a ConvBR after an
        # Upsample reads it through conv(size=...) (interpolation fused/commuted)
        if lh == h:
            y = last
        elif lh == h // 2:
            y = self._resample(self.conv("last_6", last), full)
        elif lh == h // 4:
            y = self.conv("last_6", self.conv("last_12", last), size=half)
            y = self._resample(y, full)
        elif lh == h // 8:
            # new_model_2d.py:163: last_12(up_24(last_24(x))), then last_6(up_12(.)), up_6
            y = self.conv("last_12", self.conv("last_24", last), size=quarter)
            y = self._resample(self.conv("last_6", y, size=half), full)
        else:
            # the reference raises UnboundLocalError here (new_model_2d.py:156-165)
            raise ValueError(f"feature size {tuple(x.shape[2:])} is not legal for the feature net")
        return self._maps(self.conv("last_3", y))


def _fresh_memo(run):
    """A forward of a bf16 executor: the resample memo (_C8Layout._downsampled) empty before it and
    dropped after it, however it ends."""
    @functools.wraps(run)
    def forward(self, *args, **kw):
        self._rs_memo = None
        try:
            return run(self, *args, **kw)
        finally:
            self._rs_memo = None
    return forward


class _C8Layout:
    """Activation-layout hooks of the bf16 executors: c8 tensors
    ([B, C/8, D, H, W, 8] bfloat16), channel slices on block boundaries."""

    C8 = True
    _rs_memo = None

    # down-sampling 1x1 convs read their input through the interpolating gather-GEMM
    # (lea_conv1x1_resampled_bf16), so the shared-preprocess stacking applies as in fp32
    # (LEASTEREO_BF16_FUSED_RS=0: materialise + memoise the resampled tensor instead)
    FUSED_RS = os.environ.get("LEASTEREO_BF16_FUSED_RS", "1") != "0"
    SHARE_DOWNSAMPLE = FUSED_RS and CellGraphExecutor.SHARE_DOWNSAMPLE

    def _empty(self, b, c, size, like):
        return torch.empty((b, c // 8) + tuple(size) + (8,), device=like.device, dtype=torch.bfloat16)

    @staticmethod
    def _as_f32(t):
        return kernels.from_c8(t)

    @staticmethod
    def _channels(t, c0, c1):
        return t[:, c0 // 8:c1 // 8]

    @staticmethod
    def _nchannels(t):
        return t.shape[1] * 8

    @staticmethod
    def _resample(x, size):
        return kernels.resample_trilinear_bf16(x, size)

    @staticmethod
    def _maps(t):
        return t

    def _pack(self, name, p):
        """The bf16 engines' fragments of a planned entry, and nothing else (same scale/shift).  A
        pair step: each half packed, the packs one after the other."""
        ws = _source_weights(self._convs, p)
        if p.kind == "2d":
            p.packed, p.kind = kernels.pack_conv2d_weight_bf16(_cat(ws)), "bf16_2d"
        elif p.axis == 1:
            p.packed, p.kind = torch.cat([kernels.pack_conv_weight_bf16(w) for w in ws]), "bf16"
        else:
            p.packed, p.kind = kernels.pack_conv_weight_bf16(_cat(ws)), "bf16"

    def _downsampled(self, x, size):
        """Materialised trilinear resample of a c8 tensor, memoised for one reuse: cell i
        resizes its s1 (skip_model_3d.py:44-48) and cell i+1 resizes the same raw tensor
        as its s0 to the same size (:49-51) -- stem1 L0->L1, cell1's output and conv1's
        L1->L2.  The memo holds the source itself (no address reuse while cached) and
        is dropped at the end of every forward (_fresh_memo)."""
        memo = self._rs_memo
        if memo is not None and memo[0] is x and memo[1] == tuple(size):
            return memo[2]
        y = kernels.resample_trilinear_bf16(x, size)
        self._rs_memo = (x, tuple(size), y)
        return y

    def _conv_c8(self, name, x, out=None, accumulate=False, x2=None, size=None, residual=None):
        p = self.p[name]
        cin = (x.shape[1] + (x2.shape[1] if x2 is not None else 0)) * 8
        if cin != p.cin:
            raise ValueError(f"{name}: expected {p.cin} input channels, got {cin}")
        if size is not None and tuple(size) != tuple(x.shape[2:5]):
            if x2 is not None or residual is not None or accumulate:
                raise ValueError("resampled conv takes one input and no residual")
            up = all(int(o) >= int(i) for o, i in zip(size, x.shape[2:5]))
            if p.k == 1 and up:  # commuted: 1x1 at the low resolution, resample + BN/ReLU
                z = kernels.conv3d_bnrelu_bf16(x, p.packed, p.cout, 1, None, None, relu=False)
                return kernels.resample_trilinear_bf16(z, size, True, out, p.scale, p.shift, p.relu)
            if (self.FUSED_RS and p.k == 1 and p.kind == "bf16" and p.cin % 32 == 0 and p.cin <= 128
                    and p.cout in (16, 32, 64)):
                return kernels.conv1x1_resampled_bf16(x, size, p.packed, p.cout, p.scale, p.shift,
                                                      p.relu, out)
            x = self._downsampled(x, size)
        if p.kind == "bf16_2d":
            if x2 is not None:
                raise ValueError(f"{name}: 2D conv takes one input")
            return kernels.conv2d_bnrelu_bf16(x, p.packed, p.cout, p.scale, p.shift, p.relu, out,
                                              accumulate, residual)
        return kernels.conv3d_bnrelu_bf16(x, p.packed, p.cout, p.k, p.scale, p.shift, p.relu, out,
                                          accumulate, x2, residual)


class MatchingExecutorBF16(_C8Layout, MatchingExecutor):
    """newMatching.forward at bf16 (configs 3/4): activations in the c8 layout
    ([B, C/8, D, H, W, 8] bfloat16), convs on the bf16 matrix cores with f32
    accumulation and the f32 BN epilogue; the head's output (the matching cost)
    is f32 for the disparity regression.  Same graph as MatchingExecutor."""

    SPLIT_S1_GROUP48 = False
    FANOUT_1X1 = False  # (the two-head 1x1 is an f32 kernel)
    # the L0 / L1 cells' steps (8 or 16 channels: one K chunk per conv) as LEA_PAIR_SUM
    # launches of the D-streaming kernel; the L2 cells keep the group + accumulating launches
    PAIR_STEPS = os.environ.get("LEASTEREO_PAIR_STEPS", "1") != "0"

    def _pack(self, name, p):
        if name != "last_3":  # runs through last_3.taps + tap-sum: only its cout and BN are read
            super()._pack(name, p)

    def _pair_ok(self, x, x2, out):
        return kernels.pair_sum_supported_bf16(x, x2, out)

    def pair_conv(self, name, x, x2, out):
        p = self.p[name]
        return kernels.conv3d_bnrelu_bf16(x, p.packed, p.cout, 3, p.scale, p.shift, True, out, x2=x2,
                                          pair_sum=True)

    def _cv_stem_pack(self, wl, wr):
        return kernels.pack_conv2d_weight_bf16(wl), kernels.pack_conv2d_weight_bf16(wr)

    def _cv_stem(self, fl8, fr8, d3):
        p, (wl, wr) = self.p["stem0"], self.cv
        lm = kernels.conv2d_bnrelu_bf16(fl8, wl, 9 * p.cout, None, None, relu=False)
        rm = kernels.conv2d_bnrelu_bf16(fr8, wr, 6 * p.cout, None, None, relu=False)
        return kernels.cv_stem_combine(lm, rm, p.cout, d3, p.scale, p.shift, p.relu,
                                       name="cv_stem_c8_kernel")

    @staticmethod
    def _tapsum(q, p3, full):
        return kernels.tapsum_upsample_bf16(q, p3.cout, full, p3.scale, p3.shift, p3.relu)

    def _last3_same_size(self, last):
        # per-tap partial sums + a tap-sum at the same size (identity interpolation)
        return self._tapsum(self.conv("last_3.taps", last), self.p["last_3"], self._volume(last))

    def conv(self, *args, **kw):
        return self._conv_c8(*args, **kw)

    @_fresh_memo
    def run(self, x):
        """x: f32 cost volume [B, 64, D3, H3, W3] -> f32 matching cost [B, 1, D3, H3, W3]."""
        return self._from_stem0(self.conv("stem0", kernels.to_c8(x)))

    @_fresh_memo
    def run_features(self, fl, fr, maxdisp):
        p = self.p["stem0"]
        cf = fl.shape[1] * (8 if fl.dtype == torch.bfloat16 else 1)
        if cf * 2 != p.cin:
            raise ValueError(f"stem0 expects {p.cin} cost-volume channels, got 2*{cf}")
        if fl.dtype == torch.bfloat16:  # the bf16 feature net already hands over c8 maps
            f8, b = _stacked(fl, fr), fl.shape[0]
        else:
            f8 = kernels.to_c8(_stacked(fl, fr))  # [2B, C/8, 1, H, W, 8]
            b = fl.shape[0]
        d3 = int(maxdisp / 3)
        if self.cv is not None and kernels.cv_stem_supported(p.cout, d3, f8.shape[4], True):
            return self._from_stem0(self._cv_stem(f8[:b], f8[b:], d3))
        stem0 = kernels.conv3d_bnrelu_costvolume_bf16(f8[:b], f8[b:], maxdisp, p.packed, p.cout,
                                                      p.scale, p.shift, p.relu)
        return self._from_stem0(stem0)


class FeatureExecutorBF16(_C8Layout, FeatureExecutor):
    """newFeature.forward at bf16 (configs 3/4): stem0 (3 input channels) and the
    stride-3 stem1 stay f32; from stem2 on the maps are c8 and the 3x3 convs run on
    the bf16 engine's 2D tiles.  Returns c8 feature maps [N, 32/8, 1, H3, W3, 8],
    which the bf16 matching net reads directly."""
    PAIR_S0 = False  # (the pair launch is the f32 few-channel tile's)

    def _pack(self, name, p):
        if name in ("stem0", "stem1"):
            CellGraphExecutor._pack(self, name, p)
        else:
            super()._pack(name, p)

    def conv(self, name, x, *args, **kw):
        if name in ("stem0", "stem1"):
            return CellGraphExecutor.conv(self, name, x, *args, **kw)
        return self._conv_c8(name, x, *args, **kw)

    run = _fresh_memo(FeatureExecutor.run)
