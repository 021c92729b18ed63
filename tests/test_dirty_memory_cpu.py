"""tests/dirty_memory.py on the CPU: the allocation path, the guards, the restore."""
import ast
import math
import os

import pytest
import torch

from tests import dirty_memory as dm

ORIG = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


def _restored():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty) == ORIG


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.uint8])
def test_payload_pattern(dtype):
    with dm.dirty(dm.NAN, "cpu") as mem:
        t = torch.empty((3, 5), dtype=dtype, device="cpu")
        assert t.dtype == dtype and tuple(t.shape) == (3, 5)
        if dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        elif dtype == torch.uint8:
            assert bool((t == 255).all())
        else:
            assert bool((t == -1).all())
        mem.check()
    with dm.dirty(dm.BIG, "cpu") as mem:
        t = torch.empty(7, dtype=dtype, device="cpu")
        if dtype in (torch.float32, torch.bfloat16):
            assert bool(torch.isfinite(t).all()) and 1.4e13 < float(t[0]) < 1.6e13
        elif dtype == torch.int32:
            assert int(t[0]) == 0x55555555
        elif dtype == torch.uint8:
            assert int(t[0]) == 0x55
        else:
            assert bool(torch.isfinite(t).all())
        mem.check()
    with dm.dirty(dm.CLEAN, "cpu") as mem:
        assert not bool(torch.empty(4, 4, dtype=dtype).any())
        mem.check()
    assert _restored()


def test_shapes_strides_alignment():
    with dm.dirty(dm.NAN, "cpu") as mem:
        for shape in [(2, 3, 4), (1,), (5, 1, 7), (0,), (3, 0, 2), ()]:
            t = torch.empty(shape, dtype=torch.float32, device="cpu")
            want = torch.zeros(shape)
            assert tuple(t.shape) == shape and t.stride() == want.stride() and t.is_contiguous()
            assert t.data_ptr() % 16 == 0
            t.zero_()  # writable over the whole payload
        assert tuple(torch.empty(2, 3).shape) == (2, 3)  # varargs size, default dtype and device
        assert tuple(torch.empty(size=(4,)).shape) == (4,)
        assert torch.empty(torch.Size((2, 2)), dtype=torch.int64).dtype == torch.int64
        assert len(mem.allocations) == 9
        mem.check()


def test_empty_like_and_new_empty_are_guarded():
    with dm.dirty(dm.NAN, "cpu") as mem:
        a = torch.empty((4, 6), dtype=torch.float32)
        b = torch.empty_like(a)
        c = torch.empty_like(a, dtype=torch.int32)
        d = a.new_empty((2, 5))
        e = a.new_empty(3, dtype=torch.uint8)
        assert len(mem.allocations) == 5
        assert bool(torch.isnan(b).all()) and bool((c == -1).all()) and c.shape == a.shape
        assert bool(torch.isnan(d).all()) and d.dtype == torch.float32 and tuple(d.shape) == (2, 5)
        assert bool((e == 255).all())
        # a permuted (dense, non-contiguous) prototype keeps its strides, as the real empty_like does
        p = a.t()
        q = torch.empty_like(p)
        assert q.shape == p.shape and q.stride() == p.stride() and bool(torch.isnan(q).all())
        assert len(mem.allocations) == 6
        mem.check()


@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_overrun_by_one_element_is_seen(side, dtype):
    with dm.dirty(dm.CLEAN, "cpu") as mem:
        t = torch.empty((3, 4), dtype=dtype)
        mem.check()
        off = t.storage_offset() - 1 if side == "before" else t.storage_offset() + t.numel()
        t.as_strided((1,), (1,), off).fill_(1)
        with pytest.raises(AssertionError) as err:
            mem.check()
        text = str(err.value)
        assert side in text and "(3, 4)" in text and str(dtype) in text
        with pytest.raises(AssertionError):
            dm.check()  # the module-level form checks the active block


def test_restored_after_exception():
    with pytest.raises(KeyError):
        with dm.dirty(dm.NAN, "cpu"):
            assert not _restored()
            raise KeyError("boom")
    assert _restored()
    assert not math.isnan(float(torch.zeros(1)))
    with pytest.raises(RuntimeError):
        dm.check()


def test_other_device_and_unknown_keywords_pass_through():
    with dm.dirty(dm.NAN, "cpu") as mem:
        m = torch.empty((2, 2), device="meta")
        assert m.device.type == "meta"
        assert torch.empty_like(m).device.type == "meta"
        assert m.new_empty((3,)).device.type == "meta"
        out = torch.zeros(4)
        assert torch.empty(4, out=out) is out
        torch.empty((2,), requires_grad=True)
        torch.empty((2,), pin_memory=False)
        torch.empty((1, 1, 2, 2), memory_format=torch.channels_last)
        torch.empty_like(out, requires_grad=False)
        assert mem.allocations == []
    with dm.dirty(dm.NAN, "meta") as mem:  # and the other way round: the CPU is the other device
        torch.empty(3, device="cpu")
        assert mem.allocations == []


def test_bits_compares_nan_equal():
    a = torch.tensor([float("nan"), 1.0])
    assert torch.equal(dm.bits(a), dm.bits(a.clone()))
    assert not torch.equal(a, a.clone())
    assert dm.bits(a.to(torch.bfloat16)).dtype == torch.int16 and dm.bits(a.double()).dtype == torch.int64


# ------------------------------------------------------------------ the coverage guard
ALLOCATORS = {"empty", "empty_like", "new_empty"}
MODULES = ("kernels", "training")


def _allocating_public_functions(module):
    """``module.name`` of every public top-level function of leastereo_amd/<module>.py whose body
    calls torch.empty / empty_like / new_empty, directly or through private top-level functions or
    classes of the same module (an autograd Function's methods count as the class)."""
    import leastereo_amd
    path = os.path.join(os.path.dirname(os.path.abspath(leastereo_amd.__file__)), module + ".py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    top = {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    direct, refs = {}, {}
    for name, node in top.items():
        calls = [c for c in ast.walk(node) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)]
        direct[name] = any(c.func.attr in ALLOCATORS for c in calls)
        refs[name] = {n.id for n in ast.walk(node) if isinstance(n, ast.Name) and n.id in top
                      and n.id.startswith("_") and n.id != name}

    def allocates(name, seen=()):
        return direct[name] or any(allocates(r, seen + (name,)) for r in refs[name] if r not in seen)
    return {f"{module}.{name}" for name, node in top.items()
            if isinstance(node, ast.FunctionDef) and not name.startswith("_") and allocates(name)}


def test_every_allocating_wrapper_has_a_dirty_memory_case():
    """A new wrapper cannot join the library without a case in tests/test_gpu_dirty_memory.py (or
    an exemption with its reason there)."""
    from tests import test_gpu_dirty_memory as G
    need = set().union(*(_allocating_public_functions(m) for m in MODULES))
    assert len(need) >= 60, sorted(need)  # sanity of the parse
    assert {"kernels.conv3d_bnrelu", "kernels.speckle_filter", "training.convbr3d", "training.resample3d_backward"} <= need
    have = G.covered()
    assert all(isinstance(r, str) and r for r in G.EXEMPT.values())
    missing = sorted(need - have - set(G.EXEMPT))
    assert not missing, f"no dirty-memory case and no exemption: {missing}"
    import leastereo_amd.kernels
    import leastereo_amd.training
    stale = sorted(n for n in have | set(G.EXEMPT) if not callable(getattr(getattr(leastereo_amd, n.split(".")[0]),
                                                                           n.split(".")[1], None)))
    assert not stale, f"named in the case table or the exemptions but no function of the library: {stale}"
    assert set(G.EXEMPT) <= need, "an exemption for a function that does not allocate"
    assert not set(G.EXEMPT) & have, "exempt and covered at once"
    assert all(key in open(G.__file__).read() for key in G.UNDEFINED)
