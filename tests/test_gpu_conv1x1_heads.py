"""The two-head streaming 1x1 (lea_conv1x1_heads): two 1x1 ConvBR3d of the same input over one
read of it.  It merges work and changes no arithmetic -- each output's k-steps are those of its
own single launch -- so every comparison is torch.equal against the two ``conv3d_bnrelu(k=1)``
launches it replaces.

Shapes: the matching net's pairs (64 -> 16 with BN + ReLU and 8 raw; 128 -> 32 and 16), a cin
with a partial 32-channel chunk, a second source; a volume on the scalar tail (3 x 5 x 7: 105
voxels, not a multiple of 4) and one on the vector path (4 x 6 x 16); batch 2 with head A written
into a channel slice of a wider tensor (batch stride != cout * V)."""
import ctypes

import pytest
import torch

from leastereo_amd import _lib, kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"

VOLUMES = [(3, 5, 7), (4, 6, 16)]
# (cin, cin2, cout_a, BN + ReLU on a, cout_b, BN + ReLU on b)
HEADS = [(64, 0, 16, True, 8, False), (128, 0, 32, True, 16, False), (64, 0, 8, False, 16, True),
         (40, 0, 16, True, 16, True), (32, 32, 16, True, 8, False), (24, 16, 32, True, 32, True)]


def _operands(b, cin, cin2, cout_a, cout_b, vol, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((b, cin) + vol, device=DEV, generator=g)
    x2 = torch.randn((b, cin2) + vol, device=DEV, generator=g) if cin2 else None
    ws, folds = [], []
    for cout in (cout_a, cout_b):
        ws.append(torch.randn(cout, cin + cin2, 1, 1, 1, device=DEV, generator=g) / (cin + cin2) ** 0.5)
        folds.append((torch.rand(cout, device=DEV, generator=g) + 0.5,
                      torch.randn(cout, device=DEV, generator=g) * 0.1))
    return x, x2, ws, folds


@pytest.mark.parametrize("vol", VOLUMES)
@pytest.mark.parametrize("cin,cin2,cout_a,bn_a,cout_b,bn_b", HEADS)
@pytest.mark.parametrize("b", [1, 2])
def test_each_head_is_its_single_launch(b, cin, cin2, cout_a, bn_a, cout_b, bn_b, vol):
    x, x2, (wa, wb), (fa, fb) = _operands(b, cin, cin2, cout_a, cout_b, vol, cin + cout_a + vol[2])
    fa = fa if bn_a else (None, None)
    fb = fb if bn_b else (None, None)
    want_a = kernels.conv3d_bnrelu(x, kernels.pack_conv_weight(wa), cout_a, 1, *fa, relu=bn_a, x2=x2)
    want_b = kernels.conv3d_bnrelu(x, kernels.pack_conv_weight(wb), cout_b, 1, *fb, relu=bn_b, x2=x2)
    stacked = kernels.pack_conv_weight(torch.cat((wa, wb), 0))
    # head A into channels [4, 4 + cout_a) of a wider tensor, head B into a tensor of its own
    wide = torch.full((b, cout_a + 12) + vol, float("nan"), device=DEV)
    got_a, got_b = kernels.conv1x1_heads(x, stacked, cout_a, *fa, bn_a, cout_b, *fb, bn_b,
                                         out_a=wide[:, 4:4 + cout_a], x2=x2)
    assert got_a.data_ptr() == wide[:, 4:4 + cout_a].data_ptr()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    assert wide[:, :4].isnan().all() and wide[:, 4 + cout_a:].isnan().all()
    assert not want_a.isnan().any() and not want_b.isnan().any()


def test_both_forms_of_the_kernel_agree():
    """The vector form (lea_conv1x1_set_vector) and the one-float-per-lane form of the two-head
    kernel store the same values, as the single-output kernel's do."""
    x, _, (wa, wb), (fa, fb) = _operands(2, 64, 0, 16, 8, (4, 6, 16), 5)
    stacked = kernels.pack_conv_weight(torch.cat((wa, wb), 0))
    outs = []
    for on in (0, 1):
        with _lib.tuning(lea_conv1x1_set_vector=on):
            outs.append(kernels.conv1x1_heads(x, stacked, 16, *fa, True, 8, None, None, False))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_residual_and_accumulate_are_refused():
    x, _, (wa, wb), (fa, fb) = _operands(1, 32, 0, 16, 8, (2, 4, 8), 9)
    stacked = kernels.pack_conv_weight(torch.cat((wa, wb), 0))
    ya, yb = torch.empty((1, 16, 2, 4, 8), device=DEV), torch.empty((1, 8, 2, 4, 8), device=DEV)
    with pytest.raises(ValueError, match="residual"):
        kernels.conv1x1_heads(x, stacked, 16, *fa, True, 8, *fb, True, out_a=ya, out_b=yb, accumulate=True)
    with pytest.raises(ValueError, match="residual"):
        kernels.conv1x1_heads(x, stacked, 16, *fa, True, 8, *fb, True, residual=ya)
    lib = _lib.load()

    def entry(flags_a, flags_b):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return lib.lea_conv1x1_heads(p(x), x.stride(0), None, 0, 0, p(stacked), p(fa[0]), p(fa[1]), p(ya),
                                     ya.stride(0), 16, flags_a, p(fb[0]), p(fb[1]), p(yb), yb.stride(0), 8,
                                     flags_b, 1, 32, 2, 4, 8, _lib.LEA_F32, None)

    assert entry(_lib.LEA_RELU | _lib.LEA_RESIDUAL, _lib.LEA_RELU) == _lib.LEA_E_INVALID
    assert b"lea_conv1x1_heads" in lib.lea_last_error()
    assert entry(_lib.LEA_RELU, _lib.LEA_RESIDUAL) == _lib.LEA_E_INVALID
    assert entry(_lib.LEA_RELU, _lib.LEA_PAIR_SUM) == 1002


def test_probe_record():
    """bench.py --full and tools/layer_list.py see the launch: name, FLOPs, algorithmic bytes."""
    x, _, (wa, wb), (fa, fb) = _operands(1, 64, 0, 16, 8, (4, 6, 16), 3)
    stacked = kernels.pack_conv_weight(torch.cat((wa, wb), 0))
    with kernels.KernelProbe() as probe:
        kernels.conv1x1_heads(x, stacked, 16, *fa, True, 8, None, None, False)
    (rec,) = probe.records
    v = 4 * 6 * 16
    assert rec.name.startswith("conv1x1_heads_kernel<2, ")
    assert rec.flops == 2.0 * v * 24 * 64 and rec.bytes == 4 * v * (64 + 24) + 4.0 * 24 * 64
