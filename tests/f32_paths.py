"""The fp32 conv dispatch paths as a table: one row per kernel instantiation the planner or a
tuning hook can reach, with the entry that launches it on a tests/f32_judge.py case.  Shared by
tests/test_gpu_f32_numerics.py (error bars) and tests/test_gpu_dirty_memory.py (recycled memory).
Imports the library wrappers, so it lives beside f32_judge.py (which stays CPU-only)."""
import torch

from leastereo_amd import kernels

DEV = "cuda"


def _direct(j, split=0, **_):
    x, w = torch.from_numpy(j.x).to(DEV), torch.from_numpy(j.w).to(DEV)
    cout, k = w.shape[0], w.shape[-1]
    name = kernels.conv_kernel_name(x.shape[0], cout, *x.shape[2:], k)
    x1, x2 = (x[:, :split].contiguous(), x[:, split:].contiguous()) if split else (x, None)
    y = kernels.conv3d_bnrelu(x1, kernels.pack_conv_weight(w), cout, k, None, None, relu=False, x2=x2)
    return name, y


def _wino(j, pair=False, **_):
    x, w = torch.from_numpy(j.x).to(DEV), torch.from_numpy(j.w).to(DEV)
    cout, cin = w.shape[0], w.shape[1]
    packed = kernels.pack_conv_weight_wino(w)
    if pair:  # LEA_PAIR_SUM: always the F(2,3) x F(2,3) tile (csrc/conv3d_wino.hip:1023-1026)
        xa, xb = x[:, :cin // 2].contiguous(), x[:, cin // 2:].contiguous()
        out = torch.empty((x.shape[0], cout) + tuple(x.shape[2:]), device=DEV)
        assert kernels.pair_sum_supported(xa, xb, out)
        return "conv3d_wino22_kernel", kernels.conv3d_bnrelu_wino(xa, packed, cout, None, None, relu=False,
                                                                   out=out, x2=xb, pair_sum=True)
    name = kernels.wino_kernel_name(x.shape[0], cout, *x.shape[2:], cin=cin)
    return name, kernels.conv3d_bnrelu_wino(x, packed, cout, None, None, relu=False)


W44 = "lea_conv3d_wino44_set"
TILE = "lea_conv3d_wino_set_tile_override"
# id: (tuple of f32_judge.TUPLES, model, entry, settings, kernel name (exact, or a prefix ending
#      in "<" / ", "), the csrc line that states which algorithm the kernel computes, entry options)
PATHS = {
    # direct MFMA engine, k = 3: couts 16 / 32 / 64 (the last with two sources)
    "direct16": ("c16x16", "direct", _direct, (), "conv3d_dma_kernel<1, ", "conv3d.hip:603,743", {}),
    "direct32": ("c32x32", "direct", _direct, (), "conv3d_dma_kernel<2, ", "conv3d.hip:603,743", {}),
    "direct64_x2": ("c128x64", "direct", _direct, (), "conv3d_dma_kernel<4, ", "conv3d.hip:603,743", {"split": 64}),
    # small couts: the VALU engine (couts 1, 2) and the depth-paired MFMA tile (couts 3 .. 8)
    "valu1": ("c16x1", "direct", _direct, (), "conv3d_valu_kernel<1>", "conv3d.hip:587-588", {}),
    "valu2": ("c16x2", "direct", _direct, (), "conv3d_valu_kernel<2>", "conv3d.hip:587-588", {}),
    "direct5_dp": ("c16x5", "direct", _direct, (), "conv3d_dma_kernel<1, ", "conv3d.hip:594-595,746", {}),
    # 1x1x1, one float per lane and NT-float vectors
    "conv1x1_scalar": ("k1c128", "direct", _direct, (("lea_conv1x1_set_vector", (0,)),), "conv1x1_kernel<2, ",
                       "conv3d.hip:579-580", {}),
    "conv1x1_vector": ("k1c128", "direct", _direct, (("lea_conv1x1_set_vector", (1,)),), "conv1x1_kernel<2, ",
                       "conv3d.hip:579-580", {}),
    # 1-D Winograd along W: F(2,3), F(4,3) on 64-wide rows, F(4,3) on 32-wide row pairs (f = 8)
    "wino1d_f2": ("c32x32r", "wino21", _wino, ((TILE, (1, 2, 2)),), "conv3d_wino_kernel<2, 16, 2, 1, 2, false>",
                  "conv3d_wino.hip:9-11,877-878", {}),
    "wino1d_f4": ("c32x32r", "wino41", _wino, ((TILE, (1, 1, 4)),), "conv3d_wino_kernel<4, 16, 2, 1, 1, false>",
                  "conv3d_wino.hip:12-16,877-878", {}),
    "wino1d_f8": ("c32x32r", "wino41", _wino, ((TILE, (1, 2, 8)),), "conv3d_wino_kernel<4, 8, 2, 1, 2, false>",
                  "conv3d_wino.hip:12-16,877-878", {}),
    # depth-paired tile, couts <= 8: F(4,3) along W, direct along D (the F of the kernel name)
    "wino_dp8": ("c8x8w", "wino41", _wino, (), "conv3d_wino_kernel<4, 16, 0, 1, 2, false, true, true>",
                 "conv3d_wino.hip:881-882", {}),
    "wino_dp4": ("c8x4", "wino41", _wino, (), "conv3d_wino_kernel<4, 8, 0, 1, 2, false>",
                 "conv3d_wino.hip:881-882", {}),
    # F(4,3) along W x F(2,3) along D, the one-barrier pipeline
    "wino2p_32": ("c32x32", "wino42", _wino, ((W44, (0,)),), "conv3d_wino2p_kernel", "conv3d_wino2.hip:1-12", {}),
    "wino2p_96": ("c32x96", "wino42", _wino, ((W44, (0,)),), "conv3d_wino2p_kernel", "conv3d_wino2.hip:1-12", {}),
    # the per-lane W x D kernel (16 couts): 16-byte halo pieces (the default) and dword pieces
    "wino2_lane": ("c16x16", "wino42", _wino, (("lea_conv3d_wino_set_variant", (0,)),),
                   "conv3d_wino2_kernel<8, 1, 1, 4, 2, 5, false>", "conv3d_wino2.hip:1-12", {}),
    "wino2_lane_v2": ("c16x16r", "wino42", _wino, (("lea_conv3d_wino_set_variant", (2,)),),
                      "conv3d_wino2_kernel<8, 1, 1, 4, 2, 0, false>", "conv3d_wino2.hip:1-12", {}),
    # F(4,3) x F(4,3): modes 1 (couts 32 / 64), 2 (cin 8, cout 24), 3 (cout 16)
    "wino44_32": ("c32x32", "wino44", _wino, ((W44, (1,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    "wino44_64": ("c128x64", "wino44", _wino, ((W44, (1,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    "wino44_24": ("c8x24", "wino44", _wino, ((W44, (2,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    "wino44_16": ("c16x16", "wino44", _wino, ((W44, (3,)),), "conv3d_wino44_kernel", "conv3d_wino44.hip:1-9", {}),
    # F(2,3) x F(2,3): the 16-cout tile, and LEA_PAIR_SUM against the sum of two models
    "wino22_16": ("c16x16", "wino22", _wino, (("lea_conv3d_wino_set_w22", (1,)),), "conv3d_wino22_kernel",
                  "conv3d_wino22.hip:3", {}),
    "wino22_pair": ("p32x16", "pair22", _wino, (), "conv3d_wino22_kernel", "conv3d_wino22.hip:3,193-202",
                    {"pair": True}),
}
