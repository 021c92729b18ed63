"""Model arguments, field-compatible with config_utils/leastereo_args.py:4-40 and
config_utils/predict_args.py:4-28 (same names, defaults and argparse flags)."""
from __future__ import annotations

import argparse
import os
from dataclasses import dataclass

ARCH_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "architecture")


@dataclass
class LEAStereoArgsNoArch:
    fea_num_layers: int = 6
    mat_num_layers: int = 12
    fea_filter_multiplier: int = 8
    mat_filter_multiplier: int = 8
    fea_block_multiplier: int = 4
    mat_block_multiplier: int = 4
    fea_step: int = 3
    mat_step: int = 3


@dataclass
class LEAStereoArgs(LEAStereoArgsNoArch):
    net_arch_fea: str = None
    cell_arch_fea: str = None
    net_arch_mat: str = None
    cell_arch_mat: str = None
    maxdisp: int = 192
    cuda: bool = True


def default_arch_args(args: LEAStereoArgs) -> LEAStereoArgs:
    """Fill unset .npy paths with the SceneFlow search result shipped in data/
    (run/sceneflow/best/architecture/*.npy of the reference)."""
    for field, fname in (("net_arch_fea", "feature_network_path.npy"),
                         ("cell_arch_fea", "feature_genotype.npy"),
                         ("net_arch_mat", "matching_network_path.npy"),
                         ("cell_arch_mat", "matching_genotype.npy")):
        if getattr(args, field) is None:
            setattr(args, field, os.path.join(ARCH_DIR, fname))
    return args


def add_leastereo_args_without_arch(parser: argparse.ArgumentParser):
    for name, default in LEAStereoArgsNoArch().__dict__.items():
        parser.add_argument("--" + name, type=int, default=default)


def add_leastereo_args(parser: argparse.ArgumentParser):
    add_leastereo_args_without_arch(parser)
    for name in ("net_arch_fea", "cell_arch_fea", "net_arch_mat", "cell_arch_mat"):
        parser.add_argument("--" + name, default=None, type=str)


def obtain_predict_args(argv=None):
    """predict_args.py:4-28: same flags.  (--cuda keeps the reference's
    ``type=bool`` quirk: any non-empty string enables it.)"""
    parser = argparse.ArgumentParser(description="LEStereo Prediction (MI355X)")
    parser.add_argument("--crop_height", type=int, required=True, help="crop height")
    parser.add_argument("--crop_width", type=int, required=True, help="crop width")
    parser.add_argument("--maxdisp", type=int, default=192, help="max disp")
    parser.add_argument("--resume", type=str, default="", help="resume from saved model")
    parser.add_argument("--cuda", type=bool, default=False, help="use cuda?")
    parser.add_argument("--data_path", type=str, required=True, help="data root")
    parser.add_argument("--test_list", type=str, required=True, help="training list")
    parser.add_argument("--save_path", type=str, default="./result/", help="location to save result")
    for flag in ("sceneflow", "kitti2012", "kitti2015", "middlebury", "satellite", "mvs3d",
                 "new_tagil", "whu"):
        parser.add_argument("--" + flag, type=int, default=0)
    parser.add_argument("--precision", choices=("f32", "bf16"), default="f32",
                        help="matching-net arithmetic (bf16: configs 3/4; not in the reference)")
    parser.add_argument("--confidence", choices=("none", "entropy", "peak"), default="none",
                        help="also write a per-pixel confidence map in [0, 1]: 1 - entropy / ln(maxdisp) "
                             "of the disparity distribution, or the probability mass within "
                             "--conf_radius of its winner (not in the reference)")
    parser.add_argument("--conf_radius", type=int, default=4,
                        help="window radius in disparities for --confidence=peak (1..16)")
    parser.add_argument("--lr_check", type=float, default=0.0, metavar="THR",
                        help="left-right check with this threshold in pixels (0 = off): also write the "
                             "right-view disparity, the occlusion mask and the filled disparity "
                             "(not in the reference)")
    parser.add_argument("--photo_check", action="store_true",
                        help="photometric consistency of the prediction with its image pair: also write "
                             "the right image warped to the left view and the per-pixel SSIM + L1 error, "
                             "and print its mean; with --lr_check the flagged pixels take no part "
                             "(not in the reference)")
    parser.add_argument("--scene", type=int, default=0,
                        help="1: whole-scene inference -- --crop_height/--crop_width name the tile, an image "
                             "larger than it is cut into overlapping tiles, gathered and blended on the "
                             "device, and every output has the image's size (not in the reference)")
    parser.add_argument("--scene_batch", type=int, default=1, help="tiles per forward under --scene")
    parser.add_argument("--scene_context", type=int, default=16,
                        help="pixels of context dropped on every cut side of a tile under --scene")
    parser.add_argument("--scene_ramp", type=int, default=32,
                        help="width of the blend ramp between tiles under --scene (1..256)")
    parser.add_argument("--refine", type=int, default=0,
                        help="1: confidence-weighted edge-preserving refinement of the disparity (the fast "
                             "global smoother; guide the left image, confidence the peak mass, the pixels the "
                             "left-right check flags excluded): also write {index}_refined.npy/.png and "
                             "{index}_support.png; implies the confidence and left-right heads it needs "
                             "(not in the reference)")
    parser.add_argument("--refine_lambda", type=float, default=8000.0,
                        help="smoothness weight of --refine (OpenCV's default; untuned)")
    parser.add_argument("--refine_sigma", type=float, default=0.05,
                        help="edge sensitivity of --refine in units of the standardised image (untuned)")
    parser.add_argument("--refine_iters", type=int, default=3, help="iterations of --refine (1..8)")
    parser.add_argument("--speckle", type=int, default=0, metavar="SIZE",
                        help="speckle filter (0 = off): remove the connected components of the disparity of at "
                             "most SIZE pixels (OpenCV's filterSpeckles; 50-200 is its recommended window, "
                             "untuned here): also write {index}_speckle.png and {index}_despeckled.npy; with "
                             "--lr_check the flagged pixels are walls, with --refine 1 the refinement fills the "
                             "removed pixels (not in the reference)")
    parser.add_argument("--speckle_diff", type=float, default=1.0, metavar="D",
                        help="largest disparity step in pixels between connected neighbours under --speckle "
                             "(OpenCV's speckleRange, 1-2 recommended; untuned)")
    parser.add_argument("--pointcloud", type=int, default=0,
                        help="1: also write {index}.ply, the point cloud of the best map the other flags made "
                             "(the refined map under --refine, else the disparity without the pixels --speckle "
                             "and --lr_check flag), coloured from the left image; needs --pc_focal and "
                             "--pc_baseline (not in the reference)")
    parser.add_argument("--pc_focal", type=float, default=0.0, metavar="PX",
                        help="focal length of the rectified pair in pixels under --pointcloud")
    parser.add_argument("--pc_baseline", type=float, default=0.0, metavar="M",
                        help="baseline of the pair under --pointcloud; its unit is the cloud's")
    parser.add_argument("--pc_cx", type=float, default=None, metavar="X",
                        help="principal point of the left image under --pointcloud (default: the image's centre)")
    parser.add_argument("--pc_cy", type=float, default=None, metavar="Y", help="see --pc_cx")
    parser.add_argument("--pc_max_depth", type=float, default=0.0, metavar="M",
                        help="drop the points farther than this under --pointcloud (0 = keep all): the "
                             "disparities at or below focal * baseline / M")
    parser.add_argument("--pc_normals", type=int, default=0,
                        help="1: also write the normals of the points under --pointcloud")
    parser.add_argument("--calib", type=str, default="", metavar="FILE",
                        help="a stereo calibration (.json or .npz with K1, D1, K2, D2, R, T, size, model: "
                             "rectify.load_calibration): every decoded pair is undistorted and rectified on the "
                             "device before anything else, and --pointcloud takes focal, baseline and principal "
                             "point from the rectification (the --pc_focal/--pc_baseline/--pc_cx/--pc_cy flags are "
                             "then refused) (not in the reference)")
    parser.add_argument("--rect_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                        help="size of the rectified images under --calib (default: the raw images')")
    parser.add_argument("--rect_fill", type=int, default=0, metavar="V",
                        help="grey level 0..255 of the rectified pixels that have no source under --calib; the "
                             "standardisation statistics include this border")
    parser.add_argument("--save_rectified", type=int, default=0,
                        help="1: also write {index}_rect_left.png, {index}_rect_right.png and "
                             "{index}_rect_valid.png under --calib")
    parser.add_argument("--novel_view", type=float, default=None, metavar="S",
                        help="also write {index}_view.png and {index}_view_holes.png: the left image warped forward "
                             "to baseline fraction S (0 = the left camera, 1 = the right one, beyond either is "
                             "legal) through the best map the other flags made (the refined map under --refine, "
                             "else the filled one under --lr_check, else the disparity without the pixels "
                             "--speckle flags); at S = 1 also print the mean absolute difference to the real "
                             "right image (not in the reference)")
    parser.add_argument("--view_fill", type=int, default=1, choices=(0, 1),
                        help="1: the holes of --novel_view take the background beside them, 0: they stay black")
    parser.add_argument("--dsm", type=int, default=0,
                        help="1: also write {index}_dsm.npy (float32 heights, NaN = nodata), {index}_dsm.png, "
                             "{index}_ortho.png, {index}_dsm_state.png and {index}_dsm.json: the digital surface "
                             "model and orthophoto of the map --pointcloud would take, on a ground grid under a "
                             "camera looking straight down; needs --pc_focal and --pc_baseline, or --calib (not in "
                             "the reference)")
    parser.add_argument("--dsm_cell", type=float, default=0.0, metavar="C",
                        help="cell size of --dsm in the baseline's unit (0 = the ground sample distance at the "
                             "farthest point)")
    parser.add_argument("--dsm_radius", type=float, default=0.5, metavar="R",
                        help="footprint radius of a point under --dsm, in cells, 0 .. 2")
    parser.add_argument("--dsm_fill", type=int, default=0, metavar="T",
                        help="fill passes of --dsm: an empty cell with three or more measured neighbours takes the "
                             "lowest of them")
    add_leastereo_args(parser)
    return parser.parse_args(argv)
