"""predict.py of the reference, on the MI355X model (config 1 plumbing).

Restates the host-side steps around ``LEAStereo.forward`` (predict.py:144-243):
  * ``load_images``    predict.py:163-169  PIL decode (uint8, stays uint8)
  * ``load_transform`` predict.py:144-184  load_data's per-channel standardisation
                       (whole-image float64 statistics, stored float32) fused with
                       test_transform's pad/centre-crop, on the device
                       (``lea_standardize_crop_u8``; numpy checker: oracle/predict_ref.py)
  * ``crop_output``    predict.py:236-239  undo the padding on the disparity
  * ``read_pfm``       dataloaders/datasets/common.py:8-40
  * ``plot_disparity`` predict.py:246-247  turbo-coloured PNG, vmin 0, vmax 192
  * ``save_float_png`` / ``crop_image``  predict.py:128-141,207-211  the satellite
                       branch's skimage.io.imsave of float arrays (imageio's min-max
                       8-bit conversion, restated: skimage / imageio are absent here)
  * ``main``           predict.py:249-286  the list-file loop: --sceneflow writes
                       {index}.png and {index}_gt.png (and {index}.npy, the raw
                       disparity), --satellite writes {name}.png and {name}_in.png
  * ``predict_pair_lr`` / ``save_lr``  not in the reference: --lr_check THR adds the
                       left-right check of ``LEAStereo.forward_lr`` ({index}_right.npy,
                       {index}_occ.png, {index}_filled.npy / .png; {name}_occ.png)
  * ``photometric_check`` / ``save_photo``  not in the reference: --photo_check warps the right
                       image to the left view with the prediction and scores it against
                       the left image ({index}_warped.png, {index}_photo.npy / .png, the
                       pair's mean error printed); with --lr_check the flagged pixels are
                       excluded
  * ``predict_scene``  not in the reference: --scene 1 makes --crop_height/--crop_width the
                       tile of ``scene.SceneRunner``; an image larger than it is cut into
                       overlapping tiles, gathered and blended on the device, and every output
                       above has the image's size under its usual name
  * ``predict_pair_refined`` / ``predict_scene_refined`` / ``save_refined``  not in the reference:
                       --refine 1 adds the confidence-weighted edge-preserving refinement of
                       ``LEAStereo.forward_refined`` ({index}_refined.npy / .png, {index}_support.png);
                       under --scene it runs once on the blended scene (``scene.refine_scene``)
  * ``despeckle`` / ``save_speckle``  not in the reference: --speckle SIZE [--speckle_diff D]
                       adds the speckle filter of ``kernels.speckle_filter`` on the written
                       disparity ({index}_speckle.png, {index}_despeckled.npy; the flags of
                       --lr_check are its walls), and feeds --refine 1 the removed pixels
  * ``pointcloud_options`` / ``map_origin`` / ``pointcloud_of_map`` / ``save_pointcloud``  not in the
                       reference: --pointcloud 1 --pc_focal PX --pc_baseline M [--pc_cx X --pc_cy Y
                       --pc_max_depth M --pc_normals 1] reprojects the best map the other flags
                       made (``kernels.reproject``: the refined map under --refine, else the
                       disparity without the pixels --speckle and --lr_check flag) and writes
                       {index}.ply, coloured from the decoded left image; the calibration is the
                       source image's, whatever the crop
  * ``rectify_options`` / ``set_rectifier`` / ``load_pair`` / ``save_rectified``  not in the reference:
                       --calib FILE [--rect_size H W --rect_fill V --save_rectified 1] rectifies every
                       decoded pair on the device (``rectify.Rectifier``, ``kernels.rectify_u8``)
                       before the transform or the scene path; --pointcloud 1 then takes focal,
                       baseline and principal point from the rectification and leaves out the left
                       pixels that have no source
  * ``dsm_options`` / ``dsm_of_map`` / ``save_dsm``  not in the reference: --dsm 1 [--dsm_cell C
                       --dsm_radius R --dsm_fill T] rasterises the cloud of the map --pointcloud
                       would take into a z-buffered ground grid on the device (``dsm.Surface``)
                       and writes {index}_dsm.npy / _dsm.png / _ortho.png / _dsm_state.png /
                       _dsm.json; needs the calibration --pointcloud needs.
  * ``novel_view_options`` / ``novel_view_of_map`` / ``save_view``  not in the reference: --novel_view S
                       [--view_fill 0|1] warps the decoded left image forward to baseline fraction S
                       (``kernels.forward_warp``) through the best map the other flags made -- the
                       refined map under --refine, else the filled one under --lr_check, else the
                       disparity; the pixels --lr_check and --speckle flag carry no surface -- and
                       writes {index}_view.png and {index}_view_holes.png; at S = 1 the mean absolute
                       difference to the real right image is printed
Arithmetic runs on the HIP kernels; what stays on the host is file I/O (PIL, PFM, PNG).

    python predict.py --sceneflow=1 --maxdisp=192 --crop_height=576 --crop_width=960 \
        --data_path=./dataset/SceneFlow/ --test_list=./lists/sceneflow_test.list \
        --save_path=./predict/ [--resume ckpt.pth] [arch flags as the reference]
"""
from __future__ import annotations

import os
import re
import sys
import time

import numpy as np
import torch


def read_pfm(path):
    """dataloaders/datasets/common.py:8-40: (image [H, W] float, height, width)."""
    with open(path, "rb") as f:
        kind = f.readline().decode("latin-1")
        if "PF" in kind:
            channels = 3
        elif "Pf" in kind:
            channels = 1
        else:
            raise ValueError(f"{path}: not a PFM file")
        width, height = (int(v) for v in re.findall(r"\d+", f.readline().decode("latin-1")))
        little = "-" in f.readline().decode("latin-1")
        data = np.frombuffer(f.read(width * height * channels * 4),
                             dtype="<f4" if little else ">f4").astype(np.float64)
    if channels != 1:
        raise ValueError(f"{path}: {channels}-channel PFM (the reference reshapes to [H, W])")
    return np.flipud(data.reshape(height, width)), height, width


def load_images(leftname, rightname):
    """The PIL decode of predict.py:163-169: two uint8 [H, W, 3|4] arrays."""
    from PIL import Image
    left = np.asarray(Image.open(leftname))
    right = np.asarray(Image.open(rightname))
    if left.shape != right.shape or left.ndim != 3 or left.dtype != np.uint8:
        raise ValueError(f"{leftname}, {rightname}: need two 8-bit colour images of one size, "
                         f"got {left.shape} {left.dtype} and {right.shape} {right.dtype}")
    return left, right


_rectifier = None      # set_rectifier: the rectify.Rectifier of --calib, None without the flag
_rectified_last = None  # the RectifiedPair of the last load_pair under --calib


def set_rectifier(rectifier):
    """Install (or, with None, remove) the ``rectify.Rectifier`` that ``load_pair`` applies."""
    global _rectifier, _rectified_last
    _rectifier, _rectified_last = rectifier, None


def load_pair(leftname, rightname):
    """``load_images``; under --calib the pair rectified on the device: two uint8 device
    tensors [Ho, Wo, 3|4] (``last_rectified`` keeps the whole ``RectifiedPair``)."""
    global _rectified_last
    left, right = load_images(leftname, rightname)
    if _rectifier is None:
        return left, right
    _rectified_last = _rectifier(left, right)
    return _rectified_last.left, _rectified_last.right


def last_rectified():
    """The ``kernels.RectifiedPair`` of the last ``load_pair`` under --calib, else None."""
    return _rectified_last


def _device_u8(a, device):
    """A decoded image (numpy) or a rectified one (device tensor) as a device tensor."""
    if isinstance(a, torch.Tensor):
        return a.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device, non_blocking=True)


def load_transform(left_u8, right_u8, crop_height, crop_width, device="cuda"):
    """load_data (predict.py:162-184) + test_transform (:144-159) on the device:
    the uint8 images go up as they were decoded (a quarter of the float32 bytes)
    and ``lea_standardize_crop_u8`` standardises with whole-image statistics and
    pads or crops in one pass.  Returns (left, right [1, 3, ch, cw], h, w)."""
    from . import kernels
    h, w = left_u8.shape[:2]
    lt, rt = _device_u8(left_u8, device), _device_u8(right_u8, device)
    left, right = kernels.standardize_crop_u8(lt, rt, crop_height, crop_width)
    return left, right, h, w


def crop_output(pred: np.ndarray, height: int, width: int, crop_height: int, crop_width: int):
    """predict.py:236-239 (the reference's ``or``: a crop on either axis triggers it)."""
    if height <= crop_height or width <= crop_width:
        return pred[0, crop_height - height: crop_height, crop_width - width: crop_width]
    return pred[0]


def predict_pair(model, leftname, rightname, crop_height, crop_width, device="cuda", confidence="none",
                 radius=4):
    """test() of predict.py:213-243 without the plotting: disparity [h', w'] numpy.
    ``confidence`` "entropy" or "peak" (not in the reference): returns (disparity, conf, local)
    instead -- conf in [0, 1], ``DisparityStats.confidence`` or the peak mass within ``radius``
    of the winner; local the winner-window disparity under "peak", else None -- from
    ``model.forward_with_confidence``, each cropped like the disparity."""
    left, right, h, w = load_transform(*load_pair(leftname, rightname), crop_height, crop_width,
                                       device)
    if confidence in (None, "none"):
        with torch.no_grad():
            pred = model(left, right)
        return crop_output(pred.cpu().numpy(), h, w, crop_height, crop_width)
    if confidence not in ("entropy", "peak"):
        raise ValueError(f"confidence {confidence!r}: one of none, entropy, peak")
    with torch.no_grad():
        st = model.forward_with_confidence(left, right, radius)
    conf = st.confidence if confidence == "entropy" else st.peak
    disp, conf, local = (crop_output(t.cpu().numpy(), h, w, crop_height, crop_width)
                         for t in (st.disp, conf, st.disp_local))
    return disp, conf, (local if confidence == "peak" else None)


def save_confidence(prefix, conf, local=None):
    """<prefix>_conf.npy (float32) and <prefix>_conf.png (8-bit, values in [0, 1] scale by 255);
    <prefix>_local.npy when the winner-window disparity came with it (--confidence=peak)."""
    np.save(prefix + "_conf.npy", conf.astype(np.float32))
    save_float_png(prefix + "_conf.png", np.clip(conf, 0.0, 1.0))
    if local is not None:
        np.save(prefix + "_local.npy", local.astype(np.float32))


def predict_pair_lr(model, leftname, rightname, crop_height, crop_width, threshold, device="cuda"):
    """``predict_pair`` through ``model.forward_lr``: (disparity, right-view disparity, state
    uint8, filled disparity), each cropped like the disparity.  The disparity is
    ``predict_pair``'s bit for bit."""
    left, right, h, w = load_transform(*load_pair(leftname, rightname), crop_height, crop_width,
                                       device)
    with torch.no_grad():
        lr = model.forward_lr(left, right, threshold)
    return tuple(crop_output(t.cpu().numpy(), h, w, crop_height, crop_width) for t in lr)


def predict_scene(runner, leftname, rightname, confidence="none"):
    """One pair through ``scene.SceneRunner`` (--scene): (disp, lr) at the image's size, shaped
    as ``predict_pair`` and ``predict_pair_lr`` shape them -- disp the disparity, or (disparity,
    conf, local) under ``confidence``; lr (disparity, right-view disparity, state, filled) when
    the runner has an ``lr_threshold``, else None."""
    return _scene_maps(runner(*load_pair(leftname, rightname)), runner.model.maxdisp, confidence)


def _scene_maps(res, maxdisp, confidence):
    """A ``SceneResult`` as ``predict_scene`` returns it."""
    import math
    disp = res.disp.cpu().numpy()
    lr = None
    if res.disp_right is not None:
        lr = (disp,) + tuple(t.cpu().numpy() for t in (res.disp_right, res.state, res.disp_filled))
    if confidence in (None, "none"):
        return disp, lr
    if confidence not in ("entropy", "peak"):
        raise ValueError(f"confidence {confidence!r}: one of none, entropy, peak")
    if confidence == "entropy":  # DisparityStats.confidence on the blended entropy
        return (disp, (1.0 - res.entropy / math.log(maxdisp)).cpu().numpy(), None), lr
    return (disp, res.peak.cpu().numpy(), res.disp_local.cpu().numpy()), lr


def predict_pair_refined(model, leftname, rightname, crop_height, crop_width, lam, sigma, iterations, radius=4,
                         lr_threshold=1.0, device="cuda", speckle=None):
    """``predict_pair`` through ``model.forward_refined``: (disparity, refined disparity,
    support), each cropped like the disparity.  The disparity is ``predict_pair``'s bit for bit.
    ``speckle``: the dict of ``forward_refined`` (None: the call as it is without it)."""
    left, right, h, w = load_transform(*load_pair(leftname, rightname), crop_height, crop_width,
                                       device)
    kw = {} if speckle is None else {"speckle": speckle}
    with torch.no_grad():
        out = model.forward_refined(left, right, lam=lam, sigma=sigma, iterations=iterations, radius=radius,
                                    lr_threshold=lr_threshold, **kw)
    return tuple(crop_output(t.cpu().numpy(), h, w, crop_height, crop_width)
                 for t in (out.disp, out.disp_refined, out.support))


def predict_scene_refined(runner, leftname, rightname, lam, sigma, iterations, confidence="none", speckle=None):
    """``predict_scene`` plus the refinement of the blended scene (``scene.refine_scene``: once,
    at the image's size, never per tile): (disp, lr, (refined, support)), the first two as
    ``predict_scene`` returns them.  The runner should blend the peak mass and run the
    left-right check (``confidence=True``, an ``lr_threshold``): they are the refinement's
    confidence and exclusion.  ``speckle``: the dict of ``refine_scene`` (None: the call as it
    is without it)."""
    from .scene import refine_scene
    left, right = load_pair(leftname, rightname)
    res = runner(left, right)
    kw = {} if speckle is None else {"speckle": speckle}
    refined, support = refine_scene(res, left, lam, sigma, iterations, return_support=True, **kw)
    disp, lr = _scene_maps(res, runner.model.maxdisp, confidence)
    return disp, lr, (refined.cpu().numpy(), support.cpu().numpy())


def refine_pair(model, runner, leftname, rightname, opt):
    """--refine on one pair: through the scene runner when there is one (--scene), else one
    ``forward_refined`` on the crop.  Returns (disp, lr, (refined, support)); disp and lr are
    None without a runner (the pair's other outputs then come from their own calls)."""
    kw = {} if speckle_options(opt) is None else {"speckle": speckle_options(opt)}
    if runner is not None:
        return predict_scene_refined(runner, leftname, rightname, opt.refine_lambda, opt.refine_sigma,
                                     opt.refine_iters, opt.confidence, **kw)
    out = predict_pair_refined(model, leftname, rightname, opt.crop_height, opt.crop_width, opt.refine_lambda,
                               opt.refine_sigma, opt.refine_iters, opt.conf_radius,
                               opt.lr_check if opt.lr_check > 0 else 1.0, **kw)
    return None, None, out[1:]


def speckle_options(opt):
    """--speckle SIZE [--speckle_diff D] as the ``speckle`` dict of ``forward_refined`` /
    ``refine_scene``; None when the filter is off (SIZE 0).  Refuses a negative SIZE and a D that
    is negative or not finite."""
    size, diff = getattr(opt, "speckle", 0), getattr(opt, "speckle_diff", 1.0)
    if size < 0 or size > 2 ** 31 - 1:
        raise ValueError(f"--speckle {size}: a component size in pixels > 0, or 0 for off")
    if not 0 <= diff < float("inf"):
        raise ValueError(f"--speckle_diff {diff}: a finite disparity step in pixels >= 0")
    if not size:
        return None
    if getattr(opt, "satellite", 0):
        raise NotImplementedError("--speckle writes its maps beside the --sceneflow outputs only")
    return dict(max_size=int(size), max_diff=float(diff))


def despeckle(disp, state, max_size, max_diff, device="cuda"):
    """``kernels.speckle_filter`` of a written disparity map [H, W] (numpy; under --scene the
    blended scene, never a tile: a component cut by a tile's edge looks small), with the
    left-right check's ``state`` as walls when there is one: (removed, despeckled), the pixels
    the filter removed (bool) and the disparity with 0 on every flagged pixel."""
    from . import kernels
    d = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32)).to(device)
    e = None if state is None else torch.from_numpy(np.ascontiguousarray(state, dtype=np.uint8)).to(device)
    out = kernels.speckle_filter(d, e, max_size, max_diff, want_size=False)
    return (out.state == kernels.LR_SPECKLE).cpu().numpy(), out.filtered.cpu().numpy()


def save_speckle(prefix, removed, despeckled):
    """<prefix>_speckle.png (8-bit: 255 on the removed pixels) and <prefix>_despeckled.npy (float32)."""
    save_float_png(prefix + "_speckle.png", np.where(removed, 255, 0).astype(np.uint8))
    np.save(prefix + "_despeckled.npy", despeckled.astype(np.float32))


def pointcloud_options(opt):
    """--pointcloud 1 --pc_focal PX --pc_baseline M [--pc_cx X --pc_cy Y --pc_max_depth M
    --pc_normals 1] as a dict (focal, baseline, cx, cy, max_depth, normals; cx / cy None for the
    image's centre); None when the flag is off.  Refuses a focal length or baseline that is not a
    finite number > 0, a negative or NaN depth limit, and --satellite."""
    if not getattr(opt, "pointcloud", 0):
        return None
    focal, baseline, depth = opt.pc_focal, opt.pc_baseline, opt.pc_max_depth
    if getattr(opt, "calib", ""):  # the rectification is the calibration: main fills focal .. cx_right from it
        given = [f"--{n}" for n in ("pc_focal", "pc_baseline") if getattr(opt, n)]
        given += [f"--{n}" for n in ("pc_cx", "pc_cy") if getattr(opt, n) is not None]
        if given:
            raise ValueError(f"{', '.join(given)} with --calib: the point cloud takes focal, baseline and principal "
                             f"point from the rectification, a second calibration would contradict it")
        if not depth >= 0:
            raise ValueError(f"--pc_max_depth {depth}: a depth > 0 in the baseline's unit, or 0 for no limit")
        if getattr(opt, "satellite", 0):
            raise NotImplementedError("--pointcloud writes its file beside the --sceneflow outputs only")
        return dict(focal=None, baseline=None, cx=None, cy=None, max_depth=float(depth), normals=bool(opt.pc_normals))
    if not (0 < focal < float("inf") and 0 < baseline < float("inf")):
        raise ValueError(f"--pointcloud needs --pc_focal {focal} (pixels) and --pc_baseline {baseline} as finite "
                         f"numbers > 0")
    if not depth >= 0:
        raise ValueError(f"--pc_max_depth {depth}: a depth > 0 in the baseline's unit, or 0 for no limit")
    for name in ("pc_cx", "pc_cy"):
        v = getattr(opt, name)
        if v is not None and not abs(v) < float("inf"):
            raise ValueError(f"--{name} {v}: a finite pixel coordinate")
    if getattr(opt, "satellite", 0):
        raise NotImplementedError("--pointcloud writes its file beside the --sceneflow outputs only")
    return dict(focal=float(focal), baseline=float(baseline), cx=opt.pc_cx, cy=opt.pc_cy, max_depth=float(depth),
                normals=bool(opt.pc_normals))


def map_origin(height: int, width: int, map_height: int, map_width: int):
    """(x0, y0): where pixel (0, 0) of a written map of ``map_height`` x ``map_width`` lies in
    its ``height`` x ``width`` source image -- the centre crop that ``crop_output`` leaves of an
    image larger than the crop and that ``main`` cuts out of the ground truth; (0, 0) for a map
    of the image's own size (an image that fits the crop, and every map under --scene)."""
    return max(int((width - map_width) / 2), 0), max(int((height - map_height) / 2), 0)


def rectify_options(opt):
    """--calib FILE [--rect_size H W --rect_fill V --save_rectified 1] as a dict (path, size,
    fill, save); None without --calib (the other three are then not looked at).  Refuses a fill
    outside 0 .. 255, a size below 1 and --satellite."""
    if not getattr(opt, "calib", ""):
        return None
    size = getattr(opt, "rect_size", None)
    if size is not None and (len(size) != 2 or min(size) < 1):
        raise ValueError(f"--rect_size {size}: a height and a width >= 1")
    if not 0 <= opt.rect_fill <= 255:
        raise ValueError(f"--rect_fill {opt.rect_fill}: a grey level in 0 .. 255")
    if getattr(opt, "satellite", 0):
        raise NotImplementedError("--calib rectifies the pairs of the --sceneflow list only")
    return dict(path=opt.calib, size=None if size is None else (int(size[0]), int(size[1])), fill=int(opt.rect_fill),
                save=bool(opt.save_rectified))


def make_rectifier(path, size=None, fill=0, device="cuda", **_):
    """The ``rectify.Rectifier`` of a calibration file (``rectify.load_calibration``), with
    ``size`` (height, width) as the rectified images' size (None: the raw images')."""
    from . import rectify
    cam_l, cam_r, R, T, raw = rectify.load_calibration(path)
    return rectify.Rectifier(rectify.stereo_rectify(cam_l, cam_r, R, T, raw, out_size=size), device, fill=fill)


def save_rectified(prefix, pair):
    """<prefix>_rect_left.png, <prefix>_rect_right.png (the rectified images as they go on) and
    <prefix>_rect_valid.png (8-bit: 255 where the left pixel has a source in the raw image)."""
    from PIL import Image
    Image.fromarray(pair.left.cpu().numpy()).save(prefix + "_rect_left.png")
    Image.fromarray(pair.right.cpu().numpy()).save(prefix + "_rect_right.png")
    v = pair.valid.cpu().numpy()
    Image.fromarray((v[0] * 255).astype(np.uint8)).save(prefix + "_rect_valid.png")


def pointcloud_of_map(disp, exclude, left_u8, focal, baseline, cx=None, cy=None, max_depth=0.0, normals=False,
                      device="cuda", cx_right=None, valid=None):
    """``kernels.reproject`` of a written map [h', w'] (numpy: the disparity or the refined
    disparity, at the crop's or the scene's size) with the source image's calibration:
    ``left_u8`` is the decoded left image the map was cut from, (``cx``, ``cy``) its principal
    point (None: its centre), the map's origin in it is ``map_origin``'s.  ``exclude`` [h', w']
    or None: non-zero pixels give no point.  ``max_depth`` > 0 becomes the disparity bound
    min_disp = focal * baseline / max_depth here, so that validity stays a test on the
    disparity.  Under --calib ``left_u8`` is the rectified left image (a device tensor),
    ``cx_right`` the right view's principal point and ``valid`` [h, w] its validity map: pixels
    without a source give no point.  Returns ``kernels.HostPointCloud`` (count, xyz, rgb, index,
    normals)."""
    return _cloud_of_map(disp, exclude, left_u8, focal, baseline, cx, cy, max_depth, normals, device, cx_right,
                         valid)[0].to_host()


def _cloud_of_map(disp, exclude, left_u8, focal, baseline, cx, cy, max_depth, normals, device, cx_right, valid):
    """The device ``kernels.PointCloud`` of ``pointcloud_of_map``, its float64 Q, and the excluded
    pixels as a host bool map (None without any)."""
    from . import kernels
    from .pointcloud import q_matrix
    h, w = left_u8.shape[:2]
    mh, mw = disp.shape
    x0, y0 = map_origin(h, w, mh, mw)
    Q = q_matrix(focal, baseline, w / 2 if cx is None else cx, h / 2 if cy is None else cy, cx_right, origin=(x0, y0))
    d = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32)).to(device)
    e = None if exclude is None else torch.from_numpy(np.ascontiguousarray(exclude != 0).view(np.uint8)).to(device)
    if valid is not None:
        border = (_device_u8(valid, device)[y0:y0 + mh, x0:x0 + mw] == 0).to(torch.uint8)
        e = border if e is None else torch.maximum(e, border)
    img = _device_u8(left_u8[y0:y0 + mh, x0:x0 + mw], device)
    cloud = kernels.reproject(d, Q, img, e, min_disp=focal * baseline / max_depth if max_depth > 0 else 0.0,
                              normals=normals)
    return cloud, Q, e


def dsm_options(opt):
    """--dsm 1 [--dsm_cell C --dsm_radius R --dsm_fill T] as a dict (calib: the dict of
    ``pointcloud_options``, cell: None for the ground sample distance at the far disparity,
    radius, fill); None when the flag is off (the other three are then not looked at).  Needs
    the calibration --pointcloud needs (--pc_focal and --pc_baseline, or --calib) and refuses a
    cell that is not a finite number >= 0, a radius outside 0 .. 2, a fill count outside
    0 .. 1024 and --satellite."""
    import argparse
    if not getattr(opt, "dsm", 0):
        return None
    from .dsm import MAX_FILL, MAX_RADIUS
    if getattr(opt, "satellite", 0):
        raise NotImplementedError("--dsm writes its files beside the --sceneflow outputs only")
    try:
        calib = pointcloud_options(argparse.Namespace(**dict(vars(opt), pointcloud=1)))
    except ValueError as e:
        raise ValueError(f"--dsm needs the calibration of --pointcloud: {e}") from None
    if not 0 <= opt.dsm_cell < float("inf"):
        raise ValueError(f"--dsm_cell {opt.dsm_cell}: a cell size > 0 in the baseline's unit, or 0 for the ground "
                         f"sample distance at the farthest point")
    if not 0 <= opt.dsm_radius <= MAX_RADIUS:
        raise ValueError(f"--dsm_radius {opt.dsm_radius}: a footprint radius in cells, 0 .. {MAX_RADIUS}")
    if not 0 <= opt.dsm_fill <= MAX_FILL:
        raise ValueError(f"--dsm_fill {opt.dsm_fill}: a number of fill passes, 0 .. {MAX_FILL}")
    return dict(calib=calib, cell=float(opt.dsm_cell) or None, radius=float(opt.dsm_radius), fill=int(opt.dsm_fill))


DSM_MAX_CELLS = 1 << 28  # of the grid --dsm makes for one pair


def dsm_of_map(disp, exclude, left_u8, calib, cell=None, radius=0.5, fill=0, device="cuda", cx_right=None,
               valid=None):
    """The surface model of a written map: ``pointcloud_of_map``'s cloud, kept on the device, on
    the bounding grid (``dsm.grid_from_view``) of the view between the smallest and the largest
    disparity that gives a point (the smallest is focal * baseline / max_depth with a depth
    limit), the camera looking straight down: height = -Z, in the baseline's unit.  ``calib`` is
    the dict of ``pointcloud_options`` with focal and baseline filled in.  Returns (height
    [GH, GW] float32, NaN for nodata; ortho [GH, GW, 3] uint8; state [GH, GW] uint8; meta: G,
    cell, origin, size) as numpy arrays and a dict."""
    from . import dsm
    focal, baseline, max_depth = calib["focal"], calib["baseline"], calib["max_depth"]
    cloud, Q, e = _cloud_of_map(disp, exclude, left_u8, focal, baseline, calib["cx"], calib["cy"], max_depth, False,
                                device, cx_right, valid)
    d = np.asarray(disp, dtype=np.float32)
    lo = focal * baseline / max_depth if max_depth > 0 else 0.0
    ok = np.isfinite(d) & (d > lo)
    if e is not None:
        ok &= e.cpu().numpy() == 0
    if not ok.any():
        raise ValueError("--dsm: no pixel of the map gives a point")
    far, near = float(d[ok].min()), float(d[ok].max())
    if far == near:
        near = far * 2.0
    mh, mw = d.shape
    G, gh, gw = dsm.grid_from_view(Q, mh, mw, (far, near), cell)
    if gh * gw > DSM_MAX_CELLS:
        raise ValueError(f"--dsm: the grid would be {gh} x {gw} cells; give a larger --dsm_cell or a --pc_max_depth")
    surface = dsm.Surface(gh, gw, device)
    maps = surface.add_cloud(cloud, G, radius=radius).resolve(fill_iterations=fill)
    size = 1.0 / float(G[0, 0])
    meta = dict(G=[[float(v) for v in row] for row in G], cell=size,
                origin=[-float(G[0, 3]) * size, -float(G[1, 3]) * size, 0.0], size=[gh, gw])
    return maps.height.cpu().numpy(), maps.rgb.cpu().numpy(), maps.state.cpu().numpy(), meta


def save_dsm(prefix, height, ortho, state, meta):
    """<prefix>_dsm.npy (float32, NaN for nodata), <prefix>_dsm.png (the heights min-max 8-bit,
    nodata black), <prefix>_ortho.png, <prefix>_dsm_state.png (8-bit: measured 0, filled 127,
    empty 255) and <prefix>_dsm.json (G, cell, origin, size)."""
    import json

    from PIL import Image
    np.save(prefix + "_dsm.npy", height.astype(np.float32))
    seen = np.isfinite(height)
    grey = np.zeros(height.shape, np.float64)
    if seen.any():
        lo, hi = float(height[seen].min()), float(height[seen].max())
        grey[seen] = (height[seen] - lo) / (hi - lo) if hi > lo else 1.0
    save_float_png(prefix + "_dsm.png", grey)
    Image.fromarray(ortho).save(prefix + "_ortho.png")
    save_float_png(prefix + "_dsm_state.png", occlusion_u8(state))
    with open(prefix + "_dsm.json", "w") as f:
        json.dump(meta, f, indent=1)


def save_pointcloud(prefix, cloud):
    """<prefix>.ply (binary little-endian: x y z, the normals when the cloud has them, red green blue)."""
    from .pointcloud import write_ply
    return write_ply(prefix + ".ply", cloud.xyz, cloud.rgb, cloud.normals)


def novel_view_options(opt):
    """--novel_view S [--view_fill 0|1] as a dict (s, fill); None without the flag.  Refuses an S
    that is not finite, a fill that is neither 0 nor 1, and --satellite."""
    s = getattr(opt, "novel_view", None)
    if s is None:
        return None
    if not abs(s) < float("inf"):
        raise ValueError(f"--novel_view {s}: a finite baseline fraction (0 = the left camera, 1 = the right one)")
    fill = getattr(opt, "view_fill", 1)
    if fill not in (0, 1):
        raise ValueError(f"--view_fill {fill}: 0 or 1")
    if getattr(opt, "satellite", 0):
        raise NotImplementedError("--novel_view writes its files beside the --sceneflow outputs only")
    return dict(s=float(s), fill=bool(fill))


def novel_view_of_map(disp, exclude, left_u8, s, fill=True, right_u8=None, device="cuda"):
    """``kernels.forward_warp`` of the decoded left image through a written map [h', w'] (numpy:
    the disparity, the filled or the refined one, at the crop's or the scene's size) to baseline
    fraction ``s``.  The map's origin in the image is ``map_origin``'s; ``exclude`` [h', w'] or
    None: non-zero pixels carry no surface.  The image goes to float32 with torch ops, off the
    hot path.  Returns (view uint8 [h', w', 3], holes bool [h', w'], mad): holes are the pixels
    no surface covers (black with ``fill`` off, else taken from the background beside them);
    mad is the mean absolute difference in grey levels to ``right_u8`` over the other pixels, or
    None without it.  Refuses a map wider than the kernel's limit."""
    from . import kernels
    mh, mw = disp.shape
    if mw > kernels.FORWARD_WARP_MAX_W:
        raise ValueError(f"--novel_view: the map is {mw} pixels wide, the warp's limit is "
                         f"{kernels.FORWARD_WARP_MAX_W}")
    h, w = left_u8.shape[:2]
    x0, y0 = map_origin(h, w, mh, mw)

    def planes(img):
        t = _device_u8(img[y0:y0 + mh, x0:x0 + mw], device)
        return t[..., :3].permute(2, 0, 1).to(torch.float32).contiguous()[None]

    d = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32)).to(device)[None]
    e = None if exclude is None else torch.from_numpy(np.ascontiguousarray(exclude != 0).view(np.uint8)).to(device)[None]
    out = kernels.forward_warp(planes(left_u8), d, float(s), e, fill=bool(fill), want_zview=False)
    holes = out.state[0] != 0
    mad = None
    if right_u8 is not None:
        seen = ~holes
        diff = (out.image[0] - planes(right_u8)[0]).abs().mean(0)
        mad = float(diff[seen].mean().item()) if bool(seen.any().item()) else float("nan")
    view = out.image[0].round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    return view.cpu().numpy(), holes.cpu().numpy(), mad


def save_view(prefix, view, holes):
    """<prefix>_view.png (the synthesised view) and <prefix>_view_holes.png (8-bit: 255 where no
    surface of the source view covers the pixel)."""
    from PIL import Image
    Image.fromarray(view).save(prefix + "_view.png")
    save_float_png(prefix + "_view_holes.png", np.where(holes, 255, 0).astype(np.uint8))


def save_refined(prefix, refined, support, max_disp=192):
    """<prefix>_refined.npy (float32), <prefix>_refined.png (coloured like the disparity) and
    <prefix>_support.png (8-bit: the smoothed confidence, in [0, 1], scaled by 255)."""
    np.save(prefix + "_refined.npy", refined.astype(np.float32))
    plot_disparity(prefix + "_refined.png", refined, max_disp)
    save_float_png(prefix + "_support.png", np.clip(support, 0.0, 1.0))


def occlusion_u8(state):
    """The state map as an 8-bit image: consistent 0, inconsistent 127, out of view 255."""
    state = np.asarray(state)
    return np.where(state == 2, 255, state.astype(np.int32) * 127).astype(np.uint8)


def save_lr(prefix, right, state, filled, max_disp=192):
    """<prefix>_right.npy (float32), <prefix>_occ.png (``occlusion_u8``), <prefix>_filled.npy
    (float32) and <prefix>_filled.png (coloured like the disparity)."""
    np.save(prefix + "_right.npy", right.astype(np.float32))
    save_float_png(prefix + "_occ.png", occlusion_u8(state))
    np.save(prefix + "_filled.npy", filled.astype(np.float32))
    plot_disparity(prefix + "_filled.png", filled, max_disp)


def photometric_check(model, leftname, rightname, crop_height, crop_width, lr_threshold=0.0, device="cuda"):
    """The label-free quality measure of ``kernels.photometric_sums`` on one pair: (warped
    [h', w', 3], err [h', w'], loss, l1, dssim), the maps cropped like the disparity.  The
    images are the standardised network inputs, so the error is in units of their standard
    deviation.  ``err`` is -1 where a pixel takes no part: warped from outside the right
    image, in the padding of a pair smaller than the crop, or -- with ``lr_threshold`` > 0
    -- flagged by the left-right check (``DisparityLR.state`` passed as it is)."""
    from . import kernels
    left, right, h, w = load_transform(*load_pair(leftname, rightname), crop_height, crop_width,
                                       device)
    with torch.no_grad():
        if lr_threshold > 0:
            lr = model.forward_lr(left, right, lr_threshold)
            disp, exclude = lr.disp, lr.state
        else:
            disp, exclude = model(left, right), None
    if h < crop_height or w < crop_width:  # the zero padding is no image
        pad = torch.ones(disp.shape, device=disp.device, dtype=torch.uint8)
        pad[:, max(crop_height - h, 0):, max(crop_width - w, 0):] = 0
        exclude = pad if exclude is None else torch.maximum(exclude, pad)
    alpha = 0.85
    sums, warped, err = kernels.photometric_sums(left, right, disp, exclude, alpha, want_warped=True, want_err=True)
    s = sums.cpu().tolist()
    l1 = s[1] / s[0] if s[0] else 0.0
    dssim = s[3] / s[2] if s[2] else 0.0
    warped = crop_output(warped[0].permute(1, 2, 0).unsqueeze(0).cpu().numpy(), h, w, crop_height, crop_width)
    err = crop_output(err.cpu().numpy(), h, w, crop_height, crop_width)
    return warped, err, (1 - alpha) * l1 + alpha * dssim, l1, dssim


def save_photo(prefix, warped, err):
    """<prefix>_warped.png (the warped right image, min-max 8-bit like the satellite branch's
    float images), <prefix>_photo.npy (float32, -1 where a pixel takes no part) and
    <prefix>_photo.png (the error clipped to [0, 1])."""
    save_float_png(prefix + "_warped.png", warped)
    np.save(prefix + "_photo.npy", err.astype(np.float32))
    save_float_png(prefix + "_photo.png", np.clip(err, 0.0, 1.0))


def plot_disparity(savename, data, max_disp=192):
    """predict.py:246-247: ``plt.imsave(savename, data, vmin=0, vmax=max_disp, cmap='turbo')``."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.imsave(savename, data, vmin=0, vmax=max_disp, cmap="turbo")


def float_to_u8(img: np.ndarray) -> np.ndarray:
    """What skimage.io.imsave (predict.py:207,211) writes for a float array: its imageio
    plugin's ``image_as_uint(im, bitdepth=8)`` -- values already in [0, 1] scale by 255,
    anything else is min-max normalised first -- ``* 255 + 0.499999999`` then truncated
    (imageio 2.x, a third-party dependency absent here; restated from its source)."""
    im = np.asarray(img, dtype=np.float64)
    mi, ma = float(np.nanmin(im)), float(np.nanmax(im))
    if not (mi >= 0 and ma <= 1):
        if not (np.isfinite(mi) and np.isfinite(ma)):
            raise ValueError("image values are not finite")
        if ma == mi:  # imageio returns the values cast as they are
            return im.astype(np.uint8)
        im = (im - mi) / (ma - mi)
    return (im * 255.0 + 0.499999999).astype(np.uint8)


def save_float_png(savename, img):
    """skimage.io.imsave(savename, img) of predict.py:207,211 (PNG)."""
    from PIL import Image
    a = np.asarray(img)
    if a.dtype != np.uint8:
        a = float_to_u8(a)
    Image.fromarray(a).save(savename)


def crop_image(image, crop_height, crop_width):
    """predict.py:128-141: zero-pad the HWC image into the bottom-right of the crop
    (float32 result) when it fits, else centre-crop (its own dtype)."""
    data = np.moveaxis(np.asarray(image), [2], [0])
    n_layers, h, w = data.shape
    if h <= crop_height and w <= crop_width:
        result = np.zeros([n_layers, crop_height, crop_width], "float32")
        result[:, crop_height - h: crop_height, crop_width - w: crop_width] = data
    else:
        start_x = (w - crop_width) // 2
        start_y = (h - crop_height) // 2
        result = data[:, start_y: start_y + crop_height, start_x: start_x + crop_width]
    return np.moveaxis(result, [0], [2])


def satellite_names(data_path, save_path, line):
    """predict.py:258-263: the list line minus its last character names a directory
    holding satiml.png / satimr.png; outputs <save_path><name>.png and <name>_in.png."""
    cur = line[:-1]
    return (data_path + cur + "/satiml.png", data_path + cur + "/satimr.png",
            save_path + cur + ".png", save_path + cur + "_in.png")


def test_satellite(model, leftname, rightname, savename, in_savename, crop_height, crop_width,
                   confidence="none", radius=4, lr_threshold=0.0, runner=None):
    """predict.py:187-211: the disparity as a PNG (min-max 8-bit, as skimage writes a
    float image) and the left input cropped / padded to the crop.  With ``confidence``
    also <name>_conf.png beside <name>.png, with ``lr_threshold`` > 0 <name>_occ.png.
    With ``runner`` (--scene) the same files at the image's own size."""
    from PIL import Image
    if runner is not None:
        disp, lr = predict_scene(runner, leftname, rightname, confidence)
        if lr is not None:
            save_float_png(os.path.splitext(savename)[0] + "_occ.png", occlusion_u8(lr[2]))
        if confidence not in (None, "none"):
            disp, conf, _ = disp
            save_float_png(os.path.splitext(savename)[0] + "_conf.png", np.clip(conf, 0.0, 1.0))
        save_float_png(savename, disp)
        save_float_png(in_savename, crop_image(Image.open(leftname), *disp.shape))
        return disp
    if lr_threshold > 0:
        state = predict_pair_lr(model, leftname, rightname, crop_height, crop_width, lr_threshold)[2]
        save_float_png(os.path.splitext(savename)[0] + "_occ.png", occlusion_u8(state))
    disp = predict_pair(model, leftname, rightname, crop_height, crop_width, confidence=confidence,
                        radius=radius)
    if confidence not in (None, "none"):
        disp, conf, _ = disp
        save_float_png(os.path.splitext(savename)[0] + "_conf.png", np.clip(conf, 0.0, 1.0))
    save_float_png(savename, disp)
    save_float_png(in_savename, crop_image(Image.open(leftname), crop_height, crop_width))
    return disp


def load_checkpoint(model, path):
    """predict.py:52-67: checkpoint['state_dict'] with an optional 'module.' prefix,
    loaded with a loader that executes nothing from the file."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    sd = {(k.split(".", 1)[1] if k.startswith("module") else k): v
          for k, v in ckpt["state_dict"].items()}
    model.load_state_dict(sd, strict=True)


def sceneflow_names(data_path, line):
    """predict.py:267-273: left, right and GT names of one sceneflow list line."""
    cur = line.rstrip("\n")
    leftname = data_path + "frames_finalpass/" + cur
    rightname = data_path + "frames_finalpass/" + cur[: len(cur) - 13] + "right/" + cur[len(cur) - 8:]
    gtname = data_path + "disparity/" + cur[: len(cur) - 3] + "pfm"
    return leftname, rightname, gtname


def main(argv=None):
    from . import metrics
    from .config import default_arch_args, obtain_predict_args
    from .model import LEAStereo
    opt = default_arch_args(obtain_predict_args(argv))
    if not opt.lr_check >= 0:
        raise ValueError(f"--lr_check {opt.lr_check}: a threshold in pixels > 0, or 0 for off")
    if opt.refine and not (opt.refine_lambda > 0 and opt.refine_sigma > 0 and 1 <= opt.refine_iters <= 8):
        raise ValueError(f"--refine_lambda {opt.refine_lambda} and --refine_sigma {opt.refine_sigma} must be > 0, "
                         f"--refine_iters {opt.refine_iters} in 1..8")
    if opt.refine and opt.satellite:
        raise NotImplementedError("--refine writes its maps beside the --sceneflow outputs only")
    speckle = speckle_options(opt)
    cloud_opt = pointcloud_options(opt)
    rect_opt = rectify_options(opt)
    view_opt = novel_view_options(opt)
    dsm_opt = dsm_options(opt)
    if not torch.cuda.is_available():
        raise RuntimeError("leastereo_amd runs on a ROCm device only")
    set_rectifier(None if rect_opt is None else make_rectifier(**rect_opt))
    model = LEAStereo(opt, "cuda")
    if opt.resume:
        if not os.path.isfile(opt.resume):
            raise FileNotFoundError(opt.resume)
        load_checkpoint(model, opt.resume)
    model = model.cuda().eval()
    runner = None
    if opt.scene:
        if opt.photo_check:
            raise NotImplementedError("--photo_check with --scene is not supported: the photometric check "
                                      "scores one forward's crop; run it without --scene")
        from .scene import SceneRunner
        runner = SceneRunner(model, opt.crop_height, opt.crop_width, tile_batch=opt.scene_batch,
                             context=opt.scene_context, ramp=opt.scene_ramp,
                             confidence=opt.confidence != "none" or bool(opt.refine), radius=opt.conf_radius,
                             lr_threshold=opt.lr_check if opt.lr_check > 0 else (1.0 if opt.refine else None))
    os.makedirs(opt.save_path, exist_ok=True)
    with open(opt.test_list) as f:
        lines = f.readlines()
    if not (opt.sceneflow or opt.satellite):
        raise NotImplementedError("predict.py has list layouts for --sceneflow and --satellite only "
                                  "(the reference's other dataset flags write nothing)")
    for index, line in enumerate(lines):
        if opt.satellite:  # predict.py:258-264
            test_satellite(model, *satellite_names(opt.data_path, opt.save_path, line),
                           opt.crop_height, opt.crop_width, opt.confidence, opt.conf_radius, opt.lr_check,
                           runner)
        if not opt.sceneflow:
            continue
        print(f"Running for sceneflow {index}")
        leftname, rightname, gtname = sceneflow_names(opt.data_path, line)
        gt = None
        if os.path.isfile(gtname):  # predict.py:275-277 (the reference requires it)
            gt, _, _ = read_pfm(gtname)
            plot_disparity(opt.save_path + f"{index:d}_gt.png", gt, 192)
        t0 = time.time()
        lr, refined = None, None
        if runner is None and opt.lr_check > 0:
            lr = predict_pair_lr(model, leftname, rightname, opt.crop_height, opt.crop_width, opt.lr_check)
        if runner is not None and opt.refine:  # --scene --refine: the refinement of the blended maps with them
            disp, lr, refined = refine_pair(model, runner, leftname, rightname, opt)
            if not opt.lr_check > 0:
                lr = None  # the check that --refine implies writes no files of its own
        elif runner is not None:  # --scene: every map of the pair from one call
            disp, lr = predict_scene(runner, leftname, rightname, opt.confidence)
        elif lr is None or opt.confidence != "none":  # with --confidence: its own call on the pair
            disp = predict_pair(model, leftname, rightname, opt.crop_height, opt.crop_width,
                                confidence=opt.confidence, radius=opt.conf_radius)
        else:
            disp = lr[0]
        if runner is None and opt.refine:  # its own call on the pair
            refined = refine_pair(model, None, leftname, rightname, opt)[2]
        print(f"Processing time: {time.time() - t0:.4f}")
        if rect_opt is not None and rect_opt["save"]:
            save_rectified(os.path.join(opt.save_path, f"{index}"), last_rectified())
        if lr is not None:
            save_lr(os.path.join(opt.save_path, f"{index}"), *lr[1:])
            print(f"{index}: left-right check at {opt.lr_check:g} px flags {100.0 * float((lr[2] != 0).mean()):.2f} % "
                  f"of the pixels ({100.0 * float((lr[2] == 2).mean()):.2f} % out of view)")
        if opt.confidence != "none":
            disp, conf, local = disp
            save_confidence(os.path.join(opt.save_path, f"{index}"), conf, local)
        if refined is not None:
            save_refined(os.path.join(opt.save_path, f"{index}"), *refined)
            print(f"{index}: refined at lambda {opt.refine_lambda:g}, sigma {opt.refine_sigma:g}, "
                  f"{opt.refine_iters} iterations; {100.0 * float((refined[1] <= 1e-30).mean()):.2f} % of the pixels "
                  f"without support")
        if speckle is not None:  # on the map that is written, at its size
            removed, despeckled = despeckle(disp, None if lr is None else lr[2], **speckle)
            save_speckle(os.path.join(opt.save_path, f"{index}"), removed, despeckled)
            print(f"{index}: speckle filter at {speckle['max_size']} px, {speckle['max_diff']:g} px steps removes "
                  f"{100.0 * float(removed.mean()):.2f} % of the pixels")
        if cloud_opt is not None:  # from the best map the other flags made, at its size
            flagged = None if lr is None else lr[2] != 0
            if speckle is not None:
                flagged = removed if flagged is None else (flagged | removed)
            best, flagged = (refined[0], None) if refined is not None else (disp, flagged)
            if rect_opt is None:
                cloud = pointcloud_of_map(best, flagged, load_images(leftname, rightname)[0], **cloud_opt)
            else:  # the rectification is the calibration; left pixels without a source give no point
                pair, r = last_rectified(), _rectifier.rect
                cloud = pointcloud_of_map(best, flagged, pair.left, **dict(
                    cloud_opt, focal=r.focal, baseline=r.baseline, cx=r.cx, cy=r.cy, cx_right=r.cx_right,
                    valid=pair.valid[0]))
            save_pointcloud(os.path.join(opt.save_path, f"{index}"), cloud)
            print(f"{index}: point cloud of {cloud.xyz.shape[0]} points "
                  f"({100.0 * cloud.xyz.shape[0] / best.size:.2f} % of the pixels)")
        if dsm_opt is not None:  # from the map --pointcloud takes, at its size
            flagged = None if lr is None else lr[2] != 0
            if speckle is not None:
                flagged = removed if flagged is None else (flagged | removed)
            best, flagged = (refined[0], None) if refined is not None else (disp, flagged)
            if rect_opt is None:
                surface = dsm_of_map(best, flagged, load_images(leftname, rightname)[0], **dsm_opt)
            else:  # the rectification is the calibration, as for --pointcloud
                pair, r = last_rectified(), _rectifier.rect
                surface = dsm_of_map(best, flagged, pair.left, **dict(
                    dsm_opt, calib=dict(dsm_opt["calib"], focal=r.focal, baseline=r.baseline, cx=r.cx, cy=r.cy),
                    cx_right=r.cx_right, valid=pair.valid[0]))
            save_dsm(os.path.join(opt.save_path, f"{index}"), *surface)
            print(f"{index}: surface model of {surface[3]['size'][0]} x {surface[3]['size'][1]} cells of "
                  f"{surface[3]['cell']:g}; {100.0 * float((surface[2] == 2).mean()):.2f} % of the cells are empty")
        if view_opt is not None:  # from the best map the other flags made, at its size
            flagged = None if lr is None else lr[2] != 0
            if speckle is not None:
                flagged = removed if flagged is None else (flagged | removed)
            if refined is not None:
                best, flagged = refined[0], None
            else:
                best = disp if lr is None else lr[3]
            if rect_opt is None:
                left_img, right_img = load_images(leftname, rightname)
            else:
                left_img, right_img = last_rectified().left, last_rectified().right
            view, holes, mad = novel_view_of_map(best, flagged, left_img, view_opt["s"], view_opt["fill"],
                                                 right_img if view_opt["s"] == 1.0 else None)
            save_view(os.path.join(opt.save_path, f"{index}"), view, holes)
            print(f"{index}: view from baseline fraction {view_opt['s']:g}: {100.0 * float(holes.mean()):.2f} % of "
                  f"the pixels are holes" + ("" if mad is None else
                                             f"; mean absolute difference to the right image {mad:.3f} grey levels"))
        if opt.photo_check:
            warped, err, loss, l1, dssim = photometric_check(model, leftname, rightname, opt.crop_height,
                                                             opt.crop_width, opt.lr_check)
            save_photo(os.path.join(opt.save_path, f"{index}"), warped, err)
            print(f"{index}: mean photometric error {loss:.4f} (L1 {l1:.4f}, (1 - SSIM) / 2 {dssim:.4f}) over "
                  f"{100.0 * float((err >= 0).mean()):.2f} % of the pixels")
        plot_disparity(opt.save_path + f"{index:d}.png", disp, 192)  # predict.py:240
        np.save(os.path.join(opt.save_path, f"{index}.npy"), disp.astype(np.float32))
        if gt is not None and rect_opt is None:  # a ground truth of the raw view says nothing about a rectified pair
            ch, cw = disp.shape
            h, w = gt.shape
            y0, x0 = max(int((h - ch) / 2), 0), max(int((w - cw) / 2), 0)
            gt = np.ascontiguousarray(gt[y0:y0 + ch, x0:x0 + cw], dtype=np.float32)
            m = metrics.evaluate(disp, gt, opt.maxdisp)[0]  # evaluation.py:287-307, device
            print(f"{index}: EPE vs GT {m['epe']:.4f} px, 3px error {m['three_px_error']:.3f}, "
                  f"bad 1.0 {m['bad_1']:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
