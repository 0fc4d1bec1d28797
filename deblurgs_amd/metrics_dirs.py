"""The reference's metrics.py restated: SSIM, PSNR and LPIPS-vgg of every render against its ground truth in

    <scene>/test/<method>/renders/<name>      <scene>/test/<method>/gt/<name>

written to <scene>/results.json (the means per method) and <scene>/per_view.json (the values per image), with the
reference's keys and nesting (metrics.py:81-91).  Images are read with PIL and converted as torchvision's `to_tensor`
does: bytes / 255, the first three channels, [1,3,H,W] float32 (metrics.py:29-32).  Per image: `metrics.ssim` of the pair,
`metrics.psnr` of the [1,3,H,W] tensors (one value over the three channels, as the reference's call gives it) and
`lpips(..., vgg weights)` (metrics.py:72-74); on a HIP device SSIM and LPIPS run the library's kernels.

Three deviations from metrics.py:24-34,92, all on purpose:
  * names are sorted (os.listdir's order is the file system's);
  * a scene that fails raises (the reference swallows every exception in a bare `except` and prints one line);
  * renders and ground truth are matched by name, and a file without its partner raises FileNotFoundError.

The weights are the caller's (lpips.LPIPSVggWeights); nothing is fetched.

    python -m deblurgs_amd.metrics_dirs -m SCENE... --vgg-backbone vgg16-397923af.pth --vgg-lin vgg.pth
"""
import argparse
import json
import os

import torch

from . import lpips as _lpips
from . import metrics


def _to_tensor(path, device):
    """torchvision.transforms.functional.to_tensor(Image.open(path)).unsqueeze(0)[:, :3] for 8-bit images."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint8:
        raise ValueError(f"{path}: only 8-bit images are read (got {a.dtype})")
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(a.copy()).permute(2, 0, 1).to(torch.float32).div(255)
    return t[None, :3].contiguous().to(device)


def read_images(renders_dir, gt_dir, device):
    """(renders, gts, names) of a method directory, names sorted; a file present on one side only raises."""
    names, gt_names = sorted(os.listdir(renders_dir)), sorted(os.listdir(gt_dir))
    for n in names:
        if n not in gt_names:
            raise FileNotFoundError(f"{os.path.join(renders_dir, n)} has no ground truth {os.path.join(gt_dir, n)}")
    for n in gt_names:
        if n not in names:
            raise FileNotFoundError(f"{os.path.join(gt_dir, n)} has no render {os.path.join(renders_dir, n)}")
    renders = [_to_tensor(os.path.join(renders_dir, n), device) for n in names]
    gts = [_to_tensor(os.path.join(gt_dir, n), device) for n in names]
    return renders, gts, names


@torch.no_grad()
def evaluate_directories(model_paths, lpips_weights, device=None):
    """metrics.py:36-93 for every scene directory of model_paths; returns (full_dict, per_view_dict) and writes each
    scene's two JSON files.  lpips_weights: an lpips.LPIPSVggWeights (moved to `device`; default: the current HIP
    device)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    w = lpips_weights if lpips_weights.device == device else lpips_weights.to(device)
    full_dict, per_view_dict = {}, {}
    for scene_dir in model_paths:
        scene_dir = str(scene_dir)
        full_dict[scene_dir], per_view_dict[scene_dir] = {}, {}
        test_dir = os.path.join(scene_dir, "test")
        for method in sorted(os.listdir(test_dir)):
            method_dir = os.path.join(test_dir, method)
            renders, gts, names = read_images(os.path.join(method_dir, "renders"), os.path.join(method_dir, "gt"), device)
            ssims, psnrs, lpipss = [], [], []
            for r, g in zip(renders, gts):
                ssims.append(metrics.ssim(r[0], g[0]))
                psnrs.append(metrics.psnr(r, g))
                lpipss.append(_lpips.lpips(r, g, w))
            ssims, psnrs, lpipss = (torch.stack([v.reshape(()) for v in vs]).float().cpu() for vs in (ssims, psnrs, lpipss))
            full_dict[scene_dir][method] = {"SSIM": ssims.mean().item(), "PSNR": psnrs.mean().item(),
                                            "LPIPS": lpipss.mean().item()}
            per_view_dict[scene_dir][method] = {key: dict(zip(names, vals.tolist()))
                                                for key, vals in (("SSIM", ssims), ("PSNR", psnrs), ("LPIPS", lpipss))}
        with open(os.path.join(scene_dir, "results.json"), "w") as fp:
            json.dump(full_dict[scene_dir], fp, indent=True)
        with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
            json.dump(per_view_dict[scene_dir], fp, indent=True)
    return full_dict, per_view_dict


def main(argv=None):
    ap = argparse.ArgumentParser(description="SSIM, PSNR and LPIPS-vgg of rendered test views (the reference's metrics.py)")
    ap.add_argument("--model_paths", "-m", required=True, nargs="+", type=str)
    ap.add_argument("--vgg-backbone", required=True, help="torchvision's VGG16 checkpoint (vgg16-*.pth), a local file")
    ap.add_argument("--vgg-lin", required=True, help="the LPIPS v0.1 linear layers (vgg.pth), a local file")
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    w = _lpips.LPIPSVggWeights.load(a.vgg_backbone, a.vgg_lin)
    full, _ = evaluate_directories(a.model_paths, w, a.device)
    for scene, methods in full.items():
        print("Scene:", scene)
        for method, v in methods.items():
            print("Method:", method)
            for key in ("SSIM", "PSNR", "LPIPS"):
                print("  {:<5}: {:>12.7f}".format(key, v[key]))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
