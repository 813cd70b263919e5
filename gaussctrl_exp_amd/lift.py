"""Image values splatted back onto the Gaussians: mask lifting and label rendering.

The reference edits locally through 2D masks (one LangSAM mask per rendered view,
gaussctrl/gc_pipeline.py:264-282, composited in 2D at :417-422).  With a rasterizer the
multi-view-consistent mask is the rasterizer's transpose: every composited (pixel, Gaussian)
pair deposits its blend weight w = alpha T times the pixel's value on the Gaussian
(`splat_back`, csrc/raster.hip raster_splat_back_kernel); summed over the views and divided by
the total weight this is a per-Gaussian label (`lift_masks`, the vote of GaussianEditor and
Gaussian Grouping), the total weight alone a per-Gaussian visibility, and rendering the labels
as colours gives the consistent 2D mask back (`render_labels`).

`sums` is accumulated with fp32 atomics: it is not bit-reproducible from run to run, and
`set_deterministic` does not change that.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
from .project_gaussians import project_gaussians
from .rasterize import BLOCK_X, BLOCK_Y, bin_gaussians, rasterize_gaussians


class LiftResult(NamedTuple):
    score: Tensor     # [N] weighted mean of the mask over the pixels the Gaussian was blended into
    weight: Tensor    # [N] total blend weight over the views (visibility)
    selected: Tensor  # [N] bool


def splat_back(xys: Tensor, conics: Tensor, opacity: Tensor, gaussian_ids_sorted: Tensor,
               tile_bins: Tensor, values: Tensor, H: int, W: int,
               out: Optional[Tensor] = None) -> Tensor:
    """Add one view's sums to `out` [N,4] (a new zeroed tensor when None) and return it:
    out[g, c] += sum over the composited pixels p of w values[p, c] (c < C), out[g, 3] += sum w,
    with w = alpha T and exactly rasterize_gaussians' forward decisions.  xys [N,2], conics
    [N,3], opacity [N] or [N,1] (project_gaussians' outputs and the activated opacity),
    gaussian_ids_sorted / tile_bins from bin_gaussians, values [H,W,C] or [H,W], C <= 3, fp32."""
    H, W = int(H), int(W)
    n = xys.shape[0]
    if values.dim() == 2:
        values = values[..., None]
    if values.dim() != 3 or tuple(values.shape[:2]) != (H, W):
        raise ValueError("splat_back: values must be [H, W, C] (or [H, W])")
    C = values.shape[2]
    if not 1 <= C <= 3:
        raise ValueError(f"splat_back: 1 to 3 channels, not {C}")
    if xys.dim() != 2 or xys.shape[1] != 2 or conics.shape != (n, 3) or opacity.numel() != n:
        raise ValueError("splat_back: inconsistent per-Gaussian tensor shapes")
    tbx, tby = (W + BLOCK_X - 1) // BLOCK_X, (H + BLOCK_Y - 1) // BLOCK_Y
    if tile_bins.shape != (tbx * tby, 2):
        raise ValueError("splat_back: tile_bins must be [tiles, 2]")
    if out is None:
        out = torch.zeros((n, 4), device=xys.device, dtype=torch.float32)
    elif out.shape != (n, 4):
        raise ValueError("splat_back: out must be [N, 4]")
    tensors = (xys, conics, opacity, gaussian_ids_sorted, tile_bins, values, out)
    dev = _lib.check_device("splat_back", *tensors)
    if any(t.dtype != torch.float32 for t in (xys, conics, opacity, values, out)) or \
            gaussian_ids_sorted.dtype != torch.int32 or tile_bins.dtype != torch.int32:
        raise RuntimeError("splat_back: fp32 tensors and int32 binning only")
    if n == 0 or gaussian_ids_sorted.numel() == 0:
        return out
    P = _lib.ptr
    _lib.call("gsplat_rasterize_splat_back", tbx, tby, H, W, C, P(gaussian_ids_sorted),
              P(tile_bins), P(xys), P(conics), P(opacity), P(values), P(out), _lib.stream(dev))
    return out


def select(sums: Tensor, threshold: float = 0.5, min_weight: float = 1e-3) -> LiftResult:
    """The vote over splat_back's sums [N,4] (channel 0 the mask): weight = sums[:, 3], score =
    sums[:, 0] / weight where weight > 0 (else 0), selected = weight > min_weight and score >
    threshold.  Plain torch ops on any device."""
    if sums.dim() != 2 or sums.shape[1] != 4:
        raise ValueError("select: sums must be [N, 4]")
    weight = sums[:, 3]
    seen = weight > 0
    score = torch.where(seen, sums[:, 0] / torch.where(seen, weight, torch.ones_like(weight)),
                        torch.zeros_like(weight))
    return LiftResult(score, weight, (weight > min_weight) & (score > threshold))


def _project(scene, cam):
    """scene.render's activations and projection (gc_model.py:158-187)."""
    quats = scene.quats
    return project_gaussians(scene.means, torch.exp(scene.scales), 1,
                             quats / quats.norm(dim=-1, keepdim=True), *cam.project_args())


@torch.no_grad()
def lift_sums(scene, cams, masks) -> Tensor:
    """splat_back of masks[k] ([H,W] bool / uint8 / float) under cams[k], summed over the views
    into one [N,4] buffer; a view whose binning is empty adds nothing."""
    if len(cams) != len(masks):
        raise ValueError("lift_masks: one mask per camera")
    dev = scene.means.device
    sums = torch.zeros((scene.num_points, 4), device=dev, dtype=torch.float32)
    opacity = torch.sigmoid(scene.opacities).float().contiguous()
    for cam, mask in zip(cams, masks):
        H, W = cam.height, cam.width
        if tuple(mask.shape) != (H, W):
            raise ValueError("lift_masks: masks must be [H, W] of their camera")
        xys, depths, radii, conics, nth, _ = _project(scene, cam)
        num_intersects, gids, bins = bin_gaussians(xys, depths, radii, nth, H, W)
        if num_intersects < 1:
            continue
        values = mask.to(device=dev, dtype=torch.float32).contiguous()
        splat_back(xys.float().contiguous(), conics.float().contiguous(), opacity, gids, bins,
                   values, H, W, out=sums)
    return sums


def lift_masks(scene, cams, masks, threshold: float = 0.5,
               min_weight: float = 1e-3) -> LiftResult:
    """Lift per-view 2D masks onto the Gaussians: score = the blend-weighted mean of the masks
    over every (view, pixel) the Gaussian was composited at, weight = its total blend weight,
    selected = weight > min_weight and score > threshold (see select)."""
    return select(lift_sums(scene, cams, masks), threshold, min_weight)


@torch.no_grad()
def render_labels(scene, cam, labels: Tensor) -> Tensor:
    """Per-Gaussian labels ([N] or [N,C], C <= 3) rendered as colours over a zero background
    with rasterize_gaussians: [H,W,C], the multi-view-consistent 2D mask of a selection."""
    if labels.dim() == 1:
        labels = labels[:, None]
    if labels.dim() != 2 or labels.shape[0] != scene.num_points or not 1 <= labels.shape[1] <= 3:
        raise ValueError("render_labels: labels must be [N] or [N, C <= 3]")
    C = labels.shape[1]
    colors = torch.zeros((scene.num_points, 3), device=scene.means.device, dtype=torch.float32)
    colors[:, :C] = labels.to(colors)
    xys, depths, radii, conics, nth, _ = _project(scene, cam)
    img = rasterize_gaussians(xys, depths, radii, conics, nth, colors,
                              torch.sigmoid(scene.opacities), cam.height, cam.width,
                              background=torch.zeros(3, device=colors.device))
    return img[..., :C]
