"""Density control: splatfacto's refinement statistics and cull / split / duplicate.

The reference trains through nerfstudio's SplatfactoModel with its refinement defaults
(GaussCtrlModelConfig): after every iteration `after_train` folds xys.grad and radii into
three per-Gaussian statistics, and every `refine_every` steps `refinement_after` culls,
splits and duplicates Gaussians and edits the Adam state to match.  Here the statistics are
one HIP launch per step without a host sync (DensityStats.accumulate ->
gsplat_density_accumulate) and a refinement is a plan (gsplat_density_plan: per-row
predicates + exclusive scans), one host read of the four totals, and one gather over the six
parameters and their twelve Adam moments (gsplat_density_apply); csrc/density.hip.

The semantics are splatfacto 1.0.0's as recalled (nerfstudio is not a dependency; DESIGN.md
§4 "Density control" is the specification, tests/density_ref.py its torch restatement).
`step` is the 0-based iteration index nerfstudio passes its callbacks.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .scene import GaussianScene

_BASES = (1, 4, 9, 16, 25)


@dataclass
class DensityConfig:
    """splatfacto's refinement settings under its names, with its defaults."""
    num_train_data: int
    warmup_length: int = 500
    refine_every: int = 100
    cull_alpha_thresh: float = 0.1
    cull_scale_thresh: float = 0.5
    continue_cull_post_densification: bool = True
    reset_alpha_every: int = 30
    densify_grad_thresh: float = 0.0002
    densify_size_thresh: float = 0.01
    n_split_samples: int = 2
    cull_screen_size: float = 0.15
    split_screen_size: float = 0.05
    stop_screen_size_at: int = 4000
    stop_split_at: int = 15000

    @property
    def reset_interval(self) -> int:
        return self.reset_alpha_every * self.refine_every

    # ---- the schedule (pure functions of the step) ----
    def accumulates(self, step: int) -> bool:
        """after_train folds this step's gradients into the statistics."""
        return step < self.stop_split_at

    def should_refine(self, step: int) -> bool:
        return step % self.refine_every == 0 and step > self.warmup_length

    def densifies(self, step: int) -> bool:
        """A refinement at `step` splits / duplicates (and culls the concatenated set)."""
        return self.should_refine(step) and step < self.stop_split_at and \
            step % self.reset_interval > self.num_train_data + self.refine_every

    def culls_only(self, step: int) -> bool:
        return self.should_refine(step) and not self.densifies(step) and \
            step >= self.stop_split_at and self.continue_cull_post_densification

    def resets_opacity(self, step: int) -> bool:
        return self.should_refine(step) and step < self.stop_split_at and \
            step % self.reset_interval == self.refine_every

    def toobig_on(self, step: int) -> bool:
        return step > self.reset_interval

    def screen_on(self, step: int) -> bool:
        return step < self.stop_screen_size_at

    def opacity_cap(self) -> float:
        """logit(2 * cull_alpha_thresh): what an opacity reset clamps the logits to."""
        p = 2.0 * self.cull_alpha_thresh
        return math.log(p / (1.0 - p))


def _device_f32(name, *tensors):
    dev = _lib.check_device(name, *tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name}: fp32 tensors only")
    return dev


class DensityStats:
    """The three refinement statistics (grad_norm, vis_counts, max_2Dsize: fp32 [N] each).
    `fresh` until the first accumulate after a reset: that call writes every row, so the
    vectors are never memset."""

    def __init__(self, n: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DensityStats: expected a ROCm device, got {device} "
                               "(density control has no CPU path)")
        self.grad_norm = torch.empty((n,), device=device, dtype=torch.float32)
        self.vis_counts = torch.empty((n,), device=device, dtype=torch.float32)
        self.max_2Dsize = torch.empty((n,), device=device, dtype=torch.float32)
        self.fresh = True

    @property
    def num_points(self) -> int:
        return self.grad_norm.shape[0]

    def reset(self, n: Optional[int] = None):
        """Forget the statistics (after a refinement); n: the new number of Gaussians."""
        if n is not None and n != self.num_points:
            dev = self.grad_norm.device
            self.grad_norm, self.vis_counts, self.max_2Dsize = (
                torch.empty((n,), device=dev, dtype=torch.float32) for _ in range(3))
        self.fresh = True

    @torch.no_grad()
    def accumulate(self, xys_grad: torch.Tensor, radii: torch.Tensor, H: int, W: int):
        """splatfacto's after_train for one rendered view: one launch, no host sync."""
        n = self.num_points
        if xys_grad.dtype != torch.float32 or not xys_grad.is_contiguous():
            xys_grad = xys_grad.float().contiguous()
        if radii.dtype != torch.int32 or not radii.is_contiguous():
            radii = radii.to(torch.int32).contiguous()
        dev = _lib.check_device("DensityStats.accumulate", xys_grad, radii, self.grad_norm)
        if xys_grad.shape != (n, 2) or radii.shape != (n,):
            raise ValueError(f"DensityStats.accumulate: expected v_xy [{n},2] and radii [{n}]")
        P = _lib.ptr
        _lib.call("gsplat_density_accumulate", n, P(xys_grad), P(radii), int(H), int(W),
                  int(self.fresh), P(self.grad_norm), P(self.vis_counts), P(self.max_2Dsize),
                  _lib.stream(dev))
        self.fresh = False


def draw_split_samples(cfg: DensityConfig, n: int, generator: torch.Generator, device):
    """The split children's standard-normal samples z [n_split_samples, N, 3], indexed by
    original row (splatfacto draws per split row: the same distribution), drawn on the
    generator's device and moved to `device` -- a CPU generator gives every device and every
    rank the same samples."""
    z = torch.randn((cfg.n_split_samples, n, 3), generator=generator, dtype=torch.float32,
                    device=generator.device)
    return z.to(device)


def _pointer_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for k, t in enumerate(tensors):
        arr[k] = None if t is None or t.numel() == 0 else t.data_ptr()
    return arr


@torch.no_grad()
def refine(scene: GaussianScene, opt, stats: Optional[DensityStats], cfg: DensityConfig,
           step: int, H: int, W: int, generator: Optional[torch.Generator] = None,
           z: Optional[torch.Tensor] = None):
    """splatfacto's refinement_after at `step` (the caller checks cfg.should_refine(step)):
    cull / split / duplicate per the schedule, the Adam moments edited to match, then the
    opacity reset.  opt: the optim.FusedAdam holding the six parameters; the refined
    parameters and moments replace them in it (FusedAdam.replace; the step count stays).
    Returns (scene, report): the new GaussianScene (leaf, contiguous fp32 tensors that require
    grad) and dict(n_before, n_after, n_split: split rows whose children survive, n_dup:
    surviving duplicates, n_culled: original rows removed -- split parents included --, so
    n_after = n_before - n_culled + n_split_samples n_split + n_dup; reset_opacity).  z: the split samples
    (draw_split_samples), else drawn from `generator`.  The statistics are reset."""
    params = scene.params()
    dev = _device_f32("density.refine", *params)
    n = scene.num_points
    K = 1 + scene.features_rest.shape[1]
    if K not in _BASES or scene.features_rest.shape[2:] != (3,):
        raise ValueError("density.refine: bad features_rest shape")
    mode = 1 if cfg.densifies(step) else (2 if cfg.culls_only(step) else 0)
    reset = cfg.resets_opacity(step)
    ns = int(cfg.n_split_samples)
    if mode == 1:
        if stats is None or stats.fresh or stats.num_points != n:
            raise RuntimeError("density.refine: a densifying step needs accumulated statistics")
        if z is None:
            if generator is None:
                raise ValueError("density.refine: a densifying step needs z or a generator")
            z = draw_split_samples(cfg, n, generator, dev)
        if z.shape != (ns, n, 3):
            raise ValueError(f"density.refine: z must be [{ns},{n},3]")
        z = z.to(device=dev, dtype=torch.float32).contiguous()
    else:
        z = torch.empty((1,), device=dev, dtype=torch.float32)  # (no children: never read)
    by_param = {id(g["params"][0]): g for g in opt.param_groups}
    moments = []
    for p in params:
        if id(p) not in by_param:
            raise ValueError("density.refine: the optimiser does not hold the scene's parameters")
        st = opt._buffers(p)
        moments.append((st["exp_avg"], st["exp_avg_sq"]))
    P, st = _lib.ptr, _lib.stream(dev)
    words = 4 + 4 * n + 3 * ((n + 255) // 256)  # GSPLAT_DENSITY_PLAN_WORDS
    plan = torch.empty((words,), device=dev, dtype=torch.int32)
    use_stats = mode == 1
    _lib.call("gsplat_density_plan", n, P(scene.scales), P(scene.opacities),
              P(stats.grad_norm) if use_stats else None,
              P(stats.vis_counts) if use_stats else None,
              P(stats.max_2Dsize) if use_stats else None,
              mode, int(cfg.toobig_on(step)), int(cfg.screen_on(step)), ns, max(int(H), int(W)),
              cfg.cull_alpha_thresh, cfg.cull_scale_thresh, cfg.cull_screen_size,
              cfg.densify_grad_thresh, cfg.densify_size_thresh, cfg.split_screen_size,
              P(plan), 4 * words, st)
    kept, n_split, n_dup, new_n = (int(v) for v in plan[:4].tolist())  # the refinement's sync
    f32 = dict(device=dev, dtype=torch.float32)
    shapes = [(new_n,) + tuple(p.shape[1:]) for p in params]
    out_p = [torch.empty(s, **f32) for s in shapes]
    out_m = [torch.empty(s, **f32) for s in shapes]
    out_v = [torch.empty(s, **f32) for s in shapes]
    src_rows = torch.empty((max(new_n, 1),), device=dev, dtype=torch.int32)
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    _lib.call("gsplat_density_apply", n, new_n, K, ns, P(plan), 4 * words,
              cast(_pointer_array(params)), cast(_pointer_array([m for m, _ in moments])),
              cast(_pointer_array([v for _, v in moments])), P(z),
              cast(_pointer_array(out_p)), cast(_pointer_array(out_m)),
              cast(_pointer_array(out_v)), P(src_rows), int(reset), cfg.opacity_cap(), st)
    if stats is not None:
        stats.reset(new_n)
    new_scene = GaussianScene(*out_p).requires_grad_()
    for p, q, m, v in zip(params, out_p, out_m, out_v):
        opt.replace(p, q, m, v)
    report = {"n_before": n, "n_after": new_n, "n_split": n_split, "n_dup": n_dup,
              "n_culled": n - kept, "reset_opacity": bool(reset)}
    return new_scene, report
