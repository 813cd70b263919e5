"""A torch restatement of the density-control specification (DESIGN.md §4 "Density control":
splatfacto 1.0.0's after_train / refinement_after as recalled), the reference of
test_density_ref.py and test_gpu_density.py.  Indexed like splatfacto -- boolean masks, repeat
and cat -- with float64 arithmetic for every computed quantity (the norms, the sizes, the
sigmoid, avg, the children's means and scales); copied rows stay the fp32 values they were.
Runs on any device; plain tensors in, plain tensors out."""
import math

import torch

PARAM_NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


class RefStats:
    """grad_norm (float64), vis_counts and max_2Dsize (float32: exact in either precision);
    None until the first accumulate after a reset."""

    def __init__(self):
        self.grad_norm = self.vis_counts = self.max_2Dsize = None

    def reset(self):
        self.grad_norm = self.vis_counts = self.max_2Dsize = None


def accumulate(stats: RefStats, cfg, step, v_xy, radii, H, W):
    """after_train."""
    if step >= cfg.stop_split_at:
        return
    vis = radii > 0
    g = v_xy.double().norm(dim=-1)
    if stats.grad_norm is None:
        stats.grad_norm = g.clone()
        stats.vis_counts = torch.ones_like(g, dtype=torch.float32)  # every row: the quirk
        stats.max_2Dsize = torch.zeros_like(g, dtype=torch.float32)
    else:
        stats.vis_counts[vis] = stats.vis_counts[vis] + 1
        stats.grad_norm[vis] = stats.grad_norm[vis] + g[vis]
    newradii = (radii[vis].double() / float(max(H, W))).float()
    stats.max_2Dsize[vis] = torch.maximum(stats.max_2Dsize[vis], newradii)


def quat_to_rotmat(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
        dim=-1).reshape(-1, 3, 3)


def refine(params, exp_avg, exp_avg_sq, stats, cfg, step, H, W, z):
    """refinement_after at a step with cfg.should_refine(step).  params / exp_avg / exp_avg_sq:
    {name: tensor} (fp32); z [n_split_samples, N, 3].  Returns (params, exp_avg, exp_avg_sq,
    report, info): the new tensors -- means and scales float64 (copied rows are the exact fp32
    values, children computed in float64), the rest the copied fp32 rows --, the report of
    density.refine, and info: `source` (the original row of every output row), `kind` (0
    survivor, 1 child, 2 duplicate per output row) and `margins`, the (name, values, threshold)
    of every comparison that decided a mask.  The statistics are reset."""
    n = params["means"].shape[0]
    dev = params["means"].device
    D = float(max(H, W))
    ns = cfg.n_split_samples
    reset_interval = cfg.reset_alpha_every * cfg.refine_every
    toobig_on = step > reset_interval
    screen_on = step < cfg.stop_screen_size_at
    densify = step < cfg.stop_split_at and \
        step % reset_interval > cfg.num_train_data + cfg.refine_every
    cull_only = not densify and step >= cfg.stop_split_at and \
        cfg.continue_cull_post_densification
    margins = []
    rows = torch.arange(n, device=dev)
    out = {k: (v.double() if k in ("means", "scales") else v) for k, v in params.items()}
    source, kind = rows, torch.zeros(n, dtype=torch.long, device=dev)
    n_split_all = 0

    def cull_mask(scales, opacities, max2d, use_screen):
        size = scales.double().exp().max(dim=-1).values
        sig = torch.sigmoid(opacities.double())[:, 0]
        margins.append(("sigmoid(opacity) vs cull_alpha_thresh", sig, cfg.cull_alpha_thresh))
        culls = sig < cfg.cull_alpha_thresh
        if toobig_on:
            margins.append(("size vs cull_scale_thresh", size, cfg.cull_scale_thresh))
            toobig = size > cfg.cull_scale_thresh
            if use_screen and screen_on:
                margins.append(("max_2Dsize vs cull_screen_size", max2d.double(),
                                cfg.cull_screen_size))
                toobig = toobig | (max2d > cfg.cull_screen_size)
            culls = culls | toobig
        return culls

    culls = None
    if densify:
        size = params["scales"].double().exp().max(dim=-1).values
        avg = stats.grad_norm.double() / stats.vis_counts.double() * 0.5 * D
        margins.append(("avg vs densify_grad_thresh", avg, cfg.densify_grad_thresh))
        margins.append(("size vs densify_size_thresh", size, cfg.densify_size_thresh))
        high = avg > cfg.densify_grad_thresh
        splits = size > cfg.densify_size_thresh
        if screen_on:
            margins.append(("max_2Dsize vs split_screen_size", stats.max_2Dsize.double(),
                            cfg.split_screen_size))
            splits = splits | (stats.max_2Dsize > cfg.split_screen_size)
        splits = splits & high
        dups = (size <= cfg.densify_size_thresh) & high
        n_split_all, n_dup_all = int(splits.sum()), int(dups.sum())
        # split_gaussians: n_split_samples children per split row, sample-major
        q = params["quats"][splits].double()
        rots = quat_to_rotmat(q / q.norm(dim=-1, keepdim=True))
        scaled = params["scales"][splits].double().exp().repeat(ns, 1) * \
            z[:, splits].reshape(-1, 3).double()
        child = {
            "means": torch.bmm(rots.repeat(ns, 1, 1), scaled[..., None]).squeeze(-1) +
            params["means"][splits].double().repeat(ns, 1),
            "scales": torch.log(params["scales"][splits].double().exp() / 1.6).repeat(ns, 1),
            "quats": params["quats"][splits].repeat(ns, 1),
            "opacities": params["opacities"][splits].repeat(ns, 1),
            "features_dc": params["features_dc"][splits].repeat(ns, 1),
            "features_rest": params["features_rest"][splits].repeat(ns, 1, 1)}
        out = {k: torch.cat([out[k], child[k], out[k][dups]]) for k in PARAM_NAMES}
        source = torch.cat([rows, rows[splits].repeat(ns), rows[dups]])
        kind = torch.cat([kind, torch.ones(ns * n_split_all, dtype=torch.long, device=dev),
                          2 * torch.ones(n_dup_all, dtype=torch.long, device=dev)])
        max2d = torch.cat([stats.max_2Dsize, torch.zeros(ns * n_split_all + n_dup_all,
                                                         device=dev)])
        culls = cull_mask(out["scales"], out["opacities"], max2d, True)
        culls[:n] = culls[:n] | splits
    elif cull_only:
        culls = cull_mask(out["scales"], out["opacities"], None, False)
    new_m = {k: torch.cat([exp_avg[k], torch.zeros((source.shape[0] - n,) + tuple(
        exp_avg[k].shape[1:]), device=dev)]) for k in PARAM_NAMES}
    new_v = {k: torch.cat([exp_avg_sq[k], torch.zeros((source.shape[0] - n,) + tuple(
        exp_avg_sq[k].shape[1:]), device=dev)]) for k in PARAM_NAMES}
    report = {"n_before": n, "n_split": 0, "n_dup": 0, "n_culled": 0}
    if culls is not None:
        keep = ~culls
        report["n_culled"] = int(culls[:n].sum())
        report["n_split"] = int(keep[n:n + n_split_all].sum())
        report["n_dup"] = int(keep[n + ns * n_split_all:].sum())
        out = {k: v[keep] for k, v in out.items()}
        new_m = {k: v[keep] for k, v in new_m.items()}
        new_v = {k: v[keep] for k, v in new_v.items()}
        source, kind = source[keep], kind[keep]
    reset = step < cfg.stop_split_at and step % reset_interval == cfg.refine_every
    if reset:
        p = 2.0 * cfg.cull_alpha_thresh
        out["opacities"] = torch.clamp(out["opacities"], max=math.log(p / (1.0 - p)))
        new_m["opacities"] = torch.zeros_like(new_m["opacities"])
        new_v["opacities"] = torch.zeros_like(new_v["opacities"])
    report["n_after"] = int(source.shape[0])
    report["reset_opacity"] = bool(reset)
    stats.reset()
    return out, new_m, new_v, report, {"source": source, "kind": kind, "margins": margins}


def assert_clear_of_thresholds(margins, rel=1e-3):
    """No compared value within `rel` (relative) of its threshold -- zero rows (new rows'
    max_2Dsize, unseen rows) excluded --, so a device-versus-host ulp cannot flip a mask."""
    for name, values, thr in margins:
        v = values[values != 0]
        if v.numel():
            gap = ((v - thr).abs() / abs(thr)).min().item()
            assert gap > rel, f"{name}: a row lies within {gap:.2e} of the threshold"
