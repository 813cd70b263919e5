"""Density control A/B at the headline size: the HIP paths (csrc/density.hip) against the same
work in torch ops (tests/density_ref.py: boolean-mask indexing, repeat, cat), on the same GPU
tensors, in one process, timed with HIP events after settle iterations.

  accumulate   gsplat_density_accumulate (one launch)  vs  the torch-ops after_train
  refine       one densify-branch refinement: gsplat_density_plan + the totals' host read +
               gsplat_density_apply  vs  the torch-ops restatement

Byte model: accumulate 36 B per Gaussian; apply ~2 x 708 B per output row at SH degree 3 (59
floats x 3 tensors read and written).  Prints one line per measurement.

  python tools/density_bench.py [--n 1000000] [--iters 20] [--settle 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import density_ref as R  # noqa: E402
from gaussctrl_exp_amd.density import (DensityConfig, DensityStats, draw_split_samples,  # noqa: E402
                                       refine)
from gaussctrl_exp_amd.optim import FusedAdam  # noqa: E402
from gaussctrl_exp_amd.scene import PARAM_NAMES, GaussianScene, synthetic_scene  # noqa: E402
from gaussctrl_exp_amd.train import GROUP_LR  # noqa: E402


def timed(fn, iters, settle):
    """Median / min milliseconds of fn() by HIP events, after `settle` untimed calls."""
    for _ in range(settle):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--size", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("density_bench: needs a ROCm device (no CPU timing)")
    dev = torch.device("cuda:0")
    n, H, W = a.n, a.size, a.size
    lines = [f"density_bench: N={n} SH degree 3 frame {W}x{H} device {torch.cuda.get_device_name(0)}"
             f" iters={a.iters} settle={a.settle} (ms: median / min, HIP events)"]
    g = torch.Generator().manual_seed(0)
    cfg = DensityConfig(num_train_data=100)
    step = 3500  # a densifying step with the too-big cull and the screen tests on

    # ---- accumulate ----
    v_xy = (torch.randn(n, 2, generator=g) * 1e-4).to(dev)
    radii = torch.randint(1, 60, (n,), generator=g, dtype=torch.int32)
    radii[torch.rand(n, generator=g) < 0.4] = 0
    radii = radii.to(dev)
    stats, ref = DensityStats(n, dev), R.RefStats()
    hip = timed(lambda: stats.accumulate(v_xy, radii, H, W), a.iters, a.settle)
    tor = timed(lambda: R.accumulate(ref, cfg, 0, v_xy, radii, H, W), a.iters, a.settle)
    gb = 36 * n / 1e9
    lines.append(f"accumulate  hip   {hip[0]:8.4f} / {hip[1]:8.4f} ms   "
                 f"{gb / hip[0] * 1e3:7.1f} GB/s of the 36 B/Gaussian model, no host sync")
    lines.append(f"accumulate  torch {tor[0]:8.4f} / {tor[1]:8.4f} ms   "
                 f"(boolean-mask indexing: a host sync per index)   x{tor[0] / hip[0]:.1f}")

    # ---- one densify-branch refinement ----
    sc = synthetic_scene(n, 3, seed=1, scale_lo=0.004, scale_hi=0.03)
    p = {k: getattr(sc, k).to(dev) for k in PARAM_NAMES}
    m = {k: torch.randn(v.shape, device=dev) * 1e-3 for k, v in p.items()}
    v2 = {k: m[k] * m[k] for k in PARAM_NAMES}
    avg = 2e-4 * torch.where(torch.rand(n, generator=g) < 0.3, 3.0, 0.3)
    st_cpu = {"grad_norm": avg / (0.5 * max(H, W)), "vis_counts": torch.ones(n),
              "max_2Dsize": torch.rand(n, generator=g) * 0.04}
    z = draw_split_samples(cfg, n, torch.Generator().manual_seed(1), dev)
    last = {}

    def hip_refine():
        scene = GaussianScene(*[p[k] for k in PARAM_NAMES])
        opt = FusedAdam([{"params": [p[k]], "lr": GROUP_LR[k], "name": k} for k in PARAM_NAMES],
                        eps=1e-15)
        for k in PARAM_NAMES:
            opt.state[p[k]] = {"exp_avg": m[k], "exp_avg_sq": v2[k]}
        s = DensityStats(n, dev)
        s.grad_norm, s.vis_counts, s.max_2Dsize = (st_cpu[k].to(dev) for k in (
            "grad_norm", "vis_counts", "max_2Dsize"))
        s.fresh = False
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        _, last["hip"] = refine(scene, opt, s, cfg, step, H, W, z=z)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def torch_refine():
        s = R.RefStats()
        s.grad_norm, s.vis_counts, s.max_2Dsize = (st_cpu[k].to(dev) for k in (
            "grad_norm", "vis_counts", "max_2Dsize"))
        s.grad_norm = s.grad_norm.double()
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        last["torch"] = R.refine(p, m, v2, s, cfg, step, H, W, z)[3]
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    res = {}
    for name, fn in (("hip", hip_refine), ("torch", torch_refine)):
        for _ in range(a.settle):
            fn()
        ms = [fn() for _ in range(a.iters)]
        res[name] = (statistics.median(ms), min(ms))
    assert last["hip"] == last["torch"], (last["hip"], last["torch"])
    rep = last["hip"]
    gb = 2 * 708 * rep["n_after"] / 1e9
    lines.append(f"refine      {rep}")
    lines.append(f"refine      hip   {res['hip'][0]:8.3f} / {res['hip'][1]:8.3f} ms   "
                 f"{gb / res['hip'][0] * 1e3:7.1f} GB/s of the 2 x 708 B/output-row model "
                 "(plan + totals read + apply + allocations)")
    lines.append(f"refine      torch {res['torch'][0]:8.3f} / {res['torch'][1]:8.3f} ms   "
                 f"(float64 restatement: masks, repeat, cat over 18 tensors)   "
                 f"x{res['torch'][0] / res['hip'][0]:.1f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
