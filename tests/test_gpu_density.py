"""Density control on the GPU (csrc/density.hip through gaussctrl_exp_amd.density, FusedAdam
and TrainStep) against the torch restatement of the specification (density_ref.py).

Copied rows (survivors, duplicates, a child's four copied fields, survivors' Adam moments) must
be bit-equal; computed values (a child's mean and scales) within the project's 1e-5 absolute +
1e-4 relative of the float64 restatement; grad_norm within rtol 2e-6 (the norm and up to three
adds in fp32, with or without contraction: a few ulp).  Every compared quantity of the
constructed populations lies at least 1 % from its threshold (asserted at 1e-3 on the
restatement's values), so a device-versus-host ulp cannot flip a mask.

The end-to-end test's short schedule (warmup_length 2, refine_every 3, reset_alpha_every 2,
num_train_data 1) can never densify under the specification -- its refinements fall on
step % 6 in {0, 3}, never above num_train_data + refine_every = 4
(test_density_ref.test_schedule_truth_table) -- so it runs as it is (opacity resets only)
and again with reset_alpha_every 4, whose step 6 is its first densifying refinement."""
import math
import os
import socket

import numpy as np
import pytest
import torch

import density_ref as R
from gaussctrl_exp_amd import _lib
from gaussctrl_exp_amd.density import (DensityConfig, DensityStats, draw_split_samples,
                                       refine)
from gaussctrl_exp_amd.optim import FusedAdam
from gaussctrl_exp_amd.scene import PARAM_NAMES, GaussianScene
from gaussctrl_exp_amd.train import GROUP_LR

pytestmark = pytest.mark.gpu
H, W = 64, 96
npy = lambda t: t.detach().cpu().numpy()


# ---- accumulate -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_accumulate_matches_restatement(gpu, n):
    cfg = DensityConfig(num_train_data=10)
    g = torch.Generator().manual_seed(n)
    stats, ref = DensityStats(n, gpu), R.RefStats()
    assert stats.fresh
    for call in range(3):
        v_xy = torch.randn(n, 2, generator=g) * 1e-4
        radii = torch.randint(1, 40, (n,), generator=g, dtype=torch.int32)
        radii[torch.rand(n, generator=g) < 0.4] = 0
        if n == 1:
            radii[0] = (7, 0, 11)[call]
        stats.accumulate(v_xy.to(gpu), radii.to(gpu), H, W)
        R.accumulate(ref, cfg, call, v_xy, radii, H, W)
        assert not stats.fresh
        np.testing.assert_array_equal(npy(stats.vis_counts), ref.vis_counts.numpy())
        np.testing.assert_array_equal(npy(stats.max_2Dsize), ref.max_2Dsize.numpy())
        np.testing.assert_allclose(npy(stats.grad_norm).astype(np.float64),
                                   ref.grad_norm.numpy(), rtol=2e-6, atol=0)
    if n > 1:
        assert ref.vis_counts.min() == 1 and ref.vis_counts.max() == 3
    stats.reset()
    assert stats.fresh


# ---- plan and apply -------------------------------------------------------------------------
def _population(n, K, seed, low_frac=0.2, high_frac=0.5, sizes=(0.004, 0.02, 0.7, 0.9)):
    """Every class in known proportions, each compared quantity >= 1 % from its threshold:
    sizes around 0.004 / 0.02 (either side of densify_size_thresh 0.01), 0.7 (too big, its
    child 0.44 not) and 0.9 (child 0.56 too big as well), each +-5 %; sigmoid(opacity) below
    0.076 or above 0.18; avg 0.1-0.5x or 2-5x densify_grad_thresh; max_2Dsize 0 / ~0.02 /
    ~0.09 (above split_screen_size) / ~0.3 (above cull_screen_size)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    size = torch.tensor(sizes)[torch.randint(0, len(sizes), (n,), generator=g)] * \
        (0.95 + 0.1 * rnd(n))
    scales = torch.log(size[:, None] * (0.3 + 0.6 * rnd(n, 3)))
    scales[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = torch.log(size)
    low = rnd(n) < low_frac
    opac = torch.where(low, -4 + 1.5 * rnd(n), -1.5 + 4.5 * rnd(n))[:, None]
    p = {"means": torch.randn(n, 3, generator=g), "scales": scales,
         "quats": torch.randn(n, 4, generator=g), "opacities": opac,
         "features_dc": torch.randn(n, 3, generator=g),
         "features_rest": torch.randn(n, K - 1, 3, generator=g)}
    m = {k: torch.randn(v.shape, generator=g) * 1e-3 for k, v in p.items()}
    # (second moments a real Adam history could hold, |exp_avg| <= 1.4 sqrt(exp_avg_sq): with
    # exp_avg_sq far below exp_avg^2 one step moves a parameter by many times its learning rate
    # and the fp32 rounding of that update alone exceeds test_gpu_optim.py's tolerance)
    v = {k: m[k] * m[k] * (0.5 + torch.rand(x.shape, generator=g)) + 1e-12
         for k, x in p.items()}
    high = rnd(n) < high_frac
    avg = 2e-4 * torch.where(high, 2 + 3 * rnd(n), 0.1 + 0.4 * rnd(n))
    vis = torch.randint(1, 4, (n,), generator=g).float()
    st = R.RefStats()
    st.grad_norm = (avg * vis / (0.5 * max(H, W))).double()
    st.vis_counts = vis
    st.max_2Dsize = torch.tensor([0.0, 0.02, 0.09, 0.3])[
        torch.randint(0, 4, (n,), generator=g)] * (0.95 + 0.1 * rnd(n))
    return p, m, v, st


def _to_gpu(p, m, v, st, dev, step_count=7):
    scene = GaussianScene(*[p[k].to(dev) for k in PARAM_NAMES]).requires_grad_()
    opt = FusedAdam([{"params": [getattr(scene, k)], "lr": GROUP_LR[k], "name": k}
                     for k in PARAM_NAMES], eps=1e-15)
    for k in PARAM_NAMES:
        buf = opt._buffers(getattr(scene, k))
        buf["exp_avg"].copy_(m[k])
        buf["exp_avg_sq"].copy_(v[k])
    opt.step_count = step_count
    stats = DensityStats(p["means"].shape[0], dev)
    if st.grad_norm is not None:
        stats.grad_norm.copy_(st.grad_norm.float())
        stats.vis_counts.copy_(st.vis_counts)
        stats.max_2Dsize.copy_(st.max_2Dsize)
        stats.fresh = False
    return scene, opt, stats


def _assert_refined(scene, opt, report, want, cfg):
    """The GPU's refined scene / optimiser state / report against the restatement's."""
    out, wm, wv, wreport, info = want
    assert report == wreport
    n2 = wreport["n_after"]
    child = info["kind"].cpu().numpy() == 1
    for k in PARAM_NAMES:
        got = getattr(scene, k)
        assert got.is_leaf and got.is_contiguous() and got.dtype == torch.float32 and \
            got.requires_grad and got.shape == (n2,) + tuple(out[k].shape[1:])
        a, b = npy(got), out[k].cpu().numpy()
        if k in ("means", "scales"):
            np.testing.assert_array_equal(a[~child], b[~child].astype(np.float32))
            d = np.abs(a[child].astype(np.float64) - b[child])
            assert (d <= 1e-5 + 1e-4 * np.abs(b[child])).all(), (k, d.max() if d.size else 0)
        else:  # copied bit for bit, children included (the opacity reset is an exact min)
            np.testing.assert_array_equal(a, b)
        st = opt.state[got]
        assert {id(g["params"][0]) for g in opt.param_groups} >= {id(got)}
        np.testing.assert_array_equal(npy(st["exp_avg"]), wm[k].cpu().numpy())
        np.testing.assert_array_equal(npy(st["exp_avg_sq"]), wv[k].cpu().numpy())
        new = info["kind"].cpu().numpy() != 0
        assert not npy(st["exp_avg"])[new].any() and not npy(st["exp_avg_sq"])[new].any()
    if wreport["reset_opacity"]:
        cap = cfg.opacity_cap()
        assert (npy(scene.opacities) <= cap + 1e-5 + 1e-4 * abs(cap)).all()
        st = opt.state[scene.opacities]
        assert not npy(st["exp_avg"]).any() and not npy(st["exp_avg_sq"]).any()


def _run_case(dev, p, m, v, st, cfg, step, seed=5):
    n = p["means"].shape[0]
    z = draw_split_samples(cfg, n, torch.Generator().manual_seed(seed), "cpu")
    scene, opt, stats = _to_gpu(p, m, v, st, dev)
    count = opt.step_count
    new_scene, report = refine(scene, opt, stats, cfg, step, H, W,
                               generator=torch.Generator().manual_seed(seed))
    assert opt.step_count == count and stats.fresh and stats.num_points == report["n_after"]
    want = R.refine(p, m, v, st, cfg, step, H, W, z)
    R.assert_clear_of_thresholds(want[4]["margins"])
    _assert_refined(new_scene, opt, report, want, cfg)
    return new_scene, opt, report, want


STEPS = {"densify_before_reset_interval": 600, "densify_toobig_and_screen": 3500,
         "densify_past_stop_screen_size": 4200, "cull_only_past_stop_split": 15000,
         "opacity_reset": 3100}


@pytest.mark.parametrize("K", [16, 1])
@pytest.mark.parametrize("case", list(STEPS))
def test_plan_and_apply_match_restatement(gpu, K, case):
    cfg = DensityConfig(num_train_data=10)
    step = STEPS[case]
    assert cfg.should_refine(step)
    assert cfg.densifies(step) == case.startswith("densify")
    assert cfg.culls_only(step) == (case == "cull_only_past_stop_split")
    assert cfg.resets_opacity(step) == (case == "opacity_reset")
    assert cfg.toobig_on(step) == (step > 3000) and cfg.screen_on(step) == (step < 4000)
    p, m, v, st = _population(777, K, seed=11)
    _, _, report, want = _run_case(gpu, p, m, v, st, cfg, step)
    kinds = want[4]["kind"]
    if cfg.densifies(step):  # every class is there
        assert report["n_split"] > 20 and report["n_dup"] > 20 and report["n_culled"] > 100
        assert int((kinds == 1).sum()) == 2 * report["n_split"]
        both = set(want[4]["source"][kinds == 1].tolist()) & \
            set(want[4]["source"][kinds == 2].tolist())
        assert (len(both) > 0) == cfg.screen_on(step)  # split and dup: by screen size only
    elif case == "cull_only_past_stop_split":
        assert 100 < report["n_culled"] < 777 and report["n_after"] == 777 - report["n_culled"]
    else:
        assert report["n_after"] == 777 and report["n_culled"] == 0


def test_nothing_selected_everything_culled_and_one_row(gpu):
    cfg = DensityConfig(num_train_data=10)
    # nothing selected at a densifying step: the outputs are the inputs, bit for bit
    p, m, v, st = _population(777, 16, seed=12, low_frac=0.0, high_frac=0.0)
    new_scene, opt, report, _ = _run_case(gpu, p, m, v, st, cfg, 600)
    assert report["n_after"] == 777 and report["n_culled"] == report["n_split"] == 0
    for k in PARAM_NAMES:
        np.testing.assert_array_equal(npy(getattr(new_scene, k)), p[k].numpy())
        np.testing.assert_array_equal(npy(opt.state[getattr(new_scene, k)]["exp_avg"]),
                                      m[k].numpy())
    # everything culled
    p, m, v, st = _population(777, 16, seed=13, low_frac=1.0)
    for step in (15000, 3500):
        new_scene, _, report, _ = _run_case(gpu, p, m, v, st, cfg, step)
        assert report["n_after"] == 0 and new_scene.num_points == 0
        assert new_scene.features_rest.shape == (0, 15, 3)
        st = _population(777, 16, seed=13, low_frac=1.0)[3]  # (the restatement reset it)
    # N = 1: split (two children replace it), duplicated, culled
    for sizes, high, low, n_after in (((0.02,), 1.0, 0.0, 2), ((0.004,), 1.0, 0.0, None),
                                      ((0.02,), 0.0, 1.0, 0)):
        p, m, v, st = _population(1, 4, seed=14, low_frac=low, high_frac=high, sizes=sizes)
        st.max_2Dsize[:] = 0.02
        _, _, report, _ = _run_case(gpu, p, m, v, st, cfg, 600)
        assert report["n_after"] == (2 if n_after is None else n_after)


def test_refine_has_no_cpu_path():
    p, m, v, st = _population(5, 4, seed=1)
    scene = GaussianScene(*[p[k] for k in PARAM_NAMES])
    with pytest.raises(RuntimeError, match="ROCm device"):
        refine(scene, None, None, DensityConfig(num_train_data=10), 600, H, W)
    with pytest.raises(RuntimeError, match="ROCm device"):
        DensityStats(5, "cpu")


def test_plan_rejects_row_counts_beyond_int32(gpu):
    n = (2 ** 31 - 1) // 4 + 1  # n (2 + 2 samples) > int32
    with pytest.raises(RuntimeError, match="exceed int32"):
        _lib.call("gsplat_density_plan", n, *([None] * 5), 0, 0, 0, 2, 96, *([0.1] * 6),
                  None, 0, None)


# ---- optimiser continuity ---------------------------------------------------------------------
def test_adam_step_after_refine_matches_torch(gpu):
    """One FusedAdam step after a refinement equals torch.optim.Adam on the restated state:
    survivors' moments, zero moments for the new rows, the same step number
    (test_gpu_optim.py's tolerance)."""
    cfg = DensityConfig(num_train_data=10)
    p, m, v, st = _population(777, 16, seed=21)
    scene, opt, report, want = _run_case(gpu, p, m, v, st, cfg, 3500)
    assert report["n_split"] and report["n_dup"] and report["n_culled"]
    g = torch.Generator().manual_seed(22)
    grads = {k: (torch.randn(getattr(scene, k).shape, generator=g) * 1e-3).to(gpu)
             for k in PARAM_NAMES}
    ref_p = {k: getattr(scene, k).detach().clone().requires_grad_() for k in PARAM_NAMES}
    ref = torch.optim.Adam([{"params": [ref_p[k]], "lr": GROUP_LR[k]} for k in PARAM_NAMES],
                           eps=1e-15, foreach=True)
    for k in PARAM_NAMES:
        ref.state[ref_p[k]] = {"step": torch.tensor(float(opt.step_count)),
                               "exp_avg": want[1][k].to(gpu).clone(),
                               "exp_avg_sq": want[2][k].to(gpu).clone()}
        ref_p[k].grad = grads[k].clone()
        getattr(scene, k).grad = grads[k].clone()
    before = opt.step_count
    opt.step()
    ref.step()
    assert opt.step_count == before + 1 == 8
    for k in PARAM_NAMES:
        torch.testing.assert_close(getattr(scene, k).detach(), ref_p[k].detach(), rtol=1e-6,
                                   atol=1e-7, msg=lambda s: f"{k}: {s}")
    # fused_spec / next_step_groups hand out the refined buffers
    spec = opt.fused_spec(scene.params())
    assert [int(a) for a in spec["exp_avgs"]] == \
        [opt.state[t]["exp_avg"].data_ptr() for t in scene.params()]
    assert opt.next_step_groups([scene.features_dc])[0][1] is \
        opt.state[scene.features_dc]["exp_avg"]


# ---- TrainStep end to end ---------------------------------------------------------------------
def _widest_gap(values, lo=0.25, hi=0.75):
    """The middle of the widest gap between consecutive sorted non-zero values around the
    median (between the lo and hi quantiles)."""
    s = torch.sort(values[values > 0].double()).values
    s = s[int(lo * len(s)):int(hi * len(s))]
    i = int(torch.argmax(s[1:] / s[:-1]))
    return float(0.5 * (s[i] + s[i + 1]))


def _capture(t):
    """Record the render outputs of t's steps (the restatement is driven from them by hand)."""
    outs, orig = [], t.forward_backward

    def fb(*a, **k):
        loss, out = orig(*a, **k)
        outs.append(out)
        return loss, out
    t.forward_backward = fb
    return outs


def _state(t):
    P = {k: getattr(t.scene, k).detach().clone() for k in PARAM_NAMES}
    M = {k: t.opt._buffers(getattr(t.scene, k))["exp_avg"].clone() for k in PARAM_NAMES}
    V = {k: t.opt._buffers(getattr(t.scene, k))["exp_avg_sq"].clone() for k in PARAM_NAMES}
    return P, M, V


def _install(t, want):
    """Continue the plain TrainStep `t` from a restated refinement."""
    out, wm, wv = want[:3]
    new = GaussianScene(*[out[k].float().contiguous() for k in PARAM_NAMES]).requires_grad_()
    for k in PARAM_NAMES:
        t.opt.replace(getattr(t.scene, k), getattr(new, k), wm[k].contiguous(),
                      wv[k].contiguous())
    t.rebind(new)


@pytest.mark.parametrize("fuse_adam", [True, False])
@pytest.mark.parametrize("reset_alpha_every", [2, 4])
def test_trainstep_density_end_to_end(gpu, fuse_adam, reset_alpha_every):
    from gaussctrl_exp_amd.camera import synthetic_camera
    from gaussctrl_exp_amd.fused import render_fused
    from gaussctrl_exp_amd.scene import synthetic_scene
    from gaussctrl_exp_amd.train import TrainStep
    base = dict(num_train_data=1, warmup_length=2, refine_every=3,
                reset_alpha_every=reset_alpha_every)
    sched = DensityConfig(**base)
    last = 6  # the second refinement: the first densifying one with reset_alpha_every 4
    assert sched.resets_opacity(3) and sched.densifies(6) == (reset_alpha_every == 4)
    cam = synthetic_camera(W, H).to(gpu)
    bg = torch.tensor([0.2, 0.4, 0.6], device=gpu)
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2)).to(gpu)
    scene = lambda: synthetic_scene(2000, 3, seed=1, scale_lo=0.01, scale_hi=0.05, device=gpu)
    kw = dict(sh_degree=3, loss="l1", render_mode="fused", fuse_adam=fuse_adam)
    seed = 31
    prev = _lib.set_deterministic(True)
    try:
        # run A: a plain TrainStep, the restatement driven by hand from its render outputs
        a = TrainStep(scene(), **kw)
        assert a.fuse_adam == fuse_adam
        outs, stats, cfg = _capture(a), R.RefStats(), sched
        zgen = torch.Generator().manual_seed(seed)
        for step in range(last + 1):
            a.step(cam, gt, background=bg)
            R.accumulate(stats, cfg, step, outs[-1]["xys_grad"](), outs[-1]["radii"], H, W)
            if not cfg.should_refine(step):
                continue
            if cfg.densifies(step):  # thresholds in the widest gaps around the medians
                avg = stats.grad_norm / stats.vis_counts.double() * 0.5 * max(H, W)
                size = a.scene.scales.detach().double().exp().max(dim=-1).values
                cfg = DensityConfig(densify_grad_thresh=_widest_gap(avg),
                                    densify_size_thresh=_widest_gap(size), **base)
                z = draw_split_samples(cfg, a.scene.num_points, zgen, gpu)
            else:
                z = None
            want = R.refine(*_state(a), stats, cfg, step, H, W, z)
            R.assert_clear_of_thresholds(want[4]["margins"])
            if step < last:
                _install(a, want)
        report = want[3]
        if cfg.densifies(last):  # split, dup and cull sets all non-empty
            assert report["n_split"] > 0 and report["n_dup"] > 0 and report["n_culled"] > 0
        # run B: the same steps with density control inside TrainStep
        b = TrainStep(scene(), density=cfg, density_seed=seed, **kw)
        for step in range(last + 1):
            b.step(cam, gt, background=bg)
            if step == 3:
                assert b.last_refine["reset_opacity"] and b.last_refine["n_after"] == 2000
        _assert_refined(b.scene, b.opt, b.last_refine, want, cfg)
        assert all(x is y for x, y in zip(b.params, b.scene.params()))
        assert b.scene.num_points == report["n_after"]
        for _ in range(3):
            assert math.isfinite(float(b.step(cam, gt, background=bg)))
        # stale N-keyed state would show here: the next render against a fresh clone's
        with torch.no_grad():
            mine = render_fused(b.scene, cam, 3, bg, clamp=False)["rgb"]
            clone = GaussianScene(*[p.detach().clone() for p in b.scene.params()])
            theirs = render_fused(clone, cam, 3, bg, clamp=False)["rgb"]
        np.testing.assert_array_equal(npy(mine), npy(theirs))
    finally:
        _lib.set_deterministic(prev)


def test_trainstep_caller_mode_accumulates_xys_grad(gpu):
    """render_mode="caller": the statistics come from out["xys"].grad."""
    from gaussctrl_exp_amd.camera import synthetic_camera
    from gaussctrl_exp_amd.scene import synthetic_scene
    from gaussctrl_exp_amd.train import TrainStep
    cfg = DensityConfig(num_train_data=1)
    t = TrainStep(synthetic_scene(2000, 3, seed=1, scale_lo=0.01, scale_hi=0.05, device=gpu),
                  sh_degree=3, loss="l1", render_mode="caller", density=cfg)
    outs, ref = _capture(t), R.RefStats()
    cam = synthetic_camera(W, H).to(gpu)
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2)).to(gpu)
    t.step(cam, gt, background=torch.tensor([0.2, 0.4, 0.6], device=gpu))
    assert outs[-1]["xys"].grad is not None and float(outs[-1]["xys"].grad.abs().max()) > 0
    R.accumulate(ref, cfg, 0, outs[-1]["xys"].grad, outs[-1]["radii"], H, W)
    np.testing.assert_array_equal(npy(t.density_stats.vis_counts), npy(ref.vis_counts))
    np.testing.assert_array_equal(npy(t.density_stats.max_2Dsize), npy(ref.max_2Dsize))
    np.testing.assert_allclose(npy(t.density_stats.grad_norm).astype(np.float64),
                               npy(ref.grad_norm), rtol=2e-6, atol=0)


# ---- two ranks ----------------------------------------------------------------------------------
RANK_CFG = dict(num_train_data=1, warmup_length=2, refine_every=3, reset_alpha_every=4)
RANK_SEED = 41


def _rank_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gaussctrl_exp_amd.camera import gc_camera, look_at_c2w
    from gaussctrl_exp_amd.scene import synthetic_scene
    from gaussctrl_exp_amd.train import TrainStep
    eye = ((0.0, 0.0, 4.0), (1.5, 0.5, 3.6))[rank]
    cam = gc_camera(look_at_c2w(eye, up=(0.0, 1.0, 0.0)), 110.0, 110.0, 48.0, 32.0, W, H).to(dev)
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(rank)).to(dev)
    cfg = DensityConfig(**RANK_CFG)
    t = TrainStep(synthetic_scene(3000, 3, seed=12, scale_lo=0.01, scale_hi=0.05, device=dev),
                  sh_degree=3, world_size=world, loss="l1", render_mode="fused", density=cfg,
                  density_seed=RANK_SEED)
    inner = t._refine

    def hooked(step, frame):  # this rank's state and statistics as the refinement starts
        if cfg.densifies(step):
            for name, d in zip(("p", "m", "v"), _state(t)):
                np.save(os.path.join(out_dir, f"pre_{name}{rank}.npy"),
                        torch.cat([d[k].reshape(-1) for k in PARAM_NAMES]).cpu().numpy())
            st = t.density_stats
            np.save(os.path.join(out_dir, f"stats{rank}.npy"),
                    np.stack([npy(st.grad_norm), npy(st.vis_counts), npy(st.max_2Dsize)]))
        inner(step, frame)
    t._refine = hooked
    bg = torch.tensor([0.3, 0.5, 0.7], device=dev)
    for step in range(7):
        t.step(cam, gt, background=bg)
    np.save(os.path.join(out_dir, f"report{rank}.npy"),
            np.array([t.last_refine[k] for k in ("n_before", "n_after", "n_split", "n_dup",
                                                 "n_culled")]))
    for name, d in zip(("p", "m", "v"), _state(t)):
        np.save(os.path.join(out_dir, f"post_{name}{rank}.npy"),
                torch.cat([d[k].reshape(-1) for k in PARAM_NAMES]).cpu().numpy())
    torch.cuda.synchronize()
    dist.destroy_process_group()


def _unflatten(flat, n, dev="cpu"):
    out, at = {}, 0
    for k, w in zip(PARAM_NAMES, (3, 3, 4, 1, 3, 45)):
        shape = (n, 15, 3) if k == "features_rest" else (n, w)
        out[k] = torch.from_numpy(flat[at:at + n * w].reshape(shape).copy())
        at += n * w
    assert at == flat.size
    return out


def test_two_ranks_refine_to_identical_tensors(tmp_path):
    """World 2 on one GPU over gloo, a camera per rank, through the first densifying refinement
    (step 6): both ranks end with bit-identical parameters and moments, and the result is the
    restatement's fed the ranks' summed (grad_norm, vis_counts) and max-ed (max_2Dsize)
    statistics and the shared split samples."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["GSPLAT_MI355X_DETERMINISTIC"] = "1"
    try:
        mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    finally:
        os.environ.pop("GSPLAT_MI355X_DETERMINISTIC", None)
    load = lambda name: np.load(tmp_path / name)
    for name in ("pre_p", "pre_m", "pre_v", "post_p", "post_m", "post_v", "report"):
        np.testing.assert_array_equal(load(f"{name}0.npy"), load(f"{name}1.npy"))
    n_before, n_after, n_split, n_dup, n_culled = load("report0.npy").tolist()
    assert n_before == 3000 and n_split + n_dup > 0
    s0, s1 = load("stats0.npy"), load("stats1.npy")
    assert not np.array_equal(s0[0], s1[0])  # the ranks saw different views
    st = R.RefStats()
    st.grad_norm = torch.from_numpy(s0[0] + s1[0]).double()
    st.vis_counts = torch.from_numpy(s0[1] + s1[1])
    st.max_2Dsize = torch.from_numpy(np.maximum(s0[2], s1[2]))
    cfg = DensityConfig(**RANK_CFG)
    z = draw_split_samples(cfg, 3000, torch.Generator().manual_seed(RANK_SEED), "cpu")
    want = R.refine(_unflatten(load("pre_p0.npy"), 3000), _unflatten(load("pre_m0.npy"), 3000),
                    _unflatten(load("pre_v0.npy"), 3000), st, cfg, 6, H, W, z)
    assert want[3] == {"n_before": 3000, "n_after": n_after, "n_split": n_split,
                       "n_dup": n_dup, "n_culled": n_culled, "reset_opacity": False}
    got = _unflatten(load("post_p0.npy"), n_after)
    for k in ("quats", "opacities", "features_dc", "features_rest"):
        np.testing.assert_array_equal(got[k].numpy(), want[0][k].numpy())
    np.testing.assert_allclose(got["means"].numpy(), want[0]["means"].numpy(), rtol=1e-4,
                               atol=1e-5)
