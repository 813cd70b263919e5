"""Density control without a GPU: the schedule predicates of density.DensityConfig around every
boundary, and the torch restatement (density_ref.py) on a hand-worked six-row scene, one row per
class, against rows written out by hand."""
import math

import numpy as np
import torch

import density_ref as R
from gaussctrl_exp_amd.density import DensityConfig


def test_schedule_truth_table():
    c = DensityConfig(num_train_data=10)
    assert c.reset_interval == 3000
    # warmup_length (500) and refine_every (100)
    assert [c.should_refine(s) for s in (0, 100, 499, 500, 501, 550, 600)] == \
        [False, False, False, False, False, False, True]
    assert not c.densifies(500) and c.densifies(600) and not c.densifies(601)
    # num_train_data + refine_every (110) within a reset interval (3000)
    assert [c.densifies(s) for s in (2900, 3000, 3100, 3200)] == [True, False, False, True]
    c100 = DensityConfig(num_train_data=100)
    assert [c100.densifies(s) for s in (3100, 3200, 3300)] == [False, False, True]
    assert [c100.densifies(s) for s in (600, 700)] == [True, True]
    assert not DensityConfig(num_train_data=500).densifies(600)  # 600 > 600 fails
    assert DensityConfig(num_train_data=499).densifies(600)
    # the opacity reset: refine_every steps into every reset interval, after the warm-up
    assert [c.resets_opacity(s) for s in (100, 3000, 3100, 3101, 3200, 6100, 12100)] == \
        [False, False, True, False, False, True, True]
    assert not any(c.densifies(s) and c.resets_opacity(s) for s in range(0, 16000, 100))
    # reset_interval: the too-big cull starts after the first interval
    assert [c.toobig_on(s) for s in (2900, 3000, 3001, 3100)] == [False, False, True, True]
    # stop_screen_size_at (4000)
    assert [c.screen_on(s) for s in (3900, 3999, 4000, 4100)] == [True, True, False, False]
    # stop_split_at (15000)
    assert [c.densifies(s) for s in (14900, 15000, 15200)] == [True, False, False]
    assert [c.culls_only(s) for s in (14900, 15000, 15050, 15200)] == [False, True, False, True]
    assert [c.accumulates(s) for s in (14999, 15000)] == [True, False]
    assert c.resets_opacity(12100) and not c.resets_opacity(15100)
    off = DensityConfig(num_train_data=10, continue_cull_post_densification=False)
    assert not off.culls_only(15000) and off.should_refine(15000)
    # a schedule in which no refinement step can densify (refinements fall on step % 6 in {0, 3},
    # never above num_train_data + refine_every = 4), and one in which they can
    never = DensityConfig(num_train_data=1, warmup_length=2, refine_every=3, reset_alpha_every=2)
    assert [s for s in range(40) if never.should_refine(s)][:3] == [3, 6, 9]
    assert not any(never.densifies(s) for s in range(400))
    assert [s for s in range(13) if never.resets_opacity(s)] == [3, 9]
    can = DensityConfig(num_train_data=1, warmup_length=2, refine_every=3, reset_alpha_every=4)
    assert [s for s in range(25) if can.densifies(s)] == [6, 9, 18, 21]
    assert [s for s in range(25) if can.resets_opacity(s)] == [3, 15]
    assert math.isclose(c.opacity_cap(), math.log(0.2 / 0.8))


# ---- the hand-worked scene ------------------------------------------------------------------
# H x W = 80 x 100 (D = 100), defaults, num_train_data = 10, step 3500: a densifying step
# (3500 % 3000 = 500 > 110) with the too-big cull (3500 > 3000) and the screen tests (< 4000) on.
#   row  class            size    logit  g per call  radii (2 calls)   fate
#   0    untouched        0.02    2      5e-7        4, 4              kept
#   1    low opacity      0.02   -3      5e-7        0, 0              culled (sigmoid 0.047 < 0.1)
#   2    split            0.02    2      5e-5        3, 0              2 children, original removed
#   3    duplicate        0.005   2      5e-5        2, 2              kept + 1 copy
#   4    split and dup    0.005   2      5e-5        8, 8              screen 0.08 > 0.05: 2 children
#                                                                      + 1 copy, original removed
#   5    too big          0.6     2      5e-7        20, 20            culled (0.6 > 0.5)
SIZES = (0.02, 0.02, 0.02, 0.005, 0.005, 0.6)
LOGITS = (2.0, -3.0, 2.0, 2.0, 2.0, 2.0)


def _hand_scene():
    g = torch.Generator().manual_seed(3)
    p = {"means": torch.arange(18, dtype=torch.float32).reshape(6, 3) * 0.1,
         "scales": torch.log(torch.tensor(SIZES))[:, None].repeat(1, 3),
         "quats": torch.tensor([[1.0, 0, 0, 0]] * 4 + [[0, 0, 0, 2.0]] + [[1.0, 0, 0, 0]]),
         "opacities": torch.tensor(LOGITS)[:, None],
         "features_dc": torch.randn(6, 3, generator=g),
         "features_rest": torch.randn(6, 3, 3, generator=g)}
    m = {k: torch.randn(v.shape, generator=g) for k, v in p.items()}
    v = {k: torch.rand(v.shape, generator=g) for k, v in p.items()}
    return p, m, v


def _hand_stats(cfg):
    st = R.RefStats()
    small, large = (3e-7, 4e-7), (3e-5, 4e-5)  # norms 5e-7 and 5e-5
    v_xy = torch.tensor([small, small, large, large, large, small], dtype=torch.float32)
    R.accumulate(st, cfg, 3498, v_xy, torch.tensor([4, 0, 3, 2, 8, 20]), 80, 100)
    # the first call counts every row once, seen or not
    assert st.vis_counts.tolist() == [1, 1, 1, 1, 1, 1]
    R.accumulate(st, cfg, 3499, v_xy, torch.tensor([4, 0, 0, 2, 8, 20]), 80, 100)
    return st


def test_statistics_by_hand():
    st = _hand_stats(DensityConfig(num_train_data=10))
    assert st.vis_counts.tolist() == [2, 1, 1, 2, 2, 2]
    np.testing.assert_array_equal(
        st.max_2Dsize.numpy(), np.array([0.04, 0, 0.03, 0.02, 0.08, 0.2], dtype=np.float32))
    np.testing.assert_allclose(st.grad_norm.numpy(), [1e-6, 5e-7, 5e-5, 1e-4, 1e-4, 1e-6],
                               rtol=1e-6)
    late = R.RefStats()
    R.accumulate(late, DensityConfig(num_train_data=10), 15000, torch.zeros(6, 2),
                 torch.ones(6, dtype=torch.int64), 80, 100)
    assert late.grad_norm is None  # skipped from stop_split_at


def test_refinement_by_hand():
    cfg = DensityConfig(num_train_data=10)
    step = 3500
    assert cfg.densifies(step) and cfg.toobig_on(step) and cfg.screen_on(step)
    p, m, v = _hand_scene()
    z = torch.tensor([[[0.0] * 3, [0.0] * 3, [1.0, -2.0, 0.5], [0.0] * 3, [2.0, 1.0, -1.0],
                       [0.0] * 3],
                      [[0.0] * 3, [0.0] * 3, [-1.0, 0.0, 3.0], [0.0] * 3, [0.5, -0.5, 4.0],
                       [0.0] * 3]])
    st = _hand_stats(cfg)
    out, nm, nv, report, info = R.refine(p, m, v, st, cfg, step, 80, 100, z)
    R.assert_clear_of_thresholds(info["margins"])
    assert st.grad_norm is None  # reset
    assert report == {"n_before": 6, "n_after": 8, "n_split": 2, "n_dup": 2, "n_culled": 4,
                      "reset_opacity": False}
    # [originals] [children s=0, parent order] [children s=1] [duplicates, row order]
    src = [0, 3, 2, 4, 2, 4, 3, 4]
    assert info["source"].tolist() == src
    assert info["kind"].tolist() == [0, 0, 1, 1, 1, 1, 2, 2]
    for k in ("quats", "opacities", "features_dc", "features_rest"):
        np.testing.assert_array_equal(out[k].numpy(), p[k][src].numpy())
    # means: row 2 has the identity rotation (mean + 0.02 z); row 4's quaternion (0,0,0,2) is a
    # half turn about z (mean + 0.005 (-z_x, -z_y, z_z))
    f32 = lambda a: p["means"].numpy()[a].astype(np.float64)
    want = np.stack([
        f32(0), f32(3),
        f32(2) + 0.02 * np.array([1.0, -2.0, 0.5]), f32(4) + 0.005 * np.array([-2.0, -1.0, -1.0]),
        f32(2) + 0.02 * np.array([-1.0, 0.0, 3.0]), f32(4) + 0.005 * np.array([-0.5, 0.5, 4.0]),
        f32(3), f32(4)])
    np.testing.assert_allclose(out["means"].numpy(), want, rtol=0, atol=1e-8)
    np.testing.assert_array_equal(out["means"].numpy()[[0, 1, 6, 7]],
                                  p["means"].numpy()[[0, 3, 3, 4]])
    s = lambda x: [math.log(x)] * 3
    want = np.array([s(0.02), s(0.005), s(0.02 / 1.6), s(0.005 / 1.6), s(0.02 / 1.6),
                     s(0.005 / 1.6), s(0.005), s(0.005)])
    np.testing.assert_allclose(out["scales"].numpy(), want, rtol=0, atol=1e-7)
    # moments: the two kept originals keep theirs, the six new rows start from zero
    for k in R.PARAM_NAMES:
        for new, old in ((nm, m), (nv, v)):
            np.testing.assert_array_equal(new[k].numpy()[:2], old[k].numpy()[[0, 3]])
            assert not new[k].numpy()[2:].any()


def test_cull_only_and_reset_by_hand():
    p, m, v = _hand_scene()
    cfg = DensityConfig(num_train_data=10)
    # after stop_split_at: low opacity and too big go, nothing else; no statistics needed
    out, nm, nv, report, info = R.refine(p, m, v, R.RefStats(), cfg, 15000, 80, 100, None)
    assert info["source"].tolist() == [0, 2, 3, 4] and report["n_culled"] == 2
    assert report["n_split"] == report["n_dup"] == 0 and not report["reset_opacity"]
    np.testing.assert_array_equal(nm["quats"].numpy(), m["quats"].numpy()[[0, 2, 3, 4]])
    # an opacity-reset step deletes nothing, clamps the logits and zeroes the opacity moments
    out, nm, nv, report, info = R.refine(p, m, v, R.RefStats(), cfg, 3100, 80, 100, None)
    assert report == {"n_before": 6, "n_after": 6, "n_split": 0, "n_dup": 0, "n_culled": 0,
                      "reset_opacity": True}
    cap = np.float32(math.log(0.25))
    np.testing.assert_array_equal(out["opacities"].numpy()[:, 0],
                                  np.array([cap, -3.0, cap, cap, cap, cap], dtype=np.float32))
    assert not nm["opacities"].numpy().any() and not nv["opacities"].numpy().any()
    np.testing.assert_array_equal(nm["means"].numpy(), m["means"].numpy())
    np.testing.assert_array_equal(out["scales"].float().numpy(), p["scales"].numpy())
