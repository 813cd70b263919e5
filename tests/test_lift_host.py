"""Mask lifting on the host: lift.select, and the reference the GPU tests rest on.

tests/test_gpu_lift.py checks gsplat_rasterize_splat_back against the oracle's rasterize backward
(v_colors with v_out = the pixel values, the forward's alpha clamp).  That this is the sum of
w v over the forward's composited pairs is shown here on the oracle alone, against a direct
per-pixel restatement (tests/lift_ref.py), together with the condition the selection test needs:
few Gaussians of the two-cluster scene sit on the vote's threshold.
"""
import numpy as np
import pytest
import torch

import lift_ref as R
import structured_scenes as S
from gaussctrl_exp_amd import lift


def test_select_hand_made():
    sums = torch.tensor([[3.0, 9.0, 9.0, 4.0],      # score 0.75, seen
                         [1.0, 0.0, 0.0, 4.0],      # score 0.25
                         [0.0, 0.0, 0.0, 0.0],      # never composited: score 0, no NaN
                         [5e-4, 0.0, 0.0, 5e-4],    # score 1 but below min_weight
                         [2.0, 0.0, 0.0, 4.0],      # score exactly at the threshold: not above
                         [-1.0, 0.0, 0.0, 2.0]],    # a negative vote
                        dtype=torch.float64)
    res = lift.select(sums, threshold=0.5, min_weight=1e-3)
    assert isinstance(res, lift.LiftResult)
    assert torch.equal(res.weight, sums[:, 3])
    assert torch.equal(res.score, torch.tensor([0.75, 0.25, 0.0, 1.0, 0.5, -0.5],
                                               dtype=torch.float64))
    assert res.selected.tolist() == [True, False, False, False, False, False]
    assert torch.isfinite(res.score).all()
    # the thresholds are arguments
    assert lift.select(sums, threshold=0.2, min_weight=1e-4).selected.tolist() == \
        [True, True, False, True, True, False]
    # float32 sums as the kernel writes them, and an empty scene
    assert lift.select(sums.float()).selected.tolist() == res.selected.tolist()
    empty = lift.select(torch.zeros(0, 4))
    assert empty.score.shape == empty.weight.shape == empty.selected.shape == (0,)
    with pytest.raises(ValueError):
        lift.select(torch.zeros(5, 3))


@pytest.mark.parametrize("scene", [S.early_exit, S.clamped], ids=["early_exit", "clamped"])
@pytest.mark.parametrize("channels", [1, 3])
def test_backward_colors_are_the_splat_sums(scene, channels, oracle_lib):
    """sum w v restated per pixel from the forward's decisions == the oracle backward's v_colors
    (v_out = values, zero v_out_alpha, the forward's clamp) to 1e-12 in float64; the weight
    column is the same identity for v_out = 1."""
    s = scene()
    st = s.state
    values = R.seeded_values(s.H, s.W, channels)
    direct = R.direct_sums(s.cam.tile_bounds, s.H, s.W, st["gids"], st["bins"], st["xys"],
                           st["conics"], st["opac"], values)
    ref, _ = R.scene_sums(s, values)
    print(f"[lift] {s.name} C={channels}: max |direct - backward| "
          f"{np.abs(direct - ref).max():.3e}, max |ref| {np.abs(ref).max():.3e}")
    assert np.abs(ref[:, 3]).max() > 1.0  # (something is composited)
    assert (ref[:, channels:3] == 0).all() and (direct[:, channels:3] == 0).all()
    assert np.abs(direct - ref).max() <= 1e-12


def test_backward_default_clamp_is_not_the_forward(oracle_lib):
    """With the backward's default clamp (0.99) the same call differs on clamped(): the GPU tests
    must -- and do -- ask for the forward's 0.999."""
    s = S.clamped()
    values = R.seeded_values(s.H, s.W, 3)
    ref, _ = R.scene_sums(s, values)
    quirk, _ = R.scene_sums(s, values, alpha_max=0.99)
    diff = np.abs(quirk - ref)
    print(f"[lift] clamped: max |v_colors(0.99) - v_colors(0.999)| {diff.max():.3e}")
    assert (diff > 1e-5 + 1e-4 * np.abs(ref)).any()


def test_two_clusters_condition(oracle_lib):
    """The selection test's condition: at least 90 % of the Gaussians with weight > min_weight
    have an oracle score farther than 1e-3 from the threshold; and the scene is what its
    docstring says (the right cluster farther than its radius from the boundary, in both views)."""
    tc = R.two_clusters()
    sums, _ = R.two_clusters_reference()
    res = lift.select(R.sums_tensor(sums), R.THRESHOLD, R.MIN_WEIGHT)
    score, weight = res.score.numpy(), res.weight.numpy()
    seen = weight > R.MIN_WEIGHT
    clear = np.abs(score - R.THRESHOLD) > 1e-3
    print(f"[lift] two clusters: {int(seen.sum())} of {seen.size} seen, "
          f"{int((seen & clear).sum())} clear of the threshold, "
          f"{int(res.selected.sum())} selected")
    assert seen.sum() >= 0.9 * seen.size
    assert (seen & clear).sum() >= 0.9 * seen.sum()
    for st in tc["states"]:
        assert st["fwd"]["num_intersects"] > 0
        assert (st["xys"][tc["right"], 0] - st["radii"][tc["right"]] > R.BOUNDARY).all()
        assert (st["xys"][tc["left"], 0] + st["radii"][tc["left"]] < R.BOUNDARY - 1).all()
    sel = res.selected.numpy()
    assert sel[tc["left"] & seen].all() and not sel[tc["right"]].any()
    # the straddling Gaussians see both halves: their votes are strictly between 0 and 1
    mid = tc["straddle"] & seen
    assert mid.any() and ((score[mid] > 0.02) & (score[mid] < 0.98)).all()
