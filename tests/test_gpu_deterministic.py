"""Deterministic rasterize backward (gsplat_set_deterministic / GSPLAT_MI355X_DETERMINISTIC,
SURVEY.md §5): two runs give bit-identical gradients -- through the gsplat API (caller path),
the fused training render (records) and the list-split backward -- and the gradients still
meet the oracle bar."""
import numpy as np
import pytest
import torch

import oracle as O
from gaussctrl_exp_amd import _lib, quirks
from gaussctrl_exp_amd.camera import synthetic_camera
from gaussctrl_exp_amd.fused import render_fused
from gaussctrl_exp_amd.scene import render, synthetic_scene

pytestmark = pytest.mark.gpu


@pytest.fixture
def deterministic():
    prev = _lib.set_deterministic(True)
    assert _lib.lib().gsplat_get_deterministic() == 1
    yield
    _lib.set_deterministic(prev)
    assert _lib.lib().gsplat_get_deterministic() == int(prev)


def _grads(gpu, mode, sc, cam, api=None):
    s = sc.to(gpu).requires_grad_()
    bg = torch.tensor([0.2, 0.4, 0.6], device=gpu)
    gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(3))
    if mode == "fused":
        out = render_fused(s, cam.to(gpu), 3, bg, return_alpha=True)
    else:
        out = render(s, cam.to(gpu), 3, bg, api=api)
    ((out["rgb"] - gt.to(gpu)).abs().sum() + 0.1 * out["accumulation"].sum()).backward()
    return [p.grad.detach().cpu().numpy() for p in s.params()]


# 128x96: the plain strip backward; 512x512: 1,024 tiles, the list-split backward
@pytest.mark.parametrize("size", [(128, 96, 4000), (512, 512, 30000)])
@pytest.mark.parametrize("mode", ["caller", "fused"])
def test_two_runs_bit_identical(gpu, deterministic, mode, size):
    W, H, n = size
    sc = synthetic_scene(n, 3, seed=7, scale_lo=0.005, scale_hi=0.05)
    cam = synthetic_camera(W, H)
    a = _grads(gpu, mode, sc, cam)
    b = _grads(gpu, mode, sc, cam)
    for name, x, y in zip(("means", "scales", "quats", "opacities", "dc", "rest"), a, b):
        assert np.abs(x).max() > 0, name
        np.testing.assert_array_equal(x, y, err_msg=name)


def test_deterministic_grads_meet_the_oracle_bar(gpu, deterministic):
    """Raster-level gradients of the deterministic backward vs the oracle (same bar as the
    atomic backward: their fp32 wave totals are summed exactly, so the slack is smaller)."""
    from parity import CaptureAPI, check_raster_level
    sc = synthetic_scene(3000, 3, seed=21, scale_lo=0.01, scale_hi=0.06)
    cam = synthetic_camera(128, 96)
    cap = CaptureAPI()
    _grads(gpu, "caller", sc, cam, api=cap)
    k = cap.cap
    check_raster_level(gpu, k["xys_in"], k["depths"], k["radii"], k["conics_in"], k["nth"],
                       k["colors_in"], k["opacity_in"], k["background"], 96, 128, k["v_img"],
                       k["v_alpha"], cap.raster_grads(sc.num_points))


def _fused_raster_level(gpu, sc, cam, loss="sum"):
    """The fused render's raster-level gradients (v_xy, v_conic, v_colors, v_opacity), its
    rasterizer inputs and the upstream gradients (v_img, v_alpha) it was fed."""
    s = sc.to(gpu).requires_grad_()
    bg = torch.tensor([0.2, 0.4, 0.6], device=gpu)
    gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(3))
    out = render_fused(s, cam.to(gpu), 3, bg, return_alpha=True, clamp=False)
    up = {}
    out["rgb"].register_hook(lambda g: up.__setitem__("v_img", g.detach().cpu().numpy()))
    out["accumulation"].register_hook(
        lambda g: up.__setitem__("v_alpha", g.detach().cpu().numpy()[..., 0]))
    d = (out["rgb"] - gt.to(gpu)).abs()
    a = out["accumulation"]
    ((d.sum() + 0.1 * a.sum()) if loss == "sum" else (d.mean() + 0.1 * a.mean())).backward()
    r = {k: v.detach().cpu().numpy() for k, v in out["raster_inputs"].items()}
    return [g.detach().cpu().numpy() for g in out["raster_grads"]()], r, up, bg.cpu().numpy()


def _oracle_sums(gpu, r, up, bg, H, W):
    """The oracle's raster backward on the GPU's forward state: (ref, sum|terms|, drift, flip)."""
    from parity import gpu_forward_state
    st = gpu_forward_state(gpu, r["xys"], r["depths"], r["radii"], r["conics"],
                           r["num_tiles_hit"], r["colors"], r["opacity"], bg, H, W)
    return O.rasterize_backward(st["tile_bounds"], H, W, st["gids"], st["bins"], r["xys"],
                                r["conics"], r["colors"], r["opacity"].reshape(-1), bg,
                                st["final_Ts"], st["final_idx"], up["v_img"], up["v_alpha"],
                                alpha_max=quirks.backward_alpha_clamp(), return_abs=True,
                                return_drift=True, return_flip=True)


@pytest.mark.parametrize("loss", ["sum", "mean"])
def test_deterministic_and_atomic_agree(gpu, loss):
    """The two accumulation modes add the same fp32 wave totals, exactly (deterministic) or in
    the atomics' order, so they differ by fp32 summation order alone: per element within the
    bar's summation slack (1e-5 + 1e-4 |ref| + 2^-20 sum|terms|, sum|terms| from the oracle) --
    not a loose rtol -- and each meets the oracle bar on its own.  `mean`: ADVICE r2's
    mean-reduced loss at 512x384 (per-pixel upstream gradients ~1e-6; the integer sums in units
    of 2^-80 must keep them), with the bar's 1e-5 absolute term scaled to the gradients."""
    from parity import assert_close, assert_raster_close
    if loss == "sum":
        sc = synthetic_scene(4000, 3, seed=9, scale_lo=0.005, scale_hi=0.05)
        cam = synthetic_camera(128, 96)
    else:
        sc = synthetic_scene(30000, 3, seed=13, scale_lo=0.005, scale_hi=0.05)
        cam = synthetic_camera(512, 384)
    prev = _lib.set_deterministic(True)
    try:
        d, r, up, bg = _fused_raster_level(gpu, sc, cam, loss)
    finally:
        _lib.set_deterministic(prev)
    a, r2, up2, _ = _fused_raster_level(gpu, sc, cam, loss)
    for k in r:  # identical forward state
        np.testing.assert_array_equal(r[k], r2[k], err_msg=k)
    np.testing.assert_array_equal(up["v_img"], up2["v_img"])
    ref, absum, drift, flip = _oracle_sums(gpu, r, up, bg, cam.height, cam.width)
    for k, name in enumerate(("v_xy", "v_conic", "v_colors", "v_opacity")):
        x, y = d[k].reshape(ref[k].shape), a[k].reshape(ref[k].shape)
        scale = max(float(np.abs(y).max()), 1e-30)
        if loss == "mean":
            assert scale < 1e-2, name  # the mean-loss regime
            assert np.count_nonzero(x) == np.count_nonzero(y), name  # nothing quantised away
        atol = 1e-5 if loss == "sum" else 1e-5 * scale
        assert_close(f"det vs atomic {name}", x, y, atol=atol, abs_sum=absum[k])
        assert_raster_close(f"det {name}", x, ref[k], absum[k], drift[k], flip[k])


@pytest.mark.parametrize("bwd,mode", [(0, "fused"), (1, "caller"), (2, "caller"),
                                      (1, "fused"), (2, "fused")])
@pytest.mark.parametrize("chunk", [64, 192])
def test_list_split_bit_identical_to_the_full_walk(gpu, deterministic, bwd, mode, chunk, hooks):
    """The list-split backward re-walks the positions behind each part with the full walk's
    operations, so every wave's per-Gaussian totals -- and the deterministic mode's exact sums of
    them -- equal the unsplit walk's bit for bit (8x8 blocks, 16x8 strips, and the frame-size
    dispatch through the fused records)."""
    sc = synthetic_scene(30000, 3, seed=5, scale_lo=0.005, scale_hi=0.06)
    cam = synthetic_camera(512, 384)
    _lib.call("gsplat_debug_set_raster_variant", 1, bwd, 0)
    try:
        _lib.call("gsplat_debug_set_chunk", -1)
        full = _grads(gpu, mode, sc, cam)
        _lib.call("gsplat_debug_set_chunk", chunk)
        split = _grads(gpu, mode, sc, cam)
    finally:
        _lib.call("gsplat_debug_set_chunk", 0)
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
    for name, x, y in zip(("means", "scales", "quats", "opacities", "dc", "rest"), full, split):
        assert np.abs(x).max() > 0, name
        np.testing.assert_array_equal(y, x, err_msg=name)


@pytest.mark.parametrize("bwd", [1, 2])
@pytest.mark.parametrize("chunk", [64, 0])
def test_keep_bits_on_off_bit_identical(gpu, deterministic, bwd, chunk, hooks):
    """the list-split backward after a plan-filling forward walks only the positions
    the forward's culls kept (keep bits); the cull is exactness-preserving, so with the keep
    bits off (debug flag bit 30: the backward re-stages and culls every position) the six
    gradients are bit-identical -- for the 8x8 blocks (bwd 1) and the 16x8 strips reading the
    union of two blocks' words (bwd 2, the headline geometry).  chunk 0: the frame-size split
    of a 512x384 frame (768 tiles)."""
    sc = synthetic_scene(30000, 3, seed=5, scale_lo=0.005, scale_hi=0.06)
    cam = synthetic_camera(512, 384)
    try:
        if chunk:
            _lib.call("gsplat_debug_set_chunk", chunk)
        _lib.call("gsplat_debug_set_raster_variant", 1, bwd, 0)
        on = _grads(gpu, "fused", sc, cam)
        _lib.call("gsplat_debug_set_raster_variant", 1, bwd, 1 << 30)
        off = _grads(gpu, "fused", sc, cam)
    finally:
        _lib.call("gsplat_debug_set_chunk", 0)
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
    for name, x, y in zip(("means", "scales", "quats", "opacities", "dc", "rest"), off, on):
        assert np.abs(x).max() > 0, name
        np.testing.assert_array_equal(y, x, err_msg=name)


def test_keep_bits_switch_between_forward_and_backward(gpu, deterministic, hooks):
    """keep bits switched ON between a forward that did not write them and its
    backward: the backward must not walk the never-written words (it re-stages instead), so the
    gradients equal a run with keep bits off throughout."""
    sc = synthetic_scene(30000, 3, seed=5, scale_lo=0.005, scale_hi=0.06)
    cam = synthetic_camera(512, 384)
    bg = torch.tensor([0.2, 0.4, 0.6], device=gpu)
    gt = torch.rand(cam.height, cam.width, 3, generator=torch.Generator().manual_seed(3)).to(gpu)

    def run(flip):
        s = sc.to(gpu).requires_grad_()
        _lib.call("gsplat_debug_set_raster_variant", 1, 2, 1 << 30)
        out = render_fused(s, cam.to(gpu), 3, bg, return_alpha=True)
        if flip:
            _lib.call("gsplat_debug_set_raster_variant", 1, 2, 0)
        ((out["rgb"] - gt).abs().sum() + 0.1 * out["accumulation"].sum()).backward()
        return [p.grad.detach().cpu().numpy() for p in s.params()]
    try:
        _lib.call("gsplat_debug_set_chunk", 64)
        ref = run(False)
        got = run(True)
    finally:
        _lib.call("gsplat_debug_set_chunk", 0)
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
    for name, x, y in zip(("means", "scales", "quats", "opacities", "dc", "rest"), got, ref):
        np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("bwd", [1, 2], ids=["blocks8x8", "strips16x8"])
def test_list_modes_bit_identical_records(gpu, deterministic, bwd, hooks, oracle_lib):
    """The three list modes of one geometry -- the unsplit walk, the list split (chunk 64: five
    parts of the centre tile) and the list split on the forward's keep bits -- add the same
    per-wave totals, so the deterministic records (the four raster-level gradients) are equal bit
    for bit, on the tiny 40x48 scene of tests/structured_scenes.py (dispatch_cells)."""
    import structured_scenes as S
    s = S.dispatch_cells()
    bg = torch.from_numpy(s.state["bg"]).to(gpu)
    gen = torch.Generator().manual_seed(77)
    v_img = torch.randn(s.H, s.W, 3, generator=gen).to(gpu)
    v_alpha = torch.randn(s.H, s.W, generator=gen).to(gpu)
    got = {}
    try:
        for lists, (chunk, flags) in (("unsplit", (-1, 0)), ("split", (64, 1 << 30)),
                                      ("split-keep", (64, 0))):
            _lib.call("gsplat_debug_set_chunk", chunk)
            _lib.call("gsplat_debug_set_raster_variant", 1, bwd, flags)
            out = render_fused(s.scene.to(gpu).requires_grad_(), s.cam.to(gpu), 0, bg,
                               return_alpha=True, clamp=False)
            ((out["rgb"] * v_img).sum() + (out["accumulation"][..., 0] * v_alpha).sum()).backward()
            got[lists] = [g.detach().cpu().numpy() for g in out["raster_grads"]()]
    finally:
        _lib.call("gsplat_debug_set_chunk", 0)
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
    for lists in ("split", "split-keep"):
        for name, x, y in zip(("v_xy", "v_conic", "v_colors", "v_opacity"), got["unsplit"],
                              got[lists]):
            assert np.abs(x).max() > 0, name
            np.testing.assert_array_equal(y, x, err_msg=f"{lists} {name}")
