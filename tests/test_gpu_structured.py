"""The blend kernels on the structured scenes (tests/structured_scenes.py) vs the CPU oracle.

The scenes put the rasterizer's list-position logic on its edges: tile lists of 63 .. 8,200
positions at range.x = 0, 1, 63 (mod 64) (keep words, the 4,096-position windows of the kept
walk), a block whose walk crosses a whole window without a kept position, pixels that end at
their second position next to pixels that walk the whole list, equal depth keys, frames
smaller than a tile, and alphas below 1/255 or on the clamp.  Their preconditions are asserted
on the CPU (tests/test_structured_scenes.py), together with the flip cap that keeps the
threshold-flip allowance out of these comparisons; here every comparison is the existing bar
of tests/parity.py (1e-5 + 1e-4 |ref|, zero outliers; raster-level gradients with the fp32
summation slack and the recovery drift), with no tolerance of its own.

Two callers: rasterize_gaussians on the oracle's (bit-exact) projection of the scene -- the
gsplat API's backward kernels -- and render_fused on the scene itself: the clearing forward that
fills the list-split plan and the keep bits, and the record backward that walks them.  The keep
bits exist only behind a plan-filling forward, so the geometry x keep-bits x determinism
product runs on both callers.
"""
import numpy as np
import pytest
import torch

import oracle as O
import structured_scenes as S
from gaussctrl_exp_amd import _lib, quirks
from gaussctrl_exp_amd.fused import render_fused
from gaussctrl_exp_amd.rasterize import bin_gaussians, rasterize_gaussians
from gaussctrl_exp_amd.scene import render
from parity import (assert_close, assert_close_or_flip, assert_raster_close, check_raster_level,
                    gpu_forward_state, injected_api)

pytestmark = pytest.mark.gpu

BIN_SETTINGS = {"shipped": -1, "tilesort": 0, "bucket": 1}  # gsplat_debug_binning_scheme
GRADS = ("v_xy", "v_conic", "v_colors", "v_opacity")
NAMES = ["means", "scales", "quats", "opacities", "features_dc", "features_rest"]

ALL = S.all_scenes()
BY_ID = dict(ALL)
# the whole geometry x keep-bits x determinism product: the lists past a 4,096 window, the
# empty window, the divergent exits; every other scene: as shipped plus one alternative
FULL = [f"deep_tile-{L}-{lead}" for L, lead in S.DEEP_FULL] + ["sparse_windows", "early_exit"]
REST = [name for name, _ in ALL if name not in FULL]
BINNED = [name for name, _ in ALL if name.startswith("deep_tile")] + ["sparse_windows",
                                                                      "depth_ties"]
SPLIT = [f"deep_tile-8200-{lead}" for lead in (0, 1, 63)] + ["sparse_windows"]


def _np(t):
    return t.detach().cpu().numpy()


def _upstream(H, W, scale=1.0):
    gen = torch.Generator().manual_seed(77)
    return scale * torch.randn(H, W, 3, generator=gen), scale * torch.randn(H, W, generator=gen)


@pytest.fixture
def scene(request, oracle_lib):
    return BY_ID[request.param]()


def _inputs(s):
    st = s.state
    return dict(xys=st["xys"], depths=st["depths"], radii=st["radii"], conics=st["conics"],
                num_tiles_hit=st["nth"], colors=st["colors"], opacity=st["opac"])


_REF = {}


def _reference(gpu, key, r, bg, H, W):
    """The oracle's rasterize backward (with its abs / drift / flip sums) on the GPU's own
    forward state for raster inputs r, computed once per scene, caller and alpha clamp and left
    unchanged: no backward variant changes the forward state."""
    key = (key, quirks.backward_alpha_clamp())
    if key not in _REF:
        v_img, v_alpha = _upstream(H, W)
        fs = gpu_forward_state(gpu, r["xys"], r["depths"], r["radii"], r["conics"],
                               r["num_tiles_hit"], r["colors"], r["opacity"], bg, H, W)
        _REF[key] = O.rasterize_backward(
            fs["tile_bounds"], H, W, fs["gids"], fs["bins"], r["xys"], r["conics"], r["colors"],
            np.asarray(r["opacity"]).reshape(-1), bg, fs["final_Ts"], fs["final_idx"],
            v_img.numpy(), v_alpha.numpy(), alpha_max=quirks.backward_alpha_clamp(),
            return_abs=True, return_drift=True, return_flip=True)
    return _REF[key]


def _assert_raster(label, got, ref4):
    ref, absum, drift, flip = ref4
    for k, name in enumerate(GRADS):
        a = np.asarray(got[k], np.float64).reshape(ref[k].shape)
        assert_raster_close(f"{label} {name}", a, ref[k], absum[k], drift[k], flip[k])


def _assert_forward(label, s, img, alpha):
    st, f = s.state, s.state["fwd"]
    tbx = s.cam.tile_bounds[0]
    assert img.shape == (s.H, s.W, 3) and alpha.shape == (s.H, s.W)
    assert np.isfinite(img).all() and np.isfinite(alpha).all(), f"{label}: non-finite output"
    for name, got, ref in (("img", img, f["img"]), ("alpha", alpha[..., None],
                                                    f["alpha"][..., None])):
        assert_close_or_flip(f"{label} {name}", got, ref, st["xys"], st["conics"], st["opac"],
                             st["gids"], st["bins"], tbx)
        # (worst diff / allowed of the pixels inside the bar)
        tol = 1e-5 + 1e-4 * np.abs(ref)
        print(f"[parity] {label} {name}: worst diff/allowed "
              f"{float((np.abs(got - ref) / tol).max()):.3f}")


def _caller(gpu, s):
    """rasterize_gaussians (the gsplat API) on the oracle's projection of the scene: image,
    alpha and the four raster-level gradients for the shared random upstream gradients."""
    r = _inputs(s)
    d = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(gpu, dt)
    v_img, v_alpha = _upstream(s.H, s.W)
    xy, cn = d(r["xys"]).requires_grad_(), d(r["conics"]).requires_grad_()
    col, op = d(r["colors"]).requires_grad_(), d(r["opacity"])[:, None].requires_grad_()
    img, alpha = rasterize_gaussians(
        xy, d(r["depths"]), d(r["radii"], torch.int32), cn, d(r["num_tiles_hit"], torch.int32),
        col, op, s.H, s.W, d(s.state["bg"]), return_alpha=True)
    ((img * v_img.to(gpu)).sum() + (alpha * v_alpha.to(gpu)).sum()).backward()
    return _np(img), _np(alpha), [_np(t.grad) for t in (xy, cn, col, op)]


def _fused(gpu, s, scale=1.0):
    """render_fused on the scene (SH degree 0): image, alpha, the record backward's four
    raster-level gradients, the six parameter gradients and the rasterizer's inputs / state."""
    sc = s.scene.to(gpu).requires_grad_()
    v_img, v_alpha = _upstream(s.H, s.W, scale)
    out = render_fused(sc, s.cam.to(gpu), 0, torch.from_numpy(s.state["bg"]).to(gpu),
                       return_alpha=True, clamp=False)
    img, acc = out["rgb"], out["accumulation"]
    ((img * v_img.to(gpu)).sum() + (acc[..., 0] * v_alpha.to(gpu)).sum()).backward()
    r = {k: _np(v) for k, v in out["raster_inputs"].items()}
    # the scene the kernels saw is the one whose preconditions the CPU test asserted
    st = s.state
    for k, ref in (("xys", st["xys"]), ("depths", st["depths"]), ("radii", st["radii"]),
                   ("num_tiles_hit", st["nth"])):
        np.testing.assert_array_equal(r[k], ref, err_msg=k)
    return dict(img=_np(img), alpha=_np(acc)[..., 0], raster=[_np(g) for g in out["raster_grads"]()],
                params=[_np(p.grad) for p in sc.params()], inputs=r,
                state={k: (_np(v) if torch.is_tensor(v) else v)
                       for k, v in out["raster_state"].items()},
                num_intersects=out["num_intersects"])


def _check_both_callers(gpu, s, label):
    """Forward and raster-level backward parity of both callers under the current switches;
    returns the gradients (for bit-identity checks between switch settings)."""
    img, alpha, got = _caller(gpu, s)
    _assert_forward(f"{label} caller", s, img, alpha)
    _assert_raster(f"{label} caller", got, _reference(gpu, (s.name, "caller"), _inputs(s),
                                                      s.state["bg"], s.H, s.W))
    fz = _fused(gpu, s)
    _assert_forward(f"{label} fused", s, fz["img"], fz["alpha"])
    _assert_raster(f"{label} fused", fz["raster"], _reference(gpu, (s.name, "fused"), fz["inputs"],
                                                              s.state["bg"], s.H, s.W))
    return got, fz["raster"]


# ---- binning ---------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", list(BIN_SETTINGS))
@pytest.mark.parametrize("scene", BINNED, indirect=True)
def test_binning_bitexact(gpu, scene, scheme, hooks):
    """bin_gaussians under every scheme: bit-exact vs the oracle's stable sort (4,096+ equal
    tile keys in one tile; depth_ties: equal depth keys as well, the order is by id)."""
    st = scene.state
    d = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(gpu, dt)
    prev = hooks.gsplat_debug_binning_scheme(BIN_SETTINGS[scheme])
    try:
        I, gids, bins = bin_gaussians(d(st["xys"]), d(st["depths"]), d(st["radii"], torch.int32),
                                      d(st["nth"], torch.int32), scene.H, scene.W)
    finally:
        hooks.gsplat_debug_binning_scheme(prev)
    assert I == st["fwd"]["num_intersects"]
    np.testing.assert_array_equal(_np(gids), st["gids"])
    np.testing.assert_array_equal(_np(bins), st["bins"])


@pytest.mark.parametrize("scene", BINNED, indirect=True)
def test_fused_binning_bitexact(gpu, scene):
    """render_fused's binning -- the first call of a frame shape (synchronous), then the
    speculative one launched at the learned capacity -- bit-exact vs the oracle."""
    st = scene.state
    modes = []
    for _ in range(2):
        with torch.no_grad():
            out = render_fused(scene.scene.to(gpu), scene.cam.to(gpu), 0,
                               torch.from_numpy(st["bg"]).to(gpu), return_alpha=True)
        rs = out["raster_state"]
        modes.append(rs["binning"])
        assert out["num_intersects"] == st["fwd"]["num_intersects"]
        np.testing.assert_array_equal(_np(rs["gaussian_ids_sorted"])[:out["num_intersects"]],
                                      st["gids"])
        np.testing.assert_array_equal(_np(rs["tile_bins"]), st["bins"])
    print(f"[binning] {scene.name}: {modes}")
    assert modes[1] in ("speculative", "host"), modes


# ---- the product: geometry x keep bits x determinism, both callers ----------------------------

@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("bwd", [1, 2], ids=["blocks8x8", "strips16x8"])
@pytest.mark.parametrize("scene", FULL, indirect=True)
def test_backward_geometries_keep_bits(gpu, scene, bwd, det, hooks):
    """Both backward geometries, keep bits on and off (debug flag bit 30), the atomic and the
    deterministic accumulation, at the shipped chunk: forward and the four raster-level
    gradients of both callers vs the oracle; deterministic: keep bits on == off bit for bit."""
    prev = _lib.set_deterministic(det)
    grads = {}
    try:
        for keep, flags in (("on", 0), ("off", 1 << 30)):
            _lib.call("gsplat_debug_set_raster_variant", 1, bwd, flags)
            grads[keep] = _check_both_callers(gpu, scene, f"{scene.name} bwd{bwd} keep-{keep}")
    finally:
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
        _lib.set_deterministic(prev)
    if det:
        for caller, on, off in zip(("caller", "fused"), grads["on"], grads["off"]):
            for name, x, y in zip(GRADS, on, off):
                assert np.abs(x).max() > 0, (caller, name)
                np.testing.assert_array_equal(x, y, err_msg=f"{caller} {name}")


@pytest.mark.parametrize("scene", REST, indirect=True)
def test_backward_shipped(gpu, scene):
    """The other scenes as shipped (the shipped library, no switch set), both callers."""
    assert not _lib.hooks_active()
    _check_both_callers(gpu, scene, f"{scene.name} shipped")


@pytest.mark.parametrize("scene", REST, indirect=True)
def test_backward_alternative(gpu, scene, hooks):
    """The other scenes once more on the 16x8 strips with a forced chunk of 64 (lists of 63 /
    64 / 65 end on a part boundary) in the deterministic mode."""
    prev = _lib.set_deterministic(True)
    try:
        _lib.call("gsplat_debug_set_chunk", 64)
        _lib.call("gsplat_debug_set_raster_variant", 1, 2, 0)
        _check_both_callers(gpu, scene, f"{scene.name} strips chunk64 det")
    finally:
        _lib.call("gsplat_debug_set_chunk", 0)
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
        _lib.set_deterministic(prev)


# ---- every cell of the backward's kernel dispatch ---------------------------------------------

# list mode -> (gsplat_debug_set_chunk, raster-variant flags): the keep bits exist only behind
# render_fused's plan-filling forward (the gsplat API caller's split walks without them)
LIST_MODES = {"unsplit": (-1, 0), "split": (64, 1 << 30), "split-keep": (64, 0)}


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("lists", list(LIST_MODES))
@pytest.mark.parametrize("bwd", [1, 2], ids=["blocks8x8", "strips16x8"])
@pytest.mark.parametrize("scene", ["dispatch_cells"], indirect=True)
def test_backward_dispatch_cells(gpu, scene, bwd, lists, det, hooks):
    """{8x8 blocks, 16x8 strips} x {unsplit, split, split + keep bits} x {atomic, deterministic}
    on the tiny 40x48 scene (a forced chunk of 64: five parts of the centre tile): forward and
    the four raster-level gradients of both callers vs the oracle.  (The pair-count
    instantiations of the same cells: tests/test_gpu_pair_count.py; bit-identity of the
    deterministic records across the list modes: tests/test_gpu_deterministic.py.)"""
    chunk, flags = LIST_MODES[lists]
    prev = _lib.set_deterministic(det)
    try:
        _lib.call("gsplat_debug_set_chunk", chunk)
        _lib.call("gsplat_debug_set_raster_variant", 1, bwd, flags)
        _check_both_callers(gpu, scene, f"{scene.name} bwd{bwd} {lists}")
    finally:
        _lib.call("gsplat_debug_set_chunk", 0)
        _lib.call("gsplat_debug_set_raster_variant", 1, 0, 0)
        _lib.set_deterministic(prev)


# ---- the shipped split plan, unforced -----------------------------------------------------------

@pytest.mark.parametrize("scene", SPLIT, indirect=True)
def test_shipped_split_plan_unforced(gpu, scene):
    """One deep tile among near-empty ones: the shipped chunk (gsplat_rasterize_chunk_size, no
    override, the shipped library) splits the tile into more than four parts; same parity."""
    tb = scene.cam.tile_bounds
    I = scene.state["fwd"]["num_intersects"]
    chunk = _lib.query("gsplat_rasterize_chunk_size", tb[0], tb[1], I)
    L = scene.info["list_len"]
    print(f"[split] {scene.name}: list {L}, shipped chunk {chunk}: {-(-L // chunk)} parts")
    assert chunk > 0 and L > 4 * chunk
    assert not _lib.hooks_active()
    _check_both_callers(gpu, scene, f"{scene.name} shipped plan")


# ---- the fused path end to end ----------------------------------------------------------------

# The scenes' opacities (0.005 .. 0.0072, so that thousands of positions composite without a
# pixel terminating) make a Gaussian's gradients ~1e-3 of a random scene's: upstream gradients of
# N(0, 1000^2) bring the parameter gradients back to O(1), where the bar's absolute 1e-5 cannot
# hide a wrong one and the degenerate-reference guard (> 1e-3) means what it does in test_gpu_fused
UPSTREAM_SCALE = 1000.0

@pytest.mark.parametrize("quirk_mask", [7, 0], indirect=True)
@pytest.mark.parametrize("scene", [name for name, _ in ALL], indirect=True)
def test_fused_render_grads_match_oracle(gpu, scene, quirk_mask):
    """render_fused forward and backward: the records vs the oracle's rasterize backward on
    the same forward state (check_raster_level), image, alpha and the six parameter gradients vs
    the oracle caller chain fed those raster gradients (test_gpu_fused's pattern)."""
    s = scene
    fz = _fused(gpu, s, UPSTREAM_SCALE)
    r = fz["inputs"]
    v_img, v_alpha = _upstream(s.H, s.W, UPSTREAM_SCALE)
    check_raster_level(gpu, r["xys"], r["depths"], r["radii"], r["conics"], r["num_tiles_hit"],
                       r["colors"], r["opacity"], s.state["bg"], s.H, s.W, v_img.numpy(),
                       v_alpha.numpy(), fz["raster"], label=f"{s.name} ")
    sc = s.scene.detach().requires_grad_()
    out = render(sc, s.cam, 0, torch.from_numpy(s.state["bg"]), api=injected_api(fz["raster"]))
    (out["rgb"].sum() + out["accumulation"].sum()).backward()  # (upstream replaced anyway)
    ref = [_np(out["rgb"]), _np(out["accumulation"])[..., 0]] + [_np(p.grad) for p in sc.params()]
    got = [fz["img"], fz["alpha"]] + fz["params"]
    _assert_forward(f"{s.name} fused", s, fz["img"], fz["alpha"])
    # an isotropic covariance does not depend on its rotation (v_quat == 0), below_threshold
    # composites nothing (every gradient is zero: test_below_threshold_exact), and clamped's
    # opacity logits of 20 sit where the sigmoid's slope is 2e-9
    isotropic = bool((s.scene.scales == s.scene.scales[:, :1]).all())
    for i, name in enumerate(["rgb", "alpha"] + NAMES):
        assert np.isfinite(got[i]).all(), f"{name}: non-finite values"
        if got[i].size and i >= 2 and s.name != "below_threshold" and \
                not (name == "quats" and isotropic) and \
                not (name == "opacities" and s.name == "clamped"):
            assert np.abs(ref[i]).max() > 1e-3, f"{name}: degenerate reference gradient"
        if i >= 2:
            assert_close(f"{s.name} {name}", got[i], ref[i])


# ---- exact results ------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["below_threshold"], indirect=True)
def test_below_threshold_exact(gpu, scene):
    """Every opacity below 1/255: lists are walked, nothing is composited -- the image is
    exactly the background, alpha exactly 0 and every gradient exactly 0, on both callers."""
    bg = scene.state["bg"]
    img, alpha, got = _caller(gpu, scene)
    fz = _fused(gpu, scene)
    assert fz["num_intersects"] == scene.state["fwd"]["num_intersects"] > 0
    for label, im, al, grads in (("caller", img, alpha, got),
                                 ("fused", fz["img"], fz["alpha"], fz["raster"] + fz["params"])):
        assert (im == bg[None, None]).all(), label
        assert not al.any(), label
        for k, g in enumerate(grads):
            assert not np.asarray(g).any(), (label, k)


@pytest.mark.parametrize("scene", [f"tiny_frame-{W}x{H}" for W, H in S.TINY_SIZES],
                         indirect=True)
def test_tiny_frame_shapes(gpu, scene):
    """Frames smaller than a tile or a block: [H, W, 3] / [H, W] outputs without a NaN, in the
    image, alpha and every gradient (parity: test_backward_shipped / _alternative)."""
    img, alpha, got = _caller(gpu, scene)
    fz = _fused(gpu, scene)
    for im, al, grads in ((img, alpha, got), (fz["img"], fz["alpha"], fz["raster"] + fz["params"])):
        assert im.shape == (scene.H, scene.W, 3) and al.shape == (scene.H, scene.W)
        assert np.isfinite(im).all() and np.isfinite(al).all()
        assert all(np.isfinite(np.asarray(g)).all() for g in grads)
