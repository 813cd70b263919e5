"""gsplat_rasterize_splat_back, lift_masks and render_labels on the GPU vs the CPU oracle.

Reference (tests/lift_ref.py, shown on the host by tests/test_lift_host.py): the float64
oracle's rasterize backward v_colors with v_out = the pixel values padded to three channels, zero
v_out_alpha and the forward's alpha clamp -- and the same with v_out = 1 for the weight column.
Bar: 1e-5 + 1e-4 |ref| + 2^-20 sum|terms| per element, zero outliers (parity.assert_close with
abs_sum).  Nothing is divided, so there is no drift term; the structured scenes have no
marginal alpha decision, so there is no flip allowance.
"""
import numpy as np
import pytest
import torch

import lift_ref as R
import structured_scenes as S
from gaussctrl_exp_amd import _lib, lift
from gaussctrl_exp_amd.project_gaussians import project_gaussians
from gaussctrl_exp_amd.rasterize import rasterize_gaussians
from parity import ATOL, RTOL, assert_close

pytestmark = pytest.mark.gpu

ALL = S.all_scenes()
BY_ID = dict(ALL)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(gpu, a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu, dt)


_REF = {}


def _reference(s, C, seed=11):
    """(values, oracle sums, oracle sums of |terms|) of scene s, computed once and left alone."""
    key = (s.name, C, seed)
    if key not in _REF:
        values = R.seeded_values(s.H, s.W, C, seed)
        _REF[key] = (values,) + R.scene_sums(s, values)
    return _REF[key]


def _inputs(gpu, s):
    """The oracle's projection and binning of the scene on the device: both sides of every
    comparison walk the same lists."""
    st = s.state
    return dict(xys=_dev(gpu, st["xys"]), conics=_dev(gpu, st["conics"]),
                opacity=_dev(gpu, st["opac"]), gids=_dev(gpu, st["gids"], torch.int32),
                bins=_dev(gpu, st["bins"], torch.int32))


def _splat(gpu, s, values, out=None, d=None):
    d = d or _inputs(gpu, s)
    return lift.splat_back(d["xys"], d["conics"], d["opacity"], d["gids"], d["bins"],
                           _dev(gpu, values), s.H, s.W, out=out)


@pytest.fixture
def scene(request, oracle_lib):
    return BY_ID[request.param]()


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("scene", [name for name, _ in ALL], indirect=True)
def test_splat_back_matches_oracle(gpu, scene, channels):
    """sums [N, 4] of one call into a zeroed buffer: the value columns and the weight column
    (the oracle's v_colors for v_out = 1) within the bar; the unused value columns stay zero."""
    values, ref, absum = _reference(scene, channels)
    got = _np(_splat(gpu, scene, values))
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (got[:, channels:3] == 0).all()
    assert_close(f"{scene.name} C={channels} sums", got, ref, abs_sum=absum)


@pytest.mark.parametrize("scene", [name for name, _ in ALL], indirect=True)
def test_gpu_backward_colors_match(gpu, scene):
    """The route the sums could be had by before: the GPU's own forward + rasterize backward
    (C = 3, alpha_max = 0.999, zero v_output_alpha) gives v_colors within the same bar of the
    same reference."""
    s = scene
    values, ref, absum = _reference(s, 3)
    d = _inputs(gpu, s)
    n, H, W = d["xys"].shape[0], s.H, s.W
    tbx, tby = s.cam.tile_bounds[:2]
    P, st = _lib.ptr, _lib.stream(gpu)
    colors, bg = torch.zeros(n, 3, device=gpu), torch.zeros(3, device=gpu)
    img, fT = torch.empty(H, W, 3, device=gpu), torch.empty(H, W, device=gpu)
    fi = torch.empty(H, W, device=gpu, dtype=torch.int32)
    _lib.call("gsplat_rasterize_forward", tbx, tby, H, W, 3, P(d["gids"]), P(d["bins"]),
              P(d["xys"]), P(d["conics"]), P(colors), P(d["opacity"]), P(bg), P(img), P(fT),
              P(fi), st)
    g = [torch.empty(n, k, device=gpu) for k in (2, 3, 3, 1)]
    wsz = _lib.query("gsplat_rasterize_backward_workspace_size", n, 3)
    ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=gpu)
    _lib.call("gsplat_rasterize_backward", tbx, tby, H, W, 3, n, P(d["gids"]), P(d["bins"]),
              P(d["xys"]), P(d["conics"]), P(colors), P(d["opacity"]), P(bg), P(fT), P(fi),
              P(_dev(gpu, values)), None, R.ALPHA_FWD, *[P(x) for x in g], P(ws), wsz, st)
    assert_close(f"{s.name} backward v_colors", _np(g[2]), ref[:, :3], abs_sum=absum[:, :3])


@pytest.mark.parametrize("scene", ["dispatch_cells", "tiny_frame-17x17"], indirect=True)
def test_accumulates(gpu, scene):
    """Two calls into one buffer == the sum of two single calls (and of the two references)
    within the bar; a call over all-empty tile_bins leaves a pre-filled buffer bit-unchanged."""
    s = scene
    v1, ref1, ab1 = _reference(s, 3, seed=11)
    v2, ref2, ab2 = _reference(s, 3, seed=12)
    d = _inputs(gpu, s)
    a, b = _splat(gpu, s, v1, d=d), _splat(gpu, s, v2, d=d)
    both = _splat(gpu, s, v1, d=d)
    assert _splat(gpu, s, v2, out=both, d=d) is both
    assert_close(f"{s.name} two calls vs singles", _np(both),
                 _np(a).astype(np.float64) + _np(b).astype(np.float64), abs_sum=ab1 + ab2)
    assert_close(f"{s.name} two calls vs oracle", _np(both), ref1 + ref2, abs_sum=ab1 + ab2)
    gen = torch.Generator().manual_seed(3)
    filled = torch.randn(d["xys"].shape[0], 4, generator=gen).to(gpu)
    before = filled.clone()
    empty = dict(d, bins=torch.zeros_like(d["bins"]))
    assert _splat(gpu, s, v1, out=filled, d=empty) is filled
    assert torch.equal(filled, before)


def test_lift_masks_two_clusters(gpu, oracle_lib):
    tc = R.two_clusters()
    ref, absum = R.two_clusters_reference()
    want = lift.select(R.sums_tensor(ref), R.THRESHOLD, R.MIN_WEIGHT)
    sc = tc["scene"].to(gpu)
    cams = [c.to(gpu) for c in tc["cams"]]
    masks = [torch.from_numpy(m).to(gpu) for m in tc["masks"]]
    # the kernels see the scene whose reference the oracle computed
    for cam, st in zip(cams, tc["states"]):
        with torch.no_grad():
            xys = project_gaussians(sc.means, torch.exp(sc.scales), 1,
                                    sc.quats / sc.quats.norm(dim=-1, keepdim=True),
                                    *cam.project_args())[0]
        np.testing.assert_array_equal(_np(xys), st["xys"])
    sums = _np(lift.lift_sums(sc, cams, masks))
    assert_close("two clusters sums", sums, ref, abs_sum=absum)
    res = lift.lift_masks(sc, cams, masks, R.THRESHOLD, R.MIN_WEIGHT)
    # bool, uint8 and float masks are one mask
    for conv in (lambda m: m.to(torch.uint8), lambda m: m.float()):
        other = lift.lift_masks(sc, cams, [conv(m) for m in masks], R.THRESHOLD, R.MIN_WEIGHT)
        assert torch.equal(other.selected, res.selected)
    score, weight, sel = _np(res.score), _np(res.weight), _np(res.selected)
    w_ref, s_ref = want.weight.numpy(), want.score.numpy()
    assert_close("two clusters weight", weight, w_ref, abs_sum=absum[:, 3])
    # score = a / b with a, b inside their bars: |d(a / b)| <= (tol_a + |a / b| tol_b) / b
    seen = w_ref > R.MIN_WEIGHT
    tol_a = ATOL + RTOL * np.abs(ref[:, 0]) + 2.0 ** -20 * absum[:, 0]
    tol_b = ATOL + RTOL * np.abs(ref[:, 3]) + 2.0 ** -20 * absum[:, 3]
    tol_s = (tol_a + np.abs(s_ref) * tol_b) / np.where(seen, w_ref, 1.0)
    ratio = np.abs(score - s_ref)[seen] / tol_s[seen]
    print(f"[parity] two clusters score: worst diff/allowed {ratio.max():.3f}")
    assert (ratio <= 1.0).all()
    clear = np.abs(s_ref - R.THRESHOLD) > 1e-3
    np.testing.assert_array_equal(sel[clear], want.selected.numpy()[clear])
    # no Gaussian of the right cluster (all farther than their radius from the boundary,
    # tests/test_lift_host.py) is selected; the left cluster is
    assert not sel[tc["right"]].any() and sel[tc["left"]].all()


def test_lift_masks_skips_empty_view(gpu, oracle_lib):
    """A view that sees nothing (the camera turned away from the scene: every Gaussian is behind
    it, an empty binning) is skipped; the other view's sums are its single-call sums."""
    from gaussctrl_exp_amd.camera import gc_camera, look_at_c2w
    tc = R.two_clusters()
    sc = tc["scene"].to(gpu)
    cam0 = tc["cams"][0]
    cam, mask = cam0.to(gpu), torch.from_numpy(tc["masks"][0]).to(gpu)
    away = gc_camera(look_at_c2w((0.0, 0.0, 4.0), target=(0.0, 0.0, 8.0), up=(0.0, 1.0, 0.0)),
                     cam0.fx, cam0.fy, cam0.cx, cam0.cy, 48, 48).to(gpu)
    ref, absum = R.oracle_sums(cam0.tile_bounds, 48, 48, *(tc["states"][0][k] for k in (
        "gids", "bins", "xys", "conics", "opac")), tc["masks"][0].astype(np.float32))
    both = _np(lift.lift_sums(sc, [away, cam, away], [mask, mask, mask]))
    assert_close("one seeing view of three", both, ref, abs_sum=absum)
    assert not lift.lift_sums(sc, [away], [mask]).any()


def test_render_labels_bit_equal(gpu, oracle_lib):
    tc = R.two_clusters()
    sc, cam = tc["scene"].to(gpu), tc["cams"][0].to(gpu)
    n = sc.num_points
    gen = torch.Generator().manual_seed(5)
    for labels in (torch.rand(n, generator=gen).to(gpu), torch.rand(n, 2, generator=gen).to(gpu),
                   torch.from_numpy(tc["left"]).to(gpu)):
        got = lift.render_labels(sc, cam, labels)
        lab2 = labels[:, None] if labels.dim() == 1 else labels
        C = lab2.shape[1]
        padded = torch.zeros(n, 3, device=gpu)
        padded[:, :C] = lab2.float()
        with torch.no_grad():
            xys, depths, radii, conics, nth, _ = project_gaussians(
                sc.means, torch.exp(sc.scales), 1,
                sc.quats / sc.quats.norm(dim=-1, keepdim=True), *cam.project_args())
            want = rasterize_gaussians(xys, depths, radii, conics, nth, padded,
                                       torch.sigmoid(sc.opacities), cam.height, cam.width,
                                       background=torch.zeros(3, device=gpu))
        assert got.shape == (cam.height, cam.width, C)
        assert torch.equal(got, want[..., :C])
    # the left cluster's labels light the left half only
    img = _np(lift.render_labels(sc, cam, torch.from_numpy(tc["left"]).to(gpu)))[..., 0]
    assert img[:, :20].max() > 0.1 and img[:, 28:].max() == 0.0


def test_error_paths(gpu, oracle_lib):
    s = S.tiny_frame(17, 17)
    d = _inputs(gpu, s)
    args = lambda v, **kw: (kw.get("xys", d["xys"]), d["conics"], d["opacity"], d["gids"],
                            d["bins"], v, s.H, s.W)
    for C in (0, 4):
        with pytest.raises(ValueError):
            lift.splat_back(*args(torch.zeros(s.H, s.W, C, device=gpu)))
    with pytest.raises(ValueError):
        lift.splat_back(*args(torch.zeros(s.H + 1, s.W, 1, device=gpu)))
    with pytest.raises(ValueError):
        lift.splat_back(*args(torch.zeros(s.H, s.W, 1, device=gpu)),
                        out=torch.zeros(3, 4, device=gpu))
    with pytest.raises(RuntimeError):  # CPU tensors: no CPU path
        lift.splat_back(*args(torch.zeros(s.H, s.W, 1)))
    with pytest.raises(RuntimeError):
        lift.splat_back(*args(torch.zeros(s.H, s.W, 1, device=gpu), xys=d["xys"].cpu()))
    with pytest.raises(RuntimeError):  # non-contiguous values
        lift.splat_back(*args(torch.zeros(s.H, s.W, 6, device=gpu)[..., ::2]))
    # the C entry itself rejects a channel count outside 1..3
    P = _lib.ptr
    v = torch.zeros(s.H, s.W, 4, device=gpu)
    out = torch.zeros(d["xys"].shape[0], 4, device=gpu)
    for C in (0, 4):
        with pytest.raises(RuntimeError):
            _lib.call("gsplat_rasterize_splat_back", 2, 2, s.H, s.W, C, P(d["gids"]),
                      P(d["bins"]), P(d["xys"]), P(d["conics"]), P(d["opacity"]), P(v), P(out),
                      _lib.stream(gpu))
    assert not out.any()
