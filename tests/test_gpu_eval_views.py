"""The eval render of a batch of views on the MI355X (fused.render_fused_eval_views): one fused
preprocess over V cameras, one binning and one RGB+depth blend with the eval epilogue over the
views' tile grids stacked along y.

The reference is fused.render_fused_eval per camera, and equality is np.testing.
assert_array_equal: every view of a batch is the single-view render bit for bit (rgb, depth,
accumulation, radii, xys), whatever else shares the batch.  One view is also held against the
CPU oracle's caller chain at the project's bar, so the file does not lean on the GPU single-view
path alone.
"""
import math

import numpy as np
import pytest
import torch

from gaussctrl_exp_amd.camera import gc_camera, look_at_c2w, synthetic_camera
from gaussctrl_exp_amd.fused import render_fused, render_fused_eval, render_fused_eval_views
from gaussctrl_exp_amd.rasterize import BUCKET_MAX_N, bin_gaussians
from gaussctrl_exp_amd.scene import render, synthetic_scene

pytestmark = pytest.mark.gpu

# 8.5 x 12.5 tiles: a partial tile row and a partial tile column, so a row stride of tby * 16
# where H belongs shows up
W, H = 200, 136
TBX, TBY = (W + 15) // 16, (H + 15) // 16
N = 3000
EYES = ((0.0, 0.0, 4.0), (1.5, 0.5, 3.5), (-1.0, 1.0, 3.8))
BG = (0.2, 0.4, 0.6)


def _np(t):
    return t.detach().cpu().numpy()


def _cams(gpu, eyes=EYES, w=W, h=H):
    return [synthetic_camera(w, h, eye=e).to(gpu) for e in eyes]


def _away_camera(gpu, w=W, h=H):
    """At (0, 0, 4) looking away from the scene (extent 1.5 around the origin): every Gaussian
    is behind it."""
    fx = 0.5 * w / math.tan(math.radians(50.0) / 2)
    c2w = look_at_c2w((0.0, 0.0, 4.0), target=(0.0, 0.0, 8.0), up=(0.0, 1.0, 0.0))
    return gc_camera(c2w, fx, fx, w / 2.0, h / 2.0, w, h).to(gpu)


def _single(sc, cam, deg, bg):
    """render_fused_eval as numpy; a view that sees nothing (depth None) as the batch's
    documented fill: background / 0 / 1000."""
    r = render_fused_eval(sc, cam, deg, bg)
    h, w = cam.height, cam.width
    if r["depth"] is None:
        return {"rgb": _np(r["rgb"]), "depth": np.full((h, w, 1), 1000.0, np.float32),
                "accumulation": np.zeros((h, w, 1), np.float32), "xys": _np(r["xys"]),
                "radii": _np(r["radii"]), "empty": True}
    out = {k: _np(r[k]) for k in ("rgb", "depth", "accumulation", "xys", "radii")}
    out["empty"] = False
    return out


def _assert_views_equal(batch, refs, views=None):
    for v, ref in enumerate(refs):
        if views is not None and v not in views:
            continue
        for k in ("rgb", "depth", "accumulation", "radii", "xys"):
            np.testing.assert_array_equal(_np(batch[k][v]), ref[k], err_msg=f"view {v} {k}")


@pytest.fixture(scope="module")
def bg(gpu):
    return torch.tensor(BG, device=gpu)


@pytest.fixture(scope="module")
def base(gpu, bg):
    """The K = 16 scene, its three cameras and their single-view renders at degree 3 (computed
    once, shared, never modified)."""
    sc = synthetic_scene(N, 3, seed=5, scale_lo=0.01, scale_hi=0.05, device=gpu)
    cams = _cams(gpu)
    refs = [_single(sc, c, 3, bg) for c in cams]
    assert all((r["accumulation"] > 0).mean() > 0.3 for r in refs)
    assert all((r["depth"] == 1000).any() and (r["depth"] < 1000).any() for r in refs)
    return sc, cams, refs


@pytest.mark.parametrize("sh_degree,deg", [(3, 3), (3, 0), (0, 0), (4, 4)],
                         ids=["K16@3", "K16@0", "K1", "K25@4"])
def test_batch_equals_single_views(gpu, bg, base, sh_degree, deg):
    if (sh_degree, deg) == (3, 3):
        sc, cams, refs = base
    else:
        sc = synthetic_scene(N, sh_degree, seed=5, scale_lo=0.01, scale_hi=0.05, device=gpu)
        cams = _cams(gpu)
        refs = [_single(sc, c, deg, bg) for c in cams]
    out = render_fused_eval_views(sc, cams, deg, bg)
    assert out["rgb"].shape == (3, H, W, 3) and out["depth"].shape == (3, H, W, 1)
    assert out["accumulation"].shape == (3, H, W, 1)
    assert out["radii"].shape == (3, N) and out["radii"].dtype == torch.int32
    assert out["xys"].shape == (3, N, 2)
    _assert_views_equal(out, refs)
    # the views differ from one another: a batch that repeated one view would not pass
    assert np.abs(refs[0]["rgb"] - refs[1]["rgb"]).max() > 0.05


def test_footprints_across_the_seam(gpu, bg):
    """Radii of several tiles: footprints reach past a view's last tile row, which on the
    stacked grid is the next view's first.  The box is clamped to the view's own rows before the
    offset, so every view still equals its single render."""
    sc = synthetic_scene(N, 3, seed=6, scale_lo=0.05, scale_hi=0.3, device=gpu)
    cams = _cams(gpu)
    refs = [_single(sc, c, 3, bg) for c in cams]
    for r in refs[:2]:  # (views with a view stacked below them)
        vis = r["radii"] > 0
        y, rad = r["xys"][:, 1], r["radii"].astype(np.float32)
        assert rad[vis].max() >= 48  # several tiles
        lo_row, hi = np.floor((y - rad) / 16), (y + rad) / 16 + 1
        in_last_row = vis & (lo_row <= TBY - 1) & (hi >= TBY)
        assert in_last_row.any()  # a single-view tile box that touches the last tile row
        assert (vis & (hi > TBY)).any()  # ... and one the clamp cuts at the view's bottom
    out = render_fused_eval_views(sc, cams, 3, bg)
    _assert_views_equal(out, refs)


def test_empty_view_in_the_middle(gpu, bg, base):
    sc, cams, refs = base
    away = _away_camera(gpu)
    ref_away = _single(sc, away, 3, bg)
    assert ref_away["empty"] and (ref_away["radii"] == 0).all()
    out = render_fused_eval_views(sc, [cams[0], away, cams[2]], 3, bg, return_state=True)
    _assert_views_equal(out, [refs[0], ref_away, refs[2]])
    np.testing.assert_array_equal(_np(out["rgb"][1]),
                                  np.broadcast_to(np.float32(BG), (H, W, 3)))
    assert (_np(out["accumulation"][1]) == 0).all() and (_np(out["depth"][1]) == 1000).all()
    assert out["state"][0]["blended"]


def test_all_empty_batch_needs_no_blend(gpu, bg, base):
    sc = base[0]
    away = _away_camera(gpu)
    out = render_fused_eval_views(sc, [away, away], 3, bg, return_state=True)
    assert [s["num_intersects"] for s in out["state"]] == [0]
    assert not out["state"][0]["blended"]
    np.testing.assert_array_equal(_np(out["rgb"]),
                                  np.broadcast_to(np.float32(BG), (2, H, W, 3)))
    assert (_np(out["accumulation"]) == 0).all() and (_np(out["depth"]) == 1000).all()
    assert (_np(out["radii"]) == 0).all()


def test_one_view_and_a_repeated_view(gpu, bg, base):
    sc, cams, refs = base
    one = render_fused_eval_views(sc, cams[1:2], 3, bg)
    _assert_views_equal(one, refs[1:2])
    # the same camera twice: equal depths across the views (ties broken by the virtual id)
    two = render_fused_eval_views(sc, [cams[0], cams[0]], 3, bg)
    _assert_views_equal(two, [refs[0], refs[0]])


def test_backgrounds_and_intrinsics(gpu, base):
    sc, cams, _ = base
    bgs = torch.tensor([[0.2, 0.4, 0.6], [1.0, 0.0, 0.5], [0.0, 0.0, 0.0]], device=gpu)
    out = render_fused_eval_views(sc, cams, 3, bgs)
    _assert_views_equal(out, [_single(sc, c, 3, bgs[v]) for v, c in enumerate(cams)])
    shared = bgs[1].clone()
    out = render_fused_eval_views(sc, cams, 3, shared)
    _assert_views_equal(out, [_single(sc, c, 3, shared) for c in cams])
    # different focal lengths and principal points in one batch
    varied = []
    for k, eye in enumerate(EYES):
        fx = 0.5 * W / math.tan(math.radians(40.0 + 10.0 * k) / 2)
        c2w = look_at_c2w(eye, up=(0.0, 1.0, 0.0))
        varied.append(gc_camera(c2w, fx, 1.1 * fx, W / 2.0 + 7.5 * k, H / 2.0 - 3.25 * k, W,
                                H).to(gpu))
    out = render_fused_eval_views(sc, varied, 3, shared)
    refs = [_single(sc, c, 3, shared) for c in varied]
    _assert_views_equal(out, refs)
    assert np.abs(refs[0]["rgb"] - refs[2]["rgb"]).max() > 0.05


def test_chunked_equals_unchunked(gpu, bg, base):
    sc, cams, refs = base
    out = render_fused_eval_views(sc, cams, 3, bg, max_points=2 * N, return_state=True)
    assert [s["views"] for s in out["state"]] == [(0, 2), (2, 3)]
    whole = render_fused_eval_views(sc, cams, 3, bg)
    for k in ("rgb", "depth", "accumulation", "radii", "xys"):
        np.testing.assert_array_equal(_np(out[k]), _np(whole[k]))
    _assert_views_equal(out, refs)


def test_binning_scheme_crossing(gpu, bg):
    """N = 50,000: a single view bins with the small-scene tile buckets, the batch of three
    (150,000 points > 131,072) with the depth sort + tile sort."""
    n = 50000
    assert n <= BUCKET_MAX_N < 3 * n
    sc = synthetic_scene(n, 3, seed=8, scale_lo=0.005, scale_hi=0.02, device=gpu)
    cams = _cams(gpu, w=64, h=48)
    refs = [_single(sc, c, 3, bg) for c in cams]
    out = render_fused_eval_views(sc, cams, 3, bg)
    _assert_views_equal(out, refs)


def test_staging_variant_crossing(gpu, bg):
    """1,225 tiles per view: a single view's blend stages pipelined (below 3,584 tiles), the
    batch of three (3,675 stacked tiles) plainly -- the batch kernel's other instantiation."""
    w = h = 560
    assert (w // 16) * (h // 16) < 3584 <= 3 * (w // 16) * (h // 16)
    sc = synthetic_scene(N, 3, seed=9, scale_lo=0.01, scale_hi=0.05, device=gpu)
    cams = _cams(gpu, w=w, h=h)
    refs = [_single(sc, c, 3, bg) for c in cams]
    out = render_fused_eval_views(sc, cams, 3, bg)
    _assert_views_equal(out, refs)


def test_lists_equal_the_single_view_binning(gpu, bg, base):
    sc, cams, _ = base
    out = render_fused_eval_views(sc, cams, 3, bg, return_state=True)
    (st,) = out["state"]
    gids, bins = _np(st["gaussian_ids_sorted"]), _np(st["tile_bins"])
    tiles = TBX * TBY
    assert bins.shape == (3 * tiles, 2)
    for v, cam in enumerate(cams):
        with torch.no_grad():
            r = render_fused(sc, cam, 3, bg)["raster_inputs"]
        num, ref_ids, ref_bins = bin_gaussians(r["xys"], r["depths"], r["radii"],
                                               r["num_tiles_hit"], H, W)
        assert num > 0
        mine = bins[v * tiles:(v + 1) * tiles]
        lo, hi = int(mine[:, 0].min()), int(mine[:, 1].max())
        assert hi - lo == num
        np.testing.assert_array_equal(gids[lo:hi] - v * N, _np(ref_ids))
        # an empty tile's entry is (0, 0) in both tables; the others shift by the view's base
        ref_bins = _np(ref_bins)
        empty = ref_bins[:, 0] == ref_bins[:, 1]
        np.testing.assert_array_equal(mine[~empty] - lo, ref_bins[~empty])
        assert (mine[empty, 0] == mine[empty, 1]).all()


def test_one_view_against_the_cpu_oracle(gpu, bg, base, oracle_lib):
    """View 1 of the batch vs the CPU oracle's caller chain (scene.render on the oracle-backed
    gsplat API, two rasterize calls for the depth): the project's bar, zero outliers."""
    import oracle_gsplat as OG
    from parity import assert_close
    sc, cams, _ = base
    out = render_fused_eval_views(sc, cams, 3, bg)
    with torch.no_grad():
        ref = render(sc.to("cpu"), cams[1].to("cpu"), 3, bg.cpu(), return_depth=True, api=OG)
    for k in ("rgb", "accumulation", "depth"):
        assert_close(f"batch view 1 {k} vs oracle", _np(out[k][1]), _np(ref[k]))
