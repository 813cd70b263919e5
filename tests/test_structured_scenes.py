"""The structured scenes (tests/structured_scenes.py) on the CPU oracle alone.

For every scene: its preconditions hold (the list lengths, word offsets, empty windows, early
exits ... the GPU tests rely on, none of which they assert themselves); the oracle's float
build -- the checker the GPU tests use -- agrees with its double build at the project bar on
image, alpha and the four raster-level gradients (1e-5 + 1e-4 |ref|, plus the fp32 summation
slack 2^-20 sum|terms| and the transmittance-recovery drift for the gradients, tests/parity.py),
so the reference alone stays within the bar on these inputs; and the flip cap: at most 5 % of
the pixels meet a threshold decision within 1e-5 (parity.near_threshold_pixel) and at most 5 %
of the gradient elements carry a non-zero oracle flip_sum, so the threshold-flip allowance
cannot hide a failure in tests/test_gpu_structured.py.
"""
import numpy as np
import pytest
import torch

import structured_scenes as S

SCENES = S.all_scenes()
FLIP_CAP = 0.05


def _d(a):
    return np.asarray(a, np.float64)


@pytest.fixture(params=[mk for _, mk in SCENES], ids=[name for name, _ in SCENES])
def scene(request, oracle_lib):
    return request.param()


def test_preconditions(scene):
    print(f"[scene] {scene.name}: {scene.info}")
    failed = [k for k, ok in scene.pre.items() if not ok]
    assert not failed, (scene.name, failed, scene.info)


def _upstream(H, W, seed=77):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(H, W, 3, generator=gen).numpy(), torch.randn(H, W, generator=gen).numpy())


def test_float_oracle_matches_double_oracle(scene, oracle_lib):
    O = oracle_lib
    from parity import assert_close, drift_slack
    st, H, W = scene.state, scene.H, scene.W
    f = st["fwd"]
    with O.float64():
        f64 = O.render_forward(_d(st["xys"]), _d(st["depths"]), st["radii"], _d(st["conics"]),
                               st["nth"], _d(st["colors"]), _d(st["opac"]), H, W, _d(st["bg"]))
    np.testing.assert_array_equal(f["gaussian_ids_sorted"], f64["gaussian_ids_sorted"])
    np.testing.assert_array_equal(f["final_idx"], f64["final_idx"])
    assert_close(f"{scene.name} img", f["img"], f64["img"])
    assert_close(f"{scene.name} alpha", f["alpha"], f64["alpha"])
    v_img, v_alpha = _upstream(H, W)
    got32, absum, drift, _ = O.rasterize_backward(
        f["tile_bounds"], H, W, st["gids"], st["bins"], st["xys"], st["conics"], st["colors"],
        st["opac"], st["bg"], f["final_Ts"], f["final_idx"], v_img, v_alpha, return_abs=True,
        return_drift=True, return_flip=True)
    with O.float64():
        got64 = O.render_backward(f64, _d(st["xys"]), _d(st["conics"]), _d(st["colors"]),
                                  _d(st["opac"]), _d(st["bg"]), _d(v_img), _d(v_alpha))
    for k, name in enumerate(("v_xy", "v_conic", "v_colors", "v_opacity")):
        assert_close(f"{scene.name} {name}", got32[k], got64[k], abs_sum=absum[k],
                     extra=drift_slack(drift[k]).reshape(got64[k].shape))


def near_threshold_map(st, H, W, alpha_max=0.999, rel=1e-5):
    """parity.near_threshold_pixel for every pixel at once: the same float32 expressions, over
    [list, rows, columns] arrays per tile (the transmittance as a sequential float32 product)."""
    f = np.float32
    tbx = (W + 15) // 16
    out = np.zeros((H, W), bool)
    for t in range(tbx * ((H + 15) // 16)):
        alpha, sigma, i, j = S.pair_alpha(st, t, tbx, H, W)
        if not alpha.shape[0]:
            continue
        alpha = np.minimum(f(alpha_max), alpha)
        a64 = alpha.astype(np.float64)
        near = ((np.abs(sigma.astype(np.float64)) <= 1e-6) & (a64 >= 1 / 255)) | \
            (np.abs(a64 * 255.0 - 1.0) <= rel)
        skip = (sigma < 0) | (alpha < f(1.0 / 255.0))
        fac = np.where(skip, f(1.0), f(1.0) - alpha).astype(f)
        # T after each position had the walk not stopped: exact up to the first stop, where the
        # walk ends (later positions are masked out below)
        nT = np.cumprod(fac, axis=0, dtype=f)
        near |= ~skip & (np.abs(nT.astype(np.float64) / 1e-4 - 1.0) <= rel)
        stop = ~skip & (nT <= f(1e-4))
        # positions up to and including the first stop are the walk's
        walked = np.cumsum(stop, axis=0) - stop == 0
        out[i[0]:i[-1] + 1, j[0]:j[-1] + 1] = (near & walked).any(0)
    return out


def test_flip_cap(scene, oracle_lib):
    O = oracle_lib
    from parity import near_threshold_pixel
    st, H, W = scene.state, scene.H, scene.W
    f = st["fwd"]
    tbx = (W + 15) // 16
    near = near_threshold_map(st, H, W)
    # the vectorised walk is parity.near_threshold_pixel: every flagged pixel and a sample of
    # the others, through the function itself
    rng = np.random.default_rng(0)
    flagged = [tuple(p) for p in np.argwhere(near)[:8]]
    others = np.argwhere(~near)
    sample = [tuple(p) for p in others[rng.choice(len(others), min(6, len(others)),
                                                  replace=False)]] if len(others) else []
    for i, j in flagged + sample:
        assert near_threshold_pixel(int(i), int(j), st["xys"], st["conics"], st["opac"],
                                    st["gids"], st["bins"], tbx) == bool(near[i, j]), (i, j)
    share = float(near.mean())
    v_img, v_alpha = _upstream(H, W)
    _, flip = O.rasterize_backward(
        f["tile_bounds"], H, W, st["gids"], st["bins"], st["xys"], st["conics"], st["colors"],
        st["opac"], st["bg"], f["final_Ts"], f["final_idx"], v_img, v_alpha, return_flip=True)
    nz = sum(int(np.count_nonzero(a)) for a in flip)
    total = sum(a.size for a in flip)
    print(f"[flip] {scene.name}: {int(near.sum())} of {near.size} pixels near a threshold "
          f"({share:.2%}), {nz} of {total} gradient elements with a flip sum ({nz / total:.2%})")
    assert share <= FLIP_CAP, (scene.name, share)
    assert nz / total <= FLIP_CAP, (scene.name, nz / total)
