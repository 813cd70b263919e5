"""References of the splat-back tests (test infrastructure only), on the CPU oracle alone.

splat_back's sums are the forward's blend weights w = alpha T times the pixel values, summed
per Gaussian.  The oracle has no such entry, but its rasterize backward computes exactly that
sum as v_colors = sum alpha T v_out when it runs with the forward's alpha clamp: `oracle_sums`
is that call, in the oracle's float64 build, with the forward state of the same build.
`direct_sums` restates sum w v per pixel from the forward's decisions, without the backward's
transmittance recovery; tests/test_lift_host.py shows the two agree to 1e-12, and that the
backward's default clamp (0.99) would not.

The forward clamps alpha at the float constant 0.999f; the float64 build keeps float constants,
so the clamp handed to its backward is that constant, ALPHA_FWD -- the double 0.999 differs from
it by 1.3e-8, which the recovery T / (1 - alpha) magnifies a thousandfold.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import oracle as O
import structured_scenes as S
from gaussctrl_exp_amd.camera import synthetic_camera

ALPHA_FWD = float(np.float32(0.999))
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))


def _d(a):
    return np.ascontiguousarray(a, np.float64)


def seeded_values(H, W, C, seed=11):
    """values [H, W, C] ~ U(-1, 1): signed, so that a sign error cannot cancel."""
    return np.random.default_rng(seed + 7 * C).uniform(-1.0, 1.0, (H, W, C)).astype(np.float32)


def forward_state64(tb, H, W, gids, bins, xys, conics, opac):
    """(final_Ts, final_idx) of the float64 oracle forward (colours play no part in them)."""
    n = np.asarray(xys).shape[0]
    with O.float64():
        _, fT, fi = O.rasterize_forward(tb, H, W, gids, bins, _d(xys), _d(conics),
                                        np.zeros((n, 3)), _d(opac), np.zeros(3))
    return fT, fi


def oracle_sums(tb, H, W, gids, bins, xys, conics, opac, values, alpha_max=ALPHA_FWD):
    """(sums [N, 4], abs_sums [N, 4]) float64: the oracle backward's v_colors for v_out = values
    padded to three channels (columns < C) and for v_out = 1 (column 3, the weight), zero
    v_out_alpha, with their sums of |terms|."""
    values = np.asarray(values)
    if values.ndim == 2:
        values = values[..., None]
    C = values.shape[2]
    n = np.asarray(xys).shape[0]
    fT, fi = forward_state64(tb, H, W, gids, bins, xys, conics, opac)
    v3 = np.zeros((H, W, 3))
    v3[..., :C] = values
    out, ab = np.zeros((n, 4)), np.zeros((n, 4))
    with O.float64():
        for v, cols in ((v3, slice(0, 3)), (np.ones((H, W, 3)), slice(3, 4))):
            g, a = O.rasterize_backward(tb, H, W, gids, bins, _d(xys), _d(conics),
                                        np.zeros((n, 3)), _d(opac), np.zeros(3), fT, fi, v,
                                        np.zeros((H, W)), alpha_max=alpha_max, return_abs=True)
            width = cols.stop - cols.start
            out[:, cols], ab[:, cols] = g[2][:, :width], a[2][:, :width]
    return out, ab


def direct_sums(tb, H, W, gids, bins, xys, conics, opac, values):
    """sum over the composited pairs of w v, restated per pixel in float64 from the float64
    oracle forward's decisions: a pair is composited when sigma >= 0, alpha >= 1/255 and its
    list position is at most the pixel's final_idx; w = alpha * prod over the composited pairs
    before it of (1 - alpha)."""
    values = np.asarray(values, np.float64)
    if values.ndim == 2:
        values = values[..., None]
    C = values.shape[2]
    xys, conics, opac = _d(xys), _d(conics), _d(opac).reshape(-1)
    n = xys.shape[0]
    _, fi = forward_state64(tb, H, W, gids, bins, xys, conics, opac)
    tbx = int(tb[0])
    sums = np.zeros((n, 4))
    for t in range(tbx * int(tb[1])):
        lo, hi = (int(v) for v in bins[t])
        if hi <= lo:
            continue
        g = np.asarray(gids[lo:hi])
        i = np.arange((t // tbx) * 16, min((t // tbx) * 16 + 16, H))
        j = np.arange((t % tbx) * 16, min((t % tbx) * 16 + 16, W))
        dx = xys[g, 0][:, None, None] - j[None, None, :].astype(np.float64)
        dy = xys[g, 1][:, None, None] - i[None, :, None].astype(np.float64)
        a, b, c = (conics[g, k][:, None, None] for k in range(3))
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        alpha = np.minimum(ALPHA_FWD, opac[g][:, None, None] * np.exp(-sigma))
        k = np.arange(lo, hi)[:, None, None]
        comp = (sigma >= 0) & (alpha >= ALPHA_MIN) & (k <= fi[i[0]:i[-1] + 1, j[0]:j[-1] + 1][None])
        am = np.where(comp, alpha, 0.0)
        T_before = np.concatenate([np.ones_like(am[:1]), np.cumprod(1.0 - am, axis=0)[:-1]])
        w = am * T_before
        v = values[i[0]:i[-1] + 1, j[0]:j[-1] + 1]
        for ch in range(C):
            np.add.at(sums[:, ch], g, (w * v[None, :, :, ch]).sum((1, 2)))
        np.add.at(sums[:, 3], g, w.sum((1, 2)))
    return sums


def scene_sums(s, values, alpha_max=ALPHA_FWD):
    """oracle_sums of a structured scene (its oracle projection and binning)."""
    st = s.state
    return oracle_sums(s.cam.tile_bounds, s.H, s.W, st["gids"], st["bins"], st["xys"],
                       st["conics"], st["opac"], values, alpha_max)


# ---- the two-cluster scene of the mask-lifting tests --------------------------------------
THRESHOLD, MIN_WEIGHT = 0.5, 1e-3
BOUNDARY = 24  # the mask is the left half of a 48x48 frame: columns < 24


@functools.lru_cache(maxsize=None)
def two_clusters(seed=9):
    """A 48x48 scene under two cameras: two lattice clusters of 150 Gaussians left and right of
    x = 24 (every one farther than its radius from the boundary column) and 12 wider Gaussians
    straddling it; the mask of both views is the left half.  Returns dict(scene, cams, masks,
    states, left, right, straddle): states are the oracle's projection and binning per view."""
    cam0 = synthetic_camera(48, 48)
    cam1 = synthetic_camera(48, 48, eye=(0.0, 0.5, 4.0))
    rng = np.random.default_rng(seed)
    n_side, n_mid = 150, 12
    lx, ly = S._lattice(rng, n_side, 6.0, 17.0, 6.0, 42.0)
    rx, ry = S._lattice(rng, n_side, 31.0, 42.0, 6.0, 42.0)
    mx, my = S._lattice(rng, n_mid, 22.5, 25.5, 6.0, 42.0)
    n = 2 * n_side + n_mid
    z = rng.uniform(-0.1, 0.1, n)
    scale = np.r_[np.full(2 * n_side, S.SCALE), np.full(n_mid, 3 * S.SCALE)]
    rgb = rng.uniform(0.1, 0.9, (n, 3))
    sc = S.make_scene(cam0, np.r_[lx, rx, mx], np.r_[ly, ry, my], z, scale, 0.3, rgb)
    mask = np.zeros((48, 48), bool)
    mask[:, :BOUNDARY] = True
    idx = np.arange(n)
    return dict(scene=sc, cams=[cam0, cam1], masks=[mask, mask.copy()],
                states=[S.oracle_state(sc, cam) for cam in (cam0, cam1)],
                left=idx < n_side, right=(idx >= n_side) & (idx < 2 * n_side),
                straddle=idx >= 2 * n_side)


@functools.lru_cache(maxsize=None)
def two_clusters_reference():
    """(sums, abs_sums) [N, 4] float64 of the oracle over both views of two_clusters()."""
    tc = two_clusters()
    n = tc["scene"].num_points
    sums, ab = np.zeros((n, 4)), np.zeros((n, 4))
    for cam, mask, st in zip(tc["cams"], tc["masks"], tc["states"]):
        if st["fwd"]["num_intersects"] < 1:
            continue
        s, a = oracle_sums(cam.tile_bounds, cam.height, cam.width, st["gids"], st["bins"],
                           st["xys"], st["conics"], st["opac"], mask.astype(np.float32))
        sums += s
        ab += a
    return sums, ab


def sums_tensor(sums):
    return torch.from_numpy(np.ascontiguousarray(sums))
