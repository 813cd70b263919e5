"""Structured scenes for the blend kernels' list-walk edges (test infrastructure only).

synthetic_scene draws uniform random Gaussians, so every tile list is about as long as the mean
and the rasterizer's position-indexed logic (64-position keep words, 4,096-position windows, the
list-split plan, lane-divergent exits) meets its edges only by accident.  The builders here
construct those edges on purpose.  Every scene is a GaussianScene in 3D under
synthetic_camera(W, H) (axis-aligned, eye (0, 0, 4)): a pixel position (px, py) at depth d
is the mean ((px + 0.5 - cx) d / f, -(py + 0.5 - cy) d / f, 4 - d), identity quaternions,
isotropic scales and SH degree 0 unless the scene needs otherwise -- so the same scene feeds
rasterize_gaussians (through the oracle's bit-exact projection) and render_fused.

Each builder returns a Structured: the scene, the camera, and `pre`, a dict of preconditions
(name -> bool) evaluated from the CPU oracle alone (project_forward, bin_and_sort,
render_forward); `info` holds the measured figures behind them.  The GPU tests assert nothing
about a scene's shape themselves: tests/test_structured_scenes.py asserts `pre` on the CPU.

Positions lie on a half-pixel lattice offset by a quarter pixel (px = k / 2 + 1 / 4), and the
lattice scenes share one scale: every (Gaussian, pixel) pair's sigma is then one of a few
discrete levels (r^2 = 1/8 + m / 2 px^2), and the opacities are chosen so that 1/255 falls
between two levels with >= 10 % to spare.  No alpha decision is marginal, which is what keeps
the threshold-flip allowance of tests/parity.py out of these comparisons (the flip cap).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

import oracle as O
from gaussctrl_exp_amd.camera import synthetic_camera
from gaussctrl_exp_amd.scene import GaussianScene

ALPHA_MIN = 1.0 / 255.0
SCALE = 0.05           # the lattice scenes' isotropic scale (~0.64 px at depth 4 on 48x48)
DEEP_OPACITY = 0.0072  # 1/255 between the r^2 = 5/8 and 9/8 levels, >= 10 % from both
BACKGROUND = np.array([0.3, 0.6, 0.9], np.float32)


@dataclass
class Structured:
    name: str
    scene: GaussianScene
    cam: object
    pre: dict
    info: dict = field(default_factory=dict)
    state: dict = field(default_factory=dict)  # the oracle's projection / forward (shared)

    @property
    def W(self):
        return self.cam.width

    @property
    def H(self):
        return self.cam.height


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p))


def make_scene(cam, px, py, z, scale, opacity=None, rgb=None, opacity_logit=None):
    """The GaussianScene of Gaussians at pixel positions (px, py), world height z (depth 4 - z),
    world scale `scale` ([n] isotropic or [n, 3]), opacity (or its logit) and colour rgb."""
    px, py, z = (np.asarray(a, np.float64) for a in (px, py, z))
    n = px.shape[0]
    d = 4.0 - z
    means = np.stack([(px + 0.5 - cam.cx) * d / cam.fx, -(py + 0.5 - cam.cy) * d / cam.fy, z], 1)
    scale = np.asarray(scale, np.float64)
    scale = np.broadcast_to(scale.reshape(-1, 1) if scale.ndim < 2 else scale, (n, 3))
    if opacity_logit is None:
        opacity_logit = _logit(np.broadcast_to(np.asarray(opacity, np.float64), (n,)))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    quats = np.zeros((n, 4))
    quats[:, 0] = 1.0
    return GaussianScene(t(means), t(np.log(scale)), t(quats),
                         t(np.asarray(opacity_logit).reshape(n, 1)), t(_logit(rgb)),
                         torch.zeros(n, 0, 3))


def oracle_state(scene, cam, background=BACKGROUND):
    """The oracle's view of a scene: the caller's activations (scene.render: exp, normalise,
    sigmoid), project_forward, and render_forward (binning + blend)."""
    scales = torch.exp(scene.scales).numpy()
    quats = (scene.quats / scene.quats.norm(dim=-1, keepdim=True)).numpy()
    opac = torch.sigmoid(scene.opacities).numpy().reshape(-1)
    colors = torch.sigmoid(scene.features_dc).numpy()
    xys, depths, radii, conics, nth, _ = O.project_forward(
        scene.means.numpy(), scales, 1.0, quats, cam.viewmat.numpy(), cam.projmat.numpy(),
        cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, cam.tile_bounds)
    fwd = O.render_forward(xys, depths, radii, conics, nth, colors, opac, cam.height, cam.width,
                           background)
    return dict(xys=xys, depths=depths, radii=radii, conics=conics, nth=nth, colors=colors,
                opac=opac, bg=np.asarray(background, np.float32), fwd=fwd,
                gids=fwd["gaussian_ids_sorted"], bins=fwd["tile_bins"])


def pair_alpha(st, tile, tbx, H, W):
    """(alpha [L, h, w] of the tile's list positions at the tile's pixels: opacity exp(-sigma)
    in float32 as the oracle evaluates it, unclamped; sigma; the pixel rows i and columns j)."""
    f = np.float32
    lo, hi = (int(v) for v in st["bins"][tile])
    g = st["gids"][lo:hi]
    i = np.arange((tile // tbx) * 16, min((tile // tbx) * 16 + 16, H))
    j = np.arange((tile % tbx) * 16, min((tile % tbx) * 16 + 16, W))
    dx = (st["xys"][g, 0].astype(f)[:, None, None] - j.astype(f)[None, None, :])
    dy = (st["xys"][g, 1].astype(f)[:, None, None] - i.astype(f)[None, :, None])
    a, b, c = (st["conics"][g, k].astype(f)[:, None, None] for k in range(3))
    sigma = f(0.5) * (a * dx * dx + c * dy * dy) + b * dx * dy
    alpha = st["opac"][g].astype(f)[:, None, None] * np.exp(-sigma, dtype=f)
    return alpha, sigma, i, j


def touches_rect(st, g, rx0, rx1, ry0, ry1):
    """csrc/raster.hip's touches_rect restated in float64 for Gaussians g against the
    pixel-centre rectangle [rx0, rx1] x [ry0, ry1]: False only where the per-pixel test
    rejects the Gaussian at every pixel of the rectangle (with the kernel's rounding margin)."""
    gx, gy = st["xys"][g, 0].astype(np.float64), st["xys"][g, 1].astype(np.float64)
    a, b, c = (st["conics"][g, k].astype(np.float64) for k in range(3))
    o = st["opac"][g].astype(np.float64)
    dx0, dx1, dy0, dy1 = gx - rx1, gx - rx0, gy - ry1, gy - ry0

    def q_edge(e, lo, hi, diag_e, diag_f):
        fm = np.clip(-b * e / diag_f, lo, hi)
        t0, t1, t2 = diag_e * e * e, 2.0 * b * e * fm, diag_f * fm * fm
        return t0 + t1 + t2, t0 + np.abs(t1) + t2
    qs = [q_edge(dx0, dy0, dy1, a, c), q_edge(dx1, dy0, dy1, a, c),
          q_edge(dy0, dx0, dx1, c, a), q_edge(dy1, dx0, dx1, c, a)]
    q = np.stack([v[0] for v in qs])
    m = np.stack([v[1] for v in qs])
    k = q.argmin(0)
    q, m = np.take_along_axis(q, k[None], 0)[0], np.take_along_axis(m, k[None], 0)[0]
    sigma_lb = 0.5 * (q - 1e-5 * m) - 1e-3
    inside = (dx0 <= 0) & (dx1 >= 0) & (dy0 <= 0) & (dy1 >= 0)
    pd = (a > 0) & (a * c - b * b > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        far = sigma_lb > np.log(255.0 * o)
    return (o >= ALPHA_MIN) & (~pd | inside | ~far)


def _lattice(rng, n, x0, x1, y0, y1):
    """n positions on the quarter-offset half-pixel lattice inside [x0, x1] x [y0, y1]."""
    xs = np.arange(math.ceil((x0 - 0.25) * 2), math.floor((x1 - 0.25) * 2) + 1) / 2 + 0.25
    ys = np.arange(math.ceil((y0 - 0.25) * 2), math.floor((y1 - 0.25) * 2) + 1) / 2 + 0.25
    return rng.choice(xs, n), rng.choice(ys, n)


def _margin(alpha):
    """The smallest relative distance of an alpha from 1/255."""
    return float(np.abs(alpha.astype(np.float64) * 255.0 - 1.0).min()) if alpha.size else 1.0


CENTRE = 4  # the centre tile of a 48x48 frame (3x3 tiles): pixels 16..31


def _deep(L, lead, seed, z_spread=0.1, opacity=DEEP_OPACITY, name=None):
    cam = synthetic_camera(48, 48)
    rng = np.random.default_rng(seed)
    # radius 3-4 px: centres in [20.5, 26.5] keep every box inside the centre tile
    px, py = _lattice(rng, L, 20.5, 26.5, 20.5, 26.5)
    lx, ly = _lattice(rng, lead, 5.0, 10.0, 5.0, 10.0)  # tile 0 only
    n = L + lead
    z = rng.uniform(-z_spread, z_spread, n) if z_spread else np.zeros(n)
    rgb = rng.uniform(0.1, 0.9, (n, 3))
    sc = make_scene(cam, np.r_[px, lx], np.r_[py, ly], z, np.full(n, SCALE), opacity, rgb)
    st = oracle_state(sc, cam)
    f = st["fwd"]
    lo, hi = (int(v) for v in st["bins"][CENTRE])
    alpha, _, _, _ = pair_alpha(st, CENTRE, 3, 48, 48)
    tile = (slice(16, 32), slice(16, 32))
    info = dict(list_len=hi - lo, range_x=lo, final_T_min=float(f["final_Ts"][tile].min()),
                final_idx_max=int(f["final_idx"][tile].max()), alpha_margin=_margin(alpha),
                num_intersects=int(f["num_intersects"]))
    pre = {"centre tile list length == L": hi - lo == L,
           "range.x % 64 == lead % 64": lo % 64 == lead % 64,
           "all visible, one tile each": bool((st["nth"] == 1).all()),
           "alphas >= 10 % from 1/255": info["alpha_margin"] >= 0.1}
    return Structured(name or f"deep_tile({L},{lead})", sc, cam, pre, info, st), tile, lo, hi


@functools.lru_cache(maxsize=None)
def deep_tile(L, lead, seed=0):
    """L small low-opacity Gaussians inside the centre tile of a 48x48 frame (no pixel
    terminates: every pixel walks the whole list), behind `lead` Gaussians in tile 0 that shift
    the centre tile's range.x to lead (mod 64)."""
    s, tile, lo, hi = _deep(L, lead, seed)
    s.pre["final_Ts > 1e-3 over the tile"] = s.info["final_T_min"] > 1e-3
    s.pre["final_idx max == range.y - 1"] = s.info["final_idx_max"] == hi - 1
    return s


@functools.lru_cache(maxsize=None)
def depth_ties(seed=1):
    """deep_tile(1000, 0) with every z equal (all depth keys identical: the order inside the tile
    is the stable sort's, by id) and opacity 0.34, random colours, so the order shows."""
    s, tile, lo, hi = _deep(1000, 0, seed, z_spread=0.0, opacity=0.34, name="depth_ties")
    st = s.state
    s.pre["depth bit patterns identical"] = np.unique(st["depths"].view(np.uint32)).size == 1
    gids = st["gids"].copy()
    gids[lo:hi] = gids[lo:hi][::-1]
    rev, _, _ = O.rasterize_forward((3, 3, 1), 48, 48, gids, st["bins"], st["xys"], st["conics"],
                                    st["colors"], st["opac"], st["bg"])
    img = st["fwd"]["img"]
    ratio = np.abs(rev - img) / (1e-5 + 1e-4 * np.abs(img))
    s.info["reversed_order_ratio"] = float(ratio.max())
    s.pre["reversed id order changes the image > 100x the bar"] = ratio.max() > 100.0
    return s


@functools.lru_cache(maxsize=None)
def sparse_windows(seed=2):
    """One tile (the centre of 48x48) whose list is 40 + 4,300 + 4,096 positions by depth: a few
    front Gaussians over the bottom-right 8x8 block, then 4,300 over the top-left block only, then
    4,000 over the bottom-right block only.  The bottom-right block's walk down from its last
    position crosses one whole aligned 4,096-position window without a kept position before it
    reaches the front ones; the top-left block ends > 4,096 positions below it."""
    cam = synthetic_camera(48, 48)
    rng = np.random.default_rng(seed)
    n_front, n_tl, n_br = 40, 4300, 4096
    # boxes (radius 4) inside the centre tile: centres in [20, 28); reach < 1 px, so a centre
    # >= 2 px inside its block touches no other block
    fx_, fy_ = _lattice(rng, n_front, 26.0, 28.0, 26.0, 28.0)
    tx_, ty_ = _lattice(rng, n_tl, 20.0, 22.0, 20.0, 22.0)
    bx_, by_ = _lattice(rng, n_br, 26.0, 28.0, 26.0, 28.0)
    z = np.r_[rng.uniform(0.08, 0.1, n_front), rng.uniform(-0.02, 0.06, n_tl),
              rng.uniform(-0.1, -0.04, n_br)]  # nearer = larger z
    n = z.size
    rgb = rng.uniform(0.1, 0.9, (n, 3))
    # 1/255 between the r^2 = 1/8 and 5/8 levels: only the four nearest sites composite, so
    # ~270 Gaussians per site leave T ~ 0.01
    sc = make_scene(cam, np.r_[fx_, tx_, bx_], np.r_[fy_, ty_, by_], z, np.full(n, SCALE), 0.0048,
                    rgb)
    st = oracle_state(sc, cam)
    f = st["fwd"]
    lo, hi = (int(v) for v in st["bins"][CENTRE])
    g = st["gids"][lo:hi]
    kept_tl = touches_rect(st, g, 16.0, 23.0, 16.0, 23.0)
    kept_br = touches_rect(st, g, 24.0, 31.0, 24.0, 31.0)
    kept_other = touches_rect(st, g, 24.0, 31.0, 16.0, 23.0) | \
        touches_rect(st, g, 16.0, 23.0, 24.0, 31.0)
    top_br = int(f["final_idx"][24:32, 24:32].max())
    top_tl = int(f["final_idx"][16:24, 16:24].max())
    # the walk's windows: 4,096 positions each, aligned at the block's last position
    wins = []
    for wtop in range(top_br, lo - 1, -4096):
        wlo = max(wtop - 4095, lo)
        wins.append((wtop - wlo + 1, int(kept_br[wlo - lo:wtop - lo + 1].sum())))
    empty_then_some = any(size == 4096 and cnt == 0 and any(c > 0 for _, c in wins[k + 1:])
                          for k, (size, cnt) in enumerate(wins))
    alpha, _, _, _ = pair_alpha(st, CENTRE, 3, 48, 48)
    info = dict(list_len=hi - lo, windows_bottom_right=wins, top_bottom_right=top_br,
                top_top_left=top_tl, alpha_margin=_margin(alpha),
                final_T_min=float(f["final_Ts"][16:32, 16:32].min()),
                num_intersects=int(f["num_intersects"]))
    pre = {"list length >= 8200": hi - lo >= 8200 and hi - lo == n,
           "all visible, one tile each": bool((st["nth"] == 1).all()),
           "first positions touch the expected blocks only":
               bool(kept_br[:n_front].all() and not kept_tl[:n_front].any() and
                    kept_tl[n_front:n_front + n_tl].all() and
                    not kept_br[n_front:n_front + n_tl].any() and
                    kept_br[n_front + n_tl:].all() and not kept_tl[n_front + n_tl:].any() and
                    not kept_other.any()),
           "bottom-right: an empty whole window, then a window with kept positions":
               empty_then_some,
           "top-left ends >= 4096 positions below bottom-right": top_br - top_tl >= 4096,
           "alphas >= 10 % from 1/255": info["alpha_margin"] >= 0.1,
           "no pixel terminates": info["final_T_min"] > 1e-3}
    return Structured("sparse_windows", sc, cam, pre, info, st)


@functools.lru_cache(maxsize=None)
def early_exit(seed=3):
    """A deep tile of 1,500 low-opacity Gaussians (over its right 7 columns) behind two stacked opaque Gaussians (opacity
    logit 20: sigmoid == 1.0f; anisotropic, tens of pixels wide) centred on the left 8 columns
    of the centre tile.  One alpha clamps at 0.999 and leaves T = 1e-3 > 1e-4, so it takes
    both to end a pixel: where both reach alpha >= 0.99 -- the left 8 columns, i.e. the two
    left 8x8 blocks entirely -- the pixel ends at its second position, while the right half of
    every 16-pixel row walks to the end of the list (kmax0 != kmax1 in every strip).  A Gaussian
    profile has no sharp edge, so the deep pixels' transmittance is 1e-4 .. 3e-3 here: the
    image and v_opacity stay well above the bar's absolute term, v_xy / v_conic / v_colors of
    the deep list are small."""
    cam = synthetic_camera(48, 48)
    rng = np.random.default_rng(seed)
    L = 1500
    px, py = _lattice(rng, L, 24.5, 31.0, 16.5, 31.0)  # (boxes spill into the tiles around)
    z = rng.uniform(-0.1, 0.1, L)
    # sigma <= 0.01 at the corners (dx 3.5, dy 7.5) of the left 8 columns: var >= dx^2 / 0.01
    # per axis, with 10 % to spare
    pix = cam.fx / 3.5  # px per world unit at depth 3.5
    sx, sy = math.sqrt(1.1 * 3.5 ** 2 / 0.01) / pix, math.sqrt(1.1 * 7.5 ** 2 / 0.01) / pix
    scale = np.r_[np.tile([[sx, sy, SCALE]], (2, 1)), np.full((L, 3), SCALE)]
    logit = np.r_[[20.0, 20.0], _logit(np.full(L, DEEP_OPACITY))]
    rgb = rng.uniform(0.1, 0.9, (L + 2, 3))
    sc = make_scene(cam, np.r_[[19.5, 19.5], px], np.r_[[23.5, 23.5], py],
                    np.r_[[0.5, 0.5], z], scale, rgb=rgb, opacity_logit=logit)
    st = oracle_state(sc, cam)
    f = st["fwd"]
    lo, hi = (int(v) for v in st["bins"][CENTRE])
    fi = f["final_idx"][16:32, 16:32]
    early, deep = fi <= lo + 2, fi >= lo + 500
    both = lambda a, b: bool(a.any() and b.any())
    strips = [both(early[r:r + 4], deep[r:r + 4]) for r in range(0, 16, 4)]
    blocks = [both(early[r:r + 8, c:c + 8], deep[r:r + 8, c:c + 8])
              for r in (0, 8) for c in (0, 8)]
    info = dict(list_len=hi - lo, range_x=lo, early_pixels=int(early.sum()),
                deep_pixels=int(deep.sum()), mixed_strips=int(sum(strips)),
                mixed_blocks=int(sum(blocks)),
                deep_T=(float(f["final_Ts"][16:32, 16:32][deep].min()) if deep.any() else 0.0,
                        float(f["final_Ts"][16:32, 16:32][deep].max()) if deep.any() else 0.0))
    pre = {"opaque opacity == 1.0f": bool((st["opac"][:2] == np.float32(1.0)).all()),
           "deep list of >= 600": hi - lo >= 600 + 2,
           "the opaque two lead the tile's list": set(st["gids"][lo:lo + 2]) == {0, 1},
           "covered (left 8 columns): final_idx <= range.x + 2": bool(early[:, :8].all()),
           "whole 8x8 blocks end at once": bool(early[:8, :8].all() and early[8:, :8].all()),
           ">= 64 pixels walk >= 500 positions": int(deep.sum()) >= 64,
           "a 16x4 strip holds both kinds": any(strips),
           "an 8x8 block holds both kinds": any(blocks)}
    return Structured("early_exit", sc, cam, pre, info, st)


TINY_SIZES = [(1, 1), (1, 17), (17, 1), (15, 15), (16, 16), (17, 17), (8, 24)]


@functools.lru_cache(maxsize=None)
def tiny_frame(W, H, seed=4):
    """~200 Gaussians over a frame smaller than (or just past) a tile or a block."""
    cam = synthetic_camera(W, H)
    rng = np.random.default_rng(seed + 31 * W + H)
    n = 200
    px, py = _lattice(rng, n, -0.5, W - 0.5, -0.5, H - 0.5)
    z = rng.uniform(-0.02, 0.02, n)
    rgb = rng.uniform(0.1, 0.9, (n, 3))
    sc = make_scene(cam, px, py, z, np.full(n, SCALE), 0.3, rgb)
    st = oracle_state(sc, cam)
    f = st["fwd"]
    tb = cam.tile_bounds
    comp = 0
    for t in range(tb[0] * tb[1]):
        alpha, sigma, i, j = pair_alpha(st, t, tb[0], H, W)
        lo = int(st["bins"][t][0])
        k = np.arange(lo, lo + alpha.shape[0])[:, None, None]
        ok = (alpha >= np.float32(ALPHA_MIN)) & (sigma >= 0) & \
            (k <= f["final_idx"][i[0]:i[-1] + 1, j[0]:j[-1] + 1][None])
        comp = max(comp, int(ok.sum(0).max()))
    info = dict(num_intersects=int(f["num_intersects"]), max_composited=comp)
    pre = {"num_intersects > 0": f["num_intersects"] > 0,
           "some pixel composites >= 3": comp >= 3}
    return Structured(f"tiny_frame({W},{H})", sc, cam, pre, info, st)


@functools.lru_cache(maxsize=None)
def below_threshold(seed=5):
    """500 Gaussians of opacity 0.003 (0.765 / 255) on 32x32: listed, walked, never composited."""
    cam = synthetic_camera(32, 32)
    rng = np.random.default_rng(seed)
    n = 500
    px, py = rng.uniform(2, 30, n), rng.uniform(2, 30, n)
    sc = make_scene(cam, px, py, rng.uniform(-0.1, 0.1, n), np.full(n, SCALE), 0.003,
                    rng.uniform(0.1, 0.9, (n, 3)))
    st = oracle_state(sc, cam)
    f = st["fwd"]
    info = dict(num_intersects=int(f["num_intersects"]),
                opacity_times_255=float(st["opac"].max()) * 255)
    pre = {"listed": f["num_intersects"] >= n,
           "opacity >= 10 % below 1/255": info["opacity_times_255"] <= 0.9,
           "nothing composited: final_idx == 0": not f["final_idx"].any(),
           "image == background": bool((f["img"] == st["bg"][None, None]).all()),
           "alpha == 0": not f["alpha"].any()}
    return Structured("below_threshold", sc, cam, pre, info, st)


@functools.lru_cache(maxsize=None)
def clamped(seed=6):
    """300 Gaussians of opacity exactly 1.0f whose projected centres are exact pixel centres
    (sigma == 0 there, computed exactly by any implementation) on 32x32, ~16 px wide: around its
    centre a Gaussian's alpha sits on the forward's 0.999 and the backward's 0.99 clamp.  The
    nearest few end every pixel, so the sigma == 0 pairs that are ever composited are few."""
    cam = synthetic_camera(32, 32)
    rng = np.random.default_rng(seed)
    n = 300
    px = rng.integers(2, 30, n).astype(np.float64)
    py = rng.integers(2, 30, n).astype(np.float64)
    z = rng.uniform(-0.1, 0.1, n)
    scale = np.full(n, 16.0 * 4.0 / cam.fx)
    rgb = rng.uniform(0.1, 0.9, (n, 3))
    sc = make_scene(cam, px, py, z, scale, rgb=rgb, opacity_logit=np.full(n, 20.0))
    # the projection rounds: step the means by 2^-23 until the oracle's xys are the integers
    # (one step moves a centre by ~1e-6 px, half an ulp of the pixel coordinate); a centre no
    # step reaches gets another depth and tries again
    target = np.stack([px, py], 1).astype(np.float32)
    means = sc.means.numpy().copy()
    for _ in range(50):
        base = means.copy()
        done = oracle_state_xys(sc, cam) == target
        for k in sorted(range(-32, 33), key=abs):
            if done.all():
                break
            trial = means.copy()
            trial[:, :2] = np.where(done, means[:, :2],
                                    base[:, :2].astype(np.float64) + k * 2.0 ** -23)
            sc.means = torch.from_numpy(trial.astype(np.float32))
            hit = (oracle_state_xys(sc, cam) == target) & ~done
            means[:, :2] = np.where(hit, trial[:, :2], means[:, :2])
            done |= hit
        redo = ~done.all(1)
        if not redo.any():
            break
        z[redo] = rng.uniform(-0.1, 0.1, int(redo.sum()))
        fresh = make_scene(cam, px, py, z, scale, rgb=rgb, opacity_logit=np.full(n, 20.0))
        means[redo] = fresh.means.numpy()[redo]
        sc.means = torch.from_numpy(means.copy())
    sc.means = torch.from_numpy(means)
    st = oracle_state(sc, cam)
    f = st["fwd"]
    pairs, exact0 = 0, 0
    for t in range(4):
        alpha, sigma, i, j = pair_alpha(st, t, 2, 32, 32)
        lo = int(st["bins"][t][0])
        k = np.arange(lo, lo + alpha.shape[0])[:, None, None]
        comp = (sigma >= 0) & (k <= f["final_idx"][i[0]:i[-1] + 1, j[0]:j[-1] + 1][None]) & \
            (alpha >= np.float32(ALPHA_MIN))
        pairs += int((comp & (alpha >= np.float32(0.99))).sum())
        exact0 += int((comp & (sigma == 0)).sum())
    info = dict(pairs_at_clamp=pairs, composited_sigma0_pairs=exact0,
                num_intersects=int(f["num_intersects"]))
    pre = {"opacity == 1.0f": bool((st["opac"] == np.float32(1.0)).all()),
           "centres on exact pixel centres": bool((st["xys"] == target).all()),
           ">= 50 composited pairs at the 0.99 clamp": pairs >= 50,
           "a composited sigma == 0 pair exists": exact0 >= 1}
    return Structured("clamped", sc, cam, pre, info, st)


@functools.lru_cache(maxsize=None)
def dispatch_cells(seed=7):
    """The tiny scene of the backward's dispatch cells ({8x8, strips} x {unsplit, split, split +
    keep bits} x {atomic, deterministic, pair count}): a 40x48 frame (3x3 tiles, the right column
    8 pixels wide), 260 low-opacity Gaussians inside the centre tile that every pixel of it walks
    to the end (a forced chunk of 64 cuts the walk into five parts) and 120 of opacity 0.3 over
    the whole frame, in front of and behind them."""
    cam = synthetic_camera(40, 48)
    rng = np.random.default_rng(seed)
    n_deep, n_rest = 260, 120
    px, py = _lattice(rng, n_deep, 20.5, 26.5, 20.5, 26.5)
    qx, qy = _lattice(rng, n_rest, 1.0, 38.0, 1.0, 46.0)
    z = np.r_[rng.uniform(-0.1, 0.1, n_deep), rng.uniform(0.15, 0.3, n_rest // 2),
              rng.uniform(-0.3, -0.15, n_rest - n_rest // 2)]
    n = n_deep + n_rest
    rgb = rng.uniform(0.1, 0.9, (n, 3))
    opacity = np.r_[np.full(n_deep, DEEP_OPACITY), np.full(n_rest, 0.3)]
    sc = make_scene(cam, np.r_[px, qx], np.r_[py, qy], z, np.full(n, SCALE), opacity, rgb)
    st = oracle_state(sc, cam)
    f = st["fwd"]
    lo, hi = (int(v) for v in st["bins"][CENTRE])
    walk = int(f["final_idx"][16:32, 16:32].max()) - lo + 1
    lens = st["bins"][:, 1] - st["bins"][:, 0]
    info = dict(list_len=hi - lo, walk=walk, list_lens=[int(v) for v in lens],
                final_T_min=float(f["final_Ts"].min()), num_intersects=int(f["num_intersects"]))
    pre = {"3x3 tiles, the right column partial": tuple(cam.tile_bounds[:2]) == (3, 3) and
           cam.width % 16 != 0,
           "centre tile list > 192": hi - lo > 192,
           "centre tile walk > 192 (>= 4 parts of 64)": walk > 192,
           "every tile has a list": bool((lens > 0).all()),
           "no pixel terminates": info["final_T_min"] > 1e-3}
    return Structured("dispatch_cells", sc, cam, pre, info, st)


def oracle_state_xys(scene, cam):
    scales = torch.exp(scene.scales).numpy()
    return O.project_forward(scene.means.numpy(), scales, 1.0, scene.quats.numpy(),
                             cam.viewmat.numpy(), cam.projmat.numpy(), cam.fx, cam.fy, cam.cx,
                             cam.cy, cam.height, cam.width, cam.tile_bounds)[0]


DEEP_CASES = [(63, 0), (64, 0), (65, 1), (4095, 63)] + \
    [(L, lead) for L in (4096, 4097, 8200) for lead in (0, 1, 63)]
# the scenes that take the whole geometry x keep-bits x determinism product
DEEP_FULL = [c for c in DEEP_CASES if c[0] >= 4096]


def all_scenes():
    """(id, builder thunk) of every structured scene."""
    out = [(f"deep_tile-{L}-{lead}", functools.partial(deep_tile, L, lead))
           for L, lead in DEEP_CASES]
    out += [("sparse_windows", sparse_windows), ("early_exit", early_exit),
            ("depth_ties", depth_ties)]
    out += [(f"tiny_frame-{W}x{H}", functools.partial(tiny_frame, W, H)) for W, H in TINY_SIZES]
    out += [("below_threshold", below_threshold), ("clamped", clamped),
            ("dispatch_cells", dispatch_cells)]
    return out
