"""Row-frozen Adam: gsplat_adam_step_rows and TrainStep(trainable=...).

A row whose mask byte is 0 keeps its parameter and both moments bit for bit; every other
element gets gsplat_adam_step's update bit for bit.  Comparisons are torch.equal throughout:
the two kernels run the same element arithmetic (csrc/adam_math.h), so nothing is approximate.
"""
import ctypes

import pytest
import torch

from gaussctrl_exp_amd import _lib
from gaussctrl_exp_amd.camera import synthetic_camera
from gaussctrl_exp_amd.optim import FusedAdam
from gaussctrl_exp_amd.scene import PARAM_NAMES, synthetic_scene
from gaussctrl_exp_amd.train import GROUP_LR, TrainStep

pytestmark = pytest.mark.gpu

N = 1003  # odd: 16-byte vectors straddle rows in every group (row widths 3, 4, 1, 45)


def _shapes(K):
    return {"means": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N, 1),
            "features_dc": (N, 3), "features_rest": (N, K - 1, 3)}


def _mask(kind, gpu):
    gen = torch.Generator().manual_seed(21)
    if kind == "random":
        m = torch.rand(N, generator=gen) < 0.5
    elif kind == "sparse":
        m = torch.rand(N, generator=gen) < 0.02
    else:
        m = torch.full((N,), kind == "ones")
    return m.to(gpu)


def _c_step(entry, P, G, M, V, step, extra=()):
    """One C-ABI Adam call over the six groups (the reference's learning rates, eps 1e-15)."""
    n = len(P)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    numel = (ctypes.c_int64 * n)(*[t.numel() for t in P])
    lrs = (ctypes.c_float * n)(*[GROUP_LR[k] for k in PARAM_NAMES])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    _lib.call(entry, n, cast(arr(P)), cast(arr(G)), cast(arr(M)), cast(arr(V)), cast(numel),
              cast(lrs), step, 0.9, 0.999, 1e-15, *extra, _lib.stream(P[0].device))


@pytest.mark.parametrize("mask_kind", ["random", "sparse", "ones", "zeros"])
@pytest.mark.parametrize("K", [16, 1])
def test_adam_step_rows(gpu, K, mask_kind):
    """Six groups, N = 1003, K = 16 and K = 1 (an empty features_rest), warm moments, step 3."""
    gen = torch.Generator().manual_seed(K)
    shapes = _shapes(K)
    mk = lambda scale=1.0: [(torch.randn(*shapes[k], generator=gen) * scale).to(gpu)
                            for k in PARAM_NAMES]
    P0, G, M0 = mk(), mk(1e-3), mk(1e-3)
    V0 = [t.abs() * 1e-3 for t in mk()]
    rows = _mask(mask_kind, gpu)
    clone = lambda ts: [t.clone() for t in ts]
    Pa, Ma, Va = clone(P0), clone(M0), clone(V0)  # gsplat_adam_step
    Pb, Mb, Vb = clone(P0), clone(M0), clone(V0)  # gsplat_adam_step_rows
    _c_step("gsplat_adam_step", Pa, G, Ma, Va, 3)
    row_elems = (ctypes.c_int64 * 6)(*[t.numel() // N for t in Pb])
    rows_u8 = rows.to(torch.uint8)
    _c_step("gsplat_adam_step_rows", Pb, G, Mb, Vb, 3,
            extra=(N, ctypes.cast(row_elems, ctypes.c_void_p), rows_u8.data_ptr()))
    torch.cuda.synchronize()
    for k, name in enumerate(PARAM_NAMES):
        for what, got, full, init in (("param", Pb[k], Pa[k], P0[k]),
                                      ("exp_avg", Mb[k], Ma[k], M0[k]),
                                      ("exp_avg_sq", Vb[k], Va[k], V0[k])):
            assert torch.equal(got[~rows], init[~rows]), f"{name} {what}: a frozen row moved"
            assert torch.equal(got[rows], full[rows]), f"{name} {what}: differs from adam_step"
        if P0[k].numel() and rows.any():
            assert not torch.equal(Pb[k][rows], P0[k][rows])  # (the live rows did move)


def test_adam_step_rows_rejects_bad_rows(gpu):
    p = [torch.zeros(N, 3, device=gpu)]
    rows = torch.ones(N, dtype=torch.uint8, device=gpu)
    one = lambda v: ctypes.cast((ctypes.c_int64 * 1)(v), ctypes.c_void_p)
    arr = lambda t: ctypes.cast((ctypes.c_void_p * 1)(t.data_ptr()), ctypes.c_void_p)
    lrs = ctypes.cast((ctypes.c_float * 1)(1e-3), ctypes.c_void_p)
    with pytest.raises(RuntimeError):  # numels[0] != num_rows * row_elems[0]
        _lib.call("gsplat_adam_step_rows", 1, arr(p[0]), arr(p[0]), arr(p[0]), arr(p[0]),
                  one(3 * N), lrs, 1, 0.9, 0.999, 1e-15, N, one(4), rows.data_ptr(),
                  _lib.stream(gpu))


def test_fused_adam_rows_argument(gpu):
    """FusedAdam.step(rows=...): the masked step through the optimiser, per-name calls included;
    the step count stays global."""
    gen = torch.Generator().manual_seed(2)
    shapes = _shapes(16)
    init = {k: torch.randn(*shapes[k], generator=gen) for k in PARAM_NAMES}
    grads = {k: torch.randn(*shapes[k], generator=gen) * 1e-3 for k in PARAM_NAMES}
    rows = _mask("random", gpu)
    opts = []
    for _ in range(2):
        prm = {k: v.clone().to(gpu).requires_grad_() for k, v in init.items()}
        opts.append((FusedAdam([{"params": [prm[k]], "lr": GROUP_LR[k], "name": k}
                                for k in PARAM_NAMES], eps=1e-15), prm))
    for opt, prm in opts:
        for k in PARAM_NAMES:
            prm[k].grad = grads[k].to(gpu)
    (full, pf), (masked, pm) = opts
    for _ in range(2):
        full.step()
        masked.step(names=("features_dc", "features_rest"), rows=rows)
        masked.step(names=[k for k in PARAM_NAMES if not k.startswith("features")],
                    advance=False, rows=rows)
    assert masked.step_count == full.step_count == 2
    for k in PARAM_NAMES:
        assert torch.equal(pm[k].detach()[rows], pf[k].detach()[rows]), k
        assert torch.equal(pm[k].detach()[~rows].cpu(), init[k][~rows.cpu()]), k
        st = masked.state[pm[k]]
        assert not st["exp_avg"][~rows].any() and not st["exp_avg_sq"][~rows].any(), k
    with pytest.raises(ValueError):
        masked.step(rows=rows[:-1])
    with pytest.raises(ValueError):
        masked.step(rows=rows.float())


@pytest.fixture
def deterministic():
    prev = _lib.set_deterministic(True)
    yield
    _lib.set_deterministic(prev)


def test_train_step_trainable(gpu, deterministic):
    """TrainStep(render_mode="fused", trainable=m), deterministic mode, 64x48, N = 500."""
    n = 500
    base = synthetic_scene(n, 3, seed=3, scale_lo=0.01, scale_hi=0.05)
    cam = synthetic_camera(64, 48).to(gpu)
    gen = torch.Generator().manual_seed(4)
    gt = torch.rand(48, 64, 3, generator=gen).to(gpu)
    bg = torch.tensor([0.2, 0.4, 0.6], device=gpu)
    m = (torch.rand(n, generator=gen) < 0.4).to(gpu)
    fresh = lambda: synthetic_scene(n, 3, seed=3, scale_lo=0.01, scale_hi=0.05).to(gpu)
    init = [p.to(gpu) for p in base.params()]

    plain = TrainStep(fresh(), render_mode="fused", fuse_adam=False)
    plain.step(cam, gt, bg)
    masked = TrainStep(fresh(), render_mode="fused", trainable=m)
    assert not masked.fuse_adam and not masked.fuse_sh_adam
    loss = masked.step(cam, gt, bg)
    assert torch.isfinite(loss)
    moved = 0
    for name, p, q, p0 in zip(PARAM_NAMES, masked.params, plain.params, init):
        assert torch.equal(p.detach()[m], q.detach()[m]), f"{name}: selected rows differ"
        assert torch.equal(p.detach()[~m], p0[~m]), f"{name}: a frozen row moved"
        moved += int((p.detach()[m] != p0[m]).sum())
    assert moved > 0
    for _ in range(2):
        loss = masked.step(cam, gt, bg)
    assert torch.isfinite(loss) and masked.step_count == 3 and masked.opt.step_count == 3
    for name, p, p0 in zip(PARAM_NAMES, masked.params, init):
        assert torch.equal(p.detach()[~m], p0[~m]), f"{name}: a frozen row moved (3 steps)"
        st = masked.opt.state[p]
        assert not st["exp_avg"][~m].any() and not st["exp_avg_sq"][~m].any(), name

    from gaussctrl_exp_amd.density import DensityConfig
    with pytest.raises(ValueError):
        TrainStep(fresh(), render_mode="fused", trainable=m, density=DensityConfig(num_train_data=10))
    with pytest.raises(ValueError):
        TrainStep(fresh(), trainable=m, api=object())
