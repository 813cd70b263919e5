"""Timing of splat-back against the only other route to the same sums (HIP events on the launch
stream, one process): gsplat_rasterize_splat_back with one channel vs gsplat_rasterize_forward
followed by gsplat_rasterize_backward with alpha_max 0.999, v_output = the values, on the same
binning.  Settle launches first, then the median of RUNS timed launches per route, the two
routes interleaved.  Usage: CFG=c3|headline python tools/exp_lift.py [out.txt]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import bench
from gaussctrl_exp_amd import _lib
from gaussctrl_exp_amd.project_gaussians import project_gaussians
from gaussctrl_exp_amd.rasterize import bin_gaussians

SETTLE, RUNS = 40, 20
dev = torch.device("cuda:0")
P, st = _lib.ptr, _lib.stream(dev)
lines = []
for cfg in os.environ.get("CFG", "c3,headline").split(","):
    sc, cam = bench.make_workload(cfg, 0, dev)
    cam = cam.to(dev)
    N, H, W = sc.num_points, cam.height, cam.width
    with torch.no_grad():
        xys, depths, radii, conics, nth, _ = project_gaussians(
            sc.means, torch.exp(sc.scales), 1, sc.quats / sc.quats.norm(dim=-1, keepdim=True),
            *cam.project_args())
        I, gids, bins = bin_gaussians(xys, depths, radii, nth, H, W)
    tb = cam.tile_bounds
    opac = torch.sigmoid(sc.opacities).contiguous()
    mask = (torch.rand(H, W, device=dev) < 0.5).float().contiguous()
    sums = torch.zeros(N, 4, device=dev)
    colors, bg = torch.zeros(N, 3, device=dev), torch.zeros(3, device=dev)
    out = torch.empty(H, W, 3, device=dev); fT = torch.empty(H, W, device=dev)
    fi = torch.empty(H, W, device=dev, dtype=torch.int32)
    v_out = mask[..., None].repeat(1, 1, 3).contiguous()
    g = [torch.empty(N, k, device=dev) for k in (2, 3, 3, 1)]
    wsz = _lib.query("gsplat_rasterize_backward_workspace_size", N, 3)
    ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=dev)

    def splat():
        _lib.call("gsplat_rasterize_splat_back", tb[0], tb[1], H, W, 1, P(gids), P(bins), P(xys),
                  P(conics), P(opac), P(mask), P(sums), st)

    def fwd_bwd():
        _lib.call("gsplat_rasterize_forward", tb[0], tb[1], H, W, 3, P(gids), P(bins), P(xys),
                  P(conics), P(colors), P(opac), P(bg), P(out), P(fT), P(fi), st)
        _lib.call("gsplat_rasterize_backward", tb[0], tb[1], H, W, 3, N, P(gids), P(bins), P(xys),
                  P(conics), P(colors), P(opac), P(bg), P(fT), P(fi), P(v_out), None, 0.999,
                  *[P(x) for x in g], P(ws), wsz, st)

    def timeit(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e)

    for _ in range(SETTLE):
        splat(); fwd_bwd()
    torch.cuda.synchronize()
    t = {"splat": [], "fwd_bwd": []}
    for _ in range(RUNS):
        t["splat"].append(timeit(splat))
        t["fwd_bwd"].append(timeit(fwd_bwd))
    # the two routes' sums agree (the weight-times-mask column vs v_colors' first channel)
    sums.zero_(); splat(); fwd_bwd(); torch.cuda.synchronize()
    err = float((sums[:, 0] - g[2][:, 0]).abs().max()) / max(float(g[2][:, 0].abs().max()), 1e-30)
    lines.append(f"{cfg}: N={N} {W}x{H} I={I}  splat_back(C=1) {np.median(t['splat']):.3f} ms  "
                 f"forward+backward(alpha_max 0.999) {np.median(t['fwd_bwd']):.3f} ms  "
                 f"(median of {RUNS} after {SETTLE} settle launches; max |diff| / max |v_colors| "
                 f"{err:.2e})")
    print(lines[-1], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
