"""Timing of the eval render of a batch of views (fused.render_fused_eval_views) against a loop
of fused.render_fused_eval over the same cameras: both routes in one process on the same
tensors, HIP events on the render stream (the span includes the host's reads of the intersection
counts, which is what the batch removes), SETTLE rounds of both routes first, then the median and
min / max of RUNS samples per route, the routes interleaved.

Frames: the bear frame (bench config c3: 300k Gaussians @ 512^2) and the headline (1M @ 1080^2);
SH degrees to use 0 and 3; V = 1, 4, 8, 16 cameras of an orbit built from look_at_c2w around the
scene's centre, starting at the config's own camera (its distance, up vector and intrinsics).

The bar: at the bear frame with V = 8 the batch's median is below the MINIMUM of the loop's
samples, at both degrees (reported as "bar: met / MISSED"; the exit status is 1 when missed).
Usage: [CFG=c3,headline] python tools/exp_eval_views.py [profiles/eval_views_timing.txt]"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import bench
from gaussctrl_exp_amd.camera import gc_camera, look_at_c2w
from gaussctrl_exp_amd.fused import render_fused_eval, render_fused_eval_views

SETTLE, RUNS = 40, 20
VIEWS, DEGREES = (1, 4, 8, 16), (0, 3)
ORBIT_STEP = 2 * math.pi / 64  # 16 views span a quarter turn


def orbit(sc, cam, count, dev):
    """`count` cameras on the circle through cam's position around the scene's centre, about
    cam's up vector, looking at the centre; cam's intrinsics and frame."""
    centre = sc.means.mean(0).cpu()
    c2w = cam.c2w.cpu().float()
    up = c2w[:3, 1] / c2w[:3, 1].norm()
    arm = c2w[:3, 3] - centre
    out = []
    for k in range(count):
        a = k * ORBIT_STEP  # Rodrigues' rotation of the arm about up
        r = arm * math.cos(a) + torch.linalg.cross(up, arm) * math.sin(a) + \
            up * float(up @ arm) * (1 - math.cos(a))
        eye = centre + r
        out.append(gc_camera(look_at_c2w(eye.tolist(), centre.tolist(), up.tolist()), cam.fx,
                             cam.fy, cam.cx, cam.cy, cam.width, cam.height).to(dev))
    return out


def timeit(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    dev = torch.device("cuda:0")
    lines, missed = [], False
    for cfg in os.environ.get("CFG", "c3,headline").split(","):
        sc, cam = bench.make_workload(cfg, 0, dev)
        cams = orbit(sc, cam, max(VIEWS), dev)
        bg = torch.zeros(3, device=dev)
        N, H, W = sc.num_points, cam.height, cam.width
        for deg in DEGREES:
            for V in VIEWS:
                sub = cams[:V]

                def batch():
                    return render_fused_eval_views(sc, sub, deg, bg)

                def loop():
                    return [render_fused_eval(sc, c, deg, bg) for c in sub]

                for _ in range(SETTLE):
                    batch()
                    loop()
                torch.cuda.synchronize()
                t = {"batch": [], "loop": []}
                for _ in range(RUNS):
                    t["batch"].append(timeit(batch))
                    t["loop"].append(timeit(loop))
                b, l = np.asarray(t["batch"]), np.asarray(t["loop"])
                # the two routes render the same images (bit for bit: tests/test_gpu_eval_views.py)
                same = all(r["depth"] is not None and torch.equal(r["rgb"], o) for r, o in
                           zip(loop(), batch()["rgb"]))
                line = (f"{cfg}: N={N} {W}x{H} degree {deg} V={V:2d}  batch {np.median(b):.3f} ms "
                        f"[{b.min():.3f}, {b.max():.3f}]  loop {np.median(l):.3f} ms "
                        f"[{l.min():.3f}, {l.max():.3f}]  batch/loop {np.median(b) / np.median(l):.2f}"
                        f"  per view {np.median(b) / V:.3f} vs {np.median(l) / V:.3f} ms"
                        f"  (median [min, max] of {RUNS} after {SETTLE} settle rounds; images "
                        f"{'equal' if same else 'DIFFER'})")
                if cfg == "c3" and V == 8:
                    met = np.median(b) < l.min()
                    missed = missed or not met
                    line += f"  bar (batch median < loop min): {'met' if met else 'MISSED'}"
                lines.append(line)
                print(line, flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
