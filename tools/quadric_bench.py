#!/usr/bin/env python3
"""RT1M with 150 cylinders and 150 disks among the triangles (radii 0.01-0.08, rotated, some clipped in phi or with an inner radius), 64 spp:
one JSON line with the Mrays/s of three renders of one upload.  The scene of profiles/quadric_scene.txt; under a kernel trace the same
script gives the time of ptq::k_trace_sph_dist per launch.

    python tools/quadric_bench.py
"""
import importlib, os, sys, time, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa
pkg = importlib.import_module("pbrt-r3_amd")
T = pkg.scenes
def finish(b):
    rng = np.random.default_rng(7)
    b.material_matte((0.6, 0.4, 0.3))
    for k in range(300):
        c = rng.uniform(-0.85, 0.85, 3)
        t = T.transform_mul(T.transform_translate(*c), T.transform_rotate_x(float(rng.uniform(0, 180))))
        if k % 2:
            b.shape_cylinder(radius=float(rng.uniform(0.01, 0.04)), zmin=-0.1, zmax=0.1, phimax=float(rng.choice([360.0, 270.0])), object_to_world=t[0], world_to_object=t[1])
        else:
            b.shape_disk(height=0.0, radius=float(rng.uniform(0.02, 0.08)), innerradius=float(rng.choice([0.0, 0.01])), object_to_world=t[0], world_to_object=t[1])
sd = T.rt1m(1000000, res=1024, spp=64, max_depth=8, finish=finish)
ctx = pkg.Context(0)
info = ctx.upload(sd)
tiles = T.all_tiles(info)
res = []
for i in range(3):
    ctx.film_clear(); ctx.reset_counters()
    torch.cuda.synchronize(); t0 = time.time()
    ctx.render(tiles)
    torch.cuda.synchronize(); dt = time.time() - t0
    c = ctx.counters()
    rays = c["regular_rays"] + c["shadow_rays"]
    res.append(rays / dt / 1e6)
rgb = ctx.film_rgb()
print(json.dumps({"scene": "RT1M + 150 cylinders + 150 disks, 1024^2, 64 spp, depth 8", "n_analytic": int(sd.desc.n_spheres), "mrays_per_s": [round(r, 1) for r in res],
                  "film_finite": bool(np.isfinite(rgb).all()), "film_mean": float(rgb.mean())}))
ctx.close()
