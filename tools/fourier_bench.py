#!/usr/bin/env python3
"""Mrays/s of the lit room of tests/test_gpu_translucent.py (room_scene: the room of feature_scenes with a smooth-shaded blob and a slab)
at a benchmark-sized film, with the blob and the slab under

    fourier_roughgold   Material "fourier" reading tests/golden/roughgold_alpha_0.2.bsdf (58 nodes, three channels, up to 172 coefficients
                        per node pair): the sixth build of the kernels
    metal_rough_0.2     Material "metal" at roughness 0.2 with copper's eta and k: the first build

and the share of the frame's device time spent in the shading kernels (pt_counters: shade_ms / render_ms).  Prints one line per setup
and writes them to profiles/fourier_scene.txt.  There is no bar: the first figure is the baseline a later performance change of the
table evaluation is measured against.

    python3 tools/fourier_bench.py [--res 1024] [--spp 16] [--steps 3]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pkg = importlib.import_module("pbrt-r3_amd")
OUT = os.path.join(ROOT, "profiles", "fourier_scene.txt")
GOLD = os.path.join(ROOT, "tests", "golden", "roughgold_alpha_0.2.bsdf")
CU_ETA, CU_K = (0.2, 0.92, 1.1), (3.9, 2.45, 2.14)
SETUPS = {
    "fourier_roughgold": lambda b: b.material_fourier(bsdffile=GOLD),
    "metal_rough_0.2": lambda b: b.material_metal(CU_ETA, CU_K, roughness=0.2),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    from test_gpu_translucent import room_scene
    lines = ["tools/fourier_bench.py --res %d --spp %d --steps %d: room_scene(plain, path_sobol), best of the steps" % (args.res, args.spp, args.steps)]
    for setup, mat in SETUPS.items():
        ctx = pkg.Context(0)
        ctx.upload(room_scene(mat, "plain", "path_sobol", res=args.res, spp=args.spp))
        ctx.film_clear()
        ctx.render()                     # warm-up
        best = None
        for _ in range(args.steps):
            ctx.reset_counters()
            ctx.film_clear()
            t0 = time.time()
            ctx.render()
            rgb = ctx.film_rgb()
            dt = time.time() - t0
            c = ctx.counters()
            rate = (c["regular_rays"] + c["shadow_rays"]) / dt / 1e6
            if best is None or rate > best[0]:
                best = (rate, dt, c)
        rate, dt, c = best
        info = pkg.capi.pt_scene_info()
        ctx.lib.pt_scene_info_get(ctx.h, info)
        lines.append("%-18s kernel set %d  %8.1f Mrays/s  %8.2f ms  rays %d  shading kernels %.3f of the device time (shade %.2f ms, trace %.2f ms, frame %.2f ms)  "
                     "mean rgb %s  samples at an iteration cap %d" % (setup, ctx.kernel_set(), rate, dt * 1e3, c["regular_rays"] + c["shadow_rays"],
                                                                 c["shade_ms"] / c["render_ms"], c["shade_ms"], c["trace_ms"], c["render_ms"],
                                                                 [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], info.fourier_capped))
        print(lines[-1], flush=True)
        ctx.close()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
