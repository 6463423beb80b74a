#!/usr/bin/env python3
"""Mrays/s of the mixed-materials scene (scenes.rt1m(materials="mixed"): 40 % of the filler triangles matte, 60 % under five lobe-list
materials) with that 60 % under one material instead, so that every setup shades through the _mix kernel family:

    disney_default   Material "disney" with the reference's defaults: three lobes (diffuse, retro, microfacet)
    disney_thin_all  disney_cases' `thin_all`: all eight lobes
    uber5_mix        uber "five" of bsdf_cases wrapped in a mix with a lobeless sibling at amount 1: the same kernel family with five lobes
                     (the first build's k_shade_mix; the Disney setups run the third build's)

Prints one JSON line per setup and writes them all to profiles/disney_bench.json.  There is no bar: the first figure is the baseline for
later work on the _mix family.

    python3 tools/disney_bench.py [--triangles 1000000] [--res 512] [--spp 16] [--steps 3]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pkg = importlib.import_module("pbrt-r3_amd")
f32 = np.float32
OUT = os.path.join(ROOT, "profiles", "disney_bench.json")
THIN_ALL = dict(color=(0.6, 0.45, 0.3), thin=True, flatness=0.3, difftrans=0.8, sheen=0.6, sheentint=0.7, clearcoat=0.5, clearcoatgloss=0.0, spectrans=0.4,
                metallic=0.2, anisotropic=0.4, roughness=0.45)
UBER_FIVE = dict(Kd=(0.3, 0.2, 0.5), Ks=(0.2, 0.3, 0.1), Kr=(0.1, 0.15, -0.2), Kt=(0.25, 0.2, 0.15), opacity=(0.6, 1.2, 0.8), eta=1.4, roughness=0.3, vroughness=0.1)


def scene(setup, args):
    S = pkg.scenes
    n_fill = max(0, args.triangles - 12)
    n_matte = int(0.40 * n_fill)

    def finish(b):
        """The other 60 % of RT1M's filler triangles (scenes.rt1m's recipe, the same PCG32 sequence), under the setup's material."""
        u = S.pcg32_uniform_float(12 * n_fill, 1).reshape(n_fill, 12)[n_matte:]
        one, s = f32(1.0), 0.005
        c = (one - u[:, 0:3]) * f32(-0.9) + u[:, 0:3] * f32(0.9)
        off = (one - u[:, 3:12]) * f32(-s) + u[:, 3:12] * f32(s)
        verts = (np.repeat(c, 3, axis=0).reshape(len(u), 9) + off).astype(np.float32).reshape(-1, 3)
        b.no_area_light()
        if setup == "disney_default":
            b.material_disney()
        elif setup == "disney_thin_all":
            b.material_disney(**THIN_ALL)
        else:
            b.material_uber(**UBER_FIVE)
            k = b.cur_material
            b.material_matte(Kd=(0.0, 0.0, 0.0))
            b.material_mix(k, b.cur_material, (1.0, 1.0, 1.0))
        b.shape_trianglemesh_fast(verts, np.arange(len(verts)), twosided=True)
    return S.rt1m(12 + n_matte, res=args.res, spp=args.spp, finish=finish)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--setups", default="disney_default,disney_thin_all,uber5_mix")
    args = ap.parse_args()
    lines = []
    for setup in args.setups.split(","):
        ctx = pkg.Context(0)
        ctx.upload(scene(setup, args))
        ctx.film_clear()
        ctx.render()                     # warm-up
        rates = []
        for _ in range(args.steps):
            ctx.reset_counters()
            ctx.film_clear()
            t0 = time.time()
            ctx.render()
            rgb = ctx.film_rgb()
            dt = time.time() - t0
            c = ctx.counters()
            rates.append((c["regular_rays"] + c["shadow_rays"]) / dt / 1e6)
        lines.append({"setup": setup, "mrays_s": round(max(rates), 1), "mean": round(float(np.mean(rates)), 1), "min": round(min(rates), 1),
                      "max": round(max(rates), 1), "runs": len(rates), "rays": int(c["regular_rays"] + c["shadow_rays"]), "triangles": args.triangles,
                      "mean_rgb": [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], "res": args.res, "spp": args.spp})
        print(json.dumps(lines[-1]), flush=True)
        ctx.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
