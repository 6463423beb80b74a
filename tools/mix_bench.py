#!/usr/bin/env python3
"""Mrays/s of the RT1M geometry (BASELINE config 2) with a share of its filler triangles under Material "mix", next to the same scene with
those triangles under an "uber" of equal lobe count, all under an environment light, so that every setup shades over the unsorted queue
(k_shade_mix for the mixes, k_shade_env for uber).  Appends one JSON line per setup to profiles/mix_bench.jsonl:

    mix_const      share of the triangles mix(plastic, matte, 0.3): three lobes, the tree built once at upload
    mix_textured   ... with "amount" = a checkerboard: the tree's scales built at every hit
    uber3          the same triangles uber (Kd, Ks, Kr: three lobes)
    headline       bench.py's headline scene (no mix, no environment), several runs: mean, min and max.  With --parent-lib (a libpbrtgpu.so
                   built from the parent commit) the same runs through that library in the same call, as headline_parent; the two agree
                   when this commit's mean lies within the parent's own min .. max

    python3 tools/mix_bench.py [--triangles 1000000] [--share 0.3] [--res 512] [--spp 16] [--steps 3] [--parent-lib PATH]
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
OUT = os.path.join(ROOT, "profiles", "mix_bench.jsonl")


def scene(setup, args):
    S = pkg.scenes
    if setup.startswith("headline"):
        return S.rt1m(args.triangles, res=args.res, spp=args.spp)
    n_fill = max(0, args.triangles - 12)
    n_share = int(round(args.share * n_fill))

    def finish(b):
        """The share: RT1M's filler recipe (scenes.rt1m) continued on PCG32 sequence 2, under the setup's material."""
        b.no_area_light()
        b.light_infinite(L=(0.5, 0.5, 0.5))
        u = S.pcg32_uniform_float(12 * n_share, 2).reshape(n_share, 12)
        one, s = f32(1.0), 0.005
        c = (one - u[:, 0:3]) * f32(-0.9) + u[:, 0:3] * f32(0.9)
        off = (one - u[:, 3:12]) * f32(-s) + u[:, 3:12] * f32(s)
        verts = (np.repeat(c, 3, axis=0).reshape(n_share, 9) + off).astype(np.float32).reshape(-1, 3)
        if setup == "uber3":
            b.material_uber(Kd=(0.3, 0.6, 0.2), Ks=(0.2, 0.2, 0.2), Kr=(0.1, 0.1, 0.1), roughness=0.2)
        else:
            b.material_plastic(Kd=(0.3, 0.6, 0.2), Ks=(0.2, 0.2, 0.2), roughness=0.2)
            p = b.cur_material
            b.material_matte((0.6, 0.3, 0.2))
            m = b.cur_material
            amount = (0.3, 0.3, 0.3) if setup == "mix_const" else b.texture_checkerboard(0.1, 0.8, uscale=4.0, vscale=4.0, aamode="none")
            b.material_mix(p, m, amount)
        b.shape_trianglemesh_fast(verts, np.arange(3 * n_share), twosided=True)
    return S.rt1m(12 + n_fill - n_share, res=args.res, spp=args.spp, finish=finish)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--headline-steps", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--setups", default="mix_const,mix_textured,uber3,headline")
    args = ap.parse_args()
    setups = args.setups.split(",")
    if args.parent_lib and "headline" in setups:
        setups.insert(setups.index("headline"), "headline_parent")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for setup in setups:
        sd = scene(setup, args)
        lib = pkg.capi.load_library(args.parent_lib) if setup == "headline_parent" else None
        ctx = pkg.Context(0, lib=lib)
        ctx.upload(sd)
        ctx.film_clear()
        ctx.render()                     # warm-up
        rates = []
        for _ in range(args.headline_steps if setup.startswith("headline") else args.steps):
            ctx.reset_counters()
            ctx.film_clear()
            t0 = time.time()
            ctx.render()
            rgb = ctx.film_rgb()
            dt = time.time() - t0
            c = ctx.counters()
            rates.append((c["regular_rays"] + c["shadow_rays"]) / dt / 1e6)
        line = json.dumps({"setup": setup, "mrays_s": round(max(rates), 1), "mean": round(float(np.mean(rates)), 1), "min": round(min(rates), 1),
                           "max": round(max(rates), 1), "runs": len(rates), "rays": int(c["regular_rays"] + c["shadow_rays"]), "triangles": args.triangles,
                           "share": args.share, "mean_rgb": [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], "res": args.res, "spp": args.spp})
        print(line, flush=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")
        ctx.close()


if __name__ == "__main__":
    main()
