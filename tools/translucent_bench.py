#!/usr/bin/env python3
"""Mrays/s of the RT1M geometry (BASELINE config 2) with a share of its filler triangles carrying Material "translucent", next to the same
scene with those triangles "uber" (the same lobe kinds minus LambertianTransmission), each with and without an alpha mask on them.  One JSON
line per setup:

    translucent          share of the triangles translucent (Kd, Ks, reflect, transmit all non-black: four lobes)
    translucent_masked   ... with "alpha" = a checkerboard float texture on them (k_trace_alpha)
    uber                 the same triangles uber (Kd, Ks: two lobes)
    uber_masked          ... with the same mask
    matte                the same triangles matte: the headline scene's own material, through the same scene construction

    python3 tools/translucent_bench.py [--triangles 1000000] [--share 0.3] [--res 512] [--spp 16] [--steps 3]
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


def scene(setup, args):
    S = pkg.scenes
    n_fill = max(0, args.triangles - 12)
    n_share = int(round(args.share * n_fill))

    def finish(b):
        """The share: RT1M's filler recipe (scenes.rt1m) continued on PCG32 sequence 2, under the setup's material."""
        b.no_area_light()
        u = S.pcg32_uniform_float(12 * n_share, 2).reshape(n_share, 12)
        one, s = f32(1.0), 0.005
        c = (one - u[:, 0:3]) * f32(-0.9) + u[:, 0:3] * f32(0.9)
        off = (one - u[:, 3:12]) * f32(-s) + u[:, 3:12] * f32(s)
        verts = (np.repeat(c, 3, axis=0).reshape(n_share, 9) + off).astype(np.float32).reshape(-1, 3)
        kind = setup.split("_")[0]
        if kind == "translucent":
            b.material_translucent(Kd=(0.3, 0.6, 0.2), Ks=(0.2, 0.2, 0.2), reflect=(0.5, 0.5, 0.5), transmit=(0.5, 0.5, 0.5), roughness=0.2)
        elif kind == "uber":
            b.material_uber(Kd=(0.3, 0.6, 0.2), Ks=(0.2, 0.2, 0.2), roughness=0.2)
        else:
            b.material_matte((0.3, 0.6, 0.2))
        kw = {}
        if setup.endswith("_masked"):
            kw["alpha"] = b.texture_checkerboard(1.0, 0.0, uscale=4.0, vscale=4.0, aamode="none")
        b.shape_trianglemesh_fast(verts, np.arange(3 * n_share), twosided=True, **kw)
    return S.rt1m(12 + n_fill - n_share, res=args.res, spp=args.spp, finish=finish)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--setups", default="translucent,translucent_masked,uber,uber_masked,matte")
    args = ap.parse_args()
    for setup in args.setups.split(","):
        sd = scene(setup, args)
        ctx = pkg.Context(0)
        ctx.upload(sd)
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
            best = rate if best is None else max(best, rate)
        print(json.dumps({"setup": setup, "mrays_s": round(best, 1), "rays": int(c["regular_rays"] + c["shadow_rays"]), "triangles": args.triangles,
                          "share": args.share, "mean_rgb": [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], "res": args.res,
                          "spp": args.spp}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
