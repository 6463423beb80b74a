#!/usr/bin/env python3
"""Mrays/s of the RT1M geometry (bench.py's headline scene, its quad light kept) with an environment added three ways: a constant
LightSource "infinite", a 2048 x 1024 image-mapped one, and the enclosing-sphere equivalent (a two-sided sphere area light of radius 10
around the scene, black matte).  One JSON line per setup.

    python3 tools/env_light_bench.py [--triangles 1000000] [--res 512] [--spp 16] [--steps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

pkg = importlib.import_module("pbrt-r3_amd")


def scene(kind, args):
    def finish(b):
        if kind == "constant":
            b.light_infinite(L=(0.8, 0.9, 1.0))
        elif kind == "map":
            rng = np.random.default_rng(7)
            y, x = np.mgrid[0:1024, 0:2048].astype(np.float32)
            sky = 0.5 + 0.5 * np.cos(np.pi * y / 1024.0)[..., None] * np.array([0.6, 0.8, 1.0], np.float32)
            sun = 40.0 * np.exp(-((x - 600.0) ** 2 + (y - 300.0) ** 2) / 200.0)[..., None]
            b.light_infinite(image=(sky + sun + 0.05 * rng.random((1024, 2048, 3), dtype=np.float32)).astype(np.float32))
        elif kind == "sphere":
            b.material_matte((0.0, 0.0, 0.0))
            b.area_light_source_diffuse(L=(0.8, 0.9, 1.0), twosided=True)
            b.shape_sphere(radius=10.0)
            b.no_area_light()
    return pkg.scenes.rt1m(args.triangles, res=args.res, spp=args.spp, finish=finish)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kinds", default="constant,map,sphere")
    args = ap.parse_args()
    for kind in args.kinds.split(","):
        sd = scene(kind, args)
        ctx = pkg.Context(0)
        t0 = time.time()
        info = ctx.upload(sd)
        up_s = time.time() - t0
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
        print(json.dumps({"setup": kind, "mrays_s": round(best, 1), "n_lights": info.n_lights, "upload_s": round(up_s, 2),
                          "mean_rgb": [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], "res": args.res, "spp": args.spp}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
