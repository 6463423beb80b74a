#!/usr/bin/env python3
"""Mrays/s of a foliage stand-in built at run time: an object of randomly placed and oriented leaf cards, instanced on a grid over a ground
plane under a quad light, path integrator.  Each card is 8 x 8 sub-quads with their own uv; a 64 x 64 imagemap of 8 x 8 blocks (about half of
them 0) is the mask.  Three setups, one JSON line each:

    masked    every sub-quad, "texture alpha" = the imagemap (k_trace_alpha)
    opaque    the same cards without the mask (the scene's usual traversal kernel)
    cutout    only the sub-quads the mask keeps, as explicit triangles (the same image as "masked", bit for bit)

    python3 tools/alpha_bench.py [--cards 2000] [--instances 16] [--res 512] [--spp 16] [--steps 3]
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
G = 8


def cards(n, keep, seed=3):
    """n cards of 0.2 x 0.2 inside the unit cube: P, indices, uv of their sub-quads (only those keep[j, i] allows)."""
    rng = np.random.default_rng(seed)
    P, uv = [], []
    for _ in range(n):
        c = rng.random(3).astype(np.float32)
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3)); b /= np.linalg.norm(b)
        e1, e2 = (0.2 / G) * a, (0.2 / G) * np.cross(a, b)
        for j in range(G):
            for i in range(G):
                if not keep[j, i]:
                    continue
                o = c + (i - G / 2) * e1 + (j - G / 2) * e2
                P += [o, o + e1, o + e1 + e2, o + e2]
                u0, v0, u1, v1 = (i + 0.1) / G, (j + 0.1) / G, (i + 0.9) / G, (j + 0.9) / G
                uv += [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
    P = np.array(P, np.float32)
    idx = (np.arange(len(P) // 4)[:, None] * 4 + np.array([0, 1, 2, 0, 2, 3])).reshape(-1)
    return P, idx, np.array(uv, np.float32)


def scene(setup, args):
    rng = np.random.default_rng(11)
    blocks = (rng.random((G, G)) < 0.5).astype(np.float32)
    sb = pkg.scenes.SceneBuilder()
    sb.look_at((-2, -2, 3), (2, 2, 0.5), (0, 0, 1))
    sb.camera_perspective(fov=60)
    sb.film(xresolution=args.res, yresolution=args.res)
    sb.sampler_sobol(pixelsamples=args.spp)
    sb.integrator_path(maxdepth=5)
    mask = sb.texture_imagemap(sb.image_pyramid(np.kron(blocks, np.ones((8, 8), np.float32))), uscale=1.0, vscale=1.0)
    sb.area_light_source_diffuse(L=(20, 20, 18))
    sb.shape_trianglemesh([0, 0, 4, 1, 0, 4, 1, 1, 4, 0, 1, 4], [0, 2, 1, 0, 3, 2])
    sb.no_area_light()
    sb.material_matte(Kd=(0.4, 0.35, 0.3))
    n = int(np.sqrt(args.instances))
    sb.shape_trianglemesh([-1, -1, 0, n + 1, -1, 0, n + 1, n + 1, 0, -1, n + 1, 0], [0, 1, 2, 0, 2, 3])
    sb.material_matte(Kd=(0.2, 0.5, 0.15))
    keep = blocks > 0 if setup == "cutout" else np.ones((G, G), bool)
    P, idx, uv = cards(args.cards, keep)
    sb.object_begin("tree")
    sb.shape_trianglemesh(P, idx, uv=uv, **({"alpha": mask} if setup == "masked" else {}))
    sb.object_end()
    for k in range(n * n):
        m = np.eye(4, dtype=np.float32); m[:3, 3] = (k % n, k // n, 0.0)
        mi = np.eye(4, dtype=np.float32); mi[:3, 3] = (-(k % n), -(k // n), 0.0)
        sb.object_instance("tree", (m.reshape(-1), mi.reshape(-1)))
    return sb.build(), float(blocks.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cards", type=int, default=2000)
    ap.add_argument("--instances", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--setups", default="masked,opaque,cutout")
    args = ap.parse_args()
    for setup in args.setups.split(","):
        sd, kept = scene(setup, args)
        ctx = pkg.Context(0)
        info = ctx.upload(sd)
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
        print(json.dumps({"setup": setup, "mrays_s": round(best, 1), "triangles": int(info.n_triangles) if hasattr(info, "n_triangles") else None,
                          "kept_fraction": kept, "mean_rgb": [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], "res": args.res,
                          "spp": args.spp, "cards": args.cards, "instances": args.instances}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
