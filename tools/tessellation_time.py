#!/usr/bin/env python3
"""Host tessellation time of the shapes the front end turns into triangle meshes (host/pth_tessellate.cpp):

  * "loopsubdiv" of an icosahedron at levels 4 ... 8 (5 120 ... 1 310 720 triangles);
  * "loopsubdiv" of a ~10 k-face open mesh at levels 3;
  * a "nurbs" bicubic patch diced 1000 x 1000.

Each case runs through the pth_tessellate_* entry point (the front end's code) --repeat times; the best and median wall times are
reported.  With --upload (needs a GPU) the tessellated mesh is also uploaded as a scene (pt_scene_upload: BVH build and copies),
so the two costs can be compared.  One JSON line per case on stdout, and appended to --out when given."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("pbrt-r3_amd")
import tess_inputs as ti  # noqa: E402


def cases():
    P, I = ti.icosahedron()
    for lv in range(4, 9):
        yield "loopsubdiv_icosahedron_levels_%d" % lv, lambda lv=lv: pkg.capi.tessellate_loopsubdiv(I, P, lv)
    gP, gI = ti.grid(71, 71, z=lambda x, y: 0.05 * ((x * 7 + y * 3) % 11), flip=lambda x, y: (x * y) % 3 == 0)   # 10 082 faces, open
    yield "loopsubdiv_open_grid_%dfaces_levels_3" % (len(gI) // 3), lambda: pkg.capi.tessellate_loopsubdiv(gI, gP, 3)
    rng = np.random.default_rng(1)
    cp = np.concatenate([np.stack(np.meshgrid(np.linspace(0, 1, 4), np.linspace(0, 1, 4)), -1).reshape(-1, 2), rng.normal(0, 0.2, (16, 1))], 1)
    kw = dict(nu=4, nv=4, uorder=4, vorder=4, uknots=[0, 0, 0, 0, 1, 1, 1, 1], vknots=[0, 0, 0, 0, 1, 1, 1, 1], P=cp.astype(np.float32).reshape(-1))
    yield "nurbs_bicubic_dice_1000x1000", lambda: pkg.capi.tessellate_nurbs(diceu=1000, dicev=1000, **kw)


def upload_time(mesh, repeat):
    sb = pkg.scenes.SceneBuilder()
    sb.film(xresolution=16, yresolution=16)
    sb.sampler_halton(pixelsamples=1)
    sb._append_mesh(mesh["P"], mesh["indices"].astype(np.int64), mesh["N"], None, mesh["uv"], True, False)
    sd = sb.build()
    ctx = pkg.Context(0)
    try:
        ctx.upload(sd)                                   # warm: module load, first allocations
        ts = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            ctx.upload(sd)
            ts.append(time.perf_counter() - t0)
    finally:
        ctx.close()
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--upload", action="store_true", help="also time pt_scene_upload of each mesh (needs a GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name, fn in cases():
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            m = fn()
            ts.append(time.perf_counter() - t0)
        rec = {"case": name, "triangles": int(len(m["indices"])), "vertices": int(len(m["P"])),
               "tessellate_s_best": round(min(ts), 4), "tessellate_s_median": round(float(np.median(ts)), 4), "repeat": a.repeat}
        if a.upload:
            us = upload_time(m, a.repeat)
            rec["upload_s_best"], rec["upload_s_median"] = round(min(us), 4), round(float(np.median(us)), 4)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
