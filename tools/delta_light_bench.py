#!/usr/bin/env python3
"""Frame time and Mrays/s of the RT1M geometry (bench.py's headline scene) lit three ways: its quad emitter (the headline's kernels), a
distant light in the emitter's place (the delta family: one shadow ray per vertex, no MIS probe), and a spot added beside the emitter.
One JSON line per setup: the best of --steps frames, each timed from an idle device to an idle device, the film's read-back outside it.

    python3 tools/delta_light_bench.py [--triangles 1000000] [--res 512] [--spp 16] [--steps 3]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("pbrt-r3_amd")


def scene(kind, args):
    if kind == "distant":
        return pkg.scenes.rt1m(args.triangles, res=args.res, spp=args.spp, light="distant")
    finish = None
    if kind == "quad+spot":
        def finish(b):
            b.light_spot(I=(8.0, 8.0, 8.0), coneangle=40.0, conedelta=10.0, frm=(0.5, 0.9, -0.9), to=(0.0, -0.5, 0.3))
    return pkg.scenes.rt1m(args.triangles, res=args.res, spp=args.spp, finish=finish)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kinds", default="quad,distant,quad+spot")
    args = ap.parse_args()
    for kind in args.kinds.split(","):
        ctx = pkg.Context(0)
        info = ctx.upload(scene(kind, args))
        ctx.film_clear()
        ctx.render()                     # warm-up
        best = None
        for _ in range(args.steps):
            ctx.reset_counters()
            ctx.film_clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.render()
            torch.cuda.synchronize()     # as bench.py brackets its frames: the device is idle at both ends
            dt = time.perf_counter() - t0
            rgb = ctx.film_rgb()         # the read-back is outside the timed interval
            c = ctx.counters()
            if best is None or dt < best[0]:
                best = (dt, c["regular_rays"], c["shadow_rays"])
        print(json.dumps({"setup": kind, "frame_ms": round(best[0] * 1e3, 2), "mrays_s": round((best[1] + best[2]) / best[0] / 1e6, 1),
                          "regular_rays": best[1], "shadow_rays": best[2], "n_lights": info.n_lights,
                          "mean_rgb": [round(float(v), 5) for v in rgb.reshape(-1, 3).mean(0)], "res": args.res, "spp": args.spp}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
