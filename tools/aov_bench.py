#!/usr/bin/env python3
"""Camera rays per second of `Integrator "aov"` on the RT1M geometry (1M triangles, 1024 x 1024, 16 spp), targets `n` and `dpdx`, and
k_aov's share of the device time; next to them the same frame under `ao` with `nsamples` 1, for scale.  One JSON line per setup, printed
and appended to profiles/aov_bench.jsonl.  Device times are the context's own HIP-event spans (pt_counters: trace_ms is the traversal
kernel, shade_ms what follows it in a pass -- k_aov here; k_ao_rays' occlusion pass counts as traversal for `ao`).

    python3 tools/aov_bench.py [--triangles 1000000] [--res 1024] [--spp 16] [--steps 3] [--out profiles/aov_bench.jsonl]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_bench.jsonl"))
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as bench.py has it)
    pkg = importlib.import_module("pbrt-r3_amd")
    capi = pkg.capi
    ctx = pkg.Context(0)
    rows = []
    for setup in ("aov:n", "aov:dpdx", "ao:1"):
        sd = pkg.scenes.rt1m(n_triangles=args.triangles, res=args.res, spp=args.spp)
        if setup.startswith("aov:"):
            sd.desc.integrator, sd.aov = capi.PT_INTEGRATOR_AOV, (capi.AOV_TARGETS[setup[4:]], 1.0)
        else:
            sd.desc.integrator, sd.desc.ao_samples, sd.desc.ao_cos_sample = capi.PT_INTEGRATOR_AO, 1, 1
        ctx.upload(sd)
        ctx.film_clear()
        ctx.render()                     # warm-up
        best = None
        for _ in range(args.steps):
            ctx.reset_counters()
            ctx.film_clear()
            t0 = time.time()
            ctx.render()
            ctx.film_xyzw()
            dt = time.time() - t0
            c = ctx.counters()
            row = {"setup": setup, "camera_mrays_s": round(c["camera_rays"] / dt / 1e6, 1), "seconds": round(dt, 4),
                   "render_ms": round(c["render_ms"], 3), "trace_ms": round(c["trace_ms"], 3), "after_trace_ms": round(c["shade_ms"], 3),
                   "after_trace_share": round(c["shade_ms"] / c["render_ms"], 4) if c["render_ms"] else None,
                   "rays": int(c["regular_rays"] + c["shadow_rays"]), "triangles": args.triangles, "res": args.res, "spp": args.spp}
            if best is None or row["seconds"] < best["seconds"]:
                best = row
        rows.append(best)
        print(json.dumps(best), flush=True)
    ctx.close()
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
