#!/usr/bin/env python3
"""What an upload leaves on the device, scene by scene, as text: run once per build of libpbrtgpu.so (PBRTGPU_LIB names the library)
and compare the outputs line for line.  Every scene goes up under BVH_BUILD_HOST and under BVH_BUILD_DEVICE; a line holds the two
bvh_digest words, pt_scene_info without its two timings, the sha256 of the XYZW film after one render() (of the per-sample radiance where a
filter wider than a pixel makes the film's last bits depend on the order of its atomic adds) and the counters -- or, for a refused upload,
the status and the message.

    PBRTGPU_LIB=/path/to/other/libpbrtgpu.so python tools/upload_equivalence.py > other.txt
    python tools/upload_equivalence.py > this.txt && cmp other.txt this.txt
"""
import hashlib
import importlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("pbrt-r3_amd")
scenes, capi = pkg.scenes, pkg.capi

import aov_cases
import disney_cases
import feature_scenes as fs
import mix_cases
import quadric_cases
import test_gpu_delta_light as delta
import test_gpu_translucent as translucent

# left out: the timings, and the one counter that depends on how the blocks were scheduled (which visits found their node in a block's LDS copy)
TIMINGS = ("bvh_build_ms", "upload_ms", "trace_ms", "shade_ms", "render_ms", "nodes_from_lds")


def scene_list():
    out = []
    for name, fn in sorted(inspect.getmembers(fs, inspect.isfunction)):
        if name.startswith("scene_") and all(p.default is not p.empty for p in inspect.signature(fn).parameters.values()):
            out.append((name, fn))
    out += [("scene_accel_" + m, lambda m=m: fs.scene_accel(m, 4)) for m in ("sah", "hlbvh", "middle", "equal")]
    out += [("scene_materials_lights_" + s, lambda s=s: fs.scene_materials_lights(s)) for s in ("uniform", "power", "spatial")]
    out += [("mix_nested", lambda: mix_cases.palette({"nested": mix_cases.SETTINGS["nested"]})),
            ("disney_first", lambda: disney_cases.palette([next(iter(disney_cases.SETTINGS))])),
            ("quadric_world", quadric_cases.scene_world),
            ("translucent_glass_sphere", lambda: translucent.room_scene(translucent.PAIRS["glass"]()[0], "sphere")),
            ("delta_selection_power", lambda: delta.selection_scene("power")),
            ("aov_plain", aov_cases.case_plain),
            ("rt1m_20000", lambda: scenes.rt1m(20000, res=32, spp=1, max_depth=3))]
    return out


def run(ctx, name, make, where):
    line = {"scene": name, "build": where}
    try:
        ctx.set_bvh_build(where)
        sd = make()
        info = ctx.upload(sd)
        if max(sd.desc.filter_radius) > 0.5:       # samples land in several pixels by float atomics: the film's last bits follow their order, run by run
            rad = ctx.radiance_samples(tuple(info.sample_bounds))
            line["radiance_sha256"] = hashlib.sha256(rad.tobytes()).hexdigest()
        ctx.reset_counters()
        ctx.film_clear()
        ctx.render()
        line["digest"] = ["%016x" % w for w in ctx.bvh_digest()]
        line["info"] = {k: (list(getattr(info, k)) if hasattr(getattr(info, k), "__len__") else getattr(info, k))
                        for k, _ in info._fields_ if k not in TIMINGS}
        if "radiance_sha256" not in line:
            line["film_sha256"] = hashlib.sha256(ctx.film_xyzw().tobytes()).hexdigest()
        line["counters"] = {k: v for k, v in ctx.counters().items() if k not in TIMINGS}
    except capi.PtError as e:
        line["refused"] = [getattr(e, "status", None), str(e)]
    print(json.dumps(line, sort_keys=True), flush=True)


def main():
    ctx = pkg.Context(0)
    try:
        for name, make in scene_list():
            for where in (capi.BVH_BUILD_HOST, capi.BVH_BUILD_DEVICE):
                run(ctx, name, make, where)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
