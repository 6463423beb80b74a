"""The device's area-lit next-event estimation and MIS held to the float64 truth of tests/direct_ref.py with no oracle on its side: per
camera sample of a 16 x 16 film at 4 spp, radiance_samples against the composition of the BSDF, light and geometry truths -- within the
bound derived per sample, exactly where the truth is decided without one, at most 3 % of a row left out (the union of all reasons), every
kind of first vertex at least 30 times, at least 300 decided lit samples of more than 50 distinct values.

Rows by what ptk_shade launches (pt_kernels.hip), each asserted through the kernel set and the properties of the scene description that
select the route -- PtScene's own flags are not exported, they are functions of these:

  matte, matte_le             all Matte                                              k_shade
  sorted                      Matte / plastic halves, PBRTGPU_SHADE_LOCAL=0          k_sort_count/scan/scatter, k_shade_matte_sorted, k_shade_general
  local                       the same, PBRTGPU_SHADE_LOCAL=1                        k_sort_local, k_shade_all
  lobes, uber_kr              anisotropic metal / substrate; uber with Kr / plastic  lobe lists, the specular lobe left out of the estimate
  textured                    plastic's roughness from an image map of one value     k_tex_resolve, k_shade_general_res
  instance, instance_textured the floor inside a translated instance                 k_shade_general_inst_plain, k_shade_general_inst
  specular                    mirror / smooth glass halves                           the specular_bounce emission, no estimate at the vertex
  sphere, sphere_halves       the side emitter is a sphere light (cone sampling)     the *_sph forms: a sphere scene takes the sorted queue even when all Matte
  env                         a constant infinite light beside the emitters           k_shade_env: the material sorts are routed around
  mix                         mix(plastic, matte, 0.3)                                k_shade_mix
  disney                      disney (default setting) / Matte halves                 the disney build (kernel set 2)
  disk                        the big emitter is a disk of the quad's extent          the quadric build (kernel set 1)
  below                       translucent halves (diffuse; four lobes), camera under  the transmission lobes, light half and probe across the surface

and k_nee_resolve in its folded form (a vertex with a shadow ray and no probe) and its three-array form (with a probe) in every row.
`path` with lightsamplestrategy uniform (spatial, with three lights) in every row, power and spatial on matte and sorted, and
`directlighting` "one" and "all" with nsamples 1 and 2 (the sample arrays, ABI 8, quirk Q23) on matte, sorted and sphere; power and
spatial on sphere as well; power and "all" on env; Halton on matte and lobes, the sampler hook's values held to the exact rational
Halton value of each sample (tests/halton_ref.py) before the truth takes them.  The kernels are named
from the launch code; no launch counter or exported flag confirms them, and whether PBRTGPU_SHADE_LOCAL took effect is not observable here.

Every case is one upload, one radiance_samples call and a few hook calls: well under 2 s, the file under 60 s (DESIGN.md section 7 has the
measured times).  DIRECT_TRUTH_WRITE=<file> appends the lines of profiles/direct_truth.txt to it."""
import pytest

import direct_cases as DC
from helpers import pkg

pytestmark = pytest.mark.gpu
capi = pkg.capi
MATTE = capi.PT_MATERIAL_MATTE


@pytest.fixture(autouse=True)
def counters_left_clean(gpu_ctx):
    """The context is the session's: tests after this file read its counters without resetting them first."""
    yield
    gpu_ctx.reset_counters()


def route_of(ctx, sd):
    """What selects the shade kernels: (kernel set, some material is not Matte, some parameter is textured, spheres, instances, infinite
    and delta lights, mix materials)."""
    d = sd.desc
    mats = [sd.buffers["materials"][i] for i in range(d.n_materials)]
    used = {int(sd.buffers["meshes"][i].material) for i in range(d.n_meshes)}
    general = any(mats[i].type != MATTE for i in used if i >= 0)
    # (a mix carries its children's indices in tex_kr / tex_kt: not textures)
    textured = any(getattr(mats[i], f) for i in used if i >= 0 and mats[i].type != capi.PT_MATERIAL_MIX
                   for f, _ in capi.pt_material._fields_ if f.startswith("tex_"))
    n_env = len(getattr(sd, "infinite_lights", None) or [])
    n_delta = len(getattr(sd, "delta_lights", None) or [])
    n_mix = sum(m.type == capi.PT_MATERIAL_MIX for m in mats)
    return (ctx.kernel_set(), general, bool(textured), int(d.n_spheres), int(d.n_instances), n_env + n_delta, n_mix)


def route(general=True, textured=False, instances=0, spheres=0, env=0, mix=0, kernels=capi.PT_KERNELS_BASE, lights=3):
    return dict(key=(kernels, general, textured, spheres, instances, env, mix), lights=lights)


ROUTE = {  # row, or the route where it is not "plain" or "halton" -> what route_of must report, and the number of lights
    "matte": route(general=False), "matte_le": route(general=False), "halves": route(), "lobes": route(), "uber_kr": route(),
    "specular": route(), "below": route(), "sphere": route(general=False, spheres=1), "sphere_halves": route(spheres=1),
    "env": route(env=1, lights=4), "mix": route(mix=1), "disney": route(kernels=capi.PT_KERNELS_DISNEY),
    "disk": route(spheres=1, kernels=capi.PT_KERNELS_QUADRIC, lights=2),
    "textured": route(textured=True), "instance": route(instances=1), "instance_textured": route(textured=True, instances=1),
}


def run_case(ctx, case, label=None):
    row, integ, strategy, way = case
    sd, truth_sd, extent = DC.scenes_of(case)
    info = ctx.upload(sd)
    want = ROUTE[row if way in ("plain", "halton") else way]
    assert route_of(ctx, sd) == want["key"], (route_of(ctx, sd), want["key"])
    assert info.n_lights == want["lights"]
    inp = DC.Inputs(ctx, info, DC.nsamples_of(integ), halton=way == "halton")
    rad = ctx.radiance_samples(inp.bounds).reshape(-1, 3)
    _, tr = DC.truth_of(truth_sd, inp, integ, strategy, extent)
    stat = DC.Stat(("gpu", label or "%s-%s-%s-%s" % case), tr, rad)
    DC.report(stat)
    DC.hold(stat, row)
    return stat


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_device_meets_the_truth(gpu_ctx, case):
    run_case(gpu_ctx, case)


@pytest.mark.parametrize("local", ["0", "1"], ids=["sorted", "local"])
@pytest.mark.parametrize("case", [c for c in DC.CASES if c[0] in ("halves", "sphere_halves") and c[3] == "plain"],
                         ids=lambda c: "%s-%s-%s" % (c[0], c[1], c[2]))
def test_both_material_sorts_meet_the_truth(monkeypatch, case, local):
    """PBRTGPU_SHADE_LOCAL is read when a context is created: 0 takes the global sort and the two segment kernels, 1 the sort inside runs
    of 4 096 entries and k_shade_all.  Both are held to the one truth."""
    import torch  # noqa: F401  (tests/conftest.py: torch's HIP runtime is mapped before the library's)
    monkeypatch.setenv("PBRTGPU_SHADE_LOCAL", local)
    ctx = pkg.Context(0)
    try:
        run_case(ctx, case, "-".join(("sorted" if local == "0" else "local",) + case[:3]))
    finally:
        ctx.close()
