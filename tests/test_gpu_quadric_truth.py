"""The device's cylinder and disk hits, occlusion flags and light samples held to the float64 truth of quadric_ref.py (the oracle does
not know these shapes and is never loaded here).

Every ray case of quadric_cases sends its 8 191 rays through both entrances -- pt_trace_closest / pt_trace_any and pt_trace_wavefront
with kinds 1 / 2 / 3 dealt at random: same hit or miss, same primitive, |t - t64| <= bound, occlusion flag equal on decisive rays, the two
entrances bit-equal, at most 3 % left out, and the median of err / bound over the cylinder hits below quadric_cases.MEDIAN_LIMIT.  The
instanced case holds t and hit / miss only, as geometry_cases does.  Light samples: pt_light_sample_li over a 64 x 64 stratum grid plus
corners for a disk light, a cylinder light and a partial annulus (Disk::sample's whole-disk quirk), and mean(1 / pdf) against the
quadrature of the solid angle for the two full shapes.  pt_light_pdf_from (DiffuseAreaLight::pdf_li, the default Shape::pdf_from: the route of
the BSDF-sampling half of MIS) over a grid of directions against quadric_ref.pdf_from, and against the device's own sample_li pdf where the
sampled point is what a ray along wi meets first."""
import numpy as np
import pytest

import geometry_cases as GC
import geometry_ref as G
import quadric_cases as QC
import quadric_ref as Q
from helpers import pkg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(QC.RAY_CASES))
def test_device_rays_against_truth(gpu_ctx, name):
    make, key, inst = QC.RAY_CASES[name]
    sd = make()
    info = gpu_ctx.upload(sd)
    rays = QC.make_rays(name, sd, info, gpu_ctx.generate_camera_rays)
    o, d, t, kind = rays
    tr = QC.truth_of(key, sd, rays)
    every = np.ones(len(t), bool)
    hits = gpu_ctx.trace_closest(o, d, t)
    occ = gpu_ctx.trace_any(o, d, t)
    ratio = GC.hold_hits(name + " batch", tr, every, hits, inst=inst)
    GC.hold_occlusion(name + " batch", tr, every, occ)
    left = float((tr["rule"] != 0).mean())
    by = np.bincount(tr["rule"], minlength=5)
    print("device %-22s left out %.2f %% (a %d, b %d, c %d, d %d)  err/bound worst %.3f median %.4f (%d hits)" % (
        name, 100 * left, by[1], by[2], by[3], by[4], ratio.max(), np.median(ratio), len(ratio)))
    assert left <= GC.MAX_LEFT_OUT and len(ratio) >= 1000
    whits, wocc = gpu_ctx.trace_wavefront(o, d, t, kind)
    m1, m2, m3 = kind == 1, kind == 2, kind == 3
    wratio = GC.hold_hits(name + " wavefront", tr, m1, whits[m1], inst=inst)
    GC.hold_occlusion(name + " wavefront", tr, m2, wocc[m2])
    if not inst:
        GC.hold_hits(name + " wavefront probes", tr, m3, whits[m3], probe=True)
    assert len(wratio) >= 300
    assert np.array_equal(whits["t"][m1], hits["t"][m1]) and np.array_equal(wocc[m2], occ[m2])
    if not inst:
        # the median over the cylinder hits alone
        sc = Q.Scene(sd)
        cyl_prims = [int(sc.sphere_prim[i]) for i, s in enumerate(sc.spheres) if Q._kind(s) == Q.SHAPE_CYLINDER and s.object == 0]
        sel = (tr["rule"] == 0) & (hits["prim"] >= 0) & np.isin(tr["prim"], cyl_prims)
        r = np.abs(hits["t"].astype(np.float64) - tr["t"])[sel] / tr["bound"][sel]
        print("device %-22s cylinder hits: err/bound worst %.3f median %.4f (%d hits; limit %.4f)" % (name, r.max(), np.median(r), len(r), QC.MEDIAN_LIMIT[key]))
        assert len(r) >= 300 and float(np.median(r)) <= QC.MEDIAN_LIMIT[key]


def test_host_and_device_builds_agree(gpu_ctx):
    """The world-list case under HLBVH: the tree built on the host and the tree built on the device give equal digests."""
    sd = QC.scene_world("hlbvh", 2)
    ctx = pkg.Context(0)
    try:
        ctx.set_bvh_build(1)          # host
        ctx.upload(sd)
        host = ctx.bvh_digest()
        ctx.set_bvh_build(2)          # device
        info = ctx.upload(sd)
        assert info.bvh_on_device == 1
        assert ctx.bvh_digest() == host
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def light_scene():
    sd = QC.scene_lights()
    return sd, Q.Scene(sd)


@pytest.mark.parametrize("case", QC.LIGHT_CASES, ids=QC.light_id)
def test_device_light_samples_against_truth(gpu_ctx, light_scene, case):
    light, p = case
    sd, sc = light_scene
    gpu_ctx.upload(sd)
    u = G.stratum_grid(64)
    tr = Q.light_truth(sc, light, p, u)
    li, wi, pdf = gpu_ctx.light_sample_li(light, np.float32(p), u)
    GC.hold_light("device " + QC.light_id(case), tr, li, wi, pdf, p)


@pytest.mark.parametrize("case", QC.SOLID_ANGLE_CASES, ids=QC.light_id)
def test_device_mean_inverse_pdf_is_the_solid_angle(gpu_ctx, light_scene, case):
    light, p = case
    sd, sc = light_scene
    gpu_ctx.upload(sd)
    QC.hold_solid_angle("device " + QC.light_id(case), sc, light, p, lambda u: gpu_ctx.light_sample_li(light, np.float32(p), u)[2])


@pytest.mark.parametrize("case", QC.LIGHT_CASES, ids=QC.light_id)
def test_device_pdf_from_against_truth(gpu_ctx, light_scene, case):
    """Directions: towards the 64 x 64 sampled points of the light (the float32 wi pt_light_sample_li returns) and as many spread over a
    cone around the light, part of which miss it.  On every direction the truth decides (no rim, no graze, |cos| above the margin):
    pdf == 0 exactly where the truth's is, and within its relative bound elsewhere."""
    light, p = case
    sd, sc = light_scene
    gpu_ctx.upload(sd)
    u = G.stratum_grid(64)
    li, wi_s, pdf_s = gpu_ctx.light_sample_li(light, np.float32(p), u)
    trs = Q.light_truth(sc, light, p, u, quadrature=False)
    rng = np.random.default_rng(17)
    centre = trs["p"].mean(0) - np.asarray(p, np.float64)
    spread = np.linalg.norm(trs["p"] - trs["p"].mean(0), axis=1).max()
    wi_r = centre[None] + rng.standard_normal((len(u), 3)) * 0.8 * spread
    wi_r = (wi_r / np.linalg.norm(wi_r, axis=1)[:, None]).astype(np.float32)          # unit vectors, as pdf_li is given them
    ok_s = pdf_s > 0
    wi = np.concatenate([wi_s[ok_s], wi_r])
    got = gpu_ctx.light_pdf_from(light, np.float32(p), wi).astype(np.float64)
    tr = Q.pdf_from(sc, light, p, wi)
    dec = (tr["rule"] == 0) & (~tr["hit"] | (np.abs(tr["cos"]) > GC.COS_MARGIN))
    left = float((~dec).mean())
    assert ((got == 0) == (tr["pdf"] == 0))[dec].all(), "%d decisive directions differ in hit / miss" % ((got == 0) != (tr["pdf"] == 0))[dec].sum()
    both = dec & (tr["pdf"] > 0)
    ratio = np.abs(got / np.where(both, tr["pdf"], 1.0) - 1.0)[both] / tr["pdf_rel"][both]
    assert both.sum() >= 1000 and (ratio <= 1.0).all(), "pdf off by %.3f of its bound" % ratio.max()
    # pdf_from at a direction sample_from produced is sample_from's pdf, where the sampled point is what the ray meets first
    ns = int(ok_s.sum())
    with np.errstate(all="ignore"):
        same = dec[:ns] & tr["hit"][:ns] & (np.linalg.norm(tr["p"][:ns] - trs["p"][ok_s], axis=1) <= 1e-4 * trs["dist"][ok_s]) & (np.abs(trs["cos"][ok_s]) > 1e-2)
        r2 = np.abs(got[:ns] / pdf_s[ok_s].astype(np.float64) - 1.0)[same] / (tr["pdf_rel"][:ns] + trs["pdf_rel"][ok_s])[same]
    assert same.sum() >= 300 and (r2 <= 1.0).all(), "pdf_from and sample_from disagree by %.3f of their bounds" % r2.max()
    print("device pdf_from %-24s left out %.2f %%  misses %d  err/bound worst %.3f (%d directions); against sample_li's pdf worst %.3f (%d coincide of %d)" % (
        QC.light_id(case), 100 * left, (dec & ~tr["hit"]).sum(), ratio.max(), both.sum(), r2.max(), same.sum(), ns))
    assert left <= GC.MAX_LEFT_OUT
