"""Integrator "aov" over a cylinder seen from outside and from inside and a disk seen from both faces: `distance`, `n`, `ns`, `uv`, `dpdu`
and `dpdv` of every camera sample (16 x 16 at 4 spp, Sobol' and Halton) held to the float64 interaction of quadric_ref.interaction.

Bounds.  With B the truth's bound on t (origin shift included), the object-space hit point is off by at most
    e = |d| B + |o_err + |t| d_err| + gamma(4) |p|
(the ray's own error terms through the matrix, t's error along the ray, the roundings of o + t d and of the refinement).  Every target is a
smooth function of that point, so its bound is its Lipschitz constant times e plus the roundings of its own few operations:
    u = phi / phi_max            e / (rho phi_max) + gamma(10) 2 pi / phi_max        (atan2 to a few ulp of its range)
    v (cylinder)                 e / (zmax - zmin) + gamma(4) (|z| + |zmin|) / (zmax - zmin)
    v (disk)                     e / (r - ri) + gamma(5) (r + rho) / (r - ri)
    dpdu = phi_max (-y, x, 0)    phi_max e + gamma(3) |dpdu|, through |object_to_world| with gamma(4) more
    dpdv (cylinder)              constant: gamma(5) |object_to_world| |dpdv|
    dpdv (disk) = (x, y, 0) (ri - r) / rho        2 (r - ri) e / rho + gamma(6) |dpdv|, through |object_to_world|
    n (cylinder) = (x, y, 0) / r                  e / r + gamma(12), then 2 s_max(world_to_object) / |world_to_object^T n| for the normalised transform
    n (disk)                     constant: gamma(12); its sign is the ray's side, undecided where |d.z| <= 4 d_err.z
    distance = t / |d|           B / |d| + gamma(6) distance
and v2c (x / 2 + 1 / 2, clamped) halves a bound and adds an ulp of 1.  Samples the truth leaves out (rims, grazes) are left out here; their
share is capped at 3 %.

`dpdx` / `dpdy` (compute_differentials over the new p, n, dpdu, dpdv and the camera's offset rays) and, on a bump-mapped shape, `ns`, `dpdus`
and `dpdvs` (material_bump reads dndu / dndv: the cylinder's Weingarten terms) are held by the other route: quadric_ref.interaction_E carries
a first-order bound beside every value in aov_ref's E arithmetic, and aov_ref's own camera model, compute_differentials and bump
restatement run on its result."""
import numpy as np
import pytest

import geometry_ref as G
import quadric_ref as Q
from geometry_ref import gamma
from helpers import scenes
from test_texture_oracle import MAX_LEFT_OUT

pytestmark = pytest.mark.gpu
T = scenes
TARGETS = ("distance", "n", "ns", "uv", "dpdu", "dpdv")

# view -> (shape, eye, look)
VIEWS = {
    "cylinder_outside": ("cylinder", (0.55, -0.5, 0.2), (0.0, 0.0, 0.0)),
    "cylinder_inside": ("cylinder", (0.02, 0.03, -0.05), (0.1, 0.12, 0.05)),
    "disk_front": ("disk", (0.2, -0.3, 0.55), (0.0, 0.0, 0.0)),
    "disk_back": ("disk", (-0.25, 0.2, -0.6), (0.0, 0.0, 0.0)),
}


def _scene(view, target, sampler, bump=False):
    shape, eye, look = VIEWS[view]
    b = scenes.SceneBuilder()
    b.look_at(eye, look, (0, 0, 1) if shape == "cylinder" else (0, 1, 0))
    b.camera_perspective(fov=55.0)
    b.film(xresolution=16, yresolution=16)
    b.pixel_filter_box()
    b.sampler_sobol(4) if sampler == "sobol" else b.sampler_halton(4)
    b.integrator_aov(target=target, scale=1.0)
    b.material_matte((0.5, 0.5, 0.5), bumpmap=b.texture_bilerp(v00=0.01, v01=0.05, v10=0.04, v11=0.08) if bump else None)
    t = T.transform_mul(T.transform_translate(0.01, -0.02, 0.015), T.transform_mul(T.transform_rotate_x(12.0), T.transform_scale(1.0, 0.9, 1.1)))
    if shape == "cylinder":
        b.shape_cylinder(radius=0.15, zmin=-0.4, zmax=0.35, phimax=330.0, object_to_world=t[0], world_to_object=t[1])
    else:
        b.shape_disk(height=0.02, radius=0.3, innerradius=0.04, phimax=320.0, object_to_world=t[0], world_to_object=t[1])
    return b.build()


def _truth(sd, o, d):
    """{target: (value, bound)} of the v2c'd outputs, the hit mask and the left-out mask."""
    sp = Q._Quadric(sd.buffers["spheres"][0])
    n = len(o)
    tr = Q.single_shape_hits(sp, o, d, np.full(n, np.inf, np.float32))
    with np.errstate(all="ignore"):
        it = Q.interaction(sp, o, d, np.float64, t=tr["t"])
    O, D, oerr, derr, _ = G._transform_rays([sp.w2o], o.astype(np.float64), d.astype(np.float64))
    hit = tr["hit"]
    und = tr["rule"] != 0
    with np.errstate(all="ignore"):
        t, B = tr["t"], tr["bound"]
        p = O + t[:, None] * D
        e = np.linalg.norm(D, axis=1) * B + np.linalg.norm(oerr + np.abs(t)[:, None] * derr, axis=1) + gamma(4) * np.linalg.norm(p, axis=1)
        A, Ai = np.abs(sp.o2w[:3, :3]), sp.w2o[:3, :3]
        rho = np.hypot(p[:, 0], p[:, 1])
        e_u = e / (rho * sp.phimax) + gamma(10) * 2 * np.pi / sp.phimax
        dpdu_o = sp.phimax * np.stack([-p[:, 1], p[:, 0], 0 * rho], 1)
        e_dpdu = (sp.phimax * e + gamma(3) * np.linalg.norm(dpdu_o, axis=1))[:, None] * A.sum(1)[None, :] + gamma(4) * (np.abs(dpdu_o) @ A.T)
        if sp.kind == Q.SHAPE_CYLINDER:
            dz = sp.zmax - sp.zmin
            e_v = e / dz + gamma(4) * (np.abs(p[:, 2]) + abs(sp.zmin)) / dz
            e_dpdv = np.repeat((gamma(5) * (A @ np.array([0.0, 0.0, dz])))[None], n, 0)
            e_n_obj = e / sp.r + gamma(12)
        else:
            e_v = e / (sp.r - sp.ri) + gamma(5) * (sp.r + rho) / (sp.r - sp.ri)
            dpdv_o = np.stack([p[:, 0], p[:, 1], 0 * rho], 1) * ((sp.ri - sp.r) / rho)[:, None]
            e_dpdv = (2 * (sp.r - sp.ri) * e / rho + gamma(6) * np.linalg.norm(dpdv_o, axis=1))[:, None] * A.sum(1)[None, :]
            e_n_obj = np.full(n, gamma(12))
            und |= hit & (np.abs(D[:, 2]) <= 4 * derr[:, 2])
        smax = np.linalg.norm(Ai, 2)
        n_obj_len = np.linalg.norm(it["n"] @ sp.o2w[:3, :3], axis=1)          # |o2w^T n_w| = 1 / |w2o^T n_obj| up to the normalisation
        e_n = (2 * smax * e_n_obj * n_obj_len + gamma(12))[:, None] * np.ones(3)
        dlen = np.linalg.norm(d.astype(np.float64), axis=1)
        dist = t / dlen
        e_dist = B / dlen + gamma(6) * dist

    def v2c(v, ev):
        return np.clip(v * 0.5 + 0.5, 0.0, 1.0), 0.5 * ev + 2.0 ** -23

    out = {"n": v2c(it["n"], e_n), "dpdu": v2c(it["dpdu"], e_dpdu), "dpdv": v2c(it["dpdv"], e_dpdv)}
    out["ns"] = out["n"]
    out["distance"] = (np.repeat(np.clip(dist, 0, 1)[:, None], 3, 1), np.repeat((e_dist + 2.0 ** -24)[:, None], 3, 1))
    uv = np.stack([np.clip(it["uv"][:, 0], 0, 1), np.clip(it["uv"][:, 1], 0, 1), 0 * rho], 1)
    out["uv"] = (uv, np.stack([e_u + 2.0 ** -24, e_v + 2.0 ** -24, 0 * rho], 1))
    return out, hit, und, it


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("view", list(VIEWS))
def test_targets_against_the_float64_interaction(gpu_ctx, view, sampler):
    got = {}
    for target in TARGETS:
        sd = _scene(view, target, sampler)
        info = gpu_ctx.upload(sd)
        sb = tuple(info.sample_bounds)
        got[target] = gpu_ctx.radiance_samples(sb).reshape(-1, 3).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(sb[0], sb[2]), np.arange(sb[1], sb[3]))
    px = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32), info.spp, 0)
    si = np.tile(np.arange(info.spp, dtype=np.uint32), len(xs.reshape(-1)))
    o, d, _ = gpu_ctx.generate_camera_rays(px, si)
    truth, hit, und, it = _truth(sd, o, d)
    keep = hit & ~und
    left = float(und.mean())
    assert left <= MAX_LEFT_OUT, "%s: %.2f %% left out" % (view, 100 * left)
    assert keep.sum() >= 300, "%s: only %d samples on the shape" % (view, keep.sum())
    if view.startswith("disk"):            # the disk's normal faces the camera from either side
        assert ((it["n"][keep] * -d[keep].astype(np.float64)).sum(1) > 0).all()
    line = []
    for target in TARGETS:
        val, bound = truth[target]
        err, b = np.abs(got[target] - val)[keep], bound[keep]
        ratio = (err / np.where(b > 0, b, 1.0))[b > 0]
        line.append("%s %.3f" % (target, ratio.max()))
        assert (err <= b).all(), "%s %s %s: worst err / bound %.3f" % (view, sampler, target, ratio.max())
        miss = ~hit & ~und
        assert not got[target][miss].any()          # a camera ray that escapes is black
    assert np.array_equal(got["n"], got["ns"])
    print("%-17s %-7s left out %.2f %%, %d samples on the shape; worst err / bound: %s" % (view, sampler, 100 * left, keep.sum(), ", ".join(line)))
    gpu_ctx.reset_counters()


def _truth_E(sd, o, d, pf):
    """aov_ref's E arithmetic over quadric_ref.interaction_E: {target: (value, bound)} of dpdx, dpdy and (bumped or not) ns, dpdus, dpdvs."""
    import aov_ref as R
    ps = sd.buffers["spheres"][0]
    sp = Q._Quadric(ps)
    n = len(o)
    tr = Q.single_shape_hits(sp, o, d, np.full(n, np.inf, np.float32))
    und = tr["rule"] != 0
    with np.errstate(all="ignore"):
        s = Q.interaction_E(ps, R.vexact(o, np.float64), R.vexact(d, np.float64), R.E(tr["t"], tr["bound"]), np.float64, und)
        diffs = R.differentials(R.Camera(sd), o, d, pf, np.zeros((n, 2), np.float32), np.float64)
        df = R._compute_differentials(s, *diffs, und)
        m = sd.buffers["materials"][ps.material]
        if m.tex_bump:
            s = R._bump(sd.buffers["textures"][m.tex_bump - 1], s, df, und)
        res = {"dpdx": R._v2c(df["dpdx"], 1.0), "dpdy": R._v2c(df["dpdy"], 1.0), "ns": R._v2c(s["sh_n"], 1.0), "dpdus": R._v2c(s["sh_dpdu"], 1.0),
               "dpdvs": R._v2c(s["sh_dpdv"], 1.0)}
    out = {k: (np.stack([c.v for c in v], 1), np.stack([c.e for c in v], 1)) for k, v in res.items()}
    return out, tr["hit"], und, s


def _render(gpu_ctx, view, sampler, targets, bump):
    got = {}
    for target in targets:
        sd = _scene(view, target, sampler, bump=bump)
        info = gpu_ctx.upload(sd)
        sb = tuple(info.sample_bounds)
        got[target] = gpu_ctx.radiance_samples(sb).reshape(-1, 3).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(sb[0], sb[2]), np.arange(sb[1], sb[3]))
    px = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32), info.spp, 0)
    si = np.tile(np.arange(info.spp, dtype=np.uint32), len(xs.reshape(-1)))
    o, d, pf = gpu_ctx.generate_camera_rays(px, si)
    gpu_ctx.reset_counters()
    return sd, got, o, d, pf


def _hold(label, got, truth, keep, targets):
    line = []
    for target in targets:
        val, bound = truth[target]
        err, b = np.abs(got[target] - val)[keep], bound[keep]
        assert np.isfinite(b).all(), (label, target)
        ratio = (err / np.where(b > 0, b, 1.0))[b > 0]
        line.append("%s %.3f (values %.3f..%.3f)" % (target, ratio.max(), val[keep].min(), val[keep].max()))
        assert (err <= b).all(), "%s %s: worst err / bound %.3f" % (label, target, ratio.max())
    print("%-32s %d samples; worst err / bound: %s" % (label, keep.sum(), ", ".join(line)))


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("view", list(VIEWS))
def test_dpdx_against_compute_differentials(gpu_ctx, view, sampler):
    targets = ("dpdx", "dpdy")
    sd, got, o, d, pf = _render(gpu_ctx, view, sampler, targets, bump=False)
    truth, hit, und, _ = _truth_E(sd, o, d, pf)
    keep = hit & ~und
    assert und.mean() <= MAX_LEFT_OUT and keep.sum() >= 300
    _hold("%s %s" % (view, sampler), got, truth, keep, targets)
    assert got["dpdx"][keep].std(0).max() > 1e-4          # the target is not a constant: the offset rays land somewhere else on the shape


@pytest.mark.parametrize("view", ["cylinder_outside", "cylinder_inside", "disk_front"])
def test_bump_mapped_shading_frame_reads_dndu(gpu_ctx, view):
    """A bilerp bump map on the shape: material_bump builds the shading dpdu / dpdv from dpdu + (du_disp) n + disp dndu -- the only reader of
    the cylinder's Weingarten terms -- and the shading normal from their cross product."""
    targets = ("ns", "dpdus", "dpdvs")
    sd, got, o, d, pf = _render(gpu_ctx, view, "sobol", targets, bump=True)
    truth, hit, und, s = _truth_E(sd, o, d, pf)
    keep = hit & ~und
    assert und.mean() <= MAX_LEFT_OUT and keep.sum() >= 300
    _hold("%s bumped" % view, got, truth, keep, targets)
    _, plain, _, _, _ = _render(gpu_ctx, view, "sobol", ("ns",), bump=False)
    assert np.abs(plain["ns"] - got["ns"])[keep].max() > 1e-3          # the bump map moved the shading normal
    if view.startswith("cylinder"):          # ... and dndu is in it: dropping the disp * dndu term (disp >= 0.01) would move dpdus by many bounds
        term = 0.5 * 0.01 * np.abs(np.stack([c.v for c in s["sh_dndu"]], 1))[keep].max(1)
        assert np.median(term / truth["dpdus"][1][keep].max(1)) > 20
