"""The cases of the `aov` truth (tests/aov_ref.py) and what is asserted on them -- shared by test_aov_host.py, which holds the float32
run of the restatement to its float64 run without a GPU (the calibration), and test_gpu_aov.py, which holds the device to the float64
run.

Every case: a 33 x 17 film (partial 16 x 16 tiles, a partial last wave), the camera inside the unit cube and geometry scaled so that
positions and distances lie in (-1, 1) and v2c does not clamp them.  build(target, scale) -> SceneDesc."""
import os

import numpy as np

import aov_ref as R
import geometry_ref as G
from helpers import scenes
from test_texture_oracle import MAX_LEFT_OUT        # 3 %: the cap the geometry truths use

XRES, YRES = 33, 17
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aov_truth.txt")
MEDIAN_FACTOR = 4.0        # the device's median err / bound against the float32 restatement's: the margin tests/geometry_cases.py gives the device
                           # over the oracle, for the same reason (the same arithmetic in another operation order)


def _builder(target, scale, sampler="sobol", spp=4, lens=0.0, filt="box"):
    b = scenes.SceneBuilder()
    b.look_at((0.05, 0.02, 0.1), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    b.camera_perspective(fov=60.0, lensradius=lens, focaldistance=0.7)
    b.film(XRES, YRES)
    if filt == "gaussian":
        b.pixel_filter_gaussian(1.5, 1.5, 2.0)
    else:
        b.pixel_filter_box()
    if sampler == "halton":
        b.sampler_halton(spp)
    else:
        b.sampler_sobol(spp)
    b.integrator_aov(target, scale)
    return b


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _two_triangles(b):
    """Two tilted triangles with uv, N and S (one mesh each)."""
    for P, uv, tilt in (([(-0.8, -0.5, -0.7), (0.1, -0.5, -0.5), (-0.3, 0.5, -0.6)], [(0.1, 0.2), (0.9, 0.1), (0.4, 0.8)], 0.15),
                        ([(0.0, -0.45, -0.55), (0.8, -0.4, -0.75), (0.5, 0.5, -0.6)], [(0.0, 0.0), (0.7, 0.2), (0.3, 0.9)], -0.2)):
        P = np.array(P, np.float64)
        ng = _unit(np.cross(P[0] - P[2], P[1] - P[2]))
        N = _unit(ng[None] + tilt * np.array([[1.0, 0.0, 0.2], [0.0, 1.0, 0.1], [-0.6, -0.5, 0.0]]))
        S = _unit((P[1] - P[0])[None] + tilt * np.array([[0.0, 0.3, 0.1], [0.2, 0.0, -0.3], [0.1, -0.2, 0.2]]))
        b.shape_trianglemesh(P, [0, 1, 2], N=N, S=S, uv=uv)


def case_frame(target="uv", scale=1.0, **kw):
    b = _builder(target, scale, **kw)
    _two_triangles(b)
    return b.build()


def case_plain(target="uv", scale=1.0, **kw):
    """A quad with neither uv nor N (its two triangles share vertices in different slots: no uv fill) and a triangle whose three uvs coincide."""
    b = _builder(target, scale, **kw)
    b.shape_trianglemesh([(-0.6, -0.4, -0.65), (0.1, -0.42, -0.5), (0.12, 0.38, -0.55), (-0.58, 0.4, -0.62)], [0, 1, 2, 0, 2, 3])
    b.shape_trianglemesh([(0.3, -0.4, -0.5), (0.8, -0.3, -0.7), (0.55, 0.4, -0.6)], [0, 1, 2], uv=[(0.3, 0.3)] * 3)
    return b.build()


def case_sphere(target="uv", scale=1.0, **kw):
    """A partial sphere (phimax 250) under a rotation and a non-uniform scale: its outside, and its inside through the cut."""
    b = _builder(target, scale, sampler="halton", spp=3, **kw)
    t = scenes.transform_mul(scenes.transform_translate(0.05, 0.0, -0.75), scenes.transform_mul(scenes.transform_rotate_x(35.0), scenes.transform_scale(1.2, 0.7, 0.9)))
    b.shape_sphere(radius=0.5, zmin=-0.4, zmax=0.45, phimax=250.0, object_to_world=t[0], world_to_object=t[1])
    return b.build()


def case_instances(target="uv", scale=1.0, **kw):
    """One object (a quad with uv and N) instanced twice, the second instance mirrored in x."""
    b = _builder(target, scale, **kw)
    P = np.array([(-0.3, -0.35, 0.0), (0.3, -0.3, 0.05), (0.25, 0.35, -0.05), (-0.28, 0.3, 0.02)], np.float64)
    N = _unit(np.array([0.0, 0.0, 1.0])[None] + 0.2 * np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]))
    b.object_begin("quad")
    b.shape_trianglemesh(P, [0, 1, 2, 0, 2, 3], N=N, uv=[(0.0, 0.0), (1.0, 0.1), (0.9, 1.0), (0.1, 0.8)])
    b.object_end()
    b.object_instance("quad", scenes.transform_translate(-0.35, 0.0, -0.7))
    b.object_instance("quad", scenes.transform_mul(scenes.transform_translate(0.4, 0.02, -0.6), scenes.transform_scale(-1.0, 1.1, 1.0)))
    return b.build()


def case_bump(target="uv", scale=1.0, bump="bilerp", **kw):
    """A matte quad bump-mapped by a bilerp displacement that is linear in uv (the finite differences of material_bump are exact).
    bump "fbm": an fbm displacement (held only to "the normal moved and is a unit vector"); None: the same quad without a bump map."""
    b = _builder(target, scale, **kw)
    if bump == "bilerp":
        b.material_matte(bumpmap=b.texture_bilerp(v00=0.01, v01=0.05, v10=0.04, v11=0.08))
    elif bump == "fbm":
        b.material_matte(bumpmap=b.texture_scale(b.texture_fbm(octaves=4, roughness=0.6, to_world=scenes.transform_scale(8.0, 8.0, 8.0)), 0.05))
    b.shape_trianglemesh([(-0.7, -0.45, -0.75), (0.7, -0.4, -0.55), (0.65, 0.45, -0.6), (-0.65, 0.4, -0.8)], [0, 1, 2, 0, 2, 3],
                         uv=[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
    return b.build()


def case_lens(target="uv", scale=1.0, **kw):
    """lensradius > 0: the offset rays leave the lens point, rx_origin differs from the camera's position."""
    b = _builder(target, scale, lens=0.05, **kw)
    _two_triangles(b)
    return b.build()


def case_reports(target="uv", scale=1.0, **kw):
    """A surface with Material "none", an emissive triangle, and rays that miss."""
    b = _builder(target, scale, **kw)
    b.material_none()
    b.shape_trianglemesh([(-0.8, -0.5, -0.7), (-0.05, -0.5, -0.5), (-0.4, 0.45, -0.6)], [0, 1, 2], uv=[(0.1, 0.2), (0.9, 0.1), (0.4, 0.8)])
    b.material_matte()
    b.area_light_source_diffuse(L=(3.0, 3.0, 3.0))
    b.shape_trianglemesh([(0.1, -0.4, -0.55), (0.7, -0.35, -0.7), (0.45, 0.3, -0.6)], [0, 1, 2], uv=[(0.0, 0.0), (0.7, 0.2), (0.3, 0.9)])
    b.no_area_light()
    return b.build()


ALPHA_CHECKS = 4.0        # the mask: a checkerboard of 4 x 4 cells over the front quad's uv, 1 / 0


def case_alpha(target="uv", scale=1.0, front=True, **kw):
    """A quad behind (declared first: its primitive numbers do not depend on `front`) and a checkerboard-alpha quad in front of it."""
    b = _builder(target, scale, **kw)
    b.shape_trianglemesh([(-0.5, -0.35, -0.55), (0.5, -0.35, -0.5), (0.5, 0.35, -0.58), (-0.5, 0.35, -0.6)], [0, 1, 2, 0, 2, 3],
                         uv=[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
    if front:
        mask = b.texture_checkerboard(1.0, 0.0, uscale=ALPHA_CHECKS, vscale=ALPHA_CHECKS)
        b.shape_trianglemesh([(-0.3, -0.2, -0.28), (0.3, -0.21, -0.32), (0.31, 0.2, -0.35), (-0.29, 0.21, -0.3)], [0, 1, 2, 0, 2, 3],
                             uv=[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], alpha=mask)
    return b.build()


def alpha_hits(o, d):
    """The truth's hits of the alpha case: the front quad's where its mask is 1, else the quad's behind.  Returns (hits, undecided)."""
    from alpha_mask_ref import Checker, Const
    sd_full, sd_back = case_alpha(), case_alpha(front=False)
    tmax = np.full(len(o), np.inf, np.float32)
    hf, hb = G.closest_hits(sd_full, o, d, tmax), G.closest_hits(sd_back, o, d, tmax)
    on_front = (hf["kind"] != G.MISS) & (hf["prim"] >= 2)
    first = R.evaluate(sd_full, o, d, np.zeros((len(o), 2), np.float32), np.zeros((len(o), 2), np.float32), hf, np.float64)
    uv = first["value"]["uv"]
    val, near = Checker(Const(1.0), Const(0.0), uscale=ALPHA_CHECKS, vscale=ALPHA_CHECKS).val(uv[:, 0], uv[:, 1])
    cut = on_front & (val <= 0)
    hits = {k: np.where(cut, hb[k], hf[k]) for k in hf}
    return hits, (hits["rule"] != 0) | (on_front & (near | (hf["rule"] != 0)))


CASES = {"frame": case_frame, "plain": case_plain, "sphere": case_sphere, "instances": case_instances, "bump": case_bump, "lens": case_lens,
         "reports": case_reports, "alpha": case_alpha}


def truth_hits(name, sd, o, d):
    """geometry_ref's hits of a case's rays and the samples they leave undecided."""
    if name == "alpha":
        return alpha_hits(o, d)
    h = G.closest_hits(sd, o, d, np.full(len(o), np.inf, np.float32))
    return h, h["rule"] != 0


def pixel_samples(sd, spp, bounds=(0, 0, XRES, YRES)):
    """(pixel_xy, sample_index) of every camera sample of the sample bounds (x0, y0, x1, y1), pixel-major as pt_radiance_samples reports them."""
    xs, ys = np.meshgrid(np.arange(bounds[0], bounds[2]), np.arange(bounds[1], bounds[3]))
    px = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32)
    return np.repeat(px, spp, 0), np.tile(np.arange(spp, dtype=np.uint32), len(px))


def check(name, got, truth, und, medians=None, report=None):
    """err <= bound outside the left-out set, left-out share <= 3 % per target.  got: {target: (n, 3)} of the implementation under test;
    truth: aov_ref.evaluate's float64 result; und: samples left out by rule.  Returns {target: (worst, median) of err / bound}."""
    out = {}
    keep = ~und
    for k in R.TARGETS:
        assert und.mean() <= MAX_LEFT_OUT, (name, k, "left out", und.mean())
        err = np.abs(got[k].astype(np.float64) - truth["value"][k])[keep]
        bound = truth["bound"][k][keep]
        hitk = truth["hit"][keep]
        if k == "rdyc" or not hitk.any():
            assert not err.any(), (name, k, "must be exactly 0")
            out[k] = (0.0, 0.0)
            continue
        assert not err[~hitk].any(), (name, k, "a miss must report exactly 0")
        e, b = err[hitk], bound[hitk]
        ratio = np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e > 0, np.inf, 0.0))
        nz = ratio[b > 0]
        out[k] = (float(ratio.max()), float(np.median(nz)) if len(nz) else 0.0)
        if report is not None:
            report.append("%-10s %-9s worst %.6e median %.6e" % (name, k, out[k][0], out[k][1]))
        assert ratio.max() <= 1.0, (name, k, "err / bound", float(ratio.max()), int(np.argmax(ratio.max(1) if ratio.ndim > 1 else ratio)))
        if medians is not None and (name, k) in medians and medians[(name, k)] > 0:
            assert out[k][1] <= MEDIAN_FACTOR * medians[(name, k)], (name, k, "median err / bound", out[k][1], "float32 restatement", medians[(name, k)])
    return out


def read_medians():
    med = {}
    if os.path.exists(PROFILE):
        for line in open(PROFILE):
            f = line.split()
            if len(f) == 6 and f[2] == "worst":
                med[(f[0], f[1])] = float(f[5])
    return med


XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])


def fold_film(sd, p_film, rgb):
    """Film (X, Y, Z, weight) from per-sample values in float64: FilmTile::add_sample_filter with the footprint's weights normalised to
    sum 1 (quirk Q1), Film's 16 x 16 table lookup (film_tile.rs:84-183)."""
    d = sd.desc
    rx, ry = float(d.filter_radius[0]), float(d.filter_radius[1])
    tab = np.array(list(d.filter_table), np.float64).reshape(16, 16)
    film = np.zeros((YRES, XRES, 4))
    for (fx, fy), l in zip(np.asarray(p_film, np.float64), np.asarray(rgb, np.float64)):
        x0, y0 = max(int(np.floor(fx - rx)), 0), max(int(np.floor(fy - ry)), 0)
        x1, y1 = min(int(np.ceil(fx + rx)), XRES), min(int(np.ceil(fy + ry)), YRES)
        ws = []
        for y in range(y0, y1):
            for x in range(x0, x1):
                dx, dy = abs(np.float32(x + 0.5) - np.float32(fx)), abs(np.float32(y + 0.5) - np.float32(fy))
                if not (dx <= np.float32(rx)) or not (dy <= np.float32(ry)):
                    continue
                ix = min(int(np.floor(np.float32(dx) * (np.float32(1.0 / np.float32(rx)) * np.float32(15.0)))), 15)
                iy = min(int(np.floor(np.float32(dy) * (np.float32(1.0 / np.float32(ry)) * np.float32(15.0)))), 15)
                ws.append((x, y, tab[iy, ix]))
        s = sum(w for _, _, w in ws)
        if s <= 0:
            continue
        for x, y, w in ws:
            film[y, x, :3] += XYZ_FROM_RGB @ l * (w / s)
            film[y, x, 3] += w / s
    return film
