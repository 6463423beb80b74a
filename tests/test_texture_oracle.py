"""The oracle's texture evaluator (orc_texture.hpp, through orc_texture_eval) held to the float64 restatements of texture_ref.py, on
identical float32 inputs; the two tables the device and the oracle share held to the reference's recipe and digest; and the filtered
value as the oracle renders it (a textured mirror lit with radiance 1 from every direction) held to a float64 pipeline from the scene description.

Every comparison is texture_ref.judge: |oracle - float64| <= the bound derived for that evaluation; evaluations next to a discontinuity
or whose bound exceeds 1e-3 of their scale are left out, and the share left out, printed per case, may not exceed 3 %."""
import hashlib
import os
import re

import numpy as np
import pytest

import feature_scenes as fs
import texture_ref as R
from helpers import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEFT_OUT = 0.03
NOISE_PERM_SHA256 = "3682c3d0020436c45462995a4f64438c144bbfeba725b00de5906ab322b6b915"       # of the 256 bytes of NOISEPERM[..256], noise.rs:31-44


def _macro_body(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    body = text[text.index("#define " + name) + len("#define " + name):]
    end = re.search(r"[^\\]\n", body)
    return body[:end.end()].replace("\\\n", " ")


def shared_noise_perm():
    """PT_NOISE_PERM_256 of include/pbrtgpu_noise_perm.h, accepted only with the digest of the reference's table: texture_ref.noise is
    handed this permutation, so that the table is not written out a third time."""
    v = np.array([int(x) for x in re.findall(r"\d+", _macro_body("pbrtgpu_noise_perm.h", "PT_NOISE_PERM_256"))], np.int64)
    assert len(v) == 256 and sorted(v.tolist()) == list(range(256))
    assert hashlib.sha256(bytes(v.astype(np.uint8).tolist())).hexdigest() == NOISE_PERM_SHA256
    return v


# ---------------------------------------------------------------------------------------------------------------- the two tables
def test_noise_permutation_is_the_references():
    shared_noise_perm()


def test_ewa_weight_table_is_the_references_recipe():
    """Bit for bit the table of the reference's build script (build_mipmap_weight_lut.rs:14-42), recomputed here; tools/make_ewa_lut.py,
    which generated the header, is checked by the same comparison."""
    vals = [float.fromhex(x.rstrip("f")) for x in re.findall(r"-?0x[0-9a-fA-F.]+p[-+]?\d+f?", _macro_body("pbrtgpu_ewa_lut.h", "PT_EWA_LUT_VALUES"))]
    got = np.array(vals, np.float64).astype(np.float32)
    want = R.ewa_lut()
    assert len(vals) == 128 and np.array_equal(got.astype(np.float64), np.array(vals))          # every entry is an f32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want[127] == 0.0 and np.all(np.diff(want) < 0)


# ---------------------------------------------------------------------------------------------------------------- plumbing
class Bench:
    """Textures of several specs in one oracle scene (a scene needs a primitive: one triangle nobody looks at)."""

    def __init__(self, oracle, specs):
        b = scenes.SceneBuilder()
        self.tex = [fs.texture_from_spec(b, s) for s in specs]
        b.material_matte()
        b.shape_trianglemesh(np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32), [0, 1, 2])
        self.sd = b.build()
        self.osc = oracle.scene(self.sd)
        self.ref = [fs.texture_ref_spec(s, R.pyramid) for s in specs]

    def close(self):
        self.osc.close()


def hold(bench, k, perm=None, **inputs):
    """Evaluate texture k of the bench on float32 `inputs` by the oracle and by float64; returns (excess, share left out, report)."""
    f32 = {n: np.ascontiguousarray(a, np.float32) for n, a in inputs.items()}
    n = len(next(iter(f32.values())))
    got = bench.osc.texture_eval(bench.tex[k], **f32)
    val, bound, scale = R.evaluate(bench.ref[k], R.Hit(n, **{a: v.astype(np.float64) for a, v in f32.items()}), perm)
    excess, left, i = R.judge(got, val, bound, scale)
    return excess, left, "worst #%d: oracle %s float64 %s bound %.3g inputs %s" % (i, got[i], val[i], bound[i], {a: v[i].tolist() for a, v in f32.items()})


class Tally:
    """The evaluations of one case.  The cap on the share left out holds for the case and for every spec (texture setting) in it, so
    that no single wrap pair or maxanisotropy can be left out wholesale behind the others."""

    def __init__(self, name):
        self.name, self.n, self.left, self.per_spec = name, 0, 0.0, {}

    def add(self, n, res, spec=0):
        excess, left, report = res
        assert excess <= 0.0, "%s: beyond the bound by %.3g; %s" % (self.name, excess, report)
        self.n += n
        self.left += left * n
        k = self.per_spec.setdefault(spec, [0, 0.0])
        k[0] += n
        k[1] += left * n

    def done(self, at_least=10000):
        share = self.left / self.n
        worst = max(v[1] / v[0] for v in self.per_spec.values())
        print("texture truth [%s]: %d evaluations, left out %.2f %%%s" % (self.name, self.n, 100 * share,
                                                                          ", %.2f %% in the worst of %d specs" % (100 * worst, len(self.per_spec)) if len(self.per_spec) > 1 else ""))
        assert self.n >= at_least, self.n
        assert share <= MAX_LEFT_OUT, "%s: %.2f %% left out" % (self.name, 100 * share)
        assert worst <= MAX_LEFT_OUT, "%s: %.2f %% left out in one spec" % (self.name, 100 * worst)


def waves_image(w, h, c, seed, noise=0.25):
    """Texels in [0, 1]: low-frequency waves plus white noise of a quarter of the range, so that neighbouring texels differ by a fraction
    of the range, as photographs do."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, c), np.float32)
    for k in range(c):
        fx, fy, ph = rng.integers(1, 3), rng.integers(1, 3), rng.uniform(0, 6.28)
        out[:, :, k] = 0.5 + 0.25 * np.sin(2 * np.pi * (fx * x / max(w, 2) + fy * y / max(h, 2)) + ph) + noise * rng.uniform(-1, 1, (h, w))
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def footprints(rng, n, lo=1e-3, hi=0.5, max_aniso=40.0, st_lo=-0.5, st_hi=1.5):
    """Log-uniform size, anisotropy 1 .. max_aniso, random orientation, the two axes within +-0.6 rad of perpendicular."""
    st = rng.uniform(st_lo, st_hi, (n, 2))
    size = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    aniso = np.exp(rng.uniform(0, np.log(max_aniso), n))
    th = rng.uniform(0, 2 * np.pi, n)
    ph = th + np.pi / 2 + rng.uniform(-0.6, 0.6, n)
    d0 = size[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    d1 = (size / aniso)[:, None] * np.stack([np.cos(ph), np.sin(ph)], 1)
    flip = rng.random(n) < 0.5                                           # the longer axis comes first or second
    d0, d1 = np.where(flip[:, None], d1, d0), np.where(flip[:, None], d0, d1)
    return dict(uv=st, dudx=d0[:, 0], dvdx=d0[:, 1], dudy=d1[:, 0], dvdy=d1[:, 1])


def directed_footprints(levels_n, max_aniso, rng, m=40):
    """The branches of lookup_delta on purpose, m of each."""
    one = np.ones(m)
    st = rng.uniform(-0.25, 1.25, (m, 2))
    r = np.exp(rng.uniform(np.log(2e-3), np.log(0.3), m))
    th = rng.uniform(0, 2 * np.pi, m)
    c, s = np.cos(th), np.sin(th)
    z = 0 * one
    rows = []
    add = lambda a, b2, st_=st: rows.append((st_, np.stack(a, 1), np.stack(b2, 1)))
    add((r * c, r * s), (-r * s, r * c))                                 # exactly isotropic (up to rounding), |dst0| == |dst1|: no swap
    add((r, z), (z, r))                                                  # axis-aligned circle
    add((r * c, r * s), (r * c, r * s))                                  # dst0 == dst1: a degenerate ellipse
    add((r * c, r * s), (z, z))                                          # one of them zero: lookup(st, 0)
    add((z, z), (r * c, r * s))
    add((z, z), (z, z))                                                  # both zero
    for k in (0.98, 1.02):                                               # minor axis just above / below major / maxanisotropy
        add((r * c, r * s), (-r * s / max_aniso * k, r * c / max_aniso * k))
    add((r, z), (z, r / 7.0))                                            # axis-aligned ellipses
    add((z, r / 7.0), (r, z))
    q = np.sqrt(0.5)
    add((r * q, r * q), (-r * q / 5.0, r * q / 5.0))                     # 45 degrees
    tiny = np.exp(rng.uniform(np.log(2.0 ** -(levels_n + 6)), np.log(2.0 ** -(levels_n + 1)), m))
    add((tiny * c, tiny * s), (-tiny * s, tiny * c))                     # lod below 0
    for lod_from_top in (1.5, 0.5, 0.0, -0.5, -1.5):                     # both EWA levels, ilod + 1 == levels, at and beyond the last level
        ml = 2.0 ** (-lod_from_top) * one
        add((2 * ml * c, 2 * ml * s), (-ml * s, ml * c))
    far = np.round(rng.uniform(-1e3, 1e3, (m, 2))) + rng.integers(0, 64, (m, 2)) / 64.0      # |st| up to 1e3, on the texel grid's sixty-fourths
    add((r * c, r * s), (-r * s / 3.0, r * c / 3.0), far)
    add((r * c, r * s), (-r * s / 3.0, r * c / 3.0), -np.abs(st) - 1.0)  # negative st
    st_, d0, d1 = (np.concatenate([x[i] for x in rows]) for i in range(3))
    return dict(uv=st_, dudx=d0[:, 0], dvdx=d0[:, 1], dudy=d1[:, 0], dvdy=d1[:, 1])


IMAGE_SIZES = [(64, 32), (32, 64), (1, 16), (16, 1), (1, 1), (2, 2)]
WRAP_PAIRS = [(a, b) for a in (R.REPEAT, R.BLACK, R.CLAMP) for b in (R.REPEAT, R.BLACK, R.CLAMP)]


# ---------------------------------------------------------------------------------------------------------------- image maps
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("size", IMAGE_SIZES, ids=["%dx%d" % s for s in IMAGE_SIZES])
def test_image_map_ewa(oracle, size, channels):
    """lookup_delta and ewa: maxanisotropy 1 / 8 / 16 x the nine wrap pairs, random and directed footprints."""
    w, h = size
    img = waves_image(w, h, channels, seed=w * 7 + h)
    specs = [dict(type="imagemap", image=img, maxanisotropy=ma, swrap=sw, twrap=tw) for ma in (1.0, 8.0, 16.0) for sw, tw in WRAP_PAIRS]
    bench = Bench(oracle, specs)
    rng = np.random.default_rng(11)
    tally = Tally("imagemap ewa %dx%d c%d" % (w, h, channels))
    for k, spec in enumerate(specs):
        tally.add(340, hold(bench, k, **footprints(rng, 340)), k)
        d = directed_footprints(len(bench.ref[k]["levels"]), spec["maxanisotropy"], rng, m=4)
        tally.add(len(d["uv"]), hold(bench, k, **d), k)
    bench.close()
    tally.done()


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("size", IMAGE_SIZES, ids=["%dx%d" % s for s in IMAGE_SIZES])
def test_image_map_trilinear(oracle, size, channels):
    w, h = size
    img = waves_image(w, h, channels, seed=w * 5 + h)
    specs = [dict(type="imagemap", image=img, trilinear=True, swrap=sw, twrap=tw) for sw, tw in WRAP_PAIRS]
    bench = Bench(oracle, specs)
    rng = np.random.default_rng(12)
    tally = Tally("imagemap trilinear %dx%d c%d" % (w, h, channels))
    for k in range(len(specs)):
        tally.add(1100, hold(bench, k, **footprints(rng, 1100, lo=1e-4, hi=2.0)), k)
        d = directed_footprints(len(bench.ref[k]["levels"]), 8.0, rng, m=4)
        tally.add(len(d["uv"]), hold(bench, k, **d), k)
    bench.close()
    tally.done()


def test_pyramid_is_the_references(oracle):
    """image_pyramid (the front end's) against texture_ref.pyramid: the same float32 texels, every size and channel count used here."""
    for (w, h) in IMAGE_SIZES:
        for c in (1, 3):
            img = waves_image(w, h, c, seed=1)
            b = scenes.SceneBuilder()
            buf = b.images[b.image_pyramid(img if c == 3 else img[:, :, 0])][1]
            lv = R.pyramid(img)
            assert [l.shape[:2] for l in lv][-1] == (1, 1) and len(lv) == 1 + int(np.log2(max(w, h)))
            assert np.array_equal(buf.view(np.uint32), np.concatenate([l.reshape(-1) for l in lv]).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- mappings
def _surface_points(rng, n, kind):
    """Points around the origin at radius 0.5 .. 2 with differentials of 0.05 .. 0.5 (the finite differences of the angular mappings
    divide by 0.1: a smaller footprint leaves nothing of them in float32), and the directed ones: the poles, both sides of the phi seam."""
    v = rng.standard_normal((n, 3))
    p = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.5, 2.0, (n, 1))
    m = n // 10
    p[:m, 1] = rng.choice([-1.0, 1.0], m) * np.exp(rng.uniform(np.log(1e-6), np.log(1e-2), m))      # next to the seam half-planes, both signs
    p[:m, 0] = np.abs(p[:m, 0]) * (1.0 if kind == "spherical" else -1.0)
    p[m:2 * m, :2] *= np.exp(rng.uniform(np.log(1e-4), np.log(0.1), (m, 1)))                         # next to the poles / the axis
    p[2 * m:2 * m + 4] = [(0, 0, 1.5), (0, 0, -0.7), (1.0, 0.0, 0.3), (-1.0, 0.0, 0.3)]              # on them
    dp = [rng.standard_normal((n, 3)) * np.exp(rng.uniform(np.log(0.3), np.log(1.0), (n, 1))) for _ in range(2)]
    return dict(p=p, dpdx=dp[0], dpdy=dp[1])


def test_mappings(oracle):
    """map2d feeding an image map and a checkerboard: spherical (poles, the phi seam on both signs of fix_wrap), cylindrical (its seam),
    planar with v1, v2 not orthogonal, uv with negative scales."""
    T = scenes
    tw = T.transform_mul(T.transform_translate(0.1, -0.05, 0.08), T.transform_mul(T.transform_rotate_x(25.0), T.transform_scale(1.1, 0.9, 1.3)))
    img = waves_image(64, 32, 3, seed=21)
    # The differentials of the two angular mappings are differences of two mapped points over 0.1, so they carry 1e-5 .. 1e-4 relative
    # in float32, and that many more texels of an EWA sum may change their table entry: 5.5 % (cylindrical) to 11 % (spherical under a
    # transform) of the derived bounds pass the cap.  So those two feed the trilinear lookup, which has no table,
    # the checkerboard, uv and bilerp; EWA is held to float64 under the uv and planar mappings.
    maps = {
        "spherical": dict(mapping="spherical"), "spherical_xf": dict(mapping="spherical", to_world=tw),
        "cylindrical": dict(mapping="cylindrical"), "cylindrical_xf": dict(mapping="cylindrical", to_world=tw),
        "planar": dict(mapping="planar", v1=(0.9, 0.3, -0.2), v2=(0.4, 1.1, 0.5), udelta=0.3, vdelta=-0.7),
        "uv_negative": dict(mapping="uv", uscale=-2.5, vscale=-0.75, udelta=0.25, vdelta=1.5),
    }
    rng = np.random.default_rng(13)
    for name, mp in maps.items():
        specs = ([dict(type="imagemap", image=img, maxanisotropy=8.0, wrap=R.REPEAT, **mp)] if name in ("uv_negative", "planar") else []) + [
            dict(type="imagemap", image=img, trilinear=True, wrap=R.CLAMP, **mp),
            dict(type="checkerboard", tex1=(0.9, 0.8, 0.1), tex2=(0.1, 0.2, 0.7), **dict(mp, **({"uscale": -6.0, "vscale": 5.0} if name == "uv_negative" else {}))),
            dict(type="uv", **mp), dict(type="bilerp", v00=(0.1, 0.2, 0.3), v01=0.9, v10=(0.5, 0.0, 0.2), v11=0.4, **mp)]
        bench = Bench(oracle, specs)
        for k, spec in enumerate(specs):
            tally = Tally("%s -> %s%s" % (name, spec["type"], " trilinear" if spec.get("trilinear") else ""))
            for _ in range(2):
                if name in ("planar", "uv_negative"):
                    inp = footprints(rng, 5000, lo=5e-3, hi=0.4, max_aniso=20.0)
                    if name == "planar":
                        q = _surface_points(rng, 5000, "planar")
                        s = np.exp(rng.uniform(np.log(5e-3), np.log(0.4), (5000, 1)))
                        inp = dict(p=q["p"] * 2.0, dpdx=q["dpdx"] * s, dpdy=q["dpdy"] * s * 0.3)
                else:
                    inp = _surface_points(rng, 5000, name.split("_")[0])
                tally.add(5000, hold(bench, k, **inp))
            tally.done()
        bench.close()


# ---------------------------------------------------------------------------------------------------------------- checkerboard
def _checker_inputs(rng, n):
    """Boxes inside one cell, straddling one and two edges, ds or dt just below / above 1, ds = 0 with dt > 0, negative st; half-widths
    of at least 0.01 where the box straddles (the closed form divides a difference of ~ds by 2 ds)."""
    st = rng.uniform(-6.0, 6.0, (n, 2))
    ds = np.exp(rng.uniform(np.log(0.01), np.log(0.9), (n, 2)))
    k = n // 8
    ds[:k] = rng.choice([1 - 3e-3, 1 + 3e-3, 0.999, 1.001], (k, 2))                                    # next to the ds > 1 switch
    ds[k:2 * k, 0] = 0.0                                                                               # ds = 0, dt > 0
    ds[2 * k:3 * k] = np.exp(rng.uniform(np.log(1.0), np.log(10.0), (k, 2)))                           # wide boxes
    ds[3 * k:4 * k] = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), (k, 2)))                          # small boxes: almost always inside one cell
    st[4 * k:5 * k] = np.round(st[4 * k:5 * k]) + rng.uniform(-0.3, 0.3, (k, 2)) * ds[4 * k:5 * k]      # over a corner: two edges
    sg = rng.choice([-1.0, 1.0], (n, 4))
    f = rng.uniform(0.0, 1.0, (n, 2))                                                                  # the other differential is the smaller one
    return dict(uv=st, dudx=sg[:, 0] * ds[:, 0], dvdx=sg[:, 1] * ds[:, 1] * f[:, 0], dudy=sg[:, 2] * ds[:, 0] * f[:, 1], dvdy=sg[:, 3] * ds[:, 1])


def test_checkerboard_closed_form_is_the_area():
    """The float64 closed form against the area of the odd cells inside the box, summed cell by cell, wherever the reference uses it
    (0 < ds, dt <= 1): the truth the oracle is held to below is itself checked a second way."""
    rng = np.random.default_rng(14)
    inp = _checker_inputs(rng, 3000)
    inp = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in inp.items()}
    one, zero = np.ones((3000, 3)), np.zeros((3000, 3))
    val, _ = R.checkerboard2d(dict(type="checkerboard"), R.Hit(3000, **inp), zero, one, np.zeros(3000), np.zeros(3000))
    ds = np.maximum(np.abs(inp["dudx"]), np.abs(inp["dudy"]))
    dt = np.maximum(np.abs(inp["dvdx"]), np.abs(inp["dvdy"]))
    use = (ds > 0) & (dt > 0) & (ds <= 1) & (dt <= 1)
    assert use.sum() > 1500
    area = np.array([R.checker_area(inp["uv"][i, 0], inp["uv"][i, 1], ds[i], dt[i]) for i in np.nonzero(use)[0]])
    assert np.abs(val[use, 0] - area).max() < 1e-12
    assert ((area > 0.01) & (area < 0.99)).sum() > 500


def test_checkerboards(oracle):
    rng = np.random.default_rng(15)
    T = scenes
    tw = T.transform_mul(T.transform_translate(0.3, 0.1, -0.2), T.transform_mul(T.transform_rotate_x(-40.0), T.transform_scale(2.0, 3.5, 0.6)))
    specs = [dict(type="checkerboard", tex1=(0.9, 0.8, 0.1), tex2=(0.1, 0.2, 0.7)),
             dict(type="checkerboard", tex1=0.2, tex2=1.0, aamode="none", uscale=3.0, vscale=-2.0, udelta=0.5),
             dict(type="checkerboard", dimension=3, tex1=(1.0, 0.5, 0.0), tex2=0.25, to_world=tw),
             dict(type="dots", tex1=(0.9, 0.1, 0.1), tex2=(0.1, 0.9, 0.9), uscale=4.0, vscale=4.0)]
    bench = Bench(oracle, specs)
    perm = shared_noise_perm()
    for k, name in enumerate(("checkerboard closed form", "checkerboard aamode none", "checkerboard 3-D", "dots")):
        tally = Tally(name)
        for _ in range(2):
            inp = _checker_inputs(rng, 6000)
            if k == 2:
                inp = dict(p=rng.uniform(-4, 4, (6000, 3)))
            tally.add(6000, hold(bench, k, perm, **inp))
        tally.done()
    bench.close()


# ---------------------------------------------------------------------------------------------------------------- noise
def _noise_inputs(rng, n):
    """Footprints from 1e-6 to 10 (the octave count over its whole range), zero differentials (log2(0)), points with negative and > 256
    coordinates (the & 255 of the lattice) and on lattice planes."""
    p = rng.uniform(-6.0, 6.0, (n, 3))
    k = n // 8
    p[:k] = rng.uniform(-300.0, 300.0, (k, 3))
    p[k:2 * k, rng.integers(0, 3)] = np.round(p[k:2 * k, 0])
    p[2 * k:2 * k + 8] = np.array([(0, 0, 0), (1, 2, 3), (-1, -2, -3), (255, 256, 257), (-256, 0.5, 255.5), (0.5, 0.5, 0.5), (256, 256, 256), (-0.0, 3, -7)], float)
    s = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), (n, 1)))
    dx, dy = rng.standard_normal((n, 3)) * s, rng.standard_normal((n, 3)) * s
    s[:k] = np.maximum(s[:k], 0.2)                                       # far points: at most two octaves (lambda * p leaves float32 no fraction beyond)
    dx, dy = rng.standard_normal((n, 3)) * s, rng.standard_normal((n, 3)) * s
    dx[3 * k:4 * k] = 0.0
    dy[3 * k:3 * k + k // 2] = 0.0
    return dict(p=p, dpdx=dx, dpdy=dy)


def test_noise_textures(oracle):
    """fbm, wrinkled, marble for octaves 1 .. 8 and roughness 0.3 .. 0.7, windy; one under a transform."""
    rng = np.random.default_rng(16)
    perm = shared_noise_perm()
    T = scenes
    tw = T.transform_mul(T.transform_translate(0.3, 0.1, -0.2), T.transform_mul(T.transform_rotate_x(-40.0), T.transform_scale(2.0, 3.5, 0.6)))
    for kind in ("fbm", "wrinkled", "marble", "windy"):
        if kind == "windy":
            specs = [dict(type="windy"), dict(type="windy", to_world=tw)]
        else:
            specs = [dict(type=kind, octaves=o, roughness=float(r)) for o, r in zip(range(1, 9), np.linspace(0.3, 0.7, 8))]
            specs[2 if kind == "marble" else 3]["to_world"] = tw              # marble: the spec of scale 0.5 (the transform stretches y by 3.5, and the far points reach 300)
            if kind == "marble":
                for s, sc, va in zip(specs, (1.0, 2.0, 0.5, 3.0, 1.0, 1.5, 0.7, 1.0), (0.8, 0.5, 1.0, 0.1, 0.0, 0.3, 0.2, 0.2)):      # variation at most 1: it carries the error of fbm (up to ~1e-4 far from the origin) into the slope of a spline that runs to t = 5
                    s["scale"], s["variation"] = sc, va
        bench = Bench(oracle, specs)
        tally = Tally(kind)
        per = 12000 // len(specs) + 1
        for k in range(len(specs)):
            tally.add(per, hold(bench, k, perm, **_noise_inputs(rng, per)), k)
        tally.done()
        bench.close()


# ---------------------------------------------------------------------------------------------------------------- scale and mix
def test_scale_and_mix(oracle):
    """scale and mix over the kinds above, nested two deep, with a constant and a textured amount."""
    rng = np.random.default_rng(17)
    perm = shared_noise_perm()
    img = waves_image(32, 64, 3, seed=22)
    gray = waves_image(16, 16, 1, seed=23)
    image = dict(type="imagemap", image=img, maxanisotropy=8.0, wrap=R.REPEAT, uscale=2.0)
    mono = dict(type="imagemap", image=gray, trilinear=True, wrap=R.CLAMP)
    checker = dict(type="checkerboard", tex1=(0.9, 0.8, 0.1), tex2=(0.1, 0.2, 0.7), uscale=3.0, vscale=3.0)
    f = dict(type="fbm", octaves=4, roughness=0.5)
    specs = [dict(type="scale", tex1=image, tex2=(0.5, 0.7, 0.9)),
             dict(type="scale", tex1=mono, tex2=checker),
             dict(type="mix", tex1=image, tex2=checker, amount=0.3),
             dict(type="mix", tex1=image, tex2=checker, amount=f),
             dict(type="mix", tex1=dict(type="scale", tex1=mono, tex2=image), tex2=dict(type="mix", tex1=checker, tex2=0.5, amount=mono), amount=mono),
             dict(type="scale", tex1=dict(type="mix", tex1=(0.2, 0.4, 0.6), tex2=image, amount=0.75), tex2=dict(type="scale", tex1=mono, tex2=2.0))]
    bench = Bench(oracle, specs)
    for k in range(len(specs)):
        tally = Tally("scale / mix #%d" % k)
        for _ in range(2):
            inp = footprints(rng, 5000, lo=5e-3, hi=0.3, max_aniso=20.0)
            inp.update(p=rng.uniform(-3, 3, (5000, 3)), dpdx=rng.standard_normal((5000, 3)) * 0.01, dpdy=rng.standard_normal((5000, 3)) * 0.01)
            tally.add(5000, hold(bench, k, perm, **inp))
        tally.done()
    bench.close()


# ---------------------------------------------------------------------------------------------------------------- the observable
def truth(hooks, row, perm):
    """The float64 side of one row of fs.TEXTURE_TRUTH, computed from the scene description: camera ray, offset rays, their hits on
    the quad, uv differences, mapping, filtered value -- at the film positions `hooks` (an uploaded device context or an oracle scene)
    reports for the tile's samples.  Asserts that the float64 camera reproduces the hook's rays.  Returns pixels, value, bound, scale;
    the bound is infinite for samples whose main or offset rays miss the quad or pass within their error of its edge."""
    texture, camera, sampler, spp, placement = row[:5]
    t = fs.TRUTH_TILE
    ys, xs = np.mgrid[t[1]:t[3], t[0]:t[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
    si = np.tile(np.arange(spp, dtype=np.uint32), len(pix) // spp)
    o, d, pf = hooks.generate_camera_rays(pix, si)
    lens = fs.TRUTH_LENS if camera == "lens" else (0.0, 1e6)
    plens = None
    if camera == "lens":
        plens = np.stack([hooks.sobol_samples(pix, si, np.full(len(si), k, np.uint32)) for k in (2, 3)], 1).astype(np.float64)
    cam = R.Camera(fs.TRUTH_EYE, fs.TRUTH_LOOK, fs.TRUTH_UP, fs.TRUTH_FOV, fs.TRUTH_RES, fs.TRUTH_RES, lens[0], lens[1], spp)
    rays = cam.rays(pf.astype(np.float64), plens)
    # the camera hooks against float64: a unit direction through ~30 float32 roundings (two matrix applications, two normalisations;
    # the thin lens adds the focus point and a third normalisation), an origin within 8 roundings of the eye's magnitude
    assert np.abs(d - rays[1]).max() <= (64 if camera == "lens" else 32) * R.U, np.abs(d - rays[1]).max()
    assert np.abs(o - rays[0]).max() <= 8 * R.U * (np.abs(np.asarray(fs.TRUTH_EYE)).max() + 1), np.abs(o - rays[0]).max()
    P32, Pw, xf = fs.truth_quad(placement)
    h = R.quad_hit(Pw, fs.TRUTH_UV, *rays)
    gain = 1.0 if xf is None else 2.0                                   # an instance: the hit and its normal come back through one more matrix
    e = R.quad_hit_errors(Pw, fs.TRUTH_UV, h, rays[0], *rays[2:], gain=gain)
    on_quad = h["inside"] & (h["margin"] > 4 * (e["e_uv"] + e["e_duv"]))
    hit = R.Hit(len(si), **{k: h[k] for k in ("p", "uv", "dpdx", "dpdy", "dudx", "dvdx", "dudy", "dvdy")}, **e)
    val, bound, scale = R.evaluate(fs.texture_ref_spec(fs.truth_texture_spec(texture), R.pyramid), hit, perm)
    return pix, np.maximum(val, 0.0), np.where(on_quad, bound, np.inf), scale         # MirrorMaterial: Kr.clamp_zero() (mirror.rs:32)


def observe(hooks, row, integrator, perm):
    """The radiance `hooks` renders for the row against truth(): (excess over bound + 8 * 2^-24 * value, share left out, report)."""
    pix, val, bound, scale = truth(hooks, row, perm)
    got = hooks.radiance_samples(fs.TRUTH_TILE).reshape(-1, 3)
    excess, left, i = R.judge(got, val, bound, scale, extra=8 * R.U * np.abs(val).max(1))
    return excess, left, "%s %s: worst sample %d pixel %s: radiance %s float64 %s bound %.3g" % (integrator, row, i, pix[i], got[i], val[i], bound[i])


def test_truth_rows_are_pairwise():
    """Every pair of values of any two columns of fs.TEXTURE_TRUTH occurs in some row (the integrators of a row: truth_cases)."""
    rows = fs.TEXTURE_TRUTH
    ncol = len(rows[0])
    vals = [sorted({r[c] for r in rows}, key=str) for c in range(ncol)]
    assert vals[0] == sorted(fs.TRUTH_TEXTURES) and [len(v) for v in vals[1:]] == [2, 2, 2, 2, 2]
    for a in range(ncol):
        for b in range(a + 1, ncol):
            have = {(r[a], r[b]) for r in rows}
            assert len(have) == len(vals[a]) * len(vals[b]), (a, b)
    assert set(fs.TRUTH_INTEGRATORS) == {"path", "whitted"} and len(fs.TRUTH_DIRECTLIGHTING_ROWS) == 2
    for t in fs.TRUTH_TEXTURES:                                         # the row `path` shades through k_tex_resolve, for every texture
        assert any(r[0] == t and r[4:] == ("world", "box") for r in rows), t


def truth_cases():
    """Every row under `path`; the rows under the infinite light under `whitted` as well, and two of them under `directlighting`; the
    rows inside the emitting box under `directlighting` instead (the reference's whitted integrator never adds the emission of a
    surface it hits, whitted.rs:59-87, so a reflected ray that ends on an emitter brings nothing back)."""
    cases = []
    for i, row in enumerate(fs.TEXTURE_TRUTH):
        integs = fs.TRUTH_INTEGRATORS if row[5] == "env" else ("path", "directlighting")
        cases += [(i, integ) for integ in integs]
    return cases + [(i, "directlighting") for i in fs.TRUTH_DIRECTLIGHTING_ROWS]


def truth_id(case):
    return "%s-%s" % (case[1], "-".join(str(x) for x in fs.TEXTURE_TRUTH[case[0]]))


@pytest.mark.parametrize("row", fs.TEXTURE_TRUTH, ids=["-".join(str(x) for x in r) for r in fs.TEXTURE_TRUTH])
def test_observable_left_out_share(oracle, row):
    """The float64 side alone: the share of a row's samples left out (off the quad, next to a discontinuity, or with a derived bound
    above 1e-3 of the scale) may not exceed 3 %.  The device rows of test_gpu_texture_truth.py see the same film positions, so this
    is their share too.  A ray differential is a difference of two float32 plane hits and carries 2e-5 .. 7e-5 relative here, so
    the EWA rows depend on the scene's choice of image (fs.truth_image): measured, at most 2.44 % (the closed-form checkerboard in an
    instance), EWA rows at most 1.56 %."""
    osc = oracle.scene(fs.scene_texture_truth(row, "path"))
    try:
        pix, val, bound, scale = truth(osc, row, shared_noise_perm())
    finally:
        osc.close()
    left = 1.0 - float((np.isfinite(bound) & (bound <= R.CAP * scale)).mean())
    print("texture truth [observable %s]: left out %.2f %%" % ("-".join(str(x) for x in row), 100 * left))
    assert left <= MAX_LEFT_OUT, "%.2f %% left out" % (100 * left)


@pytest.mark.parametrize("case", truth_cases(), ids=truth_id)
def test_rendered_texture_value_is_the_float64_one(oracle, case):
    """The oracle's radiance of a mirror whose Kr is the texture, under a constant environment of radiance 1, is the float64 filtered
    value within bound(the float32 hit's error) + 8 * 2^-24 * value, on every sample test_observable_left_out_share does not leave out."""
    row, integ = fs.TEXTURE_TRUTH[case[0]], case[1]
    osc = oracle.scene(fs.scene_texture_truth(row, integ))
    try:
        excess, left, report = observe(osc, row, integ, shared_noise_perm())
    finally:
        osc.close()
    assert excess <= 0.0, "beyond the bound by %.3g: %s" % (excess, report)
    assert left <= MAX_LEFT_OUT, "%.2f %% left out" % (100 * left)
