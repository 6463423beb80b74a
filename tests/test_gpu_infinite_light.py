"""LightSource "infinite" on the GPU path: the light hooks against numpy restatements of infinite.rs / distribution.rs, escaped camera rays,
the enclosing-sphere equivalence, an image-mapped environment against a quadrature, a black environment, the routing switches and the CLI.
Truth comes from closed forms and from the equivalent area-light scene, and the environment scenes are held to the oracle's restatement
(orc_render.hpp EnvLight) bit for bit as well; test_gpu_infinite_light_parity.py does that over a matrix of scenes, and
test_infinite_light_oracle.py checks the restatement itself on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import pkg, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def env_map(h=8, w=16, seed=5):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    base = 1.0 + 0.8 * np.sin(2 * np.pi * x / w)[..., None] * np.array([1.0, 0.6, 0.3]) + 0.5 * (y / h)[..., None]
    return (base + 0.2 * rng.random((h, w, 3))).astype(np.float32)


def rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def bilerp(img, s, t):
    """MIPMap::triangle on level 0 (mipmap.rs:711-765), s repeat, t clamp; float64."""
    h, w, _ = img.shape
    s = np.asarray(s, np.float64) * w - 0.5
    t = np.asarray(t, np.float64) * h - 0.5
    s0, t0 = np.floor(s).astype(np.int64), np.floor(t).astype(np.int64)
    ds, dt = (s - s0)[..., None], (t - t0)[..., None]

    def tx(si, ti):
        return img[np.clip(ti, 0, h - 1), np.mod(si, w)].astype(np.float64)
    return tx(s0, t0) * (1 - ds) * (1 - dt) + tx(s0, t0 + 1) * (1 - ds) * dt + tx(s0 + 1, t0) * ds * (1 - dt) + tx(s0 + 1, t0 + 1) * ds * dt


def dist2d(img):
    """make_distribution (infinite.rs:69-91) for maps twice as wide as high: the lookups fall below level 0, i.e. bilinear on level 0."""
    h, w, _ = img.shape
    nu, nv = 2 * w, 2 * h
    up = (np.arange(nu) + 0.5) / nu
    vp = (np.arange(nv) + 0.5) / nv
    uu, vv = np.meshgrid(up, vp)
    c = bilerp(img, uu, vv)
    y = np.maximum(0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2], 0.0)
    func = y * np.sin(np.pi * vv)
    m_int = func.mean()
    return func, m_int


def spherical(w):
    theta = np.arccos(np.clip(w[:, 2], -1, 1))
    phi = np.arctan2(w[:, 1], w[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    return theta, phi


def camera(sb, res, spp, eye=(0, -4, 1.5), look=(0, 0, 0.5), up=(0, 0, 1), fov=60.0):
    sb.look_at(eye, look, up)
    sb.camera_perspective(fov=fov)
    sb.film(xresolution=res, yresolution=res)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=spp)


def quad(sb, x0, x1, y0, y1, z):
    sb.shape_trianglemesh([x0, y0, z, x1, y0, z, x1, y1, z, x0, y1, z], [0, 1, 2, 0, 2, 3])


def escaped_camera_samples(sd):
    """Per (pixel, sample), pixel-major like pt_radiance_samples: whether the GPU's camera ray leaves the scene."""
    ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        b = list(info.sample_bounds)
        w, h, spp = b[2] - b[0], b[3] - b[1], info.spp
        ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        o, d, _ = ctx.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
        return ctx.trace_closest(o, d, np.full(len(d), np.inf, np.float32))["prim"] < 0
    finally:
        ctx.close()


def render_samples(sd):
    ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        return ctx.radiance_samples(tuple(info.sample_bounds)), info
    finally:
        ctx.close()


# ---------------------------------------------------------------- hooks
@pytest.fixture(scope="module")
def hook_ctx():
    img = env_map()
    sb = scenes.SceneBuilder()
    camera(sb, 8, 1)
    sb.integrator_path()
    quad(sb, -1, 1, -1, 1, 0)
    l2w = rot(2, 20) @ rot(0, 30)
    sb.light_infinite(image=img, L=(1.5, 1.0, 0.5), light_to_world=l2w)
    sd = sb.build()
    ctx = pkg.Context(0)
    ctx.upload(sd)
    yield ctx, (img * np.array([1.5, 1.0, 0.5], np.float32)).astype(np.float32), l2w
    ctx.close()


def test_hooks_le_matches_bilinear_lookup(hook_ctx):
    ctx, img, l2w = hook_ctx
    rng = np.random.default_rng(1)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    le = ctx.light_le(0, d.astype(np.float32))
    wl = d @ np.linalg.inv(l2w)[:3, :3].T
    theta, phi = spherical(wl)
    want = bilerp(img, phi / (2 * np.pi), theta / np.pi)
    np.testing.assert_allclose(le, want, rtol=2e-4, atol=2e-4)


def test_hooks_pdf_li_and_sample_li_match_distribution2d(hook_ctx):
    ctx, img, l2w = hook_ctx
    func, m_int = dist2d(img)
    nv, nu = func.shape
    rng = np.random.default_rng(2)
    n = 200000
    u = rng.random((n, 2)).astype(np.float32)
    li, wi, pdf = ctx.light_sample_li(0, np.zeros((1, 3), np.float32), u)
    ok = pdf > 0
    assert ok.mean() > 0.999
    # uv recovered from wi; map pdf of the cell
    wl = wi.astype(np.float64) @ np.linalg.inv(l2w)[:3, :3].T
    theta, phi = spherical(wl)
    uu, vv = phi / (2 * np.pi), theta / np.pi
    iu, iv = np.clip((uu * nu).astype(np.int64), 0, nu - 1), np.clip((vv * nv).astype(np.int64), 0, nv - 1)
    want_pdf = func[iv, iu] / m_int / (2 * np.pi * np.pi * np.sin(theta))
    away = ok & (np.sin(theta) > 0.05)
    close = np.isclose(pdf[away], want_pdf[away], rtol=2e-3)
    assert close.mean() > 0.995, close.mean()          # the rest sit on a cell edge, where f32 and f64 pick neighbouring cells
    # pdf_li(wi) == the sampled pdf away from the poles
    pl = ctx.light_pdf_li(0, wi[away])
    same = np.isclose(pl, pdf[away], rtol=1e-4)
    assert same.mean() > 0.995, same.mean()
    # Li of the sample is the map at the sampled point
    np.testing.assert_allclose(li[ok], ctx.light_le(0, wi[ok]), rtol=2e-3, atol=2e-3)
    # chi-square of the sampled cells against Distribution2D's cell probabilities func / (m_int nu nv)
    counts = np.bincount((iv * nu + iu)[ok], minlength=nu * nv).astype(np.float64)
    expect = (func / (m_int * nu * nv)).reshape(-1) * ok.sum()
    keep = expect >= 5
    chi2 = ((counts[keep] - expect[keep]) ** 2 / expect[keep]).sum()
    dof = keep.sum() - 1
    z = (chi2 - dof) / np.sqrt(2 * dof)
    print("chi2 %.1f over %d dof (z = %.2f)" % (chi2, dof, z))
    assert z < 5, (chi2, dof)


# ---------------------------------------------------------------- escaped camera rays
def test_escaped_camera_rays_see_le():
    img = env_map(seed=9)
    sb = scenes.SceneBuilder()
    camera(sb, 24, 4)
    sb.integrator_path(maxdepth=3)
    quad(sb, -0.5, 0.5, -0.5, 0.5, 0.2)
    sb.light_infinite(image=img, light_to_world=rot(0, 40) @ rot(2, 75))
    sd = sb.build()
    ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        sb_ = list(info.sample_bounds)
        rad = ctx.radiance_samples(tuple(sb_))
        w, h = sb_[2] - sb_[0], sb_[3] - sb_[1]
        spp = info.spp
        ys, xs = np.mgrid[sb_[1]:sb_[3], sb_[0]:sb_[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        si = np.tile(np.arange(spp, dtype=np.uint32), w * h)
        o, d, _ = ctx.generate_camera_rays(pix, si)
        hits = ctx.trace_closest(o, d, np.full(len(d), np.inf, np.float32))
        miss = hits["prim"] < 0
        assert 0.2 < miss.mean() < 0.99
        le = ctx.light_le(0, d)
        got = rad.reshape(-1, 3)
        assert np.array_equal(got[miss], le[miss])
        # and the whole tile is the oracle's, bit for bit
        import oracle_lib
        r = oracle_lib.load().scene(sd).radiance_samples(tuple(sb_))
        assert np.array_equal(rad.view(np.uint32), r.view(np.uint32))
    finally:
        ctx.close()


# ---------------------------------------------------------------- enclosing sphere
def equivalence_scene(env, family, strategy, L=(1.2, 1.0, 0.8), extra_light=False, res=24, spp=16, integrator="path", env_first=False):
    sb = scenes.SceneBuilder()
    camera(sb, res, spp)
    if integrator == "path":
        sb.integrator_path(maxdepth=4, lightsamplestrategy=strategy)
    elif integrator == "directlighting":
        sb.integrator_directlighting(maxdepth=4, strategy=strategy)
    else:
        sb.integrator_whitted(maxdepth=4)
    if env and env_first:
        sb.light_infinite(L=L)                  # the directive before the area lights: they follow it in the light list
    if extra_light:
        sb.area_light_source_diffuse(L=(3, 3, 3))
        quad(sb, -0.3, 0.3, -0.3, 0.3, 2.0)
        sb.no_area_light()
    sb.material_matte(Kd=(0.6, 0.5, 0.4))
    quad(sb, -2, 2, -2, 2, 0)
    if family == "general":
        sb.material_plastic(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.3), roughness=0.2)
        quad(sb, -0.5, 0.5, -0.5, 0.5, 0.6)
    elif family == "textured":
        tex = sb.texture_checkerboard(tex1=(0.8, 0.2, 0.2), tex2=(0.2, 0.8, 0.2), uscale=4, vscale=4)
        sb.material_matte(Kd=tex)
        quad(sb, -0.5, 0.5, -0.5, 0.5, 0.6)
    elif family == "sphere":
        sb.material_matte(Kd=(0.7, 0.7, 0.7))
        o2w = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5], [0, 0, 0, 1]], np.float32)
        w2o = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -0.5], [0, 0, 0, 1]], np.float32)
        sb.shape_sphere(radius=0.4, object_to_world=o2w.reshape(-1), world_to_object=w2o.reshape(-1))
    elif family == "instanced":
        sb.object_begin("q")
        sb.material_matte(Kd=(0.5, 0.7, 0.3))
        quad(sb, -0.3, 0.3, -0.3, 0.3, 0.0)
        sb.object_end()
        for k in range(3):
            t = np.eye(4)
            t[:3, 3] = [-0.8 + 0.8 * k, 0.0, 0.4 + 0.2 * k]
            ti = np.eye(4)
            ti[:3, 3] = -t[:3, 3]
            sb.object_instance("q", to_world=(t.astype(np.float32), ti.astype(np.float32)))
    if env and not env_first:
        sb.light_infinite(L=L)
    elif not env:
        sb.material_matte(Kd=(0.0, 0.0, 0.0))
        sb.area_light_source_diffuse(L=L, twosided=True)
        sb.shape_sphere(radius=30.0)
        sb.no_area_light()
    return sb.build()


@pytest.mark.parametrize("family,strategy,extra,integrator,env_first", [
    ("matte", "uniform", False, "path", False), ("matte", "power", False, "path", False), ("matte", "spatial", False, "path", False),
    ("general", "spatial", True, "path", False), ("general", "power", True, "path", True), ("textured", "power", False, "path", False),
    ("sphere", "spatial", False, "path", False), ("instanced", "power", True, "path", True),
    ("matte", "all", True, "directlighting", True), ("general", "one", True, "directlighting", False), ("sphere", "all", False, "directlighting", False),
    ("matte", None, True, "whitted", True), ("textured", None, False, "whitted", False),
])
def test_enclosing_sphere_equivalence(family, strategy, extra, integrator, env_first):
    sd_a = equivalence_scene(True, family, strategy, extra_light=extra, integrator=integrator, env_first=env_first)
    a, info_a = render_samples(sd_a)
    sd_b = equivalence_scene(False, family, strategy, extra_light=extra, integrator=integrator)
    b, info_b = render_samples(sd_b)
    b_full = b
    assert np.all(np.isfinite(a))
    if integrator == "whitted":
        # WhittedIntegrator::li never adds isect.le (whitted.rs:48-88): a camera ray that meets the emissive sphere returns 0, one that leaves
        # the environment scene returns le(ray).  Those samples are checked as such and left out of the comparison.
        esc = escaped_camera_samples(equivalence_scene(True, family, strategy, extra_light=extra, integrator=integrator, env_first=env_first))
        assert esc.any()
        np.testing.assert_allclose(a.reshape(-1, 3)[esc], np.broadcast_to(np.array([1.2, 1.0, 0.8], np.float32), (esc.sum(), 3)), rtol=1e-6)
        assert np.all(b.reshape(-1, 3)[esc] == 0.0)
        a, b = a.reshape(-1, 3)[~esc], b.reshape(-1, 3)[~esc]
    ya = a @ np.array([0.212671, 0.715160, 0.072169], np.float32)
    yb = b @ np.array([0.212671, 0.715160, 0.072169], np.float32)
    diff = (ya - yb).reshape(-1).astype(np.float64)
    z = diff.mean() / (diff.std() / np.sqrt(diff.size) + 1e-30)
    print("%s %s %s extra=%s first=%s: mean env %.5f sphere %.5f z = %.2f" % (integrator, family, strategy, extra, env_first, ya.mean(), yb.mean(), z))
    assert abs(z) < 5
    # camera rays that leave the scene: the sphere version sees exactly L; the environment gives the 1 x 1 map's bilinear lookup of L,
    # whose four weights sum to 1 only up to rounding (the reference's MIPMap::triangle does the same arithmetic)
    if integrator != "whitted":
        sky = np.all(b == np.array([1.2, 1.0, 0.8], np.float32), axis=-1)
        assert sky.any()
        np.testing.assert_allclose(a[sky], b[sky], rtol=1e-6)
    # the sphere version is the oracle's render
    import oracle_lib
    osc = oracle_lib.load().scene(sd_b)
    r = osc.radiance_samples(tuple(info_b.sample_bounds))
    err = np.sqrt(((b_full.astype(np.float64) - r) ** 2).sum() / (r.astype(np.float64) ** 2).sum())
    assert err < 1e-4, err
    # and so is the environment version, bit for bit
    a_full = render_samples(sd_a)[0]
    ra = oracle_lib.load().scene(sd_a).radiance_samples(tuple(info_a.sample_bounds))
    assert np.array_equal(a_full.view(np.uint32), ra.view(np.uint32))


def test_emitters_after_the_directive_keep_their_own_radiance():
    """An environment read before the area lights takes place 0 of the light list: two emitters seen directly return their own L."""
    sb = scenes.SceneBuilder()
    camera(sb, 24, 4, eye=(0, -3, 0.5), look=(0, 0, 0.5))
    sb.integrator_path(maxdepth=3)
    sb.light_infinite(L=(0.0, 0.0, 0.0))
    sb.material_none()
    sb.area_light_source_diffuse(L=(5, 4, 3), twosided=True)
    sb.shape_trianglemesh([-1.2, 0, 0, -0.2, 0, 0, -0.2, 0, 1, -1.2, 0, 1], [0, 1, 2, 0, 2, 3])
    sb.area_light_source_diffuse(L=(1, 2, 6), twosided=True)
    sb.shape_trianglemesh([0.2, 0, 0, 1.2, 0, 0, 1.2, 0, 1, 0.2, 0, 1], [0, 1, 2, 0, 2, 3])
    sb.no_area_light()
    sd = sb.build()
    assert sd.infinite_lights[0].light_index == 0
    ctx = pkg.Context(0)
    try:
        info = ctx.upload(sd)
        assert info.n_lights == 5
        b = list(info.sample_bounds)
        rad = ctx.radiance_samples(tuple(b)).reshape(-1, 3)
        w, h, spp = b[2] - b[0], b[3] - b[1], info.spp
        ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        o, d, _ = ctx.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
        prim = ctx.trace_closest(o, d, np.full(len(d), np.inf, np.float32))["prim"]
        left, right = (prim == 0) | (prim == 1), (prim == 2) | (prim == 3)
        assert left.sum() > 50 and right.sum() > 50
        assert np.all(rad[left] == np.array([5, 4, 3], np.float32))
        assert np.all(rad[right] == np.array([1, 2, 6], np.float32))
        assert np.all(rad[prim < 0] == 0.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- image map against a quadrature
@pytest.mark.parametrize("maxdepth,strategy", [(1, "spatial"), (1, "uniform")])
def test_image_map_irradiance_matches_quadrature(maxdepth, strategy):
    img = env_map(seed=11)
    kd = np.array([0.5, 0.4, 0.3])
    sb = scenes.SceneBuilder()
    camera(sb, 16, 64, eye=(0, 0, 1), look=(0, 0, 0), up=(0, 1, 0), fov=20.0)
    sb.integrator_path(maxdepth=maxdepth, lightsamplestrategy=strategy)
    sb.material_matte(Kd=tuple(kd))
    quad(sb, -1000, 1000, -1000, 1000, 0)
    sb.light_infinite(image=img)
    a, _ = render_samples(sb.build())
    a = a.reshape(-1, 3).astype(np.float64)
    nt, nph = 1000, 2000
    th = (np.arange(nt) + 0.5) / nt * (np.pi / 2)
    ph = (np.arange(nph) + 0.5) / nph * 2 * np.pi
    T, PH = np.meshgrid(th, ph, indexing="ij")
    le = bilerp(img, PH / (2 * np.pi), T / np.pi)
    e = (le * (np.cos(T) * np.sin(T))[..., None]).sum(axis=(0, 1)) * (np.pi / 2 / nt) * (2 * np.pi / nph)
    want = kd / np.pi * e
    z = (a.mean(0) - want) / (a.std(0) / np.sqrt(len(a)))
    print("maxdepth %d %s: mean %s want %s z %s" % (maxdepth, strategy, a.mean(0), want, z))
    assert np.all(np.abs(z) < 5), z


# ---------------------------------------------------------------- black environment
def test_black_environment_changes_nothing():
    """L 0 0 0 next to one single-triangle light under the power strategy: the environment's pmf is 0, the triangle's pdf exactly 1 and
    escaped rays add 0, so the render is the oracle's render of the scene without the environment, bit for bit."""
    import oracle_lib

    def scene(env, first):
        sb = scenes.SceneBuilder()
        camera(sb, 24, 16)
        sb.integrator_path(maxdepth=5, lightsamplestrategy="power")
        if env and first:
            sb.light_infinite(L=(0, 0, 0))
        sb.area_light_source_diffuse(L=(4, 4, 4))
        sb.shape_trianglemesh([-0.4, -0.4, 2.0, 0.4, -0.4, 2.0, 0.0, 0.4, 2.0], [0, 2, 1])
        sb.no_area_light()
        sb.material_matte(Kd=(0.6, 0.6, 0.6))
        quad(sb, -2, 2, -2, 2, 0)
        if env and not first:
            sb.light_infinite(L=(0, 0, 0))
        return sb.build()
    sd_b = scene(False, False)
    osc = oracle_lib.load().scene(sd_b)
    for first in (False, True):
        a, ia = render_samples(scene(True, first))
        assert ia.n_lights == 2
        r = osc.radiance_samples(tuple(ia.sample_bounds))
        assert np.array_equal(a, r.astype(np.float32)), (first, np.abs(a - r).max())


# ---------------------------------------------------------------- switches and CLI
SWITCH_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_infinite_light as t
a, _ = t.render_samples(t.equivalence_scene(True, sys.argv[3], "spatial", extra_light=True))
np.save(sys.argv[2], a)
"""


@pytest.mark.parametrize("family", ["textured", "general"])
def test_switches_are_routed_around(tmp_path, family):
    base, _ = render_samples(equivalence_scene(True, family, "spatial", extra_light=True))
    env = dict(os.environ, PBRTGPU_SHADE_LOCAL="1", PBRTGPU_TRACE_FAR="1")
    out = str(tmp_path / "r.npy")
    r = subprocess.run([sys.executable, "-c", SWITCH_SCRIPT, ROOT, out, family], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out), base)


def test_cli_renders_mapname(tmp_path):
    img = env_map(seed=4)
    h, w, _ = img.shape
    with open(tmp_path / "sky.pfm", "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1]).astype("<f4").tobytes())
    (tmp_path / "s.pbrt").write_text("""LookAt 0 -4 1.5  0 0 0.5  0 0 1
Camera "perspective" "float fov" [60]
Film "image" "integer xresolution" [32] "integer yresolution" [32]
Sampler "sobol" "integer pixelsamples" [4]
WorldBegin
AttributeBegin
Rotate -90 1 0 0
LightSource "infinite" "string mapname" "sky.pfm" "integer samples" [2]
AttributeEnd
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 0 2 -2 0 2 2 0 -2 2 0]
WorldEnd
""")
    exe = os.path.join(ROOT, "pbrt-r3_amd", "csrc", "pbrt_gpu")
    out = tmp_path / "o.pfm"
    r = subprocess.run([exe, "-i", str(tmp_path / "s.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    body = raw.split(b"\n", 3)[3]
    px = np.frombuffer(body, "<f4")
    assert px.size == 32 * 32 * 3 and np.all(np.isfinite(px)) and px.mean() > 0.1


def test_wide_map_distribution_uses_the_trilinear_level():
    """A map eight times as wide as high: make_distribution's lookup width 0.5 / min(2w, 2h) lands on level log2(w / h) - 2 = 1 of the
    pyramid (MIPMap::lookup, mipmap.rs:620-637), not below level 0.  pdf_li against a numpy make_distribution over that level."""
    rng = np.random.default_rng(8)
    img = (0.2 + rng.random((8, 64, 3))).astype(np.float32)
    sb = scenes.SceneBuilder()
    camera(sb, 8, 1)
    sb.integrator_path()
    quad(sb, -1, 1, -1, 1, 0)
    sb.light_infinite(image=img)
    ctx = pkg.Context(0)
    try:
        ctx.upload(sb.build())
        lv1 = (img[:, 0::2] * f32(0.5) + img[:, 1::2] * f32(0.5)).astype(np.float32)
        lv1 = (lv1[0::2] * f32(0.5) + lv1[1::2] * f32(0.5)).astype(np.float32)       # level 1: 32 x 4
        nu, nv = 128, 16
        uu, vv = np.meshgrid((np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv)
        c = bilerp(lv1, uu, vv)
        func = np.maximum(0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2], 0.0) * np.sin(np.pi * vv)
        m_int = func.mean()
        d = rng.normal(size=(20000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        theta, phi = spherical(d)
        keep = np.sin(theta) > 0.05
        iu = np.clip((phi / (2 * np.pi) * nu).astype(np.int64), 0, nu - 1)
        iv = np.clip((theta / np.pi * nv).astype(np.int64), 0, nv - 1)
        want = func[iv, iu] / m_int / (2 * np.pi * np.pi * np.sin(theta))
        got = ctx.light_pdf_li(0, d.astype(np.float32))
        close = np.isclose(got[keep], want[keep], rtol=1e-3)
        assert close.mean() > 0.995, close.mean()
        # and the level-0 restatement does NOT describe it
        func0, m0 = dist2d(img)
        want0 = func0[np.clip(iv, 0, 15), np.clip(iu, 0, 127)] / m0 / (2 * np.pi * np.pi * np.sin(theta))
        assert np.isclose(got[keep], want0[keep], rtol=1e-3).mean() < 0.9
    finally:
        ctx.close()


@pytest.mark.parametrize("maxdepth", [1, 3])
def test_image_map_directlighting_matches_quadrature(maxdepth):
    img = env_map(seed=11)
    kd = np.array([0.5, 0.4, 0.3])
    sb = scenes.SceneBuilder()
    camera(sb, 16, 64, eye=(0, 0, 1), look=(0, 0, 0), up=(0, 1, 0), fov=20.0)
    sb.integrator_directlighting(maxdepth=maxdepth, strategy="all")
    sb.material_matte(Kd=tuple(kd))
    quad(sb, -1000, 1000, -1000, 1000, 0)
    sb.light_infinite(image=img, nsamples=2)
    a, _ = render_samples(sb.build())
    a = a.reshape(-1, 3).astype(np.float64)
    nt, nph = 1000, 2000
    th = (np.arange(nt) + 0.5) / nt * (np.pi / 2)
    ph = (np.arange(nph) + 0.5) / nph * 2 * np.pi
    T, PH = np.meshgrid(th, ph, indexing="ij")
    le = bilerp(img, PH / (2 * np.pi), T / np.pi)
    e = (le * (np.cos(T) * np.sin(T))[..., None]).sum(axis=(0, 1)) * (np.pi / 2 / nt) * (2 * np.pi / nph)
    want = kd / np.pi * e
    z = (a.mean(0) - want) / (a.std(0) / np.sqrt(len(a)))
    print("directlighting maxdepth %d: mean %s want %s z %s" % (maxdepth, a.mean(0), want, z))
    assert np.all(np.abs(z) < 5), z
