"""The oracle's restatement of LightSource "infinite" (lights/infinite.rs, orc_render.hpp EnvLight) on the CPU: its hooks against the float64
numpy restatements of test_gpu_infinite_light.py, renders against closed forms and the enclosing-sphere scene, the light-list order, the
committed environment-lit fixture -- and that no environment scene reaches the oracle without its environment."""
import os

import numpy as np
import pytest

import feature_scenes as fs
from helpers import bits, scenes
from test_gpu_infinite_light import bilerp, camera, dist2d, env_map, equivalence_scene, quad, rot, spherical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
f32 = np.float32


def hook_scene(oracle, img, L=(1.5, 1.0, 0.5), l2w=None):
    sb = scenes.SceneBuilder()
    camera(sb, 8, 1)
    sb.integrator_path()
    quad(sb, -1, 1, -1, 1, 0)
    sb.light_infinite(image=img, L=L, light_to_world=l2w)
    return oracle.scene(sb.build())


@pytest.fixture(scope="module")
def hooks(oracle):
    img = env_map()
    l2w = rot(2, 20) @ rot(0, 30)
    return hook_scene(oracle, img, l2w=l2w), (img * np.array([1.5, 1.0, 0.5], np.float32)).astype(np.float32), l2w


def test_le_matches_bilinear_lookup(hooks):
    osc, img, l2w = hooks
    rng = np.random.default_rng(1)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    le = osc.light_le(0, d.astype(np.float32))
    theta, phi = spherical(d @ np.linalg.inv(l2w)[:3, :3].T)
    np.testing.assert_allclose(le, bilerp(img, phi / (2 * np.pi), theta / np.pi), rtol=2e-4, atol=2e-4)
    # le normalises its direction: a scaled direction gives the same radiance
    assert np.array_equal(bits(osc.light_le(0, (d * 7.5).astype(np.float32))), bits(osc.light_le(0, (d * 7.5).astype(np.float32))))
    np.testing.assert_allclose(osc.light_le(0, (d * 7.5).astype(np.float32)), le, rtol=1e-6, atol=1e-6)


def test_sample_li_and_pdf_li_match_distribution2d(hooks):
    osc, img, l2w = hooks
    func, m_int = dist2d(img)
    nv, nu = func.shape
    rng = np.random.default_rng(2)
    u = rng.random((200000, 2)).astype(np.float32)
    li, wi, pdf = osc.light_sample_li(0, np.zeros((1, 3), np.float32), u)
    ok = pdf > 0
    assert ok.mean() > 0.999
    theta, phi = spherical(wi.astype(np.float64) @ np.linalg.inv(l2w)[:3, :3].T)
    iu = np.clip((phi / (2 * np.pi) * nu).astype(np.int64), 0, nu - 1)
    iv = np.clip((theta / np.pi * nv).astype(np.int64), 0, nv - 1)
    want_pdf = func[iv, iu] / m_int / (2 * np.pi * np.pi * np.sin(theta))
    away = ok & (np.sin(theta) > 0.05)
    assert np.isclose(pdf[away], want_pdf[away], rtol=2e-3).mean() > 0.995
    assert np.isclose(osc.light_pdf_li(0, wi[away]), pdf[away], rtol=1e-4).mean() > 0.995
    np.testing.assert_allclose(li[ok], osc.light_le(0, wi[ok]), rtol=2e-3, atol=2e-3)
    # chi-square of the sampled cells against Distribution2D's cell probabilities func / (m_int nu nv)
    counts = np.bincount((iv * nu + iu)[ok], minlength=nu * nv).astype(np.float64)
    expect = (func / (m_int * nu * nv)).reshape(-1) * ok.sum()
    keep = expect >= 5
    chi2 = ((counts[keep] - expect[keep]) ** 2 / expect[keep]).sum()
    dof = keep.sum() - 1
    assert (chi2 - dof) / np.sqrt(2 * dof) < 5, (chi2, dof)


def test_sample_li_swapped_axes_would_show(hooks):
    """sample_li takes u.y for the marginal (theta) and u.x for the conditional (phi), distribution.rs:133-137: swapping them samples the
    same density, but not the same direction for a given u -- the sampled theta follows u.y alone."""
    osc, _, l2w = hooks
    u = np.stack([np.full(64, 0.3, np.float32), np.linspace(0.01, 0.99, 64, dtype=np.float32)], 1)
    _, wi, _ = osc.light_sample_li(0, np.zeros((1, 3), np.float32), u)
    theta, _ = spherical(wi.astype(np.float64) @ np.linalg.inv(l2w)[:3, :3].T)
    assert np.all(np.diff(theta) > 0)
    u2 = u[:, ::-1].copy()
    _, wi2, _ = osc.light_sample_li(0, np.zeros((1, 3), np.float32), u2)
    theta2, _ = spherical(wi2.astype(np.float64) @ np.linalg.inv(l2w)[:3, :3].T)
    assert np.ptp(theta2) < 0.2 * np.ptp(theta)


def test_poles_and_the_first_sobol_sample(oracle):
    """Q29: pdf_li is exactly 0 at the poles, and sample_li at u = (0, 0) -- Sobol's first sample -- lands on theta = 0 and returns a
    sample with pdf 0 (Some, not None: li and wi are set)."""
    osc = hook_scene(oracle, env_map())
    poles = np.array([[0, 0, 1], [0, 0, -1], [0, -0.0, 3], [-0.0, 0, -1.0]], np.float32)
    assert np.all(osc.light_pdf_li(0, poles) == 0.0)
    assert osc.light_pdf_li(0, np.array([[0, 0, -0.25]], np.float32))[0] > 0      # not normalised (infinite.rs:161-180): z -0.25 is no pole
    li, wi, pdf = osc.light_sample_li(0, np.zeros((1, 3), np.float32), np.array([[0.0, 0.0], [0.5, 0.0]], np.float32))
    assert np.all(pdf == 0.0)
    assert np.all(li > 0) and np.all(wi[:, 2] == 1.0) and np.all(wi[:, :2] == 0.0)


def test_wide_map_distribution_uses_the_trilinear_level(oracle):
    """An 8:1 map: make_distribution's lookup width 0.5 / min(2w, 2h) lands on level 1 of the pyramid (mipmap.rs:620-637)."""
    rng = np.random.default_rng(8)
    img = (0.2 + rng.random((8, 64, 3))).astype(np.float32)
    osc = hook_scene(oracle, img, L=(1, 1, 1))
    lv1 = (img[:, 0::2] * f32(0.5) + img[:, 1::2] * f32(0.5)).astype(np.float32)
    lv1 = (lv1[0::2] * f32(0.5) + lv1[1::2] * f32(0.5)).astype(np.float32)
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
    got = osc.light_pdf_li(0, d.astype(np.float32))
    assert np.isclose(got[keep], want[keep], rtol=1e-3).mean() > 0.995
    func0, m0 = dist2d(img)
    want0 = func0[iv, iu] / m0 / (2 * np.pi * np.pi * np.sin(theta))
    assert np.isclose(got[keep], want0[keep], rtol=1e-3).mean() < 0.9


def test_black_rows_and_columns_have_zero_pdf(oracle):
    """Cells of a map's black rows and columns have probability 0: sample_li never lands there, pdf_li is 0 there."""
    img = fs.env_map_image("holes")
    osc = hook_scene(oracle, img, L=(1, 1, 1))
    u = np.random.default_rng(3).random((50000, 2)).astype(np.float32)
    _, wi, pdf = osc.light_sample_li(0, np.zeros((1, 3), np.float32), u)
    theta, phi = spherical(wi[pdf > 0].astype(np.float64))
    h, w, _ = img.shape
    col = (phi / (2 * np.pi) * 2 * w).astype(np.int64)       # cells of the (2w) x (2h) table
    assert not np.any((col >= 10) & (col <= 15))             # texels 4..8 black: table cells 9..16 have every bilinear tap black
    d = np.random.default_rng(4).normal(size=(20000, 3)).astype(np.float32)
    th, ph = spherical(d.astype(np.float64))
    c = (ph / (2 * np.pi) * 2 * w).astype(np.int64)
    inside = (c >= 10) & (c <= 15) & (np.sin(th) > 0.05)
    assert inside.sum() > 100 and np.all(osc.light_pdf_li(0, d[inside]) == 0.0)


# ---------------------------------------------------------------- renders
def escaped_camera_samples(osc):
    """Per (pixel, sample), pixel-major like radiance_samples: whether the camera ray leaves the scene, and the rays."""
    b = list(osc.info.sample_bounds)
    w, h, spp = b[2] - b[0], b[3] - b[1], osc.info.spp
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
    o, d, _ = osc.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
    return osc.trace_closest(o, d, np.full(len(d), np.inf, np.float32))[0]["prim"] < 0


def _z(a, b):
    y = np.array([0.212671, 0.715160, 0.072169], np.float32)
    diff = ((a @ y) - (b @ y)).reshape(-1).astype(np.float64)
    return diff.mean() / (diff.std() / np.sqrt(diff.size) + 1e-30)


@pytest.mark.parametrize("family,strategy,extra,integrator,env_first", [
    ("matte", "uniform", False, "path", False), ("general", "power", True, "path", True), ("sphere", "spatial", False, "path", False),
    ("matte", "all", True, "directlighting", True), ("general", "one", True, "directlighting", False),
    ("textured", None, False, "whitted", False),
])
def test_enclosing_sphere_equivalence_on_the_oracle(oracle, family, strategy, extra, integrator, env_first):
    """The environment (L constant) against an emissive sphere of radius 30 around the scene: the same expected radiance."""
    sd_a = equivalence_scene(True, family, strategy, extra_light=extra, integrator=integrator, env_first=env_first)
    sd_b = equivalence_scene(False, family, strategy, extra_light=extra, integrator=integrator)
    oa, ob = oracle.scene(sd_a), oracle.scene(sd_b)
    tile = tuple(oa.info.sample_bounds)
    a, b = oa.radiance_samples(tile), ob.radiance_samples(tile)
    assert np.all(np.isfinite(a))
    if integrator == "whitted":          # its camera rays never see the sphere's emission (whitted.rs:48-88), the environment's they do
        esc = escaped_camera_samples(oa)
        assert esc.any() and np.all(b.reshape(-1, 3)[esc] == 0.0)
        np.testing.assert_allclose(a.reshape(-1, 3)[esc], np.broadcast_to(np.array([1.2, 1.0, 0.8], np.float32), (esc.sum(), 3)), rtol=1e-6)
        a, b = a.reshape(-1, 3)[~esc], b.reshape(-1, 3)[~esc]
    z = _z(a, b)
    print("%s %s %s: z = %.2f" % (integrator, family, strategy, z))
    assert abs(z) < 5


@pytest.mark.parametrize("integrator,maxdepth,strategy", [("path", 1, "spatial"), ("path", 1, "uniform"), ("directlighting", 1, "all"),
                                                          ("directlighting", 3, "all")])
def test_image_map_irradiance_matches_quadrature(oracle, integrator, maxdepth, strategy):
    img = env_map(seed=11)
    kd = np.array([0.5, 0.4, 0.3])
    sb = scenes.SceneBuilder()
    camera(sb, 16, 64, eye=(0, 0, 1), look=(0, 0, 0), up=(0, 1, 0), fov=20.0)
    if integrator == "path":
        sb.integrator_path(maxdepth=maxdepth, lightsamplestrategy=strategy)
    else:
        sb.integrator_directlighting(maxdepth=maxdepth, strategy=strategy)
    sb.material_matte(Kd=tuple(kd))
    quad(sb, -1000, 1000, -1000, 1000, 0)
    sb.light_infinite(image=img, nsamples=2)
    osc = oracle.scene(sb.build())
    xyzw, _, _ = osc.render(threads=8)
    a = osc.radiance_samples(tuple(osc.info.sample_bounds)).reshape(-1, 3).astype(np.float64)
    nt, nph = 1000, 2000
    th = (np.arange(nt) + 0.5) / nt * (np.pi / 2)
    ph = (np.arange(nph) + 0.5) / nph * 2 * np.pi
    T, PH = np.meshgrid(th, ph, indexing="ij")
    le = bilerp(img, PH / (2 * np.pi), T / np.pi)
    want = kd / np.pi * (le * (np.cos(T) * np.sin(T))[..., None]).sum(axis=(0, 1)) * (np.pi / 2 / nt) * (2 * np.pi / nph)
    z = (a.mean(0) - want) / (a.std(0) / np.sqrt(len(a)))
    assert np.all(np.abs(z) < 5), z


@pytest.mark.parametrize("strategy", ["power", "uniform", "spatial"])
def test_black_environment_changes_nothing(oracle, strategy):
    """L 0 0 0 next to one triangle light: escaped rays add 0 and the environment's selection weight is 0 under the power strategy (the
    render is the scene without it, bit for bit).  Under spatial selection (uniform with two lights is spatial, quirk Q12) the black
    environment keeps the minimum weight 0.001 * average (spatial.rs:183-193): the same expected image, not the same bits."""
    def scene(env, first):
        sb = scenes.SceneBuilder()
        camera(sb, 24, 16)
        sb.integrator_path(maxdepth=5, lightsamplestrategy=strategy)
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
    ob = oracle.scene(scene(False, False))
    r = ob.radiance_samples(tuple(ob.info.sample_bounds))
    for first in (False, True):
        oa = oracle.scene(scene(True, first))
        assert oa.info.n_lights == 2
        a = oa.radiance_samples(tuple(oa.info.sample_bounds))
        if strategy == "power":
            assert np.array_equal(bits(a), bits(r)), first
        else:
            ya, yr = (a.reshape(-1, 3) @ np.array([0.212671, 0.715160, 0.072169])), (r.reshape(-1, 3) @ np.array([0.212671, 0.715160, 0.072169]))
            z = (ya.mean() - yr.mean()) / np.sqrt(ya.var() / ya.size + yr.var() / yr.size)        # unpaired: the paired difference is systematic
            assert not np.array_equal(bits(a), bits(r)) and abs(z) < 5, z


def test_emitters_after_the_directive_keep_their_own_radiance(oracle):
    """An environment read before two area lights takes place 0 of the light list: each emitter seen directly returns its own L."""
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
    osc = oracle.scene(sd)
    assert osc.info.n_lights == 5
    b = list(osc.info.sample_bounds)
    rad = osc.radiance_samples(tuple(b)).reshape(-1, 3)
    w, h, spp = b[2] - b[0], b[3] - b[1], osc.info.spp
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
    o, d, _ = osc.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
    prim = osc.trace_closest(o, d, np.full(len(d), np.inf, np.float32))[0]["prim"]
    left, right = (prim == 0) | (prim == 1), (prim == 2) | (prim == 3)
    assert left.sum() > 50 and right.sum() > 50
    assert np.all(rad[left] == np.array([5, 4, 3], np.float32))
    assert np.all(rad[right] == np.array([1, 2, 6], np.float32))
    assert np.all(rad[prim < 0] == 0.0)
    # the light list as the light distribution sees it: place 0 is the (black) environment
    func, _ = osc.light_distribution([0.0, 0.0, 0.5])
    assert len(func) == 5


@pytest.mark.parametrize("integrator", ["path", "directlighting", "whitted"])
def test_environment_is_never_dropped(oracle, integrator):
    """An environment scene handed to the oracle renders WITH its environment: the light count includes it, the render differs from the
    same scene without it, and camera rays that leave the scene return the map's le."""
    img = env_map(seed=9)
    def scene(env):
        sb = scenes.SceneBuilder()
        camera(sb, 24, 4)
        if integrator == "path":
            sb.integrator_path(maxdepth=3)
        elif integrator == "directlighting":
            sb.integrator_directlighting(maxdepth=3)
        else:
            sb.integrator_whitted(maxdepth=3)
        sb.area_light_source_diffuse(L=(3, 3, 3))
        quad(sb, -0.3, 0.3, -0.3, 0.3, 2.0)
        sb.no_area_light()
        quad(sb, -0.5, 0.5, -0.5, 0.5, 0.2)
        if env:
            sb.light_infinite(image=img, light_to_world=rot(0, 40) @ rot(2, 75))
        return sb.build()
    oa, ob = oracle.scene(scene(True)), oracle.scene(scene(False))
    assert oa.info.n_lights == ob.info.n_lights + 1
    b = list(oa.info.sample_bounds)
    ra, rb = oa.radiance_samples(tuple(b)), ob.radiance_samples(tuple(b))
    assert not np.array_equal(ra, rb) and ra.mean() > rb.mean()
    w, h, spp = b[2] - b[0], b[3] - b[1], oa.info.spp
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
    o, d, _ = oa.generate_camera_rays(pix, np.tile(np.arange(spp, dtype=np.uint32), w * h))
    miss = oa.trace_closest(o, d, np.full(len(d), np.inf, np.float32))[0]["prim"] < 0
    assert 0.2 < miss.mean() < 0.99
    assert np.array_equal(bits(ra.reshape(-1, 3)[miss]), bits(oa.light_le(2, d[miss])))


def test_specular_escape_adds_le(oracle):
    """path.rs:86-98: Le is added when the ray escapes at bounce 0 or after a specular bounce -- a camera ray that meets a mirror and
    leaves the scene returns Kr times the map's le in the reflected direction, exactly."""
    sb = scenes.SceneBuilder()
    camera(sb, 16, 4, eye=(0, -3, 1.0), look=(0, 0, 0), up=(0, 0, 1), fov=30.0)
    sb.integrator_path(maxdepth=3, lightsamplestrategy="uniform")
    sb.material_mirror(Kr=(0.5, 0.5, 0.5))
    quad(sb, -100, 100, -100, 100, 0)
    sb.light_infinite(L=(2.0, 1.0, 0.5))
    osc = oracle.scene(sb.build())
    a = osc.radiance_samples(tuple(osc.info.sample_bounds)).reshape(-1, 3)
    le = osc.light_le(0, np.array([[0, 0, 1]], np.float32))[0]
    np.testing.assert_allclose(a, np.broadcast_to(le * f32(0.5), a.shape), rtol=1e-6)


def test_env_golden_fixture(oracle):
    """The oracle's environment-lit restatement frozen against accidental edits (tools/make_golden.py): film, per-sample radiance of the
    middle tile and the ray counters, bit for bit."""
    g = np.load(os.path.join(GOLD, "env_directlighting_halton_32x32_4spp.npz"))
    sc = oracle.scene(fs.scene_env_golden())
    xyzw, cnt, _ = sc.render(threads=4)
    assert np.array_equal(bits(xyzw), bits(g["xyzw"]))
    rad = sc.radiance_samples(fs.golden_tile(sc.info))
    assert np.array_equal(bits(rad), bits(g["radiance"]))
    assert [cnt[k] for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices")] == list(g["counters"])
    assert np.isfinite(rad).all() and rad.max() > 0 and len(np.unique(rad)) > 10
    sc.close()
