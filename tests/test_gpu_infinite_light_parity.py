"""LightSource "infinite" on the GPU against the oracle's restatement of lights/infinite.rs, bit for bit: the light hooks element for element
(poles, the phi = 0 / 2 pi seam, cell edges and the CDF's dyadic breakpoints among the inputs), then renders over a pairwise matrix of
integrators, materials, maps, transforms, light-list orders, world bounds, samplers and both traversal kernels -- per-sample radiance of a
tile, film weights under the box filter and every counter, as test_gpu_features._compare holds the other features."""
import os

import numpy as np
import pytest

import feature_scenes as fs
from helpers import bits, pkg, scenes
from test_gpu_features import _compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def far_ctx():
    """A context that traces with k_trace_far (the switch is read when the context is made, as in test_gpu_fuzz.fuzz_ctx_far)."""
    import torch  # noqa: F401  (see conftest.gpu_ctx)
    old = os.environ.get("PBRTGPU_TRACE_FAR")
    os.environ["PBRTGPU_TRACE_FAR"] = "1"
    try:
        ctx = pkg.Context(0)
    finally:
        if old is None:
            del os.environ["PBRTGPU_TRACE_FAR"]
        else:
            os.environ["PBRTGPU_TRACE_FAR"] = old
    yield ctx
    ctx.close()


def hook_inputs(n=100000, seed=3):
    """Directions and sample points where the restatements part ways if they part at all."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 10
    d[:k // 4] = [0.0, 0.0, 1.0]                                     # poles, with and without sign bits and scale
    d[k // 4:k // 2] = [0.0, 0.0, -1.0]
    d[k // 2:k // 2 + 64] = [[0.0, -0.0, 2.5], [-0.0, 0.0, -0.5]] * 32
    s = slice(k, 2 * k)                                              # the seam phi = 0 / 2 pi: y = +-0 and tiny y of either sign
    d[s, 1] = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30, 1e-7, -1e-7], np.float32), k)
    d[s, 0] = np.abs(d[s, 0])
    d[2 * k:2 * k + 6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [-1, -0.0, 0], [-1, 0.0, 0]]
    u = rng.random((n, 2), dtype=np.float32)
    edges = np.concatenate([np.arange(0, 129) / 128.0, np.arange(0, 65) / 64.0 + 1e-7, 1.0 - 2.0 ** -24 - np.zeros(1)]).astype(np.float32)
    u[:k, 0] = rng.choice(edges, k)                                  # cell edges / dyadic breakpoints on either axis and both
    u[k:2 * k, 1] = rng.choice(edges, k)
    u[2 * k:3 * k] = rng.choice(edges, (k, 2))
    u[3 * k] = [0.0, 0.0]                                            # the first Sobol' sample: theta = 0, sin theta = 0 (Q29)
    u[3 * k + 1] = [0.5, 0.5]
    u[3 * k + 2] = [0.5, 0.0]
    u[3 * k + 3] = [0.0, 0.5]
    return d, u


@pytest.mark.parametrize("env_map,transform", [
    ("constant", "identity"), ("image", "rotated"), ("wide", "identity"), ("tall", "scaled"), ("row", "mirrored"), ("column", "rotated"),
    ("holes", "identity"), ("holes", "scaled"),
])
def test_hooks_match_oracle_bit_for_bit(gpu_ctx, oracle, env_map, transform):
    sd = fs.scene_env("path", "power", ("matte",), env_map=env_map, transform=transform, order="before", far=(env_map == "tall"))
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    assert gpu_ctx.info.n_lights == osc.info.n_lights == 3
    d, u = hook_inputs()
    ref = np.random.default_rng(4).normal(size=(len(u), 3)).astype(np.float32)
    ref[:1000] = 0.0
    g, o = gpu_ctx.light_sample_li(0, ref, u), osc.light_sample_li(0, ref, u)
    for name, a, b in zip(("li", "wi", "pdf"), g, o):
        bad = np.flatnonzero(np.any((bits(a) != bits(b)).reshape(len(u), -1), axis=1))
        assert bad.size == 0, (name, bad.size, u[bad[:3]], a[bad[:3]], b[bad[:3]])
    assert (o[2] == 0).any() and (o[2] > 0).mean() > 0.5
    for w in (d, o[1]):                                              # arbitrary directions, and the sampled ones
        gp, op = gpu_ctx.light_pdf_li(0, w), osc.light_pdf_li(0, w)
        bad = np.flatnonzero(bits(gp) != bits(op))
        assert bad.size == 0, ("pdf_li", bad.size, w[bad[:3]], gp[bad[:3]], op[bad[:3]])
        gl, ol = gpu_ctx.light_le(0, w), osc.light_le(0, w)
        bad = np.flatnonzero(np.any(bits(gl) != bits(ol), axis=1))
        assert bad.size == 0, ("le", bad.size, w[bad[:3]], gl[bad[:3]], ol[bad[:3]])
    if transform == "identity":
        assert np.all(osc.light_pdf_li(0, d[:1000]) == 0.0)          # the poles: pdf 0, not a division by 0
    if env_map == "holes":
        assert (osc.light_pdf_li(0, d) == 0.0).mean() > 0.1          # zero-probability cells


# (integrator, strategy, materials, map, transform, order, n_env, sampler, nsamples, far, area_light)
CASES = {
    "path_uniform_env_only_matte": ("path", "uniform", ("matte",), "constant", "identity", "after", 1, "sobol", 1, False, False),
    "path_uniform_env_only_specular": ("path", "uniform", ("mirror", "glass"), "image", "rotated", "after", 1, "halton", 1, False, False),
    "path_power_all_materials": ("path", "power", ("matte", "plastic", "mirror", "glass"), "image", "identity", "after", 1, "sobol", 1, False, True),
    "path_power_wide_mirrored_before": ("path", "power", ("glass", "metal", "textured"), "wide", "mirrored", "before", 1, "sobol", 1, False, True),
    "path_spatial_tall_scaled_halton": ("path", "spatial", ("mirror", "glass", "sphere"), "tall", "scaled", "after", 1, "halton", 1, False, True),
    "path_spatial_holes_instanced_far": ("path", "spatial", ("instanced", "matte"), "holes", "rotated", "before", 1, "sobol", 1, True, True),
    "path_spatial_row_two_envs": ("path", "spatial", ("mirror", "plastic"), "row", "identity", "after", 2, "sobol", 1, False, True),
    "path_power_column_two_envs_before": ("path", "power", ("glass", "matte"), "column", "scaled", "before", 2, "halton", 1, False, True),
    "direct_all1_image_rotated": ("directlighting", "all", ("matte", "mirror", "glass"), "image", "rotated", "after", 1, "sobol", 1, False, True),
    "direct_all3_wide_scaled_halton": ("directlighting", "all", ("plastic", "glass", "textured"), "wide", "scaled", "before", 1, "halton", 3, False, True),
    "direct_all3_holes_two_envs_far": ("directlighting", "all", ("mirror", "sphere", "instanced"), "holes", "mirrored", "after", 2, "sobol", 3, True, True),
    "direct_one_tall": ("directlighting", "one", ("matte", "mirror", "glass", "metal"), "tall", "identity", "before", 1, "sobol", 1, False, True),
    "direct_one_constant_far_halton": ("directlighting", "one", ("glass", "plastic"), "constant", "rotated", "after", 1, "halton", 2, True, True),
    "whitted_image_mirrored": ("whitted", None, ("mirror", "glass", "matte"), "image", "mirrored", "before", 1, "sobol", 1, False, True),
    "whitted_holes_two_envs_halton": ("whitted", None, ("glass", "metal", "instanced"), "holes", "scaled", "after", 2, "halton", 1, False, True),
    "whitted_row_far": ("whitted", None, ("sphere", "mirror"), "row", "rotated", "after", 1, "sobol", 1, True, True),
    "path_spatial_column_mirrored_far": ("path", "spatial", ("matte", "textured"), "column", "mirrored", "before", 1, "sobol", 1, True, True),
}


def case_scene(name):
    integ, strat, mats, m, t, order, n_env, sampler, ns, far, area = CASES[name]
    return fs.scene_env(integ, strat, mats, env_map=m, transform=t, order=order, n_env=n_env, sampler=sampler, nsamples=ns, far=far,
                        area_light=area, spp=8 if sampler == "sobol" else 6)


@pytest.mark.parametrize("name", sorted(CASES))
def test_env_render_matches_oracle(gpu_ctx, oracle, name):
    sd = case_scene(name)
    gpu_ctx.upload(sd)
    osc = oracle.scene(sd)
    assert gpu_ctx.info.n_lights == osc.info.n_lights
    oracle.reference_panics()
    err, frac = _compare(gpu_ctx, osc, exact_film=True)
    assert frac == 0.0
    assert oracle.reference_panics() == 0
    print("%s: rel-L2 %.2e" % (name, err))


@pytest.mark.parametrize("name", ["path_power_all_materials", "direct_all3_holes_two_envs_far", "whitted_image_mirrored", "path_spatial_holes_instanced_far"])
def test_env_render_matches_oracle_trace_far(far_ctx, oracle, name):
    """The same scenes through k_trace_far (PBRTGPU_TRACE_FAR=1 applies to environment scenes unchanged)."""
    sd = case_scene(name)
    far_ctx.upload(sd)
    _, frac = _compare(far_ctx, oracle.scene(sd), exact_film=True)
    assert frac == 0.0


def test_env_golden_fixture(gpu_ctx):
    """The committed environment-lit fixture (tools/make_golden.py, from the oracle): per-sample radiance of the middle tile bit for bit,
    the ray counters, the film weights bit for bit and its colour within tolerance."""
    from helpers import rel_l2
    g = np.load(os.path.join(ROOT, "tests", "golden", "env_directlighting_halton_32x32_4spp.npz"))
    gpu_ctx.upload(fs.scene_env_golden())
    rad = gpu_ctx.radiance_samples(fs.golden_tile(gpu_ctx.info))
    assert np.array_equal(bits(rad), bits(g["radiance"]))
    gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
    c = gpu_ctx.counters()
    assert [c[k] for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices")] == list(g["counters"])
    got = gpu_ctx.film_xyzw()
    assert np.array_equal(bits(got[..., 3]), bits(g["xyzw"][..., 3])) and rel_l2(got[..., :3], g["xyzw"][..., :3]) <= 1e-3
