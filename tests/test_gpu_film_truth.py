"""The device's film -- film_weight, film_add, k_film, k_film_xyzw, k_film_add, k_film_rgb, validate_radiance and the host's crop and
sample bounds -- held straight to the float64 restatement (tests/film_ref.py), no oracle in between.

Every case hands the whole sample bounds to ctx.radiance_samples as one tile and the same pixels and sample indices to
ctx.generate_camera_rays for p_film; the filter table, the radii, the crop, the scale and the clamp come from the scene description.
film_xyzw() and film_rgb() must lie within the truth's per-pixel bounds outside the left-out pixels, of which there may be 1 % at most.
That the film agrees with a truth fed with generate_camera_rays' p_film is also what says that this is the p_film k_gen hands to k_film.

Measured on an MI355X: no case leaves a pixel out; the largest err / bound per case is printed (-s) and recorded in DESIGN.md section 7."""
import functools
import os

import numpy as np
import pytest

import film_cases as fc
import film_ref as fr
from helpers import bits, pkg, scenes
from test_film_truth_oracle import RADII, WINDOWS, _bounds_scene

pytestmark = pytest.mark.gpu
CAP = 0.01
POOL_FLOOR = 65536          # the least PBRTGPU_POOL_PATHS is taken as (render_tiles): a pass holds that many paths at least


def _hold(name, truth, xyzw, rgb):
    c = fr.compare(truth, xyzw, rgb)
    print("\n[%s] err / bound: xyz %.3f weight %.3f rgb %.3f; left out %.2f %%; undecided steps %d"
          % (name, c["xyz"], c["weight"], c["rgb"], 100 * c["left_out"], truth["n_steps"]))
    assert c["left_out"] <= CAP, c
    assert c["ok"], c
    return c


@functools.lru_cache(maxsize=None)
def _scene(name):
    return fc.make_scene(name)


def _upload_and_truth(ctx, sd, repeat=1):
    ctx.upload(sd)
    p_film, rad, pix = fc.samples_of(ctx, ctx.info)
    truth = fc.truth_of(sd, p_film, rad, repeat)
    assert tuple(ctx.info.sample_bounds) == truth["sample_bounds"] and tuple(ctx.info.cropped_bounds) == truth["cropped"]
    assert ctx.film_shape == truth["weight"].shape
    return truth, p_film, rad, pix


@pytest.mark.parametrize("name", list(fc.CASES))
def test_device_film_holds_to_the_truth(gpu_ctx, name):
    sd = _scene(name)
    truth, p_film, rad, pix = _upload_and_truth(gpu_ctx, sd)
    gpu_ctx.film_clear(); gpu_ctx.render()
    xyzw, rgb = gpu_ctx.film_xyzw(), gpu_ctx.film_rgb()
    _hold(name, truth, xyzw, rgb)
    clamped, outside = truth["n_clamped"] / truth["n_samples"], fc.outside_share(truth, pix)
    print("[%s] clamped %.1f %%; contributors outside the crop %.1f %%; contributing %d of %d" % (name, 100 * clamped, 100 * outside,
                                                                                               truth["n_contributing"], truth["n_samples"]))
    assert rad.max() > 0
    if np.isfinite(fc.CASES[name][4]):
        assert 0.01 <= clamped <= 0.5, clamped
    if name in fc.WIDE_CROPPED:
        assert outside >= 0.1, outside
    if name == "box_0.5":         # every sample lands on its own pixel with weight 1: counts, exactly
        assert np.array_equal(xyzw[..., 3], truth["weight"].astype(np.float32))
    if name == "box_0.3":
        assert truth["n_contributing"] < 0.5 * truth["n_samples"]


@pytest.mark.parametrize("res,window,decisive", WINDOWS)
def test_device_bounds_hold_to_the_restatement(gpu_ctx, res, window, decisive):
    """pt_scene_info's cropped bounds, sample bounds and film shape against Film::new and get_sample_bounds restated in np.float32."""
    for radius in RADII:
        cropped, sb, _ = fr.film_bounds(res[0], res[1], window, radius)
        info = gpu_ctx.upload(_bounds_scene(res, window, radius))
        assert tuple(info.cropped_bounds) == cropped and tuple(info.sample_bounds) == sb, (radius, tuple(info.cropped_bounds), tuple(info.sample_bounds))
        assert gpu_ctx.film_shape == (cropped[3] - cropped[1], cropped[2] - cropped[0])


def _tiles(sb, tw=7, th=5):
    return [(x, y, min(x + tw, sb[2]), min(y + th, sb[3])) for y in range(sb[1], sb[3], th) for x in range(sb[0], sb[2], tw)]


def test_tiles_calls_and_sums(gpu_ctx):
    """Caller-given tiles of 7 x 5 plus remainders in two render calls with disjoint lists; two renders without a clear (the sums double);
    a clear and one render; film_add_xyzw of the film to itself (the sums double, the resolved image does not move)."""
    sd = _scene("sinc")            # sample bounds of 32 x 32: 7 x 5 leaves remainders on both axes
    truth, p_film, rad, pix = _upload_and_truth(gpu_ctx, sd)
    fi = fc.film_inputs(sd)
    sums = fr.add_samples(p_film, rad, fi["table"], fi["radius"], truth["cropped"], fi["clamp"])
    twice = fr.resolve(fr.add_samples(p_film, rad, fi["table"], fi["radius"], truth["cropped"], fi["clamp"], repeat=2), fi["scale"])
    tiles = _tiles(tuple(gpu_ctx.info.sample_bounds))
    assert len(tiles) > 20 and any(t[2] - t[0] < 7 for t in tiles) and any(t[3] - t[1] < 5 for t in tiles)
    gpu_ctx.film_clear()
    gpu_ctx.render(tiles[0::2]); gpu_ctx.render(tiles[1::2])
    _hold("tiles, two calls", truth, gpu_ctx.film_xyzw(), gpu_ctx.film_rgb())
    gpu_ctx.film_clear()
    gpu_ctx.render(); gpu_ctx.render()
    _hold("two renders", twice, gpu_ctx.film_xyzw(), gpu_ctx.film_rgb())
    gpu_ctx.film_clear(); gpu_ctx.render()
    once, rgb_once = gpu_ctx.film_xyzw(), gpu_ctx.film_rgb()
    _hold("clear, one render", truth, once, rgb_once)
    gpu_ctx.film_add_xyzw(once)
    doubled = fr.resolve(fr.scaled(sums, 2.0), fi["scale"])          # a doubling is exact in float32: values and bounds scale
    _hold("film_add_xyzw(own film)", doubled, gpu_ctx.film_xyzw(), gpu_ctx.film_rgb())
    assert np.array_equal(bits(gpu_ctx.film_xyzw()), bits(2.0 * once))
    assert np.array_equal(bits(gpu_ctx.film_rgb()), bits(rgb_once))


def test_passes_and_pixel_chunks(gpu_ctx):
    """A film of more than 65 536 sample pixels at 3 spp under PBRTGPU_POOL_PATHS=65536: two pixel chunks (c0) and three sample passes (s0,
    spp_total).  Held to the same truth; under the box filter of radius 0.5 bit-identical to the single-pass render."""
    films = {}
    for kind, widths, params in (("gaussian", (1.5, 1.5), {"alpha": 2.0}), ("box", (0.5, 0.5), {})):
        sd = fc.make_scene(spec=(kind, widths, params, fc.FULL, 3.0, 1.0, "halton", "path"), res=(300, 224), spp=3)
        if kind == "gaussian":
            truth, p_film, rad, pix = _upload_and_truth(gpu_ctx, sd)
        else:
            gpu_ctx.upload(sd)
        sb = tuple(gpu_ctx.info.sample_bounds)
        n_pix = (sb[2] - sb[0]) * (sb[3] - sb[1])
        # read from the scene's size against the pool floor: more pixels than a pass may hold -> chunks of pixels, one sample per pass
        assert n_pix > POOL_FLOOR and gpu_ctx.info.spp == 3
        gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
        single, c_single = gpu_ctx.film_xyzw(), gpu_ctx.counters()
        try:
            os.environ["PBRTGPU_POOL_PATHS"] = str(POOL_FLOOR)
            gpu_ctx.film_clear(); gpu_ctx.reset_counters(); gpu_ctx.render()
        finally:
            os.environ.pop("PBRTGPU_POOL_PATHS", None)
        chunked, rgb, c_chunked = gpu_ctx.film_xyzw(), gpu_ctx.film_rgb(), gpu_ctx.counters()
        assert c_chunked["camera_rays"] == c_single["camera_rays"] == 3 * n_pix
        assert c_chunked["trace_launches"] > c_single["trace_launches"]
        films[kind] = (single, chunked)
        if kind == "gaussian":
            _hold("chunks and passes", truth, chunked, rgb)
            clamped = truth["n_clamped"] / truth["n_samples"]
            assert 0.01 <= clamped <= 0.5, clamped
    single, chunked = films["box"]
    assert np.array_equal(bits(single), bits(chunked))


def _emitter_scene(L):
    b = scenes.SceneBuilder()
    b.look_at((0, 0, -3), (0, 0, 0), (0, 1, 0))
    b.camera_perspective(fov=40.0)
    b.film(xresolution=16, yresolution=12)
    b.pixel_filter_box()
    b.sampler_sobol(2)
    b.integrator_path(maxdepth=0)
    b.area_light_source_diffuse(L=L, twosided=True)
    scenes._quad(b, (-4, -4, 1), (4, -4, 1), (4, 4, 1), (-4, 4, 1))
    return b.build()


def test_validate_radiance_on_the_device(gpu_ctx):
    """A camera that looks straight at an emitter, maxdepth 0.  With a luminance below -1e-5 every sample is set to black
    (sampler.rs:159-167) and the film is exactly 0; with L = 0.5 every sample is 0.5 and the film holds to the truth."""
    for L, want in (((-1.0, -2.0, -0.5), 0.0), ((0.5, 0.5, 0.5), 0.5), ((1.0, -0.1, 1.0), None)):
        sd = _emitter_scene(L)
        truth, p_film, rad, pix = _upload_and_truth(gpu_ctx, sd)
        if want is None:      # luminance 0.2127 - 0.0715 + 0.0722 > 0: a negative channel alone is not guarded
            want_rad = np.tile(np.array(L, np.float32), (len(rad), 1))
        else:
            want_rad = np.full(rad.shape, want, np.float32)
        assert np.array_equal(bits(rad), bits(want_rad)), L
        assert np.array_equal(bits(fr.validate_radiance(rad)), bits(rad))
        gpu_ctx.film_clear(); gpu_ctx.render()
        xyzw, rgb = gpu_ctx.film_xyzw(), gpu_ctx.film_rgb()
        _hold("emitter %s" % (L,), truth, xyzw, rgb)
        assert np.array_equal(xyzw[..., 3], truth["weight"].astype(np.float32)) and truth["weight"].sum() == truth["n_contributing"]      # quarters, halves and ones: exact sums
        if want == 0.0:
            assert not xyzw[..., :3].any() and not rgb.any()
        elif want == 0.5:
            assert np.abs(rgb - 0.5).max() <= 1e-5
