"""Next-event estimation's light record through both of its address spaces, against the oracle bit for bit.

The shading kernels keep the light table in LDS when the scene has at most 8 lights and read it from global memory otherwise; shade_body
instantiates the estimate once per address space.  A closed matte box with 1, 2, 8 (the last LDS slot) and 9 (the global path) emissive
triangles under its ceiling, 16 x 16 pixels, 4 spp, depth 5: per-sample radiance and the ray counters equal the oracle's.  The second
material set puts a plastic floor in, so that the material-sorted pair (k_shade_matte_sorted + k_shade_general) shades the scene instead
of k_shade.

A scene is accepted only if the oracle ALONE shows samples that pick its first and its last light: the first light's radiance has a red
component, the last one's a blue one, every light a green one, the walls are grey.  At depth 1 a sample whose camera ray meets no emitter
returns the estimate of the one light picked at its first vertex, so red > 0 there means the first light was picked, blue > 0 the last."""
import numpy as np
import pytest

from helpers import bits, scenes

pytestmark = pytest.mark.gpu

RES, SPP = 16, 4
LIGHT_Z = 0.96
COUNTS = [1, 2, 8, 9]
MATERIALS = ["matte", "matte_plastic"]


def box_scene(n_lights, materials, maxdepth):
    sb = scenes.SceneBuilder()
    sb.look_at((0.0, -0.9, -0.2), (0.0, 1.0, -0.6), (0, 0, 1))
    sb.camera_perspective(fov=70.0)
    sb.film(xresolution=RES, yresolution=RES)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=SPP)
    sb.integrator_path(maxdepth=maxdepth)

    def quad(p0, p1, p2, p3):
        sb.shape_trianglemesh([p0, p1, p2, p3], [0, 1, 2, 0, 2, 3])
    grey = (0.6, 0.6, 0.6)
    sb.material_matte(grey)
    quad((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1))            # ceiling
    quad((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1))        # x = -1
    quad((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1))            # x = +1
    quad((-1, -1, -1), (-1, -1, 1), (1, -1, 1), (1, -1, -1))        # y = -1
    quad((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1))            # y = +1
    if materials == "matte_plastic":
        sb.material_plastic(Kd=(0.4, 0.4, 0.4), Ks=(0.3, 0.3, 0.3), roughness=0.2)
    quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1))        # floor
    sb.material_matte(grey)
    for i in range(n_lights):                                        # a 3 x 3 raster of small triangles under the ceiling, in list order
        cx, cy = -0.6 + 0.6 * (i % 3), -0.6 + 0.6 * (i // 3)
        L = (6.0 if i == 0 else 0.0, 3.0, 6.0 if i == n_lights - 1 else 0.0)
        sb.area_light_source_diffuse(L=L, twosided=True)
        sb.shape_trianglemesh([(cx - 0.15, cy - 0.15, LIGHT_Z), (cx + 0.15, cy - 0.15, LIGHT_Z), (cx, cy + 0.15, LIGHT_Z)], [0, 1, 2])
    sb.no_area_light()
    return sb.build()


def oracle_shows_first_and_last_pick(oracle, n_lights, materials):
    """From the oracle alone: (samples that picked the first light, samples that picked the last) at the first vertex of a depth-1 render."""
    osc = oracle.scene(box_scene(n_lights, materials, 1))
    b = list(osc.info.sample_bounds)
    rad = osc.radiance_samples(tuple(b)).reshape(-1, 3)
    ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
    pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), SPP, axis=0).astype(np.int32)
    o, d, _ = osc.generate_camera_rays(pix, np.tile(np.arange(SPP, dtype=np.uint32), len(xs.reshape(-1))))
    hit, _ = osc.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    z = o[:, 2] + hit["t"] * d[:, 2]
    wall = (hit["prim"] >= 0) & (np.abs(z - LIGHT_Z) > 1e-3)           # the camera ray met no emitter: all of the radiance is the estimate
    osc.close()
    return int((wall & (rad[:, 0] > 0)).sum()), int((wall & (rad[:, 2] > 0)).sum()), int(wall.sum())


@pytest.mark.parametrize("materials", MATERIALS)
@pytest.mark.parametrize("n_lights", COUNTS)
def test_light_record_from_lds_and_from_global(gpu_ctx, oracle, n_lights, materials):
    first, last, walls = oracle_shows_first_and_last_pick(oracle, n_lights, materials)
    print("%d lights, %s: of %d wall samples the oracle picks the first light %d times, the last %d times" % (n_lights, materials, walls, first, last))
    assert first > 0 and last > 0, (first, last, walls)

    sd = box_scene(n_lights, materials, 5)
    osc = oracle.scene(sd)
    info = gpu_ctx.upload(sd)
    assert info.n_lights == n_lights == osc.info.n_lights
    b = tuple(info.sample_bounds)
    g = gpu_ctx.radiance_samples(b)
    r = osc.radiance_samples(b)
    assert r.sum() > 0 and np.isfinite(r).all()
    differ = int((bits(g) != bits(r)).any(-1).sum())
    print("per-sample radiance: %d of %d samples differ" % (differ, g.shape[0] * g.shape[1]))
    assert differ == 0
    gpu_ctx.film_clear()
    gpu_ctx.reset_counters()
    gpu_ctx.render()
    gc = gpu_ctx.counters()
    _, oc, _ = osc.render(threads=4, want_image=False)
    osc.close()
    for k in ("camera_rays", "regular_rays", "shadow_rays", "path_vertices", "nodes_visited", "tris_tested"):
        assert gc[k] == oc[k], (k, gc[k], oc[k])
