"""The scenes, maps, light poses and closed forms the goniometric / projection light tests share: tests/test_map_light_host.py proves on
the CPU, with the float64 restatement alone (tests/map_light_ref.py), that these poses give lit, black-outside-the-image and
black-behind samples and keep the share of samples near a discontinuity under the cap; tests/test_gpu_map_light.py renders them."""
import numpy as np

import delta_light_ref as dref
import map_light_ref as mref
from helpers import scenes

EPS = mref.EPS
KD = (0.6, 0.5, 0.4)
FLOOR = (-2.0, 2.0, -2.0, 2.0)                  # x0 x1 y0 y1 at z = 0: a quad of side 4
EXTENT = 4.0                                    # coordinates of everything a test looks at stay below this
P_ERR = 16 * EPS * EXTENT                       # a hit point rebuilt from barycentrics in f32: at most 7 roundings on terms below EXTENT, doubled
NEAR_CAP = 0.02
T = scenes


def make_map(w, h):
    """A (h, w, 3) map of distinct positive texels (at most 96 of them: 37 is coprime to 97)."""
    idx = np.arange(w * h * 3)
    return (0.2 + ((idx * 37) % 97) / 60.0).astype(np.float32).reshape(h, w, 3)


MAP_4x2, MAP_8x4 = make_map(4, 2), make_map(8, 4)


def chain(*ts):
    out = ts[0]
    for t in ts[1:]:
        out = T.transform_mul(out, t)
    return out


def rotate_y(deg):
    """A rotation about y as an (m, m_inv) pair of f32 matrices (any affine pair will do for a record)."""
    a = np.radians(deg)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return m.astype(np.float32).reshape(-1), m.T.astype(np.float32).reshape(-1)


# light poses: (m, m_inv) pairs as SceneBuilder takes them
# goniometric: above the floor, rotated and non-uniformly scaled; the scale keeps the translation's image in light space small, so that
# world_to_light.transform_point(w) = M^-1 w - M^-1 t stays inside the unit ball's z range and theta varies over the floor
GONIO_CTM = chain(T.transform_translate(0.3, -0.2, 1.5), T.transform_rotate_x(20.0), T.transform_scale(3.0, 2.0, 4.0))
GONIO = dict(L=(30.0, 20.0, 10.0), scale=(0.5, 1.0, 1.5))
# projection, looking down: light space +z is world -z (a half turn about x, tilted by 10 degrees); fov 45 at height 2.5 lights a
# rectangle of about 4.1 x 2.1 for the 4 x 2 map: its long edges lie across the quad
PROJ_DOWN_CTM = chain(T.transform_translate(0.2, -0.3, 2.5), T.transform_rotate_x(170.0))
# projection, grazing: from the quad's left, aimed along +x and 10 degrees down: floor points behind the light's plane are black-behind
PROJ_GRAZE_CTM = chain(T.transform_translate(-1.0, 0.1, 0.8), rotate_y(100.0), T.transform_rotate_x(15.0))
PROJ = dict(I=(40.0, 30.0, 20.0), scale=(1.0, 0.5, 2.0))
# the hooks' second transform: translated, rotated, non-uniformly scaled
HOOK_CTM = chain(T.transform_translate(0.5, -0.25, 0.75), T.transform_rotate_x(25.0), T.transform_scale(1.5, 0.75, 2.0))


def hook_points(light_to_world, seed=11):
    """600 f32 points for the light hooks: 300 in front of the light around its +z axis (the projector's image and its surroundings),
    100 behind it, 200 anywhere in a box of side 6."""
    m = np.asarray(light_to_world, np.float64).reshape(4, 4)
    rng = np.random.default_rng(seed)
    axis = dref.normalize(m[:3, :3] @ np.array([0.0, 0.0, 1.0]))
    pos = m[:3, 3]
    return np.concatenate([pos + rng.uniform(0.5, 3.0, (300, 1)) * dref.normalize(axis + rng.normal(0, 0.5, (300, 3))),
                           pos - rng.uniform(0.5, 3.0, (100, 1)) * dref.normalize(axis + rng.normal(0, 0.5, (100, 3))),
                           rng.uniform(-3, 3, (200, 3))]).astype(np.float32).astype(np.float64)


def add_gonio(sb, image=MAP_4x2, ctm=GONIO_CTM, **over):
    g = dict(GONIO, **over)
    return sb.light_goniometric(L=g["L"], scale=g["scale"], image=image, ctm=ctm)


def add_proj(sb, image=MAP_4x2, ctm=PROJ_DOWN_CTM, fov=45.0, resolution=None, **over):
    g = dict(PROJ, **over)
    return sb.light_projection(I=g["I"], scale=g["scale"], fov=fov, image=image, resolution=resolution, ctm=ctm)


LIGHTS = {
    "goniometric": lambda sb: add_gonio(sb),
    "projection": lambda sb: add_proj(sb),
    "projection_grazing": lambda sb: add_proj(sb, image=MAP_8x4, ctm=PROJ_GRAZE_CTM, fov=60.0),
}


def base(integrator="path", sampler="sobol", res=16, spp=4, **kw):
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=res, yresolution=res)
    sb.pixel_filter_box()
    (sb.sampler_halton if sampler == "halton" else sb.sampler_sobol)(pixelsamples=spp)
    if integrator == "path":
        sb.integrator_path(maxdepth=kw.get("maxdepth", 5), lightsamplestrategy=kw.get("strategy", "spatial"))
    elif integrator == "whitted":
        sb.integrator_whitted(maxdepth=kw.get("maxdepth", 5))
    else:
        sb.integrator_directlighting(maxdepth=kw.get("maxdepth", 5), strategy=integrator)          # "all" / "one"
    return sb


def quad(sb, x0, x1, y0, y1, z, uv=False):
    sb.shape_trianglemesh([x0, y0, z, x1, y0, z, x1, y1, z, x0, y1, z], [0, 1, 2, 0, 2, 3], uv=[0, 0, 1, 0, 1, 1, 0, 1] if uv else None)


def floor(sb, **kw):
    sb.material_matte(KD, **kw)
    quad(sb, FLOOR[0], FLOOR[1], FLOOR[2], FLOOR[3], 0.0)


def level0(sd_or_builder_images, index):
    """Level 0 (H, W, 3) of image `index` of a SceneBuilder's image list [(pt_image, buffer)]."""
    im, buf = sd_or_builder_images[index]
    return np.asarray(buf[:im.width * im.height * 3], np.float64).reshape(im.height, im.width, 3)


def restate_lights(sb, radius=0.0):
    """The builder's delta and map lights restated, in light-list order: [(light_index, restated light)]."""
    out = [(dl.light_index, dref.from_record(dl, radius)) for dl in sb.delta_lights]
    out += [(ml.light_index, mref.from_record(ml, level0(sb.images, ml.image))) for ml in sb.map_lights]
    return [lt for _, lt in sorted(out, key=lambda e: e[0])]


def light_sample(lt, p, p_err=0.0):
    """sample_li of a restated delta or map light in one shape: li, wi, li_rel, wi_err, near, target, lit-independent."""
    if isinstance(lt, mref.MapLight):
        return mref.sample_li(lt, p, p_err)
    return dref.sample_li(lt, p, p_err)


def camera_rays(res=16, spp=4):
    """The camera of base() in float64, one ray through a regular sub-pixel grid per sample: where the GPU tests' samples fall, closely
    enough to count regions and near shares on the CPU (the film's own sample positions need the device)."""
    eye, at, up = np.array([0.0, -4.0, 3.0]), np.zeros(3), np.array([0.0, 0.0, 1.0])
    fwd = dref.normalize(at - eye)
    right = dref.normalize(np.cross(fwd, up))
    upv = np.cross(right, fwd)
    k = int(np.ceil(np.sqrt(spp)))
    g = (np.arange(res * k) + 0.5) / (res * k) * 2 - 1
    xs, ys = np.meshgrid(g, -g)
    tan = np.tan(np.radians(50.0) / 2)
    d = fwd[None, :] + tan * xs.reshape(-1, 1) * right[None, :] + tan * ys.reshape(-1, 1) * upv[None, :]
    return np.tile(eye, (len(d), 1)), dref.normalize(d)


def plane_hit(o, d, z, rect, p_err):
    """Where rays o + t d meet the rectangle rect = (x0 x1 y0 y1) of the plane at height z: (p, hit, near the rectangle's edge)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (z - o[:, 2]) / d[:, 2]
    p = o + t[:, None] * d
    p[:, 2] = z
    ok = np.isfinite(t) & (t > 0)
    ex = np.minimum(np.minimum(p[:, 0] - rect[0], rect[1] - p[:, 0]), np.minimum(p[:, 1] - rect[2], rect[3] - p[:, 1]))
    return p, ok & (ex > 0), ok & (np.abs(ex) <= p_err)


def light_terms(lights, p, occluders=(), p_err=P_ERR, brdf=None):
    """Per light: (c (n, 3) = f Li |cos| at floor points p with the shadow applied, relative bound (n,), near (n,), lit (n,) bool =
    non-black f Li before the shadow test).  occluders: rectangles (x0 x1 y0 y1 z) in horizontal planes."""
    out = []
    for lt in lights:
        s = light_sample(lt, p, p_err)
        cos = s["wi"][:, 2]
        f = np.tile(np.array(KD) / np.pi, (len(p), 1)) if brdf is None else brdf(s["wi"])
        c = f * s["li"] * np.abs(cos)[:, None]
        # Kd * INV_PI (2 roundings), |wi . n| (5, on a wi known to wi_err per component), f cos, f Li, then beta * (Ld / pdf) and L += (4)
        rel = s["li_rel"] + 3 * s["wi_err"] / np.maximum(np.abs(cos), 1e-30) + 14 * EPS
        near = s["near"].copy()
        lit = (s["li"].sum(1) > 0) & (np.abs(cos) > 0)
        for (x0, x1, y0, y1, z) in occluders:
            tgt = s["target"]
            with np.errstate(divide="ignore", invalid="ignore"):
                u = (z - p[:, 2]) / (tgt[:, 2] - p[:, 2])
            q = p + u[:, None] * (tgt - p)
            crosses = np.isfinite(u) & (u > 0) & (u < 1)
            ex = np.minimum(np.minimum(q[:, 0] - x0, x1 - q[:, 0]), np.minimum(q[:, 1] - y0, y1 - q[:, 1]))
            # the f32 shadow segment starts at the error-offset point and ends at the f32 light: its crossing moves by a few p_err
            margin = 8 * p_err + 64 * EPS * EXTENT
            near |= crosses & (np.abs(ex) <= margin)
            near |= np.isfinite(u) & (np.abs(u - 1) <= 1e-3) & (ex > -margin)          # an occluder at the segment's very end
            c = np.where((crosses & (ex > 0))[:, None], 0.0, c)
        out.append((c, rel, near, lit))
    return out
