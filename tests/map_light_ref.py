"""Float64 restatement of the reference's two image-reading delta lights -- lights/goniometric.rs and lights/projection.rs, with the
bilinear triangle lookup of core/texture/mipmap.rs (MIPMap::lookup, triangle, texel; s repeat, t clamp) -- written from those files,
with, for every evaluation, a bound on what the same evaluation in f32 may differ by.  The bound counts the f32 roundings on the way
(EPS = 2^-24 each, first order) and adds the lookup's sensitivity: |d texel / d st| times the error of st.  It never comes from what the
code under test returns.

The quirks restated as the reference has them:
  goniometric  `scale` maps w with world_to_light.transform_point: the translation is added to a direction and the result is not
               normalised; spherical_theta clamps z into [-1, 1]; the y/z swap of pbrt-v3 is only a comment; st = (phi / 2 pi, theta / pi).
  projection   black when wl.z < 1e-3; transform_point of the perspective matrix with its homogeneous divide; Bounds2f::inside is
               inclusive on both ends; Bounds2f::offset gives st.
  both         lookup(st, 0): width 0 is below level 0, the bilinear triangle filter on level 0.  The map is not multiplied by the
               intensity; with no map it is a 1 x 1 image of ones.

Discontinuities: the projection's screen-bounds edge and its wl.z = 1e-3 plane; for the goniometric light theta's clamp at the poles
(and the pole itself, where phi is undefined).  An evaluation within its own bound of one of them is flagged `near` and left out of
comparisons; callers count those and cap their share.  Bilinear lookup is continuous across texel cells and across the s wrap."""
import numpy as np

import delta_light_ref as dref

EPS = dref.EPS
GONIOMETRIC, PROJECTION = 3, 4
HITHER = float(np.float32(1e-3))
YON = float(np.float32(1e30))
# pt_acosf / pt_atan2f are ports of a libm's: within 2 ulp of a result of size at most pi (acos) or 2 pi (atan2 + 2 pi), and the + 2 pi's own rounding
ACOS_ERR = 2 * EPS * np.pi
ATAN2_ERR = 3 * EPS * 2 * np.pi


# ---------------------------------------------------------------- the map
def pyramid(level0):
    """MIPMap::new over a power-of-two image (H, W, 3): every level halves the dimensions still > 1 with a * 0.5 + b * 0.5."""
    levels = [np.asarray(level0, np.float64)]
    while levels[-1].shape[0] * levels[-1].shape[1] != 1:
        cur = levels[-1]
        if cur.shape[1] > 1:
            cur = cur[:, 0::2] * 0.5 + cur[:, 1::2] * 0.5
        if cur.shape[0] > 1:
            cur = cur[0::2] * 0.5 + cur[1::2] * 0.5
        levels.append(cur)
    return levels


def _texel(img, s, t):
    h, w, _ = img.shape
    return img[np.clip(t, 0, h - 1), np.mod(s, w)]           # s repeat, t clamp (create_spectrum_mipmap)


def triangle(img, st, st_err=0.0):
    """MIPMap::triangle (mipmap.rs) on one level `img` (H, W, 3) at st (n, 2): (value (n, 3), abs bound (n, 3)).
    s = st.x * W - 0.5, s0 = floor(s), ds = s - s0; the four texels weighted (1 - ds)(1 - dt), (1 - ds) dt, ds (1 - dt), ds dt.
    Bound: the weights' roundings (s, ds, 1 - ds, the product: 5 each) and the 4 products and 3 sums, on the largest texel met, plus
    |d value / d st| * st_err with the derivative taken as the larger texel difference along each axis over the cell -- and over the cells
    st +- st_err falls into, since the slope changes from cell to cell though the value does not jump."""
    st = np.asarray(st, np.float64).reshape(-1, 2)
    st_err = np.broadcast_to(np.asarray(st_err, np.float64), st.shape)
    h, w, _ = img.shape

    def cell(q):
        s, t = q[:, 0] * w - 0.5, q[:, 1] * h - 0.5
        s0, t0 = np.floor(s).astype(np.int64), np.floor(t).astype(np.int64)
        ds, dt = (s - s0)[:, None], (t - t0)[:, None]
        a, b, c, e = _texel(img, s0, t0), _texel(img, s0, t0 + 1), _texel(img, s0 + 1, t0), _texel(img, s0 + 1, t0 + 1)
        val = a * ((1 - ds) * (1 - dt)) + b * ((1 - ds) * dt) + c * (ds * (1 - dt)) + e * (ds * dt)
        slope_s = np.maximum(np.abs(c - a), np.abs(e - b)) * w
        slope_t = np.maximum(np.abs(b - a), np.abs(e - c)) * h
        big = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(e)))
        return val, slope_s, slope_t, big
    val, ss, stt, big = cell(st)
    for sign in (-1.0, 1.0):
        for axis in (0, 1):
            q = st.copy()
            q[:, axis] += sign * st_err[:, axis]
            _, s2, t2, b2 = cell(q)
            ss, stt, big = np.maximum(ss, s2), np.maximum(stt, t2), np.maximum(big, b2)
    # st * W - 0.5 rounds twice on a number of size |st| W + 0.5: as an error of st, 2 EPS (|st| + 1 / W)
    e_s = st_err[:, 0:1] + 2 * EPS * (np.abs(st[:, 0:1]) + 1.0 / w)
    e_t = st_err[:, 1:2] + 2 * EPS * (np.abs(st[:, 1:2]) + 1.0 / h)
    return val, ss * e_s + stt * e_t + 12 * EPS * big


def lookup_trilinear(levels, st, width):
    """MIPMap::lookup(st, width) for one st (2,): the host's power() call."""
    max_level = len(levels) - 1
    level = max_level + np.log2(max(width, 1e-8))
    st = np.asarray(st, np.float64).reshape(1, 2)
    if level < 0:
        return triangle(levels[0], st)[0][0]
    if level >= max_level:
        return levels[-1][0, 0]
    il = int(np.floor(level))
    d = min(max(level - il, 0.0), 1.0)
    return (1 - d) * triangle(levels[il], st)[0][0] + d * triangle(levels[il + 1], st)[0][0]


# ---------------------------------------------------------------- the lights
class MapLight:
    """kind GONIOMETRIC / PROJECTION.  w2l: world_to_light (4 x 4).  levels: the map's pyramid.  PROJECTION: proj = light_projection.m,
    screen = (min.x, min.y, max.x, max.y), cos_total; proj_rel: relative bound on the f32 matrix' 1 / tan(fov / 2) entries."""

    def __init__(self, kind, spectrum, p_light, w2l, levels, proj=None, screen=None, cos_total=1.0, proj_rel=0.0):
        self.kind, self.spectrum, self.v = kind, np.asarray(spectrum, np.float64), np.asarray(p_light, np.float64)
        self.w2l, self.levels = np.asarray(w2l, np.float64), levels
        self.proj, self.screen, self.cos_total, self.proj_rel = proj, screen, cos_total, proj_rel
        self.point = dref.Light(dref.POINT, self.spectrum, self.v)          # wi, distance and the visibility target are the point light's


def perspective(fov, n=HITHER, f=YON):
    """Transform::perspective (transform.rs:89-99): scale(1 / tan(radians(fov) / 2)) * persp."""
    persp = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, f / (f - n), -f * n / (f - n)], [0, 0, 1.0, 0]])
    it = 1.0 / np.tan(np.radians(fov) / 2.0)
    return np.diag([it, it, 1.0, 1.0]) @ persp


def screen_bounds(resolution):
    aspect = float(resolution[0]) / float(resolution[1])
    return (-aspect, -1.0, aspect, 1.0) if aspect > 1.0 else (-1.0, -1.0 / aspect, 1.0, 1.0 / aspect)


def transform_point(m, p):
    q = m @ np.append(np.asarray(p, np.float64), 1.0)
    return q[:3] if q[3] == 1.0 else q[:3] / q[3]


def goniometric(light_to_world, spectrum, level0):
    l2w = np.asarray(light_to_world, np.float64)
    return MapLight(GONIOMETRIC, spectrum, l2w[:3, 3], np.linalg.inv(l2w), pyramid(level0))


def projection(light_to_world, spectrum, level0, fov, resolution, world_to_light=None):
    """ProjectionLight::new (projection.rs:19-57)."""
    l2w = np.asarray(light_to_world, np.float64)
    proj = perspective(fov)
    sb = screen_bounds(resolution)
    corner = dref.normalize(transform_point(np.linalg.inv(proj), (sb[2], sb[3], 0.0)))
    # radians(fov) / 2 = h carries the roundings of PI / 180 and of the product (2 EPS, relative); d(1 / tan h) / (1 / tan h) = 2 h / sin 2h times that;
    # then tanf (2 ulp), the reciprocal and the matrix product's one rounding
    h = np.radians(fov) / 2.0
    proj_rel = (2 * (2 * h / np.sin(2 * h)) + 4) * EPS
    w2l = np.linalg.inv(l2w) if world_to_light is None else np.asarray(world_to_light, np.float64)
    return MapLight(PROJECTION, spectrum, l2w[:3, 3], w2l, pyramid(level0), proj, sb, float(corner[2]), proj_rel)


def from_record(ml, level0):
    """A MapLight from a pt_map_light record (what the front end or SceneBuilder produced) and its image's level 0 (H, W, 3): the
    constructors' arithmetic in float64 on the record's f32 fields."""
    m = np.array(list(ml.light_to_world), np.float64).reshape(4, 4)
    mi = np.array(list(ml.world_to_light), np.float64).reshape(4, 4)
    sp = np.array(list(ml.spectrum), np.float64)
    if ml.kind == GONIOMETRIC:
        return MapLight(GONIOMETRIC, sp, m[:3, 3], mi, pyramid(level0))
    return projection(m, sp, level0, float(ml.fov), (int(ml.resolution[0]), int(ml.resolution[1])), world_to_light=mi)


# ---------------------------------------------------------------- scale, sample_li, power
def _linear(m3, w, w_err):
    """m3 (3 x 3) times directions w (n, 3) known to w_err (n,) per component: (value, abs bound): 5 roundings per component on the
    products' sizes, plus the input's error through the matrix."""
    val = w @ m3.T
    mag = np.abs(w) @ np.abs(m3).T
    return val, 5 * EPS * mag + np.abs(m3).sum(1)[None, :] * np.reshape(w_err, (-1, 1))


def gonio_scale(light, w, w_err=0.0):
    """GonioPhotometricLight::scale (goniometric.rs:35-44) for world directions w (n, 3): (rgb (n, 3), abs bound (n, 3), near (n,))."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    w_err = np.broadcast_to(np.asarray(w_err, np.float64), (len(w),))
    lin, lin_err = _linear(light.w2l[:3, :3], w, w_err)
    t = light.w2l[:3, 3]
    wp = lin + t[None, :]                                         # transform_point: the translation added to a direction, no normalisation
    wp_err = lin_err + EPS * (np.abs(lin) + np.abs(t)[None, :])   # one more rounding, on a sum of that size
    z = wp[:, 2]
    zc = np.clip(z, -1.0, 1.0)
    theta = np.arccos(zc)
    clamped = np.abs(z) > 1.0
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - zc * zc))
    with np.errstate(divide="ignore", invalid="ignore"):
        theta_err = np.where(clamped, 0.0, wp_err[:, 2] / sin_t) + ACOS_ERR
    r2 = wp[:, 0] ** 2 + wp[:, 1] ** 2
    phi = np.arctan2(wp[:, 1], wp[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi_err = (np.abs(wp[:, 0]) * wp_err[:, 1] + np.abs(wp[:, 1]) * wp_err[:, 0]) / r2 + ATAN2_ERR
    # near: theta's clamp (|z| within its bound of 1: the slope of acos is unbounded there, and beyond it theta stops moving), and the axis,
    # where phi is undefined
    near = (np.abs(np.abs(z) - 1.0) <= 4 * wp_err[:, 2] + 64 * EPS) | (np.sqrt(r2) <= 4 * np.maximum(wp_err[:, 0], wp_err[:, 1]))
    st = np.stack([phi / (2 * np.pi), theta / np.pi], 1)
    # INV_2_PI, INV_PI are rounded constants, the products round once
    st_err = np.stack([phi_err / (2 * np.pi) + 2 * EPS * st[:, 0], theta_err / np.pi + 2 * EPS * st[:, 1]], 1)
    st_err = np.where(np.isfinite(st_err), st_err, 1.0)
    val, err = triangle(light.levels[0], st, st_err)
    return val, err, near


def projection_scale(light, w, w_err=0.0):
    """ProjectionLight::projection (projection.rs:59-76): (rgb (n, 3), abs bound (n, 3), near (n,), region (n,): 0 lit, 1 outside the
    image, 2 behind the near plane)."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    w_err = np.broadcast_to(np.asarray(w_err, np.float64), (len(w),))
    wl, wl_err = _linear(light.w2l[:3, :3], w, w_err)             # transform_vector
    behind = wl[:, 2] < HITHER
    near = np.abs(wl[:, 2] - HITHER) <= wl_err[:, 2]
    z = np.where(behind, 1.0, wl[:, 2])
    it = light.proj[0, 0]
    # rows 0, 1 of light_projection are (it 0 0 0), (0 it 0 0), row 3 is (0 0 1 0): p = it * wl.xy / wl.z after one product's rounding and the divide's
    p = it * wl[:, :2] / z[:, None]
    p_err = np.abs(p) * (light.proj_rel + 2 * EPS + (wl_err[:, 2] / np.abs(z))[:, None]) + it * wl_err[:, :2] / np.abs(z)[:, None]
    lo, hi = np.array(light.screen[:2]), np.array(light.screen[2:])
    b_err = 2 * EPS * np.abs(hi)                                  # aspect = x / y and 1 / aspect in f32
    inside = ((p >= lo) & (p <= hi)).all(1)                       # Bounds2f::inside: inclusive on both ends
    near |= ~behind & ((np.abs(p - lo) <= p_err + b_err) | (np.abs(p - hi) <= p_err + b_err)).any(1)
    span = hi - lo
    st = (p - lo) / span                                          # Bounds2f::offset
    st_err = (p_err + 3 * b_err) / span + 3 * EPS * np.abs(st)
    lit = ~behind & inside
    val, err = triangle(light.levels[0], np.where(lit[:, None], st, 0.5), np.where(lit[:, None], st_err, 0.0))
    val, err = np.where(lit[:, None], val, 0.0), np.where(lit[:, None], err, 0.0)
    return val, err, near, np.where(behind, 2, np.where(inside, 0, 1))


def sample_li(light, p, p_abs_err=0.0):
    """Light::sample_li at points p (n, 3), each known to p_abs_err per component (goniometric.rs:48-64, projection.rs:80-97):
    dict(li (n, 3), wi, li_err (n, 3) absolute, li_rel (n,) = the largest li_err / li over the channels (0 where black), wi_err, near,
    target, scale (n, 3), region).  pdf is 1.  Li = intensity * scale(-wi) / distance_squared."""
    s = dref.sample_li(light.point, p, p_abs_err)                 # li = I / d^2 with li_rel = the distance's bound + 1 rounding
    if light.kind == GONIOMETRIC:
        sc, sc_err, near = gonio_scale(light, -s["wi"], s["wi_err"])
        region = np.zeros(len(sc), np.int64)
    else:
        sc, sc_err, near, region = projection_scale(light, -s["wi"], s["wi_err"])
    li = s["li"] * sc
    li_err = s["li"] * sc_err + li * (s["li_rel"] + 2 * EPS)[:, None]      # I * scale (1 rounding), / d^2 (1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(li > 0, li_err / np.where(li > 0, li, 1.0), 0.0).max(1)
    return dict(li=li, wi=s["wi"], li_err=li_err, li_rel=rel, wi_err=s["wi_err"], near=near, target=s["target"], scale=sc, region=region)


def power(light):
    """4 pi I lookup((.5, .5), .5) (goniometric.rs:66-70); I lookup((.5, .5), .5) 2 pi (1 - cos_total_width) (projection.rs:99-103)."""
    c = lookup_trilinear(light.levels, (0.5, 0.5), 0.5)
    if light.kind == GONIOMETRIC:
        return 4.0 * np.pi * light.spectrum * c
    return c * light.spectrum * (2.0 * np.pi * (1.0 - light.cos_total))


# ---------------------------------------------------------------- record builders for the two directives
def goniometric_record(ctm, L, scale):
    """create_goniometric_light: light_to_world is the CTM, the spectrum "L" * "scale" in f32."""
    return dict(light_to_world=np.asarray(ctm, np.float64), spectrum=(np.float32(L) * np.float32(scale)).astype(np.float64))


def projection_record(ctm, I, scale, fov=45.0, resolution=(1, 1)):
    """create_projection_light: the CTM, "I" * "scale" in f32, "fov" (default 45) and the map's resolution as read."""
    return dict(light_to_world=np.asarray(ctm, np.float64), spectrum=(np.float32(I) * np.float32(scale)).astype(np.float64), fov=float(np.float32(fov)),
                resolution=(int(resolution[0]), int(resolution[1])))
