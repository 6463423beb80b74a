"""Float64 restatement of the reference's delta lights -- lights/point.rs, spot.rs, distant.rs, their create_* transform products, and
SpatialLightDistribution::compute_distribution (core/lightdistrib/spatial.rs:113-196) over them -- with, for every evaluation, a bound on
what the same evaluation in f32 may differ by.  The bound is derived from the number of f32 roundings on the way (EPS = 2^-24 each, first
order) and the conditioning of the step, never from what the code under test returns.

Discontinuities: `falloff` jumps to 0 at cos_total_width and changes slope at cos_falloff_start.  An evaluation whose cos(theta) lies
within its own bound of either cosine is flagged `near` and left out of comparisons; callers count those and cap their share."""
import numpy as np

EPS = 2.0 ** -24
POINT, SPOT, DISTANT = 0, 1, 2
Y_WEIGHT = np.array([0.212671, 0.715160, 0.072169])


# ---------------------------------------------------------------- transforms (create_point_light, create_spot_light, create_distant_light)
def translate(v):
    m = np.eye(4)
    m[:3, 3] = v
    return m


def normalize(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def coordinate_system(d):
    """Vector3f::coordinate_system, the normalising variant (vector3.rs:72-83)."""
    v1 = normalize(d)
    v2 = normalize([-v1[2], 0.0, v1[0]]) if abs(v1[0]) > abs(v1[1]) else normalize([0.0, v1[2], -v1[1]])
    return v1, v2, normalize(np.cross(v1, v2))


def spot_light_to_world(ctm, frm, to):
    """ctm * Translate(from) * Inverse(dir_to_z), dir_to_z rows du, dv, dir (spot.rs:148-154)."""
    d, du, dv = coordinate_system(normalize(np.asarray(to, np.float64) - np.asarray(frm, np.float64)))
    dir_to_z = np.eye(4)
    dir_to_z[0, :3], dir_to_z[1, :3], dir_to_z[2, :3] = du, dv, d
    return np.asarray(ctm, np.float64) @ translate(frm) @ np.linalg.inv(dir_to_z)


def point_light_to_world(ctm, frm):
    """Translate(from) * light2world (point.rs:121): the opposite order to pbrt-v3."""
    return translate(frm) @ np.asarray(ctm, np.float64)


def distant_w_light(ctm, frm, to):
    """normalize(light_to_world.transform_vector(from - to)) (distant.rs:28, :144)."""
    return normalize(np.asarray(ctm, np.float64)[:3, :3] @ (np.asarray(frm, np.float64) - np.asarray(to, np.float64)))


def cone_cosines(coneangle, conedelta):
    """cos(radians(total_width)), cos(radians(falloff_start)) with falloff_start = coneangle - conedelta formed in f32 (spot.rs:160)."""
    total = np.float32(coneangle)
    start = np.float32(total - np.float32(conedelta))
    return float(np.cos(np.radians(np.float64(total)))), float(np.cos(np.radians(np.float64(start))))


# the f32 cosines differ from these by the rounding of x * (PI / 180) (an angle error of 2 EPS x) and cosf's own rounding
def cone_cosine_bound(angle_deg):
    return 2 * EPS * abs(np.radians(angle_deg)) + 2 * EPS


class Light:
    """kind POINT / SPOT: v = p_light; DISTANT: v = w_light.  w2l: world_to_light (3 x 3 part), SPOT only."""

    def __init__(self, kind, spectrum, v, w2l=None, cos_total=0.0, cos_start=0.0, radius=0.0, cos_bound=0.0):
        self.kind, self.spectrum, self.v = kind, np.asarray(spectrum, np.float64), np.asarray(v, np.float64)
        self.w2l = None if w2l is None else np.asarray(w2l, np.float64)[:3, :3]
        self.cos_total, self.cos_start, self.radius, self.cos_bound = cos_total, cos_start, radius, cos_bound


def spot(ctm, frm, to, intensity, coneangle=30.0, conedelta=5.0):
    l2w = spot_light_to_world(ctm, frm, to)
    ct, cs = cone_cosines(coneangle, conedelta)
    return Light(SPOT, intensity, l2w[:3, 3], np.linalg.inv(l2w), ct, cs, cos_bound=cone_cosine_bound(coneangle))


def point(ctm, frm, intensity):
    return Light(POINT, intensity, point_light_to_world(ctm, frm)[:3, 3])


def distant(ctm, frm, to, radiance, radius):
    return Light(DISTANT, radiance, distant_w_light(ctm, frm, to), radius=radius)


def from_record(dl, radius=0.0):
    """A Light from a pt_delta_light record (what the front end or SceneBuilder produced): the constructors' arithmetic in float64."""
    m = np.array(list(dl.light_to_world), np.float64).reshape(4, 4)
    mi = np.array(list(dl.world_to_light), np.float64).reshape(4, 4)
    sp = np.array(list(dl.spectrum), np.float64)
    if dl.kind == DISTANT:
        return Light(DISTANT, sp, normalize(m[:3, :3] @ np.array(list(dl.direction), np.float64)), radius=radius)
    if dl.kind == POINT:
        return Light(POINT, sp, m[:3, 3])
    ct = float(np.cos(np.radians(np.float64(dl.cone_total_width))))
    cs = float(np.cos(np.radians(np.float64(dl.cone_falloff_start))))
    return Light(SPOT, sp, m[:3, 3], mi, ct, cs, cos_bound=cone_cosine_bound(dl.cone_total_width))


# ---------------------------------------------------------------- falloff, sample_li, power
def falloff(light, w, w_abs_err=0.0):
    """SpotLight::falloff for world directions w (n, 3) known to w_abs_err per component: (value, abs bound, near).
    f32 roundings: transform_vector 5 per component on inputs that carry w_abs_err, normalize 8, delta 3, its fourth power 2."""
    w = np.asarray(w, np.float64)
    wl = w @ light.w2l.T
    mag = np.abs(w) @ np.abs(light.w2l).T                     # sum |m_ij w_j|: what the roundings of the products scale with
    wl_err = 5 * EPS * mag + np.abs(light.w2l).sum(1)[None, :] * np.reshape(np.asarray(w_abs_err, np.float64) * np.ones(len(w)), (-1, 1))
    ln = np.sqrt((wl * wl).sum(1))
    cos_t = wl[:, 2] / ln
    # d(cos) <= (|d wl_z| + |d len|) / len, |d len| <= |d wl|; then the normalisation's own 8 roundings
    cos_err = (wl_err[:, 2] + np.sqrt((wl_err ** 2).sum(1))) / ln + 8 * EPS
    span = light.cos_start - light.cos_total
    delta = (cos_t - light.cos_total) / span
    inside = cos_t >= light.cos_start
    outside = cos_t < light.cos_total
    val = np.where(outside, 0.0, np.where(inside, 1.0, delta ** 4))
    d_err = (cos_err + 2 * light.cos_bound) / span + 3 * EPS * np.abs(delta) + 2 * light.cos_bound * np.abs(delta) / span
    err = np.where(outside | inside, 0.0, 4 * np.abs(delta) ** 3 * d_err + 2 * EPS * delta ** 4)
    margin = cos_err + light.cos_bound
    near = (np.abs(cos_t - light.cos_total) <= margin) | (np.abs(cos_t - light.cos_start) <= margin)
    return val, err, near


def sample_li(light, p, p_abs_err=0.0):
    """Light::sample_li at points p (n, 3), each known to p_abs_err per component: dict(li (n, 3), wi (n, 3), li_rel (n,) relative
    bound on li's non-zero components, wi_err abs per component, near, target (n, 3) the visibility tester's far end).  pdf is 1."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n = len(p)
    if light.kind == DISTANT:
        return dict(li=np.tile(light.spectrum, (n, 1)), wi=np.tile(light.v, (n, 1)), li_rel=np.zeros(n), wi_err=np.full(n, 12 * EPS),
                    near=np.zeros(n, bool), target=p + light.v * (2.0 * light.radius), falloff=np.ones(n))
    d = light.v[None, :] - p
    d2 = (d * d).sum(1)
    dist = np.sqrt(d2)
    wi = d / dist[:, None]
    # the subtraction rounds once on operands of size |p_light| + |p|; the interaction point itself is uncertain by p_abs_err
    d_err = EPS * (np.abs(light.v)[None, :] + np.abs(p)).max(1) + p_abs_err
    wi_err = 2 * d_err / dist + 8 * EPS
    d2_rel = 2 * np.sqrt(3.0) * d_err / dist + 5 * EPS
    if light.kind == POINT:
        return dict(li=light.spectrum[None, :] / d2[:, None], wi=wi, li_rel=d2_rel + EPS, wi_err=wi_err, near=np.zeros(n, bool),
                    target=np.tile(light.v, (n, 1)), falloff=np.ones(n))
    f, f_err, near = falloff(light, -wi, wi_err)
    li = light.spectrum[None, :] * (f / d2)[:, None]
    rel = np.where(f > 0, f_err / np.where(f > 0, f, 1.0), 0.0) + d2_rel + 2 * EPS
    return dict(li=li, wi=wi, li_rel=rel, wi_err=wi_err, near=near, target=np.tile(light.v, (n, 1)), falloff=f)


def power(light):
    """Light::power: 4 pi I (point.rs:61-63), I 2 pi (1 - .5 (cf - ct)) (spot.rs:81-84), L pi r^2 (distant.rs:77-81)."""
    if light.kind == POINT:
        return light.spectrum * (4.0 * np.pi)
    if light.kind == SPOT:
        return light.spectrum * (2.0 * np.pi * (1.0 - 0.5 * (light.cos_start - light.cos_total)))
    return light.spectrum * (np.pi * light.radius * light.radius)


def luminance(c):
    return np.asarray(c, np.float64) @ Y_WEIGHT


# ---------------------------------------------------------------- light distributions
def radical_inverse(base, i):
    inv, r, f = 1.0 / base, 0.0, 1.0 / base
    while i:
        r += (i % base) * f
        i //= base
        f *= inv
    return r


PROBES = np.array([[radical_inverse(b, i) for b in (2, 3, 5, 7, 11)] for i in range(128)])


def distribution_pdf(func):
    """Distribution1D::new + discrete_pdf (distribution.rs:12-31, :88-106): func[i] / (func_int * n), func_int = mean(func)."""
    func = np.asarray(func, np.float64)
    return func / func.sum() if func.sum() > 0 else np.full(len(func), 1.0 / len(func))


def spatial_voxels(wb_min, wb_max, max_voxels=64):
    """SpatialLightDistribution::new (spatial.rs:36-58): voxels per axis."""
    diag = np.asarray(wb_max, np.float64) - np.asarray(wb_min, np.float64)
    return [int(min(max(np.ceil(diag[i] / diag.max() * max_voxels), 1), max_voxels)) for i in range(3)]


def voxel_of(p, wb_min, wb_max, voxels):
    """get_hash_key's voxel coordinates (spatial.rs:84-104) for points p (n, 3)."""
    wb_min, wb_max = np.asarray(wb_min, np.float64), np.asarray(wb_max, np.float64)
    ext = wb_max - wb_min
    o = np.where(ext > 0, (np.asarray(p, np.float64) - wb_min) / np.where(ext > 0, ext, 1.0), np.asarray(p, np.float64) - wb_min)
    o = np.clip(o, 0.0, 1.0)
    return np.minimum((o * np.array(voxels)).astype(np.int64), np.array(voxels) - 1)


def compute_distribution(lights, pi, wb_min, wb_max, voxels):
    """compute_distribution (spatial.rs:113-196) for voxel pi over delta lights: (pdf per light, relative bound per light, near).
    near: some probe of some light lies within its bound of a cone cosine, where one probe's term may flip between 0 and its value."""
    wb_min, wb_max = np.asarray(wb_min, np.float64), np.asarray(wb_max, np.float64)
    v = np.array(voxels, np.float64)
    lo = wb_min + (np.array(pi) / v) * (wb_max - wb_min)
    hi = wb_min + ((np.array(pi) + 1) / v) * (wb_max - wb_min)
    po = lo + PROBES[:, :3] * (hi - lo)
    p_err = 4 * EPS * np.abs(np.stack([wb_min, wb_max])).max()           # two lerps of two roundings each
    contrib, rel, near = np.zeros(len(lights)), np.zeros(len(lights)), False
    for j, lt in enumerate(lights):
        s = sample_li(lt, po, p_err)
        y = luminance(s["li"])
        contrib[j] = y.sum()
        near = near or bool(s["near"].any())
        rel[j] = ((s["li_rel"] + 3 * EPS) * y).sum() / contrib[j] + 128 * EPS if contrib[j] > 0 else 0.0
    avg = contrib.sum() / (128 * len(lights))
    floor = 0.001 * avg if avg > 0 else 1.0
    func = np.maximum(floor, contrib)
    # pdf_j = func_j / sum(func): its relative bound is func_j's plus the sum's (at most the largest), plus the table's own roundings
    return distribution_pdf(func), rel + rel.max() + (2 * len(lights) + 4) * EPS, near


# ---------------------------------------------------------------- shading closed forms
def lambert_term(kd, li, wi, n):
    """Kd / pi * Li * |cos| for a matte surface with normal n: what every integrator returns for an unoccluded delta light."""
    return np.asarray(kd, np.float64)[None, :] / np.pi * li * np.abs(np.asarray(wi) @ np.asarray(n, np.float64))[:, None]


def oren_nayar_f(kd, sigma_deg, wo, wi):
    """OrenNayar::f (oren_nayar.rs:16-66) in the local frame (z = normal) for unit wo (3,) and wi (n, 3)."""
    sigma = np.radians(sigma_deg)
    s2 = sigma * sigma
    a, b = 1.0 - s2 / (2.0 * (s2 + 0.33)), 0.45 * s2 / (s2 + 0.09)
    wo = np.asarray(wo, np.float64)
    ct_i, ct_o = np.abs(wi[:, 2]), abs(wo[2])
    st_i, st_o = np.sqrt(np.maximum(0.0, 1 - wi[:, 2] ** 2)), np.sqrt(max(0.0, 1 - wo[2] ** 2))
    max_cos = np.zeros(len(wi))
    ok = (st_i > 1e-4) & (st_o > 1e-4)
    if st_o > 1e-4:
        sp_i, cp_i = wi[:, 1] / np.where(ok, st_i, 1.0), wi[:, 0] / np.where(ok, st_i, 1.0)
        sp_o, cp_o = wo[1] / st_o, wo[0] / st_o
        max_cos = np.where(ok, np.maximum(0.0, cp_i * cp_o + sp_i * sp_o), 0.0)
    big = ct_i > ct_o
    sin_a = np.where(big, st_o, st_i)
    tan_b = np.where(big, st_i / ct_i, st_o / ct_o)
    return np.asarray(kd, np.float64)[None, :] / np.pi * (a + b * max_cos * sin_a * tan_b)[:, None]
