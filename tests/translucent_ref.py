"""TranslucentMaterial (materials/translucent.rs:38-107) and LambertianTransmission (core/reflection/lambertian.rs:49-99) restated in
numpy, independent of the library: the lobe list from the parameters, and BSDF::f / pdf / sample_f over it with the reference's
matching, averaging and geometric-normal rules (core/reflection/bsdf.rs:111-234) on the canonical frame (ns = ng = +z).

Everything is float64 except `diffuse_f32_*`, which restate the diffuse-only material in float32 operation for operation (it is a
handful of operations: t * kd, * INV_PI, a sum with 0, a division by the matching count), so the device can be held to it bit for bit.

sample_f draws from the two Lambertian lobes only: a glossy lobe's sampling (TrowbridgeReitz::sample_wh) is not restated here -- the
glossy half of the material is held bit for bit to uber / glass, which the oracle pins (tests/test_gpu_translucent.py)."""
import numpy as np

REFL, TRANS, DIFFUSE, GLOSSY, SPECULAR = 1, 2, 4, 8, 16
ALL = 31
ETA = 1.5                                   # translucent.rs:48: a constant, "eta" / "index" are not read
f32 = np.float32
INV_PI32 = f32(0.31830988618379067154)


def roughness_to_alpha(r):                  # trowbridge_reitz.rs:113-121
    x = np.log(max(float(r), 1e-3))
    return 1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x ** 3 + 0.000640711 * x ** 4


def lobes(Kd=(0.25,) * 3, Ks=(0.25,) * 3, reflect=(0.5,) * 3, transmit=(0.5,) * 3, roughness=0.1, remaproughness=True):
    """None: compute_scattering_functions returns before it sets si.bsdf (r and t black).  Otherwise the BxDFs in the order they are
    added -- possibly none at all (an empty BSDF: the path ends there, it does not pass through)."""
    cz = lambda c: np.maximum(np.asarray(c, np.float64), 0.0)
    black = lambda c: not np.any(c != 0.0)
    r, t = cz(reflect), cz(transmit)
    if black(r) and black(t):
        return None
    out = []
    kd = cz(Kd)
    if not black(kd):
        if not black(r):
            out.append({"kind": "lambert_r", "type": REFL | DIFFUSE, "c": r * kd})
        if not black(t):
            out.append({"kind": "lambert_t", "type": TRANS | DIFFUSE, "c": t * kd})
    ks = cz(Ks)
    if not black(ks):
        a = roughness_to_alpha(roughness) if remaproughness else float(roughness)
        a = max(a, 1e-3)                    # TrowbridgeReitzDistribution::new
        if not black(r):
            out.append({"kind": "mf_r", "type": REFL | GLOSSY, "c": r * ks, "alpha": a})
        if not black(t):
            out.append({"kind": "mf_t", "type": TRANS | GLOSSY, "c": t * ks, "alpha": a})
    return out


# ---- the BxDFs (local frame, arrays of directions (n, 3))
def _same_hemisphere(wo, wi):
    return wo[:, 2] * wi[:, 2] > 0


def lambert_t_pdf(wo, wi):
    """lambertian.rs:80-86: |cos theta_i| on the other hemisphere -- WITHOUT the INV_PI of pbrt-v3 and of LambertianReflection."""
    return np.where(~_same_hemisphere(wo, wi), np.abs(wi[:, 2]), 0.0)


def lambert_r_pdf(wo, wi):
    return np.where(_same_hemisphere(wo, wi), np.abs(wi[:, 2]) / np.pi, 0.0)


def _fr_dielectric(cos_i, eta_i, eta_t):    # fresnel.rs fr_dielectric
    cos_i = np.clip(cos_i, -1.0, 1.0)
    ent = cos_i > 0
    ei = np.where(ent, eta_i, eta_t); et = np.where(ent, eta_t, eta_i)
    ci = np.abs(cos_i)
    st = ei / et * np.sqrt(np.maximum(0.0, 1 - ci * ci))
    ct = np.sqrt(np.maximum(0.0, 1 - st * st))
    rl = (et * ci - ei * ct) / (et * ci + ei * ct)
    rp = (ei * ci - et * ct) / (ei * ci + et * ct)
    return np.where(st >= 1, 1.0, 0.5 * (rl * rl + rp * rp))


def _tr_d(a, wh):                           # isotropic TrowbridgeReitz (rough, rough)
    c2 = wh[:, 2] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t2 = (1 - c2) / c2
        d = 1.0 / (np.pi * a * a * c2 * c2 * (1 + t2 / (a * a)) ** 2)
    return np.where(np.isfinite(t2), d, 0.0)


def _tr_lambda(a, w):
    c2 = w[:, 2] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t2 = (1 - c2) / c2
        lam = (-1 + np.sqrt(1 + a * a * t2)) / 2
    return np.where(np.isfinite(t2), lam, 0.0)


def _norm(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tr_pdf(a, wo, wh):
    with np.errstate(divide="ignore", invalid="ignore"):
        return _tr_d(a, wh) / (1 + _tr_lambda(a, wo)) * np.abs((wo * wh).sum(1)) / np.abs(wo[:, 2])


def lobe_f(l, wo, wi):
    n = len(wo)
    if l["kind"] in ("lambert_r", "lambert_t"):
        return np.tile(l["c"] / np.pi, (n, 1))
    a = l["alpha"]
    with np.errstate(divide="ignore", invalid="ignore"):
        if l["kind"] == "mf_r":                  # microfacet.rs MicrofacetReflection::f, FresnelDielectric(1, 1.5)
            co, ci = np.abs(wo[:, 2]), np.abs(wi[:, 2])
            wh = wi + wo
            bad = (co == 0) | (ci == 0) | ~np.any(wh != 0, axis=1)
            wh = _norm(wh)
            whf = np.where((wh[:, 2:3] < 0), -wh, wh)
            fr = _fr_dielectric((wi * whf).sum(1), 1.0, ETA)
            v = fr * _tr_d(a, wh) / (1 + _tr_lambda(a, wo) + _tr_lambda(a, wi)) / (4 * ci * co)
            return np.where(bad[:, None], 0.0, l["c"][None, :] * v[:, None])
        co, ci = wo[:, 2], wi[:, 2]              # MicrofacetTransmission::f (1, 1.5, Radiance)
        eta = np.where(co > 0, ETA, 1.0 / ETA)
        wh = _norm(wo + wi * eta[:, None])
        wh = np.where(wh[:, 2:3] < 0, -wh, wh)
        ow, iw = (wo * wh).sum(1), (wi * wh).sum(1)
        bad = _same_hemisphere(wo, wi) | (co == 0) | (ci == 0) | (ow * iw > 0)
        fr = _fr_dielectric(ow, 1.0, ETA)
        sd = ow + eta * iw
        g = 1.0 / (1 + _tr_lambda(a, wo) + _tr_lambda(a, wi))
        v = (1 - fr) * np.abs(_tr_d(a, wh) * g * eta * eta * np.abs(iw) * np.abs(ow) / (eta * eta) / (ci * co * sd * sd))
        return np.where(bad[:, None], 0.0, l["c"][None, :] * v[:, None])


def lobe_pdf(l, wo, wi):
    if l["kind"] == "lambert_r":
        return lambert_r_pdf(wo, wi)
    if l["kind"] == "lambert_t":
        return lambert_t_pdf(wo, wi)
    a = l["alpha"]
    with np.errstate(divide="ignore", invalid="ignore"):
        if l["kind"] == "mf_r":
            wh = _norm(wo + wi)
            ow = (wo * wh).sum(1)
            return np.where(_same_hemisphere(wo, wi) & ~(ow < 0), _tr_pdf(a, wo, wh) / (4 * ow), 0.0)
        eta = np.where(wo[:, 2] > 0, ETA, 1.0 / ETA)
        wh = _norm(wo + wi * eta[:, None])
        ow, iw = (wo * wh).sum(1), (wi * wh).sum(1)
        sd = ow + eta * iw
        return np.where(~_same_hemisphere(wo, wi) & ~(ow * iw > 0), _tr_pdf(a, wo, wh) * np.abs(eta * eta * iw / (sd * sd)), 0.0)


# ---- BSDF over the lobe list (bsdf.rs), canonical frame: local == world, ng = +z
def _matches(l, flags):
    return (l["type"] & flags) == l["type"]


def bsdf_f(ls, wo, wi, flags=ALL):
    wo, wi = np.asarray(wo, np.float64), np.asarray(wi, np.float64)
    out = np.zeros((len(wo), 3))
    if not ls:
        return out
    reflect = wi[:, 2] * wo[:, 2] > 0
    for l in ls:
        if not _matches(l, flags):
            continue
        use = reflect if (l["type"] & REFL) else ~reflect
        out += np.where(use[:, None], lobe_f(l, wo, wi), 0.0)
    out[wo[:, 2] == 0] = 0.0
    return out


def bsdf_pdf(ls, wo, wi, flags=ALL):
    wo, wi = np.asarray(wo, np.float64), np.asarray(wi, np.float64)
    m = [l for l in (ls or []) if _matches(l, flags)]
    if not m:
        return np.zeros(len(wo))
    p = sum(lobe_pdf(l, wo, wi) for l in m) / len(m)
    return np.where(wo[:, 2] == 0, 0.0, p)


def concentric_sample_disk(u):
    u = np.asarray(u, np.float64)
    ox, oy = 2 * u[:, 0] - 1, 2 * u[:, 1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.abs(ox) > np.abs(oy)
        r = np.where(first, ox, oy)
        th = np.where(first, np.pi / 4 * (oy / ox), np.pi / 2 - np.pi / 4 * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    return np.where(zero, 0.0, r * np.cos(th)), np.where(zero, 0.0, r * np.sin(th))


def bsdf_sample_f(ls, wo, u, flags=ALL):
    """BSDF::sample_f: (f, wi, pdf, type); type 0 = None.  Only for lists whose matching lobes are Lambertian (see the module text)."""
    wo, u = np.asarray(wo, np.float64), np.asarray(u, np.float64)
    n = len(wo)
    f, wi, pdf, typ = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.uint32)
    m = [l for l in (ls or []) if _matches(l, flags)]
    if not m:
        return f, wi, pdf, typ
    if any(l["kind"] not in ("lambert_r", "lambert_t") for l in m):
        raise NotImplementedError("sampling a glossy lobe is not restated")
    comp = np.minimum(np.floor(u[:, 0] * len(m)).astype(int), len(m) - 1)
    one_minus_eps = float(np.nextafter(f32(1), f32(0)))
    ur = np.stack([np.minimum(u[:, 0] * len(m) - comp, one_minus_eps), u[:, 1]], 1)
    x, y = concentric_sample_disk(ur)
    z = np.sqrt(np.maximum(0.0, 1 - x * x - y * y))
    for k, l in enumerate(m):
        sel = comp == k
        trans = l["kind"] == "lambert_t"
        flip = (wo[:, 2] > 0) if trans else (wo[:, 2] < 0)          # lambertian.rs:68-71 / BxDF::sample_f_default
        w = np.stack([x, y, np.where(flip, -z, z)], 1)
        p = lobe_pdf(l, wo, w)
        ok = sel & (p > 0) & (wo[:, 2] != 0)
        for j, o in enumerate(m):
            if j != k:
                p = p + lobe_pdf(o, wo, w)
        p = p / len(m)
        wi[ok], pdf[ok], typ[ok] = w[ok], p[ok], l["type"]
        f[ok] = bsdf_f(ls, wo, w, flags)[ok]
    return f, wi, pdf, typ


# ---- the diffuse-only material in float32, operation for operation (pt_bsdf_eval / pt_bsdf_sample of the device are held to these bits)
def diffuse_f32_lobes(Kd, reflect, transmit):
    """(type, colour) per lobe: clamp_zero, then r * kd / t * kd in float32."""
    kd = np.maximum(np.asarray(Kd, f32), f32(0)); r = np.maximum(np.asarray(reflect, f32), f32(0)); t = np.maximum(np.asarray(transmit, f32), f32(0))
    out = []
    if np.any(r != 0):
        out.append((REFL | DIFFUSE, (r * kd).astype(f32)))
    if np.any(t != 0):
        out.append((TRANS | DIFFUSE, (t * kd).astype(f32)))
    return out


def diffuse_f32_eval(ls, wo, wi, flags=ALL):
    """BSDF::f and BSDF::pdf in float32: f = 0 + c * INV_PI over the lobes on the side the geometric normal selects; pdf = the sum (from 0) of
    the matching lobes' pdfs divided by their count."""
    wo, wi = np.asarray(wo, f32), np.asarray(wi, f32)
    n = len(wo)
    f = np.zeros((n, 3), f32); p = np.zeros(n, f32)
    reflect = wi[:, 2] * wo[:, 2] > 0
    same = reflect                               # same_hemisphere is the same product on the canonical frame
    count = 0
    for typ, c in ls:
        if (typ & flags) != typ:
            continue
        count += 1
        val = (c * INV_PI32).astype(f32)
        use = reflect if (typ & REFL) else ~reflect
        f = np.where(use[:, None], (f + val[None, :]).astype(f32), f)
        if typ & REFL:
            lp = np.where(same, (np.abs(wi[:, 2]) * INV_PI32).astype(f32), f32(0))
        else:
            lp = np.where(~same, np.abs(wi[:, 2]), f32(0))
        p = (p + lp).astype(f32)
    if count:
        p = (p / f32(count)).astype(f32)
    bad = (wo[:, 2] == 0) | ~np.isfinite(wo).all(axis=1)
    f[bad] = 0; p[bad] = 0
    return f, p
