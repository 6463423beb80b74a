"""The cases of the Material "fourier" truths (tests/fourier_ref.py): the four tables, the drawn and the directed inputs, and the
comparison of an implementation's pt_bsdf_eval / pt_bsdf_sample outputs against the float64 truth.  Shared by test_fourier_host.py (the
float32 run of the restatement, no GPU) and test_gpu_fourier.py (the device).

About 2 000 direction pairs and samples per table: N_BULK pairs drawn on the sphere (both hemispheres, |cos| >= bsdf_cases.COS_MIN), then
the directed ones -- wo at every node of the table, wi at every node (mu_i = -wi.z), wo and wi along the normal (z = +-1 exactly),
mu_i == 0 (wi in the plane), wo.z == 0 (BSDF::f's own zero), near-normal wo.  Undecided evaluations count under bsdf_cases.MAX_LEFT_OUT; an evaluation whose
bound is a large share of its value is held to that bound, not left out (fourier_ref.Eval.left_out).  Sampling is held by inversion (fourier_ref.BSDF.inversion): a sample whose returned direction does not determine it --
wo along the normal, where sample_f's norm is 0 and wi comes back as +-z whatever mu_i was drawn -- is left out of the inversion and of
the pdf check and counts in the share.
"""
import functools
import os

import numpy as np

import bsdf_cases as C
import bsdf_ref as R
import fourier_ref as FR
import fourier_tables as FT
from aov_ref import E, U
from helpers import pkg, scenes

capi = pkg.capi
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUGHGOLD = os.path.join(GOLDEN, "roughgold_alpha_0.2.bsdf")
TABLES = ("roughgold", "two_sided", "rgb_long", "dark")
N_BULK = 1600
FLAG_SETS = C.FLAG_SETS

# tests/fourierbsdf.rs of the reference, as values: wo = normalize(-0.5, -0.5, 0.8), wi = normalize(0.4, 0.52, 0.7), u = (0.1, 0.8);
# f(wo, wi).y, pdf(wo, wi), pdf(wi, wo), then sample_f(wo, u): f.y, pdf, wi.  Its tolerance is 1e-3 relative.
RECORDED = dict(wo=(-0.5, -0.5, 0.8), wi=(0.4, 0.52, 0.7), u=(0.1, 0.8), f_y=2.679294, pdf=2.438230, pdf_swapped=2.503326,
                sample_f_y=2.596391, sample_pdf=1.855472, sample_wi=(0.539052, 0.617347, 0.572980))
RECORDED_REL = 1e-3


def luminance(f):
    f = np.asarray(f, np.float64)
    return 0.212671 * f[..., 0] + 0.715160 * f[..., 1] + 0.072169 * f[..., 2]


def normalize32(v):
    """Vector3f::normalize in float32."""
    v = np.asarray(v, np.float32)
    l = np.sqrt((v * v).sum(dtype=np.float32), dtype=np.float32)
    return (v / l).astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(name):
    """The table as a capi.FourierTable: the fixture through an independent numpy parse, the synthetic ones from their generator."""
    if name == "roughgold":
        d = FR.parse_file(ROUGHGOLD)
        return capi.FourierTable(d["mu"], d["cdf"], d["offset_and_length"], d["a"], d["n_channels"], d["m_max"], d["eta"])
    return getattr(FT, name)()


@functools.lru_cache(maxsize=None)
def truth(name):
    return FR.BSDF(table(name), np.float64)


def palette():
    """One small triangle per table: the scene only carries the material table for the BSDF hooks."""
    sb = scenes.SceneBuilder()
    sb.look_at((0, -4, 3), (0, 0, 0), (0, 0, 1))
    sb.camera_perspective(fov=50.0)
    sb.film(xresolution=8, yresolution=8)
    sb.pixel_filter_box()
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path(maxdepth=1)
    index = {}
    for k, name in enumerate(TABLES):
        sb.material_fourier(table=table(name))
        index[name] = sb.cur_material
        x = -2.0 + 0.1 * k
        sb.shape_trianglemesh([x, 0, 0, x + 0.05, 0, 0, x, 0.05, 0], [0, 1, 2])
    sb.light_distant(L=(1, 1, 1), frm=(0, 0, 1), to=(0, 0, 0))
    sd = sb.build()
    sd.material_index = index
    return sd


def _with_z(rng, z):
    """Float32 unit vectors whose z is exactly the given float32 numbers."""
    z = np.asarray(z, np.float32)
    a = rng.uniform(0, 2 * np.pi, len(z))
    s = np.sqrt(np.maximum(0.0, 1.0 - z.astype(np.float64) ** 2))
    return np.stack([(s * np.cos(a)).astype(np.float32), (s * np.sin(a)).astype(np.float32), z], 1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(wo, wi, u): N_BULK drawn pairs, then the directed blocks of the module's docstring."""
    rng = np.random.default_rng(sum(ord(c) for c in "fourier/" + name))
    mu = np.asarray(table(name).mu, np.float32)
    nodes = np.resize(mu[np.abs(mu) < 1], 96)                             # every node but the poles (their own block, below), each at least once
    wo, wi = [C.sphere_dirs(rng, N_BULK)], [C.sphere_dirs(rng, N_BULK)]

    def block(o, i):
        wo.append(np.asarray(o, np.float32)); wi.append(np.asarray(i, np.float32))
    block(_with_z(rng, nodes), C.sphere_dirs(rng, 96))                    # wo at the nodes
    block(C.sphere_dirs(rng, 96), -_with_z(rng, nodes))                   # mu_i = -wi.z at the nodes
    block(_with_z(rng, nodes[:48]), -_with_z(rng, np.roll(nodes, 7)[:48]))        # both
    pole = np.tile(np.array([[0, 0, 1], [0, 0, -1]], np.float32), (10, 1))
    block(pole, C.sphere_dirs(rng, 20))                                   # wo along the normal
    block(C.sphere_dirs(rng, 20), pole)                                   # wi along the normal
    block(C.sphere_dirs(rng, 24), _with_z(rng, np.zeros(24)))             # mu_i == 0
    block(_with_z(rng, np.zeros(12)), C.sphere_dirs(rng, 12))             # wo.z == 0
    near = C.sphere_dirs(rng, 20)                                         # near-normal wo: sin(theta_o) between 3e-3 and 1.5e-2
    r = 10.0 ** rng.uniform(np.log10(3e-3), np.log10(1.5e-2), 20)
    near[:, :2] *= (r / np.linalg.norm(near[:, :2].astype(np.float64), axis=1))[:, None].astype(np.float32)
    near[:, 2] = np.sign(near[:, 2])
    near /= np.linalg.norm(near.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    block(near, C.sphere_dirs(rng, 20))
    wo, wi = np.concatenate(wo), np.concatenate(wi)
    u = rng.random((len(wo), 2)).astype(np.float32)
    u[N_BULK:N_BULK + 8, 0] = 0.0
    u[N_BULK + 8:N_BULK + 16, 1] = 0.0
    u[N_BULK + 16:N_BULK + 24, 0] = np.float32(0.99999994)
    u[N_BULK + 24:N_BULK + 32, 1] = np.float32(0.99999994)
    u[N_BULK + 32:N_BULK + 40, 0] = 0.5
    return wo, wi, u


@functools.lru_cache(maxsize=None)
def truth_eval(name, flags):
    wo, wi, _ = inputs(name)
    return truth(name).eval(wo, wi, flags)


@functools.lru_cache(maxsize=None)
def truth_sample(name, flags):
    wo, _, u = inputs(name)
    return truth(name).sample(wo, u, flags)


def check_sample(tag, name, flags, got):
    """An implementation's (f, wi, pdf, type) for inputs(name) against the float64 truth: the None decisions, the two inversions, f and
    pdf at the returned direction.  A list of bsdf_cases.Stat."""
    b = truth(name)
    wo, _, u = inputs(name)
    f, wi, pdf, typ = [np.asarray(a) for a in got]
    s = truth_sample(name, flags)
    N = len(wo)
    # (a) None decisions.  Undecided: the row's energy `maximum` within its float32 bound of zero, or the truth's own pdf within the
    # bound of its evaluation of zero (both are signs a float32 run may read differently).
    und = (s["maximum"] != 0) & (np.abs(s["maximum"]) <= 8.0 * U * s["max_abs"])
    some_t = s["type"] != 0
    if some_t.any():
        at_t = b.eval(wo[some_t], s["wi"][some_t].astype(np.float32), flags)
        und[np.flatnonzero(some_t)] |= at_t.und | (at_t.pdf <= 2.0 * at_t.pdf_e)
    bad = ~und & (typ != s["type"])
    assert not bad.any(), (tag, "type / None", int(bad.sum()), np.flatnonzero(bad)[:8], typ[bad][:4], s["type"][bad][:4])
    stats = []
    ret = (typ != 0) & ~und
    if not ret.any():
        return [C.Stat(tag + " sample none", und.mean(), np.zeros(0), 0)]
    idx = np.flatnonzero(ret)
    inv = b.inversion(wo[idx], u[idx], wi[idx])
    ok = inv["ok"]
    with np.errstate(all="ignore"):
        r_mu = (inv["mu_res"] / inv["mu_tol"])[ok]
        r_phi = (inv["phi_res"] / inv["phi_tol"])[ok]
    assert (r_mu <= 1.0).all(), (tag, "cdf(mu_i) - u[1] over its bound", float(r_mu.max()), int((r_mu > 1).sum()))
    assert (r_phi <= 1.0).all(), (tag, "cdf(phi) - u[0] over its bound", float(r_phi.max()), int((r_phi > 1).sum()))
    left_inv = (und.sum() + (~ok).sum()) / N
    stats += [C.Stat(tag + " sample mu", left_inv, r_mu, int(ok.sum())), C.Stat(tag + " sample phi", left_inv, r_phi, int(ok.sum()))]
    # (c) f at the returned wi (the BSDF evaluates it there again); pdf at the sample the returned wi determines: mu_i recovered as in
    # inversion(), 10 roundings of it and 18 of the angle turned into pdf by the slopes (a difference in float64, sum k |a_k| / rho)
    at = b.eval(wo[idx], wi[idx], flags)
    good = ~at.und & np.isfinite(at.f_e).all(1) & np.isfinite(at.f).all(1)
    rcf = C.hold(tag + " (c) f", f[idx].astype(np.float64), at.f, at.f_e, good)
    mwi = -wi[idx]
    cphi = FR.cos_d_phi(mwi, wo[idx], np.float64)
    mu_o = E(wo[idx][:, 2].astype(np.float64))
    h = 10.0 * U * np.maximum(np.abs(inv["mu_i"]), 2.0 ** -20)
    p0 = b.eval_core(E(inv["mu_i"]), mu_o, cphi, flags, with_f=False)
    p1 = b.eval_core(E(np.clip(inv["mu_i"] + h, float(b.T.mu[0]), float(b.T.mu[-1]))), mu_o, cphi, flags, with_f=False)
    p2 = b.eval_core(E(np.clip(inv["mu_i"] - h, float(b.T.mu[0]), float(b.T.mu[-1]))), mu_o, cphi, flags, with_f=False)
    pe = p0.pdf_e + np.maximum(np.abs(p1.pdf - p0.pdf), np.abs(p2.pdf - p0.pdf)) + 18.0 * U * p0.pdf_slope_phi
    goodp = ok & ~p0.und & np.isfinite(pe) & np.isfinite(p0.pdf)
    rcp = C.hold(tag + " (c) pdf", pdf[idx].astype(np.float64), p0.pdf, pe, goodp)
    stats += [C.Stat(tag + " sample (c) f", (und.sum() + (~good).sum()) / N, rcf, int(good.sum())),
              C.Stat(tag + " sample (c) pdf", (und.sum() + (~goodp).sum()) / N, rcp, int(goodp.sum()))]
    return stats


def run_table(name, impl_eval, impl_sample, label):
    """Every check for one table and every flag set: a list of Stat.  impl_eval(wo, wi, flags) -> (f, pdf); impl_sample(wo, u, flags) ->
    (f, wi, pdf, type)."""
    wo, wi, u = inputs(name)
    stats = []
    for fname, flags in FLAG_SETS:
        tag = "%s fourier/%s %s" % (label, name, fname)
        f, pdf = impl_eval(wo, wi, flags)
        stats += C.check_eval(tag, truth_eval(name, flags), f, pdf)
        stats += check_sample(tag, name, flags, impl_sample(wo, u, flags))
    return stats


@functools.lru_cache(maxsize=None)
def calibration(name):
    """The float32 restatement's own Stats, by `what` without the label: the medians the device is held to bsdf_cases.MEDIAN_FACTOR of."""
    r = FR.Restatement32(table(name))
    return {s.what[4:]: s for s in run_table(name, r.eval, r.sample, "f32")}


def hold_caps_and_medians(stats, name, label):
    cal = calibration(name)
    for s in stats:
        print(s)
        assert s.left <= C.MAX_LEFT_OUT, (s.what, "left out", s.left)
        ref = cal[s.what[len(label) + 1:]]
        assert s.median <= C.MEDIAN_FACTOR * ref.median, (s.what, "median err / bound", s.median, "float32 restatement", ref.median)


def summary(label, name, stats):
    """One line of profiles/fourier_truth.txt: per quantity the worst and the largest median err / bound over the flag sets, and the
    largest share left out."""
    def agg(key):
        sel = [s for s in stats if s.what.endswith(key) and s.n]
        return "%s worst %.3f median %.4f" % (key, max(s.worst for s in sel), max(s.median for s in sel)) if sel else "%s -" % key
    keys = ["eval f", "eval pdf", "sample mu", "sample phi", "sample (c) f", "sample (c) pdf"]
    return "%-3s %-10s left out %.4f | %s" % (label, name, max(s.left for s in stats), " | ".join(agg(k) for k in keys))


@functools.lru_cache(maxsize=None)
def iteration_maxima():
    """The most iterations the float32 restatement's two inversion loops take over every sampling input of the four tables: what the
    device's caps (pt_fourier.h) are at least four times of."""
    mu = phi = 0
    for name in TABLES:
        wo, _, u = inputs(name)
        s = FR.BSDF(table(name), np.float32).sample(wo, u, R.ALL)
        mu, phi = max(mu, int(s["it_mu"].max())), max(phi, int(s["it_phi"].max()))
    return mu, phi


# ---- one estimate_direct (core/integrator/sample_lights.rs:330-455) at a Fourier surface in the plane z = 0 under ONE triangle light
# (a single light: the selection pdf is 1 whatever the strategy), by quadrature in float64 over the light's area: the moments
# test_gpu_fourier.py holds the path integrator's two halves under MIS to.  f and the reported pdf sp come from fourier_ref; the lobe's
# true sampling density IS its reported pdf (pdf_mu pdf_phi = y / rho, Q-notes in fourier_ref.inversion), so the BSDF half is
# an expectation over sp.  Light half: y uniform on the triangle, lp = r^2 / (cos_l Area), contributes A = f cos L lp / (lp^2 + sp'^2);
# BSDF half: wi ~ sp, contributes B = f cos L sp' / (sp'^2 + lp^2) where wi meets the light, 0 elsewhere.  sp' = pdf_factor * sp is what
# the integrator is ASSUMED to carry into the weights and to divide by: 1 for the reported pdf, another factor for "some other pdf".
MIS_FOV = 20.0
MIS_LIGHT = ((-1.5, -1.0, 3.0), (0.0, 1.5, 3.0), (1.5, -1.0, 3.0))


@functools.lru_cache(maxsize=None)
def _mis_terms(name, res, ng):
    """Per film pixel (its centre) and per point of a midpoint grid on the light: f, the reported pdf, cos, lp and the solid angle."""
    b = truth(name)
    tan_h = np.tan(np.radians(MIS_FOV / 2))
    sx = ((np.arange(res) + 0.5) / res * 2.0 - 1.0) * tan_h
    px, py = [a.reshape(-1) for a in np.meshgrid(sx, sx)]
    g = (np.arange(ng) + 0.5) / ng
    su, tu = [a.reshape(-1) for a in np.meshgrid(g, g)]
    b0, b1 = 1.0 - np.sqrt(su), tu * np.sqrt(su)                      # uniform_sample_triangle: the midpoint grid is uniform in area
    v0, v1, v2 = [np.array(v) for v in MIS_LIGHT]
    y = b0[:, None] * v0 + b1[:, None] * v1 + (1.0 - b0 - b1)[:, None] * v2
    area = 0.5 * np.linalg.norm(np.cross(v1 - v0, v2 - v0))
    P, Y = len(px), len(y)
    p = np.stack([np.repeat(px, Y), np.repeat(py, Y), np.zeros(P * Y)], 1)
    d = np.tile(y, (P, 1)) - p
    r2 = (d * d).sum(1)
    wi = d / np.sqrt(r2)[:, None]
    wo = np.array([0.0, 0.0, 1.0]) - p
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    v = b.eval(wo.astype(np.float32), wi.astype(np.float32), R.NOSPEC)
    cos_l = np.abs(wi[:, 2])
    return v.f, v.pdf, wi[:, 2], r2 / (cos_l * area), cos_l / r2 * (area / Y), P, Y


def mis_moments(name, pdf_factor=1.0, res=4, ng=24):
    """(mean, variance) per channel of one camera sample of `path` at maxdepth 1, drawn anywhere on a res x res film of MIS_FOV degrees
    that looks straight down at the plane from height 1; L = 1."""
    f, pdf, cos, lp, dw, P, Y = _mis_terms(name, res, ng)
    sp = pdf * pdf_factor
    with np.errstate(all="ignore"):
        A = f * (cos * lp / (lp * lp + sp * sp))[:, None]
        B = np.where((pdf > 0)[:, None], f * (cos * sp / (sp * sp + lp * lp))[:, None], 0.0)
    wB = (pdf * dw)[:, None]                                           # the true density times d omega
    A, B, wB = A.reshape(P, Y, 3), B.reshape(P, Y, 3), wB.reshape(P, Y, 1)
    ea, ea2 = A.mean(1), (A * A).mean(1)
    eb, eb2 = (B * wB).sum(1), (B * B * wB).sum(1)
    m = ea + eb
    var = (ea2 - ea * ea) + (eb2 - eb * eb)
    return m.mean(0), var.mean(0) + m.var(0)
