"""The BSDF layer held to the float64 truth of tests/bsdf_ref.py, without a GPU: the restatement's own float32 run (the calibration) and
the oracle's orc_bsdf_eval / orc_bsdf_sample, per material setting and flag set -- eval within bound, sampled type and None decisions,
sampled wi within bound, the returned f and pdf at the returned wi (c), left-out shares under 3 %, medians within 4 x the float32
restatement's.  And the truth itself is held to things that are not its own: quadratures of D and D G1, pdfs that integrate to one (and
Q19's that does not), reciprocity, and the closed forms of the Fresnel terms.

The oracle does not know Material "translucent" (DESIGN.md section 7): those settings are held by the float32 run here and by the device
in test_gpu_bsdf_truth.py.  BSDF_TRUTH_WRITE=1 prints the lines of profiles/bsdf_truth.txt."""
import os

import numpy as np
import pytest

import bsdf_cases as C
import bsdf_ref as R

ORACLE_SETTINGS = [(c, s) for c, s in C.SETTINGS if c != "translucent"]


def report(label, case, setting, stats):
    if os.environ.get("BSDF_TRUTH_WRITE"):
        print("\n" + C.summary(label, case, setting, stats))


@pytest.fixture(scope="module")
def orc_scene(oracle):
    sd = C.scene()
    sc = oracle.scene(sd)
    yield sd, sc
    sc.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the truth is met
@pytest.mark.parametrize("case,setting", C.SETTINGS, ids=["%s-%s" % cs for cs in C.SETTINGS])
def test_float32_restatement_meets_the_truth(case, setting):
    """The restatement run in float32 lies within the bounds its float64 run derives, and leaves out at most 3 % of any flag set."""
    stats = list(C.calibration(case, setting).values())
    report("f32", case, setting, stats)
    for s in stats:
        assert s.left <= C.MAX_LEFT_OUT, (s.what, s.left)
    assert sum(s.n for s in stats if " all eval f" in s.what) > 0.97 * C.N_BULK


@pytest.mark.parametrize("case,setting", ORACLE_SETTINGS, ids=["%s-%s" % cs for cs in ORACLE_SETTINGS])
def test_oracle_meets_the_truth(orc_scene, case, setting):
    sd, sc = orc_scene
    mat = sd.material_index[(case, setting)]
    stats = C.run_setting(case, setting, lambda wo, wi, fl: sc.bsdf_eval(mat, wo, wi, fl), lambda wo, u, fl: sc.bsdf_sample(mat, wo, u, fl), "orc")
    report("orc", case, setting, stats)
    C.hold_caps_and_medians(stats, case, setting, "orc")


@pytest.mark.parametrize("setting", list(C.FLOOR_CASES))
def test_alpha_floor_is_held_through_the_sampling_check(orc_scene, setting):
    """alpha = 0.001 (the floor of TrowbridgeReitzDistribution::new) and grazing wo: no f bound is asked of these, but whatever sample_f
    returns is f and pdf at the direction it returns."""
    sd, sc = orc_scene
    mat = sd.material_index[("floor", setting)]
    b = C.truth("floor", setting)
    assert all(abs(float(l.dist.ax.v) - R.c32(0.001)) < 1e-9 for l in b.lobes if l.dist is not None)
    report("f32", "floor", setting, list(C.calibration("floor", setting).values()))
    stats = C.run_floor(setting, lambda wo, u, fl: sc.bsdf_sample(mat, wo, u, fl), "orc")
    report("orc", "floor", setting, stats)
    C.hold_caps_and_medians(stats, "floor", setting, "orc", capped=False)
    assert sum(s.n for s in stats if "(c) f" in s.what) > 1000


def test_lobe_lists_follow_the_materials():
    """Which lobes exist, in what order, with what colour: the clamps, uber's opacity * clamp(K), the uroughness -> roughness fallback,
    the 0.001 floor, translucent's constant 1.5."""
    def kinds(c, s): return [l.kind for l in C.truth(c, s).lobes]
    assert kinds("uber", "five") == ["spec_t", "lambert", "mf_r", "spec_r", "spec_t"]
    assert kinds("uber", "opaque") == ["lambert", "mf_r", "spec_r"]
    assert kinds("translucent", "four") == ["lambert", "lambert_t", "mf_r", "mf_t"]
    assert kinds("rough_glass", "kr_only") == ["mf_r"] and kinds("rough_glass", "kt_only") == ["mf_t"]
    five = C.truth("uber", "five").lobes
    assert [float(c.v) for c in five[0].r] == [float(np.float32(1) - np.float32(0.6)), 0.0, float(np.float32(1) - np.float32(0.8))]   # clamp(1 - opacity)
    assert float(five[3].r[2].v) == 0.0 and abs(float(five[3].r[1].v) - 1.2 * 0.15) < 1e-7                 # opacity * clamp(Kr), opacity unclamped
    fb = C.truth("metal", "fallback").lobes[0].dist
    assert abs(float(fb.ax.v) - 0.05) < 1e-8 and abs(float(fb.ay.v) - 0.3) < 1e-7                             # vroughness falls back to roughness
    assert float(C.truth("translucent", "glossy_t").lobes[0].eta_b.v) == 1.5
    assert C.truth("matte", "oren_90").lobes[0].kind == "oren"
    s90 = np.radians(90.0) ** 2
    assert abs(float(C.truth("matte", "oren_90").lobes[0].b.v) - 0.45 * s90 / (s90 + 0.09)) < 1e-6          # sigma clamped to 90


# ------------------------------------------------------------------------------------------------------------------ 5. the truth is held
def sphere_grid(nt, nph, lo=0.0, hi=np.pi):
    """Midpoint rule on [lo, hi] x [0, 2 pi): directions (n, 3) and their solid-angle weights."""
    th = lo + (np.arange(nt) + 0.5) * ((hi - lo) / nt)
    ph = (np.arange(nph) + 0.5) * (2 * np.pi / nph)
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    return d, (np.sin(T) * ((hi - lo) / nt) * (2 * np.pi / nph)).reshape(-1)


def exact(a):
    a = np.atleast_2d(np.asarray(a, np.float64))
    return [R.E(a[:, i].copy()) for i in range(3)]


def dist(ax, ay):
    return R.TR(R.E(np.asarray(ax)), R.E(np.asarray(ay)))


def theta_grid(alpha, nt, nph):
    """D is a peak of width alpha at the pole: the polar angle is stepped uniformly in tan(theta) / alpha = sinh(t)."""
    t = (np.arange(nt) + 0.5) * (np.arcsinh(1e4 / alpha) / nt)
    th = np.arctan(alpha * np.sinh(t))
    dth = alpha * np.cosh(t) / (1 + (alpha * np.sinh(t)) ** 2) * (np.arcsinh(1e4 / alpha) / nt)
    ph = (np.arange(nph) + 0.5) * (2 * np.pi / nph)
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    w = (np.sin(T) * dth[:, None] * (2 * np.pi / nph)).reshape(-1)
    return d, w


@pytest.mark.parametrize("ax,ay", [(0.3, 0.3), (0.05, 0.4), (0.4, 0.05), (0.02, 0.02)])
def test_d_is_normalised_and_g1_is_the_visible_share(ax, ay):
    """The integral of D(wh) cos(theta_h) over the hemisphere is 1, and of D G1(wo) max(0, wo . wh) is cos(theta_o): what makes D a
    distribution of normals and G1 its masking term, whichever way round ax and ay are."""
    d, w = theta_grid(min(ax, ay), 1500, 720)
    tr = dist(ax, ay)
    und = np.zeros(len(d), bool)
    D = tr.d(exact(d), und).v
    assert abs((D * d[:, 2] * w).sum() - 1.0) < 2e-3
    for wo in ([0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.3, 0.7, np.sqrt(1 - 0.58)], [0.0, 0.95, np.sqrt(1 - 0.9025)]):
        g1 = float(tr.g1(exact(wo), np.zeros(1, bool)).v[0])
        vis = (D * g1 * np.maximum(0.0, d @ np.array(wo)) * w).sum()
        assert abs(vis - wo[2]) < 3e-3 * wo[2], (wo, vis)


REFLECTING = [("matte", "oren_25"), ("plastic", "noremap"), ("metal", "aniso_uv"), ("substrate", "aniso"), ("rough_glass", "kr_only"),
              ("translucent", "lambert_r")]


def visible_share(tr, wo):
    """The share of the visible normals of wo whose mirror image of wo stays on wo's side: the integral of D G1 max(0, wo . wh) /
    cos(theta_o) over those wh, in plain numpy on the half-vector grid -- the reflection pdf's integral over wi after the change of
    variables d(wi) = 4 (wo . wh) d(wh), stated without pdf() or the sampler."""
    wo = np.array(wo, np.float64)
    wo = -wo if wo[2] < 0 else wo                                      # D is even and G1 reads |tan|: the lower side mirrors the upper
    d, w = theta_grid(min(float(tr.ax.v), float(tr.ay.v)), 800, 360)
    D = tr.d(exact(d), np.zeros(len(d), bool)).v
    g1 = float(tr.g1(exact(wo), np.zeros(1, bool)).v[0])
    c = d @ wo
    wi = 2.0 * c[:, None] * d - wo
    return (D * g1 * c * ((c > 0) & (wi[:, 2] > 0)) * w).sum() / wo[2]


def expected_pdf_integral(b, wo):
    """BSDF::pdf over the sphere from outside the restatement's pdf and sampler: the mean over the lobes of 1 (cosine-weighted), the
    visible share (MicrofacetReflection), and their mean (FresnelBlend draws either with probability one half)."""
    per = {"lambert": lambda l: 1.0, "oren": lambda l: 1.0, "mf_r": lambda l: visible_share(l.dist, wo),
           "blend": lambda l: 0.5 * (1.0 + visible_share(l.dist, wo))}
    return float(np.mean([per[l.kind](l) for l in b.lobes]))


@pytest.mark.parametrize("case,setting", REFLECTING)
def test_reflection_pdfs_integrate_to_the_share_the_sampler_returns(case, setting):
    """BSDF::pdf over the sphere is 1 for the diffuse lobes.  A microfacet lobe's sample_f returns None where the reflected direction
    leaves the hemisphere and its pdf is 0 there, so its pdf integrates to the share of samples that sample_f returns -- two parts of
    the restatement written apart, the density and the sampler, held to each other by quadrature (5e-3) and a count (4 sigma) -- and
    to the visible-normal integral over the half vectors whose reflection stays on wo's side, which uses neither."""
    b = C.truth(case, setting)
    d, w = sphere_grid(500, 600)
    rng = np.random.default_rng(17)
    n = 20000
    u = rng.random((n, 2)).astype(np.float32)
    for wo in ([0.0, 0.0, 1.0], [0.5, -0.3, np.sqrt(1 - 0.34)], [-0.6, 0.6, -np.sqrt(1 - 0.72)]):
        wo = [float(np.float32(c)) for c in wo]
        wov = [R.E(np.full(len(d), c)) for c in wo]
        _, _, t = b.terms(wov, exact(d))
        total = (b.combine(wov, exact(d), t, R.ALL).pdf * w).sum()
        s = b.sample(np.tile(np.array(wo, np.float32), (n, 1)), u)
        share = (s["type"] != 0).mean()
        if all(l.kind in ("lambert", "oren") for l in b.lobes):
            assert share == 1.0
        assert abs(total - share) < 5e-3 + 4 * np.sqrt(share * (1 - share) / n), (wo, total, share)
        assert total <= 1.0 + 5e-3
        want = expected_pdf_integral(b, wo)                            # and to a statement that uses neither: two quadratures, 5e-3 each
        assert abs(total - want) < 1e-2, (wo, total, want)


def test_transmission_pdfs_are_not_densities_as_documented():
    """Q19: MicrofacetTransmission::pdf has no wo . wh < 0 guard and integrates to more than one away from the normal; Q53:
    LambertianTransmission::pdf has no INV_PI and integrates to pi."""
    d, w = sphere_grid(600, 600)
    b = R.BSDF(dict(type="glass", Kr=(0.0, 0.0, 0.0), Kt=(0.8, 0.9, 0.8), eta=1.33, uroughness=0.1, vroughness=0.2))
    tot = []
    for deg in (0.0, 54.0):
        wo = (np.sin(np.radians(deg)), 0.0, np.cos(np.radians(deg)))
        wov = [R.E(np.full(len(d), c)) for c in wo]
        _, _, t = b.terms(wov, exact(d))
        tot.append((b.combine(wov, exact(d), t, R.ALL).pdf * w).sum())
    print("MicrofacetTransmission::pdf over the sphere at 0 and 54 degrees:", tot)
    assert tot[0] <= 1.0 + 5e-3 and tot[1] > 1.02, tot
    b = C.truth("translucent", "lambert_t")
    wov = [R.E(np.full(len(d), c)) for c in (0.0, 0.6, 0.8)]
    _, _, t = b.terms(wov, exact(d))
    assert abs((b.combine(wov, exact(d), t, R.ALL).pdf * w).sum() - np.pi) < 1e-3


@pytest.mark.parametrize("case,setting", [("matte", "lambert"), ("matte", "oren_25"), ("metal", "aniso_vu"), ("substrate", "aniso"),
                                          ("plastic", "remap"), ("uber", "opaque")])
def test_reflection_lobes_are_reciprocal(case, setting):
    """f(wo, wi) = f(wi, wo) for the reflection lobes whose formula in the reference is symmetric: Lambert, Oren-Nayar, the microfacet
    reflection with a conductor (|cos| enters the Fresnel term) or a dielectric entered from outside, FresnelBlend."""
    b = C.truth(case, setting)
    rng = np.random.default_rng(3)
    a, c = C.sphere_dirs(rng, 4000), C.sphere_dirs(rng, 4000)
    a[:, 2], c[:, 2] = np.abs(a[:, 2]), np.abs(c[:, 2])                # the upper side: plastic's Fresnel(1.5, 1.0) is entered from above
    f1, e1 = b.f(a, c, R.NOSPEC)
    f2, e2 = b.f(c, a, R.NOSPEC)
    ok = np.isfinite(e1).all(1) & np.isfinite(e2).all(1)
    assert ok.mean() > 0.99 and (np.abs(f1 - f2)[ok] <= (e1 + e2)[ok] + 1e-12 * np.abs(f1[ok])).all()


def test_fresnel_closed_forms():
    """The dielectric is ((eta - 1) / (eta + 1))^2 at normal incidence and has rparl = 0 at Brewster's angle (where it is rperp^2 / 2
    with rperp = cos(2 theta_B)); the conductor with k = 0 is the dielectric."""
    one = R.E(np.asarray(1.0))
    for eta in (1.33, 1.5, 2.4):
        et = R.E(np.asarray(eta))
        r0 = float(R.fr_dielectric(R.E(np.array([1.0])), one, et, np.zeros(1, bool)).v[0])
        assert abs(r0 - ((eta - 1) / (eta + 1)) ** 2) < 1e-14
        r0 = float(R.fr_dielectric(R.E(np.array([-1.0])), one, et, np.zeros(1, bool)).v[0])          # from inside: the same
        assert abs(r0 - ((eta - 1) / (eta + 1)) ** 2) < 1e-14
        tb = np.arctan(eta)
        rb = float(R.fr_dielectric(R.E(np.array([np.cos(tb)])), one, et, np.zeros(1, bool)).v[0])
        assert abs(rb - 0.5 * np.cos(2 * tb) ** 2) < 1e-14
        cs = R.E(np.linspace(0.02, 1.0, 50))
        d = R.fr_dielectric(cs, one, et, np.zeros(50, bool)).v
        c = R.fr_conductor(cs, [one] * 3, [et] * 3, [R.E(np.asarray(0.0))] * 3)[0].v
        assert np.abs(d - c).max() < 1e-13
    crit = R.fr_dielectric(R.E(np.array([-0.5])), one, R.E(np.asarray(1.5)), np.zeros(1, bool)).v[0]    # past the critical angle from inside
    assert crit == 1.0
