"""Area-lit next-event estimation and MIS held to the float64 truth of tests/direct_ref.py, without a GPU: the cases of
tests/direct_cases.py against the restatement's own float32 run (the calibration) and against the oracle's radiance_samples -- err <= bound
on every decided sample, exact values where the truth is decided without a bound, the 3 % cap on the union of all reasons, the kind counts
from the float64 truth alone, the oracle's median err / bound within 4 x the float32 run's.

And the truth itself is held to what is not its own: the mean of its estimate over stratified (u_light, u_scattering) against a float64
quadrature of the emitters, under MIS and under light-only weighting (the weights sum to one), and pick pdfs that sum to one.

DIRECT_TRUTH_WRITE=<file> appends the lines of profiles/direct_truth.txt to it."""
import numpy as np
import pytest

import direct_cases as DC
import direct_ref as D


@pytest.fixture(scope="module")
def runs(oracle):
    """One oracle scene per case, its inputs, its truth and the float32 run's Stat, made on first use and kept for the module."""
    made = {}

    def get(case):
        if case not in made:
            row, integ, strategy, route = case
            sd, truth_sd, extent = DC.scenes_of(case)
            # a row the oracle cannot render takes only its inputs (camera rays, sampler values) from the oracle, through a proxy scene
            osc = oracle.scene(DC.scene(row, integ, strategy, proxy=True) if row in DC.NOT_IN_THE_ORACLE else sd)
            inp = DC.Inputs(osc, osc.info, DC.nsamples_of(integ), halton=route == "halton")
            setup, tr = DC.truth_of(truth_sd, inp, integ, strategy, extent)
            f32 = setup.radiance(inp.o, inp.d, inp.u, integ[:3] if integ.startswith("all") else integ, strategy, dtype=np.float32, u_arrays=inp.u_arrays)
            made[case] = (osc, inp, tr, DC.Stat(("f32", "%s-%s-%s-%s" % case), tr, f32["value"]))
        return made[case]
    yield get
    for osc, _, _, _ in made.values():
        osc.close()


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_float32_restatement_meets_the_truth(runs, case):
    """The composition run in float32 on float32 hit points and directions lies within the bounds its float64 run derives; the cap and the
    kind counts hold before anything else is compared."""
    _, _, tr, f32 = runs(case)
    DC.report(f32)
    DC.hold(f32, case[0])


ORACLE_CASES = [c for c in DC.CASES if c[0] not in DC.NOT_IN_THE_ORACLE]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=["%s-%s-%s-%s" % c for c in ORACLE_CASES])
def test_oracle_meets_the_truth(runs, case):
    osc, inp, tr, f32 = runs(case)
    got = osc.radiance_samples(inp.bounds).reshape(-1, 3)
    stat = DC.Stat(("orc", "%s-%s-%s-%s" % case), tr, got)
    DC.report(stat)
    DC.hold(stat, case[0], calibration=f32)


def test_uniform_with_three_lights_is_spatial(runs):
    """create_light_sample_distribution.rs:23-26: the two cases share one truth."""
    a, b = runs(("matte", "path", "uniform", "plain"))[2], runs(("matte", "path", "spatial", "plain"))[2]
    assert np.array_equal(a["value"], b["value"]) and np.array_equal(a["reason"], b["reason"])
    p = runs(("matte", "path", "power", "plain"))[2]
    assert not np.array_equal(a["value"], p["value"])


# ------------------------------------------------------------------------------------------------------------------ the truth is held
# none of them has the side emitter between itself and the quad: the quadrature knows no occluder (asserted below)
POINTS = [(-0.6, -1.5), (-0.5, 0.3), (-0.3, 1.5), (0.2, -0.6), (0.7, 0.9), (1.2, -1.7), (1.7, 0.1), (1.5, 1.8)]
WO = np.array([0.1, -0.6, 0.8]) / np.linalg.norm([0.1, -0.6, 0.8])


@pytest.fixture(scope="module")
def open_setup():
    """The matte scene without its blocker."""
    sd = DC.scene("matte", blocker=False)
    P = np.asarray(sd.buffers["P"], np.float32).reshape(-1, 3)
    return D.Setup(sd, sd.direct_params, list(P.min(0)) + list(P.max(0)), DC.EXTENT)


def stratified(rng, k):
    g = (np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2) + rng.random((k * k, 2))) / k
    return np.minimum(g, 1.0 - 2.0 ** -24).astype(np.float32)


def mean_estimate(setup, mis):
    """Per point: the sum over the lights of the mean of estimate_direct over 64 x 64 stratified (u_light, u_scattering), and its standard
    error from the estimate's own sample variance."""
    rng = np.random.default_rng(23)
    k, nl, npt = 64, len(setup.lights), len(POINTS)
    n = k * k
    ul = stratified(rng, k)
    us = stratified(rng, k)[rng.permutation(n)]
    p = np.repeat(np.array([(x, y, 0.0) for x, y in POINTS]), nl * n, axis=0)
    j = np.tile(np.repeat(np.arange(nl), n), npt)
    floor_tri = 0
    est = setup.estimate(np.full(len(p), floor_tri), p, np.tile(WO, (len(p), 1)), j, np.tile(ul, (npt * nl, 1)), np.tile(us, (npt * nl, 1)),
                         mis=mis, bsdf_half=mis, spread=False)
    v = np.stack([est["A"][c].v + est["B"][c].v for c in range(3)], 1).reshape(npt, nl, n, 3)
    return v.mean(2).sum(1), np.sqrt((v.var(2, ddof=1) / n).sum(1)), est


def test_mis_estimate_integrates_to_the_emitters_quadrature(open_setup):
    """(i) and (ii): at 8 floor points the mean of the MIS estimate equals the float64 quadrature of Kd / pi L cos cos' / r^2 over the three
    emitters within three standard errors; so does the light-only estimate (w = 1, no BSDF half); and the two agree within the same
    margin: the weights of the two halves sum to one."""
    kd = np.clip(DC.M["matte"]["Kd"], 0.0, None)
    want = D.emitter_quadrature(open_setup, np.array([(x, y, 0.0) for x, y in POINTS]), np.array([0.0, 0.0, 1.0]), kd)
    assert np.abs(D.emitter_quadrature(open_setup, np.array([(0.2, -0.6, 0.0)]), np.array([0.0, 0.0, 1.0]), kd, k=128) - want[3]).max() < 1e-5 * want[3].max()
    mis, se_mis, est = mean_estimate(open_setup, True)
    one, se_one, _ = mean_estimate(open_setup, False)
    print("\nquadrature", want[:, 0], "\nMIS       ", mis[:, 0], "+-", se_mis[:, 0], "\nlight only", one[:, 0], "+-", se_one[:, 0])
    assert est["kinds"][:, 1].sum() == 0 and est["kinds"][:, 0].reshape(len(POINTS), 3, -1).any(2).all()      # every light reaches every point
    assert (est["kinds"][:, 2].sum() > 1000) and (est["kinds"][:, 3].sum() > 1000)            # probes that meet the picked light, and the other
    assert (np.abs(mis - want) <= 3 * se_mis).all(), np.abs(mis - want) / se_mis
    assert (np.abs(one - want) <= 3 * se_one).all(), np.abs(one - want) / se_one
    assert (np.abs(mis - one) <= 3 * np.hypot(se_mis, se_one)).all()
    assert (se_mis > 0).all() and (se_mis < 0.02 * want).all()                              # the margin is a tight one: below 2 % of the value


@pytest.mark.parametrize("strategy", ["uniform", "power", "spatial", "one"])
def test_pick_pdfs_sum_to_one(open_setup, strategy):
    """(iii): over the lights, at 100 points of the scene's volume."""
    rng = np.random.default_rng(5)
    p = open_setup.wb[:3] + rng.random((100, 3)) * (open_setup.wb[3:] - open_setup.wb[:3])
    pdf, rel, _ = open_setup.pick_pdfs(p, strategy)
    assert pdf.shape == (100, 3) and (pdf > 0).all() and np.abs(pdf.sum(1) - 1.0).max() < 1e-12
    assert np.isfinite(rel).all()
    if strategy in ("uniform", "spatial"):
        assert len(np.unique(np.round(pdf, 9), axis=0)) > 50                               # it varies over the volume
    idx, und = open_setup.pick(pdf, rel, np.linspace(0.0, 1.0 - 2.0 ** -24, 100).astype(np.float32))
    assert idx.min() == 0 and idx.max() == 2 and und.sum() <= 3
