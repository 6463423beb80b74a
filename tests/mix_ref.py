"""Restatement of Material "mix" in numpy, on top of bsdf_ref (which it imports and leaves alone): MixMaterial::compute_scattering_functions
(materials/mix.rs:53-96) and ScaledBxDF (core/reflection/scaled.rs) under BSDF::f / pdf / sample_f (core/reflection/bsdf.rs:92-270), on
the canonical frame.  Written from the reference's text; independent of the oracle and of the product.

Input is a nested dict: {"type": "mix", "m1": ..., "m2": ..., "amount": (r, g, b)} with bsdf_ref parameter dicts (or further mixes) as
m1 / m2.  What is restated:

  * mix.rs:62-63    s1 = amount.clamp_zero(), s2 = (1 - s1).clamp_zero(), per channel.  s1 weights m1 (the opposite sense to Texture "mix")
                    and is not clamped above 1.
  * mix.rs:30-45    every BxDF of m1 in its order wrapped in ScaledBxDF(s1), then every BxDF of m2 wrapped in ScaledBxDF(s2).  No limit.
  * scaled.rs:32-47 f and the spectrum of sample_f are scale * inner: one multiply per channel.  pdf, type and wi are the inner lobe's.
                    A lobe scaled by 0 stays in the list: num_components, the component choice and the averaged pdf count it.
  * nesting         a child that is a mix hands over wrapped lobes, which are wrapped again: f = s_outer * (s_inner * f), innermost
                    multiply first.
  * a child without a BSDF (black glass / translucent) trips the reference's assert; here it contributes no lobes.

Run in float64 it is the truth; run in float32 it is the calibration.  Bounds are propagated as bsdf_ref does: every scale multiply is
one E multiplication, i.e. first-order propagation plus one float32 rounding.  No constant is fitted.

The class has the interface bsdf_cases.check_eval / check_sample use: terms, combine, eval, sample, eval_at_sampled, lobes[i].kind /
.matches.  bsdf_ref.BSDF.sample calls the module-level lobe_* functions directly, so sample() is restated here with the scale applied
where ScaledBxDF applies it."""
import numpy as np

import bsdf_ref as R
from bsdf_ref import E, decide, emax, emin, vexact

ALL = R.ALL


def _scales(amount, dt):
    """(s1, s2) of one mix node, three E scalars each."""
    s1 = [emax(E(np.asarray(R.c32(a), dt)), 0.0) for a in amount]
    s2 = [emax(1.0 - s, 0.0) for s in s1]
    return s1, s2


def flatten(tree, dt):
    """[(Lobe, chain)] in list order; chain = the scales above the lobe, innermost first."""
    if tree["type"] != "mix":
        has, lobes = R.build_lobes(tree, dt)
        return [(l, []) for l in lobes] if has else []
    s1, s2 = _scales(tree.get("amount", (0.5, 0.5, 0.5)), dt)
    out = []
    for child, s in ((tree["m1"], s1), (tree["m2"], s2)):
        out += [(l, chain + [s]) for l, chain in flatten(child, dt)]
    return out


def leaf_count(tree):
    return 1 if tree["type"] != "mix" else leaf_count(tree["m1"]) + leaf_count(tree["m2"])


def scale(chain, f):
    """ScaledBxDF::f applied once per wrapper, innermost first: one multiply per channel and wrapper."""
    for s in chain:
        f = [R.bcast(s[c], f[c]) * f[c] for c in range(3)]
    return f


class BSDF(R.BSDF):
    """The BSDF a mix tree leaves on the canonical frame, in the run's dtype."""

    def __init__(self, tree, dtype=np.float64):
        self.dt = np.dtype(dtype).type
        flat = flatten(tree, self.dt)
        self.has_bsdf = True                       # MixMaterial always allocates its BSDF (mix.rs:81-88)
        self.lobes = [l for l, _ in flat]
        self.chains = [c for _, c in flat]

    def terms(self, wo, wi):
        wo, wi = self._in(wo), self._in(wi)
        out = []
        for l, chain in zip(self.lobes, self.chains):
            und = np.zeros(len(wo[2].v), bool)
            out.append((scale(chain, R.lobe_f(l, wo, wi, und)), R.lobe_pdf(l, wo, wi, und), und))
        return wo, wi, out

    def sample(self, wo, u, flags=ALL):
        """BSDF::sample_f (bsdf.rs:92-206) over the wrapped lobes: bsdf_ref.BSDF.sample with ScaledBxDF::sample_f's multiply after the inner
        lobe's sample_f (scaled.rs:38-47) and ScaledBxDF::f in the re-summed f."""
        n = len(wo)
        dt = self.dt
        out = dict(wi=np.zeros((n, 3)), wi_e=np.zeros((n, 3)), type=np.zeros(n, np.uint32), und=np.zeros(n, bool), pick=np.full(n, -1),
                   specular=np.zeros(n, bool), f=np.zeros((n, 3)), f_e=np.zeros((n, 3)), pdf=np.zeros(n), pdf_e=np.zeros(n))
        match = [i for i, l in enumerate(self.lobes) if l.matches(flags)]
        m = len(match)
        if m == 0:
            return out
        wov = vexact(wo, dt)
        u1, u2 = E(np.asarray(u, np.float32)[:, 0].astype(dt)), E(np.asarray(u, np.float32)[:, 1].astype(dt))
        um = u1 * float(m)
        fl = np.floor(um.v)
        und = np.zeros(n, bool)
        for b in range(1, m):
            decide(um, und, float(b))
        comp = np.minimum(fl.astype(np.int64), m - 1)
        remapped = emin(um - E(comp.astype(dt)), R.ONE_MINUS_EPSILON)
        dead = (wov[2].v == 0) | ~np.isfinite(wov[0].v + wov[1].v + wov[2].v)
        for j, li in enumerate(match):
            sel = (comp == j) & ~dead
            if not sel.any():
                continue
            l = self.lobes[li]
            w = [c.take(sel) for c in wov]
            ul = np.zeros(int(sel.sum()), bool)
            s = R.lobe_sample(l, w, remapped.take(sel), u2.take(sel), ul)
            some = s["some"].copy()
            up = np.zeros(len(ul), bool)
            decide(s["pdf"], up)
            ul |= up & some
            some &= ~(s["pdf"].v <= 0)
            spec = bool(l.type & R.SPECULAR)
            t = np.where(s["type"] != 0, s["type"], l.type).astype(np.uint32)
            idx = np.flatnonzero(sel)
            out["pick"][idx] = li
            out["specular"][idx] = spec
            out["type"][idx] = np.where(some, t, 0)
            out["und"][idx] = ul
            out["wi"][idx] = np.where(some[:, None], np.stack([c.v for c in s["wi"]], 1).astype(np.float64), 0.0)
            out["wi_e"][idx] = np.where(some[:, None], np.stack([c.e for c in s["wi"]], 1), 0.0)
            if spec:
                with np.errstate(all="ignore"):
                    sf = scale(self.chains[li], s["f"])
                pdf = s["pdf"] / float(m) if m > 1 else s["pdf"]
                out["f"][idx] = np.where(some[:, None], np.stack([c.v for c in sf], 1).astype(np.float64), 0.0)
                out["f_e"][idx] = np.where(some[:, None], np.stack([c.e for c in sf], 1), 0.0)
                out["pdf"][idx] = np.where(some, pdf.v.astype(np.float64), 0.0)
                out["pdf_e"][idx] = np.where(some, pdf.e, 0.0)
            else:
                terms = []
                with np.errstate(all="ignore"):
                    for k, l2 in enumerate(self.lobes):
                        u2_ = np.zeros(len(ul), bool)
                        terms.append((scale(self.chains[k], R.lobe_f(l2, w, s["wi"], u2_)), s["pdf"] if k == li else R.lobe_pdf(l2, w, s["wi"], u2_), u2_))
                    val = self.combine(w, s["wi"], terms, flags)
                out["f"][idx], out["f_e"][idx] = np.where(some[:, None], val.f, 0.0), np.where(some[:, None], val.f_e, 0.0)
                out["pdf"][idx], out["pdf_e"][idx] = np.where(some, val.pdf, 0.0), np.where(some, val.pdf_e, 0.0)
        out["und"] |= und & ~dead
        return out


class Restatement32:
    """The float32 run behind the hooks' interface (bsdf_cases.Restatement32 for a mix tree)."""

    def __init__(self, tree):
        self.b = BSDF(tree, np.float32)

    def eval(self, wo, wi, flags):
        v = self.b.eval(wo, wi, flags)
        return v.f.astype(np.float32), v.pdf.astype(np.float32)

    def sample(self, wo, u, flags):
        s = self.b.sample(wo, u, flags)
        return s["f"].astype(np.float32), s["wi"].astype(np.float32), s["pdf"].astype(np.float32), s["type"]
