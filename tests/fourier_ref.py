"""Restatement of Material "fourier" in numpy, parameterised by dtype: FourierBSDF::f / pdf / sample_f (core/reflection/fourier.rs:251-456)
with the code they call -- catmull_rom_weights, sample_catmull_rom_2d (core/interpolation/catmul_rom.rs:3-179), evaluate_fourier,
sample_fourier (core/interpolation/fourier.rs:4-89) -- and FourierBSDFTable::read_body (fourier.rs:90-161) as an independent parse of the
file.  Independent of the product.  Run in float64 it is the truth the device is held to; run in float32 it is the reference's arithmetic
without a device (the calibration of test_fourier_host.py, and where the iteration maxima behind the device's loop caps are measured).

Bounds.  Every evaluated quantity is aov_ref's E: a value in the run's dtype and a float64 bound on the distance of a float32 evaluation
of the same expression from its exact value (first-order propagation, one rounding of 2^-24 |value| per operation).  Table entries and
directions are exact float32 numbers.  One place is not propagated step by step: the cosine iterates cos(k phi) of evaluate_fourier,
    c[k+1] = 2 cos_phi c[k] - c[k-1],
whose step-by-step bound grows like (1 + sqrt 2)^k while the recurrence does not.  A perturbation d entering at step j reaches step k
multiplied by U_{k-j-1}(cos_phi), the Chebyshev polynomial of the second kind, |U_n| <= min(n + 1, 1 / sin phi); each step rounds a
product and a difference of numbers that are at most about 1 and 2 (3 roundings of 2^-24 in all), and the error e_c of cos_phi itself
reaches cos(k phi) through its derivative k sin(k phi) / sin phi.  So
    |error of c[k]| <= 3 * 2^-24 * sum_{j=1..k} min(j, 1 / sin phi)  +  e_c * k * min(k, 1 / sin phi).
No constant is fitted to any implementation.

Sampling is held by inversion, not by equality: sample_catmull_rom_2d and sample_fourier stop a Newton-bisection at 1e-6, in the residual or
in the bracket, so two correct runs agree only to that.  inversion() turns a returned (wi, f, pdf) into the residuals of the two
cumulative distributions at the returned direction, with the bounds that follow from the stopping rules; see there.
"""
import numpy as np

from aov_ref import E, U, where
import bsdf_ref as R

F32 = np.float32
TYPE = R.REFL | R.TRANS | R.GLOSSY
C_G = (float(F32(1.39829)), float(F32(0.100913)), float(F32(0.297375)))
PI32 = float(F32(np.pi))
INV_2PI32 = float(F32(F32(1 / np.pi) * F32(0.5)))


def parse_file(path):
    """The file as read_body reads it, with numpy alone: a dict of the header fields and the arrays; trailing bytes are ignored."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"SCATFUN\x01", "magic"
    head = np.frombuffer(raw, "<i4", 14, 8)
    flags, n_mu, n_coeffs, m_max, n_channels, n_bases = [int(v) for v in head[:6]]
    eta = float(np.frombuffer(raw, "<f4", 1, 8 + 36)[0])
    assert flags == 1 and n_channels in (1, 3) and n_bases == 1
    at = 8 + 56
    mu = np.frombuffer(raw, "<f4", n_mu, at); at += 4 * n_mu
    cdf = np.frombuffer(raw, "<f4", n_mu * n_mu, at); at += 4 * n_mu * n_mu
    oal = np.frombuffer(raw, "<i4", 2 * n_mu * n_mu, at); at += 8 * n_mu * n_mu
    a = np.frombuffer(raw, "<f4", n_coeffs, at); at += 4 * n_coeffs
    return dict(n_mu=n_mu, n_coeffs=n_coeffs, m_max=m_max, n_channels=n_channels, eta=eta, mu=mu.copy(), cdf=cdf.copy(),
                offset_and_length=oal.copy(), a=a.copy(), trailing=len(raw) - at)


class Table:
    """FourierBSDFTable as read_body leaves it (a0 and recip included).  `t`: anything with the fields of capi.FourierTable."""

    def __init__(self, t):
        self.n = int(t.n_mu)
        self.n_channels, self.m_max, self.eta = int(t.n_channels), int(t.m_max), float(F32(t.eta))
        self.mu = np.asarray(t.mu, F32)
        self.cdf = np.asarray(t.cdf, F32).reshape(self.n, self.n)
        oal = np.asarray(t.offset_and_length, np.int64).reshape(self.n, self.n, 2)
        self.off, self.m = oal[..., 0], oal[..., 1]
        self.a = np.asarray(t.a, F32)
        self.a0 = np.where(self.m > 0, self.a[np.minimum(self.off, max(len(self.a) - 1, 0))] if len(self.a) else 0.0, 0.0).astype(F32)
        self.recip = np.concatenate([[np.inf], 1.0 / np.arange(1, max(self.m_max, 2), dtype=F32)]).astype(F32)


def _c(x, dt):
    return E(np.asarray(x).astype(dt))


def weights(T, x, dt):
    """catmull_rom_weights over T.mu at x (an E whose value decides the interval): ok, offset, [w0..w3]."""
    n, mu = T.n, T.mu
    xv = x.v.astype(np.float64)
    ok = (xv >= mu[0]) & (xv <= mu[-1])
    idx = np.clip(np.searchsorted(mu.astype(np.float64), xv, side="right") - 1, 0, n - 2)
    x0, x1 = _c(mu[idx], dt), _c(mu[idx + 1], dt)
    t = (x - x0) / (x1 - x0)
    t2 = t * t
    t3 = t2 * t
    w1 = 2.0 * t3 - 3.0 * t2 + 1.0
    w2 = -2.0 * t3 + 3.0 * t2
    has0, has3 = idx > 0, idx + 2 < n
    xm, xp = _c(mu[np.maximum(idx - 1, 0)], dt), _c(mu[np.minimum(idx + 2, n - 1)], dt)
    with np.errstate(all="ignore"):
        w0a = (t3 - 2.0 * t2 + t) * (x1 - x0) / where(has0, x1 - xm, x1 - x0)
        w0b = t3 - 2.0 * t2 + t
        w3a = (t3 - t2) * (x1 - x0) / where(has3, xp - x0, x1 - x0)
        w3b = t3 - t2
    zero = E(np.zeros(len(xv), dt))
    w0 = where(has0, -w0a, zero)
    w2 = where(has0, w2 + w0a, w2 + w0b)
    w1 = where(has0, w1, w1 - w0b)
    w3 = where(has3, w3a, zero)
    w1 = where(has3, w1 - w3a, w1 - w3b)
    w2 = where(has3, w2, w2 + w3b)
    return ok, idx - 1, [w0, w1, w2, w3]


class Ak:
    """create_ak without the array: the sixteen node pairs (b outer, a inner) with weight, length and offset; a pair of weight zero has
    length 0.  coeffs(c) gives a_k of channel c for every k < K as one E of shape (N, K): entries past a lane's own m_max are 0."""

    def __init__(self, T, off_i, w_i, off_o, w_o, dt):
        self.T, self.dt = T, dt
        n = T.n
        self.w, self.m, self.off = [], [], []
        for b in range(4):
            for a in range(4):
                w = w_i[a] * w_o[b]
                nz = w.v != 0
                oi, oo = np.clip(off_i + a, 0, n - 1), np.clip(off_o + b, 0, n - 1)
                self.w.append(w)
                self.m.append(np.where(nz, T.m[oo, oi], 0))
                self.off.append(np.where(nz, T.off[oo, oi], 0))
        self.m_max = np.maximum(1, np.max(np.stack(self.m), 0))
        self.K = int(self.m_max.max())

    def coeffs(self, c):
        N, K, T = len(self.m_max), self.K, self.T
        k = np.arange(K)[None, :]
        acc = E(np.zeros((N, K), self.dt))
        for j in range(16):
            act = k < self.m[j][:, None]
            if not act.any():
                continue
            idx = np.where(act, self.off[j][:, None] + c * self.m[j][:, None] + k, 0)
            term = E(np.repeat(self.w[j].v[:, None], K, 1), np.repeat(self.w[j].e[:, None], K, 1)) * E(T.a[idx].astype(self.dt))
            acc = where(act, acc + term, acc)
        return acc


def cos_d_phi(wa, wb, dt):
    """reflection/math.rs:70-81 on arrays of exact float32 components; an E."""
    return cos_d_phi_E(*[_c(v, dt) for v in (wa[:, 0], wa[:, 1], wb[:, 0], wb[:, 1])])


def cos_d_phi_E(ax, ay, bx, by):
    """... on components that are E's already (directions known within a bound)."""
    dt = ax.v.dtype.type
    waxy, wbxy = ax * ax + ay * ay, bx * bx + by * by
    flat = (waxy.v <= 0) | (wbxy.v <= 0)
    with np.errstate(all="ignore"):
        v = (ax * bx + ay * by) / (waxy * wbxy).sqrt()
    v = E(np.clip(v.v, -1, 1), v.e)
    return where(flat, E(np.ones(len(flat), dt)), v)


def series(AK, cos_phi, m_max):
    """evaluate_fourier over AK (an E of shape (N, K)): the sum in increasing k, the cosine iterates by the recurrence in the run's dtype
    with the bound of the module's docstring."""
    dt = AK.v.dtype.type
    N, K = AK.v.shape
    c = cos_phi.v.astype(dt)
    s = np.sqrt(np.maximum(1.0 - cos_phi.v.astype(np.float64) ** 2, 0.0))
    with np.errstate(all="ignore"):
        inv_s = np.where(s > 0, 1.0 / s, np.inf)
    value = E(np.zeros(N, dt))
    prev, cur = c.copy(), np.ones(N, dt)
    S = np.zeros(N)
    for k in range(K):
        if k > 0:
            S = S + np.minimum(k, inv_s)
        ck = E(cur.copy(), 3.0 * U * S + cos_phi.e * k * np.minimum(k, inv_s))
        live = k < m_max
        value = where(live, value + E(AK.v[:, k], AK.e[:, k]) * ck, value)
        nxt = (dt(2.0) * c * cur - prev).astype(dt)
        prev, cur = cur, nxt
    return value


def scale_of(T, mu_i, mu_o, dt):
    """1 / |mu_i| (0 at mu_i == 0), times eta^2 or 1 / eta^2 where mu_i mu_o > 0: the transport mode is radiance (fourier.rs:287-300)."""
    mi = mu_i.v.astype(np.float64)
    with np.errstate(all="ignore"):
        sc = where(mi != 0, 1.0 / mu_i.abs(), E(np.zeros(len(mi), dt)))
    eta = _c(np.full(len(mi), T.eta), dt)
    e = where(mi > 0, 1.0 / eta, eta)
    return where(mi * mu_o.v.astype(np.float64) > 0, sc * (e * e), sc)


class Eval:
    """f (N, 3), pdf (N) with their bounds, and `und`: an evaluation a branch of which lies within its own bound of its threshold."""

    def __init__(self, f, pdf, und):
        self.f = np.stack([c.v for c in f], 1).astype(np.float64)
        self.f_e = np.stack([c.e for c in f], 1)
        self.pdf, self.pdf_e = pdf.v.astype(np.float64), pdf.e
        self.und = und

    def left_out(self):
        """und, or a value or a bound that is not finite.  Unlike bsdf_ref's rule, a bound past R.REL_CAP of its value does NOT leave an
        evaluation out: away from its peak a Fourier series is a small difference of large terms, the bound (a share of sum |a_k|) is
        then a large share of the value -- 18 % of the drawn pairs on the rough-gold table -- and the evaluation is held to that bound
        all the same.  wide() reports the share."""
        return self.und | ~np.isfinite(self.f_e).all(1) | ~np.isfinite(self.f).all(1) | ~np.isfinite(self.pdf_e) | ~np.isfinite(self.pdf)

    def wide(self):
        with np.errstate(all="ignore"):
            return ((self.f_e > R.REL_CAP * np.abs(self.f)) & (self.f_e > 0)).any(1) | ((self.pdf_e > R.REL_CAP * np.abs(self.pdf)) & (self.pdf_e > 0))


class BSDF:
    """The BSDF of a Material "fourier" on the canonical frame (ns = ng = z): one lobe of type reflection | transmission | glossy."""

    def __init__(self, table, dtype=np.float64):
        self.T = table if isinstance(table, Table) else Table(table)
        self.dt = np.dtype(dtype).type

    def matches(self, flags):
        return (TYPE & flags) == TYPE

    def eval(self, wo, wi, flags, with_f=True):
        """BSDF::f and BSDF::pdf (bsdf.rs:208-270) for one lobe: zero where wo.z == 0 or the flags leave the lobe out."""
        dt = self.dt
        mwi = -np.asarray(wi, F32)
        wo = np.asarray(wo, F32)
        return self.eval_core(_c(mwi[:, 2], dt), _c(wo[:, 2], dt), cos_d_phi(mwi, wo, dt), flags, with_f)

    def eval_core(self, mu_i, mu_o, cphi, flags, with_f=True):
        """f and pdf from the two zenith cosines and cos(phi) (E's; the float64 run also takes numbers that are no float32)."""
        dt, T = self.dt, self.T
        ok_i, off_i, w_i = weights(T, mu_i, dt)
        ok_o, off_o, w_o = weights(T, mu_o, dt)
        ak = Ak(T, off_i, w_i, off_o, w_o, dt)
        ok = ok_i & ok_o
        N = len(mu_o.v)
        zero = E(np.zeros(N, dt))
        und = np.zeros(N, bool)
        AK0 = ak.coeffs(0)
        y_raw = series(AK0, cphi, ak.m_max)
        dead = ~ok | (mu_o.v == 0) | (not self.matches(flags))
        f = [zero, zero, zero]
        if with_f:
            y = E(np.maximum(y_raw.v, 0), y_raw.e)
            sc = scale_of(T, mu_i, mu_o, dt)
            if T.n_channels == 1:
                v = y * sc
                f = [v, v, v]
            else:
                r, b = series(ak.coeffs(1), cphi, ak.m_max), series(ak.coeffs(2), cphi, ak.m_max)
                g = _c(np.full(N, C_G[0]), dt) * y - _c(np.full(N, C_G[1]), dt) * b - _c(np.full(N, C_G[2]), dt) * r
                f = [E(np.maximum(c.v, 0), c.e) for c in (r * sc, g * sc, b * sc)]
            f = [where(dead, zero, c) for c in f]
        # pdf (fourier.rs:417-456): rho from the last column of the cdf rows of mu_o, zero weights skipped
        rho = zero
        two_pi = _c(np.full(N, float(F32(2.0) * F32(np.pi))), dt)
        for o in range(4):
            idx = np.clip(off_o + o, 0, T.n - 1)
            nz = w_o[o].v != 0
            rho = where(nz, rho + w_o[o] * _c(T.cdf[idx, T.n - 1], dt) * two_pi, rho)
        with np.errstate(all="ignore"):
            p = y_raw / rho
        pos = (rho.v > 0) & (y_raw.v > 0)
        # the two signs pdf reads: undecided within their bounds (an exact zero -- a row or a pair without energy -- is decided)
        und |= ~dead & (((np.abs(rho.v) <= rho.e) & (rho.e > 0)) | ((np.abs(y_raw.v) <= y_raw.e) & (y_raw.e > 0)))
        pdf = where(pos & ~dead, p, zero)
        ev = Eval(f, pdf, und)
        # sum k |a_k| / rho: the slope of pdf in phi (inversion's users turn an error of the angle into one of pdf with it)
        kk = np.arange(AK0.v.shape[1])[None, :]
        with np.errstate(all="ignore"):
            ev.pdf_slope_phi = np.where(pos & ~dead, (np.abs(AK0.v.astype(np.float64)) * kk * (kk < ak.m_max[:, None])).sum(1) / np.abs(rho.v.astype(np.float64)), 0.0)
        return ev

    # ---- the float sampler (the restatement as an implementation, and the source of the None decisions)
    def _interp(self, arr, off, w, idx):
        v = np.zeros(len(idx), self.dt)
        for i in range(4):
            nz = w[i] != 0
            row = np.clip(off + i, 0, self.T.n - 1)
            v = np.where(nz, (v + arr[row, idx].astype(self.dt) * w[i]).astype(self.dt), v)
        return v

    def sample_mu(self, mu_o, u):
        """sample_catmull_rom_2d(mu, mu, a0, cdf, mu_o, u): (ok, mu_i, pdf, iterations, maximum), in the run's dtype without bounds."""
        dt, T, n = self.dt, self.T, self.T.n
        ok, off, wE = weights(T, _c(mu_o, dt), dt)
        w = [c.v for c in wE]
        N = len(mu_o)
        last = np.full(N, n - 1)
        with np.errstate(all="ignore"):
            maximum = self._interp(T.cdf, off, w, last)
            uu = (np.asarray(u, dt) * maximum).astype(dt)
            first, length = np.zeros(N, np.int64), np.full(N, n, np.int64)
            while (length > 0).any():
                live = length > 0
                half = length >> 1
                mid = np.minimum(first + half, n - 1)
                pred = self._interp(T.cdf, off, w, mid) <= uu
                first = np.where(live & pred, mid + 1, first)
                length = np.where(live, np.where(pred, length - (half + 1), half), length)
            idx = np.where(first == 0, n - 2, np.minimum(first - 1, n - 2))
            f0, f1 = self._interp(T.a0, off, w, idx), self._interp(T.a0, off, w, idx + 1)
            x0, x1 = T.mu[idx].astype(dt), T.mu[idx + 1].astype(dt)
            width = (x1 - x0).astype(dt)
            uu = ((uu - self._interp(T.cdf, off, w, idx)) / width).astype(dt)
            fm = self._interp(T.a0, off, w, np.maximum(idx - 1, 0))
            fp = self._interp(T.a0, off, w, np.minimum(idx + 2, n - 1))
            d0 = np.where(idx > 0, width * (f1 - fm) / (x1 - T.mu[np.maximum(idx - 1, 0)].astype(dt)), f1 - f0).astype(dt)
            d1 = np.where(idx + 2 < n, width * (fp - f0) / (T.mu[np.minimum(idx + 2, n - 1)].astype(dt) - x0), f1 - f0).astype(dt)
            t = np.where(f0 != f1, (f0 - np.sqrt(np.maximum(dt(0), f0 * f0 + dt(2) * uu * (f1 - f0)))) / (f0 - f1), uu / f0).astype(dt)
            a, b = np.zeros(N, dt), np.ones(N, dt)
            fhat = np.zeros(N, dt)
            done = ~ok
            iters = np.zeros(N, np.int64)
            for _ in range(200):
                if done.all():
                    break
                t = np.where(~done & ~((t >= a) & (t <= b)), dt(0.5) * (a + b), t).astype(dt)
                third = dt(1.0) / dt(3.0)
                Fh = (t * (f0 + t * (dt(0.5) * d0 + t * (third * (dt(-2.0) * d0 - d1) + f1 - f0 + t * (dt(0.25) * (d0 + d1) + dt(0.5) * (f0 - f1)))))).astype(dt)
                fh = (f0 + t * (d0 + t * (dt(-2.0) * d0 - d1 + dt(3.0) * (f1 - f0) + t * (d0 + d1 + dt(2.0) * (f0 - f1))))).astype(dt)
                fhat = np.where(done, fhat, fh)
                iters += ~done
                stop = (np.abs(Fh - uu) < dt(1e-6)) | (b - a < dt(1e-6))
                go = ~done & ~stop
                lo = go & (Fh - uu < 0)
                a = np.where(lo, t, a)
                b = np.where(go & ~lo, t, b)
                t = np.where(go, t - (Fh - uu) / fh, t).astype(dt)
                done = done | stop
            assert done.all(), "sample_catmull_rom_2d: 200 iterations"
            pdf = (fhat / maximum).astype(dt)
            value = (x0 + width * t).astype(dt)
        return ok, value, pdf, iters, maximum

    def sample_phi(self, ak0, AK, m_max, u):
        """sample_fourier over the luminance coefficients (the float32 numbers AK.v, as the reference holds them) in float64, whatever the
        run's dtype: (y, pdf, phi, iterations)."""
        N, K = AK.shape
        u = np.asarray(u, F32)
        flip = u >= F32(0.5)
        u = np.where(flip, F32(1.0) - F32(2.0) * (u - F32(0.5)), u * F32(2.0)).astype(F32)
        a, b, phi = np.zeros(N), np.full(N, float(F32(np.pi))), np.full(N, 0.5 * float(F32(np.pi)))
        rec = self.T.recip
        with np.errstate(all="ignore"):          # (ak[k] * recip[k]) as f64: one float32 product; entry 0 (recip[0] = inf) is never read
            ak_rec = (AK * rec[None, :K].astype(AK.dtype)).astype(AK.dtype).astype(np.float64)
        ak64 = AK.astype(np.float64)
        f = np.zeros(N)
        done = np.zeros(N, bool)
        iters = np.zeros(N, np.int64)
        target = (u.astype(AK.dtype) * ak0 * AK.dtype.type(PI32)).astype(np.float64)
        with np.errstate(all="ignore"):
            for _ in range(400):
                if done.all():
                    break
                cp = np.cos(phi)
                sp = np.sqrt(np.maximum(0.0, 1.0 - cp * cp))
                cprev, ccur, sprev, scur = cp.copy(), np.ones(N), -sp, np.zeros(N)
                Fv = ak64[:, 0] * phi
                fv = ak64[:, 0].copy()
                for k in range(1, K):
                    sn = 2.0 * cp * scur - sprev
                    cn = 2.0 * cp * ccur - cprev
                    sprev, scur, cprev, ccur = scur, sn, ccur, cn
                    live = k < m_max
                    Fv = np.where(live, Fv + ak_rec[:, k] * sn, Fv)
                    fv = np.where(live, fv + ak64[:, k] * cn, fv)
                Fv = Fv - target
                f = np.where(done, f, fv)
                iters += ~done
                up = Fv > 0
                b = np.where(~done & up, phi, b)
                a = np.where(~done & ~up, phi, a)
                stop = (np.abs(Fv) < 1e-6) | (b - a < 1e-6)
                go = ~done & ~stop
                nphi = phi - Fv / fv
                nphi = np.where(~((nphi > a) & (nphi < b)), 0.5 * (a + b), nphi)
                phi = np.where(go, nphi, phi)
                done = done | stop
            assert done.all(), "sample_fourier: 400 iterations"
            phi = np.where(flip, float(F32(2.0) * F32(np.pi)) - phi, phi)
            pdf = (AK.dtype.type(INV_2PI32) / ak0 * f.astype(AK.dtype)).astype(AK.dtype)
        return f.astype(AK.dtype), pdf, phi.astype(AK.dtype), iters

    def sample(self, wo, u, flags):
        """BSDF::sample_f for the one lobe: f, wi, pdf, type (0: None) and the two iteration counts, in the run's dtype."""
        dt, T = self.dt, self.T
        wo = np.asarray(wo, F32)
        u = np.asarray(u, F32)
        N = len(wo)
        mu_o = wo[:, 2].astype(dt)
        ok, mu_i, pdf_mu, it_mu, maximum = self.sample_mu(mu_o, u[:, 1])
        ok_i, off_i, w_i = weights(T, _c(mu_i, dt), dt)
        ok_o, off_o, w_o = weights(T, _c(mu_o, dt), dt)
        ak = Ak(T, off_i, w_i, off_o, w_o, dt)
        AK = ak.coeffs(0).v
        y, pdf_phi, phi, it_phi = self.sample_phi(AK[:, 0], AK, ak.m_max, u[:, 0])
        with np.errstate(all="ignore"):
            pdf = np.fmax(dt(0), pdf_phi * pdf_mu)          # f32::max: a NaN product is 0
            pdf = np.where(np.isnan(pdf_phi * pdf_mu), dt(0), pdf)
            some = ok & ok_i & (pdf > 0) & (wo[:, 2] != 0) & self.matches(flags)
            sin2_i = np.maximum(dt(0), dt(1) - mu_i * mu_i).astype(dt)
            sin2_o = np.maximum(dt(0), dt(1) - mu_o * mu_o).astype(dt)
            norm = np.sqrt(sin2_i / sin2_o).astype(dt)
            norm = np.where(np.isinf(norm), dt(0), norm)
            sp, cp = np.sin(phi).astype(dt), np.cos(phi).astype(dt)
            x, yv = wo[:, 0].astype(dt), wo[:, 1].astype(dt)
            v = np.stack([norm * (cp * x - sp * yv), norm * (sp * x + cp * yv), mu_i], 1).astype(dt)
            wi = -(v / np.sqrt((v * v).sum(1))[:, None]).astype(dt)
        wi = np.where(some[:, None], wi, 0)
        typ = np.where(some, TYPE, 0).astype(np.uint32)
        f = np.zeros((N, 3))
        if some.any():          # the BSDF evaluates f again at the returned wi: the lobe is not specular (bsdf.rs:186-200)
            ev = self.eval(wo[some], wi[some].astype(F32), flags)
            f[some] = ev.f
        # `maximum` is a sum of four products: a float32 run forms it within 8 roundings of sum |w| cdf (what decides "a row without energy")
        max_abs = sum(np.abs(w_o[i].v.astype(np.float64)) * T.cdf[np.clip(off_o + i, 0, T.n - 1), T.n - 1] for i in range(4))
        return dict(f=f, wi=wi, pdf=np.where(some, pdf, 0), type=typ, max_abs=max_abs, it_mu=np.where(ok, it_mu, 0), it_phi=np.where(ok & ok_i & (pdf_mu > 0), it_phi, 0),
                    maximum=maximum, pdf_mu=pdf_mu, ok=ok)

    # ---- a returned sample held by inversion
    def inversion(self, wo, u, wi):
        """For samples (wo, u) that returned the direction wi (float32 arrays): the residuals of the two cumulative distributions at the
        returned direction and their bounds, in this run's arithmetic (meant for the float64 run).

        mu.  sample_f normalises (norm (..), norm (..), mu_i) with norm^2 = (1 - mu_i^2) / sin2(wo), sin2(wo) = fl(1 - fl(wo.z^2)), so
        the vector's length is sqrt((1 - mu_i^2) r + mu_i^2) with r = (wo.x^2 + wo.y^2) / sin2(wo), which is 1 only as far as wo is a
        unit vector; mu_i is recovered from z = -wi.z as z sqrt(r / (1 - z^2 (1 - r))).  With C the interpolated cdf (rows weighted at
        mu_o) and the spline segment [x0, x1] of width w the sampler solves  C(x0) + w That(t) = u maximum  and stops at
        |That(t) - u'| < 1e-6 or at a bracket below 1e-6 in t, so
            |cdf(mu_i) - u| <= 1e-6 w max(1, Fmax) / maximum          Fmax = |f0| + |d0| + |-2 d0 - d1 + 3 (f1 - f0)| + |d0 + d1 + 2 (f0 - f1)|
        (Fmax bounds |fhat| on [0, 1], the slope of That).  Rounding on top: That's Horner form has 12 operations on magnitudes up to
        M = |f0| + |f1| + |d0| + |d1| (12 U w M / maximum); u', the interpolated cdf values and maximum take 20 operations on
        magnitudes up to maximum (20 U); mu_i = x0 + w t, the normalisation and the recovery above take 10 more on mu_i, each moving
        the cdf by its slope, pdf_mu = fhat / maximum (10 U |mu_i| fhat / maximum).

        phi.  The angle from wo's azimuth to -wi's.  sample_fourier solves  a0 phi + sum a_k sin(k phi) / k = u' a0 pi  on [0, pi]
        (u' = 2 u, or 2 - 2 u and phi -> 2 pi - phi past one half) and stops at a residual of 1e-6 or a bracket of 1e-6 in phi, so
            |G(phi) - u'| <= 1e-6 max(1, sum |a_k|) / (a0 pi)         G = (a0 phi + sum a_k sin(k phi) / k) / (a0 pi)
        Rounding on top: phi is rounded to float32 (2 pi U), its sine and cosine are libm's (2 ulp each, 4 U), the rotation, the
        product with norm and the normalisation take 7 more (7 U): 18 U of angle in all, times the slope sum |a_k| / (a0 pi); and the
        a_k themselves carry their bounds e_k from create_ak (sum e_k (phi or 1 / k) / (a0 pi)).

        Returns dict(mu_res, mu_tol, phi_res, phi_tol, mu_i, ok): ok is False where the returned direction does not determine the sample
        (wo or wi along the normal: norm is 0 or the azimuth is gone)."""
        dt, T, n = np.float64, self.T, self.T.n
        wo, wi, u = np.asarray(wo, F32), np.asarray(wi, F32), np.asarray(u, F32)
        N = len(wo)
        z2 = (wo[:, 2] * wo[:, 2]).astype(F32)
        sin2_o = np.maximum(F32(0), (F32(1) - z2).astype(F32)).astype(np.float64)
        wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
        with np.errstate(all="ignore"):
            r = (wo64[:, 0] ** 2 + wo64[:, 1] ** 2) / sin2_o
            z = -wi64[:, 2]
            mu_i = z * np.sqrt(r / (1.0 - z * z * (1.0 - r)))
        okk = (sin2_o > 0) & np.isfinite(mu_i) & (np.abs(mu_i) <= 1) & ((wi64[:, 0] ** 2 + wi64[:, 1] ** 2) > 0) & ((wo64[:, 0] ** 2 + wo64[:, 1] ** 2) > 0)
        mu_i = np.where(okk, mu_i, 0.0)
        mu_i = np.clip(mu_i, float(T.mu[0]), float(T.mu[-1]))
        ok_o, off, wE = weights(T, _c(wo[:, 2], dt), dt)
        w = [c.v for c in wE]
        sav = self.dt
        self.dt = np.float64
        try:
            maximum = self._interp(T.cdf, off, w, np.full(N, n - 1))
            idx = np.clip(np.searchsorted(T.mu.astype(np.float64), mu_i, side="right") - 1, 0, n - 2)
            f0, f1 = self._interp(T.a0, off, w, idx), self._interp(T.a0, off, w, idx + 1)
            x0, x1 = T.mu[idx].astype(dt), T.mu[idx + 1].astype(dt)
            width = x1 - x0
            fm = self._interp(T.a0, off, w, np.maximum(idx - 1, 0))
            fp = self._interp(T.a0, off, w, np.minimum(idx + 2, n - 1))
            d0 = np.where(idx > 0, width * (f1 - fm) / (x1 - T.mu[np.maximum(idx - 1, 0)]), f1 - f0)
            d1 = np.where(idx + 2 < n, width * (fp - f0) / (T.mu[np.minimum(idx + 2, n - 1)] - x0), f1 - f0)
            c0 = self._interp(T.cdf, off, w, idx)
        finally:
            self.dt = sav
        with np.errstate(all="ignore"):
            t = (mu_i - x0) / width
            That = t * (f0 + t * (0.5 * d0 + t * ((1.0 / 3.0) * (-2.0 * d0 - d1) + f1 - f0 + t * (0.25 * (d0 + d1) + 0.5 * (f0 - f1)))))
            fhat = f0 + t * (d0 + t * (-2.0 * d0 - d1 + 3.0 * (f1 - f0) + t * (d0 + d1 + 2.0 * (f0 - f1))))
            cdf_mu = (c0 + width * That) / maximum
            Fmax = np.abs(f0) + np.abs(d0) + np.abs(-2.0 * d0 - d1 + 3.0 * (f1 - f0)) + np.abs(d0 + d1 + 2.0 * (f0 - f1))
            M = np.abs(f0) + np.abs(f1) + np.abs(d0) + np.abs(d1)
            mu_tol = (1e-6 * width * np.maximum(1.0, Fmax) + 12.0 * U * width * M) / maximum + 20.0 * U + 10.0 * U * np.abs(mu_i) * np.abs(fhat) / maximum
            mu_res = np.abs(cdf_mu - u[:, 1].astype(np.float64))
        # phi
        ok_i, off_i, w_i = weights(T, _c(mu_i, dt), dt)
        ak = Ak(T, off_i, w_i, off, wE, dt)
        AK = ak.coeffs(0)
        a, b = -wi64[:, :2], wo64[:, :2]
        phi = np.arctan2(b[:, 0] * a[:, 1] - b[:, 1] * a[:, 0], b[:, 0] * a[:, 0] + b[:, 1] * a[:, 1]) % (2.0 * np.pi)
        flip = phi > np.pi
        ph = np.where(flip, 2.0 * np.pi - phi, phi)
        k = np.arange(1, max(ak.K, 2))
        live = k[None, :] < ak.m_max[:, None]
        akv, ake = AK.v[:, 1:], AK.e[:, 1:]
        if akv.shape[1] == 0:
            akv, ake = np.zeros((N, 1)), np.zeros((N, 1))
        a0 = AK.v[:, 0]
        with np.errstate(all="ignore"):
            G = (a0 * ph + np.where(live, akv * np.sin(k[None, :] * ph[:, None]) / k[None, :], 0.0).sum(1)) / (a0 * np.pi)
            uu = u[:, 0].astype(np.float64)
            target = np.where(flip, 2.0 - 2.0 * uu, 2.0 * uu)
            # u == 0.5 exactly flips in the sampler (u >= 0.5) while phi == pi is read here as not flipped: both targets are 1 there
            slope = (np.abs(a0) + np.where(live, np.abs(akv), 0.0).sum(1)) / (np.abs(a0) * np.pi)
            e_ak = (AK.e[:, 0] * ph + np.where(live, ake / k[None, :], 0.0).sum(1)) / (np.abs(a0) * np.pi)
            phi_tol = 1e-6 * np.maximum(1.0 / (np.abs(a0) * np.pi), slope) + 18.0 * U * slope + e_ak + 4.0 * U
            phi_res = np.abs(G - target)
            phi_res = np.minimum(phi_res, 2.0 - phi_res)          # the angle is periodic: u[0] at 0 or next to 1 returns phi next to 0 from either side
        return dict(mu_res=mu_res, mu_tol=mu_tol, phi_res=phi_res, phi_tol=phi_tol, mu_i=mu_i, ok=okk & ok_o & ok_i & (maximum > 0) & (a0 > 0))


class FrameTruth:
    """A BSDF behind bsdf_ref's interface: directions on the shading frame as lists of three E (values with their bounds), as the
    lit-quad checks hand them over."""

    def __init__(self, bsdf):
        self.b = bsdf

    def eval(self, wo, wi, flags):
        return self.b.eval_core(-wi[2], wo[2], cos_d_phi_E(-wi[0], -wi[1], wo[0], wo[1]), flags)


class Restatement32:
    """The float32 run behind the hooks' interface."""

    def __init__(self, table):
        self.b = BSDF(table, np.float32)

    def eval(self, wo, wi, flags):
        v = self.b.eval(wo, wi, flags)
        return v.f.astype(F32), v.pdf.astype(F32)

    def sample(self, wo, u, flags):
        s = self.b.sample(wo, u, flags)
        return s["f"].astype(F32), s["wi"].astype(F32), s["pdf"].astype(F32), s["type"]
