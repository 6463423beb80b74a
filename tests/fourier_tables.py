"""Synthetic tabulated BSDFs for the Material "fourier" tests, and a writer of the "SCATFUN" file format.

Every table is made from a positive analytic function.  A node pair (mu_i, mu_o) of length m holds the first m coefficients of
    A(mu_i, mu_o) * P_r(phi),      P_r(phi) = 1 + 2 sum_k r^k cos(k phi) = (1 - r^2) / (1 - 2 r cos(phi) + r^2)   (the Poisson kernel),
with r = q^(m_ref / m), so that r^m = q^m_ref whatever the length: the truncated series stays positive (its tail, at most
2 r^m / (1 - r), is far below the kernel's minimum (1 - r) / (1 + r)).  A carries the |mu_i| that FourierBSDF::f divides out again.
cdf rows are integrate_catmull_rom (core/interpolation/catmul_rom.rs:181-212) of the row's zeroth coefficients over mu_i, in float64,
then rounded to float32.

  two_sided  6 non-uniform nodes including -1, 0 and 1, one channel, eta 1.5, lengths 0..5 varying per pair, energy on both sides
  rgb_long   8 nodes, three channels, lengths up to 70 (past one wavefront's width), odd offsets (no run is 16-byte aligned), some pairs empty
  dark       every length 0: f = 0, pdf = 0, every sample None
"""
import functools
import struct

import numpy as np

from helpers import pkg

capi = pkg.capi


def integrate_catmull_rom(x, values):
    n = len(x)
    cdf = np.zeros(n)
    total = 0.0
    for i in range(n - 1):
        x0, x1, f0, f1 = x[i], x[i + 1], values[i], values[i + 1]
        width = x1 - x0
        d0 = width * (f1 - values[i - 1]) / (x1 - x[i - 1]) if i > 0 else f1 - f0
        d1 = width * (values[i + 2] - f0) / (x[i + 2] - x0) if i + 2 < n else f1 - f0
        total += ((d0 - d1) * (1.0 / 12.0) + (f0 + f1) * 0.5) * width
        cdf[i + 1] = total
    return cdf


def _make(mu, n_channels, eta, length_of, amplitude, q, m_ref, odd_offsets):
    mu = np.asarray(mu, np.float32)
    n = len(mu)
    oal = np.zeros((n, n, 2), np.int32)
    a = []
    a0 = np.zeros((n, n))
    at = 0
    for o in range(n):
        for i in range(n):
            m = int(length_of(o, i))
            if odd_offsets and at % 2 == 0:          # a filler coefficient no pair points at
                a.append(123.0)
                at += 1
            oal[o, i] = (at, m)
            if m == 0:
                continue
            r = q ** (m_ref / m)
            base = np.concatenate([[1.0], 2.0 * r ** np.arange(1, m)])
            for c in range(n_channels):
                run = (amplitude(float(mu[i]), float(mu[o]), c) * base).astype(np.float32)
                a.extend(run.tolist())
                if c == 0:
                    a0[o, i] = float(run[0])
            at += n_channels * m
    cdf = np.stack([integrate_catmull_rom(mu.astype(np.float64), a0[o]) for o in range(n)]).astype(np.float32)
    m_max = int(oal[..., 1].max())
    return capi.FourierTable(mu, cdf, oal, np.asarray(a, np.float32), n_channels, m_max, eta)


@functools.lru_cache(maxsize=None)
def two_sided():
    mu = [-1.0, -0.6, 0.0, 0.3, 0.8, 1.0]

    def length_of(o, i):
        return (2 * o + 3 * i + 1) % 6          # 0..5, every value taken, zeros scattered over the pairs

    def amplitude(mi, mo, c):
        return (abs(mi) + 0.05) * (0.25 + 0.5 * np.exp(-3.0 * (mi + mo) ** 2) + 0.2 * np.exp(-3.0 * (mi - mo) ** 2))
    return _make(mu, 1, 1.5, length_of, amplitude, 0.3, 5, False)


@functools.lru_cache(maxsize=None)
def rgb_long():
    mu = [-1.0, -0.7, -0.35, -0.1, 0.2, 0.5, 0.85, 1.0]

    def length_of(o, i):
        if (o + 2 * i) % 7 == 3:
            return 0
        return 1 + (11 * o + 23 * i) % 70          # 1..70, both ends taken

    def amplitude(mi, mo, c):
        y = (abs(mi) + 0.05) * (0.3 + 0.6 * np.exp(-4.0 * (mi + mo) ** 2))
        return y * (1.0, 0.9, 0.6)[c]                # Y, R, B: green = 1.39829 Y - 0.100913 B - 0.297375 R stays positive
    return _make(mu, 3, 1.33, length_of, amplitude, 0.85, 70, True)


@functools.lru_cache(maxsize=None)
def dark():
    mu = [-1.0, -0.2, 0.4, 1.0]
    return _make(mu, 1, 1.0, lambda o, i: 0, lambda mi, mo, c: 0.0, 0.5, 1, False)


def write_bsdf(path, t, flags=1, n_bases=1, trailing=b""):
    """The table as a "SCATFUN\\x01" file, in FourierBSDFTable::read_body's order (core/reflection/fourier.rs:90-128)."""
    with open(path, "wb") as f:
        f.write(b"SCATFUN\x01")
        f.write(struct.pack("<6i", flags, t.n_mu, t.n_coeffs, t.m_max, t.n_channels, n_bases))
        f.write(struct.pack("<3i", 0, 0, 0))
        f.write(struct.pack("<f", t.eta))
        f.write(struct.pack("<4i", 0, 0, 0, 0))
        for arr, dt in ((t.mu, "<f4"), (t.cdf, "<f4"), (t.offset_and_length, "<i4"), (t.a, "<f4")):
            f.write(np.asarray(arr).astype(dt).tobytes())
        f.write(trailing)
    return str(path)
