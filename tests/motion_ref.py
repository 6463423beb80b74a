"""Float64 truth for rays against instances that move (motion blur), on top of geometry_ref.py.

Independent of the oracle and of the kernels: numpy only.  The input is the float32 decomposition the library itself produced for the
two ends of every moving instance (capi.motion_decompose -- held on its own, against decompose64 below, in test_motion_host.py): T, R, S.

  * M64(t) is the exact-arithmetic image of what AnimatedTransform::interpolate computes from those values
    (animated_transform.rs:63-81): dt = (t - t0) / (t1 - t0), T = (1 - dt) T0 + dt T1, R = slerp(dt, R0, R1) with the reference's
    clamp of the dot to [0, 1] and its `c > 1 - EPSILON` early return (quaternion.rs:45-55), S likewise, M = translate * rotate * scale;
    M64(t)^-1 is numpy.linalg.inv of it.  At t <= t0 (or when the two ends are equal) and at t1 <= t the reference returns the stored
    transforms: the truth then takes the stored float32 inverse exactly as geometry_ref does for a static instance.
  * A ray at time t against a moving instance is geometry_ref's instance case under M64(t)^-1, one matrix per ray.

The bound per ray is geometry_ref's instance bound plus the effect of the float32 error of M(t)^-1 on the instance-space origin and
direction, |dM^-1| |o| and |dM^-1| |d| entrywise, added to o_err and d_err and carried through the same first-order forms.  |dM^-1| is
derived, not fitted (u = 2^-24, gamma(k) = k u / (1 - k u); DESIGN.md section 7 has the same text with the operation counts):

    dt      two subtractions and a division:                              d_dt = gamma(3) |dt|
    T, S    (1 - dt) a + dt b, four roundings on the longest path:        d_T  = gamma(3) (|1 - dt| |a| + |dt| |b|) + |b - a| d_dt
    c       the four-term dot of the quaternions:                          d_c  = gamma(4) sum |R0_i R1_i|
    theta   acosf: d_theta = d_c / sin(theta) + U_ACOS u theta
    w_k     sin(a_k theta) / sin(theta), a_0 = 1 - dt, a_1 = dt.  theta's error enters numerator and denominator together, so it goes
            through the derivative of the quotient, f_k' = (a_k cos(a_k theta) sin(theta) - sin(a_k theta) cos(theta)) / sin^2(theta),
            which stays bounded as theta -> 0 where the two parts alone would not:
                d_w_k = |f_k'| d_theta + |cos(a_k theta)| / sin(theta) (theta d_dt + gamma(2) a_k theta) + |w_k| (2 U_SIN u + u)
    q       (R0 w_0 + R1 w_1) (1 / sin):  d_q_i = |R0_i| d_w_0 + |R1_i| d_w_1 + gamma(3) (|R0_i w_0| + |R1_i w_1|); where |c - (1 - 2^-23)|
            <= d_c the float32 code may take the other side of the early return, and |slerp - R0| is added.
    R       to_matrix's quadratic forms: the off-diagonal 2 (a b +- c d) moves by 2 (|a| d_b + |b| d_a + |c| d_d + |d| d_c) + gamma(3) 2 (|a b|
            + |c d|), the diagonal 1 - 2 (a a + b b) by 4 (|a| d_a + |b| d_b) + gamma(4) (1 + 2 (a a + b b)).
    M       M_ij = R_ij S_j, M_i3 = T_i:  d_M_ij = |S_j| d_R_ij + |R_ij| d_S_j + u |R_ij S_j|,  d_M_i3 = d_T_i.
    M^-1    first order, (M + dM)^-1 - M^-1 = -M^-1 dM M^-1, plus the elimination's own rounding: Gauss-Jordan with full pivoting on a
            4 x 4 does, per entry, four steps of a scaling, a product and a subtraction -- twelve roundings, taken as gamma(16) on the
            usual |M^-1| |M| |M^-1| (Higham, Accuracy and Stability of Numerical Algorithms, section 14.4):
                |dM^-1| <= |M^-1| d_M |M^-1| + gamma(16) |M^-1| |M| |M^-1|.

U_SIN = U_ACOS = 2 ulp.  The kernels evaluate the two functions with pt_sincosf / pt_acosf (pt_device_math.h), restatements of glibc's sinf
and acosf that tools/check_sincosf_port.py and tools/check_atan_acos_port.c hold to libm.so.6 bit for bit; the glibc manual ("Known
Maximum Errors in Math Functions", x86_64) lists 1 ulp for both, and one more is added.

A mirror keeps its sign through the motion in every case here (asserted): geometry_ref takes a group's handedness from one matrix.
"""
import numpy as np

import geometry_ref as G
from helpers import pkg

U = 2.0 ** -24
U_SIN = U_ACOS = 2.0
SLERP_EARLY = 1.0 - 2.0 ** -23          # Quaternion::slerp's T = 1.0 - f32::EPSILON


# ------------------------------------------------------------------------------------------------- decompose.rs, widened to float64
def _inverse64(m):
    """Matrix4x4::inverse: Gauss-Jordan with full pivoting, None where the reference returns None."""
    w = np.array(m, np.float64).reshape(4, 4).copy()
    ipiv = [0] * 4
    indxr, indxc = [0] * 4, [0] * 4
    for i in range(4):
        irow = icol = 0
        big = 0.0
        for j in range(4):
            if ipiv[j] != 1:
                for k in range(4):
                    if ipiv[k] == 0:
                        if abs(w[j, k]) >= big:
                            big, irow, icol = abs(w[j, k]), j, k
                    elif ipiv[k] > 1:
                        return None
        ipiv[icol] += 1
        if irow != icol:
            w[[irow, icol]] = w[[icol, irow]]
        indxr[i], indxc[i] = irow, icol
        if w[icol, icol] == 0.0:
            return None
        pivinv = 1.0 / w[icol, icol]
        w[icol, icol] = 1.0
        w[icol] *= pivinv
        for j in range(4):
            if j != icol:
                save = w[j, icol]
                w[j, icol] = 0.0
                w[j] -= w[icol] * save
    for j in (3, 2, 1, 0):
        if indxr[j] != indxc[j]:
            w[:, [indxr[j], indxc[j]]] = w[:, [indxc[j], indxr[j]]]
    return w


def _quat_new(x, y, z, w):
    return np.array([x, y, z, w]) if w >= 0.0 else np.array([-x, -y, -z, -w])


def _quat_from_matrix(m):
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0.0:
        s = np.sqrt(tr + 1.0) * 2.0
        return _quat_new((m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, s / 4.0)
    if m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2.0
        return _quat_new(s / 4.0, (m[1, 0] + m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s)
    if m[1, 1] > m[2, 2]:
        s = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2.0
        return _quat_new((m[1, 0] + m[0, 1]) / s, s / 4.0, (m[2, 1] + m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s)
    s = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2.0
    return _quat_new((m[0, 2] + m[2, 0]) / s, (m[2, 1] + m[1, 2]) / s, s / 4.0, (m[1, 0] - m[0, 1]) / s)


def _quat_normalize(q):
    q = q / np.sqrt((q * q).sum())
    return _quat_new(*q)


def quat_matrix(q):
    """Quaternion::to_matrix (the transposed form it returns), 3 x 3; q[..., 4] -> [..., 3, 3]."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r = np.empty(q.shape[:-1] + (3, 3))
    r[..., 0, 0] = 1.0 - 2.0 * (y * y + z * z); r[..., 0, 1] = 2.0 * (x * y - w * z); r[..., 0, 2] = 2.0 * (x * z + w * y)
    r[..., 1, 0] = 2.0 * (x * y + w * z); r[..., 1, 1] = 1.0 - 2.0 * (x * x + z * z); r[..., 1, 2] = 2.0 * (y * z - w * x)
    r[..., 2, 0] = 2.0 * (x * z - w * y); r[..., 2, 1] = 2.0 * (y * z + w * x); r[..., 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return r


def _suppress(m):
    r = np.eye(4)
    for i in range(3):
        r[i, i] = m[i, i]
    return r


def decompose64(m, epsilon=float(np.float32(2.0 ** -23) * np.float32(1e2)), max_count=100):
    """decompose() of core/transform/decompose.rs, the same algorithm with every operation in float64: (T, R as x y z w, S), or None."""
    m = np.array(m, np.float32).astype(np.float64).reshape(4, 4)
    T = m[:3, 3].copy()
    mm = m.copy()
    mm[:3, 3] = 0.0
    mm[3, 3] = 1.0
    r = mm.copy()
    for i in range(3):                                  # the column lengths divide the rows, as written
        s = np.sqrt((r[:3, i] ** 2).sum())
        if s != 0.0:
            r[i, :3] /= s
    count, norm = 0, 0.0
    while True:
        if _inverse64(r) is None:
            return None
        r_it = _inverse64(r.T)
        if r_it is None:
            return None
        r_next = 0.5 * r + 0.5 * r_it
        ir_next = _inverse64(r_next)
        if ir_next is None:
            return None
        isc = _inverse64(_suppress(ir_next @ mm))
        if isc is not None:
            r_next = mm @ isc
        rn = np.eye(4)
        rn[:3, :3] = quat_matrix(_quat_normalize(_quat_from_matrix(r_next)))
        norm = max(norm, np.abs(r[:3, :3] - rn[:3, :3]).sum(1).max())       # never reset
        r = rn
        count += 1
        if not (count < max_count and norm > epsilon):
            break
    ir = _inverse64(r)
    if ir is None:
        return None
    s = _suppress(ir @ mm)
    isc = _inverse64(s)
    if isc is not None:
        r = mm @ isc
    return T, _quat_normalize(_quat_from_matrix(r)), np.array([s[0, 0], s[1, 1], s[2, 2]])


# ------------------------------------------------------------------------------------------------------------- AnimatedTransform
def _m32(a):
    return np.array(list(a), np.float32).reshape(4, 4)


class Record:
    """AnimatedTransform::new on the library's own float32 decomposition of the two ends."""

    def __init__(self, m0, inv0, m1, inv1, times):
        self.m = [_m32(m0), _m32(m1)]
        self.inv = [_m32(inv0), _m32(inv1)]
        self.times = np.array(times, np.float32).astype(np.float64)
        self.animated = not (np.array_equal(self.m[0], self.m[1]) and np.array_equal(self.inv[0], self.inv[1]))
        d = [pkg.capi.motion_decompose(m) for m in self.m]
        self.T = [d[0][0].astype(np.float64), d[1][0].astype(np.float64)]
        self.R = [d[0][1].astype(np.float64), d[1][1].astype(np.float64)]
        self.S = [d[0][2].astype(np.float64), d[1][2].astype(np.float64)]
        dot32 = np.float32(0)
        for a, b in zip(d[0][1], d[1][1]):              # Quaternion::dot in float32, as the flip is decided
            dot32 = np.float32(dot32 + np.float32(a * b))
        if dot32 < 0:
            self.R[1] = -self.R[1]

    def m64(self, time):
        """(M64(t) as [n, 4, 4], the entrywise bound on the float32 M(t)'s error as [n, 4, 4]) for the interpolating branch."""
        g = G.gamma
        t = np.asarray(time, np.float64)
        n = len(t)
        t0, t1 = self.times
        dt = (t - t0) / (t1 - t0)
        ddt = g(3) * np.abs(dt)
        a = [1.0 - dt, dt]

        def lerp3(v):
            val = a[0][:, None] * v[0] + a[1][:, None] * v[1]
            err = g(3) * (np.abs(a[0])[:, None] * np.abs(v[0]) + np.abs(a[1])[:, None] * np.abs(v[1])) + np.abs(v[1] - v[0]) * ddt[:, None]
            return val, err
        T, dT = lerp3(self.T)
        S, dS = lerp3(self.S)
        q0, q1 = self.R
        c_raw = float((q0 * q1).sum())
        dc = g(4) * float(np.abs(q0 * q1).sum())
        c = min(max(c_raw, 0.0), 1.0)
        if c > SLERP_EARLY:
            q, dq = np.tile(q0, (n, 1)), np.zeros((n, 4))
            q_other = None
        if c <= SLERP_EARLY or abs(c - SLERP_EARLY) <= dc:
            cc = min(c, 1.0 - 1e-300)
            th = np.arccos(cc)
            sth = np.sin(th) if th > 0 else 1.0
            dth = dc / sth + U_ACOS * U * th
            w, dw = [], []
            for k in range(2):
                arg = a[k] * th
                f = np.sin(arg) / sth if th > 0 else a[k]
                fp = (a[k] * np.cos(arg) * sth - np.sin(arg) * np.cos(th)) / (sth * sth) if th > 0 else np.zeros(n)
                w.append(f)
                dw.append(np.abs(fp) * dth + np.abs(np.cos(arg)) / sth * (th * ddt + g(2) * np.abs(arg)) + np.abs(f) * (2 * U_SIN * U + U))
            qs = w[0][:, None] * q0 + w[1][:, None] * q1
            dqs = (np.abs(q0) * dw[0][:, None] + np.abs(q1) * dw[1][:, None]
                   + g(3) * (np.abs(w[0])[:, None] * np.abs(q0) + np.abs(w[1])[:, None] * np.abs(q1)))
            if c <= SLERP_EARLY:
                q, dq, q_other = qs, dqs, (np.tile(q0, (n, 1)) if abs(c - SLERP_EARLY) <= dc else None)
            else:
                q_other = qs
        if q_other is not None:                          # the float32 dot may fall on the other side of the early return
            dq = dq + np.abs(q_other - q)
        R = quat_matrix(q)
        aq = np.abs(q)
        dR = np.empty((n, 3, 3))
        off = {(0, 1): (0, 1, 3, 2), (0, 2): (0, 2, 3, 1), (1, 0): (0, 1, 3, 2), (1, 2): (1, 2, 3, 0), (2, 0): (0, 2, 3, 1), (2, 1): (1, 2, 3, 0)}
        diag = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
        for (i, j), (p, r, s, v) in off.items():
            dR[:, i, j] = (2.0 * (aq[:, p] * dq[:, r] + aq[:, r] * dq[:, p] + aq[:, s] * dq[:, v] + aq[:, v] * dq[:, s])
                           + g(3) * 2.0 * (aq[:, p] * aq[:, r] + aq[:, s] * aq[:, v]))
        for i, (p, r) in diag.items():
            dR[:, i, i] = 4.0 * (aq[:, p] * dq[:, p] + aq[:, r] * dq[:, r]) + g(4) * (1.0 + 2.0 * (aq[:, p] ** 2 + aq[:, r] ** 2))
        M = np.zeros((n, 4, 4))
        dM = np.zeros((n, 4, 4))
        M[:, :3, :3] = R * S[:, None, :]
        M[:, :3, 3] = T
        M[:, 3, 3] = 1.0
        dM[:, :3, :3] = np.abs(S)[:, None, :] * dR + np.abs(R) * dS[:, None, :] + U * np.abs(M[:, :3, :3])
        dM[:, :3, 3] = dT
        return M, dM

    def world_to_instance(self, time):
        """Per ray: the exact matrix the truth sends it through, [n, 4, 4], and the entrywise bound on the float32 inverse's distance from
        it, [n, 3, 4] (zero on the two clamped branches, where the stored inverse is used as a static instance's is)."""
        t = np.asarray(time, np.float32).astype(np.float64)
        n = len(t)
        W = np.empty((n, 4, 4))
        E = np.zeros((n, 3, 4))
        start = (t <= self.times[0]) | (not self.animated)
        end = ~start & (self.times[1] <= t)
        mid = ~start & ~end
        W[start] = self.inv[0].astype(np.float64)
        W[end] = self.inv[1].astype(np.float64)
        if mid.any():
            M, dM = self.m64(t[mid])
            Wi = np.linalg.inv(M)
            aW = np.abs(Wi)
            Em = aW @ dM @ aW + G.gamma(16) * (aW @ np.abs(M) @ aW)
            W[mid] = Wi
            E[mid] = Em[:, :3, :]
        return W, E

    def instance_to_world(self, time):
        """The exact instance-to-world matrices, [n, 4, 4] (for the bounds' and the camera's checks)."""
        t = np.asarray(time, np.float32).astype(np.float64)
        out = np.empty((len(t), 4, 4))
        start = (t <= self.times[0]) | (not self.animated)
        end = ~start & (self.times[1] <= t)
        mid = ~start & ~end
        out[start] = self.m[0].astype(np.float64)
        out[end] = self.m[1].astype(np.float64)
        if mid.any():
            out[mid] = self.m64(t[mid])[0]
        return out


class PerRay:
    """A link of geometry_ref's chain of world-to-local matrices with one matrix per ray, and the bound on its float32 counterpart."""

    def __init__(self, W, E):
        self.W, self.E = W, E
        s = np.sign(np.linalg.det(W[:, :3, :3]))
        assert (s == s[0]).all(), "an instance changes handedness during its motion"

    def __getitem__(self, key):                          # geometry_ref reads the handedness off chain[0][:3, :3]
        return self.W[0][key]


def _transform_rays(chain, o, d):
    """geometry_ref._transform_rays with PerRay links."""
    n = len(o)
    oerr, derr, shift = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    g = G.gamma
    for m in chain:
        if isinstance(m, PerRay):
            A, tr = m.W[:, :3, :3], m.W[:, :3, 3]
            aA = np.abs(A)
            mul = lambda X, v: np.einsum("nij,nj->ni", X, v)
            oe = g(3) * (mul(aA, np.abs(o)) + np.abs(tr))
            de = g(3) * mul(aA, np.abs(d))
            xo = mul(m.E[:, :, :3], np.abs(o)) + m.E[:, :, 3]          # |dM^-1| on the origin and on the direction
            xd = mul(m.E[:, :, :3], np.abs(d))
            o, d = mul(A, o) + tr, mul(A, d)
            oerr, derr = mul(aA, oerr) + oe + xo, mul(aA, derr) + de + xd
        else:
            A, tr = m[:3, :3], m[:3, 3]
            aA = np.abs(A)
            oe = g(3) * (np.abs(o) @ aA.T + np.abs(tr))
            de = g(3) * (np.abs(d) @ aA.T)
            o, d = o @ A.T + tr, d @ A.T
            oerr, derr = oerr @ aA.T + oe, derr @ aA.T + de
        l2 = (d * d).sum(1)
        dt = np.where(l2 > 0, (np.abs(d) * oe).sum(1) / np.where(l2 > 0, l2, 1.0), 0.0)
        shift = shift + dt
        oerr = oerr + g(2) * (np.abs(o) + np.abs(d) * dt[:, None])
    return o, d, oerr, derr, shift


def records_of(sd):
    """instance index -> Record, for the instances of a scene description that carry a motion record."""
    mo = getattr(sd, "motion", None)
    out = {}
    if mo is None:
        return out
    times = [mo.transform_times[0], mo.transform_times[1]]
    for k in range(mo.n_instances):
        r = mo.instances[k]
        it = sd.buffers["instances"][r.instance]
        out[int(r.instance)] = Record(it.instance_to_world, it.world_to_instance, r.instance_to_world_end, r.world_to_instance_end, times)
    return out


def closest_hits(sd, o, d, tmax, time):
    """geometry_ref.closest_hits for rays that carry a time: every moving instance's group goes through its per-ray matrices."""
    sc = G.Scene(sd)
    for k, rec in records_of(sd).items():
        chain, tri, sph, inst = sc.groups[k + 1]
        assert inst == k
        sc.groups[k + 1] = ([PerRay(*rec.world_to_instance(time))], tri, sph, inst)
    saved = G._transform_rays
    G._transform_rays = _transform_rays
    try:
        return G.closest_hits(sc, o, d, tmax)
    finally:
        G._transform_rays = saved
