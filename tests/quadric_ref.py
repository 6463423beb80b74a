"""Float64 truths for Shape "cylinder" and Shape "disk" (src/shapes/cylinder.rs, src/shapes/disk.rs of the reference), and a float32
restatement of the same two files.

The oracle does not know these shapes, so the truth is numpy alone, built on geometry_ref.py: its Scene (primitive numbering, groups,
instances), its triangles and spheres, its _Best bookkeeping and its four rules of decisiveness.  An analytic shape of kind 1 or 2 in a
scene's "spheres" table is routed to _cylinder / _disk below instead of geometry_ref._sphere; everything else is geometry_ref's.

Cylinder t, absolute.  t is a root of a t^2 + b t + c with a = dx^2 + dy^2, b = 2 (dx ox + dy oy), c = ox^2 + oy^2 - r^2 in object space, so
the sphere's first-order bound holds with the sums over x and y only:
    [2 sum_xy |p_i| (o_err_i + |t| d_err_i) + t^2 da + |t| db + dc] / sqrt(disc) + gamma(6) |t|  +  the origin shift of transform_ray,
with da = gamma(3) a, db = gamma(4) 2 sum|d_i o_i|, dc = gamma(4) (sum o_i^2 + r^2) (one term fewer than the sphere's sums: an upper bound).
The reference's own interval [t.lo, t.hi] is available too (hit_f32 returns it): the float32 restatement's t64 must lie in it widened by the
shift.  Clips: z = o.z + t d.z is not refined, its error is |d.z| B + o_err.z + |t| d_err.z + gamma(3) (|o.z| + |t d.z|); phi's is the
refined point's error over r.  Both wraps of a negative phi are by 2 PI (cylinder.rs:113-115, :135-137), so intersect and intersect_p
agree on every ray.

Disk t.  No intervals in the reference: t = (h - o.z) / d.z on the ray transform_ray returns.  With the exact image (o, d) of the ray:
    |t32 - t64| <= (o_err.z + |t| d_err.z) / |d.z| + gamma(3) |t| + shift
(the transformed components' errors through the quotient; the subtraction, the division and the shifted origin's rounding; the shift
itself, which the reference applies and no shape adds back).  A ray with |d.z| <= 4 d_err.z is left out (rule a) unless d.z and d_err.z
are both exactly zero (an axis-aligned transform and a ray in the plane: a decided miss, disk.rs:60-62).  t <= 0 and t >= t_max reject,
so a t within two bounds of either is rule (c); a point within its bound of the outer or inner rim, the phi seam or phi_max is rule (d).

Light samples (light_truth): Cylinder::sample / Disk::sample and the default Shape::sample_from (shape.rs:20-38) in float64.  The disk is
sampled over its WHOLE disk whatever inner_radius and phi_max say while the density is that of the partial annulus (disk.rs:171-191): the
truth restates this.  pdf = dist^2 / (area |cos|).  The solid angle is a float64 quadrature of |cos| / dist^2 over the surface that is
sampled (both walls of a cylinder count: sample_from keeps back-facing points, their density is that of |cos|).
"""
import numpy as np

import geometry_ref as G
from geometry_ref import EPS, gamma

SHAPE_SPHERE, SHAPE_CYLINDER, SHAPE_DISK = 0, 1, 2
TWO_PI = 2.0 * np.pi


class _Quadric:
    """Cylinder::new / Disk::new: the parameters as the reference holds them, widened to float64."""

    def __init__(self, ps):
        self.kind = int(ps.kind)
        self.o2w, self.w2o = G._mat(ps.object_to_world), G._mat(ps.world_to_object)
        self.r = float(np.float32(ps.radius))
        deg = np.clip(np.float32(ps.phimax), np.float32(0), np.float32(360))
        self.phimax32 = deg * (np.float32(np.pi) / np.float32(180))
        self.phimax = float(self.phimax32)
        self.full_phi = float(deg) >= 360.0
        self.reverse = bool(ps.flags & G.SPHERE_REVERSE)
        self.area_light, self.object = int(ps.area_light), int(ps.object)
        if self.kind == SHAPE_CYLINDER:
            lo, hi = float(np.float32(ps.zmin)), float(np.float32(ps.zmax))
            self.zmin, self.zmax = (hi, lo) if lo > hi else (lo, hi)            # create_cylinder_shape's swap; no clamp
            self.area = (self.zmax - self.zmin) * self.r * self.phimax
        else:
            self.h = float(np.float32(ps.zmin))
            self.ri = float(np.float32(ps.inner_radius))
            self.zmin = self.zmax = self.h
            self.area = self.phimax * 0.5 * (self.r * self.r - self.ri * self.ri)
        self.swaps = np.linalg.det(self.o2w[:3, :3]) < 0


class Scene(G.Scene):
    """geometry_ref.Scene whose table of analytic shapes knows the kinds."""

    def __init__(self, sd):
        super().__init__(sd)
        for i in range(sd.desc.n_spheres):
            if int(sd.buffers["spheres"][i].kind) != SHAPE_SPHERE:
                self.spheres[i] = _Quadric(sd.buffers["spheres"][i])


def _kind(sp):
    return getattr(sp, "kind", SHAPE_SPHERE)


def _cylinder(sp, chain, o_w, d_w, tmax, best, prim, kind_code):
    """Every ray against one cylinder (after geometry_ref._sphere)."""
    o, d, oerr, derr, shift = G._transform_rays(chain + [sp.w2o], o_w, d_w)
    n = len(o)
    r = sp.r
    o2, d2, oe2, de2 = o[:, :2], d[:, :2], oerr[:, :2], derr[:, :2]
    a = (d2 * d2).sum(1); b = 2.0 * (d2 * o2).sum(1); c = (o2 * o2).sum(1) - r * r
    da, db, dc = gamma(3) * a, gamma(4) * 2.0 * np.abs(d2 * o2).sum(1), gamma(4) * ((o2 * o2).sum(1) + r * r)
    disc = b * b - 4.0 * a * c
    with np.errstate(all="ignore"):
        rb = 2.0 * (np.abs(d2) * oe2 + np.abs(o2) * de2).sum(1) + db
        rc = 2.0 * (np.abs(o2) * oe2).sum(1) + dc
        ra = 2.0 * (np.abs(d2) * de2).sum(1) + da
        ddisc = 2.0 * np.abs(b) * rb + 4.0 * np.abs(c) * ra + 4.0 * a * rc
        root = np.sqrt(np.maximum(disc, 0.0))
        q = np.where(b < 0, -0.5 * (b - root), -0.5 * (b + root))
        ta, tb = q / a, c / q
        t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
    has = (disc >= 0) & np.isfinite(t0) & np.isfinite(t1) & (a > 0)
    # a ray exactly parallel to the axis under a transform that keeps it so (a == 0, no error on d.x, d.y): a decided miss
    parallel = (a == 0) & (de2.sum(1) == 0)
    sil = (np.abs(disc) <= 16.0 * ddisc) & ~parallel

    def bound_of(t):
        with np.errstate(all="ignore"):
            p = o + t[:, None] * d
            first = (2.0 * (np.abs(p[:, :2]) * (oe2 + np.abs(t)[:, None] * de2)).sum(1) + t * t * da + np.abs(t) * db + dc) / root + gamma(6) * np.abs(t)
        return first + shift, p

    B0, p0 = bound_of(t0)
    B1, p1 = bound_of(t1)
    dlen = np.sqrt((d * d).sum(1))

    def clip(p, B, t):
        with np.errstate(all="ignore"):
            Bz = np.abs(d[:, 2]) * B + oerr[:, 2] + np.abs(t) * derr[:, 2] + gamma(3) * (np.abs(o[:, 2]) + np.abs(t * d[:, 2]))
            Bp = dlen * B + np.linalg.norm(oe2 + np.abs(t)[:, None] * de2, axis=1) + gamma(8) * r
            raw = np.arctan2(p[:, 1], p[:, 0])
            phi = np.where(raw < 0, raw + TWO_PI, raw)
            Bphi = Bp / r
        rej = (p[:, 2] < sp.zmin) | (p[:, 2] > sp.zmax) | (phi > sp.phimax)
        edge = (np.abs(p[:, 2] - sp.zmin) <= Bz) | (np.abs(p[:, 2] - sp.zmax) <= Bz) | ~np.isfinite(Bz)
        if not sp.full_phi:
            edge |= (np.abs(phi - sp.phimax) <= Bphi) | (np.abs(raw) <= Bphi) | ~np.isfinite(Bphi)
        return rej, edge

    live = has & ~((t0 > tmax) | (t1 <= 0))
    first_is_t1 = t0 <= 0
    live &= ~(first_is_t1 & (t1 > tmax))
    tf, Bf, pf = np.where(first_is_t1, t1, t0), np.where(first_is_t1, B1, B0), np.where(first_is_t1[:, None], p1, p0)
    rej_f, edge_f = clip(pf, Bf, tf)
    retry = live & rej_f & ~first_is_t1 & ~(t1 > tmax)
    rej_s, edge_s = clip(p1, B1, t1)
    ok_first = live & ~rej_f
    ok_second = retry & ~rej_s
    t = np.where(ok_first, tf, np.where(ok_second, t1, np.inf))
    B = np.where(ok_first, Bf, B1)
    edge = (live & edge_f) | (retry & edge_s)
    zone = has & ((np.abs(t0) <= 4.0 * B0) | (np.abs(t1) <= 4.0 * B1) | (np.abs(t0 - tmax) <= 4.0 * B0) | ((first_is_t1 | rej_f) & (np.abs(t1 - tmax) <= 4.0 * B1)))
    rows = np.nonzero(np.isfinite(t) & ~sil)[0]
    best.offer(rows, t=t[rows], bound=B[rows], kind=kind_code, prim=prim, b0=0.0, b1=0.0, bb=0.0, uid=best.next_uid)
    best.next_uid += 1
    best.occ |= np.isfinite(t) & ~sil
    with np.errstate(all="ignore"):
        t_mid = np.where(a > 0, -b / (2.0 * a), 0.0)
        cand = np.where(t0 > -B0, t0 - B0, t1 - B1)
    for rule, mask, tc in ((1, sil & ((t_mid > 0) | (c <= 0)), np.minimum(t_mid, np.where(np.isfinite(cand), cand, np.inf))), (3, zone & (t1 > -4.0 * B1), cand),
                           (4, edge & has, cand)):
        rr = np.nonzero(mask)[0]
        if len(rr):
            best.amb.append((rule, rr, np.where(np.isfinite(tc[rr]), tc[rr], 0.0)))


def _disk(sp, chain, o_w, d_w, tmax, best, prim, kind_code):
    """Every ray against one disk."""
    o, d, oerr, derr, shift = G._transform_rays(chain + [sp.w2o], o_w, d_w)
    r, ri, h = sp.r, sp.ri, sp.h
    dz = d[:, 2]
    with np.errstate(all="ignore"):
        t = (h - o[:, 2]) / dz
        B = (oerr[:, 2] + np.abs(t) * derr[:, 2]) / np.abs(dz) + gamma(3) * np.abs(t) + shift
        p = o + t[:, None] * d
        rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
        Bp = np.sqrt((d * d).sum(1)) * B + np.linalg.norm(oerr + np.abs(t)[:, None] * derr, axis=1) + gamma(6) * (np.abs(o) + np.abs(t[:, None] * d)).sum(1)
        raw = np.arctan2(p[:, 1], p[:, 0])
        phi = np.where(raw < 0, raw + TWO_PI, raw)
        Bphi = Bp / rho
    decided_parallel = (dz == 0) & (derr[:, 2] == 0)
    undecided = (np.abs(dz) <= 4.0 * derr[:, 2]) & ~decided_parallel            # rule (a): the plane is met, if at all, anywhere
    fin = np.isfinite(t) & ~decided_parallel & ~undecided
    rej = (rho > r) | (rho < ri) | (phi > sp.phimax)
    edge = (np.abs(rho - r) <= Bp) | ((ri > 0) & (np.abs(rho - ri) <= Bp))
    if not sp.full_phi:
        edge |= (np.abs(phi - sp.phimax) <= Bphi) | (np.abs(raw) <= Bphi) | (rho <= 4.0 * Bp) | ~np.isfinite(Bphi)
    with np.errstate(all="ignore"):
        acc = fin & (t > 0) & (t < tmax) & ~rej
        zone = fin & ((np.abs(t) <= 2.0 * B) | (np.abs(t - tmax) <= 2.0 * B)) & (~rej | edge)
        in_range = fin & (t > -2.0 * B) & (t < tmax + 2.0 * B)
    rows = np.nonzero(acc)[0]
    best.offer(rows, t=t[rows], bound=B[rows], kind=kind_code, prim=prim, b0=0.0, b1=0.0, bb=0.0, uid=best.next_uid)
    best.next_uid += 1
    best.occ |= acc
    for rule, mask, tc in ((1, undecided, np.zeros(len(t))), (3, zone, t - B), (4, edge & in_range, t - B)):
        rr = np.nonzero(mask)[0]
        if len(rr):
            best.amb.append((rule, rr, np.where(np.isfinite(tc[rr]), tc[rr], 0.0)))


def closest_hits(scene, o, d, tmax):
    """geometry_ref.closest_hits over a scene whose analytic shapes may be cylinders and disks: the same dict of arrays."""
    sc = scene if isinstance(scene, Scene) else Scene(scene)
    o = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
    tmax = np.asarray(tmax, np.float32).astype(np.float64).reshape(-1)
    n = len(o)
    best = G._Best(n)
    differs = np.zeros(n, bool)
    for chain, tri, sph, inst in sc.groups:
        lo, ld, oerr, derr, shift = G._transform_rays(chain, o, d)
        flip = bool(chain) and np.linalg.det(chain[0][:3, :3]) < 0
        if inst is None:
            G._triangles(sc, tri, flip, lo, ld, tmax, oerr, derr, shift, best, lambda t: sc.tri_prim[t], G.TRIANGLE)
        else:
            p = int(sc.instance_prim[inst])
            G._triangles(sc, tri, flip, lo, ld, tmax, oerr, derr, shift, best, lambda t: np.full(len(t), p), G.INSTANCE)
        for i in sph:
            prim, kind = (int(sc.sphere_prim[i]), G.SPHERE) if inst is None else (int(sc.instance_prim[inst]), G.INSTANCE)
            k = _kind(sc.spheres[i])
            if k == SHAPE_SPHERE:
                differs |= G._sphere(sc.spheres[i], chain, o, d, tmax, best, prim, kind)
            elif k == SHAPE_CYLINDER:
                _cylinder(sc.spheres[i], chain, o, d, tmax, best, prim, kind)
            else:
                _disk(sc.spheres[i], chain, o, d, tmax, best, prim, kind)
    hit = np.isfinite(best.t[:, 0])
    t = np.where(hit, best.t[:, 0], 0.0)
    limit = np.where(hit & ~differs, best.t[:, 0] + best.bound[:, 0], tmax)
    rule = np.zeros(n, np.int64)
    for r, rows, tc in best.amb:
        m = tc <= limit[rows]
        rr = rows[m]
        rule[rr] = np.where(rule[rr] == 0, r, rule[rr])
    two = np.isfinite(best.t[:, 1]) & (best.uid[:, 1] != best.uid[:, 0])
    with np.errstate(invalid="ignore"):
        tie = two & (best.t[:, 1] - best.t[:, 0] <= best.bound[:, 0] + best.bound[:, 1])
    rule = np.where((rule == 0) & tie, 2, rule)
    return {"kind": np.where(hit, best.kind[:, 0], G.MISS), "prim": np.where(hit, best.prim[:, 0], -1), "t": t,
            "b0": best.b0[:, 0], "b1": best.b1[:, 0], "bound": best.bound[:, 0], "bound_b": best.bb[:, 0], "occluded": best.occ,
            "rule": rule, "tied_t": best.t[:, 1], "tied_bound": best.bound[:, 1], "tied_prim": best.prim[:, 1]}


def single_shape_hits(sp, o, d, tmax):
    """One shape alone (a _Quadric): the dict of closest_hits with prim 0."""
    o = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
    tmax = np.asarray(tmax, np.float32).astype(np.float64).reshape(-1)
    best = G._Best(len(o))
    (_cylinder if sp.kind == SHAPE_CYLINDER else _disk)(sp, [], o, d, tmax, best, 0, G.SPHERE)
    hit = np.isfinite(best.t[:, 0])
    limit = np.where(hit, best.t[:, 0] + best.bound[:, 0], tmax)
    rule = np.zeros(len(o), np.int64)
    for r, rows, tc in best.amb:
        rr = rows[tc <= limit[rows]]
        rule[rr] = np.where(rule[rr] == 0, r, rule[rr])
    return {"hit": hit, "t": np.where(hit, best.t[:, 0], 0.0), "bound": best.bound[:, 0], "rule": rule, "occluded": best.occ}


# ------------------------------------------------------------------------------------------------- the float32 restatement
F = np.float32
_INF32 = F(np.inf)


def _up(v):
    return np.nextafter(v, _INF32).astype(F)


def _down(v):
    return np.nextafter(v, -_INF32).astype(F)


class EF:
    """core/efloat/efloat.rs over arrays: value, lower and upper bound, float32 throughout."""

    def __init__(self, v, lo, hi):
        self.v, self.lo, self.hi = v, lo, hi

    @staticmethod
    def make(v, err):
        v = np.asarray(v, F); err = np.broadcast_to(np.asarray(err, F), v.shape)
        z = err == 0
        return EF(v, np.where(z, v, _down(v - err)).astype(F), np.where(z, v, _up(v + err)).astype(F))

    def __add__(a, b):
        return EF(a.v + b.v, _down(a.lo + b.lo), _up(a.hi + b.hi))

    def __sub__(a, b):
        return EF(a.v - b.v, _down(a.lo - b.hi), _up(a.hi - b.lo))

    def __mul__(a, b):
        if not isinstance(b, EF):
            b = EF.make(np.full(a.v.shape, b, F), F(0))
        p = [a.lo * b.lo, a.hi * b.lo, a.lo * b.hi, a.hi * b.hi]
        return EF(a.v * b.v, _down(np.fmin(np.fmin(p[0], p[1]), np.fmin(p[2], p[3]))), _up(np.fmax(np.fmax(p[0], p[1]), np.fmax(p[2], p[3]))))

    def __truediv__(a, b):
        q = [a.lo / b.lo, a.hi / b.lo, a.lo / b.hi, a.hi / b.hi]
        lo = _down(np.fmin(np.fmin(q[0], q[1]), np.fmin(q[2], q[3])))
        hi = _up(np.fmax(np.fmax(q[0], q[1]), np.fmax(q[2], q[3])))
        strad = (b.lo < 0) & (b.hi > 0)
        return EF(a.v / b.v, np.where(strad, -_INF32, lo).astype(F), np.where(strad, _INF32, hi).astype(F))


def _where_ef(m, a, b):
    return EF(np.where(m, a.v, b.v), np.where(m, a.lo, b.lo), np.where(m, a.hi, b.hi))


def _ef_quadratic(a, b, c):
    av, bv, cv = a.v.astype(np.float64), b.v.astype(np.float64), c.v.astype(np.float64)
    discrim = bv * bv - 4.0 * av * cv
    ok = ~(discrim < 0)
    root = np.sqrt(np.where(ok, discrim, 0.0))
    frd = EF.make(root.astype(F), (2.220446049250313e-16 * root).astype(F))
    q = _where_ef(b.v < 0, (b - frd) * F(-0.5), (b + frd) * F(-0.5))
    r0, r1 = q / a, c / q
    sw = r0.v <= r1.v
    return ok, _where_ef(sw, r0, r1), _where_ef(sw, r1, r0)


def transform_ray_f32(w2o, o, d):
    """Transform::transform_ray (transform.rs:184-203, :245-282): the shifted origin, the direction and the two error vectors."""
    m = np.asarray(w2o, F)
    o = np.asarray(o, F); d = np.asarray(d, F)
    g3 = F(gamma(3))
    ox = [m[i, 0] * o[:, 0] + m[i, 1] * o[:, 1] + m[i, 2] * o[:, 2] + m[i, 3] for i in range(3)]
    oe = [g3 * (np.abs(m[i, 0] * o[:, 0]) + np.abs(m[i, 1] * o[:, 1]) + np.abs(m[i, 2] * o[:, 2]) + np.abs(m[i, 3])) for i in range(3)]
    dx = [m[i, 0] * d[:, 0] + m[i, 1] * d[:, 1] + m[i, 2] * d[:, 2] for i in range(3)]
    de = [g3 * (np.abs(m[i, 0] * d[:, 0]) + np.abs(m[i, 1] * d[:, 1]) + np.abs(m[i, 2] * d[:, 2])) for i in range(3)]
    ls = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]
    with np.errstate(all="ignore"):
        dt = (np.abs(dx[0]) * oe[0] + np.abs(dx[1]) * oe[1] + np.abs(dx[2]) * oe[2]) / ls
    pos = ls > 0
    ox = [np.where(pos, ox[i] + dx[i] * dt, ox[i]).astype(F) for i in range(3)]
    return ox, dx, oe, de


def hit_f32(sp, o, d, tmax):
    """Cylinder::intersect / Disk::intersect up to the clips, restated in float32 operation for operation (intersect_p is the same
    test in both files).  Returns (hit, t, t_lo, t_hi, p_hit, phi): the reference's interval for a cylinder, t itself for a disk."""
    tmax = np.asarray(tmax, F)
    O, D, oe, de = transform_ray_f32(sp.w2o, o, d)
    n = len(tmax)
    r = F(sp.r)
    phimax = sp.phimax32
    two_pi = F(2.0) * F(np.pi)
    with np.errstate(all="ignore"):
        if sp.kind == SHAPE_DISK:
            h, ri = F(sp.h), F(sp.ri)
            t = (h - O[2]) / D[2]
            ok = ~(D[2] == 0) & ~((t <= 0) | (t >= tmax))
            p = [O[i] + D[i] * t for i in range(3)]
            dist2 = p[0] * p[0] + p[1] * p[1]
            ok &= ~((dist2 > r * r) | (dist2 < ri * ri))
            phi = np.arctan2(p[1], p[0]).astype(F)
            phi = np.where(phi < 0, phi + two_pi, phi).astype(F)
            ok &= ~(phi > phimax)
            return ok, t, t, t, p, phi
        ox, oy = EF.make(O[0], oe[0]), EF.make(O[1], oe[1])
        dx, dy = EF.make(D[0], de[0]), EF.make(D[1], de[1])
        rad = EF.make(np.full(n, r, F), F(0))
        a = dx * dx + dy * dy
        b = (dx * ox + dy * oy) * F(2.0)
        c = ox * ox + oy * oy - rad * rad
        ok, t0, t1 = _ef_quadratic(a, b, c)
        ok &= ~(np.isinf(t0.v) | np.isinf(t1.v))
        ok &= ~((t0.hi > tmax) | (t1.lo <= 0))
        use1 = t0.lo <= 0
        th = _where_ef(use1, t1, t0)
        ok &= ~(use1 & (tmax < th.hi))

        def refine(t):
            p = [O[i] + D[i] * t for i in range(3)]
            hr = np.sqrt(p[0] * p[0] + p[1] * p[1])
            p[0] = p[0] * (r / hr); p[1] = p[1] * (r / hr)
            phi = np.arctan2(p[1], p[0]).astype(F)
            return p, np.where(phi < 0, phi + two_pi, phi).astype(F)

        zmin, zmax = F(sp.zmin), F(sp.zmax)
        p, phi = refine(th.v)
        clipped = (p[2] < zmin) | (p[2] > zmax) | (phi > phimax)
        same = (th.v == t1.v) & (th.lo == t1.lo) & (th.hi == t1.hi)
        ok &= ~(clipped & (same | (t1.hi > tmax)))
        p1, phi1 = refine(t1.v)
        clipped1 = (p1[2] < zmin) | (p1[2] > zmax) | (phi1 > phimax)
        ok &= ~(clipped & clipped1)
        th = _where_ef(clipped, t1, th)
        p = [np.where(clipped, p1[i], p[i]) for i in range(3)]
        phi = np.where(clipped, phi1, phi)
        return ok, th.v, th.lo, th.hi, p, phi


# ------------------------------------------------------------------------------------------------------------- area lights
def _concentric(u):
    ox, oy = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
    with np.errstate(all="ignore"):
        first = np.abs(ox) > np.abs(oy)
        rr = np.where(first, ox, oy)
        theta = np.where(first, (np.pi / 4) * (oy / ox), np.pi / 2 - (np.pi / 4) * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    return np.where(zero, 0.0, rr * np.cos(theta)), np.where(zero, 0.0, rr * np.sin(theta))


def sample_points(sp, u):
    """Cylinder::sample / Disk::sample in float64: world point, world normal, the object-space point."""
    u = np.asarray(u, np.float64).reshape(-1, 2)
    if sp.kind == SHAPE_CYLINDER:
        z = (1.0 - u[:, 0]) * sp.zmin + u[:, 0] * sp.zmax
        phi = u[:, 1] * sp.phimax
        po = np.stack([sp.r * np.cos(phi), sp.r * np.sin(phi), z], 1)
        no = np.stack([po[:, 0], po[:, 1], np.zeros(len(u))], 1)
    else:
        x, y = _concentric(u)
        po = np.stack([x * sp.r, y * sp.r, np.full(len(u), sp.h)], 1)
        no = np.repeat(np.array([[0.0, 0.0, 1.0]]), len(u), 0)
    nn = no @ sp.w2o[:3, :3]                                  # transform_normal: the inverse's transpose
    nn = nn / np.linalg.norm(nn, axis=1)[:, None]
    if sp.reverse:
        nn = -nn
    return po @ sp.o2w[:3, :3].T + sp.o2w[:3, 3], nn, po


def surface_quadrature(sp, ref, k=1024):
    """The integral of |cos| / dist^2 over the surface Shape::sample covers, midpoint rule on a k x k grid of its own parameters
    (z, phi for the cylinder; rho, phi of the whole disk), in world space."""
    g = (np.arange(k) + 0.5) / k
    o2w = sp.o2w
    A = o2w[:3, :3]
    if sp.kind == SHAPE_CYLINDER:
        z = sp.zmin + g * (sp.zmax - sp.zmin)
        phi = g * sp.phimax
        Z, PH = np.meshgrid(z, phi, indexing="ij")
        po = np.stack([sp.r * np.cos(PH), sp.r * np.sin(PH), Z], -1).reshape(-1, 3)
        dpa = np.stack([-sp.r * np.sin(PH), sp.r * np.cos(PH), np.zeros_like(PH)], -1).reshape(-1, 3) * sp.phimax
        dpb = np.repeat(np.array([[0.0, 0.0, sp.zmax - sp.zmin]]), len(po), 0)
    else:
        rho = g * sp.r
        phi = g * TWO_PI
        R, PH = np.meshgrid(rho, phi, indexing="ij")
        po = np.stack([R * np.cos(PH), R * np.sin(PH), np.full_like(R, sp.h)], -1).reshape(-1, 3)
        dpa = np.stack([np.cos(PH), np.sin(PH), np.zeros_like(PH)], -1).reshape(-1, 3) * sp.r
        dpb = np.stack([-R * np.sin(PH), R * np.cos(PH), np.zeros_like(PH)], -1).reshape(-1, 3) * TWO_PI
    pw = po @ A.T + o2w[:3, 3]
    nw = np.cross(dpa @ A.T, dpb @ A.T)                        # the world-space area element (a vector), per unit parameter square
    w = pw - np.asarray(ref, np.float64)
    dist2 = (w * w).sum(1)
    return float((np.abs((nw * w).sum(1)) / dist2 ** 1.5).sum() / (k * k))


def light_truth(scene, light, ref_p, u, quadrature=True):
    """DiffuseAreaLight::sample_li over a cylinder or a disk: the dict of geometry_ref.light_truth (solid_angle: the quadrature of
    the sampled surface, one per reference point; branch "cylinder" / "disk")."""
    sc = scene if isinstance(scene, Scene) else Scene(scene)
    kind, idx, L, two_sided_light = sc.lights()[light]
    sp = sc.spheres[idx]
    assert kind == G.SPHERE and _kind(sp) != SHAPE_SPHERE
    u = np.asarray(u, np.float32).astype(np.float64).reshape(-1, 2)
    ref = np.asarray(ref_p, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(u)
    if len(ref) == 1:
        ref = np.repeat(ref, n, 0)
    with np.errstate(all="ignore"):
        p, nn, po = sample_points(sp, u)
        w = p - ref
        dist2 = (w * w).sum(1)
        wi = w / np.sqrt(dist2)[:, None]
        cos = -(nn * wi).sum(1)
        pdf = dist2 / (sp.area * np.abs(cos))
        valid = (dist2 > 0) & (pdf > 0) & np.isfinite(pdf)
        # the float32 point: the lerp or the concentric map, sin / cos, the reprojection and the matrix, each a few ulp of the
        # components' magnitudes (gamma(12) of them in all, as geometry_ref takes for Sphere::sample)
        p_bound = gamma(12) * np.linalg.norm(np.abs(po) @ np.abs(sp.o2w[:3, :3]).T + np.abs(sp.o2w[:3, 3]), axis=1)
        # the area (a few products), dist^2, and the cosine, whose absolute error is that of wi and n and weighs 1 / |cos|
        pdf_rel = gamma(24) + gamma(16) / np.abs(cos) + 4.0 * p_bound / np.sqrt(dist2) / np.abs(cos)
    li = np.where((two_sided_light | (cos > 0))[:, None], L[None, :], 0.0)
    sa = np.full(n, np.nan)
    for i in range(n if quadrature else 0):
        sa[i] = sa[i - 1] if i and np.array_equal(ref[i], ref[i - 1]) else surface_quadrature(sp, ref[i])
    branch = np.empty(n, object)
    branch[:] = "cylinder" if sp.kind == SHAPE_CYLINDER else "disk"
    return {"p": p, "wi": wi, "pdf": np.where(valid, pdf, 0.0), "li": li, "valid": valid, "p_bound": p_bound, "pdf_rel": pdf_rel,
            "solid_angle": sa, "branch": branch, "cos": cos, "dist": np.sqrt(dist2)}


# ------------------------------------------------------------------------------------------------------------- interactions
def interaction(sp, o, d, dtype=np.float64, t=None):
    """The object-space half of Cylinder::intersect / Disk::intersect after the hit (cylinder.rs:143-174, disk.rs:87-104) and
    transform_surface_interaction: world p, n, uv, dpdu, dpdv, dndu, dndv.  dtype float64: the truth (exact image of the ray; the root is
    `t` where given -- the truth's, from single_shape_hits -- else the first positive one, no clip retry).  Plain float64 values; the
    same interaction with a bound beside every value, in either dtype, is interaction_E below."""
    assert dtype == np.float64
    T = dtype
    o64 = np.asarray(o, np.float32).astype(np.float64); d64 = np.asarray(d, np.float32).astype(np.float64)
    O = o64 @ sp.w2o[:3, :3].T + sp.w2o[:3, 3]; D = d64 @ sp.w2o[:3, :3].T
    if t is not None:
        t = np.asarray(t, np.float64)
        p = O + t[:, None] * D
        if sp.kind == SHAPE_CYLINDER:
            p[:, :2] *= (sp.r / np.sqrt((p[:, :2] ** 2).sum(1)))[:, None]
    elif sp.kind == SHAPE_DISK:
        t = (sp.h - O[:, 2]) / D[:, 2]
        p = O + t[:, None] * D
    else:
        a = (D[:, :2] ** 2).sum(1); b = 2.0 * (D[:, :2] * O[:, :2]).sum(1); c = (O[:, :2] ** 2).sum(1) - sp.r ** 2
        root = np.sqrt(np.maximum(b * b - 4 * a * c, 0.0))
        q = np.where(b < 0, -0.5 * (b - root), -0.5 * (b + root))
        t0, t1 = np.minimum(q / a, c / q), np.maximum(q / a, c / q)
        t = np.where(t0 > 0, t0, t1)
        p = O + t[:, None] * D
        p[:, :2] *= (sp.r / np.sqrt((p[:, :2] ** 2).sum(1)))[:, None]
    raw = np.arctan2(p[:, 1], p[:, 0])
    phi = np.where(raw < 0, raw + TWO_PI, raw)
    ok = np.ones(len(t), bool)
    phimax = sp.phimax
    r = T(sp.r)
    zero = np.zeros(len(t), T)
    with np.errstate(all="ignore"):
        if sp.kind == SHAPE_CYLINDER:
            zmin, zmax = T(sp.zmin), T(sp.zmax)
            uv = np.stack([phi / phimax, (p[:, 2] - zmin) / (zmax - zmin)], 1)
            dpdu = np.stack([-phimax * p[:, 1], phimax * p[:, 0], zero], 1)
            dpdv = np.stack([zero, zero, zero + (zmax - zmin)], 1)
            nn = np.cross(dpdu, dpdv)
            nn = nn / np.sqrt((nn * nn).sum(1))[:, None]
            if sp.reverse ^ bool(sp.swaps):
                nn = -nn
            d2pduu = (-phimax * phimax) * np.stack([p[:, 0], p[:, 1], zero], 1)
            E, Fq, Gq = (dpdu * dpdu).sum(1), (dpdu * dpdv).sum(1), (dpdv * dpdv).sum(1)
            e = (nn * d2pduu).sum(1)
            inv = 1 / (E * Gq - Fq * Fq)
            dndu = dpdu * ((0 * Fq - e * Gq) * inv)[:, None] + dpdv * ((e * Fq - 0 * E) * inv)[:, None]
            dndv = np.zeros_like(dndu)
        else:
            ri = T(sp.ri)
            rh = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
            uv = np.stack([phi / phimax, (r - rh) / (r - ri)], 1)
            dpdu = np.stack([-phimax * p[:, 1], phimax * p[:, 0], zero], 1)
            dpdv = np.stack([p[:, 0], p[:, 1], zero], 1) * ((ri - r) / rh)[:, None]
            nn = np.cross(dpdu, dpdv)
            nn = nn / np.sqrt((nn * nn).sum(1))[:, None]
            if sp.reverse ^ bool(sp.swaps):
                nn = -nn
            nn = np.where(((D * nn).sum(1) > 0)[:, None], -nn, nn)
            p = p.copy(); p[:, 2] = T(sp.h)
            dndu = np.zeros_like(dpdu); dndv = np.zeros_like(dpdu)
        A, Ai = sp.o2w[:3, :3].astype(T), sp.w2o[:3, :3].astype(T)
        pw = p @ A.T + sp.o2w[:3, 3].astype(T)
        nw = nn @ Ai
        nw = nw / np.sqrt((nw * nw).sum(1))[:, None]
    return {"ok": ok, "t": t, "p": pw, "n": nw, "uv": uv, "dpdu": dpdu @ A.T, "dpdv": dpdv @ A.T, "dndu": dndu @ Ai, "dndv": dndv @ Ai}


# ------------------------------------------------------- the interaction with a bound per value (aov_ref's E arithmetic)
def interaction_E(ps, o, d, t, dtype, und):
    """Cylinder::intersect / Disk::intersect after the hit (cylinder.rs:143-174, disk.rs:87-104) and transform_surface_interaction, as
    aov_ref._sphere does it for the sphere: every value with a first-order bound carried beside it (aov_ref.E).  ps: the pt_sphere record;
    o, d: E vectors of the world ray; t: E (the truth's t with its bound, or a float32 t with none).  Returns aov_ref's interaction dict
    (p, uv, n, dpdu, dpdv, sh_n, sh_dpdu, sh_dpdv, sh_dndu, sh_dndv); und collects undecided branches (the phi seam, the side of a disk
    the ray is on)."""
    import aov_ref as R
    sp = _Quadric(ps)
    n = len(t.v)
    w2o, o2w = R.mat(ps.world_to_object, n, dtype), R.mat(ps.object_to_world, n, dtype)
    oo, dd = R.xpoint(w2o, o), R.xvec(w2o, d)
    r = R.const(sp.r, n, dtype)
    zero = R.const(0.0, n, dtype)
    ph = R.vadd(oo, R.vscale(dd, t))
    if sp.kind == SHAPE_CYLINDER:
        hr = (ph[0] * ph[0] + ph[1] * ph[1]).sqrt()
        ph = [ph[0] * (r / hr), ph[1] * (r / hr), ph[2]]
    raw = R.atan2(ph[1], ph[0])
    und |= np.abs(raw.v) <= raw.e
    phi = R.where(raw.v < 0, raw + R.const(float(np.float32(2 * np.pi)), n, dtype), raw)
    phimax = R.const(sp.phimax, n, dtype)
    dpdu = [-(phimax * ph[1]), phimax * ph[0], zero]
    flip = bool(sp.reverse) ^ bool(sp.swaps)
    if sp.kind == SHAPE_CYLINDER:
        zmin, zmax = R.const(sp.zmin, n, dtype), R.const(sp.zmax, n, dtype)
        uv = [phi / phimax, (ph[2] - zmin) / (zmax - zmin)]
        dpdv = [zero, zero, zmax - zmin]
        d2pduu = R.vscale([ph[0], ph[1], zero], -(phimax * phimax))
        d2pduv = d2pdvv = [zero, zero, zero]
        EE, FF, GG = R.vdot(dpdu, dpdu), R.vdot(dpdu, dpdv), R.vdot(dpdv, dpdv)
        nn = R.vnorm(R.vcross(dpdu, dpdv))
        if flip:
            nn = R.vneg(nn)
        ee, ff, gg = R.vdot(nn, d2pduu), R.vdot(nn, d2pduv), R.vdot(nn, d2pdvv)
        inv = 1.0 / (EE * GG - FF * FF)
        dndu = R.vadd(R.vscale(dpdu, (ff * FF - ee * GG) * inv), R.vscale(dpdv, (ee * FF - ff * EE) * inv))
        dndv = R.vadd(R.vscale(dpdu, (gg * FF - ff * GG) * inv), R.vscale(dpdv, (ff * FF - gg * EE) * inv))
    else:
        ri = R.const(sp.ri, n, dtype)
        rh = (ph[0] * ph[0] + ph[1] * ph[1]).sqrt()
        uv = [phi / phimax, (r - rh) / (r - ri)]
        dpdv = R.vscale([ph[0], ph[1], zero], (ri - r) / rh)
        nn = R.vnorm(R.vcross(dpdu, dpdv))
        if flip:
            nn = R.vneg(nn)
        side = R.vdot(dd, nn)
        und |= np.abs(side.v) <= side.e
        nn = R.vwhere(side.v > 0, R.vneg(nn), nn)
        ph = [ph[0], ph[1], R.const(sp.h, n, dtype)]
        dndu = dndv = [zero, zero, zero]
    nw = R.vnorm(R.xnormal(w2o, nn))
    dpdu_w, dpdv_w = R.xvec(o2w, dpdu), R.xvec(o2w, dpdv)
    return {"p": R.xpoint(o2w, ph), "uv": uv, "n": nw, "dpdu": dpdu_w, "dpdv": dpdv_w, "sh_n": nw, "sh_dpdu": dpdu_w, "sh_dpdv": dpdv_w,
            "sh_dndu": R.xnormal(w2o, dndu), "sh_dndv": R.xnormal(w2o, dndv)}


# ---------------------------------------------------------------------------------------------------------------- pdf_from
def pdf_from(scene, light, ref_p, wi):
    """The default Shape::pdf_from (shape.rs:40-54) of an area light on a cylinder or a disk, in float64: the shape's own intersect along wi
    from the bare point ref_p, then dist^2 / (|n . -wi| area), infinite -> 0, a miss -> 0.  Returns a dict: pdf, hit, rule (the truth's
    decisiveness of the intersection: a direction that meets a rim or grazes is left out), pdf_rel (the relative bound: the hit point moves
    by the t bound along the ray and by the point's own error, which dist^2 takes twice over dist and the cosine once over |cos|; the normal,
    the area and the quotient add gamma(24)), cos."""
    sc = scene if isinstance(scene, Scene) else Scene(scene)
    kind, idx, L, two_sided = sc.lights()[light]
    sp = sc.spheres[idx]
    assert kind == G.SPHERE and _kind(sp) != SHAPE_SPHERE
    wi = np.asarray(wi, np.float32).astype(np.float64).reshape(-1, 3)
    ref = np.asarray(ref_p, np.float32).astype(np.float64).reshape(-1, 3)
    if len(ref) == 1:
        ref = np.repeat(ref, len(wi), 0)
    tr = single_shape_hits(sp, ref, wi, np.full(len(wi), np.inf))
    with np.errstate(all="ignore"):
        it = interaction(sp, ref, wi, np.float64, t=tr["t"])
        w = it["p"] - ref
        dist2 = (w * w).sum(1)
        cos = -(it["n"] * wi).sum(1)                 # wi as it is given: the reference takes it for a unit vector (shape.rs:46)
        pdf = dist2 / (np.abs(cos) * sp.area)
        pdf = np.where(tr["hit"] & np.isfinite(pdf), pdf, 0.0)
        dp = np.linalg.norm(wi, axis=1) * tr["bound"] + gamma(12) * np.linalg.norm(np.abs(it["p"]) + np.abs(sp.o2w[:3, 3]), axis=1)
        # the cylinder's object normal is the radial unit vector: it turns by the object-space point error over r, and the normalised
        # transform by the inverse's transpose at most doubles that times the matrix's condition
        si, so = np.linalg.norm(sp.w2o[:3, :3], 2), np.linalg.norm(sp.o2w[:3, :3], 2)
        dn = 2.0 * si * si * so * dp / sp.r if sp.kind == SHAPE_CYLINDER else 0.0
        rel = gamma(24) + 2.0 * dp / np.sqrt(dist2) + (dn + gamma(16)) / np.abs(cos)
    return {"pdf": pdf, "hit": tr["hit"], "rule": tr["rule"], "pdf_rel": rel, "cos": cos, "p": it["p"], "dist": np.sqrt(dist2)}
