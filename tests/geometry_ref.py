"""Float64 truths for the geometric results: closest hit, occlusion and area-light samples.

Independent of the oracle and of the product: numpy only, brute force over every primitive, no tree and no order table.  The
inputs are the scene description's own float32 buffers (sd.buffers["P"], ["indices"], ["tri_mesh"], ["meshes"], ["spheres"],
["instances"], ["area_lights"]; the pt_sphere / pt_instance / pt_mesh fields of capi.py), widened exactly to float64.

What is computed (closest_hits):

  * Triangles: the watertight test's sheared-space edge functions (shapes/triangle.rs:240-347) in float64, one ray against every
    triangle.  A degenerate triangle (get_dpdu_dpdv fails in the reference) is not modelled: the builders drop them.
  * Spheres: the quadratic of the ray's float64 image under world_to_object with the z and phi clips (shapes/sphere.rs:61-131 and
    :198-269).  Q58: `intersect` wraps a negative phi of the SECOND root by PI, not 2 PI (sphere.rs:121-124); `intersect_p` wraps
    both by 2 PI.  The truth restates this: the closest-hit and the any-hit acceptance of a clipped sphere's far side differ.
  * Instances: the ray's exact float64 image under world_to_instance meets the object's primitives in object space -- the same
    set of points as flattening the object's geometry to world space by the exact inverse (the reference transforms the ray with
    the stored inverse, transformed_primitive.rs:26-45; the map is affine, so t is the same number) -- and the reference's
    delta_t is evaluated on the quantities it is defined on.  An analytic sphere inside an instance stays analytic: the two
    transforms compose.

Bounds, per evaluation (|device t - t64| <= bound is what the tests assert):

  * Triangle t: the reference's own delta_t (triangle.rs:328-344: gamma(3), gamma(5), delta_e, max_e, |inv_det|) in float64.
  * Triangle barycentrics.  b_i = e_i / det, det = e0 + e1 + e2.  The reference's delta_e bounds each computed edge function's
    distance from the exact one, so the computed det is off by at most 3 delta_e plus the two additions' roundings
    (gamma(2) sum|e_i|, and sum|e_i| = |det| for a ray inside the triangle).  With e_i = b_i det:
        |b_i' - b_i| <= (delta_e + |b_i| (3 delta_e + gamma(2) |det|)) / |det| + gamma(3) |b_i|      (the reciprocal, the product)
                     <= delta_e (1 + 3 |b_i|) / |det| + gamma(5) |b_i|  =: bound_b.
  * Sphere t, absolute.  t is a root of a t^2 + b t + c with a = d.d, b = 2 d.o, c = o.o - r^2, and 2 a t + b = +-sqrt(disc), so
    to first order  dt/do_i = -2 p_i / (2 a t + b),  dt/dd_i = -2 t p_i / (2 a t + b)  with p = o + t d.  Two terms:
      (1) transform_ray's error terms o_err, d_err (gamma(3) sums, transform.rs:184-282), the rounding of the shifted origin
          and of the coefficients (gamma(3) sum d_i^2, gamma(4) 2 sum|d_i o_i|, gamma(4) (sum o_i^2 + r^2)) through that:
             [2 sum|p_i| (o_err_i + |t| d_err_i) + t^2 da + |t| db + dc] / sqrt(disc) + gamma(6) |t|;
      (2) the origin shift dt = dot(|d|, o_err) / |d|^2 that transform_ray applies and no shape adds back: the returned t is
          measured from the shifted origin.  This is the reference's behaviour (quirk Q57), so the bound holds it in full.
    A ray that enters an instance takes the shift once more, and its o_err / d_err are carried through the second matrix.
    The first-order form needs disc well above its own error; where it is not, the ray grazes the silhouette (rule a).
  * Triangles inside an instance: delta_t plus the plane form of (1), (|n|.o_err + |t| |n|.d_err) / |n.d|, plus the shift (2).

Decisiveness.  A ray is left out of a comparison, and the rule that fired is returned, when within the part of the ray that
matters (up to the closest hit plus its bound; up to t_max for a ray that hits nothing)
  (a) it meets a triangle's plane with a barycentric within max(1e-5, bound_b) of zero while no barycentric is further outside
      than that (an edge graze), or a sphere with |disc| below 16 times its error (a silhouette graze), or a one-sided triangle
      edge-on;
  (b) the two nearest hits lie on distinct primitives and closer than the sum of their bounds (ties, coincident faces);
  (c) a candidate's t is within its bound of t_max, or in (0, 2 bound] (the reference rejects t <= delta_t; a triangle met at
      t64 <= 0 is a decided miss, since the float32 t then cannot exceed delta_t -- rays that start on a surface are decided
      for the half of them that round to behind it), or for a sphere a root in the conservative zone around zero / t_max that
      the reference's intervals straddle (4 bounds);
  (d) a sphere root's point is within its bound of a z or phi clip edge or of the pole axis.

Area lights (light_truth): the float64 image of u under the reference's mapping (uniform_sample_triangle; Sphere::sample inside,
the cone form outside with the sin^2 theta_max < 0.00068523 branch), the exact solid-angle density there, Li by facing and
two-sidedness, and the solid angle the light subtends (Van Oosterom-Strackee; 2 pi (1 - cos theta_max)).  Q59: seen from outside,
Sphere::sample_from samples the WORLD sphere of the shape's radius around the transformed centre (sphere.rs:327-377), which is
the shape only under a rigid transform; the inside test uses the same world sphere.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

THREADS = max(1, min(16, os.cpu_count() or 1))
EPS = 2.0 ** -24
BARY_MARGIN = 1e-5
MISS, TRIANGLE, SPHERE, INSTANCE = 0, 1, 2, 3
RULES = ("", "a", "b", "c", "d")

MESH_TWO_SIDED, MESH_REVERSE, MESH_SWAPS, MESH_HAS_N = 1, 2, 4, 8
SPHERE_REVERSE = 1


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


def _mat(a):
    return np.array(list(a), np.float32).astype(np.float64).reshape(4, 4)


# --------------------------------------------------------------------------------------------------------------- the scene
class _Sphere:
    def __init__(self, ps):
        self.o2w, self.w2o = _mat(ps.object_to_world), _mat(ps.world_to_object)
        r = np.float32(ps.radius)
        zlo, zhi = np.float32(min(ps.zmin, ps.zmax)), np.float32(max(ps.zmin, ps.zmax))
        self.r = float(r)
        self.zmin, self.zmax = float(np.clip(zlo, -r, r)), float(np.clip(zhi, -r, r))          # sphere.rs:35-36
        deg = np.clip(np.float32(ps.phimax), np.float32(0), np.float32(360))
        self.phimax = float(deg * (np.float32(np.pi) / np.float32(180)))                        # radians(), in float32 as the reference
        self.full_phi = float(deg) >= 360.0
        self.reverse = bool(ps.flags & SPHERE_REVERSE)
        self.area_light, self.object = int(ps.area_light), int(ps.object)


class Scene:
    """The primitives of a scene description as float64 arrays, and the world primitive list's numbering."""

    def __init__(self, sd):
        d = sd.desc
        self.P = np.asarray(sd.buffers["P"], np.float32).astype(np.float64).reshape(-1, 3)
        self.N = np.asarray(sd.buffers["N"], np.float32).astype(np.float64).reshape(-1, 3) if "N" in sd.buffers else None
        self.idx = np.asarray(sd.buffers["indices"]).astype(np.int64).reshape(-1, 3)
        tri_mesh = np.asarray(sd.buffers["tri_mesh"]).astype(np.int64).reshape(-1)
        meshes = sd.buffers["meshes"]
        mflags = np.array([meshes[i].flags for i in range(d.n_meshes)], np.int64)
        mobject = np.array([meshes[i].object for i in range(d.n_meshes)], np.int64)
        mlight = np.array([meshes[i].area_light for i in range(d.n_meshes)], np.int64)
        nt = len(self.idx)
        self.tri_flags = mflags[tri_mesh] if nt else np.zeros(0, np.int64)
        self.tri_object = mobject[tri_mesh] if nt else np.zeros(0, np.int64)
        self.tri_light = mlight[tri_mesh] if nt else np.zeros(0, np.int64)
        self.spheres = [_Sphere(sd.buffers["spheres"][i]) for i in range(d.n_spheres)]
        ins = [sd.buffers["instances"][i] for i in range(d.n_instances)]
        self.instances = [(_mat(i.world_to_instance), int(i.object)) for i in ins]
        self.area_lights = [(np.array(list(sd.buffers["area_lights"][i].L), np.float32).astype(np.float64), bool(sd.buffers["area_lights"][i].two_sided))
                            for i in range(d.n_area_lights)]
        # the world's primitive list: spheres and instances spliced in before triangle `before_triangle`, ties in creation order
        extra = [(int(sd.buffers["spheres"][i].before_triangle), int(sd.buffers["spheres"][i].order), SPHERE, i)
                 for i in range(d.n_spheres) if self.spheres[i].object == 0]
        extra += [(int(ins[i].before_triangle), int(ins[i].order), INSTANCE, i) for i in range(d.n_instances)]
        extra.sort(key=lambda e: (e[0], e[1]))
        self.tri_prim = np.full(nt, -1, np.int64)
        self.sphere_prim = np.full(len(self.spheres), -1, np.int64)
        self.instance_prim = np.full(len(self.instances), -1, np.int64)
        self.prim_list = []                     # (kind, index) per world primitive
        e = 0
        for t in range(nt + 1):
            while e < len(extra) and extra[e][0] <= t:
                (self.sphere_prim if extra[e][2] == SPHERE else self.instance_prim)[extra[e][3]] = len(self.prim_list)
                self.prim_list.append((extra[e][2], extra[e][3]))
                e += 1
            if t < nt and self.tri_object[t] == 0:
                self.tri_prim[t] = len(self.prim_list)
                self.prim_list.append((TRIANGLE, t))
        # groups: (chain of world-to-local matrices, triangle indices, sphere indices, world prim per member or the instance's)
        self.groups = [([], np.nonzero(self.tri_object == 0)[0], [i for i, s in enumerate(self.spheres) if s.object == 0], None)]
        for k, (w2i, obj) in enumerate(self.instances):
            self.groups.append(([w2i], np.nonzero(self.tri_object == obj + 1)[0], [i for i, s in enumerate(self.spheres) if s.object == obj + 1], k))

    def lights(self):
        """One area light per emissive world primitive, in primitive order: (kind, index, L, light two-sided)."""
        out = []
        for kind, i in self.prim_list:
            al = self.tri_light[i] if kind == TRIANGLE else (self.spheres[i].area_light if kind == SPHERE else -1)
            if al >= 0:
                out.append((kind, int(i), self.area_lights[al][0], self.area_lights[al][1]))
        return out


# ------------------------------------------------------------------------------------------------------ rays through a chain
def _transform_rays(chain, o, d):
    """The exact float64 image of the rays under the chain of matrices, and what the reference's float32 transform_ray adds at
    each step to first order: componentwise o_err, d_err (carried through later matrices) and the summed origin shift dt."""
    n = len(o)
    oerr, derr, shift = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    for m in chain:
        A, tr = m[:3, :3], m[:3, 3]
        aA = np.abs(A)
        oe = gamma(3) * (np.abs(o) @ aA.T + np.abs(tr))            # transform_point_with_error
        de = gamma(3) * (np.abs(d) @ aA.T)                         # transform_vector_with_error
        o, d = o @ A.T + tr, d @ A.T
        oerr, derr = oerr @ aA.T + oe, derr @ aA.T + de
        l2 = (d * d).sum(1)
        dt = np.where(l2 > 0, (np.abs(d) * oe).sum(1) / np.where(l2 > 0, l2, 1.0), 0.0)
        shift = shift + dt
        oerr = oerr + gamma(2) * (np.abs(o) + np.abs(d) * dt[:, None])          # o += d * dt, rounded
    return o, d, oerr, derr, shift


class _Best:
    """Per ray: the nearest and second nearest accepted candidates, and the undecided candidates by rule."""
    FIELDS = ("t", "bound", "kind", "prim", "b0", "b1", "bb", "uid")

    def __init__(self, n):
        self.t = np.full((n, 2), np.inf); self.bound = np.zeros((n, 2)); self.kind = np.zeros((n, 2), np.int64)
        self.prim = np.full((n, 2), -1, np.int64); self.b0 = np.zeros((n, 2)); self.b1 = np.zeros((n, 2))
        self.bb = np.zeros((n, 2)); self.uid = np.full((n, 2), -1, np.int64)
        self.occ = np.zeros(n, bool)       # accepted by some primitive's intersect_p
        self.amb = []                      # (rule, rows, t - bound of the undecided candidate)
        self.next_uid = 0

    def offer(self, rows, **vals):
        """One candidate per listed ray (rows are distinct); scalars are broadcast."""
        vals = {k: np.broadcast_to(np.asarray(vals[k]), rows.shape).copy() for k in self.FIELDS}
        for slot in (0, 1):
            better = vals["t"] < self.t[rows, slot]
            r = rows[better]
            old = {k: getattr(self, k)[r, slot].copy() for k in self.FIELDS}
            for k in self.FIELDS:
                getattr(self, k)[r, slot] = vals[k][better]
            vals = {k: np.concatenate([vals[k][~better], old[k]]) for k in self.FIELDS}      # what was displaced moves on
            rows = np.concatenate([rows[~better], r])


def _triangles(sc, tri, flip, o, d, tmax, oerr, derr, shift, best, prim_of, kind_code, chunk=256):
    """Every ray against every triangle of one group.  flip: the instance transform mirrors (n.d changes sign with it)."""
    if len(tri) == 0:
        return
    p0, p1, p2 = sc.P[sc.idx[tri, 0]], sc.P[sc.idx[tri, 1]], sc.P[sc.idx[tri, 2]]
    nrm = np.cross(p0 - p2, p1 - p2)
    neg = ((sc.tri_flags[tri] & MESH_REVERSE) != 0) ^ ((sc.tri_flags[tri] & MESH_SWAPS) != 0)
    nrm = np.where(neg[:, None], -nrm, nrm)
    one_sided = (sc.tri_flags[tri] & MESH_TWO_SIDED) == 0
    prims = prim_of(tri)
    nxt = np.array([1, 2, 0])
    nabs = np.abs(nrm)
    p0T, p1T, p2T = np.ascontiguousarray(p0.T), np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T)
    uid0 = best.next_uid
    best.next_uid += len(tri)
    def one(s):
        e = min(len(o), s + chunk)
        oo, dd, tm = o[s:e], d[s:e], tmax[s:e]
        kz = np.argmax(np.abs(dd), axis=1)
        kx = nxt[kz]; ky = nxt[kx]
        perm = np.stack([kx, ky, kz], 1)
        dp = np.take_along_axis(dd, perm, 1)

        ar = np.arange(e - s)
        ox, oy, oz = oo[ar, kx][:, None], oo[ar, ky][:, None], oo[ar, kz][:, None]
        with np.errstate(all="ignore"):
            sx, sy, sz = (-dp[:, 0] / dp[:, 2])[:, None], (-dp[:, 1] / dp[:, 2])[:, None], (1.0 / dp[:, 2])[:, None]
            zz0, zz1, zz2 = p0T[kz] - oz, p1T[kz] - oz, p2T[kz] - oz
            x0, y0 = p0T[kx] - ox + sx * zz0, p0T[ky] - oy + sy * zz0
            x1, y1 = p1T[kx] - ox + sx * zz1, p1T[ky] - oy + sy * zz1
            x2, y2 = p2T[kx] - ox + sx * zz2, p2T[ky] - oy + sy * zz2
            e0, e1, e2 = x1 * y2 - y1 * x2, x2 * y0 - y2 * x0, x0 * y1 - y0 * x1
            det = e0 + e1 + e2
            z0, z1, z2 = zz0 * sz, zz1 * sz, zz2 * sz
            inv = 1.0 / det
            t = (e0 * z0 + e1 * z1 + e2 * z2) * inv
            b0, b1, b2 = e0 * inv, e1 * inv, e2 * inv
            max_zt = np.maximum(np.maximum(np.abs(z0), np.abs(z1)), np.abs(z2))
            max_xt = np.maximum(np.maximum(np.abs(x0), np.abs(x1)), np.abs(x2))
            max_yt = np.maximum(np.maximum(np.abs(y0), np.abs(y1)), np.abs(y2))
            delta_z = gamma(3) * max_zt
            delta_x, delta_y = gamma(5) * (max_xt + max_zt), gamma(5) * (max_yt + max_zt)
            delta_e = 2.0 * (gamma(2) * max_xt * max_yt + delta_y * max_xt + delta_x * max_yt)
            max_e = np.maximum(np.maximum(np.abs(e0), np.abs(e1)), np.abs(e2))
            delta_t = 3.0 * (gamma(3) * max_e * max_zt + delta_e * max_zt + delta_z * max_e) * np.abs(inv)
            bmin = np.minimum(np.minimum(b0, b1), b2)
            babs = np.maximum(np.maximum(np.abs(b0), np.abs(b1)), np.abs(b2))
            bb = delta_e * (1.0 + 3.0 * babs) * np.abs(inv) + gamma(5) * babs
            nd = dd @ nrm.T
            ndotd = -nd if flip else nd
            nd_scale = np.sqrt((dd * dd).sum(1))[:, None] * np.sqrt((nrm * nrm).sum(1))[None, :]
            # the ray's own error (rays inside an instance): plane form, plus the never-restored shift
            ray_term = (oerr[s:e] @ nabs.T + np.abs(t) * (derr[s:e] @ nabs.T)) / np.abs(nd) + shift[s:e, None]
            bound = delta_t + np.where(np.isfinite(ray_term), ray_term, 0.0)
            # an edge function's sign is decided where |e_i| = |b_i det| exceeds delta_e
            margin = np.maximum(BARY_MARGIN, delta_e * np.abs(inv))
            ok = np.isfinite(t) & (det != 0)
            culled = one_sided[None, :] & (ndotd >= 0)
            edge_on = one_sided[None, :] & (np.abs(ndotd) <= 1e-6 * nd_scale)
            inside = ok & (bmin >= 0) & ~culled
            graze = ok & (bmin > -margin) & ((bmin < margin) | edge_on) & ~(culled & ~edge_on)
            in_range = (t > delta_t) & (t <= tm[:, None])
            near_zero = (t > 0) & (t <= 2.0 * bound)          # t64 <= 0 is a decided miss: the float32 t is then below delta_t
            near_tmax = np.abs(t - tm[:, None]) <= bound
        hit = inside & in_range
        tt = np.where(hit, t, np.inf)
        rows = np.arange(e - s)
        offers, amb = [], []
        for _ in range(2):                                  # the two nearest of this group
            c = np.argmin(tt, axis=1)
            m = np.isfinite(tt[rows, c])
            r, c = rows[m], c[m]
            offers.append((r + s, dict(t=t[r, c], bound=bound[r, c], kind=kind_code, prim=prims[c], b0=b0[r, c], b1=b1[r, c], bb=bb[r, c], uid=uid0 + c)))
            tt[r, c] = np.inf
        for rule, mask in ((1, graze & (t > -bound)), (3, (inside | graze) & (near_zero | near_tmax))):
            rr, cc = np.nonzero(mask)
            if len(rr):
                amb.append((rule, rr + s, t[rr, cc] - bound[rr, cc]))
        return s, e, hit.any(1), offers, amb

    starts = list(range(0, len(o), chunk))
    with ThreadPoolExecutor(max_workers=THREADS) as pool:            # numpy releases the interpreter lock inside its loops
        for s, e, any_hit, offers, amb in pool.map(one, starts):
            best.occ[s:e] |= any_hit
            for rows, vals in offers:
                best.offer(rows, **vals)
            best.amb += amb


def _sphere(sp, chain, o_w, d_w, tmax, best, prim, kind_code):
    """Every ray against one sphere: offers intersect's candidate, records intersect_p's acceptance and the undecided roots.
    Returns the rays on which the two acceptances differ (Q58)."""
    o, d, oerr, derr, shift = _transform_rays(chain + [sp.w2o], o_w, d_w)
    n = len(o)
    r = sp.r
    a = (d * d).sum(1); b = 2.0 * (d * o).sum(1); c = (o * o).sum(1) - r * r
    da, db, dc = gamma(3) * a, gamma(4) * 2.0 * np.abs(d * o).sum(1), gamma(4) * ((o * o).sum(1) + r * r)
    disc = b * b - 4.0 * a * c
    with np.errstate(all="ignore"):
        # error of the discriminant from the same sources: d(disc) = 2 b db - 4 c da - 4 a dc, with the ray's own errors in b and c
        rb = 2.0 * (np.abs(d) * oerr + np.abs(o) * derr).sum(1) + db
        rc = 2.0 * (np.abs(o) * oerr).sum(1) + dc
        ra = 2.0 * (np.abs(d) * derr).sum(1) + da
        ddisc = 2.0 * np.abs(b) * rb + 4.0 * np.abs(c) * ra + 4.0 * a * rc
        root = np.sqrt(np.maximum(disc, 0.0))
        q = np.where(b < 0, -0.5 * (b - root), -0.5 * (b + root))
        ta, tb = q / a, c / q
        t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)
    has = (disc >= 0) & np.isfinite(t0) & np.isfinite(t1) & (a > 0)
    sil = (np.abs(disc) <= 16.0 * ddisc) & (a > 0)                # rule (a): silhouette graze, the first-order bound does not hold

    def bound_of(t):
        with np.errstate(all="ignore"):
            p = o + t[:, None] * d
            first = (2.0 * (np.abs(p) * (oerr + np.abs(t)[:, None] * derr)).sum(1) + t * t * da + np.abs(t) * db + dc) / root + gamma(6) * np.abs(t)
        return first + shift, p

    B0, p0 = bound_of(t0)
    B1, p1 = bound_of(t1)
    clipped_shape = (sp.zmin > -r) or (sp.zmax < r) or not sp.full_phi
    dlen = np.sqrt(a)

    def clip(p, B, wrap):
        """(rejected by the clips, within the point's bound of a clip edge)."""
        if not clipped_shape:
            return np.zeros(n, bool), np.zeros(n, bool)
        with np.errstate(all="ignore"):
            p = p * (r / np.sqrt((p * p).sum(1)))[:, None]
            Bp = dlen * B + gamma(8) * r
            raw = np.arctan2(p[:, 1], p[:, 0])
            phi = np.where(raw < 0, raw + wrap, raw)
            rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
            Bphi = Bp / rho
        rej = ((sp.zmin > -r) & (p[:, 2] < sp.zmin)) | ((sp.zmax < r) & (p[:, 2] > sp.zmax)) | (phi > sp.phimax)
        edge = ((sp.zmin > -r) & (np.abs(p[:, 2] - sp.zmin) <= Bp)) | ((sp.zmax < r) & (np.abs(p[:, 2] - sp.zmax) <= Bp))
        if not sp.full_phi:
            edge |= (np.abs(phi - sp.phimax) <= Bphi) | (np.abs(raw) <= Bphi) | (rho <= 4.0 * Bp) | ~np.isfinite(Bphi)
        return rej, edge

    TWO_PI = 2.0 * np.pi
    # the reference's flow (sphere.rs:84-131), intervals replaced by exact roots
    live = has & ~((t0 > tmax) | (t1 <= 0))
    first_is_t1 = t0 <= 0
    live &= ~(first_is_t1 & (t1 > tmax))
    tf, Bf, pf = np.where(first_is_t1, t1, t0), np.where(first_is_t1, B1, B0), np.where(first_is_t1[:, None], p1, p0)
    rej_f, edge_f = clip(pf, Bf, TWO_PI)
    retry = live & rej_f & ~first_is_t1 & ~(t1 > tmax)
    results = {}
    for name, wrap in (("closest", np.pi), ("any", TWO_PI)):       # Q58: intersect's second wrap is PI, intersect_p's 2 PI
        rej_s, edge_s = clip(p1, B1, wrap)
        ok_first = live & ~rej_f
        ok_second = retry & ~rej_s
        t = np.where(ok_first, tf, np.where(ok_second, t1, np.inf))
        B = np.where(ok_first, Bf, B1)
        results[name] = (t, B, (live & edge_f) | (retry & edge_s))
    # rule (c): roots in the zone the reference's conservative intervals straddle
    zone = has & ((np.abs(t0) <= 4.0 * B0) | (np.abs(t1) <= 4.0 * B1) | (np.abs(t0 - tmax) <= 4.0 * B0) | ((first_is_t1 | rej_f) & (np.abs(t1 - tmax) <= 4.0 * B1)))
    t, B, edge = results["closest"]
    rows = np.nonzero(np.isfinite(t) & ~sil)[0]
    best.offer(rows, t=t[rows], bound=B[rows], kind=kind_code, prim=prim, b0=0.0, b1=0.0, bb=0.0, uid=best.next_uid)
    best.next_uid += 1
    ta_, _, edge_a = results["any"]
    best.occ |= np.isfinite(ta_) & ~sil
    with np.errstate(all="ignore"):
        t_mid = -b / (2.0 * a)
        cand = np.where(t0 > -B0, t0 - B0, t1 - B1)          # the first root that is not behind the origin
    for rule, mask, tc in ((1, sil & ((t_mid > 0) | (c <= 0)), np.minimum(t_mid, np.where(np.isfinite(cand), cand, np.inf))), (3, zone & (t1 > -4.0 * B1), cand),
                           (4, (edge | edge_a) & has, cand)):
        rr = np.nonzero(mask)[0]
        if len(rr):
            best.amb.append((rule, rr, np.where(np.isfinite(tc[rr]), tc[rr], 0.0)))
    return np.isfinite(t) != np.isfinite(ta_)


def closest_hits(scene, o, d, tmax):
    """The float64 closest hit, occlusion and decisiveness of float32 rays.  Returns a dict of arrays, one entry per ray:
    kind (MISS / TRIANGLE / SPHERE / INSTANCE), prim (world primitive list position), t, b0, b1, bound (on t), bound_b,
    occluded ("some hit in (bound, t_max)", with intersect_p's acceptance), rule (0 = decisive, else index into RULES),
    tied_t / tied_bound (the second nearest hit, for rule b)."""
    sc = scene if isinstance(scene, Scene) else Scene(scene)
    o = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
    tmax = np.asarray(tmax, np.float32).astype(np.float64).reshape(-1)
    n = len(o)
    best = _Best(n)
    differs = np.zeros(n, bool)            # rays on which a sphere's intersect and intersect_p disagree (Q58)
    for chain, tri, sph, inst in sc.groups:
        lo, ld, oerr, derr, shift = _transform_rays(chain, o, d)
        flip = bool(chain) and np.linalg.det(chain[0][:3, :3]) < 0
        if inst is None:
            _triangles(sc, tri, flip, lo, ld, tmax, oerr, derr, shift, best, lambda t: sc.tri_prim[t], TRIANGLE)
        else:
            p = int(sc.instance_prim[inst])
            _triangles(sc, tri, flip, lo, ld, tmax, oerr, derr, shift, best, lambda t: np.full(len(t), p), INSTANCE)
        for i in sph:
            prim, kind = (int(sc.sphere_prim[i]), SPHERE) if inst is None else (int(sc.instance_prim[inst]), INSTANCE)
            differs |= _sphere(sc.spheres[i], chain, o, d, tmax, best, prim, kind)
    hit = np.isfinite(best.t[:, 0])
    t = np.where(hit, best.t[:, 0], 0.0)
    limit = np.where(hit & ~differs, best.t[:, 0] + best.bound[:, 0], tmax)          # (the any-hit query may go on where the two disagree)
    rule = np.zeros(n, np.int64)
    for r, rows, tc in best.amb:                       # undecided candidates that lie before the closest hit (or before t_max)
        m = tc <= limit[rows]
        rr = rows[m]
        rule[rr] = np.where(rule[rr] == 0, r, rule[rr])
    two = np.isfinite(best.t[:, 1]) & (best.uid[:, 1] != best.uid[:, 0])
    with np.errstate(invalid="ignore"):
        tie = two & (best.t[:, 1] - best.t[:, 0] <= best.bound[:, 0] + best.bound[:, 1])
    rule = np.where((rule == 0) & tie, 2, rule)
    occluded = best.occ
    return {"kind": np.where(hit, best.kind[:, 0], MISS), "prim": np.where(hit, best.prim[:, 0], -1), "t": t,
            "b0": best.b0[:, 0], "b1": best.b1[:, 0], "bound": best.bound[:, 0], "bound_b": best.bb[:, 0], "occluded": occluded,
            "rule": rule, "tied_t": best.t[:, 1], "tied_bound": best.bound[:, 1], "tied_prim": best.prim[:, 1]}


# ------------------------------------------------------------------------------------------------------------- area lights
def triangle_solid_angle(p, a, b, c):
    """Van Oosterom-Strackee: the solid angle triangle abc subtends at p."""
    A, B, C = a - p, b - p, c - p
    la, lb, lc = np.linalg.norm(A), np.linalg.norm(B), np.linalg.norm(C)
    num = np.dot(A, np.cross(B, C))
    den = la * lb * lc + np.dot(A, B) * lc + np.dot(A, C) * lb + np.dot(B, C) * la
    return abs(2.0 * np.arctan2(num, den))


def _coordinate_system(v1):
    if abs(v1[0]) > abs(v1[1]):
        v2 = np.array([-v1[2], 0.0, v1[0]]) / np.sqrt(v1[0] ** 2 + v1[2] ** 2)
    else:
        v2 = np.array([0.0, v1[2], -v1[1]]) / np.sqrt(v1[1] ** 2 + v1[2] ** 2)
    v3 = np.cross(v1, v2)
    return v2, v3 / np.linalg.norm(v3)


def light_truth(scene, light, ref_p, u, solid_angle=True):
    """DiffuseAreaLight::sample_li of light `light` for reference points ref_p (one, or one per u) and samples u, in float64.
    solid_angle=False leaves the solid angle out (NaN): it is one arctangent per reference point, in a Python loop.
    Returns a dict: p (the sampled point), wi, pdf (0 where the reference returns None), li, valid, p_bound (how far the float32
    point may lie from p), pdf_rel (the relative bound on pdf), solid_angle (per reference point; NaN where not defined: inside
    a sphere), branch ("triangle", "inside", "cone", "cone_small")."""
    sc = scene if isinstance(scene, Scene) else Scene(scene)
    kind, idx, L, two_sided_light = sc.lights()[light]
    u = np.asarray(u, np.float32).astype(np.float64).reshape(-1, 2)
    ref = np.asarray(ref_p, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(u)
    if len(ref) == 1:
        ref = np.repeat(ref, n, 0)
    out_branch = np.empty(n, object)
    sa = np.full(n, np.nan)
    pdf_rel = np.zeros(n)
    with np.errstate(all="ignore"):
        if kind == TRIANGLE:
            p0, p1, p2 = (sc.P[sc.idx[idx, k]] for k in range(3))
            flags = int(sc.tri_flags[idx])
            su0 = np.sqrt(u[:, 0])
            b0, b1 = 1.0 - su0, u[:, 1] * su0
            b2 = 1.0 - b0 - b1
            p = b0[:, None] * p0 + b1[:, None] * p1 + b2[:, None] * p2
            nn = np.cross(p1 - p0, p2 - p0)
            area = 0.5 * np.linalg.norm(nn)
            nn = np.repeat((nn / np.linalg.norm(nn))[None], n, 0)
            if flags & MESH_HAS_N:
                ns = b0[:, None] * sc.N[sc.idx[idx, 0]] + b1[:, None] * sc.N[sc.idx[idx, 1]] + b2[:, None] * sc.N[sc.idx[idx, 2]]
                nn = np.where(((nn * ns).sum(1) < 0)[:, None], -nn, nn)
            elif bool(flags & MESH_REVERSE) ^ bool(flags & MESH_SWAPS):
                nn = -nn
            p_bound = gamma(6) * np.linalg.norm(np.abs(b0[:, None] * p0) + np.abs(b1[:, None] * p1) + np.abs(b2[:, None] * p2), axis=1)
            w = p - ref
            dist2 = (w * w).sum(1)
            wi = w / np.sqrt(dist2)[:, None]
            cos = -(nn * wi).sum(1)
            valid = dist2 > 0
            if not (flags & MESH_TWO_SIDED):
                valid &= cos > 0
            pdf = dist2 / (area * np.abs(cos))
            # area (gamma(8): two differences, a cross product, a length), dist^2 and the cosine, whose absolute error is that
            # of wi and n (a few ulp each) and weighs 1 / |cos|; the point's own error moves dist by p_bound
            pdf_rel = gamma(24) + gamma(8) / np.abs(cos) + 4.0 * p_bound / np.sqrt(dist2) / np.abs(cos)
            out_branch[:] = "triangle"
            for i in range(n if solid_angle else 0):
                sa[i] = sa[i - 1] if i and np.array_equal(ref[i], ref[i - 1]) else triangle_solid_angle(ref[i], p0, p1, p2)
        else:
            sp = sc.spheres[idx]
            r = sp.r
            centre = sp.o2w[:3, 3].copy()
            inside = ((ref - centre) ** 2).sum(1) <= r * r
            # inside: Sphere::sample (sphere.rs:275-294)
            z = 1.0 - 2.0 * u[:, 0]
            rr = np.sqrt(np.maximum(0.0, 1.0 - z * z))
            phi = 2.0 * np.pi * u[:, 1]
            po = r * np.stack([rr * np.cos(phi), rr * np.sin(phi), z], 1)
            n_in = po @ sp.w2o[:3, :3]                       # transform_normal: the inverse's transpose
            n_in = n_in / np.linalg.norm(n_in, axis=1)[:, None]
            po = po * (r / np.linalg.norm(po, axis=1))[:, None]
            p_in = po @ sp.o2w[:3, :3].T + sp.o2w[:3, 3]
            area = sp.phimax * r * (sp.zmax - sp.zmin)
            # outside: the cone (sphere.rs:323-377)
            wc = centre - ref
            dc = np.linalg.norm(wc, axis=1)
            wc = wc / dc[:, None]
            s_max = r / dc
            s_max2 = s_max * s_max
            cos_max = np.sqrt(np.maximum(0.0, 1.0 - s_max2))
            cos_t = (cos_max - 1.0) * u[:, 0] + 1.0
            sin_t2 = 1.0 - cos_t * cos_t
            small = s_max2 < 0.00068523
            sin_t2 = np.where(small, np.maximum(0.0, s_max2 * u[:, 0]), sin_t2)
            cos_t = np.where(small, np.sqrt(1.0 - sin_t2), cos_t)
            cos_a = sin_t2 / s_max + cos_t * np.sqrt(np.maximum(0.0, 1.0 - sin_t2 / s_max / s_max))
            sin_a = np.sqrt(np.maximum(0.0, 1.0 - cos_a * cos_a))
            n_out = np.empty((n, 3))
            for i in range(n):
                if inside[i]:
                    n_out[i] = 0.0
                    continue
                x, y = _coordinate_system(wc[i])
                n_out[i] = sin_a[i] * np.cos(phi[i]) * -x + sin_a[i] * np.sin(phi[i]) * -y + cos_a[i] * -wc[i]
            p_out = centre + r * n_out
            p = np.where(inside[:, None], p_in, p_out)
            nn = np.where(inside[:, None], n_in, n_out)
            if sp.reverse:
                nn = -nn
            w = p - ref
            dist2 = (w * w).sum(1)
            wi = w / np.sqrt(dist2)[:, None]
            cos = -(nn * wi).sum(1)
            pdf_in = dist2 / (area * np.abs(cos))
            pdf_out = 1.0 / (2.0 * np.pi * (1.0 - cos_max))
            pdf = np.where(inside, pdf_in, pdf_out)
            valid = (dist2 > 0) & (pdf > 0) & np.isfinite(pdf)
            # the cone's density in float32: 1 - cos_max cancels.  cos_max carries half an ulp of 1 from the square root and the
            # subtraction under it, and gamma(4) s^2 / 2 from s^2; the difference is exact (Sterbenz), the rest gamma(4)
            rel_out = (2.0 * EPS + 0.5 * gamma(4) * s_max2) / (1.0 - cos_max) + gamma(4)
            p_bound_in = gamma(12) * np.linalg.norm(np.abs(po) @ np.abs(sp.o2w[:3, :3]).T + np.abs(sp.o2w[:3, 3]), axis=1)
            rel_in = gamma(24) + gamma(16) / np.abs(cos) + 4.0 * p_bound_in / np.sqrt(dist2) / np.abs(cos)
            pdf_rel = np.where(inside, rel_in, rel_out)
            # outside, the float32 point c + r n(sin_alpha, cos_alpha, phi).  sin^2 theta = 1 - cos^2 theta carries 9 ulp of 1 (two
            # for cos theta_max, two for cos theta, the square and the difference); the small-angle branch's s^2 u only gamma(3) of
            # itself.  E = 1 - sin^2 theta / s^2 divides that by s^2 -- the cancellation the branch exists for -- and a square root
            # near zero keeps half the digits: err(sqrt E) <= min(sqrt dE, dE / (2 sqrt E)).  The same twice for sin_alpha.
            d_s2 = np.where(small, gamma(3) * sin_t2, 9.0 * EPS)
            q = sin_t2 / s_max2
            E = np.maximum(0.0, 1.0 - q)
            dE = gamma(4) * (1.0 + q) + d_s2 / s_max2
            d_rootE = np.minimum(np.sqrt(dE), dE / (2.0 * np.sqrt(E))) + EPS * np.sqrt(E)
            d_ca = gamma(4) * np.abs(cos_a) + d_s2 / s_max + d_rootE + 4.0 * EPS
            dF = 2.0 * np.abs(cos_a) * d_ca + 2.0 * EPS
            d_sa = np.minimum(np.sqrt(dF), dF / (2.0 * sin_a)) + EPS * sin_a
            p_bound_out = r * (d_sa + d_ca + gamma(12)) + gamma(4) * (np.linalg.norm(centre) + r)       # gamma(12): the frame's three axes
            p_bound = np.where(inside, p_bound_in, p_bound_out)
            out_branch[:] = np.where(inside, "inside", np.where(small, "cone_small", "cone"))
            sa = np.where(inside, np.nan, 2.0 * np.pi * (1.0 - cos_max))
    facing = cos > 0
    li = np.where((two_sided_light | facing)[:, None], L[None, :], 0.0)
    pdf = np.where(valid, pdf, 0.0)
    return {"p": p, "wi": wi, "pdf": pdf, "li": li, "valid": valid, "p_bound": p_bound, "pdf_rel": pdf_rel, "solid_angle": sa,
            "branch": out_branch, "cos": cos, "dist": np.sqrt(dist2)}


def stratum_grid(k=64):
    """k x k stratum midpoints, then the four corners of [0, 1 - 2^-24]^2."""
    g = (np.arange(k) + 0.5) / k
    uu = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    hi = 1.0 - 2.0 ** -24
    return np.concatenate([uu, [[0.0, 0.0], [0.0, hi], [hi, 0.0], [hi, hi]]]).astype(np.float32)
