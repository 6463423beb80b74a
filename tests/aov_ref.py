"""Restatement of Integrator "aov" (integrators/aov.rs) in numpy, parameterised by dtype: the seventeen targets of a camera sample from
its ray, its restated differentials and its hit.  Independent of the oracle and of the product.

Run in float64 it is the truth the device is held to; run in float32 it is the reference's arithmetic without a device (the calibration
of test_aov_host.py).  Hits come from geometry_ref.closest_hits: primitive, t and barycentrics with their bounds.

What is restated
  * PerspectiveCamera::generate_ray_differential (perspective.rs:121-183), pinhole and thin lens, then render_tile's
    scale_differentials(1 / sqrt(spp)) (sampler.rs:218-233, ray_differential.rs:26-35).  The main ray is an INPUT (the device's, or
    main_ray() below for the calibration): only the offset rays are restated.
  * Triangle::intersect's interaction (triangle.rs:349-449): p and uv from the barycentrics, n from the winding with
    reverse_orientation ^ swaps_handedness, turned towards the shading normal when the mesh has N; shading n / dpdu / dpdv from N and
    S; get_dpdu_dpdv (triangle.rs:132-186) with the degenerate-uv fallback to coordinate_system; default uvs (0,0) (1,0) (1,1).
  * Sphere::intersect's interaction (sphere.rs:95-198): the refined point, phi with Q58's wrap by PI on the second root, uv, dpdu, dpdv,
    calc_normal, brought to the world by transform_surface_interaction.
  * TransformedPrimitive (transformed_primitive.rs:26-45): the ray's image under world_to_instance, the interaction brought back with
    transform_surface_interaction (transform.rs:299-323).
  * SurfaceInteraction::compute_differentials (surface_interaction.rs:221-282) with both failure branches and solve_linear_system_2x2's.
  * material_bump (core/material.rs:31-72) for a displacement that is a `bilerp` texture under the uv mapping.
  * v2c / clamp / scale (aov.rs:58-66).

Bounds.  Every quantity is a pair (value, bound): class E.  The value is computed in the run's dtype.  The bound is carried in float64
beside it by the first-order rules
    a + b : e_a + e_b                       a * b : |a| e_b + |b| e_a
    a / b : (e_a + |a / b| e_b) / |b|       sqrt a : e_a / (2 sqrt a)       (sqrt e_a at a = 0)
and every operation adds one float32 rounding of its result, 2^-24 |value|: an expression of n operations ends up with the gamma(n)
of its operation count times the magnitudes it passed through.  Inputs are exact float32 numbers (bound 0) except
  * the hit's t and barycentrics, which enter with geometry_ref's bounds (delta_t and bound_b), and
  * the raster-to-camera map, which the float32 products build from fov, the screen window and the resolution in at most 48 operations
    (perspective 6, its Gauss-Jordan inverse 12, three 4 x 4 products of 7 each, the point transform and its divide 8: 47): its exact
    closed form enters with gamma(48) of each term.
libm-grade functions (tan, sin, cos, acos, atan2) add 2 ulp.  No constant is fitted to any implementation.

A branch whose condition lies within its own bound of its threshold makes the sample undecided (`und`): the finiteness of tx / ty, the
|det| < 1e-10 test of the 2 x 2 solves, the axis choice of compute_differentials, the uv-determinant test of get_dpdu_dpdv, and the
signs face_forward reads.
"""
import numpy as np

import geometry_ref as G

U = 2.0 ** -24
TARGETS = ("distance", "depth", "n", "ns", "uv", "rdxc", "rdyc", "drodx", "drddx", "dpdx", "dpdy", "dpdu", "dpdv", "duvdx", "duvdy", "dpdus", "dpdvs")
SCENE_NAME = {"duvdy": "dstdy"}        # the name a scene asks a target by, where it is not the target's own: the reference has no "duvdy"
MESH_REVERSE, MESH_SWAPS, MESH_HAS_N, MESH_HAS_S, MESH_HAS_UV = 2, 4, 8, 16, 32
G48 = G.gamma(48)


class E:
    """value (the run's dtype) and a float64 bound on its distance from the exact value."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v)
        self.e = np.zeros(self.v.shape) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    def _lift(self, x):
        return x if isinstance(x, E) else E(np.full(self.v.shape, x, self.v.dtype))

    @staticmethod
    def _round(v, e):
        return E(v, e + U * np.abs(v.astype(np.float64)))

    def __add__(self, o):
        o = self._lift(o)
        return E._round(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        return E._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return self._lift(o) - self

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        o = self._lift(o)
        return E._round(self.v * o.v, np.abs(self.v.astype(np.float64)) * o.e + np.abs(o.v.astype(np.float64)) * self.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            e = (self.e + np.abs(v.astype(np.float64)) * o.e) / np.abs(o.v.astype(np.float64))
        return E._round(v, e)

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def sqrt(self):
        with np.errstate(all="ignore"):
            v = np.sqrt(np.maximum(self.v, 0))
            e = np.where(v > 0, self.e / (2.0 * v.astype(np.float64)), np.sqrt(self.e))
        return E._round(v, e)

    def abs(self):
        return E(np.abs(self.v), self.e)

    def take(self, m):
        return E(self.v[m], self.e[m])


def where(m, a, b):
    return E(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def const(x, n, dtype, rel=0.0):
    """A number known in float64 (a parameter of the scene) as the run's dtype; rel: relative bound of the float32 the reference holds."""
    return E(np.full(n, x, dtype), rel * abs(float(x)))


def _fn(f, a, e):
    with np.errstate(all="ignore"):
        v = f(a.v)
    return E(v, e + 2.0 * U * np.maximum(np.abs(v.astype(np.float64)), U))


def cos(a): return _fn(np.cos, a, a.e)
def sin(a): return _fn(np.sin, a, a.e)


def acos(a):
    x = np.clip(a.v, -1, 1)
    with np.errstate(all="ignore"):
        return _fn(np.arccos, E(x, a.e), a.e / np.sqrt(np.maximum(1.0 - x.astype(np.float64) ** 2, U)))


def atan2(y, x):
    with np.errstate(all="ignore"):
        v = np.arctan2(y.v, x.v)
        r2 = x.v.astype(np.float64) ** 2 + y.v.astype(np.float64) ** 2
        e = (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / r2
    return E(v, e + 2.0 * U * np.abs(v.astype(np.float64)))


# ---- vectors: lists of three E
def vadd(a, b): return [a[i] + b[i] for i in range(3)]
def vsub(a, b): return [a[i] - b[i] for i in range(3)]
def vscale(a, s): return [a[i] * s for i in range(3)]
def vneg(a): return [-a[i] for i in range(3)]
def vdot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def vcross(a, b): return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
def vlen(a): return vdot(a, a).sqrt()
def vwhere(m, a, b): return [where(m, a[i], b[i]) for i in range(3)]
def vtake(a, m): return [c.take(m) for c in a]


def vnorm(a):
    l = vlen(a)
    return [a[i] / l for i in range(3)]


def vconst(x, n, dtype):
    return [const(x[i], n, dtype) for i in range(3)]


def vexact(a, dtype):
    """(n, 3) float32 data as exact quantities of the run's dtype."""
    a = np.asarray(a, np.float32)
    return [E(a[:, i].astype(dtype)) for i in range(3)]


def xpoint(m, p):
    return [m[i][0] * p[0] + m[i][1] * p[1] + m[i][2] * p[2] + m[i][3] for i in range(3)]


def xvec(m, v):
    return [m[i][0] * v[0] + m[i][1] * v[1] + m[i][2] * v[2] for i in range(3)]


def xnormal(minv, n):                       # transform_normal: the inverse's transpose
    return [minv[0][i] * n[0] + minv[1][i] * n[1] + minv[2][i] * n[2] for i in range(3)]


def mat(a, n, dtype):
    """A float32 4 x 4 matrix (exact) as constants of the run."""
    a = np.array(list(a), np.float32).reshape(4, 4)
    return [[const(float(a[i, j]), n, dtype) for j in range(4)] for i in range(4)]


def face_forward(n, v, und):
    d = vdot(n, v)
    und |= np.abs(d.v) <= d.e
    return vwhere(d.v < 0, vneg(n), n)


def coordinate_system(v1):
    big = np.abs(v1[0].v) > np.abs(v1[1].v)
    zero = v1[0] * 0.0
    za = E(zero.v)
    l1 = (v1[0] * v1[0] + v1[2] * v1[2]).sqrt()
    l2 = (v1[1] * v1[1] + v1[2] * v1[2]).sqrt()
    a = [(-v1[2]) / l1, za, v1[0] / l1]
    b = [za, v1[2] / l2, (-v1[1]) / l2]
    v2 = vwhere(big, a, b)
    return v2, vcross(v1, v2)


# ------------------------------------------------------------------------------------------------------------------ camera
class Camera:
    def __init__(self, sd):
        d = sd.desc
        self.c2w = list(d.camera_to_world)
        self.tan_half = float(np.tan(np.radians(np.float64(np.float32(d.fov))) / 2.0))
        self.sw = [float(np.float32(v)) for v in d.screen_window]
        self.xres, self.yres = int(d.xres), int(d.yres)
        self.lens_radius, self.focal = float(np.float32(d.lens_radius)), float(np.float32(d.focal_distance))
        spp = int(d.spp)
        self.spp = spp if d.sampler == 1 else 1 << max(0, (spp - 1).bit_length())       # Sobol' rounds up to a power of two (sobol.rs:16-31)
        self.near = 0.01

    def p_camera(self, pf, dtype):
        """raster (x, y, 0) in camera space and the camera-space steps of one pixel in x and y (perspective.rs:60-77)."""
        n = len(pf)
        k = self.tan_half * self.near
        kx, ky = k * (self.sw[1] - self.sw[0]) / self.xres, k * (self.sw[2] - self.sw[3]) / self.yres
        fx, fy = E(np.asarray(pf[:, 0], np.float32).astype(dtype)), E(np.asarray(pf[:, 1], np.float32).astype(dtype))
        pc = [const(kx, n, dtype, G48) * fx + const(k * self.sw[0], n, dtype, G48), const(ky, n, dtype, G48) * fy + const(k * self.sw[3], n, dtype, G48),
              const(self.near, n, dtype, G48)]
        zero = const(0.0, n, dtype)
        return pc, [const(kx, n, dtype, G48), zero, zero], [zero, const(ky, n, dtype, G48), zero]


def concentric_sample_disk(u, dtype):
    ux, uy = E(np.asarray(u[:, 0], np.float32).astype(dtype)) * 2.0 - 1.0, E(np.asarray(u[:, 1], np.float32).astype(dtype)) * 2.0 - 1.0
    centre = (ux.v == 0) & (uy.v == 0)
    wide = np.abs(ux.v) > np.abs(uy.v)
    pi4, pi2 = float(np.float32(np.pi / 4)), float(np.float32(np.pi / 2))
    with np.errstate(all="ignore"):
        r = where(wide, ux, uy)
        theta = where(wide, (uy / ux) * pi4, pi2 - (ux / uy) * pi4)
    x, y = r * cos(theta), r * sin(theta)
    z = E(np.zeros_like(ux.v))
    return where(centre, z, x), where(centre, z, y)


def differentials(cam, o, d, p_film, u_lens, dtype):
    """The camera sample's offset rays after scale_differentials: rx_o, ry_o, rx_d, ry_d (E vectors).  o, d: the main ray (float32)."""
    n = len(o)
    pc, dxc, dyc = cam.p_camera(np.asarray(p_film), dtype)
    zero = const(0.0, n, dtype)
    m = mat(cam.c2w, n, dtype)
    outs = []
    for step in (dxc, dyc):
        dirc = vnorm(vadd(pc, step))
        oc = [zero, zero, zero]
        if cam.lens_radius > 0.0:
            lx, ly = concentric_sample_disk(np.asarray(u_lens), dtype)
            oc = [lx * cam.lens_radius, ly * cam.lens_radius, zero]
            ft = const(cam.focal, n, dtype) / dirc[2]
            focus = vscale(dirc, ft)
            dirc = vnorm(vsub(focus, oc))
        outs.append((xpoint(m, oc), xvec(m, dirc)))
    s = const(float(np.float32(1.0) / np.float32(cam.spp)), n, dtype, U).sqrt()
    ro, rd = vexact(o, dtype), vexact(d, dtype)
    rx_o, ry_o = (vadd(ro, vscale(vsub(w[0], ro), s)) for w in outs)
    rx_d, ry_d = (vadd(rd, vscale(vsub(w[1], rd), s)) for w in outs)
    return rx_o, ry_o, rx_d, ry_d


def main_ray(cam, p_film, u_lens):
    """generate_ray's main ray in float32 (without transform_ray's origin nudge): the calibration's input rays."""
    f = np.float32
    n = len(p_film)
    pc, _, _ = cam.p_camera(np.asarray(p_film), f)
    d = vnorm(pc)
    zero = const(0.0, n, f)
    o = [zero, zero, zero]
    if cam.lens_radius > 0.0:
        lx, ly = concentric_sample_disk(np.asarray(u_lens), f)
        o = [lx * cam.lens_radius, ly * cam.lens_radius, zero]
        d = vnorm(vsub(vscale(d, const(cam.focal, n, f) / d[2]), o))
    m = mat(cam.c2w, n, f)
    ow, dw = xpoint(m, o), xvec(m, d)
    return np.stack([c.v for c in ow], 1).astype(np.float32), np.stack([c.v for c in dw], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- interactions
def _tri_hit(o, d, p0, p1, p2):
    """The watertight test's t and barycentrics (triangle.rs:240-347) in the dtype of its arguments (plain arrays, (n, 3))."""
    kz = np.argmax(np.abs(d), axis=1)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    perm = np.stack([kx, ky, kz], 1)
    dp = np.take_along_axis(d, perm, 1)
    q = [np.take_along_axis(p - o, perm, 1) for p in (p0, p1, p2)]
    with np.errstate(all="ignore"):
        sx, sy, sz = -dp[:, 0] / dp[:, 2], -dp[:, 1] / dp[:, 2], 1 / dp[:, 2]
        x = [p[:, 0] + sx * p[:, 2] for p in q]
        y = [p[:, 1] + sy * p[:, 2] for p in q]
        e0, e1, e2 = x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]
        inv = 1 / (e0 + e1 + e2)
        t = (e0 * (q[0][:, 2] * sz) + e1 * (q[1][:, 2] * sz) + e2 * (q[2][:, 2] * sz)) * inv
        return t, e0 * inv, e1 * inv, e2 * inv


class Geometry:
    """The description's buffers by primitive, and the objects' members (for hits inside an instance)."""

    def __init__(self, sd):
        self.sd, self.sc = sd, G.Scene(sd)
        d = sd.desc
        self.P32 = np.asarray(sd.buffers["P"], np.float32).reshape(-1, 3)
        self.N32 = np.asarray(sd.buffers["N"], np.float32).reshape(-1, 3) if sd.buffers.get("N") is not None else None
        self.S32 = np.asarray(sd.buffers["S"], np.float32).reshape(-1, 3) if sd.buffers.get("S") is not None else None
        self.UV32 = np.asarray(sd.buffers["UV"], np.float32).reshape(-1, 2) if sd.buffers.get("UV") is not None else None
        self.idx = self.sc.idx
        self.tri_mesh = np.asarray(sd.buffers["tri_mesh"]).astype(np.int64).reshape(-1)
        self.meshes = [sd.buffers["meshes"][i] for i in range(d.n_meshes)]
        self.materials = [sd.buffers["materials"][i] for i in range(d.n_materials)]
        self.textures = [sd.buffers["textures"][i] for i in range(d.n_textures)] if d.n_textures else []
        self.spheres = [sd.buffers["spheres"][i] for i in range(d.n_spheres)]
        self.instances = [sd.buffers["instances"][i] for i in range(d.n_instances)]

    def members(self, o64, d64, t64, kind, prim):
        """Per ray: (instance or -1, 'T' / 'S', index) of the primitive the truth's hit lies on.  Inside an instance the member is the one whose
        own float64 hit is nearest the truth's t."""
        n = len(t64)
        inst = np.full(n, -1, np.int64)
        shape = np.zeros(n, np.int64)          # 0 triangle, 1 sphere
        index = np.full(n, -1, np.int64)
        for i in np.nonzero(kind != G.MISS)[0]:
            k, j = self.sc.prim_list[int(prim[i])]
            if k == G.TRIANGLE:
                index[i] = j
            elif k == G.SPHERE:
                shape[i], index[i] = 1, j
            else:
                inst[i] = j
        for k in np.unique(inst[inst >= 0]):
            rows = np.nonzero(inst == k)[0]
            w2i, obj = self.sc.instances[k]
            oo, dd = o64[rows] @ w2i[:3, :3].T + w2i[:3, 3], d64[rows] @ w2i[:3, :3].T
            best = np.full(len(rows), np.inf)
            for tri in np.nonzero(self.sc.tri_object == obj + 1)[0]:
                p = [np.repeat(self.sc.P[self.idx[tri, c]][None], len(rows), 0) for c in range(3)]
                t, b0, b1, b2 = _tri_hit(oo, dd, *p)
                ok = (np.minimum(np.minimum(b0, b1), b2) >= -1e-9) & np.isfinite(t)
                err = np.where(ok, np.abs(t - t64[rows]), np.inf)
                m = err < best
                best[m], shape[rows[m]], index[rows[m]] = err[m], 0, tri
            for j, sp in enumerate(self.sc.spheres):
                if sp.object != obj + 1:
                    continue
                o2, d2 = oo @ sp.w2o[:3, :3].T + sp.w2o[:3, 3], dd @ sp.w2o[:3, :3].T
                for t in _sphere_roots(o2, d2, sp.r):
                    err = np.where(np.isfinite(t), np.abs(t - t64[rows]), np.inf)
                    m = err < best
                    best[m], shape[rows[m]], index[rows[m]] = err[m], 1, j
        return inst, shape, index


def _sphere_roots(o, d, r):
    a, b, c = (d * d).sum(1), 2 * (d * o).sum(1), (o * o).sum(1) - r * r
    with np.errstate(all="ignore"):
        root = np.sqrt(np.maximum((b.astype(np.float64) ** 2 - 4.0 * a.astype(np.float64) * c.astype(np.float64)), 0)).astype(o.dtype)
        q = np.where(b < 0, -0.5 * (b - root), -0.5 * (b + root))
        t0, t1 = q / a, c / q
    return np.minimum(t0, t1), np.maximum(t0, t1)


def _get_dpdu_dpdv(uv, p, und):
    """Triangle::get_dpdu_dpdv (triangle.rs:132-186).  uv: three [u, v] of E, p: three E vectors."""
    duv02 = [uv[0][0] - uv[2][0], uv[0][1] - uv[2][1]]
    duv12 = [uv[1][0] - uv[2][0], uv[1][1] - uv[2][1]]
    dp02, dp12 = vsub(p[0], p[2]), vsub(p[1], p[2])
    det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
    und |= np.abs(np.abs(det.v.astype(np.float64)) - 1e-8) <= det.e
    degenerate = np.abs(det.v) < 1e-8
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        dpdu = vscale(vsub(vscale(dp02, duv12[1]), vscale(dp12, duv02[1])), inv)
        dpdv = vscale(vadd(vscale(dp02, -duv12[0]), vscale(dp12, duv02[0])), inv)
        cr = vcross(dpdu, dpdv)
        degenerate = degenerate | ~((cr[0].v ** 2 + cr[1].v ** 2 + cr[2].v ** 2) > 0)
        ng = vnorm(vcross(vsub(p[2], p[0]), vsub(p[1], p[0])))
        fu, fv = coordinate_system(ng)
    return vwhere(degenerate, fu, dpdu), vwhere(degenerate, fv, dpdv)


def _triangle(geo, tri, o, d, b0, b1, dtype, und):
    """The interaction on triangle `tri` in the space its vertices are in.  b0, b1: E."""
    n = len(b0.v)
    b2 = 1.0 - b0 - b1
    v = geo.idx[tri]
    flags = int(geo.meshes[geo.tri_mesh[tri]].flags)
    p = [vconst([float(c) for c in geo.P32[v[k]]], n, dtype) for k in range(3)]
    if (flags & MESH_HAS_UV) and geo.UV32 is not None:
        uvs = [[const(float(geo.UV32[v[k], 0]), n, dtype), const(float(geo.UV32[v[k], 1]), n, dtype)] for k in range(3)]
    else:
        uvs = [[const(a, n, dtype), const(b, n, dtype)] for a, b in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0))]
    dpdu, dpdv = _get_dpdu_dpdv(uvs, p, und)
    b = [b0, b1, b2]
    ph = vadd(vadd(vscale(p[0], b0), vscale(p[1], b1)), vscale(p[2], b2))
    uv = [b0 * uvs[0][c] + b1 * uvs[1][c] + b2 * uvs[2][c] for c in range(2)]
    nn = vnorm(vcross(vsub(p[0], p[2]), vsub(p[1], p[2])))
    if bool(flags & MESH_REVERSE) ^ bool(flags & MESH_SWAPS):
        nn = vneg(nn)
    zero3 = vconst([0.0, 0.0, 0.0], n, dtype)
    out = {"p": ph, "uv": uv, "n": nn, "dpdu": dpdu, "dpdv": dpdv, "sh_n": nn, "sh_dpdu": dpdu, "sh_dpdv": dpdv, "sh_dndu": zero3, "sh_dndv": zero3}
    has_n, has_s = bool(flags & MESH_HAS_N) and geo.N32 is not None, bool(flags & MESH_HAS_S) and geo.S32 is not None
    if has_n or has_s:
        def interp(A):
            vs = [vconst([float(c) for c in A[v[k]]], n, dtype) for k in range(3)]
            return vadd(vadd(vscale(vs[0], b[0]), vscale(vs[1], b[1])), vscale(vs[2], b[2])), vs
        ns = nn
        if has_n:
            nns, nv = interp(geo.N32)
            ns = vnorm(nns)
        ss = vnorm(dpdu)
        if has_s:
            ss = vnorm(interp(geo.S32)[0])
        ts = vnorm(vcross(ns, ss))
        ss = vnorm(vcross(ts, ns))
        if has_n:
            duv02 = [uvs[0][0] - uvs[2][0], uvs[0][1] - uvs[2][1]]
            duv12 = [uvs[1][0] - uvs[2][0], uvs[1][1] - uvs[2][1]]
            dn1, dn2 = vsub(nv[0], nv[2]), vsub(nv[1], nv[2])
            det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
            if np.all(np.abs(det.v) < 1e-8):
                dn = vcross(vsub(nv[2], nv[0]), vsub(nv[1], nv[0]))
                out["sh_dndu"], out["sh_dndv"] = coordinate_system(dn)
            else:
                inv = 1.0 / det
                out["sh_dndu"] = vscale(vsub(vscale(dn1, duv12[1]), vscale(dn2, duv02[1])), inv)
                out["sh_dndv"] = vscale(vadd(vscale(dn1, -duv12[0]), vscale(dn2, duv02[0])), inv)
        if flags & MESH_REVERSE:
            ts = vneg(ts)
        sh_n = vnorm(vcross(ss, ts))                       # set_shading_geometry(.., true)
        out["n"] = face_forward(nn, sh_n, und)
        out.update(sh_n=sh_n, sh_dpdu=ss, sh_dpdv=ts)
    return out


def _sphere(geo, j, o, d, t, second, dtype, und):
    """The interaction on sphere j, in the space its object_to_world maps to.  o, d: E vectors of the ray there; t: E; second: the hit is the
    second root after the first was clipped (Q58: a negative phi is wrapped by PI)."""
    ps, sp = geo.spheres[j], geo.sc.spheres[j]
    n = len(t.v)
    w2o, o2w = mat(ps.world_to_object, n, dtype), mat(ps.object_to_world, n, dtype)
    oo, dd = xpoint(w2o, o), xvec(w2o, d)
    r = const(sp.r, n, dtype)
    ph = vadd(oo, vscale(dd, t))
    ph = vscale(ph, r / vlen(ph))
    raw = atan2(ph[1], ph[0])
    und |= np.abs(raw.v) <= raw.e
    phi = where(raw.v < 0, raw + where(second, const(float(np.float32(np.pi)), n, dtype), const(float(np.float32(2 * np.pi)), n, dtype)), raw)
    phimax = const(sp.phimax, n, dtype)
    tmin_v, tmax_v = float(np.arccos(np.clip(sp.zmin / sp.r, -1, 1))), float(np.arccos(np.clip(sp.zmax / sp.r, -1, 1)))
    theta_min, theta_max = const(tmin_v, n, dtype, 3 * U), const(tmax_v, n, dtype, 3 * U)
    dtheta = theta_max - theta_min
    theta = acos(ph[2] / r)
    uv = [phi / phimax, (theta - theta_min) / dtheta]
    zr = (ph[0] * ph[0] + ph[1] * ph[1]).sqrt()
    inv_zr = 1.0 / zr
    cphi, sphi = ph[0] * inv_zr, ph[1] * inv_zr
    zero = const(0.0, n, dtype)
    dpdu = [-(phimax * ph[1]), phimax * ph[0], zero]
    dpdv = vscale([ph[2] * cphi, ph[2] * sphi, -(r * sin(theta))], dtheta)
    nn = vnorm(vcross(dpdu, dpdv))
    swaps = np.linalg.det(sp.o2w[:3, :3]) < 0
    if bool(sp.reverse) ^ bool(swaps):
        nn = vneg(nn)
    nw = vnorm(xnormal(w2o, nn))
    zero3 = [zero, zero, zero]
    dpdu_w, dpdv_w = xvec(o2w, dpdu), xvec(o2w, dpdv)
    return {"p": xpoint(o2w, ph), "uv": uv, "n": nw, "dpdu": dpdu_w, "dpdv": dpdv_w, "sh_n": nw, "sh_dpdu": dpdu_w, "sh_dpdv": dpdv_w,
            "sh_dndu": zero3, "sh_dndv": zero3}


def _to_world(geo, k, s, n, dtype, und):
    """transform_surface_interaction (transform.rs:299-323) of instance k."""
    it = geo.instances[k]
    m, mi = mat(it.instance_to_world, n, dtype), mat(it.world_to_instance, n, dtype)
    out = dict(s)
    out["p"] = xpoint(m, s["p"])
    out["n"] = vnorm(xnormal(mi, s["n"]))
    for key in ("dpdu", "dpdv", "sh_dpdu", "sh_dpdv"):
        out[key] = xvec(m, s[key])
    for key in ("sh_dndu", "sh_dndv"):
        out[key] = xnormal(mi, s[key])
    out["sh_n"] = face_forward(vnorm(xnormal(mi, s["sh_n"])), out["n"], und)
    return out


def _solve_2x2(a, b, und):
    det = a[0][0] * a[1][1] - a[0][1] * a[1][0]
    und |= np.abs(np.abs(det.v.astype(np.float64)) - 1e-10) <= det.e
    fail = np.abs(det.v) < 1e-10
    with np.errstate(all="ignore"):
        x0 = (a[1][1] * b[0] - a[0][1] * b[1]) / det
        x1 = (a[0][0] * b[1] - a[1][0] * b[0]) / det
    fail = fail | np.isnan(x0.v) | np.isnan(x1.v)
    z = E(np.zeros_like(x0.v))
    return where(fail, z, x0), where(fail, z, x1)


def _compute_differentials(s, rx_o, ry_o, rx_d, ry_d, und):
    """SurfaceInteraction::compute_differentials (surface_interaction.rs:221-282)."""
    p, nn = s["p"], s["n"]
    dd = vdot(nn, p)
    with np.errstate(all="ignore"):
        den_x, den_y = vdot(nn, rx_d), vdot(nn, ry_d)
        tx = -(vdot(nn, rx_o) - dd) / den_x
        ty = -(vdot(nn, ry_o) - dd) / den_y
    und |= (np.abs(den_x.v) <= den_x.e) | (np.abs(den_y.v) <= den_y.e)
    fail = ~np.isfinite(tx.v) | ~np.isfinite(ty.v)
    px, py = vadd(rx_o, vscale(rx_d, tx)), vadd(ry_o, vscale(ry_d, ty))
    dpdx, dpdy = vsub(px, p), vsub(py, p)
    ax, ay, az = (np.abs(nn[i].v) for i in range(3))
    ex, ey, ez = (nn[i].e for i in range(3))
    und |= (np.abs(ax - ay) <= ex + ey) & (np.maximum(ax, ay) >= az - ez) | (np.abs(ax - az) <= ex + ez) & (np.maximum(ax, az) >= ay - ey) | \
           (np.abs(ay - az) <= ey + ez) & (np.maximum(ay, az) >= ax - ex)
    c1 = (ax > ay) & (ax > az)
    c2 = ~c1 & (ay > az)
    pick = lambda v, k: where(k == 0, v[0], where(k == 1, v[1], v[2]))
    d0 = np.where(c1, 1, 0)
    d1 = np.where(c1 | c2, 2, 1)
    a = [[pick(s["dpdu"], d0), pick(s["dpdv"], d0)], [pick(s["dpdu"], d1), pick(s["dpdv"], d1)]]
    bx = [pick(px, d0) - pick(p, d0), pick(px, d1) - pick(p, d1)]
    by = [pick(py, d0) - pick(p, d0), pick(py, d1) - pick(p, d1)]
    dudx, dvdx = _solve_2x2(a, bx, und)
    dudy, dvdy = _solve_2x2(a, by, und)
    z = E(np.zeros_like(tx.v))
    zero3 = [z, z, z]
    return {"dpdx": vwhere(fail, zero3, dpdx), "dpdy": vwhere(fail, zero3, dpdy), "dudx": where(fail, z, dudx), "dvdx": where(fail, z, dvdx),
            "dudy": where(fail, z, dudy), "dvdy": where(fail, z, dvdy)}


def _bilerp(tex, u, v):
    """BilerpTexture over UVMapping2D (textures/bilerp.rs, mapping2d.rs:20-40), channel 0."""
    n, dtype = len(u.v), u.v.dtype
    s = u * float(np.float32(tex.su)) + float(np.float32(tex.du))
    t = v * float(np.float32(tex.sv)) + float(np.float32(tex.dv))
    v00, v01, v10, v11 = (const(float(np.float32(tex.value[k][0])), n, dtype) for k in range(4))
    return (1.0 - s) * (1.0 - t) * v00 + (1.0 - s) * t * v01 + s * (1.0 - t) * v10 + s * t * v11


def _bump(tex, s, df, und):
    """material_bump (core/material.rs:31-72); set_shading_geometry(.., false)."""
    du = (df["dudx"].abs() + df["dudy"].abs()) * 0.5
    dv = (df["dvdx"].abs() + df["dvdy"].abs()) * 0.5
    du = where(du.v == 0, E(np.full_like(du.v, 0.0005)), du)
    dv = where(dv.v == 0, E(np.full_like(dv.v, 0.0005)), dv)
    u, v = s["uv"]
    u_disp, v_disp, disp = _bilerp(tex, u + du, v + 0.0), _bilerp(tex, u + 0.0, v + dv), _bilerp(tex, u, v)
    dpdu = vadd(vadd(s["sh_dpdu"], vscale(s["sh_n"], (u_disp - disp) / du)), vscale(s["sh_dndu"], disp))
    dpdv = vadd(vadd(s["sh_dpdv"], vscale(s["sh_n"], (v_disp - disp) / dv)), vscale(s["sh_dndv"], disp))
    out = dict(s)
    out.update(sh_n=face_forward(vnorm(vcross(dpdu, dpdv)), s["n"], und), sh_dpdu=dpdu, sh_dpdv=dpdv)
    return out


def _clamp01(x):
    return E(np.clip(x.v, 0, 1), x.e)


def _v2c(v, scale):
    return [_clamp01(c * 0.5 + 0.5) * scale for c in v]


# ------------------------------------------------------------------------------------------------------------------ the seventeen
def evaluate(sd, o, d, p_film, u_lens, hits, dtype, scale=1.0, geo=None, hits32=False):
    """All targets of n camera samples.  o, d: the main rays (float32); p_film, u_lens: the camera samples; hits: geometry_ref.closest_hits
    of those rays.  dtype float64: t and the barycentrics are the truth's, with its bounds.  dtype float32 (hits32): they are recomputed
    in float32 on the truth's primitive -- the reference's arithmetic.  Returns {"value": {target: (n, 3)}, "bound": {target: (n, 3)},
    "hit": (n,), "und": (n,) undecided branches, "t": (n,)}; misses report 0 with bound 0."""
    geo = geo or Geometry(sd)
    cam = Camera(sd)
    n = len(o)
    o32, d32 = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    o64, d64 = o32.astype(np.float64), d32.astype(np.float64)
    kind, t64 = hits["kind"], hits["t"]
    inst, shape, index = geo.members(o64, d64, t64, kind, hits["prim"])
    value = {k: np.zeros((n, 3)) for k in TARGETS}
    bound = {k: np.zeros((n, 3)) for k in TARGETS}
    und_all = np.zeros(n, bool)
    t_out = np.zeros(n)
    hit = kind != G.MISS
    keys = np.stack([inst, shape, index], 1)
    for key in np.unique(keys[hit], axis=0) if hit.any() else []:
        rows = np.nonzero(hit & (keys == key).all(1))[0]
        m = len(rows)
        und = np.zeros(m, bool)
        k_inst, k_shape, k_idx = (int(x) for x in key)
        ro, rd = vexact(o32[rows], dtype), vexact(d32[rows], dtype)
        lo, ld = ro, rd
        if k_inst >= 0:
            w2i = mat(geo.instances[k_inst].world_to_instance, m, dtype)
            lo, ld = xpoint(w2i, ro), xvec(w2i, rd)
        t = E(t64[rows].astype(dtype), hits["bound"][rows])
        if k_shape == 0:
            b0, b1 = E(hits["b0"][rows].astype(dtype), hits["bound_b"][rows]), E(hits["b1"][rows].astype(dtype), hits["bound_b"][rows])
            if hits32:
                lov, ldv = np.stack([c.v for c in lo], 1), np.stack([c.v for c in ld], 1)
                pv = [np.repeat(geo.P32[geo.idx[k_idx, c]][None].astype(dtype), m, 0) for c in range(3)]
                tt, bb0, bb1, _ = _tri_hit(lov, ldv, *pv)
                t, b0, b1 = E(tt), E(bb0), E(bb1)
            s = _triangle(geo, k_idx, lo, ld, b0, b1, dtype, und)
        else:
            sp = geo.sc.spheres[k_idx]
            w2o = sp.w2o
            ol, dl = np.stack([c.v for c in lo], 1).astype(np.float64), np.stack([c.v for c in ld], 1).astype(np.float64)
            r0, r1 = _sphere_roots(ol @ w2o[:3, :3].T + w2o[:3, 3], dl @ w2o[:3, :3].T, sp.r)
            second = (np.abs(r1 - t64[rows]) < np.abs(r0 - t64[rows])) & (r0 > 0)
            if hits32:
                w32 = mat(geo.spheres[k_idx].world_to_object, m, dtype)
                o_, d_ = xpoint(w32, lo), xvec(w32, ld)
                q0, q1 = _sphere_roots(np.stack([c.v for c in o_], 1), np.stack([c.v for c in d_], 1), dtype(sp.r))
                t = E(np.where(np.abs(r1 - t64[rows]) < np.abs(r0 - t64[rows]), q1, q0))
            s = _sphere(geo, k_idx, lo, ld, t, second, dtype, und)
        if k_inst >= 0:
            s = _to_world(geo, k_inst, s, m, dtype, und)
        sub = lambda x: x[rows] if x is not None else None
        rx_o, ry_o, rx_d, ry_d = differentials(cam, o32[rows], d32[rows], np.asarray(p_film)[rows], sub(np.asarray(u_lens)), dtype)
        df = _compute_differentials(s, rx_o, ry_o, rx_d, ry_d, und)
        mat_i = geo.meshes[geo.tri_mesh[k_idx]].material if k_shape == 0 else geo.spheres[k_idx].material
        if mat_i >= 0 and geo.materials[mat_i].type != 0 and geo.materials[mat_i].tex_bump:
            tex = geo.textures[geo.materials[mat_i].tex_bump - 1]
            if tex.type != 6:
                raise NotImplementedError("the restatement bumps with bilerp displacements only")
            s = _bump(tex, s, df, und)
        dist = t / vlen(rd)
        depth = vlen(vsub(s["p"], ro))
        z = E(np.zeros(m, dtype))
        sc_ = float(np.float32(scale))
        res = {"distance": [_clamp01(dist) * sc_] * 3, "depth": [_clamp01(depth) * sc_] * 3, "n": _v2c(s["n"], sc_), "ns": _v2c(s["sh_n"], sc_),
               "uv": [_clamp01(s["uv"][0]) * sc_, _clamp01(s["uv"][1]) * sc_, z * sc_], "rdxc": _v2c(rx_o, sc_), "rdyc": [z, z, z],
               "drodx": _v2c(rx_o, sc_), "drddx": _v2c(rx_d, sc_), "dpdx": _v2c(df["dpdx"], sc_), "dpdy": _v2c(df["dpdy"], sc_),
               "dpdu": _v2c(s["dpdu"], sc_), "dpdv": _v2c(s["dpdv"], sc_), "duvdx": _v2c([df["dudx"].abs(), df["dvdx"].abs(), z], sc_),
               "duvdy": _v2c([df["dudy"].abs(), df["dvdy"].abs(), z], sc_), "dpdus": _v2c(s["sh_dpdu"], sc_), "dpdvs": _v2c(s["sh_dpdv"], sc_)}
        for k in TARGETS:
            value[k][rows] = np.stack([c.v.astype(np.float64) for c in res[k]], 1)
            bound[k][rows] = np.stack([c.e for c in res[k]], 1)
        und_all[rows] = und
        t_out[rows] = t.v
    return {"value": value, "bound": bound, "hit": hit, "und": und_all, "t": t_out}
