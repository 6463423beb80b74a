"""Independent float32 restatement of the reference's three tessellated shapes, for the host tests.

Written from the reference's Rust (shapes/loopsubdiv.rs, shapes/nurbs.rs, shapes/heightfield.rs) and kept close to its
shape: loopsubdiv below is the pointer graph of SDVertex / SDFace objects with edges keyed by vertex pair, not the index
arrays of the library.  Every arithmetic step is a numpy float32 scalar operation in the reference's order; cos / sin are
glibc's cosf / sinf through ctypes (numpy's float32 cos is not glibc's), as Rust's f32::cos / f32::sin call them.

Each function returns {"P": (n, 3) f32, "N": (n, 3) f32 or None, "uv": (n, 2) f32 or None, "indices": (m, 3) u32} in
object space, or raises RefError with the reference's message where it returns an error.
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = ctypes.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [ctypes.c_float]
PI = f32(np.pi)                      # std::f32::consts::PI


def cosf(x):
    return f32(_libm.cosf(float(x)))


def sinf(x):
    return f32(_libm.sinf(float(x)))


class RefError(Exception):
    pass


# ---- f32 vectors as 3-tuples of np.float32
def add(a, b):
    return (f32(a[0] + b[0]), f32(a[1] + b[1]), f32(a[2] + b[2]))


def sub(a, b):
    return (f32(a[0] - b[0]), f32(a[1] - b[1]), f32(a[2] - b[2]))


def mul(s, a):
    s = f32(s)
    return (f32(s * a[0]), f32(s * a[1]), f32(s * a[2]))


def cross(a, b):
    return (f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0])))


def normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2])), dtype=f32)
        return (f32(v[0] / l), f32(v[1] / l), f32(v[2] / l))


# ---------------------------------------------------------------- loopsubdiv.rs
NEXT = (1, 2, 0)
PREV = (2, 0, 1)


class SDVertex:
    __slots__ = ("p", "start_face", "child", "regular", "boundary")

    def __init__(self, p):
        self.p = p
        self.start_face = None
        self.child = None
        self.regular = False
        self.boundary = False

    def valence(self):
        return len(self.one_ring())

    def one_ring(self):
        pts = []
        if not self.boundary:
            face = self.start_face
            while True:
                pts.append(face.next_vert(self).p)
                face = face.next_face(self)
                if face is self.start_face:
                    break
        else:
            face = self.start_face
            while face.next_face(self) is not None:
                face = face.next_face(self)
            pts.append(face.next_vert(self).p)
            while True:
                pts.append(face.prev_vert(self).p)
                f2 = face.prev_face(self)
                if f2 is None:
                    break
                face = f2
        return pts


class SDFace:
    __slots__ = ("v", "f", "children")

    def __init__(self):
        self.v = [None, None, None]
        self.f = [None, None, None]
        self.children = [None, None, None, None]

    def vnum(self, vert):
        for i in range(3):
            if self.v[i] is vert:
                return i
        return -1

    def next_face(self, vert):
        return self.f[self.vnum(vert)]

    def prev_face(self, vert):
        return self.f[PREV[self.vnum(vert)]]

    def next_vert(self, vert):
        return self.v[NEXT[self.vnum(vert)]]

    def prev_vert(self, vert):
        return self.v[PREV[self.vnum(vert)]]

    def other_vert(self, v0, v1):
        for i in range(3):
            if self.v[i] is not v0 and self.v[i] is not v1:
                return self.v[i]
        return None


def _edge_key(a, b):
    return (id(a), id(b)) if id(a) < id(b) else (id(b), id(a))


def weight_one_ring(vert, beta):
    ring = vert.one_ring()
    valence = f32(len(ring))
    beta = f32(beta)
    p = mul(f32(f32(1.0) - f32(valence * beta)), vert.p)
    for q in ring:
        p = add(p, mul(beta, q))
    return p


def weight_boundary(vert, beta):
    ring = vert.one_ring()
    beta = f32(beta)
    p = mul(f32(f32(1.0) - f32(f32(2.0) * beta)), vert.p)
    p = add(p, mul(beta, ring[0]))
    p = add(p, mul(beta, ring[-1]))
    return p


def beta(valence):
    if valence == 3:
        return f32(3.0) / f32(16.0)
    return f32(f32(3.0) / f32(f32(8.0) * f32(valence)))


def loop_gamma(valence):
    return f32(f32(1.0) / f32(f32(valence) + f32(f32(3.0) / f32(f32(8.0) * beta(valence)))))


def loopsubdiv(indices, P, n_levels):
    """loop_subdiv (loopsubdiv.rs:311-703) on object-space P (flat or (n, 3)) and indices."""
    P = np.asarray(P, f32).reshape(-1)
    vi = [int(i) for i in np.asarray(indices).reshape(-1)]
    vertices = [SDVertex((P[3 * i], P[3 * i + 1], P[3 * i + 2])) for i in range(len(P) // 3)]
    faces = [SDFace() for _ in range(len(vi) // 3)]
    for i, face in enumerate(faces):
        for j in range(3):
            v = vertices[vi[3 * i + j]]
            face.v[j] = v
            v.start_face = face
    edges = {}
    for face in faces:
        for en in range(3):
            key = _edge_key(face.v[en], face.v[NEXT[en]])
            if key not in edges:
                edges[key] = (face, en)
            else:
                f0, f0en = edges.pop(key)
                f0.f[f0en] = face
                face.f[en] = f0
    for v in vertices:
        face = v.start_face
        while True:
            f2 = face.next_face(v)
            if f2 is None:
                v.boundary = True
                break
            if f2 is v.start_face:
                break
            face = f2
        val = v.valence()
        v.regular = (not v.boundary and val == 6) or (v.boundary and val == 4)

    f, v = faces, vertices
    for _ in range(n_levels):
        new_faces, new_vertices = [], []
        for vert in v:
            nv = SDVertex(vert.p)
            nv.regular, nv.boundary = vert.regular, vert.boundary
            vert.child = nv
            new_vertices.append(nv)
        for face in f:
            for k in range(4):
                nf = SDFace()
                face.children[k] = nf
                new_faces.append(nf)
        for vert in v:
            if not vert.boundary:
                vert.child.p = weight_one_ring(vert, f32(1.0) / f32(16.0) if vert.regular else beta(vert.valence()))
            else:
                vert.child.p = weight_boundary(vert, f32(1.0) / f32(8.0))
        edge_verts = {}
        for face in f:
            for k in range(3):
                a, b = face.v[k], face.v[NEXT[k]]
                key = _edge_key(a, b)
                if key in edge_verts:
                    continue
                vert = SDVertex((f32(0), f32(0), f32(0)))
                new_vertices.append(vert)
                vert.regular = True
                vert.boundary = face.f[k] is None
                vert.start_face = face.children[3]
                e0, e1 = (a, b) if id(a) < id(b) else (b, a)       # SDEdge orders by pointer
                if vert.boundary:
                    vert.p = add(mul(0.5, e0.p), mul(0.5, e1.p))
                else:
                    po0 = face.other_vert(e0, e1).p
                    po1 = face.f[k].other_vert(e0, e1).p
                    c3, c1 = f32(3.0) / f32(8.0), f32(1.0) / f32(8.0)
                    vert.p = add(add(add(mul(c3, e0.p), mul(c3, e1.p)), mul(c1, po0)), mul(c1, po1))
                edge_verts[key] = vert
        for vert in v:
            vert.child.start_face = vert.start_face.children[vert.start_face.vnum(vert)]
        for face in f:
            for j in range(3):
                face.children[3].f[j] = face.children[NEXT[j]]
                face.children[j].f[NEXT[j]] = face.children[3]
                f2 = face.f[j]
                if f2 is not None:
                    face.children[j].f[j] = f2.children[f2.vnum(face.v[j])]
                f2 = face.f[PREV[j]]
                if f2 is not None:
                    face.children[j].f[PREV[j]] = f2.children[f2.vnum(face.v[j])]
        for face in f:
            for j in range(3):
                face.children[j].v[j] = face.v[j].child
                vert = edge_verts[_edge_key(face.v[j], face.v[NEXT[j]])]
                face.children[j].v[NEXT[j]] = vert
                face.children[NEXT[j]].v[j] = vert
                face.children[3].v[j] = vert
        f, v = new_faces, new_vertices

    p_limit = []
    for vert in v:                  # in place, vertex by vertex: later rings see pushed neighbours
        if vert.boundary:
            vert.p = weight_boundary(vert, f32(1.0) / f32(5.0))
        else:
            vert.p = weight_one_ring(vert, loop_gamma(vert.valence()))
        p_limit.append(vert.p)
    ns = []
    zero = (f32(0), f32(0), f32(0))
    for vert in v:
        s, t = zero, zero
        ring = vert.one_ring()
        valence = len(ring)
        if not vert.boundary:
            for j in range(valence):
                ang = f32(f32(f32(f32(2.0) * PI) * f32(j)) / f32(valence))
                s = add(s, mul(cosf(ang), ring[j]))
                t = add(t, mul(sinf(ang), ring[j]))
        else:
            s = sub(ring[-1], ring[0])
            if valence == 2:
                t = sub(add(ring[0], ring[1]), mul(2.0, vert.p))
            elif valence == 3:
                t = sub(ring[1], vert.p)
            elif valence == 4:
                t = add(add(add(add(mul(-1.0, ring[0]), mul(2.0, ring[1])), mul(2.0, ring[2])), mul(-1.0, ring[3])), mul(-2.0, vert.p))
            else:
                theta = f32(PI / f32(valence - 1))
                t = mul(sinf(theta), add(ring[0], ring[-1]))
                for k in range(1, valence - 1):
                    wt = f32(f32(f32(f32(2.0) * cosf(theta)) - f32(2.0)) * sinf(f32(f32(k) * theta)))
                    t = add(t, mul(wt, ring[k]))
                t = (-t[0], -t[1], -t[2])
        ns.append(normalize(cross(s, t)))
    index = {id(vert): i for i, vert in enumerate(v)}
    tri = [[index[id(face.v[j])] for j in range(3)] for face in f]
    return {"P": np.array(p_limit, f32).reshape(-1, 3), "N": np.array(ns, f32).reshape(-1, 3), "uv": None,
            "indices": np.array(tri, np.uint32).reshape(-1, 3)}


# ---------------------------------------------------------------- nurbs.rs
def knot_offset(knot, order, t):
    off = order - 1
    while t > knot[off + 1]:
        off += 1
    assert knot[off] <= t <= knot[off + 1]
    return off


def nurbs_evaluate(order, knot, cp, cp_off, cp_stride, t):
    """(homogeneous value (x, y, z, w), derivative (x, y, z)); cp[cp_off + k] is the OffsetArray of the reference."""
    ko = knot_offset(knot, order, t)
    cp_offset = ko - order + 1
    w = [list(cp[cp_off + (cp_offset + i) * cp_stride]) for i in range(order)]
    kn = lambda i: knot[ko + i]
    for i in range(order - 2):
        for j in range(order - 1 - i):
            with np.errstate(invalid="ignore", divide="ignore"):
                alpha = f32(f32(kn(1 + j) - t) / f32(kn(1 + j) - kn(j + 2 - order + i)))
            assert 0.0 <= alpha <= 1.0
            oma = f32(f32(1.0) - alpha)
            w[j] = [f32(f32(alpha * w[j][c]) + f32(oma * w[j + 1][c])) for c in range(4)]
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = f32(f32(kn(1) - t) / f32(kn(1) - kn(0)))
    assert 0.0 <= alpha <= 1.0
    oma = f32(f32(1.0) - alpha)
    val = [f32(f32(alpha * w[0][c]) + f32(oma * w[1][c])) for c in range(4)]
    factor = f32(f32(order - 1) / f32(kn(1) - kn(0)))
    d = [f32(factor * f32(w[1][c] - w[0][c])) for c in range(4)]
    with np.errstate(invalid="ignore", divide="ignore"):
        ww = f32(val[3] * val[3])
        deriv = tuple(f32(f32(d[c] / val[3]) - f32(f32(val[c] * d[3]) / ww)) for c in range(3))
    return val, deriv


def nurbs_evaluate_surface(uorder, uknot, ucp, u, vorder, vknot, vcp, v, cp):
    iso = [None] * max(uorder, vorder)
    u_first = knot_offset(uknot, uorder, u) - uorder + 1
    for i in range(uorder):
        iso[i] = nurbs_evaluate(vorder, vknot, cp, u_first + i, ucp, v)[0]
    v_first = knot_offset(vknot, vorder, v) - vorder + 1
    assert v_first < vcp
    p, dpdu = nurbs_evaluate(uorder, uknot, iso, -u_first, 1, u)
    for i in range(vorder):
        iso[i] = nurbs_evaluate(uorder, uknot, cp, (v_first + i) * ucp, 1, u)[0]
    _, dpdv = nurbs_evaluate(vorder, vknot, iso, -v_first, 1, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (f32(p[0] / p[3]), f32(p[1] / p[3]), f32(p[2] / p[3])), dpdu, dpdv


def _clamp(x, lo, hi):
    if x < lo:
        x = lo
    if x > hi:
        x = hi
    return x


def nurbs(nu, nv, uorder, vorder, uknots, vknots, P=None, Pw=None, u0=None, u1=None, v0=None, v1=None, diceu=30, dicev=30):
    """create_nurbs + create_tesselated_mesh (nurbs.rs:175-406); errors as RefError with the reference's text."""
    if nu == -1:
        raise RefError('Must provide number of control points "nu" with NURBS shape.')
    if uorder == -1:
        raise RefError('Must provide u order "uorder" with NURBS shape.')
    uknots = [f32(k) for k in (uknots if uknots is not None else [])]
    if not uknots:
        raise RefError('Must provide u knot vector "uknots" with NURBS shape.')
    if len(uknots) != nu + uorder:
        raise RefError("Number of knots in u knot vector %d doesn't match sum of number of u control points %d and u order %d."
                       % (len(uknots), nu, uorder))
    if nv == -1:
        raise RefError('Must provide number of control points "nv" with NURBS shape.')
    if vorder == -1:
        raise RefError('Must provide v order "vorder" with NURBS shape.')
    vknots = [f32(k) for k in (vknots if vknots is not None else [])]
    if not vknots:
        raise RefError('Must provide v knot vector "vknots" with NURBS shape.')
    if len(vknots) != nv + vorder:
        raise RefError("Number of knots in v knot vector %d doesn't match sum of number of v control points %d and v order %d."
                       % (len(vknots), nv, vorder))
    if P is not None and len(P):
        pts, hom = [f32(x) for x in np.asarray(P, f32).reshape(-1)], False
    elif Pw is not None and len(Pw):
        pts, hom = [f32(x) for x in np.asarray(Pw, f32).reshape(-1)], True
    else:
        raise RefError('Must provide control points via "P" or "Pw" parameter to NURBS shape.')
    if not hom and len(pts) % 3 == 0:
        npts = len(pts) // 3
    elif hom and len(pts) % 4 == 0:
        npts = len(pts) // 4
    else:
        raise RefError("Number of control points must be multiple of 3 or 4.")
    if npts != nu * nv:
        raise RefError("Number of control points %d doesn't match nu * nv = %d * %d = %d." % (npts, nu, nv, nu * nv))
    if hom:
        cp = [tuple(pts[4 * i:4 * i + 4]) for i in range(npts)]
    else:
        cp = [(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], f32(1.0)) for i in range(npts)]
    u0x, u1x, v0x, v1x = uknots[uorder - 1], uknots[nu], vknots[vorder - 1], vknots[nv]
    u0 = _clamp(f32(u0) if u0 is not None else u0x, u0x, u1x)
    u1 = _clamp(f32(u1) if u1 is not None else u1x, u0x, u1x)
    v0 = _clamp(f32(v0) if v0 is not None else v0x, v0x, v1x)
    v1 = _clamp(f32(v1) if v1 is not None else v1x, v0x, v1x)
    diceu, dicev = max(int(diceu), 2), max(int(dicev), 2)

    def lerp(t, a, b):
        return f32(f32(f32(1.0) - t) * a) + f32(t * b)

    ueval = [f32(lerp(f32(f32(i) / f32(diceu - 1)), u0, u1)) for i in range(diceu)]
    veval = [f32(lerp(f32(f32(i) / f32(dicev - 1)), v0, v1)) for i in range(dicev)]
    Ps, Ns, uvs = [], [], []
    for v in range(dicev):
        for u in range(diceu):
            uu, vv = ueval[u], veval[v]
            uvs.append((uu, vv))
            p, dpdu, dpdv = nurbs_evaluate_surface(uorder, uknots, nu, uu, vorder, vknots, nv, vv, cp)
            Ps.append(p)
            Ns.append(normalize(cross(dpdu, dpdv)))
    tri = []
    vn = lambda u, v: v * diceu + u
    for v in range(dicev - 1):
        for u in range(diceu - 1):
            tri.append((vn(u, v), vn(u + 1, v), vn(u + 1, v + 1)))
            tri.append((vn(u, v), vn(u + 1, v + 1), vn(u, v + 1)))
    return {"P": np.array(Ps, f32), "N": np.array(Ns, f32), "uv": np.array(uvs, f32), "indices": np.array(tri, np.uint32).reshape(-1, 3)}


# ---------------------------------------------------------------- heightfield.rs
def heightfield(nu, nv, Pz):
    if nu == -1 or nv == -1:
        raise RefError('Must provide "nu" and "nv" parameters to heightfield shape.')
    if Pz is None:
        raise RefError("No vertex positions provided for heightfield shape.")
    z = np.asarray(Pz, f32).reshape(-1)
    if len(z) != nu * nv:
        raise RefError("Number of \"Pz\" values doesn't match resolution.")
    P, uv = np.zeros((nu * nv, 3), f32), np.zeros((nu * nv, 2), f32)
    for y in range(nv):
        for x in range(nu):
            pos = nu * y + x
            with np.errstate(invalid="ignore", divide="ignore"):
                xx, yy = f32(f32(x) / f32(nu - 1)), f32(f32(y) / f32(nv - 1))
            P[pos] = (xx, yy, z[pos])
            uv[pos] = (xx, yy)
    tri = np.zeros((2 * (nu - 1) * (nv - 1), 3), np.uint32)
    vert = lambda x, y: x + y * nu
    for y in range(nv - 1):
        for x in range(nu - 1):
            i = (x + y * (nu - 1)) * 2
            tri[i] = (vert(x, y), vert(x + 1, y), vert(x + 1, y + 1))
            tri[i + 1] = (vert(x, y), vert(x + 1, y + 1), vert(x, y + 1))
    return {"P": P, "N": None, "uv": uv, "indices": tri}
