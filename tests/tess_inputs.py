"""Inputs for the tessellated-shape tests: control meshes for "loopsubdiv", NURBS patches, height grids, a seeded generator of
manifold meshes and patches, and .pbrt text for them."""
import numpy as np


def tetrahedron():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return P, np.array([0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3], np.int64)


def icosahedron(radius=1.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    P = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    P = (P / np.linalg.norm(P, axis=1, keepdims=True) * radius).astype(np.float32)
    F = [0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
         3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1]
    return P, np.array(F, np.int64)


def grid(nx, ny, z=lambda x, y: 0.1 * ((7 * x + 3 * y) % 5), flip=lambda x, y: False):
    """An open (nx+1) x (ny+1) grid; flip(x, y) swaps the diagonal of a cell (corner valences 2 / 3, edges 4, interior 4 ... 8)."""
    P = np.array([[x, y, z(x, y)] for y in range(ny + 1) for x in range(nx + 1)], np.float32)
    I = []
    for y in range(ny):
        for x in range(nx):
            a, b, c, d = y * (nx + 1) + x, y * (nx + 1) + x + 1, (y + 1) * (nx + 1) + x + 1, (y + 1) * (nx + 1) + x
            I += [a, b, d, b, c, d] if flip(x, y) else [a, b, c, a, c, d]
    return P, np.array(I, np.int64)


def fan(n, closed=False):
    """A centre vertex with n rim vertices on a half (or full) circle: a boundary (or interior) vertex of valence n (+1)."""
    ang = np.linspace(0, 2 * np.pi if closed else np.pi, n, endpoint=not closed)
    P = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], 1)]).astype(np.float32)
    I = []
    for i in range(n if closed else n - 1):
        I += [0, 1 + i, 1 + (i + 1) % n]
    return P, np.array(I, np.int64)


def bipyramid(k, h=1.0):
    """k equator vertices and two apexes: apex valence k, equator valence 4 (closed)."""
    ang = 2 * np.pi * np.arange(k) / k
    P = np.concatenate([np.stack([np.cos(ang), np.sin(ang), 0.05 * np.sin(2 * ang)], 1), [[0, 0, h], [0, 0, -h * 0.8]]]).astype(np.float32)
    I = []
    for i in range(k):
        j = (i + 1) % k
        I += [i, j, k, j, i, k + 1]
    return P, np.array(I, np.int64)


def valence_mesh():
    """A closed mesh whose vertices have every valence from 3 to 12: bipyramids of 3 ... 12 equator vertices, side by side."""
    Ps, Is, base = [], [], 0
    for k in range(3, 13):
        P, I = bipyramid(k)
        Ps.append(P + np.float32([3.0 * (k - 3), 0, 0]))
        Is.append(I + base)
        base += len(P)
    return np.concatenate(Ps), np.concatenate(Is)


def _edges(F):
    out = {}
    for fi, f in enumerate(F):
        for k in range(3):
            out[(f[k], f[(k + 1) % 3])] = fi
    return out


def random_manifold(rng):
    """A closed or open manifold mesh with consistent winding: a base mesh, random edge flips (valences move between 3 and 10 or
    so), jitter, rotated faces, shuffled faces and relabelled vertices."""
    kind = rng.integers(0, 4)
    if kind == 0:
        P, I = icosahedron()
    elif kind == 1:
        P, I = bipyramid(int(rng.integers(3, 9)))
    elif kind == 2:
        P, I = grid(int(rng.integers(1, 4)), int(rng.integers(1, 4)), flip=lambda x, y: bool(rng.integers(0, 2)))
    else:
        P, I = fan(int(rng.integers(3, 9)), closed=False)
    F = [list(f) for f in I.reshape(-1, 3)]
    for _ in range(int(rng.integers(0, 12))):
        E = _edges(F)
        val = np.bincount(np.array(F).reshape(-1), minlength=len(P))
        inner = [(a, b) for (a, b) in E if (b, a) in E and a < b]
        if not inner:
            break
        a, b = inner[int(rng.integers(0, len(inner)))]
        f1, f2 = E[(a, b)], E[(b, a)]
        c = [v for v in F[f1] if v not in (a, b)][0]
        d = [v for v in F[f2] if v not in (a, b)][0]
        if c == d or (c, d) in E or (d, c) in E or val[a] <= 3 or val[b] <= 3:
            continue
        F[f1], F[f2] = [a, d, c], [d, b, c]
    P = P + rng.normal(0, 0.05, P.shape).astype(np.float32)
    F = [f[r:] + f[:r] for f, r in zip(F, rng.integers(0, 3, len(F)))]
    F = [F[i] for i in rng.permutation(len(F))]
    relabel = rng.permutation(len(P))
    P2 = np.empty_like(P)
    P2[relabel] = P
    I = relabel[np.array(F, np.int64).reshape(-1)]
    return P2.astype(np.float32), I.astype(np.int64)


def nurbs_sphere(r=1.0):
    """The rational quadratic sphere: 9 x 5 control points, double interior knots; dpdu vanishes at the poles."""
    s = 0.5 ** 0.5
    circ = [(1, 0, 1), (1, 1, s), (0, 1, 1), (-1, 1, s), (-1, 0, 1), (-1, -1, s), (0, -1, 1), (1, -1, s), (1, 0, 1)]
    arc = [(0, -1, 1), (1, -1, s), (1, 0, 1), (1, 1, s), (0, 1, 1)]          # (radius, z, w) from the south pole to the north
    Pw = []
    for (rr, z, wv) in arc:
        for (x, y, wu) in circ:
            w = wu * wv
            Pw += [r * x * rr * w, r * y * rr * w, r * z * w, w]
    return dict(nu=9, nv=5, uorder=3, vorder=3, uknots=[0, 0, 0, .25, .25, .5, .5, .75, .75, 1, 1, 1],
                vknots=[0, 0, 0, .5, .5, 1, 1, 1], Pw=np.array(Pw, np.float32))


def random_nurbs(rng):
    """A random patch: orders 2 ... 4, clamped or open knot vectors (repeats allowed), P or Pw with positive weights, ranges
    inside and outside the knot range, dice 2 ... 9."""
    kw = {}
    for d in "uv":
        order = int(rng.integers(2, 5))
        n = order + int(rng.integers(0, 4))
        if rng.random() < 0.5:
            inner = np.sort(np.round(rng.random(n - order), 2))
            knots = np.concatenate([np.zeros(order), inner, np.ones(order)])
        else:
            knots = np.cumsum(rng.choice([0.0, 0.5, 1.0, 1.25], n + order, p=[0.1, 0.3, 0.4, 0.2]))
        kw["n" + d], kw[d + "order"], kw[d + "knots"] = n, order, knots.astype(np.float32)
    ncp = kw["nu"] * kw["nv"]
    if rng.random() < 0.5:
        kw["P"] = rng.normal(0, 1, ncp * 3).astype(np.float32)
    else:
        pts = rng.normal(0, 1, (ncp, 3))
        w = rng.uniform(0.3, 2.0, (ncp, 1))
        kw["Pw"] = np.concatenate([pts * w, w], 1).astype(np.float32).reshape(-1)
    for k in ("u0", "u1", "v0", "v1"):
        if rng.random() < 0.3:
            kw[k] = float(np.float32(rng.uniform(-1, 6)))
    kw["diceu"], kw["dicev"] = int(rng.integers(0, 10)), int(rng.integers(2, 10))
    return kw


# ---- .pbrt text
def _arr(a, fmt=repr):
    return " ".join(fmt(float(x)) if fmt is repr else fmt(x) for x in np.asarray(a).reshape(-1))


def loopsubdiv_text(P, I, levels=None, extra=""):
    lv = "" if levels is None else ' "integer levels" [%d]' % levels
    return 'Shape "loopsubdiv"%s "integer indices" [%s] "point P" [%s]%s\n' % (lv, _arr(I, str), _arr(P), extra)


def nurbs_text(kw, extra=""):
    s = 'Shape "nurbs" "integer nu" [%d] "integer nv" [%d] "integer uorder" [%d] "integer vorder" [%d] "float uknots" [%s] "float vknots" [%s]' % (
        kw["nu"], kw["nv"], kw["uorder"], kw["vorder"], _arr(kw["uknots"]), _arr(kw["vknots"]))
    if kw.get("P") is not None:
        s += ' "point P" [%s]' % _arr(kw["P"])
    if kw.get("Pw") is not None:
        s += ' "point4 Pw" [%s]' % _arr(kw["Pw"])
    for k in ("u0", "u1", "v0", "v1"):
        if kw.get(k) is not None:
            s += ' "float %s" [%s]' % (k, repr(float(kw[k])))
    for k in ("diceu", "dicev"):
        if kw.get(k) is not None:
            s += ' "integer %s" [%d]' % (k, kw[k])
    return s + extra + "\n"


def heightfield_text(nu, nv, Pz, extra=""):
    return 'Shape "heightfield" "integer nu" [%d] "integer nv" [%d] "float Pz" [%s]%s\n' % (nu, nv, _arr(Pz), extra)
