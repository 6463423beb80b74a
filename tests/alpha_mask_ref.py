"""A float64 numpy reading of the float textures an alpha mask can be, written from the scene-file parameters and pbrt's formulas (the
bilinear image lookup of MIPMap level 0 with its three wrap modes, Checkerboard2DTexture, BilerpTexture, ScaleTexture, MixTexture, UVMapping2D)
and from nothing under oracle/ or pbrt-r3_amd/csrc/: an independent statement of where a mask that varies inside a triangle lets a ray through.
Shared by the CPU tests of the oracle (test_alpha_mask_oracle.py) and the GPU tests of the device (test_gpu_alpha_mask_parity.py).

An alpha mask is evaluated on the interaction the triangle's intersect returns: no ray differentials, every filter footprint zero.  An image
map (EWA or trilinear) is then the bilinear read of level 0; the closed-form checkerboard finds its filter box inside one cell and returns the
point value."""
import numpy as np

from helpers import scenes

f32 = np.float32
BAND = 1e-3          # |a| below this: float32 rounding of st (~1e-7) times the steepest image gradient (~128 per unit st) is ~1e-5; two decades of room
EDGE = 1e-4          # piecewise-constant textures: st closer than this to a cell edge
CAP = 0.01           # at most this share of the points may be left out


def noise_image(res, seed=5):
    """Values in [-1, 1], independent per texel: |bilinear| < 1e-3 on ~0.2 % of [0, 1]^2 (res 16: 0.19 %, res 64: 0.18 %)."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (res, res)).astype(f32)


class Ref:
    """A float texture: tex(sb) declares it in a SceneBuilder, val(u, v) -> (value float64, True where a discontinuity is within EDGE)."""
    def tex(self, sb):
        raise NotImplementedError

    def val(self, u, v):
        raise NotImplementedError


class UVMap:
    """UVMapping2D: s = su * u + du, t = sv * v + dv."""
    def __init__(self, uscale=1.0, vscale=1.0, udelta=0.0, vdelta=0.0):
        self.kw = dict(uscale=uscale, vscale=vscale, udelta=udelta, vdelta=vdelta)

    def st(self, u, v):
        return self.kw["uscale"] * u + self.kw["udelta"], self.kw["vscale"] * v + self.kw["vdelta"]


class Const(Ref):
    def __init__(self, c):
        self.c = float(c)

    def tex(self, sb):
        return self.c

    def val(self, u, v):
        return np.full(u.shape, self.c), np.zeros(u.shape, bool)


class Image(Ref):
    """Bilinear read of the full-resolution image: texel (i, j) has its centre at ((i + .5) / W, (j + .5) / H), row 0 is t = 0."""
    def __init__(self, img, wrap, trilinear=False, **kw):
        self.img, self.wrap, self.trilinear, self.map = np.asarray(img, np.float64), wrap, trilinear, UVMap(**kw)

    def tex(self, sb):
        return sb.texture_imagemap(sb.image_pyramid(self.img.astype(f32)), trilinear=self.trilinear, wrap=self.wrap, **self.map.kw)

    def texel(self, i, j):
        h, w = self.img.shape
        if self.wrap == "repeat":
            return self.img[np.mod(j, h), np.mod(i, w)]
        if self.wrap == "clamp":
            return self.img[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)]
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        return np.where(inside, self.img[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)], 0.0)

    def val(self, u, v):
        h, w = self.img.shape
        s, t = self.map.st(u, v)
        x, y = s * w - 0.5, t * h - 0.5
        i0, j0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
        dx, dy = x - i0, y - j0
        a = ((1 - dx) * (1 - dy) * self.texel(i0, j0) + (1 - dx) * dy * self.texel(i0, j0 + 1) + dx * (1 - dy) * self.texel(i0 + 1, j0) +
             dx * dy * self.texel(i0 + 1, j0 + 1))
        return a, np.zeros(u.shape, bool)


class Checker(Ref):
    """Checkerboard2DTexture: tex1 where floor(s) + floor(t) is even, else tex2; "none" and "closedform" agree at a zero footprint."""
    def __init__(self, t1, t2, aamode="closedform", **kw):
        self.t1, self.t2, self.aamode, self.map = t1, t2, aamode, UVMap(**kw)

    def tex(self, sb):
        return sb.texture_checkerboard(self.t1.tex(sb), self.t2.tex(sb), aamode=self.aamode, **self.map.kw)

    def val(self, u, v):
        s, t = self.map.st(u, v)
        (a1, e1), (a2, e2) = self.t1.val(u, v), self.t2.val(u, v)
        even = np.mod(np.floor(s) + np.floor(t), 2) == 0
        near = (np.abs(s - np.round(s)) < EDGE) | (np.abs(t - np.round(t)) < EDGE)
        return np.where(even, a1, a2), near | np.where(even, e1, e2)


class Bilerp(Ref):
    def __init__(self, v00, v01, v10, v11, **kw):
        self.v, self.map = (v00, v01, v10, v11), UVMap(**kw)

    def tex(self, sb):
        return sb.texture_bilerp(*self.v, **self.map.kw)

    def val(self, u, v):
        s, t = self.map.st(u, v)
        v00, v01, v10, v11 = self.v
        return (1 - s) * (1 - t) * v00 + (1 - s) * t * v01 + s * (1 - t) * v10 + s * t * v11, np.zeros(u.shape, bool)


class Scale(Ref):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def tex(self, sb):
        return sb.texture_scale(self.a.tex(sb), self.b.tex(sb))

    def val(self, u, v):
        (a, ea), (b, eb) = self.a.val(u, v), self.b.val(u, v)
        return a * b, ea | eb


class Mix(Ref):
    def __init__(self, a, b, amount):
        self.a, self.b, self.amount = a, b, amount

    def tex(self, sb):
        return sb.texture_mix(self.a.tex(sb), self.b.tex(sb), amount=self.amount.tex(sb))

    def val(self, u, v):
        (a, ea), (b, eb), (m, em) = self.a.val(u, v), self.b.val(u, v), self.amount.val(u, v)
        return (1 - m) * a + m * b, ea | eb | em


def cases():
    """name -> Ref.  Image maps of 16 and 64 texels under each wrap mode, with st scaled and shifted so that [-0.75, 1.75]^2 in uv runs well
    outside [0, 1]^2 in st; the checkerboard in both modes; bilerp; scale and mix over those."""
    im16, im64 = noise_image(16), noise_image(64)
    m = dict(uscale=1.3, vscale=0.8, udelta=0.21, vdelta=-0.37)
    m64 = dict(uscale=0.9, vscale=1.7, udelta=-0.4, vdelta=0.3)
    pm = (Const(0.5), Const(-0.5))
    # "black" reads exactly 0 outside the image, which is inside the band: the mask is 0.8 * image + 0.05, so that outside [0, 1]^2 it passes
    # everywhere (a wrongly wrapped or clamped read would not) and inside it follows the image
    lift = lambda img: Mix(img, Const(0.25), Const(0.2))
    c = {"image16_repeat": Image(im16, "repeat", **m), "image16_black": lift(Image(im16, "black", **m)), "image16_clamp": Image(im16, "clamp", **m)}
    c.update({"image64_repeat_trilinear": Image(im64, "repeat", trilinear=True, **m64), "image64_black_trilinear": lift(Image(im64, "black", trilinear=True, **m64)),
              "image64_clamp_trilinear": Image(im64, "clamp", trilinear=True, **m64)})
    c["image16_plain"] = lift(Image(im16, "black"))                            # st = uv: texel centres and edges of the point set land exactly
    c["checker_closedform"] = Checker(*pm, uscale=3.7, vscale=2.9, udelta=0.13, vdelta=0.41)
    c["checker_none"] = Checker(pm[1], pm[0], aamode="none", uscale=4.0, vscale=4.0)      # cell edges on the point set's own grid lines
    c["bilerp"] = Bilerp(-1.0, 0.5, 0.7, -0.6, uscale=0.8, vscale=0.9, udelta=0.1, vdelta=0.05)
    c["scale"] = Scale(c["image16_repeat"], c["checker_closedform"])           # (a product of two smooth masks spends too much of the plane near zero)
    c["mix"] = Mix(c["image64_clamp_trilinear"], c["checker_closedform"], Bilerp(0.1, 0.9, 0.8, 0.2))
    c["checker_of_images"] = Checker(c["image16_clamp"], c["image64_repeat_trilinear"], uscale=2.3, vscale=1.9)
    return c


LO, HI = -0.75, 1.75          # the planes cover [LO, HI]^2


def points(n=400000, seed=17):
    """(x, y): n uniform points of the plane and a lattice of the image's special places on both sides of [0, 1] -- every texel centre and
    texel edge of the 16-texel image from -11/32 to 55/32 (the last texels, where "repeat" blends texel 15 with texel 0 and "clamp" and
    "black" part, and a full period past 1), every third of the 64-texel image's from -6/128 to 198/128, uv = 0 and 1 -- all strictly
    inside the plane."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(LO + 0.01, HI - 0.01, (n, 2))
    k16 = np.arange(-11, 56) / 32.0            # i / 16 and (i + .5) / 16
    k64 = np.arange(-6, 200, 3) / 128.0        # a third of the 64-texel centres and edges
    g = np.unique(np.concatenate([k16, k64, [0.0, 1.0]]))
    assert LO < g.min() < 0.0 and 1.0 < g.max() < HI
    gx, gy = np.meshgrid(g, g)
    return np.concatenate([p, np.stack([gx.reshape(-1), gy.reshape(-1)], 1)]).astype(f32)


def plane_uv():
    """3 x 3 vertices over [LO, HI]^2 at z = 0, 8 large triangles, uv = (x, y): P, indices, uv."""
    g = np.linspace(LO, HI, 3)
    P = np.array([(x, y, 0.0) for y in g for x in g], f32)
    idx = []
    for j in range(2):
        for i in range(2):
            a = 3 * j + i
            idx += [a, a + 1, a + 4, a, a + 4, a + 3]
    return P, np.array(idx), P[:, :2].copy()


def plane_no_uv():
    """The same plane as two triangles without uv: each carries (0, 0), (1, 0), (1, 1) at its three vertices (triangle.rs:115-130)."""
    P = np.array([(LO, LO, 0), (HI, LO, 0), (HI, HI, 0), (LO, HI, 0)], f32)
    return P, np.array([0, 1, 2, 0, 2, 3])


def default_uv(x, y):
    """uv at (x, y) of plane_no_uv() in float64: b1 + b2 and b2 of the triangle the point lies in."""
    fx, fy = (x - LO) / (HI - LO), (y - LO) / (HI - LO)
    lower = fy <= fx                          # triangle (0, 1, 2): x = b1 + b2, y = b2; triangle (0, 2, 3): x = b1, y = b1 + b2 -> u = y, v = y - x
    return np.where(lower, fx, fy), np.where(lower, fy, fy - fx), np.abs(fx - fy) < 1e-5


def plane_scene(alpha, shadowalpha, uv=True):
    """The masked plane at z = 0 over an unmasked backdrop at z = -1 (a rejected candidate must leave the ray its length: it reaches the
    backdrop).  alpha / shadowalpha: Ref or None.  Returns the scene and the number of plane triangles (they come first)."""
    sb = scenes.SceneBuilder()
    sb.look_at((0.5, 0.5, 6), (0.5, 0.5, 0), (0, 1, 0))
    sb.camera_perspective(fov=40)
    sb.film(xresolution=8, yresolution=8)
    sb.sampler_sobol(pixelsamples=1)
    sb.integrator_path()
    kw = {}
    if alpha is not None:
        kw["alpha"] = alpha.tex(sb)
    if shadowalpha is not None:
        kw["shadowalpha"] = shadowalpha.tex(sb)
    if uv:
        P, idx, UV = plane_uv()
        sb.shape_trianglemesh(P, idx, uv=UV, **kw)
    else:
        P, idx = plane_no_uv()
        sb.shape_trianglemesh(P, idx, **kw)
    sb.shape_trianglemesh([-2, -2, -1, 3, -2, -1, 3, 3, -1, -2, 3, -1], [0, 1, 2, 0, 2, 3])
    return sb.build(), len(idx) // 3


def rays(pts):
    """Dropped straight onto the plane from z = 1."""
    o = np.concatenate([pts, np.ones((len(pts), 1), f32)], 1).astype(f32)
    d = np.tile(np.array([[0, 0, -1]], f32), (len(pts), 1))
    return o, d


def check_plane(tracer, alpha, shadowalpha, uv, label):
    """tracer: an OracleScene-like pair of calls (closest(o, d, tmax) -> hits, any(o, d, tmax) -> occlusion) over plane_scene(alpha, shadowalpha, uv).
    Holds it to the float64 masks at every point outside the band, asserts the cap on what is left out and prints the share."""
    closest, any_hit, n_plane = tracer
    pts = points()
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    if uv:
        u, v, seam = x, y, np.zeros(len(x), bool)
    else:
        u, v, seam = default_uv(x, y)
    a, ea = alpha.val(u, v)
    s, es = shadowalpha.val(u, v) if shadowalpha is not None else (np.ones(len(x)), np.zeros(len(x), bool))
    out_a = (np.abs(a) < BAND) | ea | seam
    out_s = out_a | (np.abs(s) < BAND) | es
    print("\n[%s] left out: closest %.3f %%, any-hit %.3f %% of %d points; %.1f %% pass alpha" % (label, 100 * out_a.mean(), 100 * out_s.mean(), len(pts), 100 * (a > 0).mean()))
    assert out_a.mean() <= CAP and out_s.mean() <= CAP
    assert isinstance(alpha, Const) or min(((a > 0) & ~out_a).sum(), ((a <= 0) & ~out_a).sum()) >= 1000      # the mask varies: both answers are asked for
    o, d = rays(pts)
    h = closest(o, d, np.full(len(pts), np.inf, f32))
    assert np.all(h["prim"] >= 0)                                  # the plane, or the backdrop behind it
    on_plane = h["prim"] < n_plane
    bad = (on_plane != (a > 0)) & ~out_a
    assert not bad.any(), (label, int(bad.sum()), pts[bad][:5], a[bad][:5])
    want_t = np.where(on_plane, 1.0, 2.0)
    assert np.allclose(h["t"], want_t, rtol=1e-6, atol=0.0)
    occ = np.asarray(any_hit(o, d, np.full(len(pts), 1.5, f32))).astype(bool)          # the backdrop is out of reach
    bad = (occ != ((a > 0) & (s > 0))) & ~out_s
    assert not bad.any(), (label, int(bad.sum()), pts[bad][:5], a[bad][:5], s[bad][:5])
