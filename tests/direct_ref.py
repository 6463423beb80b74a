"""Float64 truth for the place where the truths below it are COMPOSED: next-event estimation with multiple importance sampling at the
first vertex of a camera path, for `path` at maxdepth 1 and `directlighting` "one" and "all" at maxdepth 1, in scenes lit by diffuse area lights on
triangles.  Numpy only; it imports neither the oracle nor the package.

What is restated (file:line of the reference)
  * core/integrator/sample_lights.rs:129-176   uniform_sample_one_light_surface: the pick, its pdf, the division by it; :80-127 the same
    without a distribution (`directlighting` "one": index min(u n, n - 1), pdf 1 / n)
  * core/integrator/sample_lights.rs:330-453   estimate_direct_surface: flags ALL & ~SPECULAR; the light half f |cos| Li w / light_pdf behind
    the shadow test, taken only for non-black f; the BSDF half f |cos| Le w / scattering_pdf, where light_pdf is Shape::pdf_from at the point
    the sampled direction MEETS the picked light's shape (core/shape/shape.rs:40-54: not at the light half's sample), the early return at
    light_pdf == 0, no weight for a specular lobe, and Le only if the probe's closest hit is the picked light (:430-442)
  * core/sampling/sampling.rs:168-172          power_heuristic: f^2 / (f^2 + g^2)
  * core/sampling/distribution.rs:12-31, :88-102   find_interval_cdf and Distribution1D::sample_discrete
  * core/lightdistrib/create_light_sample_distribution.rs:23-29 ("uniform" with more than one light IS "spatial"), power.rs:9-17,
    spatial.rs:84-196 (voxel, 128 probes of radical inverses in bases 2 3 5 7 11, li.y() / pdf, the 0.001 floor)
  * lights/diffuse.rs:65-68 power, :70-87 sample_li, :89-94 pdf_li, :156-162 l (facing and two-sidedness)
  * integrators/path.rs:85-103 Le at the camera hit and, after a specular bounce, at the next hit -- added at maxdepth 1 before the depth test
    breaks the loop; :119 no estimate at a vertex without a non-specular lobe (it then draws NO pick and no u_light / u_scattering: the
    bounce's two dimensions follow the camera's five directly); :141-167 the bounce, beta = f |cos| / pdf
  * integrators/directlighting.rs:76-109       Le at the hit plus the estimate; no bounce at maxdepth 1

It composes the truths that exist and does not re-derive them: bsdf_ref.BSDF (eval and sample with their bounds and undecided marks;
mix_ref.BSDF for a Material "mix" and disney_ref.BSDF for a Material "disney", which have the same interface),
geometry_ref.light_truth (the light's sample, solid-angle pdf, Li, pdf_rel, p_bound) and closest_hits (hits and occlusion with rules (a) to
(d)), delta_light_ref's distribution_pdf / spatial_voxels / voxel_of / PROBES, and aov_ref's error class E, in which the composition's own
arithmetic runs: in float64 it is the truth with a first-order bound per sample, in float32 it is the reference's arithmetic (the calibration).

Sphere lights: the cone sample is geometry_ref.light_truth's; the reference has no Sphere::pdf_from, so the BSDF half weighs a sphere light
by the default Shape::pdf_from, distance^2 / (|cos| area) at the probe's point on the sphere (shape.rs:40-54) -- not the cone's density.
A constant infinite light after the emitters is the last light of the list: its sample, pdf_li and le are restated here (infinite.rs).
Not restated: Russian roulette (bounces > 3), anything past the first vertex, clipped or transformed sphere lights, cylinder lights, partial or rotated disk lights (a whole translated disk is quadric_ref's), image-mapped or transformed infinite lights, instances, textured parameters.  Inputs are exact float32 numbers: the camera ray and
the sampler's dimensions 5 .. 11 of the camera sample.

The vertex.  The camera hit is geometry_ref's; its point is o + t d in float64, known to p_err = 16 eps extent (a float32 point rebuilt from
barycentrics: 7 roundings on terms below the extent, doubled).  Rays leave it from p_err off the surface on the side they head for -- the
reference's spawn_ray offsets by its own error bound, of the same size -- so that the vertex's own triangle is a decided miss.

Undecided samples are left out and counted, one reason each (REASONS, in this order):
  camera  the camera hit is undecided by rules (a) to (d)
  shadow  the shadow segment is, or it changes its answer when moved sideways by its end points' bounds
  probe   the probe (or the ray after a specular bounce) is
  edge    the probe's closest primitive changes when origin and direction move by their bounds (the shared diagonal of an emissive quad is
          such an edge)
  pick    u is within 2 ulp, or within the CDF's own bound, of a CDF breakpoint; the point is within p_err of a voxel face; a probe of the
          voxel's distribution sees a light edge-on
  bsdf    an evaluation or a sample the BSDF truth marks undecided or left_out()
  cos     |cos| at the surface or at the light below COS_FLOOR = 2e-3 (the floor of the BSDF tests' draws)
  wide    the sum's bound passes REL_CAP = 1e-3 of a channel's value
"""
import numpy as np

import bsdf_ref as R
import delta_light_ref as dref
import disney_ref
import geometry_ref as G
import mix_ref
import quadric_ref as Q
from aov_ref import E

EPS = G.EPS
COS_FLOOR = 2e-3
REL_CAP = 1e-3
ENV = -1                      # the kind of the infinite light in Setup.lights
REASONS = ("camera", "shadow", "probe", "edge", "pick", "bsdf", "cos", "wide")
KINDS = ("light half unoccluded", "light half occluded", "probe meets the picked light", "probe meets another light",
         "probe meets no emitter")
MESH_HAS_UV = 32
PI32 = R.PI
SHADOW_EPSILON = float(np.float32(0.0001))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _e(v, e, dtype):
    return E(np.asarray(v, np.float64).astype(dtype), np.asarray(e, np.float64))


def _as(a, dt):
    """A quantity an implementation holds in float32 (a hit point, a direction), as the run's dtype holds it."""
    return np.asarray(a, np.float64).astype(dt).astype(np.float64)


def _masked(x, m):
    """x where m, an exact zero elsewhere."""
    with np.errstate(all="ignore"):
        return E(np.where(m, x.v, 0), np.where(m, x.e, 0.0))


def _tangents(d):
    """Two unit vectors across each direction."""
    a = np.where((np.abs(d[:, 0]) > np.abs(d[:, 1]))[:, None], np.stack([-d[:, 2], 0 * d[:, 0], d[:, 0]], 1), np.stack([0 * d[:, 0], d[:, 2], -d[:, 1]], 1))
    a = _unit(a)
    return a, _unit(np.cross(d, a))


def sphere_sample32(centre, r, ref, u):
    """Sphere::sample_from seen from outside (sphere.rs:323-377) in float32 arithmetic, for the float32 run: (wi, pdf) as float64 copies
    of the float32 results.  The float64 form and its bounds are geometry_ref.light_truth's."""
    f = np.float32
    c, ref, u = np.asarray(centre, f), np.asarray(ref, f), np.asarray(u, f)
    with np.errstate(all="ignore"):
        w = c - ref
        d2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]).astype(f)
        wc = (w / np.sqrt(d2)[:, None]).astype(f)
        big = np.abs(wc[:, 0]) > np.abs(wc[:, 1])
        la, lb = np.sqrt(wc[:, 0] * wc[:, 0] + wc[:, 2] * wc[:, 2]), np.sqrt(wc[:, 1] * wc[:, 1] + wc[:, 2] * wc[:, 2])
        zero = np.zeros_like(la)
        x = np.where(big[:, None], np.stack([-wc[:, 2] / la, zero, wc[:, 0] / la], 1), np.stack([zero, wc[:, 2] / lb, -wc[:, 1] / lb], 1)).astype(f)
        y = np.cross(wc, x).astype(f)
        s2 = (f(r) * f(r) / d2).astype(f)
        smax = np.sqrt(s2)
        cmax = np.sqrt(np.maximum(f(0), f(1) - s2))
        ct = ((cmax - f(1)) * u[:, 0] + f(1)).astype(f)
        st2 = (f(1) - ct * ct).astype(f)
        small = s2 < f(0.00068523)
        st2 = np.where(small, s2 * u[:, 0], st2).astype(f)
        ct = np.where(small, np.sqrt(f(1) - st2), ct).astype(f)
        ca = (st2 / smax + ct * np.sqrt(np.maximum(f(0), f(1) - st2 / smax / smax))).astype(f)
        sa = np.sqrt(np.maximum(f(0), f(1) - ca * ca)).astype(f)
        phi = (u[:, 1] * f(2) * f(np.pi)).astype(f)
        n = ((sa * np.cos(phi))[:, None] * -x + (sa * np.sin(phi))[:, None] * -y + ca[:, None] * -wc).astype(f)
        pw = (c + f(r) * n).astype(f)
        wi = pw - ref
        wi = (wi / np.sqrt((wi * wi).sum(1, dtype=f))[:, None]).astype(f)
        pdf = (f(1) / (f(2) * f(np.pi) * (f(1) - cmax))).astype(f)
    return wi.astype(np.float64), pdf.astype(np.float64)


class Setup:
    """A scene description's triangles, lights and material parameters.  params: material index -> the parameters as the scene names them
    (bsdf_cases.CASES).  world_bound: the six numbers the scene's info reports (the spatial distribution's grid)."""

    def __init__(self, sd, params, world_bound, extent=4.0):
        quadric = any(int(sd.buffers["spheres"][i].kind) != Q.SHAPE_SPHERE for i in range(sd.desc.n_spheres))
        self.sc = sc = Q.Scene(sd) if quadric else G.Scene(sd)                          # a disk: quadric_ref's scene, hits and light samples
        self.closest_hits = Q.closest_hits if quadric else G.closest_hits
        assert not sc.instances, "world triangles and spheres only"
        self.p_err = 16 * EPS * extent
        self.params = params
        self.wb = np.array(list(world_bound), np.float64)
        tm = np.asarray(sd.buffers["tri_mesh"]).astype(np.int64).reshape(-1)
        meshes = sd.buffers["meshes"]
        self.tri_material = np.array([int(meshes[int(m)].material) for m in tm])
        uv = sd.buffers.get("UV")
        self.UV = None if uv is None else np.asarray(uv, np.float32).astype(np.float64).reshape(-1, 2)
        self.lights = sc.lights()
        # a constant LightSource "infinite" read after every emitter: the last light of the list (lights/infinite.rs).  Its 1 x 1 map gives
        # a 2 x 2 sampling image of four equal cells (:69-91): the distribution is uniform in (u, v) and its density is 1
        self.env = -1
        inf = list(getattr(sd, "infinite_lights", None) or [])
        if inf:
            assert len(inf) == 1 and inf[0].light_index == len(self.lights), "one infinite light, after the emitters"
            img = sd.buffers["images"][inf[0].image]
            assert img.width == 1 and img.height == 1 and np.array_equal(np.array(list(inf[0].light_to_world)).reshape(4, 4), np.eye(4))
            L = np.asarray(sd.buffers["image_texels"][inf[0].image], np.float32).astype(np.float64).reshape(-1)[:3]
            self.env = len(self.lights)
            self.lights = self.lights + [(ENV, -1, L, False)]
        c = 0.5 * (self.wb[:3] + self.wb[3:])
        self.world_radius = float(np.linalg.norm(self.wb[3:] - c))                      # Bounds3::bounding_sphere
        self.light_tri = np.array([i if k == G.TRIANGLE else -1 for k, i, _, _ in self.lights])
        self.light_sphere = np.array([i if k == G.SPHERE else -1 for k, i, _, _ in self.lights])
        self.light_of_prim = np.full(len(sc.prim_list) + 1, -1)
        for j, (k, i, _, _) in enumerate(self.lights):
            if k == ENV:
                continue
            self.light_of_prim[sc.tri_prim[i] if k == G.TRIANGLE else sc.sphere_prim[i]] = j
        self.light_disk = np.array([i if k == G.SPHERE and getattr(sc.spheres[i], "kind", 0) == Q.SHAPE_DISK else -1 for k, i, _, _ in self.lights])
        self.light_sphere = np.where(self.light_disk >= 0, -1, self.light_sphere)
        for sp in sc.spheres:                       # a sphere light is a whole sphere under a translation: its world sphere is the shape
            if getattr(sp, "kind", 0) == Q.SHAPE_DISK:                                  # a disk light is a whole disk under a translation
                assert sp.full_phi and sp.ri == 0.0 and np.array_equal(sp.o2w[:3, :3], np.eye(3))
                continue
            assert sp.full_phi and sp.zmin == -sp.r and sp.zmax == sp.r and np.array_equal(sp.o2w[:3, :3], np.eye(3)) and not sp.reverse
        self._bsdf, self._frames = {}, {}

    def bsdf(self, material, dtype):
        if (material, dtype) not in self._bsdf:
            prm = self.params[material]                                                 # mix and disney: their own truths, on bsdf_ref's interface
            cls = {"mix": mix_ref.BSDF, "disney": disney_ref.BSDF}.get(prm["type"], R.BSDF)
            self._bsdf[(material, dtype)] = cls(prm, dtype)
        return self._bsdf[(material, dtype)]

    def tri_normal_area(self, tri):
        """Triangle::intersect's n (triangle.rs:240-245) and Triangle::area (:579-588)."""
        sc = self.sc
        p0, p1, p2 = (sc.P[sc.idx[tri, k]] for k in range(3))
        n = np.cross(p0 - p2, p1 - p2)
        area = 0.5 * np.linalg.norm(n)
        n = n / np.linalg.norm(n)
        f = int(sc.tri_flags[tri])
        if bool(f & G.MESH_REVERSE) ^ bool(f & G.MESH_SWAPS):
            n = -n
        return n, area

    def light_area(self, j):
        """Shape::area of light j: Triangle::area; Sphere::area = phi_max r (z_max - z_min) (sphere.rs)."""
        if j == self.env:                           # power is L pi r^2 (infinite.rs:101-106): an "area" of r^2 in diffuse.rs's form
            return self.world_radius ** 2
        if self.light_tri[j] >= 0:
            return self.tri_normal_area(int(self.light_tri[j]))[1]
        if self.light_disk[j] >= 0:
            return self.sc.spheres[int(self.light_disk[j])].area                        # disk.rs: phi_max / 2 (r^2 - r_i^2)
        sp = self.sc.spheres[int(self.light_sphere[j])]
        return sp.phimax * sp.r * (sp.zmax - sp.zmin)

    def light_sample(self, j, ref, u):
        """Light::sample_li of light j in geometry_ref.light_truth's form.  The infinite light (infinite.rs:121-158): theta = v pi,
        phi = u 2 pi, pdf = 1 / (2 pi^2 sin theta), the far end 2 world radii along wi."""
        if j != self.env and self.light_disk[j] >= 0:
            return Q.light_truth(self.sc, j, ref, u, quadrature=False)
        if j != self.env:
            return G.light_truth(self.sc, j, ref, u, solid_angle=False)
        u = np.asarray(u, np.float32).astype(np.float64).reshape(-1, 2)
        ref = np.asarray(ref, np.float64).reshape(-1, 3)
        n = len(u)
        theta, phi = u[:, 1] * PI32, u[:, 0] * 2.0 * PI32
        st = np.clip(np.sin(theta), 0.0, 1.0)
        wi = np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)], 1)
        with np.errstate(all="ignore"):
            pdf = np.where(st > 0, 1.0 / (2.0 * PI32 * PI32 * st), 0.0)
            # theta and phi carry 2 roundings, sin and cos 2 ulp each; the density weighs sin theta's absolute error by 1 / sin theta;
            # the map's pdf and the sampled (u, v) pass the distribution's two divisions
            rel = 8 * EPS + 8 * EPS / np.maximum(st, 1e-30)
        dist = np.full(n, 2.0 * self.world_radius)
        return {"p": ref + wi * dist[:, None], "wi": wi, "pdf": pdf, "li": np.tile(self.lights[j][2], (n, 1)), "valid": st > 0,
                "p_bound": 16 * EPS * dist, "pdf_rel": rel, "cos": np.ones(n), "dist": dist}

    def light_meet(self, j, o, w):
        """Where rays o + t w (t > 0) meet light j's shape first, as Shape::pdf_from (shape.rs:40-54) intersects it alone: (distance,
        |cos| at the shape, its normal . -w / |w| signed, the scale the point's error has against: the distance, or a sphere's radius)."""
        ln = np.linalg.norm(w, axis=1)
        with np.errstate(all="ignore"):
            if j == self.env:                       # pdf_li (infinite.rs:160-177) is 1 / (2 pi^2 sin theta): as distance^2 / (|cos| area) it has
                st = np.sqrt(np.maximum(0.0, 1.0 - (w[:, 2] / ln) ** 2))                # distance^2 = 1, |cos| = sin theta, area = 2 pi^2
                return np.ones(len(w)), st, st, np.full(len(w), np.inf)
            if self.light_tri[j] >= 0:
                tri = int(self.light_tri[j])
                nl, _ = self.tri_normal_area(tri)
                c = -(w @ nl) / ln
                dist = np.abs((self.sc.P[self.sc.idx[tri, 0]] - o) @ nl) / np.abs(c)
                return dist, np.abs(c), c, dist
            if self.light_disk[j] >= 0:             # the plane z = height of a translated disk, its normal +z, turned by ReverseOrientation
                dk = self.sc.spheres[int(self.light_disk[j])]
                c = -(w[:, 2] / ln) * (-1.0 if dk.reverse else 1.0)
                dist = np.abs(dk.o2w[2, 3] + dk.h - o[:, 2]) / np.abs(c)
                return dist, np.abs(c), c, dist
            sp = self.sc.spheres[int(self.light_sphere[j])]
            oc = o - sp.o2w[:3, 3]
            a, b, cc = (w * w).sum(1), 2.0 * (w * oc).sum(1), (oc * oc).sum(1) - sp.r * sp.r
            t0 = (-b - np.sqrt(b * b - 4.0 * a * cc)) / (2.0 * a)
            nn = (oc + t0[:, None] * w) / sp.r
            c = -(nn * w).sum(1) / ln
            return t0 * ln, np.abs(c), c, np.minimum(t0 * ln, sp.r)

    def frame(self, tri):
        """BSDF::new's frame (bsdf.rs:40-53) on a triangle without N or S: ns = n, ss = normalize(dpdu), ts = cross(ns, ss), dpdu from
        get_dpdu_dpdv (triangle.rs:132-186) with the default uvs (0,0) (1,0) (1,1)."""
        if tri not in self._frames:
            sc = self.sc
            assert not (int(sc.tri_flags[tri]) & (G.MESH_HAS_N | 16)), "no shading normals or tangents"
            p = [sc.P[sc.idx[tri, k]] for k in range(3)]
            if (int(sc.tri_flags[tri]) & MESH_HAS_UV) and self.UV is not None:
                t = [self.UV[sc.idx[tri, k]] for k in range(3)]
            else:
                t = [np.array(x) for x in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0))]
            dp02, dp12, duv02, duv12 = p[0] - p[2], p[1] - p[2], t[0] - t[2], t[1] - t[2]
            det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
            assert abs(det) > 1e-6
            dpdu = (duv12[1] * dp02 - duv02[1] * dp12) / det
            ns, _ = self.tri_normal_area(tri)
            ss = _unit(dpdu)
            self._frames[tri] = (ss, np.cross(ns, ss), ns)
        return self._frames[tri]

    # ------------------------------------------------------------------------------------------------------------ the pick
    def pick_pdfs(self, p, strategy, dtype=np.float64):
        """Per point the pdf of every light (n, L), its relative bound (n, L) and `near` (n,): the lookup itself is undecided.  In a
        float32 run the 128 terms of a voxel are summed one after the other in float32, as compute_distribution does."""
        dt = np.dtype(dtype).type
        n, nl = len(p), len(self.lights)
        if strategy == "one" or (strategy == "uniform" and nl == 1):          # sample_lights.rs:104-110; uniform.rs
            return np.full((n, nl), 1.0 / nl), np.full((n, nl), 2 * EPS), np.zeros(n, bool)
        if strategy == "power":                                               # power.rs:9-17, diffuse.rs:65-68
            y = [dref.luminance(L * ((2.0 if two else 1.0) * self.light_area(j) * PI32)) for j, (_, _, L, two) in enumerate(self.lights)]
            return np.tile(dref.distribution_pdf(y), (n, 1)), np.full((n, nl), 16 * EPS), np.zeros(n, bool)
        assert strategy in ("spatial", "uniform"), strategy
        lo_w, hi_w = self.wb[:3], self.wb[3:]
        vox = dref.spatial_voxels(lo_w, hi_w)
        v = np.array(vox, np.float64)
        pi = dref.voxel_of(p, lo_w, hi_w, vox)
        ext = np.where(hi_w > lo_w, hi_w - lo_w, 1.0)
        fr = (p - lo_w) / ext * v
        face = np.round(fr)
        near = ((np.abs(fr - face) * ext / v <= 4 * self.p_err) & (face > 0) & (face < v)).any(1)
        keys, inv = np.unique(pi, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        nv = len(keys)
        lo = lo_w + keys / v * (hi_w - lo_w)
        hi = lo_w + (keys + 1) / v * (hi_w - lo_w)
        po = (lo[:, None, :] + dref.PROBES[None, :, :3] * (hi - lo)[:, None, :]).reshape(-1, 3)
        u = np.tile(dref.PROBES[:, 3:5], (nv, 1))
        po_err = 4 * EPS * np.abs(self.wb).max()
        contrib, rel, near_v = np.zeros((nv, nl)), np.zeros((nv, nl)), np.zeros(nv, bool)
        for j in range(nl):
            t = self.light_sample(j, po, u)
            with np.errstate(all="ignore"):
                ok = t["valid"] & (t["pdf"] > 0)
                term = np.where(ok, dref.luminance(t["li"]) / np.where(ok, t["pdf"], 1.0), 0.0)
                term_rel = t["pdf_rel"] + 3 * po_err / t["dist"] / np.abs(t["cos"]) + 16 * EPS
                edge_on = (np.abs(t["cos"]) < 1e-3) & (t["dist"] > 0)
            contrib[:, j] = np.cumsum(term.astype(dt).reshape(nv, 128), axis=1, dtype=dt)[:, -1] if dt is np.float32 else term.reshape(nv, 128).sum(1)
            with np.errstate(all="ignore"):
                rel[:, j] = np.where(contrib[:, j] > 0, np.where(ok, term_rel * term, 0.0).reshape(nv, 128).sum(1) / contrib[:, j] + 128 * EPS, 0.0)
            near_v |= edge_on.reshape(nv, 128).any(1)
        avg = contrib.sum(1) / (128 * nl)
        floor = np.where(avg > 0, 0.001 * avg, 1.0)
        func = np.maximum(floor[:, None], contrib).astype(dt)
        pdf = (func / np.cumsum(func, axis=1, dtype=dt)[:, -1:]).astype(np.float64)
        rel = rel + rel.max(1, keepdims=True) + (2 * nl + 4) * EPS
        return pdf[inv], rel[inv], near | near_v[inv]

    def pick(self, pdf, rel, u):
        """find_interval_cdf (distribution.rs:12-31): the last i with cdf[i] <= u.  Returns (index, undecided)."""
        u = np.asarray(u, np.float32).astype(np.float64)
        cdf = np.cumsum(pdf, 1)[:, :-1]
        idx = (u[:, None] >= cdf).sum(1)
        margin = 2 * 2 * EPS * np.maximum(u[:, None], 2.0 ** -24) + rel.max(1, keepdims=True) * cdf
        return idx, (np.abs(u[:, None] - cdf) <= margin).any(1)

    # ------------------------------------------------------------------------------------------------------------ tracing
    def trace(self, o, d, tmax, ss, ts, o_spread, d_spread, moved=True):
        """closest_hits, and whether the answer holds when the ray moves: the origin by o_spread within the surface it leaves, the
        direction by d_spread across itself.  Returns (hits, undecided by a rule, changed under the move)."""
        h = self.closest_hits(self.sc, o, d, tmax)
        changed = np.zeros(len(o), bool)
        a, b = _tangents(_unit(d))
        a = np.where(((a * ss).sum(1) < 0)[:, None], -a, a)
        b = np.where(((b * ts).sum(1) < 0)[:, None], -b, b)
        # a moved segment ends that much short of its far end: moved sideways, the end of a segment to a curved light would dip into the
        # light's own surface, which the reference's target offset (interaction.rs:118-127) keeps it out of
        with np.errstate(all="ignore"):
            tmax_moved = np.where(np.isfinite(tmax), tmax - 4.0 * o_spread / np.linalg.norm(d, axis=1), tmax)
        for so, sd_ in ((ss, a), (-ss, -a), (ts, b), (-ts, -b)) if moved else ():
            h2 = self.closest_hits(self.sc, o + np.sqrt(2.0) * o_spread[:, None] * so, d + np.sqrt(2.0) * d_spread[:, None] * sd_, tmax_moved)
            changed |= (h2["prim"] != h["prim"]) | (h2["occluded"] != h["occluded"]) | (h2["rule"] != 0)
        return h, h["rule"] != 0, changed

    def le_at(self, h, w, o=None):
        """isect.le(w) of closest hits h of rays from o along -w (diffuse.rs:156-162): (Le (n, 3), |cos| at the emitter, emitter hit).
        o is needed only where a sphere may be met."""
        n = len(w)
        le, cos = np.zeros((n, 3)), np.ones(n)
        lj = self.light_of_prim[h["prim"]]
        for j in np.unique(lj[lj >= 0]):
            rows = np.nonzero(lj == j)[0]
            _, _, L, two = self.lights[j]
            if self.light_tri[j] >= 0:
                c = w[rows] @ self.tri_normal_area(int(self.light_tri[j]))[0]
            else:
                c = self.light_meet(j, o[rows], -w[rows])[2]
            cos[rows] = np.abs(c)
            le[rows] = np.where((two | (c > 0))[:, None], L[None, :], 0.0)
        return le, cos, lj >= 0

    # ------------------------------------------------------------------------------------------------------------ one estimate
    def estimate(self, tri, p, wo_w, j, u_light, u_scat, dtype=np.float64, mis=True, bsdf_half=True, spread=True):
        """estimate_direct_surface of light j[i] at point p[i] of world triangle tri[i] seen from the unit direction wo_w[i].  mis=False:
        both weights are 1 (with bsdf_half=False the light-only estimator).  Returns the dict of the two halves as E per channel, the
        reasons (n, len(REASONS)) and the kinds (n, len(KINDS))."""
        n = len(p)
        dt = np.dtype(dtype).type
        sc = self.sc
        reasons = np.zeros((n, len(REASONS)), bool)
        kinds = np.zeros((n, len(KINDS)), bool)
        R_ = {k: i for i, k in enumerate(REASONS)}
        ss, ts, ns = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        z = lambda *s: np.zeros((n,) + s)
        # light half
        a_f, a_fe, a_bp, a_bpe, a_cos, a_cose = z(3), z(3), z(), z(), z(), z()
        a_lp, a_lpe, a_li, a_ok = np.ones(n), z(), z(3), np.zeros(n, bool)
        a_end = p.copy()
        a_pb = z()
        # BSDF half
        b_wil, b_wile = np.tile([0.0, 0.0, 1.0], (n, 1)), z(3)
        b_wi, b_wie, b_ok, b_spec = np.tile([0.0, 0.0, 1.0], (n, 1)), z(), np.zeros(n, bool), np.zeros(n, bool)
        side_a, side_b = np.ones(n), np.ones(n)
        for t_ in np.unique(tri):
            fr = self.frame(int(t_))
            m = tri == t_
            ss[m], ts[m], ns[m] = fr
        wo_l = np.stack([(wo_w * ax).sum(1) for ax in (ss, ts, ns)], 1)
        reasons[:, R_["cos"]] |= np.abs(wo_l[:, 2]) < COS_FLOOR
        for t_, j_ in {(int(a), int(b)) for a, b in zip(tri, j)}:
            rows = np.nonzero((tri == t_) & (j == j_))[0]
            b = self.bsdf(int(self.tri_material[t_]), dt)
            # wo = -d of a float32 unit vector brought to the frame by three dot products on exact axes
            wo = [_e(wo_l[rows, c], 6 * EPS, dt) for c in range(3)]
            lt = self.light_sample(j_, p[rows], u_light[rows])
            ok = lt["valid"] & (lt["pdf"] > 0) & (lt["li"].sum(1) > 0)                   # :355-356
            with np.errstate(all="ignore"):
                wi_err = (lt["p_bound"] + self.p_err) / lt["dist"] + 4 * EPS
                lp_rel = lt["pdf_rel"] + 3 * self.p_err / lt["dist"] / np.abs(lt["cos"])
            wi_w, lpdf = lt["wi"], lt["pdf"]
            if dt is np.float32 and self.light_sphere[j_] >= 0:                        # the float32 run samples the cone in float32
                sp = sc.spheres[int(self.light_sphere[j_])]
                wi32, pdf32 = sphere_sample32(sp.o2w[:3, 3], sp.r, p[rows], u_light[rows])
                wi_w, lpdf = np.where(ok[:, None], wi32, wi_w), np.where(ok, pdf32, lpdf)
            wi_l = np.stack([(wi_w * ax[rows]).sum(1) for ax in (ss, ts, ns)], 1)
            wi_l = _as(np.where(ok[:, None], wi_l, [0.0, 0.0, 1.0]), dt)
            wi = [_e(wi_l[:, c], np.where(ok, wi_err + 4 * EPS, 0.0), dt) for c in range(3)]
            with np.errstate(all="ignore"):
                v = b.eval(wo, wi, R.NOSPEC)
            reasons[rows, R_["bsdf"]] |= ok & v.left_out()
            reasons[rows, R_["cos"]] |= ok & ((np.abs(wi_l[:, 2]) < COS_FLOOR) | (np.abs(lt["cos"]) < COS_FLOOR))
            reasons[rows, R_["cos"]] |= (np.abs(lt["cos"]) < COS_FLOOR) & (lt["dist"] > 0)      # facing, and with it None, is not decided
            a_ok[rows] = ok
            a_f[rows], a_fe[rows], a_bp[rows], a_bpe[rows] = v.f, v.f_e, v.pdf, v.pdf_e
            a_cos[rows], a_cose[rows] = np.abs(wi_l[:, 2]), wi_err + 4 * EPS
            a_lp[rows], a_lpe[rows] = np.where(ok, lpdf, 1.0), np.where(ok, lt["pdf"] * lp_rel, 0.0)
            a_li[rows] = np.where(ok[:, None], lt["li"], 0.0)
            a_end[rows], a_pb[rows] = lt["p"], lt["p_bound"]
            side_a[rows] = np.where(wi_l[:, 2] < 0, -1.0, 1.0)
            if not bsdf_half:
                continue
            wo32 = wo_l[rows].astype(np.float32)
            with np.errstate(all="ignore"):
                s = b.sample(wo32, u_scat[rows], R.NOSPEC)                              # :402-411
            some = s["type"] != 0
            reasons[rows, R_["bsdf"]] |= s["und"]
            wide = some & ((s["wi_e"] > R.REL_CAP).any(1) | ~np.isfinite(s["wi_e"]).all(1))
            reasons[rows, R_["bsdf"]] |= wide
            reasons[rows, R_["cos"]] |= some & (np.abs(s["wi"][:, 2]) < COS_FLOOR)
            okb = some & (s["f"].sum(1) > 0) & (s["pdf"] > 0) & ~wide                    # :413
            b_ok[rows], b_spec[rows] = okb, s["specular"]
            # the float32 wo of an implementation is within 6 eps of this one's: 16 eps more on the direction sampled from it
            wie = np.abs(s["wi_e"]).sum(1) + 16 * EPS
            b_wil[rows], b_wile[rows] = _as(np.where(okb[:, None], s["wi"], [0.0, 0.0, 1.0]), dt), np.where(okb[:, None], s["wi_e"] + 16 * EPS, 0.0)
            w = s["wi"][:, 0:1] * ss[rows] + s["wi"][:, 1:2] * ts[rows] + s["wi"][:, 2:3] * ns[rows]
            b_wi[rows], b_wie[rows] = np.where(okb[:, None], w, [0.0, 0.0, 1.0]), np.where(okb, wie, 0.0)
            side_b[rows] = np.where(s["wi"][:, 2] < 0, -1.0, 1.0)
        # the shadow test (:372-377): only for a non-black f
        shadow = a_ok & (a_f.sum(1) > 0)
        occluded = np.zeros(n, bool)
        if shadow.any():
            r = np.nonzero(shadow)[0]
            o = p[r] + (side_a[r] * self.p_err)[:, None] * ns[r]
            tmax = np.full(len(r), 1.0 - SHADOW_EPSILON)
            sp = (self.p_err + a_pb[r]) if spread else np.zeros(len(r))
            h, und, changed = self.trace(o, a_end[r] - o, tmax, ss[r], ts[r], sp, np.zeros(len(r)), spread)
            occluded[r] = h["occluded"]
            reasons[r, R_["shadow"]] |= und | changed
            kinds[r, 0], kinds[r, 1] = ~h["occluded"], h["occluded"]
        # the probe (:413-446)
        b_lp, b_lpe, b_le, picked = np.ones(n), z(), z(3), np.zeros(n, bool)
        if b_ok.any():
            r = np.nonzero(b_ok)[0]
            o = p[r] + (side_b[r] * self.p_err)[:, None] * ns[r]
            sp_o = np.full(len(r), self.p_err if spread else 0.0)
            h, und, changed = self.trace(o, b_wi[r], np.full(len(r), np.inf), ss[r], ts[r], sp_o, b_wie[r], spread)
            reasons[r, R_["probe"]] |= und
            reasons[r, R_["edge"]] |= changed & ~und
            le, cos_l, emitter = self.le_at(h, -b_wi[r], o)
            lj = self.light_of_prim[h["prim"]]
            pk = np.where(j[r] == self.env, h["kind"] == G.MISS, lj == j[r])             # :443-445: an escaped probe counts for the infinite light
            le = np.where(((j[r] == self.env) & pk)[:, None], self.lights[self.env][2][None, :] if self.env >= 0 else 0.0, le)
            cos_l = np.where((j[r] == self.env) & pk, 1.0, cos_l)
            kinds[r, 2], kinds[r, 3], kinds[r, 4] = pk, emitter & ~pk, ~emitter & ~pk
            reasons[r, R_["cos"]] |= pk & (cos_l < COS_FLOOR)
            picked[r] = pk
            b_le[r] = np.where(pk[:, None], le, 0.0)
        # the two terms, in the run's dtype with E's bounds
        with np.errstate(all="ignore"):
            lp, bp = _e(a_lp, a_lpe, dt), _e(a_bp, a_bpe, dt)
            wa = (lp * lp) / (lp * lp + bp * bp) if mis else _e(np.ones(n), 0.0, dt)
            scale_a = _e(a_cos, a_cose, dt) * (wa / lp)
            use_a = shadow & ~occluded
            A = [_masked(_e(a_f[:, c], a_fe[:, c], dt) * scale_a * _e(a_li[:, c], 0.0, dt), use_a) for c in range(3)]
        # The BSDF half is a function of the sampled direction alone: f(wi) |cos| Le w(pdf(wi), light_pdf(wi)) / pdf(wi).  f and pdf at a
        # sampled direction move together, so the term is bounded as a whole: its rounding bound at the truth's direction taken as exact,
        # plus its first-order variation over the direction's own bound (three one-sided differences, summed and doubled).
        use_b = b_ok & picked
        Bv, Be = np.zeros((n, 3), dt), np.zeros((n, 3))
        for t_, j_ in {(int(a), int(b)) for a, b in zip(tri[use_b], j[use_b])}:
            rows = np.nonzero(use_b & (tri == t_) & (j == j_))[0]
            b = self.bsdf(int(self.tri_material[t_]), dt)
            wo = [_e(wo_l[rows, c], 6 * EPS, dt) for c in range(3)]
            area = 2.0 * PI32 * PI32 if j_ == self.env else self.light_area(j_)
            origin = p[rows] + (side_b[rows] * self.p_err)[:, None] * ns[rows]

            def term(wi_l):
                with np.errstate(all="ignore"):
                    v = b.eval(wo, [_e(wi_l[:, c], 0.0, dt) for c in range(3)], R.NOSPEC)
                    w = wi_l[:, 0:1] * ss[rows] + wi_l[:, 1:2] * ts[rows] + wi_l[:, 2:3] * ns[rows]
                    dist, cos_l, _, scale_p = self.light_meet(j_, origin, w)
                    lpv = dist * dist / (cos_l * area)                                  # shape.rs:45-46, at the point the probe meets
                    lp_rel = G.gamma(24) + G.gamma(8) / cos_l + 3 * self.p_err / scale_p / cos_l
                    lp, bp = _e(lpv, lpv * lp_rel, dt), _e(v.pdf, v.pdf_e, dt)
                    wgt = (bp * bp) / (bp * bp + lp * lp) if mis else _e(np.ones(len(rows)), 0.0, dt)      # a specular lobe (:414-421) is not in these flags
                    scale = _e(np.abs(wi_l[:, 2]), 0.0, dt) * (wgt / bp)
                    out = [_e(v.f[:, c], v.f_e[:, c], dt) * scale * _e(b_le[rows, c], 0.0, dt) for c in range(3)]
                return np.stack([x.v for x in out], 1), np.stack([x.e for x in out], 1), v.left_out() | (v.pdf <= 0)
            v0, e0, lo = term(b_wil[rows])
            var = np.zeros_like(e0)
            for c in range(3):
                step = np.zeros((len(rows), 3))
                step[:, c] = b_wile[rows, c]
                v1, _, lo1 = term(b_wil[rows] + step)
                var += np.abs(v1.astype(np.float64) - v0.astype(np.float64))
                lo |= lo1
            reasons[rows, R_["bsdf"]] |= lo
            Bv[rows], Be[rows] = v0, e0 + 2.0 * var
        with np.errstate(all="ignore"):
            B = [E(np.where(use_b, Bv[:, c], 0), np.where(use_b, Be[:, c], 0.0)) for c in range(3)]
        return dict(A=A, B=B, reasons=reasons, kinds=kinds)

    # ------------------------------------------------------------------------------------------------------------ one camera sample
    def radiance(self, o, d, u, integrator="path", strategy="spatial", dtype=np.float64, u_arrays=None):
        """The radiance of n camera samples.  o, d: the camera rays (float32); u (n, 7): the sampler's dimensions 5 .. 11 of each sample.
        integrator: "path", "one" (`directlighting` "one") or "all" (`directlighting` "all"), each at maxdepth 1.  "all" reads u_arrays
        (n, nsamples, 2) and not u: element k of EVERY light's u_light and u_scattering array, which start_pixel fills from one pair of
        dimensions (quirk Q23: sobol.rs:60-75) at sample number s nsamples + k (base_sampler.rs:59-70); the vertex's direct light is the
        sum over the lights j, in list order, of (sum over k of estimate_direct) / nsamples (sample_lights.rs:24-78).  Returns dict: value (n, 3), bound (n, 3) absolute,
        reason (n,) index into REASONS or -1 where decided, kinds (n, len(KINDS)), vertex (n,) = the sample has a first vertex."""
        assert integrator in ("path", "one", "all")
        dt = np.dtype(dtype).type
        sc = self.sc
        o = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3)
        d = np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
        u = np.asarray(u, np.float32).reshape(len(o), 7)
        n = len(o)
        R_ = {k: i for i, k in enumerate(REASONS)}
        reasons = np.zeros((n, len(REASONS)), bool)
        kinds = np.zeros((n, len(KINDS)), bool)
        total = [E(np.zeros(n, dt)) for _ in range(3)]
        cam = self.closest_hits(sc, o, d, np.full(n, np.inf))
        reasons[:, R_["camera"]] = cam["rule"] != 0
        hit = cam["kind"] == G.TRIANGLE
        assert (hit | (cam["kind"] == G.MISS)).all(), "no camera ray may meet a sphere: a vertex is on a triangle"
        r = np.nonzero(hit)[0]
        tri = np.array([sc.prim_list[int(q)][1] for q in cam["prim"][r]], np.int64)
        wo = -_unit(d[r])
        p = o[r] + cam["t"][r, None] * d[r]
        for t_ in np.unique(tri):                                                       # onto the triangle's plane: the residue of o + t d
            nn, _ = self.tri_normal_area(int(t_))
            m = tri == t_
            for _ in range(2):
                p[m] -= ((p[m] - sc.P[sc.idx[t_, 0]]) @ nn)[:, None] * nn
        p = _as(p, dt)
        le, cos_e, emitter = self.le_at({"prim": cam["prim"][r]}, wo)                    # path.rs:87-91, directlighting.rs:85
        reasons[r, R_["cos"]] |= emitter & (cos_e < COS_FLOOR)
        for c in range(3):
            total[c].v[r] += le[:, c].astype(dt)
        if self.env >= 0:                          # an escaped camera ray: the infinite light's le (path.rs:92-94, directlighting.rs:115-124), a
            miss = np.nonzero(cam["kind"] == G.MISS)[0]                                # filtered lookup of a constant map: a dozen roundings
            for c in range(3):
                total[c].v[miss] += dt(self.lights[self.env][2][c])
                total[c].e[miss] += 16 * EPS * self.lights[self.env][2][c]
        mats = self.tri_material[tri]
        nospec = np.array([any(l.matches(R.NOSPEC) for l in self.bsdf(int(m), dt).lobes) for m in mats], bool)
        lit = np.nonzero(nospec)[0]
        if len(lit) and integrator == "all":                                            # sample_lights.rs:24-78
            ua = np.asarray(u_arrays, np.float32).reshape(n, -1, 2)[r[lit]]
            for j_ in range(len(self.lights)):
                ld = [E(np.zeros(len(lit), dt)) for _ in range(3)]
                for k in range(ua.shape[1]):
                    est = self.estimate(tri[lit], p[lit], wo[lit], np.full(len(lit), j_), ua[:, k], ua[:, k], dtype)
                    reasons[r[lit]] |= est["reasons"]
                    kinds[r[lit]] |= est["kinds"]
                    ld = [ld[c] + (est["A"][c] + est["B"][c]) for c in range(3)]
                for c in range(3):
                    term = ld[c] / float(ua.shape[1])
                    total[c].v[r[lit]] += term.v
                    total[c].e[r[lit]] += term.e + EPS * np.abs(term.v.astype(np.float64))
        elif len(lit):                                                                  # path.rs:119-137
            strat = "one" if integrator == "one" else strategy
            pdf, rel, near = self.pick_pdfs(p[lit], strat)
            jj, und = self.pick(pdf, rel, u[r[lit], 0])
            if dt is np.float32:                                                        # the decisions are the truth's, the numbers the run's
                pdf = self.pick_pdfs(p[lit], strat, dt)[0]
            reasons[r[lit], R_["pick"]] |= near | und
            est = self.estimate(tri[lit], p[lit], wo[lit], jj, u[r[lit], 1:3], u[r[lit], 3:5], dtype)
            reasons[r[lit]] |= est["reasons"]
            kinds[r[lit]] = est["kinds"]
            pp = _e(pdf[np.arange(len(lit)), jj], (pdf * rel)[np.arange(len(lit)), jj], dt)
            for c in range(3):
                ld = (est["A"][c] + est["B"][c]) / pp
                total[c].v[r[lit]] += ld.v
                total[c].e[r[lit]] += ld.e + EPS * np.abs(ld.v.astype(np.float64))
        if integrator == "path":                                                        # path.rs:141-167, then :86-91 at bounces == 1
            ub = np.where(nospec[:, None], u[r, 5:7], u[r, 0:2])
            ss, ts, ns = (np.stack([self.frame(int(t_))[k] for t_ in tri]) if len(tri) else np.zeros((0, 3)) for k in range(3))
            wo_l = np.stack([(wo * ax).sum(1) for ax in (ss, ts, ns)], 1)
            for m_ in np.unique(mats):
                rows = np.nonzero(mats == m_)[0]
                b = self.bsdf(int(m_), dt)
                if not any(l.type & R.SPECULAR for l in b.lobes):
                    continue
                with np.errstate(all="ignore"):
                    s = b.sample(wo_l[rows].astype(np.float32), ub[rows], R.ALL)
                reasons[r[rows], R_["bsdf"]] |= s["und"]
                sp = s["specular"] & (s["type"] != 0) & (s["f"].sum(1) > 0) & (s["pdf"] > 0)
                k = rows[sp]
                if not len(k):
                    continue
                wi_l, wie = _as(s["wi"][sp], dt), np.abs(s["wi_e"][sp]).sum(1) + 16 * EPS
                reasons[r[k], R_["cos"]] |= np.abs(wi_l[:, 2]) < COS_FLOOR
                w = wi_l[:, 0:1] * ss[k] + wi_l[:, 1:2] * ts[k] + wi_l[:, 2:3] * ns[k]
                side = np.where(wi_l[:, 2] < 0, -1.0, 1.0)
                oo = p[k] + (side * self.p_err)[:, None] * ns[k]
                h, und, changed = self.trace(oo, w, np.full(len(k), np.inf), ss[k], ts[k], np.full(len(k), self.p_err), wie)
                reasons[r[k], R_["probe"]] |= und
                reasons[r[k], R_["edge"]] |= changed & ~und
                le2, cos2, em2 = self.le_at(h, -w, oo)
                if self.env >= 0:
                    le2 = np.where((h["kind"] == G.MISS)[:, None], self.lights[self.env][2][None, :], le2)
                reasons[r[k], R_["cos"]] |= em2 & (cos2 < COS_FLOOR)
                with np.errstate(all="ignore"):
                    scale = _e(np.abs(wi_l[:, 2]), s["wi_e"][sp][:, 2] + 16 * EPS, dt) / _e(s["pdf"][sp], s["pdf_e"][sp], dt)
                    for c in range(3):
                        term = _e(s["f"][sp][:, c], s["f_e"][sp][:, c], dt) * scale * _e(le2[:, c], 0.0, dt)
                        total[c].v[r[k]] += term.v
                        total[c].e[r[k]] += term.e + EPS * np.abs(term.v.astype(np.float64))
        value = np.stack([t.v.astype(np.float64) for t in total], 1)
        bound = np.stack([t.e for t in total], 1)
        with np.errstate(all="ignore"):
            reasons[:, R_["wide"]] |= ((bound > REL_CAP * np.abs(value)) & (bound > 0)).any(1) | ~np.isfinite(bound).all(1) | ~np.isfinite(value).all(1)
        reason = np.where(reasons.any(1), reasons.argmax(1), -1)
        vertex = np.zeros(n, bool)
        vertex[r] = True
        return dict(value=value, bound=bound, reason=reason, kinds=kinds, vertex=vertex)


def emitter_quadrature(setup, p, n_surface, kd, k=256):
    """The float64 integral of Kd / pi L cos cos' / r^2 over every emitter as seen from points p with surface normal n_surface, no
    occluder: the midpoint rule on k^2 sub-triangles of each emissive triangle."""
    out = np.zeros((len(p), 3))
    i, jn = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    lower = (i + jn) < k
    b0 = np.concatenate([(i[lower] + 1 / 3) / k, (i[(i + jn) < k - 1] + 2 / 3) / k])
    b1 = np.concatenate([(jn[lower] + 1 / 3) / k, (jn[(i + jn) < k - 1] + 2 / 3) / k])
    for _, tri, L, two in setup.lights:
        p0, p1, p2 = (setup.sc.P[setup.sc.idx[tri, c]] for c in range(3))
        nn, area = setup.tri_normal_area(tri)
        q = b0[:, None] * p0 + b1[:, None] * p1 + (1 - b0 - b1)[:, None] * p2
        for a in range(len(p)):
            w = q - p[a]
            r2 = (w * w).sum(1)
            wi = w / np.sqrt(r2)[:, None]
            cs, cl = wi @ n_surface, -(wi @ nn)
            g = np.where((cs > 0) & ((cl > 0) | two), cs * np.abs(cl) / r2, 0.0)
            out[a] += np.asarray(kd) / np.pi * L * g.mean() * area
    return out
