"""The cases of the direct-lighting truth (tests/direct_ref.py) and what is asserted on them -- shared by test_direct_truth_oracle.py (the
float32 run of the restatement and the oracle, no GPU) and test_gpu_direct_truth.py (the device, no oracle).

The scene, the smallest with every kind of first vertex: a 4 x 4 floor at z = 0, split along x = 0 where a row has two materials; a
one-sided emissive quad of 3 x 3 facing down at z = 2 (two triangle lights: the pick and the "other triangle" case are live with one
emitter); a dimmer, smaller, tilted emissive triangle to one side (the power and spatial distributions are not uniform); a matte blocker
under part of the quad; a camera low enough that no camera ray meets an emitter from behind.  The `le` camera looks up at the quad's lit
face, the `below` camera is under the floor (translucent halves).  In the sphere rows the side emitter is a sphere light out of the
cameras' sight; in the disk row the big emitter is a disk of the quad's extent; the env row adds a constant infinite light after the
emitters; the mix and disney rows change the floor's material.  The route "halton" renders under the Halton sampler.  The emitters carry a black Matte: a vertex on them has a BSDF and adds nothing but Le.  16 x 16 pixels, 4 samples each, box
filter.  Integrators: "path", "one" (`directlighting` "one"), "all1" / "all2" (`directlighting` "all", every light with that nsamples).

The coordinates are fixed by the kind counts (MIN_KIND of each of direct_ref.KINDS among a row's decided samples, from the float64 truth
alone).  Materials are settings of bsdf_cases whose left-out share in profiles/bsdf_truth.txt is at most 1.4 %."""
import os

import numpy as np

import bsdf_cases as C
import direct_ref as D
import disney_cases
import halton_ref
import mix_cases
from helpers import scenes

RES, SPP = 16, 4
MAX_LEFT_OUT = C.MAX_LEFT_OUT            # 3 %: the BSDF truth's own cap, on the union of all reasons
MEDIAN_FACTOR = C.MEDIAN_FACTOR          # an implementation's median err / bound against the float32 run's
MIN_KIND = 30
EXTENT = 2.0                             # no coordinate of the scene is past it: the scale of a rebuilt hit point's roundings
FLOOR = (-2.0, 2.0, -2.0, 2.0)
EMITTER = (-1.5, 1.5, -1.2, 1.8, 2.0)                                   # x0 x1 y0 y1 z, faces down
SIDE = [(-2.0, -1.2, 1.0), (-2.0, 0.6, 1.0), (-1.3, -0.3, 1.5)]         # its normal points down and towards the floor's middle
SIDE_SPHERE = (-1.75, 0.25, 1.25, 0.25)                                 # centre and radius of the sphere rows' side emitter
BLOCKER = (-0.2, 1.4, -1.0, 0.6, 0.45)
L_QUAD, L_SIDE, L_ENV = (6.0, 5.0, 4.0), (2.0, 3.0, 2.5), (0.5, 0.6, 0.7)
# eye, look-at, fov.  Every eye is below the emitters' planes
CAMERAS = {"low": ((0.0, -4.0, 1.9), (0.0, -0.5, 0.0), 32.0), "le": ((0.0, -3.8, 0.8), (0.0, 0.0, 1.0), 50.0), "steep": ((0.0, -2.5, 1.95), (0.0, -0.9, 0.0), 50.0),
           "below": ((0.0, -4.0, -1.9), (0.0, -0.5, 0.0), 32.0)}
BLACK = dict(type="matte", Kd=(0.0, 0.0, 0.0))
GREY = dict(type="matte", Kd=(0.5, 0.4, 0.3))
M = {"matte": C.CASES["matte"]["lambert"], "plastic": C.CASES["plastic"]["remap"], "metal": C.CASES["metal"]["aniso_uv"],
     "substrate": C.CASES["substrate"]["aniso"], "uber": C.CASES["uber"]["opaque"], "translucent": C.CASES["translucent"]["four"],
     "translucent_t": C.CASES["translucent"]["lambert_t"],
     "mix": dict(type="mix", m1=C.CASES["plastic"]["remap"], m2=C.CASES["matte"]["lambert"], amount=(0.3, 0.3, 0.3)),
     "disney": disney_cases.SETTINGS["default"], "mirror": C.CASES["mirror"]["mirror"], "glass": C.CASES["glass"]["smooth"]}
# row -> (material of the floor's x < 0 half, of its x > 0 half (None: one mesh), camera)
ROWS = {
    "matte": ("matte", None, "low"),
    "matte_le": ("matte", None, "le"),
    "halves": ("matte", "plastic", "low"),
    "lobes": ("metal", "substrate", "low"),
    "uber_kr": ("uber", "plastic", "low"),            # a specular lobe beside the others: left out of the estimate, met by the bounce
    "specular": ("mirror", "glass", "steep"),
    "sphere": ("matte", None, "low"),                  # the side emitter is a sphere light (cone sampling), out of the camera's sight
    "sphere_halves": ("matte", "plastic", "low"),
    "env": ("matte", "plastic", "low"),                # a constant infinite light beside the emitters: k_shade_env
    "disk": ("matte", "plastic", "low"),                 # the big emitter is a disk of the quad's extent: the quadric build
    "mix": ("mix", None, "low"),                       # mix(plastic, matte, 0.3): k_shade_mix
    "disney": ("disney", "matte", "low"),              # the disney build
    "below": ("translucent_t", "translucent", "below"),         # the camera under the floor: the transmission lobes carry the emitters' light down
}
NOT_IN_THE_ORACLE = ("below", "mix", "disney", "disk")          # Materials "translucent", "mix", "disney" and Shape "disk": the oracle does not know them
SPECULAR_ROWS = ("specular",)
# route -> how the scene is built (scene()'s switches)
ROUTES = {"plain": {}, "halton": dict(sampler="halton"), "textured": dict(textured=True), "instance": dict(instance=True), "instance_textured": dict(instance=True, textured=True)}
# (row, integrator, light sample strategy, route)
CASES = [(r, "path", "uniform", "plain") for r in ROWS] + [(r, "path", s, "plain") for r in ("matte", "halves") for s in ("power", "spatial")] + \
        [(r, i, "uniform", "plain") for r in ("matte", "halves", "sphere") for i in ("one", "all1", "all2")] + \
        [("sphere", "path", s, "plain") for s in ("power", "spatial")] + [("env", "path", "power", "plain"), ("env", "all1", "uniform", "plain")] + [("halves", "path", "uniform", r) for r in ROUTES if r not in ("plain", "halton")] + \
        [(r, "path", "uniform", "halton") for r in ("matte", "lobes")]
IDS = ["%s-%s-%s-%s" % c for c in CASES]


def scenes_of(case):
    """(the scene an implementation renders, the scene the truth is computed on, the extent of the coordinates a hit point is rebuilt from).
    An instanced floor is met in the instance's space, INSTANCE_OFFSET away, and brought back: coordinates up to 2.5, two transforms."""
    row, integ, strategy, route = case
    kw = ROUTES[route]
    sd = scene(row, integ, strategy, **kw)
    if not kw.get("instance"):
        return sd, sd, EXTENT
    return sd, scene(row, integ, strategy, textured=kw.get("textured", False)), 2.0 * (EXTENT + max(abs(c) for c in INSTANCE_OFFSET))


INSTANCE_OFFSET = (0.5, -0.25, 0.25)      # exact in float32, as is every floor coordinate less it: the instanced floor IS the floor


def rect(sb, x0, x1, y0, y1, z, down=False, uv=False, offset=(0.0, 0.0, 0.0)):
    pts = [x0, y0, z, x1, y0, z, x1, y1, z, x0, y1, z]
    pts = [c - offset[i % 3] for i, c in enumerate(pts)]
    sb.shape_trianglemesh(pts, [0, 2, 1, 0, 3, 2] if down else [0, 1, 2, 0, 2, 3], uv=[0, 0, 1, 0, 1, 1, 0, 1] if uv else None)


def scene(row, integrator="path", strategy="uniform", blocker=True, textured=False, instance=False, proxy=False, sampler="sobol"):
    """The scene description, with .direct_params: material index -> the parameters the truth starts from.  textured: "roughness" comes
    from an image map of one value and the floor carries uvs.  instance: the floor is built INSTANCE_OFFSET away inside an object and
    brought back by the instance's translation -- the same points, so the truth of such a scene is the plain scene's.  proxy: every
    translucent, mix or disney material is a Matte -- a scene the oracle can load, for the camera rays and sampler values of a row it cannot render."""
    left, right, cam = ROWS[row]
    sb = scenes.SceneBuilder()
    sb.look_at(CAMERAS[cam][0], CAMERAS[cam][1], (0, 0, 1))
    sb.camera_perspective(fov=CAMERAS[cam][2])
    sb.film(xresolution=RES, yresolution=RES)
    sb.pixel_filter_box()
    (sb.sampler_halton if sampler == "halton" else sb.sampler_sobol)(pixelsamples=SPP)
    nsamples = int(integrator[3:]) if integrator.startswith("all") else 1          # "all2": `directlighting` "all", every light with nsamples 2
    if integrator == "path":
        sb.integrator_path(maxdepth=1, lightsamplestrategy=strategy)
    else:
        sb.integrator_directlighting(maxdepth=1, strategy=integrator[:3])
    params = {}

    def material(p):
        if proxy and p["type"] in ("translucent", "mix", "disney"):
            p = GREY
        if p["type"] == "mix":
            params[mix_cases.apply(sb, p)] = p
            return
        if p["type"] == "disney":
            params[disney_cases.apply(sb, p)] = p
            return
        if textured and "roughness" in p:          # "roughness" from an image map of one value: the lobes are built on the device at the hit
            img = np.full((4, 4, 1), p["roughness"], np.float32)
            params[C.apply(sb, dict(p, roughness=sb.texture_imagemap(sb.image_pyramid(img))))] = p
        else:
            params[C.apply(sb, p)] = p
    off = INSTANCE_OFFSET if instance else (0.0, 0.0, 0.0)
    if instance:
        sb.object_begin("floor")
    material(M[left])
    rect(sb, FLOOR[0], FLOOR[1] if right is None else 0.0, FLOOR[2], FLOOR[3], 0.0, uv=textured, offset=off)
    if right is not None:
        material(M[right])
        rect(sb, 0.0, FLOOR[1], FLOOR[2], FLOOR[3], 0.0, uv=textured, offset=off)
    if instance:
        sb.object_end()
        sb.object_instance("floor", to_world=scenes.transform_translate(*off))
    if blocker:
        material(GREY)
        rect(sb, *BLOCKER)
    material(BLACK)
    sb.area_light_source_diffuse(L=L_QUAD, twosided=False, nsamples=nsamples)
    if row == "disk" and not proxy:            # (the proxy keeps the quad: the same extent, the same world bound)
        t = scenes.transform_translate(0.5 * (EMITTER[0] + EMITTER[1]), 0.5 * (EMITTER[2] + EMITTER[3]), EMITTER[4])
        sb.reverse_orientation = True          # the disk's normal is +z: ReverseOrientation turns its lit face down
        sb.shape_disk(height=0.0, radius=0.5 * (EMITTER[1] - EMITTER[0]), object_to_world=t[0], world_to_object=t[1])
        sb.reverse_orientation = False
    else:
        rect(sb, *EMITTER, down=True)
    sb.area_light_source_diffuse(L=L_SIDE, twosided=False, nsamples=nsamples)
    if row.startswith("sphere"):
        t = scenes.transform_translate(*SIDE_SPHERE[:3])
        sb.shape_sphere(radius=SIDE_SPHERE[3], object_to_world=t[0], world_to_object=t[1])
    else:
        sb.shape_trianglemesh([c for v in SIDE for c in v], [0, 1, 2])
    sb.no_area_light()
    if row == "env":
        sb.light_infinite(L=L_ENV, nsamples=nsamples)
    sd = sb.build()
    sd.direct_params = params
    return sd


class Inputs:
    """What the truth takes from an implementation as exact float32 numbers: the camera rays and the sampler's dimensions 5 .. 11 of every
    camera sample of the film, pixel by pixel, sample by sample (the order of radiance_samples)."""

    def __init__(self, impl, info, nsamples=0, halton=False):
        """nsamples > 0: also u_arrays (n, nsamples, 2), the elements of `directlighting` "all"'s sample arrays: dimensions 5 and 6 at
        sample number s nsamples + k of the pixel."""
        b = tuple(info.sample_bounds)
        spp = int(info.spp)
        ys, xs = np.mgrid[b[1]:b[3], b[0]:b[2]]
        pix = np.repeat(np.stack([xs.reshape(-1), ys.reshape(-1)], 1), spp, axis=0).astype(np.int32)
        si = np.tile(np.arange(spp, dtype=np.uint32), xs.size)
        self.bounds = b
        self.o, self.d, _ = impl.generate_camera_rays(pix, si)
        dims = np.repeat(np.arange(5, 12, dtype=np.uint32), len(si))
        self.u = impl.sobol_samples(np.tile(pix, (7, 1)), np.tile(si, 7), dims).reshape(7, len(si)).T.copy()
        self.world_bound = [float(x) for x in info.world_bound]
        if halton:
            # Under Halton the hook's numbers are held to the exact rational value of the sample (tests/halton_ref.py) before the truth takes
            # them: the float32 radical inverse of up to 12 digits is within 4e-7 of it (the margin tests/test_halton.py holds the oracle to)
            perms, P = halton_ref.default_permutations(12), halton_ref.primes(12)
            for i in range(len(si)):
                idx = halton_ref.pixel_sample_index(b, int(pix[i, 0]), int(pix[i, 1]), int(si[i]))
                want = [float(halton_ref.scrambled_radical_inverse(P[dim], perms[dim], idx)) for dim in range(5, 12)]
                assert np.abs(self.u[i] - want).max() <= 4e-7, (i, self.u[i], want)
        self.u_arrays = None
        if nsamples:
            sk = (si[:, None] * np.uint32(nsamples) + np.arange(nsamples, dtype=np.uint32)[None, :]).reshape(-1)
            pk = np.repeat(pix, nsamples, axis=0)
            ua = [impl.sobol_samples(pk, sk, np.full(len(sk), dim, np.uint32)) for dim in (5, 6)]
            self.u_arrays = np.stack(ua, 1).reshape(len(si), nsamples, 2)


_truths = {}


def truth_of(sd, inp, integrator, strategy, extent=EXTENT):
    """(setup, float64 truth) of a scene and its inputs, computed once per process and left unchanged."""
    geometry = tuple(bytes(np.ascontiguousarray(sd.buffers[k])) for k in ("P", "indices", "tri_mesh", "UV") if sd.buffers.get(k) is not None)
    flags = tuple(int(sd.buffers["meshes"][i].flags) for i in range(sd.desc.n_meshes))
    flags += tuple((il.light_index, il.image) for il in sd.infinite_lights)
    flags += tuple(bytes(sd.buffers["spheres"][i]) for i in range(sd.desc.n_spheres)) + tuple(bytes(sd.buffers["area_lights"][i]) for i in range(sd.desc.n_area_lights))
    ua = b"" if inp.u_arrays is None else inp.u_arrays.tobytes()
    key = (geometry, flags, tuple(sorted((k, str(v)) for k, v in sd.direct_params.items())), inp.o.tobytes(), inp.d.tobytes(), inp.u.tobytes(), ua,
           tuple(inp.world_bound), integrator, strategy, extent)
    if key not in _truths:
        setup = D.Setup(sd, sd.direct_params, inp.world_bound, extent)
        tr = setup.radiance(inp.o, inp.d, inp.u, integrator[:3] if integrator.startswith("all") else integrator, strategy, u_arrays=inp.u_arrays)
        for a in tr.values():
            a.setflags(write=False)
        _truths[key] = (setup, tr)
    return _truths[key]


def nsamples_of(integrator):
    return int(integrator[3:]) if integrator.startswith("all") else 0


def report(stat):
    """One line per implementation and case.  DIRECT_TRUTH_WRITE names the file the run appends them to (profiles/direct_truth.txt is
    the CPU file's and the GPU file's lines of one run each); DIRECT_TRUTH_WRITE=1 prints them."""
    where = os.environ.get("DIRECT_TRUTH_WRITE")
    if where == "1":
        print("\n" + stat.line())
    elif where:
        with open(where, "a") as f:
            f.write(stat.line() + "\n")


class Stat:
    """One implementation on one case: decided, left out per reason, worst and median err / bound, the kind counts."""

    def __init__(self, label, tr, got):
        got = np.asarray(got, np.float64).reshape(-1, 3)
        dec = tr["reason"] < 0
        self.label, self.n = label, len(dec)
        self.by_reason = np.bincount(tr["reason"][~dec], minlength=len(D.REASONS))
        self.left = float((~dec).mean())
        want, bound = tr["value"][dec], tr["bound"][dec]
        g = got[dec]
        self.zero_bad = int(((bound == 0) & (g != want)).sum())                  # a decided value (0, or Le alone) is met exactly
        with np.errstate(all="ignore"):
            ratio = np.where(bound > 0, np.abs(g - want) / bound, 0.0)
        self.ratio = ratio[bound > 0]
        self.worst = float(self.ratio.max()) if len(self.ratio) else 0.0
        self.median = float(np.median(self.ratio)) if len(self.ratio) else 0.0
        self.kinds = tr["kinds"][dec].sum(0)
        self.lit = int((dec & (tr["value"].sum(1) > 0)).sum())
        self.distinct = len(np.unique(np.round(tr["value"][dec & (tr["value"].sum(1) > 0)], 6), axis=0))
        self.decided = int(dec.sum())

    def line(self):
        return "%-4s %-28s decided %4d of %d  left out %.4f (%s)  err/bound worst %.3f median %.4f  lit %d  kinds %s" % (
            self.label[0], self.label[1], self.decided, self.n, self.left,
            " ".join("%s %d" % (k, c) for k, c in zip(D.REASONS, self.by_reason)), self.worst, self.median, self.lit, "/".join(str(int(k)) for k in self.kinds))


def hold(stat, row, calibration=None):
    """The assertions of a row, the same for every implementation.  `lit` and `distinct` count the TRUTH's decided values, not the
    implementation's: they say that the row is worth comparing, the bound says that the implementation agrees."""
    assert stat.zero_bad == 0, (stat.label, "a decided value is not met exactly", stat.zero_bad)
    assert stat.worst <= 1.0, (stat.label, "err / bound", stat.worst, int((stat.ratio > 1.0).sum()))
    assert stat.left <= MAX_LEFT_OUT, (stat.label, "left out", stat.left, dict(zip(D.REASONS, stat.by_reason)))
    # A specular floor has no estimate at its vertices: only the blocker's and the emitters' vertices have kinds.  Its lit samples are the
    # mirror's and the glass's reflections of the emitters (and the blocker), which vary with the Fresnel term and the Kr colour.
    if row not in SPECULAR_ROWS:
        assert (stat.kinds >= MIN_KIND).all(), (stat.label, dict(zip(D.KINDS, stat.kinds)))
    assert stat.lit >= 300, (stat.label, "lit", stat.lit)
    assert stat.distinct > 50, (stat.label, "distinct values", stat.distinct)
    if calibration is not None:
        assert stat.median <= MEDIAN_FACTOR * calibration.median, (stat.label, "median err / bound", stat.median, "float32 run", calibration.median)
