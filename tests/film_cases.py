"""The case list that holds the film to tests/film_ref.py, shared by the oracle leg (test_film_truth_oracle.py) and the device leg
(test_gpu_film_truth.py): the room of feature_scenes.scene_camera_film (area light, matte sphere, thin lens: radiance varies from
sample to sample and the samples that see the light are bright) on a 40 x 32 film, 4 spp Sobol' or 3 spp Halton."""
import numpy as np

import feature_scenes as fs
import film_ref

FULL = (0.0, 1.0, 0.0, 1.0)
CROP = (0.2, 0.85, 0.1, 0.9)              # 40 x 32: pixels [8, 34) x [3, 29)
ONE_PIXEL = (0.5, 0.51, 0.5, 0.52)        # 40 x 32: 20 .. ceil(20.4), 16 .. ceil(16.64): the single pixel (20, 16)
FAR_CORNER = (0.8, 1.0, 0.75, 1.0)        # 40 x 32: [32, 40) x [24, 32), touching the right and the bottom border

# name: (filter, (xwidth, ywidth), filter parameters, crop window, maxsampleluminance, scale, sampler, integrator)
CASES = {
    # filters
    "box_0.5":        ("box", (0.5, 0.5), {}, FULL, np.inf, 1.0, "sobol", "path"),            # every sample takes the `own` path
    "box_0.3":        ("box", (0.3, 0.3), {}, CROP, 3.0, 2.0, "halton", "path"),              # footprints without a pixel centre are dropped
    "box_1.0":        ("box", (1.0, 1.0), {}, CROP, 3.0, 1.0, "halton", "path"),               # several equal weights through `spill`
    "triangle":       ("triangle", (1.5, 2.0), {}, CROP, 3.0, 2.0, "halton", "path"),
    "gaussian":       ("gaussian", (2.0, 2.0), {"alpha": 2.0}, CROP, 3.0, 2.0, "sobol", "path"),
    "gaussian_aniso": ("gaussian", (1.2, 2.5), {"alpha": 0.5}, FULL, np.inf, 1.0, "sobol", "path"),
    "mitchell":       ("mitchell", (2.0, 1.5), {"B": 1.0 / 3.0, "C": 1.0 / 3.0}, CROP, 3.0, 2.0, "sobol", "path"),
    "mitchell_0_0.5": ("mitchell", (2.0, 1.5), {"B": 0.0, "C": 0.5}, FULL, np.inf, 1.0, "halton", "path"),
    "sinc":           ("sinc", (3.0, 2.5), {"tau": 2.0}, CROP, 3.0, 2.0, "sobol", "path"),
    "sinc_4_4":       ("sinc", (4.0, 4.0), {"tau": 3.0}, FULL, np.inf, 1.0, "halton", "path"),
    # windows
    "one_pixel":      ("gaussian", (2.5, 2.5), {"alpha": 2.0}, ONE_PIXEL, np.inf, 1.0, "sobol", "path"),      # nearly every sample is "outside"
    "far_corner":     ("mitchell", (2.0, 1.5), {"B": 1.0 / 3.0, "C": 1.0 / 3.0}, FAR_CORNER, np.inf, 2.0, "halton", "path"),
    # the other integrators: their samples reach the film by other routes
    "directlighting": ("gaussian", (2.0, 2.0), {"alpha": 2.0}, CROP, 3.0, 2.0, "sobol", "directlighting"),
    "whitted":        ("gaussian", (2.0, 2.0), {"alpha": 2.0}, CROP, np.inf, 2.0, "halton", "whitted"),
    "ao":             ("gaussian", (2.0, 2.0), {"alpha": 2.0}, CROP, np.inf, 1.0, "sobol", "ao"),
    "aov":            ("gaussian", (2.0, 2.0), {"alpha": 2.0}, CROP, np.inf, 1.0, "halton", "aov"),        # the device only: the oracle has no "aov"
}
# the window cases under a wide filter: at least a tenth of the contributing samples belong to pixels outside the crop.  (Under the negative
# lobes of "mitchell" and "sinc" on the same window many outside samples sum to <= 0 and are dropped, which is a path of its own.)
WIDE_CROPPED = ("triangle", "gaussian", "one_pixel", "far_corner", "directlighting", "whitted", "ao", "aov")
ORACLE_CASES = [k for k in CASES if k != "aov"]


def pixel_filter(b, kind, widths, params):
    getattr(b, "pixel_filter_" + kind)(widths[0], widths[1], **params)


def make_scene(name=None, spec=None, res=(40, 32), spp=None):
    kind, widths, params, window, clamp, scale, sampler, integrator = spec or CASES[name]
    b = fs.base(res=res[0], spp=4)
    b.camera_perspective(fov=40.0, lensradius=0.15, focaldistance=6.0)
    b.film(xresolution=res[0], yresolution=res[1], cropwindow=window, scale=scale, maxsampleluminance=clamp)
    pixel_filter(b, kind, widths, params)
    if sampler == "sobol":
        b.sampler_sobol(spp or 4)
    else:
        b.sampler_halton(spp or 3)
    if integrator == "directlighting":
        b.integrator_directlighting(maxdepth=3)
    elif integrator == "whitted":
        b.integrator_whitted(maxdepth=3)
    elif integrator == "ao":
        b.integrator_ao(nsamples=4)
    elif integrator == "aov":
        b.integrator_aov("n")
    fs.room(b)
    b.material_matte((0.6, 0.6, 0.6))
    P, N, UV, idx = fs.uv_sphere((0.0, -1.0, 0.0), 1.0, 6, 10)
    b.shape_trianglemesh(P, idx, N=N)
    return b.build()


def film_inputs(sd):
    """What the truth takes from the scene description, as data."""
    d = sd.desc
    return {"table": np.array(list(d.filter_table), np.float32), "radius": (d.filter_radius[0], d.filter_radius[1]),
            "crop_window": tuple(d.crop_window), "res": (d.xres, d.yres), "scale": d.film_scale, "clamp": d.max_sample_luminance}


def samples_of(renderer, info):
    """Every sample of the whole sample bounds from `renderer` (the oracle's scene or the device context): one tile to radiance_samples,
    the same pixels and sample indices to generate_camera_rays.  Returns (p_film (n, 2), radiance (n, 3), pixel (n, 2))."""
    sb = tuple(info.sample_bounds)
    rad = renderer.radiance_samples(sb)
    spp = rad.shape[1]
    ys, xs = np.mgrid[sb[1]:sb[3], sb[0]:sb[2]]
    pix = np.repeat(np.stack([xs.ravel(), ys.ravel()], axis=1), spp, axis=0).astype(np.int32)
    k = np.tile(np.arange(spp, dtype=np.uint32), (sb[2] - sb[0]) * (sb[3] - sb[1]))
    _, _, pf = renderer.generate_camera_rays(pix, k)
    return pf, rad.reshape(-1, 3), pix


def truth_of(sd, p_film, radiance, repeat=1):
    fi = film_inputs(sd)
    cropped, sample_bounds, _ = film_ref.film_bounds(fi["res"][0], fi["res"][1], fi["crop_window"], fi["radius"])
    t = film_ref.film_truth(p_film, radiance, fi["table"], fi["radius"], cropped, fi["clamp"], fi["scale"], repeat)
    t["cropped"], t["sample_bounds"] = cropped, sample_bounds
    return t


def outside_share(truth, pix):
    """The share of the contributing samples whose own pixel lies outside the crop."""
    x0, y0, x1, y1 = truth["cropped"]
    out = (pix[:, 0] < x0) | (pix[:, 0] >= x1) | (pix[:, 1] < y0) | (pix[:, 1] >= y1)
    c = truth["contributes"]
    return float((out & c).sum()) / max(1, int(c.sum()))
