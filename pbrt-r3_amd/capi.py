"""ctypes bindings for include/pbrtgpu.h (libpbrtgpu.so).

Every binding goes through the C ABI; there is no Python or CPU re-implementation
of any kernel here.  If the shared library is absent, load_library() raises.
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBRTGPU_LIB") or os.path.join(HERE, "csrc", "libpbrtgpu.so")   # override: tuning builds only
DATA_DIR = os.path.join(HERE, "data")

PT_MATERIAL_NONE, PT_MATERIAL_MATTE, PT_MATERIAL_PLASTIC, PT_MATERIAL_MIRROR = 0, 1, 2, 3
PT_MATERIAL_GLASS, PT_MATERIAL_METAL, PT_MATERIAL_UBER, PT_MATERIAL_SUBSTRATE = 4, 5, 6, 7
PT_MATERIAL_TRANSLUCENT = 8
PT_MATERIAL_MIX = 9
PT_MATERIAL_DISNEY = 10
PT_MATERIAL_FOURIER = 11
(PT_DISNEY_METALLIC, PT_DISNEY_SPECULARTINT, PT_DISNEY_ANISOTROPIC, PT_DISNEY_SHEEN, PT_DISNEY_SHEENTINT, PT_DISNEY_CLEARCOAT,
 PT_DISNEY_CLEARCOATGLOSS, PT_DISNEY_SPECTRANS, PT_DISNEY_FLATNESS, PT_DISNEY_DIFFTRANS) = range(10)
PT_MIX_MAX_LEAVES, PT_MIX_MAX_LOBES = 4, 16
PTH_FEATURE_MIX_MATERIAL, PTH_FEATURE_DELTA_LIGHTS, PTH_FEATURE_QUADRIC_SHAPES, PTH_FEATURE_DISNEY_MATERIAL, PTH_FEATURE_POINT_LIGHTS = 1, 2, 4, 8, 16
PTH_FEATURE_MOTION_BLUR = 32
PTH_FEATURE_FOURIER_MATERIAL = 64
PT_SHAPE_SPHERE, PT_SHAPE_CYLINDER, PT_SHAPE_DISK = 0, 1, 2
PT_ROUGHNESS_UNSET = -1.0
PT_MESH_TWO_SIDED, PT_MESH_REVERSE_ORIENTATION, PT_MESH_SWAPS_HANDEDNESS = 1, 2, 4
PT_MESH_HAS_N, PT_MESH_HAS_S, PT_MESH_HAS_UV = 8, 16, 32
PT_SPLIT_SAH, PT_SPLIT_HLBVH, PT_SPLIT_MIDDLE, PT_SPLIT_EQUAL_COUNTS = 0, 1, 2, 3
PT_LIGHTS_UNIFORM, PT_LIGHTS_POWER, PT_LIGHTS_SPATIAL = 0, 1, 2
PT_SAMPLER_SOBOL, PT_SAMPLER_HALTON = 0, 1

STATUS_NAMES = {0: "PT_OK", 1: "PT_ERR_INVALID_ARGUMENT", 2: "PT_ERR_NO_DEVICE", 3: "PT_ERR_DEVICE",
                4: "PT_ERR_UNSUPPORTED", 5: "PT_ERR_NO_SCENE", 6: "PT_ERR_OUT_OF_MEMORY"}


class PtError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), msg))
        self.status = status


class pt_material(C.Structure):
    _fields_ = [("type", C.c_int32), ("kd", C.c_float * 3), ("sigma", C.c_float), ("ks", C.c_float * 3), ("kr", C.c_float * 3),
                ("kt", C.c_float * 3), ("opacity", C.c_float * 3), ("eta", C.c_float), ("roughness", C.c_float),
                ("uroughness", C.c_float), ("vroughness", C.c_float), ("remap_roughness", C.c_int32),
                ("metal_eta", C.c_float * 3), ("metal_k", C.c_float * 3),
                ("tex_kd", C.c_uint32), ("tex_ks", C.c_uint32), ("tex_kr", C.c_uint32), ("tex_kt", C.c_uint32),
                ("tex_opacity", C.c_uint32), ("tex_sigma", C.c_uint32), ("tex_metal_eta", C.c_uint32), ("tex_metal_k", C.c_uint32),
                ("tex_bump", C.c_uint32), ("tex_roughness", C.c_uint32), ("tex_uroughness", C.c_uint32), ("tex_vroughness", C.c_uint32), ("tex_eta", C.c_uint32)]


class pt_texture(C.Structure):
    _fields_ = [("type", C.c_int32), ("tex", C.c_int32 * 3), ("value", (C.c_float * 3) * 4), ("mapping", C.c_int32),
                ("aa_none", C.c_int32), ("su", C.c_float), ("sv", C.c_float), ("du", C.c_float), ("dv", C.c_float),
                ("v1", C.c_float * 3), ("v2", C.c_float * 3), ("world_to_texture", C.c_float * 16),
                ("octaves", C.c_int32), ("omega", C.c_float), ("scale", C.c_float), ("variation", C.c_float),
                ("image", C.c_int32), ("trilinear", C.c_int32), ("max_anisotropy", C.c_float), ("swrap", C.c_int32), ("twrap", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class pt_image(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("n_levels", C.c_uint32),
                ("texels", C.POINTER(C.c_float))]


PT_WRAP_REPEAT, PT_WRAP_BLACK, PT_WRAP_CLAMP = range(3)


(PT_TEX_CONSTANT, PT_TEX_SCALE, PT_TEX_MIX, PT_TEX_CHECKERBOARD_2D, PT_TEX_CHECKERBOARD_3D, PT_TEX_UV, PT_TEX_BILERP, PT_TEX_DOTS, PT_TEX_FBM,
 PT_TEX_WRINKLED, PT_TEX_WINDY, PT_TEX_MARBLE, PT_TEX_IMAGEMAP) = range(13)
PT_MAPPING_UV, PT_MAPPING_SPHERICAL, PT_MAPPING_CYLINDRICAL, PT_MAPPING_PLANAR = range(4)


class pt_area_light(C.Structure):
    _fields_ = [("L", C.c_float * 3), ("two_sided", C.c_int32), ("n_samples", C.c_int32)]


class pt_infinite_light(C.Structure):
    _fields_ = [("light_to_world", C.c_float * 16), ("world_to_light", C.c_float * 16), ("image", C.c_int32), ("n_samples", C.c_int32),
                ("light_index", C.c_uint32), ("reserved", C.c_uint32)]


PT_DELTA_POINT, PT_DELTA_SPOT, PT_DELTA_DISTANT = range(3)


class pt_delta_light(C.Structure):
    _fields_ = [("kind", C.c_int32), ("light_index", C.c_uint32), ("light_to_world", C.c_float * 16), ("world_to_light", C.c_float * 16),
                ("spectrum", C.c_float * 3), ("cone_total_width", C.c_float), ("cone_falloff_start", C.c_float), ("direction", C.c_float * 3)]


PT_DELTA_GONIOMETRIC, PT_DELTA_PROJECTION = 3, 4


class pt_map_light(C.Structure):
    """GonioPhotometricLight / ProjectionLight: the constructors' arguments (pt_scene_set_map_lights)."""
    _fields_ = [("kind", C.c_int32), ("light_index", C.c_uint32), ("light_to_world", C.c_float * 16), ("world_to_light", C.c_float * 16),
                ("spectrum", C.c_float * 3), ("image", C.c_int32), ("fov", C.c_float), ("resolution", C.c_int32 * 2)]


PT_ALPHA_NONE, PT_ALPHA_CONSTANT, PT_ALPHA_TEXTURE = range(3)


class pt_alpha_mask(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("alpha_kind", C.c_int32), ("alpha_value", C.c_float), ("alpha_texture", C.c_int32),
                ("shadow_kind", C.c_int32), ("shadow_value", C.c_float), ("shadow_texture", C.c_int32), ("reserved", C.c_uint32 * 5)]


class pt_disney(C.Structure):
    """Material "disney": what pt_material has no field for (value / tex by PT_DISNEY_*)."""
    _fields_ = [("material", C.c_uint32), ("value", C.c_float * 10), ("tex", C.c_uint32 * 10), ("thin", C.c_int32),
                ("scatterdistance", C.c_float * 3), ("tex_scatterdistance", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class pt_fourier_table(C.Structure):
    """Material "fourier": one tabulated BSDF as the C ABI takes it (the arrays stay the caller's)."""
    _fields_ = [("n_mu", C.c_int32), ("n_channels", C.c_int32), ("m_max", C.c_int32), ("n_coeffs", C.c_int32), ("eta", C.c_float),
                ("reserved", C.c_uint32 * 3), ("mu", C.POINTER(C.c_float)), ("cdf", C.POINTER(C.c_float)),
                ("offset_and_length", C.POINTER(C.c_int32)), ("a", C.POINTER(C.c_float))]


class pt_fourier(C.Structure):
    """Material "fourier": which table a PT_MATERIAL_FOURIER material reads."""
    _fields_ = [("material", C.c_uint32), ("table", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class FourierTable:
    """A tabulated BSDF in numpy arrays: mu [n_mu] f4, cdf [n_mu * n_mu] f4, offset_and_length [n_mu * n_mu, 2] i4, a [n_coeffs] f4.
    Nothing is checked here: the upload (and read_fourier_table, for files) refuses a table the kernels could not read safely."""

    def __init__(self, mu, cdf, offset_and_length, a, n_channels, m_max, eta, n_mu=None, n_coeffs=None):
        self.mu = np.ascontiguousarray(mu, dtype=np.float32).reshape(-1)
        self.cdf = np.ascontiguousarray(cdf, dtype=np.float32).reshape(-1)
        self.offset_and_length = np.ascontiguousarray(offset_and_length, dtype=np.int32).reshape(-1)
        self.a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self.n_channels, self.m_max, self.eta = int(n_channels), int(m_max), float(eta)
        self.n_mu = int(self.mu.size if n_mu is None else n_mu)              # (given: a header that disagrees with its arrays, for the refusal tests)
        self.n_coeffs = int(self.a.size if n_coeffs is None else n_coeffs)

    def as_struct(self):
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        t = pt_fourier_table()
        t.n_mu, t.n_channels, t.m_max, t.n_coeffs, t.eta = self.n_mu, self.n_channels, self.m_max, self.n_coeffs, self.eta
        t.mu, t.cdf = self.mu.ctypes.data_as(fp), self.cdf.ctypes.data_as(fp)
        t.offset_and_length = self.offset_and_length.ctypes.data_as(ip)
        t.a = self.a.ctypes.data_as(fp) if self.a.size else None
        return t

    @classmethod
    def from_struct(cls, t):
        """Copies of the arrays a pt_fourier_table points at (a table the library has accepted)."""
        n2 = t.n_mu * t.n_mu
        cp = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt)
        return cls(cp(t.mu, t.n_mu, np.float32), cp(t.cdf, n2, np.float32), cp(t.offset_and_length, 2 * n2, np.int32),
                   cp(t.a, t.n_coeffs, np.float32), t.n_channels, t.m_max, t.eta)


def read_fourier_table(filename, lib=None):
    """pth_fourier_read: a "SCATFUN" file as a FourierTable; PtError (with the file's name) for a file the reader refuses."""
    lib = lib or load_library()
    lib.pth_fourier_read.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    lib.pth_fourier_table_of.argtypes = [C.c_void_p]
    lib.pth_fourier_table_of.restype = C.POINTER(pt_fourier_table)
    lib.pth_fourier_free.argtypes = [C.c_void_p]
    lib.pth_fourier_free.restype = None
    h = C.c_void_p()
    err = C.create_string_buffer(2048)
    st = lib.pth_fourier_read(str(filename).encode(), C.byref(h), err, 2048)
    if st != 0:
        raise PtError(st, err.value.decode())
    try:
        return FourierTable.from_struct(lib.pth_fourier_table_of(h).contents)
    finally:
        lib.pth_fourier_free(h)


class pt_mesh(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("material", C.c_int32), ("area_light", C.c_int32), ("object", C.c_uint32)]


class pt_sphere(C.Structure):
    _fields_ = [("object_to_world", C.c_float * 16), ("world_to_object", C.c_float * 16),
                ("radius", C.c_float), ("zmin", C.c_float), ("zmax", C.c_float), ("phimax", C.c_float),
                ("flags", C.c_uint32), ("material", C.c_int32), ("area_light", C.c_int32),
                ("before_triangle", C.c_uint32), ("object", C.c_uint32), ("order", C.c_uint32), ("kind", C.c_uint32), ("inner_radius", C.c_float)]


class pt_instance(C.Structure):
    _fields_ = [("instance_to_world", C.c_float * 16), ("world_to_instance", C.c_float * 16), ("object", C.c_uint32),
                ("before_triangle", C.c_uint32), ("order", C.c_uint32), ("reserved", C.c_uint32)]


class pt_motion_instance(C.Structure):
    _fields_ = [("instance", C.c_uint32), ("instance_to_world_end", C.c_float * 16), ("world_to_instance_end", C.c_float * 16)]


class pt_motion(C.Structure):
    """Motion blur (pt_scene_set_motion): the transforms at transform_times[1]; the descriptor's are those at transform_times[0]."""
    _fields_ = [("transform_times", C.c_float * 2), ("camera_animated", C.c_int32), ("camera_to_world_end", C.c_float * 16),
                ("n_instances", C.c_uint32), ("instances", C.POINTER(pt_motion_instance))]


PT_SPHERE_REVERSE_ORIENTATION = 1


class pt_scene_desc(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_uint32), ("P", C.POINTER(C.c_float)), ("N", C.POINTER(C.c_float)),
        ("S", C.POINTER(C.c_float)), ("UV", C.POINTER(C.c_float)),
        ("n_triangles", C.c_uint32), ("indices", C.POINTER(C.c_uint32)), ("tri_mesh", C.POINTER(C.c_uint32)),
        ("n_meshes", C.c_uint32), ("meshes", C.POINTER(pt_mesh)),
        ("n_materials", C.c_uint32), ("materials", C.POINTER(pt_material)),
        ("n_area_lights", C.c_uint32), ("area_lights", C.POINTER(pt_area_light)),
        ("split_method", C.c_int32), ("max_node_prims", C.c_int32),
        ("camera_to_world", C.c_float * 16), ("fov", C.c_float), ("screen_window", C.c_float * 4),
        ("lens_radius", C.c_float), ("focal_distance", C.c_float),
        ("shutter_open", C.c_float), ("shutter_close", C.c_float),
        ("xres", C.c_int32), ("yres", C.c_int32), ("crop_window", C.c_float * 4),
        ("filter_radius", C.c_float * 2), ("filter_table", C.c_float * 256),
        ("film_scale", C.c_float), ("max_sample_luminance", C.c_float),
        ("sampler", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
        ("rr_threshold", C.c_float), ("light_strategy", C.c_int32),
        ("halton_sample_at_center", C.c_int32),
        ("n_spheres", C.c_uint32), ("spheres", C.POINTER(pt_sphere)),
        ("n_textures", C.c_uint32), ("textures", C.POINTER(pt_texture)),
        ("n_images", C.c_uint32), ("images", C.POINTER(pt_image)),
        ("n_instances", C.c_uint32), ("instances", C.POINTER(pt_instance)), ("integrator", C.c_int32), ("ao_samples", C.c_int32), ("ao_cos_sample", C.c_int32), ("direct_strategy", C.c_int32),
    ]


class pt_tile(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32)]


class pt_hit(C.Structure):
    _fields_ = [("t", C.c_float), ("prim", C.c_int32), ("b0", C.c_float), ("b1", C.c_float)]


class pt_counters(C.Structure):
    _fields_ = [("camera_rays", C.c_uint64), ("regular_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64), ("path_vertices", C.c_uint64),
                ("trace_launches", C.c_uint64), ("trace_ms", C.c_double), ("shade_ms", C.c_double),
                ("render_ms", C.c_double), ("nodes_from_lds", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class pt_scene_info(C.Structure):
    _fields_ = [("sample_bounds", C.c_int32 * 4), ("cropped_bounds", C.c_int32 * 4), ("spp", C.c_int32),
                ("n_lights", C.c_uint32), ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32),
                ("world_bound", C.c_float * 6), ("bvh_build_ms", C.c_double), ("upload_ms", C.c_double),
                ("bvh_on_device", C.c_int32), ("fourier_capped", C.c_int32)]


BVH_BUILD_AUTO, BVH_BUILD_HOST, BVH_BUILD_DEVICE = 0, 1, 2
PT_INTEGRATOR_PATH, PT_INTEGRATOR_AO, PT_INTEGRATOR_DIRECTLIGHTING, PT_INTEGRATOR_WHITTED, PT_INTEGRATOR_AOV = 0, 1, 2, 3, 4
# pt_aov_target, and the names get_aov_target gives them (integrators/aov.rs:27-56; there is no "duvdy")
(PT_AOV_DISTANCE, PT_AOV_DEPTH, PT_AOV_N, PT_AOV_NS, PT_AOV_UV, PT_AOV_RDXC, PT_AOV_RDYC, PT_AOV_DRODX, PT_AOV_DRDDX, PT_AOV_DPDX, PT_AOV_DPDY,
 PT_AOV_DPDU, PT_AOV_DPDV, PT_AOV_DUVDX, PT_AOV_DUVDY, PT_AOV_DPDUS, PT_AOV_DPDVS) = range(17)
AOV_TARGETS = {"distance": PT_AOV_DISTANCE, "depth": PT_AOV_DEPTH, "n": PT_AOV_N, "ng": PT_AOV_N, "ns": PT_AOV_NS, "uv": PT_AOV_UV,
               "rdxc": PT_AOV_RDXC, "rdyc": PT_AOV_RDYC, "drodx": PT_AOV_DRODX, "drddx": PT_AOV_DRDDX, "dpdx": PT_AOV_DPDX, "dpdy": PT_AOV_DPDY,
               "dpdu": PT_AOV_DPDU, "dpdv": PT_AOV_DPDV, "dstdx": PT_AOV_DUVDX, "dstdy": PT_AOV_DUVDY, "duvdx": PT_AOV_DUVDX,
               "dpdus": PT_AOV_DPDUS, "dpdvs": PT_AOV_DPDVS, "shading.n": PT_AOV_NS, "shading.dpdu": PT_AOV_DPDUS, "shading.dpdv": PT_AOV_DPDVS}
PT_DIRECT_ALL, PT_DIRECT_ONE = 0, 1


HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("b0", "<f4"), ("b1", "<f4")])

# Every symbol include/pbrtgpu.h declares (tests check the library exports them all).
SYMBOLS = [
    "pt_context_create", "pt_context_destroy", "pt_last_error", "pt_abi_version", "pt_set_data_dir",
    "pt_scene_upload", "pt_scene_info_get", "pt_film_clear", "pt_render", "pt_film_download_xyzw",
    "pt_film_device_xyzw", "pt_film_commit_xyzw", "pt_film_allreduce", "pt_film_add_xyzw", "pt_film_resolve_rgb", "pt_trace_closest", "pt_trace_any", "pt_trace_wavefront",
    "pt_generate_camera_rays", "pt_sobol_samples", "pt_radiance_samples", "pt_get_counters", "pt_reset_counters",
    "pt_bvh_leaf_order", "pt_bsdf_eval", "pt_bsdf_sample", "pt_set_bvh_build", "pt_scene_bvh_digest",
    "pt_scene_set_infinite_lights", "pt_light_sample_li", "pt_light_pdf_li", "pt_light_pdf_from", "pt_light_le", "pt_scene_set_alpha_masks",
    "pt_scene_set_aov", "pt_scene_set_delta_lights", "pt_scene_set_disney", "pt_scene_set_map_lights", "pt_scene_kernel_set",
    "pt_scene_set_motion", "pt_trace_closest_time", "pt_trace_any_time", "pt_trace_wavefront_time", "pt_generate_camera_rays_time",
    "pt_motion_decompose", "pt_motion_bounds", "pt_scene_set_fourier",
]
PT_KERNELS_BASE, PT_KERNELS_QUADRIC, PT_KERNELS_DISNEY, PT_KERNELS_MAP_LIGHT, PT_KERNELS_MOTION, PT_KERNELS_FOURIER = 0, 1, 2, 3, 4, 5

_lib = None


def load_library(path=None):
    """dlopen libpbrtgpu.so.  Raises (never substitutes another implementation) if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError("libpbrtgpu.so not found at %s -- build it with __graft_entry__.build(); "
                      "there is no CPU fallback" % p)
    lib = C.CDLL(p)
    vp, u32, fp = C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
    lib.pt_context_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.pt_context_destroy.argtypes = [vp]
    lib.pt_context_destroy.restype = None
    lib.pt_last_error.argtypes = [vp]
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_set_data_dir.argtypes = [vp, C.c_char_p]
    lib.pt_scene_set_aov.argtypes = [vp, C.c_int32, C.c_float]
    lib.pt_scene_upload.argtypes = [vp, C.POINTER(pt_scene_desc)]
    lib.pt_scene_info_get.argtypes = [vp, C.POINTER(pt_scene_info)]
    lib.pt_film_clear.argtypes = [vp]
    lib.pt_render.argtypes = [vp, C.POINTER(pt_tile), u32]
    lib.pt_film_download_xyzw.argtypes = [vp, vp]
    lib.pt_film_device_xyzw.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.pt_film_commit_xyzw.argtypes = [vp]
    lib.pt_film_allreduce.argtypes = [vp, vp, C.c_int]
    lib.pt_film_add_xyzw.argtypes = [vp, fp]
    lib.pt_film_resolve_rgb.argtypes = [vp, vp]
    lib.pt_trace_closest.argtypes = [vp, u32, vp, vp, vp, vp]
    lib.pt_trace_any.argtypes = [vp, u32, vp, vp, vp, vp]
    lib.pt_trace_wavefront.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
    lib.pt_generate_camera_rays.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    lib.pt_sobol_samples.argtypes = [vp, u32, vp, vp, vp, vp]
    lib.pt_radiance_samples.argtypes = [vp, C.POINTER(pt_tile), vp]
    lib.pt_bsdf_eval.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp]
    lib.pt_bsdf_sample.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, vp]
    lib.pt_get_counters.argtypes = [vp, C.POINTER(pt_counters)]
    lib.pt_reset_counters.argtypes = [vp]
    lib.pt_set_bvh_build.argtypes = [vp, C.c_int]
    lib.pt_scene_bvh_digest.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.pt_bvh_leaf_order.argtypes = [C.POINTER(pt_scene_desc), vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def tiles_array(tiles):
    arr = (pt_tile * len(tiles))()
    for i, t in enumerate(tiles):
        arr[i] = pt_tile(*[int(v) for v in t])
    return arr


HOST_SYMBOLS = ["pth_parse_file", "pth_parse_file_opts", "pth_parse_string", "pth_parse_string_opts", "pth_scene_get_desc", "pth_scene_output_filename",
                "pth_scene_set_pixelsamples", "pth_scene_warnings", "pth_scene_free", "pth_write_pfm", "pth_write_image", "pth_parse_to_log",
                "pth_display_connect", "pth_display_start", "pth_display_update", "pth_display_close", "pth_tev_create_packet", "pth_tev_update_packet", "pth_blackbody",
                "pth_scene_get_infinite_lights", "pth_scene_get_alpha_masks", "pth_scene_get_aov", "pth_scene_get_delta_lights", "pth_scene_get_disney", "pth_scene_get_map_lights", "pth_scene_get_motion", "pth_parse_file_features", "pth_parse_string_features",
                "pth_tessellate_loopsubdiv", "pth_tessellate_nurbs", "pth_tessellate_heightfield", "pth_tess_mesh_free",
                "pth_scene_get_fourier", "pth_fourier_read", "pth_fourier_table_of", "pth_fourier_free"]


class pth_options(C.Structure):
    _fields_ = [("quick", C.c_int32), ("quick_full_resolution", C.c_int32), ("pixelsamples", C.c_int32), ("delta_lights", C.c_int32)]


class ParsedScene:
    """A scene parsed from .pbrt text by the C++ front end (include/pbrtgpu_host.h).  Quacks like
    scenes.SceneDesc (has .desc), so it can be uploaded or handed to the oracle."""

    def __init__(self, text=None, filename=None, work_dir=None, lib=None, delta_lights=False, mix_materials=False, quadric_shapes=False,
                 disney_materials=False, point_lights=False, motion_blur=False, fourier_materials=False):
        """delta_lights: take LightSource "spot" / "distant" (pth_options.delta_lights); off, they are refused as before.
        mix_materials: take Material "mix" (PTH_FEATURE_MIX_MATERIAL through pth_parse_*_features); off, it is refused as before.
        quadric_shapes: take Shape "cylinder" and Shape "disk" (PTH_FEATURE_QUADRIC_SHAPES, the same way); off, they are refused as before.
        disney_materials: take Material "disney" (PTH_FEATURE_DISNEY_MATERIAL, the same way); off, it is refused as before.
        point_lights: take LightSource "goniometric", "projection" and "point" (PTH_FEATURE_POINT_LIGHTS, the same way); off, they are refused as before.
        motion_blur: take animated ObjectInstance, Shape and Camera transforms (PTH_FEATURE_MOTION_BLUR, the same way; .motion is then the
        pt_motion record, or None when nothing moves); off, they are refused as before.
        fourier_materials: take Material "fourier" (PTH_FEATURE_FOURIER_MATERIAL, the same way; .fourier_tables / .fourier are then the
        tables read from the "bsdffile"s and the records that name them); off, it is refused as before."""
        self.lib = lib or load_library()
        L = self.lib
        L.pth_parse_file.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        L.pth_parse_string.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        L.pth_scene_get_desc.argtypes = [C.c_void_p]
        L.pth_scene_get_desc.restype = C.POINTER(pt_scene_desc)
        L.pth_scene_output_filename.argtypes = [C.c_void_p]
        L.pth_scene_output_filename.restype = C.c_char_p
        L.pth_scene_warnings.argtypes = [C.c_void_p]
        L.pth_scene_warnings.restype = C.c_char_p
        L.pth_scene_set_pixelsamples.argtypes = [C.c_void_p, C.c_int]
        L.pth_scene_set_pixelsamples.restype = None
        L.pth_scene_free.argtypes = [C.c_void_p]
        L.pth_scene_free.restype = None
        self.h = C.c_void_p()
        err = C.create_string_buffer(2048)
        opts = pth_options(0, 0, 0, 1)
        feat_args = [C.POINTER(pth_options), C.c_uint32, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        features = (PTH_FEATURE_MIX_MATERIAL if mix_materials else 0) | (PTH_FEATURE_DELTA_LIGHTS if delta_lights else 0) | \
                   (PTH_FEATURE_QUADRIC_SHAPES if quadric_shapes else 0) | (PTH_FEATURE_DISNEY_MATERIAL if disney_materials else 0) | \
                   (PTH_FEATURE_POINT_LIGHTS if point_lights else 0) | (PTH_FEATURE_MOTION_BLUR if motion_blur else 0) | \
                   (PTH_FEATURE_FOURIER_MATERIAL if fourier_materials else 0)
        if features & ~PTH_FEATURE_DELTA_LIGHTS and filename is not None:
            L.pth_parse_file_features.argtypes = [C.c_char_p] + feat_args
            st = L.pth_parse_file_features(filename.encode(), None, features, C.byref(self.h), err, 2048)
        elif features & ~PTH_FEATURE_DELTA_LIGHTS:
            L.pth_parse_string_features.argtypes = [C.c_char_p, C.c_char_p] + feat_args
            st = L.pth_parse_string_features(text.encode(), (work_dir or ".").encode(), None, features, C.byref(self.h), err, 2048)
        elif filename is not None and delta_lights:
            L.pth_parse_file_opts.argtypes = [C.c_char_p, C.POINTER(pth_options), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
            st = L.pth_parse_file_opts(filename.encode(), C.byref(opts), C.byref(self.h), err, 2048)
        elif filename is not None:
            st = L.pth_parse_file(filename.encode(), C.byref(self.h), err, 2048)
        elif delta_lights:
            L.pth_parse_string_opts.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(pth_options), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
            st = L.pth_parse_string_opts(text.encode(), (work_dir or ".").encode(), C.byref(opts), C.byref(self.h), err, 2048)
        else:
            st = L.pth_parse_string(text.encode(), (work_dir or ".").encode(), C.byref(self.h), err, 2048)
        if st != 0:
            raise PtError(st, err.value.decode())
        self.desc = L.pth_scene_get_desc(self.h).contents
        self.buffers = {}
        L.pth_scene_get_infinite_lights.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pth_scene_get_infinite_lights.restype = C.POINTER(pt_infinite_light)
        n_inf = C.c_uint32()
        arr = L.pth_scene_get_infinite_lights(self.h, C.byref(n_inf))
        self.infinite_lights = [arr[i] for i in range(n_inf.value)]       # LightSource "infinite" (copies)
        L.pth_scene_get_delta_lights.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pth_scene_get_delta_lights.restype = C.POINTER(pt_delta_light)
        n_dl = C.c_uint32()
        dl = L.pth_scene_get_delta_lights(self.h, C.byref(n_dl))
        self.delta_lights = [pt_delta_light.from_buffer_copy(dl[i]) for i in range(n_dl.value)]    # LightSource "spot" / "distant" (copies)
        L.pth_scene_get_map_lights.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pth_scene_get_map_lights.restype = C.POINTER(pt_map_light)
        n_ml = C.c_uint32()
        ml = L.pth_scene_get_map_lights(self.h, C.byref(n_ml))
        self.map_lights = [pt_map_light.from_buffer_copy(ml[i]) for i in range(n_ml.value)]       # LightSource "goniometric" / "projection" (copies)
        L.pth_scene_get_alpha_masks.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pth_scene_get_alpha_masks.restype = C.POINTER(pt_alpha_mask)
        n_am = C.c_uint32()
        am = L.pth_scene_get_alpha_masks(self.h, C.byref(n_am))
        self.alpha_masks = [pt_alpha_mask.from_buffer_copy(am[i]) for i in range(n_am.value)]      # "alpha" / "shadowalpha" of the meshes (copies)
        L.pth_scene_get_disney.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pth_scene_get_disney.restype = C.POINTER(pt_disney)
        n_dis = C.c_uint32()
        dis = L.pth_scene_get_disney(self.h, C.byref(n_dis))
        self.disney = [pt_disney.from_buffer_copy(dis[i]) for i in range(n_dis.value)]      # Material "disney" records (copies)
        L.pth_scene_get_aov.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        L.pth_scene_get_aov.restype = None
        tgt, scl = C.c_int32(), C.c_float()
        L.pth_scene_get_aov(self.h, C.byref(tgt), C.byref(scl))
        self.aov = (tgt.value, scl.value)         # Integrator "aov": (pt_aov_target, scale)
        L.pth_scene_get_fourier.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(pt_fourier)), C.POINTER(C.c_uint32)]
        L.pth_scene_get_fourier.restype = C.POINTER(pt_fourier_table)
        n_ft, n_fr, frs = C.c_uint32(), C.c_uint32(), C.POINTER(pt_fourier)()
        fts = L.pth_scene_get_fourier(self.h, C.byref(n_ft), C.byref(frs), C.byref(n_fr))
        self.fourier_tables = [FourierTable.from_struct(fts[i]) for i in range(n_ft.value)]          # Material "fourier": the tables (copies) ...
        self.fourier = [pt_fourier.from_buffer_copy(frs[i]) for i in range(n_fr.value)]               # ... and the records that name them
        self.motion = None
        if motion_blur:                           # the motion record (its instance records stay the parsed scene's, which this object keeps alive)
            L.pth_scene_get_motion.argtypes = [C.c_void_p]
            L.pth_scene_get_motion.restype = C.POINTER(pt_motion)
            mo = L.pth_scene_get_motion(self.h)
            self.motion = mo.contents if mo else None

    @property
    def output_filename(self):
        return self.lib.pth_scene_output_filename(self.h).decode()

    @property
    def warnings(self):
        return self.lib.pth_scene_warnings(self.h).decode()

    def set_pixelsamples(self, spp):
        self.lib.pth_scene_set_pixelsamples(self.h, int(spp))

    def __del__(self):
        try:
            if self.h:
                self.lib.pth_scene_free(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


def parse_to_log(text, lib=None):
    """Directive log of the parser alone (pth_parse_to_log); raises PtError on a syntax error."""
    lib = lib or load_library()
    lib.pth_parse_to_log.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    out = C.create_string_buffer(1 << 20)
    st = lib.pth_parse_to_log(text.encode(), b".", out, 1 << 20)
    if st != 0:
        raise PtError(st, out.value.decode())
    return out.value.decode().splitlines()


class pth_tess_mesh(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("P", C.POINTER(C.c_float)), ("N", C.POINTER(C.c_float)),
                ("uv", C.POINTER(C.c_float)), ("indices", C.POINTER(C.c_uint32))]


class pth_nurbs_params(C.Structure):
    _fields_ = [("nu", C.c_int32), ("nv", C.c_int32), ("uorder", C.c_int32), ("vorder", C.c_int32),
                ("uknots", C.POINTER(C.c_float)), ("n_uknots", C.c_size_t), ("vknots", C.POINTER(C.c_float)), ("n_vknots", C.c_size_t),
                ("P", C.POINTER(C.c_float)), ("n_p", C.c_size_t), ("homogeneous", C.c_int32), ("range_given", C.c_int32),
                ("u0", C.c_float), ("u1", C.c_float), ("v0", C.c_float), ("v1", C.c_float), ("diceu", C.c_int32), ("dicev", C.c_int32)]


def _f32_array(a):
    """(contiguous float32 copy, ctypes pointer to it) -- or (None, None) for a missing parameter."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _tess_result(lib, st, m, err):
    """Copy a pth_tess_mesh into numpy arrays (P, N, uv, indices; N / uv None when absent) and free it."""
    if st != 0:
        raise PtError(st, err.value.decode())
    try:
        nv, nt = m.n_vertices, m.n_triangles
        P = np.ctypeslib.as_array(m.P, (nv, 3)).copy() if nv else np.zeros((0, 3), np.float32)
        N = np.ctypeslib.as_array(m.N, (nv, 3)).copy() if m.N else None
        uv = np.ctypeslib.as_array(m.uv, (nv, 2)).copy() if m.uv else None
        idx = np.ctypeslib.as_array(m.indices, (nt, 3)).copy() if nt else np.zeros((0, 3), np.uint32)
    finally:
        lib.pth_tess_mesh_free(C.byref(m))
    return {"P": P, "N": N, "uv": uv, "indices": idx}


def _tess_lib(lib):
    lib = lib or load_library()
    lib.pth_tessellate_loopsubdiv.argtypes = [C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_float), C.c_size_t, C.c_int32,
                                              C.POINTER(pth_tess_mesh), C.c_char_p, C.c_size_t]
    lib.pth_tessellate_nurbs.argtypes = [C.POINTER(pth_nurbs_params), C.POINTER(pth_tess_mesh), C.c_char_p, C.c_size_t]
    lib.pth_tessellate_heightfield.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_size_t, C.POINTER(pth_tess_mesh),
                                               C.c_char_p, C.c_size_t]
    lib.pth_tess_mesh_free.argtypes = [C.POINTER(pth_tess_mesh)]
    lib.pth_tess_mesh_free.restype = None
    return lib


def tessellate_loopsubdiv(indices, P, levels=3, lib=None):
    """Shape "loopsubdiv" (shapes/loopsubdiv.rs) in object space: {"P", "N", "uv": None, "indices"}.  indices / P = None: the
    parameter is missing (the reference's errors).  Raises PtError on what the reference rejects or cannot handle."""
    lib = _tess_lib(lib)
    vi = None if indices is None else np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1).astype(np.int32))
    pa, pp = _f32_array(P)
    m, err = pth_tess_mesh(), C.create_string_buffer(1024)
    st = lib.pth_tessellate_loopsubdiv(vi.ctypes.data_as(C.POINTER(C.c_int32)) if vi is not None else None, 0 if vi is None else len(vi),
                                       pp, 0 if pa is None else len(pa), int(levels), C.byref(m), err, 1024)
    return _tess_result(lib, st, m, err)


def tessellate_nurbs(nu, nv, uorder, vorder, uknots, vknots, P=None, Pw=None, u0=None, u1=None, v0=None, v1=None, diceu=30, dicev=30, lib=None):
    """Shape "nurbs" (shapes/nurbs.rs) in object space: {"P", "N", "uv", "indices"}.  P: 3 floats per control point; Pw: 4
    (homogeneous), used when P is absent; u0 ... v1 = None: the knot range.  -1 / None for nu ... vknots = missing."""
    lib = _tess_lib(lib)
    prm = pth_nurbs_params()
    prm.nu, prm.nv, prm.uorder, prm.vorder = int(nu), int(nv), int(uorder), int(vorder)
    uk, prm.uknots = _f32_array(uknots)
    vk, prm.vknots = _f32_array(vknots)
    prm.n_uknots, prm.n_vknots = 0 if uk is None else len(uk), 0 if vk is None else len(vk)
    cp, prm.homogeneous = (P, 0) if P is not None and len(np.asarray(P).reshape(-1)) else (Pw, 1 if Pw is not None else 0)
    cpa, prm.P = _f32_array(cp)
    prm.n_p = 0 if cpa is None else len(cpa)
    given = 0
    for bit, (name, val) in enumerate((("u0", u0), ("u1", u1), ("v0", v0), ("v1", v1))):
        if val is not None:
            given |= 1 << bit
            setattr(prm, name, float(val))
    prm.range_given = given
    prm.diceu, prm.dicev = int(diceu), int(dicev)
    m, err = pth_tess_mesh(), C.create_string_buffer(1024)
    st = lib.pth_tessellate_nurbs(C.byref(prm), C.byref(m), err, 1024)
    return _tess_result(lib, st, m, err)


def tessellate_heightfield(nu, nv, Pz, lib=None):
    """Shape "heightfield" (shapes/heightfield.rs) in object space: {"P", "N": None, "uv", "indices"}.  Pz = None: missing."""
    lib = _tess_lib(lib)
    za, zp = _f32_array(Pz)
    m, err = pth_tess_mesh(), C.create_string_buffer(1024)
    st = lib.pth_tessellate_heightfield(int(nu), int(nv), zp, 0 if za is None else len(za), C.byref(m), err, 1024)
    return _tess_result(lib, st, m, err)


def bvh_leaf_order(scene, lib=None):
    """Host-only BVH build (no GPU): returns (order, n_nodes, n_leaves, max_stack)."""
    lib = lib or load_library()
    order = np.empty(scene.desc.n_triangles + scene.desc.n_spheres, np.uint32)
    nn, nl, ms = C.c_uint32(), C.c_uint32(), C.c_uint32()
    st = lib.pt_bvh_leaf_order(C.byref(scene.desc), _ptr(order), C.byref(nn), C.byref(nl), C.byref(ms))
    if st != 0:
        raise PtError(st, "pt_bvh_leaf_order failed")
    return order, nn.value, nl.value, ms.value


class Context:
    """One device context (pt_context).  Mirrors the call sequence of the reference's
    render_scene(): build scene -> integrator.render(scene) -> film.write_image()."""

    def __init__(self, device=0, lib=None):
        self.lib = lib or load_library()
        self.h = C.c_void_p()
        st = self.lib.pt_context_create(int(device), C.byref(self.h))
        if st != 0:
            raise PtError(st, "pt_context_create(device=%d) failed (no HIP device? there is no CPU fallback)" % device)
        self._check(self.lib.pt_set_data_dir(self.h, DATA_DIR.encode()))
        self.info = None
        self._keep = None

    def _check(self, st):
        if st != 0:
            msg = self.lib.pt_last_error(self.h)
            raise PtError(st, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.pt_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, scene):
        """scene: scenes.SceneDesc (keeps its numpy buffers alive)."""
        self._keep = scene
        inf = list(getattr(scene, "infinite_lights", None) or [])
        arr = (pt_infinite_light * max(1, len(inf)))(*inf)
        self._check(self.lib.pt_scene_set_infinite_lights(self.h, C.c_uint32(len(inf)), arr if inf else None))
        dls = list(getattr(scene, "delta_lights", None) or [])
        dl_arr = (pt_delta_light * max(1, len(dls)))(*dls)
        self._check(self.lib.pt_scene_set_delta_lights(self.h, C.c_uint32(len(dls)), dl_arr if dls else None))
        mls = list(getattr(scene, "map_lights", None) or [])
        if mls:                      # goniometric / projection lights (an upload consumes them, so a scene without any has nothing to clear)
            ml_arr = (pt_map_light * len(mls))(*mls)
            self.lib.pt_scene_set_map_lights.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(pt_map_light)]
            self._check(self.lib.pt_scene_set_map_lights(self.h, C.c_uint32(len(mls)), ml_arr))
        am = list(getattr(scene, "alpha_masks", None) or [])
        am_arr = (pt_alpha_mask * max(1, len(am)))(*am)
        self._check(self.lib.pt_scene_set_alpha_masks(self.h, C.c_uint32(len(am)), am_arr if am else None))
        dis = list(getattr(scene, "disney", None) or [])
        if dis:                      # Material "disney" records (an upload consumes them, so a scene without any has nothing to clear)
            dis_arr = (pt_disney * len(dis))(*dis)
            self.lib.pt_scene_set_disney.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(pt_disney)]
            self._check(self.lib.pt_scene_set_disney(self.h, C.c_uint32(len(dis)), dis_arr))
        frs = list(getattr(scene, "fourier", None) or [])
        if frs:                      # Material "fourier": the tables and the records that name them (consumed by the upload, like the Disney records)
            tabs = list(getattr(scene, "fourier_tables", None) or [])
            tab_arr = (pt_fourier_table * max(1, len(tabs)))(*[t.as_struct() for t in tabs])
            rec_arr = (pt_fourier * len(frs))(*frs)
            self.lib.pt_scene_set_fourier.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(pt_fourier_table), C.c_uint32, C.POINTER(pt_fourier)]
            self._check(self.lib.pt_scene_set_fourier(self.h, C.c_uint32(len(tabs)), tab_arr, C.c_uint32(len(frs)), rec_arr))
        aov = getattr(scene, "aov", None)
        if aov is not None:          # Integrator "aov": (target, scale); otherwise the upload takes the defaults (uv, 1)
            self._check(self.lib.pt_scene_set_aov(self.h, C.c_int32(int(aov[0])), C.c_float(float(aov[1]))))
        mo = getattr(scene, "motion", None)
        if mo is not None:           # motion blur: a pt_motion (an upload consumes it, so a scene without one has nothing to clear)
            self.lib.pt_scene_set_motion.argtypes = [C.c_void_p, C.POINTER(pt_motion)]
            self._check(self.lib.pt_scene_set_motion(self.h, C.byref(mo)))
        self._check(self.lib.pt_scene_upload(self.h, C.byref(scene.desc)))
        info = pt_scene_info()
        self._check(self.lib.pt_scene_info_get(self.h, C.byref(info)))
        self.info = info
        return info

    def set_bvh_build(self, where):
        """BVH_BUILD_AUTO / _HOST / _DEVICE: where the lower half of an HLBVH build runs at the next upload."""
        self._check(self.lib.pt_set_bvh_build(self.h, int(where)))

    def kernel_set(self):
        """Which build of the kernels renders the uploaded scene: 0 base, 1 quadric (ptq), 2 disney (ptd), 3 map light (ptm), 4 motion (ptv), 5 fourier (ptf)."""
        k = C.c_int32()
        self.lib.pt_scene_kernel_set.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        self._check(self.lib.pt_scene_kernel_set(self.h, C.byref(k)))
        return k.value

    def bvh_digest(self):
        """(nodes, records) FNV-1a digests of the uploaded tree."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.pt_scene_bvh_digest(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def film_shape(self):
        cb = self.info.cropped_bounds
        return (cb[3] - cb[1], cb[2] - cb[0])

    def film_clear(self):
        self._check(self.lib.pt_film_clear(self.h))

    def render(self, tiles=None):
        if tiles is None:
            self._check(self.lib.pt_render(self.h, None, 0))
        else:
            arr = tiles_array(tiles)
            self._check(self.lib.pt_render(self.h, arr, len(tiles)))

    def film_xyzw(self):
        h, w = self.film_shape
        out = np.empty((h, w, 4), np.float32)
        self._check(self.lib.pt_film_download_xyzw(self.h, _ptr(out)))
        return out

    def film_device_xyzw(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self.lib.pt_film_device_xyzw(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def film_commit_xyzw(self):
        self._check(self.lib.pt_film_commit_xyzw(self.h))

    def film_add_xyzw(self, xyzw):
        """Add another rank's {X,Y,Z,weight} film (as film_xyzw() returns it) and make the sum authoritative: the exchange step staged
        through the host."""
        a = np.ascontiguousarray(xyzw, np.float32)
        assert a.size == 4 * self.film_shape[0] * self.film_shape[1]
        self._check(self.lib.pt_film_add_xyzw(self.h, a.ctypes.data_as(C.POINTER(C.c_float))))

    def film_allreduce(self, nccl_comm, root=-1):
        """Sum the XYZW film over an RCCL communicator (ncclComm_t as an integer / c_void_p) inside the library."""
        self._check(self.lib.pt_film_allreduce(self.h, C.c_void_p(nccl_comm), root))

    def film_rgb(self):
        h, w = self.film_shape
        out = np.empty((h, w, 3), np.float32)
        self._check(self.lib.pt_film_resolve_rgb(self.h, _ptr(out)))
        return out

    def trace_closest(self, o, d, tmax, time=None):
        """time: one Ray::time per ray (pt_trace_closest_time); None traces at time 0."""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = len(tmax)
        out = np.empty(n, HIT_DTYPE)
        if time is not None:
            time = np.ascontiguousarray(time, np.float32)
            assert len(time) == n
            self.lib.pt_trace_closest_time.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
            self._check(self.lib.pt_trace_closest_time(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(time), _ptr(out)))
            return out
        self._check(self.lib.pt_trace_closest(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(out)))
        return out

    def trace_any(self, o, d, tmax, time=None):
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = len(tmax)
        out = np.empty(n, np.uint8)
        if time is not None:
            time = np.ascontiguousarray(time, np.float32)
            assert len(time) == n
            self.lib.pt_trace_any_time.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
            self._check(self.lib.pt_trace_any_time(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(time), _ptr(out)))
            return out
        self._check(self.lib.pt_trace_any(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(out)))
        return out

    def trace_wavefront(self, o, d, tmax, kind, time=None):
        """Rays through the renderer's own traversal kernel; kind: 1 continuation, 2 shadow, 3 probe.  Returns (hits, occluded)."""
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32); kind = np.ascontiguousarray(kind, np.uint8)
        n = len(tmax)
        out = np.empty(n, HIT_DTYPE); occ = np.empty(n, np.uint8)
        if time is not None:
            time = np.ascontiguousarray(time, np.float32)
            assert len(time) == n
            self.lib.pt_trace_wavefront_time.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
            self._check(self.lib.pt_trace_wavefront_time(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(time), _ptr(kind), _ptr(out), _ptr(occ)))
            return out, occ
        self._check(self.lib.pt_trace_wavefront(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), _ptr(kind), _ptr(out), _ptr(occ)))
        return out, occ

    def generate_camera_rays(self, pixel_xy, sample_index, with_time=False):
        """(o, d, p_film), and with with_time the rays' times as a fourth array (pt_generate_camera_rays_time)."""
        pixel_xy = np.ascontiguousarray(pixel_xy, np.int32); sample_index = np.ascontiguousarray(sample_index, np.uint32)
        n = len(sample_index)
        o = np.empty((n, 3), np.float32); d = np.empty((n, 3), np.float32); pf = np.empty((n, 2), np.float32)
        if with_time:
            tm = np.empty(n, np.float32)
            self.lib.pt_generate_camera_rays_time.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
            self._check(self.lib.pt_generate_camera_rays_time(self.h, n, _ptr(pixel_xy), _ptr(sample_index), _ptr(o), _ptr(d), _ptr(pf), _ptr(tm)))
            return o, d, pf, tm
        self._check(self.lib.pt_generate_camera_rays(self.h, n, _ptr(pixel_xy), _ptr(sample_index), _ptr(o), _ptr(d), _ptr(pf)))
        return o, d, pf

    def sobol_samples(self, pixel_xy, sample_index, dim):
        pixel_xy = np.ascontiguousarray(pixel_xy, np.int32); sample_index = np.ascontiguousarray(sample_index, np.uint32)
        dim = np.ascontiguousarray(dim, np.uint32)
        n = len(dim)
        out = np.empty(n, np.float32)
        self._check(self.lib.pt_sobol_samples(self.h, n, _ptr(pixel_xy), _ptr(sample_index), _ptr(dim), _ptr(out)))
        return out

    def bsdf_eval(self, material, wo, wi, flags=31):
        """BSDF::f / pdf of one material on the canonical frame (local == world)."""
        wo = np.ascontiguousarray(wo, np.float32); wi = np.ascontiguousarray(wi, np.float32)
        n = len(wo)
        f = np.empty((n, 3), np.float32); pdf = np.empty(n, np.float32)
        self._check(self.lib.pt_bsdf_eval(self.h, C.c_uint32(material), C.c_uint32(n), _ptr(wo), _ptr(wi), C.c_uint32(flags), _ptr(f), _ptr(pdf)))
        return f, pdf

    def bsdf_sample(self, material, wo, u, flags=31):
        """BSDF::sample_f; type 0 = None."""
        wo = np.ascontiguousarray(wo, np.float32); u = np.ascontiguousarray(u, np.float32)
        n = len(wo)
        f = np.empty((n, 3), np.float32); wi = np.empty((n, 3), np.float32); pdf = np.empty(n, np.float32); t = np.empty(n, np.uint32)
        self._check(self.lib.pt_bsdf_sample(self.h, C.c_uint32(material), C.c_uint32(n), _ptr(wo), _ptr(u), C.c_uint32(flags), _ptr(f), _ptr(wi),
                                            _ptr(pdf), _ptr(t)))
        return f, wi, pdf, t

    def light_sample_li(self, light, ref_p, u):
        """Light::sample_li of light `light` (index into the scene's light list): (Li, wi, pdf); pdf 0 where it returns None."""
        ref_p = np.ascontiguousarray(ref_p, np.float32).reshape(-1, 3); u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        n = len(u)
        if len(ref_p) == 1 and n > 1:
            ref_p = np.ascontiguousarray(np.repeat(ref_p, n, axis=0))
        li = np.empty((n, 3), np.float32); wi = np.empty((n, 3), np.float32); pdf = np.empty(n, np.float32)
        self._check(self.lib.pt_light_sample_li(self.h, C.c_uint32(light), C.c_uint32(n), _ptr(ref_p), _ptr(u), _ptr(li), _ptr(wi), _ptr(pdf)))
        return li, wi, pdf

    def light_pdf_li(self, light, wi):
        """InfiniteAreaLight::pdf_li for world directions wi; 0 for a delta light."""
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        pdf = np.empty(len(wi), np.float32)
        self._check(self.lib.pt_light_pdf_li(self.h, C.c_uint32(light), C.c_uint32(len(wi)), _ptr(wi), _ptr(pdf)))
        return pdf

    def light_pdf_from(self, light, ref_p, wi):
        """DiffuseAreaLight::pdf_li (the default Shape::pdf_from) of area light `light` for directions wi from the points ref_p."""
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        ref_p = np.ascontiguousarray(ref_p, np.float32).reshape(-1, 3)
        if len(ref_p) == 1 and len(wi) > 1:
            ref_p = np.ascontiguousarray(np.repeat(ref_p, len(wi), axis=0))
        pdf = np.empty(len(wi), np.float32)
        self.lib.pt_light_pdf_from.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.lib.pt_light_pdf_from(self.h, C.c_uint32(light), C.c_uint32(len(wi)), _ptr(ref_p), _ptr(wi), _ptr(pdf)))
        return pdf

    def light_le(self, light, d):
        """InfiniteAreaLight::le for world ray directions d: RGB."""
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        out = np.empty((len(d), 3), np.float32)
        self._check(self.lib.pt_light_le(self.h, C.c_uint32(light), C.c_uint32(len(d)), _ptr(d), _ptr(out)))
        return out

    def radiance_samples(self, tile):
        t = pt_tile(*[int(v) for v in tile])
        npx = (t.x1 - t.x0) * (t.y1 - t.y0)
        out = np.empty((npx, self.info.spp, 3), np.float32)
        self._check(self.lib.pt_radiance_samples(self.h, C.byref(t), _ptr(out)))
        return out

    def counters(self):
        c = pt_counters()
        self._check(self.lib.pt_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        self._check(self.lib.pt_reset_counters(self.h))


def motion_decompose(m, lib=None):
    """pt_motion_decompose of a 4 x 4 (row-major): (T[3], R[4] as x y z w, S[3]) in float32; raises PtError where the reference's decompose fails."""
    L = lib or load_library()
    a = np.ascontiguousarray(m, np.float32).reshape(16)
    T = np.empty(3, np.float32); R = np.empty(4, np.float32); S = np.empty(3, np.float32)
    L.pt_motion_decompose.argtypes = [C.c_void_p] * 4
    st = L.pt_motion_decompose(_ptr(a), _ptr(T), _ptr(R), _ptr(S))
    if st != 0:
        raise PtError(st, "pt_motion_decompose failed")
    return T, R, S


def motion_bounds(start, end, times, box, lib=None):
    """pt_motion_bounds: AnimatedTransform::motion_bounds of box (min xyz, max xyz) under (start, end) over times; 6 floats."""
    L = lib or load_library()
    a = np.ascontiguousarray(start, np.float32).reshape(16); b = np.ascontiguousarray(end, np.float32).reshape(16)
    t = np.ascontiguousarray(times, np.float32).reshape(2); bx = np.ascontiguousarray(box, np.float32).reshape(6)
    out = np.empty(6, np.float32)
    L.pt_motion_bounds.argtypes = [C.c_void_p] * 5
    st = L.pt_motion_bounds(_ptr(a), _ptr(b), _ptr(t), _ptr(bx), _ptr(out))
    if st != 0:
        raise PtError(st, "pt_motion_bounds failed")
    return out
