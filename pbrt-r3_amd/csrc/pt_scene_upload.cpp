// pt_scene_upload.cpp -- pt_scene_upload of include/pbrtgpu.h: a scene description becomes the device arrays the kernels read (the role of pbrt-r3's
// SceneContext::make_scene + make_integrator, src/core/api/scene_context/scene_context.rs:675-729).  scene_upload() at the end of the file is the
// list of stages; each stage above it is a function of the context, the description and what it reads.
#include "pt_context_impl.h"
#include "pt_fourier_table.h"

namespace {

bool load_sobol(pt_context* ctx) {
    std::string path = ctx->data_dir + "/sobol_tables.bin";
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[8];
    uint32_t hdr[4];
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "PTSOBOL1", 8) == 0 && std::fread(hdr, 4, 4, f) == 4;
    if (ok) {
        ctx->sobol_msize = hdr[1];
        ctx->sobol_n_vdc = hdr[2];
        ctx->sobol_n_inv = hdr[3];
        ctx->sobol_m32.resize((size_t)hdr[0] * hdr[1]);
        ctx->sobol_vdc.resize((size_t)hdr[2] * hdr[1]);
        ctx->sobol_inv.resize((size_t)hdr[3] * hdr[1]);
        ok = std::fread(ctx->sobol_m32.data(), 4, ctx->sobol_m32.size(), f) == ctx->sobol_m32.size() &&
             std::fread(ctx->sobol_vdc.data(), 8, ctx->sobol_vdc.size(), f) == ctx->sobol_vdc.size() &&
             std::fread(ctx->sobol_inv.data(), 8, ctx->sobol_inv.size(), f) == ctx->sobol_inv.size();
    }
    std::fclose(f);
    return ok;
}

pt_status ensure_traversal_scratch(pt_context* ctx) {
    // +1: the top entry is stored too; -1: the pooled-leaf kernels keep a sentinel in LDS slot 0
    uint32_t need = ctx->max_stack + 1 > PT_FS_SLOTS - 1 ? ctx->max_stack + 1 - (PT_FS_SLOTS - 1) : 0;
    size_t threads = (size_t)std::max(ctx->grid_trace, 2048) * PT_BLOCK;
    if (!ctx->d_spill.p || ctx->spill_depth < need) {
        PT_HIP(ctx->d_spill.alloc((size_t)std::max(need, 1u) * threads * 4 + PT_DIAG_WORDS * 4));
        PT_HIP(hipMemsetAsync(ctx->d_spill.p, 0, PT_DIAG_WORDS * 4, ctx->stream));
        ctx->spill_depth = need;
    }
    return PT_OK;
}

// trowbridge_reitz.rs:104-113 (host only: logf)
float roughness_to_alpha(float roughness) {
    roughness = roughness > 1e-3f ? roughness : 1e-3f;
    float x = std::log(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}
// The three roughness parameters after the optional remap (plastic.rs:55-58, glass.rs:76-81, metal.rs:58-69, uber.rs:96-104, substrate.rs:49-54)
void material_alphas(const pt_material& in, float* a_r, float* a_u, float* a_v) {
    auto remap = [&](float r) { return in.remap_roughness ? roughness_to_alpha(r) : r; };
    *a_r = remap(in.roughness); *a_u = remap(in.uroughness); *a_v = remap(in.vroughness);
}
void build_lobes(const pt_material& in, PtMaterial& m) {
    std::memset(&m, 0, sizeof(m));
    float a_r, a_u, a_v;
    material_alphas(in, &a_r, &a_u, &a_v);
    ::build_lobes(in, a_r, a_u, a_v, m);
}

// PCG32 with the reference's default state (core/rng.rs:8-67) -- only the bounded draw that
// shuffle_array (core/sampling/sampling.rs:4-15) needs
struct Pcg32 {
    uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
    uint32_t next() {
        uint64_t old = state;
        state = old * 0x5851f42d4c957f2dULL + inc;
        uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27), rot = (uint32_t)(old >> 59);
        return (xs >> rot) | (xs << ((32u - rot) & 31u));
    }
    uint32_t below(uint32_t b) {
        uint32_t threshold = (0u - b) % b;
        for (;;) {
            uint32_t r = next();
            if (r >= threshold) return r % b;
        }
    }
};
int64_t floor_mod(int64_t a, int64_t b) { int64_t r = a % b; return r < 0 ? r + b : r; }
// x with a*x = 1 (mod n), by the extended Euclid recursion of halton.rs:31-44
int64_t mod_inverse(int64_t a, int64_t n) {
    int64_t r0 = a, r1 = n, x0 = 1, x1 = 0;
    while (r1 != 0) {
        int64_t q = r0 / r1, t = r0 - q * r1;
        r0 = r1; r1 = t;
        t = x0 - q * x1;
        x0 = x1; x1 = t;
    }
    return floor_mod(x0, n);
}
// HaltonSampler::new (samplers/halton.rs:57-112) + compute_radical_inverse_permutations (:12-20)
pt_status setup_halton(pt_context* ctx, PtSobol& sb, int32_t res_x, int32_t res_y, bool at_center) {
    constexpr uint32_t kDims = 1000;          // PRIMES / PRIME_SUMS hold 1000 entries (primes.rs)
    if (!ctx->d_hdims.p) {
        std::vector<uint32_t> primes;
        std::vector<uint8_t> composite(8000, 0);
        for (uint32_t i = 2; primes.size() < kDims; i++) {
            if (composite[i]) continue;
            primes.push_back(i);
            for (uint32_t j = i * i; j < composite.size(); j += i) composite[j] = 1;
        }
        std::vector<uint32_t> dims(4 * (size_t)kDims);
        std::vector<uint16_t> perms;
        Pcg32 rng;
        for (uint32_t i = 0; i < kDims; i++) {
            const uint32_t p = primes[i], off = (uint32_t)perms.size();
            for (uint32_t j = 0; j < p; j++) perms.push_back((uint16_t)j);
            for (uint32_t j = 0; j < p; j++) std::swap(perms[off + j], perms[off + j + rng.below(p - j)]);
            const uint64_t magic = ~0ull / p + 1;           // floor(2^64 / p) + 1 for p not a power of two; p = 2 is never divided this way
            dims[4 * i] = p; dims[4 * i + 1] = off; dims[4 * i + 2] = (uint32_t)magic; dims[4 * i + 3] = (uint32_t)(magic >> 32);
        }
        pt_status st;
        if ((st = upload(ctx, ctx->d_hdims, dims.data(), dims.size())) != PT_OK) return st;
        if ((st = upload(ctx, ctx->d_hperms, perms.data(), perms.size())) != PT_OK) return st;
    }
    sb.h_dims = ctx->d_hdims.as<uint4>();
    sb.h_perms = ctx->d_hperms.as<uint16_t>();
    sb.h_n_dims = kDims;

    sb.h_center = at_center ? 1u : 0u;
    const int32_t res[2] = {res_x, res_y}, bases[2] = {2, 3};
    int32_t scale[2], exp[2];
    for (int i = 0; i < 2; i++) {
        scale[i] = 1; exp[i] = 0;
        while (scale[i] < std::min(res[i], 128)) { scale[i] *= bases[i]; exp[i]++; }
    }
    const int32_t stride = scale[0] * scale[1];
    sb.h_exp[0] = (uint32_t)exp[0]; sb.h_exp[1] = (uint32_t)exp[1];
    sb.h_scale1 = (uint32_t)scale[1];
    sb.h_stride = (uint32_t)stride;
    sb.h_mul[0] = (uint32_t)((stride / scale[0]) * (int32_t)mod_inverse(scale[1], scale[0]));
    sb.h_mul[1] = (uint32_t)((stride / scale[1]) * (int32_t)mod_inverse(scale[0], scale[1]));
    return PT_OK;
}
// Sphere::new + world_bound (sphere.rs:18-59, transform.rs:134-182), or the cylinder's / the disk's by `kind`: device records and BVH build items
static void build_spheres(const pt_scene_desc* d, std::vector<PtSphere>& sph, std::vector<ptbvh::SpherePrim>& sprims) {
    sph.assign(d->n_spheres, PtSphere());
    sprims.assign(d->n_spheres, ptbvh::SpherePrim());
    for (uint32_t i = 0; i < d->n_spheres; i++) {
        const pt_sphere& in = d->spheres[i];
        PtSphere& s = sph[i];
        std::memset(&s, 0, sizeof(s));
        std::memcpy(s.o2w, in.object_to_world, 48);
        std::memcpy(s.w2o, in.world_to_object, 48);
        const float* m = in.object_to_world;
        const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
        const bool swaps = det < 0.0f, reverse = (in.flags & PT_SPHERE_REVERSE_ORIENTATION) != 0;
        auto clampf = [](float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); };
        s.radius = in.radius;
        s.phi_max = clampf(in.phimax, 0.0f, 360.0f) * (3.14159265358979323846f / 180.0f);
        s.flags = (reverse ? PT_SPH_REVERSE : 0u) | ((reverse ^ swaps) ? PT_SPH_FLIP : 0u);
        s.kind = in.kind;
        float lo[3], hi[3];                              // Shape::object_bound
        if (in.kind == PT_SHAPE_CYLINDER) {              // Cylinder::new, object_bound, area (cylinder.rs:20-49, :289-295) after create_cylinder_shape's swap (:340-342)
            s.z_min = in.zmin > in.zmax ? in.zmax : in.zmin;
            s.z_max = in.zmin > in.zmax ? in.zmin : in.zmax;
            s.area = (s.z_max - s.z_min) * s.radius * s.phi_max;
            lo[0] = -s.radius; lo[1] = -s.radius; lo[2] = s.z_min;
            hi[0] = s.radius; hi[1] = s.radius; hi[2] = s.z_max;
        } else if (in.kind == PT_SHAPE_DISK) {           // Disk::new, object_bound (padded by 0.001 along z, as written), area (disk.rs:17-45, :164-169)
            s.z_min = in.zmin;                           // the height
            s.z_max = in.zmin;
            s.inner_radius = in.inner_radius;
            s.area = s.phi_max * 0.5f * (s.radius * s.radius - s.inner_radius * s.inner_radius);
            lo[0] = -s.radius; lo[1] = -s.radius; lo[2] = s.z_min - 0.001f;
            hi[0] = s.radius; hi[1] = s.radius; hi[2] = s.z_min + 0.001f;
        } else {
            s.z_min = clampf(std::fmin(in.zmin, in.zmax), -in.radius, in.radius);
            s.z_max = clampf(std::fmax(s.z_min, in.zmax), -in.radius, in.radius);        // as written (sphere.rs:28)
            s.theta_min = std::acos(clampf(s.z_min / in.radius, -1.0f, 1.0f));
            s.theta_max = std::acos(clampf(s.z_max / in.radius, -1.0f, 1.0f));
            s.area = s.phi_max * s.radius * (s.z_max - s.z_min);
            const float r = s.radius * 1.001f, diff = r - s.radius;
            lo[0] = -r; lo[1] = -r; lo[2] = s.z_min - diff;
            hi[0] = r; hi[1] = r; hi[2] = s.z_max + diff;
        }
        ptbvh::SpherePrim& sp = sprims[i];
        for (int c = 0; c < 8; c++) {
            const float x = (c & 4) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 1) ? hi[2] : lo[2];
            const float q[3] = {m[0] * x + m[1] * y + m[2] * z + m[3], m[4] * x + m[5] * y + m[6] * z + m[7], m[8] * x + m[9] * y + m[10] * z + m[11]};
            for (int k = 0; k < 3; k++) {
                sp.lo[k] = c == 0 ? q[k] : std::fmin(sp.lo[k], q[k]);
                sp.hi[k] = c == 0 ? q[k] : std::fmax(sp.hi[k], q[k]);
            }
        }
        sp.before_triangle = in.before_triangle;
        sp.flags = PT_TRI_SPHERE;
        if (in.material >= 0 && d->materials && d->materials[in.material].type != PT_MATERIAL_NONE) sp.flags |= (uint32_t)(in.material + 1) << PT_TRI_MATERIAL_SHIFT;
    }
}

// ---- InfiniteAreaLight on the host: MIPMap::lookup over a pyramid of pt_image (core/texture/mipmap.rs:503-544, :620-637, :711-765, s repeat,
// t clamp) and make_distribution (lights/infinite.rs:69-91), rows built on the host's threads.
struct EnvMap {
    const pt_image* im;
    std::vector<size_t> off;
    explicit EnvMap(const pt_image& i) : im(&i) {
        size_t o = 0;
        uint32_t w = i.width, h = i.height;
        for (uint32_t l = 0; l < i.n_levels; l++) { off.push_back(o); o += (size_t)w * h * i.channels; if (w > 1) w /= 2; if (h > 1) h /= 2; }
    }
    void dims(uint32_t l, int32_t* w, int32_t* h) const { uint32_t ww = im->width >> l, hh = im->height >> l; *w = (int32_t)(ww ? ww : 1u); *h = (int32_t)(hh ? hh : 1u); }
    void texel(uint32_t l, int32_t s, int32_t t, float out[3]) const {
        int32_t w, h;
        dims(l, &w, &h);
        s &= w - 1;                                                   // repeat
        t = t < 0 ? 0 : (t > h - 1 ? h - 1 : t);                      // clamp
        const float* d = im->texels + off[l] + ((size_t)t * (size_t)w + (size_t)s) * im->channels;
        for (int k = 0; k < 3; k++) out[k] = d[im->channels == 1 ? 0 : k];
    }
    static int32_t f2i(float f) { return std::isnan(f) ? 0 : (f >= 2147483647.0f ? 2147483647 : (f <= -2147483648.0f ? (int32_t)0x80000000 : (int32_t)f)); }
    void triangle(uint32_t l, float st0, float st1, float out[3]) const {
        if (l > im->n_levels - 1) l = im->n_levels - 1;
        int32_t w, h;
        dims(l, &w, &h);
        const float s = st0 * (float)w - 0.5f, t = st1 * (float)h - 0.5f;
        const int32_t s0 = f2i(std::floor(s)), t0 = f2i(std::floor(t));
        const float ds = s - (float)s0, dt = t - (float)t0;
        float a[3], b[3], c[3], e[3];
        texel(l, s0, t0, a); texel(l, s0, t0 + 1, b); texel(l, s0 + 1, t0, c); texel(l, s0 + 1, t0 + 1, e);
        for (int k = 0; k < 3; k++)
            out[k] = a[k] * ((1.0f - ds) * (1.0f - dt)) + b[k] * ((1.0f - ds) * dt) + c[k] * (ds * (1.0f - dt)) + e[k] * (ds * dt);
    }
    void lookup(float st0, float st1, float width, float out[3]) const {          // MIPMap::lookup (trilinear)
        const float max_level = (float)(im->n_levels - 1);
        const float level = max_level + std::log2(std::max(width, 1e-8f));
        if (level < 0.0f) { triangle(0, st0, st1, out); return; }
        if (level >= max_level) { texel(im->n_levels - 1, 0, 0, out); return; }
        const uint32_t il = (uint32_t)std::floor(level);
        const float delta = std::min(std::max(level - (float)il, 0.0f), 1.0f);
        float a[3], b[3];
        triangle(il, st0, st1, a); triangle(il + 1, st0, st1, b);
        for (int k = 0; k < 3; k++) out[k] = (1.0f - delta) * a[k] + delta * b[k];
    }
};
float rgb_y(const float c[3]) { return 0.212671f * c[0] + 0.715160f * c[1] + 0.072169f * c[2]; }
// Distribution1D::new (distribution.rs:34-56) over func[0..n): cdf[0..n], returns func_int
float dist1d_build(const float* func, uint32_t n, float* cdf) {
    cdf[0] = 0.0f;
    for (uint32_t i = 1; i < n + 1; i++) cdf[i] = cdf[i - 1] + func[i - 1] / (float)n;
    const float func_int = cdf[n];
    if (func_int == 0.0f) for (uint32_t i = 1; i < n + 1; i++) cdf[i] = (float)i / (float)n;
    else for (uint32_t i = 1; i < n + 1; i++) cdf[i] /= func_int;
    return func_int;
}
// make_distribution + Distribution2D::new: tables laid out as PtEnvLight reads them -- func [nv][nu], cdf [nv][nu+1], marginal func [nv], cdf [nv+1]
void env_distribution(const pt_image& im, uint32_t* nu_out, uint32_t* nv_out, std::vector<float>* tabs, float* m_int) {
    const EnvMap map(im);
    const uint32_t nu = im.width * 2, nv = im.height * 2;
    const float fwidth = 0.5f / (float)std::min(nu, nv);
    tabs->assign((size_t)nv * nu + (size_t)nv * (nu + 1) + nv + (nv + 1), 0.0f);
    float* func = tabs->data();
    float* cdf = func + (size_t)nv * nu;
    float* mfunc = cdf + (size_t)nv * (nu + 1);
    float* mcdf = mfunc + nv;
    const unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; k++)
        th.emplace_back([&, k] {
            for (uint32_t v = k; v < nv; v += nt) {
                const float vp = ((float)v + 0.5f) / (float)nv;
                const float sin_theta = std::sin(3.14159265358979323846f * vp);
                for (uint32_t u = 0; u < nu; u++) {
                    const float up = ((float)u + 0.5f) / (float)nu;
                    float c[3];
                    map.lookup(up, vp, fwidth, c);
                    func[(size_t)v * nu + u] = std::max(rgb_y(c), 0.0f) * sin_theta;
                }
                mfunc[v] = dist1d_build(func + (size_t)v * nu, nu, cdf + (size_t)v * (nu + 1));
            }
        });
    for (auto& t : th) t.join();
    *m_int = dist1d_build(mfunc, nv, mcdf);
    *nu_out = nu; *nv_out = nv;
}

// ---- what the stages of scene_upload() hand to one another (fields only)
struct SceneChecks { std::vector<uint8_t> mesh_alpha; bool any_alpha = false; };          // mesh_alpha[m] 1: the mesh's triangles carry PT_TRI_ALPHA
// What either build path (build_world_on_device, or the three host stages) leaves for the rest of the upload.  The host path's output arrays are
// ctx->host_bvh: they live in the context between uploads (cleared, capacity retained) while they stay below 1 GB.
struct WorldBuild {
    std::vector<PtSphere> sph;
    std::vector<PtInstance> dinst;
    // motion (pt_scene_set_motion): entry 0 the camera's record, then one per instance that actually moves; per instance its entry (0 = static)
    // and whether its AnimatedTransform has_rotation (motion_bounds' third branch)
    std::vector<PtMotion> motion;
    std::vector<uint32_t> inst_motion;
    std::vector<uint32_t> inst_motion_rec;          // per instance: its pt_motion_instance in ctx->next_motion_inst (read where inst_motion is set)
    std::vector<uint8_t> inst_has_rotation;
    bool camera_moves = false, instances_move = false;
    std::vector<PtLight> lights;
    std::vector<PtTriInfo> tinfo;                   // host path: per leaf record (sphere / instance entries unused)
    std::vector<uint32_t> tri_flags;
    size_t n_world_nodes = 0, up_n_nodes = 0, up_n_tris = 0;
    uint32_t n_top = 0, up_root_ref = PT_EMPTY_REF, up_max_leaf = 0, up_n_leaves = 0;
    float up_root_lo[3] = {0, 0, 0}, up_root_hi[3] = {0, 0, 0};
    bool any_one_sided = false;
    double t1 = 0;
    ptbvh::DeviceBuild dev_build{};
    int max_node_prims = 4;
};
struct MaterialTables {
    std::vector<PtMaterial> mats;
    std::vector<PtMix> mixes;
    std::vector<PtMatParams> mparams;               // textured materials: parameter block + one evaluation program per texture-driven parameter (pt_texture.h)
    std::vector<uint32_t> tex_prog;
    bool general_materials = false, any_textured = false, any_alpha_tex = false;
};
struct Entry { uint32_t kind, idx; };               // a member of a primitive list: 0 triangle, 1 sphere, 2 instance

// A PBRTGPU_BUILD_TRACE line; `last` is null without the switch
void mark(double* last, const char* what) {
    if (last) { const double t = now_ms(); std::fprintf(stderr, "[upload] %s %.1f ms\n", what, t - *last); *last = t; }
}
bool affine(const float* m) { return m[12] == 0.0f && m[13] == 0.0f && m[14] == 0.0f && m[15] == 1.0f; }

// Reads the description and the records set for this upload; writes nothing but the refusal's message.  The first failing check decides status and message.
pt_status check_scene(pt_context* ctx, const pt_scene_desc* d, SceneChecks& chk) {
    // ---- validation (the kernels index these arrays unchecked)
    if (d->n_triangles == 0 && d->n_spheres == 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "scene has no primitives");
    if (d->n_instances > 0 && !d->instances) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "instances array missing");
    for (uint32_t i = 0; i < d->n_instances; i++) {
        const pt_instance& in = d->instances[i];
        if (in.before_triangle > d->n_triangles) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "instance before_triangle exceeds n_triangles");
        if (!affine(in.instance_to_world) || !affine(in.world_to_instance))
            return ctx->fail(PT_ERR_UNSUPPORTED, "object instance under a projective transform (last matrix row must be 0 0 0 1)");
    }
    if (ctx->next_has_motion) {
        const pt_motion& mo = ctx->next_motion;
        if (mo.camera_animated && !affine(mo.camera_to_world_end)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: the camera's end transform is projective (last matrix row must be 0 0 0 1)");
        if (mo.camera_animated && !affine(d->camera_to_world)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: the camera's start transform is projective (last matrix row must be 0 0 0 1)");
        std::vector<uint8_t> seen(d->n_instances, 0);
        for (const pt_motion_instance& mi : ctx->next_motion_inst) {
            if (mi.instance >= d->n_instances) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: instance index out of range");
            if (seen[mi.instance]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: two records for one instance");
            seen[mi.instance] = 1;
            if (!affine(mi.instance_to_world_end) || !affine(mi.world_to_instance_end))
                return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: an instance's end transform is projective (last matrix row must be 0 0 0 1)");
        }
    }
    if (d->n_triangles > 0 && (!d->P || !d->indices || !d->tri_mesh || !d->meshes)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "triangle arrays missing");
    if (d->n_spheres > 0 && !d->spheres) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "spheres array missing");
    if (d->xres <= 0 || d->yres <= 0 || d->spp <= 0 || d->max_depth < 0 || d->max_depth > 250) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bad film / sampler / integrator parameters");
    if (d->integrator < PT_INTEGRATOR_PATH || d->integrator > PT_INTEGRATOR_AOV) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "unknown integrator");
    if (d->integrator == PT_INTEGRATOR_DIRECTLIGHTING && d->direct_strategy != PT_DIRECT_ALL && d->direct_strategy != PT_DIRECT_ONE)
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "unknown directlighting strategy");
    if ((d->integrator == PT_INTEGRATOR_DIRECTLIGHTING || d->integrator == PT_INTEGRATOR_WHITTED) && d->max_depth > 16)
        return ctx->fail(PT_ERR_UNSUPPORTED, "directlighting / whitted: maxdepth above 16 (one frame per level is kept per camera sample)");
    if (d->n_materials > 0 && !d->materials) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "materials array missing");
    if (d->n_area_lights > 0 && !d->area_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "area lights array missing");
    for (uint32_t i = 0; i < d->n_area_lights; i++)
        if (d->area_lights[i].n_samples < 0 || d->area_lights[i].n_samples > 4096) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "area light nsamples outside [0, 4096]");
    if (d->sampler != PT_SAMPLER_SOBOL && d->sampler != PT_SAMPLER_HALTON)
        return ctx->fail(PT_ERR_UNSUPPORTED, "sampler not on the accelerated path: only the index-addressed samplers (sobol, halton) are reproducible on a wavefront");
    if (d->n_triangles >= 0x7fffffffu) return ctx->fail(PT_ERR_UNSUPPORTED, "too many triangles");
    for (uint32_t t = 0; t < d->n_triangles; t++) {
        for (int k = 0; k < 3; k++)
            if (d->indices[3 * (size_t)t + k] >= d->n_vertices) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "vertex index out of range");
        if (d->tri_mesh[t] >= d->n_meshes) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "mesh index out of range");
    }
    for (uint32_t m = 0; m < d->n_meshes; m++) {
        if (d->meshes[m].material >= (int32_t)d->n_materials) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "material index out of range");
        if (d->meshes[m].material >= 65535) return ctx->fail(PT_ERR_UNSUPPORTED, "more than 65534 materials");
        if (d->meshes[m].area_light >= (int32_t)d->n_area_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "area light index out of range");

        int32_t mi = d->meshes[m].material;
        if (mi >= 0 && (d->materials[mi].type < PT_MATERIAL_NONE || d->materials[mi].type > PT_MATERIAL_FOURIER))
            return ctx->fail(PT_ERR_UNSUPPORTED, "material type not on the accelerated path");
    }
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const pt_material& m = d->materials[i];
        if (m.type == PT_MATERIAL_MIX) {       // "amount" in kd / tex_kd, the children as material index + 1 in tex_kr / tex_kt; nothing else is read
            if (m.tex_kd > d->n_textures || (m.tex_kd && !d->textures)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "material texture index out of range");
            if (m.tex_kr == 0 || m.tex_kr > i || m.tex_kt == 0 || m.tex_kt > i)
                return ctx->fail(PT_ERR_INVALID_ARGUMENT, "material " + std::to_string(i) + " (mix): a child's material index must be smaller than the mix's own (definition order)");
            continue;
        }
        const uint32_t refs[13] = {m.tex_kd, m.tex_ks, m.tex_kr, m.tex_kt, m.tex_opacity, m.tex_sigma, m.tex_metal_eta, m.tex_metal_k, m.tex_bump,
                                   m.tex_roughness, m.tex_uroughness, m.tex_vroughness, m.tex_eta};
        for (uint32_t r : refs)
            if (r > d->n_textures || (r && !d->textures)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "material texture index out of range");
    }
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const pt_texture& t = d->textures[i];
        if (t.type < PT_TEX_CONSTANT || t.type > PT_TEX_IMAGEMAP) return ctx->fail(PT_ERR_UNSUPPORTED, "texture class not on the accelerated path");
        if (t.mapping < PT_MAPPING_UV || t.mapping > PT_MAPPING_PLANAR) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "unknown texture mapping");
        for (int k = 0; k < 3; k++)
            if (t.tex[k] >= (int32_t)i) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "texture child index must be smaller than the texture's own (definition order)");
        if (t.type == PT_TEX_IMAGEMAP) {
            if (t.image < 0 || (uint32_t)t.image >= d->n_images || !d->images) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "imagemap image index out of range");
            if (t.swrap < PT_WRAP_REPEAT || t.swrap > PT_WRAP_CLAMP || t.twrap < PT_WRAP_REPEAT || t.twrap > PT_WRAP_CLAMP) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "unknown image wrap mode");
        }
    }
    for (uint32_t i = 0; i < d->n_images; i++) {
        const pt_image& im = d->images[i];
        auto pow2 = [](uint32_t v) { return v != 0 && (v & (v - 1)) == 0; };
        uint32_t lv = 1;
        for (uint32_t m = std::max(im.width, im.height); m > 1; m >>= 1) lv++;
        if (!pow2(im.width) || !pow2(im.height) || (im.channels != 1 && im.channels != 3) || !im.texels || im.n_levels != lv || lv > PT_MAX_MIP_LEVELS)
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "image pyramid: level 0 must be power-of-two sized, 1 or 3 channels, with 1 + log2(max(w, h)) levels");
    }
    for (uint32_t i = 0; i < d->n_spheres; i++) {
        const pt_sphere& sp = d->spheres[i];
        if (sp.kind > PT_SHAPE_DISK) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "analytic shape of unknown kind (PT_SHAPE_SPHERE, PT_SHAPE_CYLINDER and PT_SHAPE_DISK are known)");
        const std::string shape = sp.kind == PT_SHAPE_CYLINDER ? "cylinder" : (sp.kind == PT_SHAPE_DISK ? "disk" : "sphere");
        if (sp.material >= (int32_t)d->n_materials || sp.material >= 65535) return ctx->fail(PT_ERR_INVALID_ARGUMENT, shape + " material index out of range");
        if (sp.area_light >= (int32_t)d->n_area_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, shape + " area light index out of range");
        if (sp.material >= 0 && (d->materials[sp.material].type < PT_MATERIAL_NONE || d->materials[sp.material].type > PT_MATERIAL_FOURIER))
            return ctx->fail(PT_ERR_UNSUPPORTED, "material type not on the accelerated path");
        if (sp.before_triangle > d->n_triangles) return ctx->fail(PT_ERR_INVALID_ARGUMENT, shape + " before_triangle exceeds n_triangles");
        if (sp.kind != PT_SHAPE_SPHERE) {
            const bool finite = std::isfinite(sp.radius) && std::isfinite(sp.zmin) && std::isfinite(sp.phimax) && (sp.kind == PT_SHAPE_DISK ? std::isfinite(sp.inner_radius) : std::isfinite(sp.zmax));
            if (!finite) return ctx->fail(PT_ERR_INVALID_ARGUMENT, shape + " parameters must be finite");
        }
        if (!(sp.radius > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, shape + " radius must be positive");
        if (sp.kind == PT_SHAPE_DISK && !(sp.inner_radius >= 0.0f && sp.inner_radius < sp.radius))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disk inner_radius must be in [0, radius)");
        if (!affine(sp.object_to_world) || !affine(sp.world_to_object))
            return ctx->fail(PT_ERR_UNSUPPORTED, shape + " under a projective transform (last matrix row must be 0 0 0 1)");
    }
    for (const pt_infinite_light& il : ctx->inf_lights) {
        if (il.image < 0 || (uint32_t)il.image >= d->n_images || !d->images) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "infinite light: image index out of range");
        const pt_image& im = d->images[il.image];
        if (!im.texels || im.width == 0 || im.height == 0 || (im.width & (im.width - 1)) || (im.height & (im.height - 1)) || (im.channels != 1 && im.channels != 3) ||
            im.n_levels == 0 || im.n_levels > PT_MAX_MIP_LEVELS || im.width > (1u << 14) || im.height > (1u << 14))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "infinite light: its image is not a power-of-two pyramid of 1 or 3 channels (at most 16384 wide)");
        if (il.n_samples < 0 || il.n_samples > 4096) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "infinite light: n_samples outside [0, 4096]");
    }
    for (const pt_delta_light& dl : ctx->delta_lights) {
        if (dl.kind < PT_DELTA_POINT || dl.kind > PT_DELTA_DISTANT) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "delta light: unknown kind");
        if (!affine(dl.light_to_world) || !affine(dl.world_to_light))
            return ctx->fail(PT_ERR_UNSUPPORTED, "delta light under a projective transform (last matrix row must be 0 0 0 1)");
    }
    for (const pt_map_light& ml : ctx->map_lights) {
        if (ml.kind != PT_DELTA_GONIOMETRIC && ml.kind != PT_DELTA_PROJECTION) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "map light: unknown kind (PT_DELTA_GONIOMETRIC and PT_DELTA_PROJECTION are known)");
        const char* name = ml.kind == PT_DELTA_GONIOMETRIC ? "goniometric light" : "projection light";
        if (!affine(ml.light_to_world) || !affine(ml.world_to_light))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, std::string(name) + " under a projective transform (last matrix row must be 0 0 0 1)");
        if (ml.image < 0 || (uint32_t)ml.image >= d->n_images || !d->images) return ctx->fail(PT_ERR_INVALID_ARGUMENT, std::string(name) + ": image index out of range");
        const pt_image& im = d->images[ml.image];
        if (!im.texels || im.width == 0 || im.height == 0 || (im.width & (im.width - 1)) || (im.height & (im.height - 1)) || im.channels != 3 || im.n_levels == 0 ||
            im.n_levels > PT_MAX_MIP_LEVELS || im.width > (1u << 14) || im.height > (1u << 14))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, std::string(name) + ": its image is not a power-of-two pyramid of 3 channels (at most 16384 wide)");
        if (ml.kind == PT_DELTA_PROJECTION && (ml.resolution[0] <= 0 || ml.resolution[1] <= 0))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "projection light: resolution must be positive");
    }
    // alpha masks: one record per mesh, float textures only (a texture whose channels are equal wherever it is evaluated)
    std::vector<uint8_t>& mesh_alpha = chk.mesh_alpha;
    mesh_alpha.assign(d->n_meshes, 0);
    {
        std::vector<int8_t> is_float(d->n_textures, 0);
        auto eq3 = [](const float* v) { return v[0] == v[1] && v[1] == v[2]; };
        for (uint32_t i = 0; i < d->n_textures; i++) {
            const pt_texture& t = d->textures[i];
            auto slot = [&](int k) { return t.tex[k] >= 0 ? is_float[t.tex[k]] != 0 : eq3(t.value[k]); };
            bool f = false;
            switch (t.type) {
                case PT_TEX_CONSTANT: f = eq3(t.value[0]); break;
                case PT_TEX_SCALE: case PT_TEX_CHECKERBOARD_2D: case PT_TEX_CHECKERBOARD_3D: case PT_TEX_DOTS: f = slot(0) && slot(1); break;
                case PT_TEX_MIX: f = slot(0) && slot(1); break;       // (the amount is read as channel 0 either way)
                case PT_TEX_BILERP: f = eq3(t.value[0]) && eq3(t.value[1]) && eq3(t.value[2]) && eq3(t.value[3]); break;
                case PT_TEX_FBM: case PT_TEX_WRINKLED: case PT_TEX_WINDY: f = true; break;
                case PT_TEX_IMAGEMAP: f = d->images[t.image].channels == 1; break;
                default: f = false; break;           // uv, marble: three different channels
            }
            is_float[i] = f ? 1 : 0;
        }
        for (const pt_alpha_mask& am : ctx->alpha_masks) {
            if (am.mesh >= d->n_meshes) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "alpha mask: mesh index out of range");
            if (mesh_alpha[am.mesh]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "alpha mask: two records for one mesh");
            const int32_t kinds[2] = {am.alpha_kind, am.shadow_kind}, texs[2] = {am.alpha_texture, am.shadow_texture};
            for (int k = 0; k < 2; k++) {
                if (kinds[k] < PT_ALPHA_NONE || kinds[k] > PT_ALPHA_TEXTURE) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "alpha mask: unknown kind");
                if (kinds[k] == PT_ALPHA_TEXTURE) {
                    if (texs[k] < 0 || (uint32_t)texs[k] >= d->n_textures || !d->textures) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "alpha mask: texture index out of range");
                    if (!is_float[texs[k]]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "alpha mask: not a float texture");
                }
            }
            // AlphaMaskShape::new (alphamask.rs:27-53): a constant > 0 does nothing
            const bool live = am.alpha_kind == PT_ALPHA_TEXTURE || am.shadow_kind == PT_ALPHA_TEXTURE || (am.alpha_kind == PT_ALPHA_CONSTANT && am.alpha_value <= 0.0f) ||
                              (am.shadow_kind == PT_ALPHA_CONSTANT && am.shadow_value <= 0.0f);
            mesh_alpha[am.mesh] = live ? 1 : 2;
        }
        for (uint8_t& m : mesh_alpha) if (m == 2) m = 0;
        // Material "disney": one record per Disney material, float textures behind its float parameters ("eta" and "roughness" of pt_material included)
        std::vector<uint8_t> seen(d->n_materials, 0);
        for (const pt_disney& r : ctx->disney_recs) {
            if (r.material >= d->n_materials) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: material index out of range");
            if (d->materials[r.material].type != PT_MATERIAL_DISNEY) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: a record for a material that is not a Disney material");
            if (seen[r.material]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: two records for one material");
            seen[r.material] = 1;
            for (uint32_t t : r.tex) {
                if (t > d->n_textures || (t && !d->textures)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: texture index out of range");
                if (t && !is_float[t - 1]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: a colour texture behind a float parameter");
            }
            if (r.tex_scatterdistance > d->n_textures || (r.tex_scatterdistance && !d->textures)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: texture index out of range");
            if (!r.thin && (r.tex_scatterdistance || r.scatterdistance[0] != 0.0f || r.scatterdistance[1] != 0.0f || r.scatterdistance[2] != 0.0f))
                return ctx->fail(PT_ERR_UNSUPPORTED, "disney: non-black \"scatterdistance\" on a material that is not thin asks for the Disney BSSRDF, which the reference does not "
                                                     "finish (todo!(), disney.rs:712); set \"thin\" or leave \"scatterdistance\" black");
        }
        for (uint32_t i = 0; i < d->n_materials; i++) {
            const pt_material& m = d->materials[i];
            if (m.type != PT_MATERIAL_DISNEY) continue;
            for (uint32_t t : {m.tex_eta, m.tex_roughness, m.tex_bump})
                if (t && !is_float[t - 1]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "disney: a colour texture behind a float parameter");
        }
    }
    {   // Material "fourier": exactly one record per such material, each naming a table that keeps the rules of pt_fourier_table.h
        std::vector<uint8_t> seen(d->n_materials, 0);
        for (const pt_fourier& r : ctx->fourier_recs) {
            if (r.material >= d->n_materials) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "fourier: material index out of range");
            if (d->materials[r.material].type != PT_MATERIAL_FOURIER) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "fourier: a record for a material that is not a Fourier material");
            if (seen[r.material]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "fourier: two records for one material");
            if (r.table >= ctx->fourier_tables.size()) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "fourier: table index out of range");
            seen[r.material] = 1;
        }
        for (size_t t = 0; t < ctx->fourier_tables.size(); t++)
            if (!ctx->fourier_tables[t].refusal.empty()) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "fourier: table " + std::to_string(t) + ": " + ctx->fourier_tables[t].refusal);
        for (uint32_t i = 0; i < d->n_materials; i++)
            if (d->materials[i].type == PT_MATERIAL_FOURIER && !seen[i])
                return ctx->fail(PT_ERR_INVALID_ARGUMENT, "fourier: material " + std::to_string(i) + " has no record (pt_scene_set_fourier names its table)");
    }
    chk.any_alpha = false;
    for (uint8_t m : mesh_alpha) chk.any_alpha |= m != 0;
    // integrator-specific refusals come after the index range checks above (they dereference materials[])
    if (d->integrator == PT_INTEGRATOR_PATH && d->sampler == PT_SAMPLER_HALTON && d->max_depth > 124)
        return ctx->fail(PT_ERR_UNSUPPORTED, "path with the Halton sampler and maxdepth above 124: a path that long asks for more than the sampler's 1000 "
                                             "dimensions (5 for the camera, 8 per vertex), where the reference panics (halton.rs:103-108)");
    if (d->integrator == PT_INTEGRATOR_AO) {
        if (d->ao_samples < 1 || d->ao_samples > 4096) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "ao: nsamples outside [1, 4096]");
        for (uint32_t i = 0; i < d->n_meshes; i++)
            if (d->meshes[i].material < 0 || d->materials[d->meshes[i].material].type == PT_MATERIAL_NONE)
                return ctx->fail(PT_ERR_UNSUPPORTED, "ao: a surface without a material makes the reference request its sample array twice and panic (ao.rs:66-69, :78)");
        for (uint32_t i = 0; i < d->n_spheres; i++)
            if (d->spheres[i].material < 0 || d->materials[d->spheres[i].material].type == PT_MATERIAL_NONE)
                return ctx->fail(PT_ERR_UNSUPPORTED, "ao: a surface without a material makes the reference request its sample array twice and panic (ao.rs:66-69, :78)");
        for (uint32_t i = 0; i < d->n_materials; i++)
            if (d->materials[i].tex_bump) return ctx->fail(PT_ERR_UNSUPPORTED, "ao: bump-mapped materials (the bump can flip the frame's normal) are not on the accelerated path");
    }
    return PT_OK;
}

// ---- the records both build paths make, written once
// A mesh's flags with the attribute bits of arrays the description lacks masked out (PtTriInfo::mesh_flags, PtLight::mesh_flags)
static inline uint32_t mesh_attr_flags(const pt_scene_desc* d, uint32_t mesh) {
    uint32_t mf = d->meshes[mesh].flags;
    if (!d->N) mf &= ~PT_MESH_HAS_N;
    if (!d->S) mf &= ~PT_MESH_HAS_S;
    if (!d->UV) mf &= ~PT_MESH_HAS_UV;
    return mf;
}
// The leaf-record flags every triangle of a mesh carries
static inline uint32_t mesh_tri_flags(const pt_scene_desc* d, uint32_t mesh, const std::vector<uint8_t>& mesh_alpha) {
    const uint32_t mf = mesh_attr_flags(d, mesh);
    uint32_t f = 0;
    if (!(mf & PT_MESH_TWO_SIDED)) f |= PT_TRI_ONE_SIDED;
    if (((mf & PT_MESH_REVERSE_ORIENTATION) != 0) ^ ((mf & PT_MESH_SWAPS_HANDEDNESS) != 0)) f |= PT_TRI_FLIP;
    if (mf & (PT_MESH_HAS_N | PT_MESH_HAS_S | PT_MESH_HAS_UV)) f |= PT_TRI_HAS_ATTR;
    const int32_t mat = d->meshes[mesh].material;
    if (mat >= 0 && d->materials[mat].type != PT_MATERIAL_NONE) f |= (uint32_t)(mat + 1) << PT_TRI_MATERIAL_SHIFT;
    if (mesh_alpha[mesh]) f |= PT_TRI_ALPHA;
    return f;
}
// What every DiffuseAreaLight record holds, the rest zero
static inline PtLight area_light_record(const pt_area_light& al, uint32_t rec, uint32_t prim) {
    PtLight L;
    std::memset(&L, 0, sizeof(L));
    L.two_sided = al.two_sided;
    L.n_samples = (uint32_t)std::max(1, al.n_samples);
    std::memcpy(L.L, al.L, 12);
    L.tri_rec = rec;
    L.prim = prim;
    return L;
}
// The light of emissive triangle t, whose leaf record is `rec` and which is primitive `prim` of the world list; mesh_flags = mesh_attr_flags of its mesh
static inline PtLight triangle_light(const pt_scene_desc* d, uint32_t t, uint32_t mesh_flags, uint32_t rec, uint32_t prim) {
    const pt_area_light& al = d->area_lights[d->meshes[d->tri_mesh[t]].area_light];
    const uint32_t v0 = d->indices[3 * (size_t)t], v1 = d->indices[3 * (size_t)t + 1], v2 = d->indices[3 * (size_t)t + 2];
    const float* p0 = d->P + 3 * (size_t)v0; const float* p1 = d->P + 3 * (size_t)v1; const float* p2 = d->P + 3 * (size_t)v2;
    PtLight L = area_light_record(al, rec, prim);
    std::memcpy(L.p0, p0, 12); std::memcpy(L.p1, p1, 12); std::memcpy(L.p2, p2, 12);
    // Triangle::area (triangle.rs:579-588)
    float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    float cx = (ay * bz) - (az * by), cy = (az * bx) - (ax * bz), cz = (ax * by) - (ay * bx);
    L.area = 0.5f * std::sqrt(cx * cx + cy * cy + cz * cz);
    L.mesh_flags = mesh_flags;
    if (mesh_flags & PT_MESH_HAS_N) { std::memcpy(L.n0, d->N + 3 * (size_t)v0, 12); std::memcpy(L.n1, d->N + 3 * (size_t)v1, 12); std::memcpy(L.n2, d->N + 3 * (size_t)v2, 12); }
    return L;
}
// The light of emissive sphere (cylinder, disk) si of surface area `area`
static inline PtLight sphere_light(const pt_scene_desc* d, uint32_t si, float area, uint32_t rec, uint32_t prim) {
    PtLight L = area_light_record(d->area_lights[d->spheres[si].area_light], rec, prim);
    std::memcpy(&L.p0[0], &si, 4);
    L.area = area;
    L.mesh_flags = PT_LIGHT_SPHERE;
    return L;
}

// ---- BVH, records and nodes on the device --------------------------------
// A world list of triangles only (no spheres, objects or instances) under the SAH or HLBVH split -- BASELINE's scenes -- never leaves the
// AnimatedTransform::new (animated_transform.rs:23-61) for the camera and for every instance with a motion record: both ends decomposed, the record
// the kernels interpolate from.  A pair whose ends are equal is not actually animated and stays what it was: no record, the kernels it ran before.
// interpolate lerps the scale: a component that changes sign (or is zero at an end) passes through zero, M(t) is singular there and the
// reference's Transform::from panics.  Such a pair is refused.
bool scale_keeps_its_sign(const PtMotion& r) {
    for (int i = 0; i < 3; i++) if (!(r.S[0][i] * r.S[1][i] > 0.0f)) return false;
    return true;
}
pt_status build_motion_records(pt_context* ctx, const pt_scene_desc* d, WorldBuild& w) {
    w.inst_motion.assign(d->n_instances, 0u);
    w.inst_has_rotation.assign(d->n_instances, 0);
    w.inst_motion_rec.assign(d->n_instances, 0u);
    // The build of the kernels that knows Material "fourier" contains the motion build: it reads the camera's record whatever the scene does, so a
    // scene that holds such a material and does not move gets that one record, not animated (pt_motion_at hands back the stored transforms)
    bool fourier = false;
    for (uint32_t i = 0; i < d->n_materials; i++) fourier |= d->materials[i].type == PT_MATERIAL_FOURIER;
    if (!ctx->next_has_motion) {
        if (fourier) { PtMotion still; std::memset(&still, 0, sizeof(still)); w.motion.push_back(still); }
        return PT_OK;
    }
    const pt_motion& mo = ctx->next_motion;
    PtMotion cam;
    std::memset(&cam, 0, sizeof(cam));
    bool rot = false;
    if (mo.camera_animated) {
        // (the camera keeps no inverse: the same stand-in at both ends leaves the comparison to the matrices)
        if (!ptmotion::make_record(d->camera_to_world, d->camera_to_world, mo.camera_to_world_end, d->camera_to_world, mo.transform_times, &cam, &rot))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: decompose failed on a camera transform");
        w.camera_moves = cam.animated != 0;
        if (w.camera_moves && !scale_keeps_its_sign(cam)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: the camera's scale changes sign between the two times (the interpolated transform is singular on the way)");
    }
    w.motion.push_back(cam);
    for (const pt_motion_instance& mi : ctx->next_motion_inst) {
        const pt_instance& in = d->instances[mi.instance];
        PtMotion rec;
        if (!ptmotion::make_record(in.instance_to_world, in.world_to_instance, mi.instance_to_world_end, mi.world_to_instance_end, mo.transform_times, &rec, &rot))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: decompose failed on a transform of instance " + std::to_string(mi.instance));
        if (!rec.animated) continue;
        if (!scale_keeps_its_sign(rec))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: the scale of instance " + std::to_string(mi.instance) + " changes sign between the two times (the interpolated transform is singular on the way)");
        w.inst_motion[mi.instance] = (uint32_t)w.motion.size();
        w.inst_motion_rec[mi.instance] = (uint32_t)(&mi - ctx->next_motion_inst.data());
        w.inst_has_rotation[mi.instance] = rot ? 1 : 0;
        w.motion.push_back(rec);
        w.instances_move = true;
    }
    if (!w.camera_moves && !w.instances_move) {
        w.motion.clear();
        if (fourier) { std::memset(&cam, 0, sizeof(cam)); w.motion.push_back(cam); }
    }
    return PT_OK;
}

// device: vertices and indices go up, pt_sah.hip / pt_hlbvh.hip build the binary tree, pt_sah.hip writes the leaf and shading records in leaf order, collapses
// the tree into the 4-wide node array in the reference's depth-first numbering and finishes it (breadth-first top, order tables, axis
// bits, inverted empty slots).  Same arrays as the host path below, byte for byte (tests/test_gpu_hlbvh.py compares the digests).
// A list that needs a fallback split, PT_BVH_BUILD_HOST or PBRTGPU_HOST_FINISH=1 take the host path: *took stays false.
pt_status build_world_on_device(pt_context* ctx, const pt_scene_desc* d, const SceneChecks& chk, WorldBuild& w, double* trace, bool* took) {
    uint32_t any_object = 0;
    for (uint32_t i = 0; i < d->n_meshes; i++) any_object |= d->meshes[i].object;
    for (uint32_t i = 0; i < d->n_spheres; i++) any_object |= d->spheres[i].object;
    const int mnp = std::min(std::max(w.max_node_prims, 0), 255);
    const bool sah = d->split_method == PT_SPLIT_SAH && mnp >= 2, hl = d->split_method == PT_SPLIT_HLBVH && mnp >= 1;
    const uint64_t n_world = (uint64_t)d->n_triangles + d->n_spheres;
    // (round 4: analytic spheres of the world list ride along -- a handful of them among the triangles, killeroo-simple's two sphere lights --;
    // objects and instances still take the host path)
    if (!(d->n_instances == 0 && any_object == 0 && (sah || hl) && n_world >= 2 &&
          n_world < PT_LEAF_FIRST_MASK - 16u && ctx->bvh_build_where != PT_BVH_BUILD_HOST &&
          (ctx->bvh_build_where == PT_BVH_BUILD_DEVICE || n_world >= ptbvh::kDeviceMinPrims) && !std::getenv("PBRTGPU_HOST_FINISH"))) return PT_OK;
    std::vector<uint32_t> m_triflags(d->n_meshes), m_flags(d->n_meshes);
    std::vector<int32_t> m_material(d->n_meshes);
    for (uint32_t i = 0; i < d->n_meshes; i++) {
        m_triflags[i] = mesh_tri_flags(d, i, chk.mesh_alpha);
        m_flags[i] = mesh_attr_flags(d, i);
        m_material[i] = d->meshes[i].material;
    }
    // the world list's spheres in list order (spliced in before triangle `before_triangle`, ties in creation order: make_list below)
    std::vector<ptbvh::SpherePrim> sprims;
    std::vector<uint32_t> s_order(d->n_spheres), s_prim(d->n_spheres), s_rec(4 * (size_t)d->n_spheres);
    std::vector<float> s_bounds(6 * (size_t)d->n_spheres);
    if (d->n_spheres) {
        build_spheres(d, w.sph, sprims);
        for (uint32_t i = 0; i < d->n_spheres; i++) s_order[i] = i;
        std::stable_sort(s_order.begin(), s_order.end(), [&](uint32_t x, uint32_t y) {
            return d->spheres[x].before_triangle != d->spheres[y].before_triangle ? d->spheres[x].before_triangle < d->spheres[y].before_triangle
                                                                                 : d->spheres[x].order < d->spheres[y].order;
        });
        for (uint32_t j = 0; j < d->n_spheres; j++) {
            const uint32_t i = s_order[j];
            s_prim[j] = d->spheres[i].before_triangle + j;          // the triangles before it and the j spheres listed before it
            std::memcpy(&s_bounds[6 * (size_t)j], sprims[i].lo, 12); std::memcpy(&s_bounds[6 * (size_t)j + 3], sprims[i].hi, 12);
            s_rec[4 * (size_t)j] = i; s_rec[4 * (size_t)j + 1] = sprims[i].flags; s_rec[4 * (size_t)j + 2] = (uint32_t)d->spheres[i].material; s_rec[4 * (size_t)j + 3] = 0;
        }
    }
    ptbvh::SceneIn in{d->P, d->n_vertices, d->indices, d->tri_mesh, d->n_triangles, m_triflags.data(), m_material.data(), m_flags.data(), d->n_meshes};
    in.sph_prim = s_prim.data(); in.sph_bounds = s_bounds.data(); in.sph_rec = s_rec.data(); in.n_spheres = d->n_spheres;
    ptbvh::SceneOut out;
    hipError_t herr = hipSuccess;
    const int rc = sah ? ptbvh::device_sah_scene(ctx->stream, in, (uint32_t)mnp, &out, &herr) : ptbvh::device_hlbvh_scene(ctx->stream, in, (uint32_t)mnp, &out, &herr);
    if (rc == -2) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "hlbvh: all treelet centroids coincide along the split axis (the reference panics on this input)");
    if (rc < 0) return ctx->hip_fail(herr, "scene build on the device");
    mark(trace, "device scene (bounds, SAH, records, collapse)");
    if (rc != 0) return PT_OK;                // this list needs the host path
    // light i = the i-th emissive primitive in primitive order (scene_context.rs:1218-1231); `lit` holds primitive numbers of the merged list,
    // `lit_src` what each stands for (bit 31: a sphere, else the triangle)
    std::vector<uint32_t> lit, lit_src;
    bool any_light_mesh = false;
    for (uint32_t i = 0; i < d->n_meshes; i++) any_light_mesh |= d->meshes[i].area_light >= 0;
    if (any_light_mesh) {                     // the host's threads scan their share of the triangles; the shares are joined in order
        const size_t n_chunks = 64, step = ((size_t)d->n_triangles + n_chunks - 1) / n_chunks;
        std::vector<std::vector<uint32_t>> part(n_chunks);
        ptbvh::parallel_tasks(n_chunks, [&](size_t c) {
            const size_t a = c * step, b = std::min((size_t)d->n_triangles, a + step);
            for (size_t t = a; t < b; t++) if (d->meshes[d->tri_mesh[t]].area_light >= 0) part[c].push_back((uint32_t)t);
        });
        for (const auto& v : part) lit_src.insert(lit_src.end(), v.begin(), v.end());
    }
    if (d->n_spheres) {                       // triangle numbers -> primitive numbers, the emissive spheres merged in at their places
        std::vector<uint32_t> tri_lit;
        tri_lit.swap(lit_src);
        size_t ti = 0;
        uint32_t j = 0;                       // spheres listed so far
        auto flush_tris = [&](uint32_t before) {          // emissive triangles t < before: primitive t + j
            while (ti < tri_lit.size() && tri_lit[ti] < before) { lit.push_back(tri_lit[ti] + j); lit_src.push_back(tri_lit[ti]); ti++; }
        };
        for (; j < d->n_spheres; j++) {
            const uint32_t i = s_order[j];
            flush_tris(d->spheres[i].before_triangle);
            if (d->spheres[i].area_light >= 0) { lit.push_back(s_prim[j]); lit_src.push_back(0x80000000u | i); }
        }
        flush_tris(0xffffffffu);
    } else {
        lit = lit_src;
    }
    if (lit.size() >= (1u << 24)) { out.free_all(); return ctx->fail(PT_ERR_UNSUPPORTED, "more than 2^24 emissive primitives"); }
    std::vector<uint32_t> lit_rec(lit.size());
    if (ptbvh::device_scene_lights(ctx->stream, &out, lit.data(), (uint32_t)lit.size(), lit_rec.data(), &herr) < 0) { out.free_all(); return ctx->hip_fail(herr, "light records on the device"); }
    for (size_t i = 0; i < lit.size(); i++) {
        const uint32_t src = lit_src[i], si = src & 0x7fffffffu;
        w.lights.push_back((src & 0x80000000u) ? sphere_light(d, si, w.sph[si].area, lit_rec[i], lit[i]) : triangle_light(d, src, m_flags[d->tri_mesh[src]], lit_rec[i], lit[i]));
    }
    (void)hipFree(out.d_rec_of_prim);
    out.d_rec_of_prim = nullptr;
    // the context's buffers take the blocks over
    ctx->d_nodes.release(); ctx->d_tris.release(); ctx->d_tri_info.release();
    ctx->d_nodes.p = out.d_nodes; ctx->d_nodes.bytes = (size_t)out.n_nodes4 * sizeof(PtNode);
    ctx->d_tris.p = out.d_tris; ctx->d_tris.bytes = ((size_t)n_world + 1) * sizeof(PtTri);
    ctx->d_tri_info.p = out.d_tinfo; ctx->d_tri_info.bytes = (size_t)n_world * sizeof(PtTriInfo);
    w.up_n_nodes = out.n_nodes4; w.up_n_tris = (size_t)n_world + 1;
    w.n_world_nodes = out.n_nodes4; w.n_top = out.n_top;
    w.up_root_ref = 0; w.up_max_leaf = out.max_leaf; w.up_n_leaves = out.n_leaves;
    std::memcpy(w.up_root_lo, out.root_lo, 12); std::memcpy(w.up_root_hi, out.root_hi, 12);
    w.any_one_sided = out.any_one_sided != 0;
    ctx->max_stack = 3u * out.max_depth4 + 2u;
    w.dev_build.used = true;
    *took = true;
    w.t1 = now_ms();
    mark(trace, "lights + hand-over");
    return PT_OK;
}

// ---- BVH (host) ---------------------------------------------------------
// Primitive lists (render_options.primitives and each object's list, scene_context.rs:1301-1316): triangles in array order with
// the spheres / instances of the list spliced in before triangle `before_triangle`, ties in creation order.  tag 0 is the world, k + 1 object k.
std::vector<Entry> make_list(const pt_scene_desc* d, uint32_t tag, uint32_t n_objects) {
    struct Extra { uint32_t before, order, kind, idx; };
    std::vector<Extra> extra;
    for (uint32_t i = 0; i < d->n_spheres; i++) if (d->spheres[i].object == tag) extra.push_back({d->spheres[i].before_triangle, d->spheres[i].order, 1u, i});
    if (tag == 0) for (uint32_t i = 0; i < d->n_instances; i++) extra.push_back({d->instances[i].before_triangle, d->instances[i].order, 2u, i});
    std::stable_sort(extra.begin(), extra.end(), [](const Extra& x, const Extra& y) { return x.before != y.before ? x.before < y.before : x.order < y.order; });
    std::vector<Entry> out;
    if (extra.empty() && n_objects == 0) {            // triangles only, all in the world: the list is the triangle array
        out.resize(d->n_triangles);
        ptbvh::parallel_for(d->n_triangles, [&](size_t a, size_t b) { for (size_t t = a; t < b; t++) out[t] = {0u, (uint32_t)t}; });
        return out;
    }
    if (extra.empty()) {              // triangles only: the list's members counted and written by the host's threads, chunk by chunk, in triangle order
        const size_t n_chunks = 64, step = ((size_t)d->n_triangles + n_chunks - 1) / n_chunks;
        std::vector<size_t> cnt_c(n_chunks + 1, 0);
        ptbvh::parallel_tasks(n_chunks, [&](size_t c) {
            const size_t a = std::min((size_t)d->n_triangles, c * step), b = std::min((size_t)d->n_triangles, a + step);
            size_t k = 0;
            for (size_t t = a; t < b; t++) k += d->meshes[d->tri_mesh[t]].object == tag;
            cnt_c[c + 1] = k;
        });
        for (size_t c = 0; c < n_chunks; c++) cnt_c[c + 1] += cnt_c[c];
        out.resize(cnt_c[n_chunks]);
        ptbvh::parallel_tasks(n_chunks, [&](size_t c) {
            const size_t a = std::min((size_t)d->n_triangles, c * step), b = std::min((size_t)d->n_triangles, a + step);
            size_t k = cnt_c[c];
            for (size_t t = a; t < b; t++) if (d->meshes[d->tri_mesh[t]].object == tag) out[k++] = {0u, (uint32_t)t};
        });
        return out;
    }
    size_t e = 0;
    for (uint32_t t = 0; t <= d->n_triangles; t++) {
        while (e < extra.size() && extra[e].before <= t) { out.push_back({extra[e].kind, extra[e].idx}); e++; }
        if (t < d->n_triangles && d->meshes[d->tri_mesh[t]].object == tag) out.push_back({0u, t});
    }
    return out;
}

// The world's list and tree (ctx->host_bvh) with every object's tree merged in behind it; rec_entry: leaf record -> what it stands for
pt_status build_lists_and_trees(pt_context* ctx, const pt_scene_desc* d, const SceneChecks& chk, WorldBuild& w, double* trace, std::vector<Entry>& world, std::vector<Entry>& rec_entry) {
    ptbvh::Result& bvh = ctx->host_bvh;
    w.tri_flags.resize(d->n_triangles);
    ptbvh::parallel_for(d->n_triangles, [&](size_t t0_, size_t t1_) {
        for (size_t t = t0_; t < t1_; t++) w.tri_flags[t] = mesh_tri_flags(d, d->tri_mesh[t], chk.mesh_alpha);
    });
    mark(trace, "triangle flags");
    std::vector<ptbvh::SpherePrim> sprims;
    build_spheres(d, w.sph, sprims);
    uint32_t n_objects = 0;
    for (uint32_t i = 0; i < d->n_meshes; i++) n_objects = std::max(n_objects, d->meshes[i].object);
    for (uint32_t i = 0; i < d->n_spheres; i++) n_objects = std::max(n_objects, d->spheres[i].object);
    const char* hlbvh_msg = "hlbvh: all treelet centroids coincide along the split axis (the reference panics on this input)";
    // objects first: an instance's bound is its object's root bound under the instance transform
    struct ObjectBvh { std::vector<Entry> list; ptbvh::Result res; float lo[3], hi[3]; bool direct = false; };
    std::vector<ObjectBvh> objs(n_objects);
    auto fill_prim = [&](const Entry& en, ptbvh::Prim* pr) {
        if (en.kind == 0) ptbvh::triangle_prim(d->P, d->indices, en.idx, w.tri_flags[en.idx], pr);
        else {
            std::memcpy(pr->lo, sprims[en.idx].lo, 12); std::memcpy(pr->hi, sprims[en.idx].hi, 12);
            ptbvh::sphere_record(en.idx, sprims[en.idx].flags, &pr->rec);
        }
    };
    for (uint32_t k = 0; k < n_objects; k++) {
        ObjectBvh& ob = objs[k];
        ob.list = make_list(d, k + 1, n_objects);
        // (the context's primitive buffer, shared with the world list below: uninitialised storage that survives from upload to upload)
        if (ctx->host_prims_cap < ob.list.size()) {
            ctx->host_prims.reset();
            ctx->host_prims.reset(new ptbvh::Prim[ob.list.size()]);
            ctx->host_prims_cap = ob.list.size();
        }
        struct { ptbvh::Prim* p; size_t n; ptbvh::Prim* data() const { return p; } size_t size() const { return n; } bool empty() const { return n == 0; }
                 ptbvh::Prim& operator[](size_t i) const { return p[i]; } } prims{ctx->host_prims.get(), ob.list.size()};
        ptbvh::parallel_for(ob.list.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) fill_prim(ob.list[i], &prims[i]); });
        if (prims.size() == 1) {             // a single primitive is wrapped without an accelerator (scene_context.rs:1370-1377)
            ob.direct = true;
            ob.res.tris.assign(1, prims[0].rec);
            ob.res.tris[0].prim = 0; ob.res.tris[0].flags |= PT_TRI_LAST; ob.res.tris[0].light1 = 0;
            ob.res.max_stack = 0; ob.res.max_leaf = 1;
            std::memcpy(ob.lo, prims[0].lo, 12); std::memcpy(ob.hi, prims[0].hi, 12);
        } else if (!prims.empty()) {
            if (!ptbvh::build_prims(prims.data(), (uint32_t)prims.size(), d->split_method, w.max_node_prims, &ob.res, &w.dev_build))
                return w.dev_build.err != hipSuccess ? ctx->hip_fail(w.dev_build.err, "HLBVH build on the device") : ctx->fail(PT_ERR_INVALID_ARGUMENT, hlbvh_msg);
            ob.res.tris.pop_back();          // the pad record: one for the whole array, below
            std::memcpy(ob.lo, ob.res.root_lo, 12); std::memcpy(ob.hi, ob.res.root_hi, 12);
        }
    }
    for (uint32_t i = 0; i < d->n_instances; i++)
        if (d->instances[i].object >= n_objects || objs[d->instances[i].object].list.empty()) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "instance of an unknown or empty object");
    w.dinst.resize(d->n_instances);
    mark(trace, "object trees");
    world = make_list(d, 0, n_objects);
    mark(trace, "world primitive list");
    if (world.empty()) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "scene has no world primitives (objects are only rendered through ObjectInstance)");
    if ((uint64_t)world.size() >= PT_LEAF_FIRST_MASK - 16u) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "more than 2^26 primitives");
    {
        // the world's primitive list: uninitialised storage, first touched by the threads that fill it, kept by the context for the next
        // upload (allocating and returning 72 MB per million triangles costs more than the device-side build)
        if (ctx->host_prims_cap < world.size()) {
            ctx->host_prims.reset();
            ctx->host_prims.reset(new ptbvh::Prim[world.size()]);
            ctx->host_prims_cap = world.size();
        }
        struct PrimsView { ptbvh::Prim* p; size_t n; ptbvh::Prim* data() const { return p; } size_t size() const { return n; } ptbvh::Prim& operator[](size_t i) const { return p[i]; } };
        PrimsView prims{ctx->host_prims.get(), world.size()};
        ptbvh::parallel_for(world.size(), [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) if (world[i].kind != 2) fill_prim(world[i], &prims[i]);
        });
        for (size_t i = 0; d->n_instances && i < world.size(); i++) {
            const Entry& en = world[i];
            if (en.kind != 2) continue;
            const pt_instance& in = d->instances[en.idx];
            const ObjectBvh& ob = objs[in.object];
            const float* m = in.instance_to_world;          // motion_bounds of a static transform = transform_bounds (transform.rs:134-182)
            if (w.inst_motion[en.idx]) {                    // ... and of one that moves the sampled form (animated_transform.rs:154-187), whatever the split method
                const pt_motion_instance& mi = ctx->next_motion_inst[w.inst_motion_rec[en.idx]];
                ptmotion::motion_bounds(w.motion[w.inst_motion[en.idx]], w.inst_has_rotation[en.idx] != 0, m, mi.instance_to_world_end, ob.lo, ob.hi, prims[i].lo, prims[i].hi);
                ptbvh::instance_record(en.idx, &prims[i].rec);
                continue;
            }
            for (int c = 0; c < 8; c++) {
                const float x = (c & 4) ? ob.hi[0] : ob.lo[0], y = (c & 2) ? ob.hi[1] : ob.lo[1], z = (c & 1) ? ob.hi[2] : ob.lo[2];
                float q[3] = {m[0] * x + m[1] * y + m[2] * z + m[3], m[4] * x + m[5] * y + m[6] * z + m[7], m[8] * x + m[9] * y + m[10] * z + m[11]};
                const float wq = m[12] * x + m[13] * y + m[14] * z + m[15];
                if (wq != 1.0f) { q[0] /= wq; q[1] /= wq; q[2] /= wq; }
                for (int a2 = 0; a2 < 3; a2++) {
                    prims[i].lo[a2] = c == 0 ? q[a2] : std::fmin(prims[i].lo[a2], q[a2]);
                    prims[i].hi[a2] = c == 0 ? q[a2] : std::fmax(prims[i].hi[a2], q[a2]);
                }
            }
            ptbvh::instance_record(en.idx, &prims[i].rec);
        }
        mark(trace, "world primitives (bounds + records)");
        if (!ptbvh::build_prims(prims.data(), (uint32_t)prims.size(), d->split_method, w.max_node_prims, &bvh, &w.dev_build))
            return w.dev_build.err != hipSuccess ? ctx->hip_fail(w.dev_build.err, "HLBVH build on the device") : ctx->fail(PT_ERR_INVALID_ARGUMENT, hlbvh_msg);
        mark(trace, "build_prims");
    }
    if (ctx->host_prims_cap > ((size_t)4 << 20)) { ctx->host_prims.reset(); ctx->host_prims_cap = 0; }
    mark(trace, "free primitive list");
    w.n_world_nodes = bvh.nodes.size();          // the objects' trees are appended behind these
    if (d->n_instances) for (size_t prim = 0; prim < world.size(); prim++) if (world[prim].kind == 2) w.dinst[world[prim].idx].world_prim = (uint32_t)prim;
    // one node array and one record array: the world first, then each object with its references shifted
    rec_entry.resize(bvh.tris.size() - 1);        // record -> what it stands for (build_shading_records)
    ptbvh::parallel_for(world.size(), [&](size_t a, size_t b) { for (size_t prim = a; prim < b; prim++) rec_entry[bvh.rec_of_prim[prim]] = world[prim]; });
    uint32_t max_inner_stack = 0;
    if (n_objects) {
        bvh.tris.pop_back();
        std::vector<uint32_t> node_off(n_objects), rec_off(n_objects);
        for (uint32_t k = 0; k < n_objects; k++) {
            ObjectBvh& ob = objs[k];
            node_off[k] = (uint32_t)bvh.nodes.size(); rec_off[k] = (uint32_t)bvh.tris.size();
            if ((uint64_t)rec_off[k] + ob.res.tris.size() >= PT_LEAF_FIRST_MASK - 16u) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "more than 2^26 primitives");
            auto shift = [&](uint32_t ref) {
                if (ref == PT_EMPTY_REF) return ref;
                return (ref & PT_LEAF_BIT) ? ((ref & ~PT_LEAF_FIRST_MASK) | ((ref & PT_LEAF_FIRST_MASK) + rec_off[k])) : ref + node_off[k];
            };
            bvh.nodes.resize((size_t)node_off[k] + ob.res.nodes.size());
            ptbvh::parallel_for(ob.res.nodes.size(), [&](size_t a, size_t b) {
                for (size_t i = a; i < b; i++) { PtNode nd = ob.res.nodes[i]; for (int c = 0; c < 4; c++) nd.child[c] = shift(nd.child[c]); bvh.nodes[(size_t)node_off[k] + i] = nd; }
            });
            bvh.tris.resize((size_t)rec_off[k] + ob.res.tris.size());
            rec_entry.resize((size_t)rec_off[k] + ob.res.tris.size());
            ptbvh::parallel_for(ob.res.tris.size(), [&](size_t a, size_t b) {
                for (size_t r = a; r < b; r++) {
                    bvh.tris[(size_t)rec_off[k] + r] = ob.res.tris[r];
                    rec_entry[(size_t)rec_off[k] + r] = ob.direct ? ob.list[0] : ob.list[ob.res.tris[r].prim];
                }
            });
            ob.res.root_ref = ob.direct ? rec_off[k] : shift(ob.res.root_ref);
            max_inner_stack = std::max(max_inner_stack, ob.res.max_stack);
            bvh.max_leaf = std::max(bvh.max_leaf, ob.res.max_leaf);
        }
        PtTri pad;
        std::memset(&pad, 0, sizeof(pad));
        pad.flags = PT_TRI_LAST;
        bvh.tris.push_back(pad);
        for (uint32_t i = 0; i < d->n_instances; i++) {
            const pt_instance& in = d->instances[i];
            const ObjectBvh& ob = objs[in.object];
            PtInstance& o = w.dinst[i];
            const uint32_t wp = o.world_prim;
            std::memset(&o, 0, sizeof(o));
            o.world_prim = wp;
            std::memcpy(o.m, in.instance_to_world, 48); std::memcpy(o.minv, in.world_to_instance, 48);
            o.root_ref = ob.res.root_ref; o.direct = ob.direct ? 1u : 0u;
            o.motion1 = w.inst_motion[i];
            std::memcpy(o.root_lo, ob.lo, 12); std::memcpy(o.root_hi, ob.hi, 12);
        }
    }
    mark(trace, "record map + objects");
    w.t1 = now_ms();
    ctx->max_stack = bvh.max_stack + max_inner_stack + (d->n_instances ? 4u : 0u);      // (+ what a ray leaves behind when it enters an object: the rest of its leaf, its slab interval, the marker)
    return PT_OK;
}

// ---- shading records ----------------------------------------------------
pt_status build_shading_records(pt_context* ctx, const pt_scene_desc* d, WorldBuild& w, const std::vector<Entry>& world, const std::vector<Entry>& rec_entry) {
    ptbvh::Result& bvh = ctx->host_bvh;
    w.tinfo.resize(bvh.tris.size() - 1);
    ptbvh::parallel_for(w.tinfo.size(), [&](size_t r0_, size_t r1_) {
        for (size_t r = r0_; r < r1_; r++) {
            PtTriInfo& ti = w.tinfo[r];
            std::memset(&ti, 0, sizeof(ti));
            ti.light = -1; ti.material = -1;
            const Entry& en = rec_entry[r];
            if (en.kind == 1) ti.material = d->spheres[en.idx].material;
            if (en.kind != 0) continue;
            const uint32_t t = en.idx;
            const pt_mesh& m = d->meshes[d->tri_mesh[t]];
            ti.v[0] = d->indices[3 * (size_t)t]; ti.v[1] = d->indices[3 * (size_t)t + 1]; ti.v[2] = d->indices[3 * (size_t)t + 2];
            ti.mesh = d->tri_mesh[t];
            ti.material = m.material;
            ti.mesh_flags = mesh_attr_flags(d, ti.mesh);
        }
    });
    // one DiffuseAreaLight per emissive world primitive, in primitive order (scene_context.rs:1218-1231); lights inside objects are
    // dropped as in the reference (:1302-1304), instances carry none (TransformedPrimitive::get_area_light)
    for (uint32_t prim = 0; prim < world.size(); prim++) {
        const Entry& en = world[prim];
        const uint32_t rec = bvh.rec_of_prim[prim];
        if (en.kind == 1 && d->spheres[en.idx].area_light >= 0) w.lights.push_back(sphere_light(d, en.idx, w.sph[en.idx].area, rec, prim));
        else if (en.kind == 0 && d->meshes[d->tri_mesh[en.idx]].area_light >= 0) w.lights.push_back(triangle_light(d, en.idx, w.tinfo[rec].mesh_flags, rec, prim));
        else continue;
        w.tinfo[rec].light = (int32_t)w.lights.size() - 1;
        bvh.tris[rec].light1 = (uint32_t)w.lights.size();
    }
    if (w.lights.size() >= (1u << 24)) return ctx->fail(PT_ERR_UNSUPPORTED, "more than 2^24 emissive primitives");
    for (uint32_t f : w.tri_flags) if (f & PT_TRI_ONE_SIDED) { w.any_one_sided = true; break; }
    return PT_OK;
}

// What the lean node visit (pt_kernels.hip node_step_lean) reads beside the builder's output: the per-octant order tables, and
// empty child slots as inverted boxes so that they fail the slab test by themselves (the builders leave them all-zero, as the
// reference does; the general visit masks them out by the occupied-slot bits either way).
pt_status finish_and_upload_nodes(pt_context* ctx, WorldBuild& w) {
    ptbvh::Result& bvh = ctx->host_bvh;
    pt_status st;
    if (bvh.nodes.size() >= (1u << 25)) return ctx->fail(PT_ERR_UNSUPPORTED, "more than 2^25 BVH nodes (32-bit node offsets)");
    // The builders emit nodes depth-first.  The top of the WORLD tree is renumbered breadth-first (the first PT_TOP_BFS_NODES nodes in
    // level order, everything else behind them in the old order), so that "node index < n" means "one of the top levels": k_trace keeps
    // those in LDS (PT_TOP_NODES).  Traversal order, boxes and references are untouched -- only where a node lives.
    if (w.n_world_nodes > 0 && !(bvh.root_ref & PT_LEAF_BIT) && bvh.root_ref != PT_EMPTY_REF) {
        std::vector<uint32_t> bfs;
        bfs.reserve(PT_TOP_BFS_NODES);
        bfs.push_back(bvh.root_ref & PT_REF_INDEX_MASK);
        for (size_t head = 0; head < bfs.size() && bfs.size() < PT_TOP_BFS_NODES; head++)
            for (int ch = 0; ch < 4 && bfs.size() < PT_TOP_BFS_NODES; ch++) {
                const uint32_t r = bvh.nodes[bfs[head]].child[ch];
                if (r != PT_EMPTY_REF && !(r & PT_LEAF_BIT)) bfs.push_back(r & PT_REF_INDEX_MASK);
            }
        w.n_top = (uint32_t)bfs.size();
        std::vector<uint32_t> new_of(w.n_world_nodes, 0xffffffffu);
        for (uint32_t k = 0; k < w.n_top; k++) new_of[bfs[k]] = k;
        uint32_t next = w.n_top;
        for (size_t n = 0; n < w.n_world_nodes; n++) if (new_of[n] == 0xffffffffu) new_of[n] = next++;
        std::vector<PtNode> moved(w.n_world_nodes);
        ptbvh::parallel_for(w.n_world_nodes, [&](size_t n0, size_t n1) {
            for (size_t n = n0; n < n1; n++) {
                PtNode nd = bvh.nodes[n];
                for (int ch = 0; ch < 4; ch++)
                    if (nd.child[ch] != PT_EMPTY_REF && !(nd.child[ch] & PT_LEAF_BIT)) nd.child[ch] = (nd.child[ch] & ~PT_REF_INDEX_MASK) | new_of[nd.child[ch] & PT_REF_INDEX_MASK];
                moved[new_of[n]] = nd;
            }
        });
        std::copy(moved.begin(), moved.end(), bvh.nodes.begin());
        bvh.root_ref = (bvh.root_ref & ~PT_REF_INDEX_MASK) | new_of[bvh.root_ref & PT_REF_INDEX_MASK];
    }
    ptbvh::parallel_for(bvh.nodes.size(), [&](size_t n0, size_t n1) {
        for (size_t n = n0; n < n1; n++) {
            PtNode& nd = bvh.nodes[n];
            uint32_t lut = 0;
            for (uint32_t oct = 0; oct < 8; oct++)
                for (uint32_t k = 0; k < 3; k++)
                    if ((oct >> ((nd.axes >> (2 * k)) & 3u)) & 1u) lut |= 1u << (8 * k + oct);
            nd.order_lut = lut;
            // -0.0 and +0.0 bounds: the host builders keep whichever came first, the device builders order them; one spelling for both
            for (int a = 0; a < 3; a++)
                for (int ch = 0; ch < 4; ch++) { if (nd.bmin[a][ch] == 0.0f) nd.bmin[a][ch] = 0.0f; if (nd.bmax[a][ch] == 0.0f) nd.bmax[a][ch] = 0.0f; }
            const uint32_t ax_of[4] = {nd.axes & 3u, (nd.axes >> 2) & 3u, 0u, (nd.axes >> 4) & 3u};     // child 0: axis_top, 1: axis_left, 3: axis_right
            for (int ch = 0; ch < 4; ch++)
                if (nd.child[ch] != PT_EMPTY_REF) nd.child[ch] = (nd.child[ch] & ~(3u << PT_REF_AXIS_SHIFT)) | (ax_of[ch] << PT_REF_AXIS_SHIFT);
            for (int ch = 0; ch < 4; ch++)
                if (!((nd.axes >> (8 + ch)) & 1u))
                    for (int a = 0; a < 3; a++) { nd.bmin[a][ch] = INFINITY; nd.bmax[a][ch] = -INFINITY; }
        }
    });
    if ((st = upload(ctx, ctx->d_nodes, bvh.nodes.data(), bvh.nodes.size())) != PT_OK) return st;
    if ((st = upload(ctx, ctx->d_tris, bvh.tris.data(), bvh.tris.size())) != PT_OK) return st;
    if ((st = upload(ctx, ctx->d_tri_info, w.tinfo.data(), w.tinfo.size())) != PT_OK) return st;
    w.up_n_nodes = bvh.nodes.size(); w.up_n_tris = bvh.tris.size();
    w.up_root_ref = bvh.root_ref; w.up_max_leaf = bvh.max_leaf; w.up_n_leaves = bvh.n_leaves;
    std::memcpy(w.up_root_lo, bvh.root_lo, 12); std::memcpy(w.up_root_hi, bvh.root_hi, 12);
    return PT_OK;
}

// ---- materials
// Appends the evaluation program of texture `root` to tex_prog and returns its offset: post-order over the nodes the root needs; 0 on overflow
uint32_t add_program(const pt_scene_desc* d, std::vector<uint32_t>& tex_prog, uint32_t root) {
    std::vector<uint32_t> order;
    std::vector<int32_t> pos(d->n_textures, -1);
    std::vector<std::pair<uint32_t, int>> stack{{root, 0}};
    while (!stack.empty()) {
        auto& top = stack.back();
        const pt_texture& t = d->textures[top.first];
        const int n_children = t.type == PT_TEX_MIX ? 3 : ((t.type == PT_TEX_SCALE || t.type == PT_TEX_CHECKERBOARD_2D || t.type == PT_TEX_CHECKERBOARD_3D || t.type == PT_TEX_DOTS) ? 2 : 0);
        if (top.second < n_children) {
            int32_t c = t.tex[top.second++];
            if (c >= 0 && pos[c] < 0) stack.push_back({(uint32_t)c, 0});
            continue;
        }
        if (pos[top.first] < 0) { pos[top.first] = (int32_t)order.size(); order.push_back(top.first); }
        stack.pop_back();
    }
    if (order.size() > PT_TEX_PROG_MAX || d->n_textures > 0xffffu) return 0u;
    const uint32_t off = (uint32_t)tex_prog.size();
    tex_prog.push_back((uint32_t)order.size());
    for (uint32_t node : order) {
        const pt_texture& t = d->textures[node];
        uint32_t e = node;
        for (int k = 0; k < 3; k++) e |= (t.tex[k] >= 0 ? (uint32_t)pos[t.tex[k]] : PT_TEX_CHILD_CONST) << (16 + 4 * k);
        tex_prog.push_back(e);
    }
    return off;
}

// Material "disney": its parameter block rides in the lobe slots of its PtMaterial record (PtDisneyParams), its up to eight lobes in a
// PtMix record of one leaf with no scale chain -- built here when every parameter is constant (and left in `lobes` for a mix above it), at every
// hit otherwise (disney_hit_lobes, pt_kernels.hip).  `rec` is the material's pt_disney record, null without one.
pt_status build_disney_material(pt_context* ctx, const pt_scene_desc* d, uint32_t i, const pt_disney* rec, MaterialTables& mt, std::vector<PtLobe>& lobes, uint32_t& n_general_bins) {
    const pt_material& in = d->materials[i];
    PtMaterial& mm = mt.mats[i];
    PtDisneyParams dp;
    std::memset(&dp, 0, sizeof(dp));
    std::memcpy(dp.color, in.kd, 12);
    const float defaults[10] = {0.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f};          // create_disney_material (disney.rs:806-841), by PT_DISNEY_*
    const int slot[10] = {PT_DP_METALLIC, PT_DP_SPECULARTINT, PT_DP_ANISOTROPIC, PT_DP_SHEEN, PT_DP_SHEENTINT, PT_DP_CLEARCOAT, PT_DP_CLEARCOATGLOSS,
                          PT_DP_SPECTRANS, PT_DP_FLATNESS, PT_DP_DIFFTRANS};
    uint32_t tex[PT_DP_COUNT] = {};
    for (int k = 0; k < 10; k++) {
        dp.f[slot[k]] = rec ? rec->value[k] : defaults[k];
        tex[slot[k]] = rec ? rec->tex[k] : 0u;
    }
    dp.f[PT_DP_ETA] = in.eta; tex[PT_DP_ETA] = in.tex_eta;
    dp.f[PT_DP_ROUGHNESS] = in.roughness; tex[PT_DP_ROUGHNESS] = in.tex_roughness;
    dp.thin = rec && rec->thin ? 1u : 0u;
    bool per_hit = false, too_big = false;
    auto program = [&](uint32_t t) -> uint32_t {
        if (!t) return 0u;
        per_hit = true;
        const uint32_t off = add_program(d, mt.tex_prog, t - 1);
        too_big |= off == 0;
        return off;
    };
    dp.prog_color = program(in.tex_kd);
    for (int k = 0; k < PT_DP_COUNT; k++) dp.prog[k] = program(tex[k]);
    dp.prog_bump = program(in.tex_bump);
    if (too_big) return ctx->fail(PT_ERR_UNSUPPORTED, "a material parameter's texture graph needs more than 12 nodes");
    PtMix mx;
    std::memset(&mx, 0, sizeof(mx));
    mx.n_leaves = 1;
    mx.leaf_material[0] = (int32_t)i;
    if (!per_hit) {
        mx.n_lobes = build_disney_lobes(dp, mx.lobes);
        count_lobes(mx.lobes, mx.n_lobes, mm);
        lobes.assign(mx.lobes, mx.lobes + mx.n_lobes);
    } else {
        mx.per_hit = 1;
        mm.textured = 1;
        mt.any_textured = true;
        ctx->per_hit_lobes[i] = pt_context::PER_HIT_DISNEY;
        mt.mparams[i].m = in;
        mt.mparams[i].prog[8] = dp.prog_bump;          // where the aov kernel looks for a bump map
    }
    mm.n_lobes = 0; mm.has_bsdf = 1; mm.bsdf_eta = 1.0f;            // the BSDF is allocated with eta 1 (disney.rs:658)
    static_assert(sizeof(dp) <= sizeof(mm.lobes), "PtDisneyParams in PtMaterial::lobes");
    std::memcpy(mm.lobes, &dp, sizeof(dp));
    mt.mixes.push_back(mx);
    mm.mix1 = (uint32_t)mt.mixes.size();
    mt.general_materials = true;
    ctx->disney_kernels = true;
    mm.sort_bin = PT_SORT_GENERAL0 + std::min(n_general_bins++, PT_SORT_TEX0 - PT_SORT_GENERAL0 - 1u);
    return PT_OK;
}

// Material "fourier": the tables of this upload in one device buffer -- the PtFourierTable records first, then each table's arrays as
// FourierBSDFTable::read_body leaves them (a0 and recip computed here, fourier.rs:130-146) -- and per table the device address of its record.
pt_status upload_fourier_tables(pt_context* ctx, std::vector<uint64_t>& table_addr) {
    const size_t n = ctx->fourier_tables.size();
    table_addr.assign(n, 0);
    ctx->n_fourier_tables = 0;
    if (n == 0) { ctx->d_fourier.release(); return PT_OK; }
    auto pad = [](size_t b) { return (b + 15u) & ~(size_t)15u; };
    size_t total = pad(n * sizeof(PtFourierTable));
    struct Layout { size_t mu, cdf, a0, a, recip, m, off; };
    std::vector<Layout> lay(n);
    for (size_t t = 0; t < n; t++) {
        const pt_context::FourierTable& ft = ctx->fourier_tables[t];
        const size_t n2 = (size_t)ft.n_mu * ft.n_mu, nr = (size_t)std::max(ft.m_max, 1), na = (size_t)std::max(ft.n_coeffs, 1);
        Layout& l = lay[t];
        l.mu = total; total += pad(4 * (size_t)ft.n_mu);
        l.cdf = total; total += pad(4 * n2);
        l.a0 = total; total += pad(4 * n2);
        l.a = total; total += pad(4 * na);
        l.recip = total; total += pad(4 * nr);
        l.m = total; total += pad(4 * n2);
        l.off = total; total += pad(4 * n2);
    }
    PT_HIP(ctx->d_fourier.alloc(total));
    std::vector<unsigned char> buf(total, 0);
    unsigned char* base = ctx->d_fourier.as<unsigned char>();
    for (size_t t = 0; t < n; t++) {
        const pt_context::FourierTable& ft = ctx->fourier_tables[t];
        const size_t n2 = (size_t)ft.n_mu * ft.n_mu;
        const Layout& l = lay[t];
        std::memcpy(buf.data() + l.mu, ft.mu.data(), 4 * ft.mu.size());
        std::memcpy(buf.data() + l.cdf, ft.cdf.data(), 4 * n2);
        if (!ft.a.empty()) std::memcpy(buf.data() + l.a, ft.a.data(), 4 * ft.a.size());
        float* a0 = reinterpret_cast<float*>(buf.data() + l.a0);
        int32_t* m = reinterpret_cast<int32_t*>(buf.data() + l.m);
        int32_t* off = reinterpret_cast<int32_t*>(buf.data() + l.off);
        for (size_t i = 0; i < n2; i++) {
            off[i] = ft.offset_and_length[2 * i];
            m[i] = ft.offset_and_length[2 * i + 1];
            a0[i] = m[i] > 0 ? ft.a[(size_t)off[i]] : 0.0f;
        }
        float* recip = reinterpret_cast<float*>(buf.data() + l.recip);
        recip[0] = INFINITY;
        for (int32_t k = 1; k < ft.m_max; k++) recip[k] = 1.0f / (float)k;
        PtFourierTable rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.mu = reinterpret_cast<const float*>(base + l.mu);
        rec.cdf = reinterpret_cast<const float*>(base + l.cdf);
        rec.a0 = reinterpret_cast<const float*>(base + l.a0);
        rec.a = reinterpret_cast<const float*>(base + l.a);
        rec.recip = reinterpret_cast<const float*>(base + l.recip);
        rec.m = reinterpret_cast<const int32_t*>(base + l.m);
        rec.a_offset = reinterpret_cast<const int32_t*>(base + l.off);
        rec.n_mu = (uint32_t)ft.n_mu; rec.n_channels = (uint32_t)ft.n_channels; rec.m_max = (uint32_t)ft.m_max;
        rec.eta = ft.eta;
        std::memcpy(buf.data() + t * sizeof(PtFourierTable), &rec, sizeof(rec));
        table_addr[t] = (uint64_t)(uintptr_t)(base + t * sizeof(PtFourierTable));
    }
    PT_HIP(hipMemcpy(ctx->d_fourier.p, buf.data(), total, hipMemcpyHostToDevice));
    ctx->n_fourier_tables = (uint32_t)n;
    return PT_OK;
}

// Fills `mt` (empty on entry), ctx->per_hit_lobes, ctx->disney_kernels and ctx->fourier_kernels
pt_status build_materials(pt_context* ctx, const pt_scene_desc* d, const SceneChecks& chk, MaterialTables& mt) {
    mt.mats.resize(std::max<uint32_t>(d->n_materials, 1));
    std::memset(mt.mats.data(), 0, mt.mats.size() * sizeof(PtMaterial));
    uint32_t n_matte_bins = 0, n_general_bins = 0, n_tex_bins = 0;
    mt.mparams.resize(mt.mats.size());
    std::memset(mt.mparams.data(), 0, mt.mparams.size() * sizeof(PtMatParams));
    mt.tex_prog.assign(1, 0u);          // offset 0 = "constant"
    ctx->per_hit_lobes.assign(mt.mats.size(), 0);
    std::vector<std::vector<PtLobe>> disney_lobes(mt.mats.size());        // per constant Disney material: its list (a mix above it copies from here)
    std::vector<const pt_disney*> disney_of(mt.mats.size(), nullptr);
    for (const pt_disney& r : ctx->disney_recs) disney_of[r.material] = &r;
    ctx->disney_kernels = false;
    ctx->fourier_kernels = false;
    std::vector<uint64_t> fourier_addr;
    std::vector<int32_t> fourier_of(mt.mats.size(), -1);
    for (const pt_fourier& r : ctx->fourier_recs) fourier_of[r.material] = (int32_t)r.table;
    for (uint32_t i = 0; i < d->n_materials; i++) ctx->fourier_kernels |= d->materials[i].type == PT_MATERIAL_FOURIER;
    if (ctx->fourier_kernels) { const pt_status st = upload_fourier_tables(ctx, fourier_addr); if (st != PT_OK) return st; }
    else { ctx->d_fourier.release(); ctx->n_fourier_tables = 0; }
    for (uint32_t i = 0; i < d->n_materials; i++) {
        build_lobes(d->materials[i], mt.mats[i]);
        if (d->materials[i].type == PT_MATERIAL_FOURIER) {
            // Material "fourier" (materials/fourier.rs:23-43): one FourierBSDF, added whenever the table has channels (every table the upload
            // takes has), in a BSDF allocated with eta 1.  build_lobes knows no such type (the kernels of the other builds compile it too, and keep
            // their code); the lobe is written here, its table's device address as bits in t[0] / t[1] (pt_device.h).  Of the material's own
            // fields only "bumpmap" is read, below, like any other material's.
            PtMaterial& mm = mt.mats[i];
            const float zero[3] = {0.0f, 0.0f, 0.0f};
            PtLobe* l = push_lobe(mm, PT_LOBE_FOURIER, kRefl | kTrans | kGlossy, zero);
            const uint64_t addr = fourier_addr[(size_t)fourier_of[i]];
            const uint32_t lo = (uint32_t)addr, hi = (uint32_t)(addr >> 32);
            std::memcpy(&l->t[0], &lo, 4); std::memcpy(&l->t[1], &hi, 4);
            mm.nonspecular = 1; mm.spec_mask = 0; mm.bsdf_eta = 1.0f; mm.has_bsdf = 1;
        }
        if (d->materials[i].type == PT_MATERIAL_DISNEY) {
            const pt_status st = build_disney_material(ctx, d, i, disney_of[i], mt, disney_lobes[i], n_general_bins);
            if (st != PT_OK) return st;
            continue;
        }
        if (d->materials[i].type == PT_MATERIAL_MIX) {
            // Flatten the tree under the mix (children precede it, so their PtMaterial records exist): leaves in lobe order, per leaf the
            // mix nodes above it innermost first.  Constant trees get their lobe list and scales here, once; a tree with a textured
            // "amount" or a textured leaf gets them at every hit (mix_hit_lobes, pt_kernels.hip).
            PtMix mx;
            std::memset(&mx, 0, sizeof(mx));
            uint32_t n_leaves = 0, n_lobes = 0;
            std::string refusal;
            std::vector<std::pair<uint32_t, uint32_t>> above;          // (node, side) from the root down
            std::function<void(uint32_t)> walk = [&](uint32_t mi) {
                const pt_material& in = d->materials[mi];
                if (n_leaves > 4u * PT_MIX_MAX_LEAVES) { n_leaves++; return; }      // far past the cap: refused below; the count in the message stops growing here
                if (in.type == PT_MATERIAL_MIX) {
                    if (above.size() >= 4u * PT_MIX_MAX_NODES) { mx.n_nodes++; n_leaves += 2; return; }      // that deep a tree has more leaves than the cap: no need to go down (bounds the recursion)
                    const uint32_t k = mx.n_nodes++;
                    if (k < PT_MIX_MAX_NODES) {
                        std::memcpy(mx.amount[k], in.kd, 12);
                        if (in.tex_kd) {
                            mx.amount_prog[k] = add_program(d, mt.tex_prog, in.tex_kd - 1);
                            if (!mx.amount_prog[k] && refusal.empty()) refusal = "a material parameter's texture graph needs more than 12 nodes";
                            mx.per_hit = 1;
                        }
                    }
                    above.push_back({k, 0u});
                    walk(in.tex_kr - 1);
                    above.back().second = 1u;
                    walk(in.tex_kt - 1);
                    above.pop_back();
                    return;
                }
                const uint32_t j = n_leaves++;
                if (in.type < PT_MATERIAL_NONE || (in.type > PT_MATERIAL_TRANSLUCENT && in.type != PT_MATERIAL_DISNEY && in.type != PT_MATERIAL_FOURIER)) {
                    if (refusal.empty()) refusal = "child material " + std::to_string(mi) + " has a material type that is not on the accelerated path";
                    return;
                }
                n_lobes += mt.mats[mi].textured ? pt_lobes_most(in.type)          // a texture-driven leaf: the most its type can add
                                             : (in.type == PT_MATERIAL_DISNEY ? (uint32_t)disney_lobes[mi].size() : mt.mats[mi].n_lobes);
                if (in.type == PT_MATERIAL_NONE && refusal.empty())
                    refusal = "child material " + std::to_string(mi) + " is \"none\": it leaves no BSDF to scale (the reference asserts, mix.rs:78-79)";
                else if (!mt.mats[mi].textured && !mt.mats[mi].has_bsdf && refusal.empty())
                    refusal = "child material " + std::to_string(mi) + " never has a BSDF (black Kr and Kt / reflect and transmit): nothing to scale (the reference asserts, mix.rs:78-79)";
                if (j >= PT_MIX_MAX_LEAVES) return;
                if (mt.mats[mi].textured) mx.per_hit = 1;
                mx.leaf_material[j] = (int32_t)mi;
                mx.scales.n_chain[j] = (uint32_t)above.size();
                for (size_t c = 0; c < above.size() && c < PT_MIX_MAX_NODES; c++) {
                    const auto& a = above[above.size() - 1 - c];
                    mx.chain[j][c] = a.first | (a.second << 8);
                }
            };
            walk(i);
            if (!refusal.empty()) return ctx->fail(PT_ERR_UNSUPPORTED, "material " + std::to_string(i) + " (mix): " + refusal);
            if (n_leaves > PT_MIX_MAX_LEAVES || n_lobes > PT_MIX_MAX_LOBES)
                return ctx->fail(PT_ERR_UNSUPPORTED, "material " + std::to_string(i) + " (mix): its tree has " + std::to_string(n_leaves) + " leaves and " + std::to_string(n_lobes) +
                                                     " lobes; the accelerated path takes at most " + std::to_string(PT_MIX_MAX_LEAVES) + " leaves and " +
                                                     std::to_string(PT_MIX_MAX_LOBES) + " lobes per mix tree");
            mx.n_leaves = n_leaves;
            PtMaterial& mm = mt.mats[i];
            mm.n_lobes = 0; mm.has_bsdf = 1;                            // a mix always allocates its BSDF (mix.rs:81-88)
            mm.bsdf_eta = mt.mats[mx.leaf_material[0]].bsdf_eta;           // child 1's, recursively (mix.rs:83)
            if (!mx.per_hit) {
                float ns[PT_MIX_MAX_NODES][2][3];
                for (uint32_t k = 0; k < mx.n_nodes; k++)
                    for (int c = 0; c < 3; c++) {
                        ns[k][0][c] = clamp_zero(mx.amount[k][c]);               // s1 = amount.clamp_zero()
                        ns[k][1][c] = clamp_zero(1.0f - ns[k][0][c]);            // s2 = (1 - s1).clamp_zero()
                    }
                for (uint32_t j = 0; j < mx.n_leaves; j++) {
                    const PtMaterial& lm = mt.mats[mx.leaf_material[j]];
                    const std::vector<PtLobe>& dl = disney_lobes[mx.leaf_material[j]];          // a Disney leaf's list lives beside its record
                    if (lm.type == PT_MATERIAL_DISNEY) for (const PtLobe& l : dl) { mx.scales.lobe_leaf[mx.n_lobes] = j; mx.lobes[mx.n_lobes++] = l; }
                    else
                    for (uint32_t l = 0; l < lm.n_lobes; l++) { mx.scales.lobe_leaf[mx.n_lobes] = j; mx.lobes[mx.n_lobes++] = lm.lobes[l]; }
                    for (uint32_t c = 0; c < mx.scales.n_chain[j]; c++)
                        std::memcpy(mx.scales.s[j][c], ns[mx.chain[j][c] & 0xffu][mx.chain[j][c] >> 8], 12);
                }
                mm.nonspecular = 0; mm.spec_mask = 0;
                for (uint32_t l = 0; l < mx.n_lobes; l++) {
                    if (!(mx.lobes[l].type & kSpecular)) mm.nonspecular++;
                    if ((mx.lobes[l].type & (kRefl | kSpecular)) == mx.lobes[l].type) mm.spec_mask |= 1u;
                    if ((mx.lobes[l].type & (kTrans | kSpecular)) == mx.lobes[l].type) mm.spec_mask |= 2u;
                }
            } else {
                mm.textured = 1;                   // the per-hit route of the *_mix kernels
                mt.any_textured = true;
                ctx->per_hit_lobes[i] = pt_context::PER_HIT_MIX;
                mt.mparams[i].m = d->materials[i];
            }
            mt.mixes.push_back(mx);
            mm.mix1 = (uint32_t)mt.mixes.size();
            mt.general_materials = true;
            mm.sort_bin = PT_SORT_GENERAL0 + std::min(n_general_bins++, PT_SORT_TEX0 - PT_SORT_GENERAL0 - 1u);
            continue;
        }
        {
            const pt_material& in = d->materials[i];
            const uint32_t refs[13] = {in.tex_kd, in.tex_ks, in.tex_kr, in.tex_kt, in.tex_opacity, in.tex_sigma, in.tex_metal_eta, in.tex_metal_k, in.tex_bump,
                                       in.tex_roughness, in.tex_uroughness, in.tex_vroughness, in.tex_eta};
            PtMatParams& mp = mt.mparams[i];
            mp.m = in;
            material_alphas(in, &mp.a_r, &mp.a_u, &mp.a_v);
            for (int k = 0; k < 13; k++) {
                if (!refs[k] || in.type == PT_MATERIAL_NONE || (in.type == PT_MATERIAL_FOURIER && k != 8)) continue;
                mp.prog[k] = add_program(d, mt.tex_prog, refs[k] - 1);
                if (!mp.prog[k]) return ctx->fail(PT_ERR_UNSUPPORTED, "a material parameter's texture graph needs more than 12 nodes");
                mt.mats[i].textured = 1;
                mt.any_textured = true;
            }
        }
        // (with object instances every material rides in the general half: only k_shade_general_inst knows how to bring a hit back)
        const bool general = d->materials[i].type != PT_MATERIAL_NONE && (d->materials[i].type != PT_MATERIAL_MATTE || mt.mats[i].textured || d->n_instances > 0);
        if (general) mt.general_materials = true;
        // shade-queue bin: one per material while they last, the remainder of a class shares its last bin
        // (textured materials get the last 32 bins: their own queue segment and kernel; with object instances everything is
        // shaded by one kernel, which reads the whole general..end range)
        if (general && mt.mats[i].textured && d->n_instances == 0) mt.mats[i].sort_bin = PT_SORT_TEX0 + std::min(n_tex_bins++, PT_SORT_BINS - PT_SORT_TEX0 - 1u);
        else mt.mats[i].sort_bin = general ? PT_SORT_GENERAL0 + std::min(n_general_bins++, PT_SORT_TEX0 - PT_SORT_GENERAL0 - 1u)
                                        : std::min(n_matte_bins++, PT_SORT_GENERAL0 - 1u);
    }
    // alpha masks: the mask textures' programs and the per-mesh table behind them, located by word 0 (PT_ALPHA_CUT, pt_device.h)
    if (chk.any_alpha) {
        std::vector<uint32_t> words(2 * (size_t)d->n_meshes, 0u);
        for (const pt_alpha_mask& am : ctx->alpha_masks) {
            const int32_t kinds[2] = {am.alpha_kind, am.shadow_kind}, texs[2] = {am.alpha_texture, am.shadow_texture};
            const float vals[2] = {am.alpha_value, am.shadow_value};
            for (int k = 0; k < 2; k++) {
                uint32_t w = 0;
                if (kinds[k] == PT_ALPHA_CONSTANT && vals[k] <= 0.0f) w = PT_ALPHA_CUT;
                else if (kinds[k] == PT_ALPHA_TEXTURE) {
                    w = add_program(d, mt.tex_prog, (uint32_t)texs[k]);
                    if (!w) return ctx->fail(PT_ERR_UNSUPPORTED, "an alpha mask's texture graph needs more than 12 nodes");
                }
                words[2 * (size_t)am.mesh + k] = w;
            }
        }
        mt.tex_prog[0] = (uint32_t)mt.tex_prog.size();
        mt.tex_prog.insert(mt.tex_prog.end(), words.begin(), words.end());
    }
    for (const pt_alpha_mask& am : ctx->alpha_masks) mt.any_alpha_tex |= chk.mesh_alpha[am.mesh] && (am.alpha_kind == PT_ALPHA_TEXTURE || am.shadow_kind == PT_ALPHA_TEXTURE);
    return PT_OK;
}

// ---- uploads, the scene record and the lights (the order of allocations matters: render_tiles sizes the path pool from what is left)
pt_status upload_materials_and_lights(pt_context* ctx, const pt_scene_desc* d, MaterialTables& mt, WorldBuild& w) {
    pt_status st;
    if (mt.mixes.empty()) { if ((st = upload(ctx, ctx->d_materials, mt.mats.data(), mt.mats.size())) != PT_OK) return st; }
    else {          // the PtMix records ride behind the PtMaterial records (material_mix, pt_device.h)
        std::vector<unsigned char> both(mt.mats.size() * sizeof(PtMaterial) + mt.mixes.size() * sizeof(PtMix));
        for (PtMaterial& m : mt.mats) m.mix_base = (uint32_t)mt.mats.size();
        std::memcpy(both.data(), mt.mats.data(), mt.mats.size() * sizeof(PtMaterial));
        std::memcpy(both.data() + mt.mats.size() * sizeof(PtMaterial), mt.mixes.data(), mt.mixes.size() * sizeof(PtMix));
        if ((st = upload(ctx, ctx->d_materials, both.data(), both.size())) != PT_OK) return st;
    }
    {   // infinite and delta lights: their records at their places in the light list (scene_context.rs:1178-1188), in directive order
        // (the goniometric / projection lights are delta lights whose PtDeltaLight records follow those of pt_scene_set_delta_lights)
        const uint32_t n_inf = (uint32_t)ctx->inf_lights.size(), n_dl = (uint32_t)ctx->delta_lights.size(), n_all = n_inf + n_dl + (uint32_t)ctx->map_lights.size();
        auto index_of = [&](uint32_t k) {
            return k < n_inf ? ctx->inf_lights[k].light_index : (k < n_inf + n_dl ? ctx->delta_lights[k - n_inf].light_index : ctx->map_lights[k - n_inf - n_dl].light_index);
        };
        std::vector<uint32_t> order(n_all);
        for (uint32_t k = 0; k < n_all; k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return index_of(a) < index_of(b); });
        for (uint32_t k : order) {
            PtLight L;
            std::memset(&L, 0, sizeof(L));
            const uint32_t side = k < n_inf ? k : k - n_inf;          // index of its PtEnvLight / PtDeltaLight record
            std::memcpy(&L.p0[0], &side, 4);
            L.mesh_flags = k < n_inf ? PT_LIGHT_INFINITE : PT_LIGHT_DELTA;
            L.tri_rec = 0xffffffffu;
            L.prim = 0xffffffffu;
            L.n_samples = k < n_inf ? (uint32_t)std::max(1, ctx->inf_lights[k].n_samples) : 1u;        // BaseLight::new(.., 1) for the three delta lights
            const size_t at = std::min<size_t>(index_of(k), w.lights.size());
            w.lights.insert(w.lights.begin() + (ptrdiff_t)at, L);
        }
    }
    ctx->light_samples_total = 0;
    for (const PtLight& L : w.lights) ctx->light_samples_total += L.n_samples;
    if ((st = upload(ctx, ctx->d_lights, w.lights.data(), w.lights.size())) != PT_OK) return st;
    if (d->n_spheres) { if ((st = upload(ctx, ctx->d_spheres, w.sph.data(), w.sph.size())) != PT_OK) return st; } else ctx->d_spheres.release();
    if (!w.motion.empty()) {          // the PtMotion records ride behind the instances (scene_motions)
        std::vector<unsigned char> buf(w.dinst.size() * sizeof(PtInstance) + w.motion.size() * sizeof(PtMotion));
        if (!w.dinst.empty()) std::memcpy(buf.data(), w.dinst.data(), w.dinst.size() * sizeof(PtInstance));
        std::memcpy(buf.data() + w.dinst.size() * sizeof(PtInstance), w.motion.data(), w.motion.size() * sizeof(PtMotion));
        if ((st = upload(ctx, ctx->d_instances, buf.data(), buf.size())) != PT_OK) return st;
    } else
    if (d->n_instances) { if ((st = upload(ctx, ctx->d_instances, w.dinst.data(), w.dinst.size())) != PT_OK) return st; } else ctx->d_instances.release();
    return PT_OK;
}

pt_status upload_images_and_textures(pt_context* ctx, const pt_scene_desc* d, const SceneChecks& chk, const MaterialTables& mt, bool& images_on_device) {
    pt_status st;
    std::vector<PtImage> dimages(d->n_images);
    images_on_device =(mt.any_textured || !ctx->inf_lights.empty() || !ctx->map_lights.empty() || mt.any_alpha_tex) && d->n_images;
    if (images_on_device) {           // all pyramids in one buffer
        size_t total = 0;
        for (uint32_t i = 0; i < d->n_images; i++) {
            const pt_image& im = d->images[i];
            PtImage& o = dimages[i];
            std::memset(&o, 0, sizeof(o));
            o.width = im.width; o.height = im.height; o.channels = im.channels; o.n_levels = im.n_levels;
            uint32_t w = im.width, h = im.height;
            size_t off = 0;
            for (uint32_t l = 0; l < im.n_levels; l++) {
                if (off > 0xffffffffull) return ctx->fail(PT_ERR_UNSUPPORTED, "image pyramid larger than 2^32 floats");
                o.level_off[l] = (uint32_t)off;
                off += (size_t)w * h * im.channels;
                if (w > 1) w /= 2;
                if (h > 1) h /= 2;
            }
            total += off;
        }
        std::vector<float> all(total);
        size_t at = 0;
        std::vector<size_t> base(d->n_images);
        for (uint32_t i = 0; i < d->n_images; i++) {
            size_t n = 0;
            uint32_t w = d->images[i].width, h = d->images[i].height;
            for (uint32_t l = 0; l < d->images[i].n_levels; l++) { n += (size_t)w * h * d->images[i].channels; if (w > 1) w /= 2; if (h > 1) h /= 2; }
            std::memcpy(all.data() + at, d->images[i].texels, n * sizeof(float));
            base[i] = at;
            at += n;
        }
        if ((st = upload(ctx, ctx->d_image_texels, all.data(), all.size())) != PT_OK) return st;
        for (uint32_t i = 0; i < d->n_images; i++) dimages[i].texels = ctx->d_image_texels.as<float>() + base[i];
        if ((st = upload(ctx, ctx->d_images, dimages.data(), dimages.size())) != PT_OK) return st;
    } else { ctx->d_image_texels.release(); ctx->d_images.release(); }
    if (mt.any_textured || chk.any_alpha) {
        if (d->n_textures) { if ((st = upload(ctx, ctx->d_textures, d->textures, d->n_textures)) != PT_OK) return st; } else ctx->d_textures.release();
        if ((st = upload(ctx, ctx->d_tex_prog, mt.tex_prog.data(), mt.tex_prog.size())) != PT_OK) return st;
    } else { ctx->d_textures.release(); ctx->d_tex_prog.release(); }
    if (mt.any_textured) { if ((st = upload(ctx, ctx->d_mat_params, mt.mparams.data(), mt.mparams.size())) != PT_OK) return st; } else ctx->d_mat_params.release();
    if (d->N) { if ((st = upload(ctx, ctx->d_N, d->N, 3 * (size_t)d->n_vertices)) != PT_OK) return st; } else ctx->d_N.release();
    if (d->S) { if ((st = upload(ctx, ctx->d_S, d->S, 3 * (size_t)d->n_vertices)) != PT_OK) return st; } else ctx->d_S.release();
    if (d->UV) { if ((st = upload(ctx, ctx->d_UV, d->UV, 2 * (size_t)d->n_vertices)) != PT_OK) return st; } else ctx->d_UV.release();
    return PT_OK;
}

void fill_scene_record(pt_context* ctx, const pt_scene_desc* d, const SceneChecks& chk, const MaterialTables& mt, const WorldBuild& w, bool images_on_device) {
    PtScene& sc = ctx->sc;
    sc.nodes = ctx->d_nodes.as<PtNode>();
    sc.tris = ctx->d_tris.as<PtTri>();
    sc.tri_info = ctx->d_tri_info.as<PtTriInfo>();
    sc.N = d->N ? ctx->d_N.as<float>() : nullptr;
    sc.S = d->S ? ctx->d_S.as<float>() : nullptr;
    sc.UV = d->UV ? ctx->d_UV.as<float>() : nullptr;
    sc.materials = ctx->d_materials.as<PtMaterial>();
    sc.general_materials = mt.general_materials ? 1u : 0u;
    ctx->scene_has_lobe_materials = mt.general_materials;          // (before spheres / instances force the sorted queue on)
    sc.any_one_sided = w.any_one_sided ? 1u : 0u;
    sc.dist_leaves = (w.up_max_leaf <= 8 && !std::getenv("PBRTGPU_SEQ_LEAVES")) ? 1u : 0u;
    ctx->n_materials = d->n_materials;
    sc.lights = ctx->d_lights.as<PtLight>();
    sc.n_lights = (uint32_t)w.lights.size();
    sc.textured = mt.any_textured ? 1u : 0u;
    sc.textures = (mt.any_textured || chk.any_alpha) && d->n_textures ? ctx->d_textures.as<pt_texture>() : nullptr;
    sc.tex_prog = (mt.any_textured || chk.any_alpha) ? ctx->d_tex_prog.as<uint32_t>() : nullptr;
    ctx->scene_alpha = chk.any_alpha;
    ctx->quadric_kernels = false;
    for (uint32_t i = 0; i < d->n_spheres; i++) ctx->quadric_kernels |= d->spheres[i].kind != PT_SHAPE_SPHERE;
    sc.images = images_on_device ? ctx->d_images.as<PtImage>() : nullptr;
    sc.mat_params = mt.any_textured ? ctx->d_mat_params.as<PtMatParams>() : nullptr;
    sc.spheres = d->n_spheres ? ctx->d_spheres.as<PtSphere>() : nullptr;
    sc.instances = (d->n_instances || !w.motion.empty()) ? ctx->d_instances.as<PtInstance>() : nullptr;
    ctx->motion_kernels = w.camera_moves || w.instances_move;
    ctx->motion_instances = w.instances_move;
    sc.n_instances = d->n_instances;
    sc.n_spheres = d->n_spheres;
    if (d->n_spheres) sc.general_materials = 1;     // sphere scenes run the sphere-capable kernel instantiations (sorted shade queue)
    if (d->n_instances) { sc.general_materials = 1; sc.dist_leaves = 0; }      // k_trace_inst walks leaves per lane; one shade kernel handles everything
    // The mix materials' count rides above bit 0 (scene_n_mix).  This is the LAST write to the field: the assignments above set bit 0 and would
    // erase the count, and every reader takes the field as a truth value or through scene_n_mix, never by comparing it with 1.
    sc.general_materials = (sc.general_materials & 1u) | ((uint32_t)mt.mixes.size() << 1);
    sc.root_ref = w.up_root_ref;
    sc.n_top = w.n_top;
    for (int a = 0; a < 3; a++) { const float ext = w.up_root_hi[a] - w.up_root_lo[a]; sc.cell_scale[a] = ext > 0.0f ? (float)(1u << PT_SORT_CELL_BITS) / ext : 0.0f; }
    std::memcpy(sc.wb_min, w.up_root_lo, 12);
    std::memcpy(sc.wb_max, w.up_root_hi, 12);
}

// The PtDeltaLight / PtEnvLight records behind the light list, each light's power for the "power" strategy, and the integrator's settings
pt_status build_delta_and_env_records(pt_context* ctx, const pt_scene_desc* d, const std::vector<PtLight>& lights, std::vector<float>& env_power, std::vector<float>& delta_power) {
    PtScene& sc = ctx->sc;
    pt_status st;
    env_power.assign(ctx->inf_lights.size(), 0.0f);
    delta_power.assign(ctx->delta_lights.size() + ctx->map_lights.size(), 0.0f);
    sc.n_envs = 0;
    sc.n_deltas = 0;
    std::vector<PtEnvLight> envs(ctx->inf_lights.size());
    std::vector<PtDeltaLight> deltas(ctx->delta_lights.size() + ctx->map_lights.size());
    std::vector<PtMapLight> maps(ctx->map_lights.size());
    ctx->maplight_kernels = !ctx->map_lights.empty();
    // Light::preprocess: Bounds3::bounding_sphere of the world bound (bounds3.rs:173-177), half the diagonal
    const float dx = sc.wb_max[0] - sc.wb_min[0], dy = sc.wb_max[1] - sc.wb_min[1], dz = sc.wb_max[2] - sc.wb_min[2];
    const float radius = std::sqrt(dx * dx + dy * dy + dz * dz) * 0.5f;
    if (!ctx->delta_lights.empty()) {    // PtDeltaLight records: what PointLight::new / SpotLight::new / DistantLight::new + preprocess compute
        const float kPiF = 3.14159265358979323846f;
        auto lum = [](float r, float g, float b) { return 0.212671f * r + 0.715160f * g + 0.072169f * b; };
        for (size_t k = 0; k < ctx->delta_lights.size(); k++) {
            const pt_delta_light& dl = ctx->delta_lights[k];
            PtDeltaLight& o = deltas[k];
            std::memset(&o, 0, sizeof(o));
            o.kind = (uint32_t)dl.kind;
            std::memcpy(o.spectrum, dl.spectrum, 12);
            const float* m = dl.light_to_world;
            float s = 0.0f;
            if (dl.kind == PT_DELTA_DISTANT) {
                // w_light = normalize(light_to_world.transform_vector(from - to)) (distant.rs:28); power = L * (pi r^2) (:77-81)
                const float x = dl.direction[0], y = dl.direction[1], z = dl.direction[2];
                const float vx = m[0] * x + m[1] * y + m[2] * z, vy = m[4] * x + m[5] * y + m[6] * z, vz = m[8] * x + m[9] * y + m[10] * z;
                const float len = std::sqrt(vx * vx + vy * vy + vz * vz);
                o.v[0] = vx / len; o.v[1] = vy / len; o.v[2] = vz / len;
                o.radius = radius;
                s = kPiF * radius * radius;
            } else {
                // p_light = light_to_world.transform_point(0) (point.rs:33, spot.rs:32; matrix4x4.rs:284-297 with w = 1 for an affine matrix)
                for (int a = 0; a < 3; a++) o.v[a] = m[4 * a] * 0.0f + m[4 * a + 1] * 0.0f + m[4 * a + 2] * 0.0f + m[4 * a + 3];
                if (dl.kind == PT_DELTA_SPOT) {
                    o.cos_total_width = std::cos(dl.cone_total_width * (kPiF / 180.0f));        // spot.rs:13-16, :34-35
                    o.cos_falloff_start = std::cos(dl.cone_falloff_start * (kPiF / 180.0f));
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) o.w2l[3 * a + b] = dl.world_to_light[4 * a + b];
                    s = 2.0f * kPiF * (1.0f - 0.5f * (o.cos_falloff_start - o.cos_total_width));      // spot.rs:81-84
                } else {
                    s = 4.0f * kPiF;                                                                   // point.rs:61-63
                }
            }
            delta_power[k] = lum(o.spectrum[0] * s, o.spectrum[1] * s, o.spectrum[2] * s);
        }
    }
    // GonioPhotometricLight::new / ProjectionLight::new (goniometric.rs:13-33, projection.rs:19-57) and their power() (:66-70, :99-103)
    for (size_t k = 0; k < maps.size(); k++) {
        const pt_map_light& ml = ctx->map_lights[k];
        PtDeltaLight& o = deltas[ctx->delta_lights.size() + k];
        PtMapLight& mo = maps[k];
        std::memset(&o, 0, sizeof(o));
        std::memset(&mo, 0, sizeof(mo));
        o.kind = (uint32_t)ml.kind;
        o.pad = (uint32_t)k;
        std::memcpy(o.spectrum, ml.spectrum, 12);
        const float* m = ml.light_to_world;
        for (int a = 0; a < 3; a++) o.v[a] = m[4 * a] * 0.0f + m[4 * a + 1] * 0.0f + m[4 * a + 2] * 0.0f + m[4 * a + 3];       // p_light = light_to_world.transform_point(0)
        std::memcpy(mo.w2l, ml.world_to_light, 48);
        mo.image = (uint32_t)ml.image;
        const EnvMap map(d->images[ml.image]);
        float c[3];
        map.lookup(0.5f, 0.5f, 0.5f, c);
        const float kPiF = 3.14159265358979323846f;
        float pw[3];
        if (ml.kind == PT_DELTA_GONIOMETRIC) {
            for (int a = 0; a < 3; a++) pw[a] = 4.0f * kPiF * o.spectrum[a] * c[a];
        } else {
            const float aspect = (float)ml.resolution[0] / (float)ml.resolution[1];
            if (aspect > 1.0f) { mo.screen[0] = -aspect; mo.screen[1] = -1.0f; mo.screen[2] = aspect; mo.screen[3] = 1.0f; }
            else { mo.screen[0] = -1.0f; mo.screen[1] = -1.0f / aspect; mo.screen[2] = 1.0f; mo.screen[3] = 1.0f / aspect; }
            pth::Xf proj;
            if (!pth::xf_perspective(ml.fov, 1e-3f, 1e30f, &proj)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "projection light: fov gives a singular projection");
            std::memcpy(mo.proj, proj.m.a, 64);
            // w_corner = screen_to_light.transform_point((max.x, max.y, 0)).normalize(); cos_total_width = w_corner.z
            const float* q = proj.inv.a;
            const float x = mo.screen[2], y = mo.screen[3], z = 0.0f;
            float cx = q[0] * x + q[1] * y + q[2] * z + q[3], cy = q[4] * x + q[5] * y + q[6] * z + q[7], cz = q[8] * x + q[9] * y + q[10] * z + q[11];
            const float cw = q[12] * x + q[13] * y + q[14] * z + q[15];
            if (cw != 1.0f) { cx = cx / cw; cy = cy / cw; cz = cz / cw; }
            const float len = std::sqrt(cx * cx + cy * cy + cz * cz);
            o.cos_total_width = cz / len;
            const float cone = 2.0f * kPiF * (1.0f - o.cos_total_width);
            for (int a = 0; a < 3; a++) pw[a] = c[a] * o.spectrum[a] * cone;
        }
        delta_power[ctx->delta_lights.size() + k] = 0.212671f * pw[0] + 0.715160f * pw[1] + 0.072169f * pw[2];
    }
    if (!ctx->inf_lights.empty()) {      // PtEnvLight records + their Distribution2D tables (one buffer; its bytes are gone from what the path pool may take)
        const size_t ne = ctx->inf_lights.size();
        std::vector<std::vector<float>> tabs(ne);
        std::vector<size_t> tab_off(ne);
        size_t total = 0;
        for (size_t k = 0; k < ne; k++) {
            const pt_infinite_light& il = ctx->inf_lights[k];
            PtEnvLight& e = envs[k];
            std::memset(&e, 0, sizeof(e));
            std::memcpy(e.l2w, il.light_to_world, 48);
            std::memcpy(e.w2l, il.world_to_light, 48);
            e.radius = radius;
            e.image = (uint32_t)il.image;
            env_distribution(d->images[il.image], &e.nu, &e.nv, &tabs[k], &e.m_int);
            tab_off[k] = total;
            total += (tabs[k].size() + 3) & ~(size_t)3;
            // power (infinite.rs:100-109): pi r^2 * lookup((.5, .5), .5), its y() for the power strategy
            const EnvMap map(d->images[il.image]);
            float c[3];
            map.lookup(0.5f, 0.5f, 0.5f, c);
            const float s = 3.14159265358979323846f * radius * radius;
            const float r = c[0] * s, g = c[1] * s, b = c[2] * s;
            env_power[k] = 0.212671f * r + 0.715160f * g + 0.072169f * b;
        }
        std::vector<float> all(total);
        for (size_t k = 0; k < ne; k++) std::memcpy(all.data() + tab_off[k], tabs[k].data(), tabs[k].size() * sizeof(float));
        if ((st = upload(ctx, ctx->d_env_tabs, all.data(), all.size())) != PT_OK) return st;
        for (size_t k = 0; k < ne; k++) {
            PtEnvLight& e = envs[k];
            const float* base = ctx->d_env_tabs.as<float>() + tab_off[k];
            e.func = base;
            e.cdf = e.func + (size_t)e.nv * e.nu;
            e.mfunc = e.cdf + (size_t)e.nv * (e.nu + 1);
            e.mcdf = e.mfunc + e.nv;
        }
    } else { ctx->d_env_tabs.release(); }
    if (!envs.empty() || !deltas.empty()) {
        const size_t ne = envs.size(), nd = deltas.size(), lb = lights.size() * sizeof(PtLight);
        std::vector<uint8_t> lbuf(lb + ne * sizeof(PtEnvLight) + nd * sizeof(PtDeltaLight) + maps.size() * sizeof(PtMapLight));       // the records behind the lights (scene_envs, scene_deltas, scene_map_lights)
        std::memcpy(lbuf.data(), lights.data(), lb);
        if (ne) std::memcpy(lbuf.data() + lb, envs.data(), ne * sizeof(PtEnvLight));
        if (nd) std::memcpy(lbuf.data() + lb + ne * sizeof(PtEnvLight), deltas.data(), nd * sizeof(PtDeltaLight));
        if (!maps.empty()) std::memcpy(lbuf.data() + lb + ne * sizeof(PtEnvLight) + nd * sizeof(PtDeltaLight), maps.data(), maps.size() * sizeof(PtMapLight));
        if ((st = upload(ctx, ctx->d_lights, lbuf.data(), lbuf.size())) != PT_OK) return st;
        sc.lights = ctx->d_lights.as<PtLight>();
        sc.n_envs = (uint32_t)ne;
        sc.n_deltas = (uint32_t)nd;
        // the hit records were numbered over the area lights alone: give every emitter its index in the merged list
        PT_HIP(ptk_light_renumber(ctx->stream, ctx->d_tris.as<PtTri>(), ctx->d_tri_info.p ? ctx->d_tri_info.as<PtTriInfo>() : nullptr, sc.lights, (uint32_t)lights.size()));
        PT_HIP(hipStreamSynchronize(ctx->stream));
    }
    sc.max_depth = d->max_depth;
    sc.integrator = d->integrator;
    ctx->aov_target = ctx->next_aov_target;
    ctx->aov_scale = ctx->next_aov_scale;
    sc.direct_strategy = d->direct_strategy;
    sc.ao_samples = d->ao_samples > 0 ? d->ao_samples : 64;
    sc.ao_cos_sample = d->ao_cos_sample != 0;
    sc.rr_threshold = d->rr_threshold;
    return PT_OK;
}

// ---- camera ---------------------------------------------------------------
pt_status setup_camera(pt_context* ctx, const pt_scene_desc* d) {
    PtScene& sc = ctx->sc;
    pth::M44 r2c;
    if (!pth::raster_to_camera(d->fov, d->screen_window, d->xres, d->yres, &r2c)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "singular camera projection");
    std::memcpy(sc.cam.raster_to_camera, r2c.a, 64);
    std::memcpy(sc.cam.camera_to_world, d->camera_to_world, 64);
    sc.cam.lens_radius = d->lens_radius;
    sc.cam.focal_distance = d->focal_distance;
    sc.cam.shutter_open = d->shutter_open; sc.cam.shutter_close = d->shutter_close;
    return PT_OK;
}

// ---- film (Film::new, film.rs:62-100; get_sample_bounds :166-179) ---------
pt_status setup_film(pt_context* ctx, const pt_scene_desc* d) {
    PtFilm& fm = ctx->sc.film;
    fm.crop[0] = std::max(0, (int)std::floor((float)d->xres * d->crop_window[0]));
    fm.crop[1] = std::max(0, (int)std::floor((float)d->yres * d->crop_window[2]));
    fm.crop[2] = std::min((int)std::ceil((float)d->xres * d->crop_window[1]), d->xres);
    fm.crop[3] = std::min((int)std::ceil((float)d->yres * d->crop_window[3]), d->yres);
    if (fm.crop[2] <= fm.crop[0] || fm.crop[3] <= fm.crop[1]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "empty crop window");
    fm.filter_radius[0] = d->filter_radius[0]; fm.filter_radius[1] = d->filter_radius[1];
    fm.inv_filter_radius[0] = 1.0f / d->filter_radius[0]; fm.inv_filter_radius[1] = 1.0f / d->filter_radius[1];
    fm.sample_bounds[0] = (int)std::floor((float)fm.crop[0] - fm.filter_radius[0]);
    fm.sample_bounds[1] = (int)std::floor((float)fm.crop[1] - fm.filter_radius[1]);
    fm.sample_bounds[2] = (int)std::ceil((float)fm.crop[2] + fm.filter_radius[0]);
    fm.sample_bounds[3] = (int)std::ceil((float)fm.crop[3] + fm.filter_radius[1]);
    fm.max_sample_luminance = d->max_sample_luminance;
    fm.scale = d->film_scale;
    std::memcpy(fm.filter_table, d->filter_table, sizeof(fm.filter_table));
    ctx->film_w = (uint32_t)(fm.crop[2] - fm.crop[0]);
    ctx->film_h = (uint32_t)(fm.crop[3] - fm.crop[1]);
    uint32_t sbw = (uint32_t)(fm.sample_bounds[2] - fm.sample_bounds[0]), sbh = (uint32_t)(fm.sample_bounds[3] - fm.sample_bounds[1]);
    if (sbw >= 65536 || sbh >= 65536) return ctx->fail(PT_ERR_UNSUPPORTED, "film larger than 65535 pixels on a side");
    return PT_OK;
}

// ---- sampler (SobolSampler::new, samplers/sobol.rs:16-31) -----------------
pt_status setup_sampler(pt_context* ctx, const pt_scene_desc* d) {
    pt_status st;
    const PtFilm& fm = ctx->sc.film;
    const uint32_t sbw = (uint32_t)(fm.sample_bounds[2] - fm.sample_bounds[0]), sbh = (uint32_t)(fm.sample_bounds[3] - fm.sample_bounds[1]);
    PtSobol& sb = ctx->sc.sobol;
    sb.resolution = round_up_pow2(std::max(sbw, sbh));
    sb.log2_resolution = log2int(sb.resolution);
    sb.kind = (uint32_t)d->sampler;
    sb.spp = sb.kind == PT_SAMPLER_HALTON ? (uint32_t)d->spp : round_up_pow2((uint32_t)d->spp);
    if (sb.kind == PT_SAMPLER_HALTON) {
        if ((st = setup_halton(ctx, sb, (int32_t)sbw, (int32_t)sbh, d->halton_sample_at_center != 0)) != PT_OK) return st;
        sb.resolution = 1;
        sb.log2_resolution = 0;      // the Sobol' index tables are not consulted
    }
    if (sb.log2_resolution > 0 && (sb.log2_resolution - 1 >= ctx->sobol_n_vdc || sb.log2_resolution - 1 >= ctx->sobol_n_inv))
        return ctx->fail(PT_ERR_UNSUPPORTED, "film resolution beyond the VdC Sobol' tables");
    if ((st = upload(ctx, ctx->d_m32, ctx->sobol_m32.data(), ctx->sobol_m32.size())) != PT_OK) return st;
    size_t row = sb.log2_resolution > 0 ? (size_t)(sb.log2_resolution - 1) * ctx->sobol_msize : 0;
    if ((st = upload(ctx, ctx->d_vdc, ctx->sobol_vdc.data() + row, ctx->sobol_msize)) != PT_OK) return st;
    if ((st = upload(ctx, ctx->d_vdc_inv, ctx->sobol_inv.data() + row, ctx->sobol_msize)) != PT_OK) return st;
    sb.m32 = ctx->d_m32.as<uint32_t>();
    sb.m32_len = (uint32_t)ctx->sobol_m32.size();
    if (!ctx->d_bytetab.p) {
        // byte-sliced form of SOBOL_MATRICES_32: T[dim][k][x] = XOR over set bits j of x of column 8k+j,
        // with the reference's column indexing ((dim*52 + c) % len, sobol.rs:43-52) for c up to 55
        const uint32_t n_dims = (uint32_t)(ctx->sobol_m32.size() / ctx->sobol_msize);
        const size_t len = ctx->sobol_m32.size();
        std::vector<uint32_t> tab((size_t)n_dims * 7 * 256);
        for (uint32_t dim = 0; dim < n_dims; dim++) {
            size_t base = std::min((size_t)dim * 52, len - 1);
            for (uint32_t k = 0; k < 7; k++) {
                uint32_t* t = &tab[((size_t)dim * 7 + k) * 256];
                t[0] = 0;
                for (uint32_t x = 1; x < 256; x++) {
                    uint32_t low = x & (~x + 1u);              // lowest set bit
                    uint32_t j = (uint32_t)__builtin_ctz(x);
                    t[x] = t[x ^ low] ^ ctx->sobol_m32[(base + 8 * k + j) % len];
                }
            }
        }
        if ((st = upload(ctx, ctx->d_bytetab, tab.data(), tab.size())) != PT_OK) return st;
    }
    sb.bytetab = ctx->d_bytetab.as<uint32_t>();
    sb.n_tab_dims = (uint32_t)(ctx->sobol_m32.size() / ctx->sobol_msize);
    sb.vdc = ctx->d_vdc.as<uint64_t>();
    sb.vdc_inv = ctx->d_vdc_inv.as<uint64_t>();
    return PT_OK;
}

// ---- light sampling distribution (create_light_sample_distribution.rs:11-50) -
pt_status build_light_distribution(pt_context* ctx, const pt_scene_desc* d, const std::vector<PtLight>& lights, const std::vector<float>& env_power, const std::vector<float>& delta_power) {
    PtScene& sc = ctx->sc;
    pt_status st;
    PtLightGrid& g = sc.grid;
    g.n_lights = sc.n_lights;
    g.stride = (2 * sc.n_lights + 2 + 3) & ~3u;     // rows are 16-byte aligned
    std::memcpy(g.wb_min, sc.wb_min, 12);
    std::memcpy(g.wb_max, sc.wb_max, 12);
    int strategy = d->light_strategy;
    if (strategy == PT_LIGHTS_UNIFORM && sc.n_lights != 1) strategy = PT_LIGHTS_SPATIAL;
    ctx->grid_lazy = false;
    ctx->trace_far_choice = -1;          // a new scene: the trial runs again
    if (sc.n_lights > 0) {
        if (strategy == PT_LIGHTS_SPATIAL) {
            const uint32_t max_voxels = 64;
            float diag[3] = {sc.wb_max[0] - sc.wb_min[0], sc.wb_max[1] - sc.wb_min[1], sc.wb_max[2] - sc.wb_min[2]};
            int ext = (diag[0] > diag[1] && diag[0] > diag[2]) ? 0 : (diag[1] > diag[2] ? 1 : 2);
            float bmax = diag[ext];
            size_t nvox = 1;
            for (int i = 0; i < 3; i++) {
                float c = std::ceil(diag[i] / bmax * (float)max_voxels);
                uint32_t v = c > 0.0f ? (c >= 4294967296.0f ? 0xffffffffu : (uint32_t)c) : 0u;
                v = std::min(std::max(v, 1u), max_voxels);
                g.voxels[i] = v;
                nvox *= v;
            }
            g.single = 0;
            size_t bytes = nvox * g.stride * sizeof(float);
            // Dense while it is small (every voxel's tables made here, at upload: 0.6 ms for RT1M's 262 144 voxels x 2 lights); from
            // PBRTGPU_LIGHT_GRID_DENSE_MAX bytes on (default 2 GiB: about a thousand lights) the grid is filled as the reference fills its hash table
            // (spatial.rs:199-260), voxel by voxel on first touch -- render_tiles lists the voxels each bounce's hits fall in (k_grid_mark) and makes
            // their rows before the bounce is shaded.  A mesh light of ten thousand triangles is 80 KB per voxel: 21 GB dense, a few hundred MB for
            // the voxels a frame actually visits.
            size_t dense_max = (size_t)2 << 30;
            if (const char* e = std::getenv("PBRTGPU_LIGHT_GRID_DENSE_MAX")) dense_max = std::strtoull(e, nullptr, 10);
            ctx->grid_lazy = bytes > dense_max;
            ctx->grid_nvox = nvox;
            if (!ctx->grid_lazy) {
                PT_HIP(ctx->d_grid.alloc(bytes + 64));
                g.data = ctx->d_grid.as<float>();
                PT_HIP(ptk_light_grid_any(ctx, ctx->stream, sc, ctx->d_grid.as<float>(), (uint32_t)nvox));
                PT_HIP(hipStreamSynchronize(ctx->stream));
            } else {
                const size_t row_bytes = (size_t)g.stride * sizeof(float);
                ctx->grid_rows_cap = std::min<size_t>(nvox, std::max<size_t>(256, ((size_t)256 << 20) / row_bytes));
                ctx->grid_rows_used = 0;
                PT_HIP(ctx->d_grid.alloc(ctx->grid_rows_cap * row_bytes + 64));
                PT_HIP(ctx->d_grid_rows.alloc(nvox * 4));
                PT_HIP(ctx->d_grid_todo.alloc(nvox * 4 + 64));          // the voxel list, then its counter
                PT_HIP(hipMemsetAsync(ctx->d_grid_rows.p, 0xff, nvox * 4, ctx->stream));
                PT_HIP(hipMemsetAsync(ctx->d_grid_todo.as<uint32_t>() + nvox, 0, 64, ctx->stream));
                g.data = ctx->d_grid.as<float>();
                g.row_of = ctx->d_grid_rows.as<int32_t>();
            }
        } else {
            // uniform / power: one Distribution1D (lightdistrib/uniform.rs, power.rs:9-17)
            g.voxels[0] = g.voxels[1] = g.voxels[2] = 1;
            g.single = 1;
            uint32_t nl = sc.n_lights;
            std::vector<float> tab(g.stride + 16);
            for (uint32_t i = 0; i < nl; i++) {
                if (strategy == PT_LIGHTS_UNIFORM) tab[i] = 1.0f;
                else if (lights[i].mesh_flags & PT_LIGHT_INFINITE) {
                    uint32_t k;
                    std::memcpy(&k, &lights[i].p0[0], 4);
                    tab[i] = env_power[k];
                } else if (lights[i].mesh_flags & PT_LIGHT_DELTA) {
                    uint32_t k;
                    std::memcpy(&k, &lights[i].p0[0], 4);
                    tab[i] = delta_power[k];
                } else {
                    float n = lights[i].two_sided ? 2.0f : 1.0f;
                    float s = n * lights[i].area * 3.14159265358979323846f;
                    float r = lights[i].L[0] * s, gg = lights[i].L[1] * s, b = lights[i].L[2] * s;
                    tab[i] = 0.212671f * r + 0.715160f * gg + 0.072169f * b;
                }
            }
            float* cdf = tab.data() + nl;
            cdf[nl + 1] = dist1d_build(tab.data(), nl, cdf);
            if ((st = upload(ctx, ctx->d_grid, tab.data(), tab.size())) != PT_OK) return st;
            g.data = ctx->d_grid.as<float>();
        }
    }
    return PT_OK;
}

// ---- film + scratch buffers ---------------------------------------------------
pt_status alloc_film_and_scratch(pt_context* ctx) {
    size_t npx = (size_t)ctx->film_w * ctx->film_h;
    PT_HIP(ctx->d_own.alloc(npx * 16));
    PT_HIP(ctx->d_spillfilm.alloc(npx * 16));
    PT_HIP(ctx->d_xyzw.alloc(npx * 16));
    PT_HIP(ctx->d_rgb.alloc(npx * 12));
    // every kernel runs on ctx->stream (non-blocking: no implicit ordering with the null stream), so do these
    PT_HIP(hipMemsetAsync(ctx->d_own.p, 0, npx * 16, ctx->stream));
    PT_HIP(hipMemsetAsync(ctx->d_spillfilm.p, 0, npx * 16, ctx->stream));
    PT_HIP(hipMemsetAsync(ctx->d_xyzw.p, 0, npx * 16, ctx->stream));
    ctx->xyzw_committed = false;
    if (!ctx->d_counters.p) {
        PT_HIP(ctx->d_counters.alloc(sizeof(PtCounters)));
        PT_HIP(hipMemsetAsync(ctx->d_counters.p, 0, sizeof(PtCounters), ctx->stream));
        if (!ctx->d_err.p) {
            PT_HIP(ctx->d_err.alloc(16));
            PT_HIP(hipMemsetAsync(ctx->d_err.p, 0, 16, ctx->stream));
        }
        PT_HIP(ctx->d_ticket.alloc(16));
        PT_HIP(ctx->d_counts.alloc(PT_COUNTS_WORDS * 4));
        PT_HIP(hipMemsetAsync(ctx->d_counts.p, 0, PT_COUNTS_WORDS * 4, ctx->stream));
    }
    PT_HIP(hipStreamSynchronize(ctx->stream));
    return ensure_traversal_scratch(ctx);
}

void fill_info(pt_context* ctx, const WorldBuild& w, double t0, double t2) {
    const PtScene& sc = ctx->sc;
    pt_scene_info& inf = ctx->info;
    std::memset(&inf, 0, sizeof(inf));
    for (int i = 0; i < 4; i++) { inf.sample_bounds[i] = sc.film.sample_bounds[i]; inf.cropped_bounds[i] = sc.film.crop[i]; }
    inf.spp = (int32_t)sc.sobol.spp;
    inf.n_lights = sc.n_lights;
    inf.n_nodes = (uint32_t)w.up_n_nodes;
    inf.n_leaves = w.up_n_leaves;
    std::memcpy(inf.world_bound, sc.wb_min, 12);
    std::memcpy(inf.world_bound + 3, sc.wb_max, 12);
    inf.bvh_build_ms = w.t1 - t0;
    inf.upload_ms = t2 - w.t1;
    inf.bvh_on_device = w.dev_build.used ? 1 : 0;
    inf.fourier_capped = 0;
}

// The stages in order.  The first refusal or device error ends the upload: have_scene stays false and no buffer of the half-made scene is observable.
pt_status scene_upload(pt_context* ctx, const pt_scene_desc* d) {
    (void)hipSetDevice(ctx->device);
    ctx->have_scene = false;
    pt_status st;
    SceneChecks chk;
    if ((st = check_scene(ctx, d, chk)) != PT_OK) return st;
    if (ctx->sobol_m32.empty() && !load_sobol(ctx)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "cannot read sobol_tables.bin from data dir '" + ctx->data_dir + "'");

    const double t0 = now_ms();
    double tm_last = t0;
    double* trace = std::getenv("PBRTGPU_BUILD_TRACE") ? &tm_last : nullptr;
    WorldBuild w;
    w.t1 = t0;
    w.dev_build = ptbvh::DeviceBuild{ctx->stream, ctx->bvh_build_where, false, hipSuccess};
    w.max_node_prims = d->max_node_prims > 0 ? d->max_node_prims : 4;
    struct TrimBvh { pt_context* c; ~TrimBvh() { if (c->host_bvh.nodes.capacity() * sizeof(PtNode) > ((size_t)1 << 30)) c->host_bvh = ptbvh::Result(); } } trim_bvh{ctx};
    if ((st = build_motion_records(ctx, d, w)) != PT_OK) return st;
    bool on_device = false;
    if ((st = build_world_on_device(ctx, d, chk, w, trace, &on_device)) != PT_OK) return st;
    if (!on_device) {
        std::vector<Entry> world, rec_entry;
        if ((st = build_lists_and_trees(ctx, d, chk, w, trace, world, rec_entry)) != PT_OK) return st;
        if ((st = build_shading_records(ctx, d, w, world, rec_entry)) != PT_OK) return st;
        if ((st = finish_and_upload_nodes(ctx, w)) != PT_OK) return st;
    }
    MaterialTables mt;
    if ((st = build_materials(ctx, d, chk, mt)) != PT_OK) return st;
    std::memset(&ctx->sc, 0, sizeof(ctx->sc));
    if (w.up_n_nodes >= (1u << 25)) return ctx->fail(PT_ERR_UNSUPPORTED, "more than 2^25 BVH nodes (32-bit node offsets)");
    ctx->n_nodes_up = w.up_n_nodes; ctx->n_tris_up = w.up_n_tris;
    bool images_on_device = false;
    if ((st = upload_materials_and_lights(ctx, d, mt, w)) != PT_OK) return st;
    if ((st = upload_images_and_textures(ctx, d, chk, mt, images_on_device)) != PT_OK) return st;
    fill_scene_record(ctx, d, chk, mt, w, images_on_device);
    std::vector<float> env_power, delta_power;
    if ((st = build_delta_and_env_records(ctx, d, w.lights, env_power, delta_power)) != PT_OK) return st;
    if ((st = setup_camera(ctx, d)) != PT_OK) return st;
    if ((st = setup_film(ctx, d)) != PT_OK) return st;
    if ((st = setup_sampler(ctx, d)) != PT_OK) return st;
    if ((st = build_light_distribution(ctx, d, w.lights, env_power, delta_power)) != PT_OK) return st;
    if ((st = alloc_film_and_scratch(ctx)) != PT_OK) return st;
    const double t2 = now_ms();

    fill_info(ctx, w, t0, t2);
    ctx->have_scene = true;
    return PT_OK;
}

}  // namespace

extern "C" {

// The infinite lights set with pt_scene_set_infinite_lights belong to this upload alone: a later upload of another scene does not inherit
// them (their image indices point into this descriptor's images[]).
pt_status pt_scene_upload(pt_context* ctx, const pt_scene_desc* d) {
    if (!ctx || !d) return PT_ERR_INVALID_ARGUMENT;
    const pt_status st = scene_upload(ctx, d);
    ctx->inf_lights.clear();
    ctx->delta_lights.clear();
    ctx->map_lights.clear();
    ctx->alpha_masks.clear();
    ctx->disney_recs.clear();
    ctx->fourier_tables.clear();
    ctx->fourier_recs.clear();
    ctx->next_has_motion = false;
    ctx->next_motion_inst.clear();
    ctx->next_aov_target = PT_AOV_UV;
    ctx->next_aov_scale = 1.0f;
    return st;
}

pt_status pt_scene_set_infinite_lights(pt_context* ctx, uint32_t n, const pt_infinite_light* lights) {
    if (!ctx || (n && !lights)) return PT_ERR_INVALID_ARGUMENT;
    ctx->inf_lights.assign(lights, lights + n);
    return PT_OK;
}

pt_status pt_scene_set_delta_lights(pt_context* ctx, uint32_t n, const pt_delta_light* lights) {
    if (!ctx || (n && !lights)) return PT_ERR_INVALID_ARGUMENT;
    ctx->delta_lights.assign(lights, lights + n);
    return PT_OK;
}

pt_status pt_scene_set_map_lights(pt_context* ctx, uint32_t n, const pt_map_light* lights) {
    if (!ctx || (n && !lights)) return PT_ERR_INVALID_ARGUMENT;
    ctx->map_lights.assign(lights, lights + n);
    return PT_OK;
}

pt_status pt_scene_set_alpha_masks(pt_context* ctx, uint32_t n, const pt_alpha_mask* masks) {
    if (!ctx || (n && !masks)) return PT_ERR_INVALID_ARGUMENT;
    ctx->alpha_masks.assign(masks, masks + n);
    return PT_OK;
}

pt_status pt_scene_set_disney(pt_context* ctx, uint32_t n, const pt_disney* records) {
    if (!ctx || (n && !records)) return PT_ERR_INVALID_ARGUMENT;
    ctx->disney_recs.assign(records, records + n);
    return PT_OK;
}

pt_status pt_scene_set_fourier(pt_context* ctx, uint32_t n_tables, const pt_fourier_table* tables, uint32_t n_records, const pt_fourier* records) {
    if (!ctx || (n_tables && !tables) || (n_records && !records)) return PT_ERR_INVALID_ARGUMENT;
    ctx->fourier_tables.assign(n_tables, pt_context::FourierTable());
    for (uint32_t t = 0; t < n_tables; t++) {
        const pt_fourier_table& in = tables[t];
        pt_context::FourierTable& o = ctx->fourier_tables[t];
        o.n_mu = in.n_mu; o.n_channels = in.n_channels; o.m_max = in.m_max; o.n_coeffs = in.n_coeffs; o.eta = in.eta;
        o.refusal = pt_fourier_table_refusal(in);          // (it looks at the counts before it reads an array)
        if (!o.refusal.empty()) continue;                   // the upload reports it
        const size_t n2 = (size_t)in.n_mu * (size_t)in.n_mu;
        o.mu.assign(in.mu, in.mu + in.n_mu);
        o.cdf.assign(in.cdf, in.cdf + n2);
        o.offset_and_length.assign(in.offset_and_length, in.offset_and_length + 2 * n2);
        if (in.n_coeffs) o.a.assign(in.a, in.a + in.n_coeffs);
    }
    ctx->fourier_recs.assign(records, records + n_records);
    return PT_OK;
}

pt_status pt_scene_set_motion(pt_context* ctx, const pt_motion* motion) {
    if (!ctx || (motion && motion->n_instances && !motion->instances)) return PT_ERR_INVALID_ARGUMENT;
    ctx->next_has_motion = motion != nullptr;
    ctx->next_motion_inst.clear();
    if (motion) {
        ctx->next_motion = *motion;
        ctx->next_motion_inst.assign(motion->instances, motion->instances + motion->n_instances);
        ctx->next_motion.instances = nullptr;
    }
    return PT_OK;
}

pt_status pt_scene_set_aov(pt_context* ctx, int32_t target, float scale) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (target < PT_AOV_DISTANCE || target > PT_AOV_DPDVS) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "unknown AOV target");
    ctx->next_aov_target = target;
    ctx->next_aov_scale = scale;
    return PT_OK;
}

pt_status pt_bvh_leaf_order(const pt_scene_desc* d, uint32_t* order_out, uint32_t* n_nodes, uint32_t* n_leaves, uint32_t* max_stack) {
    if (!d || !order_out || (d->n_triangles == 0 && d->n_spheres == 0)) return PT_ERR_INVALID_ARGUMENT;
    if (d->n_triangles > 0 && (!d->P || !d->indices || !d->tri_mesh || !d->meshes)) return PT_ERR_INVALID_ARGUMENT;
    if (d->n_spheres > 0 && !d->spheres) return PT_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> tri_flags(d->n_triangles, 0);
    std::vector<PtSphere> sph;
    std::vector<ptbvh::SpherePrim> sprims;
    build_spheres(d, sph, sprims);
    for (ptbvh::SpherePrim& sp : sprims) sp.flags = PT_TRI_SPHERE;
    ptbvh::Result bvh;
    if (!ptbvh::build(d->P, d->indices, tri_flags.data(), d->n_triangles, sprims.data(), d->n_spheres, d->split_method,
                      d->max_node_prims > 0 ? d->max_node_prims : 4, &bvh))
        return PT_ERR_UNSUPPORTED;
    for (uint32_t r = 0; r < d->n_triangles + d->n_spheres; r++) order_out[r] = bvh.tris[r].prim;
    if (n_nodes) *n_nodes = (uint32_t)bvh.nodes.size();
    if (n_leaves) *n_leaves = bvh.n_leaves;
    if (max_stack) *max_stack = bvh.max_stack;
    return PT_OK;
}

}  // extern "C"
