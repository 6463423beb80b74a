// pt_context_impl.h -- what the translation units of the C ABI's host side share: the context, its device buffers and the launch dispatchers.
// Internal: nothing here is exported from libpbrtgpu.so.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <array>
#include <memory>
#include <vector>
#include <algorithm>
#include <thread>

#include "../../include/pbrtgpu.h"
#include "pt_bvh.h"
#include "pt_device.h"
#include "pt_host_math.h"
#include "pt_kernels.h"
#include "pt_lobes.h"

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
    hipError_t alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

uint32_t round_up_pow2(uint32_t v) { v -= 1; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; }
uint32_t log2int(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

}  // namespace

struct pt_context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err, data_dir;
    int n_cu = 256;

    // ---- scene
    bool have_scene = false;
    PtScene sc;
    pt_scene_info info;
    std::vector<pt_infinite_light> inf_lights;      // pt_scene_set_infinite_lights: the next upload's infinite lights
    std::vector<pt_delta_light> delta_lights;       // pt_scene_set_delta_lights: the next upload's point / spot / distant lights
    std::vector<pt_map_light> map_lights;           // pt_scene_set_map_lights: the next upload's goniometric / projection lights
    std::vector<pt_alpha_mask> alpha_masks;         // pt_scene_set_alpha_masks: the next upload's alpha masks
    std::vector<pt_disney> disney_recs;             // pt_scene_set_disney: the next upload's Disney parameter records
    // pt_scene_set_fourier: the next upload's tabulated BSDFs (deep copies; `refusal` is what pt_fourier_table.h said about the caller's
    // arrays, empty for a table fit to upload) and the records that name them
    struct FourierTable { int32_t n_mu = 0, n_channels = 0, m_max = 0, n_coeffs = 0; float eta = 1.0f; std::vector<float> mu, cdf, a; std::vector<int32_t> offset_and_length; std::string refusal; };
    std::vector<FourierTable> fourier_tables;
    std::vector<pt_fourier> fourier_recs;
    bool next_has_motion = false;                   // pt_scene_set_motion: the next upload's motion (the instance records copied)
    pt_motion next_motion{};
    std::vector<pt_motion_instance> next_motion_inst;
    int32_t next_aov_target = PT_AOV_UV;            // pt_scene_set_aov: the next upload's AOV target and scale (create_aov_integrator's defaults)
    float next_aov_scale = 1.0f;
    int32_t aov_target = PT_AOV_UV;                 // of the uploaded scene (read when its integrator is PT_INTEGRATOR_AOV)
    float aov_scale = 1.0f;
    bool quadric_kernels = false;                   // the uploaded scene holds a cylinder or a disk: it runs the kernels of namespace ptq (pt_kernels_quadric.hip)
    bool disney_kernels = false;                    // the uploaded scene holds a Material "disney": it runs the kernels of namespace ptd (pt_kernels_disney.hip)
    bool maplight_kernels = false;                  // the uploaded scene holds a goniometric or a projection light: it runs the kernels of namespace ptm (pt_kernels_maplight.hip)
    bool motion_kernels = false;                    // the uploaded scene's camera or one of its instances moves: it runs the kernels of namespace ptv (pt_kernels_motion.hip)
    bool fourier_kernels = false;                   // the uploaded scene holds a Material "fourier": it runs the kernels of namespace ptf (pt_kernels_fourier.hip)
    uint32_t n_fourier_tables = 0;                  // ... and that many PtFourierTable records lie at the head of d_fourier
    bool motion_instances = false;                  // ... an instance does (the trace hooks with a time need their own batch kernel then)
    bool scene_alpha = false;                       // the uploaded scene has a mask: every ray runs the alpha traversal kernels
    DevBuf d_fourier;                               // the PtFourierTable records, then their arrays
    DevBuf d_env_tabs;                              // their Distribution2D tables (the PtEnvLight records ride behind the lights in d_lights)
    DevBuf d_nodes, d_tris, d_tri_info, d_spheres, d_instances, d_hit_inst, d_textures, d_tex_prog, d_mat_params, d_images, d_image_texels, d_N, d_S, d_UV, d_materials, d_lights, d_m32, d_vdc, d_vdc_inv, d_grid, d_bytetab, d_hdims, d_hperms;
    std::vector<uint32_t> sobol_m32;
    std::vector<uint64_t> sobol_vdc, sobol_inv;
    uint32_t sobol_n_vdc = 0, sobol_n_inv = 0, sobol_msize = 52;
    uint32_t n_materials = 0;
    std::vector<uint8_t> per_hit_lobes;             // per material, what the BSDF hooks refuse: PER_HIT_MIX a "mix", PER_HIT_DISNEY a "disney" whose lobes are built at every hit
    enum { PER_HIT_NONE = 0, PER_HIT_MIX = 1, PER_HIT_DISNEY = 2 };
    uint32_t max_stack = 1;
    uint32_t film_w = 0, film_h = 0;
    int bvh_build_where = PT_BVH_BUILD_AUTO;
    size_t n_nodes_up = 0, n_tris_up = 0;

    // ---- traversal scratch
    DevBuf d_spill, d_err, d_counters, d_ticket, d_tex_res;
    uint32_t spill_depth = 0;
    int grid_trace = 1024, grid_trace_dist = 768, grid_shade = 512, grid_wide = 2048;

    // ---- path pool
    size_t pool_paths = 0;
    DevBuf d_pool;          // one slab carved into the SoA arrays of PtPaths
    PtPaths paths{};
    DevBuf d_qa, d_qb, d_qnee, d_qshadow, d_qprobe, d_qsorted, d_counts, d_pixels, d_tiles, d_tilebits;
    ptbvh::Result host_bvh;                       // upload scratch: the world tree's arrays
    std::unique_ptr<ptbvh::Prim[]> host_prims;    // upload scratch (see pt_scene_upload); released when it exceeds 4 M primitives
    size_t host_prims_cap = 0;
    DevBuf d_qbin;                                     // PtQueues::bin
    DevBuf d_sort_ids, d_sort_keys[2], d_sort_temp;   // pt_raysort.hip: the second id list, the key lists and rocprim's scratch
    size_t sort_cap = 0;
    DevBuf d_csort_ids, d_csort_keys[2], d_csort_temp; // the continuation rays' key list, the ordered copy (ids + keys) and rocprim's scratch
    size_t csort_cap = 0;
    // the lazily filled light grid (PtLightGrid::row_of): voxel -> row table, the list of voxels a bounce touched first, rows in use / allocated
    DevBuf d_grid_rows, d_grid_todo;
    size_t grid_rows_used = 0, grid_rows_cap = 0, grid_nvox = 0;
    bool grid_lazy = false;
    uint32_t* h_live = nullptr;                        // page-locked: the recursive integrators' live-sample count, read one level behind
    // k_trace_far (nodes fetched by lane pairs: scenes whose rays miss the caches): PBRTGPU_TRACE_FAR 0 never, 1 always, default -1 = decided per scene by
    // a timed trial on the scene's own rays -- the first incoherent bounce after an upload is traced twice, once by each kernel
    int trace_far = -1, trace_far_choice = -1;
    DevBuf d_cnt_save;
    // PBRTGPU_SHADE_LOCAL: the material sort inside runs of 4 096 queue entries + one lobe-list kernel (k_sort_local) instead of the global sort and a
    // kernel per class, for scenes without textured materials, instances, infinite or delta lights or a Material "mix" (every other scene keeps its own
    // path whatever this says): 0 never, 1 always -- a Matte scene lit by a sphere included --, default -1 = scenes that have lobe-list (non-Matte) constant
    // materials (mixed materials 889 -> 916 Mrays/s, with a sphere light as well 834 -> 843; a Matte scene lit by a sphere, where the sorted queue exists
    // only to select the sphere-capable kernels, loses 1.4 % and keeps the global sort)
    int shade_local = -1;
    bool scene_has_lobe_materials = false;
    int sort_cont = -1;                                // continuation rays of a bounce ordered like the shadow rays: 0 never, 1 for the traversal kernel only
                                                       // (shading keeps path order), 2 for both, -1 (default): mode 1 for scenes larger than the Infinity Cache
    int sort_cont_min = 1 << 20;                       // ... and the continuation rays (when sort_cont is on) from this many up: its own threshold (PBRTGPU_SORT_CONT_MIN)
    int sort_shadow_min = 1 << 20;                     // shadow rays of a launch are ordered by origin cell from this many up (0: never)
    DevBuf d_rec, d_counts2; // recursive integrators (directlighting, whitted): frames, differentials, next-event entries and lists; the second counter block
    size_t rec_paths = 0;
    uint32_t rec_epp = 0, rec_depth = 0;
    uint32_t light_samples_total = 0;     // sum of the lights' sample counts (DirectLighting "all")
    DevBuf d_ao;             // AO integrator: occlusion-ray batch (o, d, tmax, weight, occluded) for ao_rays_cap rays
    size_t ao_rays_cap = 0;
    size_t pixels_cap = 0;

    // ---- film
    DevBuf d_own, d_spillfilm, d_xyzw, d_rgb;
    bool xyzw_committed = false;

    // ---- timing
    std::vector<hipEvent_t> ev;
    double trace_ms = 0, shade_ms = 0, render_ms = 0;
    uint64_t trace_launches = 0;

    pt_status fail(pt_status st, const std::string& m) { err = m; return st; }
    pt_status hip_fail(hipError_t e, const char* what) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE;
    }
};

// The launchers whose kernels hold analytic-shape code (traversal, surface reconstruction, light sampling), by the scene: a cylinder or a disk asks for the second build of the kernels
// (namespace ptq, pt_kernels_quadric.hip), every other scene runs the first.  A scene that holds a Material "disney" runs the third build (namespace ptd,
// pt_kernels_disney.hip), which knows both the shapes and Disney's BxDFs.  A scene that holds a goniometric or a projection light runs the fourth (namespace
// ptm, pt_kernels_maplight.hip), which knows all of that and the two lights' image lookup.  A scene whose camera or instances move runs the fifth (namespace ptv,
// pt_kernels_motion.hip), which knows all of that and AnimatedTransform::interpolate; its k_gen keeps the time sample, so ray generation is dispatched as well.
// A scene that holds a Material "fourier" runs the sixth (namespace ptf, pt_kernels_fourier.hip), which knows all of that and FourierBSDF.
#define PTK_BY_SCENE(fn)                                                                                            \
    template <class... A>                                                                                           \
    static hipError_t fn##_any(const pt_context* ctx, A&&... a) {                                                   \
        if (ctx->fourier_kernels) return ptf::fn(std::forward<A>(a)...);                                            \
        if (ctx->motion_kernels) return ptv::fn(std::forward<A>(a)...);                                             \
        if (ctx->maplight_kernels) return ptm::fn(std::forward<A>(a)...);                                           \
        if (ctx->disney_kernels) return ptd::fn(std::forward<A>(a)...);                                             \
        return ctx->quadric_kernels ? ptq::fn(std::forward<A>(a)...) : ::fn(std::forward<A>(a)...);                 \
    }
PTK_BY_SCENE(ptk_light_grid)
PTK_BY_SCENE(ptk_grid_mark)
PTK_BY_SCENE(ptk_trace)
PTK_BY_SCENE(ptk_ao_rays)
PTK_BY_SCENE(ptk_ao_resolve)
PTK_BY_SCENE(ptk_aov)
PTK_BY_SCENE(ptk_rec_init)
PTK_BY_SCENE(ptk_rec_enter)
PTK_BY_SCENE(ptk_rec_next)
PTK_BY_SCENE(ptk_nee_resolve)
PTK_BY_SCENE(ptk_shade)
PTK_BY_SCENE(ptk_trace_batch)
PTK_BY_SCENE(ptk_wavefront_results)
PTK_BY_SCENE(ptk_light_hooks)
PTK_BY_SCENE(ptk_light_pdf_from)
PTK_BY_SCENE(ptk_gen)
PTK_BY_SCENE(ptk_camera_rays)
#undef PTK_BY_SCENE
// The BSDF hooks hold no analytic-shape code: the first build serves every scene but a Disney one
#define PTK_BY_MATERIAL(fn)                                                                                         \
    template <class... A>                                                                                           \
    static hipError_t fn##_any(const pt_context* ctx, A&&... a) {                                                   \
        if (ctx->fourier_kernels) return ptf::fn(std::forward<A>(a)...);                                            \
        if (ctx->motion_kernels) return ptv::fn(std::forward<A>(a)...);                                             \
        if (ctx->maplight_kernels) return ptm::fn(std::forward<A>(a)...);                                           \
        return ctx->disney_kernels ? ptd::fn(std::forward<A>(a)...) : ::fn(std::forward<A>(a)...);                  \
    }
PTK_BY_MATERIAL(ptk_bsdf_eval)
PTK_BY_MATERIAL(ptk_bsdf_sample)
#undef PTK_BY_MATERIAL

#define PT_HIP(call)                                             \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return ctx->hip_fail(e_, #call);   \
    } while (0)

template <class T>
static pt_status upload(pt_context* ctx, DevBuf& b, const T* src, size_t n) {
    PT_HIP(b.alloc(n * sizeof(T)));
    if (n) PT_HIP(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PT_OK;
}
