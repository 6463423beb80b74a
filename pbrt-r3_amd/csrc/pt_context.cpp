// pt_context.cpp -- host side of libpbrtgpu.so: the C ABI of include/pbrtgpu.h.
//
// Plays the role of pbrt-r3's SceneContext::make_scene + make_integrator
// (src/core/api/scene_context/scene_context.rs:675-729) and of
// SampleIntegratorCore::render (src/core/integrator/sampler.rs:259-325), re-designed as
// a wavefront scheduler: camera samples are generated for a pass of S samples per pixel
// into an SoA path pool in HBM, then every bounce is one traversal launch (continuation
// rays + the previous bounce's shadow / MIS probe rays) and one shading launch; queues are
// compacted on the device and no host synchronisation happens inside a pass except one
// counter read at its end.  There is no CPU rendering path in this library.
// The scene upload (pt_scene_upload and the pt_scene_set_* setters) lives in pt_scene_upload.cpp.
#include "pt_context_impl.h"

namespace {

pt_status ensure_pool(pt_context* ctx, size_t n_paths) {
    if (ctx->sc.n_instances && ctx->d_hit_inst.bytes < std::max(n_paths, ctx->pool_paths) * 4) {      // scenes with object instances only
        PT_HIP(ctx->d_hit_inst.alloc(std::max(n_paths, ctx->pool_paths) * 4));
        ctx->paths.hit_inst = ctx->d_hit_inst.as<uint32_t>();
    }
    const bool tex_split = ctx->sc.textured && !ctx->sc.n_instances;      // k_tex_resolve -> k_shade_general_res: 144 bytes per path, for such scenes only
    if (tex_split && ctx->d_tex_res.bytes < std::max(n_paths, ctx->pool_paths) * (size_t)(PT_TEX_RES_F4 * 16)) {
        PT_HIP(ctx->d_tex_res.alloc(std::max(n_paths, ctx->pool_paths) * (size_t)(PT_TEX_RES_F4 * 16)));
        ctx->paths.tex_res = ctx->d_tex_res.as<float4>();
    } else if (!tex_split && ctx->d_tex_res.p) {
        ctx->d_tex_res.release();
        ctx->paths.tex_res = nullptr;
    }
    if (ctx->pool_paths >= n_paths && ctx->d_pool.p) return PT_OK;
    // 11 float4 + float2 + u64 + 6 x 4-byte + 1 byte per path
    const size_t per_path = 11 * 16 + 8 + 8 + 6 * 4 + 4;
    PT_HIP(ctx->d_pool.alloc(n_paths * per_path + 16384));
    char* base = ctx->d_pool.as<char>();
    size_t off = 0;
    auto carve = [&](size_t elem) { void* p = base + off; off += (n_paths * elem + 255) & ~(size_t)255; return p; };
    PtPaths& P = ctx->paths;
    P.ray_o = (float4*)carve(16); P.ray_d = (float4*)carve(16);
    P.sh_o = (float4*)carve(16); P.sh_d = (float4*)carve(16);
    P.pr_o = (float4*)carve(16); P.pr_d = (float4*)carve(16);
    P.beta = (float4*)carve(16); P.L = (float4*)carve(16);
    P.pendA = (float4*)carve(16); P.pendB = (float4*)carve(16); P.pbeta = (float4*)carve(16);
    P.p_film = (float2*)carve(8);
    P.sobol_index = (uint64_t*)carve(8);
    P.pixel = (uint32_t*)carve(4); P.state = (uint32_t*)carve(4);
    P.hit_t = (float*)carve(4); P.hit_rec = (int32_t*)carve(4);
    P.nee = (uint32_t*)carve(4);
    P.probe_rec = (int32_t*)carve(4);
    P.occluded = (uint8_t*)carve(1);
    if (off > ctx->d_pool.bytes) return ctx->fail(PT_ERR_DEVICE, "internal: path pool carve overflow");
    PT_HIP(ctx->d_qa.alloc(n_paths * 4));
    PT_HIP(ctx->d_qb.alloc(n_paths * 4));
    PT_HIP(ctx->d_qnee.alloc(n_paths * 4));
    PT_HIP(ctx->d_qsorted.alloc(n_paths * 4));
    PT_HIP(ctx->d_qshadow.alloc(n_paths * 4));
    PT_HIP(ctx->d_qprobe.alloc(n_paths * 4));
    ctx->pool_paths = n_paths;
    return PT_OK;
}

hipEvent_t get_event(pt_context* ctx, size_t i) {
    while (ctx->ev.size() <= i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ctx->ev.push_back(e);
    }
    return ctx->ev[i];
}

}  // namespace

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

pt_status pt_context_create(int device, pt_context** out) {
    if (!out) return PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return PT_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return PT_ERR_NO_DEVICE;
    pt_context* ctx = new pt_context;
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return PT_ERR_DEVICE; }
    std::memset(&ctx->sc, 0, sizeof(ctx->sc));
    std::memset(&ctx->info, 0, sizeof(ctx->info));
    std::memset(&ctx->paths, 0, sizeof(ctx->paths));
    // occupancy-sized persistent grids: blocks per CU from register/LDS use x CU count
    ctx->grid_trace = ctx->n_cu * 4;
    ctx->grid_trace_dist = ctx->n_cu * ptk_trace_dist_blocks_per_cu();
    if (const char* e = std::getenv("PBRTGPU_TRACE_BLOCKS_PER_CU")) {
        ctx->grid_trace = ctx->n_cu * std::max(1, std::atoi(e));
        if (!ptk_trace_wide()) ctx->grid_trace_dist = ctx->grid_trace;          // (a PT_TRACE_WIDE build runs one 1024-thread block per CU: sixteen waves, all a CU holds)
    }
    ctx->grid_shade = ctx->n_cu * 2;
    if (const char* e = std::getenv("PBRTGPU_SHADE_BLOCKS_PER_CU")) ctx->grid_shade = ctx->n_cu * std::max(1, std::atoi(e));
    if (const char* e = std::getenv("PBRTGPU_SORT_SHADOW_MIN")) ctx->sort_shadow_min = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("PBRTGPU_SORT_CONT_MIN")) ctx->sort_cont_min = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("PBRTGPU_SORT_CONT")) ctx->sort_cont = std::min(2, std::max(-1, std::atoi(e)));
    if (const char* e = std::getenv("PBRTGPU_TRACE_FAR")) ctx->trace_far = std::atoi(e);
    if (const char* e = std::getenv("PBRTGPU_SHADE_LOCAL")) ctx->shade_local = std::atoi(e);
    ctx->grid_wide = ctx->n_cu * 8;
    // Sobol' tables: $PBRTGPU_DATA_DIR, else <directory of this shared library>/../data
    const char* dd = std::getenv("PBRTGPU_DATA_DIR");
    if (dd) ctx->data_dir = dd;
    else {
        Dl_info di;
        if (dladdr((const void*)&pt_abi_version, &di) && di.dli_fname) {
            std::string so = di.dli_fname;
            size_t slash = so.find_last_of('/');
            ctx->data_dir = (slash == std::string::npos ? std::string(".") : so.substr(0, slash)) + "/../data";
        }
    }
    *out = ctx;
    return PT_OK;
}

void pt_context_destroy(pt_context* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
    if (ctx->h_live) (void)hipHostFree(ctx->h_live);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* pt_last_error(const pt_context* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

pt_status pt_set_data_dir(pt_context* ctx, const char* dir) {
    if (!ctx || !dir) return PT_ERR_INVALID_ARGUMENT;
    ctx->data_dir = dir;
    return PT_OK;
}

pt_status pt_scene_info_get(const pt_context* ctx, pt_scene_info* out) {
    if (!ctx || !out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return PT_ERR_NO_SCENE;
    *out = ctx->info;
    if (ctx->n_fourier_tables) {          // Material "fourier": the samples the kernels turned away at an iteration cap, summed over the tables
        (void)hipSetDevice(ctx->device);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return PT_ERR_DEVICE;
        std::vector<PtFourierTable> tabs(ctx->n_fourier_tables);
        if (hipMemcpy(tabs.data(), ctx->d_fourier.p, tabs.size() * sizeof(PtFourierTable), hipMemcpyDeviceToHost) != hipSuccess) return PT_ERR_DEVICE;
        uint64_t capped = 0;
        for (const PtFourierTable& t : tabs) capped += t.capped;
        out->fourier_capped = (int32_t)std::min<uint64_t>(capped, 0x7fffffffu);
    }
    return PT_OK;
}

pt_status pt_film_clear(pt_context* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    size_t npx = (size_t)ctx->film_w * ctx->film_h;
    PT_HIP(hipMemsetAsync(ctx->d_own.p, 0, npx * 16, ctx->stream));
    PT_HIP(hipMemsetAsync(ctx->d_spillfilm.p, 0, npx * 16, ctx->stream));
    PT_HIP(hipMemsetAsync(ctx->d_xyzw.p, 0, npx * 16, ctx->stream));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    ctx->xyzw_committed = false;
    return PT_OK;
}

// Renders the listed tiles; radiance_out (device, optional) receives per-sample radiance.
// The lazily filled light grid, before a bounce is shaded: the voxels this bounce's hits fall in and nobody has asked for yet get their rows.
// One counter read-back per bounce (scenes with thousands of lights only: the dense grid needs none of this).
static pt_status fill_light_grid(pt_context* ctx, const PtQueues& Q) {
    PtScene& sc = ctx->sc;
    uint32_t* todo = ctx->d_grid_todo.as<uint32_t>();
    uint32_t* todo_count = todo + ctx->grid_nvox;
    PT_HIP(ptk_grid_mark_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, Q, ctx->d_grid_rows.as<int32_t>(), todo, todo_count));
    uint32_t n = 0;
    PT_HIP(hipMemcpyAsync(&n, todo_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    if (n == 0) return PT_OK;
    const size_t row_bytes = (size_t)sc.grid.stride * sizeof(float);
    if (ctx->grid_rows_used + n > ctx->grid_rows_cap) {          // grow the row store (doubling, never past one row per voxel) and move the rows made so far
        size_t cap = ctx->grid_rows_cap;
        while (cap < ctx->grid_rows_used + n) cap *= 2;
        cap = std::min(cap, ctx->grid_nvox);
        void* bigger = nullptr;
        if (hipMalloc(&bigger, cap * row_bytes + 64) != hipSuccess)
            return ctx->fail(PT_ERR_DEVICE, "light grid: no memory for the tables of the voxels this frame visits (" + std::to_string(cap * row_bytes >> 20) + " MiB)");
        PT_HIP(hipMemcpyAsync(bigger, ctx->d_grid.p, ctx->grid_rows_used * row_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        PT_HIP(hipStreamSynchronize(ctx->stream));
        ctx->d_grid.release();
        ctx->d_grid.p = bigger; ctx->d_grid.bytes = cap * row_bytes + 64;
        ctx->grid_rows_cap = cap;
        sc.grid.data = ctx->d_grid.as<float>();
    }
    float* rows = ctx->d_grid.as<float>() + ctx->grid_rows_used * (size_t)sc.grid.stride;
    PT_HIP(ptk_light_grid_any(ctx, ctx->stream, sc, rows, n, todo));
    PT_HIP(ptk_grid_assign(ctx->stream, ctx->d_grid_rows.as<int32_t>(), todo, n, (uint32_t)ctx->grid_rows_used, todo_count));
    ctx->grid_rows_used += n;
    if (std::getenv("PBRTGPU_BUILD_TRACE")) std::fprintf(stderr, "[light grid] %u voxels filled on first touch (%zu of %zu so far, %zu MiB of rows)\n", n, ctx->grid_rows_used, ctx->grid_nvox,
                                                         ctx->grid_rows_used * row_bytes >> 20);
    return PT_OK;
}

static pt_status render_tiles(pt_context* ctx, const pt_tile* tiles, uint32_t n_tiles, float* d_radiance_out) {
    const PtScene& sc = ctx->sc;
    const int32_t* sbnd = sc.film.sample_bounds;
    std::vector<pt_tile> all;
    if (n_tiles == 0 && tiles == nullptr) {      // the reference's 16x16 decomposition (sampler.rs:266-289)
        for (int32_t y = sbnd[1]; y < sbnd[3]; y += 16)
            for (int32_t x = sbnd[0]; x < sbnd[2]; x += 16) {
                pt_tile t = {x, y, std::min(x + 16, sbnd[2]), std::min(y + 16, sbnd[3])};
                all.push_back(t);
            }
        tiles = all.data();
        n_tiles = (uint32_t)all.size();
    }
    // The pass's pixel list is expanded from the tiles on the device (k_expand_tiles); the host only checks the tiles and
    // prefix-sums their sizes.
    std::vector<uint32_t> tile_off(n_tiles);
    size_t n_pixels_total = 0;
    for (uint32_t i = 0; i < n_tiles; i++) {
        const pt_tile& t = tiles[i];
        if (t.x0 < sbnd[0] || t.y0 < sbnd[1] || t.x1 > sbnd[2] || t.y1 > sbnd[3] || t.x1 < t.x0 || t.y1 < t.y0)
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "tile outside the sample bounds");
        tile_off[i] = (uint32_t)n_pixels_total;
        n_pixels_total += (size_t)(t.x1 - t.x0) * (size_t)(t.y1 - t.y0);
        if (n_pixels_total > (size_t)(sbnd[2] - sbnd[0]) * (size_t)(sbnd[3] - sbnd[1])) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "tiles overlap (more pixels than the sample bounds hold)");
    }
    if (n_pixels_total == 0) return PT_OK;
    const uint32_t spp = sc.sobol.spp;

    // Paths in flight per pass.  Every k_trace launch ends with a drain tail (ray lengths are heavy-tailed and a
    // lane sees only a handful of rays per launch), so big launches pay: 4 M paths -> 662 Mrays/s, 64 M -> 850 on
    // RT1M, 192 M (the 256-spp frame in two passes instead of five) 1 037, 288 M (one pass: nine launches of up to 140 M rays) 1 048:
    // 277 M slots are 64 GB of path state, 6.6 GB of queues and 3.3 GB of sort buffers -- HBM3E is 288 GB, and a pool never takes more
    // than half of what is free.
    size_t pool_target = (size_t)288 << 20;
    if (const char* e = std::getenv("PBRTGPU_POOL_PATHS")) pool_target = std::max<size_t>(65536, std::strtoull(e, nullptr, 10));
    pool_target = std::min<size_t>(pool_target, (size_t)1 << 30);      // 32-bit path ids and queue counters with room to spare
    const bool ao = sc.integrator == PT_INTEGRATOR_AO;
    const bool aov = sc.integrator == PT_INTEGRATOR_AOV;
    const bool rec = sc.integrator == PT_INTEGRATOR_DIRECTLIGHTING || sc.integrator == PT_INTEGRATOR_WHITTED;
    // next-event entries per path: Whitted one per light, DirectLighting "one" a single one, "all" one per light sample
    const uint32_t rec_epp = !rec ? 0u : (sc.integrator == PT_INTEGRATOR_DIRECTLIGHTING && sc.direct_strategy == PT_DIRECT_ONE) ? 1u
                             : sc.integrator == PT_INTEGRATOR_WHITTED ? std::max(1u, sc.n_lights) : std::max(1u, ctx->light_samples_total);
    const uint32_t rec_depth = (uint32_t)std::max(1, sc.max_depth);
    const size_t rec_per_path = 64 + (size_t)rec_depth * PT_REC_FRAME_F4 * 16 + (size_t)rec_epp * (6 * 16 + 1 + 4 + 4 + 8);
    {   // never more than half of what the device has free (what this render still has to allocate: a pool or frame store that exists is not counted twice)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            // per path: the pool's eleven float4 and its words, five queues + the sort's lists; textured scenes: the evaluated parameters; large scenes: the
            // continuation sort's lists; the recursive integrators: their frames and next-event entries
            size_t per_path = 11 * 16 + 8 + 8 + 6 * 4 + 4 + 6 * 4 + 4 * 4;
            if (sc.textured && !sc.n_instances) per_path += PT_TEX_RES_F4 * 16;
            if (ctx->sort_cont != 0) per_path += 4 * 4;
            if (rec) {
                // The frame store used to be held under 6 GB whatever the device had: a 64-spp directlighting frame of RT1M then ran as 22 passes of
                // 3 M camera samples, each ending in the traversal kernel's drain tail (5.9 ms launches: 687 Mrays/s where the same kernel does
                // 1 070 on launches of 150 ms).  Now it takes what the pool takes: up to half of the free memory together.
                const size_t have = ctx->pool_paths * per_path + ctx->rec_paths * rec_per_path;      // already allocated: comes back to the budget
                const size_t budget = (free_b + have) / 2;
                pool_target = std::min(pool_target, std::max<size_t>(65536, budget / (per_path + rec_per_path)));
            } else if (ctx->pool_paths < pool_target) {
                pool_target = std::min(pool_target, std::max<size_t>(ctx->pool_paths, std::max<size_t>(1u << 20, (free_b / 2) / per_path)));
            }
        }
    }
    if (rec) pool_target = std::min<size_t>(pool_target, ((size_t)1 << 31) / std::max(1u, rec_epp));      // next-event entries are numbered path x entries-per-path in 32 bits
    if (rec) if (const char* e = std::getenv("PBRTGPU_REC_POOL_BYTES")) pool_target = std::max<size_t>(65536, std::min<size_t>(pool_target, std::strtoull(e, nullptr, 10) / rec_per_path));
    if (ao) pool_target = std::max<size_t>(65536, std::min<size_t>(pool_target, ((size_t)128 << 20) / (size_t)sc.ao_samples));      // <= 128 M occlusion rays (4.4 GB) per pass: big launches amortise the drain tail
    size_t chunk_pix = std::min(n_pixels_total, pool_target);
    uint32_t S = (uint32_t)std::max<size_t>(1, std::min<size_t>(spp, pool_target / chunk_pix));
    {   // equal passes: 256 spp at 63 spp per pass would leave a 4-spp runt
        const uint32_t passes = (spp + S - 1) / S;
        S = (spp + passes - 1) / passes;
    }
    pt_status st;
    if ((st = ensure_pool(ctx, chunk_pix * S)) != PT_OK) return st;
    if (ctx->pixels_cap < n_pixels_total) {
        PT_HIP(ctx->d_pixels.alloc(n_pixels_total * 4));
        ctx->pixels_cap = n_pixels_total;
    }
    {
        const size_t sb_w = (size_t)(sbnd[2] - sbnd[0]), sb_h = (size_t)(sbnd[3] - sbnd[1]);
        const size_t bm_bytes = ((sb_w * sb_h + 31) / 32) * 4;
        if (ctx->d_tilebits.bytes < bm_bytes) PT_HIP(ctx->d_tilebits.alloc(bm_bytes));
        if (ctx->d_tiles.bytes < (size_t)n_tiles * 20) PT_HIP(ctx->d_tiles.alloc((size_t)n_tiles * 20));
        uint32_t* d_off = reinterpret_cast<uint32_t*>(ctx->d_tiles.as<char>() + (size_t)n_tiles * 16);
        PT_HIP(hipMemsetAsync(ctx->d_tilebits.p, 0, bm_bytes, ctx->stream));
        PT_HIP(hipMemsetAsync(ctx->d_err.p, 0, 4, ctx->stream));          // this call's errors only (a sampler hook may have left the Halton bit behind)
        PT_HIP(hipMemcpyAsync(ctx->d_tiles.p, tiles, (size_t)n_tiles * 16, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(hipMemcpyAsync(d_off, tile_off.data(), (size_t)n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ptk_expand_tiles(ctx->stream, ctx->d_tiles.as<int4>(), d_off, n_tiles, sbnd[0], sbnd[1], (uint32_t)sb_w, ctx->d_pixels.as<uint32_t>(),
                                ctx->d_tilebits.as<uint32_t>(), ctx->d_err.as<uint32_t>()));
        uint32_t herr0 = 0;      // pageable source buffers above: the copies have been staged when the calls return; one sync covers the check
        PT_HIP(hipMemcpyAsync(&herr0, ctx->d_err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        PT_HIP(hipStreamSynchronize(ctx->stream));
        if (herr0 & 2u) {
            PT_HIP(hipMemsetAsync(ctx->d_err.p, 0, 4, ctx->stream));
            PT_HIP(hipStreamSynchronize(ctx->stream));
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "tiles overlap: the tiles of one pt_render call must be disjoint");
        }
    }

    PtQueues Q;
    Q.nee = ctx->d_qnee.as<uint32_t>();
    Q.counts = ctx->d_counts.as<uint32_t>();
    Q.sorted = ctx->d_qsorted.as<uint32_t>();
    Q.shadow = ctx->d_qshadow.as<uint32_t>();
    Q.probe = ctx->d_qprobe.as<uint32_t>();
    Q.bin = nullptr;
    if (sc.general_materials) {          // the material sort keeps each entry's bin between its two kernels
        if (ctx->d_qbin.bytes < ctx->pool_paths * 2) PT_HIP(ctx->d_qbin.alloc(ctx->pool_paths * 2));
        Q.bin = ctx->d_qbin.as<uint16_t>();
    }
    Q.shadow_key = nullptr;
    // pt_raysort.hip: a key per shadow ray beside the list (k_shade writes it; k_rec_nee_lists for the recursive integrators, whose lists hold
    // next-event ENTRIES, rec_epp per camera sample), each launch's list is sorted by it
    const bool rec_i = sc.integrator == PT_INTEGRATOR_DIRECTLIGHTING || sc.integrator == PT_INTEGRATOR_WHITTED;
    if (ctx->sort_shadow_min > 0 && (sc.integrator == PT_INTEGRATOR_PATH || rec_i)) {
        const size_t want_cap = rec_i ? chunk_pix * (size_t)S * std::max(1u, rec_epp) : ctx->pool_paths;
        if (ctx->sort_cap < want_cap) {
            const size_t tb = ptk_sort_rays_temp_bytes((uint32_t)want_cap);
            if (tb == 0) return ctx->fail(PT_ERR_DEVICE, "radix sort scratch size query failed");
            PT_HIP(ctx->d_sort_ids.alloc(want_cap * 4));
            PT_HIP(ctx->d_sort_keys[0].alloc(want_cap * 4));
            PT_HIP(ctx->d_sort_keys[1].alloc(want_cap * 4));
            PT_HIP(ctx->d_sort_temp.alloc(tb));
            ctx->sort_cap = want_cap;
        }
        Q.shadow_key = ctx->d_sort_keys[0].as<uint32_t>();
    }
    // Continuation rays in origin order as well, where it pays: once nodes + leaf records outgrow the 256 MiB Infinity Cache the traversal
    // kernel waits on HBM, and rays that start in one cell miss the caches together instead of one by one.
    int sort_cont = ctx->sort_cont;
    if (sort_cont < 0) sort_cont = (ctx->n_nodes_up * sizeof(PtNode) + ctx->n_tris_up * sizeof(PtTri) > ((size_t)256 << 20)) ? 1 : 0;
    if (sc.integrator != PT_INTEGRATOR_PATH) sort_cont = 0;
    if (sort_cont) {
        if (ctx->csort_cap < ctx->pool_paths) {
            const size_t tb = ptk_sort_rays_keep_temp_bytes((uint32_t)ctx->pool_paths);
            if (tb == 0) return ctx->fail(PT_ERR_DEVICE, "radix sort scratch size query failed");
            PT_HIP(ctx->d_csort_ids.alloc(ctx->pool_paths * 4));
            PT_HIP(ctx->d_csort_keys[0].alloc(ctx->pool_paths * 4));
            PT_HIP(ctx->d_csort_keys[1].alloc(ctx->pool_paths * 4));
            PT_HIP(ctx->d_csort_temp.alloc(tb));
            ctx->csort_cap = ctx->pool_paths;
        }
    }
    PtCounters* cnt = ctx->d_counters.as<PtCounters>();
    uint32_t* err = ctx->d_err.as<uint32_t>();
    size_t ev_i = 0;
    std::vector<std::pair<size_t, int>> spans;   // (event index, kind) kind 0 = trace, 1 = shade
    const bool bounce_log = std::getenv("PBRTGPU_BOUNCE_LOG") != nullptr;
    std::vector<std::array<uint32_t, 3>> bounce_counts;
    const bool no_events = std::getenv("PBRTGPU_NO_EVENTS") != nullptr;   // experiment: cost of the per-bounce event records

    hipEvent_t ev_begin = get_event(ctx, ev_i++), ev_end = get_event(ctx, ev_i++);
    PT_HIP(hipEventRecord(ev_begin, ctx->stream));

    for (size_t c0 = 0; c0 < n_pixels_total; c0 += chunk_pix) {
        uint32_t n_pix = (uint32_t)std::min(chunk_pix, n_pixels_total - c0);
        const uint32_t* d_pix = ctx->d_pixels.as<uint32_t>() + c0;
        for (uint32_t s0 = 0; s0 < spp; s0 += S) {
            uint32_t ns = std::min(S, spp - s0);
            uint32_t* qa = ctx->d_qa.as<uint32_t>();
            uint32_t* qb = ctx->d_qb.as<uint32_t>();
            Q.cur = qa; Q.next = qb;
            PT_HIP(ptk_gen_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, Q, d_pix, n_pix, s0, ns, cnt));
            if (ao) {
                // camera rays -> closest hits -> ao_samples occlusion rays per hit (compacted) -> any-hit -> ordered sum
                const uint32_t n_paths = n_pix * ns;
                const size_t cap = (size_t)n_paths * (size_t)sc.ao_samples;
                if (ctx->ao_rays_cap < cap) {      // per ray: origin + t_max, direction (the record of a shadow work item), weight, item id, occlusion flag
                    PT_HIP(ctx->d_ao.alloc(cap * 41 + 256));
                    ctx->ao_rays_cap = cap;
                    PT_HIP(ptk_iota(ctx->stream, ctx->grid_wide, reinterpret_cast<uint32_t*>(ctx->d_ao.as<char>() + ctx->ao_rays_cap * 36), (uint32_t)cap));
                }
                float4* ao_o = ctx->d_ao.as<float4>();
                float4* ao_d = ao_o + ctx->ao_rays_cap;
                float* ao_w = reinterpret_cast<float*>(ao_d + ctx->ao_rays_cap);
                uint32_t* ao_ids = reinterpret_cast<uint32_t*>(ao_w + ctx->ao_rays_cap);
                uint8_t* ao_occ = reinterpret_cast<uint8_t*>(ao_ids + ctx->ao_rays_cap);
                uint32_t* ao_count = ctx->d_ticket.as<uint32_t>() + 2;
                hipEvent_t a = get_event(ctx, ev_i), b = get_event(ctx, ev_i + 1), c = get_event(ctx, ev_i + 2);
                if (!a || !b || !c) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                spans.push_back({ev_i, 0});
                ev_i += 3;
                PT_HIP(hipMemsetAsync(ctx->d_ticket.p, 0, 16, ctx->stream));
                PT_HIP(ptk_ao_tag(ctx->stream, ctx->grid_wide, ctx->paths, n_pix, n_paths, s0));
                PT_HIP(hipEventRecord(a, ctx->stream));
                PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, ctx->paths, Q, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err, 0, ctx->scene_alpha ? 1 : 0));
                ctx->trace_launches++;
                PT_HIP(ptk_ao_rays_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, n_paths, ao_o, ao_d, ao_w, ao_count, cnt));
                {   // the occlusion rays as shadow work items of the wavefront traversal kernel itself (any hit -> occlusion flag);
                    // the item count is read on the device, so the pass never waits for the host
                    PtPaths AP = ctx->paths;
                    AP.sh_o = ao_o; AP.sh_d = ao_d; AP.occluded = ao_occ;
                    PtQueues AQ = Q;
                    AQ.shadow = ao_ids;
                    PT_HIP(ptk_ao_queue(ctx->stream, AQ, ao_count, (uint32_t)sc.ao_samples));
                    PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, AP, AQ, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err, 0, ctx->scene_alpha ? 1 : 0));
                    ctx->trace_launches++;
                }
                PT_HIP(hipEventRecord(b, ctx->stream));
                PT_HIP(ptk_ao_resolve_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, n_paths, ao_w, ao_occ));
                PT_HIP(hipEventRecord(c, ctx->stream));
            } else if (aov) {
                // camera rays -> closest hits -> one field of the interaction per hit
                const uint32_t n_paths = n_pix * ns;
                hipEvent_t a = get_event(ctx, ev_i), b = get_event(ctx, ev_i + 1), c = get_event(ctx, ev_i + 2);
                if (!a || !b || !c) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                spans.push_back({ev_i, 0});
                ev_i += 3;
                PT_HIP(hipEventRecord(a, ctx->stream));
                PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, ctx->paths, Q, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err, 0, ctx->scene_alpha ? 1 : 0));
                ctx->trace_launches++;
                PT_HIP(hipEventRecord(b, ctx->stream));
                PT_HIP(ptk_aov_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, n_paths, ctx->aov_target, ctx->aov_scale, cnt));
                PT_HIP(hipEventRecord(c, ctx->stream));
            } else if (rec) {
                // DirectLighting / Whitted: depth-first walk over the specular trees, two traversal launches per tree level
                const uint32_t n_paths = n_pix * ns;
                // sized by THIS render's largest pass (chunk_pix * S, which the 6 GB bound on pool_target above limits), not by the path
                // pool: the pool never shrinks, and a context that has rendered a 288 M-path frame before would ask for 230 GB here
                const size_t np = chunk_pix * (size_t)S, ne = np * rec_epp;
                if (ctx->rec_paths < np || ctx->rec_epp != rec_epp || ctx->rec_depth != rec_depth || !ctx->d_rec.p) {
                    PT_HIP(ctx->d_rec.alloc(np * rec_per_path + 65536));
                    ctx->rec_paths = np; ctx->rec_epp = rec_epp; ctx->rec_depth = rec_depth;
                    if (!ctx->d_counts2.p) PT_HIP(ctx->d_counts2.alloc(PT_COUNTS_WORDS * 4));
                }
                PT_HIP(hipMemsetAsync(ctx->d_counts2.p, 0, PT_COUNTS_WORDS * 4, ctx->stream));
                PtRec R;
                char* rb = ctx->d_rec.as<char>();
                auto take = [&](size_t bytes) { char* q = rb; rb += (bytes + 255) & ~(size_t)255; return q; };
                R.diff = (float4*)take(np * 64);
                R.frames = (float4*)take(np * (size_t)rec_depth * PT_REC_FRAME_F4 * 16);
                R.sh_o = (float4*)take(ne * 16); R.sh_d = (float4*)take(ne * 16); R.pr_o = (float4*)take(ne * 16); R.pr_d = (float4*)take(ne * 16);
                R.A = (float4*)take(ne * 16); R.B = (float4*)take(ne * 16);
                R.panic = err;
                R.prec = (int32_t*)take(ne * 4); R.flags = (uint32_t*)take(ne * 4);
                uint32_t* nl_shadow = (uint32_t*)take(ne * 4);
                uint32_t* nl_probe = (uint32_t*)take(ne * 4);
                R.occ = (uint8_t*)take(ne);
                R.n_paths = (uint32_t)np; R.max_depth = rec_depth; R.epp = rec_epp;
                R.n_arrays = (sc.integrator == PT_INTEGRATOR_DIRECTLIGHTING && sc.direct_strategy == PT_DIRECT_ALL) ? 2u * sc.n_lights * (uint32_t)std::max(sc.max_depth, 0) : 0u;
                R.s0 = s0; R.n_pix = n_pix;
                if (5u + 2u * R.n_arrays > 60000u) return ctx->fail(PT_ERR_UNSUPPORTED, "directlighting \"all\": too many lights x maxdepth for the sampler's array dimensions");
                PtPaths NP = ctx->paths;             // the node's next-event rays as shadow / probe work items
                NP.sh_o = R.sh_o; NP.sh_d = R.sh_d; NP.pr_o = R.pr_o; NP.pr_d = R.pr_d; NP.occluded = R.occ; NP.probe_rec = R.prec;
                PtQueues Qn = Q;
                Qn.counts = ctx->d_counts2.as<uint32_t>(); Qn.shadow = nl_shadow; Qn.probe = nl_probe;
                PT_HIP(ptk_rec_init_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, R, n_paths));
                // The walk ends when no camera sample is live.  That count comes back through page-locked memory ONE LEVEL BEHIND: level i + 1 is
                // queued before the host looks at level i's count, so the device never waits for the host (a level launched after the last one
                // finds empty lists and does nothing).
                if (!ctx->h_live) PT_HIP(hipHostMalloc((void**)&ctx->h_live, 64));
                hipEvent_t rb_ev[2] = {get_event(ctx, ev_i), get_event(ctx, ev_i + 1)};
                if (!rb_ev[0] || !rb_ev[1]) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                ev_i += 2;
                for (uint32_t iter = 0; iter < 100000u; iter++) {
                    hipEvent_t a = get_event(ctx, ev_i), b = get_event(ctx, ev_i + 1), c = get_event(ctx, ev_i + 2);
                    if (!a || !b || !c) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                    if (ev_i < 3000) { spans.push_back({ev_i, 0}); ev_i += 3; }
                    Qn.cur = Q.cur;
                    PT_HIP(hipEventRecord(a, ctx->stream));
                    PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, ctx->paths, Q, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err, 0, ctx->scene_alpha ? 1 : 0));
                    PT_HIP(ptk_prep(ctx->stream, Qn, 0));
                    PT_HIP(ptk_rec_enter_any(ctx, ctx->stream, ctx->grid_shade, sc, ctx->paths, Q, Qn, R, cnt, rec_epp));
                    PtQueues Qt = Qn;
                    if (Qn.shadow_key) {
                        // The node's shadow rays start at the hit points of this level -- scattered through a scene of small triangles -- and head for the
                        // lights: ordered by origin cell and direction octant like the path integrator's (pt_raysort.hip).  Costs this level one
                        // counter read-back; only the work list moves (results are written per entry).
                        uint32_t n_sh = 0;
                        PT_HIP(hipMemcpyAsync(&n_sh, Qn.counts + PT_Q_SHADOW, 4, hipMemcpyDeviceToHost, ctx->stream));
                        PT_HIP(hipStreamSynchronize(ctx->stream));
                        if (n_sh >= (uint32_t)ctx->sort_shadow_min) {
                            uint32_t* sorted = nullptr;
                            PT_HIP(ptk_sort_shadow_rays(ctx->stream, Qn.shadow, ctx->d_sort_ids.as<uint32_t>(), ctx->d_sort_keys[0].as<uint32_t>(),
                                                        ctx->d_sort_keys[1].as<uint32_t>(), ctx->d_sort_temp.p, ctx->d_sort_temp.bytes, n_sh, &sorted));
                            Qt.shadow = sorted;
                        }
                    }
                    PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, NP, Qt, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err, 0, ctx->scene_alpha ? 1 : 0));
                    ctx->trace_launches += 2;
                    PT_HIP(hipEventRecord(b, ctx->stream));
                    PT_HIP(ptk_rec_next_any(ctx, ctx->stream, ctx->grid_shade, sc, ctx->paths, Q, R));
                    PT_HIP(ptk_prep(ctx->stream, Q, 1));
                    PT_HIP(hipEventRecord(c, ctx->stream));
                    std::swap(Q.cur, Q.next);
                    PT_HIP(hipMemcpyAsync(&ctx->h_live[iter & 1u], Q.counts + PT_Q_CUR, 4, hipMemcpyDeviceToHost, ctx->stream));
                    PT_HIP(hipEventRecord(rb_ev[iter & 1u], ctx->stream));
                    if (iter >= 1u) {
                        PT_HIP(hipEventSynchronize(rb_ev[(iter - 1u) & 1u]));
                        if (ctx->h_live[(iter - 1u) & 1u] == 0) { ctx->trace_launches -= 2; break; }      // the level just queued is an empty one
                    }
                }
            } else if (sc.n_lights > 0) {          // no lights: li() returns zero immediately (path.rs:71-74)
                uint32_t* shadow_sorted = nullptr;          // the ordered shadow list for the next traversal launch, if one was made
                uint32_t* cont_sorted = nullptr;            // the ordered copy of cur for the next traversal launch (sort_cont == 1)
                uint32_t* cont_spare = ctx->d_csort_ids.as<uint32_t>();
                // Which traversal kernel: k_trace_far (nodes fetched by lane pairs) only pays where rays miss the caches -- 16 M sparse triangles +15 %, but
                // 8 M triangles whose rays end early -12 %, RT1M -4 % -- and neither the scene's size nor its depth tells the two apart.  So a scene larger than
                // the Infinity Cache decides by trial: its first incoherent bounce after an upload (bounce 1 of the first pass: the largest one) is
                // traced twice, by each kernel, on the same lists; results are identical (the second launch rewrites them), the counters are put back.
                const char* far_min_env = std::getenv("PBRTGPU_TRACE_FAR_MIN_BYTES");          // (tests: the trial on small scenes)
                const size_t far_min_bytes = far_min_env ? (size_t)std::strtoull(far_min_env, nullptr, 10) : ((size_t)256 << 20);
                // (a scene with alpha masks runs k_trace_alpha for every ray: no far trial, PBRTGPU_TRACE_FAR ignored)
                const bool far_able = !ctx->scene_alpha && ptk_trace_has_far(sc) && ctx->n_nodes_up * sizeof(PtNode) + ctx->n_tris_up * sizeof(PtTri) > far_min_bytes;
                if (ctx->trace_far >= 0 || !far_able) ctx->trace_far_choice = (ctx->trace_far > 0 && ptk_trace_has_far(sc) && !ctx->scene_alpha) ? 1 : 0;
                int bounce_i = 0;
                PtQueues Q_last_trace = Q;
                auto trace = [&]() -> hipError_t {
                    PtQueues Qt = Q;
                    if (shadow_sorted) Qt.shadow = shadow_sorted;
                    shadow_sorted = nullptr;
                    if (cont_sorted) Qt.cur = cont_sorted;
                    cont_sorted = nullptr;
                    Q_last_trace = Qt;
                    return ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, ctx->paths, Qt, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err,
                                     ctx->trace_far_choice > 0 ? 1 : 0, ctx->scene_alpha ? 1 : 0);
                };
                auto far_trial = [&](hipEvent_t near_a, hipEvent_t near_b) -> pt_status {      // right after bounce 1's launch by k_trace (timed by near_a .. near_b)
                    hipEvent_t fa = get_event(ctx, ev_i), fb = get_event(ctx, ev_i + 1);
                    if (!fa || !fb) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                    ev_i += 2;
                    if (!ctx->d_cnt_save.p) PT_HIP(ctx->d_cnt_save.alloc(sizeof(PtCounters)));
                    PT_HIP(hipMemcpyAsync(ctx->d_cnt_save.p, cnt, sizeof(PtCounters), hipMemcpyDeviceToDevice, ctx->stream));
                    PT_HIP(hipMemsetAsync(Q.counts + PT_Q_SEG_TICKET0, 0, 8u * 32u * 4u, ctx->stream));          // the launch's work tickets
                    PT_HIP(hipEventRecord(fa, ctx->stream));
                    PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, sc, ctx->paths, Q_last_trace, cnt, ctx->d_spill.as<uint32_t>(), ctx->spill_depth, err, 1, 0));
                    PT_HIP(hipEventRecord(fb, ctx->stream));
                    PT_HIP(hipMemcpyAsync(cnt, ctx->d_cnt_save.p, sizeof(PtCounters), hipMemcpyDeviceToDevice, ctx->stream));
                    PT_HIP(hipStreamSynchronize(ctx->stream));
                    float near_ms = 0, far_ms = 0;
                    PT_HIP(hipEventElapsedTime(&near_ms, near_a, near_b));
                    PT_HIP(hipEventElapsedTime(&far_ms, fa, fb));
                    ctx->trace_far_choice = far_ms < 0.97f * near_ms ? 1 : 0;          // (a tie stays with the kernel everybody else runs)
                    if (std::getenv("PBRTGPU_BUILD_TRACE")) std::fprintf(stderr, "[trace] trial on bounce 1: k_trace %.2f ms, k_trace_far %.2f ms -> %s\n", near_ms, far_ms, ctx->trace_far_choice ? "k_trace_far" : "k_trace");
                    return PT_OK;
                };
                // after a bounce's shading: order its shadow rays by where they start (pt_raysort.hip); costs one counter read-back
                auto sort_shadow = [&]() -> pt_status {
                    if (!Q.shadow_key && !sort_cont) return PT_OK;
                    uint32_t qc[PT_Q_SHADOW + 1];             // one read-back: the next bounce's continuation rays (prep has moved next to cur) and its shadow rays
                    qc[PT_Q_SHADOW] = 0;
                    PT_HIP(hipMemcpyAsync(qc, Q.counts, Q.shadow_key ? sizeof(qc) : 4 * (PT_Q_CUR + 1u), hipMemcpyDeviceToHost, ctx->stream));      // (the shadow list unsorted: the first word alone)
                    PT_HIP(hipStreamSynchronize(ctx->stream));
                    const uint32_t n_sh = qc[PT_Q_SHADOW], n_next = qc[PT_Q_CUR];
                    if (sort_cont && n_next >= (uint32_t)ctx->sort_cont_min) {
                        // Q.next holds the list k_shade has just written: its rays' keys, then the ordered copy into the spare list
                        PT_HIP(ptk_cont_keys(ctx->stream, ctx->grid_wide, sc, ctx->paths, Q.next, n_next, ctx->d_csort_keys[0].as<uint32_t>()));
                        PT_HIP(ptk_sort_rays_keep(ctx->stream, Q.next, cont_spare, ctx->d_csort_keys[0].as<uint32_t>(), ctx->d_csort_keys[1].as<uint32_t>(),
                                                  ctx->d_csort_temp.p, ctx->d_csort_temp.bytes, n_next));
                        if (sort_cont == 2) std::swap(Q.next, cont_spare);      // shading walks the ordered list too; the old list is the spare now
                        else cont_sorted = cont_spare;
                    }
                    if (!Q.shadow_key || n_sh < (uint32_t)ctx->sort_shadow_min) return PT_OK;
                    PT_HIP(ptk_sort_shadow_rays(ctx->stream, Q.shadow, ctx->d_sort_ids.as<uint32_t>(), ctx->d_sort_keys[0].as<uint32_t>(),
                                                ctx->d_sort_keys[1].as<uint32_t>(), ctx->d_sort_temp.p, ctx->d_sort_temp.bytes, n_sh, &shadow_sorted));
                    return PT_OK;
                };
                auto bounce = [&]() -> pt_status {
                    const bool timed = !no_events;
                    hipEvent_t a = nullptr, b = nullptr, c = nullptr;
                    if (bounce_log) {          // diagnostic (PBRTGPU_BOUNCE_LOG): queue sizes going into this bounce; costs a sync per bounce
                        uint32_t qc[PT_Q_PROBE + 1];
                        PT_HIP(hipMemcpyAsync(qc, Q.counts, sizeof(qc), hipMemcpyDeviceToHost, ctx->stream));
                        PT_HIP(hipStreamSynchronize(ctx->stream));
                        bounce_counts.push_back({qc[PT_Q_CUR], qc[PT_Q_SHADOW], qc[PT_Q_PROBE]});
                    }
                    if (timed) {
                        a = get_event(ctx, ev_i); b = get_event(ctx, ev_i + 1); c = get_event(ctx, ev_i + 2);
                        if (!a || !b || !c) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                        spans.push_back({ev_i, 0});
                        ev_i += 3;
                        PT_HIP(hipEventRecord(a, ctx->stream));
                    }
                    const bool trial = ctx->trace_far_choice < 0 && bounce_i == 1;
                    hipEvent_t ta = a, tb = b;
                    if (trial && !timed) {
                        ta = get_event(ctx, ev_i); tb = get_event(ctx, ev_i + 1);
                        if (!ta || !tb) return ctx->fail(PT_ERR_DEVICE, "hipEventCreate failed");
                        ev_i += 2;
                        PT_HIP(hipEventRecord(ta, ctx->stream));
                    }
                    PT_HIP(trace());
                    if (timed || trial) PT_HIP(hipEventRecord(tb, ctx->stream));
                    if (trial) {
                        const pt_status ts = far_trial(ta, tb);
                        if (ts != PT_OK) return ts;
                    }
                    bounce_i++;
                    PT_HIP(ptk_nee_resolve_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, Q));
                    ctx->trace_launches++;
                    PT_HIP(ptk_prep(ctx->stream, Q, 0));
                    if (ctx->grid_lazy) {
                        const pt_status gs = fill_light_grid(ctx, Q);
                        if (gs != PT_OK) return gs;
                    }
                    PT_HIP(ptk_shade_any(ctx, ctx->stream, ctx->grid_shade, ctx->sc, ctx->paths, Q, cnt, ctx->shade_local < 0 ? ((ctx->scene_has_lobe_materials && !ctx->sc.textured) ? 1 : 0) : ctx->shade_local));
                    PT_HIP(ptk_prep(ctx->stream, Q, 1));
                    {
                        const pt_status ss = sort_shadow();
                        if (ss != PT_OK) return ss;
                    }
                    if (timed) PT_HIP(hipEventRecord(c, ctx->stream));
                    std::swap(Q.cur, Q.next);
                    return PT_OK;
                };
                for (int b = 0; b <= sc.max_depth; b++)
                    if ((st = bounce()) != PT_OK) return st;
                // paths can outlive max_depth+1 iterations only by passing through material-less
                // surfaces; the last SHADE may also have queued NEE work.  One counter read per pass.
                for (;;) {
                    uint32_t counts[PT_Q_NEE + 1];
                    PT_HIP(hipMemcpyAsync(counts, Q.counts, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
                    PT_HIP(hipStreamSynchronize(ctx->stream));
                    if (counts[PT_Q_CUR] == 0 && counts[PT_Q_NEE] == 0) break;
                    if (counts[PT_Q_CUR] == 0) {     // only NEE resolves left
                        PT_HIP(trace());
                        PT_HIP(ptk_nee_resolve_any(ctx, ctx->stream, ctx->grid_wide, sc, ctx->paths, Q));
                        ctx->trace_launches++;
                        PT_HIP(ptk_prep(ctx->stream, Q, 0));
                    } else if ((st = bounce()) != PT_OK) return st;
                }
            }
            PT_HIP(ptk_film(ctx->stream, ctx->grid_wide, sc, ctx->paths, d_pix, n_pix, ns, ctx->d_own.as<float4>(), ctx->d_spillfilm.as<float4>(),
                            d_radiance_out ? d_radiance_out + (size_t)c0 * spp * 3 : nullptr, s0, spp));
        }
    }
    PT_HIP(hipEventRecord(ev_end, ctx->stream));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t herr = 0;
    PT_HIP(hipMemcpy(&herr, err, 4, hipMemcpyDeviceToHost));
    if (herr) {
        PT_HIP(hipMemsetAsync(err, 0, 4, ctx->stream));
        PT_HIP(hipStreamSynchronize(ctx->stream));
        if (herr & 1u) return ctx->fail(PT_ERR_DEVICE, "traversal stack overflow (BVH deeper than the computed bound)");
        return ctx->fail(PT_ERR_UNSUPPORTED, "a path asked the Halton sampler for more than its 1000 dimensions: the reference panics there (halton.rs:103-107); "
                                             "lower maxdepth or use the Sobol' sampler");
    }
#ifdef PT_PROFILE_PHASES
    {   // diagnostic build (tools/tune_trace.sh "prof:-DPT_PROFILE_PHASES:3"): where a traversal wave's clocks go (the slots: PhaseProf in pt_kernels.hip;
        // a node round's "issue" and "wait" were the staged node fetch's halves and read 0: the slots keep their numbers so that profiles/r05, r06 stay comparable)
        unsigned long long pr[24];
        PT_HIP(hipMemcpy(pr, ctx->d_spill.p, sizeof(pr), hipMemcpyDeviceToHost));
        PT_HIP(hipMemsetAsync(ctx->d_spill.p, 0, sizeof(pr), ctx->stream)); PT_HIP(hipStreamSynchronize(ctx->stream));
        const double tot = (double)pr[11];
        std::fprintf(stderr, "[phases] wave clocks %.3e | node rounds %llu (%.1f lanes): issue %.1f%% wait %.1f%% finish %.1f%% = %.0f clk/round | leaf rounds %llu (%.1f items): issue %.1f%% wait %.1f%% finish %.1f%% = %.0f clk/round | general visits %llu: %.1f%% | service %.1f%%\n",
                     tot, pr[3], pr[3] + pr[13] ? (double)pr[4] / (double)(pr[3] + pr[13]) : 0.0, 100.0 * pr[0] / tot, 100.0 * pr[1] / tot, 100.0 * pr[2] / tot,
                     pr[3] ? (double)(pr[0] + pr[1] + pr[2]) / (double)pr[3] : 0.0, pr[8], pr[8] ? (double)pr[9] / (double)pr[8] : 0.0, 100.0 * pr[5] / tot, 100.0 * pr[6] / tot,
                     100.0 * pr[7] / tot, pr[8] ? (double)(pr[5] + pr[6] + pr[7]) / (double)pr[8] : 0.0, pr[13], 100.0 * pr[12] / tot, 100.0 * pr[10] / tot);
        std::fprintf(stderr, "[phases] service in parts: prefetch state machine %.1f%%, retiring + handing out rays %.1f%% (%.0f + %.0f clocks per iteration)\n", 100.0 * pr[14] / tot,
                     100.0 * pr[15] / tot, (double)pr[14] / (double)(pr[3] + pr[8] + pr[13] + 1), (double)pr[15] / (double)(pr[3] + pr[8] + pr[13] + 1));
        // The counter's own cost: an empty timed section (two reads back to back, every 64th iteration) is taken off each section, once per iteration.
        const double iters = (double)pr[16] + 1.0, empty = pr[19] ? (double)pr[20] / (double)pr[19] : 0.0, n_ho = (double)pr[17], n_no = iters - n_ho;
        std::fprintf(stderr, "[phases] loop iterations %llu (%.2f node rounds per pass with one), empty timed section %.0f clocks; less that: prefetch state machine %.0f clocks per iteration = %.1f%%, "
                     "retiring + handing out %.0f = %.1f%%; iterations with a hand-out %.1f%%: %.0f clocks each, without: %.0f clocks each = %.1f%% of wave clocks\n",
                     pr[16], (double)pr[3] / (double)(pr[16] - pr[8] - pr[13] + 1), empty, (double)pr[14] / iters - empty, 100.0 * ((double)pr[14] - empty * iters) / tot,
                     (double)pr[15] / iters - empty, 100.0 * ((double)pr[15] - empty * iters) / tot, 100.0 * n_ho / iters, n_ho > 0 ? (double)pr[18] / n_ho - empty : 0.0,
                     n_no > 0 ? ((double)pr[15] - (double)pr[18]) / n_no - empty : 0.0, 100.0 * ((double)pr[15] - (double)pr[18] - empty * n_no) / tot);
    }
#endif
    {   // diagnostic build -DPT_PROFILE_SHADE: where a shading wave's clocks go
        unsigned long long sp[16];
        if (ctx->fourier_kernels ? ptf::ptk_shade_prof_read(sp) : ctx->motion_kernels ? ptv::ptk_shade_prof_read(sp) : ctx->maplight_kernels ? ptm::ptk_shade_prof_read(sp) : ctx->disney_kernels ? ptd::ptk_shade_prof_read(sp) : ctx->quadric_kernels ? ptq::ptk_shade_prof_read(sp) : ptk_shade_prof_read(sp)) {       // (each set of kernels counts into its own g_shade_prof)
            double tot = 0;
            for (int k = 0; k < 16; k++) if (k != 12) tot += (double)sp[k];
            static const char* names[16] = {"surface", "emit+bsdf setup", "grid+pick light", "u_light,u_scat", "light sample+f", "bsdf MIS+probe", "pend stores",
                                            "u continuation", "continuation", "compaction", "sample tables", "ticket", "", "wait list[item]", "wait path state", "wait record+index"};
            std::fprintf(stderr, "[shade phases] %llu iterations of 64 paths, %.0f clocks each:", sp[12], sp[12] ? tot / (double)sp[12] : 0.0);
            for (int k = 0; k < 16; k++) if (k != 12 && sp[k]) std::fprintf(stderr, " %s %.1f%%", names[k], 100.0 * (double)sp[k] / tot);
            std::fprintf(stderr, "\n");
        }
    }
    float ms = 0;
    PT_HIP(hipEventElapsedTime(&ms, ev_begin, ev_end));
    ctx->render_ms += ms;
    size_t span_i = 0;
    for (auto& sp : spans) {
        float t_ms = 0, s_ms = 0;
        PT_HIP(hipEventElapsedTime(&t_ms, ctx->ev[sp.first], ctx->ev[sp.first + 1]));
        PT_HIP(hipEventElapsedTime(&s_ms, ctx->ev[sp.first + 1], ctx->ev[sp.first + 2]));
        ctx->trace_ms += t_ms;
        ctx->shade_ms += s_ms;
        if (bounce_log && span_i < bounce_counts.size()) {
            const auto& q = bounce_counts[span_i];
            std::fprintf(stderr, "[bounce %zu] rays: %u continuation + %u shadow + %u probe | trace %.3f ms (%.1f Mrays/s) | resolve + shade %.3f ms (%.2f ns per shaded path)\n", span_i, q[0],
                         q[1], q[2], t_ms, ((double)q[0] + q[1] + q[2]) / (t_ms * 1e3), s_ms, q[0] ? s_ms * 1e6 / q[0] : 0.0);
        }
        span_i++;
    }
    ctx->xyzw_committed = false;
    return PT_OK;
}

pt_status pt_render(pt_context* ctx, const pt_tile* tiles, uint32_t n_tiles) {
    if (!ctx || (n_tiles > 0 && !tiles)) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    return render_tiles(ctx, tiles, n_tiles, nullptr);
}

static pt_status film_to_xyzw(pt_context* ctx) {
    if (ctx->xyzw_committed) return PT_OK;
    uint32_t n = ctx->film_w * ctx->film_h;
    PT_HIP(ptk_film_xyzw(ctx->stream, ctx->d_own.as<float4>(), ctx->d_spillfilm.as<float4>(), ctx->d_xyzw.as<float4>(), n));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

pt_status pt_film_download_xyzw(pt_context* ctx, float* out) {
    if (!ctx || !out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    pt_status st = film_to_xyzw(ctx);
    if (st != PT_OK) return st;
    PT_HIP(hipMemcpy(out, ctx->d_xyzw.p, (size_t)ctx->film_w * ctx->film_h * 16, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_film_device_xyzw(pt_context* ctx, void** dev_ptr, size_t* n_floats) {
    if (!ctx || !dev_ptr || !n_floats) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    pt_status st = film_to_xyzw(ctx);
    if (st != PT_OK) return st;
    *dev_ptr = ctx->d_xyzw.p;
    *n_floats = (size_t)ctx->film_w * ctx->film_h * 4;
    return PT_OK;
}

pt_status pt_film_commit_xyzw(pt_context* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    ctx->xyzw_committed = true;
    return PT_OK;
}

// The exchange step without a collective: add another rank's film, handed over in host memory (a host whose ranks talk through MPI or
// shared memory rather than RCCL; two contexts on one device, which RCCL refuses to put in one communicator).
pt_status pt_film_add_xyzw(pt_context* ctx, const float* xyzw) {
    if (!ctx || !xyzw) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    pt_status st = film_to_xyzw(ctx);
    if (st != PT_OK) return st;
    const uint32_t n = ctx->film_w * ctx->film_h;
    DevBuf other;
    PT_HIP(other.alloc((size_t)n * 16));
    PT_HIP(hipMemcpyAsync(other.p, xyzw, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    PT_HIP(ptk_film_add(ctx->stream, ctx->d_xyzw.as<float4>(), other.as<float4>(), n));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    ctx->xyzw_committed = true;
    return PT_OK;
}

// The path's one exchange step, inside the library: sum the per-rank XYZW films over an RCCL communicator the caller owns
// (Film::merge_film_tile across GPUs, film.rs:219-241).  librccl is looked up at run time -- first the copy already mapped into
// the process (the communicator must come from that very copy: a torch process carries its own), else the system's.
}  // extern "C"
namespace {
struct RcclApi {
    int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t) = nullptr;
    const char* (*error_string)(int) = nullptr;
};
// Resolved once, by whichever thread asks first: `pbrt_gpu --gpus N` calls pt_film_allreduce from N host threads at the same time, and a
// thread that saw a half-filled table would skip the collective its peers are already blocked in.  (A function-local static's
// initialiser runs under the language's own once-guard.)
const RcclApi& rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
        a.all_reduce = reinterpret_cast<decltype(a.all_reduce)>(dlsym(h, "ncclAllReduce"));
        a.reduce = reinterpret_cast<decltype(a.reduce)>(dlsym(h, "ncclReduce"));
        a.error_string = reinterpret_cast<decltype(a.error_string)>(dlsym(h, "ncclGetErrorString"));
        return a;
    }();
    return api;
}
}  // namespace
extern "C" {

pt_status pt_film_allreduce(pt_context* ctx, void* nccl_comm, int root) {
    if (!ctx || !nccl_comm) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    const RcclApi& api = rccl_api();
    if (!api.all_reduce || !api.reduce) return ctx->fail(PT_ERR_UNSUPPORTED, "librccl.so.1 (ncclAllReduce / ncclReduce) not found");
    pt_status st = film_to_xyzw(ctx);
    if (st != PT_OK) return st;
    const size_t n = (size_t)ctx->film_w * ctx->film_h * 4;
    const int kFloat = 7, kSum = 0;          // ncclFloat32, ncclSum (rccl.h)
    int rc = root < 0 ? api.all_reduce(ctx->d_xyzw.p, ctx->d_xyzw.p, n, kFloat, kSum, nccl_comm, ctx->stream)
                      : api.reduce(ctx->d_xyzw.p, ctx->d_xyzw.p, n, kFloat, kSum, root, nccl_comm, ctx->stream);
    if (rc != 0) return ctx->fail(PT_ERR_DEVICE, std::string("RCCL: ") + (api.error_string ? api.error_string(rc) : "error"));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    ctx->xyzw_committed = true;
    return PT_OK;
}

pt_status pt_film_resolve_rgb(pt_context* ctx, float* rgb_out) {
    if (!ctx || !rgb_out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    pt_status st = film_to_xyzw(ctx);
    if (st != PT_OK) return st;
    uint32_t n = ctx->film_w * ctx->film_h;
    PT_HIP(ptk_film_rgb(ctx->stream, ctx->d_xyzw.as<float4>(), ctx->d_rgb.as<float>(), n, ctx->sc.film.scale));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    PT_HIP(hipMemcpy(rgb_out, ctx->d_rgb.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    return PT_OK;
}

// time: a time per ray (pt_trace_closest_time / pt_trace_any_time), read by a scene with a moving instance; nullptr: every ray at time 0
static pt_status trace_batch(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, pt_hit* out, uint8_t* occ, int any_hit, const float* time = nullptr) {
    if (!ctx || !o || !d || !tmax || (!any_hit && !out) || (any_hit && !occ)) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return PT_OK;
    (void)hipSetDevice(ctx->device);
    DevBuf d_o, d_d, d_t, d_out;
    PT_HIP(d_o.alloc((size_t)n * 12)); PT_HIP(d_d.alloc((size_t)n * 12)); PT_HIP(d_t.alloc((size_t)n * 4));
    PT_HIP(d_out.alloc((size_t)n * (any_hit ? 1 : sizeof(pt_hit))));
    PT_HIP(hipMemcpy(d_o.p, o, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_d.p, d, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_t.p, tmax, (size_t)n * 4, hipMemcpyHostToDevice));
    PT_HIP(hipMemsetAsync(ctx->d_ticket.p, 0, 16, ctx->stream));
    hipEvent_t a = get_event(ctx, 0), b = get_event(ctx, 1);
    DevBuf d_time;
    const bool timed = time && ctx->motion_instances;
    if (timed) {
        PT_HIP(d_time.alloc((size_t)n * 4));
        PT_HIP(hipMemcpy(d_time.p, time, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    PT_HIP(hipEventRecord(a, ctx->stream));
    if (timed)
        PT_HIP(ptv::ptk_trace_batch_time(ctx->stream, ctx->grid_trace, ctx->sc, n, d_o.as<float>(), d_d.as<float>(), d_t.as<float>(), d_time.as<float>(),
                                         any_hit ? nullptr : d_out.as<pt_hit>(), any_hit ? d_out.as<uint8_t>() : nullptr, any_hit, ctx->d_ticket.as<uint32_t>(),
                                         ctx->d_counters.as<PtCounters>(), ctx->d_spill.as<uint32_t>(), ctx->spill_depth, ctx->d_err.as<uint32_t>(), ctx->scene_alpha ? 1 : 0));
    else
    PT_HIP(ptk_trace_batch_any(ctx, ctx->stream, ctx->grid_trace, ctx->sc, n, d_o.as<float>(), d_d.as<float>(), d_t.as<float>(), any_hit ? nullptr : d_out.as<pt_hit>(),
                           any_hit ? d_out.as<uint8_t>() : nullptr, any_hit, ctx->d_ticket.as<uint32_t>(), ctx->d_counters.as<PtCounters>(),
                           ctx->d_spill.as<uint32_t>(), ctx->spill_depth, ctx->d_err.as<uint32_t>(), ctx->scene_alpha ? 1 : 0));
    PT_HIP(hipEventRecord(b, ctx->stream));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    PT_HIP(hipEventElapsedTime(&ms, a, b));
    ctx->trace_ms += ms;
    ctx->trace_launches++;
    uint32_t herr = 0;
    PT_HIP(hipMemcpy(&herr, ctx->d_err.p, 4, hipMemcpyDeviceToHost));
    if (herr) { PT_HIP(hipMemsetAsync(ctx->d_err.p, 0, 4, ctx->stream)); PT_HIP(hipStreamSynchronize(ctx->stream)); return ctx->fail(PT_ERR_DEVICE, "traversal stack overflow"); }
    if (any_hit) PT_HIP(hipMemcpy(occ, d_out.p, n, hipMemcpyDeviceToHost));
    else PT_HIP(hipMemcpy(out, d_out.p, (size_t)n * sizeof(pt_hit), hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_trace_closest(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, pt_hit* out) {
    return trace_batch(ctx, n, o, d, tmax, out, nullptr, 0);
}
pt_status pt_trace_any(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, uint8_t* occluded_out) {
    return trace_batch(ctx, n, o, d, tmax, nullptr, occluded_out, 1);
}
pt_status pt_trace_closest_time(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const float* time, pt_hit* out) {
    if (!time) return PT_ERR_INVALID_ARGUMENT;
    return trace_batch(ctx, n, o, d, tmax, out, nullptr, 0, time);
}
pt_status pt_trace_any_time(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const float* time, uint8_t* occluded_out) {
    if (!time) return PT_ERR_INVALID_ARGUMENT;
    return trace_batch(ctx, n, o, d, tmax, nullptr, occluded_out, 1, time);
}

// Caller rays through the kernel the renderer itself traces with (see k_wavefront_results): ray i becomes path slot i; the
// continuation / shadow / probe queues list the rays of each kind in caller order, exactly the mix one bounce launches.
static pt_status trace_wavefront(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const float* time, const uint8_t* kind, pt_hit* out,
                                 uint8_t* occluded_out);
pt_status pt_trace_wavefront(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const uint8_t* kind, pt_hit* out,
                             uint8_t* occluded_out) {
    return trace_wavefront(ctx, n, o, d, tmax, nullptr, kind, out, occluded_out);
}
pt_status pt_trace_wavefront_time(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const float* time, const uint8_t* kind,
                                  pt_hit* out, uint8_t* occluded_out) {
    if (!time) return PT_ERR_INVALID_ARGUMENT;
    return trace_wavefront(ctx, n, o, d, tmax, time, kind, out, occluded_out);
}
// (time: the w lane of a ray's direction, which only the motion build reads; nullptr: time 0)
static pt_status trace_wavefront(pt_context* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const float* time, const uint8_t* kind, pt_hit* out,
                                 uint8_t* occluded_out) {
    if (!ctx || !o || !d || !tmax || !kind || !out || !occluded_out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return PT_OK;
    (void)hipSetDevice(ctx->device);
    std::vector<float> o4((size_t)n * 4), d4((size_t)n * 4);
    std::vector<uint32_t> ids[3];
    for (uint32_t i = 0; i < n; i++) {
        if (kind[i] < 1 || kind[i] > 3) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "ray kind must be 1 (continuation), 2 (shadow) or 3 (probe)");
        ids[kind[i] - 1].push_back(i);
        for (int k = 0; k < 3; k++) { o4[4 * (size_t)i + k] = o[3 * (size_t)i + k]; d4[4 * (size_t)i + k] = d[3 * (size_t)i + k]; }
        o4[4 * (size_t)i + 3] = tmax[i];
        d4[4 * (size_t)i + 3] = time ? time[i] : 0.0f;
    }
    pt_status st;
    if ((st = ensure_pool(ctx, std::max<size_t>(n, 65536))) != PT_OK) return st;
    const PtPaths& P = ctx->paths;
    float4* const dst_o[3] = {P.ray_o, P.sh_o, P.pr_o};
    float4* const dst_d[3] = {P.ray_d, P.sh_d, P.pr_d};
    for (int k = 0; k < 3; k++) {
        PT_HIP(hipMemcpyAsync(dst_o[k], o4.data(), (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(hipMemcpyAsync(dst_d[k], d4.data(), (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    }
    PtQueues Q;
    Q.cur = ctx->d_qa.as<uint32_t>(); Q.next = ctx->d_qb.as<uint32_t>();
    Q.nee = ctx->d_qnee.as<uint32_t>(); Q.counts = ctx->d_counts.as<uint32_t>(); Q.sorted = ctx->d_qsorted.as<uint32_t>();
    Q.shadow = ctx->d_qshadow.as<uint32_t>(); Q.probe = ctx->d_qprobe.as<uint32_t>(); Q.shadow_key = nullptr; Q.bin = nullptr;
    uint32_t* const dst_q[3] = {Q.cur, Q.shadow, Q.probe};
    for (int k = 0; k < 3; k++)
        if (!ids[k].empty()) PT_HIP(hipMemcpyAsync(dst_q[k], ids[k].data(), ids[k].size() * 4, hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint32_t> counts(PT_COUNTS_WORDS, 0u);
    counts[PT_Q_CUR] = (uint32_t)ids[0].size(); counts[PT_Q_SHADOW] = (uint32_t)ids[1].size(); counts[PT_Q_PROBE] = (uint32_t)ids[2].size();
    PT_HIP(hipMemcpyAsync(Q.counts, counts.data(), counts.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    DevBuf d_kind, d_out, d_occ;
    PT_HIP(d_kind.alloc(n)); PT_HIP(d_out.alloc((size_t)n * sizeof(pt_hit))); PT_HIP(d_occ.alloc(n));
    PT_HIP(hipMemcpyAsync(d_kind.p, kind, n, hipMemcpyHostToDevice, ctx->stream));
    hipEvent_t a = get_event(ctx, 0), b = get_event(ctx, 1);
    PT_HIP(hipEventRecord(a, ctx->stream));
    PT_HIP(ptk_trace_any(ctx, ctx->stream, ctx->grid_trace, ctx->grid_trace_dist, ctx->sc, P, Q, ctx->d_counters.as<PtCounters>(), ctx->d_spill.as<uint32_t>(), ctx->spill_depth,
                     ctx->d_err.as<uint32_t>(), ctx->trace_far > 0 ? 1 : 0, ctx->scene_alpha ? 1 : 0));      // PBRTGPU_TRACE_FAR=1 forces k_trace_far here too (no trial: the caller's rays are not a bounce)
    PT_HIP(hipEventRecord(b, ctx->stream));
    PT_HIP(ptk_wavefront_results_any(ctx, ctx->stream, ctx->grid_wide, ctx->sc, P, n, d_kind.as<uint8_t>(), d_out.as<pt_hit>(), d_occ.as<uint8_t>()));
    PT_HIP(hipMemsetAsync(Q.counts, 0, PT_COUNTS_WORDS * 4, ctx->stream));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    PT_HIP(hipEventElapsedTime(&ms, a, b));
    ctx->trace_ms += ms;
    ctx->trace_launches++;
    uint32_t herr = 0;
    PT_HIP(hipMemcpy(&herr, ctx->d_err.p, 4, hipMemcpyDeviceToHost));
    if (herr) { PT_HIP(hipMemsetAsync(ctx->d_err.p, 0, 4, ctx->stream)); PT_HIP(hipStreamSynchronize(ctx->stream)); return ctx->fail(PT_ERR_DEVICE, "traversal stack overflow"); }
    PT_HIP(hipMemcpy(out, d_out.p, (size_t)n * sizeof(pt_hit), hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(occluded_out, d_occ.p, n, hipMemcpyDeviceToHost));
    return PT_OK;
}

static pt_status camera_rays(pt_context* ctx, uint32_t n, const int32_t* pixel_xy, const uint32_t* sample_index, float* out_o, float* out_d,
                             float* out_pfilm, float* out_time);
pt_status pt_generate_camera_rays(pt_context* ctx, uint32_t n, const int32_t* pixel_xy, const uint32_t* sample_index, float* out_o, float* out_d,
                                  float* out_pfilm) {
    return camera_rays(ctx, n, pixel_xy, sample_index, out_o, out_d, out_pfilm, nullptr);
}
pt_status pt_generate_camera_rays_time(pt_context* ctx, uint32_t n, const int32_t* pixel_xy, const uint32_t* sample_index, float* out_o, float* out_d,
                                       float* out_pfilm, float* out_time) {
    if (!out_time) return PT_ERR_INVALID_ARGUMENT;
    return camera_rays(ctx, n, pixel_xy, sample_index, out_o, out_d, out_pfilm, out_time);
}
// out_time: the rays' times as well.  A scene that moves asks its own k_gen twin (the ray depends on the time); every other scene gets the
// time from the sampler's fifth dimension, lerp(u, shutter_open, shutter_close) in float32 as perspective.rs:111-117 has it.
static pt_status camera_rays(pt_context* ctx, uint32_t n, const int32_t* pixel_xy, const uint32_t* sample_index, float* out_o, float* out_d,
                             float* out_pfilm, float* out_time) {
    if (!ctx || !pixel_xy || !sample_index || !out_o || !out_d || !out_pfilm) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return PT_OK;
    (void)hipSetDevice(ctx->device);
    DevBuf d_px, d_si, d_o, d_d, d_pf;
    PT_HIP(d_px.alloc((size_t)n * 8)); PT_HIP(d_si.alloc((size_t)n * 4));
    PT_HIP(d_o.alloc((size_t)n * 12)); PT_HIP(d_d.alloc((size_t)n * 12)); PT_HIP(d_pf.alloc((size_t)n * 8));
    PT_HIP(hipMemcpy(d_px.p, pixel_xy, (size_t)n * 8, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_si.p, sample_index, (size_t)n * 4, hipMemcpyHostToDevice));
    DevBuf d_tm, d_dim;
    if (out_time) PT_HIP(d_tm.alloc((size_t)n * 4));
    if (out_time && ctx->motion_kernels)
        PT_HIP(ptv::ptk_camera_rays_time(ctx->stream, ctx->sc, n, d_px.as<int32_t>(), d_si.as<uint32_t>(), d_o.as<float>(), d_d.as<float>(), d_pf.as<float>(), d_tm.as<float>()));
    else {
        PT_HIP(ptk_camera_rays_any(ctx, ctx->stream, ctx->sc, n, d_px.as<int32_t>(), d_si.as<uint32_t>(), d_o.as<float>(), d_d.as<float>(), d_pf.as<float>()));
        if (out_time) {
            const std::vector<uint32_t> dims(n, 4u);
            PT_HIP(d_dim.alloc((size_t)n * 4));
            PT_HIP(hipMemcpy(d_dim.p, dims.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            PT_HIP(ptk_sobol_samples(ctx->stream, ctx->sc, n, d_px.as<int32_t>(), d_si.as<uint32_t>(), d_dim.as<uint32_t>(), d_tm.as<float>()));
        }
    }
    PT_HIP(hipStreamSynchronize(ctx->stream));
    if (out_time) {
        PT_HIP(hipMemcpy(out_time, d_tm.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (!ctx->motion_kernels)
            for (uint32_t i = 0; i < n; i++) out_time[i] = (1.0f - out_time[i]) * ctx->sc.cam.shutter_open + out_time[i] * ctx->sc.cam.shutter_close;
    }
    PT_HIP(hipMemcpy(out_o, d_o.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(out_d, d_d.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(out_pfilm, d_pf.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_bsdf_eval(pt_context* ctx, uint32_t material, uint32_t n, const float* wo, const float* wi, uint32_t flags, float* f_out, float* pdf_out) {
    if (!ctx || !wo || !wi || !f_out || !pdf_out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (material >= ctx->n_materials) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "material index out of range");
    if (material < ctx->per_hit_lobes.size() && ctx->per_hit_lobes[material] == pt_context::PER_HIT_DISNEY)
        return ctx->fail(PT_ERR_UNSUPPORTED, "BSDF hooks: this Disney material's lobes are built at every hit (a textured parameter or a bump map); the hooks take constant materials");
    if (material < ctx->per_hit_lobes.size() && ctx->per_hit_lobes[material])
        return ctx->fail(PT_ERR_UNSUPPORTED, "BSDF hooks: this mix material's lobes are built at every hit (a textured amount or leaf); the hooks take constant trees");
    if (n == 0) return PT_OK;
    (void)hipSetDevice(ctx->device);
    DevBuf d_wo, d_wi, d_f, d_pdf;
    PT_HIP(d_wo.alloc((size_t)n * 12)); PT_HIP(d_wi.alloc((size_t)n * 12)); PT_HIP(d_f.alloc((size_t)n * 12)); PT_HIP(d_pdf.alloc((size_t)n * 4));
    PT_HIP(hipMemcpy(d_wo.p, wo, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_wi.p, wi, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(ptk_bsdf_eval_any(ctx, ctx->stream, ctx->sc, material, n, d_wo.as<float>(), d_wi.as<float>(), flags, d_f.as<float>(), d_pdf.as<float>()));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    PT_HIP(hipMemcpy(f_out, d_f.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(pdf_out, d_pdf.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Light hooks (k_light_hooks): mode 0 sample_li, 1 pdf_li, 2 le
static pt_status light_hook(pt_context* ctx, uint32_t light, uint32_t mode, uint32_t n, const float* a, const float* b, float* o3a, float* o3b, float* o1) {
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (light >= ctx->sc.n_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "light index out of range");
    (void)hipSetDevice(ctx->device);
    if (mode != 0) {
        PtLight L;
        PT_HIP(hipMemcpy(&L, ctx->d_lights.as<PtLight>() + light, sizeof(L), hipMemcpyDeviceToHost));
        if (mode == 1 && (L.mesh_flags & PT_LIGHT_DELTA)) {         // pdf_li of a delta light is 0 for every direction
            if (n) std::memset(o1, 0, (size_t)n * 4);
            return PT_OK;
        }
        if (!(L.mesh_flags & PT_LIGHT_INFINITE)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_light_pdf_li / pt_light_le: not an infinite light");
    }
    if (n == 0) return PT_OK;
    DevBuf d_a, d_b, d_3a, d_3b, d_1;
    PT_HIP(d_a.alloc((size_t)n * 12)); PT_HIP(d_b.alloc((size_t)n * 8)); PT_HIP(d_3a.alloc((size_t)n * 12)); PT_HIP(d_3b.alloc((size_t)n * 12)); PT_HIP(d_1.alloc((size_t)n * 4));
    PT_HIP(hipMemcpy(d_a.p, a, (size_t)n * 12, hipMemcpyHostToDevice));
    if (b) PT_HIP(hipMemcpy(d_b.p, b, (size_t)n * 8, hipMemcpyHostToDevice));
    PT_HIP(ptk_light_hooks_any(ctx, ctx->stream, ctx->sc, light, mode, n, d_a.as<float>(), d_b.as<float>(), d_3a.as<float>(), d_3b.as<float>(), d_1.as<float>()));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    if (o3a) PT_HIP(hipMemcpy(o3a, d_3a.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (o3b) PT_HIP(hipMemcpy(o3b, d_3b.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (o1) PT_HIP(hipMemcpy(o1, d_1.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}
pt_status pt_light_sample_li(pt_context* ctx, uint32_t light, uint32_t n, const float* ref_p, const float* u, float* li_out, float* wi_out, float* pdf_out) {
    if (!ctx || !ref_p || !u || !li_out || !wi_out || !pdf_out) return PT_ERR_INVALID_ARGUMENT;
    return light_hook(ctx, light, 0, n, ref_p, u, li_out, wi_out, pdf_out);
}
pt_status pt_light_pdf_li(pt_context* ctx, uint32_t light, uint32_t n, const float* wi, float* pdf_out) {
    if (!ctx || !wi || !pdf_out) return PT_ERR_INVALID_ARGUMENT;
    return light_hook(ctx, light, 1, n, wi, nullptr, nullptr, nullptr, pdf_out);
}
pt_status pt_light_pdf_from(pt_context* ctx, uint32_t light, uint32_t n, const float* ref_p, const float* wi, float* pdf_out) {
    if (!ctx || !ref_p || !wi || !pdf_out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (light >= ctx->sc.n_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "light index out of range");
    (void)hipSetDevice(ctx->device);
    PtLight L;
    PT_HIP(hipMemcpy(&L, ctx->d_lights.as<PtLight>() + light, sizeof(L), hipMemcpyDeviceToHost));
    if (L.mesh_flags & (PT_LIGHT_INFINITE | PT_LIGHT_DELTA)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_light_pdf_from: not an area light (pt_light_pdf_li answers for the others)");
    if (n == 0) return PT_OK;
    DevBuf d_p, d_w, d_o;
    PT_HIP(d_p.alloc((size_t)n * 12)); PT_HIP(d_w.alloc((size_t)n * 12)); PT_HIP(d_o.alloc((size_t)n * 4));
    PT_HIP(hipMemcpy(d_p.p, ref_p, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_w.p, wi, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(ptk_light_pdf_from_any(ctx, ctx->stream, ctx->sc, light, n, d_p.as<float>(), d_w.as<float>(), d_o.as<float>()));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    PT_HIP(hipMemcpy(pdf_out, d_o.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}
pt_status pt_light_le(pt_context* ctx, uint32_t light, uint32_t n, const float* d, float* rgb_out) {
    if (!ctx || !d || !rgb_out) return PT_ERR_INVALID_ARGUMENT;
    return light_hook(ctx, light, 2, n, d, nullptr, rgb_out, nullptr, nullptr);
}

pt_status pt_bsdf_sample(pt_context* ctx, uint32_t material, uint32_t n, const float* wo, const float* u, uint32_t flags, float* f_out, float* wi_out,
                         float* pdf_out, uint32_t* type_out) {
    if (!ctx || !wo || !u || !f_out || !wi_out || !pdf_out || !type_out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (material >= ctx->n_materials) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "material index out of range");
    if (material < ctx->per_hit_lobes.size() && ctx->per_hit_lobes[material] == pt_context::PER_HIT_DISNEY)
        return ctx->fail(PT_ERR_UNSUPPORTED, "BSDF hooks: this Disney material's lobes are built at every hit (a textured parameter or a bump map); the hooks take constant materials");
    if (material < ctx->per_hit_lobes.size() && ctx->per_hit_lobes[material])
        return ctx->fail(PT_ERR_UNSUPPORTED, "BSDF hooks: this mix material's lobes are built at every hit (a textured amount or leaf); the hooks take constant trees");
    if (n == 0) return PT_OK;
    (void)hipSetDevice(ctx->device);
    DevBuf d_wo, d_u, d_f, d_wi, d_pdf, d_t;
    PT_HIP(d_wo.alloc((size_t)n * 12)); PT_HIP(d_u.alloc((size_t)n * 8)); PT_HIP(d_f.alloc((size_t)n * 12)); PT_HIP(d_wi.alloc((size_t)n * 12));
    PT_HIP(d_pdf.alloc((size_t)n * 4)); PT_HIP(d_t.alloc((size_t)n * 4));
    PT_HIP(hipMemcpy(d_wo.p, wo, (size_t)n * 12, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_u.p, u, (size_t)n * 8, hipMemcpyHostToDevice));
    PT_HIP(ptk_bsdf_sample_any(ctx, ctx->stream, ctx->sc, material, n, d_wo.as<float>(), d_u.as<float>(), flags, d_f.as<float>(), d_wi.as<float>(), d_pdf.as<float>(),
                           d_t.as<uint32_t>()));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    PT_HIP(hipMemcpy(f_out, d_f.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(wi_out, d_wi.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(pdf_out, d_pdf.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    PT_HIP(hipMemcpy(type_out, d_t.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_sobol_samples(pt_context* ctx, uint32_t n, const int32_t* pixel_xy, const uint32_t* sample_index, const uint32_t* dim, float* out) {
    if (!ctx || !pixel_xy || !sample_index || !dim || !out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return PT_OK;
    (void)hipSetDevice(ctx->device);
    DevBuf d_px, d_si, d_dim, d_out;
    PT_HIP(d_px.alloc((size_t)n * 8)); PT_HIP(d_si.alloc((size_t)n * 4)); PT_HIP(d_dim.alloc((size_t)n * 4)); PT_HIP(d_out.alloc((size_t)n * 4));
    PT_HIP(hipMemcpy(d_px.p, pixel_xy, (size_t)n * 8, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_si.p, sample_index, (size_t)n * 4, hipMemcpyHostToDevice));
    PT_HIP(hipMemcpy(d_dim.p, dim, (size_t)n * 4, hipMemcpyHostToDevice));
    PT_HIP(ptk_sobol_samples(ctx->stream, ctx->sc, n, d_px.as<int32_t>(), d_si.as<uint32_t>(), d_dim.as<uint32_t>(), d_out.as<float>()));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    PT_HIP(hipMemcpy(out, d_out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_radiance_samples(pt_context* ctx, const pt_tile* tile, float* out_rgb) {
    if (!ctx || !tile || !out_rgb) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    size_t npx = (size_t)std::max(0, tile->x1 - tile->x0) * (size_t)std::max(0, tile->y1 - tile->y0);
    if (npx == 0) return PT_OK;
    size_t n = npx * ctx->sc.sobol.spp * 3;
    DevBuf d_rad;
    PT_HIP(d_rad.alloc(n * 4));
    // the film is left untouched: render into scratch copies
    size_t fpx = (size_t)ctx->film_w * ctx->film_h;
    DevBuf keep_own, keep_spill;
    PT_HIP(keep_own.alloc(fpx * 16)); PT_HIP(keep_spill.alloc(fpx * 16));
    PT_HIP(hipMemcpyAsync(keep_own.p, ctx->d_own.p, fpx * 16, hipMemcpyDeviceToDevice, ctx->stream));
    PT_HIP(hipMemcpyAsync(keep_spill.p, ctx->d_spillfilm.p, fpx * 16, hipMemcpyDeviceToDevice, ctx->stream));
    pt_status st = render_tiles(ctx, tile, 1, d_rad.as<float>());
    PT_HIP(hipMemcpyAsync(ctx->d_own.p, keep_own.p, fpx * 16, hipMemcpyDeviceToDevice, ctx->stream));
    PT_HIP(hipMemcpyAsync(ctx->d_spillfilm.p, keep_spill.p, fpx * 16, hipMemcpyDeviceToDevice, ctx->stream));
    PT_HIP(hipStreamSynchronize(ctx->stream));
    if (st != PT_OK) return st;
    PT_HIP(hipMemcpy(out_rgb, d_rad.p, n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_set_bvh_build(pt_context* ctx, int where) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (where != PT_BVH_BUILD_AUTO && where != PT_BVH_BUILD_HOST && where != PT_BVH_BUILD_DEVICE) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "unknown BVH build location");
    ctx->bvh_build_where = where;
    return PT_OK;
}

pt_status pt_scene_kernel_set(pt_context* ctx, int32_t* set_out) {
    if (!ctx || !set_out) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    *set_out = ctx->fourier_kernels ? PT_KERNELS_FOURIER : ctx->motion_kernels ? PT_KERNELS_MOTION : ctx->maplight_kernels ? PT_KERNELS_MAP_LIGHT : (ctx->disney_kernels ? PT_KERNELS_DISNEY : (ctx->quadric_kernels ? PT_KERNELS_QUADRIC : PT_KERNELS_BASE));
    return PT_OK;
}

pt_status pt_scene_bvh_digest(pt_context* ctx, uint64_t* nodes_digest, uint64_t* records_digest) {
    if (!ctx || !nodes_digest || !records_digest) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->have_scene) return ctx->fail(PT_ERR_NO_SCENE, "no scene uploaded");
    (void)hipSetDevice(ctx->device);
    auto digest = [&](const DevBuf& b, size_t bytes, uint64_t* out) -> pt_status {
        std::vector<unsigned char> h(bytes);
        if (bytes) PT_HIP(hipMemcpy(h.data(), b.p, bytes, hipMemcpyDeviceToHost));
        uint64_t x = 1469598103934665603ull;
        for (size_t i = 0; i < bytes; i++) { x ^= h[i]; x *= 1099511628211ull; }
        *out = x;
        return PT_OK;
    };
    pt_status st = digest(ctx->d_nodes, ctx->n_nodes_up * sizeof(PtNode), nodes_digest);
    if (st != PT_OK) return st;
    return digest(ctx->d_tris, ctx->n_tris_up * sizeof(PtTri), records_digest);
}

pt_status pt_get_counters(pt_context* ctx, pt_counters* out) {
    if (!ctx || !out) return PT_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    std::memset(out, 0, sizeof(*out));
    if (ctx->d_counters.p) {
        PtCounters c;
        PT_HIP(hipMemcpy(&c, ctx->d_counters.p, sizeof(c), hipMemcpyDeviceToHost));
        out->camera_rays = c.camera_rays; out->regular_rays = c.regular_rays; out->shadow_rays = c.shadow_rays;
        out->nodes_visited = c.nodes; out->tris_tested = c.tris; out->path_vertices = c.vertices;
        out->nodes_from_lds = c.nodes_lds;
    }
    out->trace_launches = ctx->trace_launches;
    out->trace_ms = ctx->trace_ms; out->shade_ms = ctx->shade_ms; out->render_ms = ctx->render_ms;
    return PT_OK;
}

pt_status pt_reset_counters(pt_context* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    if (ctx->d_counters.p) {
        PT_HIP(hipMemsetAsync(ctx->d_counters.p, 0, sizeof(PtCounters), ctx->stream));
        PT_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->trace_launches = 0;
    ctx->trace_ms = ctx->shade_ms = ctx->render_ms = 0;
    return PT_OK;
}

}  // extern "C"
