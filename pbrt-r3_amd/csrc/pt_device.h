// pt_device.h -- plain-old-data layouts shared by the host side (pt_context.cpp,
// pt_bvh.cpp) and the gfx950 kernels (pt_kernels.hip).  Everything here lives in
// HBM; layouts are chosen for 16-byte lane loads and 128-byte node fetches.
#pragma once
#include <stdint.h>
#include "../../include/pbrtgpu.h"
#include "pt_motion.h"

#define PT_WAVE 64
#define PT_BLOCK 256
#ifndef PT_LDS_STACK
#define PT_LDS_STACK 32          // per-lane traversal stack entries kept in LDS
#endif
// PT_TRACE_WIDE 1: the pooled-leaf traversal kernels (k_trace, k_trace_sph_dist) run as ONE 1024-thread block per CU instead of four 256-thread
// blocks: same sixteen waves, same registers, but the LDS copy of the top of the tree is shared by all of them -- one copy of 341 nodes
// (levels 0..4) instead of four copies of 85 (levels 0..3).
#ifndef PT_TRACE_WIDE
#define PT_TRACE_WIDE 1
#endif
#define PT_TBLOCK (PT_TRACE_WIDE ? 1024 : PT_BLOCK)      // threads per block of the pooled-leaf traversal kernels
#define PT_SLOT (PT_TBLOCK * 4u)   // bytes between two entries of a lane's LDS traversal stack ([entry][lane] layout; pooled-leaf kernels)
// PT_TOP_NODES > 0: the pooled-leaf traversal kernels keep the first PT_TOP_NODES nodes of the world tree (the upload numbers the top
// of the tree breadth-first, so these are its top levels: 85 = levels 0..3) in LDS, 112 bytes each, and visits to them read LDS instead
// of going through the vector L1, whose request rate bounds the kernel.  Paid for with 8 of the 32 stack slots.
#ifndef PT_TOP_NODES
#define PT_TOP_NODES (PT_TRACE_WIDE ? 341 : 85)
#endif
#ifndef PT_SORT_CELL_BITS
#define PT_SORT_CELL_BITS 4      // shadow-ray sort key (pt_raysort.hip): bits per axis of the origin's cell; the key is 3 x this + 3 octant bits wide.
                                 // RT1M, k_trace ms per launch: no sort 164.9, 0 bits (octant only) 162.2, 1: 161.5, 2: 158.9, 3: 157.3, 4: 156.8, 5: 156.6, 6 .. 9: 156.8
#endif
#define PT_TOP_BFS_NODES 1365u   // what the upload renumbers breadth-first (levels 0..5), whatever PT_TOP_NODES the kernels were built with
// LDS stack slots per lane of the pooled-leaf traversal kernels (slot 0 holds a sentinel; deeper entries spill to HBM)
#if PT_TOP_NODES > 0
#define PT_FS_SLOTS (PT_LDS_STACK < 24 ? PT_LDS_STACK : 24)
#else
#define PT_FS_SLOTS PT_LDS_STACK
#endif
#define PT_DIAG_WORDS 2048u       // words at the head of the traversal spill buffer reserved for the diagnostic builds (phase clocks, histograms)
#define PT_EMPTY_REF 0xffffffffu
#define PT_LEAF_BIT 0x80000000u
#define PT_LEAF_COUNT_SHIFT 28          // bits 28..30 of a leaf reference: min(triangles in the leaf, 8) - 1
#define PT_LEAF_FIRST_MASK 0x03ffffffu   // bits 0..25: first triangle record
#define PT_REF_INDEX_MASK 0x03ffffffu    // interior reference: bits 0..25 node index
#define PT_REF_AXIS_SHIFT 26             // bits 26..27 of a CHILD reference stored in a node: one of the node's three split axes, so that the
                                         // lean visit needs no separate load for them -- child 0 carries axis_top, child 1 axis_left, child 3
                                         // axis_right (slots 0 and 2 are always occupied; slot 1 / 3 exactly when the left / right pair is one)

// One 4-wide BVH node = one 128-byte line.  Replaces the reference's 144-byte
// SIMDBVHNode + separate leaf nodes (qbvh_x86.rs:15-24, :93-176): a child that is
// a leaf is referenced as PT_LEAF_BIT | first_triangle_record, so leaves cost no
// node fetch; an empty slot is PT_EMPTY_REF.
struct PtNode {
    float bmin[3][4];            // [axis][child]
    float bmax[3][4];
    uint32_t child[4];
    uint32_t axes;               // axis_top | axis_left << 2 | axis_right << 4 | occupied-slot mask << 8
    uint32_t order_lut;          // written at upload (pt_context.cpp finish_nodes): bit o of byte 0 / 1 / 2 = the ray of direction octant o
                                 // (bit 0 x < 0, bit 1 y < 0, bit 2 z < 0) is negative along axis_top / axis_left / axis_right
    uint32_t pad[2];
};

// Triangle record in BVH leaf order (48 bytes = 3 x dwordx4).  The last record of
// a leaf carries PT_TRI_LAST, so a leaf reference needs no count.
#define PT_TRI_LAST 1u
#define PT_TRI_ONE_SIDED 2u      // !two_sided: cull when dot(n, d) >= 0 (triangle.rs:247-251)
#define PT_TRI_FLIP 4u           // reverse_orientation ^ swaps_handedness
#define PT_TRI_HAS_ATTR 8u       // mesh carries N / S / UV: shading must also read PtTriInfo
#define PT_TRI_SPHERE 16u        // the record stands for a sphere: p0[0] holds its index into PtScene::spheres (as bits)
#define PT_TRI_INSTANCE 32u      // the record stands for an object instance: p0[0] holds its index into PtScene::instances (as bits)
#define PT_TRI_ALPHA 64u         // the mesh has an alpha mask (pt_alpha_mask): the alpha traversal kernels evaluate it at each candidate hit
#define PT_TRI_MATERIAL_SHIFT 16 // bits 16..31: material index + 1 (0 = no material)
// Alpha masks on the device: in a scene with one, word 0 of PtScene::tex_prog (never a program: offset 0 means "constant") is the offset of
// a per-mesh table of two words, "alpha" then "shadowalpha": 0 no mask, PT_ALPHA_CUT a constant <= 0, else the offset of the texture's program.
#define PT_ALPHA_CUT 0xffffffffu
struct PtTri {
    float p0[3];
    uint32_t prim;               // caller's triangle index
    float p1[3];
    uint32_t flags;              // PT_TRI_* | (material + 1) << 16: shading needs no second record
    float p2[3];
    uint32_t light1;             // area light index + 1 (0 = not emissive)
};

// Per original triangle shading record.
struct PtTriInfo {
    uint32_t v[3];               // vertex indices (N / S / UV lookups)
    uint32_t mesh;
    int32_t light;               // index into lights[] or -1
    int32_t material;            // index into materials[] or -1
    uint32_t mesh_flags;         // PT_MESH_* of include/pbrtgpu.h
    uint32_t pad;
};

// One BxDF of a material's BSDF.  With constant textures Material::compute_scattering_functions adds
// the same BxDFs at every hit, so the host evaluates it once per material (pt_context.cpp build_lobes).
enum { PT_LOBE_LAMBERT = 0, PT_LOBE_OREN_NAYAR = 1, PT_LOBE_SPEC_REFL = 2, PT_LOBE_SPEC_TRANS = 3, PT_LOBE_FRESNEL_SPEC = 4,
       PT_LOBE_MF_REFL = 5, PT_LOBE_MF_TRANS = 6, PT_LOBE_FRESNEL_BLEND = 7,
       // Material "disney" (materials/disney.rs:44-323), known to the kernels of pt_kernels_disney.hip only: R in `r`; FakeSS / Retro keep their
       // roughness in `oa`; Clearcoat keeps its weight in `oa` and its gloss in `ob`
       PT_LOBE_DISNEY_DIFFUSE = 8, PT_LOBE_DISNEY_FAKE_SS = 9, PT_LOBE_DISNEY_RETRO = 10, PT_LOBE_DISNEY_SHEEN = 11, PT_LOBE_DISNEY_CLEARCOAT = 12,
       // Material "fourier" (core/reflection/fourier.rs:178-465), known to the kernels of pt_kernels_fourier.hip only: the device address of the
       // material's PtFourierTable rides as bits in t[0] (low word) and t[1] (high word), which no other field of the lobe depends on
       PT_LOBE_FOURIER = 13 };
// (LambertianTransmission, lambertian.rs:49-99, is PT_LOBE_LAMBERT whose `type` carries BSDF_TRANSMISSION instead of BSDF_REFLECTION: pt_bxdf.h)
// PT_FR_DISNEY: DisneyFresnel (disney.rs:330-345): r0 in `t`, metallic in fr_eta_i, eta in fr_eta_t
enum { PT_FR_NOOP = 0, PT_FR_DIELECTRIC = 1, PT_FR_CONDUCTOR = 2, PT_FR_DISNEY = 3 };
#define PT_FR_MASK 0xffu
#define PT_LOBE_G_SEPARABLE 0x100u    // in PtLobe::fresnel of a microfacet lobe: DisneyMicrofacetDistribution, whose g is g1(wo) * g1(wi) (disney.rs:368-371)
struct PtLobe {                  // 80 bytes
    uint32_t kind;               // PT_LOBE_*
    uint32_t type;               // BxDFType bits (bxdf.rs:8-14)
    uint32_t fresnel;            // PT_FR_* of SpecularReflection / MicrofacetReflection
    float ax;                    // TrowbridgeReitz alpha_x (after max(0.001, .))
    float r[3];                  // R / T / Kd / Rd
    float ay;
    float t[3];                  // FresnelSpecular T, FresnelBlend Rs, conductor eta
    float eta_a;
    float k[3];                  // conductor k
    float eta_b;
    float fr_eta_i, fr_eta_t;    // FresnelDielectric
    float oa, ob;                // OrenNayar A, B
};
#define PT_MAX_LOBES 5           // UberMaterial adds at most five BxDFs
struct PtMaterial {
    int32_t type;
    float kd[3];
    float sigma;
    float oren_a, oren_b;        // OrenNayar::new (oren_nayar.rs:16-23), precomputed on the host
    uint32_t n_lobes;
    uint32_t has_bsdf;           // 0: compute_scattering_functions leaves bsdf = None (glass with Kr = Kt = 0, translucent with reflect = transmit = 0)
    uint32_t nonspecular;        // num_components(BSDF_ALL & !BSDF_SPECULAR)
    float bsdf_eta;              // BSDF::eta
    uint32_t sort_bin;           // shade-queue bin: [0,128) Matte materials, [128,256) the others
    uint32_t textured;           // 1: parameters come from textures at each hit (PtMatParams), the lobes below are unused
    uint32_t spec_mask;          // bit 0: some lobe matches BSDF_REFLECTION | BSDF_SPECULAR, bit 1: ... BSDF_TRANSMISSION | BSDF_SPECULAR (what specular_reflect /
                                 // specular_transmit ask BSDF::sample_f for: with the bit clear the call returns None before it looks at anything)
    uint32_t mix1;               // PT_MATERIAL_MIX: index + 1 of the material's PtMix record (0: not a mix); read by the *_mix kernels only
    uint32_t mix_base;           // ... and where the PtMix table starts: that many PtMaterial records into the materials buffer (material_mix below)
    PtLobe lobes[PT_MAX_LOBES];  // n_lobes of them.  PT_MATERIAL_DISNEY: n_lobes is 0 (its list lives in a PtMix record or is built per hit) and these
                                 // bytes hold the material's PtDisneyParams instead (material_disney below): read them as lobes only up to n_lobes
};
// Material "mix" (materials/mix.rs:53-96): the tree under one mix material, flattened at upload.  Its BSDF is the leaves' BxDFs in order
// (child 1's, then child 2's, recursively), each wrapped in one ScaledBxDF (core/reflection/scaled.rs) per mix node above its leaf: the
// scale multiplies what the inner lobe returns, innermost node first, and never enters PtLobe::r.  PT_MAX_LOBES stays what it is for
// every other kernel: these lists live here, beside the materials.
#define PT_MIX_MAX_NODES (PT_MIX_MAX_LEAVES - 1)     // a binary tree of PT_MIX_MAX_LEAVES leaves has that many inner nodes, and no leaf more above it
struct PtMixScales {
    uint32_t lobe_leaf[PT_MIX_MAX_LOBES];                       // per lobe: the leaf it came from
    uint32_t n_chain[PT_MIX_MAX_LEAVES];                        // per leaf: mix nodes above it
    float s[PT_MIX_MAX_LEAVES][PT_MIX_MAX_NODES][3];            // per leaf: the scale (s1 or s2) of each of them, innermost first
};
struct PtMix {
    uint32_t n_leaves, n_nodes;
    uint32_t n_lobes;            // constant trees: entries of lobes[]
    uint32_t per_hit;            // 1: some "amount" or some leaf is texture-driven -- lobes and scales are built at every hit (mix_hit_lobes)
    int32_t leaf_material[PT_MIX_MAX_LEAVES];                   // in lobe order; [0] is the leftmost leaf: its bump map gives the frame, its BSDF the eta
    uint32_t chain[PT_MIX_MAX_LEAVES][PT_MIX_MAX_NODES];        // per leaf, innermost first: node index | side << 8 (0: the node's s1, 1: its s2)
    float amount[PT_MIX_MAX_NODES][3];                          // per node: "amount" where it is constant
    uint32_t amount_prog[PT_MIX_MAX_NODES];                     // ... or the offset of its texture program in PtScene::tex_prog (0 = constant)
    uint32_t pad;
    PtMixScales scales;          // constant trees: complete.  Per-hit trees: n_chain only
    PtLobe lobes[PT_MIX_MAX_LOBES];
};
// One MIP pyramid (core/texture/mipmap.rs) in HBM: all levels back to back, level l at texels + level_off[l] floats.
#define PT_MAX_MIP_LEVELS 16
struct PtImage {
    const float* texels;
    uint32_t width, height;      // level 0 (powers of two); level l is max(1, width >> l) x max(1, height >> l)
    uint32_t channels;           // 1 or 3
    uint32_t n_levels;
    uint32_t level_off[PT_MAX_MIP_LEVELS];
    uint32_t pad[2];
};
#define PT_TEX_PROG_MAX 12          // nodes one parameter's texture graph may need
#define PT_TEX_CHILD_CONST 15u      // texture program entry, child slot: the node's own constant (pt_texture.h)
// A material with texture-driven parameters: the caller's parameter block, the roughness values after the optional
// roughness_to_alpha remap (host-side: logf), and per parameter the offset of its texture program in PtScene::tex_prog
// (0 = constant).  Parameter order: Kd Ks Kr Kt opacity sigma metal-eta metal-k bump roughness uroughness vroughness eta.
struct PtMatParams {
    pt_material m;
    float a_r, a_u, a_v;
    uint32_t prog[13];           // [8] = the bump map's displacement texture, [9..12] = roughness, uroughness, vroughness, eta
};
// Material "disney": its thirteen parameters as create_disney_material reads them (disney.rs:806-841) and per parameter the offset of its
// texture program (0 = constant).  f[]: metallic eta roughness speculartint anisotropic sheen sheentint clearcoat clearcoatgloss spectrans
// flatness difftrans.  A Disney material's eight lobes do not fit PtMaterial::lobes (they live in a PtMix record of one leaf, or in the
// per-hit list), so the block lives there: PtMaterial and PtScene keep their sizes.
#define PT_DISNEY_MOST_LOBES 8
enum { PT_DP_METALLIC = 0, PT_DP_ETA, PT_DP_ROUGHNESS, PT_DP_SPECULARTINT, PT_DP_ANISOTROPIC, PT_DP_SHEEN, PT_DP_SHEENTINT, PT_DP_CLEARCOAT,
       PT_DP_CLEARCOATGLOSS, PT_DP_SPECTRANS, PT_DP_FLATNESS, PT_DP_DIFFTRANS, PT_DP_COUNT };
struct PtDisneyParams {
    float color[3];
    float f[PT_DP_COUNT];
    uint32_t thin;
    uint32_t prog_color;
    uint32_t prog[PT_DP_COUNT];
    uint32_t prog_bump;
};
static_assert(sizeof(PtDisneyParams) <= sizeof(PtLobe) * PT_MAX_LOBES, "the Disney parameter block lives in PtMaterial::lobes");

// Material "fourier": one tabulated BSDF (FourierBSDFTable, core/reflection/fourier.rs:30-41) in HBM, shared by every material that names
// it.  The upload has checked every (offset, length) pair against the coefficient array (pt_fourier_table.h).  A PT_LOBE_FOURIER lobe
// carries this record's address, so PtScene, PtMaterial and PtLobe keep their sizes and no kernel argument changes.
struct PtFourierTable {          // 80 bytes
    const float* mu;             // [n_mu]
    const float* cdf;            // [n_mu * n_mu]
    const float* a0;             // [n_mu * n_mu]: a[offset] where length > 0, else 0
    const float* a;              // [n_coeffs]
    const float* recip;          // [max(m_max, 1)]: inf, then 1 / k
    const int32_t* m;            // [n_mu * n_mu]: lengths
    const int32_t* a_offset;     // [n_mu * n_mu]
    uint32_t n_mu, n_channels, m_max;
    float eta;
    uint32_t capped;             // samples whose inversion reached its iteration cap (pt_fourier.h); the kernels add, pt_scene_info_get reads
    uint32_t pad;
};
static_assert(sizeof(PtFourierTable) == 80, "PtFourierTable records lie back to back at the head of the table buffer");

// One DiffuseAreaLight (one emissive triangle).
struct PtLight {
    float p0[3]; float area;
    float p1[3]; uint32_t mesh_flags;
    float p2[3]; int32_t two_sided;
    float L[3];  uint32_t tri_rec;   // index of the triangle's PtTri record
    float n0[3]; uint32_t prim;
    float n1[3]; uint32_t n_samples;   // the light's sample count (DirectLighting "all": size of its sample arrays), >= 1
    float n2[3]; uint32_t pad1;
};

// Sphere (shapes/sphere.rs:7-41), affine transforms only.  The slot also holds the other analytic shapes, told apart by `kind`
// (PT_SHAPE_* of pbrtgpu.h): Cylinder (shapes/cylinder.rs:11-38: z_min / z_max unclamped, theta_* unused) and Disk (shapes/disk.rs:8-35:
// its height in z_min, z_max and theta_* unused).  `area` is the kind's Shape::area.
#define PT_SPH_REVERSE 1u        // reverse_orientation: flips sampled normals (sphere.rs:293-295, :380-382)
#define PT_SPH_FLIP 2u           // reverse_orientation ^ transform_swaps_handedness: flips the intersection normal
struct PtSphere {                // 144 bytes
    float o2w[12];               // rows 0..2 of object_to_world.m
    float w2o[12];               // rows 0..2 of object_to_world.m_inv
    float radius, z_min, z_max, phi_max;
    float theta_min, theta_max, area;
    uint32_t flags;
    uint32_t kind;               // PT_SHAPE_SPHERE 0 / PT_SHAPE_CYLINDER 1 / PT_SHAPE_DISK 2
    float inner_radius;          // disk only
    uint32_t pad[2];
};
// ObjectInstance: TransformedPrimitive over an object's accelerator (affine, static).
struct PtInstance {              // 144 bytes
    float m[12];                 // rows 0..2 of instance_to_world
    float minv[12];              // rows 0..2 of its stored inverse
    uint32_t root_ref;           // the object's root (node index or leaf reference); direct: its single record's index
    uint32_t direct;             // 1: one primitive, wrapped without an accelerator (no root box test)
    float root_lo[3], root_hi[3];// the accelerator's bound (QBVHAccel::intersect starts with it)
    uint32_t world_prim;         // the instance's index in the world primitive list (pt_hit.prim)
    uint32_t motion1;            // index of the instance's PtMotion record (scene_motions; >= 1, entry 0 is the camera's), 0 = static.  Only the
                                 // fifth build of the kernels (pt_kernels_motion.hip) reads it
    uint32_t pad[2];
};
#define PT_LIGHT_SPHERE 0x80000000u   // PtLight::mesh_flags: the light's shape is entry number bits(p0[0]) of PtScene::spheres (any kind)
#ifdef __HIPCC__
#define PT_HOSTDEV_ENVS __host__ __device__
#else
#define PT_HOSTDEV_ENVS
#endif
#define PT_LIGHT_INFINITE 0x40000000u // PtLight::mesh_flags: an InfiniteAreaLight, side record PtScene::envs[bits(p0[0])]; tri_rec = ~0u
// InfiniteAreaLight (lights/infinite.rs): its transforms, the world's bounding-sphere radius and the Distribution2D over its map
// (core/sampling/distribution.rs:109-145), all tables in HBM.
struct PtEnvLight {
    float l2w[12];               // rows 0..2 of light_to_world.m
    float w2l[12];               // rows 0..2 of its stored inverse
    float radius;                // Bounds3::bounding_sphere of the world bound: half the diagonal (bounds3.rs:173-177)
    uint32_t image;              // index into PtScene::images: the map (s repeat, t clamp)
    uint32_t nu, nv;             // nv conditional distributions of nu entries each
    const float* func;           // [nv][nu]
    const float* cdf;            // [nv][nu + 1]
    const float* mfunc;          // [nv]: the marginal's function (the conditionals' func_int)
    const float* mcdf;           // [nv + 1]
    float m_int;                 // the marginal's func_int
    uint32_t pad[3];
};
#define PT_LIGHT_DELTA 0x20000000u    // PtLight::mesh_flags: a PointLight / SpotLight / DistantLight, side record scene_deltas(sc)[bits(p0[0])]; tri_rec = ~0u
// The delta lights (lights/point.rs, spot.rs, distant.rs) as their constructors leave them: every field is computed at upload from a
// pt_delta_light.  Their estimate has no MIS weight and no probe ray (sample_lights.rs:380-397).
struct PtDeltaLight {            // 80 bytes
    uint32_t kind;               // PT_DELTA_POINT / PT_DELTA_SPOT / PT_DELTA_DISTANT
    float v[3];                  // p_light (point, spot) or w_light (distant)
    float spectrum[3];           // I (point, spot) or L (distant), scale included
    float cos_total_width;       // spot: cos(radians(coneangle)), f32 on the host
    float cos_falloff_start;     // spot: cos(radians(coneangle - conedelta))
    float radius;                // distant: the world bound's bounding-sphere radius (PtEnvLight::radius)
    float w2l[9];                // spot: rows 0..2 of world_to_light.m, the 3 x 3 part transform_vector reads (SpotLight::falloff)
    uint32_t pad;                // goniometric, projection: index of the light's PtMapLight record (scene_map_lights)
};
// GonioPhotometricLight / ProjectionLight (lights/goniometric.rs, projection.rs): a PtDeltaLight of kind PT_DELTA_GONIOMETRIC /
// PT_DELTA_PROJECTION (v = p_light, spectrum = intensity) plus this side record, so that PtDeltaLight keeps its 80 bytes for the kernels
// that read it today.  Only the fourth build of the kernels (pt_kernels_maplight.hip) reads these records.
struct PtMapLight {              // 136 bytes
    float w2l[12];               // rows 0..2 of world_to_light.m: goniometric reads all twelve (transform_point on a direction, as written), projection the 3 x 3 part
    uint32_t image;              // index into PtScene::images: the map (s repeat, t clamp)
    float proj[16];              // projection: light_projection.m = (scale(1/tan(fov/2)) * perspective(1e-3, 1e30)).m, all sixteen for transform_point as written
    float screen[4];             // projection: screen_bounds min.x min.y max.x max.y
    uint32_t pad;
};

struct PtCamera {
    float raster_to_camera[16];
    float camera_to_world[16];
    float lens_radius, focal_distance;
    float shutter_open, shutter_close;      // read by the motion build's k_gen only (the two words were padding)
};

struct PtFilm {
    int32_t crop[4];             // x0 y0 x1 y1
    int32_t sample_bounds[4];
    float filter_radius[2];
    float inv_filter_radius[2];
    float max_sample_luminance;
    float scale;
    int32_t box_unit;            // 1 when every in-pixel sample has a one-pixel footprint of weight 1
    int32_t pad;
    float filter_table[256];
};

struct PtSobol {
    const uint32_t* m32;         // [n_dims * 52]
    const uint64_t* vdc;         // row (log2_resolution - 1) of VDC_SOBOL_MATRICES
    const uint64_t* vdc_inv;     // row (log2_resolution - 1) of VDC_SOBOL_MATRICES_INV
    uint32_t m32_len;
    const uint32_t* bytetab;     // [n_tab_dims][7][256]: XOR of the columns selected by one index byte
    uint32_t n_tab_dims;
    uint32_t pad;
    uint32_t log2_resolution;
    uint32_t resolution;
    uint32_t spp;                // Sobol': rounded up to a power of two; Halton: as given
    // ---- HaltonSampler (samplers/halton.rs:46-162); kind selects the sampler
    uint32_t kind;               // PT_SAMPLER_SOBOL / PT_SAMPLER_HALTON
    uint32_t h_center;           // "samplepixelcenter"
    uint32_t h_exp[2];           // base_exponents
    uint32_t h_scale1;           // base_scales[1]
    uint32_t h_stride;           // sample_stride
    uint32_t h_mul[2];           // (sample_stride / base_scales[i]) * mult_inverse[i]
    const uint4* h_dims;         // per dimension: {prime, offset into perms, magic lo, magic hi}; magic = floor(2^64/prime)+1
    const uint16_t* h_perms;     // radical-inverse digit permutations (halton.rs:12-20)
    uint32_t h_n_dims;
    uint32_t pad2;
};

struct PtLightGrid {
    // dense replacement for the reference's lazily filled hash table (spatial.rs:199-260):
    // voxel v owns floats [v*stride, (v+1)*stride): func[nl], cdf[nl+1], func_int
    const float* data;
    uint32_t voxels[3];
    uint32_t n_lights;
    uint32_t stride;
    uint32_t single;             // 1: uniform / power strategy, one table for every point
    float wb_min[3], wb_max[3];
    // Lazy fill (scenes whose dense grid would not fit: thousands of lights): row_of[voxel] = the row of `data` that holds the voxel's tables, or
    // a negative number while nobody has asked for it (spatial.rs:199-260 fills on first touch as well).  nullptr: dense, row = voxel.
    const int32_t* row_of;
};

struct PtCounters {
    unsigned long long regular_rays, shadow_rays, nodes, tris, vertices, camera_rays;
    unsigned long long nodes_lds;       // of `nodes`: visits k_trace served from its LDS copy of the top of the tree (no L1 request)
};

struct PtScene {
    uint32_t dist_leaves;        // 1: no leaf holds more than 8 triangles, k_trace spreads leaf tests over the wave
    uint32_t any_one_sided;      // 1: some triangle is one-sided ("twosided" false): leaf rounds also need the ray direction
    uint32_t general_materials;  // bit 0: some material is not Matte, k_shade_general runs instead of k_shade (read as a truth value).  Bits 1..: the
                                 // number of Material "mix" materials (scene_n_mix); > 0: the *_mix kernels run.  PtScene keeps its size and layout:
                                 // it is a kernel argument that the shading kernels also hold in scratch, so a new field would move their figures
    uint32_t n_deltas;           // delta lights (PtLight records with PT_LIGHT_DELTA; side records: scene_deltas); > 0: the *_env kernels run.  (It sits in
                                 // what was the alignment hole before `nodes`: PtScene keeps its size and every other field its offset.)
    const PtNode* nodes;
    const PtTri* tris;
    const PtTriInfo* tri_info;
    const float* N; const float* S; const float* UV;     // per-vertex attributes or null
    const PtMaterial* materials;
    const PtLight* lights;
    const PtSphere* spheres;
    const PtInstance* instances;
    uint32_t n_instances;        // > 0: k_trace_inst / k_shade_general_inst run
    uint32_t n_envs;             // infinite lights (PtLight records with PT_LIGHT_INFINITE; side records: scene_envs); > 0: the *_env kernels run
    const pt_texture* textures;  // pt_scene_desc.textures as given
    const uint32_t* tex_prog;    // texture programs (pt_texture.h)
    const PtImage* images;       // MIP pyramids of the imagemap textures
    const PtMatParams* mat_params;   // per material; read for textured materials only
    uint32_t textured;           // 1: some material is textured (k_shade_general_full runs)
    uint32_t n_spheres;          // > 0: the sphere-capable kernel instantiations run
    uint32_t n_lights;
    uint32_t root_ref;           // node 0, or a leaf reference when the whole scene is one leaf
    uint32_t n_top;              // nodes 0 .. n_top-1 are the top of the world tree in breadth-first order (at most PT_TOP_BFS_NODES)
    float cell_scale[3];         // 2^PT_SORT_CELL_BITS / the world bound's extent per axis (0 for a flat axis): ray origin -> cell coordinate
    float wb_min[3], wb_max[3];  // BVH root bounds (Scene::world_bound)
    int32_t max_depth;
    float rr_threshold;
    int32_t integrator;          // pt_integrator_type
    int32_t direct_strategy;     // pt_direct_strategy (directlighting)
    int32_t ao_samples, ao_cos_sample;
    PtCamera cam;
    PtFilm film;
    PtSobol sobol;
    PtLightGrid grid;
};
// The infinite lights' PtEnvLight records follow the n_lights PtLight records in the same buffer (PtScene keeps its size and layout).
PT_HOSTDEV_ENVS inline const PtEnvLight* scene_envs(const PtScene& sc) { return reinterpret_cast<const PtEnvLight*>(sc.lights + sc.n_lights); }
// ... and the delta lights' PtDeltaLight records follow those.
PT_HOSTDEV_ENVS inline const PtDeltaLight* scene_deltas(const PtScene& sc) { return reinterpret_cast<const PtDeltaLight*>(scene_envs(sc) + sc.n_envs); }
// ... and the PtMapLight records of the goniometric / projection lights among them follow the last PtDeltaLight (n_deltas counts every delta record).
PT_HOSTDEV_ENVS inline const PtMapLight* scene_map_lights(const PtScene& sc) { return reinterpret_cast<const PtMapLight*>(scene_deltas(sc) + sc.n_deltas); }
// The mix materials' count rides above bit 0 of general_materials; their PtMix records follow the PtMaterial records in the materials buffer.
PT_HOSTDEV_ENVS inline uint32_t scene_n_mix(const PtScene& sc) { return sc.general_materials >> 1; }
PT_HOSTDEV_ENVS inline const PtMix& material_mix(const PtScene& sc, const PtMaterial& m) {
    return reinterpret_cast<const PtMix*>(sc.materials + m.mix_base)[m.mix1 - 1u];
}
// The PtMotion records of a scene that moves (pt_motion.h) follow the n_instances PtInstance records in the instances buffer: entry 0 is the
// camera's (its start transform is PtCamera::camera_to_world), entry PtInstance::motion1 an instance's.  Only pt_kernels_motion.hip reads them.
static_assert(sizeof(PtInstance) == 144 && sizeof(PtInstance) % 16 == 0, "PtMotion records behind the instances");
PT_HOSTDEV_ENVS inline const PtMotion* scene_motions(const PtScene& sc) { return reinterpret_cast<const PtMotion*>(sc.instances + sc.n_instances); }
// A Disney material's parameter block, in the lobe slots its PtMaterial record does not use (PtDisneyParams above).
PT_HOSTDEV_ENVS inline const PtDisneyParams& material_disney(const PtMaterial& m) { return *reinterpret_cast<const PtDisneyParams*>(m.lobes); }
static_assert(sizeof(PtMaterial) % 16 == 0 && sizeof(PtMix) % 4 == 0, "the PtMix table behind the materials");
static_assert(sizeof(PtDeltaLight) == 80 && sizeof(PtEnvLight) % 8 == 0 && sizeof(PtLight) % 16 == 0, "side records of the light buffer");
static_assert(__builtin_offsetof(PtScene, nodes) == 16, "n_deltas fills the hole in front of PtScene::nodes");

// ---- wavefront path pool (SoA, one slot per in-flight camera sample)
struct PtPaths {
    float4* ray_o;       // xyz origin, w = t_max
    float4* ray_d;       // xyz direction
    float4* sh_o;        // shadow ray (NEE light sample), w = t_max
    float4* sh_d;
    float4* pr_o;        // MIS probe ray, w = t_max (inf)
    float4* pr_d;
    float4* beta;        // xyz, w = eta_scale
    float4* L;           // xyz radiance, w unused
    float4* pendA;       // light-sample term f*Li*(w/pdf), w = selection pdf; w = +0: the folded estimate beta*((0+A)/pdf), pendB / pbeta / nee not written (shade_body)
    float4* pendB;       // BSDF-sample term,              w = beta snapshot index unused
    float4* pbeta;       // beta at NEE time
    float2* p_film;
    uint64_t* sobol_index;
    uint32_t* pixel;     // x | y << 16 relative to sample_bounds.min
    uint32_t* state;     // dim (16) | bounces (8) | flags (8)
    float* hit_t;
    int32_t* hit_rec;    // triangle record index or -1
    uint32_t* nee;       // bit0 shadow ray live, bit1 probe live, bits 8.. light index
    uint8_t* occluded;
    int32_t* probe_rec;
    uint32_t* hit_inst;  // instance index + 1 of the closest hit (0 = a world primitive); allocated for scenes with instances only
    float4* tex_res;     // [n_paths][PT_TEX_RES_F4]: what k_tex_resolve evaluated at a textured hit (parameter values, alphas, the bump-mapped
                         // shading frame), read by k_shade_general_res; allocated for scenes with textured materials only
};
#define PT_TEX_RES_F4 9u

// ---- DirectLightingIntegrator / WhittedIntegrator on the wavefront (pt_kernels.hip, "recursive integrators"): the per-camera-sample
// state of the depth-first walk over the specular_reflect / specular_transmit tree
#define PT_REC_FRAME_F4 8u       // float4 per frame
struct PtRec {
    float4* diff;            // [4][n_paths]: the current ray's offset rays rx_o, ry_o, rx_d, ry_d (valid when PT_ST_DIFF is set)
    float4* frames;          // [max_depth][PT_REC_FRAME_F4][n_paths]: ray o | hit record, ray d | instance, rx_o | phase, ry_o, rx_d | pending scale,
                             //                                        ry_d, l, pending f
    // next-event entries, entry e = path * epp + j (j: light by light, one entry per light sample; 0 for "one"): shadow ray, MIS probe ray, the two
    // pending terms
    float4 *sh_o, *sh_d, *pr_o, *pr_d, *A, *B;       // A.w = what the light's summed estimate is divided by ("one": the selection pdf; "all": the sample count), B.w unused
    uint8_t* occ;            // shadow ray result
    int32_t* prec;           // probe ray result (closest record)
    uint32_t* flags;         // per entry: PT_NEE_SHADOW | PT_NEE_PROBE | light << 8
    uint32_t n_paths, max_depth, epp, n_arrays;      // epp: entries per path ("all": the lights' sample counts added up); n_arrays: 2-D sample arrays
                                                     // requested per pixel ("all": two per light and depth)
    uint32_t s0, n_pix;                              // of the pass: path p is sample number s0 + p / n_pix of its pixel (the arrays are indexed by it)
    uint32_t* panic;                                 // the context's error word: bit 2 (4) = a node asked the Halton sampler for a dimension past its
                                                     // table, where the reference panics (halton.rs:103-108)
};
#define PT_REC_OUT_FRAME 0u      // k_rec_enter outcomes (bits 2..3 of the state's flag byte): a frame was pushed, next-event rays may be pending
#define PT_REC_OUT_RETURN0 1u    // the ray left the scene (or Whitted met a surface without BSDF): the node returns zero
#define PT_REC_OUT_RETRACE 2u    // DirectLighting passed through a surface without BSDF: the new ray is traced at the same depth
#define PT_ST_DIFF 1u            // recursive integrators: the current ray carries differentials

#define PT_ST_SPECULAR 1u
#define PT_ST_CAMERA 2u         // the ray is still the camera ray: it has differentials (textures filter with them)
#define PT_NEE_SHADOW 1u
#define PT_NEE_PROBE 2u

struct PtQueues {
    uint32_t* cur;       // path ids to shade / whose continuation ray is traced
    uint32_t* next;
    uint32_t* nee;       // path ids with a pending NEE resolve (k_nee_resolve)
    uint32_t* shadow;    // path ids whose NEE shadow ray (any hit) is to be traced   (counts[7])
    uint32_t* probe;     // path ids whose MIS probe ray (closest hit) is to be traced (counts[8])
    uint32_t* counts;    // counters, PT_Q_* below.  The ones every wave bumps with an atomic sit 128 bytes apart:
                         // atomics on one line serialise in a single L2 channel (k_shade was bound by exactly that)
    uint32_t* sorted;    // cur re-ordered by material bin, misses dropped (scenes with non-Matte materials)
    uint16_t* bin;       // per entry of cur: its material bin (0xffff: a miss), written by k_sort_count for k_sort_scatter; nullptr: recomputed there
    uint32_t* shadow_key;// per entry of shadow: the sort key of its ray (origin cell | direction octant, pt_raysort.hip); nullptr: not wanted
};
#define PT_Q_CUR 0u          // items in cur
#define PT_Q_MATTE_END 1u    // material sort: end of the Matte segment of sorted
#define PT_Q_GENERAL_END 2u  // material sort: end of the sorted queue (= end of the textured segment)
#define PT_Q_TEX_BEGIN 3u    // material sort: end of the general segment = start of the textured-material segment
#define PT_Q_NEXT 32u        // items pushed to next
#define PT_Q_NEE 64u         // paths with a pending NEE resolve
#define PT_Q_TICKET 96u      // work ticket (k_trace, k_shade Matte segment)
#define PT_Q_TICKET2 128u    // work ticket of k_shade_general
#define PT_Q_TICKET3 224u    // work ticket of k_shade_general_res (textured-material segment)
#define PT_Q_SHADOW 160u     // shadow rays queued
#define PT_Q_PROBE 192u      // probe rays queued
#define PT_SORT_BINS 256u
#define PT_SORT_GENERAL0 128u
#define PT_SORT_TEX0 224u       // bins [224, 256): materials with texture-driven parameters (lobes built per hit)
#define PT_SORT_COUNT0 256u                       // [+256) bin counts
#define PT_SORT_CURSOR0 (256u + 256u)             // [+256) bin cursors
#define PT_Q_SEG_TICKET0 768u                     // k_trace: one ticket per queue segment (8 segments, 128 B apart)
#define PT_COUNTS_WORDS (768u + 8u * 32u)
