// pt_lobes.h -- Material::compute_scattering_functions (src/materials/*.rs) as "parameters in, BxDF list out", shared by the host
// (constant materials: once per material at upload) and the device (textured materials: at every hit, after the parameter
// textures have been evaluated).  One source, so both produce the same lobes.
#pragma once
#include "pt_device.h"
#include "../../include/pbrtgpu.h"
#ifdef __HIP__
#define PT_HD __host__ __device__
#else
#define PT_HD
#endif

// ---- Material::compute_scattering_functions for constant parameter textures (src/materials/*.rs), evaluated
// once per material: the list of BxDFs the BSDF receives, in the order the material adds them.
static const uint32_t kRefl = 1, kTrans = 2, kDiffuse = 4, kGlossy = 8, kSpecular = 16;    // bxdf.rs:8-14
PT_HD inline float clamp_zero(float v) { return v < 0.0f ? 0.0f : v; }                            // Spectrum::clamp_zero per channel
PT_HD inline bool black(const float* c) { return c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f; }
PT_HD inline PtLobe* push_lobe(PtMaterial& m, uint32_t kind, uint32_t type, const float* r) {
    PtLobe* l = &m.lobes[m.n_lobes++];
    l->fresnel = 0;
    l->t[0] = l->t[1] = l->t[2] = 0.0f; l->k[0] = l->k[1] = l->k[2] = 0.0f;
    l->oa = l->ob = 0.0f;
    l->kind = kind; l->type = type;
    l->r[0] = r[0]; l->r[1] = r[1]; l->r[2] = r[2];
    l->eta_a = l->eta_b = l->fr_eta_i = l->fr_eta_t = 1.0f;
    l->ax = l->ay = 0.001f;
    return l;
}
// The most BxDFs build_lobes below can add for a material type (a mix tree counts a texture-driven leaf at this: pt_context.cpp).  Kept beside
// the switch it summarises: a type that gains a lobe there changes its entry here.
PT_HD inline uint32_t pt_lobes_most(int32_t type) {
    switch (type) {
        case PT_MATERIAL_MATTE: case PT_MATERIAL_MIRROR: case PT_MATERIAL_METAL: case PT_MATERIAL_SUBSTRATE: return 1;
        case PT_MATERIAL_FOURIER: return 1;                        // (not from build_lobes: the upload writes its one lobe, pt_scene_upload.cpp)
        case PT_MATERIAL_PLASTIC: case PT_MATERIAL_GLASS: return 2;
        case PT_MATERIAL_TRANSLUCENT: return 4;
        case PT_MATERIAL_UBER: return 5;
        case PT_MATERIAL_DISNEY: return PT_DISNEY_MOST_LOBES;      // build_disney_lobes below
        default: return 0;
    }
}
PT_HD inline void set_distribution(PtLobe* l, float ax, float ay) {                               // TrowbridgeReitzDistribution::new
    l->ax = 0.001f > ax ? 0.001f : ax;     // f32::max: a NaN roughness becomes 0.001
    l->ay = 0.001f > ay ? 0.001f : ay;
    if (ax != ax) l->ax = 0.001f;
    if (ay != ay) l->ay = 0.001f;
}
// a_r / a_u / a_v: "roughness" / "uroughness" / "vroughness" after the optional roughness_to_alpha remap (done by the caller on
// the host: it needs logf).  Every field of `m` read afterwards is written here.
PT_HD inline void build_lobes(const pt_material& in, float a_r, float a_u, float a_v, PtMaterial& m) {
    m.type = in.type;
    m.n_lobes = 0; m.nonspecular = 0; m.oren_a = 0.0f; m.oren_b = 0.0f;      // every field read afterwards is written here
    m.spec_mask = 0;
    m.kd[0] = in.kd[0]; m.kd[1] = in.kd[1]; m.kd[2] = in.kd[2];
    m.sigma = in.sigma;
    m.bsdf_eta = 1.0f;
    m.has_bsdf = in.type != PT_MATERIAL_NONE;
    const float pick_u = in.uroughness == PT_ROUGHNESS_UNSET ? a_r : a_u;      // Metal / Uber: "uroughness" falls back to "roughness"
    const float pick_v = in.vroughness == PT_ROUGHNESS_UNSET ? a_r : a_v;
    auto cz = [](const float* c, float* out) { for (int i = 0; i < 3; i++) out[i] = clamp_zero(c[i]); };
    auto mul = [](const float* a, const float* b, float* out) { for (int i = 0; i < 3; i++) out[i] = a[i] * b[i]; };
    switch (in.type) {
        case PT_MATERIAL_MATTE: {                       // matte.rs:25-53 (Kd is not clamped here)
            float sig = in.sigma < 0.0f ? 0.0f : (in.sigma > 90.0f ? 90.0f : in.sigma);
            const float pi = 3.14159265358979323846f;
            float sigma = sig * (pi / 180.0f);
            float sigma2 = sigma * sigma;
            m.oren_a = 1.0f - (sigma2 / (2.0f * (sigma2 + 0.33f)));
            m.oren_b = 0.45f * sigma2 / (sigma2 + 0.09f);
            if (!black(in.kd)) {
                PtLobe* l = push_lobe(m, sig == 0.0f ? PT_LOBE_LAMBERT : PT_LOBE_OREN_NAYAR, kRefl | kDiffuse, in.kd);
                l->oa = m.oren_a; l->ob = m.oren_b;
            }
            break;
        }
        case PT_MATERIAL_PLASTIC: {                     // plastic.rs:31-71
            float kd[3], ks[3];
            cz(in.kd, kd); cz(in.ks, ks);
            if (!black(kd)) push_lobe(m, PT_LOBE_LAMBERT, kRefl | kDiffuse, kd);
            if (!black(ks)) {
                float rough = a_r;
                PtLobe* l = push_lobe(m, PT_LOBE_MF_REFL, kRefl | kGlossy, ks);
                set_distribution(l, rough, rough);
                l->fresnel = PT_FR_DIELECTRIC; l->fr_eta_i = 1.5f; l->fr_eta_t = 1.0f;
            }
            break;
        }
        case PT_MATERIAL_MIRROR: {                      // mirror.rs:19-41
            float kr[3];
            cz(in.kr, kr);
            if (!black(kr)) push_lobe(m, PT_LOBE_SPEC_REFL, kRefl | kSpecular, kr)->fresnel = PT_FR_NOOP;
            break;
        }
        case PT_MATERIAL_GLASS: {                       // glass.rs:46-110 (Kr, Kt unclamped; allow_multiple_lobes = true)
            if (black(in.kr) && black(in.kt)) { m.has_bsdf = 0; break; }
            m.bsdf_eta = in.eta;
            if (in.uroughness == 0.0f && in.vroughness == 0.0f) {
                PtLobe* l = push_lobe(m, PT_LOBE_FRESNEL_SPEC, kRefl | kTrans | kSpecular, in.kr);
                for (int i_ = 0; i_ < 3; i_++) (l->t)[i_] = (in.kt)[i_];
                l->eta_a = 1.0f; l->eta_b = in.eta;
            } else {
                float ur = a_u, vr = a_v;
                if (!black(in.kr)) {
                    PtLobe* l = push_lobe(m, PT_LOBE_MF_REFL, kRefl | kGlossy, in.kr);
                    set_distribution(l, ur, vr);
                    l->fresnel = PT_FR_DIELECTRIC; l->fr_eta_i = 1.0f; l->fr_eta_t = in.eta;
                }
                if (!black(in.kt)) {
                    PtLobe* l = push_lobe(m, PT_LOBE_MF_TRANS, kTrans | kGlossy, in.kt);
                    set_distribution(l, ur, vr);
                    l->eta_a = 1.0f; l->eta_b = in.eta;
                }
            }
            break;
        }
        case PT_MATERIAL_METAL: {                       // metal.rs:51-85
            const float one[3] = {1.0f, 1.0f, 1.0f};
            PtLobe* l = push_lobe(m, PT_LOBE_MF_REFL, kRefl | kGlossy, one);
            set_distribution(l, pick_u, pick_v);
            l->fresnel = PT_FR_CONDUCTOR;
            for (int i_ = 0; i_ < 3; i_++) (l->t)[i_] = (in.metal_eta)[i_];
            for (int i_ = 0; i_ < 3; i_++) (l->k)[i_] = (in.metal_k)[i_];
            break;
        }
        case PT_MATERIAL_UBER: {                        // uber.rs:63-127
            float t[3], c[3], tmp[3];
            for (int i = 0; i < 3; i++) t[i] = clamp_zero(1.0f - in.opacity[i]);
            m.bsdf_eta = !black(t) ? 1.0f : in.eta;
            if (!black(t)) push_lobe(m, PT_LOBE_SPEC_TRANS, kTrans | kSpecular, t);       // eta_a = eta_b = 1
            cz(in.kd, tmp); mul(in.opacity, tmp, c);
            if (!black(c)) push_lobe(m, PT_LOBE_LAMBERT, kRefl | kDiffuse, c);
            cz(in.ks, tmp); mul(in.opacity, tmp, c);
            if (!black(c)) {
                PtLobe* l = push_lobe(m, PT_LOBE_MF_REFL, kRefl | kGlossy, c);
                set_distribution(l, pick_u, pick_v);
                l->fresnel = PT_FR_DIELECTRIC; l->fr_eta_i = 1.0f; l->fr_eta_t = in.eta;
            }
            cz(in.kr, tmp); mul(in.opacity, tmp, c);
            if (!black(c)) {
                PtLobe* l = push_lobe(m, PT_LOBE_SPEC_REFL, kRefl | kSpecular, c);
                l->fresnel = PT_FR_DIELECTRIC; l->fr_eta_i = 1.0f; l->fr_eta_t = in.eta;
            }
            cz(in.kt, tmp); mul(in.opacity, tmp, c);
            if (!black(c)) {
                PtLobe* l = push_lobe(m, PT_LOBE_SPEC_TRANS, kTrans | kSpecular, c);
                l->eta_a = 1.0f; l->eta_b = in.eta;
            }
            break;
        }
        case PT_MATERIAL_SUBSTRATE: {                   // substrate.rs:34-68
            float d[3], s[3];
            cz(in.kd, d); cz(in.ks, s);
            if (!black(d) && !black(s)) {
                PtLobe* l = push_lobe(m, PT_LOBE_FRESNEL_BLEND, kRefl | kGlossy, d);
                for (int i_ = 0; i_ < 3; i_++) (l->t)[i_] = (s)[i_];
                set_distribution(l, a_u, a_v);
            }
            break;
        }
        case PT_MATERIAL_TRANSLUCENT: {                 // translucent.rs:38-107 ("reflect" in kr, "transmit" in kt; eta is the constant 1.5)
            float r[3], t[3], k[3], c[3];
            cz(in.kr, r); cz(in.kt, t);
            if (black(r) && black(t)) { m.has_bsdf = 0; break; }           // returns before si.bsdf is set (:56-58)
            m.bsdf_eta = 1.5f;
            cz(in.kd, k);
            if (!black(k)) {
                if (!black(r)) { mul(r, k, c); push_lobe(m, PT_LOBE_LAMBERT, kRefl | kDiffuse, c); }
                if (!black(t)) { mul(t, k, c); push_lobe(m, PT_LOBE_LAMBERT, kTrans | kDiffuse, c); }        // LambertianTransmission: the kTrans bit selects it
            }
            cz(in.ks, k);
            if (!black(k)) {
                if (!black(r)) {
                    mul(r, k, c);
                    PtLobe* l = push_lobe(m, PT_LOBE_MF_REFL, kRefl | kGlossy, c);
                    set_distribution(l, a_r, a_r);
                    l->fresnel = PT_FR_DIELECTRIC; l->fr_eta_i = 1.0f; l->fr_eta_t = 1.5f;
                }
                if (!black(t)) {
                    mul(t, k, c);
                    PtLobe* l = push_lobe(m, PT_LOBE_MF_TRANS, kTrans | kGlossy, c);
                    set_distribution(l, a_r, a_r);
                    l->eta_a = 1.0f; l->eta_b = 1.5f;
                }
            }
            break;
        }
        default: break;
    }
    for (uint32_t i = 0; i < m.n_lobes; i++) {
        if (!(m.lobes[i].type & kSpecular)) m.nonspecular++;
        if ((m.lobes[i].type & (kRefl | kSpecular)) == m.lobes[i].type) m.spec_mask |= 1u;          // matches_flags (bxdf.rs:17-20) against what specular_reflect asks for
        if ((m.lobes[i].type & (kTrans | kSpecular)) == m.lobes[i].type) m.spec_mask |= 2u;         // ... and specular_transmit
    }
}

// ---- Material "disney" (materials/disney.rs:644-804): parameters in, BxDF list out, in the order the text adds them.  At most
// PT_DISNEY_MOST_LOBES lobes, so the list is written to `out` directly (a PtMix record's lobes for a constant material, the per-hit
// list for a textured one), not into a PtMaterial.  The conditions (diffuse_weight > 0, sheen_weight > 0, cc > 0, strans > 0, thin) are
// taken on the evaluated values, per call.  Non-black "scatterdistance" without "thin" never gets here: the upload refuses it.
PT_HD inline PtLobe* disney_lobe(PtLobe* l, uint32_t kind, uint32_t type, float r0, float r1, float r2) {
    l->fresnel = 0;
    l->t[0] = l->t[1] = l->t[2] = 0.0f; l->k[0] = l->k[1] = l->k[2] = 0.0f;
    l->oa = l->ob = 0.0f;
    l->kind = kind; l->type = type;
    l->r[0] = r0; l->r[1] = r1; l->r[2] = r2;
    l->eta_a = l->eta_b = l->fr_eta_i = l->fr_eta_t = 1.0f;
    l->ax = l->ay = 0.001f;
    return l;
}
PT_HD inline float disney_lerp(float t, float a, float b) { return (1.0f - t) * a + t * b; }           // core lerp
PT_HD inline float disney_max(float a, float b) { return b != b ? a : (a > b ? a : b); }                // Float::max(a, b) for a number a: a NaN b gives a
PT_HD inline uint32_t build_disney_lobes(const PtDisneyParams& p, PtLobe* out) {
    uint32_t n = 0;
    const float c[3] = {clamp_zero(p.color[0]), clamp_zero(p.color[1]), clamp_zero(p.color[2])};
    const float metallic_weight = p.f[PT_DP_METALLIC], e = p.f[PT_DP_ETA], strans = p.f[PT_DP_SPECTRANS];
    const float diffuse_weight = (1.0f - 0.5f * metallic_weight) * (1.0f - strans);
    const float dt = p.f[PT_DP_DIFFTRANS] * (1.0f / 2.0f);
    const float rough = p.f[PT_DP_ROUGHNESS];
    const float lum = 0.212671f * c[0] + 0.715160f * c[1] + 0.072169f * c[2];                               // RGBSpectrum::y
    const bool thin = p.thin != 0;
    float c_tint[3], c_sheen[3];
    for (int i = 0; i < 3; i++) c_tint[i] = lum > 0.0f ? c[i] / lum : 1.0f;
    const float sheen_weight = p.f[PT_DP_SHEEN];
    for (int i = 0; i < 3; i++) c_sheen[i] = sheen_weight > 0.0f ? disney_lerp(p.f[PT_DP_SHEENTINT], 1.0f, c_tint[i]) : 0.0f;
    if (diffuse_weight > 0.0f) {
        if (thin) {
            const float flat = p.f[PT_DP_FLATNESS];
            const float sd = diffuse_weight * (1.0f - flat) * (1.0f - dt);
            disney_lobe(&out[n++], PT_LOBE_DISNEY_DIFFUSE, kRefl | kDiffuse, sd * c[0], sd * c[1], sd * c[2]);
            const float ss = diffuse_weight * flat * (1.0f - dt);
            disney_lobe(&out[n++], PT_LOBE_DISNEY_FAKE_SS, kRefl | kDiffuse, ss * c[0], ss * c[1], ss * c[2])->oa = rough;
        } else {
            disney_lobe(&out[n++], PT_LOBE_DISNEY_DIFFUSE, kRefl | kDiffuse, diffuse_weight * c[0], diffuse_weight * c[1], diffuse_weight * c[2]);
        }
        disney_lobe(&out[n++], PT_LOBE_DISNEY_RETRO, kRefl | kDiffuse, diffuse_weight * c[0], diffuse_weight * c[1], diffuse_weight * c[2])->oa = rough;
        if (sheen_weight > 0.0f) {
            const float sw = diffuse_weight * sheen_weight;
            disney_lobe(&out[n++], PT_LOBE_DISNEY_SHEEN, kRefl | kDiffuse, sw * c_sheen[0], sw * c_sheen[1], sw * c_sheen[2]);
        }
    }
    const float aspect = __builtin_sqrtf(1.0f - p.f[PT_DP_ANISOTROPIC] * 0.9f);
    const float ax = disney_max(0.001f, rough * rough / aspect);
    const float ay = disney_max(0.001f, rough * rough * aspect);
    {
        const float spec_tint = p.f[PT_DP_SPECULARTINT];
        const float r0e = ((e - 1.0f) * (e - 1.0f)) / ((e + 1.0f) * (e + 1.0f));                              // schlick_r0_from_eta
        PtLobe* l = disney_lobe(&out[n++], PT_LOBE_MF_REFL, kRefl | kGlossy, 1.0f, 1.0f, 1.0f);
        for (int i = 0; i < 3; i++) l->t[i] = disney_lerp(metallic_weight, r0e * disney_lerp(spec_tint, 1.0f, c_tint[i]), c[i]);      // cspec0
        set_distribution(l, ax, ay);
        l->fresnel = PT_FR_DISNEY | PT_LOBE_G_SEPARABLE;
        l->fr_eta_i = metallic_weight; l->fr_eta_t = e;
    }
    const float cc = p.f[PT_DP_CLEARCOAT];
    if (cc > 0.0f) {
        PtLobe* l = disney_lobe(&out[n++], PT_LOBE_DISNEY_CLEARCOAT, kRefl | kGlossy, 0.0f, 0.0f, 0.0f);
        l->oa = cc;
        l->ob = disney_lerp(p.f[PT_DP_CLEARCOATGLOSS], 0.1f, 0.001f);
    }
    if (strans > 0.0f) {
        PtLobe* l = disney_lobe(&out[n++], PT_LOBE_MF_TRANS, kTrans | kGlossy, strans * __builtin_sqrtf(c[0]), strans * __builtin_sqrtf(c[1]), strans * __builtin_sqrtf(c[2]));
        if (thin) {                                  // a plain TrowbridgeReitzDistribution on the roughness scaled by the IOR
            const float rscaled = (0.65f * e - 0.35f) * rough;
            set_distribution(l, disney_max(0.001f, (rscaled * rscaled) / aspect), disney_max(0.001f, (rscaled * rscaled) * aspect));
        } else {
            set_distribution(l, ax, ay);
            l->fresnel = PT_LOBE_G_SEPARABLE;
        }
        l->eta_a = 1.0f; l->eta_b = e;
    }
    if (thin) disney_lobe(&out[n++], PT_LOBE_LAMBERT, kTrans | kDiffuse, dt * c[0], dt * c[1], dt * c[2]);      // LambertianTransmission, black or not
    return n;
}
// what build_lobes leaves in a PtMaterial for the lobes of a list that lives elsewhere (a mix tree's, a Disney material's)
PT_HD inline void count_lobes(const PtLobe* lobes, uint32_t n, PtMaterial& m) {
    m.nonspecular = 0; m.spec_mask = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!(lobes[i].type & kSpecular)) m.nonspecular++;
        if ((lobes[i].type & (kRefl | kSpecular)) == lobes[i].type) m.spec_mask |= 1u;
        if ((lobes[i].type & (kTrans | kSpecular)) == lobes[i].type) m.spec_mask |= 2u;
    }
}
