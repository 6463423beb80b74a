// pt_quadric.h -- the reference's Cylinder and Disk shapes on the device (src/shapes/cylinder.rs, src/shapes/disk.rs) and the default
// Shape::sample_from (src/core/shape/shape.rs:20-38).  They live in the sphere's slot: a PtSphere with `kind` PT_SHAPE_CYLINDER or
// PT_SHAPE_DISK, the same leaf-record kind (PT_TRI_SPHERE) and the same traversal round, in a second build of the kernels
// (pt_kernels_quadric.hip) that a scene without them never runs.  As in pt_sphere.h every product and sum is the one the Rust source
// writes, in its order.  A sphere (`kind` 0) takes none of this code: the shape_* entrances at the end of the file branch to the
// functions of pt_sphere.h, which are as they were.
#pragma once
#include "pt_sphere.h"

// Transform::transform_ray with world_to_object (transform.rs:184-203, :245-282): the ray with its origin shifted along d by the origin's
// error, and both error vectors
PT_DEV void quad_object_ray(const PtSphere& s, V3 ro, V3 rd, V3* o_out, V3* d_out, V3* oe_out, V3* de_out) {
    const float* m = s.w2o;
    const float g3 = PT_GAMMA(3.0f);
    V3 o = sph_point(m, ro);
    V3 oe = g3 * mk3(fabsf(m[0] * ro.x) + fabsf(m[1] * ro.y) + fabsf(m[2] * ro.z) + fabsf(m[3]),
                     fabsf(m[4] * ro.x) + fabsf(m[5] * ro.y) + fabsf(m[6] * ro.z) + fabsf(m[7]),
                     fabsf(m[8] * ro.x) + fabsf(m[9] * ro.y) + fabsf(m[10] * ro.z) + fabsf(m[11]));
    V3 de = g3 * mk3(fabsf(m[0] * rd.x) + fabsf(m[1] * rd.y) + fabsf(m[2] * rd.z), fabsf(m[4] * rd.x) + fabsf(m[5] * rd.y) + fabsf(m[6] * rd.z),
                     fabsf(m[8] * rd.x) + fabsf(m[9] * rd.y) + fabsf(m[10] * rd.z));
    V3 d = sph_vector(m, rd);
    float ls = length_squared(d);
    if (ls > 0.0f) {
        float dt = dot(vabs(d), oe) / ls;
        o = o + d * dt;
    }
    *o_out = o; *d_out = d; *oe_out = oe; *de_out = de;
}

// ---- Cylinder
PT_DEV bool cyl_clipped(const PtSphere& s, V3 p_hit, float phi) {                  // cylinder.rs:118, :138 (no "unless the whole range" as the sphere has)
    return p_hit.z < s.z_min || p_hit.z > s.z_max || phi > s.phi_max;
}
PT_DEV V3 cyl_refine(const PtSphere& s, V3 o, V3 d, float t, float* phi) {          // cylinder.rs:104-115; the retry (:127-137) wraps by 2 PI as well
    V3 p = o + d * t;
    float hit_rad = sqrtf(p.x * p.x + p.y * p.y);
    p.x = p.x * (s.radius / hit_rad);
    p.y = p.y * (s.radius / hit_rad);
    float ph = pt_atan2f(p.y, p.x);
    if (ph < 0.0f) ph += 2.0f * PT_PI;
    *phi = ph;
    return p;
}
// Front of Cylinder::intersect / intersect_p (cylinder.rs:56-141, :196-287): the two are the same test.  SphHit's a_hi / b_hi as for the sphere.
PT_DEV bool cyl_hit_test(const PtSphere& s, V3 o, V3 d, V3 oe, V3 de, float t_max, SphHit* h) {
    {   // The value lane alone, as in sph_hit_test_inl and under its condition: the same operations in the same order, every EFloat keeps
        // lo <= v <= hi, the discriminant and the infinity guard read value lanes only -- a miss proved here is a miss of the whole test.
        // A ray parallel to the axis (a == 0, b == 0): q = -0.5 * (0 + sqrt(0)), q / a is NaN and c / q infinite, NaN <= x is false, so the
        // infinite root becomes t0 and the guard ends the test, here as below.
        const float av = d.x * d.x + d.y * d.y;
        const float bv = (d.x * o.x + d.y * o.y) * 2.0f;
        const float cv = (o.x * o.x + o.y * o.y) - s.radius * s.radius;
        const double discrim = (double)bv * (double)bv - 4.0 * (double)av * (double)cv;
        if (discrim < 0.0) return false;
        const float fr = (float)sqrt(discrim);
        const float qv = bv < 0.0f ? (bv - fr) * -0.5f : (bv + fr) * -0.5f;
        const float r0 = qv / av, r1 = cv / qv;
        const float t0v = r0 <= r1 ? r0 : r1, t1v = r0 <= r1 ? r1 : r0;
        if (isinf(t0v) || isinf(t1v)) return false;
        if (t0v > t_max) return false;
    }
    PtEF ox = ef_make(o.x, oe.x), oy = ef_make(o.y, oe.y);
    PtEF dx = ef_make(d.x, de.x), dy = ef_make(d.y, de.y);
    PtEF rad = ef_make(s.radius, 0.0f);
    PtEF a = ef_add(ef_mul(dx, dx), ef_mul(dy, dy));
    PtEF b = ef_mulf(ef_add(ef_mul(dx, ox), ef_mul(dy, oy)), 2.0f);
    PtEF c = ef_sub(ef_add(ef_mul(ox, ox), ef_mul(oy, oy)), ef_mul(rad, rad));
    PtEF t0, t1;
    if (!ef_quadratic(a, b, c, &t0, &t1)) return false;
    if (isinf(t0.v) || isinf(t1.v)) return false;
    if (t0.hi > t_max || t1.lo <= 0.0f) return false;
    PtEF th = t0;
    if (th.lo <= 0.0f) {
        th = t1;
        if (t_max < th.hi) return false;
    }
    float phi;
    V3 p_hit = cyl_refine(s, o, d, th.v, &phi);
    if (cyl_clipped(s, p_hit, phi)) {
        if (ef_eq(th, t1)) return false;
        if (t1.hi > t_max) return false;
        th = t1;
        p_hit = cyl_refine(s, o, d, th.v, &phi);
        if (cyl_clipped(s, p_hit, phi)) return false;
    }
    h->o = o; h->d = d; h->p_hit = p_hit; h->t = th.v; h->phi = phi;
    h->a_hi = t0.hi;
    h->b_hi = ef_eq(th, t0) ? -PT_INF : t1.hi;
    return true;
}
// ---- Disk: front of Disk::intersect / intersect_p (disk.rs:52-85, :126-159), no intervals.  t_max is tested strictly on both sides; for
// the traversal's deferred test (!(a_hi > t_max) && !(b_hi > t_max)) t >= t_max is next_float_up(t) > t_max.
PT_DEV bool disk_hit_test(const PtSphere& s, V3 o, V3 d, float t_max, SphHit* h) {
    const float height = s.z_min;
    if (d.z == 0.0f) return false;
    const float t = (height - o.z) / d.z;
    if (t <= 0.0f || t >= t_max) return false;
    V3 p_hit = o + d * t;
    const float dist2 = p_hit.x * p_hit.x + p_hit.y * p_hit.y;
    if (dist2 > s.radius * s.radius || dist2 < s.inner_radius * s.inner_radius) return false;
    float phi = pt_atan2f(p_hit.y, p_hit.x);
    if (phi < 0.0f) phi += 2.0f * PT_PI;
    if (phi > s.phi_max) return false;
    h->o = o; h->d = d; h->p_hit = p_hit; h->t = t; h->phi = phi;
    h->a_hi = next_float_up(t);
    h->b_hi = -PT_INF;
    return true;
}
__device__ __forceinline__ bool quad_hit_test_inl(const PtSphere& s, V3 ro, V3 rd, float t_max, SphHit* h) {
    V3 o, d, oe, de;
    quad_object_ray(s, ro, rd, &o, &d, &oe, &de);
    if (s.kind == PT_SHAPE_DISK) return disk_hit_test(s, o, d, t_max, h);
    return cyl_hit_test(s, o, d, oe, de, t_max, h);
}
__device__ __noinline__ bool quad_hit_test(const PtSphere& s, V3 ro, V3 rd, float t_max, SphHit* h) { return quad_hit_test_inl(s, ro, rd, t_max, h); }

// Object-space interaction of a cylinder hit (cylinder.rs:143-174)
PT_DEV void cyl_interaction_obj(const PtSphere& s, const SphHit& h, V3* ph_out, V3* pe, V3* nn_out, V3* dpdu_out, V3* dpdv_out, V2* uv, V3* dndu, V3* dndv) {
    const V3 ph = h.p_hit;
    *uv = mk2(h.phi / s.phi_max, (ph.z - s.z_min) / (s.z_max - s.z_min));
    const V3 dpdu = mk3(-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f);
    const V3 dpdv = mk3(0.0f, 0.0f, s.z_max - s.z_min);
    const V3 d2pduu = (-s.phi_max * s.phi_max) * mk3(ph.x, ph.y, 0.0f);
    const V3 d2pduv = mk3(0.0f, 0.0f, 0.0f), d2pdvv = mk3(0.0f, 0.0f, 0.0f);
    const float E = dot(dpdu, dpdu), F = dot(dpdu, dpdv), G = dot(dpdv, dpdv);
    V3 nn = normalize(cross(dpdu, dpdv));                         // BaseShape::calc_normal (base_shape.rs:27-33)
    if (s.flags & PT_SPH_FLIP) nn = nn * -1.0f;
    const float ee = dot(nn, d2pduu), ff = dot(nn, d2pduv), gg = dot(nn, d2pdvv);
    const float inv_egf2 = 1.0f / (E * G - F * F);
    *dndu = dpdu * ((ff * F - ee * G) * inv_egf2) + dpdv * ((ee * F - ff * E) * inv_egf2);
    *dndv = dpdu * ((gg * F - ff * G) * inv_egf2) + dpdv * ((ff * F - gg * E) * inv_egf2);
    *pe = PT_GAMMA(3.0f) * vabs(mk3(ph.x, ph.y, 0.0f));
    *ph_out = ph; *nn_out = nn; *dpdu_out = dpdu; *dpdv_out = dpdv;
}
// ... and of a disk hit (disk.rs:87-104): the normal is turned to face the ray, so a ray sees the same side from either face
PT_DEV void disk_interaction_obj(const PtSphere& s, const SphHit& h, V3* ph_out, V3* pe, V3* nn_out, V3* dpdu_out, V3* dpdv_out, V2* uv, V3* dndu, V3* dndv) {
    V3 ph = h.p_hit;
    const float dist2 = ph.x * ph.x + ph.y * ph.y;
    const float r_hit = sqrtf(dist2);
    *uv = mk2(h.phi / s.phi_max, (s.radius - r_hit) / (s.radius - s.inner_radius));
    const V3 dpdu = mk3(-s.phi_max * ph.y, s.phi_max * ph.x, 0.0f);
    const V3 dpdv = mk3(ph.x, ph.y, 0.0f) * ((s.inner_radius - s.radius) / r_hit);
    V3 nn = normalize(cross(dpdu, dpdv));
    if (s.flags & PT_SPH_FLIP) nn = nn * -1.0f;
    if (dot(h.d, nn) > 0.0f) nn = nn * -1.0f;
    ph.z = s.z_min;
    *dndu = mk3(0.0f, 0.0f, 0.0f); *dndv = mk3(0.0f, 0.0f, 0.0f);
    *pe = mk3(0.0f, 0.0f, 0.0f);
    *ph_out = ph; *nn_out = nn; *dpdu_out = dpdu; *dpdv_out = dpdv;
}
// World-space interaction (transform_surface_interaction, transform.rs:299-323), the outputs of sph_interaction
__device__ __noinline__ void quad_interaction(const PtSphere& s, const SphHit& h, V3* p, V3* p_error, V3* n, V3* wo, V3* sh_n, V3* dpdu_w, V3* dpdv_w, V2* uv,
                                              V3* dndu_w, V3* dndv_w) {
    V3 ph, pe, nn, dpdu, dpdv, dndu, dndv;
    if (s.kind == PT_SHAPE_DISK) disk_interaction_obj(s, h, &ph, &pe, &nn, &dpdu, &dpdv, uv, &dndu, &dndv);
    else cyl_interaction_obj(s, h, &ph, &pe, &nn, &dpdu, &dpdv, uv, &dndu, &dndv);
    *p = sph_point(s.o2w, ph);
    *p_error = sph_point_abs_error(s.o2w, ph, pe);
    V3 nw = normalize(sph_normal(s.w2o, nn));
    *n = nw;
    *wo = normalize(sph_vector(s.o2w, -h.d));
    *sh_n = face_forward(nw, nw);
    *dpdu_w = sph_vector(s.o2w, dpdu);
    *dpdv_w = sph_vector(s.o2w, dpdv);
    *dndu_w = sph_normal(s.w2o, dndu);
    *dndv_w = sph_normal(s.w2o, dndv);
}

// Cylinder::sample (cylinder.rs:297-326) and Disk::sample (disk.rs:171-191: the whole disk whatever inner_radius and phi_max are, the
// pdf that of the partial annulus -- as written), then the default Shape::sample_from (shape.rs:20-38)
__device__ __noinline__ bool quad_sample_from(const PtSphere& s, V3 ref_p, V2 u, V3* p, V3* n, V3* p_error, float* pdf_out) {
    V3 po, pe, nn;
    if (s.kind == PT_SHAPE_DISK) {
        V2 pd = concentric_sample_disk(u);
        po = mk3(pd.x * s.radius, pd.y * s.radius, s.z_min);
        nn = normalize(sph_normal(s.w2o, mk3(0.0f, 0.0f, 1.0f)));
        pe = mk3(0.0f, 0.0f, 0.0f);
    } else {
        float z = lerpf(u.x, s.z_min, s.z_max);
        float phi = u.y * s.phi_max;
        float sn, cs;
        pt_sincosf(phi, &sn, &cs);
        po = mk3(s.radius * cs, s.radius * sn, z);
        nn = normalize(sph_normal(s.w2o, mk3(po.x, po.y, 0.0f)));
        float hit_rad = sqrtf(po.x * po.x + po.y * po.y);
        po.x = po.x * (s.radius / hit_rad);
        po.y = po.y * (s.radius / hit_rad);
        pe = PT_GAMMA(3.0f) * vabs(mk3(po.x, po.y, 0.0f));
    }
    if (s.flags & PT_SPH_REVERSE) nn = nn * -1.0f;
    *p = sph_point(s.o2w, po);
    *p_error = sph_point_abs_error(s.o2w, po, pe);
    *n = nn;
    float pdf = 1.0f / s.area;
    V3 wi = *p - ref_p;
    if (length_squared(wi) <= 0.0f) return false;
    wi = normalize(wi);
    pdf = pdf * distance_squared(ref_p, *p) / abs_dot(nn, -wi);
    if (pdf <= 0.0f || isinf(pdf)) return false;
    *pdf_out = pdf;
    return true;
}

// ---- by kind, in the build that knows the kinds (PT_QUADRIC: pt_kernels_quadric.hip); the other build calls the sphere's functions as it
// always did.  (second_wrap is the sphere's alone.)
#if PT_QUADRIC
PT_DEV bool shape_hit_test(const PtSphere& s, V3 ro, V3 rd, float t_max, float second_wrap, SphHit* h) {
    if (s.kind == PT_SHAPE_SPHERE) return sph_hit_test(s, ro, rd, t_max, second_wrap, h);
    return quad_hit_test(s, ro, rd, t_max, h);
}
PT_DEV bool shape_hit_test_inl(const PtSphere& s, V3 ro, V3 rd, float t_max, float second_wrap, SphHit* h) {      // the traversal's sphere round
    if (s.kind == PT_SHAPE_SPHERE) return sph_hit_test_inl(s, ro, rd, t_max, second_wrap, h);
    return quad_hit_test_inl(s, ro, rd, t_max, h);
}
PT_DEV void shape_interaction(const PtSphere& s, const SphHit& h, V3* p, V3* p_error, V3* n, V3* wo, V3* sh_n, V3* dpdu_w, V3* dpdv_w, V2* uv, V3* dndu_w,
                              V3* dndv_w) {
    if (s.kind == PT_SHAPE_SPHERE) sph_interaction(s, h, p, p_error, n, wo, sh_n, dpdu_w, dpdv_w, uv, dndu_w, dndv_w);
    else quad_interaction(s, h, p, p_error, n, wo, sh_n, dpdu_w, dpdv_w, uv, dndu_w, dndv_w);
}
PT_DEV bool shape_sample_from(const PtSphere& s, V3 ref_p, V3 ref_pe, V3 ref_n, V2 u, V3* p, V3* n, V3* p_error, float* pdf_out) {
    if (s.kind == PT_SHAPE_SPHERE) return sph_sample_from(s, ref_p, ref_pe, ref_n, u, p, n, p_error, pdf_out);
    return quad_sample_from(s, ref_p, u, p, n, p_error, pdf_out);
}
#else
#define shape_hit_test sph_hit_test
#define shape_hit_test_inl sph_hit_test_inl
#define shape_interaction sph_interaction
#define shape_sample_from sph_sample_from
#endif
