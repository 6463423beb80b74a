// pt_motion.cpp -- the host side of AnimatedTransform (core/transform/animated_transform.rs): decompose() as the reference has it
// (core/transform/decompose.rs, its own variant of pbrt-v3's polar decomposition), AnimatedTransform::new, motion_bounds, and the two
// host-only entry points of the C ABI.  float32, operation for operation (-ffp-contract=off).
#include "pt_motion.h"

#include <cstring>

#include "../../include/pbrtgpu.h"
#include "pt_host_math.h"

namespace {

using pth::M44;

M44 transpose(const M44& m) {
    M44 r;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.a[4 * i + j] = m.a[4 * j + i];
    return r;
}
float length3(float x, float y, float z) { return std::sqrt(x * x + y * y + z * z); }
// suppress_for_scale (decompose.rs:13-19): the identity with the argument's diagonal -- the scale keeps no shear
M44 suppress_for_scale(const M44& m) {
    M44 r = pth::m_identity();
    for (int i = 0; i < 3; i++) r.a[5 * i] = m.a[5 * i];
    return r;
}
struct Quat { float x, y, z, w; };
Quat quat_new(float x, float y, float z, float w) { return w >= 0.0f ? Quat{x, y, z, w} : Quat{-x, -y, -z, -w}; }      // Quaternion::new: w >= 0
float quat_dot(const Quat& a, const Quat& b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z) + (a.w * b.w); }
Quat quat_normalize(const Quat& q) {
    const float l = std::sqrt(quat_dot(q, q));
    return quat_new(q.x / l, q.y / l, q.z / l, q.w / l);
}
// Quaternion::from_matrix (quaternion.rs:137-170)
Quat quat_from_matrix(const M44& mm) {
    const float* m = mm.a;
    const float trace = m[0] + m[5] + m[10];
    if (trace > 0.0f) {
        const float s = std::sqrt(trace + 1.0f) * 2.0f;
        return quat_new((m[9] - m[6]) / s, (m[2] - m[8]) / s, (m[4] - m[1]) / s, s / 4.0f);
    } else if (m[0] > m[5] && m[0] > m[10]) {
        const float s = std::sqrt(1.0f + m[0] - m[5] - m[10]) * 2.0f;
        return quat_new(s / 4.0f, (m[4] + m[1]) / s, (m[2] + m[8]) / s, (m[9] - m[6]) / s);
    } else if (m[5] > m[10]) {
        const float s = std::sqrt(1.0f + m[5] - m[0] - m[10]) * 2.0f;
        return quat_new((m[4] + m[1]) / s, s / 4.0f, (m[9] + m[6]) / s, (m[2] - m[8]) / s);
    }
    const float s = std::sqrt(1.0f + m[10] - m[0] - m[5]) * 2.0f;
    return quat_new((m[2] + m[8]) / s, (m[9] + m[6]) / s, s / 4.0f, (m[4] - m[1]) / s);
}
M44 quat_to_matrix(const Quat& q) {
    const float v[4] = {q.x, q.y, q.z, q.w};
    float r9[9];
    pt_motion_quat_matrix(v, r9);
    M44 m = pth::m_identity();
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[4 * i + j] = r9[3 * i + j];
    return m;
}
float lerp(float t, float a, float b) { return (1.0f - t) * a + t * b; }

// Transform::transform_bounds (transform.rs:134-182) with the matrix alone
void transform_bounds(const float* m, const float lo[3], const float hi[3], float out_lo[3], float out_hi[3]) {
    for (int c = 0; c < 8; c++) {
        const float x = (c & 4) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 1) ? hi[2] : lo[2];
        float q[3] = {m[0] * x + m[1] * y + m[2] * z + m[3], m[4] * x + m[5] * y + m[6] * z + m[7], m[8] * x + m[9] * y + m[10] * z + m[11]};
        const float wq = m[12] * x + m[13] * y + m[14] * z + m[15];
        if (wq != 1.0f) { q[0] /= wq; q[1] /= wq; q[2] /= wq; }
        for (int a = 0; a < 3; a++) {
            out_lo[a] = c == 0 ? q[a] : std::fmin(out_lo[a], q[a]);
            out_hi[a] = c == 0 ? q[a] : std::fmax(out_hi[a], q[a]);
        }
    }
}
void box_union(float lo[3], float hi[3], const float lo2[3], const float hi2[3]) {
    for (int a = 0; a < 3; a++) { lo[a] = std::fmin(lo[a], lo2[a]); hi[a] = std::fmax(hi[a], hi2[a]); }
}
bool affine(const float* m) { return m[12] == 0.0f && m[13] == 0.0f && m[14] == 0.0f && m[15] == 1.0f; }

}  // namespace

namespace ptmotion {

bool decompose(const float m[16], float T[3], float R[4], float S[3]) {
    const float epsilon = 1.1920929e-7f * 1e+2f;       // AnimatedTransform::new: Float::EPSILON * 1e+2, at most 100 rounds
    const int max_count = 100;
    T[0] = m[3]; T[1] = m[7]; T[2] = m[11];
    M44 mm;
    std::memcpy(mm.a, m, sizeof(mm.a));
    for (int i = 0; i < 3; i++) mm.a[4 * i + 3] = 0.0f;
    mm.a[15] = 1.0f;
    M44 r = mm;
    // the reference's own step: the COLUMN lengths divide the ROWS
    const float sx = length3(r.a[0], r.a[4], r.a[8]), sy = length3(r.a[1], r.a[5], r.a[9]), sz = length3(r.a[2], r.a[6], r.a[10]);
    if (sx != 0.0f) { r.a[0] /= sx; r.a[1] /= sx; r.a[2] /= sx; }
    if (sy != 0.0f) { r.a[4] /= sy; r.a[5] /= sy; r.a[6] /= sy; }
    if (sz != 0.0f) { r.a[8] /= sz; r.a[9] /= sz; r.a[10] /= sz; }
    int count = 0;
    float norm = 0.0f;                                  // never reset: it only grows, so a first step above epsilon runs all 100
    M44 tmp;
    do {
        if (!pth::m_inverse(r, &tmp)) return false;     // assert!(invertible(&r))
        M44 r_it;
        if (!pth::m_inverse(transpose(r), &r_it)) return false;
        M44 r_next = r;
        for (int i = 0; i < 16; i++) r_next.a[i] = lerp(0.5f, r.a[i], r_it.a[i]);
        M44 ir_next;
        if (!pth::m_inverse(r_next, &ir_next)) return false;      // assert!(invertible(&r_next))
        M44 is;
        if (pth::m_inverse(suppress_for_scale(pth::m_mul(ir_next, mm)), &is)) r_next = pth::m_mul(mm, is);
        r_next = quat_to_matrix(quat_normalize(quat_from_matrix(r_next)));      // re-projected through a quaternion every round
        for (int i = 0; i < 3; i++) {
            const float n = std::fabs(r.a[4 * i] - r_next.a[4 * i]) + std::fabs(r.a[4 * i + 1] - r_next.a[4 * i + 1]) + std::fabs(r.a[4 * i + 2] - r_next.a[4 * i + 2]);
            norm = std::fmax(norm, n);
        }
        r = r_next;
        count++;
    } while (count < max_count && norm > epsilon);
    M44 ir;
    if (!pth::m_inverse(r, &ir)) return false;
    const M44 s = suppress_for_scale(pth::m_mul(ir, mm));
    M44 is;
    if (pth::m_inverse(s, &is)) r = pth::m_mul(mm, is);
    const Quat q = quat_normalize(quat_from_matrix(r));
    R[0] = q.x; R[1] = q.y; R[2] = q.z; R[3] = q.w;
    S[0] = s.a[0]; S[1] = s.a[5]; S[2] = s.a[10];
    for (int i = 0; i < 3; i++) if (!std::isfinite(T[i]) || !std::isfinite(S[i])) return false;
    for (int i = 0; i < 4; i++) if (!std::isfinite(R[i])) return false;
    return true;
}

bool make_record(const float m0[16], const float inv0[16], const float m1[16], const float inv1[16], const float times[2], PtMotion* out, bool* has_rotation) {
    PtMotion mo;
    std::memset(&mo, 0, sizeof(mo));
    if (!decompose(m0, mo.T[0], mo.R[0], mo.S[0]) || !decompose(m1, mo.T[1], mo.R[1], mo.S[1])) return false;
    const Quat q0{mo.R[0][0], mo.R[0][1], mo.R[0][2], mo.R[0][3]};
    Quat q1{mo.R[1][0], mo.R[1][1], mo.R[1][2], mo.R[1][3]};
    if (quat_dot(q0, q1) < 0.0f) { q1 = Quat{-q1.x, -q1.y, -q1.z, -q1.w}; mo.R[1][0] = q1.x; mo.R[1][1] = q1.y; mo.R[1][2] = q1.z; mo.R[1][3] = q1.w; }
    *has_rotation = quat_dot(q0, q1) < 0.9995f;
    mo.times[0] = times[0]; mo.times[1] = times[1];
    std::memcpy(mo.m1, m1, 48); std::memcpy(mo.minv1, inv1, 48);
    bool same = true;                                   // Transform's derived PartialEq: m and m_inv, entry by entry
    for (int i = 0; i < 16; i++) if (!(m0[i] == m1[i]) || !(inv0[i] == inv1[i])) same = false;
    mo.animated = same ? 0u : 1u;
    *out = mo;
    return true;
}

void motion_bounds(const PtMotion& mo, bool has_rotation, const float m0[16], const float end16[16], const float lo[3], const float hi[3], float out_lo[3], float out_hi[3]) {
    transform_bounds(m0, lo, hi, out_lo, out_hi);
    if (!mo.animated) return;
    float lo2[3], hi2[3];
    transform_bounds(end16, lo, hi, lo2, hi2);
    box_union(out_lo, out_hi, lo2, hi2);
    if (!has_rotation) return;
    for (int i = 0; i < 64; i++) {
        const float t = lerp((float)i / 64.0f, mo.times[0], mo.times[1]);
        float m[16], minv[12];
        if (t <= mo.times[0]) std::memcpy(m, m0, 64);
        else if (mo.times[1] <= t) std::memcpy(m, end16, 64);
        else {
            if (!pt_motion_interpolate(mo, t, m, minv)) continue;
            m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = 1.0f;
        }
        transform_bounds(m, lo, hi, lo2, hi2);
        box_union(out_lo, out_hi, lo2, hi2);
    }
    for (int a = 0; a < 3; a++) {                       // expand_bounds(.., 0.1)
        const float d = (out_hi[a] - out_lo[a]) * 0.1f;
        out_lo[a] = out_lo[a] - d; out_hi[a] = out_hi[a] + d;
    }
}

}  // namespace ptmotion

extern "C" {

pt_status pt_motion_decompose(const float* m, float* T, float* R, float* S) {
    if (!m || !T || !R || !S) return PT_ERR_INVALID_ARGUMENT;
    return ptmotion::decompose(m, T, R, S) ? PT_OK : PT_ERR_INVALID_ARGUMENT;
}

pt_status pt_motion_bounds(const float* start, const float* end, const float* times, const float* box, float* out) {
    if (!start || !end || !times || !box || !out) return PT_ERR_INVALID_ARGUMENT;
    if (!affine(start) || !affine(end)) return PT_ERR_INVALID_ARGUMENT;
    M44 s, e, si, ei;
    std::memcpy(s.a, start, 64); std::memcpy(e.a, end, 64);
    if (!pth::m_inverse(s, &si) || !pth::m_inverse(e, &ei)) return PT_ERR_INVALID_ARGUMENT;
    PtMotion mo;
    bool has_rotation = false;
    if (!ptmotion::make_record(start, si.a, end, ei.a, times, &mo, &has_rotation)) return PT_ERR_INVALID_ARGUMENT;
    ptmotion::motion_bounds(mo, has_rotation, start, end, box, box + 3, out, out + 3);
    return PT_OK;
}

}
