// pt_motion.h -- AnimatedTransform::interpolate (core/transform/animated_transform.rs:63-81) in float32, operation for operation, as one
// function that the host (motion_bounds, pt_motion.cpp) and the fifth build of the kernels (pt_kernels_motion.hip) both compile:
//   dt = (time - t0) / (t1 - t0);  T = (1 - dt) T0 + dt T1;  R = slerp(dt, R0, R1) (quaternion.rs:45-55: dot clamped to [0, 1], no
//   renormalisation);  S = (1 - dt) S0 + dt S1;  M = translate(T) * R.to_matrix() * scale(S);  Transform::from(M) inverts M with
//   Matrix4x4::inverse (Gauss-Jordan, full pivoting, matrix4x4.rs:209-282).
// The two clamped branches (not actually animated or time <= t0; t1 <= time) hand back the stored matrices and the stored inverses, the
// ones a static instance uses.  The products with translate() and scale() are written out: their zero terms only ever add +-0 to an
// entry, so the entries agree with the reference's 4 x 4 products except, possibly, in the sign of a zero.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PT_MOTION_FN __host__ __device__ inline
#else
#define PT_MOTION_FN inline
#endif

// One AnimatedTransform as the device reads it (192 bytes).  The start transform is not here: an instance's is PtInstance::m / minv, the
// camera's PtCamera::camera_to_world.
struct PtMotion {
    float T[2][3];               // decompose() of the two ends: translation,
    float R[2][4];               //   rotation quaternions x y z w (R[1] negated when the dot was negative),
    float S[2][3];               //   the diagonal of the scale
    float times[2];              // TransformTimes
    float m1[12];                // rows 0..2 of the end transform
    float minv1[12];             // rows 0..2 of its stored inverse
    uint32_t animated;           // actually_animated: the two ends differ
    uint32_t pad;
};
static_assert(sizeof(PtMotion) == 192, "PtMotion records follow the PtInstance records in one buffer");

// Matrix4x4::inverse on a full 4 x 4 (row-major); false: singular
PT_MOTION_FN bool pt_motion_inverse4(const float* src, float* w) {
    int col_of[4], row_of[4], used[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; i++) w[i] = src[i];
    for (int step = 0; step < 4; step++) {
        int prow = 0, pcol = 0;
        float best = 0.0f;
        for (int r = 0; r < 4; r++) {
            if (used[r] == 1) continue;
            for (int c = 0; c < 4; c++) {
                if (used[c] == 0) {
                    const float v = fabsf(w[4 * r + c]);
                    if (v >= best) { best = v; prow = r; pcol = c; }
                } else if (used[c] > 1) return false;
            }
        }
        used[pcol]++;
        if (prow != pcol)
            for (int k = 0; k < 4; k++) { const float t = w[4 * prow + k]; w[4 * prow + k] = w[4 * pcol + k]; w[4 * pcol + k] = t; }
        row_of[step] = prow; col_of[step] = pcol;
        if (w[4 * pcol + pcol] == 0.0f) return false;
        const float inv = 1.0f / w[4 * pcol + pcol];
        w[4 * pcol + pcol] = 1.0f;
        for (int k = 0; k < 4; k++) w[4 * pcol + k] *= inv;
        for (int r = 0; r < 4; r++) {
            if (r == pcol) continue;
            const float f = w[4 * r + pcol];
            w[4 * r + pcol] = 0.0f;
            for (int k = 0; k < 4; k++) w[4 * r + k] -= w[4 * pcol + k] * f;
        }
    }
    for (int step = 3; step >= 0; step--)
        if (row_of[step] != col_of[step])
            for (int k = 0; k < 4; k++) { const float t = w[4 * k + row_of[step]]; w[4 * k + row_of[step]] = w[4 * k + col_of[step]]; w[4 * k + col_of[step]] = t; }
    return true;
}

// Quaternion::to_matrix (quaternion.rs:57-84), rows 0..2 x columns 0..2 of the transposed result
PT_MOTION_FN void pt_motion_quat_matrix(const float* q, float* r9) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = x * w, wy = y * w, wz = z * w;
    r9[0] = 1.0f - 2.0f * (yy + zz); r9[3] = 2.0f * (xy + wz);        r9[6] = 2.0f * (xz - wy);
    r9[1] = 2.0f * (xy - wz);        r9[4] = 1.0f - 2.0f * (xx + zz); r9[7] = 2.0f * (yz + wx);
    r9[2] = 2.0f * (xz + wy);        r9[5] = 2.0f * (yz - wx);        r9[8] = 1.0f - 2.0f * (xx + yy);
}

// The reference's acos and sin are glibc's acosf and sinf.  The host calls them; the kernels pass their own restatements of the two
// (pt_acosf, pt_sincosf of pt_device_math.h: the same bits as libm.so.6), so both sides interpolate the same matrices.
struct PtMotionLibm {
    static PT_MOTION_FN float acos(float x) { return acosf(x); }
    static PT_MOTION_FN float sin(float x) { return sinf(x); }
};

// Quaternion::slerp (quaternion.rs:45-55)
template <class M>
PT_MOTION_FN void pt_motion_slerp(float t, const float* q1, const float* q2, float* out) {
    float c = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3];
    c = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
    if (c > 1.0f - 1.1920929e-7f) { for (int i = 0; i < 4; i++) out[i] = q1[i]; return; }
    const float theta = M::acos(c);
    const float s = 1.0f / M::sin(theta);
    const float a = M::sin((1.0f - t) * theta), b = M::sin(t * theta);
    for (int i = 0; i < 4; i++) out[i] = (q1[i] * a + q2[i] * b) * s;
}

// The interpolating branch: rows 0..2 of M(time) and of its Gauss-Jordan inverse.  false: M(time) is singular (the reference's
// Transform::from would panic); the outputs are then untouched.
template <class M = PtMotionLibm>
PT_MOTION_FN bool pt_motion_interpolate(const PtMotion& mo, float time, float* m, float* minv) {
    const float dt = (time - mo.times[0]) / (mo.times[1] - mo.times[0]);
    float tr[3], sc[3], q[4], r9[9];
    for (int i = 0; i < 3; i++) tr[i] = (1.0f - dt) * mo.T[0][i] + dt * mo.T[1][i];
    pt_motion_slerp<M>(dt, mo.R[0], mo.R[1], q);
    for (int i = 0; i < 3; i++) sc[i] = (1.0f - dt) * mo.S[0][i] + dt * mo.S[1][i];
    pt_motion_quat_matrix(q, r9);
    float full[16], inv[16];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) full[4 * i + j] = (r9[3 * i + j] + 0.0f) * sc[j] + 0.0f;
        full[4 * i + 3] = tr[i] + 0.0f;
    }
    full[12] = 0.0f; full[13] = 0.0f; full[14] = 0.0f; full[15] = 1.0f;
    if (!pt_motion_inverse4(full, inv)) return false;
    for (int i = 0; i < 12; i++) { m[i] = full[i]; minv[i] = inv[i]; }
    return true;
}

// AnimatedTransform::interpolate: the transform at `time` as the pair (m, minv), rows 0..2.  m0 / minv0: the stored start transform.
template <class M = PtMotionLibm>
PT_MOTION_FN void pt_motion_at(const PtMotion& mo, const float* m0, const float* minv0, float time, float* m, float* minv) {
    if (!mo.animated || time <= mo.times[0]) { for (int i = 0; i < 12; i++) { m[i] = m0[i]; minv[i] = minv0[i]; } return; }
    if (mo.times[1] <= time) { for (int i = 0; i < 12; i++) { m[i] = mo.m1[i]; minv[i] = mo.minv1[i]; } return; }
    if (!pt_motion_interpolate<M>(mo, time, m, minv)) for (int i = 0; i < 12; i++) { m[i] = m0[i]; minv[i] = minv0[i]; }
}

// ---- host side (pt_motion.cpp)
namespace ptmotion {
// decompose() (core/transform/decompose.rs) in float32: T, R (x y z w), S (the diagonal of R^-1 M); false where the reference gives None or panics
bool decompose(const float m[16], float T[3], float R[4], float S[3]);
// AnimatedTransform::new: the record of the pair (start, end), each given as Transform.m / Transform.m_inv; false: decompose failed
bool make_record(const float m0[16], const float inv0[16], const float m1[16], const float inv1[16], const float times[2], PtMotion* out, bool* has_rotation);
// AnimatedTransform::motion_bounds of the box lo..hi; m0: the start transform's matrix
void motion_bounds(const PtMotion& mo, bool has_rotation, const float m0[16], const float end16[16], const float lo[3], const float hi[3], float out_lo[3], float out_hi[3]);
}
