// pt_fourier.h -- FourierBSDF (core/reflection/fourier.rs:178-465) over a PtFourierTable, with the spline and series code it calls
// (core/interpolation/catmul_rom.rs:3-179, core/interpolation/fourier.rs:4-89), in the reference's float32 operations and order.
// Included by pt_bxdf.h when PT_FOURIER is set, that is by the kernels of pt_kernels_fourier.hip only.
//
// The coefficients a_k of one (mu_i, mu_o) are never stored.  create_ak (fourier.rs:206-247) adds, for k < m of each of up to sixteen
// node pairs whose weight is not zero, weight * a[offset + c * m + k] to a sum that starts at 0.0, pair by pair with b outer and a
// inner; a_k depends on k alone, so fourier_ak below forms it from its gathers at the place the series consumes it and gets the
// reference's value bit for bit, with no array of m_max floats per lane.  sample_fourier reads the luminance coefficients once per
// Newton iteration: they are formed again each time (DESIGN.md section 9 has the reasons), so no table is too long for the kernels.
//
// The loop caps.  sample_catmull_rom_2d and sample_fourier iterate until a residual or a bracket is below 1e-6, with no bound on the
// count.  Over every sampling input of the tests (tests/fourier_cases.py: four tables, 1 936 samples each, u at 0, at 1 - 2^-24 and at one
// half among them) the float32 restatement on the CPU (tests/fourier_ref.py) takes at most 9 iterations in the first loop and 19 in the
// second (fourier_cases.iteration_maxima; a test holds the caps to four times that).  The device stops at PT_FOURIER_MU_ITERS = 48 and
// PT_FOURIER_PHI_ITERS = 96, returns "no sample" and counts the sample in PtFourierTable::capped (pt_scene_info.fourier_capped).
#pragma once

#define PT_FOURIER_MU_ITERS 48
#define PT_FOURIER_PHI_ITERS 96

PT_DEV const PtFourierTable* fourier_table(const PtLobe& l) {
    const uint64_t a = (uint64_t)__float_as_uint(l.t[0]) | ((uint64_t)__float_as_uint(l.t[1]) << 32);
    return reinterpret_cast<const PtFourierTable*>(a);
}

// catmull_rom_weights (catmul_rom.rs:3-60).  false: x lies outside [nodes[0], nodes[size - 1]] (or is NaN).
PT_DEV bool fourier_weights(const float* nodes, int size, float x, int* offset, float* w) {
    if (!(x >= nodes[0] && x <= nodes[size - 1])) return false;
    int first = 0, len = size;                                  // find_interval (base/functions.rs:105-120) with v[i] <= x
    while (len > 0) {
        const int half = len >> 1, middle = first + half;
        if (nodes[middle] <= x) { first = middle + 1; len -= half + 1; }
        else len = half;
    }
    const int idx = min(max(first - 1, 0), size - 2);
    *offset = idx - 1;
    const float x0 = nodes[idx], x1 = nodes[idx + 1];
    const float t = (x - x0) / (x1 - x0);
    const float t2 = t * t;
    const float t3 = t2 * t;
    w[1] = 2.0f * t3 - 3.0f * t2 + 1.0f;
    w[2] = -2.0f * t3 + 3.0f * t2;
    if (idx > 0) {
        const float w0 = (t3 - 2.0f * t2 + t) * (x1 - x0) / (x1 - nodes[idx - 1]);
        w[0] = -w0;
        w[2] += w0;
    } else {
        const float w0 = t3 - 2.0f * t2 + t;
        w[0] = 0.0f;
        w[1] -= w0;
        w[2] += w0;
    }
    if (idx + 2 < size) {
        const float w3 = (t3 - t2) * (x1 - x0) / (nodes[idx + 2] - x0);
        w[1] -= w3;
        w[3] = w3;
    } else {
        const float w3 = t3 - t2;
        w[1] -= w3;
        w[2] += w3;
        w[3] = 0.0f;
    }
    return true;
}

// The sixteen node pairs of create_ak: weight, length and offset of pair 4 * b + a (a pair of weight zero is left out, as there: its
// length is 0 here), and the series length m_max = max(1, lengths).  Every loop over it is unrolled, so no index is a runtime value;
// all the same the compiler keeps most of the 48 words in scratch across the k loops (fourier_ak reads each under a runtime
// `k < A.m[j]`): they are the scratch the shading kernels of this build gain (k_shade_general 80 -> 312 bytes, k_bsdf_eval 16 -> 108;
// profiles/fourier_kernel_resources.txt).  A performance change starts there.
struct FourierAk {
    float w[16];
    int m[16];
    int off[16];
    int m_max;
};
PT_DEV void fourier_ak_setup(const PtFourierTable& T, int offset_i, const float* weights_i, int offset_o, const float* weights_o, FourierAk& A) {
    const int n_mu = (int)T.n_mu;
    A.m_max = 1;
#pragma unroll
    for (int b = 0; b < 4; b++) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const float weight = weights_i[a] * weights_o[b];
            A.w[4 * b + a] = weight;
            A.m[4 * b + a] = 0;
            A.off[4 * b + a] = 0;
            if (weight != 0.0f) {                               // get_ak (fourier.rs:167-175): it clamps both offsets
                const int oi = min(max(offset_i + a, 0), n_mu - 1), oo = min(max(offset_o + b, 0), n_mu - 1);
                const int pair = oo * n_mu + oi;
                A.m[4 * b + a] = T.m[pair];
                A.off[4 * b + a] = T.a_offset[pair];
                A.m_max = max(A.m_max, A.m[4 * b + a]);
            }
        }
    }
}
// a_k of channel c.  Plain dword loads: offsets in real tables have no alignment.
PT_DEV float fourier_ak(const PtFourierTable& T, const FourierAk& A, int c, int k) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (k < A.m[j]) v += A.w[j] * T.a[A.off[j] + c * A.m[j] + k];
    return v;
}
// cos_d_phi (reflection/math.rs:70-81); the clamp keeps a NaN, as f32::clamp does
PT_DEV float fourier_cos_d_phi(V3 wa, V3 wb) {
    const float waxy = wa.x * wa.x + wa.y * wa.y, wbxy = wb.x * wb.x + wb.y * wb.y;
    if (waxy <= 0.0f || wbxy <= 0.0f) return 1.0f;
    const float v = (wa.x * wb.x + wa.y * wb.y) / sqrtf(waxy * wbxy);
    return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}
// 1 / |mu_i| (0 at mu_i == 0), times eta^2 or 1 / eta^2 on the reflection side of the table's convention: the transport mode of this
// path is always radiance (fourier.rs:287-300)
PT_DEV float fourier_scale(const PtFourierTable& T, float mu_i, float mu_o) {
    float scale = mu_i != 0.0f ? 1.0f / fabsf(mu_i) : 0.0f;
    if (mu_i * mu_o > 0.0f) {
        const float eta = mu_i > 0.0f ? 1.0f / T.eta : T.eta;
        scale *= eta * eta;
    }
    return scale;
}
// evaluate_fourier (interpolation/fourier.rs:4-17) of the channels the caller wants, in one pass over k: the cosine iterates are shared,
// each channel's sum is its own and grows in increasing k
PT_DEV void fourier_series(const PtFourierTable& T, const FourierAk& A, float cos_phi, bool with_y, bool with_rb, float* y, float* r, float* b) {
    float vy = 0.0f, vr = 0.0f, vb = 0.0f;
    float cos_kminus_one_phi = cos_phi, cos_kphi = 1.0f;
    for (int k = 0; k < A.m_max; k++) {
        if (with_y) vy += fourier_ak(T, A, 0, k) * cos_kphi;
        if (with_rb) {
            vr += fourier_ak(T, A, 1, k) * cos_kphi;
            vb += fourier_ak(T, A, 2, k) * cos_kphi;
        }
        const float cos_kplus_one_phi = 2.0f * cos_phi * cos_kphi - cos_kminus_one_phi;
        cos_kminus_one_phi = cos_kphi;
        cos_kphi = cos_kplus_one_phi;
    }
    *y = vy; *r = vr; *b = vb;
}
PT_DEV V3 fourier_rgb(float y, float r, float b, float scale) {                 // fourier.rs:305-309; clamp_zero is f32::clamp(0, inf) per channel: a NaN stays
    const float g = 1.39829f * y - 0.100913f * b - 0.297375f * r;
    const float cr = r * scale, cg = g * scale, cb = b * scale;
    return mk3(cr < 0.0f ? 0.0f : cr, cg < 0.0f ? 0.0f : cg, cb < 0.0f ? 0.0f : cb);
}

__device__ __noinline__ V3 fourier_f(const PtLobe& l, V3 wo, V3 wi) {           // fourier.rs:251-313
    const PtFourierTable& T = *fourier_table(l);
    const V3 mwi = mk3(-wi.x, -wi.y, -wi.z);
    const float mu_i = mwi.z, mu_o = wo.z;
    const float cos_phi = fourier_cos_d_phi(mwi, wo);
    int offset_i, offset_o;
    float weights_i[4], weights_o[4];
    if (!fourier_weights(T.mu, (int)T.n_mu, mu_i, &offset_i, weights_i) || !fourier_weights(T.mu, (int)T.n_mu, mu_o, &offset_o, weights_o))
        return mk3(0.0f, 0.0f, 0.0f);
    FourierAk A;
    fourier_ak_setup(T, offset_i, weights_i, offset_o, weights_o, A);
    float y, r, b;
    fourier_series(T, A, cos_phi, true, T.n_channels != 1u, &y, &r, &b);
    y = fmaxf(0.0f, y);
    const float scale = fourier_scale(T, mu_i, mu_o);
    if (T.n_channels == 1u) { const float v = y * scale; return mk3(v, v, v); }
    return fourier_rgb(y, r, b, scale);
}

__device__ __noinline__ float fourier_pdf(const PtLobe& l, V3 wo, V3 wi) {     // fourier.rs:417-456: the luminance channel alone
    const PtFourierTable& T = *fourier_table(l);
    const V3 mwi = mk3(-wi.x, -wi.y, -wi.z);
    const float mu_i = mwi.z, mu_o = wo.z;
    const float cos_phi = fourier_cos_d_phi(mwi, wo);
    int offset_i, offset_o;
    float weights_i[4], weights_o[4];
    if (!fourier_weights(T.mu, (int)T.n_mu, mu_i, &offset_i, weights_i) || !fourier_weights(T.mu, (int)T.n_mu, mu_o, &offset_o, weights_o)) return 0.0f;
    FourierAk A;
    fourier_ak_setup(T, offset_i, weights_i, offset_o, weights_o, A);
    const int n_mu = (int)T.n_mu;
    float rho = 0.0f;
#pragma unroll
    for (int o = 0; o < 4; o++) {
        if (weights_o[o] == 0.0f) continue;
        const int index = min(max(offset_o + o, 0), n_mu - 1);
        rho += weights_o[o] * T.cdf[index * n_mu + n_mu - 1] * (2.0f * PT_PI);
    }
    float y, r, b;
    fourier_series(T, A, cos_phi, true, false, &y, &r, &b);
    return (rho > 0.0f && y > 0.0f) ? y / rho : 0.0f;
}

// `interpolate` of sample_catmull_rom_2d (catmul_rom.rs:77-89).  The reference indexes row offset + i unclamped, which is in range
// wherever the weight is not zero; the clamp here changes nothing then and keeps a load inside the table whatever the weights are.
PT_DEV float fourier_interp(const float* array, int n, int offset, const float* w, int idx) {
    float value = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (w[i] != 0.0f) value += array[min(max(offset + i, 0), n - 1) * n + idx] * w[i];
    return value;
}
// sample_catmull_rom_2d (catmul_rom.rs:62-179) with nodes1 = nodes2 = mu, values = a0.  0: no sample (alpha outside the nodes),
// 1: a sample, 2: the Newton-bisection reached PT_FOURIER_MU_ITERS.
PT_DEV int fourier_sample_mu(const PtFourierTable& T, float alpha, float u, float* value, float* pdf) {
    const int n = (int)T.n_mu;
    int offset;
    float w[4];
    if (!fourier_weights(T.mu, n, alpha, &offset, w)) return 0;
    const float maximum = fourier_interp(T.cdf, n, offset, w, n - 1);
    u *= maximum;
    int first = 0, len = n;                                     // find_interval_range((0, n), ..) with interpolate(cdf, i) <= u
    while (len > 0) {
        const int half = len >> 1, middle = first + half;
        if (fourier_interp(T.cdf, n, offset, w, middle) <= u) { first = middle + 1; len -= half + 1; }
        else len = half;
    }
    // usize::clamp(first - 1, 0, n - 2): with first == 0 (u is NaN or negative) the subtraction wraps and the clamp gives n - 2
    const int idx = first == 0 ? n - 2 : min(first - 1, n - 2);
    const float f0 = fourier_interp(T.a0, n, offset, w, idx), f1 = fourier_interp(T.a0, n, offset, w, idx + 1);
    const float x0 = T.mu[idx], x1 = T.mu[idx + 1];
    const float width = x1 - x0;
    u = (u - fourier_interp(T.cdf, n, offset, w, idx)) / width;
    const float d0 = idx > 0 ? width * (f1 - fourier_interp(T.a0, n, offset, w, idx - 1)) / (x1 - T.mu[idx - 1]) : f1 - f0;
    const float d1 = idx + 2 < n ? width * (fourier_interp(T.a0, n, offset, w, idx + 2) - f0) / (T.mu[idx + 2] - x0) : f1 - f0;
    float t = f0 != f1 ? (f0 - sqrtf(fmaxf(0.0f, f0 * f0 + 2.0f * u * (f1 - f0)))) / (f0 - f1) : u / f0;
    float a = 0.0f, b = 1.0f, fhat = 0.0f;
    int it = 0;
    for (;; it++) {
        if (it == PT_FOURIER_MU_ITERS) return 2;
        if (!(t >= a && t <= b)) t = 0.5f * (a + b);
        const float t_fhat = t * (f0 + t * (0.5f * d0 + t * ((1.0f / 3.0f) * (-2.0f * d0 - d1) + f1 - f0 + t * (0.25f * (d0 + d1) + 0.5f * (f0 - f1)))));
        fhat = f0 + t * (d0 + t * (-2.0f * d0 - d1 + 3.0f * (f1 - f0) + t * (d0 + d1 + 2.0f * (f0 - f1))));
        if (fabsf(t_fhat - u) < 1e-6f || b - a < 1e-6f) break;
        if (t_fhat - u < 0.0f) a = t; else b = t;
        t -= (t_fhat - u) / fhat;
    }
    *pdf = fhat / maximum;
    *value = x0 + width * t;
    return 1;
}
// sample_fourier (interpolation/fourier.rs:19-89) over the luminance coefficients of A: float64 where the reference has f64, the
// device's cos(double) for f64::cos (the iteration stops at 1e-6, so the last bits of the cosine move the result below that).
// false: the iteration reached PT_FOURIER_PHI_ITERS.
PT_DEV bool fourier_sample_phi(const PtFourierTable& T, const FourierAk& A, float u, float* y_out, float* pdf_out, float* phi_out) {
    const bool flip = u >= 0.5f;
    if (flip) u = 1.0f - 2.0f * (u - 0.5f);
    else u *= 2.0f;
    double a = 0.0, b = (double)PT_PI, phi = 0.5 * (double)PT_PI;
    const float ak0 = fourier_ak(T, A, 0, 0);
    double f = 0.0;
    int it = 0;
    for (;; it++) {
        if (it == PT_FOURIER_PHI_ITERS) return false;
        const double cos_phi = cos(phi);
        const double sin_phi = sqrt(fmax(0.0, 1.0 - cos_phi * cos_phi));
        double cos_phi_prev = cos_phi, cos_phi_cur = 1.0;
        double sin_phi_prev = -sin_phi, sin_phi_cur = 0.0;
        double tf = (double)ak0 * phi;
        f = (double)ak0;
        for (int k = 1; k < A.m_max; k++) {
            const double sin_phi_next = 2.0 * cos_phi * sin_phi_cur - sin_phi_prev;
            const double cos_phi_next = 2.0 * cos_phi * cos_phi_cur - cos_phi_prev;
            sin_phi_prev = sin_phi_cur; sin_phi_cur = sin_phi_next;
            cos_phi_prev = cos_phi_cur; cos_phi_cur = cos_phi_next;
            const float akk = fourier_ak(T, A, 0, k);
            tf += (double)(akk * T.recip[k]) * sin_phi_next;
            f += (double)akk * cos_phi_next;
        }
        tf -= (double)(u * ak0 * PT_PI);
        if (tf > 0.0) b = phi; else a = phi;
        if (fabs(tf) < 1e-6 || b - a < 1e-6) break;
        phi -= tf / f;
        if (!(phi > a && phi < b)) phi = 0.5 * (a + b);
    }
    if (flip) phi = (double)(2.0f * PT_PI) - phi;
    *pdf_out = (PT_INV_PI * 0.5f) / ak0 * (float)f;
    *y_out = (float)f;
    *phi_out = (float)phi;
    return true;
}

__device__ __noinline__ bool fourier_sample_f(const PtLobe& l, V3 wo, V2 u, V3* f_out, V3* wi_out, float* pdf_out) {          // fourier.rs:315-415
    const PtFourierTable* Tp = fourier_table(l);
    const PtFourierTable& T = *Tp;
    const float mu_o = wo.z;
    float mu_i, pdf_mu;
    const int got = fourier_sample_mu(T, mu_o, u.y, &mu_i, &pdf_mu);           // u[1] picks mu_i, u[0] picks phi
    if (got == 2) atomicAdd(const_cast<uint32_t*>(&Tp->capped), 1u);
    if (got != 1) return false;
    // pdf = max(0, pdf_phi * pdf_mu) and "pdf <= 0 is no sample": a pdf_mu of 0 or NaN (a row without energy: maximum == 0) ends there
    // whatever pdf_phi turns out to be, so the series need not be looked at
    if (pdf_mu == 0.0f || pdf_mu != pdf_mu) return false;
    int offset_i, offset_o;
    float weights_i[4], weights_o[4];
    if (!fourier_weights(T.mu, (int)T.n_mu, mu_i, &offset_i, weights_i) || !fourier_weights(T.mu, (int)T.n_mu, mu_o, &offset_o, weights_o)) return false;
    FourierAk A;
    fourier_ak_setup(T, offset_i, weights_i, offset_o, weights_o, A);
    float y, pdf_phi, phi;
    if (!fourier_sample_phi(T, A, u.x, &y, &pdf_phi, &phi)) {
        atomicAdd(const_cast<uint32_t*>(&Tp->capped), 1u);
        return false;
    }
    const float pdf = fmaxf(0.0f, pdf_phi * pdf_mu);
    if (pdf <= 0.0f) return false;
    const float sin2_theta_i = fmaxf(0.0f, 1.0f - mu_i * mu_i);
    float norm = sqrtf(sin2_theta_i / fmaxf(0.0f, 1.0f - wo.z * wo.z));
    if (isinf(norm)) norm = 0.0f;
    float sin_phi, cos_phi;
    pt_sincosf(phi, &sin_phi, &cos_phi);
    const V3 v = normalize(mk3(norm * (cos_phi * wo.x - sin_phi * wo.y), norm * (sin_phi * wo.x + cos_phi * wo.y), mu_i));
    *wi_out = mk3(-v.x, -v.y, -v.z);
    const float scale = fourier_scale(T, mu_i, mu_o);
    if (T.n_channels == 1u) { const float s = y * scale; *f_out = mk3(s, s, s); }
    else {
        float y2, r, b;
        fourier_series(T, A, cos_phi, false, true, &y2, &r, &b);
        *f_out = fourier_rgb(y, r, b, scale);
    }
    *pdf_out = pdf;
    return true;
}
