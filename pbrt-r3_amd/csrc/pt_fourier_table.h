// pt_fourier_table.h -- the rules a tabulated BSDF (pt_fourier_table, include/pbrtgpu.h) has to keep before the device may read it, in one
// place for the file reader (host/pth_fourier.cpp) and the upload (pt_scene_upload.cpp).  The reference trusts the file
// (FourierBSDFTable::read_body, core/reflection/fourier.rs:90-161); a kernel that follows an offset out of the coefficient array cannot.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include "../../include/pbrtgpu.h"

// Empty: the table is fit to upload.  Otherwise the refusal, by name.
inline std::string pt_fourier_table_refusal(const pt_fourier_table& t) {
    if (t.n_channels != 1 && t.n_channels != 3) return "n_channels is " + std::to_string(t.n_channels) + " (1 or 3 are taken)";
    if (t.n_mu < 2) return "n_mu is " + std::to_string(t.n_mu) + " (a spline needs two nodes)";
    if (t.n_mu > 32768) return "n_mu is " + std::to_string(t.n_mu) + " (at most 32768: n_mu * n_mu entries are indexed with 32 bits)";
    if (t.m_max < 0 || t.n_coeffs < 0) return "m_max or n_coeffs is negative";
    if (!t.mu || !t.cdf || !t.offset_and_length || (t.n_coeffs > 0 && !t.a)) return "an array is missing";
    for (int32_t i = 0; i < t.n_mu; i++) {
        if (!std::isfinite(t.mu[i])) return "mu[" + std::to_string(i) + "] is not finite";
        // (never decreasing, not strictly increasing: measured tables carry the node 0 twice, once for each side of the surface -- the
        // reference's own fixture does.  catmull_rom_weights never lands in the empty interval between the two: it takes the last node
        // that is <= x.  The cdf search of sample_catmull_rom_2d stays out of it exactly when the two nodes' cdf columns are equal, as
        // integrating over an interval of width 0 leaves them; with columns that differ it would divide by that width, so such a pair
        // is refused)
        if (i > 0 && t.mu[i] < t.mu[i - 1]) return "mu steps back at node " + std::to_string(i);
        if (i > 0 && t.mu[i] == t.mu[i - 1])
            for (int32_t o = 0; o < t.n_mu; o++)
                if (!(t.cdf[(int64_t)o * t.n_mu + i] == t.cdf[(int64_t)o * t.n_mu + i - 1]))
                    return "mu repeats at node " + std::to_string(i) + " and the cdf columns of the two nodes differ (row " + std::to_string(o) + ")";
    }
    const int64_t n2 = (int64_t)t.n_mu * t.n_mu;
    for (int64_t i = 0; i < n2; i++) {
        const int64_t offset = t.offset_and_length[2 * i], length = t.offset_and_length[2 * i + 1];
        if (length < 0) return "node pair " + std::to_string(i) + " has a negative length";
        if (length > t.m_max) return "node pair " + std::to_string(i) + " has a length above m_max";
        if (offset < 0) return "node pair " + std::to_string(i) + " has a negative offset";
        if (offset + (int64_t)t.n_channels * length > t.n_coeffs) return "node pair " + std::to_string(i) + " has coefficients past the end of the array";
    }
    return std::string();
}
