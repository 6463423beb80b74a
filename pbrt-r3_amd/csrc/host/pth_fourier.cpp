// pth_fourier.cpp -- FourierBSDFTable::read (src/core/reflection/fourier.rs:52-161) for the front end, the command line and Python: one
// reader, and behind it the rules the upload also applies (pt_fourier_table.h), because a kernel follows the offsets the file gives.
#include "pth_fourier.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>

#include "../pt_fourier_table.h"

namespace {

pt_status refuse(const char* filename, const std::string& why, char* err, size_t err_cap) {
    if (err && err_cap) std::snprintf(err, err_cap, "Tabulated BSDF file \"%s\": %s", filename, why.c_str());
    return PT_ERR_INVALID_ARGUMENT;
}

// little-endian words, as read_i32 / read_f32 take them (fourier.rs:16-28)
bool read_words(std::FILE* fp, void* out, size_t n) {
    if (n == 0) return true;
    if (std::fread(out, 4, n, fp) != n) return false;
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
    unsigned char* b = static_cast<unsigned char*>(out);
    for (size_t i = 0; i < n; i++) { std::swap(b[4 * i], b[4 * i + 3]); std::swap(b[4 * i + 1], b[4 * i + 2]); }
#endif
    return true;
}

}  // namespace

extern "C" {

pt_status pth_fourier_read(const char* filename, pth_fourier_file** out, char* err, size_t err_cap) {
    if (out) *out = nullptr;
    if (!filename || !out) return PT_ERR_INVALID_ARGUMENT;
    std::FILE* fp = std::fopen(filename, "rb");
    if (!fp) return refuse(filename, "cannot be opened", err, err_cap);
    struct Close { std::FILE* f; ~Close() { std::fclose(f); } } close_it{fp};
    unsigned char magic[8];
    if (std::fread(magic, 1, 8, fp) != 8) return refuse(filename, "is truncated (no header)", err, err_cap);
    if (std::memcmp(magic, "SCATFUN\x01", 8) != 0) return refuse(filename, "has an incompatible file format or version (magic)", err, err_cap);
    int32_t head[16];          // flags n_mu n_coeffs m_max n_channels n_bases, three unused, eta, four unused
    if (!read_words(fp, head, 14)) return refuse(filename, "is truncated (header)", err, err_cap);
    const int32_t flags = head[0], n_mu = head[1], n_coeffs = head[2], m_max = head[3], n_channels = head[4], n_bases = head[5];
    float eta;
    std::memcpy(&eta, &head[9], 4);
    if (flags != 1) return refuse(filename, "has an incompatible file format or version (flags is " + std::to_string(flags) + ", 1 is taken)", err, err_cap);
    if (n_channels != 1 && n_channels != 3) return refuse(filename, "has an incompatible file format or version (n_channels is " + std::to_string(n_channels) + ", 1 or 3 are taken)", err, err_cap);
    if (n_bases != 1) return refuse(filename, "has an incompatible file format or version (n_bases is " + std::to_string(n_bases) + ", 1 is taken)", err, err_cap);
    if (n_mu < 2 || n_mu > 32768) return refuse(filename, "n_mu is " + std::to_string(n_mu) + " (2 to 32768 nodes are taken)", err, err_cap);
    if (n_coeffs < 0 || m_max < 0) return refuse(filename, "n_coeffs or m_max is negative", err, err_cap);
    std::unique_ptr<pth_fourier_file> f(new pth_fourier_file());
    const size_t n2 = (size_t)n_mu * (size_t)n_mu;
    // Every count comes from the 64-byte header: each array is held against the bytes the file still has BEFORE it is allocated, so
    // that a short file that claims 32768 nodes or 2^31 coefficients is refused without a gigabyte having been asked for.
    uint64_t left = 0;
    {
        const long here = std::ftell(fp);
        if (here < 0 || std::fseek(fp, 0, SEEK_END) != 0) return refuse(filename, "cannot be read", err, err_cap);
        const long end = std::ftell(fp);
        if (end < here || std::fseek(fp, here, SEEK_SET) != 0) return refuse(filename, "cannot be read", err, err_cap);
        left = (uint64_t)(end - here);
    }
    auto take = [&](uint64_t words) { if (left < 4ull * words) return false; left -= 4ull * words; return true; };
    if (!take((uint64_t)n_mu)) return refuse(filename, "is truncated (mu)", err, err_cap);
    f->mu.resize((size_t)n_mu);
    if (!read_words(fp, f->mu.data(), f->mu.size())) return refuse(filename, "is truncated (mu)", err, err_cap);
    if (!take(n2)) return refuse(filename, "is truncated (cdf)", err, err_cap);
    f->cdf.resize(n2);
    if (!read_words(fp, f->cdf.data(), n2)) return refuse(filename, "is truncated (cdf)", err, err_cap);
    if (!take(2 * (uint64_t)n2)) return refuse(filename, "is truncated (offsets and lengths)", err, err_cap);
    f->offset_and_length.resize(2 * n2);
    if (!read_words(fp, f->offset_and_length.data(), 2 * n2)) return refuse(filename, "is truncated (offsets and lengths)", err, err_cap);
    if (!take((uint64_t)n_coeffs)) return refuse(filename, "is truncated (coefficients)", err, err_cap);
    f->a.resize((size_t)n_coeffs);
    if (!read_words(fp, f->a.data(), f->a.size())) return refuse(filename, "is truncated (coefficients)", err, err_cap);
    pt_fourier_table& t = f->table;
    std::memset(&t, 0, sizeof(t));
    t.n_mu = n_mu; t.n_channels = n_channels; t.m_max = m_max; t.n_coeffs = n_coeffs; t.eta = eta;
    t.mu = f->mu.data(); t.cdf = f->cdf.data(); t.offset_and_length = f->offset_and_length.data(); t.a = f->a.data();
    const std::string why = pt_fourier_table_refusal(t);
    if (!why.empty()) return refuse(filename, why, err, err_cap);
    *out = f.release();
    return PT_OK;
}

const pt_fourier_table* pth_fourier_table_of(const pth_fourier_file* f) { return f ? &f->table : nullptr; }

void pth_fourier_free(pth_fourier_file* f) { delete f; }

}  // extern "C"
