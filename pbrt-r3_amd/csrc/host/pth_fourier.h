// pth_fourier.h -- a tabulated BSDF file in memory (pth_fourier_read, include/pbrtgpu_host.h): the arrays, and the pt_fourier_table that points at them
#pragma once
#include <cstdint>
#include <vector>
#include "../../../include/pbrtgpu_host.h"

struct pth_fourier_file {
    pt_fourier_table table;
    std::vector<float> mu, cdf, a;
    std::vector<int32_t> offset_and_length;
};
