// pt_kernels.h -- host-callable launchers of the kernels in pt_kernels.hip, in namespace ptq those of its second build
// (pt_kernels_quadric.hip: scenes that hold a cylinder or a disk), and in namespace ptd those of its third (pt_kernels_disney.hip:
// scenes that hold a Material "disney"), and in namespace ptm those of its fourth (pt_kernels_maplight.hip: scenes that hold a
// goniometric or a projection light).  Namespace ptf: those of its sixth (pt_kernels_fourier.hip: scenes that hold a Material "fourier").
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "../../include/pbrtgpu.h"

#include "pt_kernels_decl.inc"
namespace ptq {
#include "pt_kernels_decl.inc"
}
namespace ptd {
#include "pt_kernels_decl.inc"
}
namespace ptm {
#include "pt_kernels_decl.inc"
}
// the fifth build (pt_kernels_motion.hip: scenes whose camera or instances move), and what only it has: the hooks that take a time per ray
namespace ptv {
#include "pt_kernels_decl.inc"
hipError_t ptk_trace_batch_time(hipStream_t st, int grid, const PtScene& sc, uint32_t n, const float* o, const float* d, const float* tmax, const float* time,
                                pt_hit* out, uint8_t* occ, int any_hit, uint32_t* ticket, PtCounters* cnt, uint32_t* spill, uint32_t spill_depth, uint32_t* err, int alpha);
hipError_t ptk_camera_rays_time(hipStream_t st, const PtScene& sc, uint32_t n, const int32_t* pixel_xy, const uint32_t* sample_index, float* o, float* d,
                                float* pf, float* time);
}
namespace ptf {
#include "pt_kernels_decl.inc"
}
