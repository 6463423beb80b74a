// pt_kernels.h -- host-callable launchers of the kernels in pt_kernels.hip, in namespace ptq those of its second build
// (pt_kernels_quadric.hip: scenes that hold a cylinder or a disk), and in namespace ptd those of its third (pt_kernels_disney.hip:
// scenes that hold a Material "disney"), and in namespace ptm those of its fourth (pt_kernels_maplight.hip: scenes that hold a
// goniometric or a projection light).
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
