// pt_kernels_disney.hip -- the kernels and launchers of pt_kernels.hip a third time, in namespace ptd, with the BxDFs of Material "disney"
// compiled into the lobe evaluators (pt_bxdf.h) and the analytic-shape slot dispatched by kind as in pt_kernels_quadric.hip, so that a
// Disney scene with a cylinder needs no fourth set.  pt_context.cpp runs this set for a scene that holds a Disney material and the other
// two for every other scene, so those keep the kernels they had, instruction for instruction.
#define PT_QUADRIC 1
#define PT_DISNEY 1
#define PT_KERNEL_NS ptd
#include "pt_kernels.hip"
