// pt_kernels_quadric.hip -- the kernels and launchers of pt_kernels.hip once more, in namespace ptq, with the analytic-shape slot
// dispatched by kind: sphere, cylinder or disk (pt_quadric.h).  pt_context.cpp runs this set for a scene that holds a cylinder or a
// disk and the first set for every other scene, so those keep the kernels they had, instruction for instruction.
#define PT_QUADRIC 1
#include "pt_kernels.hip"
