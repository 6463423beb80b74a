// pt_kernels_maplight.hip -- the kernels and launchers of pt_kernels.hip a fourth time, in namespace ptm, with the two delta lights that
// read an image (goniometric, projection: delta_sample_li's PT_MAPLIGHT branch) on top of everything the third build knows (the analytic
// shapes by kind, the BxDFs of Material "disney"), so that such a light works beside every shape and material and needs no further sets.
// pt_context.cpp runs this set for a scene that holds one of the two lights and the other three for every other scene, so those keep
// the kernels they had, instruction for instruction.
#define PT_QUADRIC 1
#define PT_DISNEY 1
#define PT_MAPLIGHT 1
#define PT_KERNEL_NS ptm
#include "pt_kernels.hip"
