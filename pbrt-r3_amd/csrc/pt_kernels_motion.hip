// pt_kernels_motion.hip -- the kernels and launchers of pt_kernels.hip a fifth time, in namespace ptv, with motion blur: a time per camera
// sample (k_gen keeps the sampler's fifth dimension) that rides in the w lane of every ray direction, and AnimatedTransform::interpolate
// (animated_at, pt_motion.h) at the four places a transform that moves is read -- the two instance entrances of the traversal,
// make_surf_inst, the camera -- on top of everything the fourth build knows, so that a moving scene may hold any shape, material or light.
// pt_context.cpp runs this set for a scene whose camera or at least one instance actually moves and the other four for every other
// scene, so those keep the kernels they had, instruction for instruction.
#define PT_QUADRIC 1
#define PT_DISNEY 1
#define PT_MAPLIGHT 1
#define PT_MOTION 1
#define PT_KERNEL_NS ptv
#include "pt_kernels.hip"
