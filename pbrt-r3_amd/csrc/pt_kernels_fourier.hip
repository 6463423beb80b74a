// pt_kernels_fourier.hip -- the kernels and launchers of pt_kernels.hip a sixth time, in namespace ptf, with FourierBSDF among the lobes
// (PT_LOBE_FOURIER: pt_fourier.h, reached from globe_f / globe_pdf / globe_sample_f of pt_bxdf.h) on top of everything the fifth build
// knows, so that a Material "fourier" works beside every shape, material and light, in a scene that moves as well.  pt_context.cpp runs
// this set for a scene that holds such a material and the other five for every other scene, so those keep the kernels they had,
// instruction for instruction.
#define PT_QUADRIC 1
#define PT_DISNEY 1
#define PT_MAPLIGHT 1
#define PT_MOTION 1
#define PT_FOURIER 1
#define PT_KERNEL_NS ptf
#include "pt_kernels.hip"
