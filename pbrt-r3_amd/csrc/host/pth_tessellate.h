// pth_tessellate.h -- the shapes the reference only ever renders as triangle meshes: "loopsubdiv" (shapes/loopsubdiv.rs),
// "nurbs" (shapes/nurbs.rs) and "heightfield" (shapes/heightfield.rs).  Each produces the object-space arrays its
// create_triangle_mesh call receives (triangle.rs:696-731), in the reference's vertex and face order and with its f32
// operations; the scene context and the pth_tessellate_* C entry points (include/pbrtgpu_host.h) share this code.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pth {

struct TessMesh {
    std::vector<float> P;               // 3 per vertex
    std::vector<float> N;               // 3 per vertex, or empty
    std::vector<float> UV;              // 2 per vertex, or empty
    std::vector<uint32_t> indices;      // 3 per triangle
};

// Inputs the reference rejects give its message; inputs it would panic on or loop over (an edge shared by more than two
// faces, inconsistent winding, an unused vertex, levels < 0, knots it asserts on) are refused.  Every message names the shape.
// indices / P: nullptr = the parameter is missing.
bool tessellate_loopsubdiv(const std::vector<int>* indices, const std::vector<float>* P, int levels, TessMesh* out, std::string* err);

struct NurbsInput {
    int nu = -1, nv = -1, uorder = -1, vorder = -1;
    std::vector<float> uknots, vknots;
    std::vector<float> P;               // 3 per control point, or 4 (x, y, z, w) when homogeneous
    bool have_p = false, homogeneous = false;
    bool have_u0 = false, have_u1 = false, have_v0 = false, have_v1 = false;
    float u0 = 0.0f, u1 = 0.0f, v0 = 0.0f, v1 = 0.0f;
    int diceu = 30, dicev = 30;
};
bool tessellate_nurbs(const NurbsInput& in, TessMesh* out, std::string* err);

// Pz: nullptr = the parameter is missing.
bool tessellate_heightfield(int nu, int nv, const std::vector<float>* Pz, TessMesh* out, std::string* err);

}  // namespace pth
