// pth_tessellate.cpp -- "loopsubdiv", "nurbs" and "heightfield" as the triangle meshes the reference builds from them
// (shapes/loopsubdiv.rs, shapes/nurbs.rs, shapes/heightfield.rs).  Same vertex numbering, face order and f32 operations
// (no fused multiply-add: the library is built with -ffp-contract=off), so the BVH built over the result is the reference's.
#include "pth_tessellate.h"
#include "../../../include/pbrtgpu_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace pth {

namespace {

const int NEXT[3] = {1, 2, 0};
const int PREV[3] = {2, 0, 1};
const float PI_F = 3.14159265358979323846f;      // std::f32::consts::PI

struct V3 { float x, y, z; };
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline V3 cross(V3 a, V3 b) { return {(a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)}; }
inline V3 normalize(V3 v) {                                      // vector3.rs:108-120: v / sqrt(x*x + y*y + z*z)
    float l = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return {v.x / l, v.y / l, v.z / l};
}

// ---- loopsubdiv.rs: SDVertex / SDFace as index arrays.  Face f's vertices are fv[3f..3f+2]; ff[3f+i] is the face across
// the edge (v[i], v[NEXT[i]]) or -1; the four children of face f at the next level are 4f+0 .. 4f+3; the child of vertex v
// keeps index v and the edge (odd) vertices follow in creation order -- exactly the reference's vector order.
struct SubdivMesh {
    std::vector<V3> p;
    std::vector<int32_t> start;                 // start_face
    std::vector<uint8_t> boundary, regular;
    std::vector<int32_t> fv, ff;
};

inline int vnum(const SubdivMesh& m, int32_t f, int32_t v) {
    const int32_t* w = &m.fv[3 * (size_t)f];
    return w[0] == v ? 0 : w[1] == v ? 1 : w[2] == v ? 2 : -1;
}

// SDVertex::one_ring (loopsubdiv.rs:96-157) as vertex indices.  The walk is bounded by the face count, so a topology the
// reference would loop on or unwrap None in ends in an error instead.
bool one_ring(const SubdivMesh& m, int32_t v, std::vector<int32_t>& ring) {
    ring.clear();
    const int32_t start = m.start[v];
    const size_t cap = m.ff.size() / 3 + 1;
    int32_t face = start;
    if (!m.boundary[v]) {
        for (size_t n = 0;; n++) {
            int i = vnum(m, face, v);
            if (i < 0 || n > cap) return false;
            ring.push_back(m.fv[3 * (size_t)face + NEXT[i]]);
            int32_t f2 = m.ff[3 * (size_t)face + i];
            if (f2 < 0) return false;
            if (f2 == start) break;
            face = f2;
        }
        return true;
    }
    for (size_t n = 0;; n++) {
        int i = vnum(m, face, v);
        if (i < 0 || n > cap) return false;
        int32_t f2 = m.ff[3 * (size_t)face + i];
        if (f2 < 0) break;
        face = f2;
    }
    ring.push_back(m.fv[3 * (size_t)face + NEXT[vnum(m, face, v)]]);
    for (size_t n = 0;; n++) {
        int i = vnum(m, face, v);
        if (i < 0 || n > cap) return false;
        ring.push_back(m.fv[3 * (size_t)face + PREV[i]]);
        int32_t f2 = m.ff[3 * (size_t)face + PREV[i]];
        if (f2 < 0) break;
        face = f2;
    }
    return true;
}

inline float loop_beta(uint32_t valence) { return valence == 3 ? 3.0f / 16.0f : 3.0f / (8.0f * (float)valence); }
inline float loop_gamma(uint32_t valence) { return 1.0f / ((float)valence + 3.0f / (8.0f * loop_beta(valence))); }

V3 weight_one_ring(const std::vector<V3>& p, int32_t v, const std::vector<int32_t>& ring, float beta) {
    float valence = (float)ring.size();
    V3 r = (1.0f - valence * beta) * p[v];
    for (int32_t q : ring) r = r + beta * p[q];
    return r;
}
V3 weight_boundary(const std::vector<V3>& p, int32_t v, const std::vector<int32_t>& ring, float beta) {
    V3 r = (1.0f - 2.0f * beta) * p[v];
    r = r + beta * p[ring[0]];
    r = r + beta * p[ring[ring.size() - 1]];
    return r;
}

bool loop_fail(std::string* err, const std::string& m) { *err = "loopsubdiv: " + m; return false; }

}  // namespace

bool tessellate_loopsubdiv(const std::vector<int>* indices, const std::vector<float>* P, int levels, TessMesh* out, std::string* err) {
    // create_loop_subdiv (loopsubdiv.rs:705-755)
    if (!indices) return loop_fail(err, "Vertex indices \"indices\" not provided for LoopSubdiv shape.");
    if (!P) return loop_fail(err, "Vertex positions \"P\" not provided for LoopSubdiv shape.");
    if (levels < 0) return loop_fail(err, "levels must not be negative");
    if (levels > 12) return loop_fail(err, "levels above 12 (over 16 million triangles per input face) are refused");
    const size_t nv = P->size() / 3, nf = indices->size() / 3;         // trailing values are ignored, as there
    if (nv > (size_t)INT32_MAX / 2 || nf > (size_t)INT32_MAX / 4) return loop_fail(err, "mesh too large");
    if (((uint64_t)nf << (2 * levels)) > (uint64_t)INT32_MAX / 3) return loop_fail(err, "subdivided mesh would exceed 2^31 indices");

    SubdivMesh m;
    m.p.resize(nv);
    for (size_t i = 0; i < nv; i++) m.p[i] = {(*P)[3 * i], (*P)[3 * i + 1], (*P)[3 * i + 2]};
    m.start.assign(nv, -1);
    m.fv.resize(3 * nf);
    m.ff.assign(3 * nf, -1);
    for (size_t i = 0; i < nf; i++) {                               // face -> vertex pointers; start_face = the last face seen
        for (int j = 0; j < 3; j++) {
            int v = (*indices)[3 * i + j];
            if (v < 0 || (size_t)v >= nv) return loop_fail(err, "vertex index " + std::to_string(v) + " out of range");
            m.fv[3 * i + j] = v;
            m.start[v] = (int32_t)i;
        }
        const int32_t* w = &m.fv[3 * i];
        if (w[0] == w[1] || w[1] == w[2] || w[0] == w[2]) return loop_fail(err, "face " + std::to_string(i) + " repeats a vertex");
    }
    {   // neighbour pointers (:349-391): the reference pairs the two faces of an edge by its vertex pair
        struct E { int32_t f; int32_t en; int32_t n; };
        std::unordered_map<uint64_t, E> edges;
        edges.reserve(3 * nf / 2 + 1);
        for (size_t i = 0; i < nf; i++)
            for (int en = 0; en < 3; en++) {
                uint32_t a = (uint32_t)m.fv[3 * i + en], b = (uint32_t)m.fv[3 * i + NEXT[en]];
                uint64_t key = a < b ? ((uint64_t)a << 32 | b) : ((uint64_t)b << 32 | a);
                auto it = edges.find(key);
                if (it == edges.end()) { edges.emplace(key, E{(int32_t)i, en, 1}); continue; }
                E& e = it->second;
                if (e.n != 1)
                    return loop_fail(err, "edge (" + std::to_string(a) + ", " + std::to_string(b) + ") is shared by more than two faces");
                if ((uint32_t)m.fv[3 * (size_t)e.f + e.en] != b)
                    return loop_fail(err, "faces " + std::to_string(e.f) + " and " + std::to_string(i) + " are wound inconsistently");
                m.ff[3 * (size_t)e.f + e.en] = (int32_t)i;
                m.ff[3 * i + en] = e.f;
                e.n = 2;
            }
    }
    m.boundary.assign(nv, 0);
    m.regular.assign(nv, 0);
    std::vector<int32_t> ring;
    for (size_t v = 0; v < nv; v++) {                               // finish vertex initialization (:393-418)
        if (m.start[v] < 0) return loop_fail(err, "vertex " + std::to_string(v) + " belongs to no face");
        int32_t face = m.start[v];
        for (size_t n = 0;; n++) {
            int32_t f2 = m.ff[3 * (size_t)face + vnum(m, face, (int32_t)v)];
            if (f2 < 0) { m.boundary[v] = 1; break; }
            if (f2 == m.start[v]) break;
            if (n > nf) return loop_fail(err, "vertex " + std::to_string(v) + " has a face cycle that does not close");
            face = f2;
        }
        if (!one_ring(m, (int32_t)v, ring)) return loop_fail(err, "vertex " + std::to_string(v) + " has a broken face ring");
        size_t valence = ring.size();
        m.regular[v] = (!m.boundary[v] && valence == 6) || (m.boundary[v] && valence == 4);
    }

    for (int level = 0; level < levels; level++) {                  // :420-611
        const size_t V = m.p.size(), F = m.fv.size() / 3;
        SubdivMesh n;
        n.p.resize(V);
        n.start.resize(V);
        n.boundary.assign(m.boundary.begin(), m.boundary.end());
        n.regular.assign(m.regular.begin(), m.regular.end());
        n.fv.assign(12 * F, -1);
        n.ff.assign(12 * F, -1);
        for (size_t v = 0; v < V; v++) {                            // even vertices
            if (!one_ring(m, (int32_t)v, ring)) return loop_fail(err, "broken face ring while subdividing");
            if (!m.boundary[v]) n.p[v] = weight_one_ring(m.p, (int32_t)v, ring, m.regular[v] ? 1.0f / 16.0f : loop_beta((uint32_t)ring.size()));
            else n.p[v] = weight_boundary(m.p, (int32_t)v, ring, 1.0f / 8.0f);
        }
        std::vector<int32_t> edge_vert(3 * F);
        for (size_t f = 0; f < F; f++)                               // odd vertices, in the order their edges are first seen
            for (int k = 0; k < 3; k++) {
                const int32_t f2 = m.ff[3 * f + k];
                const int32_t a = m.fv[3 * f + k], b = m.fv[3 * f + NEXT[k]];
                if (f2 >= 0 && (size_t)f2 < f) { edge_vert[3 * f + k] = edge_vert[3 * (size_t)f2 + vnum(m, f2, b)]; continue; }
                const int32_t id = (int32_t)n.p.size();
                edge_vert[3 * f + k] = id;
                V3 q;
                if (f2 < 0) q = 0.5f * m.p[a] + 0.5f * m.p[b];
                else {
                    const V3 po0 = m.p[m.fv[3 * f + PREV[k]]];
                    const V3 po1 = m.p[m.fv[3 * (size_t)f2 + PREV[vnum(m, f2, b)]]];
                    q = (3.0f / 8.0f) * m.p[a] + (3.0f / 8.0f) * m.p[b] + (1.0f / 8.0f) * po0 + (1.0f / 8.0f) * po1;
                }
                n.p.push_back(q);
                n.start.push_back((int32_t)(4 * f + 3));
                n.boundary.push_back(f2 < 0);
                n.regular.push_back(1);
            }
        for (size_t v = 0; v < V; v++) {                            // even vertex face pointers
            int32_t s = m.start[v];
            n.start[v] = 4 * s + vnum(m, s, (int32_t)v);
        }
        for (size_t f = 0; f < F; f++)                               // face neighbour pointers
            for (int j = 0; j < 3; j++) {
                const size_t c3 = 3 * (4 * f + 3), cj = 3 * (4 * f + j);
                n.ff[c3 + j] = (int32_t)(4 * f + NEXT[j]);
                n.ff[cj + NEXT[j]] = (int32_t)(4 * f + 3);
                const int32_t vj = m.fv[3 * f + j];
                int32_t f2 = m.ff[3 * f + j];
                if (f2 >= 0) n.ff[cj + j] = 4 * f2 + vnum(m, f2, vj);
                f2 = m.ff[3 * f + PREV[j]];
                if (f2 >= 0) n.ff[cj + PREV[j]] = 4 * f2 + vnum(m, f2, vj);
            }
        for (size_t f = 0; f < F; f++)                               // face vertex pointers
            for (int j = 0; j < 3; j++) {
                n.fv[3 * (4 * f + j) + j] = m.fv[3 * f + j];
                const int32_t ev = edge_vert[3 * f + j];
                n.fv[3 * (4 * f + j) + NEXT[j]] = ev;
                n.fv[3 * (4 * f + NEXT[j]) + j] = ev;
                n.fv[3 * (4 * f + 3) + j] = ev;
            }
        m = std::move(n);
    }

    const size_t V = m.p.size();
    for (size_t v = 0; v < V; v++) {                                // push to the limit surface in place, in vertex order (:613-623)
        if (!one_ring(m, (int32_t)v, ring)) return loop_fail(err, "broken face ring at the limit");
        if (m.boundary[v]) m.p[v] = weight_boundary(m.p, (int32_t)v, ring, 1.0f / 5.0f);
        else m.p[v] = weight_one_ring(m.p, (int32_t)v, ring, loop_gamma((uint32_t)ring.size()));
    }
    out->P.resize(3 * V);
    out->N.resize(3 * V);
    out->UV.clear();
    for (size_t v = 0; v < V; v++) {                                // limit tangents and normals (:625-669)
        one_ring(m, (int32_t)v, ring);
        const size_t valence = ring.size();
        V3 s = {0.0f, 0.0f, 0.0f}, t = {0.0f, 0.0f, 0.0f};
        const V3 vp = m.p[v];
        if (!m.boundary[v]) {
            for (size_t j = 0; j < valence; j++) {
                float ang = 2.0f * PI_F * (float)j / (float)valence;
                s = s + std::cos(ang) * m.p[ring[j]];
                t = t + std::sin(ang) * m.p[ring[j]];
            }
        } else {
            const V3 r0 = m.p[ring[0]], rl = m.p[ring[valence - 1]];
            s = rl - r0;
            if (valence == 2) t = r0 + m.p[ring[1]] - 2.0f * vp;
            else if (valence == 3) t = m.p[ring[1]] - vp;
            else if (valence == 4) t = -1.0f * r0 + 2.0f * m.p[ring[1]] + 2.0f * m.p[ring[2]] + -1.0f * m.p[ring[3]] + -2.0f * vp;
            else {
                float theta = PI_F / (float)(valence - 1);
                t = std::sin(theta) * (r0 + rl);
                for (size_t k = 1; k < valence - 1; k++) {
                    float wt = (2.0f * std::cos(theta) - 2.0f) * std::sin((float)k * theta);
                    t = t + wt * m.p[ring[k]];
                }
                t = {-t.x, -t.y, -t.z};
            }
        }
        V3 nn = normalize(cross(s, t));
        out->P[3 * v] = vp.x; out->P[3 * v + 1] = vp.y; out->P[3 * v + 2] = vp.z;
        out->N[3 * v] = nn.x; out->N[3 * v + 1] = nn.y; out->N[3 * v + 2] = nn.z;
    }
    out->indices.assign(m.fv.begin(), m.fv.end());
    return true;
}

// ---- nurbs.rs.  Where the reference asserts (or indexes out of bounds) the shape is refused.
namespace {

struct H4 { float x, y, z, w; };

bool nurbs_fail(std::string* err, const std::string& m) { *err = "nurbs: " + m; return false; }

bool knot_offset(const std::vector<float>& knot, int order, float t, int* out) {         // :21-31
    size_t off = (size_t)(order - 1);
    if (off + 1 >= knot.size()) return false;
    while (t > knot[off + 1]) {
        off++;
        if (off + 1 >= knot.size()) return false;
    }
    if (!(t >= knot[off] && t <= knot[off + 1])) return false;
    *out = (int)off;
    return true;
}

// nurbs_evaluate (:72-131): cp is the OffsetArray (array, offset) of the reference; every index it forms is checked.
bool nurbs_evaluate(int order, const std::vector<float>& knots, const H4* arr, long arr_len, long cp_base, int cp_stride, float t,
                    H4* val_out, V3* deriv) {
    const long np = arr_len - cp_base;
    int ko;
    if (!knot_offset(knots, order, t, &ko)) return false;
    auto knot = [&](long i) -> float { return knots[(size_t)(ko + i)]; };    // ko + i lies in [0, ko + 1] below
    if (ko < order - 1 || (size_t)(ko + order - 1) >= knots.size()) return false;
    const long cp_offset = ko - order + 1;
    if (!(cp_offset < np)) return false;
    H4 w[8];
    for (int i = 0; i < order; i++) {
        long k = cp_base + (cp_offset + i) * cp_stride;
        if (k < 0 || k >= arr_len) return false;
        w[i] = arr[k];
    }
    for (int i = 0; i < order - 2; i++)
        for (int j = 0; j < order - 1 - i; j++) {
            float alpha = (knot(1 + j) - t) / (knot(1 + j) - knot(j + 2 - order + i));
            if (!(alpha >= 0.0f && alpha <= 1.0f)) return false;
            w[j].x = alpha * w[j].x + (1.0f - alpha) * w[j + 1].x;
            w[j].y = alpha * w[j].y + (1.0f - alpha) * w[j + 1].y;
            w[j].z = alpha * w[j].z + (1.0f - alpha) * w[j + 1].z;
            w[j].w = alpha * w[j].w + (1.0f - alpha) * w[j + 1].w;
        }
    float alpha = (knot(1) - t) / (knot(1) - knot(0));
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return false;
    H4 val = {alpha * w[0].x + (1.0f - alpha) * w[1].x, alpha * w[0].y + (1.0f - alpha) * w[1].y,
              alpha * w[0].z + (1.0f - alpha) * w[1].z, alpha * w[0].w + (1.0f - alpha) * w[1].w};
    float factor = (float)(order - 1) / (knot(1) - knot(0));
    float dx = factor * (w[1].x - w[0].x), dy = factor * (w[1].y - w[0].y), dz = factor * (w[1].z - w[0].z), dw = factor * (w[1].w - w[0].w);
    deriv->x = (dx / val.w) - (val.x * dw / (val.w * val.w));
    deriv->y = (dy / val.w) - (val.y * dw / (val.w * val.w));
    deriv->z = (dz / val.w) - (val.z * dw / (val.w * val.w));
    *val_out = val;
    return true;
}

// nurbs_evaluate_surface (:133-173)
bool nurbs_evaluate_surface(int u_order, const std::vector<float>& u_knot, int u_cp, float u, int v_order, const std::vector<float>& v_knot,
                            int v_cp, float v, const std::vector<H4>& cp, V3* p, V3* dpdu, V3* dpdv) {
    H4 iso[8];
    const long iso_len = std::max(u_order, v_order);
    V3 unused;
    int u_offset, v_offset;
    if (!knot_offset(u_knot, u_order, u, &u_offset) || u_offset < u_order - 1) return false;
    const int u_first_cp = u_offset - u_order + 1;
    for (int i = 0; i < u_order; i++)
        if (!nurbs_evaluate(v_order, v_knot, cp.data(), (long)cp.size(), u_first_cp + i, u_cp, v, &iso[i], &unused)) return false;
    if (!knot_offset(v_knot, v_order, v, &v_offset) || v_offset < v_order - 1) return false;
    const int v_first_cp = v_offset - v_order + 1;
    if (!(v_first_cp < v_cp)) return false;
    H4 pw;
    if (!nurbs_evaluate(u_order, u_knot, iso, iso_len, -u_first_cp, 1, u, &pw, dpdu)) return false;
    for (int i = 0; i < v_order; i++)
        if (!nurbs_evaluate(u_order, u_knot, cp.data(), (long)cp.size(), (long)(v_first_cp + i) * u_cp, 1, u, &iso[i], &unused)) return false;
    H4 unused_h;
    if (!nurbs_evaluate(v_order, v_knot, iso, iso_len, -v_first_cp, 1, v, &unused_h, dpdv)) return false;
    *p = {pw.x / pw.w, pw.y / pw.w, pw.z / pw.w};
    return true;
}

inline float clampf(float x, float lo, float hi) { if (x < lo) x = lo; if (x > hi) x = hi; return x; }   // f32::clamp

}  // namespace

bool tessellate_nurbs(const NurbsInput& in, TessMesh* out, std::string* err) {
    // create_nurbs (:267-406): the reference's checks and messages, in its order
    if (in.nu == -1) return nurbs_fail(err, "Must provide number of control points \"nu\" with NURBS shape.");
    if (in.uorder == -1) return nurbs_fail(err, "Must provide u order \"uorder\" with NURBS shape.");
    if (in.uknots.empty()) return nurbs_fail(err, "Must provide u knot vector \"uknots\" with NURBS shape.");
    if (in.nu < 1 || in.uorder < 1) return nurbs_fail(err, "\"nu\" and \"uorder\" must be positive");
    if (in.uknots.size() != (size_t)in.nu + (size_t)in.uorder)
        return nurbs_fail(err, "Number of knots in u knot vector " + std::to_string(in.uknots.size()) + " doesn't match sum of number of u control points " +
                                   std::to_string(in.nu) + " and u order " + std::to_string(in.uorder) + ".");
    if (in.nv == -1) return nurbs_fail(err, "Must provide number of control points \"nv\" with NURBS shape.");
    if (in.vorder == -1) return nurbs_fail(err, "Must provide v order \"vorder\" with NURBS shape.");
    if (in.vknots.empty()) return nurbs_fail(err, "Must provide v knot vector \"vknots\" with NURBS shape.");
    if (in.nv < 1 || in.vorder < 1) return nurbs_fail(err, "\"nv\" and \"vorder\" must be positive");
    if (in.vknots.size() != (size_t)in.nv + (size_t)in.vorder)
        return nurbs_fail(err, "Number of knots in v knot vector " + std::to_string(in.vknots.size()) + " doesn't match sum of number of v control points " +
                                   std::to_string(in.nv) + " and v order " + std::to_string(in.vorder) + ".");
    if (!in.have_p) return nurbs_fail(err, "Must provide control points via \"P\" or \"Pw\" parameter to NURBS shape.");
    size_t npts = in.P.size();
    if (!in.homogeneous && npts % 3 == 0) npts /= 3;
    else if (in.homogeneous && npts % 4 == 0) npts /= 4;
    else return nurbs_fail(err, "Number of control points must be multiple of 3 or 4.");
    const size_t nunv = (size_t)in.nu * (size_t)in.nv;
    if (npts != nunv)
        return nurbs_fail(err, "Number of control points " + std::to_string(npts) + " doesn't match nu * nv = " + std::to_string(in.nu) + " * " +
                                   std::to_string(in.nv) + " = " + std::to_string(nunv) + ".");
    // beyond the reference's own checks: what it would panic on
    if (in.uorder < 2 || in.vorder < 2 || in.uorder > 8 || in.vorder > 8) return nurbs_fail(err, "orders outside 2 ... 8 are refused");
    std::vector<H4> pw(npts);
    for (size_t i = 0; i < npts; i++)
        pw[i] = in.homogeneous ? H4{in.P[4 * i], in.P[4 * i + 1], in.P[4 * i + 2], in.P[4 * i + 3]} : H4{in.P[3 * i], in.P[3 * i + 1], in.P[3 * i + 2], 1.0f};
    const float u0x = in.uknots[in.uorder - 1], u1x = in.uknots[in.nu];
    const float v0x = in.vknots[in.vorder - 1], v1x = in.vknots[in.nv];
    if (!(u0x <= u1x) || !(v0x <= v1x)) return nurbs_fail(err, "the knot vectors give an empty parameter range");
    const float u0 = clampf(in.have_u0 ? in.u0 : u0x, u0x, u1x), u1 = clampf(in.have_u1 ? in.u1 : u1x, u0x, u1x);
    const float v0 = clampf(in.have_v0 ? in.v0 : v0x, v0x, v1x), v1 = clampf(in.have_v1 ? in.v1 : v1x, v0x, v1x);
    const size_t diceu = (size_t)std::max(in.diceu, 2), dicev = (size_t)std::max(in.dicev, 2);
    if (diceu * dicev > ((size_t)1 << 28)) return nurbs_fail(err, "diceu * dicev above 2^28 is refused");

    // create_tesselated_mesh (:175-257)
    std::vector<float> ueval(diceu), veval(dicev);
    for (size_t i = 0; i < diceu; i++) { float t = (float)i / (float)(diceu - 1); ueval[i] = (1.0f - t) * u0 + t * u1; }
    for (size_t i = 0; i < dicev; i++) { float t = (float)i / (float)(dicev - 1); veval[i] = (1.0f - t) * v0 + t * v1; }
    out->P.resize(3 * diceu * dicev);
    out->N.resize(3 * diceu * dicev);
    out->UV.resize(2 * diceu * dicev);
    for (size_t v = 0; v < dicev; v++)
        for (size_t u = 0; u < diceu; u++) {
            const size_t k = v * diceu + u;
            const float uu = ueval[u], vv = veval[v];
            out->UV[2 * k] = uu; out->UV[2 * k + 1] = vv;
            V3 p, dpdu, dpdv;
            if (!nurbs_evaluate_surface(in.uorder, in.uknots, in.nu, uu, in.vorder, in.vknots, in.nv, vv, pw, &p, &dpdu, &dpdv)) {
                char b[96];
                std::snprintf(b, sizeof(b), " (u, v) = (%.9g, %.9g)", (double)uu, (double)vv);
                return nurbs_fail(err, std::string("the knot vectors cannot be evaluated (the reference asserts) at") + b);
            }
            V3 n = normalize(cross(dpdu, dpdv));                    // NaN where dpdu x dpdv vanishes, as there
            out->P[3 * k] = p.x; out->P[3 * k + 1] = p.y; out->P[3 * k + 2] = p.z;
            out->N[3 * k] = n.x; out->N[3 * k + 1] = n.y; out->N[3 * k + 2] = n.z;
        }
    out->indices.resize(6 * (diceu - 1) * (dicev - 1));
    size_t idx = 0;
    auto vn = [&](size_t u, size_t v) { return (uint32_t)(v * diceu + u); };
    for (size_t v = 0; v + 1 < dicev; v++)
        for (size_t u = 0; u + 1 < diceu; u++) {
            out->indices[idx++] = vn(u, v); out->indices[idx++] = vn(u + 1, v); out->indices[idx++] = vn(u + 1, v + 1);
            out->indices[idx++] = vn(u, v); out->indices[idx++] = vn(u + 1, v + 1); out->indices[idx++] = vn(u, v + 1);
        }
    return true;
}

bool tessellate_heightfield(int nu, int nv, const std::vector<float>* Pz, TessMesh* out, std::string* err) {
    // create_heightfield (heightfield.rs:5-75)
    if (nu == -1 || nv == -1) { *err = "heightfield: Must provide \"nu\" and \"nv\" parameters to heightfield shape."; return false; }
    if (nu < 1 || nv < 1) { *err = "heightfield: \"nu\" and \"nv\" must be positive"; return false; }
    if (!Pz) { *err = "heightfield: No vertex positions provided for heightfield shape."; return false; }
    const size_t nx = (size_t)nu, ny = (size_t)nv;
    if (Pz->size() != nx * ny) { *err = "heightfield: Number of \"Pz\" values doesn't match resolution."; return false; }
    out->P.resize(3 * nx * ny);
    out->UV.resize(2 * nx * ny);
    out->N.clear();
    for (size_t y = 0; y < ny; y++)
        for (size_t x = 0; x < nx; x++) {
            const size_t pos = nx * y + x;
            const float xx = (float)x / (float)(nx - 1), yy = (float)y / (float)(ny - 1);
            out->P[3 * pos] = xx; out->P[3 * pos + 1] = yy; out->P[3 * pos + 2] = (*Pz)[pos];
            out->UV[2 * pos] = xx; out->UV[2 * pos + 1] = yy;
        }
    out->indices.resize(6 * (nx - 1) * (ny - 1));
    auto vert = [&](size_t x, size_t y) { return (uint32_t)(x + y * nx); };
    for (size_t y = 0; y + 1 < ny; y++)
        for (size_t x = 0; x + 1 < nx; x++) {
            const size_t i = (x + y * (nx - 1)) * 6;
            out->indices[i] = vert(x, y); out->indices[i + 1] = vert(x + 1, y); out->indices[i + 2] = vert(x + 1, y + 1);
            out->indices[i + 3] = vert(x, y); out->indices[i + 4] = vert(x + 1, y + 1); out->indices[i + 5] = vert(x, y + 1);
        }
    return true;
}

}  // namespace pth

// ---- C ABI (include/pbrtgpu_host.h)
namespace {

pt_status tess_result(bool ok, pth::TessMesh& m, const std::string& e, pth_tess_mesh* out, char* err, size_t cap) {
    std::memset(out, 0, sizeof(*out));
    if (!ok) {
        if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
        return PT_ERR_INVALID_ARGUMENT;
    }
    auto dup = [](const void* src, size_t bytes) -> void* {
        if (!bytes) return nullptr;
        void* d = std::malloc(bytes);
        if (d) std::memcpy(d, src, bytes);
        return d;
    };
    out->n_vertices = (uint32_t)(m.P.size() / 3);
    out->n_triangles = (uint32_t)(m.indices.size() / 3);
    out->P = (float*)dup(m.P.data(), m.P.size() * sizeof(float));
    out->N = (float*)dup(m.N.data(), m.N.size() * sizeof(float));
    out->uv = (float*)dup(m.UV.data(), m.UV.size() * sizeof(float));
    out->indices = (uint32_t*)dup(m.indices.data(), m.indices.size() * sizeof(uint32_t));
    if ((!m.P.empty() && !out->P) || (!m.N.empty() && !out->N) || (!m.UV.empty() && !out->uv) || (!m.indices.empty() && !out->indices)) {
        pth_tess_mesh_free(out);
        if (err && cap) std::snprintf(err, cap, "out of host memory");
        return PT_ERR_OUT_OF_MEMORY;
    }
    return PT_OK;
}

}  // namespace

extern "C" pt_status pth_tessellate_loopsubdiv(const int32_t* indices, size_t n_indices, const float* P, size_t n_p, int32_t levels,
                                                pth_tess_mesh* out, char* err, size_t err_cap) {
    if (!out) return PT_ERR_INVALID_ARGUMENT;
    std::vector<int> vi, *pvi = nullptr;
    std::vector<float> vp, *pvp = nullptr;
    if (indices) { vi.assign(indices, indices + n_indices); pvi = &vi; }
    if (P) { vp.assign(P, P + n_p); pvp = &vp; }
    pth::TessMesh m;
    std::string e;
    bool ok = pth::tessellate_loopsubdiv(pvi, pvp, levels, &m, &e);
    return tess_result(ok, m, e, out, err, err_cap);
}

extern "C" pt_status pth_tessellate_nurbs(const pth_nurbs_params* prm, pth_tess_mesh* out, char* err, size_t err_cap) {
    if (!out || !prm) return PT_ERR_INVALID_ARGUMENT;
    pth::NurbsInput in;
    in.nu = prm->nu; in.nv = prm->nv; in.uorder = prm->uorder; in.vorder = prm->vorder;
    if (prm->uknots) in.uknots.assign(prm->uknots, prm->uknots + prm->n_uknots);
    if (prm->vknots) in.vknots.assign(prm->vknots, prm->vknots + prm->n_vknots);
    in.have_p = prm->P != nullptr && prm->n_p > 0;
    if (in.have_p) in.P.assign(prm->P, prm->P + prm->n_p);
    in.homogeneous = prm->homogeneous != 0;
    in.have_u0 = prm->range_given & 1; in.have_u1 = prm->range_given & 2; in.have_v0 = prm->range_given & 4; in.have_v1 = prm->range_given & 8;
    in.u0 = prm->u0; in.u1 = prm->u1; in.v0 = prm->v0; in.v1 = prm->v1;
    in.diceu = prm->diceu; in.dicev = prm->dicev;
    pth::TessMesh m;
    std::string e;
    bool ok = pth::tessellate_nurbs(in, &m, &e);
    return tess_result(ok, m, e, out, err, err_cap);
}

extern "C" pt_status pth_tessellate_heightfield(int32_t nu, int32_t nv, const float* Pz, size_t n_pz, pth_tess_mesh* out, char* err, size_t err_cap) {
    if (!out) return PT_ERR_INVALID_ARGUMENT;
    std::vector<float> z, *pz = nullptr;
    if (Pz) { z.assign(Pz, Pz + n_pz); pz = &z; }
    pth::TessMesh m;
    std::string e;
    bool ok = pth::tessellate_heightfield(nu, nv, pz, &m, &e);
    return tess_result(ok, m, e, out, err, err_cap);
}

extern "C" void pth_tess_mesh_free(pth_tess_mesh* m) {
    if (!m) return;
    std::free(m->P); std::free(m->N); std::free(m->uv); std::free(m->indices);
    std::memset(m, 0, sizeof(*m));
}
