// planetree.cpp — host side of the single-scattering photon-plane integrator (src/integrators/explicit/plane_single.rs): the rectangular lights
// (RectangularLightSource::from_shape, 38-75) and the tree its gather walks — BHVAccel::create (src/accel.rs:458-543, build_element_tree of photontree.h)
// over SinglePhotonPlane::aabb / position (plane_single.rs:101-117).  A plane's box is the union of its four corners o, o + d0 l0, o + d1 l1 and
// (o + d0 l0) + d1 l1; its sort key is the plane's middle ((o + (d0 l0) 0.5) + (d1 l1) 0.5)[axis].
//
// The deviations are the photon tree's: a stable sort, and a plane with a non-finite corner is refused where the reference's
// partial_cmp().unwrap() panics.  Node order and skip links are the photon tree's too: both are ElementTrees, and the device walks them with one loop (kernels/gather.hip.h).
#include <cmath>
#include <cstring>

#include "photontree.h"
#include "scene.h"
#include "../kernels/wavefront.h"     // rl_set_error

namespace rl {
namespace {

struct PlaneElems {
    const uint32_t* words;
    float f(uint32_t rec, int k) const {
        float v;
        std::memcpy(&v, words + (size_t)rec * RL_PLANE_WORDS + k, sizeof v);
        return v;
    }
    // the corners, per axis: o, p0 = o + d0 * length0, p1 = o + d1 * length1, p2 = p0 + d1 * length1
    void corners(uint32_t rec, int a, float c[4]) const {
        const float o = f(rec, a), e0 = f(rec, 3 + a) * f(rec, 9), e1 = f(rec, 6 + a) * f(rec, 10);
        c[0] = o; c[1] = o + e0; c[2] = o + e1; c[3] = c[1] + e1;
    }
    // AABB::default().union_vec(o).union_vec(p0).union_vec(p1).union_vec(p2)
    void box(uint32_t rec, float lo[3], float hi[3]) const {
        for (int a = 0; a < 3; a++) {
            float c[4];
            corners(rec, a, c);
            lo[a] = 3.402823466e+38f; hi[a] = -3.402823466e+38f;
            for (int k = 0; k < 4; k++) { lo[a] = std::fmin(lo[a], c[k]); hi[a] = std::fmax(hi[a], c[k]); }
        }
    }
    // self.o + self.d0 * self.length0 * 0.5 + self.d1 * self.length1 * 0.5
    float key(uint32_t rec, int a) const { return (f(rec, a) + (f(rec, 3 + a) * f(rec, 9)) * 0.5f) + (f(rec, 6 + a) * f(rec, 10)) * 0.5f; }
};

}  // namespace

int check_plane_records(const uint32_t* words, size_t n) {
    if (n && !words) return RL_ERR_INVALID_ARGUMENT;
    const PlaneElems e{words};
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            float c[4];
            e.corners((uint32_t)i, a, c);
            for (int k = 0; k < 4; k++)
                if (!std::isfinite(c[k])) { rl_set_error("a plane corner is not finite"); return RL_ERR_INVALID_ARGUMENT; }
        }
    return RL_OK;
}

int build_plane_tree(const uint32_t* words, size_t n, ElementTree* out) {
    if (!out || (n && !words)) return RL_ERR_INVALID_ARGUMENT;
    if (n > kElementTreeMax) { rl_set_error("too many planes"); return RL_ERR_INVALID_ARGUMENT; }
    const int rcode = check_plane_records(words, n);
    if (rcode != RL_OK) return rcode;
    build_element_tree(PlaneElems{words}, n, out);
    return RL_OK;
}

int build_rect_lights(const rl_scene& scene, std::vector<RectLight>* out, const char** err) {
    out->clear();
    for (const HostMesh& m : scene.meshes) {
        if (!m.is_light) continue;
        // the reference's own test (`vertices.len() != 3 && indices.len() != 2`) lets other shapes through to vertices[3], which panics or reads a triangle's
        // corner as the quad's: a quad is what the integrator is written for
        if (m.n_tris() != 2 || m.positions.size() < 4) { *err = "plane-single supports rectangular emitters only (a light mesh of 2 triangles over 4 vertices)"; return RL_ERR_UNSUPPORTED; }
        if (m.emission_type != RL_EMISSION_COLOR) { *err = "plane-single takes constant-colour emitters only (the reference panics on HSV and textured emission)"; return RL_ERR_UNSUPPORTED; }
        RectLight l;
        const Vec3 o = m.positions[0];
        Vec3 u = vsub(m.positions[1], m.positions[0]), v = vsub(m.positions[3], m.positions[0]);
        l.u_l = vlen(u); l.v_l = vlen(v);
        u = vdiv(u, l.u_l); v = vdiv(v, l.v_l);
        const Vec3 n = vcross(u, v);
        for (int k = 0; k < 3; k++) { l.o[k] = o.get(k); l.u[k] = u.get(k); l.v[k] = v.get(k); l.n[k] = n.get(k); l.emission[k] = m.emission[k]; }
        out->push_back(l);
    }
    if (out->empty()) { *err = "plane-single needs an emissive mesh"; return RL_ERR_NO_EMITTER; }
    return RL_OK;
}

}  // namespace rl

extern "C" int rl_plane_tree_build(const uint32_t* words, size_t n_planes, size_t node_capacity, size_t* n_nodes, float* node_boxes, uint32_t* node_links,
                                   uint32_t* order) {
    if (!n_nodes) return RL_ERR_INVALID_ARGUMENT;
    rl::ElementTree t;
    const int rcode = rl::build_plane_tree(words, n_planes, &t);
    if (rcode != RL_OK) return rcode;
    return rl::copy_tree_out(t, node_capacity, n_nodes, node_boxes, node_links, order, "rl_plane_tree_build");
}
