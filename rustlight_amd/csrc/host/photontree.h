// photontree.h — the element trees the volumetric gathers walk (BHVAccel, src/accel.rs:458-581): the photon tree of the beam radiance estimate
// (photontree.cpp) and the plane tree of the single-scattering photon planes (planetree.cpp), as the host hands them to the device and to
// rl_photon_tree_build / rl_plane_tree_build.  Both are ElementTrees built by build_element_tree below; what differs is an element's box and its sort key.
// The device walks either with one loop (kernels/gather.hip.h); kernels/gather_render.hip.h packs the nodes for it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/rustlight_amd.h"

namespace rl {

// the most elements a tree takes: a generation stops at RL_VPL_MAX records and may overshoot by one path's
constexpr size_t kElementTreeMax = (size_t)RL_VPL_MAX + 4096;

// Nodes in the order the reference's gather visits them (node, right subtree, left subtree), so a walk needs no stack:
// `i = entered ? i + 1 : skip[i]`, done at i == number of nodes.
struct ElementTree {
    std::vector<float> boxes;          // [node][6]: p_min, p_max
    std::vector<uint32_t> links;       // [node][3]: skip, first, count (count = 0: an inner node; first indexes `order`)
    std::vector<uint32_t> order;       // [element]: the record that stands at this place once every sort is done
    size_t n_nodes() const { return links.size() / 3; }
};

// BHVAccel::create / build (accel.rs:458-543) over n elements.  E: `void box(uint32_t rec, float lo[3], float hi[3]) const` = BVHElement::aabb,
// `float key(uint32_t rec, int axis) const` = BVHElement::position()[axis].  A node's box is the union, in index order, of its elements' boxes; a range of
// at most 4 elements is a leaf; otherwise the range is sorted by key on the longest axis of the box (the reference's comparisons; stable) and
// split at (begin + end) / 2.  The node of a range goes to the next free index, its right subtree behind it, then the left one.
template <class E>
struct ElementTreeBuilder {
    const E& e;
    ElementTree* t;
    void build(size_t begin, size_t end) {
        float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};   // AABB::default()
        for (size_t i = begin; i < end; i++) {
            float e_lo[3], e_hi[3];
            e.box(t->order[i], e_lo, e_hi);
            for (int a = 0; a < 3; a++) { lo[a] = std::fmin(lo[a], e_lo[a]); hi[a] = std::fmax(hi[a], e_hi[a]); }      // union_aabb
        }
        const size_t node = t->n_nodes();
        t->boxes.insert(t->boxes.end(), {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]});
        t->links.insert(t->links.end(), {0u, 0u, 0u});
        if (end - begin <= 4) {
            t->links[3 * node + 1] = (uint32_t)begin; t->links[3 * node + 2] = (uint32_t)(end - begin);
        } else {
            const float sx = hi[0] - lo[0], sy = hi[1] - lo[1], sz = hi[2] - lo[2];      // aabb.size()
            const int axis = sx > sy ? (sx > sz ? 0 : 2) : (sy > sz ? 1 : 2);
            std::stable_sort(t->order.begin() + begin, t->order.begin() + end, [&](uint32_t a, uint32_t b) { return e.key(a, axis) < e.key(b, axis); });
            const size_t split = (begin + end) / 2;
            build(split, end);            // the two ranges are disjoint: which one is built first changes nothing but the node numbers
            build(begin, split);
        }
        t->links[3 * node] = (uint32_t)t->n_nodes();      // the first node behind this subtree
    }
};
template <class E>
void build_element_tree(const E& e, size_t n, ElementTree* out) {
    out->boxes.clear(); out->links.clear();
    out->order.resize(n);
    for (size_t i = 0; i < n; i++) out->order[i] = (uint32_t)i;
    ElementTreeBuilder<E> b{e, out};
    if (n > 0) b.build(0, n);
}

// words: n records of RL_VPL_WORDS u32 (only the position, words 4..6, is read).  RL_OK, or RL_ERR_INVALID_ARGUMENT with rl_last_error set.
int build_photon_tree(const uint32_t* words, size_t n, float radius, ElementTree* out);
// what every photon entry point asks of the radius: RL_ERR_INVALID_ARGUMENT with rl_last_error set unless it is finite and > 0
int check_photon_radius(float radius);
// the tail of rl_photon_tree_build / rl_plane_tree_build (`who`): the node count, then — unless all three arrays are null — the tree into the caller's arrays
int copy_tree_out(const ElementTree& tree, size_t node_capacity, size_t* n_nodes, float* node_boxes, uint32_t* node_links, uint32_t* order, const char* who);

// The rectangular lights of the photon-plane integrators (planetree.cpp: RectangularLightSource::from_shape, plane_single.rs:38-75), in mesh order
struct RectLight { float o[3], n[3], u[3], v[3], u_l, v_l, emission[3]; };
// words: n records of RL_PLANE_WORDS u32 (o, d0, d1, length0, length1 are read).  RL_OK, or RL_ERR_INVALID_ARGUMENT with rl_last_error set.
int build_plane_tree(const uint32_t* words, size_t n, ElementTree* out);
// what build_plane_tree refuses, alone: RL_ERR_INVALID_ARGUMENT with rl_last_error set when a plane has a non-finite corner
int check_plane_records(const uint32_t* words, size_t n);

}  // namespace rl

struct rl_scene;
namespace rl {
// RL_OK and the lights, or the refusal's code with its one-line message in *err (no light mesh, a light mesh that is no quad, an emission that is no colour)
int build_rect_lights(const rl_scene& scene, std::vector<RectLight>* out, const char** err);
}  // namespace rl
