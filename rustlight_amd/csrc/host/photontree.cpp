// photontree.cpp — host-side build of the photon tree the beam radiance estimate gathers through: BHVAccel::create / build (src/accel.rs:458-543,
// build_element_tree of photontree.h) over Photon::aabb / position (src/integrators/explicit/vol_primitives.rs:48-60).  A node's box is the union, in index order, of pos -+ (r, r, r); a
// range of at most 4 photons is a leaf; otherwise the range is sorted by pos[axis] on the longest axis of the box (the reference's comparisons)
// and split at (begin + end) / 2.
//
// Two deliberate differences: the sort is stable — the reference's sort_unstable_by leaves the order of equal keys (-0 == +0
// included) unspecified, here they keep their order — and a non-finite position is refused where the reference's partial_cmp().unwrap() panics.
//
// The reference numbers its nodes as the recursion returns and walks them with a stack (gather, accel.rs:545-581: pop, push left, push right, so a
// node is followed by its right subtree, then its left one).  The nodes are stored here in exactly that visiting order with a skip link each — the
// index to go on with when the box is missed — so that the device walks them without a stack.  Built once per photon map, untimed like the BVH.
#include "photontree.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../kernels/wavefront.h"     // rl_set_error

namespace rl {
namespace {

// Photon::aabb / position (vol_primitives.rs:48-60)
struct PhotonElems {
    const uint32_t* words;
    float radius;
    float pos(uint32_t rec, int axis) const {
        float v;
        std::memcpy(&v, words + (size_t)rec * RL_VPL_WORDS + 4 + axis, sizeof v);
        return v;
    }
    // default().union_vec(pos - radius).union_vec(pos + radius)
    void box(uint32_t rec, float lo[3], float hi[3]) const {
        for (int a = 0; a < 3; a++) {
            const float p = pos(rec, a);
            lo[a] = std::fmin(std::fmin(3.402823466e+38f, p - radius), p + radius);
            hi[a] = std::fmax(std::fmax(-3.402823466e+38f, p - radius), p + radius);
        }
    }
    float key(uint32_t rec, int axis) const { return pos(rec, axis); }
};

}  // namespace

int check_photon_radius(float radius) {
    if (!std::isfinite(radius) || !(radius > 0.0f)) { rl_set_error("the photon radius must be finite and > 0"); return RL_ERR_INVALID_ARGUMENT; }
    return RL_OK;
}

int copy_tree_out(const ElementTree& tree, size_t node_capacity, size_t* n_nodes, float* node_boxes, uint32_t* node_links, uint32_t* order, const char* who) {
    *n_nodes = tree.n_nodes();
    if (!node_boxes && !node_links && !order) return RL_OK;      // the size only
    if (!node_boxes || !node_links || !order) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < tree.n_nodes()) { rl_set_error(std::string(who) + ": node_capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    std::copy(tree.boxes.begin(), tree.boxes.end(), node_boxes);
    std::copy(tree.links.begin(), tree.links.end(), node_links);
    std::copy(tree.order.begin(), tree.order.end(), order);
    return RL_OK;
}

int build_photon_tree(const uint32_t* words, size_t n, float radius, ElementTree* out) {
    if (!out || (n && !words)) return RL_ERR_INVALID_ARGUMENT;
    if (check_photon_radius(radius) != RL_OK) return RL_ERR_INVALID_ARGUMENT;
    if (n > kElementTreeMax) { rl_set_error("too many photons"); return RL_ERR_INVALID_ARGUMENT; }
    const PhotonElems e{words, radius};
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(e.pos((uint32_t)i, a))) { rl_set_error("a photon position is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    build_element_tree(e, n, out);
    return RL_OK;
}

}  // namespace rl

extern "C" int rl_photon_tree_build(const uint32_t* words, size_t n_photons, float radius, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                                    uint32_t* node_links, uint32_t* order) {
    if (!n_nodes) return RL_ERR_INVALID_ARGUMENT;
    rl::ElementTree t;
    const int rcode = rl::build_photon_tree(words, n_photons, radius, &t);
    if (rcode != RL_OK) return rcode;
    return rl::copy_tree_out(t, node_capacity, n_nodes, node_boxes, node_links, order, "rl_photon_tree_build");
}
