// photontree.cpp — host-side build of the photon tree the beam radiance estimate gathers through: BHVAccel::create / build (src/accel.rs:458-543)
// over Photon::aabb / position (src/integrators/explicit/vol_primitives.rs:48-60).  A node's box is the union, in index order, of pos -+ (r, r, r); a
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

#include "../kernels/wavefront.h"     // rl_set_error
#include "../../../include/rustlight_amd.h"

namespace rl {
namespace {

struct Builder {
    const uint32_t* words;
    float radius;
    PhotonTree* t;

    float pos(uint32_t rec, int axis) const {
        float v;
        std::memcpy(&v, words + (size_t)rec * RL_VPL_WORDS + 4 + axis, sizeof v);
        return v;
    }
    // build(begin, end): the node of the range goes to the next free index, its right subtree behind it, then the left one
    void build(size_t begin, size_t end) {
        float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};   // AABB::default()
        for (size_t i = begin; i < end; i++)
            for (int a = 0; a < 3; a++) {
                const float p = pos(t->order[i], a);
                // Photon::aabb: default().union_vec(pos - radius).union_vec(pos + radius), then union_aabb into the node's box
                const float e_lo = std::fmin(std::fmin(3.402823466e+38f, p - radius), p + radius), e_hi = std::fmax(std::fmax(-3.402823466e+38f, p - radius), p + radius);
                lo[a] = std::fmin(lo[a], e_lo); hi[a] = std::fmax(hi[a], e_hi);
            }
        const size_t node = t->n_nodes();
        t->boxes.insert(t->boxes.end(), {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]});
        t->links.insert(t->links.end(), {0u, 0u, 0u});
        if (end - begin <= 4) {
            t->links[3 * node + 1] = (uint32_t)begin; t->links[3 * node + 2] = (uint32_t)(end - begin);
        } else {
            const float sx = hi[0] - lo[0], sy = hi[1] - lo[1], sz = hi[2] - lo[2];      // aabb.size()
            const int axis = sx > sy ? (sx > sz ? 0 : 2) : (sy > sz ? 1 : 2);
            std::stable_sort(t->order.begin() + begin, t->order.begin() + end, [&](uint32_t a, uint32_t b) { return pos(a, axis) < pos(b, axis); });
            const size_t split = (begin + end) / 2;
            build(split, end);            // the two ranges are disjoint: which one is built first changes nothing but the node numbers
            build(begin, split);
        }
        t->links[3 * node] = (uint32_t)t->n_nodes();      // the first node behind this subtree
    }
};

}  // namespace

int build_photon_tree(const uint32_t* words, size_t n, float radius, PhotonTree* out) {
    if (!out || (n && !words)) return RL_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(radius) || !(radius > 0.0f)) { rl_set_error("the photon radius must be finite and > 0"); return RL_ERR_INVALID_ARGUMENT; }
    if (n > (size_t)RL_VPL_MAX + 4096) { rl_set_error("too many photons"); return RL_ERR_INVALID_ARGUMENT; }
    out->boxes.clear(); out->links.clear();
    out->order.resize(n);
    Builder b{words, radius, out};
    for (size_t i = 0; i < n; i++) {
        out->order[i] = (uint32_t)i;
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(b.pos((uint32_t)i, a))) { rl_set_error("a photon position is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    }
    if (n > 0) b.build(0, n);
    return RL_OK;
}

}  // namespace rl

extern "C" int rl_photon_tree_build(const uint32_t* words, size_t n_photons, float radius, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                                    uint32_t* node_links, uint32_t* order) {
    if (!n_nodes) return RL_ERR_INVALID_ARGUMENT;
    rl::PhotonTree t;
    const int rcode = rl::build_photon_tree(words, n_photons, radius, &t);
    if (rcode != RL_OK) return rcode;
    *n_nodes = t.n_nodes();
    if (!node_boxes && !node_links && !order) return RL_OK;      // the size only
    if (!node_boxes || !node_links || !order) return RL_ERR_INVALID_ARGUMENT;
    if (node_capacity < t.n_nodes()) { rl_set_error("rl_photon_tree_build: node_capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    std::copy(t.boxes.begin(), t.boxes.end(), node_boxes);
    std::copy(t.links.begin(), t.links.end(), node_links);
    std::copy(t.order.begin(), t.order.end(), order);
    return RL_OK;
}
