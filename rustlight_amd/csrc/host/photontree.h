// photontree.h — the photon tree of the beam radiance estimate (photontree.cpp), as the host hands it to the device and to rl_photon_tree_build.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rl {

// Nodes in the order the reference's gather visits them (node, right subtree, left subtree), so a walk needs no stack:
// `i = entered ? i + 1 : skip[i]`, done at i == number of nodes.
struct PhotonTree {
    std::vector<float> boxes;          // [node][6]: p_min, p_max
    std::vector<uint32_t> links;       // [node][3]: skip, first, count (count = 0: an inner node; first indexes `order`)
    std::vector<uint32_t> order;       // [photon]: the record that stands at this place once every sort is done
    size_t n_nodes() const { return links.size() / 3; }
};

// words: n records of RL_VPL_WORDS u32 (only the position, words 4..6, is read).  RL_OK, or RL_ERR_INVALID_ARGUMENT with rl_last_error set.
int build_photon_tree(const uint32_t* words, size_t n, float radius, PhotonTree* out);

}  // namespace rl
