// phototree.h — host side of the device builds of the element trees (the kernels and the shared driver are in phototree.hip.h): the photon tree
// (phototree.hip) and the plane tree (planetree.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace rl {

// Every pointer is device memory.  words: n records of RL_VPL_WORDS u32.  group: photons one workgroup finishes in LDS (clamped to 4 .. RL_PHOTON_TREE_GROUP_PHOTONS).
// nodes: [photon_tree_node_count(n)][2] in the gather's format, NULL = the check pass alone; order: [n] or NULL; photons: [n][3] in leaf order or NULL.
struct PhotonTreeJob {
    const unsigned* words;
    unsigned n;
    float radius;
    unsigned group;
    bool check_kind;        // refuse records that are no volume records (a photon map), as well as positions that are not finite
    float4* nodes;
    unsigned* order;
    float4* photons;
};
unsigned photon_tree_node_count(unsigned n_photons);
// Check pass, then the build, on `st`; returns synchronised.  RL_OK, RL_ERR_INVALID_ARGUMENT with the host build's messages, or RL_ERR_HIP.
// The flag word of the check pass is all that comes back to the host.  ms_kernels (may be NULL): the HIP-event time of the launches when `timing`.
int photon_tree_run(const PhotonTreeJob& job, hipStream_t st, bool timing, float* ms_kernels);

// The same for planes.  words: n records of RL_PLANE_WORDS u32; group is clamped to 4 .. RL_PLANE_TREE_GROUP_PLANES; planes: [n][4] in leaf order or NULL.
// The node count is photon_tree_node_count(n): the topology depends on n alone.
struct PlaneTreeJob {
    const unsigned* words;
    unsigned n;
    unsigned group;
    float4* nodes;
    unsigned* order;
    float4* planes;
};
int plane_tree_run(const PlaneTreeJob& job, hipStream_t st, bool timing, float* ms_kernels);

}  // namespace rl
