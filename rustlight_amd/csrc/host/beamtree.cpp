// beamtree.cpp — host side of the photon beams (src/integrators/explicit/vol_primitives.rs): the split of the beams into sub-beams (647-684) and the tree the
// gather walks — BHVAccel::create (src/accel.rs:458-543, build_element_tree of photontree.h) over PhotonBeam::aabb / position (vol_primitives.rs:123-136).
//
// Split, SPLIT = 5: avg_split = (the lengths summed in f32 in record order) / (n * 5) as f32; a beam yields number_split = ceil(length / avg_split) as u32
// sub-beams of new_length = length / number_split as f32, sub-beam i starting at o + d * (i as f32) * new_length.  A beam of length 0 yields none.  A sub-beam
// keeps its beam's record layout (RL_BEAM_WORDS u32) with o and length replaced.
//
// Tree: a sub-beam's box is the union of o - r, o + r, (o + d * length) - r and (o + d * length) + r; its sort key is its middle o + d * length * 0.5.
//
// The deviations are the photon tree's: a stable sort, and a record with a non-finite o, d, length, box or key is refused where the reference's
// partial_cmp().unwrap() panics.  A split whose avg_split is zero or not finite (no beam has a length, or the sum overflows) is refused too: the reference
// divides by it.  Node order and skip links are the photon tree's: the device walks all three trees with one loop (kernels/gather.hip.h).
#include <cmath>
#include <cstring>

#include "beamtree.h"
#include "../kernels/wavefront.h"     // rl_set_error

namespace rl {
namespace {

constexpr float kF32Max = 3.402823466e+38f;

float word_f(const uint32_t* words, size_t rec, int k) {
    float v;
    std::memcpy(&v, words + rec * RL_BEAM_WORDS + k, sizeof v);
    return v;
}
// `x as u32` of a float that went through ceil(): saturating, NaN = 0
uint32_t as_u32(float x) {
    if (!(x > 0.0f)) return 0u;
    if (x >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)x;
}

// PhotonBeam::aabb / position (vol_primitives.rs:123-136)
struct BeamElems {
    const uint32_t* words;
    float radius;
    float f(uint32_t rec, int k) const { return word_f(words, rec, k); }
    float end(uint32_t rec, int a) const { return f(rec, a) + f(rec, 4 + a) * f(rec, 3); }      // self.o + self.d * self.length
    // default().union_vec(o - radius).union_vec(o + radius).union_vec(end - radius).union_vec(end + radius)
    void box(uint32_t rec, float lo[3], float hi[3]) const {
        for (int a = 0; a < 3; a++) {
            const float o = f(rec, a), e = end(rec, a);
            const float c[4] = {o - radius, o + radius, e - radius, e + radius};
            lo[a] = kF32Max; hi[a] = -kF32Max;
            for (int k = 0; k < 4; k++) { lo[a] = std::fmin(lo[a], c[k]); hi[a] = std::fmax(hi[a], c[k]); }
        }
    }
    // self.o + self.d * self.length * 0.5
    float key(uint32_t rec, int a) const { return f(rec, a) + (f(rec, 4 + a) * f(rec, 3)) * 0.5f; }
};

// o, d and the length of every record are finite
int check_beam_records(const uint32_t* words, size_t n) {
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 7; k++)
            if (!std::isfinite(word_f(words, i, k))) { rl_set_error("a beam's origin, direction or length is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    return RL_OK;
}

}  // namespace

int split_beams(const uint32_t* words, size_t n, std::vector<uint32_t>* out) {
    if (!out || (n && !words)) return RL_ERR_INVALID_ARGUMENT;
    out->clear();
    if (n > (size_t)RL_BEAM_MAX + 4096) { rl_set_error("too many beams"); return RL_ERR_INVALID_ARGUMENT; }
    int rcode;
    if ((rcode = check_beam_records(words, n)) != RL_OK) return rcode;
    if (n == 0) return RL_OK;
    float sum = 0.0f;
    for (size_t i = 0; i < n; i++) sum = sum + word_f(words, i, 3);         // beams.iter().map(|b| b.length).sum::<f32>()
    const float avg_split = sum / (float)(n * kBeamSplit);                  // / (beams.len() * SPLIT) as f32
    if (!std::isfinite(avg_split) || avg_split == 0.0f) { rl_set_error("the beams' average split length is zero or not finite"); return RL_ERR_INVALID_ARGUMENT; }
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        total += as_u32(std::ceil(word_f(words, i, 3) / avg_split));
        if (total > kElementTreeMax) { rl_set_error("the split makes more sub-beams than a tree takes"); return RL_ERR_UNSUPPORTED; }
    }
    out->reserve(total * RL_BEAM_WORDS);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* w = words + i * RL_BEAM_WORDS;
        const float length = word_f(words, i, 3);
        const uint32_t number_split = as_u32(std::ceil(length / avg_split));
        const float new_length = length / (float)number_split;
        for (uint32_t s = 0; s < number_split; s++) {
            uint32_t sub[RL_BEAM_WORDS];
            std::memcpy(sub, w, sizeof sub);
            for (int a = 0; a < 3; a++) {
                const float o = word_f(words, i, a) + (word_f(words, i, 4 + a) * (float)s) * new_length;      // b.o + b.d * (i as f32) * new_length
                std::memcpy(&sub[a], &o, sizeof o);
            }
            std::memcpy(&sub[3], &new_length, sizeof new_length);
            out->insert(out->end(), sub, sub + RL_BEAM_WORDS);
        }
    }
    return RL_OK;
}

int build_beam_tree(const uint32_t* sub_words, size_t n_sub, float radius, ElementTree* out) {
    if (!out || (n_sub && !sub_words)) return RL_ERR_INVALID_ARGUMENT;
    int rcode;
    if ((rcode = check_photon_radius(radius)) != RL_OK) return rcode;
    if (n_sub > kElementTreeMax) { rl_set_error("too many sub-beams"); return RL_ERR_INVALID_ARGUMENT; }
    if ((rcode = check_beam_records(sub_words, n_sub)) != RL_OK) return rcode;
    const BeamElems e{sub_words, radius};
    for (size_t i = 0; i < n_sub; i++) {
        float lo[3], hi[3];
        e.box((uint32_t)i, lo, hi);
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !std::isfinite(e.key((uint32_t)i, a))) { rl_set_error("a beam's box is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    }
    build_element_tree(e, n_sub, out);
    return RL_OK;
}

}  // namespace rl

extern "C" int rl_beam_split(const uint32_t* words, size_t n_beams, size_t capacity, size_t* n_sub, uint32_t* sub_words) {
    if (!n_sub) return RL_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> sub;
    const int rcode = rl::split_beams(words, n_beams, &sub);
    if (rcode != RL_OK) return rcode;
    *n_sub = sub.size() / RL_BEAM_WORDS;
    if (!sub_words) return RL_OK;      // the size only
    if (capacity < *n_sub) { rl_set_error("rl_beam_split: capacity is too small"); return RL_ERR_INVALID_ARGUMENT; }
    std::copy(sub.begin(), sub.end(), sub_words);
    return RL_OK;
}

extern "C" int rl_beam_tree_build(const uint32_t* sub_words, size_t n_sub, float radius, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                                  uint32_t* node_links, uint32_t* order) {
    if (!n_nodes) return RL_ERR_INVALID_ARGUMENT;
    rl::ElementTree t;
    const int rcode = rl::build_beam_tree(sub_words, n_sub, radius, &t);
    if (rcode != RL_OK) return rcode;
    return rl::copy_tree_out(t, node_capacity, n_nodes, node_boxes, node_links, order, "rl_beam_tree_build");
}
