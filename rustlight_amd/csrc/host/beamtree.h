// beamtree.h — the host side of the photon beams (beamtree.cpp): the split into sub-beams and the tree over them, an ElementTree of photontree.h
#pragma once
#include "photontree.h"

namespace rl {

constexpr size_t kBeamSplit = 5;      // SPLIT (vol_primitives.rs:652)

// words: n records of RL_BEAM_WORDS u32 -> the sub-beams, records of the same layout in beam order.  RL_OK; RL_ERR_INVALID_ARGUMENT for a record whose o, d or
// length is not finite or a zero or non-finite avg_split; RL_ERR_UNSUPPORTED when the split exceeds kElementTreeMax — each with rl_last_error set.
int split_beams(const uint32_t* words, size_t n, std::vector<uint32_t>* out);
// sub_words: n_sub records of RL_BEAM_WORDS u32 (o, length and d are read).  RL_OK, or RL_ERR_INVALID_ARGUMENT with rl_last_error set.
int build_beam_tree(const uint32_t* sub_words, size_t n_sub, float radius, ElementTree* out);

}  // namespace rl
