// phototree.hip.h — the photon tree of the beam radiance estimate built on the device, bit for bit the tree of host/photontree.cpp.
// Instantiated by phototree.hip, which also holds the host driver (photon_tree_run).
//
// Two facts carry it (tests/test_photon_tree_levels.py pins both to the host build):
//  1. The topology depends on n alone.  A range of m photons is a leaf iff m <= 4, else it splits into floor(m / 2) on the left and ceil(m / 2) on the
//     right, and the right subtree is numbered first: a node i over m photons has skip = i + N(m), its right child at i + 1 and its left child at
//     i + 1 + N(ceil(m / 2)), N = pt_node_count.  Every lane finds the range its place belongs to at a depth by halving from [0, n): no table.
//  2. The host's stable sort of a range by pos[axis] is ANY sort by the unique pair (ordered key of pos[axis], place before this node's sort).  Ordered
//     key: -0 -> +0 (the host compares with <), then negative -> all bits inverted, else sign bit set.
// Boxes are min / max over finite floats (exact, associative, commutative; p -+ r with r > 0 is never -0), taken on the same ordered integers.
//
// Levels whose ranges hold more than T photons (T = RL_PHOTON_TREE_GROUP_PHOTONS, or the knob photon_tree_group_photons) run over the whole array:
//   k_pt_box       min / max of every such range into 6 ordered integers per range (atomicMin; the maxima stored inverted)
//   k_pt_sort      one workgroup per aligned chunk of T places: writes the nodes of the ranges that start in the chunk, sorts the chunk's part of every
//                  range in LDS (bitonic, on (range start | key | place)) and stores (key << 32 | place) per place
//   k_pt_merge     one pass per doubling of the run length: a key's new place is its index in its own run + the keys of the sibling run below it
//                  (binary search; the pairs are unique, so no tie rule is needed)
//   k_pt_permute   order'[j] = order[place of the key that ended at j]
// then k_pt_finish gives every range of at most T photons to one workgroup, which stages positions and indices in LDS and runs every remaining
// level there down to the leaves, and k_pt_photons writes the photons in leaf order.  Nothing depends on launch geometry, arrival order or T:
// every stored value is a min / max or a function of a unique key.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/rustlight_amd.h"

namespace rl {

static constexpr unsigned kPtThreads = 256;
static constexpr unsigned kPtGroup = RL_PHOTON_TREE_GROUP_PHOTONS;     // T: photons one workgroup finishes in LDS
static constexpr unsigned kPtSlots = kPtGroup / kPtThreads;           // places per lane in k_pt_sort / k_pt_finish
static constexpr unsigned kPtPlaceBits = 11;                           // a place within a group: kPtGroup = 1 << kPtPlaceBits
static constexpr unsigned kPtSerialBox = 32;                           // k_pt_finish: a range of at most this many photons has its box taken by one lane
static constexpr unsigned kPtBoxRanges = kPtGroup / kPtSerialBox;      // larger ranges: LDS atomics, one row per range (range start / kPtSerialBox is unique)
static_assert(kPtGroup == 1u << kPtPlaceBits && kPtGroup % kPtThreads == 0, "the group is a power of two and a multiple of the workgroup");

// N(m): nodes of the subtree over m photons.  Every level holds ranges of two sizes only, s (c0 of them) and s + 1 (c1 of them).
__host__ __device__ inline unsigned pt_node_count(unsigned m) {
    if (m <= 4u) return m ? 1u : 0u;
    unsigned s = m, c0 = 1u, c1 = 0u, total = 0u;
    for (;;) {
        total += c0 + c1;
        if (s + 1u <= 4u || (s <= 4u && c1 == 0u)) break;      // all of them leaves
        if (s == 4u) { total += 2u * c1; break; }              // the 4s are leaves, the 5s split into leaves of 2 and 3
        if (s & 1u) { c1 = c0 + 2u * c1; s = (s - 1u) / 2u; }  // s -> (s-1)/2, (s+1)/2; s+1 -> (s+1)/2 twice
        else { c0 = 2u * c0 + c1; s = s / 2u; }                // s -> s/2 twice; s+1 -> s/2, s/2+1
    }
    return total;
}

__device__ inline unsigned pt_ord(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ inline float pt_unord(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ inline unsigned pt_sort_key(float f) { return pt_ord(__float_as_uint(f) == 0x80000000u ? 0.0f : f); }
__device__ inline float pt_pos(const unsigned* words, unsigned rec, unsigned axis) { return __uint_as_float(words[(size_t)rec * RL_VPL_WORDS + 4u + axis]); }
// the host's axis rule on hi - lo
__device__ inline unsigned pt_axis(const float* lo, const float* hi) {
    const float sx = hi[0] - lo[0], sy = hi[1] - lo[1], sz = hi[2] - lo[2];
    return sx > sy ? (sx > sz ? 0u : 2u) : (sy > sz ? 1u : 2u);
}
__device__ inline void pt_store_node(float4* nodes, unsigned node, const float* lo, const float* hi, unsigned skip, unsigned first_count) {
    nodes[2u * (size_t)node] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    nodes[2u * (size_t)node + 1u] = make_float4(hi[1], hi[2], __uint_as_float(skip), __uint_as_float(first_count));
}

// The range place j belongs to at `depth`, while every range above it holds more than `group` photons: b, e, h = its index in heap numbering
// (root 1, left 2h, right 2h + 1).  active = false: j >= n, or a range on the way down already fits a workgroup (k_pt_finish takes it).
struct PtRange { unsigned b, e, h; bool active; };
__device__ inline PtRange pt_descend(unsigned n, unsigned j, unsigned depth, unsigned group) {
    PtRange r{0u, n, 1u, j < n};
    if (!r.active) return r;
    for (unsigned d = 0; d < depth; d++) {
        if (r.e - r.b <= group) { r.active = false; return r; }
        const unsigned split = (r.b + r.e) / 2u;
        if (j < split) { r.e = split; r.h = 2u * r.h; } else { r.b = split; r.h = 2u * r.h + 1u; }
    }
    r.active = r.e - r.b > group;
    return r;
}
// the node index of the range [b, e) at `depth` that starts at place b (walked again with the closed form; one lane per range does it)
__device__ inline unsigned pt_node_of(unsigned n, unsigned j, unsigned depth) {
    unsigned b = 0u, e = n, node = 0u;
    for (unsigned d = 0; d < depth; d++) {
        const unsigned m = e - b, split = (b + e) / 2u;
        if (j < split) { node += 1u + pt_node_count(m - m / 2u); e = split; } else { node += 1u; b = split; }
    }
    return node;
}

// ---- the check pass: bit 0 = a record that is no volume record (check_kind), bit 1 = a position that is not finite
__global__ void __launch_bounds__(kPtThreads) k_pt_check(const unsigned* words, unsigned n, int check_kind, unsigned* flag) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned* w = words + (size_t)j * RL_VPL_WORDS;
    unsigned bad = (check_kind && w[0] != (unsigned)RL_VPL_KIND_VOLUME) ? 1u : 0u;
    for (unsigned a = 0; a < 3u; a++)
        if ((w[4u + a] & 0x7f800000u) == 0x7f800000u) bad |= 2u;
    if (bad) atomicOr(flag, bad);
}
__global__ void __launch_bounds__(kPtThreads) k_pt_iota(unsigned* order, unsigned n) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j < n) order[j] = j;
}

// ---- global levels
// acc[h][6]: ordered lo.xyz, then INVERTED ordered hi.xyz, so that one memset to 0xff initialises both and both are atomicMin
__global__ void __launch_bounds__(kPtThreads) k_pt_box(const unsigned* words, const unsigned* order, unsigned n, float radius, unsigned depth, unsigned group, unsigned* acc) {
    __shared__ unsigned s_red[kPtThreads / 64u][6];
    const unsigned j0 = blockIdx.x * kPtThreads, j = j0 + threadIdx.x;
    const PtRange r = pt_descend(n, j, depth, group);
    unsigned v[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (r.active) {
        const unsigned rec = order[j];
        for (unsigned a = 0; a < 3u; a++) {
            const float p = pt_pos(words, rec, a);
            v[a] = pt_ord(fminf(p - radius, p + radius));
            v[3u + a] = ~pt_ord(fmaxf(p - radius, p + radius));
        }
    }
    // the whole workgroup inside one range (the common case on the top levels): reduce first, 6 atomics per workgroup
    const PtRange r0 = pt_descend(n, j0, depth, group);
    const unsigned last = min(n, j0 + kPtThreads) - 1u;
    if (r0.active && r0.e > last) {
        for (unsigned a = 0; a < 6u; a++) {
            unsigned x = v[a];
            for (unsigned off = 32u; off > 0u; off >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, (int)off, 64));
            if ((threadIdx.x & 63u) == 0u) s_red[threadIdx.x >> 6][a] = x;
        }
        __syncthreads();
        if (threadIdx.x < 6u) {
            unsigned x = s_red[0][threadIdx.x];
            for (unsigned w = 1; w < kPtThreads / 64u; w++) x = min(x, s_red[w][threadIdx.x]);
            atomicMin(&acc[(size_t)r0.h * 6u + threadIdx.x], x);
        }
    } else if (r.active) {
        for (unsigned a = 0; a < 6u; a++) atomicMin(&acc[(size_t)r.h * 6u + a], v[a]);
    }
}

// bitonic sort of a[0 .. p2) (p2 a power of two >= 2) by the whole workgroup; the caller has synchronised after filling a, and it ends synchronised
__device__ inline void pt_bitonic(unsigned long long* a, unsigned p2) {
    for (unsigned k = 2u; k <= p2; k <<= 1)
        for (unsigned jj = k >> 1; jj > 0u; jj >>= 1) {
            for (unsigned t = threadIdx.x; t < p2 / 2u; t += kPtThreads) {
                const unsigned i = ((t & ~(jj - 1u)) << 1) | (t & (jj - 1u)), l = i | jj;
                const bool up = (i & k) == 0u;
                const unsigned long long x = a[i], y = a[l];
                if ((x > y) == up) { a[i] = y; a[l] = x; }
            }
            __syncthreads();
        }
}

// one workgroup per chunk [c * group, (c + 1) * group): nodes of the active ranges that start here, then the chunk's part of every active range sorted
// by (key of pos[axis], place); keys[j] = key << 32 | place for the active places.  p2: the power of two >= group the LDS sort runs over.
__global__ void __launch_bounds__(kPtThreads) k_pt_sort(const unsigned* words, const unsigned* order, unsigned n, unsigned depth, unsigned group, unsigned p2,
                                                        const unsigned* acc, float4* nodes, unsigned long long* keys) {
    __shared__ unsigned long long s_key[kPtGroup];
    const unsigned c0 = blockIdx.x * group;
    unsigned active = 0u;
#pragma unroll
    for (unsigned s = 0; s < kPtSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        if (i >= p2) continue;
        unsigned long long key = ~0ull;                                  // padding sorts to the end
        const unsigned j = c0 + i;
        if (i < group && j < n) {
            key = (unsigned long long)i << (32u + kPtPlaceBits) | i;       // a place of a range that is not sorted here stays where it is
            const PtRange r = pt_descend(n, j, depth, group);
            if (r.active) {
                float lo[3], hi[3];
                for (unsigned a = 0; a < 3u; a++) { lo[a] = pt_unord(acc[(size_t)r.h * 6u + a]); hi[a] = pt_unord(~acc[(size_t)r.h * 6u + 3u + a]); }
                const unsigned axis = pt_axis(lo, hi);
                if (j == r.b) { const unsigned node = pt_node_of(n, j, depth); pt_store_node(nodes, node, lo, hi, node + pt_node_count(r.e - r.b), 0u); }
                const unsigned start = max(r.b, c0) - c0;              // the range's first place in this chunk
                key = (unsigned long long)start << (32u + kPtPlaceBits) | (unsigned long long)pt_sort_key(pt_pos(words, order[j], axis)) << kPtPlaceBits | i;
                active |= 1u << s;
            }
        }
        s_key[i] = key;
    }
    if (!__syncthreads_or((int)active)) return;
    pt_bitonic(s_key, p2);
#pragma unroll
    for (unsigned s = 0; s < kPtSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        if (!(active >> s & 1u)) continue;
        const unsigned long long k = s_key[i];
        keys[c0 + i] = (k >> kPtPlaceBits & 0xffffffffull) << 32 | (c0 + (unsigned)(k & (kPtGroup - 1u)));
    }
}

// pass p: runs of 2^p chunks (cut to the range) merge in pairs
__global__ void __launch_bounds__(kPtThreads) k_pt_merge(const unsigned long long* in, unsigned long long* out, unsigned n, unsigned depth, unsigned group, unsigned p) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    const PtRange r = pt_descend(n, j, depth, group);
    if (!r.active) return;
    const unsigned first = r.b / group, c = j / group - first, run = 1u << p;
    const unsigned ca = first + ((c >> (p + 1u)) << (p + 1u));           // the pair's first chunk
    const unsigned a0 = max(r.b, ca * group), a1 = min(r.e, (ca + run) * group), b1 = min(r.e, (ca + 2u * run) * group);      // A = [a0, a1), B = [a1, b1)
    const unsigned long long key = in[j];
    const bool in_a = j < a1;
    unsigned lo = in_a ? a1 : a0, hi = in_a ? b1 : a1;                    // count the other run's keys below this one
    const unsigned other = lo;
    while (lo < hi) {
        const unsigned mid = (lo + hi) / 2u;
        if (in[mid] < key) lo = mid + 1u; else hi = mid;
    }
    out[a0 + (j - (in_a ? a0 : a1)) + (lo - other)] = key;
}

__global__ void __launch_bounds__(kPtThreads) k_pt_permute(const unsigned long long* keys, const unsigned* order_in, unsigned* order_out, unsigned n, unsigned depth, unsigned group) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const PtRange r = pt_descend(n, j, depth, group);
    order_out[j] = order_in[r.active ? (unsigned)(keys[j] & 0xffffffffull) : j];
}

// ---- subtree finish: workgroup = one range of at most `group` photons, roots[g] = (begin, end, node index).  LDS: positions and record indices as staged,
// s_lidx[place] = the staged photon that stands at the place, the sort keys, the axis per range start, the box rows of the large ranges
__global__ void __launch_bounds__(kPtThreads) k_pt_finish(const uint3* roots, const unsigned* words, float radius, const unsigned* order_in, unsigned* order_out,
                                                          float4* nodes, unsigned p2) {
    __shared__ float s_pos[3][kPtGroup];
    __shared__ unsigned s_rec[kPtGroup];
    __shared__ unsigned long long s_key[kPtGroup];
    __shared__ unsigned short s_lidx[kPtGroup];
    __shared__ unsigned char s_axis[kPtGroup];
    __shared__ unsigned s_box[kPtBoxRanges][6];
    const uint3 root = roots[blockIdx.x];
    const unsigned rb = root.x, m = root.y - root.x;
    unsigned lb[kPtSlots], le[kPtSlots], node[kPtSlots], moved[kPtSlots];
    unsigned done = 0u;                                                  // bit s: the place's leaf is written
#pragma unroll
    for (unsigned s = 0; s < kPtSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        lb[s] = 0u; le[s] = m; node[s] = root.z; moved[s] = 0u;
        if (i < m) {
            const unsigned rec = order_in[rb + i];
            s_rec[i] = rec; s_lidx[i] = (unsigned short)i;
            for (unsigned a = 0; a < 3u; a++) s_pos[a][i] = pt_pos(words, rec, a);
        } else done |= 1u << s;                                          // no place
    }
    const unsigned no_place = done;
    for (unsigned cm = m;; cm = (cm + 1u) / 2u) {                        // cm: the largest range of this level
        for (unsigned t = threadIdx.x; t < kPtBoxRanges * 6u; t += kPtThreads) s_box[t / 6u][t % 6u] = 0xffffffffu;
        __syncthreads();
#pragma unroll
        for (unsigned s = 0; s < kPtSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if ((done >> s & 1u) || le[s] - lb[s] <= kPtSerialBox) continue;
            const unsigned li = s_lidx[i];
            for (unsigned a = 0; a < 3u; a++) {
                const float p = s_pos[a][li];
                atomicMin(&s_box[lb[s] / kPtSerialBox][a], pt_ord(fminf(p - radius, p + radius)));
                atomicMin(&s_box[lb[s] / kPtSerialBox][3u + a], ~pt_ord(fmaxf(p - radius, p + radius)));
            }
        }
        __syncthreads();
        // the lane at a range's first place writes its node
#pragma unroll
        for (unsigned s = 0; s < kPtSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if ((done >> s & 1u) || i != lb[s]) continue;
            const unsigned sm = le[s] - lb[s];
            float lo[3], hi[3];
            if (sm > kPtSerialBox) {
                for (unsigned a = 0; a < 3u; a++) { lo[a] = pt_unord(s_box[i / kPtSerialBox][a]); hi[a] = pt_unord(~s_box[i / kPtSerialBox][3u + a]); }
            } else {
                unsigned v[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
                for (unsigned q = i; q < i + sm; q++) {
                    const unsigned li = s_lidx[q];
                    for (unsigned a = 0; a < 3u; a++) {
                        const float p = s_pos[a][li];
                        v[a] = min(v[a], pt_ord(fminf(p - radius, p + radius)));
                        v[3u + a] = min(v[3u + a], ~pt_ord(fmaxf(p - radius, p + radius)));
                    }
                }
                for (unsigned a = 0; a < 3u; a++) { lo[a] = pt_unord(v[a]); hi[a] = pt_unord(~v[3u + a]); }
            }
            if (sm <= 4u) pt_store_node(nodes, node[s], lo, hi, node[s] + 1u, (rb + i) << 3 | sm);
            else { s_axis[i] = (unsigned char)pt_axis(lo, hi); pt_store_node(nodes, node[s], lo, hi, node[s] + pt_node_count(sm), 0u); }
        }
        __syncthreads();
        if (cm <= 4u) break;                                             // every range of this level was a leaf
#pragma unroll
        for (unsigned s = 0; s < kPtSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if (i >= p2) continue;
            unsigned long long key = ~0ull;
            if (!(no_place >> s & 1u)) {
                key = (unsigned long long)i << (32u + kPtPlaceBits) | i;   // a leaf's places stay
                if (!(done >> s & 1u) && le[s] - lb[s] > 4u)
                    key = (unsigned long long)lb[s] << (32u + kPtPlaceBits) | (unsigned long long)pt_sort_key(s_pos[s_axis[lb[s]]][s_lidx[i]]) << kPtPlaceBits | i;
            }
            s_key[i] = key;
        }
        __syncthreads();
        pt_bitonic(s_key, p2);
#pragma unroll
        for (unsigned s = 0; s < kPtSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if (!(no_place >> s & 1u)) moved[s] = s_lidx[(unsigned)(s_key[i] & (kPtGroup - 1u))];
        }
        __syncthreads();
#pragma unroll
        for (unsigned s = 0; s < kPtSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if (no_place >> s & 1u) continue;
            s_lidx[i] = (unsigned short)moved[s];
            if (done >> s & 1u) continue;
            const unsigned sm = le[s] - lb[s], split = (lb[s] + le[s]) / 2u;
            if (sm <= 4u) done |= 1u << s;
            else if (i < split) { node[s] += 1u + pt_node_count(sm - sm / 2u); le[s] = split; }
            else { node[s] += 1u; lb[s] = split; }
        }
    }
#pragma unroll
    for (unsigned s = 0; s < kPtSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        if (!(no_place >> s & 1u)) order_out[rb + i] = s_rec[s_lidx[i]];
    }
}

// ---- emit: the photons in leaf order, 3 float4 each = pos | radiance | d_in (words 4 .. 12 of the record), w = 0
__global__ void __launch_bounds__(kPtThreads) k_pt_photons(const unsigned* words, const unsigned* order, unsigned n, float4* photons) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned* w = words + (size_t)order[j] * RL_VPL_WORDS + 4u;
    for (unsigned q = 0; q < 3u; q++)
        photons[3u * (size_t)j + q] = make_float4(__uint_as_float(w[3u * q]), __uint_as_float(w[3u * q + 1u]), __uint_as_float(w[3u * q + 2u]), 0.0f);
}

}  // namespace rl
