// phototree.hip.h — the element trees of the camera-beam gathers built on the device, bit for bit the trees of host/photontree.cpp and host/planetree.cpp
// (DESIGN.md §7).  Every kernel body and the host driver (element_tree_run) are templates over an element type E, the device's form of the E of the host's
// ElementTreeBuilder: the box of a record and its sort key on an axis; the check of the records is a pass of each family's own (k_pt_check, k_plt_pre).  phototree.hip instantiates them for photons (PhotonElem, the
// kernels k_pt_*), planetree.hip for the photon planes (PlaneElem, the kernels k_plt_*): the kernels themselves are plain wrappers, so that each family
// keeps its own names in its own code object.
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
//
// Planes (PlaneElem).  k_plt_pre computes a plane's 6 box floats and 3 keys once per build into pre[n][9] (the host's operations, each a separately rounded
// f32: contraction is off) and raises the check flag for a corner that is not finite; the levels read pre[], and k_plt_finish stages the 9 floats.
// Group: T = RL_PLANE_TREE_GROUP_PLANES = 1024.  k_plt_finish's LDS is 52.5 bytes per place (36 staged floats, 4 record index, 8 sort key, 2 place, 1 axis,
// 1.5 box rows of 64-bit words) = 53,760 bytes at 1024: under half of the 160 KiB a gfx950 workgroup may declare, so two workgroups share a compute unit as
// they do for photons (56,832 bytes at 2048).  At 2048 it would take 107,520 bytes, legal, but one workgroup per compute unit.
// Signed zeros.  A photon box never holds -0; a plane box can (a corner at -0 beside one at +0).  The host takes std::fmin / std::fmax in index order,
// which the host build compiles to libm's fminf / fmaxf: of two zeros of different sign BOTH return their SECOND argument (x < y ? x : y, x > y ? x : y).
// So a box coordinate that is zero carries the sign of the LAST zero that entered it: the last such corner of a plane, then the last such plane of the
// range in the order the range has before its own sort.  The device takes that minimum on 64-bit words: the ordered integer of the value with -0 mapped
// to +0 in the high half, ~(place << 1 | sign) in the low half, so that among equal values the largest place wins and brings its sign along.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../../include/rustlight_amd.h"
#include "../host/hip_buffer.h"

#pragma clang fp contract(off)

namespace rl {

static constexpr unsigned kPtThreads = 256;
static constexpr unsigned kPtPlaceBits = 11;                           // a place within a group: every group is at most 1 << kPtPlaceBits
static constexpr unsigned kPtSerialBox = 32;                           // k_pt_finish: a range of at most this many elements has its box taken by one lane

// N(m): nodes of the subtree over m elements.  Every level holds ranges of two sizes only, s (c0 of them) and s + 1 (c1 of them).
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
__device__ inline unsigned pt_shfl_xor(unsigned x, unsigned off) { return (unsigned)__shfl_xor((int)x, (int)off, 64); }
__device__ inline unsigned long long pt_shfl_xor(unsigned long long x, unsigned off) {
    return (unsigned long long)pt_shfl_xor((unsigned)(x >> 32), off) << 32 | pt_shfl_xor((unsigned)x, off);
}

// ---- the elements.  An element type E holds the build's inputs and supplies
//   kGroup, kStage      the largest group T, and the floats k_pt_finish stages per element
//   Acc                 the word a box coordinate is reduced in with atomicMin (all bits set = empty): enc_lo / enc_hi (value, place), dec_lo / dec_hi
//   box(rec, lo, hi), key(rec, axis)          from global memory (the levels over the whole array)
//   stage(rec, k), s_lo / s_hi / s_key(g, axis)      the k-th staged float, and the same three from the staged floats g(k)
struct PhotonElem {
    static constexpr unsigned kGroup = RL_PHOTON_TREE_GROUP_PHOTONS, kStage = 3u;
    using Acc = unsigned;
    const unsigned* words;      // [n][RL_VPL_WORDS]
    float radius;
    __device__ void box(unsigned rec, float* lo, float* hi) const {
        for (unsigned a = 0; a < 3u; a++) { const float p = pt_pos(words, rec, a); lo[a] = fminf(p - radius, p + radius); hi[a] = fmaxf(p - radius, p + radius); }
    }
    __device__ float key(unsigned rec, unsigned axis) const { return pt_pos(words, rec, axis); }
    __device__ float stage(unsigned rec, unsigned k) const { return pt_pos(words, rec, k); }
    template <class G> __device__ float s_lo(G g, unsigned a) const { const float p = g(a); return fminf(p - radius, p + radius); }
    template <class G> __device__ float s_hi(G g, unsigned a) const { const float p = g(a); return fmaxf(p - radius, p + radius); }
    template <class G> __device__ float s_key(G g, unsigned a) const { return g(a); }
    // p -+ r with r > 0 is never -0: the ordered integer alone
    static __device__ Acc enc_lo(float v, unsigned) { return pt_ord(v); }
    static __device__ Acc enc_hi(float v, unsigned) { return ~pt_ord(v); }
    static __device__ float dec_lo(Acc x) { return pt_unord(x); }
    static __device__ float dec_hi(Acc x) { return pt_unord(~x); }
};

// the host's fminf / fmaxf on finite floats: of two equal values (two zeros of different sign) the second
__device__ inline float pt_host_min(float x, float y) { return x < y ? x : y; }
__device__ inline float pt_host_max(float x, float y) { return x > y ? x : y; }
struct PlaneElem {
    static constexpr unsigned kGroup = RL_PLANE_TREE_GROUP_PLANES, kStage = 9u;
    using Acc = unsigned long long;
    const float* pre;           // [n][9]: lo.xyz, hi.xyz, key.xyz (k_plt_pre)
    __device__ void box(unsigned rec, float* lo, float* hi) const {
        for (unsigned a = 0; a < 3u; a++) { lo[a] = pre[(size_t)rec * 9u + a]; hi[a] = pre[(size_t)rec * 9u + 3u + a]; }
    }
    __device__ float key(unsigned rec, unsigned axis) const { return pre[(size_t)rec * 9u + 6u + axis]; }
    __device__ float stage(unsigned rec, unsigned k) const { return pre[(size_t)rec * 9u + k]; }
    template <class G> __device__ float s_lo(G g, unsigned a) const { return g(a); }
    template <class G> __device__ float s_hi(G g, unsigned a) const { return g(3u + a); }
    template <class G> __device__ float s_key(G g, unsigned a) const { return g(6u + a); }
    // value with -0 -> +0 | ~(place << 1 | sign): among equal values the last place wins, with its sign (the header comment)
    static __device__ unsigned tie(float v, unsigned place) { return ~(place << 1 | __float_as_uint(v) >> 31); }
    static __device__ Acc enc_lo(float v, unsigned place) { return (Acc)pt_ord(v == 0.0f ? 0.0f : v) << 32 | tie(v, place); }
    static __device__ Acc enc_hi(float v, unsigned place) { return (Acc)~pt_ord(v == 0.0f ? 0.0f : v) << 32 | tie(v, place); }
    static __device__ float signed_zero(float v, Acc x) { return v == 0.0f ? __uint_as_float((~(unsigned)x & 1u) << 31) : v; }
    static __device__ float dec_lo(Acc x) { return signed_zero(pt_unord((unsigned)(x >> 32)), x); }
    static __device__ float dec_hi(Acc x) { return signed_zero(pt_unord(~(unsigned)(x >> 32)), x); }
};
// the prepass of a plane build: box and keys of record j as host/planetree.cpp's PlaneElems takes them, flag bit 2 = a corner that is not finite
__device__ __forceinline__ void plt_pre_body(const unsigned* words, unsigned n, float* pre, unsigned* flag) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned* w = words + (size_t)j * RL_PLANE_WORDS;
    const float l0 = __uint_as_float(w[9]), l1 = __uint_as_float(w[10]);
    bool bad = false;
    for (unsigned a = 0; a < 3u; a++) {
        const float o = __uint_as_float(w[a]), e0 = __uint_as_float(w[3u + a]) * l0, e1 = __uint_as_float(w[6u + a]) * l1;
        const float p0 = o + e0;
        const float c[4] = {o, p0, o + e1, p0 + e1};
        float lo = 3.402823466e+38f, hi = -3.402823466e+38f;
        for (unsigned k = 0; k < 4u; k++) {
            bad |= (__float_as_uint(c[k]) & 0x7f800000u) == 0x7f800000u;
            lo = pt_host_min(lo, c[k]); hi = pt_host_max(hi, c[k]);
        }
        pre[(size_t)j * 9u + a] = lo; pre[(size_t)j * 9u + 3u + a] = hi;
        pre[(size_t)j * 9u + 6u + a] = (o + e0 * 0.5f) + e1 * 0.5f;
    }
    if (bad) atomicOr(flag, 4u);
}
// the planes in leaf order, 4 float4 each = o, length0 | d0, length1 | d1, type | id_emitter << 2 | weight, 0 (what rl_plane_map_build packs)
__device__ __forceinline__ void plt_planes_body(const unsigned* words, const unsigned* order, unsigned n, float4* planes) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned* w = words + (size_t)order[j] * RL_PLANE_WORDS;
    const auto f = [&](unsigned k) { return __uint_as_float(w[k]); };
    planes[4u * (size_t)j] = make_float4(f(0), f(1), f(2), f(9));
    planes[4u * (size_t)j + 1u] = make_float4(f(3), f(4), f(5), f(10));
    planes[4u * (size_t)j + 2u] = make_float4(f(6), f(7), f(8), __uint_as_float(w[16] | w[17] << 2));
    planes[4u * (size_t)j + 3u] = make_float4(f(11), f(12), f(13), 0.0f);
}

// The range place j belongs to at `depth`, while every range above it holds more than `group` elements: b, e, h = its index in heap numbering
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

// ---- the photons' check pass: bit 0 = a record that is no volume record (check_kind), bit 1 = a position that is not finite
__device__ __forceinline__ void pt_check_body(const unsigned* words, unsigned n, int check_kind, unsigned* flag) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned* w = words + (size_t)j * RL_VPL_WORDS;
    unsigned bad = (check_kind && w[0] != (unsigned)RL_VPL_KIND_VOLUME) ? 1u : 0u;
    for (unsigned a = 0; a < 3u; a++)
        if ((w[4u + a] & 0x7f800000u) == 0x7f800000u) bad |= 2u;
    if (bad) atomicOr(flag, bad);
}
__device__ __forceinline__ void pt_iota_body(unsigned* order, unsigned n) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j < n) order[j] = j;
}

// ---- global levels
// acc[h][6]: lo.xyz, then hi.xyz with the value INVERTED, so that one memset to 0xff initialises both and both are atomicMin
template <class E>
__device__ __forceinline__ void pt_box_body(const E& el, const unsigned* order, unsigned n, unsigned depth, unsigned group, typename E::Acc* acc) {
    using Acc = typename E::Acc;
    __shared__ Acc s_red[kPtThreads / 64u][6];
    const unsigned j0 = blockIdx.x * kPtThreads, j = j0 + threadIdx.x;
    const PtRange r = pt_descend(n, j, depth, group);
    Acc v[6] = {~(Acc)0, ~(Acc)0, ~(Acc)0, ~(Acc)0, ~(Acc)0, ~(Acc)0};
    if (r.active) {
        float lo[3], hi[3];
        el.box(order[j], lo, hi);
        for (unsigned a = 0; a < 3u; a++) { v[a] = E::enc_lo(lo[a], j); v[3u + a] = E::enc_hi(hi[a], j); }
    }
    // the whole workgroup inside one range (the common case on the top levels): reduce first, 6 atomics per workgroup
    const PtRange r0 = pt_descend(n, j0, depth, group);
    const unsigned last = min(n, j0 + kPtThreads) - 1u;
    if (r0.active && r0.e > last) {
        for (unsigned a = 0; a < 6u; a++) {
            Acc x = v[a];
            for (unsigned off = 32u; off > 0u; off >>= 1) x = min(x, pt_shfl_xor(x, off));
            if ((threadIdx.x & 63u) == 0u) s_red[threadIdx.x >> 6][a] = x;
        }
        __syncthreads();
        if (threadIdx.x < 6u) {
            Acc x = s_red[0][threadIdx.x];
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
// by (key on the axis, place); keys[j] = key << 32 | place for the active places.  p2: the power of two >= group the LDS sort runs over.
template <class E>
__device__ __forceinline__ void pt_sort_body(const E& el, const unsigned* order, unsigned n, unsigned depth, unsigned group, unsigned p2, const typename E::Acc* acc,
                                    float4* nodes, unsigned long long* keys) {
    constexpr unsigned kSlots = E::kGroup / kPtThreads;
    __shared__ unsigned long long s_key[E::kGroup];
    const unsigned c0 = blockIdx.x * group;
    unsigned active = 0u;
#pragma unroll
    for (unsigned s = 0; s < kSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        if (i >= p2) continue;
        unsigned long long key = ~0ull;                                  // padding sorts to the end
        const unsigned j = c0 + i;
        if (i < group && j < n) {
            key = (unsigned long long)i << (32u + kPtPlaceBits) | i;       // a place of a range that is not sorted here stays where it is
            const PtRange r = pt_descend(n, j, depth, group);
            if (r.active) {
                float lo[3], hi[3];
                for (unsigned a = 0; a < 3u; a++) { lo[a] = E::dec_lo(acc[(size_t)r.h * 6u + a]); hi[a] = E::dec_hi(acc[(size_t)r.h * 6u + 3u + a]); }
                const unsigned axis = pt_axis(lo, hi);
                if (j == r.b) { const unsigned node = pt_node_of(n, j, depth); pt_store_node(nodes, node, lo, hi, node + pt_node_count(r.e - r.b), 0u); }
                const unsigned start = max(r.b, c0) - c0;              // the range's first place in this chunk
                key = (unsigned long long)start << (32u + kPtPlaceBits) | (unsigned long long)pt_sort_key(el.key(order[j], axis)) << kPtPlaceBits | i;
                active |= 1u << s;
            }
        }
        s_key[i] = key;
    }
    if (!__syncthreads_or((int)active)) return;
    pt_bitonic(s_key, p2);
#pragma unroll
    for (unsigned s = 0; s < kSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        if (!(active >> s & 1u)) continue;
        const unsigned long long k = s_key[i];
        keys[c0 + i] = (k >> kPtPlaceBits & 0xffffffffull) << 32 | (c0 + (unsigned)(k & ((1u << kPtPlaceBits) - 1u)));
    }
}

// pass p: runs of 2^p chunks (cut to the range) merge in pairs
__device__ __forceinline__ void pt_merge_body(const unsigned long long* in, unsigned long long* out, unsigned n, unsigned depth, unsigned group, unsigned p) {
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

__device__ __forceinline__ void pt_permute_body(const unsigned long long* keys, const unsigned* order_in, unsigned* order_out, unsigned n, unsigned depth, unsigned group) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const PtRange r = pt_descend(n, j, depth, group);
    order_out[j] = order_in[r.active ? (unsigned)(keys[j] & 0xffffffffull) : j];
}

// ---- subtree finish: workgroup = one range of at most `group` elements, roots[g] = (begin, end, node index).  LDS: the staged floats and record indices,
// s_lidx[place] = the staged element that stands at the place, the sort keys, the axis per range start, the box rows of the large ranges
template <class E>
__device__ __forceinline__ void pt_finish_body(const E& el, const uint3* roots, const unsigned* order_in, unsigned* order_out, float4* nodes, unsigned p2) {
    using Acc = typename E::Acc;
    constexpr unsigned kGroup = E::kGroup, kSlots = kGroup / kPtThreads, kBoxRanges = kGroup / kPtSerialBox;      // box rows: range start / kPtSerialBox is unique
    static_assert(kGroup <= 1u << kPtPlaceBits && kGroup % kPtThreads == 0 && (kGroup & (kGroup - 1u)) == 0, "the group is a power of two, a multiple of the workgroup");
    __shared__ float s_pos[E::kStage][kGroup];
    __shared__ unsigned s_rec[kGroup];
    __shared__ unsigned long long s_key[kGroup];
    __shared__ unsigned short s_lidx[kGroup];
    __shared__ unsigned char s_axis[kGroup];
    __shared__ Acc s_box[kBoxRanges][6];
    const uint3 root = roots[blockIdx.x];
    const unsigned rb = root.x, m = root.y - root.x;
    unsigned lb[kSlots], le[kSlots], node[kSlots], moved[kSlots];
    unsigned done = 0u;                                                  // bit s: the place's leaf is written
#pragma unroll
    for (unsigned s = 0; s < kSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        lb[s] = 0u; le[s] = m; node[s] = root.z; moved[s] = 0u;
        if (i < m) {
            const unsigned rec = order_in[rb + i];
            s_rec[i] = rec; s_lidx[i] = (unsigned short)i;
            for (unsigned k = 0; k < E::kStage; k++) s_pos[k][i] = el.stage(rec, k);
        } else done |= 1u << s;                                          // no place
    }
    const unsigned no_place = done;
    for (unsigned cm = m;; cm = (cm + 1u) / 2u) {                        // cm: the largest range of this level
        for (unsigned t = threadIdx.x; t < kBoxRanges * 6u; t += kPtThreads) s_box[t / 6u][t % 6u] = ~(Acc)0;
        __syncthreads();
#pragma unroll
        for (unsigned s = 0; s < kSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if ((done >> s & 1u) || le[s] - lb[s] <= kPtSerialBox) continue;
            const unsigned li = s_lidx[i];
            const auto g = [&](unsigned k) { return s_pos[k][li]; };
            for (unsigned a = 0; a < 3u; a++) {
                atomicMin(&s_box[lb[s] / kPtSerialBox][a], E::enc_lo(el.s_lo(g, a), i));
                atomicMin(&s_box[lb[s] / kPtSerialBox][3u + a], E::enc_hi(el.s_hi(g, a), i));
            }
        }
        __syncthreads();
        // the lane at a range's first place writes its node
#pragma unroll
        for (unsigned s = 0; s < kSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if ((done >> s & 1u) || i != lb[s]) continue;
            const unsigned sm = le[s] - lb[s];
            float lo[3], hi[3];
            if (sm > kPtSerialBox) {
                for (unsigned a = 0; a < 3u; a++) { lo[a] = E::dec_lo(s_box[i / kPtSerialBox][a]); hi[a] = E::dec_hi(s_box[i / kPtSerialBox][3u + a]); }
            } else {
                Acc v[6] = {~(Acc)0, ~(Acc)0, ~(Acc)0, ~(Acc)0, ~(Acc)0, ~(Acc)0};
                for (unsigned q = i; q < i + sm; q++) {
                    const unsigned li = s_lidx[q];
                    const auto g = [&](unsigned k) { return s_pos[k][li]; };
                    for (unsigned a = 0; a < 3u; a++) {
                        v[a] = min(v[a], E::enc_lo(el.s_lo(g, a), q));
                        v[3u + a] = min(v[3u + a], E::enc_hi(el.s_hi(g, a), q));
                    }
                }
                for (unsigned a = 0; a < 3u; a++) { lo[a] = E::dec_lo(v[a]); hi[a] = E::dec_hi(v[3u + a]); }
            }
            if (sm <= 4u) pt_store_node(nodes, node[s], lo, hi, node[s] + 1u, (rb + i) << 3 | sm);
            else { s_axis[i] = (unsigned char)pt_axis(lo, hi); pt_store_node(nodes, node[s], lo, hi, node[s] + pt_node_count(sm), 0u); }
        }
        __syncthreads();
        if (cm <= 4u) break;                                             // every range of this level was a leaf
#pragma unroll
        for (unsigned s = 0; s < kSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if (i >= p2) continue;
            unsigned long long key = ~0ull;
            if (!(no_place >> s & 1u)) {
                key = (unsigned long long)i << (32u + kPtPlaceBits) | i;   // a leaf's places stay
                if (!(done >> s & 1u) && le[s] - lb[s] > 4u)
                    key = (unsigned long long)lb[s] << (32u + kPtPlaceBits) | (unsigned long long)pt_sort_key(el.s_key([&](unsigned k) { return s_pos[k][s_lidx[i]]; }, s_axis[lb[s]])) << kPtPlaceBits | i;
            }
            s_key[i] = key;
        }
        __syncthreads();
        pt_bitonic(s_key, p2);
#pragma unroll
        for (unsigned s = 0; s < kSlots; s++) {
            const unsigned i = threadIdx.x + s * kPtThreads;
            if (!(no_place >> s & 1u)) moved[s] = s_lidx[(unsigned)(s_key[i] & ((1u << kPtPlaceBits) - 1u))];
        }
        __syncthreads();
#pragma unroll
        for (unsigned s = 0; s < kSlots; s++) {
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
    for (unsigned s = 0; s < kSlots; s++) {
        const unsigned i = threadIdx.x + s * kPtThreads;
        if (!(no_place >> s & 1u)) order_out[rb + i] = s_rec[s_lidx[i]];
    }
}

// ---- emit: the photons in leaf order, 3 float4 each = pos | radiance | d_in (words 4 .. 12 of the record), w = 0
__device__ __forceinline__ void pt_photons_body(const unsigned* words, const unsigned* order, unsigned n, float4* photons) {
    const unsigned j = blockIdx.x * kPtThreads + threadIdx.x;
    if (j >= n) return;
    const unsigned* w = words + (size_t)order[j] * RL_VPL_WORDS + 4u;
    for (unsigned q = 0; q < 3u; q++)
        photons[3u * (size_t)j + q] = make_float4(__uint_as_float(w[3u * q]), __uint_as_float(w[3u * q + 1u]), __uint_as_float(w[3u * q + 2u]), 0.0f);
}

// The kernels of one family: PFX the prefix of their names (k_pt_ / k_plt_), E its element.  PFX##Kernels names them for element_tree_run.
#define RL_ELEMENT_TREE_KERNELS(PFX, E)                                                                                                                         \
    __global__ void __launch_bounds__(kPtThreads) PFX##iota(unsigned* order, unsigned n) { pt_iota_body(order, n); }                                           \
    __global__ void __launch_bounds__(kPtThreads) PFX##box(E el, const unsigned* order, unsigned n, unsigned depth, unsigned group, E::Acc* acc) {             \
        pt_box_body(el, order, n, depth, group, acc);                                                                                                           \
    }                                                                                                                                                           \
    __global__ void __launch_bounds__(kPtThreads) PFX##sort(E el, const unsigned* order, unsigned n, unsigned depth, unsigned group, unsigned p2,              \
                                                            const E::Acc* acc, float4* nodes, unsigned long long* keys) {                                      \
        pt_sort_body(el, order, n, depth, group, p2, acc, nodes, keys);                                                                                         \
    }                                                                                                                                                           \
    __global__ void __launch_bounds__(kPtThreads) PFX##merge(const unsigned long long* in, unsigned long long* out, unsigned n, unsigned depth, unsigned group, \
                                                             unsigned p) {                                                                                      \
        pt_merge_body(in, out, n, depth, group, p);                                                                                                             \
    }                                                                                                                                                           \
    __global__ void __launch_bounds__(kPtThreads) PFX##permute(const unsigned long long* keys, const unsigned* order_in, unsigned* order_out, unsigned n,      \
                                                               unsigned depth, unsigned group) {                                                                \
        pt_permute_body(keys, order_in, order_out, n, depth, group);                                                                                            \
    }                                                                                                                                                           \
    __global__ void __launch_bounds__(kPtThreads) PFX##finish(E el, const uint3* roots, const unsigned* order_in, unsigned* order_out, float4* nodes,          \
                                                              unsigned p2) {                                                                                    \
        pt_finish_body(el, roots, order_in, order_out, nodes, p2);                                                                                              \
    }                                                                                                                                                           \
    struct PFX##Kernels {                                                                                                                                       \
        static constexpr auto iota = PFX##iota;                                                                                                                 \
        static constexpr auto box = PFX##box;                                                                                                                   \
        static constexpr auto sort = PFX##sort;                                                                                                                 \
        static constexpr auto merge = PFX##merge;                                                                                                               \
        static constexpr auto permute = PFX##permute;                                                                                                           \
        static constexpr auto finish = PFX##finish;                                                                                                             \
    };

// ---- the host driver
// the ranges k_pt_finish takes: the first range on every way down that holds at most `group` elements
inline void pt_finish_roots(unsigned b, unsigned e, unsigned node, unsigned group, std::vector<uint3>* out) {
    const unsigned m = e - b;
    if (m <= group) { out->push_back(make_uint3(b, e, node)); return; }
    const unsigned split = (b + e) / 2u;
    pt_finish_roots(split, e, node + 1u, group, out);
    pt_finish_roots(b, split, node + 1u + pt_node_count(m - m / 2u), group, out);
}
// the scratch of one build: it lives until the caller has synchronised the stream
template <class E>
struct ElementTreeScratch {
    HipBuffer<unsigned> order[2];
    HipBuffer<typename E::Acc> acc;
    HipBuffer<unsigned long long> keys[2];
    HipBuffer<uint3> roots;
    std::vector<uint3> h_roots;
};
// Enqueues the build of the tree over n > 0 checked elements on `st`: nodes [pt_node_count(n)][2]; *order_out = `order` if given, else a scratch array,
// [n] in leaf order once the stream has run.  group is clamped to 4 .. E::kGroup.
template <class K, class E>
int element_tree_run(const E& el, unsigned n, unsigned group, float4* nodes, unsigned* order, hipStream_t st, ElementTreeScratch<E>* s, const unsigned** order_out) {
    using Acc = typename E::Acc;
    group = std::min(std::max(group, 4u), E::kGroup);
    const unsigned blocks = (n + kPtThreads - 1u) / kPtThreads;
    int rcode;
    // ---- the levels that run over the whole array: while the largest range holds more than `group` elements
    unsigned depth_global = 0u;
    for (unsigned cm = n; cm > group; cm = (cm + 1u) / 2u) depth_global++;
    unsigned p2 = 4u;
    while (p2 < group) p2 <<= 1;
    s->h_roots.clear();
    pt_finish_roots(0u, n, 0u, group, &s->h_roots);
    if ((rcode = s->order[0].ensure(n)) != RL_OK || (rcode = s->roots.ensure(s->h_roots.size())) != RL_OK) return rcode;
    if (depth_global > 0u) {
        if ((rcode = s->order[1].ensure(n)) != RL_OK || (rcode = s->keys[0].ensure(n)) != RL_OK || (rcode = s->keys[1].ensure(n)) != RL_OK ||
            (rcode = s->acc.ensure((size_t)6u << depth_global)) != RL_OK) return rcode;
        HIP_OK(hipMemsetAsync(s->acc.get(), 0xff, ((size_t)6u << depth_global) * sizeof(Acc), st));
    }
    HIP_OK(hipMemcpyAsync(s->roots.get(), s->h_roots.data(), s->h_roots.size() * sizeof(uint3), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(K::iota, dim3(blocks), dim3(kPtThreads), 0, st, s->order[0].get(), n);
    unsigned cur = 0u;
    unsigned cm = n;
    for (unsigned depth = 0; depth < depth_global; depth++, cm = (cm + 1u) / 2u) {
        const unsigned chunks = (n + group - 1u) / group;
        unsigned max_runs = (cm + group - 2u) / group + 1u, passes = 0u;      // a range of cm elements touches at most this many chunks
        while ((1u << passes) < max_runs) passes++;
        hipLaunchKernelGGL(K::box, dim3(blocks), dim3(kPtThreads), 0, st, el, s->order[cur].get(), n, depth, group, s->acc.get());
        hipLaunchKernelGGL(K::sort, dim3(chunks), dim3(kPtThreads), 0, st, el, s->order[cur].get(), n, depth, group, p2, s->acc.get(), nodes, s->keys[0].get());
        unsigned kc = 0u;
        for (unsigned p = 0; p < passes; p++, kc ^= 1u)
            hipLaunchKernelGGL(K::merge, dim3(blocks), dim3(kPtThreads), 0, st, s->keys[kc].get(), s->keys[kc ^ 1u].get(), n, depth, group, p);
        hipLaunchKernelGGL(K::permute, dim3(blocks), dim3(kPtThreads), 0, st, s->keys[kc].get(), s->order[cur].get(), s->order[cur ^ 1u].get(), n, depth, group);
        cur ^= 1u;
    }
    // ---- every range of at most `group` elements: one workgroup each, down to the leaves
    unsigned* out = order ? order : s->order[cur].get();                      // (a workgroup reads its range before it writes it)
    hipLaunchKernelGGL(K::finish, dim3((unsigned)s->h_roots.size()), dim3(kPtThreads), 0, st, el, s->roots.get(), s->order[cur].get(), out, nodes, p2);
    *order_out = out;
    return RL_OK;
}

}  // namespace rl
