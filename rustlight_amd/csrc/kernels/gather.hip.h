// gather.hip.h — the camera-beam gather the volumetric integrators share: the beam radiance estimate (bre.hip.h) and the single-scattering photon planes
// (plane.hip.h) trace one camera ray per sample and add what the elements of a tree — photon spheres, planes — contribute along it.  beam_gather holds
// everything but the element; the integrator supplies that as a leaf object.
//
// Workgroup = one owned block, lane c = ix * bh + iy of it.  A camera sample takes exactly 2 draws (the pixel jitter), so sample (ix, iy, s) of a block
// starts at draw ((ix * bh + iy) * spp + s) * 2 of the block's stream (ix outer, vol_primitives.rs:712-714): a lane enters its pixel's place with one
// rng_advance and walks the pixel's samples in order, which is also the order im_block.accumulate adds them in.
//
// The element tree (host/photontree.h) is stored in the order BHVAccel::gather (accel.rs:545-581) visits it — node, right subtree, left subtree — with a
// skip link per node, so the walk is `i = entered ? i + 1 : skip` and keeps no stack; a leaf hands its elements over in index order, and the contributions
// are added in that order (f32 sums depend on it).  Node: 2 float4 = p_min.xyz, p_max.x | p_max.yz, skip, first << 3 | count (count = 0: inner node).
//
// A leaf type has
//   c                     its constants, a kernel argument; c.nodes and c.n_nodes are the tree
//   kCounters             how many 64-bit walk counters it keeps beyond the nodes entered
//   kLo[], kHi[]          the statistics rows of their low and high parts (launch.h: gather_split24)
//   element(idx, cam, rd, tfar, sc, recs, stack, cs, n)      tests element idx against the ray and adds its contribution to cs, counting in n[0 .. kCounters - 1]
// and is a template argument: the call is inlined, n is indexed by constants only and stays in registers.
#pragma once
#include "rngjump.h"        // rng_advance

namespace rl {

template <int N> struct GatherRows { int v[N]; };
// STAT_SAMPLES, then low and high row of the nodes entered and of each of the leaf's counters
template <class LEAF>
constexpr GatherRows<3 + 2 * LEAF::kCounters> gather_rows() {
    GatherRows<3 + 2 * LEAF::kCounters> r{};
    r.v[0] = STAT_SAMPLES; r.v[1] = STAT_GATHER_NODES; r.v[2] = STAT_GATHER_NODES_HI;
    for (int k = 0; k < LEAF::kCounters; k++) { r.v[3 + 2 * k] = LEAF::kLo[k]; r.v[4 + 2 * k] = LEAF::kHi[k]; }
    return r;
}

template <bool LDS_SCENE, class LEAF>
RL_DEV void beam_gather(const RenderConst& rc, const DeviceScene& sc, const StackConf& stc, float4* smem, const LEAF& leaf) {
    constexpr int K = LEAF::kCounters, N = 3 + 2 * K;
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    const unsigned ob = blockIdx.x, c = threadIdx.x;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[ob], &bx, &by, &bw, &bh);
    const bool active = c < bw * bh;
    unsigned n_samples = 0;
    unsigned long long n_entered = 0, n_leaf[K] = {};       // (a lane may enter more than 2^32 nodes over its samples)
    if (active) {
        Rng rng = rng_seed(rc.block_seeds[rc.owned_blocks[ob]], rc.seed_variant);
        rng_advance<false>(rng, c * rc.spp * 2u);
        const unsigned ix = c / bh, iy = c - (c / bh) * bh;
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        Col sum = czero();
        for (unsigned s = 0; s < rc.spp; s++) {
            n_samples++;
            const float u = (float)(bx + ix) + rng_next_f32(rng);         // Point2::new(ix_c + next(), iy_c + next())
            const float v = (float)(by + iy) + rng_next_f32(rng);
            const V3 rd = camera_direction(sc, u, v);
            Hit hit;
            const float tfar = trace_closest(sc, recs, stack, cam, rd, hit) ? hit.t : kF32Max;     // ray.tfar = max_dist; a miss still gathers
            const V3 inv_d = mk3(div_rn(1.0f, rd.x), div_rn(1.0f, rd.y), div_rn(1.0f, rd.z));
            Col cs = czero();
            unsigned i = 0u;
            while (i < leaf.c.n_nodes) {
                const float4 a = leaf.c.nodes[2u * i], b = leaf.c.nodes[2u * i + 1u];
                float te;
                if (!slab(mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), cam, inv_d, kEps, tfar, &te)) { i = __float_as_uint(b.z); continue; }
                n_entered++;
                const unsigned fc = __float_as_uint(b.w), first = fc >> 3, count = fc & 7u;
                for (unsigned k = 0; k < count; k++) leaf.element(first + k, cam, rd, tfar, sc, recs, stack, cs, n_leaf);
                i++;
            }
            sum = sum + cs;                                                 // im_block.accumulate, in sample order
        }
        const Col px = scale_unguarded(sum, rc.inv_spp);                    // im_block.scale(1 / spp)
        const size_t pix = (size_t)(by + iy) * rc.W + (bx + ix);
        rc.out[3 * pix] = px.r; rc.out[3 * pix + 1] = px.g; rc.out[3 * pix + 2] = px.b;
    }
    {
        // extension rays and draws follow from the samples on the host
        static constexpr GatherRows<N> rows = gather_rows<LEAF>();
        unsigned vals[N];
        vals[0] = n_samples;
        gather_split24(n_entered, &vals[1], &vals[2]);
#pragma unroll
        for (int k = 0; k < K; k++) gather_split24(n_leaf[k], &vals[3 + 2 * k], &vals[4 + 2 * k]);
        block_stats<N>(rc.partials, rows.v, vals);
    }
}

}  // namespace rl
