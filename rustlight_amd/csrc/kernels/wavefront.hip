// wavefront.hip — the gfx950 wavefront path tracer behind `IntegratorPathTracing::compute`
// (src/integrators/explicit/path.rs:186-238 -> compute_mc, src/integrators/mod.rs:403-450).
//
// One path "slot" per GPU lane; all per-path state lives in HBM as structure-of-arrays so that
// lane i of every kernel touches element i of every array (fully coalesced, 4/8-byte words).
// A slot owns one work item — a pixel (throughput stream mode) or a whole 16x16 block
// (reference-order stream mode) — and regenerates a fresh camera sample in place when its path
// ends, so every slot carries exactly one extension ray per iteration until its item is done.
//
// Per iteration (one HIP launch each, same stream):
//   k_raygen   persistent threads: finished samples are folded into the pixel accumulator in
//              sample order, the next (pixel, sample) is seeded and its camera ray generated
//              (Path::from_sensor + Camera::generate; paths/path.rs:56-73, camera.rs:81-91)
//   k_extend   BVH2 closest-hit traversal (Acceleration::trace; accel.rs:292-315)
//   k_shade<M> per-BSDF kernels: medium distance sampling, fill_intersection, emission + MIS of
//              the arriving edge, BSDF / phase sampling, Russian roulette, NEE light sampling with
//              its MIS weight (strategies/directional.rs, strategies/emitters.rs, path.rs:37-111)
//   k_shadow   any-hit traversal for the NEE shadow rays (Acceleration::visible; accel.rs:316-343),
//              adds the pre-weighted contribution to the path's radiance
// (k_shade_sorted when the scene mixes BSDF types: block-local stream compaction + material sort with
// wave64 ballot + prefix popcounts, then one packed pass per BSDF).  Radiance is accumulated front-to-back (DESIGN.md §Radiance order).
// k_path_fused runs the same four stages back to back in one persistent launch with the state in registers / LDS — the form every
// per-sample render takes by default (BSDF code specialised for single-BSDF scenes, a run-time switch otherwise);
// k_pixel_mc is the `ao` / `direct` form.  This file holds the kernels and the host driver behind the C-ABI
// (rl_context_*, rl_render_path / _ao / _direct, rl_trace_batch, rl_visible_batch; path_render.hip.h and gather_render.hip.h hold the host drivers of
// rl_render_path and of the two camera-beam gathers); the device code it instantiates is in
//   pathstate.hip.h  pool layout, state accessors, block-local statistics / compaction
//   stages.hip.h     raygen_slot, extend_slot, shade_slot, shadow_slot
//   mc.hip.h         ao / direct pixel estimators
//   trace.hip.h      BVH2 traversal;   shading.hip.h  BSDFs, emitters, light tree, medium;   devmath.hip.h  f32 contract, RNG
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "common.hip.h"
#include "rngjump.h"
#include "../host/hip_buffer.h"
#include "../host/photontree.h"
#include "../host/beamtree.h"
#include "phototree.h"
#include "../host/scene.h"
#include "wavefront.h"
#include "knobs.h"
#include "light.hip.h"     // STAT_SPLATS*: the statistics slots of k_light_fused (the kernel itself is instantiated by light_*.hip)

namespace rl {

// ------------------------------------------------------------------------------------------
// per-sample stream mode: fork the block sampler once per pixel in the block's (iy, ix) loop order
// with the reference's own clone_box rule (samplers/independent.rs:18-22)
__global__ void k_seed_pixels(RenderConst rc) {
    unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rc.n_owned) return;
    unsigned b = rc.owned_blocks[j];
    unsigned bx, by, bw, bh;
    block_geometry(rc, b, &bx, &by, &bw, &bh);
    Rng rng = rng_seed(rc.block_seeds[b], rc.seed_variant);
    unsigned base = rc.block_item_base[j];
    for (unsigned iy = 0; iy < bh; iy++)
        for (unsigned ix = 0; ix < bw; ix++) {
            unsigned k = base + iy * bw + ix;
            rc.item_seed[k] = rng_next_u64(rng);
            rc.item_pixel[k] = (by + iy) * rc.W + (bx + ix);
        }
}

// reference-order streams in two passes: pixel of every work item of the chunk (block cursors [cursor_begin, cursor_end) of each owned block)
__global__ void k_chunk_pixels(RenderConst rc) {
    unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rc.n_owned) return;
    unsigned bx, by, bw, bh;
    block_geometry(rc, rc.owned_blocks[j], &bx, &by, &bw, &bh);
    const unsigned c_end = min(rc.cursor_end, bw * bh), base = rc.block_item_base[j];
    for (unsigned c = rc.cursor_begin; c < c_end; c++) rc.item_pixel[base + (c - rc.cursor_begin)] = (by + c / bw) * rc.W + (bx + c % bw);
}

__global__ void k_init(RenderConst rc, Pool pool) {
    unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= pool.P) return;
    PoolState ps{pool, slot};
    PU(U_ITEM) = slot;
    PU(U_CURSOR) = 0u;
    PU(U_SAMPLE) = 0u;
    PU(U_DEPTH) = 0u;
    PU(U_PRIM) = 0xffffffffu;
    PU(U_FLAGS) = slot < rc.n_items ? (ST_REGEN | ST_FRESH) : ST_FINISHED;
    storec(ps, F_AR, czero());
    storec(ps, F_LR, czero());
}

// k_raygen — persistent threads (grid-stride loop over the pool).
__global__ void __launch_bounds__(256) k_raygen(RenderConst rc, DeviceScene sc, Pool pool) {
    unsigned n_samples = 0, n_draws = 0;
    for (unsigned slot = blockIdx.x * blockDim.x + threadIdx.x; slot < pool.P; slot += gridDim.x * blockDim.x) {
        PoolState ps{pool, slot};
        raygen_slot<true>(rc, sc, ps, n_samples, n_draws);
    }
    { const int which[2] = {STAT_SAMPLES, STAT_DRAWS}; const unsigned vals[2] = {n_samples, n_draws}; block_stats<2>(rc.partials, which, vals); }
}

// k_fold_samples — sample-parallel pixels (split > 1): add the parked per-sample radiances of each pixel in sample
// order and scale by 1 / spp, i.e. exactly the accumulate / scale sequence of compute_mc (mod.rs:431-436).
__global__ void __launch_bounds__(256) k_fold_samples(RenderConst rc) {
    const bool tail = rc.tail_lanes != 0u;       // only the tail's pixels were parked (RenderConst::tail_*): [spp][tail pixel][3]
    const unsigned n_pix = tail ? rc.tail_pixels : rc.n_items / rc.split;
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    Col acc = czero();
    for (unsigned s = 0; s < rc.spp; s++) {
        const float* src = rc.sample_buf + 3 * ((size_t)s * n_pix + p);
        acc = acc + mkc(src[0], src[1], src[2]);
    }
    const Col px = scale_unguarded(acc, rc.inv_spp);
    const size_t pix = rc.item_pixel[tail ? rc.tail_begin + p : p];
    rc.out[3 * pix] = px.r; rc.out[3 * pix + 1] = px.g; rc.out[3 * pix + 2] = px.b;
}

#ifdef RL_TRAV_STATS
// dev-only: traversal statistics of k_extend, totals over the render: [0] rays, [1] node steps, [2] triangle tests,
// [3] sum over waves of 64 * (max node steps in the wave) = what the wave pays, [4] waves, [5] rays with zero steps
__device__ unsigned long long g_trav_stats[8];
#endif
// k_extend / k_shadow — traversal kernels.  Dynamic LDS = [staged scene][compaction list][per-lane stacks].
template <bool LDS_SCENE, bool SHADOW>
RL_DEV void trace_kernel_body(const DeviceScene& sc, const Pool& pool, const StackConf& stc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    float4* after_scene = LDS_SCENE ? smem + lds_scene_float4s(sc.n_nodes, sc.n_prims) : smem;
    unsigned* list = reinterpret_cast<unsigned*>(after_scene);
    unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = make_stack<LDS_SCENE>(stc, list + 272, slot);
    const unsigned flags = slot < pool.P ? pool.u[(size_t)U_FLAGS * pool.P + slot] : 0u;
    const unsigned n_live = block_compact((flags & (SHADOW ? ST_SHADOW : ST_RAY)) != 0u, slot, list);
    if (n_live == 0u) return;          // whole tile idle (finished pixels): skip the scene staging too
    SceneRecs recs;
    if (LDS_SCENE) {
        stage_scene_lds(sc, smem, smem + lds_nodes_float4s(sc.n_nodes));
        recs.nodes = smem; recs.tris = smem + lds_nodes_float4s(sc.n_nodes);
    } else {
        recs.nodes = streamed_nodes<TravStackT<false>>(sc);
        recs.tris = reinterpret_cast<const float4*>(sc.tris);
    }
#ifdef RL_TRAV_STATS
    int dbg[2] = {-1, 0};
    if (threadIdx.x < n_live) {
        PoolState ps{pool, list[threadIdx.x]};
        if (SHADOW) shadow_slot(sc, recs, stack, ps);
        else extend_slot(sc, recs, stack, ps, dbg);
    }
    if (!SHADOW) {
        int mx = dbg[0];
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off, 64));
        if (dbg[0] >= 0) { atomicAdd(&g_trav_stats[0], 1ull); atomicAdd(&g_trav_stats[1], (unsigned long long)dbg[0]); atomicAdd(&g_trav_stats[2], (unsigned long long)dbg[1]); if (dbg[0] == 0) atomicAdd(&g_trav_stats[5], 1ull); }
        if ((threadIdx.x & 63u) == 0u && mx >= 0) { atomicAdd(&g_trav_stats[3], 64ull * (unsigned long long)mx); atomicAdd(&g_trav_stats[4], 1ull); }
    }
#else
    if (threadIdx.x < n_live) {
        PoolState ps{pool, list[threadIdx.x]};
        if (SHADOW) shadow_slot(sc, recs, stack, ps);
        else extend_slot(sc, recs, stack, ps);
    }
#endif
}

template <bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_extend(RenderConst rc, DeviceScene sc, Pool pool, StackConf stc) { trace_kernel_body<LDS_SCENE, false>(sc, pool, stc); }
template <bool LDS_SCENE>
__global__ void __launch_bounds__(256) k_shadow(RenderConst rc, DeviceScene sc, Pool pool, StackConf stc) { trace_kernel_body<LDS_SCENE, true>(sc, pool, stc); }

// ------------------------------------------------------------------------------------------
// operator-level kernels: batched Acceleration::trace / visible for the parity tests
__global__ void __launch_bounds__(256) k_trace_batch(DeviceScene sc, StackConf stc, unsigned n, const float* o, const float* d, float* t_out, float* u_out,
                                                     float* v_out, int* mesh_out, int* tri_out) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    recs.nodes = streamed_nodes<TravStackT<false>>(sc);
    recs.tris = reinterpret_cast<const float4*>(sc.tris);
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStack stack = make_stack(stc, reinterpret_cast<unsigned*>(smem), i);
    if (i >= n) return;
    V3 ro = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    Hit hit;
    trace_closest(sc, recs, stack, ro, rd, hit);
    t_out[i] = hit.t; u_out[i] = hit.u; v_out[i] = hit.v;
    if (hit.prim >= 0) { mesh_out[i] = sc.tris[hit.prim].mesh; tri_out[i] = sc.tris[hit.prim].tri; }
    else { mesh_out[i] = -1; tri_out[i] = -1; }
}

// test hook: the same batch through the two-level records (trace.hip.h: traverse2), whatever the build traverses by default
__global__ void __launch_bounds__(256) k_trace_batch_two_level(DeviceScene sc, StackConf stc, unsigned n, const float* o, const float* d, float* t_out, float* u_out,
                                                               float* v_out, int* mesh_out, int* tri_out, int* steps_out, int any_hit) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    recs.nodes = reinterpret_cast<const float4*>(sc.nodes2);
    recs.tris = reinterpret_cast<const float4*>(sc.tris);
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStack2 stack(make_stack(stc, reinterpret_cast<unsigned*>(smem), i));
    if (i >= n) return;
    V3 ro = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    Hit hit; hit.t = kF32Max; hit.u = 0.0f; hit.v = 0.0f; hit.prim = -1;
    if (any_hit) {   // t_out in: the segment length (not trace_none's whole ray)
        hit.t = t_out[i];
        const bool f = traverse<true>(recs, sc.root, mk3(sc.root_min[0], sc.root_min[1], sc.root_min[2]), mk3(sc.root_max[0], sc.root_max[1], sc.root_max[2]), ro, rd, kEps, hit.t, hit, stack);
        t_out[i] = f ? 1.0f : 0.0f; steps_out[i] = hit.steps;
        return;
    }
    trace_closest(sc, recs, stack, ro, rd, hit);
    t_out[i] = hit.t; u_out[i] = hit.u; v_out[i] = hit.v; steps_out[i] = hit.steps;
    if (hit.prim >= 0) { mesh_out[i] = sc.tris[hit.prim].mesh; tri_out[i] = sc.tris[hit.prim].tri; }
    else { mesh_out[i] = -1; tri_out[i] = -1; }
}

__global__ void __launch_bounds__(256) k_visible_batch(DeviceScene sc, StackConf stc, unsigned n, const float* p0a, const float* p1a, unsigned char* out) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    recs.nodes = streamed_nodes<TravStackT<false>>(sc);
    recs.tris = reinterpret_cast<const float4*>(sc.tris);
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStack stack = make_stack(stc, reinterpret_cast<unsigned*>(smem), i);
    if (i >= n) return;
    V3 p0 = mk3(p0a[3 * i], p0a[3 * i + 1], p0a[3 * i + 2]), p1 = mk3(p1a[3 * i], p1a[3 * i + 1], p1a[3 * i + 2]);
    out[i] = shadow_visible(sc, recs, stack, p0, p1) ? 1 : 0;
}

// test hook: batched Acceleration::visible on a scene staged in LDS — the per-lane any-hit loop (packed = 0) or the wave's packed form (occluded_packed: every lane of
// the workgroup stays to the end, lanes past the batch hold no segment)
__global__ void __launch_bounds__(256) k_visible_batch_lds(DeviceScene sc, StackConf stc, unsigned n, const float* p0a, const float* p1a, unsigned char* out, int packed) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<true> stack = open_scene<true>(sc, stc, smem, i, &recs);
    const bool has = i < n;
    const unsigned j = has ? i : 0u;
    const V3 p0 = mk3(p0a[3 * j], p0a[3 * j + 1], p0a[3 * j + 2]), p1 = mk3(p1a[3 * j], p1a[3 * j + 1], p1a[3 * j + 2]);
    bool vis = false;
    if (packed) vis = shadow_visible<true>(sc, recs, stack, p0, p1, has, stc.pack_cap);
    else if (has) vis = shadow_visible(sc, recs, stack, p0, p1);
    if (has) out[i] = vis ? 1 : 0;
}

// device self-test of the numerics contract: IEEE divide / sqrt, denormals, no contraction
__global__ void k_numerics_probe(unsigned n, const float* a, const float* b, float* out_div, float* out_sqrt, float* out_mad, float* out_sin,
                                 float* out_cos, float* out_exp, float* out_log, float* out_pow, float* out_acos, float* out_atan2) {
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_div[i] = div_rn(a[i], b[i]);
    out_sqrt[i] = sqrt_rn(fabsf(a[i]));
    out_mad[i] = a[i] * b[i] + a[i];
    out_sin[i] = dm::sinf_det(a[i]);
    out_cos[i] = dm::cosf_det(a[i]);
    out_exp[i] = dm::expf_det(a[i]);
    out_log[i] = dm::logf_det(fabsf(a[i]));
    out_pow[i] = dm::powf_det(fabsf(a[i]), b[i]);
    out_acos[i] = dm::acosf_det(a[i] * 0.15f);
    out_atan2[i] = dm::atan2f_det(a[i], b[i]);
}

// rl_debug_math_sweep: ONE function of the numerics contract per launch, its swept argument made from bit patterns (nothing is uploaded for it) —
// the functions are the ones the kernels call (dm::*_det, div_rn, sqrt_rn of this exact build); there is no second text of them here
__global__ void k_math_sweep(int fn, int swap, unsigned first_bits, unsigned stride, unsigned period, unsigned n, const float* b, float b_const, float* out) {
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = __uint_as_float(first_bits + (period ? i % period : i) * stride);
    const float c = b ? b[i] : b_const;
    const float x = swap ? c : g, y = swap ? g : c;
    float r;
    switch (fn) {
        case RL_MATH_SINF: r = dm::sinf_det(x); break;
        case RL_MATH_COSF: r = dm::cosf_det(x); break;
        case RL_MATH_EXPF: r = dm::expf_det(x); break;
        case RL_MATH_LOGF: r = dm::logf_det(x); break;
        case RL_MATH_POWF: r = dm::powf_det(x, y); break;
        case RL_MATH_ACOSF: r = dm::acosf_det(x); break;
        case RL_MATH_ATAN2F: r = dm::atan2f_det(x, y); break;
        case RL_MATH_ASINF: r = dm::asinf_det(x); break;
        case RL_MATH_SQRT_RN: r = sqrt_rn(x); break;
        case RL_MATH_DIV_RN: r = div_rn(x, y); break;
        default: r = x * y + x; break;      // RL_MATH_MUL_ADD: two roundings (k_numerics_probe's out_mad)
    }
    out[i] = r;
}

}  // namespace rl

// ==========================================================================================
// host side
// ==========================================================================================
using namespace rl;

static thread_local std::string g_last_error;
void rl_set_error(const std::string& s) { g_last_error = s; }
extern "C" const char* rl_last_error(void) { return g_last_error.c_str(); }

struct rl_context {
    int device = 0;
    hipStream_t stream = nullptr;
    DeviceScene ds{};
    std::vector<HipBuffer<unsigned char>> allocs;      // the scene's arrays
    uint32_t width = 0, height = 0;
    bool single_bsdf = true;
    int bsdf_type = 0;
    bool lds_scene = false;
    bool area_lights_only = false;   // every emitter is a mesh area light, no light tree: the fused kernel's NEE code is specialised (same results)
    bool has_directional = false;    // a directional light among the emitters (vpl refuses it with a medium)
    bool surface_emitters_only = true;      // every emitter is a mesh (what LightSamplerATS::new asserts; point-normal-ats refuses anything else)
    std::vector<float> ats_angles;          // [light tree node][2] theta_o, theta_e of the host tree's LightBounds; rl_render_point_normal_ats uploads them
    const float* d_ats_angles = nullptr;    // on first use, into one of `allocs`
    size_t scene_lds_bytes = 0;
    size_t lds_limit = 64 * 1024;     // dynamic LDS a workgroup may ask for on this device (hipDeviceAttributeMaxSharedMemoryPerBlock)
    // render scratch (grown on demand)
    HipBuffer<float> pool_f; HipBuffer<unsigned> pool_u; HipBuffer<unsigned long long> pool_q;    // the wavefront pipeline's path-state pool: all three planes or none
    HipBuffer<unsigned> d_owned, d_item_base;
    HipBuffer<unsigned long long> d_block_seeds, d_item_seed;
    HipBuffer<unsigned> d_item_pixel;
    HipBuffer<float> d_out;
    HipBuffer<Counters> d_counters;
    HipBuffer<Counters, Mem::Pinned> h_counters;
    HipBuffer<unsigned long long> d_partials;
    HipBuffer<int> d_overflow;
    HipBuffer<int> d_overflow2;                         // the overlapped evaluation pass's own overflow levels (it runs beside the chain pass, which uses d_overflow)
    HipBuffer<float> d_sample_buf;                      // sample-parallel pixels: [spp][pixel item][3]
    HipBuffer<unsigned long long> d_sample_states;      // reference-order streams, two passes: [spp][chunk pixel][4]; the light tracer's splat image
    HipBuffer<unsigned long long> d_chain_states;       // [owned block][4]
    // k_stream_spec (spec.hip.h): per-lane tracks of the speculative first pass, the trivial-pixel masks and its counters
    HipBuffer<unsigned> d_trk_off;
    HipBuffer<ulonglong2> d_trk_st;
    HipBuffer<unsigned> d_trivial;
    uint64_t trivial_key = ~0ull;         // (shard index, shard count, sensor expanded?) the masks on the device were computed for
    std::vector<unsigned char> heavy_blocks;      // per owned block: it can see the scene (PathRender::plan_tail), for the shard and sensor of heavy_key
    uint64_t heavy_key = ~0ull;
    HipBuffer<unsigned long long> d_spec_stats;
    std::vector<hipEvent_t> events;
    // the evaluation pass overlapped with the chain pass (reference-order streams): its own low-priority stream, the completion queue, ordering events
    static constexpr int kEvalStreams = 4;      // the evaluation launches beside the chain pass go round these (a launch lasts as long as its slowest pixel: several may have to be in flight)
    hipStream_t stream2 = nullptr; hipStream_t eval_streams[kEvalStreams] = {};
    HipBuffer<unsigned> d_queue;                        // device: [0] chain workgroups started, [16 + k] item-claim counter of the k-th evaluation launch, then the block lists
    hipEvent_t ev_chain_done = nullptr;
    HipBuffer<unsigned, Mem::Mapped> h_flags;           // [0] the chain kernel's "every workgroup runs" word, [16 + j] block j's chain is complete
    HipBuffer<unsigned, Mem::Pinned> h_list;            // the block lists of the evaluation launches (staging of the copies to the device)
    unsigned queue_seq = 0;
    BvhBuild bvh_dump;                // kept for rl_debug_bvh and for the two-level records (built on first use)
    Knobs knobs;                      // execution options: the environment as rl_context_create found it, then rl_context_set_option (knobs.h)
    LightConst light_cam{};           // rl_render_light: the camera's inverses and image rectangle (the splat buffers are set per render)
    std::vector<RectLight> rect_lights;      // plane-single: the light meshes as RectangularLightSource, or why they are refused
    int rect_lights_rc = RL_OK;
    std::string rect_lights_err;
};

template <typename T>
static int upload(rl_context* ctx, const std::vector<T>& v, const T** out) {
    *out = nullptr;
    ctx->allocs.emplace_back();
    HipBuffer<unsigned char>& b = ctx->allocs.back();
    int rcode;
    if ((rcode = b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T))) != RL_OK) return rcode;
    if (!v.empty()) HIP_OK(hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const T*>(b.get());
    return RL_OK;
}

// BvhNode2 records of the context's BVH, built and uploaded on first use
static int ensure_two_level(rl_context* ctx) {
    if (ctx->ds.nodes2) return RL_OK;
    std::vector<BvhNode2> n2;
    two_level_nodes(ctx->bvh_dump, &n2);
    return upload(ctx, n2, &ctx->ds.nodes2);
}

extern "C" int rl_device_count(int* count) {
    if (!count) return RL_ERR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { *count = 0; return RL_ERR_NO_DEVICE; }
    *count = n;
    return RL_OK;
}

extern "C" int rl_context_create(const rl_scene* scene, int device, rl_context** out) {
    if (!scene || !out) return RL_ERR_INVALID_ARGUMENT;
    if (!scene->has_camera) return RL_ERR_INVALID_ARGUMENT;
    if (!scene->emitters_built) return RL_ERR_NOT_BUILT;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        rl_set_error("no HIP device available (hipGetDeviceCount); the MI355X path has no CPU fallback");
        return RL_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n_dev) { rl_set_error("device ordinal out of range"); return RL_ERR_NO_DEVICE; }
    HIP_OK(hipSetDevice(device));
    rl_context* ctx = new rl_context();
    ctx->device = device;
    ctx->width = scene->width; ctx->height = scene->height;
    ctx->knobs.from_environment();       // the ONLY look at the environment: renders read the context's table (knobs.h)
    int rc = RL_OK;
    do {
        {   // the context's stream takes the highest priority the device offers, the overlapped evaluation pass's the lowest: where both have workgroups to place, the chain pass goes first
            int prio_least = 0, prio_greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = prio_greatest = 0; }
            if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) { rl_set_error("hipStreamCreate failed"); rc = RL_ERR_HIP; break; }
            if (hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_least) != hipSuccess) { (void)hipGetLastError(); ctx->stream2 = nullptr; }      // (no second stream: no overlap)
            if (ctx->stream2 && hipEventCreateWithFlags(&ctx->ev_chain_done, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); hipStreamDestroy(ctx->stream2); ctx->stream2 = nullptr; }
            if (ctx->stream2) {
                ctx->eval_streams[0] = ctx->stream2;
                for (int k = 1; k < rl_context::kEvalStreams; k++)
                    if (hipStreamCreateWithPriority(&ctx->eval_streams[k], hipStreamNonBlocking, prio_least) != hipSuccess) { (void)hipGetLastError(); ctx->eval_streams[k] = ctx->stream2; }      // (fewer streams: launches share them)
            }
        }
        BvhBuild& bvh = ctx->bvh_dump;
        build_bvh(*scene, &bvh);                  // BVHAccel::new — untimed (mod.rs:280)
        FlatScene flat;
        flatten_scene(*scene, &flat);
        DeviceScene& ds = ctx->ds;
        if ((rc = upload(ctx, bvh.nodes, &ds.nodes)) != RL_OK) break;
        if ((rc = upload(ctx, bvh.tris, &ds.tris)) != RL_OK) break;
        for (int i = 0; i < 3; i++) { ds.root_min[i] = bvh.root_min[i]; ds.root_max[i] = bvh.root_max[i]; }
        ds.root = bvh.root;
        ds.n_nodes = (uint32_t)bvh.nodes.size();
        ds.n_prims = (uint32_t)bvh.tris.size();
        ds.stack_depth = bvh.stack_depth;
        ds.nodes4 = nullptr; ds.root4 = RL_CHILD_NONE; ds.stack_depth4 = 0;
        ds.nodes_t = nullptr; ds.root_t = RL_CHILD_NONE;
        ds.nodes2 = nullptr;
        // the two-level records (traverse2; 128 B per node, twice the node array) are read only by the test hook rl_debug_trace_batch_two_level, which builds them
        // on its first call
        if ((rc = upload(ctx, flat.tri_indices, &ds.tri_indices)) != RL_OK) break;
        if ((rc = upload(ctx, flat.positions, &ds.positions)) != RL_OK) break;
        if ((rc = upload(ctx, flat.normals, &ds.normals)) != RL_OK) break;
        if ((rc = upload(ctx, flat.uvs, &ds.uvs)) != RL_OK) break;
        // `-x ats`: every emissive mesh learns where its triangles' leaves are listed; the tree itself is uploaded below
        for (MeshRecord& mr : flat.meshes) mr.ats_base = 0xffffffffu;
        std::vector<int32_t> ats_light_mesh;
        if (scene->ats_root >= 0) {
            for (size_t e = 0; e < scene->emitters.size(); e++) flat.meshes[scene->emitters[e].mesh].ats_base = scene->ats_emitter_base[e];
            for (int32_t e : scene->ats_light_emitter) ats_light_mesh.push_back(scene->emitters[e].mesh);
        }
        if ((rc = upload(ctx, flat.meshes, &ds.meshes)) != RL_OK) break;
        ds.ats_root = scene->ats_root;
        if ((rc = upload(ctx, scene->ats_nodes, &ds.ats_nodes)) != RL_OK) break;
        if ((rc = upload(ctx, ats_light_mesh, &ds.ats_light_mesh)) != RL_OK) break;
        if ((rc = upload(ctx, scene->ats_light_prim, &ds.ats_light_prim)) != RL_OK) break;
        if ((rc = upload(ctx, scene->ats_leaf_of, &ds.ats_leaf_of)) != RL_OK) break;
        if ((rc = upload(ctx, flat.materials, &ds.materials)) != RL_OK) break;
        if ((rc = upload(ctx, flat.bitmaps, &ds.bitmaps)) != RL_OK) break;
        if ((rc = upload(ctx, flat.bitmap_texels, &ds.bitmap_texels)) != RL_OK) break;
        if ((rc = upload(ctx, scene->emitters, &ds.emitters)) != RL_OK) break;
        if ((rc = upload(ctx, scene->emitters_cdf, &ds.emitters_cdf)) != RL_OK) break;
        ds.n_emitters = (uint32_t)scene->emitters.size();
        ds.env_emitter = -1;
        for (size_t e = 0; e < scene->emitters.size(); e++)
            if (scene->emitters[e].kind == EMITTER_ENV) {
                ds.env_emitter = (int32_t)e;
                for (int k = 0; k < 3; k++) ds.env_color[k] = scene->emitters[e].c[k];
                // EnvironmentLight::direct_pdf = SolidAngle(1 / (4 pi)) * EmitterSampler::pdf(env)
                ds.env_pdf = (1.0f / (3.14159265358979323846f * 4.0f)) * (scene->emitters_cdf[e + 1] - scene->emitters_cdf[e]);
                ds.env_sel_pdf = scene->emitters_cdf[e + 1] - scene->emitters_cdf[e];
            }
        ds.env_w = ds.env_h = 0;
        if (ds.env_emitter >= 0 && scene->env_map.w) {
            ds.env_w = scene->env_map.w; ds.env_h = scene->env_map.h;
            ds.env_marg_func_int = scene->env_marg_func_int;
            if ((rc = upload(ctx, scene->env_map.rgb, &ds.env_texels)) != RL_OK) break;
            if ((rc = upload(ctx, scene->env_cond_cdf, &ds.env_cond_cdf)) != RL_OK) break;
            if ((rc = upload(ctx, scene->env_cond_func, &ds.env_cond_func)) != RL_OK) break;
            if ((rc = upload(ctx, scene->env_marg_cdf, &ds.env_marg_cdf)) != RL_OK) break;
        }
        if (ds.env_emitter >= 0 && scene->medium.enabled) { rl_set_error("an environment emitter cannot be combined with a medium (paths/edge.rs:94)"); rc = RL_ERR_UNSUPPORTED; break; }
        if ((rc = upload(ctx, flat.mesh_cdf, &ds.mesh_cdf)) != RL_OK) break;
        ds.n_meshes = (uint32_t)flat.meshes.size();
        scene->sample_to_camera.to_cols(ds.camera.sample_to_camera);
        scene->to_world.to_cols(ds.camera.to_world);
        ds.camera.position[0] = scene->cam_pos.x; ds.camera.position[1] = scene->cam_pos.y; ds.camera.position[2] = scene->cam_pos.z;
        ds.camera.width = scene->width; ds.camera.height = scene->height;
        {   // Camera::new's image rectangle in sample space (camera.rs:54-58), for the light tracer
            scene->camera_to_sample.to_cols(ctx->light_cam.camera_to_sample);
            scene->to_local.to_cols(ctx->light_cam.to_local);
            const Vec3 p0 = scene->sample_to_camera.xform_point({0.0f, 0.0f, 0.0f}), p1 = scene->sample_to_camera.xform_point({1.0f, 1.0f, 0.0f});
            const float zmin = std::fmin(p0.z, p1.z), zmax = std::fmax(p0.z, p1.z);
            ctx->light_cam.rect_min[0] = std::fmin(p0.x, p1.x) / zmin; ctx->light_cam.rect_min[1] = std::fmin(p0.y, p1.y) / zmin;
            ctx->light_cam.rect_max[0] = std::fmax(p0.x, p1.x) / zmax; ctx->light_cam.rect_max[1] = std::fmax(p0.y, p1.y) / zmax;
        }
        ds.medium = scene->medium;
        {
            const char* why = "";
            if ((ctx->rect_lights_rc = build_rect_lights(*scene, &ctx->rect_lights, &why)) != RL_OK) ctx->rect_lights_err = why;
        }
        ctx->area_lights_only = scene->ats_root < 0 && !ctx->knobs.has(K_GENERIC_LIGHTS);
        for (const EmitterRecord& e : scene->emitters) if (e.kind != EMITTER_MESH) ctx->area_lights_only = false;
        for (const EmitterRecord& e : scene->emitters) if (e.kind == EMITTER_DIRECTIONAL) ctx->has_directional = true;
        for (const EmitterRecord& e : scene->emitters) if (e.kind != EMITTER_MESH) ctx->surface_emitters_only = false;
        ctx->ats_angles = scene->ats_angles;
        for (const HostMesh& hm : scene->meshes) if (hm.is_light && hm.emission_type != RL_EMISSION_COLOR) ctx->area_lights_only = false;      // uv-dependent emission (`-x hvs-light | texture-light`): the generic instantiation
        ctx->single_bsdf = true;
        ctx->bsdf_type = flat.materials.empty() ? 0 : flat.materials[0].type;
        for (const Material& m : flat.materials) if (m.type != ctx->bsdf_type) ctx->single_bsdf = false;
        // stage the scene in LDS when nodes + triangles are small (<= 48 KiB leaves room for the stacks)
        ctx->scene_lds_bytes = (size_t)16 * lds_scene_float4s(ds.n_nodes, ds.n_prims);     // padded LDS layout (trace.hip.h)
        // LDS-staged scenes also keep their whole traversal stack in LDS (TravStackT<true>)
        ctx->lds_scene = ctx->scene_lds_bytes <= 48 * 1024 && ds.stack_depth <= (uint32_t)kLdsStackLevels;
        {   // worst-case dynamic LDS of any kernel that stages the scene: [scene][compaction list | cold path state][12 stack levels];
            // it must fit what a workgroup may ask for on this device, else the scene streams from L2 / HBM instead
            int lds_limit = 64 * 1024;
            if (hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) { (void)hipGetLastError(); lds_limit = 64 * 1024; }
            ctx->lds_limit = (size_t)std::max(lds_limit, 16 * 1024);
            const size_t worst = ctx->scene_lds_bytes + std::max<size_t>(272 * sizeof(unsigned), kFusedColdBytes) + (size_t)2 * kLdsStackLevels * 256 * sizeof(int);
            if (worst > (size_t)lds_limit) ctx->lds_scene = false;
        }
        if (ctx->knobs.has(K_FORCE_STREAMING)) ctx->lds_scene = false;     // dev / test knob: small scenes through the kernels that stream the BVH (tests/parity_fuzz.py)
        if (!ctx->lds_scene) {
            // scenes that stream their BVH: the tolerance build (`numerics = fast`) traverses the same tree collapsed into quantised BVH4 nodes
            Bvh4Build b4;
            build_bvh4(bvh, &b4);
            if ((rc = upload(ctx, b4.nodes, &ds.nodes4)) != RL_OK) break;
            ds.root4 = b4.root; ds.stack_depth4 = b4.stack_depth;
            // ... and the draw-count pass of reference-order streams reads the exact BVH2 through a copy laid out in 16-node treelet blocks (traverse_treelet)
            std::vector<BvhNode> blocks;
            int32_t root_t = RL_CHILD_NONE;
            treelet_blocks(bvh, &blocks, &root_t);
            if ((rc = upload(ctx, blocks, &ds.nodes_t)) != RL_OK) break;
            ds.root_t = root_t;
        }
        if (ctx->d_counters.ensure(1) != RL_OK) { rl_set_error("hipMalloc counters"); rc = RL_ERR_HIP; break; }
        if (ctx->h_counters.ensure(1) != RL_OK) { rl_set_error("hipHostMalloc counters"); rc = RL_ERR_HIP; break; }
    } while (0);
    if (rc != RL_OK) { rl_context_destroy(ctx); return rc; }
    *out = ctx;
    return RL_OK;
}

extern "C" void rl_context_destroy(rl_context* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);        // (the buffers are freed by `delete ctx`, on this device)
    for (hipEvent_t ev : ctx->events) hipEventDestroy(ev);
    if (ctx->ev_chain_done) hipEventDestroy(ctx->ev_chain_done);
    for (int k = 1; k < rl_context::kEvalStreams; k++) if (ctx->eval_streams[k] && ctx->eval_streams[k] != ctx->stream2) hipStreamDestroy(ctx->eval_streams[k]);
    if (ctx->stream2) hipStreamDestroy(ctx->stream2);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

// Scenes that stream their BVH keep only kLdsStackLevelsStreaming levels in LDS: their pools are sparse (most waves of a
// workgroup exit after the compaction), so what limits the live waves per CU is how many workgroups' stacks fit in LDS —
// 508 k-triangle scene, 32 spp: 12 / 8 / 6 / 4 / 2 / 0 levels in LDS = 258 / 233 / 228 / 229 / 240 / 251 ms.
#ifndef RL_LDS_LEVELS_STREAMING
#define RL_LDS_LEVELS_STREAMING 6
#endif
static constexpr int kLdsStackLevelsStreaming = RL_LDS_LEVELS_STREAMING;
static int lds_levels_of(const rl_context* ctx) { return std::min<int>((int)ctx->ds.stack_depth, ctx->lds_scene ? kLdsStackLevels : kLdsStackLevelsStreaming); }
static size_t traversal_lds_bytes(const rl_context* ctx, bool lds_scene, unsigned block, bool with_list, int lds_levels = -1) {
    size_t stack = (size_t)2 * (lds_levels >= 0 ? lds_levels : lds_levels_of(ctx)) * block * sizeof(int);
    return (lds_scene ? ctx->scene_lds_bytes : 0) + (with_list ? 272 * sizeof(unsigned) : 0) + stack;   // [scene][compaction list][stacks]
}
// overflow levels beyond the LDS part, [2 * levels][n_threads] ints
static int stack_conf(rl_context* ctx, size_t n_threads, StackConf* out, bool second = false, int lds_levels = -1) {
    HipBuffer<int>& d_overflow = second ? ctx->d_overflow2 : ctx->d_overflow;
    out->lds_levels = lds_levels >= 0 ? std::min(lds_levels, lds_levels_of(ctx)) : lds_levels_of(ctx);
    out->pre_group = 0;          // only k_stream_chain uses it (its launch code sets it)
    out->pack_cap = 0;           // only k_path_fused's tail form uses it (path_render.hip.h sets it)
    out->overflow = nullptr;
    out->overflow_stride = n_threads;
    int extra = (int)std::max(ctx->ds.stack_depth, ctx->ds.stack_depth4) - out->lds_levels;     // (the tolerance build's BVH4 stacks are the deeper ones)
    if (extra > 0) {
        const int rcode = d_overflow.ensure((size_t)2 * extra * n_threads);
        if (rcode != RL_OK) return rcode;
        out->overflow = d_overflow.get();
    }
    return RL_OK;
}

// block b's pixels: blocks are numbered x-major, nby = ceil(H / 16) to a column (mod.rs:351-374; the kernels' block_geometry)
struct BlockRect { unsigned x, y, w, h; };
static BlockRect block_rect(size_t b, size_t nby, uint32_t W, uint32_t H) {
    const unsigned x = (unsigned)(b / nby) * 16u, y = (unsigned)(b % nby) * 16u;
    return {x, y, std::min(16u, W - x), std::min(16u, H - y)};
}

// ---- k_stream_spec: pixels whose camera samples take exactly two draws (Path::from_sensor's jitter) whatever the stream holds.
// Without a medium a camera ray that misses the scene ends its path at once (path.rs:152-166), and every camera ray of a pixel misses when the
// scene's bounding box lies outside the pyramid spanned by the camera position and the pixel's footprint [ix, ix+1) x [iy, iy+1).  The rays
// through a rectangle of the image plane (Camera::generate is a projective map of the raster position, camera.rs:81-91) fill the convex cone of its four
// corner rays; a box that lies wholly beyond ONE side plane of that cone touches none of them.  Evaluated in f64 on a footprint grown by a quarter
// pixel and a box grown by 1e-3 of its size — orders of magnitude more than the f32 rounding of the device's ray generation and slab / triangle
// tests — so a pixel flagged here cannot produce a hit on the device.  Bit c of words [8 b .. 8 b + 7]: block cursor c of owned block b.
struct TrivialInput { uint32_t W, H; bool medium, empty; float root_min[3], root_max[3]; CameraRecord camera; };
static TrivialInput trivial_input(const rl_context* ctx) {
    TrivialInput in{};
    in.W = ctx->width; in.H = ctx->height; in.medium = ctx->ds.medium.enabled != 0; in.empty = ctx->ds.root == RL_CHILD_NONE || ctx->ds.n_prims == 0;
    for (int k = 0; k < 3; k++) { in.root_min[k] = ctx->ds.root_min[k]; in.root_max[k] = ctx->ds.root_max[k]; }
    in.camera = ctx->ds.camera;
    return in;
}
// blocks_only: only the block-wide test (a block's bits are then all set or all clear)
static void trivial_pixel_masks(const TrivialInput& ti, const rl_path_params* params, const std::vector<unsigned>& owned, size_t nby, bool no_shortcut, std::vector<unsigned>* out, bool blocks_only = false) {
    const uint32_t W = ti.W, H = ti.H;
    out->assign(owned.size() * 8, 0u);
    const bool expand = !params->has_max_depth || 1u < params->max_depth;
    auto all_of_block = [&](size_t j, unsigned npx) { for (unsigned c = 0; c < npx; c++) (*out)[j * 8 + (c >> 5)] |= 1u << (c & 31u); };
    if (!expand) {      // the sensor vertex is never expanded: two draws per sample everywhere
        for (size_t j = 0; j < owned.size(); j++) { const BlockRect r = block_rect(owned[j], nby, W, H); all_of_block(j, r.w * r.h); }
        return;
    }
    if (ti.medium || no_shortcut) return;      // Edge::from_ray samples the medium on a miss too: no shortcut
    const bool empty = ti.empty;
    double lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        lo[k] = ti.root_min[k]; hi[k] = ti.root_max[k];
        if (!empty && !(std::isfinite(lo[k]) && std::isfinite(hi[k]) && lo[k] <= hi[k])) return;      // hostile geometry: no shortcut
        const double grow = 1e-3 * (hi[k] - lo[k]) + 1e-4 * std::max(1.0, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
        lo[k] -= grow; hi[k] += grow;
    }
    const float* m = ti.camera.sample_to_camera; const float* tw = ti.camera.to_world;
    const double cam[3] = {ti.camera.position[0], ti.camera.position[1], ti.camera.position[2]};
    // direction of the ray through raster position (u, v), not normalised; false when the projective map degenerates there
    auto ray_dir = [&](double u, double v, double* d) -> bool {
        const double sx = u / (double)W, sy = v / (double)H;
        const double hx = m[0] * sx + m[4] * sy + m[12], hy = m[1] * sx + m[5] * sy + m[13], hz = m[2] * sx + m[6] * sy + m[14], hw = m[3] * sx + m[7] * sy + m[15];
        if (!(std::fabs(hw) > 1e-12) || !std::isfinite(hx + hy + hz + hw)) return false;
        const double nx = hx / hw, ny = hy / hw, nz = hz / hw;
        d[0] = tw[0] * nx + tw[4] * ny + tw[8] * nz; d[1] = tw[1] * nx + tw[5] * ny + tw[9] * nz; d[2] = tw[2] * nx + tw[6] * ny + tw[10] * nz;
        d[3] = hw;
        const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(len > 1e-30) || !std::isfinite(len)) return false;
        d[0] /= len; d[1] /= len; d[2] /= len;
        return true;
    };
    // true when no ray through the raster rectangle [u0, u1] x [v0, v1] can meet the grown box
    auto misses = [&](double u0, double v0, double u1, double v1) -> bool {
        if (empty) return true;
        double d[4][4];
        const double us[4] = {u0, u1, u1, u0}, vs[4] = {v0, v0, v1, v1};
        for (int k = 0; k < 4; k++) if (!ray_dir(us[k], vs[k], d[k])) return false;
        for (int k = 1; k < 4; k++) if ((d[k][3] > 0) != (d[0][3] > 0)) return false;       // the footprint crosses the map's pole
        for (int k = 0; k < 4; k++) {
            const double* a = d[k]; const double* b = d[(k + 1) & 3]; const double* o = d[(k + 2) & 3];
            double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
            const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(nl > 1e-14)) return false;
            double inside = (n[0] * o[0] + n[1] * o[1] + n[2] * o[2]) / nl;          // the cone lies on the side of the opposite corner
            if (!(std::fabs(inside) > 1e-9)) return false;
            const double sgn = inside > 0 ? 1.0 : -1.0;
            bool all_out = true;
            for (int cbit = 0; cbit < 8 && all_out; cbit++) {
                const double p[3] = {((cbit & 1) ? hi[0] : lo[0]) - cam[0], ((cbit & 2) ? hi[1] : lo[1]) - cam[1], ((cbit & 4) ? hi[2] : lo[2]) - cam[2]};
                const double pl = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                const double s = sgn * (n[0] * p[0] + n[1] * p[1] + n[2] * p[2]) / nl;
                if (!(s < -1e-7 * pl - 1e-12)) all_out = false;
            }
            if (all_out) return true;
        }
        return false;
    };
    for (size_t j = 0; j < owned.size(); j++) {
        const BlockRect r = block_rect(owned[j], nby, W, H);
        const unsigned bx = r.x, by = r.y, bw = r.w, bh = r.h;
        if (misses(bx - 0.25, by - 0.25, bx + bw + 0.25, by + bh + 0.25)) { all_of_block(j, bw * bh); continue; }
        if (blocks_only) continue;
        for (unsigned c = 0; c < bw * bh; c++) {
            const double x = bx + c % bw, y = by + c / bw;
            if (misses(x - 0.25, y - 0.25, x + 1.25, y + 1.25)) (*out)[j * 8 + (c >> 5)] |= 1u << (c & 31u);
        }
    }
}

// test hook, host only (no GPU): the pixels k_stream_spec would treat as taking two draws per sample — out[y * W + x] = 1 — for the scene's camera and the bounding box of
// its BVH (built here as rl_context_create builds it).  tests/test_abi.py checks every flagged pixel against the oracle's camera rays and traversal.
extern "C" int rl_debug_trivial_pixels(const rl_scene* scene, int has_max_depth, uint32_t max_depth, uint8_t* out) {
    if (!scene || !out || !scene->has_camera) return RL_ERR_INVALID_ARGUMENT;
    BvhBuild bvh;
    build_bvh(*scene, &bvh);
    TrivialInput ti{};
    ti.W = scene->width; ti.H = scene->height; ti.medium = scene->medium.enabled != 0; ti.empty = bvh.root == RL_CHILD_NONE || bvh.tris.empty();
    for (int k = 0; k < 3; k++) { ti.root_min[k] = bvh.root_min[k]; ti.root_max[k] = bvh.root_max[k]; }
    scene->sample_to_camera.to_cols(ti.camera.sample_to_camera);
    scene->to_world.to_cols(ti.camera.to_world);
    ti.camera.position[0] = scene->cam_pos.x; ti.camera.position[1] = scene->cam_pos.y; ti.camera.position[2] = scene->cam_pos.z;
    ti.camera.width = scene->width; ti.camera.height = scene->height;
    rl_path_params pp{};
    pp.has_max_depth = has_max_depth; pp.max_depth = max_depth;
    const size_t nbx = (ti.W + 15) / 16, nby = (ti.H + 15) / 16;
    std::vector<unsigned> owned(nbx * nby), masks;
    for (size_t b = 0; b < owned.size(); b++) owned[b] = (unsigned)b;
    trivial_pixel_masks(ti, &pp, owned, nby, false, &masks);
    std::memset(out, 0, (size_t)ti.W * ti.H);
    for (size_t b = 0; b < owned.size(); b++) {
        const BlockRect r = block_rect(b, nby, ti.W, ti.H);
        for (unsigned c = 0; c < r.w * r.h; c++) if ((masks[b * 8 + (c >> 5)] >> (c & 31u)) & 1u) out[(size_t)(r.y + c / r.w) * ti.W + r.x + c % r.w] = 1;
    }
    return RL_OK;
}

// ---- what every render entry point does the same way, one RenderFrame per call: this shard's blocks, the tables, the image and the statistics rows, the
// RenderConst fields they fill alike, the event pool, and the finish (image download, rows summed, the counters every kind reports)
static int check_frame(const rl_context* ctx, uint32_t spp, const uint64_t* block_seeds, size_t n_blocks, const float* out_rgb) {
    if (!ctx || !block_seeds || !out_rgb) return RL_ERR_INVALID_ARGUMENT;
    if (n_blocks != (size_t)((ctx->width + 15) / 16) * ((ctx->height + 15) / 16)) { rl_set_error("n_blocks does not match the image size"); return RL_ERR_INVALID_ARGUMENT; }
    if (spp == 0) { rl_set_error("spp must be > 0 (assert_ne!(scene.nb_samples, 0), mod.rs:410)"); return RL_ERR_INVALID_ARGUMENT; }
    return RL_OK;
}
template <typename Params>
static int check_frame(const rl_context* ctx, const Params* params, const uint64_t* block_seeds, size_t n_blocks, const float* out_rgb) {
    return params ? check_frame(ctx, params->spp, block_seeds, n_blocks, out_rgb) : RL_ERR_INVALID_ARGUMENT;
}
// path, ao and direct: the stream mode, the numerics (ao / direct pass RL_NUMERICS_EXACT) and the shard
static int check_streams(int32_t stream_mode, uint32_t spp, uint32_t numerics, uint32_t shard_index, uint32_t shard_count) {
    if (stream_mode < RL_STREAM_REFERENCE_ORDER || stream_mode > RL_STREAM_STRATIFIED) { rl_set_error("stream_mode must be 0 (reference order), 1 (per sample) or 2 (stratified)"); return RL_ERR_INVALID_ARGUMENT; }
    if (stream_mode == RL_STREAM_STRATIFIED && spp > (1u << 30)) { rl_set_error("the stratified sampler takes at most 2^30 spp"); return RL_ERR_INVALID_ARGUMENT; }
    if (numerics > RL_NUMERICS_FAST) { rl_set_error("numerics must be 0 (exact) or 1 (fast)"); return RL_ERR_INVALID_ARGUMENT; }
    if (shard_index >= (shard_count ? shard_count : 1)) return RL_ERR_INVALID_ARGUMENT;
    return RL_OK;
}

namespace {

struct RenderFrame {
    rl_context* const ctx;
    const uint64_t* const block_seeds;
    const size_t n_blocks;
    float* const out_rgb;
    const int out_is_device;
    const hipStream_t st;
    rl_render_stats* const stats;
    const Knobs knobs;                 // the context's options as they stood when the render started
    const uint32_t W, H;
    const size_t nby;
    const uint32_t shard_count;
    const std::chrono::steady_clock::time_point t_start;
    const bool timing;                 // HIP events around the kernels
    int cus = 256;
    std::vector<unsigned> owned, item_base;      // this shard's blocks in creation order (mod.rs:351-374: `b % shard_count`), their first pixel items
    unsigned n_pixels = 0;
    float* d_out = nullptr;            // the caller's buffer or the context's staging copy
    size_t n_rows = 0;                 // statistics rows
    unsigned long long totals[STAT_COUNT] = {};

    RenderFrame(rl_context* c, const uint64_t* seeds, size_t nb, float* out, int out_dev, void* stream_arg, rl_render_stats* s, uint32_t shard_index, uint32_t n_shards)
        : ctx(c), block_seeds(seeds), n_blocks(nb), out_rgb(out), out_is_device(out_dev), st(stream_arg ? (hipStream_t)stream_arg : c->stream), stats(s),
          knobs(c->knobs), W(c->width), H(c->height), nby((c->height + 15) / 16), shard_count(n_shards ? n_shards : 1), t_start(std::chrono::steady_clock::now()),
          timing(s != nullptr && !knobs.has(K_NO_EVENTS)) {
        for (size_t b = 0; b < n_blocks; b++) {
            if (b % shard_count != shard_index) continue;
            const BlockRect r = block_rect(b, nby, W, H);
            owned.push_back((unsigned)b);
            item_base.push_back(n_pixels);
            n_pixels += r.w * r.h;
        }
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    }

    // the recorded sampler states of reference-order streams may take this many bytes (test knob state_budget_mb: forces several chunks)
    size_t max_state_bytes() const { return knobs.has(K_STATE_BUDGET_MB) ? std::max<size_t>(1, (size_t)knobs.i(K_STATE_BUDGET_MB, 0)) << 20 : (size_t)24 << 30; }

    int alloc_tables() {
        int rcode;
        if ((rcode = ctx->d_owned.ensure(owned.size())) != RL_OK || (rcode = ctx->d_item_base.ensure(owned.size())) != RL_OK ||
            (rcode = ctx->d_block_seeds.ensure(n_blocks)) != RL_OK) return rcode;
        return RL_OK;
    }
    int alloc_output(size_t rows) {
        d_out = out_rgb;
        if (!out_is_device) {
            const int rcode = ctx->d_out.ensure((size_t)3 * W * H);
            if (rcode != RL_OK) return rcode;
            d_out = ctx->d_out.get();
        }
        n_rows = rows;
        return ctx->d_partials.ensure(n_rows * STAT_COUNT);
    }
    int upload(bool with_item_base, bool zero_image) {
        HIP_OK(hipMemcpyAsync(ctx->d_owned.get(), owned.data(), owned.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
        if (with_item_base) HIP_OK(hipMemcpyAsync(ctx->d_item_base.get(), item_base.data(), item_base.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(ctx->d_block_seeds.get(), block_seeds, n_blocks * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (zero_image) HIP_OK(hipMemsetAsync(d_out, 0, (size_t)3 * W * H * sizeof(float), st));
        return RL_OK;
    }
    int zero_rows() {
        HIP_OK(hipMemsetAsync(ctx->d_partials.get(), 0, n_rows * STAT_COUNT * sizeof(unsigned long long), st));
        return RL_OK;
    }
    RenderConst render_const(uint32_t spp, int32_t stream_mode, int32_t seed_variant) const {
        RenderConst rc{};
        rc.spp = spp;
        rc.stream_mode = stream_mode; rc.seed_variant = seed_variant;
        rc.inv_spp = 1.0f / (float)spp;
        rc.W = W; rc.H = H; rc.nby = (unsigned)nby;
        rc.owned_blocks = ctx->d_owned.get(); rc.block_item_base = ctx->d_item_base.get(); rc.n_owned = (unsigned)owned.size();
        rc.block_seeds = ctx->d_block_seeds.get();
        rc.item_seed = ctx->d_item_seed.get(); rc.item_pixel = ctx->d_item_pixel.get();
        rc.out = d_out;
        rc.counters = ctx->d_counters.get();
        rc.partials = ctx->d_partials.get();
        return rc;
    }
    int grow_events(size_t n) {
        if (timing) while (ctx->events.size() < n) { hipEvent_t ev; HIP_OK(hipEventCreate(&ev)); ctx->events.push_back(ev); }
        return RL_OK;
    }
    // the image to the caller and the statistics rows summed into `totals`; with stats: the counters every kind reports and the call's wall time
    int download() {
        if (!out_is_device) HIP_OK(hipMemcpyAsync(out_rgb, d_out, (size_t)3 * W * H * sizeof(float), hipMemcpyDeviceToHost, st));
        std::vector<unsigned long long> partials(n_rows * STAT_COUNT);
        HIP_OK(hipMemcpyAsync(partials.data(), ctx->d_partials.get(), partials.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipGetLastError());
        for (size_t r = 0; r < n_rows; r++) for (int k = 0; k < STAT_COUNT; k++) totals[k] += partials[r * STAT_COUNT + k];
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->camera_samples = totals[STAT_SAMPLES]; stats->vertices = totals[STAT_VERTICES]; stats->extension_rays = totals[STAT_EXT_RAYS];
            stats->shadow_rays = totals[STAT_SHADOW_RAYS]; stats->rng_draws = totals[STAT_DRAWS];
            stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        }
        return RL_OK;
    }
};

// The one-lane generation run of rl_vpl_generate and rl_plane_generate: the sampler's four words go up in front of n_counters zeroed words, launch(d_gen) — the
// kernel reads and leaves its sampler in d_gen[0..4) and counts into d_gen[4..) — runs between the event pair, and the block comes back once the stream is idle.
struct LaneRun {
    std::vector<unsigned long long> words;               // [4] the sampler the lane left (the callers store it once every check has passed), then the counters
    EventPair ev;                                        // ev.ms: the kernel, 0 without timing
    std::chrono::steady_clock::time_point t0;            // just before the launch: the callers' render_ms counts from here
};
template <class Launch>
int run_one_lane(hipStream_t st, bool timing, const rl_sampler* sampler, size_t n_counters, LaneRun* run, Launch&& launch) {
    int rcode;
    HipBuffer<unsigned long long> d_gen;
    if ((rcode = d_gen.ensure(4 + n_counters)) != RL_OK || (rcode = run->ev.open(timing)) != RL_OK) return rcode;
    run->words.assign(4 + n_counters, 0ull);
    for (int i = 0; i < 4; i++) run->words[i] = sampler->s[i];
    HIP_OK(hipMemcpyAsync(d_gen.get(), run->words.data(), run->words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    run->ev.begin(st);
    run->t0 = std::chrono::steady_clock::now();
    launch(d_gen.get());
    run->ev.end(st);
    HIP_OK(hipMemcpyAsync(run->words.data(), d_gen.get(), run->words.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    run->ev.add();
    return RL_OK;
}
}  // namespace

#include "path_render.hip.h"

extern "C" int rl_render_path(rl_context* ctx, const rl_path_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                              int out_is_device, void* stream_arg, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (params->strategy < 0 || params->strategy > 2) return RL_ERR_INVALID_ARGUMENT;
    if ((rcode = check_streams(params->stream_mode, params->spp, params->numerics, params->shard_index, params->shard_count)) != RL_OK) return rcode;
    if (params->strategy != RL_STRATEGY_BSDF && ctx->ds.n_emitters == 0) { rl_set_error("light sampling requested but the scene has no emitter"); return RL_ERR_NO_EMITTER; }
    HIP_OK(hipSetDevice(ctx->device));
    PathRender job(ctx, params, block_seeds, n_blocks, out_rgb, out_is_device, stream_arg, stats);
    return job.run();
}

// Execution options of a context (kernels/knobs.h): `name` as listed there ("spec_force", "no_overlap", "state_budget_mb", ...), `value` its value as text, NULL = back to
// the default.  rl_context_create fills the table from the environment once; nothing below rl_render_path / rl_render_ao / rl_render_direct reads the environment.
// Not to be called while a render runs on the same context (a render works on the copy it took when it started).  The two options that shape the context itself
// (force_streaming, generic_lights) are read when it is created and refused here.
extern "C" int rl_context_set_option(rl_context* ctx, const char* name, const char* value) {
    if (!ctx || !name) return RL_ERR_INVALID_ARGUMENT;
    const int k = Knobs::find(name);
    if (k < 0) { rl_set_error(std::string("unknown option: ") + name); return RL_ERR_INVALID_ARGUMENT; }
    if (k == K_FORCE_STREAMING || k == K_GENERIC_LIGHTS) { rl_set_error(std::string(name) + " is read when the context is created (environment RL_FORCE_STREAMING / RL_GENERIC_LIGHTS)"); return RL_ERR_UNSUPPORTED; }
    ctx->knobs.e[k].set = value != nullptr;
    ctx->knobs.e[k].value = value ? value : "";
    return RL_OK;
}
// the value an option holds (NULL: not set, the default applies); the pointer stays valid until the option is set again
extern "C" const char* rl_context_get_option(const rl_context* ctx, const char* name) {
    if (!ctx) return nullptr;
    const int k = Knobs::find(name);
    return k < 0 ? nullptr : ctx->knobs.str(k);
}

// test hook: rng_advance (rngjump.h) on the device — states_out[i] = the sampler states_in[i] after counts[i] more draws
namespace rl {
__global__ void k_debug_rng_advance(unsigned n, const unsigned long long* in, const unsigned* counts, unsigned long long* out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    Rng r; r.s0 = r.s1 = r.s2 = r.s3 = 0ull;
    if (i < n) { r.s0 = in[4 * i]; r.s1 = in[4 * i + 1]; r.s2 = in[4 * i + 2]; r.s3 = in[4 * i + 3]; }
    rng_advance(r, i < n ? counts[i] : 0u);
    if (i < n) { out[4 * i] = r.s0; out[4 * i + 1] = r.s1; out[4 * i + 2] = r.s2; out[4 * i + 3] = r.s3; }
}
}  // namespace rl
extern "C" int rl_debug_rng_advance(int device, size_t n, const uint64_t* states_in, const uint32_t* counts, uint64_t* states_out) {
    if (!states_in || !counts || !states_out || n == 0 || n > (1u << 24)) return RL_ERR_INVALID_ARGUMENT;
    HIP_OK(hipSetDevice(device));
    HipBuffer<unsigned long long> d_in, d_out; HipBuffer<unsigned> d_c;
    int rcode;
    if ((rcode = d_in.ensure(4 * n)) != RL_OK || (rcode = d_out.ensure(4 * n)) != RL_OK || (rcode = d_c.ensure(n)) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(d_in.get(), states_in, n * 32, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_c.get(), counts, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rl::k_debug_rng_advance, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (unsigned)n, d_in.get(), d_c.get(), d_out.get());
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(states_out, d_out.get(), n * 32, hipMemcpyDeviceToHost));
    return RL_OK;
}

// ---- ao / direct: Integrator::compute through the same tiling driver (one launch)
static int render_mc(rl_context* ctx, int kind, const rl_mc_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                     int out_is_device, void* stream_arg, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if ((rcode = check_streams(params->stream_mode, params->spp, RL_NUMERICS_EXACT, params->shard_index, params->shard_count)) != RL_OK) return rcode;
    if (kind == 1 && params->nb_light_samples > 0 && ctx->ds.n_emitters == 0) { rl_set_error("light sampling requested but the scene has no emitter"); return RL_ERR_NO_EMITTER; }
    HIP_OK(hipSetDevice(ctx->device));
    RenderFrame fr(ctx, block_seeds, n_blocks, out_rgb, out_is_device, stream_arg, stats, params->shard_index, params->shard_count);
    const bool strat = params->stream_mode == RL_STREAM_STRATIFIED;
    const bool per_sample = params->stream_mode == RL_STREAM_PER_SAMPLE || strat;      // (stratified: per-pixel items, the pixel seeds k_seed_pixels writes)
    // reference-order streams in two passes, as for `path` (chain.hip.h): k_mc_chain records where every camera sample starts in its block's stream (a sample's
    // draw count follows from its camera ray alone), then the per-pixel form evaluates all samples from those states.  One chunk: when the states do not fit
    // their budget the single-pass walk (one lane per block) runs instead, as it does under RL_REF_SINGLE_PASS.
    const bool two_pass = !per_sample && !fr.owned.empty() && !fr.knobs.has(K_REF_SINGLE_PASS) && (size_t)fr.n_pixels * params->spp * 32 <= fr.max_state_bytes();
    const bool per_pixel = per_sample || two_pass;
    const unsigned n_items = per_pixel ? fr.n_pixels : (unsigned)fr.owned.size();
    unsigned chain_shift = 0;
    if (two_pass) {
        while (chain_shift < 6u && (fr.owned.size() << (chain_shift + 1u)) <= (size_t)fr.cus * 4u * 256u) chain_shift++;
        if (fr.knobs.has(K_ITEM_SHIFT)) chain_shift = std::min(6u, (unsigned)std::max<long long>(0, fr.knobs.i(K_ITEM_SHIFT, 0)));
    }
    const unsigned chain_threads = two_pass ? std::max(256u, (unsigned)((((size_t)fr.owned.size() << chain_shift) + 255u) / 256u * 256u)) : 0u;
    const unsigned n_threads = std::max(chain_threads, std::max(256u, (n_items + 255u) / 256u * 256u));
    if ((rcode = fr.alloc_tables()) != RL_OK) return rcode;
    if (per_pixel && ((rcode = ctx->d_item_seed.ensure(fr.n_pixels)) != RL_OK || (rcode = ctx->d_item_pixel.ensure(fr.n_pixels)) != RL_OK)) return rcode;
    if (two_pass && (rcode = ctx->d_sample_states.ensure((size_t)fr.n_pixels * params->spp * 4)) != RL_OK) return rcode;
    if ((rcode = fr.alloc_output(n_threads / 256)) != RL_OK) return rcode;
    if ((rcode = fr.upload(true, true)) != RL_OK || (rcode = fr.zero_rows()) != RL_OK) return rcode;
    RenderConst rc = fr.render_const(params->spp, params->stream_mode, params->seed_variant);
    rc.n_items = n_items;
    rc.split = 1;
    rc.sample_states = ctx->d_sample_states.get(); rc.n_state_pixels = fr.n_pixels;
    McConst mp{params->has_max_distance, params->max_distance, params->normal_correction, params->nb_bsdf_samples, params->nb_light_samples};
    StackConf stc;
    if ((rcode = stack_conf(ctx, n_threads, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    const dim3 grid((std::max(256u, (n_items + 255u) / 256u * 256u)) / 256), block(256);
    if ((rcode = fr.grow_events(4)) != RL_OK) return rcode;
    const hipStream_t st = fr.st;
    if (per_pixel && !fr.owned.empty()) hipLaunchKernelGGL(k_seed_pixels, dim3(((unsigned)fr.owned.size() + 63) / 64), dim3(64), 0, st, rc);     // (two-pass: for item_pixel)
    if (two_pass) {
        RenderConst ra = rc;
        ra.n_items = (unsigned)fr.owned.size(); ra.item_shift = chain_shift;
        if (fr.timing) hipEventRecord(ctx->events[0], st);
        launch_mc_chain(kind, ctx->lds_scene, dim3(chain_threads / 256), block, lds, st, ra, ctx->ds, stc, mp);
        if (fr.timing) hipEventRecord(ctx->events[1], st);
        rc.stream_mode = kStreamGivenStates;
    }
    if (fr.timing) hipEventRecord(ctx->events[2], st);
    (strat ? launch_pixel_mc_strat : launch_pixel_mc)(kind, ctx->lds_scene, grid, block, lds, st, rc, ctx->ds, stc, mp);
    if (fr.timing) hipEventRecord(ctx->events[3], st);
    if ((rcode = fr.download()) != RL_OK) return rcode;
    if (stats) {
        stats->iterations = 1; stats->kernel_launches = per_sample ? 2 : (two_pass ? 3 : 1);
        if (fr.timing) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ctx->events[2], ctx->events[3]) == hipSuccess) stats->ms_other = t;
            if (two_pass && hipEventElapsedTime(&t, ctx->events[0], ctx->events[1]) == hipSuccess) stats->ms_prepass = t;
            (void)hipGetLastError();
        }
    }
    return RL_OK;
}
extern "C" int rl_render_ao(rl_context* ctx, const rl_mc_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, int out_is_device,
                            void* stream, rl_render_stats* stats) { return render_mc(ctx, 0, params, block_seeds, n_blocks, out_rgb, out_is_device, stream, stats); }
extern "C" int rl_render_direct(rl_context* ctx, const rl_mc_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, int out_is_device,
                                void* stream, rl_render_stats* stats) { return render_mc(ctx, 1, params, block_seeds, n_blocks, out_rgb, out_is_device, stream, stats); }

// ---- IntegratorLightTracing::compute (light.rs:219-300) through the per-sample streams: k_seed_pixels forks one stream per light-path slot, k_light_fused
// traces spp light paths per slot and splats them into the fixed-point image, k_light_resolve writes the f32 image (light.hip.h).
extern "C" int rl_render_light(rl_context* ctx, const rl_path_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                               int out_is_device, void* stream_arg, rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (params->strategy < RL_LIGHT_ALL || params->strategy > RL_LIGHT_VOLUME) { rl_set_error("strategy must be RL_LIGHT_ALL, RL_LIGHT_SURFACE or RL_LIGHT_VOLUME"); return RL_ERR_INVALID_ARGUMENT; }
    if (params->stream_mode != RL_STREAM_PER_SAMPLE) { rl_set_error("the light tracer runs on per-sample streams only (stream_mode = RL_STREAM_PER_SAMPLE)"); return RL_ERR_UNSUPPORTED; }
    if (params->numerics != RL_NUMERICS_EXACT) { rl_set_error("the light tracer has no tolerance build (numerics = RL_NUMERICS_EXACT only)"); return RL_ERR_UNSUPPORTED; }
    if (params->shard_count > 1) { rl_set_error("the light tracer renders on one device (shard_count <= 1): every light path may splat anywhere"); return RL_ERR_UNSUPPORTED; }
    if (ctx->ds.env_emitter >= 0) { rl_set_error("the light tracer does not sample environment emitters"); return RL_ERR_UNSUPPORTED; }
    if (ctx->ds.n_emitters == 0) { rl_set_error("the light tracer needs an emitter"); return RL_ERR_NO_EMITTER; }
    if ((size_t)ctx->width * ctx->height > 0x7fffff00u) { rl_set_error("image too large"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    RenderFrame fr(ctx, block_seeds, n_blocks, out_rgb, out_is_device, stream_arg, stats, 0, 1);      // every block (shard_index is not read)
    const size_t n_pix = (size_t)fr.W * fr.H;
    const unsigned n_items = fr.n_pixels;
    if ((rcode = fr.alloc_tables()) != RL_OK) return rcode;
    if ((rcode = ctx->d_item_seed.ensure(n_items)) != RL_OK || (rcode = ctx->d_item_pixel.ensure(n_items)) != RL_OK) return rcode;
    // the splat image: [W*H*3] u64 low words of the sums, then [W*H] u32 inf flags, then [W*H*3] u32 carry words — in the sample-state buffer of
    // reference-order streams, which this call does not use
    const size_t acc_words = (3 * n_pix + (4 * n_pix + 1) / 2 + 3) / 4;     // in units of the buffer's 4 x u64 entries
    if ((rcode = ctx->d_sample_states.ensure(acc_words * 4)) != RL_OK) return rcode;
    // lanes per light-path slot: small frames get several (each tracing every split-th sample of the slot), so that about two rounds of the chip's resident waves run
    const size_t want_lanes = (size_t)std::max(fr.cus, 1) * kLightWaves * 4 * 64 * 2;
    unsigned split = 1;
    while (split * 2 <= params->spp && (size_t)n_items * split < want_lanes && (size_t)n_items * split * 2 <= 0x7fffff00u) split *= 2;
    const unsigned n_threads = std::max(256u, (unsigned)(((size_t)n_items * split + 255u) / 256u * 256u));
    if ((rcode = fr.alloc_output(n_threads / 256)) != RL_OK) return rcode;
    LightConst lc = ctx->light_cam;
    lc.render_surface = params->strategy != RL_LIGHT_VOLUME;
    lc.render_volume = params->strategy != RL_LIGHT_SURFACE;
    lc.accum = ctx->d_sample_states.get();
    lc.inf_flags = reinterpret_cast<unsigned*>(lc.accum + 3 * n_pix);
    lc.carry = lc.inf_flags + n_pix;
    if ((rcode = fr.upload(true, false)) != RL_OK) return rcode;
    HIP_OK(hipMemsetAsync(ctx->d_sample_states.get(), 0, acc_words * 4 * sizeof(unsigned long long), fr.st));
    if ((rcode = fr.zero_rows()) != RL_OK) return rcode;
    RenderConst rc = fr.render_const(params->spp, RL_STREAM_PER_SAMPLE, params->seed_variant);
    rc.has_min = params->has_min_depth; rc.min_depth = params->min_depth;
    rc.has_max = params->has_max_depth; rc.max_depth = params->max_depth;
    rc.has_rr = params->has_rr_depth; rc.rr_depth = params->rr_depth;
    rc.n_items = n_items;
    rc.split = split;
    StackConf stc;
    if ((rcode = stack_conf(ctx, n_threads, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    if ((rcode = fr.grow_events(4)) != RL_OK) return rcode;
    const hipStream_t st = fr.st;
    hipLaunchKernelGGL(k_seed_pixels, dim3(((unsigned)fr.owned.size() + 63) / 64), dim3(64), 0, st, rc);
    if (fr.timing) hipEventRecord(ctx->events[2], st);
    (ctx->lds_scene ? launch_light_lds : launch_light_stream)(ctx->single_bsdf ? ctx->bsdf_type : -1, ctx->ds.medium.enabled != 0, dim3(n_threads / 256), dim3(256), lds, st, rc, ctx->ds, stc, lc);
    if (fr.timing) hipEventRecord(ctx->events[3], st);
    launch_light_resolve(dim3((unsigned)((n_pix + 255) / 256)), dim3(256), st, rc, lc);
    if ((rcode = fr.download()) != RL_OK) return rcode;
    if (stats) {
        stats->reserved[0] = fr.totals[STAT_SPLATS]; stats->reserved[1] = fr.totals[STAT_SPLATS_INVALID]; stats->reserved[2] = fr.totals[STAT_SPLATS_SATURATED];
        stats->iterations = 1; stats->kernel_launches = 3;
        if (fr.timing) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ctx->events[2], ctx->events[3]) == hipSuccess) stats->ms_other = t;
            (void)hipGetLastError();
        }
    }
    return RL_OK;
}

// ---- IntegratorVPL::compute (vpl.rs:182-535): rl_vpl_generate shoots the VPLs on one lane (k_vpl_generate), rl_render_vpl gathers them per sample index
// (k_vpl_primary, k_vpl_gather) and scales the pixel sums (k_vpl_resolve); see vpl.hip.h
static constexpr unsigned kVplTimedPasses = 256;
struct rl_vpl_set {
    const rl_context* ctx;            // the context that made it (compared, never dereferenced: the context may be destroyed first)
    int device;
    HipBuffer<unsigned> words;        // [n_vpl][RL_VPL_WORDS]
    uint64_t n_vpl = 0, n_paths = 0;
};
static int check_vpl_scene(const rl_context* ctx) {
    if (ctx->ds.env_emitter >= 0) { rl_set_error("vpl does not sample environment emitters"); return RL_ERR_UNSUPPORTED; }
    if (ctx->ds.n_emitters == 0) { rl_set_error("vpl needs an emitter"); return RL_ERR_NO_EMITTER; }
    return RL_OK;
}
// what both generation entry points refuse before any kernel runs
static int check_vpl_generate(const rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, const rl_sampler* sampler, rl_vpl_set** out) {
    if (!ctx || !params || !sampler || !out) return RL_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (option_vpl < RL_VPL_ALL || option_vpl > RL_VPL_VOLUME) { rl_set_error("option_vpl must be RL_VPL_ALL, RL_VPL_SURFACE or RL_VPL_VOLUME"); return RL_ERR_INVALID_ARGUMENT; }
    if (nb_vpl == 0 || nb_vpl > (uint32_t)RL_VPL_MAX) { rl_set_error("nb_vpl must be 1 .. RL_VPL_MAX"); return RL_ERR_INVALID_ARGUMENT; }
    if (params->has_max_depth && params->max_depth <= 1) { rl_set_error("vpl needs max_depth >= 2 (the light vertex has no edge otherwise, vpl.rs:138)"); return RL_ERR_INVALID_ARGUMENT; }
    int rcode;
    if ((rcode = check_vpl_scene(ctx)) != RL_OK) return rcode;
    const bool medium = ctx->ds.medium.enabled != 0;
    if (option_vpl == RL_VPL_VOLUME && !medium) { rl_set_error("vpl -v volume needs a medium (the reference never stores a VPL)"); return RL_ERR_UNSUPPORTED; }
    if (medium) {
        if (ctx->has_directional) { rl_set_error("vpl does not take a directional light with a medium (vpl.rs:324, 418)"); return RL_ERR_UNSUPPORTED; }
    }
    return RL_OK;
}
// The light passes that store records along light paths — the VPLs (and the photons they double as) and the photon beams (beam_render.hip.h) — share their two
// host sequences; a pass names its record size and its refusal, and launches its own kernels.
struct LightPassKind {
    unsigned rec_words;               // u32 per record
    const char* too_few;              // rl_last_error when RL_VPL_MAX_PATHS paths store fewer than nb records
};
static const LightPassKind kVplPass{RL_VPL_WORDS, "vpl: fewer than nb_vpl VPLs stored within RL_VPL_MAX_PATHS light paths"};
// A pass that stores a second kind of record along the same paths (the photon planes' surface beams, pplane_render.hip.h) hands both sequences one of these.
// The first kind is the one the shooting stops on; the second is not bounded by it, so the pass is refused once more than max_records of it arise before the
// first kind's count is reached.  A path stores at most kDepthCap of them.  The sequences fill the last three members for the pass's launch to read.
struct LightPassSecond {
    unsigned rec_words;               // u32 per record
    unsigned max_records;
    const char* too_many;             // rl_last_error of that refusal (RL_ERR_UNSUPPORTED)
    HipBuffer<unsigned>* words;       // on RL_OK [*n_records][rec_words]
    uint64_t* n_records;
    unsigned cap = 0;                 // records *words has room for
    unsigned* d_words = nullptr;
    const unsigned* d_offsets = nullptr;      // the per-path write pass: [path] the index of the path's first record
};
// The serial pass (k_vpl_generate, k_beam_generate): one lane on the main sampler's stream.  launch(lds_bytes, rc, stc, vc); on RL_OK *words holds *n_records
// records of *n_paths paths and `sampler` is the one the lane left
template <class Launch>
static int light_pass_serial(rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, const LightPassKind& kind, rl_sampler* sampler,
                             HipBuffer<unsigned>* words, uint64_t* n_records, uint64_t* n_paths, rl_render_stats* stats, Launch&& launch, LightPassSecond* second = nullptr) {
    int rcode;
    const unsigned cap = nb_vpl + kDepthCap + 1u;        // the last path adds at most one record per vertex
    if ((rcode = words->ensure((size_t)cap * kind.rec_words)) != RL_OK) return rcode;
    if (second) {                                        // the lane stops once more than max_records are stored: one path beyond that at most
        second->cap = second->max_records + kDepthCap + 1u;
        if ((rcode = second->words->ensure((size_t)second->cap * second->rec_words)) != RL_OK) return rcode;
        second->d_words = second->words->get();
    }
    RenderConst rc{};
    rc.has_max = params->has_max_depth; rc.max_depth = params->max_depth;
    rc.has_rr = params->has_rr_depth; rc.rr_depth = params->rr_depth;
    VplConst vc{};
    vc.nb_vpl = nb_vpl; vc.cap = cap; vc.max_paths = RL_VPL_MAX_PATHS;
    vc.option_vpl = option_vpl;
    vc.vpl_words = words->get();
    StackConf stc;
    if ((rcode = stack_conf(ctx, 256, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    LaneRun run;
    if ((rcode = run_one_lane(ctx->stream, stats != nullptr && !ctx->knobs.has(K_NO_EVENTS), sampler, VPL_GEN_WORDS + (second ? 1 : 0), &run, [&](unsigned long long* d_gen) {
            vc.gen_state = d_gen; vc.gen_out = d_gen + 4;
            launch(lds, rc, stc, vc);
        })) != RL_OK) return rcode;
    const unsigned long long* g = run.words.data() + 4;
    if (g[VPL_GEN_VPLS] < nb_vpl && second && g[VPL_GEN_WORDS] > second->max_records) { rl_set_error(second->too_many); return RL_ERR_UNSUPPORTED; }
    if (g[VPL_GEN_VPLS] < nb_vpl) { rl_set_error(kind.too_few); return RL_ERR_UNSUPPORTED; }
    if (second) *second->n_records = g[VPL_GEN_WORDS];          // the lane's counter beyond the shared five
    for (int i = 0; i < 4; i++) sampler->s[i] = run.words[i];
    *n_records = g[VPL_GEN_VPLS]; *n_paths = g[VPL_GEN_PATHS];
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->camera_samples = g[VPL_GEN_PATHS]; stats->vertices = g[VPL_GEN_VERTICES]; stats->extension_rays = g[VPL_GEN_EXT]; stats->rng_draws = g[VPL_GEN_DRAWS];
        stats->iterations = 1; stats->kernel_launches = 1; stats->ms_prepass = run.ev.ms;
        stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - run.t0).count();
    }
    return RL_OK;
}
extern "C" int rl_vpl_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, rl_sampler* sampler, rl_vpl_set** out,
                               rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_vpl_generate(ctx, params, nb_vpl, option_vpl, sampler, out)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    auto set = std::make_unique<rl_vpl_set>();
    set->ctx = ctx; set->device = ctx->device;
    if ((rcode = light_pass_serial(ctx, params, nb_vpl, option_vpl, kVplPass, sampler, &set->words, &set->n_vpl, &set->n_paths, stats,
                                   [&](size_t lds, const RenderConst& rc, const StackConf& stc, const VplConst& vc) {
            (ctx->lds_scene ? launch_vpl_lds : launch_vpl_stream)(0, ctx->single_bsdf ? ctx->bsdf_type : -1, ctx->ds.medium.enabled != 0, dim3(1), dim3(256), lds, ctx->stream, rc, ctx->ds, stc, vc);
        })) != RL_OK) return rcode;
    *out = set.release();
    return RL_OK;
}
// rl_vpl_generate_paths: the same generation with one light path per lane, each on its own stream (vpl_paths.hip.h has the contract).  Rounds: a count pass
// over a batch of path indices, the counts brought to the host, which takes their prefix sum and looks for K (the smallest path count that stores nb_vpl
// records); when the batch did not reach it, the next one is sized from the records per path measured so far.  Then one write pass over paths 0 .. K-1.
static constexpr unsigned kVplFirstBatch = 4096, kVplShootGroupsPerCu = 2;
// launch(write, groups, lds_bytes, rc, stc, pc) on ctx->stream (k_vpl_shoot, k_beam_shoot); the results as light_pass_serial leaves them
template <class Launch>
static int light_pass_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, const LightPassKind& kind, rl_sampler* sampler,
                            HipBuffer<unsigned>* words, uint64_t* n_records, uint64_t* n_paths, rl_render_stats* stats, Launch&& launch, LightPassSecond* second = nullptr) {
    int rcode;
    const hipStream_t st = ctx->stream;
    const size_t cw = VPL_PATH_WORDS + (second ? 1 : 0);     // count words per path: a second kind of record adds its count behind the shared four
    const long long forced = ctx->knobs.has(K_VPL_BATCH_PATHS) ? std::max<long long>(1, ctx->knobs.i(K_VPL_BATCH_PATHS, 0)) : 0;
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) { (void)hipGetLastError(); cus = 256; }
    const unsigned max_groups = (unsigned)std::max(cus, 1) * kVplShootGroupsPerCu;
    RenderConst rc{};
    rc.has_max = params->has_max_depth; rc.max_depth = params->max_depth;
    rc.has_rr = params->has_rr_depth; rc.rr_depth = params->rr_depth;
    rc.seed_variant = params->seed_variant;
    VplPathsConst pc{};
    for (int i = 0; i < 4; i++) pc.main[i] = sampler->s[i];
    pc.option_vpl = option_vpl;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    EventPair ev;
    if ((rcode = ev.open(stats != nullptr && !ctx->knobs.has(K_NO_EVENTS))) != RL_OK) return rcode;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned launches = 0, rounds = 0;
    // one launch over paths first .. first + count - 1: persistent workgroups stride over the batch
    auto shoot = [&](bool write, unsigned first, unsigned count) -> int {
        const unsigned groups = std::min((count + 255u) / 256u, max_groups);
        StackConf stc;
        int r = stack_conf(ctx, (size_t)groups * 256, &stc);
        if (r != RL_OK) return r;
        pc.first = first; pc.count = count;
        ev.begin(st);
        launch(write, groups, lds, rc, stc, pc);
        ev.end(st);
        launches++;
        return RL_OK;
    };
    // ---- count rounds
    HipBuffer<unsigned> d_counts;
    std::vector<unsigned> counts;                    // [path][cw], every path walked so far
    std::vector<unsigned> offsets, offsets2;         // [path] exclusive prefix sum of the record counts (of the second kind's), paths 0 .. K-1 once K is known
    unsigned long long stored = 0, stored2 = 0;
    unsigned walked = 0, K = 0;
    while (K == 0 && walked < (unsigned)RL_VPL_MAX_PATHS) {
        unsigned batch;
        if (forced) batch = (unsigned)std::min<long long>(forced, RL_VPL_MAX_PATHS);
        else if (walked == 0) batch = std::max(kVplFirstBatch, nb_vpl / 8u);       // a light path seldom stores more than 8 records
        else {
            // the measured records per path, plus a margin of an eighth and 64 paths; when nothing was stored yet, twice what was walked
            const double per_path = (double)stored / (double)walked;
            batch = stored ? (unsigned)std::min<double>((double)RL_VPL_MAX_PATHS, (double)(nb_vpl - stored) / per_path * 1.125 + 64.0) : 2u * walked;
        }
        batch = std::min(batch, (unsigned)RL_VPL_MAX_PATHS - walked);
        if ((rcode = d_counts.ensure((size_t)batch * cw)) != RL_OK) return rcode;
        pc.counts = d_counts.get();
        if ((rcode = shoot(false, walked, batch)) != RL_OK) return rcode;
        counts.resize((size_t)(walked + batch) * cw);
        HIP_OK(hipMemcpyAsync(counts.data() + (size_t)walked * cw, d_counts.get(), (size_t)batch * cw * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipGetLastError());
        ev.add();
        rounds++;
        for (unsigned k = walked; k < walked + batch && K == 0; k++) {            // the cut: `while stored < nb` on this path sequence
            offsets.push_back((unsigned)stored);
            stored += counts[(size_t)k * cw + VPL_PATH_RECORDS];
            if (second) { offsets2.push_back((unsigned)stored2); stored2 += counts[(size_t)k * cw + VPL_PATH_WORDS]; }
            if (stored >= nb_vpl) K = k + 1u;
            else if (second && stored2 > second->max_records) { rl_set_error(second->too_many); return RL_ERR_UNSUPPORTED; }      // where the serial lane stops
        }
        walked += batch;
    }
    if (K == 0) { rl_set_error(kind.too_few); return RL_ERR_UNSUPPORTED; }
    // ---- write pass: paths 0 .. K-1 again, each to its own offset
    HipBuffer<unsigned> d_offsets, d_offsets2;
    if ((rcode = words->ensure((size_t)stored * kind.rec_words)) != RL_OK || (rcode = d_offsets.ensure(K)) != RL_OK) return rcode;
    HIP_OK(hipMemcpyAsync(d_offsets.get(), offsets.data(), (size_t)K * sizeof(unsigned), hipMemcpyHostToDevice, st));
    if (second) {
        if ((rcode = second->words->ensure((size_t)stored2 * second->rec_words)) != RL_OK || (rcode = d_offsets2.ensure(K)) != RL_OK) return rcode;
        HIP_OK(hipMemcpyAsync(d_offsets2.get(), offsets2.data(), (size_t)K * sizeof(unsigned), hipMemcpyHostToDevice, st));
        second->cap = (unsigned)stored2; second->d_words = second->words->get(); second->d_offsets = d_offsets2.get();
        *second->n_records = stored2;
    }
    pc.cap = (unsigned)stored; pc.vpl_words = words->get(); pc.offsets = d_offsets.get(); pc.counts = nullptr;
    if ((rcode = shoot(true, 0u, K)) != RL_OK) return rcode;
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    ev.add();
    for (unsigned k = 0; k < K; k++) (void)rl_sampler_next_u64(sampler);           // the K clone_box calls
    *n_records = stored; *n_paths = K;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->camera_samples = K;
        for (unsigned k = 0; k < K; k++) {
            const unsigned* c = &counts[k * cw];
            stats->vertices += c[VPL_PATH_VERTICES]; stats->extension_rays += c[VPL_PATH_EXT]; stats->rng_draws += c[VPL_PATH_DRAWS];
        }
        stats->iterations = rounds; stats->kernel_launches = launches; stats->ms_prepass = ev.ms;
        stats->reserved[0] = walked;
        stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RL_OK;
}
extern "C" int rl_vpl_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, rl_sampler* sampler, rl_vpl_set** out,
                                     rl_render_stats* stats) {
    int rcode;
    if ((rcode = check_vpl_generate(ctx, params, nb_vpl, option_vpl, sampler, out)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    auto set = std::make_unique<rl_vpl_set>();
    set->ctx = ctx; set->device = ctx->device;
    if ((rcode = light_pass_paths(ctx, params, nb_vpl, option_vpl, kVplPass, sampler, &set->words, &set->n_vpl, &set->n_paths, stats,
                                  [&](bool write, unsigned groups, size_t lds, const RenderConst& rc, const StackConf& stc, const VplPathsConst& pc) {
            (ctx->lds_scene ? launch_vpl_paths_lds : launch_vpl_paths_stream)(write, ctx->single_bsdf ? ctx->bsdf_type : -1, ctx->ds.medium.enabled != 0, dim3(groups), dim3(256), lds,
                                                                              ctx->stream, rc, ctx->ds, stc, pc);
        })) != RL_OK) return rcode;
    *out = set.release();
    return RL_OK;
}
extern "C" int rl_vpl_info(const rl_vpl_set* set, uint64_t* n_vpl, uint64_t* n_paths) {
    if (!set) return RL_ERR_INVALID_ARGUMENT;
    if (n_vpl) *n_vpl = set->n_vpl;
    if (n_paths) *n_paths = set->n_paths;
    return RL_OK;
}
extern "C" int rl_vpl_read(const rl_vpl_set* set, uint32_t* words, size_t n_words) {
    if (!set || !words || n_words != set->n_vpl * RL_VPL_WORDS) return RL_ERR_INVALID_ARGUMENT;
    HIP_OK(hipSetDevice(set->device));
    HIP_OK(hipMemcpy(words, set->words.get(), n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RL_OK;
}
extern "C" void rl_vpl_destroy(rl_vpl_set* set) {
    if (!set) return;
    (void)hipSetDevice(set->device);
    delete set;
}
extern "C" int rl_render_vpl(rl_context* ctx, const rl_vpl_set* set, const rl_path_params* params, int option_lt, const uint64_t* block_seeds, size_t n_blocks,
                             float* out_rgb, int out_is_device, void* stream_arg, rl_render_stats* stats) {
    int rcode;
    if (!set) return RL_ERR_INVALID_ARGUMENT;
    if ((rcode = check_frame(ctx, params, block_seeds, n_blocks, out_rgb)) != RL_OK) return rcode;
    if (set->ctx != ctx) { rl_set_error("the VPL set belongs to another context"); return RL_ERR_INVALID_ARGUMENT; }
    if (option_lt < RL_VPL_ALL || option_lt > RL_VPL_VOLUME) { rl_set_error("option_lt must be RL_VPL_ALL, RL_VPL_SURFACE or RL_VPL_VOLUME"); return RL_ERR_INVALID_ARGUMENT; }
    if (params->shard_index >= (params->shard_count ? params->shard_count : 1)) return RL_ERR_INVALID_ARGUMENT;
    if (params->stream_mode != RL_STREAM_REFERENCE_ORDER) { rl_set_error("vpl runs on reference-order streams only (stream_mode = RL_STREAM_REFERENCE_ORDER)"); return RL_ERR_UNSUPPORTED; }
    if (params->numerics != RL_NUMERICS_EXACT) { rl_set_error("vpl has no tolerance build (numerics = RL_NUMERICS_EXACT only)"); return RL_ERR_UNSUPPORTED; }
    if (params->spp > (uint32_t)RL_VPL_MAX_SPP) { rl_set_error("vpl takes at most RL_VPL_MAX_SPP spp (a block's stream is entered with 32-bit jumps)"); return RL_ERR_UNSUPPORTED; }
    if ((rcode = check_vpl_scene(ctx)) != RL_OK) return rcode;
    HIP_OK(hipSetDevice(ctx->device));
    RenderFrame fr(ctx, block_seeds, n_blocks, out_rgb, out_is_device, stream_arg, stats, params->shard_index, params->shard_count);
    const bool medium = ctx->ds.medium.enabled != 0;
    const unsigned n_items = fr.n_pixels;
    const unsigned n_owned = (unsigned)fr.owned.size();
    const unsigned gather_threads = std::max(256u, (n_items + 255u) / 256u * 256u);
    const unsigned n_threads = std::max(gather_threads, n_owned * 256u);
    if ((rcode = fr.alloc_tables()) != RL_OK) return rcode;
    // per pixel item: the stream state [4 u64], the gather point [kVplGatherWords u32], the sum [3 f32]; then the live-point counter
    const size_t state_words = (size_t)n_items * 4, gp_u64 = ((size_t)n_items * kVplGatherWords + 1) / 2, acc_u64 = ((size_t)n_items * 3 + 1) / 2;
    if ((rcode = ctx->d_sample_states.ensure(state_words + gp_u64 + acc_u64 + 1)) != RL_OK) return rcode;
    if ((rcode = fr.alloc_output(std::max(n_threads / 256, 1u))) != RL_OK) return rcode;
    if ((rcode = fr.upload(true, true)) != RL_OK || (rcode = fr.zero_rows()) != RL_OK) return rcode;
    RenderConst rc = fr.render_const(params->spp, RL_STREAM_REFERENCE_ORDER, params->seed_variant);
    rc.n_items = n_items;
    VplConst vc{};
    vc.option_lt = option_lt;
    vc.vpls = set->words.get(); vc.n_vpl = (unsigned)set->n_vpl;
    vc.norm_vpl = 1.0f / (float)set->n_paths;               // norm_vpl = 1.0 / nb_path_shot as f32 (vpl.rs:213)
    vc.draws = medium ? 3u : 2u;
    unsigned long long* base = ctx->d_sample_states.get();
    vc.pix_state = base;
    vc.gpoints = reinterpret_cast<unsigned*>(base + state_words);
    vc.acc = reinterpret_cast<float*>(base + state_words + gp_u64);
    vc.n_live = reinterpret_cast<unsigned*>(base + state_words + gp_u64 + acc_u64);
    StackConf stc;
    if ((rcode = stack_conf(ctx, n_threads, &stc)) != RL_OK) return rcode;
    const size_t lds = traversal_lds_bytes(ctx, ctx->lds_scene, 256, false);
    const hipStream_t st = fr.st;
    const int mat = ctx->single_bsdf ? ctx->bsdf_type : -1;
    auto launch = ctx->lds_scene ? launch_vpl_lds : launch_vpl_stream;
    const bool timing = fr.timing && params->spp <= kVplTimedPasses;      // per-pass events (beyond that many passes the kernel times are not taken)
    if (timing && (rcode = fr.grow_events(2 * (size_t)params->spp + 1)) != RL_OK) return rcode;
    for (unsigned s = 0; s < params->spp && n_owned > 0; s++) {
        vc.sample = s;
        HIP_OK(hipMemsetAsync(vc.n_live, 0, sizeof(unsigned), st));
        if (timing) hipEventRecord(ctx->events[2 * s], st);
        launch(2, mat, medium, dim3(n_owned), dim3(256), lds, st, rc, ctx->ds, stc, vc);
        if (timing) hipEventRecord(ctx->events[2 * s + 1], st);
        launch(1, mat, medium, dim3(gather_threads / 256), dim3(256), lds, st, rc, ctx->ds, stc, vc);
    }
    if (timing) hipEventRecord(ctx->events[2 * (size_t)params->spp], st);
    if (n_owned > 0) launch_vpl_resolve(dim3(n_owned), dim3(256), st, rc, vc);
    if ((rcode = fr.download()) != RL_OK) return rcode;
    if (stats) {
        stats->reserved[0] = fr.totals[STAT_VPL_SURFACE]; stats->reserved[1] = fr.totals[STAT_VPL_VOLUME];
        stats->iterations = params->spp; stats->kernel_launches = n_owned > 0 ? 2ull * params->spp + 1 : 0;
        if (timing && n_owned > 0) {
            double raygen = 0.0, gather = 0.0;
            for (unsigned s = 0; s < params->spp; s++) {
                float t = 0.0f;
                if (hipEventElapsedTime(&t, ctx->events[2 * s], ctx->events[2 * s + 1]) == hipSuccess) raygen += t;
                hipEvent_t end = s + 1 < params->spp ? ctx->events[2 * (s + 1)] : ctx->events[2 * (size_t)params->spp];
                if (hipEventElapsedTime(&t, ctx->events[2 * s + 1], end) == hipSuccess) gather += t;
            }
            stats->ms_raygen = raygen; stats->ms_other = gather;
            (void)hipGetLastError();
        }
    }
    return RL_OK;
}

#include "gather_render.hip.h"
#include "beam_render.hip.h"
#include "vrl_render.hip.h"
#include "pplane_render.hip.h"
#include "pn_render.hip.h"
#include "pnmis_render.hip.h"
#include "pntaylor_render.hip.h"
#include "pnats_render.hip.h"

// ---- batched Acceleration::{trace, visible}
namespace {
constexpr size_t kMaxBatch = 0x7fffff00u;   // grid and kernel argument are 32-bit
}  // namespace
extern "C" int rl_trace_batch(rl_context* ctx, size_t n, const float* origins, const float* directions, float* t_out, float* u_out,
                              float* v_out, int32_t* mesh_out, int32_t* tri_out) {
    if (!ctx || (n && (!origins || !directions || !t_out || !u_out || !v_out || !mesh_out || !tri_out))) return RL_ERR_INVALID_ARGUMENT;
    if (n == 0) return RL_OK;
    if (n > kMaxBatch) { rl_set_error("batch too large"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    HipBuffer<float> b_o, b_d, b_t, b_u, b_v; HipBuffer<int> b_m, b_tr;
    int rcode;
    if ((rcode = b_o.ensure(3 * n)) != RL_OK || (rcode = b_d.ensure(3 * n)) != RL_OK || (rcode = b_t.ensure(n)) != RL_OK || (rcode = b_u.ensure(n)) != RL_OK ||
        (rcode = b_v.ensure(n)) != RL_OK || (rcode = b_m.ensure(n)) != RL_OK || (rcode = b_tr.ensure(n)) != RL_OK) return rcode;
    float *d_o = b_o.get(), *d_d = b_d.get(), *d_t = b_t.get(), *d_u = b_u.get(), *d_v = b_v.get();
    int *d_m = b_m.get(), *d_tr = b_tr.get();
    HIP_OK(hipMemcpy(d_o, origins, 3 * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_d, directions, 3 * n * 4, hipMemcpyHostToDevice));
    size_t lds = traversal_lds_bytes(ctx, false, 256, false);
    StackConf stc;
    if ((rcode = stack_conf(ctx, (n + 255) / 256 * 256, &stc)) != RL_OK) return rcode;
    hipLaunchKernelGGL(k_trace_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), lds, ctx->stream, ctx->ds, stc, (unsigned)n, d_o, d_d, d_t, d_u, d_v, d_m, d_tr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(ctx->stream));
    HIP_OK(hipMemcpy(t_out, d_t, n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(u_out, d_u, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(v_out, d_v, n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(mesh_out, d_m, n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tri_out, d_tr, n * 4, hipMemcpyDeviceToHost));
    return RL_OK;
}

extern "C" int rl_visible_batch(rl_context* ctx, size_t n, const float* p0, const float* p1, uint8_t* visible_out) {
    if (!ctx || (n && (!p0 || !p1 || !visible_out))) return RL_ERR_INVALID_ARGUMENT;
    if (n == 0) return RL_OK;
    if (n > kMaxBatch) { rl_set_error("batch too large"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    HipBuffer<float> b_a, b_b; HipBuffer<unsigned char> b_o;
    int rcode;
    if ((rcode = b_a.ensure(3 * n)) != RL_OK || (rcode = b_b.ensure(3 * n)) != RL_OK || (rcode = b_o.ensure(n)) != RL_OK) return rcode;
    float *d_a = b_a.get(), *d_b = b_b.get(); unsigned char* d_o = b_o.get();
    HIP_OK(hipMemcpy(d_a, p0, 3 * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_b, p1, 3 * n * 4, hipMemcpyHostToDevice));
    size_t lds = traversal_lds_bytes(ctx, false, 256, false);
    StackConf stc;
    if ((rcode = stack_conf(ctx, (n + 255) / 256 * 256, &stc)) != RL_OK) return rcode;
    hipLaunchKernelGGL(k_visible_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), lds, ctx->stream, ctx->ds, stc, (unsigned)n, d_a, d_b, d_o);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(ctx->stream));
    HIP_OK(hipMemcpy(visible_out, d_o, n, hipMemcpyDeviceToHost));
    return RL_OK;
}

// ---- debug / test hooks (declared in wavefront.h, exported for the test-suite)
extern "C" int rl_debug_visible_batch_lds(rl_context* ctx, size_t n, const float* p0, const float* p1, int packed, int capacity, uint8_t* visible_out) {
    if (!ctx || (n && (!p0 || !p1 || !visible_out)) || capacity < 0) return RL_ERR_INVALID_ARGUMENT;
    if (!ctx->lds_scene) { rl_set_error("rl_debug_visible_batch_lds: the scene is not staged in LDS"); return RL_ERR_UNSUPPORTED; }
    if (n == 0) return RL_OK;
    if (n > kMaxBatch) { rl_set_error("batch too large"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    HipBuffer<float> b_a, b_b; HipBuffer<unsigned char> b_o;
    int rcode;
    if ((rcode = b_a.ensure(3 * n)) != RL_OK || (rcode = b_b.ensure(3 * n)) != RL_OK || (rcode = b_o.ensure(n)) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(b_a.get(), p0, 3 * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b_b.get(), p1, 3 * n * 4, hipMemcpyHostToDevice));
    const size_t lds = traversal_lds_bytes(ctx, true, 256, false);
    StackConf stc;
    if ((rcode = stack_conf(ctx, (n + 255) / 256 * 256, &stc)) != RL_OK) return rcode;
    stc.pack_cap = std::min(capacity, kLdsStackLevels);
    hipLaunchKernelGGL(k_visible_batch_lds, dim3((unsigned)((n + 255) / 256)), dim3(256), lds, ctx->stream, ctx->ds, stc, (unsigned)n, b_a.get(), b_b.get(), b_o.get(), packed);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(ctx->stream));
    HIP_OK(hipMemcpy(visible_out, b_o.get(), n, hipMemcpyDeviceToHost));
    return RL_OK;
}
extern "C" int rl_debug_numerics(int device, size_t n, const float* a, const float* b, float* out8) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return RL_ERR_NO_DEVICE;
    if (n > kMaxBatch / 16) return RL_ERR_INVALID_ARGUMENT;
    HIP_OK(hipSetDevice(device));
    HipBuffer<float> b_a, b_b, b_out;
    int rcode;
    if ((rcode = b_a.ensure(n)) != RL_OK || (rcode = b_b.ensure(n)) != RL_OK || (rcode = b_out.ensure(10 * n)) != RL_OK) return rcode;
    float *d_a = b_a.get(), *d_b = b_b.get(), *d_out = b_out.get();
    HIP_OK(hipMemcpy(d_a, a, n * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(d_b, b, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_numerics_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (unsigned)n, d_a, d_b, d_out, d_out + n, d_out + 2 * n,
                       d_out + 3 * n, d_out + 4 * n, d_out + 5 * n, d_out + 6 * n, d_out + 7 * n, d_out + 8 * n, d_out + 9 * n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out8, d_out, 10 * n * 4, hipMemcpyDeviceToHost));
    return RL_OK;
}

extern "C" int rl_debug_math_sweep(int device, int where, int fn, uint32_t first_bits, uint32_t stride, uint32_t period, size_t n, const float* b, size_t n_b,
                                   int swap, float* out) {
    if (fn < 0 || fn >= RL_MATH_COUNT || !out || n == 0 || (n_b != 0 && !b) || (n_b != 0 && n_b != 1 && n_b != n)) return RL_ERR_INVALID_ARGUMENT;
    if (n > kMaxBatch) { rl_set_error("batch too large"); return RL_ERR_INVALID_ARGUMENT; }
    if (where == RL_MATH_ON_HOST) return host_math_sweep(fn, first_bits, stride, period, n, b, n_b, swap, out);     // no HIP call on this arm
    if (where != RL_MATH_ON_DEVICE) return RL_ERR_INVALID_ARGUMENT;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return RL_ERR_NO_DEVICE;
    HIP_OK(hipSetDevice(device));
    HipBuffer<float> b_b, b_out;
    int rcode;
    if ((rcode = b_out.ensure(n)) != RL_OK || (n_b == n && n > 1 && (rcode = b_b.ensure(n)) != RL_OK)) return rcode;
    const float* d_b = nullptr;
    if (n_b == n && n > 1) { HIP_OK(hipMemcpy(b_b.get(), b, n * 4, hipMemcpyHostToDevice)); d_b = b_b.get(); }
    hipLaunchKernelGGL(k_math_sweep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, swap, (unsigned)first_bits, (unsigned)stride, (unsigned)period, (unsigned)n,
                       d_b, n_b ? b[0] : 0.0f, b_out.get());
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, b_out.get(), n * 4, hipMemcpyDeviceToHost));
    return RL_OK;
}

extern "C" int rl_debug_trace_batch_fast(rl_context* ctx, size_t n, const float* origins, const float* directions, float* t_out, int32_t* mesh_out, int32_t* tri_out, int32_t* steps_out) {
    if (!ctx || !n || !origins || !directions || !t_out || !mesh_out || !tri_out || !steps_out) return RL_ERR_INVALID_ARGUMENT;
    if (!ctx->ds.nodes4) { rl_set_error("the scene is staged in LDS: no BVH4"); return RL_ERR_UNSUPPORTED; }
    if (n > kMaxBatch) { rl_set_error("batch too large"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    HipBuffer<float> b_o, b_d, b_t; HipBuffer<int> b_m, b_tr, b_s;
    int rcode;
    if ((rcode = b_o.ensure(3 * n)) != RL_OK || (rcode = b_d.ensure(3 * n)) != RL_OK || (rcode = b_t.ensure(n)) != RL_OK || (rcode = b_m.ensure(n)) != RL_OK ||
        (rcode = b_tr.ensure(n)) != RL_OK || (rcode = b_s.ensure(n)) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(b_o.get(), origins, 3 * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b_d.get(), directions, 3 * n * 4, hipMemcpyHostToDevice));
    StackConf stc;
    if ((rcode = stack_conf(ctx, (n + 255) / 256 * 256, &stc)) != RL_OK) return rcode;
    launch_trace_batch_fast(dim3((unsigned)((n + 255) / 256)), dim3(256), traversal_lds_bytes(ctx, false, 256, false), ctx->stream, ctx->ds, stc, (unsigned)n, b_o.get(), b_d.get(),
                            b_t.get(), b_m.get(), b_tr.get(), b_s.get());
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(ctx->stream));
    HIP_OK(hipMemcpy(t_out, b_t.get(), n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(mesh_out, b_m.get(), n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tri_out, b_tr.get(), n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(steps_out, b_s.get(), n * 4, hipMemcpyDeviceToHost));
    return RL_OK;
}

// test hook: rl_trace_batch through the two-level records (traverse2) + node trips per ray; any_hit != 0: t_inout holds the segment lengths on entry and 1 / 0
// (a triangle was found / not) on return, as Acceleration::visible's inner `intersect` would (u, v, mesh, tri untouched)
extern "C" int rl_debug_trace_batch_two_level(rl_context* ctx, size_t n, const float* origins, const float* directions, float* t_inout, float* u_out, float* v_out,
                                              int32_t* mesh_out, int32_t* tri_out, int32_t* steps_out, int any_hit) {
    if (!ctx || !n || !origins || !directions || !t_inout || !u_out || !v_out || !mesh_out || !tri_out || !steps_out) return RL_ERR_INVALID_ARGUMENT;
    if (n > kMaxBatch) { rl_set_error("batch too large"); return RL_ERR_INVALID_ARGUMENT; }
    HIP_OK(hipSetDevice(ctx->device));
    { const int r2 = ensure_two_level(ctx); if (r2 != RL_OK) return r2; }
    HipBuffer<float> b_o, b_d, b_t, b_u, b_v; HipBuffer<int> b_m, b_tr, b_s;
    int rcode;
    if ((rcode = b_o.ensure(3 * n)) != RL_OK || (rcode = b_d.ensure(3 * n)) != RL_OK || (rcode = b_t.ensure(n)) != RL_OK || (rcode = b_u.ensure(n)) != RL_OK ||
        (rcode = b_v.ensure(n)) != RL_OK || (rcode = b_m.ensure(n)) != RL_OK || (rcode = b_tr.ensure(n)) != RL_OK || (rcode = b_s.ensure(n)) != RL_OK) return rcode;
    HIP_OK(hipMemcpy(b_o.get(), origins, 3 * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b_d.get(), directions, 3 * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b_t.get(), t_inout, n * 4, hipMemcpyHostToDevice));
    StackConf stc;
    if ((rcode = stack_conf(ctx, (n + 255) / 256 * 256, &stc)) != RL_OK) return rcode;
    hipLaunchKernelGGL(k_trace_batch_two_level, dim3((unsigned)((n + 255) / 256)), dim3(256), traversal_lds_bytes(ctx, false, 256, false), ctx->stream, ctx->ds, stc, (unsigned)n,
                       b_o.get(), b_d.get(), b_t.get(), b_u.get(), b_v.get(), b_m.get(), b_tr.get(), b_s.get(), any_hit);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(ctx->stream));
    HIP_OK(hipMemcpy(t_inout, b_t.get(), n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(steps_out, b_s.get(), n * 4, hipMemcpyDeviceToHost));
    if (!any_hit) {
        HIP_OK(hipMemcpy(u_out, b_u.get(), n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(v_out, b_v.get(), n * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(mesh_out, b_m.get(), n * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(tri_out, b_tr.get(), n * 4, hipMemcpyDeviceToHost));
    }
    return RL_OK;
}

extern "C" int rl_debug_sample_buf_bytes(const rl_context* ctx, uint64_t* bytes) {
    if (!ctx || !bytes) return RL_ERR_INVALID_ARGUMENT;
    *bytes = (uint64_t)ctx->d_sample_buf.capacity() * sizeof(float);
    return RL_OK;
}
extern "C" int rl_debug_bvh_sizes(const rl_context* ctx, uint64_t* n_ref_nodes, uint64_t* n_prims, uint32_t* stack_depth, int* lds_scene) {
    if (!ctx) return RL_ERR_INVALID_ARGUMENT;
    *n_ref_nodes = ctx->bvh_dump.ref_info.size(); *n_prims = ctx->bvh_dump.ref_prim_mesh.size();
    *stack_depth = ctx->bvh_dump.stack_depth; *lds_scene = ctx->lds_scene ? 1 : 0;
    return RL_OK;
}

extern "C" const char* rl_build_info(void) { return "rustlight_amd wavefront path tracer; kernels: gfx950 (hipcc, -ffp-contract=off)"; }
