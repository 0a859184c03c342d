// plane_generate.hip — IntegratorSinglePlane's plane pass (plane_single.rs:326-427): k_plane_generate, one lane, walks the main sampler's serial stream as
// the reference does; k_plane_generate_lanes, one lane per iteration of the loop, enters the same stream by jump-ahead and gives the same bytes.  The pass runs
// on the device because it needs the deterministic logf / sinf / cosf, which only devmath.hip.h holds; it traces nothing, so it opens no scene.  The state of the sampler comes from the host and goes back to it.
//
// Per iteration of `while planes.len() < nb_primitive`: one draw for id_emitter = (next() * n_lights as f32) as usize — clamped to n_lights - 1, where the
// reference would index out of range: the one deliberate difference —, then one plane (UV / VT / UT / UAlpha / CMIS) or the three planes UV, VT, UT
// (Average / DiscreteMIS).  A plane draws cosine_sample_hemisphere(next2d()) again while its z is 0, then next() for the medium's distance (of which
// continued_t is used), next2d() for `sample` and next() for alpha.
// Record (RL_PLANE_WORDS u32, the layout rl_plane_read documents): [0..2] o, [3..5] d0, [6..8] d1, [9] length0, [10] length1, [11..13] weight,
// [14..15] sample, [16] plane type, [17] id_emitter.
#include "common.hip.h"
#include "plane.hip.h"

namespace rl {

static constexpr unsigned kPlaneLanesBlock = 64;

__global__ void __launch_bounds__(64) k_plane_generate(PlaneGenConst gc) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    Rng rng; rng.s0 = gc.gen_state[0]; rng.s1 = gc.gen_state[1]; rng.s2 = gc.gen_state[2]; rng.s3 = gc.gen_state[3];
    const Col sigma_t = mkc(gc.sigma_t[0], gc.sigma_t[1], gc.sigma_t[2]), sigma_s = mkc(gc.sigma_s[0], gc.sigma_s[1], gc.sigma_s[2]);
    const bool three = gc.strategy == RL_PLANE_STRATEGY_AVERAGE || gc.strategy == RL_PLANE_STRATEGY_DISCRETE_MIS;
    const unsigned single = gc.strategy == RL_PLANE_STRATEGY_UV ? RL_PLANE_UV : gc.strategy == RL_PLANE_STRATEGY_VT ? RL_PLANE_VT
                          : gc.strategy == RL_PLANE_STRATEGY_UT ? RL_PLANE_UT : RL_PLANE_UALPHAT;
    unsigned long long n_planes = 0, n_gen = 0, n_draws = 0;
    while (n_planes < gc.nb_primitive) {
        unsigned id = (unsigned)(rng_next_f32(rng) * (float)gc.n_lights);
        n_draws++;
        if (id >= gc.n_lights) id = gc.n_lights - 1u;
        const PlaneLight& light = gc.lights[id];
        for (unsigned k = 0; k < (three ? 3u : 1u); k++) {
            const unsigned type = three ? (k == 0 ? RL_PLANE_UV : k == 1 ? RL_PLANE_VT : RL_PLANE_UT) : single;
            // generate_plane (326-361): the direction is drawn again while its z is 0
            Plane p; V2 sample;
            while (!plane_sample(rng, type, light, sigma_t, sigma_s, &p, &sample)) n_draws += 2;
            n_draws += 6;
            if (n_planes < gc.cap) {
                unsigned* w = gc.words + (size_t)n_planes * RL_PLANE_WORDS;
                w[0] = __float_as_uint(p.o.x); w[1] = __float_as_uint(p.o.y); w[2] = __float_as_uint(p.o.z);
                w[3] = __float_as_uint(p.d0.x); w[4] = __float_as_uint(p.d0.y); w[5] = __float_as_uint(p.d0.z);
                w[6] = __float_as_uint(p.d1.x); w[7] = __float_as_uint(p.d1.y); w[8] = __float_as_uint(p.d1.z);
                w[9] = __float_as_uint(p.l0); w[10] = __float_as_uint(p.l1);
                w[11] = __float_as_uint(p.weight.r); w[12] = __float_as_uint(p.weight.g); w[13] = __float_as_uint(p.weight.b);
                w[14] = __float_as_uint(sample.x); w[15] = __float_as_uint(sample.y);
                w[16] = type; w[17] = id;
            }
            n_planes++;
        }
        n_gen++;
    }
    gc.gen_state[0] = rng.s0; gc.gen_state[1] = rng.s1; gc.gen_state[2] = rng.s2; gc.gen_state[3] = rng.s3;
    gc.gen_out[PLANE_GEN_PLANES] = n_planes; gc.gen_out[PLANE_GEN_ITERATIONS] = n_gen; gc.gen_out[PLANE_GEN_DRAWS] = n_draws;
}

// One plane of the lane-parallel form: plane_sample for a plane of type `type` from light `id`, stored at `index`.  false, and nothing stored, when the
// direction's z is 0 (the serial walk draws it again).
RL_DEV bool plane_lane_one(const PlaneGenConst& gc, Rng& rng, unsigned type, unsigned id, unsigned index, Plane* made) {
    const Col sigma_t = mkc(gc.sigma_t[0], gc.sigma_t[1], gc.sigma_t[2]), sigma_s = mkc(gc.sigma_s[0], gc.sigma_s[1], gc.sigma_s[2]);
    Plane p; V2 sample;
    if (!plane_sample(rng, type, gc.lights[id], sigma_t, sigma_s, &p, &sample)) return false;
    unsigned* w = gc.words + (size_t)index * RL_PLANE_WORDS;
    w[0] = __float_as_uint(p.o.x); w[1] = __float_as_uint(p.o.y); w[2] = __float_as_uint(p.o.z);
    w[3] = __float_as_uint(p.d0.x); w[4] = __float_as_uint(p.d0.y); w[5] = __float_as_uint(p.d0.z);
    w[6] = __float_as_uint(p.d1.x); w[7] = __float_as_uint(p.d1.y); w[8] = __float_as_uint(p.d1.z);
    w[9] = __float_as_uint(p.l0); w[10] = __float_as_uint(p.l1);
    w[11] = __float_as_uint(p.weight.r); w[12] = __float_as_uint(p.weight.g); w[13] = __float_as_uint(p.weight.b);
    w[14] = __float_as_uint(sample.x); w[15] = __float_as_uint(sample.y);
    w[16] = type; w[17] = id;
    *made = p;
    return true;
}

// The lane-parallel form: lane i runs iteration i of the loop above.  Without a redraw an iteration takes D = 1 + 6 * per draws (the emitter; per plane 2 for the direction, 1 for the distance, 2 for `sample`, 1 for alpha), so iteration i starts D * i
// draws down the stream of the sampler in gc.gen_state, which every lane reads and nobody writes; lane 0 leaves the state D * n_gen draws on in gc.gen_out[0..4).
// gc.gen_out[PLANE_LANES_FLAG]: bit 0 = a lane met a direction with z == 0 (the stream is then not where the lanes took it to be: the host runs k_plane_generate instead),
// bit 1 = a plane with a corner that is not finite (what check_plane_records refuses, in its arithmetic).
__global__ void __launch_bounds__(kPlaneLanesBlock) k_plane_generate_lanes(PlaneGenConst gc, unsigned n_gen) {
    const unsigned i = blockIdx.x * kPlaneLanesBlock + threadIdx.x;
    if (i >= n_gen) return;
    const bool three = gc.strategy == RL_PLANE_STRATEGY_AVERAGE || gc.strategy == RL_PLANE_STRATEGY_DISCRETE_MIS;
    const unsigned single = gc.strategy == RL_PLANE_STRATEGY_UV ? RL_PLANE_UV : gc.strategy == RL_PLANE_STRATEGY_VT ? RL_PLANE_VT
                          : gc.strategy == RL_PLANE_STRATEGY_UT ? RL_PLANE_UT : RL_PLANE_UALPHAT;
    const unsigned per = three ? 3u : 1u, draws = 1u + 6u * per;
    Rng rng; rng.s0 = gc.gen_state[0]; rng.s1 = gc.gen_state[1]; rng.s2 = gc.gen_state[2]; rng.s3 = gc.gen_state[3];
    if (i == 0u) {
        Rng end = rng;
        rng_advance<false>(end, n_gen * draws);
        gc.gen_out[0] = end.s0; gc.gen_out[1] = end.s1; gc.gen_out[2] = end.s2; gc.gen_out[3] = end.s3;
    }
    rng_advance<false>(rng, i * draws);
    unsigned id = (unsigned)(rng_next_f32(rng) * (float)gc.n_lights);
    if (id >= gc.n_lights) id = gc.n_lights - 1u;
    unsigned flag = 0u;
    for (unsigned k = 0; k < per && flag == 0u; k++) {
        const unsigned type = three ? (k == 0 ? RL_PLANE_UV : k == 1 ? RL_PLANE_VT : RL_PLANE_UT) : single;
        Plane p;
        if (!plane_lane_one(gc, rng, type, id, i * per + k, &p)) { flag = 1u; break; }
        const V3 e0 = p.d0 * p.l0, e1 = p.d1 * p.l1, p0 = p.o + e0, p1 = p.o + e1, p2 = p0 + e1;
        if (!(finite_f(p.o.x) && finite_f(p.o.y) && finite_f(p.o.z) && finite_f(p0.x) && finite_f(p0.y) && finite_f(p0.z) && finite_f(p1.x) && finite_f(p1.y) &&
              finite_f(p1.z) && finite_f(p2.x) && finite_f(p2.y) && finite_f(p2.z))) flag = 2u;
    }
    if (flag) atomicOr((unsigned*)&gc.gen_out[PLANE_LANES_FLAG], flag);
}

void launch_plane_generate(hipStream_t st, const PlaneGenConst& gc) {
    hipLaunchKernelGGL(k_plane_generate, dim3(1), dim3(64), 0, st, gc);
}
void launch_plane_generate_lanes(hipStream_t st, const PlaneGenConst& gc, unsigned n_gen) {
    hipLaunchKernelGGL(k_plane_generate_lanes, dim3((n_gen + kPlaneLanesBlock - 1u) / kPlaneLanesBlock), dim3(kPlaneLanesBlock), 0, st, gc, n_gen);
}

}  // namespace rl
