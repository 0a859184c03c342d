// wavefront.h — test/debug hooks exported next to the public C-ABI (not part of the drop-in surface).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

struct rl_context;
struct rl_scene;
void rl_set_error(const std::string& s);

extern "C" {
// runs div/sqrt/mul-add and the deterministic transcendentals on the device: out8 = 8 arrays of n
int rl_debug_numerics(int device, size_t n, const float* a, const float* b, float* out8);
// one function of the numerics contract (fn: rl_math_fn) over an arithmetic progression of f32 bit patterns: out[i] = f(g_i, c_i), or f(c_i, g_i) when swap != 0,
// with g_i = the float whose bits are first_bits + (period ? i % period : i) * stride (mod 2^32; made where the function runs, nothing is uploaded for it) and
// c_i = b[i] (n_b == n), b[0] (n_b == 1) or 0 (n_b == 0: unary functions).  where = RL_MATH_ON_DEVICE: the kernels' own dm::*_det / div_rn / sqrt_rn on `device`;
// RL_MATH_ON_HOST: the host compiler's instantiation of detmath_shared.h in lighttree.cpp (sin, cos, acos, asin, atan2; RL_ERR_UNSUPPORTED for the rest), no GPU touched
enum rl_math_fn { RL_MATH_SINF = 0, RL_MATH_COSF = 1, RL_MATH_EXPF = 2, RL_MATH_LOGF = 3, RL_MATH_POWF = 4, RL_MATH_ACOSF = 5, RL_MATH_ATAN2F = 6, RL_MATH_ASINF = 7,
                  RL_MATH_SQRT_RN = 8, RL_MATH_DIV_RN = 9, RL_MATH_MUL_ADD = 10 /* a * b + a, uncontracted */, RL_MATH_COUNT = 11 };   // 0 ... 7 = orc_math_batch's codes
enum rl_math_where { RL_MATH_ON_DEVICE = 0, RL_MATH_ON_HOST = 1 };
int rl_debug_math_sweep(int device, int where, int fn, uint32_t first_bits, uint32_t stride, uint32_t period, size_t n, const float* b, size_t n_b, int swap, float* out);
// closest hits of a batch of rays through the tolerance build's traversal of a streaming scene (quantised BVH4, numerics = fast); steps = node trips per ray.
// RL_ERR_UNSUPPORTED for scenes staged in LDS (they have no BVH4).
int rl_debug_trace_batch_fast(rl_context* ctx, size_t n, const float* origins, const float* directions, float* t_out, int32_t* mesh_out, int32_t* tri_out, int32_t* steps_out);
// rl_trace_batch through the two-level node records (trace.hip.h: traverse2, which no renderer uses) + node trips per ray; any_hit: t_inout = segment lengths in, 1 / 0 out
int rl_debug_trace_batch_two_level(rl_context* ctx, size_t n, const float* origins, const float* directions, float* t_inout, float* u_out, float* v_out,
                                   int32_t* mesh_out, int32_t* tri_out, int32_t* steps_out, int any_hit);
// rl_visible_batch on a scene staged in LDS (RL_ERR_UNSUPPORTED otherwise): packed = 0 the per-lane any-hit loop, != 0 the wave's packed form (trace.hip.h: occluded_packed)
// with option shadow_pack_capacity = capacity (0: the stack's levels decide)
int rl_debug_visible_batch_lds(rl_context* ctx, size_t n, const float* p0, const float* p1, int packed, int capacity, uint8_t* visible_out);
// host only: the two-level records against the BVH2 they are derived from (bvh.cpp)
int rl_debug_check_two_level(const rl_scene* scene, uint64_t* out6);
// rng_advance (kernels/rngjump.h) on the device: states_out[i] = sampler states_in[i] (4 x u64) after counts[i] more draws
int rl_debug_rng_advance(int device, size_t n, const uint64_t* states_in, const uint32_t* counts, uint64_t* states_out);
// the stratified sampler of RL_STREAM_STRATIFIED (sampler.hip.h) on the device: pixel p (its per-sample-mode seed pixel_seeds[p]) walks its spp samples as the
// renderers do, each taking the call pattern (n_calls entries, 1 = next(), 2 = next2d()); out[(p * spp + s) * n_out + j] = the j-th value drawn by sample s,
// n_out = sum of the pattern
int rl_debug_stratified_draws(int device, size_t n_pixels, const uint64_t* pixel_seeds, uint32_t spp, int seed_variant, size_t n_calls, const int32_t* pattern, float* out);
// host only: out[y * W + x] = 1 where every camera sample of the pixel takes exactly two draws (its rays cannot reach the scene's bounding box; k_stream_spec's shortcut)
int rl_debug_trivial_pixels(const rl_scene* scene, int has_max_depth, uint32_t max_depth, uint8_t* out);
// bytes of the per-sample parking buffer the context holds (sample-parallel pixels, the tail of the persistent kernel): 0 until a render needed it
int rl_debug_sample_buf_bytes(const rl_context* ctx, uint64_t* bytes);
int rl_debug_bvh_sizes(const rl_context* ctx, uint64_t* n_ref_nodes, uint64_t* n_prims, uint32_t* stack_depth, int* lds_scene);
// host-only: builds the BVH of `scene` and returns it in the reference's node shape (no GPU needed)
int rl_debug_bvh(const rl_scene* scene, uint64_t* n_nodes, uint64_t* n_prims, float* boxes, uint64_t* info, uint64_t* count,
                 int32_t* prim_mesh, int32_t* prim_tri);
// host-only: Camera::generate for one pixel position
int rl_debug_emitters_cdf(const rl_scene* scene, uint64_t* n_entries, float* cdf);
int rl_debug_ats(const rl_scene* scene, uint64_t* n_nodes, float* nodes16, uint64_t* n_lights, int32_t* light_emitter, int32_t* light_prim);
int rl_debug_ats_angles(const rl_scene* scene, uint64_t* n_nodes, float* angles2);      // [node][2] theta_o, theta_e (importance_ray reads the angles)
int rl_debug_camera_ray(const rl_scene* scene, float px, float py, float* origin, float* direction);
}
