// light.hip.h — IntegratorLightTracing (src/integrators/explicit/light.rs): light paths traced from the emitters and splatted onto the image
// through the camera (Camera::sample_direct, camera.rs:94-140).  Instantiated by light_lds.hip (scene staged in LDS) and light_stream.hip
// (BVH streamed from L2 / HBM).  Everything specific to the light tracer lives here: the shared headers are only called, so that no other
// kernel's code or register allocation changes.
//
// Streams.  The jobs are the 16x16 blocks in creation order with the block seeds of rl_render_path; job b traces spp x (pixels of block b)
// light paths, so spp * W * H in all (the reference splits spp * W * H / nb_jobs over 4 x threads jobs and drops the remainder).  Light path
// (block b, slot p, sample s) draws from the sampler that RL_STREAM_PER_SAMPLE gives camera sample (b, pixel p, s): the clone_box fork of the
// block stream, then of the slot stream (k_seed_pixels).  The slot decides nothing about where the path splats.  The reference's job split
// depends on its thread count, so no mode of this port matches it seed for seed: the image agrees in distribution.
//
// Draw order of one light path (evaluation draws nothing): Path::from_light next(), next(), next2d(); the light vertex's
// sample_direction next2d(); the edge's medium draw next() (with a medium); then per expanded vertex the bounce of `path` (next2d(), the
// Russian-roulette next() when rr applies, the medium next()).
//
// Accumulation.  Every splat is added to a per-pixel 96-bit unsigned fixed-point sum per channel: one global 64-bit atomic add per non-zero
// channel into the low word, and when that add carries out of 64 bits (the returned old value plus the addend wraps) one 32-bit atomic add to
// the channel's carry word.  Integer adds commute and every addend is non-negative, so the sum and its carry count do not depend on the order
// in which lanes arrive: same seeds, same bits, in every execution form.  A channel value v becomes rint(v * 2^kLightFixBits); a splat channel
// at or above kLightSplatMax is clamped to it and counted as saturated; a +inf channel sets the pixel's flag bit for that channel (the resolve
// writes +inf there, as the reference's accumulate would) and is counted as saturated too.  A splat with a negative or NaN channel is dropped
// whole (Color::is_valid, structure.rs:156) and counted as invalid.  A channel's sum is exact while it takes fewer than 2^41 clamped splats
// (2^96 / 2^55); no finite splat can make a pixel negative or wrap it.  The resolve writes the f32 of
// (carry * 2^64 + (double)low) * 2^-kLightFixBits / spp, every step in f64.
#pragma once

namespace rl {

static constexpr int kLightFixBits = 24;                      // fraction bits of the splat accumulator: 2^-24 ~ 6e-8 resolution
static constexpr float kLightFixScale = 16777216.0f;          // 2^kLightFixBits
static constexpr float kLightSplatMax = 2147483648.0f;        // 2^31: largest splat channel (2^55 in fixed point)
// statistics rows (pathstate.hip.h: STAT_COUNT = 8) — the light tracer's splat counters take the three free slots
enum { STAT_SPLATS = 5, STAT_SPLATS_INVALID = 6, STAT_SPLATS_SATURATED = 7 };

// Matrix4::transform_point (cgmath): column-major product, then x, y, z times 1 / w
RL_DEV V3 light_xform_point(const float* m, V3 p) {
    const float hx = ((m[0] * p.x + m[4] * p.y) + m[8] * p.z) + m[12];
    const float hy = ((m[1] * p.x + m[5] * p.y) + m[9] * p.z) + m[13];
    const float hz = ((m[2] * p.x + m[6] * p.y) + m[10] * p.z) + m[14];
    const float hw = ((m[3] * p.x + m[7] * p.y) + m[11] * p.z) + m[15];
    const float inv_w = div_rn(1.0f, hw);
    return mk3(hx * inv_w, hy * inv_w, hz * inv_w);
}

// Camera::sample_direct (camera.rs:94-118) + Camera::importance (120-138): false = None; *imp = Color::value(importance) / dist^2, (*px, *py) the pixel
RL_DEV bool light_sample_camera(const DeviceScene& sc, const LightConst& lc, V3 p, Col* imp, int* px, int* py) {
    const V3 ref = light_xform_point(lc.to_local, p);
    if (ref.z < 0.0f) return false;
    const V3 s = light_xform_point(lc.camera_to_sample, ref);
    if (s.x < 0.0f || s.x > 1.0f || s.y < 0.0f || s.y > 1.0f) return false;
    const float sx = s.x * (float)sc.camera.width, sy = s.y * (float)sc.camera.height;
    const float inv_dist = div_rn(1.0f, length(ref));
    const V3 d = ref * inv_dist;
    const float cos_theta = d.z;
    if (cos_theta <= 0.0f) return false;
    const float inv_cos = div_rn(1.0f, cos_theta);
    const float qx = d.x * inv_cos, qy = d.y * inv_cos;
    if (qx < lc.rect_min[0] || qx > lc.rect_max[0] || qy < lc.rect_min[1] || qx > lc.rect_max[1]) return false;    // `p.x > image_rect_max.y` (sic)
    const float size = (lc.rect_max[0] - lc.rect_min[0]) * (lc.rect_max[1] - lc.rect_min[1]);
    const float importance = div_rn(1.0f, size) * inv_cos * inv_cos * inv_cos;
    if (importance == 0.0f) return false;
    *imp = cval(importance) * inv_dist * inv_dist;
    *px = f32_as_i32(sx); *py = f32_as_i32(sy);       // Point2::new(uv.x as i32, uv.y as i32)
    return true;
}

// BufferCollection::accumulate_safe of one splat into the fixed-point image (see the header comment)
RL_DEV void light_splat(const RenderConst& rc, const LightConst& lc, Col c, int px, int py, unsigned& n_add, unsigned& n_invalid, unsigned& n_sat) {
    if (!(c.r >= 0.0f && c.g >= 0.0f && c.b >= 0.0f)) { n_invalid++; return; }       // !Color::is_valid: negative or NaN
    if (px < 0 || py < 0 || px >= (int)rc.W || py >= (int)rc.H) return;                // outside the image: dropped
    n_add++;
    const size_t pix = (size_t)py * rc.W + (size_t)px;
    bool sat = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v = cget(c, k);
        if (v == 0.0f) continue;
        if (v == f32_inf()) { atomicOr(&lc.inf_flags[pix], 1u << k); sat = true; continue; }
        if (v >= kLightSplatMax) { v = kLightSplatMax; sat = true; }
        const unsigned long long q = (unsigned long long)rintf(v * kLightFixScale);
        const unsigned long long old = atomicAdd(lc.accum + 3 * pix + k, q);
        if (old + q < old) atomicAdd(lc.carry + 3 * pix + k, 1u);       // the low word wrapped: carry into the high word
    }
    if (sat) n_sat++;
}

// Mesh::sample_position (emitter.rs:640-644) after the emitter pick: triangle by the mesh's area cdf, point by Mesh::sample_tri
// (geometry.rs:261-337), flux = emit(uv) * PI / pdf_area.  (mesh_sample_triangle folds the direct-sampling tail into the same statements: the
// position and normal below are its own expressions.)
RL_DEV void light_mesh_position(const DeviceScene& sc, const MeshRecord& mr, float r, V2 uv, V3* pos_out, V3* n_out, Col* flux) {
    const unsigned prim = cdf_sample(sc.mesh_cdf + mr.cdf_base, mr.n_tris + 1, r);
    const unsigned gtri = mr.tri_base + prim;
    const unsigned i0 = sc.tri_indices[3 * gtri], i1 = sc.tri_indices[3 * gtri + 1], i2 = sc.tri_indices[3 * gtri + 2];
    const V3 v0 = mk3(sc.positions[3 * i0], sc.positions[3 * i0 + 1], sc.positions[3 * i0 + 2]);
    const V3 v1 = mk3(sc.positions[3 * i1], sc.positions[3 * i1 + 1], sc.positions[3 * i1 + 2]);
    const V3 v2 = mk3(sc.positions[3 * i2], sc.positions[3 * i2 + 1], sc.positions[3 * i2 + 2]);
    const V2 b = uniform_sample_triangle(uv);
    const float w2 = 1.0f - b.x - b.y;
    *pos_out = v0 * b.x + v1 * b.y + v2 * w2;
    V3 n_g = normalize(cross(v2 - v0, v1 - v0));
    if (mr.flags & MESH_HAS_NORMALS) {
        const V3 n0 = mk3(sc.normals[3 * i0], sc.normals[3 * i0 + 1], sc.normals[3 * i0 + 2]);
        const V3 n1 = mk3(sc.normals[3 * i1], sc.normals[3 * i1 + 1], sc.normals[3 * i1 + 2]);
        const V3 n2 = mk3(sc.normals[3 * i2], sc.normals[3 * i2 + 1], sc.normals[3 * i2 + 2]);
        V3 n = n0 * b.x + n1 * b.y + n2 * w2;
        const float nl = length2(n);
        if (nl == 0.0f) n = n_g;
        else if (nl != 1.0f) n = n / sqrt_rn(nl);
        if (dot(n_g, n) < 0.0f) n_g = -n_g;
    }
    *n_out = n_g;
    Col emit;
    if (__builtin_expect(mr.emission_type == 0, 1)) emit = mkc(mr.emission[0], mr.emission[1], mr.emission[2]);
    else emit = mesh_emit_sampled(sc.bitmaps, sc.bitmap_texels, sc.uvs, mr.emission_type, mr.emission_scale, mr.emission_bitmap, (mr.flags & MESH_HAS_UV) != 0, i0, i1, i2, b.x, b.y, w2);
    *flux = div_unguarded(emit * kPi, mr.inv_area);
}

// ------------------------------------------------------------------------------------------
// k_light_fused<MAT, LDS_SCENE, MEDIUM> — rc.split lanes per light-path slot (block b, slot p), each tracing every split-th of its spp light paths
// one after the other (the sum does not depend on which lane adds a splat); per path the
// light vertex is built and splatted, then every vertex is splatted before it is expanded (splat, then bounce).  MAT: the scene's one BSDF
// type, or -1 = run-time switch per vertex (as k_path_fused).  No splat from a smooth BSDF (light.rs:95-97).  Four waves per SIMD (128 VGPRs)
// for both scene kinds: the streaming kernels' six-wave budget of 80 VGPRs spilled ~400 registers here.
static constexpr int kLightWaves = 4;
template <int MAT, bool LDS_SCENE, bool MEDIUM>
__global__ void __launch_bounds__(256, kLightWaves) k_light_fused(RenderConst rc, DeviceScene sc, StackConf stc, LightConst lc) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneRecs recs;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const TravStackT<LDS_SCENE> stack = open_scene<LDS_SCENE>(sc, stc, smem, tid, &recs);
    // rc.split lanes per slot (small images: enough lanes to fill the chip): lane `sub` of the slot traces samples sub, sub + split, ...
    const unsigned item = tid / rc.split, sub = tid - item * rc.split;
    unsigned n_paths = 0, n_draws = 0, n_ext = 0, n_shadow = 0, n_vertices = 0, n_add = 0, n_invalid = 0, n_sat = 0;
    if (item < rc.n_items) {
        const V3 cam = mk3(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        Rng slot_rng = rng_seed(rc.item_seed[item], rc.seed_variant);
        for (unsigned k = 0; k < sub; k++) rng_next_u64(slot_rng);        // the forks of the samples before this lane's first
        for (unsigned s = sub; s < rc.spp; s += rc.split) {
            Rng rng = rng_seed(rng_next_u64(slot_rng), rc.seed_variant);      // the sample's sampler = slot_sampler.clone_box()
            for (unsigned k = 1; k < rc.split; k++) rng_next_u64(slot_rng);   // the forks the slot's other lanes take
            n_paths++;
            // ---- Path::from_light: EmitterSampler::random_sample_emitter_position (emitter.rs:1752-1762)
            const float r_sel = rng_next_f32(rng);
            const float r_pos = rng_next_f32(rng);
            const V2 uv = smp_next2d(rng);
            n_draws += 4;
            const unsigned id = cdf_sample(sc.emitters_cdf, sc.n_emitters + 1, r_sel);
            const float pdf_sel = sc.emitters_cdf[id + 1] - sc.emitters_cdf[id];
            const EmitterRecord em = sc.emitters[id];
            V3 lp, ln; Col flux;
            if (em.kind == EMITTER_MESH) light_mesh_position(sc, sc.meshes[em.mesh], r_pos, uv, &lp, &ln, &flux);
            else if (em.kind == EMITTER_POINT) {                       // PointEmitter::sample_position (emitter.rs:217-229)
                lp = mk3(em.v[0], em.v[1], em.v[2]); ln = mk3(0.0f, 0.0f, 0.0f);
                flux = mkc(em.c[0], em.c[1], em.c[2]) * 4.0f * kPi;
            } else {                                                   // DirectionalLight::sample_position (emitter.rs:135-162)
                const V2 dp = concentric_sample_disk(uv);
                const float area = kPi * powi_f(em.radius, 2);
                const V3 dir = mk3(em.v[0], em.v[1], em.v[2]);
                const V3 poff = to_world(make_frame(dir), mk3(dp.x, dp.y, 0.0f) * em.radius);
                lp = (mk3(em.center[0], em.center[1], em.center[2]) - dir * em.radius) + poff;
                ln = dir;
                flux = mkc(em.c[0], em.c[1], em.c[2]) * area;
            }
            flux = div_unguarded(flux, pdf_sel);                       // w / pdf_sel
            // ---- the light vertex (generate depth 1, evaluate depth 0): expanded only if 1 < max_depth; unexpanded it has no edge and no splat
            if (rc.has_max && !(1u < rc.max_depth)) continue;
            n_vertices++;
            const V2 u2 = smp_next2d(rng);                             // Emitter::sample_direction
            n_draws += 2;
            V3 rd; Col w_edge = cone(); bool solid_angle = true;
            if (em.kind == EMITTER_MESH) {                             // cosine hemisphere around n (emitter.rs:646-664)
                const V3 dl = cosine_sample_hemisphere(u2);
                if (dl.z < 0.0f) w_edge = czero();
                rd = to_world(make_frame(ln), dl);
            } else if (em.kind == EMITTER_POINT) rd = sample_uniform_sphere(u2);
            else { rd = ln; solid_angle = false; }                     // PDF::Discrete
            if (is_zero(w_edge)) continue;                             // throughput zero: no edge (strategies/directional.rs:119-122)
            Col thr = w_edge;
            float xi = 0.0f;
            if (MEDIUM) { xi = rng_next_f32(rng); n_draws++; }         // Edge::from_ray's medium.sample(ray, next())
            const bool acc0 = rc.has_min ? rc.min_depth == 0u : true;
            if (solid_angle && lc.render_surface && acc0) {           // light.rs:128-170
                Col imp; int px, py;
                if (light_sample_camera(sc, lc, lp, &imp, &px, &py)) {
                    const V3 dc = normalize(cam - lp);
                    const Col tr = MEDIUM ? medium_transmittance(sc.medium, length(lp - cam)) : cone();
                    const Col c = (((tr * flux) * imp) * dot(dc, ln)) * kInvPi;
                    n_shadow++;
                    if (shadow_visible(sc, recs, stack, lp, cam)) light_splat(rc, lc, c, px, py, n_add, n_invalid, n_sat);
                }
            }
            // ---- the rest of the path: trace the edge, splat the vertex it reaches, expand it (strategies/mod.rs:35-80).  Per vertex the splat's value
            // is computed first, then the vertex is expanded, then the camera connection is traced: what lives across the two traversals is the
            // path state and one pending splat, not the surface point (evaluation draws nothing, so the draws keep their order).
            V3 ro = lp;
            float rr = 1.0f;
            unsigned gen = 1u;                                         // generate depth of the edge's origin = evaluate depth of the vertex it reaches
            for (;;) {
                n_ext++;
                Hit hit;
                const bool is_hit = trace_closest(sc, recs, stack, ro, rd, hit);
                bool is_volume = false;
                V3 vp = mk3(0.0f, 0.0f, 0.0f);
                if (MEDIUM) {
                    const MediumSample ms = medium_sample(sc.medium, is_hit ? hit.t : kF32Max, xi);
                    w_edge = w_edge * ms.w;
                    is_volume = !is_hit || !ms.exited;
                    if (is_volume) vp = ro + rd * ms.t;
                } else if (!is_hit) break;                             // no next vertex
                flux = (flux * w_edge) * rr;                           // flux * edge.weight * edge.rr_weight
                SurfacePoint sp;
                const Material* mat = nullptr;
                if (!is_volume) {
                    sp = fill_intersection(sc, hit.prim, hit.u, hit.v, ro, rd, hit.t);
                    mat = &sc.materials[sc.meshes[sp.mesh].material];
                    vp = sp.p;
                }
                // ---- the splat's value (light.rs:50-125)
                bool pending = false;
                Col c = czero(); int px = 0, py = 0;
                const bool acc = rc.has_min ? rc.min_depth <= gen : true;
                if (acc && (is_volume ? lc.render_volume : (lc.render_surface && !mat->smooth))) {
                    Col imp;
                    if (light_sample_camera(sc, lc, vp, &imp, &px, &py)) {
                        pending = true;
                        const V3 dc = normalize(cam - vp);
                        const Col tr = MEDIUM ? medium_transmittance(sc.medium, length(vp - cam)) : cone();
                        if (is_volume) c = ((flux * imp) * phase_eval(sc.medium, -rd, dc)) * tr;
                        else {
                            const V3 wo = to_local(sp.frame, dc);
                            const V3 wi_world = to_world(sp.frame, sp.wi);
                            const Col f = bsdf_eval<MAT>(sc, *mat, sp.has_uv, sp.uv, sp.wi, wo, false);
                            const float correction = div_rn(sp.wi.z * dot(dc, sp.n_g), wo.z * dot(wi_world, sp.n_g));   // no abs (light.rs:105-106)
                            c = (((flux * imp) * f) * correction) * tr;
                        }
                    }
                }
                // ---- expand: DirectionalSamplingStrategy::bounce with Transport::Importance (strategies/directional.rs:44-153)
                bool more = false;
                const unsigned gnew = gen + 1u;
                if ((rc.has_max ? gnew < rc.max_depth : true) && gnew < kDepthCap) {
                    n_vertices++;
                    const V2 s2 = smp_next2d(rng);
                    n_draws += 2;
                    V3 nd; Col sw;
                    bool sampled = true;
                    if (is_volume) { float spdf; phase_sample(sc.medium, -rd, s2, &nd, &sw, &spdf); }
                    else {
                        BsdfSample bs;
                        sampled = bsdf_sample<MAT>(sc, *mat, sp.has_uv, sp.uv, sp.wi, s2, &bs);
                        sw = bs.weight; nd = to_world(sp.frame, bs.d);
                    }
                    if (sampled) {
                        thr = thr * sw;
                        if (!is_zero(thr)) {
                            float rr_new = 1.0f;
                            bool alive = true;
                            if (rc.has_rr ? rc.rr_depth <= gnew : true) {
                                const float q = rmin(channel_max(thr), 0.95f);
                                const float x = rng_next_f32(rng);
                                n_draws++;
                                if (q < x) alive = false; else rr_new = div_rn(1.0f, q);
                            }
                            if (alive) {
                                thr = scale_unguarded(thr, rr_new);
                                if (MEDIUM) { xi = rng_next_f32(rng); n_draws++; }
                                more = true;
                                rd = nd; w_edge = sw; rr = rr_new; gen = gnew;
                            }
                        }
                    }
                }
                ro = vp;
                // ---- the camera connection: Acceleration::visible(p, camera)
                if (pending) {
                    n_shadow++;
                    if (shadow_visible(sc, recs, stack, vp, cam)) light_splat(rc, lc, c, px, py, n_add, n_invalid, n_sat);
                }
                if (!more) break;
            }
        }
    }
    {
        const int which[8] = {STAT_SAMPLES, STAT_VERTICES, STAT_DRAWS, STAT_SHADOW_RAYS, STAT_EXT_RAYS, STAT_SPLATS, STAT_SPLATS_INVALID, STAT_SPLATS_SATURATED};
        const unsigned vals[8] = {n_paths, n_vertices, n_draws, n_shadow, n_ext, n_add, n_invalid, n_sat};
        block_stats<8>(rc.partials, which, vals);
    }
}

template <bool LDS_SCENE>
static void launch_light_impl(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const LightConst& lc) {
    with_bsdf(mat, [&](auto M) { with_flag(medium, [&](auto MED) {
        hipLaunchKernelGGL((k_light_fused<decltype(M)::value, LDS_SCENE, decltype(MED)::value>), grid, block, lds_bytes, st, rc, ds, stc, lc);
    }); });
}

}  // namespace rl
