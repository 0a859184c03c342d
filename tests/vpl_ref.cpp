// vpl_ref.cpp — TEST INFRASTRUCTURE: a CPU restatement of IntegratorVPL (src/integrators/explicit/vpl.rs) on the oracle's scene, path graph, BSDF,
// medium and visibility code, which it includes whole.  tests/vpl_ref.py compiles it with the oracle's flags and -fvisibility=hidden (its copy of
// the orc_* symbols stays private) and binds the vref_* entry points with ctypes.
//
// It follows vpl.rs line by line with one deliberate difference, the port's: a camera ray that leaves the scene inside a medium gives +0 without a
// gather (the reference's `l_i *= ..` with l_i = 0, vpl.rs:483).  `literal_miss` = 1 evaluates the reference's own form instead.  Records, counters
// and the sampler come back in the layouts of include/rustlight_amd.h (rl_vpl_read, rl_render_stats).
#include "../oracle/rl_oracle.cpp"

#define VREF_API extern "C" __attribute__((visibility("default")))

namespace orc {
namespace vref {

struct Rec { uint32_t w[RL_VPL_WORDS]; };
static void put3(uint32_t* w, V3 v) { std::memcpy(w, &v.x, 4); std::memcpy(w + 1, &v.y, 4); std::memcpy(w + 2, &v.z, 4); }
static void putc(uint32_t* w, Color c) { std::memcpy(w, &c.r, 4); std::memcpy(w + 1, &c.g, 4); std::memcpy(w + 2, &c.b, 4); }
static float getf(const uint32_t* w) { float f; std::memcpy(&f, w, 4); return f; }
static V3 get3(const uint32_t* w) { return {getf(w), getf(w + 1), getf(w + 2)}; }
static Color getc(const uint32_t* w) { return {getf(w), getf(w + 1), getf(w + 2)}; }

// ---- generation (vpl.rs:182-210)
struct Gen {
    const Scene& scene;
    PathParams prm;
    LightTracer lt;             // Path::from_light's emitter code lives in LightTracer::trace; light_bounce is the light vertex's DirectionalSamplingStrategy
    PathTracer& pt;
    Counters& cnt;
    int option_vpl;
    std::vector<Rec> vpls;
    Gen(const Scene& s, const PathParams& p, int opt) : scene(s), prm(p), lt(s, LightParams{p}), pt(lt.pt), cnt(lt.cnt), option_vpl(opt) {}

    // DirectionalSamplingStrategy { transport: Transport::Radiance }::bounce (directional.rs:44-153) of a surface or volume vertex
    int radiance_sample(int vid, Color& throughput, Sampler& sampler, uint32_t depth) {
        int edge = -1, nv = -1;
        Vertex::Kind kind = pt.path.vertices[vid].kind;
        if (kind == Vertex::Surface) {
            Intersection its = pt.path.vertices[vid].its;
            const BSDF& bsdf = scene.meshes[its.mesh].bsdf;
            SampledDirection sd;
            V2 s2 = sampler.next2d();
            if (!bsdf.sample(its.has_uv, its.uv, its.wi, s2, &sd)) return -1;
            if (bsdf.type == RL_BSDF_GLASS) {          // glass.rs:99-107: transmission scaled by factor * factor under Radiance
                float fres, cos_t;
                fresnel_dielectric(its.wi.z, bsdf.g_eta, &fres, &cos_t);
                if (!(s2.x <= fres)) { float factor = cos_t < 0.0f ? bsdf.g_inv_eta : bsdf.g_eta; sd.weight = sd.weight * factor * factor; }
            }
            V3 d_out_global = its.frame.to_world(sd.d);
            mul_assign(throughput, sd.weight);
            V3 wi_global = its.frame.to_world(its.wi);
            float correction = (its.wi.z * dot(d_out_global, its.n_g)) / (sd.d.z * dot(wi_global, its.n_g));
            throughput.scale(std::fabs(correction));   // *throughput *= correction.abs() (MulAssign<f32>)
            if (throughput.is_zero()) return -1;
            bool do_rr = prm.has_rr ? prm.rr_depth <= depth : true;
            float rr_weight = 1.0f;
            if (do_rr) {
                float q = rmin(throughput.channel_max(), 0.95f);
                if (q < sampler.next()) return -1;
                rr_weight = 1.0f / q;
            }
            throughput.scale(rr_weight);
            Ray ray = {its.p, d_out_global, EPSILON, F32_MAX};
            pt.edge_from_ray(ray, vid, sd.pdf, sd.weight, rr_weight, sampler, 0, &edge, &nv);
        } else if (kind == Vertex::Volume) {
            V3 d_in = pt.path.vertices[vid].d_in, pos = pt.path.vertices[vid].pos;
            V3 d; Color w; float pdf;
            scene.volume.phase_sample(d_in, sampler.next2d(), &d, &w, &pdf);
            mul_assign(throughput, w);
            if (throughput.is_zero()) return -1;
            bool do_rr = prm.has_rr ? prm.rr_depth <= depth : true;
            float rr_weight = 1.0f;
            if (do_rr) {
                float q = rmin(throughput.channel_max(), 0.95f);
                if (q < sampler.next()) return -1;
                rr_weight = 1.0f / q;
            }
            throughput.scale(rr_weight);
            pt.edge_from_ray(Ray::make(pos, d), vid, PDF::solid_angle(pdf), w, rr_weight, sampler, 0, &edge, &nv);
        }
        if (edge >= 0) { Vertex& v = pt.path.vertices[vid]; v.edge_out[v.n_out++] = edge; }
        return nv;
    }
    // paths/strategies/mod.rs:35-80 with TechniqueVPL::expand (vpl.rs:58-60)
    void generate(int root, Sampler& sampler) {
        int curr = root;
        Color thr = Color::one();
        uint32_t depth = 1;
        while (curr >= 0) {
            int next = -1;
            bool expand = prm.has_max ? depth < prm.max_depth : true;
            if (depth >= ORC_DEPTH_CAP) expand = false;
            if (expand) {
                cnt.vertices++;
                Color t = thr;
                int nv = pt.path.vertices[curr].kind == Vertex::Light ? lt.light_bounce(curr, t, sampler) : radiance_sample(curr, t, sampler, depth);
                if (nv >= 0) { next = nv; thr = t; }
            }
            curr = next;
            depth++;
        }
    }
    void push(int kind, V3 p, Color radiance, V3 dir, const Intersection* its) {
        Rec r{};
        r.w[0] = (uint32_t)kind;
        put3(r.w + 4, p); putc(r.w + 7, radiance); put3(r.w + 10, dir);
        if (its) {
            r.w[1] = (uint32_t)its->mesh; r.w[2] = its->has_uv ? 1u : 0u;
            std::memcpy(r.w + 13, &its->uv.x, 4); std::memcpy(r.w + 14, &its->uv.y, 4);
            put3(r.w + 15, its->frame.x); put3(r.w + 18, its->frame.y); put3(r.w + 21, its->frame.z);
        }
        vpls.push_back(r);
    }
    // TechniqueVPL::convert_vpl (vpl.rs:67-162)
    void convert(int vid, Color flux) {
        const Vertex& v = pt.path.vertices[vid];
        if (v.kind == Vertex::Surface) {
            if (option_vpl != RL_VPL_VOLUME && !scene.meshes[v.its.mesh].bsdf.is_smooth()) push(RL_VPL_KIND_SURFACE, v.its.p, flux, v.its.wi, &v.its);
        } else if (v.kind == Vertex::Volume) {
            if (option_vpl != RL_VPL_SURFACE) push(RL_VPL_KIND_VOLUME, v.pos, flux, v.d_in, nullptr);
        } else if (v.kind == Vertex::Light) {
            if (option_vpl != RL_VPL_VOLUME) {
                if (v.n_out == 0) std::abort();          // edge_out.unwrap() (vpl.rs:138): max_depth <= 1 is refused before this
                const Edge& e = pt.path.edges[v.edge_out[0]];
                if (e.pdf_direction.kind == PDF::Discrete) push(RL_VPL_KIND_EMITTER_INFINITE, e.d, flux, v3(0, 0, 0), nullptr);
                else push(RL_VPL_KIND_EMITTER_POSITION, v.pos, flux, v.n, nullptr);
            }
        } else return;
        for (int k = 0; k < pt.path.vertices[vid].n_out; k++) {
            const Edge& e = pt.path.edges[pt.path.vertices[vid].edge_out[k]];
            if (e.v1 < 0) continue;
            Color f = pt.path.vertices[vid].kind == Vertex::Light ? e.weight * flux * e.rr_weight : flux * e.weight * e.rr_weight;
            convert(e.v1, f);
        }
    }
    // one light path: Path::from_light, generate, convert_vpl (vpl.rs:199-203)
    void shoot(Sampler& sampler) {
        pt.path.clear();
        float v1 = sampler.next();
        float v2 = sampler.next();
        V2 uv = sampler.next2d();
        size_t id = scene.emitters_cdf.sample_discrete(v1);
        float pdf_sel = scene.emitters_cdf.pdf(id);
        const EmitterRec& em = scene.emitters[id];
        Vertex lv; lv.kind = Vertex::Light; lv.emitter = (int)id;
        Color w;
        if (em.kind == EM_MESH) {
            const Mesh& m = scene.meshes[em.mesh];
            Mesh::SampledPosition sp = m.sample(v2, uv);
            lv.pos = sp.p; lv.n = sp.n; lv.its.has_uv = sp.has_uv; lv.its.uv = sp.uv;
            w = m.emit(sp.has_uv, sp.uv) * PI_F / sp.pdf.value();
        } else if (em.kind == EM_POINT) {
            lv.pos = em.v; lv.n = {0, 0, 0};
            w = em.c * 4.0f * PI_F;
        } else {
            V2 p = concentric_sample_disk(uv);
            float area = PI_F * powi(em.bsphere.radius, 2);
            V3 poff = Frame::make(em.v).to_world(v3(p.x, p.y, 0.0f) * em.bsphere.radius);
            lv.pos = (em.bsphere.center - em.v * em.bsphere.radius) + poff;
            lv.n = em.v;
            w = em.c * area;
        }
        Color flux = w / pdf_sel;
        pt.path.vertices.push_back(lv);
        generate(0, sampler);
        convert(0, flux);
    }
};

// ---- gather (vpl.rs:212-535)
struct Gather {
    const Scene& scene;
    const uint32_t* vpls;
    size_t n_vpl;
    float norm_vpl;
    int option_lt;
    bool literal_miss;
    uint64_t shadow = 0, on_surface = 0, in_volume = 0;

    Color transmittance(V3 p1, V3 p2) const { return scene.has_volume ? scene.volume.transmittance(magnitude(p2 - p1)) : Color::one(); }

    Color gathering_surface(const Intersection& its) {
        on_surface++;
        Color l_i = Color::zero();
        const Mesh& mesh = scene.meshes[its.mesh];
        if (its.wi.z > 0.0f) add_assign(l_i, mesh.emit(its.has_uv, its.uv));       // self emission (vpl.rs:279)
        if (mesh.bsdf.is_smooth()) return l_i;        // every VPL adds nothing here: its visibility ray is not traced
        for (size_t i = 0; i < n_vpl; i++) {
            const uint32_t* r = vpls + i * RL_VPL_WORDS;
            const V3 vpos = get3(r + 4), v3_ = get3(r + 10);
            const Color rad = getc(r + 7);
            switch (r[0]) {
                case RL_VPL_KIND_EMITTER_POSITION: {
                    shadow++;
                    if (scene.visible(vpos, its.p)) {
                        V3 d = vpos - its.p;
                        float dist = magnitude(d);
                        d = d / dist;
                        Color emitted = rad * rmax(dot(v3_, -d), 0.0f) * FRAC_1_PI;
                        Color bsdf_val = mesh.bsdf.eval(its.has_uv, its.uv, its.wi, its.frame.to_local(d), DomSolidAngle);
                        Color trans = transmittance(its.p, vpos);
                        add_assign(l_i, trans * norm_vpl * emitted * bsdf_val / (dist * dist));
                    }
                    break;
                }
                case RL_VPL_KIND_EMITTER_INFINITE: {
                    shadow++;
                    Intersection hit;
                    if (!scene.trace(Ray::make(its.p, -vpos), &hit)) {            // Ray::spawn_ray(&its, -d)
                        Color bsdf_val = mesh.bsdf.eval(its.has_uv, its.uv, its.wi, its.frame.to_local(-vpos), DomSolidAngle);
                        add_assign(l_i, norm_vpl * rad * bsdf_val);
                    }
                    break;
                }
                case RL_VPL_KIND_VOLUME: {                   // no visibility test (vpl.rs:333)
                    V3 d = vpos - its.p;
                    float dist = magnitude(d);
                    d = d / dist;
                    Color emitted = scene.volume.phase_eval(v3_, d);
                    Color bsdf_val = mesh.bsdf.eval(its.has_uv, its.uv, its.wi, its.frame.to_local(d), DomSolidAngle);
                    Color trans = transmittance(its.p, vpos);
                    add_assign(l_i, trans * norm_vpl * emitted * bsdf_val * rad / (dist * dist));
                    break;
                }
                default: {
                    shadow++;
                    if (scene.visible(vpos, its.p)) {
                        V3 d = vpos - its.p;
                        float dist = magnitude(d);
                        d = d / dist;
                        Frame fr{get3(r + 15), get3(r + 18), get3(r + 21)};
                        const BSDF& vb = scene.meshes[r[1]].bsdf;
                        Color emitted = vb.eval(r[2] != 0, V2{getf(r + 13), getf(r + 14)}, v3_, fr.to_local(-d), DomSolidAngle);
                        Color bsdf_val = mesh.bsdf.eval(its.has_uv, its.uv, its.wi, its.frame.to_local(d), DomSolidAngle);
                        Color trans = transmittance(its.p, vpos);
                        add_assign(l_i, trans * norm_vpl * emitted * bsdf_val * rad / (dist * dist));
                    }
                }
            }
        }
        return l_i;
    }

    Color gathering_volume(V3 d_cam, V3 its_pos) {
        in_volume++;
        Color l_i = Color::zero();
        for (size_t i = 0; i < n_vpl; i++) {
            const uint32_t* r = vpls + i * RL_VPL_WORDS;
            const V3 vpos = get3(r + 4), v3_ = get3(r + 10);
            const Color rad = getc(r + 7);
            switch (r[0]) {
                case RL_VPL_KIND_EMITTER_POSITION: {
                    shadow++;
                    if (scene.visible(vpos, its_pos)) {
                        V3 d = vpos - its_pos;
                        float dist = magnitude(d);
                        d = d / dist;
                        Color emitted = rad * rmax(dot(v3_, -d), 0.0f) * FRAC_1_PI;
                        Color phase_val = scene.volume.phase_eval(d_cam, d);
                        Color trans = transmittance(vpos, its_pos);
                        add_assign(l_i, trans * norm_vpl * emitted * phase_val / (dist * dist));
                    }
                    break;
                }
                case RL_VPL_KIND_EMITTER_INFINITE: std::abort();     // assert!(medium.is_none()) (vpl.rs:418): refused before this
                case RL_VPL_KIND_VOLUME: {                   // no visibility test (vpl.rs:426)
                    V3 d = vpos - its_pos;
                    float dist = magnitude(d);
                    d = d / dist;
                    Color emitted = scene.volume.phase_eval(v3_, d);
                    Color phase_val = scene.volume.phase_eval(d_cam, d);
                    Color trans = transmittance(its_pos, vpos);
                    add_assign(l_i, trans * norm_vpl * emitted * phase_val * rad / (dist * dist));
                    break;
                }
                default: {
                    shadow++;
                    if (scene.visible(vpos, its_pos)) {
                        V3 d = vpos - its_pos;
                        float dist = magnitude(d);
                        d = d / dist;
                        Frame fr{get3(r + 15), get3(r + 18), get3(r + 21)};
                        const BSDF& vb = scene.meshes[r[1]].bsdf;
                        Color emitted = vb.eval(r[2] != 0, V2{getf(r + 13), getf(r + 14)}, v3_, fr.to_local(-d), DomSolidAngle);
                        Color phase_val = scene.volume.phase_eval(d_cam, d);
                        Color trans = transmittance(its_pos, vpos);
                        add_assign(l_i, trans * norm_vpl * emitted * phase_val * rad / (dist * dist));
                    }
                }
            }
        }
        return l_i;
    }

    // compute_vpl_contrib (vpl.rs:444-535)
    Color contrib(uint32_t ix, uint32_t iy, Sampler& sampler) {
        V2 pix{(float)ix + sampler.next(), (float)iy + sampler.next()};
        Ray ray = scene.camera.generate(pix);
        Color l_i = Color::zero();
        Intersection its;
        if (!scene.trace(ray, &its)) {
            if (scene.has_volume) {
                SampledDistance mrec = scene.volume.sample(ray, sampler.next());
                if (mrec.exited) std::abort();
                if (!literal_miss) return l_i;          // the port's +0 (see the header)
                V3 pos = ray.o + ray.d * mrec.t;
                mul_assign(l_i, gathering_volume(-ray.d, pos) * mrec.w);
                return l_i;
            }
            return l_i;                                 // (environment emitters are refused)
        }
        if (scene.has_volume) {
            Ray ray_med = ray;
            ray_med.tfar = its.dist;
            SampledDistance mrec = scene.volume.sample(ray_med, sampler.next());
            if (!mrec.exited) {
                V3 pos = ray.o + ray.d * mrec.t;
                add_assign(l_i, gathering_volume(-ray.d, pos) * mrec.w);
            } else if (option_lt != RL_VPL_VOLUME) {
                add_assign(l_i, gathering_surface(its) * mrec.w);
            }
            return l_i;
        }
        if (option_lt != RL_VPL_SURFACE) add_assign(l_i, gathering_surface(its));     // the inverted test (vpl.rs:527)
        return l_i;
    }
};

}  // namespace vref
}  // namespace orc

using namespace orc;

// the scene, as the oracle builds it
VREF_API orc_scene* vref_scene_create(void) { return orc_scene_create(); }
VREF_API void vref_scene_destroy(orc_scene* s) { orc_scene_destroy(s); }
VREF_API int vref_scene_set_camera(orc_scene* sc, uint32_t w, uint32_t h, float fov, int fov_axis, const float* to_world, int flip) { return orc_scene_set_camera(sc, w, h, fov, fov_axis, to_world, flip); }
VREF_API int vref_scene_add_bitmap(orc_scene* sc, uint32_t w, uint32_t h, const float* rgb) { return orc_scene_add_bitmap(sc, w, h, rgb); }
VREF_API int vref_scene_add_mesh(orc_scene* sc, const float* vertices, size_t nv, const uint32_t* indices, size_t ntri, const float* normals, const float* uvs,
                                 const rl_bsdf_desc* bsdf, const float* emission) { return orc_scene_add_mesh(sc, vertices, nv, indices, ntri, normals, uvs, bsdf, emission); }
VREF_API int vref_scene_set_mesh_emission(orc_scene* sc, int mesh, int type, float scale, int bitmap_id) { return orc_scene_set_mesh_emission(sc, mesh, type, scale, bitmap_id); }
VREF_API int vref_scene_set_medium(orc_scene* sc, const float* sigma_a, const float* sigma_s, int phase, float g) { return orc_scene_set_medium(sc, sigma_a, sigma_s, phase, g); }
VREF_API int vref_scene_add_point_light(orc_scene* sc, const float* p, const float* i) { return orc_scene_add_point_light(sc, p, i); }
VREF_API int vref_scene_add_directional_light(orc_scene* sc, const float* d, const float* i) { return orc_scene_add_directional_light(sc, d, i); }
VREF_API int vref_scene_build(orc_scene* sc) { return orc_scene_build(sc); }

// IntegratorVPL's generation from the main sampler `state` (advanced in place).  counts = [VPLs, paths, vertices, extension rays, draws].  Returns the
// number of VPLs, or -1 when `cap` records do not hold them or RL_VPL_MAX_PATHS paths store fewer than nb_vpl.
VREF_API long vref_generate(const orc_scene* sc, int has_max, uint32_t max_depth, int has_rr, uint32_t rr_depth, uint32_t nb_vpl, int option_vpl,
                            uint64_t* state, uint32_t* words, size_t cap, uint64_t* counts) {
    PathParams p;
    p.has_max = has_max != 0; p.max_depth = max_depth;
    p.has_rr = has_rr != 0; p.rr_depth = rr_depth;
    vref::Gen gen(sc->s, p, option_vpl);
    Sampler sm;
    std::memcpy(sm.rnd.s, state, 32);
    uint64_t paths = 0;
    while (gen.vpls.size() < nb_vpl) {
        if (paths == RL_VPL_MAX_PATHS) return -1;
        gen.shoot(sm);
        paths++;
    }
    if (gen.vpls.size() > cap) return -1;
    std::memcpy(state, sm.rnd.s, 32);
    for (size_t i = 0; i < gen.vpls.size(); i++) std::memcpy(words + i * RL_VPL_WORDS, gen.vpls[i].w, sizeof(gen.vpls[i].w));
    counts[0] = gen.vpls.size(); counts[1] = paths; counts[2] = gen.cnt.vertices; counts[3] = gen.cnt.extension_rays; counts[4] = sm.draws;
    return (long)gen.vpls.size();
}

// The gather over the blocks b % shard_count == shard_index (others stay 0).  counts = [camera samples, extension rays, shadow rays, draws,
// gather points on surfaces, gather points in the medium].
VREF_API int vref_render(const orc_scene* sc, const uint32_t* words, uint64_t n_vpl, uint64_t n_paths, int option_lt, const uint64_t* block_seeds,
                         size_t n_blocks, uint32_t spp, int seed_variant, uint32_t shard_index, uint32_t shard_count, int literal_miss, float* out_rgb,
                         uint64_t* counts) {
    const Scene& scene = sc->s;
    const uint32_t W = scene.camera.w, H = scene.camera.h;
    const size_t nby = (H + 15) / 16;
    if (n_blocks != ((W + 15) / 16) * nby || spp == 0 || shard_count == 0) return -1;
    vref::Gather g{scene, words, (size_t)n_vpl, 1.0f / (float)n_paths, option_lt, literal_miss != 0};
    uint64_t samples = 0, draws = 0;
    const float inv_spp = 1.0f / (float)spp;
    std::memset(out_rgb, 0, sizeof(float) * 3 * W * H);
    for (size_t b = 0; b < n_blocks; b++) {
        if (b % shard_count != shard_index) continue;
        uint32_t bx = (uint32_t)(b / nby) * 16, by = (uint32_t)(b % nby) * 16;
        uint32_t bw = std::min(16u, W - bx), bh = std::min(16u, H - by);
        Sampler sm; sm.rnd = Rng::seed_from_u64(block_seeds[b], seed_variant); sm.variant = seed_variant;
        for (uint32_t ix = 0; ix < bw; ix++)
            for (uint32_t iy = 0; iy < bh; iy++) {
                Color acc = Color::zero();
                for (uint32_t s = 0; s < spp; s++) { add_assign(acc, g.contrib(bx + ix, by + iy, sm)); samples++; }
                acc.scale(inv_spp);                     // im_block.scale(1 / spp)
                float* o = out_rgb + 3 * ((size_t)(by + iy) * W + bx + ix);
                o[0] = acc.r; o[1] = acc.g; o[2] = acc.b;
            }
        draws += sm.draws;
    }
    counts[0] = samples; counts[1] = samples; counts[2] = g.shadow; counts[3] = draws; counts[4] = g.on_surface; counts[5] = g.in_volume;
    return 0;
}
