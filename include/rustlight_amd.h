/*
 * rustlight_amd.h — C-ABI of the MI355X-native drop-in for rustlight's `path` integrator.
 *
 * Everything here is plain C: POD structs, pointers and sizes.  No torch / HIP / C++ types
 * cross this boundary.  Each entry point cites the rustlight interface it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the Rust `extern "C"` block
 * and the `impl Integrator for ...` a rustlight maintainer would add on top of this header.
 *
 * Conventions
 *   - all functions return RL_OK (0) or a negative rl_status; they never throw or abort
 *     (the reference panics instead: src/scene_loader.rs:34, examples/cli.rs:36,348);
 *   - vectors are tightly packed f32 triples, matrices are column-major 4x4 f32 (cgmath);
 *   - colours are linear RGB f32 triples (src/structure.rs:105-110);
 *   - images are row-major, origin top-left, W*H*3 f32 (src/structure.rs:383-402).
 *
 * Execution options.  None of them changes a result; they exist for the tests and for measurements and are NOT part of the
 * drop-in surface.  rl_context_create copies them ONCE from the process environment (RL_<NAME>) into the context; afterwards
 * rl_context_set_option(ctx, "<name>", value) changes them per context, and no render entry point ever reads the environment
 * (a render works on the copy of the table it took when it started).  The full list is rustlight_amd/csrc/kernels/knobs.h; the ones the tests use:
 *   force_streaming = 1       (creation time: environment RL_FORCE_STREAMING only) keep small scenes out of LDS — the kernels that stream the BVH
 *                             from L2 / HBM on scenes the oracle finishes in seconds
 *   generic_lights = 1        (creation time: RL_GENERIC_LIGHTS) do not specialise the NEE code for area-light-only scenes
 *   item_shift = k            reference-order streams: one block chain per 2^k lanes
 *   ref_single_pass = 1       reference-order streams through the persistent kernel in ONE pass (the form of rounds 1-2) instead of
 *                             chain pass + per-sample evaluation
 *   chain_serial = 1          the chain pass by k_stream_chain (one lane per block) instead of k_stream_spec; spec_force = 1: the opposite
 *   spec_draws_per_sample = x the draws a camera sample takes on this scene (the choice between the two chain kernels; default 150 with a medium, 12 without —
 *                             rl_render_stats.rng_draws / camera_samples of an earlier render is the measured figure)
 *   chain_no_pre = 1, chain_no_treelets = 1     k_stream_chain without its lane-parallel records / treelet blocks
 *   no_overlap = 1            the evaluation pass after the chain pass instead of beside it
 *   state_budget_mb = n       MB the recorded sampler states of the two-pass form may take (default 24 GB): small values force several chunks
 *   fused_dynamic = 0|1       persistent kernel: static tile order / work items from the atomic dispenser
 *   fused_tail_blocks = T, fused_tail_split = S     persistent kernel, per-sample streams in static tile order on an LDS-staged scene without a medium: the last T
 *                             blocks that see the scene run at S lanes per pixel (S a power of two), their samples parked and folded in sample order (0: off)
 *   shadow_pack_capacity = n  the shadow stage of the kernel with a tail: the wave tests its candidate leaves whenever a lane holds n of them (tests; 0: the stack decides)
 *   no_events = 1             no HIP events around the kernels (rl_render_stats.ms_* stay 0)
 *   vpl_batch_paths = n       rl_vpl_generate_paths: every batch of a generation holds n light paths (default: sized from the records per path measured so far)
 * rl_multi_* reads RL_MULTI_FORCE_HOST_MERGE=1, RL_MULTI_NO_FALLBACK=1, RL_MULTI_REDUCE_TIMEOUT_S=s when the communicator is built / a reduce runs: see rl_multi_describe.
 */
#ifndef RUSTLIGHT_AMD_H
#define RUSTLIGHT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rl_status {
    RL_OK = 0,
    RL_ERR_INVALID_ARGUMENT = -1,
    RL_ERR_NO_DEVICE = -2,       /* HIP runtime / GPU missing: the product path never falls back to CPU */
    RL_ERR_HIP = -3,             /* a HIP call failed; see rl_last_error() */
    RL_ERR_NOT_BUILT = -4,       /* scene used before rl_scene_build_emitters() */
    RL_ERR_IO = -5,
    RL_ERR_PARSE = -6,
    RL_ERR_UNSUPPORTED = -7,
    RL_ERR_NO_EMITTER = -8       /* NEE requested on a scene without emitters (reference: warn + crash, src/scene.rs:96-99) */
} rl_status;

/* ---------------------------------------------------------------- materials ------------- */

/* BSDFColor (src/bsdfs/mod.rs:11-29) */
typedef enum rl_tex_type {
    RL_TEX_CONSTANT = 0,
    RL_TEX_CHECKERBOARD = 1,
    RL_TEX_GRID = 2,
    RL_TEX_BITMAP = 3
} rl_tex_type;

typedef struct rl_color_desc {
    int32_t type;          /* rl_tex_type */
    float color0[3];       /* Constant colour / checker+grid colour 0 */
    float color1[3];
    float offset[2];
    float scale[2];
    float line_width;      /* grid only */
    int32_t bitmap_id;     /* RL_TEX_BITMAP: id returned by rl_scene_add_bitmap */
} rl_color_desc;

/* concrete `impl BSDF` types (src/bsdfs/{diffuse,phong,metal,glass,substrate}.rs) */
typedef enum rl_bsdf_type {
    RL_BSDF_DIFFUSE = 0,
    RL_BSDF_PHONG = 1,
    RL_BSDF_METAL = 2,
    RL_BSDF_GLASS = 3,
    RL_BSDF_SUBSTRATE = 4
} rl_bsdf_type;

/* MicrofacetType (src/bsdfs/distribution.rs:13-17); 0 = `distribution: None` */
typedef enum rl_microfacet_type {
    RL_MICROFACET_NONE = 0,
    RL_MICROFACET_BECKMANN = 1,
    RL_MICROFACET_GGX = 2
} rl_microfacet_type;

typedef struct rl_bsdf_desc {
    int32_t type;                 /* rl_bsdf_type */
    rl_color_desc diffuse;        /* Diffuse.diffuse, Phong.diffuse, Substrate.diffuse */
    rl_color_desc specular;       /* Phong.specular, Metal.specular, Substrate.specular, Glass.specular_reflectance */
    rl_color_desc transmittance;  /* Glass.specular_transmittance */
    rl_color_desc eta;            /* Metal.eta */
    rl_color_desc k;              /* Metal.k */
    float exponent;               /* Phong.exponent */
    float weight_specular;        /* Phong.weight_specular */
    int32_t distribution;         /* one of rl_microfacet_type; Metal and Substrate only */
    float alpha_u, alpha_v;
    float glass_eta;              /* BSDFGlass.eta = int_ior / ext_ior (src/bsdfs/glass.rs:44-49) */
} rl_bsdf_desc;

/* PhaseFunction (src/volume.rs:12-16) */
typedef enum rl_phase_type { RL_PHASE_ISOTROPIC = 0, RL_PHASE_HG = 1 } rl_phase_type;

/* ---------------------------------------------------------------- scene ----------------- */

/* Opaque host-side scene: the flattened counterpart of `struct Scene` (src/scene.rs:16-30). */
typedef struct rl_scene rl_scene;

/* Scene { .. } literal (src/scene_loader.rs:302-312): empty scene, nb_samples = 1. */
int rl_scene_create(rl_scene** out);
void rl_scene_destroy(rl_scene* scene);

/* Camera::new(img, fov, mat, flip) (src/camera.rs:31-67).
 * fov_axis: 0 = Fov::X, 1 = Fov::Y (the reference multiplies Fov::Y by the aspect ratio, camera.rs:41-44).
 * to_world: column-major camera-to-world matrix.  flip: true for the Mitsuba loader, false for PBRT. */
int rl_scene_set_camera(rl_scene* scene, uint32_t width, uint32_t height, float fov_degrees,
                        int fov_axis, const float to_world[16], int flip);

/* The camera as rustlight ALREADY HOLDS it (SURVEY.md 8(b) SceneDesc: `sample_to_camera[16], to_world[16]`): the two matrices Camera::generate reads
 * (src/camera.rs:81-91: `sample_to_camera.transform_point(px / img)`, `to_world.transform_vector(d)`, position = to_world * origin, camera.rs:140-142),
 * column-major as cgmath stores them (`let m: &[f32; 16] = camera.sample_to_camera.as_ref()`).  This is the entry a Rust host should use: nothing of
 * Camera::new (cgmath's `perspective`, `inverse_transform`, the Fov::Y x aspect rule — camera.rs:31-67) is re-derived on this side, so the rays are
 * rustlight's own by construction.  The two fields are private in rustlight: the host-side patch adds two accessors.
 * rl_scene_set_camera (below, fov / flip: what the scene FILES carry) stays for the loaders and derives the same two matrices itself. */
int rl_scene_set_camera_matrices(rl_scene* scene, uint32_t width, uint32_t height, const float sample_to_camera[16], const float to_world[16]);
/* The matrices the scene's camera uses (whichever call set it): sample_to_camera, to_world (column-major), and Camera::position. */
int rl_scene_get_camera_matrices(const rl_scene* scene, float sample_to_camera[16], float to_world[16], float position[3]);

/* EmissionType (src/geometry.rs:99-104) of a light mesh: the constant colour rl_scene_add_mesh gave it, or one of the two uv-dependent kinds
 * Mesh::emit evaluates (geometry.rs:184-206): HSV { scale } = scale * (x, 1 - x, 0) with x = |uv.x| % 1, Texture { scale, img } = scale * img.pixel_uv(uv).
 * The mesh must be a light and — for the two uv-dependent kinds — carry uv coordinates (the reference's `uv.unwrap()` panics otherwise).
 * Emitter::flux takes Color::value(scale) for them (emitter.rs:591-599).  Call before rl_scene_build_emitters. */
typedef enum rl_emission_type { RL_EMISSION_COLOR = 0, RL_EMISSION_HSV = 1, RL_EMISSION_TEXTURE = 2 } rl_emission_type;
int rl_scene_set_mesh_emission(rl_scene* scene, uint32_t mesh, int type, float scale, int bitmap_id);
/* The CLI's `-x hvs-light` / `-x texture-light` (examples/cli.rs:410-429): EVERY light mesh becomes HSV { scale } / Texture { scale, img = bitmap_id } with
 * scale = Color::luminance of its colour (1 if it already was uv-dependent).  `type`: RL_EMISSION_HSV or RL_EMISSION_TEXTURE. */
int rl_scene_override_light_emission(rl_scene* scene, int type, int bitmap_id);

/* Camera::scale_image (src/camera.rs:73-78), the CLI's -s flag. */
int rl_scene_scale_image(rl_scene* scene, float scale);

/* Mesh::new(name, vertices, indices, normals, uv) + `.bsdf = ...` + `.emission = EmissionType::Color`
 * (src/geometry.rs:122-182, src/scene_loader.rs:134-150).  normals / uv / emission may be NULL.
 * Returns the mesh index (>= 0) or a negative rl_status.  Meshes keep insertion order
 * (it fixes the emitter order, src/scene.rs:64-69, and the BVH primitive order, src/accel.rs:206-219). */
int rl_scene_add_mesh(rl_scene* scene, const float* vertices, size_t n_vertices,
                      const uint32_t* indices, size_t n_triangles, const float* normals,
                      const float* uv, const rl_bsdf_desc* bsdf, const float* emission_rgb);

/* Bitmap used by BSDFColor::Bitmap (src/bsdfs/mod.rs:13-15): row-major W*H*3 f32.  Returns its id. */
int rl_scene_add_bitmap(rl_scene* scene, uint32_t width, uint32_t height, const float* rgb);

/* scene.volume = Some(HomogenousVolume{..}) — the CLI's `-m sigma_s[:sigma_a[:g]]` (examples/cli.rs:355-399).
 * sigma_t = sigma_a + sigma_s is formed here exactly as cli.rs:383-385 does. */
int rl_scene_set_medium(rl_scene* scene, const float sigma_a[3], const float sigma_s[3],
                        int phase_type, float g);

/* Non-mesh emitters (`EmittersState::Unbuild`, src/scene_loader.rs:177-204): PointEmitter { intensity, position }
 * (src/emitter.rs:183-250) and DirectionalLight { direction, intensity } (src/emitter.rs:96-181), kept in
 * insertion order after the emissive meshes and the environment. */
int rl_scene_add_point_light(rl_scene* scene, const float position[3], const float intensity[3]);
int rl_scene_add_directional_light(rl_scene* scene, const float direction[3], const float intensity[3]);
/* scene.emitter_environment = EnvironmentLight { luminance: EnvironmentLightColor::Constant(rgb) }
 * (src/emitter.rs:300-568, src/scene_loader.rs:205-224).  Not combinable with a medium (the reference
 * asserts, src/paths/edge.rs:94). */
int rl_scene_set_environment(rl_scene* scene, const float rgb[3]);
/* EnvironmentLightColor::Texture { image, image_cdf } = EnvironmentLightColor::new_texture(image) (src/emitter.rs:340-353,
 * src/scene_loader.rs:259-271): lat-long image, z up, w x h RGB f32 row-major (row 0 = theta 0), importance sampled by
 * luminance x sin(theta) through a Distribution2D (src/math.rs:489-532); nearest-texel lookups as in the reference. */
int rl_scene_set_environment_map(rl_scene* scene, uint32_t w, uint32_t h, const float* rgb);

/* Scene::build_emitters(false) (src/scene.rs:53-123): scene bounding sphere, emitter list
 * (emissive meshes in mesh order), CDF over flux().channel_max().  The ATS light tree
 * (`-x ats`) is out of scope. */
int rl_scene_build_emitters(rl_scene* scene);
/* The `build_ats` argument of Scene::build_emitters (src/scene.rs:53,118-120; CLI `-x ats`): when set, the next
 * rl_scene_build_emitters() also builds the LightSamplerATS light tree over the emissive triangles (src/emitter.rs:1117-1292)
 * and light sampling / its MIS pdf descend that tree (importance_point, emitter.rs:1024-1086) instead of the flux cdf.
 * Every emitter must then be an emissive mesh (the reference asserts is_surface()). */
int rl_scene_enable_ats(rl_scene* scene, int build_ats);

/* SceneLoaderManager::load(path, use_shading_normals) for the `.pbrt` subset the reference's
 * PBRT loader consumes (src/scene_loader.rs:77-315): Transform/LookAt/Camera perspective/Film,
 * MakeNamedMaterial matte|..., NamedMaterial, Shape trianglemesh, AreaLightSource diffuse. */
int rl_scene_load_pbrt(const char* path, int use_shading_normals, rl_scene** out);
/* MTSSceneLoader::load (src/scene_loader.rs:318-795): the Mitsuba 0.5/0.6 XML subset the reference consumes — one perspective
 * sensor (flip = true), shapes obj | ply | serialized | rectangle | sphere with bsdf / area emitter / toWorld, bsdf_mts
 * materials (src/bsdfs/mod.rs:499-612), point emitters, the first homogeneous medium.  Needs rl_scene_build_emitters(). */
int rl_scene_load_mitsuba(const char* path, int use_shading_normals, rl_scene** out);
/* SceneLoaderManager::load (src/scene_loader.rs:27-58): picks the loader by extension (.pbrt | .xml). */
int rl_scene_load(const char* path, int use_shading_normals, rl_scene** out);

int rl_scene_image_size(const rl_scene* scene, uint32_t* width, uint32_t* height);
int rl_scene_counts(const rl_scene* scene, uint64_t* n_meshes, uint64_t* n_triangles,
                    uint64_t* n_emitters);

/* ---------------------------------------------------------------- sampler --------------- */

/* IndependentSampler (src/samplers/independent.rs:5-34) over rand 0.8.5 SmallRng = Xoshiro256++.
 * The reference trait object hides the raw u64 stream, so the drop-in owns the concrete sampler. */
typedef struct rl_sampler {
    uint64_t s[4];
} rl_sampler;

/* SmallRng::seed_from_u64(seed) as the CLI's `-r independent:SEED` does (examples/cli.rs:886-890).
 * variant 0 = rand_core 0.6.4 default (PCG32 fill), 1 = SplitMix64 (see oracle header for why both). */
void rl_sampler_seed(rl_sampler* sampler, uint64_t seed, int variant);
uint64_t rl_sampler_next_u64(rl_sampler* sampler);
/* Sampler::next() (samplers/independent.rs:9-11): rng.gen::<f32>() */
float rl_sampler_next_f32(rl_sampler* sampler);

/* ---------------------------------------------------------------- integrator ------------ */

/* IntegratorPathTracingStrategies (src/integrators/explicit/path.rs:9-13) */
typedef enum rl_path_strategy { RL_STRATEGY_ALL = 0, RL_STRATEGY_BSDF = 1, RL_STRATEGY_EMITTER = 2 } rl_path_strategy;

/* How the per-block random stream is mapped onto GPU lanes:
 *  RL_STREAM_REFERENCE_ORDER: one serial stream per 16x16 block, consumed over (iy, ix, sample)
 *      exactly as compute_mc does (src/integrators/mod.rs:420-435) — equals rustlight proper.  Runs in two passes on the
 *      GPU: a draw-count walk of every block's stream records the sampler state at the start of each camera sample (what is
 *      serial is only how many numbers a sample takes; since round 4 that walk is speculative: per-pixel windows of the block's stream walked by
 *      every lane, the true chain threaded through them), then all samples are evaluated in parallel from those states; 5x
 *      slower than RL_STREAM_PER_SAMPLE on the Cornell box at 1080p x 128 spp, same image and counters as the one-lane-per-block walk.
 *  RL_STREAM_PER_SAMPLE: the block stream is forked with the reference's own clone_box rule
 *      (samplers/independent.rs:18-22) once per pixel and once per sample — throughput mode.
 *  RL_STREAM_STRATIFIED: rustlight's StratifiedSampler (samplers/stratified.rs, CLI `-r stratified`) on the forks of RL_STREAM_PER_SAMPLE:
 *      n = the power of four >= spp; the first 4 next() of a camera sample each take a stratum of [0, 1) in n, the first 4 next2d()
 *      each a cell of a sqrt(n) x sqrt(n) grid, every dimension's strata dealt to the pixel's samples by its own keyed permutation
 *      (with spp < n only the first spp of them); later draws come from the sample's sampler.  Deterministic given the block
 *      seeds (and seed_variant): the image does not depend on pipeline, split, sharding, frames in flight or the number of GPUs.
 *      The reference seeds its arrays from random(): statistically the same sampler, not seed-for-seed equivalent.  spp <= 2^30;
 *      not with numerics = RL_NUMERICS_FAST (RL_ERR_UNSUPPORTED). */
typedef enum rl_stream_mode { RL_STREAM_REFERENCE_ORDER = 0, RL_STREAM_PER_SAMPLE = 1, RL_STREAM_STRATIFIED = 2 } rl_stream_mode;
typedef enum rl_numerics { RL_NUMERICS_EXACT = 0, RL_NUMERICS_FAST = 1 } rl_numerics;

/* struct IntegratorPathTracing (explicit/path.rs:14-20) + scene.nb_samples + sharding. */
typedef struct rl_path_params {
    uint32_t spp;              /* scene.nb_samples (CLI global -n) */
    int32_t has_min_depth;     /* Option<u32>: 0 = None */
    uint32_t min_depth;
    int32_t has_max_depth;
    uint32_t max_depth;
    int32_t has_rr_depth;
    uint32_t rr_depth;
    int32_t strategy;          /* rl_path_strategy */
    int32_t single_scattering;
    int32_t stream_mode;       /* rl_stream_mode */
    int32_t seed_variant;      /* 0 = PCG32 fill, 1 = SplitMix64; used when forking child streams */
    /* multi-GPU sharding of the 16x16 blocks: this context renders blocks with
     * b % shard_count == shard_index, b = (ix/16)*ceil(H/16) + iy/16 (creation order, mod.rs:357-358). */
    uint32_t shard_index;
    uint32_t shard_count;
    /* tuning: number of path slots resident on the device (0 = auto). Does not change results. */
    uint32_t pool_slots;
    /* 0 = auto, 1 = wavefront stage kernels (raygen / extend / shade / shadow per iteration, state in HBM),
     * 2 = persistent fused kernel (same stages in one launch, state in registers; the BSDF code is specialised when the scene has
     * one BSDF type and switches per vertex otherwise).  Auto takes the fused kernel whenever pool_slots = 0 (reference-order
     * streams too: k_stream_chain walks the block streams — one per 16x16 block, dealt to every 32nd lane so that all SIMDs have waves — and
     * the fused kernel evaluates the samples from the recorded states) and the wavefront kernels otherwise.  Does not change results. */
    uint32_t pipeline;
    /* per-sample stream mode: lanes working on one pixel at a time (sample s of a pixel runs on lane s % sample_split; the
     * per-sample radiances are parked in HBM and added up in sample order afterwards, so the sum keeps the reference's
     * association). 0 = auto, 1 = one lane per pixel. Does not change results. */
    uint32_t sample_split;
    /* rl_numerics: 0 = exact (default; every f32 operation as the reference performs it — the only mode the parity tests bless),
     * 1 = fast (opt-in: FMA contraction, a * v_rcp(b) / raw v_sqrt / v_rsq (1 ulp, no refinement step) instead of the IEEE divide / sqrt
     * sequences, hardware sin / cos / exp2 / log2; the RNG sequence stays bit-exact, pixels agree with the exact mode within
     * BASELINE.json's per-pixel L2 tolerance in the MEAN, not bit for bit and not for every pixel on glossy scenes — DESIGN.md §2
     * "Tolerance mode").  With RL_STREAM_REFERENCE_ORDER the first flipped decision of a block shifts the rest of that block's stream: the render is then
     * statistically, not seed-for-seed, the exact build's. */
    uint32_t numerics;
} rl_path_params;

void rl_path_params_default(rl_path_params* params);   /* CLI defaults: examples/cli.rs:53-61,167-168; stream_mode = RL_STREAM_REFERENCE_ORDER */

/* Counters returned by a render (device atomics). */
typedef struct rl_render_stats {
    uint64_t camera_samples;      /* W*H*spp of this shard */
    uint64_t vertices;            /* expanded non-sensor vertices (Sigma V) */
    uint64_t extension_rays;      /* closest-hit rays traced (primary + bounce) */
    uint64_t shadow_rays;         /* NEE visibility rays traced (Sigma S) */
    uint64_t rng_draws;           /* f32 draws consumed */
    uint64_t iterations;          /* wavefront iterations */
    uint64_t kernel_launches;
    double render_ms;             /* wall time of the call (the reference's own timed region, mod.rs:324-334) */
    /* per-kernel accumulated device time from HIP events on the render stream (ms) */
    double ms_raygen, ms_extend, ms_shade, ms_shadow, ms_prepass, ms_other;   /* ms_other = the fused kernel; ms_prepass = k_stream_chain, the draw-count pass of reference-order streams */
    uint64_t n_extend_launches;
    uint64_t reserved[4];         /* k_stream_spec: samples walked speculatively / serially / by the probes, lanes per block (0: k_stream_chain ran) */
    /* reference-order streams in two passes (round 6): */
    uint32_t chunks;              /* chunks of block cursors the frame was cut into (the recorded sampler states fit their buffer); 0 = not the two-pass form */
    uint32_t overlapped;          /* 1: the evaluation pass ran BESIDE the chain pass (every chunk) — then ms_other is only the part of it left after the chain pass
                                   * had ended; 0: after it */
    double ms_eval_span;          /* the evaluation pass from its first launch to its last completion (overlapped: host clock over launches on several streams;
                                   * otherwise = ms_other): what a roofline of k_path_fused must divide by */
} rl_render_stats;

/* Opaque device context: BVHAccel::new(scene) (src/accel.rs:202-239) + flattened scene in HBM. */
typedef struct rl_context rl_context;

/* Number of HIP devices visible to the process (0 and RL_ERR_NO_DEVICE when there is none). */
int rl_device_count(int* count);

/* IntegratorType::compute's untimed prologue (src/integrators/mod.rs:280): builds the BVH2
 * (full-sweep SAH, leaf <= 2) on the host and uploads scene + BVH to `device` (HIP ordinal).
 * Fails with RL_ERR_NO_DEVICE when no GPU is present — there is no CPU fallback. */
int rl_context_create(const rl_scene* scene, int device, rl_context** out);
void rl_context_destroy(rl_context* ctx);
/* Execution options of a context (see the list at the top of this header): `value` as text, NULL = back to the default.  RL_ERR_INVALID_ARGUMENT for an unknown
 * name, RL_ERR_UNSUPPORTED for the two creation-time options.  Not to be called while a render runs on the same context.  rl_context_get_option returns the text
 * an option holds, NULL when it is not set.  (No counterpart in rustlight: these are test / measurement hooks of this implementation.) */
int rl_context_set_option(rl_context* ctx, const char* name, const char* value);
const char* rl_context_get_option(const rl_context* ctx, const char* name);
const char* rl_last_error(void);

/* generate_img_blocks (src/integrators/mod.rs:351-374): number of <=16x16 blocks, and the
 * per-block seeds `master.next_u64()` drawn in creation order (x-major). Advances `master`. */
size_t rl_block_count(uint32_t width, uint32_t height);
int rl_generate_block_seeds(rl_sampler* master, uint32_t width, uint32_t height,
                            uint64_t* seeds_out, size_t n_blocks);

/* Integrator::compute for IntegratorPathTracing (explicit/path.rs:186-196 -> compute_mc,
 * integrators/mod.rs:403-450).  Renders this shard's blocks into `out_rgb` (W*H*3 f32; pixels of
 * other shards are written as 0 so that a sum over shards is the full image).
 * out_is_device != 0: `out_rgb` is a device pointer on the context's device (e.g. a torch tensor
 * that is then reduced with RCCL); otherwise a host pointer (the framebuffer download is timed).
 * `stream`: a hipStream_t to enqueue on, or NULL for the context's own stream.  Blocking.
 * In RL_STREAM_REFERENCE_ORDER (two passes through the persistent kernel) the call also launches on low-priority streams the context owns: the evaluation pass runs beside the
 * chain pass, launched by THIS thread over the blocks the chain kernel reports complete through a few words of mapped host memory (the thread polls them every 50 us until the
 * chain pass has ended; nothing on the device waits).  The image and the counters are those of the two passes back to back (RL_NO_OVERLAP=1: a test knob that keeps them so).
 * Frames in flight: contexts share nothing mutable (each owns its stream and buffers; rl_last_error is per thread), so independent frames may be
 * rendered concurrently from several host threads, one context each, on the same device — a frame's render is a chain of dependent launches whose
 * tail leaves much of the chip idle, and another context's frame fills it (Cornell box 1080p x 128 spp in reference-order streams: 1.07 -> 1.4 G
 * samples/s with two or three in flight; the images are those of one frame after the other).  What rustlight's `-a` wrapper (avg.rs:5-131: N independent
 * renders of one scene) can use as it is; host mirrors: integrator.hpp IntegratorPathTracing::frames_in_flight, rustlight-amd --frames-in-flight K. */
int rl_render_path(rl_context* ctx, const rl_path_params* params, const uint64_t* block_seeds,
                   size_t n_blocks, float* out_rgb, int out_is_device, void* stream,
                   rl_render_stats* stats);

/* Integrator::compute for IntegratorLightTracing (src/integrators/explicit/light.rs, CLI `light-tracing`): spp * W * H light paths from the emitters, every
 * vertex splatted through the camera (Camera::sample_direct).  Takes rl_path_params: spp, the three depth options, `strategy` as rl_light_strategy, `seed_variant`;
 * `block_seeds` as for rl_render_path.  Job b (the 16x16 blocks in creation order) traces spp x (pixels of block b) light paths; light path (b, slot p, sample s)
 * draws from the stream RL_STREAM_PER_SAMPLE gives camera sample (b, pixel p, s).  The reference splits its paths over 4 x threads jobs, so no seed matches it
 * path for path: the image agrees in distribution.  Splats are summed per pixel and channel in 96-bit unsigned fixed point (24 fraction bits; a 64-bit
 * low word and a 32-bit carry count): same seeds, same bits, exact while a channel takes fewer than 2^41 clamped splats, so no finite splat can make a pixel
 * negative or wrap it; the pixel is the f32 of (carry * 2^64 + low) * 2^-24 / spp computed in f64.  A splat with a
 * negative or NaN channel is dropped (Color::is_valid); a +inf channel makes the pixel's channel +inf; a channel >= 2^31 is clamped.  RL_ERR_UNSUPPORTED for
 * stream_mode other than RL_STREAM_PER_SAMPLE, numerics = RL_NUMERICS_FAST, shard_count > 1 and scenes with an environment emitter; RL_ERR_NO_EMITTER without
 * emitters.  The counters mean: camera_samples = light paths traced, vertices = expanded vertices (the light vertex included), extension_rays = closest-hit rays,
 * shadow_rays = camera-connection visibility rays, rng_draws, kernel_launches; ms_other = k_light_fused's device time; reserved[0] = splats added,
 * reserved[1] = splats dropped as invalid, reserved[2] = splats with a saturated (clamped or +inf) channel. */
typedef enum rl_light_strategy { RL_LIGHT_ALL = 0, RL_LIGHT_SURFACE = 1, RL_LIGHT_VOLUME = 2 } rl_light_strategy;
int rl_render_light(rl_context* ctx, const rl_path_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                    int out_is_device, void* stream, rl_render_stats* stats);

/* IntegratorVPL (src/integrators/explicit/vpl.rs, CLI `vpl`): virtual point lights shot from the emitters, then gathered at every camera sample, seed for
 * seed the reference in its reference-order streams.  IntegratorVPL::compute = rl_vpl_generate with the main sampler, rl_generate_block_seeds with the
 * sampler it leaves, rl_render_vpl.  option_vpl / option_lt take an rl_vpl_option, as `-v` / `-l` do.
 *
 * rl_vpl_generate: the generation loop (vpl.rs:182-210) on one device lane, from `sampler`'s state, which it advances as the reference's main sampler is
 * advanced.  Light paths are shot while fewer than nb_vpl VPLs are stored, so the set holds at least nb_vpl of them (all of the last path's).  Of
 * rl_path_params it reads max_depth and rr_depth (min_depth is ignored, as by the reference).  nb_vpl is 1 .. RL_VPL_MAX; at most RL_VPL_MAX_PATHS paths
 * are shot, and RL_ERR_UNSUPPORTED is returned (no set) when they store fewer than nb_vpl VPLs.  Refused before any kernel runs: max_depth <= 1
 * (RL_ERR_INVALID_ARGUMENT; the reference panics at vpl.rs:138), option_vpl = RL_VPL_VOLUME without a medium and a directional light with a medium
 * (RL_ERR_UNSUPPORTED; the reference loops forever or asserts), environment emitters (RL_ERR_UNSUPPORTED), no emitter (RL_ERR_NO_EMITTER).  Counters:
 * camera_samples = light paths shot, vertices = expanded vertices, extension_rays, rng_draws; ms_prepass = generation kernel time.
 *
 * rl_vpl_read: RL_VPL_WORDS u32 per VPL in VPL order (f32 fields as their bits): [0] kind (rl_vpl_kind), [1] mesh (surface), [2] has_uv (surface), [3] 0,
 * [4..6] position (RL_VPL_EMITTER_INFINITE: the direction d), [7..9] radiance, [10..12] wi in the shading frame (surface) / d_in (volume) / n (emitter
 * position), [13..14] uv (surface), [15..23] the shading frame's x, y, z axes (surface); unused words are 0.  n_words must be n_vpl * RL_VPL_WORDS.
 *
 * rl_render_vpl: the gather (vpl.rs:212-535) with `block_seeds` as for rl_render_path.  Sample (ix, iy, s) of a block draws D numbers (2, 3 when the scene
 * has a medium) from draw ((ix * bh + iy) * spp + s) * D of the block's stream.  Reads spp, seed_variant, shard_index / shard_count (every shard gets the
 * whole set: each generates the same one); RL_ERR_UNSUPPORTED for stream_mode other than RL_STREAM_REFERENCE_ORDER, numerics = RL_NUMERICS_FAST and
 * spp > RL_VPL_MAX_SPP; the set must come from the same context.  One deliberate difference: where a camera ray leaves the scene inside a medium the
 * pixel gets +0 without a gather (the reference's `l_i *= ..` with l_i = 0, vpl.rs:483, differs only where that gather is not finite).  Counters:
 * camera_samples = W*H*spp of the shard, extension_rays = camera rays, shadow_rays = connection rays traced (none at smooth gather points, where they add
 * nothing), rng_draws = D * camera_samples, kernel_launches; ms_raygen = the primary passes, ms_other = the gather passes (spp <= 256); reserved[0] = gather points on
 * surfaces, reserved[1] = gather points in the medium. */
typedef enum rl_vpl_option { RL_VPL_ALL = 0, RL_VPL_SURFACE = 1, RL_VPL_VOLUME = 2 } rl_vpl_option;
typedef enum rl_vpl_kind { RL_VPL_KIND_SURFACE = 0, RL_VPL_KIND_VOLUME = 1, RL_VPL_KIND_EMITTER_POSITION = 2, RL_VPL_KIND_EMITTER_INFINITE = 3 } rl_vpl_kind;
enum { RL_VPL_WORDS = 24, RL_VPL_MAX = 1 << 20, RL_VPL_MAX_PATHS = 1 << 18, RL_VPL_MAX_SPP = 1 << 22 };
typedef struct rl_vpl_set rl_vpl_set;       /* opaque: the VPLs of one generation, on the context's device */
int rl_vpl_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, rl_sampler* sampler, rl_vpl_set** out,
                    rl_render_stats* stats);
/* rl_vpl_generate_paths: the generation with one light path per device lane, each on its own sampler stream — an opt-in, as RL_STREAM_PER_SAMPLE is for the
 * camera passes; rl_vpl_generate stays the drop-in default.  Statistically, not seed-for-seed, the same image as the serial mode's.  The stream contract:
 *   - light path k = 0, 1, 2, .. draws from the sampler the k-th clone_box() call on the main sampler returns (src/samplers/independent.rs:18-22): seed_k is the
 *     k-th next_u64() of `sampler` counted from its incoming state, the path's stream is rl_sampler_seed(seed_k, params->seed_variant);
 *   - inside its stream a path draws exactly what a path of rl_vpl_generate draws (kernels/light.hip.h lists the order);
 *   - the set holds paths 0 .. K-1, K the smallest count at which at least nb_vpl records are stored: the reference's `while stored < nb` on this path
 *     sequence (all of the last path's records are kept); n_paths = K;
 *   - records stand in path order, and in vertex order within a path; record layout and option_vpl filter are rl_vpl_generate's;
 *   - `sampler` leaves advanced by exactly K next_u64(); the block seeds are then drawn from it as after rl_vpl_generate;
 *   - paths walked speculatively beyond K leave no trace in the records, the counters or the sampler;
 *   - nothing in the result depends on batch size, launch geometry, lane assignment or run: the same incoming state gives the same bits.
 * Of rl_path_params it reads max_depth, rr_depth and seed_variant; stream_mode is not read (it is about the gather).  Refuses what rl_vpl_generate refuses, with the
 * same codes, and returns RL_ERR_UNSUPPORTED when RL_VPL_MAX_PATHS paths store fewer than nb_vpl records.  The set is an ordinary rl_vpl_set: rl_vpl_info,
 * rl_vpl_read, rl_render_vpl and rl_photon_map_build take it unchanged.  It runs in rounds: a count pass walks a batch of paths and stores four counts per path,
 * the host takes the prefix sum and looks for K, a further batch follows when the first did not reach nb_vpl, and a write pass walks paths 0 .. K-1 again, each
 * to its own offset.  Counters: camera_samples = K; vertices, extension_rays, rng_draws = sums over the K kept paths (the K fork draws are not counted);
 * iterations = rounds; kernel_launches; ms_prepass = the summed kernel time; reserved[0] = paths walked in the count passes, discarded ones included. */
int rl_vpl_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_vpl, int option_vpl, rl_sampler* sampler, rl_vpl_set** out,
                          rl_render_stats* stats);
int rl_vpl_info(const rl_vpl_set* set, uint64_t* n_vpl, uint64_t* n_paths);
int rl_vpl_read(const rl_vpl_set* set, uint32_t* words, size_t n_words);
void rl_vpl_destroy(rl_vpl_set* set);
int rl_render_vpl(rl_context* ctx, const rl_vpl_set* set, const rl_path_params* params, int option_lt, const uint64_t* block_seeds, size_t n_blocks,
                  float* out_rgb, int out_is_device, void* stream, rl_render_stats* stats);

/* ---- IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: BRE } (src/integrators/explicit/vol_primitives.rs; CLI `vol-primitivies -p bre`,
 * examples/cli.rs:189-196, 692-716): the beam radiance estimate.  Beams, planes and VRL have entry points of their own (rl_beam_*, rl_pplane_*, rl_vrl_*, below).
 * The photons are the records of a set generated by rl_vpl_generate with option_vpl = RL_VPL_VOLUME and nb_vpl = nb_primitive: convert_photons
 * (vol_primitives.rs:525-565) stores at every Vertex::Volume what convert_vpl stores under `-v volume`, from the same light paths, and the shooting stops on the
 * same count — words 4..6 = pos, 7..9 = radiance, 10..12 = d_in; the set's path count is nb_path_shot.
 * rl_photon_map_build sorts them into BHVAccel's tree (src/accel.rs:458-543: leaves of at most 4, otherwise sorted along the longest axis of the node's box and
 * split in the middle) on the host and uploads it.  `radius`: the photon radius; the reference hard-codes RL_PHOTON_RADIUS_DEFAULT (vol_primitives.rs:618).
 * Two deliberate differences: the sort is stable (the reference's sort_unstable_by leaves the order of equal keys unspecified) and a non-finite position is
 * RL_ERR_INVALID_ARGUMENT (the reference panics).  Also refused: a scene without a medium (RL_ERR_UNSUPPORTED), a set that holds a record of another kind or
 * belongs to another context, a radius that is not finite and > 0 (RL_ERR_INVALID_ARGUMENT).
 * rl_render_bre (vol_primitives.rs:712-790): per camera sample 2 draws (the jitter), the camera ray with tfar = its closest hit's distance (f32::MAX on a miss:
 * the ray still gathers), BHVAccel::gather in the reference's visiting order (node, right subtree, left subtree; a leaf's photons in index order) and
 * c += radiance * exp(-sigma_t * t) * phase(-d, d_in) * 1 / (PI r^2) * 1 / nb_path_shot per photon whose sphere the ray meets; samples are added in order and
 * scaled by 1 / spp.  Reference-order streams (sample (ix, iy, s) of a block starts at draw ((ix * bh + iy) * spp + s) * 2 of its stream), exact numerics, one
 * device, host output; shards as rl_render_vpl; spp > RL_VPL_MAX_SPP is RL_ERR_UNSUPPORTED.  Counters: camera_samples, extension_rays = camera_samples,
 * rng_draws = 2 * camera_samples, kernel_launches, ms_other = the gather kernel; reserved[0] = photon-tree nodes entered, reserved[1] = photons gathered.
 * rl_photon_tree_build: the host part alone, no GPU — the tree of `n_photons` records (RL_VPL_WORDS u32 each, only words 4..6 are read) as the device walks
 * it: nodes in visiting order, node_boxes [n][6] = p_min, p_max, node_links [n][3] = skip (the node to go on with when the box is missed; entered: the next
 * one), first, count (count = 0: inner node; a leaf holds places first .. first + count - 1), order[place] = index of the record that stands there.  With the
 * three arrays NULL only *n_nodes is written (at most 2 * n_photons).
 * rl_photon_map_build_device: what rl_photon_map_build does, built where the records are — device kernels (kernels/phototree.hip.h) check the records, sort
 * every level and write tree and photons; no record, node or photon crosses to the host, only the flag word of the check pass.  The map is the same type and
 * holds the same bytes as the host build's (the topology depends on the photon count alone, a stable sort equals any sort by (key, place before the sort), and
 * float min / max is exact in any order); refusals, codes and rl_last_error texts are the same.  ms_kernels (may be NULL): the summed HIP-event time of the
 * launches, 0 under the option no_events.  Ranges of at most RL_PHOTON_TREE_GROUP_PHOTONS photons are finished by one workgroup each in LDS; the option
 * photon_tree_group_photons = n forces a smaller group (4 .. RL_PHOTON_TREE_GROUP_PHOTONS; tests) and changes no result.
 * rl_photon_tree_build_device: rl_photon_tree_build's contract, the size-only call included, computed by the same device kernels: the words are uploaded, the
 * arrays downloaded.  `ctx` names the device (and carries the options); the scene needs no medium.
 * rl_photon_map_read: a map of either build as host arrays — node_boxes [n_nodes][6], node_links [n_nodes][3] = skip, first, count as rl_photon_tree_build
 * writes them, photons [n_photons][9] = pos, radiance, d_in in leaf order.  The capacities are in nodes / photons and must cover rl_photon_map_info's counts. */
#define RL_PHOTON_RADIUS_DEFAULT 0.001f
enum { RL_PHOTON_TREE_GROUP_PHOTONS = 2048 };
typedef struct rl_photon_map rl_photon_map;       /* opaque: photon tree and photons, on the context's device */
int rl_photon_map_build(rl_context* ctx, const rl_vpl_set* set, float radius, rl_photon_map** out);
int rl_photon_map_info(const rl_photon_map* map, uint64_t* n_photons, uint64_t* n_nodes, uint64_t* n_paths, float* radius);
void rl_photon_map_destroy(rl_photon_map* map);
int rl_render_bre(rl_context* ctx, const rl_photon_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                  const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats);
int rl_photon_tree_build(const uint32_t* words, size_t n_photons, float radius, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                         uint32_t* node_links, uint32_t* order);
int rl_photon_map_build_device(rl_context* ctx, const rl_vpl_set* set, float radius, rl_photon_map** out, float* ms_kernels);
int rl_photon_tree_build_device(rl_context* ctx, const uint32_t* words, size_t n_photons, float radius, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                                uint32_t* node_links, uint32_t* order);
int rl_photon_map_read(const rl_photon_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t photon_capacity, float* photons);

/* ---- Photon beams: IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: Beams } (src/integrators/explicit/vol_primitives.rs), behind entry
 * points and a CLI word (`photon-beams`) of their own: `vol-primitivies -p beam` stays refused with the other unbuilt primitives.
 * rl_beam_generate (vol_primitives.rs:437-523, 608-630): the light paths of rl_vpl_generate — Path::from_light, `generate` with max_depth / rr_depth and
 * DirectionalSamplingStrategy { Radiance }, the same draws in the same order on the main sampler, seed for seed — stored by convert_beams(false, ..) while
 * fewer than nb_primitive beams are stored (every beam of the last path is kept).  A beam is a traced edge that ends in a vertex; with a medium every traced
 * edge does (src/paths/edge.rs:90-126), so a path stores one beam per extension ray.  nb_primitive is 1 .. RL_BEAM_MAX (the split below makes at most about 6
 * sub-beams per beam, and the tree takes RL_VPL_MAX + 4096 elements).  Refused with rl_vpl_generate(RL_VPL_VOLUME)'s codes: a scene without a medium, with an
 * environment emitter or a directional light (RL_ERR_UNSUPPORTED), without an emitter (RL_ERR_NO_EMITTER), max_depth <= 1, nb_primitive out of range
 * (RL_ERR_INVALID_ARGUMENT); RL_ERR_UNSUPPORTED when RL_VPL_MAX_PATHS paths store fewer beams than asked.  Counters and the sampler on return: rl_vpl_generate's.
 * rl_beam_generate_paths: the same pass with one light path per device lane under rl_vpl_generate_paths' stream contract (path k on the k-th clone_box; a
 * count pass, then a write pass; records in path order and in vertex order within a path; `sampler` advanced by K next_u64()); its counters.
 * rl_beam_read: RL_BEAM_WORDS u32 per beam in storing order (f32 fields as their bits): [0..2] o, the position of the vertex the edge leaves, [3] length =
 * edge.dist (the sampled medium distance where the path scattered, the hit distance otherwise), [4..6] d, the edge's direction, [7] bit 0 = from_surface (o is
 * the light vertex or a surface vertex), [8..10] radiance, the flux that reached o (before this edge's weight * rr_weight, :453-520), [11] the path's index
 * within the generation.  n_words must be n_beams * RL_BEAM_WORDS.  A beam's phase function is Isotropic whatever the medium's is (:457, 483, 500): kept.
 * rl_beam_split (vol_primitives.rs:647-684), the host part alone, no GPU: SPLIT = 5, avg_split = (the lengths summed in f32 in record order) / (n * 5) as f32,
 * a beam yields ceil(length / avg_split) as u32 sub-beams of new_length = length / that count, sub-beam i starting at o + d * (i as f32) * new_length; a beam of
 * length 0 yields none.  Sub-beams are records of the same layout in beam order.  With sub_words NULL only *n_sub is written; `capacity` is in records.
 * RL_ERR_INVALID_ARGUMENT for a non-finite o, d or length and for an avg_split that is zero or not finite, RL_ERR_UNSUPPORTED when the split makes more than
 * RL_VPL_MAX + 4096 sub-beams.
 * rl_beam_tree_build (vol_primitives.rs:123-136, 686-699), no GPU, rl_photon_tree_build's calling convention over sub-beam records: box = the union of
 * o - r, o + r, (o + d * length) - r, (o + d * length) + r, sort key = o + d * length * 0.5, otherwise rl_photon_map_build's tree with its two deliberate
 * differences (a stable sort; a non-finite record or box is RL_ERR_INVALID_ARGUMENT).
 * rl_beam_map_build: split, tree, upload (the tree and the sub-beams in leaf order as 48-byte records o, length | d, 0 | radiance, 0).  `radius` as for
 * rl_photon_map_build; the set must come from the same context.  rl_beam_map_build_words: the same from caller-supplied beam records; n_paths >= 1 stands for
 * nb_path_shot.  rl_beam_map_read: node_boxes / node_links as rl_photon_map_read writes them, beams [n_sub][12] f32 in leaf order.
 * rl_render_beams (vol_primitives.rs:140-199, 705-790): rl_render_bre's camera loop, streams, shards, refusals and counters over the beam tree; per sub-beam
 * PhotonBeam::intersection statement by statement (tnear = 1e-4) and c += radiance * transmittance(w) * (sigma_s * 1 / (4 PI)) * ((1 / sin_theta) * (0.5 /
 * radius)) * (1 / nb_path_shot) in gather order.  reserved[0] = beam-tree nodes entered, reserved[1] = beams accepted. */
enum { RL_BEAM_WORDS = 12, RL_BEAM_MAX = 1 << 17 };
typedef struct rl_beam_set rl_beam_set;         /* opaque: the beams of one generation, on the context's device */
typedef struct rl_beam_map rl_beam_map;         /* opaque: beam tree and sub-beams, on the context's device */
int rl_beam_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats);
int rl_beam_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_beam_set** out, rl_render_stats* stats);
int rl_beam_info(const rl_beam_set* set, uint64_t* n_beams, uint64_t* n_paths);
int rl_beam_read(const rl_beam_set* set, uint32_t* words, size_t n_words);
void rl_beam_destroy(rl_beam_set* set);
int rl_beam_split(const uint32_t* words, size_t n_beams, size_t capacity, size_t* n_sub, uint32_t* sub_words);
int rl_beam_tree_build(const uint32_t* sub_words, size_t n_sub, float radius, size_t node_capacity, size_t* n_nodes, float* node_boxes, uint32_t* node_links,
                       uint32_t* order);
int rl_beam_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_beam_map** out);
int rl_beam_map_build_words(rl_context* ctx, const uint32_t* words, size_t n_beams, uint64_t n_paths, float radius, rl_beam_map** out);
int rl_beam_map_info(const rl_beam_map* map, uint64_t* n_beams, uint64_t* n_sub, uint64_t* n_nodes, uint64_t* n_paths, float* radius);
int rl_beam_map_read(const rl_beam_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t beam_capacity, float* beams);
void rl_beam_map_destroy(rl_beam_map* map);
int rl_render_beams(rl_context* ctx, const rl_beam_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                    const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats);

/* ---- Photon planes: IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: Planes } (src/integrators/explicit/vol_primitives.rs), behind entry
 * points and a CLI word (`photon-planes`) of their own: `vol-primitivies -p plane` stays refused with the other unbuilt primitives.
 * rl_pplane_generate (vol_primitives.rs:376-523, 608-630): the light paths of rl_beam_generate — the same draws in the same order on the main sampler, seed for
 * seed — stored by convert_beams(true, ..) and convert_planes(..) while fewer than nb_primitive planes are stored (every record of the last path is kept).  An
 * edge that leaves the light vertex or a surface vertex is a beam.  An edge e that leaves a volume vertex V1 is a plane when it ends in a volume vertex V2 that
 * was expanded with an edge e2, and a beam otherwise (V2 on a surface, or not expanded: depth limit, Russian roulette, zero throughput).  nb_primitive is 1 ..
 * RL_BEAM_MAX.  Refused with rl_beam_generate's codes for what it refuses; max_depth <= 3 is RL_ERR_INVALID_ARGUMENT (V2 is expanded only when 3 < max_depth: no
 * plane exists below that and the reference never stops shooting); RL_ERR_UNSUPPORTED when RL_VPL_MAX_PATHS paths store fewer planes than asked, or when more
 * than RL_BEAM_MAX + 2048 beams arise before nb_primitive planes are stored (the beams are not bounded by the plane count; the message names the medium).
 * Counters and the sampler on return: rl_vpl_generate's, camera_samples = paths shot.
 * rl_pplane_generate_paths: the same pass with one light path per device lane under rl_vpl_generate_paths' stream contract (a count pass, then a write pass;
 * both kinds of record in path order; `sampler` advanced by K next_u64()); its counters.
 * rl_pplane_read: the planes, RL_PLANE_WORDS u32 each in rl_plane_read's geometry layout (:404-412) — [0..2] o = V1, [3..5] d0 = e.d, [6..8] d1 = e2.d, [9]
 * length0 = continued_t(e) = e.dist, [10] length1 = continued_t(e2), the distance e2's medium sample drew before it was cut at the hit distance (volume.rs:102-130;
 * it exceeds the hit distance when e2 ends on a surface), [11..13] radiance, the flux that reached V1, [14] the path's index within the generation, [15] the
 * index of e within the path, [16..17] 0 — and the beams, RL_BEAM_WORDS u32 each in rl_beam_read's layout; both in storing order.  The word counts must be
 * n_planes * RL_PLANE_WORDS and n_beams * RL_BEAM_WORDS.  A plane's phase function is Isotropic whatever the medium's is (:410): kept.
 * rl_pplane_map_build (vol_primitives.rs:647-699): the beams through rl_beam_map_build's split and beam tree (`radius` as there; the reference hard-codes
 * 0.001), the planes through rl_plane_tree_build's tree (aabb = the four corners, position = the middle, :275-291), both uploaded: sub-beams as 48-byte records,
 * planes as 4 x float4 in leaf order, o, length0 | d0, length1 | d1, 0 | radiance, 0.  The context option pplane_tree_device = 1 builds the plane tree with the
 * kernels of rl_plane_map_build_device: the same bytes.  rl_pplane_map_build_words: the same from caller-supplied records; n_paths >= 1 stands for nb_path_shot.
 * Refused: what rl_beam_map_build_words and rl_plane_tree_build refuse (a radius that is not finite and > 0, non-finite o, d, length or corner, a zero or
 * non-finite avg_split, n_paths = 0, a split beyond the tree's capacity), a caller's plane record whose words 16 or 17 are not 0, a set of another context.
 * rl_pplane_map_read: which = 0 the beam tree with the sub-beams [n_sub][12] f32, which = 1 the plane tree with the planes [n_planes][16] f32; node_boxes /
 * node_links as rl_photon_map_read writes them.
 * rl_render_photon_planes (vol_primitives.rs:295-373, 705-790): rl_render_beams' camera loop, streams, shards and refusals; per camera sample first the beam
 * tree with rl_render_beams' test and contribution, then the plane tree, both added into one c, which is then accumulated (in f32 the order matters, so one
 * kernel walks both).  Per plane PhotonPlane::intersection statement by statement (tnear = 1e-4), one visibility ray visible(o + d0 * t0, ray.o + ray.d * t_cam),
 * c += radiance * 1 / (4 PI) * sigma_s * sigma_s * transmittance(t_cam) * (1 / |d0 . (d1 x -ray.d)|) * (1 / nb_path_shot).  reserved[0] = nodes entered in both
 * trees, reserved[1] = beams accepted, reserved[2] = planes intersected (= shadow_rays), reserved[3] = of those, visible. */
typedef struct rl_pplane_set rl_pplane_set;     /* opaque: the planes and surface beams of one generation, on the context's device */
typedef struct rl_pplane_map rl_pplane_map;     /* opaque: beam tree, sub-beams, plane tree and planes, on the context's device */
int rl_pplane_generate(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats);
int rl_pplane_generate_paths(rl_context* ctx, const rl_path_params* params, uint32_t nb_primitive, rl_sampler* sampler, rl_pplane_set** out, rl_render_stats* stats);
int rl_pplane_info(const rl_pplane_set* set, uint64_t* n_planes, uint64_t* n_beams, uint64_t* n_paths);
int rl_pplane_read(const rl_pplane_set* set, uint32_t* plane_words, size_t n_plane_words, uint32_t* beam_words, size_t n_beam_words);
void rl_pplane_destroy(rl_pplane_set* set);
int rl_pplane_map_build(rl_context* ctx, const rl_pplane_set* set, float radius, rl_pplane_map** out);
int rl_pplane_map_build_words(rl_context* ctx, const uint32_t* beam_words, size_t n_beams, const uint32_t* plane_words, size_t n_planes, uint64_t n_paths,
                              float radius, rl_pplane_map** out);
int rl_pplane_map_info(const rl_pplane_map* map, uint64_t* n_beams, uint64_t* n_sub, uint64_t* n_beam_nodes, uint64_t* n_planes, uint64_t* n_plane_nodes,
                       uint64_t* n_paths, float* radius);
int rl_pplane_map_read(const rl_pplane_map* map, int which, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t element_capacity, float* elements);
void rl_pplane_map_destroy(rl_pplane_map* map);
int rl_render_photon_planes(rl_context* ctx, const rl_pplane_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                            const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats);

/* ---- Virtual ray lights: IntegratorVolPrimitives { nb_primitive, max_depth, rr_depth, primitives: VRL } (src/integrators/explicit/vol_primitives.rs:201-253,
 * 608-699, 741-764), behind entry points and a CLI word (`virtual-ray-lights`) of their own: `vol-primitivies -p vrl` stays refused.
 * The beams are rl_beam_generate's / rl_beam_generate_paths': the VRL arm shoots with convert_beams(false, ..) and stops on the same count.
 * rl_vrl_map_build (vol_primitives.rs:632-699): the beams whose word 7 bit 0 (from_surface) is clear are the VRLs, in storing order and unsplit; avg = (their
 * channel_max(radiance) summed in f32 in that order) / n_vrl as f32, rr = ((channel_max(radiance) / avg) * 0.01).min(1.0) (f32::min returns the operand that
 * is no NaN: avg = 0 gives rr = 1).  The surface beams go through rl_beam_map_build's split and tree; avg_split is taken over them alone.  rl_vrl_map_build_words:
 * the same from caller-supplied beam records.  Refused: what rl_beam_map_build_words refuses, with its codes; no surface beam among the records, or a VRL record
 * with a non-finite o, d, length or radiance (RL_ERR_INVALID_ARGUMENT).  No VRL at all is valid (max_depth = 2).
 * rl_vrl_map_info: surface beams, their sub-beams, tree nodes, VRLs, light paths, radius, avg (0 when there is no VRL).  rl_vrl_map_read: node_boxes / node_links
 * and beams as rl_beam_map_read writes them, then vrls [n_vrl][12] f32 = o, length | d, rr | radiance, 0 in storing order (vrls may be NULL when there is none).
 * rl_render_vrl (vol_primitives.rs:741-764): rl_render_beams' camera loop, streams, shards and refusals; per camera sample c = the surface beams' contributions
 * in gather order, then for each VRL in order `if rr >= next()`: t_cam = (tfar - 1e-4) * next() + 1e-4, t_vrl = length * next(), one visibility ray
 * visible(ray.o + ray.d * t_cam, o + d * t_vrl), c += ((radiance * (sigma_s / 4 PI) * (sigma_s / 4 PI) * transmittance(t_cam) * transmittance(dist) * (length *
 * (tfar - 1e-4)) / (dist * dist)) / rr) * (1 / nb_path_shot), left to right with Color's guards.  A sample takes 2 + n_vrl + 2 A draws (A = the VRLs that passed
 * its roulette), so a first kernel walks every block's stream for the draw at which each pixel starts.  RL_ERR_UNSUPPORTED when 256 * spp * (2 + 3 * n_vrl)
 * reaches 2^32.  rng_draws = the draws walked; reserved[0] = beam-tree nodes entered, reserved[1] = beams accepted, reserved[2] = VRLs that passed the roulette
 * (= shadow_rays), reserved[3] = of those, visible; ms_prepass = the first kernel, ms_other = both. */
typedef struct rl_vrl_map rl_vrl_map;           /* opaque: beam tree and sub-beams of the surface beams, and the VRLs, on the context's device */
int rl_vrl_map_build(rl_context* ctx, const rl_beam_set* set, float radius, rl_vrl_map** out);
int rl_vrl_map_build_words(rl_context* ctx, const uint32_t* words, size_t n_beams, uint64_t n_paths, float radius, rl_vrl_map** out);
int rl_vrl_map_info(const rl_vrl_map* map, uint64_t* n_surface, uint64_t* n_sub, uint64_t* n_nodes, uint64_t* n_vrl, uint64_t* n_paths, float* radius, float* avg);
int rl_vrl_map_read(const rl_vrl_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t beam_capacity, float* beams, size_t vrl_capacity,
                    float* vrls);
void rl_vrl_map_destroy(rl_vrl_map* map);
int rl_render_vrl(rl_context* ctx, const rl_vrl_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                  const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats);

/* ---- IntegratorSinglePlane { nb_primitive, strategy } (src/integrators/explicit/plane_single.rs; CLI `plane-single`, examples/cli.rs:197-202, 664-691): single
 * scattering from rectangular area lights, estimated with photon planes under one of seven sampling strategies.
 * The lights: RectangularLightSource::from_shape (plane_single.rs:38-75) of every emissive mesh, in mesh order — o = v[0], u = v[1] - v[0], v = v[3] - v[0],
 * normalised by their lengths, n = u x v.  Point, directional and environment lights are ignored, as the reference ignores them.  Refused before any kernel
 * runs, by every entry point below that takes a context: a scene without a medium (RL_ERR_UNSUPPORTED; the reference panics), without an emissive mesh
 * (RL_ERR_NO_EMITTER), with an emissive mesh that is not 2 triangles over at least 4 vertices, or whose emission is HSV or textured (RL_ERR_UNSUPPORTED).
 * rl_plane_generate: the loop `while planes.len() < nb_primitive` (plane_single.rs:363-427) on the main sampler, seed for seed — per iteration one draw for
 * id_emitter, then one plane (UV / VT / UT / UALPHA / CMIS) or the three planes UV, VT, UT (AVERAGE / DISCRETE_MIS); a plane takes 2 draws for its direction
 * (drawn again while the direction's z is 0), 1 for the distance, 2 for `sample`, 1 for alpha.  It runs on one device lane (the pass needs the deterministic
 * log / sin / cos the kernels hold).  nb_primitive is 1 .. RL_VPL_MAX; `sampler` leaves advanced exactly as the reference's main sampler is.  One deliberate
 * difference: id_emitter is clamped to the last light where the reference would index out of range.  A plane with a non-finite corner is
 * RL_ERR_INVALID_ARGUMENT (the sampler is then left as it was).  Counters: camera_samples = iterations (number_plane_gen), vertices = planes, rng_draws,
 * kernel_launches, ms_prepass = the kernel.
 * rl_plane_read: the planes as records of RL_PLANE_WORDS u32 — [0..2] o, [3..5] d0, [6..8] d1, [9] length0, [10] length1, [11..13] weight, [14..15] sample,
 * [16] rl_plane_type, [17] id_emitter.  n_words must be n_planes * RL_PLANE_WORDS.
 * rl_plane_map_build sorts them into BHVAccel's tree on the host — box = the union of the plane's four corners, sort key = the plane's middle
 * (plane_single.rs:101-117), otherwise rl_photon_map_build's tree with its two deliberate differences (a stable sort; a non-finite corner is
 * RL_ERR_INVALID_ARGUMENT) — and uploads the tree, the planes in leaf order as 64-byte records and the lights.  The set must come from the same context.
 * rl_plane_tree_build: the host part alone, no GPU, with rl_photon_tree_build's calling convention over records of RL_PLANE_WORDS u32.
 * rl_plane_map_read: node_boxes / node_links as rl_photon_map_read writes them, planes [n_planes][16] f32 = o, length0 | d0, length1 | d1, the bits of
 * type + 4 * id_emitter | weight, 0, in leaf order.
 * rl_render_plane_single (plane_single.rs:436-611): per camera sample 2 draws (the jitter), the camera ray with tfar = its closest hit's distance (f32::MAX on
 * a miss), BHVAccel::gather in the reference's visiting order; per plane the ray meets (tnear = 1e-4): the point on the light, one visibility ray, and
 * c += w * rho * transmittance * sigma_s * flux * n_lights * (1 / number_plane_gen) with the strategy's w and flux (DISCRETE_MIS: the balance heuristic over the
 * three planes re-made through the point; CMIS: its closed-form weight).  rho is the isotropic phase function whatever the medium's is: the reference
 * hard-codes it.  Samples are added in order and scaled by 1 / spp.  Reference-order streams, exact numerics, one device, host output; shards, spp limit and
 * their codes as rl_render_bre.  Counters: camera_samples, extension_rays = camera_samples, shadow_rays = planes intersected, rng_draws = 2 * camera_samples,
 * kernel_launches, ms_other = the gather kernel; reserved[0] = plane-tree nodes entered, reserved[1] = planes intersected, reserved[2] = of those, visible.
 * The device forms (opt-in; each is byte for byte the form above, so the options plane_generate_lanes / plane_tree_device = 1 make rl_plane_generate /
 * rl_plane_map_build forward to them):
 * rl_plane_generate_lanes: rl_plane_generate's arguments, refusals, set, sampler state and counters, one device lane per iteration of the loop.  An
 * iteration takes D = 1 + 6 k draws (k = 3 planes for AVERAGE / DISCRETE_MIS, else 1) unless a direction is drawn again, so lane i starts D i draws down
 * the main sampler's stream (jump-ahead); a lane that meets such a redraw raises a flag, and the call then runs rl_plane_generate's serial kernel from the
 * original state instead.  The set keeps its records on the device as well: rl_plane_map_build_device uploads nothing, rl_plane_read and the host build
 * download them on first use.
 * rl_plane_map_build_device: rl_plane_map_build's map — nodes, planes, lights, counts, strategy — built by the kernels of kernels/phototree.hip.h over the
 * plane element: a prepass takes every plane's box and keys with the host's separately rounded operations, the levels sort as for photons, a last kernel
 * writes the planes in leaf order.  A set made by rl_plane_generate is uploaded once.  ms_kernels as for rl_photon_map_build_device.  Ranges of at most
 * RL_PLANE_TREE_GROUP_PLANES planes are finished by one workgroup in LDS; the option plane_tree_group_planes = n forces a smaller group (tests).
 * rl_plane_tree_build_device: rl_plane_tree_build's contract (codes, size-only call, refusals) computed by the same kernels, with
 * rl_photon_tree_build_device's calling convention.
 * ---- IntegratorSinglePlaneUncorrelated { nb_primitive, strategy } (src/integrators/explicit/uncorrelated_plane_single.rs; the reference's CLI word is
 * `uncorrelated-plane-single`, here `plane-single --uncorrelated`): the same estimate with no plane set — every camera sample makes nb_primitive planes of
 * its own.  rl_render_plane_uncorrelated is the whole integrator behind the block seeds (:83: they come straight from the main sampler, as for `path`): no
 * light pass, no tree, one kernel (kernels/uplane.hip.h).  Per camera sample, in the block's loop order ix, iy, sample (:95-97), the block's stream gives 2
 * draws for the jitter (:99-102) — the camera ray takes tfar = its closest hit's distance, f32::MAX on a miss (:103-110) — and per plane j < nb_primitive:
 * 1 for id_emitter (:115; clamped to the last light, the deviation rl_plane_generate has), 1 more under AVERAGE / DISCRETE_MIS for the plane type (< 1/3 UV,
 * < 2/3 VT, else UT, :142-167), 2 for the direction (drawn again while its z is 0, :51-55), 1 for the distance (:65), 2 for `sample` (:68), 1 for alpha (:74).
 * The plane is then treated as rl_render_plane_single treats one (:179-292): c += w * rho * transmittance * sigma_s * flux * n_lights * (1 / nb_primitive).
 * A sample so takes D = 2 + nb_primitive * (7 or 8) draws plus 2 per redraw; the 256 lanes of a block enter its stream D * spp draws apart by jump-ahead and a
 * block in which a direction is drawn again resolves the moved starts inside the kernel, so the image is the serial walk's bit for bit.
 * Two behaviours of the reference are kept: (1) a plane with a non-finite corner is not refused — there is no tree to refuse it — and goes through the
 * intersection's comparisons as it does there; (2) AVERAGE and DISCRETE_MIS pick ONE of the three plane types with probability 1/3 and still weight it by 1/3
 * (or by a balance weight that sums to 1 over the types) while dividing by nb_primitive: they return a third of the radiance of the other strategies.
 * Refused before any kernel: what rl_plane_generate refuses about the scene, with its codes; nb_primitive outside 1 .. RL_VPL_MAX, an unknown strategy, spp = 0,
 * a bad shard (RL_ERR_INVALID_ARGUMENT); 256 * spp * D > 2^32 - 1, the jump-ahead's reach (RL_ERR_UNSUPPORTED).  Reference-order streams, exact numerics, one
 * device, host output; shards as rl_render_bre.  Counters: camera_samples, extension_rays = camera_samples, shadow_rays = planes intersected, rng_draws =
 * camera_samples * D + 2 * redraws, kernel_launches, ms_other = the kernel; reserved[0] = direction redraws, reserved[1] = planes intersected, reserved[2] = of
 * those, visible. */
typedef enum rl_plane_type { RL_PLANE_UV = 0, RL_PLANE_VT = 1, RL_PLANE_UT = 2, RL_PLANE_UALPHAT = 3 } rl_plane_type;
typedef enum rl_plane_strategy { RL_PLANE_STRATEGY_UV = 0, RL_PLANE_STRATEGY_VT = 1, RL_PLANE_STRATEGY_UT = 2, RL_PLANE_STRATEGY_AVERAGE = 3,
                                 RL_PLANE_STRATEGY_DISCRETE_MIS = 4, RL_PLANE_STRATEGY_UALPHA = 5, RL_PLANE_STRATEGY_CMIS = 6 } rl_plane_strategy;
enum { RL_PLANE_WORDS = 18, RL_PLANE_TREE_GROUP_PLANES = 1024 };
typedef struct rl_plane_set rl_plane_set;       /* opaque: the planes of one generation */
typedef struct rl_plane_map rl_plane_map;       /* opaque: plane tree, planes and lights, on the context's device */
int rl_plane_generate(rl_context* ctx, uint32_t nb_primitive, int strategy, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats);
int rl_plane_info(const rl_plane_set* set, uint64_t* n_planes, uint64_t* number_plane_gen, int* strategy);
int rl_plane_read(const rl_plane_set* set, uint32_t* words, size_t n_words);
void rl_plane_destroy(rl_plane_set* set);
int rl_plane_tree_build(const uint32_t* words, size_t n_planes, size_t node_capacity, size_t* n_nodes, float* node_boxes, uint32_t* node_links, uint32_t* order);
int rl_plane_map_build(rl_context* ctx, const rl_plane_set* set, rl_plane_map** out);
int rl_plane_map_info(const rl_plane_map* map, uint64_t* n_planes, uint64_t* n_nodes, uint64_t* number_plane_gen, int* strategy);
int rl_plane_map_read(const rl_plane_map* map, size_t node_capacity, float* node_boxes, uint32_t* node_links, size_t plane_capacity, float* planes);
void rl_plane_map_destroy(rl_plane_map* map);
int rl_plane_generate_lanes(rl_context* ctx, uint32_t nb_primitive, int strategy, rl_sampler* sampler, rl_plane_set** out, rl_render_stats* stats);
int rl_plane_map_build_device(rl_context* ctx, const rl_plane_set* set, rl_plane_map** out, float* ms_kernels);
int rl_plane_tree_build_device(rl_context* ctx, const uint32_t* words, size_t n_planes, size_t node_capacity, size_t* n_nodes, float* node_boxes,
                               uint32_t* node_links, uint32_t* order);
int rl_render_plane_single(rl_context* ctx, const rl_plane_map* map, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                           const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats);
int rl_render_plane_uncorrelated(rl_context* ctx, uint32_t nb_primitive, int strategy, uint32_t spp, int32_t seed_variant, uint32_t shard_index, uint32_t shard_count,
                                 const uint64_t* block_seeds, size_t n_blocks, float* out_rgb, rl_render_stats* stats);

/* ---- IntegratorPointNormal { strategy, use_mis, warps, warps_strategy, splitting, use_aa } (src/integrators/explicit/point_normal.rs:1172-1179; CLI
 * `point-normal`, examples/cli.rs:209-224, 436-521): single scattering from the lights along the camera ray.  A plain compute_mc integrator like `ao` and
 * `direct`: no light pass, no tree.  Built: the seven plain strategies — compute_pixel (:2585-2633) with use_mis = false and splitting = None,
 * compute_single_tr (:2209-2284), compute_single_tr_phase (:2287-2334), compute_single_strategy (:2336-2453), create_distance_sampling's three arms without a
 * flavour bit (:1393, :1547, :1550), EquiAngularSampling::{new, new_clamping, sample} (:26-166), PointNormalSampling::{new, sample} (:660-739),
 * TransmittanceSampling::sample (:1087-1116), fix_random_sample_emitter's non-ATS arm (:1201-1216).  Left out: the Taylor / warp / "best" flavours, MIS,
 * splitting, ATS, the stratified sampler, several devices.
 * Draws per camera sample, after the 2 of the pixel jitter (none with use_aa = 0: the pixel centre): tr_ex 1 distance + 4 emitter (next, next, next2d);
 * tr_phase 1 + 2 phase; eq_ex 4 + 1; eq_phase 4 + 1 + 2; eq_clamped_ex and pn_ex 4, then 1 only when a distance sampler exists; eq_clamped_phase 4, then 3
 * only then (new_clamping / PointNormalSampling::new return None, :2364-2367; the point light's zero normal always does).  Every other early return comes
 * after all draws of its sample.  Defined where the reference panics: a sample whose equi-angular range is empty (assert!(theta_a < theta_b), :42) and a
 * transmittance sample that `exited` on an unbounded ray (:1093-1096) take their usual draws and add zero.  atan(x) = atan2f_det(x, 1), tan(x) =
 * sinf_det(x) / cosf_det(x) — it departs from libm's tan by this construction.
 * stream_mode: RL_STREAM_PER_SAMPLE (the per-pixel, per-sample fork of rl_render_ao) or RL_STREAM_REFERENCE_ORDER, the reference's image seed for seed: a
 * constant-count strategy enters the block's stream by jump-ahead, a data-dependent one takes a chain pass first (stats->ms_prepass) that records where every
 * pixel starts; the context option ref_single_pass walks every block on one lane instead (same bytes, same counters).
 * Refused before any kernel: no medium (the reference unwraps scene.volume), a scene built with the light tree (`-x ats`), a directional light (its
 * correct_flux is todo!()), an environment emitter, RL_STREAM_STRATIFIED: RL_ERR_UNSUPPORTED; no emitter: RL_ERR_NO_EMITTER; an unknown strategy or stream
 * mode, spp = 0, a bad shard: RL_ERR_INVALID_ARGUMENT; a jump-ahead frame with 256 * spp * D > 2^32 - 1: RL_ERR_UNSUPPORTED.  Exact numerics, one device, host
 * output; shards as rl_render_ao.  Counters: camera_samples; rng_draws, the exact count; extension_rays = camera rays + phase rays (the chain pass's rays are
 * not counted); shadow_rays = visible() calls; vertices = samples for which a distance sampler existed; kernel_launches, ms_other = k_pn_pixel.
 * The struct is declared in two statements: tests/test_abi_layout.py holds the ten structs above to their mirrors, tests/test_pn_abi.py holds this one. */
typedef enum rl_pn_strategy { RL_PN_TR_EX = 0, RL_PN_TR_PHASE = 1, RL_PN_EQ_EX = 2, RL_PN_EQ_PHASE = 3, RL_PN_EQ_CLAMPED_EX = 4, RL_PN_EQ_CLAMPED_PHASE = 5,
                              RL_PN_PN_EX = 6 } rl_pn_strategy;
struct rl_point_normal_params {
    uint32_t spp;               /* scene.nb_samples */
    int32_t strategy;           /* rl_pn_strategy: the names of cli.rs:455-492 without a flavour */
    int32_t use_aa;             /* !disable_aa (cli.rs:213, 516) */
    int32_t stream_mode;        /* rl_stream_mode: reference order or per sample */
    int32_t seed_variant;
    uint32_t shard_index, shard_count;
};
typedef struct rl_point_normal_params rl_point_normal_params;
void rl_point_normal_params_default(rl_point_normal_params* params);   /* cli.rs:209-224: strategy tr_ex, AA on; spp 1, reference order, one shard */
int rl_render_point_normal(rl_context* ctx, const rl_point_normal_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                           rl_render_stats* stats);

/* ---- IntegratorPointNormal with use_mis = true (point_normal.rs:2605-2612; CLI `point-normal -x`, here `point-normal-mis`: `point-normal -x` stays refused):
 * phase sampling and explicit light sampling combined with two or three distance samplers under the power heuristic.  Only the distance family of `strategy`
 * selects the function, the EX / PHASE bit is ignored: tr_* compute_multiple_tr (:2095-2206), eq_ex | eq_phase compute_multiple_equiangular (:1849-2091),
 * eq_clamped_* and pn_ex compute_multiple_strategy (:1560-1847); the two names of a family render the same bytes.  New beside rl_render_point_normal:
 * EquiAngularSampling::{inside_bound, pdf} (:135-175), PointNormalSampling::pdf (:741-754), TransmittanceSampling::pdf (:1118-1130), the non-ATS arm of
 * EmitterSampler::direct_pdf_ray / direct_pdf (emitter.rs:1537, 1574) and the four-pdf power heuristic, pdf_current^2 / sum of squares in the order of the
 * vec!, plain IEEE arithmetic: a 0 / 0 or inf / inf weight is NaN and reaches the colour as the reference's would.  Only the non-ATS arms are built.
 * Draws per camera sample after the 2 of the jitter, in order: tr 1 distance, 4 emitter, 2 phase = 7; eq 1 transmittance, 4 emitter, 1 equi-angular, 2 phase =
 * 8; clamped and pn 4 emitter, 2 phase, 1 transmittance, 1 equi-angular, and 1 more only when create_distance_sampling gave Some = 8 | 9.  Second rays: tr 1
 * visibility + 1 phase, the others 2 + 2.
 * Kept as the reference has them: compute_multiple_strategy and compute_multiple_equiangular scale the flux by FRAC_1_PI whatever the emitter is
 * (compute_multiple_tr uses correct_flux()); a point light adds nothing (its zero normal makes n . (-d) <= 0 in every explicit technique and no phase ray hits
 * it).  Defined where the reference panics: (1) an EquiAngularSampling::new whose assert!(theta_a < theta_b) (:42) would fire — built on the sampled light
 * position: the sample takes its usual draws, traces no second ray and adds zero; built to evaluate a pdf at a phase ray's hit: that contribution is zero;
 * (2) a transmittance sample that `exited` on an unbounded ray (:1093-1096): the usual draws, no second ray, zero.
 * Stream modes, shards, refusals and their codes are rl_render_point_normal's (a jump-ahead frame with 256 * spp * D > 2^32 - 1, D = 7 or 8 plus the jitter's
 * 2: RL_ERR_UNSUPPORTED; clamped and pn take the chain pass, stats->ms_prepass).  Counters: camera_samples; rng_draws, the exact count; extension_rays =
 * camera rays + phase rays traced; shadow_rays = visible() calls (none when n . (-d) <= 0 or t_light is zero or not finite); vertices = for tr and eq the
 * samples no defined panic ended, for clamped and pn the samples whose third sampler was Some; kernel_launches; ms_other = k_pnmis_pixel.
 * The struct has rl_point_normal_params' fields and is declared in two statements like it; tests/test_pnmis_abi.py holds it to its mirrors. */
struct rl_point_normal_mis_params {
    uint32_t spp;               /* scene.nb_samples */
    int32_t strategy;           /* rl_pn_strategy: only its distance family matters */
    int32_t use_aa;             /* !disable_aa */
    int32_t stream_mode;        /* rl_stream_mode: reference order or per sample */
    int32_t seed_variant;
    uint32_t shard_index, shard_count;
};
typedef struct rl_point_normal_mis_params rl_point_normal_mis_params;
void rl_point_normal_mis_params_default(rl_point_normal_mis_params* params);   /* strategy tr_ex, AA on; spp 1, reference order, one shard */
int rl_render_point_normal_mis(rl_context* ctx, const rl_point_normal_mis_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                               rl_render_stats* stats);

/* ---- IntegratorPointNormal's Taylor strategies (the six `*_taylor_ex` names of cli.rs:455-492; CLI `point-normal-taylor`: `point-normal -s <flavoured>` stays
 * refused): compute_single_strategy's EX arm (:2336-2453) over create_distance_sampling's Taylor arms (:1276-1290, :1404-1418).  The scattering angle is drawn
 * from a degree-six Taylor polynomial of the transmittance (`tr`) or of the Henyey-Greenstein phase function (`phase`) up to a clamp angle, by a Newton /
 * bisection inversion of at most 30 steps (math::newton_raphson_iterate, math.rs:136-225), and beyond it uniformly (eq, eq_clamped: TaylorSampling, :401-518)
 * or by the point-normal pdf (pn: PointNormalTaylorSampling with warp = None, :757-976).  Poly6 is point_normal_poly.rs:178-393.  Not built: the warp and
 * "best" flavours, Poly6::tr_phase, PolyClamped, Poly4, HybridSampling.
 * Draws of one camera sample: 2 jitter (none without AA), 4 emitter, then 1 distance only when the sampler is Some — either `new` can return None, so every
 * strategy takes the chain pass on reference-order streams (stats->ms_prepass, kernel_launches = 3).
 * RL_PN_TAYLOR_EQ_PHASE and RL_PN_TAYLOR_EQ_CLAMPED_PHASE in an Isotropic medium are the reference's plain eq_ex / eq_clamped_ex (:1278): the call forwards to
 * rl_render_point_normal, image and counters are its bytes.  RL_PN_TAYLOR_PN_PHASE with g = 0 (Isotropic counts as g = 0) meets assert!(g != 0.0) (:1414) at
 * every sample: RL_ERR_UNSUPPORTED.  Defined (kernels/pntaylor.hip.h has the list): powi is __powisf2's order, Newton's factor is 2^-9, a div_zero solver
 * gives the distance and pdf (0, 0) and so zero, EquiAngularSampling::new's assert (:42) is None.
 * Stream modes, shards, the other refusals and their codes are rl_render_point_normal's.  Counters: camera_samples; rng_draws, the exact count; extension_rays =
 * camera rays; shadow_rays = visible() calls; vertices = samples whose distance sampler was Some; ms_other = k_pn_pixel.
 * The struct has rl_point_normal_params' fields and is declared in two statements like it; tests/test_pntaylor_abi.py holds it to its mirrors. */
typedef enum rl_pn_taylor_strategy { RL_PN_TAYLOR_EQ_PHASE = 0, RL_PN_TAYLOR_EQ_TR = 1, RL_PN_TAYLOR_EQ_CLAMPED_PHASE = 2, RL_PN_TAYLOR_EQ_CLAMPED_TR = 3,
                                     RL_PN_TAYLOR_PN_TR = 4, RL_PN_TAYLOR_PN_PHASE = 5 } rl_pn_taylor_strategy;
struct rl_point_normal_taylor_params {
    uint32_t spp;               /* scene.nb_samples */
    int32_t strategy;           /* rl_pn_taylor_strategy */
    int32_t use_aa;             /* !disable_aa */
    int32_t stream_mode;        /* rl_stream_mode: reference order or per sample */
    int32_t seed_variant;
    uint32_t shard_index, shard_count;
};
typedef struct rl_point_normal_taylor_params rl_point_normal_taylor_params;
void rl_point_normal_taylor_params_default(rl_point_normal_taylor_params* params);   /* strategy eq_tr_taylor_ex, AA on; spp 1, reference order, one shard */
int rl_render_point_normal_taylor(rl_context* ctx, const rl_point_normal_taylor_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                                  rl_render_stats* stats);

/* ---- IntegratorPointNormal over the light tree (the reference's `-x ats point-normal`; CLI `point-normal-ats`: `point-normal -x ats` stays refused).  The
 * scene's emitters are built with the tree (rl_scene_build_emitters with build_ats); the sample bodies are rl_render_point_normal's (family RL_PN_ATS_PLAIN,
 * strategy an rl_pn_strategy) and rl_render_point_normal_taylor's (RL_PN_ATS_TAYLOR, an rl_pn_taylor_strategy) but for where the emitter position comes from.
 * Every strategy but the two tr_*: fix_random_sample_emitter's ATS arm (point_normal.rs:1217-1228) — next, next2d, LightSamplerATS::sample from the root with
 * LightBounds::importance_ray(ray, max_dist) (emitter.rs:975-1032: the closest point of the segment, acos_fast, the stored angles theta_o and theta_e), then
 * sample_position_tri.  tr_ex: the distance first, then random_sample_emitter_position_point(&p, None, ..) at the scattering point (:2237-2243).  tr_phase
 * takes no emitter sample and renders rl_render_point_normal's bytes of the same scene without the tree.
 * Draws of one camera sample behind the jitter's 2: tr_ex 4, tr_phase 3, eq_ex 4, eq_phase 6, eq_clamped_ex and pn_ex 3 | 4, eq_clamped_phase 3 | 6, the
 * Taylor names 3 | 4 (one less than over the power pick); the data-dependent ones take the chain pass, which walks the tree as the sample does.
 * Defined where the reference panics: importance_ray's assert!(cos_phi_0.is_finite()) (emitter.rs:1008; the cluster's centre on the ray's line, or its axis
 * normal to the plane of the segment's ends seen from the centre) gives the node importance 0; LightSamplerATS::new's assert that every emitter is a surface:
 * a scene with a point, directional or environment light is RL_ERR_UNSUPPORTED, as is a scene without the tree.  Kept: two children of importance 0 give
 * prob_left = 0.5.  The Taylor names' forward in an Isotropic medium (to the plain strategy over the tree) and the g = 0 refusal are
 * rl_render_point_normal_taylor's; stream modes, shards, the other refusals, their codes and the counters are rl_render_point_normal's (D in the reach check
 * 256 * spp * D is the count above plus the jitter's).  Not built: MIS over the tree, splitting, the warp and best flavours, point lights in the tree.
 * The struct has rl_point_normal_params' fields, then the family, and is declared in two statements like it; tests/test_pnats_abi.py holds it to its mirrors. */
typedef enum rl_pn_ats_family { RL_PN_ATS_PLAIN = 0, RL_PN_ATS_TAYLOR = 1 } rl_pn_ats_family;
struct rl_point_normal_ats_params {
    uint32_t spp;               /* scene.nb_samples */
    int32_t strategy;           /* family plain: an rl_pn_strategy | family Taylor: an rl_pn_taylor_strategy */
    int32_t use_aa;             /* !disable_aa */
    int32_t stream_mode;        /* rl_stream_mode: reference order or per sample */
    int32_t seed_variant;
    uint32_t shard_index, shard_count;
    int32_t family;             /* rl_pn_ats_family: which names `strategy` is one of */
};
typedef struct rl_point_normal_ats_params rl_point_normal_ats_params;
void rl_point_normal_ats_params_default(rl_point_normal_ats_params* params);   /* family plain, strategy eq_ex, AA on; spp 1, reference order, one shard */
int rl_render_point_normal_ats(rl_context* ctx, const rl_point_normal_ats_params* params, const uint64_t* block_seeds, size_t n_blocks, float* out_rgb,
                               rl_render_stats* stats);

/* Frames in flight behind one call (the progressive wrappers' passes, avg.rs:5-131 / equal_time.rs:4-66: N independent renders of one scene): frame f — block
 * seeds `block_seeds[f]`, host image `out_rgb[f]` (W*H*3 f32) — renders on `ctxs[f % k]` from host thread f % k, k = min(n_ctx, n_frames); `ctxs` are distinct
 * contexts of the same scene.  Returns when every frame is done; the images (and `stats[f]`, if not NULL) are those of `n_frames` rl_render_path calls one after
 * the other.  On an error the first failing thread's code is returned and rl_last_error carries its message; the other threads stop before their next frame
 * (frames not yet started are not rendered).  Every context in flight keeps its own render buffers (several GB at 1080p x 128 spp in reference-order streams)
 * until it is destroyed.  The process environment must not be changed (setenv / putenv) while frames are in flight: the library reads its test-only RL_* knobs
 * with getenv during a render. */
int rl_render_path_frames(rl_context* const* ctxs, size_t n_ctx, const rl_path_params* params,
                          const uint64_t* const* block_seeds, size_t n_blocks, size_t n_frames,
                          float* const* out_rgb, rl_render_stats* stats);

/* ---- the whole scene as ONE plain-old-data description ("SceneDesc POD: counts + pointers") ------------------
 * What a Rust host fills from `&Scene` (src/scene.rs:16-30) in one go instead of the builder calls above; the arrays are only read during
 * the call.  Equivalent to: rl_scene_create, rl_scene_set_camera_matrices (has_camera_matrices) or rl_scene_set_camera, rl_scene_add_bitmap (in order: their ids are 0, 1, ...), rl_scene_add_mesh
 * (in order), rl_scene_set_medium, rl_scene_add_point_light / _directional_light (in order), rl_scene_set_environment[_map],
 * rl_scene_enable_ats, rl_scene_build_emitters — with the same checks and error codes.
 * The structs below carry no size or version member: ZERO-INITIALISE them (memset / `= {0}` / Rust `std::mem::zeroed()`) before filling the fields you know —
 * fields added later (round 4: emission_type / _scale / _bitmap_id, has_camera_matrices / sample_to_camera / to_world) then read as 0 = the old behaviour
 * (EmissionType::Color, Camera::new from the scalar parameters); a consumer built against an older header must be rebuilt (the layout is checked by
 * tests/test_abi_layout.py against this header, the ctypes mirror and the Rust block of INTEGRATION.md). */
typedef struct rl_mesh_desc {          /* struct Mesh (src/geometry.rs:107-119) */
    const float* vertices; size_t n_vertices;      /* xyz */
    const uint32_t* indices; size_t n_triangles;   /* 3 per triangle */
    const float* normals;                          /* xyz per vertex or NULL */
    const float* uv;                               /* uv per vertex or NULL */
    rl_bsdf_desc bsdf;
    int32_t has_emission; float emission_rgb[3];   /* EmissionType::Color */
    int32_t emission_type; float emission_scale; int32_t emission_bitmap_id;   /* rl_emission_type; != RL_EMISSION_COLOR: as rl_scene_set_mesh_emission (needs has_emission and uv) */
} rl_mesh_desc;
typedef struct rl_bitmap_desc { uint32_t width, height; const float* rgb; } rl_bitmap_desc;
typedef struct rl_light_desc { int32_t kind;       /* 0 = PointEmitter { position = a }, 1 = DirectionalLight { direction = a } */
                               float a[3]; float intensity[3]; } rl_light_desc;
typedef struct rl_scene_desc {
    uint32_t width, height; float fov_degrees; int32_t fov_axis; float to_world[16]; int32_t flip;   /* Camera::new */
    const rl_mesh_desc* meshes; size_t n_meshes;
    const rl_bitmap_desc* bitmaps; size_t n_bitmaps;
    const rl_light_desc* lights; size_t n_lights;
    int32_t has_environment; float environment_rgb[3];            /* EnvironmentLightColor::Constant */
    uint32_t env_map_width, env_map_height; const float* env_map_rgb;   /* EnvironmentLightColor::Texture (0 x 0 / NULL: none) */
    int32_t has_medium; float sigma_a[3], sigma_s[3]; int32_t phase_type; float g;   /* HomogenousVolume */
    int32_t build_ats;                                             /* Scene::build_emitters(build_ats) */
    /* != 0: the camera is (width, height, sample_to_camera, to_world) as rl_scene_set_camera_matrices takes it — rustlight's own matrices; fov_degrees,
     * fov_axis and flip are ignored.  0: Camera::new from fov / flip (what scene files carry). */
    int32_t has_camera_matrices; float sample_to_camera[16];
} rl_scene_desc;
int rl_scene_create_from_desc(const rl_scene_desc* desc, rl_scene** out);

/* ---- several GPUs of one node behind one call ------------------------------------------------------
 * The reference merges its per-block bitmaps with `accumulate_bitmap` (src/integrators/mod.rs:445-448); here every GPU renders the
 * blocks b % N == g into its own zeroed framebuffer in HBM and ONE ncclReduce(sum, root = first device) over xGMI merges them —
 * device to device, no per-GPU download, no host adds; sums with zeros are exact, so the image equals the 1-GPU image bit for
 * bit.  One process: rl_multi owns N device contexts (BVHAccel::new once per device, untimed), an RCCL communicator clique
 * (ncclCommInitAll) and the per-device framebuffers.  `devices` = HIP ordinals, one per shard (NULL: round-robin over the
 * visible devices).  Shards that share a device (more shards than GPUs: a plumbing mode for tests) are added on that device
 * before the reduce; the communicator spans the distinct devices. */
typedef struct rl_multi rl_multi;
int rl_multi_create(const rl_scene* scene, const int* devices, int n_shards, rl_multi** out);
void rl_multi_destroy(rl_multi* m);
int rl_multi_info(const rl_multi* m, int* n_shards, int* n_comm_ranks, int* rccl_version);
/* Diagnostics as one JSON object (NUL-terminated, `capacity` bytes available): shards, RCCL version, communicator ranks, how the framebuffers are
 * merged ("ncclReduce(sum) onto device D" or "host sum (<why>)": when the communicator cannot be built or a reduce fails / exceeds
 * RL_MULTI_REDUCE_TIMEOUT_S the shards are still rendered on their GPUs and their sums added on the host — same bits —, with a line on stderr;
 * RL_MULTI_NO_FALLBACK=1 turns that into RL_ERR_HIP), and per device: name, CUs, shards, hipDeviceCanAccessPeer towards every other device; of the
 * last render: wall ms of the merge step and kernel ms per shard. */
int rl_multi_describe(const rl_multi* m, char* buf, size_t capacity);
/* Device and counters of one shard of the last rl_multi_render_path call (per-GPU kernel time: stats->ms_other [+ ms_prepass]). */
int rl_multi_shard_stats(const rl_multi* m, int shard, int* device, rl_render_stats* stats);
/* Integrator::compute over all shards: params->shard_index / shard_count are set per GPU by the call; `out_rgb` is a HOST
 * buffer of W*H*3 f32 (the framebuffer download from the root GPU is part of the call); `stats` = sums over the shards
 * (render_ms, ms_other: maximum).  Blocking. */
int rl_multi_render_path(rl_multi* m, const rl_path_params* params, const uint64_t* block_seeds, size_t n_blocks,
                         float* out_rgb, rl_render_stats* stats);

/* ---- the two other `compute_mc` integrators that reuse this path's kernels ---- */

/* struct IntegratorAO { max_distance: Option<f32>, normal_correction } (src/integrators/ao.rs:4-7; CLI `ao -d 1.0 -n`,
 * examples/cli.rs:149-154,856-865) and struct IntegratorDirect { nb_bsdf_samples, nb_light_samples }
 * (src/integrators/direct.rs:5-8; CLI `direct -b 1 -l 1`). */
typedef struct rl_mc_params {
    uint32_t spp;               /* scene.nb_samples */
    int32_t stream_mode;        /* rl_stream_mode */
    int32_t seed_variant;
    uint32_t shard_index, shard_count;
    int32_t has_max_distance;   /* ao: Option<f32> */
    float max_distance;
    int32_t normal_correction;  /* ao */
    uint32_t nb_bsdf_samples;   /* direct */
    uint32_t nb_light_samples;  /* direct */
    uint32_t reserved[4];
} rl_mc_params;

/* Integrator::compute for IntegratorAO (src/integrators/ao.rs:9-70). Same output / sharding contract as rl_render_path.  In RL_STREAM_REFERENCE_ORDER both
 * integrators run in two passes like `path` (stats->ms_prepass: the pass that records where every camera sample starts in its block's stream). */
int rl_render_ao(rl_context* ctx, const rl_mc_params* params, const uint64_t* block_seeds, size_t n_blocks,
                 float* out_rgb, int out_is_device, void* stream, rl_render_stats* stats);
/* Integrator::compute for IntegratorDirect (src/integrators/direct.rs:10-233): direct lighting with the power
 * heuristic `mis_weight` (src/integrators/mod.rs:462-478). */
int rl_render_direct(rl_context* ctx, const rl_mc_params* params, const uint64_t* block_seeds, size_t n_blocks,
                     float* out_rgb, int out_is_device, void* stream, rl_render_stats* stats);

/* Batched `Acceleration::trace` (src/accel.rs:292-315): rays (o, d, tnear=1e-4, tfar=MAX).
 * Host pointers.  mesh[i] = -1 on a miss. */
int rl_trace_batch(rl_context* ctx, size_t n, const float* origins, const float* directions,
                   float* t_out, float* u_out, float* v_out, int32_t* mesh_out, int32_t* tri_out);

/* Batched `Acceleration::visible` (src/accel.rs:316-343). visible_out[i] = 1 if unoccluded. */
int rl_visible_batch(rl_context* ctx, size_t n, const float* p0, const float* p1,
                     uint8_t* visible_out);

/* Bitmap::read_pfm (src/structure.rs:563-607): colour PFM, little endian ("-1.0"), rows stored bottom-up and returned
 * top-down, RGB f32.  `rgb == NULL` only reports the size; otherwise `capacity_floats >= 3 * w * h`. */
int rl_load_pfm(const char* path, uint32_t* width, uint32_t* height, float* rgb, size_t capacity_floats);
/* Bitmap::read (src/structure.rs:670-683): by extension — .pfm, .exr (read_exr: R, G, B of a scanline file, NONE / RLE / ZIPS / ZIP,
 * HALF / FLOAT / UINT), .png (8/16-bit), .jpg / .jpeg (baseline and progressive Huffman) or .tga (value / 255 as read_ldr_image does). */
int rl_load_image(const char* path, uint32_t* width, uint32_t* height, float* rgb, size_t capacity_floats);
/* Bitmap::save_pfm (src/structure.rs:547-560): bottom-up rows, |value|, little-endian, "-1.0" scale. */
int rl_save_pfm(const char* path, const float* rgb, uint32_t width, uint32_t height);

/* Bitmap::save_ldr_image (src/structure.rs:471-484) with Color::to_rgba (161-168): 8-bit RGB PNG,
 * (min(c, 1)^(1/2.2) * 255) as u8. */
int rl_save_png(const char* path, const float* rgb, uint32_t width, uint32_t height);
/* Bitmap::save_exr (src/structure.rs:490-527): scanline OpenEXR, FLOAT channels R, G, B, no compression. */
int rl_save_exr(const char* path, const float* rgb, uint32_t width, uint32_t height);
/* Bitmap::save (src/structure.rs:528-545): dispatch on the file extension (.pfm | .png | .exr). */
int rl_save_image(const char* path, const float* rgb, uint32_t width, uint32_t height);

/* Library/build info (for tests: which arch the kernels were compiled for). */
const char* rl_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* RUSTLIGHT_AMD_H */
