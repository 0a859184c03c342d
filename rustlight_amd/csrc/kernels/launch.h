// launch.h — host-side launchers of the kernel families that live in their own translation units (fused_*.hip, fusedq_*.hip, fused_strat_*.hip,
// chain_*.hip, spec_*.hip, shade.hip, shade_strat.hip, mc.hip, mc_strat.hip, light_*.hip, vpl_*.hip, vpl_paths_*.hip, bre_*.hip, beamgen_*.hip, beam_*.hip, pplanegen_*.hip, pplane_*.hip, vrl_*.hip, plane_*.hip, uplane_*.hip, pn_*.hip, pnmis_*.hip, pntaylor_*.hip), so that the families compile in parallel, and
// the dispatcher every one of them maps its run-time arguments to template arguments with (with_bsdf, with_flag).  Launch errors are picked up by
// the caller's hipGetLastError().
#pragma once
#include <type_traits>

namespace rl {

// with_bsdf(mat, f): f(std::integral_constant<int, MAT>{}) for the scene's one BSDF type, MAT = -1 (the run-time switch per vertex) for a scene
// that mixes types.  Any other value also gets -1, in every family: the run-time switch is correct for any scene.
// The order of the cases is load-bearing: the kernels are instantiated, and so laid out in the code objects, in this order, and with `default`
// (-1) before BSDF_SUBSTRATE the objects of fused_*, fusedq_*, chain_* and spec_* disassemble exactly as before this dispatcher existed.  It is not
// a misplaced label; do not sort it to the end.
template <class F>
static void with_bsdf(int mat, F&& f) {
    switch (mat) {
        case BSDF_DIFFUSE: f(std::integral_constant<int, BSDF_DIFFUSE>{}); break;
        case BSDF_PHONG: f(std::integral_constant<int, BSDF_PHONG>{}); break;
        case BSDF_METAL: f(std::integral_constant<int, BSDF_METAL>{}); break;
        case BSDF_GLASS: f(std::integral_constant<int, BSDF_GLASS>{}); break;
        default: f(std::integral_constant<int, -1>{}); break;
        case BSDF_SUBSTRATE: f(std::integral_constant<int, BSDF_SUBSTRATE>{}); break;
    }
}
// with_flag(b, f): f(std::true_type{}) or f(std::false_type{})
template <class F>
static void with_flag(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// IntegratorAO / IntegratorDirect parameters (ao.rs:4-7, direct.rs:5-8)
struct McConst {
    int has_max_distance; float max_distance; int normal_correction;
    unsigned nb_bsdf_samples, nb_light_samples;
};

// IntegratorLightTracing (light.rs): what the light kernel needs beyond RenderConst / DeviceScene — the camera's inverse matrices and image
// rectangle (camera.rs:5-15, 54-58), kept out of DeviceScene so that no other kernel's argument block changes, and the fixed-point splat image.
struct LightConst {
    float camera_to_sample[16];         // column-major, as CameraRecord
    float to_local[16];
    float rect_min[2], rect_max[2];     // image_rect_min / image_rect_max
    int render_surface, render_volume;  // strategy all | surface | volume
    unsigned long long* accum;          // W*H*3 fixed-point sums, low 64 bits (light.hip.h: kLightFixBits)
    unsigned* inf_flags;                // W*H: bit c = channel c received a +inf splat
    unsigned* carry;                    // W*H*3 high 32 bits of the sums: how often the low word wrapped
};

// IntegratorVPL (vpl.hip.h): the VPL records, the generation's sampler and counters, and the per-sample gather buffers
static constexpr int kVplGatherWords = 12;       // gather point: [0] item, [1] kind bits, [2] prim, [3] u, [4] v, [5] t, [6..8] ray direction, [9..11] mrec.w
enum { VPL_GEN_VPLS = 0, VPL_GEN_PATHS = 1, VPL_GEN_VERTICES = 2, VPL_GEN_EXT = 3, VPL_GEN_DRAWS = 4, VPL_GEN_WORDS = 5 };
enum { STAT_VPL_SURFACE = 5, STAT_VPL_VOLUME = 6 };      // the gather's statistics rows (pathstate.hip.h: STAT_COUNT = 8): gather points on surfaces / in the medium
struct VplConst {
    unsigned nb_vpl, cap, max_paths;    // generation: stop once nb_vpl VPLs are stored or max_paths paths were shot; records beyond cap are not written
    int option_vpl, option_lt;          // rl_vpl_option
    unsigned* vpl_words;                // generation: [cap][kVplWords]
    unsigned long long* gen_state;      // [4] the main sampler, read and written back
    unsigned long long* gen_out;        // [VPL_GEN_WORDS] VPLs stored, paths shot, vertices, extension rays, draws
    const unsigned* vpls;               // gather: [n_vpl][kVplWords]
    unsigned n_vpl;
    float norm_vpl;                     // 1 / paths shot
    unsigned draws;                     // D: draws per camera sample (2, 3 with a medium)
    unsigned sample;                    // the sample index of this pass
    unsigned long long* pix_state;      // [pixel item][4] the pixel's place in its block stream
    unsigned* gpoints;                  // [pixel item][kVplGatherWords] this pass's live gather points
    unsigned* n_live;                   // how many
    float* acc;                         // [pixel item][3] the pixel's sum over the samples so far
};

// Light-path generation on per-path streams (vpl_paths.hip.h): one round's batch of path indices, the main sampler they fork from, and where the two passes write
enum { VPL_PATH_RECORDS = 0, VPL_PATH_VERTICES = 1, VPL_PATH_EXT = 2, VPL_PATH_DRAWS = 3, VPL_PATH_WORDS = 4 };
struct VplPathsConst {
    unsigned long long main[4];         // the main sampler's incoming state: path k is seeded by its k-th next_u64
    unsigned first, count;              // this launch walks paths first .. first + count - 1
    int option_vpl;                     // rl_vpl_option
    unsigned cap;                       // write pass: records vpl_words holds (records beyond it are not written)
    unsigned* vpl_words;                // write pass: [cap][kVplWords]
    const unsigned* offsets;            // write pass: [path] the record index the path's first record gets
    unsigned* counts;                   // count pass: [path - first][VPL_PATH_WORDS] records kept, vertices, extension rays, draws
};

// The camera-beam gather (gather.hip.h) the beam radiance estimate and the photon planes share.  block_stats sums 32-bit values over the workgroup, and a lane
// may enter more than 2^32 nodes over its samples: each 64-bit walk counter goes through it as its bits 0..23 in one statistics row and the bits from 24 up
// in another.  Nodes entered takes rows STAT_GATHER_NODES / _HI; a leaf's own counters take the rows it names.  The high rows are those of STAT_VERTICES /
// STAT_EXT_RAYS / STAT_SHADOW_RAYS, which the gather leaves empty (the host derives those counters).
enum { STAT_GATHER_NODES = 5, STAT_GATHER_NODES_HI = 1 };
RL_DEV void gather_split24(unsigned long long n, unsigned* lo, unsigned* hi) { *lo = (unsigned)n & 0xffffffu; *hi = (unsigned)(n >> 24); }
inline unsigned long long gather_merge24(const unsigned long long* totals, int lo, int hi) { return totals[lo] + (totals[hi] << 24); }

// The beam radiance estimate (bre.hip.h): the photon tree in visiting order and the photons in leaf order (host/photontree.cpp), the kernel's constants
enum { STAT_BRE_PHOTONS = 6, STAT_BRE_PHOTONS_HI = 3 };    // its leaf's statistics rows: photons gathered
struct BreConst {
    const float4* nodes;                // [n_nodes][2]: p_min.xyz, p_max.x | p_max.yz, skip, first << 3 | count
    const float4* photons;              // [n_photons][3]: pos | radiance | d_in
    unsigned n_nodes;
    float radius2;                      // radius * radius (radius.powi(2))
    float kernel;                       // 1 / (PI * radius^2)
    float norm_photon;                  // 1 / paths shot
};

// The photon beams (beam.hip.h): the beam tree in visiting order and the sub-beams in leaf order (host/beamtree.cpp), the kernel's constants
enum { STAT_BEAM_ACCEPTED = 6, STAT_BEAM_ACCEPTED_HI = 3 };    // its leaf's statistics rows: beams accepted
struct BeamConst {
    const float4* nodes;                // [n_nodes][2]: p_min.xyz, p_max.x | p_max.yz, skip, first << 3 | count
    const float4* beams;                // [n_sub][3]: o, length | d, 0 | radiance, 0
    unsigned n_nodes;
    float radius2;                      // self.radius * self.radius
    float half_inv_radius;              // 0.5 / self.radius
    float norm_photon;                  // 1 / paths shot
};

// The photon planes (pplanegen.hip.h, pplane.hip.h).  The plane pass stores two kinds of record: the planes go where VplConst / VplPathsConst say, the surface
// beams where PPlaneGenConst says.  The gather walks two trees: the beam tree with BeamLeaf's constants, then the plane tree.
// where the two generation kernels put the beam count: behind the counters they share with the beam pass
enum { PPLANE_GEN_BEAMS = VPL_GEN_WORDS, PPLANE_GEN_WORDS = VPL_GEN_WORDS + 1, PPLANE_PATH_BEAMS = VPL_PATH_WORDS, PPLANE_PATH_WORDS = VPL_PATH_WORDS + 1 };
struct PPlaneGenConst {
    unsigned* beam_words;               // [beam_cap][kBeamWords] (records beyond beam_cap are not written)
    unsigned beam_cap;
    unsigned beam_max;                  // k_pplane_generate: the loop ends once more beams than this are stored
    const unsigned* beam_offsets;       // k_pplane_shoot's write pass: [path] the record index the path's first beam gets
};
// the gather's statistics rows: all STAT_COUNT = 8, the samples being derived on the host (pplane.hip.h)
enum { STAT_PPLANE_BEAMS = 6, STAT_PPLANE_BEAMS_HI = 3, STAT_PPLANE_ISECT = 7, STAT_PPLANE_ISECT_HI = 2, STAT_PPLANE_VISIBLE = 0, STAT_PPLANE_VISIBLE_HI = 4 };
struct PPlaneConst {
    BeamConst beam;                     // the beam tree, the sub-beams and PhotonBeam's constants; beam.norm_photon serves the planes too
    const float4* nodes;                // the plane tree, [n_nodes][2]: p_min.xyz, p_max.x | p_max.yz, skip, first << 3 | count
    const float4* planes;               // [n_planes][4]: o, length0 | d0, length1 | d1, 0 | radiance, 0
    unsigned n_nodes;
};

// The virtual ray lights (vrl.hip.h): the surface beams' tree with BeamLeaf's constants, the VRLs in storing order, and what the chain pass hands the gather.
// The gather's statistics rows are the photon planes' eight: STAT_PPLANE_ISECT = VRLs that passed the roulette, STAT_PPLANE_VISIBLE = of those, visible
struct VrlConst {
    BeamConst beam;                     // the beam tree over the surface beams' sub-beams; beam.norm_photon serves the VRLs too
    const float4* vrls;                 // [n_vrl][3]: o, length | d, rr | radiance, 0
    unsigned n_vrl;
    unsigned* starts;                   // [owned block][256] the draw of the block's stream at which pixel c = ix * bh + iy starts: k_vrl_chain writes, k_vrl_gather reads
    unsigned* totals;                   // [owned block] the draws the block takes
};

// IntegratorSinglePlane (plane.hip.h): the rectangular lights, the generation's constants, and for the gather the plane tree in visiting order with the
// planes in leaf order (host/planetree.cpp)
struct PlaneLight { float o[3], u_l, u[3], v_l, v[3], pad0, n[3], pad1, emission[3], pad2; };      // RectangularLightSource, 5 float4
enum { PLANE_GEN_PLANES = 0, PLANE_GEN_ITERATIONS = 1, PLANE_GEN_DRAWS = 2, PLANE_GEN_WORDS = 3, PLANE_LANES_FLAG = 4, PLANE_LANES_WORDS = 5 };
struct PlaneGenConst {
    unsigned nb_primitive, cap;         // stop once nb_primitive planes are stored; records beyond cap are not written
    int strategy;                       // rl_plane_strategy
    unsigned n_lights;
    const PlaneLight* lights;
    float sigma_t[3], sigma_s[3];       // the medium's
    unsigned* words;                    // [cap][RL_PLANE_WORDS]
    unsigned long long* gen_state;      // [4] the main sampler, read and written back
    unsigned long long* gen_out;        // [PLANE_GEN_WORDS] planes stored, iterations (number_plane_gen), draws; k_plane_generate_lanes: [PLANE_LANES_WORDS] the sampler it leaves, the flag word
};
enum { STAT_PLANE_ISECT = 6, STAT_PLANE_VISIBLE = 7, STAT_PLANE_ISECT_HI = 2, STAT_PLANE_VISIBLE_HI = 3 };      // its leaf's statistics rows: planes intersected, of those visible
enum { PLANE_MODE_PLAIN = 0, PLANE_MODE_DISCRETE_MIS = 1, PLANE_MODE_CMIS = 2 };      // k_plane_gather's instantiations: a constant weight, DiscreteMIS, ContinousMIS
struct PlaneConst {
    const float4* nodes;                // [n_nodes][2]: p_min.xyz, p_max.x | p_max.yz, skip, first << 3 | count
    const float4* planes;               // [n_planes][4]: o, length0 | d0, length1 | d1, type + 4 * id_emitter | weight, 0
    const PlaneLight* lights;
    unsigned n_nodes;
    float w;                            // the strategy's constant weight: 1, or 1 / 3 for Average (DiscreteMIS computes its own)
    float n_lights_f;                   // emitters.len() as f32
    float inv_gen;                      // 1.0 / number_plane_gen as f32
};

// with_plane_mode(mode, f): f(std::integral_constant<int, MODE>{}) for MODE = PLANE_MODE_*
template <class F>
static void with_plane_mode(int mode, F&& f) {
    if (mode == PLANE_MODE_DISCRETE_MIS) f(std::integral_constant<int, PLANE_MODE_DISCRETE_MIS>{});
    else if (mode == PLANE_MODE_CMIS) f(std::integral_constant<int, PLANE_MODE_CMIS>{});
    else f(std::integral_constant<int, PLANE_MODE_PLAIN>{});
}
// IntegratorSinglePlaneUncorrelated (uplane.hip.h): every camera sample makes its own nb_primitive planes.  Its statistics rows are the plane gather's, and the
// direction redraws take the row of the nodes entered, which it has none of
enum { STAT_UPLANE_REDRAWS = STAT_GATHER_NODES };
struct UPlaneConst {
    const PlaneLight* lights;
    unsigned n_lights;
    unsigned nb_primitive;
    unsigned draws;                     // D: draws per camera sample without a redraw, 2 + nb_primitive * (7, or 8 when the plane type is drawn)
    int pick_type;                      // Average / DiscreteMIS: one more draw per plane picks UV / VT / UT
    unsigned type;                      // rl_plane_type of every plane otherwise
    float w;                            // the strategy's constant weight: 1, or 1 / 3 for Average (DiscreteMIS computes its own)
    float n_lights_f;                   // rect_lights.len() as f32
    float inv_nb;                       // 1.0 / nb_primitive as f32
};

// IntegratorPointNormal (pn.hip.h, and with use_mis pnmis.hip.h: k_pn_pixel and k_pn_chain are templates over the sample body, PnPlain<STRATEGY> or
// PnMis<FAMILY>).  How a lane of k_pn_pixel comes by its sampler: forked per sample from the pixel's seed (per-sample streams); the block's stream entered by
// jump-ahead (reference order, a constant number of draws per sample); the state k_pn_chain recorded for the pixel (reference order, a data-dependent
// number); or one lane per block walking the block's stream (reference order in a single pass)
enum { PN_MODE_PER_SAMPLE = 0, PN_MODE_ADVANCE = 1, PN_MODE_GIVEN = 2, PN_MODE_BLOCK = 3 };
struct PnConst {
    int use_aa;                         // 0: the pixel centre instead of the two jitter draws (-z)
    int mode;                           // PN_MODE_*
    unsigned draws;                     // PN_MODE_ADVANCE: D, the draws of one camera sample
    unsigned long long* pixel_states;   // [pixel item][4] the block sampler's state at the pixel's first sample: k_pn_chain writes, k_pn_pixel reads (PN_MODE_GIVEN)
    float taylor[8];                    // PnTaylor's phase strategies: Poly6::phase(g)'s seven coefficients and clamp_angle_phase(g), which the frame fixes (pntaylor_render.hip.h)
    const float* ats_angles;            // PnAtsPick: [light tree node][2] theta_o, theta_e as the host tree's LightBounds hold them (pnats_render.hip.h); null for the other kinds
};

// mat: the scene's one BSDF type, or -1 = run-time switch per vertex.  area_only: every emitter is a mesh area light and there is no light
// tree (the NEE code of the other emitter kinds is compiled out: same results, 84 -> 21 spilled VGPRs on the diffuse Cornell box)
void launch_fused_lds(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_fused_stream(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
// the same kernels built with RL_FAST_MATH (fused_*_fast.hip): rl_path_params.numerics = RL_NUMERICS_FAST
void launch_fused_lds_fast(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_fused_stream_fast(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
// the queue-fed form (exact build): the evaluation pass of reference-order streams beside the chain pass (fusedq_*.hip)
void launch_fusedq_lds(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_fusedq_stream(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
// k_stream_chain (chain.hip.h): first pass of reference-order streams — one lane per 16x16 block records the sampler state at the start of every sample
void launch_chain_lds(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_chain_stream(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_chain_lds_fast(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_chain_stream_fast(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
// k_stream_spec (spec.hip.h): the same first pass with every lane busy — windows of the stream walked speculatively per pixel, the chain threaded through them
void launch_spec_lds(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const SpecConf& spc);
void launch_spec_stream(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const SpecConf& spc);
void launch_trace_batch_fast(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const DeviceScene& ds, const StackConf& stc, unsigned n, const float* o, const float* d, float* t_out,
                             int* mesh_out, int* tri_out, int* steps_out);   // test hook: the tolerance build's BVH4 traversal, batched
void launch_shade_type(int type, bool medium, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool);
void launch_shade_sorted(bool medium, unsigned chunks, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool);
// RL_STREAM_STRATIFIED (sampler.hip.h: StratSampler): the persistent kernel for the run-time material switch (fused_strat_*.hip), the wavefront pipeline's
// raygen / material-sorted shade (shade_strat.hip), ao / direct (mc_strat.hip)
void launch_fused_strat_lds(bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_fused_strat_stream(bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc);
void launch_raygen_strat(dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool);
void launch_shade_sorted_strat(bool medium, unsigned chunks, dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const Pool& pool);
void launch_pixel_mc_strat(int kind, bool lds_scene, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const McConst& mp);
void launch_pixel_mc(int kind, bool lds_scene, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const McConst& mp);
void launch_mc_chain(int kind, bool lds_scene, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const McConst& mp);   // first pass of reference-order streams for ao / direct
// IntegratorLightTracing (light.hip.h): k_light_fused over the light-path slots (mat as for launch_fused_*), k_light_resolve turns the fixed-point sums into the f32 image
void launch_light_lds(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const LightConst& lc);
void launch_light_stream(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const LightConst& lc);
void launch_light_resolve(dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const LightConst& lc);
// IntegratorVPL (vpl.hip.h): which = 0 k_vpl_generate, 1 k_vpl_gather (mat as for launch_light_*), 2 k_vpl_primary; k_vpl_resolve scales the pixel sums into the image
void launch_vpl_lds(int which, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplConst& vc);
void launch_vpl_stream(int which, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplConst& vc);
void launch_vpl_resolve(dim3 grid, dim3 block, hipStream_t st, const RenderConst& rc, const VplConst& vc);
// rl_vpl_generate_paths (vpl_paths.hip.h): k_vpl_shoot over a batch of light paths, write = false the count pass, true the write pass (mat as for launch_vpl_*)
void launch_vpl_paths_lds(bool write, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplPathsConst& pc);
void launch_vpl_paths_stream(bool write, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplPathsConst& pc);
// IntegratorVolPrimitives' beam radiance estimate (bre.hip.h): k_bre_gather over the owned blocks; hg: the medium's phase function is Henyey-Greenstein
void launch_bre_lds(bool hg, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BreConst& bc);
void launch_bre_stream(bool hg, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BreConst& bc);
// The photon beams: the beam pass (beamgen.hip.h; which = 0 k_beam_generate reading vc as k_vpl_generate does, 1 / 2 k_beam_shoot's count / write pass reading pc as
// k_vpl_shoot does, mat as for launch_vpl_*; the scene has a medium) and k_beam_gather over the owned blocks (beam.hip.h)
void launch_beamgen_lds(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                        const VplConst& vc, const VplPathsConst& pc);
void launch_beamgen_stream(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                           const VplConst& vc, const VplPathsConst& pc);
void launch_beam_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BeamConst& bc);
void launch_beam_stream(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BeamConst& bc);
// The photon planes: the plane pass (pplanegen.hip.h; which and mat as for launch_beamgen_*, xc: where the surface beams go) and k_pplane_gather over the owned blocks (pplane.hip.h)
void launch_pplanegen_lds(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                          const VplConst& vc, const VplPathsConst& pc, const PPlaneGenConst& xc);
void launch_pplanegen_stream(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                             const VplConst& vc, const VplPathsConst& pc, const PPlaneGenConst& xc);
void launch_pplane_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PPlaneConst& pc);
void launch_pplane_stream(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PPlaneConst& pc);
// The virtual ray lights (vrl.hip.h): k_vrl_chain, one lane per owned block (rc.n_owned of them), then k_vrl_gather over the owned blocks
void launch_vrl_chain(hipStream_t st, const RenderConst& rc, const VrlConst& vc);
void launch_vrl_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VrlConst& vc);
void launch_vrl_stream(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VrlConst& vc);
// IntegratorSinglePlane (plane.hip.h): k_plane_generate on one lane, k_plane_generate_lanes on one lane per iteration (plane_generate.hip); k_plane_gather over the owned blocks, mode = PLANE_MODE_*
void launch_plane_generate(hipStream_t st, const PlaneGenConst& gc);
void launch_plane_generate_lanes(hipStream_t st, const PlaneGenConst& gc, unsigned n_gen);      // k_plane_generate_lanes: one lane per iteration, n_gen of them
void launch_plane_lds(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PlaneConst& pc);
void launch_plane_stream(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PlaneConst& pc);
// IntegratorSinglePlaneUncorrelated (uplane.hip.h): k_uplane over the owned blocks, mode = PLANE_MODE_*
void launch_uplane_lds(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const UPlaneConst& uc);
void launch_uplane_stream(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const UPlaneConst& uc);
// IntegratorPointNormal (pn.hip.h): chain = false k_pn_pixel<.., PnPlain<strategy>> over the pixel items (or, PN_MODE_BLOCK, the owned blocks), true
// k_pn_chain<.., PnPlain<strategy>> over the owned blocks; strategy = rl_pn_strategy
void launch_pn_lds(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
void launch_pn_stream(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
// IntegratorPointNormal with use_mis (pnmis.hip.h): chain = false k_pn_pixel<.., PnMis<family>>, true k_pn_chain<.., PnMis<family>> (clamped and pn);
// family = PNMIS_* (0 tr, 1 eq, 2 clamped, 3 pn); the constants are point-normal's PnConst and PN_MODE_*
void launch_pnmis_lds(bool chain, int family, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
void launch_pnmis_stream(bool chain, int family, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
// IntegratorPointNormal's Taylor strategies (pntaylor.hip.h): chain = false k_pn_pixel<.., PnTaylor<strategy>>, true k_pn_chain<.., PnTaylor<strategy>> (every
// strategy's count depends on the data); strategy = rl_pn_taylor_strategy; the constants are point-normal's PnConst, with pc.taylor for the phase polynomials
void launch_pntaylor_lds(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
void launch_pntaylor_stream(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
// IntegratorPointNormal over the light tree (pnats.hip.h): chain = false k_pn_pixel<.., PnAts<family, strategy>>, true k_pn_chain<.., PnAts<family, strategy>>
// (the Taylor names and the three plain strategies whose sampler can be None); selector = 8 * rl_pn_ats_family + the strategy within the family; the constants
// are point-normal's PnConst with pc.ats_angles, and pc.taylor for the phase polynomials
void launch_pnats_lds(bool chain, int selector, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
void launch_pnats_stream(bool chain, int selector, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc);
void dump_stage_timers(bool lds_scene);   // dev-only (-DRL_STAGE_TIMERS)
void dump_stage_timers_stream();
void dump_chain_timers_lds();      // dev-only (-DRL_STAGE_TIMERS): cycle shares of k_stream_chain's stages
void dump_chain_timers_stream();

}  // namespace rl
