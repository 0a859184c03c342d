// knobs.h — the execution options of a device context (rl_context_set_option).  None of them changes a result: they pick between bit-identical
// forms of the same render (cross-checks of the tests) or tune the speculative chain pass (measurement sweeps, profiles/NEGATIVES.md).
//
// Where they come from: rl_context_create reads the process environment ONCE (RL_<NAME IN CAPITALS>) into the context's table — that is the only
// place the library's render path looks at the environment — and rl_context_set_option(ctx, "<name>", "<value>" | NULL) changes an entry afterwards.
// A render takes a copy of the table when it starts: rl_render_path and everything below it read that copy and never getenv(), so a render's
// configuration cannot change under it (VERDICT r5 weak 8 / ADVICE r4: 37 getenv calls inside a function that library-owned threads call concurrently).
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

namespace rl {

enum KnobId {
    // which form of reference-order streams runs (all bit-identical)
    K_REF_SINGLE_PASS,      // one pass through the persistent kernel (the form of rounds 1-2) instead of chain pass + evaluation pass
    K_STATE_BUDGET_MB,      // MB the recorded sampler states may take (default 24 GB): small values force several chunks
    K_NO_OVERLAP,           // the evaluation pass AFTER the chain pass instead of beside it
    K_CHAIN_SERIAL,         // k_stream_chain (one lane per block) instead of k_stream_spec
    K_CHAIN_NO_PRE,         // k_stream_chain on tiny scenes without the lane-parallel node / triangle records
    K_CHAIN_NO_TREELETS,    // k_stream_chain on streaming scenes without the 16-node treelet blocks
    K_SPEC_FORCE,           // k_stream_spec whatever the draws per sample (tests), also inside the kernel
    K_SPEC_DRAWS_PER_SAMPLE,// the draws a camera sample takes on this scene, for the choice between k_stream_spec and k_stream_chain (default: 150 with a medium, 12 without)
    K_ITEM_SHIFT,           // one block chain per 2^k lanes
    K_FUSED_DYNAMIC,        // persistent kernel: 0 static tile order, 1 work items from the dispenser
    K_FUSED_TAIL_BLOCKS,    // persistent kernel, per-sample streams in static tile order: the last T blocks that see the scene run at several lanes per pixel (0: off; default: auto)
    K_FUSED_TAIL_SPLIT,     // ... lanes per pixel of those blocks, a power of two (0 or 1: off; default: auto)
    K_FUSED_TAIL_NO_BUFFER_TEST, // test knob: the tail's parking buffer "cannot be allocated" (the render goes on without a tail)
    K_SHADOW_PACK_CAPACITY, // test knob: the tail form's packed shadow stage (trace.hip.h: occluded_packed) tests what it has whenever a lane holds this many candidate leaves (small scenes reach the flush)
    K_EVAL_SPLIT,           // lanes per pixel of the evaluation launches beside the chain pass (default 4)
    K_EVAL_MIN, K_EVAL_DIV, // a launch when 1 / div of the blocks still to come (at least min) have come in
    K_NO_EVENTS,            // no HIP events around the kernels (rl_render_stats.ms_* stay 0)
    K_QUEUE_DEBUG,
    // k_stream_spec's shape and windows (sweeps of round 4)
    K_SPEC_GROUP, K_SPEC_SUB, K_SPEC_CAP, K_SPEC_PROBE, K_SPEC_LEAD, K_SPEC_LEAD_MAX, K_SPEC_LEAD_VAR, K_SPEC_EXTRA, K_SPEC_DENSE, K_SPEC_DENSE_FRAC,
    K_SPEC_PROBE_EVERY, K_SPEC_KS, K_SPEC_KE, K_SPEC_SERIAL_RATIO, K_SPEC_NO_TRIVIAL, K_SPEC_LDS_LIMIT_TEST, K_SPEC_STATS, K_SPEC_WAVE_TIMES,
    K_SPEC_LDS_LEVELS,      // traversal-stack levels k_stream_spec keeps in LDS on scenes that stream their BVH (the rest in the global overflow buffer)
    K_VPL_BATCH_PATHS,      // rl_vpl_generate_paths: every batch of a generation holds this many light paths (tests: rounds and cuts at chosen places)
    K_PHOTON_TREE_GROUP_PHOTONS, // rl_photon_map_build_device: a workgroup finishes ranges of at most this many photons (tests: several global levels from a few hundred photons)
    K_PLANE_GENERATE_LANES, // rl_plane_generate forwards to rl_plane_generate_lanes (one lane per iteration; the same set, sampler and counters)
    K_PLANE_TREE_DEVICE,    // rl_plane_map_build forwards to rl_plane_map_build_device (the same map from device kernels)
    K_PLANE_TREE_GROUP_PLANES, // rl_plane_map_build_device: a workgroup finishes ranges of at most this many planes (tests, as photon_tree_group_photons)
    K_PPLANE_TREE_DEVICE,   // rl_pplane_map_build builds its plane tree with the device kernels of rl_plane_map_build_device (the same map)
    // read when the context is created only
    K_FORCE_STREAMING,      // keep small scenes out of LDS (the kernels that stream the BVH, on scenes the oracle finishes in seconds)
    K_GENERIC_LIGHTS,       // do not specialise the NEE code for area-light-only scenes
    K_COUNT
};

struct Knobs {
    struct Entry { bool set = false; std::string value; };
    Entry e[K_COUNT];

    static const char* name_of(int k) {
        static const char* const names[K_COUNT] = {
            "ref_single_pass", "state_budget_mb", "no_overlap", "chain_serial", "chain_no_pre", "chain_no_treelets", "spec_force", "spec_draws_per_sample", "item_shift",
            "fused_dynamic", "fused_tail_blocks", "fused_tail_split", "fused_tail_no_buffer_test", "shadow_pack_capacity", "eval_split", "eval_min", "eval_div", "no_events", "queue_debug",
            "spec_group", "spec_sub", "spec_cap", "spec_probe", "spec_lead", "spec_lead_max", "spec_lead_var", "spec_extra", "spec_dense", "spec_dense_frac",
            "spec_probe_every", "spec_ks", "spec_ke", "spec_serial_ratio", "spec_no_trivial", "spec_lds_limit_test", "spec_stats", "spec_wave_times", "spec_lds_levels", "vpl_batch_paths", "photon_tree_group_photons",
            "plane_generate_lanes", "plane_tree_device", "plane_tree_group_planes", "pplane_tree_device",
            "force_streaming", "generic_lights"};
        return names[k];
    }
    static int find(const char* name) {
        if (!name) return -1;
        for (int k = 0; k < K_COUNT; k++) if (std::strcmp(name, name_of(k)) == 0) return k;
        return -1;
    }
    // rl_context_create: RL_<NAME> of the process environment, once
    void from_environment() {
        for (int k = 0; k < K_COUNT; k++) {
            std::string env = "RL_";
            for (const char* p = name_of(k); *p; p++) env += (char)((*p >= 'a' && *p <= 'z') ? *p - 'a' + 'A' : *p);
            const char* v = std::getenv(env.c_str());
            e[k].set = v != nullptr;
            e[k].value = v ? v : "";
        }
    }
    bool has(int k) const { return e[k].set; }
    const char* str(int k) const { return e[k].set ? e[k].value.c_str() : nullptr; }
    long long i(int k, long long dflt) const { return e[k].set ? std::atoll(e[k].value.c_str()) : dflt; }
    double f(int k, double dflt) const { return e[k].set ? std::atof(e[k].value.c_str()) : dflt; }
};

}  // namespace rl
