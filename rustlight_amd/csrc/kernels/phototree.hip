// phototree.hip — the device build of the photon tree: the kernels of phototree.hip.h and the host driver that strings them together
#include "phototree.hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../host/hip_buffer.h"
#include "phototree.h"

namespace rl {

unsigned photon_tree_node_count(unsigned n_photons) { return pt_node_count(n_photons); }

namespace {
// the ranges k_pt_finish takes: the first range on every way down that holds at most `group` photons
void finish_roots(unsigned b, unsigned e, unsigned node, unsigned group, std::vector<uint3>* out) {
    const unsigned m = e - b;
    if (m <= group) { out->push_back(make_uint3(b, e, node)); return; }
    const unsigned split = (b + e) / 2u;
    finish_roots(split, e, node + 1u, group, out);
    finish_roots(b, split, node + 1u + pt_node_count(m - m / 2u), group, out);
}
}  // namespace

int photon_tree_run(const PhotonTreeJob& job, hipStream_t st, bool timing, float* ms_kernels) {
    const unsigned n = job.n, group = std::min(std::max(job.group, 4u), kPtGroup);
    if (ms_kernels) *ms_kernels = 0.0f;
    if (n == 0) return RL_OK;
    const unsigned blocks = (n + kPtThreads - 1u) / kPtThreads;
    EventPair ev;
    int rcode;
    if ((rcode = ev.open(timing)) != RL_OK) return rcode;
    // ---- check pass: the one word that comes back
    HipBuffer<unsigned> d_flag;
    if ((rcode = d_flag.ensure(1)) != RL_OK) return rcode;
    unsigned flag = 0u;
    HIP_OK(hipMemsetAsync(d_flag.get(), 0, sizeof(unsigned), st));
    ev.begin(st);
    hipLaunchKernelGGL(k_pt_check, dim3(blocks), dim3(kPtThreads), 0, st, job.words, n, job.check_kind ? 1 : 0, d_flag.get());
    ev.end(st);
    HIP_OK(hipMemcpyAsync(&flag, d_flag.get(), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    ev.add();
    if (flag & 1u) { rl_set_error("a photon map takes volume records only: generate the set with RL_VPL_VOLUME"); return RL_ERR_INVALID_ARGUMENT; }
    if (flag & 2u) { rl_set_error("a photon position is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    if (!job.nodes) { if (ms_kernels) *ms_kernels = ev.ms; return RL_OK; }      // the check alone (a size-only call)
    // ---- the levels that run over the whole array: while the largest range holds more than `group` photons
    unsigned depth_global = 0u;
    for (unsigned cm = n; cm > group; cm = (cm + 1u) / 2u) depth_global++;
    unsigned p2 = 4u;
    while (p2 < group) p2 <<= 1;
    std::vector<uint3> roots;
    finish_roots(0u, n, 0u, group, &roots);
    HipBuffer<unsigned> d_order[2], d_acc;
    HipBuffer<unsigned long long> d_keys[2];
    HipBuffer<uint3> d_roots;
    if ((rcode = d_order[0].ensure(n)) != RL_OK || (rcode = d_roots.ensure(roots.size())) != RL_OK) return rcode;
    if (depth_global > 0u) {
        if ((rcode = d_order[1].ensure(n)) != RL_OK || (rcode = d_keys[0].ensure(n)) != RL_OK || (rcode = d_keys[1].ensure(n)) != RL_OK ||
            (rcode = d_acc.ensure((size_t)6u << depth_global)) != RL_OK) return rcode;
        HIP_OK(hipMemsetAsync(d_acc.get(), 0xff, ((size_t)6u << depth_global) * sizeof(unsigned), st));
    }
    HIP_OK(hipMemcpyAsync(d_roots.get(), roots.data(), roots.size() * sizeof(uint3), hipMemcpyHostToDevice, st));
    ev.begin(st);
    hipLaunchKernelGGL(k_pt_iota, dim3(blocks), dim3(kPtThreads), 0, st, d_order[0].get(), n);
    unsigned cur = 0u;
    unsigned cm = n;
    for (unsigned depth = 0; depth < depth_global; depth++, cm = (cm + 1u) / 2u) {
        const unsigned chunks = (n + group - 1u) / group;
        unsigned max_runs = (cm + group - 2u) / group + 1u, passes = 0u;      // a range of cm photons touches at most this many chunks
        while ((1u << passes) < max_runs) passes++;
        hipLaunchKernelGGL(k_pt_box, dim3(blocks), dim3(kPtThreads), 0, st, job.words, d_order[cur].get(), n, job.radius, depth, group, d_acc.get());
        hipLaunchKernelGGL(k_pt_sort, dim3(chunks), dim3(kPtThreads), 0, st, job.words, d_order[cur].get(), n, depth, group, p2, d_acc.get(), job.nodes, d_keys[0].get());
        unsigned kc = 0u;
        for (unsigned p = 0; p < passes; p++, kc ^= 1u)
            hipLaunchKernelGGL(k_pt_merge, dim3(blocks), dim3(kPtThreads), 0, st, d_keys[kc].get(), d_keys[kc ^ 1u].get(), n, depth, group, p);
        hipLaunchKernelGGL(k_pt_permute, dim3(blocks), dim3(kPtThreads), 0, st, d_keys[kc].get(), d_order[cur].get(), d_order[cur ^ 1u].get(), n, depth, group);
        cur ^= 1u;
    }
    // ---- every range of at most `group` photons: one workgroup each, down to the leaves
    unsigned* order_out = job.order ? job.order : d_order[cur].get();        // (a workgroup reads its range before it writes it)
    hipLaunchKernelGGL(k_pt_finish, dim3((unsigned)roots.size()), dim3(kPtThreads), 0, st, d_roots.get(), job.words, job.radius, d_order[cur].get(), order_out, job.nodes, p2);
    if (job.photons) hipLaunchKernelGGL(k_pt_photons, dim3(blocks), dim3(kPtThreads), 0, st, job.words, order_out, n, job.photons);
    ev.end(st);
    HIP_OK(hipStreamSynchronize(st));        // the scratch buffers go out of scope here
    HIP_OK(hipGetLastError());
    ev.add();
    if (ms_kernels) *ms_kernels = ev.ms;
    return RL_OK;
}

}  // namespace rl
