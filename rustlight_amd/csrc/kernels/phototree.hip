// phototree.hip — the device build of the photon tree: the kernels of phototree.hip.h over the photon element and the host sequence around the shared driver
#include "phototree.hip.h"

#include "phototree.h"

namespace rl {

RL_ELEMENT_TREE_KERNELS(k_pt_, PhotonElem)
__global__ void __launch_bounds__(kPtThreads) k_pt_check(const unsigned* words, unsigned n, int check_kind, unsigned* flag) { pt_check_body(words, n, check_kind, flag); }
__global__ void __launch_bounds__(kPtThreads) k_pt_photons(const unsigned* words, const unsigned* order, unsigned n, float4* photons) { pt_photons_body(words, order, n, photons); }

unsigned photon_tree_node_count(unsigned n_photons) { return pt_node_count(n_photons); }

int photon_tree_run(const PhotonTreeJob& job, hipStream_t st, bool timing, float* ms_kernels) {
    const unsigned n = job.n;
    if (ms_kernels) *ms_kernels = 0.0f;
    if (n == 0) return RL_OK;
    const unsigned blocks = (n + kPtThreads - 1u) / kPtThreads;
    const PhotonElem el{job.words, job.radius};
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
    ElementTreeScratch<PhotonElem> scratch;
    const unsigned* order = nullptr;
    ev.begin(st);
    if ((rcode = element_tree_run<k_pt_Kernels>(el, n, job.group, job.nodes, job.order, st, &scratch, &order)) != RL_OK) return rcode;
    if (job.photons) hipLaunchKernelGGL(k_pt_photons, dim3(blocks), dim3(kPtThreads), 0, st, job.words, order, n, job.photons);
    ev.end(st);
    HIP_OK(hipStreamSynchronize(st));        // the scratch buffers go out of scope here
    HIP_OK(hipGetLastError());
    ev.add();
    if (ms_kernels) *ms_kernels = ev.ms;
    return RL_OK;
}

}  // namespace rl
