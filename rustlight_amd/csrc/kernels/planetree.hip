// planetree.hip — the device build of the plane tree (host/planetree.cpp's tree, byte for byte): the kernels of phototree.hip.h over the plane element,
// the prepass that takes every plane's box and keys, the kernel that writes the planes in leaf order, and the host sequence around the shared driver
#include "phototree.hip.h"

#include "phototree.h"

namespace rl {

RL_ELEMENT_TREE_KERNELS(k_plt_, PlaneElem)
__global__ void __launch_bounds__(kPtThreads) k_plt_pre(const unsigned* words, unsigned n, float* pre, unsigned* flag) { plt_pre_body(words, n, pre, flag); }
__global__ void __launch_bounds__(kPtThreads) k_pt_planes(const unsigned* words, const unsigned* order, unsigned n, float4* planes) { plt_planes_body(words, order, n, planes); }

int plane_tree_run(const PlaneTreeJob& job, hipStream_t st, bool timing, float* ms_kernels) {
    const unsigned n = job.n;
    if (ms_kernels) *ms_kernels = 0.0f;
    if (n == 0) return RL_OK;
    const unsigned blocks = (n + kPtThreads - 1u) / kPtThreads;
    EventPair ev;
    int rcode;
    if ((rcode = ev.open(timing)) != RL_OK) return rcode;
    // ---- the prepass, which is the check pass too: the one word that comes back
    HipBuffer<unsigned> d_flag;
    HipBuffer<float> d_pre;
    if ((rcode = d_flag.ensure(1)) != RL_OK || (rcode = d_pre.ensure(9 * (size_t)n)) != RL_OK) return rcode;
    unsigned flag = 0u;
    HIP_OK(hipMemsetAsync(d_flag.get(), 0, sizeof(unsigned), st));
    ev.begin(st);
    hipLaunchKernelGGL(k_plt_pre, dim3(blocks), dim3(kPtThreads), 0, st, job.words, n, d_pre.get(), d_flag.get());
    ev.end(st);
    HIP_OK(hipMemcpyAsync(&flag, d_flag.get(), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    ev.add();
    if (flag) { rl_set_error("a plane corner is not finite"); return RL_ERR_INVALID_ARGUMENT; }
    if (!job.nodes) { if (ms_kernels) *ms_kernels = ev.ms; return RL_OK; }      // the check alone (a size-only call)
    const PlaneElem el{d_pre.get()};
    ElementTreeScratch<PlaneElem> scratch;
    const unsigned* order = nullptr;
    ev.begin(st);
    if ((rcode = element_tree_run<k_plt_Kernels>(el, n, job.group, job.nodes, job.order, st, &scratch, &order)) != RL_OK) return rcode;
    if (job.planes) hipLaunchKernelGGL(k_pt_planes, dim3(blocks), dim3(kPtThreads), 0, st, job.words, order, n, job.planes);
    ev.end(st);
    HIP_OK(hipStreamSynchronize(st));        // the scratch buffers go out of scope here
    HIP_OK(hipGetLastError());
    ev.add();
    if (ms_kernels) *ms_kernels = ev.ms;
    return RL_OK;
}

}  // namespace rl
