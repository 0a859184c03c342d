// beamgen_stream.hip — the photon beams' generation kernels (k_beam_generate, k_beam_shoot) for scenes whose BVH is streamed from L2 / HBM; see beamgen.hip.h
#include "common.hip.h"
#include "beamgen.hip.h"

namespace rl {
void launch_beamgen_stream(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                       const VplConst& vc, const VplPathsConst& pc) {
    launch_beamgen_impl<false>(which, mat, grid, block, lds_bytes, st, rc, ds, stc, vc, pc);
}
}  // namespace rl
