// beamgen_lds.hip — the photon beams' generation kernels (k_beam_generate, k_beam_shoot) for scenes staged in LDS; see beamgen.hip.h
#include "common.hip.h"
#include "beamgen.hip.h"

namespace rl {
void launch_beamgen_lds(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                       const VplConst& vc, const VplPathsConst& pc) {
    launch_beamgen_impl<true>(which, mat, grid, block, lds_bytes, st, rc, ds, stc, vc, pc);
}
}  // namespace rl
