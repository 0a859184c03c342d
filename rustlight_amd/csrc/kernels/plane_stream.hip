// plane_stream.hip — the photon-plane gather with the BVH streamed from L2 / HBM; see plane.hip.h
#include "common.hip.h"
#include "plane.hip.h"

namespace rl {
void launch_plane_stream(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PlaneConst& pc) {
    launch_plane_impl<false>(mode, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
