// OAC exploration action for twin critics and a policy of ONE hidden layer
// (expl_shallow.hip; the networks of OAC_KIND_SAC_SHALLOW): one workgroup per
// observation, no hand-off between workgroups.  The launchers take the
// ExplFusedArgs of the two-layer forms (kernels.h; the fc1 offsets, K, nq,
// ub_index, fail and the group scratch are unused).
#pragma once
#include "kernels.h"

namespace oac {

constexpr int kExplShallowMaxH = 512;
// dynamic LDS of a workgroup, bytes (a function of the dimensions alone)
size_t expl_shallow_lds_bytes(int Do, int Da, int H);
// all a.n observations in one launch
hipError_t launch_expl_shallow(const ExplFusedArgs& a, hipStream_t s);
// the single-observation call with the observation inside the kernel
// arguments and the outputs as tagged granules (a.n == 1, a.tags set, Do <= kExplObsArg)
hipError_t launch_expl_shallow_obs(const ExplFusedArgs& a, const ExplObsArg& obs, hipStream_t s);

}  // namespace oac
