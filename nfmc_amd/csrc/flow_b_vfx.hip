// flow-MH register kernels of kind 10 (VaryEffPot, varying-effects regression), affine couplings, in a unit of their own,
// compiled in parallel with flow_b_kernels.hip: launch_b_kind, flow_b_mh.hpp
#include "flow_b_mh.hpp"
#include "pot_vfx.hpp"

template int nfmc::launch_b_kind<nfmc::VaryEffPot, 0>(const NfmcFlowMhArgs&, nfmc::BCfg, int, int64_t, int, hipStream_t, bool);
