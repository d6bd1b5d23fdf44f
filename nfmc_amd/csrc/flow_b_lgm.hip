// flow-MH register kernels of kind 12 (LatentGaussPot, the latent Gaussian model), affine couplings, in a unit of their own,
// compiled in parallel with flow_b_kernels.hip: launch_b_kind, flow_b_mh.hpp
#include "flow_b_mh.hpp"
#include "pot_lgm.hpp"

template int nfmc::launch_b_kind<nfmc::LatentGaussPot, 0>(const NfmcFlowMhArgs&, nfmc::BCfg, int, int64_t, int, hipStream_t, bool);
