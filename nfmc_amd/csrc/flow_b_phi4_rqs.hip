// flow-MH register kernels of kind 8 (Phi4Pot, the phi^4 lattice field), spline couplings, in a unit of their own,
// compiled in parallel with flow_b_kernels.hip: launch_b_kind, flow_b_mh.hpp
#include "flow_b_mh.hpp"
#include "pot_phi4.hpp"

template int nfmc::launch_b_kind<nfmc::Phi4Pot, nfmc::kRqsBins>(const NfmcFlowMhArgs&, nfmc::BCfg, int, int64_t, int, hipStream_t, bool);
