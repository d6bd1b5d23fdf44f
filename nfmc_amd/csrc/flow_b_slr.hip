// flow-MH register kernels of kind 7 (SparseLogRegPot, the sparse logistic regression), affine couplings, in a unit of their own,
// compiled in parallel with flow_b_kernels.hip: launch_b_kind, flow_b_mh.hpp
#include "flow_b_mh.hpp"
#include "pot_slr.hpp"

template int nfmc::launch_b_kind<nfmc::SparseLogRegPot, 0>(const NfmcFlowMhArgs&, nfmc::BCfg, int, int64_t, int, hipStream_t, bool);
