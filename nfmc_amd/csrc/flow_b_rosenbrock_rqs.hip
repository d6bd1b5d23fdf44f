// flow-MH register kernels of kind 5 (RosenbrockPot, the blocked Rosenbrock target), spline couplings, in a unit of their own,
// compiled in parallel with flow_b_kernels.hip: launch_b_kind, flow_b_mh.hpp
#include "flow_b_mh.hpp"
#include "pot_rosenbrock.hpp"

template int nfmc::launch_b_kind<nfmc::RosenbrockPot, nfmc::kRqsBins>(const NfmcFlowMhArgs&, nfmc::BCfg, int, int64_t, int, hipStream_t, bool);
