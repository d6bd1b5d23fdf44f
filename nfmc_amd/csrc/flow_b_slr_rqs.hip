// Flow-MH register kernels for the sparse logistic regression (kind 7, SparseLogRegPot), spline couplings: see
// flow_b_mh.hpp
#include "flow_b_mh.hpp"

namespace nfmc {

int flow_mh_b_slr_rqs(const NfmcFlowMhArgs& a, int cpl, int lpc, int hp, int64_t tiles, int grid, hipStream_t st,
                      bool dry) {
    int rc = NFMC_EUNSUPPORTED;
#define M(CPL, LPC)                                                                                              \
    if (cpl == CPL && lpc == LPC)                                                                                \
        rc = hp == 4 ? launch_b_general<SparseLogRegPot, CPL, LPC, 4, kRqsBins>(a, tiles, grid, st, dry)           \
                     : launch_b_general<SparseLogRegPot, CPL, LPC, 8, kRqsBins>(a, tiles, grid, st, dry);
    NFMC_FOR_BCFG(M)
#undef M
    return rc;
}

}  // namespace nfmc
