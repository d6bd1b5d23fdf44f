// Flow-MH register kernels for the sparse logistic regression (kind 7, SparseLogRegPot), affine couplings, in a
// translation unit of their own so that they compile in parallel with flow_b_kernels.hip: see flow_b_mh.hpp
#include "flow_b_mh.hpp"

namespace nfmc {

int flow_mh_b_slr(const NfmcFlowMhArgs& a, int cpl, int lpc, int hp, bool rqs, int64_t tiles, int grid, hipStream_t st,
                  bool dry) {
    if (rqs) return flow_mh_b_slr_rqs(a, cpl, lpc, hp, tiles, grid, st, dry);
    int rc = NFMC_EUNSUPPORTED;
#define M(CPL, LPC)                                                                                              \
    if (cpl == CPL && lpc == LPC)                                                                                \
        rc = hp == 4 ? launch_b_general<SparseLogRegPot, CPL, LPC, 4, 0>(a, tiles, grid, st, dry)                  \
                     : launch_b_general<SparseLogRegPot, CPL, LPC, 8, 0>(a, tiles, grid, st, dry);
    NFMC_FOR_BCFG(M)
#undef M
    return rc;
}

}  // namespace nfmc
