// mala sampler kernels for the sparse logistic regression (kind 7, SparseLogRegPot), every jump-tail width, in a
// translation unit of their own so that they compile in parallel with the other units: see sampler_impl.hpp
#include "sampler_impl.hpp"

namespace nfmc {
int launch_mala_slr(const NfmcMalaArgs& a, const JumpDev& jd, Cfg c, int jhp, int64_t tiles, int grid, float sqrt2h,
                    hipStream_t st) {
    int rc = NFMC_EUNSUPPORTED;
#define M0(CPL, LPC) \
    if (jhp == 0 && c.cpl == CPL && c.lpc == LPC) rc = launch_mala_general_cfg<SparseLogRegPot, CPL, LPC, 0>(a, jd, tiles, grid, sqrt2h, st);
#define M4(CPL, LPC) \
    if (jhp == 4 && c.cpl == CPL && c.lpc == LPC) rc = launch_mala_general_cfg<SparseLogRegPot, CPL, LPC, 4>(a, jd, tiles, grid, sqrt2h, st);
#define M8(CPL, LPC) \
    if (jhp == 8 && c.cpl == CPL && c.lpc == LPC) rc = launch_mala_general_cfg<SparseLogRegPot, CPL, LPC, 8>(a, jd, tiles, grid, sqrt2h, st);
    NFMC_FOR_DEFAULT_CFG(M0)
    NFMC_FOR_BCFG(M4)
    NFMC_FOR_BCFG(M8)
#undef M0
#undef M4
#undef M8
    return rc;
}
}  // namespace nfmc
