// mala sampler kernels, jump-tail conditioner width 8 (0 = no jump tail): see sampler_impl.hpp
#include "sampler_impl.hpp"
#include "pot_basic.hpp"

namespace nfmc {
int launch_mala_j8(const NfmcMalaArgs& a, const JumpDev& jd, Cfg c, bool fast, int64_t tiles, int grid, float sqrt2h, hipStream_t st) {
    int rc = NFMC_EUNSUPPORTED;
#define M(CPL, LPC) \
    if (c.cpl == CPL && c.lpc == LPC) rc = launch_mala_cfg<CPL, LPC, 8>(a, jd, fast, tiles, grid, sqrt2h, st);
    NFMC_FOR_JUMP_CFG(M)
#undef M
    return rc;
}
}  // namespace nfmc
