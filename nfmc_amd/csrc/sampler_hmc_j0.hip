// hmc sampler kernels, jump-tail conditioner width 0 (0 = no jump tail): see sampler_impl.hpp; and the mclmc kernels of
// kinds 0 to 3 (sampler_mclmc.hpp), which have no jump tail
#include "sampler_impl.hpp"
#include "sampler_mclmc.hpp"
#include "pot_basic.hpp"

namespace nfmc {
int launch_hmc_j0(const NfmcHmcArgs& a, const JumpDev& jd, Cfg c, bool fast, int64_t tiles, int grid, hipStream_t st) {
    int rc = NFMC_EUNSUPPORTED;
#define M(CPL, LPC) \
    if (c.cpl == CPL && c.lpc == LPC) rc = launch_hmc_cfg<CPL, LPC, 0>(a, jd, fast, tiles, grid, st);
    NFMC_FOR_CFG(M)
#undef M
    return rc;
}

int launch_mclmc_j0(const NfmcMclmcArgs& a, Cfg c, int64_t tiles, int grid, hipStream_t st) {
    switch (a.pot.kind) {
    case NFMC_POT_QUADRATIC: return launch_mclmc_kind<QuadraticPot>(a, c, tiles, grid, st);
    case NFMC_POT_FUNNEL: return launch_mclmc_kind<FunnelPot>(a, c, tiles, grid, st);
    case NFMC_POT_GAUSSIAN_MIXTURE: return launch_mclmc_kind<MixturePot>(a, c, tiles, grid, st);
    case NFMC_POT_LOGISTIC_REGRESSION: return launch_mclmc_kind<LogRegPot>(a, c, tiles, grid, st);
    }
    return NFMC_EUNSUPPORTED;
}
}  // namespace nfmc
