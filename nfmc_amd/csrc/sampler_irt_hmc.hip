// hmc sampler kernels of kind 9 (IrtPot, item-response theory) in a unit of their own, compiled in parallel
// with the others: launch_hmc_kind, sampler_impl.hpp; launch_mclmc_kind, sampler_mclmc.hpp
#include "sampler_impl.hpp"
#include "sampler_mclmc.hpp"
#include "pot_irt.hpp"

template int nfmc::launch_hmc_kind<nfmc::IrtPot>(const NfmcHmcArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, hipStream_t);
template int nfmc::launch_mclmc_kind<nfmc::IrtPot>(const NfmcMclmcArgs&, nfmc::Cfg, int64_t, int, hipStream_t);
