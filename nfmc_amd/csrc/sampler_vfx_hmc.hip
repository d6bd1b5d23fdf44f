// hmc sampler kernels of kind 10 (VaryEffPot, varying-effects regression) in a unit of their own, compiled in parallel
// with the others: launch_hmc_kind, sampler_impl.hpp; launch_mclmc_kind, sampler_mclmc.hpp
#include "sampler_impl.hpp"
#include "sampler_mclmc.hpp"
#include "pot_vfx.hpp"

template int nfmc::launch_hmc_kind<nfmc::VaryEffPot>(const NfmcHmcArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, hipStream_t);
template int nfmc::launch_mclmc_kind<nfmc::VaryEffPot>(const NfmcMclmcArgs&, nfmc::Cfg, int64_t, int, hipStream_t);
