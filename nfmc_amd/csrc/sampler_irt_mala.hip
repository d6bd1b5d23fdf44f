// mala sampler kernels of kind 9 (IrtPot, item-response theory) in a unit of their own, compiled in parallel
// with the others: launch_mala_kind, sampler_impl.hpp
#include "sampler_impl.hpp"
#include "pot_irt.hpp"

template int nfmc::launch_mala_kind<nfmc::IrtPot>(const NfmcMalaArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, float, hipStream_t);
