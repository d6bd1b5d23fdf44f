// mala sampler kernels of kind 12 (LatentGaussPot, the latent Gaussian model) in a unit of their own, compiled in parallel
// with the others: launch_mala_kind, sampler_impl.hpp
#include "sampler_impl.hpp"
#include "pot_lgm.hpp"

template int nfmc::launch_mala_kind<nfmc::LatentGaussPot>(const NfmcMalaArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, float, hipStream_t);
