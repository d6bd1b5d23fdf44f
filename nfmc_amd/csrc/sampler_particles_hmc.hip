// hmc sampler kernels of kind 11 (ParticlePot, interacting particles) in a unit of their own, compiled in parallel
// with the others: launch_hmc_kind, sampler_impl.hpp
#include "sampler_impl.hpp"
#include "pot_particles.hpp"

template int nfmc::launch_hmc_kind<nfmc::ParticlePot>(const NfmcHmcArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, hipStream_t);
