// mala sampler kernels of kind 11 (ParticlePot, interacting particles) in a unit of their own, compiled in parallel
// with the others: launch_mala_kind, sampler_impl.hpp
#include "sampler_impl.hpp"
#include "pot_particles.hpp"

template int nfmc::launch_mala_kind<nfmc::ParticlePot>(const NfmcMalaArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, float, hipStream_t);
