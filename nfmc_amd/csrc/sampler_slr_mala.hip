// mala sampler kernels of kind 7 (SparseLogRegPot, the sparse logistic regression) in a unit of their own, compiled in parallel
// with the others: launch_mala_kind, sampler_impl.hpp
#include "sampler_impl.hpp"
#include "pot_slr.hpp"

template int nfmc::launch_mala_kind<nfmc::SparseLogRegPot>(const NfmcMalaArgs&, const nfmc::JumpDev&, nfmc::Cfg, int, int64_t, int, float, hipStream_t);
