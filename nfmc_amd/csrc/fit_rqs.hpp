// f1 for spline couplings ('c-rqnsf'): launch interface of the gradient kernel in fit_rqs.hip (conditioner width <= 8,
// d <= 256, both losses).  The fold / AdamW / bookkeeping launch is fit_fold_kernel of fit_kernels.hip, unchanged.
#pragma once

#include "fit_rows.hpp"

namespace nfmc {

constexpr int kRqThreads = 256;   // four waves per workgroup
constexpr int kRqRows = 16;       // batch rows per workgroup tile
constexpr int kRqChunk = 16;      // target coordinates per chunk of the reverse sweep: kRqRows * kRqChunk = one (row, target) pair per thread
constexpr int kRqOut = 3 * kRqsBins - 1;
constexpr int kRqDrawStride = kRqRows + 1;   // odd: (target, output) threads read a row's deltas conflict-free
constexpr int64_t kRqMaxPartialBytes = (int64_t)64 << 20;

struct FitRqsArgs {
    NfmcRealNVP f;
    NfmcPotential pot;
    const float* x;
    int64_t n;
    const float* xv;
    int64_t nv;
    float* partial;
    int64_t pstride;
    int64_t ea_off;
    int d4;
    int64_t n_params;
    int64_t tiles, vtiles;
    const float* run_state;
};

__host__ __device__ inline size_t fit_rqs_lds_floats(int d, int hp) {
    return (size_t)2 * kRqRows * tile_stride(d) + (size_t)4 * kRqRows * hp + (size_t)kRqChunk * kRqOut * kRqDrawStride +
           (size_t)kRqRows * kRqChunk * hp;
}

// workgroups of a launch over n batch and nv validation rows: one per tile, at most 256 (the fold's tail sum), and never more
// slabs of partial gradients than 64 MiB hold
inline int fit_rqs_grid(int64_t n, int64_t nv, int64_t n_params) {
    const int64_t tiles = (n + kRqRows - 1) / kRqRows + (nv + kRqRows - 1) / kRqRows;
    int64_t cap = kRqMaxPartialBytes / ((n_params + kFitTailFloats) * (int64_t)sizeof(float));
    cap = cap > 256 ? 256 : (cap < 1 ? 1 : cap);
    return (int)(tiles < 1 ? 1 : (tiles < cap ? tiles : cap));
}

int fit_rqs_launch(bool rkl, int hp, const FitRqsArgs& a, int grid, hipStream_t st);

}  // namespace nfmc
