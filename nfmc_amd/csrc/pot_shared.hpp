// Device helpers that more than one potential kind uses.
#pragma once

#include "pot_kinds.hpp"

namespace nfmc {

// softplus(z) and sigmoid(z) from one e^-|z|: finite for every finite z.  log1p(e) is ln(1 + e) on v_log_f32 for
// e >= 2^-8 and the series e - e^2/2 + e^3/3 below (relative error < 2e-8 there), where 1 + e would drop e's low bits
__device__ __forceinline__ void softplus_sigmoid(float z, float& sp, float& sg) {
    const float e = fast_exp(-fabsf(z));                 // (0, 1]; 0 for |z| past ~104
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float l1p = e < 0x1p-8f ? e * fmaf(e, fmaf(e, 1.f / 3.f, -0.5f), 1.f) : fast_ln(1.f + e);
    sp = fmaxf(z, 0.f) + l1p;
    sg = (z >= 0.f ? 1.f : e) * inv;
}

// All threads of the workgroup: rows t0 .. t0 + rows - 1 of the row-major matrix src (`cols` floats per row) into the
// kLogRegTileFloats floats of `tile` as (kLogRegTileFloats / DP, DP), zero past column `cols` and past row `rows`.  Opens
// with the barrier after which no wave reads the previous tile; the caller closes with one after its own stores.
template <int DP>
__device__ __forceinline__ void load_tile_rows(float* tile, const float* src, int cols, int t0, int rows) {
    constexpr int kPer = kLogRegTileFloats / kBlock;   // floats per thread and tile
    static_assert(kLogRegTileFloats % kBlock == 0, "whole tiles per thread");
    __syncthreads();   // every wave is done with the previous tile
    float v[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {   // all loads in flight before the first LDS write
        const int e = threadIdx.x + k * kBlock, r = e / DP, j = e % DP;
        v[k] = (j < cols && r < rows) ? src[(int64_t)(t0 + r) * cols + j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) tile[threadIdx.x + k * kBlock] = v[k];
}

// The latent Gaussian kinds 12 and 13 (pot_lgm.hpp, pot_gmrf.hpp) put a Gaussian prior on f and a likelihood term
// l_j(f_j) on every coordinate.  latent_lik<LIK> is that term and its derivative for one coordinate (LIK 0 Poisson, 1 binomial,
// 2 Student-t; c0 = (nu+1)/2, c1 = 1/(nu s^2), c2 = nu s^2 of the table's header); an unobserved coordinate (w = 0, the
// padding included) gets exactly 0 for both, by a select, so that an overflowing e^f cannot turn 0 * inf into NaN.
// The register classes and the row forms share it.  log1p as in softplus_sigmoid.
template <int LIK>
__device__ __forceinline__ void latent_lik(float f, float y, float w, float c0, float c1, float c2, float& l, float& lp) {
    if constexpr (LIK == 0) {
        const float e = w * fast_exp(f);
        l = fmaf(-y, f, e);
        lp = e - y;
    } else if constexpr (LIK == 1) {
        float sp, sg;
        softplus_sigmoid(f, sp, sg);
        l = fmaf(w, sp, -y * f);
        lp = fmaf(w, sg, -y);
    } else {
        const float t = y - f, q = t * t, e = q * c1;
        const float l1p = e < 0x1p-8f ? e * fmaf(e, fmaf(e, 1.f / 3.f, -0.5f), 1.f) : fast_ln(1.f + e);
        l = w * c0 * l1p;
        lp = -2.f * w * c0 * t * __builtin_amdgcn_rcpf(c2 + q);
    }
    const bool on = w > 0.f;
    l = on ? l : 0.f;
    lp = on ? lp : 0.f;
}

constexpr int kFullRankJB = 8;   // outputs the dense row forms keep in registers per sweep (fullrank_value_grad_row)

// Potentials with an LDS block (kStaged) stage it behind the `img_floats` floats of flow image a kernel keeps at the
// start of its dynamic LDS (16-byte aligned), synchronise the workgroup and bind to it.  lds_with_potential()
// (pot_kinds.hpp) is the host side.
template <class P>
__device__ __forceinline__ void init_staged(P& pot, const NfmcPotential& p, int g, int d, float* lds, int img_floats) {
    float* blk = lds + ((img_floats + 3) & ~3);
    P::stage(blk, p, d);
    __syncthreads();
    pot.init(p, g, d, blk);
}

}  // namespace nfmc
