// Full-rank Gaussian (kind 4): its register class and its one-row NeuTra form.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

// Full-rank Gaussian (NFMC_POT_GAUSSIAN_FULL; Lambda (d, d) row-major in a, mu (d,) in b, d = p.n_components):
//   U = 1/2 r^T Lambda r,   dU/dx = Lambda r,   r = x - mu
// Lambda streams through the same LDS tile as the logistic regression's X (load_tile_rows: T = kLogRegTileFloats / DP
// rows of DP floats, zero-padded), so the same rule holds: every thread of the workgroup calls prepare() equally often.
// One pass over the rows: rows 4 b .. 4 b + 3 of Lambda belong to coordinates 4 b .. 4 b + 3, which are register quad
// b / LPC of lane b % LPC of the chain.  That lane's four r_i are broadcast to the chain's LPC lanes (ds_bpermute;
// v_readlane when one chain fills the wave; nothing with one lane per chain), and every lane adds r_i Lambda_ij to its
// own coordinates j: row i is column i (symmetry), read as one ds_read_b128 per register quad at 4 (q LPC + g) -- the
// gradient pass of LogRegPot with r_i in place of the residuals, no reduction per row.  U = 1/2 sum_j r_j g_j is
// lane-local, then ONE group_allreduce.  Padding coordinates have r = 0 and zero rows / columns, so d need not be a
// multiple of 4.  d^2 FMAs per chain and evaluation, d^2 / LPC per lane.
template <int CPL, int LPC, bool FAST>
struct GaussFullPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int T = kLogRegTileFloats / DP;   // rows of Lambda per tile
    static_assert(T % 4 == 0, "whole register quads per tile");
    float* tile;          // LDS: Lambda rows (T, DP)
    const float* lam;
    int dd;
    int grp;              // byte address of the chain's first lane for ds_bpermute
    bool lead;            // this lane holds coordinate 0 in register 0
    float mu[CPL];        // 0 for padding
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        lam = p.a;
        dd = d;
        grp = 4 * ((int)(threadIdx.x & 63) - g);
        lead = (g == 0);
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            mu[i] = c < d ? p.b[c] : 0.f;
        }
    }
    // value v of lane `src` (uniform) of this lane's chain group
    __device__ __forceinline__ float from_lane(float v, int src) const {
        if constexpr (LPC == 1) return v;
        else if constexpr (LPC == 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(grp + 4 * src, __float_as_int(v)));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        Ctx cx;
        float r[CPL];
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            r[i] = coord_of<CPL, LPC>(g, i) < dd ? x[i] - mu[i] : 0.f;
            cx.gr[i] = 0.f;
        }
        for (int t0 = 0; t0 < dd; t0 += T) {
            const int rows = dd - t0 < T ? dd - t0 : T;
            load_tile_rows<DP>(tile, lam, dd, t0, rows);
            __syncthreads();
            const int b1 = (t0 + rows + 3) >> 2;   // register quads (4 rows each) of this tile: t0 / 4 .. b1 - 1
            for (int b = t0 >> 2; b < b1;) {
                const int q = b / LPC;             // the quad's register index, constant over LPC consecutive quads
                float rq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < CPL / 4; ++k)
                    if (k == q) {
                        rq[0] = r[4 * k];
                        rq[1] = r[4 * k + 1];
                        rq[2] = r[4 * k + 2];
                        rq[3] = r[4 * k + 3];
                    }
                const int bq = b1 < (q + 1) * LPC ? b1 : (q + 1) * LPC;
                for (; b < bq; ++b) {
                    const int src = b - q * LPC;   // the lane that holds coordinates 4 b .. 4 b + 3
                    const float ri[4] = {from_lane(rq[0], src), from_lane(rq[1], src), from_lane(rq[2], src),
                                         from_lane(rq[3], src)};
                    const float* rows4 = tile + (4 * b - t0) * DP + 4 * g;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int k = 0; k < CPL / 4; ++k) {
                            const float4 w = *reinterpret_cast<const float4*>(rows4 + c * DP + 4 * k * LPC);
                            cx.gr[4 * k] = fmaf(ri[c], w.x, cx.gr[4 * k]);
                            cx.gr[4 * k + 1] = fmaf(ri[c], w.y, cx.gr[4 * k + 1]);
                            cx.gr[4 * k + 2] = fmaf(ri[c], w.z, cx.gr[4 * k + 2]);
                            cx.gr[4 * k + 3] = fmaf(ri[c], w.w, cx.gr[4 * k + 3]);
                        }
                    }
                }
            }
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) s = fmaf(r[i], cx.gr[i], s);
        cx.u = 0.5f * group_allreduce<LPC>(s);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Full-rank Gaussian (NFMC_POT_GAUSSIAN_FULL) for the row of one chain, as potential_value_grad_row:
//   U = 1/2 r^T Lambda r,   grow = Lambda r,   r = x - mu
// Lambda and mu are wave-uniform, so the compiler reads them with scalar loads.  A block of kFullRankJB outputs stays in
// registers while the loop runs over i: one LDS read of x_i feeds kFullRankJB FMAs with row i of Lambda (= column i, by
// symmetry).  Kept out of potential_value_grad_row, which the fit and DLMC kernels share and which never see kind 4.
__device__ __forceinline__ float fullrank_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                         const NfmcPotential& p, int d) {
    const float* __restrict__ lam = p.a;
    const float* __restrict__ mu = p.b;
    float u = 0.f;
    int j0 = 0;
    for (; j0 + kFullRankJB <= d; j0 += kFullRankJB) {
        float acc[kFullRankJB];
#pragma unroll
        for (int k = 0; k < kFullRankJB; ++k) acc[k] = 0.f;
        for (int i = 0; i < d; ++i) {
            const float ri = row[i] - mu[i];
            const float* __restrict__ li = lam + (int64_t)i * d + j0;
#pragma unroll
            for (int k = 0; k < kFullRankJB; ++k) acc[k] = fmaf(li[k], ri, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < kFullRankJB; ++k) {
            grow[j0 + k] = acc[k];
            u = fmaf(row[j0 + k] - mu[j0 + k], acc[k], u);
        }
    }
    for (; j0 < d; ++j0) {   // the last d % kFullRankJB outputs
        float acc = 0.f;
        for (int i = 0; i < d; ++i) acc = fmaf(lam[(int64_t)i * d + j0], row[i] - mu[i], acc);
        grow[j0] = acc;
        u = fmaf(row[j0] - mu[j0], acc, u);
    }
    return 0.5f * u;
}

}  // namespace nfmc
