// Sparse logistic regression (kind 7): its register class and its one-row NeuTra form.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

// Sparse logistic regression (NFMC_POT_SPARSE_LOGISTIC_REGRESSION; X (N, D) row-major in a, y (N,) in {0, 1} in b,
// N = p.n_components, a = a_scalar, b = b_scalar, D = (d - 1) / 2).  Coordinates x_{2j} = w_j, x_{2j+1} = l_j =
// log lambda_j, x_{2D} = s = log tau; with beta_j = e^{s + l_j} w_j, z = X beta, r_i = sigmoid(z_i) - y_i, g = X^T r:
//   U = sum_i [softplus(z_i) - y_i z_i] + 1/2 sum_j w_j^2 + sum_j (b e^{l_j} - a l_j) + (b e^s - a s)
//   dU/dw_j = e^{s + l_j} g_j + w_j,   dU/dl_j = beta_j g_j + b e^{l_j} - a,   dU/ds = sum_j beta_j g_j + b e^s - a
// Register quad q of lane g holds coordinates 4 (q LPC + g) .. + 3 (coord_of), i.e. the pairs (w_j, l_j) of the two
// columns j = 2 (q LPC + g) and j + 1: every pair is lane-local, and only s crosses lanes.  prepare() (1) broadcasts s
// from the lane that holds coordinate 2D with one group_allreduce of a masked value, (2) forms beta of the lane's columns
// in registers, (3) streams X through a COMPACT LDS tile -- slr_tile_rows(DP) rows of DP / 2 columns, zero past D and past
// the last row, their labels behind them -- in LogRegPot's batches of 4 rows: per row and register quad one ds_read_b64
// of the quad's two columns feeds two FMAs of the dot product and, after the batch's reduce-scatter (LPC >= 4; one
// butterfly per row below) and the residual broadcast, two FMAs of g; (4) applies the chain rule pair by pair, and (5)
// all-reduces sum_j beta_j g_j (one butterfly) for the gradient of s.  The data term is summed in fp64 per lane as in
// LogRegPot, and term() puts the lane's share of U on its register 0.  LogRegPot's tile rule holds: every thread of the
// workgroup calls prepare() equally often.  e^{s + l_j}, e^{l_j}, e^s or z overflow fp32 far in the tails; such a
// state's U is inf or NaN, so the samplers reject it and count its log ratio as non-finite.
template <int CPL, int LPC, bool FAST>
struct SparseLogRegPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int DH = DP / 2;                  // tile columns: two per register quad
    static constexpr int T = kLogRegTileFloats / DH;   // rows per tile (slr_tile_rows)
    static constexpr int NP = CPL / 2;                 // column pairs (w_j, l_j) per lane
    static_assert(T % 4 == 0, "batches of 4 rows");
    float* tile;          // LDS: X rows (T, DH) | y (T)
    const float* X;
    const float* y;
    int nr, nd;           // N, D
    float ca, cb;         // a, b
    int sreg;             // the register of this lane that holds s (coordinate 2D), -1 if none
    uint32_t pm;          // bit p: pair p (registers 2p, 2p + 1) is a column j < D
    struct Ctx {
        float u;          // this lane's share of U
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        X = p.a;
        y = p.b;
        nr = p.n_components;
        nd = (d - 1) >> 1;
        ca = p.a_scalar;
        cb = p.b_scalar;
        sreg = -1;
        pm = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            if (c == d - 1) sreg = i;
            if ((i & 1) == 0 && c < d - 1) pm |= 1u << (i >> 1);
        }
    }
    // columns 2 (q LPC + g) and + 1 of tile row r
    __device__ __forceinline__ float2 row2(int r, int q, int g) const {
        return *reinterpret_cast<const float2*>(tile + r * DH + 2 * (q * LPC + g));
    }
    // all threads of the workgroup: rows t0 .. t0 + rows - 1 into the tile, zeros past them
    __device__ __forceinline__ void load_tile(int t0, int rows) const {
        load_tile_rows<DH>(tile, X, nd, t0, rows);
        for (int r = threadIdx.x; r < T; r += kBlock) tile[T * DH + r] = r < rows ? y[t0 + r] : 0.f;
        __syncthreads();
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        float sv = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) sv = i == sreg ? x[i] : sv;
        const float s = group_allreduce<LPC>(sv);   // s = log tau: the one value that crosses lanes
        float es[NP], bt[NP], gg[NP];                // e^{s + l_j}, beta_j, g_j of the lane's columns (0 past D)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const bool ok = (pm >> p) & 1u;
            es[p] = ok ? fast_exp(s + x[2 * p + 1]) : 0.f;
            bt[p] = ok ? es[p] * x[2 * p] : 0.f;
            gg[p] = 0.f;
        }
        double ul = 0.0;   // this lane's share of the data term, in fp64 (LogRegPot)
        const float* yt = tile + T * DH;
        for (int t0 = 0; t0 < nr; t0 += T) {
            const int rows = nr - t0 < T ? nr - t0 : T;
            load_tile(t0, rows);
            for (int r0 = 0; r0 < rows; r0 += 4) {
                float h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float sz = 0.f;
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float2 v = row2(r0 + b, q, g);
                        sz = fmaf(v.x, bt[2 * q], sz);
                        sz = fmaf(v.y, bt[2 * q + 1], sz);
                    }
                    h[b] = sz;
                }
                float rb[4];   // sigmoid(z) - y of the batch's rows (0 past the last row)
                if constexpr (LPC >= 4) {
                    const int b = g & 3;
                    const float z = group_reduce_scatter<4, LPC>(h);   // z of row r0 + b
                    const float yv = yt[r0 + b];
                    float sp, sg;
                    softplus_sigmoid(z, sp, sg);
                    const bool ok = r0 + b < rows;
                    if (ok && g < 4) ul += (double)(sp - yv * z);   // one lane per row
                    const float res = ok ? sg - yv : 0.f;
                    rb[0] = dpp_mov<0x00>(res);   // quad_perm [b, b, b, b]: the value of lane b of the quad
                    rb[1] = dpp_mov<0x55>(res);
                    rb[2] = dpp_mov<0xAA>(res);
                    rb[3] = dpp_mov<0xFF>(res);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float z = group_allreduce<LPC>(h[b]);
                        const float yv = yt[r0 + b];
                        float sp, sg;
                        softplus_sigmoid(z, sp, sg);
                        const bool ok = r0 + b < rows;
                        if (ok && g == 0) ul += (double)(sp - yv * z);
                        rb[b] = ok ? sg - yv : 0.f;
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float2 v = row2(r0 + b, q, g);
                        gg[2 * q] = fmaf(rb[b], v.x, gg[2 * q]);
                        gg[2 * q + 1] = fmaf(rb[b], v.y, gg[2 * q + 1]);
                    }
                }
            }
        }
        Ctx cx;
        float u = 0.f, sbg = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float w = x[2 * p], l = x[2 * p + 1];
            cx.gr[2 * p] = 0.f;
            cx.gr[2 * p + 1] = 0.f;
            if ((pm >> p) & 1u) {
                const float el = fast_exp(l), bg = bt[p] * gg[p];
                cx.gr[2 * p] = fmaf(es[p], gg[p], w);
                cx.gr[2 * p + 1] = bg + fmaf(cb, el, -ca);
                sbg += bg;
                u += fmaf(0.5f * w, w, fmaf(cb, el, -ca * l));
            }
        }
        sbg = group_allreduce<LPC>(sbg);   // sum_j beta_j g_j
        if (sreg >= 0) {
            const float e = fast_exp(s);
#pragma unroll
            for (int i = 0; i < CPL; ++i)
                if (i == sreg) cx.gr[i] = sbg + fmaf(cb, e, -ca);
            u += fmaf(cb, e, -ca * s);
        }
        cx.u = (float)(ul + (double)u);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Sparse logistic regression (NFMC_POT_SPARSE_LOGISTIC_REGRESSION) for the row of one chain, as potential_value_grad_row:
// U and dU/dx of SparseLogRegPot (above), x_{2j} = w_j, x_{2j+1} = log lambda_j, x_{2D} = log tau.  The gradient
// row is the workspace: beta_j goes to grow[2j] and g_j accumulates in grow[2j + 1] over one pass through the rows of X
// (z_i, then its residual into g), and the chain rule then overwrites both, pair by pair.  X and y are wave-uniform
// (scalar loads); the data term is summed in fp64, as in SparseLogRegPot.  Kept out of potential_value_grad_row, which
// the fit and DLMC kernels share and which never see kind 7.
__device__ __forceinline__ float slr_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                    const NfmcPotential& p, int d) {
    const float* __restrict__ X = p.a;
    const float* __restrict__ y = p.b;
    const int nd = (d - 1) >> 1, nr = p.n_components;
    const float ca = p.a_scalar, cb = p.b_scalar, s = row[2 * nd];
    for (int j = 0; j < nd; ++j) {
        grow[2 * j] = fast_exp(s + row[2 * j + 1]) * row[2 * j];   // beta_j
        grow[2 * j + 1] = 0.f;                                     // g_j
    }
    double ul = 0.0;
    for (int i = 0; i < nr; ++i) {
        const float* __restrict__ xi = X + (int64_t)i * nd;
        float z = 0.f;
        for (int j = 0; j < nd; ++j) z = fmaf(xi[j], grow[2 * j], z);
        float sp, sg;
        softplus_sigmoid(z, sp, sg);
        const float yv = y[i];
        ul += (double)(sp - yv * z);
        const float r = sg - yv;
        for (int j = 0; j < nd; ++j) grow[2 * j + 1] = fmaf(r, xi[j], grow[2 * j + 1]);
    }
    float u = 0.f, sbg = 0.f;
    for (int j = 0; j < nd; ++j) {
        const float w = row[2 * j], l = row[2 * j + 1], bt = grow[2 * j], gj = grow[2 * j + 1];
        const float el = fast_exp(l), bg = bt * gj;
        grow[2 * j] = fmaf(fast_exp(s + l), gj, w);
        grow[2 * j + 1] = bg + fmaf(cb, el, -ca);
        sbg += bg;
        u += fmaf(0.5f * w, w, fmaf(cb, el, -ca * l));
    }
    const float es = fast_exp(s);
    grow[2 * nd] = sbg + fmaf(cb, es, -ca);
    return (float)(ul + (double)(u + fmaf(cb, es, -ca * s)));
}

}  // namespace nfmc
