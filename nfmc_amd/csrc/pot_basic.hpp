// Kinds 0 to 3 (quadratic, funnel, Gaussian mixture, logistic regression): the units of the general kernels run them together.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

// ------------------------------------------------------------------------------------------------
// Potentials.  `term` is the coordinate's share of U (U = group sum of terms), `grad` dU/dx_c.
// Coordinates beyond d carry a = 0 / x = 0 so they contribute exactly zero.
template <int CPL, int LPC, bool FAST>
struct QuadraticPot {
    // U = sum a_c (x_c - b_c)^2
    static constexpr bool kQuadratic = true;
    static constexpr bool kStaged = false;   // parameters in registers (no LDS block, see MixturePot)
    float a_s, b_s;
    float a[FAST ? 1 : CPL], b[FAST ? 1 : CPL];
    struct Ctx {};

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        a_s = p.a_scalar;
        b_s = p.b_scalar;
        if constexpr (!FAST) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = coord_of<CPL, LPC>(g, i);
                const bool ok = c < d;
                a[i] = ok ? (p.a ? p.a[c] : p.a_scalar) : 0.f;
                b[i] = ok ? (p.b ? p.b[c] : p.b_scalar) : 0.f;
            }
        }
    }
    __device__ __forceinline__ Ctx prepare(const float (&)[CPL], int, int) const { return Ctx{}; }
    __device__ __forceinline__ float aa(int i) const { return FAST ? a_s : a[FAST ? 0 : i]; }
    __device__ __forceinline__ float bb(int i) const { return FAST ? b_s : b[FAST ? 0 : i]; }
    __device__ __forceinline__ float grad(const Ctx&, int i, float x) const { return 2.f * aa(i) * (x - bb(i)); }
    __device__ __forceinline__ float term(const Ctx&, int i, float x) const {
        const float t = x - bb(i);
        return aa(i) * t * t;
    }
};

template <int CPL, int LPC, bool FAST>
struct FunnelPot {
    // U = x0^2/(2 s^2) + sum_{i>=1} [ x_i^2 e^{-x0} / 2 + x0 / 2 ]
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    float inv_s2, half_dm1;
    bool lead;          // this lane holds coordinate 0 in register 0
    float valid[CPL];   // 1 for real coordinates, 0 for padding
    struct Ctx {
        float x0, e, s;  // x_0, exp(-x_0), sum_{i>=1} x_i^2
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        inv_s2 = 1.f / (p.a_scalar * p.a_scalar);
        half_dm1 = 0.5f * (float)(d - 1);
        lead = (g == 0);
#pragma unroll
        for (int i = 0; i < CPL; ++i) valid[i] = coord_of<CPL, LPC>(g, i) < d ? 1.f : 0.f;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        Ctx c;
        c.x0 = group_broadcast0<LPC>(x[0]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) s = fmaf(x[i], (lead && i == 0) ? 0.f : x[i], s);
        c.s = group_allreduce<LPC>(s);
        c.e = fast_exp(-c.x0);
        return c;
    }
    __device__ __forceinline__ float grad(const Ctx& c, int i, float x) const {
        const float g0 = c.x0 * inv_s2 - 0.5f * c.e * c.s + half_dm1;
        return (lead && i == 0) ? g0 : x * c.e * valid[i];
    }
    __device__ __forceinline__ float term(const Ctx& c, int i, float x) const {
        const float t0 = 0.5f * c.x0 * c.x0 * inv_s2 + half_dm1 * c.x0;
        return (lead && i == 0) ? t0 : 0.5f * c.e * x * x;
    }
};

// Diagonal Gaussian mixture (NFMC_POT_GAUSSIAN_MIXTURE, K = p.n_components <= kMixMaxK):
//   U = -logsumexp_k [ c_k - 1/2 sum_j lam_kj (x_j - mu_kj)^2 ]
//   dU/dx_j = sum_k r_k lam_kj (x_j - mu_kj),   r_k = softmax_k(e_k)
// Every chain group of a workgroup reads the same (lam, mu) rows, so they are staged ONCE per workgroup in LDS
// (stage(), before init()), padded to the layout's DP coordinates with lam = mu = 0 -- padding lanes then add exactly
// zero to every sum and get a zero gradient.  A lane reads its register quad q of row k as one ds_read_b128 at
// coordinate 4 (q LPC + g): consecutive lanes read consecutive 16 bytes, the chain groups of a wave the same ones
// (broadcast).  The c_k are wave-uniform and stay in registers.  prepare() does K group reductions (one butterfly
// each), the logsumexp on the fast exp2 / log2 helpers, and the gradient of the lane's coordinates in a second pass
// over the rows; term() puts the whole U on coordinate 0 of lane 0 (the FunnelPot trick).
template <int CPL, int LPC, bool FAST>
struct MixturePot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    const float* tab;     // LDS: lam (K, DP) | mu (K, DP)
    float c[kMixMaxK];    // log w_k + 1/2 sum_j log lam_kj
    int nk;
    bool lead;            // this lane holds coordinate 0 in register 0
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    // all threads of the workgroup; the caller synchronises before the first prepare()
    __device__ __forceinline__ static void stage(float* __restrict__ lds, const NfmcPotential& p, int d) {
        const int kd = p.n_components * DP;
        for (int t = threadIdx.x; t < 2 * kd; t += kBlock) {
            const int half = t >= kd, r = half ? t - kd : t;
            const int k = r / DP, j = r - k * DP;
            lds[t] = j < d ? (half ? p.b : p.a)[(int64_t)k * d + j] : 0.f;
        }
    }
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, const float* lds) {
        tab = lds;
        nk = p.n_components;
        lead = (g == 0);
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) c[k] = k < nk ? p.a[(int64_t)nk * d + k] : 0.f;
    }
    __device__ __forceinline__ float4 row4(int k, int half, int q, int g) const {
        return *reinterpret_cast<const float4*>(tab + (half * nk + k) * DP + 4 * (q * LPC + g));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        float e[kMixMaxK];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) {
            e[k] = -INFINITY;
            if (k < nk) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < CPL / 4; ++q) {
                    const float4 l = row4(k, 0, q, g), mu = row4(k, 1, q, g);
                    const float t0 = x[4 * q] - mu.x, t1 = x[4 * q + 1] - mu.y, t2 = x[4 * q + 2] - mu.z,
                                t3 = x[4 * q + 3] - mu.w;
                    s = fmaf(l.x * t0, t0, s);
                    s = fmaf(l.y * t1, t1, s);
                    s = fmaf(l.z * t2, t2, s);
                    s = fmaf(l.w * t3, t3, s);
                }
                e[k] = fmaf(-0.5f, group_allreduce<LPC>(s), c[k]);
                m = fmaxf(m, e[k]);
            }
        }
        float w[kMixMaxK], sum = 0.f;
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) {
            w[k] = k < nk ? fast_exp(e[k] - m) : 0.f;   // e_k - m <= 0: no overflow; NaN propagates through sum
            sum += w[k];
        }
        Ctx cx;
        cx.u = -(m + fast_ln(sum));
        const float inv = 1.f / sum;
#pragma unroll
        for (int i = 0; i < CPL; ++i) cx.gr[i] = 0.f;
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) {
            if (k < nk) {
                const float r = w[k] * inv;
#pragma unroll
                for (int q = 0; q < CPL / 4; ++q) {
                    const float4 l = row4(k, 0, q, g), mu = row4(k, 1, q, g);
                    cx.gr[4 * q] = fmaf(r * l.x, x[4 * q] - mu.x, cx.gr[4 * q]);
                    cx.gr[4 * q + 1] = fmaf(r * l.y, x[4 * q + 1] - mu.y, cx.gr[4 * q + 1]);
                    cx.gr[4 * q + 2] = fmaf(r * l.z, x[4 * q + 2] - mu.z, cx.gr[4 * q + 2]);
                    cx.gr[4 * q + 3] = fmaf(r * l.w, x[4 * q + 3] - mu.w, cx.gr[4 * q + 3]);
                }
            }
        }
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

template <int CPL, int LPC, bool FAST>
struct LogRegPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int T = kLogRegTileFloats / DP;   // rows per tile
    static_assert(T % 4 == 0, "batches of 4 rows");
    float* tile;          // LDS: X rows (T, DP) | y (T)
    const float* X;
    const float* y;
    int nr, dd;
    float inv_s2;
    bool lead;            // this lane holds coordinate 0 in register 0
    float valid[CPL];     // 1 for real coordinates, 0 for padding
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        X = p.a;
        y = p.b;
        nr = p.n_components;
        dd = d;
        inv_s2 = p.a_scalar;
        lead = (g == 0);
#pragma unroll
        for (int i = 0; i < CPL; ++i) valid[i] = coord_of<CPL, LPC>(g, i) < d ? 1.f : 0.f;
    }
    __device__ __forceinline__ float4 row4(int r, int q, int g) const {
        return *reinterpret_cast<const float4*>(tile + r * DP + 4 * (q * LPC + g));
    }
    // all threads of the workgroup: rows t0 .. t0 + rows - 1 into the tile, zeros past them
    __device__ __forceinline__ void load_tile(int t0, int rows) const {
        load_tile_rows<DP>(tile, X, dd, t0, rows);
        for (int r = threadIdx.x; r < T; r += kBlock) tile[T * DP + r] = r < rows ? y[t0 + r] : 0.f;
        __syncthreads();
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        Ctx cx;
        float pr = 0.f;   // this lane's share of |x|^2
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const float xv = valid[i] * x[i];
            cx.gr[i] = inv_s2 * xv;
            pr = fmaf(xv, xv, pr);
        }
        // this lane's share of the data term, summed in fp64: U is a sum of N terms of O(1), and fp32 partial sums over
        // thousands of rows lose ~sqrt(N) ulps of U -- 1e-2 in a log ratio at N = 2500 -- which fp64 keeps to the one
        // rounding of the result
        double ul = 0.0;
        const float* yt = tile + T * DP;
        for (int t0 = 0; t0 < nr; t0 += T) {
            const int rows = nr - t0 < T ? nr - t0 : T;
            load_tile(t0, rows);
            for (int r0 = 0; r0 < rows; r0 += 4) {
                float h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float4 w = row4(r0 + b, q, g);
                        s = fmaf(w.x, x[4 * q], s);
                        s = fmaf(w.y, x[4 * q + 1], s);
                        s = fmaf(w.z, x[4 * q + 2], s);
                        s = fmaf(w.w, x[4 * q + 3], s);
                    }
                    h[b] = s;
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
                        const float4 w = row4(r0 + b, q, g);
                        cx.gr[4 * q] = fmaf(rb[b], w.x, cx.gr[4 * q]);
                        cx.gr[4 * q + 1] = fmaf(rb[b], w.y, cx.gr[4 * q + 1]);
                        cx.gr[4 * q + 2] = fmaf(rb[b], w.z, cx.gr[4 * q + 2]);
                        cx.gr[4 * q + 3] = fmaf(rb[b], w.w, cx.gr[4 * q + 3]);
                    }
                }
            }
        }
        cx.u = group_allreduce<LPC>((float)(ul + (double)(0.5f * inv_s2 * pr)));
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

}  // namespace nfmc
