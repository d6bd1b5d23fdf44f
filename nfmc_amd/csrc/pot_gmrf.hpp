// Latent Gaussian Markov random field (kind 13): its register class and its one-row NeuTra form.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

// Latent Gaussian Markov random field (NFMC_POT_LATENT_GMRF, nfmc_hip.h): n sites with the sparse structure matrix R in
// slot-major ELL form (W = p.n_components slots; p.a = W rows of n4 = 4 ceil(n / 4) values, then W rows of n4 column
// indices as integer-valued floats; a padding slot has value 0 and its own row as index), kind 12's likelihoods on the
// sites (latent_lik, table p.b = 8 header floats, then the rows m, y, w of n4 floats) and optionally s = log tau as
// coordinate n.  With v the vector of the mode, q = v^T R v, (a, b, rho/2, (n - rho)/2) = p.b[4 .. 7]:
//   fixed tau  (d = n, v = x - m):      U = 1/2 q + sum l_j(x_j),                               dU/dx = R v + l'(x)
//   centred    (d = n + 1, v = x - m):  U = 1/2 e^s q - (rho/2 + a) s + sum l_j(x_j) + b e^s,   dU/dx_j = e^s (R v)_j + l'_j,
//                                       dU/ds = 1/2 e^s q - rho/2 + b e^s - a
//   scaled     (d = n + 1, v = u, f = m + e^(-s/2) u):
//                                       U = 1/2 q + sum l_j(f_j) + b e^s - a s + (n - rho)/2 s,
//                                       dU/du_j = (R u)_j + e^(-s/2) l'_j(f_j),
//                                       dU/ds = -1/2 e^(-s/2) sum u_j l'_j(f_j) + b e^s - a + (n - rho)/2
// The access pattern is a gather: coordinate j needs v at the W columns of its row, anywhere in the chain.  The
// workgroup's block is IrtPot's: one wave-private row of DP + 4 floats per chain (irt_floats).  prepare() stores the
// lane's quads of v into the row (zeros on the padding; s itself at position n, which every lane then reads back: one
// address per chain, a broadcast), and forms (R v)_j of its own coordinates slot by slot: per register quad and slot ONE
// 16-byte load of values and ONE of indices from global memory (consecutive lanes consecutive 16 bytes, every chain the
// same ones: the block of at most 2 x 32 x 1024 floats stays in L2) and four ds_read_b32 gathers.  ds_bpermute cannot
// serve: it moves one register of one other lane, and the column a lane needs sits in a register whose index depends
// on the column.  Every gathered index is clamped into the sites 0 .. n - 1 (gmrf_row below clamps
// alike), so a bad table reads a wrong site of the chain's own row: never s, another chain's row or memory outside
// the block.  Row pitch DP + 4 as in IrtPot: the gathers of one
// chain spread over the banks like the columns of R do; chains of one 32-lane half that gather the same column (the
// same stencil offset) would meet in one bank at a pitch of DP >= 32 and sit 4 banks apart here.  The row is written
// and read by ONE wave: wavefront fences (Phi4Pot), no workgroup barrier.  1/2 v^T R v, the data term and sum u l' are
// lane-local sums; what crosses lanes goes through group_allreduce: U alone when tau is fixed, q and the data term
// when centred, U's site part and sum u l' when scaled.  No atomics: bitwise repeatable.  The likelihood is dispatched
// once per prepare() outside the loops (LatentGaussPot), the mode is a wave-uniform branch behind them.  Nothing is
// clamped: an overflowing e^s or e^f gives a non-finite U, which the samplers reject and count.
template <int CPL, int LPC, bool FAST>
struct GmrfPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    const float* ell;                    // this lane's quad 0 of slot 0: values; the indices wn4 floats behind
    const float* tab;                    // rows m, y, w of n4 floats (behind the 8 floats of the header)
    int nn, n4, nw, wn4;                 // n, 4 ceil(n / 4), W, W n4
    int lik;
    bool tau, scaled;
    bool lead;                           // this lane holds coordinate 0 in register 0
    float c0, c1, c2;                    // Student-t constants
    float pa, pb, hr, hn;                // Gamma(a, b) prior of tau, rho / 2, (n - rho) / 2
    struct Ctx {
        float u;                         // U of the chain (every lane of the group)
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        lik = 0;
        tau = scaled = false;
        gmrf_code(p.a_scalar, lik, tau, scaled);
        nn = tau ? d - 1 : d;
        n4 = latent_row(nn);
        nw = p.n_components;
        wn4 = nw * n4;
        ell = p.a + 4 * g;
        tab = p.b + 8;
        lead = (g == 0);
        c0 = p.b[0];
        c1 = p.b[1];
        c2 = p.b[2];
        pa = p.b[4];
        pb = p.b[5];
        hr = p.b[6];
        hn = p.b[7];
    }
    // register quad q of table row k (0 m, 1 y, 2 w) for this lane; zeros past the row
    __device__ __forceinline__ float4 tab4(int k, int q, int g) const {
        const int c = 4 * (q * LPC + g);
        return c < n4 ? *reinterpret_cast<const float4*>(tab + k * n4 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // value of the chain's row at the column a table entry names, clamped into the sites 0 .. n - 1
    __device__ __forceinline__ float gather(float col) const {
        const int j = (int)col;
        return row[j < 0 ? 0 : (j > nn - 1 ? nn - 1 : j)];
    }
    // l'(f) of this lane's coordinates into lp, their share of sum_j l_j(f_j) returned
    template <int LIK>
    __device__ __forceinline__ float likelihood(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 y = tab4(1, q, g), w = tab4(2, q, g);
            const float yy[4] = {y.x, y.y, y.z, y.w}, ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float l;
                latent_lik<LIK>(f[4 * q + k], yy[k], ww[k], c0, c1, c2, l, lp[4 * q + k]);
                s += l;
            }
        }
        return s;
    }
    __device__ __forceinline__ float likelihood_of(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        return lik == 0 ? likelihood<0>(f, lp, g) : lik == 1 ? likelihood<1>(f, lp, g) : likelihood<2>(f, lp, g);
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        float v[CPL], mv[CPL];           // r or u on the sites, 0 elsewhere / the prior mean
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 m = tab4(0, q, g);
            mv[4 * q] = m.x;
            mv[4 * q + 1] = m.y;
            mv[4 * q + 2] = m.z;
            mv[4 * q + 3] = m.w;
            float st[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = 4 * q + k, c = coord_of<CPL, LPC>(g, i);
                v[i] = c < nn ? (scaled ? x[i] : x[i] - mv[i]) : 0.f;
                st[k] = (tau && c == nn) ? x[i] : v[i];
            }
            *reinterpret_cast<float4*>(row + 4 * (q * LPC + g)) = make_float4(st[0], st[1], st[2], st[3]);
        }
        order();   // the wave's stores precede its reads
        const float s = tau ? row[nn] : 0.f;
        const float es = tau ? fast_exp(s) : 1.f, eh = scaled ? fast_exp(-0.5f * s) : 1.f;
        float rv[CPL];                   // (R v)_j of this lane's coordinates
#pragma unroll
        for (int i = 0; i < CPL; ++i) rv[i] = 0.f;
        const float* slot = ell;
        for (int k = 0; k < nw; ++k, slot += n4) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (4 * (q * LPC + g) < n4) {
                    const float4 a = *reinterpret_cast<const float4*>(slot + 4 * q * LPC);
                    const float4 j = *reinterpret_cast<const float4*>(slot + wn4 + 4 * q * LPC);
                    rv[4 * q] = fmaf(a.x, gather(j.x), rv[4 * q]);
                    rv[4 * q + 1] = fmaf(a.y, gather(j.y), rv[4 * q + 1]);
                    rv[4 * q + 2] = fmaf(a.z, gather(j.z), rv[4 * q + 2]);
                    rv[4 * q + 3] = fmaf(a.w, gather(j.w), rv[4 * q + 3]);
                }
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        float f[CPL], lp[CPL];
#pragma unroll
        for (int i = 0; i < CPL; ++i) f[i] = scaled ? fmaf(eh, v[i], mv[i]) : x[i];
        const float ls = likelihood_of(f, lp, g);
        float qf = 0.f;                  // this lane's share of v^T R v
#pragma unroll
        for (int i = 0; i < CPL; ++i) qf = fmaf(v[i], rv[i], qf);
        Ctx cx;
        float gs = 0.f;                  // dU/ds
        if (!tau) {
            cx.u = group_allreduce<LPC>(fmaf(0.5f, qf, ls));
#pragma unroll
            for (int i = 0; i < CPL; ++i) cx.gr[i] = rv[i] + lp[i];
        } else if (!scaled) {
            const float qq = group_allreduce<LPC>(qf), lt = group_allreduce<LPC>(ls);
            const float hq = 0.5f * es * qq, be = pb * es;
            cx.u = (hq + lt) + (be - (hr + pa) * s);
            gs = (hq - hr) + (be - pa);
#pragma unroll
            for (int i = 0; i < CPL; ++i) cx.gr[i] = fmaf(es, rv[i], lp[i]);
        } else {
            float ul = 0.f;              // this lane's share of sum u l'
#pragma unroll
            for (int i = 0; i < CPL; ++i) ul = fmaf(v[i], lp[i], ul);
            const float us = group_allreduce<LPC>(fmaf(0.5f, qf, ls)), ut = group_allreduce<LPC>(ul);
            const float be = pb * es;
            cx.u = us + (be + (hn - pa) * s);
            gs = fmaf(-0.5f * eh, ut, be) + (hn - pa);
#pragma unroll
            for (int i = 0; i < CPL; ++i) cx.gr[i] = fmaf(eh, lp[i], rv[i]);
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            cx.gr[i] = c < nn ? cx.gr[i] : ((tau && c == nn) ? gs : 0.f);
        }
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Latent Gaussian Markov random field (NFMC_POT_LATENT_GMRF) for the row of one chain, as potential_value_grad_row: U and
// dU/dx of GmrfPot (above), the sites first and s = log tau behind them when tau is unknown.  The row is
// addressable here, so the gather is direct: (R v)_j = sum_k val[k][j] v[idx[k][j]] with v = row - m (fixed tau,
// centred) or row (scaled), the ELL block and the table wave-uniform (scalar loads), every index clamped into the
// sites 0 .. n - 1.  One pass over the sites: O(W n), the three sums of GmrfPot run in registers, the s entry follows
// the pass.  The likelihood is chosen outside the loop.  Kept out of potential_value_grad_row, which the fit and DLMC
// kernels share and which never see kind 13.
template <int LIK>
__device__ __forceinline__ float gmrf_row(const float* __restrict__ row, float* __restrict__ grow, const NfmcPotential& p, int d,
                                          bool tau, bool scaled) {
    const int n = tau ? d - 1 : d, n4 = latent_row(n), nw = p.n_components;
    const float c0 = p.b[0], c1 = p.b[1], c2 = p.b[2], pa = p.b[4], pb = p.b[5], hr = p.b[6], hn = p.b[7];
    const float* __restrict__ m = p.b + 8;
    const float* __restrict__ y = m + n4;
    const float* __restrict__ w = y + n4;
    const float* __restrict__ val = p.a;
    const float* __restrict__ idx = p.a + (int64_t)nw * n4;
    const float s = tau ? row[n] : 0.f;
    const float es = tau ? fast_exp(s) : 1.f, eh = scaled ? fast_exp(-0.5f * s) : 1.f;
    float us = 0.f, qq = 0.f, ls = 0.f, ut = 0.f;   // sum 1/2 v Rv + l | v^T R v | sum l | sum u l'
    for (int j = 0; j < n; ++j) {
        float t = 0.f;
        for (int k = 0; k < nw; ++k) {
            int i = (int)idx[k * n4 + j];
            i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
            t = fmaf(val[k * n4 + j], scaled ? row[i] : row[i] - m[i], t);
        }
        const float xj = row[j], v = scaled ? xj : xj - m[j];
        float l, lp;
        latent_lik<LIK>(scaled ? fmaf(eh, v, m[j]) : xj, y[j], w[j], c0, c1, c2, l, lp);
        qq = fmaf(v, t, qq);
        ls += l;
        us += fmaf(0.5f * v, t, l);
        ut = fmaf(v, lp, ut);
        grow[j] = !tau ? t + lp : (scaled ? fmaf(eh, lp, t) : fmaf(es, t, lp));
    }
    if (!tau) return us;
    const float be = pb * es;
    if (!scaled) {
        const float hq = 0.5f * es * qq;
        grow[n] = (hq - hr) + (be - pa);
        return (hq + ls) + (be - (hr + pa) * s);
    }
    grow[n] = fmaf(-0.5f * eh, ut, be) + (hn - pa);
    return us + (be + (hn - pa) * s);
}
__device__ __forceinline__ float gmrf_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                     const NfmcPotential& p, int d) {
    int lik = 0;
    bool tau = false, scaled = false;
    gmrf_code(p.a_scalar, lik, tau, scaled);
    return lik == 0 ? gmrf_row<0>(row, grow, p, d, tau, scaled)
         : lik == 1 ? gmrf_row<1>(row, grow, p, d, tau, scaled)
                    : gmrf_row<2>(row, grow, p, d, tau, scaled);
}

}  // namespace nfmc
