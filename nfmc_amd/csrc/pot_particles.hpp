// Interacting particles (kind 11): its register class and its one-row NeuTra form.
#pragma once

#include "pot_kinds.hpp"

namespace nfmc {

// One pair of particles at squared distance s: e = beta phi(r) and w = beta phi'(r) / r, the factor of (r_i - r_j) in
// the force.  Lennard-Jones (p0 = beta eps, p1 = r_m^2) from s alone, t = r_m^2 / s:  e = p0 t^3 (t^3 - 2),
// w = -12 p0 t^3 (t^3 - 1) / s; at s = 0 e = inf and w (r_i - r_j) = NaN: the samplers reject the state.  Double well
// (p0 .. p2 = beta (a, b, c), p3 = r0) with u = sqrt(s) - r0:  e = u (p0 + u (p1 + p2 u^2)), w = (p0 + u (2 p1 + 4 p2
// u^2)) / sqrt(s), and w = 0 at s = 0.  Shared by ParticlePot and particles_value_grad_row (below).
template <bool LJ>
__device__ __forceinline__ void particle_pair(float s, float p0, float p1, float p2, float p3, float& e, float& w) {
    if constexpr (LJ) {
        const float is = __builtin_amdgcn_rcpf(s), t = p1 * is, t3 = t * t * t;
        const float pt = p0 * t3;
        e = pt * (t3 - 2.f);
        w = -12.f * pt * (t3 - 1.f) * is;
    } else {
        const float u = __builtin_amdgcn_sqrtf(s) - p3, u2 = u * u;
        e = u * fmaf(u, fmaf(p2, u2, p1), p0);
        w = s > 0.f ? fmaf(u, fmaf(4.f * p2, u2, 2.f * p1), p0) * __builtin_amdgcn_rsqf(s) : 0.f;
    }
}

// Interacting particles (NFMC_POT_PARTICLES; P = p.n_components particles in D = d / P dimensions, particle-major
// x = [r_0 | .. | r_{P-1}]; p.a = (pair code 0 Lennard-Jones / 1 double well, D, beta k, four pair parameters, 0)):
//   U = 1/2 beta k sum_i |r_i|^2 + sum_{i<j} beta phi(r_ij),   dU/dr_i = beta k r_i + sum_{j != i} w(r_ij) (r_i - r_j)
// (particle_pair).  Every coordinate meets every other, and a particle's D coordinates straddle register quads and
// lanes, so the chain's state goes through a wave-private LDS row as in IrtPot (one row of DP + 4 floats per chain,
// particles_floats; the pitch for IrtPot's bank reason: the reads below are the same broadcasts).  prepare() stores the
// lane's quads into the row (ds_write_b128).  Particle p belongs to lane p % LPC of its chain: lane g owns particles g,
// g + LPC, .., at most NP = ceil(CPL / D) of them (P D <= CPL LPC), keeps their positions and forces in registers and
// loops j = 0 .. P-1 -- a uniform trip count; r_j is read from the row at an address all lanes of the chain share, a
// broadcast -- adding w (r_p - r_j) to the force of each owned p and 1/2 beta phi to its share of U.  An unordered pair
// is evaluated twice, once per owner: no atomics and a fixed summation order, so runs are bitwise repeatable.  j = p
// and owned slots p >= P are taken out by a select on w and e, not by a branch; slot m is skipped when no lane of the
// wave owns a particle in it (m LPC >= P, uniform).  D and the pair form are wave-uniform and chosen ONCE, outside the
// loops (pairs<D, LJ>): NP and the register arrays have compile-time bounds.  After the loop the owners write their
// forces over their particles' slots in the row -- every read of a position is behind them: one wave, LDS operations
// complete in order, a fence between -- and each lane reads back the quads it holds as the pair part of dU/dx and adds
// the trap term from its own registers.  Padding coordinates (c >= d) get a zero gradient and add zero to U.  No
// workgroup barrier (LogRegPot's rule); wavefront fences as in Phi4Pot.  term() puts the lane's share of U on register 0.
template <int CPL, int LPC, bool FAST>
struct ParticlePot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    int np, nd, dd;                      // P, D, d
    bool lj;
    float bk, p0, p1, p2, p3;            // beta k and the pair parameters
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int, int d, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        np = p.n_components;
        dd = d;
        nd = d / np;
        lj = p.a[0] == 0.f;
        bk = p.a[2];
        p0 = p.a[3];
        p1 = p.a[4];
        p2 = p.a[5];
        p3 = p.a[6];
    }
    template <int D, bool LJ>
    __device__ __forceinline__ Ctx pairs(const float (&x)[CPL], int g) const {
        constexpr int NP = (CPL + D - 1) / D;   // owned particles per lane, at most
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int k = 0; k < Q; ++k)
            *reinterpret_cast<float4*>(row + 4 * (k * LPC + g)) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        order();   // the wave's stores precede its reads
        float rp[NP][D], f[NP][D], e = 0.f;
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            const int own = min(m * LPC + g, np - 1);   // a slot past P reads particle P - 1 and is selected away
#pragma unroll
            for (int c = 0; c < D; ++c) {
                rp[m][c] = row[own * D + c];
                f[m][c] = 0.f;
            }
        }
#pragma unroll 1
        for (int j = 0; j < np; ++j) {
            float rj[D];
#pragma unroll
            for (int c = 0; c < D; ++c) rj[c] = row[j * D + c];
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                if (m * LPC < np) {   // uniform
                    float dx[D], s = 0.f;
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        dx[c] = rp[m][c] - rj[c];
                        s = fmaf(dx[c], dx[c], s);
                    }
                    float ep, w;
                    particle_pair<LJ>(s, p0, p1, p2, p3, ep, w);
                    const int own = m * LPC + g;
                    const bool on = own != j && own < np;
                    e += on ? ep : 0.f;
                    w = on ? w : 0.f;
#pragma unroll
                    for (int c = 0; c < D; ++c) f[m][c] = fmaf(w, dx[c], f[m][c]);
                }
            }
        }
        order();   // every read of a position precedes the owners' stores
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            const int own = m * LPC + g;
            if (own < np) {
#pragma unroll
                for (int c = 0; c < D; ++c) row[own * D + c] = f[m][c];
            }
        }
        order();   // the owners' stores precede the reads below
        Ctx cx;
        float u = 0.5f * e;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const float4 t4 = *reinterpret_cast<const float4*>(row + 4 * (k * LPC + g));
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * k + j;
                const bool in = 4 * (k * LPC + g) + j < dd;
                const float xv = x[i], kx = bk * xv;
                cx.gr[i] = in ? kx + t[j] : 0.f;
                u += in ? 0.5f * kx * xv : 0.f;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        if (lj) return nd == 3 ? pairs<3, true>(x, g) : (nd == 2 ? pairs<2, true>(x, g) : pairs<1, true>(x, g));
        return nd == 3 ? pairs<3, false>(x, g) : (nd == 2 ? pairs<2, false>(x, g) : pairs<1, false>(x, g));
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Interacting particles (NFMC_POT_PARTICLES) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// ParticlePot (above), P = n_components particles of D = d / P coordinates each, particle-major.  A double loop:
// the position and the force of particle i stay in registers over j (three components; those past D are zero and add
// nothing to s), r_j is read from the lane's own LDS row, the pair j = i is taken out by a select, every unordered
// pair is evaluated twice and 1/2 phi added each time.  D, the pair form and the parameters are wave-uniform; the pair
// form is chosen outside the j loop.  Kept out of potential_value_grad_row, which the fit and DLMC kernels share and
// which never see kind 11.
template <bool LJ>
__device__ __forceinline__ float particles_force_row(const float* __restrict__ row, int np, int D, int i, float a0, float a1,
                                                     float a2, float p0, float p1, float p2, float p3, float& f0, float& f1,
                                                     float& f2) {
    float e = 0.f;
    f0 = f1 = f2 = 0.f;
    for (int j = 0; j < np; ++j) {
        const float* __restrict__ rj = row + j * D;
        const float d0 = a0 - rj[0], d1 = D > 1 ? a1 - rj[1] : 0.f, d2 = D > 2 ? a2 - rj[2] : 0.f;
        const float s = fmaf(d2, d2, fmaf(d1, d1, d0 * d0));
        float ep, w;
        particle_pair<LJ>(s, p0, p1, p2, p3, ep, w);
        e += j != i ? ep : 0.f;
        w = j != i ? w : 0.f;
        f0 = fmaf(w, d0, f0);
        f1 = fmaf(w, d1, f1);
        f2 = fmaf(w, d2, f2);
    }
    return e;
}
__device__ __forceinline__ float particles_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                          const NfmcPotential& p, int d) {
    const int np = p.n_components, D = d / np;
    const bool lj = p.a[0] == 0.f;
    const float bk = p.a[2], p0 = p.a[3], p1 = p.a[4], p2 = p.a[5], p3 = p.a[6];
    float u = 0.f, e = 0.f;
    for (int i = 0; i < np; ++i) {
        const float* __restrict__ ri = row + i * D;
        const float a0 = ri[0], a1 = D > 1 ? ri[1] : 0.f, a2 = D > 2 ? ri[2] : 0.f;
        float f0, f1, f2;
        e += lj ? particles_force_row<true>(row, np, D, i, a0, a1, a2, p0, p1, p2, p3, f0, f1, f2)
                : particles_force_row<false>(row, np, D, i, a0, a1, a2, p0, p1, p2, p3, f0, f1, f2);
        float* __restrict__ gi = grow + i * D;
        gi[0] = fmaf(bk, a0, f0);
        if (D > 1) gi[1] = fmaf(bk, a1, f1);
        if (D > 2) gi[2] = fmaf(bk, a2, f2);
        u = fmaf(0.5f * bk, fmaf(a2, a2, fmaf(a1, a1, a0 * a0)), u);
    }
    return fmaf(0.5f, e, u);
}

}  // namespace nfmc
