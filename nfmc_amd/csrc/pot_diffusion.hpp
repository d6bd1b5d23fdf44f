// Diffusion bridge (kind 14): its register class and its one-row NeuTra form.
#pragma once

#include "pot_kinds.hpp"

namespace nfmc {

// Drifts of the diffusion bridge (NFMC_POT_DIFFUSION_BRIDGE), DR the drift code, M the state's dimension, (p0 .. p3) the
// drift parameters of the header: f(x) into f, and J_f(x)^T e into v.  Fixed operation order: DiffusionPot and
// diffusion_row (below) share them.
//   0 cubic (any M)       f_c = x_c (p0 - p1 x_c^2),                              J = diag(p0 - 3 p1 x_c^2)
//   1 fitzhugh_nagumo (2) f = (x0 - x0^3/3 - x1 + p3, p2 (x0 + p0 - p1 x1)),      J = [[1 - x0^2, -1], [p2, -p2 p1]]
//   2 lorenz63 (3)        f = (p0 (x1 - x0), x0 (p1 - x2) - x1, x0 x1 - p2 x2),   J = [[-p0, p0, 0], [p1 - x2, -1, -x0], [x1, x0, -p2]]
template <int DR, int M>
__device__ __forceinline__ void diffusion_drift(const float (&x)[M], float p0, float p1, float p2, float p3, float (&f)[M]) {
    if constexpr (DR == 0) {
#pragma unroll
        for (int c = 0; c < M; ++c) f[c] = x[c] * fmaf(-p1 * x[c], x[c], p0);
    } else if constexpr (DR == 1) {
        f[0] = (fmaf(-(1.f / 3.f) * x[0] * x[0], x[0], x[0]) - x[1]) + p3;
        f[1] = p2 * fmaf(-p1, x[1], x[0] + p0);
    } else {
        f[0] = p0 * (x[1] - x[0]);
        f[1] = fmaf(x[0], p1 - x[2], -x[1]);
        f[2] = fmaf(x[0], x[1], -p2 * x[2]);
    }
}
template <int DR, int M>
__device__ __forceinline__ void diffusion_jte(const float (&x)[M], const float (&e)[M], float p0, float p1, float p2, float,
                                              float (&v)[M]) {
    if constexpr (DR == 0) {
#pragma unroll
        for (int c = 0; c < M; ++c) v[c] = fmaf(-3.f * p1 * x[c], x[c], p0) * e[c];
    } else if constexpr (DR == 1) {
        v[0] = fmaf(fmaf(-x[0], x[0], 1.f), e[0], p2 * e[1]);
        v[1] = fmaf(-p2 * p1, e[1], -e[0]);
    } else {
        v[0] = fmaf(x[1], e[2], fmaf(p1 - x[2], e[1], -p0 * e[0]));
        v[1] = fmaf(x[0], e[2], fmaf(p0, e[0], -e[1]));
        v[2] = fmaf(-x[0], e[1], -p2 * e[2]);
    }
}
// Diffusion bridge (NFMC_POT_DIFFUSION_BRIDGE, nfmc_hip.h): the latent path X_0 .. X_{T-1} in R^m of a discretised
// stochastic differential equation, time-major (coordinate t m + c is X_{t,c}), then p = log sigma and q = log tau when
// the scales are unknown.  T = p.n_components, the header p.a (kDif*), the rows y and w of n4 = 4 ceil(T m / 4) floats
// in p.b.  With e_t = X_t - X_{t-1} - dt f(X_{t-1}), om = 1 / (sigma^2 dt), rho = 1 / tau^2, S_e = sum_{t>=1} |e_t|^2,
// S_v = sum_{observed} (X - y)^2:
//   U       = 1/2 |X_0 - mu0|^2 / s0^2 + 1/2 om S_e + 1/2 rho S_v
//             [ + (T-1) m p + N_o q + ((p - l)^2 + (q - l)^2) / (2 c^2) ]
//   dU/dX_t = [t = 0] (X_0 - mu0) / s0^2 + [t >= 1] om e_t - [t < T-1] om (I + dt J_f(X_t))^T e_{t+1} + rho w_t (X_t - y_t)
//   dU/dp   = -om S_e + (T-1) m + (p - l) / c^2,    dU/dq = -rho S_v + N_o + (q - l) / c^2
// A coordinate needs the whole vectors X_{t-1}, X_t and X_{t+1}: up to nine values that with m = 3 straddle register quads
// and lanes at no fixed offset, so ds_bpermute (one register of one other lane, the register chosen at compile time)
// would take a fetch of every candidate register with selects behind it.  The exchange is IrtPot's and GmrfPot's instead:
// one wave-private LDS row of DP + 4 floats per chain (irt_floats), written once per evaluation, one 16-byte store per
// register quad; every lane then reads, per register quad, the window of steps the quad's four coordinates and their
// neighbours lie in (6, 8 or 12 values for m = 1, 2, 3: the steps tl - 1 .. tl + 4 or tl - 1 .. tl + 2) with ds_read_b32,
// evaluates the drift once per step of the window, and picks each coordinate's e_{t,c} and successor term from the
// step-major lists by its offset r in step tl (selects; r = 0 unless m = 3); p and q are read at positions T m and
// T m + 1 (one address per chain: a broadcast).  Every index is formed from a step clamped into 0 .. T-1, so it lies
// in the path's part of the chain's own row whatever the masks say.  The row is written and read by ONE
// wave: wavefront fences, no workgroup barrier.  (drift, m) is dispatched ONCE per prepare() to a body with compile-time
// bounds (ParticlePot's rule): no register array is indexed by a run-time value, the own component is taken by selects
// (never a run-time register index).  A lane recomputes the drift of the steps around its quads in the fixed order of
// diffusion_drift; e_{t,c}^2 enters S_e exactly once, at the coordinate (t, c) that owns it.  y and the roles "on the
// path" / "t >= 1" / "t < T-1" / "observed" (w != 0) are registers and bit masks set once in init() (SVPot); a padding
// coordinate has no role, adds exactly zero to U and both sums and gets a zero gradient.  S_e and S_v cross lanes through
// one group_allreduce each: fixed order, no atomics, bitwise repeatable.  Nothing is clamped: an overflowing e^{-2p} or
// cubic term gives a non-finite U, which the samplers reject and count.  term() puts the lane's share of U (its part of
// the X_0 term; the rest on the lane of coordinate 0) on its register 0.
template <int CPL, int LPC, bool FAST>
struct DiffusionPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    int nt, tm, drift, mm;               // T, T m, drift code, m
    bool unk, lead;                      // scales unknown / this lane holds coordinate 0 in register 0
    float dt, om0, rho0, mu0, is0, loc, ic2, nobs, tm1m, p0, p1, p2, p3;
    float y[CPL];                        // y of the lane's path coordinates (0 elsewhere)
    uint32_t in, pd, sc, ob;             // bit i: register i is on the path / has t >= 1 / has t < T-1 / is observed
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        drift = 0;
        mm = 1;
        unk = false;
        diffusion_code(p.a_scalar, drift, unk, mm);
        nt = p.n_components;
        tm = nt * mm;
        lead = (g == 0);
        const float* h = p.a;
        dt = h[kDifDt];
        om0 = 1.f / (h[kDifSigma] * h[kDifSigma] * dt);
        rho0 = 1.f / (h[kDifTau] * h[kDifTau]);
        mu0 = h[kDifMu0];
        is0 = h[kDifIs0];
        loc = h[kDifLoc];
        ic2 = h[kDifIc2];
        nobs = h[kDifNobs];
        tm1m = h[kDifTm1m];
        p0 = h[kDifPar0];
        p1 = h[kDifPar0 + 1];
        p2 = h[kDifPar0 + 2];
        p3 = h[kDifPar0 + 3];
        const int n4 = latent_row(tm);
        in = pd = sc = ob = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            y[i] = 0.f;
            if (c < tm) {
                y[i] = p.b[c];
                in |= 1u << i;
                if (c >= mm) pd |= 1u << i;
                if (c + mm < tm) sc |= 1u << i;
                if (p.b[n4 + c] != 0.f) ob |= 1u << i;
            }
        }
    }
    template <int DR, int M>
    __device__ __forceinline__ Ctx body(const float (&x)[CPL], int g) const {
        constexpr int NS = M == 1 ? 4 : 2;   // time steps a register quad touches: 4 (m = 1), 2 (m = 2), 2 (m = 3)
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int k = 0; k < Q; ++k)
            *reinterpret_cast<float4*>(row + 4 * (k * LPC + g)) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        order();   // the wave's stores precede its reads
        const float ps = unk ? row[tm] : 0.f, qs = unk ? row[tm + 1] : 0.f;
        const float om = unk ? fast_exp(-2.f * ps) / dt : om0, rho = unk ? fast_exp(-2.f * qs) : rho0;
        Ctx cx;
        float se = 0.f, sv = 0.f, u0 = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            // the quad's coordinates c0 .. c0 + 3 lie in the steps tl and tl + 1 (.. tl + 3 for m = 1), the first at
            // component r of step tl (r = 0 unless m = 3); a quad past the path reads about step T - 1, unused
            const int c0 = min(4 * (q * LPC + g), tm - 1);
            const int tl = c0 / M, r = c0 - tl * M;
            float w[NS + 2][M], e[NS + 1][M];   // X of the steps tl - 1 .. tl + NS (clamped into the path); e of tl .. tl + NS
#pragma unroll
            for (int s = 0; s < NS + 2; ++s) {
                const int b = min(max(tl - 1 + s, 0), nt - 1) * M;
#pragma unroll
                for (int k = 0; k < M; ++k) w[s][k] = row[b + k];
            }
#pragma unroll
            for (int s = 0; s < NS + 1; ++s) {
                float f[M];
                diffusion_drift<DR, M>(w[s], p0, p1, p2, p3, f);
#pragma unroll
                for (int k = 0; k < M; ++k) e[s][k] = fmaf(-dt, f[k], w[s + 1][k] - w[s][k]);
            }
            float ge[NS * M], gs[NS * M];       // step-major: e_{t,c} and ((I + dt J_f(X_t))^T e_{t+1})_c of the steps tl ..
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float jt[M];
                diffusion_jte<DR, M>(w[s + 1], e[s + 1], p0, p1, p2, p3, jt);
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    ge[s * M + k] = e[s][k];
                    gs[s * M + k] = fmaf(dt, jt[k], e[s + 1][k]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * q + j;
                float ej, sn;                   // entry r + j of the two lists, by selects
                if constexpr (M == 3) {
                    ej = r == 0 ? ge[j] : (r == 1 ? ge[j + 1] : ge[j + 2]);
                    sn = r == 0 ? gs[j] : (r == 1 ? gs[j + 1] : gs[j + 2]);
                } else {
                    ej = ge[j];
                    sn = gs[j];
                }
                const bool on = (in >> i) & 1u, hp = (pd >> i) & 1u, hs = (sc >> i) & 1u, ho = (ob >> i) & 1u;
                const float d0 = x[i] - mu0, rr = x[i] - y[i];
                float gr = (on && !hp) ? is0 * d0 : 0.f;
                u0 += (on && !hp) ? 0.5f * is0 * d0 * d0 : 0.f;
                gr = hp ? om * ej : gr;
                se += hp ? ej * ej : 0.f;
                gr = hs ? fmaf(-om, sn, gr) : gr;
                gr = ho ? fmaf(rho, rr, gr) : gr;
                sv += ho ? rr * rr : 0.f;
                cx.gr[i] = gr;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        se = group_allreduce<LPC>(se);
        sv = group_allreduce<LPC>(sv);
        float ug = 0.5f * (om * se + rho * sv);
        if (unk) {
            const float dp = ps - loc, dq = qs - loc;
            ug += fmaf(tm1m, ps, nobs * qs) + 0.5f * ic2 * fmaf(dp, dp, dq * dq);
            const float gp = fmaf(-om, se, tm1m) + dp * ic2, gq = fmaf(-rho, sv, nobs) + dq * ic2;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = coord_of<CPL, LPC>(g, i);
                cx.gr[i] = c == tm ? gp : (c == tm + 1 ? gq : cx.gr[i]);
            }
        }
        cx.u = u0 + (lead ? ug : 0.f);
        return cx;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        if (drift == 2) return body<2, 3>(x, g);
        if (drift == 1) return body<1, 2>(x, g);
        return mm == 3 ? body<0, 3>(x, g) : (mm == 2 ? body<0, 2>(x, g) : body<0, 1>(x, g));
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Diffusion bridge (NFMC_POT_DIFFUSION_BRIDGE) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// DiffusionPot (above), the path time-major and p = log sigma, q = log tau behind it when the scales are unknown.
// One pass over t: X_{t-1} carries over in registers, and e_t's successor term -om (I + dt J_f(X_{t-1}))^T e_t is added
// to the gradient of X_{t-1} when t is reached (sv_value_grad_row), so each coordinate reads the row once and the drift
// is evaluated once per step; S_e and S_v accumulate on the way and the scales' gradients follow the loop.  The header
// and the rows y, w are wave-uniform (scalar loads).  (drift, m) is chosen outside the loop.  Kept out of
// potential_value_grad_row, which the fit and DLMC kernels share and which never see kind 14.
template <int DR, int M>
__device__ __forceinline__ float diffusion_row(const float* __restrict__ row, float* __restrict__ grow, const NfmcPotential& p,
                                               bool unk) {
    const int nt = p.n_components, tm = nt * M, n4 = latent_row(tm);
    const float* __restrict__ h = p.a;
    const float* __restrict__ y = p.b;
    const float* __restrict__ w = p.b + n4;
    const float dt = h[kDifDt], mu0 = h[kDifMu0], is0 = h[kDifIs0];
    const float p0 = h[kDifPar0], p1 = h[kDifPar0 + 1], p2 = h[kDifPar0 + 2], p3 = h[kDifPar0 + 3];
    const float ps = unk ? row[tm] : 0.f, qs = unk ? row[tm + 1] : 0.f;
    const float om = unk ? fast_exp(-2.f * ps) / dt : 1.f / (h[kDifSigma] * h[kDifSigma] * dt);
    const float rho = unk ? fast_exp(-2.f * qs) : 1.f / (h[kDifTau] * h[kDifTau]);
    float xm[M], se = 0.f, sv = 0.f, u0 = 0.f;
#pragma unroll
    for (int c = 0; c < M; ++c) xm[c] = 0.f;
    for (int t = 0; t < nt; ++t) {
        float xt[M], gr[M];
#pragma unroll
        for (int c = 0; c < M; ++c) xt[c] = row[t * M + c];
        if (t == 0) {
#pragma unroll
            for (int c = 0; c < M; ++c) {
                const float d0 = xt[c] - mu0;
                gr[c] = is0 * d0;
                u0 = fmaf(0.5f * is0 * d0, d0, u0);
            }
        } else {
            float fm[M], e[M], jt[M];
            diffusion_drift<DR, M>(xm, p0, p1, p2, p3, fm);
#pragma unroll
            for (int c = 0; c < M; ++c) {
                e[c] = fmaf(-dt, fm[c], xt[c] - xm[c]);
                se = fmaf(e[c], e[c], se);
                gr[c] = om * e[c];
            }
            diffusion_jte<DR, M>(xm, e, p0, p1, p2, p3, jt);
#pragma unroll
            for (int c = 0; c < M; ++c) grow[(t - 1) * M + c] = fmaf(-om, fmaf(dt, jt[c], e[c]), grow[(t - 1) * M + c]);
        }
#pragma unroll
        for (int c = 0; c < M; ++c) {
            if (w[t * M + c] != 0.f) {
                const float r = xt[c] - y[t * M + c];
                sv = fmaf(r, r, sv);
                gr[c] = fmaf(rho, r, gr[c]);
            }
            grow[t * M + c] = gr[c];
            xm[c] = xt[c];
        }
    }
    float u = u0 + 0.5f * (om * se + rho * sv);
    if (unk) {
        const float loc = h[kDifLoc], ic2 = h[kDifIc2], nobs = h[kDifNobs], tm1m = h[kDifTm1m];
        const float dp = ps - loc, dq = qs - loc;
        u += fmaf(tm1m, ps, nobs * qs) + 0.5f * ic2 * fmaf(dp, dp, dq * dq);
        grow[tm] = fmaf(-om, se, tm1m) + dp * ic2;
        grow[tm + 1] = fmaf(-rho, sv, nobs) + dq * ic2;
    }
    return u;
}
__device__ __forceinline__ float diffusion_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                          const NfmcPotential& p, int) {
    int drift = 0, m = 1;
    bool unk = false;
    diffusion_code(p.a_scalar, drift, unk, m);
    return drift == 2 ? diffusion_row<2, 3>(row, grow, p, unk)
         : drift == 1 ? diffusion_row<1, 2>(row, grow, p, unk)
         : m == 3     ? diffusion_row<0, 3>(row, grow, p, unk)
         : m == 2     ? diffusion_row<0, 2>(row, grow, p, unk)
                      : diffusion_row<0, 1>(row, grow, p, unk);
}

}  // namespace nfmc
