// Stochastic volatility (kind 6): its register class and its one-row NeuTra form.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

// Stochastic volatility (NFMC_POT_STOCHASTIC_VOLATILITY; T = p.n_components = d - 3, y = p.a[0 .. T-1], (alpha, beta) =
// p.b[0 .. 1], c_mu = a_scalar, c_sigma = b_scalar).  Coordinates x_0 = mu, x_1 = s = log sigma, x_2 = r = atanh phi,
// x_{3+t} = h_t; with w = e^{-2s}, phi = tanh r, q = 1 - phi^2, delta_0 = h_0 - mu, a_t = h_{t-1} - mu, e_t = h_t - mu -
// phi a_t (t >= 1) and S1 = sum e_t, S2 = sum e_t^2, S3 = sum e_t a_t:
//   U = log1p((mu/c_mu)^2) + softplus(2(s - log c_sigma)) + (alpha + 1/2) softplus(-2r) + (beta + 1/2) softplus(2r)
//     + 1/2 q w delta_0^2 + (T - 1) s + sum_{t>=1} 1/2 w e_t^2 + sum_{t>=0} 1/2 [h_t + y_t^2 e^{-h_t}]
//   dU/dmu  = 2 mu/(c_mu^2 + mu^2) - q w delta_0 - (1 - phi) w S1
//   dU/ds   = 2 sigmoid(2(s - log c_sigma)) - q w delta_0^2 - w S2 + (T - 1)
//   dU/dr   = 2(beta + 1/2) sigmoid(2r) - 2(alpha + 1/2) sigmoid(-2r) - phi q w delta_0^2 - q w S3
//   dU/dh_t = 1/2 - 1/2 y_t^2 e^{-h_t} + [t = 0] q w delta_0 + [t >= 1] w e_t - [t + 1 < T] phi w e_{t+1}
// (the -s of sigma's Jacobian and the +s of h_0's normaliser cancel).  mu, s, r and h_0 are coordinates 0 .. 3, register
// quad 0 of lane 0 at every layout (coord_of).  prepare() broadcasts registers 0 .. 2 of lane 0 to the chain's lanes
// (FunnelPot), fetches the neighbours h_{t-1} and h_{t+1} across register quads and lanes with RosenbrockPot's two
// ds_bpermute per quad, forms every h_t's terms lane-locally, and all-reduces S1, S2 and S3 (one butterfly each); lane 0
// then writes the global gradients into its registers 0 .. 2 and adds delta_0's term to h_0's.  y_t^2 of the lane's h
// coordinates sit in registers (QuadraticPot's b[]); the "is an h" / "has a predecessor term" (t >= 1) / "has a successor
// term" (t + 1 < T) roles are bit masks set once in init().  Padding coordinates have none, so they add exactly zero to U
// and the sums and get a zero gradient.  q = 4 sigmoid(2r) sigmoid(-2r) and 1 - phi = 2 sigmoid(-2r) stay finite and
// accurate at any r; w and e^{-h_t} overflow fp32 for s < -44 or h_t < -88, and such a state's U is inf or NaN, so the
// samplers reject it and count its log ratio as non-finite.  term() puts the lane's share of U on its register 0.
template <int CPL, int LPC, bool FAST>
struct SVPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    static constexpr int Q = CPL / 4;   // register quads
    float cmu, lcs, ca, cb, tm1;        // c_mu, log c_sigma, alpha + 1/2, beta + 1/2, T - 1
    float y2[CPL];                      // y_t^2 of the lane's h coordinates (0 elsewhere)
    uint32_t hm, pd, sc;                // bit i: register i is an h_t / has t >= 1 / has t + 1 < T
    int prv, nxt;                       // ds_bpermute byte addresses of lanes (g - 1) mod LPC and (g + 1) mod LPC
    bool first, last;                   // g == 0 (holds mu, s, r, h_0) / g == LPC - 1
    struct Ctx {
        float u;                        // this lane's share of U
        float gr[CPL];                  // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        cmu = p.a_scalar;
        lcs = logf(p.b_scalar);
        ca = p.b[0] + 0.5f;
        cb = p.b[1] + 0.5f;
        tm1 = (float)(p.n_components - 1);
        hm = pd = sc = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            y2[i] = 0.f;
            if (c >= 3 && c < d) {
                const float yv = p.a[c - 3];
                y2[i] = yv * yv;
                hm |= 1u << i;
                if (c >= 4) pd |= 1u << i;
                if (c + 1 < d) sc |= 1u << i;
            }
        }
        const int base = (int)(threadIdx.x & 63) - g;
        prv = 4 * (base + (g + LPC - 1) % LPC);
        nxt = 4 * (base + (g + 1) % LPC);
        first = g == 0;
        last = g == LPC - 1;
    }
    __device__ __forceinline__ static float fetch(float v, int addr) {
        if constexpr (LPC == 1) return v;
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        const float mu = group_broadcast0<LPC>(x[0]), s = group_broadcast0<LPC>(x[1]), r = group_broadcast0<LPC>(x[2]);
        float pv[Q], nv[Q];   // register 4q + 3 of lane g - 1 / register 4q of lane g + 1 (cyclic in the group)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            pv[q] = fetch(x[4 * q + 3], prv);
            nv[q] = fetch(x[4 * q], nxt);
        }
        float spp, sgp, spm, sgm;   // softplus / sigmoid of 2r and of -2r
        softplus_sigmoid(2.f * r, spp, sgp);
        softplus_sigmoid(-2.f * r, spm, sgm);
        const float phi = sgp - sgm, w = fast_exp(-2.f * s), pw = phi * w;
        Ctx cx;
        float u = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int q = i >> 2, k = i & 3;
            float xm, xn;   // h_{t-1}, h_{t+1} (any finite value where the mask bits leave them unused)
            if (k > 0) xm = x[i - 1];
            else if (q > 0) xm = first ? pv[q - 1] : pv[q];
            else xm = first ? 0.f : pv[0];
            if (k < 3) xn = x[i + 1];
            else if (q + 1 < Q) xn = last ? nv[q + 1] : nv[q];
            else xn = last ? 0.f : nv[q];
            float t = 0.f, gr = 0.f;
            if ((hm >> i) & 1u) {
                const float ye = y2[i] * fast_exp(-x[i]), dh = x[i] - mu;
                t = 0.5f * (x[i] + ye);
                gr = fmaf(-0.5f, ye, 0.5f);
                if ((pd >> i) & 1u) {
                    const float a = xm - mu, e = fmaf(-phi, a, dh);
                    t = fmaf(0.5f * w * e, e, t);
                    gr = fmaf(w, e, gr);
                    s1 += e;
                    s2 = fmaf(e, e, s2);
                    s3 = fmaf(e, a, s3);
                }
                if ((sc >> i) & 1u) gr = fmaf(-pw, fmaf(-phi, dh, xn - mu), gr);   // - phi w e_{t+1}
            }
            u += t;
            cx.gr[i] = gr;
        }
        s1 = group_allreduce<LPC>(s1);
        s2 = group_allreduce<LPC>(s2);
        s3 = group_allreduce<LPC>(s3);
        if (first) {
            const float d0 = x[3] - mu, qw = 4.f * sgp * sgm * w, qwd = qw * d0, m = mu / cmu;
            float sps, sgs;   // softplus / sigmoid of 2(s - log c_sigma)
            softplus_sigmoid(2.f * (s - lcs), sps, sgs);
            cx.gr[0] = 2.f * m / (cmu * fmaf(m, m, 1.f)) - qwd - 2.f * sgm * w * s1;
            cx.gr[1] = 2.f * sgs - qwd * d0 - w * s2 + tm1;
            cx.gr[2] = 2.f * cb * sgp - 2.f * ca * sgm - phi * qwd * d0 - qw * s3;
            cx.gr[3] += qwd;
            u += log1pf(m * m) + sps + tm1 * s + ca * spm + cb * spp + 0.5f * qwd * d0;
        }
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Stochastic volatility (NFMC_POT_STOCHASTIC_VOLATILITY) for the row of one chain, as potential_value_grad_row: U and
// dU/dx of SVPot (above), x_0 = mu, x_1 = log sigma, x_2 = atanh phi, x_{3+t} = h_t.  One pass over h_0 .. h_{T-1}:
// h_{t-1} carries over in a register, and e_t (the successor term of t - 1) is added to the gradient of h_{t-1} when t is
// reached, so each coordinate reads the row once; the sums S1, S2, S3 accumulate on the way and the global gradients
// follow the loop.  y is wave-uniform (scalar loads).  Kept out of potential_value_grad_row, which the fit and DLMC
// kernels share and which never see kind 6.
__device__ __forceinline__ float sv_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                   const NfmcPotential& p, int d) {
    const float* __restrict__ y = p.a;
    const float cmu = p.a_scalar, ca = p.b[0] + 0.5f, cb = p.b[1] + 0.5f, tm1 = (float)(d - 4);
    const float mu = row[0], s = row[1], r = row[2];
    float spp, sgp, spm, sgm, sps, sgs;   // softplus / sigmoid of 2r, -2r and 2(s - log c_sigma)
    softplus_sigmoid(2.f * r, spp, sgp);
    softplus_sigmoid(-2.f * r, spm, sgm);
    softplus_sigmoid(2.f * (s - logf(p.b_scalar)), sps, sgs);
    const float phi = sgp - sgm, w = fast_exp(-2.f * s), pw = phi * w;
    float u = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, hm = 0.f;
    for (int c = 3; c < d; ++c) {
        const float h = row[c], yv = y[c - 3];
        const float ye = (yv * yv) * fast_exp(-h), dh = h - mu;
        u += 0.5f * (h + ye);
        float gr = fmaf(-0.5f, ye, 0.5f);
        if (c > 3) {
            const float a = hm - mu, e = fmaf(-phi, a, dh);
            u = fmaf(0.5f * w * e, e, u);
            gr = fmaf(w, e, gr);
            grow[c - 1] = fmaf(-pw, e, grow[c - 1]);   // successor term of h_{t-1}
            s1 += e;
            s2 = fmaf(e, e, s2);
            s3 = fmaf(e, a, s3);
        }
        grow[c] = gr;
        hm = h;
    }
    const float d0 = row[3] - mu, qw = 4.f * sgp * sgm * w, qwd = qw * d0, m = mu / cmu;
    grow[0] = 2.f * m / (cmu * fmaf(m, m, 1.f)) - qwd - 2.f * sgm * w * s1;
    grow[1] = 2.f * sgs - qwd * d0 - w * s2 + tm1;
    grow[2] = 2.f * cb * sgp - 2.f * ca * sgm - phi * qwd * d0 - qw * s3;
    grow[3] += qwd;
    return u + log1pf(m * m) + sps + tm1 * s + ca * spm + cb * spp + 0.5f * qwd * d0;
}

}  // namespace nfmc
