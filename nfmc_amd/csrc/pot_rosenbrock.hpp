// Blocked Rosenbrock (kind 5): its register class and its one-row NeuTra form.
#pragma once

#include "common.hpp"

namespace nfmc {

// Blocked Rosenbrock (NFMC_POT_ROSENBROCK; block B = p.n_components, a = a_scalar, b = b_scalar, mu = p.a[0]):
//   U = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2,   c a head when c % B == 0
//   dU/dx_c = [head] 2a (x_c - mu) + [non-head] 2b (x_c - x_{c-1}^2) - [c+1 < d non-head] 4b x_c (x_{c+1} - x_c^2)
// Every coordinate couples to its neighbours c - 1 and c + 1 in the flattened order, and nothing else: no reduction and
// no LDS table.  Inside a register quad the neighbours are the lane's own registers.  Across the quad's ends, with
// quad q of lane g holding 4 (q LPC + g) .. + 3 (coord_of):
//   predecessor of its first coordinate = register 4q + 3 of lane g - 1, for g = 0 register 4(q - 1) + 3 of lane LPC - 1
//   successor of its last coordinate    = register 4q of lane g + 1, for g = LPC - 1 register 4(q + 1) of lane 0
// so prepare() fetches register 4q + 3 from lane (g - 1) mod LPC and register 4q from lane (g + 1) mod LPC for every
// quad (two ds_bpermute per quad; nothing with one lane per chain), and lane 0 / lane LPC - 1 take the neighbouring
// quad's fetch.  The head / non-head / successor roles of the lane's coordinates are bit masks set once in init();
// padding coordinates (c >= d) have none, so they add exactly zero to U and get a zero gradient, and a coordinate
// has a successor term only when c + 1 < d is a non-head.  term() puts the lane's share of U on its register 0.
template <int CPL, int LPC, bool FAST>
struct RosenbrockPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    static constexpr int Q = CPL / 4;   // register quads
    float ca, cb, mu;
    uint32_t hd, nh, sc;   // bit i: register i is a head / a non-head / has a successor term
    int prv, nxt;          // ds_bpermute byte addresses of lanes (g - 1) mod LPC and (g + 1) mod LPC of the group
    bool first, last;      // g == 0 / g == LPC - 1
    struct Ctx {
        float u;           // this lane's share of U
        float gr[CPL];     // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        ca = p.a_scalar;
        cb = p.b_scalar;
        mu = p.a[0];
        const int blk = p.n_components;
        hd = nh = sc = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            if (c < d) {
                if (c % blk == 0) hd |= 1u << i;
                else nh |= 1u << i;
                if (c + 1 < d && (c + 1) % blk != 0) sc |= 1u << i;
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
        float pv[Q], nv[Q];   // register 4q + 3 of lane g - 1 / register 4q of lane g + 1 (cyclic in the group)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            pv[q] = fetch(x[4 * q + 3], prv);
            nv[q] = fetch(x[4 * q], nxt);
        }
        Ctx cx;
        float u = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int q = i >> 2, k = i & 3;
            float xm, xn;   // x_{c-1}, x_{c+1} (any finite value where the mask bits leave them unused)
            if (k > 0) xm = x[i - 1];
            else if (q > 0) xm = first ? pv[q - 1] : pv[q];
            else xm = first ? 0.f : pv[0];
            if (k < 3) xn = x[i + 1];
            else if (q + 1 < Q) xn = last ? nv[q + 1] : nv[q];
            else xn = last ? 0.f : nv[q];
            float t = 0.f, gr = 0.f;
            if ((hd >> i) & 1u) {
                const float r = x[i] - mu;
                t = ca * (r * r);
                gr = 2.f * ca * r;
            } else if ((nh >> i) & 1u) {
                const float r = fmaf(-xm, xm, x[i]);
                t = cb * (r * r);
                gr = 2.f * cb * r;
            }
            if ((sc >> i) & 1u) gr = fmaf(-4.f * cb * x[i], fmaf(-x[i], x[i], xn), gr);
            u += t;
            cx.gr[i] = gr;
        }
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Blocked Rosenbrock (NFMC_POT_ROSENBROCK) for the row of one chain, as potential_value_grad_row:
//   U = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2,   c a head when c % B == 0
// One pass over the row: x_{c-1} and the residual of c (the successor term of c - 1) carry over in registers, so each
// coordinate reads the row once and writes its gradient once.  Kept out of potential_value_grad_row, which the fit and
// DLMC kernels share and which never see kind 5.
__device__ __forceinline__ float rosenbrock_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                           const NfmcPotential& p, int d) {
    const float ca = p.a_scalar, cb = p.b_scalar, mu = p.a[0];
    const int blk = p.n_components;
    float u = 0.f, xm = 0.f;
    int k = 0;   // c % blk
    for (int c = 0; c < d; ++c) {
        const float xc = row[c];
        float gr;
        if (k == 0) {
            const float r = xc - mu;
            u = fmaf(ca * r, r, u);
            gr = 2.f * ca * r;
        } else {
            const float r = fmaf(-xm, xm, xc);
            u = fmaf(cb * r, r, u);
            gr = 2.f * cb * r;
            grow[c - 1] = fmaf(-4.f * cb * xm, r, grow[c - 1]);   // successor term of c - 1
        }
        grow[c] = gr;
        xm = xc;
        k = k + 1 == blk ? 0 : k + 1;
    }
    return u;
}

}  // namespace nfmc
