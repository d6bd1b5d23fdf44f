// Varying-effects regression (kind 10): its register class and its one-row NeuTra form.
#pragma once

#include "pot_kinds.hpp"

namespace nfmc {

// One group of the varying-effects regression: from its statistics s0 = (n, xbar, ybar, Sxx), s1 = (Sxy, Syy, 0, 0) and its
// effects (a, b) on the natural scale, Q_c = n e^2 + Syy - 2 b Sxy + b^2 Sxx with e = ybar - a - b xbar, and
// gA = -w_y n e, gB = w_y (-n e xbar - Sxy + b Sxx).  Shared by VaryEffPot and vfx_value_grad_row (below).
__device__ __forceinline__ void vfx_group(const float4& s0, const float4& s1, float a, float b, float wy, float& qc,
                                          float& ga, float& gb) {
    const float e = fmaf(-b, s0.y, s0.z - a), ne = s0.x * e, bs = fmaf(b, s0.w, -s1.x);   // bs = b Sxx - Sxy
    qc = fmaf(ne, e, fmaf(b, bs - s1.x, s1.y));
    ga = -wy * ne;
    gb = wy * fmaf(-ne, s0.y, bs);
}
// One group coordinate xv of a varying side (mu, w = e^{-2s}, es = e^{s}) with the likelihood's gradient gv with respect
// to the natural effect.  Centered: r = xv - mu, s1 += r, s2 += r^2, gradient gv + w r (the prior's 1/2 w sum r^2 is
// added from s2).  Non-centered: s1 += gv, s2 += gv xv, u += 1/2 xv^2, gradient es gv + xv.
__device__ __forceinline__ float vfx_vary(bool ncp, float xv, float mu, float w, float es, float gv, float& s1, float& s2,
                                          float& u) {
    if (ncp) {
        s1 += gv;
        s2 = fmaf(gv, xv, s2);
        u = fmaf(0.5f * xv, xv, u);
        return fmaf(es, gv, xv);
    }
    const float r = xv - mu;
    s1 += r;
    s2 = fmaf(r, r, s2);
    return fmaf(w, r, gv);
}
// The globals of one side and their share of U, from the chain-wide sums (s1, s2) of vfx_vary (varying side) or
// s1 = sum gV_c (shared side): g0 = dU/dmu or dU/dv, g1 = dU/ds.  fc = C.
__device__ __forceinline__ float vfx_side_globals(int mode, bool ncp, float mu, float s, float w, float es, float s1, float s2,
                                                  float fc, float P, float Hh, float& g0, float& g1) {
    g1 = 0.f;
    if (mode == 2) {
        const float he = Hh * fast_exp(2.f * s);
        g0 = ncp ? fmaf(P, mu, s1) : fmaf(P, mu, -w * s1);
        g1 = (ncp ? es * s2 : fmaf(-w, s2, fc)) + he - 1.f;
        return fmaf(0.5f * P * mu, mu, fmaf(0.5f, he, ncp ? -s : fmaf(fc, s, -s)));
    }
    g0 = mode == 1 ? fmaf(P, mu, s1) : 0.f;
    return mode == 1 ? 0.5f * P * mu * mu : 0.f;
}

// Gaussian regression with varying effects (NFMC_POT_VARYING_EFFECTS; C = p.n_components groups, p.a = the group table,
// C rows (n, xbar, ybar, Sxx, Sxy, Syy, 0, 0), (P, Hh) = p.b[0 .. 1], layout code = a_scalar (vfx_layout), N = b_scalar).
// The formulas are in nfmc_hip.h.  Coordinates: the group block -- (a_c, b_c) interleaved when both sides vary, so a
// pair is two neighbouring registers of one lane (coord_of: quads start at multiples of 4), or v_c alone -- then up to
// five globals.  The globals start at coordinate gb = 2 C or C, anywhere in a register quad, and may run into the next
// quad in coordinate order: quad gb / 4 is register quad kA of lane gA, quad gb / 4 + 1 register quad kB of lane gB,
// all four wave-uniform and set once in init().  prepare() (1) picks the two register quads by uniform compares
// (k == kA, no dynamic register index), masks them to the lanes that hold them, shifts by off = gb % 4 (uniform
// selects) and broadcasts each global that exists with one group_allreduce of the masked value (SparseLogRegPot's
// pattern); (2) evaluates the lane's groups: the statistics of group j are two 16-byte loads from the table -- read per
// evaluation at every layout, not kept in registers: at CPL = 16 they would be 48 registers beside the 16 of the state
// and the 16 of the gradient in kernels that also carry momentum, proposal and a flow tail, the table is at most 32 KiB,
// the same for all chains, and stays in L1 / L2, and consecutive lanes read consecutive rows; (3) all-reduces sum Q_c
// and two sums per side (five fixed-order butterflies: bitwise repeatable); (4) forms the globals' gradients on every
// lane and writes them back through the same compares into the registers of the lanes that hold them; the globals'
// share of U goes to lane 0.  No LDS block.  A register that holds neither a group coordinate nor a global (padding) has
// no bit in `pm`, adds exactly zero to U and to every sum and gets a zero gradient.  term() puts the lane's share of U
// on its register 0.  e^{-2s}, e^{2s}, e^{s} overflow fp32 far in the tails; U is then inf or NaN, the samplers reject
// the state and count its log ratio as non-finite.
template <int CPL, int LPC, bool FAST>
struct VaryEffPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    static constexpr int Q = CPL / 4;   // register quads
    const float4* tab;                  // the group table, two float4 per group
    VfxLayout L;
    float P, Hh, nobs, fc;              // 1 / m^2, 1 / h^2, N, C
    int kA, kB, off;                    // register quads of the globals' first and second quad; gb % 4
    bool inA, inB, first;               // this lane holds the first / second quad; g == 0
    uint32_t pm;                        // bit i: register i is a group coordinate
    struct Ctx {
        float u;                        // this lane's share of U
        float gr[CPL];                  // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int) {
        tab = reinterpret_cast<const float4*>(p.a);
        vfx_layout(p.a_scalar, p.n_components, L);   // valid: check_vfx
        P = p.b[0];
        Hh = p.b[1];
        nobs = p.b_scalar;
        fc = (float)p.n_components;
        const int q0 = L.gb >> 2;
        off = L.gb & 3;
        kA = q0 / LPC;
        kB = (q0 + 1) / LPC;
        inA = g == q0 % LPC;
        inB = g == (q0 + 1) % LPC;
        first = g == 0;
        pm = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (coord_of<CPL, LPC>(g, i) < L.gb) pm |= 1u << i;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        // (1) the globals
        float cat[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // the two quads, each on the lane that holds it
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const bool a = inA && k == kA, b = inB && k == kB;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cat[j] = a ? x[4 * k + j] : cat[j];
                cat[4 + j] = b ? x[4 * k + j] : cat[4 + j];
            }
        }
        float val[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float v = cat[k];
#pragma unroll
            for (int o = 1; o < 4; ++o) v = off == o ? cat[k + o] : v;
            val[k] = group_allreduce<LPC>(k < L.ng ? v : 0.f);
        }
        const bool va = L.ma == 2, vb = L.mb == 2, ncp = L.ncp;
        // the roles by scalar selects on the uniform layout (an array indexed by L.ib or L.iy would go to scratch memory)
        const float v0 = val[0], v1 = val[1], v2 = val[2], v3 = val[3], v4 = val[4];
        const float mua = v0, sa = va ? v1 : 0.f;                         // mu_a or the shared a
        const float mub = L.mb ? (va ? v2 : v1) : 0.f;                    // mu_b, the shared b or 0
        const float sb = vb ? (va ? v3 : v2) : 0.f;
        const float sy = L.known ? 0.f : (L.iy == 1 ? v1 : L.iy == 2 ? v2 : L.iy == 3 ? v3 : v4);
        const float wy = L.known ? 1.f : fast_exp(-2.f * sy);
        const float wa = fast_exp(-2.f * sa), esa = fast_exp(sa), wb = fast_exp(-2.f * sb), esb = fast_exp(sb);
        // (2) the lane's groups
        Ctx cx;
        float u = 0.f, sq = 0.f, a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
        if (va && vb) {
#pragma unroll
            for (int p = 0; p < CPL / 2; ++p) {
                cx.gr[2 * p] = 0.f;
                cx.gr[2 * p + 1] = 0.f;
                if ((pm >> (2 * p)) & 1u) {
                    const int j = 2 * ((p >> 1) * LPC + g) + (p & 1);
                    const float4 s0 = tab[2 * j], s1 = tab[2 * j + 1];
                    const float xa = x[2 * p], xb = x[2 * p + 1];
                    float qc, ga, gb;
                    vfx_group(s0, s1, ncp ? fmaf(esa, xa, mua) : xa, ncp ? fmaf(esb, xb, mub) : xb, wy, qc, ga, gb);
                    sq += qc;
                    cx.gr[2 * p] = vfx_vary(ncp, xa, mua, wa, esa, ga, a1, a2, u);
                    cx.gr[2 * p + 1] = vfx_vary(ncp, xb, mub, wb, esb, gb, b1, b2, u);
                }
            }
            u = ncp ? u : fmaf(0.5f * wa, a2, fmaf(0.5f * wb, b2, u));
        } else {
            const float muv = va ? mua : mub, wv = va ? wa : wb, esv = va ? esa : esb;
            float v1 = 0.f, v2 = 0.f, o1 = 0.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                cx.gr[i] = 0.f;
                if ((pm >> i) & 1u) {
                    const int j = coord_of<CPL, LPC>(g, i);
                    const float4 s0 = tab[2 * j], s1 = tab[2 * j + 1];
                    const float xv = x[i], v = ncp ? fmaf(esv, xv, muv) : xv;
                    float qc, ga, gb;
                    vfx_group(s0, s1, va ? v : mua, va ? mub : v, wy, qc, ga, gb);
                    sq += qc;
                    cx.gr[i] = vfx_vary(ncp, xv, muv, wv, esv, va ? ga : gb, v1, v2, u);
                    o1 += va ? gb : ga;
                }
            }
            u = ncp ? u : fmaf(0.5f * wv, v2, u);
            a1 = va ? v1 : o1;
            a2 = va ? v2 : 0.f;
            b1 = va ? o1 : v1;
            b2 = va ? 0.f : v2;
        }
        u = fmaf(0.5f * wy, sq, u);
        // (3) the chain-wide sums
        sq = group_allreduce<LPC>(sq);
        a1 = group_allreduce<LPC>(a1);
        a2 = group_allreduce<LPC>(a2);
        b1 = group_allreduce<LPC>(b1);
        b2 = group_allreduce<LPC>(b2);
        // (4) the globals' gradients, in the order of the coordinates
        float ga0, ga1, gb0, gb1;
        float ug = vfx_side_globals(L.ma, ncp, mua, sa, wa, esa, a1, a2, fc, P, Hh, ga0, ga1);
        ug += vfx_side_globals(L.mb, ncp, mub, sb, wb, esb, b1, b2, fc, P, Hh, gb0, gb1);
        float gy = 0.f;
        if (!L.known) {
            const float he = Hh * fast_exp(2.f * sy);
            gy = fmaf(-wy, sq, nobs) + he - 1.f;
            ug += fmaf(nobs, sy, fmaf(0.5f, he, -sy));
        }
        float gl[5];
        gl[0] = ga0;
        gl[1] = va ? ga1 : (L.mb ? gb0 : gy);
        gl[2] = va ? (L.mb ? gb0 : gy) : (vb ? gb1 : gy);
        gl[3] = (va && vb) ? gb1 : gy;
        gl[4] = gy;
        float cg[8];   // the gradients at their places in the two quads
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (q - o >= 0 && q - o < 5) v = off == o ? gl[q - o] : v;
            cg[q] = v;
        }
        const int end = off + L.ng;   // the globals are places off .. end - 1 of the two quads
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const bool a = inA && k == kA, b = inB && k == kB;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cx.gr[4 * k + j] = (a && j >= off && j < end) ? cg[j] : cx.gr[4 * k + j];
                cx.gr[4 * k + j] = (b && 4 + j < end) ? cg[4 + j] : cx.gr[4 * k + j];
            }
        }
        cx.u = first ? u + ug : u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Varying-effects regression (NFMC_POT_VARYING_EFFECTS) for the row of one chain, as potential_value_grad_row: U and
// dU/dx of VaryEffPot (above), the group block first and the globals behind it.  One pass over the groups: the
// table row of a group (two 16-byte loads), the layout and (P, Hh) are wave-uniform; the group's one or two coordinates
// are read from and its gradient written to the lane's own LDS row; the five sums run in registers and the globals'
// gradients follow the pass.  O(d), no pass over the observations.  Kept out of potential_value_grad_row, which the fit
// and DLMC kernels share and which never see kind 10.
__device__ __forceinline__ float vfx_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                    const NfmcPotential& p, int) {
    VfxLayout L;
    vfx_layout(p.a_scalar, p.n_components, L);   // valid: check_vfx
    const int nc = p.n_components;
    const bool va = L.ma == 2, vb = L.mb == 2, both = va && vb, ncp = L.ncp;
    const float P = p.b[0], Hh = p.b[1], fc = (float)nc;
    const float* __restrict__ gl = row + L.gb;
    float* __restrict__ gg = grow + L.gb;
    const float mua = gl[0], sa = va ? gl[1] : 0.f, mub = L.mb ? gl[L.ib] : 0.f, sb = vb ? gl[L.ib + 1] : 0.f;
    const float sy = L.known ? 0.f : gl[L.iy];
    const float wy = L.known ? 1.f : fast_exp(-2.f * sy);
    const float wa = fast_exp(-2.f * sa), esa = fast_exp(sa), wb = fast_exp(-2.f * sb), esb = fast_exp(sb);
    const float4* __restrict__ tab = reinterpret_cast<const float4*>(p.a);
    float u = 0.f, sq = 0.f, a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float4 s0 = tab[2 * c], s1 = tab[2 * c + 1];
        const int ia = both ? 2 * c : c, ib = both ? 2 * c + 1 : c;
        const float xa = va ? row[ia] : 0.f, xb = vb ? row[ib] : 0.f;
        const float a = va ? (ncp ? fmaf(esa, xa, mua) : xa) : mua, b = vb ? (ncp ? fmaf(esb, xb, mub) : xb) : mub;
        float qc, ga, gb;
        vfx_group(s0, s1, a, b, wy, qc, ga, gb);
        sq += qc;
        if (va) grow[ia] = vfx_vary(ncp, xa, mua, wa, esa, ga, a1, a2, u);
        else a1 += ga;
        if (vb) grow[ib] = vfx_vary(ncp, xb, mub, wb, esb, gb, b1, b2, u);
        else b1 += gb;
    }
    if (!ncp) u = fmaf(0.5f * wa, va ? a2 : 0.f, fmaf(0.5f * wb, vb ? b2 : 0.f, u));
    u = fmaf(0.5f * wy, sq, u);
    float g0, g1;
    u += vfx_side_globals(L.ma, ncp, mua, sa, wa, esa, a1, a2, fc, P, Hh, g0, g1);
    gg[0] = g0;
    if (va) gg[1] = g1;
    u += vfx_side_globals(L.mb, ncp, mub, sb, wb, esb, b1, b2, fc, P, Hh, g0, g1);
    if (L.mb) gg[L.ib] = g0;
    if (vb) gg[L.ib + 1] = g1;
    if (!L.known) {
        const float he = Hh * fast_exp(2.f * sy);
        gg[L.iy] = fmaf(-wy, sq, p.b_scalar) + he - 1.f;
        u += fmaf(p.b_scalar, sy, fmaf(0.5f, he, -sy));
    }
    return u;
}

}  // namespace nfmc
