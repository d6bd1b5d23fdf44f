// phi^4 lattice field (kind 8): its register class and its one-row NeuTra form.
#pragma once

#include "pot_kinds.hpp"

namespace nfmc {

// phi^4 scalar field on a lattice (NFMC_POT_LATTICE_PHI4; rows of W = p.n_components sites, H = d / W of them, row-major;
// (m2, lam, kappa, boundary) = p.a[0 .. 3], boundary 0 periodic / 1 zero field outside).  With L_c = sum over the
// neighbours c' of c of (x_c - x_c') -- two per axis; a periodic axis wraps, a zero-boundary axis reads 0 past its ends:
//   dU/dx_c = m2 x_c + lam x_c^3 + kappa L_c
//   U = sum_c x_c [1/2 m2 x_c + 1/4 lam x_c^3 + 1/2 kappa L_c]
// (sum_c x_c L_c counts (x_c' - x_c)^2 once per bond, a boundary bond of the zero boundary included: each bond's
// a^2 + b^2 - 2ab is a (a - b) at one end plus b (b - a) at the other).  H = 1 is the 1-D lattice: no second axis.
// W % 4 == 0 (check_phi4), so every lattice row starts on a register quad and d % 4 == 0: inside a quad the left and
// right neighbours are the lane's own registers, the upper and lower neighbours of a quad are ONE aligned quad W floats
// before / behind it in the chain's row, and only register 0's left and register 3's right neighbour lie in other quads.
// In the interleaved layout those quads sit in other lanes at a register index that depends on the lane, so the lanes
// exchange through LDS, not through ds_bpermute (one permute per source register and a select chain per target quad):
// the workgroup's block is one zeroed quad and one row of DP floats per chain (phi4_floats); prepare() stores the
// lane's quads into its chain's row (ds_write_b128) and reads, per quad, the upper and the lower quad (ds_read_b128) and
// the two single neighbours (ds_read_b32): 5 Q LDS operations per evaluation.  The four addresses of a quad are set once
// in init().  A periodic wrap is another address in the row; a neighbour the zero boundary leaves out is the zeroed
// quad; with H = 1 "up" and "down" are the quad itself, whose differences are exactly zero; a padding quad (c >= d)
// reads the zeroed quad and has no bit in `ok`, so its term and gradient are exactly zero.  No branch on the boundary
// in prepare().  A chain's row is written and read by the lanes of ONE wave, whose LDS operations complete in order, so
// no workgroup barrier is needed (and none is possible: the waves do not call prepare() in step); wavefront-scope fences
// and wave barriers keep the compiler from moving the reads over the stores of this or the next evaluation.  term() puts
// the lane's share of U on its register 0.
template <int CPL, int LPC, bool FAST>
struct Phi4Pot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;   // register quads
    float* blk;                          // LDS: zero quad | rows (kBlock / LPC, DP)
    float m2, lam, kap;
    int own;                             // float index of this lane's quad 0 in its chain's row (quad q: + 4 q LPC)
    int up[Q], dn[Q], lf[Q], rt[Q];      // float indices of the quad above / below and of the single neighbours
    uint32_t ok;                         // bit q: quad q holds lattice sites (c < d)
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // all threads of the workgroup; the caller synchronises before the first prepare()
    __device__ __forceinline__ static void stage(float* __restrict__ lds, const NfmcPotential&, int) {
        if (threadIdx.x < 4) lds[threadIdx.x] = 0.f;
    }
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        blk = lds;
        m2 = p.a[0];
        lam = p.a[1];
        kap = p.a[2];
        const bool zero = p.a[3] != 0.f;
        const int W = p.n_components, H = d / W;
        const int row = 4 + (int)(threadIdx.x / LPC) * DP;   // this chain's row, behind the zero quad
        own = row + 4 * g;
        ok = 0u;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c0 = 4 * (q * LPC + g);   // the quad's first site (coord_of)
            up[q] = dn[q] = lf[q] = rt[q] = 0;  // the zero quad
            if (c0 < d) {
                ok |= 1u << q;
                const int r = c0 / W, k = c0 - r * W, at = row + c0;
                if (k > 0) lf[q] = at - 1;
                else if (!zero) lf[q] = at + W - 1;
                if (k + 4 < W) rt[q] = at + 4;
                else if (!zero) rt[q] = at + 4 - W;
                if (H == 1) {
                    up[q] = dn[q] = at;
                } else {
                    if (r > 0) up[q] = at - W;
                    else if (!zero) up[q] = at + (H - 1) * W;
                    if (r + 1 < H) dn[q] = at + W;
                    else if (!zero) dn[q] = at - (H - 1) * W;
                }
            }
        }
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int q = 0; q < Q; ++q)
            *reinterpret_cast<float4*>(blk + own + 4 * q * LPC) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
        order();   // the wave's stores precede its reads
        Ctx cx;
        float u = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(blk + up[q]), b = *reinterpret_cast<const float4*>(blk + dn[q]);
            const float va[4] = {a.x, a.y, a.z, a.w}, vb[4] = {b.x, b.y, b.z, b.w};
            const float row[6] = {blk[lf[q]], x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3], blk[rt[q]]};
            const bool site = (ok >> q) & 1u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xc = row[k + 1];
                const float L = ((xc - row[k]) + (xc - row[k + 2])) + ((xc - va[k]) + (xc - vb[k]));
                const float x2 = xc * xc;
                const float gr = fmaf(kap, L, xc * fmaf(lam, x2, m2));
                const float t = xc * fmaf(0.5f * kap, L, xc * fmaf(0.25f * lam, x2, 0.5f * m2));
                cx.gr[4 * q + k] = site ? gr : 0.f;
                u += site ? t : 0.f;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// phi^4 lattice field (NFMC_POT_LATTICE_PHI4) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// Phi4Pot (above), H = d / W rows of W = n_components sites.  A plain loop over the sites with index arithmetic for
// the four neighbours (two with H = 1): a periodic axis wraps, the zero boundary reads 0 past its ends.  The constants
// are wave-uniform (scalar loads).  Kept out of potential_value_grad_row, which the fit and DLMC kernels share and which
// never see kind 8.
__device__ __forceinline__ float phi4_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                     const NfmcPotential& p, int d) {
    const float m2 = p.a[0], lam = p.a[1], kap = p.a[2];
    const bool zero = p.a[3] != 0.f;
    const int W = p.n_components, H = d / W, wrap = (H - 1) * W;
    float u = 0.f;
    int c = 0;
    for (int r = 0; r < H; ++r) {
        for (int k = 0; k < W; ++k, ++c) {
            const float xc = row[c];
            const float xl = k > 0 ? row[c - 1] : (zero ? 0.f : row[c + W - 1]);
            const float xr = k + 1 < W ? row[c + 1] : (zero ? 0.f : row[c + 1 - W]);
            float L = (xc - xl) + (xc - xr);
            if (H > 1) {
                const float xu = r > 0 ? row[c - W] : (zero ? 0.f : row[c + wrap]);
                const float xd = r + 1 < H ? row[c + W] : (zero ? 0.f : row[c - wrap]);
                L += (xc - xu) + (xc - xd);
            }
            const float x2 = xc * xc;
            grow[c] = fmaf(kap, L, xc * fmaf(lam, x2, m2));
            u = fmaf(xc, fmaf(0.5f * kap, L, xc * fmaf(0.25f * lam, x2, 0.5f * m2)), u);
        }
    }
    return u;
}

}  // namespace nfmc
