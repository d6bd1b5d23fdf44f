// Latent Gaussian model (kind 12): its register class and its one-row NeuTra form.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

// Latent Gaussian model (NFMC_POT_LATENT_GAUSSIAN, nfmc_hip.h): a Gaussian prior N(m, K) on f with a likelihood term
// l_j(f_j) per coordinate (latent_lik, pot_shared.hpp).
// centred (x = f):  U = 1/2 r^T Lambda r + sum_j l_j(x_j),  dU/dx = Lambda r + l'(x),  r = x - m;
// whitened (x = z, f = m + L z):  U = 1/2 |z|^2 + sum_j l_j(f_j),  dU/dz = z + L^T l'(f).
// matvec() is GaussFullPot's loop: the (d, d) row-major matrix M streams through the LDS tile and every lane adds
// v_i M_ij to its own coordinates j, v_i broadcast from its owner, one ds_read_b128 per register quad and row, no
// reduction per row: out += M^T v.  The centred form is one pass (M = Lambda = Lambda^T, v = r).  The whitened form is
// two passes through the same tile: M = L^T with v = z leaves L z in the lane's registers, the lane evaluates l and l'
// of its own coordinates, and M = L with v = l'(f) gives L^T l'.  The known-zero triangle of L is streamed like the
// rest.  The rows m, y, w are read from the table (global memory, one 16-byte load per register quad) where they are
// used, not held in registers across the sampler's loop.  U: lane-local sums, then ONE group_allreduce.  The tile rule
// of LogRegPot holds: every thread of the workgroup calls prepare() equally often; the parameterisation is
// workgroup-uniform, so every thread runs the same number of passes.  Likelihood and parameterisation are dispatched
// once per prepare(), outside the loops.  Padding coordinates have v = 0, zero rows / columns and w = 0.
template <int CPL, int LPC, bool FAST>
struct LatentGaussPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int T = kLogRegTileFloats / DP;   // matrix rows per tile
    static_assert(T % 4 == 0, "whole register quads per tile");
    float* tile;          // LDS: matrix rows (T, DP)
    const float* mat;     // Lambda | L^T then L
    const float* tab;     // rows m, y, w of d4 floats (behind the 8 floats of the header)
    int dd, d4;
    int grp;              // byte address of the chain's first lane for ds_bpermute
    int lik;
    bool white;
    bool lead;            // this lane holds coordinate 0 in register 0
    float c0, c1, c2;     // Student-t constants
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        mat = p.a;
        tab = p.b + 8;
        dd = d;
        d4 = latent_row(d);
        grp = 4 * ((int)(threadIdx.x & 63) - g);
        lead = (g == 0);
        lik = 0;
        white = false;
        latent_code(p.a_scalar, lik, white);
        c0 = p.b[0];
        c1 = p.b[1];
        c2 = p.b[2];
    }
    // value v of lane `src` (uniform) of this lane's chain group
    __device__ __forceinline__ float from_lane(float v, int src) const {
        if constexpr (LPC == 1) return v;
        else if constexpr (LPC == 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(grp + 4 * src, __float_as_int(v)));
    }
    // register quad q of table row k (0 m, 1 y, 2 w) for this lane; zeros past the row
    __device__ __forceinline__ float4 tab4(int k, int q, int g) const {
        const int c = 4 * (q * LPC + g);
        return c < d4 ? *reinterpret_cast<const float4*>(tab + k * d4 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // all threads of the workgroup: out += M^T v, M (dd, dd) row-major in global memory, v = 0 on padding coordinates
    __device__ __forceinline__ void matvec(const float* __restrict__ M, const float (&v)[CPL], float (&out)[CPL], int g) const {
        for (int t0 = 0; t0 < dd; t0 += T) {
            const int rows = dd - t0 < T ? dd - t0 : T;
            load_tile_rows<DP>(tile, M, dd, t0, rows);
            __syncthreads();
            const int b1 = (t0 + rows + 3) >> 2;   // register quads (4 rows each) of this tile: t0 / 4 .. b1 - 1
            for (int b = t0 >> 2; b < b1;) {
                const int q = b / LPC;             // the quad's register index, constant over LPC consecutive quads
                float vq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < CPL / 4; ++k)
                    if (k == q) {
                        vq[0] = v[4 * k];
                        vq[1] = v[4 * k + 1];
                        vq[2] = v[4 * k + 2];
                        vq[3] = v[4 * k + 3];
                    }
                const int bq = b1 < (q + 1) * LPC ? b1 : (q + 1) * LPC;
                for (; b < bq; ++b) {
                    const int src = b - q * LPC;   // the lane that holds coordinates 4 b .. 4 b + 3
                    const float vi[4] = {from_lane(vq[0], src), from_lane(vq[1], src), from_lane(vq[2], src),
                                         from_lane(vq[3], src)};
                    const float* rows4 = tile + (4 * b - t0) * DP + 4 * g;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int k = 0; k < CPL / 4; ++k) {
                            const float4 w = *reinterpret_cast<const float4*>(rows4 + c * DP + 4 * k * LPC);
                            out[4 * k] = fmaf(vi[c], w.x, out[4 * k]);
                            out[4 * k + 1] = fmaf(vi[c], w.y, out[4 * k + 1]);
                            out[4 * k + 2] = fmaf(vi[c], w.z, out[4 * k + 2]);
                            out[4 * k + 3] = fmaf(vi[c], w.w, out[4 * k + 3]);
                        }
                    }
                }
            }
        }
    }
    // l'(f) of this lane's coordinates into lp, their share of sum_j l_j(f_j) returned
    template <int LIK>
    __device__ __forceinline__ float likelihood(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < CPL / 4; ++q) {
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
        Ctx cx;
        float v[CPL], mv[CPL];   // x on the real coordinates, 0 on the padding / the prior mean
#pragma unroll
        for (int q = 0; q < CPL / 4; ++q) {
            const float4 m = tab4(0, q, g);
            mv[4 * q] = m.x;
            mv[4 * q + 1] = m.y;
            mv[4 * q + 2] = m.z;
            mv[4 * q + 3] = m.w;
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) v[i] = coord_of<CPL, LPC>(g, i) < dd ? x[i] : 0.f;
        float s = 0.f;
        if (white) {
            float f[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) f[i] = 0.f;
            matvec(mat, v, f, g);                                   // L z
#pragma unroll
            for (int i = 0; i < CPL; ++i) f[i] += mv[i];
            float lp[CPL];
            s = likelihood_of(f, lp, g);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                cx.gr[i] = v[i];
                s = fmaf(0.5f * v[i], v[i], s);
            }
            matvec(mat + (int64_t)dd * dd, lp, cx.gr, g);           // z + L^T l'(f)
        } else {
            float r[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                r[i] = coord_of<CPL, LPC>(g, i) < dd ? x[i] - mv[i] : 0.f;
                cx.gr[i] = 0.f;
            }
            matvec(mat, r, cx.gr, g);                               // Lambda r
            float lp[CPL];
            s = likelihood_of(v, lp, g);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                s = fmaf(0.5f * r[i], cx.gr[i], s);
                cx.gr[i] += lp[i];
            }
        }
        cx.u = group_allreduce<LPC>(s);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Latent Gaussian model (NFMC_POT_LATENT_GAUSSIAN) for the row of one chain, as potential_value_grad_row: U and dU/dx
// of LatentGaussPot (above).  The matrices and the table are wave-uniform (scalar loads); blocks of kFullRankJB
// outputs stay in registers over i as in fullrank_value_grad_row.  latent_row_lik is the elementwise part: l'(f_j)
// into grow[j], sum_j l_j(f_j) returned, the likelihood chosen outside the loop.
//   centred:   grow = Lambda (x - m), one sweep; then l'(x) is added.
//   whitened:  a first sweep over the row forms f_j = m_j + sum_{i <= j} L_ji z_i from the rows of L^T and leaves
//              l'(f_j) in grow[j]; a second sweep over grow, held in LDS, forms z_j + sum_{i >= j} L_ij l'_i from the
//              rows of L and overwrites grow block by block in ascending j: block j0 reads entries i >= j0 only, none of
//              them overwritten yet.  Both sweeps skip the triangle of L that is zero by construction.
// Kept out of potential_value_grad_row, which the fit and DLMC kernels share and which never see kind 12.
template <int LIK>
__device__ __forceinline__ float latent_row_lik(const float* __restrict__ f, float* __restrict__ grow, const float* __restrict__ y,
                                                const float* __restrict__ w, float c0, float c1, float c2, int j0, int nj) {
    float s = 0.f;
    for (int k = 0; k < nj; ++k) {
        float l, lp;
        latent_lik<LIK>(f[k], y[j0 + k], w[j0 + k], c0, c1, c2, l, lp);
        grow[j0 + k] = lp;
        s += l;
    }
    return s;
}
__device__ __forceinline__ float latent_row_lik_of(int lik, const float* __restrict__ f, float* __restrict__ grow,
                                                   const float* __restrict__ y, const float* __restrict__ w, float c0, float c1,
                                                   float c2, int j0, int nj) {
    return lik == 0 ? latent_row_lik<0>(f, grow, y, w, c0, c1, c2, j0, nj)
         : lik == 1 ? latent_row_lik<1>(f, grow, y, w, c0, c1, c2, j0, nj)
                    : latent_row_lik<2>(f, grow, y, w, c0, c1, c2, j0, nj);
}
__device__ __forceinline__ float latent_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                       const NfmcPotential& p, int d) {
    constexpr int JB = kFullRankJB;
    int lik = 0;
    bool white = false;
    latent_code(p.a_scalar, lik, white);
    const int d4 = latent_row(d);
    const float c0 = p.b[0], c1 = p.b[1], c2 = p.b[2];
    const float* __restrict__ m = p.b + 8;
    const float* __restrict__ y = m + d4;
    const float* __restrict__ w = y + d4;
    float u = 0.f;
    if (!white) {
        const float* __restrict__ lam = p.a;
        for (int j0 = 0; j0 < d; j0 += JB) {
            const int nj = d - j0 < JB ? d - j0 : JB;
            float acc[JB], f[JB];
#pragma unroll
            for (int k = 0; k < JB; ++k) acc[k] = 0.f;
            for (int i = 0; i < d; ++i) {
                const float ri = row[i] - m[i];
                const float* __restrict__ li = lam + (int64_t)i * d + j0;
#pragma unroll
                for (int k = 0; k < JB; ++k) acc[k] = fmaf(k < nj ? li[k] : 0.f, ri, acc[k]);
            }
#pragma unroll
            for (int k = 0; k < JB; ++k) f[k] = k < nj ? row[j0 + k] : 0.f;
            u += latent_row_lik_of(lik, f, grow, y, w, c0, c1, c2, j0, nj);
#pragma unroll
            for (int k = 0; k < JB; ++k)
                if (k < nj) {
                    u = fmaf(0.5f * (f[k] - m[j0 + k]), acc[k], u);
                    grow[j0 + k] += acc[k];
                }
        }
        return u;
    }
    const float* __restrict__ lt = p.a;                       // rows of L^T
    const float* __restrict__ lo = p.a + (int64_t)d * d;      // rows of L
    for (int j0 = 0; j0 < d; j0 += JB) {
        const int nj = d - j0 < JB ? d - j0 : JB;
        float f[JB];
#pragma unroll
        for (int k = 0; k < JB; ++k) f[k] = k < nj ? m[j0 + k] : 0.f;
        for (int i = 0; i < j0 + nj; ++i) {                   // L^T_ij = 0 for i > j
            const float zi = row[i];
            const float* __restrict__ li = lt + (int64_t)i * d + j0;
#pragma unroll
            for (int k = 0; k < JB; ++k) f[k] = fmaf(k < nj ? li[k] : 0.f, zi, f[k]);
        }
        u += latent_row_lik_of(lik, f, grow, y, w, c0, c1, c2, j0, nj);
    }
    for (int j0 = 0; j0 < d; j0 += JB) {
        const int nj = d - j0 < JB ? d - j0 : JB;
        float acc[JB];
#pragma unroll
        for (int k = 0; k < JB; ++k) acc[k] = 0.f;
        for (int i = j0; i < d; ++i) {                        // L_ij = 0 for i < j
            const float gi = grow[i];
            const float* __restrict__ li = lo + (int64_t)i * d + j0;
#pragma unroll
            for (int k = 0; k < JB; ++k) acc[k] = fmaf(k < nj ? li[k] : 0.f, gi, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < JB; ++k)
            if (k < nj) {
                const float z = row[j0 + k];
                grow[j0 + k] = z + acc[k];
                u = fmaf(0.5f * z, z, u);
            }
    }
    return u;
}

}  // namespace nfmc
