// (kernels and device code of neutra_kernels.hip and its per-rows-per-wave units neutra_kernels_r*.hip)
// K5 + K2: NeuTra -- HMC in the flow's latent space on the adjusted potential
//     U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)|                 (neutra.py:58-68)
// with grad U~ from a hand-written reverse sweep through the coupling stack (the reference gets it from
// torch.autograd through torchflows, hmc.py:40-48), fused with the leapfrog integrator, the Hamiltonian
// test and the statistics (hmc.py:61-77,96-126; mcmc/base.py:74-90).
//
// VALU path (conditioner width <= 32): one chain per lane, four (64, d) wave tiles in LDS
//   zt latent position | pt momentum | wt work (x and the layer inputs re-materialised on the way back) | gt gradient
// Coupling layers are invertible, so the reverse sweep needs no stored activations: the layer input is
// rebuilt from its output (v_b = alpha y_b + beta) and the conditioner's hidden stack is recomputed from
// the pass-through half.  Weights are wave-uniform (scalar loads).
//
// Adjacent leapfrog half-steps evaluate grad U~ at the same z; the value is computed once and reused
// (bitwise what the reference's two evaluations return), counters still report the reference's 2L(+2).
#pragma once

#include "mfma_device.hpp"

namespace nfmc {

constexpr int kMaxHiddenLayers = 4;

// Reverse sweep through one inverse coupling layer.  On entry wrow holds the layer OUTPUT y and grow
// dL/dy; on exit wrow holds the layer INPUT v and grow dL/dv, where L = U(x) + sum_layers sum_t log alpha.
template <int HP>
__device__ __forceinline__ void coupling_inverse_backward(float* __restrict__ wrow, float* __restrict__ grow,
                                                          const float* __restrict__ W, const FlowGeom& g, bool rev) {
    // recompute the hidden stack from the pass-through half, keeping every layer's activations
    float hs[kMaxHiddenLayers][HP];
    const float* b1 = W + (int64_t)g.d_a * HP;
#pragma unroll
    for (int k = 0; k < HP; ++k) hs[0][k] = b1[k];
    for (int j = 0; j < g.d_a; ++j) {
        const float xj = wrow[phys(j, g.d, rev)];
        const float* w = W + (int64_t)j * HP;
#pragma unroll
        for (int k = 0; k < HP; ++k) hs[0][k] = fmaf(w[k], xj, hs[0][k]);
    }
#pragma unroll
    for (int k = 0; k < HP; ++k) hs[0][k] = fast_tanh(hs[0][k]);
    const float* Wh0 = b1 + HP;
#pragma unroll
    for (int l = 1; l < kMaxHiddenLayers; ++l) {
        if (l < g.n_hl) {
            const float* Wh = Wh0 + (int64_t)(l - 1) * (HP * HP + HP);
            const float* bh = Wh + HP * HP;
#pragma unroll
            for (int k = 0; k < HP; ++k) hs[l][k] = bh[k];
#pragma unroll
            for (int i = 0; i < HP; ++i) {
#pragma unroll
                for (int k = 0; k < HP; ++k) hs[l][k] = fmaf(Wh[i * HP + k], hs[l - 1][i], hs[l][k]);
            }
#pragma unroll
            for (int k = 0; k < HP; ++k) hs[l][k] = fast_tanh(hs[l][k]);
        }
    }
    float hl[HP];  // activations of the last hidden layer
#pragma unroll
    for (int k = 0; k < HP; ++k) {
        hl[k] = hs[0][k];
#pragma unroll
        for (int l = 1; l < kMaxHiddenLayers; ++l)
            if (l == g.n_hl - 1) hl[k] = hs[l][k];
    }
    // output layer: transform parameters per target coordinate, their gradients, and dL/dh_last
    const float* W3 = w3_of(W, g, HP);
    const float* b3 = W3 + (int64_t)g.out_rows * HP;
    float dh[HP];
#pragma unroll
    for (int k = 0; k < HP; ++k) dh[k] = 0.f;
    if (g.n_bins > 0) {
        // rational-quadratic spline couplings ('c-rqnsf'): 3K - 1 conditioner outputs per target coordinate
        constexpr int P = 3 * kRqsBins - 1;
        for (int t = 0; t < g.d_b; ++t) {
            float raw[P], draw[P];
            const float* wr = W3 + (int64_t)t * P * HP;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                float u = b3[t * P + q];
#pragma unroll
                for (int k = 0; k < HP; ++k) u = fmaf(wr[q * HP + k], hl[k], u);
                raw[q] = u;
            }
            const int p = phys(g.d_a + t, g.d, rev);
            float v, gv;
            rqs_inverse_backward(wrow[p], grow[p], raw, g.bound, draw, v, gv);
#pragma unroll
            for (int q = 0; q < P; ++q) {
#pragma unroll
                for (int k = 0; k < HP; ++k) dh[k] = fmaf(wr[q * HP + k], draw[q], dh[k]);
            }
            grow[p] = gv;
            wrow[p] = v;                                 // rebuild the layer input
        }
    } else
    for (int t = 0; t < g.d_b; ++t) {
        float ua = b3[t], ub = b3[g.d_b + t];
        const float* wa = W3 + (int64_t)t * HP;
        const float* wb = W3 + (int64_t)(g.d_b + t) * HP;
#pragma unroll
        for (int k = 0; k < HP; ++k) {
            ua = fmaf(wa[k], hl[k], ua);
            ub = fmaf(wb[k], hl[k], ub);
        }
        const float alpha = fast_exp(fmaf(0.5f, ua, g.log1m)) + g.m;
        const float beta = 0.5f * ub;
        const float ra = __builtin_amdgcn_rcpf(alpha);
        const int p = phys(g.d_a + t, g.d, rev);
        const float y = wrow[p];
        const float gy = grow[p];
        const float gv = gy * ra;                        // dL/dv_t
        const float d_alpha = fmaf(-gv, y, ra);          // -gy*y/alpha + 1/alpha (log alpha term of this layer)
        const float d_ua = 0.5f * d_alpha * (alpha - g.m);
        const float d_ub = -0.5f * gv;
#pragma unroll
        for (int k = 0; k < HP; ++k) dh[k] = fmaf(wa[k], d_ua, fmaf(wb[k], d_ub, dh[k]));
        grow[p] = gv;
        wrow[p] = fmaf(alpha, y, beta);                  // rebuild the layer input
    }
    // back through the hidden stack
#pragma unroll
    for (int l = kMaxHiddenLayers - 1; l >= 1; --l) {
        if (l < g.n_hl) {
            const float* Wh = Wh0 + (int64_t)(l - 1) * (HP * HP + HP);
            float dpre[HP], dprev[HP];
#pragma unroll
            for (int k = 0; k < HP; ++k) dpre[k] = dh[k] * (1.f - hs[l][k] * hs[l][k]);
#pragma unroll
            for (int i = 0; i < HP; ++i) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < HP; ++k) acc = fmaf(Wh[i * HP + k], dpre[k], acc);
                dprev[i] = acc;
            }
#pragma unroll
            for (int k = 0; k < HP; ++k) dh[k] = dprev[k];
        }
    }
    float dpre[HP];
#pragma unroll
    for (int k = 0; k < HP; ++k) dpre[k] = dh[k] * (1.f - hs[0][k] * hs[0][k]);
    for (int j = 0; j < g.d_a; ++j) {
        const float* w = W + (int64_t)j * HP;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < HP; ++k) acc = fmaf(w[k], dpre[k], acc);
        grow[phys(j, g.d, rev)] += acc;
    }
}

// Full-rank Gaussian (NFMC_POT_GAUSSIAN_FULL) for the row of one chain, as potential_value_grad_row:
//   U = 1/2 r^T Lambda r,   grow = Lambda r,   r = x - mu
// Lambda and mu are wave-uniform, so the compiler reads them with scalar loads.  A block of kFullRankJB outputs stays in
// registers while the loop runs over i: one LDS read of x_i feeds kFullRankJB FMAs with row i of Lambda (= column i, by
// symmetry).  Kept out of potential_value_grad_row, which the fit and DLMC kernels share and which never see kind 4.
constexpr int kFullRankJB = 8;
__device__ __forceinline__ float fullrank_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                         const NfmcPotential& p, int d) {
    const float* __restrict__ lam = p.a;
    const float* __restrict__ mu = p.b;
    float u = 0.f;
    int j0 = 0;
    for (; j0 + kFullRankJB <= d; j0 += kFullRankJB) {
        float acc[kFullRankJB];
#pragma unroll
        for (int k = 0; k < kFullRankJB; ++k) acc[k] = 0.f;
        for (int i = 0; i < d; ++i) {
            const float ri = row[i] - mu[i];
            const float* __restrict__ li = lam + (int64_t)i * d + j0;
#pragma unroll
            for (int k = 0; k < kFullRankJB; ++k) acc[k] = fmaf(li[k], ri, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < kFullRankJB; ++k) {
            grow[j0 + k] = acc[k];
            u = fmaf(row[j0 + k] - mu[j0 + k], acc[k], u);
        }
    }
    for (; j0 < d; ++j0) {   // the last d % kFullRankJB outputs
        float acc = 0.f;
        for (int i = 0; i < d; ++i) acc = fmaf(lam[(int64_t)i * d + j0], row[i] - mu[i], acc);
        grow[j0] = acc;
        u = fmaf(row[j0] - mu[j0], acc, u);
    }
    return 0.5f * u;
}

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

// Stochastic volatility (NFMC_POT_STOCHASTIC_VOLATILITY) for the row of one chain, as potential_value_grad_row: U and
// dU/dx of SVPot (common.hpp), x_0 = mu, x_1 = log sigma, x_2 = atanh phi, x_{3+t} = h_t.  One pass over h_0 .. h_{T-1}:
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

// Sparse logistic regression (NFMC_POT_SPARSE_LOGISTIC_REGRESSION) for the row of one chain, as potential_value_grad_row:
// U and dU/dx of SparseLogRegPot (common.hpp), x_{2j} = w_j, x_{2j+1} = log lambda_j, x_{2D} = log tau.  The gradient
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

// phi^4 lattice field (NFMC_POT_LATTICE_PHI4) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// Phi4Pot (common.hpp), H = d / W rows of W = n_components sites.  A plain loop over the sites with index arithmetic for
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

// Item-response theory (NFMC_POT_ITEM_RESPONSE) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// IrtPot (common.hpp), x = [alpha (S) | beta (Q) | mu].  One pass over the questions: the students' entries of the
// gradient row accumulate r_sq = sigmoid(l_sq) - y_sq, question q's entry gets -sum_s r_sq when its row is done, and the
// sum of those is mu's.  The responses are wave-uniform (scalar loads); a negative entry is a missing answer.  The data
// term is summed in fp64, as in IrtPot.  grow[s] += r is a read and a write of the lane's own LDS row per pair, beside
// the exp, log and reciprocal of softplus_sigmoid: the price of evaluating every pair once with the responses read in
// storage order (a second pass for the students' sums would evaluate every pair twice, student-major blocks would
// read each 64-byte line of the responses in four far-apart visits).  Kept out of potential_value_grad_row, which the fit and DLMC kernels share and
// which never see kind 9.
__device__ __forceinline__ float irt_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                    const NfmcPotential& p, int d) {
    const int ns = p.n_components, nq = d - 1 - ns, sa = (ns + 3) & ~3;
    const float m0 = p.b[0], pmu = p.b[1], pa = p.b[2], pb = p.b[3], mu = row[d - 1];
    float u = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float a = row[s];
        grow[s] = pa * a;
        u = fmaf(0.5f * pa * a, a, u);
    }
    double ul = 0.0;
    float sr = 0.f;
    for (int q = 0; q < nq; ++q) {
        const float* __restrict__ aq = p.a + (int64_t)q * sa;
        const float beta = row[ns + q];
        float rs = 0.f;
        for (int s = 0; s < ns; ++s) {
            const float v = aq[s];
            if (v >= 0.f) {   // wave-uniform
                const float l = (mu + row[s]) - beta;
                float sp, sg;
                softplus_sigmoid(l, sp, sg);
                const float r = sg - v;
                grow[s] += r;
                rs += r;
                ul += (double)(sp - v * l);
            }
        }
        grow[ns + q] = fmaf(pb, beta, -rs);
        u = fmaf(0.5f * pb * beta, beta, u);
        sr += rs;
    }
    const float dm = mu - m0;
    grow[d - 1] = fmaf(pmu, dm, sr);
    return (float)(ul + (double)fmaf(0.5f * pmu * dm, dm, u));
}

// Varying-effects regression (NFMC_POT_VARYING_EFFECTS) for the row of one chain, as potential_value_grad_row: U and
// dU/dx of VaryEffPot (common.hpp), the group block first and the globals behind it.  One pass over the groups: the
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

// Interacting particles (NFMC_POT_PARTICLES) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// ParticlePot (common.hpp), P = n_components particles of D = d / P coordinates each, particle-major.  A double loop:
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

// Latent Gaussian model (NFMC_POT_LATENT_GAUSSIAN) for the row of one chain, as potential_value_grad_row: U and dU/dx
// of LatentGaussPot (common.hpp).  The matrices and the table are wave-uniform (scalar loads); blocks of kFullRankJB
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

// Latent Gaussian Markov random field (NFMC_POT_LATENT_GMRF) for the row of one chain, as potential_value_grad_row: U and
// dU/dx of GmrfPot (common.hpp), the sites first and s = log tau behind them when tau is unknown.  The row is
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

// Diffusion bridge (NFMC_POT_DIFFUSION_BRIDGE) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// DiffusionPot (common.hpp), the path time-major and p = log sigma, q = log tau behind it when the scales are unknown.
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

// U~(z) and grad U~(z) for this lane's chain.  zrow: latent (tile columns in latent order), read only;
// wrow: scratch, ends holding z again (rebuilt); grow: gradient in the same column order as zrow.
template <int HP>
__device__ __forceinline__ float adjusted_potential_grad_row(const float* __restrict__ zrow, float* __restrict__ wrow,
                                                             float* __restrict__ grow, const NfmcRealNVP& f,
                                                             const FlowGeom& g, const NfmcPotential& pot) {
    for (int c = 0; c < g.d; ++c) wrow[c] = zrow[c];
    const float ld = flow_inverse_row<HP>(wrow, f, g);          // w = x, ld = logdet_inverse (neutra.py:60)
    const float u = pot.kind == NFMC_POT_GAUSSIAN_FULL ? fullrank_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_ROSENBROCK    ? rosenbrock_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_STOCHASTIC_VOLATILITY ? sv_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_SPARSE_LOGISTIC_REGRESSION ? slr_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_LATTICE_PHI4 ? phi4_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_ITEM_RESPONSE ? irt_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_VARYING_EFFECTS ? vfx_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_PARTICLES ? particles_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_LATENT_GAUSSIAN ? latent_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_LATENT_GMRF ? gmrf_value_grad_row(wrow, grow, pot, g.d)
                    : pot.kind == NFMC_POT_DIFFUSION_BRIDGE ? diffusion_value_grad_row(wrow, grow, pot, g.d)
                                                         : potential_value_grad_row(wrow, grow, pot, g.d);  // U(x), dU/dx (neutra.py:62)
    // reverse sweep, mirror image of flow_inverse_row
    for (int c = 0; c < g.d; ++c) {                               // EA0^-1
        const float s = fast_exp(-f.ea0_log_scale[c]);
        grow[c] *= s;
    }
    for (int c = 0; c < g.d; ++c) wrow[c] = fmaf(fast_exp(f.ea0_log_scale[c]), wrow[c], f.ea0_shift[c]);
    for (int l = 0; l < g.n_coupling; ++l)
        coupling_inverse_backward<HP>(wrow, grow, f.weights + l * g.layer_stride, g, (l & 1) == 0);
    const bool rev_last = (g.n_coupling & 1) != 0;
    for (int c = 0; c < g.d; ++c) {                               // EA1^-1
        const int p = phys(c, g.d, rev_last);
        grow[p] *= fast_exp(-f.ea1_log_scale[c]);
    }
    return u - ld;                                                // neutra.py:63-64
}

constexpr int kNeutraBlock = 64;
constexpr int kNeutraSlots = 8;

// Rows (chains) per wave.  The kernels keep 3 (gradient) or 4 (trajectory) tiles of RPW x d floats in LDS; at 64 rows they fit
// the CU's 160 KB up to d ~ 156 / 208, and until round 3 wider events sent NeuTra to torch autograd on the GPU.  With 32 or 16
// rows per wave (the other lanes idle in the per-row phases, all 64 lanes still share the column phases: tile IO, statistics)
// every d <= 512 has a kernel.
static int neutra_rows_per_wave(int d, int tiles_of_d) {
    for (int rpw = 64; rpw >= 16; rpw >>= 1)
        if ((size_t)tiles_of_d * rpw * tile_stride(d) * sizeof(float) <= 150 * 1024) return rpw;
    return 0;
}
template <int RPW>
__device__ __forceinline__ void tile_load_rows(float* __restrict__ tile, int stride, const float* __restrict__ src, int64_t r0,
                                               int64_t n, int d, bool rev) {
    const int lane = threadIdx.x & 63;
    const int64_t rows = n - r0 < RPW ? n - r0 : RPW;
    const int total = (int)rows * d;
    const float* s = src + r0 * d;
    for (int i = lane; i < RPW * d; i += kWave) {
        const int r = i / d, c = i - r * d;
        tile[r * stride + (rev ? d - 1 - c : c)] = i < total ? s[i] : 0.f;  // rows beyond n: zeros
    }
}
template <int RPW>
__device__ __forceinline__ void tile_store_rows(const float* __restrict__ tile, int stride, float* __restrict__ dst, int64_t r0,
                                                int64_t n, int d, bool rev) {
    const int lane = threadIdx.x & 63;
    const int64_t rows = n - r0 < RPW ? n - r0 : RPW;
    const int total = (int)rows * d;
    float* o = dst + r0 * d;
    for (int i = lane; i < total; i += kWave) {
        const int r = i / d, c = i - r * d;
        o[i] = tile[r * stride + (rev ? d - 1 - c : c)];
    }
}

template <int HP, int RPW>
__global__ void __launch_bounds__(kNeutraBlock) neutra_potential_grad_kernel(NfmcRealNVP f, NfmcPotential pot,
                                                                             const float* __restrict__ z, int64_t n,
                                                                             float* __restrict__ u_out,
                                                                             float* __restrict__ grad_out,
                                                                             int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FlowGeom g = make_geom(f);
    const int stride = tile_stride(g.d);
    const int lane = threadIdx.x;
    float* zt = lds;
    float* wt = lds + RPW * stride;
    float* gt = lds + 2 * RPW * stride;
    const bool rev = (g.n_coupling & 1) != 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * RPW;
        __syncthreads();
        tile_load_rows<RPW>(zt, stride, z, r0, n, g.d, rev);
        __syncthreads();
        if (lane < RPW) {
            const float u = adjusted_potential_grad_row<HP>(zt + lane * stride, wt + lane * stride, gt + lane * stride, f,
                                                            g, pot);
            if (r0 + lane < n && u_out) u_out[r0 + lane] = u;
        }
        __syncthreads();
        if (grad_out) tile_store_rows<RPW>(gt, stride, grad_out, r0, n, g.d, rev);
    }
}

template <int HP, int RPW>
__global__ void __launch_bounds__(kNeutraBlock) neutra_hmc_kernel(NfmcNeutraHmcArgs a, int64_t tiles, int dp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const NfmcRealNVP& f = a.flow;
    const FlowGeom g = make_geom(f);
    const int d = g.d;
    const int stride = tile_stride(d);
    const int lane = threadIdx.x;
    float* zt = lds;
    float* pt = lds + RPW * stride;
    float* wt = lds + 2 * RPW * stride;
    float* gt = lds + 3 * RPW * stride;
    const bool rowlane = lane < RPW;   // lanes that own a chain (all 64 lanes share the column phases)
    float* zr = zt + lane * stride;
    float* pr = pt + lane * stride;
    float* wr = wt + lane * stride;
    float* gr = gt + lane * stride;
    const int64_t n = a.n;
    const bool rev = (g.n_coupling & 1) != 0;
    const float h = a.step_size, hh = a.step_size / 2;

    double sx[kNeutraSlots], sxx[kNeutraSlots];
#pragma unroll
    for (int k = 0; k < kNeutraSlots; ++k) sx[k] = sxx[k] = 0.0;
    uint32_t n_acc = 0, n_bad = 0;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * RPW;
        const int64_t row = r0 + lane;
        const bool active = rowlane && row < n;
        const int rows = (int)(n - r0 < RPW ? n - r0 : RPW);
        const uint32_t gchain = (uint32_t)(a.rng.chain_offset + (uint64_t)row);
        __syncthreads();
        tile_load_rows<RPW>(zt, stride, a.z, r0, n, d, rev);
        __syncthreads();
        float u_cur = rowlane ? adjusted_potential_grad_row<HP>(zr, wr, gr, f, g, a.pot) : 0.f;  // U~(z), grad at the current state
        uint4 ur = make_uint4(0, 0, 0, 0);
        StoreCursor keep(a.samples);
        for (int s = 0; s < a.n_steps; ++s) {
            bool accept = false;
            float lr = 0.f;
            if (rowlane) {
            // momentum p = eps / sqrt(m)  (hmc.py:100); tile columns are latent positions: logical c <-> col latent_col(c)
            float kin0 = 0.f;
            if (a.rng.replay_normals) {
                const float* src = a.rng.replay_normals + ((int64_t)s * n + row) * d;
                for (int c = 0; c < d; ++c) {
                    const float m = a.inv_mass_diag ? a.inv_mass_diag[c] : 1.f;
                    const float v = (active ? src[c] : 0.f) * (1.f / sqrtf(m));
                    pr[latent_col(c, g)] = v;
                    kin0 = fmaf(v * v, m, kin0);
                }
            } else {
                const uint32_t k0 = (uint32_t)a.rng.seed, k1 = (uint32_t)(a.rng.seed >> 32);
                for (int b = 0; b < (d + 3) / 4; ++b) {
                    float zz[4];
                    philox_normal4(gchain, a.rng.step0 + (uint32_t)s, (uint32_t)b, kTagNoise, k0, k1, zz);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = 4 * b + k;
                        if (c < d) {
                            const float m = a.inv_mass_diag ? a.inv_mass_diag[c] : 1.f;
                            const float v = zz[k] * (1.f / sqrtf(m));
                            pr[latent_col(c, g)] = v;
                            kin0 = fmaf(v * v, m, kin0);
                        }
                    }
                }
            }
            const float h0 = u_cur + 0.5f * kin0;                      // hmc.py:103-106
            float u_new = u_cur;
            // gr holds grad U~(z) here (from the previous trajectory's last evaluation or the tile prologue);
            // a rejected trajectory restores it below by re-evaluating at the restored z.
            for (int l = 0; l < a.n_leapfrog; ++l) {                    // hmc.py:67-71
                for (int c = 0; c < d; ++c) {
                    const int col = latent_col(c, g);
                    const float m = a.inv_mass_diag ? a.inv_mass_diag[c] : 1.f;
                    const float pv = fmaf(-hh, gr[col], pr[col]);
                    pr[col] = pv;
                    zr[col] = fmaf(h, pv * m, zr[col]);
                }
                u_new = adjusted_potential_grad_row<HP>(zr, wr, gr, f, g, a.pot);
                for (int c = 0; c < d; ++c) pr[c] = fmaf(-hh, gr[c], pr[c]);
            }
            accept = true;
            if (a.adjust) {
                float kin1 = 0.f;
                for (int c = 0; c < d; ++c) {
                    const float m = a.inv_mass_diag ? a.inv_mass_diag[c] : 1.f;
                    const float v = pr[latent_col(c, g)];
                    kin1 = fmaf(v * v, m, kin1);
                }
                lr = h0 - (u_new + 0.5f * kin1);                       // hmc.py:107-111
                float u;
                if (a.rng.replay_uniforms) {
                    u = active ? a.rng.replay_uniforms[(int64_t)s * n + row] : 0.5f;
                } else {
                    const uint32_t step = a.rng.step0 + (uint32_t)s;
                    if (s == 0 || (step & 3u) == 0u)
                        ur = philox4x32_10(gchain, step >> 2, 0u, kTagAccept, (uint32_t)a.rng.seed,
                                           (uint32_t)(a.rng.seed >> 32));
                    u = u32_to_uniform(pick_word(ur, step & 3u));
                }
                accept = fast_ln(u) < lr;                               // hmc.py:112-113
                if (active && !(fabsf(lr) <= 3.0e38f)) n_bad++;
            }
            accept = accept && active;
            if (accept) {
                u_cur = u_new;
                n_acc++;
            } else {
                // restore the trajectory's start point from HBM (the tile is only written back on accept)
                for (int c = 0; c < d; ++c) zr[latent_col(c, g)] = active ? a.z[row * d + c] : 0.f;
            }
            }   // rowlane
            __syncthreads();
            // write accepted rows back so HBM always holds the current state (row-contiguous stores)
            if (accept)
                for (int c = 0; c < d; ++c) a.z[row * d + c] = zr[latent_col(c, g)];
            if (rowlane && !accept && s + 1 < a.n_steps) u_cur = adjusted_potential_grad_row<HP>(zr, wr, gr, f, g, a.pot);
            if (active) {
                if (a.masks_out) a.masks_out[(int64_t)s * n + row] = accept ? 1 : 0;
                if (a.log_ratio_out) a.log_ratio_out[(int64_t)s * n + row] = lr;
            }
            __syncthreads();
            if (a.stats.sum_x) {  // moments of the latent state (reference quirk: SURVEY App. C #1)
#pragma unroll
                for (int k = 0; k < kNeutraSlots; ++k) {
                    const int c = lane + 64 * k;
                    if (c < d) {
                        const int col = latent_col(c, g);
                        float t1 = 0.f, t2 = 0.f;
                        for (int r = 0; r < rows; ++r) {
                            const float v = zt[r * stride + col];
                            t1 += v;
                            t2 = fmaf(v, v, t2);
                        }
                        sx[k] += (double)t1;
                        sxx[k] += (double)t2;
                    }
                }
            }
            if (float* kept = keep.next(n * (int64_t)d)) tile_store_rows<RPW>(zt, stride, kept, r0, n, d, rev);
            __syncthreads();
        }
    }
    if (a.stats.sum_x) {
        for (int m = 1; m < kWave; m <<= 1) {
            n_acc += __shfl_xor(n_acc, m, kWave);
            n_bad += __shfl_xor(n_bad, m, kWave);
        }
        double* out = a.stats.scratch + (size_t)blockIdx.x * (2 * dp + kStatTail);
        for (int c = lane; c < 2 * dp + kStatTail; c += kWave) out[c] = 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kNeutraSlots; ++k) {
            const int c = lane + 64 * k;
            if (c < d) {
                out[c] = sx[k];
                out[dp + c] = sxx[k];
            }
        }
        if (lane == 0) {
            out[2 * dp] = (double)n_acc;
            out[2 * dp + 1] = (double)n_bad;
        }
    }
}

static int check_flow_neutra(const NfmcRealNVP* f) {
    if (!f || !f->ea0_log_scale || !f->ea0_shift || !f->ea1_log_scale || !f->ea1_shift) return NFMC_EINVAL;
    if (f->d <= 0 || f->n_coupling < 0 || f->n_hidden <= 0 || f->n_hidden_layers <= 0) return NFMC_EINVAL;
    if (f->n_coupling > 0 && !f->weights) return NFMC_EINVAL;
    if (f->d < 2 && f->n_coupling > 0) return NFMC_ESHAPE;
    if (f->d > 512) return NFMC_ESHAPE;
    if (f->n_hidden_layers > kMaxHiddenLayers) return NFMC_ESHAPE;
    if (f->n_hidden > 32 || (f->n_bins != 0 && f->n_bins != kRqsBins)) return NFMC_EUNSUPPORTED;
    if (f->n_coupling > 0 && f->layer_stride < nfmc_coupling_layer_floats(f->d, f->n_hidden, f->n_hidden_layers, f->n_bins))
        return NFMC_EINVAL;
    return NFMC_OK;
}

static int hp_bucket_n(int h) { return h <= 4 ? 4 : (h <= 8 ? 8 : (h <= 16 ? 16 : 32)); }

template <class K>
static int set_lds_n(K kernel, size_t bytes) {
    if (bytes > 160 * 1024) return NFMC_ESHAPE;
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// The kernels are instantiated per rows-per-wave variant in a unit of its own (neutra_kernels_r64 / r32 / r16.hip: together
// they were 222 s of compile time in one unit, the critical path of the build); the C entry points in neutra_kernels.hip
// call these launchers.  hp: conditioner width bucket (hp_bucket_n).  Return 0 or an error code.
#define NFMC_NEUTRA_RPW_DECL(RPWV)                                                                                              \
    int neutra_grad_launch_r##RPWV(int hp, size_t lds, int grid, hipStream_t st, const NfmcRealNVP& f, const NfmcPotential& pot, \
                                  const float* z, int64_t n, float* u_out, float* grad_out, int64_t tiles);                      \
    int neutra_hmc_launch_r##RPWV(int hp, size_t lds, int grid, hipStream_t st, const NfmcNeutraHmcArgs& a, int64_t tiles, int dp);
NFMC_NEUTRA_RPW_DECL(64)
NFMC_NEUTRA_RPW_DECL(32)
NFMC_NEUTRA_RPW_DECL(16)

#define NFMC_NEUTRA_HP_SWITCH(CALL)                             \
    if (hp == 4) { constexpr int HP = 4; CALL; }                \
    else if (hp == 8) { constexpr int HP = 8; CALL; }           \
    else if (hp == 16) { constexpr int HP = 16; CALL; }         \
    else if (hp == 32) { constexpr int HP = 32; CALL; }         \
    else return NFMC_EUNSUPPORTED;

#define NFMC_NEUTRA_RPW_UNIT(RPWV)                                                                                              \
    namespace nfmc {                                                                                                            \
    int neutra_grad_launch_r##RPWV(int hp, size_t lds, int grid, hipStream_t st, const NfmcRealNVP& f, const NfmcPotential& pot, \
                                  const float* z, int64_t n, float* u_out, float* grad_out, int64_t tiles) {                     \
        int rc = 0;                                                                                                             \
        NFMC_NEUTRA_HP_SWITCH({                                                                                                 \
            if ((rc = set_lds_n(neutra_potential_grad_kernel<HP, RPWV>, lds))) return rc;                                       \
            hipLaunchKernelGGL((neutra_potential_grad_kernel<HP, RPWV>), dim3(grid), dim3(kNeutraBlock), lds, st, f, pot, z, n,  \
                               u_out, grad_out, tiles);                                                                         \
        })                                                                                                                      \
        return 0;                                                                                                               \
    }                                                                                                                           \
    int neutra_hmc_launch_r##RPWV(int hp, size_t lds, int grid, hipStream_t st, const NfmcNeutraHmcArgs& a, int64_t tiles, int dp) { \
        int rc = 0;                                                                                                             \
        NFMC_NEUTRA_HP_SWITCH({                                                                                                 \
            if ((rc = set_lds_n(neutra_hmc_kernel<HP, RPWV>, lds))) return rc;                                                  \
            hipLaunchKernelGGL((neutra_hmc_kernel<HP, RPWV>), dim3(grid), dim3(kNeutraBlock), lds, st, a, tiles, dp);           \
        })                                                                                                                      \
        return 0;                                                                                                               \
    }                                                                                                                           \
    }

}  // namespace nfmc
