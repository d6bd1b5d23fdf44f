// (device code of the NeuTra-MH kernel; included at the end of neutra_kernels.hpp, instantiated in neutra_kernels_r*.hip)
// Random-walk Metropolis in the flow's latent space on the adjusted potential
//     U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)|                 (neutra.py:58-68,147-159; mh.py:44-73)
// One flow inverse and one potential value per transition: no gradient, so no reverse sweep.  Layout and launch
// geometry are neutra_hmc_kernel's: one chain per lane, four (RPW, d) wave tiles in LDS
//   zt latent state | pt proposal | wt work (x = f^-1 of the row under evaluation) | gt gradient of the own-unit kinds, unused
// The own-unit kinds have no value-only row form; their *_value_grad_row writes its gradient to gt and it is dropped.
//
// A non-finite log ratio always rejects (and counts as non-finite).  mh.py and neutra_hmc_kernel take `log u < lr` as it
// stands, which accepts a ratio of +inf; here a chain whose own U~ is +inf or NaN therefore never moves, where the
// reference would let it go anywhere.  Such a start is reported by the counter and is not one to sample from.
#pragma once

#include "neutra_kernels.hpp"

namespace nfmc {

// U~(z) for this lane's chain, value only.  zrow: latent (tile columns in latent order), read only; wrow: scratch, ends
// holding x = f^-1(z); grow: scratch for the kinds whose row form also writes dU/dx.
template <int HP>
__device__ __forceinline__ float adjusted_potential_row(const float* __restrict__ zrow, float* __restrict__ wrow,
                                                        float* __restrict__ grow, const NfmcRealNVP& f, const FlowGeom& g,
                                                        const NfmcPotential& pot) {
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
                                                         : potential_row(wrow, pot, g.d);   // kinds 0 and 1: U(x) alone (neutra.py:62)
    return u - ld;                                                // neutra.py:63-64
}

template <int HP, int RPW>
__global__ void __launch_bounds__(kNeutraBlock) neutra_mh_kernel(NfmcNeutraMhArgs a, int64_t tiles, int dp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const NfmcRealNVP& f = a.flow;
    const FlowGeom g = make_geom(f);
    const int d = g.d;
    const int stride = tile_stride(d);
    const int lane = threadIdx.x;
    float* zt = lds;
    const bool rowlane = lane < RPW;   // lanes that own a chain (all 64 lanes share the column phases)
    float* zr = zt + lane * stride;
    float* pr = lds + RPW * stride + lane * stride;
    float* wr = lds + 2 * RPW * stride + lane * stride;
    float* gr = lds + 3 * RPW * stride + lane * stride;
    const int64_t n = a.n;
    const bool rev = (g.n_coupling & 1) != 0;

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
        float u_cur = 0.f;
        uint4 ur = make_uint4(0, 0, 0, 0);
        StoreCursor keep(a.samples);
        // s = -1 (adjusted runs only) evaluates U~ at the tile's state; every s >= 0 is one transition.  One loop, so that
        // the kernel holds the flow inverse and the thirteen potential forms once.
        for (int s = a.adjust ? -1 : 0; s < a.n_steps; ++s) {
            bool accept = false;
            float lr = 0.f;
            if (rowlane) {
                if (s >= 0) {
                    // z' = z + eps * inv_mass_diag, the diagonal itself and a separate multiply and add (mh.py:50-55);
                    // tile columns are latent positions: logical c <-> col latent_col(c)
                    if (a.rng.replay_normals) {
                        const float* src = a.rng.replay_normals + ((int64_t)s * n + row) * d;
                        for (int c = 0; c < d; ++c) {
                            const float m = a.inv_mass_diag ? a.inv_mass_diag[c] : 1.f;
                            const int col = latent_col(c, g);
                            pr[col] = __fadd_rn(zr[col], __fmul_rn(active ? src[c] : 0.f, m));
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
                                    const int col = latent_col(c, g);
                                    pr[col] = __fadd_rn(zr[col], __fmul_rn(zz[k], m));
                                }
                            }
                        }
                    }
                }
                float u_new = 0.f;
                if (a.adjust) u_new = adjusted_potential_row<HP>(s < 0 ? zr : pr, wr, gr, f, g, a.pot);
                if (s < 0) {
                    u_cur = u_new;
                } else {
                    accept = true;
                    if (a.adjust) {
                        lr = u_cur - u_new;                                     // mh.py:58
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
                        const bool finite = fabsf(lr) <= 3.0e38f;
                        accept = finite && fast_ln(u) < lr;                     // mh.py:59-60; a non-finite ratio rejects
                        if (active && !finite) n_bad++;
                    }
                    accept = accept && active;
                    if (accept) {
                        // the proposal becomes the tile's row and the state in HBM; a rejected one leaves both as they are
                        u_cur = u_new;
                        n_acc++;
                        for (int c = 0; c < d; ++c) {
                            const int col = latent_col(c, g);
                            const float v = pr[col];
                            zr[col] = v;
                            a.z[row * d + c] = v;
                        }
                    }
                    if (active) {
                        if (a.masks_out) a.masks_out[(int64_t)s * n + row] = accept ? 1 : 0;
                        if (a.log_ratio_out) a.log_ratio_out[(int64_t)s * n + row] = lr;
                    }
                }
            }   // rowlane
            if (s < 0) continue;
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

}  // namespace nfmc
