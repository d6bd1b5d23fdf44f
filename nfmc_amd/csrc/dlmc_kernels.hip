// DLMC (nfmc/algorithms/sampling/nfmc/dlmc.py): the input gradient of the flow's log-density, grad_x log q(x), and the
// fused gradient step of the sampler, x <- x - eps (grad U(x) + grad_x log q(x))   (dlmc.py:85-87).
//
// The reference gets the gradient from torch.autograd through torchflows (`compute_grad`, dlmc.py:85).  Here it is a
// hand-written reverse sweep through the FORWARD map x -> z of the register-layout flows (affine / additive couplings,
// conditioner width <= 8, d <= 512), in the sampler layout of the NeuTra gradient kernel (neutra_kernels.hpp): one chain
// per lane, three (RPW, d) wave tiles in LDS -- x (read only), w (the layer state: z after the forward pass, rebuilt back
// to x by the sweep) and g (the gradient).  Coupling layers are invertible, so nothing is stored between the passes: the
// sweep rebuilds every layer's input from its output, v_b = (y_b - beta) / alpha, and re-evaluates the conditioner from
// the unchanged half.
//
//   log q(x) = -|z|^2 / 2 - d log(2 pi) / 2 + sum(ea0 log_scale) + sum_layers sum_t log alpha_t + sum(ea1 log_scale)
//   dL/dz = -z;  per coupling (y_b = alpha v_b + beta):  dL/dv_b = alpha dL/dy_b,
//                dL/dalpha = dL/dy_b v_b + 1/alpha,  dL/dbeta = dL/dy_b,  then back through the conditioner to v_a.
#include "neutra_kernels.hpp"

using namespace nfmc;

namespace {

// Reverse sweep through one FORWARD coupling layer.  On entry wrow holds the layer OUTPUT y and grow dL/dy; on exit
// wrow holds the layer INPUT v and grow dL/dv, L = log q.
template <int HP>
__device__ __forceinline__ void coupling_forward_backward(float* __restrict__ wrow, float* __restrict__ grow,
                                                          const float* __restrict__ W, const FlowGeom& g, bool rev) {
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
    float hl[HP];
#pragma unroll
    for (int k = 0; k < HP; ++k) {
        hl[k] = hs[0][k];
#pragma unroll
        for (int l = 1; l < kMaxHiddenLayers; ++l)
            if (l == g.n_hl - 1) hl[k] = hs[l][k];
    }
    const float* W3 = w3_of(W, g, HP);
    const float* b3 = W3 + (int64_t)g.out_rows * HP;
    float dh[HP];
#pragma unroll
    for (int k = 0; k < HP; ++k) dh[k] = 0.f;
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
        const float gy = grow[p];
        const float v = (wrow[p] - beta) * ra;           // rebuild the layer input
        const float d_alpha = fmaf(gy, v, ra);           // dL/dy v + 1/alpha (the layer's log alpha term)
        const float d_ua = 0.5f * d_alpha * (alpha - g.m);
        const float d_ub = 0.5f * gy;
#pragma unroll
        for (int k = 0; k < HP; ++k) dh[k] = fmaf(wa[k], d_ua, fmaf(wb[k], d_ub, dh[k]));
        grow[p] = gy * alpha;
        wrow[p] = v;
    }
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

// log q(x) and grad_x log q(x) of this lane's chain.  xrow: x in x order (read only); wrow: scratch; grow: the gradient,
// in x order.
template <int HP>
__device__ __forceinline__ float flow_logq_grad_row(const float* __restrict__ xrow, float* __restrict__ wrow,
                                                    float* __restrict__ grow, const NfmcRealNVP& f, const FlowGeom& g) {
    for (int c = 0; c < g.d; ++c) wrow[c] = xrow[c];
    const float ld = flow_forward_row<HP>(wrow, f, g);           // w = z (latent tile order), ld = logdet_forward
    float zz = 0.f;
    for (int c = 0; c < g.d; ++c) {
        const float z = wrow[c];
        zz = fmaf(z, z, zz);
        grow[c] = -z;                                             // d/dz of the standard normal's log-density
    }
    const bool rev_last = (g.n_coupling & 1) != 0;
    for (int c = 0; c < g.d; ++c) {                               // EA1: z = e^s v + shift
        const int p = phys(c, g.d, rev_last);
        const float ls = f.ea1_log_scale[c];
        wrow[p] = (wrow[p] - f.ea1_shift[c]) * fast_exp(-ls);
        grow[p] *= fast_exp(ls);
    }
    for (int l = g.n_coupling - 1; l >= 0; --l)
        coupling_forward_backward<HP>(wrow, grow, f.weights + l * g.layer_stride, g, (l & 1) == 0);
    for (int c = 0; c < g.d; ++c) grow[c] *= fast_exp(f.ea0_log_scale[c]);   // EA0
    return fmaf(-0.5f, zz, -0.5f * (float)g.d * kLog2Pi) + ld;
}

constexpr int kDlmcBlock = 64;

// MODE 0: grad_x log q (and log q) of every row.  MODE 1: the fused DLMC step on x in place.
template <int HP, int RPW, int MODE>
__global__ void __launch_bounds__(kDlmcBlock) dlmc_kernel(NfmcRealNVP f, NfmcPotential pot, const float* __restrict__ x_in,
                                                          float* __restrict__ x_io, const float* __restrict__ grad_u,
                                                          int64_t n, float step_size, float* __restrict__ grad_out,
                                                          float* __restrict__ logq_out, int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FlowGeom g = make_geom(f);
    const int d = g.d;
    const int stride = tile_stride(d);
    const int lane = threadIdx.x;
    float* xt = lds;
    float* wt = lds + RPW * stride;
    float* gt = lds + 2 * RPW * stride;
    const float* src = MODE == 0 ? x_in : x_io;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * RPW;
        const int64_t row = r0 + lane;
        __syncthreads();
        tile_load_rows<RPW>(xt, stride, src, r0, n, d, false);
        __syncthreads();
        if (lane < RPW) {
            float* xr = xt + lane * stride;
            float* wr = wt + lane * stride;
            float* gr = gt + lane * stride;
            const float lq = flow_logq_grad_row<HP>(xr, wr, gr, f, g);
            if (row < n && logq_out) logq_out[row] = lq;
            if (MODE == 1) {
                if (grad_u) {
                    const float* gu = grad_u + row * d;
                    for (int c = 0; c < d; ++c) wr[c] = row < n ? gu[c] : 0.f;
                } else {
                    potential_value_grad_row(xr, wr, pot, d);
                }
                for (int c = 0; c < d; ++c) xr[c] = fmaf(-step_size, wr[c] + gr[c], xr[c]);
            }
        }
        __syncthreads();
        if (MODE == 0) {
            if (grad_out) tile_store_rows<RPW>(gt, stride, grad_out, r0, n, d, false);
        } else {
            tile_store_rows<RPW>(xt, stride, x_io, r0, n, d, false);
        }
    }
}

template <int MODE>
int dlmc_launch(const NfmcRealNVP& f, const NfmcPotential& pot, const float* x_in, float* x_io, const float* grad_u,
                int64_t n, float step_size, float* grad_out, float* logq_out, hipStream_t st) {
    const int rpw = neutra_rows_per_wave(f.d, 3);
    if (!rpw) return NFMC_ESHAPE;
    const int64_t tiles = (n + rpw - 1) / rpw;
    const int grid = (int)(tiles < 4 * kMaxGrid ? tiles : 4 * kMaxGrid);
    const size_t lds = (size_t)3 * rpw * tile_stride(f.d) * sizeof(float);
    const int hp = hp_bucket_n(f.n_hidden);
#define NFMC_DLMC_LAUNCH(HPV, RPWV)                                                                                       \
    do {                                                                                                                  \
        int rc = set_lds_n(dlmc_kernel<HPV, RPWV, MODE>, lds);                                                            \
        if (rc) return rc;                                                                                                \
        hipLaunchKernelGGL((dlmc_kernel<HPV, RPWV, MODE>), dim3(grid), dim3(kDlmcBlock), lds, st, f, pot, x_in, x_io,     \
                           grad_u, n, step_size, grad_out, logq_out, tiles);                                              \
    } while (0)
    if (hp == 4) {
        if (rpw == 64) NFMC_DLMC_LAUNCH(4, 64);
        else if (rpw == 32) NFMC_DLMC_LAUNCH(4, 32);
        else NFMC_DLMC_LAUNCH(4, 16);
    } else {
        if (rpw == 64) NFMC_DLMC_LAUNCH(8, 64);
        else if (rpw == 32) NFMC_DLMC_LAUNCH(8, 32);
        else NFMC_DLMC_LAUNCH(8, 16);
    }
#undef NFMC_DLMC_LAUNCH
    NFMC_HIP_CHECK_LAUNCH();
    return NFMC_OK;
}

// the register-layout flows this unit has kernels for: affine / additive couplings, conditioner width <= 8, d <= 512
int check_flow_dlmc(const NfmcRealNVP& f) {
    int rc = check_flow_neutra(&f);
    if (rc) return rc;
    if (f.n_bins != 0 || f.n_hidden > 8) return NFMC_EUNSUPPORTED;
    if (!neutra_rows_per_wave(f.d, 3)) return NFMC_ESHAPE;
    return NFMC_OK;
}

int check_logq_grad(const NfmcFlowLogqGradArgs* a) {
    if (!a) return NFMC_EINVAL;
    if (int rc = check_flow_dlmc(a->flow)) return rc;
    if (!a->x || a->n <= 0 || (!a->grad_out && !a->logq_out)) return NFMC_EINVAL;
    return NFMC_OK;
}

int check_dlmc_step(const NfmcDlmcStepArgs* a) {
    if (!a) return NFMC_EINVAL;
    if (int rc = check_flow_dlmc(a->flow)) return rc;
    if (!a->x || a->n <= 0 || !(a->step_size >= 0.f) || !(a->step_size <= 3.0e38f)) return NFMC_EINVAL;
    if (!a->grad_u && a->pot.kind != NFMC_POT_QUADRATIC && a->pot.kind != NFMC_POT_FUNNEL) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

}  // namespace

extern "C" int nfmc_flow_logq_grad_supported_f32(const NfmcFlowLogqGradArgs* args) { return check_logq_grad(args); }

extern "C" int nfmc_flow_logq_grad_f32(const NfmcFlowLogqGradArgs* args, nfmc_stream_t stream) {
    if (int rc = check_logq_grad(args)) return rc;
    NfmcPotential none{};
    return dlmc_launch<0>(args->flow, none, args->x, nullptr, nullptr, args->n, 0.f, args->grad_out, args->logq_out,
                          (hipStream_t)stream);
}

extern "C" int nfmc_dlmc_step_supported_f32(const NfmcDlmcStepArgs* args) { return check_dlmc_step(args); }

extern "C" int nfmc_dlmc_step_f32(const NfmcDlmcStepArgs* args, nfmc_stream_t stream) {
    if (int rc = check_dlmc_step(args)) return rc;
    return dlmc_launch<1>(args->flow, args->pot, nullptr, args->x, args->grad_u, args->n, args->step_size, nullptr,
                          args->logq_out, (hipStream_t)stream);
}
