// f1 for spline couplings: mean loss of a batch and its gradient with respect to every parameter of a 'c-rqnsf' flow
// (8-bin rational-quadratic spline couplings, conditioner width <= 8, d <= 256), for the maximum-likelihood fit
// (jump.py:139-151,193-201; imh.py:166-170) and the reverse-KL fit to a closed-form potential (imh.py:67-72,
// neutra.py:84-91).  One launch per optimiser step; fit_fold_kernel (fit_kernels.hip) folds the slabs and applies AdamW.
//
// Where the work is.  A spline target coordinate costs 23 conditioner outputs of HP multiply-adds each, the spline, its
// adjoint down to the 23 raw outputs, and 23 * HP weight-gradient entries: ~1300 instructions per (row, target, layer)
// against ~2 d_a HP for a row's whole hidden stack.  So the unit of parallelism is the (row, target) PAIR:
//   * a workgroup of 256 threads owns a tile of 16 rows (state and its gradient in LDS, as in fit_grad_kernel); 1024 rows
//     are 64 workgroups of four waves, not 16 waves;
//   * hidden stack: one thread per (row, hidden unit), activations to LDS;
//   * forward / inverse sweep: threads stride over the tile's (row, target) pairs, rows fastest, so the 16 lanes of a
//     target read the same W3 rows (16-byte loads from L1 / L2: at d = 256 the trainable vector is 220 KB and is not staged);
//   * reverse sweep, 16 targets at a time: thread (row, target) takes the layer input, evaluates the spline adjoint
//     (rqs_forward_backward / rqs_inverse_backward, flow_device.hpp), stages its 23 output deltas and its HP-vector of
//     dL/dh in LDS; then thread (target, output) walks the 16 rows in order and accumulates its W3 row (HP registers) and
//     bias, while thread (row, unit) adds the targets' dL/dh in target order.  No atomics, every sum in a fixed order;
//   * W1 / Wh / bias gradients and the ElementwiseAffine layers: transposed phases as in fit_grad_kernel.
// No activation is stored, so any number of coupling layers fits.  Reverse KL: going backward a layer's input is rebuilt from
// its output with the forward map, v = F(y), closed form and well conditioned wherever the inverse pass was.  Maximum
// likelihood: the input of layer l is recomputed from the tile's rows by running layers 0 .. l - 1 forward again, L (L - 1) / 2
// extra layer evaluations per tile of an L-layer flow (one for the default two layers), each a fraction of a layer's reverse
// step.  x_b = F^-1(z_b) would be closed form too, but fp32 cannot carry x through a forward pass of derivative 1e-3 and
// back.  The conditioner is re-evaluated from the unchanged half.  Slabs, tails, validation tiles, `first`-tile stores and
// run_state follow fit_grad_kernel.
#include "fit_rqs.hpp"

namespace nfmc {

template <int HP>
__device__ __forceinline__ void rqs_raw_outputs(const float* __restrict__ W3t, const float* __restrict__ b3t,
                                                const float* __restrict__ hrow, float (&raw)[kRqOut]) {
    float h[HP];
#pragma unroll
    for (int k = 0; k < HP; ++k) h[k] = hrow[k];
    const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(W3t);
#pragma unroll
    for (int q = 0; q < kRqOut; ++q) {
        float u = b3t[q];
#pragma unroll
        for (int k4 = 0; k4 < HP / 4; ++k4) {
            const f32x4 w = w4[q * (HP / 4) + k4];
            u = fmaf(w.x, h[4 * k4], u);
            u = fmaf(w.y, h[4 * k4 + 1], u);
            u = fmaf(w.z, h[4 * k4 + 2], u);
            u = fmaf(w.w, h[4 * k4 + 3], u);
        }
        raw[q] = u;
    }
}

// RKL = false: rows are data x; forward sweep x -> z, loss_i = -log N(z_i) - logdet_forward; reverse sweep last layer first.
// RKL = true:  rows are latents z; inverse sweep z -> x, loss_i = log N(z_i) - logdet_inverse + U(x_i); reverse sweep first
//              layer first.  Tiles [0, tiles) are batch rows, [tiles, tiles + vtiles) validation rows (loss only).
template <int HP, bool RKL>
__global__ void __launch_bounds__(kRqThreads) fit_rqs_kernel(FitRqsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (a.run_state && (a.run_state[3] != 0.f || a.run_state[4] != 0.f)) return;   // the run has ended
    constexpr int R = kRqRows, TC = kRqChunk, P = kRqOut, DS = kRqDrawStride, NT = kRqThreads;
    const NfmcRealNVP& f = a.f;
    const FlowGeom g = make_geom(f);
    const int d = g.d, stride = tile_stride(d), tid = threadIdx.x;
    float* const xt = lds;                      // state tile: row r at xt + r * stride
    float* const gt = xt + R * stride;          // gradient of the loss with respect to the state
    float* const h1 = gt + R * stride;          // [R][HP] first hidden layer
    float* const hl = h1 + R * HP;              // last hidden layer
    float* const dl = hl + R * HP;              // delta of the last hidden layer
    float* const df = dl + R * HP;              // delta of the first
    float* const dr = df + R * HP;              // [TC * P][DS] output deltas of a chunk: (target, output) major, rows minor
    float* const ghp = dr + TC * P * DS;        // [TC][HP][R] dL/dh of each (row, target) pair of a chunk
    float* const Pg = a.partial + (int64_t)blockIdx.x * a.pstride;
    const int o_b1 = g.d_a * HP, o_wht = o_b1 + HP, o_bh = o_wht + HP * HP;
    const int o_w3 = o_b1 + HP + (g.n_hl - 1) * (HP * HP + HP), o_b3 = o_w3 + P * g.d_b * HP;
    const int64_t ea_off = a.ea_off;
    const int d4 = a.d4;
    const bool rev_last = (g.n_coupling & 1) != 0;
    const int hr = tid / HP, hk = tid % HP;     // (row, hidden unit) of threads tid < R * HP
    const bool hthread = tid < R * HP;
    const int pr = tid % R, ptc = tid / R;      // (row, target of the chunk) of the reverse sweep: R * TC = NT
    bool first = true;
    float loss_acc = 0.f, rows_acc = 0.f, vloss_acc = 0.f, vrows_acc = 0.f;
    auto emit = [&](int64_t idx, float v) { Pg[idx] = first ? v : Pg[idx] + v; };
    // hidden stack of every row of the tile from the source half (xt must be settled; ends settled)
    auto hidden = [&](const float* __restrict__ W, bool rev) {
        if (hthread) {
            float acc = W[o_b1 + hk];
            const float* xr = xt + hr * stride;
#pragma unroll 8
            for (int j = 0; j < g.d_a; ++j) acc = fmaf(W[j * HP + hk], xr[phys(j, d, rev)], acc);   // loads run ahead of the chain
            h1[tid] = fast_tanh(acc);
        }
        __syncthreads();
        if (hthread) {
            float v = h1[tid];
            if (g.n_hl > 1) {
                float acc = W[o_bh + hk];
#pragma unroll
                for (int i = 0; i < HP; ++i) acc = fmaf(W[o_wht + i * HP + hk], h1[hr * HP + i], acc);
                v = fast_tanh(acc);
            }
            hl[tid] = v;
        }
        __syncthreads();
    };
    for (int64_t tile = blockIdx.x; tile < a.tiles + a.vtiles; tile += gridDim.x) {
        const bool val = tile >= a.tiles;          // workgroup-uniform
        const float* __restrict__ src = val ? a.xv : a.x;
        const int64_t nsrc = val ? a.nv : a.n, r0 = (val ? tile - a.tiles : tile) * R;
        const int nrow = (int)(nsrc - r0 < R ? nsrc - r0 : R);
        float lacc = 0.f;
        // the tile's rows into xt (all threads must be done with the tile's previous contents)
        auto load_rows = [&]() {
            __syncthreads();
            const int total = nrow * d;
            const float* s = src + r0 * d;
            const bool rev = RKL && rev_last;
            for (int i = tid; i < R * d; i += NT) {
                const int r = i / d, c = i - r * d;
                xt[r * stride + (rev ? d - 1 - c : c)] = i < total ? s[i] : 0.f;   // rows beyond the batch: zeros
            }
            __syncthreads();
        };
        // maximum likelihood: the first ElementwiseAffine and coupling layers [0, n_layers) applied to xt in place; with
        // `count` their log-derivatives go to the loss.  The reverse sweep runs it again, without, to get a layer's input.
        auto forward_layers = [&](int n_layers, bool count) {
            for (int i = tid; i < R * d; i += NT) {
                const int r = i / d, c = i - r * d;
                const float ls = f.ea0_log_scale[c];
                xt[r * stride + c] = fmaf(fast_exp(ls), xt[r * stride + c], f.ea0_shift[c]);
                if (count && r < nrow) lacc -= ls;
            }
            __syncthreads();
            for (int l = 0; l < n_layers; ++l) {
                const bool rev = (l & 1) == 0;
                const float* __restrict__ W = f.weights + l * g.layer_stride;
                hidden(W, rev);
                for (int idx = tid; idx < R * g.d_b; idx += NT) {
                    const int r = idx % R, t = idx / R;
                    float raw[P];
                    rqs_raw_outputs<HP>(W + o_w3 + (int64_t)t * P * HP, W + o_b3 + t * P, hl + r * HP, raw);
                    const int p = phys(g.d_a + t, d, rev);
                    float ld = 0.f;
                    xt[r * stride + p] = rqs_coordinate<false>(xt[r * stride + p], raw, g.bound, ld);
                    if (count && r < nrow) lacc -= ld;
                }
                __syncthreads();
            }
        };
        load_rows();
        if constexpr (!RKL) {
            // ---- forward sweep: z = f(x) in place
            forward_layers(g.n_coupling, true);
            for (int i = tid; i < R * d; i += NT) {
                const int r = i / d, c = i - r * d, p = phys(c, d, rev_last);
                const float ls = f.ea1_log_scale[c];
                const float z = fmaf(fast_exp(ls), xt[r * stride + p], f.ea1_shift[c]);
                xt[r * stride + p] = z;
                gt[r * stride + p] = r < nrow ? z : 0.f;     // dL/dz of 0.5 |z|^2; rows beyond the batch carry no gradient
                if (r < nrow) lacc += fmaf(0.5f * z, z, -ls);
            }
            if (tid < nrow) lacc += 0.5f * (float)d * kLog2Pi;
        } else {
            // ---- inverse sweep: x = f^-1(z) in place; -logdet_inverse = sum of the forward log-derivatives
            for (int i = tid; i < R * d; i += NT) {
                const int r = i / d, c = i - r * d, p = phys(c, d, rev_last);
                const float ls = f.ea1_log_scale[c], z = xt[r * stride + p];
                xt[r * stride + p] = (z - f.ea1_shift[c]) * fast_exp(-ls);
                if (r < nrow) lacc += fmaf(-0.5f * z, z, ls);
            }
            __syncthreads();
            for (int l = g.n_coupling - 1; l >= 0; --l) {
                const bool rev = (l & 1) == 0;
                const float* __restrict__ W = f.weights + l * g.layer_stride;
                hidden(W, rev);
                for (int idx = tid; idx < R * g.d_b; idx += NT) {
                    const int r = idx % R, t = idx / R;
                    float raw[P];
                    rqs_raw_outputs<HP>(W + o_w3 + (int64_t)t * P * HP, W + o_b3 + t * P, hl + r * HP, raw);
                    const int p = phys(g.d_a + t, d, rev);
                    float ld = 0.f;
                    xt[r * stride + p] = rqs_coordinate<true>(xt[r * stride + p], raw, g.bound, ld);
                    if (r < nrow) lacc += ld;
                }
                __syncthreads();
            }
            for (int i = tid; i < R * d; i += NT) {
                const int r = i / d, c = i - r * d;
                const float ls = f.ea0_log_scale[c];
                xt[r * stride + c] = (xt[r * stride + c] - f.ea0_shift[c]) * fast_exp(-ls);
                if (r < nrow) lacc += ls;
            }
            __syncthreads();
            if (tid < R) {   // U(x) and dL/dx = grad U, one thread per row
                float* grow = gt + tid * stride;
                const float u = potential_value_grad_row(xt + tid * stride, grow, a.pot, d);
                if (tid < nrow) {
                    lacc += u - 0.5f * (float)d * kLog2Pi;
                } else {
                    for (int c = 0; c < d; ++c) grow[c] = 0.f;
                }
            }
        }
        if (val) {
            vloss_acc += lacc;
            if (tid < nrow) vrows_acc += 1.f;
            continue;
        }
        loss_acc += lacc;
        if (tid < nrow) rows_acc += 1.f;
        __syncthreads();
        // ---- reverse sweep.  ElementwiseAffine next to the loss, transposed (thread = coordinate, rows in order)
        if constexpr (!RKL) {
            for (int c = tid; c < d; c += NT) {   // z_p = e^s y_p + t
                const int p = phys(c, d, rev_last);
                const float s = f.ea1_log_scale[c], t = f.ea1_shift[c];
                const float es = fast_exp(s);
                float as = 0.f, at = 0.f;
                for (int r = 0; r < R; ++r) {
                    const float gz = gt[r * stride + p], zc = xt[r * stride + p] - t;
                    as = fmaf(gz, zc, as);
                    at += gz;
                    gt[r * stride + p] = gz * es;
                }
                emit(ea_off + 2 * d4 + c, as - (float)nrow);   // d(-logdet)/ds = -1 per row
                emit(ea_off + 3 * d4 + c, at);
            }
        } else {
            for (int c = tid; c < d; c += NT) {   // x = (y - t) e^-s, -logdet_inverse contains +s
                const float s = f.ea0_log_scale[c], t = f.ea0_shift[c];
                const float es = fast_exp(s), eis = fast_exp(-s);
                float as = 0.f, at = 0.f;
                for (int r = 0; r < R; ++r) {
                    const float gx = gt[r * stride + c], xv = xt[r * stride + c];
                    const float gy = gx * eis;
                    as = fmaf(-gx, xv, as);
                    at -= gy;
                    gt[r * stride + c] = gy;
                    xt[r * stride + c] = fmaf(es, xv, t);
                }
                emit(ea_off + c, as + (float)nrow);
                emit(ea_off + d4 + c, at);
            }
        }
        __syncthreads();
        for (int li = 0; li < g.n_coupling; ++li) {
            const int l = RKL ? li : g.n_coupling - 1 - li;
            const bool rev = (l & 1) == 0;
            const float* __restrict__ W = f.weights + l * g.layer_stride;
            const int64_t L0 = (int64_t)l * g.layer_stride;
            if constexpr (!RKL) {
                // The layer's INPUT, by running the rows forward again through the layers before it.  Inverting the layer's
                // output instead loses it: through a knot of derivative 1e-3 (fitted splines have them) one ulp of z spans
                // 5e-4 of x, and every gradient of this and the earlier layers inherits that error.
                load_rows();
                forward_layers(l, false);
            }
            hidden(W, rev);
            float ghacc = 0.f;   // dL/dh_last of (row hr, unit hk)
            for (int c0 = 0; c0 < g.d_b; c0 += TC) {
                const int nt = g.d_b - c0 < TC ? g.d_b - c0 : TC;
                if (ptc < nt) {
                    // ---- thread = (row, target): layer input rebuilt, spline adjoint, output deltas and dL/dh to LDS
                    const int t = c0 + ptc, p = phys(g.d_a + t, d, rev);
                    const float* __restrict__ W3t = W + o_w3 + (int64_t)t * P * HP;
                    float raw[P], draw[P];
                    rqs_raw_outputs<HP>(W3t, W + o_b3 + t * P, hl + pr * HP, raw);
                    const bool ok = pr < nrow;
                    const float so = xt[pr * stride + p], go = gt[pr * stride + p];   // reverse KL: the layer's output side
                    float gi;
                    if constexpr (!RKL) {
                        rqs_forward_backward(so, go, raw, g.bound, draw, gi);     // xt holds the layer's input already
                    } else {
                        float si;                                                 // v = F(y), rebuilt with the forward map
                        rqs_inverse_backward(so, go, raw, g.bound, draw, si, gi);
                        xt[pr * stride + p] = si;
                    }
                    gt[pr * stride + p] = ok ? gi : 0.f;
                    float gh[HP];
#pragma unroll
                    for (int k = 0; k < HP; ++k) gh[k] = 0.f;
                    const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(W3t);
#pragma unroll
                    for (int q = 0; q < P; ++q) {
                        const float dq = ok ? draw[q] : 0.f;    // rows beyond the batch: no log-derivative term either
                        dr[(ptc * P + q) * DS + pr] = dq;
#pragma unroll
                        for (int k4 = 0; k4 < HP / 4; ++k4) {
                            const f32x4 w = w4[q * (HP / 4) + k4];
                            gh[4 * k4] = fmaf(w.x, dq, gh[4 * k4]);
                            gh[4 * k4 + 1] = fmaf(w.y, dq, gh[4 * k4 + 1]);
                            gh[4 * k4 + 2] = fmaf(w.z, dq, gh[4 * k4 + 2]);
                            gh[4 * k4 + 3] = fmaf(w.w, dq, gh[4 * k4 + 3]);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < HP; ++k) ghp[(ptc * HP + k) * R + pr] = gh[k];
                }
                __syncthreads();
                // ---- thread = (target, output): its W3 row and bias over the rows of the tile, in row order
                for (int e = tid; e < nt * P; e += NT) {
                    const int tc = e / P, q = e - tc * P;
                    float acc[HP], sb = 0.f;
#pragma unroll
                    for (int k = 0; k < HP; ++k) acc[k] = 0.f;
                    for (int r = 0; r < R; ++r) {
                        const float dv = dr[e * DS + r];
                        sb += dv;
#pragma unroll
                        for (int k = 0; k < HP; ++k) acc[k] = fmaf(dv, hl[r * HP + k], acc[k]);
                    }
                    const int64_t row = (int64_t)(c0 + tc) * P + q;
#pragma unroll
                    for (int k = 0; k < HP; ++k) emit(L0 + o_w3 + row * HP + k, acc[k]);
                    emit(L0 + o_b3 + row, sb);
                }
                if (hthread)
                    for (int tc = 0; tc < nt; ++tc) ghacc += ghp[(tc * HP + hk) * R + hr];
                __syncthreads();
            }
            // ---- back through the hidden stack
            if (hthread) {
                const float hv = hl[tid];
                dl[tid] = ghacc * (1.f - hv * hv);
            }
            __syncthreads();
            if (hthread) {
                float v = dl[tid];
                if (g.n_hl > 1) {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < HP; ++k) acc = fmaf(W[o_wht + hk * HP + k], dl[hr * HP + k], acc);
                    const float hv = h1[tid];
                    v = acc * (1.f - hv * hv);
                }
                df[tid] = v;
            }
            __syncthreads();
            for (int idx = tid; idx < R * g.d_a; idx += NT) {   // dL/dx_a += W1^T delta_first
                const int r = idx % R, j = idx / R;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < HP; ++k) acc = fmaf(W[j * HP + k], df[r * HP + k], acc);
                gt[r * stride + phys(j, d, rev)] += acc;
            }
            for (int e = tid; e < g.d_a * HP; e += NT) {        // W1^T (d_a, HP)
                const int j = e / HP, k = e - j * HP, p = phys(j, d, rev);
                float acc = 0.f;
                for (int r = 0; r < R; ++r) acc = fmaf(xt[r * stride + p], df[r * HP + k], acc);
                emit(L0 + e, acc);
            }
            if (g.n_hl > 1) {
                for (int e = tid; e < HP * HP; e += NT) {       // Wh^T (HP_in, HP_out)
                    const int i = e / HP, k = e - i * HP;
                    float acc = 0.f;
                    for (int r = 0; r < R; ++r) acc = fmaf(h1[r * HP + i], dl[r * HP + k], acc);
                    emit(L0 + o_wht + e, acc);
                }
            }
            if (tid < HP) {
                float a1 = 0.f, a2 = 0.f;
                for (int r = 0; r < R; ++r) {
                    a1 += df[r * HP + tid];
                    a2 += dl[r * HP + tid];
                }
                emit(L0 + o_b1 + tid, a1);
                if (g.n_hl > 1) emit(L0 + o_bh + tid, a2);
            }
            __syncthreads();
        }
        if constexpr (!RKL) {
            for (int c = tid; c < d; c += NT) {   // first ElementwiseAffine: the tile holds its OUTPUT y = e^s x + t and dL/dy
                const float t = f.ea0_shift[c];
                float as = 0.f, at = 0.f;
                for (int r = 0; r < R; ++r) {
                    const float gy = gt[r * stride + c];
                    as = fmaf(gy, xt[r * stride + c] - t, as);
                    at += gy;
                }
                emit(ea_off + c, as - (float)nrow);
                emit(ea_off + d4 + c, at);
            }
        } else {
            for (int c = tid; c < d; c += NT) {   // last ElementwiseAffine inverted: the tile holds v = (z - t) e^-s and dL/dv
                const int p = phys(c, d, rev_last);
                const float eis = fast_exp(-f.ea1_log_scale[c]);
                float as = 0.f, at = 0.f;
                for (int r = 0; r < R; ++r) {
                    const float gv = gt[r * stride + p];
                    as = fmaf(-gv, xt[r * stride + p], as);
                    at = fmaf(-gv, eis, at);
                }
                emit(ea_off + 2 * d4 + c, as + (float)nrow);
                emit(ea_off + 3 * d4 + c, at);
            }
        }
        first = false;
    }
    // losses and row counts of this workgroup's rows: fixed-order sums over the threads
    __syncthreads();
    dr[tid] = loss_acc;
    dr[NT + tid] = rows_acc;
    dr[2 * NT + tid] = vloss_acc;
    dr[3 * NT + tid] = vrows_acc;
    __syncthreads();
    if (tid < 4) {
        float s = 0.f;
        for (int r = 0; r < NT; ++r) s += dr[NT * tid + r];
        Pg[a.n_params + tid] = s;
    }
}

int fit_rqs_launch(bool rkl, int hp, const FitRqsArgs& a, int grid, hipStream_t st) {
    static_assert(kRqRows * kRqChunk == kRqThreads, "one (row, target) pair per thread and chunk");
    static_assert(kRqChunk * kRqOut * kRqDrawStride >= 4 * kRqThreads, "the loss reduction reuses the delta stage");
    const size_t lds = fit_rqs_lds_floats(a.f.d, hp) * sizeof(float);
    int rc = NFMC_EUNSUPPORTED;
    if (hp == 4) rc = rkl ? launch_lds(fit_rqs_kernel<4, true>, grid, kRqThreads, lds, st, a)
                          : launch_lds(fit_rqs_kernel<4, false>, grid, kRqThreads, lds, st, a);
    if (hp == 8) rc = rkl ? launch_lds(fit_rqs_kernel<8, true>, grid, kRqThreads, lds, st, a)
                          : launch_lds(fit_rqs_kernel<8, false>, grid, kRqThreads, lds, st, a);
    if (rc != NFMC_OK) return rc;
    NFMC_HIP_CHECK_LAUNCH();
    return NFMC_OK;
}

}  // namespace nfmc
