// K1/K2 (+K6, K7): fused Langevin (MALA/ULA) and HMC/UHMC transitions for closed-form potentials.
//
// Replaces, per transition, the reference's eager-op sequence
//   Langevin.propose  nfmc/algorithms/sampling/mcmc/langevin.py:61-122
//   HMC.propose       nfmc/algorithms/sampling/mcmc/hmc.py:61-77,96-126
//   masked update, counters, streaming moments, sample store   mcmc/base.py:74-90, sampling/base.py:75-95,234-259
//
// Layout: a chain is spread over LPC consecutive lanes, lane g holding the CPL contiguous
// coordinates g*CPL.. (16-byte vector IO).  The state stays in VGPRs for all n_steps of a call, so
// HBM sees one read and one write of (n, d) per call (plus one write per step if samples are kept);
// the kernel is VALU-bound (Philox + Box-Muller + ~25 flop per coordinate), not HBM-bound.
// One butterfly reduction per transition produces the log acceptance ratio in every lane of the
// group; the accept count comes from a wave ballot.
#pragma once

#include "flow_b.hpp"
#include "pot_shared.hpp"

namespace nfmc {

template <int CPL, int LPC, bool FAST>
struct MassCoef {
    // Langevin: c1 = -h/m^2, c2 = sqrt(2h)/m, hA = h/m^2, invA = m^2 ; HMC: rs = 1/sqrt(m), m
    // Random-walk proposals (mh.py:51-55): x' = x + m eps, symmetric => c1 = 0, c2 = m and no q terms.
    float c1_s, c2_s, hA_s, cg_s, kap_s;
    float c1[FAST ? 1 : CPL], c2[FAST ? 1 : CPL], hA[FAST ? 1 : CPL], invA[FAST ? 1 : CPL];
    float m[FAST ? 1 : CPL], rs[FAST ? 1 : CPL], cg[FAST ? 1 : CPL], kap[FAST ? 1 : CPL];

    // coefficients of the closed-form quadratic-potential transition: x' = x + cg t + c2 eps,
    // log r = sum kap (t^2 - t'^2);  MALA: cg = -2 a h/m^2, kap = a^2 h/m^2;  random walk: cg = 0, kap = a
    template <class PotT>
    __device__ __forceinline__ void init_quadratic(const PotT& pot, bool rw) {
        cg_s = rw ? 0.f : c1_s * (2.f * pot.aa(0));
        kap_s = rw ? pot.aa(0) : pot.aa(0) * pot.aa(0) * hA_s;
        if constexpr (!FAST) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                cg[i] = rw ? 0.f : c1[i] * (2.f * pot.aa(i));
                kap[i] = rw ? pot.aa(i) : pot.aa(i) * pot.aa(i) * hA[i];
            }
        }
    }
    __device__ __forceinline__ float CG(int i) const { return FAST ? cg_s : cg[FAST ? 0 : i]; }
    __device__ __forceinline__ float KAP(int i) const { return FAST ? kap_s : kap[FAST ? 0 : i]; }

    __device__ __forceinline__ void init(float h, float sqrt2h, const float* __restrict__ imd, int g, int d,
                                         bool rw = false) {
        c1_s = rw ? 0.f : -h;
        c2_s = rw ? 1.f : sqrt2h;
        hA_s = h;
        if constexpr (!FAST) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = coord_of<CPL, LPC>(g, i);
                const bool ok = c < d;
                const float mm = (ok && imd) ? imd[c] : 1.f;
                const float A = 1.f / (mm * mm);
                c1[i] = (ok && !rw) ? (-h) / (mm * mm) : 0.f;
                c2[i] = ok ? (rw ? mm : sqrt2h / mm) : 0.f;
                hA[i] = ok ? h * A : 0.f;
                invA[i] = ok ? 1.f / A : 0.f;
                m[i] = ok ? mm : 0.f;
                rs[i] = ok ? 1.f / sqrtf(mm) : 0.f;
            }
        }
    }
    __device__ __forceinline__ float C1(int i) const { return FAST ? c1_s : c1[FAST ? 0 : i]; }
    __device__ __forceinline__ float C2(int i) const { return FAST ? c2_s : c2[FAST ? 0 : i]; }
    __device__ __forceinline__ float HA(int i) const { return FAST ? hA_s : hA[FAST ? 0 : i]; }
    __device__ __forceinline__ float IA(int i) const { return FAST ? 1.f : invA[FAST ? 0 : i]; }
    __device__ __forceinline__ float M(int i) const { return FAST ? 1.f : m[FAST ? 0 : i]; }
    __device__ __forceinline__ float RS(int i) const { return FAST ? 1.f : rs[FAST ? 0 : i]; }
};

// Tuning launches (NfmcTune) accumulate the variance sums about a per-coordinate shift c -- x - c and (x - c)^2 -- that
// the controller keeps near the chains' mean (tune_finish_kernel un-shifts in fp64): raw fp32 sums of x and x^2 cancel
// for chains far from the origin relative to their spread.  ON only in the TUNE instantiations of the general kernels
// (launch_*_kernel picks them for launches with a tuning state): every other instantiation carries no shift registers
// and sums x itself, as before.
template <int CPL, int LPC, bool ON>
struct StatShift {
    float c[ON ? CPL : 1];
    // per tile: the rows past n hold x = 0 and must add 0, not -c (a few L2-resident loads per tile)
    __device__ __forceinline__ void init(const NfmcTune& tn, int g, int d, bool active) {
        if constexpr (ON) {
            const double* __restrict__ src = tn.state + NFMC_TUNE_WORDS + 2 * CPL * LPC + kStatTail;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int k = coord_of<CPL, LPC>(g, i);
                c[i] = (active && k < d) ? (float)src[k] : 0.f;
            }
        }
    }
    __device__ __forceinline__ float operator()(const float (&x)[CPL], int i) const {
        if constexpr (ON) return x[i] - c[i];
        else return x[i];
    }
};

// Leapfrog steps of the transition with Philox step counter k under a jittered trajectory (NfmcTune.trajectory, header
// comment in nfmc_hip.h): clamp(ceil(u T / h), 1, L_max), u the base-2 radical inverse of k + 1 plus half a grid step.
// THE definition: the hmc kernel, the controller's leapfrog total (tune_finish_kernel) and tuning.leapfrog_count on the
// host all evaluate these fp64 operations in this order, without contraction, so they agree to the integer.
__host__ __device__ inline int trajectory_leapfrog_count(uint32_t k, double T, double h, double lmax) {
#pragma clang fp contract(off)
    const double u = ((double)__builtin_bitreverse32(k + 1u) + 0.5) * 0x1p-32;
    const double r = ceil(u * T / h);
    const double cap = lmax >= 1.0 ? (lmax < 1048576.0 ? lmax : 1048576.0) : 1.0;
    return r >= 1.0 ? (int)(r < cap ? r : cap) : 1;   // NaN -> 1
}

// The jittered trajectory of the TUNE instantiations of hmc_kernel (ON; every other kernel carries nothing of it): the
// leapfrog count of each transition and, while the length adapts, this lane's fp32 sums over the launch's transitions
// and tiles of alpha g and alpha, the ChEES terms about the lagged centre (StatShift's c).  Every lane of a chain holds
// the chain's sums; flush() adds the group leaders' in fp64 into the two jump columns of the workgroup's statistics
// slab, which a tuning launch (no jump tail) leaves zero, so the fold kernels total them with the other columns.
template <int CPL, int LPC, bool ON>
struct Trajectory {
    int mode, L;   // L: the leapfrog count of the transition in flight
    double T, h, lmax;
    float sum_g, sum_alpha;
    __device__ __forceinline__ void init(const NfmcTune& tn) {
        if constexpr (ON) {
            mode = tn.trajectory;
            sum_g = sum_alpha = 0.f;
            if (mode) {
                const double* __restrict__ tr = tn.state + NFMC_TUNE_WORDS + 3 * CPL * LPC + kStatTail;
                T = tr[NFMC_TRAJ_LENGTH];
                lmax = tr[NFMC_TRAJ_MAX_LEAPFROG];
                h = tn.state[NFMC_TUNE_STEP_SIZE];
            }
        }
    }
    // wave-uniform: every chain of a launch runs the same trajectory
    __device__ __forceinline__ int leapfrogs(int fixed, uint32_t k) {
        if constexpr (ON) {
            L = mode ? __builtin_amdgcn_readfirstlane(trajectory_leapfrog_count(k, T, h, lmax)) : fixed;
            return L;
        }
        return fixed;
    }
    // after the Metropolis test, before the state moves: x the current state, q the proposal, p the final momentum
    template <class Shift, class Mass>
    __device__ __forceinline__ void accumulate(const float (&x)[CPL], const float (&q)[CPL], const float (&p)[CPL],
                                               const Shift& shift, const Mass& mc, float lr, bool active) {
        if constexpr (ON) {
            if (mode != NFMC_TRAJECTORY_ADAPT) return;
            float a0 = 0.f, a1 = 0.f, b = 0.f;   // padded coordinates: x = q = c = 0 and zero mass
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const float dx = x[i] - shift.c[i], dq = q[i] - shift.c[i];
                a0 = fmaf(dx, dx, a0);
                a1 = fmaf(dq, dq, a1);
                b = fmaf(dq, p[i] * mc.M(i), b);
            }
            a0 = group_allreduce<LPC>(a0);
            a1 = group_allreduce<LPC>(a1);
            b = group_allreduce<LPC>(b);
            const float t = (float)((double)L * h);
            const bool ok = active && fabsf(lr) <= 3.0e38f && a0 <= 3.0e38f && a1 <= 3.0e38f && fabsf(b) <= 3.0e38f;
            const float alpha = ok ? fast_exp(fminf(lr, 0.f)) : 0.f;
            const float g = ok ? t * (a1 - a0) * b : 0.f;
            sum_g = fmaf(alpha, g, sum_g);
            sum_alpha += alpha;
        }
    }
    // behind block_stats_flush, whose owner threads have written this workgroup's slab (the jump columns as zeros)
    __device__ __forceinline__ void flush(const NfmcStats& st) {
        if constexpr (ON) {
            if (mode != NFMC_TRAJECTORY_ADAPT) return;
            __shared__ double tail[kWavesPerBlock][2];
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            const double wg = cross_chain_reduce_f64<LPC>((double)sum_g);       // lane 0: the sum over the group leaders
            const double wa = cross_chain_reduce_f64<LPC>((double)sum_alpha);
            if (lane == 0) {
                tail[wave][0] = wg;
                tail[wave][1] = wa;
            }
            __syncthreads();   // also orders the owner threads' stores of the two columns before the stores below
            if (threadIdx.x == 0) {
                double sg = 0.0, sa = 0.0;
#pragma unroll
                for (int w = 0; w < kWavesPerBlock; ++w) {
                    sg += tail[w][0];
                    sa += tail[w][1];
                }
                double* out = st.scratch + (size_t)blockIdx.x * (2 * CPL * LPC + kStatTail) + 2 * CPL * LPC;
                out[2] = sg;
                out[3] = sa;
            }
        }
    }
};

// noise for this lane's CPL coordinates of (chain, step): native Philox or (REPLAY) replay from HBM
template <int CPL, int LPC, int R = 10, bool REPLAY = true>
__device__ __forceinline__ void draw_normals(const NfmcRng& rng, uint32_t tag, uint32_t gchain, int64_t row, int64_t n,
                                             int d, int g, int s, float (&e)[CPL]) {
    if (REPLAY && rng.replay_normals) {
        const float* p = rng.replay_normals + ((int64_t)s * n + row) * d;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            e[i] = (row < n && c < d) ? p[c] : 0.f;
        }
    } else {
        const uint32_t k0 = (uint32_t)rng.seed, k1 = (uint32_t)(rng.seed >> 32);
#pragma unroll
        for (int b = 0; b < CPL / 4; ++b) {   // philox_normal4, with the step (wave-uniform) folded on the SALU
            const uint4 r = philox4x32<R, true>(gchain, rng.step0 + (uint32_t)s, (uint32_t)(b * LPC + g), tag, k0, k1);
            const nfmc_f2 z0 = box_muller_pk(r.x, r.y), z1 = box_muller_pk(r.z, r.w);
            e[4 * b] = z0.x;
            e[4 * b + 1] = z0.y;
            e[4 * b + 2] = z1.x;
            e[4 * b + 3] = z1.y;
        }
    }
}

// ln u of the Metropolis test of transition s: word step & 3 of Philox block step >> 2 on stream kTagAccept, or (REPLAY)
// the replayed u.  LPC == 1: every lane draws its chain's block once per 4 transitions and picks the word.  LPC >= 2:
// all lanes of a chain need the same value, so they share the work: lane g draws block q0 + g, converts its four words to
// ln u once and leaves them in its 16 bytes of `slab` (LDS, one float4 per lane of the workgroup); one refresh covers the
// chain's next 4 LPC transitions, each of which reads word step - 4 q0 of the chain's LPC float4 (a broadcast read, one
// VALU address add).  Same block, same word, same conversion, same v_log as the per-lane draw: bitwise the same ln u.
template <int LPC, int R = 10, bool REPLAY = true>
struct AcceptLnU {
    uint4 r;                 // LPC == 1: the current block
    float4* mine;            // LPC >= 2: this lane's four ln u
    const float* chain;      // ... and its chain's 4 LPC of them
    uint32_t base;           // step of chain[0] (a multiple of 4; wave-uniform)
    __device__ __forceinline__ AcceptLnU(float4* slab, int g) {
        if constexpr (LPC > 1) {
            mine = slab + threadIdx.x;
            chain = reinterpret_cast<const float*>(slab + (threadIdx.x - g));
        }
    }
    __device__ __forceinline__ float draw(const NfmcRng& rng, uint32_t gchain, int64_t row, int64_t n, int g, int s) {
        if (REPLAY && rng.replay_uniforms) return fast_ln(row < n ? rng.replay_uniforms[(int64_t)s * n + row] : 0.5f);
        const uint32_t step = rng.step0 + (uint32_t)s, k0 = (uint32_t)rng.seed, k1 = (uint32_t)(rng.seed >> 32);
        if constexpr (LPC == 1) {
            if (s == 0 || (step & 3u) == 0u) r = philox4x32<R>(gchain, step >> 2, 0u, kTagAccept, k0, k1);
            return fast_ln(u32_to_uniform(pick_word(r, step & 3u)));
        } else {
            // refresh at the first transition, when the slab is used up, and where the 32-bit step wraps (block 0 next)
            if (s == 0 || step - base == 4u * LPC || step == 0u) {
                base = step & ~3u;
                const uint4 w = philox4x32<R>(gchain, (base >> 2) + (uint32_t)g, 0u, kTagAccept, k0, k1);
                *mine = make_float4(fast_ln(u32_to_uniform(w.x)), fast_ln(u32_to_uniform(w.y)),
                                    fast_ln(u32_to_uniform(w.z)), fast_ln(u32_to_uniform(w.w)));
                __builtin_amdgcn_wave_barrier();   // a chain's lanes write and read in one wave: keep the order, no s_barrier
            }
            return chain[step - base];
        }
    }
};

// ------------------------------------------------------------------------------------------------
// Device-side copy of NfmcJumpTail (the header's struct is a host pointer target).
struct JumpDev {
    NfmcRealNVP flow;
    int adjusted;
    const float* replay_latent;
    const float* replay_uniform;
    uint8_t* mask_out;
    float* log_ratio_out;
};

// One flow-proposal Metropolis jump on the registers of the chain (jump.py:205-243).  Returns accept.
// The flow code lifts a fused kernel to ~208 VGPRs (occupancy 5 -> 2 for the whole launch), which costs the inner
// transitions more than the separate flow-MH launch: the tail is exercised by the tests but off by default.
template <int CPL, int LPC, int HP, class FlowT, class PotT>
__device__ __forceinline__ bool jump_once(float (&x)[CPL], const FlowT& fl, const PotT& pot,
                                          const JumpDev& j, uint64_t seed, uint32_t step, uint32_t gchain, int64_t row,
                                          int64_t n, int d, int g, bool active, float& lr_out, bool& bad) {
    const bool revl = (j.flow.n_coupling & 1) != 0;
    float part;  // this lane's share of  -u(x) ... assembled so that ONE butterfly gives log alpha
    {
        const auto ctx = pot.prepare(x, g, d);
        float w[CPL];
        part = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            part += pot.term(ctx, i, x[i]);       // + u(x)                      jump.py:212
            w[i] = x[i];
        }
        part += fl.forward(w);                    // + log q(x) = logdet_fwd - z^2/2 (+c)   jump.py:218
#pragma unroll
        for (int i = 0; i < CPL; ++i) part = fmaf(-0.5f * w[i], w[i], part);
    }
    float xp[CPL];
    draw_latent<CPL, LPC>(xp, j.replay_latent, seed, step, gchain, row, n, d, g, revl);  // flow.sample  jump.py:205
#pragma unroll
    for (int i = 0; i < CPL; ++i) part = fmaf(0.5f * xp[i], xp[i], part);               // - log q(x') ...
    part += fl.inverse(xp);                                                               // ... = z'^2/2 + logdet_inv (-c)
    {
        const auto ctx = pot.prepare(xp, g, d);
#pragma unroll
        for (int i = 0; i < CPL; ++i) part -= pot.term(ctx, i, xp[i]);                   // - u(x')     jump.py:213
    }
    const float lr = group_allreduce<LPC>(part);                                          // util.py:392
    bool accept = true;
    bad = false;
    if (j.adjusted) {
        float u;
        if (j.replay_uniform) {
            u = active ? j.replay_uniform[row] : 0.5f;
        } else {
            const uint4 r = philox4x32_10(gchain, step, 0u, kTagJump, (uint32_t)seed, (uint32_t)(seed >> 32));
            u = u32_to_uniform(r.x);
        }
        accept = fast_ln(u) < lr;                                                         // jump.py:225
        bad = active && !(fabsf(lr) <= 3.0e38f);
    }
    accept = accept && active;
    const uint64_t am = __ballot(accept);
#pragma unroll
    for (int i = 0; i < CPL; ++i) x[i] = select_f32(am, xp[i], x[i]);                    // jump.py:231
    lr_out = lr;
    return accept;
}

// ------------------------------------------------------------------------------------------------
// LEAN: the launch has no per-step output and no replay (masks_out, log_ratio_out, samples.base, replay_normals and
// replay_uniforms all null; launch_mala_cfg checks), so none of their pointers or branches is in the step loop.
// TUNE: a warmup launch (a.tune.state set): the variance sums are taken about the tuning state's shift (StatShift)
template <int CPL, int LPC, template <int, int, bool> class Pot, bool FAST, int JHP, int RR = 10, bool LEAN = false,
          bool TUNE = false>
__global__ void __launch_bounds__(kBlock, NFMC_WPE) mala_kernel(NfmcMalaArgs a, float sqrt2h, int64_t tiles, JumpDev jd) {
    static_assert(!LEAN || JHP == 0, "the jump tail keeps its own outputs");
    static_assert(!TUNE || (JHP == 0 && !FAST && !LEAN), "tuning launches run the general kernels without a jump tail");
    extern __shared__ __attribute__((aligned(16))) float flow_lds[];
    __shared__ float4 accept_slab[LPC > 1 ? kBlock : 1];
    constexpr int CPW = kWave / LPC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane % LPC, cw = lane / LPC;
    const int d = a.d;
    const int64_t n = a.n;
    // warmup: the step size lives in device memory, where the controller of the previous call left it (NfmcTune)
    const double h_dev = a.tune.state ? a.tune.state[NFMC_TUNE_STEP_SIZE] : 0.0;
    const float h = a.tune.state ? (float)h_dev : a.step_size;
    if (a.tune.state) sqrt2h = (float)sqrt(2.0 * h_dev);   // math.sqrt(2 * step_size) of the fp64 step, langevin.py:75
    const bool adjust = (a.adjust & 1) != 0, rw = (a.adjust & 2) != 0;
    const float inv4h = rw ? 0.f : 1.f / (4.f * h);

    MassCoef<CPL, LPC, FAST> mc;
    mc.init(h, sqrt2h, a.inv_mass_diag, g, d, rw);
    Pot<CPL, LPC, FAST> pot;
    if constexpr (!Pot<CPL, LPC, FAST>::kStaged) pot.init(a.pot, g, d);
    if constexpr (Pot<CPL, LPC, FAST>::kQuadratic) mc.init_quadratic(pot, rw);
    FlowB<CPL, LPC, JHP == 0 ? 4 : JHP, true, (FAST && CPL >= 8 && JHP > 0)> fl;
    if constexpr (JHP > 0) {
        decltype(fl)::Img::stage(flow_lds, jd.flow, kBlock);
        __syncthreads();
        fl.init(flow_lds, jd.flow, g);
    }
    if constexpr (Pot<CPL, LPC, FAST>::kStaged)
        init_staged(pot, a.pot, g, d, flow_lds,
                    JHP > 0 ? decltype(fl)::Img::total_floats(jd.flow.n_hidden_layers, jd.flow.n_coupling) : 0);

    float sx[CPL], sxx[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) sx[i] = sxx[i] = 0.f;
    StatShift<CPL, LPC, TUNE> shift;
    uint32_t n_acc = 0, n_bad = 0, j_acc = 0, j_bad = 0;
    constexpr unsigned long long leaders = group_leaders(LPC);

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (tile * kWavesPerBlock + wave) * CPW + cw;
        const bool active = row < n;
        const uint32_t gchain = (uint32_t)(a.rng.chain_offset + (uint64_t)row);
        float x[CPL];
        load_row<CPL, LPC, FAST>(a.x, row, d, g, active, x);
        shift.init(a.tune, g, d, active);
        AcceptLnU<LPC, RR, !LEAN> au(accept_slab, g);
        StoreCursor keep(a.samples);
        const uint64_t live = __ballot(active);   // the wave's lanes with a chain
        float sq = 0.f, sq_prop = 0.f;   // FAST quadratic: this lane's share of |x|^2 (current state / proposal)
        if constexpr (Pot<CPL, LPC, FAST>::kQuadratic && FAST) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) sq = fmaf(x[i], x[i], sq);
        }

        for (int s = 0; s < a.n_steps; ++s) {
            float e[CPL], xp[CPL];
            draw_normals<CPL, LPC, RR, !LEAN>(a.rng, kTagNoise, gchain, row, n, d, g, s, e);
            float lr = 0.f;
            if constexpr (Pot<CPL, LPC, FAST>::kQuadratic && FAST) {
                // FAST: scalar a, b = 0, unit mass.  The ratio below, a^2 h (sum_j x_j^2 - sum_j x'_j^2), needs only
                // this lane's share of |x'|^2: the share of |x|^2 is carried from the previous transition (`sq`,
                // replaced by the proposal's on acceptance).  3 VALU instructions per coordinate for proposal + ratio.
                // Coordinate pairs as v_pk_fma_f32 (the even / odd partial sums of |x'|^2 are the two halves of sp).
                nfmc_f2 sp = {0.f, 0.f};
                const nfmc_f2 cg = {mc.CG(0), mc.CG(0)}, c2 = {mc.C2(0), mc.C2(0)};
#pragma unroll
                for (int i = 0; i < CPL; i += 2) {
                    const nfmc_f2 xi = {x[i], x[i + 1]}, ei = {e[i], e[i + 1]};
                    // langevin.py:74-76 / mh.py:55
                    const nfmc_f2 p = __builtin_elementwise_fma(c2, ei, __builtin_elementwise_fma(cg, xi, xi));
                    xp[i] = p.x;
                    xp[i + 1] = p.y;
                    sp = __builtin_elementwise_fma(p, p, sp);
                }
                sq_prop = sp.x + sp.y;
                // rounded product: where the compiler places this multiply in the reduction's block it would otherwise
                // contract it with the reduction's first add into one fma, which changes the bits of log r
                {
#pragma clang fp contract(off)
                    lr = mc.KAP(0) * (sq - sq_prop);
                }
            } else if constexpr (Pot<CPL, LPC, FAST>::kQuadratic) {
                // U = sum a (x-b)^2: with t = x - b, t' = x' - b the reference's ratio (langevin.py:88-105)
                //   (u - u') + [q(x'|x) - q(x|x')]   collapses term by term to   a^2 (h/m^2) (t^2 - t'^2)
                // (expand tf = d + 2 a hA t, tb = -d + 2 a hA t', d = t' - t; invA hA = h): same value, 7
                // instead of 17 VALU instructions per coordinate; checked against the golden vectors.
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const float t = x[i] - pot.bb(i);
                    xp[i] = fmaf(mc.C2(i), e[i], fmaf(mc.CG(i), t, x[i]));  // langevin.py:74-76 / mh.py:55
                    const float tp = xp[i] - pot.bb(i);
                    lr = fmaf(mc.KAP(i) * (t - tp), t + tp, lr);
                }
            } else {
                const auto ctx = pot.prepare(x, g, d);
#pragma unroll
                for (int i = 0; i < CPL; ++i)
                    xp[i] = fmaf(mc.C2(i), e[i], fmaf(mc.C1(i), pot.grad(ctx, i, x[i]), x[i]));  // langevin.py:74-76
                if (adjust) {
                    const auto ctxp = pot.prepare(xp, g, d);
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        const float gj = pot.grad(ctx, i, x[i]), gp = pot.grad(ctxp, i, xp[i]);
                        const float tf = (xp[i] - x[i]) + mc.HA(i) * gj;  // q(x'|x)  langevin.py:31-42
                        const float tb = (x[i] - xp[i]) + mc.HA(i) * gp;  // q(x|x')
                        lr += (pot.term(ctx, i, x[i]) - pot.term(ctxp, i, xp[i])) +
                              inv4h * mc.IA(i) * (tf * tf - tb * tb);
                    }
                }
            }
            // accept mask of the wave.  Each ballot takes one compare, so its v_cmp writes the mask directly (a ballot of a
            // combined bool went through a VGPR 0/1 and a compare back)
            uint64_t am = live;
            if (adjust) {
                // exact-fit path: the 8-lane stage as one DPP add (dpp_add_half_mirror), the same sum
                lr = group_allreduce<LPC, Pot<CPL, LPC, FAST>::kQuadratic && FAST>(lr);
                const float ln_u = au.draw(a.rng, gchain, row, n, g, s);
                am &= __ballot(ln_u < lr);  // NaN -> reject (langevin.py:106, mh.py:59)
                n_bad += (uint32_t)__popcll(__ballot(!(fabsf(lr) <= 3.0e38f)) & live & leaders);
            }
            n_acc += (uint32_t)__popcll(am & leaders);
            // mcmc/base.py:77.  Exact-fit path: x and the carried |x|^2 as moves under the accept mask (assign_where)
            if constexpr (Pot<CPL, LPC, FAST>::kQuadratic && FAST) assign_where<CPL>(am, x, xp, sq, sq_prop);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                if constexpr (!(Pot<CPL, LPC, FAST>::kQuadratic && FAST)) x[i] = select_f32(am, xp[i], x[i]);
                const float xs = shift(x, i);
                sx[i] += xs;
                sxx[i] = fmaf(xs, xs, sxx[i]);
            }
            if constexpr (!LEAN) {
                if (float* kept = keep.next(n * d)) store_row<CPL, LPC, FAST>(kept, row, d, g, active, x);
                if (g == 0 && active) {
                    if (a.masks_out) a.masks_out[(int64_t)s * n + row] = (am >> lane) & 1u;
                    if (a.log_ratio_out) a.log_ratio_out[(int64_t)s * n + row] = lr;
                }
            }
        }
        if constexpr (JHP > 0) {
            float lr;
            bool bad;
            fl.launder();
            const bool acc = jump_once<CPL, LPC, JHP>(x, fl, pot, jd, a.rng.seed, a.rng.step0 + (uint32_t)a.n_steps, gchain,
                                                      row, n, d, g, active, lr, bad);
            j_acc += (uint32_t)__popcll(__ballot(acc) & leaders);
            j_bad += (uint32_t)__popcll(__ballot(bad) & leaders);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const float xs = shift(x, i);
                sx[i] += xs;
                sxx[i] = fmaf(xs, xs, sxx[i]);
            }
            if (float* kept = keep.next(n * d)) store_row<CPL, LPC, FAST>(kept, row, d, g, active, x);
            if (g == 0 && active) {
                if (jd.mask_out) jd.mask_out[row] = acc ? 1 : 0;
                if (jd.log_ratio_out) jd.log_ratio_out[row] = lr;
            }
        }
        store_row<CPL, LPC, FAST>(a.x, row, d, g, active, x);
    }
    if (a.stats.sum_x) block_stats_flush<CPL, LPC>(sx, sxx, n_acc, n_bad, a.stats, j_acc, j_bad);
}

// ------------------------------------------------------------------------------------------------
template <int CPL, int LPC, template <int, int, bool> class Pot, bool FAST, int JHP, int RR = 10, bool TUNE = false>
__global__ void __launch_bounds__(kBlock, NFMC_WPE) hmc_kernel(NfmcHmcArgs a, int64_t tiles, JumpDev jd) {
    static_assert(!TUNE || (JHP == 0 && !FAST), "tuning launches run the general kernels without a jump tail");
    extern __shared__ __attribute__((aligned(16))) float flow_lds[];
    __shared__ float4 accept_slab[LPC > 1 ? kBlock : 1];
    constexpr int CPW = kWave / LPC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane % LPC, cw = lane / LPC;
    const int d = a.d;
    const int64_t n = a.n;
    const float h = a.tune.state ? (float)a.tune.state[NFMC_TUNE_STEP_SIZE] : a.step_size, hh = h / 2;

    MassCoef<CPL, LPC, FAST> mc;
    mc.init(h, 0.f, a.inv_mass_diag, g, d);
    Pot<CPL, LPC, FAST> pot;
    if constexpr (!Pot<CPL, LPC, FAST>::kStaged) pot.init(a.pot, g, d);
    FlowB<CPL, LPC, JHP == 0 ? 4 : JHP, true, (FAST && CPL >= 8 && JHP > 0)> fl;
    if constexpr (JHP > 0) {
        decltype(fl)::Img::stage(flow_lds, jd.flow, kBlock);
        __syncthreads();
        fl.init(flow_lds, jd.flow, g);
    }
    if constexpr (Pot<CPL, LPC, FAST>::kStaged)
        init_staged(pot, a.pot, g, d, flow_lds,
                    JHP > 0 ? decltype(fl)::Img::total_floats(jd.flow.n_hidden_layers, jd.flow.n_coupling) : 0);

    float sx[CPL], sxx[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) sx[i] = sxx[i] = 0.f;
    StatShift<CPL, LPC, TUNE> shift;
    Trajectory<CPL, LPC, TUNE> traj;
    traj.init(a.tune);
    uint32_t n_acc = 0, n_bad = 0, j_acc = 0, j_bad = 0;
    constexpr unsigned long long leaders = group_leaders(LPC);

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (tile * kWavesPerBlock + wave) * CPW + cw;
        const bool active = row < n;
        const uint32_t gchain = (uint32_t)(a.rng.chain_offset + (uint64_t)row);
        float x[CPL];
        load_row<CPL, LPC, FAST>(a.x, row, d, g, active, x);
        shift.init(a.tune, g, d, active);
        AcceptLnU<LPC, RR> au(accept_slab, g);
        StoreCursor keep(a.samples);

        for (int s = 0; s < a.n_steps; ++s) {
            float p[CPL], q[CPL];
            draw_normals<CPL, LPC, RR>(a.rng, kTagNoise, gchain, row, n, d, g, s, p);
            float dh = 0.f;  // this lane's share of H0 - H1
            {
                const auto ctx = pot.prepare(x, g, d);
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    p[i] *= mc.RS(i);  // hmc.py:100
                    q[i] = x[i];
                    dh += pot.term(ctx, i, x[i]) + 0.5f * (p[i] * p[i] * mc.M(i));  // hmc.py:103-106
                }
            }
            // hmc.py:67-71.  The reference's trajectory is L x [half step of p, full step of q, half step of p]; the closing
            // half step of one leapfrog step and the opening half step of the next use the SAME gradient (q has not moved),
            // so they are applied as one full step of p -- the textbook leapfrog, one gradient evaluation per position, the
            // same trajectory up to one rounding of p per step (the reference rounds twice).  Round 3: 3 -> 2 fused
            // multiply-adds per coordinate and leapfrog step on the exact-fit path (C5: hmc_kernel 100 -> 83 us per launch of 5 trajectories).
            if constexpr (Pot<CPL, LPC, FAST>::kQuadratic && FAST) {
                // scalar a, b = 0, unit mass: (h/2) grad U(q) = (h/2 * 2a) q
                const float cq = hh * (2.f * pot.aa(0)), cq2 = 2.f * cq;
                const int L = a.n_leapfrog;
                if (L > 0) {
#pragma unroll
                    for (int i = 0; i < CPL; ++i) p[i] = fmaf(-cq, q[i], p[i]);
                    for (int l = 0; l + 1 < L; ++l) {
#pragma unroll
                        for (int i = 0; i < CPL; ++i) {
                            q[i] = fmaf(h, p[i], q[i]);
                            p[i] = fmaf(-cq2, q[i], p[i]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        q[i] = fmaf(h, p[i], q[i]);
                        p[i] = fmaf(-cq, q[i], p[i]);
                    }
                }
            } else {
                const int L = traj.leapfrogs(a.n_leapfrog, a.rng.step0 + (uint32_t)s);
                if (L > 0) {
                    const auto c0 = pot.prepare(q, g, d);
#pragma unroll
                    for (int i = 0; i < CPL; ++i) p[i] = fmaf(-hh, pot.grad(c0, i, q[i]), p[i]);
                    for (int l = 0; l < L; ++l) {
#pragma unroll
                        for (int i = 0; i < CPL; ++i) q[i] = fmaf(h, p[i] * mc.M(i), q[i]);
                        const auto c1 = pot.prepare(q, g, d);
                        const float hs = l + 1 < L ? h : hh;
#pragma unroll
                        for (int i = 0; i < CPL; ++i) p[i] = fmaf(-hs, pot.grad(c1, i, q[i]), p[i]);
                    }
                }
            }
            bool accept = true;
            float lr = 0.f;
            if (a.adjust) {
                const auto ctx = pot.prepare(q, g, d);
#pragma unroll
                for (int i = 0; i < CPL; ++i) dh -= pot.term(ctx, i, q[i]) + 0.5f * (p[i] * p[i] * mc.M(i));  // :107-110
                lr = group_allreduce<LPC>(dh);
                accept = au.draw(a.rng, gchain, row, n, g, s) < lr;  // ln u < log r, hmc.py:111-113
                n_bad += (uint32_t)__popcll(__ballot(active && !(fabsf(lr) <= 3.0e38f)) & leaders);
            }
            traj.accumulate(x, q, p, shift, mc, lr, active);
            accept = accept && active;
            const uint64_t am = __ballot(accept);
            n_acc += (uint32_t)__popcll(am & leaders);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                x[i] = select_f32(am, q[i], x[i]);
                const float xs = shift(x, i);
                sx[i] += xs;
                sxx[i] = fmaf(xs, xs, sxx[i]);
            }
            if (float* kept = keep.next(n * d)) store_row<CPL, LPC, FAST>(kept, row, d, g, active, x);
            if (g == 0 && active) {
                if (a.masks_out) a.masks_out[(int64_t)s * n + row] = accept ? 1 : 0;
                if (a.log_ratio_out) a.log_ratio_out[(int64_t)s * n + row] = lr;
            }
        }
        if constexpr (JHP > 0) {
            float lr;
            bool bad;
            fl.launder();
            const bool acc = jump_once<CPL, LPC, JHP>(x, fl, pot, jd, a.rng.seed, a.rng.step0 + (uint32_t)a.n_steps, gchain,
                                                      row, n, d, g, active, lr, bad);
            j_acc += (uint32_t)__popcll(__ballot(acc) & leaders);
            j_bad += (uint32_t)__popcll(__ballot(bad) & leaders);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const float xs = shift(x, i);
                sx[i] += xs;
                sxx[i] = fmaf(xs, xs, sxx[i]);
            }
            if (float* kept = keep.next(n * d)) store_row<CPL, LPC, FAST>(kept, row, d, g, active, x);
            if (g == 0 && active) {
                if (jd.mask_out) jd.mask_out[row] = acc ? 1 : 0;
                if (jd.log_ratio_out) jd.log_ratio_out[row] = lr;
            }
        }
        store_row<CPL, LPC, FAST>(a.x, row, d, g, active, x);
    }
    if (a.stats.sum_x) {
        block_stats_flush<CPL, LPC>(sx, sxx, n_acc, n_bad, a.stats, j_acc, j_bad);
        traj.flush(a.stats);
    }
}


// ------------------------------------------------------------------------------------------------
// host-side launchers, one set per JHP (instantiated in sampler_j*.hip so the variants compile in parallel)
struct Cfg {
    int cpl, lpc;
};

// The layouts choose_cfg picks without the NFMC_SAMPLER_CFG override: the smallest capacity CPL * LPC >= d, at equal
// capacity the first in kCfgs.  (4, 16), (16, 4), (16, 8), (16, 16) and (16, 32) tie with an earlier layout and are
// reachable only through the override, which skips them for the kinds whose row in kPotKinds says default_cfg_only:
// their classes are not instantiated there.
constexpr bool is_default_cfg(int cpl, int lpc) {
    return !((cpl == 4 && lpc == 16) || (cpl == 16 && lpc != 64));
}
// whether sampler_{mala,hmc}_j*.hip hold kernels of `kind` at this layout and jump-tail width
template <int CPL, int LPC, int JHP>
constexpr bool cfg_instantiated(int kind) {
    return !pot_kind(kind)->own_units && (JHP > 0 || is_default_cfg(CPL, LPC) || !pot_kind(kind)->default_cfg_only);
}

// dynamic LDS of a launch: the jump tail's flow image, then the potential's block (the mixture's parameters / the tile
// of X or Lambda) behind it
template <int CPL, int LPC, int JHP>
size_t sampler_lds(const NfmcPotential& p, const JumpDev& jd) {
    size_t lds = 0;
    if constexpr (JHP > 0)
        lds = (size_t)FlowImage<CPL, LPC, JHP>::total_floats(jd.flow.n_hidden_layers, jd.flow.n_coupling) * sizeof(float);
    return lds_with_potential(lds, p, CPL, LPC);
}

template <int CPL, int LPC, template <int, int, bool> class POT, bool F, int JHP>
int launch_mala_kernel(const NfmcMalaArgs& a, const JumpDev& jd, size_t lds, int64_t tiles, int grid, float sqrt2h,
                       hipStream_t st) {
    auto kern = mala_kernel<CPL, LPC, POT, F, JHP>;
    if constexpr (JHP == 0 && !F) {
        if (a.tune.state) kern = mala_kernel<CPL, LPC, POT, F, JHP, 10, false, true>;
    }
    return launch_lds(kern, grid, kBlock, lds, st, a, sqrt2h, tiles, jd);
}

template <int CPL, int LPC, template <int, int, bool> class POT, bool F, int JHP>
int launch_hmc_kernel(const NfmcHmcArgs& a, const JumpDev& jd, size_t lds, int64_t tiles, int grid, hipStream_t st) {
    auto kern = hmc_kernel<CPL, LPC, POT, F, JHP>;
    if constexpr (JHP == 0 && !F) {
        if (a.tune.state) kern = hmc_kernel<CPL, LPC, POT, F, JHP, 10, true>;
    }
    return launch_lds(kern, grid, kBlock, lds, st, a, tiles, jd);
}

// kinds 0 to 3 at one layout and jump-tail width (launch_{mala,hmc}_j*): the class, and FAST where it has such kernels.
// The units that instantiate these include pot_basic.hpp; here the classes are names only.
template <int CPL, int LPC, bool FAST> struct QuadraticPot;
template <int CPL, int LPC, bool FAST> struct FunnelPot;
template <int CPL, int LPC, bool FAST> struct MixturePot;
template <int CPL, int LPC, bool FAST> struct LogRegPot;
template <int CPL, int LPC, int JHP>
int launch_mala_cfg(const NfmcMalaArgs& a, const JumpDev& jd, bool fast, int64_t tiles, int grid, float sqrt2h,
                    hipStream_t st) {
    const size_t lds = sampler_lds<CPL, LPC, JHP>(a.pot, jd);
    if (lds > 120 * 1024 || !cfg_instantiated<CPL, LPC, JHP>(a.pot.kind)) return NFMC_EUNSUPPORTED;
    // no per-step output and no replay: the FAST quadratic kernels without a jump tail have a LEAN instantiation
    const bool lean = !a.masks_out && !a.log_ratio_out && !a.samples.base && !a.rng.replay_normals && !a.rng.replay_uniforms;
#define NFMC_L(POT, F) return launch_mala_kernel<CPL, LPC, POT, F, JHP>(a, jd, lds, tiles, grid, sqrt2h, st);
    if (rng_rounds(a.rng) == 7) {   // opt-in Philox4x32-7 stream: the exact-fit quadratic kernel without a jump tail
        if constexpr (JHP == 0) {
            if (fast && a.pot.kind == NFMC_POT_QUADRATIC) {
                auto kern = lean ? mala_kernel<CPL, LPC, QuadraticPot, true, 0, 7, true>
                                 : mala_kernel<CPL, LPC, QuadraticPot, true, 0, 7>;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, a, sqrt2h, tiles, jd);
                return NFMC_OK;
            }
        }
        return NFMC_EUNSUPPORTED;
    }
    if (a.pot.kind == NFMC_POT_GAUSSIAN_MIXTURE) {   // never exact-fit: a and b are tables
        NFMC_L(MixturePot, false)
    } else if (a.pot.kind == NFMC_POT_LOGISTIC_REGRESSION) {
        if constexpr (cfg_instantiated<CPL, LPC, JHP>(NFMC_POT_LOGISTIC_REGRESSION)) NFMC_L(LogRegPot, false)
    } else if (a.pot.kind == NFMC_POT_FUNNEL) {
        if (fast) NFMC_L(FunnelPot, true) else NFMC_L(FunnelPot, false)
    } else {
        if constexpr (JHP == 0) {
            if (fast && lean) {
                auto kern = mala_kernel<CPL, LPC, QuadraticPot, true, 0, 10, true>;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, a, sqrt2h, tiles, jd);
                return NFMC_OK;
            }
        }
        if (fast) NFMC_L(QuadraticPot, true) else NFMC_L(QuadraticPot, false)
    }
#undef NFMC_L
    return NFMC_EUNSUPPORTED;
}

template <int CPL, int LPC, int JHP>
int launch_hmc_cfg(const NfmcHmcArgs& a, const JumpDev& jd, bool fast, int64_t tiles, int grid, hipStream_t st) {
    const size_t lds = sampler_lds<CPL, LPC, JHP>(a.pot, jd);
    if (lds > 120 * 1024 || !cfg_instantiated<CPL, LPC, JHP>(a.pot.kind)) return NFMC_EUNSUPPORTED;
#define NFMC_L(POT, F) return launch_hmc_kernel<CPL, LPC, POT, F, JHP>(a, jd, lds, tiles, grid, st);
    if (rng_rounds(a.rng) == 7) {
        if constexpr (JHP == 0) {
            if (fast && a.pot.kind == NFMC_POT_QUADRATIC) {
                auto kern = hmc_kernel<CPL, LPC, QuadraticPot, true, 0, 7>;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, a, tiles, jd);
                return NFMC_OK;
            }
        }
        return NFMC_EUNSUPPORTED;
    }
    if (a.pot.kind == NFMC_POT_GAUSSIAN_MIXTURE) {   // never exact-fit: a and b are tables
        NFMC_L(MixturePot, false)
    } else if (a.pot.kind == NFMC_POT_LOGISTIC_REGRESSION) {
        if constexpr (cfg_instantiated<CPL, LPC, JHP>(NFMC_POT_LOGISTIC_REGRESSION)) NFMC_L(LogRegPot, false)
    } else if (a.pot.kind == NFMC_POT_FUNNEL) {
        if (fast) NFMC_L(FunnelPot, true) else NFMC_L(FunnelPot, false)
    } else {
        if (fast) NFMC_L(QuadraticPot, true) else NFMC_L(QuadraticPot, false)
    }
#undef NFMC_L
    return NFMC_EUNSUPPORTED;
}

// all sampler layouts (kCfgs, sampler_kernels.hip)
#define NFMC_FOR_CFG(M)                                                                                             \
    M(4, 1) M(4, 2) M(4, 4) M(4, 8) M(4, 16) M(8, 8) M(16, 4) M(8, 16) M(16, 8) M(8, 32) M(16, 16) M(8, 64) M(16, 32) \
        M(16, 64)
// the layouts choose_cfg picks by default (is_default_cfg) among NFMC_FOR_CFG
#define NFMC_FOR_DEFAULT_CFG(M) M(4, 1) M(4, 2) M(4, 4) M(4, 8) M(8, 8) M(8, 16) M(8, 32) M(8, 64) M(16, 64)
// the samplers' jump-tail layouts (JHP > 0), in choose_cfg's order of preference: kJumpCfgs is this list
#define NFMC_FOR_JUMP_CFG(M) M(4, 1) M(4, 2) M(4, 4) M(4, 8) M(8, 8) M(8, 16) M(8, 32) M(8, 64)
#define NFMC_CFG_ENTRY(CPL, LPC) {CPL, LPC},
constexpr Cfg kJumpCfgs[] = {NFMC_FOR_JUMP_CFG(NFMC_CFG_ENTRY)};

// The own_units kinds (kPotKinds): every layout and jump-tail width of one class in a translation unit of its own
// (the sampler_<kind>_{mala,hmc}.hip of NFMC_FOR_OWN_UNIT_POT instantiate these explicitly), the layouts kind 3 gets, general
// kernels on the default Philox4x32-10 stream only
template <template <int, int, bool> class POT>
int launch_mala_kind(const NfmcMalaArgs& a, const JumpDev& jd, Cfg c, int jhp, int64_t tiles, int grid, float sqrt2h,
                     hipStream_t st) {
    if (rng_rounds(a.rng) != 10) return NFMC_EUNSUPPORTED;
#define NFMC_AT(JHP, CPL, LPC)                                                       \
    if (jhp == JHP && c.cpl == CPL && c.lpc == LPC) {                                \
        const size_t lds = sampler_lds<CPL, LPC, JHP>(a.pot, jd);                    \
        if (lds > 120 * 1024) return NFMC_EUNSUPPORTED;                              \
        return launch_mala_kernel<CPL, LPC, POT, false, JHP>(a, jd, lds, tiles, grid, sqrt2h, st); \
    }
#define M0(CPL, LPC) NFMC_AT(0, CPL, LPC)
#define M4(CPL, LPC) NFMC_AT(4, CPL, LPC)
#define M8(CPL, LPC) NFMC_AT(8, CPL, LPC)
    NFMC_FOR_DEFAULT_CFG(M0) NFMC_FOR_JUMP_CFG(M4) NFMC_FOR_JUMP_CFG(M8)
#undef NFMC_AT
    return NFMC_EUNSUPPORTED;
}
template <template <int, int, bool> class POT>
int launch_hmc_kind(const NfmcHmcArgs& a, const JumpDev& jd, Cfg c, int jhp, int64_t tiles, int grid, hipStream_t st) {
    if (rng_rounds(a.rng) != 10) return NFMC_EUNSUPPORTED;
#define NFMC_AT(JHP, CPL, LPC)                                                       \
    if (jhp == JHP && c.cpl == CPL && c.lpc == LPC) {                                \
        const size_t lds = sampler_lds<CPL, LPC, JHP>(a.pot, jd);                    \
        if (lds > 120 * 1024) return NFMC_EUNSUPPORTED;                              \
        return launch_hmc_kernel<CPL, LPC, POT, false, JHP>(a, jd, lds, tiles, grid, st); \
    }
    NFMC_FOR_DEFAULT_CFG(M0) NFMC_FOR_JUMP_CFG(M4) NFMC_FOR_JUMP_CFG(M8)
#undef NFMC_AT
#undef M0
#undef M4
#undef M8
    return NFMC_EUNSUPPORTED;
}
// the dispatching unit (sampler_kernels.hip) does not instantiate them, and so none of their kernels, itself
#define NFMC_EXTERN_KIND(KIND, POT)                                                                                       \
    static_assert(kPotKinds[KIND].own_units, #POT);                                                                       \
    extern template int launch_mala_kind<POT>(const NfmcMalaArgs&, const JumpDev&, Cfg, int, int64_t, int, float, hipStream_t); \
    extern template int launch_hmc_kind<POT>(const NfmcHmcArgs&, const JumpDev&, Cfg, int, int64_t, int, hipStream_t);
NFMC_FOR_OWN_UNIT_POT(NFMC_EXTERN_KIND)
#undef NFMC_EXTERN_KIND

// defined in sampler_mala_j*.hip / sampler_hmc_j*.hip: kinds 0 to 3
int launch_mala_j0(const NfmcMalaArgs&, const JumpDev&, Cfg, bool, int64_t, int, float, hipStream_t);
int launch_mala_j4(const NfmcMalaArgs&, const JumpDev&, Cfg, bool, int64_t, int, float, hipStream_t);
int launch_mala_j8(const NfmcMalaArgs&, const JumpDev&, Cfg, bool, int64_t, int, float, hipStream_t);
int launch_hmc_j0(const NfmcHmcArgs&, const JumpDev&, Cfg, bool, int64_t, int, hipStream_t);
int launch_hmc_j4(const NfmcHmcArgs&, const JumpDev&, Cfg, bool, int64_t, int, hipStream_t);
int launch_hmc_j8(const NfmcHmcArgs&, const JumpDev&, Cfg, bool, int64_t, int, hipStream_t);

}  // namespace nfmc
