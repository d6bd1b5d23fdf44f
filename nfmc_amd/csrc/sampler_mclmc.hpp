// Microcanonical Langevin Monte Carlo (NfmcMclmcArgs, nfmc_hip.h): n_steps fused steps B(eps/2) A(eps) B(eps/2) O per
// chain on the register layout of the mala / hmc kernels, over the same potential classes (prepare / grad / term).
//
// Per chain and launch the registers hold x, the unit velocity u, grad U(x) and U(x): the second B of a step and the
// first B of the next use the same gradient (O does not move x), so a step costs ONE prepare(), one gradient and one
// value; the launch evaluates both once on entry.  Reductions over the chain's lanes per step: three per B (|sigma g|^2
// and u . sigma g side by side, then |uu|^2), one for U(x') and one for |u + nu z|^2: eight butterflies, against one in
// a mala transition.  There is no accept / reject; a step whose energy error or new state is not finite is not taken,
// by selects under one wave mask: prepare() stays in workgroup-uniform control flow (LogRegPot's rule, pot_kinds.hpp).
// General kernels only: Philox4x32-10, the default layouts, no jump tail.
#pragma once

#include "sampler_impl.hpp"

namespace nfmc {

// B(e) on the lanes of one chain: u <- the velocity after a kick of length e along -sigma g, returns dK.  sig is 0 on the
// padded coordinates, so they enter neither norm nor dot product and their u stays 0.  dm1 = d - 1.
// log(1 + ue + (1 - ue) zeta^2) - ln 2 is evaluated as log1p(-(1 - ue)(1 - zeta)(1 + zeta) / 2): the same value without the
// cancellation against ln 2, which costs (d - 1) ulps of 1 at small e.
template <int CPL, int LPC>
__device__ __forceinline__ float mclmc_kick(float (&u)[CPL], const float (&gr)[CPL], const float (&sig)[CPL], float e,
                                            float dm1) {
    float gt[CPL], a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        gt[i] = sig[i] * gr[i];
        a = fmaf(gt[i], gt[i], a);
        b = fmaf(u[i], gt[i], b);
    }
    a = group_allreduce<LPC>(a);
    b = group_allreduce<LPC>(b);
    const float gn = sqrtf(a);
    const bool still = gn == 0.f;   // no force: u unchanged, dK = 0 (a NaN norm goes through and voids the step)
    const float inv = 1.f / gn;
    const float ue = -b * inv;
    const float delta = e * gn / dm1;
    const float zeta = expf(-delta), omz = -expm1f(-delta);
    const float c = omz * (1.f + zeta + ue * omz), tz = 2.f * zeta;
    float uu[CPL], s = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        uu[i] = fmaf(-(gt[i] * inv), c, tz * u[i]);
        s = fmaf(uu[i], uu[i], s);
    }
    s = group_allreduce<LPC>(s);
    const float rn = 1.f / sqrtf(s);
#pragma unroll
    for (int i = 0; i < CPL; ++i) u[i] = still ? u[i] : uu[i] * rn;
    const float dk = dm1 * (delta + log1pf(-0.5f * (1.f - ue) * omz * (1.f + zeta)));
    return still ? 0.f : dk;
}

// A launch with a tuning state sums x about the state's shift words (StatShift, laid out as in NfmcTune's state) and
// reads eps and L from it; without one the shift is zero and x - 0 is x.
template <int CPL, int LPC, template <int, int, bool> class Pot>
__global__ void __launch_bounds__(kBlock, NFMC_WPE) mclmc_kernel(NfmcMclmcArgs a, int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float flow_lds[];
    constexpr int CPW = kWave / LPC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane % LPC, cw = lane / LPC;
    const int d = a.d;
    const int64_t n = a.n;
    const bool tuning = a.tune.state != nullptr;
    const float eps = tuning ? (float)a.tune.state[NFMC_MCLMC_STEP_SIZE] : a.step_size, he = 0.5f * eps;
    const float len = tuning ? (float)a.tune.state[NFMC_MCLMC_DECOHERENCE_LENGTH] : a.decoherence_length;
    const float nu = (float)sqrt(expm1(2.0 * (double)eps / (double)len) / (double)d);
    const float dm1 = (float)(d - 1);

    float sig[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = coord_of<CPL, LPC>(g, i);
        sig[i] = c < d ? (a.inv_mass_diag ? sqrtf(a.inv_mass_diag[c]) : 1.f) : 0.f;
    }
    Pot<CPL, LPC, false> pot;
    if constexpr (!Pot<CPL, LPC, false>::kStaged) pot.init(a.pot, g, d);
    else init_staged(pot, a.pot, g, d, flow_lds, 0);

    float sx[CPL], sxx[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) sx[i] = sxx[i] = 0.f;
    StatShift<CPL, LPC, true> shift;
    NfmcTune shift_src = {};
    shift_src.state = a.tune.state;
    uint32_t n_acc = 0, n_bad = 0;
    double se2 = 0.0, se = 0.0;   // this chain's sums of finite dE^2 and dE over the launch (every lane of the chain)
    constexpr unsigned long long leaders = group_leaders(LPC);
    const uint64_t mine = (LPC == 64 ? ~0ull : ((1ull << (LPC & 63)) - 1ull)) << (lane - g);   // the chain's lanes

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (tile * kWavesPerBlock + wave) * CPW + cw;
        const bool active = row < n;
        const uint32_t gchain = (uint32_t)(a.rng.chain_offset + (uint64_t)row);
        float x[CPL], u[CPL], gr[CPL];
        load_row<CPL, LPC, false>(a.x, row, d, g, active, x);
        load_row<CPL, LPC, false>(a.velocity, row, d, g, active, u);
        shift.init(shift_src, g, d, active && tuning);
        StoreCursor keep(a.samples);
        float U = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) gr[i] = 0.f;

        // Pass -1 is the launch's own evaluation of grad U and U at its starting x.  It goes through the step's ONE
        // evaluation site, so a run cut into launches computes bitwise what one launch computes, dE included: a second
        // site is compiled apart (packed or fused differently) and U(x) from it differed in the last bit.
#pragma clang loop unroll(disable)
        for (int s = -1; s < a.n_steps; ++s) {
            const bool entry = s < 0;
            float u0[CPL], xn[CPL], gn[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) u0[i] = u[i];
            float dk1 = 0.f;
            if (!entry) dk1 = mclmc_kick<CPL, LPC>(u, gr, sig, he, dm1);
            bool wild = false;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                xn[i] = entry ? x[i] : fmaf(eps * sig[i], u[i], x[i]);
                wild = wild || !(fabsf(xn[i]) <= 3.0e38f);
            }
            float un;
            {
                const auto ctx = pot.prepare(xn, g, d);
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    gn[i] = pot.grad(ctx, i, xn[i]);
                    part += pot.term(ctx, i, xn[i]);
                }
                un = group_allreduce<LPC>(part);
            }
            if (entry) {
#pragma unroll
                for (int i = 0; i < CPL; ++i) gr[i] = gn[i];
                U = un;
                continue;
            }
            const float dk2 = mclmc_kick<CPL, LPC>(u, gn, sig, he, dm1);
            const float de = (un - U) + dk1 + dk2;
            const bool ok = active && fabsf(de) <= 3.0e38f && (__ballot(wild) & mine) == 0;
            const uint64_t om = __ballot(ok);
            n_acc += (uint32_t)__popcll(__ballot(active) & leaders);
            n_bad += (uint32_t)__popcll(__ballot(active && !ok) & leaders);
            const double dee = ok ? (double)de : 0.0;
            se2 = fma(dee, dee, se2);
            se += dee;
            U = ok ? un : U;
            // O, from the velocity the step left or, for a step not taken, from the one it started with
            float z[CPL], w[CPL], ss = 0.f;
            draw_normals<CPL, LPC>(a.rng, kTagNoise, gchain, row, n, d, g, s, z);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                x[i] = select_f32(om, xn[i], x[i]);
                gr[i] = select_f32(om, gn[i], gr[i]);
                const float ui = select_f32(om, u[i], u0[i]);
                w[i] = coord_of<CPL, LPC>(g, i) < d ? fmaf(nu, z[i], ui) : 0.f;
                ss = fmaf(w[i], w[i], ss);
                const float xs = shift(x, i);
                sx[i] += xs;
                sxx[i] = fmaf(xs, xs, sxx[i]);
            }
            ss = group_allreduce<LPC>(ss);
            const float rn = 1.f / sqrtf(ss);
#pragma unroll
            for (int i = 0; i < CPL; ++i) u[i] = w[i] * rn;
            if (float* kept = keep.next(n * d)) store_row<CPL, LPC, false>(kept, row, d, g, active, x);
            if (a.energy_out && g == 0 && active) a.energy_out[(int64_t)s * n + row] = de;
        }
        store_row<CPL, LPC, false>(a.x, row, d, g, active, x);
        store_row<CPL, LPC, false>(a.velocity, row, d, g, active, u);
    }
    if (a.stats.sum_x) {
        block_stats_flush<CPL, LPC>(sx, sxx, n_acc, n_bad, a.stats);
        // The energy sums ride in the two jump columns of the workgroup's slab, which a launch without a jump tail leaves
        // zero (as Trajectory::flush does): fp64 sums of the group leaders', in a fixed order.
        __shared__ double tail[kWavesPerBlock][2];
        const double w2 = cross_chain_reduce_f64<LPC>(se2);
        const double w1 = cross_chain_reduce_f64<LPC>(se);
        if (lane == 0) {
            tail[wave][0] = w2;
            tail[wave][1] = w1;
        }
        __syncthreads();   // also orders the owner threads' stores of the two columns before the stores below
        if (threadIdx.x == 0) {
            double s2 = 0.0, s1 = 0.0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) {
                s2 += tail[w][0];
                s1 += tail[w][1];
            }
            double* out = a.stats.scratch + (size_t)blockIdx.x * (2 * CPL * LPC + kStatTail) + 2 * CPL * LPC;
            out[2] = s2;
            out[3] = s1;
        }
    }
}

template <int CPL, int LPC, template <int, int, bool> class POT>
int launch_mclmc_kernel(const NfmcMclmcArgs& a, int64_t tiles, int grid, hipStream_t st) {
    const size_t lds = lds_with_potential(0, a.pot, CPL, LPC);
    if (lds > 120 * 1024) return NFMC_EUNSUPPORTED;
    return launch_lds(mclmc_kernel<CPL, LPC, POT>, grid, kBlock, lds, st, a, tiles);
}

// every default layout of one class: the own_units kinds instantiate it explicitly in their sampler_<kind>_hmc.hip, kinds 0
// to 3 through launch_mclmc_j0 in sampler_hmc_j0.hip
template <template <int, int, bool> class POT>
int launch_mclmc_kind(const NfmcMclmcArgs& a, Cfg c, int64_t tiles, int grid, hipStream_t st) {
#define NFMC_AT(CPL, LPC) \
    if (c.cpl == CPL && c.lpc == LPC) return launch_mclmc_kernel<CPL, LPC, POT>(a, tiles, grid, st);
    NFMC_FOR_DEFAULT_CFG(NFMC_AT)
#undef NFMC_AT
    return NFMC_EUNSUPPORTED;
}
#define NFMC_EXTERN_KIND(KIND, POT) \
    extern template int launch_mclmc_kind<POT>(const NfmcMclmcArgs&, Cfg, int64_t, int, hipStream_t);
NFMC_FOR_OWN_UNIT_POT(NFMC_EXTERN_KIND)
#undef NFMC_EXTERN_KIND

int launch_mclmc_j0(const NfmcMclmcArgs&, Cfg, int64_t, int, hipStream_t);   // sampler_hmc_j0.hip: kinds 0 to 3

}  // namespace nfmc
