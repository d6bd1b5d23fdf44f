// flow_mh_b_kernel: the flow-proposal Metropolis transitions of flow_b_kernels.hip, in a header of its own so that the
// instantiations of the own_units kinds (kPotKinds, pot_kinds.hpp) compile in translation units of their own.
#pragma once

#include "flow_b.hpp"
#include "pot_shared.hpp"

namespace nfmc {

// DIAG = false is the production instantiation: no replayed noise, no sample store, no mask / log-ratio outputs --
// the branches on those pointers (and the scalar registers that carry them through the tile loop: the DIAG kernel
// spills SGPRs into VGPR lanes there) are compiled out.  The host picks it when all of those arguments are NULL.
// NB = 8: rational-quadratic spline couplings ('c-rqnsf') on the same skeleton (round 3; before, spline flows ran the jump on
// the one-chain-per-lane kernel of flow_kernels.hip only).
// WPE: the waves per SIMD that the register allocation has to leave room for (the occupancy argument of
// __launch_bounds__).  1, the default, is the rich schedule that wins when the kernel has the SIMDs to itself; the lean
// forms of the pipelined jump (flow_b_lean.hip) ask for more, so that their waves fit beside the inner kernel's, fence
// the flow's weight loads (FlowB LEAN), form lane addresses and Philox block numbers where they are used instead of
// holding them across the loops, and raise their waves' issue priority.  None of that changes a floating-point
// operation, its operands or the order of the operations of a chain.
#ifndef NFMC_FLOWB_WPE
#define NFMC_FLOWB_WPE 1
#endif
#ifndef NFMC_FLOWB_LEAN_PRIO
#define NFMC_FLOWB_LEAN_PRIO 3   // s_setprio of the lean forms (0 .. 3; every other kernel of the library runs at 0)
#endif
template <int CPL, int LPC, int HP, template <int, int, bool> class Pot, bool FAST, bool DIAG, int RR = 10, int NB = 0,
          int WPE = NFMC_FLOWB_WPE>
__global__ void __launch_bounds__(kBlock, WPE) flow_mh_b_kernel(NfmcFlowMhArgs a, int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int CPW = kWave / LPC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane % LPC, cw = lane / LPC;
    const int d = a.flow.d;
    const int64_t n = a.n;
    // The lean forms run beside another kernel's waves, which were there first.  At equal priority the SIMD issues the
    // older wave and the younger gets the slots it leaves: beside four MALA waves at 0.9 VALU busy the C3 jump took the
    // whole inner launch (105 us for 12 us of issue) and kept the other part's inner launch waiting behind it.
    if constexpr (WPE > 1) __builtin_amdgcn_s_setprio(NFMC_FLOWB_LEAN_PRIO);
    using Flow = FlowB<CPL, LPC, HP, (WPE > 1), (FAST && CPL >= 8), NB>;   // WPE > 1: no weight loads hoisted en bloc
    Flow::Img::stage(lds, a.flow, kBlock);
    __syncthreads();
    Flow fl;
    fl.init(lds, a.flow, g);
    Pot<CPL, LPC, FAST> pot;
    if constexpr (Pot<CPL, LPC, FAST>::kStaged)
        init_staged(pot, a.pot, g, d, lds, Flow::Img::total_floats(a.flow.n_hidden_layers, a.flow.n_coupling));
    else
        pot.init(a.pot, g, d);
    const bool revl = (a.flow.n_coupling & 1) != 0;
    const float base_c = -0.5f * (float)d * kLog2Pi;

    float sx[CPL], sxx[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) sx[i] = sxx[i] = 0.f;
    uint32_t n_acc = 0, n_bad = 0;
    constexpr unsigned long long leaders = group_leaders(LPC);

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (tile * kWavesPerBlock + wave) * CPW + cw;
        const bool active = row < n;
        const uint32_t gchain = (uint32_t)(a.rng.chain_offset + (uint64_t)row);
        float x[CPL];
        int gr = g;   // lean forms: the lane's address in the row is formed per tile (not held in a VGPR pair across the loop)
        if constexpr (WPE > 1) asm volatile("" : "+v"(gr));
        load_row<CPL, LPC, FAST>(a.x, row, d, gr, active, x);
        float u_x;
        {
            const auto ctx = pot.prepare(x, g, d);
            float up = 0.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i) up += pot.term(ctx, i, x[i]);
            u_x = group_allreduce<LPC>(up);                                  // jump.py:212 / imh.py:224
        }
        float f_x;
        if (a.logq_cached) {
            f_x = active ? a.logq[row] : 0.f;
        } else {                                                             // flow.log_prob(x): jump.py:218 / imh.py:214
            float w[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) w[i] = x[i];
            float part = fl.forward(w);
#pragma unroll
            for (int i = 0; i < CPL; ++i) part = fmaf(-0.5f * w[i], w[i], part);
            f_x = group_allreduce<LPC>(part) + base_c;
        }
        StoreCursor keep(a.samples);
        for (int s = 0; s < a.n_steps; ++s) {
            float xp[CPL];
            // lean forms: the lane's Philox block numbers are formed anew for every transition.  Left visible, the first
            // round's products of the (loop-invariant) block numbers are hoisted out of the tile loop and held in 4 VGPRs
            // per block through the whole flow pass.
            int gl = g;
            if constexpr (WPE > 1) asm volatile("" : "+v"(gl));
            draw_latent<CPL, LPC, FAST, RR>(xp, (DIAG && a.rng.replay_normals) ? a.rng.replay_normals + (int64_t)s * n * d : nullptr, a.rng.seed,
                                  a.rng.step0 + (uint32_t)s, gchain, row, n, d, gl, revl);  // flow.sample: jump.py:205 / imh.py:221
            float part = 0.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i) part = fmaf(-0.5f * xp[i], xp[i], part);
            part -= fl.inverse(xp);
            const float f_xp = group_allreduce<LPC>(part) + base_c;
            float up = 0.f;
            {
                const auto ctx = pot.prepare(xp, g, d);
#pragma unroll
                for (int i = 0; i < CPL; ++i) up += pot.term(ctx, i, xp[i]);
            }
            const float u_xp = group_allreduce<LPC>(up);                     // jump.py:213 / imh.py:225
            const float lr = (-u_xp) - (-u_x) + f_x - f_xp;                  // util.py:392
            bool accept = true;
            if (a.adjusted) {
                float u;
                if (DIAG && a.rng.replay_uniforms) {
                    u = active ? a.rng.replay_uniforms[(int64_t)s * n + row] : 0.5f;
                } else {
                    const uint4 r = philox4x32<RR>(gchain, a.rng.step0 + (uint32_t)s, 0u, kTagJump, (uint32_t)a.rng.seed,
                                                  (uint32_t)(a.rng.seed >> 32));
                    u = u32_to_uniform(r.x);
                }
                accept = fast_ln(u) < lr;                                     // jump.py:225 / imh.py:229-230
                n_bad += (uint32_t)__popcll(__ballot(active && !(fabsf(lr) <= 3.0e38f)) & leaders);
            }
            accept = accept && active;
            const uint64_t am = __ballot(accept);
            n_acc += (uint32_t)__popcll(am & leaders);
            f_x = select_f32(am, f_xp, f_x);
            u_x = select_f32(am, u_xp, u_x);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                x[i] = select_f32(am, xp[i], x[i]);                                // jump.py:231 / imh.py:232-233
                sx[i] += x[i];
                sxx[i] = fmaf(x[i], x[i], sxx[i]);
            }
            if constexpr (DIAG) {
                if (float* kept = keep.next(n * d)) store_row<CPL, LPC, FAST>(kept, row, d, g, active, x);
            }
            if (DIAG && g == 0 && active) {
                if (a.masks_out) a.masks_out[(int64_t)s * n + row] = accept ? 1 : 0;
                if (a.log_ratio_out) a.log_ratio_out[(int64_t)s * n + row] = lr;
            }
        }
        int gs = g;   // lean forms: the lane's address in the row is formed again here, not held from the load on
        if constexpr (WPE > 1) asm volatile("" : "+v"(gs));
        store_row<CPL, LPC, FAST>(a.x, row, d, gs, active, x);
        if (g == 0 && active) a.logq[row] = f_x;
    }
    if (a.stats.sum_x) block_stats_flush<CPL, LPC>(sx, sxx, n_acc, n_bad, a.stats);
}

// the register layouts (CPL, LPC) of the flow-MH kernels, in flow_mh_b_launch's order of preference: kFlowBCfgs is
// this list.  (Not the samplers' jump-tail layouts, NFMC_FOR_JUMP_CFG in sampler_impl.hpp.)
struct BCfg {
    int cpl, lpc;
};
#define NFMC_FOR_FLOWB_CFG(M) M(4, 1) M(4, 2) M(4, 4) M(4, 8) M(8, 8) M(4, 16) M(8, 16) M(4, 32) M(8, 32) M(4, 64) M(8, 64)
#define NFMC_BCFG_ENTRY(CPL, LPC) {CPL, LPC},
constexpr BCfg kFlowBCfgs[] = {NFMC_FOR_FLOWB_CFG(NFMC_BCFG_ENTRY)};

// The register-lean forms of the exact-fit quadratic one-chain kernel (flow_b_lean.hip): a part of a
// split run (run_parts.hpp) launches its jump on them, so that several jump waves fit into the registers that the
// inner kernel's waves of the other part leave of a SIMD's 512.
// lean_wpe: the WPE of the lean form of layout c at conditioner bucket hp, 0 when the layout has none.
// launch_b_lean: that form (diag: with the diagnostics compiled in); arguments and NFMC_EUNSUPPORTED / dry as in
// flow_mh_b_launch.
int lean_wpe(BCfg c, int hp);
int launch_b_lean(const NfmcFlowMhArgs& a, BCfg c, int hp, bool diag, int64_t tiles, int grid, hipStream_t st, bool dry);

// The own_units kinds (kPotKinds): class POT at layout c, conditioner bucket hp (4 / 8), affine (NB = 0) or spline
// (NB = kRqsBins) couplings; one general kernel (diagnostics compiled in, default stream) per layout and width.  The
// arguments and NFMC_EUNSUPPORTED / dry as in flow_mh_b_launch.  Never exact-fit or dual: their parameters are tables.
// The flow_b_<kind>{,_rqs}.hip of NFMC_FOR_OWN_UNIT_POT instantiate it explicitly.
template <template <int, int, bool> class POT, int NB>
int launch_b_kind(const NfmcFlowMhArgs& a, BCfg c, int hp, int64_t tiles, int grid, hipStream_t st, bool dry) {
    if (rng_rounds(a.rng) != 10) return NFMC_EUNSUPPORTED;
#define NFMC_AT(HP, CPL, LPC)                                                                                          \
    if (hp == HP && c.cpl == CPL && c.lpc == LPC) {                                                                    \
        const size_t img = (size_t)FlowImage<CPL, LPC, HP, false, NB>::total_floats(a.flow.n_hidden_layers, a.flow.n_coupling) * \
                           sizeof(float);                                                                              \
        const size_t lds = lds_with_potential(img, a.pot, CPL, LPC);                                                  \
        if (lds > 120 * 1024) return NFMC_EUNSUPPORTED;                                                                \
        return dry ? NFMC_OK : launch_lds(flow_mh_b_kernel<CPL, LPC, HP, POT, false, true, 10, NB>, grid, kBlock, lds, st, a, tiles); \
    }
#define M4(CPL, LPC) NFMC_AT(4, CPL, LPC)
#define M8(CPL, LPC) NFMC_AT(8, CPL, LPC)
    NFMC_FOR_FLOWB_CFG(M4) NFMC_FOR_FLOWB_CFG(M8)
#undef NFMC_AT
#undef M4
#undef M8
    return NFMC_EUNSUPPORTED;
}
// the dispatching unit (flow_b_kernels.hip) does not instantiate them, and so none of their kernels, itself
#define NFMC_EXTERN_KIND(KIND, POT)                                                                                  \
    static_assert(kPotKinds[KIND].own_units, #POT);                                                                  \
    extern template int launch_b_kind<POT, 0>(const NfmcFlowMhArgs&, BCfg, int, int64_t, int, hipStream_t, bool);    \
    extern template int launch_b_kind<POT, kRqsBins>(const NfmcFlowMhArgs&, BCfg, int, int64_t, int, hipStream_t, bool);
NFMC_FOR_OWN_UNIT_POT(NFMC_EXTERN_KIND)
#undef NFMC_EXTERN_KIND

}  // namespace nfmc
