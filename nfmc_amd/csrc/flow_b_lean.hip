// Lean forms of the flow-MH kernel, for the jump of a split run (nfmc_jump_run_f32 with parts).
//
// flow_mh_b_kernel is compiled for one wave per SIMD: nothing makes the compiler economise, and the exact-fit quadratic
// kernel takes 116 VGPRs at (8, 8).  Alone that is the faster schedule.  In a split run the jump of one part runs beside
// the inner kernel of the other, whose waves were there first: the forms here are the same kernel with an occupancy
// bound (WPE, flow_b_mh.hpp), so that two of its waves fit beside the inner waves (table below), and with a raised issue
// priority, so that the jump does not live on the issue slots the inner waves leave.  Same operations on the same
// operands in the same order per chain: tests/test_gpu_flow_mh_lean.py compares every output for equality.
//
//   form (CPL, LPC, HP, WPE)   VGPRs   beside                                              budget
//   (8, 8, 4, 5)               96      4 waves of mala_kernel<8, 8, ..., LEAN> (80 each)   (512 - 4 * 80) / 2 = 96
//
// tests/test_host_flow_mh_lean.py holds the forms to their budgets (and to no scratch) on the built library.  A layout
// without a form here keeps its kernel of the unsplit run: at (8, 32) (the C5 jump) no form shortened the step.
#include "flow_b_mh.hpp"
#include "pot_basic.hpp"

namespace nfmc {

// M(CPL, LPC, HP, WPE)
#define NFMC_FOR_LEAN_FORM(M) M(8, 8, 4, 5)

int lean_wpe(BCfg c, int hp) {
#define M(CPL, LPC, HP, WPE) \
    if (c.cpl == CPL && c.lpc == LPC && hp == HP) return WPE;
    NFMC_FOR_LEAN_FORM(M)
#undef M
    return 0;
}

int launch_b_lean(const NfmcFlowMhArgs& a, BCfg c, int hp, bool diag, int64_t tiles, int grid, hipStream_t st, bool dry) {
    const bool r7 = rng_rounds(a.rng) == 7;
#define M(CPL, LPC, HP, WPE)                                                                                           \
    if (c.cpl == CPL && c.lpc == LPC && hp == HP) {                                                                    \
        const size_t img = (size_t)FlowImage<CPL, LPC, HP, true>::total_floats(a.flow.n_hidden_layers, a.flow.n_coupling) * \
                           sizeof(float);                                                                              \
        const size_t lds = lds_with_potential(img, a.pot, CPL, LPC);                                                  \
        if (lds > 120 * 1024) return NFMC_EUNSUPPORTED;                                                                \
        if (dry) return NFMC_OK;                                                                                       \
        auto kern = r7 ? (diag ? flow_mh_b_kernel<CPL, LPC, HP, QuadraticPot, true, true, 7, 0, WPE>                   \
                               : flow_mh_b_kernel<CPL, LPC, HP, QuadraticPot, true, false, 7, 0, WPE>)                 \
                       : (diag ? flow_mh_b_kernel<CPL, LPC, HP, QuadraticPot, true, true, 10, 0, WPE>                  \
                               : flow_mh_b_kernel<CPL, LPC, HP, QuadraticPot, true, false, 10, 0, WPE>);               \
        return launch_lds(kern, grid, kBlock, lds, st, a, tiles);                                                      \
    }
    NFMC_FOR_LEAN_FORM(M)
#undef M
    return NFMC_EUNSUPPORTED;
}

}  // namespace nfmc
