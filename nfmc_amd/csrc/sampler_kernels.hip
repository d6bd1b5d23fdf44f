// K1/K2 (+K6, K7): C entry points of the fused Langevin / HMC samplers.  Kernels: sampler_impl.hpp; the
// template instantiations live in sampler_{mala,hmc}_j{0,4,8}.hip (j = conditioner width of the optional
// jump tail, 0 = none) and, for the kinds whose row in kPotKinds (pot_kinds.hpp) says own_units, in a mala and an hmc
// unit per kind, so they compile in parallel.
#include <mutex>
#include <type_traits>

#include "run_parts.hpp"
#include "sampler_impl.hpp"
#include "sampler_mclmc.hpp"

namespace nfmc {

// (CPL, LPC) layouts, ordered by capacity CPL*LPC; equal capacities in order of measured preference
// (CPL = 8 keeps 4 waves/SIMD resident).
static const Cfg kCfgs[] = {{4, 1}, {4, 2}, {4, 4}, {4, 8}, {8, 8}, {4, 16}, {16, 4}, {8, 16}, {16, 8}, {8, 32}, {16, 16}, {8, 64}, {16, 32}, {16, 64}};

// with_jump: among the jump-tail layouts (kJumpCfgs, sampler_impl.hpp).  default_only: the override may name only
// layouts the default choice picks (the kinds with no instantiation at the other layouts: default_cfg_only in kPotKinds)
static Cfg choose_cfg(int d, bool with_jump, bool default_only) {
    const Cfg* list = with_jump ? kJumpCfgs : kCfgs;
    const int len = with_jump ? (int)(sizeof(kJumpCfgs) / sizeof(Cfg)) : (int)(sizeof(kCfgs) / sizeof(Cfg));
    int c = 0, l = 0;
    const char* e = getenv("NFMC_SAMPLER_CFG");   // "cpl,lpc" override (tuning)
    const bool named = e && sscanf(e, "%d,%d", &c, &l) == 2 && (!default_only || is_default_cfg(c, l));
    Cfg best = {0, 0};
    for (int i = 0; i < len; ++i) {
        const Cfg& k = list[i];
        if (k.cpl * k.lpc < d) continue;
        if (named && k.cpl == c && k.lpc == l) return k;
        if (best.cpl == 0 || k.cpl * k.lpc < best.cpl * best.lpc) best = k;
    }
    return best;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the argument checks of every sampler entry point (mala, hmc, mclmc); each adds its own behind them
template <class Args>
static int check_common(const Args* a) {
    if (!a || !a->x) return NFMC_EINVAL;
    if (a->n <= 0 || a->d <= 0 || a->n_steps <= 0) return NFMC_EINVAL;
    if (a->n_steps > NFMC_MAX_STEPS_PER_CALL) return NFMC_ESHAPE;
    if (a->d > 1024) return NFMC_ESHAPE;
    if (!(a->step_size > 0.f)) return NFMC_EINVAL;
    if (int rc = check_potential(a->pot, a->d, PotFamily::kRegister)) return rc;
    if (((uintptr_t)a->x & 3u) != 0) return NFMC_EALIGN;
    if (!store_ok(a->samples)) return NFMC_EINVAL;
    if (a->stats.sum_x && (!a->stats.sum_x2 || !a->stats.counters || !a->stats.scratch)) return NFMC_EINVAL;
    return NFMC_OK;
}

template <class Args>   // mala, hmc
static int check_metropolis(const Args* a) {
    if (int rc = check_common(a)) return rc;
    if (!rng_rounds_ok(a->rng, true)) return NFMC_EINVAL;
    if ((a->rng.replay_normals == nullptr) != (a->rng.replay_uniforms == nullptr) && (a->adjust & 1)) return NFMC_EINVAL;
    if (a->jump) {
        const NfmcJumpTail& j = *a->jump;
        if (j.flow.d != a->d || !j.counters) return NFMC_EINVAL;
        if (!j.flow.ea0_log_scale || !j.flow.ea0_shift || !j.flow.ea1_log_scale || !j.flow.ea1_shift) return NFMC_EINVAL;
        if (j.flow.n_coupling > 0 && !j.flow.weights) return NFMC_EINVAL;
        if (j.flow.n_hidden <= 0 || j.flow.n_hidden_layers <= 0) return NFMC_EINVAL;
        if (j.flow.n_hidden > 8 || a->d > 512 || j.flow.n_bins != 0) return NFMC_EUNSUPPORTED;
        if (!a->stats.sum_x) return NFMC_EINVAL;  // the jump counters travel through the statistics slab
        if (j.adjusted && (j.replay_latent != nullptr) != (j.replay_uniform != nullptr)) return NFMC_EINVAL;
    }
    return NFMC_OK;
}

template <class Args>
static bool fast_path(const Args* a, const Cfg& c) {
    // the FAST kernels assume a scalar potential with b = 0 (the carried |x|^2 of the Langevin ratio)
    return a->d == c.cpl * c.lpc && a->inv_mass_diag == nullptr && a->pot.a == nullptr && a->pot.b == nullptr &&
           (a->pot.kind != NFMC_POT_QUADRATIC || a->pot.b_scalar == 0.f) && aligned16(a->x) &&
           (!a->samples.base || aligned16(a->samples.base));
}

// ------------------------------------------------------------------------------------------------
// Warmup: statistics fold + tuning controller in one launch of ONE workgroup (NfmcTune).  The column totals of the
// call's per-workgroup partials are folded into the run's accumulators like stats_finish_kernel<true> does and kept in
// the tuning state; then the same workgroup runs the controller: mass-diagonal update over the coordinates, dual
// averaging of the step size on thread 0.  (A first version spread the fold over several workgroups and let the last
// one to arrive -- ticket counter, device-scope fences -- run the controller: on this multi-XCD part a device-scope
// release writes back the whole L2 of the XCD, 25-30 us per controller update with the sampler's 32 MB of state dirty
// in it.  Tuning launches therefore use at most kTuneGrid workgroups, so that one workgroup folds their slabs in a
// few load round trips.)
constexpr int kTuneGrid = 256;   // one load round trip of the folding workgroup (two need more than its 128 VGPRs per thread)
template <int NCHUNK>   // round trips: slabs / 256
__global__ void __launch_bounds__(kFinishBlock) tune_finish_kernel(double* __restrict__ scratch, int nblocks, int dp, int d,
                                                                   NfmcStats st, NfmcTune tn, unsigned long long attempted,
                                                                   uint32_t step0, int pool) {
    __shared__ double part[kFinishSlices][kFinishCols];
    const int width = 2 * dp + kStatTail;
    const int col = threadIdx.x % kFinishCols, slice = threadIdx.x / kFinishCols;
    double* __restrict__ totals = tn.state + NFMC_TUNE_WORDS;
    // The slabs were written by workgroups on all eight XCDs, so every dependent load round trip of this workgroup goes
    // through memory: a thread therefore issues ALL its loads of kGroups column groups -- 8 rows each, what kTuneGrid
    // workgroups leave per thread -- before it adds anything (5 groups cover d <= 64 in one round trip).
    constexpr int kGroups = 5, kRows = 8;   // 40 fp64 loads in flight per thread (1024 threads: 128 VGPRs each)
    for (int t0 = 0; t0 < width; t0 += kGroups * kFinishCols) {
        double acc[kGroups];
#pragma unroll
        for (int gi = 0; gi < kGroups; ++gi) acc[gi] = 0.0;
#pragma unroll
        for (int r0 = 0; r0 < NCHUNK * kRows * kFinishSlices; r0 += kRows * kFinishSlices) {   // 256 slabs per round trip
            double v[kGroups][kRows];
#pragma unroll
            for (int gi = 0; gi < kGroups; ++gi) {
                const int t = t0 + gi * kFinishCols + col;
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    const int b = r0 + slice + u * kFinishSlices;
                    v[gi][u] = (t < width && b < nblocks) ? scratch[(size_t)b * width + t] : 0.0;
                }
            }
#pragma unroll
            for (int gi = 0; gi < kGroups; ++gi) {
                const int t = t0 + gi * kFinishCols + col;
#pragma unroll
                for (int u = 0; u < kRows; ++u) acc[gi] += v[gi][u];   // row order
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    const int b = r0 + slice + u * kFinishSlices;
                    if (t < width && b < nblocks) scratch[(size_t)b * width + t] = 0.0;
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // one chunk's 40 loads in flight at a time (128 VGPRs per thread)
        }
#pragma unroll
        for (int gi = 0; gi < kGroups; ++gi) {
            const int t = t0 + gi * kFinishCols + col;
            const double p0 = acc[gi];
            __syncthreads();   // part[] of the previous column group has been consumed
            part[slice][col] = p0;
            __syncthreads();
            if (slice == 0 && t < width) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < kFinishSlices; ++k) s += part[k][col];
                totals[t] = s;   // coordinate columns: sums of x - c and (x - c)^2, un-shifted below
                if (t == 2 * dp) {
                    st.counters[NFMC_CNT_ACCEPTED] += (unsigned long long)(s + 0.5);
                    st.counters[NFMC_CNT_ATTEMPTED] += attempted;
                } else if (t == 2 * dp + 1) {
                    st.counters[NFMC_CNT_NONFINITE] += (unsigned long long)(s + 0.5);
                }
            }
        }
    }
    __syncthreads();   // totals[] written by this workgroup's own threads: workgroup scope is enough
    const double n_tot = (double)attempted;
    // The kernels summed y = x - c about the shift c (StatShift): the run's sums of x and x^2 are un-shifted here in fp64,
    // the variance comes from the shifted sums, which do not cancel while c stays near the mean, and c moves to this
    // update's mean (an fp32 value: the kernels subtract it in fp32).
    double* __restrict__ shift = tn.state + NFMC_TUNE_WORDS + 2 * dp + kStatTail;
    const bool tune_imd = tn.tune_inv_mass_diag && tn.inv_mass_diag && n_tot > 1.0;   // mcmc/base.py:146-151
    const double beta = tn.state[NFMC_TUNE_IMD_ADJUSTMENT];
    for (int j = threadIdx.x; j < d; j += kFinishBlock) {
        const double c = shift[j], s1 = totals[j], s2 = totals[dp + j];
        st.sum_x[j] += s1 + n_tot * c;
        st.sum_x2[j] += s2 + c * (2.0 * s1 + n_tot * c);
        if (tune_imd) {
            // torch.var (unbiased); held at >= 0 against rounding -- the next launch takes 1 / inv_mass_diag^2 and its root
            double var = (s2 - s1 * s1 / n_tot) / (n_tot - 1.0);
            var = var > 0.0 ? var : 0.0;
            tn.inv_mass_diag[j] = (float)(beta * var + (1.0 - beta) * (double)tn.inv_mass_diag[j]);
        }
        if (n_tot > 0.0) shift[j] = (double)(float)(c + s1 / n_tot);
    }
    if (threadIdx.x != 0) return;
    const double h_used = tn.trajectory ? tn.state[NFMC_TUNE_STEP_SIZE] : 0.0;   // what the update's transitions ran with
    if (tn.tune_step_size) {                                                       // mcmc/base.py:153-161, tuning.py:22-38
        const double acc = totals[2 * dp];
        const double err = tn.state[NFMC_TUNE_TARGET] - acc / n_tot;
        const double S = tn.state[NFMC_TUNE_ERROR_SUM] + err;
        const double it = tn.state[NFMC_TUNE_ITERATION];
        const double log_raw = tn.state[NFMC_TUNE_ANCHOR] - S / (sqrt(it) * tn.state[NFMC_TUNE_GAMMA]);
        const double w = pow(it, -tn.state[NFMC_TUNE_KAPPA]);
        const double log_smooth = w * log_raw + (1.0 - w) * tn.state[NFMC_TUNE_LOG_SMOOTH];
        tn.state[NFMC_TUNE_ERROR_SUM] = S;
        tn.state[NFMC_TUNE_LOG_RAW] = log_raw;
        tn.state[NFMC_TUNE_LOG_SMOOTH] = log_smooth;
        tn.state[NFMC_TUNE_ITERATION] = it + 1.0;
        tn.state[NFMC_TUNE_STEP_SIZE] = exp(log_smooth);
    }
    // Trajectory length (NfmcTune.trajectory; estimator and controller in the header comment): the leapfrog steps of the
    // update's transitions [step0, step0 + pool) recounted as the kernel counted them, then, while T adapts, one Adam step
    // on log T from the pooled sums the launch left in the two jump columns, with the step size set just above.
    if (tn.trajectory) {
        double* __restrict__ tr = tn.state + NFMC_TUNE_WORDS + 3 * dp + kStatTail;
        const double T_used = tr[NFMC_TRAJ_LENGTH], lmax = tr[NFMC_TRAJ_MAX_LEAPFROG];
        double steps = 0.0;
        for (int s = 0; s < pool; ++s) steps += (double)trajectory_leapfrog_count(step0 + (uint32_t)s, T_used, h_used, lmax);
        tr[NFMC_TRAJ_LEAPFROG_TOTAL] += steps;
        if (tn.trajectory == NFMC_TRAJECTORY_ADAPT) {
            const double h_new = tn.state[NFMC_TUNE_STEP_SIZE];
            const double sum_g = totals[2 * dp + 2], sum_alpha = totals[2 * dp + 3];
            const double g_hat = sum_alpha > 0.0 ? sum_g / sum_alpha : 0.0;
            double log_T = tr[NFMC_TRAJ_LOG_LENGTH], v = tr[NFMC_TRAJ_V], log_bar = tr[NFMC_TRAJ_LOG_AVERAGED];
            if (sum_alpha > 0.0 && fabs(g_hat) <= 1.7e308) {   // else: the update leaves T alone
                const double j = tr[NFMC_TRAJ_COUNT] + 1.0, b2 = tr[NFMC_TRAJ_BETA2], clip = tr[NFMC_TRAJ_CLIP];
                v = b2 * v + (1.0 - b2) * g_hat * g_hat;
                double delta = tr[NFMC_TRAJ_LEARNING_RATE] * g_hat / (sqrt(v / (1.0 - pow(b2, j))) + 1e-8);
                delta = delta > clip ? clip : (delta < -clip ? -clip : delta);
                const double lo = log(h_new), hi = log(lmax * h_new);
                log_T += delta;
                log_T = log_T < lo ? lo : log_T;
                log_T = log_T > hi ? hi : log_T;
                const double w = pow(j, -0.75);
                log_bar = w * log_T + (1.0 - w) * log_bar;
                tr[NFMC_TRAJ_COUNT] = j;
                tr[NFMC_TRAJ_V] = v;
                tr[NFMC_TRAJ_LOG_LENGTH] = log_T;
                tr[NFMC_TRAJ_LOG_AVERAGED] = log_bar;
                tr[NFMC_TRAJ_LENGTH] = exp(log_T);
            }
            tr[NFMC_TRAJ_G_HAT] = g_hat;
            tr[NFMC_TRAJ_ALPHA_SUM] = sum_alpha;
            const double used = tr[NFMC_TRAJ_HISTORY_USED];
            if (used < tr[NFMC_TRAJ_HISTORY_ROWS]) {   // updates beyond the capacity overwrite nothing
                double* __restrict__ row = tr + NFMC_TRAJ_WORDS + (size_t)used * NFMC_TRAJ_ROW_WORDS;
                row[NFMC_TRAJ_ROW_LENGTH] = T_used;
                row[NFMC_TRAJ_ROW_STEP_SIZE] = h_used;
                row[NFMC_TRAJ_ROW_G_HAT] = g_hat;
                row[NFMC_TRAJ_ROW_ALPHA_SUM] = sum_alpha;
                row[NFMC_TRAJ_ROW_LEAPFROGS] = steps;
                row[NFMC_TRAJ_ROW_LOG_LENGTH] = log_T;
                row[NFMC_TRAJ_ROW_V] = v;
                row[NFMC_TRAJ_ROW_LOG_AVERAGED] = log_bar;
                row[NFMC_TRAJ_ROW_NEXT_STEP_SIZE] = h_new;
            }
            tr[NFMC_TRAJ_HISTORY_USED] = used + 1.0;
        }
    }
}

// Round 4: the tuning launches no longer run at a quarter of the machine.  With kTuneGrid workgroups a one-transition launch
// of 65536 x 64 chains is 1024 waves, one per SIMD, each walking eight chain tiles one after the other (26 us); with the full
// grid it is ~8 us, but leaves up to 2032 slabs -- which kTuneFoldWgs workgroups first fold 128 at a time (every thread has all
// its loads in flight at once, as in tune_finish_kernel) into partial slabs at the END of the scratch, and tune_finish_kernel
// then folds those.  Three launches per controller update instead of two, ~30 us instead of 47 (profiles/r04_warmup_probe.txt).
constexpr int kTuneFoldSlabs = 128, kTuneFoldWgs = 16;
__global__ void __launch_bounds__(kFinishBlock) tune_fold_kernel(double* __restrict__ scratch, int nblocks, int width,
                                                                 double* __restrict__ partial) {
    __shared__ double part[kFinishSlices][kFinishCols];
    const int col = threadIdx.x % kFinishCols, slice = threadIdx.x / kFinishCols;
    const int b0 = blockIdx.x * kTuneFoldSlabs;
    double* __restrict__ dst = partial + (size_t)blockIdx.x * width;
    constexpr int kGroups = 5, kRows = kTuneFoldSlabs / kFinishSlices;   // 20 fp64 loads in flight per thread
    for (int t0 = 0; t0 < width; t0 += kGroups * kFinishCols) {
        double v[kGroups][kRows];
#pragma unroll
        for (int gi = 0; gi < kGroups; ++gi) {
            const int t = t0 + gi * kFinishCols + col;
#pragma unroll
            for (int u = 0; u < kRows; ++u) {
                const int b = b0 + slice + u * kFinishSlices;
                v[gi][u] = (t < width && b < nblocks) ? scratch[(size_t)b * width + t] : 0.0;
            }
        }
#pragma unroll
        for (int gi = 0; gi < kGroups; ++gi) {
            const int t = t0 + gi * kFinishCols + col;
            double acc = 0.0;
#pragma unroll
            for (int u = 0; u < kRows; ++u) acc += v[gi][u];   // row order
#pragma unroll
            for (int u = 0; u < kRows; ++u) {
                const int b = b0 + slice + u * kFinishSlices;
                if (t < width && b < nblocks) scratch[(size_t)b * width + t] = 0.0;
            }
            __syncthreads();   // part[] of the previous column group has been consumed
            part[slice][col] = acc;
            __syncthreads();
            if (slice == 0 && t < width) {
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < kFinishSlices; ++k) sum += part[k][col];
                dst[t] = sum;
            }
        }
    }
}

// grid of a tuning launch and whether its slabs are folded in two levels (the scratch then holds the partial slabs behind
// the last workgroup's)
static int tune_grid(int64_t tiles, int dp, int64_t scratch_bytes, bool* two_level) {
    const int64_t width = 2 * dp + kStatTail;
    *two_level = tiles > kTuneGrid && scratch_bytes >= (int64_t)kMaxGrid * width * (int64_t)sizeof(double) && !getenv("NFMC_TUNE_ONE_LEVEL");
    const int cap = *two_level ? kMaxGrid - kTuneFoldWgs : kTuneGrid;
    return (int)(tiles < cap ? tiles : cap);
}

// The slabs a controller kernel is to finish behind a tuning launch of `grid` workgroups, *count of them: the launch's own,
// or, behind a two-level launch, the partial slabs that tune_fold_kernel, enqueued here, folds them into
static double* tune_fold(double* scratch, int grid, bool two_level, int width, hipStream_t st, int* count) {
    *count = two_level ? (grid + kTuneFoldSlabs - 1) / kTuneFoldSlabs : grid;
    if (!two_level) return scratch;
    double* partial = scratch + (size_t)(kMaxGrid - kTuneFoldWgs) * width;
    hipLaunchKernelGGL(tune_fold_kernel, dim3(*count), dim3(kFinishBlock), 0, st, scratch, grid, width, partial);
    return partial;
}

template <class Args>
static int check_tune(const Args& a, const NfmcJumpTail* jump, int dp, bool hmc) {
    // the jittered trajectory: the hmc kernel with a tuning state, a trajectory block behind it and the Metropolis test
    if (a.tune.trajectory != NFMC_TRAJECTORY_OFF) {
        if (!hmc || !a.tune.state || !(a.adjust & 1)) return NFMC_EINVAL;
        if (a.tune.trajectory != NFMC_TRAJECTORY_ADAPT && a.tune.trajectory != NFMC_TRAJECTORY_FROZEN) return NFMC_EINVAL;
    }
    if (!a.tune.state) return NFMC_OK;
    if (!a.stats.sum_x || a.stats.defer || jump) return NFMC_EINVAL;   // the controller rides on the per-call fold
    if (a.tune.tune_inv_mass_diag && (!a.tune.inv_mass_diag || a.tune.inv_mass_diag != a.inv_mass_diag)) return NFMC_EINVAL;
    // the state holds 2 * padded_d(d) + kStatTail column totals and padded_d(d) shift words (nfmc_tune_state_doubles):
    // a layout override of a larger capacity would not fit them
    if (dp != padded_d(a.d)) return NFMC_EINVAL;
    return NFMC_OK;
}

// one launch of the mala / hmc kernels at layout c with jump-tail width jhp: the own_units kinds (kPotKinds) from their
// units, kinds 0 to 3 from the unit of the width
#define NFMC_KIND_CASE(KIND, POT) \
    case KIND: return launch_mala_kind<POT>(a, jd, c, jhp, tiles, grid, sqrt2h, st);
static int launch_mala(const NfmcMalaArgs& a, const JumpDev& jd, Cfg c, int jhp, bool fast, int64_t tiles, int grid,
                       float sqrt2h, hipStream_t st) {
    switch (a.pot.kind) { NFMC_FOR_OWN_UNIT_POT(NFMC_KIND_CASE) }
    return jhp == 0 ? launch_mala_j0(a, jd, c, fast, tiles, grid, sqrt2h, st)
                    : (jhp == 4 ? launch_mala_j4(a, jd, c, fast, tiles, grid, sqrt2h, st)
                                : launch_mala_j8(a, jd, c, fast, tiles, grid, sqrt2h, st));
}
#undef NFMC_KIND_CASE
#define NFMC_KIND_CASE(KIND, POT) \
    case KIND: return launch_hmc_kind<POT>(a, jd, c, jhp, tiles, grid, st);
static int launch_hmc(const NfmcHmcArgs& a, const JumpDev& jd, Cfg c, int jhp, bool fast, int64_t tiles, int grid,
                      hipStream_t st) {
    switch (a.pot.kind) { NFMC_FOR_OWN_UNIT_POT(NFMC_KIND_CASE) }
    return jhp == 0 ? launch_hmc_j0(a, jd, c, fast, tiles, grid, st)
                    : (jhp == 4 ? launch_hmc_j4(a, jd, c, fast, tiles, grid, st) : launch_hmc_j8(a, jd, c, fast, tiles, grid, st));
}
#undef NFMC_KIND_CASE

#define NFMC_KIND_CASE(KIND, POT) \
    case KIND: return launch_mclmc_kind<POT>(a, c, tiles, grid, st);
static int launch_mclmc(const NfmcMclmcArgs& a, Cfg c, int64_t tiles, int grid, hipStream_t st) {
    switch (a.pot.kind) { NFMC_FOR_OWN_UNIT_POT(NFMC_KIND_CASE) }
    return launch_mclmc_j0(a, c, tiles, grid, st);
}
#undef NFMC_KIND_CASE

// ------------------------------------------------------------------------------------------------
// mclmc (sampler_mclmc.hpp).  The kernel leaves, per workgroup slab, the sums of x and x^2, the steps taken and not
// taken, and in the two jump columns the fp64 sums of the finite dE^2 and dE.
//
// A call without tuning: the three energy columns of the call's slabs into energy_sums (+=), by one workgroup in a fixed
// order, ahead of stats_finish_kernel, which zeroes the slabs.
__global__ void __launch_bounds__(kBlock) mclmc_energy_fold_kernel(const double* __restrict__ scratch, int nblocks, int width,
                                                                   double* __restrict__ energy_sums, unsigned long long attempted) {
    __shared__ double red[3][kBlock];
    double s[3] = {0.0, 0.0, 0.0};   // not taken, sum dE^2, sum dE
    for (int b = threadIdx.x; b < nblocks; b += kBlock) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += scratch[(size_t)b * width + (width - 3 + k)];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        energy_sums[0] += red[1][0];
        energy_sums[1] += red[2][0];
        energy_sums[2] += (double)attempted - red[0][0];
    }
}

// Warmup: statistics fold and the controller of NfmcMclmcTune in one launch of one workgroup, behind a tuning launch of
// at most kTuneGrid slabs (or behind tune_fold_kernel's partial slabs), as tune_finish_kernel is for mala / hmc.  A thread
// owns a column and adds its rows in row order.  imd: the call's inv_mass_diag (NULL = ones).
__global__ void __launch_bounds__(kFinishBlock) mclmc_tune_finish_kernel(double* __restrict__ scratch, int nblocks, int dp, int d,
                                                                         NfmcStats st, NfmcMclmcTune tn, const float* imd,
                                                                         double* __restrict__ energy_sums,
                                                                         unsigned long long attempted) {
    __shared__ double red[kFinishBlock];
    const int width = 2 * dp + kStatTail;
    double* __restrict__ totals = tn.state + NFMC_MCLMC_WORDS;
    for (int t = threadIdx.x; t < width; t += kFinishBlock) {
        double s = 0.0;
#pragma unroll 8
        for (int b = 0; b < nblocks; ++b) {
            s += scratch[(size_t)b * width + t];
            scratch[(size_t)b * width + t] = 0.0;
        }
        totals[t] = s;
    }
    __syncthreads();   // totals[] written by this workgroup's own threads: workgroup scope is enough
    const double n_tot = (double)attempted;
    const double bad = totals[2 * dp + 1], se2 = totals[2 * dp + 2], se = totals[2 * dp + 3];
    const double count = n_tot - bad;
    const double V = count > 0.0 ? se2 / (count * (double)d) : 0.0;
    const bool good = count > 0.0 && fabs(V) <= 1.7e308;
    const bool tune_imd = good && tn.tune_inv_mass_diag && tn.inv_mass_diag && n_tot > 1.0;
    const double beta = tn.state[NFMC_MCLMC_IMD_ADJUSTMENT];
    double* __restrict__ shift = totals + width;
    double ratio = 0.0;   // this thread's share of sum_j v_j / s_j
    for (int j = threadIdx.x; j < d; j += kFinishBlock) {
        const double c = shift[j], s1 = totals[j], s2 = totals[dp + j];
        st.sum_x[j] += s1 + n_tot * c;
        st.sum_x2[j] += s2 + c * (2.0 * s1 + n_tot * c);
        double var = n_tot > 1.0 ? (s2 - s1 * s1 / n_tot) / (n_tot - 1.0) : 0.0;   // unbiased, about the lagged centre
        var = var > 0.0 ? var : 0.0;
        double sj = imd ? (double)imd[j] : 1.0;
        if (tune_imd) {
            const float next = (float)((1.0 - beta) * sj + beta * var);
            tn.inv_mass_diag[j] = next;
            sj = (double)next;   // what the next launch reads
        }
        ratio += var / sj;
        if (n_tot > 0.0) shift[j] = (double)(float)(c + s1 / n_tot);
    }
    red[threadIdx.x] = ratio;
    __syncthreads();
    for (int off = kFinishBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    st.counters[NFMC_CNT_ACCEPTED] += (unsigned long long)(totals[2 * dp] + 0.5);
    st.counters[NFMC_CNT_ATTEMPTED] += attempted;
    st.counters[NFMC_CNT_NONFINITE] += (unsigned long long)(bad + 0.5);
    if (energy_sums) {
        energy_sums[0] += se2;
        energy_sums[1] += se;
        energy_sums[2] += count;
    }
    const double eps_used = tn.state[NFMC_MCLMC_STEP_SIZE], len_used = tn.state[NFMC_MCLMC_DECOHERENCE_LENGTH];
    double eps = eps_used, len = len_used;
    if (!good) {
        if (tn.tune_step_size) eps = 0.5 * eps_used;
    } else {
        if (tn.tune_step_size) {
            const double ln2 = 0.6931471805599453;
            double move = log(tn.state[NFMC_MCLMC_TARGET] / V) / 6.0;   // the local energy error is of third order in eps
            move = move > ln2 ? ln2 : (move < -ln2 ? -ln2 : move);
            eps = exp(log(eps_used) + move);
        }
        if (tn.tune_decoherence_length && n_tot > 1.0) {
            const double next = tn.state[NFMC_MCLMC_DECOHERENCE_FACTOR] * sqrt(red[0]);
            if (next > 0.0 && next <= 1.7e308) len = next;   // all variances zero: L stays
        }
    }
    tn.state[NFMC_MCLMC_STEP_SIZE] = eps;
    tn.state[NFMC_MCLMC_DECOHERENCE_LENGTH] = len;
    tn.state[NFMC_MCLMC_ENERGY_VARIANCE] = V;
    tn.state[NFMC_MCLMC_COUNT] = count;
    const double used = tn.state[NFMC_MCLMC_HISTORY_USED];
    if (used < tn.state[NFMC_MCLMC_HISTORY_ROWS]) {   // updates beyond the capacity overwrite nothing
        double* __restrict__ row = shift + dp + (size_t)used * NFMC_MCLMC_ROW_WORDS;
        row[NFMC_MCLMC_ROW_STEP_SIZE] = eps_used;
        row[NFMC_MCLMC_ROW_DECOHERENCE_LENGTH] = len_used;
        row[NFMC_MCLMC_ROW_ENERGY_VARIANCE] = V;
        row[NFMC_MCLMC_ROW_COUNT] = count;
        row[NFMC_MCLMC_ROW_NEXT_STEP_SIZE] = eps;
        row[NFMC_MCLMC_ROW_NEXT_DECOHERENCE_LENGTH] = len;
    }
    tn.state[NFMC_MCLMC_HISTORY_USED] = used + 1.0;
}

static JumpDev jump_dev(const NfmcJumpTail* j) {
    JumpDev jd = {};
    if (j) {
        jd.flow = j->flow;
        jd.adjusted = j->adjusted;
        jd.replay_latent = j->replay_latent;
        jd.replay_uniform = j->replay_uniform;
        jd.mask_out = j->mask_out;
        jd.log_ratio_out = j->log_ratio_out;
    }
    return jd;
}

}  // namespace nfmc

using namespace nfmc;

extern "C" int64_t nfmc_stats_scratch_bytes(int32_t d) {
    if (d <= 0 || d > 1024) return 0;
    return stats_scratch_doubles(padded_d(d)) * (int64_t)sizeof(double);
}

extern "C" int64_t nfmc_tune_state_doubles(int32_t d) {
    if (d <= 0 || d > 1024) return 0;
    return NFMC_TUNE_WORDS + 3 * padded_d(d) + kStatTail;   // controller words, column totals, shift
}

extern "C" int64_t nfmc_tune_trajectory_doubles(int32_t history_rows) {
    if (history_rows < 0) return 0;
    return NFMC_TRAJ_WORDS + (int64_t)history_rows * NFMC_TRAJ_ROW_WORDS;
}

extern "C" int nfmc_sampler_layout(int32_t d, int32_t pot_kind_id, int32_t* cpl, int32_t* lpc) {
    if (!cpl || !lpc || d <= 0) return NFMC_EINVAL;
    if (d > 1024) return NFMC_ESHAPE;
    const PotKind* pk = pot_kind(pot_kind_id);
    if (!pk) return NFMC_EUNSUPPORTED;
    const Cfg c = choose_cfg(d, false, pk->default_cfg_only);   // as sampler_steps, no jump tail
    if (!c.cpl) return NFMC_ESHAPE;
    *cpl = c.cpl;
    *lpc = c.lpc;
    return NFMC_OK;
}

// What differs between the samplers behind sampler_steps, beside the launch.  mala and hmc:
template <class Args>
struct MetropolisParts {
    static constexpr bool kJumpTail = true, kDefaultCfgOnly = false;
    static const NfmcJumpTail* take_jump(Args& a) {   // a host pointer: never dereferenced on the device
        const NfmcJumpTail* jump = a.jump;
        a.jump = nullptr;
        return jump;
    }
    static int check(const Args& a, const NfmcJumpTail* jump, int dp) {
        return check_tune(a, jump, dp, std::is_same<Args, NfmcHmcArgs>::value);
    }
    // the per-step outputs of the pool that starts `off` chain-steps into the call (the driver moves the replay normals)
    static void advance(Args& b, const Args& a, int64_t off) {
        if (a.rng.replay_uniforms) b.rng.replay_uniforms = a.rng.replay_uniforms + off;
        if (a.masks_out) b.masks_out = a.masks_out + off;
        if (a.log_ratio_out) b.log_ratio_out = a.log_ratio_out + off;
    }
    // the controller behind a pool, over the slabs tune_fold left
    static void update(const Args& a, double* slabs, int count, int dp, unsigned long long attempted, uint32_t step0, int pool, hipStream_t st) {
        hipLaunchKernelGGL(tune_finish_kernel<1>, dim3(1), dim3(kFinishBlock), 0, st, slabs, count, dp, a.d, a.stats, a.tune, attempted, step0, pool);
    }
    static void fold(const Args&, int, int, unsigned long long, hipStream_t) {}   // ahead of stats_finish_kernel, without tuning
};

struct MclmcParts {
    static constexpr bool kJumpTail = false, kDefaultCfgOnly = true;   // the default layouts: the only ones with mclmc kernels
    static const NfmcJumpTail* take_jump(NfmcMclmcArgs&) { return nullptr; }
    static int check(const NfmcMclmcArgs& a, const NfmcJumpTail*, int dp) { return dp != padded_d(a.d) ? NFMC_EINVAL : NFMC_OK; }
    static void advance(NfmcMclmcArgs& b, const NfmcMclmcArgs& a, int64_t off) {
        if (a.energy_out) b.energy_out = a.energy_out + off;
    }
    static void update(const NfmcMclmcArgs& a, double* slabs, int count, int dp, unsigned long long attempted, uint32_t, int, hipStream_t st) {
        hipLaunchKernelGGL(mclmc_tune_finish_kernel, dim3(1), dim3(kFinishBlock), 0, st, slabs, count, dp, a.d, a.stats, a.tune,
                           a.inv_mass_diag, a.energy_sums, attempted);
    }
    static void fold(const NfmcMclmcArgs& a, int grid, int width, unsigned long long attempted, hipStream_t st) {
        if (a.energy_sums)
            hipLaunchKernelGGL(mclmc_energy_fold_kernel, dim3(1), dim3(kBlock), 0, st, a.stats.scratch, grid, width, a.energy_sums, attempted);
    }
};

// The part the sampler entry points share, behind their own argument checks: layout, tile and grid arithmetic, the
// scratch / defer / tune checks, then either the warmup loop (one launch + controller update per `every` transitions, all
// of the call enqueued here) or one launch and the statistics finish.  launch(args, jd, c, jhp, fast, tiles, grid);
// P: the sampler's parts above.  part: the call is one part of a split run (run_parts.hpp).
template <class P, class Args, class Launch>
static int sampler_steps(const Args* args, hipStream_t st, Launch launch, const LaunchPart* part = nullptr) {
    Args a = *args;
    const NfmcJumpTail* jump = P::take_jump(a);
    const int jhp = jump ? (jump->flow.n_hidden <= 4 ? 4 : 8) : 0;
    const Cfg c = choose_cfg(a.d, jhp > 0, P::kDefaultCfgOnly || pot_kind(a.pot.kind)->default_cfg_only);
    if (!c.cpl) return NFMC_ESHAPE;
    const bool fast = fast_path(&a, c) && !a.tune.state;   // tuning launches sum about a shift (StatShift): general kernels
    const int dp = c.cpl * c.lpc;
    const int cpw = kWave / c.lpc;
    const int64_t tiles = (a.n + (int64_t)kWavesPerBlock * cpw - 1) / ((int64_t)kWavesPerBlock * cpw);
    bool two_level = false;
    const int gcap = part ? part->grid_cap : kMaxGrid;
    const int grid = a.tune.state ? tune_grid(tiles, dp, a.stats.scratch_bytes, &two_level) : (int)(tiles < gcap ? tiles : gcap);
    if (a.stats.sum_x && a.stats.scratch_bytes < (int64_t)grid * (2 * dp + kStatTail) * (int64_t)sizeof(double))
        return NFMC_ESCRATCH;
    if (check_defer(a.stats, dp, a.d)) return NFMC_EINVAL;
    if (int rc = P::check(a, jump, dp)) return rc;
    const int width = 2 * dp + kStatTail;
    if (part && a.stats.sum_x) a.stats.scratch += (size_t)part->slab0 * width;   // checked as the caller gave it
    const JumpDev jd = jump_dev(jump);
    if (a.tune.state) {
        const int every = (a.tune.every > 0 && a.tune.every < a.n_steps) ? a.tune.every : a.n_steps;
        const int total = a.n_steps;
        for (int s0 = 0; s0 < total; s0 += every) {
            const int k = total - s0 < every ? total - s0 : every;
            Args b = a;
            b.n_steps = k;
            b.rng.step0 = a.rng.step0 + (uint32_t)s0;
            if (a.rng.replay_normals) b.rng.replay_normals = a.rng.replay_normals + (int64_t)s0 * a.n * a.d;
            P::advance(b, a, (int64_t)s0 * a.n);
            if (int rc = launch(b, jd, c, 0, fast, tiles, grid)) return rc;
            int count = 0;
            double* slabs = tune_fold(a.stats.scratch, grid, two_level, width, st, &count);
            P::update(a, slabs, count, dp, (unsigned long long)a.n * (unsigned long long)k, b.rng.step0, k, st);
            NFMC_HIP_CHECK_LAUNCH();
            store_advance(a.samples, k);
        }
        return NFMC_OK;
    }
    if (int rc = launch(a, jd, c, jhp, fast, tiles, grid)) return rc;
    NFMC_HIP_CHECK_LAUNCH();
    if (a.stats.sum_x && !a.stats.defer) {
        const unsigned long long attempted = (unsigned long long)a.n * (unsigned long long)a.n_steps;
        P::fold(a, grid, width, attempted, st);
        hipLaunchKernelGGL(stats_finish_kernel<true>, dim3(stats_finish_grid(dp)), dim3(kFinishBlock), 0, st, a.stats.scratch,
                           grid, dp, a.d, a.stats, attempted, jump ? jump->counters : nullptr,
                           P::kJumpTail ? (unsigned long long)a.n : 0ull);
        NFMC_HIP_CHECK_LAUNCH();
    }
    return NFMC_OK;
}

static int mala_steps(const NfmcMalaArgs* args, hipStream_t st, const LaunchPart* part) {
    if (int rc = check_metropolis(args)) return rc;
    const float sqrt2h = (float)sqrt(2.0 * (double)args->step_size);  // math.sqrt(2*step_size), langevin.py:75
    return sampler_steps<MetropolisParts<NfmcMalaArgs>>(args, st, [=](const NfmcMalaArgs& a, const JumpDev& jd, Cfg c, int jhp, bool fast, int64_t tiles, int grid) {
        return launch_mala(a, jd, c, jhp, fast, tiles, grid, sqrt2h, st);
    }, part);
}

static int hmc_steps(const NfmcHmcArgs* args, hipStream_t st, const LaunchPart* part) {
    if (int rc = check_metropolis(args)) return rc;
    if (args->n_leapfrog <= 0) return NFMC_EINVAL;
    return sampler_steps<MetropolisParts<NfmcHmcArgs>>(args, st, [=](const NfmcHmcArgs& a, const JumpDev& jd, Cfg c, int jhp, bool fast, int64_t tiles, int grid) {
        return launch_hmc(a, jd, c, jhp, fast, tiles, grid, st);
    }, part);
}

extern "C" int nfmc_mala_steps_f32(const NfmcMalaArgs* args, nfmc_stream_t stream) {
    return mala_steps(args, (hipStream_t)stream, nullptr);
}

extern "C" int nfmc_hmc_steps_f32(const NfmcHmcArgs* args, nfmc_stream_t stream) {
    return hmc_steps(args, (hipStream_t)stream, nullptr);
}

extern "C" int64_t nfmc_mclmc_state_doubles(int32_t d, int32_t history_rows) {
    if (d <= 0 || d > 1024 || history_rows < 0) return 0;
    return nfmc_tune_state_doubles(d) + (int64_t)history_rows * NFMC_MCLMC_ROW_WORDS;
}

extern "C" int nfmc_mclmc_steps_f32(const NfmcMclmcArgs* args, nfmc_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = check_common(args)) return rc;
    const NfmcMclmcArgs& a = *args;
    if (!a.velocity) return NFMC_EINVAL;
    if (((uintptr_t)a.velocity & 3u) != 0) return NFMC_EALIGN;
    if (a.d < 2 || !(a.decoherence_length > 0.f)) return NFMC_EINVAL;
    if (int rc = rng_default_only(a.rng)) return rc;
    if (a.stats.defer) return NFMC_EINVAL;   // the energy columns are folded by the call itself
    if ((a.energy_sums || a.tune.state) && !a.stats.sum_x) return NFMC_EINVAL;
    if (a.tune.state && a.tune.tune_inv_mass_diag && (!a.tune.inv_mass_diag || a.tune.inv_mass_diag != a.inv_mass_diag))
        return NFMC_EINVAL;
    return sampler_steps<MclmcParts>(args, st, [=](const NfmcMclmcArgs& b, const JumpDev&, Cfg c, int, bool, int64_t tiles, int grid) {
        return launch_mclmc(b, c, tiles, grid, st);
    });
}

// ------------------------------------------------------------------------------------------------
// nfmc_jump_run_f32: the launches of a whole JumpNFMC.sample run, split into parts of chains on streams of their own.
//
// Nothing couples one chain to another in these kernels (the Philox streams are keyed by the global chain id, the
// statistics are per-workgroup slabs), so jump i of a part depends on inner launch i of the same part only: with two parts
// on two streams the jump of one -- a short kernel of one round of waves that stages a weight image and flushes statistics,
// well short of the vector pipes' rate -- runs while the inner kernel of the other fills the SIMDs, and the launch
// boundaries of one part fall inside kernels of the other.

// The side streams of the current device: non-blocking, created on first use, kept for the life of the process.
static int side_streams(int count, hipStream_t* out) {
    constexpr int kMaxDevices = 64;
    static std::mutex mu;
    static hipStream_t streams[kMaxDevices][NFMC_JUMP_RUN_MAX_PARTS - 1] = {};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return (int)e;
    if (dev < 0 || dev >= kMaxDevices) return NFMC_EUNSUPPORTED;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < count; ++i) {
        if (!streams[dev][i])
            if (hipError_t e = hipStreamCreateWithFlags(&streams[dev][i], hipStreamNonBlocking)) return (int)e;
        out[i] = streams[dev][i];
    }
    return NFMC_OK;
}

// chains per workgroup tile of the sampler kernels at event size d (sampler_steps: jump-tail-free layout)
static int64_t sampler_tile_chains(int d, int pot_kind_id) {
    const PotKind* pk = pot_kind(pot_kind_id);
    const Cfg c = choose_cfg(d, false, pk && pk->default_cfg_only);
    return c.cpl ? (int64_t)kWavesPerBlock * (kWave / c.lpc) : 0;
}

template <class Args, class Steps>
static int jump_run(const NfmcJumpRun& r, const Args& inner, hipStream_t st, Steps steps) {
    const NfmcFlowMhArgs& jump = *r.jump;
    const int64_t n = inner.n;
    const int d = inner.d, K = r.n_inner, T = r.n_outer;
    if (T <= 0 || K <= 0 || r.n_parts < 1 || r.n_parts > NFMC_JUMP_RUN_MAX_PARTS) return NFMC_EINVAL;
    if (!inner.x || n <= 0 || d <= 0 || jump.x != inner.x || jump.n != n || jump.flow.d != d || !jump.logq) return NFMC_EINVAL;
    if (jump.rng.seed != inner.rng.seed || jump.rng.chain_offset != inner.rng.chain_offset || jump.rng.rounds != inner.rng.rounds)
        return NFMC_EINVAL;
    // nothing a host would advance between the launches
    if (inner.jump || inner.tune.state || inner.samples.base || jump.samples.base || inner.masks_out || jump.masks_out ||
        inner.log_ratio_out || jump.log_ratio_out || inner.rng.replay_normals || inner.rng.replay_uniforms ||
        jump.rng.replay_normals || jump.rng.replay_uniforms)
        return NFMC_EINVAL;
    if ((inner.stats.sum_x != nullptr) != (jump.stats.sum_x != nullptr)) return NFMC_EINVAL;
    if (inner.stats.sum_x && (!inner.stats.defer || !jump.stats.defer || inner.stats.scratch != jump.stats.scratch)) return NFMC_EINVAL;

    // parts: whole tiles of both kernels, so that every chain keeps its place in its tile (and its wave's partial sums)
    int parts = r.n_parts;
    int64_t m = n;
    if (parts > 1) {
        const int64_t ti = sampler_tile_chains(d, inner.pot.kind), tj = flow_mh_tile_chains(jump);
        if (ti <= 0 || tj <= 0) {
            parts = 1;   // the jump runs on kernels that take no part; the checks of the unsplit launches speak for the rest
        } else {
            const int64_t tile = ti > tj ? ti : tj, per = (n + parts - 1) / parts;
            m = (per + tile - 1) / tile * tile;
        }
    }
    const int share = (kMaxGrid + parts - 1) / parts;
    int used = 0;   // parts with chains
    while (used < parts && (int64_t)used * m < n) ++used;

    // events[p], p < used - 1: the fork of part p + 1, recorded on part p's stream; events[used - 2 + p], p >= 1: the join of part p
    hipStream_t streams[NFMC_JUMP_RUN_MAX_PARTS] = {st};
    hipEvent_t events[2 * NFMC_JUMP_RUN_MAX_PARTS] = {};
    const int n_events = used > 1 ? 2 * (used - 1) : 0;
    if (used > 1) {
        if (int rc = side_streams(used - 1, streams + 1)) return rc;
        for (int p = 0; p < n_events; ++p)
            if (hipError_t e = hipEventCreateWithFlags(&events[p], hipEventDisableTiming)) {
                for (int q = 0; q < p; ++q) (void)hipEventDestroy(events[q]);
                return (int)e;
            }
    }
    // Fork.  Parts that start together stay in step -- their inner kernels run side by side, then their jumps do, and
    // nothing is won -- so part p + 1 starts behind the first inner block of part p: the parts run a fraction of an
    // iteration apart from then on, and the jump of one falls into the inner kernel of the others.  (NFMC_JUMP_STAGGER=0,
    // for measurements: every part starts behind what the caller's stream held on entry.)
    const char* stagger_env = getenv("NFMC_JUMP_STAGGER");
    const bool stagger = !(stagger_env && atoi(stagger_env) == 0);

    int rc = NFMC_OK;
    for (int i = 0; i < T && !rc; ++i) {
        const uint32_t base = inner.rng.step0 + (uint32_t)i * (uint32_t)(K + 1);
        for (int p = 0; p < used && !rc; ++p) {
            const int64_t lo = (int64_t)p * m, np = (n - lo < m ? n - lo : m);
            const LaunchPart lp = {p * share, share < kMaxGrid - p * share ? share : kMaxGrid - p * share, n};
            const LaunchPart* part = parts > 1 ? &lp : nullptr;
            if (i == 0 && p > 0) {   // behind the fork event of the part before (a side stream has no other work: every call joins it)
                if (hipError_t e = hipStreamWaitEvent(streams[p], events[p - 1], 0)) rc = (int)e;
            }
            if (i == 0 && p + 1 < used && !stagger && !rc)
                if (hipError_t e = hipEventRecord(events[p], streams[p])) rc = (int)e;
            for (int off = 0; off < K && !rc; off += NFMC_MAX_STEPS_PER_CALL) {
                Args b = inner;
                b.x = inner.x + lo * d;
                b.n = np;
                b.n_steps = K - off < NFMC_MAX_STEPS_PER_CALL ? K - off : NFMC_MAX_STEPS_PER_CALL;
                b.rng.chain_offset = inner.rng.chain_offset + (uint64_t)lo;
                b.rng.step0 = base + (uint32_t)off;
                rc = steps(&b, streams[p], part);
            }
            // recorded also behind a failed enqueue: the next part's wait must find a recorded event
            if (i == 0 && p + 1 < used && (stagger || rc)) {
                hipError_t e = hipEventRecord(events[p], streams[p]);
                if (e != hipSuccess && !rc) rc = (int)e;
            }
            if (rc) break;
            NfmcFlowMhArgs j = jump;
            j.x = jump.x + lo * d;
            j.logq = jump.logq + lo;
            j.n = np;
            j.n_steps = 1;
            j.logq_cached = 0;
            j.rng.chain_offset = jump.rng.chain_offset + (uint64_t)lo;
            j.rng.step0 = base + (uint32_t)K;
            rc = flow_mh_steps(j, streams[p], part);
        }
    }

    // join, also behind a failed enqueue: no side stream runs past the call
    for (int p = 1; p < used; ++p) {
        hipError_t e = hipEventRecord(events[used - 1 + p - 1], streams[p]);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, events[used - 1 + p - 1], 0);
        if (e != hipSuccess && !rc) rc = (int)e;
    }
    for (int p = 0; p < n_events; ++p) (void)hipEventDestroy(events[p]);
    return rc;
}

extern "C" int nfmc_jump_run_f32(const NfmcJumpRun* run, nfmc_stream_t stream) {
    if (!run || !run->inner || !run->jump) return NFMC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (run->inner_kind == NFMC_INNER_MALA) return jump_run(*run, *(const NfmcMalaArgs*)run->inner, st, mala_steps);
    if (run->inner_kind == NFMC_INNER_HMC) return jump_run(*run, *(const NfmcHmcArgs*)run->inner, st, hmc_steps);
    return NFMC_EINVAL;
}
