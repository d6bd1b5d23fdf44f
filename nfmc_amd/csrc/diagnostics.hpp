// Convergence diagnostics of the kept states (include/nfmc_hip.h: nfmc_chain_diagnostics_f32).
//
// A series is one (chain, coordinate) pair; row t of the slab holds the n * d series side by side.
//
// diag_mean_kernel (first read of the slab): one thread per series, lanes on neighbouring series, the draws summed in
// fp64 in time order -> the chain's own mean m, kept in `work` for the other kernels.
//
// diag_series_kernel (second read) gives every series one lane, 64 neighbouring series per workgroup tile, so each wave
// load is 256 contiguous bytes of a row whatever d is:
//   d <  64: a tile is 64 / d whole chains (cpt), lane i = chain i / d, coordinate i % d (64 % d lanes idle);
//   d >= 64: a tile is 64 coordinates (chunk cc) of one chain.
// Either way a lane keeps ITS coordinate over all the tiles its workgroup strides through (same chunk, next chains), so
// the cross-chain totals are per-lane fp64 registers and one row of partials per workgroup; diag_fold_kernel sums the rows
// in a fixed order (the K7 pattern: moments_kernel + stats_finish_kernel).
// It walks (chain tile, time tile of 32 draws) steps with a workgroup of eight waves.  Per step the waves centre the
// staged draws in fp64 (x - m; the half-chain sums are taken from these fp64 values), round them to fp32 and store them to
// a ring of five time tiles in LDS ([draw][lane]: lanes on consecutive banks, no conflicts), issue the global loads of
// the NEXT step (the next chain tile's first draws included, so only a workgroup's very first loads are exposed), and
// then wave w accumulates the 16 lags 16 w .. 16 w + 15: per draw it reads v = x[t] and the one new window entry
// x[t - 16 w] from the ring, keeps the other 15 in registers (slot (t - l) mod 16, compile-time after unrolling: no
// moves), and issues 16 FMAs (the compiler pairs them into v_pk_fma_f32).  Draws before 0 enter the window as zeros and
// draws past n_draws are stored as zeros, so no lag needs a bound check and a_l = 0 for l >= n_draws.  16 lags per wave,
// not 32 on four waves: the window, its odd-aligned copy for the packed FMAs, the fp32 and the fp64 accumulators of 32
// lags do not fit 256 registers, and spill reloads inside the product loop wait on the same counter as the prefetch.
#pragma once
#include "common.hpp"

namespace nfmc {

constexpr int kDiagTile = 32;        // draws per time tile
constexpr int kDiagLags = 16;        // lags per wave
constexpr int kDiagWaves = (NFMC_DIAG_MAX_LAG + 1) / kDiagLags, kDiagBlock = kDiagWaves * kWave;   // 8 waves, 512 threads
constexpr int kDiagSlots = 5;        // ring tiles: the current one + 4 back (lag 127 reaches 4 tiles back)
constexpr int kDiagStage = kDiagTile / kDiagWaves;   // draws of a time tile each thread stages
constexpr int kDiagMain = 5;         // SUM_M, SUM_M2, SUM_MH, SUM_MH2, SUM_S2H: rows of the series kernel before the lags
constexpr int kDiagGroup = 3;        // SUM_MU, SUM_MU2, SUM_BT
constexpr int kDiagGroupThreads = 65536;   // (superchain slice, coordinate) threads of the group kernel at most
constexpr int kDiagFoldCols = 32, kDiagFoldSlices = kBlock / kDiagFoldCols;
static_assert(NFMC_DIAG_MAX_LAG + 1 == kDiagWaves * kDiagLags && kDiagTile == 2 * kDiagLags, "one wave per 16 lags");
static_assert(NFMC_DIAG_ACOV == kDiagMain + kDiagGroup, "row layout of sums");

struct DiagPlan {
    int cpt;          // chains per tile (d < 64), else 1
    int nchunk;       // 64-coordinate chunks per chain (d >= 64), else 1
    int64_t ntile;    // chain tiles
    int nb;           // workgroups per chunk = rows of partials
    int rows_main;    // kDiagMain + max_lag + 1
    int64_t gs;       // superchain slices = rows of group partials (bound: min(n, cap))
    int64_t off_main, off_group, total;   // doubles into work: [m (n d)] [main (nb, rows_main, d)] [group (gs, 3, d)]
};

inline DiagPlan diag_plan(int64_t n, int d, int max_lag, int64_t groups) {
    DiagPlan p;
    p.cpt = d < kWave ? kWave / d : 1;
    p.nchunk = d < kWave ? 1 : (d + kWave - 1) / kWave;
    p.ntile = (n + p.cpt - 1) / p.cpt;
    const int cap = kMaxGrid / p.nchunk;
    p.nb = (int)(p.ntile < cap ? p.ntile : cap);
    p.rows_main = kDiagMain + max_lag + 1;
    const int64_t gcap = kDiagGroupThreads / d > 1 ? kDiagGroupThreads / d : 1;
    p.gs = groups < gcap ? groups : gcap;
    p.off_main = n * d;
    p.off_group = p.off_main + (int64_t)p.nb * p.rows_main * d;
    p.total = p.off_group + p.gs * kDiagGroup * d;
    return p;
}

// m[s] = mean over the K draws of series s (S = n d of them), fp64, summed in time order
__global__ void __launch_bounds__(kBlock) diag_mean_kernel(const float* __restrict__ x, int64_t K, int64_t S,
                                                           double* __restrict__ m) {
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < S; s += (int64_t)gridDim.x * kBlock) {
        const float* p = x + s;
        double a = 0.0;
#pragma unroll 8
        for (int64_t t = 0; t < K; ++t) a += (double)p[t * S];
        m[s] = a / (double)K;
    }
}

__global__ void __launch_bounds__(kDiagBlock, 2) diag_series_kernel(const float* __restrict__ x, int64_t K, int64_t n, int d,
                                                                int nlag, int cpt, int nchunk, int64_t ntile, int nb,
                                                                const double* __restrict__ m_in,
                                                                double* __restrict__ partial) {
    __shared__ float ring[kDiagSlots * kDiagTile][kWave];
    __shared__ double hsum[4][kDiagWaves][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cc = blockIdx.x % nchunk;
    const int b = blockIdx.x / nchunk;
    const int64_t row = n * d;
    const bool narrow = d < kWave;
    const int coord = narrow ? lane % d : cc * kWave + lane;
    const int sub = narrow ? lane / d : 0;
    const bool lane_ok = narrow ? lane < cpt * d : coord < d;
    const bool lag_wave = wave * kDiagLags < nlag;
    const int64_t h = K / 2;
    const int64_t ntt = (K + kDiagTile - 1) / kDiagTile;
    const int64_t nstep = (ntile - b + nb - 1) / nb * ntt;   // this workgroup's chain tiles b, b + nb, ... x time tiles

    double dacc[kDiagLags], e[kDiagMain];
#pragma unroll
    for (int k = 0; k < kDiagLags; ++k) dacc[k] = 0.0;
#pragma unroll
    for (int q = 0; q < kDiagMain; ++q) e[q] = 0.0;
    float acc[kDiagLags], win[kDiagLags];
    double sv0 = 0.0, sq0 = 0.0, sv1 = 0.0, sq1 = 0.0;   // half-chain sums of x - m and its square (fp64, before the rounding to fp32), over the draws this thread stages

    // staged step (raw draws, loaded one step ahead) and the chain tile it belongs to
    float pre[kDiagStage];
    const float* xs_st = x;
    double m_st = 0.0, m_cur = 0.0;
    bool act_st = false, act_cur = false;
    auto fetch = [&](int64_t step) {
        const int64_t q = step / ntt, tt = step - q * ntt;
        if (tt == 0) {
            const int64_t chain = (b + q * nb) * cpt + sub;
            act_st = lane_ok && chain < n;
            const int64_t off = act_st ? chain * d + coord : 0;
            xs_st = x + off;
            m_st = act_st ? m_in[off] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kDiagStage; ++r) {
            const int64_t t = tt * kDiagTile + wave + kDiagWaves * r;
            pre[r] = (act_st && t < K) ? xs_st[t * row] : 0.f;
        }
    };
    // wave 0, once all four waves' half sums of a chain tile are in hsum: the chain's terms of the head rows
    auto finish_chain = [&]() {
        if (wave != 0 || !act_cur) return;
        double hs[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            hs[q] = 0.0;
#pragma unroll
            for (int w = 0; w < kDiagWaves; ++w) hs[q] += hsum[q][w][lane];
        }
        const double dh = (double)h;
        const double mh0 = m_cur + hs[0] / dh, mh1 = m_cur + hs[2] / dh;
        e[0] += m_cur;
        e[1] += m_cur * m_cur;
        e[2] += mh0 + mh1;
        e[3] += mh0 * mh0 + mh1 * mh1;
        e[4] += (hs[1] - hs[0] * hs[0] / dh) / (dh - 1.0) + (hs[3] - hs[2] * hs[2] / dh) / (dh - 1.0);
    };

    fetch(0);
    for (int64_t step = 0; step < nstep; ++step) {
        const int64_t tt = step % ntt;
        const int slot = (int)(tt % kDiagSlots);
        if (step) __syncthreads();   // the products of the step before are done (its ring tiles may go), its hsum is in
        if (tt == 0) {               // a new chain tile
            if (step) finish_chain();
            m_cur = m_st;
            act_cur = act_st;
            sv0 = sq0 = sv1 = sq1 = 0.0;
#pragma unroll
            for (int k = 0; k < kDiagLags; ++k) acc[k] = win[k] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < kDiagStage; ++r) {
            const int64_t t = tt * kDiagTile + wave + kDiagWaves * r;
            const double v = (act_cur && t < K) ? (double)pre[r] - m_cur : 0.0;
            ring[slot * kDiagTile + wave + kDiagWaves * r][lane] = (float)v;
            if (t < h) {
                sv0 += v;
                sq0 = fma(v, v, sq0);
            }
            if (t >= K - h) {        // draws past K are zeros
                sv1 += v;
                sq1 = fma(v, v, sq1);
            }
        }
        __syncthreads();
        if (step + 1 < nstep) fetch(step + 1);
        if (lag_wave) {
            const float* cur = &ring[slot * kDiagTile][lane];
#pragma unroll
            for (int hh = 0; hh < kDiagTile / kDiagLags; ++hh) {   // 16 draws at a time: their window entries are 16 ring rows in a run
                const int64_t u0 = tt * kDiagTile + (hh - wave) * kDiagLags;   // draw of the first new window entry
                const bool past = u0 >= 0;   // else they lie before draw 0 (the ring rows hold another chain's draws)
                const float* old = &ring[(int)((u0 + kDiagSlots * kDiagTile) % (kDiagSlots * kDiagTile))][lane];
#pragma unroll
                for (int j = 0; j < kDiagLags; ++j) {
                    const float v = cur[(hh * kDiagLags + j) * kWave];
                    win[j] = past ? old[j * kWave] : 0.f;   // x[t - 16 wave]: replaces x[t - 16 wave - 16]
#pragma unroll
                    for (int k = 0; k < kDiagLags; ++k) acc[k] = fmaf(v, win[(j - k) & (kDiagLags - 1)], acc[k]);
                }
            }
        }
        if (tt == ntt - 1) {         // the chain tile is complete
            if (lag_wave) {
#pragma unroll
                for (int k = 0; k < kDiagLags; ++k) dacc[k] += (double)acc[k];
            }
            hsum[0][wave][lane] = sv0;
            hsum[1][wave][lane] = sq0;
            hsum[2][wave][lane] = sv1;
            hsum[3][wave][lane] = sq1;
        }
    }
    __syncthreads();
    finish_chain();

    // d < 64: lanes c, c + d, ... hold the same coordinate; lane c adds them in lane order
    if (narrow) {
#pragma unroll
        for (int k = 0; k < kDiagLags; ++k) {
            double s = 0.0;
            for (int r = 0; r < cpt; ++r) s += __shfl(dacc[k], coord + r * d, kWave);
            dacc[k] = s;
        }
#pragma unroll
        for (int q = 0; q < kDiagMain; ++q) {
            double s = 0.0;
            for (int r = 0; r < cpt; ++r) s += __shfl(e[q], coord + r * d, kWave);
            e[q] = s;
        }
    }
    if (coord < d && sub == 0 && lane_ok) {
        double* prow = partial + (int64_t)b * (kDiagMain + nlag) * d;
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < kDiagMain; ++q) prow[(int64_t)q * d + coord] = e[q];
        }
        if (lag_wave) {
            const double inv_k = 1.0 / (double)K;
#pragma unroll
            for (int k = 0; k < kDiagLags; ++k) {
                const int l = wave * kDiagLags + k;
                if (l < nlag) prow[(int64_t)(kDiagMain + l) * d + coord] = dacc[k] * inv_k;
            }
        }
    }
}

// superchains: thread (slice gs, coordinate c) walks the groups gs, gs + GS, ...; per group the mean of its M chain
// means and their variance about it.  partial (GS, 3, d).
__global__ void __launch_bounds__(kBlock) diag_group_kernel(const double* __restrict__ m, int64_t G, int64_t M, int d,
                                                            int64_t GS, double* __restrict__ partial) {
    const int64_t total = GS * d;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t gs = idx / d;
        const int c = (int)(idx - gs * d);
        double smu = 0.0, smu2 = 0.0, sbt = 0.0;
        for (int64_t k = gs; k < G; k += GS) {
            const double* p = m + k * M * d + c;
            double s = 0.0;
            for (int64_t j = 0; j < M; ++j) s += p[j * d];
            const double mu = s / (double)M;
            double ss = 0.0;
            if (M > 1) {
                for (int64_t j = 0; j < M; ++j) {
                    const double dv = p[j * d] - mu;
                    ss += dv * dv;
                }
                ss /= (double)(M - 1);
            }
            smu += mu;
            smu2 += mu * mu;
            sbt += ss;
        }
        double* out = partial + gs * kDiagGroup * d + c;
        out[0] = smu;
        out[d] = smu2;
        out[2 * (int64_t)d] = sbt;
    }
}

// partial (rows, width) -> out (width): a workgroup takes 32 columns at a time, thread (column, slice s) adds rows s,
// s + 8, ... and slice 0 adds the eight slices in order.  Column c lands at out[c] below `split` and at out[c + gap] from
// there on (the superchain rows of `sums` sit between the series kernel's head rows and its lags).
__global__ void __launch_bounds__(kBlock) diag_fold_kernel(const double* __restrict__ partial, int64_t rows, int64_t width,
                                                           int64_t split, int64_t gap, double* __restrict__ out) {
    __shared__ double red[kDiagFoldSlices][kDiagFoldCols];
    const int col = threadIdx.x % kDiagFoldCols, slice = threadIdx.x / kDiagFoldCols;
    const int64_t nblk = (width + kDiagFoldCols - 1) / kDiagFoldCols;
    for (int64_t cb = blockIdx.x; cb < nblk; cb += gridDim.x) {
        const int64_t c = cb * kDiagFoldCols + col;
        double s = 0.0;
        if (c < width)
            for (int64_t r = slice; r < rows; r += kDiagFoldSlices) s += partial[r * width + c];
        red[slice][col] = s;
        __syncthreads();
        if (slice == 0 && c < width) {
            double t = red[0][col];
            for (int q = 1; q < kDiagFoldSlices; ++q) t += red[q][col];
            out[c < split ? c : c + gap] = t;
        }
        __syncthreads();
    }
}

}  // namespace nfmc
