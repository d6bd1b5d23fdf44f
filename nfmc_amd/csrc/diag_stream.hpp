// Running convergence diagnostics for runs that keep no states (include/nfmc_hip.h: nfmc_diag_stream_*).
//
// The accumulator is fed every kept draw once, in blocks of R draws that sit in a small staging ring, and carries per
// series (chain j, coordinate c; S = n d of them, row-major like a state row) in device memory
//     shift  s = the first draw (fp32)               ssum   S = sum_t y_t, y_t = x_t - s (fp64 of the exact difference)
//     half   sum and sum of squares of y over [0, h) and [Kp - h, Kp), h = Kp / 2, Kp = the planned number of draws (fp64)
//     head   fl32(y_t) for t < L                     tail   fl32(y_t) of the last L draws, draw t in row t mod L
// and per workgroup one row of fp64 lag products P_l = sum_j sum_t y_t y_{t-l}, l = 0 .. L (fp32 products of the rounded
// y, summed in fp32 inside one block of draws and in fp64 from there on; the row is added to across updates and the rows
// are folded in a fixed order at the end: the K7 pattern of diagnostics.hpp).  With mu_j = S_j / K after K draws
//     K a_{j,l} = P_{j,l} - mu_j (2 S_j - head_l(j) - tail_l(j)) + (K - l) mu_j^2,   l < K
// (head_l / tail_l = sum of the first / last l shifted draws), so summed over chains, with Q = sum_j mu_j^2,
// H_t = sum_j mu_j y_t(j) and T_u = sum_j mu_j y_{K-1-u}(j):
//     K sum_j a_{j,l} = P_l + sum_{t<l} H_t + sum_{u<l} T_u - (K + l) Q.
//
// diag_stream_update_kernel has the shape of diag_series_kernel: one lane per series, 64 neighbouring series per tile,
// eight waves of 16 lags each, the lag window in an LDS ring of five time tiles indexed by LOCAL time i (i < 128: the
// 128 draws before the block, read from `tail`, zeros before draw 0 and beyond lag L; i = 128 + r: new draw r), the
// 16-entry register window of a wave preloaded from that history.  Per chain tile and block it reads R staging rows and L
// tail rows and writes min(R, L) tail rows (the ring is indexed by draw number, nothing is shifted in memory).
#pragma once
#include "diagnostics.hpp"

namespace nfmc {

constexpr int kStreamHist = (kDiagSlots - 1) * kDiagTile;   // 128 local rows of history
constexpr int kStreamGrid = 1024;                           // workgroups of the update at most = rows of lag partials
constexpr int kStreamHalf = 4;                              // half-chain sums per series
constexpr int kStreamHead = 6;                              // rows of the finish kernel before H and T: the five main rows, Q
constexpr int kStreamSlices = 64;                           // chain slices of the finish kernel (per 64-coordinate chunk)
static_assert(kStreamHist >= NFMC_DIAG_MAX_LAG + 1, "the history covers every lag");

struct StreamPlan {
    int cpt, nchunk;
    int64_t ntile;
    int nb;                 // workgroups per chunk of the update
    int nb2;                // chain slices of the finish kernel
    int rows2;              // kStreamHead + 2 L
    int64_t S;
    // state, in bytes: doubles first
    int64_t off_ssum, off_half, off_part, off_shift, off_head, off_tail, state_bytes;
    // work of the sums call, in doubles
    int64_t w_rows, w_fold, w_lags, w_group, work_doubles;
};

inline StreamPlan stream_plan(int64_t n, int d, int max_lag) {
    StreamPlan p;
    p.cpt = d < kWave ? kWave / d : 1;
    p.nchunk = d < kWave ? 1 : (d + kWave - 1) / kWave;
    p.ntile = (n + p.cpt - 1) / p.cpt;
    const int cap = kStreamGrid / p.nchunk;
    p.nb = (int)(p.ntile < cap ? p.ntile : cap);
    const int cap2 = kStreamSlices / p.nchunk > 1 ? kStreamSlices / p.nchunk : 1;
    p.nb2 = (int)(p.ntile < cap2 ? p.ntile : cap2);
    p.rows2 = kStreamHead + 2 * max_lag;
    p.S = n * d;
    const int64_t L = max_lag;
    p.off_ssum = 0;
    p.off_half = p.off_ssum + 8 * p.S;
    p.off_part = p.off_half + 8 * kStreamHalf * p.S;
    p.off_shift = p.off_part + 8 * (int64_t)p.nb * (L + 1) * d;
    p.off_head = p.off_shift + 4 * p.S;
    p.off_tail = p.off_head + 4 * L * p.S;
    p.state_bytes = (p.off_tail + 4 * L * p.S + 7) / 8 * 8;
    const int64_t gcap = kDiagGroupThreads / d > 1 ? kDiagGroupThreads / d : 1;
    const int64_t gs = n < gcap ? n : gcap;   // group = 1 has the most superchains
    p.w_rows = p.S;
    p.w_fold = p.w_rows + (int64_t)p.nb2 * p.rows2 * d;
    p.w_lags = p.w_fold + (int64_t)p.rows2 * d;
    p.w_group = p.w_lags + (L + 1) * d;
    p.work_doubles = p.w_group + gs * kDiagGroup * d;
    return p;
}

struct StreamState {
    double *ssum, *half, *part;
    float *shift, *head, *tail;
};

inline StreamState stream_state(void* base, const StreamPlan& p) {
    char* b = (char*)base;
    return {(double*)(b + p.off_ssum), (double*)(b + p.off_half), (double*)(b + p.off_part),
            (float*)(b + p.off_shift), (float*)(b + p.off_head), (float*)(b + p.off_tail)};
}

// R new draws, global indices t0 .. t0 + R - 1, in rows (row0 + r) mod ring_rows of the staging ring xr
__global__ void __launch_bounds__(kDiagBlock, 2)
diag_stream_update_kernel(const float* __restrict__ xr, int ring_rows, int row0, int R, int64_t t0, int64_t Kp, int64_t n,
                          int d, int nlag, int cpt, int nchunk, int64_t ntile, int nb, StreamState st) {
    __shared__ float ring[kDiagSlots * kDiagTile][kWave];
    __shared__ double hsum[kStreamHalf + 1][kDiagWaves][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cc = blockIdx.x % nchunk;
    const int b = blockIdx.x / nchunk;
    const int64_t row = n * d;
    const bool narrow = d < kWave;
    const int coord = narrow ? lane % d : cc * kWave + lane;
    const int sub = narrow ? lane / d : 0;
    const bool lane_ok = narrow ? lane < cpt * d : coord < d;
    const bool lag_wave = wave * kDiagLags < nlag;
    const int L = nlag - 1;
    const int64_t h = Kp / 2;
    const int ntt = (R + kDiagTile - 1) / kDiagTile;
    const int64_t nq = (ntile - b + nb - 1) / nb;   // this workgroup's chain tiles b, b + nb, ...

    double dacc[kDiagLags];
#pragma unroll
    for (int k = 0; k < kDiagLags; ++k) dacc[k] = 0.0;
    float acc[kDiagLags], win[kDiagLags];

    // staged time tile (raw draws, loaded one step ahead) and the chain tile it belongs to
    float pre[kDiagStage];
    int64_t off_st = 0, off = 0;
    float s_st = 0.f, s = 0.f;
    bool act_st = false, act = false;
    auto fetch = [&](int64_t q, int tt) {
        if (tt == 0) {
            const int64_t chain = (b + q * nb) * cpt + sub;
            act_st = lane_ok && chain < n;
            off_st = act_st ? chain * d + coord : 0;
            s_st = !act_st ? 0.f : t0 == 0 ? xr[(int64_t)row0 * row + off_st] : st.shift[off_st];
        }
#pragma unroll
        for (int r = 0; r < kDiagStage; ++r) {
            const int j = tt * kDiagTile + wave + kDiagWaves * r;
            pre[r] = (act_st && j < R) ? xr[(int64_t)((row0 + j) % ring_rows) * row + off_st] : 0.f;
        }
    };

    fetch(0, 0);
    for (int64_t q = 0; q < nq; ++q) {
        if (q) __syncthreads();   // the products and the half sums of the chain tile before are done
        act = act_st;
        off = off_st;
        s = s_st;
        if (t0 == 0 && act && wave == 0) st.shift[off] = s;
        // the 128 draws before the block: local row i holds draw t0 - 128 + i
#pragma unroll
        for (int r = 0; r < kStreamHist / kDiagWaves; ++r) {
            const int i = wave + kDiagWaves * r;
            const int64_t t = t0 - kStreamHist + i;
            float v = 0.f;
            if (act && t >= 0 && i >= kStreamHist - L) v = st.tail[(t % L) * row + off];
            ring[i][lane] = v;
        }
        double ss = 0.0, sv0 = 0.0, sq0 = 0.0, sv1 = 0.0, sq1 = 0.0;
#pragma unroll
        for (int k = 0; k < kDiagLags; ++k) acc[k] = 0.f;
        for (int tt = 0; tt < ntt; ++tt) {
            __syncthreads();   // tt = 0: the history is read (its tail rows may be overwritten); else the products before
            const int slot = (kDiagSlots - 1 + tt) % kDiagSlots;
#pragma unroll
            for (int r = 0; r < kDiagStage; ++r) {
                const int j = tt * kDiagTile + wave + kDiagWaves * r;
                const bool in = act && j < R;
                const double v = in ? (double)pre[r] - (double)s : 0.0;
                const float y = (float)v;
                ring[slot * kDiagTile + wave + kDiagWaves * r][lane] = y;
                if (in) {
                    const int64_t t = t0 + j;
                    ss += v;
                    if (t < h) {
                        sv0 += v;
                        sq0 = fma(v, v, sq0);
                    }
                    if (t >= Kp - h) {
                        sv1 += v;
                        sq1 = fma(v, v, sq1);
                    }
                    if (t < L) st.head[t * row + off] = y;
                    if (j >= R - L) st.tail[(t % L) * row + off] = y;
                }
            }
            __syncthreads();
            if (tt + 1 < ntt) fetch(q, tt + 1);
            else if (q + 1 < nq) fetch(q + 1, 0);
            if (lag_wave) {
                if (tt == 0) {   // the 15 window entries before the block's first draw
#pragma unroll
                    for (int j = 1; j < kDiagLags; ++j) win[j] = ring[kStreamHist - kDiagLags + j - wave * kDiagLags][lane];
                    win[0] = 0.f;
                }
                const float* cur = &ring[slot * kDiagTile][lane];
#pragma unroll
                for (int hh = 0; hh < kDiagTile / kDiagLags; ++hh) {
                    const int u0 = kStreamHist + tt * kDiagTile + (hh - wave) * kDiagLags;   // local row of the first new window entry, >= 0
                    const float* old = &ring[u0 % (kDiagSlots * kDiagTile)][lane];
#pragma unroll
                    for (int j = 0; j < kDiagLags; ++j) {
                        const float v = cur[(hh * kDiagLags + j) * kWave];
                        win[j] = old[j * kWave];
#pragma unroll
                        for (int k = 0; k < kDiagLags; ++k) acc[k] = fmaf(v, win[(j - k) & (kDiagLags - 1)], acc[k]);
                    }
                }
            }
        }
        if (lag_wave) {
#pragma unroll
            for (int k = 0; k < kDiagLags; ++k) dacc[k] += (double)acc[k];
        }
        hsum[0][wave][lane] = ss;
        hsum[1][wave][lane] = sv0;
        hsum[2][wave][lane] = sq0;
        hsum[3][wave][lane] = sv1;
        hsum[4][wave][lane] = sq1;
        __syncthreads();
        if (wave == 0 && act) {
#pragma unroll
            for (int g = 0; g < kStreamHalf + 1; ++g) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < kDiagWaves; ++w) t += hsum[g][w][lane];
                double* dst = g == 0 ? st.ssum + off : st.half + (int64_t)(g - 1) * row + off;
                *dst += t;
            }
        }
    }

    // d < 64: lanes c, c + d, ... hold the same coordinate; lane c adds them in lane order
    if (narrow) {
#pragma unroll
        for (int k = 0; k < kDiagLags; ++k) {
            double t = 0.0;
            for (int r = 0; r < cpt; ++r) t += __shfl(dacc[k], coord + r * d, kWave);
            dacc[k] = t;
        }
    }
    if (coord < d && sub == 0 && lane_ok && lag_wave) {
        double* prow = st.part + (int64_t)b * nlag * d;
#pragma unroll
        for (int k = 0; k < kDiagLags; ++k) {
            const int l = wave * kDiagLags + k;
            if (l < nlag) prow[(int64_t)l * d + coord] += dacc[k];
        }
    }
}

// Row r of the finish, summed over the chains of slice b: partial (nb2, rows2, d).  r = 0 .. 4 the main rows of `sums`
// (zeros when the run ended early: combine writes NaN there), 5 Q, 6 + t H_t, 6 + L + u T_u.  Row 0 also leaves the chain
// means m in `m_out` for diag_group_kernel.  Wave w takes the chain tiles b + (4 i + w) nb2; the four waves and, for
// d < 64, the lanes of one coordinate are added in a fixed order.
__global__ void __launch_bounds__(kBlock)
diag_stream_rows_kernel(StreamState st, int64_t K, int64_t Kp, int64_t n, int d, int L, int cpt, int nchunk, int64_t ntile,
                        int nb2, int rows2, double* __restrict__ m_out, double* __restrict__ partial) {
    __shared__ double red[kWavesPerBlock][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cc = blockIdx.x % nchunk;
    const int b = blockIdx.x / nchunk;
    const int r = blockIdx.y;
    const int64_t row = n * d;
    const bool narrow = d < kWave;
    const int coord = narrow ? lane % d : cc * kWave + lane;
    const int sub = narrow ? lane / d : 0;
    const bool lane_ok = narrow ? lane < cpt * d : coord < d;
    const bool whole = K == Kp;
    const double dk = (double)K, dh = (double)(Kp / 2);
    const float* lagrow = nullptr;   // r >= 6: the draw that multiplies mu
    if (r >= kStreamHead) {
        const int t = r - kStreamHead;
        if (t < L) {
            if (t < K) lagrow = st.head + (int64_t)t * row;
        } else if (t - L < K) {
            lagrow = st.tail + ((K - 1 - (t - L)) % L) * row;
        }
    }
    double a = 0.0;
    for (int64_t q = b + (int64_t)wave * nb2; q < ntile; q += (int64_t)kWavesPerBlock * nb2) {
        const int64_t chain = q * cpt + sub;
        if (!lane_ok || chain >= n) continue;
        const int64_t off = chain * d + coord;
        const double mu = st.ssum[off] / dk;
        const double s = (double)st.shift[off];
        if (r >= kStreamHead) {
            if (lagrow) a += mu * (double)lagrow[off];
        } else if (r == 0) {
            a += s + mu;
            m_out[off] = s + mu;
        } else if (r == 1) {
            a += (s + mu) * (s + mu);
        } else if (r == 5) {
            a += mu * mu;
        } else if (whole) {
            const double v0 = st.half[off], q0 = st.half[row + off], v1 = st.half[2 * row + off], q1 = st.half[3 * row + off];
            const double mh0 = s + v0 / dh, mh1 = s + v1 / dh;
            if (r == 2) a += mh0 + mh1;
            else if (r == 3) a += mh0 * mh0 + mh1 * mh1;
            else a += (q0 - v0 * v0 / dh) / (dh - 1.0) + (q1 - v1 * v1 / dh) / (dh - 1.0);
        }
    }
    red[wave][lane] = a;
    __syncthreads();
    if (wave != 0) return;
    double t = red[0][lane];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) t += red[w][lane];
    if (narrow) {
        double u = 0.0;
        for (int k = 0; k < cpt; ++k) u += __shfl(t, coord + k * d, kWave);
        t = u;
    }
    if (coord < d && sub == 0 && lane_ok) partial[((int64_t)b * rows2 + r) * d + coord] = t;
}

// thread c: the five main rows and the lags of `sums` from the folded finish rows f (rows2, d) and lag products p (L + 1, d)
__global__ void __launch_bounds__(kBlock)
diag_stream_combine_kernel(const double* __restrict__ f, const double* __restrict__ p, int64_t K, int64_t Kp, int d, int L,
                           double* __restrict__ sums) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= d) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    sums[(int64_t)NFMC_DIAG_SUM_M * d + c] = f[c];
    sums[(int64_t)NFMC_DIAG_SUM_M2 * d + c] = f[d + c];
    for (int r = NFMC_DIAG_SUM_MH; r <= NFMC_DIAG_SUM_S2H; ++r) sums[(int64_t)r * d + c] = K == Kp ? f[(int64_t)r * d + c] : nan;
    const double Q = f[(int64_t)5 * d + c], dk = (double)K;
    double cum = 0.0;
    for (int l = 0; l <= L; ++l) {
        if (l > 0) cum += f[(int64_t)(kStreamHead + l - 1) * d + c] + f[(int64_t)(kStreamHead + L + l - 1) * d + c];
        sums[(int64_t)(NFMC_DIAG_ACOV + l) * d + c] = l < K ? (p[(int64_t)l * d + c] + cum - (dk + l) * Q) / dk : 0.0;
    }
}

}  // namespace nfmc
