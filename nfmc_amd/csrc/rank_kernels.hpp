// Rank transform of the kept states (include/nfmc_hip.h: nfmc_rank_series_f32): the four series of the
// rank-normalised diagnostics of Vehtari et al. 2021, each an (n_draws, n, d) slab that goes through
// nfmc_chain_diagnostics_f32 unchanged.
//
// Per coordinate the S = n_draws * n pooled values are ranked by sorting their keys:
//   rank_key_kernel      reads the slab in 64 x 64 (pooled index, coordinate) tiles through LDS, so both the row-major
//                        reads and the coordinate-major writes are runs of up to 256 bytes, and maps every fp32 to an
//                        order-preserving uint32 (-0 -> +0, positives get the sign bit, negatives all bits flipped, NaN
//                        and +-Inf -> 0xFFFFFFFF, above every finite key).  keys (d, S).
//   rank_hist / rank_scan / rank_scatter_kernel   keys-only LSD radix sort, four passes of 8 bits, one segment per
//                        coordinate.  A tile is 2048 consecutive keys of one segment.  Per pass: the digit counts of every
//                        tile (LDS integer atomics), their exclusive scan per coordinate in (digit, tile) order, and the
//                        scatter.  In the scatter wave w owns keys [512 w, 512 w + 512) of the tile and walks them 64 at a
//                        time in order: eight ballots give each lane the lanes that hold its digit, the lanes below it
//                        among them are its place, and the wave's running base of that digit sits in LDS -- stable, without
//                        a global atomic.  Every pass is run, so a digit that is constant over a segment copies it and the
//                        sorted keys always end in the first buffer.
//   rank_stats_kernel    one thread per coordinate: the four order statistics of the definitions and the count of
//                        non-finite values (the keys at the top of the segment).
//   rank_fold_kernel     f = fl32(|fp64(v) - med|), ranked by a second sort for the folded series.
//   rank_emit_kernel     per element two binary searches of its key in its coordinate's sorted segment (lower and upper
//                        bound: lo = #{v < v_i}, hi = #{v <= v_i}), r = (lo + hi + 1) / 2, z = PPND16((r - 3/8) / (S + 1/4))
//                        in fp64 rounded once; or the comparison with the tail's order statistic.
// Everything is a function of the values alone: no floating-point atomic, no order of arrival, the same bits every call.
#pragma once
#include "common.hpp"

namespace nfmc {

constexpr int kRankBins = 256;                       // 8-bit digits
constexpr int kRankPasses = 4;
constexpr int kRankTile = 2048;                      // keys of one segment per scatter step
constexpr int kRankPer = kRankTile / kBlock;         // keys per thread
constexpr int kRankWaveKeys = kRankTile / kWavesPerBlock;
constexpr int kRankScanSlices = 4, kRankScanBlock = kRankScanSlices * kRankBins;
constexpr int kRankXp = 64;                          // transpose tile edge of the key kernel
constexpr uint32_t kRankTop = 0xFFFFFFFFu;           // key of NaN / +-Inf
static_assert(kRankPer * kBlock == kRankTile && kRankWaveKeys == kRankPer * kWave, "a wave owns kRankPer runs of 64 keys");

struct RankPlan {
    int64_t S, ntile, tiles;                // pooled values per coordinate, tiles per segment, tiles in all
    int64_t off_keys, off_alt, off_hist;    // bytes into work: [order statistics (d, 4) fp64] [keys] [keys] [hist]
    int64_t total;                          // bytes
};

inline RankPlan rank_plan(int64_t n_draws, int64_t n, int d) {
    RankPlan p;
    p.S = n_draws * n;
    p.ntile = (p.S + kRankTile - 1) / kRankTile;
    p.tiles = p.ntile * d;
    p.off_keys = (int64_t)d * 4 * (int64_t)sizeof(double);
    p.off_alt = p.off_keys + p.S * d * (int64_t)sizeof(uint32_t);
    p.off_hist = p.off_alt + p.S * d * (int64_t)sizeof(uint32_t);
    p.total = p.off_hist + p.tiles * kRankBins * (int64_t)sizeof(uint32_t);
    return p;
}

__device__ __forceinline__ uint32_t rank_key(float v) {
    const uint32_t b = __float_as_uint(v);
    if ((b << 1) == 0u) return 0x80000000u;                       // +-0 (bits, so a flushed denormal is not one of them)
    if ((b & 0x7F800000u) == 0x7F800000u) return kRankTop;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ double rank_key_value(uint32_t k) {
    return (double)__uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);   // the top key comes back as NaN
}

__global__ void __launch_bounds__(kBlock) rank_key_kernel(const float* __restrict__ x, int64_t S, int d,
                                                          uint32_t* __restrict__ keys) {
    __shared__ uint32_t tile[kRankXp][kRankXp + 1];
    const int tx = threadIdx.x & (kRankXp - 1), ty = threadIdx.x / kRankXp;
    const int ncb = (d + kRankXp - 1) / kRankXp;
    const int64_t nsb = (S + kRankXp - 1) / kRankXp, total = nsb * ncb;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const int64_t s0 = (t / ncb) * kRankXp;
        const int c0 = (int)(t % ncb) * kRankXp;
#pragma unroll
        for (int r = ty; r < kRankXp; r += kBlock / kRankXp) {
            const int64_t s = s0 + r;
            if (s < S && c0 + tx < d) tile[r][tx] = rank_key(x[s * d + c0 + tx]);
        }
        __syncthreads();
#pragma unroll
        for (int r = ty; r < kRankXp; r += kBlock / kRankXp) {
            const int c = c0 + r;
            if (c < d && s0 + tx < S) keys[(int64_t)c * S + s0 + tx] = tile[tx][r];
        }
        __syncthreads();
    }
}

// hist (tiles, 256): the digit counts of every tile
__global__ void __launch_bounds__(kBlock) rank_hist_kernel(const uint32_t* __restrict__ keys, int64_t S, int64_t ntile,
                                                           int64_t tiles, int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kRankBins];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t c = tile / ntile, s0 = (tile - c * ntile) * kRankTile;
        h[threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t* seg = keys + c * S;
#pragma unroll
        for (int r = 0; r < kRankPer; ++r) {
            const int64_t s = s0 + r * kBlock + threadIdx.x;
            if (s < S) atomicAdd(&h[(seg[s] >> shift) & (kRankBins - 1)], 1u);
        }
        __syncthreads();
        hist[tile * kRankBins + threadIdx.x] = h[threadIdx.x];
    }
}

// per coordinate, in place: hist[tile][digit] -> the number of keys of the segment with a smaller digit, or with this digit in
// an earlier tile.  Thread (slice q, digit b) takes the tiles of its quarter of the segment.
__global__ void __launch_bounds__(kRankScanBlock) rank_scan_kernel(uint32_t* __restrict__ hist, int64_t ntile, int d) {
    __shared__ uint32_t part[kRankScanSlices][kRankBins];
    __shared__ uint32_t base[kRankBins];
    const int b = threadIdx.x & (kRankBins - 1), q = threadIdx.x / kRankBins;
    const int64_t per = (ntile + kRankScanSlices - 1) / kRankScanSlices;
    const int64_t t0 = q * per, t1 = t0 + per < ntile ? t0 + per : ntile;
    for (int c = blockIdx.x; c < d; c += gridDim.x) {
        uint32_t* h = hist + (int64_t)c * ntile * kRankBins + b;
        uint32_t sum = 0u;
#pragma unroll 8
        for (int64_t t = t0; t < t1; ++t) sum += h[t * kRankBins];
        part[q][b] = sum;
        __syncthreads();
        if (threadIdx.x < kWave) {   // one wave: the 256 digit totals, four per lane, then a scan over the lanes
            uint32_t tot[4], lane_sum = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tot[k] = 0u;
#pragma unroll
                for (int s = 0; s < kRankScanSlices; ++s) tot[k] += part[s][4 * threadIdx.x + k];
                lane_sum += tot[k];
            }
            uint32_t incl = lane_sum;
#pragma unroll
            for (int m = 1; m < kWave; m <<= 1) {
                const uint32_t up = __shfl_up(incl, m, kWave);
                if ((int)threadIdx.x >= m) incl += up;
            }
            uint32_t run = incl - lane_sum;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                base[4 * threadIdx.x + k] = run;
                run += tot[k];
            }
        }
        __syncthreads();
        uint32_t run = base[b];
        for (int s = 0; s < q; ++s) run += part[s][b];
#pragma unroll 8
        for (int64_t t = t0; t < t1; ++t) {
            const uint32_t v = h[t * kRankBins];
            h[t * kRankBins] = run;
            run += v;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) rank_scatter_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                              int64_t S, int64_t ntile, int64_t tiles, int shift,
                                                              const uint32_t* __restrict__ offs) {
    __shared__ uint32_t wh[kWavesPerBlock][kRankBins];   // per wave: the digit counts, then the running place of each digit
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t below = (1ull << lane) - 1ull;
    volatile uint32_t* mine = wh[wave];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t c = tile / ntile, s0 = (tile - c * ntile) * kRankTile + wave * kRankWaveKeys;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) wh[w][threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t* seg = src + c * S;
        uint32_t key[kRankPer];
#pragma unroll
        for (int r = 0; r < kRankPer; ++r) {
            const int64_t s = s0 + r * kWave + lane;
            key[r] = s < S ? seg[s] : 0u;
            if (s < S) atomicAdd(&wh[wave][(key[r] >> shift) & (kRankBins - 1)], 1u);
        }
        __syncthreads();
        {   // thread = digit: the segment-wide place of the tile's first key with it, handed on from wave to wave
            uint32_t run = offs[tile * kRankBins + threadIdx.x];
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) {
                const uint32_t cnt = wh[w][threadIdx.x];
                wh[w][threadIdx.x] = run;
                run += cnt;
            }
        }
        __syncthreads();
        uint32_t* out = dst + c * S;
#pragma unroll
        for (int r = 0; r < kRankPer; ++r) {
            const bool ok = s0 + r * kWave + lane < S;
            const uint32_t digit = (key[r] >> shift) & (kRankBins - 1);
            uint64_t same = __ballot(ok);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (digit >> bit) & 1u;
                const uint64_t vote = __ballot(one);
                same &= one ? vote : ~vote;
            }
            const uint32_t before = (uint32_t)__popcll(same & below);
            uint32_t place = 0u;
            if (ok) place = mine[digit];
            __builtin_amdgcn_wave_barrier();
            if (ok) {
                out[place + before] = key[r];
                if (before == 0u) mine[digit] = place + (uint32_t)__popcll(same);   // the lowest lane of the digit moves its base on
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int64_t rank_lower(const uint32_t* __restrict__ seg, int64_t S, uint32_t key) {
    int64_t lo = 0, hi = S;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t rank_upper(const uint32_t* __restrict__ seg, int64_t S, uint32_t key) {
    int64_t lo = 0, hi = S;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ostat (d, 4): x_(floor((S-1)/20)), x_(floor((S-1)/2)), x_(ceil((S-1)/2)), x_(ceil(19 (S-1)/20)); NaN where the order
// statistic is a non-finite value.  `copy` (the caller's order_stats) may be NULL.
__global__ void __launch_bounds__(kBlock) rank_stats_kernel(const uint32_t* __restrict__ keys, int64_t S, int d,
                                                            double* __restrict__ ostat, double* __restrict__ copy,
                                                            int32_t* __restrict__ nonfinite) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= d) return;
    const uint32_t* seg = keys + (int64_t)c * S;
    const int64_t idx[4] = {(S - 1) / 20, (S - 1) / 2, S / 2, (19 * (S - 1) + 19) / 20};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double v = rank_key_value(seg[idx[k]]);
        ostat[4 * c + k] = v;
        if (copy) copy[4 * c + k] = v;
    }
    nonfinite[c] = (int32_t)(S - rank_lower(seg, S, kRankTop));
}

__global__ void __launch_bounds__(kBlock) rank_fold_kernel(const float* __restrict__ x, int64_t total, int d,
                                                           const double* __restrict__ ostat, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(i % d);
        const double med = 0.5 * (ostat[4 * c + 1] + ostat[4 * c + 2]);
        out[i] = (float)fabs((double)x[i] - med);
    }
}

// Wichura's AS 241, PPND16: the normal quantile to about 1e-16 relative
__device__ __forceinline__ double rank_ppnd16(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                               2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                            4.2313330701600911252e+1) * r + 1.0;
        return num / den;
    }
    double r = sqrt(-log(q <= 0.0 ? p : 1.0 - p));
    double num, den;
    if (r <= 5.0) {
        r -= 1.6;
        num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                  1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
               4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
        den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                  1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
               2.05319162663775882187e+0) * r + 1.0;
    } else {
        r -= 5.0;
        num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                  2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
               5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
        den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                  7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
               5.99832206555888793769e-1) * r + 1.0;
    }
    const double z = num / den;
    return q < 0.0 ? -z : z;
}

// `v` is the slab whose keys were sorted (x, or the folded values in `out` itself: each thread reads its element before it
// writes it).  series FOLDED ranks like BULK.  A coordinate with a non-finite value of x is NaN throughout.
__global__ void __launch_bounds__(kBlock) rank_emit_kernel(const float* v, int64_t S, int d, int series,
                                                           const uint32_t* __restrict__ keys,
                                                           const double* __restrict__ ostat,
                                                           const int32_t* __restrict__ nonfinite, float* out) {
    const int64_t total = S * d;
    const double denom = (double)S + 0.25;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(i % d);
        const float val = v[i];
        float res;
        if (nonfinite[c] > 0) {
            res = __uint_as_float(0x7FC00000u);
        } else if (series == NFMC_RANK_TAIL_LOW) {
            res = (double)val <= ostat[4 * c] ? 1.f : 0.f;
        } else if (series == NFMC_RANK_TAIL_HIGH) {
            res = (double)val >= ostat[4 * c + 3] ? 1.f : 0.f;
        } else {
            const uint32_t key = rank_key(val);
            const uint32_t* seg = keys + (int64_t)c * S;
            const int64_t lo = rank_lower(seg, S, key), hi = rank_upper(seg, S, key);
            const double r = 0.5 * (double)(lo + hi + 1);
            res = (float)rank_ppnd16((r - 0.375) / denom);   // a division: all ties give 0.5 exactly, z = 0
        }
        out[i] = res;
    }
}

}  // namespace nfmc
