// Shared device helpers for the nfmc gfx950 kernels: Philox4x32-10, Box-Muller on the hardware
// transcendentals, chain-group reductions, closed-form potentials, deterministic statistics.
// gfx950 only: wave = 64 lanes, no portability layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nfmc_hip.h"

namespace nfmc {

constexpr int kWave = 64;
constexpr int kBlock = 256;          // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxGrid = 2048;       // 256 CUs x 8 workgroups; larger problems grid-stride (1024 measured 4 % slower).
                                     // Also the row count of the statistics slab the fold kernel walks.
#ifndef NFMC_WPE
#define NFMC_WPE 1
#endif
constexpr int kStatTail = 4;         // per-workgroup scratch tail: accepted, nonfinite, jump accepted, jump nonfinite

// Wave mask with the bit of the first lane of every group of LPC lanes (LPC a power of 2): one chain's lanes agree on
// every per-chain predicate, so a ballot & leaders counts chains
constexpr unsigned long long group_leaders(int lpc) {
    unsigned long long m = 0;
    for (int lane = 0; lane < kWave; lane += lpc) m |= 1ull << lane;
    return m;
}
static_assert(group_leaders(1) == ~0ull && group_leaders(4) == 0x1111111111111111ull && group_leaders(64) == 1ull, "");

// RNG stream tags (oracle/philox.py)
constexpr uint32_t kTagNoise = 0, kTagAccept = 1, kTagLatent = 2, kTagJump = 3;

// ------------------------------------------------------------------------------------------------
// Philox4x32-R (Salmon et al. SC'11); R = 10 is the library's stream, R = 7 an opt-in one (NfmcRng.rounds: the
// smallest round count the Random123 authors report as passing BigCrush, 30 % fewer generator instructions).  The key
// schedule is wave-uniform, so the compiler keeps the round keys in SGPRs; the 32x32->64 products become
// v_mad_u64_u32, the two xors of a word one v_bitop3_b32.
// UC1: the caller guarantees c1 is wave-uniform (the step of a sampler transition).  Round 0's c1 ^ k0 is then one s_xor
// on the SALU and the word one VOP2 v_xor_b32 with that SGPR: v_bitop3_b32 is VOP3, which reads one SGPR at most on gfx9,
// so with c1 and k0 both in SGPRs it needs a v_mov first.  Same bits either way.
// Measured and not kept: the round keys as per-lane copies in VGPRs.  Alone, v_bitop3_b32 issues 12 % faster without an
// SGPR operand (tools/ubench.hip), but in mala_kernel's step loop the 19 extra VGPRs (74 -> 92) bought nothing: 224-226 us
// per launch with them against 221 us without, at the C3 shape.
template <int R, bool UC1 = false>
__device__ __forceinline__ uint4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        // gfx950's three-input bit op (truth table 0x96 = a ^ b ^ c): one VOP3 instead of two dependent v_xor --
        // the compiler does not form it by itself; mala_kernel 0.327 -> 0.291 ms per launch (tools/ubench.hip:
        // v_bitop3_b32 with an SGPR key issues at 1.31x a v_fma, the xor pair at 1.5x, and the chain is one op shorter)
        const uint32_t n0 = (UC1 && r == 0) ? (uint32_t)(p1 >> 32) ^ (c1 ^ k0)
                                            : __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}
__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
    return philox4x32<10>(c0, c1, c2, c3, k0, k1);
}
// NfmcRng.rounds: 0 and 10 mean Philox4x32-10; 7 is the opt-in stream; anything else is an argument error
inline int rng_rounds(const NfmcRng& r) { return r.rounds == 0 ? 10 : (int)r.rounds; }
inline bool rng_rounds_ok(const NfmcRng& r, bool seven_supported) {
    return r.rounds == 0 || r.rounds == 10 || (r.rounds == 7 && seven_supported);
}
// for entry points that only have the default stream: 0 ok, NFMC_EUNSUPPORTED for the opt-in one, NFMC_EINVAL otherwise
inline int rng_default_only(const NfmcRng& r) {
    return (r.rounds == 0 || r.rounds == 10) ? NFMC_OK : (r.rounds == 7 ? NFMC_EUNSUPPORTED : NFMC_EINVAL);
}

// (0,1) uniform with 23 random bits, exact in fp32: (2 (r >> 9) + 1) 2^-24.
__device__ __forceinline__ float u32_to_uniform(uint32_t r) {
    return (float)(2u * (r >> 9) + 1u) * 0x1p-24f;
}

// Two standard normals from two words.  v_log_f32 is log2, v_cos/v_sin take revolutions, so
// R = sqrt(-2 ln2 log2 u1), angle = u2 -- no 2 pi multiply and no range reduction.
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& za, float& zb) {
    const float u1 = fmaf((float)ra, 0x1p-32f, 0x1p-33f);
    const float u2 = (float)rb * 0x1p-32f;
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    za = rad * __builtin_amdgcn_cosf(u2);
    zb = rad * __builtin_amdgcn_sinf(u2);
}

// box_muller with each pair's two products rad * (cos, sin) as one v_pk_mul_f32: the same bits.  Written packed because
// the SLP vectorizer forms the packed multiply in some instantiations of a kernel and not in others.
typedef float nfmc_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ nfmc_f2 box_muller_pk(uint32_t ra, uint32_t rb) {
    const float u1 = fmaf((float)ra, 0x1p-32f, 0x1p-33f);
    const float u2 = (float)rb * 0x1p-32f;
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    const nfmc_f2 cs = {__builtin_amdgcn_cosf(u2), __builtin_amdgcn_sinf(u2)};
    return cs * rad;
}

// Four normals for coordinate block `blk` of (chain, step) on stream `tag`.
template <int R = 10>
__device__ __forceinline__ void philox_normal4(uint32_t chain, uint32_t step, uint32_t blk, uint32_t tag, uint32_t k0,
                                               uint32_t k1, float (&z)[4]) {
    const uint4 r = philox4x32<R>(chain, step, blk, tag, k0, k1);
    box_muller(r.x, r.y, z[0], z[1]);
    box_muller(r.z, r.w, z[2], z[3]);
}

__device__ __forceinline__ uint32_t pick_word(const uint4& r, uint32_t i) {
    return i == 0 ? r.x : (i == 1 ? r.y : (i == 2 ? r.z : r.w));
}

// natural log on v_log_f32 (log2): |err| <~ 1 ulp of log2 -- used for the Metropolis test log(u).
__device__ __forceinline__ float fast_ln(float v) { return 0.6931471805599453f * __builtin_amdgcn_logf(v); }
__device__ __forceinline__ float fast_exp(float v) { return __builtin_amdgcn_exp2f(1.4426950408889634f * v); }

// ------------------------------------------------------------------------------------------------
// Butterfly all-reduce over the LPC consecutive lanes that share one chain.  fp add is commutative,
// so every lane of the group ends with the bitwise same sum: the accept decision needs no broadcast.
// Steps inside a 16-lane row are DPP moves on the VALU (quad_perm for xor 1/2, row_half_mirror and
// row_mirror pair the already-uniform halves for 8 and 16 lanes); only 32/64-lane groups go through the
// LDS crossbar (ds_bpermute).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false);
    return v + __int_as_float(moved);
}

// Per-lane select with the condition in an SGPR pair (mask = __ballot(cond)).  Measured on gfx950
// (tools/ubench.hip, profiles/): the VOP2 form the compiler shrinks `c ? a : b` to, v_cndmask_b32_e32 with the
// implicit vcc, issues at 6.6x a v_fma (~22 cycles per wave instruction); the VOP3 form is 1.3x.  Hot loops
// that select a whole register row on one condition (the Metropolis update) use this; the exact-fit Gaussian MALA loop,
// which only ever replaces a row by the proposal, uses plain moves under the mask instead (assign_where below).
__device__ __forceinline__ float select_f32(uint64_t mask, float if_true, float if_false) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_false), "v"(if_true), "s"(mask));
    return r;
}

// x <- xp and sq <- sqp in the lanes of `mask`, as plain moves with exec narrowed to the mask: a v_mov_b32 issues in about
// half the time of the VOP3 select (tools/ubench.hip).  exec is saved, narrowed and restored inside ONE asm statement (the
// compiler never sees it changed), and narrowed by AND, so lanes that were off stay off.  The same values land in the same
// lanes as with select_f32.  One statement holds every move where the operand limit of an asm allows it (CPL = 8: the
// benchmark's layout); otherwise one statement per four registers.
#define NFMC_MOV4(I) \
    "v_mov_b32 %[x" #I "0], %[p" #I "0]\n v_mov_b32 %[x" #I "1], %[p" #I "1]\n v_mov_b32 %[x" #I "2], %[p" #I "2]\n v_mov_b32 %[x" #I "3], %[p" #I "3]\n"
template <int CPL>
__device__ __forceinline__ void assign_where(uint64_t mask, float (&x)[CPL], const float (&xp)[CPL], float& sq, float sqp) {
    static_assert(CPL % 4 == 0, "whole register quads");
    uint64_t saved;
    if constexpr (CPL == 8) {
        asm("s_and_saveexec_b64 %[sv], %[m]\n" NFMC_MOV4(a) NFMC_MOV4(b) "v_mov_b32 %[sq], %[sp]\n"
            "s_mov_b64 exec, %[sv]"
            : [xa0] "+v"(x[0]), [xa1] "+v"(x[1]), [xa2] "+v"(x[2]), [xa3] "+v"(x[3]), [xb0] "+v"(x[4]), [xb1] "+v"(x[5]),
              [xb2] "+v"(x[6]), [xb3] "+v"(x[7]), [sq] "+v"(sq), [sv] "=&s"(saved)
            : [pa0] "v"(xp[0]), [pa1] "v"(xp[1]), [pa2] "v"(xp[2]), [pa3] "v"(xp[3]), [pb0] "v"(xp[4]), [pb1] "v"(xp[5]),
              [pb2] "v"(xp[6]), [pb3] "v"(xp[7]), [sp] "v"(sqp), [m] "s"(mask)
            : "scc");
    } else {
#pragma unroll
        for (int i = 0; i < CPL; i += 4)
            asm("s_and_saveexec_b64 %[sv], %[m]\n" NFMC_MOV4(a) "s_mov_b64 exec, %[sv]"
                : [xa0] "+v"(x[i]), [xa1] "+v"(x[i + 1]), [xa2] "+v"(x[i + 2]), [xa3] "+v"(x[i + 3]), [sv] "=&s"(saved)
                : [pa0] "v"(xp[i]), [pa1] "v"(xp[i + 1]), [pa2] "v"(xp[i + 2]), [pa3] "v"(xp[i + 3]), [m] "s"(mask)
                : "scc");
        asm("s_and_saveexec_b64 %[sv], %[m]\n v_mov_b32 %[sq], %[sp]\n s_mov_b64 exec, %[sv]"
            : [sq] "+v"(sq), [sv] "=&s"(saved)
            : [sp] "v"(sqp), [m] "s"(mask)
            : "scc");
    }
}
#undef NFMC_MOV4

// v + (v of lane i ^ 7 within each 8 lanes), the row_half_mirror stage of group_allreduce, as ONE v_add_f32_dpp like
// the two quad_perm stages: the compiler's own lowering of dpp_add<0x141> is v_mov 0 + v_mov_dpp + v_add.  The same add
// of the same two values.  The s_nop covers the two wait states between a VALU write of v and a DPP read of it.
__device__ __forceinline__ float dpp_add_half_mirror(float v) {
    float r;
    asm("s_nop 1\n v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));
    return r;
}

// HM_ASM: the 8-lane stage through dpp_add_half_mirror (off by default: every other caller compiles as before)
template <int LPC, bool HM_ASM = false>
__device__ __forceinline__ float group_allreduce(float v) {
    if constexpr (LPC >= 2) v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]  : lane ^ 1
    if constexpr (LPC >= 4) v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]  : lane ^ 2
    if constexpr (LPC >= 8) v = HM_ASM ? dpp_add_half_mirror(v) : dpp_add<0x141>(v);  // row_half_mirror : i <-> 7 - i
    if constexpr (LPC >= 16) v = dpp_add<0x140>(v); // row_mirror           : i <-> 15 - i
    if constexpr (LPC >= 32) v += __shfl_xor(v, 16, kWave);
    if constexpr (LPC >= 64) v += __shfl_xor(v, 32, kWave);
    return v;
}

// ------------------------------------------------------------------------------------------------
// Reduce-scatter / all-gather of NU (4 or 8) per-lane values over the LPC >= NU lanes of a chain: the register
// flow kernels give each conditioner hidden unit to ONE lane class (unit = lane % NU) instead of evaluating the
// whole hidden stack redundantly on every lane.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// value of lane ^ 4: row_shl:4 into the even 4-lane banks, row_shr:4 into the odd ones
__device__ __forceinline__ float dpp_xor4(float v) {
    int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x104, 0xf, 0x5, false);
    t = __builtin_amdgcn_update_dpp(t, __float_as_int(v), 0x114, 0xf, 0xa, false);
    return __int_as_float(t);
}

// position r of an all-gathered register row holds unit (lane % NU) ^ unit_xor<NU>(r)
template <int NU>
__host__ __device__ constexpr int unit_xor(int r) {
    return NU == 8 ? (((r & 1) << 2) | (r & 2) | ((r >> 2) & 1)) : (((r & 1) << 1) | ((r >> 1) & 1));
}

// h[k] = this lane's partial of unit k.  Returns the sum over the chain's LPC lanes of unit (lane % NU), with the
// association of group_allreduce (pairs at lane distance 1, then 2, 4, ...), so both give bitwise the same sums.
template <int NU, int LPC>
__device__ __forceinline__ float group_reduce_scatter(const float (&h)[NU]) {
    static_assert((NU == 4 || NU == 8) && LPC >= NU, "one lane class per unit");
    constexpr uint64_t M0 = 0xAAAAAAAAAAAAAAAAull, M1 = 0xCCCCCCCCCCCCCCCCull, M2 = 0xF0F0F0F0F0F0F0F0ull;
    float a[NU / 2];
#pragma unroll
    for (int r = 0; r < NU / 2; ++r)
        a[r] = select_f32(M0, h[2 * r + 1], h[2 * r]) + dpp_mov<0xB1>(select_f32(M0, h[2 * r], h[2 * r + 1]));
    float c;
    if constexpr (NU == 8) {
        float b[2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
            b[r] = select_f32(M1, a[2 * r + 1], a[2 * r]) + dpp_mov<0x4E>(select_f32(M1, a[2 * r], a[2 * r + 1]));
        c = select_f32(M2, b[1], b[0]) + dpp_xor4(select_f32(M2, b[0], b[1]));
    } else {
        c = select_f32(M1, a[1], a[0]) + dpp_mov<0x4E>(select_f32(M1, a[0], a[1]));
        if constexpr (LPC >= 8) c += dpp_xor4(c);
    }
    if constexpr (LPC >= 16) c += dpp_mov<0x128>(c);  // row_ror:8 : lane ^ 8
    if constexpr (LPC >= 32) c += __shfl_xor(c, 16, kWave);
    if constexpr (LPC >= 64) c += __shfl_xor(c, 32, kWave);
    return c;
}

// v = value of unit (lane % NU); h[r] = value of unit (lane % NU) ^ unit_xor<NU>(r)
template <int NU>
__device__ __forceinline__ void group_all_gather(float v, float (&h)[NU]) {
    h[0] = v;
    if constexpr (NU == 8) {
        h[1] = dpp_xor4(h[0]);
        h[2] = dpp_mov<0x4E>(h[0]);
        h[3] = dpp_mov<0x4E>(h[1]);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[4 + r] = dpp_mov<0xB1>(h[r]);
    } else {
        h[1] = dpp_mov<0x4E>(h[0]);
        h[2] = dpp_mov<0xB1>(h[0]);
        h[3] = dpp_mov<0xB1>(h[1]);
    }
}

template <int LPC>
__device__ __forceinline__ float group_broadcast0(float v) {
    // value held by the group's first lane
    return __shfl(v, (int)(threadIdx.x & 63) & ~(LPC - 1), kWave);
}

// Sum over the lanes of a wave that hold the SAME coordinates of DIFFERENT chains (stride LPC), in fp32: the
// addends are each lane's fp32 partial sums over the launch's transitions, at most 64 of them meet here, and the
// result is widened to fp64 before it joins the other waves' sums.  Steps inside a 16-lane row are DPP moves, the
// two across rows go through ds_bpermute: for LPC = 8 one DPP + two permutes per value instead of the six permutes
// and three v_add_f64 of a double butterfly (the epilogue was ~25 % of a one-tile-per-wave flow-MH launch).
template <int LPC>
__device__ __forceinline__ float cross_chain_reduce(float v) {
    if constexpr (LPC <= 1) v = dpp_add<0xB1>(v);
    if constexpr (LPC <= 2) v = dpp_add<0x4E>(v);
    if constexpr (LPC <= 4) v += dpp_xor4(v);
    if constexpr (LPC <= 8) v += dpp_mov<0x128>(v);   // row_ror:8 : lane ^ 8 within the row
    if constexpr (LPC <= 16) v += __shfl_xor(v, 16, kWave);
    if constexpr (LPC <= 32) v += __shfl_xor(v, 32, kWave);
    return v;
}

// ------------------------------------------------------------------------------------------------
// Register layout of a chain ("interleaved 4-blocks"): lane g of the chain's LPC lanes holds, in register i,
// coordinate 4 * ((i / 4) * LPC + g) + (i % 4): 4-coordinate blocks dealt round-robin over the lanes.
// One register quad = one Philox block = one 16-byte global access; consecutive lanes touch consecutive
// 16-byte pieces of the row (coalesced); with d = CPL * LPC, quad q of every lane lies in the q-th 1/(CPL/4)
// of the coordinates, which flow_b.hpp uses to give coupling layers compile-time source/target roles.
template <int CPL, int LPC>
__device__ __forceinline__ int coord_of(int g, int i) {
    return 4 * ((i >> 2) * LPC + g) + (i & 3);
}

// ------------------------------------------------------------------------------------------------
// Potentials.  `term` is the coordinate's share of U (U = group sum of terms), `grad` dU/dx_c.
// Coordinates beyond d carry a = 0 / x = 0 so they contribute exactly zero.
template <int CPL, int LPC, bool FAST>
struct QuadraticPot {
    // U = sum a_c (x_c - b_c)^2
    static constexpr bool kQuadratic = true;
    static constexpr bool kStaged = false;   // parameters in registers (no LDS block, see MixturePot)
    float a_s, b_s;
    float a[FAST ? 1 : CPL], b[FAST ? 1 : CPL];
    struct Ctx {};

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        a_s = p.a_scalar;
        b_s = p.b_scalar;
        if constexpr (!FAST) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = coord_of<CPL, LPC>(g, i);
                const bool ok = c < d;
                a[i] = ok ? (p.a ? p.a[c] : p.a_scalar) : 0.f;
                b[i] = ok ? (p.b ? p.b[c] : p.b_scalar) : 0.f;
            }
        }
    }
    __device__ __forceinline__ Ctx prepare(const float (&)[CPL], int, int) const { return Ctx{}; }
    __device__ __forceinline__ float aa(int i) const { return FAST ? a_s : a[FAST ? 0 : i]; }
    __device__ __forceinline__ float bb(int i) const { return FAST ? b_s : b[FAST ? 0 : i]; }
    __device__ __forceinline__ float grad(const Ctx&, int i, float x) const { return 2.f * aa(i) * (x - bb(i)); }
    __device__ __forceinline__ float term(const Ctx&, int i, float x) const {
        const float t = x - bb(i);
        return aa(i) * t * t;
    }
};

template <int CPL, int LPC, bool FAST>
struct FunnelPot {
    // U = x0^2/(2 s^2) + sum_{i>=1} [ x_i^2 e^{-x0} / 2 + x0 / 2 ]
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    float inv_s2, half_dm1;
    bool lead;          // this lane holds coordinate 0 in register 0
    float valid[CPL];   // 1 for real coordinates, 0 for padding
    struct Ctx {
        float x0, e, s;  // x_0, exp(-x_0), sum_{i>=1} x_i^2
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        inv_s2 = 1.f / (p.a_scalar * p.a_scalar);
        half_dm1 = 0.5f * (float)(d - 1);
        lead = (g == 0);
#pragma unroll
        for (int i = 0; i < CPL; ++i) valid[i] = coord_of<CPL, LPC>(g, i) < d ? 1.f : 0.f;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        Ctx c;
        c.x0 = group_broadcast0<LPC>(x[0]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) s = fmaf(x[i], (lead && i == 0) ? 0.f : x[i], s);
        c.s = group_allreduce<LPC>(s);
        c.e = fast_exp(-c.x0);
        return c;
    }
    __device__ __forceinline__ float grad(const Ctx& c, int i, float x) const {
        const float g0 = c.x0 * inv_s2 - 0.5f * c.e * c.s + half_dm1;
        return (lead && i == 0) ? g0 : x * c.e * valid[i];
    }
    __device__ __forceinline__ float term(const Ctx& c, int i, float x) const {
        const float t0 = 0.5f * c.x0 * c.x0 * inv_s2 + half_dm1 * c.x0;
        return (lead && i == 0) ? t0 : 0.5f * c.e * x * x;
    }
};

// Diagonal Gaussian mixture (NFMC_POT_GAUSSIAN_MIXTURE, K = p.n_components <= kMixMaxK):
//   U = -logsumexp_k [ c_k - 1/2 sum_j lam_kj (x_j - mu_kj)^2 ]
//   dU/dx_j = sum_k r_k lam_kj (x_j - mu_kj),   r_k = softmax_k(e_k)
// Every chain group of a workgroup reads the same (lam, mu) rows, so they are staged ONCE per workgroup in LDS
// (stage(), before init()), padded to the layout's DP coordinates with lam = mu = 0 -- padding lanes then add exactly
// zero to every sum and get a zero gradient.  A lane reads its register quad q of row k as one ds_read_b128 at
// coordinate 4 (q LPC + g): consecutive lanes read consecutive 16 bytes, the chain groups of a wave the same ones
// (broadcast).  The c_k are wave-uniform and stay in registers.  prepare() does K group reductions (one butterfly
// each), the logsumexp on the fast exp2 / log2 helpers, and the gradient of the lane's coordinates in a second pass
// over the rows; term() puts the whole U on coordinate 0 of lane 0 (the FunnelPot trick).
constexpr int kMixMaxK = 8;

__host__ __device__ inline int mixture_floats(int k, int dp) { return 2 * k * dp; }

// argument check of a kind-2 descriptor (the check of its row in kPotKinds, as the check_* below are of theirs)
inline int check_mixture(const NfmcPotential& p, int) {
    if (!p.a || !p.b || p.n_components < 1) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0 || (((uintptr_t)p.b) & 15u) != 0) return NFMC_EALIGN;
    if (p.n_components > kMixMaxK) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

// Bayesian logistic regression (NFMC_POT_LOGISTIC_REGRESSION; X (N, d) row-major in a, y (N,) in {0, 1} in b,
// N = p.n_components, 1/s^2 = a_scalar):
//   U = sum_i [softplus(z_i) - y_i z_i] + |x|^2 / (2 s^2),   z_i = X_i . x,   softplus(z) = max(z, 0) + log1p(e^-|z|)
//   dU/dx = X^T (sigmoid(z) - y) + x / s^2
// X does not fit in LDS, and every chain of a workgroup reads the same rows, so prepare() streams it through one LDS tile
// of kLogRegTileFloats floats: logreg_tile_rows(DP) rows padded to DP coordinates with zeros, their labels behind them.
// The whole workgroup loads a tile between two barriers, so every thread of the workgroup must call prepare() equally
// often: the sampler and flow-MH kernels call it in workgroup-uniform control flow only.  Per batch of 4 rows a lane
// forms its partial dot products from one ds_read_b128 per register quad and row (consecutive lanes read consecutive
// 16 bytes, the chain groups of a wave the same ones: broadcast).  LPC >= 4: ONE reduce-scatter over the batch
// (group_reduce_scatter<4>) leaves z of row g & 3 on lane g, which alone evaluates that row's softplus and sigmoid, and
// four quad_perm broadcasts hand every lane the batch's residuals sigmoid(z) - y for the gradient pass over the same
// rows.  LPC < 4: one butterfly per row.  No cap on N: the cost is 2 N d FMAs per chain and evaluation.
constexpr int kLogRegTileFloats = 4096;   // the X part of a tile: 16 KB

__host__ __device__ inline int logreg_tile_rows(int dp) { return kLogRegTileFloats / dp; }   // dp: a power of 2, 4 .. 1024
__host__ __device__ inline int logreg_floats(int dp) { return logreg_tile_rows(dp) * (dp + 1); }

// argument check of a kind-3 descriptor
inline int check_logreg(const NfmcPotential& p, int) {
    if (!p.a || !p.b || p.n_components < 1 || !(p.a_scalar > 0.f && p.a_scalar <= 3.0e38f)) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0) return NFMC_EALIGN;
    return NFMC_OK;
}

// argument check of a kind-4 descriptor: Lambda (d, d) and mu (d,) present, n_components = d, Lambda 16-byte aligned
inline int check_fullrank(const NfmcPotential& p, int d) {
    if (!p.a || !p.b || p.n_components != d || (((uintptr_t)p.a) & 15u) != 0) return NFMC_EINVAL;
    return NFMC_OK;
}

// argument check of a kind-5 descriptor: mu present, block 1 .. d, a and b positive and finite
inline int check_rosenbrock(const NfmcPotential& p, int d) {
    if (!p.a || p.n_components < 1 || p.n_components > d) return NFMC_EINVAL;
    if (!(p.a_scalar > 0.f && p.a_scalar <= 3.0e38f) || !(p.b_scalar > 0.f && p.b_scalar <= 3.0e38f)) return NFMC_EINVAL;
    return NFMC_OK;
}

// argument check of a kind-6 descriptor: y and (alpha, beta) present, T = d - 3 >= 1, c_mu and c_sigma positive and finite
inline int check_sv(const NfmcPotential& p, int d) {
    if (!p.a || !p.b || p.n_components < 1 || p.n_components != d - 3) return NFMC_EINVAL;
    if (!(p.a_scalar > 0.f && p.a_scalar <= 3.0e38f) || !(p.b_scalar > 0.f && p.b_scalar <= 3.0e38f)) return NFMC_EINVAL;
    return NFMC_OK;
}

// Sparse logistic regression (kind 7): its compact tile holds DP / 2 columns of X per row (SparseLogRegPot), so twice
// the rows of a logistic-regression tile fit the same kLogRegTileFloats floats
__host__ __device__ inline int slr_tile_rows(int dp) { return kLogRegTileFloats / (dp / 2); }   // dp: a power of 2, 4 .. 1024
__host__ __device__ inline int slr_floats(int dp) { return slr_tile_rows(dp) * (dp / 2 + 1); }

// argument check of a kind-7 descriptor: X and y present, d = 2 D + 1 odd and >= 3, N >= 1, X 16-byte aligned, a and b
// positive and finite
inline int check_slr(const NfmcPotential& p, int d) {
    if (!p.a || !p.b || p.n_components < 1 || d < 3 || (d & 1) == 0) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0) return NFMC_EINVAL;
    if (!(p.a_scalar > 0.f && p.a_scalar <= 3.0e38f) || !(p.b_scalar > 0.f && p.b_scalar <= 3.0e38f)) return NFMC_EINVAL;
    return NFMC_OK;
}

// phi^4 lattice field (kind 8): the exchange block of a workgroup is one zeroed register quad and, behind it, one row of
// DP = CPL * LPC floats for each of its kBlock / LPC chains (Phi4Pot)
__host__ __device__ inline int phi4_floats(int cpl) { return 4 + kBlock * cpl; }

// argument check of a kind-8 descriptor: (m2, lam, kappa, boundary) present, rows of W = n_components sites that tile d;
// the register kernels need every row to start on a register quad, so W % 4 != 0 is a valid request they do not run
inline int check_phi4(const NfmcPotential& p, int d) {
    if (!p.a || p.n_components < 1 || d % p.n_components != 0) return NFMC_EINVAL;
    if (p.n_components % 4 != 0) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

// Item-response theory (kind 9): the exchange block of a workgroup is one row of DP + 4 floats for each of its
// kBlock / LPC chains (IrtPot; LPC = dp / cpl).  The 4 floats of padding keep every row 16-byte aligned and move
// consecutive chains 4 banks apart: see IrtPot.
__host__ __device__ inline int irt_floats(int dp, int cpl) { return (kBlock / (dp / cpl)) * (dp + 4); }

// argument check of a kind-9 descriptor: the responses and (m0, p_mu, p_a, p_b) present, 1 <= S = n_components <= d - 2
// (so Q = d - 1 - S >= 1), the responses 16-byte aligned
inline int check_irt(const NfmcPotential& p, int d) {
    if (!p.a || !p.b || p.n_components < 1 || p.n_components > d - 2) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0) return NFMC_EALIGN;
    return NFMC_OK;
}

// Varying-effects regression (kind 10): what the layout code in a_scalar says.  A side's mode (0 none, 1 shared,
// 2 varying) is also the number of its globals: (mu, s) for a varying side, the value itself for a shared one.
struct VfxLayout {
    int ma, mb;        // mode of the intercept side (1 or 2) and of the slope side (0, 1 or 2); one of them is 2
    bool known, ncp;   // known noise scales (no s_y) / non-centered group coordinates
    int gb, ng;        // coordinates of the group block (2 C when both sides vary, else C) / number of globals (2 .. 5)
    int ib, iy;        // index among the globals of the slope side's first one / of s_y
};
// false for a code that is none of the 16 valid ones (code = mode_a + 4 mode_b + 16 known + 32 non_centered).  Forced
// inline: as a call it would keep the caller's VfxLayout in scratch memory.
__host__ __device__ __forceinline__ bool vfx_layout(float code, int nc, VfxLayout& L) {
    if (!(code >= 0.f && code < 64.f)) return false;
    const int ic = (int)code;
    if ((float)ic != code) return false;
    L.ma = ic & 3;
    L.mb = (ic >> 2) & 3;
    L.known = (ic >> 4) & 1;
    L.ncp = (ic >> 5) & 1;
    if (L.ma < 1 || L.ma > 2 || L.mb > 2 || (L.ma != 2 && L.mb != 2)) return false;
    L.gb = (L.ma == 2 && L.mb == 2) ? 2 * nc : nc;
    L.ib = L.ma;
    L.iy = L.ib + L.mb;
    L.ng = L.iy + (L.known ? 0 : 1);
    return true;
}

// argument check of a kind-10 descriptor: the group table and (P, Hh) present, 1 <= C = n_components, a valid layout
// code, d = group block + globals of that code, N = b_scalar positive and finite when the noise is unknown, the table
// 16-byte aligned
inline int check_vfx(const NfmcPotential& p, int d) {
    VfxLayout L;
    if (!p.a || !p.b || p.n_components < 1 || p.n_components > d) return NFMC_EINVAL;
    if (!vfx_layout(p.a_scalar, p.n_components, L) || L.gb + L.ng != d) return NFMC_EINVAL;
    if (!L.known && !(p.b_scalar > 0.f && p.b_scalar <= 3.0e38f)) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0) return NFMC_EALIGN;
    return NFMC_OK;
}

// Interacting particles (kind 11): the exchange block of a workgroup is one row of DP + 4 floats for each of its
// kBlock / LPC chains, the block of kind 9 (ParticlePot)
__host__ __device__ inline int particles_floats(int dp, int cpl) { return irt_floats(dp, cpl); }

// argument check of a kind-11 descriptor: the parameter block present, P = n_components >= 2 particles of D = d / P in
// 1 .. 3 dimensions with d = P D (the check sees host values only, so D is recovered from d), the block 16-byte aligned;
// d > 1024 is a valid request no kernel runs
inline int check_particles(const NfmcPotential& p, int d) {
    if (!p.a || p.n_components < 2 || d < p.n_components || d % p.n_components != 0 || d / p.n_components > 3) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0) return NFMC_EALIGN;
    if (d > 1024) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

// Latent Gaussian model (kind 12): what the code in a_scalar says (likelihood + 4 whitened).  false for a value that is
// none of 0, 1, 2, 4, 5, 6.
__host__ __device__ __forceinline__ bool latent_code(float code, int& lik, bool& white) {
    if (!(code >= 0.f && code < 8.f)) return false;
    const int ic = (int)code;
    if ((float)ic != code) return false;
    lik = ic & 3;
    white = (ic >> 2) & 1;
    return lik < 3;
}
// floats of a kind-12 table row: rows m, y, w start 8 + k latent_row(d) floats into b
__host__ __device__ inline int latent_row(int d) { return 4 * ((d + 3) / 4); }

// argument check of a kind-12 descriptor: the matrix block and the table present, n_components = d, a valid code, both
// blocks 16-byte aligned; d > 1024 is a valid request no kernel runs
inline int check_latent(const NfmcPotential& p, int d) {
    int lik;
    bool white;
    if (!p.a || !p.b || p.n_components != d || !latent_code(p.a_scalar, lik, white)) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0 || (((uintptr_t)p.b) & 15u) != 0) return NFMC_EALIGN;
    if (d > 1024) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

// Latent Gaussian Markov random field (kind 13): what the code in a_scalar says (likelihood + 4 [tau unknown] +
// 8 [scaled]).  false for a value that is none of 0, 1, 2, 4, 5, 6, 12, 13, 14 (scaled needs tau unknown).
__host__ __device__ __forceinline__ bool gmrf_code(float code, int& lik, bool& tau, bool& scaled) {
    if (!(code >= 0.f && code < 16.f)) return false;
    const int ic = (int)code;
    if ((float)ic != code) return false;
    lik = ic & 3;
    tau = (ic >> 2) & 1;
    scaled = (ic >> 3) & 1;
    return lik < 3 && (tau || !scaled);
}

// argument check of a kind-13 descriptor: the ELL block and the table present, 1 <= W = n_components, a valid code,
// d >= 1 (d >= 2 with tau unknown: d = n + 1), both blocks 16-byte aligned; W > 32 or d > 1024 is a valid request no
// kernel runs.  The column indices are device data the check never sees: the kernels clamp them.
inline int check_gmrf(const NfmcPotential& p, int d) {
    int lik;
    bool tau, scaled;
    if (!p.a || !p.b || p.n_components < 1 || !gmrf_code(p.a_scalar, lik, tau, scaled)) return NFMC_EINVAL;
    if (d < (tau ? 2 : 1)) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0 || (((uintptr_t)p.b) & 15u) != 0) return NFMC_EALIGN;
    if (p.n_components > 32 || d > 1024) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

// Diffusion bridge (kind 14): what the code in a_scalar says (drift + 4 [scales unknown] + 8 (m - 1)).  false for a value
// that is no such integer, for a drift code past 2 and for an m the drift does not take (cubic 1 .. 3, fitzhugh_nagumo 2,
// lorenz63 3).
__host__ __device__ __forceinline__ bool diffusion_code(float code, int& drift, bool& unk, int& m) {
    if (!(code >= 0.f && code < 32.f)) return false;
    const int ic = (int)code;
    if ((float)ic != code) return false;
    drift = ic & 3;
    unk = (ic >> 2) & 1;
    m = (ic >> 3) + 1;
    return drift < 3 && m <= 3 && (drift != 1 || m == 2) && (drift != 2 || m == 3);
}

// the 16 floats of a kind-14 header (p.a): indices
enum { kDifDt = 0, kDifSigma, kDifTau, kDifMu0, kDifIs0, kDifLoc, kDifIc2, kDifNobs, kDifTm1m, kDifPar0, kDifHeader = 16 };

// argument check of a kind-14 descriptor: the header and the rows y, w present, T = n_components >= 2, a valid code with
// an m that fits the drift, d = T m + 2 [scales unknown], both blocks 16-byte aligned; d > 1024 is a valid request no
// kernel runs
inline int check_diffusion(const NfmcPotential& p, int d) {
    int drift, m;
    bool unk;
    if (!p.a || !p.b || p.n_components < 2 || !diffusion_code(p.a_scalar, drift, unk, m)) return NFMC_EINVAL;
    if ((int64_t)d != (int64_t)p.n_components * m + (unk ? 2 : 0)) return NFMC_EINVAL;
    if ((((uintptr_t)p.a) & 15u) != 0 || (((uintptr_t)p.b) & 15u) != 0) return NFMC_EALIGN;
    if (d > 1024) return NFMC_EUNSUPPORTED;
    return NFMC_OK;
}

// LDS bytes a register-layout kernel with DP = CPL * LPC padded coordinates stages for `p` beside its flow image
inline size_t mixture_bytes(const NfmcPotential& p, int dp, int) { return (size_t)mixture_floats(p.n_components, dp) * sizeof(float); }
inline size_t logreg_bytes(const NfmcPotential&, int dp, int) { return (size_t)logreg_floats(dp) * sizeof(float); }
inline size_t fullrank_bytes(const NfmcPotential&, int, int) { return (size_t)kLogRegTileFloats * sizeof(float); }
inline size_t slr_bytes(const NfmcPotential&, int dp, int) { return (size_t)slr_floats(dp) * sizeof(float); }
inline size_t phi4_bytes(const NfmcPotential&, int, int cpl) { return (size_t)phi4_floats(cpl) * sizeof(float); }
inline size_t irt_bytes(const NfmcPotential&, int dp, int cpl) { return (size_t)irt_floats(dp, cpl) * sizeof(float); }
inline size_t particles_bytes(const NfmcPotential&, int dp, int cpl) { return (size_t)particles_floats(dp, cpl) * sizeof(float); }

// ------------------------------------------------------------------------------------------------
// The potential kinds, as the host sees them: one row per NFMC_POT_* value, indexed by it.  Every entry point that asks
// "does this family of kernels run the kind, and is its descriptor well formed" goes through check_potential(); every
// host decision that depends on the kind reads a column here.  Adding a potential kind:
//   1. nfmc_hip.h: its NFMC_POT_* value and descriptor fields; here: its check_* function and its row.  The check
//      answers NFMC_EINVAL / NFMC_EALIGN for a malformed descriptor and NFMC_EUNSUPPORTED for a well-formed one no
//      kernel runs (check_phi4: a row length that is no multiple of 4); it sees host values only, never what a or b
//      point to.
//   2. Its device class Pot<CPL, LPC, FAST> below (prepare / grad / term, and stage() with a *_bytes function if kStaged).
//      The *_bytes function gets the layout as (DP, CPL): a read-only table is sized by DP, a block with a slot per
//      chain by CPL (phi4_bytes), or by both where its rows are padded (irt_bytes).  A block the lanes write (Phi4Pot)
//      must not rely on workgroup barriers inside prepare() unless every thread of the workgroup calls it equally often
//      (LogRegPot's rule).  A class that reads its data straight from global memory (VaryEffPot) has kStaged = false,
//      the three-argument init(p, g, d) and nullptr for the *_bytes function in its row.
//      A class in which every coordinate meets every other (ParticlePot) exchanges the chain's state through a
//      wave-private LDS row like Phi4Pot and IrtPot; its number of registers depends on how many objects a lane owns,
//      which depends on a run-time shape (D): dispatch on that shape ONCE per prepare(), outside the loops, to bodies
//      with compile-time bounds, or a register array indexed by it goes to scratch memory.
//   3. own_units: a line in NFMC_FOR_OWN_UNIT_POT and four units that instantiate launch_{mala,hmc}_kind and
//      launch_b_kind{,_rqs} for the class (sampler_slr_mala.hip and its three siblings are the pattern).  The build
//      picks up every .hip file of this directory; a unit that takes a minute or more also goes into SLOW_FIRST
//      (nfmc_amd/build.py).
//   4. neutra_valu: its *_value_grad_row and its arm of adjusted_potential_grad_row (neutra_kernels.hpp), and its class
//      in the tuple of NeuTra._min_hidden (nfmc_amd/samplers/neutra.py) that keeps it off the matrix-core kernels.
//   5. Python: POT_* in nfmc_amd/hip.py, its class in nfmc_amd/potentials.py, an fp64 oracle tests/<kind>_fp64.py and
//      tests/test_{host,gpu}_<kind>.py, which assert the codes of step 1's check.
//   6. Words: the kind's comment in nfmc_hip.h, its line in INTEGRATION.md, its paragraph in README.md and its
//      subsection of DESIGN.md 3.3 with the measured cost (a tools/probe_<kind>.py).
struct PotKind {
    int kind;
    int (*check)(const NfmcPotential&, int d);              // its own argument check (nullptr: nothing to check)
    size_t (*staged_bytes)(const NfmcPotential&, int dp, int cpl);   // the LDS block its class stages (nullptr: none)
    bool own_units;          // samplers and flow-MH: general kernels only, in translation units of its own
    bool default_cfg_only;   // samplers: instantiated at the default layouts only (is_default_cfg, sampler_impl.hpp)
    bool register_only;      // flow-MH: the register-layout kernels only (no matrix-core or one-chain-per-lane kernel)
    bool neutra_valu;        // evaluated by the VALU NeuTra kernels (neutra_kernels.hpp)
};
constexpr PotKind kPotKinds[] = {
    {NFMC_POT_QUADRATIC, nullptr, nullptr, false, false, false, true},
    {NFMC_POT_FUNNEL, nullptr, nullptr, false, false, false, true},
    {NFMC_POT_GAUSSIAN_MIXTURE, check_mixture, mixture_bytes, false, false, true, false},
    {NFMC_POT_LOGISTIC_REGRESSION, check_logreg, logreg_bytes, false, true, true, false},
    {NFMC_POT_GAUSSIAN_FULL, check_fullrank, fullrank_bytes, true, true, true, true},
    {NFMC_POT_ROSENBROCK, check_rosenbrock, nullptr, true, true, true, true},
    {NFMC_POT_STOCHASTIC_VOLATILITY, check_sv, nullptr, true, true, true, true},
    {NFMC_POT_SPARSE_LOGISTIC_REGRESSION, check_slr, slr_bytes, true, true, true, true},
    {NFMC_POT_LATTICE_PHI4, check_phi4, phi4_bytes, true, true, true, true},
    {NFMC_POT_ITEM_RESPONSE, check_irt, irt_bytes, true, true, true, true},
    {NFMC_POT_VARYING_EFFECTS, check_vfx, nullptr, true, true, true, true},
    {NFMC_POT_PARTICLES, check_particles, particles_bytes, true, true, true, true},
    {NFMC_POT_LATENT_GAUSSIAN, check_latent, fullrank_bytes, true, true, true, true},
    {NFMC_POT_LATENT_GMRF, check_gmrf, irt_bytes, true, true, true, true},
    {NFMC_POT_DIFFUSION_BRIDGE, check_diffusion, irt_bytes, true, true, true, true},
};
constexpr int kNumPotKinds = (int)(sizeof(kPotKinds) / sizeof(PotKind));
constexpr bool pot_kinds_indexed(int i = 0) { return i == kNumPotKinds || (kPotKinds[i].kind == i && pot_kinds_indexed(i + 1)); }
static_assert(pot_kinds_indexed(), "row i of kPotKinds describes kind i");
// the row of `kind`; nullptr for a value that is no kind
constexpr const PotKind* pot_kind(int kind) { return kind >= 0 && kind < kNumPotKinds ? &kPotKinds[kind] : nullptr; }

// The own_units kinds with their device classes: the explicit instantiations' extern declarations and the dispatch
// switches (sampler_impl.hpp, flow_b_mh.hpp) expand this list, and each expansion asserts the row's flag.
#define NFMC_FOR_OWN_UNIT_POT(M)                                            \
    M(NFMC_POT_GAUSSIAN_FULL, GaussFullPot) M(NFMC_POT_ROSENBROCK, RosenbrockPot) \
    M(NFMC_POT_STOCHASTIC_VOLATILITY, SVPot) M(NFMC_POT_SPARSE_LOGISTIC_REGRESSION, SparseLogRegPot) \
    M(NFMC_POT_LATTICE_PHI4, Phi4Pot) M(NFMC_POT_ITEM_RESPONSE, IrtPot) \
    M(NFMC_POT_VARYING_EFFECTS, VaryEffPot) M(NFMC_POT_PARTICLES, ParticlePot) \
    M(NFMC_POT_LATENT_GAUSSIAN, LatentGaussPot) M(NFMC_POT_LATENT_GMRF, GmrfPot) \
    M(NFMC_POT_DIFFUSION_BRIDGE, DiffusionPot)

// The families of kernels that take a potential descriptor of any kind.  (The entry points that run kinds 0 and 1 only
// say so themselves.)
enum class PotFamily { kRegister, kNeutraValu };   // samplers and flow-MH / VALU NeuTra
// NFMC_EUNSUPPORTED for a kind the family does not run, then the kind's own NFMC_EINVAL / NFMC_EALIGN / NFMC_EUNSUPPORTED
inline int check_potential(const NfmcPotential& p, int d, PotFamily family) {
    const PotKind* k = pot_kind(p.kind);
    if (!k || (family == PotFamily::kNeutraValu && !k->neutra_valu)) return NFMC_EUNSUPPORTED;
    return k->check ? k->check(p, d) : NFMC_OK;
}
inline size_t staged_potential_bytes(const NfmcPotential& p, int dp, int cpl) {
    const PotKind* k = pot_kind(p.kind);
    return k && k->staged_bytes ? k->staged_bytes(p, dp, cpl) : 0;
}

template <int CPL, int LPC, bool FAST>
struct MixturePot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    const float* tab;     // LDS: lam (K, DP) | mu (K, DP)
    float c[kMixMaxK];    // log w_k + 1/2 sum_j log lam_kj
    int nk;
    bool lead;            // this lane holds coordinate 0 in register 0
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    // all threads of the workgroup; the caller synchronises before the first prepare()
    __device__ __forceinline__ static void stage(float* __restrict__ lds, const NfmcPotential& p, int d) {
        const int kd = p.n_components * DP;
        for (int t = threadIdx.x; t < 2 * kd; t += kBlock) {
            const int half = t >= kd, r = half ? t - kd : t;
            const int k = r / DP, j = r - k * DP;
            lds[t] = j < d ? (half ? p.b : p.a)[(int64_t)k * d + j] : 0.f;
        }
    }
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, const float* lds) {
        tab = lds;
        nk = p.n_components;
        lead = (g == 0);
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) c[k] = k < nk ? p.a[(int64_t)nk * d + k] : 0.f;
    }
    __device__ __forceinline__ float4 row4(int k, int half, int q, int g) const {
        return *reinterpret_cast<const float4*>(tab + (half * nk + k) * DP + 4 * (q * LPC + g));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        float e[kMixMaxK];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) {
            e[k] = -INFINITY;
            if (k < nk) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < CPL / 4; ++q) {
                    const float4 l = row4(k, 0, q, g), mu = row4(k, 1, q, g);
                    const float t0 = x[4 * q] - mu.x, t1 = x[4 * q + 1] - mu.y, t2 = x[4 * q + 2] - mu.z,
                                t3 = x[4 * q + 3] - mu.w;
                    s = fmaf(l.x * t0, t0, s);
                    s = fmaf(l.y * t1, t1, s);
                    s = fmaf(l.z * t2, t2, s);
                    s = fmaf(l.w * t3, t3, s);
                }
                e[k] = fmaf(-0.5f, group_allreduce<LPC>(s), c[k]);
                m = fmaxf(m, e[k]);
            }
        }
        float w[kMixMaxK], sum = 0.f;
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) {
            w[k] = k < nk ? fast_exp(e[k] - m) : 0.f;   // e_k - m <= 0: no overflow; NaN propagates through sum
            sum += w[k];
        }
        Ctx cx;
        cx.u = -(m + fast_ln(sum));
        const float inv = 1.f / sum;
#pragma unroll
        for (int i = 0; i < CPL; ++i) cx.gr[i] = 0.f;
#pragma unroll
        for (int k = 0; k < kMixMaxK; ++k) {
            if (k < nk) {
                const float r = w[k] * inv;
#pragma unroll
                for (int q = 0; q < CPL / 4; ++q) {
                    const float4 l = row4(k, 0, q, g), mu = row4(k, 1, q, g);
                    cx.gr[4 * q] = fmaf(r * l.x, x[4 * q] - mu.x, cx.gr[4 * q]);
                    cx.gr[4 * q + 1] = fmaf(r * l.y, x[4 * q + 1] - mu.y, cx.gr[4 * q + 1]);
                    cx.gr[4 * q + 2] = fmaf(r * l.z, x[4 * q + 2] - mu.z, cx.gr[4 * q + 2]);
                    cx.gr[4 * q + 3] = fmaf(r * l.w, x[4 * q + 3] - mu.w, cx.gr[4 * q + 3]);
                }
            }
        }
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// softplus(z) and sigmoid(z) from one e^-|z|: finite for every finite z.  log1p(e) is ln(1 + e) on v_log_f32 for
// e >= 2^-8 and the series e - e^2/2 + e^3/3 below (relative error < 2e-8 there), where 1 + e would drop e's low bits
__device__ __forceinline__ void softplus_sigmoid(float z, float& sp, float& sg) {
    const float e = fast_exp(-fabsf(z));                 // (0, 1]; 0 for |z| past ~104
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float l1p = e < 0x1p-8f ? e * fmaf(e, fmaf(e, 1.f / 3.f, -0.5f), 1.f) : fast_ln(1.f + e);
    sp = fmaxf(z, 0.f) + l1p;
    sg = (z >= 0.f ? 1.f : e) * inv;
}

// All threads of the workgroup: rows t0 .. t0 + rows - 1 of the row-major matrix src (`cols` floats per row) into the
// kLogRegTileFloats floats of `tile` as (kLogRegTileFloats / DP, DP), zero past column `cols` and past row `rows`.  Opens
// with the barrier after which no wave reads the previous tile; the caller closes with one after its own stores.
template <int DP>
__device__ __forceinline__ void load_tile_rows(float* tile, const float* src, int cols, int t0, int rows) {
    constexpr int kPer = kLogRegTileFloats / kBlock;   // floats per thread and tile
    static_assert(kLogRegTileFloats % kBlock == 0, "whole tiles per thread");
    __syncthreads();   // every wave is done with the previous tile
    float v[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {   // all loads in flight before the first LDS write
        const int e = threadIdx.x + k * kBlock, r = e / DP, j = e % DP;
        v[k] = (j < cols && r < rows) ? src[(int64_t)(t0 + r) * cols + j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) tile[threadIdx.x + k * kBlock] = v[k];
}

template <int CPL, int LPC, bool FAST>
struct LogRegPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int T = kLogRegTileFloats / DP;   // rows per tile
    static_assert(T % 4 == 0, "batches of 4 rows");
    float* tile;          // LDS: X rows (T, DP) | y (T)
    const float* X;
    const float* y;
    int nr, dd;
    float inv_s2;
    bool lead;            // this lane holds coordinate 0 in register 0
    float valid[CPL];     // 1 for real coordinates, 0 for padding
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        X = p.a;
        y = p.b;
        nr = p.n_components;
        dd = d;
        inv_s2 = p.a_scalar;
        lead = (g == 0);
#pragma unroll
        for (int i = 0; i < CPL; ++i) valid[i] = coord_of<CPL, LPC>(g, i) < d ? 1.f : 0.f;
    }
    __device__ __forceinline__ float4 row4(int r, int q, int g) const {
        return *reinterpret_cast<const float4*>(tile + r * DP + 4 * (q * LPC + g));
    }
    // all threads of the workgroup: rows t0 .. t0 + rows - 1 into the tile, zeros past them
    __device__ __forceinline__ void load_tile(int t0, int rows) const {
        load_tile_rows<DP>(tile, X, dd, t0, rows);
        for (int r = threadIdx.x; r < T; r += kBlock) tile[T * DP + r] = r < rows ? y[t0 + r] : 0.f;
        __syncthreads();
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        Ctx cx;
        float pr = 0.f;   // this lane's share of |x|^2
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const float xv = valid[i] * x[i];
            cx.gr[i] = inv_s2 * xv;
            pr = fmaf(xv, xv, pr);
        }
        // this lane's share of the data term, summed in fp64: U is a sum of N terms of O(1), and fp32 partial sums over
        // thousands of rows lose ~sqrt(N) ulps of U -- 1e-2 in a log ratio at N = 2500 -- which fp64 keeps to the one
        // rounding of the result
        double ul = 0.0;
        const float* yt = tile + T * DP;
        for (int t0 = 0; t0 < nr; t0 += T) {
            const int rows = nr - t0 < T ? nr - t0 : T;
            load_tile(t0, rows);
            for (int r0 = 0; r0 < rows; r0 += 4) {
                float h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float4 w = row4(r0 + b, q, g);
                        s = fmaf(w.x, x[4 * q], s);
                        s = fmaf(w.y, x[4 * q + 1], s);
                        s = fmaf(w.z, x[4 * q + 2], s);
                        s = fmaf(w.w, x[4 * q + 3], s);
                    }
                    h[b] = s;
                }
                float rb[4];   // sigmoid(z) - y of the batch's rows (0 past the last row)
                if constexpr (LPC >= 4) {
                    const int b = g & 3;
                    const float z = group_reduce_scatter<4, LPC>(h);   // z of row r0 + b
                    const float yv = yt[r0 + b];
                    float sp, sg;
                    softplus_sigmoid(z, sp, sg);
                    const bool ok = r0 + b < rows;
                    if (ok && g < 4) ul += (double)(sp - yv * z);   // one lane per row
                    const float res = ok ? sg - yv : 0.f;
                    rb[0] = dpp_mov<0x00>(res);   // quad_perm [b, b, b, b]: the value of lane b of the quad
                    rb[1] = dpp_mov<0x55>(res);
                    rb[2] = dpp_mov<0xAA>(res);
                    rb[3] = dpp_mov<0xFF>(res);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float z = group_allreduce<LPC>(h[b]);
                        const float yv = yt[r0 + b];
                        float sp, sg;
                        softplus_sigmoid(z, sp, sg);
                        const bool ok = r0 + b < rows;
                        if (ok && g == 0) ul += (double)(sp - yv * z);
                        rb[b] = ok ? sg - yv : 0.f;
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float4 w = row4(r0 + b, q, g);
                        cx.gr[4 * q] = fmaf(rb[b], w.x, cx.gr[4 * q]);
                        cx.gr[4 * q + 1] = fmaf(rb[b], w.y, cx.gr[4 * q + 1]);
                        cx.gr[4 * q + 2] = fmaf(rb[b], w.z, cx.gr[4 * q + 2]);
                        cx.gr[4 * q + 3] = fmaf(rb[b], w.w, cx.gr[4 * q + 3]);
                    }
                }
            }
        }
        cx.u = group_allreduce<LPC>((float)(ul + (double)(0.5f * inv_s2 * pr)));
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Full-rank Gaussian (NFMC_POT_GAUSSIAN_FULL; Lambda (d, d) row-major in a, mu (d,) in b, d = p.n_components):
//   U = 1/2 r^T Lambda r,   dU/dx = Lambda r,   r = x - mu
// Lambda streams through the same LDS tile as the logistic regression's X (load_tile_rows: T = kLogRegTileFloats / DP
// rows of DP floats, zero-padded), so the same rule holds: every thread of the workgroup calls prepare() equally often.
// One pass over the rows: rows 4 b .. 4 b + 3 of Lambda belong to coordinates 4 b .. 4 b + 3, which are register quad
// b / LPC of lane b % LPC of the chain.  That lane's four r_i are broadcast to the chain's LPC lanes (ds_bpermute;
// v_readlane when one chain fills the wave; nothing with one lane per chain), and every lane adds r_i Lambda_ij to its
// own coordinates j: row i is column i (symmetry), read as one ds_read_b128 per register quad at 4 (q LPC + g) -- the
// gradient pass of LogRegPot with r_i in place of the residuals, no reduction per row.  U = 1/2 sum_j r_j g_j is
// lane-local, then ONE group_allreduce.  Padding coordinates have r = 0 and zero rows / columns, so d need not be a
// multiple of 4.  d^2 FMAs per chain and evaluation, d^2 / LPC per lane.
template <int CPL, int LPC, bool FAST>
struct GaussFullPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int T = kLogRegTileFloats / DP;   // rows of Lambda per tile
    static_assert(T % 4 == 0, "whole register quads per tile");
    float* tile;          // LDS: Lambda rows (T, DP)
    const float* lam;
    int dd;
    int grp;              // byte address of the chain's first lane for ds_bpermute
    bool lead;            // this lane holds coordinate 0 in register 0
    float mu[CPL];        // 0 for padding
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        lam = p.a;
        dd = d;
        grp = 4 * ((int)(threadIdx.x & 63) - g);
        lead = (g == 0);
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            mu[i] = c < d ? p.b[c] : 0.f;
        }
    }
    // value v of lane `src` (uniform) of this lane's chain group
    __device__ __forceinline__ float from_lane(float v, int src) const {
        if constexpr (LPC == 1) return v;
        else if constexpr (LPC == 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(grp + 4 * src, __float_as_int(v)));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        Ctx cx;
        float r[CPL];
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            r[i] = coord_of<CPL, LPC>(g, i) < dd ? x[i] - mu[i] : 0.f;
            cx.gr[i] = 0.f;
        }
        for (int t0 = 0; t0 < dd; t0 += T) {
            const int rows = dd - t0 < T ? dd - t0 : T;
            load_tile_rows<DP>(tile, lam, dd, t0, rows);
            __syncthreads();
            const int b1 = (t0 + rows + 3) >> 2;   // register quads (4 rows each) of this tile: t0 / 4 .. b1 - 1
            for (int b = t0 >> 2; b < b1;) {
                const int q = b / LPC;             // the quad's register index, constant over LPC consecutive quads
                float rq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < CPL / 4; ++k)
                    if (k == q) {
                        rq[0] = r[4 * k];
                        rq[1] = r[4 * k + 1];
                        rq[2] = r[4 * k + 2];
                        rq[3] = r[4 * k + 3];
                    }
                const int bq = b1 < (q + 1) * LPC ? b1 : (q + 1) * LPC;
                for (; b < bq; ++b) {
                    const int src = b - q * LPC;   // the lane that holds coordinates 4 b .. 4 b + 3
                    const float ri[4] = {from_lane(rq[0], src), from_lane(rq[1], src), from_lane(rq[2], src),
                                         from_lane(rq[3], src)};
                    const float* rows4 = tile + (4 * b - t0) * DP + 4 * g;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int k = 0; k < CPL / 4; ++k) {
                            const float4 w = *reinterpret_cast<const float4*>(rows4 + c * DP + 4 * k * LPC);
                            cx.gr[4 * k] = fmaf(ri[c], w.x, cx.gr[4 * k]);
                            cx.gr[4 * k + 1] = fmaf(ri[c], w.y, cx.gr[4 * k + 1]);
                            cx.gr[4 * k + 2] = fmaf(ri[c], w.z, cx.gr[4 * k + 2]);
                            cx.gr[4 * k + 3] = fmaf(ri[c], w.w, cx.gr[4 * k + 3]);
                        }
                    }
                }
            }
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) s = fmaf(r[i], cx.gr[i], s);
        cx.u = 0.5f * group_allreduce<LPC>(s);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Latent Gaussian model (NFMC_POT_LATENT_GAUSSIAN, nfmc_hip.h): a Gaussian prior N(m, K) on f with a likelihood term
// l_j(f_j) per coordinate.  latent_lik<LIK> is that term and its derivative for one coordinate (LIK 0 Poisson, 1 binomial,
// 2 Student-t; c0 = (nu+1)/2, c1 = 1/(nu s^2), c2 = nu s^2 of the table's header); an unobserved coordinate (w = 0, the
// padding included) gets exactly 0 for both, by a select, so that an overflowing e^f cannot turn 0 * inf into NaN.
// Shared with latent_value_grad_row (neutra_kernels.hpp).  log1p as in softplus_sigmoid.
template <int LIK>
__device__ __forceinline__ void latent_lik(float f, float y, float w, float c0, float c1, float c2, float& l, float& lp) {
    if constexpr (LIK == 0) {
        const float e = w * fast_exp(f);
        l = fmaf(-y, f, e);
        lp = e - y;
    } else if constexpr (LIK == 1) {
        float sp, sg;
        softplus_sigmoid(f, sp, sg);
        l = fmaf(w, sp, -y * f);
        lp = fmaf(w, sg, -y);
    } else {
        const float t = y - f, q = t * t, e = q * c1;
        const float l1p = e < 0x1p-8f ? e * fmaf(e, fmaf(e, 1.f / 3.f, -0.5f), 1.f) : fast_ln(1.f + e);
        l = w * c0 * l1p;
        lp = -2.f * w * c0 * t * __builtin_amdgcn_rcpf(c2 + q);
    }
    const bool on = w > 0.f;
    l = on ? l : 0.f;
    lp = on ? lp : 0.f;
}

// The device class.  centred (x = f):  U = 1/2 r^T Lambda r + sum_j l_j(x_j),  dU/dx = Lambda r + l'(x),  r = x - m;
// whitened (x = z, f = m + L z):  U = 1/2 |z|^2 + sum_j l_j(f_j),  dU/dz = z + L^T l'(f).
// matvec() is GaussFullPot's loop: the (d, d) row-major matrix M streams through the LDS tile and every lane adds
// v_i M_ij to its own coordinates j, v_i broadcast from its owner, one ds_read_b128 per register quad and row, no
// reduction per row: out += M^T v.  The centred form is one pass (M = Lambda = Lambda^T, v = r).  The whitened form is
// two passes through the same tile: M = L^T with v = z leaves L z in the lane's registers, the lane evaluates l and l'
// of its own coordinates, and M = L with v = l'(f) gives L^T l'.  The known-zero triangle of L is streamed like the
// rest.  The rows m, y, w are read from the table (global memory, one 16-byte load per register quad) where they are
// used, not held in registers across the sampler's loop.  U: lane-local sums, then ONE group_allreduce.  The tile rule
// of LogRegPot holds: every thread of the workgroup calls prepare() equally often; the parameterisation is
// workgroup-uniform, so every thread runs the same number of passes.  Likelihood and parameterisation are dispatched
// once per prepare(), outside the loops.  Padding coordinates have v = 0, zero rows / columns and w = 0.
template <int CPL, int LPC, bool FAST>
struct LatentGaussPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int T = kLogRegTileFloats / DP;   // matrix rows per tile
    static_assert(T % 4 == 0, "whole register quads per tile");
    float* tile;          // LDS: matrix rows (T, DP)
    const float* mat;     // Lambda | L^T then L
    const float* tab;     // rows m, y, w of d4 floats (behind the 8 floats of the header)
    int dd, d4;
    int grp;              // byte address of the chain's first lane for ds_bpermute
    int lik;
    bool white;
    bool lead;            // this lane holds coordinate 0 in register 0
    float c0, c1, c2;     // Student-t constants
    struct Ctx {
        float u;          // U of the chain (every lane of the group)
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        mat = p.a;
        tab = p.b + 8;
        dd = d;
        d4 = latent_row(d);
        grp = 4 * ((int)(threadIdx.x & 63) - g);
        lead = (g == 0);
        lik = 0;
        white = false;
        latent_code(p.a_scalar, lik, white);
        c0 = p.b[0];
        c1 = p.b[1];
        c2 = p.b[2];
    }
    // value v of lane `src` (uniform) of this lane's chain group
    __device__ __forceinline__ float from_lane(float v, int src) const {
        if constexpr (LPC == 1) return v;
        else if constexpr (LPC == 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(grp + 4 * src, __float_as_int(v)));
    }
    // register quad q of table row k (0 m, 1 y, 2 w) for this lane; zeros past the row
    __device__ __forceinline__ float4 tab4(int k, int q, int g) const {
        const int c = 4 * (q * LPC + g);
        return c < d4 ? *reinterpret_cast<const float4*>(tab + k * d4 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // all threads of the workgroup: out += M^T v, M (dd, dd) row-major in global memory, v = 0 on padding coordinates
    __device__ __forceinline__ void matvec(const float* __restrict__ M, const float (&v)[CPL], float (&out)[CPL], int g) const {
        for (int t0 = 0; t0 < dd; t0 += T) {
            const int rows = dd - t0 < T ? dd - t0 : T;
            load_tile_rows<DP>(tile, M, dd, t0, rows);
            __syncthreads();
            const int b1 = (t0 + rows + 3) >> 2;   // register quads (4 rows each) of this tile: t0 / 4 .. b1 - 1
            for (int b = t0 >> 2; b < b1;) {
                const int q = b / LPC;             // the quad's register index, constant over LPC consecutive quads
                float vq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < CPL / 4; ++k)
                    if (k == q) {
                        vq[0] = v[4 * k];
                        vq[1] = v[4 * k + 1];
                        vq[2] = v[4 * k + 2];
                        vq[3] = v[4 * k + 3];
                    }
                const int bq = b1 < (q + 1) * LPC ? b1 : (q + 1) * LPC;
                for (; b < bq; ++b) {
                    const int src = b - q * LPC;   // the lane that holds coordinates 4 b .. 4 b + 3
                    const float vi[4] = {from_lane(vq[0], src), from_lane(vq[1], src), from_lane(vq[2], src),
                                         from_lane(vq[3], src)};
                    const float* rows4 = tile + (4 * b - t0) * DP + 4 * g;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int k = 0; k < CPL / 4; ++k) {
                            const float4 w = *reinterpret_cast<const float4*>(rows4 + c * DP + 4 * k * LPC);
                            out[4 * k] = fmaf(vi[c], w.x, out[4 * k]);
                            out[4 * k + 1] = fmaf(vi[c], w.y, out[4 * k + 1]);
                            out[4 * k + 2] = fmaf(vi[c], w.z, out[4 * k + 2]);
                            out[4 * k + 3] = fmaf(vi[c], w.w, out[4 * k + 3]);
                        }
                    }
                }
            }
        }
    }
    // l'(f) of this lane's coordinates into lp, their share of sum_j l_j(f_j) returned
    template <int LIK>
    __device__ __forceinline__ float likelihood(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < CPL / 4; ++q) {
            const float4 y = tab4(1, q, g), w = tab4(2, q, g);
            const float yy[4] = {y.x, y.y, y.z, y.w}, ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float l;
                latent_lik<LIK>(f[4 * q + k], yy[k], ww[k], c0, c1, c2, l, lp[4 * q + k]);
                s += l;
            }
        }
        return s;
    }
    __device__ __forceinline__ float likelihood_of(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        return lik == 0 ? likelihood<0>(f, lp, g) : lik == 1 ? likelihood<1>(f, lp, g) : likelihood<2>(f, lp, g);
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        Ctx cx;
        float v[CPL], mv[CPL];   // x on the real coordinates, 0 on the padding / the prior mean
#pragma unroll
        for (int q = 0; q < CPL / 4; ++q) {
            const float4 m = tab4(0, q, g);
            mv[4 * q] = m.x;
            mv[4 * q + 1] = m.y;
            mv[4 * q + 2] = m.z;
            mv[4 * q + 3] = m.w;
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) v[i] = coord_of<CPL, LPC>(g, i) < dd ? x[i] : 0.f;
        float s = 0.f;
        if (white) {
            float f[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) f[i] = 0.f;
            matvec(mat, v, f, g);                                   // L z
#pragma unroll
            for (int i = 0; i < CPL; ++i) f[i] += mv[i];
            float lp[CPL];
            s = likelihood_of(f, lp, g);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                cx.gr[i] = v[i];
                s = fmaf(0.5f * v[i], v[i], s);
            }
            matvec(mat + (int64_t)dd * dd, lp, cx.gr, g);           // z + L^T l'(f)
        } else {
            float r[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                r[i] = coord_of<CPL, LPC>(g, i) < dd ? x[i] - mv[i] : 0.f;
                cx.gr[i] = 0.f;
            }
            matvec(mat, r, cx.gr, g);                               // Lambda r
            float lp[CPL];
            s = likelihood_of(v, lp, g);
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                s = fmaf(0.5f * r[i], cx.gr[i], s);
                cx.gr[i] += lp[i];
            }
        }
        cx.u = group_allreduce<LPC>(s);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Latent Gaussian Markov random field (NFMC_POT_LATENT_GMRF, nfmc_hip.h): n sites with the sparse structure matrix R in
// slot-major ELL form (W = p.n_components slots; p.a = W rows of n4 = 4 ceil(n / 4) values, then W rows of n4 column
// indices as integer-valued floats; a padding slot has value 0 and its own row as index), kind 12's likelihoods on the
// sites (latent_lik, table p.b = 8 header floats, then the rows m, y, w of n4 floats) and optionally s = log tau as
// coordinate n.  With v the vector of the mode, q = v^T R v, (a, b, rho/2, (n - rho)/2) = p.b[4 .. 7]:
//   fixed tau  (d = n, v = x - m):      U = 1/2 q + sum l_j(x_j),                               dU/dx = R v + l'(x)
//   centred    (d = n + 1, v = x - m):  U = 1/2 e^s q - (rho/2 + a) s + sum l_j(x_j) + b e^s,   dU/dx_j = e^s (R v)_j + l'_j,
//                                       dU/ds = 1/2 e^s q - rho/2 + b e^s - a
//   scaled     (d = n + 1, v = u, f = m + e^(-s/2) u):
//                                       U = 1/2 q + sum l_j(f_j) + b e^s - a s + (n - rho)/2 s,
//                                       dU/du_j = (R u)_j + e^(-s/2) l'_j(f_j),
//                                       dU/ds = -1/2 e^(-s/2) sum u_j l'_j(f_j) + b e^s - a + (n - rho)/2
// The access pattern is a gather: coordinate j needs v at the W columns of its row, anywhere in the chain.  The
// workgroup's block is IrtPot's: one wave-private row of DP + 4 floats per chain (irt_floats).  prepare() stores the
// lane's quads of v into the row (zeros on the padding; s itself at position n, which every lane then reads back: one
// address per chain, a broadcast), and forms (R v)_j of its own coordinates slot by slot: per register quad and slot ONE
// 16-byte load of values and ONE of indices from global memory (consecutive lanes consecutive 16 bytes, every chain the
// same ones: the block of at most 2 x 32 x 1024 floats stays in L2) and four ds_read_b32 gathers.  ds_bpermute cannot
// serve: it moves one register of one other lane, and the column a lane needs sits in a register whose index depends
// on the column.  Every gathered index is clamped into the sites 0 .. n - 1 (gmrf_row in neutra_kernels.hpp clamps
// alike), so a bad table reads a wrong site of the chain's own row: never s, another chain's row or memory outside
// the block.  Row pitch DP + 4 as in IrtPot: the gathers of one
// chain spread over the banks like the columns of R do; chains of one 32-lane half that gather the same column (the
// same stencil offset) would meet in one bank at a pitch of DP >= 32 and sit 4 banks apart here.  The row is written
// and read by ONE wave: wavefront fences (Phi4Pot), no workgroup barrier.  1/2 v^T R v, the data term and sum u l' are
// lane-local sums; what crosses lanes goes through group_allreduce: U alone when tau is fixed, q and the data term
// when centred, U's site part and sum u l' when scaled.  No atomics: bitwise repeatable.  The likelihood is dispatched
// once per prepare() outside the loops (LatentGaussPot), the mode is a wave-uniform branch behind them.  Nothing is
// clamped: an overflowing e^s or e^f gives a non-finite U, which the samplers reject and count.
template <int CPL, int LPC, bool FAST>
struct GmrfPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    const float* ell;                    // this lane's quad 0 of slot 0: values; the indices wn4 floats behind
    const float* tab;                    // rows m, y, w of n4 floats (behind the 8 floats of the header)
    int nn, n4, nw, wn4;                 // n, 4 ceil(n / 4), W, W n4
    int lik;
    bool tau, scaled;
    bool lead;                           // this lane holds coordinate 0 in register 0
    float c0, c1, c2;                    // Student-t constants
    float pa, pb, hr, hn;                // Gamma(a, b) prior of tau, rho / 2, (n - rho) / 2
    struct Ctx {
        float u;                         // U of the chain (every lane of the group)
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        lik = 0;
        tau = scaled = false;
        gmrf_code(p.a_scalar, lik, tau, scaled);
        nn = tau ? d - 1 : d;
        n4 = latent_row(nn);
        nw = p.n_components;
        wn4 = nw * n4;
        ell = p.a + 4 * g;
        tab = p.b + 8;
        lead = (g == 0);
        c0 = p.b[0];
        c1 = p.b[1];
        c2 = p.b[2];
        pa = p.b[4];
        pb = p.b[5];
        hr = p.b[6];
        hn = p.b[7];
    }
    // register quad q of table row k (0 m, 1 y, 2 w) for this lane; zeros past the row
    __device__ __forceinline__ float4 tab4(int k, int q, int g) const {
        const int c = 4 * (q * LPC + g);
        return c < n4 ? *reinterpret_cast<const float4*>(tab + k * n4 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // value of the chain's row at the column a table entry names, clamped into the sites 0 .. n - 1
    __device__ __forceinline__ float gather(float col) const {
        const int j = (int)col;
        return row[j < 0 ? 0 : (j > nn - 1 ? nn - 1 : j)];
    }
    // l'(f) of this lane's coordinates into lp, their share of sum_j l_j(f_j) returned
    template <int LIK>
    __device__ __forceinline__ float likelihood(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 y = tab4(1, q, g), w = tab4(2, q, g);
            const float yy[4] = {y.x, y.y, y.z, y.w}, ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float l;
                latent_lik<LIK>(f[4 * q + k], yy[k], ww[k], c0, c1, c2, l, lp[4 * q + k]);
                s += l;
            }
        }
        return s;
    }
    __device__ __forceinline__ float likelihood_of(const float (&f)[CPL], float (&lp)[CPL], int g) const {
        return lik == 0 ? likelihood<0>(f, lp, g) : lik == 1 ? likelihood<1>(f, lp, g) : likelihood<2>(f, lp, g);
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        float v[CPL], mv[CPL];           // r or u on the sites, 0 elsewhere / the prior mean
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 m = tab4(0, q, g);
            mv[4 * q] = m.x;
            mv[4 * q + 1] = m.y;
            mv[4 * q + 2] = m.z;
            mv[4 * q + 3] = m.w;
            float st[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = 4 * q + k, c = coord_of<CPL, LPC>(g, i);
                v[i] = c < nn ? (scaled ? x[i] : x[i] - mv[i]) : 0.f;
                st[k] = (tau && c == nn) ? x[i] : v[i];
            }
            *reinterpret_cast<float4*>(row + 4 * (q * LPC + g)) = make_float4(st[0], st[1], st[2], st[3]);
        }
        order();   // the wave's stores precede its reads
        const float s = tau ? row[nn] : 0.f;
        const float es = tau ? fast_exp(s) : 1.f, eh = scaled ? fast_exp(-0.5f * s) : 1.f;
        float rv[CPL];                   // (R v)_j of this lane's coordinates
#pragma unroll
        for (int i = 0; i < CPL; ++i) rv[i] = 0.f;
        const float* slot = ell;
        for (int k = 0; k < nw; ++k, slot += n4) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (4 * (q * LPC + g) < n4) {
                    const float4 a = *reinterpret_cast<const float4*>(slot + 4 * q * LPC);
                    const float4 j = *reinterpret_cast<const float4*>(slot + wn4 + 4 * q * LPC);
                    rv[4 * q] = fmaf(a.x, gather(j.x), rv[4 * q]);
                    rv[4 * q + 1] = fmaf(a.y, gather(j.y), rv[4 * q + 1]);
                    rv[4 * q + 2] = fmaf(a.z, gather(j.z), rv[4 * q + 2]);
                    rv[4 * q + 3] = fmaf(a.w, gather(j.w), rv[4 * q + 3]);
                }
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        float f[CPL], lp[CPL];
#pragma unroll
        for (int i = 0; i < CPL; ++i) f[i] = scaled ? fmaf(eh, v[i], mv[i]) : x[i];
        const float ls = likelihood_of(f, lp, g);
        float qf = 0.f;                  // this lane's share of v^T R v
#pragma unroll
        for (int i = 0; i < CPL; ++i) qf = fmaf(v[i], rv[i], qf);
        Ctx cx;
        float gs = 0.f;                  // dU/ds
        if (!tau) {
            cx.u = group_allreduce<LPC>(fmaf(0.5f, qf, ls));
#pragma unroll
            for (int i = 0; i < CPL; ++i) cx.gr[i] = rv[i] + lp[i];
        } else if (!scaled) {
            const float qq = group_allreduce<LPC>(qf), lt = group_allreduce<LPC>(ls);
            const float hq = 0.5f * es * qq, be = pb * es;
            cx.u = (hq + lt) + (be - (hr + pa) * s);
            gs = (hq - hr) + (be - pa);
#pragma unroll
            for (int i = 0; i < CPL; ++i) cx.gr[i] = fmaf(es, rv[i], lp[i]);
        } else {
            float ul = 0.f;              // this lane's share of sum u l'
#pragma unroll
            for (int i = 0; i < CPL; ++i) ul = fmaf(v[i], lp[i], ul);
            const float us = group_allreduce<LPC>(fmaf(0.5f, qf, ls)), ut = group_allreduce<LPC>(ul);
            const float be = pb * es;
            cx.u = us + (be + (hn - pa) * s);
            gs = fmaf(-0.5f * eh, ut, be) + (hn - pa);
#pragma unroll
            for (int i = 0; i < CPL; ++i) cx.gr[i] = fmaf(eh, lp[i], rv[i]);
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            cx.gr[i] = c < nn ? cx.gr[i] : ((tau && c == nn) ? gs : 0.f);
        }
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return (lead && i == 0) ? cx.u : 0.f; }
};

// Drifts of the diffusion bridge (NFMC_POT_DIFFUSION_BRIDGE), DR the drift code, M the state's dimension, (p0 .. p3) the
// drift parameters of the header: f(x) into f, and J_f(x)^T e into v.  Fixed operation order: DiffusionPot and
// diffusion_row (neutra_kernels.hpp) share them.
//   0 cubic (any M)       f_c = x_c (p0 - p1 x_c^2),                              J = diag(p0 - 3 p1 x_c^2)
//   1 fitzhugh_nagumo (2) f = (x0 - x0^3/3 - x1 + p3, p2 (x0 + p0 - p1 x1)),      J = [[1 - x0^2, -1], [p2, -p2 p1]]
//   2 lorenz63 (3)        f = (p0 (x1 - x0), x0 (p1 - x2) - x1, x0 x1 - p2 x2),   J = [[-p0, p0, 0], [p1 - x2, -1, -x0], [x1, x0, -p2]]
template <int DR, int M>
__device__ __forceinline__ void diffusion_drift(const float (&x)[M], float p0, float p1, float p2, float p3, float (&f)[M]) {
    if constexpr (DR == 0) {
#pragma unroll
        for (int c = 0; c < M; ++c) f[c] = x[c] * fmaf(-p1 * x[c], x[c], p0);
    } else if constexpr (DR == 1) {
        f[0] = (fmaf(-(1.f / 3.f) * x[0] * x[0], x[0], x[0]) - x[1]) + p3;
        f[1] = p2 * fmaf(-p1, x[1], x[0] + p0);
    } else {
        f[0] = p0 * (x[1] - x[0]);
        f[1] = fmaf(x[0], p1 - x[2], -x[1]);
        f[2] = fmaf(x[0], x[1], -p2 * x[2]);
    }
}
template <int DR, int M>
__device__ __forceinline__ void diffusion_jte(const float (&x)[M], const float (&e)[M], float p0, float p1, float p2, float,
                                              float (&v)[M]) {
    if constexpr (DR == 0) {
#pragma unroll
        for (int c = 0; c < M; ++c) v[c] = fmaf(-3.f * p1 * x[c], x[c], p0) * e[c];
    } else if constexpr (DR == 1) {
        v[0] = fmaf(fmaf(-x[0], x[0], 1.f), e[0], p2 * e[1]);
        v[1] = fmaf(-p2 * p1, e[1], -e[0]);
    } else {
        v[0] = fmaf(x[1], e[2], fmaf(p1 - x[2], e[1], -p0 * e[0]));
        v[1] = fmaf(x[0], e[2], fmaf(p0, e[0], -e[1]));
        v[2] = fmaf(-x[0], e[1], -p2 * e[2]);
    }
}
// Diffusion bridge (NFMC_POT_DIFFUSION_BRIDGE, nfmc_hip.h): the latent path X_0 .. X_{T-1} in R^m of a discretised
// stochastic differential equation, time-major (coordinate t m + c is X_{t,c}), then p = log sigma and q = log tau when
// the scales are unknown.  T = p.n_components, the header p.a (kDif*), the rows y and w of n4 = 4 ceil(T m / 4) floats
// in p.b.  With e_t = X_t - X_{t-1} - dt f(X_{t-1}), om = 1 / (sigma^2 dt), rho = 1 / tau^2, S_e = sum_{t>=1} |e_t|^2,
// S_v = sum_{observed} (X - y)^2:
//   U       = 1/2 |X_0 - mu0|^2 / s0^2 + 1/2 om S_e + 1/2 rho S_v
//             [ + (T-1) m p + N_o q + ((p - l)^2 + (q - l)^2) / (2 c^2) ]
//   dU/dX_t = [t = 0] (X_0 - mu0) / s0^2 + [t >= 1] om e_t - [t < T-1] om (I + dt J_f(X_t))^T e_{t+1} + rho w_t (X_t - y_t)
//   dU/dp   = -om S_e + (T-1) m + (p - l) / c^2,    dU/dq = -rho S_v + N_o + (q - l) / c^2
// A coordinate needs the whole vectors X_{t-1}, X_t and X_{t+1}: up to nine values that with m = 3 straddle register quads
// and lanes at no fixed offset, so ds_bpermute (one register of one other lane, the register chosen at compile time)
// would take a fetch of every candidate register with selects behind it.  The exchange is IrtPot's and GmrfPot's instead:
// one wave-private LDS row of DP + 4 floats per chain (irt_floats), written once per evaluation, one 16-byte store per
// register quad; every lane then reads, per register quad, the window of steps the quad's four coordinates and their
// neighbours lie in (6, 8 or 12 values for m = 1, 2, 3: the steps tl - 1 .. tl + 4 or tl - 1 .. tl + 2) with ds_read_b32,
// evaluates the drift once per step of the window, and picks each coordinate's e_{t,c} and successor term from the
// step-major lists by its offset r in step tl (selects; r = 0 unless m = 3); p and q are read at positions T m and
// T m + 1 (one address per chain: a broadcast).  Every index is formed from a step clamped into 0 .. T-1, so it lies
// in the path's part of the chain's own row whatever the masks say.  The row is written and read by ONE
// wave: wavefront fences, no workgroup barrier.  (drift, m) is dispatched ONCE per prepare() to a body with compile-time
// bounds (ParticlePot's rule): no register array is indexed by a run-time value, the own component is taken by selects
// (never a run-time register index).  A lane recomputes the drift of the steps around its quads in the fixed order of
// diffusion_drift; e_{t,c}^2 enters S_e exactly once, at the coordinate (t, c) that owns it.  y and the roles "on the
// path" / "t >= 1" / "t < T-1" / "observed" (w != 0) are registers and bit masks set once in init() (SVPot); a padding
// coordinate has no role, adds exactly zero to U and both sums and gets a zero gradient.  S_e and S_v cross lanes through
// one group_allreduce each: fixed order, no atomics, bitwise repeatable.  Nothing is clamped: an overflowing e^{-2p} or
// cubic term gives a non-finite U, which the samplers reject and count.  term() puts the lane's share of U (its part of
// the X_0 term; the rest on the lane of coordinate 0) on its register 0.
template <int CPL, int LPC, bool FAST>
struct DiffusionPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    int nt, tm, drift, mm;               // T, T m, drift code, m
    bool unk, lead;                      // scales unknown / this lane holds coordinate 0 in register 0
    float dt, om0, rho0, mu0, is0, loc, ic2, nobs, tm1m, p0, p1, p2, p3;
    float y[CPL];                        // y of the lane's path coordinates (0 elsewhere)
    uint32_t in, pd, sc, ob;             // bit i: register i is on the path / has t >= 1 / has t < T-1 / is observed
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        drift = 0;
        mm = 1;
        unk = false;
        diffusion_code(p.a_scalar, drift, unk, mm);
        nt = p.n_components;
        tm = nt * mm;
        lead = (g == 0);
        const float* h = p.a;
        dt = h[kDifDt];
        om0 = 1.f / (h[kDifSigma] * h[kDifSigma] * dt);
        rho0 = 1.f / (h[kDifTau] * h[kDifTau]);
        mu0 = h[kDifMu0];
        is0 = h[kDifIs0];
        loc = h[kDifLoc];
        ic2 = h[kDifIc2];
        nobs = h[kDifNobs];
        tm1m = h[kDifTm1m];
        p0 = h[kDifPar0];
        p1 = h[kDifPar0 + 1];
        p2 = h[kDifPar0 + 2];
        p3 = h[kDifPar0 + 3];
        const int n4 = latent_row(tm);
        in = pd = sc = ob = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            y[i] = 0.f;
            if (c < tm) {
                y[i] = p.b[c];
                in |= 1u << i;
                if (c >= mm) pd |= 1u << i;
                if (c + mm < tm) sc |= 1u << i;
                if (p.b[n4 + c] != 0.f) ob |= 1u << i;
            }
        }
    }
    template <int DR, int M>
    __device__ __forceinline__ Ctx body(const float (&x)[CPL], int g) const {
        constexpr int NS = M == 1 ? 4 : 2;   // time steps a register quad touches: 4 (m = 1), 2 (m = 2), 2 (m = 3)
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int k = 0; k < Q; ++k)
            *reinterpret_cast<float4*>(row + 4 * (k * LPC + g)) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        order();   // the wave's stores precede its reads
        const float ps = unk ? row[tm] : 0.f, qs = unk ? row[tm + 1] : 0.f;
        const float om = unk ? fast_exp(-2.f * ps) / dt : om0, rho = unk ? fast_exp(-2.f * qs) : rho0;
        Ctx cx;
        float se = 0.f, sv = 0.f, u0 = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            // the quad's coordinates c0 .. c0 + 3 lie in the steps tl and tl + 1 (.. tl + 3 for m = 1), the first at
            // component r of step tl (r = 0 unless m = 3); a quad past the path reads about step T - 1, unused
            const int c0 = min(4 * (q * LPC + g), tm - 1);
            const int tl = c0 / M, r = c0 - tl * M;
            float w[NS + 2][M], e[NS + 1][M];   // X of the steps tl - 1 .. tl + NS (clamped into the path); e of tl .. tl + NS
#pragma unroll
            for (int s = 0; s < NS + 2; ++s) {
                const int b = min(max(tl - 1 + s, 0), nt - 1) * M;
#pragma unroll
                for (int k = 0; k < M; ++k) w[s][k] = row[b + k];
            }
#pragma unroll
            for (int s = 0; s < NS + 1; ++s) {
                float f[M];
                diffusion_drift<DR, M>(w[s], p0, p1, p2, p3, f);
#pragma unroll
                for (int k = 0; k < M; ++k) e[s][k] = fmaf(-dt, f[k], w[s + 1][k] - w[s][k]);
            }
            float ge[NS * M], gs[NS * M];       // step-major: e_{t,c} and ((I + dt J_f(X_t))^T e_{t+1})_c of the steps tl ..
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float jt[M];
                diffusion_jte<DR, M>(w[s + 1], e[s + 1], p0, p1, p2, p3, jt);
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    ge[s * M + k] = e[s][k];
                    gs[s * M + k] = fmaf(dt, jt[k], e[s + 1][k]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * q + j;
                float ej, sn;                   // entry r + j of the two lists, by selects
                if constexpr (M == 3) {
                    ej = r == 0 ? ge[j] : (r == 1 ? ge[j + 1] : ge[j + 2]);
                    sn = r == 0 ? gs[j] : (r == 1 ? gs[j + 1] : gs[j + 2]);
                } else {
                    ej = ge[j];
                    sn = gs[j];
                }
                const bool on = (in >> i) & 1u, hp = (pd >> i) & 1u, hs = (sc >> i) & 1u, ho = (ob >> i) & 1u;
                const float d0 = x[i] - mu0, rr = x[i] - y[i];
                float gr = (on && !hp) ? is0 * d0 : 0.f;
                u0 += (on && !hp) ? 0.5f * is0 * d0 * d0 : 0.f;
                gr = hp ? om * ej : gr;
                se += hp ? ej * ej : 0.f;
                gr = hs ? fmaf(-om, sn, gr) : gr;
                gr = ho ? fmaf(rho, rr, gr) : gr;
                sv += ho ? rr * rr : 0.f;
                cx.gr[i] = gr;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        se = group_allreduce<LPC>(se);
        sv = group_allreduce<LPC>(sv);
        float ug = 0.5f * (om * se + rho * sv);
        if (unk) {
            const float dp = ps - loc, dq = qs - loc;
            ug += fmaf(tm1m, ps, nobs * qs) + 0.5f * ic2 * fmaf(dp, dp, dq * dq);
            const float gp = fmaf(-om, se, tm1m) + dp * ic2, gq = fmaf(-rho, sv, nobs) + dq * ic2;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = coord_of<CPL, LPC>(g, i);
                cx.gr[i] = c == tm ? gp : (c == tm + 1 ? gq : cx.gr[i]);
            }
        }
        cx.u = u0 + (lead ? ug : 0.f);
        return cx;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        if (drift == 2) return body<2, 3>(x, g);
        if (drift == 1) return body<1, 2>(x, g);
        return mm == 3 ? body<0, 3>(x, g) : (mm == 2 ? body<0, 2>(x, g) : body<0, 1>(x, g));
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Blocked Rosenbrock (NFMC_POT_ROSENBROCK; block B = p.n_components, a = a_scalar, b = b_scalar, mu = p.a[0]):
//   U = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2,   c a head when c % B == 0
//   dU/dx_c = [head] 2a (x_c - mu) + [non-head] 2b (x_c - x_{c-1}^2) - [c+1 < d non-head] 4b x_c (x_{c+1} - x_c^2)
// Every coordinate couples to its neighbours c - 1 and c + 1 in the flattened order, and nothing else: no reduction and
// no LDS table.  Inside a register quad the neighbours are the lane's own registers.  Across the quad's ends, with
// quad q of lane g holding 4 (q LPC + g) .. + 3 (coord_of):
//   predecessor of its first coordinate = register 4q + 3 of lane g - 1, for g = 0 register 4(q - 1) + 3 of lane LPC - 1
//   successor of its last coordinate    = register 4q of lane g + 1, for g = LPC - 1 register 4(q + 1) of lane 0
// so prepare() fetches register 4q + 3 from lane (g - 1) mod LPC and register 4q from lane (g + 1) mod LPC for every
// quad (two ds_bpermute per quad; nothing with one lane per chain), and lane 0 / lane LPC - 1 take the neighbouring
// quad's fetch.  The head / non-head / successor roles of the lane's coordinates are bit masks set once in init();
// padding coordinates (c >= d) have none, so they add exactly zero to U and get a zero gradient, and a coordinate
// has a successor term only when c + 1 < d is a non-head.  term() puts the lane's share of U on its register 0.
template <int CPL, int LPC, bool FAST>
struct RosenbrockPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    static constexpr int Q = CPL / 4;   // register quads
    float ca, cb, mu;
    uint32_t hd, nh, sc;   // bit i: register i is a head / a non-head / has a successor term
    int prv, nxt;          // ds_bpermute byte addresses of lanes (g - 1) mod LPC and (g + 1) mod LPC of the group
    bool first, last;      // g == 0 / g == LPC - 1
    struct Ctx {
        float u;           // this lane's share of U
        float gr[CPL];     // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        ca = p.a_scalar;
        cb = p.b_scalar;
        mu = p.a[0];
        const int blk = p.n_components;
        hd = nh = sc = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            if (c < d) {
                if (c % blk == 0) hd |= 1u << i;
                else nh |= 1u << i;
                if (c + 1 < d && (c + 1) % blk != 0) sc |= 1u << i;
            }
        }
        const int base = (int)(threadIdx.x & 63) - g;
        prv = 4 * (base + (g + LPC - 1) % LPC);
        nxt = 4 * (base + (g + 1) % LPC);
        first = g == 0;
        last = g == LPC - 1;
    }
    __device__ __forceinline__ static float fetch(float v, int addr) {
        if constexpr (LPC == 1) return v;
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        float pv[Q], nv[Q];   // register 4q + 3 of lane g - 1 / register 4q of lane g + 1 (cyclic in the group)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            pv[q] = fetch(x[4 * q + 3], prv);
            nv[q] = fetch(x[4 * q], nxt);
        }
        Ctx cx;
        float u = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int q = i >> 2, k = i & 3;
            float xm, xn;   // x_{c-1}, x_{c+1} (any finite value where the mask bits leave them unused)
            if (k > 0) xm = x[i - 1];
            else if (q > 0) xm = first ? pv[q - 1] : pv[q];
            else xm = first ? 0.f : pv[0];
            if (k < 3) xn = x[i + 1];
            else if (q + 1 < Q) xn = last ? nv[q + 1] : nv[q];
            else xn = last ? 0.f : nv[q];
            float t = 0.f, gr = 0.f;
            if ((hd >> i) & 1u) {
                const float r = x[i] - mu;
                t = ca * (r * r);
                gr = 2.f * ca * r;
            } else if ((nh >> i) & 1u) {
                const float r = fmaf(-xm, xm, x[i]);
                t = cb * (r * r);
                gr = 2.f * cb * r;
            }
            if ((sc >> i) & 1u) gr = fmaf(-4.f * cb * x[i], fmaf(-x[i], x[i], xn), gr);
            u += t;
            cx.gr[i] = gr;
        }
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Stochastic volatility (NFMC_POT_STOCHASTIC_VOLATILITY; T = p.n_components = d - 3, y = p.a[0 .. T-1], (alpha, beta) =
// p.b[0 .. 1], c_mu = a_scalar, c_sigma = b_scalar).  Coordinates x_0 = mu, x_1 = s = log sigma, x_2 = r = atanh phi,
// x_{3+t} = h_t; with w = e^{-2s}, phi = tanh r, q = 1 - phi^2, delta_0 = h_0 - mu, a_t = h_{t-1} - mu, e_t = h_t - mu -
// phi a_t (t >= 1) and S1 = sum e_t, S2 = sum e_t^2, S3 = sum e_t a_t:
//   U = log1p((mu/c_mu)^2) + softplus(2(s - log c_sigma)) + (alpha + 1/2) softplus(-2r) + (beta + 1/2) softplus(2r)
//     + 1/2 q w delta_0^2 + (T - 1) s + sum_{t>=1} 1/2 w e_t^2 + sum_{t>=0} 1/2 [h_t + y_t^2 e^{-h_t}]
//   dU/dmu  = 2 mu/(c_mu^2 + mu^2) - q w delta_0 - (1 - phi) w S1
//   dU/ds   = 2 sigmoid(2(s - log c_sigma)) - q w delta_0^2 - w S2 + (T - 1)
//   dU/dr   = 2(beta + 1/2) sigmoid(2r) - 2(alpha + 1/2) sigmoid(-2r) - phi q w delta_0^2 - q w S3
//   dU/dh_t = 1/2 - 1/2 y_t^2 e^{-h_t} + [t = 0] q w delta_0 + [t >= 1] w e_t - [t + 1 < T] phi w e_{t+1}
// (the -s of sigma's Jacobian and the +s of h_0's normaliser cancel).  mu, s, r and h_0 are coordinates 0 .. 3, register
// quad 0 of lane 0 at every layout (coord_of).  prepare() broadcasts registers 0 .. 2 of lane 0 to the chain's lanes
// (FunnelPot), fetches the neighbours h_{t-1} and h_{t+1} across register quads and lanes with RosenbrockPot's two
// ds_bpermute per quad, forms every h_t's terms lane-locally, and all-reduces S1, S2 and S3 (one butterfly each); lane 0
// then writes the global gradients into its registers 0 .. 2 and adds delta_0's term to h_0's.  y_t^2 of the lane's h
// coordinates sit in registers (QuadraticPot's b[]); the "is an h" / "has a predecessor term" (t >= 1) / "has a successor
// term" (t + 1 < T) roles are bit masks set once in init().  Padding coordinates have none, so they add exactly zero to U
// and the sums and get a zero gradient.  q = 4 sigmoid(2r) sigmoid(-2r) and 1 - phi = 2 sigmoid(-2r) stay finite and
// accurate at any r; w and e^{-h_t} overflow fp32 for s < -44 or h_t < -88, and such a state's U is inf or NaN, so the
// samplers reject it and count its log ratio as non-finite.  term() puts the lane's share of U on its register 0.
template <int CPL, int LPC, bool FAST>
struct SVPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    static constexpr int Q = CPL / 4;   // register quads
    float cmu, lcs, ca, cb, tm1;        // c_mu, log c_sigma, alpha + 1/2, beta + 1/2, T - 1
    float y2[CPL];                      // y_t^2 of the lane's h coordinates (0 elsewhere)
    uint32_t hm, pd, sc;                // bit i: register i is an h_t / has t >= 1 / has t + 1 < T
    int prv, nxt;                       // ds_bpermute byte addresses of lanes (g - 1) mod LPC and (g + 1) mod LPC
    bool first, last;                   // g == 0 (holds mu, s, r, h_0) / g == LPC - 1
    struct Ctx {
        float u;                        // this lane's share of U
        float gr[CPL];                  // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d) {
        cmu = p.a_scalar;
        lcs = logf(p.b_scalar);
        ca = p.b[0] + 0.5f;
        cb = p.b[1] + 0.5f;
        tm1 = (float)(p.n_components - 1);
        hm = pd = sc = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            y2[i] = 0.f;
            if (c >= 3 && c < d) {
                const float yv = p.a[c - 3];
                y2[i] = yv * yv;
                hm |= 1u << i;
                if (c >= 4) pd |= 1u << i;
                if (c + 1 < d) sc |= 1u << i;
            }
        }
        const int base = (int)(threadIdx.x & 63) - g;
        prv = 4 * (base + (g + LPC - 1) % LPC);
        nxt = 4 * (base + (g + 1) % LPC);
        first = g == 0;
        last = g == LPC - 1;
    }
    __device__ __forceinline__ static float fetch(float v, int addr) {
        if constexpr (LPC == 1) return v;
        else return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        const float mu = group_broadcast0<LPC>(x[0]), s = group_broadcast0<LPC>(x[1]), r = group_broadcast0<LPC>(x[2]);
        float pv[Q], nv[Q];   // register 4q + 3 of lane g - 1 / register 4q of lane g + 1 (cyclic in the group)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            pv[q] = fetch(x[4 * q + 3], prv);
            nv[q] = fetch(x[4 * q], nxt);
        }
        float spp, sgp, spm, sgm;   // softplus / sigmoid of 2r and of -2r
        softplus_sigmoid(2.f * r, spp, sgp);
        softplus_sigmoid(-2.f * r, spm, sgm);
        const float phi = sgp - sgm, w = fast_exp(-2.f * s), pw = phi * w;
        Ctx cx;
        float u = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int q = i >> 2, k = i & 3;
            float xm, xn;   // h_{t-1}, h_{t+1} (any finite value where the mask bits leave them unused)
            if (k > 0) xm = x[i - 1];
            else if (q > 0) xm = first ? pv[q - 1] : pv[q];
            else xm = first ? 0.f : pv[0];
            if (k < 3) xn = x[i + 1];
            else if (q + 1 < Q) xn = last ? nv[q + 1] : nv[q];
            else xn = last ? 0.f : nv[q];
            float t = 0.f, gr = 0.f;
            if ((hm >> i) & 1u) {
                const float ye = y2[i] * fast_exp(-x[i]), dh = x[i] - mu;
                t = 0.5f * (x[i] + ye);
                gr = fmaf(-0.5f, ye, 0.5f);
                if ((pd >> i) & 1u) {
                    const float a = xm - mu, e = fmaf(-phi, a, dh);
                    t = fmaf(0.5f * w * e, e, t);
                    gr = fmaf(w, e, gr);
                    s1 += e;
                    s2 = fmaf(e, e, s2);
                    s3 = fmaf(e, a, s3);
                }
                if ((sc >> i) & 1u) gr = fmaf(-pw, fmaf(-phi, dh, xn - mu), gr);   // - phi w e_{t+1}
            }
            u += t;
            cx.gr[i] = gr;
        }
        s1 = group_allreduce<LPC>(s1);
        s2 = group_allreduce<LPC>(s2);
        s3 = group_allreduce<LPC>(s3);
        if (first) {
            const float d0 = x[3] - mu, qw = 4.f * sgp * sgm * w, qwd = qw * d0, m = mu / cmu;
            float sps, sgs;   // softplus / sigmoid of 2(s - log c_sigma)
            softplus_sigmoid(2.f * (s - lcs), sps, sgs);
            cx.gr[0] = 2.f * m / (cmu * fmaf(m, m, 1.f)) - qwd - 2.f * sgm * w * s1;
            cx.gr[1] = 2.f * sgs - qwd * d0 - w * s2 + tm1;
            cx.gr[2] = 2.f * cb * sgp - 2.f * ca * sgm - phi * qwd * d0 - qw * s3;
            cx.gr[3] += qwd;
            u += log1pf(m * m) + sps + tm1 * s + ca * spm + cb * spp + 0.5f * qwd * d0;
        }
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Sparse logistic regression (NFMC_POT_SPARSE_LOGISTIC_REGRESSION; X (N, D) row-major in a, y (N,) in {0, 1} in b,
// N = p.n_components, a = a_scalar, b = b_scalar, D = (d - 1) / 2).  Coordinates x_{2j} = w_j, x_{2j+1} = l_j =
// log lambda_j, x_{2D} = s = log tau; with beta_j = e^{s + l_j} w_j, z = X beta, r_i = sigmoid(z_i) - y_i, g = X^T r:
//   U = sum_i [softplus(z_i) - y_i z_i] + 1/2 sum_j w_j^2 + sum_j (b e^{l_j} - a l_j) + (b e^s - a s)
//   dU/dw_j = e^{s + l_j} g_j + w_j,   dU/dl_j = beta_j g_j + b e^{l_j} - a,   dU/ds = sum_j beta_j g_j + b e^s - a
// Register quad q of lane g holds coordinates 4 (q LPC + g) .. + 3 (coord_of), i.e. the pairs (w_j, l_j) of the two
// columns j = 2 (q LPC + g) and j + 1: every pair is lane-local, and only s crosses lanes.  prepare() (1) broadcasts s
// from the lane that holds coordinate 2D with one group_allreduce of a masked value, (2) forms beta of the lane's columns
// in registers, (3) streams X through a COMPACT LDS tile -- slr_tile_rows(DP) rows of DP / 2 columns, zero past D and past
// the last row, their labels behind them -- in LogRegPot's batches of 4 rows: per row and register quad one ds_read_b64
// of the quad's two columns feeds two FMAs of the dot product and, after the batch's reduce-scatter (LPC >= 4; one
// butterfly per row below) and the residual broadcast, two FMAs of g; (4) applies the chain rule pair by pair, and (5)
// all-reduces sum_j beta_j g_j (one butterfly) for the gradient of s.  The data term is summed in fp64 per lane as in
// LogRegPot, and term() puts the lane's share of U on its register 0.  LogRegPot's tile rule holds: every thread of the
// workgroup calls prepare() equally often.  e^{s + l_j}, e^{l_j}, e^s or z overflow fp32 far in the tails; such a
// state's U is inf or NaN, so the samplers reject it and count its log ratio as non-finite.
template <int CPL, int LPC, bool FAST>
struct SparseLogRegPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int DH = DP / 2;                  // tile columns: two per register quad
    static constexpr int T = kLogRegTileFloats / DH;   // rows per tile (slr_tile_rows)
    static constexpr int NP = CPL / 2;                 // column pairs (w_j, l_j) per lane
    static_assert(T % 4 == 0, "batches of 4 rows");
    float* tile;          // LDS: X rows (T, DH) | y (T)
    const float* X;
    const float* y;
    int nr, nd;           // N, D
    float ca, cb;         // a, b
    int sreg;             // the register of this lane that holds s (coordinate 2D), -1 if none
    uint32_t pm;          // bit p: pair p (registers 2p, 2p + 1) is a column j < D
    struct Ctx {
        float u;          // this lane's share of U
        float gr[CPL];    // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // prepare() streams the tiles
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        tile = lds;
        X = p.a;
        y = p.b;
        nr = p.n_components;
        nd = (d - 1) >> 1;
        ca = p.a_scalar;
        cb = p.b_scalar;
        sreg = -1;
        pm = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            if (c == d - 1) sreg = i;
            if ((i & 1) == 0 && c < d - 1) pm |= 1u << (i >> 1);
        }
    }
    // columns 2 (q LPC + g) and + 1 of tile row r
    __device__ __forceinline__ float2 row2(int r, int q, int g) const {
        return *reinterpret_cast<const float2*>(tile + r * DH + 2 * (q * LPC + g));
    }
    // all threads of the workgroup: rows t0 .. t0 + rows - 1 into the tile, zeros past them
    __device__ __forceinline__ void load_tile(int t0, int rows) const {
        load_tile_rows<DH>(tile, X, nd, t0, rows);
        for (int r = threadIdx.x; r < T; r += kBlock) tile[T * DH + r] = r < rows ? y[t0 + r] : 0.f;
        __syncthreads();
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        float sv = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) sv = i == sreg ? x[i] : sv;
        const float s = group_allreduce<LPC>(sv);   // s = log tau: the one value that crosses lanes
        float es[NP], bt[NP], gg[NP];                // e^{s + l_j}, beta_j, g_j of the lane's columns (0 past D)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const bool ok = (pm >> p) & 1u;
            es[p] = ok ? fast_exp(s + x[2 * p + 1]) : 0.f;
            bt[p] = ok ? es[p] * x[2 * p] : 0.f;
            gg[p] = 0.f;
        }
        double ul = 0.0;   // this lane's share of the data term, in fp64 (LogRegPot)
        const float* yt = tile + T * DH;
        for (int t0 = 0; t0 < nr; t0 += T) {
            const int rows = nr - t0 < T ? nr - t0 : T;
            load_tile(t0, rows);
            for (int r0 = 0; r0 < rows; r0 += 4) {
                float h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float sz = 0.f;
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float2 v = row2(r0 + b, q, g);
                        sz = fmaf(v.x, bt[2 * q], sz);
                        sz = fmaf(v.y, bt[2 * q + 1], sz);
                    }
                    h[b] = sz;
                }
                float rb[4];   // sigmoid(z) - y of the batch's rows (0 past the last row)
                if constexpr (LPC >= 4) {
                    const int b = g & 3;
                    const float z = group_reduce_scatter<4, LPC>(h);   // z of row r0 + b
                    const float yv = yt[r0 + b];
                    float sp, sg;
                    softplus_sigmoid(z, sp, sg);
                    const bool ok = r0 + b < rows;
                    if (ok && g < 4) ul += (double)(sp - yv * z);   // one lane per row
                    const float res = ok ? sg - yv : 0.f;
                    rb[0] = dpp_mov<0x00>(res);   // quad_perm [b, b, b, b]: the value of lane b of the quad
                    rb[1] = dpp_mov<0x55>(res);
                    rb[2] = dpp_mov<0xAA>(res);
                    rb[3] = dpp_mov<0xFF>(res);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float z = group_allreduce<LPC>(h[b]);
                        const float yv = yt[r0 + b];
                        float sp, sg;
                        softplus_sigmoid(z, sp, sg);
                        const bool ok = r0 + b < rows;
                        if (ok && g == 0) ul += (double)(sp - yv * z);
                        rb[b] = ok ? sg - yv : 0.f;
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int q = 0; q < CPL / 4; ++q) {
                        const float2 v = row2(r0 + b, q, g);
                        gg[2 * q] = fmaf(rb[b], v.x, gg[2 * q]);
                        gg[2 * q + 1] = fmaf(rb[b], v.y, gg[2 * q + 1]);
                    }
                }
            }
        }
        Ctx cx;
        float u = 0.f, sbg = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float w = x[2 * p], l = x[2 * p + 1];
            cx.gr[2 * p] = 0.f;
            cx.gr[2 * p + 1] = 0.f;
            if ((pm >> p) & 1u) {
                const float el = fast_exp(l), bg = bt[p] * gg[p];
                cx.gr[2 * p] = fmaf(es[p], gg[p], w);
                cx.gr[2 * p + 1] = bg + fmaf(cb, el, -ca);
                sbg += bg;
                u += fmaf(0.5f * w, w, fmaf(cb, el, -ca * l));
            }
        }
        sbg = group_allreduce<LPC>(sbg);   // sum_j beta_j g_j
        if (sreg >= 0) {
            const float e = fast_exp(s);
#pragma unroll
            for (int i = 0; i < CPL; ++i)
                if (i == sreg) cx.gr[i] = sbg + fmaf(cb, e, -ca);
            u += fmaf(cb, e, -ca * s);
        }
        cx.u = (float)(ul + (double)u);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// phi^4 scalar field on a lattice (NFMC_POT_LATTICE_PHI4; rows of W = p.n_components sites, H = d / W of them, row-major;
// (m2, lam, kappa, boundary) = p.a[0 .. 3], boundary 0 periodic / 1 zero field outside).  With L_c = sum over the
// neighbours c' of c of (x_c - x_c') -- two per axis; a periodic axis wraps, a zero-boundary axis reads 0 past its ends:
//   dU/dx_c = m2 x_c + lam x_c^3 + kappa L_c
//   U = sum_c x_c [1/2 m2 x_c + 1/4 lam x_c^3 + 1/2 kappa L_c]
// (sum_c x_c L_c counts (x_c' - x_c)^2 once per bond, a boundary bond of the zero boundary included: each bond's
// a^2 + b^2 - 2ab is a (a - b) at one end plus b (b - a) at the other).  H = 1 is the 1-D lattice: no second axis.
// W % 4 == 0 (check_phi4), so every lattice row starts on a register quad and d % 4 == 0: inside a quad the left and
// right neighbours are the lane's own registers, the upper and lower neighbours of a quad are ONE aligned quad W floats
// before / behind it in the chain's row, and only register 0's left and register 3's right neighbour lie in other quads.
// In the interleaved layout those quads sit in other lanes at a register index that depends on the lane, so the lanes
// exchange through LDS, not through ds_bpermute (one permute per source register and a select chain per target quad):
// the workgroup's block is one zeroed quad and one row of DP floats per chain (phi4_floats); prepare() stores the
// lane's quads into its chain's row (ds_write_b128) and reads, per quad, the upper and the lower quad (ds_read_b128) and
// the two single neighbours (ds_read_b32): 5 Q LDS operations per evaluation.  The four addresses of a quad are set once
// in init().  A periodic wrap is another address in the row; a neighbour the zero boundary leaves out is the zeroed
// quad; with H = 1 "up" and "down" are the quad itself, whose differences are exactly zero; a padding quad (c >= d)
// reads the zeroed quad and has no bit in `ok`, so its term and gradient are exactly zero.  No branch on the boundary
// in prepare().  A chain's row is written and read by the lanes of ONE wave, whose LDS operations complete in order, so
// no workgroup barrier is needed (and none is possible: the waves do not call prepare() in step); wavefront-scope fences
// and wave barriers keep the compiler from moving the reads over the stores of this or the next evaluation.  term() puts
// the lane's share of U on its register 0.
template <int CPL, int LPC, bool FAST>
struct Phi4Pot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;   // register quads
    float* blk;                          // LDS: zero quad | rows (kBlock / LPC, DP)
    float m2, lam, kap;
    int own;                             // float index of this lane's quad 0 in its chain's row (quad q: + 4 q LPC)
    int up[Q], dn[Q], lf[Q], rt[Q];      // float indices of the quad above / below and of the single neighbours
    uint32_t ok;                         // bit q: quad q holds lattice sites (c < d)
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // all threads of the workgroup; the caller synchronises before the first prepare()
    __device__ __forceinline__ static void stage(float* __restrict__ lds, const NfmcPotential&, int) {
        if (threadIdx.x < 4) lds[threadIdx.x] = 0.f;
    }
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        blk = lds;
        m2 = p.a[0];
        lam = p.a[1];
        kap = p.a[2];
        const bool zero = p.a[3] != 0.f;
        const int W = p.n_components, H = d / W;
        const int row = 4 + (int)(threadIdx.x / LPC) * DP;   // this chain's row, behind the zero quad
        own = row + 4 * g;
        ok = 0u;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c0 = 4 * (q * LPC + g);   // the quad's first site (coord_of)
            up[q] = dn[q] = lf[q] = rt[q] = 0;  // the zero quad
            if (c0 < d) {
                ok |= 1u << q;
                const int r = c0 / W, k = c0 - r * W, at = row + c0;
                if (k > 0) lf[q] = at - 1;
                else if (!zero) lf[q] = at + W - 1;
                if (k + 4 < W) rt[q] = at + 4;
                else if (!zero) rt[q] = at + 4 - W;
                if (H == 1) {
                    up[q] = dn[q] = at;
                } else {
                    if (r > 0) up[q] = at - W;
                    else if (!zero) up[q] = at + (H - 1) * W;
                    if (r + 1 < H) dn[q] = at + W;
                    else if (!zero) dn[q] = at - (H - 1) * W;
                }
            }
        }
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int, int) const {
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int q = 0; q < Q; ++q)
            *reinterpret_cast<float4*>(blk + own + 4 * q * LPC) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
        order();   // the wave's stores precede its reads
        Ctx cx;
        float u = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(blk + up[q]), b = *reinterpret_cast<const float4*>(blk + dn[q]);
            const float va[4] = {a.x, a.y, a.z, a.w}, vb[4] = {b.x, b.y, b.z, b.w};
            const float row[6] = {blk[lf[q]], x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3], blk[rt[q]]};
            const bool site = (ok >> q) & 1u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xc = row[k + 1];
                const float L = ((xc - row[k]) + (xc - row[k + 2])) + ((xc - va[k]) + (xc - vb[k]));
                const float x2 = xc * xc;
                const float gr = fmaf(kap, L, xc * fmaf(lam, x2, m2));
                const float t = xc * fmaf(0.5f * kap, L, xc * fmaf(0.25f * lam, x2, 0.5f * m2));
                cx.gr[4 * q + k] = site ? gr : 0.f;
                u += site ? t : 0.f;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// One-parameter item-response theory (NFMC_POT_ITEM_RESPONSE; S = p.n_components students, Q = d - 1 - S questions;
// (m0, p_mu, p_a, p_b) = p.b[0 .. 3]; p.a = the responses, Q rows of SA = 4 ceil(S / 4) floats, A[q][s] = 1 / 0 for an
// observed answer of student s to question q and any negative value for a missing one and for s >= S).  Coordinates
// x = [alpha_0 .. alpha_{S-1} | beta_0 .. beta_{Q-1} | mu]; with l_sq = (mu + alpha_s) - beta_q and r_sq =
// sigmoid(l_sq) - y_sq over the observed pairs:
//   U = 1/2 p_mu (mu - m0)^2 + 1/2 p_a sum_s alpha_s^2 + 1/2 p_b sum_q beta_q^2 + sum_sq [softplus(l_sq) - y_sq l_sq]
//   dU/dalpha_s = p_a alpha_s + sum_q r_sq,  dU/dbeta_q = p_b beta_q - sum_s r_sq,  dU/dmu = p_mu (mu - m0) + sum_sq r_sq
// Every pair is evaluated ONCE, by the lane that holds alpha_s, in one pass over the questions.  The workgroup's block is
// one row of DP + 4 floats per chain (irt_floats); prepare() stores the lane's quads into its chain's row as Phi4Pot
// does, reads mu once and, for question q, beta_q -- both the same address for all lanes of a chain, a broadcast -- and
// for each of its quads that holds a student (bit k of `am`, set once in init(): the only divergence) the aligned 16
// bytes at coordinate 4 (k LPC + g) of A[q]: a plain global load, consecutive lanes consecutive 16 bytes, every chain
// the same ones.  The block is the same for all chains and stays in L2; an LDS tile would need workgroup barriers in
// prepare() (LogRegPot's rule) for data each lane reads once per evaluation.  Mask and label come out of the one float
// without a branch (m = v >= 0, y = max(v, 0)), so a quad that straddles S, and padding, see "missing" for what is no
// student.  r_sq goes to the lane's own alpha registers; the lane's sum over its students, all-reduced over the chain's
// lanes (one butterfly per question: the fixed association of group_allreduce, no atomics, bitwise repeatable), is
// sum_s r_sq on every lane: lane 0 stores it over beta_q in the row, which is read no more, and every lane adds it to
// its copy of sum_sq r_sq, so mu's gradient needs no reduction of its own.  After the pass a lane reads the quads that
// hold questions (bit k of `bm`) back from the row.  Row pitch DP + 4: the broadcast reads are ds_read_b32 (bank =
// dword % 32, conflicts within a 32-lane half); at pitch DP chain j of the 32 / LPC chains of a half reads bank
// (j DP + const) % 32: one bank for DP >= 32 (4-way at LPC = 8, DP = 32 or 64; 2-way at LPC = 16) and two banks for the
// eight chains at DP = 16, LPC = 4 (4-way); at DP + 4 chain j sits at bank 4 j + const: distinct for the at most 8
// chains of a half at LPC >= 4; the quad stores and reads keep their 16-byte alignment.  The row is written and read
// by ONE wave, so wavefront fences order it (Phi4Pot) and no workgroup barrier is needed.  The data term is summed in
// fp64 per lane as in SparseLogRegPot, and term() puts the lane's share of U on its register 0.  Far in the tails x^2
// overflows fp32; U is then inf or NaN, the samplers reject the proposal and count its log ratio as non-finite.
template <int CPL, int LPC, bool FAST>
struct IrtPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    const float4* A;                     // this lane's quad 0 of A[0]
    int ns, nq, sa4;                     // S, Q, float4 per row of A
    float m0, pmu, pa, pb;
    uint32_t am, bm;                     // bit k: quad k holds a student / a question
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int d, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        ns = p.n_components;
        nq = d - 1 - ns;
        sa4 = (ns + 3) >> 2;
        A = reinterpret_cast<const float4*>(p.a) + g;
        m0 = p.b[0];
        pmu = p.b[1];
        pa = p.b[2];
        pb = p.b[3];
        am = bm = 0u;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const int c0 = 4 * (k * LPC + g);   // the quad's first coordinate (coord_of)
            if (c0 < ns) am |= 1u << k;
            if (c0 + 3 >= ns && c0 < ns + nq) bm |= 1u << k;
        }
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int k = 0; k < Q; ++k)
            *reinterpret_cast<float4*>(row + 4 * (k * LPC + g)) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        order();   // the wave's stores precede its reads
        const float mu = row[ns + nq];
        float acc[CPL];
#pragma unroll
        for (int i = 0; i < CPL; ++i) acc[i] = 0.f;
        double ul = 0.0;   // this lane's share of the data term, in fp64 (SparseLogRegPot)
        float sr = 0.f;    // sum_sq r_sq, the same on every lane of the chain
        const float4* aq = A;
        for (int q = 0; q < nq; ++q, aq += sa4) {
            const float beta = row[ns + q];
            float rs = 0.f;
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                if ((am >> k) & 1u) {
                    const float4 v4 = aq[k * LPC];
                    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float l = (mu + x[4 * k + j]) - beta;
                        float sp, sg;
                        softplus_sigmoid(l, sp, sg);
                        const bool m = v[j] >= 0.f;
                        const float y = fmaxf(v[j], 0.f);
                        const float r = m ? sg - y : 0.f;
                        acc[4 * k + j] += r;
                        rs += r;
                        ul += (double)(m ? sp - y * l : 0.f);
                    }
                }
            }
            const float tot = group_allreduce<LPC>(rs);   // sum_s r_sq
            sr += tot;
            if (g == 0) row[ns + q] = tot;                // beta_q is read no more
        }
        order();   // lane 0's stores precede the reads below
        Ctx cx;
        float u = 0.f;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((bm >> k) & 1u) t4 = *reinterpret_cast<const float4*>(row + 4 * (k * LPC + g));
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * k + j, c = 4 * (k * LPC + g) + j;
                const float xv = x[i], dm = xv - m0;
                const bool isa = c < ns, isb = !isa && c < ns + nq, ismu = c == ns + nq;
                const float prec = isa ? pa : (isb ? pb : (ismu ? pmu : 0.f));
                const float dev = ismu ? dm : xv;
                const float data = isa ? acc[i] : (isb ? -t[j] : (ismu ? sr : 0.f));
                const float pd = prec * dev;
                cx.gr[i] = (isa || isb || ismu) ? pd + data : 0.f;
                u += (isa || isb || ismu) ? 0.5f * pd * dev : 0.f;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        cx.u = (float)(ul + (double)u);
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// One group of the varying-effects regression: from its statistics s0 = (n, xbar, ybar, Sxx), s1 = (Sxy, Syy, 0, 0) and its
// effects (a, b) on the natural scale, Q_c = n e^2 + Syy - 2 b Sxy + b^2 Sxx with e = ybar - a - b xbar, and
// gA = -w_y n e, gB = w_y (-n e xbar - Sxy + b Sxx).  Shared by VaryEffPot and vfx_value_grad_row (neutra_kernels.hpp).
__device__ __forceinline__ void vfx_group(const float4& s0, const float4& s1, float a, float b, float wy, float& qc,
                                          float& ga, float& gb) {
    const float e = fmaf(-b, s0.y, s0.z - a), ne = s0.x * e, bs = fmaf(b, s0.w, -s1.x);   // bs = b Sxx - Sxy
    qc = fmaf(ne, e, fmaf(b, bs - s1.x, s1.y));
    ga = -wy * ne;
    gb = wy * fmaf(-ne, s0.y, bs);
}
// One group coordinate xv of a varying side (mu, w = e^{-2s}, es = e^{s}) with the likelihood's gradient gv with respect
// to the natural effect.  Centered: r = xv - mu, s1 += r, s2 += r^2, gradient gv + w r (the prior's 1/2 w sum r^2 is
// added from s2).  Non-centered: s1 += gv, s2 += gv xv, u += 1/2 xv^2, gradient es gv + xv.
__device__ __forceinline__ float vfx_vary(bool ncp, float xv, float mu, float w, float es, float gv, float& s1, float& s2,
                                          float& u) {
    if (ncp) {
        s1 += gv;
        s2 = fmaf(gv, xv, s2);
        u = fmaf(0.5f * xv, xv, u);
        return fmaf(es, gv, xv);
    }
    const float r = xv - mu;
    s1 += r;
    s2 = fmaf(r, r, s2);
    return fmaf(w, r, gv);
}
// The globals of one side and their share of U, from the chain-wide sums (s1, s2) of vfx_vary (varying side) or
// s1 = sum gV_c (shared side): g0 = dU/dmu or dU/dv, g1 = dU/ds.  fc = C.
__device__ __forceinline__ float vfx_side_globals(int mode, bool ncp, float mu, float s, float w, float es, float s1, float s2,
                                                  float fc, float P, float Hh, float& g0, float& g1) {
    g1 = 0.f;
    if (mode == 2) {
        const float he = Hh * fast_exp(2.f * s);
        g0 = ncp ? fmaf(P, mu, s1) : fmaf(P, mu, -w * s1);
        g1 = (ncp ? es * s2 : fmaf(-w, s2, fc)) + he - 1.f;
        return fmaf(0.5f * P * mu, mu, fmaf(0.5f, he, ncp ? -s : fmaf(fc, s, -s)));
    }
    g0 = mode == 1 ? fmaf(P, mu, s1) : 0.f;
    return mode == 1 ? 0.5f * P * mu * mu : 0.f;
}

// Gaussian regression with varying effects (NFMC_POT_VARYING_EFFECTS; C = p.n_components groups, p.a = the group table,
// C rows (n, xbar, ybar, Sxx, Sxy, Syy, 0, 0), (P, Hh) = p.b[0 .. 1], layout code = a_scalar (vfx_layout), N = b_scalar).
// The formulas are in nfmc_hip.h.  Coordinates: the group block -- (a_c, b_c) interleaved when both sides vary, so a
// pair is two neighbouring registers of one lane (coord_of: quads start at multiples of 4), or v_c alone -- then up to
// five globals.  The globals start at coordinate gb = 2 C or C, anywhere in a register quad, and may run into the next
// quad in coordinate order: quad gb / 4 is register quad kA of lane gA, quad gb / 4 + 1 register quad kB of lane gB,
// all four wave-uniform and set once in init().  prepare() (1) picks the two register quads by uniform compares
// (k == kA, no dynamic register index), masks them to the lanes that hold them, shifts by off = gb % 4 (uniform
// selects) and broadcasts each global that exists with one group_allreduce of the masked value (SparseLogRegPot's
// pattern); (2) evaluates the lane's groups: the statistics of group j are two 16-byte loads from the table -- read per
// evaluation at every layout, not kept in registers: at CPL = 16 they would be 48 registers beside the 16 of the state
// and the 16 of the gradient in kernels that also carry momentum, proposal and a flow tail, the table is at most 32 KiB,
// the same for all chains, and stays in L1 / L2, and consecutive lanes read consecutive rows; (3) all-reduces sum Q_c
// and two sums per side (five fixed-order butterflies: bitwise repeatable); (4) forms the globals' gradients on every
// lane and writes them back through the same compares into the registers of the lanes that hold them; the globals'
// share of U goes to lane 0.  No LDS block.  A register that holds neither a group coordinate nor a global (padding) has
// no bit in `pm`, adds exactly zero to U and to every sum and gets a zero gradient.  term() puts the lane's share of U
// on its register 0.  e^{-2s}, e^{2s}, e^{s} overflow fp32 far in the tails; U is then inf or NaN, the samplers reject
// the state and count its log ratio as non-finite.
template <int CPL, int LPC, bool FAST>
struct VaryEffPot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = false;
    static constexpr int Q = CPL / 4;   // register quads
    const float4* tab;                  // the group table, two float4 per group
    VfxLayout L;
    float P, Hh, nobs, fc;              // 1 / m^2, 1 / h^2, N, C
    int kA, kB, off;                    // register quads of the globals' first and second quad; gb % 4
    bool inA, inB, first;               // this lane holds the first / second quad; g == 0
    uint32_t pm;                        // bit i: register i is a group coordinate
    struct Ctx {
        float u;                        // this lane's share of U
        float gr[CPL];                  // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ void init(const NfmcPotential& p, int g, int) {
        tab = reinterpret_cast<const float4*>(p.a);
        vfx_layout(p.a_scalar, p.n_components, L);   // valid: check_vfx
        P = p.b[0];
        Hh = p.b[1];
        nobs = p.b_scalar;
        fc = (float)p.n_components;
        const int q0 = L.gb >> 2;
        off = L.gb & 3;
        kA = q0 / LPC;
        kB = (q0 + 1) / LPC;
        inA = g == q0 % LPC;
        inB = g == (q0 + 1) % LPC;
        first = g == 0;
        pm = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (coord_of<CPL, LPC>(g, i) < L.gb) pm |= 1u << i;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        // (1) the globals
        float cat[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // the two quads, each on the lane that holds it
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const bool a = inA && k == kA, b = inB && k == kB;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cat[j] = a ? x[4 * k + j] : cat[j];
                cat[4 + j] = b ? x[4 * k + j] : cat[4 + j];
            }
        }
        float val[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float v = cat[k];
#pragma unroll
            for (int o = 1; o < 4; ++o) v = off == o ? cat[k + o] : v;
            val[k] = group_allreduce<LPC>(k < L.ng ? v : 0.f);
        }
        const bool va = L.ma == 2, vb = L.mb == 2, ncp = L.ncp;
        // the roles by scalar selects on the uniform layout (an array indexed by L.ib or L.iy would go to scratch memory)
        const float v0 = val[0], v1 = val[1], v2 = val[2], v3 = val[3], v4 = val[4];
        const float mua = v0, sa = va ? v1 : 0.f;                         // mu_a or the shared a
        const float mub = L.mb ? (va ? v2 : v1) : 0.f;                    // mu_b, the shared b or 0
        const float sb = vb ? (va ? v3 : v2) : 0.f;
        const float sy = L.known ? 0.f : (L.iy == 1 ? v1 : L.iy == 2 ? v2 : L.iy == 3 ? v3 : v4);
        const float wy = L.known ? 1.f : fast_exp(-2.f * sy);
        const float wa = fast_exp(-2.f * sa), esa = fast_exp(sa), wb = fast_exp(-2.f * sb), esb = fast_exp(sb);
        // (2) the lane's groups
        Ctx cx;
        float u = 0.f, sq = 0.f, a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
        if (va && vb) {
#pragma unroll
            for (int p = 0; p < CPL / 2; ++p) {
                cx.gr[2 * p] = 0.f;
                cx.gr[2 * p + 1] = 0.f;
                if ((pm >> (2 * p)) & 1u) {
                    const int j = 2 * ((p >> 1) * LPC + g) + (p & 1);
                    const float4 s0 = tab[2 * j], s1 = tab[2 * j + 1];
                    const float xa = x[2 * p], xb = x[2 * p + 1];
                    float qc, ga, gb;
                    vfx_group(s0, s1, ncp ? fmaf(esa, xa, mua) : xa, ncp ? fmaf(esb, xb, mub) : xb, wy, qc, ga, gb);
                    sq += qc;
                    cx.gr[2 * p] = vfx_vary(ncp, xa, mua, wa, esa, ga, a1, a2, u);
                    cx.gr[2 * p + 1] = vfx_vary(ncp, xb, mub, wb, esb, gb, b1, b2, u);
                }
            }
            u = ncp ? u : fmaf(0.5f * wa, a2, fmaf(0.5f * wb, b2, u));
        } else {
            const float muv = va ? mua : mub, wv = va ? wa : wb, esv = va ? esa : esb;
            float v1 = 0.f, v2 = 0.f, o1 = 0.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                cx.gr[i] = 0.f;
                if ((pm >> i) & 1u) {
                    const int j = coord_of<CPL, LPC>(g, i);
                    const float4 s0 = tab[2 * j], s1 = tab[2 * j + 1];
                    const float xv = x[i], v = ncp ? fmaf(esv, xv, muv) : xv;
                    float qc, ga, gb;
                    vfx_group(s0, s1, va ? v : mua, va ? mub : v, wy, qc, ga, gb);
                    sq += qc;
                    cx.gr[i] = vfx_vary(ncp, xv, muv, wv, esv, va ? ga : gb, v1, v2, u);
                    o1 += va ? gb : ga;
                }
            }
            u = ncp ? u : fmaf(0.5f * wv, v2, u);
            a1 = va ? v1 : o1;
            a2 = va ? v2 : 0.f;
            b1 = va ? o1 : v1;
            b2 = va ? 0.f : v2;
        }
        u = fmaf(0.5f * wy, sq, u);
        // (3) the chain-wide sums
        sq = group_allreduce<LPC>(sq);
        a1 = group_allreduce<LPC>(a1);
        a2 = group_allreduce<LPC>(a2);
        b1 = group_allreduce<LPC>(b1);
        b2 = group_allreduce<LPC>(b2);
        // (4) the globals' gradients, in the order of the coordinates
        float ga0, ga1, gb0, gb1;
        float ug = vfx_side_globals(L.ma, ncp, mua, sa, wa, esa, a1, a2, fc, P, Hh, ga0, ga1);
        ug += vfx_side_globals(L.mb, ncp, mub, sb, wb, esb, b1, b2, fc, P, Hh, gb0, gb1);
        float gy = 0.f;
        if (!L.known) {
            const float he = Hh * fast_exp(2.f * sy);
            gy = fmaf(-wy, sq, nobs) + he - 1.f;
            ug += fmaf(nobs, sy, fmaf(0.5f, he, -sy));
        }
        float gl[5];
        gl[0] = ga0;
        gl[1] = va ? ga1 : (L.mb ? gb0 : gy);
        gl[2] = va ? (L.mb ? gb0 : gy) : (vb ? gb1 : gy);
        gl[3] = (va && vb) ? gb1 : gy;
        gl[4] = gy;
        float cg[8];   // the gradients at their places in the two quads
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (q - o >= 0 && q - o < 5) v = off == o ? gl[q - o] : v;
            cg[q] = v;
        }
        const int end = off + L.ng;   // the globals are places off .. end - 1 of the two quads
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const bool a = inA && k == kA, b = inB && k == kB;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cx.gr[4 * k + j] = (a && j >= off && j < end) ? cg[j] : cx.gr[4 * k + j];
                cx.gr[4 * k + j] = (b && 4 + j < end) ? cg[4 + j] : cx.gr[4 * k + j];
            }
        }
        cx.u = first ? u + ug : u;
        return cx;
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// One pair of particles at squared distance s: e = beta phi(r) and w = beta phi'(r) / r, the factor of (r_i - r_j) in
// the force.  Lennard-Jones (p0 = beta eps, p1 = r_m^2) from s alone, t = r_m^2 / s:  e = p0 t^3 (t^3 - 2),
// w = -12 p0 t^3 (t^3 - 1) / s; at s = 0 e = inf and w (r_i - r_j) = NaN: the samplers reject the state.  Double well
// (p0 .. p2 = beta (a, b, c), p3 = r0) with u = sqrt(s) - r0:  e = u (p0 + u (p1 + p2 u^2)), w = (p0 + u (2 p1 + 4 p2
// u^2)) / sqrt(s), and w = 0 at s = 0.  Shared by ParticlePot and particles_value_grad_row (neutra_kernels.hpp).
template <bool LJ>
__device__ __forceinline__ void particle_pair(float s, float p0, float p1, float p2, float p3, float& e, float& w) {
    if constexpr (LJ) {
        const float is = __builtin_amdgcn_rcpf(s), t = p1 * is, t3 = t * t * t;
        const float pt = p0 * t3;
        e = pt * (t3 - 2.f);
        w = -12.f * pt * (t3 - 1.f) * is;
    } else {
        const float u = __builtin_amdgcn_sqrtf(s) - p3, u2 = u * u;
        e = u * fmaf(u, fmaf(p2, u2, p1), p0);
        w = s > 0.f ? fmaf(u, fmaf(4.f * p2, u2, 2.f * p1), p0) * __builtin_amdgcn_rsqf(s) : 0.f;
    }
}

// Interacting particles (NFMC_POT_PARTICLES; P = p.n_components particles in D = d / P dimensions, particle-major
// x = [r_0 | .. | r_{P-1}]; p.a = (pair code 0 Lennard-Jones / 1 double well, D, beta k, four pair parameters, 0)):
//   U = 1/2 beta k sum_i |r_i|^2 + sum_{i<j} beta phi(r_ij),   dU/dr_i = beta k r_i + sum_{j != i} w(r_ij) (r_i - r_j)
// (particle_pair).  Every coordinate meets every other, and a particle's D coordinates straddle register quads and
// lanes, so the chain's state goes through a wave-private LDS row as in IrtPot (one row of DP + 4 floats per chain,
// particles_floats; the pitch for IrtPot's bank reason: the reads below are the same broadcasts).  prepare() stores the
// lane's quads into the row (ds_write_b128).  Particle p belongs to lane p % LPC of its chain: lane g owns particles g,
// g + LPC, .., at most NP = ceil(CPL / D) of them (P D <= CPL LPC), keeps their positions and forces in registers and
// loops j = 0 .. P-1 -- a uniform trip count; r_j is read from the row at an address all lanes of the chain share, a
// broadcast -- adding w (r_p - r_j) to the force of each owned p and 1/2 beta phi to its share of U.  An unordered pair
// is evaluated twice, once per owner: no atomics and a fixed summation order, so runs are bitwise repeatable.  j = p
// and owned slots p >= P are taken out by a select on w and e, not by a branch; slot m is skipped when no lane of the
// wave owns a particle in it (m LPC >= P, uniform).  D and the pair form are wave-uniform and chosen ONCE, outside the
// loops (pairs<D, LJ>): NP and the register arrays have compile-time bounds.  After the loop the owners write their
// forces over their particles' slots in the row -- every read of a position is behind them: one wave, LDS operations
// complete in order, a fence between -- and each lane reads back the quads it holds as the pair part of dU/dx and adds
// the trap term from its own registers.  Padding coordinates (c >= d) get a zero gradient and add zero to U.  No
// workgroup barrier (LogRegPot's rule); wavefront fences as in Phi4Pot.  term() puts the lane's share of U on register 0.
template <int CPL, int LPC, bool FAST>
struct ParticlePot {
    static constexpr bool kQuadratic = false;
    static constexpr bool kStaged = true;
    static constexpr int DP = CPL * LPC;
    static constexpr int Q = CPL / 4;    // register quads
    static constexpr int PITCH = DP + 4;
    float* row;                          // LDS: this chain's row
    int np, nd, dd;                      // P, D, d
    bool lj;
    float bk, p0, p1, p2, p3;            // beta k and the pair parameters
    struct Ctx {
        float u;                         // this lane's share of U
        float gr[CPL];                   // dU/dx of this lane's coordinates
    };

    __device__ __forceinline__ static void order() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ static void stage(float*, const NfmcPotential&, int) {}   // the rows are the lanes' own
    __device__ __forceinline__ void init(const NfmcPotential& p, int, int d, float* lds) {
        row = lds + (int)(threadIdx.x / LPC) * PITCH;
        np = p.n_components;
        dd = d;
        nd = d / np;
        lj = p.a[0] == 0.f;
        bk = p.a[2];
        p0 = p.a[3];
        p1 = p.a[4];
        p2 = p.a[5];
        p3 = p.a[6];
    }
    template <int D, bool LJ>
    __device__ __forceinline__ Ctx pairs(const float (&x)[CPL], int g) const {
        constexpr int NP = (CPL + D - 1) / D;   // owned particles per lane, at most
        order();   // behind the reads of the previous evaluation
#pragma unroll
        for (int k = 0; k < Q; ++k)
            *reinterpret_cast<float4*>(row + 4 * (k * LPC + g)) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
        order();   // the wave's stores precede its reads
        float rp[NP][D], f[NP][D], e = 0.f;
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            const int own = min(m * LPC + g, np - 1);   // a slot past P reads particle P - 1 and is selected away
#pragma unroll
            for (int c = 0; c < D; ++c) {
                rp[m][c] = row[own * D + c];
                f[m][c] = 0.f;
            }
        }
#pragma unroll 1
        for (int j = 0; j < np; ++j) {
            float rj[D];
#pragma unroll
            for (int c = 0; c < D; ++c) rj[c] = row[j * D + c];
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                if (m * LPC < np) {   // uniform
                    float dx[D], s = 0.f;
#pragma unroll
                    for (int c = 0; c < D; ++c) {
                        dx[c] = rp[m][c] - rj[c];
                        s = fmaf(dx[c], dx[c], s);
                    }
                    float ep, w;
                    particle_pair<LJ>(s, p0, p1, p2, p3, ep, w);
                    const int own = m * LPC + g;
                    const bool on = own != j && own < np;
                    e += on ? ep : 0.f;
                    w = on ? w : 0.f;
#pragma unroll
                    for (int c = 0; c < D; ++c) f[m][c] = fmaf(w, dx[c], f[m][c]);
                }
            }
        }
        order();   // every read of a position precedes the owners' stores
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            const int own = m * LPC + g;
            if (own < np) {
#pragma unroll
                for (int c = 0; c < D; ++c) row[own * D + c] = f[m][c];
            }
        }
        order();   // the owners' stores precede the reads below
        Ctx cx;
        float u = 0.5f * e;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const float4 t4 = *reinterpret_cast<const float4*>(row + 4 * (k * LPC + g));
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * k + j;
                const bool in = 4 * (k * LPC + g) + j < dd;
                const float xv = x[i], kx = bk * xv;
                cx.gr[i] = in ? kx + t[j] : 0.f;
                u += in ? 0.5f * kx * xv : 0.f;
            }
        }
        order();   // the next evaluation's stores stay behind these reads
        cx.u = u;
        return cx;
    }
    __device__ __forceinline__ Ctx prepare(const float (&x)[CPL], int g, int) const {
        if (lj) return nd == 3 ? pairs<3, true>(x, g) : (nd == 2 ? pairs<2, true>(x, g) : pairs<1, true>(x, g));
        return nd == 3 ? pairs<3, false>(x, g) : (nd == 2 ? pairs<2, false>(x, g) : pairs<1, false>(x, g));
    }
    __device__ __forceinline__ float grad(const Ctx& cx, int i, float) const { return cx.gr[i]; }
    __device__ __forceinline__ float term(const Ctx& cx, int i, float) const { return i == 0 ? cx.u : 0.f; }
};

// Potentials with an LDS block (kStaged) stage it behind the `img_floats` floats of flow image a kernel keeps at the
// start of its dynamic LDS (16-byte aligned), synchronise the workgroup and bind to it.  lds_with_potential() is the
// host side: the kernel's dynamic LDS bytes for an image of `img_bytes` at layout (cpl, lpc).
template <class P>
__device__ __forceinline__ void init_staged(P& pot, const NfmcPotential& p, int g, int d, float* lds, int img_floats) {
    float* blk = lds + ((img_floats + 3) & ~3);
    P::stage(blk, p, d);
    __syncthreads();
    pot.init(p, g, d, blk);
}
inline size_t lds_with_potential(size_t img_bytes, const NfmcPotential& p, int cpl, int lpc) {
    const size_t blk = staged_potential_bytes(p, cpl * lpc, cpl);
    return blk ? ((img_bytes + 15) & ~(size_t)15) + blk : img_bytes;
}

// ------------------------------------------------------------------------------------------------
// Row IO: register quad q of lane g <-> the 16 bytes at coordinate 4 * (q * LPC + g) of the row.
template <int CPL, int LPC, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ base, int64_t row, int d, int g, bool active,
                                         float (&x)[CPL]) {
    if constexpr (VEC) {
        const float4* p = reinterpret_cast<const float4*>(base + row * d) + g;
#pragma unroll
        for (int q = 0; q < CPL / 4; ++q) {
            float4 v = active ? p[q * LPC] : make_float4(0.f, 0.f, 0.f, 0.f);
            x[4 * q] = v.x;
            x[4 * q + 1] = v.y;
            x[4 * q + 2] = v.z;
            x[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            x[i] = (active && c < d) ? base[row * d + c] : 0.f;
        }
    }
}

template <int CPL, int LPC, bool VEC>
__device__ __forceinline__ void store_row(float* __restrict__ base, int64_t row, int d, int g, bool active,
                                          const float (&x)[CPL]) {
    if constexpr (VEC) {
        if (active) {
            float4* p = reinterpret_cast<float4*>(base + row * d) + g;
#pragma unroll
            for (int q = 0; q < CPL / 4; ++q)
                p[q * LPC] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = coord_of<CPL, LPC>(g, i);
            if (active && c < d) base[row * d + c] = x[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Kept states (NfmcSampleStore): which transitions of a launch are kept, and in which ring row, is wave-uniform
// bookkeeping on scalars -- a countdown to the next kept transition and the row it goes to, advanced without divisions.
struct StoreCursor {
    float* base;
    int stride, countdown, ring, row;
    __device__ __forceinline__ explicit StoreCursor(const NfmcSampleStore& s)
        : base(s.base), stride(s.stride), countdown(s.countdown), ring(s.ring_rows), row(s.row) {}
    // the store row (pointer to its n*d floats) the CURRENT transition is kept in, or nullptr; advances to the next one
    __device__ __forceinline__ float* next(int64_t nd) {
        if (!base) return nullptr;
        if (countdown > 0) {
            --countdown;
            return nullptr;
        }
        float* p = base + (int64_t)row * nd;
        row = row + 1 == ring ? 0 : row + 1;
        countdown = stride - 1;
        return p;
    }
};
// the same for transition t of the call, out of order (the data-parallel IMH replay writes runs of equal states)
__device__ __forceinline__ float* store_row_of(const NfmcSampleStore& s, int t, int64_t nd) {
    const int k = t - s.countdown;
    if (!s.base || k < 0 || k % s.stride != 0) return nullptr;
    return s.base + (int64_t)((s.row + k / s.stride) % s.ring_rows) * nd;
}
// f(row pointer) for every KEPT transition t of the call in [t0, t1), in order: one division for the run instead of three
// per transition (the replay writes a state that lasted c steps into every kept row of those c: with thinning most of
// the c lookups found nothing, 0.8 ms of a 1.1 ms replay at the C2 shape with every 250th state kept)
template <class F>
__device__ __forceinline__ void store_rows_in(const NfmcSampleStore& s, int t0, int t1, int64_t nd, F f) {
    if (!s.base) return;
    int k0 = t0 - s.countdown;
    if (k0 < 0) k0 = 0;
    const int j = (k0 + s.stride - 1) / s.stride;             // first kept index at or after t0
    int row = (s.row + j) % s.ring_rows;
    for (int t = s.countdown + j * s.stride; t < t1; t += s.stride) {
        f(s.base + (int64_t)row * nd);
        row = row + 1 == s.ring_rows ? 0 : row + 1;
    }
}
// the store descriptor of the NEXT launch after one that offered k transitions (host side of StoreCursor)
inline void store_advance(NfmcSampleStore& s, int k) {
    if (!s.base) return;
    if (k <= s.countdown) {
        s.countdown -= k;
        return;
    }
    const int rest = k - s.countdown;                       // from the launch's first kept transition to its end
    const int kept = (rest + s.stride - 1) / s.stride;
    s.row = (s.row + kept) % s.ring_rows;
    s.countdown = s.stride - 1 - (rest - ((kept - 1) * s.stride + 1));
}
inline bool store_ok(const NfmcSampleStore& s) {
    return !s.base || (s.stride >= 1 && s.countdown >= 0 && s.countdown < s.stride && s.ring_rows >= 1 && s.row >= 0 &&
                       s.row < s.ring_rows);
}

// ------------------------------------------------------------------------------------------------
// Deterministic statistics.  Each lane carries fp32 partial sums over the <= 512 steps of one call;
// they are widened to fp64, reduced over the chains of the wave by shuffles, over the waves of the
// workgroup through LDS, written to the workgroup's slot of the scratch slab, and a second tiny
// kernel folds the slab into the accumulators in a fixed order (no atomics: run-to-run bitwise equal).
template <int CPL, int LPC>
__device__ __forceinline__ void block_stats_flush(const float (&sx)[CPL], const float (&sxx)[CPL], uint32_t accepted,
                                                  uint32_t nonfinite, const NfmcStats& st,
                                                  uint32_t jump_accepted = 0, uint32_t jump_nonfinite = 0,
                                                  const double* __restrict__ extra = nullptr) {
    // extra: 2 * DP sums another kernel prepared for this workgroup, added to its slab (imh_parallel.hip)
    double* __restrict__ scratch = st.scratch;
    const bool defer = st.defer != 0;
    const int slot = defer ? st.tail_slot : 0;   // deferred jumps book their counts in the jump slots
    constexpr int DP = CPL * LPC;
    __shared__ double red[kWavesPerBlock][2 * DP + kStatTail];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane % LPC;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const double a = (double)cross_chain_reduce<LPC>(sx[i]);
        const double b = (double)cross_chain_reduce<LPC>(sxx[i]);
        if (lane < LPC) {
            red[wave][coord_of<CPL, LPC>(g, i)] = a;
            red[wave][DP + coord_of<CPL, LPC>(g, i)] = b;
        }
    }
    if (lane == 0) {
        red[wave][2 * DP + 0] = slot == 0 ? (double)accepted : 0.0;
        red[wave][2 * DP + 1] = slot == 0 ? (double)nonfinite : 0.0;
        red[wave][2 * DP + 2] = slot == 0 ? (double)jump_accepted : (double)accepted;
        red[wave][2 * DP + 3] = slot == 0 ? (double)jump_nonfinite : (double)nonfinite;
    }
    __syncthreads();
    double* out = scratch + (size_t)blockIdx.x * (2 * DP + kStatTail);
    for (int t = threadIdx.x; t < 2 * DP + kStatTail; t += kBlock) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) s += red[w][t];
        if (extra && t < 2 * DP) s += extra[t];
        out[t] = defer ? out[t] + s : s;   // one owner thread per (workgroup, column): no race, fixed order
    }
}

// scratch (nblocks, 2*dp + kStatTail) -> stats (+=).  Workgroup b owns 32 columns; its 256 threads are
// 32 columns x 8 row-slices (loads coalesced across columns, 8 independent chains per column), and the 8
// partials of a column are added in slice order, so the result does not depend on timing.
constexpr int kFinishCols = 32, kFinishSlices = 32, kFinishBlock = kFinishCols * kFinishSlices;
template <bool ZERO>
static __device__ __forceinline__ double take(double* p) {
    const double v = *p;
    if (ZERO) *p = 0.0;
    return v;
}

// ZERO: the slabs are zeroed as they are read, so the scratch is all-zero again after every fold.  Every launch site
// uses it: a fold-per-call launch leaves nothing behind that a later DEFERRED launch (which adds to the slabs) could
// pick up when the two modes are mixed within one run.
template <bool ZERO = false>
static __global__ void __launch_bounds__(kFinishBlock) stats_finish_kernel(double* __restrict__ scratch,
                                                                           int nblocks, int dp, int d, NfmcStats st,
                                                                           unsigned long long attempted,
                                                                           unsigned long long* jump_counters = nullptr,
                                                                           unsigned long long jump_attempted = 0) {
    __shared__ double part[kFinishSlices][kFinishCols];
    const int width = 2 * dp + kStatTail;
    const int col = threadIdx.x % kFinishCols, slice = threadIdx.x / kFinishCols;
    const int t = blockIdx.x * kFinishCols + col;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;  // four loads in flight per thread, combined in fixed order
    if (t < width) {
        int b = slice;
        for (; b + 3 * kFinishSlices < nblocks; b += 4 * kFinishSlices) {
            p0 += take<ZERO>(scratch + (size_t)b * width + t);
            p1 += take<ZERO>(scratch + (size_t)(b + kFinishSlices) * width + t);
            p2 += take<ZERO>(scratch + (size_t)(b + 2 * kFinishSlices) * width + t);
            p3 += take<ZERO>(scratch + (size_t)(b + 3 * kFinishSlices) * width + t);
        }
        for (; b < nblocks; b += kFinishSlices) p0 += take<ZERO>(scratch + (size_t)b * width + t);
    }
    part[slice][col] = (p0 + p1) + (p2 + p3);
    __syncthreads();
    if (slice == 0 && t < width) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kFinishSlices; ++k) s += part[k][col];
        if (t < dp) {
            if (t < d) st.sum_x[t] += s;
        } else if (t < 2 * dp) {
            if (t - dp < d) st.sum_x2[t - dp] += s;
        } else if (t == 2 * dp) {
            st.counters[NFMC_CNT_ACCEPTED] += (unsigned long long)(s + 0.5);
            st.counters[NFMC_CNT_ATTEMPTED] += attempted;
        } else if (t == 2 * dp + 1) {
            st.counters[NFMC_CNT_NONFINITE] += (unsigned long long)(s + 0.5);
        } else if (t == 2 * dp + 2 && jump_counters) {
            jump_counters[NFMC_CNT_ACCEPTED] += (unsigned long long)(s + 0.5);
            jump_counters[NFMC_CNT_ATTEMPTED] += jump_attempted;
        } else if (t == 2 * dp + 3 && jump_counters) {
            jump_counters[NFMC_CNT_NONFINITE] += (unsigned long long)(s + 0.5);
        }
    }
}

inline int stats_finish_grid(int dp) { return (2 * dp + kStatTail + kFinishCols - 1) / kFinishCols; }

inline int64_t stats_scratch_doubles(int dp) { return (int64_t)kMaxGrid * (2 * dp + kStatTail); }

inline int padded_d(int d);

// Deferred statistics (NfmcStats.defer): every kernel of a run must lay its slabs out with the same width,
// 2 * padded_d(d) + kStatTail, and the scratch must hold kMaxGrid of them (nfmc_stats_fold_f32 reads them all).
inline int check_defer(const NfmcStats& s, int dp, int d) {
    if (!s.sum_x || !s.defer) return 0;
    if (dp != padded_d(d) || (s.tail_slot != 0 && s.tail_slot != 2)) return -1;
    if (s.scratch_bytes < stats_scratch_doubles(dp) * (int64_t)sizeof(double)) return -1;
    return 0;
}

inline int padded_d(int d) {
    int p = 4;
    while (p < d) p <<= 1;
    return p;
}

// Launch `kern` with `lds` bytes of dynamic LDS, raising the kernel's limit first where the launch needs more than the
// 48 KB every kernel may have: the hipError_t of a failed attribute call, else NFMC_OK (a failed launch shows in
// NFMC_HIP_CHECK_LAUNCH).  Per call: the attribute belongs to the (kernel, device) pair, and a process may drive several.
template <class K, class... Args>
int launch_lds(K kern, int grid, int block, size_t lds, hipStream_t st, const Args&... args) {
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, args...);
    return NFMC_OK;
}

#define NFMC_HIP_CHECK_LAUNCH()                \
    do {                                       \
        hipError_t e_ = hipGetLastError();     \
        if (e_ != hipSuccess) return (int)e_;  \
    } while (0)

}  // namespace nfmc
