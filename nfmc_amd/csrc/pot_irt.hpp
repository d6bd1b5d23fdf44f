// Item-response theory (kind 9): its register class and its one-row NeuTra form.
#pragma once

#include "pot_shared.hpp"

namespace nfmc {

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

// Item-response theory (NFMC_POT_ITEM_RESPONSE) for the row of one chain, as potential_value_grad_row: U and dU/dx of
// IrtPot (above), x = [alpha (S) | beta (Q) | mu].  One pass over the questions: the students' entries of the
// gradient row accumulate r_sq = sigmoid(l_sq) - y_sq, question q's entry gets -sum_s r_sq when its row is done, and the
// sum of those is mu's.  The responses are wave-uniform (scalar loads); a negative entry is a missing answer.  The data
// term is summed in fp64, as in IrtPot.  grow[s] += r is a read and a write of the lane's own LDS row per pair, beside
// the exp, log and reciprocal of softplus_sigmoid: the price of evaluating every pair once with the responses read in
// storage order (a second pass for the students' sums would evaluate every pair twice, student-major blocks would
// read each 64-byte line of the responses in four far-apart visits).  Kept out of potential_value_grad_row, which the fit and DLMC kernels share and
// which never see kind 9.
__device__ __forceinline__ float irt_value_grad_row(const float* __restrict__ row, float* __restrict__ grow,
                                                    const NfmcPotential& p, int d) {
    const int ns = p.n_components, nq = d - 1 - ns, sa = (ns + 3) & ~3;
    const float m0 = p.b[0], pmu = p.b[1], pa = p.b[2], pb = p.b[3], mu = row[d - 1];
    float u = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float a = row[s];
        grow[s] = pa * a;
        u = fmaf(0.5f * pa * a, a, u);
    }
    double ul = 0.0;
    float sr = 0.f;
    for (int q = 0; q < nq; ++q) {
        const float* __restrict__ aq = p.a + (int64_t)q * sa;
        const float beta = row[ns + q];
        float rs = 0.f;
        for (int s = 0; s < ns; ++s) {
            const float v = aq[s];
            if (v >= 0.f) {   // wave-uniform
                const float l = (mu + row[s]) - beta;
                float sp, sg;
                softplus_sigmoid(l, sp, sg);
                const float r = sg - v;
                grow[s] += r;
                rs += r;
                ul += (double)(sp - v * l);
            }
        }
        grow[ns + q] = fmaf(pb, beta, -rs);
        u = fmaf(0.5f * pb * beta, beta, u);
        sr += rs;
    }
    const float dm = mu - m0;
    grow[d - 1] = fmaf(pmu, dm, sr);
    return (float)(ul + (double)fmaf(0.5f * pmu * dm, dm, u));
}

}  // namespace nfmc
