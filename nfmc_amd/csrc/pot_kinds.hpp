// The potential kinds as the host sees them: argument checks, LDS sizes, the kPotKinds table and the families that run them.
#pragma once

#include "common.hpp"

namespace nfmc {

constexpr int kMixMaxK = 8;   // components of a Gaussian mixture (MixturePot, pot_basic.hpp)

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
//   1. nfmc_hip.h: its NFMC_POT_* value and descriptor fields; here: its check_* function, its *_bytes function if its
//      class stages an LDS block, and its row.  The check answers NFMC_EINVAL / NFMC_EALIGN for a malformed descriptor
//      and NFMC_EUNSUPPORTED for a well-formed one no kernel runs (check_phi4: a row length that is no multiple of 4);
//      it sees host values only, never what a or b point to.  The *_bytes function gets the layout as (DP, CPL): a
//      read-only table is sized by DP, a block with a slot per chain by CPL (phi4_bytes), or by both where its rows are
//      padded (irt_bytes).
//   2. Its header pot_<kind>.hpp, which holds all of its device code and includes pot_shared.hpp (or less) and no other
//      kind's header: the class Pot<CPL, LPC, FAST> (prepare / grad / term, and stage() if kStaged) and, for
//      neutra_valu, its *_value_grad_row, with the helpers the two share.  A block the lanes write (Phi4Pot) must not
//      rely on workgroup barriers inside prepare() unless every thread of the workgroup calls it equally often
//      (LogRegPot's rule).  A class that reads its data straight from global memory (VaryEffPot) has kStaged = false,
//      the three-argument init(p, g, d) and nullptr for the *_bytes function in its row.
//      A class in which every coordinate meets every other (ParticlePot) exchanges the chain's state through a
//      wave-private LDS row like Phi4Pot and IrtPot; its number of registers depends on how many objects a lane owns,
//      which depends on a run-time shape (D): dispatch on that shape ONCE per prepare(), outside the loops, to bodies
//      with compile-time bounds, or a register array indexed by it goes to scratch memory.
//   3. own_units: a line in NFMC_FOR_OWN_UNIT_POT and four units that include the header and instantiate
//      launch_{mala,hmc}_kind and launch_b_kind{,_rqs} for the class (sampler_slr_mala.hip and its three siblings are
//      the pattern).  The build picks up every .hip file of this directory; a unit that takes a minute or more also
//      goes into SLOW_FIRST (nfmc_amd/build.py).  neutra_valu: the header's include and the kind's arm of
//      adjusted_potential_grad_row in neutra_kernels.hpp, and `neutra_matrix_cores = False` on its class in
//      nfmc_amd/potentials.py, which keeps it off the matrix-core kernels (NeuTra._min_hidden reads it).
//   4. Python: POT_* in nfmc_amd/hip.py, its class in nfmc_amd/potentials.py, an fp64 oracle tests/<kind>_fp64.py and
//      tests/test_{host,gpu}_<kind>.py, which assert the codes of step 1's check; its units in the table of
//      tests/test_host_include_structure.py.
//   5. Words: the kind's comment in nfmc_hip.h, its line in INTEGRATION.md, its paragraph in README.md and its
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

// the device classes by name, for the declarations that need no more (each is defined in its kind's pot_*.hpp)
#define NFMC_DECLARE_POT(KIND, POT) template <int CPL, int LPC, bool FAST> struct POT;
NFMC_FOR_OWN_UNIT_POT(NFMC_DECLARE_POT)
#undef NFMC_DECLARE_POT

// a kernel's dynamic LDS bytes for a flow image of `img_bytes` at layout (cpl, lpc): init_staged (pot_shared.hpp)
inline size_t lds_with_potential(size_t img_bytes, const NfmcPotential& p, int cpl, int lpc) {
    const size_t blk = staged_potential_bytes(p, cpl * lpc, cpl);
    return blk ? ((img_bytes + 15) & ~(size_t)15) + blk : img_bytes;
}

}  // namespace nfmc
