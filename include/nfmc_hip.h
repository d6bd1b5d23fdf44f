/*
 * nfmc_hip.h -- C ABI of libnfmc_hip.so: the MI355X (gfx950) implementation of the nfmc hot path.
 *
 * The reference (davidnabergoj/nfmc) is pure Python on PyTorch and has no FFI; its two seams for
 * this path are `MCMCSampler.propose` (nfmc/algorithms/sampling/mcmc/base.py:27-34) and the
 * torchflows `Flow` methods called at jump.py:205,218, imh.py:214,221, neutra.py:60.  Each entry
 * point below names the reference code it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   ownership   every pointer is a BORROWED device allocation (e.g. torch tensor.data_ptr());
 *               the library never allocates or frees user-visible memory; scratch is caller-supplied.
 *   layout      row-major contiguous fp32 `(n, d)` state, `(n,)` per-chain vectors, u8 masks.
 *   errors      return 0 on success; negative = argument error (NFMC_E*); positive = hipError_t.
 *               No C++ exception crosses the boundary.
 *   async       every call only enqueues work on `stream` (a hipStream_t) and returns; re-entrant,
 *               no global mutable state.
 *   rng         native mode: Philox4x32-10 keyed by `seed`, counter (chain id, transition, block, stream)
 *               -- spec in oracle/philox.py; replay mode: caller-supplied normals/uniforms
 *               (non-NULL replay pointers), used for parity tests against the reference's noise.
 */
#ifndef NFMC_HIP_H
#define NFMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nfmc_stream_t; /* hipStream_t */

#define NFMC_ABI_VERSION 4

enum {
    NFMC_OK = 0,
    NFMC_EINVAL = -1,       /* NULL pointer / non-positive size */
    NFMC_ESHAPE = -2,       /* shape outside what the kernels support (see nfmc_limits) */
    NFMC_EALIGN = -3,       /* pointer not aligned as required (state rows: 4 B; 16 B enables vector IO) */
    NFMC_EUNSUPPORTED = -4, /* valid request with no kernel instantiation (e.g. unknown potential kind) */
    NFMC_ESCRATCH = -5      /* scratch buffer too small: see nfmc_stats_scratch_bytes */
};

/* ---- closed-form potentials U(x) (negative log density), evaluated with their gradient in-kernel.
 * Replaces `self.target(x)` + `torch.autograd.grad` (langevin.py:66-68,80-82; hmc.py:40-48). */
enum {
    NFMC_POT_QUADRATIC = 0, /* U = sum_j a_j (x_j - b_j)^2 ; a,b per coordinate or scalar */
    NFMC_POT_FUNNEL = 1,    /* U = x_0^2/(2 s^2) + sum_{i>=1} [x_i^2 / (2 e^{x_0}) + x_0/2], s = a_scalar */
    NFMC_POT_GAUSSIAN_MIXTURE = 2,
    /* Diagonal Gaussian mixture of K = n_components components:
         U = -logsumexp_k [ c_k - 1/2 sum_j lam_kj (x_j - mu_kj)^2 ],  lam_kj = 1/sigma_kj^2,
         c_k = log w_k + 1/2 sum_j log lam_kj   (the constant d/2 log 2 pi is dropped)
       a -> fp32 block [lam (K, d) row-major | c (K)],  b -> means mu (K, d) row-major; both device memory, 16-byte
       aligned; a_scalar / b_scalar unused.  K <= 8, and the kernel stages 2 K padded_d(d) floats of it in LDS beside its
       flow image: a larger K, or a block that does not fit, gets NFMC_EUNSUPPORTED.  Served by nfmc_mala_steps_f32 /
       nfmc_hmc_steps_f32 (general kernels, with or without a jump tail; not the Philox4x32-7 stream) and by the
       register-layout kernels of nfmc_flow_mh_steps_f32; every other entry point answers NFMC_EUNSUPPORTED. */
    NFMC_POT_LOGISTIC_REGRESSION = 3,
    /* Bayesian logistic regression over N = n_components data rows, prior x ~ N(0, s^2 I):
         U = sum_i [softplus(z_i) - y_i z_i] + |x|^2 / (2 s^2),  z_i = X_i . x,  softplus(z) = max(z, 0) + log1p(e^-|z|)
         dU/dx = X^T (sigmoid(z) - y) + x / s^2   (constants dropped)
       a -> X (N, d) fp32 row-major, device memory, 16-byte aligned;  b -> y (N,) fp32, values 0 or 1, device memory;
       a_scalar = 1/s^2 > 0;  b_scalar unused.  No cap on N (each evaluation streams X through an LDS tile of 16 KB plus
       the tile's labels; a flow image that leaves no room for it gets NFMC_EUNSUPPORTED).  Served by nfmc_mala_steps_f32
       / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail; not the Philox4x32-7 stream) and by the
       register-layout kernels of nfmc_flow_mh_steps_f32; every other entry point answers NFMC_EUNSUPPORTED. */
    NFMC_POT_GAUSSIAN_FULL = 4,
    /* Full-rank Gaussian with precision Lambda (symmetric positive definite) and mean mu:
         U = 1/2 (x - mu)^T Lambda (x - mu),   dU/dx = Lambda (x - mu)   (constants dropped)
       a -> Lambda (d, d) fp32 row-major, device memory, 16-byte aligned;  b -> mu (d,) fp32, device memory;
       n_components = d (a mismatch, a NULL a or b, or a misaligned a is NFMC_EINVAL);  a_scalar / b_scalar unused.
       Each evaluation streams Lambda through an LDS tile of 16 KB (a flow image that leaves no room for it gets
       NFMC_EUNSUPPORTED).  Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump
       tail, device warmup tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU
       NeuTra kernels (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_ROSENBROCK = 5,
    /* Blocked (hybrid) Rosenbrock over the flattened coordinates, split into consecutive blocks of B coordinates (the
       last one may be shorter); coordinate c is a head when c % B == 0:
         U = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2   (constants dropped)
         dU/dx_c = [c head] 2a (x_c - mu) + [c non-head] 2b (x_c - x_{c-1}^2) - [c+1 < d non-head] 4b x_c (x_{c+1} - x_c^2)
       n_components = B (1 <= B <= d);  a_scalar = a > 0, b_scalar = b > 0 (finite);  a -> mu, ONE fp32 in device memory;
       b unused.  A NULL a, B out of range, or a / b not positive and finite is NFMC_EINVAL.  Served by
       nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup tuning
       included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_STOCHASTIC_VOLATILITY = 6,
    /* Stochastic-volatility model (Stan User's Guide) over d = T + 3 coordinates: x_0 = mu, x_1 = s = log sigma,
       x_2 = r = atanh phi, x_{3+t} = h_t (t = 0 .. T-1); mu ~ Cauchy(0, c_mu), sigma ~ HalfCauchy(0, c_sigma),
       (phi + 1)/2 ~ Beta(alpha, beta), h_0 ~ N(mu, sigma^2/(1 - phi^2)), h_t | h_{t-1} ~ N(mu + phi (h_{t-1} - mu), sigma^2),
       y_t ~ N(0, e^{h_t}).  With w = e^{-2s}, phi = tanh r, q = 1 - phi^2, delta_0 = h_0 - mu, a_t = h_{t-1} - mu and
       e_t = h_t - mu - phi a_t (t >= 1), the Jacobians of s and r included and constants dropped:
         U = log1p((mu/c_mu)^2) + softplus(2(s - log c_sigma)) + (alpha + 1/2) softplus(-2r) + (beta + 1/2) softplus(2r)
           + 1/2 q w delta_0^2 + sum_{t>=1} [1/2 w e_t^2 + s] + sum_{t>=0} 1/2 [h_t + y_t^2 e^{-h_t}]
         dU/dmu  = 2 mu/(c_mu^2 + mu^2) - q w delta_0 - (1 - phi) w S1,   S1 = sum_{t>=1} e_t
         dU/ds   = 2 sigmoid(2(s - log c_sigma)) - q w delta_0^2 - w S2 + (T - 1),   S2 = sum e_t^2
         dU/dr   = 2(beta + 1/2) sigmoid(2r) - 2(alpha + 1/2) sigmoid(-2r) - phi q w delta_0^2 - q w S3,   S3 = sum e_t a_t
         dU/dh_t = 1/2 - 1/2 y_t^2 e^{-h_t} + [t = 0] q w delta_0 + [t >= 1] w e_t - [t + 1 < T] phi w e_{t+1}
       n_components = T (T >= 1 and T = d - 3);  a -> y (T,) fp32, device memory;  b -> (alpha, beta), two fp32 in device
       memory;  a_scalar = c_mu > 0, b_scalar = c_sigma > 0 (finite).  A NULL a or b, T out of range, or a scale not
       positive and finite is NFMC_EINVAL.  A proposal whose U or gradient overflows fp32 (w, e^{-h_t}) has a non-finite
       log ratio: rejected and counted like every other kind's.  Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32
       (general kernels, with or without a jump tail, device warmup tuning included), by the register-layout kernels of
       nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32
       with conditioners of at most 32 units).  NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the
       fit kernels, the Philox4x32-7 stream and the NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_SPARSE_LOGISTIC_REGRESSION = 7,
    /* Sparse logistic regression with a hierarchical shrinkage prior (the German-credit model of the Inference Gym) over
       d = 2 D + 1 coordinates: x_{2j} = w_j, x_{2j+1} = l_j = log lambda_j (j = 0 .. D-1), x_{2D} = s = log tau;
       tau ~ Gamma(a, b), lambda_j ~ Gamma(a, b) (shape a, rate b), w_j ~ N(0, 1), beta_j = tau lambda_j w_j,
       y_i ~ Bernoulli(sigmoid(z_i)), z = X beta.  With r_i = sigmoid(z_i) - y_i and g = X^T r, the Jacobians of the two
       logs included and constants dropped:
         U = sum_i [softplus(z_i) - y_i z_i] + 1/2 sum_j w_j^2 + sum_j (b e^{l_j} - a l_j) + (b e^s - a s)
         dU/dw_j = e^{s + l_j} g_j + w_j,   dU/dl_j = beta_j g_j + b e^{l_j} - a,   dU/ds = sum_j beta_j g_j + b e^s - a
       a -> X (N, D) fp32 row-major, device memory, 16-byte aligned;  b -> y (N,) fp32, values 0 or 1, device memory;
       n_components = N;  a_scalar = a > 0, b_scalar = b > 0 (finite).  An even d or d < 3, N < 1, a NULL or misaligned
       pointer, or a scale not positive and finite is NFMC_EINVAL.  No cap on N (each evaluation streams X through an LDS
       tile of 16 KB plus the tile's labels; a flow image that leaves no room for it gets NFMC_EUNSUPPORTED).  A proposal
       whose U or gradient overflows fp32 (e^{s + l_j}, e^{l_j}, e^s, z) has a non-finite log ratio: rejected and counted
       like every other kind's.  Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a
       jump tail, device warmup tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU
       NeuTra kernels (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_LATTICE_PHI4 = 8,
    /* phi^4 scalar field on a lattice of H rows of W sites, flattened row-major (d = H W; H = 1 is the 1-D lattice,
       which has no second axis).  Every site c has two neighbours c' per axis; a periodic axis wraps round (so an axis
       of length 2 counts its bond twice), and with the zero boundary the field is 0 past the ends of an axis:
         U = sum_c [1/2 m2 x_c^2 + 1/4 lam x_c^4] + 1/2 kappa sum_bonds (x_c' - x_c)^2   (constants dropped)
         dU/dx_c = m2 x_c + lam x_c^3 + kappa sum_{c'} (x_c - x_c')
       n_components = W;  a -> (m2, lam, kappa, boundary), four fp32 in device memory, boundary 0 = periodic, 1 = zero
       (any other value reads as zero);  b, a_scalar and b_scalar unused.  One row with the zero boundary on BOTH axes
       (a 2-D lattice of shape (1, W)) is the 1-D lattice with m2 + 2 kappa in place of m2: the caller folds it.  A NULL
       a, W < 1 or d % W != 0 is NFMC_EINVAL; W % 4 != 0 is NFMC_EUNSUPPORTED (the kernels need every lattice row to start
       on a 16-byte register quad).  The kernels exchange neighbours through a wave-private LDS block of 16 + 1024 CPL
       bytes (CPL = 4, 8 or 16 coordinates per lane; a flow image that leaves no room for it gets NFMC_EUNSUPPORTED).
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_ITEM_RESPONSE = 9,
    /* One-parameter item-response theory (the synthetic IRT model of the Inference Gym): S students answer Q questions,
       d = S + Q + 1 coordinates x = [alpha_0 .. alpha_{S-1} | beta_0 .. beta_{Q-1} | mu] (abilities, difficulties, mean
       ability);  mu ~ N(m0, 1/p_mu), alpha_s ~ N(0, 1/p_a), beta_q ~ N(0, 1/p_b), y_sq ~ Bernoulli(sigmoid(l_sq)) for
       every observed pair, l_sq = mu + alpha_s - beta_q.  With r_sq = sigmoid(l_sq) - y_sq (0 where unobserved):
         U = 1/2 p_mu (mu - m0)^2 + 1/2 p_a sum_s alpha_s^2 + 1/2 p_b sum_q beta_q^2
             + sum_{observed} [softplus(l_sq) - y_sq l_sq]                                   (constants dropped)
         dU/dalpha_s = p_a alpha_s + sum_q r_sq,  dU/dbeta_q = p_b beta_q - sum_s r_sq,  dU/dmu = p_mu (mu - m0) + sum r_sq
       n_components = S (Q = d - 1 - S);  b -> (m0, p_mu, p_a, p_b), four fp32 in device memory;  a -> the responses in
       device memory, 16-byte aligned: ONE block of Q rows of SA = 4 ceil(S / 4) fp32, question-major,
       a[q * SA + s] = 1 or 0 for the observed answer of student s to question q and any negative value (-1) for a
       missing one and for the padding s >= S.  (The kernels evaluate each pair once, in a pass over the questions, so
       there is no second, student-major block.)  a_scalar and b_scalar unused.  A NULL a or b, S < 1 or S > d - 2 is
       NFMC_EINVAL; a misaligned a is NFMC_EALIGN.  No cap on S Q; d <= 1024.  The kernels keep one LDS row of d padded
       to DP = CPL LPC floats, plus 4, per chain of a workgroup: (256 / LPC) (DP + 4) fp32 (a flow image that leaves no room
       for it gets NFMC_EUNSUPPORTED).
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_VARYING_EFFECTS = 10,
    /* Gaussian regression with group-level (varying) effects: the radon models and eight schools.  Observation i has a
       response y_i, an optional covariate x_i and a group g_i in 0 .. C-1:  y_i ~ N(a[g_i] + b[g_i] x_i, sigma_i^2).
       Intercept side: varying (a_c ~ N(mu_a, sigma_a^2), mu_a ~ N(0, m^2), sigma_a ~ HalfNormal(h)) or shared (one
       a ~ N(0, m^2)); slope side: varying, shared or none (b = 0); at least one side varies.  Noise: unknown
       (sigma_i = sigma_y ~ HalfNormal(h)) or known per observation.  Scales are sampled as logs s = log sigma (Jacobian
       included).  Centered: the group coordinates are a_c, b_c; non-centered: t_c ~ N(0, 1) with a_c = mu_a + e^{s_a} t_c.
       Coordinates: the group block, [a_0, b_0, a_1, b_1, ...] (2 C, interleaved) when both sides vary and [v_0 .. v_{C-1}]
       when one does, then the globals that exist, in this order: (mu_a, s_a) or a; (mu_b, s_b) or b or nothing; s_y if the
       noise is unknown.  d = 2 C + 5 at most.
       The likelihood enters through six sufficient statistics per group, weights omega_i = 1 / sigma_i^2 (1 when the
       noise is unknown): n_c = sum omega, the weighted means xbar_c, ybar_c and the CENTRED weighted sums Sxx_c, Sxy_c,
       Syy_c.  With P = 1 / m^2, Hh = 1 / h^2, w_y = e^{-2 s_y} (1 when known), e_c = ybar_c - a_c - b_c xbar_c:
         Q_c  = n_c e_c^2 + Syy_c - 2 b_c Sxy_c + b_c^2 Sxx_c
         gA_c = -w_y n_c e_c,   gB_c = w_y (-n_c e_c xbar_c - Sxy_c + b_c Sxx_c)
         U = 1/2 w_y sum_c Q_c  [+ N s_y + 1/2 Hh e^{2 s_y} - s_y  when the noise is unknown]
             + per varying side (mu, s), r_c = v_c - mu, w = e^{-2 s}:
                 centered      C s + 1/2 w sum r_c^2 + 1/2 P mu^2 + 1/2 Hh e^{2 s} - s
                 non-centered  1/2 sum t_c^2 + 1/2 P mu^2 + 1/2 Hh e^{2 s} - s
             + per shared side 1/2 P v^2                                                     (constants dropped)
         dU/ds_y = N - w_y sum Q_c + Hh e^{2 s_y} - 1
         centered:      dU/dv_c = gV_c + w r_c,      dU/dmu = P mu - w sum r_c,  dU/ds = C - w sum r_c^2 + Hh e^{2 s} - 1
         non-centered:  dU/dt_c = e^{s} gV_c + t_c,  dU/dmu = P mu + sum gV_c,   dU/ds = e^{s} sum gV_c t_c + Hh e^{2 s} - 1
         shared:        dU/dv = P v + sum gV_c
       n_components = C;  a -> the group table in device memory, 16-byte aligned, C rows of 8 fp32
       (n, xbar, ybar, Sxx, Sxy, Syy, 0, 0);  b -> (P, Hh), two fp32 in device memory;  a_scalar = the layout code, an
       integer-valued float mode_a + 4 mode_b + 16 known_noise + 32 non_centered with mode 0 = none, 1 = shared,
       2 = varying (mode_a is 1 or 2, mode_b 0, 1 or 2, one of them 2);  b_scalar = N, the number of observations, when
       the noise is unknown (unused otherwise).  A NULL a or b, C < 1, a code that is none of the 16 valid ones, d other
       than group block + globals of the code, or N not positive and finite with unknown noise is NFMC_EINVAL; a
       misaligned a is NFMC_EALIGN.  d <= 1024.  No LDS block: every lane reads the table rows of its own groups (two
       16-byte loads per group and evaluation).  e^{-2 s}, e^{2 s} and e^{s} overflow fp32 far in the tails: U is then inf
       or NaN and the samplers reject the state and count its log ratio as non-finite.
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_PARTICLES = 11,
    /* Interacting particles in a harmonic trap (many-particle Boltzmann density): P particles in D = 1, 2 or 3
       dimensions, coordinates particle-major x = [r_0 | r_1 | .. | r_{P-1}], d = P D.  With r_ij = |r_i - r_j|:
         U = beta [ k/2 sum_i |r_i|^2 + sum_{i<j} phi(r_ij) ]                                  (constants dropped)
         dU/dr_i = beta [ k r_i + sum_{j != i} (phi'(r_ij) / r_ij) (r_i - r_j) ]
       pair code 0, Lennard-Jones:  phi(r) = eps [ (r_m / r)^12 - 2 (r_m / r)^6 ], minimum -eps at r_m, evaluated from
       s = r^2 alone (no square root);  pair code 1, double well:  phi(r) = a (r - r0) + b (r - r0)^2 + c (r - r0)^4.
       n_components = P;  a -> one 16-byte aligned block of 8 fp32 in device memory:
         (pair code, D, beta k, q0, q1, q2, q3, 0)  with  (q0 .. q3) = (beta eps, r_m^2, 0, 0)  for Lennard-Jones and
         (beta a, beta b, beta c, r0)  for the double well;  b, a_scalar, b_scalar unused.  beta = 1 / temperature is
       folded in by the caller (ParticleSystem does it in fp64).  The check sees host values only: D is d / P, and the
       block's D is not read.  A NULL a, P < 2, or d that is not P D with D in 1 .. 3 is NFMC_EINVAL; a misaligned a is
       NFMC_EALIGN; d > 1024 is NFMC_EUNSUPPORTED.  Two coincident particles (s = 0): Lennard-Jones gives U = inf and a
       NaN force, the samplers reject the state and count its log ratio as non-finite; the double well contributes
       phi(0) and zero force.  k > 0 is the caller's business: the pair terms are translation invariant, so without
       the trap the density is improper.  Cost: P (P - 1) pair evaluations per chain and gradient (every unordered
       pair twice, once per owner: no atomics, bitwise repeatable).  LDS: one row of DP + 4 floats per chain.
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_LATENT_GAUSSIAN = 12,
    /* Latent Gaussian model: a Gaussian (process) prior f ~ N(m, K) on a latent vector of d coordinates, K = L L^T
       (L the lower-triangular Cholesky factor), Lambda = K^-1, and a non-Gaussian likelihood on each coordinate with
       an observation y_j and a weight w_j >= 0 (w_j = 0: not observed, the coordinate adds exactly 0 to U and grad U).
       The log-Gaussian Cox process, GP classification and robust GP regression.  Negative log-likelihood l_j(f),
       constants dropped, by likelihood code:
         0 Poisson, log link      l = w e^f - y f                               l' = w e^f - y            (w: exposure)
         1 binomial, logit link   l = w softplus(f) - y f                       l' = w sigmoid(f) - y     (w: trials)
         2 Student-t noise        l = w (nu+1)/2 log1p((y-f)^2 / (nu s^2))      l' = -w (nu+1)(y-f) / (nu s^2 + (y-f)^2)
       Two parameterisations of the same posterior:
         centred   x = f:             U = 1/2 (x-m)^T Lambda (x-m) + sum_j l_j(x_j),   dU/dx = Lambda (x-m) + l'(x)
         whitened  x = z, f = m + L z:  U = 1/2 |z|^2 + sum_j l_j(f_j),                  dU/dz = z + L^T l'(f)
       n_components = d;  a_scalar = likelihood code + 4 [whitened], an integer-valued float in {0, 1, 2, 4, 5, 6};
       b_scalar unused.  a -> the matrix block, fp32 row-major in device memory, 16-byte aligned: Lambda (d, d) when
       centred; when whitened L^T (d, d) and behind it L (d, d), 2 d^2 floats, the upper triangle of L (lower of L^T)
       exact zeros (the NeuTra kernels do not read it).  b -> the table, fp32 in device memory, 16-byte aligned, with
       d4 = 4 ceil(d / 4):  8 floats ((nu+1)/2, 1/(nu s^2), nu s^2, nu+1, 0, 0, 0, 0), zeros for codes 0 and 1, then the
       rows m, y, w of d4 floats each, zero past d.  A NULL a or b, n_components != d or an invalid code is NFMC_EINVAL;
       a misaligned a or b is NFMC_EALIGN; d > 1024 is NFMC_EUNSUPPORTED.  Nothing is clamped: a Poisson rate that
       overflows fp32 gives U = inf or a NaN log ratio, the samplers reject the proposal and count it as non-finite, and
       the chain's state stays finite.  Cost: d^2 FMAs per chain and evaluation when centred, 2 d^2 when whitened (two
       matrix-vector products streamed through one LDS tile of 16 KB), no atomics, bitwise repeatable.
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_LATENT_GMRF = 13,
    /* Latent Gaussian Markov random field: n sites with a sparse, symmetric, positive semi-definite structure matrix R
       of rank rho (random-walk smoothers, ICAR / Besag models on an adjacency graph, the SPDE-Matern field on a grid),
       prior x | tau ~ tau^(rho/2) exp(-tau/2 r^T R r), r = x - m, and on every site one of the likelihoods of
       NFMC_POT_LATENT_GAUSSIAN (same codes, same l and l', observation y_j, weight w_j >= 0, w_j = 0: not observed).
       Three modes; q = v^T R v for the vector v named with the mode:
         fixed tau  (d = n, v = r; the caller folds tau into the values of R)
                    U = 1/2 q + sum_j l_j(x_j),                                  dU/dx = R r + l'(x)
         centred    (d = n + 1, v = r; coordinate n is s = log tau, tau ~ Gamma(a, b) (shape, rate), Jacobian included)
                    U = 1/2 e^s q - (rho/2) s + sum_j l_j(x_j) + b e^s - a s,    dU/dx_j = e^s (R r)_j + l'_j,
                    dU/ds = 1/2 e^s q - rho/2 + b e^s - a
         scaled     (d = n + 1, v = u; the coordinates are u with f = m + e^(-s/2) u, and s)
                    U = 1/2 q + sum_j l_j(f_j) + b e^s - a s + ((n - rho)/2) s,  dU/du_j = (R u)_j + e^(-s/2) l'_j(f_j),
                    dU/ds = -1/2 e^(-s/2) sum_j u_j l'_j(f_j) + b e^s - a + (n - rho)/2
       n_components = W, the ELL width (the largest number of stored entries in a row of R), 1 <= W <= 32;
       a_scalar = likelihood code + 4 [tau unknown] + 8 [scaled], an integer-valued float in {0, 1, 2, 4, 5, 6, 12, 13, 14};
       b_scalar unused.  With n4 = 4 ceil(n / 4):  a -> the ELL block, fp32 in device memory, 16-byte aligned, slot-major:
       W rows of n4 values, a[k n4 + j] = the k-th stored entry of row j of R, then W rows of n4 column indices as
       integer-valued floats; a padding slot (and every slot of a row past n) has value 0 and its own row as index.
       b -> the table, fp32 in device memory, 16-byte aligned: 8 floats ((nu+1)/2, 1/(nu s^2), nu s^2, nu+1, a, b, rho/2,
       (n - rho)/2), then the rows m, y, w of n4 floats each, zero past n.  A NULL a or b, W < 1, an invalid code, d < 1
       (d < 2 with tau unknown) is NFMC_EINVAL; a misaligned a or b is NFMC_EALIGN; W > 32 or d > 1024 is
       NFMC_EUNSUPPORTED.  The check sees host values only; every kernel clamps every gathered column index into the
       sites 0 .. n - 1 of the chain, so a bad table gives wrong numbers and never a read outside them.  Nothing else is clamped:
       an overflowing e^s or Poisson rate gives a non-finite U or log ratio, the samplers reject the proposal and count
       it as non-finite, and the chain's state stays finite.  Cost: W n FMAs and gathers per chain and evaluation, no
       matrix stream, no atomics, bitwise repeatable.
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
    NFMC_POT_DIFFUSION_BRIDGE = 14
    /* Diffusion bridge: the latent path of a stochastic differential equation dX = f(X) dt + sigma dW discretised by
       Euler-Maruyama, T >= 2 time steps with a state X_t in R^m (m = 1, 2 or 3) and the step dt, partially observed:
         X_0 ~ N(mu0, s0^2 I),   X_t | X_{t-1} ~ N(X_{t-1} + dt f(X_{t-1}), sigma^2 dt I) (t >= 1),
         y_{t,c} ~ N(X_{t,c}, tau^2) wherever w_{t,c} != 0 (the caller writes w = 1; w = 0: not observed),
       and, when the scales are unknown, p = log sigma and q = log tau with p, q ~ N(l, c^2) independently (a
       LogNormal(l, c) prior on sigma and on tau).  Coordinates time-major: x[t m + c] = X_{t,c}, then x[T m] = p and
       x[T m + 1] = q when the scales are unknown: d = T m or T m + 2.  With e_t = X_t - X_{t-1} - dt f(X_{t-1}) (t >= 1),
       om = 1 / (sigma^2 dt), rho = 1 / tau^2, S_e = sum_{t>=1} |e_t|^2, S_v = sum w (X - y)^2, N_o = sum w, constants dropped:
         U       = 1/2 |X_0 - mu0|^2 / s0^2 + 1/2 om S_e + 1/2 rho S_v
                   [ + (T-1) m p + N_o q + (p - l)^2 / (2 c^2) + (q - l)^2 / (2 c^2) ]
         dU/dX_t = [t = 0] (X_0 - mu0) / s0^2 + [t >= 1] om e_t - [t < T-1] om (I + dt J_f(X_t))^T e_{t+1}
                   + rho w_t o (X_t - y_t)
         dU/dp   = -om S_e + (T-1) m + (p - l) / c^2,      dU/dq = -rho S_v + N_o + (q - l) / c^2
       Drift codes, with the drift parameters (p0, p1, p2, p3) of the header:
         0 cubic (any m, componentwise)  f_c = p0 x_c - p1 x_c^3,  J = diag(p0 - 3 p1 x_c^2)   (p0 = alpha, p1 = beta:
                                         0, 0 Brownian motion; alpha < 0, 0 Ornstein-Uhlenbeck; alpha = beta > 0 double well)
         1 fitzhugh_nagumo (m = 2)       f = (x0 - x0^3/3 - x1 + I, eps (x0 + a - b x1)),  J = [[1 - x0^2, -1], [eps, -eps b]]
                                         (p0, p1, p2, p3) = (a, b, eps, I)
         2 lorenz63 (m = 3)              f = (s (x1 - x0), x0 (r - x2) - x1, x0 x1 - beta x2),
                                         J = [[-s, s, 0], [r - x2, -1, -x0], [x1, x0, -beta]],  (p0, p1, p2) = (s, r, beta)
       n_components = T; a_scalar = drift code + 4 [scales unknown] + 8 (m - 1), an integer-valued float; b_scalar unused.
       a -> the header, 16 fp32 in device memory, 16-byte aligned: (dt, sigma, tau, mu0, 1/s0^2, l, 1/c^2, N_o, (T-1) m,
       p0, p1, p2, p3, 0, 0, 0); with unknown scales sigma and tau are ignored (any positive finite values).
       b -> fp32 in device memory, 16-byte aligned: the rows y and w of n4 = 4 ceil(T m / 4) floats each, time-major like
       the coordinates, zero past T m.  A NULL a or b, T < 2, an invalid code, an m that does not fit the drift
       (fitzhugh_nagumo m = 2, lorenz63 m = 3) or d != T m + 2 [scales unknown] is NFMC_EINVAL; a misaligned a or b is
       NFMC_EALIGN; d > 1024 is NFMC_EUNSUPPORTED.  The check sees host values only.  Nothing is clamped: an overflowing
       e^(-2p) or cubic term gives a non-finite U or log ratio, the samplers reject the proposal and count it as
       non-finite, and the chain's state stays finite.  Cost per evaluation: one 16-byte store of each register
       quad into the chain's own exchange row, then per register quad one window of 6, 8 or 12 reads of that row (m = 1,
       2, 3) and 5, 3 or 3 drift evaluations, shared by the quad's four coordinates; two all-reduces per chain, no
       atomics, bitwise repeatable.
       Served by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 (general kernels, with or without a jump tail, device warmup
       tuning included), by the register-layout kernels of nfmc_flow_mh_steps_f32 and by the VALU NeuTra kernels
       (nfmc_neutra_potential_grad_f32 / nfmc_neutra_hmc_steps_f32 with conditioners of at most 32 units).
       NFMC_EUNSUPPORTED from nfmc_imh_parallel_f32, nfmc_dlmc_step_f32, the fit kernels, the Philox4x32-7 stream and the
       NeuTra matrix-core kernels (conditioners wider than 32). */
};

typedef struct {
    int32_t kind;
    int32_t n_components; /* NFMC_POT_GAUSSIAN_MIXTURE: K; NFMC_POT_LOGISTIC_REGRESSION: N; NFMC_POT_GAUSSIAN_FULL: d;
                             NFMC_POT_ROSENBROCK: block length; NFMC_POT_STOCHASTIC_VOLATILITY: T = d - 3;
                             NFMC_POT_SPARSE_LOGISTIC_REGRESSION: N; NFMC_POT_LATTICE_PHI4: W (sites per lattice row);
                             NFMC_POT_ITEM_RESPONSE: S (students); NFMC_POT_VARYING_EFFECTS: C (groups);
                             NFMC_POT_PARTICLES: P (particles); NFMC_POT_LATENT_GAUSSIAN: d;
                             NFMC_POT_LATENT_GMRF: W (ELL width);
                             NFMC_POT_DIFFUSION_BRIDGE: T (time steps);
                             0 for the other kinds (was `reserved`, same layout) */
    const float* a; /* (d,) or NULL -> a_scalar */
    const float* b; /* (d,) or NULL -> b_scalar */
    float a_scalar;
    float b_scalar;
} NfmcPotential;

typedef struct {
    uint64_t seed;
    uint64_t chain_offset;        /* global id of row 0 (chains sharded over GPUs keep global ids) */
    uint32_t step0;               /* transition index of the first step of this call */
    uint32_t rounds;              /* 0 or 10: Philox4x32-10 (the library's stream).  7: Philox4x32-7, an opt-in stream with
                                     30 % fewer generator instructions (the smallest round count Random123 reports as
                                     passing BigCrush); supported by nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 on their
                                     exact-fit quadratic kernels (no jump tail), by the register-layout kernels of
                                     nfmc_flow_mh_steps_f32 without diagnostics, and by nfmc_philox_*; elsewhere
                                     NFMC_EUNSUPPORTED.  oracle/philox.py carries the same parameter. */
    const float* replay_normals;  /* NULL -> native Philox; else (n_steps, n, d) */
    const float* replay_uniforms; /* NULL -> native Philox; else (n_steps, n)     */
} NfmcRng;

/* Streaming statistics, all ACCUMULATED (+=) by the kernels.  Replaces
 * `MCMCExpectation.update` for f = x, x^2 and the counters of `MCMCStatistics`
 * (nfmc/algorithms/sampling/base.py:75-95,126-161; mcmc/base.py:79-86). */
enum { NFMC_CNT_ACCEPTED = 0, NFMC_CNT_ATTEMPTED = 1, NFMC_CNT_NONFINITE = 2, NFMC_CNT_WORDS = 4 };

typedef struct {
    double* sum_x;                /* (d,)  += sum over steps and chains of x     (NULL: statistics off) */
    double* sum_x2;               /* (d,)  += ... of x^2 */
    unsigned long long* counters; /* (NFMC_CNT_WORDS,) */
    double* scratch;              /* per-workgroup partials, >= nfmc_stats_scratch_bytes(d) bytes */
    int64_t scratch_bytes;
    int32_t defer;                /* 0: every call folds its partials into sum_x / sum_x2 / counters before it
                                     returns control of the stream (one extra small kernel per call).
                                     1: the call only ADDS its per-workgroup partials to `scratch`, which the caller
                                     zeroed once; nfmc_stats_fold_f32 folds them later (one fold per sample() instead
                                     of one per launch).  Supported by K1, K2, the flow-MH kernels and K6
                                     (nfmc_mh_accept_select_f32); the NeuTra entry points and K7 alone
                                     (nfmc_moments_update_f32) return NFMC_EUNSUPPORTED.  A defer = 0 call WRITES the
                                     slabs it uses and folds only those: partials still pending in `scratch` must be
                                     folded (nfmc_stats_fold_f32) before a defer = 0 call on the same scratch. */
    int32_t tail_slot;            /* defer = 1 only: 0 = accepted / non-finite counts are MCMC counts, 2 = this call
                                     is a jump (they go to the jump counters at fold time) */
} NfmcStats;

int64_t nfmc_stats_scratch_bytes(int32_t d);

/* Fold the deferred partials in stats->scratch into sum_x, sum_x2 and counters (+= ; ATTEMPTED += attempted), the
 * jump slots into jump_counters (may be NULL; ATTEMPTED += jump_attempted), and zero the scratch again.  The
 * fold order is fixed (run-to-run bitwise equal).  d = flattened event size the partials were produced with. */
int nfmc_stats_fold_f32(const NfmcStats* stats, int32_t d, uint64_t attempted, unsigned long long* jump_counters,
                        uint64_t jump_attempted, nfmc_stream_t stream);

/* ---- RealNVP (the build's spec: DESIGN.md "RealNVP spec"; stands in for torchflows.RealNVP,
 * call sites nfmc/util.py:280-281). */
typedef struct {
    int32_t d;                /* flattened event size */
    int32_t n_coupling;       /* number of (ReversePermutation, AffineCoupling) pairs */
    int32_t n_hidden;         /* H */
    int32_t n_hidden_layers;  /* conditioner hidden layers (>= 1) */
    float min_scale;          /* m in alpha = exp(u/2 + log(1-m)) + m  (1 = additive coupling, 'nice') */
    int32_t n_bins;           /* 0: affine coupling.  8: rational-quadratic spline coupling ('c-rqnsf') with 8 bins on
                                 [-spline_bound, spline_bound], identity outside; the last conditioner layer then has
                                 (3*n_bins - 1) * d_b outputs, target-major: [t*(3K-1) + (K widths | K heights | K-1
                                 derivatives)] (spec: DESIGN.md section 4).  Spline flows run on the one-chain-per-lane
                                 kernels with n_hidden <= 32 (forward, inverse, flow-MH, and the NeuTra reverse sweep:
                                 hand-written adjoints of the spline, csrc/flow_device.hpp rqs_inverse_backward). */
    const float* ea0_log_scale; /* (d,) first ElementwiseAffine */
    const float* ea0_shift;
    const float* ea1_log_scale; /* (d,) last ElementwiseAffine */
    const float* ea1_shift;
    const float* weights;     /* per coupling layer (logical, un-permuted coordinates), HP = padded H:
                                 W1T (d_a, HP) | b1 (HP) | [WhT (HP_in, HP_out) | bh (HP)] x (n_hidden_layers-1)
                                 | W3 (2 d_b, HP) | b3 (2 d_b);  W1T/WhT are the TRANSPOSES of the PyTorch Linear
                                 weights (in, out), W3 keeps (out, in); rows [0, d_b) of W3 give u_alpha, rows
                                 [d_b, 2 d_b) give u_beta; d_a = d/2, d_b = d - d_a */
    int64_t layer_stride;     /* floats between consecutive coupling layers */
    float spline_bound;       /* B (n_bins > 0) */
    int32_t reserved;
    float* scratch;           /* workspace of the streamed matrix-core kernels (n_hidden 33..128 at d = 32 .. 512 a multiple of
                                 32 other than 64 / 128): >= nfmc_flow_scratch_bytes(flow, n, ...) bytes, 16-byte aligned, private
                                 to one stream at a time; NULL / 0 elsewhere.  The library never allocates: a call that needs it
                                 and does not find it returns NFMC_ESCRATCH */
    int64_t scratch_bytes;
} NfmcRealNVP;

/* Bytes of NfmcRealNVP.scratch that nfmc_realnvp_forward_f32 / nfmc_realnvp_inverse_f32 (with_gradient = 0) or
 * nfmc_neutra_potential_grad_f32 (with_gradient = 1) need for n rows: the state (and gradient) of the resident workgroups'
 * chains stream through it, one private row per lane group of a workgroup SLOT -- at most 256 x 128 rows of d floats (x 2
 * with the gradient) whatever n.  0 for every shape that runs register- or LDS-resident. */
int64_t nfmc_flow_scratch_bytes(const NfmcRealNVP* flow, int64_t n, int32_t with_gradient);

/* HP: n_hidden padded to the kernels' width (4, 8, 16, 32 on the VALU path; 64 or 128 on the matrix-core path,
 * whose blob also carries every matrix in both orientations: csrc/mfma_device.hpp); 0 = unsupported. */
int32_t nfmc_realnvp_padded_hidden(int32_t n_hidden);
int64_t nfmc_realnvp_layer_floats(int32_t d, int32_t n_hidden, int32_t n_hidden_layers);
/* the same for any coupling kind (n_bins as in NfmcRealNVP; 0 = affine) */
int64_t nfmc_coupling_layer_floats(int32_t d, int32_t n_hidden, int32_t n_hidden_layers, int32_t n_bins);

/* ---- Kept states.  Replaces `MCMCSamples.add` (nfmc/algorithms/sampling/base.py:234-263): the state after a
 * transition is kept iff the transition's global index is a multiple of `thinning`, and only the newest `max_samples`
 * kept states survive.  Both decisions are made BEFORE the launch, so a kernel writes only rows that will still be
 * there at the end, into a store of `ring_rows` rows of n*d floats that is never larger than max_samples rows
 * (the reference slices its host-side list after the fact).  The store is a ring: the j-th kept state of a run goes to
 * row j mod ring_rows; the caller reads it back in order from the oldest surviving row. */
typedef struct {
    float* base;        /* NULL: keep nothing */
    int32_t stride;     /* thinning: every stride-th transition is kept (>= 1) */
    int32_t countdown;  /* transitions of THIS call to skip before its first kept one: (-seen) mod stride, where seen =
                           transitions offered to the store so far */
    int32_t ring_rows;  /* rows of the store (>= 1); kept rows wrap around */
    int32_t row;        /* ring row of this call's first kept transition: ceil(seen / stride) mod ring_rows */
} NfmcSampleStore;

/* ---- Warmup tuning on the device.  Replaces `MetropolisSampler.update_kernel` + `DualAveraging.step`
 * (nfmc/algorithms/sampling/mcmc/base.py:142-161, tuning.py:15-41): after the transitions of a call, the controller
 *     m_j <- beta var_j + (1 - beta) m_j            var_j = unbiased variance of coordinate j over the call's states
 *     err = target - accepted / attempted;  S += err;  log h_raw = anchor - S / (sqrt(t) gamma);
 *     w = t^-kappa;  log h-bar <- w log h_raw + (1 - w) log h-bar;  t += 1;  h = exp(log h-bar)
 * runs inside the statistics fold of the call (its last workgroup), on state that lives in device memory: the next call
 * reads its step size and mass diagonal from there, so a warmup is a stream of launches without one host round trip.
 * One transition per call reproduces the reference update for update; n_steps = K updates once per K transitions with
 * the statistics pooled over them.  `state` words (fp64): */
enum {
    NFMC_TUNE_STEP_SIZE = 0,   /* h: read by the sampler kernel, rewritten by the controller */
    NFMC_TUNE_LOG_SMOOTH = 1,  /* log h-bar */
    NFMC_TUNE_ERROR_SUM = 2,   /* S */
    NFMC_TUNE_ITERATION = 3,   /* t */
    NFMC_TUNE_ANCHOR = 4,      /* log(10 h0) */
    NFMC_TUNE_LOG_RAW = 5,     /* log h_raw (output) */
    NFMC_TUNE_TARGET = 6,      /* target acceptance rate (0.651) */
    NFMC_TUNE_KAPPA = 7,
    NFMC_TUNE_GAMMA = 8,
    NFMC_TUNE_IMD_ADJUSTMENT = 9, /* beta */
    NFMC_TUNE_TICKET = 10,     /* internal: workgroup counter of the fold (zero between calls) */
    NFMC_TUNE_WORDS = 12       /* followed by 2 * padded_d + 4 words of column totals, then padded_d words of the
                                  per-coordinate shift c: nfmc_tune_state_doubles(d) in all.  Tuning launches sum x - c and
                                  (x - c)^2 (fp32 sums of x and x^2 cancel for chains far from the origin relative to
                                  their spread); the controller un-shifts them in fp64 into NfmcStats and sets c to the
                                  update's mean.  The caller initialises c (the column means of x0; zeros are valid) */
};
typedef struct {
    double* state;             /* NULL: no tuning (step_size / inv_mass_diag of the call are used as given) */
    float* inv_mass_diag;      /* (d,) device, updated in place when tune_inv_mass_diag; must be the call's inv_mass_diag */
    int32_t tune_step_size;
    int32_t tune_inv_mass_diag;
    int32_t every;             /* transitions per controller update.  0 or >= n_steps: one update after the call's n_steps
                                  transitions.  Otherwise the call enqueues ceil(n_steps / every) kernel + controller
                                  pairs itself (noise, masks and the sample store advance between them), so a whole
                                  warmup is ONE call: no host work between updates */
    int32_t trajectory;        /* nfmc_hmc_steps_f32 only (was `reserved`, same layout): NFMC_TRAJECTORY_*.  Not 0: `state`
                                  is followed by a trajectory block (below), and adjust must be 1 */
} NfmcTune;
int64_t nfmc_tune_state_doubles(int32_t d);

/* ---- Trajectory length of the hmc sampler, adapted in the same warmup (ChEES-HMC: Hoffman, Radul and Sountsov, AISTATS
 * 2021; all chains share one step size h and one length T).  Per transition with Philox step counter k = rng.step0 + s:
 *     u = (bitreverse32(k + 1) + 0.5) 2^-32            base-2 radical inverse: the jitter
 *     L = clamp(ceil(u T / h), 1, L_max)               leapfrog steps of EVERY chain of the transition (fp64, no
 *                                                      contraction: a host that repeats it gets the same integer)
 *     t = L h                                          realised length
 * and per chain, with c the lagged centre (the shift words of the tuning state), x the current state, q the proposal and
 * v = p * inv_mass_diag the velocity at the end of the trajectory:
 *     a0 = sum_i (x_i - c_i)^2,  a1 = sum_i (q_i - c_i)^2,  b = sum_i (q_i - c_i) v_i,  g = t (a1 - a0) b,
 *     alpha = min(1, exp(log ratio));  alpha = 0 where the log ratio, a0, a1 or b is not finite.
 * The controller update pools g-hat = sum(alpha g) / sum(alpha) over the chains and transitions of the update and runs
 * Adam with beta1 = 0 on log T (j: the update count from 1):
 *     v <- b2 v + (1 - b2) g-hat^2;   delta = lr g-hat / (sqrt(v / (1 - b2^j)) + 1e-8), clipped to +-clip
 *     log T <- clamp(log T + delta, log h, log(L_max h))      h: the step size the same update just set
 *     log T-bar <- w log T + (1 - w) log T-bar,   w = j^-0.75
 * An update with sum(alpha) == 0 (or a g-hat that is not finite) leaves all of that alone.  Deviation from the paper: both
 * centres are the lagged pooled mean c, not the batch means of the current states and of this transition's proposals (the
 * latter needs every chain's proposal before any chain's term: a grid-wide barrier per transition).
 * NfmcTune.trajectory: */
enum {
    NFMC_TRAJECTORY_OFF = 0,     /* n_leapfrog steps per transition; no trajectory block is read */
    NFMC_TRAJECTORY_ADAPT = 1,   /* jittered L, T adapted by every controller update */
    NFMC_TRAJECTORY_FROZEN = 2   /* jittered L at the block's T; only the leapfrog total is written */
};
/* The trajectory block: fp64 words at state + nfmc_tune_state_doubles(d), nfmc_tune_trajectory_doubles(history_rows) of
 * them, caller-allocated and caller-initialised (the library never allocates). */
enum {
    NFMC_TRAJ_LENGTH = 0,          /* T the next launch runs on = exp(log T) as the controller evaluated it (in) */
    NFMC_TRAJ_LOG_LENGTH = 1,      /* log T (in: log of the word above) */
    NFMC_TRAJ_LOG_AVERAGED = 2,    /* log T-bar (in: log T) */
    NFMC_TRAJ_V = 3,               /* second-moment estimate (in: 0) */
    NFMC_TRAJ_COUNT = 4,           /* j: updates applied (in: 0) */
    NFMC_TRAJ_LEARNING_RATE = 5,   /* lr (0.025) */
    NFMC_TRAJ_BETA2 = 6,           /* b2 (0.95) */
    NFMC_TRAJ_CLIP = 7,            /* clip (0.35) */
    NFMC_TRAJ_MAX_LEAPFROG = 8,    /* L_max (128) */
    NFMC_TRAJ_LEAPFROG_TOTAL = 9,  /* leapfrog steps per chain taken so far, all launches (in: 0) */
    NFMC_TRAJ_G_HAT = 10,          /* last update's g-hat (out) */
    NFMC_TRAJ_ALPHA_SUM = 11,      /* ... and its sum(alpha) (out) */
    NFMC_TRAJ_HISTORY_ROWS = 12,   /* capacity of the history below, in rows */
    NFMC_TRAJ_HISTORY_USED = 13,   /* NFMC_TRAJECTORY_ADAPT updates so far; rows beyond the capacity are not written (in: 0) */
    NFMC_TRAJ_WORDS = 16           /* followed by the history: one row per update */
};
/* A history row: T and h the update's transitions ran with, what they measured, and what the update left */
enum {
    NFMC_TRAJ_ROW_LENGTH = 0,
    NFMC_TRAJ_ROW_STEP_SIZE = 1,
    NFMC_TRAJ_ROW_G_HAT = 2,
    NFMC_TRAJ_ROW_ALPHA_SUM = 3,
    NFMC_TRAJ_ROW_LEAPFROGS = 4,       /* leapfrog steps per chain of the update's transitions */
    NFMC_TRAJ_ROW_LOG_LENGTH = 5,
    NFMC_TRAJ_ROW_V = 6,
    NFMC_TRAJ_ROW_LOG_AVERAGED = 7,
    NFMC_TRAJ_ROW_NEXT_STEP_SIZE = 8,  /* h the update set */
    NFMC_TRAJ_ROW_WORDS = 9
};
/* NFMC_TRAJ_WORDS + history_rows * NFMC_TRAJ_ROW_WORDS; 0 for history_rows < 0 */
int64_t nfmc_tune_trajectory_doubles(int32_t history_rows);

/* The register layout nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 run a call without a jump tail on, for event size d and
 * potential kind `pot_kind`: *cpl coordinates per lane, *lpc lanes per chain (a workgroup holds 256 / lpc chains).  Host
 * arithmetic only, no device call.  NFMC_EINVAL for a NULL pointer or d <= 0, NFMC_ESHAPE for d > 1024,
 * NFMC_EUNSUPPORTED for an unknown kind. */
int nfmc_sampler_layout(int32_t d, int32_t pot_kind, int32_t* cpl, int32_t* lpc);

/* Optional tail of a sampler call: after the n_steps inner transitions, ONE flow-proposal Metropolis jump
 * (jump.py:205-243: flow.sample, flow.log_prob, 2 target calls, log u < log alpha, masked update) on the
 * same registers, as transition rng.step0 + n_steps.  With a tail, `samples` is offered n_steps + 1 states and the
 * moments include the post-jump state.  Narrow conditioners only (n_hidden <= 8, d <= 512); otherwise the
 * call returns NFMC_EUNSUPPORTED and the caller issues nfmc_flow_mh_steps_f32 separately. */
typedef struct {
    NfmcRealNVP flow;
    int32_t adjusted;             /* 0: accept every proposal (adjusted_jumps=False) */
    int32_t reserved;
    unsigned long long* counters; /* (NFMC_CNT_WORDS,) jump counters: accepted / attempted / nonfinite */
    const float* replay_latent;   /* NULL -> native stream 2; else (n, d) latents */
    const float* replay_uniform;  /* NULL -> native stream 3; else (n,) */
    uint8_t* mask_out;            /* NULL or (n,) */
    float* log_ratio_out;         /* NULL or (n,) */
} NfmcJumpTail;

/* ---- K1 (+K6, K7): n_steps fused Langevin transitions.
 * Replaces `Langevin.propose` + the masked update + counters + moments of `MCMCSampler.sample`
 * (langevin.py:61-122; mcmc/base.py:74-90). */
typedef struct {
    float* x;                   /* (n, d) in/out */
    int64_t n;
    int32_t d;
    int32_t n_steps;            /* 1..NFMC_MAX_STEPS_PER_CALL */
    float step_size;
    int32_t adjust;             /* bit 0: Metropolis test (1 = MALA, 0 = ULA); bit 1: random-walk proposal
                                   x' = x + inv_mass_diag * eps instead of the Langevin drift (mh.py:51-60:
                                   3 = MH, 2 = RandomWalk) */
    const float* inv_mass_diag; /* (d,) or NULL = ones (mcmc/base.py:113-116) */
    NfmcPotential pot;
    NfmcRng rng;
    NfmcStats stats;
    NfmcSampleStore samples;    /* state after every step, thinned / windowed as described above (MCMCSamples.add) */
    uint8_t* masks_out;         /* NULL or (n_steps, n) accept masks (tests / split path) */
    float* log_ratio_out;       /* NULL or (n_steps, n) */
    const NfmcJumpTail* jump;   /* NULL or a jump to run after the inner transitions (host pointer) */
    NfmcTune tune;              /* device-side tuning (warmup); needs stats with defer = 0 and no jump tail */
} NfmcMalaArgs;

int nfmc_mala_steps_f32(const NfmcMalaArgs* args, nfmc_stream_t stream);

/* ---- K2: n_steps fused HMC trajectories.  Replaces `HMC.propose`/`hmc_trajectory` (hmc.py:61-126). */
typedef struct {
    float* x;
    int64_t n;
    int32_t d;
    int32_t n_steps;
    float step_size;
    int32_t n_leapfrog;
    int32_t adjust;             /* 1 = HMC, 0 = UHMC */
    int32_t reserved;
    const float* inv_mass_diag;
    NfmcPotential pot;
    NfmcRng rng;
    NfmcStats stats;
    NfmcSampleStore samples;
    uint8_t* masks_out;
    float* log_ratio_out;
    const NfmcJumpTail* jump;   /* as in NfmcMalaArgs */
    NfmcTune tune;              /* as in NfmcMalaArgs */
} NfmcHmcArgs;

int nfmc_hmc_steps_f32(const NfmcHmcArgs* args, nfmc_stream_t stream);

/* ---- Microcanonical Langevin Monte Carlo (Robnik, De Luca, Silverstein and Seljak, JMLR 2023; Robnik and Seljak 2024;
 * blackjax `mclmc`).  State of a chain: x in R^d and a unit velocity u in R^d, d >= 2; parameters: step size eps,
 * decoherence length L, per-coordinate scales sigma_j = sqrt(inv_mass_diag_j).  One step is B(eps/2) A(eps) B(eps/2) O:
 *     B(e), g = grad U(x):  gt = sigma * g, gn = |gt|, e_hat = -gt / gn, ue = u . e_hat, delta = e gn / (d - 1),
 *                           zeta = exp(-delta), uu = e_hat (1 - zeta)(1 + zeta + ue (1 - zeta)) + 2 zeta u, u <- uu / |uu|,
 *                           dK = (d - 1) [delta - ln 2 + log(1 + ue + (1 - ue) zeta^2)];  gn = 0: u unchanged, dK = 0
 *     A(eps):               x <- x + eps sigma * u
 *     O:                    nu = sqrt((exp(2 eps / L) - 1) / d);  u <- (u + nu z) / |u + nu z|, z ~ N(0, I) from the chain's
 *                           Philox stream at step counter rng.step0 + s on the noise stream (tag 0)
 * and the energy error of the step is dE = U(x') - U(x) + dK_1 + dK_2.  There is no Metropolis test: ACCEPTED = ATTEMPTED.
 * A step whose dE or new x is not finite is not taken: x keeps its value, u takes the O update from its value before the
 * step, and the chain is counted in NFMC_CNT_NONFINITE.  The second B of a step and the first B of the next share one
 * gradient, so a step costs one gradient and one value of U; every launch evaluates both once more at its starting x.
 * General kernels on the Philox4x32-10 stream at the default register layouts, every potential kind, d = 2 .. 1024.
 *
 * Warmup on the device (NfmcMclmcTune): after every `every` steps of a call a controller kernel pools the update's
 * n x every steps and rewrites the state words the next launch reads:
 *     V = sum of finite dE^2 / (count d)                         count: the update's steps with a finite dE and x'
 *     count = 0 or V not finite:  eps <- eps / 2, nothing else moves
 *     else  log eps <- log eps + clamp(log(target / V) / 6, -ln 2, ln 2)        (tune_step_size)
 *           s_j <- (1 - beta) s_j + beta v_j                                    (tune_inv_mass_diag; s = inv_mass_diag,
 *                                       v_j: unbiased variance of coordinate j over the update's states)
 *           L <- factor sqrt(sum_j v_j / s_j), s_j after its own update          (tune_decoherence_length)
 * `state` words (fp64), nfmc_mclmc_state_doubles(d, history_rows) of them, caller-allocated and caller-initialised: */
enum {
    NFMC_MCLMC_STEP_SIZE = 0,           /* eps: read by the kernel, rewritten by the controller */
    NFMC_MCLMC_DECOHERENCE_LENGTH = 1,  /* L: likewise */
    NFMC_MCLMC_TARGET = 2,              /* target of V (5e-4) */
    NFMC_MCLMC_IMD_ADJUSTMENT = 3,      /* beta */
    NFMC_MCLMC_DECOHERENCE_FACTOR = 4,  /* factor */
    NFMC_MCLMC_ENERGY_VARIANCE = 5,     /* V of the last update (out) */
    NFMC_MCLMC_COUNT = 6,               /* its count (out) */
    NFMC_MCLMC_HISTORY_ROWS = 7,        /* capacity of the history, in rows */
    NFMC_MCLMC_HISTORY_USED = 8,        /* updates so far; rows beyond the capacity are not written (in: 0) */
    NFMC_MCLMC_WORDS = 12               /* = NFMC_TUNE_WORDS: followed, as there, by 2 * padded_d + 4 words of column totals
                                           and padded_d words of the per-coordinate shift c (the caller initialises c: the
                                           column means of x0; zeros are valid), nfmc_tune_state_doubles(d) in all; then the
                                           history, one row per update */
};
/* A history row: eps and L the update's steps ran with, what they measured, and what the update left */
enum {
    NFMC_MCLMC_ROW_STEP_SIZE = 0,
    NFMC_MCLMC_ROW_DECOHERENCE_LENGTH = 1,
    NFMC_MCLMC_ROW_ENERGY_VARIANCE = 2,
    NFMC_MCLMC_ROW_COUNT = 3,
    NFMC_MCLMC_ROW_NEXT_STEP_SIZE = 4,
    NFMC_MCLMC_ROW_NEXT_DECOHERENCE_LENGTH = 5,
    NFMC_MCLMC_ROW_WORDS = 6
};
typedef struct {
    double* state;                  /* NULL: no tuning (step_size / decoherence_length / inv_mass_diag as given) */
    float* inv_mass_diag;           /* (d,) device, updated in place when tune_inv_mass_diag; must be the call's inv_mass_diag */
    int32_t tune_step_size;
    int32_t tune_decoherence_length;
    int32_t tune_inv_mass_diag;
    int32_t every;                  /* steps per controller update, as NfmcTune.every: the call enqueues every (kernel,
                                       controller) pair itself */
} NfmcMclmcTune;
/* nfmc_tune_state_doubles(d) + history_rows * NFMC_MCLMC_ROW_WORDS; 0 for arguments out of range */
int64_t nfmc_mclmc_state_doubles(int32_t d, int32_t history_rows);

typedef struct {
    float* x;                    /* (n, d) in/out */
    float* velocity;             /* (n, d) in/out: unit rows */
    int64_t n;
    int32_t d;                   /* 2 .. 1024 */
    int32_t n_steps;             /* 1..NFMC_MAX_STEPS_PER_CALL */
    float step_size;
    float decoherence_length;
    const float* inv_mass_diag;  /* (d,) or NULL = ones */
    NfmcPotential pot;
    NfmcRng rng;                 /* rounds 0 or 10; replay_normals as for the other samplers, no uniforms are drawn */
    NfmcStats stats;             /* defer must be 0: the call folds its partials itself */
    NfmcSampleStore samples;     /* state after every step */
    float* energy_out;           /* NULL or (n_steps, n): dE of every step */
    double* energy_sums;         /* NULL or 3 doubles, += sum of finite dE^2, sum of finite dE, count of finite steps; needs
                                    `stats` (the sums travel through its per-workgroup partials, folded in a fixed order) */
    NfmcMclmcTune tune;          /* warmup on the device; needs `stats` */
} NfmcMclmcArgs;

/* Status codes as nfmc_hmc_steps_f32; in addition d < 2 is NFMC_EINVAL and rng.rounds == 7 NFMC_EUNSUPPORTED. */
int nfmc_mclmc_steps_f32(const NfmcMclmcArgs* args, nfmc_stream_t stream);

/* K4: x -> z, logdet_forward; log_prob = N(z;0,I) + logdet (either output may be NULL).
 * Replaces `bijection.forward` / `Flow.log_prob` (jump.py:218, imh.py:214). */
int nfmc_realnvp_forward_f32(const NfmcRealNVP* flow, const float* x, int64_t n, float* z, float* logdet,
                             float* log_prob, nfmc_stream_t stream);

/* K3: z -> x, logdet_inverse; z == NULL draws z ~ N(0,I) from `rng` (stream 2); log_q = log q(x).
 * Replaces `bijection.inverse` / `Flow.sample(n, return_log_prob=True)` (jump.py:205, imh.py:221, neutra.py:60). */
int nfmc_realnvp_inverse_f32(const NfmcRealNVP* flow, const float* z, int64_t n, float* x, float* logdet,
                             float* log_q, const NfmcRng* rng, nfmc_stream_t stream);

/* ---- K3+K4+K6+K7 fused: n_steps independent-MH transitions with the flow as proposal.
 * n_steps = 1, logq_cached = 0 is the jump of `JumpNFMC.sample` (jump.py:205-243);
 * n_steps = K with the cached log q(x) is `FixedIMH.sample` (imh.py:214-249). */
typedef struct {
    float* x;                 /* (n, d) in/out */
    float* logq;              /* (n,) cached log q(x): read if logq_cached, always written */
    int64_t n;
    int32_t n_steps;
    int32_t logq_cached;
    int32_t adjusted;         /* 0: accept every proposal (adjusted_jumps=False, jump.py:228-229) */
    int32_t reserved;
    NfmcRealNVP flow;
    NfmcPotential pot;
    NfmcRng rng;              /* replay_normals are the latents z (n_steps, n, d) */
    NfmcStats stats;          /* counters use the ACCEPTED/ATTEMPTED words */
    NfmcSampleStore samples;
    uint8_t* masks_out;
    float* log_ratio_out;
} NfmcFlowMhArgs;

int nfmc_flow_mh_steps_f32(const NfmcFlowMhArgs* args, nfmc_stream_t stream);

/* NFMC_OK when nfmc_flow_mh_steps_f32 has a kernel for `args` (launches nothing), NFMC_EUNSUPPORTED when not -- e.g.
 * ragged d > ~300 with a narrow conditioner whose weight image does not fit the LDS and whose wave tiles do not
 * either: the caller then composes the transition from nfmc_realnvp_inverse_f32 / nfmc_realnvp_forward_f32 and
 * nfmc_mh_accept_select_f32 (the split path every foreign flow object takes; jump.py:205-231). */
int nfmc_flow_mh_supported_f32(const NfmcFlowMhArgs* args);

/* ---- A whole run of `JumpNFMC.sample` (jump.py:156-246) in one call: for each of n_outer outer iterations, the n_inner
 * inner transitions -- nfmc_mala_steps_f32 / nfmc_hmc_steps_f32 launches of at most NFMC_MAX_STEPS_PER_CALL steps -- and
 * then ONE flow-MH step (nfmc_flow_mh_steps_f32, n_steps = 1, logq_cached = 0): the launches a host loop over the two entry
 * points enqueues, in its order.  With s = inner->rng.step0 the inner launch that starts `off` transitions into iteration i
 * runs from transition s + i (n_inner + 1) + off, the jump of iteration i is transition s + i (n_inner + 1) + n_inner
 * (n_steps, rng.step0 of the structs are otherwise not read).
 *
 * n_parts > 1 splits the chains into that many ranges -- part p = chains [p m, min(n, (p + 1) m)), m = n / n_parts rounded
 * up to whole workgroup tiles of both kernels; a part without chains launches nothing -- and enqueues part 0 on `stream`
 * and every other part on a stream the library keeps for it (created on first use, per device, never destroyed), so that
 * the jump of one part runs beside the inner kernel of another and their launch boundaries fall inside kernels.  The side
 * streams start behind everything enqueued on `stream` before the call, and `stream` continues behind them: to the caller
 * the call is ordered on `stream` like every other entry point, also when it returns an error.  Each chain sees the
 * arguments, the global chain id and the transitions of the unsplit run: states and logq are bitwise those of n_parts = 1,
 * the counters exact; the moments are the same per-workgroup partials folded from other slabs (fp64 rounding).  Part p
 * writes the statistics slabs from p * ceil(2048 / n_parts) on.
 *
 * Both structs describe the same chains (x, n, d, rng.seed / chain_offset / rounds, stats) and are otherwise filled as for
 * their own entry points, with statistics either off or deferred (stats.defer = 1), and without what a host would have to
 * advance between the launches: no jump tail, no tuning, no sample store, no mask / log-ratio outputs, no replayed noise
 * (NFMC_EINVAL).  Where the jump does not run on the register-layout kernels (n_hidden > 8, d > 512) the run is one part. */
enum { NFMC_INNER_MALA = 0, NFMC_INNER_HMC = 1 };
#define NFMC_JUMP_RUN_MAX_PARTS 4
typedef struct {
    int32_t inner_kind;          /* NFMC_INNER_MALA: inner -> NfmcMalaArgs; NFMC_INNER_HMC: inner -> NfmcHmcArgs */
    int32_t n_parts;             /* 1 .. NFMC_JUMP_RUN_MAX_PARTS; 1 = everything on `stream`, no event, no side stream */
    const void* inner;
    const NfmcFlowMhArgs* jump;
    int32_t n_outer;             /* T >= 1 */
    int32_t n_inner;             /* K >= 1 */
} NfmcJumpRun;

int nfmc_jump_run_f32(const NfmcJumpRun* run, nfmc_stream_t stream);

/* The same run of n_steps independent-MH transitions (FixedIMH.sample, imh.py:200-255) as a data-parallel problem:
 * the proposals of an independence sampler do not depend on the state, so all n * n_steps of them are evaluated at
 * once, a per-chain scan (one lane per chain) applies the Metropolis tests, and proposals are replayed for the moments /
 * sample store / final state: the accepted ones weighted by their dwell times, or -- when more than about half are
 * accepted and no samples are stored -- only the corrections to the sums the proposal pass kept over all of them.
 * Same noise streams and results as
 * nfmc_flow_mh_steps_f32 (states and masks bit for bit; moments up to summation order).  Faster at every
 * chain count measured (3x at n = 1000, 1.15x at n = 65536, d = 64): few chains no longer leave the GPU idle, and the
 * accept uniforms are drawn once per (chain, step) instead of once per lane.  Requires adjusted = 1, n_hidden <= 8 (affine or 8-bin spline couplings), n_steps <= NFMC_IMH_PARALLEL_MAX_STEPS;
 * `work` >= nfmc_imh_parallel_work_bytes(n, d, n_steps) bytes of device scratch, 16-byte aligned. */
#define NFMC_IMH_PARALLEL_MAX_STEPS 65536
int64_t nfmc_imh_parallel_work_bytes(int64_t n, int32_t d, int32_t n_steps);
int nfmc_imh_parallel_f32(const NfmcFlowMhArgs* args, void* work, int64_t work_bytes, nfmc_stream_t stream);
/* NFMC_OK when nfmc_imh_parallel_f32 has a kernel for `args` (validates, launches nothing). */
int nfmc_imh_parallel_supported_f32(const NfmcFlowMhArgs* args);

/* ---- K5 + K2: HMC in latent space on U~(z) = U(f^-1(z)) - logdet_inv(z), gradient by a hand-written
 * VJP through the coupling stack.  Replaces `NeuTra.adjusted_target` under `HMC.propose`
 * (neutra.py:58-68,109-129; hmc.py:40-48,96-126). */
typedef struct {
    float* z;                 /* (n, d) latent state in/out */
    int64_t n;
    int32_t n_steps;
    int32_t n_leapfrog;
    float step_size;
    int32_t adjust;
    const float* inv_mass_diag;
    NfmcRealNVP flow;
    NfmcPotential pot;
    NfmcRng rng;
    NfmcStats stats;          /* moments of the latent z (reference quirk) */
    NfmcSampleStore samples;
    uint8_t* masks_out;
    float* log_ratio_out;
    float* scratch;           /* matrix-core path (n_hidden > 32) only: >= nfmc_neutra_scratch_bytes(...) bytes */
    int64_t scratch_bytes;
} NfmcNeutraHmcArgs;

/* 0 for the VALU path (n_hidden <= 32).  Matrix-core path at d = 64 / 128: 2 (n, d) tiles + 2 (n,) vectors, plus the activation
 * checkpoints of the resident workgroups (hidden activations, alpha, beta of every coupling layer: the reverse sweep
 * reads them back instead of recomputing them) -- at most 256 workgroups x 128 chains, whatever n.  At the other multiples
 * of 32 (trajectory composed from the streamed gradient kernel, csrc/mfma_wide.hip): 4 (n, d) arrays + 3 (n,) vectors + the
 * gradient kernel's own workspace (nfmc_flow_scratch_bytes with the gradient; NfmcRealNVP.scratch is not used by this call). */
int64_t nfmc_neutra_scratch_bytes(int64_t n, int32_t d, int32_t n_hidden, int32_t n_hidden_layers, int32_t n_coupling);

int nfmc_neutra_hmc_steps_f32(const NfmcNeutraHmcArgs* args, nfmc_stream_t stream);

/* ---- Random-walk Metropolis in latent space on the same U~(z): z' = z + eps * inv_mass_diag (the diagonal itself, not
 * its square root), accepted iff log u < U~(z) - U~(z').  One flow inverse and one potential value per transition, no
 * gradient.  Replaces `NeuTra.adjusted_target` under `MH.propose` (neutra.py:147-159; mh.py:44-73).  adjust = 0 keeps
 * every proposal and never evaluates U~.  The draws are those of the HMC entry point above: its momentum normals and
 * its accept uniforms, so they are also what nfmc_philox_normals_f32 / nfmc_mh_accept_select_f32 draw for the split path.
 * VALU kernels only: n_hidden <= 32 and d <= 512; a wider conditioner answers NFMC_EUNSUPPORTED.  No workspace. */
typedef struct {
    float* z;                 /* (n, d) latent state in/out */
    int64_t n;
    int32_t n_steps;
    int32_t adjust;
    const float* inv_mass_diag;   /* (d,) or NULL for all ones */
    NfmcRealNVP flow;
    NfmcPotential pot;
    NfmcRng rng;
    NfmcStats stats;          /* moments of the latent z (reference quirk) */
    NfmcSampleStore samples;
    uint8_t* masks_out;       /* (n_steps, n) or NULL */
    float* log_ratio_out;     /* (n_steps, n) or NULL */
} NfmcNeutraMhArgs;

int nfmc_neutra_mh_steps_f32(const NfmcNeutraMhArgs* args, nfmc_stream_t stream);

/* Adjusted potential and its gradient alone (tests; split path).  n_hidden <= 32: every d <= 512.  n_hidden 33..128
 * (matrix cores): d = 64 / 128 register-resident, every other multiple of 32 up to 512 with the state and the gradient
 * streamed through the caller's workspace NfmcRealNVP.scratch (nfmc_flow_scratch_bytes; csrc/mfma_wide.hip); other d:
 * NFMC_EUNSUPPORTED.  nfmc_realnvp_forward_f32 / nfmc_realnvp_inverse_f32 use the same streamed kernels at those d. */
int nfmc_neutra_potential_grad_f32(const NfmcRealNVP* flow, const NfmcPotential* pot, const float* z, int64_t n,
                                   float* u_out, float* grad_out, nfmc_stream_t stream);

/* ---- DLMC (nfmc/algorithms/sampling/nfmc/dlmc.py).  Replaces `compute_grad(lambda v: self.target(v) +
 * flow_log_prob(v), x)` and the gradient step `x = x - self.kernel.step_size * grad` (dlmc.py:85-87), whose flow half
 * is torch.autograd through `flow.log_prob` (dlmc.py:52-53).  Kernels (csrc/dlmc_kernels.hip): a reverse sweep through
 * the forward map x -> z, one chain per lane, for affine / additive couplings with n_hidden <= 8 and d <= 512; other
 * flows (splines, wider conditioners) answer NFMC_EUNSUPPORTED and the caller composes the step from autograd. */
typedef struct {
    NfmcRealNVP flow;
    const float* x;           /* (n, d) */
    int64_t n;
    float* grad_out;          /* (n, d) grad_x log q(x), or NULL */
    float* logq_out;          /* (n,) log q(x) (flow.log_prob, jump.py:218), or NULL; not both NULL */
} NfmcFlowLogqGradArgs;

int nfmc_flow_logq_grad_f32(const NfmcFlowLogqGradArgs* args, nfmc_stream_t stream);
/* Dry run: 0 when nfmc_flow_logq_grad_f32 has a kernel for args, else the status it would return. */
int nfmc_flow_logq_grad_supported_f32(const NfmcFlowLogqGradArgs* args);

typedef struct {
    NfmcRealNVP flow;
    NfmcPotential pot;        /* closed-form U, used when grad_u is NULL (QUADRATIC or FUNNEL) */
    float* x;                 /* (n, d) in place: x <- x - step_size (grad U(x) + grad_x log q(x))  (dlmc.py:85-87) */
    const float* grad_u;      /* (n, d) grad U(x) computed by the caller (autograd targets), or NULL -> pot */
    float* logq_out;          /* (n,) log q at the PRE-step x, or NULL */
    int64_t n;
    float step_size;          /* DLMCKernel.step_size (dlmc.py:14), >= 0 */
    int32_t reserved;
} NfmcDlmcStepArgs;

int nfmc_dlmc_step_f32(const NfmcDlmcStepArgs* args, nfmc_stream_t stream);
/* Dry run: 0 when nfmc_dlmc_step_f32 has a kernel for args, else the status it would return. */
int nfmc_dlmc_step_supported_f32(const NfmcDlmcStepArgs* args);

/* ---- split path for arbitrary Python targets (U and grad U come from torch autograd on the GPU).
 * K6: mask = log(u) < lp_t' - lp_t + lp_q - lp_q' (nfmc/util.py:382-392), x[mask] = x'[mask]
 * (mcmc/base.py:77), optional carried per-chain scalars, counters.  log(u) is the hardware log2 (about one ulp of
 * log2); a NaN ratio rejects, +inf accepts; every row with !(|log_ratio| <= 3.0e38f) counts in NFMC_CNT_NONFINITE
 * whichever way it went; log_ratio = NULL accepts every row and counts none.  ATTEMPTED += n (defer = 1: what the fold is
 * told).  sum_x / sum_x2 are the fp64 sums of the fp32 values of x and of their fp32 squares up to 2048 workgroup tiles
 * of 4 * 64 / (padded_d / 4, at most 64) rows; past that a lane adds the rows of its tiles in fp32 before widening.
 * d <= 1024 (NFMC_ESHAPE); the default Philox stream only. */
typedef struct {
    float* x;                 /* (n, d) in/out */
    const float* x_prime;     /* (n, d) */
    int64_t n;
    int32_t d;
    int32_t n_carry;          /* 0..2 per-chain vectors selected with the same mask (imh.py:233) */
    const float* log_ratio;   /* (n,) or NULL = accept all */
    const float* uniforms;    /* (n,) replay uniforms or NULL -> Philox stream `rng_tag` */
    float* carry[2];
    const float* carry_prime[2];
    NfmcRng rng;
    int32_t rng_tag;          /* 1 = accept stream, 3 = jump stream */
    int32_t reserved;
    NfmcStats stats;          /* moments of the post-selection x + counters */
    uint8_t* mask_out;
} NfmcSelectArgs;

int nfmc_mh_accept_select_f32(const NfmcSelectArgs* args, nfmc_stream_t stream);

/* Langevin proposal and log acceptance ratio from externally computed U, grad U
 * (langevin.py:74-76 and :31-42,88-105). */
int nfmc_langevin_propose_f32(const float* x, const float* grad_u, const float* inv_mass_diag, float step_size,
                              int64_t n, int32_t d, const NfmcRng* rng, float* x_prime, nfmc_stream_t stream);
int nfmc_langevin_log_ratio_f32(const float* x, const float* x_prime, const float* u, const float* u_prime,
                                const float* grad_u, const float* grad_u_prime, const float* inv_mass_diag,
                                float step_size, int64_t n, int32_t d, float* log_ratio, nfmc_stream_t stream);

/* K7 alone: sum_x += sum_rows x, sum_x2 += sum_rows x^2 over a (rows, d) block. */
int nfmc_moments_update_f32(const float* x, int64_t rows, int32_t d, const NfmcStats* stats, nfmc_stream_t stream);

/* ---- convergence diagnostics of the kept states (split R-hat, nested R-hat, ESS): the per-chain part on the device.
 * x holds n_draws kept states of n chains in chronological order, row t = n * d contiguous floats.  For every
 * (chain j, coordinate c) series the kernel takes the mean m_j (fp64), the biased autocovariances about it
 * a_{j,l} = (1 / n_draws) sum_{t < n_draws - l} (x_t - m_j)(x_{t+l} - m_j), l = 0 .. max_lag (fp32 products of the
 * centred draws, lagged operands from a window held on chip; lags >= n_draws are empty sums = 0), the means m_h and
 * unbiased variances s2_h of the two half-chains [0, h) and [n_draws - h, n_draws), h = n_draws / 2, and, per superchain k
 * of `group` consecutive chains, mu_k = mean of its m_j and Bt_k = their unbiased variance (0 when group = 1).  `sums`
 * receives per-coordinate fp64 totals, NFMC_DIAG_* + max_lag + 1 rows of d doubles:
 *     row NFMC_DIAG_SUM_M       sum_j m_j               row NFMC_DIAG_SUM_M2      sum_j m_j^2
 *     row NFMC_DIAG_SUM_MH      sum_h m_h (2n halves)   row NFMC_DIAG_SUM_MH2     sum_h m_h^2
 *     row NFMC_DIAG_SUM_S2H     sum_h s2_h
 *     row NFMC_DIAG_SUM_MU      sum_k mu_k              row NFMC_DIAG_SUM_MU2     sum_k mu_k^2
 *     row NFMC_DIAG_SUM_BT      sum_k Bt_k
 *     row NFMC_DIAG_ACOV + l    sum_j a_{j,l}           (sum_j s2_j = row NFMC_DIAG_ACOV * n_draws / (n_draws - 1))
 * Every row is additive over disjoint sets of chains (whole superchains), so shards combine by one sum.  The totals are
 * folded in a fixed order through `work` (no atomics: the same input gives the same bits); `sums` is overwritten.  The
 * slab is read twice (means, centred products).  NFMC_EINVAL: NULL pointer, non-positive size, n_draws < 4, max_lag < 0,
 * group < 1 or not dividing n; NFMC_ESHAPE: d > 1024 or max_lag > NFMC_DIAG_MAX_LAG; NFMC_ESCRATCH: work too small. */
#define NFMC_DIAG_MAX_LAG 127
enum {
    NFMC_DIAG_SUM_M = 0,
    NFMC_DIAG_SUM_M2 = 1,
    NFMC_DIAG_SUM_MH = 2,
    NFMC_DIAG_SUM_MH2 = 3,
    NFMC_DIAG_SUM_S2H = 4,
    NFMC_DIAG_SUM_MU = 5,
    NFMC_DIAG_SUM_MU2 = 6,
    NFMC_DIAG_SUM_BT = 7,
    NFMC_DIAG_ACOV = 8
};
typedef struct {
    const float* x;           /* (n_draws, n, d) */
    int64_t n_draws;
    int64_t n;
    int32_t d;
    int32_t max_lag;          /* 0 .. NFMC_DIAG_MAX_LAG */
    int32_t group;            /* chains per superchain; divides n */
    int32_t reserved;
    double* sums;             /* out: nfmc_diag_sums_doubles(d, max_lag) doubles */
    void* work;               /* device scratch, 8-byte aligned, no initialisation needed */
    int64_t work_bytes;       /* >= nfmc_diag_work_bytes(n, d, max_lag) */
} NfmcDiagArgs;
int64_t nfmc_diag_sums_doubles(int32_t d, int32_t max_lag);            /* 0 for arguments out of range */
int64_t nfmc_diag_work_bytes(int64_t n, int32_t d, int32_t max_lag);   /* 0 for arguments out of range */
int nfmc_chain_diagnostics_f32(const NfmcDiagArgs* args, nfmc_stream_t stream);

/* ---- running diagnostics for runs that keep no states: an accumulator in device memory that is fed every kept draw
 * exactly once, in blocks, and from which the `sums` of nfmc_chain_diagnostics_f32 (same rows, same layout) can be
 * produced at any time.  Its size does not grow with the run.  Per series (chain j, coordinate c) it holds the shift s_j
 * (the first draw), the fp64 sum S_j of the shifted draws y_t = x_t - s_j, the fp64 sum and sum of squares of y over the
 * half-chains [0, h) and [n_draws_planned - h, n_draws_planned), h = n_draws_planned / 2, the first max_lag and the last
 * max_lag shifted draws as fp32 (the last ones in a ring: draw t in row t mod max_lag), and per workgroup of the update one
 * row of fp64 lag products P_l = sum_j sum_t y_t y_{t-l} (fp32 products of the fp32-rounded y; fp32 sums inside one block
 * of draws, fp64 from there on; no atomics).  With mu_j = S_j / K after K draws, for l < K
 *     K a_{j,l} = P_{j,l} - mu_j (2 S_j - head_l(j) - tail_l(j)) + (K - l) mu_j^2
 * (head_l / tail_l: the sum of the first / last l shifted draws) is the autocovariance sum of nfmc_chain_diagnostics_f32;
 * lags l >= K are exact zeros.  The same draws in the same blocks give the same bits; other blocks differ by the fp32
 * rounding of the sums inside a block.
 * state: nfmc_diag_stream_state_bytes = 8 (5 S + nb (max_lag + 1) d) + 4 (1 + 2 max_lag) S bytes rounded up to 8, S = n d,
 * nb = min(ceil(n / max(1, 64 / d)), 1024 / ceil(d / 64)) workgroup rows; 8-byte aligned, put into the "no draws seen"
 * condition by nfmc_diag_stream_reset_f32 (which also zeroes n_seen).  The descriptor lives in host memory; the library
 * keeps n_seen in it, advanced when an update is enqueued (calls on one stream see the draws in that order).  One
 * descriptor per state: it must not be used from two host threads at once, and a copy made before an update must not be
 * passed to a later call -- its stale n_seen would pass the first_draw check against the wrong count.  Both size functions return 0 for d > 1024 or max_lag outside 0 .. NFMC_DIAG_MAX_LAG.
 * Status of every entry point: NFMC_EINVAL: NULL pointer, non-positive size; NFMC_ESHAPE: d > 1024 or max_lag >
 * NFMC_DIAG_MAX_LAG; NFMC_ESCRATCH: state (or work) too small.  All answered before any launch. */
typedef struct {
    void* state;              /* device memory, >= nfmc_diag_stream_state_bytes(n, d, max_lag) */
    int64_t state_bytes;
    int64_t n;
    int32_t d;
    int32_t max_lag;          /* 0 .. NFMC_DIAG_MAX_LAG */
    int64_t n_draws_planned;  /* the draws the run will feed: fixes the half-chains */
    int64_t n_seen;           /* draws fed so far: written by reset and update, read by sums */
} NfmcDiagStream;
int64_t nfmc_diag_stream_state_bytes(int64_t n, int32_t d, int32_t max_lag);
int64_t nfmc_diag_stream_work_bytes(int64_t n, int32_t d, int32_t max_lag);
int nfmc_diag_stream_reset_f32(NfmcDiagStream* acc, nfmc_stream_t stream);
/* Folds n_rows new draws into the accumulator.  They sit in a staging ring described like NfmcSampleStore: draw
 * first_draw + r in ring row (row + r) mod ring_rows, each row n * d floats.  first_draw must equal acc->n_seen -- a
 * dropped or repeated block is an error, not a silently wrong answer -- and first_draw + n_rows must not pass
 * n_draws_planned; also NFMC_EINVAL: n_rows > ring_rows, row outside the ring.  The ring is only read. */
typedef struct {
    NfmcDiagStream* acc;
    const float* ring;        /* (ring_rows, n, d) */
    int32_t ring_rows;
    int32_t row;              /* ring row of the first new draw */
    int32_t n_rows;           /* 1 .. ring_rows */
    int32_t reserved;
    int64_t first_draw;       /* global index of the first new draw */
} NfmcDiagStreamArgs;
int nfmc_diag_stream_update_f32(const NfmcDiagStreamArgs* args, nfmc_stream_t stream);
/* The `sums` of nfmc_chain_diagnostics_f32 for the acc->n_seen draws fed so far (n_draws there = n_seen here), superchains
 * of `group` chains through the same group and fold kernels.  The state is only read: it may be called in mid-run and
 * the run continues to the same bits.  When n_seen != n_draws_planned the half-chain sums do not describe halves of what
 * was seen: rows NFMC_DIAG_SUM_MH, _MH2 and _S2H are NaN then, every other row is that of the draws seen.
 * NFMC_EINVAL also: n_seen < 4, group < 1 or not dividing n.  work: nfmc_diag_stream_work_bytes, 8-byte aligned, no
 * initialisation needed. */
typedef struct {
    const NfmcDiagStream* acc;
    int32_t group;            /* chains per superchain; divides n */
    int32_t reserved;
    double* sums;             /* out: nfmc_diag_sums_doubles(d, max_lag) doubles */
    void* work;
    int64_t work_bytes;       /* >= nfmc_diag_stream_work_bytes(n, d, max_lag) */
} NfmcDiagStreamSumsArgs;
int nfmc_diag_stream_sums_f32(const NfmcDiagStreamSumsArgs* args, nfmc_stream_t stream);

/* ---- rank transform for the rank-normalised diagnostics (Vehtari et al. 2021): one of four series of the kept states,
 * each again an (n_draws, n, d) slab for nfmc_chain_diagnostics_f32.  Per coordinate the S = n_draws * n values
 * v_1 .. v_S are pooled over draws and chains and compared numerically (-0 = +0); x_(k) is the k-th smallest, k = 0 .. S-1.
 *     rank       r_i = #{v < v_i} + (#{v = v_i} + 1) / 2                 (1-based average rank)
 *     score      z_i = Phi^-1((r_i - 3/8) / (S + 1/4)), in fp64 (AS 241 PPND16), rounded to fp32 once
 *     median     med = (x_(floor((S-1)/2)) + x_(ceil((S-1)/2))) / 2 in fp64
 *     NFMC_RANK_BULK       z of v
 *     NFMC_RANK_FOLDED     z of f, f_i = fl32(|fp64(v_i) - med|), ranked anew
 *     NFMC_RANK_TAIL_LOW   1 where v_i <= x_(floor((S-1)/20)), else 0   (the type-7 5 % quantile on fp32 data)
 *     NFMC_RANK_TAIL_HIGH  1 where v_i >= x_(ceil(19 (S-1)/20)), else 0 (the type-7 95 % quantile)
 * A coordinate with a NaN or +-Inf in x is NaN in every series and counted in `nonfinite`; the others are unaffected.
 * The outputs are functions of the values alone (a keys-only radix sort per coordinate, then two binary searches per
 * element): no floating-point atomic, the same bits on every call.  x is only read.
 * work: nfmc_rank_work_bytes = 32 d  +  2 * 4 S d (two key buffers of the slab's size)  +  1024 d ceil(S / 2048) (digit
 * counts of the sort) bytes, 8-byte aligned, no initialisation needed.
 * NFMC_EINVAL: NULL x / out / nonfinite / work, out == x, non-positive size, n_draws < 4, unknown series; NFMC_ESHAPE:
 * d > 1024 or S >= 2^31; NFMC_ESCRATCH: work too small.  All answered before any launch. */
#define NFMC_RANK_BULK 0
#define NFMC_RANK_FOLDED 1
#define NFMC_RANK_TAIL_LOW 2
#define NFMC_RANK_TAIL_HIGH 3
typedef struct {
    const float* x;           /* (n_draws, n, d) kept states */
    int64_t n_draws;
    int64_t n;
    int32_t d;                /* <= 1024, as nfmc_chain_diagnostics_f32 */
    int32_t series;           /* NFMC_RANK_* */
    float* out;               /* (n_draws, n, d); must not alias x */
    double* order_stats;      /* (d, 4) or NULL: x_(floor((S-1)/20)), the two middle order statistics, x_(ceil(19 (S-1)/20)),
                                 as fp64 (a zero is +0; NaN where the order statistic is not finite) */
    int32_t* nonfinite;       /* (d,) count of NaN / Inf values per coordinate */
    void* work;
    int64_t work_bytes;       /* >= nfmc_rank_work_bytes(n_draws, n, d) */
} NfmcRankArgs;
int64_t nfmc_rank_work_bytes(int64_t n_draws, int64_t n, int32_t d);   /* 0 for arguments out of range */
int nfmc_rank_series_f32(const NfmcRankArgs* args, nfmc_stream_t stream);

/* Philox normals / uniforms alone (tests pin the native stream against oracle/philox.py). */
int nfmc_philox_normals_f32(const NfmcRng* rng, int32_t tag, int64_t n, int32_t d, float* out, nfmc_stream_t stream);
int nfmc_philox_uniforms_f32(const NfmcRng* rng, int32_t tag, int64_t n, float* out, nfmc_stream_t stream);

/* ---- introspection */
#define NFMC_MAX_STEPS_PER_CALL 512
/* ---- f1: maximum-likelihood (re)fit of the RealNVP proposal on the device.
 * Replaces the torchflows `Flow.fit` epochs of jump.py:139-151 (warmup), jump.py:193-201 (refit when fit_nf) and
 * imh.py:166-170 (AdaptiveIMH).  One call = one optimiser step on one batch: the mean negative log-likelihood of the rows
 * x (n, d), its gradient with respect to every parameter (hand-written reverse sweep, csrc/fit_kernels.hip) and the AdamW
 * update (torch.optim.AdamW semantics).  The trainable vector `params` has the layout of the flow's weight blob -- coupling
 * layers (n_coupling * layer_stride floats, VALU layout above), then at `ea_off` the four ElementwiseAffine vectors
 * (ea0 log-scale, ea0 shift, ea1 log-scale, ea1 shift; d4 = d rounded up to 4 floats each) -- and `flow`'s pointers must be
 * views of it (weights = params, ea0_log_scale = params + ea_off, ...), so the sampling kernels see every step at once.
 * Shapes: affine / additive couplings (n_bins = 0), one or two hidden layers; n_hidden <= 8 at d <= 512, n_hidden 9..32 at
 * d <= 256, n_hidden 33..128 at d = 64 / 128; rational-quadratic spline couplings (n_bins = 8, `spline_bound` > 0: W3 holds
 * 23 d_b rows, target-major, and b3 as many entries; layer_stride >= nfmc_coupling_layer_floats(d, n_hidden, n_hidden_layers, 8)
 * and a multiple of 4, `params` 16-byte aligned) with n_hidden <= 8 at d <= 256, both losses, on the (row, target)-pair kernel
 * of csrc/fit_rqs.hip (nfmc_flow_fit_supported_f32); other flows are trained by the host package's torch path.
 * Conditioners of width <= 8 (every default flow) run on the row-per-wave kernel (csrc/fit_rows.hpp: up to 1024 waves per
 * launch); it needs `params` 16-byte aligned and layer_stride, ea_off multiples of 4 floats (NFMC_EALIGN otherwise). */
typedef struct {
    float lr, beta1, beta2, eps, weight_decay;
    int32_t step;             /* 1-based count of applied steps, for the bias corrections */
} NfmcAdamW;

typedef struct {
    NfmcRealNVP flow;         /* views of `params` (see above) */
    float* params;            /* (n_params) trainable vector, updated in place */
    float* adam_m;            /* (n_params) first moments, zero before the first step */
    float* adam_v;            /* (n_params) second moments */
    int64_t n_params;         /* >= ea_off + 4 * d4 */
    int64_t ea_off;           /* offset of the ElementwiseAffine vectors inside params (multiple of 4) */
    float* partial;           /* scratch, >= nfmc_flow_fit_partial_floats(n, n_params) floats, ZEROED once by the caller */
    int64_t partial_floats;
    float* status;            /* device (3): [0] mean loss of the batch at the parameters BEFORE the step;
                                 [1] 1 if the step was applied, 0 if the loss was not finite (parameters untouched);
                                 [2] mean NLL of the validation rows at the parameters BEFORE the step ([0] if none) */
    const float* x_val;       /* optional (maximum likelihood only): validation rows (n_val, d), evaluated in the same launch */
    int64_t n_val;
    float* params_prev;       /* optional (n_params): receives the parameters as they were BEFORE the step -- what the
                                 validation loss of this call belongs to (best-weights bookkeeping without a second launch) */
    float* best;              /* runs (nfmc_flow_fit_epochs_f32) with keep_best_weights: (n_params) the weights the best
                                 monitored loss so far belongs to; call 0 initialises it with the starting weights */
    float* run_state;         /* runs: device, 2 x NFMC_FIT_STATE_FLOATS floats (call c reads half c & 1, writes the other) */
    float* scratch;           /* conditioners of width 33..128 (matrix-core kernel, csrc/fit_mfma.hip): the resident waves'
                                 activation checkpoints, >= nfmc_flow_fit_workspace(...) bytes, 16-byte aligned; NULL elsewhere */
    int64_t scratch_bytes;
} NfmcFlowFit;

/* The epoch loop of `Flow.fit` / `Flow.variational_fit` (torchflows, as nfmc drives it: jump.py:139-151 early stopping +
 * keep_best_weights + ValueError on divergence; imh.py:67-72; neutra.py:84-91) with its bookkeeping ON THE DEVICE: call c of
 * a run computes the batch loss (and the validation loss) at the weights w_c, decides -- in the fold kernel -- whether the
 * monitored loss improved (best weights <- w_c with validation rows, w_{c+1} without), whether to stop early, whether the
 * run diverged (non-finite loss), and applies the AdamW step unless the run has ended; calls after the end are no-ops.
 * The host enqueues any number of calls and reads `run_state` when it wants to (at the end; every few epochs under a time
 * limit).  With validation rows the run has n_epochs + 1 calls: the last one (index n_epochs) only evaluates. */
typedef struct {
    int32_t n_epochs;                 /* optimiser steps of the run at most */
    int32_t early_stopping;           /* stop once the monitored loss has not improved for more than `threshold` epochs */
    int32_t early_stopping_threshold;
    int32_t keep_best_weights;        /* maintain NfmcFlowFit.best */
    int32_t skip_nonfinite;           /* a non-finite batch loss skips the epoch (variational fits with
                                         check_for_divergences = False) instead of ending the run as diverged */
    int32_t reserved;
} NfmcFitControl;
enum {
    NFMC_FIT_BEST_LOSS = 0,    /* best monitored loss so far (+inf before the first booked epoch) */
    NFMC_FIT_SINCE_BEST = 1,   /* booked epochs since it improved */
    NFMC_FIT_APPLIED = 2,      /* optimiser steps applied (AdamW's bias corrections use applied + 1) */
    NFMC_FIT_STOPPED = 3,      /* 1: early stopping ended the run */
    NFMC_FIT_DIVERGED = 4,     /* 1: a non-finite loss ended the run (the host package raises ValueError) */
    NFMC_FIT_LAST_LOSS = 5,    /* batch loss of the latest live call */
    NFMC_FIT_LAST_VAL = 6,     /* validation loss of the latest live call */
    NFMC_FIT_BOOKED = 7,       /* epochs whose monitored loss has been booked */
    NFMC_FIT_STATE_FLOATS = 8
};

int nfmc_flow_fit_supported_f32(const NfmcRealNVP* flow);
int64_t nfmc_flow_fit_partial_floats(int64_t n, int64_t n_params);
/* Workspace of a fit of `flow` on n batch rows (+ n_val validation rows) with a trainable vector of n_params floats:
 * returns the bytes of NfmcFlowFit.scratch (0 for conditioners of width <= 32) and stores the floats `partial` must hold
 * (one slab of n_params + 4 floats per workgroup of the gradient launch; for spline couplings the launch is capped so that
 * the slabs never exceed 64 MiB).  Conditioners of width 33..128 are trained at
 * d = 64 / 128 (the shapes of the register-resident matrix-core kernels) with the trainable vector in the matrix-core blob
 * layout (csrc/mfma_device.hpp: every matrix in both orientations; the gradient kernel writes both slots, AdamW keeps them
 * equal), layer_stride >= nfmc_realnvp_layer_floats(d, n_hidden, n_hidden_layers) and a multiple of 4. */
int64_t nfmc_flow_fit_workspace(const NfmcRealNVP* flow, int64_t n, int64_t n_val, int64_t n_params, int64_t* partial_floats);
int nfmc_flow_fit_step_f32(const NfmcFlowFit* fit, const float* x, int64_t n, const NfmcAdamW* opt, nfmc_stream_t stream);
/* The same step for the variational fit of imh.py:67-72 / neutra.py:84-91 (`Flow.variational_fit`): rows z (n, d) are
 * latents drawn from N(0, I) by the caller, the loss is the reverse KL estimate mean[log q(x) - log p(x)], x = f^-1(z),
 * with -log p = the closed-form potential `pot` (its gradient is evaluated in the kernel). */
int nfmc_flow_variational_fit_step_f32(const NfmcFlowFit* fit, const NfmcPotential* pot, const float* z, int64_t n,
                                       const NfmcAdamW* opt, nfmc_stream_t stream);
/* Calls first_call .. first_call + n_calls - 1 of a run (see NfmcFitControl), enqueued back to back: pot = NULL maximum
 * likelihood on rows x (n, d), else the variational fit on latents; call c uses the rows at x + (c - first_call) *
 * epoch_stride floats (0: the same rows every epoch; variational fits draw fresh latents per epoch).  AdamW's moments
 * count as zero at call 0 and `opt->step` is ignored (the device counts applied steps). */
int nfmc_flow_fit_epochs_f32(const NfmcFlowFit* fit, const NfmcPotential* pot, const float* x, int64_t n,
                             int64_t epoch_stride, const NfmcAdamW* opt, const NfmcFitControl* ctl, int32_t first_call,
                             int32_t n_calls, nfmc_stream_t stream);

/* nn.Parameters <-> trainable vector in ONE launch.  A piece is one parameter tensor, contiguous (rows, cols) floats at
 * `param`, whose element (r, c) lives at vec[vec_off + r * vec_row_stride + c * vec_col_stride] (the blob stores the first
 * conditioner layer transposed and every hidden width padded).  to_vector = 1 gathers the parameters into the vector,
 * 0 scatters the vector into them.  Replaces one slice copy per tensor of `Flow.fit`'s epilogue / prologue. */
#define NFMC_BLOB_MAX_PIECES 16
typedef struct {
    float* param;
    int64_t vec_off;
    int32_t rows, cols;
    int32_t vec_row_stride, vec_col_stride;
} NfmcBlobPiece;
int nfmc_flow_blob_copy_f32(float* vec, const NfmcBlobPiece* pieces, int32_t n_pieces, int32_t to_vector, nfmc_stream_t stream);

/* The shuffled split of the refit buffer (`train_val_split`, tuning.py:44-65: pooled rows shuffled by torch.randperm, cut
 * at train_pct, capped) without materialising a permutation of all N rows: out[i] = x[pi(first + i)], i < m, with pi a
 * keyed pseudo-random PERMUTATION of [0, N) (6-round balanced Feistel network on ceil(log2 N) bits + cycle walking, keys
 * from `seed` by splitmix64; nfmc_rows_sample_index evaluates pi on the host; oracle/shuffle.py restates it).  Rows
 * [0, a) and [a, a + b) of one permutation are what the reference's (train, validation) pair is in distribution: distinct
 * rows, uniformly placed.  `index_out` (optional, (m,) int64) receives the source rows. */
#define NFMC_PRP_ROUNDS 6
int nfmc_rows_sample_f32(const float* x, int64_t n, int32_t d, uint64_t seed, int64_t first, float* out, int64_t m,
                         int64_t* index_out, nfmc_stream_t stream);
int64_t nfmc_rows_sample_index(int64_t n, uint64_t seed, int64_t i);

typedef struct {
    int32_t abi_version;
    int32_t max_d_sampler;   /* largest d for nfmc_mala/hmc_steps */
    int32_t max_d_flow;      /* largest d for the RealNVP kernels */
    int32_t max_hidden_valu; /* H up to which the VALU conditioner path is used */
    int32_t max_hidden;      /* largest H (MFMA path) */
    int32_t max_steps_per_call;
} NfmcLimits;

int nfmc_limits(NfmcLimits* out);
const char* nfmc_error_string(int code);
/* sha256 (hex) of the sources and flags this library was built from (nfmc_amd/build.py: _digest): profiles record it
 * so that counter-derived figures can be tied to the code that was measured.  Static storage; never NULL. */
const char* nfmc_build_digest(void);

#ifdef __cplusplus
}
#endif
#endif /* NFMC_HIP_H */
