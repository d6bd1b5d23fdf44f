"""Warmup helpers next to the hot path: the step-size controller and the refit-buffer split
(what nfmc/algorithms/sampling/tuning.py provides to the samplers)."""
import math
from dataclasses import dataclass

import torch


@dataclass
class DualAveragingParams:
    """Constants of the controller; the defaults are the reference's (tuning.py:8-12)."""
    target_acceptance_rate: float = 0.651
    kappa: float = 0.75    # decay exponent of the averaging weight t^-kappa
    gamma: float = 0.05    # shrinkage towards the anchor log(10 h0)
    t0: int = 10           # iteration count the schedule starts from


class DualAveraging:
    """Nesterov dual averaging of log(step size), driven by `step(target_rate - observed_rate)`.

    State: the running sum E of the errors fed so far and the iteration count t (starting at t0).
      raw      log h_t   = log(10 h0) - E / (gamma sqrt(t))
      smoothed log hbar  <- w log h_t + (1 - w) log hbar,   w = t^-kappa
    `value` is exp(log hbar), the step size the sampler uses next (same recurrences, constants and update order
    as tuning.py:15-41: `test_mala_warmup_tuning_golden` replays the reference's tuned step sizes through it)."""

    def __init__(self, initial_step_size, params: DualAveragingParams):
        self.params = params
        self.iteration = int(params.t0)
        self.error_sum = 0.0
        self.anchor = math.log(10 * initial_step_size)
        self.log_raw = math.inf                          # no raw estimate before the first error
        self.log_smooth = math.log(initial_step_size)

    def step(self, acceptance_rate_error):
        p, t = self.params, self.iteration
        self.error_sum += float(acceptance_rate_error)
        self.log_raw = self.anchor - self.error_sum / (math.sqrt(t) * p.gamma)
        weight = t ** -p.kappa
        self.log_smooth = weight * self.log_raw + (1 - weight) * self.log_smooth
        self.iteration = t + 1

    @property
    def value(self) -> float:
        return math.exp(self.log_smooth)

    def __repr__(self):
        return 'DualAveraging(step=%.4g, error_sum=%.2f, t=%d)' % (self.value, self.error_sum, self.iteration)


@dataclass
class TrajectoryAdaptationParams:
    """Constants of the trajectory-length controller (ChEES-HMC, Hoffman, Radul and Sountsov, AISTATS 2021)."""
    learning_rate: float = 0.025
    beta2: float = 0.95    # decay of the second-moment estimate
    clip: float = 0.35     # largest move of log T per update


def radical_inverse(k: int) -> float:
    """Base-2 radical inverse of k + 1, offset by half an ulp of the 32-bit grid: (bitreverse32(k + 1) + 0.5) 2^-32, the
    jitter of the transition with Philox step counter k (1/2, 1/4, 3/4, 1/8, ... from k = 0).  Exact in fp64."""
    i = (int(k) + 1) & 0xffffffff
    return (int('{:032b}'.format(i)[::-1], 2) + 0.5) * 2.0 ** -32


def leapfrog_count(k: int, trajectory_length: float, step_size: float, max_leapfrog_steps: int = 128) -> int:
    """Leapfrog steps of the transition with step counter k: clamp(ceil(u T / h), 1, L_max) in fp64, u = radical_inverse(k).
    The same operations in the same order as the device's trajectory_leapfrog_count (csrc/sampler_impl.hpp): both sides
    agree to the integer when fed the same fp64 T and h."""
    r = math.ceil(radical_inverse(k) * float(trajectory_length) / float(step_size)) if step_size > 0 else 1
    return int(max(1, min(int(max_leapfrog_steps), r)))


class TrajectoryAdaptation:
    """Stochastic gradient ascent on log T of the ChEES criterion: Adam with beta1 = 0, driven by
    `step(g_hat, alpha_sum, step_size)` once per controller update.  With j the update count from 1:
      v        <- b2 v + (1 - b2) g_hat^2
      delta     = lr g_hat / (sqrt(v / (1 - b2^j)) + 1e-8), clipped to +-clip
      log T    <- clamp(log T + delta, log h, log(L_max h))       h: the step size the same update just set
      log Tbar <- w log T + (1 - w) log Tbar,   w = j^-0.75
    An update whose pooled weight `alpha_sum` is zero (or whose g_hat is not finite) changes nothing.  `value` is the
    length the warmup runs on, `averaged` the one handed to sampling.  The controller on the device
    (tune_finish_kernel, csrc/sampler_kernels.hip) is this recurrence on fp64 words of the trajectory block."""

    def __init__(self, initial_length, params: TrajectoryAdaptationParams = None, max_leapfrog_steps: int = 128):
        self.params = params if params is not None else TrajectoryAdaptationParams()
        self.max_leapfrog_steps = int(max_leapfrog_steps)
        self.log_length = math.log(initial_length)
        self.log_averaged = self.log_length
        self.v = 0.0
        self.count = 0

    def step(self, g_hat, alpha_sum, step_size):
        if not (alpha_sum > 0) or not math.isfinite(g_hat):
            return
        p = self.params
        j = self.count + 1
        self.v = p.beta2 * self.v + (1 - p.beta2) * g_hat * g_hat
        delta = p.learning_rate * g_hat / (math.sqrt(self.v / (1 - p.beta2 ** j)) + 1e-8)
        delta = max(-p.clip, min(p.clip, delta))
        lo = math.log(step_size)
        hi = math.log(self.max_leapfrog_steps * step_size)
        self.log_length = min(max(self.log_length + delta, lo), hi)
        w = j ** -0.75
        self.log_averaged = w * self.log_length + (1 - w) * self.log_averaged
        self.count = j

    @property
    def value(self) -> float:
        return math.exp(self.log_length)

    @property
    def averaged(self) -> float:
        return math.exp(self.log_averaged)

    def __repr__(self):
        return 'TrajectoryAdaptation(T=%.4g, averaged=%.4g, updates=%d)' % (self.value, self.averaged, self.count)


class MicrocanonicalAdaptation:
    """The warmup controller of the mclmc sampler, driven by `step(energy_sq_sum, count, variance)` once per update over
    the update's pooled steps (count of them with a finite energy error dE, energy_sq_sum the sum of their dE^2):
      V = energy_sq_sum / (count d)
      count = 0 or V not finite:   eps <- eps / 2, nothing else moves
      else   log eps <- log eps + clamp(log(target / V) / 6, -ln 2, ln 2)      (the local error is of third order in eps)
             s_j <- (1 - beta) s_j + beta v_j                                   (tune_inv_mass_diag; rounded to fp32)
             L <- factor sqrt(sum_j v_j / s_j), s_j after its own update         (tune_decoherence_length)
    v_j (`variance`, fp64): the unbiased variance of coordinate j over the update's states; None where there is one state
    or less, which leaves s and L alone.  `history` holds one row per update: the eps and L it ran with, V, count, the eps
    and L it left.  The controller on the device (mclmc_tune_finish_kernel, csrc/sampler_kernels.hip) is this recurrence
    on fp64 words."""

    def __init__(self, step_size, decoherence_length, inv_mass_diag, event_size, target=5e-4, imd_adjustment=0.25,
                 decoherence_factor=1.0, tune_step_size=True, tune_decoherence_length=True, tune_inv_mass_diag=False):
        self.step_size = float(step_size)
        self.decoherence_length = float(decoherence_length)
        self.inv_mass_diag = torch.as_tensor(inv_mass_diag, dtype=torch.float32).detach().cpu().clone()
        self.event_size = int(event_size)
        self.target, self.imd_adjustment, self.decoherence_factor = float(target), float(imd_adjustment), float(decoherence_factor)
        self.tune_step_size, self.tune_decoherence_length = bool(tune_step_size), bool(tune_decoherence_length)
        self.tune_inv_mass_diag = bool(tune_inv_mass_diag)
        self.energy_variance = None
        self.history = []

    def step(self, energy_sq_sum, count, variance=None):
        eps0, len0 = self.step_size, self.decoherence_length
        count = float(count)
        V = float(energy_sq_sum) / (count * self.event_size) if count > 0 else 0.0
        if not (count > 0 and math.isfinite(V)):
            if self.tune_step_size:
                self.step_size = 0.5 * eps0
        else:
            if self.tune_step_size:
                move = math.log(self.target / V) / 6.0 if V > 0 else math.inf
                self.step_size = math.exp(math.log(eps0) + max(-math.log(2.0), min(math.log(2.0), move)))
            if variance is not None:
                var = torch.as_tensor(variance, dtype=torch.float64).cpu().clamp(min=0.0)
                if self.tune_inv_mass_diag:
                    b = self.imd_adjustment
                    self.inv_mass_diag = ((1.0 - b) * self.inv_mass_diag.double() + b * var).float()
                if self.tune_decoherence_length:
                    nxt = self.decoherence_factor * math.sqrt(float((var / self.inv_mass_diag.double()).sum()))
                    if nxt > 0 and math.isfinite(nxt):
                        self.decoherence_length = nxt
        self.energy_variance = V
        self.history.append([eps0, len0, V, count, self.step_size, self.decoherence_length])

    def __repr__(self):
        return 'MicrocanonicalAdaptation(eps=%.4g, L=%.4g, updates=%d)' % (self.step_size, self.decoherence_length,
                                                                           len(self.history))


def _shuffled(rows: torch.Tensor) -> torch.Tensor:
    return rows[torch.randperm(rows.shape[0], device=rows.device)]


def _sampled_rows(rows: torch.Tensor, m: int) -> torch.Tensor:
    """The first m rows of a shuffle of `rows`, without materialising the shuffled buffer: on the GPU one launch of
    nfmc_rows_sample_f32 (rows pi(0 .. m - 1) of a keyed pseudo-random permutation, key from torch's CPU generator)."""
    total = rows.shape[0]
    if rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and 0 < m <= total:
        from . import hip
        flat = rows.reshape(total, -1)
        out = torch.empty(m, flat.shape[1], dtype=torch.float32, device=rows.device)
        seed = int(torch.randint(0, 2 ** 62, ()).item())
        hip.check(hip.lib().nfmc_rows_sample_f32(hip.ptr(flat), total, flat.shape[1], seed, 0, hip.ptr(out), m, None, hip.stream()),
                  'nfmc_rows_sample_f32')
        return out.reshape(m, *rows.shape[1:])
    return rows[torch.randperm(total, device=rows.device)[:m]].contiguous()


def train_val_split(x: torch.Tensor, train_pct: float, max_train_size: int, max_val_size: int, shuffle: bool = True,
                    shard=None):
    """(n_iterations, n_chains, *event) -> (x_train, x_val): all (step, chain) rows pooled, shuffled, cut at
    `train_pct` and capped (tuning.py:44-65).

    With `shard` (chains split over GPUs; collective C1 of SURVEY 8e) every rank contributes the same number of rows
    of the capped buffer, drawn from its own shuffled rows, and the shares are all-gathered.  The row count is agreed
    first (all-reduce MIN of what every rank can give: block sizes differ by one when the chain count does not divide,
    and a time limit can leave ranks with different numbers of kept steps), so the collective always sees equal
    sizes.  The gathered rows are then shuffled AGAIN with a seed broadcast from rank 0 before the `train_pct` cut:
    train and validation both mix rows of every rank (a cut in rank order would validate on the last ranks' chains
    only), and every rank fits the flow on the same rows in the same order."""
    rows = x.flatten(0, 1)
    if shard is not None and shard.world > 1:
        share = -(-(max_train_size + max_val_size) // shard.world)
        share = shard.all_reduce_min_int(min(share, rows.shape[0]))
        if share <= 0:
            raise ValueError('train_val_split: a rank has no rows to contribute to the refit buffer')
        if shuffle:
            local = _sampled_rows(rows, share)      # this rank's share: the first rows of a shuffle of its own rows
        else:
            local = rows[:share].contiguous()
        rows = shard.all_gather_rows(local)
        if shuffle:
            seed = shard.broadcast_int(int(torch.randint(0, 2 ** 62, ()).item()))
            perm = torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(seed))
            rows = rows[perm.to(rows.device)]
    elif shuffle:
        # the rows of the shuffled buffer that survive the cut and the caps, without materialising the shuffled buffer (at
        # the C5 shape it is 160 MiB per refit for 8192 kept rows)
        total = rows.shape[0]
        cut = int(train_pct * total)
        n_train, n_val = min(cut, int(max_train_size)), min(total - cut, int(max_val_size))
        if rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and total > 0 and n_train + n_val > 0:
            # ONE launch (csrc/fit_support.hip: nfmc_rows_sample_f32): rows pi(0 .. n_train + n_val - 1) of a keyed
            # pseudo-random permutation pi of the pooled rows -- positions [0, n_train) and [cut, cut + n_val) of a uniform
            # shuffle are, in distribution, any n_train + n_val distinct positions of it.  The key comes from torch's CPU
            # generator, like the reference's randperm (tuning.py:58-59); no sort of all rows, no index tensors.
            out = _sampled_rows(rows, n_train + n_val)
            return out[:n_train], out[n_train:]
        perm = torch.randperm(total, device=rows.device)
        return rows[perm[:cut][:max_train_size]], rows[perm[cut:][:max_val_size]]
    cut = int(train_pct * rows.shape[0])
    return rows[:cut][:max_train_size], rows[cut:][:max_val_size]
