"""Inner MCMC samplers: Langevin (MALA/ULA) and HMC/UHMC, with the reference's kernel/parameter
dataclasses (nfmc/algorithms/sampling/mcmc/{base,langevin,hmc}.py).

`sample()` runs all `n_iterations` transitions inside HIP kernels (nfmc_mala_steps_f32 /
nfmc_hmc_steps_f32) when the target is a closed-form potential; `propose()` -- the reference's plug-in
seam (mcmc/base.py:27-34) -- stays callable and serves arbitrary Python targets: U and grad U come from
torch autograd on the GPU, proposal / log-ratio / accept-select / moments from the HIP kernels.
"""
import ctypes as C
import math
import os
import time
from copy import deepcopy
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple, Union

import torch
from tqdm import tqdm

from .. import hip
from ..containers import MCMCKernel, MCMCOutput, MCMCParameters, Sampler
from ..tuning import DualAveraging, DualAveragingParams, TrajectoryAdaptationParams
from .common import Run, accept_select, imd_tensor, launch_limit, progress, resolve_target


def inv_mass_diag_of(value, event_size):
    """A kernel dataclass's inv_mass_diag: ones by default, else `value` (lists / fp64 / any device) as (event_size,) fp32."""
    if value is None:
        return torch.ones(event_size)
    value = torch.as_tensor(value, dtype=torch.float32)
    if tuple(value.shape) != (event_size,):
        raise ValueError('inv_mass_diag must have event_size = %d entries, got shape %s' % (event_size, tuple(value.shape)))
    return value


@dataclass
class MetropolisKernel(MCMCKernel):
    event_size: int
    inv_mass_diag: torch.Tensor = None
    step_size: float = 0.01
    da: DualAveraging = None
    da_params: DualAveragingParams = None

    def __post_init__(self):
        super().__post_init__()
        self.inv_mass_diag = inv_mass_diag_of(self.inv_mass_diag, self.event_size)
        if self.da_params is None:
            self.da_params = DualAveragingParams()
        if self.da is None:
            self.da = DualAveraging(self.step_size, self.da_params)


@dataclass
class MetropolisParameters(MCMCParameters):
    tune_inv_mass_diag: bool = True
    tune_step_size: bool = True
    adjustment: bool = True
    imd_adjustment: float = 1e-3
    # warmup on the device: transitions per controller update.  1 = the reference's schedule (mcmc/base.py:92-96: the
    # kernel is updated after every transition); K > 1 updates once per K transitions with the acceptance rate and the
    # per-coordinate variance pooled over them (the n K states of the K transitions, unbiased variance), K transitions per
    # launch.  A warmup of W transitions makes ceil(W / K) updates, the last one over the W mod K transitions left, however
    # the warmup is cut into calls (progress bar, time limit).  At most 512 (hip.MAX_STEPS_PER_CALL): larger is a ValueError
    tune_every: int = 1


def tuning_state(run, kernel, words):
    """What the device controllers of a warmup start from: `words` fp64 state words on the host, zero but for the shift of
    the variance sums -- the column means of x0 (fp32 values), moved to the folded mean by every update -- and the
    kernel's inv_mass_diag cloned on the device, where the controller rewrites it."""
    st = torch.zeros(int(words), dtype=torch.float64)
    c0 = hip.tune_shift_offset(run.d)
    st[c0:c0 + run.d] = run.x.double().mean(0).float().double()
    return st, kernel.inv_mass_diag.detach().to(run.dev, torch.float32).contiguous().clone()


class DeviceTuning:
    """Step size, mass diagonal and dual-averaging state in device memory for the length of a warmup (NfmcTune,
    include/nfmc_hip.h): the controller (mcmc/base.py:142-161, tuning.py:15-41) runs inside each call's statistics fold
    and the next call reads what it wrote, so the warmup loop never waits for the GPU."""

    def __init__(self, sampler, run, trajectory=hip.TRAJECTORY_OFF):
        """trajectory: NfmcTune.trajectory of the launches (hmc).  TRAJECTORY_ADAPT: the state carries the trajectory block
        with one history row per expected controller update; TRAJECTORY_FROZEN: the block alone, the length held."""
        k, p, da = sampler.kernel, sampler.params, sampler.kernel.da
        self.trajectory = int(trajectory)
        base = int(hip.lib().nfmc_tune_state_doubles(run.d))
        self.trajectory_offset, self.history_rows = base, 0
        if self.trajectory:
            if self.trajectory == hip.TRAJECTORY_ADAPT:
                every = max(1, int(getattr(p, 'tune_every', 1)))
                self.history_rows = -(-int(p.n_iterations) // every)
            base += int(hip.lib().nfmc_tune_trajectory_doubles(self.history_rows))
        st, self.imd = tuning_state(run, k, base)
        if self.trajectory:
            ap = getattr(p, 'trajectory_adaptation', None) or TrajectoryAdaptationParams()
            length = k.trajectory_length
            if length is None:
                length = int(k.n_leapfrog_steps) * float(k.step_size)
            tr = st[self.trajectory_offset:]
            tr[hip.TRAJ_LENGTH] = float(length)
            tr[hip.TRAJ_LOG_LENGTH] = tr[hip.TRAJ_LOG_AVERAGED] = math.log(float(length))
            tr[hip.TRAJ_LEARNING_RATE], tr[hip.TRAJ_BETA2], tr[hip.TRAJ_CLIP] = ap.learning_rate, ap.beta2, ap.clip
            tr[hip.TRAJ_MAX_LEAPFROG] = int(getattr(p, 'max_leapfrog_steps', 128))
            tr[hip.TRAJ_HISTORY_ROWS] = self.history_rows
        st[hip.TUNE_STEP_SIZE] = float(k.step_size)
        st[hip.TUNE_LOG_SMOOTH] = da.log_smooth
        st[hip.TUNE_ERROR_SUM] = da.error_sum
        st[hip.TUNE_ITERATION] = da.iteration
        st[hip.TUNE_ANCHOR] = da.anchor
        st[hip.TUNE_LOG_RAW] = da.log_raw if math.isfinite(da.log_raw) else 0.0
        st[hip.TUNE_TARGET] = da.params.target_acceptance_rate
        st[hip.TUNE_KAPPA] = da.params.kappa
        st[hip.TUNE_GAMMA] = da.params.gamma
        st[hip.TUNE_IMD_ADJUSTMENT] = p.imd_adjustment
        self.state = st.to(run.dev)
        self.tune_step = bool(p.tuning and p.tune_step_size and p.adjustment)            # mcmc/base.py:153
        self.tune_imd = bool(p.tuning and p.tune_inv_mass_diag and run.n > 1)            # mcmc/base.py:146
        self.updates = 0

    def struct(self, every=0, n_steps=1):
        """NfmcTune for a call of n_steps transitions with one controller update per `every` of them."""
        every = int(every) if every and every < n_steps else 0
        self.updates += -(-n_steps // every) if every else 1
        return hip.NfmcTune(hip.ptr(self.state, torch.float64), hip.ptr(self.imd), int(self.tune_step), int(self.tune_imd),
                            every, self.trajectory)

    def leapfrog_total(self):
        """Leapfrog steps per chain the launches took so far (the device word; synchronises the stream)."""
        return int(round(float(self.state[self.trajectory_offset + hip.TRAJ_LEAPFROG_TOTAL].item())))

    def download(self, kernel):
        """The tuned kernel back on the host (one copy, at the end of the warmup)."""
        st = self.state.cpu()
        if self.trajectory == hip.TRAJECTORY_ADAPT and self.updates:
            tr = st[self.trajectory_offset:]
            kernel.trajectory_length = math.exp(float(tr[hip.TRAJ_LOG_AVERAGED]))
            used = min(self.history_rows, int(round(float(tr[hip.TRAJ_HISTORY_USED]))))
            kernel.trajectory_history = tr[hip.TRAJ_WORDS:hip.TRAJ_WORDS + used * hip.TRAJ_ROW_WORDS].reshape(
                used, hip.TRAJ_ROW_WORDS).clone()
        if self.tune_imd:
            kernel.inv_mass_diag = self.imd.cpu().to(kernel.inv_mass_diag.dtype)
        if self.tune_step and self.updates:
            da = kernel.da
            da.log_smooth, da.error_sum = float(st[hip.TUNE_LOG_SMOOTH]), float(st[hip.TUNE_ERROR_SUM])
            da.iteration, da.log_raw = int(round(float(st[hip.TUNE_ITERATION]))), float(st[hip.TUNE_LOG_RAW])
            kernel.step_size = float(st[hip.TUNE_STEP_SIZE])


@dataclass
class LangevinKernel(MetropolisKernel):
    event_size: int
    step_size: Optional[float] = None

    def __post_init__(self):
        if self.step_size is None:
            self.step_size = self.event_size ** (-1 / 3)  # langevin.py:16-18
        super().__post_init__()

    def __repr__(self):
        return (f'log step: {math.log(self.step_size):.2f}, '
                f'mass norm: {torch.max(torch.abs(self.inv_mass_diag)):.2f}')


@dataclass
class LangevinParameters(MetropolisParameters):
    pass


@dataclass
class HMCKernel(MetropolisKernel):
    event_size: int
    n_leapfrog_steps: int = 20
    # Set (by a warmup with `tune_trajectory_length`, or by hand): sampling runs jittered trajectories of this mean
    # length, L = clamp(ceil(u T / h), 1, max_leapfrog_steps) per transition, and ignores n_leapfrog_steps
    trajectory_length: float = None
    # (updates, hip.TRAJ_ROW_WORDS) fp64: one row per controller update of the last adaptive warmup (DeviceTuning.download)
    trajectory_history: Any = None

    def __repr__(self):
        if self.trajectory_length is not None:
            steps = f'trajectory: {self.trajectory_length:.3g} (jittered; n_leapfrog_steps = {self.n_leapfrog_steps} ignored)'
        else:
            steps = f'leapfrogs: {self.n_leapfrog_steps}'
        return (f'log step: {math.log(self.step_size):.2f}, '
                f'{steps}, '
                f'mass norm: {torch.max(torch.abs(self.inv_mass_diag)):.2f}')


@dataclass
class HMCParameters(MetropolisParameters):
    # warmup adapts the trajectory length T on the device (ChEES-HMC; tuning.TrajectoryAdaptation) and leaves its iterate
    # average in kernel.trajectory_length
    tune_trajectory_length: bool = False
    max_leapfrog_steps: int = 128
    trajectory_adaptation: TrajectoryAdaptationParams = None


def refuse_inner_trajectory(inner, outer):
    """Jump samplers and NeuTra run their inner hmc at a fixed leapfrog count: the jittered trajectory is not built there."""
    if getattr(inner.params, 'tune_trajectory_length', False) or getattr(inner.kernel, 'trajectory_length', None) is not None:
        raise ValueError('%s: the inner hmc kernel runs a fixed number of leapfrog steps; tune_trajectory_length / '
                         'trajectory_length are supported by the plain hmc sampler only' % outer)


class TargetFailure(Exception):
    """The target raised ValueError: the reference's failure channel (langevin.py:111-114, hmc.py:117-120,
    mh.py:63-66): every chain rejects this step and the step counts as ONE divergence."""


def _guarded(fn, *args):
    """Call into user code (`target`, autograd through it).  A ValueError from there becomes TargetFailure; the
    library's own argument errors (hip.NfmcArgumentError, also a ValueError) are never swallowed."""
    try:
        return fn(*args)
    except hip.NfmcArgumentError:
        raise
    except ValueError as e:
        raise TargetFailure(str(e)) from e


def _value_and_grad(target, x, event_shape):
    """U(x), grad U(x) by autograd on the GPU (the reference's recipe, langevin.py:66-70)."""
    with torch.enable_grad():
        xr = x.detach().reshape(x.shape[0], *event_shape).clone().requires_grad_(True)
        u = target(xr)
        g, = torch.autograd.grad(u.sum(), xr)
    return u.detach().reshape(-1).float().contiguous(), g.detach().reshape(x.shape).float().contiguous()


class MCMCSampler(Sampler):

    def __init__(self, event_shape, target, kernel: MCMCKernel, params: MCMCParameters,
                 data_transform=lambda v: v):
        super().__init__(event_shape, target, kernel, params)
        self.data_transform = data_transform

    @property
    def name(self):
        return "Generic MCMC"

    def propose(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int, int, int]:
        raise NotImplementedError

    def update_kernel(self, data: Dict[str, Any]):
        raise NotImplementedError

    # ---- fused launch of k transitions; implemented by Langevin / HMC
    def _launch(self, run: Run, pot, k, step0, samples, masks_out=None, log_ratio_out=None, jump=None, rng=None, tune=None):
        raise NotImplementedError

    def _counts(self, n, k):
        raise NotImplementedError

    def _trajectory_mode(self, run, pot):
        """NfmcTune.trajectory of this run's launches (hmc); raises ValueError before any launch where the mode cannot run."""
        return hip.TRAJECTORY_OFF

    def warmup(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        # mcmc/base.py:39-54
        with torch.no_grad():
            warmup_copy = deepcopy(self)
        warmup_copy.params.tuning_mode()
        warmup_copy.params.n_iterations = self.params.n_warmup_iterations
        out = warmup_copy.sample(x0, show_progress=show_progress, time_limit_seconds=time_limit_seconds)
        self.kernel = warmup_copy.kernel
        new_params = warmup_copy.params
        new_params.n_iterations = self.params.n_iterations
        self.params = new_params
        self.params.sampling_mode()
        self._after_warmup(warmup_copy)
        return out

    def _after_warmup(self, warmup_copy):
        """What a warmup hands the sampling run beside its kernel and parameters (mclmc: the velocity)."""

    # ---- what the sample() bodies share
    def _refuse(self, run):
        """Raises ValueError where this sampler cannot run `run`; called before anything else is set up."""

    def _begin(self, x0, show_progress):
        """The prologue of sample(): (run, step0, out, K, pot, store, t0, bar)."""
        run = Run(self, x0)
        self._refuse(run)
        # a warmup draws from its own part of the Philox stream: with an explicit seed, the sampling run that follows
        # it must not reuse the innovations that produced its starting state
        step0 = hip.WARMUP_STEP0 if self.params.tuning else 0
        out = MCMCOutput(run.event_shape, kernel=self.kernel, store_samples=self.params.store_samples,
                         max_samples=getattr(self.params, 'max_samples', None))
        out.statistics.data_transform = self.data_transform
        K = int(self.params.n_iterations)
        pot = resolve_target(self.target, run.event_shape, self.fuse, run.x, family='mcmc')
        store = run.sample_store(K)
        run.stats.zero_()
        self._n_divergences = 0
        t0 = time.time()
        label = f'{self.name} (tuning)' if self.params.tuning else self.name
        return run, step0, out, K, pot, store, t0, progress(show_progress, total=K, desc=label)

    @staticmethod
    def _pool_limit(every, show_progress, time_limit_seconds):
        """Transitions per call of a device warmup with one controller update per `every` of them: calls of whole pools,
        so that the controller updates once per `every` transitions whatever the call size."""
        limit = launch_limit(max(32, every), show_progress, time_limit_seconds)
        return limit - limit % every

    def _common_args(self, a, run, pot, k, step0, samples, rows, adjusted, rng=None, tune=None, **deferred):
        """The fields every fused sampler's args struct has, for a launch of k transitions that offers `rows` states.
        `deferred`: the DeviceStats.struct arguments of a launch whose statistics are folded later (none: by the call)."""
        a.x, a.n, a.d, a.n_steps, a.step_size = hip.ptr(run.x), run.n, run.d, k, float(self.kernel.step_size)
        a._keep = tune.imd if tune is not None else imd_tensor(self.kernel, run.dev)   # borrowed until the launch is enqueued
        a.inv_mass_diag = hip.ptr(a._keep)
        a.pot = pot.descriptor(run.dev)
        # `rng`: an NfmcRng prepared by the caller (replay bookkeeping of fused jump tails)
        a.rng = rng if rng is not None else run.rng(step0, k, adjusted=adjusted)
        a.stats = run.stats.struct(**deferred)
        a.samples = hip.store_struct(samples, rows)

    def _end(self, run, out, t0, store, tune, **counters):
        """The tail of sample(): the run's results into `out`, then the tuned kernel back from the device."""
        run.finish(out, t0, run.n * run.done, store, **counters)
        if tune is not None:
            # tuning launches fold their statistics per call: the controller state was final before the finish
            tune.download(self.kernel)
        self._cur_run = None
        return out

    def sample(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        """mcmc/base.py:56-102 on the device."""
        if self.params.tuning and int(getattr(self.params, 'tune_every', 1)) > hip.MAX_STEPS_PER_CALL:
            raise ValueError('tune_every must be at most %d, got %d'
                             % (hip.MAX_STEPS_PER_CALL, int(self.params.tune_every)))
        run, step0, out, K, pot, store, t0, bar = self._begin(x0, show_progress)
        n, event_shape = run.n, run.event_shape
        stepwise = self.params.tuning or pot is None
        limit = 1 if stepwise else launch_limit(32, show_progress, time_limit_seconds)
        # warmup of a fused sampler on one GPU: kernel state and controller on the device, no host round trip per step
        # (sharded chains keep the host controller: its statistics are all-reduced over the ranks every step)
        tune = None
        trajectory = self._trajectory_mode(run, pot)
        if self.params.tuning:
            # warmup ALWAYS draws from the default Philox4x32-10 stream, whichever controller runs (device, host,
            # sharded): tuning launches use the general kernels, which carry that stream only, and a warmup must not
            # depend on where its controller lives.  `rng_rounds=7` applies to the sampling launches (documented on sample())
            run.rounds = 10
        if (self.params.tuning and pot is not None and isinstance(self, MetropolisSampler)
                and (run.shard is None or run.shard.world == 1) and os.environ.get('NFMC_TUNE_DEVICE', '1') != '0'):
            tune = DeviceTuning(self, run, trajectory)
            # one ABI call enqueues every (kernel, controller) pair of up to 512 transitions: no host work per update
            tune.every = max(1, int(getattr(self.params, 'tune_every', 1)))
            limit = self._pool_limit(tune.every, show_progress, time_limit_seconds)
        elif trajectory:
            # jittered trajectories at a frozen length: the tuning path (general kernels, per-call fold) with the tuners off
            tune = DeviceTuning(self, run, trajectory)
            tune.every = 0
            limit = launch_limit(32, show_progress, time_limit_seconds)
        for done, k in run.launches(K, limit, t0, time_limit_seconds, bar):
            if tune is not None:
                self._launch(run, pot, k, step0 + done, store, tune=tune)
            elif pot is not None:
                mask_buf = torch.empty(k, n, dtype=torch.uint8, device=run.dev) if self.params.tuning else None
                self._launch(run, pot, k, step0 + done, store, masks_out=mask_buf)
                mask = mask_buf[-1].bool() if mask_buf is not None else None
            else:
                mask = self._split_step(run, step0 + done, store)
            if self.params.tuning and tune is None:
                with torch.no_grad():
                    self.update_kernel({'x': run.x.reshape(n, *event_shape), 'mask': mask})
        # what ran: with a jittered trajectory the leapfrog steps are counted on the device, read once here
        self._leapfrog_total = tune.leapfrog_total() if tune is not None and tune.trajectory else None
        calls, grads = self._counts(n, run.done)
        return self._end(run, out, t0, store, tune, n_target_calls=calls, n_target_gradient_calls=grads,
                         n_divergences=self._n_divergences)

    def _rejected_step(self, xf, n_calls, n_grads):
        """What propose() returns when the target raised ValueError: x' = x, nobody accepts (log ratio -inf, also for
        unadjusted kernels, whose select would otherwise accept everything), one divergence; the call counters are the
        reference's, which books them after its try block whatever happened inside."""
        n = xf.shape[0]
        self._last_log_ratio = torch.full((n,), -math.inf, dtype=torch.float32, device=xf.device)
        self._last_uniforms = None
        return xf, torch.zeros(n, dtype=torch.bool, device=xf.device), n_calls, n_grads, 1

    # ---- one transition through the propose() seam (arbitrary targets)
    def _split_step(self, run: Run, step, sample_view):
        self._cur_run, self._cur_step = run, step
        x_prime, mask_or_lr, n_calls, n_grads, n_divs = self.propose(run.x)
        self._n_divergences = getattr(self, '_n_divergences', 0) + int(n_divs)
        mask = torch.empty(run.n, dtype=torch.uint8, device=run.dev)
        accept_select(run, step, x_prime, self._last_log_ratio, self._last_uniforms, hip.TAG_ACCEPT, run.stats.struct(),
                      mask_out=mask)
        run.offer_state(sample_view)
        return mask.bool()

    # ---- what the propose() bodies share.  Replay order is draw order: the normal field is taken before the first
    # target call, the uniforms only once the last one has returned, so a step whose target raised consumes none
    def _seam(self, x):
        """Start of propose(): (xf, run, rng) -- the state as (n, d) fp32 on the device, the run whose `_split_step`
        called (None: stand-alone use of the seam) and the NfmcRng of this transition on the native streams."""
        xf = x.detach().to(hip.require_gpu(), torch.float32).reshape(x.shape[0], -1).contiguous()
        run = getattr(self, '_cur_run', None)
        step = getattr(self, '_cur_step', 0)
        self._last_log_ratio = self._last_uniforms = None
        if run is None:
            return xf, None, hip.make_rng(self.seed or 0, 0, step)
        return xf, run, hip.make_rng(run.seed, run.chain_offset, step, rounds=run.rounds)

    def _seam_normals(self, xf, run, rng, native=True):
        """The transition's normal field (langevin.py:63, mh.py:50, hmc.py:100): the next replayed one, which `rng`
        then also points to, else drawn on the native noise stream -- or None with native=False, for a caller whose
        kernel draws it from `rng` itself."""
        if run is not None and run.replay is not None:
            nz, _ = run.replay.take(1, with_uniforms=False)
            rng.replay_normals = hip.ptr(nz)
            return nz[0]
        if not native:
            return None
        noise = torch.empty_like(xf)
        hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), hip.TAG_NOISE, xf.shape[0], xf.shape[1], hip.ptr(noise),
                                                    hip.stream()), 'nfmc_philox_normals_f32')
        return noise

    def _seam_accept(self, xf, run, rng, log_ratio):
        """End of an adjusted propose(), after its last target call (langevin.py:106, mh.py:59, hmc.py:112): leaves the
        log ratio, and the replayed uniforms if the run has any, to the accept-select kernel of `_split_step` and returns
        a placeholder mask; outside a run the mask is evaluated here, on the native accept stream."""
        n = xf.shape[0]
        self._last_log_ratio = log_ratio
        if run is None:
            unif = torch.empty(n, dtype=torch.float32, device=xf.device)
            hip.check(hip.lib().nfmc_philox_uniforms_f32(C.byref(rng), hip.TAG_ACCEPT, n, hip.ptr(unif), hip.stream()),
                      'nfmc_philox_uniforms_f32')
            return torch.log(unif) < log_ratio
        if run.replay is not None:
            self._last_uniforms = run.replay.take_uniforms(1)[0].contiguous()
        return torch.ones(n, dtype=torch.bool, device=xf.device)


class MetropolisSampler(MCMCSampler):
    # a fused sampler names the args struct of its entry point, the entry point and its timing label, and fills the
    # struct's fields of its own in _own_args
    _struct = _entry = _label = None

    def _own_args(self, a):
        pass

    def _args(self, run, pot, k, step0, samples, masks_out=None, log_ratio_out=None, jump=None, rng=None, tune=None,
              attempted=None):
        """NfmcMalaArgs / NfmcHmcArgs of a launch of k transitions (`attempted`: chain-transitions to book with deferred
        statistics when the struct stands for more launches than one, samplers/jump.py: launch_jump_run)."""
        a = self._struct()
        a.adjust = 1 if self.params.adjustment else 0
        self._own_args(a)
        # with a tuning state the controller rides on the per-call statistics fold
        deferred = {} if tune is not None else dict(defer=True, attempted=run.n * k if attempted is None else attempted,
                                                    jump_attempted=run.n if jump is not None else 0)
        self._common_args(a, run, pot, k, step0, samples, k + (1 if jump is not None else 0), self.params.adjustment, rng, tune,
                          **deferred)
        if tune is not None:
            a.tune = tune.struct(getattr(tune, 'every', 0), k)
        a.masks_out = hip.ptr(masks_out, torch.uint8) if masks_out is not None else None
        a.log_ratio_out = hip.ptr(log_ratio_out) if log_ratio_out is not None else None
        a.jump = C.pointer(jump) if jump is not None else None
        return a

    def _launch(self, run, pot, k, step0, samples, **kw):
        a = self._args(run, pot, k, step0, samples, **kw)
        with run.timed(self._label):
            hip.check(getattr(hip.lib(), self._entry)(C.byref(a), hip.stream()), self._entry)

    def update_kernel(self, data: Dict[str, Any]):
        """mcmc/base.py:142-161: EMA of the per-coordinate variance + dual-averaging step size.  With sharded chains
        the variance and the acceptance rate are those of ALL chains (one all-reduce of [sum x, sum x^2, n, accepted]),
        so every rank tunes the same kernel."""
        x = data['x']
        mask = data['mask']
        shard = getattr(self, 'shard', None)
        sharded = shard is not None and shard.world > 1
        n_chains = x.shape[0]
        flat = x.flatten(1, -1)
        acc_rate = None
        if sharded:
            d = flat.shape[1]
            xd = flat.double()
            pack = torch.cat([xd.sum(0), (xd * xd).sum(0),
                              xd.new_tensor([float(n_chains), float(mask.sum()) if mask is not None else 0.0])])
            shard.all_reduce_sum_(pack)
            n_all = float(pack[2 * d])
            n_chains = int(round(n_all))
            var_all = ((pack[d:2 * d] - pack[:d] ** 2 / n_all) / max(n_all - 1.0, 1.0)).float()
            acc_rate = float(pack[2 * d + 1]) / n_all
        if n_chains > 1 and self.params.tune_inv_mass_diag:
            var = (var_all if sharded else torch.var(flat, dim=0)).to(self.kernel.inv_mass_diag)
            self.kernel.inv_mass_diag = (self.params.imd_adjustment * var
                                         + (1 - self.params.imd_adjustment) * self.kernel.inv_mass_diag)
        if self.params.tune_step_size and self.params.adjustment:
            if acc_rate is None:
                acc_rate = float(torch.mean(mask.float()))
            error = self.kernel.da_params.target_acceptance_rate - acc_rate
            self.kernel.da.step(error)
            self.kernel.step_size = self.kernel.da.value


class Langevin(MetropolisSampler):
    _struct, _entry, _label = hip.NfmcMalaArgs, 'nfmc_mala_steps_f32', 'mala_steps'
    random_walk = False   # MH: the random-walk proposal of the same kernel (NfmcMalaArgs.adjust bit 1)

    def _own_args(self, a):
        if self.random_walk:
            a.adjust |= 2

    def __init__(self, event_shape, target, kernel: Optional[LangevinKernel] = None,
                 params: Optional[LangevinParameters] = None):
        if kernel is None:
            kernel = LangevinKernel(event_size=int(torch.prod(torch.as_tensor(event_shape))))
        if params is None:
            params = LangevinParameters()
        super().__init__(event_shape, target, kernel, params)

    @property
    def name(self):
        return 'LMC'

    def _counts(self, n, k):
        per = 2 * n if self.params.adjustment else n  # langevin.py:116-120
        return per * k, per * k

    def propose(self, x):
        """langevin.py:61-122 for an arbitrary target: autograd U/grad U + HIP proposal and log-ratio.
        Returns (x_prime, mask, n_calls, n_grads, n_divergences); mask is evaluated lazily by the
        accept-select kernel when called from `sample()`."""
        xf, run, rng = self._seam(x)
        n, d = xf.shape
        dev = xf.device
        h = float(self.kernel.step_size)
        imd = imd_tensor(self.kernel, dev)
        lib = hip.lib()
        # the proposal kernel draws its noise through `rng`: natively, or from the replayed field `rng` then points to,
        # which `nz` holds until the kernel is enqueued
        nz = self._seam_normals(xf, run, rng, native=False)
        per = 2 * n if self.params.adjustment else n     # langevin.py:116-120
        try:
            u, g = _guarded(_value_and_grad, self.target, xf, self.event_shape)
        except TargetFailure:
            return self._rejected_step(xf, per, per)
        x_prime = torch.empty_like(xf)
        hip.check(lib.nfmc_langevin_propose_f32(hip.ptr(xf), hip.ptr(g), hip.ptr(imd), h, n, d, C.byref(rng),
                                                hip.ptr(x_prime), hip.stream()), 'nfmc_langevin_propose_f32')
        del nz
        if not self.params.adjustment:
            return x_prime, torch.ones(n, dtype=torch.bool, device=dev), n, n, 0
        try:
            up, gp = _guarded(_value_and_grad, self.target, x_prime, self.event_shape)
        except TargetFailure:
            return self._rejected_step(xf, per, per)
        lr = torch.empty(n, dtype=torch.float32, device=dev)
        hip.check(lib.nfmc_langevin_log_ratio_f32(hip.ptr(xf), hip.ptr(x_prime), hip.ptr(u), hip.ptr(up),
                                                  hip.ptr(g), hip.ptr(gp), hip.ptr(imd), h, n, d, hip.ptr(lr),
                                                  hip.stream()), 'nfmc_langevin_log_ratio_f32')
        return x_prime, self._seam_accept(xf, run, rng, lr), 2 * n, 2 * n, 0


class MALA(Langevin):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.params.adjustment = True


class ULA(Langevin):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.params.adjustment = False


@dataclass
class MHKernel(MetropolisKernel):
    event_size: int

    def __repr__(self):
        return (f'log step: {math.log(self.step_size):.2f}, '
                f'mass norm: {torch.max(torch.abs(self.inv_mass_diag)):.2f}')


@dataclass
class MHParameters(MetropolisParameters):
    imd_adjustment: float = 1e-5

    def __post_init__(self):
        self.tune_step_size = False       # mh.py:23-25
        self.tune_inv_mass_diag = True


class MH(Langevin):
    """Random-walk Metropolis (nfmc/algorithms/sampling/mcmc/mh.py): x' = x + eps * inv_mass_diag.  Runs on the
    Langevin kernel with a random-walk proposal (NfmcMalaArgs.adjust bit 1)."""
    random_walk = True

    def __init__(self, event_shape, target, kernel: Optional[MHKernel] = None, params: Optional[MHParameters] = None):
        if kernel is None:
            kernel = MHKernel(event_size=int(torch.prod(torch.as_tensor(event_shape))))
        if params is None:
            params = MHParameters()
        MetropolisSampler.__init__(self, event_shape, target, kernel, params)

    @property
    def name(self):
        return "MH"

    def _counts(self, n, k):
        return (2 * n * k if self.params.adjustment else 0), 0   # mh.py:67-71

    def propose(self, x):
        """mh.py:44-73 for an arbitrary target (split path)."""
        xf, run, rng = self._seam(x)
        n = xf.shape[0]
        noise = self._seam_normals(xf, run, rng)
        x_prime = (xf + noise * self.kernel.inv_mass_diag.to(xf.device, torch.float32)[None]).contiguous()
        if not self.params.adjustment:
            return x_prime, torch.ones(n, dtype=torch.bool, device=xf.device), 0, 0, 0
        try:
            with torch.no_grad():
                lr = (_guarded(self.target, xf.reshape(n, *self.event_shape)).reshape(-1)
                      - _guarded(self.target, x_prime.reshape(n, *self.event_shape)).reshape(-1))
        except TargetFailure:
            return self._rejected_step(xf, 2 * n, 0)      # mh.py:63-71
        return x_prime, self._seam_accept(xf, run, rng, lr.float().contiguous()), 2 * n, 0, 0


class RandomWalk(MH):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.params.adjustment = False


class HMC(MetropolisSampler):
    _struct, _entry, _label = hip.NfmcHmcArgs, 'nfmc_hmc_steps_f32', 'hmc_steps'

    def _own_args(self, a):
        a.n_leapfrog = int(self.kernel.n_leapfrog_steps)

    def __init__(self, event_shape, target, kernel: Optional[HMCKernel] = None,
                 params: Optional[HMCParameters] = None):
        if kernel is None:
            kernel = HMCKernel(event_size=int(torch.prod(torch.as_tensor(event_shape))))
        if params is None:
            params = HMCParameters()
        super().__init__(event_shape, target, kernel, params)

    @property
    def name(self):
        return "HMC"

    def _counts(self, n, k):
        total = getattr(self, '_leapfrog_total', None)
        if total is not None:   # jittered trajectories: 2 n gradient calls per leapfrog step taken
            return 2 * n * total + (2 * n * k if self.params.adjustment else 0), 2 * n * total
        grads = 2 * self.kernel.n_leapfrog_steps * n  # hmc.py:122-125
        calls = grads + (2 * n if self.params.adjustment else 0)
        return calls * k, grads * k

    def _trajectory_mode(self, run, pot):
        p, k = self.params, self.kernel
        adapt = bool(p.tuning and getattr(p, 'tune_trajectory_length', False))
        if not adapt and getattr(k, 'trajectory_length', None) is None:
            return hip.TRAJECTORY_OFF
        what = 'tune_trajectory_length' if adapt else 'trajectory_length'
        if not p.adjustment:
            raise ValueError('%s: uhmc has no acceptance probabilities to weight the criterion with; use hmc' % what)
        if pot is None:
            raise ValueError('%s: the target takes the split path (no closed-form potential); the jittered trajectory '
                             'runs in the fused hmc kernel only' % what)
        if run.shard is not None and run.shard.world > 1:
            raise ValueError('%s: sharded chains keep the host controller, which does not adapt the trajectory length' % what)
        if os.environ.get('NFMC_TUNE_DEVICE', '1') == '0':
            raise ValueError('%s: NFMC_TUNE_DEVICE=0 selects the host controller, which does not adapt the trajectory '
                             'length' % what)
        if int(getattr(self, 'rng_rounds', 10) or 10) == 7:
            raise ValueError('%s: rng_rounds=7 runs the exact-fit kernels; the jittered trajectory runs in the general '
                             'kernels on the Philox4x32-10 stream' % what)
        if not float(k.step_size) > 0 or (k.trajectory_length is not None and not float(k.trajectory_length) > 0):
            raise ValueError('%s: step_size and trajectory_length must be positive' % what)
        if int(getattr(p, 'max_leapfrog_steps', 128)) < 1:
            raise ValueError('%s: max_leapfrog_steps must be at least 1' % what)
        return hip.TRAJECTORY_ADAPT if adapt else hip.TRAJECTORY_FROZEN

    def propose(self, x):
        """hmc.py:96-126 for an arbitrary target: leapfrog with autograd gradients on the GPU."""
        xf, run, rng = self._seam(x)
        n = xf.shape[0]
        h = float(self.kernel.step_size)
        m = self.kernel.inv_mass_diag.to(xf.device, torch.float32)
        p = self._seam_normals(xf, run, rng) * (1 / m.sqrt())
        p0 = p
        q = xf
        L = self.kernel.n_leapfrog_steps
        n_grads = 2 * L * n                                   # hmc.py:122-125
        n_calls = n_grads + (2 * n if self.params.adjustment else 0)
        # hmc.py:69,71 evaluates the gradient twice at every interior position (the second half step of one leapfrog, the
        # first of the next) and hmc.py:103-110 the target again at both ends: 2 L + 2 calls, in that order -- kept for a
        # user's callable, which may count or fail per call (tests/golden/hmc_fail_d5).  A caller that knows its target is a
        # deterministic function (NeuTra's adjusted target on the flow kernels) sets `one_evaluation_per_position`: L + 1
        # value-and-gradient calls return the same numbers (the fused kernels do the same; the reported n_calls / n_grads
        # stay the reference's formulas).
        merged = bool(getattr(self, 'one_evaluation_per_position', False))
        u0 = u1 = None
        try:
            if merged:
                u0, g = _guarded(_value_and_grad, self.target, q, self.event_shape)
                u1 = u0
                for _ in range(L):
                    p = p - h / 2 * g
                    q = q + h * (p * m)
                    u1, g = _guarded(_value_and_grad, self.target, q, self.event_shape)
                    p = p - h / 2 * g
            else:
                for _ in range(L):
                    p = p - h / 2 * _guarded(_value_and_grad, self.target, q, self.event_shape)[1]
                    q = q + h * (p * m)
                    p = p - h / 2 * _guarded(_value_and_grad, self.target, q, self.event_shape)[1]
        except TargetFailure:
            return self._rejected_step(xf, n_calls, n_grads)  # hmc.py:117-120
        if not self.params.adjustment:
            return q.contiguous(), torch.ones(n, dtype=torch.bool, device=xf.device), n_grads, n_grads, 0
        try:
            with torch.no_grad():
                if not merged:
                    u0 = _guarded(self.target, xf.reshape(n, *self.event_shape)).reshape(-1)
                    u1 = _guarded(self.target, q.reshape(n, *self.event_shape)).reshape(-1)
                h0 = u0.reshape(-1) + 0.5 * (p0 ** 2 * m).sum(-1)
                h1 = u1.reshape(-1) + 0.5 * (p ** 2 * m).sum(-1)
        except TargetFailure:
            return self._rejected_step(xf, n_calls, n_grads)
        return q.contiguous(), self._seam_accept(xf, run, rng, (h0 - h1).float().contiguous()), n_calls, n_grads, 0


class UHMC(HMC):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.params.adjustment = False


# ------------------------------------------------------------------------------------------------ mclmc
@dataclass
class MCLMCKernel(MCMCKernel):
    """Microcanonical Langevin Monte Carlo (Robnik and Seljak 2024): step size eps, decoherence length L and the
    per-coordinate scales sigma_j = sqrt(inv_mass_diag_j)."""
    event_size: int
    step_size: Optional[float] = None            # default 0.25 sqrt(d)
    decoherence_length: Optional[float] = None   # default sqrt(d)
    inv_mass_diag: torch.Tensor = None
    # (updates, hip.MCLMC_ROW_WORDS) fp64, one row per controller update of the last warmup: the eps and L it ran with, V,
    # the count of finite steps, the eps and L it left
    adaptation_history: Any = None
    # V = sum of finite dE^2 / (count d): of the last controller update after a warmup, of the whole run after sampling --
    # the bias diagnostic of an unadjusted run (the warmup steers it to MCLMCParameters.energy_variance_target)
    energy_variance: Optional[float] = None

    def __post_init__(self):
        super().__post_init__()
        d = int(self.event_size)
        if d < 2:
            raise ValueError('mclmc needs an event size of at least 2 (the velocity lives on the unit sphere of R^d), got %d' % d)
        if self.step_size is None:
            self.step_size = 0.25 * math.sqrt(d)
        if self.decoherence_length is None:
            self.decoherence_length = math.sqrt(d)
        self.inv_mass_diag = inv_mass_diag_of(self.inv_mass_diag, d)

    def __repr__(self):
        return (f'log step: {math.log(self.step_size):.2f}, decoherence length: {self.decoherence_length:.3g}, '
                f'mass norm: {torch.max(torch.abs(self.inv_mass_diag)):.2f}')


@dataclass
class MCLMCParameters(MCMCParameters):
    tune_step_size: bool = True
    tune_decoherence_length: bool = True
    tune_inv_mass_diag: bool = False
    imd_adjustment: float = 0.25
    energy_variance_target: float = 5e-4    # blackjax's default
    decoherence_factor: float = 1.0
    tune_every: int = 8                     # steps per controller update, pooled over the chains


def mclmc_kick(u, g, sigma, e, d):
    """B(e) of the mclmc step on (n, d) tensors: the velocity after a kick of length e along -sigma g and the change dK
    of the kinetic energy.  A zero force leaves u alone with dK = 0."""
    gt = sigma * g
    gn = gt.norm(dim=1)
    still = gn == 0
    safe = torch.where(still, torch.ones_like(gn), gn)
    e_hat = -gt / safe[:, None]
    ue = (u * e_hat).sum(1)
    delta = e * gn / (d - 1)
    zeta = torch.exp(-delta)
    uu = e_hat * ((1 - zeta) * (1 + zeta + ue * (1 - zeta)))[:, None] + 2 * zeta[:, None] * u
    un = uu / uu.norm(dim=1, keepdim=True)
    dk = (d - 1) * (delta - math.log(2.0) + torch.log(1 + ue + (1 - ue) * zeta * zeta))
    return torch.where(still[:, None], u, un), torch.where(still, torch.zeros_like(dk), dk)


def mclmc_refresh(u, z, eps, length, d):
    """O of the mclmc step: partial refreshment of the unit velocity with the normals z."""
    nu = math.sqrt(math.expm1(2.0 * eps / length) / d)
    w = u + nu * z
    return w / w.norm(dim=1, keepdim=True)


class MclmcTuning:
    """eps, L, the scales and the controller's words in device memory for the length of a warmup (NfmcMclmcTune,
    include/nfmc_hip.h): the controller runs behind every `tune_every` steps of a call and the next launch reads what it
    wrote, so the warmup loop never waits for the GPU."""

    def __init__(self, sampler, run, n_updates):
        k, p, lib = sampler.kernel, sampler.params, hip.lib()
        self.rows = int(n_updates)
        self.history_offset = int(lib.nfmc_tune_state_doubles(run.d))
        st, self.imd = tuning_state(run, k, lib.nfmc_mclmc_state_doubles(run.d, self.rows))
        st[hip.MCLMC_STEP_SIZE] = float(k.step_size)
        st[hip.MCLMC_DECOHERENCE_LENGTH] = float(k.decoherence_length)
        st[hip.MCLMC_TARGET] = float(p.energy_variance_target)
        st[hip.MCLMC_IMD_ADJUSTMENT] = float(p.imd_adjustment)
        st[hip.MCLMC_DECOHERENCE_FACTOR] = float(p.decoherence_factor)
        st[hip.MCLMC_HISTORY_ROWS] = self.rows
        self.state = st.to(run.dev)
        self.flags = (int(bool(p.tune_step_size)), int(bool(p.tune_decoherence_length)), int(bool(p.tune_inv_mass_diag)))
        self.every = max(1, int(p.tune_every))

    def struct(self, n_steps):
        every = self.every if self.every < n_steps else 0
        return hip.NfmcMclmcTune(hip.ptr(self.state, torch.float64), hip.ptr(self.imd), *self.flags, every)

    def download(self, kernel):
        st = self.state.cpu()
        used = min(self.rows, int(round(float(st[hip.MCLMC_HISTORY_USED]))))
        o = self.history_offset
        kernel.adaptation_history = st[o:o + used * hip.MCLMC_ROW_WORDS].reshape(used, hip.MCLMC_ROW_WORDS).clone()
        if used:
            kernel.step_size = float(st[hip.MCLMC_STEP_SIZE])
            kernel.decoherence_length = float(st[hip.MCLMC_DECOHERENCE_LENGTH])
            kernel.energy_variance = float(st[hip.MCLMC_ENERGY_VARIANCE])
            if self.flags[2]:
                kernel.inv_mass_diag = self.imd.cpu().to(kernel.inv_mass_diag.dtype)


class MCLMC(MCMCSampler):
    """Unadjusted microcanonical Langevin Monte Carlo.  A closed-form target runs nfmc_mclmc_steps_f32 (every step of a
    launch in one HIP kernel, the warmup controller on the device); any other callable runs the same step from torch ops
    on the device -- autograd gradient, the same Philox draws, the controller on the host (tuning.MicrocanonicalAdaptation):
    slow but complete.  A step costs one gradient and one value; every launch evaluates both once more at its starting
    state, which the call counters do not book."""

    def __init__(self, event_shape, target, kernel: Optional[MCLMCKernel] = None,
                 params: Optional[MCLMCParameters] = None):
        if kernel is None:
            kernel = MCLMCKernel(event_size=int(torch.prod(torch.as_tensor(event_shape))))
        if params is None:
            params = MCLMCParameters()
        super().__init__(event_shape, target, kernel, params)
        self._next_velocity = None

    @property
    def name(self):
        return 'MCLMC'

    def _after_warmup(self, warmup_copy):
        self._next_velocity = warmup_copy._last_velocity   # handed to the sampling run

    def _refuse(self, run):
        k, p = self.kernel, self.params
        if run.d < 2 or run.d != int(k.event_size):
            raise ValueError('mclmc: the chains have event size %d, the kernel %d (at least 2)' % (run.d, int(k.event_size)))
        if run.rounds == 7:
            raise ValueError('mclmc: rng_rounds=7 runs the exact-fit kernels; mclmc runs in the general kernels on the '
                             'Philox4x32-10 stream')
        if p.tuning and run.shard is not None and run.shard.world > 1:
            raise ValueError('mclmc: a sharded warmup is not supported (the controller pools the chains of one device); '
                             'warm up on one device and shard the sampling run')

    def _velocity(self, run, step0):
        """The run's unit velocities: those a warmup left, else normals of Philox stream 4 at the run's first step counter,
        normalised here."""
        u, self._next_velocity = self._next_velocity, None
        if u is not None and tuple(u.shape) == (run.n, run.d) and u.device == run.dev:
            return u.clone()
        u = torch.empty(run.n, run.d, dtype=torch.float32, device=run.dev)
        rng = hip.make_rng(run.seed, run.chain_offset, step0)
        hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), hip.TAG_VELOCITY, run.n, run.d, hip.ptr(u), hip.stream()),
                  'nfmc_philox_normals_f32')
        return (u / u.norm(dim=1, keepdim=True)).contiguous()

    def _launch_fused(self, run, pot, u, k, step0, store, esums, tune, energy_out=None):
        a = hip.NfmcMclmcArgs()
        self._common_args(a, run, pot, k, step0, store, k, False, tune=tune)
        a.velocity, a.decoherence_length = hip.ptr(u), float(self.kernel.decoherence_length)
        a.energy_out = hip.ptr(energy_out) if energy_out is not None else None
        a.energy_sums = hip.ptr(esums, torch.float64)
        if tune is not None:
            a.tune = tune.struct(k)
        with run.timed('mclmc_steps'):
            hip.check(hip.lib().nfmc_mclmc_steps_f32(C.byref(a), hip.stream()), 'nfmc_mclmc_steps_f32')

    def _torch_step(self, run, u, step, store, esums, cache, ctl):
        """One step from torch ops (targets with no closed form): returns the new velocity."""
        k = self.kernel
        n, d = run.n, run.d
        eps = float(torch.tensor(float(k.step_size), dtype=torch.float32))   # the kernels integrate with the fp32 value
        length = float(torch.tensor(float(k.decoherence_length), dtype=torch.float32))
        sigma = k.inv_mass_diag.to(run.dev, torch.float32).sqrt()[None]
        if 'g' not in cache:
            cache['U'], cache['g'] = _value_and_grad(self.target, run.x, self.event_shape)
        x, g, U = run.x, cache['g'], cache['U']
        u1, dk1 = mclmc_kick(u, g, sigma, 0.5 * eps, d)
        xn = x + eps * sigma * u1
        Un, gn = _value_and_grad(self.target, xn, self.event_shape)
        u2, dk2 = mclmc_kick(u1, gn, sigma, 0.5 * eps, d)
        de = (Un - U) + dk1 + dk2
        ok = torch.isfinite(de) & torch.isfinite(xn).all(1)
        run.x = torch.where(ok[:, None], xn, x).contiguous()
        cache['g'], cache['U'] = torch.where(ok[:, None], gn, g), torch.where(ok, Un, U)
        z = torch.empty(n, d, dtype=torch.float32, device=run.dev)
        rng = run.rng(step, 1, adjusted=False)
        if run.replay is not None:
            z = run._keep[0][0]
        else:
            hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), hip.TAG_NOISE, n, d, hip.ptr(z), hip.stream()),
                      'nfmc_philox_normals_f32')
        u = mclmc_refresh(torch.where(ok[:, None], u2, u), z, eps, length, d).contiguous()
        dee = torch.where(ok, de, torch.zeros_like(de)).double()
        esums += torch.stack([(dee * dee).sum(), dee.sum(), ok.sum().double()])
        st = run.stats.struct()
        hip.check(hip.lib().nfmc_moments_update_f32(hip.ptr(run.x), n, d, C.byref(st), hip.stream()), 'nfmc_moments_update_f32')
        run.stats._counters[hip.CNT_NONFINITE] += (~ok).sum()
        run.offer_state(store)
        if ctl is not None:
            ctl['e2'] += float((dee * dee).sum())
            ctl['count'] += float(ok.sum())
            ctl['states'].append(run.x.double())
            if len(ctl['states']) == ctl['every']:
                self._host_update(ctl)
        return u

    def _host_update(self, ctl):
        states = torch.cat(ctl['states'], 0)
        var = states.var(0, unbiased=True) if states.shape[0] > 1 else None
        ad = ctl['adaptation']
        ad.step(ctl['e2'], ctl['count'], var)
        k = self.kernel
        k.step_size, k.decoherence_length, k.energy_variance = ad.step_size, ad.decoherence_length, ad.energy_variance
        if ad.tune_inv_mass_diag:
            k.inv_mass_diag = ad.inv_mass_diag.clone()
        ctl['e2'], ctl['count'], ctl['states'] = 0.0, 0.0, []

    def sample(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        from ..tuning import MicrocanonicalAdaptation
        p, k = self.params, self.kernel
        if p.tuning and not 1 <= int(p.tune_every) <= hip.MAX_STEPS_PER_CALL:
            raise ValueError('tune_every must be in 1 .. %d, got %d' % (hip.MAX_STEPS_PER_CALL, int(p.tune_every)))
        if not (float(k.step_size) > 0 and float(k.decoherence_length) > 0):
            raise ValueError('mclmc: step_size and decoherence_length must be positive')
        run, step0, out, K, pot, store, t0, bar = self._begin(x0, show_progress)
        u = self._velocity(run, step0)
        esums = torch.zeros(3, dtype=torch.float64, device=run.dev)
        tune, ctl, cache = None, None, {}
        if pot is not None:
            limit = launch_limit(32, show_progress, time_limit_seconds)
            if p.tuning:
                tune = MclmcTuning(self, run, -(-K // max(1, int(p.tune_every))) + 1)
                limit = self._pool_limit(tune.every, show_progress, time_limit_seconds)
        else:
            limit = 1
            if p.tuning:
                ctl = {'every': max(1, int(p.tune_every)), 'e2': 0.0, 'count': 0.0, 'states': [],
                       'adaptation': MicrocanonicalAdaptation(
                           k.step_size, k.decoherence_length, k.inv_mass_diag, run.d, p.energy_variance_target,
                           p.imd_adjustment, p.decoherence_factor, p.tune_step_size, p.tune_decoherence_length,
                           p.tune_inv_mass_diag)}
        for done, kk in run.launches(K, limit, t0, time_limit_seconds, bar):
            if pot is not None:
                self._launch_fused(run, pot, u, kk, step0 + done, store, esums, tune)
            else:
                u = self._torch_step(run, u, step0 + done, store, esums, cache, ctl)
        if ctl is not None:
            if ctl['states']:
                self._host_update(ctl)   # the steps left over the last whole pool
            k.adaptation_history = torch.tensor(ctl['adaptation'].history, dtype=torch.float64).reshape(-1, hip.MCLMC_ROW_WORDS)
        steps = run.n * run.done
        self._end(run, out, t0, store, tune, n_target_calls=steps, n_target_gradient_calls=steps,
                  n_accepted_trajectories=steps, n_attempted_trajectories=steps, n_divergences=0)
        if tune is None and not p.tuning:
            s2, _, cnt = (float(v) for v in esums.cpu())
            k.energy_variance = s2 / (cnt * run.d) if cnt > 0 else math.nan
        self._last_velocity = u
        return out
