"""NeuTra HMC: HMC in the flow's latent space on U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)|
(nfmc/algorithms/sampling/nfmc/neutra.py:58-68,109-129).  The adjusted potential, its gradient (a
hand-written VJP through the coupling stack), the leapfrog integrator and the accept step run inside
`nfmc_neutra_hmc_steps_f32`.  NeuTra MH (neutra.py:147-159): the random-walk proposal, the flow inverse, the potential
value and the accept step run inside `nfmc_neutra_mh_steps_f32`.

Like the reference, the stored samples and the running moments are those of the LATENT state z: the
`data_transform` assigned at neutra.py:122 never reaches the moments;
`NeuTraParameters.transform_output=True` opts into x-space samples/moments instead.
"""
import ctypes as C
import os
import time
from dataclasses import dataclass
from typing import Optional, Type

import torch
from tqdm import tqdm

from .. import hip
from ..containers import MCMCOutput, NFMCKernel, NFMCParameters, Sampler
from ..potentials import (DiffusionBridge, FullRankGaussian, Funnel, LatticePhi4, ParticleSystem, QuadraticPotential,
                          Rosenbrock, StochasticVolatility, VaryingEffectsRegression)
from .common import Run, imd_tensor, launch_limit, progress, resolve_target
from .mcmc import (HMC, MH, HMCKernel, HMCParameters, MHKernel, MHParameters, MetropolisKernel, MetropolisParameters,
                   MetropolisSampler, refuse_inner_trajectory)


@dataclass
class NeuTraKernel(NFMCKernel):
    pass


@dataclass
class NeuTraParameters(NFMCParameters):
    batch_inverse_size: int = 128
    warmup_fit_kwargs: dict = None

    def __post_init__(self):
        super().__post_init__()
        if self.warmup_fit_kwargs is None:
            self.warmup_fit_kwargs = {
                'early_stopping': True,
                'early_stopping_threshold': 5000,
                'keep_best_weights': True,
                'n_samples': 1,
                'n_epochs': 50000,
                'lr': 0.05
            }


# The potentials whose NeuTra-MH transitions run on nfmc_neutra_mh_steps_f32: those measured no slower there than on the
# split path at 65536 and at 1024 chains (tools/probe_neutra_mh.py --kinds).  The kernel evaluates
# every neutra_valu kind, but SparseLogisticRegression, ItemResponseTheory, LatentGaussianModel and LatentGMRF walk their
# observations (or a dense covariance) once per chain and lane there, while the split path evaluates the same potential
# data-parallel over chains x observations from torch: 1.5 to 9 times faster, so those kinds stay split.
MH_KERNEL_KINDS = (QuadraticPotential, Funnel, FullRankGaussian, Rosenbrock, StochasticVolatility, LatticePhi4,
                   VaryingEffectsRegression, ParticleSystem, DiffusionBridge)


class NeuTra(Sampler):
    def __init__(self, event_shape, target, inner_sampler_class: Type[MetropolisSampler],
                 inner_kernel: MetropolisKernel, inner_params: MetropolisParameters,
                 kernel: NeuTraKernel = None, params: NeuTraParameters = None):
        if kernel is None:
            kernel = NeuTraKernel(event_shape)
        if params is None:
            params = NeuTraParameters()
        super().__init__(event_shape, target, kernel, params)
        inner_params.n_iterations = self.params.n_iterations
        self.inner_sampler = inner_sampler_class(event_shape, self.adjusted_target, inner_kernel, inner_params)
        self.inner_sampler.fuse = False  # adjusted_target is a Python closure; the fused route is sample() below
        self.mh_kernel_kinds = MH_KERNEL_KINDS   # tools/probe_neutra_mh.py widens it to time the other kinds on the kernel
        self._grad_kernel_ok = True

    def adjusted_target(self, _z, return_data: bool = False):
        """neutra.py:58-68 through the flow's API (split path and external callers)."""
        n = _z.shape[0]
        dev = hip.require_gpu()
        grad_needed = torch.is_grad_enabled() and _z.requires_grad
        if grad_needed and self._grad_kernel_ok and self._closed_form() is not None and self._flow_on_kernels():
            try:
                return _AdjustedPotential.apply(_z, self)
            except hip.NfmcArgumentError as e:
                if not e.no_kernel:
                    raise
                self._grad_kernel_ok = False   # e.g. d > ~200 (three wave tiles exceed the LDS), H > 32 off the MFMA shapes, wide spline conditioners
        if grad_needed:
            # shapes without a reverse-sweep kernel: differentiate the torch restatement of the
            # flow (on the GPU; the target is the user's callable)
            from ..flow_training import inverse_torch
            flow = self.kernel.flow
            if flow.get_device() != dev:
                flow.to(dev)
            x, log_det_inverse = inverse_torch(flow.bijection, _z.to(dev, torch.float32))
            x = x.reshape(n, *self.event_shape)
            adjusted_potential = self.target(x).reshape(-1) - log_det_inverse.reshape(-1)
            return (adjusted_potential, x) if return_data else adjusted_potential
        x, log_det_inverse = self.kernel.flow.bijection.inverse(_z)
        log_prob = -self.target(x)
        adjusted_potential = -(log_prob.reshape(-1) + log_det_inverse.to(log_prob).reshape(-1))
        return (adjusted_potential, x) if return_data else adjusted_potential

    def _flow_on_kernels(self):
        bij = getattr(self.kernel.flow, 'bijection', None)
        return hasattr(bij, 'packed') and not bij.beyond_kernels()

    def _min_hidden(self):
        """Conditioner width to present to the kernels: d = 64 / 128 with one or two hidden layers runs on the
        matrix cores (csrc/neutra_mfma.hip) also when the flow's own conditioner is narrow (zero-padded).  The matrix-core
        kernels evaluate quadratic and funnel targets only: a potential class that says so (`neutra_matrix_cores = False`,
        nfmc_amd/potentials/) keeps the flow's own width (VALU kernels).  The question goes to the target as given, not to
        its resolved descriptor: a plain callable that is recognised as a quadratic takes the matrix cores."""
        if not getattr(self.target, 'neutra_matrix_cores', True):
            return 0
        bij = self.kernel.flow.bijection
        ok = (getattr(bij, 'd', 0) in (64, 128) and getattr(bij, 'n_hidden_layers', 0) in (1, 2)
              and not getattr(bij, 'n_bins', 0) and os.environ.get('NFMC_NEUTRA_VALU', '0') != '1')
        return 64 if ok else 0

    def _closed_form(self):
        """The target as a closed-form potential descriptor (None: an arbitrary callable, differentiated by autograd)."""
        if getattr(self, '_pot_cache', None) is None or self._pot_cache[0] is not self.target:
            self._pot_cache = (self.target, resolve_target(self.target, self.event_shape, self.fuse, family='neutra'))
        return self._pot_cache[1]

    def _potential_grad(self, z):
        """U~(z), grad U~(z) from nfmc_neutra_potential_grad_f32 (closed-form targets only)."""
        dev = hip.require_gpu()
        n = z.shape[0]
        pot = self._closed_form()
        if pot is None:
            raise ValueError('NeuTra needs a closed-form potential (nfmc_amd.potentials) for the gradient kernel')
        zf = z.detach().to(dev, torch.float32).reshape(n, -1).contiguous()
        st, _keep = self.kernel.flow.bijection.packed(dev, self._min_hidden())
        pd = pot.descriptor(dev)
        u = torch.empty(n, dtype=torch.float32, device=dev)
        g = torch.empty_like(zf)
        hip.check(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(pd), hip.ptr(zf), n, hip.ptr(u),
                                                           hip.ptr(g), hip.stream()), 'nfmc_neutra_potential_grad_f32')
        return u, g.reshape(z.shape)

    def warmup(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        """neutra.py:70-107: variational fit, then tune the inner sampler."""
        refuse_inner_trajectory(self.inner_sampler, type(self).__name__)
        fit_limit = 0.3 * time_limit_seconds if time_limit_seconds is not None else None
        t0 = time.time()
        from .imh import _accepts_potential
        pot = resolve_target(self.target, tuple(x0.shape[1:]), getattr(self, 'fuse', 'auto'), x0, family='fit')
        extra = {'potential': pot} if pot is not None and _accepts_potential(self.kernel.flow) else {}
        self.kernel.flow.variational_fit(lambda v: -self.target(v),
                                         **{**dict(time_limit_seconds=fit_limit), **self.params.warmup_fit_kwargs},
                                         show_progress=show_progress, **extra)
        inner_limit = time_limit_seconds - (time.time() - t0) if time_limit_seconds is not None else None
        self.inner_sampler.params.tuning_mode()
        self.inner_sampler.params.store_samples = self.params.store_samples
        self.inner_sampler.params.n_warmup_iterations = self.params.n_warmup_iterations
        return self.inner_sampler.warmup(x0, show_progress=show_progress, time_limit_seconds=inner_limit)

    def sample(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        """neutra.py:109-129 on the device."""
        inner = self.inner_sampler
        refuse_inner_trajectory(inner, type(self).__name__)
        inner.params.n_iterations = self.params.n_iterations
        inner.params.sampling_mode()
        inner.params.store_samples = self.params.store_samples
        inner.params.thinning = getattr(self.params, 'thinning', 1)
        inner.params.max_samples = getattr(self.params, 'max_samples', None)
        run = Run(self, x0)
        pot = resolve_target(self.target, run.event_shape, self.fuse, family='neutra')

        def split():
            # arbitrary targets / shapes without a fused kernel: the inner sampler's split path on the
            # adjusted target (neutra.py:116-127)
            inner.seed, inner.shard, inner.replay = self.seed, self.shard, self.replay
            inner.rng_rounds = self.rng_rounds
            # a closed-form target on the gradient kernel is a deterministic function of z: the split path's HMC evaluates
            # the adjusted target once per position (a user's callable keeps the reference's 2 L + 2 calls per trajectory)
            inner.one_evaluation_per_position = pot is not None and self._grad_kernel_ok and self._flow_on_kernels()
            out = inner.sample(x0, show_progress=show_progress, time_limit_seconds=time_limit_seconds)
            out.kernel.flow = self.kernel.flow
            return out

        if isinstance(inner, MH) and self._mh_on_kernel(pot, run.rounds):
            return self._sample_mh(run, pot, split, show_progress, time_limit_seconds)
        if not isinstance(inner, HMC) or pot is None or not self._flow_on_kernels():
            return split()
        return self._kernel_route(run, pot, split, show_progress, time_limit_seconds, struct=hip.NfmcNeutraHmcArgs,
                                  entry='nfmc_neutra_hmc_steps_f32', label='neutra_hmc_steps', desc='NeuTra HMC',
                                  hidden=self._min_hidden(), scratch=True,
                                  own=(('n_leapfrog', int(inner.kernel.n_leapfrog_steps)),
                                       ('step_size', float(inner.kernel.step_size))))

    def _mh_on_kernel(self, pot, rounds):
        """Whether a run with an MH inner sampler goes to nfmc_neutra_mh_steps_f32: a closed-form potential of the NeuTra
        family whose kind was measured no slower on the kernel (`mh_kernel_kinds`), a flow the kernels take, the default
        Philox rounds and the flow's own conditioner at most 32 wide (there is no matrix-core MH kernel, so the padding
        of `_min_hidden` is not borrowed).  Everything else keeps the inner sampler's split path."""
        return (pot is not None and isinstance(pot, self.mh_kernel_kinds) and self._flow_on_kernels() and rounds == 10
                and int(self.kernel.flow.bijection.n_hidden) <= 32)

    def _sample_mh(self, run, pot, split, show_progress, time_limit_seconds):
        """neutra.py:147-159 with mh.py:44-73 on the device: proposal, flow inverse, potential value, Metropolis test,
        statistics and sample store of up to MAX_STEPS_PER_CALL transitions in one launch of neutra_mh_kernel, on the
        flow's own width (the kernel is a VALU one)."""
        return self._kernel_route(run, pot, split, show_progress, time_limit_seconds, struct=hip.NfmcNeutraMhArgs,
                                  entry='nfmc_neutra_mh_steps_f32', label='neutra_mh_steps', desc='NeuTra MH', hidden=0)

    def _kernel_route(self, run, pot, split, show_progress, time_limit_seconds, *, struct, entry, label, desc, hidden,
                      own=(), scratch=False):
        """A run on one of the NeuTra kernels: launches of `entry` on a `struct` until n_iterations transitions are done
        or the time is up, then the counts and the finish.  `label` names the launch for kernel timing, `desc` the
        progress bar; `hidden`: the conditioner width the flow is packed to; `own`: (field, value) pairs of the struct
        beside the shared fields; `scratch`: the entry point takes a work area (nfmc_neutra_scratch_bytes)."""
        inner = self.inner_sampler
        n = run.n
        out = MCMCOutput(run.event_shape, kernel=inner.kernel, store_samples=self.params.store_samples,
                         max_samples=getattr(self.params, 'max_samples', None))
        T = int(self.params.n_iterations)
        store = run.sample_store(T)
        # the struct borrows the packed flow, the mass diagonal and the work area: referenced here until the run's end
        st_flow, _keep = self.kernel.flow.bijection.packed(run.dev, hidden)
        imd = imd_tensor(inner.kernel, run.dev)
        if scratch:
            sbytes = int(hip.lib().nfmc_neutra_scratch_bytes(n, run.d, max(self.kernel.flow.bijection.n_hidden, hidden),
                                                             int(st_flow.n_hidden_layers), int(st_flow.n_coupling)))
            work = torch.empty(max(sbytes // 4, 1), dtype=torch.float32, device=run.dev)
            own = (*own, ('scratch', hip.ptr(work)), ('scratch_bytes', sbytes))
            if os.environ.get('NFMC_KEEP_SCRATCH'):   # diagnostics only (tools/trace_c4.py reads the marks of a trace build from its tail)
                self._scratch = work
        steps = getattr(hip.lib(), entry)
        t0 = time.time()
        bar = progress(show_progress, total=T, desc=desc)
        for done, k in run.launches(T, launch_limit(4, show_progress, time_limit_seconds), t0, time_limit_seconds, bar):
            a = struct()
            a.z, a.n, a.n_steps = hip.ptr(run.x), n, k
            a.adjust = 1 if inner.params.adjustment else 0
            a.inv_mass_diag = hip.ptr(imd)
            a.flow = st_flow
            a.pot = pot.descriptor(run.dev)
            for field, value in own:
                setattr(a, field, value)
            a.rng = run.rng(done, k, adjusted=inner.params.adjustment)
            a.stats = run.stats.struct()
            seen_before = store.seen if store is not None else 0
            a.samples = hip.store_struct(store, k)
            try:
                with run.timed(label):
                    hip.check(steps(C.byref(a), hip.stream()), entry)
            except hip.NfmcArgumentError as e:
                # validation precedes every launch, so nothing has run: the store forgets the offer, and a first launch that
                # found no kernel hands the run to the split path.  Only on the default Philox rounds: the split path must
                # not silently answer for the other stream (the MH route is entered at 10 rounds only)
                if store is not None:
                    store.seen = seen_before
                if done == 0 and e.no_kernel and run.rounds == 10:
                    bar.close()
                    return split()
                raise
        calls, grads = inner._counts(n, run.done)
        run.finish(out, t0, n * run.done, store, n_target_calls=calls, n_target_gradient_calls=grads)
        out.kernel.flow = self.kernel.flow  # neutra.py:128
        return out


class _AdjustedPotential(torch.autograd.Function):
    """Autograd view of the HIP adjusted-potential kernel, so `torch.autograd.grad(adjusted_target(z))`
    (hmc.py:40-48) works for external callers."""

    @staticmethod
    def forward(ctx, z, sampler):
        u, g = sampler._potential_grad(z)
        ctx.save_for_backward(g)
        return u

    @staticmethod
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        return grad_out.reshape(-1, *([1] * (g.dim() - 1))) * g, None


class NeuTraHMC(NeuTra):
    def __init__(self, event_shape, target, inner_kernel: HMCKernel = None, inner_params: HMCParameters = None,
                 kernel: NeuTraKernel = None, params: NeuTraParameters = None):
        if inner_kernel is None:
            inner_kernel = HMCKernel(event_size=int(torch.prod(torch.as_tensor(event_shape))))
        if inner_params is None:
            inner_params = HMCParameters()
        super().__init__(event_shape, target, HMC, inner_kernel, inner_params, kernel, params)


class NeuTraMH(NeuTra):
    """neutra.py:147-159: random-walk MH in latent space.  With a closed-form potential of the NeuTra family that is no
    slower on the kernel than on the split path (MH_KERNEL_KINDS), a flow on
    the kernels whose conditioner is at most 32 wide and the default Philox rounds, `sample` runs whole chunks of
    transitions (proposal, flow inverse, potential value, Metropolis test, statistics, sample store) inside
    `nfmc_neutra_mh_steps_f32`; every other run, and the warmup that tunes the inverse mass diagonal, goes through the
    inner sampler's split path on `adjusted_target`."""

    def __init__(self, event_shape, target, inner_kernel: MHKernel = None, inner_params: MHParameters = None,
                 kernel: NeuTraKernel = None, params: NeuTraParameters = None):
        if inner_kernel is None:
            inner_kernel = MHKernel(event_size=int(torch.prod(torch.as_tensor(event_shape))))
        if inner_params is None:
            inner_params = MHParameters()
        super().__init__(event_shape, target, MH, inner_kernel, inner_params, kernel, params)
