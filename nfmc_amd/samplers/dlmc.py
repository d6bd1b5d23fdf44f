"""DLMC (nfmc/algorithms/sampling/nfmc/dlmc.py): one flow refit per iteration, a gradient step on U + log q, then one
independent-MH step proposed by the flow.

On the device an iteration is three kinds of launch: the resident flow fit (`Flow.fit`, flow_training.py), the fused
gradient step `nfmc_dlmc_step_f32` (x <- x - eps (grad U + grad_x log q), csrc/dlmc_kernels.hip) and one
`nfmc_flow_mh_steps_f32` transition (flow.sample + flow.log_prob + 2 target calls + MH test + masked update + moments).
Flows and targets without a kernel compose the same transition: grad U by autograd on the GPU (borrowed by the fused
step), grad log q by autograd through `flow_training.forward_torch` (splines, conditioners wider than 8, shapes beyond
the kernels), the MH half through the flow's own kernels (`jump.split_flow_mh`).
"""
import ctypes as C
import time
from dataclasses import dataclass

import torch

from .. import hip
from ..containers import MCMCOutput, NFMCKernel, NFMCParameters, Sampler
from ..tuning import train_val_split
from .common import Run, _refit, progress, resolve_target
from .jump import flow_is_native, flow_mh_supported, launch_flow_mh, split_flow_mh


@dataclass
class DLMCKernel(NFMCKernel):
    step_size: float = 0.05   # dlmc.py:14


@dataclass
class DLMCParameters(NFMCParameters):
    latent_updates: bool = False   # dlmc.py:19


def _grad(fn, x, event_shape):
    """compute_grad (nfmc/util.py:395-402) on the GPU: grad of fn(x).sum(), as a contiguous (n, d) fp32 tensor."""
    with torch.enable_grad():
        xr = x.detach().reshape(x.shape[0], *event_shape).clone().requires_grad_(True)
        g, = torch.autograd.grad(fn(xr).sum(), xr)
    return g.detach().reshape(x.shape[0], -1).to(torch.float32).contiguous()


def _flow_struct(flow, dev):
    return flow.bijection.packed(dev)


def logq_grad_args(flow, x, grad_out=None, logq_out=None):
    """NfmcFlowLogqGradArgs for a (n, d) fp32 device tensor (+ keep-alive references)."""
    st, keep = _flow_struct(flow, x.device)
    a = hip.NfmcFlowLogqGradArgs()
    a.flow = st
    a.x, a.n = hip.ptr(x), int(x.shape[0])
    a.grad_out = hip.ptr(grad_out) if grad_out is not None else None
    a.logq_out = hip.ptr(logq_out) if logq_out is not None else None
    return a, keep


def logq_grad_supported(flow, n=1, d=None) -> bool:
    """Whether nfmc_flow_logq_grad_f32 has a kernel for this flow (nfmc_flow_logq_grad_supported_f32)."""
    if not flow_is_native(flow):
        return False
    dev = hip.require_gpu()
    x = torch.empty(1, flow.bijection.d, dtype=torch.float32, device=dev)
    a, _keep = logq_grad_args(flow, x, logq_out=torch.empty(1, dtype=torch.float32, device=dev))
    a.n = int(n)
    return hip.supported(int(hip.lib().nfmc_flow_logq_grad_supported_f32(C.byref(a))), 'nfmc_flow_logq_grad_supported_f32')


def logq_grad(flow, x):
    """(grad_x log q(x), log q(x)) of a (n, d) batch on the device kernel; NfmcArgumentError when it has none."""
    x = x.detach().to(hip.require_gpu(), torch.float32).reshape(x.shape[0], -1).contiguous()
    g = torch.empty_like(x)
    lq = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    a, _keep = logq_grad_args(flow, x, g, lq)
    hip.check(hip.lib().nfmc_flow_logq_grad_f32(C.byref(a), hip.stream()), 'nfmc_flow_logq_grad_f32')
    return g, lq


def logq_grad_torch(flow, x, event_shape):
    """The composed route: grad_x log q(x) by autograd (flow_training.forward_torch for this package's flows, on the
    device their parameters live on; the flow's own `log_prob` for a foreign flow object)."""
    from ..flows import Flow
    if isinstance(flow, Flow):
        from ..flow_training import forward_torch

        def lq(v):
            z, ld = forward_torch(flow.bijection, v)
            return Flow._base_log_prob(z) + ld
        pdev = flow.get_device()
        return _grad(lq, x.to(pdev), (x.shape[1],)).to(x.device)
    return _grad(lambda v: flow.log_prob(v), x, event_shape)


def step_args(flow, x, step_size, pot=None, grad_u=None):
    st, keep = _flow_struct(flow, x.device)
    a = hip.NfmcDlmcStepArgs()
    a.flow = st
    if pot is not None:
        a.pot = pot.descriptor(x.device)
    else:
        a.pot.kind = -1
    a.x, a.n = hip.ptr(x), int(x.shape[0])
    a.grad_u = hip.ptr(grad_u) if grad_u is not None else None
    a.logq_out = None
    a.step_size = float(step_size)
    return a, keep


def step_supported(flow, x, step_size, pot=None, grad_u=None) -> bool:
    """Whether nfmc_dlmc_step_f32 has a kernel for this flow / potential (nfmc_dlmc_step_supported_f32)."""
    if not flow_is_native(flow):
        return False
    a, _keep = step_args(flow, x, step_size, pot, grad_u if grad_u is not None else (x if pot is None else None))
    return hip.supported(int(hip.lib().nfmc_dlmc_step_supported_f32(C.byref(a))), 'nfmc_dlmc_step_supported_f32')


def launch_step(flow, x, step_size, pot=None, grad_u=None):
    """x <- x - step_size (grad U(x) + grad_x log q(x)) in place (dlmc.py:85-87); grad U in closed form from `pot`, or
    the caller's `grad_u`."""
    a, _keep = step_args(flow, x, step_size, pot, grad_u)
    hip.check(hip.lib().nfmc_dlmc_step_f32(C.byref(a), hip.stream()), 'nfmc_dlmc_step_f32')


class DLMC(Sampler):
    """dlmc.py:22-127.  A refit that diverges raises ValueError out of `sample()`, as dlmc.py:70 does, but one iteration
    later: the build's flow checks refit i when refit i + 1 starts, or when sampling ends after the last one (`defer_check`,
    as `JumpNFMC._refit`).  The gradient step and the MH step of iteration i have then already run on the weights that
    refit wrote back.  A refit that returns early (early stopping, the default, or a time limit) has been read back before
    it returns, and `sample()` raises at the next refit or at its end all the same."""

    def __init__(self, event_shape, target, negative_log_likelihood, kernel: DLMCKernel = None,
                 params: DLMCParameters = None):
        if kernel is None:
            kernel = DLMCKernel(event_shape)
        if params is None:
            params = DLMCParameters()
        super().__init__(event_shape, target, kernel, params)
        self.negative_log_likelihood = negative_log_likelihood
        self.last_route = None   # 'fused' / 'borrowed' / 'composed' (gradient step), set by sample()

    @property
    def name(self):
        return 'DLMC'

    def warmup(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        """dlmc.py:36-43: no tuning; the output holds x0 only."""
        out = MCMCOutput(event_shape=tuple(x0.shape[1:]), store_samples=self.params.store_samples)
        out.running_samples.add(x0)
        return out

    _refit = _refit

    def _grad_step(self, run, flow, pot, route):
        """x <- x - eps grad_x [U(x) + log q(x)] (dlmc.py:85-87)."""
        eps = float(self.kernel.step_size)
        es = run.event_shape
        if route == 'fused':
            with run.timed('dlmc_step'):
                launch_step(flow, run.x, eps, pot=pot)
            return
        gu = _grad(self.target, run.x, es)
        if route == 'borrowed':
            with run.timed('dlmc_step'):
                launch_step(flow, run.x, eps, grad_u=gu)
            return
        gq = logq_grad_torch(flow, run.x, es)
        run.x.sub_(eps * (gu + gq))

    def _latent_step(self, run, flow):
        """z = f(x); z <- z - eps (grad U(x) - z); x = f^-1(z)  (dlmc.py:80-84)."""
        n, es = run.n, run.event_shape
        with torch.no_grad():
            z, _ = flow.bijection.forward(run.x.reshape(n, *es))
        gu = _grad(self.target, run.x, es)
        z = z.detach().reshape(n, -1).to(torch.float32)
        z = z - float(self.kernel.step_size) * (gu - z)
        with torch.no_grad():
            x, _ = flow.bijection.inverse(z.reshape(n, *es))
        run.x.copy_(x.detach().reshape(n, -1))

    def sample(self, x0, show_progress: bool = True, time_limit_seconds=None) -> MCMCOutput:
        """dlmc.py:45-127 on the device."""
        run = Run(self, x0)
        n, es = run.n, run.event_shape
        flow = self.kernel.flow
        T = int(self.params.n_iterations)
        eps = float(self.kernel.step_size)
        pot = resolve_target(self.target, es, self.fuse, run.x, family='flow_mh')
        nll = resolve_target(self.negative_log_likelihood, es, self.fuse, run.x)
        native = flow_is_native(flow)
        store = run.sample_store(T)
        logq = torch.empty(n, dtype=torch.float32, device=run.dev)
        target_calls = grad_calls = 0

        # ---- initial update with the likelihood (dlmc.py:58-66)
        t0 = time.time()
        run.x.sub_(eps * _grad(nll if nll is not None else self.negative_log_likelihood, run.x, es))
        target_calls += n
        grad_calls += n

        route = None            # decided after the first refit (the probes need the packed weights)
        mh_fused = None
        pending_fit = None
        done = 0
        bar = progress(show_progress, range(T), desc='DLMC sampling')
        for i in bar:
            if run.time_is_up(t0, time_limit_seconds):
                break
            # ---- refit on the current state (dlmc.py:73-78)
            x_train, x_val = train_val_split(run.x.reshape(1, n, *es), train_pct=self.params.train_pct,
                                             max_train_size=self.params.max_train_size,
                                             max_val_size=self.params.max_val_size, shard=self.shard)
            if pending_fit is not None:
                pending_fit.result()
            pending_fit = self._refit(flow, x_train, x_val)
            if route is None:
                if self.params.latent_updates:
                    route = 'latent'
                elif native and pot is not None and pot.fused_in('dlmc_step') and step_supported(flow, run.x, eps, pot=pot):
                    route = 'fused'
                elif native and step_supported(flow, run.x, eps, grad_u=run.x):
                    route = 'borrowed'
                else:
                    route = 'composed'
                mh_fused = native and pot is not None and flow_mh_supported(run, flow, pot, logq, True)
                self.last_route = route
            # ---- gradient step (dlmc.py:80-92)
            if route == 'latent':
                self._latent_step(run, flow)
            else:
                self._grad_step(run, flow, pot, route)
            target_calls += n
            grad_calls += n
            # ---- independent-MH step proposed by the flow, at the post-step state (dlmc.py:93-119)
            if mh_fused:
                launch_flow_mh(run, flow, pot, logq, 1, i, False, True, run.stats.struct(defer=True, attempted=n), store)
                target_calls += 2 * n
            else:
                target_calls += split_flow_mh(run, flow, self.target, es, i, True, run.stats.struct())
                run.offer_state(store)
            done = i + 1
            if show_progress:
                run.sync()
                bar.set_postfix_str(f'acc {int(run.stats.counters[hip.CNT_ACCEPTED])}/{n * done}')
        if pending_fit is not None:
            pending_fit.result()
        out = MCMCOutput(es, kernel=self.kernel, store_samples=self.params.store_samples,
                         max_samples=getattr(self.params, 'max_samples', None))
        # dlmc.py:112 books one attempt per chain and iteration on the host
        return run.finish(out, t0, n * done, store, n_attempted_trajectories=n * done, n_target_calls=target_calls,
                          n_target_gradient_calls=grad_calls)
