"""fp64 references for the trajectory-length adaptation of the device warmup (ChEES-HMC with a lagged centre; DESIGN,
"Trajectory length").  No tests in here.

  replay_update   one controller update recomputed from the kernel's own kept states and the controller state it started
                  from: proposals, final momenta and log ratios in fp64 (and in torch fp32, which measures what fp32
                  arithmetic alone costs), noise from oracle.samplers.PhiloxNoise on the stream the launches drew from
  free_run        a whole adaptive warmup in fp64 on the CPU: the reference of the behaviour tests
  Snapshots       the tuning state and mass diagonal of a DeviceTuning before every launch, one launch per pool
"""
import functools
import math
from dataclasses import dataclass, field
from typing import List

import torch

from nfmc_amd.tuning import (DualAveraging, DualAveragingParams, TrajectoryAdaptation, TrajectoryAdaptationParams,
                             leapfrog_count)
from oracle import philox
from oracle import samplers as osamp


def _grad(target, x):
    return osamp._value_and_grad(target, x)[1]


def trajectory(x, p0, target, h, imd, L, grad=None):
    """L textbook leapfrog steps (one gradient per position) from (x, p0) in the dtype of x: (q, p)."""
    g = grad if grad is not None else functools.partial(_grad, target)
    q, p = x, p0 - h / 2 * g(x)
    for l in range(L):
        q = q + h * (p * imd)
        p = p - (h if l + 1 < L else h / 2) * g(q)
    return q.detach(), p.detach()


def chain_terms(x, q, p, c, imd, t, log_ratio):
    """Per chain: alpha, alpha * g and the magnitude of the terms of alpha * g (a non-finite chain adds nothing)."""
    dx, dq, v = x - c, q - c, p * imd
    a0, a1, b = (dx * dx).sum(1), (dq * dq).sum(1), (dq * v).sum(1)
    ok = torch.isfinite(log_ratio) & torch.isfinite(a0) & torch.isfinite(a1) & torch.isfinite(b)
    zero = torch.zeros_like(a0)
    alpha = torch.where(ok, torch.exp(torch.clamp(log_ratio, max=0.0)), zero)
    g = torch.where(ok, t * (a1 - a0) * b, zero)
    mag = torch.where(ok, t * ((a0 + a1) * b.abs() + (a1 - a0).abs() * (dq * v).abs().sum(1)), zero)
    return alpha, alpha * g, alpha * mag


@dataclass
class Replay:
    g_hat: float                 # fp64
    alpha_sum: float
    g_hat32: float               # the torch-fp32 restatement of the same sums
    alpha_sum32: float
    magnitude: float             # E = sum t alpha [(a0 + a1)|b| + |a1 - a0| sum_i |(q_i - c_i) v_i|] / sum alpha
    leapfrogs: List[int]
    controller: TrajectoryAdaptation   # after the update
    log_ratios: List[torch.Tensor] = field(default_factory=list)


def controller_from(row, params=None, max_leapfrog_steps=128):
    """A TrajectoryAdaptation holding the state (log T, log T-bar, v, update count) of `row`."""
    ctl = TrajectoryAdaptation(1.0, params or TrajectoryAdaptationParams(), max_leapfrog_steps)
    ctl.log_length, ctl.log_averaged, ctl.v, ctl.count = (float(row['log_length']), float(row['log_averaged']),
                                                         float(row['v']), int(row['count']))
    return ctl


def replay_update(prev_row, states, x_prev, c, h, T, k0, pool, target, imd, seed, h_next=None, params=None,
                  max_leapfrog_steps=128, g_shift=0.0):
    """The controller update over transitions k0 .. k0 + pool - 1 (Philox step counters).
    prev_row: dict(log_length, log_averaged, v, count) the update starts from.  states: (pool, n, d) the kernel's kept
    states, x_prev (n, d) the state before the pool, c (d,) the lagged centre, h and T the fp64 step size and length the
    pool ran with, imd (d,) its mass diagonal, h_next the step size the same update set (default h).
    g_shift: added to g-hat before the controller step (the sensitivity of the controller to g-hat's tolerance)."""
    states = torch.as_tensor(states)
    n, d = x_prev.shape
    sums = {torch.float64: [0.0, 0.0, 0.0], torch.float32: [0.0, 0.0, 0.0]}
    Ls, lrs = [], []
    for s in range(pool):
        k = k0 + s
        L = leapfrog_count(k, T, h, max_leapfrog_steps)
        Ls.append(L)
        pre = (x_prev if s == 0 else states[s - 1]).float()
        for dt in (torch.float64, torch.float32):
            noise = osamp.PhiloxNoise(seed, dtype=dt)
            m = torch.as_tensor(imd).to(dt).reshape(d)
            x = pre.to(dt)
            hh = float(torch.tensor(h, dtype=torch.float32))      # the kernels integrate with the fp32 step size
            p0 = noise.normal(n, (d,), k & 0xffffffff, philox.TAG_NOISE) * (1 / m.sqrt())
            q, p = trajectory(x, p0, target, hh, m, L)
            with torch.no_grad():
                lr = (target(x) + 0.5 * (p0 * p0 * m).sum(1)) - (target(q) + 0.5 * (p * p * m).sum(1))
                t = torch.tensor(L * h, dtype=dt)
                alpha, ag, amag = chain_terms(x, q, p, torch.as_tensor(c).to(dt), m, t, lr)
            acc = sums[dt]
            acc[0] += float(ag.double().sum())
            acc[1] += float(alpha.double().sum())
            acc[2] += float(amag.double().sum())
            if dt is torch.float64:
                lrs.append(lr)
    g64 = sums[torch.float64][0] / sums[torch.float64][1] if sums[torch.float64][1] > 0 else 0.0
    g32 = sums[torch.float32][0] / sums[torch.float32][1] if sums[torch.float32][1] > 0 else 0.0
    mag = sums[torch.float64][2] / sums[torch.float64][1] if sums[torch.float64][1] > 0 else 0.0
    ctl = controller_from(prev_row, params, max_leapfrog_steps)
    ctl.step(g64 + g_shift, sums[torch.float64][1], h if h_next is None else h_next)
    return Replay(g64, sums[torch.float64][1], g32, sums[torch.float32][1], mag, Ls, ctl, lrs)


def free_run(target, x0, W, seed, h0=0.25, L0=None, every=1, max_leapfrog_steps=128, params=None, grad=None,
             tune_step_size=True, tune_inv_mass_diag=True, imd_adjustment=1e-3, step0=1 << 31):
    """The adaptive warmup in fp64: W transitions of jittered HMC on the Philox stream of `seed`, per `every` of them the
    mass diagonal (EMA of the pooled variance), the step size (dual averaging) and then the trajectory length.
    Returns (T-bar, T, h, history) with history rows (T, h, g-hat, sum alpha, leapfrog steps)."""
    x = x0.double().clone()
    n, d = x.shape
    noise = osamp.PhiloxNoise(seed, dtype=torch.float64)
    h = float(h0)
    T0 = (L0 if L0 is not None else 1) * h
    ctl = TrajectoryAdaptation(T0, params or TrajectoryAdaptationParams(), max_leapfrog_steps)
    da = DualAveraging(h, DualAveragingParams())
    imd = torch.ones(d, dtype=torch.float64)
    c = x.mean(0)
    hist = []
    for s0, k in osamp.pools(W, every):
        T = ctl.value
        num = den = 0.0
        accepted, steps, kept = 0, 0, []
        for s in range(s0, s0 + k):
            step = (step0 + s) & 0xffffffff
            L = leapfrog_count(step, T, h, max_leapfrog_steps)
            steps += L
            p0 = noise.normal(n, (d,), step, philox.TAG_NOISE) * (1 / imd.sqrt())
            q, p = trajectory(x, p0, target, h, imd, L, grad=grad)
            with torch.no_grad():
                lr = (target(x) + 0.5 * (p0 * p0 * imd).sum(1)) - (target(q) + 0.5 * (p * p * imd).sum(1))
                alpha, ag, _ = chain_terms(x, q, p, c, imd, L * h, lr)
                num += float(ag.sum())
                den += float(alpha.sum())
                acc = torch.log(noise.uniform(n, step, philox.TAG_ACCEPT)) < lr
                x = torch.where(acc[:, None], q, x)
            accepted += int(acc.sum())
            kept.append(x)
        xs = torch.cat(kept)
        if n > 1 and tune_inv_mass_diag:
            imd = imd_adjustment * xs.var(0) + (1 - imd_adjustment) * imd
        c = xs.mean(0)
        h_used = h
        if tune_step_size:
            da.step(da.params.target_acceptance_rate - accepted / (n * k))
            h = da.value
        g_hat = num / den if den > 0 else 0.0
        ctl.step(g_hat, den, h)
        hist.append((T, h_used, g_hat, den, steps))
    return ctl.averaged, ctl.value, h, hist


def gaussian(scales):
    """(U, grad U, x0 draw) of N(0, diag(scales^2)) in the dtype of the argument."""
    s2 = torch.as_tensor(scales, dtype=torch.float64) ** 2

    def u(x):
        return 0.5 * (x * x / s2.to(x.dtype)).sum(1)

    def grad(x):
        return x / s2.to(x.dtype)
    return u, grad


BEHAVIOUR = {'unit8': torch.ones(8), 'lin16': torch.linspace(1.0, 10.0, 16)}
BEHAVIOUR_N, BEHAVIOUR_W, BEHAVIOUR_H0, BEHAVIOUR_L0 = 256, 300, 0.25, 1


def behaviour_x0(name, seed):
    s = BEHAVIOUR[name]
    return (torch.randn(BEHAVIOUR_N, s.numel(), generator=torch.Generator().manual_seed(1000 + seed),
                        dtype=torch.float64) * s.double()).float()


@functools.lru_cache(maxsize=None)
def behaviour_reference(name, seed):
    """T-bar of free_run on a behaviour target (computed once per process, shared by the host and the GPU test).  The
    mass diagonal stays at one: adapted, it preconditions the scales away and with them the difference the test is about."""
    u, grad = gaussian(BEHAVIOUR[name])
    return free_run(u, behaviour_x0(name, seed), BEHAVIOUR_W, seed, h0=BEHAVIOUR_H0, L0=BEHAVIOUR_L0, grad=grad,
                    tune_inv_mass_diag=False)[0]


class Snapshots:
    """Cuts a device warmup into one launch per pool and keeps, before every launch and after the last, a copy of the
    tuning state (trajectory block included) and of the mass diagonal: what each pool ran with, as the kernels saw it."""

    def __init__(self, monkeypatch, sampler, every):
        from nfmc_amd.samplers import mcmc
        self.before, self.tune = [], None
        cls = type(sampler)
        orig = cls._launch
        monkeypatch.setattr(mcmc, 'launch_limit', lambda watched, *a: max(1, int(every)))

        def launch(s, run, pot, k, step0, samples, tune=None, **kw):
            self.tune = tune
            self.before.append((tune.state.clone(), tune.imd.clone(), int(step0), int(k)))
            return orig(s, run, pot, k, step0, samples, tune=tune, **kw)
        monkeypatch.setattr(cls, '_launch', launch)
        down = mcmc.DeviceTuning.download

        def download(t, kernel):
            self.final = (t.state.clone(), t.imd.clone())
            return down(t, kernel)
        monkeypatch.setattr(mcmc.DeviceTuning, 'download', download)

    def rows(self):
        """[(state, imd, step0, k)] on the host, one per launch, then the final (state, imd)."""
        return [(s.cpu(), m.cpu(), k0, k) for s, m, k0, k in self.before], (self.final[0].cpu(), self.final[1].cpu())
