"""Stochastic volatility on the device: ms per transition of mala and hmc (L = 5) at n = 65536 chains and T = 250 / 1000
(d = T + 3), and of jump_mala (K_inner = 20) and neutra_hmc (L = 5) at T = 250, on the fused kernels (the
StochasticVolatility object) against the split path on the same object (a plain lambda wrapping it, fuse='never').  Series
simulated at mu = -1, sigma = 0.25, phi = 0.95; chains start near those values (tests/sv_fp64.py).  HIP events around the
whole sample() call after one warm-up call, REPS repetitions: median, min and max per case; one JSON line.

    python tools/probe_sv.py [T ...]
"""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from sv_fp64 import SVU64, start_states  # noqa: E402
from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import StochasticVolatility  # noqa: E402
from nfmc_amd.samplers import jump, mcmc, neutra  # noqa: E402

REPS = 5


def ev_ms(fn, reps=REPS):
    """per-call ms of `reps` calls, each between two HIP events"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def make(strategy, d, target, fuse, flow, h):
    if strategy == 'mala':
        s = mcmc.MALA((d,), target, mcmc.LangevinKernel(event_size=d, step_size=h),
                      mcmc.LangevinParameters(n_iterations=10, store_samples=False))
        steps = 10
    elif strategy == 'hmc':
        s = mcmc.HMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=h),
                     mcmc.HMCParameters(n_iterations=5, store_samples=False))
        steps = 5
    elif strategy == 'jump_mala':
        s = jump.JumpMALA((d,), target, NFMCKernel((d,), flow=flow), jump.JumpNFMCParameters(n_iterations=1), None,
                          mcmc.LangevinParameters(n_iterations=20))
        s.inner_sampler.kernel.step_size = h
        steps = 21
    else:
        s = neutra.NeuTraHMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=h),
                             mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=flow),
                             neutra.NeuTraParameters(n_iterations=2, store_samples=False))
        steps = 2
    s.seed, s.fuse = 1, fuse
    if strategy == 'jump_mala':
        s.inner_sampler.fuse = fuse
        s.params.store_samples = False
    return s, steps


def main():
    torch.cuda.set_device(0)
    n = 65536
    series = [int(v) for v in sys.argv[1:]] or [250, 1000]
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'n': n, 'mu': -1.0, 'sigma': 0.25,
           'phi': 0.95, 'cases': []}
    for T in series:
        d = T + 3
        y, x0, _ = start_states(T, n, T)
        pot, ref = StochasticVolatility(y), SVU64(y)
        x0 = x0.float()
        lm = float(torch.quantile(ref.hess_diag(x0[:1024].double()).abs().amax(dim=1), 0.9))
        flow = Flow(RealNVP((d,)))
        for strategy in ('mala', 'hmc') + (('jump_mala', 'neutra_hmc') if T == 250 else ()):
            h = 0.3 * d ** (-1 / 3) / lm if strategy in ('mala', 'jump_mala') else 0.3 * d ** (-1 / 4) / math.sqrt(lm)
            row = {'strategy': strategy, 'T': T, 'd': d}
            for label, target, fuse in (('fused', pot, 'auto'), ('split', lambda x: pot(x), 'never')):
                s, steps = make(strategy, d, target, fuse, flow, h)
                s.sample(x0, show_progress=False)
                t = [v / steps for v in ev_ms(lambda: s.sample(x0, show_progress=False))]
                row[label] = round(statistics.median(t), 4)
                row[label + '_min_max'] = [round(min(t), 4), round(max(t), 4)]
            row['speedup'] = round(row['split'] / row['fused'], 2)
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
