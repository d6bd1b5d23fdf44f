"""The diffusion bridge on the device: ms per transition of mala, hmc (L = 5), jump_mala (K_inner = 20) and neutra_hmc
(L = 5) at n = 65536 chains, on the fused kernels (the DiffusionBridge object) against the split path on the same object
(a plain lambda wrapping it, fuse='never').  Shapes: the Lorenz preset (m = 3, T = 30: d = 90, and d = 92 with unknown
scales), m = 3 with T = 341 (d = 1023) and Brownian motion with T = 1022 and unknown scales (d = 1024).  Chains start about
the generating path (DiffusionBridge.synthetic's truth + 0.5 sigma sqrt(dt) eps); steps 0.3 d^(-1/3) / lambda and
0.3 d^(-1/4) / sqrt(lambda) with lambda = 4 / (sigma^2 dt) + 1 / tau^2, the bound of the Hessian's diagonal.  HIP events
around the whole sample() call after one warm-up call, REPS repetitions: median, min and max per case; one JSON line.

    python tools/probe_diffusion.py [case ...]        cases: lorenz90 lorenz92 lorenz1023 brownian1024
"""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import DiffusionBridge  # noqa: E402
from nfmc_amd.samplers import jump, mcmc, neutra  # noqa: E402

REPS = 3
CASES = {'lorenz90': (30, 'lorenz63', 3, False, dict(dt=0.02, innovation_scale=0.1, observation_scale=1.0)),
         'lorenz92': (30, 'lorenz63', 3, True, dict(dt=0.02, innovation_scale=0.1, observation_scale=1.0)),
         'lorenz1023': (341, 'lorenz63', 3, False, dict(dt=0.02, innovation_scale=0.1, observation_scale=1.0)),
         'brownian1024': (1022, 'cubic', 1, True, dict(dt=1.0, innovation_scale=0.1, observation_scale=0.15))}


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
    names = sys.argv[1:] or list(CASES)
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'n': n, 'cases': []}
    for name in names:
        T, drift, m, unknown, model = CASES[name]
        kw = dict(model, m=m)
        if unknown:
            kw['scale_prior'] = (0.0, 2.0)
        pot, truth = DiffusionBridge.synthetic(T, drift, 7, **kw)
        d = pot.dim
        sig, tau, dt = model['innovation_scale'], model['observation_scale'], model['dt']
        g = torch.Generator().manual_seed(11)
        x0 = truth[None].repeat(n, 1)
        x0[:, :T * m] += 0.5 * sig * math.sqrt(dt) * torch.randn(n, T * m, generator=g, dtype=torch.float64)
        x0 = x0.float()
        lam = 4.0 / (sig * sig * dt) + 1.0 / (tau * tau)
        flow = Flow(RealNVP((d,)))
        for strategy in ('mala', 'hmc', 'jump_mala', 'neutra_hmc'):
            h = 0.3 * d ** (-1 / 3) / lam if strategy in ('mala', 'jump_mala') else 0.3 * d ** (-1 / 4) / math.sqrt(lam)
            row = {'case': name, 'strategy': strategy, 'T': T, 'm': m, 'd': d}
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
