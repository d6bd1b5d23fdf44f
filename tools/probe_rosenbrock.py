"""Rosenbrock on the device: ms per transition of mala, hmc (L = 5), jump_mala (K_inner = 20) and neutra_hmc (L = 5) at
n = 65536 chains and d = 64 / 256 (block 2, mu = 1, a = 0.5, b = 5), on the fused kernels (the Rosenbrock object) against
the split path on the same object (a plain lambda wrapping it, fuse='never'), and against the general (per-coordinate)
quadratic kernel of the same launch family (a QuadraticPotential with a tensor of weights).  HIP events around the whole
sample() call, best of 2; one JSON line.

    python tools/probe_rosenbrock.py [d ...]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from rosenbrock_fp64 import RosenbrockU64  # noqa: E402
from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import QuadraticPotential, Rosenbrock  # noqa: E402
from nfmc_amd.samplers import jump, mcmc, neutra  # noqa: E402


def ev_ms(fn, reps=2):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


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
    dims = [int(v) for v in sys.argv[1:]] or [64, 256]
    res = {'unit': 'ms per transition (all chains)', 'n': n, 'block': 2, 'mu': 1.0, 'a': 0.5, 'b': 5.0, 'cases': []}
    for d in dims:
        pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=2)
        ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 2)
        quad = QuadraticPotential(d, torch.linspace(0.5, 5.0, d), 1.0)   # the general (non exact-fit) quadratic kernel
        flow = Flow(RealNVP((d,)))
        x0 = ref.draw(n, 1).float()
        lm = float(torch.quantile(ref.hess_diag(x0[:4096].double()).abs().amax(dim=1), 0.9))
        h = 0.3 / math.sqrt(lm)
        for strategy in ('mala', 'hmc', 'jump_mala', 'neutra_hmc'):
            row = {'strategy': strategy, 'd': d}
            for label, target, fuse in (('fused', pot, 'auto'), ('split', lambda x: pot(x), 'never'),
                                        ('quadratic', quad, 'auto')):
                s, steps = make(strategy, d, target, fuse, flow, h if strategy != 'mala' else h * h)
                s.sample(x0, show_progress=False)
                row[label] = round(ev_ms(lambda: s.sample(x0, show_progress=False)) / steps, 4)
            row['speedup'] = round(row['split'] / row['fused'], 2)
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
