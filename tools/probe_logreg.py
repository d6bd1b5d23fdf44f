"""Bayesian logistic regression on the device: ms per transition of mala, jump_mala (K_inner = 100) and imh at
n = 65536 chains, on German-credit-sized synthetic data (N = 1000 rows, d = 25, fixed seed), on the fused kernels (the
BayesianLogisticRegression object) against the split path on the same object (a plain lambda wrapping it,
fuse='never').  HIP events around the whole sample() call, best of 3; one JSON line.

    python tools/probe_logreg.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import BayesianLogisticRegression  # noqa: E402
from nfmc_amd.samplers import imh, jump, mcmc  # noqa: E402


def ev_ms(fn, reps=3):
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


def make(strategy, d, target, fuse, flow):
    if strategy == 'mala':
        s = mcmc.MALA((d,), target, mcmc.LangevinKernel(event_size=d, step_size=1e-3),
                      mcmc.LangevinParameters(n_iterations=10, store_samples=False))
        steps = 10
    elif strategy == 'jump_mala':
        s = jump.JumpMALA((d,), target, NFMCKernel((d,), flow=flow), jump.JumpNFMCParameters(n_iterations=1), None,
                          mcmc.LangevinParameters(n_iterations=100))
        s.inner_sampler.kernel.step_size = 1e-3
        steps = 101
    else:
        s = imh.FixedIMH((d,), target, imh.IMHKernel((d,), flow=flow), imh.IMHParameters(n_iterations=10, store_samples=False))
        steps = 10
    s.seed, s.fuse = 1, fuse
    if strategy == 'jump_mala':
        s.inner_sampler.fuse = fuse
        s.params.store_samples = False
    return s, steps


def main():
    torch.cuda.set_device(0)
    n, N, d = 65536, 1000, 25
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g)
    X[:, 0] = 1.0
    w = torch.randn(d, generator=g) / d ** 0.5
    y = (torch.rand(N, generator=g) < torch.sigmoid(X @ w)).float()
    pot = BayesianLogisticRegression(X, y, prior_scale=1.0)
    flow = Flow(RealNVP((d,)))
    x0 = w + 0.05 * torch.randn(n, d, generator=g)
    res = {'unit': 'ms per transition (all chains)', 'n': n, 'N': N, 'd': d, 'cases': []}
    for strategy in ('mala', 'jump_mala', 'imh'):
        row = {'strategy': strategy}
        for label, target, fuse in (('fused', pot, 'auto'), ('split', lambda x: pot(x), 'never')):
            s, steps = make(strategy, d, target, fuse, flow)
            s.sample(x0, show_progress=False)
            row[label] = round(ev_ms(lambda: s.sample(x0, show_progress=False)) / steps, 4)
        row['speedup'] = round(row['split'] / row['fused'], 2)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
