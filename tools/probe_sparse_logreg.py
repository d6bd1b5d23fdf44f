"""Sparse logistic regression on the device: ms per transition of mala, hmc (L = 10), jump_mala (K_inner = 20) and
neutra_hmc (L = 10) at n = 65536 chains on German-credit-sized synthetic data (N = 1000 rows, D = 25 features, d = 51,
three nonzero coefficients, fixed seed), on the fused kernels (the SparseLogisticRegression object) against the split path
on the same object (a plain lambda wrapping it, fuse='never'); and the same fused runs for BayesianLogisticRegression at
d = 25 on the same X, to show what the hierarchy costs.  Every sampler is warmed once; then fused and split calls
alternate, REPS of each, HIP events around the whole sample() call: median, min and max per case; one JSON line.

    python tools/probe_sparse_logreg.py
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

from sparse_logreg_fp64 import SLRU64, start_states, synthetic  # noqa: E402
from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import BayesianLogisticRegression, SparseLogisticRegression  # noqa: E402
from nfmc_amd.samplers import jump, mcmc, neutra  # noqa: E402

REPS = 5


def ev_ms(fn):
    """ms of one call between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def make(strategy, d, target, fuse, flow, h):
    if strategy == 'mala':
        s = mcmc.MALA((d,), target, mcmc.LangevinKernel(event_size=d, step_size=h),
                      mcmc.LangevinParameters(n_iterations=10, store_samples=False))
        steps = 10
    elif strategy == 'hmc':
        s = mcmc.HMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=10, step_size=h),
                     mcmc.HMCParameters(n_iterations=5, store_samples=False))
        steps = 5
    elif strategy == 'jump_mala':
        s = jump.JumpMALA((d,), target, NFMCKernel((d,), flow=flow), jump.JumpNFMCParameters(n_iterations=1), None,
                          mcmc.LangevinParameters(n_iterations=20))
        s.inner_sampler.kernel.step_size = h
        steps = 21
    else:
        s = neutra.NeuTraHMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=10, step_size=h),
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
    n, N, D = 65536, 1000, 25
    d = 2 * D + 1
    X, y, _ = synthetic(N, D, 0)
    pot, ref = SparseLogisticRegression(X, y), SLRU64(X, y)
    x0 = start_states(D, n, 1, spread=0.5).float()
    lm = float(torch.quantile(ref.hess_diag(x0[:1024].double()).abs().amax(dim=1), 0.9))
    blr = BayesianLogisticRegression(X, y, prior_scale=1.0)
    xb = 0.05 * torch.randn(n, D, generator=torch.Generator().manual_seed(2))
    res = {'unit': 'ms per transition (all chains); median, min, max of %d alternated calls' % REPS, 'n': n, 'N': N,
           'D': D, 'd': d, 'cases': []}
    cases = [(s_, 'sparse', d, pot, x0, lm) for s_ in ('mala', 'hmc', 'jump_mala', 'neutra_hmc')]
    cases += [(s_, 'logreg', D, blr, xb, N * 0.25) for s_ in ('mala', 'hmc', 'jump_mala')]
    for strategy, model, dd, target, xs, lmax in cases:
        flow = Flow(RealNVP((dd,)))
        h = 0.3 * dd ** (-1 / 3) / lmax if strategy in ('mala', 'jump_mala') else 0.3 * dd ** (-1 / 4) / math.sqrt(lmax)
        runs = {}
        for label, tgt, fuse in (('fused', target, 'auto'), ('split', lambda x, t=target: t(x), 'never')):
            if model == 'logreg' and label == 'split':
                continue
            s, steps = make(strategy, dd, tgt, fuse, flow, h)
            s.sample(xs, show_progress=False)                      # warm this shape
            runs[label] = (s, steps)
        times = {k: [] for k in runs}
        for _ in range(REPS):
            for label, (s, steps) in runs.items():                 # fused and split alternate
                times[label].append(ev_ms(lambda: s.sample(xs, show_progress=False)) / steps)
        row = {'model': model, 'strategy': strategy, 'd': dd}
        for label, t in times.items():
            row[label] = round(statistics.median(t), 4)
            row[label + '_min_max'] = [round(min(t), 4), round(max(t), 4)]
        if 'split' in row:
            row['speedup'] = round(row['split'] / row['fused'], 2)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
