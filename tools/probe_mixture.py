"""GaussianMixture targets on the device: ms per transition of mala, hmc (L = 10), jump_mala (K_inner = 100) and imh, on
the fused kernels (the GaussianMixture object) against the split path on the same object (a plain lambda wrapping it,
fuse='never'), for K in {1, 2, 4, 8}, with the QuadraticPotential run of the same shape as the reference point.  HIP
events around the whole sample() call, best of 5; one JSON line.

    python tools/probe_mixture.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import GaussianMixture, QuadraticPotential  # noqa: E402
from nfmc_amd.samplers import imh, jump, mcmc  # noqa: E402


def ev_ms(fn, reps=5):
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
        s, steps = mcmc.MALA((d,), target, None, mcmc.LangevinParameters(n_iterations=20, store_samples=False)), 20
    elif strategy == 'hmc':
        s = mcmc.HMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=10, step_size=0.05),
                     mcmc.HMCParameters(n_iterations=5, store_samples=False))
        steps = 5
    elif strategy == 'jump_mala':
        s = jump.JumpMALA((d,), target, NFMCKernel((d,), flow=flow), jump.JumpNFMCParameters(n_iterations=1), None,
                          mcmc.LangevinParameters(n_iterations=100))
        steps = 101
    else:
        s = imh.FixedIMH((d,), target, imh.IMHKernel((d,), flow=flow), imh.IMHParameters(n_iterations=20, store_samples=False))
        steps = 20
    s.seed, s.fuse = 1, fuse
    if strategy == 'jump_mala':
        s.inner_sampler.fuse = fuse
    return s, steps


def main():
    torch.cuda.set_device(0)
    res = {'unit': 'ms per transition (all chains)', 'cases': []}
    for n, d in ((65536, 64), (32768, 256)):
        torch.manual_seed(0)
        flow = Flow(RealNVP((d,)))
        x0 = torch.randn(n, d)
        for strategy in ('mala', 'hmc', 'jump_mala', 'imh'):
            s, steps = make(strategy, d, QuadraticPotential((d,), 0.5, 0.0), 'auto', flow)
            s.sample(x0, show_progress=False)
            quad = ev_ms(lambda: s.sample(x0, show_progress=False)) / steps
            row = {'n': n, 'd': d, 'strategy': strategy, 'quadratic': round(quad, 4)}
            for K in (1, 2, 4, 8):
                g = torch.Generator().manual_seed(K)
                pot = GaussianMixture(d, 1.5 * torch.randn(K, d, generator=g), 0.8 + 0.4 * torch.rand(K, d, generator=g))
                for label, target, fuse in (('fused', pot, 'auto'), ('split', lambda x, p=pot: p(x), 'never')):
                    s, steps = make(strategy, d, target, fuse, flow)
                    s.sample(x0, show_progress=False)
                    row['K%d_%s' % (K, label)] = round(ev_ms(lambda: s.sample(x0, show_progress=False)) / steps, 4)
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
