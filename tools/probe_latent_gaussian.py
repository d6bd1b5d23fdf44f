"""The latent Gaussian model on the device: ms per fused mala transition and per hmc trajectory of five steps (all
chains) at d = 256 (256 seeded points in the unit square, K = SE(variance 1, lengthscale 0.25) + 0.05 I, Poisson counts
drawn at a seeded generating state, exposure 1) and at the 32 x 32 log-Gaussian Cox process (d = 1024,
LatentGaussianModel.log_gaussian_cox with a nugget of 0.05), in both parameterisations, against the same object on the
split path of the same build (behind a plain lambda, fuse='never') and against a FullRankGaussian of the same d (the
problem's own precision matrix) on the fused kernels: the ratios fused / split and latent / full-rank.  Steps: mala
d^(-1/3) / lambda and hmc d^(-1/4) / sqrt(lambda), lambda = hessian_bound at the generating state; chains start at the
generating state + 0.3 eps in the whitened coordinates.  HIP events around the whole sample() call after one warm-up call,
REPS repetitions: median, min and max per case; one JSON line.

    python tools/probe_latent_gaussian.py [n_chains]        (default 65536)
"""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfmc_amd.potentials import FullRankGaussian, LatentGaussianModel  # noqa: E402
from nfmc_amd.samplers import mcmc  # noqa: E402

REPS = 3
NUGGET = 0.05


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


def problems(par):
    """{name: (potential, generating state in its coordinates)}"""
    out = {}
    out['points256'] = LatentGaussianModel.synthetic(256, 'poisson', 1, mean=1.0, parameterization=par)
    g = torch.Generator().manual_seed(2)
    kw = dict(variance=1.0, lengthscale=2.0 / 32, jitter=NUGGET, mean=math.log(2000.0), parameterization=par)
    proto = LatentGaussianModel.log_gaussian_cox(torch.zeros(32, 32), **kw)
    f = proto.mean + proto.cholesky @ torch.randn(1024, generator=g, dtype=torch.float64)
    counts = torch.poisson(proto.weight * torch.exp(f), generator=g).reshape(32, 32)
    pot = LatentGaussianModel.log_gaussian_cox(counts, **kw)
    out['lgcp32x32'] = (pot, pot.coordinates(f))
    return out


def make(strategy, shape, target, fuse, lam, steps):
    d = int(math.prod(shape))
    if strategy == 'mala':
        s = mcmc.MALA(shape, target, mcmc.LangevinKernel(event_size=d, step_size=d ** (-1 / 3) / lam),
                      mcmc.LangevinParameters(n_iterations=steps, store_samples=False))
    else:
        s = mcmc.HMC(shape, target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=d ** (-1 / 4) / math.sqrt(lam)),
                     mcmc.HMCParameters(n_iterations=steps, store_samples=False))
    s.seed, s.fuse = 1, fuse
    return s


def timed(s, x0, steps):
    s.sample(x0, show_progress=False)
    t = [ms / steps for ms in ev_ms(lambda: s.sample(x0, show_progress=False))]
    return round(statistics.median(t), 4), [round(min(t), 4), round(max(t), 4)]


def main():
    torch.cuda.set_device(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'cases': []}
    for par in LatentGaussianModel.PARAMETERIZATIONS:
        for name, (pot, star) in problems(par).items():
            d, shape = pot.dim, pot.event_shape
            lam = pot.hessian_bound(star)
            g = torch.Generator().manual_seed(3)
            white = pot if pot.whitened else pot.reparameterized('whitened')
            z = white.coordinates(pot.latent(star))[None] + 0.3 * torch.randn(n, d, generator=g, dtype=torch.float64)
            x0 = pot.coordinates(white.latent(z)).float().reshape((n,) + shape)
            full = FullRankGaussian(pot.mean, precision=pot.precision, event_shape=shape)
            xg = white.latent(z).float().reshape((n,) + shape)
            for strategy in ('mala', 'hmc'):
                steps = {'mala': 10, 'hmc': 5}[strategy]
                row = {'problem': name, 'parameterization': par, 'strategy': strategy, 'n': n, 'd': d, 'lambda': round(lam, 2)}
                row['fused'], row['fused_min_max'] = timed(make(strategy, shape, pot, 'auto', lam, steps), x0, steps)
                row['split'], row['split_min_max'] = timed(make(strategy, shape, lambda x: pot(x), 'never', lam, 1), x0, 1)
                lam_full = float(torch.linalg.eigvalsh(pot.precision).max())
                row['fullrank'], row['fullrank_min_max'] = timed(make(strategy, shape, full, 'auto', lam_full, steps), xg, steps)
                row['split_over_fused'] = round(row['split'] / row['fused'], 2)
                row['fused_over_fullrank'] = round(row['fused'] / row['fullrank'], 2)
                print(json.dumps(row), file=sys.stderr, flush=True)
                res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
