"""The latent Gaussian Markov random field on the device: ms per fused mala transition and per hmc trajectory of five
steps (all chains) on the SPDE-Matern lattice (alpha = 2, the 13-point stencil, kappa^2 = 0.5) at 16 x 16 and 32 x 32 and
on the second-order random walk with 512 coordinates, Poisson counts drawn at a seeded field, with tau fixed and with
tau unknown (centred and scaled; the 32 x 32 lattice with tau has d = 1025 and is left to the split path, so it is not
timed), against the same object on the split path of the same build (behind a plain lambda, fuse='never') and, for the
lattices with fixed tau, against the dense counterpart to_dense() on the kernels of kind 12: the ratios split / fused and
dense / fused.  Steps: mala d^(-1/3) / lambda and hmc d^(-1/4) / sqrt(lambda), lambda = hessian_bound at the generating
state; chains start at the generating state + 0.1 eps.  HIP events around the whole sample() call (10 mala transitions
or 5 hmc trajectories per call, on every path) after one warm-up call, REPS repetitions: median, min and max per case;
one JSON line.

    python tools/probe_gmrf.py [n_chains]        (default 65536)
"""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfmc_amd.potentials import LatentGMRF  # noqa: E402
from nfmc_amd.samplers import mcmc  # noqa: E402

REPS = 3
KAPPA2 = 0.5
MODES = {'fixed': {}, 'centered': dict(precision_prior=(2.0, 2.0)),
         'scaled': dict(precision_prior=(2.0, 2.0), parameterization='scaled')}


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


def problems(mode):
    """{name: (potential, generating state in its coordinates)}; a shape whose d passes 1024 in this mode is left out"""
    out = {}
    for side in (16, 32):
        if side * side + (mode != 'fixed') > 1024:
            continue
        proto = LatentGMRF.lattice(torch.zeros(side, side), KAPPA2, alpha=2)
        model = dict(MODES[mode], mean=1.0, rank=side * side)
        if mode == 'fixed':
            model['event_shape'] = (side, side)
        out['lattice%dx%d' % (side, side)] = LatentGMRF.synthetic(side * side, (proto.rows, proto.cols, proto.values),
                                                                  'poisson', side, **model)
    n = 512 if mode == 'fixed' else 511
    out['rw2_d512'] = LatentGMRF.synthetic(n, 'rw2', 'poisson', 3, **dict(MODES[mode], mean=1.0))
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
    for mode in MODES:
        for name, (pot, star) in problems(mode).items():
            d, shape = pot.dim, pot.event_shape
            lam = pot.hessian_bound(star)
            g = torch.Generator().manual_seed(3)
            x0 = (star[None] + 0.1 * torch.randn(n, d, generator=g, dtype=torch.float64)).float().reshape((n,) + shape)
            dense = pot.to_dense() if mode == 'fixed' and name.startswith('lattice') else None
            for strategy in ('mala', 'hmc'):
                steps = {'mala': 10, 'hmc': 5}[strategy]
                row = {'problem': name, 'mode': mode, 'strategy': strategy, 'n': n, 'd': d, 'W': pot.width, 'lambda': round(lam, 2)}
                row['fused'], row['fused_min_max'] = timed(make(strategy, shape, pot, 'auto', lam, steps), x0, steps)
                row['split'], row['split_min_max'] = timed(make(strategy, shape, lambda x: pot(x), 'never', lam, steps), x0, steps)
                row['split_over_fused'] = round(row['split'] / row['fused'], 2)
                if dense is not None:
                    row['dense'], row['dense_min_max'] = timed(make(strategy, shape, dense, 'auto', lam, steps), x0, steps)
                    row['dense_over_fused'] = round(row['dense'] / row['fused'], 2)
                print(json.dumps(row), file=sys.stderr, flush=True)
                res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
