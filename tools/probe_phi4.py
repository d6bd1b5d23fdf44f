"""The phi^4 lattice field on the device: ms per transition of mala and hmc (L = 5) at n = 65536 chains on the periodic
(8, 8), (16, 16) and (32, 32) lattices in the broken phase (m2 = -1, lam = 1, kappa = 1), on the fused kernels (the
LatticePhi4 object) against the split path on the same object (a plain lambda wrapping it, fuse='never').  Chains start
at +-v + N(0, 1 / lm) (tests/test_gpu_phi4.py).  HIP events around the whole sample() call after one warm-up call, REPS
repetitions: median, min and max per case; one JSON line.

    python tools/probe_phi4.py [L ...]        (square lattices of side L; default 8 16 32)
"""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfmc_amd.potentials import LatticePhi4  # noqa: E402
from nfmc_amd.samplers import mcmc  # noqa: E402

REPS = 5
M2, LAM, KAPPA = -1.0, 1.0, 1.0


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


def make(strategy, shape, target, fuse, h):
    d = int(math.prod(shape))
    if strategy == 'mala':
        s = mcmc.MALA(shape, target, mcmc.LangevinKernel(event_size=d, step_size=h),
                      mcmc.LangevinParameters(n_iterations=10, store_samples=False))
        steps = 10
    else:
        s = mcmc.HMC(shape, target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=h),
                     mcmc.HMCParameters(n_iterations=5, store_samples=False))
        steps = 5
    s.seed, s.fuse = 1, fuse
    return s, steps


def main():
    torch.cuda.set_device(0)
    n = 65536
    sides = [int(v) for v in sys.argv[1:]] or [8, 16, 32]
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'n': n, 'm2': M2, 'lam': LAM,
           'kappa': KAPPA, 'boundary': 'periodic', 'cases': []}
    v = math.sqrt(-M2 / LAM)
    lm = abs(M2) + 3.0 * LAM * (v * v + 0.25) + 8.0 * KAPPA
    for side in sides:
        shape = (side, side)
        d = side * side
        pot = LatticePhi4(shape, m2=M2, lam=LAM, kappa=KAPPA)
        g = torch.Generator().manual_seed(side)
        sign = torch.where(torch.rand(n, 1, 1, generator=g) < 0.5, -1.0, 1.0)
        x0 = sign * v + torch.randn((n,) + shape, generator=g) / math.sqrt(lm)
        for strategy in ('mala', 'hmc'):
            h = 0.5 * d ** (-1 / 3) / lm if strategy == 'mala' else 0.5 * d ** (-1 / 4) / math.sqrt(lm)
            row = {'strategy': strategy, 'shape': list(shape), 'd': d}
            for label, target, fuse in (('fused', pot, 'auto'), ('split', lambda x: pot(x), 'never')):
                s, steps = make(strategy, shape, target, fuse, h)
                s.sample(x0, show_progress=False)
                t = [ms / steps for ms in ev_ms(lambda: s.sample(x0, show_progress=False))]
                row[label] = round(statistics.median(t), 4)
                row[label + '_min_max'] = [round(min(t), 4), round(max(t), 4)]
            row['speedup'] = round(row['split'] / row['fused'], 2)
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
