"""mclmc on the device: ms per step at n = 65536 chains on SumOfSquares d = 64, Rosenbrock d = 100 and
ItemResponseTheory d = 501 (and a quadratic with per-coordinate weights at d = 64), beside a mala transition of the same object (the nearest existing kernel: one gradient, one
value, d normals per transition), and ms per step of an mclmc warmup (tune_every = 8, all three tuners on).  HIP events
around the whole sample() call of 100 steps, median of 3; one JSON line.

    python tools/probe_mclmc.py [n_chains]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from nfmc_amd.potentials import ItemResponseTheory, QuadraticPotential, Rosenbrock, SumOfSquares  # noqa: E402
from nfmc_amd.samplers import mcmc  # noqa: E402

STEPS = 100


def ev_ms(fn, reps=3):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def make(strategy, d, pot, tuning=False):
    if strategy == 'mala':
        s = mcmc.MALA((d,), pot, mcmc.LangevinKernel(event_size=d, step_size=1e-3),
                      mcmc.LangevinParameters(n_iterations=STEPS, store_samples=False))
    else:
        s = mcmc.MCLMC((d,), pot, mcmc.MCLMCKernel(event_size=d, step_size=1e-2),
                       mcmc.MCLMCParameters(n_iterations=STEPS, store_samples=False, tuning=tuning, tune_inv_mass_diag=True))
    s.seed = 1
    return s


def cases(n):
    from irt_fp64 import IRTFast64, start_states
    from rosenbrock_fp64 import RosenbrockU64
    x64 = torch.randn(n, 64, generator=torch.Generator().manual_seed(1))
    yield 'sum_of_squares', 64, SumOfSquares((64,)), x64
    # the same target through the general kernels (per-coordinate weights): mala's exact-fit path taken out of the comparison
    yield 'quadratic_general', 64, QuadraticPotential((64,), torch.linspace(0.5, 2.0, 64), 0.1), x64
    yield 'rosenbrock', 100, Rosenbrock(100, mu=1.0, a=0.5, b=5.0, block=2), RosenbrockU64(100, 1.0, 0.5, 5.0, 2).draw(n, 1).float()
    pot, truth = ItemResponseTheory.synthetic(400, 100, 501, missing=0.25)
    yield 'item_response', 501, pot, start_states(IRTFast64(pot.responses, pot.observed), truth, n, 502).float()


def main():
    torch.cuda.set_device(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    res = {'unit': 'ms per step (all chains)', 'n': n, 'steps_per_call': STEPS, 'cases': []}
    for name, d, pot, x0 in cases(n):
        row = {'target': name, 'd': d}
        for label, strategy, tuning in (('mala', 'mala', False), ('mclmc', 'mclmc', False), ('mclmc_warmup', 'mclmc', True)):
            s = make(strategy, d, pot, tuning)
            s.sample(x0, show_progress=False)
            row[label] = round(ev_ms(lambda: s.sample(x0, show_progress=False)) / STEPS, 4)
        row['mclmc_over_mala'] = round(row['mclmc'] / row['mala'], 2)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
