"""NeuTra-MH on the device: ms per transition at n = 65536 chains of
  fused   neutra_mh on nfmc_neutra_mh_steps_f32 (the potential object),
  split   neutra_mh on the inner sampler's split path (the same object behind a plain lambda, fuse='never'),
  hmc1    fused neutra_hmc with one leapfrog step, the cheapest NeuTra trajectory there was,
for SumOfSquares d = 64, Funnel d = 128, SparseLogisticRegression d = 51 (N = 1000), ItemResponseTheory d = 501 (400
students, 100 questions) on the default RealNVP, and SumOfSquares d = 64 on a c-rqnsf flow.  Flows keep their initial
weights (timing does not depend on them); proposal scale 0.5 / sqrt(d), HMC step 0.1 / sqrt(d).  Every sampler is warmed
once; then the three alternate, REPS calls of STEPS transitions each, HIP events around the whole sample() call (wall
time of the call on the device's clock, host loop included): median, min and max per case; one JSON line.

    python tools/probe_neutra_mh.py
    python tools/probe_neutra_mh.py --kinds [n ...]     every neutra_valu kind, fused and split, at n chains (65536 1024)

`fused` always means the kernel: the sampler's `mh_kernel_kinds` is widened to every potential, so that a kind which
NeuTra.sample keeps on the split path (neutra.MH_KERNEL_KINDS says which, from the --kinds table) is still timed there.
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

from sparse_logreg_fp64 import start_states, synthetic  # noqa: E402
from nfmc_amd import potentials as P  # noqa: E402
from nfmc_amd.potentials import Funnel, ItemResponseTheory, SparseLogisticRegression, SumOfSquares  # noqa: E402
from nfmc_amd.samplers import mcmc, neutra  # noqa: E402
from nfmc_amd.util import create_flow_object  # noqa: E402

REPS, STEPS, N = 3, 100, 65536


def ev_ms(fn):
    """ms of one call between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def make(label, d, target, flow, steps=STEPS):
    kernel = neutra.NeuTraKernel((d,), flow=flow)
    params = neutra.NeuTraParameters(n_iterations=steps, store_samples=False)
    if label == 'hmc1':
        s = neutra.NeuTraHMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=1, step_size=0.1 / math.sqrt(d)),
                             mcmc.HMCParameters(), kernel, params)
    else:
        scale = torch.full((d,), 0.5 / math.sqrt(d))
        s = neutra.NeuTraMH((d,), target if label == 'fused' else (lambda x: target(x)),
                            mcmc.MHKernel(event_size=d, inv_mass_diag=scale), mcmc.MHParameters(), kernel, params)
    s.seed, s.fuse = 1, 'never' if label == 'split' else 'auto'
    s.mh_kernel_kinds = (P.Potential,)
    return s


def problems():
    g = torch.Generator().manual_seed(3)
    yield 'sum_of_squares', 64, 'realnvp', SumOfSquares((64,)), torch.randn(N, 64, generator=g)
    yield 'funnel', 128, 'realnvp', Funnel((128,)), torch.randn(N, 128, generator=g)
    D = 25
    X, y, _ = synthetic(1000, D, 0)
    yield 'sparse_logreg', 2 * D + 1, 'realnvp', SparseLogisticRegression(X, y), start_states(D, N, 1, spread=0.5).float()
    S, Q = 400, 100
    irt, truth = ItemResponseTheory.synthetic(S, Q, 0, missing=0.25)
    d = S + Q + 1
    yield 'item_response', d, 'realnvp', irt, (torch.as_tensor(truth).float().reshape(1, d) + 0.1 * torch.randn(N, d, generator=g))
    yield 'sum_of_squares', 64, 'c-rqnsf', SumOfSquares((64,)), torch.randn(N, 64, generator=g)


def kinds(n):
    """(name, potential, starts (n, d)) for every kind of the VALU NeuTra kernels, at a shape of its own probe or tests"""
    g = torch.Generator().manual_seed(5)

    def near(truth, s=0.05):
        truth = torch.as_tensor(truth).double().reshape(1, -1)
        return (truth + s * torch.randn(n, truth.shape[1], generator=g, dtype=torch.float64)).float()
    yield 'quadratic', SumOfSquares((64,)), torch.randn(n, 64, generator=g)
    yield 'funnel', Funnel((64,)), torch.randn(n, 64, generator=g)
    b = torch.randn(64, 64, generator=g, dtype=torch.float64)
    yield 'fullrank', P.FullRankGaussian(torch.zeros(64, dtype=torch.float64), precision=b @ b.T / 64 + torch.eye(64, dtype=torch.float64)), \
        torch.randn(n, 64, generator=g)
    yield 'rosenbrock', P.Rosenbrock((64,)), 1.0 + 0.1 * torch.randn(n, 64, generator=g)
    yield 'stochastic_volatility', P.StochasticVolatility(0.5 * torch.randn(100, generator=g)), 0.1 * torch.randn(n, 103, generator=g)
    D = 25
    X, y, _ = synthetic(1000, D, 0)
    yield 'sparse_logreg', SparseLogisticRegression(X, y), start_states(D, n, 1, spread=0.5).float()
    yield 'phi4', P.LatticePhi4((8, 8)), 1.0 + 0.3 * torch.randn(n, 64, generator=g)
    irt, truth = ItemResponseTheory.synthetic(100, 27, 0, missing=0.25)
    yield 'item_response', irt, near(truth, 0.1)
    vfx, truth = P.VaryingEffectsRegression.synthetic(85, 919, 0, intercepts='varying', slopes='varying')
    yield 'varying_effects', vfx, near(truth)
    ps = P.ParticleSystem(13)
    yield 'particles', ps, ps.start_states(n, 0, 0.03 * ps.spacing).float()
    lgm, truth = P.LatentGaussianModel.synthetic(256, 'poisson', 1, mean=1.0)
    yield 'latent_gaussian', lgm, near(truth)
    gmrf, truth = P.LatentGMRF.synthetic(256, 'rw2', 'poisson', 3, mean=1.0)
    yield 'latent_gmrf', gmrf, near(truth)
    bridge, truth = P.DiffusionBridge.synthetic(32, 'fitzhugh_nagumo', 7)
    yield 'diffusion_bridge', bridge, near(truth, 0.01)


def sweep(sizes, steps=50):
    """fused and split ms per transition of every kind at every chain count; one JSON line"""
    res = {'unit': 'ms per transition through sample() (all chains); median of %d alternated calls of %d transitions' % (REPS, steps),
           'cases': []}
    for n in sizes:
        for name, pot, z0 in kinds(n):
            d = z0.shape[1]
            torch.manual_seed(d)
            flow = create_flow_object('realnvp', (d,))
            runs = {label: make(label, d, pot, flow, steps) for label in ('fused', 'split')}
            for s in runs.values():
                s.sample(z0, show_progress=False)
            times = {label: [] for label in runs}
            for _ in range(REPS):
                for label, s in runs.items():
                    times[label].append(ev_ms(lambda: s.sample(z0, show_progress=False)) / steps)
            row = {'kind': name, 'd': d, 'n': n, 'fused': round(statistics.median(times['fused']), 4),
                   'split': round(statistics.median(times['split']), 4)}
            row['split_over_fused'] = round(row['split'] / row['fused'], 2)
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
    print(json.dumps(res))


def main():
    torch.cuda.set_device(0)
    if '--kinds' in sys.argv:
        return sweep([int(v) for v in sys.argv[sys.argv.index('--kinds') + 1:]] or [65536, 1024])
    res = {'unit': 'ms per transition (all chains); median, min, max of %d alternated calls of %d transitions' % (REPS, STEPS),
           'n': N, 'cases': []}
    for name, d, flow_name, pot, z0 in problems():
        torch.manual_seed(d)
        flow = create_flow_object(flow_name, (d,))
        runs = {label: make(label, d, pot, flow) for label in ('fused', 'split', 'hmc1')}
        routes = {}
        for label, s in runs.items():                                   # warm this shape, and see which route it takes
            calls = []
            orig = s.inner_sampler.sample
            s.inner_sampler.sample = lambda *a, _o=orig, _c=calls, **k: _c.append(1) or _o(*a, **k)
            s.sample(z0, show_progress=False)
            routes[label] = 'split' if calls else 'fused'
            s.inner_sampler.sample = orig
        assert routes == {'fused': 'fused', 'split': 'split', 'hmc1': 'fused'}, routes
        times = {label: [] for label in runs}
        for _ in range(REPS):
            for label, s in runs.items():
                times[label].append(ev_ms(lambda: s.sample(z0, show_progress=False)) / STEPS)
        row = {'target': name, 'd': d, 'flow': flow_name}
        for label, t in times.items():
            row[label] = round(statistics.median(t), 4)
            row[label + '_min_max'] = [round(min(t), 4), round(max(t), 4)]
        row['split_over_fused'] = round(row['split'] / row['fused'], 2)
        row['hmc1_over_fused'] = round(row['hmc1'] / row['fused'], 2)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
