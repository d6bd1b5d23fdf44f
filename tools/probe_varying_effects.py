"""Varying-effects regression on the device: ms per transition (all chains) at the radon shape (C = 85 groups, N = 919
observations, both sides varying, d = 175) and at C = 509 (N = 5499, d = 1023) on VaryingEffectsRegression.synthetic(C, N, 0),
65536 chains, on the fused kernels (the VaryingEffectsRegression object) against the split path of the same build (the same
object behind a plain lambda, fuse='never'), for mala, hmc (L = 5), jump_mala (one outer iteration of 10 mala transitions
and a jump, per outer iteration), imh (per flow-MH transition) and neutra_hmc (L = 5, conditioner of 8 units; per
trajectory).  Chains start one posterior standard deviation around the generating state; mass diagonals and steps as in
tests/test_gpu_varying_effects.py.  HIP events around the whole sample() call after one warm-up call, REPS repetitions:
median, min and max per case; one JSON line.

    python tools/probe_varying_effects.py [n_chains [C ...]]        (default 65536 85 509)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import VaryingEffectsRegression  # noqa: E402
from nfmc_amd.samplers import imh, jump, mcmc, neutra  # noqa: E402
from nfmc_amd.util import create_flow_object  # noqa: E402
from varying_effects_fp64 import VFX64  # noqa: E402

REPS = 3
SHAPES = {85: 919, 509: 5499}


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


def make(strategy, d, target, fuse, H, steps):
    h_mala, h_hmc = min(0.5, 2.5 * d ** (-1 / 3)), min(0.4, 1.6 * d ** (-1 / 4))
    if strategy == 'mala':
        s = mcmc.MALA((d,), target, mcmc.LangevinKernel(event_size=d, step_size=h_mala, inv_mass_diag=torch.sqrt(H).float()),
                      mcmc.LangevinParameters(n_iterations=steps, store_samples=False))
    elif strategy == 'hmc':
        s = mcmc.HMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=h_hmc, inv_mass_diag=(1 / H).float()),
                     mcmc.HMCParameters(n_iterations=steps, store_samples=False))
    elif strategy == 'jump_mala':
        s = jump.JumpMALA((d,), target, NFMCKernel((d,), flow=create_flow_object('realnvp', (d,))),
                          jump.JumpNFMCParameters(n_iterations=steps, store_samples=False),
                          mcmc.LangevinKernel(event_size=d, step_size=h_mala, inv_mass_diag=torch.sqrt(H).float()),
                          mcmc.LangevinParameters(n_iterations=10))
    elif strategy == 'imh':
        s = imh.FixedIMH((d,), target, imh.IMHKernel((d,), flow=create_flow_object('realnvp', (d,))),
                         imh.IMHParameters(n_iterations=steps, store_samples=False))
    else:
        flow = Flow(RealNVP((d,), conditioner_kwargs={'n_hidden': 8}))
        s = neutra.NeuTraHMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=0.5 * h_hmc),
                             mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=flow),
                             neutra.NeuTraParameters(n_iterations=steps, store_samples=False))
    s.seed, s.fuse = 1, fuse
    return s


def timed(s, x0, steps):
    s.sample(x0, show_progress=False)
    t = [ms / steps for ms in ev_ms(lambda: s.sample(x0, show_progress=False))]
    return round(statistics.median(t), 4), [round(min(t), 4), round(max(t), 4)]


def main():
    torch.cuda.set_device(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    groups = [int(v) for v in sys.argv[2:]] or [85, 509]
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'n': n, 'cases': []}
    for C in groups:
        N = SHAPES.get(C, 10 * C)
        pot, truth = VaryingEffectsRegression.synthetic(C, N, 0, intercepts='varying', slopes='varying')
        d = pot.event_size
        ref = VFX64(pot.y, pot.group, pot.x, 'varying', 'varying')
        H = ref.hess_diag(truth[None])[0]
        g = torch.Generator().manual_seed(n)
        x0 = (truth + torch.randn(n, d, generator=g, dtype=torch.float64) / torch.sqrt(H)).float()
        for strategy in ('mala', 'hmc', 'jump_mala', 'imh', 'neutra_hmc'):
            row = {'strategy': strategy, 'C': C, 'N': N, 'd': d}
            fsteps = {'mala': 10, 'hmc': 5, 'jump_mala': 2, 'imh': 5, 'neutra_hmc': 3}[strategy]
            try:
                for label, target, fuse, steps in (('fused', pot, 'auto', fsteps), ('split', lambda x: pot(x), 'never', 1)):
                    row[label], row[label + '_min_max'] = timed(make(strategy, d, target, fuse, H, steps), x0, steps)
                row['speedup'] = round(row['split'] / row['fused'], 2)
            except ValueError as e:   # a shape a sampler refuses: say so (any other error ends the probe)
                row['error'] = str(e)[:200]
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
