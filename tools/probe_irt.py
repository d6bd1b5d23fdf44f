"""Item-response theory on the device: ms per mala transition and per hmc trajectory (L = 5) at the Inference Gym's shape
(S = 400 students, Q = 100 questions, d = 501) on ItemResponseTheory.synthetic(400, 100, 0), at 4096 and 65536 chains, on
the fused kernels (the ItemResponseTheory object) against the split path of the same build (fuse='never'), and the jump of
jump_mala with the default flow (one outer iteration of 10 mala transitions and a jump, minus 10 transitions; `jump_on_flow_mh_kernel` says whether nfmc_flow_mh_supported_f32 took the flow).  Chains
start one posterior standard deviation around the generating state; mass diagonals and steps as in
tests/test_gpu_irt.py.  HIP events around the whole sample() call after one warm-up call, REPS repetitions: median, min
and max per case; one JSON line.

    python tools/probe_irt.py [n_chains ...]        (default 4096 65536)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.potentials import ItemResponseTheory  # noqa: E402
from nfmc_amd.samplers import jump, mcmc  # noqa: E402
from nfmc_amd.util import create_flow_object  # noqa: E402

REPS = 5
S, Q = 400, 100


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


def hess_diag(pot, x):
    """diagonal Hessian of U at one state x (d,), fp64"""
    mu, a, b = pot.unpack(x)
    p = torch.sigmoid(mu + a[:, None] - b[None, :])
    v = pot.observed * p * (1 - p)
    return torch.cat([pot.p_a + v.sum(1), pot.p_b + v.sum(0), (pot.p_mu + v.sum()).reshape(1)])


def make(strategy, d, target, fuse, H, steps):
    if strategy == 'mala':
        s = mcmc.MALA((d,), target, mcmc.LangevinKernel(event_size=d, step_size=2.0 * d ** (-1 / 3), inv_mass_diag=torch.sqrt(H).float()),
                      mcmc.LangevinParameters(n_iterations=steps, store_samples=False))
    else:
        s = mcmc.HMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=1.6 * d ** (-1 / 4),
                                                  inv_mass_diag=(1 / H).float()),
                     mcmc.HMCParameters(n_iterations=steps, store_samples=False))
    s.seed, s.fuse = 1, fuse
    return s


def timed(s, x0, steps):
    s.sample(x0, show_progress=False)
    t = [ms / steps for ms in ev_ms(lambda: s.sample(x0, show_progress=False))]
    return round(statistics.median(t), 4), [round(min(t), 4), round(max(t), 4)]


def main():
    torch.cuda.set_device(0)
    counts = [int(v) for v in sys.argv[1:]] or [4096, 65536]
    pot, truth = ItemResponseTheory.synthetic(S, Q, 0)
    d = pot.event_size
    H = hess_diag(pot, truth)
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'S': S, 'Q': Q, 'd': d,
           'observed': int(pot.observed.sum()), 'cases': []}
    for n in counts:
        g = torch.Generator().manual_seed(n)
        x0 = (truth + torch.randn(n, d, generator=g, dtype=torch.float64) / torch.sqrt(H)).float()
        for strategy in ('mala', 'hmc'):
            row = {'strategy': strategy, 'n': n}
            for label, target, fuse, steps in (('fused', pot, 'auto', 10 if strategy == 'mala' else 5),
                                               ('split', lambda x: pot(x), 'never', 2)):
                row[label], row[label + '_min_max'] = timed(make(strategy, d, target, fuse, H, steps), x0, steps)
            row['speedup'] = round(row['split'] / row['fused'], 2)
            print(json.dumps(row), file=sys.stderr, flush=True)
            res['cases'].append(row)
        # the jump of jump_mala with the default flow: one outer iteration (10 mala transitions + 1 jump) against 10 transitions
        flow = create_flow_object('realnvp', (d,))
        s = jump.JumpMALA((d,), pot, NFMCKernel((d,), flow=flow), jump.JumpNFMCParameters(n_iterations=1, store_samples=False),
                          mcmc.LangevinKernel(event_size=d, step_size=2.0 * d ** (-1 / 3), inv_mass_diag=torch.sqrt(H).float()),
                          mcmc.LangevinParameters(n_iterations=10))
        s.seed = 1
        answers, asked = [], jump.flow_mh_supported
        jump.flow_mh_supported = lambda *a, **k: answers.append(asked(*a, **k)) or answers[-1]
        outer, mm = timed(s, x0, 1)
        jump.flow_mh_supported = asked
        mala = next(c['fused'] for c in res['cases'] if c['n'] == n and c['strategy'] == 'mala')
        row = {'strategy': 'jump_mala', 'n': n, 'outer_iteration': outer, 'outer_min_max': mm, 'jump': round(outer - 10 * mala, 4),
               'jump_on_flow_mh_kernel': bool(answers) and all(answers)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
