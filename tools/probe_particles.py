"""Interacting particles on the device: ms per transition (all chains) at the double well of four particles in the plane
(DW4, d = 8) and at the Lennard-Jones clusters of 13 and 55 particles in space (LJ13, d = 39; LJ55, d = 165), at 4096 and
65536 chains, on the fused kernels (the ParticleSystem object) against the split path of the same build (the same object
behind a plain lambda, fuse='never'), for mala, hmc (L = 5), jump_mala (one outer iteration of 10 mala transitions and a
jump, per outer iteration; jump_mala_tail: the same with a conditioner of 8 units and the jump fused into the mala launch,
`fuse_jump_tail`, beside that flow without the tail), imh (per flow-MH transition) and neutra_hmc (L = 5, conditioner of 8 units; per trajectory).
Chains start at ParticleSystem.start_states(n, 0, jitter 0.03 of the spacing); mass diagonals (the median positive diagonal
Hessian over 8 starts) and steps as in tests/test_gpu_particles.py.  The flows are untrained: their proposals put the
particles of a Lennard-Jones cluster on top of each other and are rejected, which costs the kernels the same P (P - 1) pair evaluations as any other proposal (the
pair loop has a uniform trip count).  The split path evaluates ParticleSystem.__call__, which chunks over chains; autograd
still keeps every chunk's (chunk, P, P, D) tensors until the backward pass, so where it runs out of device memory the row
says so and gives the largest n, halving from the one asked for, at which it ran.  HIP events around the whole sample()
call after one warm-up call, REPS repetitions: median, min and max per case; one JSON line.

    python tools/probe_particles.py [n_chains ...]        (default 4096 65536)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfmc_amd.containers import NFMCKernel  # noqa: E402
from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import ParticleSystem  # noqa: E402
from nfmc_amd.samplers import imh, jump, mcmc, neutra  # noqa: E402
from nfmc_amd.util import create_flow_object  # noqa: E402

REPS = 3
SYSTEMS = {'DW4': (4, 2, 'double_well', ParticleSystem.double_well_4),
           'LJ13': (13, 3, 'lennard_jones', lambda: ParticleSystem.lennard_jones(13)),
           'LJ55': (55, 3, 'lennard_jones', lambda: ParticleSystem.lennard_jones(55))}
MALA_STEP = {'lennard_jones': 0.125, 'double_well': 1.0}      # tests/test_gpu_particles.py
HMC_STEP = {'lennard_jones': 0.25, 'double_well': 1.0}


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
    """the diagonal of the Hessian of U at the fp64 states x (n, d), by autograd on the CPU"""
    t = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(pot(t).sum(), t, create_graph=True)
    return torch.stack([torch.autograd.grad(g[:, c].sum(), t, retain_graph=True)[0][:, c] for c in range(x.shape[1])], dim=1).detach()


def make(strategy, pot, target, fuse, H, steps):
    d = pot.event_size
    h_mala = MALA_STEP[pot.pair] * min(0.5, 2.5 * d ** (-1 / 3))
    h_hmc = HMC_STEP[pot.pair] * min(0.4, 1.6 * d ** (-1 / 4))
    if strategy == 'mala':
        s = mcmc.MALA((d,), target, mcmc.LangevinKernel(event_size=d, step_size=h_mala, inv_mass_diag=torch.sqrt(H).float()),
                      mcmc.LangevinParameters(n_iterations=steps, store_samples=False))
    elif strategy == 'hmc':
        s = mcmc.HMC((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=5, step_size=h_hmc, inv_mass_diag=(1 / H).float()),
                     mcmc.HMCParameters(n_iterations=steps, store_samples=False))
    elif strategy in ('jump_mala', 'jump_mala_tail', 'jump_mala_no_tail'):
        # the default flow, or a conditioner of 8 units with the jump fused into the mala launch (its tail) or not
        flow = create_flow_object('realnvp', (d,)) if strategy == 'jump_mala' else Flow(RealNVP((d,), conditioner_kwargs={'n_hidden': 8}))
        s = jump.JumpMALA((d,), target, NFMCKernel((d,), flow=flow),
                          jump.JumpNFMCParameters(n_iterations=steps, store_samples=False),
                          mcmc.LangevinKernel(event_size=d, step_size=h_mala, inv_mass_diag=torch.sqrt(H).float()),
                          mcmc.LangevinParameters(n_iterations=10))
        s.fuse_jump_tail = strategy == 'jump_mala_tail'
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
    sizes = [int(v) for v in sys.argv[1:]] or [4096, 65536]
    res = {'unit': 'ms per transition (all chains), median of %d calls' % REPS, 'cases': []}
    for name, (P, D, pair, build) in SYSTEMS.items():
        pot = build()
        d = pot.event_size
        h = hess_diag(pot, pot.start_states(8, 1, 0.03 * pot.spacing))
        pos = torch.where(h > 0, h, torch.full_like(h, float('nan'))).nanmedian(0).values
        H = torch.where(torch.isnan(pos), h.abs().median(0).values, pos)
        for n in sizes:
            x0 = pot.start_states(n, 0, 0.03 * pot.spacing).float()
            for strategy in ('mala', 'hmc', 'jump_mala', 'jump_mala_tail', 'imh', 'neutra_hmc'):
                row = {'system': name, 'strategy': strategy, 'n': n, 'd': d}
                fsteps = {'mala': 10, 'hmc': 5, 'jump_mala': 2, 'jump_mala_tail': 2, 'imh': 5, 'neutra_hmc': 3}[strategy]
                row['fused'], row['fused_min_max'] = timed(make(strategy, pot, pot, 'auto', H, fsteps), x0, fsteps)
                if strategy == 'jump_mala_tail':     # the same flow with the jump on the flow-MH kernel instead
                    row['fused_no_tail'], row['fused_no_tail_min_max'] = timed(make('jump_mala_no_tail', pot, pot, 'auto', H, fsteps), x0, fsteps)
                m = n
                while m >= 64:     # the split path: at n, or at the largest n / 2^k that fits the device's memory
                    try:
                        row['split'], row['split_min_max'] = timed(make(strategy, pot, lambda x: pot(x), 'never', H, 1), x0[:m], 1)
                        break
                    except torch.cuda.OutOfMemoryError:
                        torch.cuda.empty_cache()
                        m //= 2
                if m != n:
                    row['split_n'] = m
                    row['note'] = 'the split path cannot hold %d chains; %d is its largest feasible n of the halving search' % (n, m)
                    row['fused_at_split_n'], _ = timed(make(strategy, pot, pot, 'auto', H, fsteps), x0[:m], fsteps)
                    row['speedup'] = round(row['split'] / row['fused_at_split_n'], 2)
                else:
                    row['speedup'] = round(row['split'] / row['fused'], 2)
                print(json.dumps(row), file=sys.stderr, flush=True)
                res['cases'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
