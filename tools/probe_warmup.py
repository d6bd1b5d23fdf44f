"""Cost of a warmup at the C3 shape (65536 x 64): 100 tuning transitions vs 100 sampling transitions.

    python tools/probe_warmup.py          MALA: host / device controller, fold levels, tune_every
    python tools/probe_warmup.py hmc      HMC: the device warmup with the trajectory-length adaptation off, on, and on with
                                          the leapfrog count pinned by max_leapfrog_steps (median and range of 5)
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nfmc_amd.samplers import mcmc
from nfmc_amd.potentials import SumOfSquares

d, n, K = 64, 65536, 100
x0 = (torch.randn(n, d, generator=torch.Generator().manual_seed(0)) * 0.7071).cuda()


def timed(fn, reps=4):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3


def sampling():
    s = mcmc.MALA((d,), SumOfSquares((d,)), None, mcmc.LangevinParameters(n_iterations=K, store_samples=False))
    s.seed = 1
    s.sample(x0, show_progress=False)


def warmup(every, device=True):
    os.environ['NFMC_TUNE_DEVICE'] = '1' if device else '0'
    s = mcmc.MALA((d,), SumOfSquares((d,)), None, mcmc.LangevinParameters(n_warmup_iterations=K, store_samples=False, tune_every=every))
    s.seed = 1
    s.warmup(x0, show_progress=False)
    return s.kernel.step_size


def hmc_warmup(L=5, **params):
    s = mcmc.HMC((d,), SumOfSquares((d,)), mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=0.05),
                 mcmc.HMCParameters(n_warmup_iterations=K, store_samples=False, **params))
    s.seed = 1
    out = s.warmup(x0, show_progress=False)
    return s, out


def hmc_leg(reps=5):
    legs = [('option off, L = 5', dict()),
            ('option on', dict(tune_trajectory_length=True)),
            ('option on, L pinned at 5', dict(tune_trajectory_length=True, max_leapfrog_steps=5))]
    times = {name: [] for name, _ in legs}
    hmc_warmup()                                    # code objects loaded, allocator warm
    for _ in range(reps):                           # alternating: the legs see the same machine state
        for name, kw in legs:
            torch.cuda.synchronize(); t0 = time.perf_counter(); s, out = hmc_warmup(**kw); torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            if kw and len(times[name]) == reps:
                steps = out.statistics.n_target_gradient_calls / (2 * n)
                print('  %s: T-bar %.3f, step %.4f, %.1f leapfrog steps per transition' % (
                    name, s.kernel.trajectory_length, s.kernel.step_size, steps / K))
    for name, _ in legs:
        t = sorted(times[name])
        print('hmc warmup, %d transitions, %-26s: median %.2f ms (%.2f .. %.2f)' % (K, name, t[len(t) // 2], t[0], t[-1]))


if sys.argv[1:2] == ['hmc']:
    hmc_leg()
    sys.exit(0)

t_s = timed(sampling)
print('sampling, %d transitions: %.2f ms' % (K, t_s))
for every, device, one_level in [(1, False, False), (1, True, True), (1, True, False), (5, True, False), (10, True, False), (25, True, False)]:
    if one_level:   # round 2-3: tuning launches of 256 workgroups, one workgroup folds their slabs
        os.environ['NFMC_TUNE_ONE_LEVEL'] = '1'
    else:
        os.environ.pop('NFMC_TUNE_ONE_LEVEL', None)
    t = timed(lambda: warmup(every, device))
    print('warmup tune_every=%-3d %-6s %-22s: %.2f ms  (%.1fx sampling)  tuned step %.4f' % (
        every, 'device' if device else 'host', '(256 workgroups, 1 fold)' if one_level else '', t, t / t_s, warmup(every, device)))
