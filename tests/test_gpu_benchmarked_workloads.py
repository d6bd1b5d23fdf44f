"""Every workload bench.py measures, on its FITTED flow and its own step size, followed through long runs transition by
transition against the fp64 oracle (shadowing, oracle/shadow.py).

The config-exact tests of test_gpu_configs.py compare whole runs with the fp32 oracle on near-identity flows and small
steps; the bench samples with fitted flows, whose conditioners sit deep in tanh saturation, whose coupling scales span
orders of magnitude and whose funnel chains reach |x0| well away from 0 (C4 also takes a 15x longer leapfrog step).
Here the kernels run exactly the sampler bench.build_sampler builds (store_samples switched on), with the flow weights
of bench.fitted_flow_state, from bench.initial_state, on 512 chains (several chain tiles and lane groups), and every
kept transition is recomputed in fp64 from the kernel's own pre-state with the same Philox step and tag.

Tolerance (oracle/shadow.py): decisions exact outside the tie window delta = max(1e-5 (1 + |H0| + |H1|), 8 |m32 - m64|)
(|U| + |log q| of both points for flow-proposal MH / IMH, |U0| + |U1| for MALA; m32 - m64 the fp32 oracle's margin error);
states on commonly accepted transitions within kappa x the fp32 oracle's own error against fp64, per transition:
max e <= kappa max e32 + 1e-6 (1 + max|x64|), mean e <= kappa / 2 mean e32 + 1e-7.

Observed on the MI355X (worst transition of the run; "needed" = the smallest kappa each bound passes with):

    workload   max e / max e32   mean e / mean e32   kappa needed (max, mean)   near ties   acceptance (inner, jump)
    C4         4.21              1.99                2.44, 3.84                 0.27 %      0.860
    wide       2.64              2.84                1.86, 5.51                 0.39 %      0.758 (h = 0.2)
    C3         3.64              2.05                0.00, 1.99                 0.03 %      0.335, 0.785  (launch and tail alike)
    C5         1.44              1.47                0.00, 2.25                 0.33 %      0.993, 0.548
    C2         2.36              1.48                0.00, 1.99                 0.18 %      0.857

and on the states after trajectory 20 the gradient, potential, inverse and forward kernels needed kappa <= 3.19 (C4) /
2.13 (wide).  So KAPPA = 8 leaves 1.45x headroom over the worst (the wide run's mean bound).  No clear-margin decision
differed from fp64 in any run; the mutated C4 run needed kappa 318.  A tie window of 1e-4 (1 + |H0| + |H1|) skipped 1.7 % (C2) to 4.1 % (C5) of the decisions: near-unit
acceptance puts most margins within 0.05 of zero when |H0| + |H1| ~ 500, while the fp32 margin rounding measured
<= 2.2e-7 (1 + |H0| + |H1|) on C2, C3, C5 and up to 7e-5 (C4) / 3.5e-3 (wide) only on funnel trajectories that amplify
it -- hence the smaller fixed coefficient and the per-chain term.
NFMC_SHADOW_LOG=<file> appends each workload's summary as a JSON line.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import bench
from oracle import potentials as opot, samplers as osamp, shadow

pytestmark = pytest.mark.gpu

N = 512
KAPPA = 8.0
ACC_TOL = 0.1
# bench-measured acceptance (BENCH_r04.json, one bench step each): (inner / trajectories, jumps)
BENCH_ACC = {'C4': (0.925, None), 'C3': (0.35, 0.80), 'C5': (0.994, 0.548), 'C2': (None, 0.856)}
# the bench's kernel parameters; the test fails if bench.build_sampler ever builds something else
BENCH_PARAMS = {'C4': dict(h=0.3, L=10), 'C3': dict(h=64 ** (-1 / 3), K=100), 'C5': dict(h=0.05, L=20, K=5), 'C2': dict()}
# wide-event NeuTra (not a bench config): funnel d = 256, conditioner 128 x 2, flow fitted like C4's
WIDE_D, WIDE_H, WIDE_L = 256, 0.2, 10


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module', autouse=True)
def _oracle_threads():
    """The oracle's small CPU GEMMs slow down on many threads: at most 16 while this module runs."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def _log(name, summary):
    path = os.environ.get('NFMC_SHADOW_LOG')
    if path:
        with open(path, 'a') as fh:
            fh.write(json.dumps({'workload': name, **{k: float(v) for k, v in summary.items()}}) + '\n')


def _check(rep, name, kappa=KAPPA):
    s = rep.summary()
    _log(name, s)
    fails = rep.failures(kappa)
    assert not fails, (name, fails, s)
    return s


def _no_split(sampler):
    def boom(*a, **k):
        raise AssertionError('NeuTra took the split path: the fused matrix-core kernel did not run')
    sampler.inner_sampler.sample = boom


def _acc_close(got, want, name):
    assert abs(got - want) <= ACC_TOL, (name, got, want)


def _bench_run(name, dev, n_steps, seed, flow_state=None):
    """bench.build_sampler's sampler for `name` (n_steps bench steps, fitted flow), kept states on; returns the sampler,
    x0 and the oracle flow with the bench's weights."""
    cfg = bench.CONFIGS[name]
    state = bench.fitted_flow_state(name, cfg, dev)
    s = bench.build_sampler(cfg, n_steps, flow_state=flow_state if flow_state is not None else state)
    s.params.store_samples = True
    s.seed = seed
    fcfg = dict(cfg, _flow_state=state)
    x0 = bench.initial_state(fcfg, N)
    return s, x0, bench._oracle_flow(fcfg)


# ================================================================================================ NeuTra (C4, wide)
def _neutra_kernel_checks(s, z, of, name, kappa=KAPPA):
    """On visited latent states z (n, d): the adjusted potential and its gradient from nfmc_neutra_potential_grad_f32, and
    the flow's inverse and forward kernels, against fp64 (autograd through the oracle flow), with the fp32 CPU oracle as
    the yardstick.  Gradient errors per chain relative to that chain's |grad U~64|_inf, potential errors relative to
    1 + |U~64|."""
    d = z.shape[1]
    of64 = copy.deepcopy(of).double()
    fun = opot.funnel(3.0)
    u, g = s._potential_grad(z)
    u, g = u.cpu().double(), g.cpu().double()
    u64, g64 = osamp._value_and_grad(osamp.neutra_adjusted_target(of64, fun, (d,)), z.double())
    u32, g32 = osamp._value_and_grad(osamp.neutra_adjusted_target(of, fun, (d,)), z.clone())
    gn = g64.abs().amax(dim=1)
    eg, eg32 = (g - g64).abs().amax(dim=1) / gn, (g32.double() - g64).abs().amax(dim=1) / gn
    eu, eu32 = (u - u64).abs() / (1 + u64.abs()), (u32.double() - u64).abs() / (1 + u64.abs())
    errs = [('grad', eg, eg32, 1e-6), ('potential', eu, eu32, 1e-6)]
    # the flow kernels: inverse on z, forward on the fp64 inverse image (rounded to fp32)
    x, ld = s.kernel.flow.bijection.inverse(z.cuda())
    with torch.no_grad():
        x64, ld64 = of64.bijection.inverse(z.double())
        x32, ld32 = of.bijection.inverse(z.clone())
        xin = x64.float()
        zf, ldf = s.kernel.flow.bijection.forward(xin.cuda())
        zf64, ldf64 = of64.bijection.forward(xin.double())
        zf32, ldf32 = of.bijection.forward(xin.clone())
    for what, k, r64, r32 in (('inverse', x, x64, x32), ('inverse_logdet', ld, ld64, ld32),
                              ('forward', zf, zf64, zf32), ('forward_logdet', ldf, ldf64, ldf32)):
        k, r32 = k.cpu().double().reshape(r64.shape[0], -1), r32.double().reshape(r64.shape[0], -1)
        r64 = r64.reshape(r64.shape[0], -1)
        errs.append((what, (k - r64).abs().amax(dim=1), (r32 - r64).abs().amax(dim=1), 1e-6 * (1 + float(r64.abs().max()))))
    res = {what: shadow.calibrated(e.numpy(), e32.numpy(), floor, 1e-7, kappa) for what, e, e32, floor in errs}
    _log(name + ' kernels', {'%s_kappa_%s' % (w, b): r[i] for w, r in res.items() for i, b in ((2, 'max'), (3, 'mean'))})
    for what, e, e32, _floor in errs:
        assert res[what][0] and res[what][1], (name, what, float(e.max()), float(e32.max()), float(e.mean()), float(e32.mean()))


def _neutra_shadow(s, z0, of, h, L, T, seed, name):
    _no_split(s)
    out = s.sample(z0, show_progress=False)
    states = torch.cat([z0[None], out.samples.reshape(T, N, -1).cpu()])
    rep = shadow.shadow(states, shadow.Workload('neutra_hmc', opot.funnel(3.0), of, h, L), seed)
    return out, states, rep


def test_C4_fitted_flow_h03_shadowed_40_trajectories(dev):
    """C4 as bench.py runs it: neutra_hmc on the funnel, d = 128, conditioner 128 x 2 fitted by the bench's variational
    fit, h = 0.3, L = 10, on `neutra_leapfrog_mfma_kernel` (the split path is patched out), 40 trajectories shadowed;
    then the gradient kernel and the flow kernels on the states after trajectory 20."""
    T, seed = 40, 4242
    s, z0, of = _bench_run('C4', dev, T, seed)
    k = s.inner_sampler.kernel
    assert (k.step_size, k.n_leapfrog_steps) == (BENCH_PARAMS['C4']['h'], BENCH_PARAMS['C4']['L'])
    assert bool((k.inv_mass_diag == 1).all())
    out, states, rep = _neutra_shadow(s, z0, of, k.step_size, k.n_leapfrog_steps, T, seed, 'C4')
    sm = _check(rep, 'C4')
    st = out.statistics
    L = k.n_leapfrog_steps
    assert st.n_attempted_trajectories == N * T and st.n_accepted_trajectories == rep.accepted_inner
    assert st.n_target_calls == (2 * L + 2) * N * T and st.n_target_gradient_calls == 2 * L * N * T   # hmc.py:122-125
    _acc_close(sm['acceptance_inner'], BENCH_ACC['C4'][0], 'C4')
    _neutra_kernel_checks(s, states[20], of, 'C4')


def test_C4_shadow_flags_a_shifted_output_bias_in_the_kernels_flow(dev):
    """The harness can fail on the GPU: the same C4 run with one output bias of one coupling shifted by 1e-3 in the
    kernel's flow only, against the unmodified fp64 oracle, must be flagged."""
    T, seed = 5, 4242
    state = copy.deepcopy(bench.fitted_flow_state('C4', bench.CONFIGS['C4'], dev))
    key = 'bijection.layers.2.conditioner.2.bias'
    state[key][state[key].shape[0] // 2] += 1e-3          # a shift (beta) of one target coordinate of coupling 1
    s, z0, of = _bench_run('C4', dev, T, seed, flow_state=state)
    k = s.inner_sampler.kernel
    _out, _states, rep = _neutra_shadow(s, z0, of, k.step_size, k.n_leapfrog_steps, T, seed, 'C4 mutated')
    fails = rep.failures(KAPPA)
    _log('C4 mutated', {**rep.summary(), 'flagged': float(bool(fails))})
    assert any(f.startswith('states') or 'decisions' in f for f in fails), fails


@pytest.fixture(scope='module')
def wide_flow_state(dev):
    """The wide workload's flow, fitted the way bench.fitted_flow_state fits C4's: the default-seeded RealNVP with a
    128 x 2 conditioner, variational (reverse-KL) fit to the funnel, 200 epochs of 1024 latents, lr 0.01, torch.manual_seed(1).
    The device fit kernels do not take this shape, so the fit runs through torch ops on the GPU."""
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.potentials import Funnel
    pot = Funnel((WIDE_D,), 3.0)
    torch.manual_seed(1)
    f = Flow(RealNVP((WIDE_D,), conditioner_kwargs={'n_hidden': 128, 'n_layers': 2})).to(dev)
    f.variational_fit(lambda v: -pot(v), n_epochs=200, lr=0.01, n_samples=1024, early_stopping=False,
                      keep_best_weights=True, show_progress=False, potential=pot)
    return {k: v.detach().cpu().clone() for k, v in f.state_dict().items()}


def test_wide_event_neutra_fitted_flow_shadowed_20_trajectories(dev, wide_flow_state):
    """NeuTra on the funnel at d = 256 with C4's conditioner (128 x 2), fitted flow: no fused trajectory kernel exists for
    d > 128, the trajectory is composed from the streamed matrix-core kernels of csrc/mfma_wide.hip (whose LDS weight
    staging alternates between two images).  h = WIDE_H puts the acceptance in [0.6, 0.95].  20 trajectories shadowed,
    then the gradient and flow kernels on the states after trajectory 20."""
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.potentials import Funnel
    from nfmc_amd.samplers import mcmc, neutra
    from oracle import flow as oflow
    T, seed = 20, 777
    f = Flow(RealNVP((WIDE_D,), conditioner_kwargs={'n_hidden': 128, 'n_layers': 2}))
    f.load_state_dict(wide_flow_state)
    of = oflow.Flow(oflow.RealNVP((WIDE_D,), conditioner_kwargs={'n_hidden': 128, 'n_layers': 2}))
    of.load_state_dict(wide_flow_state)
    s = neutra.NeuTraHMC((WIDE_D,), Funnel((WIDE_D,), 3.0),
                         mcmc.HMCKernel(event_size=WIDE_D, n_leapfrog_steps=WIDE_L, step_size=WIDE_H),
                         mcmc.HMCParameters(), neutra.NeuTraKernel((WIDE_D,), flow=f), neutra.NeuTraParameters(n_iterations=T))
    s.seed = seed
    z0 = torch.randn(N, WIDE_D, generator=torch.Generator().manual_seed(0))
    out, states, rep = _neutra_shadow(s, z0, of, WIDE_H, WIDE_L, T, seed, 'wide')
    sm = _check(rep, 'wide')
    st = out.statistics
    assert st.n_attempted_trajectories == N * T and st.n_accepted_trajectories == rep.accepted_inner
    assert st.n_target_calls == (2 * WIDE_L + 2) * N * T and st.n_target_gradient_calls == 2 * WIDE_L * N * T
    assert 0.6 <= sm['acceptance_inner'] <= 0.95, sm
    _neutra_kernel_checks(s, states[T], of, 'wide')


# ================================================================================================ jumps (C3, C5)
def _jump_run(name, dev, T, seed, monkeypatch, tail=False):
    from nfmc_amd.samplers import jump
    s, x0, of = _bench_run(name, dev, T, seed)
    monkeypatch.setattr(jump.JumpNFMC, 'fuse_jump_tail', tail)
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: (_ for _ in ()).throw(AssertionError('split jump')))
    s.inner_sampler._split_step = lambda *a, **k: (_ for _ in ()).throw(AssertionError('split inner step'))
    launches, tails = [], []
    orig_launch, orig_tail = jump.launch_flow_mh, jump.make_jump_tail
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: (launches.append(1), orig_launch(*a, **k))[1])
    monkeypatch.setattr(jump, 'make_jump_tail', lambda *a, **k: (tails.append(1), orig_tail(*a, **k))[1])
    out = s.sample(x0.to(dev), show_progress=False)
    if tail:
        assert len(tails) == T and not launches, 'the jump did not ride as the tail of the inner launch'
    else:
        assert len(launches) == T and not tails, 'the jump did not run on nfmc_flow_mh_steps_f32'
    return s, x0, of, out


def _jump_shadow(name, dev, T, seed, monkeypatch, inner_kind, tail=False):
    s, x0, of, out = _jump_run(name, dev, T, seed, monkeypatch, tail)
    p = BENCH_PARAMS[name]
    k = s.inner_sampler.kernel
    K = int(s.inner_sampler.params.n_iterations)
    assert K == p['K'] and k.step_size == pytest.approx(p['h'], rel=1e-12)
    assert bool((k.inv_mass_diag == 1).all())
    L = int(getattr(k, 'n_leapfrog_steps', 0))
    if 'L' in p:
        assert L == p['L']
    states = torch.cat([x0[None], out.samples.reshape(T * (K + 1), N, -1).cpu()])
    wl = shadow.Workload(inner_kind, opot.sum_squares, of, k.step_size, max(L, 1), n_inner=K)
    label = name + (' tail' if tail else '')
    rep = shadow.shadow(states, wl, seed)
    sm = _check(rep, label)
    st = out.statistics
    assert st.n_accepted_trajectories == rep.accepted_inner and st.n_accepted_jumps == rep.accepted_jumps
    assert st.n_attempted_trajectories == N * T * K and st.n_attempted_jumps == N * T
    if inner_kind == 'jump_mala':                                                  # langevin.py:116-120 + jump.py:212-213
        assert st.n_target_calls == 2 * N * T * K + 2 * N * T and st.n_target_gradient_calls == 2 * N * T * K
    else:                                                                          # hmc.py:122-125 + jump.py:212-213
        assert st.n_target_gradient_calls == 2 * L * N * T * K
        assert st.n_target_calls == (2 * L + 2) * N * T * K + 2 * N * T
    _acc_close(sm['acceptance_inner'], BENCH_ACC[name][0], label + ' inner')
    _acc_close(sm['acceptance_jump'], BENCH_ACC[name][1], label + ' jump')


@pytest.mark.parametrize('tail', [False, True], ids=['jump_launch', 'jump_tail'])
def test_C3_fitted_flow_shadowed_3_outer_iterations(dev, monkeypatch, tail):
    """C3 as bench.py runs it: jump_mala, U = sum x^2, d = 64, K = 100 MALA transitions on `mala_kernel` per jump, the
    bench's fitted default RealNVP; 3 outer iterations = 303 transitions shadowed, with the jump on its own flow-MH launch
    (the bench's route) and as the fused tail of the last inner launch."""
    _jump_shadow('C3', dev, 3, 3131, monkeypatch, 'jump_mala', tail)


def test_C5_fitted_flow_shadowed_4_outer_iterations(dev, monkeypatch):
    """C5 as bench.py runs it: jump_hmc, U = sum x^2, d = 256, K = 5 trajectories of L = 20 (h = 0.05) on `hmc_kernel` per
    jump, the bench's fitted default RealNVP; 4 outer iterations = 24 transitions shadowed."""
    _jump_shadow('C5', dev, 4, 5151, monkeypatch, 'jump_hmc')


# ================================================================================================ IMH (C2)
def test_C2_fitted_flow_shadowed_200_transitions(dev, monkeypatch):
    """C2 as bench.py runs it: imh, U = sum x^2, d = 64, the bench's variationally fitted default RealNVP, on
    `nfmc_imh_parallel_f32` (the sequential route is patched out); 4 bench steps = 200 transitions shadowed.  The kernel
    carries log q of the current states across transitions; the shadow recomputes it from each pre-state."""
    from nfmc_amd.samplers import imh, jump
    T_steps, seed = 4, 2222
    s, x0, of = _bench_run('C2', dev, T_steps, seed)
    T = int(s.params.n_iterations)
    assert T == T_steps * bench.CONFIGS['C2']['inner'] == 200
    calls = []
    orig = jump.launch_imh_parallel
    monkeypatch.setattr(imh, 'launch_imh_parallel', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    monkeypatch.setattr(imh, 'launch_flow_mh', lambda *a, **k: (_ for _ in ()).throw(AssertionError('sequential kernel')))
    out = s.sample(x0.to(dev), show_progress=False)
    assert calls, 'nfmc_imh_parallel_f32 did not run'
    states = torch.cat([x0[None], out.samples.reshape(T, N, -1).cpu()])
    rep = shadow.shadow(states, shadow.Workload('imh', opot.sum_squares, of), seed)
    sm = _check(rep, 'C2')
    st = out.statistics
    assert st.n_attempted_trajectories == N * T and st.n_accepted_trajectories == rep.accepted_jumps
    assert st.n_target_calls == 2 * N * T and st.n_target_gradient_calls == 0          # imh.py:236-240
    _acc_close(sm['acceptance_jump'], BENCH_ACC['C2'][1], 'C2')
