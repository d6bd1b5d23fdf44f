"""GPU: sparse logistic regression (NFMC_POT_SPARSE_LOGISTIC_REGRESSION) on the fused HIP kernels against the fp64 CPU
oracle, with the target restated in fp64 (tests/sparse_logreg_fp64.py).

Every problem is a synthetic data set drawn from the model (standardised X, three nonzero coefficients), X scaled by
2 / sqrt(N) so that the data curvature stays O(1) at every N; chains start at sparse_logreg_fp64.start_states.  The oracle
samplers evaluate the model's log densities from torch.distributions in fp64 (sparse_logreg_fp64.model_u64, U up to one
constant: independent of both the kernels and the class); values are checked against the loops of SLRU64.  Step sizes
scale with the largest diagonal Hessian entry at the start (90th percentile over the chains).

Tolerances are the logistic-regression tests' (tests/test_gpu_logreg.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

d = 2 D + 1 reaches every default (CPL, LPC) layout choose_cfg picks: d = 3 -> (4, 1), 5 -> (4, 2), 9 -> (4, 4), 25 ->
(4, 8), 51 -> (8, 8), 101 -> (8, 16), 255 -> (8, 32), 401 -> (8, 64), 1023 -> (16, 64), capacities 4 to 1024.  The compact
LDS tile holds 8192 / capacity rows (2048 at d = 3, 8 at d = 1023); N covers 1, 63, 64, 65, 1000 and N past one tile.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from sparse_logreg_fp64 import SLRU64, log_gamma_moments, model_u64, prior_draws, start_states, synthetic

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _problem(d, N, n, seed, spread=1.0):
    """(potential, fp64 loop, fp64 oracle target, x0 fp32 (n, d))"""
    from nfmc_amd.potentials import SparseLogisticRegression
    D = (d - 1) // 2
    X, y, _ = synthetic(N, D, seed, scale=2.0 / math.sqrt(N))
    x0 = start_states(D, n, seed + 1, spread)
    return SparseLogisticRegression(X, y), SLRU64(X, y), functools.partial(model_u64, X=X, y=y), x0.float()


def _lmax(ref, x0):
    return float(torch.quantile(ref.hess_diag(x0.double()).abs().amax(dim=1), 0.9))


def _compare(got, tr, what):
    want = tr.stacked().float()
    n = want.shape[1]
    keep = torch.ones(n, dtype=torch.bool)
    if tr.log_ratios:
        lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
        lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
        keep = ((lu - lr).abs() >= MARGIN).all(0)
    excluded = 1.0 - float(keep.float().mean())
    print('%s: %.1f %% of the chains excluded as near-ties' % (what, 100 * excluded))
    assert excluded < 0.10, (what, excluded)
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got[:, keep].numpy(), want[:, keep].numpy(), atol=ATOL, rtol=RTOL, err_msg=what)


def _sampler(kind, d, pot, T, h, L=5, imd=None):
    from nfmc_amd.samplers import mcmc
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        s = cls((d,), pot, mcmc.LangevinKernel(event_size=d, step_size=h), mcmc.LangevinParameters(n_iterations=T))
    elif kind == 'mh':
        s = mcmc.MH((d,), pot, None, mcmc.MHParameters(n_iterations=T))
        s.kernel.inv_mass_diag = imd.float()
    else:
        cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
        s = cls((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                mcmc.HMCParameters(n_iterations=T))
    return s


def _mh_scale(d, lm):
    return torch.full((d,), 0.5 / math.sqrt(d * lm), dtype=torch.float64)


def _oracle(kind, x0, target, T, h, noise, L=5, imd=None):
    from oracle import samplers as osamp
    okind = {'mala': 'langevin', 'ula': 'langevin', 'mh': 'mh', 'hmc': 'hmc', 'uhmc': 'hmc'}[kind]
    return osamp.mcmc_sample(x0.double(), target, okind, T, h, n_leapfrog=L, adjustment=kind not in ('ula', 'uhmc'),
                             noise=noise, inv_mass_diag=imd if kind == 'mh' else None)


def _step(kind, d, lm):
    """MALA h ~ d^(-1/3) / lambda_max; HMC h ~ d^(-1/4) / sqrt(lambda_max)"""
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * d ** (-1 / 4) / math.sqrt(lm)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * d ** (-1 / 3) / lm


class _Record:
    """Hands every fused mcmc launch of `sampler` mask and log-ratio buffers and keeps them (T, n)."""

    def __init__(self, monkeypatch, sampler):
        self.masks, self.log_ratios = [], []
        cls = type(sampler)
        orig = cls._launch

        def launch(s, run, pot, k, step0, samples, masks_out=None, log_ratio_out=None, **kw):
            if masks_out is None:
                masks_out = torch.zeros(k, run.n, dtype=torch.uint8, device=run.dev)
            if log_ratio_out is None:
                log_ratio_out = torch.zeros(k, run.n, dtype=torch.float32, device=run.dev)
            self.masks.append(masks_out)
            self.log_ratios.append(log_ratio_out)
            return orig(s, run, pot, k, step0, samples, masks_out=masks_out, log_ratio_out=log_ratio_out, **kw)
        monkeypatch.setattr(cls, '_launch', launch)

    def stacked(self):
        return torch.cat(self.masks).cpu().bool(), torch.cat(self.log_ratios).cpu()


def _compare_decisions(rec, tr, kind, x0, ref, what):
    """Accept masks and log ratios against the oracle's on the rows before a chain's first disagreeing decision.  Log
    ratios to 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) |U(x)|: the kernel's U(x) and U(x') are fp32 numbers of
    that magnitude."""
    got_m, got_lr = rec.stacked()
    if kind in ('ula', 'uhmc'):
        assert bool(got_m.all()), what
        return
    want_m = torch.stack([m.reshape(-1).bool() for m in tr.masks])
    want_lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    assert got_m.shape == want_m.shape, (got_m.shape, want_m.shape)
    same = got_m == want_m
    agree = torch.cumprod(torch.cat([torch.ones(1, same.shape[1], dtype=torch.bool), same[:-1]]).int(), 0).bool()
    assert float(agree.float().mean()) > 0.9, what
    assert float(same[agree].float().mean()) > 0.97, what
    d = x0.shape[1]
    states = tr.stacked()
    prev = torch.cat([x0.double()[None], states[:-1].double()]).reshape(-1, d)
    mag = ref(prev).abs().reshape(states.shape[:2])
    agree = agree & torch.isfinite(want_lr) & (want_lr > -50)
    err = (got_lr.double() - want_lr).abs()
    tol = 2e-4 * max(1.0, d / 64) + 1e-4 * want_lr.abs() + 8 * 2.0 ** -24 * mag
    print('%s: worst log-ratio error %.2e' % (what, float(err[agree].max())))
    assert bool((err[agree] <= tol[agree]).all()), (what, float(err[agree].max()))


class _Spy:
    """Counts the split-path transitions of the mcmc samplers (none on the fused route)."""

    def __init__(self, monkeypatch):
        from nfmc_amd.samplers import mcmc
        self.calls = []
        for cls in (mcmc.MCMCSampler, mcmc.MALA, mcmc.ULA, mcmc.MH, mcmc.HMC, mcmc.UHMC):
            if cls is mcmc.MCMCSampler or '_split_step' in vars(cls):
                orig = vars(cls)['_split_step']
                monkeypatch.setattr(cls, '_split_step', self._wrap(orig))

    def _wrap(self, orig):
        return lambda s, *a, **k: self.calls.append(1) or orig(s, *a, **k)


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
# (d, N): every default layout; N = 1, 63, 64, 65, 1000, and N past one tile (2048 rows at d = 3, 16 at d = 401,
# 8 at d = 1023)
GRID = [(3, 1), (3, 2100), (5, 63), (9, 64), (25, 65), (51, 1000), (101, 65), (255, 63), (401, 40), (1023, 1),
        (1023, 64)]


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d,N', GRID)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d, N):
    from oracle import samplers as osamp
    from nfmc_amd.samplers import mcmc
    n, T = 96, 4
    pot, ref, target, x0 = _problem(d, N, n, d + N)
    lm = _lmax(ref, x0)
    h = _step(kind, d, lm)
    imd = _mh_scale(d, lm)
    s = _sampler(kind, d, pot, T, h, imd=imd)
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(d + N)
    tr = _oracle(kind, x0, target, T, h, rec, imd=imd)
    s.replay = (torch.stack([v.float() for v in rec.normals]),
                torch.stack([v.float() for v in rec.uniforms]) if rec.uniforms else None)
    assert mcmc.resolve_target(pot, (d,), family='mcmc') is pot
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls                                       # every transition on the fused kernel
    what = '%s d=%d N=%d' % (kind, d, N)
    _compare(out.samples.reshape(T, n, d), tr, what)
    _compare_decisions(rec_k, tr, kind, x0, ref, what)


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d,N', [('mala', 51, 1000), ('ula', 9, 65), ('mh', 101, 300), ('hmc', 25, 129),
                                      ('uhmc', 5, 1100), ('hmc', 1023, 20), ('mala', 401, 63), ('hmc', 3, 2100)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, N):
    from oracle import samplers as osamp
    n, T, seed = 160, 5, 777 + d
    pot, ref, target, x0 = _problem(d, N, n, d + 1)
    lm = _lmax(ref, x0)
    h = _step(kind, d, lm)
    imd = _mh_scale(d, lm)
    s = _sampler(kind, d, pot, T, h, imd=imd)
    s.seed = seed
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    tr = _oracle(kind, x0, target, T, h, osamp.PhiloxNoise(seed, dtype=torch.float64), imd=imd)
    what = 'native %s d=%d N=%d' % (kind, d, N)
    _compare(out.samples.reshape(T, n, d), tr, what)
    _compare_decisions(rec_k, tr, kind, x0, ref, what)


def _flow_pair(d, seed=5, n_hidden=None, spline=False):
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.util import create_flow_object
    from oracle import flow as oflow
    ck = {} if n_hidden is None else {'conditioner_kwargs': {'n_hidden': n_hidden}}
    if spline:
        of = oflow.perturb_(oflow.Flow(oflow.CRQNSF((d,))), seed, 0.3, 0.75)
        f = create_flow_object('c-rqnsf', (d,))
    else:
        of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,), **ck)), seed, 0.2, 0.7071)
        f = Flow(RealNVP((d,), **ck))
    f.load_state_dict(of.state_dict())
    return f, of.double()


# ------------------------------------------------------------------------- 3. jump_mala and imh
@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d,N', [(5, 300), (25, 1000), (51, 64)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d, N):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, T, Kin, seed = 192, 3, 4, 31337
    pot, ref, target, x0 = _problem(d, N, n, 3 + d)
    f, of = _flow_pair(d)
    h = 0.3 * d ** (-1 / 3) / _lmax(ref, x0)
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), None,
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.inner_sampler.kernel.step_size = h
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    out = s.sample(x0, show_progress=False)
    assert not spy.calls and not split                        # inner loop and jump fused
    if not fuse_tail:
        assert len(flow_mh) == T                              # each jump on the flow-MH kernel
    tr = osamp.jump_sample(x0.double(), target, of, 'langevin', T, Kin, h,
                           noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < ATOL + RTOL * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > 0.95, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= max(2, int(0.03 * n * T))


def _imh_run(monkeypatch, pot, d, f, x0, T, seed):
    from nfmc_amd.samplers import imh
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=T))
    s.seed = seed
    calls = {'launch_imh_parallel': 0, 'launch_flow_mh': 0, 'split_flow_mh': 0}

    def spy(name):
        fn = getattr(imh, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        monkeypatch.setattr(imh, name, wrapped)
    for name in list(calls):
        spy(name)
    out = s.sample(x0, show_progress=False)
    assert calls['launch_flow_mh'] >= 1 and calls['launch_imh_parallel'] == 0 and calls['split_flow_mh'] == 0, calls
    assert out.statistics.n_attempted_trajectories == x0.shape[0] * T
    return out


@pytest.mark.parametrize('d,N,spline', [(3, 64, False), (25, 1000, False), (101, 65, False), (255, 40, False),
                                        (9, 300, True), (51, 63, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, N, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 7.  The flows are near the
    identity, so starts with a narrow spread give a useful share of accepted proposals."""
    from oracle import samplers as osamp
    n, T, seed = 256, 6, 4711 + d
    pot, ref, target, x0 = _problem(d, N, n, 9 + d, spread=0.5)
    f, of = _flow_pair(d, 3 if spline else 9, spline=spline)
    out = _imh_run(monkeypatch, pot, d, f, x0, T, seed)
    tr = osamp.imh_sample(x0.double(), target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, '%s imh d=%d N=%d' % ('c-rqnsf' if spline else 'realnvp', d, N))


# ------------------------------------------------------------------------- 4. fused equals split
@pytest.mark.parametrize('kind,d,N', [('mala', 51, 1000), ('hmc', 9, 200), ('mh', 25, 63), ('hmc', 101, 65)])
def test_fused_equals_split(dev, monkeypatch, kind, d, N):
    n, T = 200, 6
    pot, ref, _t, x0 = _problem(d, N, n, 17 + d)
    lm = _lmax(ref, x0)
    outs, counts = [], []
    for target, fuse in ((pot, 'auto'), (lambda x: pot(x), 'never')):
        spy = _Spy(monkeypatch)
        s = _sampler(kind, d, target, T, _step(kind, d, lm), imd=_mh_scale(d, lm))
        s.seed, s.fuse = 2024, fuse
        outs.append(s.sample(x0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T]
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < ATOL
    assert same.float().mean() > 0.95, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 5. NeuTra (VALU kernels)
def _neutra_grad(dev, f, pot, z):
    from nfmc_amd import hip
    n, d = z.shape
    st, _keep = f.bijection.packed(dev, 0)          # the flow's own width, as NeuTra presents it for this target
    pd = pot.descriptor(dev)
    zd = z.to(dev, torch.float32).contiguous()
    u = torch.empty(n, device=dev)
    g = torch.empty(n, d, device=dev)
    rc = int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(pd), hip.ptr(zd), n, hip.ptr(u), hip.ptr(g),
                                                        hip.stream()))
    torch.cuda.synchronize()
    return rc, u.cpu(), g.cpu()


@pytest.mark.parametrize('d,nh,N', [(3, 4, 1), (5, 8, 63), (9, 16, 64), (25, 32, 65), (51, 8, 1000), (129, 16, 100),
                                    (255, 4, 40), (511, 8, 30)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh, N):
    """U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)| and its gradient from the VALU NeuTra kernel against fp64 autograd
    through oracle/flow.py and the loops of SLRU64.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    n = 130
    pot, ref, _t, z = _problem(d, N, n, 5 + d)
    f, of = _flow_pair(d, 3, n_hidden=nh)
    z = z.double().requires_grad_(True)
    u_ref = osamp.neutra_adjusted_target(of, ref, (d,))(z)
    g_ref, = torch.autograd.grad(u_ref.sum(), z)
    rc, u, g = _neutra_grad(dev, f, pot, z.detach())
    assert rc == hip.OK
    ur = u_ref.detach()
    np.testing.assert_allclose(u.numpy(), ur.numpy(), atol=2e-4 * (1 + float(ur.abs().max())), rtol=0)
    err = (g.double() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1))
    print('d=%d H=%d N=%d: worst relative gradient error %.2e' % (d, nh, N, float(err.max())))
    assert float(err.max()) < 2e-4


@pytest.mark.parametrize('d,nh,N', [(9, 8, 200), (51, 16, 300)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh, N):
    from nfmc_amd.samplers import mcmc, neutra
    from oracle import samplers as osamp
    n, T, L = 96, 3, 4
    pot, ref, target, z0 = _problem(d, N, n, 61 + d)
    h = 0.2 / math.sqrt(_lmax(ref, z0))
    f, of = _flow_pair(d, 9, n_hidden=nh)
    s = neutra.NeuTraHMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                         mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))
    assert s._closed_form() is pot and s._min_hidden() == 0
    split = []
    monkeypatch.setattr(s.inner_sampler, 'sample', lambda *a, **k: split.append(1))
    s.seed = 12
    out = s.sample(z0, show_progress=False)
    assert not split
    tr = osamp.neutra_hmc_sample(z0.double(), target, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 6


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc, neutra
    from oracle import samplers as osamp
    d, N, n, T, L = 51, 200, 96, 3, 4
    pot, ref, target, z0 = _problem(d, N, n, 62)
    h = 0.2 / math.sqrt(_lmax(ref, z0))
    f, of = _flow_pair(d, 9, n_hidden=64)
    rc, _u, _g = _neutra_grad(dev, f, pot, z0)
    assert rc == hip.EUNSUPPORTED
    s = neutra.NeuTraHMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                         mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))
    split = []
    orig = s.inner_sampler.sample
    s.inner_sampler.sample = lambda *a, **k: split.append(1) or orig(*a, **k)
    s.seed = 12
    out = s.sample(z0, show_progress=False)
    assert split == [1]
    tr = osamp.neutra_hmc_sample(z0.double(), target, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())


def test_dlmc_borrows_the_gradient_step_and_matches_the_oracle(dev, monkeypatch):
    from nfmc_amd.samplers import dlmc as mod
    from oracle import samplers as osamp
    d, N, n, T, seed = 9, 500, 128, 3, 4242
    pot, ref, target, x0 = _problem(d, N, n, 71)
    f, of = _flow_pair(d, 3)
    f.fit = lambda *a, **k: None
    nll = lambda x: 0.125 * torch.sum(x ** 2, dim=-1)   # noqa: E731
    calls = {'launch_flow_mh': 0, 'split_flow_mh': 0}

    def spy(name):
        fn = getattr(mod, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        monkeypatch.setattr(mod, name, wrapped)
    for name in list(calls):
        spy(name)
    s = mod.DLMC((d,), pot, nll, mod.DLMCKernel((d,), flow=f, step_size=0.05), mod.DLMCParameters(n_iterations=T))
    s.seed = seed
    out = s.sample(x0, show_progress=False)
    assert s.last_route == 'borrowed'                        # grad U by autograd, not nfmc_dlmc_step_f32
    assert calls == {'launch_flow_mh': T, 'split_flow_mh': 0}   # the MH step on the flow-MH kernel
    tr = osamp.dlmc_sample(x0, target, nll, of, T, 0.05, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got = out.samples.cpu().double().reshape(T, n, d)
    same = (got - tr.stacked()).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() >= 0.95, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 0.03 * n * T


# ------------------------------------------------------------------------- 6. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,d,N,n,W,every', [('mala', 25, 300, 140, 12, 1), ('hmc', 25, 65, 150, 16, 2),
                                                ('mala', 101, 64, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, d, N, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds: the controller state after the device warmup against
    oracle.samplers.replay_controller over the kernel's kept states and accept counts, every warmup transition and the
    sampling run after it shadowed in fp64."""
    from test_gpu_warmup import _Record as _Accepts, _check_controller, _controller_params, _sampler as _wsampler, _shadow
    from nfmc_amd import hip
    from oracle import samplers as osamp
    pot, ref, target, x0 = _problem(d, N, n, 7 + d)
    h0 = 0.3 * _step(kind, d, _lmax(ref, x0))
    imd0 = torch.ones(d)
    T, L, seed = 6, 4, 4242 + d
    s = _wsampler(kind, d, pot, W, T, h0, L=L, every=every)
    h0 = float(s.kernel.step_size)
    s.seed = seed
    rec = _Accepts(monkeypatch, s)
    wout = s.warmup(x0, show_progress=False)
    what = 'slr %s d=%d n=%d every=%d' % (kind, d, n, every)
    states = wout.samples.reshape(W, n, d)
    ups, h_t, imd_t = osamp.replay_controller(states, rec.accepted(), every, _controller_params(s, h0, imd0))
    assert len(ups) == math.ceil(W / every)
    _check_controller(s, ups, what)
    _shadow(torch.cat([x0[None], states]), kind, target, h_t, imd_t, seed, hip.WARMUP_STEP0, L, what + ' warmup', 0.05)
    x1 = wout.running_samples.last_sample.cpu()
    out = s.sample(x1, show_progress=False)
    assert torch.isfinite(out.samples).all()
    _shadow(torch.cat([x1[None], out.samples.reshape(T, n, d)]), kind, target, s.kernel.step_size,
            s.kernel.inv_mass_diag.clone(), seed, 0, L, what + ' sampling', 0.05)


# ------------------------------------------------------------------------- 7. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc, imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    d, N, n = 51, 300, 256
    pot, ref, _t, x = _problem(d, N, n, 4)
    x = x.to(dev)
    f, _ = _flow_pair(d)
    f.to(dev)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_SPARSE_LOGISTIC_REGRESSION and pd.reserved == N
    a, _keep = dlmc.step_args(f, x, 0.05, pot=pot)
    assert int(hip.lib().nfmc_dlmc_step_supported_f32(C.byref(a))) == hip.EUNSUPPORTED
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k3 = _flow_mh_probe_args(run, f, pot, logq, True)
    assert int(hip.lib().nfmc_imh_parallel_supported_f32(C.byref(pa))) == hip.EUNSUPPORTED
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK        # the register kernels take it
    pa.rng.rounds = 7                                                               # the opt-in stream: not for kind 7
    before = run.x.clone()
    assert int(hip.lib().nfmc_flow_mh_steps_f32(C.byref(pa), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(run.x, before)
    # a wide conditioner (one-chain-per-lane / matrix-core flow-MH kernels): refused, never evaluated as a quadratic
    fw, _ = _flow_pair(d, 5, n_hidden=48)
    fw.to(dev)
    pw, _k4 = _flow_mh_probe_args(run, fw, pot, logq, True)
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pw))) == hip.EUNSUPPORTED
    pw.x, pw.logq, pw.n_steps = hip.ptr(x), hip.ptr(logq), 1
    before = x.clone()
    assert int(hip.lib().nfmc_flow_mh_steps_f32(C.byref(pw), hip.stream())) == hip.EUNSUPPORTED
    # NeuTra on the matrix cores (48 units): the gradient and the trajectory entry points
    u = torch.full((n,), 123.0, device=dev)
    gr = torch.full_like(x, 123.0)
    stw, _k5 = fw.bijection.packed(dev)
    rc = int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(stw), C.byref(pd), hip.ptr(x), n, hip.ptr(u), hip.ptr(gr),
                                                        hip.stream()))
    assert rc == hip.EUNSUPPORTED
    na = hip.NfmcNeutraHmcArgs()
    na.z, na.n, na.n_steps, na.n_leapfrog, na.step_size, na.adjust = hip.ptr(x), n, 1, 2, 0.01, 1
    na.flow, na.pot = stw, pd
    na.rng.seed = 3
    assert int(hip.lib().nfmc_neutra_hmc_steps_f32(C.byref(na), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((u == 123.0).all()) and bool((gr == 123.0).all())
    assert not pot.fused_in('fit') and not pot.fused_in('imh_parallel') and not pot.fused_in('dlmc_step')


def test_philox7_and_bad_descriptors_are_refused(dev):
    """The opt-in Philox4x32-7 stream has no kind-7 kernel (and sample(..., rng_rounds=7) raises ValueError); a NULL X or
    y, N < 1, a misaligned X, an even d, and a or b not positive and finite are argument errors, at the mcmc, flow-MH and
    NeuTra entry points alike.  Nothing is written."""
    from nfmc_amd import hip, sample
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    d, N, n = 25, 100, 128
    pot, ref, _t, x = _problem(d, N, n, 8)
    x = x.to(dev)
    before = x.clone()
    bad = []
    for field, value in (('a', 0), ('b', 0), ('reserved', 0), ('reserved', -1), ('a', 'misaligned'),
                         ('a_scalar', 0.0), ('a_scalar', -1.0), ('a_scalar', float('inf')), ('b_scalar', 0.0),
                         ('b_scalar', float('nan'))):
        p = pot.descriptor(dev)
        setattr(p, field, p.a + 4 if value == 'misaligned' else value)
        bad.append(p)
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = hip.ptr(x), n, d, 2, 0.01, 1
    a.pot = pot.descriptor(dev)
    a.rng.seed, a.rng.rounds = 3, 7
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    a.rng.rounds = 10
    for p in bad:
        a.pot = p
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EINVAL
    a.pot, a.d = pot.descriptor(dev), d - 1                                         # an even d
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EINVAL
    hm = hip.NfmcHmcArgs()
    hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = hip.ptr(x), n, d, 2, 0.01, 1, 3
    hm.rng.seed = 3
    for p in bad:
        hm.pot = p
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), hip.stream())) == hip.EINVAL
    f, _ = _flow_pair(d)
    f.to(dev)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k = _flow_mh_probe_args(run, f, pot, logq, True)
    st, _k2 = f.bijection.packed(dev)
    u = torch.empty(n, device=dev)
    g = torch.empty_like(x)
    for p in bad:
        pa.pot = p
        assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.EINVAL
        assert int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(p), hip.ptr(x), n, hip.ptr(u), hip.ptr(g),
                                                              hip.stream())) == hip.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    with pytest.raises(ValueError):
        sample(pot, flow=None, strategy='mala', n_iterations=2, n_chains=32, show_progress=False, seed=1,
               x0=x[:32].cpu(), rng_rounds=7)


# ------------------------------------------------------------------------- 8. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    from nfmc_amd.dist import Shard
    d, N, n, T = 21, 700, 300, 8
    pot, ref, _t, x0 = _problem(d, N, n, 44)
    h = _step(kind, d, _lmax(ref, x0))
    runs = []
    for _ in range(2):
        s = _sampler(kind, d, pot, T, h)
        s.seed = 7
        runs.append(s.sample(x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories
    dense = runs[0].samples.reshape(T, n, d)
    parts = []
    for r in range(2):
        sh = Shard(rank=r, world=2)
        sh.merge_statistics = lambda s_: s_
        s = _sampler(kind, d, pot, T, h)
        s.seed, s.shard = 7, sh
        parts.append(s.sample(x0, show_progress=False).samples.reshape(T, -1, d))
    assert torch.equal(torch.cat(parts, 1), dense)


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_proposals_are_rejected_and_counted(dev, kind):
    """Steps far past stability: proposals reach scales whose exponentials (e^{s + l_j}, e^{l_j}, e^s) or logits z
    overflow fp32, so U of the proposal is inf or NaN and the log ratio is not finite.  The adjusted kernels reject every
    such proposal and count it as non-finite (n_nonfinite_log_ratios), as for the existing kinds; the kept states stay
    finite."""
    d, N, n, T = 15, 100, 512, 10
    pot, ref, _t, x0 = _problem(d, N, n, 3)
    h = {'mala': 1e4, 'mh': 0.0, 'hmc': 50.0}[kind]
    s = _sampler(kind, d, pot, T, h, L=3, imd=torch.full((d,), 1e6, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.isfinite(out.mean).all()
    print(kind, 'non-finite', st.n_nonfinite_log_ratios, 'accepted', st.n_accepted_trajectories)
    assert st.n_nonfinite_log_ratios > n * T // 2
    assert st.n_accepted_trajectories + st.n_nonfinite_log_ratios <= n * T


# ------------------------------------------------------------------------- 9. correctness without an oracle
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_prior_stays_stationary(dev, monkeypatch, kind):
    """X = 0: the data term is the constant N log 2, so the posterior is the prior.  65536 chains start at exact prior
    draws (a = b = 2, light tails) and run a few hundred fused transitions.  A kernel that leaves the target invariant
    keeps them there however well it mixes: the mean and the variance of every w_j, l_j and s still match (0, 1) for w_j
    and (digamma(a) - log b, trigamma(a)) for l_j and s, within 5 standard errors (the variance's from the fourth sample
    moment)."""
    from nfmc_amd.potentials import SparseLogisticRegression
    D, N, n, a, b = 12, 7, 65536, 2.0, 2.0
    d = 2 * D + 1
    pot = SparseLogisticRegression(torch.zeros(N, D), torch.arange(N) % 2, scale_shape=a, scale_rate=b)
    x0 = prior_draws(D, n, a, b, 2024).float()
    T = 300
    h = 0.15 if kind == 'mala' else 0.12
    s = _sampler(kind, d, pot, T, h, L=8)
    s.params.store_samples = False
    s.seed = 31
    spy = _Spy(monkeypatch)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    print(kind, 'acceptance', acc)
    assert 0.5 < acc < 1.0, acc
    x = out.running_samples.last_sample.cpu().double()
    assert x.shape == (n, d) and bool(torch.isfinite(x).all())
    assert not torch.equal(x, x0.double())
    lm, lv = log_gamma_moments(a, b)
    mean_t = torch.tensor([0.0 if c % 2 == 0 and c < 2 * D else lm for c in range(d)], dtype=torch.float64)
    var_t = torch.tensor([1.0 if c % 2 == 0 and c < 2 * D else lv for c in range(d)], dtype=torch.float64)
    m = x.mean(0)
    v = x.var(0)
    m4 = ((x - m) ** 4).mean(0)
    z_m = (m - mean_t) / torch.sqrt(v / n)
    z_v = (v - var_t) / torch.sqrt((m4 - v * v) / n)
    print(kind, 'z of the means', [round(t, 2) for t in z_m.tolist()])
    print(kind, 'z of the variances', [round(t, 2) for t in z_v.tolist()])
    assert bool((z_m.abs() < 5).all()), z_m.tolist()
    assert bool((z_v.abs() < 5).all()), z_v.tolist()


def test_sample_jump_mala_recovers_the_sparse_signal(dev):
    """End to end: sample(..., strategy='jump_mala') on N = 1000 simulated rows, D = 25 standardised features, three
    nonzero coefficients.  Posterior means of beta (over chains and the second half of the kept states): every nonzero
    coefficient keeps its sign and lies more than 3 posterior standard deviations from 0; every null one lies within 4
    posterior standard deviations of 0, and closer to 0 than the smallest nonzero one."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import SparseLogisticRegression
    N, D, n = 1000, 25, 4096
    d = 2 * D + 1
    X, y, beta_true = synthetic(N, D, 2025)
    pot, ref = SparseLogisticRegression(X, y), SLRU64(X, y)
    x0 = start_states(D, n, 2026, spread=0.5).float()
    h = 0.3 * d ** (-1 / 3) / _lmax(ref, x0[:256])
    out = sample(pot, flow='realnvp', strategy='jump_mala', n_iterations=40, n_chains=n, x0=x0, show_progress=False,
                 seed=3, inner_kernel_kwargs={'step_size': h}, inner_param_kwargs={'n_iterations': 10})
    kept = out.samples.reshape(-1, n, d)
    assert torch.isfinite(kept).all()
    kept = kept[kept.shape[0] // 2:].reshape(-1, d).double()
    beta = pot.constrain(kept)[3]
    mean, sd = beta.mean(0), beta.std(0)
    nz = beta_true != 0
    print('true', beta_true[nz].tolist(), 'mean', mean[nz].tolist(), 'sd', sd[nz].tolist())
    print('null |mean| / sd max', float((mean[~nz].abs() / sd[~nz]).max()))
    assert bool((torch.sign(mean[nz]) == torch.sign(beta_true[nz])).all())
    assert bool((mean[nz].abs() > 3 * sd[nz]).all())
    assert bool((mean[~nz].abs() < 4 * sd[~nz]).all())
    assert float(mean[~nz].abs().max()) < float(mean[nz].abs().min())
