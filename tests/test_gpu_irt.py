"""GPU: item-response theory (NFMC_POT_ITEM_RESPONSE) on the fused HIP kernels against the fp64 CPU oracle, with the
target restated in fp64 (tests/irt_fp64.py).

Every problem is ItemResponseTheory.synthetic(S, Q, seed=d) (a quarter of the pairs missing); chains start at
irt_fp64.start_states(seed=d + 1): the generating state plus about one posterior standard deviation per coordinate.  The
oracle samplers evaluate the model's log densities from torch.distributions in fp64 (irt_fp64.model_u64, U up to one
constant: independent of both the kernels and the class); values are checked against IRTU64 / IRTFast64.  The mass
diagonals come from H = the median over the starts of the fp64 diagonal Hessian: MALA inv_mass_diag = sqrt(H) with step
2.0 d^(-1/3), HMC 1 / H with step 1.6 d^(-1/4), MH 0.5 / sqrt(d H).

Tolerances are the sparse-logistic-regression tests' (tests/test_gpu_sparse_logreg.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

(S, Q) reaches every default (CPL, LPC) layout choose_cfg picks: d = 3 -> (4, 1), 5 -> (4, 2), 9 -> (4, 4), 25 -> (4, 8),
51 -> (8, 8), 101 -> (8, 16), 255 -> (8, 32), 401 -> (8, 64), 1023 -> (16, 64); (5, 3) has a register quad that holds a
student, the questions and mu; (23, 1) and (1, 23) are the one-question and the one-student edge.  The responses are read
by plain global loads (no tile), so there is no tile edge to cover.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from irt_fp64 import IRTFast64, IRTU64, model_u64, prior_draws, start_states

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


class _Problem:
    """potential, fp64 restatement, fp64 oracle target, starts x0 fp32 (n, d), H (d,) fp64"""

    def __init__(self, S, Q, n, missing=0.25, edit=None):
        from nfmc_amd.potentials import ItemResponseTheory
        self.S, self.Q, self.d = S, Q, S + Q + 1
        pot, self.truth = ItemResponseTheory.synthetic(S, Q, self.d, missing=missing)
        if edit is not None:                       # a changed mask on the same responses
            pot = ItemResponseTheory(pot.responses, edit(pot.observed.clone()))
        self.pot = pot
        self.ref = IRTFast64(pot.responses, pot.observed)
        self.target = functools.partial(model_u64, R=pot.responses, observed=pot.observed)
        x0 = start_states(self.ref, self.truth, n, self.d + 1)
        self.x0 = x0.float()
        self.H = self.ref.hess_diag(x0).median(0).values

    def imd(self, kind):
        if kind in ('mala', 'ula'):
            return torch.sqrt(self.H)
        if kind in ('hmc', 'uhmc'):
            return 1 / self.H
        return 0.5 / torch.sqrt(self.d * self.H)

    def step(self, kind):
        if kind in ('mala', 'ula'):
            return 2.0 * self.d ** (-1 / 3)
        return 1.6 * self.d ** (-1 / 4) if kind in ('hmc', 'uhmc') else 0.0


@functools.lru_cache(maxsize=None)
def _problem(S, Q, n, missing=0.25):
    return _Problem(S, Q, n, missing)


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


def _sampler(kind, p, T, L=5, target=None, h=None, imd=None):
    from nfmc_amd.samplers import mcmc
    d = p.d
    target = p.pot if target is None else target
    h = p.step(kind) if h is None else h
    imd = (p.imd(kind) if imd is None else imd).float()
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        s = cls((d,), target, mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd),
                mcmc.LangevinParameters(n_iterations=T))
    elif kind == 'mh':
        s = mcmc.MH((d,), target, mcmc.MHKernel(event_size=d, inv_mass_diag=imd), mcmc.MHParameters(n_iterations=T))
    else:
        cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
        s = cls((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h, inv_mass_diag=imd),
                mcmc.HMCParameters(n_iterations=T))
    return s


def _oracle(kind, p, T, noise, L=5):
    from oracle import samplers as osamp
    okind = {'mala': 'langevin', 'ula': 'langevin', 'mh': 'mh', 'hmc': 'hmc', 'uhmc': 'hmc'}[kind]
    tr = osamp.mcmc_sample(p.x0.double(), p.target, okind, T, p.step(kind), n_leapfrog=L,
                           adjustment=kind not in ('ula', 'uhmc'), noise=noise, inv_mass_diag=p.imd(kind).float().double())
    if kind in ('mala', 'mh', 'hmc') and p.d <= 501:      # the decisions are exercised
        acc = tr.n_accepted / (p.x0.shape[0] * T)
        print('%s d=%d: oracle acceptance %.3f' % (kind, p.d, acc))
        assert acc < 0.995, (kind, p.d, acc)
    return tr


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
# (S, Q): every default layout (tests/test_host_irt.py asks the library's choose_cfg for each), then the one-question and
# the one-student edge
GRID =[(1, 1), (2, 2), (5, 3), (16, 8), (30, 20), (60, 40), (200, 54), (300, 100), (700, 322), (23, 1), (1, 23)]


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('S,Q', GRID)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, S, Q):
    from oracle import samplers as osamp
    from nfmc_amd.samplers import mcmc
    n, T = 96, 4
    p = _problem(S, Q, n)
    d = p.d
    L = 2 if d == 1023 else 5
    s = _sampler(kind, p, T, L=L)
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(d)
    tr = _oracle(kind, p, T, rec, L=L)
    s.replay = (torch.stack([v.float() for v in rec.normals]),
                torch.stack([v.float() for v in rec.uniforms]) if rec.uniforms else None)
    assert mcmc.resolve_target(p.pot, (d,), family='mcmc') is p.pot
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls                                       # every transition on the fused kernel
    what = '%s S=%d Q=%d' % (kind, S, Q)
    _compare(out.samples.reshape(T, n, d), tr, what)
    _compare_decisions(rec_k, tr, kind, p.x0, p.ref, what)


def _drop_one_student_and_one_question(mask):
    mask[4, :] = False
    mask[:, 2] = False
    return mask


@pytest.mark.parametrize('kind', ['mala', 'hmc'])
@pytest.mark.parametrize('edge', ['fully observed', 'an unobserved student and question'])
def test_mask_edges_match_oracle(dev, monkeypatch, kind, edge):
    """S = 13, Q = 7 (two alpha quads per chain at LPC = 8, the second straddling S) with every pair observed, and with
    student 4 and question 2 without a single observed answer: their coordinates feel the prior alone."""
    from oracle import samplers as osamp
    n, T = 96, 4
    p = _Problem(13, 7, n, missing=0.0) if edge == 'fully observed' else _Problem(13, 7, n, edit=_drop_one_student_and_one_question)
    assert bool(p.pot.observed.all()) == (edge == 'fully observed')
    if edge != 'fully observed':
        assert not bool(p.pot.observed[4].any()) and not bool(p.pot.observed[:, 2].any())
    s = _sampler(kind, p, T)
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(5)
    tr = _oracle(kind, p, T, rec)
    s.replay = (torch.stack([v.float() for v in rec.normals]), torch.stack([v.float() for v in rec.uniforms]))
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls
    what = '%s %s' % (kind, edge)
    _compare(out.samples.reshape(T, n, p.d), tr, what)
    _compare_decisions(rec_k, tr, kind, p.x0, p.ref, what)


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,S,Q', [('mala', 30, 20), ('ula', 5, 3), ('mh', 60, 40), ('hmc', 16, 8), ('uhmc', 2, 2)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, S, Q):
    from oracle import samplers as osamp
    n, T = 96, 4
    p = _problem(S, Q, n)
    seed = 777 + p.d
    s = _sampler(kind, p, T)
    s.seed = seed
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls
    tr = _oracle(kind, p, T, osamp.PhiloxNoise(seed, dtype=torch.float64))
    what = 'native %s S=%d Q=%d' % (kind, S, Q)
    _compare(out.samples.reshape(T, n, p.d), tr, what)
    _compare_decisions(rec_k, tr, kind, p.x0, p.ref, what)


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


# ------------------------------------------------------------------------- 3. jump_mala
@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('S,Q', [(5, 3), (16, 8), (30, 20)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, S, Q):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, T, Kin, seed = 192, 3, 4, 31337
    p = _problem(S, Q, n)
    d, h, imd = p.d, p.step('mala'), p.imd('mala').float()
    f, of = _flow_pair(d)
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), p.pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T),
                      mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd),
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls and not split                        # inner loop and jump fused
    if not fuse_tail:
        assert len(flow_mh) == T                              # each jump on the flow-MH kernel
    tr = osamp.jump_sample(p.x0.double(), p.target, of, 'langevin', T, Kin, h, inv_mass_diag=imd.double(),
                           noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < ATOL + RTOL * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > 0.95, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= max(2, int(0.03 * n * T))


# ------------------------------------------------------------------------- 4. imh on the sequential flow-MH kernel
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


@pytest.mark.parametrize('S,Q,spline', [(1, 1, False), (16, 8, False), (60, 40, False), (5, 3, True), (30, 20, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, S, Q, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 9."""
    from oracle import samplers as osamp
    n, T = 192, 5
    p = _problem(S, Q, n)
    d, seed = p.d, 4711 + p.d
    f, of = _flow_pair(d, 3 if spline else 9, spline=spline)
    out = _imh_run(monkeypatch, p.pot, d, f, p.x0, T, seed)
    tr = osamp.imh_sample(p.x0.double(), p.target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, '%s imh S=%d Q=%d' % ('c-rqnsf' if spline else 'realnvp', S, Q))


# ------------------------------------------------------------------------- 5. fused equals split
@pytest.mark.parametrize('kind,S,Q', [('mala', 30, 20), ('hmc', 5, 3), ('mh', 16, 8), ('hmc', 60, 40)])
def test_fused_equals_split(dev, monkeypatch, kind, S, Q):
    n, T = 96, 4
    p = _problem(S, Q, n)
    d = p.d
    outs, counts = [], []
    for target, fuse in ((p.pot, 'auto'), (lambda x: p.pot(x), 'never')):
        spy = _Spy(monkeypatch)
        s = _sampler(kind, p, T, target=target)
        s.seed, s.fuse = 2024, fuse
        outs.append(s.sample(p.x0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T]
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < ATOL
    assert same.float().mean() > 0.95, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 6. NeuTra gradient (VALU kernels)
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


@pytest.mark.parametrize('S,Q,nh', [(1, 1, 4), (2, 2, 8), (5, 3, 16), (16, 8, 32), (30, 20, 8), (60, 40, 16)])
def test_neutra_gradient_matches_fp64_autograd(dev, S, Q, nh):
    """U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)| and its gradient from the VALU NeuTra kernel against fp64 autograd
    through oracle/flow.py and IRTU64's loops.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    n = 96
    p = _problem(S, Q, n)
    d = p.d
    ref = IRTU64(p.pot.responses, p.pot.observed)
    f, of = _flow_pair(d, 3, n_hidden=nh)
    z = p.x0.double().requires_grad_(True)
    u_ref = osamp.neutra_adjusted_target(of, ref, (d,))(z)
    g_ref, = torch.autograd.grad(u_ref.sum(), z)
    rc, u, g = _neutra_grad(dev, f, p.pot, z.detach())
    assert rc == hip.OK
    ur = u_ref.detach()
    np.testing.assert_allclose(u.numpy(), ur.numpy(), atol=2e-4 * (1 + float(ur.abs().max())), rtol=0)
    err = (g.double() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1))
    print('S=%d Q=%d H=%d: worst relative gradient error %.2e' % (S, Q, nh, float(err.max())))
    assert float(err.max()) < 2e-4


# ------------------------------------------------------------------------- 7. NeuTra trajectories, wide conditioner
def _neutra_sampler(p, f, T, L, h):
    from nfmc_amd.samplers import mcmc, neutra
    d = p.d
    return neutra.NeuTraHMC((d,), p.pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                            mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))


@pytest.mark.parametrize('S,Q,nh', [(5, 3, 8), (30, 20, 16)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, S, Q, nh):
    from oracle import samplers as osamp
    n, T, L = 96, 3, 4
    p = _problem(S, Q, n)
    d = p.d
    h = 0.2 / math.sqrt(float(p.H.max()))
    f, of = _flow_pair(d, 9, n_hidden=nh)
    s = _neutra_sampler(p, f, T, L, h)
    assert s._closed_form() is p.pot and s._min_hidden() == 0
    split = []
    monkeypatch.setattr(s.inner_sampler, 'sample', lambda *a, **k: split.append(1))
    s.seed = 12
    out = s.sample(p.x0, show_progress=False)
    assert not split
    tr = osamp.neutra_hmc_sample(p.x0.double(), p.target, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 6


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    from nfmc_amd import hip
    from oracle import samplers as osamp
    n, T, L = 96, 3, 4
    p = _problem(30, 20, n)
    d = p.d
    h = 0.2 / math.sqrt(float(p.H.max()))
    f, of = _flow_pair(d, 9, n_hidden=64)
    rc, _u, _g = _neutra_grad(dev, f, p.pot, p.x0)
    assert rc == hip.EUNSUPPORTED
    s = _neutra_sampler(p, f, T, L, h)
    split = []
    orig = s.inner_sampler.sample
    s.inner_sampler.sample = lambda *a, **k: split.append(1) or orig(*a, **k)
    s.seed = 12
    out = s.sample(p.x0, show_progress=False)
    assert split == [1]
    tr = osamp.neutra_hmc_sample(p.x0.double(), p.target, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())


# ------------------------------------------------------------------------- 8. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,S,Q,n,W,every', [('mala', 16, 8, 140, 12, 1), ('hmc', 16, 8, 150, 16, 2),
                                                ('mala', 60, 40, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, S, Q, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds: the controller state after the device warmup against
    oracle.samplers.replay_controller over the kernel's kept states and accept counts, every warmup transition and the
    sampling run after it shadowed in fp64."""
    from test_gpu_warmup import _Record as _Accepts, _check_controller, _controller_params, _sampler as _wsampler, _shadow
    from nfmc_amd import hip
    from oracle import samplers as osamp
    p = _problem(S, Q, n)
    d = p.d
    lm = float(p.H.max())
    h0 = 0.3 * (0.5 * d ** (-1 / 4) / math.sqrt(lm) if kind == 'hmc' else 0.5 * d ** (-1 / 3) / lm)
    imd0 = torch.ones(d)
    T, L, seed = 6, 4, 4242 + d
    s = _wsampler(kind, d, p.pot, W, T, h0, L=L, every=every)
    h0 = float(s.kernel.step_size)
    s.seed = seed
    rec = _Accepts(monkeypatch, s)
    wout = s.warmup(p.x0, show_progress=False)
    what = 'irt %s d=%d n=%d every=%d' % (kind, d, n, every)
    states = wout.samples.reshape(W, n, d)
    ups, h_t, imd_t = osamp.replay_controller(states, rec.accepted(), every, _controller_params(s, h0, imd0))
    assert len(ups) == math.ceil(W / every)
    _check_controller(s, ups, what)
    _shadow(torch.cat([p.x0[None], states]), kind, p.target, h_t, imd_t, seed, hip.WARMUP_STEP0, L, what + ' warmup', 0.05)
    x1 = wout.running_samples.last_sample.cpu()
    out = s.sample(x1, show_progress=False)
    assert torch.isfinite(out.samples).all()
    _shadow(torch.cat([x1[None], out.samples.reshape(T, n, d)]), kind, p.target, s.kernel.step_size,
            s.kernel.inv_mass_diag.clone(), seed, 0, L, what + ' sampling', 0.05)


# ------------------------------------------------------------------------- 9. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc, imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    n = 256
    p = _problem(30, 20, n)
    d, pot = p.d, p.pot
    x = p.x0.to(dev)
    f, _ = _flow_pair(d)
    f.to(dev)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_ITEM_RESPONSE == 9 and pd.reserved == 30
    assert pd.a % 16 == 0 and pot.descriptor(dev).a == pd.a and pot.descriptor(dev).b == pd.b   # cached per device
    a, _keep = dlmc.step_args(f, x, 0.05, pot=pot)
    assert int(hip.lib().nfmc_dlmc_step_supported_f32(C.byref(a))) == hip.EUNSUPPORTED
    before = x.clone()
    assert int(hip.lib().nfmc_dlmc_step_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k3 = _flow_mh_probe_args(run, f, pot, logq, True)
    assert int(hip.lib().nfmc_imh_parallel_supported_f32(C.byref(pa))) == hip.EUNSUPPORTED
    work = torch.zeros(64, device=dev)                                               # refused before the work area is sized
    assert int(hip.lib().nfmc_imh_parallel_f32(C.byref(pa), hip.ptr(work), work.numel() * 4, hip.stream())) == hip.EUNSUPPORTED
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK        # the register kernels take it
    pa.rng.rounds = 7                                                               # the opt-in stream: not for kind 9
    before = run.x.clone()
    assert int(hip.lib().nfmc_flow_mh_steps_f32(C.byref(pa), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(run.x, before)
    # a wide conditioner (one-chain-per-lane / matrix-core flow-MH kernels): refused, never evaluated as a quadratic
    fw, _ = _flow_pair(d, 5, n_hidden=48)
    fw.to(dev)
    pw, _k4 = _flow_mh_probe_args(run, fw, pot, logq, True)
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pw))) == hip.EUNSUPPORTED
    # NeuTra on the matrix cores (48 units): the gradient and the trajectory entry points
    u = torch.full((n,), 123.0, device=dev)
    gr = torch.full_like(x, 123.0)
    before = x.clone()
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


def test_the_fit_step_refuses_kind_9(dev):
    """The device variational fit evaluates kinds 0 and 1 only: the sampler warmups are not offered the potential
    (fused_in('fit') is False) and nfmc_flow_variational_fit_step_f32 answers EUNSUPPORTED without touching the weights."""
    from nfmc_amd import hip
    from nfmc_amd.flow_training import DeviceFit
    from nfmc_amd.samplers.common import resolve_target
    n = 96
    p = _problem(16, 8, n)
    assert resolve_target(p.pot, (p.d,), family='fit') is None
    f, _ = _flow_pair(p.d)
    f.to(dev)
    fit = DeviceFit(f.bijection, dev, n, lr=1e-3)
    before = fit.params.clone()
    pd = p.pot.descriptor(dev)
    z = p.x0.to(dev)
    fit.opt.step = 1
    rc = int(hip.lib().nfmc_flow_variational_fit_step_f32(C.byref(fit.fit), C.byref(pd), hip.ptr(z), n, C.byref(fit.opt),
                                                            hip.stream()))
    torch.cuda.synchronize()
    assert rc == hip.EUNSUPPORTED and torch.equal(fit.params, before)


def test_philox7_and_bad_descriptors_are_refused(dev):
    """The opt-in Philox4x32-7 stream has no kind-9 kernel (and sample(..., rng_rounds=7) raises ValueError); check_irt's
    codes at the mcmc, flow-MH and NeuTra entry points alike: a NULL a or b, S = 0, S < 0 and S = d - 1 are EINVAL, a
    misaligned a is EALIGN.  Nothing is written."""
    from nfmc_amd import hip, sample
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    n = 128
    p = _problem(16, 8, n)
    d, pot = p.d, p.pot
    x = p.x0.to(dev)
    before = x.clone()
    bad = []
    for field, value, code in (('a', 0, hip.EINVAL), ('b', 0, hip.EINVAL), ('reserved', 0, hip.EINVAL),
                               ('reserved', -1, hip.EINVAL), ('reserved', d - 1, hip.EINVAL), ('reserved', d, hip.EINVAL),
                               ('a', 'misaligned', hip.EALIGN)):
        q = pot.descriptor(dev)
        setattr(q, field, q.a + 4 if value == 'misaligned' else value)
        bad.append((q, code))
    ok = pot.descriptor(dev)
    ok.reserved = d - 2                                                              # S = d - 2, Q = 1: well formed
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = hip.ptr(x), n, d, 2, 0.01, 1
    a.pot = pot.descriptor(dev)
    a.rng.seed, a.rng.rounds = 3, 7
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    a.rng.rounds = 10
    for q, code in bad:
        a.pot = q
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == code
    hm = hip.NfmcHmcArgs()
    hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = hip.ptr(x), n, d, 2, 0.01, 1, 3
    hm.rng.seed = 3
    for q, code in bad:
        hm.pot = q
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), hip.stream())) == code
    f, _ = _flow_pair(d)
    f.to(dev)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k = _flow_mh_probe_args(run, f, pot, logq, True)
    st, _k2 = f.bijection.packed(dev)
    u = torch.empty(n, device=dev)
    g = torch.empty_like(x)
    for q, code in bad:
        pa.pot = q
        assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == code
        assert int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(q), hip.ptr(x), n, hip.ptr(u), hip.ptr(g),
                                                              hip.stream())) == code
    pa.pot = ok
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    with pytest.raises(ValueError):
        sample(pot, flow=None, strategy='mala', n_iterations=2, n_chains=32, show_progress=False, seed=1,
               x0=x[:32].cpu(), rng_rounds=7)


def test_limits_are_unchanged(dev):
    """Kind 9 adds no shape limit of its own: nfmc_limits answers what it did for ABI version 4."""
    from nfmc_amd import hip
    lim = hip.NfmcLimits()
    assert int(hip.lib().nfmc_limits(C.byref(lim))) == hip.OK
    assert ((lim.abi_version, lim.max_d_sampler, lim.max_d_flow, lim.max_hidden_valu, lim.max_hidden, lim.max_steps_per_call)
            == (4, 1024, 512, 32, 128, hip.MAX_STEPS_PER_CALL))


# ------------------------------------------------------------------------- 10. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    from nfmc_amd.dist import Shard
    n, T = 300, 8
    p = _problem(13, 7, n)
    d = p.d
    runs = []
    for _ in range(2):
        s = _sampler(kind, p, T)
        s.seed = 7
        runs.append(s.sample(p.x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories
    dense = runs[0].samples.reshape(T, n, d)
    parts = []
    for r in range(2):
        sh = Shard(rank=r, world=2)
        sh.merge_statistics = lambda s_: s_
        s = _sampler(kind, p, T)
        s.seed, s.shard = 7, sh
        parts.append(s.sample(p.x0, show_progress=False).samples.reshape(T, -1, d))
    assert torch.equal(torch.cat(parts, 1), dense)


# ------------------------------------------------------------------------- 11. overflow
@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_starts_are_rejected_and_counted(dev, kind):
    """Chains at 1e30: x^2 overflows fp32, U(x) is inf, every log ratio is inf - inf or worse.  The adjusted kernels reject
    every proposal and count it as non-finite (n_nonfinite_log_ratios), as for the existing kinds; the states stay where
    they are, finite."""
    n, T = 256, 5
    p = _problem(9, 5, n)
    x0 = torch.full((n, p.d), 1e30)
    s = _sampler(kind, p, T, L=3, h=0.01, imd=torch.ones(p.d, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.equal(out.samples.reshape(T, n, p.d)[-1], x0)
    assert st.n_accepted_trajectories == 0 and st.n_nonfinite_log_ratios == n * T


# ------------------------------------------------------------------------- 12. correctness without an oracle
def test_prior_stays_stationary_under_an_all_missing_mask(dev, monkeypatch):
    """No observed pair: the posterior is the prior exactly, a product of normals.  4096 chains start at exact prior draws
    and run 50 fused MALA transitions; a kernel that leaves the target invariant keeps them there however well it mixes:
    the mean and the variance of every coordinate still match (0 or m0, sigma^2) within 5 standard errors (the variance's
    from the fourth sample moment).  The three scales differ, so a swapped precision shows."""
    from nfmc_amd.potentials import ItemResponseTheory
    S, Q, n, T = 9, 6, 4096, 50
    kw = dict(mean_ability_prior=(-1.5, 0.5), ability_scale=2.0, difficulty_scale=0.8)
    pot = ItemResponseTheory(torch.ones(S, Q), observed=torch.zeros(S, Q, dtype=torch.bool), **kw)
    d = S + Q + 1
    x0 = prior_draws(S, Q, n, 2024, **kw).float()
    from nfmc_amd.samplers import mcmc
    s = mcmc.MALA((d,), pot, mcmc.LangevinKernel(event_size=d, step_size=0.15), mcmc.LangevinParameters(n_iterations=T))
    s.params.store_samples = False
    s.seed = 31
    spy = _Spy(monkeypatch)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    print('acceptance', acc)
    assert 0.3 < acc < 1.0, acc
    x = out.running_samples.last_sample.cpu().double()
    assert x.shape == (n, d) and bool(torch.isfinite(x).all())
    assert not torch.equal(x, x0.double())
    mean_t = torch.tensor([0.0] * (S + Q) + [-1.5], dtype=torch.float64)
    var_t = torch.tensor([4.0] * S + [0.64] * Q + [0.25], dtype=torch.float64)
    m = x.mean(0)
    v = x.var(0)
    m4 = ((x - m) ** 4).mean(0)
    z_m = (m - mean_t) / torch.sqrt(v / n)
    z_v = (v - var_t) / torch.sqrt((m4 - v * v) / n)
    print('z of the means', [round(t, 2) for t in z_m.tolist()])
    print('z of the variances', [round(t, 2) for t in z_v.tolist()])
    assert bool((z_m.abs() < 5).all()), z_m.tolist()
    assert bool((z_v.abs() < 5).all()), z_v.tolist()


SCORE_B = 20   # from the fp64 oracle run: see the docstring below


def test_score_identity_at_stationarity(dev):
    """E[grad U] = 0 under the posterior.  S = 12, Q = 6, 4096 chains from start_states run strategy 'mala' with the device
    warmup and then SCORE_B transitions; on the final states the per-coordinate mean of the fp64 gradient IRTU64.grad is
    within 5 standard errors of 0.  The chains are independent, so the standard error, std / sqrt(n), is exact.

    SCORE_B: at the starts themselves the largest |z| is 152.8.  The fp64 oracle run the same way (mcmc_warmup of 40
    transitions from step 0.3 d^(-1/3) and a unit mass diagonal, which tunes the step to 0.110 at acceptance 0.63, then
    mcmc_sample; Philox seeds 99 and 7) has the largest |z| at 2.0 and 2.9 right after the warmup and under 3.5 at every
    one of the next 240 transitions, so the smallest B that passes is 1; 20 is that with a margin."""
    S, Q, n, W = 12, 6, 4096, 40
    p = _Problem(S, Q, n)
    d = p.d
    from test_gpu_warmup import _sampler as _wsampler
    s = _wsampler('mala', d, p.pot, W, SCORE_B, 0.3 * d ** (-1 / 3))
    s.params.store_samples = False
    s.seed = 99
    wout = s.warmup(p.x0, show_progress=False)
    out = s.sample(wout.running_samples.last_sample, show_progress=False)
    x = out.running_samples.last_sample.cpu().double()
    g = IRTU64(p.pot.responses, p.pot.observed).grad(x)
    z = g.mean(0) / (g.std(0) / math.sqrt(n))
    print('tuned step %.4f, z of the mean gradient' % s.kernel.step_size, [round(t, 2) for t in z.tolist()])
    assert bool((z.abs() < 5).all()), z.tolist()


# ------------------------------------------------------------------------- 14. public entry
def test_sample_jump_mala_orders_the_abilities(dev, monkeypatch):
    """End to end: sample(pot, strategy='jump_mala', flow='realnvp', n_chains=1024) runs fused and returns finite moments;
    the posterior mean abilities, unpack(out.mean), are in the order of the generating ones: rank correlation above 0.7.
    The data are synthetic(40, 60, 0): with the 20 questions of synthetic(40, 20, 0) a student has about 15 answers and the
    fp64 oracle's posterior means (200 MALA transitions at these settings) reach a rank correlation of 0.74 only; with 60
    questions the oracle gives 0.87."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import ItemResponseTheory
    from nfmc_amd.samplers import jump
    pot, truth = ItemResponseTheory.synthetic(40, 60, 0)
    ref = IRTFast64(pot.responses, pot.observed)
    d, n = 101, 1024
    x0 = start_states(ref, truth * 0, n, 1).float()          # around the origin: no knowledge of the truth
    H0 = ref.hess_diag(torch.zeros(1, d, dtype=torch.float64))[0]
    split = []
    orig = jump.split_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    spy = _Spy(monkeypatch)
    out = sample(pot, flow='realnvp', strategy='jump_mala', n_iterations=20, n_chains=n, x0=x0, show_progress=False,
                 seed=3, inner_kernel_kwargs={'step_size': 0.3, 'inv_mass_diag': torch.sqrt(H0).float()},
                 inner_param_kwargs={'n_iterations': 10})
    assert not spy.calls and not split
    assert torch.isfinite(out.mean).all() and torch.isfinite(out.variance).all()
    _mu, ability, _b = pot.unpack(out.mean.cpu().double().reshape(-1))
    rank = lambda v: torch.argsort(torch.argsort(v)).double()   # noqa: E731
    a, b = rank(ability), rank(pot.unpack(truth)[1])
    rho = float(torch.corrcoef(torch.stack([a, b]))[0, 1])
    print('rank correlation of the mean abilities with the truth: %.3f' % rho)
    assert rho > 0.7, rho
