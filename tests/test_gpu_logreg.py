"""GPU: BayesianLogisticRegression (NFMC_POT_LOGISTIC_REGRESSION) on the fused HIP kernels against the fp64 CPU oracle,
with the target restated in fp64 (tests/logreg_fp64.py).

Tolerances are the mixture tests' (tests/test_gpu_mixture.py):
  states        atol 1e-3 + rtol 1e-4.  U is a sum of N terms and the gradient a sum of N rows; the data are scaled so
                that the posterior curvature is O(1) at every N, and the fp32 sums move a transition by ~1e-5.
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

The (d, N) grid covers every (CPL, LPC) layout the sampler kernels pick (d = 1 ... 700: LPC 1 ... 64, CPL 4 / 8 / 16),
N = 1, 63, 64, 65 and 1000, and N past the LDS tile of its layout (4096 / (CPL LPC) rows: 1024 at d <= 4, 8 at d = 512).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from logreg_fp64 import LogRegU64, synthetic

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _problem(N, d, seed, sigma=1.5):
    """The class and its fp64 restatement on synthetic data scaled to an O(1) posterior curvature, and a start."""
    from nfmc_amd.potentials import BayesianLogisticRegression
    X, y, w = synthetic(N, d, seed, scale=2.0 / math.sqrt(N))
    return BayesianLogisticRegression(X, y, sigma), LogRegU64(X, y, sigma)


def _x0(n, d, seed):
    return 0.7 * torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


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


def _sampler(kind, d, pot, T, h, L=5):
    from nfmc_amd.samplers import mcmc
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        s = cls((d,), pot, mcmc.LangevinKernel(event_size=d, step_size=h), mcmc.LangevinParameters(n_iterations=T))
    elif kind == 'mh':
        s = mcmc.MH((d,), pot, None, mcmc.MHParameters(n_iterations=T))
        s.kernel.inv_mass_diag = torch.full((d,), 0.3 / math.sqrt(d))
    else:
        cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
        s = cls((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                mcmc.HMCParameters(n_iterations=T))
    return s


def _oracle(kind, x0, target, T, h, noise, L=5):
    from oracle import samplers as osamp
    okind = {'mala': 'langevin', 'ula': 'langevin', 'mh': 'mh', 'hmc': 'hmc', 'uhmc': 'hmc'}[kind]
    imd = torch.full((x0.shape[1],), 0.3 / math.sqrt(x0.shape[1]), dtype=torch.float64) if kind == 'mh' else None
    return osamp.mcmc_sample(x0.double(), target, okind, T, h, n_leapfrog=L, adjustment=kind not in ('ula', 'uhmc'),
                             noise=noise, inv_mass_diag=imd)


def _step(kind, d):
    return {'mala': 0.3, 'ula': 0.05, 'mh': 0.0, 'hmc': 0.1, 'uhmc': 0.05}[kind] * d ** (-1 / 3)


class _Record:
    """Hands every fused mcmc launch of `sampler` mask and log-ratio buffers and keeps them: the kernel's accept
    decisions and log ratios, stacked over the launches as (T, n)."""

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
    """The kernel's accept masks and log ratios against the oracle's, transition by transition, on the rows before a
    chain's first disagreeing decision (a near-tie flips it; the states test bounds how many).  Log ratios to
    2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) |U(x)|: the kernel's U(x) and U(x') are fp32 numbers of that
    magnitude (a sum of N terms), so their difference cannot be closer than a few of their ulps."""
    got_m, got_lr = rec.stacked()
    if kind in ('ula', 'uhmc'):
        assert bool(got_m.all()), what                        # unadjusted: every proposal kept
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
    prev = torch.cat([x0.double()[None], states[:-1].double()])         # the state each transition starts from
    u_prev = ref(prev.reshape(-1, d)).reshape(prev.shape[:2])
    err = (got_lr.double() - want_lr).abs()
    tol = 2e-4 * max(1.0, d / 64) + 1e-4 * want_lr.abs() + 8 * 2.0 ** -24 * u_prev.abs()
    print('%s: worst log-ratio error %.2e' % (what, float(err[agree].max())))
    assert bool((err[agree] <= tol[agree]).all()), (what, float(err[agree].max()))


class _Spy:
    """Counts the split-path transitions of the mcmc samplers (none on the fused route)."""

    def __init__(self, monkeypatch):
        from nfmc_amd.samplers import mcmc
        self.calls = []
        orig = mcmc.MCMCSampler._split_step
        monkeypatch.setattr(mcmc.MCMCSampler, '_split_step',
                            lambda s, *a, **k: self.calls.append(1) or orig(s, *a, **k))


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
GRID = [(1, 1), (1, 2500), (3, 64), (7, 63), (16, 65), (25, 1000), (32, 200), (64, 1000), (100, 65), (256, 63),
        (512, 1), (512, 1000), (700, 40)]


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d,N', GRID)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d, N):
    from oracle import samplers as osamp
    from nfmc_amd.samplers import mcmc
    n, T = 96, 4
    pot, ref = _problem(N, d, 10 * d + N)
    x0 = _x0(n, d, d + N)
    h = _step(kind, d)
    s = _sampler(kind, d, pot, T, h)
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(d + N)
    tr = _oracle(kind, x0, ref, T, h, rec)
    s.replay = (torch.stack([v.float() for v in rec.normals]),
                torch.stack([v.float() for v in rec.uniforms]) if rec.uniforms else None)
    assert mcmc.resolve_target(pot, (d,), family='mcmc') is pot
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls                                       # every transition on the fused kernel
    _compare(out.samples.reshape(T, n, d), tr, '%s d=%d N=%d' % (kind, d, N))
    _compare_decisions(rec_k, tr, kind, x0, ref, '%s d=%d N=%d' % (kind, d, N))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d,N', [('mala', 25, 1000), ('ula', 7, 65), ('mh', 33, 300), ('hmc', 64, 129),
                                      ('uhmc', 16, 1100)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, N):
    from oracle import samplers as osamp
    n, T, seed = 160, 5, 777 + d
    pot, ref = _problem(N, d, 7 * d + N)
    x0 = _x0(n, d, N)
    h = _step(kind, d)
    s = _sampler(kind, d, pot, T, h)
    s.seed = seed
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    tr = _oracle(kind, x0, ref, T, h, osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, 'native %s' % kind)
    _compare_decisions(rec_k, tr, kind, x0, ref, 'native %s' % kind)


def _flow_pair(d, seed=5, n_hidden=None):
    from nfmc_amd.flows import Flow, RealNVP
    from oracle import flow as oflow
    ck = {} if n_hidden is None else {'conditioner_kwargs': {'n_hidden': n_hidden}}
    of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,), **ck)), seed, 0.2, 0.7071)
    f = Flow(RealNVP((d,), **ck))
    f.load_state_dict(of.state_dict())
    return f, of.double()


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d,N', [(5, 300), (25, 1000)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d, N):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, T, Kin, seed = 192, 3, 4, 31337
    pot, ref = _problem(N, d, 3 * d + N)
    x0 = _x0(n, d, 3)
    f, of = _flow_pair(d)
    h = 0.3 * d ** (-1 / 3)
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
    tr = osamp.jump_sample(x0.double(), ref, of, 'langevin', T, Kin, h, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < ATOL + RTOL * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > 0.95, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= max(2, int(0.03 * n * T))


@pytest.mark.parametrize('d,N', [(2, 64), (25, 1000), (64, 65), (256, 100)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, N):
    from nfmc_amd.samplers import imh
    from oracle import samplers as osamp
    n, T, seed = 256, 6, 4711 + d
    pot, ref = _problem(N, d, 5 * d + N)
    x0 = _x0(n, d, 9)
    f, of = _flow_pair(d, 9)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=T))
    s.seed = seed
    calls = {'launch_imh_parallel': 0, 'launch_flow_mh': 0, 'split_flow_mh': 0}

    def spy(name):   # the names imh.py calls (bound there by its `from .jump import ...`)
        fn = getattr(imh, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        monkeypatch.setattr(imh, name, wrapped)
    for name in list(calls):
        spy(name)
    out = s.sample(x0, show_progress=False)
    # the sequential flow-MH kernel ran every transition: neither nfmc_imh_parallel_f32 nor the composed step
    assert calls['launch_flow_mh'] >= 1 and calls['launch_imh_parallel'] == 0 and calls['split_flow_mh'] == 0, calls
    assert out.statistics.n_attempted_trajectories == n * T
    tr = osamp.imh_sample(x0.double(), ref, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, 'imh d=%d N=%d' % (d, N))


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d,N', [('mala', 25, 1000), ('hmc', 9, 200), ('mh', 7, 63)])
def test_fused_equals_split(dev, monkeypatch, kind, d, N):
    n, T = 200, 6
    pot, _ = _problem(N, d, 17 * d + N)
    x0 = _x0(n, d, 17)
    outs, counts = [], []
    for target, fuse in ((pot, 'auto'), (lambda x: pot(x), 'never')):
        spy = _Spy(monkeypatch)
        s = _sampler(kind, d, target, T, _step(kind, d))
        s.seed, s.fuse = 2024, fuse
        outs.append(s.sample(x0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T]
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < ATOL
    assert same.float().mean() > 0.95, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 4. refused families
def test_neutra_takes_the_split_path_and_matches_the_oracle(dev):
    from nfmc_amd.samplers import mcmc, neutra
    from oracle import samplers as osamp
    d, n, T, L, h, N = 6, 96, 3, 4, 0.05, 300
    pot, ref = _problem(N, d, 61)
    f, of = _flow_pair(d, 9, n_hidden=8)
    z0 = _x0(n, d, 61)
    s = neutra.NeuTraHMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                         mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))
    assert s._closed_form() is None                          # no descriptor for the neutra kernels
    s.seed = 12
    out = s.sample(z0, show_progress=False)
    tr = osamp.neutra_hmc_sample(z0.double(), ref, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 6


def test_dlmc_borrows_the_gradient_step_and_matches_the_oracle(dev, monkeypatch):
    from nfmc_amd.samplers import dlmc as mod
    from oracle import samplers as osamp
    d, n, T, N, seed = 8, 128, 3, 500, 4242
    pot, ref = _problem(N, d, 71)
    f, of = _flow_pair(d, 3)
    f.fit = lambda *a, **k: None
    x0 = _x0(n, d, 71)
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
    tr = osamp.dlmc_sample(x0, ref, nll, of, T, 0.05, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got = out.samples.cpu().double().reshape(T, n, d)
    same = (got - tr.stacked()).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() >= 0.95, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 0.03 * n * T


def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc, imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    d, n, N = 64, 256, 1000
    pot, _ = _problem(N, d, 4)
    x = _x0(n, d, 4).to(dev)
    f, _ = _flow_pair(d)
    f.to(dev)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_LOGISTIC_REGRESSION and pd.reserved == N
    a, _keep = dlmc.step_args(f, x, 0.05, pot=pot)
    assert int(hip.lib().nfmc_dlmc_step_supported_f32(C.byref(a))) == hip.EUNSUPPORTED
    st, _k2 = f.bijection.packed(dev)
    u = torch.full((n,), 123.0, device=dev)
    gr = torch.full_like(x, 123.0)
    rc = int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(pd), hip.ptr(x), n, hip.ptr(u), hip.ptr(gr),
                                                        hip.stream()))
    torch.cuda.synchronize()
    assert rc == hip.EUNSUPPORTED and bool((u == 123.0).all()) and bool((gr == 123.0).all())
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k3 = _flow_mh_probe_args(run, f, pot, logq, True)
    assert int(hip.lib().nfmc_imh_parallel_supported_f32(C.byref(pa))) == hip.EUNSUPPORTED
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK        # the register kernels take it
    pa.rng.rounds = 7                                                               # the opt-in stream: not for kind 3
    before = run.x.clone()                                                          # the probe arguments' state
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
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    # the device variational fit is never handed the descriptor
    assert not pot.fused_in('fit') and not pot.fused_in('neutra') and not pot.fused_in('dlmc_step')


def test_mala_philox7_and_bad_descriptors_are_refused(dev):
    """The opt-in Philox4x32-7 stream has no kind-3 kernel; a misaligned X or a non-positive 1/s^2 is an argument
    error.  Nothing is written in any of these cases."""
    from nfmc_amd import hip
    d, n, N = 25, 128, 100
    pot, _ = _problem(N, d, 8)
    x = _x0(n, d, 8).to(dev)
    before = x.clone()
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = hip.ptr(x), n, d, 2, 0.1, 1
    a.pot = pot.descriptor(dev)
    a.rng.seed, a.rng.rounds = 3, 7
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    a.rng.rounds = 10
    Xd, _yd = pot._dev[str(dev)]
    a.pot.a = Xd.data_ptr() + 4
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EALIGN
    a.pot = pot.descriptor(dev)
    a.pot.a_scalar = 0.0
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x, before)


# ------------------------------------------------------------------------- 5. separable data
@pytest.mark.parametrize('kind', KINDS)
def test_separable_data_stay_finite(dev, kind):
    """Labels of sign(X w): the likelihood has no maximum and its logits reach hundreds along w (x0 starts there)."""
    from nfmc_amd.potentials import BayesianLogisticRegression
    d, N, n, T = 10, 500, 512, 20
    X, y, w = synthetic(N, d, 13, scale=3.0, separable=True)
    pot = BayesianLogisticRegression(X, y, 100.0)
    zmax = float((X.double() @ w.double()).abs().max())
    x0 = (300.0 / zmax) * w[None].float().repeat(n, 1) + 0.1 * torch.randn(n, d, generator=torch.Generator().manual_seed(1))
    assert float((x0.double() @ X.double().t()).abs().max()) > 200
    s = _sampler(kind, d, pot, T, _step(kind, d) * 0.1)
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    assert torch.isfinite(out.samples).all()
    assert torch.isfinite(out.mean).all() and torch.isfinite(out.second_moment).all()
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert 0 <= st.n_accepted_trajectories <= n * T
    assert getattr(st, 'n_divergences', 0) == 0


# ------------------------------------------------------------------------- 6. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    from nfmc_amd.dist import Shard
    d, n, T, N = 20, 300, 8, 700
    pot, _ = _problem(N, d, 44)
    x0 = _x0(n, d, 44)
    runs = []
    for _ in range(2):
        s = _sampler(kind, d, pot, T, _step(kind, d))
        s.seed = 7
        runs.append(s.sample(x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories
    dense = runs[0].samples.reshape(T, n, d)
    parts = []
    for r in range(2):
        sh = Shard(rank=r, world=2)
        sh.merge_statistics = lambda s_: s_
        s = _sampler(kind, d, pot, T, _step(kind, d))
        s.seed, s.shard = 7, sh
        parts.append(s.sample(x0, show_progress=False).samples.reshape(T, -1, d))
    assert torch.equal(torch.cat(parts, 1), dense)


def test_every_device_gets_its_own_copy(dev):
    from nfmc_amd import hip
    pot, _ = _problem(50, 4, 1)
    devices = [torch.device('cuda', i) for i in range(torch.cuda.device_count())]
    descs = [pot.descriptor(dv) for dv in devices]
    assert len(pot._dev) == len(devices)
    assert len({dsc.a for dsc in descs}) == len(devices)
    for dv in devices:
        Xd, yd = pot._dev[str(dv)]
        assert Xd.device == dv and yd.device == dv and Xd.data_ptr() % 16 == 0
    assert all(dsc.kind == hip.POT_LOGISTIC_REGRESSION for dsc in descs)


# ------------------------------------------------------------------------- 7. Stein identities, no oracle run
def test_stein_identities_on_the_fused_mala_kernel(dev, monkeypatch):
    """For theta ~ pi = e^-U / Z:  E[dU/dtheta_j] = 0 and E[theta_j dU/dtheta_j] = 1 (integration by parts; the prior
    makes the boundary terms vanish).  d = 5, N = 2000, sigma = 2, 4096 chains of fused MALA; the kept states of the
    second half of the run.  The Monte Carlo standard error of each mean comes from the per-chain time averages (chains
    are independent, so their averages are too); the identities must hold within 5 of them."""
    from nfmc_amd.potentials import BayesianLogisticRegression
    d, N, sigma, n, T = 5, 2000, 2.0, 4096, 400
    X, y, _ = synthetic(N, d, 2024)
    X[:, 0] = 1.0                                                        # an intercept column
    pot = BayesianLogisticRegression(X, y, sigma)
    ref = LogRegU64(X, y, sigma)
    # start near the mode: a few Newton steps in fp64
    th = torch.zeros(1, d, dtype=torch.float64)
    for _ in range(20):
        p = torch.sigmoid(th @ ref.X.t())[0]
        H = (ref.X * (p * (1 - p))[:, None]).t() @ ref.X + torch.eye(d, dtype=torch.float64) / sigma ** 2
        th = th - torch.linalg.solve(H, ref.grad(th)[0])[None]
    cov = torch.linalg.inv(H)
    g = torch.Generator().manual_seed(3)
    x0 = (th + torch.randn(n, d, generator=g, dtype=torch.float64) @ torch.linalg.cholesky(cov).t()).float()
    h = 0.5 * float(torch.linalg.eigvalsh(cov).min())
    s = _sampler('mala', d, pot, T, h)
    s.seed = 11
    spy = _Spy(monkeypatch)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    assert 0.3 < acc < 0.99, acc
    kept = out.samples.reshape(T, n, d)[T // 2::2].to(dev, torch.float64)   # (T/4, n, d)
    Xd, yd = ref.X.to(dev), ref.y.to(dev)
    gu = (torch.sigmoid(kept @ Xd.t()) - yd) @ Xd + kept / sigma ** 2     # closed-form grad U in fp64
    for name, f, target in (('E[grad U]', gu, 0.0), ('E[theta grad U]', kept * gu, 1.0)):
        per_chain = f.mean(0).cpu()                                      # (n, d)
        mean = per_chain.mean(0)
        se = per_chain.std(0) / math.sqrt(n)
        z = (mean - target) / se
        print(name, mean.tolist(), se.tolist())
        assert bool((z.abs() < 5).all()), (name, mean.tolist(), se.tolist())
