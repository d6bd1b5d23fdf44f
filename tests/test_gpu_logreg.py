"""GPU: BayesianLogisticRegression (NFMC_POT_LOGISTIC_REGRESSION) on the fused HIP kernels against the fp64 CPU oracle,
with the target restated in fp64 (tests/logreg_fp64.py).

Tolerances are the mixture tests' (tests/test_gpu_mixture.py):
  states        atol 1e-3 + rtol 1e-4.  U is a sum of N terms and the gradient a sum of N rows; the data are scaled so
                that the posterior curvature is O(1) at every N, and the fp32 sums move a transition by ~1e-5.
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

The (d, N) grid covers every (CPL, LPC) layout the sampler kernels pick (d = 1 ... 700: LPC 1 ... 64, CPL 4 / 8 / 16),
N = 1, 63, 64, 65 and 1000, and N past the LDS tile of its layout (4096 / (CPL LPC) rows: 1024 at d <= 4, 8 at d = 512).

Flow-proposal cases (section 2 and 2b): from d = 25 on a flow centred by a Laplace fit (H.flow_inputs).  The fp64 oracle
alone accepts 0.160 to 0.267 of the jumps and 0.191 to 0.436 of the IMH proposals of section 2, and in the matrix 0.104 to
0.833 up to capacity 128 and 0.115 to 0.422 above; at most 1.0 % of the chains of a case are within MARGIN of a tie.  IMH
at d = 256 and the matrix at capacity 256 have fp64 log ratios down to -76 and set skip_below_minus_50, as does the jump
at d = 5; the others keep every log ratio above -50.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import target_harness as H
from logreg_fp64 import LogRegU64, synthetic
from target_harness import Spy as _Spy, flow_pair as _flow_pair

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


def _record(N, d, seed, n, x0_seed):
    """the problem as the harness takes it: the restatement is the oracle's target"""
    pot, ref = _problem(N, d, seed)
    return H.Problem(pot, ref, ref, _x0(n, d, x0_seed), d, 'd=%d N=%d' % (d, N))


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)


def _mh_scale(d):
    return torch.full((d,), 0.3 / math.sqrt(d), dtype=torch.float64)


def _sampler(kind, d, pot, T, h, L=5):
    return H.mcmc_sampler(kind, d, pot, T, h, L, _mh_scale(d), imd_kinds=('mh',))


def _oracle(kind, x0, target, T, h, noise, L=5):
    return H.oracle_trace(kind, x0, target, T, h, noise, L, _mh_scale(x0.shape[1]), imd_kinds=('mh',))


def _step(kind, d):
    return {'mala': 0.3, 'ula': 0.05, 'mh': 0.0, 'hmc': 0.1, 'uhmc': 0.05}[kind] * d ** (-1 / 3)


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
GRID = [(1, 1), (1, 2500), (3, 64), (7, 63), (16, 65), (25, 1000), (32, 200), (64, 1000), (100, 65), (256, 63),
        (512, 1), (512, 1000), (700, 40)]


def _against_oracle(check, monkeypatch, kind, p, T, **kw):
    """Log ratios: the kernel's U(x) and U(x') are fp32 numbers of the magnitude of U (a sum of N terms), so their
    difference cannot be closer than a few of their ulps (H.compare_decisions)."""
    h = _step(kind, p.d)
    check(monkeypatch, p, kind, T, _sampler(kind, p.d, p.pot, T, h), lambda noise: _oracle(kind, p.x0, p.target, T, h, noise),
          compare=_compare, decisions=H.compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d,N', GRID)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d, N):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _record(N, d, 10 * d + N, 96, d + N), 4, torch_seed=d + N,
                    what='%s d=%d N=%d' % (kind, d, N))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d,N', [('mala', 25, 1000), ('ula', 7, 65), ('mh', 33, 300), ('hmc', 64, 129),
                                      ('uhmc', 16, 1100)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, N):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, _record(N, d, 7 * d + N, 160, N), 5, seed=777 + d,
                    what='native %s' % kind)


@functools.lru_cache(maxsize=None)
def _flow_built(N, d, seed, n, x0_seed):
    """one object per distinct problem of the flow tests: the Laplace fit (H.laplace_fit) is kept per object"""
    return _record(N, d, seed, n, x0_seed)


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d,N', [(5, 300), (25, 1000)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d, N):
    n, T = 192, 3
    p = _flow_built(N, d, 3 * d + N, n, 3)
    q, flows = H.flow_inputs(p, d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3),
                               imd=None, fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=d < 25, flows=flows)


@pytest.mark.parametrize('d,N', [(2, 64), (25, 1000), (64, 65), (256, 100)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, N):
    p = _flow_built(N, d, 5 * d + N, 256, 9)
    q, flows = H.flow_inputs(p, d, 256, 9)
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=9, spline=False,
                         compare=_compare, what='imh d=%d N=%d' % (d, N), margin=MARGIN, skip_below_minus_50=d >= 200, flows=flows)


# ------------------------------------------------------------------------- 2b. the flow-MH matrix
FLOW_CASES = H.flow_cases()
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound with this kind's 16 KB tile of X behind the image: two affine coupling layers of width 8 at the
# ragged capacity 512 are 132 KB by themselves, two spline layers of width 8 at capacity 64 are 111 KB
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8', 'mh-cap64-d50-h8-spline', 'mh-cap64-d50-h8-cpl8-spline'}


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling (the LogRegPot arms of launch_b and launch_b_rqs),
    the unadjusted carry path and the jump tails, with decisions and log ratios compared row by row (H.compare_flow_mh);
    N rotates with the capacity over row counts around the 16 KB tile"""
    d = case.d
    N = (65, 300, 1000, 63)[int(math.log2(case.cap)) % 4]
    p = _flow_built(N, d, 5 * d + N, 96, 9)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=0.3 * d ** (-1 / 3), h_hmc=_step('hmc', d), refused=H.flow_case_id(case) in FLOW_REFUSED,
                    skip_caps=(256,))    # d = 200 on N = 65 rows: fp64 log ratios down to -60


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d,N', [('mala', 25, 1000), ('hmc', 9, 200), ('mh', 7, 63)])
def test_fused_equals_split(dev, monkeypatch, kind, d, N):
    T = 6
    H.fused_equals_split(monkeypatch, _record(N, d, 17 * d + N, 200, 17),
                         lambda target: _sampler(kind, d, target, T, _step(kind, d)), T, seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


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
    d, N = 64, 1000
    pot, _ = _problem(N, d, 4)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_LOGISTIC_REGRESSION and pd.n_components == N
    # no NeuTra kernels for kind 3 either
    H.refusing_entry_points(dev, pot, _x0(256, d, 4), functools.partial(_flow_pair, d), neutra_fused=False)


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
    d, T = 20, 8
    pot, _ = _problem(700, d, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, pot, T, _step(kind, d)), _x0(300, d, 44), T, d, seed=7, world=2)


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
