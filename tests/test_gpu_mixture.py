"""GPU: GaussianMixture (NFMC_POT_GAUSSIAN_MIXTURE) on the fused HIP kernels against the fp64 CPU oracle.

Tolerances (fp32 kernels, fp64 oracle on the same noise):
  states        atol 1e-3 + rtol 1e-4.  U is a logsumexp over K group sums of d terms; at d = 512 those sums are
                O(d) and their fp32 rounding (~d * 6e-8 relative) moves U, the responsibilities and so the gradient by
                ~1e-4 per transition.
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded (its decision is ill-conditioned in fp32 and a flip changes the rest of its trajectory).  The
                excluded share is reported and must stay under 10 %; all other chains must match.

Flow-proposal cases (section 2 and 2b): from d = 25 on a flow centred by a Laplace fit (H.flow_inputs).  The fp64 oracle
alone accepts up to 0.085 of the jumps (none at d = 16, a flow about the origin: skip_below_minus_50, log ratios down to
-141) and 0.168 to 0.421 of the IMH proposals of section 2, and in the matrix 0.227 to 0.836 up to capacity 128 and 0.292
to 0.510 above; at most 2.1 % of the chains of a case are within MARGIN of a tie, and every other log ratio is above -18.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import target_harness as H
from target_harness import flow_pair as _flow_pair

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _mixture(K, d, seed, spread=2.0):
    from nfmc_amd.potentials import GaussianMixture
    g = torch.Generator().manual_seed(seed)
    means = spread * torch.randn(K, d, generator=g, dtype=torch.float64)
    scales = 0.6 + 0.8 * torch.rand(K, d, generator=g, dtype=torch.float64)
    weights = 0.2 + torch.rand(K, generator=g, dtype=torch.float64)
    return GaussianMixture((d,), means, scales, weights), g


def _x0(pot, n, g):
    k = torch.randint(0, pot.n_components, (n,), generator=g)
    return (pot.means[k] + 0.7 * torch.randn(n, pot.event_size, generator=g, dtype=torch.float64)).float()


def _record(K, d, seed, n, spread=2.0):
    """the problem as the harness takes it: the class itself, called in fp64, is the oracle's target"""
    pot, g = _mixture(K, d, seed, spread)
    return H.Problem(pot, pot, pot, _x0(pot, n, g), d, 'K=%d d=%d' % (K, d))


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(d):
    return torch.full((d,), 0.3 / math.sqrt(d))


def _step(kind, d):
    return {'mala': 0.3, 'ula': 0.05, 'mh': 0.0, 'hmc': 0.1, 'uhmc': 0.05}[kind] * d ** (-1 / 3) if kind != 'mh' else 0.0


def _against_oracle(check, monkeypatch, kind, p, T, **kw):
    """states alone: the kernel's masks and log ratios are not recorded for this kind"""
    h, imd = _step(kind, p.d), _mh_scale(p.d)
    check(monkeypatch, p, kind, T, _sampler(kind, p.d, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd.double()), compare=_compare, decisions=None, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', ['mala', 'ula', 'mh', 'hmc', 'uhmc'])
@pytest.mark.parametrize('K', [1, 2, 5, 8])
@pytest.mark.parametrize('d', [2, 7, 64, 256, 512])
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, K, d):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _record(K, d, 1000 * K + d, 96), 4, torch_seed=d + K,
                    what='%s K=%d d=%d' % (kind, K, d))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,K,d', [('mala', 3, 64), ('ula', 2, 7), ('mh', 5, 33), ('hmc', 8, 256), ('uhmc', 4, 16)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, K, d):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, _record(K, d, 7 * K + d, 160), 5, seed=777 + d,
                    what='native %s' % kind)


@functools.lru_cache(maxsize=None)
def _flow_built(K, d, seed, n, spread):
    """one object per distinct problem of the flow tests: the Laplace fit (H.laplace_fit) is kept per object"""
    return _record(K, d, seed, n, spread=spread)


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('K,d', [(2, 16), (5, 64)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, K, d):
    """jump_mala on a fixed perturbed flow: inner MALA fused, the jump on the register flow-MH kernel (or as the tail of
    the last inner launch)."""
    n, T = 192, 3
    p = _flow_built(K, d, 3 * K + d, n, 1.0)
    q, flows = H.flow_inputs(p, d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3),
                               imd=None, fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=d < 25, flows=flows)


# ------------------------------------------------------------------------- 2b. the flow-MH matrix
FLOW_CASES = H.flow_cases()
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_native_stream_matches_oracle', 'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling (the MixturePot arms of launch_b and launch_b_rqs),
    the unadjusted carry path and the jump tails, with decisions and log ratios compared row by row (H.compare_flow_mh);
    K rotates with the capacity, the components overlap (spread 0.5) so that one Gaussian proposal covers them"""
    d = case.d
    K = (2, 5, 1, 8)[int(math.log2(case.cap)) % 4]
    p = _flow_built(K, d, 5 * K + d, 96, 0.5)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=0.3 * d ** (-1 / 3), h_hmc=_step('hmc', d), refused=H.flow_case_id(case) in FLOW_REFUSED)


@pytest.mark.parametrize('K,d', [(1, 7), (4, 64), (8, 256)])
def test_imh_native_stream_matches_oracle(dev, monkeypatch, K, d):
    """nfmc_imh_parallel_supported_f32 answers no for kind 2: the sequential flow-MH kernel runs (H.imh_run asserts it)"""
    p = _flow_built(K, d, 5 * K + d, 256, 0.5)
    q, flows = H.flow_inputs(p, d, 256, 9)
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=9, spline=False, compare=_compare,
                         what='imh K=%d d=%d' % (K, d), margin=MARGIN, skip_below_minus_50=False, flows=flows)


# ------------------------------------------------------------------------- 3. K = 1 is a diagonal Gaussian
@pytest.mark.parametrize('kind', ['mala', 'hmc', 'mh'])
def test_one_component_equals_diagonal_gaussian(dev, kind):
    from nfmc_amd.potentials import DiagonalGaussian, GaussianMixture
    d, n, T = 48, 256, 8
    g = torch.Generator().manual_seed(1)
    mu = torch.randn(d, generator=g)
    sig = 0.5 + torch.rand(d, generator=g)
    mix = GaussianMixture(d, mu[None], sig[None], [3.0])
    gau = DiagonalGaussian(d, mu, sig)
    x0 = mu + sig * torch.randn(n, d, generator=g)
    outs = []
    for pot in (mix, gau):
        s = _sampler(kind, d, pot, T, _step(kind, d))
        if kind == 'mh':
            s.kernel.inv_mass_diag = torch.full((d,), 0.1)
        s.seed = 99
        outs.append(s.sample(x0, show_progress=False))
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < 1e-4
    assert same.float().mean() > 0.97, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=1e-4, rtol=1e-5)
    assert abs(outs[0].statistics.n_accepted_trajectories - outs[1].statistics.n_accepted_trajectories) <= \
        int((~same).sum()) * T


# ------------------------------------------------------------------------- 4. fused equals split
@pytest.mark.parametrize('kind,K,d', [('mala', 3, 64), ('hmc', 5, 20), ('mh', 2, 7)])
def test_fused_equals_split(dev, monkeypatch, kind, K, d):
    T = 6
    H.fused_equals_split(monkeypatch, _record(K, d, 17 * K + d, 200),
                         lambda target: _sampler(kind, d, target, T, _step(kind, d), imd=_mh_scale(d)), T,
                         seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 5. refused families take the split / composed path
def test_nine_components_take_the_split_path_and_match_the_oracle(dev):
    from oracle import samplers as osamp
    from nfmc_amd.samplers import mcmc
    d, n, T = 12, 128, 5
    pot, g = _mixture(9, d, 9)
    assert not pot.fused_in('mcmc') and not pot.fused_in('flow_mh')
    x0 = _x0(pot, n, g)
    h = _step('mala', d)
    s = _sampler('mala', d, pot, T, h)
    s.seed = 5
    spy = []
    orig = mcmc.MALA._split_step
    mcmc.MALA._split_step = lambda self, *a, **k: spy.append(1) or orig(self, *a, **k)
    try:
        out = s.sample(x0, show_progress=False)
    finally:
        mcmc.MALA._split_step = orig
    assert len(spy) == T
    tr = _oracle('mala', x0, pot, T, h, osamp.PhiloxNoise(5, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, 'mala K=9 split')


def test_refused_families_run_split_or_composed(dev):
    from nfmc_amd import flow_training
    from nfmc_amd.sample import create_sampler
    from nfmc_amd.samplers.dlmc import DLMC, DLMCKernel, DLMCParameters
    d, n = 6, 64
    pot, g = _mixture(3, d, 3, spread=1.0)
    x0 = _x0(pot, n, g)
    # NeuTra: no descriptor for kind 2 -> the inner sampler's split path on the adjusted target
    s = create_sampler(pot, (d,), strategy='neutra_hmc', param_kwargs={'n_iterations': 4})
    assert s._closed_form() is None
    s.seed = 1
    out = s.sample(x0, show_progress=False)
    assert torch.isfinite(out.samples).all()
    # dlmc: the gradient step is borrowed (grad U by autograd), the MH step runs on the flow-MH kernel
    f, _ = _flow_pair(d)
    ds = DLMC((d,), pot, lambda x: 0.5 * (x ** 2).sum(-1), DLMCKernel((d,), flow=f, step_size=0.05),
              DLMCParameters(n_iterations=3))
    ds.seed = 2
    out = ds.sample(x0, show_progress=False)
    assert ds.last_route == 'borrowed' and torch.isfinite(out.samples).all()
    # imh with the variational warmup fit: the torch loop, not the device fit (which answers NFMC_EUNSUPPORTED)
    loops = []
    orig = flow_training._loop
    flow_training._loop = lambda *a, **k: loops.append(1) or orig(*a, **k)
    try:
        si = create_sampler(pot, (d,), strategy='imh', param_kwargs={'n_iterations': 4})
        si.params.warmup_fit_kwargs = dict(si.params.warmup_fit_kwargs, n_epochs=3)
        si.seed = 3
        si.warmup(x0, show_progress=False)
    finally:
        flow_training._loop = orig
    assert loops
    out = si.sample(x0, show_progress=False)
    assert torch.isfinite(out.samples).all()


def test_jump_mala_wide_conditioner_composes_the_jump(dev):
    """Conditioner wider than 32: the flow-MH kernels answer no; inner MALA stays fused, the jump is composed from the
    flow's own kernels and the mixture's torch U -- and still matches the oracle."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.samplers import jump, mcmc
    from oracle import flow as oflow, samplers as osamp
    d, n, T, Kin, seed = 16, 128, 2, 3, 11
    pot, g = _mixture(2, d, 21, spread=1.0)
    x0 = _x0(pot, n, g)
    of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,), conditioner_kwargs={'n_hidden': 48})), 5, 0.2, 0.7071)
    f = Flow(RealNVP((d,), conditioner_kwargs={'n_hidden': 48}))
    f.load_state_dict(of.state_dict())
    spy = []
    orig = jump.split_flow_mh
    jump.split_flow_mh = lambda *a, **k: spy.append(1) or orig(*a, **k)
    try:
        s = jump.JumpMALA((d,), pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), None,
                          mcmc.LangevinParameters(n_iterations=Kin))
        s.seed = seed
        out = s.sample(x0, show_progress=False)
    finally:
        jump.split_flow_mh = orig
    assert len(spy) == T
    tr = osamp.jump_sample(x0.double(), pot, of.double(), 'langevin', T, Kin, d ** (-1 / 3),
                           noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 2e-3
    assert same.float().mean() > 0.95, float(same.float().mean())


# ------------------------------------------------------------------------- 6. kind 2 on the refusing entry points
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    d = 64
    pot, g = _mixture(3, d, 4)
    assert pot.descriptor(dev).kind == hip.POT_GAUSSIAN_MIXTURE
    # no NeuTra kernels for kind 2 either
    pa, _keep = H.refusing_entry_points(dev, pot, _x0(pot, 256, g), functools.partial(_flow_pair, d),
                                        neutra_fused=False)
    pa.pot.n_components = 9                                                             # K over the cap
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.EUNSUPPORTED
    assert hip.EUNSUPPORTED < 0 and pot.fused_in('fit') is False


# ------------------------------------------------------------------------- 7. determinism, sharding, store
def test_determinism_sharding_and_store(dev):
    d, n, T = 20, 300, 12
    p = _record(4, d, 44, n)
    make = lambda: _sampler('mala', d, p.pot, T, _step('mala', d))   # noqa: E731
    dense = H.determinism_and_sharding(make, p.x0, T, d, seed=7, world=2)
    # thinning / max_samples keep states of the dense run, in order
    s = make()
    s.seed = 7
    s.params.thinning, s.params.max_samples = 3, 3
    kept = s.sample(p.x0, show_progress=False).samples.reshape(-1, n, d)
    assert kept.shape[0] == 3
    idx = [next(t for t in range(T) if torch.equal(kept[i], dense[t])) for i in range(3)]
    assert idx == sorted(idx) and len(set(idx)) == 3


# ------------------------------------------------------------------------- 8. what the feature is for
def test_imh_reaches_mode_weights_mala_stays(dev):
    """Two modes 8 apart in each of d = 4 coordinates (weights 0.7 / 0.3, unit scales); every chain starts in the minor
    mode.  MALA at h = 0.3 cannot cross a barrier of U ~ 8^2 * 4 / 8 = 32 nats in T = 200 steps (the minor-mode share
    must stay above 0.99).  IMH with a flow fitted on exact mixture draws must reach the 0.7 / 0.3 split: with n = 4096
    chains the share of the major mode after T steps is a binomial proportion with standard error
    sqrt(0.7 * 0.3 / 4096) = 0.0072 (chains are independent; the fitted flow's leftover bias adds to it), and the test
    allows 5 of them.  Seeded: the run, the fit and the draws are deterministic."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.potentials import GaussianMixture
    from nfmc_amd.samplers import imh
    d, n = 4, 4096
    mu = torch.tensor([[4.0] * d, [-4.0] * d])
    pot = GaussianMixture(d, mu, 1.0, [0.7, 0.3])
    g = torch.Generator().manual_seed(0)
    x0 = mu[1] + torch.randn(n, d, generator=g)
    s = _sampler('mala', d, pot, 200, 0.3)
    s.seed = 1
    s.params.store_samples = False
    last = s.sample(x0, show_progress=False).running_samples.last_sample
    minor = float((last.sum(1) < 0).float().mean())
    assert minor > 0.99, minor
    # exact draws of the mixture, a flow fitted on them
    torch.manual_seed(2)
    k = (torch.rand(20000, generator=g) < 0.3).long()
    draws = mu[k] + torch.randn(20000, d, generator=g)
    f = Flow(RealNVP((d,)))
    f.fit(draws, n_epochs=100, show_progress=False)
    si = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=200))
    si.seed = 3
    si.params.store_samples = False
    last = si.sample(x0, show_progress=False).running_samples.last_sample
    major = float((last.sum(1) > 0).float().mean())
    assert abs(major - 0.7) < 5 * math.sqrt(0.21 / n), major
