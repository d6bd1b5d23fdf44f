"""GPU: Rosenbrock (NFMC_POT_ROSENBROCK) on the fused HIP kernels against the fp64 CPU oracle, with the target restated
in fp64 (tests/rosenbrock_fp64.py).

Targets: blocks of 1, 2, 3 and 5 coordinates (capped at d), plus one block = d target with a narrow head, so that one
chain of neighbours runs through every register quad and lane of the layout and across the lane-(LPC-1)-to-lane-0
wrap.  Starts are exact (ancestral) draws of the target.  Block 2 has a wide head around 0.5; longer blocks a narrower one
around 0.2 and a tighter conditional, so that x_{c-1}^2 stays O(1) along the block.  Step sizes scale with the largest
diagonal Hessian entry at the start (90th percentile over the chains), as any sampler of a curved target must.

Tolerances are the full-rank Gaussian tests' (tests/test_gpu_fullrank.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

d in {1, 3, 8, 25, 64, 130, 256, 512} covers every (CPL, LPC) layout choose_cfg picks (LPC 1 ... 64, CPL 4 / 8 / 16).

Flow-proposal cases (section 2 and 2b).  Section 2 runs from d = 25 on a flow centred by a Laplace fit (H.flow_inputs):
the fp64 oracle alone accepts 0.031 to 0.123 of the jumps, 0.192 to 0.277 of the IMH proposals and 0.001 to 0.266 of the
spline ones.  A Gaussian with the mode's marginal scales does not cover the ridge, so the matrix proposes inside it
(_flow_centre: the mode, 0.3 of the conditional standard deviations): the oracle alone accepts 0.234 to 0.573 up to
capacity 128 and 0.336 to 0.411 above.  Under 1 % of the chains of a case are within MARGIN of a tie.  A proposal off
the ridge is hopeless (fp64 log ratios down to -4375, in the matrix -63): every case sets skip_below_minus_50.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from rosenbrock_fp64 import RosenbrockU64
from target_harness import Spy as _Spy, flow_pair as _flow_pair, imh_run as _imh_run

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4
SKIP = True     # skip_below_minus_50 of the flow-MH cases: a proposal off the ridge is hopeless: see the docstring


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _params(d, blk):
    """(mu, a, b): block <= 2 a wide head; longer blocks a narrow head and a tight conditional; block = d > 5 (the
    neighbour chain through the whole layout) mu = 0 and a very narrow head"""
    if blk <= 2:
        return 0.5, 2.0, 10.0
    if blk == d and d > 5:
        return 0.0, 50.0, 20.0
    return 0.2, 8.0, 16.0


def _problem(d, blk, params=None):
    from nfmc_amd.potentials import Rosenbrock
    mu, a, b = params if params is not None else _params(d, blk)
    return Rosenbrock(d, mu=mu, a=a, b=b, block=blk), RosenbrockU64(d, mu, a, b, blk)


def _x0(ref, n, seed):
    return ref.draw(n, seed).float()


def _lmax(ref, x0):
    return float(torch.quantile(ref.hess_diag(x0.double()).abs().amax(dim=1), 0.9))


def _record(d, blk, n, seed):
    """the problem as the harness takes it (the restatement is the oracle's target), and the curvature its steps scale with"""
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, seed)
    return H.Problem(pot, ref, ref, x0, d, 'd=%d block=%d' % (d, blk)), _lmax(ref, x0)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(d, lm):
    return torch.full((d,), 0.5 / math.sqrt(d * lm), dtype=torch.float64)


def _step(kind, d, lm):
    """MALA h ~ d^(-1/3) / lambda_max; HMC h ~ d^(-1/4) / sqrt(lambda_max)"""
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * d ** (-1 / 4) / math.sqrt(lm)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * d ** (-1 / 3) / lm


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
DIMS = [1, 3, 8, 25, 64, 130, 256, 512]


def _shapes():
    out = []
    for d in DIMS:
        for blk in sorted({min(b, d) for b in (1, 2, 3, 5)}):
            out.append((d, blk))
    out += [(64, 64), (130, 130), (512, 512)]   # one neighbour chain through every lane, narrow head
    return out


def _against_oracle(check, monkeypatch, kind, d, blk, n, T, x0_seed, **kw):
    p, lm = _record(d, blk, n, x0_seed)
    h, imd = _step(kind, d, lm), _mh_scale(d, lm)
    check(monkeypatch, p, kind, T, _sampler(kind, d, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd), compare=_compare, decisions=H.compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d,blk', _shapes())
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d, blk):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, d, blk, 96, 4, d + 7 * blk, torch_seed=d + blk,
                    what='%s d=%d block=%d' % (kind, d, blk))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d,blk', [('mala', 25, 2), ('ula', 8, 3), ('mh', 130, 5), ('hmc', 64, 2), ('uhmc', 3, 3),
                                        ('hmc', 512, 512), ('mala', 256, 3)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, blk):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, d, blk, 160, 5, d, seed=777 + d,
                    what='native %s d=%d block=%d' % (kind, d, blk))


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d,blk', [(5, 2), (25, 3), (64, 2)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d, blk):
    n, T = 192, 3
    p, lm = _record(d, blk, n, 3)
    q, flows = H.flow_inputs(p, d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3) / lm, imd=None, fuse_tail=fuse_tail,
                               spline=False, atol=ATOL, rtol=RTOL, share=0.95, jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN,
                               skip_below_minus_50=SKIP, flows=flows)


@pytest.mark.parametrize('d,blk', [(2, 2), (25, 5), (64, 64), (256, 3)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, blk):
    p, _lm = _record(d, blk, 256, 9)
    q, flows = H.flow_inputs(p, d, 256, 9)
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=9, spline=False, compare=_compare,
                         what='imh d=%d block=%d' % (d, blk), margin=MARGIN, skip_below_minus_50=SKIP, flows=flows)


@pytest.mark.parametrize('d,blk', [(6, 2), (33, 3)])
def test_spline_flow_imh_matches_oracle(dev, monkeypatch, d, blk):
    """A 'c-rqnsf' flow: the spline instantiations of the register flow-MH kernel for kind 5."""
    p, _lm = _record(d, blk, 256, 11)
    q, flows = H.flow_inputs(p, d, 256, 3, spline=True)
    H.imh_matches_oracle(monkeypatch, q, T=5, seed=99 + d, flow_seed=3, spline=True, compare=_compare,
                         what='c-rqnsf imh d=%d block=%d' % (d, blk), margin=MARGIN, skip_below_minus_50=SKIP, flows=flows)


# ------------------------------------------------------------------------- 2b. the flow-MH matrix
FLOW_SKIP_CAPS = (4, 8, 16, 32, 64, 128, 256, 512)    # some proposals are hopeless at every capacity: see the docstring
FLOW_CASES = H.flow_cases()
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_spline_flow_imh_matches_oracle', 'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}
FLOW_SHRINK = 0.3


@functools.lru_cache(maxsize=None)
def _flow_problem(d):
    """one object per distinct problem of the flow tests: the fit of the proposal's centre is kept per object"""
    return _record(d, 2 + d % 2, 96, 9)


def _flow_centre(p):
    """A Gaussian with the mode's marginal scales does not cover the ridge (the fp64 oracle alone accepts under 5 % from d = 50); the
    proposals sit inside the ridge instead: the mode, FLOW_SHRINK of the conditional standard deviations"""
    return H.local_fit(p, FLOW_SHRINK, at='mode')


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh).  The inner steps of the jump cases shrink with the
    proposal (FLOW_SHRINK^2 for MALA, FLOW_SHRINK for HMC), so that a chain is still inside it when the jump comes."""
    d = case.d
    p, lm = _flow_problem(d)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=FLOW_SHRINK ** 2 * 0.3 * d ** (-1 / 3) / lm, h_hmc=FLOW_SHRINK * _step('hmc', d, lm),
                    refused=H.flow_case_id(case) in FLOW_REFUSED, centre=_flow_centre(p), skip_caps=FLOW_SKIP_CAPS)



def test_dual_chain_override_does_not_apply(dev, monkeypatch):
    """The dual-chain flow-MH kernel evaluates exact-fit quadratic targets only: with its override on, a kind-5 run
    still takes the one-chain register kernel and gives bitwise the same states."""
    d, n, T, seed = 256, 512, 3, 5
    pot, ref = _problem(d, 2)
    x0 = _x0(ref, n, 12)
    f, _ = _flow_pair(d, 4)
    outs = []
    for dual in (None, '1'):
        if dual:
            monkeypatch.setenv('NFMC_FLOWB_DUAL', dual)
        outs.append(_imh_run(monkeypatch, pot, d, f, x0, T, seed).samples)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d,blk', [('mala', 25, 2), ('hmc', 9, 3), ('mh', 64, 5), ('hmc', 130, 130)])
def test_fused_equals_split(dev, monkeypatch, kind, d, blk):
    T = 6
    p, lm = _record(d, blk, 200, 17)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, d, target, T, _step(kind, d, lm), imd=_mh_scale(d, lm)), T,
                         seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 4. NeuTra (VALU kernels)
@pytest.mark.parametrize('d,nh,blk', [(2, 4, 2), (3, 8, 3), (8, 16, 5), (25, 32, 2), (64, 8, 3), (64, 32, 64),
                                      (128, 16, 2), (130, 8, 5), (256, 4, 2)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh, blk):
    """Against fp64 autograd through oracle/flow.py, at latents whose images under the (near-identity) flow are
    target-like: exact draws.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    pot, ref = _problem(d, blk)
    H.neutra_gradient_matches_autograd(dev, pot, ref, ref.draw(130, d), nh, 'd=%d H=%d block=%d' % (d, nh, blk), flow_seed=3,
                                       bound=2e-4)


@pytest.mark.parametrize('d,nh,blk', [(8, 8, 2), (64, 16, 3), (128, 8, 2)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh, blk):
    p, lm = _record(d, blk, 96, 61)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(lm), seed=12,
                                      atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 64
    p, lm = _record(d, 2, 96, 62)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(lm), seed=12,
                                       atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 5. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    d = 64
    pot, ref = _problem(d, 2)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_ROSENBROCK and pd.n_components == 2
    H.refusing_entry_points(dev, pot, _x0(ref, 256, 4), functools.partial(_flow_pair, d))


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL mu, a block of 0 or past d and a or b not positive and finite are argument errors."""
    from nfmc_amd import hip
    d = 25
    pot, ref = _problem(d, 3)
    bad = [('a', 0), ('n_components', 0), ('n_components', d + 1), ('n_components', -1), ('a_scalar', 0.0), ('a_scalar', -1.0),
           ('a_scalar', float('inf')), ('b_scalar', 0.0), ('b_scalar', float('nan'))]
    H.bad_descriptors_are_refused(dev, pot, _x0(ref, 128, 8), _flow_pair(d)[0], [(f, v, hip.EINVAL) for f, v in bad])


# ------------------------------------------------------------------------- 6. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    d, T = 20, 8
    p, lm = _record(d, 3, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, d, lm)), p.x0, T, d, seed=7, world=2)


def test_sample_api_with_a_two_dimensional_event(dev):
    """nfmc_amd.sample() takes the object and its (2, 4) event shape; the kernels see the flattened d = 8."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import Rosenbrock
    pot = Rosenbrock((2, 4), mu=0.5, a=2.0, b=10.0, block=2)
    ref = RosenbrockU64(8, 0.5, 2.0, 10.0, 2)
    x0 = ref.draw(64, 1).float()
    out = sample(pot, flow=None, strategy='hmc', n_iterations=5, n_chains=64, show_progress=False, seed=1,
                 x0=x0.reshape(64, 2, 4), kernel_kwargs={'step_size': 0.2 / math.sqrt(_lmax(ref, x0)),
                                                         'n_leapfrog_steps': 3})
    assert out.samples.shape[-2:] == (2, 4)
    assert torch.isfinite(out.samples).all() and out.statistics.n_attempted_trajectories == 64 * 5


# ------------------------------------------------------------------------- 7. statistics of long fused runs
def _check_moments(kept, ref, what, slack=0.02):
    """kept (m, n, d): per-chain time averages (independent chains) give honest standard errors.
      mean      |E[x] - m_j| < 5 SE_j + slack sd_j
      variance  |V - v_j| < 5 SE_j + 2 slack v_j"""
    mean, var = ref.block2_moments()
    per_chain = kept.mean(0)
    n = kept.shape[1]
    m = per_chain.mean(0)
    se = per_chain.std(0) / math.sqrt(n)
    print(what, 'mean', m.tolist(), 'se', se.tolist())
    assert bool(((m - mean).abs() < 5 * se + slack * var.sqrt()).all()), (what, (m - mean).tolist(), se.tolist())
    sq = ((kept - mean) ** 2).mean(0)                   # per-chain second central moments about the true mean
    v = sq.mean(0)
    se2 = sq.std(0) / math.sqrt(n)
    print(what, 'var', v.tolist(), 'want', var.tolist())
    assert bool(((v - var).abs() < 5 * se2 + 2 * slack * var).all()), (what, (v - var).tolist(), se2.tolist())


def test_long_hmc_run_recovers_the_block2_moments(dev, monkeypatch):
    """d = 8 (four bananas), mu = 1, a = 0.5, b = 5, 4096 chains started from exact draws, 200 fused HMC transitions
    (L = 8), every 4th state of the last 160 kept."""
    from nfmc_amd.potentials import Rosenbrock
    d, n, T, L = 8, 4096, 200, 8
    pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=2)
    ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 2)
    x0 = ref.draw(n, 5).float()
    h = 0.2 / math.sqrt(_lmax(ref, x0))
    s = _sampler('hmc', d, pot, T, h, L=L)
    s.seed = 2718
    spy = _Spy(monkeypatch)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    assert 0.5 < acc < 1.0, acc
    kept = out.samples.reshape(T, n, d)[T // 5::4].double()
    _check_moments(kept, ref, 'hmc')
    assert torch.isfinite(out.mean).all()


def test_jump_mala_on_a_fitted_flow_recovers_the_block2_moments(dev, monkeypatch):
    """d = 4, the same bananas; a RealNVP fitted on exact draws proposes the jumps of jump_mala (fused inner loop and
    flow-MH kernel).  The jumps must be accepted at a useful rate (about 10 % for this flow) and the kept states must have
    the target's moments."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.potentials import Rosenbrock
    from nfmc_amd.samplers import jump, mcmc
    d, n, T, Kin = 4, 4096, 40, 4
    pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=2)
    ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 2)
    torch.manual_seed(2)
    f = Flow(RealNVP((d,)))
    f.fit(ref.draw(20000, 3).float(), n_epochs=100, show_progress=False)
    x0 = ref.draw(n, 4).float()
    split = []
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), None,
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.inner_sampler.kernel.step_size = 0.3 * d ** (-1 / 3) / _lmax(ref, x0)
    s.seed = 8
    out = s.sample(x0, show_progress=False)
    assert not spy.calls and not split
    acc = out.statistics.n_accepted_jumps / out.statistics.n_attempted_jumps
    print('jump acceptance', acc)
    assert acc > 0.05, acc
    kept = out.samples.reshape(T * (Kin + 1), n, d)[T:].double()
    _check_moments(kept, ref, 'jump_mala', slack=0.03)


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_proposals_are_rejected_and_counted(dev, kind):
    """Steps far past stability on a block-4 target: proposals reach |x| >~ 1e12, where b x^4 overflows fp32, so U of the
    proposal is inf and the log ratio is not finite.  The adjusted kernels reject every such proposal and count it as
    non-finite (n_nonfinite_log_ratios), as for the existing kinds; the kept states stay finite."""
    from nfmc_amd.potentials import Rosenbrock
    d, n, T = 16, 512, 10
    pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=4)
    ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 4)
    x0 = ref.draw(n, 3).clamp(-5, 5).float()
    h = {'mala': 1e12, 'mh': 0.0, 'hmc': 2.0}[kind]
    s = _sampler(kind, d, pot, T, h, L=3, imd=torch.full((d,), 1e24, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.isfinite(out.mean).all()
    print(kind, 'non-finite', st.n_nonfinite_log_ratios, 'accepted', st.n_accepted_trajectories)
    assert st.n_nonfinite_log_ratios > n * T // 2
    assert st.n_accepted_trajectories + st.n_nonfinite_log_ratios <= n * T
