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

Flow-proposal cases (sections 3, 4 and 4b): from d = 25 on a flow centred by a Laplace fit (H.flow_inputs).  The fp64
oracle alone accepts 0.024 to 0.222 of the jumps and 0.001 to 0.308 of the IMH proposals of sections 3 and 4 (the low ends
are the shapes under d = 25, on a flow about the origin), and in the matrix 0.073 to 0.828 up to capacity 128 and 0.026 to
0.359 above; at most 3.1 % of the chains of a case are within MARGIN of a tie.  The cases under d = 25 and from d = 50
(the matrix from capacity 128) have fp64 log ratios down to -190 and set skip_below_minus_50; the others keep every log
ratio above -50.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from irt_fp64 import IRTFast64, IRTU64, model_u64, prior_draws, start_states
from target_harness import Record as _Record, Spy as _Spy, flow_pair as _flow_pair

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
        self.name = 'S=%d Q=%d' % (S, Q)

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


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
# finite fp64 log ratios above -50 only: H.compare_decisions says why
_compare_decisions = functools.partial(H.compare_decisions, skip_below_minus_50=True)


def _sampler(kind, p, T, L=5, target=None, h=None, imd=None):
    """every kind with the problem's mass diagonal of that kind"""
    return H.mcmc_sampler(kind, p.d, p.pot if target is None else target, T, p.step(kind) if h is None else h, L,
                          p.imd(kind) if imd is None else imd, imd_kinds=H.KINDS)


def _oracle(kind, p, T, noise, L=5):
    exercised = p.d <= 501      # the decisions are exercised
    tr = H.oracle_trace(kind, p.x0, p.target, T, p.step(kind), noise, L, p.imd(kind).float().double(), imd_kinds=H.KINDS,
                        label='%s d=%d' % (kind, p.d) if exercised else None)
    if kind in ('mala', 'mh', 'hmc') and exercised:
        acc = tr.n_accepted / (p.x0.shape[0] * T)
        assert acc < 0.995, (kind, p.d, acc)
    return tr


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
# (S, Q): every default layout (tests/test_host_irt.py asks the library's choose_cfg for each), then the one-question and
# the one-student edge
GRID =[(1, 1), (2, 2), (5, 3), (16, 8), (30, 20), (60, 40), (200, 54), (300, 100), (700, 322), (23, 1), (1, 23)]


def _against_oracle(check, monkeypatch, kind, p, T, L=5, **kw):
    check(monkeypatch, p, kind, T, _sampler(kind, p, T, L=L), lambda noise: _oracle(kind, p, T, noise, L=L), compare=_compare,
          decisions=_compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('S,Q', GRID)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, S, Q):
    p = _problem(S, Q, 96)
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 4, L=2 if p.d == 1023 else 5, torch_seed=p.d,
                    what='%s S=%d Q=%d' % (kind, S, Q))


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
    p = _problem(S, Q, 96)
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, p, 4, seed=777 + p.d, what='native %s S=%d Q=%d' % (kind, S, Q))


# ------------------------------------------------------------------------- 3. jump_mala
@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('S,Q', [(5, 3), (16, 8), (30, 20)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, S, Q):
    n, T = 192, 3
    p = _problem(S, Q, n)
    q, flows = H.flow_inputs(p, p.d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=p.step('mala'), imd=p.imd('mala').float(),
                               fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=not 25 <= p.d < 50, flows=flows)


# ------------------------------------------------------------------------- 4. imh on the sequential flow-MH kernel
@pytest.mark.parametrize('S,Q,spline', [(1, 1, False), (16, 8, False), (60, 40, False), (5, 3, True), (30, 20, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, S, Q, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 9."""
    p = _problem(S, Q, 192)
    q, flows = H.flow_inputs(p, p.d, 192, 3 if spline else 9, spline=spline)
    H.imh_matches_oracle(monkeypatch, q, T=5, seed=4711 + p.d, flow_seed=3 if spline else 9, spline=spline, compare=_compare,
                         what='%s imh S=%d Q=%d' % ('c-rqnsf' if spline else 'realnvp', S, Q), margin=MARGIN,
                         skip_below_minus_50=not 25 <= p.d < 50, flows=flows)


# ------------------------------------------------------------------------- 4b. the flow-MH matrix
FLOW_SQ = {4: (1, 1), 8: (3, 3), 16: (8, 4), 32: (16, 8), 64: (30, 19), 128: (60, 39), 256: (150, 49), 512: (200, 99)}   # d = S + Q + 1
FLOW_CASES = H.flow_cases({cap: S + Q + 1 for cap, (S, Q) in FLOW_SQ.items()})
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh); the inner kernels with the problem's mass diagonals"""
    p = _problem(*FLOW_SQ[case.cap], 96)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL, h_mala=p.step('mala'),
                    h_hmc=p.step('hmc'), imd=lambda kind: p.imd(kind).float(), refused=H.flow_case_id(case) in FLOW_REFUSED,
                    skip_caps=(128, 256, 512))    # from d = 100: fp64 log ratios down to -190


# ------------------------------------------------------------------------- 5. fused equals split
@pytest.mark.parametrize('kind,S,Q', [('mala', 30, 20), ('hmc', 5, 3), ('mh', 16, 8), ('hmc', 60, 40)])
def test_fused_equals_split(dev, monkeypatch, kind, S, Q):
    T = 4
    p = _problem(S, Q, 96)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, p, T, target=target), T, seed=2024, atol=ATOL, rtol=RTOL,
                         share=0.95)


# ------------------------------------------------------------------------- 6. NeuTra gradient (VALU kernels)
@pytest.mark.parametrize('S,Q,nh', [(1, 1, 4), (2, 2, 8), (5, 3, 16), (16, 8, 32), (30, 20, 8), (60, 40, 16)])
def test_neutra_gradient_matches_fp64_autograd(dev, S, Q, nh):
    """Against fp64 autograd through oracle/flow.py and IRTU64's loops, at the starts.  Tolerance: relative 2e-4 of
    (1 + max |.|) per row."""
    p = _problem(S, Q, 96)
    H.neutra_gradient_matches_autograd(dev, p.pot, IRTU64(p.pot.responses, p.pot.observed), p.x0, nh,
                                       'S=%d Q=%d H=%d' % (S, Q, nh), flow_seed=3, bound=2e-4)


# ------------------------------------------------------------------------- 7. NeuTra trajectories, wide conditioner
@pytest.mark.parametrize('S,Q,nh', [(5, 3, 8), (30, 20, 16)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, S, Q, nh):
    p = _problem(S, Q, 96)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(p.d, 9, n_hidden=nh), T=3, L=4,
                                      h=0.2 / math.sqrt(float(p.H.max())), seed=12, atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    p = _problem(30, 20, 96)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(p.d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(float(p.H.max())),
                                       seed=12, atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 8. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,S,Q,n,W,every', [('mala', 16, 8, 140, 12, 1), ('hmc', 16, 8, 150, 16, 2),
                                                ('mala', 60, 40, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, S, Q, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds."""
    p = _problem(S, Q, n)
    d, lm = p.d, float(p.H.max())
    h0 = 0.3 * (0.5 * d ** (-1 / 4) / math.sqrt(lm) if kind == 'hmc' else 0.5 * d ** (-1 / 3) / lm)
    H.warmup_matches_controller(monkeypatch, p, kind, W=W, T=6, L=4, every=every, h0=h0, imd0=torch.ones(d), seed=4242 + d,
                                what='irt %s d=%d n=%d every=%d' % (kind, d, n, every), ties=0.05)


# ------------------------------------------------------------------------- 9. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    p = _problem(30, 20, 256)
    pd = p.pot.descriptor(dev)
    assert pd.kind == hip.POT_ITEM_RESPONSE == 9 and pd.n_components == 30
    assert pd.a % 16 == 0 and p.pot.descriptor(dev).a == pd.a and p.pot.descriptor(dev).b == pd.b   # cached per device
    H.refusing_entry_points(dev, p.pot, p.x0, functools.partial(_flow_pair, p.d))


def test_the_fit_step_refuses_kind_9(dev):
    p = _problem(16, 8, 96)
    H.fit_step_refuses(dev, p.pot, p.x0, _flow_pair(p.d)[0])


def test_philox7_and_bad_descriptors_are_refused(dev):
    """check_irt's codes: a NULL a or b, S = 0, S < 0 and S = d - 1 are EINVAL, a misaligned a is EALIGN."""
    from nfmc_amd import hip
    p = _problem(16, 8, 128)
    d = p.d
    bad = [('a', 0, hip.EINVAL), ('b', 0, hip.EINVAL), ('n_components', 0, hip.EINVAL), ('n_components', -1, hip.EINVAL),
           ('n_components', d - 1, hip.EINVAL), ('n_components', d, hip.EINVAL), ('a', 'misaligned', hip.EALIGN)]
    ok = [('n_components', d - 2)]                                                       # S = d - 2, Q = 1: well formed
    H.bad_descriptors_are_refused(dev, p.pot, p.x0, _flow_pair(d)[0], bad, ok=ok)


def test_limits_are_unchanged(dev):
    H.limits_are_unchanged()


# ------------------------------------------------------------------------- 10. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    T = 8
    p = _problem(13, 7, 300)
    H.determinism_and_sharding(lambda: _sampler(kind, p, T), p.x0, T, p.d, seed=7, world=2)


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
    s = H.warmup_sampler('mala', d, p.pot, W, SCORE_B, 0.3 * d ** (-1 / 3))
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
