"""GPU: LatentGMRF (NFMC_POT_LATENT_GMRF) on the fused HIP kernels against the fp64 CPU oracle, with the target restated
in fp64 from a dense structure matrix (tests/gmrf_fp64.py).  Section by section the latent Gaussian model's file
(tests/test_gpu_latent_gaussian.py), plus the dense cross-check and the known answers this kind needs.

Problem (gmrf_fp64.problem_data): n sites on the ring j ~ j + 1 with the chord (j, (7 j + 3) mod n) for every j divisible
by 3 (W reaches 11 at n = 63; the neighbours sit in other quads, lanes and wave halves, rows have different fill),
R = Laplacian + 0.5 I, m = 1 for Poisson and 0 otherwise, the generating field m + L^-T eps with R = L L^T and s* = 0;
weights, observations and the 20 % unobserved sites as in the latent Gaussian model's file; tau ~ Gamma(2, 2).  The
intrinsic cases are `icar` on the same graph (R = D - A, rank n - 1).  The lattice cases are R = (0.5 I + G)^2 on an
(H, W) grid, the 13-point stencil.  Starts are the generating state + 0.3 eps, rounded to fp32.

Step sizes, lambda = the largest autograd-Hessian lambda_max over the generating state and the first 8 starts
(gmrf_fp64.step_lambda): mala 1.5 d^(-1/3) / lambda, ula 0.1 d^(-1/3) / lambda, mh proposal scale 0.5 / sqrt(d lambda),
hmc c d^(-1/4) / sqrt(lambda) with L = 5 and c = 1 for fixed tau, 0.5 for unknown tau, 0.25 for the scaled form at
d < 8; uhmc 0.3 times the hmc rule.

Tolerances are the full-rank file's: MARGIN 2e-3, ATOL 1e-3 + RTOL 1e-4, and the harness's 10 % cap on near-ties.
With these inputs the fp64 oracle alone (96 chains, 4 transitions; mala, hmc and mh; the replay grid, all nine
(likelihood, mode) pairs at d = 25 and 130, the intrinsic cases, the three lattices) puts at most 3.1 % of the chains of a
run within 2e-3 of a tie, accepts 0.62 to 1.0 of the proposals and keeps every log ratio finite.  The intrinsic cases,
probed with the same rule: at most 3.1 % near-ties, acceptance 0.91 to 1.0.

The grid covers every default (CPL, LPC) layout: (16, 64) by the 32 x 32 lattice (tests/test_host_gmrf.py).

Flow-proposal cases (section 3 and 3b).  On a flow about the origin the fp64 oracle alone accepted none of 1536 IMH
proposals at d = 25, 64 and 256, so from d = 25 they run on a flow centred by a Laplace fit (H.flow_inputs).  With the
present inputs the oracle alone accepts 163, 422, 345 and 372 of 1536 IMH proposals at d = 2, 25, 64 and 256 (0.106 to
0.275) and 0.076 to 0.142 of the jumps of section 3, and in the matrix 0.214 to 0.701 up to capacity 128 and 0.135 to
0.333 above; at most 1.0 % of the chains of a case are within MARGIN of a tie.  With tau unknown some proposals are
hopeless (fp64 log ratios down to -1870): those cases set skip_below_minus_50; the others keep every log ratio above -50.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from gmrf_fp64 import COMBOS, lattice_structure, make_pair, n_of, problem_data, starts, step_lambda
from target_harness import Spy as _Spy, flow_pair as _flow_pair

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4
KAPPA2 = 0.5                           # of the lattice cases


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _data(n, lik, seed, lattice):
    return problem_data(n, lik, seed, None if lattice is None else lattice_structure(lattice[0], lattice[1], KAPPA2, 2))


class _Built:
    """What the harness takes (pot, ref, target, x0, d, name) with the problem's data, mode and lambda."""

    def __init__(self, d, lik, mode, seed, n, x0_seed, event_shape, intrinsic, lattice):
        self.data = _data(n_of(d, mode), lik, seed, lattice)
        self.pot, self.ref = make_pair(self.data, mode, event_shape, intrinsic)
        self.target = self.ref
        self.x0 = starts(self.data, self.ref, n, x0_seed)
        self.d, self.mode = d, mode
        self.name = '%s %s%s d=%d' % (lik, mode, ' icar' if intrinsic else '', d)
        self.lam = step_lambda(self.data, self.ref, self.x0)


@functools.lru_cache(maxsize=None)
def _Problem(d, lik, mode, seed, n, x0_seed, event_shape=None, intrinsic=False, lattice=None):
    """One object per distinct problem, shared by the tests that use it and left unchanged."""
    return _Built(d, lik, mode, seed, n, x0_seed, event_shape, intrinsic, lattice)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(p):
    return torch.full((p.d,), 0.5 / math.sqrt(p.d * p.lam), dtype=torch.float64)


def _hmc_factor(p):
    if p.mode == 'fixed':
        return 1.0
    return 0.25 if p.mode == 'scaled' and p.d < 8 else 0.5


def _step(kind, p):
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 1.0, 'uhmc': 0.3}[kind] * _hmc_factor(p) * p.d ** (-1 / 4) / math.sqrt(p.lam)
    return {'mala': 1.5, 'ula': 0.1, 'mh': 0.0}[kind] * p.d ** (-1 / 3) / p.lam


KINDS = list(H.KINDS)
DIMS = [1, 2, 3, 8, 25, 64, 130, 256, 512]


def _combo_of(d):
    """(likelihood, mode) rotating with d over the nine combinations; d = 1 is the first, (poisson, fixed): the unknown-tau
    forms need d >= 2"""
    return COMBOS[DIMS.index(d) % len(COMBOS)] if d in DIMS else COMBOS[(3 * d) % len(COMBOS)]


def _against_oracle(check, monkeypatch, kind, p, T, event_shape=None, decisions=H.compare_decisions, **kw):
    h, imd = _step(kind, p), _mh_scale(p)
    shape = p.d if event_shape is None else event_shape
    check(monkeypatch, p, kind, T, _sampler(kind, shape, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd, label=p.name), compare=_compare,
          decisions=decisions, **({} if event_shape is None else {'event_shape': event_shape}), **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', DIMS)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d):
    lik, mode = _combo_of(d)
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, lik, mode, 10 * d + 1, 96, d + 2), 4, torch_seed=d,
                    what='%s %s %s d=%d' % (kind, lik, mode, d))


@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_the_32_x_32_lattice(dev, monkeypatch, kind):
    """d = 1024, W = 13: the layout (16, 64), four register quads per lane, 32 chains x 2 transitions."""
    p = _Problem(1024, 'poisson', 'fixed', 5, 32, 7, lattice=(32, 32))
    assert p.pot.width == 13
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 2, torch_seed=1024, what='%s 32 x 32 lattice' % kind)


@pytest.mark.parametrize('kind,lik,shape', [('mala', 'poisson', (5, 5)), ('hmc', 'student_t', (8, 8))])
def test_two_dimensional_event_shape(dev, monkeypatch, kind, lik, shape):
    """An (H, W) lattice through event_shape=: the kernels see the flattened d = H W."""
    d = shape[0] * shape[1]
    p = _Problem(d, lik, 'fixed', 77, 96, 5, event_shape=shape, lattice=shape)
    assert p.pot.event_shape == shape and p.pot.width == 13
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 4, event_shape=shape, torch_seed=d,
                    what='%s %s %s' % (kind, shape, lik))


# ------------------------------------------------------------------------- 2. every (likelihood, mode) pair; the intrinsic form
@pytest.mark.parametrize('lik,mode', COMBOS)
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
@pytest.mark.parametrize('d', [25, 130])
def test_every_likelihood_and_mode(dev, monkeypatch, kind, d, lik, mode):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, lik, mode, 10 * d + 1, 96, d + 2), 4, torch_seed=d,
                    what='%s %s %s d=%d' % (kind, lik, mode, d))


@pytest.mark.parametrize('mode', ['centered', 'scaled'])
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
@pytest.mark.parametrize('d', [25, 64])
def test_intrinsic_icar_with_unknown_precision(dev, monkeypatch, kind, d, mode):
    """R = D - A on the same graph, rank n - 1: the header's rho / 2 and (n - rho) / 2 are not n / 2 and 0."""
    lik = 'poisson' if d == 25 else 'binomial'
    p = _Problem(d, lik, mode, 10 * d + 1, 96, d + 2, intrinsic=True)
    assert p.pot.rank == d - 2
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 4, torch_seed=d, what='%s icar %s %s d=%d' % (kind, lik, mode, d))


# ------------------------------------------------------------------------- 3. native Philox streams, jump, imh
@pytest.mark.parametrize('kind,d,lik,mode', [('mala', 25, 'binomial', 'scaled'), ('ula', 8, 'poisson', 'centered'),
                                             ('mh', 130, 'student_t', 'fixed'), ('hmc', 64, 'binomial', 'centered'),
                                             ('uhmc', 3, 'poisson', 'scaled'), ('hmc', 512, 'student_t', 'scaled')])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, lik, mode):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, _Problem(d, lik, mode, 7 * d + 3, 160, d), 5,
                    seed=777 + d, what='native %s d=%d' % (kind, d))


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d', [5, 25, 64])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d):
    n, T = 192, 3
    p = _Problem(d, 'binomial', 'fixed' if d == 25 else 'scaled', 3 * d + 5, n, 3)
    q, flows = H.flow_inputs(p, d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3) / p.lam, imd=None,
                               fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=d != 25, flows=flows)   # unknown tau: FLOW_SKIP_CAPS


@pytest.mark.parametrize('d', [2, 25, 64, 256])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d):
    mode = {2: 'scaled', 25: 'fixed', 64: 'centered', 256: 'scaled'}[d]
    p = _Problem(d, 'binomial', mode, 5 * d + 7, 256, 9)
    q, flows = H.flow_inputs(p, d, 256, 9)
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=9, spline=False, compare=_compare,
                         what='imh %s d=%d' % (mode, d), margin=MARGIN, skip_below_minus_50=mode != 'fixed', flows=flows)


# ------------------------------------------------------------------------- 3b. the flow-MH matrix
FLOW_CASES = H.flow_cases()
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}


# unknown tau at these capacities: a proposal's log precision can be far off, with fp64 log ratios down to -390
FLOW_SKIP_CAPS = (64, 256, 512)


def _flow_problem(c):
    """(likelihood, mode) rotating with the capacity; never the Poisson / scaled pair (e^f of a proposal overflows).
    _Problem keeps one object per distinct problem (lru_cache), and H.laplace_fit one fit per object."""
    lik, mode = [('binomial', 'scaled'), ('student_t', 'fixed'), ('poisson', 'centered'), ('binomial', 'centered'),
                 ('student_t', 'scaled'), ('poisson', 'fixed')][int(math.log2(c.cap)) % 6]
    return _Problem(c.d, lik, mode, 5 * c.d + 7, 96, 9)


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh)"""
    p = _flow_problem(case)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=0.3 * case.d ** (-1 / 3) / p.lam, h_hmc=0.5 * _hmc_factor(p) * case.d ** (-1 / 4) / math.sqrt(p.lam),
                    refused=H.flow_case_id(case) in FLOW_REFUSED, skip_caps=FLOW_SKIP_CAPS)


@pytest.mark.parametrize('cap', [64, 128, 256])
def test_flowb_override_launches_what_more_than_4096_chains_get(dev, monkeypatch, cap):
    """a staged kind (its ELL block sits behind the flow image)"""
    d = H.FLOW_DIMS[cap]
    p = _Problem(d, 'binomial', 'centered', 5 * d + 7, 96, 9)
    f, _of = H.centred_flow_pair(p, 5, 8, scale=0.2 if d < 200 else 0.05)
    H.flowb_override_equals_production(dev, monkeypatch, H.centred(p, 4160, 6), f, lpc=cap // 8, T=3, seed=99)


# ------------------------------------------------------------------------- 4. fused equals split
@pytest.mark.parametrize('kind,d,lik,mode', [('mala', 25, 'poisson', 'scaled'), ('hmc', 9, 'student_t', 'centered'),
                                             ('mh', 64, 'binomial', 'fixed')])
def test_fused_equals_split(dev, monkeypatch, kind, d, lik, mode):
    T = 6
    p = _Problem(d, lik, mode, 17 * d, 200, 17)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, d, target, T, _step(kind, p), imd=_mh_scale(p)), T,
                         seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 5. NeuTra (VALU kernels)
@pytest.mark.parametrize('mode', ['fixed', 'centered', 'scaled'])
@pytest.mark.parametrize('d,nh', [(2, 4), (3, 8), (8, 16), (25, 32), (64, 8), (64, 32), (128, 16), (130, 8), (256, 4)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh, mode):
    """On a perturbed RealNVP (couplings need d >= 2); the likelihood rotates with the shape.  d = 64 / 128 are the
    shapes the matrix-core kernels would take for the other kinds.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    lik = ('poisson', 'binomial', 'student_t')[(d + nh) % 3]
    p = _Problem(d, lik, mode, 11 * d + nh, 130, d)
    H.neutra_gradient_matches_autograd(dev, p.pot, p.ref, p.x0, nh, '%s %s d=%d H=%d' % (lik, mode, d, nh), flow_seed=3,
                                       bound=2e-4)


@pytest.mark.parametrize('d,nh,lik,mode', [(8, 8, 'poisson', 'scaled'), (64, 16, 'binomial', 'centered'),
                                           (128, 8, 'student_t', 'fixed')])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh, lik, mode):
    p = _Problem(d, lik, mode, 13 * d, 96, 61)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(p.lam),
                                      seed=12, atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 64
    p = _Problem(d, 'binomial', 'scaled', 29, 96, 62)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(p.lam), seed=12,
                                       atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 6. refused entry points, bad descriptors
@pytest.mark.parametrize('mode', ['fixed', 'centered', 'scaled'])
def test_refusing_entry_points_answer_unsupported(dev, mode):
    from nfmc_amd import hip
    d = 64
    p = _Problem(d, 'poisson', mode, 4, 256, 4)
    pd = p.pot.descriptor(dev)
    assert pd.kind == hip.POT_LATENT_GMRF and pd.n_components == p.pot.width
    assert pd.a_scalar == {'fixed': 0.0, 'centered': 4.0, 'scaled': 12.0}[mode]
    H.refusing_entry_points(dev, p.pot, p.x0, functools.partial(_flow_pair, d))
    H.fit_step_refuses(dev, p.pot, p.x0, _flow_pair(d)[0])


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL ELL block or table, W < 1 and an invalid code are argument errors; a misaligned block or table is an
    alignment error; W > 32 is a well-formed request no kernel runs."""
    from nfmc_amd import hip
    d = 25
    p = _Problem(d, 'student_t', 'scaled', 8, 128, 8)
    b = p.pot.descriptor(dev).b
    bad = [('a', 0, hip.EINVAL), ('b', 0, hip.EINVAL), ('a', 'misaligned', hip.EALIGN), ('b', b + 4, hip.EALIGN),
           ('b', b + 8, hip.EALIGN), ('n_components', 0, hip.EINVAL), ('n_components', -3, hip.EINVAL),
           ('n_components', 33, hip.EUNSUPPORTED), ('a_scalar', 3.0, hip.EINVAL), ('a_scalar', 7.0, hip.EINVAL),
           ('a_scalar', 8.0, hip.EINVAL), ('a_scalar', 10.0, hip.EINVAL), ('a_scalar', 15.0, hip.EINVAL),
           ('a_scalar', 16.0, hip.EINVAL), ('a_scalar', 4.5, hip.EINVAL), ('a_scalar', -1.0, hip.EINVAL)]
    ok = [('a_scalar', float(c)) for c in (0, 1, 2, 4, 5, 6, 12, 13, 14)] + [('n_components', 32), ('n_components', 1)]
    H.bad_descriptors_are_refused(dev, p.pot, p.x0, _flow_pair(d)[0], bad, ok)


# ------------------------------------------------------------------------- 7. determinism and sharding, overflow
@pytest.mark.parametrize('kind,lik,mode', [('mala', 'poisson', 'scaled'), ('hmc', 'binomial', 'centered')])
def test_determinism_and_sharding(dev, kind, lik, mode):
    d, T = 20, 8
    p = _Problem(d, lik, mode, 44, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, p)), p.x0, T, d, seed=7, world=2)


def test_overflowing_poisson_rates_are_rejected_and_the_state_stays_finite(dev, monkeypatch):
    """d = 8, Poisson, fixed tau, random-walk proposals of scale 40: many proposals have f > 89, where e^f overflows fp32
    and U = inf.  Every kept state is finite; every proposal whose fp64 log ratio is below -50 or non-finite is rejected
    by the kernel; the others are compared as everywhere.  In fp64 every proposal of these inputs is below -50 (a step
    of scale 40 in 8 coordinates), so the kernel must reject them all."""
    d, n, T = 8, 96, 4
    p = _Problem(d, 'poisson', 'fixed', 81, n, 10)
    imd = torch.full((d,), 40.0, dtype=torch.float64)
    s = _sampler('mh', d, p.pot, T, 0.0, imd=imd)
    out, tr, rec, spy = H.replay_run(monkeypatch, s, lambda noise: _oracle('mh', p.x0, p.target, T, 0.0, noise, imd=imd,
                                                                            label='overflow'), p.x0, 8, True)
    assert not spy.calls
    got = out.samples.reshape(T, n, d)
    assert bool(torch.isfinite(got).all())
    _compare(got, tr, 'overflow')
    got_m, _got_lr = rec.stacked()
    want_lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    hopeless = ~torch.isfinite(want_lr) | (want_lr < -50)
    prop = p.x0.double()[None] + 40.0 * torch.stack([v.reshape(n, d).double() for v in s.replay[0]])
    over = float((prop.amax(2) > 89).float().mean())
    print('overflow: %.0f %% of the proposals hopeless, %.0f %% with some f > 89' % (100 * float(hopeless.float().mean()), 100 * over))
    assert over > 0.05
    assert not bool(got_m[hopeless].any())
    if bool((~hopeless).any()):
        H.compare_decisions(rec, tr, 'mh', p.x0, p.ref, 'overflow', skip_below_minus_50=True)
    else:
        assert not bool(got_m.any())


# ------------------------------------------------------------------------- 8. the dense counterpart
@pytest.mark.parametrize('kind,lik', [('mala', 'poisson'), ('hmc', 'student_t')])
def test_sparse_and_dense_forms_follow_the_same_oracle(dev, monkeypatch, kind, lik):
    """A proper R with fixed tau and its to_dense() counterpart (kind 12, the d x d precision streamed through LDS) under
    the same replayed noise: each matches the oracle, and their kept states agree to the state tolerance."""
    from nfmc_amd import hip
    d, T = 25, 4
    p = _Problem(d, lik, 'fixed', 10 * d + 1, 96, d + 2)
    dense = p.pot.to_dense()
    assert dense.descriptor(dev).kind == hip.POT_LATENT_GAUSSIAN and p.pot.descriptor(dev).kind == hip.POT_LATENT_GMRF
    h = _step(kind, p)
    got, keep = [], []
    for pot in (p.pot, dense):
        out, tr, _rec, spy = H.replay_run(monkeypatch, _sampler(kind, d, pot, T, h),
                                          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise), p.x0, d, False)
        assert not spy.calls
        got.append(out.samples.reshape(T, p.x0.shape[0], d))
        keep.append(_compare(got[-1], tr, '%s %s' % (kind, type(pot).__name__)))
    both = keep[0] & keep[1]
    torch.testing.assert_close(got[0][:, both], got[1][:, both], atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 9. known answers, long fused runs
def _long_run(monkeypatch, pot, x0, T, L, h, seed):
    """T fused HMC transitions from the starts x0 (n, d) in the object's coordinates: (every 4th state of the second half
    (K, n, d) fp64, acceptance); no split-path call.  The first half is the burn-in: see
    test_both_parameterisations_sample_the_same_posterior."""
    n = x0.shape[0]
    s = _sampler('hmc', pot.event_shape, pot, T, h, L=L)
    s.seed = seed
    spy = _Spy(monkeypatch)
    out = s.sample(x0.float().reshape((n,) + pot.event_shape), show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    return out.samples.reshape(T, n, pot.dim)[T // 2::4].double(), acc


def _nothing_observed(n, seed):
    data = dict(problem_data(n, 'binomial', seed))
    data['observed'] = torch.zeros(n, dtype=torch.bool)
    data['mean'] = torch.linspace(-1.0, 1.0, n, dtype=torch.float64)
    return data


N_LONG, T_LONG, L_LONG = 4096, 200, 8


def test_the_prior_alone_has_the_variances_of_the_inverse_structure(dev, monkeypatch):
    """Every weight 0 and fixed tau: the target is N(m, R^-1) exactly.  n = 9 sites, 4096 chains started from exact draws,
    200 fused HMC transitions (L = 8), the first half discarded.  The mean over the chains of each chain's time average
    of (x_j - m_j)^2 against diag(R^-1) from an fp64 inverse, within 5 standard errors taken from the spread across the
    chains (the chains are independent).  The starts are exact draws because a fixed trajectory length does not burn a
    Gaussian in: a mode of R whose phase sqrt(lambda_k) h L is near pi is mapped to -x whatever the momentum, so its
    variance keeps its starting value.  The fp64 oracle alone from starts m + 0.3 eps still has 0.96 to 0.985 of the
    variances over transitions 100 to 200 (z down to -8.6); from exact draws a kernel with a wrong stationary law
    drifts in every other mode."""
    n = 9
    data = _nothing_observed(n, 12)
    pot, ref = make_pair(data, 'fixed')
    cov = torch.linalg.inv(data['R'])
    g = torch.Generator().manual_seed(3)
    x0 = data['mean'] + torch.randn(N_LONG, n, generator=g, dtype=torch.float64) @ torch.linalg.cholesky(cov).t()
    h = n ** (-1 / 4) / math.sqrt(step_lambda(data, ref, x0.float()))
    kept, acc = _long_run(monkeypatch, pot, x0, T_LONG, L_LONG, h, 2718)
    per_chain = ((kept - data['mean']) ** 2).mean(0)
    est, se = per_chain.mean(0), per_chain.std(0) / math.sqrt(N_LONG)
    z = (est - torch.diagonal(cov)) / se
    print('acceptance %.3f, worst |z| %.2f' % (acc, float(z.abs().max())))
    assert 0.5 < acc <= 1.0, acc
    assert bool((z.abs() < 5).all()), z.tolist()


def test_the_precision_alone_has_the_mean_of_its_log_gamma_prior(dev, monkeypatch):
    """Unknown tau, centred, nothing observed, a proper R: x integrates out to a constant, so tau ~ Gamma(a, b) and
    E[s] = psi(a) - log b = -0.2704 exactly.  Chains start away from that law, at f = m + 0.3 eps and s = 0.3 eps (the
    spread of the centred-against-scaled test), and the first half is discarded; 5 standard errors from the spread of the
    per-chain time averages.  The fp64 oracle alone on these inputs has the mean of s at 0.01 over the first 10
    transitions, -0.262 over 70 to 100 and -0.276 / -0.272 over 100 to 150 / 150 to 200, with its sd grown from 0.3 to
    0.80 (exact 0.80): burnt in by the half; z = -0.52, acceptance 0.98."""
    n = 9
    a, b = 2.0, 2.0
    data = _nothing_observed(n, 13)
    pot, ref = make_pair(data, 'centered')
    g = torch.Generator().manual_seed(4)
    f0 = data['mean'] + 0.3 * torch.randn(N_LONG, n, generator=g, dtype=torch.float64)
    x0 = pot.coordinates(f0, tau=torch.exp(0.3 * torch.randn(N_LONG, generator=g, dtype=torch.float64)))
    h = (n + 1) ** (-1 / 4) / math.sqrt(step_lambda(data, ref, x0.float()))
    kept, acc = _long_run(monkeypatch, pot, x0, T_LONG, L_LONG, h, 314)
    per_chain = kept[:, :, n].mean(0)
    want = float(torch.digamma(torch.tensor(a, dtype=torch.float64))) - math.log(b)
    est, se = float(per_chain.mean()), float(per_chain.std() / math.sqrt(N_LONG))
    print('acceptance %.3f, E[s] %.5f exact %.5f se %.5f' % (acc, est, want, se))
    assert 0.3 < acc <= 1.0, acc
    assert abs(est - want) < 5 * se, (est, want, se)


def test_both_parameterisations_sample_the_same_posterior(dev, monkeypatch):
    """d = 9 (8 observed Poisson sites and s), 4096 chains, 200 fused HMC transitions (L = 8), once per parameterisation
    from the same (f, tau) starts.  The posterior means of f and of s agree within 5 combined standard errors (from the
    per-chain time averages).  Step d^(-1/4) / sqrt(lambda), the latent Gaussian model's rule, and the first half
    discarded: the starts have s = 0 +- 0.3 where the posterior mean of s is -0.94, and the fp64 oracle alone on these
    inputs shows the mean of s still drifting at transition 80 with half that step (worst |z| 4.99 when a fifth is
    discarded) and settled by transition 40 with this one (worst |z| 0.87 with the first half discarded, acceptance
    0.99 centred and 0.94 scaled)."""
    n = 8
    data = problem_data(n, 'poisson', 21)
    g = torch.Generator().manual_seed(5)
    f0 = data['f_star'] + 0.3 * torch.randn(N_LONG, n, generator=g, dtype=torch.float64)
    tau0 = torch.exp(0.3 * torch.randn(N_LONG, generator=g, dtype=torch.float64))
    means, ses = [], []
    for mode in ('centered', 'scaled'):
        pot, ref = make_pair(data, mode)
        x0 = pot.coordinates(f0, tau=tau0)
        h = (n + 1) ** (-1 / 4) / math.sqrt(step_lambda(data, ref, x0.float()))
        kept, acc = _long_run(monkeypatch, pot, x0, T_LONG, L_LONG, h, 2718)
        print('%s: acceptance %.3f' % (mode, acc))
        assert 0.3 < acc <= 1.0, (mode, acc)
        per_chain = torch.cat([pot.latent(kept), kept[..., n:]], dim=-1).mean(0)
        means.append(per_chain.mean(0))
        ses.append(per_chain.std(0) / math.sqrt(N_LONG))
    z = (means[0] - means[1]) / torch.sqrt(ses[0] ** 2 + ses[1] ** 2)
    print('worst |z| %.2f' % float(z.abs().max()))
    assert bool((z.abs() < 5).all()), z.tolist()
