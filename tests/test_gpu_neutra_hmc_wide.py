"""The two matrix-core NeuTra-HMC trajectory kernels behind nfmc_neutra_hmc_steps_f32, row by row against the fp64 oracle

    oracle.samplers.mcmc_sample(z0.double(), neutra_adjusted_target(of, target, (d,)), 'hmc', T, h, imd, L,
                                noise=PhiloxNoise(seed, chain_offset, dtype=torch.float64), step0=step0)

  'mfma'  neutra_leapfrog_mfma_kernel (csrc/neutra_mfma.hip): d = 64 / 128, conditioner width up to 128 (narrower ones
          zero-padded to 64 by NeuTra._min_hidden), 1 or 2 hidden layers: template instances TD 4 / 8 x TH 4 / 8 x NHL 1 / 2;
  'wide'  neutra_leapfrog_wide_kernel (csrc/mfma_wide.hip): the other multiples of 32 from 32 to 512 with 32 < H <= 128, the
          state, gradient and momentum streamed through a three-row slab: instances TH 4 / 8 x NHL 1 / 2.

Both are launched once per transition by their host loops (run_hmc, nfmc_neutra_hmc_steps_wide_f32), which also walk the
sample-store cursor and fold the statistics after every transition.  Every case asserts its kernel twice: by
target_harness.neutra_hmc_kernel_of (the documented shape rules) and by the work area nfmc_neutra_scratch_bytes asks for,
which follows another formula for each kernel (target_harness.neutra_hmc_scratch_bytes); the sampler cases also assert
that the split path was not entered.

Inputs.  The flow is the identity perturbed by `scale` (H.centred_flow_pair about (0, 1), flow seed 5), the latent starts
0.5 N(0, I) (seed 1000 d + n).  n = 150 (one full 128-chain tile and 22 chains of the next), T = 4, L = 3 unless a case
says otherwise.  h and scale are chosen per case so that, for the fp64 oracle alone, the acceptance lies in 0.30 .. 0.95,
under 10 % of the chains come within their margin of a tie and every log ratio is finite;
tests/test_host_neutra_hmc_wide.py proves that on the CPU for every oracle-backed run (RUNS).

Tolerances, none taken from the kernels.  FIGURES holds, per oracle-backed run, what the oracle itself loses in fp32: the
same oracle with the flow, the inputs and the noise cast to float32 against the fp64 run (H.neutra_hmc_figures), the worst
difference of a kept state and of a log ratio.  Then
  log ratios: H.compare_decisions' own bound 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp |U~(z)|, raised to 4 x the
    log-ratio figure where that is larger (H.neutra_hmc_row_tolerance);
  near-tie margin: that row tolerance (not 4 x the figure alone: a kernel that is within the tolerance may decide any call
    closer than the tolerance the other way, and the states comparison must not hold such a chain);
  states: atol = 4 x the state figure, plus, on the native streams, 2 T L h max(m) / sqrt(min(m)) NORMAL_TOL for the
    normals: the device draws them with the hardware transcendentals and differs from oracle/philox.py by about 1e-6
    (its docstring; twice that is NORMAL_TOL, and the replay test holds the device's draws to it), both oracles get the
    same fp32 values, so the figure cannot contain it.  A momentum off by e moves the end of L leapfrog steps of a
    quadratic U~ of frequency w by at most L h m e / sqrt(1 - h^2 w^2 / 4) (the leapfrog map of a harmonic oscillator is
    a rotation in a norm that far from the Euclidean one); the root is at least 1 / 2 at every case's h (the stiffest is
    the diagonal target, w^2 = 4 at h = 0.861: 1 / 1.96), hence the 2, and T transitions add up.  A launch on replayed
    oracle normals has no such term: there atol is 4 x the figure alone.
The host file re-measures every figure and fails if the table is off by more than 10 %.

Figures: states 1.8e-7 .. 1.0e-5, log ratios 5.6e-6 .. 1.2e-4; 4 x the log-ratio figure exceeds compare_decisions' bound in
no case (the nearest: the diagonal target at d = 128, 3.8e-4 against 4e-4 and more), so no row is held at a raised
tolerance.  The oracle accepts 0.64 .. 0.80 of the trajectories.

Worst error over tolerance observed on the MI355X, mfma / wide: log ratios 0.152 / 0.189; states 0.196 / 0.351 on the
native streams, 0.481 / 0.574 on replayed oracle normals; the device's normals differ from the oracle's by 4.8e-7 at most.
Mutations on a scratch build: the accept uniform taken from word 0 instead of `step & 3` fails all 29 one-launch cases,
both step-offset, replay, second-tile and sampler cases (37); the replay index without `rev` fails both replay cases."""
import collections
import ctypes as C
import functools

import pytest
import torch

import target_harness as H

pytestmark = pytest.mark.gpu

N, T, L = 150, 4, 3
SEED, FLOW_SEED = 23, 5
CAP = 0.10
NORMAL_TOL = 2e-6                         # twice what oracle/philox.py says the device's normals differ from its own by
BIG = 256 * 128 + 40                      # 257 tiles of 128 chains on 256 workgroup slots: slot 0 takes a second tile
TAIL = 168                                # the last full tile and the 40 chains of the ragged one
STATS_RTOL = 1e-9


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple('Case', 'kernel target d nh hl cl h n mass L scale')


def _case(kernel, target, d, nh, hl, cl, h, *, n=N, mass=False, L=L, scale=0.1):
    return Case(kernel, target, d, nh, hl, cl, h, n, mass, L, scale)


def _id(c):
    return '%s-%s-d%d-h%dx%d-c%d-L%d%s%s' % (c.kernel, c.target, c.d, c.nh, c.hl, c.cl, c.L, '-mass' if c.mass else '',
                                            '' if c.n == N else '-n%d' % c.n)


# kernel, target, d, conditioner width, hidden layers, couplings, h
MFMA = [_case('mfma', 'sumsq', 64, 64, 1, 2, 0.297),                          # TD 4, TH 4, NHL 1
        _case('mfma', 'sumsq', 64, 64, 2, 2, 0.265, mass=True),               # TD 4, TH 4, NHL 2
        _case('mfma', 'sumsq', 64, 128, 1, 3, 0.265, L=4),                    # TD 4, TH 8, NHL 1; `rev`
        _case('mfma', 'sumsq', 64, 128, 2, 1, 0.297, mass=True),              # TD 4, TH 8, NHL 2
        _case('mfma', 'sumsq', 128, 64, 1, 2, 0.221, mass=True),              # TD 8, TH 4, NHL 1
        _case('mfma', 'sumsq', 128, 40, 2, 3, 0.221),                         # TD 8, TH 4, NHL 2; width padded 40 -> 64
        _case('mfma', 'sumsq', 128, 100, 1, 2, 0.311, L=1),                   # TD 8, TH 8, NHL 1; padded 100 -> 128; one leapfrog step
        _case('mfma', 'sumsq', 128, 128, 2, 2, 0.248, mass=True, L=2),        # TD 8, TH 8, NHL 2
        _case('mfma', 'sumsq', 64, 6, 2, 2, 0.265),                           # a narrow conditioner, presented as 64 wide
        _case('mfma', 'funnel', 64, 40, 2, 3, 0.14, mass=True),
        _case('mfma', 'funnel', 128, 128, 1, 2, 0.126),
        _case('mfma', 'quadratic', 64, 100, 1, 1, 0.489, mass=True),
        _case('mfma', 'diagonal', 128, 64, 2, 2, 0.861),
        _case('mfma', 'sumsq', 64, 64, 1, 2, 0.169, n=1),
        _case('mfma', 'sumsq', 128, 100, 2, 3, 0.157, n=1, mass=True)]
WIDE = [_case('wide', 'sumsq', 32, 64, 1, 2, 0.332),                          # TH 4, NHL 1; the smallest d
        _case('wide', 'sumsq', 32, 128, 2, 3, 0.332, mass=True),              # TH 8, NHL 2; `rev`
        _case('wide', 'sumsq', 96, 40, 2, 2, 0.217, L=4),                     # TH 4, NHL 2; padded 40 -> 64; a half of 48 coordinates
        _case('wide', 'sumsq', 96, 100, 1, 1, 0.243, mass=True),              # TH 8, NHL 1; padded 100 -> 128
        _case('wide', 'sumsq', 256, 64, 1, 3, 0.178, mass=True, scale=0.05),
        _case('wide', 'sumsq', 256, 128, 2, 2, 0.28, scale=0.05, L=1),
        _case('wide', 'sumsq', 512, 128, 1, 2, 0.173, mass=True, scale=0.05, L=2),
        _case('wide', 'sumsq', 512, 64, 2, 3, 0.138, scale=0.05),
        _case('wide', 'funnel', 96, 64, 1, 3, 0.135),
        _case('wide', 'funnel', 256, 100, 2, 2, 0.09, mass=True, scale=0.05),
        _case('wide', 'quadratic', 32, 40, 1, 2, 0.524, mass=True),
        _case('wide', 'diagonal', 96, 128, 2, 3, 0.861),
        _case('wide', 'sumsq', 32, 64, 1, 2, 0.15, n=1),
        _case('wide', 'sumsq', 96, 100, 2, 3, 0.217, n=1, mass=True)]
CASES = MFMA + WIDE
BY_ID = {_id(c): c for c in CASES}
assert len(BY_ID) == len(CASES)

# one shape per kernel with an odd coupling count (the reversed latent order) and a mass diagonal
ODD = {'mfma': BY_ID['mfma-funnel-d64-h40x2-c3-L3-mass'], 'wide': BY_ID['wide-sumsq-d32-h128x2-c3-L3-mass']}
EVEN = {'mfma': BY_ID['mfma-sumsq-d64-h64x2-c2-L3-mass'], 'wide': BY_ID['wide-sumsq-d96-h40x2-c2-L4']}
# the second tile of a workgroup: n = BIG
SECOND = {'mfma': _case('mfma', 'sumsq', 64, 64, 1, 2, 0.33, n=BIG, L=2), 'wide': _case('wide', 'sumsq', 32, 64, 1, 2, 0.38, n=BIG, L=2)}
KERNELS = ('mfma', 'wide')


# ------------------------------------------------------------------------------------------------ the oracle-backed runs
# rows [lo, lo + n) of the case's chains, transitions step0 .. step0 + T - 1
Run = collections.namedtuple('Run', 'case tag T step0 adjust lo n')


def _run(c, tag='base', steps=T, step0=0, adjust=True, lo=0, n=None):
    return Run(c, tag, steps, step0, adjust, lo, c.n - lo if n is None else n)


def _key(r):
    return '%s|%s' % (_id(r.case), r.tag)


RUNS = ([_run(c) for c in CASES]
        + [_run(ODD[k], 'unadjusted', adjust=False) for k in KERNELS]
        + [_run(EVEN[k], 'step6', step0=6) for k in KERNELS]
        + [_run(ODD[k], 'six', 6) for k in KERNELS]
        + [_run(SECOND[k], 'head', 2, n=128) for k in KERNELS]
        + [_run(SECOND[k], 'tail', 2, lo=BIG - TAIL, n=TAIL) for k in KERNELS])
RUN_OF = {_key(r): r for r in RUNS}
assert len(RUN_OF) == len(RUNS)

# run -> (state figure, log-ratio figure): the fp32 oracle against the fp64 oracle, CPU alone (H.neutra_hmc_figures);
# tests/test_host_neutra_hmc_wide.py measures them again and holds this table to 10 %
FIGURES = {
    'mfma-sumsq-d64-h64x1-c2-L3|base': (7.01e-07, 1.71e-05),
    'mfma-sumsq-d64-h64x2-c2-L3-mass|base': (6.97e-07, 2.22e-05),
    'mfma-sumsq-d64-h128x1-c3-L4|base': (7.89e-07, 1.60e-05),
    'mfma-sumsq-d64-h128x2-c1-L3-mass|base': (6.37e-07, 1.94e-05),
    'mfma-sumsq-d128-h64x1-c2-L3-mass|base': (6.41e-07, 2.98e-05),
    'mfma-sumsq-d128-h40x2-c3-L3|base': (5.63e-07, 2.94e-05),
    'mfma-sumsq-d128-h100x1-c2-L1|base': (2.19e-07, 2.11e-05),
    'mfma-sumsq-d128-h128x2-c2-L2-mass|base': (5.18e-07, 2.25e-05),
    'mfma-sumsq-d64-h6x2-c2-L3|base': (8.66e-07, 1.55e-05),
    'mfma-funnel-d64-h40x2-c3-L3-mass|base': (1.06e-06, 3.97e-05),
    'mfma-funnel-d128-h128x1-c2-L3|base': (8.54e-07, 6.22e-05),
    'mfma-quadratic-d64-h100x1-c1-L3-mass|base': (1.21e-06, 1.94e-05),
    'mfma-diagonal-d128-h64x2-c2-L3|base': (1.03e-05, 9.47e-05),
    'mfma-sumsq-d64-h64x1-c2-L3-n1|base': (3.31e-07, 1.16e-05),
    'mfma-sumsq-d128-h100x2-c3-L3-mass-n1|base': (3.38e-07, 6.37e-06),
    'wide-sumsq-d32-h64x1-c2-L3|base': (6.56e-07, 8.48e-06),
    'wide-sumsq-d32-h128x2-c3-L3-mass|base': (7.37e-07, 8.08e-06),
    'wide-sumsq-d96-h40x2-c2-L4|base': (6.94e-07, 2.00e-05),
    'wide-sumsq-d96-h100x1-c1-L3-mass|base': (4.62e-07, 2.06e-05),
    'wide-sumsq-d256-h64x1-c3-L3-mass|base': (6.09e-07, 4.92e-05),
    'wide-sumsq-d256-h128x2-c2-L1|base': (2.99e-07, 4.29e-05),
    'wide-sumsq-d512-h128x1-c2-L2-mass|base': (4.37e-07, 1.01e-04),
    'wide-sumsq-d512-h64x2-c3-L3|base': (4.74e-07, 7.41e-05),
    'wide-funnel-d96-h64x1-c3-L3|base': (1.71e-06, 6.64e-05),
    'wide-funnel-d256-h100x2-c2-L3-mass|base': (7.64e-07, 1.17e-04),
    'wide-quadratic-d32-h40x1-c2-L3-mass|base': (1.83e-06, 1.50e-05),
    'wide-diagonal-d96-h128x2-c3-L3|base': (7.15e-06, 7.21e-05),
    'wide-sumsq-d32-h64x1-c2-L3-n1|base': (1.79e-07, 5.64e-06),
    'wide-sumsq-d96-h100x2-c3-L3-mass-n1|base': (4.27e-07, 7.56e-06),
    'mfma-funnel-d64-h40x2-c3-L3-mass|unadjusted': (1.21e-06, 0.00e+00),
    'wide-sumsq-d32-h128x2-c3-L3-mass|unadjusted': (1.00e-06, 0.00e+00),
    'mfma-sumsq-d64-h64x2-c2-L3-mass|step6': (8.24e-07, 1.40e-05),
    'wide-sumsq-d96-h40x2-c2-L4|step6': (7.23e-07, 1.97e-05),
    'mfma-funnel-d64-h40x2-c3-L3-mass|six': (1.15e-06, 3.97e-05),
    'wide-sumsq-d32-h128x2-c3-L3-mass|six': (8.83e-07, 8.83e-06),
    'mfma-sumsq-d64-h64x1-c2-L2-n32808|head': (3.56e-07, 1.67e-05),
    'wide-sumsq-d32-h64x1-c2-L2-n32808|head': (3.72e-07, 8.04e-06),
    'mfma-sumsq-d64-h64x1-c2-L2-n32808|tail': (3.96e-07, 1.37e-05),
    'wide-sumsq-d32-h64x1-c2-L2-n32808|tail': (5.01e-07, 7.03e-06)}


def _problem(target, d, n):
    """the package potential, its fp64 restatement and the latent starts (the forms of tests/test_gpu_flow_mh_wide.py)"""
    from nfmc_amd.potentials import DiagonalGaussian, Funnel, QuadraticPotential, SumOfSquares
    from oracle import potentials as opot
    if target == 'sumsq':
        pot, ref = SumOfSquares((d,)), opot.sum_squares
    elif target == 'funnel':
        pot, ref = Funnel((d,), 3.0), opot.funnel(3.0)
    elif target == 'quadratic':
        pot = QuadraticPotential((d,), torch.linspace(0.5, 2.0, d), torch.linspace(-1.0, 1.0, d))
        ref = opot.quadratic(pot.a, pot.b)
    else:
        pot = DiagonalGaussian((d,), mu=torch.linspace(-2.0, 2.0, d), sigma=torch.linspace(0.5, 1.5, d))
        ref = opot.quadratic(pot.a, pot.b)
    z0 = 0.5 * torch.randn(n, d, generator=torch.Generator().manual_seed(1000 * d + n))
    return H.Problem(pot, ref, ref, z0, d, '%s d=%d' % (target, d))


def _imd(c):
    return torch.linspace(0.8, 1.3, c.d) if c.mass else None


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """(problem at its latent starts, package flow, fp64 oracle flow holding the same fp32 weights); shared, read-only"""
    p = _problem(c.target, c.d, c.n)
    centre = (torch.zeros(c.d, dtype=torch.float64), torch.ones(c.d, dtype=torch.float64))
    f, of = H.centred_flow_pair(p, FLOW_SEED, c.nh, False, c.cl, scale=c.scale, centre=centre, hidden_layers=c.hl)
    return p, f, of


def _rows(r):
    p, f, of = _inputs(r.case)
    return H.with_starts(p, p.x0[r.lo:r.lo + r.n]), f, of


@functools.lru_cache(maxsize=None)
def _oracle(r, dtype=torch.float64):
    q, _f, of = _rows(r)
    c = r.case
    return H.neutra_hmc_oracle(q, of, r.T, c.L, c.h, SEED, adjust=r.adjust, imd=_imd(c), step0=r.step0, chain_offset=r.lo, dtype=dtype)


def measure(r):
    """(state figure, log-ratio figure) of a run, on the CPU"""
    return H.neutra_hmc_figures(_oracle(r), _oracle(r, torch.float32))


def _atol(r, native=True):
    c = r.case
    m = 1.3 / 0.8 ** 0.5 if c.mass else 1.0
    return H.SPLINE_C_FACTOR * FIGURES[_key(r)][0] + (2 * r.T * c.L * c.h * m * NORMAL_TOL if native else 0.0)


def conditions(r):
    """the conditions on a run's inputs, from the fp64 oracle alone; (acceptance, tie share)"""
    q, _f, of = _rows(r)
    tr = _oracle(r)
    if not r.adjust:
        assert bool(torch.isfinite(tr.stacked()).all()), _key(r)
        return 1.0, 0.0
    tol = H.neutra_hmc_row_tolerance(tr, q, of, FIGURES[_key(r)][1])
    return H.neutra_hmc_inputs_ok(tr, _key(r), margin=tol, cap=CAP)


def _assert_kernel(c, run, hidden=None):
    """the kernel a launch took, by the shape rules and by the size of the work area it asked for"""
    assert H.neutra_hmc_kernel_of(c.d, c.nh, c.hl) == c.kernel, _id(c)
    presented = H.neutra_presented_hidden(c.d, c.nh, c.hl)
    n = run.masks.shape[1]
    mine, other = (H.neutra_hmc_scratch_bytes(k, n, c.d, presented, c.hl, c.cl) for k in (c.kernel, 'wide' if c.kernel == 'mfma' else 'mfma'))
    assert run.scratch_bytes == mine and mine != other, (_id(c), run.scratch_bytes, mine, other)


_launches = {}


def _launch(dev, r, **kw):
    """one direct launch of the run's rows on the native streams, with immediate statistics; the plain one is shared"""
    q, f, _of = _rows(r)
    c = r.case
    key = (r, tuple(sorted(kw.items()))) if not any(isinstance(v, (tuple, list)) or callable(v) for v in kw.values()) else None
    if key is not None and key in _launches:
        return _launches[key]
    kw.setdefault('stats', 'immediate')
    out = H._direct_neutra_hmc(dev, q, f, r.T, c.L, c.h, SEED, adjust=r.adjust, imd=_imd(c), step0=r.step0, chain_offset=r.lo, **kw)
    _assert_kernel(c, out)
    if key is not None:
        _launches[key] = out
    return out


def _follow(r, run, native=True):
    """the launch against the run's oracle, row by row; prints and returns the worst ratios"""
    q, _f, of = _rows(r)
    ratios = H.compare_neutra_hmc(run, _oracle(r), q, of, _key(r), atol=_atol(r, native), lr_figure=FIGURES[_key(r)][1], adjust=r.adjust)
    print('%s: worst state error over atol %.3f (atol %.2e), worst log-ratio error over tolerance %.3f' % ((_key(r), ratios[0], _atol(r, native), ratios[1])))
    return ratios


def _check_stats(run, n, steps, what, prefill=(0.0, 0)):
    st = run.stats
    assert st['accepted'] == prefill[1] + int(run.masks.sum()), (what, st['accepted'], int(run.masks.sum()))
    assert st['attempted'] == prefill[1] + n * steps, (what, st['attempted'])
    assert st['nonfinite'] == prefill[1], (what, st['nonfinite'])
    kept = run.samples.double()
    for name, v in (('sum_x', kept), ('sum_x2', kept * kept)):
        want, scale = prefill[0] + v.sum((0, 1)), abs(prefill[0]) + v.abs().sum((0, 1))
        err = (st[name].double() - want).abs()
        print('%s: %s worst error over bound %.3f' % (what, name, float((err / (STATS_RTOL * scale)).max())))
        assert bool((err <= STATS_RTOL * scale).all()), (what, name, float(err.max()))


# ------------------------------------------------------------------------------------------------ one launch
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_one_launch_follows_the_oracle_row_by_row(dev, case):
    """T transitions of one nfmc_neutra_hmc_steps_f32 call: every mask, log ratio and kept state, and the statistics the
    per-transition folds leave (accepted = the kernel's own masks, attempted n T, no non-finite ratio, the sums of the
    kernel's own kept states: fp64 sums of fp32 values, to 1e-9 of their size)."""
    r = _run(case)
    conditions(r)
    run = _launch(dev, r)
    _follow(r, run)
    _check_stats(run, case.n, T, _key(r))


@pytest.mark.parametrize('kernel', KERNELS)
def test_unadjusted_launch_keeps_every_trajectory(dev, kernel):
    """adjust = 0: every mask 1, no log ratio, the kept states the oracle's adjustment=False run, n T accepted."""
    r = _run(ODD[kernel], 'unadjusted', adjust=False)
    conditions(r)
    run = _launch(dev, r)
    _follow(r, run)
    assert bool(run.masks.all()) and run.stats['accepted'] == r.n * T and run.stats['attempted'] == r.n * T and run.stats['nonfinite'] == 0


@pytest.mark.parametrize('kernel', KERNELS)
def test_step_offset_crosses_a_philox_block_of_accept_uniforms(dev, kernel):
    """step0 = 6, T = 4: transitions 6 .. 9 take words 2, 3 of Philox block 1 and words 0, 1 of block 2."""
    r = _run(EVEN[kernel], 'step6', step0=6)
    conditions(r)
    _follow(r, _launch(dev, r))


@pytest.mark.parametrize('kernel', KERNELS)
def test_chain_offset_gives_the_rows_of_the_whole_launch(dev, kernel):
    """rows [75, 150) launched alone with chain_offset = 75: bit for bit those rows of the whole launch."""
    c = EVEN[kernel]
    whole = _launch(dev, _run(c))
    part = _launch(dev, _run(c, 'part', lo=75))
    assert part.masks.shape == (T, 75)
    for name in ('samples', 'masks', 'log_ratios'):
        assert torch.equal(getattr(part, name), getattr(whole, name)[:, 75:]), (_id(c), name)
    assert torch.equal(part.z, whole.z[75:])


@pytest.mark.parametrize('kernel', KERNELS)
def test_replayed_noise_gives_the_native_launch_and_follows_the_oracle(dev, kernel):
    """An odd coupling count (the kernels hold the latent in reversed order and index the replayed normals logically).
    The device's own normals of the noise stream (nfmc_philox_normals_f32) and the oracle's uniforms, which are the
    kernels' exactly, replayed under another seed: the native launch bit for bit.  The oracle's recorded normals differ
    from the device's by about 1e-6 by design (oracle/philox.py; held to NORMAL_TOL here): replayed, that launch is held
    to the oracle row by row, with no allowance for the normals."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    r = _run(ODD[kernel])
    c = r.case
    q, f, of = _rows(r)
    rec = osamp.RecordingNoise(osamp.PhiloxNoise(SEED, dtype=torch.float64))
    tr = H.neutra_hmc_oracle(q, of, T, c.L, c.h, SEED, imd=_imd(c), noise=rec)
    assert torch.equal(tr.stacked(), _oracle(r).stacked())
    recorded, uniforms = torch.stack(rec.normals).float(), torch.stack(rec.uniforms).float()
    base = _launch(dev, r)
    native = torch.empty(T, c.n, c.d, device=dev)
    for s in range(T):
        rng = hip.make_rng(SEED, 0, s)
        hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), hip.TAG_NOISE, c.n, c.d, hip.ptr(native[s]), hip.stream()),
                  'nfmc_philox_normals_f32')
    native = native.cpu()
    worst = float((native - recorded).abs().max())
    print('%s: device normals against the oracle\'s %.2e' % (_id(c), worst))
    assert worst < NORMAL_TOL, _id(c)
    again = H._direct_neutra_hmc(dev, q, f, T, c.L, c.h, SEED + 1, imd=_imd(c), replay=(native, uniforms), stats='immediate')
    for name in ('samples', 'masks', 'log_ratios', 'z'):
        assert torch.equal(getattr(again, name), getattr(base, name)), (_id(c), name)
    assert again.stats['accepted'] == base.stats['accepted'] and torch.equal(again.stats['sum_x'], base.stats['sum_x'])
    _follow(r, H._direct_neutra_hmc(dev, q, f, T, c.L, c.h, SEED + 1, imd=_imd(c), replay=(recorded, uniforms)), native=False)


@pytest.mark.parametrize('kernel', KERNELS)
def test_a_workgroup_takes_a_second_tile(dev, kernel):
    """n = 256 x 128 + 40: 257 tiles on 256 workgroup slots, so workgroup 0 runs tile 0 and then the ragged tile 256 on the
    same checkpoint area (mfma) / slab rows (wide) and adds both to its LDS statistics.  The oracle runs on chains
    [0, 128) and on the last 168 (the last full tile, which shares nothing, and the ragged one) with their chain offsets;
    the totals are held against fp64 sums of the device's own kept states over all chains."""
    c = SECOND[kernel]
    whole = _launch(dev, _run(c, 'whole', 2))
    for r in (_run(c, 'head', 2, n=128), _run(c, 'tail', 2, lo=BIG - TAIL, n=TAIL)):
        conditions(r)
        cut = slice(r.lo, r.lo + r.n)
        part = H.NeutraRun(0, whole.samples[:, cut], whole.masks[:, cut], whole.log_ratios[:, cut], whole.z[cut], None, whole.scratch_bytes)
        _follow(r, part)
    _check_stats(whole, BIG, 2, _id(c))


@pytest.mark.parametrize('kernel', KERNELS)
def test_statistics_add_to_prefilled_accumulators(dev, kernel):
    """stats_finish_kernel<true> after every transition: on zeroed accumulators the totals are the sums of the kept
    states (the matrix above); on accumulators that start at 2.5 and counters that start at 7 they are those plus the
    prefill.  n_bad stays 0: no case has a non-finite log ratio (the host file proves it for the oracle)."""
    r = _run(ODD[kernel])
    base = _launch(dev, r)
    run = _launch(dev, r, prefill=(2.5, 7))
    assert torch.equal(run.samples, base.samples) and torch.equal(run.masks, base.masks)
    _check_stats(run, r.n, T, _key(r) + ' prefilled', prefill=(2.5, 7))


@pytest.mark.parametrize('kernel', KERNELS)
def test_nonfinite_log_ratios_are_counted_and_rejected(dev, kernel):
    """n_bad: two chains started at 1e20 in every coordinate (one in the full tile, one in the ragged one) have U~ = inf in
    fp32 and a log ratio inf - inf at every transition: each is counted once per transition, rejected, and kept where it
    started; every other chain is the plain launch's bit for bit."""
    r = _run(ODD[kernel])
    c = r.case
    q, f, _of = _rows(r)
    base = _launch(dev, r)
    z0 = q.x0.clone()
    bad = [3, 140]
    z0[bad] = 1e20
    run = H._direct_neutra_hmc(dev, H.with_starts(q, z0), f, T, c.L, c.h, SEED, imd=_imd(c), stats='immediate')
    assert run.rc == 0 and run.stats['nonfinite'] == len(bad) * T and run.stats['attempted'] == c.n * T
    assert not bool(run.masks[:, bad].any()) and not bool(torch.isfinite(run.log_ratios[:, bad]).any())
    assert bool((run.samples[:, bad] == 1e20).all()) and bool((run.z[bad] == 1e20).all())
    rest = [i for i in range(c.n) if i not in bad]
    for name in ('samples', 'masks', 'log_ratios'):
        assert torch.equal(getattr(run, name)[:, rest], getattr(base, name)[:, rest]), (_id(c), name)
    assert run.stats['accepted'] == int(base.masks[:, rest].sum())


@pytest.mark.parametrize('kernel', KERNELS)
def test_two_launches_give_the_same_bits_whatever_the_scratch_held(dev, kernel):
    """the second launch starts from a work area and a statistics scratch full of NaN"""
    r = _run(ODD[kernel])
    base = _launch(dev, r)
    run = _launch(dev, r, poison=True)
    for name in ('samples', 'masks', 'log_ratios', 'z'):
        assert torch.equal(getattr(run, name), getattr(base, name)), (_key(r), name)
    assert run.stats['accepted'] == base.stats['accepted'] and run.stats['nonfinite'] == 0
    assert torch.equal(run.stats['sum_x'], base.stats['sum_x']) and torch.equal(run.stats['sum_x2'], base.stats['sum_x2'])


# ------------------------------------------------------------------------------------------------ through NeuTraHMC
def _sampler(c, steps, **params):
    from nfmc_amd.samplers import mcmc, neutra
    p, f, _of = _inputs(c)
    kw = {'inv_mass_diag': _imd(c).clone()} if c.mass else {}
    s = neutra.NeuTraHMC((c.d,), p.pot, mcmc.HMCKernel(event_size=c.d, n_leapfrog_steps=c.L, step_size=c.h, **kw), mcmc.HMCParameters(),
                         neutra.NeuTraKernel((c.d,), flow=f), neutra.NeuTraParameters(n_iterations=steps))
    for k, v in params.items():
        setattr(s.params, k, v)
    s.seed = SEED
    return s


def _sample(monkeypatch, c, steps, **params):
    """NeuTraHMC.sample under a time limit nobody reaches, so that a launch takes at most 4 transitions: (output, the
    (n_steps, step0, store countdown, store row, scratch bytes) of every nfmc_neutra_hmc_steps_f32 call).  The split path
    (inner_sampler.sample) fails the test."""
    from nfmc_amd import hip
    s = _sampler(c, steps, **params)

    def boom(*a, **k):
        raise AssertionError('the run took the split path')
    monkeypatch.setattr(s.inner_sampler, 'sample', boom)
    calls, lib = [], hip.lib()
    real = lib.nfmc_neutra_hmc_steps_f32

    def spy(ref, stream):
        a = ref._obj
        calls.append((a.n_steps, a.rng.step0, a.samples.countdown, a.samples.row, a.scratch_bytes))
        return real(ref, stream)
    monkeypatch.setattr(lib, 'nfmc_neutra_hmc_steps_f32', spy)
    p = _inputs(c)[0]
    out = s.sample(p.x0, show_progress=False, time_limit_seconds=3600.0)
    return out, calls


@pytest.mark.parametrize('kernel', KERNELS)
def test_sampler_run_of_two_launches_follows_the_oracle(dev, monkeypatch, kernel):
    """T = 6 through NeuTraHMC.sample: launches of 4 and 2 transitions, the second from step0 = 4 (words 0 and 1 of the
    second Philox block of accept uniforms); kept states against the oracle, the counters against the kept states."""
    r = _run(ODD[kernel], 'six', 6)
    c = r.case
    conditions(r)
    out, calls = _sample(monkeypatch, c, 6)
    presented = H.neutra_presented_hidden(c.d, c.nh, c.hl)
    sb = H.neutra_hmc_scratch_bytes(c.kernel, c.n, c.d, presented, c.hl, c.cl)
    assert calls == [(4, 0, 0, 0, sb), (2, 4, 0, 4, sb)], calls
    assert H.neutra_hmc_kernel_of(c.d, c.nh, c.hl) == c.kernel
    q, _f, of = _rows(r)
    tr = _oracle(r)
    got = out.samples.reshape(6, c.n, c.d)
    tol = H.neutra_hmc_row_tolerance(tr, q, of, FIGURES[_key(r)][1])
    keep = H.compare_states(got, tr, _key(r), margin=tol, atol=_atol(r), rtol=0.0)
    print('%s: worst state error over atol %.3f' % (_key(r), float((got[:, keep].double() - tr.stacked()[:, keep]).abs().max()) / _atol(r)))
    st = out.statistics
    assert st.n_attempted_trajectories == c.n * 6 and st.n_nonfinite_log_ratios == 0
    moved = (got != torch.cat([q.x0[None], got[:-1]])).any(2)             # an accepted trajectory moves its chain
    assert st.n_accepted_trajectories == int(moved.sum()), (st.n_accepted_trajectories, int(moved.sum()))
    assert abs(st.n_accepted_trajectories - tr.n_accepted) <= 6 * int((~keep).sum())


def _window(dense, thinning, max_samples):
    """MCMCSamples.add's rule (tests/test_gpu_configs.py: _reference_window)"""
    idx = [i for i in range(dense.shape[0]) if i % thinning == 0]
    return dense[idx[-max_samples:] if max_samples else idx]


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('thinning,max_samples', [(2, None), (3, None), (1, 4)], ids=['thinned', 'thinned3', 'ring'])
def test_store_cursor_crosses_launches(dev, monkeypatch, kernel, thinning, max_samples):
    """A DeviceSampleStore with thinning 2 (and 3: a launch that starts inside a stride), and one with a window of 4 rows
    under T = 6 (the ring wraps), through the
    sampler: the host loops of both kernels start each launch's cursor from NfmcSampleStore.countdown / row.  The kept
    rows equal the matching rows of the dense run bit for bit."""
    c = ODD[kernel]
    dense, _calls = _sample(monkeypatch, c, 6)
    dense = dense.samples.reshape(6, c.n, c.d)
    out, calls = _sample(monkeypatch, c, 6, thinning=thinning, max_samples=max_samples)
    want = _window(dense, thinning, max_samples)
    # the second launch starts with the cursor the first left: thinning 2 keeps 0, 2 | 4 (row 2), thinning 3 keeps 0, 3 | and
    # skips 4, 5 (countdown 2), the ring of 4 rows is back at row 0
    second = {(2, None): (2, 4, 0, 2), (3, None): (2, 4, 2, 0), (1, 4): (2, 4, 0, 0)}[(thinning, max_samples)]
    assert [k[:4] for k in calls] == [(4, 0, 0, 0), second], calls
    got = out.samples.reshape(-1, c.n, c.d)
    assert got.shape == want.shape and torch.equal(got, want), _id(c)
    assert torch.equal(out.running_samples.last_sample.reshape(c.n, c.d).cpu(), dense[-1])


# ------------------------------------------------------------------------------------------------ refusals
def _refused(dev, c, code, what, edit=None, steps=2, **kw):
    """the call answers `code` before anything runs: z, the kept states, the masks and the accumulators stay as they were"""
    p, f, _of = _inputs(c)
    q = H.with_starts(p, p.x0[:16])
    kw.setdefault('stats', 'immediate')
    run = H._direct_neutra_hmc(dev, q, f, steps, c.L, c.h, SEED, imd=_imd(c), edit=edit, **kw)
    assert run.rc == code, (what, run.rc, code)
    assert torch.equal(run.z, q.x0) and not bool(run.samples.any()) and not bool(run.masks.any()) and not bool(run.log_ratios.any()), what


def _offset(field):
    def edit(a, run):
        setattr(a, field, C.c_void_p(getattr(a, field) + 4))
    return edit


@pytest.mark.parametrize('kernel', KERNELS)
def test_refusals_precede_every_launch(dev, kernel):
    from nfmc_amd import hip
    c = ODD[kernel]                                       # with a mass diagonal
    _refused(dev, c, hip.EUNSUPPORTED, 'deferred statistics', stats='deferred')
    _refused(dev, c, hip.EUNSUPPORTED, 'rounds = 7', lambda a, run: setattr(a.rng, 'rounds', 7))
    _refused(dev, c, hip.ESHAPE, 'n_steps = 513', steps=513)
    _refused(dev, c, hip.EUNSUPPORTED, 'kind 4', lambda a, run: setattr(a.pot, 'kind', hip.POT_GAUSSIAN_FULL))
    _refused(dev, c, hip.ESCRATCH, 'scratch one byte short', lambda a, run: setattr(a, 'scratch_bytes', a.scratch_bytes - 1))
    # a spline flow is sent to the one-chain-per-lane kernels whatever its width, and those stop at 32
    _refused(dev, c, hip.EUNSUPPORTED, 'spline bins', lambda a, run: setattr(a.flow, 'n_bins', 8))
    assert H.neutra_hmc_kernel_of(c.d, c.nh, c.hl, 8) == 'valu'
    if kernel == 'wide':                                  # 16-byte tiles
        _refused(dev, c, hip.EUNSUPPORTED, 'z off by 4 bytes', _offset('z'))
        _refused(dev, c, hip.EUNSUPPORTED, 'inv_mass_diag off by 4 bytes', _offset('inv_mass_diag'))
