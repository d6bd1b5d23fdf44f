"""CPU: the inputs of tests/test_gpu_mclmc_matrix.py (tests/mclmc_cases.py), not the kernel.  Every case lands on the
register layout of its capacity and is one the fused kernels take; CASES and UNREACHABLE together are the whole grid of
15 potential kinds x 9 default layouts; and the fp64 reference (tests/mclmc_fp64.py) takes every step of every case in
fp32 and in fp64 with tolerances that mean something: finite, positive, and for the states at most 64 fp32 ulps of the
case's largest |x| (a cap against a vacuous case, not a measurement)."""
import ctypes as C
import math

import pytest
import torch

import mclmc_cases as cases

ULPS = 64.0


def _layout(d, kind):
    from nfmc_amd import hip
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(d, kind, C.byref(cpl), C.byref(lpc)) == hip.OK
    return cpl.value, lpc.value


def test_the_kinds_are_the_library_s_fifteen_in_order():
    from nfmc_amd import hip
    ids = [hip.POT_QUADRATIC, hip.POT_FUNNEL, hip.POT_GAUSSIAN_MIXTURE, hip.POT_LOGISTIC_REGRESSION, hip.POT_GAUSSIAN_FULL,
           hip.POT_ROSENBROCK, hip.POT_STOCHASTIC_VOLATILITY, hip.POT_SPARSE_LOGISTIC_REGRESSION, hip.POT_LATTICE_PHI4,
           hip.POT_ITEM_RESPONSE, hip.POT_VARYING_EFFECTS, hip.POT_PARTICLES, hip.POT_LATENT_GAUSSIAN, hip.POT_LATENT_GMRF,
           hip.POT_DIFFUSION_BRIDGE]
    assert ids == list(range(len(cases.KINDS))) and len(cases.KINDS) == 15
    assert cases.OWN_UNIT_KINDS == cases.KINDS[4:] and len(cases.OWN_UNIT_KINDS) == 11


@pytest.mark.parametrize('case', cases.CASES, ids=cases.case_id)
def test_every_case_lands_on_the_layout_of_its_capacity_and_is_fused(case):
    kind, cap, _size = case
    pot, _ref, x0 = cases.build(kind, cap)
    d = cases.case_d(case)
    assert pot.event_size == d and tuple(x0.shape) == (cases.MATRIX_N, d) and x0.dtype == torch.float32
    assert cap / 2 < d <= cap
    assert _layout(d, cases.KINDS.index(kind)) == cases.LAYOUTS[cap]
    assert pot.fused_in('mcmc')
    assert torch.isfinite(x0).all()


def test_the_cases_and_the_unreachable_pairs_are_the_whole_grid():
    have = [(k, cap) for k, cap, _ in cases.CASES]
    gone = [(k, cap) for k, cap, _ in cases.UNREACHABLE]
    assert len(set(have)) == len(have) and len(set(gone)) == len(gone) and not set(have) & set(gone)
    assert set(have) | set(gone) == {(k, cap) for k in cases.KINDS for cap in cases.CAPACITIES}
    assert len(have) + len(gone) == 15 * 9
    assert all(isinstance(r, str) and r and '\n' not in r for _, _, r in cases.UNREACHABLE)
    for kind in ('quadratic', 'funnel', 'mixture', 'logreg', 'fullrank', 'rosenbrock'):     # these take any d
        assert sum(k == kind for k, _ in have) == 9, kind


def test_the_sizes_are_ragged_where_the_kind_allows_and_every_kind_has_an_exact_fit():
    exact = {k: 0 for k in cases.KINDS}
    for case in cases.CASES:
        kind, cap, _ = case
        d, cpl = cases.case_d(case), cases.LAYOUTS[cap][0]
        if d == cap:
            exact[kind] += 1
        elif kind == 'phi4':                       # d % 4 == 0: ragged against CPL = 8 and 16 only
            assert d % 4 == 0 and (cpl == 4 or d % cpl != 0), case
        else:
            assert d % cpl != 0, case
    odd_only = {'sparse_logreg'}                   # d = 2 D + 1
    assert all((n == 0) == (k in odd_only) for k, n in exact.items()), exact
    # a ragged and an exact case on every layout
    for cap in cases.CAPACITIES:
        ds = [cases.case_d(c) for c in cases.CASES if c[1] == cap]
        assert cap in ds and any(d < cap for d in ds), cap


def _shapes_of(kind, d):
    """every way the parameterisation of `kind` produces event size d, as zero-argument constructors of the potential"""
    from nfmc_amd import potentials as P
    if kind == 'phi4':
        out = [lambda: P.LatticePhi4((d,))]
        return out + [lambda h=h: P.LatticePhi4((h, d // h)) for h in range(1, d + 1) if d % h == 0]
    if kind == 'sparse_logreg':
        if d % 2 == 0 or d < 3:
            return []
        return [lambda: P.SparseLogisticRegression(torch.ones(2, (d - 1) // 2), torch.tensor([0.0, 1.0]))]
    if kind == 'sv':
        return [lambda: P.StochasticVolatility(torch.zeros(d - 3))] if d >= 4 else []
    if kind == 'irt':
        return [lambda: P.ItemResponseTheory(torch.zeros(1, d - 2))] if d >= 3 else []
    if kind == 'particles':
        return [lambda D=D: P.ParticleSystem(d // D, D) for D in (1, 2, 3) if d % D == 0 and d // D >= 2]
    raise AssertionError('%s takes every d: it has no unreachable pair' % kind)


def test_no_size_of_an_unreachable_pair_builds_and_fuses():
    for kind, cap, _reason in cases.UNREACHABLE:
        for d in range(cap // 2 + 1, cap + 1):
            for make in _shapes_of(kind, d):
                try:
                    pot = make()
                except ValueError:
                    continue
                assert not pot.fused_in('mcmc'), (kind, cap, d)
    # the lattice is the kind that leaves sizes unfused: a row length that is no multiple of 4 is refused ...
    from nfmc_amd.potentials import LatticePhi4
    assert not LatticePhi4((7,)).fused_in('mcmc') and not LatticePhi4((6, 6)).fused_in('mcmc')
    # ... and every capacity's range still holds a multiple of 4
    assert all(any(d % 4 == 0 for d in range(cap // 2 + 1, cap + 1)) for cap in cases.CAPACITIES)


@pytest.mark.parametrize('case', cases.CASES, ids=cases.case_id)
def test_the_reference_takes_every_step_and_the_tolerances_mean_something(case):
    kind, cap, _size = case
    r = cases.reference(kind, cap)            # _figures asserts that both the fp32 and the fp64 run take every step
    xs, us, des, taken = r['r64']
    d = cases.case_d(case)
    assert bool(taken.all()) and tuple(xs.shape) == (cases.MATRIX_T, cases.MATRIX_N, d)
    assert torch.isfinite(xs).all() and torch.isfinite(us).all() and torch.isfinite(des).all()
    assert r['eps'] > 0 and math.isfinite(r['eps']) and r['L'] == math.sqrt(d)
    xmax = float(xs.abs().max())
    ulp = 2.0 ** (math.floor(math.log2(xmax)) - 23)
    print('%s d=%d eps=%.3g: |x| <= %.3g  tol x %.3g (%.1f ulp)  u %.3g  dE %.3g (|dE| <= %.3g)'
          % (cases.case_id(case), d, r['eps'], xmax, r['tol']['x'], r['tol']['x'] / ulp, r['tol']['u'], r['tol']['de'],
             float(des.abs().max())))
    for k in ('x', 'u', 'de'):
        assert math.isfinite(r['tol'][k]) and r['tol'][k] > 0, (k, r['tol'][k])
    assert r['tol']['x'] <= ULPS * ulp, (r['tol']['x'] / ulp, xmax)
    # the steps move: a case whose chains stand still would pass anything
    x0 = cases.build(kind, cap)[2].double()
    assert float((xs[-1] - x0).abs().max()) > 100 * r['tol']['x']
