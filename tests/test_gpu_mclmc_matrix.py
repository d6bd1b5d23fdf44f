"""GPU: mclmc_kernel (csrc/sampler_mclmc.hpp) at every potential kind and every default register layout, against the fp64
reference of tests/mclmc_fp64.py.  The cases are those of tests/mclmc_cases.py (CASES: 15 kinds x 9 layouts);
tests/test_host_mclmc_matrix.py checks on the CPU that each lands on its layout, that the reference takes every step and
that the tolerances are tight.

  a  every case step by step: 71 chains (odd: the last wave is part-filled at every LPC < 64), 6 steps, a mass diagonal
     linspace(0.5, 2, d), eps by the step rule on sigma g, L = sqrt(d).  x at every step, the final u and dE at every step
     of every chain to MARGIN = 4 times the reference's own fp32-against-fp64 difference on the case's inputs.
  b  a chain that never moves (x0[j, 0] = 3e38: its energy error is never finite) stays where it is, is counted, and leaves
     every other chain's bits alone: the lanes of an idle or non-finite chain against the staged blocks and lane exchanges
     of the potentials.  The per-chain `mine` mask is reached by one input only, a chain with a finite energy error and a
     state over the kernel's bound: the last test of the section, on a quadratic that is flat in one coordinate.  No
     potential indexes memory by x (the one index read from data, GmrfPot's ELL column, is table data and clamped), so
     3e38 is arithmetic only.
  c  the tuning launch (eps and L read from the state, sums about the shift) on a staged, a neighbour-exchange and an
     all-pairs kind at capacity 64: every controller update against mclmc_fp64.replay_update, the un-shifted moments against
     the kept states.

Every case prints what it measured (pytest -s); DESIGN.md 3.7 records the figures.
"""
import math

import pytest
import torch

import mclmc_cases as cases
import mclmc_fp64 as M
from mclmc_cases import MARGIN, SEED, compare, launch, velocity

pytestmark = pytest.mark.gpu

N, T = cases.MATRIX_N, cases.MATRIX_T


@pytest.fixture(scope='module')
def dev():
    from nfmc_amd import hip
    return hip.require_gpu()


# ------------------------------------------------------------------------------------------------ a. step by step
@pytest.mark.parametrize('case', cases.CASES, ids=cases.case_id)
def test_a_every_kind_follows_fp64_at_every_layout(dev, case):
    kind, cap, _size = case
    pot, _ref, x0 = cases.build(kind, cap)
    r = cases.reference(kind, cap)
    d = x0.shape[1]
    # hip.check raises unless the return code is NFMC_OK: the fused kernel of this kind and layout ran
    run = launch(dev, pot, x0, r['u0'], T, r['eps'], r['L'], r['imd'])
    compare(run, r['r64'], r['tol'], '%s layout %s d=%d eps=%.3g' % (kind, cases.LAYOUTS[cap], d, r['eps']))


# ------------------------------------------------------------------------------------------------ b. a chain that stays
STILL = (35, 70)         # a chain inside a wave, and the last chain of the last, part-filled wave (every LPC < 64)
STILL_CASES = sorted({(kind, cases.nearest(kind, cap)) for kind in cases.KINDS for cap in (16, 32, 1024)},
                     key=lambda c: (cases.KINDS.index(c[0]), c[1]))


# 3e38 rounds to the very fp32 number the kernel compares |x'| against (3.0e38f), and a step cannot move it (its ulp is 2e31):
# the chain is stopped by its non-finite energy error, on its own lanes
STILL_VALUES = (3e38,)


@pytest.mark.parametrize('kind,cap', STILL_CASES, ids=['%s-%d' % c for c in STILL_CASES])
def test_b_a_chain_that_never_moves_leaves_its_neighbours_alone(dev, kind, cap):
    from nfmc_amd import hip
    pot, ref, x0 = cases.build(kind, cap)
    d = x0.shape[1]
    imd, u0 = cases.mass_diagonal(d), velocity(N, d)
    eps, L = cases.step_size(ref, x0, imd), math.sqrt(d)
    clean = launch(dev, pot, x0, u0, T, eps, L, imd)
    still = list(STILL)
    others = [i for i in range(N) if i not in STILL]
    assert torch.isfinite(clean['kept']).all() and torch.isfinite(clean['de']).all()
    for value in STILL_VALUES:
        bad = x0.clone()
        bad[still, 0] = value
        stats = hip.DeviceStats(d, dev)
        run = launch(dev, pot, bad, u0, T, eps, L, imd, stats=stats)
        kept, u, de = run['kept'].cpu(), run['u'].cpu(), run['de'].cpu()
        # the chain holds its start, bit for bit, at every kept step, and its velocity went through O alone
        assert torch.equal(kept[:, still], bad[still][None].expand(T, -1, -1)), (kind, cap, value)
        assert torch.equal(run['x'].cpu()[still], bad[still]), (kind, cap, value)
        assert torch.isfinite(u[still]).all()
        assert torch.allclose(u[still].double().norm(dim=1), torch.ones(2, dtype=torch.float64), atol=1e-5)
        assert not torch.isfinite(de[:, still]).any()
        cnt = stats.host_totals()[2]
        assert int(cnt[hip.CNT_NONFINITE]) == len(STILL) * T and int(cnt[hip.CNT_ATTEMPTED]) == N * T, (kind, cap, value)
        # every other chain: the bits of the clean run
        assert torch.equal(kept[:, others], clean['kept'].cpu()[:, others]), (kind, cap, value)
        assert torch.equal(u[others], clean['u'].cpu()[others]), (kind, cap, value)
        assert torch.equal(de[:, others], clean['de'].cpu()[:, others]), (kind, cap, value)


@pytest.mark.parametrize('cap', [16, 32, 256])
def test_b_a_chain_stopped_by_its_state_alone_leaves_its_wave_alone(dev, cap):
    """The one way to the `mine` mask.  The kernel asks `finite dE && (ballot(wild) & mine) == 0`, so the ballot is taken
    by the chains with a finite energy error only, and every potential of the matrix answers 3e38 with a non-finite U: in
    the cases above the mask decides nothing (a kernel with `mine` of all ones passes them, measured).  A quadratic that is
    flat in coordinate 0 (a_0 = 0: term and gradient are exactly 0 there) keeps U, and so dE, finite at x_0 = 3.2e38: the
    chain is stopped by the bound on |x'| alone, through the ballot over its wave, and a mask wider than the chain's own
    lanes stops the chains that share its wave (4, 8 and 32 lanes per chain here)."""
    from nfmc_amd import hip
    from nfmc_amd.potentials import QuadraticPotential
    d = cases.RAGGED[cap]
    a = torch.linspace(0.3, 2.0, d, dtype=torch.float64).float()
    a[0] = 0.0
    pot = QuadraticPotential((d,), a, torch.linspace(-0.5, 0.5, d, dtype=torch.float64).float())
    x0, u0, imd = cases.starts(N, d, 100 + d), velocity(N, d), cases.mass_diagonal(d)
    eps, L = 0.125 * math.sqrt(d), math.sqrt(d)
    clean = launch(dev, pot, x0, u0, T, eps, L, imd)
    still = list(STILL)
    others = [i for i in range(N) if i not in STILL]
    bad = x0.clone()
    bad[still, 0] = 3.2e38
    stats = hip.DeviceStats(d, dev)
    run = launch(dev, pot, bad, u0, T, eps, L, imd, stats=stats)
    kept, u, de = run['kept'].cpu(), run['u'].cpu(), run['de'].cpu()
    assert torch.isfinite(de).all()                  # the energy error does not stop the chain: the bound on |x'| does
    assert torch.equal(kept[:, still], bad[still][None].expand(T, -1, -1))
    assert torch.isfinite(u[still]).all()
    cnt = stats.host_totals()[2]
    assert int(cnt[hip.CNT_NONFINITE]) == len(STILL) * T and int(cnt[hip.CNT_ATTEMPTED]) == N * T
    assert torch.equal(kept[:, others], clean['kept'].cpu()[:, others])
    assert torch.equal(u[others], clean['u'].cpu()[others])
    assert torch.equal(de[:, others], clean['de'].cpu()[:, others])
    assert not torch.equal(clean['kept'].cpu()[-1][others], x0[others])      # and they do move


# ------------------------------------------------------------------------------------------------ c. the tuning launch
EVERY, WARMUP = 3, 8        # pools of 3, 3 and 2 steps: the last one is short
KW = dict(target=5e-4, imd_adjustment=0.25, decoherence_factor=1.0, tune_inv_mass_diag=True)


def _tuning(dev, pot, x0, d, eps, L, imd0, updates):
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc
    from nfmc_amd.samplers.common import Run
    s = mcmc.MCLMC((d,), pot, mcmc.MCLMCKernel(d, step_size=eps, decoherence_length=L, inv_mass_diag=imd0),
                   mcmc.MCLMCParameters(n_iterations=WARMUP, tune_every=EVERY, tune_inv_mass_diag=True, tuning=True))
    s.seed, s.shard, s.fuse, s.replay = SEED, None, 'auto', None
    return mcmc.MclmcTuning(s, Run(s, x0), updates), hip.DeviceStats(d, dev)


@pytest.mark.parametrize('kind', ['irt', 'phi4', 'particles'])
def test_c_the_tuning_launch_on_own_unit_kinds_is_the_replay_of_its_records(dev, kind):
    from nfmc_amd import hip
    cap = 64
    pot, ref, x0 = cases.build(kind, cap)
    d = x0.shape[1]
    assert d < cap and d % cases.LAYOUTS[cap][0] != 0           # ragged
    imd0 = cases.mass_diagonal(d)
    eps0, L0 = cases.step_size(ref, x0, imd0), math.sqrt(d)
    pools = [min(EVERY, WARMUP - s0) for s0 in range(0, WARMUP, EVERY)]
    assert pools == [3, 3, 2]
    tune, stats = _tuning(dev, pot, x0, d, eps0, L0, imd0, len(pools))
    x, u = x0, velocity(N, d, SEED, hip.WARMUP_STEP0)
    eps, L, imd = eps0, L0, imd0.clone()
    kept_all, done = [], 0
    for j, k in enumerate(pools):
        r = launch(dev, pot, x, u, k, eps, L, tune=tune, stats=stats, step0=hip.WARMUP_STEP0 + done)
        assert torch.isfinite(r['de']).all() and torch.isfinite(r['kept']).all()
        c64 = M.replay_update(r['de'].cpu(), r['kept'].cpu(), eps, L, imd, torch.float64, **KW)
        c32 = M.replay_update(r['de'].cpu(), r['kept'].cpu(), eps, L, imd, torch.float32, **KW)
        st = tune.state.cpu()
        got = (float(st[hip.MCLMC_STEP_SIZE]), float(st[hip.MCLMC_DECOHERENCE_LENGTH]), tune.imd.cpu().double())
        want = (c64.step_size, c64.decoherence_length, c64.inv_mass_diag.double())
        spread = (abs(c32.step_size - c64.step_size), abs(c32.decoherence_length - c64.decoherence_length),
                  float((c32.inv_mass_diag.double() - want[2]).abs().max()))
        # test 7's tolerance: 4 x the replay's own fp32-against-fp64 difference, and never under an fp32 ulp of the value
        tol = [MARGIN * sp + 2.0 ** -23 * abs(w) for sp, w in zip(spread, (want[0], want[1], float(want[2].abs().max())))]
        diff = (abs(got[0] - want[0]), abs(got[1] - want[1]), float((got[2] - want[2]).abs().max()))
        print('%s d=%d update %d (%d steps): eps %.6g (diff %.3g tol %.3g)  L %.6g (diff %.3g tol %.3g)  scales diff %.3g tol %.3g'
              '  V %.3g' % (kind, d, j, k, got[0], diff[0], tol[0], got[1], diff[1], tol[1], diff[2], tol[2],
                            float(st[hip.MCLMC_ENERGY_VARIANCE])))
        assert all(dd <= tt for dd, tt in zip(diff, tol)), (kind, j, diff, tol)
        assert float(st[hip.MCLMC_COUNT]) == N * k
        assert got[0] != eps and got[1] != L and not torch.equal(got[2].float(), imd.float())      # every tuner moved
        kept_all.append(r['kept'].cpu().double())
        x, u, eps, L, imd = r['x'], r['u'], got[0], got[1], tune.imd.cpu().clone()
        done += k
    # the un-shifted moments the launches booked are those of the kept states (the tolerance test 6 holds them to)
    kept = torch.cat(kept_all)
    sx, sx2, cnt, _ = stats.host_totals()
    m = N * WARMUP
    assert int(cnt[hip.CNT_ATTEMPTED]) == m == int(cnt[hip.CNT_ACCEPTED]) and int(cnt[hip.CNT_NONFINITE]) == 0
    assert torch.allclose(sx / m, kept.mean((0, 1)), rtol=1e-5, atol=1e-6)
    assert torch.allclose(sx2 / m, (kept ** 2).mean((0, 1)), rtol=1e-5, atol=1e-6)
    assert float(tune.state.cpu()[hip.MCLMC_HISTORY_USED]) == len(pools)
    # the whole warmup in ONE call (NfmcMclmcTune.every = 3 over 8 steps) leaves the same words
    tune1, stats1 = _tuning(dev, pot, x0, d, eps0, L0, imd0, len(pools))
    r1 = launch(dev, pot, x0, velocity(N, d, SEED, hip.WARMUP_STEP0), WARMUP, eps0, L0, tune=tune1, stats=stats1,
                step0=hip.WARMUP_STEP0)
    assert torch.equal(tune1.state.cpu()[:hip.MCLMC_WORDS], tune.state.cpu()[:hip.MCLMC_WORDS])
    assert torch.equal(tune1.imd.cpu(), tune.imd.cpu())
    assert torch.equal(r1['x'], x) and torch.equal(r1['u'], u) and torch.equal(r1['kept'].cpu().double(), kept)
