"""GPU: NeuTra-MH on the fused kernel (nfmc_neutra_mh_steps_f32, csrc/neutra_mh.hpp) against the fp64 CPU oracle

    oracle.samplers.mcmc_sample(z0.double(), neutra_adjusted_target(of, ref, (d,)), 'mh', T, 0.0, imd,
                                noise=PhiloxNoise(seed, dtype=torch.float64))

on a perturbed flow pair, with inv_mass_diag = 0.5 / sqrt(d) on every coordinate (tests/neutra_mh_cases.py).  n = 96 chains
and T = 4 transitions unless a test says otherwise: one full and one ragged tile at 64 rows per wave, three tiles at 32,
six at 16.

Comparison.  A chain whose fp64 |log u - log r| falls under the project's bound on an fp32 log ratio at any transition,
    2e-4 max(1, d / 64) + 1e-4 |log r| + 8 2^-24 |U~|     (H.compare_decisions; cases.margin),
is excluded as a near-tie; at most 10 % of the chains may be (H.compare_states' cap).  The chains kept differ from the
oracle only by the fp32 rounding of z + eps m and of the Box-Muller normals: ATOL and RTOL below.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import neutra_mh_cases as cases
import target_harness as H

pytestmark = pytest.mark.gpu

N, T, SEED = cases.N, cases.T, cases.SEED
# State tolerance of the chains kept, atol + rtol |want| = 6.3e-7 (1 + |want|).  The NeuTra-HMC comparisons use atol 1e-3
# (H.neutra_hmc_fused_matches_oracle); the first run of this file with that value measured, over every case below, a worst
# error of 4.77e-7 (one ulp of a state between 4 and 8) and 1.57e-7 relative to 1 + |want|; four times the latter is kept.
# The split-path runs of sections 6 and 7 measured the same figures (they form z + eps m in the same two roundings).
ATOL, RTOL = 6.3e-7, 6.3e-7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ helpers
class Bare:
    """One call of the bare entry point from z0: the return code, the final state, the kept states (T, n, d), the masks
    and the log ratios (T, n).  `edit(args)` may spoil the arguments first."""

    def __init__(self, dev, f, pot, z0, T, seed, adjust=True, edit=None, scale=None, stats=False):
        from nfmc_amd import hip
        n, d = z0.shape
        self.z = z0.to(dev, torch.float32).contiguous().clone()
        self.kept = torch.zeros(T, n, d, device=dev)
        self.m = torch.zeros(T, n, dtype=torch.uint8, device=dev)
        self.lr = torch.zeros(T, n, device=dev)
        self.imd = (cases.imd(d) if scale is None else scale).to(dev, torch.float32)
        st, self._keep = f.bijection.packed(dev, 0)
        a = hip.NfmcNeutraMhArgs()
        a.z, a.n, a.n_steps, a.adjust = hip.ptr(self.z), n, T, 1 if adjust else 0
        a.inv_mass_diag = hip.ptr(self.imd)
        a.flow, a.pot = st, pot.descriptor(dev)
        a.rng = hip.make_rng(seed, 0, 0)
        if stats:
            self.stats = hip.DeviceStats(d, dev)
            a.stats = self.stats.struct()
        a.samples = hip.dense_store(self.kept)
        a.masks_out, a.log_ratio_out = hip.ptr(self.m, torch.uint8), hip.ptr(self.lr)
        if edit is not None:
            edit(a)
        self.args = a
        self.rc = int(hip.lib().nfmc_neutra_mh_steps_f32(C.byref(a), hip.stream()))
        torch.cuda.synchronize()

    def stacked(self):
        return self.m.cpu().bool(), self.lr.cpu()


def _states(got, tr, z0, of, ref, what, atol=ATOL, rtol=RTOL):
    """H.compare_states under the near-tie margin of the run; prints the worst error of the chains kept first.
    Returns the number of chains excluded."""
    mg = cases.margin(tr, z0, of, ref)
    lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
    keep = ((lu - lr).abs() >= mg).all(0)
    want = tr.stacked().float()
    err = (got[:, keep] - want[:, keep]).abs()
    print('%s: worst state error %.2e (relative to 1 + |want|: %.2e), oracle acceptance %.3f'
          % (what, float(err.max()), float((err / (1 + want[:, keep].abs())).max()), tr.n_accepted / tr.n_attempted))
    H.compare_states(got, tr, what, margin=mg, atol=atol, rtol=rtol)
    return int((~keep).sum())


def _spied(monkeypatch, s, through=False):
    """counts the calls of the inner sampler's sample(): the split path.  `through`: the call still runs."""
    calls = []
    orig = s.inner_sampler.sample
    monkeypatch.setattr(s.inner_sampler, 'sample', lambda *a, **k: calls.append(1) or (orig(*a, **k) if through else None))
    return calls


def _fused_matches_oracle(dev, monkeypatch, pot, ref, flows, z0, what, T=T):
    """Through NeuTraMH.sample, never the inner sampler's split path; then the bare entry point for the decisions."""
    f, of = flows
    n, d = z0.shape
    tr = cases.oracle(z0, of, ref, T)
    s = cases.sampler(d, pot, f, T)
    s.seed = SEED
    split = _spied(monkeypatch, s)
    out = s.sample(z0, show_progress=False)
    assert not split, 'the run took the split path'
    got = out.samples.reshape(T, n, d)
    excluded = _states(got, tr, z0, of, ref, what)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T and st.n_target_calls == 2 * n * T and st.n_target_gradient_calls == 0
    # a chain that is no near-tie decides as the oracle does at every transition
    assert abs(st.n_accepted_trajectories - tr.n_accepted) <= T * excluded, (st.n_accepted_trajectories, tr.n_accepted)
    b = Bare(dev, f, pot, z0, T, SEED)
    assert b.rc == 0
    assert torch.equal(b.kept.cpu(), got) and torch.equal(b.z.cpu(), got[-1])
    assert int(b.m.sum()) == st.n_accepted_trajectories
    H.compare_decisions(b, tr, 'mh', z0, ref, what, mag=cases.magnitude(of, ref, d))
    return out, tr


# ------------------------------------------------------------------------------------------------ 1. against the oracle
# (d, conditioner width): every HP bucket (3 -> 4, 8, 16, 32), d = 2, 3, 5, 64, 512 and both sides of every switch
REALNVP = [(2, 3), (3, 8), (5, 16), (64, 32), (148, 8), (149, 3), (196, 16), (197, 8), (300, 3), (301, 8), (396, 32),
           (397, 16), (512, 3)]


@pytest.mark.parametrize('target', ['sumsq', 'funnel'])
@pytest.mark.parametrize('d,nh', REALNVP)
def test_fused_matches_oracle(dev, monkeypatch, target, d, nh):
    pot, ref = cases.TARGETS[target](d)
    _fused_matches_oracle(dev, monkeypatch, pot, ref, cases.flows(d, 'realnvp', nh), cases.starts(N, d),
                          '%s d=%d H=%d' % (target, d, nh))


@pytest.mark.parametrize('target', ['sumsq', 'funnel'])
@pytest.mark.parametrize('kind,d,nh', [('nice', 5, 8), ('nice', 65, 16), ('c-rqnsf', 5, 8), ('c-rqnsf', 65, 32)])
def test_fused_matches_oracle_on_other_couplings(dev, monkeypatch, target, kind, d, nh):
    pot, ref = cases.TARGETS[target](d)
    _fused_matches_oracle(dev, monkeypatch, pot, ref, cases.flows(d, kind, nh), cases.starts(N, d),
                          '%s %s d=%d H=%d' % (target, kind, d, nh))


@pytest.mark.parametrize('n', [1, 63])
def test_a_ragged_single_tile(dev, monkeypatch, n):
    d = 5
    pot, ref = cases.funnel(d)
    z0 = cases.starts(n, d)    # n = 1: the one chain is clear of a tie at all four transitions (the oracle alone)
    _fused_matches_oracle(dev, monkeypatch, pot, ref, cases.flows(d, 'realnvp', 8), z0, 'funnel n=%d' % n)


# ------------------------------------------------------------------------------------------------ 2. own-unit kinds
@pytest.mark.parametrize('kind', sorted(cases.OWN_KINDS))
def test_kernel_matches_oracle_on_own_unit_kinds(dev, monkeypatch, kind):
    """Starts and flows as the kinds' own NeuTra-HMC tests take them (flow seed 9).  MH reuses their row forms: this
    shows that the dispatch of adjusted_potential_row reaches each.  A kind that NeuTra.sample sends to the kernel
    (cases.ON_KERNEL) runs through the sampler and the bare entry point; one that it keeps on the split path, because the
    kernel was measured slower there, runs the split path once, and the kernel through the bare entry point alone."""
    pot, ref, z0, nh = cases.OWN_KINDS[kind]()
    d = z0.shape[1]
    flows = H.flow_pair(d, 9, n_hidden=nh, init_seed=1000 + d)
    if cases.ON_KERNEL[kind]:
        return _fused_matches_oracle(dev, monkeypatch, pot, ref, flows, z0, kind)
    f, of = flows
    tr = cases.oracle(z0, of, ref, T)
    s = cases.sampler(d, pot, f, T)
    s.seed = SEED
    assert s._closed_form() is pot
    split = _spied(monkeypatch, s, through=True)
    out = s.sample(z0, show_progress=False)
    assert split == [1]
    _states(out.samples.reshape(T, N, d), tr, z0, of, ref, kind + ' (split)')
    b = Bare(dev, f, pot, z0, T, SEED)
    assert b.rc == 0 and torch.equal(b.z.cpu(), b.kept.cpu()[-1])
    excluded = _states(b.kept.cpu(), tr, z0, of, ref, kind + ' (kernel)')
    assert abs(int(b.m.sum()) - tr.n_accepted) <= T * excluded
    H.compare_decisions(b, tr, 'mh', z0, ref, kind, mag=cases.magnitude(of, ref, d))


# ------------------------------------------------------------------------------------------------ 3. unadjusted
@pytest.mark.parametrize('d', [5, 149])
def test_unadjusted_run_keeps_every_proposal(dev, monkeypatch, d):
    pot, ref = cases.sum_of_squares(d)
    f, of = cases.flows(d, 'realnvp', 8)
    z0 = cases.starts(N, d)
    s = cases.sampler(d, pot, f, T, adjustment=False)
    s.seed = SEED
    split = _spied(monkeypatch, s)
    out = s.sample(z0, show_progress=False)
    assert not split
    assert out.statistics.n_target_calls == 0 and out.statistics.n_accepted_trajectories == N * T
    tr = cases.oracle(z0, of, ref, T, adjustment=False)             # z0 plus the running sum of eps m, in fp64
    np.testing.assert_allclose(out.samples.reshape(T, N, d).numpy(), tr.stacked().numpy(), rtol=1e-6, atol=1e-6)
    b = Bare(dev, f, pot, z0, T, SEED, adjust=False)
    assert b.rc == 0 and bool((b.m == 1).all()) and bool((b.lr == 0).all())
    assert torch.equal(b.kept.cpu(), out.samples.reshape(T, N, d))


@pytest.mark.parametrize('d,adjustment', [(5, True), (149, True), (301, False)])
def test_replayed_noise_matches_oracle(dev, monkeypatch, d, adjustment):
    """The kernel's other noise source: normals (T, n, d) and uniforms (T, n) recorded from the oracle's torch draws and
    handed over through `sampler.replay` (NfmcRng.replay_normals / replay_uniforms, laid out as (s, row, c))."""
    pot, ref = cases.funnel(d)
    f, of = cases.flows(d, 'realnvp', 8)
    z0 = cases.starts(N, d)
    s = cases.sampler(d, pot, f, T, adjustment=adjustment)
    split = _spied(monkeypatch, s)
    out, tr, _rec, _spy = H.replay_run(monkeypatch, s, lambda noise: cases.oracle(z0, of, ref, T, adjustment=adjustment, noise=noise),
                                       z0, 7 + d, False)
    assert not split
    got = out.samples.reshape(T, N, d)
    if adjustment:
        _states(got, tr, z0, of, ref, 'replay d=%d' % d)
    else:
        np.testing.assert_allclose(got.numpy(), tr.stacked().numpy(), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 4. statistics, store
def test_statistics_and_sample_store(dev):
    d = 149
    pot, ref = cases.funnel(d)
    f, _of = cases.flows(d, 'realnvp', 8)
    z0 = cases.starts(N, d)

    def run(**params):
        s = cases.sampler(d, pot, f, T)
        s.seed = SEED
        for k, v in params.items():
            setattr(s.params, k, v)
        return s.sample(z0, show_progress=False)
    out = run()
    dense = out.samples.reshape(T, N, d)
    b = Bare(dev, f, pot, z0, T, SEED)
    assert b.rc == 0 and torch.equal(b.kept.cpu(), dense)
    assert out.statistics.n_accepted_trajectories == int(b.m.sum())
    assert 0 < int(b.m.sum()) < N * T
    x = dense.double()
    mean, second = x.mean((0, 1)), (x * x).mean((0, 1))
    np.testing.assert_allclose(out.mean.double().numpy(), mean.numpy(), rtol=0, atol=1e-5 * float(mean.abs().max()))
    var = second - mean ** 2
    np.testing.assert_allclose(out.variance.double().numpy(), var.numpy(), rtol=0, atol=1e-5 * float(second.abs().max()))
    assert torch.equal(run(thinning=2).samples.reshape(-1, N, d), dense[0::2])
    assert torch.equal(run(max_samples=2).samples.reshape(-1, N, d), dense[-2:])


# ------------------------------------------------------------------------------------------------ 5. repeatability
def test_determinism_and_sharding(dev):
    d, n = 16, 301
    pot, _ref = cases.funnel(d)
    f, _of = cases.flows(d, 'realnvp', 8)
    H.determinism_and_sharding(lambda: cases.sampler(d, pot, f, T), cases.starts(n, d), T, d, seed=SEED, world=3)


def test_determinism_and_sharding_when_the_grid_strides(dev):
    """2049 tiles of 16 rows: more than kMaxGrid = 2048 workgroups, so the dense run strides the grid and the three shards
    do not; both must give the same bits."""
    d, steps = 301, 2
    assert cases.rows_per_wave(d) == 16
    n = 2048 * 16 + 5
    pot, _ref = cases.sum_of_squares(d)
    f, _of = cases.flows(d, 'realnvp', 4)
    H.determinism_and_sharding(lambda: cases.sampler(d, pot, f, steps), cases.starts(n, d), steps, d, seed=SEED, world=3)


# ------------------------------------------------------------------------------------------------ 6. fused against split
@pytest.mark.parametrize('d', [5, 149])
def test_fused_equals_split(dev, monkeypatch, d):
    """The potential object against the same object behind a lambda with fuse='never': the same seed gives the same
    draws; H.fused_equals_split's convention for the share.  Counts: no split-path transition on the fused run, T on the
    other, where the callable is evaluated twice per transition (x and x', mh.py:58)."""
    pot, _ref = cases.funnel(d)
    f, _of = cases.flows(d, 'realnvp', 8)
    z0 = cases.starts(N, d)
    evaluations = []

    def behind(x):
        evaluations.append(1)
        return pot(x)
    outs, counts = [], []
    for target, fuse in ((pot, 'auto'), (behind, 'never')):
        spy = H.Spy(monkeypatch)
        s = cases.sampler(d, target, f, T)
        s.seed, s.fuse = SEED, fuse
        outs.append(s.sample(z0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T] and len(evaluations) == 2 * T
    assert outs[0].statistics.n_target_calls == outs[1].statistics.n_target_calls == 2 * N * T
    a, b = (o.samples.reshape(T, N, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < ATOL
    print('d=%d: %.3f of the chains agree, worst difference among them %.2e' % (d, float(same.float().mean()),
                                                                              float((a - b)[:, same].abs().max())))
    assert same.float().mean() > 0.9, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------------------------------ 7. what stays split
@pytest.mark.parametrize('case', [c for c in cases.ROUTES if not c.fused], ids=lambda c: c.name)
def test_what_stays_on_the_split_path(dev, monkeypatch, case):
    """Each runs the inner sampler's split path exactly once and still follows the oracle.

    rng_rounds=7 is the exception in its second half.  The split path has never carried the Philox4x32-7 stream: its
    accept/select launch (nfmc_mh_accept_select_f32) takes the default rounds only, so that run ends in the ValueError that
    DESIGN.md documents for every launch without the opt-in stream, before and after this kernel.  What the case pins is
    that the run is not sent to the fused kernel on the other stream: the split path is entered once and refuses."""
    from nfmc_amd import hip
    d = case.d
    target, ref = case.problem()
    f, of = case.flows()
    z0 = cases.starts(N, d)
    if case.name == 'wide-conditioner':
        b = Bare(dev, f, target, z0, T, SEED)
        assert b.rc == hip.EUNSUPPORTED and torch.equal(b.z.cpu(), z0)
    s = case.sampler(T, (f, of), target)
    s.seed = SEED
    assert (s._closed_form() is not None) == case.closed_form
    split = _spied(monkeypatch, s, through=True)
    if case.rounds == 7:
        with pytest.raises(hip.NfmcArgumentError, match='nfmc_mh_accept_select_f32') as refused:
            s.sample(z0, show_progress=False)
        assert split == [1] and refused.value.code == hip.EUNSUPPORTED and isinstance(refused.value, ValueError)
        return
    out = s.sample(z0, show_progress=False)
    assert split == [1]
    tr = cases.oracle(z0, of, ref, T, rounds=case.rounds)
    _states(out.samples.reshape(T, N, d), tr, z0, of, ref, case.name)


# ------------------------------------------------------------------------------------------------ 8. refusals
def _edits(dev):
    from nfmc_amd import hip
    keep = {'nz': torch.zeros(T, N, 5, device=dev), 'un': torch.full((T, N), 0.5, device=dev)}

    def field(path, value):
        def edit(a):
            obj = a
            for name in path[:-1]:
                obj = getattr(obj, name)
            setattr(obj, path[-1], value)
        return edit

    def two(*edits):
        return lambda a: [e(a) for e in edits]
    return keep, [
        ('deferred statistics', field(('stats', 'defer'), 1), hip.EUNSUPPORTED),
        ('philox-7', field(('rng', 'rounds'), 7), hip.EUNSUPPORTED),
        ('unknown rounds', field(('rng', 'rounds'), 5), hip.EINVAL),
        ('flow without its affine', field(('flow', 'ea0_shift'), None), hip.EINVAL),
        ('d beyond 512', field(('flow', 'd'), 513), hip.ESHAPE),
        ('conditioner of 40', field(('flow', 'n_hidden'), 40), hip.EUNSUPPORTED),
        ('no state', field(('z',), None), hip.EINVAL),
        ('no chains', field(('n',), 0), hip.EINVAL),
        ('no steps', field(('n_steps',), 0), hip.EINVAL),
        ('too many steps', field(('n_steps',), hip.MAX_STEPS_PER_CALL + 1), hip.ESHAPE),
        ('a kind outside the family', field(('pot', 'kind'), hip.POT_GAUSSIAN_MIXTURE), hip.EUNSUPPORTED),
        ('an unknown kind', field(('pot', 'kind'), 99), hip.EUNSUPPORTED),
        ('statistics without their second moment', field(('stats', 'sum_x2'), None), hip.EINVAL),
        ('replayed normals without uniforms', field(('rng', 'replay_normals'), hip.ptr(keep['nz'])), hip.EINVAL),
        ('replayed uniforms without normals', field(('rng', 'replay_uniforms'), hip.ptr(keep['un'])), hip.EINVAL),
        ('a store of stride 0', field(('samples', 'stride'), 0), hip.EINVAL),
        ('statistics scratch too small', field(('stats', 'scratch_bytes'), 8), hip.ESCRATCH),
    ]


def test_malformed_calls_are_refused_and_write_nothing(dev):
    from nfmc_amd import hip
    d = 5
    pot, _ref = cases.sum_of_squares(d)
    f, _of = cases.flows(d, 'realnvp', 8)
    z0 = cases.starts(N, d)
    assert int(hip.lib().nfmc_neutra_mh_steps_f32(None, hip.stream())) == hip.EINVAL
    keep, edits = _edits(dev)
    for what, edit, code in edits:
        b = Bare(dev, f, pot, z0, T, SEED, edit=edit, stats=True)
        assert b.rc == code, (what, b.rc, code)
        assert torch.equal(b.z.cpu(), z0), what
        assert not bool(b.kept.any()) and not bool(b.m.any()) and not bool(b.lr.any()), what
    ok = Bare(dev, f, pot, z0, T, SEED, stats=True)
    assert ok.rc == hip.OK and not torch.equal(ok.z.cpu(), z0)
