"""The whole-run call of the jump samplers (nfmc_jump_run_f32; samplers/jump.py: launch_jump_run): a run split into parts of
chains on streams of their own computes, chain for chain, what the unsplit run and the host loop compute.

Shapes are the smallest at which the split can go wrong: d = 6 (a lane group narrower than its layout) and d = 64 (the
benchmark's layout); n = 1000 (a ragged last part that is no whole tile of either kernel), n = 70 (with 4 parts the last
ones are empty or one partial tile), n = 4096; K = 3 inner transitions and T = 4 outer iterations, and once K = 513, one
above the per-call step limit, so that a chunk boundary falls inside an iteration.

Moments: the parts write the same per-workgroup partial sums into other slabs of the statistics scratch (no shape here has
more tiles than a part may have workgroups), and the fold adds the slabs in slab order: at most 2048 fp64 additions of
partials of O(n T K) magnitude in another order, each with a relative rounding error of 2^-53 = 1.1e-16.  Hence the bound of
1e-12 on the relative difference of every sum; it is not a measured figure (measured: 0.0 in every case)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, K = 4, 3
MOMENT_RTOL = 1e-12
COUNTERS = ('n_accepted_trajectories', 'n_attempted_trajectories', 'n_accepted_jumps', 'n_attempted_jumps',
            'n_nonfinite_log_ratios', 'n_divergences', 'n_target_calls', 'n_target_gradient_calls')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


_flows = {}


def _flow(d):
    """The package's RealNVP with perturbed weights (jumps are accepted and rejected); one per d, read-only."""
    from nfmc_amd.flows import Flow, RealNVP
    from oracle import flow as oflow
    if d not in _flows:
        torch.manual_seed(11 + d)
        of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,))), 5, 0.2, 0.7071)
        f = Flow(RealNVP((d,)))
        f.load_state_dict(of.state_dict())
        _flows[d] = f
    return _flows[d]


def _x0(n, d):
    return 0.7 * torch.randn(n, d, generator=torch.Generator().manual_seed(1000 * d + n))


def _sampler(kind, target, d, k=K, t=T, parts=None, legacy=False, shard=None):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.potentials import Funnel, SumOfSquares
    from nfmc_amd.samplers import jump, mcmc
    pot = Funnel((d,), 3.0) if target == 'funnel' else SumOfSquares((d,))
    params = jump.JumpNFMCParameters(n_iterations=t, store_samples=False)
    kern = NFMCKernel((d,), flow=_flow(d))
    if kind == 'jump_hmc':
        s = jump.JumpHMC((d,), pot, kern, params, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=3, step_size=0.4),
                         mcmc.HMCParameters(n_iterations=k))
    else:
        s = jump.JumpMALA((d,), pot, kern, params, None, mcmc.LangevinParameters(n_iterations=k))
    s.seed = 424242
    s.jump_parts = parts
    s.shard = shard
    if legacy:
        s.time_kernels = True   # per-launch events: one of the conditions that keep the host loop
    return s


def _result(out):
    st = out.statistics
    return {'x': out.running_samples.last_sample.clone(),
            'counters': {c: getattr(st, c) for c in COUNTERS},
            'sum_x': st.expectations['first_moment'].total.clone(),
            'sum_x2': st.expectations['second_moment'].total.clone(),
            'n_seen': st.expectations['first_moment'].n_seen}


_runs = {}


def _run(kind, target, d, n, k=K, parts=1, legacy=False):
    """One run per (case, parts), computed once and shared by the tests that compare against it."""
    key = (kind, target, d, n, k, parts, legacy)
    if key not in _runs:
        out = _sampler(kind, target, d, k=k, parts=parts, legacy=legacy).sample(_x0(n, d), show_progress=False)
        _runs[key] = _result(out)
    return _runs[key]


def _spy_driver(monkeypatch):
    """Counts the whole-run calls and records their parts."""
    from nfmc_amd.samplers import jump
    calls = []
    real = jump.launch_jump_run

    def spy(run, inner, flow, pot, logq, step0, n_outer, n_inner, n_parts, adjusted):
        calls.append((n_outer, n_inner, n_parts))
        return real(run, inner, flow, pot, logq, step0, n_outer, n_inner, n_parts, adjusted)
    monkeypatch.setattr(jump, 'launch_jump_run', spy)
    return calls


def _rel(a, b):
    return float(((a - b).abs() / b.abs()).max())


def _assert_same_run(got, want, moments_bitwise=False):
    assert torch.equal(got['x'], want['x'])
    assert got['counters'] == want['counters']
    assert got['n_seen'] == want['n_seen']
    for name in ('sum_x', 'sum_x2'):
        if moments_bitwise:
            assert torch.equal(got[name], want[name]), name
        else:
            rel = _rel(got[name], want[name])
            print(name, 'relative difference', rel)
            assert rel <= MOMENT_RTOL, (name, rel)


CASES = [(kind, target, d, n)
         for kind, target in (('jump_mala', 'sumsq'), ('jump_hmc', 'sumsq'), ('jump_mala', 'funnel'))
         for d in (6, 64) for n in (1000, 70, 4096)]


@pytest.mark.parametrize('kind,target,d,n', CASES)
@pytest.mark.parametrize('parts', (2, 4))
def test_parts_match_the_unsplit_run(dev, monkeypatch, kind, target, d, n, parts):
    want = _run(kind, target, d, n, parts=1)
    calls = _spy_driver(monkeypatch)
    got = _run(kind, target, d, n, parts=parts)
    assert calls in ([], [(T - 1, K, parts)])          # [] when another test computed this run before
    c = want['counters']
    assert c['n_attempted_trajectories'] == n * T * K and c['n_attempted_jumps'] == n * T
    assert 0 < c['n_accepted_trajectories'] < n * T * K and want['n_seen'] == n * T * (K + 1)
    _assert_same_run(got, want)


@pytest.mark.parametrize('parts', (2, 4))
def test_chunk_boundary_inside_an_iteration(dev, parts):
    """K = 513, one above the per-call step limit: every iteration is a launch of 512 and a launch of 1 transition."""
    from nfmc_amd import hip
    k = hip.MAX_STEPS_PER_CALL + 1
    want = _run('jump_mala', 'sumsq', 6, 70, k=k, parts=1)
    assert want['counters']['n_attempted_trajectories'] == 70 * T * k
    _assert_same_run(_run('jump_mala', 'sumsq', 6, 70, k=k, parts=parts), want)
    _assert_same_run(want, _run('jump_mala', 'sumsq', 6, 70, k=k, legacy=True), moments_bitwise=True)


@pytest.mark.parametrize('kind,target,d,n', [c for c in CASES if c[3] == 1000])
def test_one_part_is_the_host_loop(dev, monkeypatch, kind, target, d, n):
    """jump_parts = 1 issues the launches of the loop in JumpNFMC.sample: everything equal, the moments bit for bit."""
    calls = _spy_driver(monkeypatch)
    legacy = _run(kind, target, d, n, legacy=True)
    assert calls == []
    _assert_same_run(_run(kind, target, d, n, parts=1), legacy, moments_bitwise=True)


def test_sharded_run_keeps_global_chain_ids(dev):
    from nfmc_amd.dist import Shard
    d, n = 64, 1000
    full = _run('jump_mala', 'sumsq', d, n, parts=1)
    sh = Shard(rank=1, world=3)
    sh.merge_statistics = lambda st: st
    lo, hi = sh.bounds(n)
    assert lo != 0
    out = _sampler('jump_mala', 'sumsq', d, parts=2, shard=sh).sample(_x0(n, d), show_progress=False)
    assert torch.equal(out.running_samples.last_sample, full['x'][lo:hi])


def test_two_calls_in_a_row_are_bitwise_equal(dev):
    """A side stream still running when the call returns, or a slab that a fold left unzeroed, would show here."""
    d, n = 64, 4096
    s = _sampler('jump_mala', 'sumsq', d, parts=4)
    a = _result(s.sample(_x0(n, d), show_progress=False))
    b = _result(s.sample(_x0(n, d), show_progress=False))
    _assert_same_run(b, a, moments_bitwise=True)
    _assert_same_run(a, _run('jump_mala', 'sumsq', d, n, parts=4), moments_bitwise=True)


def test_the_call_is_ordered_on_the_callers_stream(dev):
    """A torch op on the states right behind the call, with no synchronise in between, sees the final states."""
    from nfmc_amd.samplers import jump
    from nfmc_amd.samplers.common import Run
    d, n, k, t = 64, 4096, 50, 4
    got = {}
    for parts in (4, 1):
        s = _sampler('jump_mala', 'sumsq', d, k=k, t=t, parts=parts)
        run = Run(s, _x0(n, d))
        logq = torch.empty(n, dtype=torch.float32, device=run.dev)
        torch.cuda.synchronize()
        jump.launch_jump_run(run, s.inner_sampler, s.kernel.flow, s.target, logq, 0, t, k, parts, True)
        got[parts] = run.x.clone()          # on the caller's stream, behind the join
        torch.cuda.synchronize()
        assert torch.equal(got[parts], run.x)
    assert torch.equal(got[4], got[1])


def test_arguments_the_call_refuses(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import jump
    from nfmc_amd.samplers.common import Run
    s = _sampler('jump_mala', 'sumsq', 6)
    run = Run(s, _x0(70, 6))
    logq = torch.empty(70, dtype=torch.float32, device=run.dev)
    for bad in (0, hip.JUMP_RUN_MAX_PARTS + 1):
        with pytest.raises(hip.NfmcArgumentError):
            jump.launch_jump_run(run, s.inner_sampler, s.kernel.flow, s.target, logq, 0, T, K, bad, True)
    with pytest.raises(ValueError):
        _sampler('jump_mala', 'sumsq', 6, parts=5).sample(_x0(70, 6), show_progress=False)
