"""The register-lean forms of the flow-MH kernel (csrc/flow_b_lean.hip), which the jump of a split whole-run call is
launched on, compute bit for bit what the kernels of a call without parts compute.

The existing route is nfmc_flow_mh_steps_f32 as it stands; the lean route is the same call under NFMC_FLOWB_LEAN=1 (the
switch that sends a call without a part to the lean form too), and nfmc_jump_run_f32 with two parts.  The lean forms are
the same per-chain operations under an occupancy bound, so every array is compared for EQUALITY: states, log q, the
accept masks and log ratios of the diagnostic instantiation, the accept counters and the moment sums.

Shapes, the smallest that reach every path: d = 64 with H = 4 on the (8, 8) layout and d = 256 with H = 8 on the
(8, 32) layout (the benchmark's C3 / C5 jump; NFMC_FLOWB_CFG pins the layout, which would otherwise follow the chain
count); n = 1 (one active lane group), 37 (inactive lanes, an odd count for the two-chain kernel that the d = 256 call
without diagnostics runs on today), 96, and two workgroup tiles + 5 chains (a partial last tile); 1 and 3 transitions per
call; adjusted and unadjusted; both generator round counts; chain_offset = 977.  The whole-run cases have 2 x 16384
chains at d = 64, where no workgroup strides over tiles, so that the moments are equal too.

Only the (8, 8) layout at H = 4 has a lean form (no form shortened the C5 step): at d = 256 the switch
must leave the call on the kernels it runs on today, one-chain with diagnostics and two-chain without, which the same
comparisons assert."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CHAIN_OFFSET = 977
# d, H, layout, chains per workgroup tile (4 waves x 64 / LPC chains)
SHAPES = {64: (4, '8,8', 32), 256: (8, '8,32', 8)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


_flows = {}


def _flow(d):
    """RealNVP with perturbed weights (jumps are accepted and rejected); one per d, read-only."""
    from nfmc_amd.flows import Flow, RealNVP
    from oracle import flow as oflow
    if d not in _flows:
        ck = {'n_hidden': SHAPES[d][0]}
        torch.manual_seed(23 + d)
        # the wider flow is perturbed less: the acceptance rate falls with d
        of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,), conditioner_kwargs=ck)), 5, 0.2 if d == 64 else 0.05, 0.7071)
        f = Flow(RealNVP((d,), conditioner_kwargs=ck))
        f.load_state_dict(of.state_dict())
        assert f.bijection.n_hidden == SHAPES[d][0]
        _flows[d] = f
    return _flows[d]


def _x0(n, d):
    return 0.7 * torch.randn(n, d, generator=torch.Generator().manual_seed(1000 * d + n))


def _direct(monkeypatch, dev, d, n, k, adjusted, rounds, lean, diag):
    """k flow-MH transitions by one nfmc_flow_mh_steps_f32 call; every output as CPU tensors."""
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import imh, jump
    from nfmc_amd.samplers.common import Run
    monkeypatch.setenv('NFMC_FLOWB_CFG', SHAPES[d][1])
    monkeypatch.setenv('NFMC_FLOWB_LEAN', '1' if lean else '0')
    f, pot = _flow(d), SumOfSquares((d,))
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=k, store_samples=False))
    s.seed, s.rng_rounds = 4242, rounds
    run = Run(s, _x0(n, d))
    run.chain_offset = CHAIN_OFFSET
    logq = torch.zeros(n, dtype=torch.float32, device=dev)
    masks = torch.zeros(k, n, dtype=torch.uint8, device=dev) if diag else None
    lr = torch.zeros(k, n, dtype=torch.float32, device=dev) if diag else None
    assert jump.flow_mh_supported(run, f, pot, logq, adjusted)
    jump.launch_flow_mh(run, f, pot, logq, k, 5, False, adjusted, run.stats.struct(), None, masks, lr)
    sum_x, sum_x2, cnt, jc = run.stats.host_totals()
    out = {'x': run.x.cpu(), 'logq': logq.cpu(), 'sum_x': sum_x.clone(), 'sum_x2': sum_x2.clone(), 'cnt': cnt.clone(),
           'jc': jc.clone()}
    if diag:
        out.update(masks=masks.cpu(), lr=lr.cpu())
    return out


@pytest.mark.parametrize('rounds', (10, 7))
@pytest.mark.parametrize('adjusted', (True, False))
@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('n_kind', ('one', '37', '96', 'tiles'))
@pytest.mark.parametrize('d', (64, 256))
def test_lean_form_equals_the_existing_kernels(dev, monkeypatch, d, n_kind, k, adjusted, rounds):
    from nfmc_amd import hip
    n = {'one': 1, '37': 37, '96': 96, 'tiles': 2 * SHAPES[d][2] + 5}[n_kind]
    got = {(lean, diag): _direct(monkeypatch, dev, d, n, k, adjusted, rounds, lean, diag)
           for lean in (False, True) for diag in (False, True)}
    want = got[False, True]
    n_acc = int(want['masks'].sum())
    assert int(want['cnt'][hip.CNT_ACCEPTED]) == n_acc
    assert n_acc == n * k if not adjusted else n_acc < n * k or n * k < 37
    assert torch.isfinite(want['lr']).all() and torch.isfinite(want['x']).all()
    for diag in (False, True):   # the lean route against the existing one, call for call: every array
        for name in got[True, diag]:
            assert torch.equal(got[True, diag][name], got[False, diag][name]), (diag, name)
    # with and without the diagnostics compiled in: the same chains.  (Not at d = 256: there the call without diagnostics
    # runs today's two-chain kernel, another kernel than the one-chain kernel with diagnostics, on either route; their
    # states and counters came out equal and their log q differed in the last bits at n = 96, on the parent's library too.)
    for name in ('x', 'cnt', 'jc') + (('logq', 'sum_x', 'sum_x2') if d == 64 else ()):
        assert torch.equal(got[True, False][name], want[name]), name


@pytest.mark.parametrize('d', (64, 256))
def test_the_cases_accept_and_reject(dev, monkeypatch, d):
    """The comparisons above are not between runs that reject (or take) every proposal."""
    from nfmc_amd import hip
    n, k = 96, 3
    got = _direct(monkeypatch, dev, d, n, k, True, 10, False, True)
    n_acc = int(got['cnt'][hip.CNT_ACCEPTED])
    print('accepted', n_acc, 'of', n * k)
    assert 0 < n_acc < n * k


_runs = {}


def _whole_run(kind, parts, d=64, n=2 * 16384, k=3, t=3):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import jump, mcmc
    if (kind, parts) in _runs:
        return _runs[kind, parts]
    pot = SumOfSquares((d,))
    params = jump.JumpNFMCParameters(n_iterations=t, store_samples=False)
    kern = NFMCKernel((d,), flow=_flow(d))
    if kind == 'jump_hmc':
        s = jump.JumpHMC((d,), pot, kern, params, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=3, step_size=0.4),
                         mcmc.HMCParameters(n_iterations=k))
    else:
        s = jump.JumpMALA((d,), pot, kern, params, None, mcmc.LangevinParameters(n_iterations=k))
    s.seed = 424242
    s.jump_parts = parts
    out = s.sample(_x0(n, d), show_progress=False)
    st = out.statistics
    _runs[kind, parts] = {
        'x': out.running_samples.last_sample.clone(),
        'counters': {c: getattr(st, c) for c in ('n_accepted_trajectories', 'n_attempted_trajectories', 'n_accepted_jumps',
                                                  'n_attempted_jumps', 'n_nonfinite_log_ratios')},
        'sum_x': st.expectations['first_moment'].total.clone(),
        'sum_x2': st.expectations['second_moment'].total.clone(),
        'n_seen': st.expectations['first_moment'].n_seen}
    return _runs[kind, parts]


@pytest.mark.parametrize('kind', ('jump_mala', 'jump_hmc'))
def test_whole_run_with_two_parts_equals_one_part(dev, monkeypatch, kind):
    """Two parts launch the jump on the lean form from iteration 1 on; one part launches the kernels of the unsplit run."""
    monkeypatch.delenv('NFMC_FLOWB_LEAN', raising=False)
    monkeypatch.delenv('NFMC_FLOWB_CFG', raising=False)
    n, k, t = 2 * 16384, 3, 3
    want, got = _whole_run(kind, 1), _whole_run(kind, 2)
    c = want['counters']
    assert c['n_attempted_jumps'] == n * t and 0 < c['n_accepted_jumps'] < n * t
    assert c['n_attempted_trajectories'] == n * t * k and want['n_seen'] == n * t * (k + 1)
    assert torch.equal(got['x'], want['x'])
    assert got['counters'] == want['counters'] and got['n_seen'] == want['n_seen']
    assert torch.equal(got['sum_x'], want['sum_x']) and torch.equal(got['sum_x2'], want['sum_x2'])
