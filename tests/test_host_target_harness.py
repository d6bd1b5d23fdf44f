"""CPU: tests/target_harness.py's own comparisons.  Ten GPU test files trust compare_states, compare_decisions and Spy: a
bug there silences all of them, so each is shown here to pass on the oracle's own output and to fail on every kind of
error it exists to catch.  The trace is a real one: oracle.samplers.mcmc_sample, MALA on a standard normal (d = 4, 64
chains, 3 transitions) with PhiloxNoise; the flow-proposal comparison (compare_flow_mh) has imh_sample traces of its own
below, and the last test runs the inputs of every flow-MH case of the GPU files through the fp64 oracle alone."""
import copy
import ctypes
import functools

import pytest
import torch

import target_harness as H

D, N, T = 4, 64, 3
MARGIN, ATOL, RTOL = 2e-3, 1e-3, 1e-4


def _u(x):
    return 0.5 * (x ** 2).sum(-1)


@functools.lru_cache(maxsize=None)
def _case():
    """(x0 fp32, oracle Trace), computed once; the tests copy what they change"""
    from oracle import samplers as osamp
    x0 = torch.randn(N, D, generator=torch.Generator().manual_seed(1))
    tr = osamp.mcmc_sample(x0.double(), _u, 'langevin', T, 0.8, adjustment=True, noise=osamp.PhiloxNoise(7, dtype=torch.float64))
    assert 0 < tr.n_accepted < N * T                       # both decisions occur
    return x0, tr


class _Rec:
    """stands for the kernel's Record: the masks and log ratios given"""

    def __init__(self, masks, log_ratios):
        self.m, self.lr = masks, log_ratios

    def stacked(self):
        return self.m, self.lr


def _oracle_rec(tr):
    return _Rec(torch.stack([m.reshape(-1).bool() for m in tr.masks]),
                torch.stack([v.reshape(-1).float() for v in tr.log_ratios]))


def _states(got, tr, margin=MARGIN):
    return H.compare_states(got, tr, 'host', margin=margin, atol=ATOL, rtol=RTOL)


def _tol(d, want_lr, mag):
    return 2e-4 * max(1.0, d / 64) + 1e-4 * abs(want_lr) + 8 * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------------ states
def test_states_pass_on_the_oracles_own():
    _x0, tr = _case()
    keep = _states(tr.stacked().float(), tr)
    assert keep.dtype == torch.bool and keep.shape == (N,) and bool(keep.any())


def test_states_fail_on_one_moved_coordinate_of_a_kept_chain():
    _x0, tr = _case()
    got = tr.stacked().float()
    chain = int(torch.nonzero(_states(got, tr))[0])
    got[1, chain, 2] += 2 * (ATOL + RTOL * float(got[1, chain, 2].abs()))
    with pytest.raises(AssertionError):
        _states(got, tr)


def test_states_fail_on_a_nan():
    _x0, tr = _case()
    got = tr.stacked().float()
    got[0, 0, 0] = float('nan')
    with pytest.raises(AssertionError):
        _states(got, tr)


def test_states_fail_when_the_excluded_share_reaches_the_cap():
    _x0, tr = _case()
    with pytest.raises(AssertionError):
        _states(tr.stacked().float(), tr, margin=1e3)          # every chain a near-tie


# --------------------------------------------------------------------------------------------- decisions
def test_decisions_pass_on_the_oracles_own():
    x0, tr = _case()
    H.compare_decisions(_oracle_rec(tr), tr, 'mala', x0, _u, 'host')
    H.compare_decisions(_oracle_rec(tr), tr, 'mala', x0, _u, 'host', skip_below_minus_50=True)


def test_decisions_fail_on_flipped_first_masks():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    rec.m = rec.m.clone()
    rec.m[0, :N // 8] ^= True                                  # 12.5 % of the chains disagree from the first transition on
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host')


def test_decisions_fail_on_one_log_ratio_off_by_twice_its_tolerance():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    want = float(tr.log_ratios[0].reshape(-1)[5])
    rec.lr = rec.lr.clone()
    rec.lr[0, 5] = want + 2 * _tol(D, want, float(_u(x0[5].double())))
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host')


def test_decisions_compare_rows_below_minus_50_unless_told_not_to():
    x0, tr = _case()
    tr = copy.deepcopy(tr)
    tr.log_ratios[0].reshape(-1)[5] = -60.0                    # fp64 says: rejected whatever the uniform
    tr.masks[0].reshape(-1)[5] = False
    rec = _oracle_rec(tr)
    rec.lr[0, 5] = -61.0                                       # the kernel's is off by far more than the tolerance
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host')
    H.compare_decisions(rec, tr, 'mala', x0, _u, 'host', skip_below_minus_50=True)


def test_decisions_use_the_magnitude_given():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    want = float(tr.log_ratios[0].reshape(-1)[5])
    rec.lr = rec.lr.clone()
    rec.lr[0, 5] = want + 2 * _tol(D, want, float(_u(x0[5].double())))
    H.compare_decisions(rec, tr, 'mala', x0, _u, 'host', mag=lambda prev: _u(prev).abs() + 1e5)


def test_unadjusted_decisions_fail_on_a_rejection():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    rec.m = torch.ones_like(rec.m)
    H.compare_decisions(rec, tr, 'ula', x0, _u, 'host')
    rec.m[1, 3] = False
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'ula', x0, _u, 'host')


# --------------------------------------------------------------------------------------------------- spy
def test_spy_counts_a_call_through_a_subclass_with_its_own_split_step(monkeypatch):
    from nfmc_amd.samplers import mcmc
    monkeypatch.setattr(mcmc.MALA, '_split_step', lambda self, *a, **k: 'ran', raising=False)   # as an earlier test may leave it
    spy = H.Spy(monkeypatch)
    assert mcmc.MALA._split_step(object()) == 'ran'
    assert spy.calls == [1]


# ------------------------------------------------------------------------- the flow-proposal Metropolis comparison
FD, FN, FT = 6, 96, 4


class _Normal:
    """the harness's Problem, standard normal scaled per coordinate: U = sum (x / sd)^2 / 2"""

    def __init__(self, d):
        self.d, self.name, self.pot = d, 'normal d=%d' % d, None
        self.sd = torch.linspace(0.5, 2.0, d, dtype=torch.float64)
        self.mean = torch.linspace(-3.0, 3.0, d, dtype=torch.float64)
        self.target = self.ref = lambda x: 0.5 * (((x - self.mean) / self.sd) ** 2).sum(-1)
        self.x0 = torch.randn(FN, d, generator=torch.Generator().manual_seed(2))


@functools.lru_cache(maxsize=None)
def _flow_case(centred=True, spline=False):
    """(problem, oracle flow, imh_sample Trace) on the CPU; centred: a centred flow and starts, else flow_pair's about the
    origin, whose proposals this target (means up to 3, scales down to 0.5) hardly ever takes from its own draws"""
    from oracle import samplers as osamp
    p = _Normal(FD)
    if centred:
        _f, of = H.centred_flow_pair(p, 3, spline=spline, scale=0.2)
        p = H.centred(p, FN, 5)
    else:
        _f, of = H.flow_pair(FD, 3, spline=spline)
        p = H.with_starts(p, (p.mean + p.sd * p.x0.double()).float())     # draws of the target: nothing to gain by moving
    tr = osamp.imh_sample(p.x0.double(), p.target, of, FT, noise=osamp.PhiloxNoise(11, dtype=torch.float64))
    return p, of, tr


def _flow_rec(tr):
    return (torch.stack([js.mask.reshape(-1) for js in tr.flow_steps]),
            torch.stack([js.log_alpha.reshape(-1).float() for js in tr.flow_steps]))


def _flow_cmp(m, lr, tr, **kw):
    kw.setdefault('floor', 0.05)
    return H.compare_flow_mh(m, lr, tr.flow_steps, 'host', c=H.affine_c(FD), margin=MARGIN, skip_below_minus_50=False, **kw)


def test_laplace_fit_finds_the_mode_and_the_marginal_scales():
    p = _Normal(FD)
    c, s = H.laplace_fit(p)
    torch.testing.assert_close(c, p.mean, atol=1e-5, rtol=0)          # LBFGS stops at a gradient of 1e-10 or a step of 1e-14
    torch.testing.assert_close(s, p.sd, atol=1e-8, rtol=0)


def test_centred_flow_maps_the_mode_to_its_perturbation_alone():
    """z = (x - c) / s plus the perturbation: the first layer sends c to its perturbed shift, at most scale in size, and
    the package flow and the oracle flow hold the same fp32 numbers"""
    p = _Normal(FD)
    f, of = H.centred_flow_pair(p, 3, scale=0.2)
    first = of.bijection.layers[0]
    z0, _ = first.forward(p.mean[None])
    assert float(z0.detach().abs().max()) <= 0.2 and float((first.log_scale.detach() + p.sd.log()).abs().max()) <= 0.2
    for k, v in f.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v.double(), of.state_dict()[k]), k
    q = H.centred(p, FN, 5)
    assert q.x0.dtype == torch.float32 and q.x0.shape == (FN, FD) and p.x0 is not q.x0


def test_flow_mh_passes_on_the_oracles_own_and_centring_makes_it_accept():
    _p, _of, tr = _flow_case()
    m, lr = _flow_rec(tr)
    follows, ratio = _flow_cmp(m, lr, tr)
    assert bool(follows.all()) and ratio < 1e-2            # fp32 rounding of the oracle's own log ratios
    assert tr.n_accepted >= 0.3 * FN * FT
    assert _flow_case(centred=False)[2].n_accepted <= 0.02 * FN * FT


def test_flow_mh_fails_on_a_log_ratio_off_by_one_coordinates_term():
    """the kernel's log q(x') without the last coordinate's -z^2 / 2: what a dropped lane or tile row gives"""
    _p, of, tr = _flow_case()
    m, lr = _flow_rec(tr)
    js = tr.flow_steps[1]
    with torch.no_grad():
        z, _ = of.bijection.forward(js.x_prime)
    lr = lr.clone()
    lr[1] -= (0.5 * z[:, -1] ** 2).float()                 # -log q(x') loses +z^2 / 2
    with pytest.raises(AssertionError):
        _flow_cmp(m, lr, tr)
    lr2 = _flow_rec(tr)[1]
    lr2[1, 7] -= float(0.5 * z[7, -1] ** 2) + 1e-2         # one row alone
    with pytest.raises(AssertionError):
        _flow_cmp(m, lr2, tr)


def test_flow_mh_fails_on_one_rejection_the_oracle_accepts_by_a_wide_margin():
    _p, _of, tr = _flow_case()
    m, lr = _flow_rec(tr)
    js = tr.flow_steps[0]
    chain = int(torch.argmax(torch.where(js.mask, js.log_alpha - js.log_u, torch.full_like(js.log_u, -1.0))))
    assert float(js.log_alpha[chain] - js.log_u[chain]) > 0.5
    m = m.clone()
    m[0, chain] = False                                    # one row of 384: no share notices it
    with pytest.raises(AssertionError, match='clear of a tie'):
        _flow_cmp(m, lr, tr)


def test_flow_mh_fails_when_nothing_is_accepted_and_the_case_demands_the_floor():
    _p, _of, tr = _flow_case(centred=False)
    assert tr.n_accepted < 0.05 * FN * FT
    m, lr = _flow_rec(tr)
    with pytest.raises(AssertionError, match='acceptance'):
        H.compare_flow_mh(m, lr, tr.flow_steps, 'host', c=H.affine_c(FD), margin=MARGIN, skip_below_minus_50=True, floor=0.05)
    H.compare_flow_mh(m, lr, tr.flow_steps, 'host', c=H.affine_c(FD), margin=MARGIN, skip_below_minus_50=True)
    with pytest.raises(AssertionError, match='log ratio'):      # below -50 and not told to skip
        H.compare_flow_mh(m, lr, tr.flow_steps, 'host', c=H.affine_c(FD), margin=MARGIN, skip_below_minus_50=False)


def test_flow_mh_unadjusted_compares_every_row():
    from oracle import samplers as osamp
    p, of, _tr = _flow_case()
    tr = osamp.imh_sample(p.x0.double(), p.target, of, FT, noise=osamp.PhiloxNoise(11, dtype=torch.float64), adjusted=False)
    m, lr = _flow_rec(tr)
    assert bool(m.all())
    for js, kept in zip(tr.flow_steps, tr.samples):
        assert torch.equal(js.x_prime, kept)                   # every proposal kept
    assert torch.equal(tr.flow_steps[1].u_x, tr.flow_steps[0].u_xp) and torch.equal(tr.flow_steps[1].f_x, tr.flow_steps[0].f_xp)
    _flow_cmp(m, lr, tr, adjusted=False)
    lr[2, 3] += 0.01
    with pytest.raises(AssertionError):
        _flow_cmp(m, lr, tr, adjusted=False)
    m[1, 0] = False
    with pytest.raises(AssertionError):
        _flow_cmp(m, _flow_rec(tr)[1], tr, adjusted=False)


def test_flow_mh_tolerance_grows_with_the_four_magnitudes():
    _p, _of, tr = _flow_case()
    js = tr.flow_steps[0]
    tol = H.flow_mh_tolerance(tr.flow_steps, 1e-4)[0]
    want = 1e-4 + 2e-5 * js.log_alpha.abs() + 8 * 2.0 ** -24 * (js.u_x.abs() + js.u_xp.abs() + js.f_x.abs() + js.f_xp.abs())
    torch.testing.assert_close(tol, want, rtol=1e-12, atol=0)


def test_spline_constant_is_measured_on_the_fp32_oracle_and_never_under_the_affine_one():
    p, of, tr = _flow_case(spline=True)
    c, worst = H.spline_c(FD, of, tr.flow_steps)
    print('spline d=%d: fp32 oracle against fp64 %.2e, c = %.2e' % (FD, worst, c))
    assert 0 < worst < 1e-3 and c == max(H.affine_c(FD), H.SPLINE_C_FACTOR * worst)


def test_jump_rows_are_comparable_until_a_state_leaves_the_oracle():
    want = torch.zeros(6, 3, 2)                                # T = 2, Kin = 2
    got = want.clone()
    got[1, 1, 0] = 1.0                                         # chain 1 leaves at inner transition 1: no jump comparable
    got[2, 2, 0] = 1.0                                         # chain 2 at the first jump itself: that jump still is
    comparable = H.jump_comparable(got, want, 2, 1e-3, 1e-4)
    assert comparable.tolist() == [[True, False, True], [True, False, False]]


def test_flow_layout_is_the_launchers_rule():
    assert [H.flow_layout(d, 96) for d in (3, 7, 13, 25, 64, 100, 130, 500)] == \
        [(4, 1), (4, 2), (4, 4), (4, 8), (4, 16), (4, 32), (4, 64), (8, 64)]
    assert [H.flow_layout(d, 4160) for d in (25, 64, 100, 130)] == [(4, 8), (8, 8), (8, 16), (8, 32)]
    assert H.flow_layout(50, 96, (8, 8)) == (8, 8) and H.flow_layout(70, 96, (8, 8)) == (4, 32)


def test_hidden_layer_argument_sets_the_conditioners_depth_in_both_flows():
    """hidden_layers is conditioner_kwargs['n_layers'] (the NHL of the matrix-core kernels), n_layers stays the coupling
    count, and leaving it out keeps the architecture's two hidden layers"""
    p = _Normal(FD)
    for spline in (False, True):
        for make in (lambda **kw: H.flow_pair(FD, 3, spline=spline, **kw), lambda **kw: H.centred_flow_pair(p, 3, spline=spline, scale=0.1, **kw)):
            f, of = make(n_hidden=5, n_layers=3, hidden_layers=1)
            assert (f.bijection.n_hidden_layers, f.bijection.n_hidden, f.bijection.n_coupling) == (1, 5, 3)
            assert len(f.bijection.couplings[0].conditioner) == 2 and len(f.state_dict()) == len(of.state_dict())
            for k, v in f.state_dict().items():
                assert torch.equal(v.double(), of.state_dict()[k].double()), k
            f2, _of2 = make(n_hidden=5, n_layers=3)
            assert f2.bijection.n_hidden_layers == 2 and len(f2.bijection.couplings[0].conditioner) == 3


def test_direct_flow_mh_options_reach_the_launch(monkeypatch):
    """_direct_flow_mh on a stand-in for the run and the launch (no GPU): `cached` arrives as the logq buffer with the
    cached flag, `replay` as the sampler's replay, stats='deferred' asks struct(defer=True, attempted=n T) and returns the
    folded totals, `store` hands the launch a DeviceSampleStore of T offered transitions whose kept rows come back in
    order, `prefill` fills the statistics scratch, and without options the three-tuple of before is returned."""
    from nfmc_amd import hip
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import common, jump
    n, d, steps = 5, FD, 7
    cpu = torch.device('cpu')
    seen = {}

    class Stats:
        scratch = torch.zeros(16, dtype=torch.float64)

        def struct(self, defer=False, attempted=0):
            seen['struct'] = (defer, attempted)
            return 'stats'

        def host_totals(self):
            cnt = torch.zeros(8, dtype=torch.int64)
            cnt[hip.CNT_ACCEPTED], cnt[hip.CNT_ATTEMPTED], cnt[hip.CNT_NONFINITE] = 11, n * steps, 2
            return torch.full((d,), 3.0, dtype=torch.float64), torch.full((d,), 4.0, dtype=torch.float64), cnt, cnt.clone()

    class Run:
        def __init__(self, sampler, x0):
            self.n, self.d, self.dev, self.stats = x0.shape[0], x0.shape[1], cpu, Stats()
            self.x = x0.clone()
            seen['replay'], seen['seed'] = sampler.replay, sampler.seed

    def launch(run, flow, pot, logq, k, step0, cached, adjusted, stats_struct, samples, masks_out, log_ratio_out):
        seen.update(logq=logq.clone(), k=k, cached=cached, adjusted=adjusted, stats=stats_struct, samples=samples)
        dense = torch.arange(k, dtype=torch.float32)[:, None, None].expand(k, run.n, run.d).contiguous()
        if hasattr(samples, 'add_dense'):
            samples.add_dense(dense)
        else:
            samples.copy_(dense)
        masks_out.fill_(1)
        log_ratio_out.fill_(0.5)
        logq.fill_(-1.0)
        run.x.fill_(float(k - 1))

    monkeypatch.setattr(common, 'Run', Run)
    monkeypatch.setattr(jump, 'flow_mh_supported', lambda *a, **k: True)
    monkeypatch.setattr(jump, 'launch_flow_mh', launch)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    f, _of = H.flow_pair(FD, 3)
    p = H.Problem(SumOfSquares((d,)), _u, _u, torch.zeros(n, d), d, 'stand-in')
    plain = H._direct_flow_mh(cpu, p, f, steps, 9, False)
    assert isinstance(plain, tuple) and len(plain) == 3 and plain[0].shape == (steps, n, d) and plain[1].dtype == torch.bool
    assert seen['seed'] == 9 and seen['replay'] is None and (seen['cached'], seen['adjusted'], seen['k']) == (False, False, steps)
    assert seen['struct'] == (False, 0) and seen['stats'] == 'stats'
    lq = torch.linspace(-3.0, -1.0, n)
    normals, uniforms = torch.randn(steps, n, d, dtype=torch.float64), torch.rand(steps, n, dtype=torch.float64)
    r = H._direct_flow_mh(cpu, p, f, steps, 9, True, cached=lq, replay=(normals, uniforms), stats='deferred', store=(3, 2))
    assert isinstance(r, H.DirectRun) and seen['cached'] is True and torch.equal(seen['logq'], lq)
    assert torch.equal(seen['replay'][0], normals.float()) and torch.equal(seen['replay'][1], uniforms.float())
    assert seen['struct'] == (True, n * steps)
    store = seen['samples']
    assert (store.thinning, store.rows, store.seen) == (3, 2, steps)
    assert r.samples.shape == (2, n, d) and r.samples[:, 0, 0].tolist() == [3.0, 6.0]          # transitions 0, 3, 6: the last two
    assert bool(r.masks.all()) and bool((r.log_ratios == 0.5).all()) and bool((r.logq == -1.0).all()) and bool((r.x == steps - 1).all())
    assert (r.stats['accepted'], r.stats['attempted'], r.stats['nonfinite']) == (11, n * steps, 2)
    assert bool((r.stats['sum_x'] == 3.0).all()) and bool((r.stats['sum_x2'] == 4.0).all())
    r = H._direct_flow_mh(cpu, p, f, steps, 9, True, replay=(normals, None), stats='immediate')
    assert seen['replay'][1] is None and seen['struct'] == (False, 0) and r.samples.shape == (steps, n, d) and r.stats['accepted'] == 11
    assert H._direct_flow_mh(cpu, p, f, steps, 9, True, detail=True).stats is None
    assert not bool(Stats.scratch.any())
    H._direct_flow_mh(cpu, p, f, steps, 9, True, stats='deferred', prefill=1.0)
    assert bool((Stats.scratch == 1.0).all())


FLOW_FILES = ['fullrank', 'gmrf', 'latent_gaussian', 'logreg', 'mixture', 'phi4', 'irt', 'varying_effects', 'rosenbrock', 'sv',
              'sparse_logreg', 'particles']


@pytest.mark.parametrize('name', FLOW_FILES)
def test_the_flow_mh_cases_of_a_gpu_file_hold_their_input_conditions_on_the_oracle_alone(monkeypatch, name, capsys):
    """Every case of the tests a GPU file lists in FLOW_TESTS, run on the CPU up to the conditions on its inputs: at least
    5 % of the proposals accepted at capacities up to 128, under 10 % of the chains near a tie, every compared log ratio
    finite and above -50 unless the case says skip_below_minus_50.  The printed lines are where the figures in the
    files' docstrings come from."""
    import importlib
    module = importlib.import_module('test_gpu_' + name)
    count = H.probe_flow_inputs(module, monkeypatch)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if 'oracle accepts' in ln or 'unadjusted' in ln]
    acc = [float(ln.split('oracle accepts ')[1].split()[0]) for ln in lines if 'oracle accepts' in ln]
    assert count >= len(getattr(module, 'FLOW_CASES', ())) and len(lines) >= count
    print('%s: %d cases, oracle acceptance %.3f .. %.3f' % (name, count, min(acc), max(acc)))


# ------------------------------------------------------------- the NeuTra-HMC comparisons (test_gpu_neutra_hmc_wide.py)
ND, NN, NT, NL, NH_STEP = 8, 48, 3, 2, 0.55


@functools.lru_cache(maxsize=None)
def _neutra_case():
    """(problem at its latent starts, oracle flow, fp64 trace, fp32 trace) of a small NeuTra-HMC run on U = sum x^2"""
    from nfmc_amd.potentials import SumOfSquares
    from oracle import potentials as opot
    z0 = 0.5 * torch.randn(NN, ND, generator=torch.Generator().manual_seed(4))
    p = H.Problem(SumOfSquares((ND,)), opot.sum_squares, opot.sum_squares, z0, ND, 'host neutra')
    centre = (torch.zeros(ND, dtype=torch.float64), torch.ones(ND, dtype=torch.float64))
    _f, of = H.centred_flow_pair(p, 5, 8, False, 3, scale=0.1, centre=centre, hidden_layers=1)
    tr = H.neutra_hmc_oracle(p, of, NT, NL, NH_STEP, 9)
    tr32 = H.neutra_hmc_oracle(p, of, NT, NL, NH_STEP, 9, dtype=torch.float32)
    assert 0 < tr.n_accepted < NN * NT
    return p, of, tr, tr32


def _neutra_run(tr, **changed):
    """the oracle's own output as a NeutraRun, with the fields given replaced"""
    kept = tr.stacked().float()
    run = H.NeutraRun(0, kept, torch.stack([m.reshape(-1).bool() for m in tr.masks]),
                      torch.stack([v.reshape(-1).float() for v in tr.log_ratios]) if tr.log_ratios else torch.zeros(NT, NN), kept[-1].clone(), None, 0)
    return run._replace(**changed)


def _neutra_compare(run, tr, adjust=True):
    p, of, _tr, _tr32 = _neutra_case()
    return H.compare_neutra_hmc(run, tr, p, of, 'host neutra', atol=1e-5, lr_figure=1e-6, adjust=adjust)


def test_neutra_figures_measure_the_fp32_oracle():
    """both figures are positive and of the size of fp32 rounding; a trace against itself gives zero; a decision that
    differs ends a chain's rows, so that its later states do not count"""
    _p, _of, tr, tr32 = _neutra_case()
    state, lr = H.neutra_hmc_figures(tr, tr32)
    assert 1e-8 < state < 1e-5 and 1e-8 < lr < 1e-4, (state, lr)
    assert H.neutra_hmc_figures(tr, tr) == (0.0, 0.0)
    other = copy.copy(tr32)
    other.masks = [m.clone() for m in tr32.masks]
    other.samples = [s.clone() for s in tr32.samples]
    other.masks[0][3] ^= True
    other.samples[1][3] += 5.0                                          # after the differing decision: not measured
    assert H.neutra_hmc_figures(tr, other)[0] <= state
    other.samples[0][4] += 5.0                                          # a chain that still follows: measured
    assert H.neutra_hmc_figures(tr, other)[0] > 4.9


def test_neutra_inputs_conditions_fail_when_they_should():
    p, of, tr, _tr32 = _neutra_case()
    tol = H.neutra_hmc_row_tolerance(tr, p, of, 1e-6)
    assert tol.shape == (NT, NN) and float(tol.min()) >= 2e-4
    assert float(H.neutra_hmc_row_tolerance(tr, p, of, 1.0).min()) == H.SPLINE_C_FACTOR
    acc, ties = H.neutra_hmc_inputs_ok(tr, 'host', margin=tol)
    assert acc == tr.n_accepted / (NN * NT) and ties < 0.10
    for kw in ({'margin': tol, 'lo': acc + 0.01}, {'margin': tol, 'hi': acc - 0.01}, {'margin': 1e3}):
        with pytest.raises(AssertionError):
            H.neutra_hmc_inputs_ok(tr, 'host', **kw)
    bad = copy.copy(tr)
    bad.log_ratios = [v.clone() for v in tr.log_ratios]
    bad.log_ratios[1][0] = float('nan')
    with pytest.raises(AssertionError):
        H.neutra_hmc_inputs_ok(bad, 'host', margin=tol)


def test_neutra_comparison_passes_on_the_oracles_own_and_fails_on_each_error():
    p, of, tr, _tr32 = _neutra_case()
    state_ratio, lr_ratio = _neutra_compare(_neutra_run(tr), tr)
    assert state_ratio < 0.1 and lr_ratio < 0.1
    tol = H.neutra_hmc_row_tolerance(tr, p, of, 1e-6)
    lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
    clear = int(torch.nonzero(((lu - lr).abs() > 10 * tol).all(0))[0])
    run = _neutra_run(tr)
    kept = run.samples.clone()
    kept[1, clear, 3] += 3e-5                                             # a kept state off by three times atol
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(samples=kept), tr)
    with pytest.raises(AssertionError):                                   # the final latents are not the last kept row
        _neutra_compare(run._replace(z=run.z + 1.0), tr)
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(rc=-4), tr)
    logr = run.log_ratios.clone()
    logr[2, clear] += 2 * float(tol[2, clear])                            # one log ratio off by twice its tolerance
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(log_ratios=logr), tr)
    masks = run.masks.clone()
    masks[NT - 1, clear] ^= True                                          # one decision clear of a tie, the states left alone
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(masks=masks), tr)
    # the raised tolerance: with the row's tolerance as the log-ratio figure (4 x it allowed) the same error passes
    H.compare_neutra_hmc(run._replace(log_ratios=logr), tr, p, of, 'host neutra', atol=1e-5, lr_figure=float(tol[2, clear]))


def test_neutra_unadjusted_comparison():
    p, of, _tr, _tr32 = _neutra_case()
    tr = H.neutra_hmc_oracle(p, of, NT, NL, NH_STEP, 9, adjust=False)
    run = _neutra_run(tr)
    assert _neutra_compare(run, tr, adjust=False)[1] == 0.0
    masks = run.masks.clone()
    masks[1, 7] = False
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(masks=masks), tr, adjust=False)
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(log_ratios=run.log_ratios + 0.5), tr, adjust=False)
    kept = run.samples.clone()
    kept[0, 0, 0] += 3e-5
    with pytest.raises(AssertionError):
        _neutra_compare(run._replace(samples=kept), tr, adjust=False)


def test_decisions_tolerance_is_raised_to_the_figure_given_and_not_lowered():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    want = float(tr.log_ratios[0].reshape(-1)[5])
    rec.lr = rec.lr.clone()
    rec.lr[0, 5] = want + 2 * _tol(D, want, float(_u(x0[5].double())))
    assert H.compare_decisions(rec, tr, 'mala', x0, _u, 'host', at_least=1.0) < 1.0
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host', at_least=1e-9)
    assert H.compare_decisions(_oracle_rec(tr), tr, 'mala', x0, _u, 'host') < 0.05


def test_oracle_chain_offset_and_step_offset_are_the_whole_runs():
    """rows [20, 48) with chain_offset = 20 are those rows of the whole run, and a run from step0 = 1 started at the
    whole run's first kept states is its transitions 1 and 2: what the GPU tests' offsets are compared with"""
    p, of, tr, _tr32 = _neutra_case()
    part = H.neutra_hmc_oracle(H.with_starts(p, p.x0[20:]), of, NT, NL, NH_STEP, 9, chain_offset=20)
    assert torch.equal(part.stacked(), tr.stacked()[:, 20:])
    later = H.neutra_hmc_oracle(H.with_starts(p, tr.stacked()[0].float()), of, NT - 1, NL, NH_STEP, 9, step0=1)
    x1 = tr.stacked()[0]
    same = (x1.float().double() == x1).all(1)                               # chains whose fp32 restart is exact: the rejected ones
    assert bool(same.any())
    assert torch.allclose(later.stacked(), tr.stacked()[1:], atol=1e-5)


def test_direct_neutra_hmc_builds_the_call(monkeypatch):
    """_direct_neutra_hmc against a stand-in library (no GPU): the arguments that reach nfmc_neutra_hmc_steps_f32 (shape,
    step size, offsets, the work area nfmc_neutra_scratch_bytes sized, a dense store, the (T, n) mask and log-ratio
    buffers, replayed noise, the packed width), the prefilled accumulators, the edit hook, and what comes back."""
    from nfmc_amd import hip
    n, d, steps = 5, ND, 3
    seen = {}

    class Lib:
        @staticmethod
        def nfmc_neutra_scratch_bytes(n_, d_, h_, hl_, cl_):
            seen['sized'] = (n_, d_, h_, hl_, cl_)
            return 4096

        @staticmethod
        def nfmc_stats_scratch_bytes(d_):
            return 8 * 64

        @staticmethod
        def nfmc_neutra_hmc_steps_f32(ref, stream):
            a = ref._obj
            seen['args'] = {k: getattr(a, k) for k in ('n', 'n_steps', 'n_leapfrog', 'adjust', 'scratch_bytes')}
            seen['h'] = a.step_size
            seen['rng'] = (a.rng.seed, a.rng.chain_offset, a.rng.step0, bool(a.rng.replay_normals), bool(a.rng.replay_uniforms))
            seen['store'] = (a.samples.stride, a.samples.countdown, a.samples.ring_rows, a.samples.row)
            seen['imd'], seen['defer'] = bool(a.inv_mass_diag), a.stats.defer
            return seen.get('rc', 0)

    class Bij:
        n_hidden, n_hidden_layers, n_bins = 6, 2, 0

        def packed(self, dev, hidden):
            seen['hidden'] = hidden
            st = hip.NfmcRealNVP()
            st.n_hidden_layers, st.n_coupling = 2, 3
            return st, None

    class Flow:
        bijection = Bij()

    class Pot:
        def descriptor(self, dev):
            return hip.NfmcPotential()

    monkeypatch.setattr(hip, 'lib', lambda: Lib)
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: None if t is None else ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(hip, 'stream', lambda: None)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    cpu = torch.device('cpu')
    p = H.Problem(Pot(), _u, _u, torch.arange(n * d, dtype=torch.float32).reshape(n, d), d, 'stand-in')
    r = H._direct_neutra_hmc(cpu, p, Flow(), steps, 2, 0.25, 9)
    assert r.rc == 0 and r.samples.shape == (steps, n, d) and r.masks.shape == r.log_ratios.shape == (steps, n) and r.stats is None
    assert torch.equal(r.z, p.x0) and r.scratch_bytes == 4096 and r.masks.dtype == torch.bool
    assert seen['sized'] == (n, d, 6, 2, 3) and seen['hidden'] == 6           # d = 8: the flow's own width
    assert seen['args'] == {'n': n, 'n_steps': steps, 'n_leapfrog': 2, 'adjust': 1, 'scratch_bytes': 4096} and seen['h'] == 0.25
    assert seen['rng'] == (9, 0, 0, False, False) and seen['store'] == (1, 0, steps, 0) and not seen['imd'] and seen['defer'] == 0
    normals, uniforms = torch.randn(steps, n, d), torch.rand(steps, n)
    r = H._direct_neutra_hmc(cpu, p, Flow(), steps, 2, 0.25, 9, adjust=False, imd=torch.ones(d), step0=6, chain_offset=75, replay=(normals, uniforms),
                             stats='immediate', prefill=(2.5, 7), store=(2, None), hidden=64,
                             edit=lambda a, run: setattr(a, 'scratch_bytes', a.scratch_bytes - 1))
    assert seen['hidden'] == 64 and seen['sized'] == (n, d, 64, 2, 3)
    assert seen['args'] == {'n': n, 'n_steps': steps, 'n_leapfrog': 2, 'adjust': 0, 'scratch_bytes': 4095}
    assert seen['rng'] == (9, 75, 6, True, True) and seen['store'] == (2, 0, 2, 0) and seen['imd'] and seen['defer'] == 0
    assert r.samples.shape == (2, n, d)
    assert r.stats['accepted'] == r.stats['attempted'] == r.stats['nonfinite'] == 7 and bool((r.stats['sum_x'] == 2.5).all())
    seen['rc'] = hip.EUNSUPPORTED
    r = H._direct_neutra_hmc(cpu, p, Flow(), steps, 2, 0.25, 9, stats='deferred')
    assert r.rc == hip.EUNSUPPORTED and r.stats is None and seen['defer'] == 1

