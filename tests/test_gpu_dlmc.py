"""GPU: DLMC (nfmc/algorithms/sampling/nfmc/dlmc.py) on the MI355X -- the grad_x log q kernel and the fused step against
fp64 autograd, the reference's fixtures replayed through DLMC.sample, a run with the real device refit against the fp64
oracle (oracle.samplers.dlmc_sample), the composed routes, the sample store and the shard slice; then every kernel
instantiation and edge (rows per wave, grid stride, output pointers, stressed weights, nonfinite rows) and every sampler
route against the oracle on replayed and native Philox noise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import golden_flow, load_golden  # noqa: E402
from test_host_dlmc import GRID_TILES, _nll, _sumsq, dlmc_rows_per_wave, hp_bucket  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _pair(kind, d, nl, nh, cl, seed, stress=False, floor_couplings=2):
    from nfmc_amd import flows
    from oracle import flow as oflow
    ck = {'n_layers': cl, 'n_hidden': nh}
    ocls = oflow.NICE if kind == 'nice' else oflow.RealNVP
    cls = flows.NICE if kind == 'nice' else flows.RealNVP
    torch.manual_seed(seed)
    of = oflow.perturb_(oflow.Flow(ocls((d,), n_layers=nl, conditioner_kwargs=ck)), seed, 0.4, 0.8)
    if stress:
        _stress_(of, seed, floor_couplings)
    f = flows.Flow(cls((d,), n_layers=nl, conditioner_kwargs=ck))
    f.load_state_dict(of.state_dict())
    return of, f


GRID = [(kind, d, nl, nh, cl) for kind in ('realnvp', 'nice') for (d, nl, nh, cl) in
        [(2, 1, 4, 1), (7, 3, 8, 3), (64, 2, 4, 2), (64, 2, 8, 1), (256, 2, 8, 2), (512, 2, 4, 3), (512, 1, 8, 2)]]


@pytest.mark.parametrize('kind,d,nl,nh,cl', GRID)
def test_logq_grad_matches_fp64_autograd(dev, kind, d, nl, nh, cl):
    from nfmc_amd.samplers import dlmc
    of, f = _pair(kind, d, nl, nh, cl, d + nl + cl)
    assert dlmc.logq_grad_supported(f)
    n = 150
    x = 0.8 * torch.randn(n, d, dtype=torch.float64)
    od = of.double()
    xr = x.clone().requires_grad_(True)
    lq_ref = od.log_prob(xr)
    g_ref, = torch.autograd.grad(lq_ref.sum(), xr)
    g, lq = dlmc.logq_grad(f, x.float().to(dev))
    scale = 1 + float(g_ref.abs().max())
    np.testing.assert_allclose(lq.cpu().double().numpy(), lq_ref.detach().numpy(),
                               atol=2e-4 * (1 + float(lq_ref.detach().abs().max())), rtol=0)
    np.testing.assert_allclose(g.cpu().double().numpy(), g_ref.numpy(), atol=2e-4 * scale, rtol=0)


@pytest.mark.parametrize('pot', ['sumsq', 'funnel', 'borrowed'])
def test_fused_step_matches_composed_autograd(dev, pot):
    from nfmc_amd.potentials import Funnel, SumOfSquares
    from nfmc_amd.samplers import dlmc
    d, n, eps = 33, 300, 0.07
    of, f = _pair('realnvp', d, 2, 8, 2, 5)
    target = Funnel((d,), 3.0) if pot == 'funnel' else SumOfSquares((d,))
    x = (0.7 * torch.randn(n, d)).to(dev)
    gu = dlmc._grad(target, x, (d,))
    want = x - eps * (gu + dlmc.logq_grad_torch(f, x, (d,)))
    y = x.clone()
    if pot == 'borrowed':
        assert dlmc.step_supported(f, y, eps, grad_u=gu)
        dlmc.launch_step(f, y, eps, grad_u=gu)
    else:
        assert dlmc.step_supported(f, y, eps, pot=target)
        dlmc.launch_step(f, y, eps, pot=target)
    torch.testing.assert_close(y, want, atol=2e-4 * (1 + float(want.abs().max())), rtol=0)


def test_unsupported_flows_answer_no_kernel(dev):
    from nfmc_amd import flows
    from nfmc_amd.samplers import dlmc
    wide = flows.Flow(flows.RealNVP((16,), conditioner_kwargs={'n_hidden': 16}))
    spline = flows.Flow(flows.CRQNSF((16,)))
    x = torch.zeros(4, 16, device=dev)
    for f in (wide, spline):
        assert not dlmc.step_supported(f, x, 0.1, grad_u=x)
    assert not dlmc.logq_grad_supported(wide)
    with pytest.raises(ValueError):
        dlmc.logq_grad(wide, x)


def _replay_run(fx, dev, latent):
    from nfmc_amd import flows
    from nfmc_amd.samplers.dlmc import DLMC, DLMCKernel, DLMCParameters
    f = flows.Flow(flows.RealNVP((6,)))
    f.load_state_dict(golden_flow(fx, 6).state_dict())
    f.fit = lambda *a, **k: None
    T = int(fx['n_iterations'])
    s = DLMC((6,), _sumsq, _nll(float(fx['nll_shift'])), DLMCKernel((6,), flow=f, step_size=float(fx['step_size'])),
             DLMCParameters(n_iterations=T, latent_updates=latent))
    s.replay = (fx['noise/normals'], fx['noise/uniforms'])
    s.seed = 1
    return s, s.sample(torch.from_numpy(fx['x0']), show_progress=False)


@pytest.mark.parametrize('name', ['dlmc_d6', 'dlmc_latent_d6'])
def test_golden_replay(dev, name):
    fx = load_golden(name)
    s, out = _replay_run(fx, dev, bool(fx['latent_updates']))
    assert s.last_route == ('latent' if fx['latent_updates'] else 'fused')
    np.testing.assert_allclose(out.samples.cpu().numpy(), fx['exp/samples'], atol=2e-4)
    st = out.statistics
    got = (st.n_accepted_trajectories, st.n_attempted_trajectories, st.n_divergences, st.n_target_calls,
           st.n_target_gradient_calls)
    assert got == tuple(int(v) for v in fx['exp/counters'])
    np.testing.assert_allclose(st.running_first_moment.cpu().numpy(), fx['exp/first_moment'], atol=2e-4)
    np.testing.assert_allclose(st.running_second_moment.cpu().numpy(), fx['exp/second_moment'], atol=2e-4)


def test_real_refit_matches_restatement(dev, monkeypatch):
    """Default refit keywords on the device; the oracle loads the weights every device refit produced (captured by a
    spy) and checks the refit rows are the rows of the state the step left, then follows the same transitions."""
    _real_refit_run(monkeypatch, 8, 256)


def test_real_refit_matches_restatement_d64(dev, monkeypatch):
    """As above at d = 64 with n = 4096 chains (2867 training and 1229 validation rows per refit)."""
    _real_refit_run(monkeypatch, 64, 4096)


def _real_refit_run(monkeypatch, d, n):
    from nfmc_amd import flows
    from nfmc_amd.samplers import dlmc as mod
    from oracle import flow as oflow, samplers as osamp
    T = 4
    torch.manual_seed(3)
    f = flows.Flow(flows.RealNVP((d,)))
    splits, weights = [], []
    orig_split, orig_refit = mod.train_val_split, mod.DLMC._refit

    def split_spy(x, **kw):
        xt, xv = orig_split(x, **kw)
        splits.append((x.clone(), xt.clone(), xv.clone()))
        return xt, xv

    def refit_spy(self, flow, x_train, x_val):
        r = orig_refit(self, flow, x_train, x_val)
        if r is not None:
            r.result()
        weights.append({k: v.detach().cpu().clone() for k, v in flow.state_dict().items()})
        return None
    monkeypatch.setattr(mod, 'train_val_split', split_spy)
    monkeypatch.setattr(mod.DLMC, '_refit', refit_spy)
    s = mod.DLMC((d,), _sumsq, _nll(0.0), mod.DLMCKernel((d,), flow=f), mod.DLMCParameters(n_iterations=T))
    assert s.params.flow_fit_kwargs == mod.DLMCParameters().flow_fit_kwargs   # the reference's defaults
    g = torch.Generator().manual_seed(9)
    normals, uniforms = torch.randn(T, n, d, generator=g), torch.rand(T, n, generator=g)
    s.replay = (normals, uniforms)
    x0 = torch.randn(n, d, generator=g)
    out = s.sample(x0, show_progress=False)
    assert s.last_route == 'fused'
    assert len(splits) == T and len(weights) == T
    for x, xt, xv in splits:
        assert xt.shape[0] == int(0.7 * n) and xv.shape[0] == n - int(0.7 * n)
        rows = torch.cat([xt, xv]).cpu()
        assert torch.equal(torch.sort(rows.reshape(-1, d), dim=0)[0], torch.sort(x.reshape(-1, d).cpu(), dim=0)[0])
    of = oflow.Flow(oflow.RealNVP((d,)))

    def refit(t, flow, x):
        flow.load_state_dict(weights[t])
        flow.double()
        np.testing.assert_allclose(x.numpy(), splits[t][0].reshape(n, d).cpu().double().numpy(), atol=1e-3)
    tr = osamp.dlmc_sample(x0, _sumsq, _nll(0.0), of, T, 0.05,
                           noise=osamp.ReplayNoise(normals.double(), uniforms.double()), refit=refit)
    assert tr.n_refits == T
    got = out.samples.cpu().double()
    same = (got - tr.stacked()).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.97
    st = out.statistics
    assert abs(st.n_accepted_trajectories - tr.n_accepted) <= 0.03 * n * T
    assert (st.n_target_calls, st.n_target_gradient_calls) == (tr.n_target_calls, tr.n_target_gradient_calls)


def test_composed_routes_autograd_target_and_spline(dev):
    from nfmc_amd import flows
    from nfmc_amd.samplers.dlmc import DLMC, DLMCKernel, DLMCParameters
    d, n, T = 6, 64, 3
    quartic = lambda x: torch.sum(x ** 4, dim=-1) / 4 + torch.sum(x, dim=-1) * 0.1   # not a quadratic
    s = DLMC((d,), quartic, quartic, DLMCKernel((d,)), DLMCParameters(n_iterations=T))
    out = s.sample(torch.randn(n, d), show_progress=False)
    assert s.last_route == 'borrowed'
    assert out.samples.shape == (T, n, d) and torch.isfinite(out.samples).all()
    s = DLMC((d,), _sumsq, _sumsq, DLMCKernel((d,), flow=flows.Flow(flows.CRQNSF((d,)))), DLMCParameters(n_iterations=T))
    out = s.sample(torch.randn(n, d), show_progress=False)
    assert s.last_route == 'composed'
    assert out.samples.shape == (T, n, d) and torch.isfinite(out.samples).all()
    assert out.statistics.n_attempted_trajectories == n * T


def test_store_thinning_shard_and_determinism(dev, monkeypatch):
    from nfmc_amd import flows
    from nfmc_amd.dist import Shard
    from nfmc_amd.samplers import dlmc as mod
    d, n, T = 5, 96, 6
    torch.manual_seed(0)
    state = flows.Flow(flows.RealNVP((d,))).state_dict()
    x0 = torch.randn(n, d)

    def run(shard=None, **params):
        f = flows.Flow(flows.RealNVP((d,)))
        f.load_state_dict(state)
        f.fit = lambda *a, **k: None
        s = mod.DLMC((d,), _sumsq, _sumsq, mod.DLMCKernel((d,), flow=f), mod.DLMCParameters(n_iterations=T, **params))
        s.seed, s.shard = 77, shard
        return s.sample(x0, show_progress=False)
    monkeypatch.setattr(mod, 'train_val_split', lambda x, **kw: (x[0], x[0]))   # the fit is a no-op here
    a, b = run(), run()
    assert torch.equal(a.samples, b.samples) and a.statistics.n_accepted_trajectories == b.statistics.n_accepted_trajectories
    assert 0 < a.statistics.n_accepted_trajectories < n * T
    thin = run(thinning=2)
    assert torch.equal(thin.samples, a.samples[1::2]) or torch.equal(thin.samples, a.samples[::2])
    none = run(store_samples=False)
    assert none.samples is None and torch.equal(none.running_samples.last_sample, a.running_samples.last_sample)
    sh = Shard(rank=1, world=2)
    sh.merge_statistics = lambda s_: s_
    part = run(shard=sh)
    lo, hi = sh.bounds(n)
    assert torch.equal(part.samples, a.samples[:, lo:hi])


def test_sample_wrapper_nll_shape(dev):
    """The reference's test_sample_wrapper_nll call shape for dlmc (test/test_samplers.py:205-224)."""
    from nfmc_amd import sample
    torch.manual_seed(0)
    out = sample(_sumsq, event_shape=(5,), strategy='dlmc', negative_log_likelihood=_sumsq, n_chains=4, n_iterations=3,
                 device=torch.device('cuda'), show_progress=False)
    assert out.samples.shape == (3, 4, 5) and torch.isfinite(out.samples).all()


# ================================================================================================ kernel edges
# Every (kind, HP, RPW, MODE) instantiation of dlmc_kernel against fp64 autograd through oracle.flow.  RPW follows d
# (test_host_dlmc.dlmc_rows_per_wave: 64 up to d = 196, 32 up to 396, 16 up to 512), HP the conditioner width (4 for
# widths 1-4, 8 for 5-8; 3, 5 and 7 are padded into their bucket).  Tolerance: 2e-4 (1 + max|ref|), as above.
SENTINEL = 12345.0   # fills the rows past n of every output buffer: a store past the last row would land there


def _stress_(of, seed, floor_couplings=2):
    """Harder weights than perturb_(.., 0.4, 0.8): element-wise log scales anywhere in [-2, 2], and in the first
    `floor_couplings` affine couplings the alpha half of the last bias at -16 .. -8 for every other target coordinate,
    which puts alpha - m = (1 - m) e^(u / 2) at ~3e-4 .. 2e-2 of the floor m = 1e-3.  The first two couplings act on
    different halves; test_stacked_floor_couplings_lose_precision_in_the_rebuild takes three, two of them on one half."""
    from oracle import flow as oflow
    g = torch.Generator().manual_seed(seed + 1)
    k = 0
    with torch.no_grad():
        for m in of.bijection.layers:
            if isinstance(m, oflow.ElementwiseAffine):
                m.log_scale.copy_(4 * torch.rand(m.log_scale.shape, generator=g) - 2)
            elif isinstance(m, oflow.AffineCoupling) and not m.additive and k < floor_couplings:
                b = m.conditioner[-1].bias
                b[:m.d_b:2] = -16 + 8 * torch.rand(b[:m.d_b:2].shape, generator=g)
                k += 1
    return of


def _x_stress(n, d, seed):
    """Inputs with |x| up to 8: uniform on [-8, 8] in half the rows, N(0, 1.5^2) clamped to it in the other half."""
    g = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn(n, d, generator=g)
    x[::2] = 16 * torch.rand(x[::2].shape, generator=g) - 8
    x[0, :] = 8.0
    return x.clamp(-8, 8)


def _ref_logq_grad(of, x):
    """fp64 autograd of the oracle flow's log q at the fp32 input x: (grad (n, d), log q (n,))."""
    import copy
    od = copy.deepcopy(of).double()
    xr = x.detach().cpu().double().clone().requires_grad_(True)
    lq = od.log_prob(xr)
    g, = torch.autograd.grad(lq.sum(), xr)
    return g, lq.detach()


def _ref_grad_u(pot, x):
    xr = x.detach().cpu().double().clone().requires_grad_(True)
    g, = torch.autograd.grad(pot(xr).sum(), xr)
    return g


def _close(got, ref, what):
    """|got - ref| <= 2e-4 (1 + max|ref|); prints the measured ratio of the worst error to that bound's scale."""
    got = got.detach().cpu().double()
    scale = 1 + float(ref.abs().max())
    err = float((got - ref).abs().max())
    print('%s: max err %.3e, err / (1 + max|ref|) = %.2e' % (what, err, err / scale))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=2e-4 * scale, rtol=0, err_msg=what)


def _buf(rows, d, dev):
    """(buffer, view of its first `rows` rows): the rows past them hold SENTINEL."""
    b = torch.full((rows + 65,) + ((d,) if d else ()), SENTINEL, dtype=torch.float32, device=dev)
    return b, b[:rows]


def _raw_logq_grad(f, x, grad_out, logq_out):
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc
    a, _keep = dlmc.logq_grad_args(f, x, grad_out, logq_out)
    return int(hip.lib().nfmc_flow_logq_grad_f32(C.byref(a), hip.stream()))


def _logq_grad(f, x):
    """MODE 0 into guarded buffers: (grad, log q) of the rows of x; asserts nothing was stored past the last row."""
    n, d = x.shape
    gb, g = _buf(n, d, x.device)
    lb, lq = _buf(n, 0, x.device)
    assert _raw_logq_grad(f, x.contiguous(), g, lq) == 0
    torch.cuda.synchronize()
    assert bool((gb[n:] == SENTINEL).all()) and bool((lb[n:] == SENTINEL).all())
    return g.clone(), lq.clone()


def _step(f, x, eps, pot=None, grad_u=None, logq=False):
    """MODE 1 on a guarded copy of x: the stepped rows (and the step's log q when `logq`)."""
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc
    n, d = x.shape
    xb, y = _buf(n, d, x.device)
    y.copy_(x)
    lb, lq = _buf(n, 0, x.device)
    a, _keep = dlmc.step_args(f, y, eps, pot, grad_u)
    a.logq_out = hip.ptr(lq) if logq else None
    hip.check(hip.lib().nfmc_dlmc_step_f32(C.byref(a), hip.stream()), 'nfmc_dlmc_step_f32')
    torch.cuda.synchronize()
    assert bool((xb[n:] == SENTINEL).all()) and bool((lb[n:] == SENTINEL).all())
    if not logq:
        assert bool((lq == SENTINEL).all())
    return (y.clone(), lq.clone()) if logq else y.clone()


# (kind, d, coupling layers, conditioner width, hidden layers): each (kind, HP, RPW) cell, d on both sides of both RPW
# switch points, d = 2, odd d and d = 512; widths 3, 5, 7 (padded) and 4, 8; 1-4 hidden layers; 1-4 couplings
EDGE_GRID = [('realnvp', 2, 1, 3, 1), ('nice', 2, 2, 5, 4), ('realnvp', 7, 3, 7, 2), ('nice', 7, 4, 4, 3),
             ('realnvp', 196, 2, 4, 4), ('nice', 196, 1, 8, 1), ('realnvp', 197, 1, 5, 3), ('nice', 197, 3, 3, 2),
             ('realnvp', 396, 2, 3, 1), ('nice', 396, 2, 8, 4), ('realnvp', 397, 3, 8, 2), ('nice', 397, 1, 4, 4),
             ('realnvp', 512, 2, 3, 3), ('nice', 512, 3, 7, 1)]


def test_edge_grid_covers_every_instantiation():
    cells = {(k, hp_bucket(nh), dlmc_rows_per_wave(d)) for k, d, _nl, nh, _cl in EDGE_GRID}
    assert cells == {(k, hp, r) for k in ('realnvp', 'nice') for hp in (4, 8) for r in (64, 32, 16)}
    assert {cl for *_, cl in EDGE_GRID} == {1, 2, 3, 4} and {nl for _k, _d, nl, _h, _c in EDGE_GRID} == {1, 2, 3, 4}
    assert {3, 4, 5, 7, 8} <= {nh for _k, _d, _nl, nh, _c in EDGE_GRID}


@pytest.mark.parametrize('kind,d,nl,nh,cl', EDGE_GRID)
def test_logq_grad_stressed_matches_fp64(dev, kind, d, nl, nh, cl):
    """MODE 0 with stressed weights and |x| up to 8, on 2 RPW + 5 rows (three tiles, the last ragged)."""
    from nfmc_amd.samplers import dlmc
    of, f = _pair(kind, d, nl, nh, cl, 11 * d + nl + cl, stress=True)
    assert dlmc.logq_grad_supported(f)
    n = 2 * dlmc_rows_per_wave(d) + 5
    x = _x_stress(n, d, d + nh)
    g, lq = _logq_grad(f, x.to(dev))
    g_ref, lq_ref = _ref_logq_grad(of, x)
    _close(lq, lq_ref, 'log q %s d=%d' % (kind, d))
    _close(g, g_ref, 'grad %s d=%d' % (kind, d))


@pytest.mark.parametrize('kind,d,nh,cl', [('realnvp', 40, 3, 2), ('nice', 300, 6, 3), ('realnvp', 450, 8, 4)])
def test_row_edges_match_fp64_and_the_full_launch(dev, kind, d, nh, cl):
    """n in {1, RPW - 1, RPW, RPW + 1, 3 RPW + 2} at each RPW, MODE 0 and MODE 1: every row equals the same row of a
    5 RPW + 7 row launch bitwise (a lane owns its row), and that launch matches fp64."""
    from nfmc_amd.potentials import SumOfSquares
    rpw = dlmc_rows_per_wave(d)
    of, f = _pair(kind, d, 2, nh, cl, d, stress=True)
    N, eps = 5 * rpw + 7, 0.1
    x = _x_stress(N, d, 3 * d)
    pot = SumOfSquares((d,))
    xd = x.to(dev)
    g_all, lq_all = _logq_grad(f, xd)
    y_all = _step(f, xd, eps, pot=pot)
    g_ref, lq_ref = _ref_logq_grad(of, x)
    _close(lq_all, lq_ref, 'log q')
    _close(g_all, g_ref, 'grad')
    _close(y_all, x.double() - eps * (_ref_grad_u(pot, x) + g_ref), 'step')
    for n in (1, rpw - 1, rpw, rpw + 1, 3 * rpw + 2):
        g, lq = _logq_grad(f, xd[:n])
        assert torch.equal(g, g_all[:n]) and torch.equal(lq, lq_all[:n]), n
        assert torch.equal(_step(f, xd[:n], eps, pot=pot), y_all[:n]), n


@pytest.mark.parametrize('d', [512, 64])
def test_grid_stride_rows_match_their_own_launch(dev, d):
    """More than 4 kMaxGrid = 8192 tiles: tiles 8192 on run in the grid-stride loop's second pass.  Those rows must be
    bitwise the rows of a launch of them alone; the last tile and ~2000 random rows (some of them in the second pass)
    are checked against fp64, for MODE 0 and MODE 1."""
    from nfmc_amd.potentials import DiagonalGaussian
    rpw = dlmc_rows_per_wave(d)
    assert rpw == {512: 16, 64: 64}[d]
    first = GRID_TILES * rpw                  # first row of the second pass
    n = first + 2 * rpw + 37                  # three tiles in the second pass, the last ragged
    of, f = _pair('realnvp', d, 2, 5, 3, 4 * d, stress=True)
    gen = torch.Generator(device=dev).manual_seed(d)
    x = 1.2 * torch.randn(n, d, device=dev, generator=gen)
    mu, sig = 0.3 * torch.randn(d), 0.5 + torch.rand(d)
    pot, eps = DiagonalGaussian((d,), mu, sig), 0.05
    g, lq = _logq_grad(f, x)
    g2, lq2 = _logq_grad(f, x[first:].clone())
    assert torch.equal(g[first:], g2) and torch.equal(lq[first:], lq2)
    y = _step(f, x, eps, pot=pot)
    y2 = _step(f, x[first:].clone(), eps, pot=pot)
    assert torch.equal(y[first:], y2)
    pick = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:2000]
    rows = torch.unique(torch.cat([pick, torch.arange((n - 1) // rpw * rpw, n), torch.arange(first, first + 40)]))
    xs = x[rows.to(dev)].cpu()
    g_ref, lq_ref = _ref_logq_grad(of, xs)
    _close(g[rows.to(dev)], g_ref, 'grad (grid stride)')
    _close(lq[rows.to(dev)], lq_ref, 'log q (grid stride)')
    _close(y[rows.to(dev)], xs.double() - eps * (_ref_grad_u(pot, xs) + g_ref), 'step (grid stride)')


@pytest.mark.parametrize('kind,d,nh', [('realnvp', 9, 6), ('nice', 250, 4), ('realnvp', 450, 3)])
def test_output_pointers(dev, kind, d, nh):
    """MODE 0 with only logq_out or only grad_out is bitwise the run with both; both NULL is NFMC_EINVAL; the step's
    logq_out is MODE 0's log q of the PRE-step x, with a closed-form potential and with a borrowed grad U."""
    from nfmc_amd import hip
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import dlmc
    of, f = _pair(kind, d, 3, nh, 2, d + 1, stress=True)
    n = 2 * dlmc_rows_per_wave(d) + 3
    x = _x_stress(n, d, d).to(dev)
    g, lq = _logq_grad(f, x)
    gb, g_only = _buf(n, d, dev)
    assert _raw_logq_grad(f, x, g_only, None) == 0
    lb, lq_only = _buf(n, 0, dev)
    assert _raw_logq_grad(f, x, None, lq_only) == 0
    torch.cuda.synchronize()
    assert torch.equal(g_only, g) and torch.equal(lq_only, lq)
    assert bool((gb[n:] == SENTINEL).all()) and bool((lb[n:] == SENTINEL).all())
    assert _raw_logq_grad(f, x, None, None) == hip.EINVAL
    with pytest.raises(ValueError):
        a, _keep = dlmc.logq_grad_args(f, x)
        hip.check(hip.lib().nfmc_flow_logq_grad_f32(C.byref(a), hip.stream()), 'nfmc_flow_logq_grad_f32')
    _y, lq_step = _step(f, x, 0.1, pot=SumOfSquares((d,)), logq=True)
    assert torch.equal(lq_step, lq)
    _y, lq_step = _step(f, x, 0.1, grad_u=torch.ones_like(x), logq=True)
    assert torch.equal(lq_step, lq)


def _step_target(name, d, seed):
    from nfmc_amd.potentials import DiagonalGaussian, Funnel, GaussianMixture, QuadraticPotential, SumOfSquares
    g = torch.Generator().manual_seed(seed)
    if name == 'sumsq':
        return SumOfSquares((d,))
    if name == 'diag':
        return DiagonalGaussian((d,), torch.randn(d, generator=g), 0.5 + torch.rand(d, generator=g))
    if name == 'quad':
        return QuadraticPotential((d,), 0.37, -0.6)
    if name == 'funnel':
        return Funnel((d,), 3.0)
    return GaussianMixture((d,), 1.5 * torch.randn(3, d, generator=g), 0.6 + 0.8 * torch.rand(3, d, generator=g),
                           [0.2, 0.5, 0.3])


STEP_TARGETS = ['sumsq', 'diag', 'quad', 'funnel', 'mixture']


@pytest.mark.parametrize('target', STEP_TARGETS)
@pytest.mark.parametrize('d,nh', [(d, nh) for d in (9, 300, 480) for nh in (3, 6)])
def test_fused_step_every_cell_and_target(dev, d, nh, target):
    """MODE 1 at every (HP, RPW) cell (both kinds over the targets of a cell) with each target the step takes: the
    closed-form quadratic (scalar a = 1, per-coordinate a and b, scalar a != 1 with b != 0) and funnel gradients, and a
    borrowed grad_u (a Gaussian mixture's, from autograd).  Against x - eps (grad U + grad log q) in fp64 at the fp32
    input; with eps = 0 x stays bitwise unchanged."""
    from nfmc_amd.samplers import dlmc
    i = STEP_TARGETS.index(target)
    kind = ('realnvp', 'nice')[(i + nh) % 2]
    of, f = _pair(kind, d, 1 + i % 3, nh, 1 + (i + nh) % 4, 7 * d + i, stress=True)
    pot = _step_target(target, d, d + i)
    n, eps = 2 * dlmc_rows_per_wave(d) + 9, 0.1
    x = 1.2 * torch.randn(n, d, generator=torch.Generator().manual_seed(i))
    if target == 'funnel':
        x[:, 0] = x[:, 0].clamp(-1.5, 1.5)
    xd = x.to(dev)
    if target == 'mixture':
        gu = dlmc._grad(pot, xd, (d,))
        kw = dict(grad_u=gu)
        assert dlmc.step_supported(f, xd, eps, grad_u=gu) and not pot.fused_in('dlmc_step')
    else:
        kw = dict(pot=pot)
        assert dlmc.step_supported(f, xd, eps, pot=pot)
    y = _step(f, xd, eps, **kw)
    g_ref, _ = _ref_logq_grad(of, x)
    _close(y, x.double() - eps * (_ref_grad_u(pot, x) + g_ref), 'step %s %s d=%d' % (kind, target, d))
    assert torch.equal(_step(f, xd, 0.0, **kw), xd)


def test_stacked_floor_couplings_lose_precision_in_the_rebuild(dev):
    """Two couplings with alpha near the floor on the same half (couplings 1 and 3 of 3): the reverse sweep rebuilds each
    layer's input as (y - beta) / alpha, and every such division by alpha ~ 1e-3 turns the fp32 rounding of y into an
    error ~ulp(beta) / alpha in the rebuilt input, which the earlier coupling's conditioner then amplifies again.
    fp64 autograd does not rebuild.  Measured on the MI355X: 6e-4 (d = 300) and 9.6e-4 (d = 480) of 1 + max|ref| for the
    step; an fp32 host emulation of the same sweep gives 2.5e-4 and 2.1e-3, and the same sweep in fp64 matches autograd to
    5e-9 absolute, so this is the fp32 conditioning of the rebuild, not a wrong term.  Weights without the stacked floor stay
    under 2e-4 (test_fused_step_every_cell_and_target: ~3e-7 at these shapes).  Bound: 1e-2 (1 + max|ref|), and the
    error must stay at least 10x under the step's size."""
    from nfmc_amd.potentials import QuadraticPotential
    d, eps = 480, 0.1
    of, f = _pair('realnvp', d, 3, 6, 1, 7 * d + 2, stress=True, floor_couplings=3)
    pot = QuadraticPotential((d,), 0.37, -0.6)
    n = 2 * dlmc_rows_per_wave(d) + 9
    x = 1.2 * torch.randn(n, d, generator=torch.Generator().manual_seed(2))
    y = _step(f, x.to(dev), eps, pot=pot).cpu().double()
    g_ref, _ = _ref_logq_grad(of, x)
    want = x.double() - eps * (_ref_grad_u(pot, x) + g_ref)
    err = float((y - want).abs().max())
    scale = 1 + float(want.abs().max())
    print('stacked floor couplings: err / (1 + max|ref|) = %.2e' % (err / scale))
    assert err <= 1e-2 * scale
    assert err <= 0.1 * float((want - x.double()).abs().max())


@pytest.mark.parametrize('d,nh', [(5, 8), (260, 3), (500, 6)])
def test_nonfinite_rows_stay_in_their_lane(dev, d, nh):
    """A NaN row and an inf row in the first tile (shared LDS with every other chain of that tile): they may come out
    nonfinite, every other row is bitwise the clean launch's, in MODE 0, MODE 1 and MODE 1 with a borrowed grad_u."""
    from nfmc_amd.potentials import SumOfSquares
    rpw = dlmc_rows_per_wave(d)
    of, f = _pair('realnvp', d, 2, nh, 2, d)
    n = 2 * rpw + 3
    x = 0.8 * torch.randn(n, d, generator=torch.Generator().manual_seed(d))
    bad = x.clone()
    bad[1, d // 2] = float('nan')
    bad[rpw - 2, 0] = float('inf')
    keep = torch.ones(n, dtype=torch.bool)
    keep[[1, rpw - 2]] = False
    xd, bd = x.to(dev), bad.to(dev)
    pot = SumOfSquares((d,))
    g, lq = _logq_grad(f, xd)
    gb, lqb = _logq_grad(f, bd)
    k = keep.to(dev)
    assert torch.equal(gb[k], g[k]) and torch.equal(lqb[k], lq[k])
    assert torch.equal(_step(f, bd, 0.1, pot=pot)[k], _step(f, xd, 0.1, pot=pot)[k])
    gu = 2 * xd
    gub = gu.clone()
    gub[1] = float('nan')
    assert torch.equal(_step(f, bd, 0.1, grad_u=gub)[k], _step(f, xd, 0.1, grad_u=gu)[k])


# ================================================================================================ sampler routes
# DLMC.sample on a frozen flow (fit a no-op) against oracle.samplers.dlmc_sample on the same noise: replayed draws, or
# the native Philox stream (iteration i draws at step i, TAG_LATENT / TAG_JUMP).  Bars of the suite: >= 97 % of the
# chains within 1e-4 (replay) / 1e-3 (Philox) over the whole run, accept counts within 3 % of n T (ties), call counters
# exact.  The route is asserted through last_route and spies on the step and flow-MH launches.
def _quartic(x):
    return torch.sum(x ** 4, dim=-1) / 4 + 0.1 * torch.sum(x, dim=-1)


def _route_run(monkeypatch, f, of, target, x0, T, noise, latent=False, seed=4242):
    from nfmc_amd.samplers import dlmc as mod
    from oracle import samplers as osamp
    n, d = x0.shape
    f.fit = lambda *a, **k: None
    calls = {'step': 0, 'flow_mh': 0, 'split_mh': 0}

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(mod, 'launch_step', spy('step', mod.launch_step))
    monkeypatch.setattr(mod, 'launch_flow_mh', spy('flow_mh', mod.launch_flow_mh))
    monkeypatch.setattr(mod, 'split_flow_mh', spy('split_mh', mod.split_flow_mh))
    s = mod.DLMC((d,), target, _nll(0.25), mod.DLMCKernel((d,), flow=f), mod.DLMCParameters(n_iterations=T,
                                                                                             latent_updates=latent))
    if noise == 'replay':
        g = torch.Generator().manual_seed(d + T)
        normals, uniforms = torch.randn(T, n, d, generator=g), torch.rand(T, n, generator=g)
        s.replay = (normals, uniforms)
        onoise, tol = osamp.ReplayNoise(normals.double(), uniforms.double()), 1e-4
    else:
        s.seed = seed
        onoise, tol = osamp.PhiloxNoise(seed, dtype=torch.float64), 1e-3
    out = s.sample(x0, show_progress=False)
    tr = osamp.dlmc_sample(x0, target, _nll(0.25), of, T, 0.05, latent=latent, noise=onoise)
    got = out.samples.cpu().double().reshape(T, n, d)
    err = (got - tr.stacked()).abs().amax(dim=(0, 2))
    same = err < tol
    print('%s: %.1f %% of the chains within %g (worst agreeing %.2e)' %
          (s.last_route, 100 * float(same.float().mean()), tol, float(err[same].max()) if same.any() else -1))
    assert same.float().mean() >= 0.97, float(same.float().mean())
    st = out.statistics
    assert abs(st.n_accepted_trajectories - tr.n_accepted) <= 0.03 * n * T, (st.n_accepted_trajectories, tr.n_accepted)
    assert 0 < tr.n_accepted < n * T
    assert st.n_attempted_trajectories == tr.n_attempted == n * T
    assert (st.n_target_calls, st.n_target_gradient_calls) == (tr.n_target_calls, tr.n_target_gradient_calls)
    assert calls['flow_mh'] + calls['split_mh'] == T
    return s, calls


def _near_identity(of, seed):
    from oracle import flow as oflow
    with torch.no_grad():
        for p in of.parameters():
            p.zero_()
    return oflow.perturb_(of, seed, 0.05)


def _route_pair(d, nh, pot, seed, spline=False):
    """For a quadratic target, a flow near the identity (every weight zeroed, then perturb_(.., 0.05)) whose first
    element-wise affine layer maps the target's Gaussian to N(0, I), so that the flow-MH step accepts a fair share of
    the proposals at every d; for other targets the flows of _pair.  Returns (oracle flow, device flow)."""
    from nfmc_amd import flows
    from nfmc_amd.potentials import QuadraticPotential
    from oracle import flow as oflow
    quad = isinstance(pot, QuadraticPotential)
    if spline:
        of = _near_identity(oflow.Flow(oflow.CRQNSF((d,))), seed) if quad else \
            oflow.perturb_(oflow.Flow(oflow.CRQNSF((d,))), seed, 0.5, 0.8)
        f = flows.Flow(flows.CRQNSF((d,)))
    elif quad:
        ck = {'n_hidden': nh}
        of = _near_identity(oflow.Flow(oflow.RealNVP((d,), conditioner_kwargs=ck)), seed)
        f = flows.Flow(flows.RealNVP((d,), conditioner_kwargs=ck))
    else:
        return _pair('realnvp', d, 2, nh, 2, seed)
    if quad:
        a = torch.as_tensor(pot.a, dtype=torch.float32).expand(d)   # U = a (x - b)^2: sigma^2 = 1 / (2 a), mean b
        b = torch.as_tensor(pot.b, dtype=torch.float32).expand(d)
        with torch.no_grad():
            ea = of.bijection.layers[0]
            ea.log_scale.copy_(0.5 * torch.log(2 * a))
            ea.shift.copy_(-b * torch.sqrt(2 * a))
    f.load_state_dict(of.state_dict())
    return of, f


FUSED_RUNS = [(64, 4, 'sumsq'), (64, 8, 'funnel'), (256, 8, 'diag'), (256, 4, 'funnel'), (512, 4, 'diag'),
              (512, 8, 'sumsq')]


@pytest.mark.parametrize('noise', ['replay', 'philox'])
@pytest.mark.parametrize('d,nh,target', FUSED_RUNS)
def test_fused_route_matches_oracle(dev, monkeypatch, d, nh, target, noise):
    pot = _step_target(target, d, d)
    of, f = _route_pair(d, nh, pot, d + nh)
    x0 = 0.8 * torch.randn(150, d, generator=torch.Generator().manual_seed(d + nh))
    s, calls = _route_run(monkeypatch, f, of, pot, x0, 5, noise)
    assert s.last_route == 'fused' and calls['step'] == 5


@pytest.mark.parametrize('noise', ['replay', 'philox'])
@pytest.mark.parametrize('target', ['mixture', 'callable'])
def test_borrowed_route_matches_oracle(dev, monkeypatch, target, noise):
    """A Gaussian mixture (no closed form in the step; the flow-MH step fused) and a plain callable (flow-MH split)."""
    d = 32 if target == 'mixture' else 16
    of, f = _pair('realnvp', d, 2, 6, 2, d)
    pot = _step_target('mixture', d, 5) if target == 'mixture' else _quartic
    x0 = 0.8 * torch.randn(150, d, generator=torch.Generator().manual_seed(d))
    s, calls = _route_run(monkeypatch, f, of, pot, x0, 5, noise)
    assert s.last_route == 'borrowed' and calls['step'] == 5
    assert calls['flow_mh' if target == 'mixture' else 'split_mh'] == 5


@pytest.mark.parametrize('noise', ['replay', 'philox'])
def test_latent_route_matches_oracle(dev, monkeypatch, noise):
    from nfmc_amd.potentials import SumOfSquares
    d = 64
    pot = SumOfSquares((d,))
    of, f = _route_pair(d, 4, pot, 3)
    x0 = 0.8 * torch.randn(150, d, generator=torch.Generator().manual_seed(1))
    s, calls = _route_run(monkeypatch, f, of, pot, x0, 5, noise, latent=True)
    assert s.last_route == 'latent' and calls['step'] == 0


@pytest.mark.parametrize('noise', ['replay', 'philox'])
@pytest.mark.parametrize('flow', ['spline', 'wide'])
def test_composed_route_matches_oracle(dev, monkeypatch, flow, noise):
    """A spline flow, and an affine flow whose conditioner (16) is wider than the step kernel's 8: grad log q by
    autograd, the step in torch."""
    from nfmc_amd.potentials import SumOfSquares
    d = 12
    pot = SumOfSquares((d,))
    of, f = _route_pair(d, 16, pot, 9, spline=flow == 'spline')
    x0 = 0.8 * torch.randn(150, d, generator=torch.Generator().manual_seed(2))
    s, calls = _route_run(monkeypatch, f, of, pot, x0, 5, noise)
    assert s.last_route == 'composed' and calls['step'] == 0
