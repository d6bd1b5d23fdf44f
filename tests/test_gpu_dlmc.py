"""GPU: DLMC (nfmc/algorithms/sampling/nfmc/dlmc.py) on the MI355X -- the grad_x log q kernel and the fused step against
fp64 autograd, the reference's fixtures replayed through DLMC.sample, a run with the real device refit against the fp64
restatement (test_host_dlmc.dlmc_restate), the composed routes, the sample store and the shard slice."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import golden_flow, load_golden  # noqa: E402
from test_host_dlmc import _nll, _sumsq, dlmc_restate  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _pair(kind, d, nl, nh, cl, seed):
    from nfmc_amd import flows
    from oracle import flow as oflow
    ck = {'n_layers': cl, 'n_hidden': nh}
    ocls = oflow.NICE if kind == 'nice' else oflow.RealNVP
    cls = flows.NICE if kind == 'nice' else flows.RealNVP
    torch.manual_seed(seed)
    of = oflow.perturb_(oflow.Flow(ocls((d,), n_layers=nl, conditioner_kwargs=ck)), seed, 0.4, 0.8)
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
    """Default refit keywords on the device; the restatement loads the weights every device refit produced (captured by
    a spy) and checks the refit rows are the rows of the state the step left, then follows the same transitions."""
    from nfmc_amd import flows
    from nfmc_amd.samplers import dlmc as mod
    from oracle import flow as oflow
    d, n, T = 8, 256, 4
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
    g = torch.Generator().manual_seed(9)
    normals, uniforms = torch.randn(T, n, d, generator=g), torch.rand(T, n, generator=g)
    s.replay = (normals, uniforms)
    x0 = torch.randn(n, d, generator=g)
    out = s.sample(x0, show_progress=False)
    assert len(splits) == T and len(weights) == T
    for x, xt, xv in splits:
        assert xt.shape[0] == int(0.7 * n) and xv.shape[0] == n - int(0.7 * n)
        rows = torch.cat([xt, xv]).cpu()
        assert torch.equal(torch.sort(rows.reshape(-1, d), dim=0)[0], torch.sort(x.reshape(-1, d).cpu(), dim=0)[0])
    of = oflow.Flow(oflow.RealNVP((d,)))

    def refit(t, x):
        of.load_state_dict(weights[t])
        of.double()
        np.testing.assert_allclose(x.numpy(), splits[t][0].reshape(n, d).cpu().double().numpy(), atol=1e-3)
    want, acc, calls, grads = dlmc_restate(x0, of, _sumsq, _nll(0.0), 0.05, T, normals, uniforms, refit=refit)
    got = out.samples.cpu().double()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.97
    st = out.statistics
    assert abs(st.n_accepted_trajectories - acc) <= 0.03 * n * T
    assert (st.n_target_calls, st.n_target_gradient_calls) == (calls, grads)


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
