"""f1 for spline couplings: the device fit of 'c-rqnsf' flows (csrc/fit_rqs.hip behind nfmc_flow_fit_step_f32,
nfmc_flow_variational_fit_step_f32 and nfmc_flow_fit_epochs_f32) against autograd of the CPU restatement (oracle/flow.py:
CRQNSF), against torch.optim.AdamW on flow_training.forward_torch, and through the public fit / warmup / refit paths.

Tolerances are the affine reverse-KL test's: every gradient entry within 3e-4 of the largest entry of its tensor, the batch
loss within 3e-5.  On rows without a spline input within 1e-4 of a knot, fp32 autograd of the restatement differs from its
fp64 autograd by at most 1.2e-5 (maximum likelihood) / 2.4e-5 (reverse KL) of that scale, so the bound is >= 12 times the
reference's own fp32 floor; the margin covers hardware exp / rcp / sqrt / log and another summation order.

The knot filter: a point within rounding of a knot may land in the neighbouring bin on the other side; the value is
continuous there, the gradient of the log-derivative term is not.  Rows with such a point (in any coupling layer, +-B
included) are removed before either side runs, by an fp64 walk of the restatement's layers (tests/spline_fixtures.py, which
also holds the gradient check; tests/test_gpu_spline_trained.py uses both on trained splines)."""
import copy
import math

import numpy as np
import pytest
import torch

from spline_fixtures import (check_gradient as _check_gradient, device_potential as _potential, filtered as _filtered,
                             knot_free as _knot_free)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _flow(d, n_hidden, n_hl, n_layers, seed):
    from nfmc_amd.flows import CRQNSF, Flow
    from oracle import flow as oflow
    ck = {'n_hidden': n_hidden, 'n_layers': n_hl}
    of = oflow.perturb_(oflow.Flow(oflow.CRQNSF((d,), n_layers=n_layers, conditioner_kwargs=ck)), seed, 0.3, 0.8)
    f = Flow(CRQNSF((d,), n_layers=n_layers, conditioner_kwargs=ck))
    f.load_state_dict(of.state_dict())
    return of, f


def _rows(n, d, seed):
    """1.2 randn, the first max(2, n // 20) rows five times as far out: some coordinates lie in the identity tails."""
    x = 1.2 * torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    x[:max(2, n // 20)] *= 5.0
    return x


SHAPES = [  # d, n_hidden, hidden layers, coupling layers, rows, potential of the reverse-KL case
    (6, 4, 2, 2, 50, 'sum'), (7, 3, 1, 3, 64, 'diag'), (25, 4, 2, 2, 200, 'funnel'), (64, 8, 2, 2, 130, 'sum'),
    (100, 7, 2, 3, 129, 'diag'), (128, 5, 2, 2, 70, 'funnel'), (256, 7, 2, 2, 300, 'sum'), (1, 4, 2, 2, 30, 'diag'),
    (33, 8, 1, 2, 65, 'funnel'), (16, 4, 2, 2, 4300, 'sum'),
    # one and four coupling layers; conditioner widths 1 and 2
    (6, 4, 2, 1, 50, 'diag'), (10, 4, 2, 4, 50, 'funnel'), (6, 1, 1, 2, 40, 'sum'), (9, 2, 2, 2, 40, 'diag'),
    # a lone row, an exactly full 16-row tile, a one-row second tile
    (12, 4, 2, 2, 1, 'funnel'), (12, 4, 2, 2, 16, 'sum'), (12, 4, 2, 2, 17, 'diag'),
    # so many parameters that 64 MiB of partial-gradient slabs hold fewer than 256: the grid is capped below the tile count
    (256, 8, 2, 3, 4200, 'sum'),
]
CAPPED = (256, 8, 2, 3, 4200)
ROW_SEED = {(6, 1): 61}      # (d, coupling layers): with d's own seed neither far-out row reaches the one coupling's tails


def _case_rows(of, d, n, inverse, nl=2):
    """The rows of a SHAPES case after the knot filter.  n = 1: a hand-made row with one coordinate in the identity tails
    (the filter's two-tail-rows assert cannot hold for it; that it is kept and has its tail coordinate is asserted here)."""
    if n == 1:
        rows = torch.linspace(-2.0, 2.0, d).reshape(1, d).clone()
        rows[0, 3] = 7.5
        keep, tail = _knot_free(of, rows, inverse)
        assert bool(keep.all()) and bool(tail.all())
        return _filtered(of, rows, inverse, need_tail=False)
    if n <= 17:     # a row count that stands for a tile edge: spare rows, so that exactly n come through the filter
        rows = _filtered(of, _rows(n + 8, d, d), inverse=inverse)[:n].contiguous()
        assert rows.shape[0] == n and int(_knot_free(of, rows, inverse)[1].sum()) >= 2
        return rows
    return _filtered(of, _rows(n, d, ROW_SEED.get((d, nl), d)), inverse=inverse)


def _assert_grid(fit, shape, n_rows):
    """The workgroups of the spline gradient launch on `n_rows` rows, from the workspace the library sizes for them (one
    slab of n_params + 4 floats each); for the CAPPED shape the 64 MiB cap falls below 256 and below the tile count, so
    workgroups stride over several tiles."""
    import ctypes as C
    from nfmc_amd import hip
    slabs = []
    for rows in (n_rows, 1 << 20):
        nfl = C.c_int64(0)
        hip.lib().nfmc_flow_fit_workspace(C.byref(fit.flow_struct), rows, 0, fit.n_params, C.byref(nfl))
        assert nfl.value % (fit.n_params + 4) == 0
        slabs.append(nfl.value // (fit.n_params + 4))
    grid, cap = slabs
    tiles = (n_rows + 15) // 16
    print('tiles %d, workgroups %d, cap %d' % (tiles, grid, cap))
    assert grid == min(tiles, cap) and cap <= 256
    if shape == CAPPED:
        assert cap < 256 and cap < tiles


@pytest.mark.parametrize('d,H,nhl,nl,n,_kind', SHAPES)
def test_spline_nll_gradient_matches_autograd(dev, d, H, nhl, nl, n, _kind):
    """One maximum-likelihood step with lr = 0, weight decay 0 and beta1 = 0 leaves the parameters alone and the first
    moment equal to the gradient: every entry against autograd of the CPU restatement, the batch loss against its value,
    the blob's padding exactly zero."""
    from nfmc_amd.flow_training import DeviceFit
    of, f = _flow(d, H, nhl, nl, 3 + d)
    x = _case_rows(of, d, n, False, nl)
    f.to(dev)
    assert DeviceFit.supported(f.bijection, dev)
    fit = DeviceFit(f.bijection, dev, x.shape[0], lr=0.0)
    _assert_grid(fit, (d, H, nhl, nl, n), x.shape[0])
    fit.opt.beta1, fit.opt.weight_decay = 0.0, 0.0
    before = fit.params.clone()
    fit.step(x.to(dev), 0)
    torch.cuda.synchronize()
    assert torch.equal(fit.params, before)                              # lr = 0: nothing moved
    _check_gradient(fit, f, of, -of.log_prob(x).mean(), dev)


@pytest.mark.parametrize('d,H,nhl,nl,n,kind', SHAPES)
def test_spline_reverse_kl_gradient_matches_autograd(dev, d, H, nhl, nl, n, kind):
    """The variational-fit step: loss mean[log q(x) - log p(x)], x = f^-1(z), and its gradient with respect to every
    parameter against autograd through the CPU restatement's inverse pass and the potential's torch form."""
    from nfmc_amd.flow_training import DeviceFit
    of, f = _flow(d, H, nhl, nl, 3 + d)
    z = _case_rows(of, d, n, True, nl)
    pot = _potential(kind, d)
    f.to(dev)
    fit = DeviceFit(f.bijection, dev, z.shape[0], lr=0.0)
    _assert_grid(fit, (d, H, nhl, nl, n), z.shape[0])
    fit.opt.beta1, fit.opt.weight_decay = 0.0, 0.0
    fit.step_variational(z.to(dev), pot.descriptor(dev), 0)
    torch.cuda.synchronize()
    x, ld = of.bijection.inverse(z)
    _check_gradient(fit, f, of, (of.base_log_prob(z) - ld + pot(x)).mean(), dev)


def test_the_same_spline_step_twice_is_bitwise_the_same(dev):
    """Fixed-order sums everywhere: batch and validation rows over several tiles and more than one chunk of targets."""
    from nfmc_amd.flow_training import DeviceFit
    d = 40
    _of, f = _flow(d, 6, 2, 3, 19)
    f.to(dev)
    g0 = torch.Generator().manual_seed(6)
    x = (torch.randn(333, d, generator=g0) * 1.5).to(dev)
    xv = (torch.randn(70, d, generator=g0) * 1.5).to(dev)
    fit = DeviceFit(f.bijection, dev, 403, lr=0.0)
    fit.opt.beta1, fit.opt.weight_decay = 0.0, 0.0
    fit.set_validation(xv)
    fit.step(x, 0)
    first, status = fit.m.clone(), fit.status.clone()
    fit.step(x, 0)
    assert torch.equal(fit.m, first) and torch.equal(fit.status, status)
    assert float(first.abs().max()) > 0 and math.isfinite(float(status[2]))


def test_a_shrinking_spline_batch_with_validation_rows_leaves_no_stale_gradients(dev):
    """Workgroups that only see validation tiles never write the gradient part of their slab, so the fold must not add
    those slabs: a large batch, then a small one on ONE fitter give the small batch's gradient exactly as a fresh fitter
    computes it."""
    from nfmc_amd.flow_training import DeviceFit
    d = 32
    _of, f = _flow(d, 6, 2, 2, 17)
    f.to(dev)
    g0 = torch.Generator().manual_seed(3)
    big = (torch.randn(900, d, generator=g0) * 0.9).to(dev)
    small = (torch.randn(70, d, generator=g0) * 0.9).to(dev)
    xv = (torch.randn(500, d, generator=g0) * 0.9).to(dev)

    def fitter():
        ft_ = DeviceFit(f.bijection, dev, 1400, lr=0.0)
        ft_.opt.beta1, ft_.opt.weight_decay = 0.0, 0.0
        ft_.set_validation(xv)
        return ft_
    a = fitter()
    a.step(big, 0)
    a.step(small, 0)
    b = fitter()
    b.step(small, 0)
    assert torch.equal(a.m, b.m)
    assert float(a.m.abs().max()) > 0
    assert torch.equal(a.status, b.status)


def test_enqueued_spline_run_equals_the_step_by_step_loop(dev):
    """nfmc_flow_fit_epochs_f32 on a spline flow against the same epochs driven one nfmc_flow_fit_step_f32 at a time with
    the bookkeeping of flow_training._loop on the host: same weights bit for bit, same best validation loss, same best
    weights, same epoch of the early stop."""
    from nfmc_amd import hip
    from nfmc_amd.flow_training import DeviceFit
    d, n, nv, lr, thr, epochs = 32, 700, 200, 0.05, 4, 60
    _of, fa = _flow(d, 6, 2, 2, 23)
    fa.to(dev)
    fb = copy.deepcopy(fa)
    g0 = torch.Generator().manual_seed(11)
    x = (torch.randn(n, d, generator=g0) * 0.6 + 0.2).to(dev)
    xv = (torch.randn(nv, d, generator=g0) * 2.5 - 1.0).to(dev)     # validation the training rows say little about: it turns
    a = DeviceFit(fa.bijection, dev, n + nv, lr=lr)
    a.set_validation(xv)
    best, since, applied, best_vec, stop_at = math.inf, 0, 0, a.params.clone(), None
    for c in range(epochs + 1):
        a.step(x, applied, lr=0.0 if c == epochs else lr)
        loss, ok, val = (float(t) for t in a.status.cpu())
        if c > 0:
            if val < best:
                best, since = val, 0
                best_vec.copy_(a.prev)
            else:
                since += 1
                if since > thr:
                    stop_at = c
                    break
        if c == epochs:
            break
        assert ok == 1.0
        applied += 1
    assert stop_at is not None and 5 < stop_at < epochs        # the scenario does stop early
    b = DeviceFit(fb.bijection, dev, n + nv, lr=lr)
    b.set_validation(xv)
    ctl = b.control(epochs, True, thr, True)
    b.run_calls(ctl, x, 0, epochs + 1)
    st = b.state_after(epochs + 1)
    assert st[hip.FIT_STOPPED] == 1.0 and st[hip.FIT_DIVERGED] == 0.0
    assert st[hip.FIT_APPLIED] == applied == stop_at
    np.testing.assert_allclose(st[hip.FIT_BEST_LOSS], best, rtol=0, atol=0)
    assert torch.equal(b.best, best_vec)
    assert torch.equal(b.params, a.prev)            # the stopping call's step is discarded on both sides


def test_spline_device_steps_follow_torch_adamw(dev):
    """The fused AdamW step on a spline flow against torch.optim.AdamW on autograd gradients of flow_training.forward_torch,
    same data, same start: the first step entry by entry wherever the gradient is not negligible, and the loss of every
    one of 25 epochs (flat directions do not move it)."""
    from nfmc_amd.flow_training import DeviceFit, _base_log_prob, forward_torch
    d, n, lr = 24, 600, 0.02
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, d, generator=g) * torch.linspace(0.4, 1.6, d) + 0.3).to(dev)
    _of, fa = _flow(d, 4, 2, 2, 11)
    fa.to(dev)
    fb = copy.deepcopy(fa)
    fit = DeviceFit(fa.bijection, dev, n, lr=lr)
    opt = torch.optim.AdamW(fb.parameters(), lr=lr)
    la, lb = [], []
    for epoch in range(25):
        fit.step(x, epoch)
        la.append(float(fit.status[0]))
        opt.zero_grad()
        z, ld = forward_torch(fb.bijection, x)
        loss = -(_base_log_prob(z) + ld).mean()
        loss.backward()
        if epoch == 0:
            grads = {k: p.grad.detach().clone() for k, p in fb.named_parameters()}
        opt.step()
        lb.append(float(loss.detach()))
        if epoch == 0:
            fit.write_back()
            for (name, pa), (_n, pb) in zip(fa.named_parameters(), fb.named_parameters()):
                gr = grads[name]
                big = gr.abs() > 1e-4 * gr.abs().max()
                assert big.float().mean() > 0.5, name
                np.testing.assert_allclose(pa.detach()[big].cpu().numpy(), pb.detach()[big].cpu().numpy(), atol=2e-6, rtol=0,
                                           err_msg=name)
    la, lb = np.array(la), np.array(lb)
    print('loss device', la[[0, 7, 24]], 'torch', lb[[0, 7, 24]])
    assert la[-1] < la[0] and lb[-1] < lb[0]                              # the loss falls
    np.testing.assert_allclose(la[:8], lb[:8], rtol=1e-3)
    np.testing.assert_allclose(la, lb, rtol=2e-2, atol=5e-2)


@pytest.mark.parametrize('bad', [1e30, float('nan')])
@pytest.mark.parametrize('loss_kind', ['nll', 'reverse_kl'])
def test_spline_run_skips_or_ends_on_a_nonfinite_epoch(dev, loss_kind, bad):
    """The spline twin of test_gpu_fit.py's test_variational_run_skips_or_ends_on_a_nonfinite_epoch, for both losses: the
    third of four batches has one row holding 1e30 (a coordinate in the identity tails whose square overflows) or NaN, so
    its loss is not finite.  The run skips that epoch (weights, AdamW moments and step count untouched) or ends as diverged,
    decided on the device; a following run on finite rows with the same fitter steps normally."""
    from nfmc_amd import hip
    from nfmc_amd.flow_training import DeviceFit
    from nfmc_amd.potentials import SumOfSquares
    d, n = 16, 128
    _of, f = _flow(d, 4, 2, 2, 5)
    f.to(dev)
    pot = SumOfSquares((d,)).descriptor(dev) if loss_kind == 'reverse_kl' else None
    g0 = torch.Generator().manual_seed(4)
    rows = [(torch.randn(n, d, generator=g0)).to(dev) for _ in range(4)]
    rows[2][5, 3] = bad
    for skip in (True, False):
        fit = DeviceFit(f.bijection, dev, n, lr=0.02)
        start = fit.params.clone()
        ctl = fit.control(4, False, 50, True, skip_nonfinite=skip)
        w, moments = [], []
        for c in range(4):
            fit.run_calls(ctl, rows[c], c, 1, pot_struct=pot)
            w.append(fit.params.clone())
            moments.append((fit.m.clone(), fit.v.clone()))
        st = fit.state_after(4)
        assert bool(torch.isfinite(torch.stack(w)).all())
        assert not torch.equal(start, w[0]) and not torch.equal(w[0], w[1])
        assert torch.equal(w[1], w[2])                                    # the non-finite epoch moved nothing
        assert torch.equal(moments[1][0], moments[2][0]) and torch.equal(moments[1][1], moments[2][1])
        if skip:
            assert st[hip.FIT_DIVERGED] == 0.0 and st[hip.FIT_APPLIED] == 3.0 and not torch.equal(w[2], w[3])
        else:
            assert st[hip.FIT_DIVERGED] == 1.0 and st[hip.FIT_APPLIED] == 2.0 and torch.equal(w[2], w[3])
        assert math.isfinite(st[hip.FIT_BEST_LOSS])
        # a fresh run on finite rows
        ctl = fit.control(2, False, 50, True, skip_nonfinite=skip)
        fit.run_calls(ctl, rows[3], 0, 1, pot_struct=pot)
        after = fit.params.clone()
        st = fit.state_after(1)
        assert st[hip.FIT_DIVERGED] == 0.0 and st[hip.FIT_APPLIED] == 1.0 and math.isfinite(st[hip.FIT_LAST_LOSS])
        assert not torch.equal(after, w[3]) and bool(torch.isfinite(after).all())
        assert float((after - w[3]).abs().max()) <= 0.021                 # one AdamW step at lr = 0.02 (+ weight decay)


@pytest.mark.parametrize('bad', [1e30, float('nan')])
def test_spline_fit_raises_on_a_nonfinite_batch_and_keeps_the_weights(dev, bad, monkeypatch):
    """The divergence part of test_device_fit_early_stopping_best_weights_and_divergence for a spline flow: a non-finite
    loss raises ValueError (the only error the samplers catch) and leaves the weights the flow came in with; the next fit
    on finite rows runs.  Both fits are counted on the device path."""
    d = 16
    calls = _count_calls(monkeypatch)
    _of, f = _flow(d, 4, 2, 2, 2)
    f.to(dev)
    x = (torch.randn(256, d, generator=torch.Generator().manual_seed(1)) * 0.5).to(dev)
    before = copy.deepcopy(f.state_dict())
    broken = x.clone()
    broken[3, 2] = bad
    with pytest.raises(ValueError):
        f.fit(broken, n_epochs=5, show_progress=False)
    assert 1 <= len(calls) <= 5                                         # the device run, ended by the non-finite epoch
    for k, v in f.state_dict().items():
        assert torch.equal(v, before[k]), k
    n0 = float(-f.log_prob(x).mean())
    del calls[:]
    f.fit(x, n_epochs=5, lr=0.02, show_progress=False)
    assert len(calls) == 5
    n1 = float(-f.log_prob(x).mean())
    assert math.isfinite(n1) and n1 < n0


# ------------------------------------------------------------------------------------------------ the public paths
def _count_calls(monkeypatch):
    from nfmc_amd import flow_training as ft
    calls = []
    orig = ft.DeviceFit.run_calls
    monkeypatch.setattr(ft.DeviceFit, 'run_calls',
                        lambda self, ctl, xx, c0, k, _o=orig, **kw: (calls.extend(range(c0, c0 + k)), _o(self, ctl, xx, c0, k, **kw))[1])
    return calls


@pytest.mark.parametrize('d', [24, 256])
def test_default_spline_flows_are_supported(dev, d):
    from nfmc_amd.flow_training import DeviceFit
    from nfmc_amd.util import create_flow_object
    f = create_flow_object('c-rqnsf', (d,)).to(dev)
    assert DeviceFit.supported(f.bijection, dev)


def test_spline_flow_fit_api_goes_through_the_device_path(dev, monkeypatch):
    """`Flow.fit(x, x_val=..., n_epochs=25)` on a 'c-rqnsf' flow: 25 epochs + the closing evaluation on the device, none with
    NFMC_FIT_TORCH=1; both end at the same validation NLL, and the flow's sampling kernels read the trained vector."""
    d, n = 24, 1500
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, d, generator=g) * torch.linspace(0.4, 1.6, d) + 0.3
    xv = torch.randn(400, d, generator=g) * torch.linspace(0.4, 1.6, d) + 0.3
    res = []
    for torch_path in ('0', '1'):
        monkeypatch.setenv('NFMC_FIT_TORCH', torch_path)
        with monkeypatch.context() as mp:
            calls = _count_calls(mp)
            _of, f = _flow(d, 4, 2, 2, 11)
            n0 = float(-f.log_prob(xv.to(dev)).mean())
            f.fit(x, x_val=xv, n_epochs=25, lr=0.02, early_stopping=False, keep_best_weights=True, show_progress=False)
            res.append((n0, float(-f.log_prob(xv.to(dev)).mean()), len(calls)))
            if torch_path == '0':
                st = f.bijection.packed(dev)[0]
                assert st.n_bins == 8 and st.spline_bound == f.bijection.spline_bound
                assert st.weights == f.bijection._device_fit.params.data_ptr()      # the trained vector, in place
    (n0, na, ca), (_n0, nb, cb) = res
    print('validation NLL start %.4f device %.4f torch %.4f' % (n0, na, nb))
    assert ca == 26 and cb == 0
    assert na < n0 - 1.0 and nb < n0 - 1.0
    assert abs(na - nb) < 2e-2 * abs(n0 - nb)


@pytest.mark.parametrize('strategy', ['imh', 'neutra_hmc', 'jump_mala'])
def test_sampler_warmups_and_refits_of_a_spline_flow_run_on_the_device(dev, monkeypatch, strategy):
    from nfmc_amd import sample
    from nfmc_amd.potentials import SumOfSquares
    d, n = 12, 64
    calls = _count_calls(monkeypatch)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(0)) * 0.7071
    torch.manual_seed(1)
    fit_kw = {'n_epochs': 6, 'lr': 0.02, 'n_samples': 64, 'early_stopping': False, 'keep_best_weights': True}
    if strategy == 'jump_mala':
        out = sample(SumOfSquares((d,)), strategy=strategy, flow='c-rqnsf', x0=x0, n_iterations=3, show_progress=False, seed=0,
                     inner_param_kwargs={'n_iterations': 4},
                     param_kwargs={'fit_nf': True, 'n_jumps_before_training': 0, 'flow_fit_kwargs': {'n_epochs': 4, 'lr': 0.02}})
    else:
        out = sample(SumOfSquares((d,)), strategy=strategy, flow='c-rqnsf', x0=x0, n_iterations=5, n_warmup_iterations=5,
                     warmup=True, show_progress=False, seed=0, param_kwargs={'warmup_fit_kwargs': fit_kw})
    assert len(calls) >= 1
    s = out.samples
    assert tuple(s.shape[-2:]) == (n, d) and bool(torch.isfinite(s).all())


@pytest.mark.parametrize('d,H', [(24, 16), (300, None)])
def test_spline_flows_beyond_the_kernel_still_fit_through_torch(dev, monkeypatch, d, H):
    """Conditioners wider than 8 and d > 256 are reported unsupported and keep fitting on the torch loop."""
    from nfmc_amd.flow_training import DeviceFit
    from nfmc_amd.util import create_flow_object
    calls = _count_calls(monkeypatch)
    torch.manual_seed(4)
    f = create_flow_object('c-rqnsf', (d,), **({'conditioner_kwargs': {'n_hidden': H}} if H else {})).to(dev)
    assert not DeviceFit.supported(f.bijection, dev)
    x = torch.randn(200, d, generator=torch.Generator().manual_seed(1)) * 0.8
    f.fit(x, n_epochs=2, lr=0.01, show_progress=False)
    assert len(calls) == 0
    assert math.isfinite(float(-f.log_prob(x.to(dev)).mean()))
