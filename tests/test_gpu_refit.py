"""The refit of the jump proposal inside a run (jump.py:193-201, `fit_nf=True`) and the device fit it runs on, against the
fp64 restatement of the fit loop (`oracle.flow.fit_run`) and the CPU jump loop (`oracle.samplers.jump_sample` with its
`refit` hook), at the reference's default refit keywords (sampling/base.py:55-61).

Tolerances: per-epoch losses 1e-3 relative for the first 8 epochs and 2e-2 after (tests/test_gpu_fit.py:
test_device_steps_follow_torch_adamw); best and stopping epochs exactly, behind a decision margin the oracle trace must show
first (every comparison the loop makes is decided by more than MARGIN relative); transitions of a jump run at 5e-4 for at
least 98 % of the chains (test_gpu_configs.py: C5)."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 10x the relative agreement of the device's loss with the restatement's at one step (test_gpu_fit.py: 2e-5)
MARGIN = 1e-4
REFIT_DEFAULTS = {'early_stopping': True, 'early_stopping_threshold': 50, 'batch_size': 'adaptive', 'show_progress': False}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _flow(d, n_hidden, n_hl, n_layers, seed, nice=False):
    from nfmc_amd.flows import Flow, NICE, RealNVP
    from oracle import flow as oflow
    ck = {'n_hidden': n_hidden, 'n_layers': n_hl}
    torch.manual_seed(seed)
    of = oflow.perturb_(oflow.Flow((oflow.NICE if nice else oflow.RealNVP)((d,), n_layers=n_layers, conditioner_kwargs=ck)),
                        seed, 0.3, 0.8)
    f = Flow((NICE if nice else RealNVP)((d,), n_layers=n_layers, conditioner_kwargs=ck))
    f.load_state_dict(of.state_dict())
    return of, f


def _decision_margin(vals):
    best, gap = math.inf, math.inf
    for v in vals:
        if math.isfinite(best):
            gap = min(gap, abs(v - best) / abs(best))
        best = min(best, v)
    return gap


# one case per fit-kernel family: d, n_hidden, hidden layers, coupling layers, train rows, validation rows, NICE,
# validation shift (away from the training rows, so that the validation loss turns and the run stops early), lr
FIT_CASES = [
    pytest.param(25, 4, 2, 2, 200, 100, False, 0.4, 0.02, id='rows_h4'),
    pytest.param(100, 7, 2, 3, 129, 100, False, 0.4, 0.02, id='rows_h8'),
    pytest.param(64, 6, 2, 2, 4200, 300, False, 1.0, 0.05, id='rows_s4_4096plus'),
    pytest.param(512, 7, 2, 2, 130, 60, False, 0.3, 0.02, id='d512'),
    pytest.param(64, 40, 1, 3, 130, 100, False, 0.3, 0.01, id='mfma_h40'),
    pytest.param(64, 16, 1, 2, 70, 100, False, 0.4, 0.02, id='padded_h16'),
    pytest.param(16, 5, 2, 2, 90, 60, True, 0.4, 0.02, id='nice'),
]


def _fit_rows(d, n, nv, shift, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g) * 0.8
    xv = torch.randn(nv, d, generator=g) * 0.7 + shift
    return x, xv


@pytest.mark.parametrize('d,H,nhl,nl,n,nv,nice,shift,lr', FIT_CASES)
def test_device_fit_run_matches_the_fp64_oracle(dev, monkeypatch, d, H, nhl, nl, n, nv, nice, shift, lr):
    """`Flow.fit(x, x_val, early_stopping=True, keep_best_weights=True)` on the device against `fit_run` in fp64 on the same
    rows and starting weights: the validation loss of every epoch (read with DeviceFit.step, which the suite shows equal to
    the enqueued run bit for bit), the best loss, the best and the stopping epoch, and weights whose validation NLL (forward
    kernel, summed in fp64) is the run's own best loss -- best weights taken from a wrong epoch would not be."""
    from nfmc_amd import flow_training as ft, hip
    from oracle import flow as oflow
    thr, epochs = 5, 300
    of, f = _flow(d, H, nhl, nl, 40 + d + H, nice)
    x, xv = _fit_rows(d, n, nv, shift, 7 + d)
    want = oflow.fit_run(of, x, xv, n_epochs=epochs, lr=lr, early_stopping=True, early_stopping_threshold=thr)
    assert _decision_margin(want.val) > MARGIN, _decision_margin(want.val)
    assert want.stopped_at is not None and 8 < want.stopped_at < epochs - 1
    # the device's per-epoch losses, one step at a time: call c reports the validation loss at w_c (closes epoch c - 1)
    f.to(dev)
    fs = copy.deepcopy(f)
    a = ft.DeviceFit(fs.bijection, dev, n + nv, lr=lr)
    a.set_validation(xv.to(dev))
    xd = x.to(dev)
    val, train = [], []
    for c in range(want.stopped_at + 2):
        a.step(xd, c)
        loss, ok, v = (float(t) for t in a.status.cpu())
        assert ok == 1.0
        train.append(loss)
        if c > 0:
            val.append(v)
    train = train[:-1]
    np.testing.assert_allclose(train[:8], want.train[:8], rtol=1e-3)
    np.testing.assert_allclose(train, want.train, rtol=2e-2)
    np.testing.assert_allclose(val[:8], want.val[:8], rtol=1e-3)
    np.testing.assert_allclose(val, want.val, rtol=2e-2)
    assert int(np.argmin(val)) == want.best_epoch
    # the enqueued run of the API call
    calls = []
    orig = ft.DeviceFit.run_calls
    monkeypatch.setattr(ft.DeviceFit, 'run_calls',
                        lambda self, ctl, xx, c0, k, _o=orig, **kw: (calls.extend(range(c0, c0 + k)), _o(self, ctl, xx, c0, k, **kw))[1])
    f.fit(x, x_val=xv, n_epochs=epochs, lr=lr, early_stopping=True, early_stopping_threshold=thr, keep_best_weights=True,
          show_progress=False)
    monkeypatch.setattr(ft.DeviceFit, 'run_calls', orig)
    st = f.bijection._device_fit.state_after(len(calls))
    assert st[hip.FIT_STOPPED] == 1.0 and st[hip.FIT_DIVERGED] == 0.0
    assert st[hip.FIT_APPLIED] - 1 == want.stopped_at                    # the stopping epoch's step is not kept
    assert st[hip.FIT_BEST_LOSS] == min(val)
    np.testing.assert_allclose(st[hip.FIT_BEST_LOSS], want.best_loss, rtol=2e-2)
    with torch.no_grad():
        nll = float(-f.log_prob(xv.to(dev)).double().mean())
    np.testing.assert_allclose(nll, st[hip.FIT_BEST_LOSS], rtol=1e-5)


# ------------------------------------------------------------------------------------------------ fit_nf inside sample()
def _default_refit_run(strategy, d, n, T, fit_nf, seed=9, **kw):
    from nfmc_amd import sample
    from nfmc_amd.potentials import SumOfSquares
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * 0.7071
    torch.manual_seed(1)
    pk = {'fit_nf': True, 'n_jumps_before_training': 0} if fit_nf else {}
    target = kw.pop('target', SumOfSquares((d,)))
    return sample(target, event_shape=(d,), strategy=strategy, x0=x0, n_iterations=T, show_progress=False, seed=seed,
                  param_kwargs=pk, **kw)


@pytest.mark.parametrize('strategy,fuse', [('jump_mala', 'auto'), ('jump_hmc', 'auto'), ('jump_ula', 'auto'),
                                           ('jump_mh', 'auto'), ('jump_mala', 'never')])
def test_fit_nf_at_the_reference_defaults_runs(dev, monkeypatch, strategy, fuse):
    """`fit_nf=True` with `flow_fit_kwargs` left at its default (early stopping: the refit is read back before it returns):
    the run completes, refits T times on the device, books exact counters, jumps more often than the same run with the
    unfitted flow, and keeps the target's moments.  `fuse='never'` (a plain callable, never recognised) takes the split
    path into the refit block."""
    from nfmc_amd import flow_training as ft
    d, n, T = 16, 256, 3
    runs = []
    orig = ft.DeviceFit.run_calls
    monkeypatch.setattr(ft.DeviceFit, 'run_calls',
                        lambda self, ctl, xx, c0, k, _o=orig, **kw: (runs.append(c0 == 0), _o(self, ctl, xx, c0, k, **kw))[1])
    kw = {'fuse': fuse}
    if fuse == 'never':
        kw['target'] = lambda x: torch.sum(x ** 2, dim=-1)
    out = _default_refit_run(strategy, d, n, T, True, **dict(kw))
    monkeypatch.setattr(ft.DeviceFit, 'run_calls', orig)
    cold = _default_refit_run(strategy, d, n, T, False, **dict(kw))
    assert sum(runs) == T                                   # one device run per outer iteration
    K = {'jump_hmc': 5}.get(strategy, 100)                  # sample.py:161-162, sampling/base.py:31
    st = out.statistics
    assert st.n_attempted_trajectories == n * T * K and st.n_attempted_jumps == n * T
    L = 20
    calls, grads = {'jump_mala': (2, 2), 'jump_ula': (1, 1), 'jump_mh': (2, 0), 'jump_hmc': (2 * L + 2, 2 * L)}[strategy]
    assert st.n_target_calls == calls * n * T * K + 2 * n * T and st.n_target_gradient_calls == grads * n * T * K
    assert st.n_attempted_jumps == cold.statistics.n_attempted_jumps
    assert st.n_accepted_jumps > cold.statistics.n_accepted_jumps + 0.05 * n * T, (st.n_accepted_jumps,
                                                                                  cold.statistics.n_accepted_jumps)
    assert torch.isfinite(out.running_samples.last_sample).all()
    var = float(out.variance.mean())
    # ULA's inner chain is unadjusted: at h = d^(-1/3) on U = |x|^2 it keeps the variance 1 / (2 (1 - h)), not 1/2
    want = 1 / (2 * (1 - d ** (-1 / 3))) if strategy == 'jump_ula' else 0.5
    np.testing.assert_allclose(var, want, rtol=0.1)
    assert float(out.mean.abs().mean()) < 0.1


def test_refit_inside_a_run_piece_by_piece(dev, monkeypatch):
    """jump_mala, T = 3, refits at the default keywords, every piece of jump.py:193-201 checked: the rows handed to refit i
    are the kept inner states of iteration i bit for bit; refit i received exactly the reference's defaults; replaying each
    refit with Flow.fit on a fresh copy of the flow as it was before gives bit for bit the weights the run went on with (the
    resident fitter reused across refits computes what a new one does); and the CPU jump loop on the same Philox streams,
    with those weights loaded at each refit, makes the same transitions."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import jump, mcmc
    from oracle import flow as oflow, potentials as opot, samplers as osamp
    d, n, T, K, seed = 16, 192, 3, 8, 4242
    torch.manual_seed(8)
    of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,))), 5, 0.2, 0.7071)
    f = Flow(RealNVP((d,)))
    f.load_state_dict(of.state_dict())
    x0 = 0.7 * torch.randn(n, d)
    splits, refits, fit_kwargs = [], [], []
    orig_split, orig_refit, orig_fit = jump.train_val_split, jump.JumpNFMC._refit, Flow.fit

    def split_spy(x, **kw):
        xt, xv = orig_split(x, **kw)
        splits.append((x.clone(), xt.clone(), xv.clone()))
        return xt, xv

    def refit_spy(self, flow, x_train, x_val):
        before = {k: v.detach().clone() for k, v in flow.state_dict().items()}
        out = orig_refit(self, flow, x_train, x_val)
        refits.append((before, {k: v.detach().clone() for k, v in flow.state_dict().items()}))
        return out

    def fit_spy(self, x_train, x_val=None, **kw):
        fit_kwargs.append(dict(kw))
        return orig_fit(self, x_train, x_val, **kw)
    monkeypatch.setattr(jump, 'train_val_split', split_spy)
    monkeypatch.setattr(jump.JumpNFMC, '_refit', refit_spy)
    monkeypatch.setattr(Flow, 'fit', fit_spy)
    params = jump.JumpNFMCParameters(n_iterations=T, fit_nf=True, n_jumps_before_training=0, store_samples=True)
    s = jump.JumpMALA((d,), SumOfSquares((d,)), NFMCKernel((d,), flow=f), params, None,
                      mcmc.LangevinParameters(n_iterations=K))
    s.seed = seed
    out = s.sample(x0, show_progress=False)
    monkeypatch.setattr(Flow, 'fit', orig_fit)
    assert len(splits) == len(refits) == len(fit_kwargs) == T
    samples = out.samples.reshape(T * (K + 1), n, d)
    for i in range(T):
        rows, _xt, _xv = splits[i]
        assert torch.equal(rows.reshape(K, n, d).cpu(), samples[i * (K + 1):i * (K + 1) + K])
        assert fit_kwargs[i] == {'defer_check': True, **REFIT_DEFAULTS}
    # each refit replayed on a fresh flow (a fitter of its own) from the weights before it
    for i in range(T):
        _rows, xt, xv = splits[i]
        before, after = refits[i]
        g = Flow(RealNVP((d,)))
        g.load_state_dict({k: v.cpu() for k, v in before.items()})
        g.fit(xt, x_val=xv, **REFIT_DEFAULTS)
        for k, v in g.state_dict().items():
            assert torch.equal(v, after[k]), (i, k)
        assert not all(torch.equal(before[k].to(v.device), v) for k, v in after.items())   # the refit moved the weights
    # the CPU jump loop with the run's refitted weights loaded where it refits
    seen = []

    def hook(i, flow, inner_states):
        seen.append(i)
        flow.load_state_dict({k: v.cpu() for k, v in refits[i][1].items()})
    tr = osamp.jump_sample(x0, opot.sum_squares, of, 'langevin', T, K, d ** (-1 / 3), noise=osamp.PhiloxNoise(seed),
                           refit=hook)
    assert seen == list(range(T)) and tr.n_refits == T
    want = tr.stacked()
    same = (samples - want).abs().amax(dim=(0, 2)) < 5e-4
    assert float(same.float().mean()) >= 0.98, float(same.float().mean())
    np.testing.assert_allclose(samples[:, same].numpy(), want[:, same].numpy(), atol=5e-4, rtol=0)
    st = out.statistics
    assert st.n_attempted_jumps == tr.n_attempted_jumps == n * T
    assert abs(st.n_accepted_jumps - tr.n_accepted_jumps) <= max(3, 0.04 * n * T)
    assert abs(st.n_accepted_trajectories - tr.n_accepted) <= max(3, 0.02 * n * T * K)


# ------------------------------------------------------------------------------------------------ the deferred check
BRANCHES = {'deferred': dict(early_stopping=False), 'early_stopping': dict(early_stopping=True, early_stopping_threshold=5),
            'time_limit': dict(early_stopping=False, time_limit_seconds=600.0)}


def _best_of_sync_fit(monkeypatch, f, x, xv, **kw):
    """`Flow.fit` without defer_check, and the best loss its device run returned (spy on flow_training._fit_device)."""
    from nfmc_amd import flow_training as ft
    got = []
    orig = ft._fit_device
    monkeypatch.setattr(ft, '_fit_device', lambda *a, **k: got.append(orig(*a, **k)) or got[-1])
    try:
        f.fit(x, x_val=xv, show_progress=False, **kw)
    finally:
        monkeypatch.setattr(ft, '_fit_device', orig)
    assert len(got) == 1 and isinstance(got[0], float)
    return got[0]


@pytest.mark.parametrize('branch', list(BRANCHES))
def test_deferred_check_equals_the_synchronous_fit(dev, monkeypatch, branch):
    """On each branch of the device fit: `fit(defer_check=True).result()` is bit for bit the best loss of the same fit made
    without defer_check, and leaves the same weights; a NaN row makes result() raise ValueError and leaves the weights the
    non-deferred call leaves."""
    from nfmc_amd.flow_training import PendingFit
    d = 16
    _of, f = _flow(d, 4, 2, 2, 12)
    f.to(dev)
    x, xv = _fit_rows(d, 400, 100, 0.4, 3)
    kw = dict(n_epochs=80, lr=0.02, **BRANCHES[branch])
    g = copy.deepcopy(f)
    best = _best_of_sync_fit(monkeypatch, g, x, xv, **kw)
    p = f.fit(x, x_val=xv, show_progress=False, defer_check=True, **kw)
    assert isinstance(p, PendingFit)
    assert p.result() == best and math.isfinite(best)
    for k, v in f.state_dict().items():
        assert torch.equal(v, g.state_dict()[k]), k
    bad = x.clone()
    bad[9, 4] = float('nan')
    g = copy.deepcopy(f)
    with pytest.raises(ValueError):
        g.fit(bad, x_val=xv, show_progress=False, **kw)
    p = f.fit(bad, x_val=xv, show_progress=False, defer_check=True, **kw)
    with pytest.raises(ValueError):
        p.result()
    for k, v in f.state_dict().items():
        assert torch.equal(v, g.state_dict()[k]), k


def test_three_pending_fits_each_report_their_own_run(dev, monkeypatch):
    """Three deferred fits on one flow (different rows, each starting from the previous one's weights) before any result():
    each result() equals the best loss of its synchronous counterpart (the same three fits made one after the other
    without defer_check) -- no fit reads another's state."""
    d = 16
    _of, f = _flow(d, 4, 2, 2, 13)
    f.to(dev)
    g = copy.deepcopy(f)
    rows = [_fit_rows(d, 300, 80, 0.2 * (j + 1), 20 + j) for j in range(3)]
    kw = dict(n_epochs=40, lr=0.02, early_stopping=False)
    want = [_best_of_sync_fit(monkeypatch, g, x, xv, **kw) for x, xv in rows]
    assert len(set(want)) == 3
    pending = [f.fit(x, x_val=xv, show_progress=False, defer_check=True, **kw) for x, xv in rows]
    torch.cuda.synchronize()           # every fit's state has reached the host before the first result() looks
    assert [p.result() for p in pending] == want
    for k, v in f.state_dict().items():
        assert torch.equal(v, g.state_dict()[k]), k


@pytest.mark.parametrize('early_stopping', [True, False])
def test_a_diverging_refit_raises_out_of_sample(dev, early_stopping):
    """A refit that diverges inside sample() raises ValueError out of it (jump.py:201 raises), with the default keywords
    (early stopping) and without early stopping (the fully deferred run): not AttributeError, and not silently.  The
    divergence is a non-finite learning rate: NaN arithmetic in the AdamW step."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import SumOfSquares
    d, n = 16, 64
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(3)) * 0.7071
    fk = {**REFIT_DEFAULTS, 'early_stopping': early_stopping, 'lr': float('nan')}
    torch.manual_seed(0)
    with pytest.raises(ValueError, match='diverged'):
        sample(SumOfSquares((d,)), strategy='jump_mala', x0=x0, n_iterations=3, show_progress=False, seed=1,
               inner_param_kwargs={'n_iterations': 10},
               param_kwargs={'fit_nf': True, 'n_jumps_before_training': 0, 'flow_fit_kwargs': fk})
