"""CPU: the refit's epoch loop (jump.py:139-151, 193-201) of the torch path of `Flow.fit` (flow_training._loop) against the
fp64 restatement `oracle.flow.fit_run`, and the `defer_check` contract of that path.

Tolerances are those of the device AdamW test (tests/test_gpu_fit.py: test_device_steps_follow_torch_adamw): per-epoch
losses to 1e-3 relative for the first 8 epochs, 2e-2 after (fp32 against fp64; flat directions of AdamW drift apart).
Which epoch is best and when the run stops are compared exactly, behind a margin the oracle trace must show first: every
comparison the loop makes (monitored loss against the best so far) is decided by far more than fp32 and fp64 differ by."""
import copy
import math

import numpy as np
import pytest
import torch

D, H = 6, 4
# smallest relative gap between a monitored loss and the best before it that the scenarios must show: 100x what fp32 and
# fp64 differ by over these runs (~1e-6 relative), so the best and stopping epochs cannot flip
MARGIN = 1e-4


def _flows(seed=5):
    from nfmc_amd.flows import Flow, RealNVP
    from oracle import flow as oflow
    ck = {'n_hidden': H, 'n_layers': 2}
    torch.manual_seed(seed)     # nn.Linear's initialisation, before the deterministic perturbation
    of = oflow.perturb_(oflow.Flow(oflow.RealNVP((D,), conditioner_kwargs=ck)), seed, 0.3, 0.8)
    f = Flow(RealNVP((D,), conditioner_kwargs=ck))
    f.load_state_dict(of.state_dict())
    return of, f


def _rows():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(300, D, generator=g) * 0.6 + 0.2
    # validation shifted away from the training rows: its loss turns after ~20 epochs
    xv = torch.randn(120, D, generator=torch.Generator().manual_seed(5)) * 0.7 + 0.6
    return x, xv


def _torch_fit(monkeypatch, f, x, xv, **kw):
    """`Flow.fit` on the torch path, with the losses `_loop` sees recorded per epoch (spy on its loss and validation
    closures) and its return value kept."""
    from nfmc_amd import flow_training as ft
    monkeypatch.setenv('NFMC_FIT_TORCH', '1')
    seen = {'train': [], 'val': [], 'best': None}
    orig = ft._loop

    def spy(flow, loss_fn, val_fn, *a, **k):
        def lf():
            v = loss_fn()
            seen['train'].append(float(v.detach()))
            return v

        def vf():
            v = val_fn()
            seen['val'].append(float(v))
            return v
        seen['best'] = orig(flow, lf, vf if val_fn is not None else None, *a, **k)
        return seen['best']
    monkeypatch.setattr(ft, '_loop', spy)
    pending = f.fit(x, x_val=xv, show_progress=False, defer_check=True, **kw)
    monkeypatch.setattr(ft, '_loop', orig)
    if xv is None:
        seen['val'] = list(seen['train'])       # the batch loss before the step is the monitored loss
    return pending, seen


def _decision_margin(vals):
    """Smallest relative gap between a monitored loss and the best before it (epoch 0 compares with inf)."""
    best, gap = math.inf, math.inf
    for v in vals:
        if math.isfinite(best):
            gap = min(gap, abs(v - best) / abs(best))
        best = min(best, v)
    return gap


def _nll(state, x):
    """Mean NLL of rows x in fp64 under the weights `state` (a state_dict, on any device)."""
    from oracle import flow as oflow
    g = oflow.Flow(oflow.RealNVP((D,), conditioner_kwargs={'n_hidden': H, 'n_layers': 2})).double()
    g.load_state_dict({k: v.detach().cpu().double() for k, v in state.items()})
    with torch.no_grad():
        return float(-g.log_prob(x.double()).mean())


def _compare_epochs(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    np.testing.assert_allclose(got[:8], want[:8], rtol=1e-3)
    np.testing.assert_allclose(got, want, rtol=2e-2)


@pytest.mark.parametrize('case', ['val_early_stop', 'no_val', 'last_weights'])
def test_torch_fit_loop_matches_the_fp64_oracle(monkeypatch, case):
    """Per-epoch batch and monitored losses, best loss, best epoch and stopping epoch of the torch loop against
    `fit_run` in fp64; the weights the fit leaves give the loss the oracle says they should (their validation NLL is the
    best loss with keep_best_weights, the last epoch's monitored loss without)."""
    from oracle import flow as oflow
    of, f = _flows()
    x, xv = _rows()
    if case == 'no_val':
        xv = None
        kw = dict(n_epochs=40, lr=0.01, early_stopping=False, keep_best_weights=True)
    else:
        kw = dict(n_epochs=300, lr=0.02, early_stopping=True, early_stopping_threshold=5,
                  keep_best_weights=case == 'val_early_stop')
    want = oflow.fit_run(of, x, xv, **kw)
    # the scenario: every decision of the oracle's loop is clear by MARGIN; with validation the run stops early
    assert _decision_margin(want.val) > MARGIN, _decision_margin(want.val)
    if case != 'no_val':
        assert want.stopped_at is not None and 8 < want.stopped_at < kw['n_epochs'] - 1
        assert want.best_epoch == want.stopped_at - kw['early_stopping_threshold'] - 1
    else:
        assert want.stopped_at is None and want.best_epoch == kw['n_epochs'] - 1
    pending, seen = _torch_fit(monkeypatch, f, x, xv, **kw)
    _compare_epochs(seen['train'], want.train)
    _compare_epochs(seen['val'], want.val)
    assert int(np.argmin(seen['val'])) == want.best_epoch
    assert len(seen['val']) - 1 == (want.stopped_at if want.stopped_at is not None else kw['n_epochs'] - 1)
    assert abs(pending.result() - want.best_loss) <= 2e-2 * abs(want.best_loss)
    assert pending.result() == seen['best'] == min(seen['val'])
    if case == 'no_val':
        # the best weights are those after the best epoch's step: their batch NLL is below every monitored loss
        assert _nll(f.state_dict(), x) < want.best_loss
        np.testing.assert_allclose(_nll(f.state_dict(), x), _nll(want.state, x), rtol=2e-2)
    elif case == 'val_early_stop':
        np.testing.assert_allclose(_nll(f.state_dict(), xv), pending.result(), rtol=1e-5)
        np.testing.assert_allclose(_nll(f.state_dict(), xv), want.best_loss, rtol=2e-2)
    else:
        np.testing.assert_allclose(_nll(f.state_dict(), xv), seen['val'][-1], rtol=1e-5)
        np.testing.assert_allclose(_nll(f.state_dict(), xv), want.val[-1], rtol=2e-2)
        assert _nll(f.state_dict(), xv) > pending.result()


def test_fit_run_is_the_build_spec():
    """fit_run leaves its argument alone, computes in the requested dtype, falls back to the starting weights when no
    epoch improves, and raises ValueError on a non-finite loss."""
    from oracle import flow as oflow
    of, _f = _flows()
    before = copy.deepcopy(of.state_dict())
    x, xv = _rows()
    tr = oflow.fit_run(of, x, xv, n_epochs=3, lr=0.0)
    assert all(torch.equal(v, before[k]) for k, v in of.state_dict().items())
    assert all(v.dtype == torch.float64 for v in tr.state.values())
    # lr = 0 and weight decay: nothing moves, the first epoch is the best and its weights are the starting ones
    assert tr.best_epoch == 0 and tr.val[0] == tr.val[1] == tr.val[2] == tr.best_loss
    assert all(torch.equal(v, before[k].double()) for k, v in tr.state.items())
    bad = x.clone()
    bad[7, 1] = float('nan')
    with pytest.raises(ValueError):
        oflow.fit_run(of, bad, xv, n_epochs=3)


def test_deferred_torch_fit_returns_a_pending_fit(monkeypatch):
    """`fit(defer_check=True)` on the torch path: a PendingFit whose result() is the best monitored loss the loop
    returned; a NaN training row leaves the same weights as the non-deferred call, and result() raises its ValueError."""
    from nfmc_amd.flow_training import PendingFit
    _of, f = _flows()
    x, xv = _rows()
    pending, seen = _torch_fit(monkeypatch, f, x, xv, n_epochs=12, lr=0.05)
    assert isinstance(pending, PendingFit)
    assert pending.result() == seen['best'] == min(seen['val']) and math.isfinite(pending.result())
    bad = x.clone()
    bad[5, 2] = float('nan')
    _of, fa = _flows()
    fb = copy.deepcopy(fa)
    monkeypatch.setenv('NFMC_FIT_TORCH', '1')
    with pytest.raises(ValueError):
        fa.fit(bad, x_val=xv, n_epochs=4, show_progress=False)
    p = fb.fit(bad, x_val=xv, n_epochs=4, show_progress=False, defer_check=True)
    assert isinstance(p, PendingFit)
    with pytest.raises(ValueError):
        p.result()
    for k, v in fa.state_dict().items():
        assert torch.equal(v, fb.state_dict()[k]), k
    # an empty batch: nothing to fit, nothing to raise
    assert fb.fit(x[:0], defer_check=True).result() == math.inf
