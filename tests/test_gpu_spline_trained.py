"""The spline-flow kernels on TRAINED splines against fp64 oracles.

Every other GPU test builds its 'c-rqnsf' flow with oracle.flow.perturb_: splines that barely leave the identity (raw
conditioner outputs within +-1.8, interior derivatives in [0.19, 1.9]).  The flows here (tests/golden/spline_trained_*.npz,
made by tests/golden/make_golden_spline.py) were fitted for 300 AdamW epochs to a funnel-plus-two-modes sample, which is
what the kernels see in use from the second refit on: raw outputs to +-25, interior derivatives from the 1e-3 floor to 25,
bin slopes from 0.0035 to 24, while the narrowest bin is still 0.1 wide (nothing saturates, the fp32 restatement stays a
sound reference).  tests/test_host_spline_trained.py asserts that regime on the CPU.  It exercises the softplus at its floor
and at large arguments, the sigmoid chains of rqs_forward_backward / rqs_inverse_backward, rcp(s) at s = 0.004, the
cancellation in d0 + d1 - 2 s, the inverse's discriminant at a derivative of 1e-3, and the cumulative-softmax knot chain
with very unequal masses.

THE TOLERANCE RULE.  For every quantity, bound = max(the bound the near-identity test of that quantity uses, 12 x floor).
The floor is the CPU restatement's own fp32 error on the very input of the check -- `spline_fixtures.floor`: the function
on the float flow against the same on its .double() copy, in the normalisation of the check -- computed on the CPU inside
the test; 12 is the ratio tests/test_gpu_fit_spline.py documents between its bound and that floor (hardware exp / rcp / sqrt
/ log, another summation order).  Nothing is taken from the device.  The host test caps 12 x floor at 4e-3 of scale for the
fit gradients and 1e-2 absolute for the log-dets, so an ill-conditioned input cannot hide a failure.  Every test prints
floor, bound and device error.

Floors measured on the CPU when the fixtures were made (rows: spline_fixtures.inputs; they move by a factor of two
between CPUs, which is why the tests compute them and do not read this table):

    quantity                              d8        d7        d24       d64
    forward z                             1.0e-5    9.8e-6    9.9e-6    7.8e-6
    forward log-det                       2.0e-4    3.5e-5    5.2e-5    2.2e-4
    log_prob                              2.0e-4    3.2e-5    5.3e-5    2.3e-4
    inverse x                             1.2e-5    8.8e-6    3.7e-5    4.1e-5
    inverse log-det                       7.0e-5    9.0e-5    1.3e-4    1.5e-4
    round trip x                          6.3e-2    1.3e-4    9.1e-3    1.2e-2
    round trip log-det                    2.0e-2    3.2e-3    2.5e-2    1.3e-1
    Metropolis: log q of the proposals    2.8e-5    9.1e-5    4.1e-4    7.9e-4
    Metropolis: entry floor, median       1.1e-5    1.1e-5    2.5e-5    6.2e-5
    Metropolis: entry floor, maximum      3.5e-4    2.8e-4    1.2e-2    3.7e-3
    fit gradient / scale, NLL             8.8e-6    1.1e-5    1.2e-5    1.7e-4
    fit gradient / scale, KL sum          1.0e-5    1.1e-4    1.3e-4    1.7e-4
    fit gradient / scale, KL diag         8.1e-6    1.7e-4    1.3e-4    1.7e-4
    fit gradient / scale, KL funnel       5.1e-5    3.3e-5    1.3e-4    1.8e-4
    fit loss / (1 + |loss|), worst        3.5e-7    8.5e-8    7.8e-8    7.1e-8
    NeuTra gradient row, median           1.0e-6    1.2e-6    1.9e-6    3.0e-6
    NeuTra gradient row, maximum          1.3e-4    1.8e-4    2.2e-4    7.1e-4

(The round trip is ill-conditioned by construction: an inverse through a bin of slope 0.0035 multiplies the forward pass's
rounding by 290, through a knot of derivative 1e-3 by 1000.)  The NeuTra floors leave two orders of magnitude under the
unchanged median bound of 2e-4 and a factor 2.8 under the 2e-3 that 97 % of the rows must meet."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import spline_fixtures as sf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module', params=sf.FIXTURES)
def case(request):
    """(name, oracle flow fp32, its fp64 copy, scalars, data rows, latent rows), shared by the tests of a fixture; no test
    changes any of it."""
    of, meta, x, z = sf.inputs(request.param)
    return request.param, of, copy.deepcopy(of).double(), meta, x, z


def _within(what, got, want, atol, rtol, fl):
    """|got - want| <= max(atol + rtol |want|, 12 floor) entry by entry; prints floor, bound and the device error."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    err = (got - want).abs()
    tol = torch.clamp(atol + rtol * want.abs(), min=sf.MARGIN * fl)
    print('%-22s floor %.2e  bound %.2e  device error %.2e  (error / bound %.3f)'
          % (what, fl, sf.bound(atol, fl), float(err.max()), float((err / tol).max())))
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= tol).all()), (what, float(err.max()), float((err / tol).max()))


# ------------------------------------------------------------------------------------ forward / inverse / log_prob kernels
def test_forward_inverse_and_log_prob_match_the_fp64_restatement(dev, case):
    """nfmc_realnvp_forward_f32 / nfmc_realnvp_inverse_f32 with n_bins = 8: z, log-det and log_prob of the data rows, x and
    log-det of the latent rows, every row (values and log-dets are continuous at knots), against the restatement in fp64;
    absolute and relative parts of test_rqs_flow_matches_oracle_and_known_answers, or 12 x floor.  The round trip
    inverse(forward(x)) against x within 12 x the restatement's own fp32 round-trip error: the largest error over the rows,
    and the rows' median and 90th percentile, which the few ill-conditioned rows do not set."""
    name, of, of64, meta, x, z = case
    f = sf.device_flow(of, meta).to(dev)
    with torch.no_grad():
        z64, ld64 = of64.bijection.forward(x.double())
        lp64 = of64.log_prob(x.double())
        xi64, ldi64 = of64.bijection.inverse(z.double())
    fl_z, fl_ld = sf.floor(sf.forward_fn, of, x)
    fl_x, fl_ldi = sf.floor(sf.inverse_fn, of, z)
    fl_lp = sf.floor(sf.log_prob_fn, of, x)
    fl_rtx, fl_rtld = sf.floor(sf.round_trip_fn, of, x)
    print(name)
    zd, ldd = f.bijection.forward(x.to(dev))
    _within('forward z', zd, z64, 2e-4, 1e-4, fl_z)
    _within('forward log-det', ldd, ld64, 1e-3, 1e-4, fl_ld)
    _within('log_prob', f.log_prob(x.to(dev)), lp64, 5e-3, 2e-4, fl_lp)
    xd, ldid = f.bijection.inverse(z.to(dev))
    _within('inverse x', xd, xi64, 5e-4, 1e-4, fl_x)
    _within('inverse log-det', ldid, ldi64, 1e-3, 1e-4, fl_ldi)
    xb, ldb = f.bijection.inverse(zd)
    _within('round trip x', xb, x, 0.0, 0.0, fl_rtx)
    _within('round trip log-det', ldb, -ldd.double(), 0.0, 0.0, fl_rtld)
    # The largest round-trip error belongs to the one or two rows that pass a knot of derivative 1e-3, so the bound above says
    # little about the others.  The rows' median and 90th percentile do not depend on those rows: each within 12 x the
    # restatement's own.
    rx32, rl32 = sf.round_trip_fn(of, x)
    for what, dev_rows, ref_rows in (('round trip x, rows', (xb.cpu() - x).abs().amax(1), rx32.abs().amax(1)),
                                     ('round trip log-det, rows', (ldb + ldd).abs().cpu(), rl32.abs())):
        for q in (0.5, 0.9):
            fl_row, got = float(ref_rows.double().quantile(q)), float(dev_rows.double().quantile(q))
            print('%-22s quantile %.1f: floor %.2e  bound %.2e  device error %.2e' % (what, q, fl_row, sf.MARGIN * fl_row, got))
            assert got <= sf.MARGIN * fl_row, (what, q, got, fl_row)


# ------------------------------------------------------------------------------------------------ flow-proposal Metropolis
@pytest.mark.parametrize('target', ['sumsq', 'funnel'])
def test_flow_metropolis_with_a_trained_spline_matches_the_fp64_oracle(dev, case, target, monkeypatch):
    """The flow-proposal Metropolis step on the register layout (launch_flow_mh), on the one-chain-per-lane kernel
    (NFMC_FLOW_TILE_PATH=1) and on the data-parallel independence sampler (launch_imh_parallel, where imh_parallel_ok),
    in the structure of test_spline_flow_metropolis_on_the_register_layout_matches_oracle: n = 70, T = 5, Philox seed 4242,
    the same decision-agreement shares; the oracle runs in fp64 on the fp32 draws (spline_fixtures.metropolis_oracle).
    Log-ratios on the agreeing prefix: entry (t, i) within max(that test's bound, 12 x the fp32 restatement's log q error
    on the oracle's proposals, 12 x the restatement's own error in log q + U of that entry's proposal and of the state its
    chain carries).  The last term widens single entries only -- a proposal that passes a knot of derivative 1e-3 carries
    6e-4 in x', which U multiplies by the target's gradient -- and the host test caps how many it may widen beyond 1e-2.
    Between two device kernels: max(0.2 x that test's bound, 12 x the entry's own floor)."""
    from nfmc_amd.samplers import imh, jump
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.potentials import Funnel, SumOfSquares
    name, of, _of64, meta, _x, _z = case
    d, n, T = meta['d'], sf.MH_CHAINS, sf.MH_STEPS
    f = sf.device_flow(of, meta)
    pot = SumOfSquares((d,)) if target == 'sumsq' else Funnel((d,), 3.0)
    o = sf.metropolis_oracle(of, meta, target)
    x0, tr, want_lr, want_m, tol, ptol, fl_x = o['x0'], o['trace'], o['want_lr'], o['want_m'], o['tol'], o['ptol'], o['fl_x']
    xtol = sf.bound(5e-5 * max(1.0, d / 64), fl_x)

    def launch(parallel):
        s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=T))
        s.seed = sf.MH_SEED
        run = Run(s, x0)
        logq = torch.empty(n, dtype=torch.float32, device=dev)
        masks = torch.zeros(T, n, dtype=torch.uint8, device=dev)
        lr = torch.zeros(T, n, dtype=torch.float32, device=dev)
        samples = torch.zeros(T, n, d, dtype=torch.float32, device=dev)
        if parallel:
            if not jump.imh_parallel_ok(run, f, pot, logq):
                return None
            jump.launch_imh_parallel(run, f, pot, logq, T, 0, False, run.stats.struct(), samples, masks, lr)
        else:
            assert jump.flow_mh_supported(run, f, pot, logq)
            jump.launch_flow_mh(run, f, pot, logq, T, 0, False, True, run.stats.struct(), samples, masks, lr)
        torch.cuda.synchronize()
        return lr.cpu().numpy(), masks.cpu().numpy().astype(bool), samples.cpu().numpy()

    def prefix(a, b):
        return np.logical_and.accumulate(np.vstack([np.ones((1, n), bool), (a == b)[:-1]]), axis=0)

    got_lr, got_m, got_x = launch(False)
    agree = prefix(got_m, want_m)
    err = np.abs(got_lr - want_lr)
    worst = np.unravel_index(np.argmax(np.where(agree, err / tol, 0.0)), err.shape)
    print('%s %s: accepted %d of %d, max |log-ratio| %.3g; log q floor %.2e, entry floors median %.2e max %.2e; bound %.2e to %.2e, '
          '%d entries widened by their own floor; device error %.2e  (error / bound %.3f, there: floor %.2e bound %.2e error %.2e)'
          % (name, target, int(want_m.sum()), n * T, float(np.abs(want_lr).max()), o['fl_q'], float(np.median(o['entry'])),
             float(o['entry'].max()), float(tol.min()), float(tol.max()), int((o['entry'] > o['fl_q']).sum()), float(err[agree].max()),
             float((err / tol)[agree].max()), float(max(o['fl_q'], o['entry'][worst])), float(tol[worst]), float(err[worst])))
    assert np.isfinite(got_lr).all()
    assert agree.mean() > 0.95
    assert (err[agree] <= tol[agree]).all(), float((err / tol)[agree].max())
    follows = agree[-1] & (got_m[-1] == want_m[-1])
    xerr = np.abs(got_x[-1][follows] - tr.samples[-1].numpy()[follows])
    print('    final states: floor %.2e  bound %.2e  device error %.2e' % (fl_x, xtol, float(xerr.max())))
    assert (xerr <= xtol).all()
    # the one-chain-per-lane kernel family
    monkeypatch.setenv('NFMC_FLOW_TILE_PATH', '1')
    t_lr, t_m, _t_x = launch(False)
    monkeypatch.delenv('NFMC_FLOW_TILE_PATH')
    both = prefix(got_m, t_m)
    assert both.mean() > 0.97
    assert (np.abs(got_lr - t_lr)[both] <= 2 * tol[both]).all()
    t_agree = prefix(t_m, want_m)
    print('    tile path: device error %.2e  (error / bound %.3f)' % (float(np.abs(t_lr - want_lr)[t_agree].max()),
                                                                  float((np.abs(t_lr - want_lr) / tol)[t_agree].max())))
    assert t_agree.mean() > 0.95 and (np.abs(t_lr - want_lr)[t_agree] <= tol[t_agree]).all()
    # the data-parallel independence sampler
    par = launch(True)
    if par is None:
        print('    imh_parallel: not available for this shape')
        return
    p_lr, p_m, p_x = par
    both = prefix(got_m, p_m)
    assert both.mean() > 0.99 and ((got_m == p_m) | ~both).mean() > 0.99
    print('    imh_parallel against the register kernel: difference %.2e  (difference / bound %.3f)'
          % (float(np.abs(p_lr - got_lr)[both].max()), float((np.abs(p_lr - got_lr) / ptol)[both].max())))
    assert (np.abs(p_lr - got_lr)[both] <= ptol[both]).all()
    p_agree = prefix(p_m, want_m)
    assert p_agree.mean() > 0.95 and (np.abs(p_lr - want_lr)[p_agree] <= tol[p_agree]).all()
    follows = both[-1] & (got_m[-1] == p_m[-1])
    assert (np.abs(p_x[-1][follows] - got_x[-1][follows]) <= sf.bound(2e-5 * max(1.0, d / 64), fl_x)).all()


# ---------------------------------------------------------------------------------------- NeuTra potential and gradient
@pytest.mark.parametrize('target', ['sumsq', 'funnel'])
def test_neutra_potential_and_gradient_of_a_trained_spline_match_fp64_autograd(dev, case, target):
    """nfmc_neutra_potential_grad_f32 (rqs_inverse_backward) against fp64 autograd through the restatement of
    NeuTra.adjusted_target, in the form and with the assertions of test_neutra_spline_potential_and_gradient_match_autograd:
    u within 2e-4 (1 + max|u|), at least 97 % of the rows' gradients within 2e-3, the row median below 2e-4."""
    from nfmc_amd import hip
    from nfmc_amd.potentials import Funnel, SumOfSquares
    from oracle import potentials as opot, samplers as osamp
    name, of, of64, meta, _x, z = case
    d, n = meta['d'], z.shape[0]
    f = sf.device_flow(of, meta)
    target_cpu = opot.sum_squares if target == 'sumsq' else opot.funnel(3.0)
    pot = SumOfSquares((d,)) if target == 'sumsq' else Funnel((d,), 3.0)

    def u_and_grad(flow, rows):
        rows = rows.clone().requires_grad_(True)
        u = osamp.neutra_adjusted_target(flow, target_cpu, (d,))(rows)
        g, = torch.autograd.grad(u.sum(), rows)
        return u.detach(), g

    def row_err(g, g_ref):
        return (g.double().cpu() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1))

    u_ref, g_ref = u_and_grad(of64, z.double())
    u32, g32 = u_and_grad(of, z)
    st, _keep = f.bijection.packed(dev)
    pd = pot.descriptor(dev)
    zd = z.to(dev).contiguous()
    u = torch.empty(n, device=dev)
    g = torch.empty(n, d, device=dev)
    hip.check(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(pd), hip.ptr(zd), n, hip.ptr(u), hip.ptr(g),
                                                       hip.stream()), 'neutra_potential_grad')
    torch.cuda.synchronize()
    fl, err = row_err(g32, g_ref), row_err(g, g_ref)
    u_bound = 2e-4 * (1 + float(u_ref.abs().max()))
    print('%s %s: u floor %.2e  bound %.2e  device error %.2e' % (name, target, sf.max_abs(u32, u_ref), u_bound, sf.max_abs(u, u_ref)))
    print('    gradient rows: floor median %.2e max %.2e; bounds 2e-4 (median), 2e-3 (97 %% of rows); device median %.2e max %.2e, '
          'share within 2e-3 %.3f' % (float(fl.median()), float(fl.max()), float(err.median()), float(err.max()),
                                      float((err < 2e-3).float().mean())))
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    np.testing.assert_allclose(u.cpu().numpy(), u_ref.numpy(), atol=u_bound, rtol=0)
    assert (err < 2e-3).float().mean() > 0.97, float((err < 2e-3).float().mean())
    assert float(err.median()) < 2e-4


# ------------------------------------------------------------------------------------------------ device fit gradient
def _fit_step(f, dev, rows, kind):
    """One device step with lr = 0, beta1 = 0, weight decay 0: fit.m is the gradient.  kind None: maximum likelihood."""
    from nfmc_amd.flow_training import DeviceFit
    assert DeviceFit.supported(f.bijection, dev)
    fit = DeviceFit(f.bijection, dev, rows.shape[0], lr=0.0)
    fit.opt.beta1, fit.opt.weight_decay = 0.0, 0.0
    before = fit.params.clone()
    if kind is None:
        fit.step(rows.to(dev), 0)
    else:
        fit.step_variational(rows.to(dev), sf.device_potential(kind, rows.shape[1]).descriptor(dev), 0)
    torch.cuda.synchronize()
    assert torch.equal(fit.params, before)                              # lr = 0: nothing moved
    return fit


@pytest.mark.parametrize('kind', [None] + list(sf.POTENTIALS))
def test_fit_gradient_on_a_trained_spline_matches_fp64_autograd(dev, case, kind):
    """fit_rqs_kernel<4|8, false|true>: loss and gradient of the maximum-likelihood step on the knot-filtered data rows and
    of the reverse-KL step ('sum', 'diag', 'funnel') on the knot-filtered latent rows, against fp64 autograd of the
    restatement; loss within max(3e-5, 12 x floor) relative and absolute, every gradient entry within max(3e-4, 12 x floor)
    of its tensor's largest, the blob's padding exactly zero (spline_fixtures.check_gradient)."""
    name, of, of64, meta, x, z = case
    inverse = kind is not None
    rows = sf.filtered(of, z if inverse else x, inverse)
    loss_fn = sf.reverse_kl_loss(kind) if inverse else sf.nll_loss
    fl_loss, fl_grad = sf.floor(sf.loss_and_grads(loss_fn), of, rows, err=sf.loss_grad_err)
    f = sf.device_flow(of, meta).to(dev)
    fit = _fit_step(f, dev, rows, kind)
    ref = copy.deepcopy(of64)
    e_loss, e_grad = sf.check_gradient(fit, f, ref, loss_fn(ref, rows.double()), dev,
                                       loss_tol=sf.bound(3e-5, fl_loss), grad_tol=sf.bound(3e-4, fl_grad))
    print('%s %s: loss floor %.2e  bound %.2e  device error %.2e | gradient floor %.2e  bound %.2e  device error %.2e  (error / bound %.3f)'
          % (name, kind or 'nll', fl_loss, sf.bound(3e-5, fl_loss), e_loss, fl_grad, sf.bound(3e-4, fl_grad), e_grad,
             e_grad / sf.bound(3e-4, fl_grad)))


# -------------------------------------------------------------------------------------- continued fit from a trained state
def test_continued_fit_from_a_trained_state_follows_the_fp64_run(dev):
    """What a refit does from the second one on: 10 device AdamW epochs at lr = 0.01 from spline_trained_d24 on 600 recipe
    rows with 200 validation rows, against oracle.flow.fit_run in fp64 from the same state -- the batch loss and the
    validation loss of every epoch within 12 x the difference between fit_run in fp32 and in fp64 at that epoch, at least
    1e-4 relative."""
    from nfmc_amd.flow_training import DeviceFit
    from oracle import flow as oflow
    of, meta = sf.load('spline_trained_d24')
    d, epochs, lr = meta['d'], 10, 0.01
    rows = sf.recipe_rows(800, d, 77)
    x, xv = rows[:600].contiguous(), rows[600:].contiguous()
    kw = dict(n_epochs=epochs, lr=lr, keep_best_weights=False)
    t64 = oflow.fit_run(of, x, xv, dtype=torch.float64, **kw)
    t32 = oflow.fit_run(of, x, xv, dtype=torch.float32, **kw)
    f = sf.device_flow(of, meta).to(dev)
    fit = DeviceFit(f.bijection, dev, 800, lr=lr)
    fit.set_validation(xv.to(dev))
    xd = x.to(dev)
    train, val = [], []
    for c in range(epochs + 1):                              # call c reports the batch and validation loss at w_c
        fit.step(xd, c, lr=0.0 if c == epochs else lr)
        loss, ok, v = (float(t) for t in fit.status.cpu())
        assert ok == 1.0
        if c < epochs:
            train.append(loss)
        if c > 0:
            val.append(v)                                    # fit_run's val[e] is taken at w_{e+1}
    for what, got, w64, w32 in (('batch', train, t64.train, t32.train), ('validation', val, t64.val, t32.val)):
        got, w64, w32 = np.array(got), np.array(w64), np.array(w32)
        fl = np.abs(w32 - w64)
        tol = np.maximum(1e-4 * np.abs(w64), sf.MARGIN * fl)
        err = np.abs(got - w64)
        print('%s loss %.4f -> %.4f: floor per epoch %s\n    bound %s\n    device error %s'
              % ((what, w64[0], w64[-1]) + tuple(' '.join('%.1e' % v for v in a) for a in (fl, tol, err))))
        assert np.isfinite(got).all() and (err <= tol).all(), (what, float((err / tol).max()))
    assert t64.train[-1] < t64.train[0]


# ----------------------------------------------------------------------------------------------------- rows at a knot
@pytest.mark.parametrize('name', sf.KNOT_FIXTURES)
@pytest.mark.parametrize('kind', [None] + list(sf.POTENTIALS))
def test_fit_gradient_of_rows_at_a_knot_is_a_valid_one_sided_answer(dev, name, kind):
    """8 rows with one spline input of the first coupling the sweep visits ON an interior knot (spline_fixtures.knot_rows).
    Either neighbouring bin is a correct answer.  The loss is continuous at a knot: it matches the fp64 loss within
    max(3e-5, 12 x floor).  Every gradient entry lies inside the band of valid answers (spline_fixtures.knot_band), widened
    by max(3e-4, 12 x floor) of the tensor's scale, the floor being the fp32 restatement's gradient error on the rows 1e-3
    of a bin to either side.  A `th` just outside [0, 1] going through a log, or a forward sweep and a rebuilt input that
    disagree about the bin, give NaN or a gradient outside the band.

    The band is not the one between the one-sided gradients 1e-3 of a bin away: on these splines the fp64 gradient AT the
    knot lies outside that by up to 13 times the tensor's scale (measured on the CPU; knot_band says why), so no correct
    kernel could meet it.  It is the hull, per row, of the fp64 one-sided limits at the knot and of the gradients 1e-4 of a
    bin to either side, the farthest fp32 rounding of knot and input can move the point.

    What the band is worth: for the coupling whose spline has the knot and the ElementwiseAffine the sweep reaches after it
    (half of the tensors) it is 0.1 to 1.7 of the tensor's scale wide, so there the check catches a non-finite value or a
    gradient of the wrong order and little else; for the other half it is narrower than 1e-2 of scale (the host test asserts
    that share) and the check is as tight as the gradient bound."""
    of, meta = sf.load(name)
    inverse = kind is not None
    seed = sf.KNOT_SEEDS[name, inverse]
    rows, lo, hi = sf.knot_rows(of, inverse, seed)
    loss_fn = sf.reverse_kl_loss(kind) if inverse else sf.nll_loss
    fl_loss = sf.floor(lambda fl_, r: loss_fn(fl_, r).detach(), of, rows, err=lambda a, b: abs(float(a) - float(b)) / (1 + abs(float(b))))
    fl_grad = max(sf.floor(sf.loss_and_grads(loss_fn), of, side, err=sf.loss_grad_err)[1] for side in (lo, hi))
    band = sf.knot_band(of, loss_fn, inverse, seed)
    f = sf.device_flow(of, meta).to(dev)
    fit = _fit_step(f, dev, rows, kind)
    loss_gpu, applied, _val = (float(v) for v in fit.status.cpu())
    assert applied == 1.0
    want = float(loss_fn(copy.deepcopy(of).double(), rows.double()).detach())
    grads = sf.device_gradient(fit, f)
    excess = sf.band_excess(grads, band)
    widths = sf.band_widths(band)
    tight = {k: (band[0][k], band[1][k]) for k, w in widths.items() if w < 1e-2}
    excess_tight = sf.band_excess(grads, ({k: v[0] for k, v in tight.items()}, {k: v[1] for k, v in tight.items()}))
    print('band narrower than 1e-2 of scale for %d of %d tensors; outside those by %.2e' % (len(tight), len(widths), excess_tight))
    e_loss = abs(loss_gpu - want) / (1 + abs(want))
    print('%s %s: loss floor %.2e  bound %.2e  device error %.2e | gradient floor %.2e  bound %.2e  device outside the band by %.2e'
          % (name, kind or 'nll', fl_loss, sf.bound(3e-5, fl_loss), e_loss, fl_grad, sf.bound(3e-4, fl_grad), excess))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and math.isfinite(loss_gpu)
    assert e_loss <= sf.bound(3e-5, fl_loss)
    assert excess <= sf.bound(3e-4, fl_grad)
