"""The trained-spline fixtures (tests/golden/spline_trained_*.npz) and the input sets of tests/test_gpu_spline_trained.py,
checked on the CPU: every fixture is in the sharp regime a fitted spline flow lives in, the knot filter leaves the input
sets nearly whole, and the fp32 floors that the GPU tests turn into tolerances (bound = max(the near-identity test's bound,
12 x floor)) stay under fixed caps, so that the rule cannot hide a failure behind an ill-conditioned input."""
import numpy as np
import pytest
import torch

import spline_fixtures as sf

GRAD_CAP, LOGDET_CAP = 4e-3, 1e-2       # on 12 x floor: of the tensor's scale for fit gradients, absolute for log-dets


@pytest.fixture(scope='module', params=sf.FIXTURES)
def case(request):
    return (request.param,) + sf.inputs(request.param)


def test_fixture_holds_the_recipe_and_the_shape(case):
    name, of, meta, x, z = case
    d = meta['d']
    assert name == 'spline_trained_d%d' % d and x.shape == z.shape == (sf.ROWS[name], d) and 130 <= sf.ROWS[name] <= 300
    assert (meta['n_rows'], meta['n_train'], meta['n_epochs'], meta['lr']) == (1000, 800, 300, 0.05)
    assert all(p.dtype == torch.float32 and bool(torch.isfinite(p).all()) for p in of.parameters())
    with np.load(sf.GOLDEN + '/' + name + '.npz') as f:
        assert float(f['val_loss'][1]) < float(f['val_loss'][0]) - 5.0          # the run did fit the sample
    assert float((x.abs() > 5).any(-1).float().sum()) >= 2 and float((z.abs() > 5).any(-1).float().sum()) >= 2


@pytest.mark.parametrize('inverse', [False, True])
def test_fixture_is_in_the_sharp_regime(case, inverse):
    """fp64 walk over the test rows, each direction on its own: raw conditioner outputs reach +-8, some interior derivative
    sits on the 1e-3 floor and some exceeds 5; nothing saturates (the narrowest bin is 0.1 wide or more)."""
    name, of, _meta, x, z = case
    raw_max, d_lo, d_hi, s_lo, s_hi, w_lo = sf.regime(of, z if inverse else x, inverse)
    print('%s inverse=%d: max|raw| %.1f, derivatives [%.3g, %.3g], slopes [%.3g, %.3g], narrowest bin %.3g'
          % (name, inverse, raw_max, d_lo, d_hi, s_lo, s_hi, 10.0 * w_lo))
    assert raw_max >= 8.0
    assert d_lo <= 2e-3
    assert d_hi >= 5.0
    assert 10.0 * w_lo >= 0.1


@pytest.mark.parametrize('inverse', [False, True])
def test_knot_filter_leaves_the_input_sets_nearly_whole(case, inverse):
    name, of, _meta, x, z = case
    keep, tail = sf.knot_free(of, z if inverse else x, inverse)
    print('%s inverse=%d: removed %.4f, rows with a tail coordinate kept %d' % (name, inverse, 1 - float(keep.float().mean()),
                                                                              int((keep & tail).sum())))
    assert float((~keep).float().mean()) <= 0.10
    assert int((keep & tail).sum()) >= 2


def test_log_det_floors_stay_under_the_cap(case):
    name, of, _meta, x, z = case
    floors = {'forward': sf.floor(sf.forward_fn, of, x)[1], 'inverse': sf.floor(sf.inverse_fn, of, z)[1],
              'log_prob': sf.floor(sf.log_prob_fn, of, x), 'log q': sf.floor(sf.log_q_fn, of, z)}
    print(name, ' '.join('%s %.2e' % kv for kv in floors.items()))
    for what, fl in floors.items():
        assert 0.0 < sf.MARGIN * fl <= LOGDET_CAP, (what, fl)


@pytest.mark.parametrize('target', ['sumsq', 'funnel'])
def test_metropolis_floors_stay_under_the_cap(case, target):
    """The floors the Metropolis check turns into bounds (spline_fixtures.metropolis_oracle): 12 x the log q floor on the
    oracle's proposals, which every entry gets, stays at or below 1e-2; an entry's own floor may exceed that only for the
    few proposals that pass a knot of derivative 1e-3, at most 2 % of the entries; the median entry floor stays under a
    tenth of the cap.  The fp32 restatement's own run meets the bounds."""
    from oracle import potentials as opot, samplers as osamp
    name, of, meta, _x, _z = case
    o = sf.metropolis_oracle(of, meta, target)
    over = sf.MARGIN * o['entry'] > LOGDET_CAP
    print('%s %s: 12 x log q floor %.2e; entry floors median %.2e max %.2e; %d of %d entries over the cap'
          % (name, target, sf.MARGIN * o['fl_q'], float(np.median(o['entry'])), float(o['entry'].max()), int(over.sum()), over.size))
    assert 0.0 < sf.MARGIN * o['fl_q'] <= LOGDET_CAP
    assert over.mean() <= 0.02
    assert sf.MARGIN * float(np.median(o['entry'])) <= 0.1 * LOGDET_CAP
    u = opot.sum_squares if target == 'sumsq' else opot.funnel(3.0)
    tr32 = osamp.imh_sample(o['x0'], u, of, sf.MH_STEPS, noise=osamp.PhiloxNoise(sf.MH_SEED))
    m32 = torch.stack(tr32.masks).numpy()
    agree = np.logical_and.accumulate(np.vstack([np.ones((1, sf.MH_CHAINS), bool), (m32 == o['want_m'])[:-1]]), axis=0)
    err = np.abs(torch.stack(tr32.log_ratios).numpy() - o['want_lr'])
    assert agree.mean() > 0.95 and (err[agree] <= o['tol'][agree]).all(), float((err / o['tol'])[agree].max())


def test_fit_gradient_floors_stay_under_the_cap(case):
    name, of, _meta, x, z = case
    xk, zk = sf.filtered(of, x, False), sf.filtered(of, z, True)
    floors = {'nll': sf.floor(sf.loss_and_grads(sf.nll_loss), of, xk, err=sf.loss_grad_err)}
    for kind in sf.POTENTIALS:
        floors[kind] = sf.floor(sf.loss_and_grads(sf.reverse_kl_loss(kind)), of, zk, err=sf.loss_grad_err)
    print(name, ' '.join('%s loss %.2e grad %.2e' % ((k,) + v) for k, v in floors.items()))
    for what, (fl_loss, fl_grad) in floors.items():
        assert 0.0 < sf.MARGIN * fl_grad <= GRAD_CAP, (what, fl_grad)
        assert sf.MARGIN * fl_loss <= GRAD_CAP, (what, fl_loss)


@pytest.mark.parametrize('name', sf.KNOT_FIXTURES)
@pytest.mark.parametrize('inverse', [False, True])
def test_rows_at_a_knot_sit_on_the_knot_and_their_neighbours_inside_one_bin(name, inverse):
    """The rows of the at-a-knot check: the first coupling's spline input of the chosen coordinate is an interior knot to
    fp32 rounding, the displaced rows pass the knot filter whole, and their fit-gradient floors stay under the cap."""
    of, meta = sf.load(name)
    seed = sf.KNOT_SEEDS[name, inverse]
    rows, lo, hi = sf.knot_rows(of, inverse, seed)
    assert rows.shape == (sf.KNOT_ROWS, meta['d']) and rows.dtype == torch.float32
    keep, _ = sf.knot_free(of, rows, inverse, tol=sf.KNOT_TOL)
    assert not bool(keep.any())                                                 # every row has a point on a knot
    assert int((rows != lo).sum()) == int((rows != hi).sum()) == sf.KNOT_ROWS   # one coordinate per row moved
    for side in (lo, hi):
        keep, _ = sf.knot_free(of, side, inverse, tol=sf.KNOT_TOL)
        assert bool(keep.all())
        for kind in (sf.POTENTIALS if inverse else (None,)):
            loss_fn = sf.reverse_kl_loss(kind) if inverse else sf.nll_loss
            fl_loss, fl_grad = sf.floor(sf.loss_and_grads(loss_fn), of, side, err=sf.loss_grad_err)
            assert sf.MARGIN * fl_grad <= GRAD_CAP and sf.MARGIN * fl_loss <= GRAD_CAP, (kind, fl_loss, fl_grad)
    # the fp32 restatement itself, whichever bins it picks, stays inside the band of valid gradients
    for kind in (sf.POTENTIALS if inverse else (None,)):
        loss_fn = sf.reverse_kl_loss(kind) if inverse else sf.nll_loss
        fl = max(sf.floor(sf.loss_and_grads(loss_fn), of, side, err=sf.loss_grad_err)[1] for side in (lo, hi))
        _loss, grads = sf.loss_and_grads(loss_fn)(of, rows)
        band = sf.knot_band(of, loss_fn, inverse, seed)
        excess = sf.band_excess(grads, band)
        # The band is wide (0.1 to 1.7 of scale) for the tensors the knot touches: the coupling whose spline has the knot and
        # the ElementwiseAffine the sweep reaches after it.  For the other coupling and the other ElementwiseAffine, half of
        # the tensors, both sides give the same gradient to within the 1e-4 displacement, and the check is a tight one.
        widths = sf.band_widths(band)
        narrow = sum(w < 1e-2 for w in widths.values())
        print('%s inverse=%d %s: band narrower than 1e-2 of scale for %d of %d tensors, widest %.2g'
              % (name, inverse, kind, narrow, len(widths), max(widths.values())))
        assert 2 * narrow >= len(widths)
        print('%s inverse=%d %s: floor %.2e bound %.2e fp32 restatement outside the band by %.2e'
              % (name, inverse, kind, fl, sf.bound(3e-4, fl), excess))
        assert excess <= sf.bound(3e-4, fl)
