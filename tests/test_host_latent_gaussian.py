"""The latent Gaussian model on the host: argument validation (one case per rule), the kernel builders and presets, U and
grad U of the torch potential against the fp64 restatement of tests/latent_gaussian_fp64.py for the 3 likelihoods x 2
parameterisations, the latent / coordinates round trip, the reparameterisation identity, inert unobserved coordinates,
the chunked evaluation, the kernels' data block and descriptor, the header's kind constant, the launch-family routing,
the default layouts of the GPU tests' dimensions and the codes of check_latent (no GPU needed: the entry points answer
a malformed descriptor before they touch a device)."""
import ctypes as C
import math

import pytest
import torch

from latent_gaussian_fp64 import (NU, PAIRS, SCALE, LatentGaussian64, make_pair, problem_data, se_covariance, starts,
                                  truth)
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, LatentGaussianModel, recognize
from nfmc_amd.samplers.common import resolve_target

NAN, INF = float('nan'), float('inf')
K3 = se_covariance(torch.tensor([[0.0, 0.0], [0.5, 0.1], [0.2, 0.9]]), 1.0, 0.5, 0.05)
Y3 = torch.tensor([1.0, 0.0, 2.0])


def _asym():
    k = K3.clone()
    k[0, 1] += 1e-3
    return k


BAD = [
    ('unknown likelihood', dict(likelihood='gamma'), 'likelihood'),
    ('unknown parameterization', dict(parameterization='noncentered'), 'parameterization'),
    ('covariance not square', dict(covariance=K3[:2]), 'square'),
    ('covariance not finite', dict(covariance=K3 * NAN), 'finite'),
    ('covariance not symmetric', dict(covariance=_asym()), 'symmetric'),
    ('covariance indefinite', dict(covariance=K3 - 2.0 * torch.eye(3, dtype=torch.float64)), 'positive definite'),
    ('precision overflows fp32', dict(covariance=K3 * 1e-39), 'fp32'),
    ('y of the wrong length', dict(y=torch.zeros(4)), 'y must have'),
    ('y not finite', dict(y=torch.tensor([1.0, INF, 0.0])), 'y must be finite'),
    ('negative count', dict(y=torch.tensor([1.0, -1.0, 0.0])), 'non-negative integers'),
    ('fractional count', dict(y=torch.tensor([1.0, 0.5, 0.0])), 'non-negative integers'),
    ('binomial y above the trials', dict(likelihood='binomial', y=torch.tensor([1.0, 2.0, 0.0]), weight=1.0), 'y <= trials'),
    ('fractional trials', dict(likelihood='binomial', y=torch.zeros(3), weight=1.5), 'integers'),
    ('negative weight', dict(weight=torch.tensor([1.0, -1.0, 1.0])), 'weight'),
    ('weight not finite', dict(weight=torch.tensor([1.0, NAN, 1.0])), 'weight'),
    ('weight of the wrong length', dict(weight=torch.ones(2)), 'weight'),
    ('mean of the wrong length', dict(mean=torch.zeros(2)), 'mean'),
    ('mean not finite in fp32', dict(mean=1e39), 'mean'),
    ('observed not a bool mask', dict(observed=torch.ones(3)), 'observed'),
    ('observed of the wrong length', dict(observed=torch.ones(4, dtype=torch.bool)), 'observed'),
    ('dof zero', dict(likelihood='student_t', dof=0.0), 'dof'),
    ('dof not finite', dict(likelihood='student_t', dof=INF), 'dof'),
    ('scale negative', dict(likelihood='student_t', scale=-1.0), 'scale'),
    ('scale underflows in fp32', dict(likelihood='student_t', scale=1e-30), 'scale'),
    ('event shape of the wrong size', dict(event_shape=(2, 2)), 'event_shape'),
]


@pytest.mark.parametrize('what,kw,match', BAD, ids=[b[0] for b in BAD])
def test_validation(what, kw, match):
    args = dict(y=Y3, covariance=K3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        LatentGaussianModel(**args)


def test_defaults_and_masters():
    pot = LatentGaussianModel(Y3, K3)
    assert (pot.likelihood, pot.parameterization, pot.whitened, pot.event_shape, pot.dim) == ('poisson', 'whitened', True, (3,), 3)
    assert pot.dof == 4.0 and pot.scale == 1.0
    for v in (pot.y, pot.weight, pot.mean, pot.covariance, pot.cholesky, pot.precision):
        assert v.dtype == torch.float64 and v.device.type == 'cpu'
    torch.testing.assert_close(pot.cholesky @ pot.cholesky.t(), K3, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(pot.precision @ K3, torch.eye(3, dtype=torch.float64), rtol=0, atol=1e-11)
    assert torch.equal(pot.cholesky, torch.tril(pot.cholesky))
    # an unobserved coordinate: weight 0, and its y is dropped (never read)
    q = LatentGaussianModel(torch.tensor([1.0, 7.0, 2.0]), K3, observed=torch.tensor([True, False, True]))
    assert q.weight.tolist() == [1.0, 0.0, 1.0] and q.y.tolist() == [1.0, 0.0, 2.0]
    # a negative count is fine where it is not observed
    LatentGaussianModel(torch.tensor([1.0, -3.0, 2.0]), K3, weight=torch.tensor([1.0, 0.0, 1.0]))


def test_kernel_builders():
    pts = torch.rand(7, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    se = LatentGaussianModel.squared_exponential(pts, 1.7, 0.3, 0.01)
    torch.testing.assert_close(se, se_covariance(pts, 1.7, 0.3, 0.01), rtol=1e-12, atol=1e-14)
    r = torch.cdist(pts, pts)
    a = math.sqrt(3.0) * r / 0.3
    torch.testing.assert_close(LatentGaussianModel.matern32(pts, 1.7, 0.3, 0.01),
                               1.7 * (1 + a) * torch.exp(-a) + 0.01 * torch.eye(7, dtype=torch.float64), rtol=1e-12, atol=1e-14)
    one = LatentGaussianModel.squared_exponential(torch.linspace(0, 1, 5), 1.0, 0.5, 0.0)      # 1-D points
    assert one.shape == (5, 5) and abs(float(one[0, 4]) - math.exp(-2.0)) < 1e-14
    for bad in (dict(variance=0.0), dict(lengthscale=-1.0), dict(jitter=-1e-3), dict(variance=INF)):
        with pytest.raises(ValueError):
            LatentGaussianModel.squared_exponential(pts, **bad)
        with pytest.raises(ValueError):
            LatentGaussianModel.matern32(pts, **bad)
    with pytest.raises(ValueError, match='points'):
        LatentGaussianModel.squared_exponential(torch.zeros(2, 2, 2))


def test_presets():
    counts = torch.tensor([[0, 2, 1], [3, 0, 5]])
    lg = LatentGaussianModel.log_gaussian_cox(counts)
    assert lg.event_shape == (2, 3) and lg.dim == 6 and lg.likelihood == 'poisson' and lg.whitened
    assert torch.equal(lg.y, counts.reshape(-1).double()) and bool((lg.weight == 1.0 / 6).all())
    assert abs(float(lg.mean[0]) - (math.log(11.0) - 1.91 / 2)) < 1e-14
    pts = torch.tensor([[(i + 0.5) / 2, (j + 0.5) / 3] for i in range(2) for j in range(3)], dtype=torch.float64)
    torch.testing.assert_close(lg.covariance, se_covariance(pts, 1.91, 2.0 / 3, 1e-6), rtol=1e-12, atol=1e-14)
    lc = LatentGaussianModel.log_gaussian_cox(counts, parameterization='centered', kernel='matern32', mean=0.5)
    assert not lc.whitened and float(lc.mean[3]) == 0.5
    assert LatentGaussianModel.log_gaussian_cox(torch.zeros(32, 32)).fused_in('mcmc')
    for bad in (torch.zeros(33, 32), torch.zeros(5), torch.zeros(2, 2, 2)):
        with pytest.raises(ValueError, match='grid'):
            LatentGaussianModel.log_gaussian_cox(bad)
    with pytest.raises(ValueError, match='kernel'):
        LatentGaussianModel.log_gaussian_cox(counts, kernel='rbf')
    pts = torch.rand(9, 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    lab = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1, 1])
    gc = LatentGaussianModel.gp_classification(pts, lab, variance=2.0, lengthscale=0.4)
    assert gc.likelihood == 'binomial' and gc.whitened and bool((gc.weight == 1).all()) and torch.equal(gc.y, lab.double())
    torch.testing.assert_close(gc.covariance, se_covariance(pts, 2.0, 0.4, 1e-6), rtol=1e-12, atol=1e-14)
    with pytest.raises(ValueError, match='labels'):
        LatentGaussianModel.gp_classification(pts, lab * 2)


@pytest.mark.parametrize('lik', ['poisson', 'binomial', 'student_t'])
def test_synthetic(lik):
    kw = dict(weight=3.0) if lik == 'binomial' else {}
    pot, tr = LatentGaussianModel.synthetic(20, lik, 5, parameterization='centered', **kw)
    pot2, tr2 = LatentGaussianModel.synthetic(20, lik, 5, parameterization='centered', **kw)
    assert torch.equal(tr, tr2) and torch.equal(pot.y, pot2.y) and tr.shape == (20,) and tr.dtype == torch.float64
    white, tz = LatentGaussianModel.synthetic(20, lik, 5, **kw)
    assert white.whitened and torch.equal(white.y, pot.y)
    torch.testing.assert_close(white.latent(tz), tr, rtol=1e-12, atol=1e-12)     # the same generating f
    assert not torch.equal(LatentGaussianModel.synthetic(20, lik, 6, **kw)[0].y, pot.y)
    assert math.isfinite(float(pot(tr[None])[0]))
    with pytest.raises(ValueError):
        LatentGaussianModel.synthetic(0, lik, 1)
    with pytest.raises(ValueError):
        LatentGaussianModel.synthetic(5, 'gamma', 1)


def _u_and_grad(pot, x, dtype, **kw):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t, **kw)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


@pytest.mark.parametrize('lik,par', PAIRS)
@pytest.mark.parametrize('d', [1, 3, 25, 130])
def test_u_and_gradient_match_the_restatement(lik, par, d):
    data = problem_data(d, lik, 100 + d)
    pot, ref = make_pair(data, par)
    x = starts(data, ref, 17, 3).double()
    u, g = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(u, ref(x), rtol=1e-12, atol=1e-11)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-11, atol=1e-11)
    u32, g32 = _u_and_grad(pot, x, torch.float32)
    assert u32.dtype == torch.float32
    torch.testing.assert_close(u32.double(), ref(x), rtol=2e-5, atol=2e-4 * max(1.0, d / 16))
    # the closed-form Hessian bound against the autograd Hessian
    t = truth(data, ref)
    assert abs(pot.hessian_bound(t) - ref.hessian_lmax(t)) < 1e-8 * ref.hessian_lmax(t)


@pytest.mark.parametrize('lik,par', PAIRS)
def test_latent_coordinates_round_trip_and_helpers(lik, par):
    data = problem_data(12, lik, 7)
    pot, ref = make_pair(data, par, event_shape=(3, 4))
    x = starts(data, ref, 5, 1).double()
    f = pot.latent(x)
    torch.testing.assert_close(f, ref.latent(x), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(pot.coordinates(f), x, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(pot.coordinates(f), ref.coordinates(f), rtol=1e-10, atol=1e-11)
    assert pot.latent(x.reshape(5, 3, 4)).shape == (5, 12) and pot.latent(x[0]).shape == (12,)
    with pytest.raises(ValueError, match='event shape'):
        pot.latent(torch.zeros(5, 11))
    mr = pot.mean_response(x)
    want = {'poisson': pot.weight * torch.exp(f), 'binomial': torch.sigmoid(f), 'student_t': f}[lik]
    torch.testing.assert_close(mr, want, rtol=1e-13, atol=0)
    pd = pot.prior_draws(4000, 3)
    assert pd.shape == (4000, 12) and pd.dtype == torch.float64 and torch.equal(pd, pot.prior_draws(4000, 3))
    fd = pot.latent(pd)
    assert float((fd.mean(0) - pot.mean).abs().max()) < 5 * float(torch.diagonal(pot.covariance).max().sqrt()) / math.sqrt(4000)
    assert float((torch.cov(fd.t()) - pot.covariance).abs().max()) < 0.15
    with pytest.raises(ValueError):
        pot.prior_draws(0, 1)


@pytest.mark.parametrize('lik', ['poisson', 'binomial', 'student_t'])
def test_reparameterized_is_the_same_posterior(lik):
    """U_whitened(z) = U_centred(m + L z) - constant: differences between states agree."""
    data = problem_data(20, lik, 9)
    white, ref = make_pair(data, 'whitened')
    cen = white.reparameterized('centered')
    assert not cen.whitened and cen.likelihood == lik and torch.equal(cen.y, white.y) and torch.equal(cen.weight, white.weight)
    assert torch.equal(cen.covariance, white.covariance) and cen.dof == white.dof and cen.scale == white.scale
    z = starts(data, ref, 9, 2).double()
    f = white.latent(z)
    uw, uc = white(z), cen(f)
    torch.testing.assert_close(uw - uw[0], uc - uc[0], rtol=0, atol=1e-10)
    back = cen.reparameterized('whitened')
    assert torch.equal(back(z), uw)
    with pytest.raises(ValueError, match='parameterization'):
        white.reparameterized('noncentered')


@pytest.mark.parametrize('lik,par', PAIRS)
def test_unobserved_coordinates_are_inert(lik, par):
    """w = 0: the coordinate's data term and its derivative are exactly 0, whatever y and f are -- also where e^f
    overflows."""
    data = problem_data(10, lik, 11)
    pot, ref = make_pair(data, par)
    off = torch.nonzero(~data['observed']).reshape(-1)
    assert off.numel() >= 1
    changed = dict(data)
    changed['y'] = data['y'].clone()
    changed['y'][off] = 3.0
    pot2, _ = make_pair(changed, par)
    x = starts(data, ref, 6, 4).double()
    assert torch.equal(pot(x), pot2(x))
    if par == 'centered':
        # the gradient of the data term at an unobserved coordinate is exactly 0, also at f = 200 (e^f = inf in fp32)
        big = x.float().clone()
        big[:, off] = 200.0
        t = big.detach().requires_grad_(True)
        lik_sum = pot._lik(t, pot.y.float(), pot.weight.float()).sum()
        (g,) = torch.autograd.grad(lik_sum, t)
        assert bool(torch.isfinite(g).all()) and bool((g[:, off] == 0).all())


def test_chunked_call_equals_unchunked(monkeypatch):
    data = problem_data(9, 'binomial', 2)
    pot, ref = make_pair(data, 'whitened')
    x = starts(data, ref, 11, 4).double()
    whole, gw = _u_and_grad(pot, x, torch.float64, chunk=11)
    for chunk in (1, 3, 4, 10, 64):
        u, g = _u_and_grad(pot, x, torch.float64, chunk=chunk)
        torch.testing.assert_close(u, whole, rtol=1e-14, atol=1e-13)
        torch.testing.assert_close(g, gw, rtol=1e-13, atol=1e-13)
    sizes = []
    orig = LatentGaussianModel._u_chunk
    monkeypatch.setattr(LatentGaussianModel, '_u_chunk', lambda s, xf, *a: sizes.append(xf.shape[0]) or orig(s, xf, *a))
    monkeypatch.setattr(LatentGaussianModel, 'CHUNK_FLOATS', 4 * 9)
    pot(x)
    assert sizes == [4, 4, 3]
    with pytest.raises(ValueError, match='chunk'):
        pot(x, chunk=0)


def test_data_block_and_descriptor():
    data = problem_data(5, 'student_t', 3)
    white, _ = make_pair(data, 'whitened')
    A, tab = white.data_block()
    assert A.dtype == torch.float32 and A.shape == (2, 5, 5) and tab.dtype == torch.float32 and tab.shape == (8 + 3 * 8,)
    assert torch.equal(A[0], white.cholesky.t().float()) and torch.equal(A[1], white.cholesky.float())
    assert bool((torch.triu(A[1], 1) == 0).all()) and bool((torch.tril(A[0], -1) == 0).all())
    ns2 = NU * SCALE ** 2
    assert torch.equal(tab[:8], torch.tensor([(NU + 1) / 2, 1 / ns2, ns2, NU + 1, 0, 0, 0, 0], dtype=torch.float64).float())
    for k, v in enumerate((white.mean, white.y, white.weight)):
        assert torch.equal(tab[8 + 8 * k:8 + 8 * k + 5], v.float()) and bool((tab[8 + 8 * k + 5:16 + 8 * k] == 0).all())
    assert white.code() == 6.0
    cen = white.reparameterized('centered')
    A, tab2 = cen.data_block()
    assert A.shape == (5, 5) and torch.equal(A, cen.precision.float()) and torch.equal(tab2, tab) and cen.code() == 2.0
    pois, _ = make_pair(problem_data(8, 'poisson', 3), 'whitened')
    A, tab = pois.data_block()
    assert tab.shape == (8 + 3 * 8,) and bool((tab[:8] == 0).all()) and pois.code() == 4.0
    bino, _ = make_pair(problem_data(8, 'binomial', 3), 'centered')
    assert bino.code() == 1.0


def test_fused_in_table_and_routing():
    pot = LatentGaussianModel(Y3, K3)
    assert {f: pot.fused_in(f) for f in FAMILIES} == {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True,
                                                      'dlmc_step': False, 'fit': False}
    with pytest.raises(ValueError, match='unknown launch family'):
        pot.fused_in('nuts')
    for fam in ('mcmc', 'flow_mh', 'neutra'):
        assert resolve_target(pot, (3,), family=fam) is pot
    for fam in ('imh_parallel', 'dlmc_step', 'fit'):
        assert resolve_target(pot, (3,), family=fam) is None
    eye = torch.eye(1025, dtype=torch.float64)
    assert LatentGaussianModel(torch.zeros(1024), eye[:1024, :1024]).fused_in('mcmc')
    assert not LatentGaussianModel(torch.zeros(1025), eye).fused_in('mcmc')
    assert pot.jump_tail_ok() is True
    # opt-in only: a plain callable with the same values is never taken for the class
    assert recognize(lambda x: pot(x), (3,)) is None


DIMS = [1, 3, 8, 25, 64, 130, 256, 512]          # tests/test_gpu_latent_gaussian.py's grid
LAYOUTS = [(1, (4, 1)), (3, (4, 1)), (5, (4, 2)), (8, (4, 2)), (16, (4, 4)), (20, (4, 8)), (25, (4, 8)), (64, (8, 8)),
           (128, (8, 16)), (130, (8, 32)), (256, (8, 32)), (512, (8, 64)), (1024, (16, 64))]


@pytest.mark.parametrize('d,layout', LAYOUTS, ids=['d%d' % d for d, _ in LAYOUTS])
def test_the_gpu_grid_reaches_every_default_layout(d, layout):
    """The (CPL, LPC) the library's choose_cfg picks for kind 12 at the dimensions of the GPU tests (and at the 32 x 32
    LGCP), asked of the library itself: nfmc_sampler_layout is host arithmetic and needs no device."""
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(d, hip.POT_LATENT_GAUSSIAN, C.byref(cpl), C.byref(lpc)) == 0
    assert (cpl.value, lpc.value) == layout
    assert cpl.value * lpc.value >= d


def test_the_gpu_grid_covers_the_default_layouts():
    """Every default layout of the register kernels is reached by a dimension the GPU file runs: its replay grid, d = 5
    and 20 of the jump and determinism cases, d = 16 of the statistics case and d = 128 of the NeuTra cases; (16, 64) by
    d = 1024, the 32 x 32 LGCP of tools/probe_latent_gaussian.py."""
    by_d = dict(LAYOUTS)
    assert {by_d[d] for d in DIMS + [5, 16, 20]} == {(4, 1), (4, 2), (4, 4), (4, 8), (8, 8), (8, 32), (8, 64)}
    assert by_d[128] == (8, 16) and by_d[1024] == (16, 64)


def _mala_args(d, pot):
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = 4096, 64, d, 2, 0.01, 1      # x: a host value, never read
    a.pot = pot
    a.rng.seed = 3
    return a


def test_check_latent_codes_without_a_device():
    """nfmc_mala_steps_f32 and nfmc_hmc_steps_f32 check their arguments, the descriptor among them, from host values
    before they touch a device, so a malformed kind-12 descriptor is answered here: a NULL a or b, n_components != d and
    an invalid code are EINVAL, a misaligned a or b is EALIGN.  The check's own answer for d > 1024, EUNSUPPORTED, is
    behind the entry points' ESHAPE for the same d, which is what a caller sees."""
    base = 1 << 20                            # a host value: the check never reads what a and b point to
    cases = [((6, 6, 0, base, 4.0), hip.EINVAL), ((6, 6, base, 0, 4.0), hip.EINVAL),
             ((6, 5, base, base, 4.0), hip.EINVAL), ((6, 7, base, base, 4.0), hip.EINVAL),
             ((6, 6, base, base, 3.0), hip.EINVAL), ((6, 6, base, base, 7.0), hip.EINVAL), ((6, 6, base, base, 8.0), hip.EINVAL),
             ((6, 6, base, base, -1.0), hip.EINVAL), ((6, 6, base, base, 0.5), hip.EINVAL), ((6, 6, base, base, NAN), hip.EINVAL),
             ((6, 6, base + 4, base, 4.0), hip.EALIGN), ((6, 6, base, base + 8, 4.0), hip.EALIGN),
             ((6, 6, base + 4, base, 0.0), hip.EALIGN),
             ((1025, 1025, base, base, 4.0), hip.ESHAPE)]
    for (d, nc, a, b, code), want in cases:
        pot = hip.NfmcPotential(hip.POT_LATENT_GAUSSIAN, nc, a or None, b or None, code, 0.0)
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(d, pot)), None)) == want, (d, nc, a, b, code)
        hm = hip.NfmcHmcArgs()
        hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = 4096, 64, d, 2, 0.01, 1, 3
        hm.pot = pot
        hm.rng.seed = 3
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), None)) == want, (d, nc, a, b, code)
    # the order of the check: a malformed descriptor that is also misaligned is EINVAL
    pot = hip.NfmcPotential(hip.POT_LATENT_GAUSSIAN, 5, base + 4, base, 4.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(6, pot)), None)) == hip.EINVAL
