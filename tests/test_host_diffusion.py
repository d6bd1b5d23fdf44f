"""The diffusion bridge on the host: argument validation (one case per rule), U and grad U of the torch potential against
the fp64 loop of tests/diffusion_fp64.py for every drift with fixed and unknown scales, U against the model's log density
from torch.distributions, the closed-form Hessian diagonal of the oracle, the Gaussian counterpart, pack / paths /
scales, prior_draws, the presets, the kernels' view of the data, the launch-family routing, the header's kind constant,
the default layouts of the GPU tests' dimensions and the codes of check_diffusion (no GPU needed: the entry points
answer a malformed descriptor before they touch a device)."""
import ctypes as C

import pytest
import torch

from diffusion_fp64 import COMBOS, MODELS, SCALE_PRIOR, make_pair, model_log_density, problem_data, step_lambda
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, DiffusionBridge, FullRankGaussian, recognize
from nfmc_amd.samplers.common import resolve_target

NAN, INF = float('nan'), float('inf')
Y = torch.tensor([[0.1, 0.2, 0.3], [0.0, NAN, 1.0], [1.0, 2.0, NAN]], dtype=torch.float64)

BAD = [
    ('unknown drift', dict(drift='rossler'), 'drift must be one of'),
    ('one time step', dict(y=Y[:1]), 'T >= 2'),
    ('y of three dimensions', dict(y=torch.zeros(2, 3, 1)), r'\(T, m\)'),
    ('lorenz63 at m = 2', dict(y=Y[:, :2]), 'needs m in'),
    ('fitzhugh_nagumo at m = 3', dict(drift='fitzhugh_nagumo'), 'needs m in'),
    ('cubic at m = 4', dict(y=torch.zeros(3, 4), drift='cubic'), 'needs m in'),
    ('y not finite', dict(y=torch.tensor([[0.0, INF, 0.0], [0.0, 0.0, 0.0]])), 'finite'),
    ('y overflows fp32', dict(y=torch.tensor([[0.0, 1e39, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)), 'fp32'),
    ('observed not a bool mask', dict(observed=torch.ones(3, 3)), 'observed'),
    ('observed of the wrong shape', dict(observed=torch.ones(2, 3, dtype=torch.bool)), 'observed'),
    ('too many drift parameters', dict(drift_params=(1.0, 2.0, 3.0, 4.0)), 'parameters'),
    ('unknown drift parameter', dict(drift_params={'rho': 28.0}), 'parameters'),
    ('drift parameter not finite', dict(drift_params=(10.0, INF, 1.0)), 'drift parameter r'),
    ('dt zero', dict(dt=0.0), 'dt'),
    ('dt not finite', dict(dt=INF), 'dt'),
    ('innovation scale negative', dict(innovation_scale=-0.1), 'innovation_scale'),
    ('innovation scale too small for fp32', dict(innovation_scale=1e-25, dt=1e-3), 'innovation_scale'),
    ('observation scale zero', dict(observation_scale=0.0), 'observation_scale'),
    ('initial scale zero', dict(initial_scale=0.0), 'initial_scale'),
    ('initial mean not finite', dict(initial_mean=NAN), 'initial_mean'),
    ('scale prior not a pair', dict(scale_prior=2.0), 'pair'),
    ('scale prior with c = 0', dict(scale_prior=(0.0, 0.0)), 'scale c'),
    ('scale prior location not finite', dict(scale_prior=(INF, 1.0)), 'location l'),
    ('event shape of the wrong size', dict(event_shape=(3, 2)), 'event_shape'),
    ('event shape without the scales', dict(scale_prior=(0.0, 2.0), event_shape=(3, 3)), 'event_shape'),
]


@pytest.mark.parametrize('name,change,message', BAD, ids=[b[0] for b in BAD])
def test_validation_messages(name, change, message):
    args = dict(y=Y)
    args.update(change)
    with pytest.raises(ValueError, match=message):
        DiffusionBridge(**args)


def test_defaults_and_the_observed_mask():
    pot = DiffusionBridge(Y)
    assert (pot.drift, pot.T, pot.m, pot.dim, pot.event_shape) == ('lorenz63', 3, 3, 9, (9,))
    assert pot.drift_params == (10.0, 28.0, 8.0 / 3.0) and pot.dt == 0.02
    assert pot.n_observed == 7 and not bool(pot.observed[1, 1]) and float(pot.y[1, 1]) == 0.0
    mask = torch.ones(3, 3, dtype=torch.bool)
    mask[0] = False
    assert DiffusionBridge(Y, observed=mask).n_observed == 4                    # NaN and the mask both switch off
    one = DiffusionBridge(torch.tensor([0.0, 1.0, NAN, 2.0]), drift='cubic')
    assert (one.T, one.m, one.dim, one.n_observed) == (4, 1, 4, 3)
    named = DiffusionBridge(Y, drift_params={'r': 20.0})
    assert named.drift_params == (10.0, 20.0, 8.0 / 3.0)
    unk = DiffusionBridge(Y, scale_prior=(0.0, 2.0), event_shape=11)
    assert unk.dim == 11 and unk.scales_unknown and unk.code() == 2 + 4 + 16


def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).clone().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


@pytest.mark.parametrize('unknown', [False, True], ids=['fixed', 'unknown'])
@pytest.mark.parametrize('model,m', COMBOS)
@pytest.mark.parametrize('T', [2, 21])
def test_u_and_gradient_match_the_restatement(T, model, m, unknown):
    data = problem_data(T, m, model, 5 + T, unknown)
    pot, ref = make_pair(data)
    assert pot.dim == ref.d == T * m + (2 if unknown else 0)
    x = pot.prior_draws(6, 3)
    u, g = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(u, ref(x), rtol=1e-12, atol=1e-10)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-11, atol=1e-9)
    u32, _g32 = _u_and_grad(pot, x, torch.float32)
    assert u32.dtype == torch.float32


def test_u_and_gradient_at_the_largest_shape():
    """m = 1, T = 1022 with unknown scales: d = 1024"""
    data = problem_data(1022, 1, 'brownian', 9, True)
    pot, ref = make_pair(data)
    assert pot.dim == 1024 and pot.fused_in('mcmc')
    x = pot.prior_draws(3, 1)
    u, g = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(u, ref(x), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-11, atol=1e-8)


@pytest.mark.parametrize('unknown', [False, True], ids=['fixed', 'unknown'])
@pytest.mark.parametrize('model,m', COMBOS)
def test_u_is_the_models_negative_log_density_up_to_a_constant(model, m, unknown):
    data = problem_data(9, m, model, 4, unknown)
    pot, ref = make_pair(data)
    x = pot.prior_draws(8, 2)
    c = pot(x) + model_log_density(ref, x)
    assert float((c - c[0]).abs().max()) < 1e-9 * (1 + float(pot(x).abs().max()))


@pytest.mark.parametrize('unknown', [False, True], ids=['fixed', 'unknown'])
@pytest.mark.parametrize('model,m', COMBOS)
def test_the_oracles_hessian_diagonal_is_autograds(model, m, unknown):
    data = problem_data(5, m, model, 6, unknown)
    pot, ref = make_pair(data)
    x = pot.prior_draws(3, 4)
    for row in x:
        hess = torch.autograd.functional.hessian(lambda v: ref(v[None]).sum(), row)
        torch.testing.assert_close(ref.hess_diag(row[None])[0], torch.diagonal(hess), rtol=1e-9, atol=1e-9)
    assert step_lambda(ref, x) > 0


@pytest.mark.parametrize('model,m', [('brownian', 1), ('ou', 2), ('ou', 3)])
def test_gaussian_differs_by_a_constant_only(model, m):
    data = problem_data(11, m, model, 4, False)
    pot, _ref = make_pair(data)
    ga = pot.gaussian()
    assert isinstance(ga, FullRankGaussian) and ga.dim == 11 * m and ga.event_shape == pot.event_shape
    x = pot.prior_draws(9, 1)
    diff = ga(x) - pot(x)
    assert float((diff - diff[0]).abs().max()) < 1e-9 * (1 + float(pot(x).abs().max()))
    (ua, gra), (ub, grb) = (_u_and_grad(p, x, torch.float64) for p in (pot, ga))
    torch.testing.assert_close(gra, grb, rtol=1e-9, atol=1e-8)
    prec = ga.precision
    band = (torch.arange(11 * m)[:, None] - torch.arange(11 * m)[None]).abs()
    assert bool((prec[(band != 0) & (band != m)] == 0).all())                   # block tridiagonal with diagonal blocks
    with pytest.raises(ValueError, match='not Gaussian'):
        make_pair(problem_data(5, m, model, 4, True))[0].gaussian()
    with pytest.raises(ValueError, match='not Gaussian'):
        make_pair(problem_data(5, 1, 'cubic', 4, False))[0].gaussian()
    with pytest.raises(ValueError, match='not Gaussian'):
        DiffusionBridge(Y).gaussian()


def test_pack_paths_and_scales_round_trip():
    data = problem_data(7, 3, 'lorenz63', 2, True)
    pot, _ref = make_pair(data)
    x = pot.prior_draws(5, 3)
    X = pot.paths(x)
    sig, tau = pot.scales(x)
    assert X.shape == (5, 7, 3) and sig.shape == tau.shape == (5,)
    assert torch.equal(X[:, 2, 1], x[:, 7]) and torch.equal(sig, torch.exp(x[:, 21])) and torch.equal(tau, torch.exp(x[:, 22]))
    torch.testing.assert_close(pot.pack(X, sig, tau), x, rtol=1e-14, atol=1e-14)
    assert pot.pack(X[0], 0.5, 2.0).shape == (23,)
    with pytest.raises(ValueError, match='needs innovation_scale'):
        pot.pack(X)
    with pytest.raises(ValueError, match='positive'):
        pot.pack(X, -1.0, 1.0)
    with pytest.raises(ValueError, match=r'\(T, m\)'):
        pot.pack(X[:, :6])
    fixed, _ = make_pair(problem_data(7, 1, 'cubic', 2, False), event_shape=(7, 1))
    xf = fixed.prior_draws(4, 1)
    assert torch.equal(fixed.pack(fixed.paths(xf)), xf) and torch.equal(fixed.pack(xf), xf)       # (.., T) is taken as m = 1
    assert torch.equal(fixed.paths(xf.reshape(4, 7, 1)), xf.reshape(4, 7, 1))
    assert torch.equal(fixed(xf.reshape(4, 7, 1)), fixed(xf))
    s, t = fixed.scales(xf)
    assert bool((s == MODELS['cubic']['sigma']).all()) and bool((t == MODELS['cubic']['tau']).all())
    with pytest.raises(ValueError, match='fixed'):
        fixed.pack(xf, 1.0, 1.0)


def test_prior_draws_are_seeded_draws_of_the_prior():
    pot = DiffusionBridge(torch.full((6, 2), NAN), drift='cubic', drift_params=(0.0, 0.0), dt=0.5, innovation_scale=0.4,
                          initial_mean=0.3, initial_scale=0.5)
    a, b = pot.prior_draws(20000, 1), pot.prior_draws(20000, 1)
    assert a.dtype == torch.float64 and a.shape == (20000, 12) and torch.equal(a, b)
    assert not torch.equal(a, pot.prior_draws(20000, 2))
    want = (0.25 + torch.arange(6, dtype=torch.float64) * 0.08).repeat_interleave(2)
    torch.testing.assert_close(a.var(0), want, rtol=0.05, atol=0)
    torch.testing.assert_close(a.mean(0), torch.full((12,), 0.3, dtype=torch.float64), rtol=0, atol=0.03)
    unk = DiffusionBridge(torch.zeros(4, 1), drift='cubic', scale_prior=(-1.0, 0.25))
    x = unk.prior_draws(20000, 3)
    assert x.shape == (20000, 6)
    torch.testing.assert_close(x[:, 4:].mean(0), torch.full((2,), -1.0, dtype=torch.float64), rtol=0, atol=0.01)
    torch.testing.assert_close(x[:, 4:].std(0), torch.full((2,), 0.25, dtype=torch.float64), rtol=0.03, atol=0)
    with pytest.raises(ValueError, match='n must be'):
        unk.prior_draws(0, 1)


def test_presets():
    bm = DiffusionBridge.brownian_motion()
    assert (bm.T, bm.m, bm.dim, bm.drift, bm.drift_params, bm.dt) == (30, 1, 30, 'cubic', (0.0, 0.0), 1.0)
    assert bm.n_observed == 20 and not bool(bm.observed[10:20].any()) and bool(bm.observed[:10].all())
    assert DiffusionBridge.brownian_motion(unknown_scales=True).dim == 32
    assert torch.equal(DiffusionBridge.brownian_motion(seed=3).y, DiffusionBridge.brownian_motion(seed=3).y)
    assert not torch.equal(DiffusionBridge.brownian_motion(seed=3).y, bm.y)
    lz = DiffusionBridge.lorenz_bridge()
    assert (lz.T, lz.m, lz.dim, lz.drift, lz.dt, lz.innovation_scale) == (30, 3, 90, 'lorenz63', 0.02, 0.1)
    assert lz.n_observed == 20 and bool(lz.observed[:10, 0].all()) and bool(lz.observed[20:, 0].all())
    assert not bool(lz.observed[:, 1:].any()) and not bool(lz.observed[10:20].any())
    unk = DiffusionBridge.lorenz_bridge(unknown_scales=True)
    assert unk.dim == 92 and (unk.prior_loc, unk.prior_scale) == (0.0, 2.0)
    dw = DiffusionBridge.double_well_path()
    assert (dw.T, dw.m, dw.dim, dw.drift_params, dw.n_observed) == (64, 1, 64, (1.0, 1.0), 2)
    assert float(dw.y[0, 0]) == -1.0 and float(dw.y[-1, 0]) == 1.0
    pot, truth = DiffusionBridge.synthetic(12, 'fitzhugh_nagumo', 4, scale_prior=(0.0, 2.0))
    assert pot.dim == 26 and truth.shape == (26,) and bool(torch.isfinite(pot(truth[None])).all())
    assert DiffusionBridge.synthetic(5, 'cubic', 1)[0].m == 1
    with pytest.raises(ValueError, match='n_steps'):
        DiffusionBridge.synthetic(1, 'cubic', 1)


def test_unobserved_entries_are_inert():
    data = problem_data(9, 3, 'lorenz63', 5, True)
    pot, _ref = make_pair(data)
    other = dict(data)
    other['y'] = data['y'].clone()
    other['y'][~data['observed']] = 1e30
    pot2, _ = make_pair(other)
    x = pot.prior_draws(5, 1)
    assert torch.equal(pot(x), pot2(x))
    assert torch.equal(pot.data_block()[1], pot2.data_block()[1])


# ------------------------------------------------------------------------------------------------- the kernels' view
def test_data_block_layout():
    data = problem_data(7, 3, 'lorenz63', 2, True)
    pot, _ref = make_pair(data)
    head, rows = pot.data_block()
    mod = MODELS['lorenz63']
    assert head.dtype == rows.dtype == torch.float32 and head.shape == (16,) and rows.shape == (2, 24)
    want = [mod['dt'], 1.0, 1.0, mod['mu0'], 1.0 / mod['s0'] ** 2, SCALE_PRIOR[0], 1.0 / SCALE_PRIOR[1] ** 2,
            float(pot.n_observed), 18.0] + list(mod['par']) + [0.0, 0.0, 0.0, 0.0]
    torch.testing.assert_close(head, torch.tensor(want, dtype=torch.float32), rtol=0, atol=0)
    assert torch.equal(rows[0, :21], pot.y.reshape(-1).float()) and torch.equal(rows[1, :21], pot.observed.reshape(-1).float())
    assert bool((rows[:, 21:] == 0).all())
    fixed, _ = make_pair(problem_data(7, 3, 'lorenz63', 2, False))
    assert fixed.data_block()[0][1:3].tolist() == [pytest.approx(mod['sigma']), pytest.approx(mod['tau'])]


def test_codes():
    codes = {}
    for model, m in COMBOS:
        for unknown in (False, True):
            codes[(model, m, unknown)] = make_pair(problem_data(3, m, model, 3, unknown))[0].code()
    assert codes[('lorenz63', 3, False)] == 18.0 and codes[('lorenz63', 3, True)] == 22.0
    assert codes[('fitzhugh_nagumo', 2, False)] == 9.0 and codes[('fitzhugh_nagumo', 2, True)] == 13.0
    assert codes[('cubic', 1, False)] == 0.0 and codes[('cubic', 3, True)] == 20.0 and codes[('ou', 2, False)] == 8.0


# ------------------------------------------------------------------------------------------------- routing
def test_fused_in_table_and_routing():
    pot = DiffusionBridge(Y)
    assert {f: pot.fused_in(f) for f in FAMILIES} == {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True,
                                                      'dlmc_step': False, 'fit': False}
    with pytest.raises(ValueError, match='unknown launch family'):
        pot.fused_in('nuts')
    for fam in ('mcmc', 'flow_mh', 'neutra'):
        assert resolve_target(pot, (9,), family=fam) is pot
    for fam in ('imh_parallel', 'dlmc_step', 'fit'):
        assert resolve_target(pot, (9,), family=fam) is None
    assert DiffusionBridge(torch.zeros(1024), drift='cubic').fused_in('mcmc')
    assert not DiffusionBridge(torch.zeros(1025), drift='cubic').fused_in('mcmc')
    assert not DiffusionBridge(torch.zeros(1023), drift='cubic', scale_prior=(0.0, 2.0)).fused_in('mcmc')      # d = 1025
    assert DiffusionBridge(torch.zeros(341, 3)).fused_in('mcmc') and not DiffusionBridge(torch.zeros(342, 3)).fused_in('mcmc')
    assert pot.jump_tail_ok() is True
    # opt-in only: a plain callable with the same values is never taken for the class
    assert recognize(lambda x: pot(x), (9,)) is None


LAYOUTS = [(2, (4, 1)), (4, (4, 1)), (6, (4, 2)), (8, (4, 2)), (14, (4, 4)), (24, (4, 8)), (26, (4, 8)), (63, (8, 8)),
           (65, (8, 16)), (100, (8, 16)), (130, (8, 32)), (252, (8, 32)), (500, (8, 64)), (1023, (16, 64)), (1024, (16, 64))]


@pytest.mark.parametrize('d,layout', LAYOUTS, ids=['d%d' % d for d, _ in LAYOUTS])
def test_the_gpu_grid_reaches_every_default_layout(d, layout):
    """The (CPL, LPC) the library's choose_cfg picks for kind 14 at the dimensions of the GPU tests' replay grid, asked of
    the library itself: nfmc_sampler_layout is host arithmetic and needs no device."""
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(d, hip.POT_DIFFUSION_BRIDGE, C.byref(cpl), C.byref(lpc)) == 0
    assert (cpl.value, lpc.value) == layout
    assert cpl.value * lpc.value >= d


def test_the_gpu_grid_covers_the_default_layouts():
    assert {layout for _d, layout in LAYOUTS} == {(4, 1), (4, 2), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64), (16, 64)}
    import test_gpu_diffusion as G
    assert {s[0] for s in G.SHAPES + G.BIG} == {d for d, _ in LAYOUTS}


def _mala_args(d, pot):
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = 4096, 64, d, 2, 0.01, 1      # x: a host value, never read
    a.pot = pot
    a.rng.seed = 3
    return a


def test_check_diffusion_codes_without_a_device():
    """nfmc_mala_steps_f32 and nfmc_hmc_steps_f32 check their arguments, the descriptor among them, from host values
    before they touch a device, so a malformed kind-14 descriptor is answered here: a NULL a or b, T < 2, an invalid
    code, an m that does not fit the drift and d != T m + 2 [unknown] are EINVAL, a misaligned a or b is EALIGN.  The
    check's own answer for d > 1024, EUNSUPPORTED, is behind the entry points' ESHAPE for the same d, which is what a
    caller sees."""
    base = 1 << 20                            # a host value: the check never reads what a and b point to
    cases = [((6, 2, 0, base, 18.0), hip.EINVAL), ((6, 2, base, 0, 18.0), hip.EINVAL),             # NULL a / b
             ((3, 1, base, base, 18.0), hip.EINVAL), ((0, 0, base, base, 0.0), hip.EINVAL),         # T < 2
             ((6, -2, base, base, 18.0), hip.EINVAL),
             ((6, 2, base, base, 19.0), hip.EINVAL), ((6, 6, base, base, 3.0), hip.EINVAL),         # drift code 3
             ((6, 2, base, base, 17.0), hip.EINVAL), ((6, 6, base, base, 1.0), hip.EINVAL),         # fitzhugh_nagumo, m = 3 / 1
             ((6, 3, base, base, 10.0), hip.EINVAL), ((6, 6, base, base, 2.0), hip.EINVAL),         # lorenz63, m = 2 / 1
             ((8, 2, base, base, 24.0), hip.EINVAL), ((6, 2, base, base, 32.0), hip.EINVAL),        # m = 4, past the codes
             ((6, 2, base, base, 18.5), hip.EINVAL), ((6, 2, base, base, -1.0), hip.EINVAL), ((6, 2, base, base, NAN), hip.EINVAL),
             ((7, 2, base, base, 18.0), hip.EINVAL), ((6, 2, base, base, 22.0), hip.EINVAL),        # d != T m (+ 2)
             ((8, 2, base, base, 18.0), hip.EINVAL), ((6, 3, base, base, 18.0), hip.EINVAL),
             ((6, 2, base + 4, base, 18.0), hip.EALIGN), ((8, 2, base, base + 8, 22.0), hip.EALIGN),
             ((4, 2, base + 4, base + 4, 9.0), hip.EALIGN),
             ((1026, 342, base, base, 18.0), hip.ESHAPE)]
    for (d, nc, a, b, code), want in cases:
        pot = hip.NfmcPotential(hip.POT_DIFFUSION_BRIDGE, nc, a or None, b or None, code, 0.0)
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(d, pot)), None)) == want, (d, nc, a, b, code)
        hm = hip.NfmcHmcArgs()
        hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = 4096, 64, d, 2, 0.01, 1, 3
        hm.pot = pot
        hm.rng.seed = 3
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), None)) == want, (d, nc, a, b, code)
    # the order of the check: a malformed descriptor that is also misaligned is EINVAL
    pot = hip.NfmcPotential(hip.POT_DIFFUSION_BRIDGE, 1, base + 4, base, 18.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(3, pot)), None)) == hip.EINVAL
    pot = hip.NfmcPotential(hip.POT_DIFFUSION_BRIDGE, 2, base + 4, base, 19.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(6, pot)), None)) == hip.EINVAL
