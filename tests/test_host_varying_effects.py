"""Varying-effects regression on the host: U and grad U of the torch potential (which works from the per-group sufficient
statistics) against the model written from torch.distributions over the raw observations (tests/varying_effects_fp64.py)
at all 16 combinations of side, noise and parameterisation, pack / unpack / effects, the seeded synthetic data set, eight
schools, the kernels' table against fp64, relabelled groups, argument validation (one case per rule),
the default layouts of the GPU tests' shapes and the launch-family routing (no GPU needed)."""
import ctypes as C
import itertools

import pytest
import torch

from varying_effects_fp64 import VFX64, model_u64, start_states
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, Potential, VaryingEffectsRegression, recognize
from nfmc_amd.samplers.common import resolve_target

NAN = float('nan')
SIDES = [('varying', 'none'), ('varying', 'shared'), ('varying', 'varying'), ('shared', 'varying')]
COMBOS = [(ia, sl, known, centered) for (ia, sl), known, centered in itertools.product(SIDES, (False, True), (True, False))]


def _model(ia, sl, known, centered, N=23, vector=True):
    kw = dict(intercepts=ia, slopes=sl, centered=centered, location_scale=3.0, scale_scale=1.5)
    if known:
        kw['noise_scale'] = (0.5 + torch.arange(N, dtype=torch.float64) / N) if vector else 0.7
    return kw


def _oracle_kw(pot):
    return dict(y=pot.y, group=pot.group, xcov=pot.x, intercepts=pot.intercepts, slopes=pot.slopes,
                noise_scale=pot.noise_scale, centered=pot.centered, location_scale=pot.location_scale,
                scale_scale=pot.scale_scale)


def _ref(pot):
    kw = _oracle_kw(pot)
    kw['x'] = kw.pop('xcov')
    return VFX64(**kw)


def _states(d, n, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.7 * torch.randn(n, d, generator=g, dtype=torch.float64)


def test_there_are_sixteen_combinations():
    assert len(COMBOS) == 16 and len(set(COMBOS)) == 16


@pytest.mark.parametrize('ia,sl,known,centered', COMBOS)
def test_u_and_grad_match_the_model_over_the_observations(ia, sl, known, centered):
    """C = 5, N = 23: __call__ minus model_u64 is one constant over random states to 1e-9 in fp64, the autograd gradients
    agree, and so do the written-out fp64 U and gradient the GPU tests' oracle samplers use."""
    pot, truth = VaryingEffectsRegression.synthetic(5, 23, 11, **_model(ia, sl, known, centered))
    d = pot.event_size
    assert d == (10 if ia == sl else 5) + (2 if ia == 'varying' else 1) + {'varying': 2, 'shared': 1, 'none': 0}[sl] + (not known)
    assert truth.shape == (d,) and truth.dtype == torch.float64
    x = torch.cat([_states(d, 40, 5), truth[None]]).requires_grad_(True)
    u = pot(x)
    um = model_u64(x, **_oracle_kw(pot))
    diff = (u - um).detach()
    print('U - model: constant %.6f, spread %.2e' % (float(diff.mean()), float(diff.max() - diff.min())))
    assert float(diff.max() - diff.min()) < 1e-9
    (g,) = torch.autograd.grad(u.sum(), x, retain_graph=True)
    (gm,) = torch.autograd.grad(um.sum(), x)
    torch.testing.assert_close(g, gm, rtol=1e-10, atol=1e-10)
    ref = _ref(pot)
    assert ref.d == d
    dr = (ref(x.detach()) - um.detach())
    assert float(dr.max() - dr.min()) < 1e-9
    torch.testing.assert_close(ref.grad(x.detach()), gm, rtol=1e-10, atol=1e-10)
    assert bool((ref.hess_diag(x.detach()) > 0).all())
    # fp32 call on fp32 states: same numbers to fp32 accuracy
    u32 = pot(x.detach().float())
    assert u32.dtype == torch.float32
    torch.testing.assert_close(u32.double(), u.detach(), rtol=2e-5, atol=2e-4)


def test_hessian_diagonal_matches_autograd_where_it_is_exact():
    """Centered parameterisation: hess_diag drops nothing and equals the diagonal of the autograd Hessian."""
    pot, truth = VaryingEffectsRegression.synthetic(4, 15, 3, intercepts='varying', slopes='varying')
    ref = _ref(pot)
    x = start_states(ref, truth, 3, 1)
    for row in x:
        H = torch.autograd.functional.hessian(lambda v: ref(v[None])[0], row)
        torch.testing.assert_close(ref.hess_diag(row[None])[0], torch.diagonal(H), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('ia,sl,known,centered', COMBOS)
def test_pack_unpack_and_effects(ia, sl, known, centered):
    pot, _ = VaryingEffectsRegression.synthetic(3, 9, 2, **_model(ia, sl, known, centered, N=9))
    d, Cn = pot.event_size, 3
    x = _states(d, 4, 9)
    parts = pot.unpack(x)
    want = set(['a' if ia == 'varying' else None, 'b' if sl == 'varying' else None]) - {None} | set(pot.names)
    assert set(parts) == want
    assert torch.equal(pot.pack(**parts), x)
    assert torch.equal(pot.pack(**{k: v[0] for k, v in parts.items()}), x[0])
    # the public layout
    if ia == sl:
        assert torch.equal(parts['a'], x[:, [0, 2, 4]]) and torch.equal(parts['b'], x[:, [1, 3, 5]])
        assert pot.names[:4] == ['mu_a', 's_a', 'mu_b', 's_b'] and torch.equal(parts['s_b'], x[:, 9])
    else:
        assert torch.equal(parts['a' if ia == 'varying' else 'b'], x[:, :3])
    if not known:
        assert pot.names[-1] == 's_y' and torch.equal(parts['s_y'], x[:, -1])
    a, b = pot.effects(x)
    assert a.shape == (4, Cn) and b.shape == (4, Cn)
    for side, mode, got in (('a', ia, a), ('b', sl, b)):
        if mode == 'varying':
            nat = parts[side] if centered else parts['mu_' + side][:, None] + torch.exp(parts['s_' + side])[:, None] * parts[side]
            torch.testing.assert_close(got, nat, rtol=0, atol=0)
        elif mode == 'shared':
            assert torch.equal(got, parts[side][:, None].expand(4, Cn))
        else:
            assert bool((got == 0).all())
    with pytest.raises(ValueError, match='parts'):
        pot.pack(**{k: v for k, v in list(parts.items())[1:]})
    with pytest.raises(ValueError, match='event shape'):
        pot.unpack(x[:, :-1])


def test_synthetic_is_repeatable_per_seed():
    kw = dict(intercepts='varying', slopes='varying')
    p1, t1 = VaryingEffectsRegression.synthetic(6, 40, 7, **kw)
    p2, t2 = VaryingEffectsRegression.synthetic(6, 40, 7, **kw)
    p3, t3 = VaryingEffectsRegression.synthetic(6, 40, 8, **kw)
    assert torch.equal(t1, t2) and torch.equal(p1.y, p2.y) and torch.equal(p1.group, p2.group) and torch.equal(p1.stats, p2.stats)
    assert not torch.equal(p1.y, p3.y)
    assert p1.y.dtype == torch.float64 and p1.n_obs == 40 and p1.n_groups == 6 and p1.event_shape == (17,)
    assert int(torch.bincount(p1.group, minlength=6).min()) >= 1
    pk, _ = VaryingEffectsRegression.synthetic(1, 1, 0)                     # the smallest model
    assert pk.event_shape == (4,)
    with pytest.raises(ValueError, match='n_obs'):
        VaryingEffectsRegression.synthetic(5, 4, 0)


def test_eight_schools():
    pot = VaryingEffectsRegression.eight_schools()
    assert pot.event_shape == (10,) and pot.names == ['mu_a', 's_a'] and pot.known_noise and pot.centered
    y = [28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0]
    sigma = [15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0]
    T = pot.data_block()
    assert T.shape == (8, 8) and T.dtype == torch.float32
    for c in range(8):   # one observation per group: n = 1 / sigma^2, ybar = y, every centred sum 0
        want = torch.tensor([1.0 / sigma[c] ** 2, 0.0, y[c], 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64).float()
        assert torch.equal(T[c], want), (c, T[c])
    nc = VaryingEffectsRegression.eight_schools(centered=False)
    x = _states(10, 5, 1)
    xc = x.clone()
    xc[:, :8] = x[:, 8:9] + torch.exp(x[:, 9:10]) * x[:, :8]
    # same posterior in both parameterisations: U_nc(t) = U_c(theta(t)) - log|d theta / d t| = U_c - 8 s, up to a constant
    diff = nc(x) - (pot(xc) - 8 * x[:, 9])
    assert float(diff.max() - diff.min()) < 1e-10


@pytest.mark.parametrize('ia,sl,known', [('varying', 'varying', False), ('varying', 'none', True), ('shared', 'varying', True)])
def test_data_block_against_fp64(ia, sl, known):
    """The table from plain fp64 loops over the observations (two-pass, centred)."""
    pot, _ = VaryingEffectsRegression.synthetic(7, 60, 4, **_model(ia, sl, known, True, N=60))
    T = pot.data_block()
    assert T.shape == (7, 8) and T.dtype == torch.float32 and T.device.type == 'cpu' and bool((T[:, 6:] == 0).all())
    y, x, g = pot.y.tolist(), pot.x.tolist(), pot.group.tolist()
    om = [1.0] * 60 if not known else [s ** -2 for s in pot.noise_scale.tolist()]
    for c in range(7):
        idx = [i for i in range(60) if g[i] == c]
        n = sum(om[i] for i in idx)
        xb = sum(om[i] * x[i] for i in idx) / n
        yb = sum(om[i] * y[i] for i in idx) / n
        row = [n, xb, yb, sum(om[i] * (x[i] - xb) ** 2 for i in idx), sum(om[i] * (x[i] - xb) * (y[i] - yb) for i in idx),
               sum(om[i] * (y[i] - yb) ** 2 for i in idx)]
        torch.testing.assert_close(pot.stats[c], torch.tensor(row, dtype=torch.float64), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(T[c, :6], torch.tensor(row, dtype=torch.float64).float(), rtol=2e-7, atol=1e-7)
    if sl == 'none':
        assert bool((pot.stats[:, [1, 3, 4]] == 0).all())


def test_relabelling_the_groups_permutes_the_table_and_leaves_u_unchanged():
    pot, _ = VaryingEffectsRegression.synthetic(5, 31, 6, intercepts='varying', slopes='varying')
    perm = torch.tensor([3, 0, 4, 1, 2])                 # old label c becomes perm[c]
    pot2 = VaryingEffectsRegression(pot.y, perm[pot.group], pot.x, intercepts='varying', slopes='varying')
    assert torch.equal(pot2.data_block()[perm], pot.data_block())
    x = _states(15, 6, 3)
    p = pot.unpack(x)
    a2, b2 = torch.empty_like(p['a']), torch.empty_like(p['b'])
    a2[:, perm], b2[:, perm] = p['a'], p['b']
    x2 = pot2.pack(**{**p, 'a': a2, 'b': b2})
    torch.testing.assert_close(pot2(x2), pot(x), rtol=1e-13, atol=1e-12)


Y3, G3, X3 = [1.0, 2.0, 0.5], [0, 1, 0], [0.1, -0.3, 0.7]
BAD = [
    ('y 2-D', dict(y=[[1.0]], group=[0]), 'y must be 1-D'),
    ('y empty', dict(y=[], group=[]), 'y must be 1-D'),
    ('group length', dict(y=Y3, group=[0, 1]), 'group must be 1-D'),
    ('group 2-D', dict(y=Y3, group=[[0, 1, 0]]), 'group must be 1-D'),
    ('group fractional', dict(y=Y3, group=[0.0, 0.5, 1.0]), 'integers'),
    ('group bool', dict(y=Y3, group=[True, False, True]), 'integers'),
    ('group negative', dict(y=Y3, group=[0, -1, 1]), '0 .. C-1'),
    ('empty group', dict(y=Y3, group=[0, 2, 0]), 'empty'),
    ('x missing', dict(y=Y3, group=G3, slopes='varying'), 'x is required'),
    ('x length', dict(y=Y3, group=G3, x=[0.1, 0.2], slopes='shared'), 'x must be 1-D'),
    ('y nan', dict(y=[1.0, NAN, 0.5], group=G3), 'finite'),
    ('x inf', dict(y=Y3, group=G3, x=[0.1, float('inf'), 0.2], slopes='varying'), 'finite'),
    ('no varying side', dict(y=Y3, group=G3, x=X3, intercepts='shared', slopes='shared'), 'varying'),
    ('no varying side, no slope', dict(y=Y3, group=G3, intercepts='shared'), 'varying'),
    ('intercepts none', dict(y=Y3, group=G3, x=X3, intercepts='none', slopes='varying'), 'intercepts'),
    ('slopes unknown', dict(y=Y3, group=G3, x=X3, slopes='fixed'), 'slopes'),
    ('centered not a bool', dict(y=Y3, group=G3, centered=1), 'centered'),
    ('noise zero', dict(y=Y3, group=G3, noise_scale=0.0), 'noise_scale'),
    ('noise negative entry', dict(y=Y3, group=G3, noise_scale=[1.0, -1.0, 1.0]), 'noise_scale'),
    ('noise nan', dict(y=Y3, group=G3, noise_scale=NAN), 'noise_scale'),
    ('noise length', dict(y=Y3, group=G3, noise_scale=[1.0, 1.0]), 'noise_scale'),
    ('noise 2-D', dict(y=Y3, group=G3, noise_scale=[[1.0, 1.0, 1.0]]), 'noise_scale'),
    ('m zero', dict(y=Y3, group=G3, location_scale=0.0), 'location_scale'),
    ('m precision overflows fp32', dict(y=Y3, group=G3, location_scale=1e-25), 'location_scale'),
    ('m precision underflows fp32', dict(y=Y3, group=G3, location_scale=1e25), 'location_scale'),
    ('h negative', dict(y=Y3, group=G3, scale_scale=-1.0), 'scale_scale'),
    ('h inf', dict(y=Y3, group=G3, scale_scale=float('inf')), 'scale_scale'),
    ('h precision overflows fp32', dict(y=Y3, group=G3, scale_scale=1e-25), 'scale_scale'),
    ('table overflows fp32', dict(y=[1e30, -1e30, 2e30], group=G3), 'finite in fp32'),
    ('weights overflow fp32', dict(y=Y3, group=G3, noise_scale=1e-25), 'finite in fp32'),
]


@pytest.mark.parametrize('what,kw,name', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw, name):
    with pytest.raises(ValueError, match=name):
        VaryingEffectsRegression(**kw)


def test_defaults_accepted_edges_and_no_cap_on_d():
    pot = VaryingEffectsRegression(Y3, G3)
    assert (pot.intercepts, pot.slopes, pot.centered, pot.known_noise) == ('varying', 'none', True, False)
    assert (pot.location_scale, pot.scale_scale) == (10.0, 1.0) and isinstance(pot, Potential)
    assert pot.event_shape == (5,) and pot.names == ['mu_a', 's_a', 's_y'] and pot.code == 2
    assert VaryingEffectsRegression(Y3, torch.tensor([0.0, 1.0, 0.0]), X3, slopes='varying', centered=False,
                                    noise_scale=2).code == 2 + 8 + 16 + 32
    assert VaryingEffectsRegression(Y3, G3, X3, intercepts='shared', slopes='varying').code == 1 + 8
    big = VaryingEffectsRegression(torch.zeros(1100), torch.arange(1100))        # d = 1103 > 1024: not an error
    assert big.event_shape == (1103,)
    assert not any(big.fused_in(f) for f in FAMILIES)
    assert resolve_target(big, (1103,), family='mcmc') is None
    edge = VaryingEffectsRegression(torch.zeros(1020), torch.arange(1020), noise_scale=1.0)   # d = 1022
    assert edge.fused_in('mcmc')


# the shapes of tests/test_gpu_varying_effects.py: (intercepts, slopes, C) -> d and the default (CPL, LPC)
LAYOUTS = [('varying', 'varying', 1, 7, (4, 2)), ('varying', 'varying', 2, 9, (4, 4)), ('varying', 'varying', 5, 15, (4, 4)),
           ('varying', 'varying', 6, 17, (4, 8)), ('varying', 'varying', 14, 33, (8, 8)), ('varying', 'varying', 30, 65, (8, 16)),
           ('varying', 'varying', 62, 129, (8, 32)), ('varying', 'varying', 126, 257, (8, 64)),
           ('varying', 'varying', 254, 513, (16, 64)), ('varying', 'varying', 509, 1023, (16, 64)),
           ('varying', 'none', 1, 3, (4, 1)), ('varying', 'none', 2, 4, (4, 1)), ('varying', 'none', 8, 10, (4, 4))]


@pytest.mark.parametrize('ia,sl,Cn,d,layout', LAYOUTS)
def test_the_gpu_grid_reaches_every_default_layout(ia, sl, Cn, d, layout):
    """Asked of the library itself: nfmc_sampler_layout is host arithmetic and needs no device.  The known-noise models
    (eight schools and its C = 1, 2 versions) have d = C + 2."""
    known = sl == 'none'
    pot, _ = VaryingEffectsRegression.synthetic(Cn, 2 * Cn, 0, intercepts=ia, slopes=sl, noise_scale=1.0 if known else None)
    assert pot.event_size == d
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(d, hip.POT_VARYING_EFFECTS, C.byref(cpl), C.byref(lpc)) == 0
    assert (cpl.value, lpc.value) == layout
    if ia == sl:   # both alignments of the five globals: they start on a quad boundary when C is even, mid-quad when odd
        assert (2 * Cn) % 4 == (0 if Cn % 2 == 0 else 2)


def test_fused_in_table_and_routing():
    pot, _ = VaryingEffectsRegression.synthetic(5, 23, 1)
    d = pot.event_size
    assert {f: pot.fused_in(f) for f in FAMILIES} == {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True,
                                                      'dlmc_step': False, 'fit': False}
    with pytest.raises(ValueError, match='unknown launch family'):
        pot.fused_in('nuts')
    for fam in ('mcmc', 'flow_mh', 'neutra'):
        assert resolve_target(pot, (d,), family=fam) is pot
    for fam in ('imh_parallel', 'dlmc_step', 'fit'):
        assert resolve_target(pot, (d,), family=fam) is None
    # opt-in only: a plain callable with the same values is never taken for the class
    assert recognize(lambda x: pot(x), (d,)) is None
