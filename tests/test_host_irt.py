"""Item-response theory on the host: argument validation (one case per rule), the defaults, U and grad U of the torch
potential against the fp64 loops of tests/irt_fp64.py and the model's log densities, pack / unpack, the seeded synthetic
data set, the kernels' data block entry by entry and the launch-family routing (no GPU needed)."""
import pytest
import torch

from irt_fp64 import IRTFast64, IRTU64, model_u64, prior_draws, start_states
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, ItemResponseTheory, Potential, recognize
from nfmc_amd.samplers.common import resolve_target

NAN = float('nan')
R23 = [[1, 0, 1], [0, 0, 1]]

BAD = [
    ('1-D', dict(responses=[1, 0]), 'responses'),
    ('3-D', dict(responses=[[[1]]]), 'responses'),
    ('no students', dict(responses=torch.zeros(0, 3)), 'responses'),
    ('no questions', dict(responses=torch.zeros(3, 0)), 'responses'),
    ('not a label', dict(responses=[[1, 2, 0], [0, 0, 1]]), '0 or 1'),
    ('fractional', dict(responses=[[1, 0.5, 0], [0, 0, 1]]), '0 or 1'),
    ('inf', dict(responses=[[1, float('inf'), 0], [0, 0, 1]]), '0 or 1'),
    ('mask shape', dict(responses=R23, observed=[[True, False], [True, True]]), 'observed'),
    ('mask not bool', dict(responses=R23, observed=[[1, 0, 1], [1, 1, 1]]), 'observed'),
    ('prior not a pair', dict(responses=R23, mean_ability_prior=0.75), 'mean_ability_prior'),
    ('prior a triple', dict(responses=R23, mean_ability_prior=(0.0, 1.0, 2.0)), 'mean_ability_prior'),
    ('m0 nan', dict(responses=R23, mean_ability_prior=(NAN, 1.0)), 'mean_ability_prior mean'),
    ('m0 overflows fp32', dict(responses=R23, mean_ability_prior=(1e39, 1.0)), 'mean_ability_prior mean'),
    ('sigma_mu zero', dict(responses=R23, mean_ability_prior=(0.0, 0.0)), 'mean_ability_prior scale'),
    ('sigma_mu negative', dict(responses=R23, mean_ability_prior=(0.0, -1.0)), 'mean_ability_prior scale'),
    ('sigma_a zero', dict(responses=R23, ability_scale=0.0), 'ability_scale'),
    ('sigma_a inf', dict(responses=R23, ability_scale=float('inf')), 'ability_scale'),
    ('sigma_a a bool', dict(responses=R23, ability_scale=True), 'ability_scale'),
    ('sigma_a precision overflows fp32', dict(responses=R23, ability_scale=1e-25), 'ability_scale'),
    ('sigma_b nan', dict(responses=R23, difficulty_scale=NAN), 'difficulty_scale'),
    ('sigma_b underflows fp32', dict(responses=R23, difficulty_scale=1e-50), 'difficulty_scale'),
    ('sigma_b precision underflows fp32', dict(responses=R23, difficulty_scale=1e25), 'difficulty_scale'),
    ('sigma_b not a scalar', dict(responses=R23, difficulty_scale=[1.0, 2.0]), 'difficulty_scale'),
]


@pytest.mark.parametrize('what,kw,name', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw, name):
    with pytest.raises(ValueError, match=name):
        ItemResponseTheory(**kw)


def test_defaults_and_accepted_edges():
    pot = ItemResponseTheory(R23)
    assert (pot.mean_ability_mean, pot.mean_ability_scale, pot.ability_scale, pot.difficulty_scale) == (0.75, 1.0, 1.0, 1.0)
    assert pot.n_students == 2 and pot.n_questions == 3
    assert pot.event_shape == (6,) and pot.event_size == 6
    assert isinstance(pot, Potential)
    assert pot.responses.dtype == torch.float64 and bool(pot.observed.all())
    ItemResponseTheory([[0]])
    ItemResponseTheory(torch.tensor([[True, False]]), mean_ability_prior=(torch.tensor(0.5), 2), ability_scale=3)
    # NaN is a missing answer; an entry that is no label is fine where the mask drops it
    p = ItemResponseTheory([[1, NAN, 0], [7, 0, 1]], observed=[[True, True, True], [False, True, True]])
    assert p.observed.tolist() == [[True, False, True], [False, True, True]]
    assert p.responses.tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    assert ItemResponseTheory(torch.zeros(700, 322)).event_shape == (1023,)


def _problem(S, Q, seed, **prior):
    pot, truth = ItemResponseTheory.synthetic(S, Q, seed, **prior)
    kw = dict(mean_ability_prior=(pot.mean_ability_mean, pot.mean_ability_scale), ability_scale=pot.ability_scale,
              difficulty_scale=pot.difficulty_scale)
    return pot, truth, IRTU64(pot.responses, pot.observed, **kw), kw


def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


@pytest.mark.parametrize('S,Q', [(1, 1), (2, 2), (5, 3), (16, 8), (30, 20), (1, 23), (23, 1)])
@pytest.mark.parametrize('prior', [{}, dict(mean_ability_prior=(-0.4, 0.5), ability_scale=2.0, difficulty_scale=0.7)])
def test_u_and_grad_match_the_fp64_loops_and_the_model(S, Q, prior):
    pot, truth, ref, kw = _problem(S, Q, S + Q, **prior)
    x = start_states(ref, truth, 12, 3) * 1.5
    u, g = _u_and_grad(pot, x, torch.float64)
    assert u.dtype == torch.float64 and u.shape == (12,)
    torch.testing.assert_close(u, ref(x), rtol=1e-12, atol=1e-11)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-11, atol=1e-11)
    m = model_u64(x, pot.responses, pot.observed, **kw)
    diff = m - ref(x)                                    # one constant: the normalisers of the three priors
    torch.testing.assert_close(diff, diff[0].expand_as(diff), rtol=0, atol=1e-10)
    u32, g32 = _u_and_grad(pot, x, torch.float32)
    assert u32.dtype == torch.float32
    torch.testing.assert_close(u32.double(), ref(x), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(g32.double(), ref.grad(x), rtol=1e-4, atol=1e-4)
    fast = IRTFast64(pot.responses, pot.observed, **kw)  # the tensor form the GPU tests use at large shapes
    torch.testing.assert_close(fast(x), ref(x), rtol=1e-13, atol=1e-12)
    torch.testing.assert_close(fast.grad(x), ref.grad(x), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fast.hess_diag(x), ref.hess_diag(x), rtol=1e-12, atol=1e-12)


def test_loop_gradient_and_hessian_match_autograd():
    pot, truth, ref, _ = _problem(6, 4, 11)
    x = start_states(ref, truth, 5, 1)
    t = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(ref(t).sum(), t, create_graph=True)
    torch.testing.assert_close(g.detach(), ref.grad(x), rtol=1e-12, atol=1e-12)
    hd = torch.stack([torch.autograd.grad(g[:, c].sum(), t, retain_graph=True)[0][:, c] for c in range(ref.d)], dim=1)
    torch.testing.assert_close(hd, ref.hess_diag(x), rtol=1e-11, atol=1e-12)


def test_stable_in_the_tails():
    pot = ItemResponseTheory([[1, 0], [0, 1]])
    x = torch.tensor([[300.0, -300.0, 200.0, -200.0, 100.0], [-300.0, 300.0, -200.0, 200.0, -100.0]], dtype=torch.float64)
    u, g = _u_and_grad(pot, x, torch.float64)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    torch.testing.assert_close(u, IRTU64([[1, 0], [0, 1]])(x), rtol=1e-13, atol=0)


def test_softplus_is_exact_above_20():
    """l_sq from 18 to 34: log1p(e^-l) is 2e-9 at l = 20 and 2e-15 at 34, which a softplus that turns into the identity
    above a threshold loses in U (about 800 here: 2e-12 of it at l = 20), and 1 - sigmoid(l) the same in the gradient.  Against the fp64 loops, whose softplus is
    max(l, 0) + log1p(e^-|l|)."""
    R = [[0, 1], [1, 0]]
    pot, ref = ItemResponseTheory(R), IRTU64(R)
    l = torch.linspace(18.0, 34.0, 12, dtype=torch.float64)
    x = torch.zeros(12, 5, dtype=torch.float64)
    x[:, 4] = l                                          # alpha = beta = 0: every l_sq = mu
    u, g = _u_and_grad(pot, x, torch.float64)
    prior = 0.5 * (l - 0.75) ** 2
    want = 4 * torch.log1p(torch.exp(-l)) + 2 * l        # two answers 0: softplus(l); two answers 1: softplus(l) - l
    torch.testing.assert_close(u, prior + want, rtol=1e-14, atol=0)
    torch.testing.assert_close(u, ref(x), rtol=1e-14, atol=0)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-13, atol=1e-15)
    # alpha_0's gradient: p_a 0 + (sigmoid(l) - 0) + (sigmoid(l) - 1), not 1 + 0 = 1
    assert bool((g[:, 0] < 1.0).all())


@pytest.mark.parametrize('S,Q,layout', [(1, 1, (4, 1)), (2, 2, (4, 2)), (5, 3, (4, 4)), (16, 8, (4, 8)), (30, 20, (8, 8)),
                                        (60, 40, (8, 16)), (200, 54, (8, 32)), (300, 100, (8, 64)), (700, 322, (16, 64)),
                                        (400, 100, (8, 64))])
def test_the_gpu_grid_reaches_every_default_layout(S, Q, layout):
    """The (CPL, LPC) the library's choose_cfg picks for kind 9 at each shape of the GPU tests' grid (and at the
    Inference Gym's), asked of the library itself: nfmc_sampler_layout is host arithmetic and needs no device."""
    import ctypes as C
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(S + Q + 1, hip.POT_ITEM_RESPONSE, C.byref(cpl), C.byref(lpc)) == 0
    assert (cpl.value, lpc.value) == layout


def test_sampler_layout_refusals():
    import ctypes as C
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    f = hip.lib().nfmc_sampler_layout
    assert f(0, hip.POT_ITEM_RESPONSE, C.byref(cpl), C.byref(lpc)) == hip.EINVAL
    assert f(9, hip.POT_ITEM_RESPONSE, None, C.byref(lpc)) == hip.EINVAL
    assert f(1025, hip.POT_ITEM_RESPONSE, C.byref(cpl), C.byref(lpc)) == hip.ESHAPE
    assert f(9, 99, C.byref(cpl), C.byref(lpc)) == hip.EUNSUPPORTED
    assert (cpl.value, lpc.value) == (0, 0)


def test_all_missing_mask_leaves_the_prior():
    S, Q = 4, 3
    kw = dict(mean_ability_prior=(1.5, 0.5), ability_scale=2.0, difficulty_scale=0.25)
    x = prior_draws(S, Q, 9, 5, **kw)
    want = ((x[:, S + Q] - 1.5) ** 2 / (2 * 0.25) + (x[:, :S] ** 2).sum(1) / (2 * 4.0)
            + (x[:, S:S + Q] ** 2).sum(1) / (2 * 0.0625))
    for pot in (ItemResponseTheory(torch.ones(S, Q), observed=torch.zeros(S, Q, dtype=torch.bool), **kw),
                ItemResponseTheory(torch.full((S, Q), NAN), **kw)):
        torch.testing.assert_close(pot(x), want, rtol=1e-13, atol=1e-13)
        assert bool((pot.data_block() == -1).all())


def test_pack_and_unpack():
    pot = ItemResponseTheory(torch.zeros(3, 2))
    x = torch.arange(12, dtype=torch.float64).reshape(2, 6)
    mu, a, b = pot.unpack(x)
    assert mu.tolist() == [5.0, 11.0] and a.shape == (2, 3) and b.shape == (2, 2)
    assert a[1].tolist() == [6.0, 7.0, 8.0] and b[1].tolist() == [9.0, 10.0]
    assert torch.equal(pot.pack(mu, a, b), x)
    assert torch.equal(pot.unpack(x[0])[1], x[0, :3])
    # leading shapes broadcast
    y = pot.pack(0.5, torch.zeros(4, 1, 3), torch.ones(5, 2))
    assert y.shape == (4, 5, 6) and bool((y[..., 5] == 0.5).all()) and bool((y[..., 3:5] == 1).all())
    assert pot.pack(1, [0, 0, 0], [1, 1]).dtype == torch.get_default_dtype()
    assert pot.pack(torch.tensor(1.0, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), [1, 1]).dtype == torch.float64
    with pytest.raises(ValueError, match='event shape'):
        pot.unpack(torch.zeros(2, 5))
    with pytest.raises(ValueError, match='ability must end'):
        pot.pack(0.0, torch.zeros(2), torch.zeros(2))
    with pytest.raises(ValueError, match='ability must end'):
        pot.pack(0.0, torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError, match='ability must end'):
        pot.pack(0.0, torch.tensor(1.0), torch.zeros(2))
    with pytest.raises(RuntimeError):
        pot.pack(torch.zeros(2), torch.zeros(3, 3), torch.zeros(2))     # leading shapes (2,) and (3,) do not broadcast


def test_synthetic_is_repeatable_per_seed():
    a, ta = ItemResponseTheory.synthetic(12, 7, 3)
    b, tb = ItemResponseTheory.synthetic(12, 7, 3)
    c, tc = ItemResponseTheory.synthetic(12, 7, 4)
    assert torch.equal(a.responses, b.responses) and torch.equal(a.observed, b.observed) and torch.equal(ta, tb)
    assert not torch.equal(ta, tc)
    assert ta.shape == (20,) and ta.dtype == torch.float64
    assert a.event_shape == (20,)
    full, _ = ItemResponseTheory.synthetic(12, 7, 3, missing=0.0)
    none, _ = ItemResponseTheory.synthetic(12, 7, 3, missing=1.0)
    assert bool(full.observed.all()) and not bool(none.observed.any())
    big, _ = ItemResponseTheory.synthetic(400, 100, 0)
    assert big.event_shape == (501,)
    assert abs(float(big.observed.double().mean()) - 0.75) < 0.01
    p, t = ItemResponseTheory.synthetic(2000, 1, 1, missing=0.0, mean_ability_prior=(5.0, 0.01), ability_scale=0.01,
                                        difficulty_scale=0.01)
    assert p.mean_ability_scale == 0.01 and abs(float(t[-1]) - 5.0) < 0.1
    assert float(p.responses.mean()) > 0.97                 # sigmoid(5) = 0.993
    with pytest.raises(ValueError):
        ItemResponseTheory.synthetic(0, 3, 1)
    with pytest.raises(ValueError):
        ItemResponseTheory.synthetic(3, 3, 1, missing=1.5)
    with pytest.raises(ValueError, match='ability_scale'):
        ItemResponseTheory.synthetic(3, 3, 1, ability_scale=-1.0)


@pytest.mark.parametrize('S,Q', [(4, 2), (5, 3), (6, 5), (7, 1), (1, 4), (8, 3)])
def test_data_block_entry_by_entry(S, Q):
    """(Q, 4 ceil(S / 4)) fp32, question-major: the response where it is used, -1 where it is not and in the padding.
    S = 5, Q = 3: the register quad of coordinates 4 .. 7 holds a student, the three questions and mu; it reads the one
    student's entry and three -1."""
    pot, _ = ItemResponseTheory.synthetic(S, Q, 10 * S + Q, missing=0.4)
    A = pot.data_block()
    SA = 4 * ((S + 3) // 4)
    assert A.shape == (Q, SA) and A.dtype == torch.float32 and A.is_contiguous()
    for q in range(Q):
        for c in range(SA):
            if c < S and bool(pot.observed[c, q]):
                assert float(A[q, c]) == float(pot.responses[c, q]) and float(A[q, c]) in (0.0, 1.0)
            else:
                assert float(A[q, c]) == -1.0
    assert int((A >= 0).sum()) == int(pot.observed.sum())


def test_copies_are_cached_per_device_and_dtype():
    pot, _ = ItemResponseTheory.synthetic(5, 3, 1)
    x = torch.zeros(2, 9)
    pot(x)
    pot(x.double())
    first = pot._copy(torch.device('cpu'), torch.float32)
    assert pot._copy(torch.device('cpu'), torch.float32)[0] is first[0]
    assert pot._copy(torch.device('cpu'), torch.float64)[0] is not first[0]
    assert first[0].dtype == torch.float32 and pot._copy(torch.device('cpu'), torch.float64)[1].dtype == torch.float64


def test_fused_in_table_and_routing():
    pot, _ = ItemResponseTheory.synthetic(5, 3, 1)
    assert {f: pot.fused_in(f) for f in FAMILIES} == {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True,
                                                      'dlmc_step': False, 'fit': False}
    with pytest.raises(ValueError, match='unknown launch family'):
        pot.fused_in('nuts')
    for fam in ('mcmc', 'flow_mh', 'neutra'):
        assert resolve_target(pot, (9,), family=fam) is pot
    for fam in ('imh_parallel', 'dlmc_step', 'fit'):
        assert resolve_target(pot, (9,), family=fam) is None
    # opt-in only: a plain callable with the same values is never taken for the class
    assert recognize(lambda x: pot(x), (9,)) is None
