"""The latent Gaussian Markov random field on the host: argument validation (one case per rule), U and grad U of the
torch potential against the fp64 restatement of tests/gmrf_fp64.py for the 3 likelihoods x 3 modes (and the intrinsic
ICAR form), the presets' structure, the ELL block's round trip, the dense counterpart, the reparameterisation identity,
inert unobserved sites, the Hessian bound, the launch-family routing, the header's kind constant, the default layouts of
the GPU tests' dimensions and the codes of check_gmrf (no GPU needed: the entry points answer a malformed descriptor
before they touch a device)."""
import ctypes as C
import math

import pytest
import torch

from gmrf_fp64 import COMBOS, NU, PRIOR, SCALE, graph_edges, laplacian, make_pair, problem_data, starts, step_lambda, truth
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, LatentGaussianModel, LatentGMRF, recognize
from nfmc_amd.samplers.common import resolve_target

NAN, INF = float('nan'), float('inf')
R3 = torch.tensor([[1.5, -1.0, 0.0], [-1.0, 2.5, -1.0], [0.0, -1.0, 1.5]], dtype=torch.float64)
Y3 = torch.tensor([1.0, 0.0, 2.0])


def _asym():
    r = R3.clone()
    r[0, 1] += 1e-3
    return r


BAD = [
    ('unknown likelihood', dict(likelihood='gamma'), 'likelihood'),
    ('unknown parameterization', dict(parameterization='whitened', precision_prior=(1, 1)), 'parameterization'),
    ('scaled without a prior', dict(parameterization='scaled'), 'precision_prior'),
    ('structure of the wrong shape', dict(structure=R3[:2]), r'\(n, n\)'),
    ('structure not finite', dict(structure=R3 * NAN), 'finite'),
    ('structure not symmetric', dict(structure=_asym()), 'symmetric'),
    ('negative diagonal', dict(structure=-R3), 'diagonal'),
    ('triple of unequal lengths', dict(structure=([0, 1], [0], [1.0, 1.0])), 'equal lengths'),
    ('triple with float indices', dict(structure=(torch.tensor([0.0]), torch.tensor([0.0]), [1.0])), 'integers'),
    ('triple out of range', dict(structure=([0, 3], [0, 3], [1.0, 1.0])), 'must lie in'),
    ('sparse tensor of the wrong shape', dict(structure=torch.eye(4).to_sparse()), r'\(n, n\)'),
    ('structure overflows fp32', dict(structure=R3 * 1e39), 'fp32'),
    ('precision zero', dict(precision=0.0), 'precision'),
    ('prior not a pair', dict(precision_prior=2.0), 'pair'),
    ('prior shape negative', dict(precision_prior=(-1.0, 1.0)), 'shape a'),
    ('prior rate zero', dict(precision_prior=(1.0, 0.0)), 'rate b'),
    ('rank above n', dict(rank=4), 'rank'),
    ('rank fractional', dict(rank=2.5), 'rank'),
    ('y not finite', dict(y=torch.tensor([1.0, INF, 0.0])), 'y must be finite'),
    ('negative count', dict(y=torch.tensor([1.0, -1.0, 0.0])), 'non-negative integers'),
    ('binomial y above the trials', dict(likelihood='binomial', y=torch.tensor([1.0, 2.0, 0.0]), weight=1.0), 'y <= trials'),
    ('fractional trials', dict(likelihood='binomial', y=torch.zeros(3), weight=1.5), 'integers'),
    ('negative weight', dict(weight=torch.tensor([1.0, -1.0, 1.0])), 'weight'),
    ('weight of the wrong length', dict(weight=torch.ones(2)), 'weight'),
    ('mean of the wrong length', dict(mean=torch.zeros(2)), 'mean'),
    ('mean not finite in fp32', dict(mean=1e39), 'mean'),
    ('observed not a bool mask', dict(observed=torch.ones(3)), 'observed'),
    ('dof zero', dict(likelihood='student_t', dof=0.0), 'dof'),
    ('scale negative', dict(likelihood='student_t', scale=-1.0), 'scale'),
    ('event shape of the wrong size', dict(event_shape=(2, 2)), 'event_shape'),
    ('event shape without log tau', dict(precision_prior=(1, 1), event_shape=(3,)), 'event_shape'),
]


@pytest.mark.parametrize('name,change,message', BAD, ids=[b[0] for b in BAD])
def test_validation_messages(name, change, message):
    args = dict(y=Y3, structure=R3)
    args.update(change)
    with pytest.raises(ValueError, match=message):
        LatentGMRF(**args)


def test_the_three_forms_of_a_structure_agree():
    dense = LatentGMRF(Y3, R3)
    r, c = torch.nonzero(R3, as_tuple=True)
    for other in (LatentGMRF(Y3, R3.to_sparse()), LatentGMRF(Y3, (r, c, R3[r, c])),
                  LatentGMRF(Y3, (torch.cat([r, r]), torch.cat([c, c]), torch.cat([R3[r, c], R3[r, c]]) / 2))):   # duplicates are summed
        assert torch.equal(other.structure_dense(), dense.structure_dense())
    assert torch.equal(dense.structure_dense(), R3) and dense.width == 3 and dense.rank == 3
    assert torch.equal(LatentGMRF(Y3, R3, precision=2.0).structure_dense(), 2.0 * R3)


def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).clone().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


@pytest.mark.parametrize('lik,mode', COMBOS)
@pytest.mark.parametrize('n', [1, 2, 7, 24, 63])
def test_u_and_gradient_match_the_restatement(n, lik, mode):
    data = problem_data(n, lik, 5 + n)
    for intrinsic in ([False, True] if mode != 'fixed' and n >= 3 else [False]):
        pot, ref = make_pair(data, mode, intrinsic=intrinsic)
        assert pot.dim == ref.d == n + (mode != 'fixed')
        x = starts(data, ref, 6, 3).double()
        u, g = _u_and_grad(pot, x, torch.float64)
        torch.testing.assert_close(u, ref(x), rtol=1e-12, atol=1e-11)
        torch.testing.assert_close(g, ref.grad(x), rtol=1e-11, atol=1e-11)
        u32, _g32 = _u_and_grad(pot, x, torch.float32)
        assert u32.dtype == torch.float32
        torch.testing.assert_close(u32.double(), ref(x), rtol=2e-5, atol=2e-4 * max(1.0, n / 8))


def test_event_shaped_states_and_the_helpers():
    data = problem_data(25, 'poisson', 3)
    flat, ref = make_pair(data, 'fixed')
    grid, _ = make_pair(data, 'fixed', event_shape=(5, 5))
    x = starts(data, ref, 4, 2).double()
    assert torch.equal(grid(x.reshape(4, 5, 5)), flat(x))
    assert torch.equal(grid.latent(x.reshape(4, 5, 5)), x) and torch.equal(grid.coordinates(x.reshape(4, 5, 5)), x)
    torch.testing.assert_close(flat.mean_response(x), flat.weight * torch.exp(x))
    assert bool((flat.precision_of(x) == 1.0).all())
    with pytest.raises(ValueError, match='tau is fixed'):
        flat.coordinates(x, tau=2.0)
    for mode in ('centered', 'scaled'):
        pot, ref = make_pair(data, mode)
        f = data['f_star'][None].repeat(3, 1)
        xs = pot.coordinates(f, tau=torch.tensor([0.5, 1.0, 4.0], dtype=torch.float64))
        assert xs.shape == (3, 26)
        torch.testing.assert_close(pot.latent(xs), f, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(pot.latent(xs), ref.latent(xs), rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(pot.precision_of(xs), torch.tensor([0.5, 1.0, 4.0], dtype=torch.float64))
        assert torch.equal(pot.coordinates(data['f_star']), truth(data, ref))


# ------------------------------------------------------------------------------------------------- presets
def _dense(pot):
    return pot.structure_dense()


def test_random_walk_structure_and_rank():
    for n, order, cyclic in [(9, 1, False), (9, 2, False), (9, 1, True), (9, 2, True), (2, 1, False), (3, 2, False)]:
        pot = LatentGMRF.random_walk(torch.zeros(n), order=order, cyclic=cyclic)
        R = _dense(pot)
        D = torch.zeros(n if cyclic else n - order, n, dtype=torch.float64)
        for k in range(D.shape[0]):
            for off, v in enumerate([-1.0, 1.0] if order == 1 else [1.0, -2.0, 1.0]):
                D[k, (k + off) % n] += v
        assert torch.equal(R, D.t() @ D) and torch.equal(R, R.t())
        assert pot.rank == (n - 1 if cyclic else n - order) == int(torch.linalg.matrix_rank(R))
        assert pot.width == min(n, 2 * order + 1)
    with pytest.raises(ValueError, match='order'):
        LatentGMRF.random_walk(torch.zeros(5), order=3)


def test_icar_structure_and_rank():
    edges = [(0, 1), (1, 0), (1, 2), (2, 2), (3, 4)]                      # a duplicate, a self loop, two components + site 5
    pot = LatentGMRF.icar(torch.zeros(6), torch.tensor(edges))
    assert torch.equal(_dense(pot), laplacian(6, [(0, 1), (1, 2), (3, 4)]))
    assert pot.rank == 6 - 3 == int(torch.linalg.matrix_rank(_dense(pot))) and pot.width == 3
    n = 25
    ring = LatentGMRF.icar(torch.zeros(n), torch.tensor(graph_edges(n)))
    assert ring.rank == n - 1 and torch.equal(_dense(ring), laplacian(n, graph_edges(n)))
    with pytest.raises(ValueError, match='edges'):
        LatentGMRF.icar(torch.zeros(3), torch.tensor([(0, 3)]))


def test_lattice_structure_stencils_and_definiteness():
    H, W, k2 = 6, 7, 0.3
    one = LatentGMRF.lattice(torch.zeros(H, W), k2, alpha=1)
    two = LatentGMRF.lattice(torch.zeros(H, W), k2, alpha=2)
    G = laplacian(H * W, [(i * W + j, i * W + j + 1) for i in range(H) for j in range(W - 1)]
                  + [(i * W + j, (i + 1) * W + j) for i in range(H - 1) for j in range(W)])
    A = G + k2 * torch.eye(H * W, dtype=torch.float64)
    torch.testing.assert_close(_dense(one), A, rtol=0, atol=0)
    torch.testing.assert_close(_dense(two), A @ A, rtol=1e-14, atol=1e-14)
    assert one.width == 5 and two.width == 13 and one.rank == two.rank == H * W
    assert one.event_shape == two.event_shape == (H, W)
    for pot in (one, two):
        assert float(torch.linalg.eigvalsh(_dense(pot)).min()) > 0
    interior = 3 * W + 3
    assert int((_dense(two)[interior] != 0).sum()) == 13 and int((_dense(one)[interior] != 0).sum()) == 5
    assert LatentGMRF.lattice(torch.zeros(H, W), k2, precision_prior=(1, 1)).event_shape == (H * W + 1,)
    assert LatentGMRF.lattice(torch.zeros(32, 32), k2, alpha=2).width == 13
    with pytest.raises(ValueError, match='alpha'):
        LatentGMRF.lattice(torch.zeros(H, W), k2, alpha=3)


def test_log_gaussian_cox_preset():
    counts = torch.tensor([[3.0, 0.0, 1.0, 2.0, 0.0, 3.0]] * 6)
    pot = LatentGMRF.log_gaussian_cox(counts, range_cells=4.0, variance=1.5)
    k2 = 8.0 / 16.0
    assert pot.likelihood == 'poisson' and pot.event_shape == (6, 6) and pot.width == 13
    assert pot.precision == pytest.approx(1.0 / (4 * math.pi * k2 * 1.5))
    ref = LatentGMRF.lattice(counts, k2, alpha=2, precision=pot.precision)
    assert torch.equal(_dense(pot), _dense(ref))
    assert float(pot.mean[0]) == pytest.approx(math.log(1.5) - 0.75)
    assert 'approximate' in LatentGMRF.log_gaussian_cox.__doc__.lower() and 'boundary' in LatentGMRF.log_gaussian_cox.__doc__


def test_synthetic_is_seeded_and_in_the_objects_coordinates():
    for structure, model in [('rw1', {}), ('rw2', dict(precision_prior=PRIOR)), ('ring', dict(precision_prior=PRIOR, parameterization='scaled'))]:
        for lik in ('poisson', 'binomial', 'student_t'):
            a, ta = LatentGMRF.synthetic(12, structure, lik, 7, **model)
            b, tb = LatentGMRF.synthetic(12, structure, lik, 7, **model)
            assert torch.equal(a.y, b.y) and torch.equal(ta, tb) and ta.shape == (a.dim,) and ta.dtype == torch.float64
            assert bool(torch.isfinite(a(ta[None])).all())
    assert not torch.equal(LatentGMRF.synthetic(12, 'rw1', 'poisson', 8)[0].y, LatentGMRF.synthetic(12, 'rw1', 'poisson', 9)[0].y)
    with pytest.raises(ValueError, match='structure'):
        LatentGMRF.synthetic(12, 'tree', 'poisson', 1)


# ------------------------------------------------------------------------------------------------- the kernels' view
@pytest.mark.parametrize('n', [1, 5, 8, 63])
def test_ell_block_round_trips_to_the_structure(n):
    data = problem_data(n, 'student_t', 3)
    pot, _ = make_pair(data, 'scaled')
    block, tab = pot.data_block()
    n4, W = 4 * ((n + 3) // 4), pot.width
    assert block.dtype == torch.float32 and block.shape == (2, W, n4) and tab.dtype == torch.float32 and tab.shape == (8 + 3 * n4,)
    val, col = block[0].double(), block[1].long()
    assert torch.equal(col.float(), block[1])                                   # integer-valued
    back = torch.zeros(n4, n4, dtype=torch.float64)
    for k in range(W):
        back[torch.arange(n4), col[k]] += val[k]
    assert torch.equal(back[:n, :n], data['R'].float().double()) and bool((back[n:] == 0).all()) and bool((back[:, n:] == 0).all())
    pad = val == 0
    assert torch.equal(col[pad], torch.arange(n4)[None, :].expand(W, n4)[pad])  # a padding slot names its own row
    assert bool(pad[:, n:].all())                                               # so have the rows past n
    fill = (data['R'] != 0).sum(1)
    assert W == int(fill.max()) and torch.equal((~pad[:, :n]).sum(0), fill)
    if n == 63:
        assert W == 11 and int(fill.min()) < W                                  # rows of different fill
    ns2 = NU * SCALE ** 2
    want = torch.tensor([(NU + 1) / 2, 1 / ns2, ns2, NU + 1, PRIOR[0], PRIOR[1], n / 2, 0.0], dtype=torch.float64).float()
    assert torch.equal(tab[:8], want)
    for k, v in enumerate((pot.mean, pot.y, pot.weight)):
        assert torch.equal(tab[8 + n4 * k:8 + n4 * k + n], v.float()) and bool((tab[8 + n4 * k + n:8 + n4 * (k + 1)] == 0).all())


def test_codes_and_header_of_the_table():
    data = problem_data(9, 'poisson', 3)
    codes = {}
    for lik, mode in COMBOS:
        pot, _ = make_pair(problem_data(9, lik, 3), mode)
        codes[(lik, mode)] = pot.code()
    assert sorted(codes.values()) == [0.0, 1.0, 2.0, 4.0, 5.0, 6.0, 12.0, 13.0, 14.0]
    assert codes[('binomial', 'centered')] == 5.0 and codes[('student_t', 'scaled')] == 14.0
    icar, _ = make_pair(data, 'centered', intrinsic=True)
    tab = icar.data_block()[1]
    assert tab[:8].tolist() == [0.0, 0.0, 0.0, 0.0, 2.0, 2.0, 4.0, 0.5]


# ------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize('lik', ['poisson', 'binomial', 'student_t'])
def test_to_dense_differs_by_a_constant_only(lik):
    data = problem_data(12, lik, 4)
    pot, ref = make_pair(data, 'fixed')
    dense = pot.to_dense()
    assert isinstance(dense, LatentGaussianModel) and not dense.whitened and dense.dim == 12
    x = starts(data, ref, 9, 1).double()
    diff = dense(x) - pot(x)
    assert float((diff - diff[0]).abs().max()) < 1e-9 * (1 + float(pot(x).abs().max()))
    (ga,), (gb,) = (torch.autograd.grad(p(t).sum(), t) for p, t in ((pot, x.clone().requires_grad_(True)), (dense, x.clone().requires_grad_(True))))
    torch.testing.assert_close(ga, gb, rtol=1e-9, atol=1e-9)
    with pytest.raises(ValueError, match='fixed tau'):
        make_pair(data, 'centered')[0].to_dense()
    with pytest.raises(ValueError, match='proper'):
        LatentGMRF.random_walk(torch.zeros(6)).to_dense()


@pytest.mark.parametrize('lik', ['poisson', 'binomial', 'student_t'])
@pytest.mark.parametrize('intrinsic', [False, True])
def test_reparameterized_gives_the_same_posterior(lik, intrinsic):
    """U_scaled(u, s) = U_centred(m + e^(-s/2) u, s) + (n / 2) s: the log Jacobian of the map, nothing else."""
    data = problem_data(10, lik, 6)
    cen, ref = make_pair(data, 'centered', intrinsic=intrinsic)
    sca = cen.reparameterized('scaled')
    assert sca.scaled and sca.rank == cen.rank and torch.equal(sca.structure_dense(), cen.structure_dense())
    x = starts(data, ref, 7, 2).double()
    u = (x[:, :10] - cen.mean) * torch.exp(0.5 * x[:, 10:])
    xs = torch.cat([u, x[:, 10:]], 1)
    torch.testing.assert_close(sca(xs), cen(x) + 5.0 * x[:, 10], rtol=1e-12, atol=1e-11)
    torch.testing.assert_close(sca.reparameterized('centered')(x), cen(x), rtol=0, atol=0)
    with pytest.raises(ValueError, match='precision_prior'):
        make_pair(data, 'fixed')[0].reparameterized('scaled')


@pytest.mark.parametrize('lik,mode', COMBOS)
def test_unobserved_sites_are_inert(lik, mode):
    """Changing y at a site with weight 0 changes nothing; its gradient is the prior's alone."""
    data = problem_data(11, lik, 5)
    pot, ref = make_pair(data, mode)
    off = torch.nonzero(~data['observed']).reshape(-1)
    assert off.numel() > 0
    other = dict(data)
    other['y'] = data['y'].clone()
    other['y'][off] = 3.0
    pot2, _ = make_pair(other, mode)
    x = starts(data, ref, 5, 1).double()
    assert torch.equal(pot(x), pot2(x))
    big = x.clone()
    big[:, off] = 200.0 if mode != 'scaled' else big[:, off]                     # e^200 overflows where it is evaluated
    assert bool(torch.isfinite(_u_and_grad(pot, big, torch.float32)[1]).all())


@pytest.mark.parametrize('lik,mode', COMBOS)
def test_hessian_bound_is_an_upper_bound(lik, mode):
    for n in (3, 24):
        data = problem_data(n, lik, n)
        for intrinsic in ([False, True] if mode != 'fixed' else [False]):
            pot, ref = make_pair(data, mode, intrinsic=intrinsic)
            for x in starts(data, ref, 4, 5).double():
                assert pot.hessian_bound(x) >= ref.hessian_lmax(x) * (1 - 1e-12)
            assert step_lambda(data, ref, starts(data, ref, 9, 5)) >= ref.hessian_lmax(truth(data, ref))


# ------------------------------------------------------------------------------------------------- routing
def test_fused_in_table_and_routing():
    pot = LatentGMRF(Y3, R3)
    assert {f: pot.fused_in(f) for f in FAMILIES} == {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True,
                                                      'dlmc_step': False, 'fit': False}
    with pytest.raises(ValueError, match='unknown launch family'):
        pot.fused_in('nuts')
    for fam in ('mcmc', 'flow_mh', 'neutra'):
        assert resolve_target(pot, (3,), family=fam) is pot
    for fam in ('imh_parallel', 'dlmc_step', 'fit'):
        assert resolve_target(pot, (3,), family=fam) is None
    assert LatentGMRF.random_walk(torch.zeros(1024)).fused_in('mcmc')
    assert not LatentGMRF.random_walk(torch.zeros(1025)).fused_in('mcmc')
    assert not LatentGMRF.random_walk(torch.zeros(1024), precision_prior=(1, 1)).fused_in('mcmc')      # d = 1025
    # a hub of degree 40: W = 41 > 32 goes to the split path like any callable
    hub = LatentGMRF.icar(torch.zeros(41), torch.tensor([(0, j) for j in range(1, 41)]))
    assert hub.width == 41 and not any(hub.fused_in(f) for f in FAMILIES)
    assert resolve_target(hub, (41,), family='mcmc') is None
    star = LatentGMRF.icar(torch.zeros(32), torch.tensor([(0, j) for j in range(1, 32)]))
    assert star.width == 32 and star.fused_in('mcmc')
    assert pot.jump_tail_ok() is True
    # opt-in only: a plain callable with the same values is never taken for the class
    assert recognize(lambda x: pot(x), (3,)) is None


DIMS = [1, 2, 3, 8, 25, 64, 130, 256, 512]          # tests/test_gpu_gmrf.py's grid
LAYOUTS = [(1, (4, 1)), (2, (4, 1)), (3, (4, 1)), (5, (4, 2)), (8, (4, 2)), (9, (4, 4)), (20, (4, 8)), (25, (4, 8)),
           (64, (8, 8)), (128, (8, 16)), (130, (8, 32)), (256, (8, 32)), (512, (8, 64)), (1024, (16, 64))]


@pytest.mark.parametrize('d,layout', LAYOUTS, ids=['d%d' % d for d, _ in LAYOUTS])
def test_the_gpu_grid_reaches_every_default_layout(d, layout):
    """The (CPL, LPC) the library's choose_cfg picks for kind 13 at the dimensions of the GPU tests, asked of the
    library itself: nfmc_sampler_layout is host arithmetic and needs no device."""
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(d, hip.POT_LATENT_GMRF, C.byref(cpl), C.byref(lpc)) == 0
    assert (cpl.value, lpc.value) == layout
    assert cpl.value * lpc.value >= d


def test_the_gpu_grid_covers_the_default_layouts():
    """Every default layout of the register kernels is reached by a dimension the GPU file runs: its replay grid, d = 5
    and 20 of the jump and determinism cases, d = 9 of the statistics case, d = 128 of the NeuTra cases and d = 1024 of
    the 32 x 32 lattice."""
    by_d = dict(LAYOUTS)
    assert {by_d[d] for d in DIMS + [5, 9, 20, 128, 1024]} == {(4, 1), (4, 2), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64),
                                                              (16, 64)}


def _mala_args(d, pot):
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = 4096, 64, d, 2, 0.01, 1      # x: a host value, never read
    a.pot = pot
    a.rng.seed = 3
    return a


def test_check_gmrf_codes_without_a_device():
    """nfmc_mala_steps_f32 and nfmc_hmc_steps_f32 check their arguments, the descriptor among them, from host values
    before they touch a device, so a malformed kind-13 descriptor is answered here: a NULL a or b, W < 1, an invalid code
    and d < 2 with tau unknown are EINVAL, a misaligned a or b is EALIGN, W > 32 is EUNSUPPORTED.  The check's own answer
    for d > 1024, EUNSUPPORTED, is behind the entry points' ESHAPE for the same d, which is what a caller sees."""
    base = 1 << 20                            # a host value: the check never reads what a and b point to
    cases = [((6, 3, 0, base, 4.0), hip.EINVAL), ((6, 3, base, 0, 4.0), hip.EINVAL),
             ((6, 0, base, base, 4.0), hip.EINVAL), ((6, -1, base, base, 0.0), hip.EINVAL),
             ((6, 3, base, base, 3.0), hip.EINVAL), ((6, 3, base, base, 7.0), hip.EINVAL), ((6, 3, base, base, 8.0), hip.EINVAL),
             ((6, 3, base, base, 9.0), hip.EINVAL), ((6, 3, base, base, 10.0), hip.EINVAL), ((6, 3, base, base, 15.0), hip.EINVAL),
             ((6, 3, base, base, 16.0), hip.EINVAL), ((6, 3, base, base, -1.0), hip.EINVAL), ((6, 3, base, base, 0.5), hip.EINVAL),
             ((6, 3, base, base, NAN), hip.EINVAL),
             ((1, 1, base, base, 4.0), hip.EINVAL), ((1, 1, base, base, 12.0), hip.EINVAL),
             ((6, 3, base + 4, base, 4.0), hip.EALIGN), ((6, 3, base, base + 8, 12.0), hip.EALIGN),
             ((6, 3, base + 4, base, 0.0), hip.EALIGN),
             ((6, 33, base, base, 0.0), hip.EUNSUPPORTED), ((64, 40, base, base, 13.0), hip.EUNSUPPORTED),
             ((1025, 3, base, base, 4.0), hip.ESHAPE)]
    for (d, nc, a, b, code), want in cases:
        pot = hip.NfmcPotential(hip.POT_LATENT_GMRF, nc, a or None, b or None, code, 0.0)
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(d, pot)), None)) == want, (d, nc, a, b, code)
        hm = hip.NfmcHmcArgs()
        hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = 4096, 64, d, 2, 0.01, 1, 3
        hm.pot = pot
        hm.rng.seed = 3
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), None)) == want, (d, nc, a, b, code)
    # the order of the check: a malformed descriptor that is also misaligned, or too wide, is EINVAL
    pot = hip.NfmcPotential(hip.POT_LATENT_GMRF, 0, base + 4, base, 4.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(6, pot)), None)) == hip.EINVAL
    pot = hip.NfmcPotential(hip.POT_LATENT_GMRF, 40, base, base, 3.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(6, pot)), None)) == hip.EINVAL
    # a misaligned block of a too-wide table is EALIGN: alignment is checked before what no kernel runs
    pot = hip.NfmcPotential(hip.POT_LATENT_GMRF, 40, base + 4, base, 4.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(6, pot)), None)) == hip.EALIGN
