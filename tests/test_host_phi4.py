"""LatticePhi4 on the host: U and grad U of the torch potential against an fp64 restatement written as loops over sites
and bonds (tests/phi4_fp64.py), the Gaussian lam = 0 case against `precision()` and FullRankGaussian, the symmetries of
the model, argument validation (one case per rule), the descriptor and the header's kind constant, the launch-family
routing with and without a last axis that is a multiple of 4, and the mapping of the 1-D double well of Gabrie,
Rotskoff and Vanden-Eijnden (2022) onto the model (no GPU needed)."""
import math

import numpy as np
import pytest
import torch

from phi4_fp64 import Phi4U64
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, FullRankGaussian, LatticePhi4, Potential, recognize
from nfmc_amd.samplers.common import resolve_target

SHAPES = [(1,), (2,), (4,), (7,), (100,), (1, 8), (2, 8), (3, 20), (5, 5), (8, 8), (32, 32)]
BOUNDARIES = ['periodic', 'zero']


def _u_and_grad(pot, x, dtype=torch.float64):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


def _points(shape, n, seed):
    """fields around both wells with O(1) fluctuations"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return sign.reshape((n,) + (1,) * len(shape)) + 0.7 * torch.randn((n,) + tuple(shape), generator=g, dtype=torch.float64)


@pytest.mark.parametrize('boundary', BOUNDARIES)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_class_matches_the_loops(shape, boundary):
    m2, lam, kappa = -0.8, 1.3, 0.6
    pot = LatticePhi4(shape, m2=m2, lam=lam, kappa=kappa, boundary=boundary)
    ref = Phi4U64(shape, m2, lam, kappa, boundary)
    assert pot.event_shape == tuple(shape) and pot.event_size == ref.d
    x = _points(shape, 3 if ref.d > 500 else 6, 11 + ref.d)
    u64, g64 = ref(x), ref.grad(x)
    u, g = _u_and_grad(pot, x)
    torch.testing.assert_close(u, u64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g.reshape(x.shape[0], -1), g64, rtol=1e-12, atol=1e-12)        # autograd = stated gradient
    # flattened states are the same states
    torch.testing.assert_close(pot(x.reshape(x.shape[0], -1)), u, rtol=0, atol=0)
    # the loops agree among themselves: autograd of the bond sum is the neighbour sum
    t = x.reshape(x.shape[0], -1).clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(ref(t).sum(), t)
    torch.testing.assert_close(ga, g64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(pot.precision(), ref.precision(), rtol=1e-12, atol=1e-12)
    # fp32 evaluation, any dtype
    u32 = pot(x.float())
    assert u32.dtype == torch.float32
    torch.testing.assert_close(u32.double(), u64, rtol=1e-5, atol=1e-5 * ref.d)


@pytest.mark.parametrize('boundary', BOUNDARIES)
@pytest.mark.parametrize('shape', [(1,), (2,), (7,), (1, 8), (2, 8), (3, 20), (5, 5)], ids=str)
def test_gaussian_case_is_the_precision_matrix(shape, boundary):
    pot = LatticePhi4(shape, m2=0.5, lam=0.0, kappa=1.0, boundary=boundary)
    d = pot.event_size
    P = pot.precision()
    assert P.dtype == torch.float64 and P.shape == (d, d)
    torch.testing.assert_close(P, P.t(), rtol=0, atol=0)
    assert float(torch.linalg.eigvalsh(P).min()) >= 0.5 - 1e-12
    x = torch.randn(9, d, generator=torch.Generator().manual_seed(d), dtype=torch.float64)
    want = 0.5 * torch.einsum('ni,ij,nj->n', x, P, x)
    torch.testing.assert_close(pot(x), want, rtol=1e-12, atol=1e-12)
    gauss = FullRankGaussian(torch.zeros(d, dtype=torch.float64), precision=P)
    torch.testing.assert_close(gauss(x), pot(x), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('boundary', BOUNDARIES)
@pytest.mark.parametrize('shape', [(7,), (2, 8), (5, 5)], ids=str)
def test_symmetries(shape, boundary):
    pot = LatticePhi4(shape, boundary=boundary)
    x = _points(shape, 5, 3)
    torch.testing.assert_close(pot(-x), pot(x), rtol=1e-13, atol=1e-13)                         # phi -> -phi
    for ax in range(len(shape)):                                                              # reflection of an axis
        torch.testing.assert_close(pot(torch.flip(x, dims=(ax + 1,))), pot(x), rtol=1e-12, atol=1e-12)
    if boundary == 'periodic':
        for ax in range(len(shape)):                                                          # translation
            for k in (1, 3):
                torch.testing.assert_close(pot(torch.roll(x, k, dims=ax + 1)), pot(x), rtol=1e-12, atol=1e-12)
    else:
        u, rolled = pot(x), pot(torch.roll(x, 1, dims=len(shape)))    # along the last axis, length >= 5
        assert float((u - rolled).abs().max()) > 1e-3                                         # the boundary is felt


def test_bond_counts_of_short_axes():
    """periodic: an axis of length 2 counts its bond twice, one of length 1 contributes nothing; zero: n + 1 bonds"""
    x = torch.tensor([[1.0, 3.0]], dtype=torch.float64)
    free = lambda v: float((0.5 * 0.5 * v * v).sum())   # noqa: E731  the m2 = 0.5, lam = 0 site terms
    assert float(LatticePhi4((2,), 0.5, 0.0, 1.0, 'periodic')(x)) == pytest.approx(free(x) + 0.5 * 2 * 4.0)
    assert float(LatticePhi4((2,), 0.5, 0.0, 1.0, 'zero')(x)) == pytest.approx(free(x) + 0.5 * (1.0 + 4.0 + 9.0))
    assert float(LatticePhi4((1, 2), 0.5, 0.0, 1.0, 'periodic')(x)) == pytest.approx(free(x) + 0.5 * 2 * 4.0)
    assert float(LatticePhi4((1, 2), 0.5, 0.0, 1.0, 'zero')(x)) == pytest.approx(free(x) + 0.5 * (14.0 + 2 * 10.0))
    y = torch.tensor([[2.0]], dtype=torch.float64)
    assert float(LatticePhi4((1,), 0.5, 0.0, 1.0, 'periodic')(y)) == pytest.approx(1.0)
    assert float(LatticePhi4((1,), 0.5, 0.0, 1.0, 'zero')(y)) == pytest.approx(1.0 + 0.5 * 8.0)


BAD = [
    ('no shape', dict(shape=None)),
    ('three axes', dict(shape=(2, 2, 2))),
    ('no axes', dict(shape=())),
    ('empty axis', dict(shape=(0,))),
    ('empty second axis', dict(shape=(4, 0))),
    ('negative length', dict(shape=(-4,))),
    ('length not an int', dict(shape=(4.0,))),
    ('length a bool', dict(shape=(True, 4))),
    ('m2 not finite', dict(shape=4, m2=float('inf'))),
    ('m2 nan', dict(shape=4, m2=float('nan'))),
    ('m2 overflows fp32', dict(shape=4, m2=-1e39)),
    ('m2 not a scalar', dict(shape=4, m2=[1.0, 2.0])),
    ('m2 complex', dict(shape=4, m2=1.0 + 0.0j)),
    ('lam negative', dict(shape=4, lam=-1.0)),
    ('lam not finite', dict(shape=4, lam=float('inf'))),
    ('lam overflows fp32', dict(shape=4, lam=1e39)),
    ('kappa negative', dict(shape=4, kappa=-0.5)),
    ('kappa nan', dict(shape=4, kappa=float('nan'))),
    ('kappa a bool', dict(shape=4, kappa=True)),
    ('free field with m2 < 0', dict(shape=4, m2=-1.0, lam=0.0)),
    ('free field with m2 = 0', dict(shape=4, m2=0.0, lam=0.0)),
    ('unknown boundary', dict(shape=4, boundary='open')),
    ('boundary not a string', dict(shape=4, boundary=0)),
]


@pytest.mark.parametrize('what,kw', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw):
    with pytest.raises(ValueError):
        LatticePhi4(**kw)


def test_defaults_and_accepted_edges():
    pot = LatticePhi4((8, 8))
    assert (pot.m2, pot.lam, pot.kappa, pot.boundary) == (-1.0, 1.0, 1.0, 'periodic')
    assert LatticePhi4(6).event_shape == (6,)
    assert LatticePhi4([2, 4]).event_shape == (2, 4)
    LatticePhi4((1,), m2=0.0, lam=1.0, kappa=0.0)
    LatticePhi4((1, 1), m2=1.0, lam=0.0, kappa=0.0, boundary='zero')
    LatticePhi4(4, m2=torch.tensor(-2.0), lam=torch.tensor(0.5), kappa=3)
    pot = LatticePhi4(4, m2=np.float32(-2.0), lam=np.float64(0.5), kappa=np.int64(3))     # numpy scalars are real scalars
    assert (pot.m2, pot.lam, pot.kappa) == (-2.0, 0.5, 3.0) and type(pot.m2) is float


FUSED = {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True, 'dlmc_step': False, 'fit': False}


@pytest.mark.parametrize('shape,ok', [((4,), True), ((8,), True), ((100,), True), ((1, 8), True), ((3, 20), True),
                                      ((32, 32), True), ((64, 4), True), ((1,), False), ((2,), False), ((7,), False),
                                      ((5, 5), False), ((6, 6), False), ((8, 6), False), ((4, 7), False),
                                      ((1028,), False), ((64, 32), False)], ids=str)
def test_routing_table(shape, ok):
    """fused where the last axis is a multiple of 4 (every lattice row starts on a register quad) and d <= 1024"""
    assert set(FUSED) == set(FAMILIES)
    for boundary in BOUNDARIES:
        pot = LatticePhi4(shape, boundary=boundary)
        assert isinstance(pot, Potential)
        for fam, want in FUSED.items():
            assert pot.fused_in(fam) is (want and ok), (fam, shape)
            assert resolve_target(pot, shape, family=fam) is (pot if want and ok else None)
        assert resolve_target(pot, shape) is pot
        with pytest.raises(ValueError):
            pot.fused_in('transport')


def test_recognize_never_infers_a_lattice():
    """A plain callable stays on the split path, also the Gaussian lam = 0 case: the object alone opts in."""
    pot = LatticePhi4((2, 4))
    assert recognize(lambda x: pot(x), (2, 4)) is None
    free = LatticePhi4((4,), m2=1.0, lam=0.0, kappa=0.5)
    assert not isinstance(recognize(lambda x: free(x), (4,)), LatticePhi4)
    assert resolve_target(lambda x: pot(x), (2, 4), fuse='never', family='mcmc') is None
    assert resolve_target(lambda x: pot(x), (2, 4), fuse='auto', family='mcmc') is None


def test_descriptor_and_header_constant(monkeypatch):
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    cpu = torch.device('cpu')
    pot = LatticePhi4((3, 8), m2=-0.25, lam=0.5, kappa=2.0, boundary='zero')
    desc = pot.descriptor(cpu)
    assert desc.kind == 8 == hip.POT_LATTICE_PHI4
    assert desc.n_components == 8                                    # the header's n_components: W
    tab = pot._dev['cpu']
    assert desc.a == tab.data_ptr() and not desc.b
    assert tab.dtype == torch.float32 and tab.tolist() == [-0.25, 0.5, 2.0, 1.0]
    assert pot.descriptor(cpu).a == desc.a                       # one copy per device
    assert LatticePhi4((12,), boundary='periodic').descriptor(cpu).n_components == 12
    assert LatticePhi4((12,), m2=-0.25, kappa=2.0).descriptor(cpu) is not None
    assert LatticePhi4((12,), m2=-0.25, kappa=2.0)._dev == {}
    one = LatticePhi4((12,), m2=-0.25, kappa=2.0, boundary='zero')
    one.descriptor(cpu)
    assert one._dev['cpu'].tolist() == [-0.25, 1.0, 2.0, 1.0]
    # one row with the zero boundary on both axes: the 1-D lattice with the vertical boundary bonds in the mass term
    row = LatticePhi4((1, 12), m2=-0.25, kappa=2.0, boundary='zero')
    row.descriptor(cpu)
    assert row._dev['cpu'].tolist() == [3.75, 1.0, 2.0, 1.0]
    x = _points((1, 12), 4, 2)
    folded = LatticePhi4((12,), m2=3.75, kappa=2.0, boundary='zero')
    torch.testing.assert_close(row(x), folded(x.reshape(4, 12)), rtol=1e-12, atol=1e-12)
    per = LatticePhi4((1, 12), m2=-0.25, kappa=2.0, boundary='periodic')
    per.descriptor(cpu)
    assert per._dev['cpu'].tolist() == [-0.25, 1.0, 2.0, 0.0]


def test_magnetisation():
    pot = LatticePhi4((2, 4))
    x = torch.arange(24, dtype=torch.float64).reshape(3, 2, 4)
    want = x.reshape(3, 8).mean(1)
    torch.testing.assert_close(pot.magnetisation(x), want)
    torch.testing.assert_close(pot.magnetisation(x.reshape(3, 8)), want)
    torch.testing.assert_close(pot.magnetisation(x.reshape(1, 3, 8)), want[None])
    assert pot.magnetisation(x[0]).shape == ()
    with pytest.raises(ValueError):
        pot.magnetisation(torch.zeros(3, 7))


@pytest.mark.parametrize('beta,a,delta,N', [(20.0, 0.1, 0.01, 100), (1.0, 1.0, 0.5, 7), (5.0, 0.3, 0.04, 32)])
def test_gabrie_double_well_mapping(beta, a, delta, N):
    """U = beta sum_i [a/(2 Delta) (phi_{i+1} - phi_i)^2 + Delta/(4a) (1 - phi_i^2)^2], phi_0 = phi_{N+1} = 0, discretised
    directly, equals LatticePhi4((N,), kappa = beta a/Delta, lam = beta Delta/a, m2 = -beta Delta/a, 'zero') up to the
    constant beta Delta N/(4a)."""
    pot = LatticePhi4((N,), m2=-beta * delta / a, lam=beta * delta / a, kappa=beta * a / delta, boundary='zero')
    phi = _points((N,), 6, N)
    u = torch.zeros(6, dtype=torch.float64)
    for k in range(6):
        ext = [0.0] + phi[k].tolist() + [0.0]
        tot = 0.0
        for i in range(N + 1):
            tot += a / (2 * delta) * (ext[i + 1] - ext[i]) ** 2
        for i in range(1, N + 1):
            tot += delta / (4 * a) * (1 - ext[i] ** 2) ** 2
        u[k] = beta * tot
    torch.testing.assert_close(pot(phi) + beta * delta * N / (4 * a), u, rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize('strategy', ['mala', 'hmc', 'mh', 'jump_mala', 'imh', 'neutra_hmc'])
def test_create_sampler_takes_the_event_shape_of_the_object(strategy):
    from nfmc_amd.sample import create_sampler
    pot = LatticePhi4((2, 4))
    s = create_sampler(pot, flow='realnvp' if strategy in ('jump_mala', 'imh', 'neutra_hmc') else None,
                       strategy=strategy)
    assert tuple(s.event_shape) == (2, 4)
    assert s.target is pot
