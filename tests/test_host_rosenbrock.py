"""Rosenbrock on the host: argument validation (one case per rule), U and grad U of the torch potential against fp64
autograd of a restatement of its formula (tests/rosenbrock_fp64.py), the descriptor and the header's kind constant, the
launch-family routing, the sampler factory, and the ancestral sampler against the closed-form block-2 moments (no GPU
needed)."""
import math

import pytest
import torch

from rosenbrock_fp64 import RosenbrockU64
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, Potential, Rosenbrock, recognize
from nfmc_amd.samplers.common import resolve_target



def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


BAD = [
    ('no event_shape', dict(event_shape=None)),
    ('empty event', dict(event_shape=(0,))),
    ('a zero', dict(event_shape=4, a=0.0)),
    ('a negative', dict(event_shape=4, a=-1.0)),
    ('a not finite', dict(event_shape=4, a=float('inf'))),
    ('a nan', dict(event_shape=4, a=float('nan'))),
    ('a underflows fp32', dict(event_shape=4, a=1e-50)),
    ('a overflows fp32', dict(event_shape=4, a=1e39)),
    ('b zero', dict(event_shape=4, b=0.0)),
    ('b negative', dict(event_shape=4, b=-5.0)),
    ('b not finite', dict(event_shape=4, b=float('nan'))),
    ('b overflows fp32', dict(event_shape=4, b=1e40)),
    ('mu not finite', dict(event_shape=4, mu=float('inf'))),
    ('mu overflows fp32', dict(event_shape=4, mu=-1e39)),
    ('mu not a scalar', dict(event_shape=4, mu=[1.0, 2.0])),
    ('block zero', dict(event_shape=4, block=0)),
    ('block past d', dict(event_shape=4, block=5)),
    ('block not an int', dict(event_shape=4, block=2.0)),
    ('block a bool', dict(event_shape=4, block=True)),
]


@pytest.mark.parametrize('what,kw', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw):
    with pytest.raises(ValueError):
        Rosenbrock(**kw)


def test_defaults_and_accepted_edges():
    pot = Rosenbrock(2)
    assert (pot.mu, pot.a, pot.b, pot.block) == (1.0, 0.05, 5.0, 2)
    Rosenbrock(3, block=3)
    Rosenbrock(1, block=1)
    Rosenbrock(4, mu=torch.tensor(0.5), a=torch.tensor(2.0), b=1)


def _cases():
    out = []
    for d in (1, 2, 3, 7, 64):
        for blk in sorted({1, 2, 3, d}):
            if blk <= d:
                out.append((d, blk))
    return out


@pytest.mark.parametrize('d,blk', _cases())
def test_u_and_grad_match_fp64_autograd(d, blk):
    """Includes ragged last blocks (d = 7, block 2 / 3; d = 64, block 3).  Points are exact draws of a tame target
    (narrow heads around 0.3), spread 1.2x, so that x_{c-1}^2 stays O(1) along blocks of any length."""
    mu, a, b = 0.3, 8.0, 16.0
    pot = Rosenbrock(d, mu=mu, a=a, b=b, block=blk)
    ref = RosenbrockU64(d, mu, a, b, blk)
    x = 1.2 * ref.draw(32, d + 10 * blk)
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 3.0
    u64, g64 = ref(x), ref.grad(x)
    # the gradient formula of the docstring, term by term
    want = torch.zeros_like(x)
    for c in range(d):
        if c % blk == 0:
            want[:, c] += 2 * a * (x[:, c] - mu)
        else:
            want[:, c] += 2 * b * (x[:, c] - x[:, c - 1] ** 2)
        if c + 1 < d and (c + 1) % blk != 0:
            want[:, c] -= 4 * b * x[:, c] * (x[:, c + 1] - x[:, c] ** 2)
    torch.testing.assert_close(g64, want, rtol=1e-12, atol=1e-12)
    u, g = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(u, u64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g, g64, rtol=1e-12, atol=1e-10)
    u, g = _u_and_grad(pot, x, torch.float32)
    mag = ref(x.abs()) + a * mu * mu * d + 1.0
    assert bool(((u.double() - u64).abs() <= 1e-6 * math.sqrt(d) * mag).all())
    torch.testing.assert_close(g.double(), g64, rtol=1e-5, atol=1e-4)


def test_two_dimensional_events_flatten_row_major():
    pot = Rosenbrock((2, 3), mu=0.5, a=1.0, b=3.0, block=2)
    flat = Rosenbrock(6, mu=0.5, a=1.0, b=3.0, block=2)
    assert pot.event_shape == (2, 3) and pot.event_size == 6 and flat.event_shape == (6,)
    x = torch.randn(5, 2, 3, dtype=torch.float64)
    torch.testing.assert_close(pot(x), flat(x.reshape(5, 6)), rtol=0, atol=0)
    # blocks run over the flattened order: (0, 1), (2, 3), (4, 5) -- coordinate 3 is row 1, column 0
    ref = RosenbrockU64(6, 0.5, 1.0, 3.0, 2)
    torch.testing.assert_close(pot(x), ref(x), rtol=1e-12, atol=1e-12)


def test_descriptor_and_header_constant(monkeypatch):
    pot = Rosenbrock((3, 3), mu=-0.25, a=0.5, b=7.0, block=4)
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    desc = pot.descriptor(torch.device('cpu'))
    assert desc.kind == 5 == hip.POT_ROSENBROCK
    assert desc.n_components == 4                                   # the header's n_components: the block length
    assert desc.a_scalar == 0.5 and desc.b_scalar == 7.0
    mu32 = pot._dev[('cpu', torch.float32)][2]
    assert desc.a == mu32.data_ptr() and not desc.b
    assert mu32.dtype == torch.float32 and mu32.shape == (1,) and float(mu32[0]) == -0.25
    assert pot.descriptor(torch.device('cpu')).a == desc.a      # one copy per device


FUSED = {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True, 'dlmc_step': False, 'fit': False}


def test_routing_table():
    assert set(FUSED) == set(FAMILIES)
    pot = Rosenbrock(3)
    assert isinstance(pot, Potential)
    for fam, want in FUSED.items():
        assert pot.fused_in(fam) is want, fam
        assert resolve_target(pot, (3,), family=fam) is (pot if want else None)
    assert resolve_target(pot, (3,)) is pot
    with pytest.raises(ValueError):
        pot.fused_in('transport')


@pytest.mark.parametrize('blk', [1, 2])
def test_recognize_never_infers_a_rosenbrock(blk):
    """A plain callable stays on the split path, also block = 1, which is a diagonal Gaussian recognize() could fit: the
    object alone opts in."""
    pot = Rosenbrock(4, block=blk)
    assert recognize(lambda x: pot(x), (4,)) is None or blk == 1
    assert not isinstance(recognize(lambda x: pot(x), (4,)), Rosenbrock)
    assert resolve_target(lambda x: pot(x), (4,), fuse='never', family='mcmc') is None
    if blk == 2:
        assert resolve_target(lambda x: pot(x), (4,), fuse='auto', family='mcmc') is None


@pytest.mark.parametrize('strategy', ['mala', 'hmc', 'mh', 'jump_mala', 'imh', 'neutra_hmc'])
def test_create_sampler_takes_the_event_shape_of_the_object(strategy):
    from nfmc_amd.sample import create_sampler
    pot = Rosenbrock((2, 3), block=3)
    s = create_sampler(pot, flow='realnvp' if strategy in ('jump_mala', 'imh', 'neutra_hmc') else None,
                       strategy=strategy)
    assert tuple(s.event_shape) == (2, 3)
    assert s.target is pot


@pytest.mark.parametrize('mu,a,b', [(1.0, 0.05, 5.0), (0.5, 2.0, 10.0), (-1.5, 0.5, 1.0)])
def test_ancestral_sampler_reproduces_the_block2_moments(mu, a, b):
    """200 000 exact draws at d = 6 (three blocks): sample means within 5 standard errors of the closed form, sample
    variances within 5 standard errors of theirs (the fourth central moment estimated from the same draws)."""
    ref = RosenbrockU64(6, mu, a, b, 2)
    x = ref.draw(200_000, 17)
    mean, var = ref.block2_moments()
    n = x.shape[0]
    assert bool(((x.mean(0) - mean).abs() < 5 * torch.sqrt(var / n)).all()), (x.mean(0), mean)
    c = x - x.mean(0)
    m4 = (c ** 4).mean(0)
    se_var = torch.sqrt((m4 - var ** 2).clamp_min(0) / n)
    assert bool(((c.pow(2).mean(0) - var).abs() < 5 * se_var).all()), (c.pow(2).mean(0), var)
    # and the draws are the target's: the Stein identity E[grad U] = 0 holds within Monte Carlo error
    g = ref.grad(x)
    assert bool((g.mean(0).abs() < 5 * g.std(0) / math.sqrt(n)).all())
