"""Interacting particles on the host: argument validation (one case per rule), the presets, U and grad U of the torch
potential against the fp64 pair sums of tests/particles_fp64.py, the observables, the chunked evaluation, the symmetries
(translation, permutation), the start states, the kernels' parameter block, the header's kind constant, the launch-family
routing, the default layouts of the GPU tests' shapes and the codes of check_particles (no GPU needed: the entry points
answer a malformed descriptor before they touch a device)."""
import ctypes as C

import pytest
import torch

from particles_fp64 import Particles64, lattice_sites, min_pair_distance, start_states
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, ParticleSystem, Potential, recognize
from nfmc_amd.samplers.common import resolve_target

NAN, INF = float('nan'), float('inf')

BAD = [
    ('one particle', dict(n_particles=1), 'n_particles'),
    ('no particle', dict(n_particles=0), 'n_particles'),
    ('P a float', dict(n_particles=4.0), 'n_particles'),
    ('P a bool', dict(n_particles=True), 'n_particles'),
    ('D = 0', dict(n_particles=3, n_dims=0), 'n_dims'),
    ('D = 4', dict(n_particles=3, n_dims=4), 'n_dims'),
    ('D a bool', dict(n_particles=3, n_dims=True), 'n_dims'),
    ('unknown pair', dict(n_particles=3, pair='morse'), 'pair'),
    ('trap zero', dict(n_particles=3, trap=0.0), 'trap'),
    ('trap negative', dict(n_particles=3, trap=-1.0), 'trap'),
    ('trap nan', dict(n_particles=3, trap=NAN), 'trap'),
    ('trap inf', dict(n_particles=3, trap=INF), 'trap'),
    ('temperature zero', dict(n_particles=3, temperature=0.0), 'temperature'),
    ('temperature negative', dict(n_particles=3, temperature=-2.0), 'temperature'),
    ('temperature underflows fp32', dict(n_particles=3, temperature=1e-50), 'temperature'),
    ('epsilon zero', dict(n_particles=3, epsilon=0.0), 'epsilon'),
    ('epsilon inf', dict(n_particles=3, epsilon=INF), 'epsilon'),
    ('r_min zero', dict(n_particles=3, r_min=0.0), 'r_min'),
    ('r_min negative', dict(n_particles=3, r_min=-1.0), 'r_min'),
    ('a nan', dict(n_particles=3, pair='double_well', a=NAN), 'a must'),
    ('b inf', dict(n_particles=3, pair='double_well', b=INF), 'b must'),
    ('r0 overflows fp32', dict(n_particles=3, pair='double_well', r0=1e39), 'r0'),
    ('c zero', dict(n_particles=3, pair='double_well', c=0.0), 'c must'),
    ('c negative', dict(n_particles=3, pair='double_well', c=-0.9), 'c must'),
    ('c not a scalar', dict(n_particles=3, pair='double_well', c=[0.9, 0.9]), 'c must'),
    ('beta eps overflows fp32', dict(n_particles=3, epsilon=1e30, temperature=1e-30), 'pair parameter 0'),
    ('beta k overflows fp32', dict(n_particles=3, trap=1e30, temperature=1e-30), 'beta trap'),
]


@pytest.mark.parametrize('what,kw,name', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw, name):
    with pytest.raises(ValueError, match=name):
        ParticleSystem(**kw)


def test_defaults_presets_and_accepted_edges():
    pot = ParticleSystem(5)
    assert (pot.n_particles, pot.n_dims, pot.pair, pot.trap, pot.temperature, pot.epsilon, pot.r_min) == (5, 3, 'lennard_jones', 1.0, 1.0, 1.0, 1.0)
    assert (pot.a, pot.b, pot.c, pot.r0) == (0.0, -4.0, 0.9, 4.0)
    assert pot.event_shape == (15,) and pot.event_size == 15 and isinstance(pot, Potential)
    dw = ParticleSystem.double_well_4()
    assert (dw.n_particles, dw.n_dims, dw.pair, dw.event_shape) == (4, 2, 'double_well', (8,))
    assert (dw.a, dw.b, dw.c, dw.r0, dw.trap, dw.temperature) == (0.0, -4.0, 0.9, 4.0, 1.0, 1.0)
    for P in (13, 55):
        lj = ParticleSystem.lennard_jones(P)
        assert (lj.n_particles, lj.n_dims, lj.pair, lj.event_shape) == (P, 3, 'lennard_jones', (3 * P,))
        assert (lj.epsilon, lj.r_min, lj.trap, lj.temperature) == (1.0, 1.0, 1.0, 1.0)
    assert ParticleSystem.lennard_jones(13, temperature=0.5).beta == 2.0
    assert ParticleSystem.double_well_4(trap=0.25).trap == 0.25
    ParticleSystem(2, 1, 'double_well', c=torch.tensor(0.5), a=-1, b=0)
    ParticleSystem(3, c=-1.0)                                   # c is the double well's: not read for Lennard-Jones
    assert ParticleSystem(400, 3).event_shape == (1200,)        # d is not capped: the split path takes it
    assert ParticleSystem.CHUNK_FLOATS // (55 * 55 * 3) == 1848   # LJ55: 65536 chains go 1848 at a time, 64 MiB in fp32


def _u_and_grad(pot, x, dtype, **kw):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t, **kw)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


KW = {'lennard_jones': dict(trap=0.7, temperature=1.3, epsilon=1.6, r_min=0.9),
      'double_well': dict(trap=0.4, temperature=0.8, a=0.3, b=-3.0, c=0.7, r0=2.5)}


@pytest.mark.parametrize('P', [2, 3, 5])
@pytest.mark.parametrize('D', [1, 2, 3])
@pytest.mark.parametrize('pair', ['lennard_jones', 'double_well'])
def test_u_and_grad_match_the_fp64_pair_sums(pair, D, P):
    pot, ref = ParticleSystem(P, D, pair, **KW[pair]), Particles64(P, D, pair, **KW[pair])
    x = pot.start_states(12, 10 * P + D, 0.15)
    u, g = _u_and_grad(pot, x, torch.float64)
    assert u.dtype == torch.float64 and u.shape == (12,)
    torch.testing.assert_close(u, ref(x), rtol=1e-12, atol=1e-11)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-11, atol=1e-10)
    torch.testing.assert_close(pot.energy(x), ref(x) * KW[pair]['temperature'], rtol=1e-12, atol=1e-11)
    u32, g32 = _u_and_grad(pot, x, torch.float32)
    assert u32.dtype == torch.float32
    torch.testing.assert_close(u32.double(), ref(x), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(g32.double(), ref.grad(x), rtol=1e-4, atol=1e-3)


def test_closed_form_hessian_diagonal_matches_autograd():
    for pair in ('lennard_jones', 'double_well'):
        for D in (1, 2, 3):
            ref = Particles64(4, D, pair, **KW[pair])
            x = start_states(4, D, 1.1 if pair == 'lennard_jones' else 2.5, 5, 3, 0.1)
            t = x.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(ref(t).sum(), t, create_graph=True)
            hd = torch.stack([torch.autograd.grad(g[:, c].sum(), t, retain_graph=True)[0][:, c] for c in range(ref.d)], dim=1)
            torch.testing.assert_close(hd, ref.hess_diag(x), rtol=1e-10, atol=1e-9)


def test_the_pair_potentials_have_their_minima_where_the_docstring_says():
    lj = ParticleSystem(2, 1, trap=1e-30, epsilon=2.0, r_min=1.5)
    r = torch.tensor([[0.0, 1.5], [0.0, 1.4], [0.0, 1.6]], dtype=torch.float64)
    u = lj(r)
    assert abs(float(u[0]) + 2.0) < 1e-12 and float(u[1]) > float(u[0]) < float(u[2])        # -eps at r_min
    dw = ParticleSystem(2, 1, 'double_well', trap=1e-30)                                       # -4 u^2 + 0.9 u^4
    um = (4.0 / 1.8) ** 0.5
    u = dw(torch.tensor([[0.0, 4.0], [0.0, 4.0 + um], [0.0, 4.0 - um]], dtype=torch.float64))
    assert abs(float(u[0])) < 1e-12
    torch.testing.assert_close(u[1:], torch.full((2,), -4.0 * um ** 2 + 0.9 * um ** 4, dtype=torch.float64), rtol=1e-12, atol=0)


def test_coincident_particles():
    """s = 0: Lennard-Jones is inf; the double well adds phi(0) and no force."""
    x = torch.tensor([[0.5, -0.25, 0.5, -0.25, 2.0, 1.0]], dtype=torch.float64)
    assert float(ParticleSystem(3, 2)(x)) == INF
    dw = ParticleSystem(3, 2, 'double_well', **KW['double_well'])
    u, g = _u_and_grad(dw, x, torch.float64)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    k = KW['double_well']
    beta, r0 = 1.0 / k['temperature'], k['r0']
    phi0 = beta * (k['a'] * (0 - r0) + k['b'] * r0 ** 2 + k['c'] * r0 ** 4)
    two = Particles64(2, 2, 'double_well', **k)                   # particles 0 and 2: the pairs 0-2 and 1-2 are equal
    rest = two(x[:, [0, 1, 4, 5]]) * 2 - beta * k['trap'] * 0.5 * float((x[0, 4:] ** 2).sum())
    torch.testing.assert_close(u, rest + phi0, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g[0, :2], g[0, 2:4], rtol=0, atol=0)     # the coincident pair pushes neither of the two


def test_positions_flatten_and_pair_distances():
    pot = ParticleSystem(5, 3)
    x = torch.arange(30, dtype=torch.float64).reshape(2, 15) ** 1.5
    r = pot.positions(x)
    assert r.shape == (2, 5, 3) and r[1, 2].tolist() == x[1, 6:9].tolist()      # particle-major
    assert torch.equal(pot.flatten(r), x)
    assert pot.positions(x[0]).shape == (5, 3) and pot.flatten(torch.zeros(4, 2, 5, 3)).shape == (4, 2, 15)
    pd = pot.pair_distances(x)
    assert pd.shape == (2, 10)
    for k in range(2):
        torch.testing.assert_close(pd[k], torch.pdist(r[k]), rtol=1e-14, atol=0)
    one = ParticleSystem(4, 1)
    torch.testing.assert_close(one.pair_distances(x[:, :4])[0], torch.pdist(x[0, :4, None]), rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match='event shape'):
        pot.positions(torch.zeros(2, 14))
    with pytest.raises(ValueError, match=r'\(P, D\)'):
        pot.flatten(torch.zeros(2, 3, 5))


@pytest.mark.parametrize('pair', ['lennard_jones', 'double_well'])
def test_chunked_call_equals_unchunked(pair, monkeypatch):
    pot = ParticleSystem(6, 3, pair, **KW[pair])
    x = pot.start_states(11, 4, 0.1)
    whole, gw = _u_and_grad(pot, x, torch.float64, chunk=11)
    for chunk in (1, 3, 4, 10, 64):
        u, g = _u_and_grad(pot, x, torch.float64, chunk=chunk)
        assert torch.equal(u, whole) and torch.equal(g, gw), chunk
    sizes = []
    orig = ParticleSystem._u_chunk
    monkeypatch.setattr(ParticleSystem, '_u_chunk', lambda s, r: sizes.append(r.shape[0]) or orig(s, r))
    monkeypatch.setattr(ParticleSystem, 'CHUNK_FLOATS', 4 * 6 * 6 * 3)      # four chains' worth of pair entries
    assert torch.equal(pot(x), whole) and sizes == [4, 4, 3]
    with pytest.raises(ValueError, match='chunk'):
        pot(x, chunk=0)


@pytest.mark.parametrize('pair', ['lennard_jones', 'double_well'])
@pytest.mark.parametrize('D', [1, 2, 3])
def test_translation_adds_the_traps_change_and_permutation_leaves_u(pair, D):
    P = 5
    pot = ParticleSystem(P, D, pair, **KW[pair])
    x = pot.start_states(7, 2, 0.1)
    r = pot.positions(x)
    t = torch.tensor([0.3, -0.2, 0.45][:D], dtype=torch.float64)
    moved = pot.flatten(r + t)
    bk = pot.beta * pot.trap
    want = 0.5 * bk * (((r + t) ** 2).sum(dim=(1, 2)) - (r ** 2).sum(dim=(1, 2)))
    torch.testing.assert_close(pot(moved) - pot(x), want, rtol=0, atol=1e-11)
    perm = torch.tensor([3, 0, 4, 2, 1])
    torch.testing.assert_close(pot(pot.flatten(r[:, perm])), pot(x), rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize('P,D', [(2, 1), (4, 2), (5, 3), (13, 3), (8, 1), (16, 2), (55, 3)])
def test_start_states(P, D):
    for pot in (ParticleSystem(P, D, r_min=1.1), ParticleSystem(P, D, 'double_well', r0=2.5)):
        sp = 1.1 if pot.pair == 'lennard_jones' else 2.5
        assert pot.spacing == sp
        x = pot.start_states(9, 5, 0.02)
        assert x.shape == (9, P * D) and x.dtype == torch.float64 and x.device.type == 'cpu'
        assert torch.equal(x, start_states(P, D, sp, 9, 5, 0.02))
        assert torch.equal(pot.start_states(9, 5, 0.02), x) and not torch.equal(pot.start_states(9, 6, 0.02), x)
        flat = pot.start_states(1, 0, 0.0)
        torch.testing.assert_close(pot.positions(flat)[0], lattice_sites(P, D, sp), rtol=0, atol=1e-14)
        torch.testing.assert_close(pot.positions(flat)[0].mean(0), torch.zeros(D, dtype=torch.float64), rtol=0, atol=1e-13)
        assert abs(float(min_pair_distance(flat, P, D)) - sp) < 1e-12            # nearest neighbours at the spacing
        assert float(min_pair_distance(x, P, D).min()) > sp - 10 * 0.02
    with pytest.raises(ValueError):
        pot.start_states(0, 1, 0.1)
    with pytest.raises(ValueError):
        pot.start_states(3, 1, -0.1)


def test_data_block_and_descriptor():
    lj = ParticleSystem(7, 2, trap=0.5, temperature=0.25, epsilon=1.5, r_min=1.2)
    b = lj.data_block()
    assert b.dtype == torch.float32 and b.shape == (8,)
    want = torch.tensor([0.0, 2.0, 4 * 0.5, 4 * 1.5, 1.2 * 1.2, 0.0, 0.0, 0.0], dtype=torch.float64).float()
    assert torch.equal(b, want)
    dw = ParticleSystem(3, 3, 'double_well', trap=2.0, temperature=2.0, a=0.5, b=-3.0, c=0.8, r0=3.5)
    assert torch.equal(dw.data_block(), torch.tensor([1.0, 3.0, 1.0, 0.25, -1.5, 0.4, 3.5, 0.0], dtype=torch.float32))


def test_fused_in_table_and_routing():
    pot = ParticleSystem.double_well_4()
    assert {f: pot.fused_in(f) for f in FAMILIES} == {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True,
                                                      'dlmc_step': False, 'fit': False}
    with pytest.raises(ValueError, match='unknown launch family'):
        pot.fused_in('nuts')
    for fam in ('mcmc', 'flow_mh', 'neutra'):
        assert resolve_target(pot, (8,), family=fam) is pot
    for fam in ('imh_parallel', 'dlmc_step', 'fit'):
        assert resolve_target(pot, (8,), family=fam) is None
    assert ParticleSystem(341, 3).fused_in('mcmc') and not ParticleSystem(342, 3).fused_in('mcmc')   # d = 1023 / 1026
    assert ParticleSystem.lennard_jones(55).fused_in('neutra')
    # the fused jump tail: offered at the four-coordinate layouts only (d <= 32); every other kind leaves it to the caller
    assert ParticleSystem.double_well_4().jump_tail_ok() and ParticleSystem(16, 2).jump_tail_ok()
    assert not ParticleSystem(11, 3).jump_tail_ok() and not ParticleSystem.lennard_jones(13).jump_tail_ok()
    assert Potential.jump_tail_ok(pot) is True
    # opt-in only: a plain callable with the same values is never taken for the class
    assert recognize(lambda x: pot(x), (8,)) is None


SHAPES = [((2, 1), (4, 1)), ((2, 2), (4, 1)), ((4, 2), (4, 2)), ((3, 3), (4, 4)), ((5, 3), (4, 4)), ((11, 3), (8, 8)),
          ((13, 3), (8, 8)), ((22, 3), (8, 16)), ((43, 3), (8, 32)), ((86, 3), (8, 64)), ((171, 3), (16, 64)),
          ((341, 3), (16, 64)), ((16, 2), (4, 8)), ((8, 1), (4, 2)), ((55, 3), (8, 32))]


@pytest.mark.parametrize('shape,layout', SHAPES, ids=['%dx%d' % s for s, _ in SHAPES])
def test_the_gpu_grid_reaches_every_default_layout(shape, layout):
    """The (CPL, LPC) the library's choose_cfg picks for kind 11 at each shape of the GPU tests' grid (and at LJ55), asked
    of the library itself: nfmc_sampler_layout is host arithmetic and needs no device."""
    P, D = shape
    cpl, lpc = C.c_int32(0), C.c_int32(0)
    assert hip.lib().nfmc_sampler_layout(P * D, hip.POT_PARTICLES, C.byref(cpl), C.byref(lpc)) == 0
    assert (cpl.value, lpc.value) == layout
    assert cpl.value * lpc.value >= P * D


def _mala_args(d, pot):
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = 4096, 64, d, 2, 0.01, 1      # x: a host value, never read
    a.pot = pot
    a.rng.seed = 3
    return a


def test_check_particles_codes_without_a_device():
    """nfmc_mala_steps_f32 and nfmc_hmc_steps_f32 check their arguments, the descriptor among them, from host values
    before they touch a device, so a malformed kind-11 descriptor is answered here: a NULL a, P < 2 and d that is not
    P D with D in 1 .. 3 are EINVAL, a misaligned a is EALIGN.  The check's own answer for d > 1024, EUNSUPPORTED, is
    behind the entry points' ESHAPE for the same d, which is what a caller sees."""
    base = 1 << 20                            # a host value: the check never reads what a points to
    cases = [((6, 3, 0), hip.EINVAL), ((6, 1, base), hip.EINVAL), ((6, 0, base), hip.EINVAL), ((6, -2, base), hip.EINVAL),
             ((6, 4, base), hip.EINVAL),      # d % P != 0
             ((8, 2, base), hip.EINVAL),      # D = 4
             ((10, 2, base), hip.EINVAL),     # D = 5
             ((3, 6, base), hip.EINVAL),      # more particles than coordinates
             ((6, 3, base + 4), hip.EALIGN), ((6, 3, base + 8), hip.EALIGN),
             ((1026, 342, base), hip.ESHAPE)]
    for (d, P, a), code in cases:
        pot = hip.NfmcPotential(hip.POT_PARTICLES, P, a or None, None, 0.0, 0.0)
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(d, pot)), None)) == code, (d, P, a)
        hm = hip.NfmcHmcArgs()
        hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = 4096, 64, d, 2, 0.01, 1, 3
        hm.pot = pot
        hm.rng.seed = 3
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), None)) == code, (d, P, a)
    # the order of the check: a malformed descriptor that is also misaligned is EINVAL
    pot = hip.NfmcPotential(hip.POT_PARTICLES, 1, base + 4, None, 0.0, 0.0)
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(_mala_args(6, pot)), None)) == hip.EINVAL
