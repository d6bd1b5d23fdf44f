"""What tests/test_gpu_mclmc.py, tests/test_gpu_mclmc_matrix.py and tests/test_host_mclmc_matrix.py share: the direct launch
of nfmc_mclmc_steps_f32, the comparison against the fp64 reference of tests/mclmc_fp64.py with its tolerance rule, and the
matrix of cases that takes mclmc_kernel through every potential kind at every default register layout.  A plain module
with no tests in it, imported like tests/neutra_mh_cases.py.

CASES holds one (kind, capacity, size) per potential kind and per capacity CPL LPC of the nine default layouts, with
capacity / 2 < d <= capacity so that nfmc_sampler_layout picks that layout.  d is ragged (under the capacity and no
multiple of CPL: the last lane of a chain is part-filled) wherever the kind's parameterisation has such a size, and
every kind has at least one exact fit, d == capacity, except the sparse regression, whose d = 2 D + 1 is odd.  The
lattice has d % 4 == 0 only, so it is ragged against CPL = 8 and 16 alone.  build(kind, capacity) makes the case: data sizes
(observations, students) are small, d is not.  UNREACHABLE lists the pairs of the 15 x 9 grid no size of which can be built
and fused; tests/test_host_mclmc_matrix.py checks both lists on the CPU.
"""
import ctypes as C
import functools
import math

import torch

import mclmc_fp64 as M

N, T, SEED = 96, 8, 77        # chains, steps and seed of tests/test_gpu_mclmc.py
MARGIN = 4.0


# ------------------------------------------------------------------------------------------------ direct launches
def launch(dev, pot, x0, u0, n_steps, eps, L, imd=None, *, seed=SEED, step0=0, chain_offset=0, stats=None, store=None,
           esums=None, tune=None, energy=True, dense=True):
    """One call of nfmc_mclmc_steps_f32: dict(x, u, kept (n_steps, n, d) or None, de (n_steps, n) or None)."""
    from nfmc_amd import hip
    x = x0.detach().to(dev, torch.float32).contiguous().clone()
    u = u0.detach().to(dev, torch.float32).contiguous().clone()
    n, d = x.shape
    a = hip.NfmcMclmcArgs()
    a.x, a.velocity, a.n, a.d, a.n_steps = hip.ptr(x), hip.ptr(u), n, d, n_steps
    a.step_size, a.decoherence_length = float(eps), float(L)
    imd_dev = None
    if tune is not None:
        imd_dev = tune.imd
    elif imd is not None:
        imd_dev = torch.as_tensor(imd).to(dev, torch.float32).contiguous()
    a.inv_mass_diag = hip.ptr(imd_dev)
    a.pot = pot.descriptor(dev)
    a.rng = hip.make_rng(seed, chain_offset, step0)
    a.stats = stats.struct() if stats is not None else hip.null_stats()
    kept = torch.full((n_steps, n, d), float('nan'), device=dev) if (dense and store is None) else None
    a.samples = hip.store_struct(store if store is not None else kept, n_steps)
    de = torch.full((n_steps, n), float('nan'), device=dev) if energy else None
    a.energy_out = hip.ptr(de)
    a.energy_sums = hip.ptr(esums, torch.float64) if esums is not None else None
    if tune is not None:
        a.tune = tune.struct(n_steps)
    hip.check(hip.lib().nfmc_mclmc_steps_f32(C.byref(a), hip.stream()), 'nfmc_mclmc_steps_f32')
    torch.cuda.synchronize()
    return {'x': x, 'u': u, 'kept': kept, 'de': de, 'imd': imd_dev}


def starts(n, d, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(n, d, generator=g, dtype=torch.float64)).float()


def _figures(target, x0, u0, eps, L, imd, n_steps, seed=SEED, step0=0):
    """(fp64 run, tolerances): per quantity the largest |fp32 - fp64| of the reference's own two runs, x MARGIN"""
    r64 = M.steps(target, x0.double(), u0.double(), eps, L, imd, seed, step0, n_steps, torch.float64)
    r32 = M.steps(target, x0.float(), u0.float(), eps, L, imd, seed, step0, n_steps, torch.float32)
    assert r64[3].all() and r32[3].all(), 'the case is meant to take every step'
    fig = [float((a.double() - b).abs().max()) for a, b in zip(r32[:3], r64[:3])]
    return r64, {'x': MARGIN * fig[0], 'u': MARGIN * fig[1], 'de': MARGIN * fig[2]}


def compare(run, r64, tol, what):
    xs, us, des, _ = r64
    got = {'x': float((run['kept'].cpu().double() - xs).abs().max()),
           'u': float((run['u'].cpu().double() - us[-1]).abs().max()),
           'de': float((run['de'].cpu().double() - des).abs().max())}
    print('%s: |x| <= %.3g  states %.3g (tol %.3g)  velocity %.3g (tol %.3g)  dE %.3g (tol %.3g)'
          % (what, float(xs.abs().max()), got['x'], tol['x'], got['u'], tol['u'], got['de'], tol['de']))
    assert torch.equal(run['kept'][-1], run['x'])
    for k in ('x', 'u', 'de'):
        assert got[k] <= tol[k], (what, k, got[k], tol[k])


def velocity(n, d, seed=SEED, step0=0):
    return M.initial_velocity(n, d, seed, step0).float()


# ------------------------------------------------------------------------------------------------ the matrix
MATRIX_N, MATRIX_T = 71, 6    # 71 is odd: the last wave is part-filled at every LPC < 64
CAPACITIES = (4, 8, 16, 32, 64, 128, 256, 512, 1024)
# the default (CPL, LPC) of each capacity (csrc/sampler_impl.hpp, NFMC_FOR_DEFAULT_CFG)
LAYOUTS = {4: (4, 1), 8: (4, 2), 16: (4, 4), 32: (4, 8), 64: (8, 8), 128: (8, 16), 256: (8, 32), 512: (8, 64), 1024: (16, 64)}
KINDS = ('quadratic', 'funnel', 'mixture', 'logreg', 'fullrank', 'rosenbrock', 'sv', 'sparse_logreg', 'phi4', 'irt', 'vfx',
         'particles', 'lgm', 'gmrf', 'diffusion')
OWN_UNIT_KINDS = KINDS[4:]
# a ragged d of each capacity: odd, so a multiple of no CPL, and over half the capacity
RAGGED = {4: 3, 8: 7, 16: 13, 32: 27, 64: 51, 128: 101, 256: 203, 512: 301, 1024: 1001}


def _sizes(exact):
    """{capacity: d}: RAGGED, and d == capacity at the capacities of `exact`"""
    out = dict(RAGGED)
    out.update({cap: cap for cap in exact})
    return out


# kind -> {capacity: d or the shape the kind is built from}.  The exact fits are spread over the capacities.
SIZES = {
    'quadratic': _sizes((4, 1024)),
    'funnel': _sizes((8, 512)),
    'mixture': _sizes((16, 256)),
    'logreg': _sizes((32, 128)),
    'fullrank': _sizes((64, 4)),
    'rosenbrock': _sizes((128, 8)),
    'sv': _sizes((4, 256)),                      # d = T + 3 with T >= 1: 4 is the one size of capacity 4
    'sparse_logreg': _sizes(()),                 # d = 2 D + 1 is odd: no exact fit
    # (H, W) or (L,), W % 4 == 0, so d % 4 == 0: 4 and 8 are the one size of their capacity; 36, 100, 300 are no multiple
    # of 8 and 812 none of 16.  (lattice, boundary)
    'phi4': {4: ((4,), 'periodic'), 8: ((2, 4), 'zero'), 16: ((3, 4), 'periodic'), 32: ((3, 8), 'zero'),
             64: ((9, 4), 'periodic'), 128: ((5, 20), 'zero'), 256: ((16, 16), 'periodic'), 512: ((15, 20), 'zero'),
             1024: ((29, 28), 'periodic')},
    # (students, questions): d = S + Q + 1
    'irt': {4: (1, 1), 8: (3, 3), 16: (8, 4), 32: (20, 11), 64: (30, 20), 128: (60, 40), 256: (150, 52), 512: (400, 111),
            1024: (700, 323)},
    # (intercepts, slopes, groups): d = 2 C + 5 with both sides varying, C + 2 for varying intercepts of known noise
    'vfx': {4: ('varying', 'none', 1), 8: ('varying', 'varying', 1), 16: ('varying', 'varying', 4),
            32: ('varying', 'none', 30), 64: ('varying', 'varying', 23), 128: ('varying', 'varying', 48),
            256: ('varying', 'varying', 99), 512: ('varying', 'varying', 148), 1024: ('varying', 'varying', 498)},
    # (particles, dimensions, pair potential): d = P D.  The double well's quartic makes a large cluster so stiff that the
    # step rule leaves it standing (eps 5e-5 at P = 16 with the default wells): it runs at two small sizes, with r0 = 2,
    # Lennard-Jones at all others.
    'particles': {4: (3, 1, 'lennard_jones'), 8: (2, 3, 'double_well'), 16: (5, 3, 'double_well'), 32: (16, 2, 'lennard_jones'),
                  64: (17, 3, 'lennard_jones'), 128: (33, 3, 'lennard_jones'), 256: (67, 3, 'lennard_jones'),
                  512: (150, 2, 'lennard_jones'), 1024: (341, 3, 'lennard_jones')},
    'lgm': _sizes((16, 512)),
    'gmrf': _sizes((8, 64)),
    'diffusion': {4: 3, 8: 8, 16: 14, 32: 26, 64: 63, 128: 100, 256: 252, 512: 500, 1024: 1023},   # tests/test_gpu_diffusion.py
}
CASES = [(kind, cap, SIZES[kind][cap]) for kind in KINDS for cap in CAPACITIES if cap in SIZES[kind]]
# (kind, capacity, reason): the pairs of the grid with no case.  Every kind has a size that builds and fuses in every
# capacity's range (a lattice of rows of 4 sites has every d % 4 == 0), so the list is empty.
UNREACHABLE = []


def case_id(case):
    return '%s-%d' % (case[0], case[1])


def _phi4_d(size):
    return math.prod(size[0])


def case_d(case):
    """d of a case of CASES"""
    kind, _cap, size = case
    if kind == 'phi4':
        return _phi4_d(size)
    if kind == 'irt':
        return size[0] + size[1] + 1
    if kind == 'vfx':
        return 2 * size[2] + 5 if size[1] == 'varying' else size[2] + 2
    if kind == 'particles':
        return size[0] * size[1]
    return size


def _quadratic(d, n):
    from nfmc_amd.potentials import QuadraticPotential
    a = torch.linspace(0.3, 2.0, d, dtype=torch.float64).float()
    b = torch.linspace(-0.5, 0.5, d, dtype=torch.float64).float()
    return QuadraticPotential((d,), a, b), M.quadratic(a.double(), b.double()), starts(n, d, 100 + d)


def _funnel(d, n):
    from nfmc_amd.potentials import Funnel
    return Funnel((d,), 3.0), M.funnel(3.0), starts(n, d, 7 + d)


def _mixture(d, n):
    """Three components of unequal weight with per-coordinate scales and means within a standard deviation of each other.
    The restatement works in the dtype of x, like mclmc_fp64.quadratic: the component exponents e_k grow like |x|^2 / 2
    while the responsibilities hang on their differences, which fp32 knows to an ulp of |e_k| only, and a restatement that
    worked in fp64 whatever it is given would not charge that to the fp32 run (at d = 1001 and starts of scale 0.8,
    |e_k| = 380 and torch's own fp32 evaluation is 3 times further from fp64 than the kernel is).  The starts shrink like
    sqrt(64 / d) above d = 64, which holds |e_k| under 40 and the state tolerance under the cap at every capacity."""
    from nfmc_amd.potentials import GaussianMixture
    g = torch.Generator().manual_seed(300 + d)
    means = (torch.randn(3, d, generator=g, dtype=torch.float64) / math.sqrt(d)).float().double()
    scales = (0.7 + 0.6 * torch.rand(3, d, generator=g, dtype=torch.float64)).float().double()
    w = torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64)
    pot = GaussianMixture((d,), means, scales, w)
    lam, c = pot.lam.float().double(), pot.log_norm.float().double()     # what the kernels read

    def ref(x):
        x = x.reshape(x.shape[0], -1)
        q = c.to(x.dtype)[None] - 0.5 * (lam.to(x.dtype)[None] * (x[:, None, :] - means.to(x.dtype)[None]) ** 2).sum(-1)
        return -torch.logsumexp(q, dim=1)
    return pot, ref, starts(n, d, 3 + d, 0.8 * min(1.0, math.sqrt(64.0 / d)))


def _logreg(d, n):
    from logreg_fp64 import LogRegU64, synthetic
    from nfmc_amd.potentials import BayesianLogisticRegression
    n_obs = 37                                   # the tile holds 4096 / DP rows: several tiles from capacity 128, a part-filled last one
    X, y, _ = synthetic(n_obs, d, 11 + d, scale=2.0 / math.sqrt(n_obs))
    return BayesianLogisticRegression(X, y, 1.5), LogRegU64(X, y, 1.5), starts(n, d, 4 + d, 0.7)


def _fullrank(d, n):
    from fullrank_fp64 import FullRankU64, draw, spd
    from nfmc_amd.potentials import FullRankGaussian
    lam = spd(d, 10.0, 13 * d)
    mu = 0.5 * torch.randn(d, generator=torch.Generator().manual_seed(13 * d + 1), dtype=torch.float64)
    ref = FullRankU64(lam, mu)
    return FullRankGaussian(mu, precision=lam), ref, draw(ref.lam, ref.mu, n, 61, spread=1.2).float()


def _rosenbrock(d, n):
    from nfmc_amd.potentials import Rosenbrock
    from rosenbrock_fp64 import RosenbrockU64
    blk, mu, a, b = (2 if d % 3 else 3), 0.5, 2.0, 10.0     # an odd d ends in a block of one
    ref = RosenbrockU64(d, mu, a, b, blk)
    return Rosenbrock(d, mu=mu, a=a, b=b, block=blk), ref, ref.draw(n, 61 + d).float()


def _sv(d, n):
    from nfmc_amd.potentials import StochasticVolatility
    from sv_fp64 import SVU64, start_states
    y, x0, _ = start_states(d - 3, n, 21 + d, -1.0, 0.25, 0.95, 0.05)
    return StochasticVolatility(y), SVU64(y), x0.float()


def _sparse_logreg(d, n):
    from nfmc_amd.potentials import SparseLogisticRegression
    from sparse_logreg_fp64 import model_u64, start_states, synthetic
    D, n_obs = (d - 1) // 2, 29
    X, y, _ = synthetic(n_obs, D, 61 + d, n_nonzero=min(3, D), scale=2.0 / math.sqrt(n_obs))
    return SparseLogisticRegression(X, y), functools.partial(model_u64, X=X, y=y), start_states(D, n, 62 + d, 1.0).float()


def _phi4(size, n):
    from nfmc_amd.potentials import LatticePhi4
    from phi4_fp64 import Phi4U64
    (shape, boundary), m2, lam, kappa = size, -1.0, 1.0, 1.0
    ref = Phi4U64(shape, m2, lam, kappa, boundary)
    g = torch.Generator().manual_seed(61 + ref.d)
    lm = abs(m2) + 3.0 * lam * (-m2 / lam + 0.25) + 4.0 * ref.ndim * kappa
    sign = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0).double()
    x0 = sign[:, None] * math.sqrt(-m2 / lam) + torch.randn(n, ref.d, generator=g, dtype=torch.float64) / math.sqrt(lm)
    return LatticePhi4(shape, m2=m2, lam=lam, kappa=kappa, boundary=boundary), ref, x0.float()


def _irt(size, n):
    from irt_fp64 import IRTFast64, start_states
    from nfmc_amd.potentials import ItemResponseTheory
    S, Q = size
    pot, truth = ItemResponseTheory.synthetic(S, Q, S + Q + 1, missing=0.25)
    ref = IRTFast64(pot.responses, pot.observed)
    return pot, ref, start_states(ref, truth, n, S + Q + 2).float()


def _vfx(size, n):
    from nfmc_amd.potentials import VaryingEffectsRegression
    from varying_effects_fp64 import VFX64, start_states
    ia, sl, Cn = size
    noise = 1.0 if sl == 'none' else None
    pot, truth = VaryingEffectsRegression.synthetic(Cn, 2 * Cn + 7, 1000 + Cn, intercepts=ia, slopes=sl, centered=True,
                                                    noise_scale=noise)
    ref = VFX64(x=pot.x, y=pot.y, group=pot.group, intercepts=ia, slopes=sl, noise_scale=pot.noise_scale, centered=True,
                location_scale=pot.location_scale, scale_scale=pot.scale_scale)
    return pot, ref, start_states(ref, truth, n, pot.event_size + 1).float()


def _particles(size, n):
    from nfmc_amd.potentials import ParticleSystem
    from particles_fp64 import Particles64
    P, D, pair = size
    kw = {'r0': 2.0} if pair == 'double_well' else {}     # wells two apart: the start lattice's diagonals sit on gentle slopes
    pot, ref = ParticleSystem(P, D, pair, **kw), Particles64(P, D, pair, **kw)
    # The double well takes r - r0 of a pair that starts at r0: in fp32 the difference keeps few digits of r, whoever forms
    # it.  Its restatement therefore works in the dtype of x (Particles64.u), like the mixture's, so that the reference's
    # fp32 run pays for that cancellation too; Lennard-Jones has none and keeps the fp64 form.
    return pot, (ref.u if pair == 'double_well' else ref), pot.start_states(n, P * D + 1, 0.03).float()


def _lgm(d, n):
    from latent_gaussian_fp64 import PAIRS, make_pair, problem_data, starts as lgm_starts
    lik, par = PAIRS[d % len(PAIRS)]
    data = problem_data(d, lik, 13 * d)
    pot, ref = make_pair(data, par, None)
    return pot, ref, lgm_starts(data, ref, n, 61).float()


def _gmrf(d, n):
    from gmrf_fp64 import COMBOS, make_pair, n_of, problem_data, starts as gmrf_starts
    lik, mode = COMBOS[d % len(COMBOS)]
    data = problem_data(n_of(d, mode), lik, 13 * d, None)
    pot, ref = make_pair(data, mode, None, False)
    return pot, ref, gmrf_starts(data, ref, n, 61).float()


# d -> (model, m, scales unknown) of tests/test_gpu_diffusion.py's kinds of problem: d = T m + 2 [unknown]
_DIFFUSION = {3: ('cubic', 1, False), 8: ('cubic', 3, True), 14: ('fitzhugh_nagumo', 2, False), 26: ('ou', 2, False),
              63: ('lorenz63', 3, False), 100: ('fitzhugh_nagumo', 2, False), 252: ('brownian', 1, False), 500: ('ou', 2, False),
              1023: ('cubic', 3, False)}


def _diffusion(d, n):
    from diffusion_fp64 import make_pair, problem_data, shape_of, starts_near_truth
    model, m, unknown = _DIFFUSION[d]
    data = problem_data(shape_of(d, m, unknown), m, model, 13 * d, unknown)
    pot, ref = make_pair(data, None)
    return pot, ref, starts_near_truth(data, pot, n, 61).float()


_BUILDERS = {'quadratic': _quadratic, 'funnel': _funnel, 'mixture': _mixture, 'logreg': _logreg, 'fullrank': _fullrank,
             'rosenbrock': _rosenbrock, 'sv': _sv, 'sparse_logreg': _sparse_logreg, 'phi4': _phi4, 'irt': _irt, 'vfx': _vfx,
             'particles': _particles, 'lgm': _lgm, 'gmrf': _gmrf, 'diffusion': _diffusion}


@functools.lru_cache(maxsize=None)
def build(kind, capacity, n=MATRIX_N):
    """(package potential, fp64 restatement, starts x0 (n, d) fp32) of the case of `kind` at `capacity`.  Built once and
    shared: callers leave all three as they are."""
    return _BUILDERS[kind](SIZES[kind][capacity], n)


def nearest(kind, capacity):
    """the capacity with a case of `kind` that is nearest to `capacity` (the smaller of two equally near)"""
    have = [cap for cap in CAPACITIES if cap in SIZES[kind]]
    return min(have, key=lambda cap: (abs(math.log2(cap) - math.log2(capacity)), cap))


def mass_diagonal(d):
    """the inv_mass_diag of every matrix case"""
    return torch.linspace(0.5, 2.0, d, dtype=torch.float64).float()


def step_size(ref, x0, imd):
    """A tenth of blackjax's default start sqrt(d), scaled down by the size of the gradient the starts see, the gradient
    taken in the coordinates the kick sees it in (sigma g): every kind takes every step."""
    d = x0.shape[1]
    g = M.value_and_grad(ref, x0.double())[1]
    if imd is not None:
        g = g * torch.as_tensor(imd).double().sqrt()[None]
    return float(0.1 * math.sqrt(d) / max(1.0, float(g.norm(dim=1).median()) / math.sqrt(d)))


@functools.lru_cache(maxsize=None)
def reference(kind, capacity, n=MATRIX_N, n_steps=MATRIX_T):
    """What a matrix case is run with and held to, computed once: dict(eps, L, imd, u0, r64, tol)"""
    _pot, ref, x0 = build(kind, capacity, n)
    d = x0.shape[1]
    imd, u0 = mass_diagonal(d), velocity(n, d)
    eps, L = step_size(ref, x0, imd), math.sqrt(d)
    r64, tol = _figures(ref, x0, u0, eps, L, imd, n_steps)
    return {'eps': eps, 'L': L, 'imd': imd, 'u0': u0, 'r64': r64, 'tol': tol}
