"""What tests/test_host_neutra_mh.py and tests/test_gpu_neutra_mh.py share: the NeuTra-MH sampler builder, the two
closed-form targets with their fp64 restatements, the fp64 oracle run, the kernel's rows-per-wave rule restated, and the
cases of the routing decision.  A plain module, imported like tests/target_harness.py."""
import collections
import functools
import math

import torch

import target_harness as H

N, T = 96, 4                  # chains and transitions of a case unless it says otherwise
SEED, FLOW_SEED, START_SEED = 12, 5, 61


def imd(d):
    """the proposal scale of every case: 0.5 / sqrt(d) on every coordinate"""
    return torch.full((d,), 0.5 / math.sqrt(d), dtype=torch.float64)


def sum_of_squares(d):
    """(package potential, fp64 restatement) of U(x) = sum x^2"""
    from nfmc_amd.potentials import SumOfSquares
    return SumOfSquares((d,)), lambda x: (x.reshape(x.shape[0], -1).double() ** 2).sum(-1)


def funnel(d, scale=3.0):
    """(package potential, fp64 restatement) of Neal's funnel"""
    from nfmc_amd.potentials import Funnel

    def ref(x):
        x = x.reshape(x.shape[0], -1).double()
        x0 = x[:, 0]
        return x0 ** 2 / (2 * scale ** 2) + 0.5 * torch.exp(-x0) * (x[:, 1:] ** 2).sum(-1) + 0.5 * (x.shape[1] - 1) * x0
    return Funnel((d,), scale), ref


TARGETS = {'sumsq': sum_of_squares, 'funnel': funnel}


def starts(n, d, seed=START_SEED):
    """latent starts: standard normal draws, fp32"""
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def sampler(d, target, f, T, adjustment=True, scale=None):
    """NeuTraMH on the flow f with the proposal scale imd(d) (or `scale`)"""
    from nfmc_amd.samplers import mcmc, neutra
    m = (imd(d) if scale is None else scale).float()
    return neutra.NeuTraMH((d,), target, mcmc.MHKernel(event_size=d, inv_mass_diag=m), mcmc.MHParameters(adjustment=adjustment),
                           neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))


def adjusted(of, ref, d):
    """U~ in fp64 on the oracle flow"""
    from oracle import samplers as osamp
    return osamp.neutra_adjusted_target(of, ref, (d,))


def oracle(z0, of, ref, T, seed=SEED, adjustment=True, rounds=10, noise=None):
    """The oracle of every comparison: random-walk MH on the fp64 adjusted target, on the native Philox stream of `seed`
    unless a `noise` source is given."""
    from oracle import samplers as osamp
    d = z0.shape[1]
    if noise is None:
        noise = osamp.PhiloxNoise(seed, rounds=rounds, dtype=torch.float64)
    with torch.no_grad():
        return osamp.mcmc_sample(z0.double(), adjusted(of, ref, d), 'mh', T, 0.0, imd(d), adjustment=adjustment, noise=noise)


def flows(d, kind='realnvp', n_hidden=None, seed=FLOW_SEED):
    """(package flow, fp64 oracle flow) with the same perturbed weights: H.flow_pair for 'realnvp' and 'c-rqnsf', the same
    recipe for 'nice' (which flow_pair does not build).  The initial weights come from a seed of the case's own."""
    if kind != 'nice':
        return H.flow_pair(d, seed, n_hidden=n_hidden, spline=kind == 'c-rqnsf', init_seed=1000 + d)
    from nfmc_amd import flows as pflows
    from oracle import flow as oflow
    kw = {} if n_hidden is None else {'conditioner_kwargs': {'n_hidden': n_hidden}}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 + d)
        f, of = pflows.Flow(pflows.NICE((d,), **kw)), oflow.Flow(oflow.NICE((d,), **kw))
    of = oflow.perturb_(of, seed, 0.2, 0.7071)
    f.load_state_dict(of.state_dict())
    return f, of.double()


def margin(tr, z0, of, ref):
    """The near-tie margin of a run, (T, n): the project's bound on an fp32 log ratio (H.compare_decisions),
    2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) |U~(z)|, z the state each transition starts from."""
    d = z0.shape[1]
    states = tr.stacked().double()
    prev = torch.cat([z0.double()[None], states[:-1]])
    size = magnitude(of, ref, d)(prev.reshape(-1, d)).reshape(states.shape[:2])
    lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    return 2e-4 * max(1.0, d / 64) + 1e-4 * lr.abs() + 8 * 2.0 ** -24 * size


def magnitude(of, ref, d):
    """|U~| of a batch of latents, for compare_decisions' `mag`"""
    u = adjusted(of, ref, d)

    def mag(z):
        with torch.no_grad():
            return u(z).abs()
    return mag


# ---- own-unit kinds
def _fullrank():
    from fullrank_fp64 import FullRankU64, draw, spd
    from nfmc_amd.potentials import FullRankGaussian
    d = 25
    lam = spd(d, 10.0, 13 * d)
    mu = 0.5 * torch.randn(d, generator=torch.Generator().manual_seed(13 * d + 1), dtype=torch.float64)
    ref = FullRankU64(lam, mu)
    return FullRankGaussian(mu, precision=lam), ref, draw(ref.lam, ref.mu, N, 61, spread=1.2).float(), 8


def _sparse_logreg():
    from nfmc_amd.potentials import SparseLogisticRegression
    from sparse_logreg_fp64 import model_u64, start_states, synthetic
    d, n_obs = 51, 300
    D = (d - 1) // 2
    X, y, _ = synthetic(n_obs, D, 61 + d, scale=2.0 / math.sqrt(n_obs))
    return SparseLogisticRegression(X, y), functools.partial(model_u64, X=X, y=y), start_states(D, N, 62 + d, 1.0).float(), 16


def _phi4():
    from nfmc_amd.potentials import LatticePhi4
    from phi4_fp64 import Phi4U64
    shape, m2, lam, kappa = (4, 4), -1.0, 1.0, 1.0
    ref = Phi4U64(shape, m2, lam, kappa, 'periodic')
    g = torch.Generator().manual_seed(61)
    lm = abs(m2) + 3.0 * lam * (-m2 / lam + 0.25) + 4.0 * ref.ndim * kappa
    sign = torch.where(torch.rand(N, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0).double()
    z0 = sign[:, None] * math.sqrt(-m2 / lam) + torch.randn(N, ref.d, generator=g, dtype=torch.float64) / math.sqrt(lm)
    return LatticePhi4(shape, m2=m2, lam=lam, kappa=kappa, boundary='periodic'), ref, z0.float(), 8


def _diffusion():
    from diffusion_fp64 import make_pair, problem_data, shape_of
    # The FitzHugh-Nagumo bridge of tests/test_gpu_diffusion.py's NeuTra-HMC case (32 time points, d = 64), from prior draws:
    # |U~| ~ 2e3 there, and rounding x = f^-1(z) to fp32 moves the fp64 U by 9e-5 (diffusion_fp64.fp32_figure), under the
    # log-ratio bound.  The Lorenz bridge is left to that file, which widens its margin by that figure: at prior draws its
    # |U~| is 6e6 and the fp32 rounding of x alone moves U by 0.9, which no bound on an fp32 log ratio is about.
    d, m = 64, 2
    data = problem_data(shape_of(d, m, False), m, 'fitzhugh_nagumo', 13 * d, False)
    pot, ref = make_pair(data, None)
    return pot, ref, pot.prior_draws(N, 61).float(), 16


def _rosenbrock():
    from nfmc_amd.potentials import Rosenbrock
    from rosenbrock_fp64 import RosenbrockU64
    d, blk, mu, a, b = 8, 2, 0.5, 2.0, 10.0
    ref = RosenbrockU64(d, mu, a, b, blk)
    return Rosenbrock(d, mu=mu, a=a, b=b, block=blk), ref, ref.draw(N, 61).float(), 8


# (potential, fp64 restatement, latent starts (N, d) fp32, conditioner width) of five own-unit kinds
OWN_KINDS = {'fullrank': _fullrank, 'rosenbrock': _rosenbrock, 'sparse_logreg': _sparse_logreg, 'phi4': _phi4,
             'diffusion': _diffusion}
# Whether NeuTra.sample sends the kind to the kernel (neutra.MH_KERNEL_KINDS): the sparse regression walks its observations
# per chain and was measured slower there than on the split path, so it stays split
ON_KERNEL = {'fullrank': True, 'rosenbrock': True, 'sparse_logreg': False, 'phi4': True, 'diffusion': True}


# ---- the kernel's tiles (csrc/neutra_kernels.hpp: neutra_rows_per_wave with four tiles; csrc/flow_device.hpp: tile_stride)
MH_TILES = 4
LDS_BUDGET = 150 * 1024


def tile_stride(d):
    s = (d + 3) & ~3
    return s + 4 if ((s >> 2) & 1) == 0 else s


def rows_per_wave(d, tiles=MH_TILES):
    for rpw in (64, 32, 16):
        if tiles * rpw * tile_stride(d) * 4 <= LDS_BUDGET:
            return rpw
    return 0


# ---- the routing decision
class Route(collections.namedtuple('Route', 'name target d n_hidden rounds fuse closed_form fused')):
    def problem(self):
        """(target handed to the sampler, fp64 restatement)"""
        if self.target == 'mixture':
            from nfmc_amd.potentials import GaussianMixture
            means = torch.tensor([[-1.0] * self.d, [1.0] * self.d], dtype=torch.float64)
            pot = GaussianMixture((self.d,), means.float(), 1.0)

            def ref(x):
                x = x.reshape(x.shape[0], -1).double()
                q = -0.5 * ((x[:, None, :] - means[None]) ** 2).sum(-1) + math.log(0.5)
                return -torch.logsumexp(q, dim=1)
            return pot, ref
        if self.target == 'callable':
            def quartic(x):
                x = x.reshape(x.shape[0], -1)
                return 0.25 * (x ** 4).sum(-1) + 0.5 * (x ** 2).sum(-1)
            return quartic, lambda x: quartic(x.double())
        return TARGETS[self.target](self.d)

    def flows(self):
        return flows(self.d, 'realnvp', self.n_hidden)

    def sampler(self, T, flows=None, target=None):
        f = (flows or self.flows())[0]
        s = sampler(self.d, self.problem()[0] if target is None else target, f, T)
        s.rng_rounds, s.fuse = self.rounds, self.fuse
        return s


ROUTES = [
    Route('sumsq-narrow', 'sumsq', 5, 8, 10, 'auto', True, True),
    Route('funnel-narrow', 'funnel', 65, 32, 10, 'auto', True, True),
    Route('wide-conditioner', 'sumsq', 5, 40, 10, 'auto', True, False),
    Route('mixture', 'mixture', 5, 8, 10, 'auto', False, False),
    Route('callable', 'callable', 5, 8, 10, 'auto', False, False),
    Route('d513', 'sumsq', 513, 4, 10, 'auto', True, False),
    Route('philox7', 'sumsq', 5, 8, 7, 'auto', True, False),
]
