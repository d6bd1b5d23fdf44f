"""Closed-form potential descriptors: callables (usable as `target` exactly like the reference's
`target(x) -> (n,)` callables, nfmc/sample.py:35-37) that ALSO describe themselves to the HIP kernels,
so U and grad U are evaluated in-kernel instead of by `torch.autograd.grad` (langevin.py:66-68).

The reference's own potential objects live in the absent third-party package `potentials`
(nfmc/sample.py:17); `SumOfSquares` is the README/test potential (README.md:45-46, test/util.py:4-5),
`Funnel` is the build's C4 potential.

`recognize(target, event_shape)` lets plain Python callables such as the README's
`lambda x: torch.sum(x**2, dim=1)` take the fused path: it probes the callable, fits
U = sum_j a_j (x_j - b_j)^2 + c and accepts it only if the fit reproduces the callable (and its autograd
gradient) on fresh points at radii from 0.1 to 100 and around the run's own x0 to 1e-5 relative.  It is an
inference from finitely many probes (see its docstring); `fuse='never'` turns it off.
"""
from ._base import FAMILIES, Potential
from .basic import (BayesianLogisticRegression, DiagonalGaussian, Funnel, GaussianMixture, QuadraticPotential,
                    SumOfSquares)
from .diffusion import DiffusionBridge
from .fullrank import FullRankGaussian
from .gmrf import LatentGMRF
from .irt import ItemResponseTheory
from .lgm import LatentGaussianModel
from .particles import ParticleSystem
from .phi4 import LatticePhi4
from .recognize import _announced, recognize
from .rosenbrock import Rosenbrock
from .slr import SparseLogisticRegression
from .sv import StochasticVolatility
from .vfx import VaryingEffectsRegression
