"""What every potential kind shares on the host: the launch families, the `Potential` base class with its device cache
and routing, and the checks the constructors apply (the host-side counterpart of csrc/pot_kinds.hpp and
csrc/pot_shared.hpp).  Every check raises ValueError with the text its callers document; the variable words of a
message are arguments."""
import math
import numbers
from typing import Tuple

import torch

from .. import hip


# Launch families a closed-form potential can be routed to (Potential.fused_in):
#   'mcmc'          mala / ula / mh / hmc / uhmc, device warmup tuning, the jump_* inner loop and its fused jump tail
#   'flow_mh'       the flow-MH step of imh / adaptive_imh / jump_* / dlmc (nfmc_flow_mh_steps_f32)
#   'imh_parallel'  the data-parallel FixedIMH kernel (nfmc_imh_parallel_f32)
#   'neutra'        the NeuTra gradient and HMC kernels
#   'dlmc_step'     dlmc's fused gradient step (nfmc_dlmc_step_f32)
#   'fit'           the device variational fit (nfmc_flow_variational_fit_step_f32)
FAMILIES = ('mcmc', 'flow_mh', 'imh_parallel', 'neutra', 'dlmc_step', 'fit')
# the families of every kind with units of its own (csrc/pot_kinds.hpp): its mcmc and flow-MH units, NeuTra's VALU kernels
VALU_FAMILIES = ('mcmc', 'flow_mh', 'neutra')


class Potential:
    """Base: `event_shape`, `__call__(x) -> (n,)` in torch ops, `descriptor(device)` for the kernels."""

    event_shape: Tuple[int, ...]
    # NeuTra may present this kind to its matrix-core kernels (csrc/neutra_mfma.hip), which evaluate quadratic and funnel
    # targets only: every other kind of the NeuTra family sets it False and keeps the flow's own width (VALU kernels)
    neutra_matrix_cores = True
    # the launch families whose kernels evaluate this kind, and the largest event size they take (None: the kernels decide
    # by themselves); `fused_in` reads both, and a kind with a further condition of its own and-s it on
    fused_families, fused_max_dim = FAMILIES, None

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def descriptor(self, device) -> hip.NfmcPotential:
        raise NotImplementedError

    def fused_in(self, family: str) -> bool:
        """Whether the kernels of launch family `family` (FAMILIES) may be handed this potential's descriptor.  False
        sends the family to the split or composed path, exactly as for an arbitrary callable.  The quadratic and funnel
        kinds answer True everywhere: their kernels decide by themselves, as before."""
        if family not in FAMILIES:
            raise ValueError('unknown launch family %r (one of %s)' % (family, ', '.join(FAMILIES)))
        return family in self.fused_families and (self.fused_max_dim is None or self.event_size <= self.fused_max_dim)

    def jump_tail_ok(self) -> bool:
        """Whether a jump sampler with `fuse_jump_tail` set may run the jump behind the inner kernel's launch for this
        potential (True), or should leave it on the flow-MH kernel where the tail measures slower (ParticleSystem)."""
        return True

    @property
    def event_size(self):
        return int(math.prod(self.event_shape))

    def _cached(self, key, make):
        """self._dev[key], filled by make() on first use.  `_dev` is a plain dict a constructor sets to {}; its keys are
        str(device) for a kind's one fp32 copy, (str(device), dtype) for torch-op tables and (str(device), 'descriptor')
        for descriptor blocks, so every shard of a sharded run gets its own copies."""
        if key not in self._dev:
            self._dev[key] = make()
        return self._dev[key]

    def _descriptor_blocks(self, device):
        """The pair of fp32 blocks data_block() returns, on `device`, made once per device"""
        return self._cached((str(device), 'descriptor'), lambda: tuple(v.to(device).contiguous() for v in self.data_block()))

    def _event_states(self, x):
        """`x` as a tensor, which must end in the (one-axis) event shape"""
        x = torch.as_tensor(x)
        if x.shape[-1:] != self.event_shape:
            raise ValueError('x must end in the event shape %s, got shape %s' % (self.event_shape, tuple(x.shape)))
        return x

    def _flat(self, x):
        """States that end in the event shape or in d, as (..., d)"""
        x = torch.as_tensor(x)
        k, d = len(self.event_shape), self.event_size
        if x.dim() >= k and tuple(x.shape[x.dim() - k:]) == self.event_shape:
            return x.reshape(x.shape[:x.dim() - k] + (d,))
        if x.shape[-1:] == (d,):
            return x
        raise ValueError('the states must end in the event shape %s or in d = %d, got shape %s'
                         % (self.event_shape, d, tuple(x.shape)))


def _positive_fp32(name, v):
    """float(v) of a real scalar that is > 0 and finite in fp64 and in fp32 (the kernels read an fp32 copy)"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) and not (torch.is_tensor(v) and v.numel() == 1):
        raise ValueError('%s must be a real scalar, got %r' % (name, v))
    v = float(v)
    v32 = float(torch.tensor(v, dtype=torch.float32))
    if not (v > 0.0 and math.isfinite(v) and v32 > 0.0 and math.isfinite(v32)):
        raise ValueError('%s must be > 0 and finite in fp32 (the kernels read an fp32 copy), got %r' % (name, v))
    return v


def _finite_fp32(name, v):
    """float(v) of a real scalar (a Python or numpy number, or a one-element tensor) that is finite in fp64 and in fp32
    (the kernels read an fp32 copy)"""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) and not (torch.is_tensor(v) and v.numel() == 1):
        raise ValueError('%s must be a real scalar, got %r' % (name, v))
    v = float(v)
    if not (math.isfinite(v) and math.isfinite(float(torch.tensor(v, dtype=torch.float32)))):
        raise ValueError('%s must be finite in fp32 (the kernels read an fp32 copy), got %r' % (name, v))
    return v


def _as_fp64(v):
    """`v` on the CPU in fp64; Python numbers and lists are read as fp64 at once (torch.as_tensor would round them to
    fp32 first)."""
    if isinstance(v, torch.Tensor):
        return v.detach().to('cpu', torch.float64)
    return torch.as_tensor(v, dtype=torch.float64)


def _check_finite(v, message):
    """ValueError(message) unless the fp64 tensor `v` is finite and stays finite rounded to fp32"""
    if not bool(torch.isfinite(v).all()) or not bool(torch.isfinite(v.float()).all()):
        raise ValueError(message)


def _one_of(name, v, choices):
    if v not in choices:
        raise ValueError('%s must be one of %s, got %r' % (name, ', '.join(choices), v))


def _event_shape(event_shape, d=None, note=''):
    """The event shape as a tuple; an int is one axis.  With `d` (a kind whose data fix the size): None is (d,), the
    entries are made ints and must multiply to d; `note` ends the message where d counts more than the data.  Without
    it the shape is taken as given."""
    if event_shape is None and d is not None:
        event_shape = (d,)
    elif isinstance(event_shape, int):
        event_shape = (event_shape,)
    if d is None:
        return tuple(event_shape)
    shape = tuple(int(v) for v in event_shape)
    if int(math.prod(shape)) != d:
        raise ValueError('event_shape %s must have d = %d elements%s' % (shape, d, note))
    return shape


def _pair(v, name, parts, sized=False):
    """The two entries of `v`, or ValueError '<name> must be a pair <parts>, got <v>'.  Anything that unpacks into two
    is a pair; `sized` is the reading of the two oldest callers, which index: len(v) == 2, and a string is none."""
    bad = ValueError('%s must be a pair %s, got %r' % (name, parts, v))
    if sized:
        if isinstance(v, (str, bytes)) or not hasattr(v, '__len__') or len(v) != 2:
            raise bad
        return v[0], v[1]
    try:
        a, b = v
    except (TypeError, ValueError):
        raise bad from None
    return a, b


def _spd(name, m, rtol):
    """(matrix, chol) of the fp64 CPU tensor `m`, which must be square, finite, symmetric to a relative `rtol` of its
    largest entry and positive definite: the symmetrised matrix and its lower Cholesky factor."""
    if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError('%s must be a square (d, d) matrix with d >= 1, got shape %s' % (name, tuple(m.shape)))
    if not bool(torch.isfinite(m).all()):
        raise ValueError('%s must be finite' % name)
    if float((m - m.t()).abs().max()) > rtol * float(m.abs().max()):
        raise ValueError('%s must be symmetric (to a relative %g of its largest entry)' % (name, rtol))
    m = 0.5 * (m + m.t())
    chol, info = torch.linalg.cholesky_ex(m)
    if int(info) != 0:
        raise ValueError('%s must be positive definite (its Cholesky factorisation fails)' % name)
    return m, chol


def _spd_inverse(chol):
    """The symmetrised inverse of the matrix whose lower Cholesky factor is `chol`"""
    inv = torch.cholesky_inverse(chol)
    return 0.5 * (inv + inv.t())


def _design_and_labels(X, y, D):
    """(X (N, D) fp64, y (N,) fp64) on the CPU of a design matrix, finite in fp32 too, and N labels in {0, 1}; `D` is
    the letter the caller's documentation gives the number of columns."""
    X = torch.as_tensor(X)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('X must be 2-D (N, %s) with N, %s >= 1, got shape %s' % (D, D, tuple(X.shape)))
    X = X.detach().to('cpu', torch.float64)
    _check_finite(X, 'X must be finite, in fp32 too (the kernels read an fp32 copy)')
    N = int(X.shape[0])
    y = torch.as_tensor(y).detach().to('cpu')
    if y.dim() != 1 or y.shape[0] != N:
        raise ValueError('y must be a vector of N = %d labels, got shape %s' % (N, tuple(y.shape)))
    y = y.to(torch.float64)
    if not bool(((y == 0) | (y == 1)).all()):
        raise ValueError('labels must be 0 or 1')
    return X.contiguous(), y.contiguous()
