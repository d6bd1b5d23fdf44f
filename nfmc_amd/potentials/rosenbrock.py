"""The blocked Rosenbrock target (csrc/pot_rosenbrock.hpp)."""
import math

import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _event_shape


class Rosenbrock(Potential):
    """Blocked (hybrid) Rosenbrock, the banana-shaped curved target.  The d coordinates of `event_shape`, flattened
    row-major, split into consecutive blocks of `block` coordinates (the last one may be shorter); coordinate c is a
    block head when c % block == 0:

        U(x) = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2

    (constants dropped).  Within a block the density factorises: x_head ~ N(mu, 1/(2a)) and x_c | x_{c-1} ~
    N(x_{c-1}^2, 1/(2b)), so the target can be drawn exactly by ancestral sampling.  The defaults are the 2-D case of the
    hybrid Rosenbrock of Pagani, Wiegand and Nadarajah (2022); `block = 1` is a diagonal Gaussian.  Long blocks with a
    wide head (small a) grow doubly exponentially along the block: their later coordinates overflow fp32, and nothing
    guards against it.  Validated in fp64 on the host: a and b finite and > 0, mu finite, all three finite (a and b
    nonzero) in fp32; `block` an int in 1 .. d.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch
    families (NeuTra on its VALU kernels, conditioners of at most 32 units); every other family runs on the split or
    composed path (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False
    fused_families = VALU_FAMILIES

    def __init__(self, event_shape, mu=1.0, a=0.05, b=5.0, block=2):
        if event_shape is None:
            raise ValueError('event_shape must be given')
        self.event_shape = tuple(int(v) for v in _event_shape(event_shape))
        d = self.event_size
        if d < 1:
            raise ValueError('event_shape %s must have at least one element' % (self.event_shape,))
        vals = {}
        for name, v in (('mu', mu), ('a', a), ('b', b)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) and not (torch.is_tensor(v) and v.numel() == 1):
                raise ValueError('%s must be a real scalar' % name)
            v = float(v)
            if not math.isfinite(v) or not math.isfinite(float(torch.tensor(v, dtype=torch.float32))):
                raise ValueError('%s must be finite in fp32 (the kernels read an fp32 copy), got %r' % (name, v))
            if name != 'mu' and not (v > 0.0 and float(torch.tensor(v, dtype=torch.float32)) > 0.0):
                raise ValueError('%s must be > 0 in fp32, got %r' % (name, v))
            vals[name] = v
        if isinstance(block, bool) or not isinstance(block, int):
            raise ValueError('block must be an int, got %r' % (block,))
        if not 1 <= block <= d:
            raise ValueError('block must lie in 1 .. d = %d, got %d' % (d, block))
        self.dim = d
        self.mu, self.a, self.b = vals['mu'], vals['a'], vals['b']   # fp64 masters; the kernels get fp32
        self.block = int(block)
        self._dev = {}

    def _tables(self, device, dtype):
        """(head mask (d,), weights a / b (d,), mu (1,)) of `device` in `dtype`, made once per (device, dtype)"""
        def make():
            head = torch.arange(self.dim, device=device) % self.block == 0
            w = torch.where(head, torch.tensor(self.a, dtype=torch.float64), torch.tensor(self.b, dtype=torch.float64))
            return head, w.to(device, dtype), torch.tensor([self.mu], dtype=dtype, device=device)
        return self._cached((str(device), dtype), make)

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        head, w, mu = self._tables(xf.device, xf.dtype)
        prev2 = torch.cat([torch.zeros_like(xf[:, :1]), xf[:, :-1] * xf[:, :-1]], dim=1)   # x_{c-1}^2 (0 for c = 0)
        r = xf - torch.where(head, mu, prev2)
        return torch.sum(w * (r * r), dim=1)

    def descriptor(self, device):
        _, _, mu = self._tables(device, torch.float32)
        return hip.NfmcPotential(hip.POT_ROSENBROCK, self.block, hip.ptr(mu), None, self.a, self.b)
