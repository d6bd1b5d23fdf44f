"""Sparse logistic regression with a hierarchical shrinkage prior (csrc/pot_slr.hpp)."""
import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _design_and_labels, _positive_fp32


class SparseLogisticRegression(Potential):
    """Sparse logistic regression with a hierarchical shrinkage prior: the German-credit sparse model of the Inference Gym
    and the 51-dimensional benchmark of the NeuTra paper.  A global scale tau and per-coefficient local scales lambda_j
    multiply the weights, with Gamma(a, b) priors (shape a = `scale_shape`, rate b = `scale_rate`):

        tau ~ Gamma(a, b),  lambda_j ~ Gamma(a, b),  w_j ~ N(0, 1),  beta_j = tau lambda_j w_j,
        y_i ~ Bernoulli(sigmoid(z_i)),  z = X beta

    X (N, D), y (N,) of bools or numbers; an intercept is a column of ones in X, shrunk like every other column.  Sampled
    on d = 2 D + 1 unconstrained coordinates: each weight beside its log local scale, the log global scale last,

        x_{2j} = w_j,  x_{2j+1} = l_j = log lambda_j  (j = 0 .. D-1),  x_{2D} = s = log tau

    (`constrain` / `unconstrain` convert).  The order is deliberate: in the kernels' interleaved 4-block register layout
    every register quad of a lane holds 4 consecutive coordinates, so each pair (w_j, l_j) lies in one quad and only s
    crosses lanes.  With r = sigmoid(z) - y and g = X^T r, the Jacobians of the two logs included, constants dropped:

        U = sum_i [softplus(z_i) - y_i z_i] + 1/2 sum_j w_j^2 + sum_j (b e^{l_j} - a l_j) + (b e^s - a s)
        dU/dw_j = e^{s + l_j} g_j + w_j,  dU/dl_j = beta_j g_j + b e^{l_j} - a,  dU/ds = sum_j beta_j g_j + b e^s - a

    Validated in fp64 on the host: X 2-D, finite, finite in fp32 too; y N labels in {0, 1}; a and b > 0 and finite in
    fp32.  Far in the tails e^{s + l_j}, e^{l_j}, e^s or z overflow fp32; the kernels then reject the proposal and count
    its log ratio as non-finite.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra
    on its VALU kernels, conditioners of at most 32 units) for d up to 1024 (D up to 511); every other family runs on the
    split or composed path (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False   # its d = 2 D + 1 is odd, so it never meets the d = 64 / 128 test; stated all the same
    fused_families = VALU_FAMILIES

    def __init__(self, X, y, scale_shape=0.5, scale_rate=0.5):
        X, y = _design_and_labels(X, y, 'D')
        N, D = (int(v) for v in X.shape)
        self.scale_shape = _positive_fp32('scale_shape', scale_shape)
        self.scale_rate = _positive_fp32('scale_rate', scale_rate)
        self.n_rows, self.n_features = N, D
        self.event_shape = (2 * D + 1,)
        self.X, self.y = X, y            # fp64 masters; the kernels get fp32
        self._dev = {}

    def _copy(self, device, dtype=torch.float32):
        """(X, y) of `device` in `dtype`, made once per (device, dtype) (every shard of a sharded run gets its own)."""
        return self._cached((str(device), dtype), lambda: (self.X.to(device, dtype).contiguous(),
                                                           self.y.to(device, dtype).contiguous()))

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        X, y = self._copy(xf.device, xf.dtype)
        D = self.n_features
        w, l, s = xf[:, 0:2 * D:2], xf[:, 1:2 * D:2], xf[:, 2 * D]
        a, b = self.scale_shape, self.scale_rate
        z = (torch.exp(s[:, None] + l) * w) @ X.t()                                # (n, N)
        data = torch.sum(torch.nn.functional.softplus(z) - y * z, dim=1)
        prior = torch.sum(0.5 * w * w + b * torch.exp(l) - a * l, dim=1) + b * torch.exp(s) - a * s
        return data + prior

    def constrain(self, x):
        """(tau, lam, w, beta) of unconstrained states x (..., 2 D + 1): tau = e^s (...), lam = e^l (..., D), w (..., D),
        beta = tau lam w (..., D)."""
        x = self._event_states(x)
        D = self.n_features
        tau, lam, w = torch.exp(x[..., 2 * D]), torch.exp(x[..., 1:2 * D:2]), x[..., 0:2 * D:2]
        return tau, lam, w, tau[..., None] * lam * w

    def unconstrain(self, tau, lam, w):
        """The unconstrained state x (..., 2 D + 1) of (tau > 0, lam > 0 (..., D), w (..., D)); the leading shapes
        broadcast.  Inverse of `constrain`."""
        w = torch.as_tensor(w)
        dt = w.dtype if w.is_floating_point() else torch.get_default_dtype()
        tau, lam, w = (torch.as_tensor(v, dtype=dt, device=w.device) for v in (tau, lam, w))
        D = self.n_features
        if lam.dim() < 1 or lam.shape[-1] != D or w.dim() < 1 or w.shape[-1] != D:
            raise ValueError('lam and w must end in D = %d entries, got shapes %s, %s'
                             % (D, tuple(lam.shape), tuple(w.shape)))
        if not bool((tau > 0).all()) or not bool((lam > 0).all()):
            raise ValueError('tau and lam must be > 0')
        lead = torch.broadcast_shapes(tau.shape, lam.shape[:-1], w.shape[:-1])
        pairs = torch.stack(torch.broadcast_tensors(w, torch.log(lam)), dim=-1).expand(lead + (D, 2))
        return torch.cat([pairs.reshape(lead + (2 * D,)), torch.log(tau).expand(lead)[..., None]], dim=-1)

    def descriptor(self, device):
        X, y = self._copy(device)
        return hip.NfmcPotential(hip.POT_SPARSE_LOGISTIC_REGRESSION, self.n_rows, hip.ptr(X), hip.ptr(y),
                                 self.scale_shape, self.scale_rate)
