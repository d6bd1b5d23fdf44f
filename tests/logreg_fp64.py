"""fp64 restatement of the Bayesian logistic-regression target (potentials.BayesianLogisticRegression), for the host and
GPU tests: U and its autograd gradient, and synthetic data sets with a fixed seed."""
import torch


class LogRegU64:
    """U(theta) = sum_i [log(1 + e^{z_i}) - y_i z_i] + |theta|^2 / (2 sigma^2),  z = X theta, in fp64.

    log(1 + e^z) is written as logaddexp(0, z): the textbook form, finite wherever the result is, and not the
    max + log1p form the class uses.  Callable on (n, d) tensors of any dtype; works under autograd."""

    def __init__(self, X, y, sigma):
        self.X = torch.as_tensor(X).double()
        self.y = torch.as_tensor(y).double()
        self.sigma = float(sigma)

    def __call__(self, theta):
        t = theta.reshape(theta.shape[0], -1).double()
        z = t @ self.X.t()
        data = (torch.logaddexp(torch.zeros_like(z), z) - self.y * z).sum(1)
        return data + (t * t).sum(1) / (2.0 * self.sigma ** 2)

    def grad(self, theta):
        t = theta.reshape(theta.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g


def synthetic(N, d, seed, scale=1.0, separable=False):
    """(X fp32 (N, d), y fp32 (N,), true theta) drawn with a fixed seed: y ~ Bernoulli(sigmoid(X theta)), or with
    separable=True the labels of sign(X theta), which no finite theta fits exactly."""
    g = torch.Generator().manual_seed(seed)
    X = (scale * torch.randn(N, d, generator=g)).float()
    theta = torch.randn(d, generator=g) / max(d, 1) ** 0.5
    z = X.double() @ theta.double()
    if separable:
        y = (z > 0).float()
    else:
        y = (torch.rand(N, generator=g, dtype=torch.float64) < torch.sigmoid(z)).float()
    return X, y, theta
