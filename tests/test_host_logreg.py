"""BayesianLogisticRegression on the host: U and grad U of the torch potential against fp64 autograd of a restatement of
its formula (tests/logreg_fp64.py), argument validation, the descriptor and the header's kind constant, and the
launch-family routing (no GPU needed)."""

import pytest
import torch

from logreg_fp64 import LogRegU64, synthetic
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, BayesianLogisticRegression, Potential, recognize
from nfmc_amd.samplers.common import resolve_target



def _u_and_grad32(pot, theta):
    t = theta.float().detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


@pytest.mark.parametrize('d', [1, 7, 25])
@pytest.mark.parametrize('N', [1, 3, 1000])
def test_u_and_grad_match_fp64_autograd(d, N):
    X, y, _ = synthetic(N, d, 100 * d + N)
    sigma = 1.7
    pot = BayesianLogisticRegression(X, y, sigma)
    ref = LogRegU64(X, y, sigma)
    theta = torch.randn(64, d, generator=torch.Generator().manual_seed(N + d), dtype=torch.float64)
    u, g = _u_and_grad32(pot, theta)
    u64, g64 = ref(theta), ref.grad(theta)
    # fp32 sums of N terms of O(1): relative 1e-5 of the sum of magnitudes
    scale_u = (ref.X.abs() @ theta.abs().t()).sum(0) + 1.0
    assert torch.all((u.double() - u64).abs() <= 1e-5 * scale_u + 1e-5)
    torch.testing.assert_close(g.double(), g64, atol=1e-4 * (N ** 0.5) + 1e-5, rtol=1e-4)
    # the closed-form gradient the kernels evaluate: X^T (sigmoid(z) - y) + theta / sigma^2
    z = theta @ ref.X.t()
    closed = (torch.sigmoid(z) - ref.y) @ ref.X + theta / sigma ** 2
    torch.testing.assert_close(g64, closed, atol=1e-9, rtol=1e-9)


@pytest.mark.parametrize('zmax', [50.0, 500.0])
def test_large_logits_stay_finite(zmax):
    """Separable data and a long theta: |z| up to `zmax`.  U is finite and equals the fp64 value to fp32 precision, the
    gradient too."""
    d, N = 7, 200
    X, y, w = synthetic(N, d, 3, separable=True)
    pot = BayesianLogisticRegression(X, y, 2.0)
    ref = LogRegU64(X, y, 2.0)
    direction = w.double() / float((X.double() @ w.double()).abs().max())
    theta = torch.stack([zmax * direction, -zmax * direction, 0.5 * zmax * direction])
    z = theta @ ref.X.t()
    assert float(z.abs().max()) == pytest.approx(zmax, rel=1e-6)
    u, g = _u_and_grad32(pot, theta)
    assert torch.isfinite(u).all() and torch.isfinite(g).all()
    u64, g64 = ref(theta), ref.grad(theta)
    torch.testing.assert_close(u.double(), u64, rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(g.double(), g64, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('kw', [
    dict(X=torch.zeros(5), y=torch.zeros(5)),                          # X not 2-D
    dict(X=torch.zeros(2, 3, 4), y=torch.zeros(2)),
    dict(X=torch.zeros(0, 3), y=torch.zeros(0)),                       # no rows
    dict(X=torch.tensor([[1.0, float('nan')]]), y=torch.zeros(1)),     # not finite
    dict(X=torch.tensor([[1.0, float('inf')]]), y=torch.zeros(1)),
    dict(X=torch.zeros(3, 2), y=torch.tensor([0.0, 1.0, 2.0])),         # label outside {0, 1}
    dict(X=torch.zeros(3, 2), y=torch.tensor([0.0, 1.0, -1.0])),        # +-1 labels are out of scope
    dict(X=torch.zeros(3, 2), y=torch.tensor([0.0, 0.5, 1.0])),
    dict(X=torch.zeros(3, 2), y=torch.zeros(4)),                       # length mismatch
    dict(X=torch.zeros(3, 2), y=torch.zeros(3, 1)),
    dict(X=torch.zeros(3, 2), y=torch.zeros(3), prior_scale=0.0),      # prior_scale <= 0
    dict(X=torch.zeros(3, 2), y=torch.zeros(3), prior_scale=-1.0),
    dict(X=torch.zeros(3, 2), y=torch.zeros(3), prior_scale=float('inf')),
    dict(X=torch.tensor([[1e39, 0.0]], dtype=torch.float64), y=torch.zeros(1)),   # finite in fp64, inf in fp32
    dict(X=torch.zeros(3, 2), y=torch.zeros(3), prior_scale=1e-30),    # 1/s^2 overflows fp32
    dict(X=torch.zeros(3, 2), y=torch.zeros(3), prior_scale=1e30),     # 1/s^2 underflows fp32 to 0
])
def test_argument_validation(kw):
    with pytest.raises(ValueError):
        BayesianLogisticRegression(**kw)


def test_bool_and_float_labels_are_the_same_target():
    X, y, _ = synthetic(50, 4, 1)
    a = BayesianLogisticRegression(X, y.bool())
    b = BayesianLogisticRegression(X, y.double(), 1.0)
    t = torch.randn(8, 4)
    assert torch.equal(a(t), b(t))
    assert a.event_shape == (4,) and a.event_size == 4 and a.n_rows == 50


def test_descriptor_and_header_constant(monkeypatch):
    X, y, _ = synthetic(37, 5, 2)
    sigma = 0.8
    pot = BayesianLogisticRegression(X, y, sigma)
    # host copies stand in for device memory: the descriptor's fields, not its pointers, are under test here
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: t.data_ptr())
    desc = pot.descriptor(torch.device('cpu'))
    assert desc.kind == 3 == hip.POT_LOGISTIC_REGRESSION
    assert desc.n_components == 37                                   # the header's n_components: N
    assert desc.a_scalar == pytest.approx(1.0 / sigma ** 2, rel=1e-7)
    assert desc.b_scalar == 0.0
    Xd, yd = pot._dev['cpu']
    assert desc.a == Xd.data_ptr() and desc.b == yd.data_ptr()
    assert Xd.dtype == torch.float32 and Xd.shape == (37, 5) and Xd.is_contiguous() and torch.equal(Xd, X)
    assert yd.dtype == torch.float32 and torch.equal(yd, y)
    assert pot.descriptor(torch.device('cpu')).a == desc.a       # one copy per device


FUSED = {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': False, 'dlmc_step': False, 'fit': False}


def test_routing_table():
    assert set(FUSED) == set(FAMILIES)
    X, y, _ = synthetic(20, 3, 4)
    pot = BayesianLogisticRegression(X, y)
    assert isinstance(pot, Potential)
    for fam, want in FUSED.items():
        assert pot.fused_in(fam) is want, fam
        assert resolve_target(pot, (3,), family=fam) is (pot if want else None)
    assert resolve_target(pot, (3,)) is pot
    with pytest.raises(ValueError):
        pot.fused_in('transport')


def test_recognize_never_infers_a_logistic_regression():
    X, y, _ = synthetic(100, 3, 5)
    pot = BayesianLogisticRegression(X, y)
    assert recognize(lambda t: pot(t), (3,)) is None
    assert resolve_target(lambda t: pot(t), (3,), fuse='auto') is None
    assert resolve_target(lambda t: pot(t), (3,), fuse='auto', family='mcmc') is None
