"""Sparse logistic regression on the host: argument validation (one case per rule), the defaults, U and grad U of the
torch potential against the fp64 loops of tests/sparse_logreg_fp64.py and the model's log densities, stability where the
naive forms overflow, the descriptor and the header's kind constant, the launch-family routing, the sampler factory and
the constrain / unconstrain round trip (no GPU needed)."""
import math

import pytest
import torch

from sparse_logreg_fp64 import SLRU64, log_gamma_moments, model_u64, prior_draws, start_states, synthetic
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, Potential, SparseLogisticRegression, recognize
from nfmc_amd.samplers.common import resolve_target



def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


X2 = [[1.0, 0.5], [-0.3, 2.0], [0.0, -1.0]]
Y3 = [1, 0, 1]
BAD = [
    ('X 1-D', dict(X=[1.0, 2.0], y=[1, 0]), 'X'),
    ('X 3-D', dict(X=[[[1.0]]], y=[1]), 'X'),
    ('X empty rows', dict(X=torch.zeros(0, 2), y=[]), 'X'),
    ('X empty columns', dict(X=torch.zeros(3, 0), y=Y3), 'X'),
    ('X nan', dict(X=[[1.0, float('nan')], [0.0, 0.0], [1.0, 1.0]], y=Y3), 'X'),
    ('X inf', dict(X=[[float('inf'), 0.0], [0.0, 0.0], [1.0, 1.0]], y=Y3), 'X'),
    ('X overflows fp32', dict(X=[[1e39, 0.0], [0.0, 0.0], [1.0, 1.0]], y=Y3), 'X'),
    ('y too short', dict(X=X2, y=[1, 0]), 'y'),
    ('y 2-D', dict(X=X2, y=[[1, 0, 1]]), 'y'),
    ('y not a label', dict(X=X2, y=[1, 0, 2]), 'labels'),
    ('y fractional', dict(X=X2, y=[1, 0, 0.5]), 'labels'),
    ('a zero', dict(X=X2, y=Y3, scale_shape=0.0), 'scale_shape'),
    ('a negative', dict(X=X2, y=Y3, scale_shape=-1.0), 'scale_shape'),
    ('a inf', dict(X=X2, y=Y3, scale_shape=float('inf')), 'scale_shape'),
    ('a underflows fp32', dict(X=X2, y=Y3, scale_shape=1e-50), 'scale_shape'),
    ('a not a scalar', dict(X=X2, y=Y3, scale_shape=[1.0, 2.0]), 'scale_shape'),
    ('b zero', dict(X=X2, y=Y3, scale_rate=0.0), 'scale_rate'),
    ('b nan', dict(X=X2, y=Y3, scale_rate=float('nan')), 'scale_rate'),
    ('b overflows fp32', dict(X=X2, y=Y3, scale_rate=1e40), 'scale_rate'),
    ('b a bool', dict(X=X2, y=Y3, scale_rate=True), 'scale_rate'),
]


@pytest.mark.parametrize('what,kw,name', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw, name):
    with pytest.raises(ValueError, match=name):
        SparseLogisticRegression(**kw)


def test_defaults_and_accepted_edges():
    pot = SparseLogisticRegression(X2, Y3)
    assert (pot.scale_shape, pot.scale_rate) == (0.5, 0.5)
    assert pot.n_rows == 3 and pot.n_features == 2
    assert pot.event_shape == (5,) and pot.event_size == 5
    assert pot.X.dtype == torch.float64 and pot.y.dtype == torch.float64 and pot.y.tolist() == [1.0, 0.0, 1.0]
    SparseLogisticRegression([[0.0]], [0])
    SparseLogisticRegression(torch.ones(4, 3, dtype=torch.float32), torch.tensor([True, False, True, True]),
                             scale_shape=torch.tensor(2.0), scale_rate=3)
    assert SparseLogisticRegression(torch.zeros(2, 511), [0, 1]).event_shape == (1023,)


def _points(D, N, n, seed):
    X, y, _ = synthetic(N, D, seed, scale=1.0 / math.sqrt(max(D, 1)))
    x = start_states(D, n, seed + 1, spread=1.5)
    return X, y, x


@pytest.mark.parametrize('D', [1, 2, 3, 12, 25, 64, 200, 511])
def test_u_and_grad_match_the_fp64_loop(D):
    N = 40 if D > 100 else 120
    X, y, x = _points(D, N, 16, D)
    kw = dict(scale_shape=1.5, scale_rate=0.7)
    pot = SparseLogisticRegression(X, y, **kw)
    ref = SLRU64(X, y, 1.5, 0.7)
    u64, g64 = ref(x), ref.grad(x)
    # the gradient formulas of the header, term by term
    Xd, yd = X.double(), y.double()
    w, l, s = x[:, 0:2 * D:2], x[:, 1:2 * D:2], x[:, 2 * D]
    e = torch.exp(s[:, None] + l)
    bt = e * w
    g = (torch.sigmoid(bt @ Xd.t()) - yd) @ Xd
    want = torch.empty_like(x)
    want[:, 0:2 * D:2] = e * g + w
    want[:, 1:2 * D:2] = bt * g + 0.7 * torch.exp(l) - 1.5
    want[:, 2 * D] = (bt * g).sum(1) + 0.7 * torch.exp(s) - 1.5
    torch.testing.assert_close(g64, want, rtol=1e-11, atol=1e-10)
    u, gr = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(u, u64, rtol=1e-12, atol=1e-10)
    torch.testing.assert_close(gr, g64, rtol=1e-11, atol=1e-10)
    u, gr = _u_and_grad(pot, x, torch.float32)
    mag = u64.abs() + N + D + 1.0
    assert bool(((u.double() - u64).abs() <= 2e-6 * mag).all())
    gs = 1.0 + g64.abs().amax(1, keepdim=True)
    assert bool(((gr.double() - g64).abs() <= 2e-5 * gs).all())


@pytest.mark.parametrize('D,N', [(1, 1), (3, 50), (25, 400)])
def test_u_matches_the_model_log_densities_up_to_one_constant(D, N):
    X, y, x = _points(D, N, 20, 100 + D)
    for kw in (dict(), dict(scale_shape=2.0, scale_rate=3.0)):
        pot = SparseLogisticRegression(X, y, **kw)
        diff = pot(x.double()) - model_u64(x, X, y, kw.get('scale_shape', 0.5), kw.get('scale_rate', 0.5))
        assert float(diff.max() - diff.min()) < 1e-9 * (1 + float(pot(x.double()).abs().max())), diff


def test_stable_where_the_naive_forms_overflow():
    """z far out (large scales and separable-looking data): the softplus form stays finite in fp32 where log(1 + e^z)
    overflows, and so does its gradient.  Scales whose exponential overflows fp32 give a non-finite U, which the kernels
    reject."""
    D, N = 4, 30
    X, y, _ = synthetic(N, D, 7)
    pot = SparseLogisticRegression(X, y)
    x = torch.zeros(4, 2 * D + 1, dtype=torch.float64)
    x[:, 0:2 * D:2] = 3.0
    x[0, 2 * D] = 5.0            # tau = e^5: |z| ~ 500, e^z overflows fp32
    x[1, 1:2 * D:2] = 4.0        # lambda_j = e^4
    x[2, 2 * D] = -30.0          # tau tiny: z ~ 0
    x[3, 2 * D], x[3, 1] = 3.0, 3.0
    naive = torch.log(1 + torch.exp(SLRU64(X, y).beta(x).float() @ X.t()))
    assert not bool(torch.isfinite(naive).all())   # the textbook form does overflow here
    u, g = _u_and_grad(pot, x, torch.float32)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    ref = SLRU64(X, y)
    torch.testing.assert_close(u.double(), ref(x), rtol=1e-5, atol=1e-2)
    u, g = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-10, atol=1e-8)
    far = x[:1].clone()
    far[0, 2 * D] = 100.0        # e^s overflows fp32
    assert not bool(torch.isfinite(pot(far.float())).all())


def test_descriptor_and_header_constant(monkeypatch):
    X, y, _ = synthetic(6, 3, 1)
    pot = SparseLogisticRegression(X, y, scale_shape=2.0, scale_rate=0.25)
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    desc = pot.descriptor(torch.device('cpu'))
    assert desc.kind == 7 == hip.POT_SPARSE_LOGISTIC_REGRESSION
    assert desc.n_components == 6 == pot.n_rows                    # the header's n_components: N
    assert desc.a_scalar == 2.0 and desc.b_scalar == 0.25
    X32, y32 = pot._dev[('cpu', torch.float32)]
    assert desc.a == X32.data_ptr() and desc.b == y32.data_ptr()
    assert X32.dtype == torch.float32 and X32.shape == (6, 3) and torch.equal(X32, X)
    assert y32.dtype == torch.float32 and torch.equal(y32, y)
    assert pot.descriptor(torch.device('cpu')).a == desc.a      # one copy per device


FUSED = {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True, 'dlmc_step': False, 'fit': False}


def test_routing_table():
    assert set(FUSED) == set(FAMILIES)
    pot = SparseLogisticRegression(X2, Y3)
    assert isinstance(pot, Potential)
    for fam, want in FUSED.items():
        assert pot.fused_in(fam) is want, fam
        assert resolve_target(pot, (5,), family=fam) is (pot if want else None)
    assert resolve_target(pot, (5,)) is pot
    with pytest.raises(ValueError):
        pot.fused_in('transport')


@pytest.mark.parametrize('D', [1, 4])
def test_recognize_never_infers_it(D):
    X, y, _ = synthetic(30, D, D)
    pot = SparseLogisticRegression(X, y)
    d = 2 * D + 1
    assert recognize(lambda x: pot(x), (d,)) is None
    assert resolve_target(lambda x: pot(x), (d,), fuse='never', family='mcmc') is None
    assert resolve_target(lambda x: pot(x), (d,), fuse='auto', family='mcmc') is None


@pytest.mark.parametrize('strategy', ['mala', 'hmc', 'mh', 'jump_mala', 'imh', 'neutra_hmc'])
def test_create_sampler_takes_the_event_shape_of_the_object(strategy):
    from nfmc_amd.sample import create_sampler
    X, y, _ = synthetic(20, 5, 3)
    pot = SparseLogisticRegression(X, y)
    s = create_sampler(pot, flow='realnvp' if strategy in ('jump_mala', 'imh', 'neutra_hmc') else None,
                       strategy=strategy)
    assert tuple(s.event_shape) == (11,)
    assert s.target is pot


def test_constrain_unconstrain_round_trip():
    D = 6
    X, y, _ = synthetic(10, D, 5)
    pot = SparseLogisticRegression(X, y)
    x = start_states(D, 11, 5, spread=2.0)
    tau, lam, w, beta = pot.constrain(x)
    assert tau.shape == (11,) and lam.shape == w.shape == beta.shape == (11, D)
    assert bool((tau > 0).all()) and bool((lam > 0).all())
    torch.testing.assert_close(tau, torch.exp(x[:, 2 * D]))
    torch.testing.assert_close(w, x[:, 0:2 * D:2])
    torch.testing.assert_close(beta, SLRU64(X, y).beta(x))
    torch.testing.assert_close(pot.unconstrain(tau, lam, w), x, rtol=1e-12, atol=1e-12)
    # leading dimensions (kept samples (steps, chains, d)) and broadcast scalars
    xs = x.reshape(1, 11, 2 * D + 1).expand(3, 11, 2 * D + 1)
    parts = pot.constrain(xs)
    assert parts[1].shape == (3, 11, D)
    torch.testing.assert_close(pot.unconstrain(*parts[:3]), xs, rtol=1e-12, atol=1e-12)
    one = pot.unconstrain(2.0, torch.ones(D), torch.arange(D, dtype=torch.float64))
    assert one.shape == (2 * D + 1,)
    torch.testing.assert_close(one, torch.tensor([v for j in range(D) for v in (float(j), 0.0)] + [math.log(2.0)],
                                                 dtype=torch.float64))
    with pytest.raises(ValueError):
        pot.unconstrain(-1.0, torch.ones(D), torch.zeros(D))
    with pytest.raises(ValueError):
        pot.unconstrain(1.0, torch.zeros(D), torch.zeros(D))
    with pytest.raises(ValueError):
        pot.unconstrain(1.0, torch.ones(D + 1), torch.zeros(D + 1))
    with pytest.raises(ValueError):
        pot.constrain(torch.zeros(4, 2 * D))


def test_synthetic_data_and_prior_draws():
    X1, y1, b1 = synthetic(500, 25, 9)
    X2_, y2, b2 = synthetic(500, 25, 9)
    assert torch.equal(X1, X2_) and torch.equal(y1, y2) and torch.equal(b1, b2)
    assert int((b1 != 0).sum()) == 3
    torch.testing.assert_close(X1.double().mean(0), torch.zeros(25, dtype=torch.float64), atol=1e-5, rtol=0)
    torch.testing.assert_close(X1.double().std(0), torch.ones(25, dtype=torch.float64), atol=1e-5, rtol=0)
    assert set(y1.tolist()) <= {0.0, 1.0}
    x = prior_draws(3, 200000, 2.0, 2.0, 4)
    m, v = log_gamma_moments(2.0, 2.0)
    assert abs(float(x[:, 1].mean()) - m) < 0.01 and abs(float(x[:, 1].var()) / v - 1) < 0.02
    assert abs(float(x[:, 6].mean()) - m) < 0.01 and abs(float(x[:, 0].var()) - 1) < 0.02


def test_hessian_diagonal_matches_autograd():
    D = 4
    X, y, x = _points(D, 30, 6, 21)
    ref = SLRU64(X, y, 1.5, 0.7)
    hd = ref.hess_diag(x)
    for i in range(x.shape[0]):
        H = torch.autograd.functional.hessian(lambda v: ref(v[None])[0], x[i])
        torch.testing.assert_close(hd[i], torch.diagonal(H), rtol=1e-10, atol=1e-10)
