"""The Metropolis uniform shared by a chain's lanes, and the lean MALA kernel.

`mala_kernel` / `hmc_kernel` with LPC >= 2 lanes per chain draw each chain's accept uniforms once per chain (lane g
of the chain draws Philox block q0 + g) instead of once per lane, and a MALA launch without per-step outputs or replay
runs a LEAN instantiation of the exact-fit quadratic kernel.  Checked here through the C ABI, at every (CPL, LPC)
layout (NFMC_SAMPLER_CFG):
  * a launch with masks_out / log_ratio_out (general kernel) and one without (lean kernel, or the same general kernel
    for the targets that have no lean one) leave bitwise the same states, moments and counters;
  * every accept mask is the Metropolis test of the kernel's own log ratio against the uniform of oracle/philox.py
    (stream 1, word step & 3 of block step >> 2), natively and with those uniforms fed through replay_uniforms.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import philox

pytestmark = pytest.mark.gpu

LAYOUTS = [(4, 1), (4, 2), (4, 4), (4, 8), (4, 16), (8, 8), (16, 4), (8, 16), (16, 8), (8, 32), (16, 16), (8, 64),
           (16, 32), (16, 64)]
SEED = 0x5EED0000000A11CE
N = 101          # chains: not a multiple of any wave's chain count, so the last wave has lanes without a chain


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from nfmc_amd import hip
    hip.lib()
    return torch.device('cuda', 0)


def _pot(kind, d, dev):
    from nfmc_amd import hip
    from nfmc_amd.potentials import Funnel, GaussianMixture
    if kind == 'quadratic':      # U = sum x^2, scalar: the exact-fit (FAST) kernels when d = CPL * LPC
        return None, hip.NfmcPotential(hip.POT_QUADRATIC, 0, None, None, 1.0, 0.0)
    if kind == 'funnel':
        p = Funnel((d,), scale=1.5)
    else:
        g = torch.Generator().manual_seed(d)
        p = GaussianMixture((d,), means=torch.randn(3, d, generator=g), scales=torch.rand(3, d, generator=g) + 0.5,
                            weights=torch.tensor([0.2, 0.5, 0.3]))
    return p, p.descriptor(dev)


def _run(dev, x0, pot, n_steps, step0, outputs, sampler='mala', replay=None, h=None):
    """One launch; returns (final x, folded statistics buffer, masks, log ratios)."""
    from nfmc_amd import hip
    n, d = x0.shape
    x = x0.clone()
    st = hip.DeviceStats(d, dev)
    masks = torch.full((n_steps, n), 7, dtype=torch.uint8, device=dev) if outputs else None
    lr = torch.full((n_steps, n), float('nan'), device=dev) if outputs else None
    a = hip.NfmcMalaArgs() if sampler == 'mala' else hip.NfmcHmcArgs()
    a.x, a.n, a.d, a.n_steps, a.adjust, a.pot = hip.ptr(x), n, d, n_steps, 1, pot
    a.step_size = h or (float(d) ** (-1 / 3) if sampler == 'mala' else 0.1)
    if sampler == 'hmc':
        a.n_leapfrog = 3
    a.rng = hip.NfmcRng(SEED, 11, step0, 0, hip.ptr(replay[0]) if replay else None, hip.ptr(replay[1]) if replay else None)
    a.stats = st.struct()
    a.samples = hip.NfmcSampleStore(None, 1, 0, 1, 0)
    a.masks_out = hip.ptr(masks, torch.uint8) if outputs else None
    a.log_ratio_out = hip.ptr(lr) if outputs else None
    fn = hip.lib().nfmc_mala_steps_f32 if sampler == 'mala' else hip.lib().nfmc_hmc_steps_f32
    hip.check(fn(C.byref(a), hip.stream()), 'steps')
    st.fold()
    torch.cuda.synchronize()
    return x, st._buf.clone(), masks, lr


def _oracle_log_u(n, n_steps, step0):
    chains = np.arange(11, 11 + n, dtype=np.uint64).astype(np.uint32)
    u = np.stack([philox.accept_uniform(SEED, chains, step0 + s) for s in range(n_steps)])
    return u, np.log(u.astype(np.float64))


def _check_masks(masks, lr, log_u):
    """accept = log u < log r wherever the decision is not within rounding of v_log_f32 of a tie."""
    m, r = masks.cpu().numpy(), lr.cpu().numpy().astype(np.float64)
    assert set(np.unique(m)) <= {0, 1}
    clear = np.abs(log_u - r) > 1e-5 * np.maximum(1.0, np.abs(r))
    assert clear.mean() > 0.99
    np.testing.assert_array_equal(m[clear], (log_u < r)[clear].astype(np.uint8))
    return m.mean()


def _case(dev, monkeypatch, cpl, lpc, kind, n_steps, step0, sampler='mala', d=None):
    monkeypatch.setenv('NFMC_SAMPLER_CFG', '%d,%d' % (cpl, lpc))
    d = d or cpl * lpc
    _, pot = _pot(kind, d, dev)
    torch.manual_seed(cpl * 1000 + lpc)
    x0 = (0.7 * torch.randn(N, d)).to(dev)
    h = None if kind == 'quadratic' else 0.02
    xg, sg, masks, lr = _run(dev, x0, pot, n_steps, step0, True, sampler, h=h)
    xl, sl, _, _ = _run(dev, x0, pot, n_steps, step0, False, sampler, h=h)
    assert torch.equal(xg, xl), 'states differ between the launches with and without outputs'
    assert torch.equal(sg, sl), 'moments / counters differ between the launches with and without outputs'
    assert torch.isfinite(lr).all()
    u, log_u = _oracle_log_u(N, n_steps, step0)
    rate = _check_masks(masks, lr, log_u)
    if kind == 'quadratic' and sampler == 'mala':
        assert 0.02 < rate < 0.98, rate   # both decisions occur, so the masks test the stream


@pytest.mark.parametrize('n_steps', [1, 3, 33, 100, 512])
@pytest.mark.parametrize('step0', [0, 1, 3, 5])
@pytest.mark.parametrize('cpl,lpc', LAYOUTS)
def test_lean_mala_equals_general_and_oracle_uniforms(dev, monkeypatch, cpl, lpc, step0, n_steps):
    _case(dev, monkeypatch, cpl, lpc, 'quadratic', n_steps, step0)


@pytest.mark.parametrize('kind', ['funnel', 'mixture'])
@pytest.mark.parametrize('step0,n_steps', [(1, 33), (5, 100), (3, 512)])
@pytest.mark.parametrize('cpl,lpc', [(4, 1), (4, 2), (8, 8), (16, 4), (8, 32), (16, 64)])
def test_shared_uniform_on_targets_without_a_lean_kernel(dev, monkeypatch, cpl, lpc, kind, step0, n_steps):
    _case(dev, monkeypatch, cpl, lpc, kind, n_steps, step0)


@pytest.mark.parametrize('step0,n_steps', [(0, 100), (3, 33)])
@pytest.mark.parametrize('cpl,lpc', [(4, 1), (4, 4), (8, 8), (8, 64)])
def test_shared_uniform_in_hmc(dev, monkeypatch, cpl, lpc, step0, n_steps):
    _case(dev, monkeypatch, cpl, lpc, 'quadratic', n_steps, step0, sampler='hmc')


@pytest.mark.parametrize('cpl,lpc', [(4, 1), (8, 8), (16, 64)])
def test_replayed_uniforms_give_the_same_decisions(dev, monkeypatch, cpl, lpc):
    """The oracle's uniforms (and normals) through replay_uniforms / replay_normals: the per-lane replay path."""
    n_steps, step0 = 33, 3
    monkeypatch.setenv('NFMC_SAMPLER_CFG', '%d,%d' % (cpl, lpc))
    d = cpl * lpc
    _, pot = _pot('quadratic', d, dev)
    torch.manual_seed(5)
    x0 = (0.7 * torch.randn(N, d)).to(dev)
    chains = np.arange(11, 11 + N, dtype=np.uint64).astype(np.uint32)
    normals = np.stack([philox.normal_field(SEED, chains, step0 + s, d, philox.TAG_NOISE) for s in range(n_steps)])
    u, log_u = _oracle_log_u(N, n_steps, step0)
    replay = (torch.from_numpy(np.ascontiguousarray(normals)).to(dev), torch.from_numpy(np.ascontiguousarray(u)).to(dev))
    _, _, masks, lr = _run(dev, x0, pot, n_steps, step0, True, replay=replay)
    _check_masks(masks, lr, log_u)
