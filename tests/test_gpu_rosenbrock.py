"""GPU: Rosenbrock (NFMC_POT_ROSENBROCK) on the fused HIP kernels against the fp64 CPU oracle, with the target restated
in fp64 (tests/rosenbrock_fp64.py).

Targets: blocks of 1, 2, 3 and 5 coordinates (capped at d), plus one block = d target with a narrow head, so that one
chain of neighbours runs through every register quad and lane of the layout and across the lane-(LPC-1)-to-lane-0
wrap.  Starts are exact (ancestral) draws of the target.  Block 2 has a wide head around 0.5; longer blocks a narrower one
around 0.2 and a tighter conditional, so that x_{c-1}^2 stays O(1) along the block.  Step sizes scale with the largest
diagonal Hessian entry at the start (90th percentile over the chains), as any sampler of a curved target must.

Tolerances are the full-rank Gaussian tests' (tests/test_gpu_fullrank.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

d in {1, 3, 8, 25, 64, 130, 256, 512} covers every (CPL, LPC) layout choose_cfg picks (LPC 1 ... 64, CPL 4 / 8 / 16).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from rosenbrock_fp64 import RosenbrockU64

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _params(d, blk):
    """(mu, a, b): block <= 2 a wide head; longer blocks a narrow head and a tight conditional; block = d > 5 (the
    neighbour chain through the whole layout) mu = 0 and a very narrow head"""
    if blk <= 2:
        return 0.5, 2.0, 10.0
    if blk == d and d > 5:
        return 0.0, 50.0, 20.0
    return 0.2, 8.0, 16.0


def _problem(d, blk, params=None):
    from nfmc_amd.potentials import Rosenbrock
    mu, a, b = params if params is not None else _params(d, blk)
    return Rosenbrock(d, mu=mu, a=a, b=b, block=blk), RosenbrockU64(d, mu, a, b, blk)


def _x0(ref, n, seed):
    return ref.draw(n, seed).float()


def _lmax(ref, x0):
    return float(torch.quantile(ref.hess_diag(x0.double()).abs().amax(dim=1), 0.9))


def _compare(got, tr, what):
    want = tr.stacked().float()
    n = want.shape[1]
    keep = torch.ones(n, dtype=torch.bool)
    if tr.log_ratios:
        lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
        lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
        keep = ((lu - lr).abs() >= MARGIN).all(0)
    excluded = 1.0 - float(keep.float().mean())
    print('%s: %.1f %% of the chains excluded as near-ties' % (what, 100 * excluded))
    assert excluded < 0.10, (what, excluded)
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got[:, keep].numpy(), want[:, keep].numpy(), atol=ATOL, rtol=RTOL, err_msg=what)


def _sampler(kind, d, pot, T, h, L=5, imd=None):
    from nfmc_amd.samplers import mcmc
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        s = cls((d,), pot, mcmc.LangevinKernel(event_size=d, step_size=h), mcmc.LangevinParameters(n_iterations=T))
    elif kind == 'mh':
        s = mcmc.MH((d,), pot, None, mcmc.MHParameters(n_iterations=T))
        s.kernel.inv_mass_diag = imd.float()
    else:
        cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
        s = cls((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                mcmc.HMCParameters(n_iterations=T))
    return s


def _mh_scale(d, lm):
    return torch.full((d,), 0.5 / math.sqrt(d * lm), dtype=torch.float64)


def _oracle(kind, x0, target, T, h, noise, L=5, imd=None):
    from oracle import samplers as osamp
    okind = {'mala': 'langevin', 'ula': 'langevin', 'mh': 'mh', 'hmc': 'hmc', 'uhmc': 'hmc'}[kind]
    return osamp.mcmc_sample(x0.double(), target, okind, T, h, n_leapfrog=L, adjustment=kind not in ('ula', 'uhmc'),
                             noise=noise, inv_mass_diag=imd if kind == 'mh' else None)


def _step(kind, d, lm):
    """MALA h ~ d^(-1/3) / lambda_max; HMC h ~ d^(-1/4) / sqrt(lambda_max)"""
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * d ** (-1 / 4) / math.sqrt(lm)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * d ** (-1 / 3) / lm


class _Record:
    """Hands every fused mcmc launch of `sampler` mask and log-ratio buffers and keeps them (T, n)."""

    def __init__(self, monkeypatch, sampler):
        self.masks, self.log_ratios = [], []
        cls = type(sampler)
        orig = cls._launch

        def launch(s, run, pot, k, step0, samples, masks_out=None, log_ratio_out=None, **kw):
            if masks_out is None:
                masks_out = torch.zeros(k, run.n, dtype=torch.uint8, device=run.dev)
            if log_ratio_out is None:
                log_ratio_out = torch.zeros(k, run.n, dtype=torch.float32, device=run.dev)
            self.masks.append(masks_out)
            self.log_ratios.append(log_ratio_out)
            return orig(s, run, pot, k, step0, samples, masks_out=masks_out, log_ratio_out=log_ratio_out, **kw)
        monkeypatch.setattr(cls, '_launch', launch)

    def stacked(self):
        return torch.cat(self.masks).cpu().bool(), torch.cat(self.log_ratios).cpu()


def _compare_decisions(rec, tr, kind, x0, ref, what):
    """Accept masks and log ratios against the oracle's on the rows before a chain's first disagreeing decision.  Log
    ratios to 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) |U(x)|."""
    got_m, got_lr = rec.stacked()
    if kind in ('ula', 'uhmc'):
        assert bool(got_m.all()), what
        return
    want_m = torch.stack([m.reshape(-1).bool() for m in tr.masks])
    want_lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    assert got_m.shape == want_m.shape, (got_m.shape, want_m.shape)
    same = got_m == want_m
    agree = torch.cumprod(torch.cat([torch.ones(1, same.shape[1], dtype=torch.bool), same[:-1]]).int(), 0).bool()
    assert float(agree.float().mean()) > 0.9, what
    assert float(same[agree].float().mean()) > 0.97, what
    d = x0.shape[1]
    states = tr.stacked()
    prev = torch.cat([x0.double()[None], states[:-1].double()])
    u_prev = ref(prev.reshape(-1, d)).reshape(prev.shape[:2])
    err = (got_lr.double() - want_lr).abs()
    tol = 2e-4 * max(1.0, d / 64) + 1e-4 * want_lr.abs() + 8 * 2.0 ** -24 * u_prev.abs()
    print('%s: worst log-ratio error %.2e' % (what, float(err[agree].max())))
    assert bool((err[agree] <= tol[agree]).all()), (what, float(err[agree].max()))


class _Spy:
    """Counts the split-path transitions of the mcmc samplers (none on the fused route).  A sampler class that holds
    `_split_step` in its own namespace (an earlier test may have left the inherited function there) is patched too, so
    that every class's lookup reaches a counting wrapper."""

    def __init__(self, monkeypatch):
        from nfmc_amd.samplers import mcmc
        self.calls = []
        for cls in (mcmc.MCMCSampler, mcmc.MALA, mcmc.ULA, mcmc.MH, mcmc.HMC, mcmc.UHMC):
            if cls is mcmc.MCMCSampler or '_split_step' in vars(cls):
                orig = vars(cls)['_split_step']
                monkeypatch.setattr(cls, '_split_step', self._wrap(orig))

    def _wrap(self, orig):
        return lambda s, *a, **k: self.calls.append(1) or orig(s, *a, **k)


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
DIMS = [1, 3, 8, 25, 64, 130, 256, 512]


def _shapes():
    out = []
    for d in DIMS:
        for blk in sorted({min(b, d) for b in (1, 2, 3, 5)}):
            out.append((d, blk))
    out += [(64, 64), (130, 130), (512, 512)]   # one neighbour chain through every lane, narrow head
    return out


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d,blk', _shapes())
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d, blk):
    from oracle import samplers as osamp
    from nfmc_amd.samplers import mcmc
    n, T = 96, 4
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, d + 7 * blk)
    lm = _lmax(ref, x0)
    h = _step(kind, d, lm)
    imd = _mh_scale(d, lm)
    s = _sampler(kind, d, pot, T, h, imd=imd)
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(d + blk)
    tr = _oracle(kind, x0, ref, T, h, rec, imd=imd)
    s.replay = (torch.stack([v.float() for v in rec.normals]),
                torch.stack([v.float() for v in rec.uniforms]) if rec.uniforms else None)
    assert mcmc.resolve_target(pot, (d,), family='mcmc') is pot
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls                                       # every transition on the fused kernel
    what = '%s d=%d block=%d' % (kind, d, blk)
    _compare(out.samples.reshape(T, n, d), tr, what)
    _compare_decisions(rec_k, tr, kind, x0, ref, what)


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d,blk', [('mala', 25, 2), ('ula', 8, 3), ('mh', 130, 5), ('hmc', 64, 2), ('uhmc', 3, 3),
                                        ('hmc', 512, 512), ('mala', 256, 3)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, blk):
    from oracle import samplers as osamp
    n, T, seed = 160, 5, 777 + d
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, d)
    lm = _lmax(ref, x0)
    h = _step(kind, d, lm)
    imd = _mh_scale(d, lm)
    s = _sampler(kind, d, pot, T, h, imd=imd)
    s.seed = seed
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    tr = _oracle(kind, x0, ref, T, h, osamp.PhiloxNoise(seed, dtype=torch.float64), imd=imd)
    what = 'native %s d=%d block=%d' % (kind, d, blk)
    _compare(out.samples.reshape(T, n, d), tr, what)
    _compare_decisions(rec_k, tr, kind, x0, ref, what)


def _flow_pair(d, seed=5, n_hidden=None, spline=False):
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.util import create_flow_object
    from oracle import flow as oflow
    ck = {} if n_hidden is None else {'conditioner_kwargs': {'n_hidden': n_hidden}}
    if spline:
        of = oflow.perturb_(oflow.Flow(oflow.CRQNSF((d,))), seed, 0.3, 0.75)
        f = create_flow_object('c-rqnsf', (d,))
    else:
        of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,), **ck)), seed, 0.2, 0.7071)
        f = Flow(RealNVP((d,), **ck))
    f.load_state_dict(of.state_dict())
    return f, of.double()


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d,blk', [(5, 2), (25, 3), (64, 2)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d, blk):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, T, Kin, seed = 192, 3, 4, 31337
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, 3)
    f, of = _flow_pair(d)
    h = 0.3 * d ** (-1 / 3) / _lmax(ref, x0)
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), None,
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.inner_sampler.kernel.step_size = h
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    out = s.sample(x0, show_progress=False)
    assert not spy.calls and not split                        # inner loop and jump fused
    if not fuse_tail:
        assert len(flow_mh) == T                              # each jump on the flow-MH kernel
    tr = osamp.jump_sample(x0.double(), ref, of, 'langevin', T, Kin, h, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < ATOL + RTOL * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > 0.95, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= max(2, int(0.03 * n * T))


def _imh_run(monkeypatch, pot, d, f, x0, T, seed):
    from nfmc_amd.samplers import imh
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=T))
    s.seed = seed
    calls = {'launch_imh_parallel': 0, 'launch_flow_mh': 0, 'split_flow_mh': 0}

    def spy(name):
        fn = getattr(imh, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        monkeypatch.setattr(imh, name, wrapped)
    for name in list(calls):
        spy(name)
    out = s.sample(x0, show_progress=False)
    assert calls['launch_flow_mh'] >= 1 and calls['launch_imh_parallel'] == 0 and calls['split_flow_mh'] == 0, calls
    assert out.statistics.n_attempted_trajectories == x0.shape[0] * T
    return out


@pytest.mark.parametrize('d,blk', [(2, 2), (25, 5), (64, 64), (256, 3)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, blk):
    from oracle import samplers as osamp
    n, T, seed = 256, 6, 4711 + d
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, 9)
    f, of = _flow_pair(d, 9)
    out = _imh_run(monkeypatch, pot, d, f, x0, T, seed)
    tr = osamp.imh_sample(x0.double(), ref, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, 'imh d=%d block=%d' % (d, blk))


@pytest.mark.parametrize('d,blk', [(6, 2), (33, 3)])
def test_spline_flow_imh_matches_oracle(dev, monkeypatch, d, blk):
    """A 'c-rqnsf' flow: the spline instantiations of the register flow-MH kernel for kind 5."""
    from oracle import samplers as osamp
    n, T, seed = 256, 5, 99 + d
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, 11)
    f, of = _flow_pair(d, 3, spline=True)
    out = _imh_run(monkeypatch, pot, d, f, x0, T, seed)
    tr = osamp.imh_sample(x0.double(), ref, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, 'c-rqnsf imh d=%d block=%d' % (d, blk))


def test_dual_chain_override_does_not_apply(dev, monkeypatch):
    """The dual-chain flow-MH kernel evaluates exact-fit quadratic targets only: with its override on, a kind-5 run
    still takes the one-chain register kernel and gives bitwise the same states."""
    d, n, T, seed = 256, 512, 3, 5
    pot, ref = _problem(d, 2)
    x0 = _x0(ref, n, 12)
    f, _ = _flow_pair(d, 4)
    outs = []
    for dual in (None, '1'):
        if dual:
            monkeypatch.setenv('NFMC_FLOWB_DUAL', dual)
        outs.append(_imh_run(monkeypatch, pot, d, f, x0, T, seed).samples)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d,blk', [('mala', 25, 2), ('hmc', 9, 3), ('mh', 64, 5), ('hmc', 130, 130)])
def test_fused_equals_split(dev, monkeypatch, kind, d, blk):
    n, T = 200, 6
    pot, ref = _problem(d, blk)
    x0 = _x0(ref, n, 17)
    lm = _lmax(ref, x0)
    outs, counts = [], []
    for target, fuse in ((pot, 'auto'), (lambda x: pot(x), 'never')):
        spy = _Spy(monkeypatch)
        s = _sampler(kind, d, target, T, _step(kind, d, lm), imd=_mh_scale(d, lm))
        s.seed, s.fuse = 2024, fuse
        outs.append(s.sample(x0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T]
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < ATOL
    assert same.float().mean() > 0.95, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 4. NeuTra (VALU kernels)
def _neutra_grad(dev, f, pot, z):
    from nfmc_amd import hip
    n, d = z.shape
    st, _keep = f.bijection.packed(dev, 0)          # the flow's own width, as NeuTra presents it for this target
    pd = pot.descriptor(dev)
    zd = z.to(dev, torch.float32).contiguous()
    u = torch.empty(n, device=dev)
    g = torch.empty(n, d, device=dev)
    rc = int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(pd), hip.ptr(zd), n, hip.ptr(u), hip.ptr(g),
                                                        hip.stream()))
    torch.cuda.synchronize()
    return rc, u.cpu(), g.cpu()


@pytest.mark.parametrize('d,nh,blk', [(2, 4, 2), (3, 8, 3), (8, 16, 5), (25, 32, 2), (64, 8, 3), (64, 32, 64),
                                      (128, 16, 2), (130, 8, 5), (256, 4, 2)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh, blk):
    """U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)| and its gradient from the VALU NeuTra kernel against fp64 autograd
    through oracle/flow.py.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    pot, ref = _problem(d, blk)
    f, of = _flow_pair(d, 3, n_hidden=nh)
    n = 130
    # latents whose images under the (near-identity) flow are target-like
    z = ref.draw(n, d).requires_grad_(True)
    u_ref = osamp.neutra_adjusted_target(of, ref, (d,))(z)
    g_ref, = torch.autograd.grad(u_ref.sum(), z)
    rc, u, g = _neutra_grad(dev, f, pot, z.detach())
    assert rc == hip.OK
    ur = u_ref.detach()
    np.testing.assert_allclose(u.numpy(), ur.numpy(), atol=2e-4 * (1 + float(ur.abs().max())), rtol=0)
    err = (g.double() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1))
    print('d=%d H=%d block=%d: worst relative gradient error %.2e' % (d, nh, blk, float(err.max())))
    assert float(err.max()) < 2e-4


@pytest.mark.parametrize('d,nh,blk', [(8, 8, 2), (64, 16, 3), (128, 8, 2)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh, blk):
    from nfmc_amd.samplers import mcmc, neutra
    from oracle import samplers as osamp
    n, T, L = 96, 3, 4
    pot, ref = _problem(d, blk)
    z0 = _x0(ref, n, 61)
    h = 0.2 / math.sqrt(_lmax(ref, z0))
    f, of = _flow_pair(d, 9, n_hidden=nh)
    s = neutra.NeuTraHMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                         mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))
    assert s._closed_form() is pot and s._min_hidden() == 0
    split = []
    monkeypatch.setattr(s.inner_sampler, 'sample', lambda *a, **k: split.append(1))
    s.seed = 12
    out = s.sample(z0, show_progress=False)
    assert not split
    tr = osamp.neutra_hmc_sample(z0.double(), ref, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 6


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc, neutra
    from oracle import samplers as osamp
    d, n, T, L = 64, 96, 3, 4
    pot, ref = _problem(d, 2)
    z0 = _x0(ref, n, 62)
    h = 0.2 / math.sqrt(_lmax(ref, z0))
    f, of = _flow_pair(d, 9, n_hidden=64)
    rc, _u, _g = _neutra_grad(dev, f, pot, z0)
    assert rc == hip.EUNSUPPORTED
    s = neutra.NeuTraHMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                         mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))
    split = []
    orig = s.inner_sampler.sample
    s.inner_sampler.sample = lambda *a, **k: split.append(1) or orig(*a, **k)
    s.seed = 12
    out = s.sample(z0, show_progress=False)
    assert split == [1]
    tr = osamp.neutra_hmc_sample(z0.double(), ref, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())


# ------------------------------------------------------------------------- 5. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc, imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    d, n = 64, 256
    pot, ref = _problem(d, 2)
    x = _x0(ref, n, 4).to(dev)
    f, _ = _flow_pair(d)
    f.to(dev)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_ROSENBROCK and pd.reserved == 2
    a, _keep = dlmc.step_args(f, x, 0.05, pot=pot)
    assert int(hip.lib().nfmc_dlmc_step_supported_f32(C.byref(a))) == hip.EUNSUPPORTED
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k3 = _flow_mh_probe_args(run, f, pot, logq, True)
    assert int(hip.lib().nfmc_imh_parallel_supported_f32(C.byref(pa))) == hip.EUNSUPPORTED
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK        # the register kernels take it
    pa.rng.rounds = 7                                                               # the opt-in stream: not for kind 5
    before = run.x.clone()
    assert int(hip.lib().nfmc_flow_mh_steps_f32(C.byref(pa), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(run.x, before)
    # a wide conditioner (one-chain-per-lane / matrix-core flow-MH kernels): refused, never evaluated as a quadratic
    fw, _ = _flow_pair(d, 5, n_hidden=48)
    fw.to(dev)
    pw, _k4 = _flow_mh_probe_args(run, fw, pot, logq, True)
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pw))) == hip.EUNSUPPORTED
    pw.x, pw.logq, pw.n_steps = hip.ptr(x), hip.ptr(logq), 1
    before = x.clone()
    assert int(hip.lib().nfmc_flow_mh_steps_f32(C.byref(pw), hip.stream())) == hip.EUNSUPPORTED
    # NeuTra on the matrix cores (d = 64, 48 units): the gradient and the trajectory entry points
    u = torch.full((n,), 123.0, device=dev)
    gr = torch.full_like(x, 123.0)
    stw, _k5 = fw.bijection.packed(dev)
    rc = int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(stw), C.byref(pd), hip.ptr(x), n, hip.ptr(u), hip.ptr(gr),
                                                        hip.stream()))
    assert rc == hip.EUNSUPPORTED
    na = hip.NfmcNeutraHmcArgs()
    na.z, na.n, na.n_steps, na.n_leapfrog, na.step_size, na.adjust = hip.ptr(x), n, 1, 2, 0.01, 1
    na.flow, na.pot = stw, pd
    na.rng.seed = 3
    assert int(hip.lib().nfmc_neutra_hmc_steps_f32(C.byref(na), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((u == 123.0).all()) and bool((gr == 123.0).all())
    assert not pot.fused_in('fit') and not pot.fused_in('imh_parallel') and not pot.fused_in('dlmc_step')


def test_philox7_and_bad_descriptors_are_refused(dev):
    """The opt-in Philox4x32-7 stream has no kind-5 kernel (and sample(..., rng_rounds=7) raises ValueError); a NULL mu,
    a block of 0 or past d and a or b not positive and finite are argument errors, at the mcmc, flow-MH and NeuTra entry
    points alike.  Nothing is written."""
    from nfmc_amd import hip, sample
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    d, n = 25, 128
    pot, ref = _problem(d, 3)
    x = _x0(ref, n, 8).to(dev)
    before = x.clone()
    bad = []
    for field, value in (('a', 0), ('reserved', 0), ('reserved', d + 1), ('reserved', -1), ('a_scalar', 0.0),
                         ('a_scalar', -1.0), ('a_scalar', float('inf')), ('b_scalar', 0.0), ('b_scalar', float('nan'))):
        p = pot.descriptor(dev)
        setattr(p, field, value)
        bad.append(p)
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = hip.ptr(x), n, d, 2, 0.01, 1
    a.pot = pot.descriptor(dev)
    a.rng.seed, a.rng.rounds = 3, 7
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    a.rng.rounds = 10
    for p in bad:
        a.pot = p
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EINVAL
    hm = hip.NfmcHmcArgs()
    hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = hip.ptr(x), n, d, 2, 0.01, 1, 3
    hm.rng.seed = 3
    for p in bad:
        hm.pot = p
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), hip.stream())) == hip.EINVAL
    f, _ = _flow_pair(d)
    f.to(dev)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k = _flow_mh_probe_args(run, f, pot, logq, True)
    st, _k2 = f.bijection.packed(dev)
    u = torch.empty(n, device=dev)
    g = torch.empty_like(x)
    for p in bad:
        pa.pot = p
        assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.EINVAL
        assert int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(p), hip.ptr(x), n, hip.ptr(u), hip.ptr(g),
                                                              hip.stream())) == hip.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    with pytest.raises(ValueError):
        sample(pot, flow=None, strategy='mala', n_iterations=2, n_chains=32, show_progress=False, seed=1,
               x0=x[:32].cpu(), rng_rounds=7)


# ------------------------------------------------------------------------- 6. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    from nfmc_amd.dist import Shard
    d, n, T = 20, 300, 8
    pot, ref = _problem(d, 3)
    x0 = _x0(ref, n, 44)
    h = _step(kind, d, _lmax(ref, x0))
    runs = []
    for _ in range(2):
        s = _sampler(kind, d, pot, T, h)
        s.seed = 7
        runs.append(s.sample(x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories
    dense = runs[0].samples.reshape(T, n, d)
    parts = []
    for r in range(2):
        sh = Shard(rank=r, world=2)
        sh.merge_statistics = lambda s_: s_
        s = _sampler(kind, d, pot, T, h)
        s.seed, s.shard = 7, sh
        parts.append(s.sample(x0, show_progress=False).samples.reshape(T, -1, d))
    assert torch.equal(torch.cat(parts, 1), dense)


def test_sample_api_with_a_two_dimensional_event(dev):
    """nfmc_amd.sample() takes the object and its (2, 4) event shape; the kernels see the flattened d = 8."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import Rosenbrock
    pot = Rosenbrock((2, 4), mu=0.5, a=2.0, b=10.0, block=2)
    ref = RosenbrockU64(8, 0.5, 2.0, 10.0, 2)
    x0 = ref.draw(64, 1).float()
    out = sample(pot, flow=None, strategy='hmc', n_iterations=5, n_chains=64, show_progress=False, seed=1,
                 x0=x0.reshape(64, 2, 4), kernel_kwargs={'step_size': 0.2 / math.sqrt(_lmax(ref, x0)),
                                                         'n_leapfrog_steps': 3})
    assert out.samples.shape[-2:] == (2, 4)
    assert torch.isfinite(out.samples).all() and out.statistics.n_attempted_trajectories == 64 * 5


# ------------------------------------------------------------------------- 7. statistics of long fused runs
def _check_moments(kept, ref, what, slack=0.02):
    """kept (m, n, d): per-chain time averages (independent chains) give honest standard errors.
      mean      |E[x] - m_j| < 5 SE_j + slack sd_j
      variance  |V - v_j| < 5 SE_j + 2 slack v_j"""
    mean, var = ref.block2_moments()
    per_chain = kept.mean(0)
    n = kept.shape[1]
    m = per_chain.mean(0)
    se = per_chain.std(0) / math.sqrt(n)
    print(what, 'mean', m.tolist(), 'se', se.tolist())
    assert bool(((m - mean).abs() < 5 * se + slack * var.sqrt()).all()), (what, (m - mean).tolist(), se.tolist())
    sq = ((kept - mean) ** 2).mean(0)                   # per-chain second central moments about the true mean
    v = sq.mean(0)
    se2 = sq.std(0) / math.sqrt(n)
    print(what, 'var', v.tolist(), 'want', var.tolist())
    assert bool(((v - var).abs() < 5 * se2 + 2 * slack * var).all()), (what, (v - var).tolist(), se2.tolist())


def test_long_hmc_run_recovers_the_block2_moments(dev, monkeypatch):
    """d = 8 (four bananas), mu = 1, a = 0.5, b = 5, 4096 chains started from exact draws, 200 fused HMC transitions
    (L = 8), every 4th state of the last 160 kept."""
    from nfmc_amd.potentials import Rosenbrock
    d, n, T, L = 8, 4096, 200, 8
    pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=2)
    ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 2)
    x0 = ref.draw(n, 5).float()
    h = 0.2 / math.sqrt(_lmax(ref, x0))
    s = _sampler('hmc', d, pot, T, h, L=L)
    s.seed = 2718
    spy = _Spy(monkeypatch)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    assert 0.5 < acc < 1.0, acc
    kept = out.samples.reshape(T, n, d)[T // 5::4].double()
    _check_moments(kept, ref, 'hmc')
    assert torch.isfinite(out.mean).all()


def test_jump_mala_on_a_fitted_flow_recovers_the_block2_moments(dev, monkeypatch):
    """d = 4, the same bananas; a RealNVP fitted on exact draws proposes the jumps of jump_mala (fused inner loop and
    flow-MH kernel).  The jumps must be accepted at a useful rate (about 10 % for this flow) and the kept states must have
    the target's moments."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.potentials import Rosenbrock
    from nfmc_amd.samplers import jump, mcmc
    d, n, T, Kin = 4, 4096, 40, 4
    pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=2)
    ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 2)
    torch.manual_seed(2)
    f = Flow(RealNVP((d,)))
    f.fit(ref.draw(20000, 3).float(), n_epochs=100, show_progress=False)
    x0 = ref.draw(n, 4).float()
    split = []
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), None,
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.inner_sampler.kernel.step_size = 0.3 * d ** (-1 / 3) / _lmax(ref, x0)
    s.seed = 8
    out = s.sample(x0, show_progress=False)
    assert not spy.calls and not split
    acc = out.statistics.n_accepted_jumps / out.statistics.n_attempted_jumps
    print('jump acceptance', acc)
    assert acc > 0.05, acc
    kept = out.samples.reshape(T * (Kin + 1), n, d)[T:].double()
    _check_moments(kept, ref, 'jump_mala', slack=0.03)


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_proposals_are_rejected_and_counted(dev, kind):
    """Steps far past stability on a block-4 target: proposals reach |x| >~ 1e12, where b x^4 overflows fp32, so U of the
    proposal is inf and the log ratio is not finite.  The adjusted kernels reject every such proposal and count it as
    non-finite (n_nonfinite_log_ratios), as for the existing kinds; the kept states stay finite."""
    from nfmc_amd.potentials import Rosenbrock
    d, n, T = 16, 512, 10
    pot = Rosenbrock(d, mu=1.0, a=0.5, b=5.0, block=4)
    ref = RosenbrockU64(d, 1.0, 0.5, 5.0, 4)
    x0 = ref.draw(n, 3).clamp(-5, 5).float()
    h = {'mala': 1e12, 'mh': 0.0, 'hmc': 2.0}[kind]
    s = _sampler(kind, d, pot, T, h, L=3, imd=torch.full((d,), 1e24, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.isfinite(out.mean).all()
    print(kind, 'non-finite', st.n_nonfinite_log_ratios, 'accepted', st.n_accepted_trajectories)
    assert st.n_nonfinite_log_ratios > n * T // 2
    assert st.n_accepted_trajectories + st.n_nonfinite_log_ratios <= n * T
