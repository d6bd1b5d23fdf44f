"""GPU: the varying-effects regression (NFMC_POT_VARYING_EFFECTS) on the fused HIP kernels against the fp64 CPU oracle,
with the target restated in fp64 over the raw observations (tests/varying_effects_fp64.py).

A problem is (model, C): 'both' = radon with varying intercepts and slopes (d = 2 C + 5), 'int' = varying intercepts and a
shared slope, 'slo' = a shared intercept and varying slopes (d = C + 4), 'es' = varying intercepts alone with known noise
(d = C + 2; C = 8 is eight schools itself, Rubin's data), optionally with known noise ('scalar' / 'vector') and
non-centered.  Data: VaryingEffectsRegression.synthetic(C, 2 C + 7, a seed per model and C).  Chains start at
varying_effects_fp64.start_states(seed = d + 1): the generating state (for eight schools: theta = y, mu = mean(y),
tau = std(y)) plus about one posterior standard deviation per coordinate.  The oracle samplers evaluate the model's log
densities from torch.distributions in fp64 over the observations (model_u64: independent of the kernels, the class and the
sufficient statistics).  The mass diagonals come from H = the median over the starts of the positive fp64 diagonal Hessian:
MALA inv_mass_diag = sqrt(H) with step min(0.5, 2.5 d^(-1/3)), HMC 1 / H with step min(0.4, 1.6 d^(-1/4)) and 5 leapfrog
steps (2 at d = 1023), MH 0.5 / sqrt(d H); ula and uhmc take a quarter of the mala and hmc steps (with no rejection the
oracle's own chains leave fp64 at C <= 4 otherwise: 1e300 within four transitions).  The caps are this posterior's: it is a funnel, and at d < 10 the
item-response tests' uncapped steps send a tenth to a quarter of the oracle's own HMC trajectories to a NaN energy.

Tolerances are the item-response tests' (tests/test_gpu_irt.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN = 2e-3 at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.
The oracle ALONE, run on the CPU with these starts and steps over the whole grid of test 1 (mala, mh and hmc), excludes at
most 2.1 % of the chains (two of 96), under the 5 % the starts and steps were chosen for; its acceptance is 0.39 to 0.92
for mala, 0.70 to 0.81 for mh and 0.76 to 0.98 for hmc (1.0 at d = 1023, two leapfrog steps).  _compare prints the share of
every case.

Shapes: 'both' at C = 1, 2, 5, 6, 14, 30, 62, 126, 254, 509 is d = 7, 9, 15, 17, 33, 65, 129, 257, 513, 1023, the default
layouts (4, 2), (4, 4), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64), (16, 64), (16, 64)
(tests/test_host_varying_effects.py asks the library); 2 C mod 4 is 2 for odd and 0 for even C, so the five globals start
mid-quad and on a quad boundary; with known noise d = 2 C + 4 = 16 and 32 fill their layouts with no padding.  'int' and
'slo' at C = 1, 2, 3, 4, 13, 61 put the four globals at every residue of C mod 4; 'es' at C = 1, 2 is layout (4, 1)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from varying_effects_fp64 import VFX64, model_u64, start_states

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4

MODELS = {'both': ('varying', 'varying'), 'int': ('varying', 'shared'), 'slo': ('shared', 'varying'), 'es': ('varying', 'none')}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


class _Problem:
    """potential, fp64 restatement, fp64 oracle target, starts x0 fp32 (n, d), H (d,) fp64"""

    def __init__(self, model, Cn, n, known=None, centered=True):
        from nfmc_amd.potentials import VaryingEffectsRegression
        ia, sl = MODELS[model]
        N = 2 * Cn + 7
        known = 'vector' if model == 'es' and known is None else known
        kw = dict(intercepts=ia, slopes=sl, centered=centered)
        if model == 'es' and Cn == 8:
            pot = VaryingEffectsRegression.eight_schools(centered=centered)
            y = pot.y
            theta, mu, tau = y, y.mean(), y.std()
            truth = pot.pack(a=theta if centered else (theta - mu) / tau, mu_a=mu, s_a=tau.log())
        else:
            if known == 'scalar':
                kw['noise_scale'] = 0.8
            elif known == 'vector':
                kw['noise_scale'] = 0.5 + torch.arange(N, dtype=torch.float64) / N
            seed = Cn + {'both': 1000, 'int': 2000, 'slo': 3000, 'es': 4000}[model] + (500 if known else 0) + (250 if not centered else 0)
            pot, truth = VaryingEffectsRegression.synthetic(Cn, N, seed, **kw)
        self.pot, self.truth, self.d = pot, truth, pot.event_size
        okw = dict(y=pot.y, group=pot.group, intercepts=ia, slopes=sl, noise_scale=pot.noise_scale, centered=centered,
                   location_scale=pot.location_scale, scale_scale=pot.scale_scale)
        self.ref = VFX64(x=pot.x, **okw)
        self.target = functools.partial(model_u64, xcov=pot.x, **okw)
        x0 = start_states(self.ref, truth, n, self.d + 1)
        self.x0 = x0.float()
        self.H = self.ref.hess_diag(x0).median(0).values
        self.name = '%s C=%d d=%d%s%s' % (model, Cn, self.d, ' known-' + known if known else '', '' if centered else ' non-centered')

    def imd(self, kind):
        if kind in ('mala', 'ula'):
            return torch.sqrt(self.H)
        if kind in ('hmc', 'uhmc'):
            return 1 / self.H
        return 0.5 / torch.sqrt(self.d * self.H)

    def step(self, kind):
        f = 0.25 if kind in ('ula', 'uhmc') else 1.0      # no rejection to stop a chain that runs down the funnel
        if kind in ('mala', 'ula'):
            return f * min(0.5, 2.5 * self.d ** (-1 / 3))
        return f * min(0.4, 1.6 * self.d ** (-1 / 4)) if kind in ('hmc', 'uhmc') else 0.0


@functools.lru_cache(maxsize=None)
def _problem(model, Cn, n, known=None, centered=True):
    return _Problem(model, Cn, n, known, centered)


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


def _sampler(kind, p, T, L=5, target=None, h=None, imd=None):
    from nfmc_amd.samplers import mcmc
    d = p.d
    target = p.pot if target is None else target
    h = p.step(kind) if h is None else h
    imd = (p.imd(kind) if imd is None else imd).float()
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        s = cls((d,), target, mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd),
                mcmc.LangevinParameters(n_iterations=T))
    elif kind == 'mh':
        s = mcmc.MH((d,), target, mcmc.MHKernel(event_size=d, inv_mass_diag=imd), mcmc.MHParameters(n_iterations=T))
    else:
        cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
        s = cls((d,), target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h, inv_mass_diag=imd),
                mcmc.HMCParameters(n_iterations=T))
    return s


def _oracle(kind, p, T, noise, L=5):
    from oracle import samplers as osamp
    okind = {'mala': 'langevin', 'ula': 'langevin', 'mh': 'mh', 'hmc': 'hmc', 'uhmc': 'hmc'}[kind]
    tr = osamp.mcmc_sample(p.x0.double(), p.target, okind, T, p.step(kind), n_leapfrog=L,
                           adjustment=kind not in ('ula', 'uhmc'), noise=noise, inv_mass_diag=p.imd(kind).float().double())
    if kind in ('mala', 'mh', 'hmc'):
        print('%s %s: oracle acceptance %.3f' % (kind, p.name, tr.n_accepted / (p.x0.shape[0] * T)))
    return tr


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
    ratios to 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) |U(x)|: the kernel's U(x) and U(x') are fp32 numbers of
    that magnitude (tests/test_gpu_irt.py)."""
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
    prev = torch.cat([x0.double()[None], states[:-1].double()]).reshape(-1, d)
    mag = ref(prev).abs().reshape(states.shape[:2])
    agree = agree & torch.isfinite(want_lr) & (want_lr > -50)
    err = (got_lr.double() - want_lr).abs()
    tol = 2e-4 * max(1.0, d / 64) + 1e-4 * want_lr.abs() + 8 * 2.0 ** -24 * mag
    print('%s: worst log-ratio error %.2e' % (what, float(err[agree].max())))
    assert bool((err[agree] <= tol[agree]).all()), (what, float(err[agree].max()))


class _Spy:
    """Counts the split-path transitions of the mcmc samplers (none on the fused route)."""

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
# (model, C, known noise, centered)
GRID = ([('both', c, None, True) for c in (1, 2, 5, 6, 14, 30, 62, 126, 254, 509)]
        + [(m, c, None, True) for m in ('int', 'slo') for c in (1, 2, 3, 4, 13, 61)]
        + [('es', 8, None, True), ('es', 1, None, True), ('es', 2, None, True)]
        + [('both', 5, None, False), ('both', 30, None, False), ('int', 13, None, False), ('slo', 4, None, False),
           ('es', 8, None, False)]
        + [('both', 6, 'vector', True), ('both', 14, 'scalar', False), ('int', 3, 'vector', True)])
IDS = ['%s-%d%s%s' % (m, c, '-' + k if k else '', '' if cen else '-nc') for m, c, k, cen in GRID]


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('model,Cn,known,centered', GRID, ids=IDS)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, model, Cn, known, centered):
    from oracle import samplers as osamp
    from nfmc_amd.samplers import mcmc
    n, T = 96, 4
    p = _problem(model, Cn, n, known, centered)
    d = p.d
    L = 2 if d == 1023 else 5
    s = _sampler(kind, p, T, L=L)
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(d)
    tr = _oracle(kind, p, T, rec, L=L)
    s.replay = (torch.stack([v.float() for v in rec.normals]),
                torch.stack([v.float() for v in rec.uniforms]) if rec.uniforms else None)
    assert mcmc.resolve_target(p.pot, (d,), family='mcmc') is p.pot
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls                                       # every transition on the fused kernel
    what = '%s %s' % (kind, p.name)
    _compare(out.samples.reshape(T, n, d), tr, what)
    _compare_decisions(rec_k, tr, kind, p.x0, p.ref, what)


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,model,Cn,known,centered', [('mala', 'both', 30, None, True), ('ula', 'int', 3, None, True),
                                                           ('mh', 'both', 62, None, True), ('hmc', 'both', 5, None, False),
                                                           ('uhmc', 'es', 8, None, True), ('hmc', 'slo', 13, None, True),
                                                           ('mala', 'both', 6, 'vector', True)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, model, Cn, known, centered):
    from oracle import samplers as osamp
    n, T = 96, 4
    p = _problem(model, Cn, n, known, centered)
    seed = 777 + p.d
    s = _sampler(kind, p, T)
    s.seed = seed
    spy = _Spy(monkeypatch)
    rec_k = _Record(monkeypatch, s)
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls
    tr = _oracle(kind, p, T, osamp.PhiloxNoise(seed, dtype=torch.float64))
    what = 'native %s %s' % (kind, p.name)
    _compare(out.samples.reshape(T, n, p.d), tr, what)
    _compare_decisions(rec_k, tr, kind, p.x0, p.ref, what)


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


# ------------------------------------------------------------------------- 3. jump_mala
@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('model,Cn,centered', [('both', 5, True), ('int', 13, False), ('both', 14, True)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, model, Cn, centered):
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, T, Kin, seed = 192, 3, 4, 31337
    p = _problem(model, Cn, n, None, centered)
    d, h, imd = p.d, p.step('mala'), p.imd('mala').float()
    f, of = _flow_pair(d)
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), p.pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T),
                      mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd),
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls and not split                        # inner loop and jump fused
    if not fuse_tail:
        assert len(flow_mh) == T                              # each jump on the flow-MH kernel
    tr = osamp.jump_sample(p.x0.double(), p.target, of, 'langevin', T, Kin, h, inv_mass_diag=imd.double(),
                           noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < ATOL + RTOL * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > 0.95, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= max(2, int(0.03 * n * T))


# ------------------------------------------------------------------------- 4. imh on the sequential flow-MH kernel
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


@pytest.mark.parametrize('model,Cn,centered,spline', [('es', 1, True, False), ('both', 6, True, False), ('both', 30, False, False),
                                                      ('int', 13, True, False), ('both', 5, True, True), ('slo', 13, True, True),
                                                      ('es', 8, False, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, model, Cn, centered, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 10."""
    from oracle import samplers as osamp
    n, T = 192, 5
    p = _problem(model, Cn, n, None, centered)
    d, seed = p.d, 4711 + p.d
    f, of = _flow_pair(d, 3 if spline else 9, spline=spline)
    out = _imh_run(monkeypatch, p.pot, d, f, p.x0, T, seed)
    tr = osamp.imh_sample(p.x0.double(), p.target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    _compare(out.samples.reshape(T, n, d), tr, '%s imh %s' % ('c-rqnsf' if spline else 'realnvp', p.name))


# ------------------------------------------------------------------------- 5. fused equals split
@pytest.mark.parametrize('kind,model,Cn,centered', [('mala', 'both', 30, True), ('hmc', 'both', 5, False), ('mh', 'int', 13, True),
                                                    ('hmc', 'slo', 61, True)])
def test_fused_equals_split(dev, monkeypatch, kind, model, Cn, centered):
    n, T = 96, 4
    p = _problem(model, Cn, n, None, centered)
    d = p.d
    outs, counts = [], []
    for target, fuse in ((p.pot, 'auto'), (lambda x: p.pot(x), 'never')):
        spy = _Spy(monkeypatch)
        s = _sampler(kind, p, T, target=target)
        s.seed, s.fuse = 2024, fuse
        outs.append(s.sample(p.x0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T]
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < ATOL
    assert same.float().mean() > 0.95, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 6. NeuTra gradient (VALU kernels)
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


@pytest.mark.parametrize('model,Cn,known,centered,nh', [('es', 1, None, True, 4), ('both', 2, None, True, 8), ('both', 5, None, False, 16),
                                                        ('int', 13, None, True, 32), ('slo', 13, None, False, 8),
                                                        ('both', 30, None, True, 16), ('both', 6, 'vector', True, 4),
                                                        ('es', 8, None, True, 32)])
def test_neutra_gradient_matches_fp64_autograd(dev, model, Cn, known, centered, nh):
    """U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)| and its gradient from the VALU NeuTra kernel against fp64 autograd
    through oracle/flow.py and the model over the observations.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    n = 96
    p = _problem(model, Cn, n, known, centered)
    d = p.d
    f, of = _flow_pair(d, 3, n_hidden=nh)
    z = p.x0.double().requires_grad_(True)
    u_ref = osamp.neutra_adjusted_target(of, p.ref, (d,))(z)
    g_ref, = torch.autograd.grad(u_ref.sum(), z)
    rc, u, g = _neutra_grad(dev, f, p.pot, z.detach())
    assert rc == hip.OK
    ur = u_ref.detach()
    np.testing.assert_allclose(u.numpy(), ur.numpy(), atol=2e-4 * (1 + float(ur.abs().max())), rtol=0)
    err = (g.double() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1))
    print('%s H=%d: worst relative gradient error %.2e' % (p.name, nh, float(err.max())))
    assert float(err.max()) < 2e-4


# ------------------------------------------------------------------------- 7. NeuTra trajectories, wide conditioner
def _neutra_sampler(p, f, T, L, h):
    from nfmc_amd.samplers import mcmc, neutra
    d = p.d
    return neutra.NeuTraHMC((d,), p.pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                            mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))


@pytest.mark.parametrize('model,Cn,centered,nh', [('both', 5, True, 8), ('int', 13, False, 16), ('both', 30, True, 16)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, model, Cn, centered, nh):
    from oracle import samplers as osamp
    n, T, L = 96, 3, 4
    p = _problem(model, Cn, n, None, centered)
    d = p.d
    h = 0.2 / math.sqrt(float(p.H.max()))
    f, of = _flow_pair(d, 9, n_hidden=nh)
    s = _neutra_sampler(p, f, T, L, h)
    assert s._closed_form() is p.pot and s._min_hidden() == 0
    split = []
    monkeypatch.setattr(s.inner_sampler, 'sample', lambda *a, **k: split.append(1))
    s.seed = 12
    out = s.sample(p.x0, show_progress=False)
    assert not split
    tr = osamp.neutra_hmc_sample(p.x0.double(), p.target, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 6


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    from nfmc_amd import hip
    from oracle import samplers as osamp
    n, T, L = 96, 3, 4
    p = _problem('both', 14, n)
    d = p.d
    h = 0.2 / math.sqrt(float(p.H.max()))
    f, of = _flow_pair(d, 9, n_hidden=64)
    rc, _u, _g = _neutra_grad(dev, f, p.pot, p.x0)
    assert rc == hip.EUNSUPPORTED
    s = _neutra_sampler(p, f, T, L, h)
    split = []
    orig = s.inner_sampler.sample
    s.inner_sampler.sample = lambda *a, **k: split.append(1) or orig(*a, **k)
    s.seed = 12
    out = s.sample(p.x0, show_progress=False)
    assert split == [1]
    tr = osamp.neutra_hmc_sample(p.x0.double(), p.target, of, T, h, None, L, noise=osamp.PhiloxNoise(12, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() > 0.93, float(same.float().mean())


# ------------------------------------------------------------------------- 8. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,model,Cn,centered,n,W,every', [('mala', 'both', 5, True, 140, 12, 1),
                                                              ('hmc', 'es', 8, False, 150, 16, 2),
                                                              ('mala', 'both', 30, True, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, model, Cn, centered, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds: the controller state after the device warmup against
    oracle.samplers.replay_controller over the kernel's kept states and accept counts, every warmup transition and the
    sampling run after it shadowed in fp64.  The hmc case is eight schools, non-centered: dual averaging starts by
    doubling the step, and with an unknown noise scale and a unit mass diagonal (radon 'int', 'slo' and 'both' at C = 13,
    14) the fp64 oracle's OWN warmup then sends 18 to 35 % of the trajectories to a NaN energy (e^{-2 s_y} feeds back
    into s_y's momentum), which the shadow counts as near-ties; on eight schools it sends none."""
    from test_gpu_warmup import _Record as _Accepts, _check_controller, _controller_params, _sampler as _wsampler, _shadow
    from nfmc_amd import hip
    from oracle import samplers as osamp
    p = _problem(model, Cn, n, None, centered)
    d = p.d
    lm = float(p.H.max())
    h0 = 0.3 * (0.5 * d ** (-1 / 4) / math.sqrt(lm) if kind == 'hmc' else 0.5 * d ** (-1 / 3) / lm)
    imd0 = torch.ones(d)
    T, L, seed = 6, 4, 4242 + d
    s = _wsampler(kind, d, p.pot, W, T, h0, L=L, every=every)
    h0 = float(s.kernel.step_size)
    s.seed = seed
    rec = _Accepts(monkeypatch, s)
    wout = s.warmup(p.x0, show_progress=False)
    what = 'vfx %s %s n=%d every=%d' % (kind, p.name, n, every)
    states = wout.samples.reshape(W, n, d)
    ups, h_t, imd_t = osamp.replay_controller(states, rec.accepted(), every, _controller_params(s, h0, imd0))
    assert len(ups) == math.ceil(W / every)
    _check_controller(s, ups, what)
    _shadow(torch.cat([p.x0[None], states]), kind, p.target, h_t, imd_t, seed, hip.WARMUP_STEP0, L, what + ' warmup', 0.05)
    x1 = wout.running_samples.last_sample.cpu()
    out = s.sample(x1, show_progress=False)
    assert torch.isfinite(out.samples).all()
    _shadow(torch.cat([x1[None], out.samples.reshape(T, n, d)]), kind, p.target, s.kernel.step_size,
            s.kernel.inv_mass_diag.clone(), seed, 0, L, what + ' sampling', 0.05)


# ------------------------------------------------------------------------- 9. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc, imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    n = 256
    p = _problem('both', 14, n)
    d, pot = p.d, p.pot
    x = p.x0.to(dev)
    f, _ = _flow_pair(d)
    f.to(dev)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_VARYING_EFFECTS == 10 and pd.reserved == 14
    assert pd.a_scalar == 10.0 and pd.b_scalar == float(pot.n_obs)                  # varying + 4 varying + 8, N
    assert pd.a % 16 == 0 and pot.descriptor(dev).a == pd.a and pot.descriptor(dev).b == pd.b   # cached per device
    a, _keep = dlmc.step_args(f, x, 0.05, pot=pot)
    assert int(hip.lib().nfmc_dlmc_step_supported_f32(C.byref(a))) == hip.EUNSUPPORTED
    before = x.clone()
    assert int(hip.lib().nfmc_dlmc_step_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k3 = _flow_mh_probe_args(run, f, pot, logq, True)
    assert int(hip.lib().nfmc_imh_parallel_supported_f32(C.byref(pa))) == hip.EUNSUPPORTED
    work = torch.zeros(64, device=dev)                                               # refused before the work area is sized
    assert int(hip.lib().nfmc_imh_parallel_f32(C.byref(pa), hip.ptr(work), work.numel() * 4, hip.stream())) == hip.EUNSUPPORTED
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK        # the register kernels take it
    pa.rng.rounds = 7                                                               # the opt-in stream: not for kind 10
    before = run.x.clone()
    assert int(hip.lib().nfmc_flow_mh_steps_f32(C.byref(pa), hip.stream())) == hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(run.x, before)
    # a wide conditioner (one-chain-per-lane / matrix-core flow-MH kernels): refused, never evaluated as a quadratic
    fw, _ = _flow_pair(d, 5, n_hidden=48)
    fw.to(dev)
    pw, _k4 = _flow_mh_probe_args(run, fw, pot, logq, True)
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pw))) == hip.EUNSUPPORTED
    # NeuTra on the matrix cores (48 units): the gradient and the trajectory entry points
    u = torch.full((n,), 123.0, device=dev)
    gr = torch.full_like(x, 123.0)
    before = x.clone()
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


def test_the_fit_step_refuses_kind_10(dev):
    """The device variational fit evaluates kinds 0 and 1 only: the sampler warmups are not offered the potential
    (fused_in('fit') is False) and nfmc_flow_variational_fit_step_f32 answers EUNSUPPORTED without touching the weights."""
    from nfmc_amd import hip
    from nfmc_amd.flow_training import DeviceFit
    from nfmc_amd.samplers.common import resolve_target
    n = 96
    p = _problem('both', 6, n)
    assert resolve_target(p.pot, (p.d,), family='fit') is None
    f, _ = _flow_pair(p.d)
    f.to(dev)
    fit = DeviceFit(f.bijection, dev, n, lr=1e-3)
    before = fit.params.clone()
    pd = p.pot.descriptor(dev)
    z = p.x0.to(dev)
    fit.opt.step = 1
    rc = int(hip.lib().nfmc_flow_variational_fit_step_f32(C.byref(fit.fit), C.byref(pd), hip.ptr(z), n, C.byref(fit.opt),
                                                            hip.stream()))
    torch.cuda.synchronize()
    assert rc == hip.EUNSUPPORTED and torch.equal(fit.params, before)


def test_philox7_and_bad_descriptors_are_refused(dev):
    """The opt-in Philox4x32-7 stream has no kind-10 kernel (and sample(..., rng_rounds=7) raises ValueError); check_vfx's
    codes at the mcmc, flow-MH and NeuTra entry points alike: a NULL a or b, C < 1, a layout code that is none of the 16
    (no varying side, mode 3, slope-only, fractional, negative, 64, NaN), a C that does not give d, and N = 0, negative,
    inf or NaN with unknown noise are EINVAL; a misaligned a is EALIGN.  Nothing is written."""
    from nfmc_amd import hip, sample
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    n = 128
    p = _problem('both', 6, n)
    d, pot = p.d, p.pot
    assert d == 17
    x = p.x0.to(dev)
    before = x.clone()
    bad = []
    for field, value, code in (('a', 0, hip.EINVAL), ('b', 0, hip.EINVAL), ('reserved', 0, hip.EINVAL),
                               ('reserved', -1, hip.EINVAL), ('reserved', 5, hip.EINVAL), ('reserved', 7, hip.EINVAL),
                               ('reserved', d + 1, hip.EINVAL), ('reserved', 2 ** 30, hip.EINVAL),
                               ('a_scalar', 5.0, hip.EINVAL),      # shared + shared: no varying side
                               ('a_scalar', 8.0, hip.EINVAL),      # no intercept side
                               ('a_scalar', 11.0, hip.EINVAL),     # mode_a = 3
                               ('a_scalar', 14.0, hip.EINVAL),     # mode_b = 3
                               ('a_scalar', 10.5, hip.EINVAL), ('a_scalar', -1.0, hip.EINVAL), ('a_scalar', 64.0 + 10.0, hip.EINVAL),
                               ('a_scalar', float('nan'), hip.EINVAL),
                               ('a_scalar', 2.0, hip.EINVAL),      # a valid code of another d (C + 3 = 9)
                               ('a_scalar', 26.0, hip.EINVAL),     # known noise: d would be 16
                               ('b_scalar', 0.0, hip.EINVAL), ('b_scalar', -3.0, hip.EINVAL),
                               ('b_scalar', float('inf'), hip.EINVAL), ('b_scalar', float('nan'), hip.EINVAL),
                               ('a', 'misaligned', hip.EALIGN)):
        q = pot.descriptor(dev)
        setattr(q, field, q.a + 4 if value == 'misaligned' else value)
        bad.append((q, code))
    ok = pot.descriptor(dev)
    ok.a_scalar = 42.0                                                               # the same shape, non-centered: well formed
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = hip.ptr(x), n, d, 2, 0.01, 1
    a.pot = pot.descriptor(dev)
    a.rng.seed, a.rng.rounds = 3, 7
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EUNSUPPORTED
    a.rng.rounds = 10
    for q, code in bad:
        a.pot = q
        assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == code, (q.reserved, q.a_scalar, q.b_scalar)
    hm = hip.NfmcHmcArgs()
    hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = hip.ptr(x), n, d, 2, 0.01, 1, 3
    hm.rng.seed = 3
    for q, code in bad:
        hm.pot = q
        assert int(hip.lib().nfmc_hmc_steps_f32(C.byref(hm), hip.stream())) == code
    f, _ = _flow_pair(d)
    f.to(dev)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k = _flow_mh_probe_args(run, f, pot, logq, True)
    st, _k2 = f.bijection.packed(dev)
    u = torch.empty(n, device=dev)
    g = torch.empty_like(x)
    for q, code in bad:
        pa.pot = q
        assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == code
        assert int(hip.lib().nfmc_neutra_potential_grad_f32(C.byref(st), C.byref(q), hip.ptr(x), n, hip.ptr(u), hip.ptr(g),
                                                              hip.stream())) == code
    pa.pot = ok
    assert int(hip.lib().nfmc_flow_mh_supported_f32(C.byref(pa))) == hip.OK
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    with pytest.raises(ValueError):
        sample(pot, flow=None, strategy='mala', n_iterations=2, n_chains=32, show_progress=False, seed=1,
               x0=x[:32].cpu(), rng_rounds=7)


def test_limits_are_unchanged(dev):
    """Kind 10 adds no shape limit of its own: nfmc_limits answers what it did for ABI version 4."""
    from nfmc_amd import hip
    lim = hip.NfmcLimits()
    assert int(hip.lib().nfmc_limits(C.byref(lim))) == hip.OK
    assert ((lim.abi_version, lim.max_d_sampler, lim.max_d_flow, lim.max_hidden_valu, lim.max_hidden, lim.max_steps_per_call)
            == (4, 1024, 512, 32, 128, hip.MAX_STEPS_PER_CALL))


# ------------------------------------------------------------------------- 11. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    from nfmc_amd.dist import Shard
    n, T = 300, 8
    p = _problem('both', 14, n)
    d = p.d
    runs = []
    for _ in range(2):
        s = _sampler(kind, p, T)
        s.seed = 7
        runs.append(s.sample(p.x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories
    dense = runs[0].samples.reshape(T, n, d)
    parts = []
    for r in range(2):
        sh = Shard(rank=r, world=2)
        sh.merge_statistics = lambda s_: s_
        s = _sampler(kind, p, T)
        s.seed, s.shard = 7, sh
        parts.append(s.sample(p.x0, show_progress=False).samples.reshape(T, -1, d))
    assert torch.equal(torch.cat(parts, 1), dense)


# ------------------------------------------------------------------------- 12. overflow
@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_starts_are_rejected_and_counted(dev, kind):
    """Centered chains with s_a = -60: e^{-2 s_a} = e^{120} overflows fp32, U(x) is inf, every log ratio is inf - inf or
    worse.  The adjusted kernels reject every proposal and count it as non-finite (n_nonfinite_log_ratios), as for the
    existing kinds; the states stay where they are, finite."""
    n, T = 256, 5
    p = _problem('both', 5, n)
    x0 = p.x0.clone()
    x0[:, p.pot.group_block + p.pot.names.index('s_a')] = -60.0
    s = _sampler(kind, p, T, L=3, h=0.01, imd=torch.ones(p.d, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.equal(out.samples.reshape(T, n, p.d)[-1], x0)
    assert st.n_accepted_trajectories == 0 and st.n_nonfinite_log_ratios == n * T


# ------------------------------------------------------------------------- 13. statistics through the public entry
SE_MULTIPLE = 6


def test_eight_schools_posterior_mean_fused_against_split(dev, monkeypatch):
    """sample(eight_schools(centered=False), strategy='jump_hmc') with 4096 chains, fused and on the split path
    (fuse='never', the object behind a plain lambda, same seed and starts): the posterior mean of mu over the final
    states.  Both runs draw the same Philox numbers, so their chains agree until a rounding difference flips a decision;
    from there two chains are, at worst, independent draws.  The difference of the two means is then bounded by that of
    two independent runs, whose standard error is sqrt(2) se with se = the split run's own between-chain standard error
    of mu, std / sqrt(4096).  SE_MULTIPLE = 6 of se is 4.2 of that standard error: a false alarm has probability about
    2e-5, and a kernel whose mu gradient or prior term were wrong would move the mean by a fraction of the posterior
    standard deviation = 64 se."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import VaryingEffectsRegression
    from nfmc_amd.samplers import jump
    pot = VaryingEffectsRegression.eight_schools(centered=False)
    n, d = 4096, 10
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(n, d, generator=g)
    x0[:, 8] = 4.0 + 3.0 * x0[:, 8]
    x0[:, 9] = 1.0 + 0.5 * x0[:, 9]
    means, ses, splits = [], [], []
    for target, fuse in ((pot, 'auto'), (lambda x: pot(x), 'never')):
        spy = _Spy(monkeypatch)
        out = sample(target, event_shape=(d,), flow='realnvp', strategy='jump_hmc', n_iterations=8, n_chains=n, x0=x0,
                     show_progress=False, seed=17, fuse=fuse,
                     inner_kernel_kwargs={'step_size': 0.25, 'n_leapfrog_steps': 5}, inner_param_kwargs={'n_iterations': 5})
        splits.append(len(spy.calls))
        x = out.running_samples.last_sample.cpu().double().reshape(n, d)
        assert bool(torch.isfinite(x).all())
        mu = pot.unpack(x)['mu_a']
        means.append(float(mu.mean()))
        ses.append(float(mu.std() / math.sqrt(n)))
    assert splits[0] == 0 and splits[1] > 0                      # the first run fused, the second on the split path
    print('posterior mean of mu: fused %.4f, split %.4f, split se %.4f' % (means[0], means[1], ses[1]))
    assert abs(means[0] - means[1]) <= SE_MULTIPLE * ses[1], (means, ses)
    assert 0.0 < means[1] < 9.0                                  # the textbook posterior mean of mu is about 4.4
