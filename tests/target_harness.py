"""What the per-target GPU test files (tests/test_gpu_<target>.py) and tests/test_gpu_warmup.py share: the comparisons
against the fp64 oracle, the spies and recorders around the fused launches, the flow and sampler builders, the sequence
of calls every refusing C entry point gets, and the bodies of the tests that differ between targets in the problem
alone.  A plain module, imported like tests/spline_fixtures.py; the fixtures stay in the test files.

The numbers of a check that differ between the files, or could (margins, tolerances, shares, slacks, seeds, counts),
are arguments without a default: each test file states its own.  Where the files differ in behaviour the difference is
an argument whose default is the stricter behaviour.  tests/test_host_target_harness.py checks on the CPU that the
comparisons here do fail when they should.

A problem is a `Problem`: the package potential, its fp64 restatement `ref` (U alone, for magnitudes and NeuTra), the
fp64 target the oracle samplers run on, the fp32 starts x0 (n, d), d and a name for messages.  The `_Problem` classes of
the newer files have the same attributes and are passed as they are."""
import collections
import ctypes as C
import math

import numpy as np
import pytest
import torch

Problem = collections.namedtuple('Problem', 'pot ref target x0 d name')

KINDS = ('mala', 'ula', 'mh', 'hmc', 'uhmc')
ORACLE_KIND = {'mala': 'langevin', 'ula': 'langevin', 'mh': 'mh', 'hmc': 'hmc', 'uhmc': 'hmc'}
KAPPA = 8.0        # oracle/shadow.py's tolerance multiple (tests/test_gpu_benchmarked_workloads.py)


# --------------------------------------------------------------------------------------------- comparisons
def compare_states(got, tr, what, *, margin, atol, rtol, cap=0.10):
    """got (T, n, d) fp32 from the kernels, tr an oracle Trace on the same noise.  Tie-aware: a chain whose fp64
    |log u - log ratio| falls under `margin` at any of its transitions is excluded; the excluded share must stay under
    `cap`, all other chains must match to atol + rtol |want|.  Returns the mask of the chains kept."""
    want = tr.stacked().float()
    n = want.shape[1]
    keep = torch.ones(n, dtype=torch.bool)
    if tr.log_ratios:
        lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
        lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
        keep = ((lu - lr).abs() >= margin).all(0)
    excluded = 1.0 - float(keep.float().mean())
    print('%s: %.1f %% of the chains excluded as near-ties' % (what, 100 * excluded))
    assert excluded < cap, (what, excluded)
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got[:, keep].numpy(), want[:, keep].numpy(), atol=atol, rtol=rtol, err_msg=what)
    return keep


def compare_decisions(rec, tr, kind, x0, ref, what, *, mag=None, skip_below_minus_50=False):
    """The kernel's accept masks and log ratios (rec.stacked()) against the oracle's, transition by transition, on the
    rows before a chain's first disagreeing decision (a near-tie flips it; the states comparison bounds how many).  Log
    ratios to 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) mag(x), x the state each transition starts from:
    `mag(x)`, |U(x)| = |ref(x)| unless given, is the size of the fp32 numbers U(x) and U(x') whose difference the kernel
    forms, which cannot be closer than a few of their ulps.

    skip_below_minus_50: a proposal whose U overflows, or whose HMC trajectory diverges, has a non-finite or hugely
    negative fp64 log ratio (below -50 no uniform can accept it); the masks already show that the kernel rejected it,
    and the fp32 and fp64 trajectories part there, so only finite ratios above -50 are compared.  Off unless a target
    has such proposals at its test inputs: every agreeing row is compared, and a non-finite fp64 ratio fails."""
    got_m, got_lr = rec.stacked()
    if kind in ('ula', 'uhmc'):
        assert bool(got_m.all()), what                        # unadjusted: every proposal kept
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
    prev = torch.cat([x0.double()[None], states[:-1].double()]).reshape(-1, d)   # the state each transition starts from
    size = (ref(prev).abs() if mag is None else mag(prev)).reshape(states.shape[:2])
    if skip_below_minus_50:
        agree = agree & torch.isfinite(want_lr) & (want_lr > -50)
    err = (got_lr.double() - want_lr).abs()
    tol = 2e-4 * max(1.0, d / 64) + 1e-4 * want_lr.abs() + 8 * 2.0 ** -24 * size
    print('%s: worst log-ratio error %.2e' % (what, float(err[agree].max())))
    assert bool((err[agree] <= tol[agree]).all()), (what, float(err[agree].max()))


# ------------------------------------------------------------------------------------- spies and recorders
class Spy:
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


class Record:
    """Hands every fused mcmc launch of `sampler` a mask buffer and, with log_ratios, a log-ratio buffer, and keeps
    them: the kernel's accept decisions and log ratios, stacked over the launches as (T, n).  Without log_ratios the
    launch is handed no log-ratio buffer (it then has one output fewer): the form the warmup checks use."""

    def __init__(self, monkeypatch, sampler, log_ratios=True):
        self.masks, self.log_ratios = [], []
        cls = type(sampler)
        orig = cls._launch

        def launch(s, run, pot, k, step0, samples, masks_out=None, log_ratio_out=None, **kw):
            if masks_out is None:
                masks_out = torch.zeros(k, run.n, dtype=torch.uint8, device=run.dev)
            self.masks.append(masks_out)
            if log_ratios:
                if log_ratio_out is None:
                    log_ratio_out = torch.zeros(k, run.n, dtype=torch.float32, device=run.dev)
                self.log_ratios.append(log_ratio_out)
            return orig(s, run, pot, k, step0, samples, masks_out=masks_out, log_ratio_out=log_ratio_out, **kw)
        monkeypatch.setattr(cls, '_launch', launch)

    def stacked(self):
        return torch.cat(self.masks).cpu().bool(), torch.cat(self.log_ratios).cpu()

    def accepted(self):
        return torch.cat(self.masks).cpu().long().sum(1)


# --------------------------------------------------------------------------------------------- builders
def flow_pair(d, seed=5, n_hidden=None, spline=False):
    """(package flow, fp64 oracle flow) with the same perturbed weights (oracle.flow.perturb_, every parameter touched)"""
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


def mcmc_sampler(kind, event_shape, target, T, h, L=5, imd=None, *, imd_kinds):
    """The package sampler of `kind` on `event_shape` (an int d stands for (d,)).  `imd_kinds`: the kinds whose kernel
    is given the mass diagonal `imd`; the others, and every kind when imd is None, keep the kernel's unit diagonal."""
    from nfmc_amd.samplers import mcmc
    shape = (event_shape,) if isinstance(event_shape, int) else tuple(event_shape)
    d = int(math.prod(shape))
    kw = {'inv_mass_diag': imd.float()} if imd is not None and kind in imd_kinds else {}
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        return cls(shape, target, mcmc.LangevinKernel(event_size=d, step_size=h, **kw), mcmc.LangevinParameters(n_iterations=T))
    if kind == 'mh':
        return mcmc.MH(shape, target, mcmc.MHKernel(event_size=d, **kw), mcmc.MHParameters(n_iterations=T))
    cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
    return cls(shape, target, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h, **kw),
               mcmc.HMCParameters(n_iterations=T))


def oracle_trace(kind, x0, target, T, h, noise, L=5, imd=None, *, imd_kinds, label=None):
    """oracle.samplers.mcmc_sample for `kind` from x0 in fp64, the mass diagonal going to the kinds of `imd_kinds` (as in
    mcmc_sampler).  With a label, prints the acceptance of an adjusted kind."""
    from oracle import samplers as osamp
    tr = osamp.mcmc_sample(x0.double(), target, ORACLE_KIND[kind], T, h, n_leapfrog=L, adjustment=kind not in ('ula', 'uhmc'),
                           noise=noise, inv_mass_diag=imd if kind in imd_kinds else None)
    if label is not None and kind in ('mala', 'mh', 'hmc'):
        print('%s: oracle acceptance %.3f' % (label, tr.n_accepted / (x0.shape[0] * T)))
    return tr


def neutra_hmc_sampler(d, pot, f, T, L, h):
    from nfmc_amd.samplers import mcmc, neutra
    return neutra.NeuTraHMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h),
                            mcmc.HMCParameters(), neutra.NeuTraKernel((d,), flow=f), neutra.NeuTraParameters(n_iterations=T))


def imh_run(monkeypatch, pot, d, f, x0, T, seed):
    """T FixedIMH transitions, every one on the sequential flow-MH kernel: neither nfmc_imh_parallel_f32 nor the
    composed step"""
    from nfmc_amd.samplers import imh
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=T))
    s.seed = seed
    calls = {'launch_imh_parallel': 0, 'launch_flow_mh': 0, 'split_flow_mh': 0}

    def spy(name):   # the names imh.py calls (bound there by its `from .jump import ...`)
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


def neutra_grad(dev, f, pot, z):
    """(return code, U~ (n,), grad U~ (n, d)) of nfmc_neutra_potential_grad_f32 at the latents z"""
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


# ------------------------------------------------------------------------ the device warmup's fp64 replay
def warmup_sampler(kind, d, pot, W, T, h, L=4, beta=1e-3, every=1, imd=None):
    from nfmc_amd.samplers import mcmc
    kw = dict(n_iterations=T, n_warmup_iterations=W, imd_adjustment=beta, tune_every=every)
    if kind in ('mala', 'ula'):
        cls = mcmc.MALA if kind == 'mala' else mcmc.ULA
        s = cls((d,), pot, mcmc.LangevinKernel(event_size=d, step_size=h), mcmc.LangevinParameters(**kw))
    elif kind == 'mh':
        s = mcmc.MH((d,), pot, mcmc.MHKernel(event_size=d, inv_mass_diag=imd), mcmc.MHParameters(**kw))
    else:
        cls = mcmc.HMC if kind == 'hmc' else mcmc.UHMC
        s = cls((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h), mcmc.HMCParameters(**kw))
    return s


def controller_params(s, h0, imd0):
    from oracle import samplers as osamp
    p = s.params
    return osamp.ControllerParams(step_size=h0, inv_mass_diag=imd0.clone(), imd_adjustment=p.imd_adjustment,
                                  tune_step_size=bool(p.tune_step_size and p.adjustment),
                                  tune_inv_mass_diag=bool(p.tune_inv_mass_diag))


def check_controller(s, ups, what):
    """step size and dual-averaging state to 1e-10 relative (integer accept counts: only fp64 reassociation separates
    them), inv_mass_diag to a few fp32 ulps (fp32 partial sums of the shifted states), iteration exact"""
    last = ups[-1]
    np.testing.assert_allclose(s.kernel.step_size, last.step_size, rtol=1e-10, err_msg=what)
    if s.params.tune_step_size and s.params.adjustment:
        np.testing.assert_allclose(s.kernel.da.error_sum, last.error_sum, rtol=1e-10, atol=1e-10, err_msg=what)
        np.testing.assert_allclose(s.kernel.da.log_smooth, last.log_smooth, rtol=1e-10, atol=1e-12, err_msg=what)
        assert s.kernel.da.iteration == last.iteration, what
    got, want = s.kernel.inv_mass_diag.double(), last.inv_mass_diag.double()
    assert torch.isfinite(got).all() and (got > 0).all(), what
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=4e-6 * len(ups) ** 0.5, atol=0, err_msg=what)


def shadow(states, kind, target, h, imd, seed, step0, L, what, max_tie_share=0.01):
    from oracle import shadow as oshadow
    wl = oshadow.Workload(kind, target, step_size=h, n_leapfrog=L, inv_mass_diag=imd, step0=step0)
    rep = oshadow.shadow(states, wl, seed)
    fails = rep.failures(KAPPA, max_tie_share)
    assert not fails, (what, fails, rep.summary())


def warmup_matches_controller(monkeypatch, p, kind, *, W, T, L, every, h0, imd0, seed, what, ties, record_log_ratios=False):
    """The controller state after the device warmup against oracle.samplers.replay_controller over the kernel's own kept
    states and accept counts; every warmup transition shadowed in fp64 with the step size and mass diagonal the replay
    says it ran with (warmup stream: hip.WARMUP_STEP0), and the sampling run that follows shadowed with the tuned
    (non-unit) mass diagonal.  `ties`: the share of near-ties the shadows allow.  MH takes imd0 as its proposal scale."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    d, n = p.d, p.x0.shape[0]
    s = warmup_sampler(kind, d, p.pot, W, T, h0, L=L, every=every, imd=imd0.clone() if kind == 'mh' else None)
    h0 = float(s.kernel.step_size)      # MH keeps its kernel's own (untuned, unused) step size
    s.seed = seed
    rec = Record(monkeypatch, s, log_ratios=record_log_ratios)
    wout = s.warmup(p.x0, show_progress=False)
    states = wout.samples.reshape(W, n, d)
    ups, h_t, imd_t = osamp.replay_controller(states, rec.accepted(), every, controller_params(s, h0, imd0))
    assert len(ups) == math.ceil(W / every)
    check_controller(s, ups, what)
    shadow(torch.cat([p.x0[None], states]), kind, p.target, h_t, imd_t, seed, hip.WARMUP_STEP0, L, what + ' warmup', ties)
    x1 = wout.running_samples.last_sample.cpu()
    out = s.sample(x1, show_progress=False)
    assert torch.isfinite(out.samples).all()
    shadow(torch.cat([x1[None], out.samples.reshape(T, n, d)]), kind, p.target, s.kernel.step_size,
           s.kernel.inv_mass_diag.clone(), seed, 0, L, what + ' sampling', ties)


# ------------------------------------------------------------- test bodies shared in all but the problem
def replay_run(monkeypatch, s, oracle, x0, torch_seed, record):
    """The oracle on recorded torch noise (oracle(noise) -> Trace, after torch.manual_seed(torch_seed)), then the package
    sampler `s` from x0 on the same noise, replayed: (sampler output, oracle trace, kernel Record or None, Spy)."""
    from oracle import samplers as osamp
    rec = osamp.RecordingNoise(osamp.TorchNoise())
    torch.manual_seed(torch_seed)
    tr = oracle(rec)
    s.replay = (torch.stack([v.float() for v in rec.normals]),
                torch.stack([v.float() for v in rec.uniforms]) if rec.uniforms else None)
    spy = Spy(monkeypatch)
    rec_k = Record(monkeypatch, s) if record else None
    out = s.sample(x0, show_progress=False)
    return out, tr, rec_k, spy


def _shape(p, event_shape):
    return (p.d,) if event_shape is None else tuple(event_shape)


def replay_matches_oracle(monkeypatch, p, kind, T, s, oracle, *, torch_seed, what, compare, decisions, event_shape=None):
    """T fused transitions of `s` on the oracle's replayed noise: states by `compare`, and, unless `decisions` is None,
    the kernel's masks and log ratios by it."""
    from nfmc_amd.samplers import mcmc
    shape, n = _shape(p, event_shape), p.x0.shape[0]
    assert mcmc.resolve_target(p.pot, shape, family='mcmc') is p.pot
    out, tr, rec_k, spy = replay_run(monkeypatch, s, oracle, p.x0.reshape((n,) + shape), torch_seed, decisions is not None)
    assert not spy.calls                                       # every transition on the fused kernel
    compare(out.samples.reshape(T, n, p.d), tr, what)
    if decisions is not None:
        decisions(rec_k, tr, kind, p.x0, p.ref, what)


def native_matches_oracle(monkeypatch, p, kind, T, s, oracle, *, seed, what, compare, decisions, event_shape=None):
    """As replay_matches_oracle on the native Philox stream of `seed`: the oracle draws the same numbers in fp64."""
    from nfmc_amd.samplers import mcmc
    from oracle import samplers as osamp
    shape, n = _shape(p, event_shape), p.x0.shape[0]
    assert mcmc.resolve_target(p.pot, shape, family='mcmc') is p.pot
    s.seed = seed
    spy = Spy(monkeypatch)
    rec_k = Record(monkeypatch, s) if decisions is not None else None
    out = s.sample(p.x0.reshape((n,) + shape), show_progress=False)
    assert not spy.calls
    tr = oracle(osamp.PhiloxNoise(seed, dtype=torch.float64))
    compare(out.samples.reshape(T, n, p.d), tr, what)
    if decisions is not None:
        decisions(rec_k, tr, kind, p.x0, p.ref, what)


def jump_mala_matches_oracle(monkeypatch, p, *, T, Kin, seed, h, imd, fuse_tail, spline, atol, rtol, share, jump_slack):
    """jump_mala on a fixed perturbed flow, native stream: inner MALA fused, the jump on the register flow-MH kernel or,
    with fuse_tail, as the tail of the last inner launch (affine flows only).  imd None: the inner kernel is the
    sampler's default one with its step size set to h; else LangevinKernel(step_size=h, inv_mass_diag=imd).  A share of
    the chains must follow the oracle through all T (Kin + 1) transitions, and the accepted jumps agree to jump_slack."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, d = p.x0.shape[0], p.d
    f, of = flow_pair(d, spline=spline)
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = Spy(monkeypatch)
    inner = None if imd is None else mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd)
    s = jump.JumpMALA((d,), p.pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), inner,
                      mcmc.LangevinParameters(n_iterations=Kin))
    if imd is None:
        s.inner_sampler.kernel.step_size = h
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    out = s.sample(p.x0, show_progress=False)
    assert not spy.calls and not split                        # inner loop and jump fused
    if not fuse_tail or spline:
        assert len(flow_mh) == T                              # each jump on the flow-MH kernel (the tail is affine only)
    tr = osamp.jump_sample(p.x0.double(), p.target, of, 'langevin', T, Kin, h,
                           inv_mass_diag=None if imd is None else imd.double(),
                           noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < atol + rtol * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > share, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= jump_slack


def imh_matches_oracle(monkeypatch, p, *, T, seed, flow_seed, spline, what, compare):
    """FixedIMH on the register flow-MH kernel (affine, or the 'c-rqnsf' spline instantiation) against imh_sample"""
    from oracle import samplers as osamp
    n, d = p.x0.shape[0], p.d
    f, of = flow_pair(d, flow_seed, spline=spline)
    out = imh_run(monkeypatch, p.pot, d, f, p.x0, T, seed)
    tr = osamp.imh_sample(p.x0.double(), p.target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    compare(out.samples.reshape(T, n, d), tr, what)


def fused_equals_split(monkeypatch, p, make, T, *, seed, atol, rtol, share):
    """make(target) -> sampler.  The potential object runs fused, the same object behind a plain lambda takes the split
    path for all T transitions (fuse='never'); a share of the chains agrees to atol, and those to atol + rtol."""
    n, d = p.x0.shape[0], p.d
    outs, counts = [], []
    for target, fuse in ((p.pot, 'auto'), (lambda x: p.pot(x), 'never')):
        spy = Spy(monkeypatch)
        s = make(target)
        s.seed, s.fuse = seed, fuse
        outs.append(s.sample(p.x0, show_progress=False))
        counts.append(len(spy.calls))
    assert counts == [0, T]
    a, b = (o.samples.reshape(T, n, d) for o in outs)
    same = (a - b).abs().amax(dim=(0, 2)) < atol
    assert same.float().mean() > share, float(same.float().mean())
    np.testing.assert_allclose(a[:, same].numpy(), b[:, same].numpy(), atol=atol, rtol=rtol)


def neutra_gradient_matches_autograd(dev, pot, ref, z, nh, label, *, flow_seed, bound):
    """U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)| and its gradient from the VALU NeuTra kernel against fp64 autograd
    through oracle/flow.py and `ref`, on a perturbed RealNVP of nh hidden units.  Tolerance: `bound` relative to
    1 + max |U~| over the rows, and per row relative to 1 + the row's largest gradient entry."""
    from nfmc_amd import hip
    from oracle import samplers as osamp
    d = z.shape[1]
    f, of = flow_pair(d, flow_seed, n_hidden=nh)
    z = z.double().requires_grad_(True)
    u_ref = osamp.neutra_adjusted_target(of, ref, (d,))(z)
    g_ref, = torch.autograd.grad(u_ref.sum(), z)
    rc, u, g = neutra_grad(dev, f, pot, z.detach())
    assert rc == hip.OK
    ur = u_ref.detach()
    np.testing.assert_allclose(u.numpy(), ur.numpy(), atol=bound * (1 + float(ur.abs().max())), rtol=0)
    err = (g.double() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1))
    print('%s: worst relative gradient error %.2e' % (label, float(err.max())))
    assert float(err.max()) < bound


def _follows_neutra_oracle(out, p, of, *, T, L, h, seed, atol, share):
    from oracle import samplers as osamp
    n, d = p.x0.shape[0], p.d
    tr = osamp.neutra_hmc_sample(p.x0.double(), p.target, of, T, h, None, L, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got, want = out.samples.reshape(T, n, d), tr.stacked().float()
    same = (got - want).abs().amax(dim=(0, 2)) < atol
    assert same.float().mean() > share, float(same.float().mean())
    return tr


def neutra_hmc_fused_matches_oracle(monkeypatch, p, flows, *, T, L, h, seed, atol, share, accept_slack):
    """Fused NeuTra HMC (nfmc_neutra_hmc_steps_f32, VALU kernel, never the inner sampler's split path) from the latents
    p.x0 against neutra_hmc_sample on the native stream; flows = (package flow, fp64 oracle flow)."""
    f, of = flows
    s = neutra_hmc_sampler(p.d, p.pot, f, T, L, h)
    assert s._closed_form() is p.pot and s._min_hidden() == 0
    split = []
    monkeypatch.setattr(s.inner_sampler, 'sample', lambda *a, **k: split.append(1))
    s.seed = seed
    out = s.sample(p.x0, show_progress=False)
    assert not split
    tr = _follows_neutra_oracle(out, p, of, T=T, L=L, h=h, seed=seed, atol=atol, share=share)
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= accept_slack


def neutra_wide_takes_the_split_path(dev, p, flows, *, T, L, h, seed, atol, share):
    """A conditioner wide enough for the matrix cores, which evaluate kinds 0 and 1 only: the gradient entry point
    answers EUNSUPPORTED, the run takes the inner sampler's split path (autograd through the flow) once and still
    follows the oracle.  Returns the sampler."""
    from nfmc_amd import hip
    f, of = flows
    rc, _u, _g = neutra_grad(dev, f, p.pot, p.x0)
    assert rc == hip.EUNSUPPORTED
    s = neutra_hmc_sampler(p.d, p.pot, f, T, L, h)
    split = []
    orig = s.inner_sampler.sample
    s.inner_sampler.sample = lambda *a, **k: split.append(1) or orig(*a, **k)
    s.seed = seed
    out = s.sample(p.x0, show_progress=False)
    assert split == [1]
    _follows_neutra_oracle(out, p, of, T=T, L=L, h=h, seed=seed, atol=atol, share=share)
    return s


def determinism_and_sharding(make, x0, T, d, *, seed, world):
    """make() -> sampler.  Two identical runs agree bitwise, and rank r of a world-way split equals its slice of the
    single-process run.  Returns the dense run's states (T, n, d)."""
    from nfmc_amd.dist import Shard
    n = x0.shape[0]
    runs = []
    for _ in range(2):
        s = make()
        s.seed = seed
        runs.append(s.sample(x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories
    dense = runs[0].samples.reshape(T, n, d)
    at = 0
    for r in range(world):
        sh = Shard(rank=r, world=world)
        sh.merge_statistics = lambda s_: s_
        s = make()
        s.seed, s.shard = seed, sh
        part = s.sample(x0, show_progress=False).samples.reshape(T, -1, d)
        assert torch.equal(part, dense[:, at:at + part.shape[1]]), r
        at += part.shape[1]
    assert at == n
    return dense


# ------------------------------------------------------------------------ the refusing C entry points
def _rc(fn, *args):
    return int(fn(*args))


def refusing_entry_points(dev, pot, x0, make_flow, *, neutra_fused=True):
    """Every entry point that has no kernel for this potential kind answers NFMC_EUNSUPPORTED before it launches
    anything, and writes nothing: dlmc's fused gradient step, imh_parallel, the flow-MH kernels on the opt-in Philox-7
    stream and with a conditioner too wide for the register kernels (fw), NeuTra on the matrix cores (fw), and, for a
    kind without NeuTra kernels at all (neutra_fused False), NeuTra with the narrow flow f.  The register flow-MH
    kernels take the kind with f.  make_flow(seed=5, n_hidden=None) -> (package flow, oracle flow): f = make_flow(), fw
    = make_flow(5, n_hidden=48).  Returns the flow-MH probe arguments of f (default stream) and what keeps them alive."""
    from nfmc_amd import hip
    from nfmc_amd.samplers import dlmc, imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    lib, U = hip.lib(), hip.EUNSUPPORTED
    n, d = x0.shape
    x = x0.to(dev)
    start = x.clone()
    f, _ = make_flow()
    f.to(dev)
    pd = pot.descriptor(dev)
    a, _keep = dlmc.step_args(f, x, 0.05, pot=pot)
    assert _rc(lib.nfmc_dlmc_step_supported_f32, C.byref(a)) == U
    assert _rc(lib.nfmc_dlmc_step_f32, C.byref(a), hip.stream()) == U
    u = torch.full((n,), 123.0, device=dev)
    gr = torch.full_like(x, 123.0)
    if not neutra_fused:
        st, _k2 = f.bijection.packed(dev)
        assert _rc(lib.nfmc_neutra_potential_grad_f32, C.byref(st), C.byref(pd), hip.ptr(x), n, hip.ptr(u), hip.ptr(gr),
                   hip.stream()) == U
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())                                                           # the probe arguments' own state
    logq = torch.empty(n, device=dev)
    pa, _k3 = _flow_mh_probe_args(run, f, pot, logq, True)
    assert _rc(lib.nfmc_imh_parallel_supported_f32, C.byref(pa)) == U
    work = torch.zeros(64, device=dev)                                              # refused before the work area is sized
    assert _rc(lib.nfmc_imh_parallel_f32, C.byref(pa), hip.ptr(work), work.numel() * 4, hip.stream()) == U
    assert _rc(lib.nfmc_flow_mh_supported_f32, C.byref(pa)) == hip.OK               # the register kernels take it
    rounds = pa.rng.rounds
    pa.rng.rounds = 7                                                               # the opt-in stream: not for this kind
    before = run.x.clone()
    assert _rc(lib.nfmc_flow_mh_steps_f32, C.byref(pa), hip.stream()) == U
    torch.cuda.synchronize()
    assert torch.equal(run.x, before)
    pa.rng.rounds = rounds
    # a wide conditioner (one-chain-per-lane / matrix-core flow-MH kernels): refused, never evaluated as a quadratic
    fw, _ = make_flow(5, n_hidden=48)
    fw.to(dev)
    pw, _k4 = _flow_mh_probe_args(run, fw, pot, logq, True)
    assert _rc(lib.nfmc_flow_mh_supported_f32, C.byref(pw)) == U
    pw.x, pw.logq, pw.n_steps = hip.ptr(x), hip.ptr(logq), 1
    assert _rc(lib.nfmc_flow_mh_steps_f32, C.byref(pw), hip.stream()) == U
    # NeuTra on the matrix cores: the gradient and the trajectory entry points
    stw, _k5 = fw.bijection.packed(dev)
    assert _rc(lib.nfmc_neutra_potential_grad_f32, C.byref(stw), C.byref(pd), hip.ptr(x), n, hip.ptr(u), hip.ptr(gr),
               hip.stream()) == U
    na = hip.NfmcNeutraHmcArgs()
    na.z, na.n, na.n_steps, na.n_leapfrog, na.step_size, na.adjust = hip.ptr(x), n, 1, 2, 0.01, 1
    na.flow, na.pot = stw, pd
    na.rng.seed = 3
    assert _rc(lib.nfmc_neutra_hmc_steps_f32, C.byref(na), hip.stream()) == U
    torch.cuda.synchronize()
    assert torch.equal(x, start) and bool((u == 123.0).all()) and bool((gr == 123.0).all())
    # the device variational fit, imh_parallel and dlmc's step are never handed the descriptor
    assert not pot.fused_in('fit') and not pot.fused_in('imh_parallel') and not pot.fused_in('dlmc_step')
    assert pot.fused_in('neutra') == neutra_fused
    return pa, (run, logq, _k3)


def fit_step_refuses(dev, pot, x0, f):
    """The device variational fit evaluates kinds 0 and 1 only: the sampler warmups are not offered the potential
    (fused_in('fit') is False) and nfmc_flow_variational_fit_step_f32 answers EUNSUPPORTED without touching the weights."""
    from nfmc_amd import hip
    from nfmc_amd.flow_training import DeviceFit
    from nfmc_amd.samplers.common import resolve_target
    n, d = x0.shape
    assert resolve_target(pot, (d,), family='fit') is None
    f.to(dev)
    fit = DeviceFit(f.bijection, dev, n, lr=1e-3)
    before = fit.params.clone()
    pd = pot.descriptor(dev)
    z = x0.to(dev)
    fit.opt.step = 1
    rc = int(hip.lib().nfmc_flow_variational_fit_step_f32(C.byref(fit.fit), C.byref(pd), hip.ptr(z), n, C.byref(fit.opt),
                                                            hip.stream()))
    torch.cuda.synchronize()
    assert rc == hip.EUNSUPPORTED and torch.equal(fit.params, before)


def mala_args(dev, pot, x):
    """NfmcMalaArgs for two adjusted transitions of the device states x (n, d) on the default stream, seed 3"""
    from nfmc_amd import hip
    a = hip.NfmcMalaArgs()
    a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = hip.ptr(x), x.shape[0], x.shape[1], 2, 0.01, 1
    a.pot = pot.descriptor(dev)
    a.rng.seed, a.rng.rounds = 3, 10
    return a


def bad_descriptors_are_refused(dev, pot, x0, f, bad, ok=(), *, event_shape=None):
    """The opt-in Philox4x32-7 stream has no kernel for this kind (nfmc_mala_steps_f32 answers EUNSUPPORTED, and
    sample(..., rng_rounds=7) raises ValueError), and every malformed descriptor of `bad` gets its code at the mcmc,
    flow-MH and NeuTra entry points alike.  bad: (field, value, code), the descriptor of `pot` with `field` set to
    `value`, 'misaligned' standing for a + 4 bytes; ok: (field, value) of descriptors that are well formed, which the
    flow-MH probe accepts.  Nothing is written."""
    from nfmc_amd import hip, sample
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    lib = hip.lib()
    n, d = x0.shape
    x = x0.to(dev)
    before = x.clone()

    def changed(field, value):
        q = pot.descriptor(dev)
        setattr(q, field, q.a + 4 if value == 'misaligned' else value)
        return q
    bad = [(changed(field, value), code, (field, value)) for field, value, code in bad]
    a = mala_args(dev, pot, x)
    a.rng.rounds = 7
    assert _rc(lib.nfmc_mala_steps_f32, C.byref(a), hip.stream()) == hip.EUNSUPPORTED
    a.rng.rounds = 10
    for q, code, which in bad:
        a.pot = q
        assert _rc(lib.nfmc_mala_steps_f32, C.byref(a), hip.stream()) == code, which
    hm = hip.NfmcHmcArgs()
    hm.x, hm.n, hm.d, hm.n_steps, hm.step_size, hm.adjust, hm.n_leapfrog = hip.ptr(x), n, d, 2, 0.01, 1, 3
    hm.rng.seed = 3
    for q, code, which in bad:
        hm.pot = q
        assert _rc(lib.nfmc_hmc_steps_f32, C.byref(hm), hip.stream()) == code, which
    f.to(dev)
    s = imh.FixedIMH((d,), pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, x.cpu())
    logq = torch.empty(n, device=dev)
    pa, _k = _flow_mh_probe_args(run, f, pot, logq, True)
    st, _k2 = f.bijection.packed(dev)
    u = torch.empty(n, device=dev)
    g = torch.empty_like(x)
    for q, code, which in bad:
        pa.pot = q
        assert _rc(lib.nfmc_flow_mh_supported_f32, C.byref(pa)) == code, which
        assert _rc(lib.nfmc_neutra_potential_grad_f32, C.byref(st), C.byref(q), hip.ptr(x), n, hip.ptr(u), hip.ptr(g),
                   hip.stream()) == code, which
    for field, value in ok:
        pa.pot = changed(field, value)
        assert _rc(lib.nfmc_flow_mh_supported_f32, C.byref(pa)) == hip.OK, (field, value)
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    shape = (d,) if event_shape is None else tuple(event_shape)
    with pytest.raises(ValueError):
        sample(pot, flow=None, strategy='mala', n_iterations=2, n_chains=32, show_progress=False, seed=1,
               x0=x[:32].cpu().reshape((32,) + shape), rng_rounds=7)


def limits_are_unchanged():
    """The potential kinds add no shape limit of their own: nfmc_limits answers what it did for ABI version 4."""
    from nfmc_amd import hip
    lim = hip.NfmcLimits()
    assert int(hip.lib().nfmc_limits(C.byref(lim))) == hip.OK
    assert ((lim.abi_version, lim.max_d_sampler, lim.max_d_flow, lim.max_hidden_valu, lim.max_hidden, lim.max_steps_per_call)
            == (4, 1024, 512, 32, 128, hip.MAX_STEPS_PER_CALL))
