"""What the per-target GPU test files (tests/test_gpu_<target>.py) and tests/test_gpu_warmup.py share: the comparisons
against the fp64 oracle, the spies and recorders around the fused launches, the flow and sampler builders, the sequence
of calls every refusing C entry point gets, and the bodies of the tests that differ between targets in the problem
alone.  A plain module, imported like tests/spline_fixtures.py; the fixtures stay in the test files.

The numbers of a check that differ between the files, or could (margins, tolerances, shares, slacks, seeds, counts),
are arguments without a default: each test file states its own.  Where the files differ in behaviour the difference is
an argument whose default is the stricter behaviour.  tests/test_host_target_harness.py checks on the CPU that the
comparisons here do fail when they should.

The flow-proposal Metropolis step (flow_mh_b_kernel, and the jump tail of mala_kernel / hmc_kernel) is compared row by
row: FlowRecord hands every launch a mask and a log-ratio buffer, compare_flow_mh holds them against the oracle's
JumpSteps, centred_flow_pair and centred give inputs under which proposals are accepted, and flow_cases is the matrix of
layouts, widths and couplings that a per-target file runs through run_flow_case.  Every figure about those inputs comes
from the fp64 (or fp32) oracle on the CPU: oracle_only and probe_flow_inputs run the cases' inputs without a GPU.
tests/test_gpu_flow_mh_wide.py holds the three kernels of wider conditioners the same way: flow_mh_kernel_of says which
kernel a launch takes, and _direct_flow_mh's options (cached log q, replayed noise, statistics, a thinned store) reach
what one nfmc_flow_mh_steps_f32 launch can be asked.  tests/test_gpu_neutra_hmc_wide.py does the same for the two
matrix-core NeuTra-HMC trajectory kernels: neutra_hmc_kernel_of and neutra_hmc_scratch_bytes name the kernel of a launch,
_direct_neutra_hmc makes one nfmc_neutra_hmc_steps_f32 call, neutra_hmc_figures measures what the oracle itself loses in
fp32, and compare_neutra_hmc holds a launch to the oracle through compare_states and compare_decisions.

A problem is a `Problem`: the package potential, its fp64 restatement `ref` (U alone, for magnitudes and NeuTra), the
fp64 target the oracle samplers run on, the fp32 starts x0 (n, d), d and a name for messages.  The `_Problem` classes of
the newer files have the same attributes and are passed as they are."""
import collections
import contextlib
import copy
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


def compare_decisions(rec, tr, kind, x0, ref, what, *, mag=None, skip_below_minus_50=False, at_least=None):
    """The kernel's accept masks and log ratios (rec.stacked()) against the oracle's, transition by transition, on the
    rows before a chain's first disagreeing decision (a near-tie flips it; the states comparison bounds how many).  Log
    ratios to 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) mag(x), x the state each transition starts from:
    `mag(x)`, |U(x)| = |ref(x)| unless given, is the size of the fp32 numbers U(x) and U(x') whose difference the kernel
    forms, which cannot be closer than a few of their ulps.

    skip_below_minus_50: a proposal whose U overflows, or whose HMC trajectory diverges, has a non-finite or hugely
    negative fp64 log ratio (below -50 no uniform can accept it); the masks already show that the kernel rejected it,
    and the fp32 and fp64 trajectories part there, so only finite ratios above -50 are compared.  Off unless a target
    has such proposals at its test inputs: every agreeing row is compared, and a non-finite fp64 ratio fails.

    at_least: a measured figure (tests/test_gpu_neutra_hmc_wide.py: four times what the fp32 oracle itself differs from
    the fp64 one by) that the tolerance of a row is raised to where the formula gives less.  Returns the worst error over
    tolerance of an adjusted kind."""
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
    if at_least is not None:
        tol = tol.clamp_min(at_least)
    print('%s: worst log-ratio error %.2e' % (what, float(err[agree].max())))
    assert bool((err[agree] <= tol[agree]).all()), (what, float(err[agree].max()))
    return float((err / tol)[agree].max())


def affine_c(d):
    """the unexplained part of a flow-MH log ratio's tolerance for affine couplings (tests/test_gpu_parity.py)"""
    return 2e-4 * max(1.0, d / 64)


SPLINE_C_FACTOR = 4.0      # see spline_c
# worst fp32-against-fp64 difference of log q over the spline cases of each file's matrix, from the CPU alone: 4 x the
# figure exceeds affine_c (2e-4 up to d = 64) only for particles, by a quarter
SPLINE_FIGURES = {'fullrank': 2.4e-5, 'gmrf': 2.8e-5, 'latent_gaussian': 2.3e-5, 'logreg': 2.4e-5, 'mixture': 2.2e-5,
                  'phi4': 2.1e-5, 'irt': 2.4e-5, 'varying_effects': 3.1e-5, 'rosenbrock': 4.2e-5, 'sv': 4.4e-5,
                  'sparse_logreg': 2.5e-5, 'particles': 6.4e-5}


def spline_c(d, of, steps):
    """The same for spline couplings, measured against the reference and not against the kernels: the oracle flow cast
    to fp32 on the CPU against itself in fp64 at the case's own proposals (the inverse pass and log q at the oracle's
    latents, re-derived from x' through the fp64 forward pass; the forward pass and log q at x'), SPLINE_C_FACTOR = 4
    times the worst difference of log q over the case, and never less than affine_c(d).  The flow alone: what the fp32
    proposal's rounding does to U(x') is no part of it, as it is none of affine_c.

    Measured on the CPU at the spline cases of the per-target files' matrices (d = 3 .. 101, widths 4 and 8), worst
    fp32-against-fp64 difference per file: SPLINE_FIGURES.  Returns (c, the worst difference)."""
    f32 = copy.deepcopy(of).float()
    worst = 0.0
    with torch.no_grad():
        for js in steps:
            xp = js.x_prime.reshape(js.x_prime.shape[0], *of.event_shape)
            z, _ = of.bijection.forward(xp)                                   # the latents the proposals came from
            _x32, ld32 = f32.bijection.inverse(z.float())
            lq_inv = (f32.base_log_prob(z.float()) - ld32).double()
            worst = max(worst, float((lq_inv - js.f_xp).abs().max()),
                        float((f32.log_prob(xp.float()).double() - of.log_prob(xp)).abs().max()))
    return max(affine_c(d), SPLINE_C_FACTOR * worst), worst


def flow_mh_tolerance(steps, c):
    """(T, n): c + 2e-5 |log r| + 8 ulp(fp32) (|U(x)| + |U(x')| + |log q(x)| + |log q(x')|), the four fp32 numbers the
    kernel subtracts (csrc/flow_b_mh.hpp: lr = -u_xp + u_x + f_x - f_xp)"""
    lr = torch.stack([js.log_alpha.reshape(-1).double() for js in steps])
    size = torch.stack([(js.u_x.abs() + js.u_xp.abs() + js.f_x.abs() + js.f_xp.abs()).reshape(-1).double() for js in steps])
    size = torch.where(torch.isfinite(size), size, torch.zeros_like(size))
    return c + 2e-5 * torch.where(torch.isfinite(lr), lr.abs(), torch.zeros_like(lr)) + 8 * 2.0 ** -24 * size


def u_sensitivity_of(steps, target, ulps=4):
    """(T, n): ulps ulp(fp32) sum_i |dU/dx_i (x')| |x'_i| in fp64 autograd: the kernel's proposal is an fp32 flow image
    whose every coordinate carries a few roundings (the elementwise layers and the coupling: 4), and a potential of r^-12
    terms turns those into a change of U(x') that the magnitudes of flow_mh_tolerance do not see"""
    out = []
    for js in steps:
        x = js.x_prime.detach().clone().requires_grad_(True)
        u = target(x)
        u = torch.where(torch.isfinite(u), u, torch.zeros_like(u))
        g, = torch.autograd.grad(u.sum(), x)
        out.append(ulps * 2.0 ** -24 * (g.abs() * x.detach().abs()).sum(1))
    return torch.stack(out)


def oracle_inputs_ok(steps, what, *, margin, floor=None, cap=0.10, skip_below_minus_50=False):
    """What a flow-MH case asks of its inputs, from the fp64 oracle alone: at least `floor` of the proposals accepted
    (None: no floor), under `cap` of the chains within `margin` of a tie, every log ratio finite and above -50 unless
    skip_below_minus_50.  Returns (acceptance, tie share, least log ratio)."""
    lr = torch.stack([js.log_alpha.reshape(-1).double() for js in steps])
    lu = torch.stack([js.log_u.reshape(-1).double() for js in steps])
    acc = float(torch.stack([js.mask.reshape(-1) for js in steps]).float().mean())
    ties = float(((lu - lr).abs() < margin).any(0).float().mean())
    print('%s: oracle accepts %.3f of the proposals, %.1f %% of the chains near a tie, log ratios %.1f .. %.1f'
          % (what, acc, 100 * ties, float(lr.min()), float(lr.max())))
    if floor is not None:
        assert acc >= floor, (what, 'acceptance', acc, floor)
    assert ties < cap, (what, 'near-ties', ties)
    if not skip_below_minus_50:
        assert bool(torch.isfinite(lr).all()) and float(lr.min()) > -50, (what, 'log ratio', float(lr.min()))
    return acc, ties, float(lr.min())


def compare_flow_mh(got_m, got_lr, steps, what, *, c, margin, comparable=None, floor=None, cap=0.10,
                    skip_below_minus_50=False, adjusted=True, min_share=0.97, u_sensitivity=None):
    """The kernel's decisions got_m (T, n) bool and log ratios got_lr (T, n) of T flow-proposal Metropolis transitions
    against the oracle's JumpSteps, row by row.  A row (transition, chain) is comparable while the chain has followed
    the oracle: before its first disagreeing decision, or, with `comparable` (T, n) given (the jump samplers: inner
    transitions lie between the jumps), where that says so.  In order:
      the inputs (oracle_inputs_ok: floor, tie cap, finite log ratios);
      more than min_share of the rows comparable;
      decisions: equal on every comparable row whose fp64 |log u - log r| exceeds margin + the row's tolerance (there
        neither the kernel's log ratio nor its log u can turn the test), and on more than min_share of all comparable rows;
      log ratios to flow_mh_tolerance(steps, c) on every comparable row (with skip_below_minus_50: on those whose fp64
        log ratio is finite and above -50; the others must be rejected).
    Unadjusted (every proposal kept): all decisions 1, the log ratios compared on every row.
    u_sensitivity (T, n), for a target as steep as a pair potential alone: what the fp32 rounding of the proposal's
    coordinates does to U(x'), u_sensitivity_of(steps, target), added to the tolerance under its own name.
    Returns (mask (n,) of the chains that followed through every transition, worst log-ratio error over tolerance)."""
    got_m, got_lr = got_m.bool(), got_lr.double()
    want_m = torch.stack([js.mask.reshape(-1).bool() for js in steps])
    want_lr = torch.stack([js.log_alpha.reshape(-1).double() for js in steps])
    lu = torch.stack([js.log_u.reshape(-1).double() for js in steps])
    assert got_m.shape == want_m.shape == got_lr.shape, (got_m.shape, want_m.shape, got_lr.shape)
    tol = flow_mh_tolerance(steps, c)
    if u_sensitivity is not None:
        tol = tol + torch.where(torch.isfinite(u_sensitivity), u_sensitivity, torch.zeros_like(u_sensitivity))
    if not adjusted:
        assert bool(got_m.all()) and bool(want_m.all()), what
        rows = torch.ones_like(want_m)
    else:
        oracle_inputs_ok(steps, what, margin=margin, floor=floor, cap=cap, skip_below_minus_50=skip_below_minus_50)
        same = got_m == want_m
        if comparable is None:
            first = torch.ones(1, same.shape[1], dtype=torch.bool)
            comparable = torch.cumprod(torch.cat([first, same[:-1]]).int(), 0).bool()
        share = float(comparable.float().mean())
        assert share > min_share, (what, 'comparable rows', share)
        clear = comparable & ((lu - want_lr).abs() > margin + tol)
        wrong = clear & ~same
        assert not bool(wrong.any()), (what, 'decisions differ on %d rows clear of a tie' % int(wrong.sum()),
                                       want_lr[wrong][:4].tolist(), got_lr[wrong][:4].tolist())
        assert float(same[comparable].float().mean()) > min_share, what
        rows = comparable
        if skip_below_minus_50:
            hopeless = ~torch.isfinite(want_lr) | (want_lr <= -50)
            assert not bool(got_m[comparable & hopeless].any()), what
            rows = comparable & ~hopeless
    assert bool(rows.any()), (what, 'no log ratio to compare')
    err = (got_lr - want_lr).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    worst = int(torch.argmax(torch.where(rows, err / tol, torch.zeros_like(err))))
    t_w, c_w = divmod(worst, err.shape[1])
    ratio = float((err / tol)[t_w, c_w])
    print('%s: worst log-ratio error %.2e at tolerance %.2e (log r %.3f), accepted %d of %d'
          % (what, float(err[t_w, c_w]), float(tol[t_w, c_w]), float(want_lr[t_w, c_w]), int(got_m.sum()), got_m.numel()))
    assert bool((err[rows] <= tol[rows]).all()), (what, float(err[t_w, c_w]), float(tol[t_w, c_w]))
    follows = (comparable & same).all(0) if adjusted else torch.ones(got_m.shape[1], dtype=torch.bool)
    return follows, ratio


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


class FlowRecord:
    """As Record for the flow-proposal Metropolis step: every launch_flow_mh (the name as nfmc_amd.samplers.jump and
    .imh bind it) is handed a mask buffer and a log-ratio buffer, and every jump tail (make_jump_tail) a mask_out and a
    log_ratio_out of its own; stacked() is (T, n) in the order of the transitions.  `tails` counts the jumps that rode
    behind an inner launch, `launches` those on the flow-MH kernel."""

    def __init__(self, monkeypatch):
        from nfmc_amd import hip
        from nfmc_amd.samplers import imh, jump
        self.masks, self.log_ratios, self.tails, self.launches = [], [], 0, 0
        orig, orig_tail = jump.launch_flow_mh, jump.make_jump_tail

        def launch(run, flow, pot, logq, k, step0, cached, adjusted, stats_struct, samples=None, masks_out=None,
                   log_ratio_out=None):
            if masks_out is None:
                masks_out = torch.zeros(k, run.n, dtype=torch.uint8, device=run.dev)
            if log_ratio_out is None:
                log_ratio_out = torch.zeros(k, run.n, dtype=torch.float32, device=run.dev)
            self.masks.append(masks_out)
            self.log_ratios.append(log_ratio_out)
            self.launches += 1
            return orig(run, flow, pot, logq, k, step0, cached, adjusted, stats_struct, samples, masks_out, log_ratio_out)

        def tail(run, flow, adjusted):
            t = orig_tail(run, flow, adjusted)
            m = torch.zeros(1, run.n, dtype=torch.uint8, device=run.dev)
            lr = torch.zeros(1, run.n, dtype=torch.float32, device=run.dev)
            t.mask_out, t.log_ratio_out = hip.ptr(m, torch.uint8), hip.ptr(lr)
            t._keep += [m, lr]
            self.masks.append(m)
            self.log_ratios.append(lr)
            self.tails += 1
            return t
        for mod in (jump, imh):
            monkeypatch.setattr(mod, 'launch_flow_mh', launch)
        monkeypatch.setattr(jump, 'make_jump_tail', tail)

    def stacked(self):
        return torch.cat(self.masks).cpu().bool(), torch.cat(self.log_ratios).cpu()


# --------------------------------------------------------------------------------------------- builders
def _flow_objects(d, n_hidden, spline, n_layers, hidden_layers=None):
    """(package flow, oracle flow) of one architecture, weights untouched; hidden_layers: the conditioner's hidden-layer
    count (conditioner_kwargs['n_layers'], the NHL of the matrix-core kernels), None: the architecture's default of 2"""
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.util import create_flow_object
    from oracle import flow as oflow
    ck = {} if n_hidden is None else {'n_hidden': n_hidden}
    if hidden_layers is not None:
        ck['n_layers'] = int(hidden_layers)
    kw = {'conditioner_kwargs': ck} if ck else {}
    if n_layers is not None:
        kw['n_layers'] = n_layers
    if spline:
        return create_flow_object('c-rqnsf', (d,), **kw), oflow.Flow(oflow.CRQNSF((d,), **kw))
    return Flow(RealNVP((d,), **kw)), oflow.Flow(oflow.RealNVP((d,), **kw))


def flow_pair(d, seed=5, n_hidden=None, spline=False, n_layers=None, init_seed=None, hidden_layers=None):
    """(package flow, fp64 oracle flow) with the same perturbed weights (oracle.flow.perturb_, every parameter touched);
    n_hidden, n_layers (coupling layers) and hidden_layers (the conditioner's hidden layers) for either coupling, None:
    the architecture's defaults.  The weights that are
    perturbed are torch's default initialisation, drawn from the global generator as it stands; with init_seed they are
    drawn from that seed instead (the global generator is left as it was), which a case whose inputs must satisfy a
    condition needs."""
    from oracle import flow as oflow
    if init_seed is None:
        f, of = _flow_objects(d, n_hidden, spline, n_layers, hidden_layers)
    else:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(init_seed)
            f, of = _flow_objects(d, n_hidden, spline, n_layers, hidden_layers)
    of = oflow.perturb_(of, seed, 0.3, 0.75) if spline else oflow.perturb_(of, seed, 0.2, 0.7071)
    f.load_state_dict(of.state_dict())
    return f, of.double()


_LAPLACE = {}


def laplace_fit(p):
    """(mode c, marginal standard deviations s) of a Laplace fit of p.target in fp64 on the CPU: LBFGS from the mean of
    the starts, then the autograd Hessian H at the mode; s = sqrt(diag(H^-1)), the eigenvalues of H clamped from below at
    1e-8 of the largest (a flat or negative direction gets a wide, finite scale).  One fit per problem object."""
    hit = _LAPLACE.get(id(p.target))
    if hit is not None and hit[0] is p.target:
        return hit[1], hit[2]
    d = p.d
    c = p.x0.double().reshape(-1, d).mean(0).clone().requires_grad_(True)
    opt = torch.optim.LBFGS([c], lr=1.0, max_iter=500, tolerance_grad=1e-10, tolerance_change=1e-14, line_search_fn='strong_wolfe')

    def closure():
        opt.zero_grad()
        u = p.target(c[None]).sum()
        u.backward()
        return u
    opt.step(closure)
    c = c.detach()
    hess = torch.autograd.functional.hessian(lambda x: p.target(x[None]).sum(), c, vectorize=True)
    lam, vec = torch.linalg.eigh(0.5 * (hess + hess.t()))
    lam = lam.clamp_min(1e-8 * float(lam.max()))
    s = ((vec ** 2) / lam[None]).sum(1).sqrt()
    assert torch.isfinite(c).all() and torch.isfinite(s).all() and bool((s > 0).all()), p.name
    _LAPLACE[id(p.target)] = (p.target, c, s)
    return c, s


def local_fit(p, shrink, at='starts'):
    """(point c, scales s) for a proposal that sits INSIDE the target where laplace_fit has no use: c the mean of the
    file's starts (at='starts'; a point of ordinary energy where the mode is degenerate, as in a funnel's neck) or the
    LBFGS mode (at='mode'), s = shrink / sqrt(|d^2 U / dx_i^2|) at c, the conditional standard deviations times shrink
    (a curvature under 1e-8 of the largest counts as that).  With chains started at c + s eps (centred) the target
    varies little across such a proposal when shrink is small, so the fp64 oracle accepts; U(x'), log q(x') and the
    carry are exercised as with any other accepting input."""
    key = (id(p.target), shrink, at)
    hit = _LAPLACE.get(key)
    if hit is not None and hit[0] is p.target:
        return hit[1], hit[2]
    c = laplace_fit(p)[0] if at == 'mode' else p.x0.double().reshape(-1, p.d).mean(0)
    hess = torch.autograd.functional.hessian(lambda x: p.target(x[None]).sum(), c, vectorize=True)
    curv = torch.diagonal(hess).abs()
    s = shrink / curv.clamp_min(1e-8 * float(curv.max())).sqrt()
    assert torch.isfinite(c).all() and torch.isfinite(s).all() and bool((s > 0).all()), p.name
    _LAPLACE[key] = (p.target, c, s)
    return c, s


def centred_flow_pair(p, seed=5, n_hidden=None, spline=False, n_layers=None, *, scale, centre=None, hidden_layers=None):
    """flow_pair's architecture (hidden_layers: the conditioner's hidden-layer count) as the identity map (every weight 0; a spline's interior knot derivatives 1), every
    parameter perturbed by `scale` (oracle.flow.perturb_), and the data-side ElementwiseAffine set so that the flow's
    forward pass starts z = (x - c) / s, (c, s) = laplace_fit(p) or the `centre` given (local_fit), the perturbation on
    top: a proposal that sits on the target closely enough for the Metropolis test to accept.  Nothing is drawn from
    torch's global generator."""
    from oracle import flow as oflow
    c, s = laplace_fit(p) if centre is None else centre
    f, of = _flow_objects(p.d, n_hidden, spline, n_layers, hidden_layers)
    of = of.double()
    with torch.no_grad():
        for prm in of.parameters():
            prm.zero_()
        for layer in of.bijection.layers:
            if isinstance(layer, oflow.RQSCoupling):             # d_k = MIN_DERIV + softplus(raw) = 1: the identity
                k, raw = layer.n_bins, math.log(math.expm1(1.0 - oflow.RQS_MIN_DERIV))
                layer.conditioner[-1].bias.reshape(layer.d_b, 3 * k - 1)[:, 2 * k:] = raw
    of = oflow.perturb_(of, seed, scale)
    with torch.no_grad():
        first = of.bijection.layers[0]                      # forward: exp(log_scale) x + shift
        first.log_scale.sub_(s.log())
        first.shift.sub_(torch.exp(first.log_scale) * c)
    f.load_state_dict({k: v.float() for k, v in of.state_dict().items()})
    of.load_state_dict({k: v.double() for k, v in f.state_dict().items()})   # the oracle holds the fp32 weights exactly
    return f, of


def flow_inputs(p, d, n, flow_seed=5, spline=False, from_d=25, centre=None):
    """The inputs of the files' IMH and jump cases from before the matrix: (problem, flows).  From d = 25 up the
    fp64 oracle alone accepts no proposal of a flow about the origin, so those cases run on a centred flow
    (centred_flow_pair about laplace_fit or the `centre` given; RealNVP perturbation 0.2, 0.05 from d = 200, splines half
    of that) from centred starts; below,
    flow_pair's flow about the origin (its initial weights drawn from flow_seed) and the file's own starts."""
    if d < from_d:
        return p, flow_pair(d, flow_seed, spline=spline, init_seed=flow_seed)
    scale = (0.2 if d < 200 else 0.05) * (0.5 if spline else 1.0)
    return centred(p, n, 3, centre), centred_flow_pair(p, flow_seed, spline=spline, scale=scale, centre=centre)


def with_starts(p, x0):
    """the problem p with other starts (p itself is shared and stays as it is)"""
    if hasattr(p, '_replace'):
        return p._replace(x0=x0)
    q = copy.copy(p)
    q.x0 = x0
    return q


def centred(p, n, seed, centre=None):
    """p started at c + s eps rounded to fp32, (c, s) = laplace_fit(p) or the `centre` given: n chains, eps ~ N(0, I) of
    `seed`"""
    c, s = laplace_fit(p) if centre is None else centre
    eps = torch.randn(n, p.d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return with_starts(p, (c + s * eps).float())


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


def imh_run(monkeypatch, pot, d, f, x0, T, seed, composed=False):
    """T FixedIMH transitions, every one on the sequential flow-MH kernel: neither nfmc_imh_parallel_f32 nor the
    composed step; with `composed`, every one on the composed step (split_flow_mh) and none on either kernel"""
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
    if composed:
        assert calls == {'launch_imh_parallel': 0, 'launch_flow_mh': 0, 'split_flow_mh': T}, calls
    else:
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


_ORACLE_ONLY = [False]


@contextlib.contextmanager
def oracle_only():
    """Inside, the flow-MH bodies below stop after the conditions on their inputs (oracle_inputs_ok), which need the fp64
    oracle alone: the host tests run every GPU case's inputs through them on the CPU."""
    _ORACLE_ONLY[0] = True
    try:
        yield
    finally:
        _ORACLE_ONLY[0] = False


def _param_sets(fn):
    """the keyword sets of a test function's pytest.mark.parametrize marks"""
    sets = [{}]
    for m in getattr(fn, 'pytestmark', []):
        if m.name != 'parametrize':
            continue
        names = [v.strip() for v in m.args[0].split(',')] if isinstance(m.args[0], str) else list(m.args[0])
        rows = [getattr(v, 'values', v) for v in m.args[1]]
        sets = [dict(s, **dict(zip(names, row if len(names) > 1 else (row,)))) for s in sets for row in rows]
    return sets


def probe_flow_inputs(module, monkeypatch):
    """Every case of the tests a GPU test file names in FLOW_TESTS, on the CPU and up to the conditions on its inputs
    (oracle_only): the acceptance floor, the tie cap and the finite log ratios hold for the fp64 oracle alone.  Returns
    the number of cases."""
    count = 0
    with oracle_only():
        for name in module.FLOW_TESTS:
            fn = getattr(module, name)
            for kw in _param_sets(fn):
                fn(None, monkeypatch, **kw)
                count += 1
    return count


def flow_layout(d, n, cfg=None):
    """(CPL, LPC) csrc/flow_b_kernels.hip: flow_mh_b_launch picks: the smallest capacity CPL LPC >= d, at equal capacity
    CPL = 4 up to 4096 chains and 8 above; cfg = (cpl, lpc): the NFMC_FLOWB_CFG override, taken when it holds d"""
    cfgs = ((4, 1), (4, 2), (4, 4), (4, 8), (8, 8), (4, 16), (8, 16), (4, 32), (8, 32), (4, 64), (8, 64))
    if cfg is not None and tuple(cfg) in cfgs and cfg[0] * cfg[1] >= d:
        return tuple(cfg)
    want, best = (4 if n <= 4096 else 8), None
    for k in cfgs:
        if k[0] * k[1] < d:
            continue
        if best is None or k[0] * k[1] < best[0] * best[1] or (k[0] * k[1] == best[0] * best[1] and k[0] == want):
            best = k
    return best


def jump_comparable(got, want, n_inner, atol, rtol):
    """(T, n): the chain's kept states of every transition before jump i agree with the oracle's, so that jump i starts
    from the oracle's state; got, want (T (n_inner + 1), n, d)"""
    ok = ((got - want).abs() <= atol + rtol * want.abs()).all(2)                    # (transitions, n)
    before = torch.cumprod(torch.cat([torch.ones(1, ok.shape[1], dtype=torch.bool), ok[:-1]]).int(), 0).bool()
    return before[n_inner::n_inner + 1]


def jump_matches_oracle(monkeypatch, p, inner_kind, *, T, Kin, seed, h, imd, fuse_tail, spline, atol, rtol, share, jump_slack,
                        margin, skip_below_minus_50, L=3, flows=None, floor=None, tail_expected=None, refused=False):
    """jump_mala / jump_hmc (inner_kind 'mala' / 'hmc', L leapfrog steps) on a fixed flow, native stream: the inner
    transitions fused, the jump on the register flow-MH kernel or, with fuse_tail, as the tail of the last inner launch
    (affine flows only).  flows None: flow_pair's perturbed flow about the origin, else (package flow, oracle flow).
    imd None: the inner kernel is the sampler's default one with its step size set to h; else the kernel of
    (step_size=h, inv_mass_diag=imd).  The jumps' decisions and log ratios by compare_flow_mh on the chains that reach
    each jump in the oracle's state; a share of the chains must follow the oracle through all T (Kin + 1) transitions, and
    the accepted jumps agree to jump_slack and equal the kernel's own masks.  refused: the flow-MH probe refuses the shape
    (the 120 KB LDS bound), every jump is composed (split_flow_mh) and the states and counters alone are compared.  tail_expected: whether every jump must have
    ridden behind the inner launch (None: fuse_tail and not spline, as production decides for most kinds)."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, d = p.x0.shape[0], p.d
    f, of = flow_pair(d, spline=spline) if flows is None else flows
    what = 'jump_%s %s%s' % (inner_kind, p.name, ' tail' if fuse_tail else '')
    tr = osamp.jump_sample(p.x0.double(), p.target, of, 'langevin' if inner_kind == 'mala' else 'hmc', T, Kin, h,
                           inv_mass_diag=None if imd is None else imd.double(), n_leapfrog=L,
                           noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    oracle_inputs_ok(tr.flow_steps, what, margin=margin, floor=floor, skip_below_minus_50=skip_below_minus_50)
    if _ORACLE_ONLY[0]:
        return
    rec = FlowRecord(monkeypatch)
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = Spy(monkeypatch)
    if inner_kind == 'mala':
        inner = None if imd is None else mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd)
        s = jump.JumpMALA((d,), p.pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T), inner,
                          mcmc.LangevinParameters(n_iterations=Kin))
    else:
        kw = {} if imd is None else {'inv_mass_diag': imd}
        s = jump.JumpHMC((d,), p.pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T),
                         mcmc.HMCKernel(event_size=d, n_leapfrog_steps=L, step_size=h, **kw), mcmc.HMCParameters(n_iterations=Kin))
    if imd is None:
        s.inner_sampler.kernel.step_size = h
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    out = s.sample(p.x0, show_progress=False)
    got, want = out.samples.reshape(T * (Kin + 1), n, d), tr.stacked().float()
    if refused:                                               # no flow-MH kernel for the shape: every jump composed
        assert flow_mh_refuses(torch.device('cuda', torch.cuda.current_device()), p, f), what   # NFMC_EUNSUPPORTED
        assert not spy.calls and len(split) == T and (rec.tails, rec.launches) == (0, 0), (len(split), rec.tails, rec.launches)
        same = (got - want).abs().amax(dim=(0, 2)) < atol + rtol * want.abs().amax(dim=(0, 2))
        assert same.float().mean() > share, float(same.float().mean())
        assert out.statistics.n_attempted_jumps == n * T
        assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= jump_slack
        return
    assert not spy.calls and not split                        # inner loop and jump fused
    if not fuse_tail or spline:
        assert len(flow_mh) == T                              # each jump on the flow-MH kernel (the tail is affine only)
    if tail_expected is None:
        tail_expected = fuse_tail and not spline and p.pot.jump_tail_ok()
    assert (rec.tails, rec.launches) == ((T, 0) if tail_expected else (0, T)), (rec.tails, rec.launches)
    got_m, got_lr = rec.stacked()
    c = spline_c(d, of, tr.flow_steps)[0] if spline else affine_c(d)
    compare_flow_mh(got_m, got_lr, tr.flow_steps, what, c=c, margin=margin, skip_below_minus_50=skip_below_minus_50,
                    comparable=jump_comparable(got, want, Kin, atol, rtol), min_share=share)
    same = (got - want).abs().amax(dim=(0, 2)) < atol + rtol * want.abs().amax(dim=(0, 2))
    assert same.float().mean() > share, float(same.float().mean())
    assert out.statistics.n_attempted_jumps == n * T
    assert out.statistics.n_accepted_jumps == int(got_m.sum())
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= jump_slack


def jump_mala_matches_oracle(monkeypatch, p, **kw):
    """jump_matches_oracle with inner MALA"""
    jump_matches_oracle(monkeypatch, p, 'mala', **kw)


def jump_hmc_matches_oracle(monkeypatch, p, **kw):
    """jump_matches_oracle with inner HMC: oracle.samplers.jump_sample(..., 'hmc', ...)"""
    jump_matches_oracle(monkeypatch, p, 'hmc', **kw)


def flow_mh_refuses(dev, p, f):
    """nfmc_flow_mh_supported_f32's answer for FixedIMH on flow f from p's starts is NFMC_EUNSUPPORTED"""
    from nfmc_amd import hip
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    s = imh.FixedIMH((p.d,), p.pot, imh.IMHKernel((p.d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, p.x0)
    logq = torch.empty(p.x0.shape[0], device=dev)
    pa, _keep = _flow_mh_probe_args(run, f, p.pot, logq, True)
    return _rc(hip.lib().nfmc_flow_mh_supported_f32, C.byref(pa)) == hip.EUNSUPPORTED


def flow_mh_matches_oracle(monkeypatch, p, flows, *, T, seed, spline, what, compare, margin, skip_below_minus_50, floor=None,
                           cfg=None, refused=False, dev=None):
    """FixedIMH from p.x0 on the register flow-MH kernel (flow_mh_b_kernel; affine, or the 'c-rqnsf' spline
    instantiation) against imh_sample on the same Philox streams; flows = (package flow, fp64 oracle flow).  Every launch
    is handed a mask and a log-ratio buffer (FlowRecord): the rows by compare_flow_mh (floor: the least share of
    proposals the oracle alone must accept), then the kept states by `compare` as before, then the counters: attempted
    n T, accepted the sum of the kernel's own masks.  cfg = (cpl, lpc): NFMC_FLOWB_CFG for the run, the sibling layout
    of the same capacity that a run of more than 4096 chains takes.
    refused (needs dev): the shape is one the kernel's LDS bound refuses: the probe answers NFMC_EUNSUPPORTED, every
    transition takes the composed path (split_flow_mh) and the kept states still follow the oracle."""
    from oracle import samplers as osamp
    n, d = p.x0.shape[0], p.d
    f, of = flows
    tr = osamp.imh_sample(p.x0.double(), p.target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    oracle_inputs_ok(tr.flow_steps, what, margin=margin, floor=floor, skip_below_minus_50=skip_below_minus_50)
    if _ORACLE_ONLY[0]:
        return
    if cfg is not None:
        monkeypatch.setenv('NFMC_FLOWB_CFG', '%d,%d' % tuple(cfg))
    if refused:
        assert flow_mh_refuses(dev, p, f), what
        out = imh_run(monkeypatch, p.pot, d, f, p.x0, T, seed, composed=True)
        compare(out.samples.reshape(T, n, d), tr, what)
        return
    rec = FlowRecord(monkeypatch)
    out = imh_run(monkeypatch, p.pot, d, f, p.x0, T, seed)
    got_m, got_lr = rec.stacked()
    c = spline_c(d, of, tr.flow_steps)[0] if spline else affine_c(d)
    compare_flow_mh(got_m, got_lr, tr.flow_steps, what, c=c, margin=margin, skip_below_minus_50=skip_below_minus_50)
    compare(out.samples.reshape(T, n, d), tr, what)
    assert out.statistics.n_accepted_trajectories == int(got_m.sum()), what


def imh_matches_oracle(monkeypatch, p, *, T, seed, flow_seed, spline, what, compare, margin, skip_below_minus_50, flows=None,
                       floor=None):
    """flow_mh_matches_oracle on flow_pair's perturbed flow about the origin (flows None) or on the pair given"""
    flows = flow_pair(p.d, flow_seed, spline=spline) if flows is None else flows
    flow_mh_matches_oracle(monkeypatch, p, flows, T=T, seed=seed, spline=spline, what=what, compare=compare, margin=margin,
                           skip_below_minus_50=skip_below_minus_50, floor=floor)


DirectRun = collections.namedtuple('DirectRun', 'samples masks log_ratios logq x stats')


def _direct_flow_mh(dev, p, f, T, seed, adjusted, *, cached=None, replay=None, stats=None, store=None, prefill=None, detail=False):
    """T transitions of one nfmc_flow_mh_steps_f32 launch from p.x0: (kept states (T, n, d), masks, log ratios), CPU.
    cached: log q of the starts (n,), computed beforehand (flow.log_prob); the launch runs with logq_cached = 1.
    replay: (normals (T, n, d), uniforms (T, n) or None), handed to the kernel in place of its Philox streams.
    stats: 'immediate' (run.stats.struct()) or 'deferred' (struct(defer=True, attempted=n T), then the fold); the totals
      come back as a dict: accepted, attempted, nonfinite, sum_x, sum_x2 (fp64).  None: immediate, not read back.
    prefill: a value the run's statistics scratch (every slab) is filled with before the launch: an immediate launch must
      overwrite its slabs, a deferred one add to them.
    store: (thinning, max_samples): the kept states go through a DeviceSampleStore of T offered transitions and come
      back in chronological order (DeviceSampleStore.ordered).
    With any of these, or detail, the result is a DirectRun: the three above, then logq (n,) as the launch left it, the
    final states x (n, d) and the statistics (or None)."""
    from nfmc_amd import hip
    from nfmc_amd.containers import DeviceSampleStore
    from nfmc_amd.samplers import imh, jump
    from nfmc_amd.samplers.common import Run
    n, d = p.x0.shape[0], p.d
    s = imh.FixedIMH((d,), p.pot, imh.IMHKernel((d,), flow=f), imh.IMHParameters(n_iterations=T))
    s.seed = seed
    if replay is not None:
        s.replay = (replay[0].float(), None if replay[1] is None else replay[1].float())
    run = Run(s, p.x0)
    logq = torch.empty(n, dtype=torch.float32, device=dev)
    if cached is not None:
        logq.copy_(cached.reshape(n).float())
    masks = torch.zeros(T, n, dtype=torch.uint8, device=dev)
    lr = torch.zeros(T, n, dtype=torch.float32, device=dev)
    samples = torch.zeros(T, n, d, dtype=torch.float32, device=dev) if store is None else DeviceSampleStore(n, d, dev, T, *store)
    assert jump.flow_mh_supported(run, f, p.pot, logq, adjusted)
    assert stats in (None, 'immediate', 'deferred'), stats
    if prefill is not None:
        run.stats.scratch.fill_(prefill)
    st = run.stats.struct(defer=True, attempted=n * T) if stats == 'deferred' else run.stats.struct()
    jump.launch_flow_mh(run, f, p.pot, logq, T, 0, cached is not None, adjusted, st, samples, masks, lr)
    torch.cuda.synchronize()
    kept = samples.cpu() if store is None else samples.ordered().cpu().clone()
    if not (detail or cached is not None or replay is not None or stats is not None or store is not None or prefill is not None):
        return kept, masks.cpu().bool(), lr.cpu()
    totals = None
    if stats is not None:
        sum_x, sum_x2, cnt, _jc = run.stats.host_totals()
        totals = {'accepted': int(cnt[hip.CNT_ACCEPTED]), 'attempted': int(cnt[hip.CNT_ATTEMPTED]),
                  'nonfinite': int(cnt[hip.CNT_NONFINITE]), 'sum_x': sum_x.clone(), 'sum_x2': sum_x2.clone()}
    return DirectRun(kept, masks.cpu().bool(), lr.cpu(), logq.cpu(), run.x.cpu(), totals)


FLOW_MH_KERNELS = ('register', 'mfma', 'wide', 'lane')


def flow_mh_kernel_of(dev, p, f, adjusted=True):
    """Which kernel nfmc_flow_mh_steps_f32 takes for flow f from p's starts under the environment as it stands: 'register'
    (flow_mh_b_kernel), 'mfma' (flow_mh_mfma_kernel), 'wide' (flow_mh_wide_kernel), 'lane' (flow_mh_kernel<HP>), or None
    where nfmc_flow_mh_supported_f32 refuses the launch.  csrc/flow_kernels.hip: flow_mh_steps' order, from the library's
    own answers about the flow as the package presents it (packed: the width it is padded to, the workspace it carries):
    the probe; nfmc_realnvp_padded_hidden (above 32: a matrix-core weight layout); nfmc_flow_scratch_bytes > 0 (the
    streamed kernel's shapes) together with a workspace; and the two switches flow_mh_steps reads on every call,
    NFMC_FLOW_TILE_PATH (no register kernel) and NFMC_FLOW_NO_MFMA (no matrix cores), set to any value."""
    import os
    from nfmc_amd import hip
    from nfmc_amd.samplers import imh
    from nfmc_amd.samplers.common import Run
    from nfmc_amd.samplers.jump import _flow_mh_probe_args
    s = imh.FixedIMH((p.d,), p.pot, imh.IMHKernel((p.d,), flow=f), imh.IMHParameters(n_iterations=1))
    run = Run(s, p.x0)
    logq = torch.empty(p.x0.shape[0], device=dev)
    pa, _keep = _flow_mh_probe_args(run, f, p.pot, logq, adjusted)
    rc = _rc(hip.lib().nfmc_flow_mh_supported_f32, C.byref(pa))
    if rc == hip.EUNSUPPORTED:
        return None
    assert rc == 0, rc
    st = pa.flow
    tile_path, no_mfma = 'NFMC_FLOW_TILE_PATH' in os.environ, 'NFMC_FLOW_NO_MFMA' in os.environ
    if st.n_hidden <= 8 and not tile_path:
        return 'register'
    hp = int(hip.lib().nfmc_realnvp_padded_hidden(st.n_hidden))
    matrix = hp > 32 and st.n_bins == 0 and st.n_coupling > 0 and st.n_hidden_layers in (1, 2) and not no_mfma
    if matrix and st.d in (64, 128):
        return 'mfma'
    if matrix and int(hip.lib().nfmc_flow_scratch_bytes(C.byref(st), run.n, 1)) > 0 and st.scratch:
        return 'wide'
    return 'lane'


def flow_mh_unadjusted_matches_oracle(dev, monkeypatch, p, flows, *, T, seed, spline, what, atol, rtol, cfg=None):
    """launch_flow_mh(..., adjusted=False): every proposal is kept, so x <- x', U(x) <- U(x') and log q(x) <- log q(x')
    run at every transition of every chain.  The kept states are the fp64 flow's samples at the same Philox latents (to
    atol + rtol |x'|), and the log ratio the kernel still writes at transition s + 1, which uses the U and log q carried
    from transition s, follows the oracle's on every row (flow_mh_tolerance)."""
    from oracle import samplers as osamp
    f, of = flows
    tr = osamp.imh_sample(p.x0.double(), p.target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64), adjusted=False)
    lr = torch.stack([js.log_alpha for js in tr.flow_steps])
    print('%s: unadjusted, log ratios %.1f .. %.1f' % (what, float(lr.min()), float(lr.max())))
    assert bool(torch.isfinite(lr).all()), what
    if _ORACLE_ONLY[0]:
        return
    if cfg is not None:
        monkeypatch.setenv('NFMC_FLOWB_CFG', '%d,%d' % tuple(cfg))
    got, got_m, got_lr = _direct_flow_mh(dev, p, f, T, seed, False)
    c = spline_c(p.d, of, tr.flow_steps)[0] if spline else affine_c(p.d)
    compare_flow_mh(got_m, got_lr, tr.flow_steps, what, c=c, margin=0.0, adjusted=False)
    want = torch.stack([js.x_prime for js in tr.flow_steps]).float()
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=atol, rtol=rtol, err_msg=what)


def flowb_override_equals_production(dev, monkeypatch, p, f, *, lpc, T, seed):
    """More than 4096 chains take the CPL = 8 sibling by themselves; the same run under NFMC_FLOWB_CFG = '8,<lpc>' must
    be that kernel again: states, masks and log ratios bit for bit.  That the override is read and does switch the
    instantiation is observed through the library, which has no entry point that names the layout: under
    '4,<2 lpc>' the log ratios (fp32 sums over another lane tree) differ from production's in some bit while agreeing
    to 1e-3 + 1e-5 |log r|, and under '8,64' a width-8 flow of two coupling layers (132 KB of LDS at capacity 512) is
    refused by nfmc_flow_mh_supported_f32 where it is taken without.  (No oracle: the 96-chain cases compare the
    CPL = 8 kernels with it through the override.)"""
    assert p.x0.shape[0] > 4096 and flow_layout(p.d, p.x0.shape[0]) == (8, lpc), (p.d, lpc)
    assert f.bijection.n_hidden > 4
    monkeypatch.delenv('NFMC_FLOWB_CFG', raising=False)
    assert not flow_mh_refuses(dev, p, f)
    a = _direct_flow_mh(dev, p, f, T, seed, True)
    monkeypatch.setenv('NFMC_FLOWB_CFG', '8,%d' % lpc)
    b = _direct_flow_mh(dev, p, f, T, seed, True)
    for u, v, name in zip(a, b, ('states', 'masks', 'log ratios')):
        assert torch.equal(u, v), name
    assert bool(torch.isfinite(a[0]).all())
    monkeypatch.setenv('NFMC_FLOWB_CFG', '4,%d' % (2 * lpc))
    c = _direct_flow_mh(dev, p, f, T, seed, True)
    fin = torch.isfinite(a[2]) & torch.isfinite(c[2])
    assert not torch.equal(a[2], c[2]), 'the CPL = 4 sibling gave the same bits: is the override read?'
    assert bool(((a[2] - c[2]).abs()[fin] <= 1e-3 + 1e-5 * a[2].abs()[fin]).all())
    monkeypatch.setenv('NFMC_FLOWB_CFG', '8,64')
    assert flow_mh_refuses(dev, p, f)


# ---- the flow-MH matrix of the per-target files
FLOW_DIMS = {4: 3, 8: 7, 16: 13, 32: 25, 64: 50, 128: 100, 256: 200, 512: 300}     # capacity CPL LPC -> a ragged d in it
FlowCase = collections.namedtuple('FlowCase', 'family cap d n_hidden cfg spline n_layers')


def flow_case_id(c):
    return '%s-cap%d-d%d-h%d%s%s%s' % (c.family, c.cap, c.d, c.n_hidden, '' if c.cfg is None else '-cpl%d' % c.cfg[0],
                                       '-spline' if c.spline else '', '' if c.n_layers is None else '-%dlayer' % c.n_layers)


def flow_cases(dims=None, *, jump_tail=True):
    """The cases every per-target file runs (n = 96 chains, T = 4), dims: capacity -> d (FLOW_DIMS where a kind takes any d).
    flow-MH, affine: one ragged d in each capacity; at 64, 128 and 256 both siblings (CPL = 4 by default, CPL = 8
      through NFMC_FLOWB_CFG) at both conditioner widths (n_hidden 4 -> HP = 4, 8 -> HP = 8), both widths at 512 (width 8 also with a
      single coupling layer: two are refused by the 120 KB LDS bound, so that one launches (8, 64) at HP = 8), the width
      rotating below 64.
    flow-MH, spline: two coupling layers at the six layouts up to capacity 64 at either width, and capacity 128 with a
      single coupling layer (width 4).
    unadjusted: capacities 256 and 512.
    jump tail (unless a kind is never offered it): jump_mala at capacities 128, 256, 512 and both tail widths (at 512 width 8 also with a single coupling layer);
      jump_hmc
      (L = 3) at one d per capacity from 8 to 512, the width rotating."""
    dims = FLOW_DIMS if dims is None else dims
    rot = {4: 3, 8: 6, 16: 4, 32: 8, 64: 4, 128: 8, 256: 4, 512: 4}
    out = [FlowCase('mh', cap, dims[cap], rot[cap], None, False, None) for cap in (4, 8, 16, 32)]
    for cap, lpc in ((64, 8), (128, 16), (256, 32)):
        out += [FlowCase('mh', cap, dims[cap], nh, cfg, False, None) for nh in (4, 8) for cfg in (None, (8, lpc))]
    out += [FlowCase('mh', 512, dims[512], nh, None, False, None) for nh in (4, 8)]
    out.append(FlowCase('mh', 512, dims[512], 8, None, False, 1))       # two width-8 layers are refused there (132 KB of LDS)
    for nh in (4, 8):
        out += [FlowCase('mh', cap, dims[cap], nh, None, True, None) for cap in (4, 8, 16, 32, 64)]
        out.append(FlowCase('mh', 64, dims[64], nh, (8, 8), True, None))
    out.append(FlowCase('mh', 128, dims[128], 4, None, True, 1))
    out += [FlowCase('unadjusted', 256, dims[256], 8, None, False, None), FlowCase('unadjusted', 512, dims[512], 4, None, False, None)]
    if jump_tail:
        out += [FlowCase('jump_mala', cap, dims[cap], nh, None, False, None) for cap in (128, 256, 512) for nh in (4, 8)]
        out.append(FlowCase('jump_mala', 512, dims[512], 8, None, False, 1))       # the (8, 64) tail at width 8
        out += [FlowCase('jump_hmc', cap, dims[cap], rot[cap], None, False, None) for cap in (8, 16, 32, 64, 128, 256, 512)]
    return out


def flow_case_scale(c):
    """the perturbation of a case's centred flow, affine or spline: 0.1 below d = 200 and 0.05 from there (at a fixed
    scale the acceptance falls with d).  The fp64 oracle alone then accepts 0.19 to 0.73 of the proposals of the
    full-rank and GMRF files' cases, splines included; with 0.2 it accepts 0.03 of the spline proposals at d = 50."""
    return 0.1 if c.d < 200 else 0.05


def run_flow_case(dev, monkeypatch, p, c, *, margin, compare, atol, rtol, h_mala, h_hmc, imd=None, refused=False, seed=2718,
                  tail_expected=None, skip_caps=(), centre=None):
    """One FlowCase on the problem p (the file's own, d = c.d): centred flow and starts (96 chains), T = 4 (unadjusted
    3; the jumps T = 2 outer iterations of 2 inner transitions).  The fp64 oracle alone must accept at least 5 % of the
    proposals at capacities up to 128, and everywhere hold the tie cap and keep every log ratio finite and above -50,
    but at the capacities of skip_caps, where the file's problem has hopeless proposals and skip_below_minus_50 is set.
    refused: the case is one the 120 KB LDS bound refuses (flow_mh_matches_oracle; the jumps then take the composed
    path too).  centre: (c, s) of local_fit where laplace_fit has no use.  imd: the inner kernels' mass diagonal, or a function of the inner kind ('mala' / 'hmc') that gives it."""
    assert p.d == c.d, (p.d, c)
    what = '%s %s' % (p.name, flow_case_id(c))
    flows = centred_flow_pair(p, 5, c.n_hidden, c.spline, c.n_layers, scale=flow_case_scale(c), centre=centre)
    q = centred(p, 96, 40 + c.cap, centre)
    floor = 0.05 if c.cap <= 128 else None
    assert c.cfg is None or flow_layout(c.d, 96, c.cfg) == tuple(c.cfg), c
    if c.family == 'mh':
        flow_mh_matches_oracle(monkeypatch, q, flows, T=4, seed=seed + c.d, spline=c.spline, what=what, compare=compare,
                               margin=margin, skip_below_minus_50=c.cap in skip_caps, floor=floor, cfg=c.cfg, refused=refused, dev=dev)
    elif c.family == 'unadjusted':
        flow_mh_unadjusted_matches_oracle(dev, monkeypatch, q, flows, T=3, seed=seed + c.d, spline=c.spline, what=what,
                                          atol=atol, rtol=rtol, cfg=c.cfg)
    else:
        jump_matches_oracle(monkeypatch, q, c.family[5:], T=2, Kin=2, seed=seed + c.d, h=h_mala if c.family == 'jump_mala' else h_hmc,
                            imd=imd(c.family[5:]) if callable(imd) else imd, fuse_tail=True, spline=False, atol=atol, rtol=rtol,
                            share=0.95, jump_slack=2, margin=margin,
                            skip_below_minus_50=c.cap in skip_caps, L=3, flows=flows, floor=floor, tail_expected=tail_expected, refused=refused)


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


# ------------------------------------------------------- the matrix-core NeuTra-HMC trajectory kernels
MFMA_CHAINS, MFMA_WAVES, CK_MAX_GRID = 128, 8, 256    # csrc/mfma_device.hpp: kMfmaChains, kMfmaWaves, kCkMaxGrid


def neutra_presented_hidden(d, nh, hl, n_bins=0):
    """the conditioner width NeuTra presents to nfmc_neutra_hmc_steps_f32 (NeuTra._min_hidden, NFMC_NEUTRA_VALU unset):
    at d = 64 / 128 with one or two hidden layers and affine couplings at least 64 (zero-padded), else the flow's own"""
    return max(nh, 64) if d in (64, 128) and hl in (1, 2) and not n_bins else nh


def neutra_hmc_kernel_of(d, nh, hl, n_bins=0):
    """Which kernel nfmc_neutra_hmc_steps_f32 runs a NeuTra-HMC launch on, from the documented shape rules (DESIGN.md
    section 3.3) for a flow of conditioner width nh, hl hidden layers and n_bins spline bins (0: affine) as the sampler
    presents it: 'mfma' (neutra_leapfrog_mfma_kernel: d = 64 / 128, width up to 128, 1-2 hidden layers, narrower
    conditioners padded to 64), 'wide' (neutra_leapfrog_wide_kernel: the other multiples of 32 from 32 to 512 with
    32 < nh <= 128), 'valu' (the one-chain-per-lane kernels: widths up to 32, and every spline flow, which the entry point
    sends there whatever its width), None where no kernel takes the shape."""
    h = neutra_presented_hidden(d, nh, hl, n_bins)
    if n_bins or h <= 32:
        return 'valu'
    if hl not in (1, 2) or h > 128:
        return None
    if d in (64, 128):
        return 'mfma'
    return 'wide' if d % 32 == 0 and 32 <= d <= 512 else None


def _padded_hidden(h):
    return 64 if h <= 64 else 128                      # nfmc_realnvp_padded_hidden above 32


def neutra_hmc_scratch_bytes(kernel, n, d, hidden, hl, cl):
    """The work area of one launch in bytes, restated per kernel; `hidden` the presented width.
    'wide' (csrc/mfma_wide.hip: nfmc_neutra_wide_scratch_floats): the gradient (n, d), U~ (n rounded up to 4), and three
      rows of d floats (position, gradient, momentum) per chain slot of min(tiles, 256) workgroups of 128 chains.
    'mfma' (csrc/neutra_kernels.hip: nfmc_neutra_scratch_bytes): momentum and gradient (n, d), U~ and H0 (n), and per
      workgroup slot and wave the checkpoints of every coupling layer: 256 floats per 16-wide tile of the hidden
      activations (of both hidden layers when there are two) and of the d / 16 output tiles."""
    tiles = -(-n // MFMA_CHAINS)
    slots = min(tiles, CK_MAX_GRID)
    if kernel == 'wide':
        return 4 * (n * d + (n + 3) // 4 * 4 + 3 * slots * MFMA_CHAINS * d)
    assert kernel == 'mfma', kernel
    layer_floats = ((2 if hl > 1 else 1) * (_padded_hidden(hidden) // 16) + d // 16) * 256
    return 4 * (2 * n * d + 2 * n + slots * MFMA_WAVES * cl * layer_floats)


NeutraRun = collections.namedtuple('NeutraRun', 'rc samples masks log_ratios z stats scratch_bytes')


def _direct_neutra_hmc(dev, p, f, T, L, h, seed, *, adjust=True, imd=None, step0=0, chain_offset=0, replay=None, stats=None,
                       store=None, hidden=None, prefill=None, poison=False, edit=None):
    """One nfmc_neutra_hmc_steps_f32 call of T transitions (L leapfrog steps of size h) from the latents p.x0 through
    ctypes: a NeutraRun of the return code, the kept states, the masks and log ratios (T, n) the kernel wrote, the final
    latents and the statistics, on the CPU.  The work area is sized with nfmc_neutra_scratch_bytes (scratch_bytes).
    imd: the inverse mass diagonal (d,), None: the kernels' unit diagonal.  step0, chain_offset: NfmcRng's.
    replay: (normals (T, n, d), uniforms (T, n)) in place of the Philox streams.
    stats: 'immediate' (DeviceStats.struct()) or 'deferred' (struct(defer=True), which the entry point refuses); the
      totals come back as a dict (accepted, attempted, nonfinite, sum_x, sum_x2) when the call returned 0.
    prefill: (value, count): sum_x and sum_x2 start at `value`, every counter at `count`.
    store: (thinning, max_samples) of a DeviceSampleStore of T offered transitions (kept rows in chronological order);
      None: a dense (T, n, d) store.
    hidden: the conditioner width the flow is packed to (None: neutra_presented_hidden).
    poison: the work area and the statistics scratch are filled with NaN before the launch.
    edit(args, run): spoils the arguments before the call (the refusals).  z, the mass diagonal and the work area each
      have 16 spare bytes behind them, so a pointer moved by 4 bytes stays inside its allocation."""
    from nfmc_amd import hip
    from nfmc_amd.containers import DeviceSampleStore
    n, d = p.x0.shape[0], p.d
    bij = f.bijection
    if hidden is None:
        hidden = neutra_presented_hidden(d, bij.n_hidden, bij.n_hidden_layers, bij.n_bins)
    st, _keep = bij.packed(dev, hidden)
    sbytes = int(hip.lib().nfmc_neutra_scratch_bytes(n, d, max(bij.n_hidden, hidden), int(st.n_hidden_layers), int(st.n_coupling)))
    zbuf = torch.zeros(n * d + 4, dtype=torch.float32, device=dev)
    z = zbuf[:n * d].view(n, d)
    z.copy_(p.x0.reshape(n, d).float())
    mbuf = None
    if imd is not None:
        mbuf = torch.ones(d + 4, dtype=torch.float32, device=dev)
        mbuf[:d].copy_(imd.float())
    work = torch.zeros(sbytes // 4 + 4, dtype=torch.float32, device=dev)
    masks = torch.zeros(T, n, dtype=torch.uint8, device=dev)
    lr = torch.zeros(T, n, dtype=torch.float32, device=dev)
    samples = torch.zeros(T, n, d, dtype=torch.float32, device=dev) if store is None else DeviceSampleStore(n, d, dev, T, *store)
    a = hip.NfmcNeutraHmcArgs()
    a.z, a.n, a.n_steps, a.n_leapfrog, a.step_size, a.adjust = hip.ptr(z), n, T, L, h, 1 if adjust else 0
    a.inv_mass_diag = None if mbuf is None else hip.ptr(mbuf)
    a.flow, a.pot = st, p.pot.descriptor(dev)
    keep = None
    if replay is not None:
        keep = (replay[0].float().reshape(T, n, d).to(dev).contiguous(), None if replay[1] is None else replay[1].float().to(dev).contiguous())
    a.rng = hip.make_rng(seed, chain_offset, step0, *(keep or ()))
    assert stats in (None, 'immediate', 'deferred'), stats
    acc = None
    if stats is not None:
        acc = hip.DeviceStats(d, dev)
        if prefill is not None:
            acc._buf[:2 * d].fill_(prefill[0])
            acc._buf[2 * d:].view(torch.int64).fill_(prefill[1])
        a.stats = acc.struct(defer=True, attempted=n * T) if stats == 'deferred' else acc.struct()
    if poison:
        work.fill_(float('nan'))
        if acc is not None:
            acc.scratch.fill_(float('nan'))
    a.samples = hip.store_struct(samples, T)
    a.masks_out, a.log_ratio_out = hip.ptr(masks, torch.uint8), hip.ptr(lr)
    a.scratch, a.scratch_bytes = hip.ptr(work), sbytes
    run = NeutraRun(None, samples, masks, lr, z, acc, sbytes)
    if edit is not None:
        edit(a, run)
    rc = int(hip.lib().nfmc_neutra_hmc_steps_f32(C.byref(a), hip.stream()))
    torch.cuda.synchronize()
    kept = samples.cpu() if store is None else samples.ordered().cpu().clone()
    totals = None
    if stats is not None and rc == 0:
        sum_x, sum_x2, cnt, _jc = acc.host_totals()
        totals = {'accepted': int(cnt[hip.CNT_ACCEPTED]), 'attempted': int(cnt[hip.CNT_ATTEMPTED]),
                  'nonfinite': int(cnt[hip.CNT_NONFINITE]), 'sum_x': sum_x.clone(), 'sum_x2': sum_x2.clone()}
    return NeutraRun(rc, kept, masks.cpu().bool(), lr.cpu(), z.cpu().clone(), totals, sbytes)


def neutra_hmc_oracle(p, of, T, L, h, seed, *, adjust=True, imd=None, step0=0, chain_offset=0, noise=None, dtype=torch.float64):
    """oracle.samplers.mcmc_sample on the adjusted target of the oracle flow `of` from the latents p.x0, on the Philox
    streams of `seed` (or the `noise` given).  dtype float32: the same oracle with the flow, the inputs and the noise
    cast to float32, which measures what fp32 arithmetic alone does to a trajectory (neutra_hmc_figures)."""
    from oracle import samplers as osamp
    if dtype == torch.float32:
        of = copy.deepcopy(of).float()
    if noise is None:
        noise = osamp.PhiloxNoise(seed, chain_offset, dtype=dtype)
    return osamp.mcmc_sample(p.x0.to(dtype), osamp.neutra_adjusted_target(of, p.target, (p.d,)), 'hmc', T, h,
                             None if imd is None else imd.to(dtype), L, adjust, noise, step0)


def neutra_hmc_figures(tr64, tr32):
    """(state figure, log-ratio figure): the worst difference of the kept states and of the log ratios between the fp32
    and the fp64 run of the oracle on the same inputs and noise, over the rows (transition, chain) up to and including
    a chain's first decision that differs between the two (from there they are on different trajectories).  An
    unadjusted run has no log ratios: its second figure is 0."""
    x64, x32 = tr64.stacked().double(), tr32.stacked().double()
    n = x64.shape[1]
    m64, m32 = (torch.stack([m.reshape(-1).bool() for m in t.masks]) for t in (tr64, tr32))
    same = m64 == m32
    first = torch.ones(1, n, dtype=torch.bool)
    before = torch.cumprod(torch.cat([first, same[:-1]]).int(), 0).bool()         # the transition starts from a common state
    state = float(((x64 - x32).abs().amax(2))[before & same].max())
    if not tr64.log_ratios:
        return state, 0.0
    l64, l32 = (torch.stack([v.reshape(-1).double() for v in t.log_ratios]) for t in (tr64, tr32))
    return state, float((l64 - l32).abs()[before].max())


def neutra_hmc_inputs_ok(tr, what, *, margin, lo=0.30, hi=0.95, cap=0.10):
    """What an oracle-backed NeuTra-HMC case asks of its inputs, from the fp64 oracle alone: an acceptance between lo
    and hi (both branches of the masked update run), under `cap` of the chains within `margin` (a number or (T, n):
    neutra_hmc_row_tolerance) of a tie at any transition, every log ratio finite.  Returns (acceptance, tie share)."""
    lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
    acc = tr.n_accepted / tr.n_attempted
    ties = float(((lu - lr).abs() < margin).any(0).float().mean())
    print('%s: oracle accepts %.3f, %.1f %% of the chains within %.1e of a tie, log ratios %.2f .. %.2f'
          % (what, acc, 100 * ties, float(torch.as_tensor(margin).max()), float(lr.min()), float(lr.max())))
    assert bool(torch.isfinite(lr).all()), (what, 'log ratio')
    assert lo <= acc <= hi, (what, 'acceptance', acc)
    assert ties < cap, (what, 'near-ties', ties)
    return acc, ties


class _Stacked:
    """a NeutraRun as compare_decisions reads a Record"""

    def __init__(self, run):
        self.run = run

    def stacked(self):
        return self.run.masks, self.run.log_ratios


def neutra_magnitude(p, of):
    """|U~| of a batch of latents in fp64 on the oracle flow: compare_decisions' `mag`"""
    from oracle import samplers as osamp
    adjusted = osamp.neutra_adjusted_target(of, p.ref, (p.d,))

    def mag(z):
        with torch.no_grad():
            return adjusted(z).abs()
    return mag


def neutra_hmc_row_tolerance(tr, p, of, lr_figure):
    """(T, n): compare_decisions' bound on an fp32 log ratio, 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) |U~(z)|
    at the state z each transition starts from, raised to SPLINE_C_FACTOR x lr_figure where that is larger.  It is also
    the near-tie margin of the run: a kernel whose log ratio is within this of the oracle's may decide a closer call the
    other way."""
    states = tr.stacked().double()
    prev = torch.cat([p.x0.double()[None], states[:-1]]).reshape(-1, p.d)
    lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    tol = 2e-4 * max(1.0, p.d / 64) + 1e-4 * lr.abs() + 8 * 2.0 ** -24 * neutra_magnitude(p, of)(prev).reshape(lr.shape)
    return tol.clamp_min(SPLINE_C_FACTOR * lr_figure)


def compare_neutra_hmc(run, tr, p, of, what, *, atol, lr_figure, adjust=True):
    """One launch against the oracle trace, row by row: the kept states by compare_states (tie-aware at the rows'
    tolerance neutra_hmc_row_tolerance, cap 0.10, to atol), the masks and log ratios by compare_decisions at that
    tolerance; and, what compare_decisions leaves to a share, every decision of a chain that has followed the oracle so
    far and is further than twice the row's tolerance from a tie equals the oracle's.  Returns (worst state error over
    atol, worst log-ratio error over tolerance)."""
    assert run.rc == 0, (what, run.rc)
    assert torch.equal(run.z, run.samples[-1]), what
    if not adjust:
        keep = compare_states(run.samples, tr, what, margin=0.0, atol=atol, rtol=0.0)
        compare_decisions(_Stacked(run), tr, 'uhmc', p.x0, p.ref, what)
        assert bool((run.log_ratios == 0).all()), what
        return float((run.samples.double() - tr.stacked().double()).abs().max()) / atol, 0.0
    tol = neutra_hmc_row_tolerance(tr, p, of, lr_figure)
    keep = compare_states(run.samples, tr, what, margin=tol, atol=atol, rtol=0.0)
    state_ratio = float((run.samples[:, keep].double() - tr.stacked()[:, keep].double()).abs().max()) / atol if bool(keep.any()) else 0.0
    ratio = compare_decisions(_Stacked(run), tr, 'hmc', p.x0, p.ref, what, mag=neutra_magnitude(p, of),
                              at_least=SPLINE_C_FACTOR * lr_figure)
    want_m = torch.stack([m.reshape(-1).bool() for m in tr.masks])
    want_lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    lu = torch.stack([v.reshape(-1).double() for v in tr.uniforms])
    same = run.masks == want_m
    follows = torch.cumprod(torch.cat([torch.ones(1, same.shape[1], dtype=torch.bool), same[:-1]]).int(), 0).bool()
    wrong = follows & ((lu - want_lr).abs() > 2 * tol) & ~same
    assert not bool(wrong.any()), (what, 'decisions differ on %d rows clear of a tie' % int(wrong.sum()))
    return state_ratio, ratio


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
        assert hasattr(type(q), field), field      # a name the struct lacks would set nothing and leave q well formed
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
