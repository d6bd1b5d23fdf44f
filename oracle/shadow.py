"""Shadowing: a kernel's run checked transition by transition against an fp64 oracle.  TEST INFRASTRUCTURE.

A whole-run comparison of two Markov chain implementations stops meaning anything after a few transitions: one accept
test that lands within rounding of a tie sends the two chains apart, and chaotic dynamics (long leapfrog trajectories,
a funnel) amplify every rounding difference.  Shadowing avoids both.  For each transition t the oracle restarts from
the KERNEL's own state before t, S[t], and recomputes that single transition in fp64 with the same Philox step and
tags; its result is compared with the kernel's state after t, S[t + 1].  Errors do not compound, so a run can be as
long as needed, and the tolerance is tied to fp32 rounding: the same transition through the fp32 oracle, from the same
pre-states, measures what fp32 arithmetic alone costs (e32); the kernel may lose at most a factor kappa more.

The Philox normals and uniforms are the fp32 values of oracle/philox.py (promoted exactly to fp64 for the fp64 run):
they are the kernel's inputs, not part of the arithmetic under test.

Checks (`ShadowReport.failures`):
  decisions  a kernel accept is a row that changed, a reject a row bitwise equal to its pre-state.  Every chain whose fp64
             margin m = log_alpha - log_u is clear of the tie window makes the fp64 decision.  The window is
                 delta = max(tie_coef * (1 + scale), tie_kappa * |m32 - m64|)
             with scale = |H0| + |H1| for HMC (Hamiltonians), |U0| + |U1| for MALA, |U| + |log q| of both points for
             flow-proposal MH and IMH, and m32 the fp32 oracle's margin of the same transition: a trajectory that
             amplifies rounding (a funnel chain thrown far out) widens its own window by what fp32 arithmetic does to it.
             Near ties are skipped and counted; at most `max_tie_share` of them.  The chains that part from the oracle at
             all must not be periodic in the row index (a layout bug hits one lane group).
  states     on the transitions that the kernel, the fp64 and the fp32 oracle all accept, per chain
             e = max_j |S[t + 1] - x64|, e32 = max_j |x32 - x64|, and per transition
                 max e  <= kappa * max e32 + 1e-6 * (1 + max |x64|)
                 mean e <= kappa / 2 * mean e32 + 1e-7
"""
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import torch

from . import samplers as osamp

KINDS = ('mala', 'hmc', 'neutra_hmc', 'jump_mala', 'jump_hmc', 'imh', 'ula', 'uhmc', 'mh')
UNADJUSTED_MARGIN = 1e30     # margin of an unadjusted transition: every chain accepts, far from any tie


@dataclass
class Workload:
    """What the kernel ran.  `target`: an oracle potential (n, d) -> (n,) that works in fp32 and fp64 (oracle/potentials.py);
    `flow`: the oracle flow with the kernel's weights (the harness makes its own fp64 copy); jump runs number their
    transitions i * (n_inner + 1) + k and jump at k = n_inner; run transition t draws at Philox step step0 + t.
    `step_size` and `inv_mass_diag` may also be sequences indexed by run transition t (a warmup: what the controller had
    set before t, oracle.samplers.replay_controller); `inv_mass_diag` is then a list of (d,) tensors or a (T, d) tensor.
    `ula` / `uhmc` accept every proposal; `mh` is the random-walk proposal x + inv_mass_diag * eps (mh.py:44-73)."""
    kind: str
    target: Callable
    flow: Optional[object] = None
    step_size: Optional[float] = None
    n_leapfrog: int = 1
    n_inner: int = 0
    inv_mass_diag: Optional[torch.Tensor] = None
    step0: int = 0

    def __post_init__(self):
        assert self.kind in KINDS, self.kind

    def h_at(self, step):
        h = self.step_size
        return float(h[step - self.step0]) if isinstance(h, (list, tuple, torch.Tensor, np.ndarray)) else h

    def imd_at(self, step, d, dtype):
        m = self.inv_mass_diag
        if m is None:
            return torch.ones(d, dtype=dtype)
        if isinstance(m, (list, tuple)) or (isinstance(m, torch.Tensor) and m.dim() == 2):
            m = m[step - self.step0]
        return torch.as_tensor(m).to(dtype).reshape(d)

    def is_jump(self, step):
        return self.kind == 'imh' or (self.kind.startswith('jump') and step % (self.n_inner + 1) == self.n_inner)


@dataclass
class Transition:
    """What one call of `one_transition` computed."""
    x: torch.Tensor              # post-state (n, d)
    mask: torch.Tensor           # accepted
    margin: torch.Tensor         # log_alpha - log_u
    scale: torch.Tensor          # magnitude of the terms of log_alpha (tie window)


def one_transition(wl: Workload, x, step, noise, flow, target):
    """Transition `step` of workload `wl` from the states x (n, d), in the dtype of x / flow / noise."""
    n, d = x.shape
    imd = wl.imd_at(step, d, x.dtype)
    h = wl.h_at(step)
    if wl.is_jump(step):
        js = osamp.jump_transition(x, target, flow, step, noise)
        scale = js.u_x.abs() + js.u_xp.abs() + js.f_x.abs() + js.f_xp.abs()
        return Transition(js.x, js.mask, js.log_alpha - js.log_u, scale)
    info = {}
    if wl.kind in ('ula', 'uhmc'):
        if wl.kind == 'ula':
            xp, mask, _lr, _lu = osamp.langevin_propose(x, target, h, imd, False, noise, step)
        else:
            xp, mask, _lr, _lu = osamp.hmc_propose(x, target, h, imd, wl.n_leapfrog, False, noise, step)
        return Transition(xp.detach().clone(), mask, torch.full((n,), UNADJUSTED_MARGIN, dtype=torch.float64),
                          torch.zeros(n, dtype=torch.float64))
    if wl.kind == 'mh':
        xp, mask, lr, lu = osamp.mh_propose(x, target, imd, True, noise, step)
        scale = target(x).abs() + target(xp).abs()
    elif wl.kind in ('mala', 'jump_mala'):
        xp, mask, lr, lu = osamp.langevin_propose(x, target, h, imd, True, noise, step, info)
        scale = info['u0'].abs() + info['u1'].abs()
    else:
        if wl.kind == 'neutra_hmc':
            target = osamp.neutra_adjusted_target(flow, target, tuple(flow.event_shape))
        xp, mask, lr, lu = osamp.hmc_propose(x, target, h, imd, wl.n_leapfrog, True, noise, step, info)
        scale = info['h0'].abs() + info['h1'].abs()
    xn = x.clone()
    xn[mask] = xp.detach()[mask]
    return Transition(xn, mask, (lr - lu).detach(), scale.detach())


def _fp64(flow):
    import copy
    return copy.deepcopy(flow).double() if flow is not None else None


def periodic_rows(bad, periods=(2, 4, 8, 16, 32, 64)):
    """The first period in which the rows `bad` crowd into one residue class, or None.  A near-tie flip hits a random chain,
    a layout bug is periodic in the row index (rows of one lane group of a wave are congruent modulo 64 / LPC, of one wave
    slot modulo the rows per workgroup): random rows fill the fullest of `period` classes with about len/period of them."""
    if len(bad) < 6:
        return None
    for period in periods:
        counts = np.bincount(np.asarray(bad) % period, minlength=period)
        if counts.max() > max(3, int(np.ceil(len(bad) * (1.0 / period + 0.45)))):
            return period, counts.tolist()
    return None


def calibrated(e, e32, floor_max, floor_mean, kappa):
    """The two kappa bounds on per-chain errors e against the fp32 yardstick e32: (ok_max, ok_mean, kappa needed by the
    max bound, kappa needed by the mean bound)."""
    e, e32 = np.asarray(e, dtype=np.float64), np.asarray(e32, dtype=np.float64)
    if e.size == 0:
        return True, True, 0.0, 0.0
    mx, mx32, mn, mn32 = e.max(), e32.max(), e.mean(), e32.mean()
    need_max = max(mx - floor_max, 0.0) / mx32 if mx32 > 0 else (math.inf if mx > floor_max else 0.0)
    need_mean = 2 * max(mn - floor_mean, 0.0) / mn32 if mn32 > 0 else (math.inf if mn > floor_mean else 0.0)
    return mx <= kappa * mx32 + floor_max, mn <= kappa / 2 * mn32 + floor_mean, need_max, need_mean


@dataclass
class ShadowReport:
    n_chains: int
    n_transitions: int = 0
    n_ties: int = 0
    accepted_inner: int = 0        # kernel rows that changed, inner transitions
    accepted_jumps: int = 0        # ... jumps (flow-proposal MH, IMH)
    attempted_inner: int = 0
    attempted_jumps: int = 0
    mismatches: List[tuple] = field(default_factory=list)     # (t, chain, margin, delta, kernel_accepted)
    parted: set = field(default_factory=set)                  # chains that differ from the fp64 decision at least once
    err: List[tuple] = field(default_factory=list)            # per transition (t, e, e32, max|x64|, chains, worst (chain, coord))
    rounding: float = 0.0          # max |m32 - m64| / (1 + scale): the fp32 rounding of the margin, in units of the tie window

    def kappa_needed(self):
        """The smallest kappa that passes the max and the mean state bound on every transition."""
        km = kn = 0.0
        for _t, e, e32, xmax, _c, _w in self.err:
            _a, _b, m, n = calibrated(e, e32, 1e-6 * (1 + xmax), 1e-7, math.inf)
            km, kn = max(km, m), max(kn, n)
        return km, kn

    def ratios(self):
        """Observed max e / max e32 and mean e / mean e32 (worst transition; transitions without an fp32 error skipped)."""
        rm = rn = 0.0
        for _t, e, e32, _x, _c, _w in self.err:
            if len(e) and e32.max() > 0:
                rm = max(rm, float(e.max() / e32.max()))
            if len(e) and e32.mean() > 0:
                rn = max(rn, float(e.mean() / e32.mean()))
        return rm, rn

    @property
    def tie_share(self):
        return self.n_ties / max(1, self.n_chains * self.n_transitions)

    def acceptance(self):
        return (self.accepted_inner / max(1, self.attempted_inner), self.accepted_jumps / max(1, self.attempted_jumps))

    def failures(self, kappa, max_tie_share=0.01):
        out = []
        if self.mismatches:
            t, c, m, dl, k = self.mismatches[0]
            out.append('%d clear-margin decisions differ from fp64; first: transition %d chain %d margin %.3g (delta %.3g) '
                       'kernel %s' % (len(self.mismatches), t, c, m, dl, 'accepted' if k else 'rejected'))
        if self.tie_share > max_tie_share:
            out.append('near-tie share %.4f > %.4f' % (self.tie_share, max_tie_share))
        per = periodic_rows(sorted(self.parted))
        if per is not None:
            out.append('chains that part from fp64 are periodic in the row index: period %d, classes %s' % per)
        for t, e, e32, xmax, chains, worst in self.err:
            ok_max, ok_mean, _m, _n = calibrated(e, e32, 1e-6 * (1 + xmax), 1e-7, kappa)
            if not (ok_max and ok_mean):
                i = int(np.argmax(e))
                out.append('states at transition %d: max e %.3g vs max e32 %.3g, mean e %.3g vs mean e32 %.3g (kappa %g); '
                           'worst chain %d coordinate %d' % (t, e.max(), e32.max(), e.mean(), e32.mean(), kappa,
                                                             int(chains[i]), int(worst[i])))
                break
        return out

    def summary(self):
        rm, rn = self.ratios()
        km, kn = self.kappa_needed()
        acc_inner, acc_jump = self.acceptance()
        return {'transitions': self.n_transitions, 'chains': self.n_chains, 'ratio_max': rm, 'ratio_mean': rn,
                'kappa_needed_max': km, 'kappa_needed_mean': kn, 'tie_share': self.tie_share,
                'acceptance_inner': acc_inner, 'acceptance_jump': acc_jump, 'margin_rounding': self.rounding,
                'clear_mismatches': len(self.mismatches)}


class _SharedDraws:
    """The fp32 Philox draws of one transition, computed once for the fp32 and the fp64 oracle (promoted for the latter)."""

    def __init__(self, inner, dtype=None, memo=None):
        self.inner, self.dtype, self.memo = inner, dtype, memo if memo is not None else {}

    def _get(self, key, fn):
        if key not in self.memo:
            if len(self.memo) > 8:     # the draws of earlier transitions
                self.memo.clear()
            self.memo[key] = fn()
        v = self.memo[key]
        return v.clone() if self.dtype is None else v.to(self.dtype)

    def normal(self, n, shape, step, tag):
        return self._get(('n', n, tuple(shape), step, tag), lambda: self.inner.normal(n, shape, step, tag))

    def uniform(self, n, step, tag):
        return self._get(('u', n, step, tag), lambda: self.inner.uniform(n, step, tag))


def shadow(states, wl: Workload, seed, chain_offset=0, rounds=10, tie_coef=1e-5, tie_kappa=8.0) -> ShadowReport:
    """Shadow the kernel's kept states `states` (T + 1, n, d): states[0] = x0, states[t + 1] = the state after run
    transition t (Philox step wl.step0 + t)."""
    states = states.detach().cpu().float()
    T1, n, d = states.shape
    flow32, flow64 = wl.flow, _fp64(wl.flow)
    philox32 = osamp.PhiloxNoise(seed, chain_offset, rounds)
    memo = {}
    noise32 = _SharedDraws(philox32, None, memo)
    noise64 = _SharedDraws(philox32, torch.float64, memo)
    rep = ShadowReport(n_chains=n)
    for t in range(T1 - 1):
        step = wl.step0 + t
        pre, post = states[t], states[t + 1]
        r64 = one_transition(wl, pre.double(), step, noise64, flow64, wl.target)
        r32 = one_transition(wl, pre.clone(), step, noise32, flow32, wl.target)
        kacc = (post != pre).any(dim=1)
        delta = torch.maximum(tie_coef * (1 + r64.scale), tie_kappa * (r32.margin.double() - r64.margin).abs())
        clear = r64.margin.abs() > delta
        rep.n_ties += int((~clear).sum())
        rep.rounding = max(rep.rounding, float(((r32.margin.double() - r64.margin).abs() / (1 + r64.scale)).max()))
        bad = clear & (kacc != r64.mask)
        for c in bad.nonzero().flatten().tolist():
            rep.mismatches.append((t, c, float(r64.margin[c]), float(delta[c]), bool(kacc[c])))
        rep.parted.update((kacc != r64.mask).nonzero().flatten().tolist())
        if wl.is_jump(step):
            rep.accepted_jumps += int(kacc.sum())
            rep.attempted_jumps += n
        else:
            rep.accepted_inner += int(kacc.sum())
            rep.attempted_inner += n
        both = (kacc & r64.mask & r32.mask).nonzero().flatten()
        diff = (post[both].double() - r64.x[both]).abs()
        e = diff.amax(dim=1).numpy() if len(both) else np.zeros(0)
        worst = diff.argmax(dim=1).numpy() if len(both) else np.zeros(0, dtype=np.int64)
        e32 = (r32.x[both].double() - r64.x[both]).abs().amax(dim=1).numpy() if len(both) else np.zeros(0)
        xmax = float(r64.x[both].abs().max()) if len(both) else 0.0
        rep.err.append((t, e, e32, xmax, both.numpy(), worst))
        rep.n_transitions += 1
    return rep
