"""fp64 references of the split path's stand-alone kernels (csrc/misc_kernels.hip, csrc/fit_support.hip) and of the
statistics fold behind them (csrc/common.hpp).  TEST INFRASTRUCTURE: plain numpy / torch-CPU in fp64, built on `oracle/`
(the proposal and its potential, the Philox streams, the keyed permutation); nothing here touches the library.

Inputs are the fp32 values the kernels read, promoted exactly; every result is fp64.  tests/test_host_split_kernels.py
checks these references against the oracle's own transition and shows that the bounds derived from them bite;
tests/test_gpu_split_kernels.py holds the kernels against them.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import philox, shuffle  # noqa: E402,F401  (re-exported: the tests take their streams from here)
from oracle import samplers as osamp  # noqa: E402

EPS32 = 2.0 ** -24            # unit roundoff of fp32
NONFINITE_ABOVE = float(np.float32(3.0e38))   # select_kernel: non-finite when !(|lr| <= 3.0e38f), the fp32 constant
TIE_MARGIN = 2.0 ** -20       # sixteen times the ~1 ulp of log2 stated for fast_ln (csrc/common.hpp)


def _t(v):
    return torch.as_tensor(np.asarray(v, dtype=np.float64))


def _imd(imd, d):
    return torch.ones(d, dtype=torch.float64) if imd is None else _t(imd)


def h32(h):
    """The step size the kernels see: the fp32 value, as a Python float."""
    return float(np.float32(h))


# ------------------------------------------------------------------------------------------------ Langevin proposal
def propose(x, g, imd, h, z):
    """x' of oracle.samplers.langevin_propose (its grad_term / noise_term / x_prime lines) for a given gradient `g` and
    noise `z`: the oracle is run unadjusted on the linear target U(v) = sum(g v), whose autograd gradient is g itself."""
    x, g, z = _t(x), _t(g), _t(z)
    xp, _, _, _ = osamp.langevin_propose(x, lambda v: (g * v).sum(-1), h32(h), _imd(imd, x.shape[1]), False,
                                         osamp.ReplayNoise([z], []), 0)
    return xp.numpy()


def propose_size(x, g, imd, h, z):
    """|x| + |h g / m^2| + |sqrt(2h) z / m| per element: what the proposal's roundings are relative to."""
    x, g, z = (np.asarray(v, dtype=np.float64) for v in (x, g, z))
    m = np.ones(x.shape[1]) if imd is None else np.asarray(imd, dtype=np.float64)
    h = h32(h)
    return np.abs(x) + np.abs(h * g / (m * m)) + np.abs(math.sqrt(2 * h) * z / m)


def propose_bound(x, g, imd, h, z, native=False):
    """8 * 2^-24 * propose_size: the kernel rounds sqrt(2h), its quotient by m, m*m, -h / (m*m) and two fmas, six
    roundings, each relative to a partial result no larger than propose_size.  `native`: the kernel's own normals are
    within 4e-6 of oracle.philox.normal_field (hardware transcendentals), scaled by sqrt(2h) / m."""
    b = 8 * EPS32 * propose_size(x, g, imd, h, z)
    if native:
        m = np.ones(np.asarray(x).shape[1]) if imd is None else np.asarray(imd, dtype=np.float64)
        b = b + 4e-6 * math.sqrt(2 * h32(h)) / m
    return b


# ------------------------------------------------------------------------------------------------ Langevin log ratio
def log_ratio(x, xp, u, up, g, gp, imd, h, drop_last=False):
    """(u - u') - proposal_potential(x, x', g', A, h) + proposal_potential(x', x, g, A, h), A = 1 / imd^2
    (oracle.samplers.langevin_propose's log_ratio).  drop_last: without the last coordinate's term (bite checks)."""
    x, xp, u, up, g, gp = (_t(v) for v in (x, xp, u, up, g, gp))
    a = 1 / _imd(imd, x.shape[1]) ** 2
    if drop_last:
        x, xp, g, gp, a = x[:, :-1], xp[:, :-1], g[:, :-1], gp[:, :-1], a[:-1]
    h = h32(h)
    out = (u - up) - osamp.proposal_potential(x, xp, gp, a, h) + osamp.proposal_potential(xp, x, g, a, h)
    return out.numpy()


def log_ratio_size(x, xp, u, up, g, gp, imd, h):
    """S = |u| + |u'| + sum_c m_c^2 / (4h) [(|x' - x| + |h A g|)^2 + (|x - x'| + |h A g'|)^2]: the log ratio's sums with
    every difference replaced by the sum of absolute values."""
    x, xp, u, up, g, gp = (np.asarray(v, dtype=np.float64) for v in (x, xp, u, up, g, gp))
    m = np.ones(x.shape[1]) if imd is None else np.asarray(imd, dtype=np.float64)
    h = h32(h)
    a = 1 / (m * m)
    dx = np.abs(xp - x)
    terms = (dx + np.abs(h * a * g)) ** 2 + (dx + np.abs(h * a * gp)) ** 2
    return np.abs(u) + np.abs(up) + (m * m / (4 * h) * terms).sum(-1)


def log_ratio_gamma(d):
    """(ceil(d / 64) + 20) * 2^-24: the longest add chain of the kernel's strided sum (ceil(d/64) per lane, six butterfly
    steps, the final u - u' + acc) plus the roundings inside one term."""
    return (-(-d // 64) + 20) * EPS32


def log_ratio_kernel_order_f32(x, xp, u, up, g, gp, imd, h):
    """fp32 emulation of langevin_log_ratio_kernel in its own order: lane c % 64 adds the terms of coordinates c, c + 64,
    ..., then the 64-lane xor butterfly, then (u - u') + acc; every operation in np.float32."""
    f = np.float32
    x, xp, u, up, g, gp = (np.asarray(v, dtype=f) for v in (x, xp, u, up, g, gp))
    n, d = x.shape
    m = np.ones(d, dtype=f) if imd is None else np.asarray(imd, dtype=f)
    h = f(h)
    inv4h = f(1) / (f(4) * h)
    a = f(1) / (m * m)
    tf = (xp - x) + h * a * g
    tb = (x - xp) + h * a * gp
    term = inv4h * (f(1) / a) * (tf * tf - tb * tb)
    lanes = np.zeros((n, 64), dtype=f)
    for c0 in range(0, d, 64):
        w = min(64, d - c0)
        lanes[:, :w] = lanes[:, :w] + term[:, c0:c0 + w]
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, idx ^ s]
    return (u - up) + lanes[:, 0]


# ------------------------------------------------------------------------------------------------ K6: accept / select
def log_uniform(u):
    return np.log(np.asarray(u, dtype=np.float64))


def near_tie(lr, u):
    """Rows whose decision the kernel's log(u) may flip: |lr - log u| < 2^-20 max(1, |log u|) in fp64."""
    lu = log_uniform(u)
    with np.errstate(invalid='ignore'):
        return np.abs(np.asarray(lr, dtype=np.float64) - lu) < TIE_MARGIN * np.maximum(1.0, np.abs(lu))


def select(x, xp, lr, u, carries=(), carries_prime=(), copy_carries=None):
    """select_kernel's rule: accept iff log(u) < lr (NaN rejects); lr = None accepts every row and counts nothing
    non-finite; non-finite means !(|lr| <= 3e38).  Returns (new x, new carries, mask, n_accepted, n_nonfinite).
    copy_carries: how many of the carries an accepted row copies (default all; the bite check passes fewer)."""
    x, xp = np.asarray(x), np.asarray(xp)
    n = x.shape[0]
    if lr is None:
        mask, bad = np.ones(n, dtype=bool), 0
    else:
        lr64 = np.asarray(lr, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            mask = log_uniform(u) < lr64
            bad = int((~(np.abs(lr64) <= NONFINITE_ABOVE)).sum())
    new_x = np.where(mask[:, None], xp, x)
    k = len(carries) if copy_carries is None else copy_carries
    new_c = [np.where(mask, cp, c) if i < k else np.array(c) for i, (c, cp) in enumerate(zip(carries, carries_prime))]
    return new_x, new_c, mask, int(mask.sum()), bad


# ------------------------------------------------------------------------------------------------ moments
def moments(x):
    """fp64 sum of x and of x^2 over the rows, of the fp32 values."""
    x = np.asarray(x, dtype=np.float64)
    return x.sum(0), (x * x).sum(0)


def moments_fp32sq(x):
    """The same with each square rounded to fp32 first: what K6's fmaf(x, x, 0) holds before it is widened."""
    x = np.asarray(x, dtype=np.float32)
    return x.astype(np.float64).sum(0), (x * x).astype(np.float64).sum(0)


def abs_moments(x):
    """sum |x| and sum x^2 per coordinate: what the statistics' roundings are relative to."""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x).sum(0), (x * x).sum(0)


# ------------------------------------------------------------------------------------------------ K6 layouts
def padded_d(d):
    p = 4
    while p < d:
        p <<= 1
    return p


def select_layout(d):
    """(CPL, LPC, rows per tile) of the select_kernel instantiation that serves event size d (misc_kernels.hip:
    nfmc_mh_accept_select_f32): CPL = 4 with LPC = padded_d / 4 up to d = 256, then LPC = 64 with CPL = 8, 16."""
    dp = padded_d(d)
    lpc = min(64, dp // 4)
    return dp // lpc, lpc, 4 * (64 // lpc)


# ------------------------------------------------------------------------------------------------ shared test inputs
LOG_RATIO_DS = (1, 7, 63, 64, 65, 128, 257, 1000, 1024)
LOG_RATIO_HS = (1e-4, 1e-2, 0.5)
BITE_H = 1e-2     # the listed step size at which ONE coordinate's term stands clear of every row's tolerance at every d
                  # (bite checks): at h = 0.5 the proposal overshoots U = |x|^2, |log ratio| and S grow to ~1e4 at
                  # d = 1024, and a single term of O(1) is then below 2^-24 S by right, not by a weak test


def _away_from_zero(v):
    """sign(v) (0.5 + |v|) on the last coordinate: a draw that happens to be ~0 there would make that coordinate's term
    vanish, and a kernel that dropped it could then not be told from a right one on that row."""
    v = v.clone()
    last = v[:, -1]
    v[:, -1] = torch.where(last < 0, -(0.5 + last.abs()), 0.5 + last.abs())
    return v


def mass_vector(d, gen):
    """inv_mass_diag drawn from exp(U(-1, 1)), fp32."""
    return torch.exp(2 * torch.rand(d, generator=gen) - 1).float().numpy()


def log_ratio_inputs(n, d, h, mass, offset, family, seed):
    """fp32 inputs of one log-ratio case, as numpy arrays (x, xp, u, up, g, gp, imd).
    family 'mala': U = |x - offset|^2 (g = 2 (x - offset)), x' from the proposal reference rounded to fp32, so that
    tf = (x' - x) + h A g is the cancelled noise term; 'independent': x, x', g, g' drawn independently."""
    gen = torch.Generator().manual_seed(seed)
    imd = mass_vector(d, gen) if mass else None
    c = _away_from_zero(torch.randn(n, d, generator=gen))
    x = (c + offset).float().numpy()
    if family == 'mala':
        z = _away_from_zero(torch.randn(n, d, generator=gen)).float().numpy()
        g = (np.float32(2) * (x - np.float32(offset))).astype(np.float32)
        xp = propose(x, g, imd, h, z).astype(np.float32)
        gp = (np.float32(2) * (xp - np.float32(offset))).astype(np.float32)
    else:
        xp = (torch.randn(n, d, generator=gen) + offset).float().numpy()
        g = torch.randn(n, d, generator=gen).float().numpy()
        gp = torch.randn(n, d, generator=gen).float().numpy()
    u = (d + 10 * torch.randn(n, generator=gen)).float().numpy()
    up = (torch.from_numpy(u) + torch.randn(n, generator=gen)).float().numpy()
    return x, xp, u, up, g, gp, imd


def replay_uniforms(n, gen):
    """fp32 uniforms of the kernels' own form, (2 k + 1) 2^-24 with 23 random bits: never 0 or 1."""
    k = torch.randint(0, 1 << 23, (n,), generator=gen, dtype=torch.int64)
    return ((2 * k + 1).double() * 2.0 ** -24).float().numpy()


def select_inputs(n, d, seed, offset=100.0, n_carry=2):
    """fp32 inputs of one K6 case: x, x' offset by `offset` (cancellation in the moments would show), lr ~ N(-0.7, 1.5),
    independent uniforms, carries and their primed values."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, d, generator=gen) + offset).float().numpy()
    xp = (torch.randn(n, d, generator=gen) + offset).float().numpy()
    lr = (-0.7 + 1.5 * torch.randn(n, generator=gen)).float().numpy()
    u = replay_uniforms(n, gen)
    carries = [torch.randn(n, generator=gen).float().numpy() for _ in range(n_carry)]
    primes = [torch.randn(n, generator=gen).float().numpy() for _ in range(n_carry)]
    return x, xp, lr, u, carries, primes
