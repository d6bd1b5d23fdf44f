"""References for the mclmc sampler (microcanonical Langevin Monte Carlo; include/nfmc_hip.h, NfmcMclmcArgs).  No tests
in here.

  steps          T steps B(eps/2) A(eps) B(eps/2) O from (x0, u0) in `dtype` (fp64: the reference; fp32: what fp32 arithmetic
                 alone costs), noise from oracle.samplers.PhiloxNoise on the stream the launches draw from
  free_run       a whole adaptive warmup on the CPU: the reference of the behaviour tests
  replay_update  one controller update recomputed from an update's recorded dE and kept states
  quadratic / funnel   the two closed-form targets in the dtype of their argument
"""
import math

import numpy as np
import torch

from nfmc_amd.tuning import MicrocanonicalAdaptation
from oracle import samplers as osamp

TAG_NOISE, TAG_VELOCITY = 0, 4
LN2 = math.log(2.0)


def quadratic(a, b):
    """U(x) = sum a (x - b)^2 in the dtype of x"""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)

    def u(x):
        return (a.to(x.dtype) * (x - b.to(x.dtype)) ** 2).sum(-1)
    return u


def funnel(scale=3.0):
    """Neal's funnel in the dtype of x"""
    def u(x):
        x0 = x[:, 0]
        return x0 ** 2 / (2 * scale ** 2) + 0.5 * torch.exp(-x0) * (x[:, 1:] ** 2).sum(-1) + 0.5 * (x.shape[1] - 1) * x0
    return u


def value_and_grad(target, x):
    """(U, grad U) of the rows of x, both in the dtype of x (a restatement that computes in fp64 is rounded to it)"""
    with torch.enable_grad():
        xr = x.detach().clone().requires_grad_(True)
        u = target(xr)
        g, = torch.autograd.grad(u.sum(), xr)
    return u.detach().reshape(-1).to(x.dtype), g.detach().reshape(x.shape).to(x.dtype)


def kick(u, g, sigma, e, d):
    """B(e): (new unit velocity, dK) per chain"""
    gt = sigma * g
    gn = torch.sqrt((gt * gt).sum(1))
    still = gn == 0
    e_hat = -gt / torch.where(still, torch.ones_like(gn), gn)[:, None]
    ue = (u * e_hat).sum(1)
    delta = e * gn / (d - 1)
    zeta = torch.exp(-delta)
    uu = e_hat * ((1 - zeta) * (1 + zeta + ue * (1 - zeta)))[:, None] + 2 * zeta[:, None] * u
    un = uu / torch.sqrt((uu * uu).sum(1, keepdim=True))
    dk = (d - 1) * (delta - LN2 + torch.log(1 + ue + (1 - ue) * zeta ** 2))
    return torch.where(still[:, None], u, un), torch.where(still, torch.zeros_like(dk), dk)


def f32(v):
    return float(np.float32(v))


def initial_velocity(n, d, seed, k0, dtype=torch.float64, chain_offset=0):
    """normals of Philox stream 4 at step counter k0, normalised"""
    z = osamp.PhiloxNoise(seed, chain_offset=chain_offset, dtype=torch.float64).normal(n, (d,), k0, TAG_VELOCITY)
    return (z / z.norm(dim=1, keepdim=True)).to(dtype)


def steps(target, x0, u0, eps, L, imd, seed, k0, T, dtype=torch.float64, chain_offset=0):
    """(states (T, n, d), velocities (T, n, d), dE (T, n), taken (T, n) bool) of T steps from (x0, u0) at Philox step
    counters k0 .. k0 + T - 1.  eps and L are rounded to fp32 first, as the kernels integrate with them."""
    x, u = x0.to(dtype), u0.to(dtype)
    n, d = x.shape
    eps, L = f32(eps), f32(L)
    sigma = (torch.ones(d, dtype=torch.float64) if imd is None else torch.as_tensor(imd).double()).to(dtype).sqrt()[None]
    nu = math.sqrt(math.expm1(2.0 * eps / L) / d)
    noise = osamp.PhiloxNoise(seed, chain_offset=chain_offset, dtype=dtype)
    U, g = value_and_grad(target, x)
    xs, us, des, oks = [], [], [], []
    for s in range(T):
        u1, dk1 = kick(u, g, sigma, eps / 2, d)
        xn = x + eps * sigma * u1
        Un, gn = value_and_grad(target, xn)
        u2, dk2 = kick(u1, gn, sigma, eps / 2, d)
        de = (Un - U) + dk1 + dk2
        ok = torch.isfinite(de) & torch.isfinite(xn).all(1)
        x = torch.where(ok[:, None], xn, x)
        g, U = torch.where(ok[:, None], gn, g), torch.where(ok, Un, U)
        w = torch.where(ok[:, None], u2, u) + nu * noise.normal(n, (d,), (k0 + s) & 0xffffffff, TAG_NOISE)
        u = w / torch.sqrt((w * w).sum(1, keepdim=True))
        xs.append(x), us.append(u), des.append(de), oks.append(ok)
    return torch.stack(xs), torch.stack(us), torch.stack(des), torch.stack(oks)


def controller(eps, L, imd, d, **kw):
    return MicrocanonicalAdaptation(eps, L, torch.ones(d) if imd is None else imd, d, **kw)


def replay_update(de, states, eps, L, imd, dtype=torch.float64, **kw):
    """One controller update from the update's recorded dE (k, n) and kept states (k, n, d), sums and variance taken in
    `dtype`: the MicrocanonicalAdaptation after its step (step_size, decoherence_length, inv_mass_diag, energy_variance)."""
    de, states = torch.as_tensor(de).to(dtype), torch.as_tensor(states).to(dtype)
    d = states.shape[-1]
    ok = torch.isfinite(de)
    dee = torch.where(ok, de, torch.zeros_like(de))
    rows = states.reshape(-1, d)
    var = rows.var(0, unbiased=True).double() if rows.shape[0] > 1 else None
    ctl = controller(eps, L, imd, d, **kw)
    ctl.step(float((dee * dee).sum()), float(ok.sum()), var)
    return ctl


def free_run(target, x0, eps, L, imd, seed, k0, W, every, dtype=torch.float64, u0=None, **kw):
    """An adaptive warmup of W steps with one update per `every`: (controller, final x, final u)."""
    n, d = x0.shape
    u = initial_velocity(n, d, seed, k0, dtype) if u0 is None else u0.to(dtype)
    x = x0.to(dtype)
    ctl = controller(eps, L, imd, d, **kw)
    done = 0
    while done < W:
        k = min(every, W - done)
        xs, us, de, ok = steps(target, x, u, ctl.step_size, ctl.decoherence_length, ctl.inv_mass_diag, seed, k0 + done, k, dtype)
        dee = torch.where(ok, de, torch.zeros_like(de)).double()
        rows = xs.reshape(-1, d).double()
        ctl.step(float((dee * dee).sum()), float(ok.sum()), rows.var(0, unbiased=True) if rows.shape[0] > 1 else None)
        x, u = xs[-1], us[-1]
        done += k
    return ctl, x, u
