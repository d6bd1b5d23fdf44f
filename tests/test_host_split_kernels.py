"""Host: the fp64 references of tests/split_fp64.py are themselves right, and the bounds the GPU tests derive from them
are neither vacuous nor tight by luck.  No GPU, no library.

- `propose` / `log_ratio` against oracle.samplers.langevin_propose on a quadratic target (fp64, ReplayNoise);
- `select` against the accept step of oracle.samplers.mcmc_sample on the golden mala_d6 fixture;
- the log-ratio bound (ceil(d/64) + 20) 2^-24 S on an fp32 emulation of the kernel's own summation order;
- bite checks: a dropped last coordinate, g in place of g', a carry that is not copied.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import split_fp64 as ref  # noqa: E402
from oracle import potentials as opot  # noqa: E402
from oracle import samplers as osamp  # noqa: E402


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize('mass', [False, True])
def test_propose_and_log_ratio_equal_the_oracle_transition(mass):
    """One fp64 oracle transition on U = |x|^2 with replayed noise: `propose` gives its x_prime, `log_ratio` its
    log_ratio, to 1e-12."""
    n, d, h = 40, 9, 0.05
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(n, d, generator=gen).float().double()
    z = torch.randn(n, d, generator=gen).float().double()
    un = torch.rand(n, generator=gen).double()
    imd = torch.from_numpy(ref.mass_vector(d, gen)).double() if mass else torch.ones(d, dtype=torch.float64)
    info = {}
    xp, _, lr, _ = osamp.langevin_propose(x, opot.sum_squares, ref.h32(h), imd, True, osamp.ReplayNoise([z], [un]), 0,
                                          info=info)
    g, gp = 2 * x, 2 * xp          # grad of sum_squares
    assert torch.equal(osamp._value_and_grad(opot.sum_squares, x)[1], g)
    imd_np = imd.numpy() if mass else None
    got_xp = ref.propose(x.numpy(), g.numpy(), imd_np, h, z.numpy())
    np.testing.assert_allclose(got_xp, xp.numpy(), atol=1e-12, rtol=0)
    got_lr = ref.log_ratio(x.numpy(), xp.numpy(), info['u0'].numpy(), info['u1'].numpy(), g.numpy(), gp.numpy(), imd_np, h)
    np.testing.assert_allclose(got_lr, lr.numpy(), atol=1e-12, rtol=0)
    # and the size the tolerance is a multiple of dominates the ratio itself
    s = ref.log_ratio_size(x.numpy(), xp.numpy(), info['u0'].numpy(), info['u1'].numpy(), g.numpy(), gp.numpy(), imd_np, h)
    assert (np.abs(got_lr) <= s).all()


def test_select_equals_the_oracle_accept_step_on_the_golden_fixture():
    """Every transition of the golden mala_d6 run: `select` on (x, x', log ratio, the fixture's uniforms) gives the
    oracle's mask and next state bit for bit."""
    fx = load_golden('mala_d6')
    h, imd = float(fx['step_size']), torch.from_numpy(fx['inv_mass_diag'])
    noise = osamp.ReplayNoise([torch.from_numpy(v) for v in fx['noise/normals']],
                              [torch.from_numpy(v) for v in fx['noise/uniforms']])
    x = torch.from_numpy(fx['x0']).clone()
    n_acc = 0
    for step in range(fx['exp/samples'].shape[0]):
        xp, mask, lr, _ = osamp.langevin_propose(x, opot.sum_squares, h, imd, True, noise, step)
        u = fx['noise/uniforms'][step]
        assert not ref.near_tie(lr.numpy(), u).any()
        new_x, _, got_mask, acc, bad = ref.select(x.numpy(), xp.numpy(), lr.numpy(), u)
        np.testing.assert_array_equal(got_mask, mask.numpy())
        x = x.clone()
        x[mask] = xp[mask]                                  # mcmc_sample's accept step
        assert new_x.dtype == np.float32 and new_x.tobytes() == x.numpy().tobytes()
        np.testing.assert_allclose(new_x, fx['exp/samples'][step], atol=2e-6, rtol=0)
        assert bad == 0
        n_acc += acc
    assert n_acc == int(fx['exp/counters'][0])


def test_select_edge_rules():
    """+inf accepts and counts, -inf and NaN reject and count, 3.0e38 is finite, NULL ratio accepts all, counts none."""
    lr = np.array([np.inf, -np.inf, np.nan, 0.0, 3.0e38, -3.0e38], dtype=np.float32)
    u = np.full(6, 0.5, dtype=np.float32)
    x, xp = np.zeros((6, 2), dtype=np.float32), np.ones((6, 2), dtype=np.float32)
    _, _, mask, acc, bad = ref.select(x, xp, lr, u)
    assert mask.tolist() == [True, False, False, True, True, False] and acc == 3 and bad == 3
    new_x, _, mask, acc, bad = ref.select(x, xp, None, None)
    assert mask.all() and acc == 6 and bad == 0 and (new_x == xp).all()


# ------------------------------------------------------------------------------------------------ the bound
CASES = [(d, h, mass, offset) for d in ref.LOG_RATIO_DS for h in ref.LOG_RATIO_HS for mass in (False, True)
         for offset in (0.0, 100.0)]


@pytest.mark.parametrize('family', ['mala', 'independent'])
def test_log_ratio_bound_holds_for_the_kernel_order_in_fp32(family):
    """At each (d, h, mass, offset) of the GPU list: an np.float32 emulation of the kernel's order (lane-strided partial
    sums, 64-lane butterfly) stays inside (ceil(d/64) + 20) 2^-24 S of the fp64 reference on every row -- well inside,
    yet not by so much that the bound says nothing: the worst ratio over the list lies between 1e-3 and 0.5."""
    worst = {}
    for i, (d, h, mass, offset) in enumerate(CASES):
        inp = ref.log_ratio_inputs(24, d, h, mass, offset, family, 1000 + i)
        want = ref.log_ratio(*inp, h)
        got = ref.log_ratio_kernel_order_f32(*inp, h).astype(np.float64)
        ratio = np.abs(got - want) / (ref.log_ratio_gamma(d) * ref.log_ratio_size(*inp, h))
        assert (ratio <= 1.0).all(), (d, h, mass, offset, ratio.max())
        worst[d] = max(worst.get(d, 0.0), float(ratio.max()))
    print('log-ratio fp32 emulation, %s: worst |err| / bound per d: %s'
          % (family, ', '.join('%d: %.2g' % kv for kv in sorted(worst.items()))))
    assert 1e-3 < max(worst.values()) < 0.5


# ------------------------------------------------------------------------------------------------ bite checks
@pytest.mark.parametrize('d', ref.LOG_RATIO_DS)
@pytest.mark.parametrize('mass', [False, True])
def test_log_ratio_tolerance_bites(d, mass):
    """On the MALA-like inputs of the GPU test at h = 1e-2: dropping the last coordinate's term, or using g in place of
    g', moves the fp64 reference by more than the tolerance of EVERY row."""
    h = ref.BITE_H
    for offset in (0.0, 100.0):
        inp = x, xp, u, up, g, gp, imd = ref.log_ratio_inputs(64, d, h, mass, offset, 'mala', 77 + d)
        tol = ref.log_ratio_gamma(d) * ref.log_ratio_size(*inp, h)
        want = ref.log_ratio(*inp, h)
        dropped = ref.log_ratio(*inp, h, drop_last=True)
        same_g = ref.log_ratio(x, xp, u, up, g, g, imd, h)
        assert (np.abs(dropped - want) > tol).all(), float((np.abs(dropped - want) / tol).min())
        assert (np.abs(same_g - want) > tol).all(), float((np.abs(same_g - want) / tol).min())


def test_select_carry_check_bites():
    """At the K6 test inputs a kernel that copied carry 0 but not carry 1 gives another carry 1 (and the same carry 0)."""
    x, xp, lr, u, carries, primes = ref.select_inputs(64, 5, 3)
    _, full, mask, _, _ = ref.select(x, xp, lr, u, carries, primes)
    _, part, _, _, _ = ref.select(x, xp, lr, u, carries, primes, copy_carries=1)
    assert 0 < mask.sum() < 64
    assert (full[0] == part[0]).all() and (full[1] != part[1]).sum() == mask.sum()
    assert (part[1] == carries[1]).all()


def test_moments_references():
    """moments is the exact sum of the fp32 values; moments_fp32sq differs from it by at most 2^-24 sum x^2."""
    x, *_ = ref.select_inputs(500, 7, 5)
    s, s2 = ref.moments(x)
    t, t2 = ref.moments_fp32sq(x)
    assert (s == t).all()
    assert (np.abs(s2 - t2) <= ref.EPS32 * s2).all() and (s2 != t2).any()
    np.testing.assert_allclose(s, [sum(float(v) for v in x[:, c]) for c in range(7)], rtol=1e-14)


def test_select_layouts_cover_the_nine_instantiations():
    ds = (1, 4, 5, 8, 13, 16, 25, 32, 50, 64, 100, 128, 200, 256, 257, 300, 512, 700, 1024)
    assert {ref.select_layout(d)[:2] for d in ds} == {(4, 1), (4, 2), (4, 4), (4, 8), (4, 16), (4, 32), (4, 64), (8, 64),
                                                      (16, 64)}
    assert ref.select_layout(4) == (4, 1, 256) and ref.select_layout(300) == (8, 64, 4)
