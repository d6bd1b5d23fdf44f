"""GPU: the stand-alone kernels of the split path (csrc/misc_kernels.hip, csrc/fit_support.hip) and the statistics fold
behind them (csrc/common.hpp), each against the fp64 references of tests/split_fp64.py at every instantiation, ragged
size, grid-stride loop and argument edge.  All calls go through hip.lib() with ctypes structs; inputs are seeded CPU draws.

Which case enters which path:
  K6 instantiations <CPL, LPC>: d = 1, 4 -> <4,1>; 5, 8 -> <4,2>; 13, 16 -> <4,4>; 25, 32 -> <4,8>; 50, 64 -> <4,16>;
    100, 128 -> <4,32>; 200, 256 -> <4,64>; 257, 300, 512 -> <8,64>; 700, 1024 -> <16,64>  (test_select_layouts)
  K6 grid stride (a lane sums two rows in fp32): test_select_grid_stride (d = 4, n = 2048*256 + 5; d = 1024, n = 8195)
  n_carry 0 / 1 / 2: test_select_carries;  rng_tag accept / jump: test_select_native_uniforms
  tail_slot 0 / 2, deferred and mixed folds: test_select_deferred_statistics
  grid strides of the others: test_philox_normals_grid_stride, test_log_ratio_many_rows, test_rows_sample_grid_stride,
  test_blob_copy (300 000 elements; 17 and 33 pieces split over launches)
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_fp64 as ref  # noqa: E402
from split_fp64 import philox, shuffle  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
CANARY = -12345.5
MAX_GRID = 2048           # kMaxGrid (csrc/common.hpp)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _dv(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(n_floats, dev):
    """A buffer of n_floats followed by 16 canary floats: (view of the first n_floats, whole buffer)."""
    buf = torch.full((n_floats + 16,), CANARY, dtype=torch.float32, device=dev)
    return buf[:n_floats], buf


def _canaries_intact(buf):
    return bool((buf[-16:] == CANARY).all())


def _ids(off, n):
    return (np.arange(n, dtype=np.uint64) + np.uint64(off)).astype(np.uint32)   # the kernels keep the low 32 bits


# ================================================================================================ Philox streams
OFFSETS = (0, 5000, 2 ** 31 - 4)          # the last one crosses the sign bit inside the rows


@pytest.mark.parametrize('d', [1, 3, 4, 5, 37, 1024])
def test_philox_normals(dev, d):
    """nfmc_philox_normals_f32 against oracle.philox.normal_field: every round count, both normal tags, every offset."""
    from nfmc_amd import hip
    n, step = 1000, 77
    out = torch.empty(n, d, device=dev)
    worst = 0.0
    for rounds in (0, 10, 7):
        for tag in (philox.TAG_NOISE, philox.TAG_LATENT):
            for off in OFFSETS:
                rng = hip.make_rng(SEED, off, step, rounds=rounds)
                out.fill_(CANARY)
                hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), tag, n, d, hip.ptr(out), hip.stream()), 'normals')
                want = philox.normal_field(SEED, _ids(off, n), step, d, tag, rounds=rounds or 10)
                err = np.abs(out.cpu().numpy().astype(np.float64) - want).max()
                worst = max(worst, err)
                assert err <= 4e-6, (rounds, tag, off, err)
    print('philox normals d=%d: worst |err| / 4e-6 = %.3g' % (d, worst / 4e-6))


def test_philox_normals_grid_stride(dev):
    """n * nblk = 70000 * 8 > 2048 * 256: a thread takes more than one block of four."""
    from nfmc_amd import hip
    n, d, step, off = 70000, 32, 3, 5000
    assert n * ((d + 3) // 4) > MAX_GRID * 256
    out, buf = _guarded(n * d, dev)
    rng = hip.make_rng(SEED, off, step)
    hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), philox.TAG_NOISE, n, d, hip.ptr(out), hip.stream()), 'normals')
    want = philox.normal_field(SEED, _ids(off, n), step, d, philox.TAG_NOISE)
    np.testing.assert_allclose(out.cpu().numpy().reshape(n, d), want, atol=4e-6, rtol=0)
    assert _canaries_intact(buf)


def test_philox_uniforms(dev):
    """Bitwise, both tags, at every packing position of the accept stream (step0 >> 2, word step0 & 3) and at 2^32 - 1."""
    from nfmc_amd import hip
    n = 1000
    u, buf = _guarded(n, dev)
    for rounds in (0, 7):
        for off in OFFSETS:
            for step in (0, 1, 2, 3, 4, 7, 2 ** 32 - 1):
                rng = hip.make_rng(SEED, off, step, rounds=rounds)
                for tag, fn in ((philox.TAG_ACCEPT, philox.accept_uniform), (philox.TAG_JUMP, philox.jump_uniform)):
                    hip.check(hip.lib().nfmc_philox_uniforms_f32(C.byref(rng), tag, n, hip.ptr(u), hip.stream()), 'uniforms')
                    np.testing.assert_array_equal(u.cpu().numpy(), fn(SEED, _ids(off, n), step, rounds=rounds or 10))
    assert _canaries_intact(buf)


def test_philox_argument_errors(dev):
    from nfmc_amd import hip
    lib, out = hip.lib(), torch.empty(64, device=dev)
    rng = hip.make_rng(SEED, 0, 0)
    for tag in (philox.TAG_NOISE, philox.TAG_LATENT, 4, -1):
        assert lib.nfmc_philox_uniforms_f32(C.byref(rng), tag, 64, hip.ptr(out), hip.stream()) == hip.EINVAL
    bad = hip.make_rng(SEED, 0, 0, rounds=5)
    assert lib.nfmc_philox_uniforms_f32(C.byref(bad), philox.TAG_ACCEPT, 64, hip.ptr(out), hip.stream()) == hip.EINVAL
    assert lib.nfmc_philox_normals_f32(C.byref(bad), philox.TAG_NOISE, 16, 4, hip.ptr(out), hip.stream()) == hip.EINVAL


# ================================================================================================ Langevin proposal
def _propose(hip, x, g, imd, h, n, d, rng, out):
    return hip.lib().nfmc_langevin_propose_f32(hip.ptr(x), hip.ptr(g), hip.ptr(imd) if imd is not None else None, h, n, d,
                                               C.byref(rng), hip.ptr(out), hip.stream())


@pytest.mark.parametrize('d', [1, 3, 4, 5, 63, 64, 65, 257, 1000])
def test_langevin_propose(dev, d):
    """nfmc_langevin_propose_f32 on replayed and on native noise: per element inside 8 * 2^-24 (|x| + |h g / m^2| +
    |sqrt(2h) z / m|) of the fp64 proposal (native: + 4e-6 sqrt(2h) / m for the hardware transcendentals)."""
    from nfmc_amd import hip
    step, off = 9, 5000
    worst = {False: 0.0, True: 0.0}
    for i, n in enumerate((1, 7, 300)):
        gen = torch.Generator().manual_seed(100 * d + i)
        imd_v = ref.mass_vector(d, gen)
        c = torch.randn(n, d, generator=gen).float().numpy()
        g = (3 * torch.randn(n, d, generator=gen)).float().numpy()
        z = torch.randn(n, d, generator=gen).float().numpy()
        zn = philox.normal_field(SEED, _ids(off, n), step, d, philox.TAG_NOISE)
        for offset in (0.0, 100.0):
            x = (c + np.float32(offset)).astype(np.float32)
            x_d, g_d, z_d = _dv(x, dev), _dv(g, dev), _dv(z, dev)
            for imd in (None, imd_v):
                imd_d = _dv(imd, dev)
                for h in (1e-4, 0.05, 1.0):
                    for native in (False, True):
                        out, buf = _guarded(n * d, dev)
                        rng = hip.make_rng(SEED, off, step, None if native else z_d)
                        hip.check(_propose(hip, x_d, g_d, imd_d, h, n, d, rng, out), 'propose')
                        noise = zn if native else z
                        want = ref.propose(x, g, imd, h, noise)
                        bound = ref.propose_bound(x, g, imd, h, noise, native=native)
                        ratio = np.abs(out.cpu().numpy().reshape(n, d).astype(np.float64) - want) / bound
                        assert (ratio <= 1.0).all(), (n, offset, imd is not None, h, native, ratio.max())
                        assert _canaries_intact(buf)
                        worst[native] = max(worst[native], float(ratio.max()))
    print('langevin_propose d=%d: worst |err| / bound = %.3g (replay), %.3g (native)' % (d, worst[False], worst[True]))


def test_langevin_propose_argument_errors(dev):
    from nfmc_amd import hip
    n, d = 8, 5
    x = torch.zeros(n, d, device=dev)
    out = torch.empty(n, d, device=dev)
    rng = hip.make_rng(SEED, 0, 0)
    for h in (0.0, -0.1, math.nan):
        assert _propose(hip, x, x, None, h, n, d, rng, out) == hip.EINVAL
    assert _propose(hip, x, x, None, 0.1, n, d, hip.make_rng(SEED, 0, 0, rounds=7), out) == hip.EUNSUPPORTED
    assert _propose(hip, x, x, None, 0.1, n, d, hip.make_rng(SEED, 0, 0, rounds=5), out) == hip.EINVAL


# ================================================================================================ Langevin log ratio
def _log_ratio(hip, t, h, n, d, out):
    x, xp, u, up, g, gp, imd = t
    return hip.lib().nfmc_langevin_log_ratio_f32(hip.ptr(x), hip.ptr(xp), hip.ptr(u), hip.ptr(up), hip.ptr(g), hip.ptr(gp),
                                                 hip.ptr(imd) if imd is not None else None, h, n, d, hip.ptr(out),
                                                 hip.stream())


def _check_log_ratio(hip, dev, inp, h, n, d):
    """One launch on the n rows of `inp`; |got - ref| / ((ceil(d/64) + 20) 2^-24 S) per row."""
    t = tuple(_dv(v, dev) for v in inp)
    out, buf = _guarded(n, dev)
    hip.check(_log_ratio(hip, t, h, n, d, out), 'log_ratio')
    want = ref.log_ratio(*inp, h)
    bound = ref.log_ratio_gamma(d) * ref.log_ratio_size(*inp, h)
    ratio = np.abs(out.cpu().numpy().astype(np.float64) - want) / bound
    assert _canaries_intact(buf)
    return ratio


@pytest.mark.parametrize('d', ref.LOG_RATIO_DS)
def test_langevin_log_ratio(dev, d):
    """nfmc_langevin_log_ratio_f32: |got - ref| <= (ceil(d/64) + 20) 2^-24 S on every row, for a MALA-like proposal (tf is
    the cancelled noise) and for independent inputs, mass on and off, every listed h and n; x centred and offset by 100."""
    from nfmc_amd import hip
    worst, k = 0.0, 0
    for family in ('mala', 'independent'):
        for mass in (False, True):
            for h in ref.LOG_RATIO_HS:
                for offset, ns in ((0.0, (1, 5, 64, 300)), (100.0, (64,))):
                    k += 1
                    inp = ref.log_ratio_inputs(max(ns), d, h, mass, offset, family, 7000 + 50 * d + k)
                    for n in ns:
                        rows = tuple(v[:n] for v in inp[:6]) + (inp[6],)
                        ratio = _check_log_ratio(hip, dev, rows, h, n, d)
                        assert (ratio <= 1.0).all(), (family, mass, h, offset, n, ratio.max())
                        worst = max(worst, float(ratio.max()))
    print('langevin_log_ratio d=%d: worst |err| / bound = %.3g' % (d, worst))


def test_log_ratio_many_rows(dev):
    """n = 70000 at d = 4: 70000 waves > 2048 * 4, so a wave takes more than one row."""
    from nfmc_amd import hip
    n, d, h = 70000, 4, 1e-2
    assert n > MAX_GRID * 4
    inp = ref.log_ratio_inputs(n, d, h, True, 0.0, 'mala', 31)
    ratio = _check_log_ratio(hip, dev, inp, h, n, d)
    assert (ratio <= 1.0).all(), ratio.max()
    print('langevin_log_ratio n=70000 d=4: worst |err| / bound = %.3g' % ratio.max())


def test_log_ratio_nonfinite_and_argument_errors(dev):
    """A non-finite u' gives a non-finite ratio (never a finite one); step sizes that are not positive are EINVAL."""
    from nfmc_amd import hip
    n, d, h = 6, 65, 0.05
    x, xp, u, up, g, gp, imd = ref.log_ratio_inputs(n, d, h, True, 0.0, 'mala', 5)
    up = up.copy()
    up[1], up[3], up[4] = np.inf, -np.inf, np.nan
    t = tuple(_dv(v, dev) for v in (x, xp, u, up, g, gp, imd))
    out = torch.empty(n, device=dev)
    hip.check(_log_ratio(hip, t, h, n, d, out), 'log_ratio')
    got = out.cpu().numpy()
    assert np.isfinite(got[[0, 2, 5]]).all()
    assert got[1] == -np.inf and got[3] == np.inf and np.isnan(got[4])
    for bad in (0.0, -1.0, math.nan):
        assert _log_ratio(hip, t, bad, n, d, out) == hip.EINVAL


L_SEAM = 2    # leapfrog steps of the HMC case


@pytest.mark.parametrize('kind, h, seed', [('langevin', 0.02, 4242), ('mh', 0.05, 4244), ('hmc', 0.75, 4242)])
def test_langevin_propose_seam_stand_alone(dev, kind, h, seed):
    """Langevin.propose, MH.propose and HMC.propose (2 leapfrog steps) outside a run (native Philox, d = 300, a mass
    vector, a callable quadratic target):
      x_prime bit-identical to the state the same sampler's in-run split path proposes in its first transition
        (fuse='never', same seed, one iteration, `propose` wrapped to record what it returns): the same code on the same
        Philox stream, so no tolerance; for Langevin also the oracle's x_prime inside the native proposal bound;
      the counters the reference's formulas: Langevin (2n, 2n, 0), MH (2n, 0, 0), HMC (2 L n + 2n, 2 L n, 0);
      the oracle's mask (PhiloxNoise(seed, 0)) on every row outside the near-tie margin.
    MH has no step size: its proposal scale is the mass vector, so that case scales the vector by h.  The MH and HMC
    seeds and step sizes were picked on the CPU, from the fp64 oracle alone (seeds 4242 .. 4249, a few h each): such that
    the oracle leaves no row out as a near-tie, accepts some rows but not all (MH 113, HMC 202 of 256), and its smallest
    |log u - log ratio| / max(1, |log u|) is 0.023 (MH) and 0.091 (HMC), far above the ~1e-4 that fp32 sums of U ~ 300
    can move the device's log ratio."""
    from nfmc_amd.samplers import mcmc
    from oracle import samplers as osamp
    n, d = 256, 300
    gen = torch.Generator().manual_seed(9)
    imd = ref.mass_vector(d, gen)
    x = torch.randn(n, d, generator=gen).float()

    def target(v):
        return (v * v).sum(-1)

    noise = osamp.PhiloxNoise(seed, 0, dtype=torch.float64)
    if kind == 'langevin':
        def make():
            return mcmc.Langevin((d,), target, kernel=mcmc.LangevinKernel(event_size=d, step_size=h,
                                                                           inv_mass_diag=torch.from_numpy(imd)))
        counters = (2 * n, 2 * n, 0)
        want_xp, want_mask, lr, log_u = osamp.langevin_propose(x.double(), target, ref.h32(h),
                                                               torch.from_numpy(imd).double(), True, noise, 0)
    elif kind == 'mh':
        imd = (np.float32(h) * imd).astype(np.float32)

        def make():
            return mcmc.MH((d,), target, kernel=mcmc.MHKernel(event_size=d, inv_mass_diag=torch.from_numpy(imd)))
        counters = (2 * n, 0, 0)
        want_xp, want_mask, lr, log_u = osamp.mh_propose(x.double(), target, torch.from_numpy(imd).double(), True, noise, 0)
    else:
        def make():
            return mcmc.HMC((d,), target, kernel=mcmc.HMCKernel(event_size=d, step_size=h, n_leapfrog_steps=L_SEAM,
                                                                 inv_mass_diag=torch.from_numpy(imd)))
        counters = (2 * L_SEAM * n + 2 * n, 2 * L_SEAM * n, 0)
        want_xp, want_mask, lr, log_u = osamp.hmc_propose(x.double(), target, ref.h32(h), torch.from_numpy(imd).double(),
                                                          L_SEAM, True, noise, 0)
    s = make()
    s.seed = seed
    xp, mask, n_calls, n_grads, n_div = s.propose(x.to(dev))
    assert (n_calls, n_grads, n_div) == counters

    # the first transition of the in-run split path
    r = make()
    r.seed, r.fuse = seed, 'never'
    r.params.n_iterations = 1
    proposed, inner = [], r.propose

    def recording(v):
        proposed.append(inner(v))
        return proposed[-1]

    r.propose = recording
    r.sample(x, show_progress=False)
    assert len(proposed) == 1 and proposed[0][2:] == counters
    assert torch.equal(xp, proposed[0][0])

    worst = math.nan   # x_prime is held against the oracle for Langevin only
    if kind == 'langevin':
        zn = philox.normal_field(seed, np.arange(n), 0, d, philox.TAG_NOISE)
        bound = ref.propose_bound(x.numpy(), (2 * x).numpy(), imd, h, zn, native=True)
        ratio = np.abs(xp.cpu().numpy().astype(np.float64) - want_xp.numpy()) / bound
        assert (ratio <= 1.0).all(), ratio.max()
        worst = ratio.max()
    lu, lr = log_u.numpy(), lr.numpy()
    keep = np.abs(lu - lr) >= ref.TIE_MARGIN * np.maximum(1.0, np.abs(lu))
    print('%s.propose stand-alone: worst x_prime |err| / bound = %.3g, rows left out as near-ties: %d of %d, the oracle '
          'accepts %d, mask rows that differ: %d' % (kind, worst, int((~keep).sum()), n, int(want_mask.sum()),
                                                     int((mask.cpu().numpy() != want_mask.numpy()).sum())))
    assert keep.mean() >= 0.999
    np.testing.assert_array_equal(mask.cpu().numpy()[keep], want_mask.numpy()[keep])
    assert 0 < int(want_mask.sum()) < n


# ================================================================================================ K6
SELECT_DS = (1, 4, 5, 8, 13, 16, 25, 32, 50, 64, 100, 128, 200, 256, 257, 300, 512, 700, 1024)


class _Select:
    """Device copies of one K6 case and the launch on them."""

    def __init__(self, hip, dev, x, xp, lr, u, carries=(), primes=()):
        self.hip, self.n, self.d = hip, x.shape[0], x.shape[1]
        self.x, self.xbuf = _guarded(x.size, dev)
        self.x.copy_(_dv(x.reshape(-1), dev))
        self.xp = _dv(xp, dev)
        self.lr, self.u = _dv(lr, dev), _dv(u, dev)
        self.carries = [_dv(c, dev) for c in carries]
        self.primes = [_dv(c, dev) for c in primes]
        self.mask = torch.full((self.n + 16,), 7, dtype=torch.uint8, device=dev)

    def args(self, stats=None, rng=None, tag=None, n_carry=None, with_mask=True):
        hip = self.hip
        st = hip.NfmcSelectArgs()
        st.x, st.x_prime, st.n, st.d = hip.ptr(self.x), hip.ptr(self.xp), self.n, self.d
        st.n_carry = len(self.carries) if n_carry is None else n_carry
        for k in range(min(st.n_carry, 2, len(self.carries))):
            st.carry[k] = hip.ptr(self.carries[k])
            st.carry_prime[k] = hip.ptr(self.primes[k])
        st.log_ratio = hip.ptr(self.lr) if self.lr is not None else None
        st.uniforms = hip.ptr(self.u) if self.u is not None else None
        st.rng = rng if rng is not None else hip.make_rng(SEED, 0, 0)
        st.rng_tag = hip.TAG_ACCEPT if tag is None else tag
        st.stats = stats if stats is not None else hip.null_stats()
        st.mask_out = hip.ptr(self.mask[:self.n], torch.uint8) if with_mask else None
        return st

    def launch(self, **kw):
        st = self.args(**kw)
        return self.hip.lib().nfmc_mh_accept_select_f32(C.byref(st), self.hip.stream())

    def state(self):
        return self.x.cpu().numpy().reshape(self.n, self.d)

    def got_mask(self):
        m = self.mask.cpu().numpy()
        assert (m[self.n:] == 7).all(), 'mask_out written past n'
        return m[:self.n]


def _assert_selected(case, x, xp, lr, u, carries, primes, cap=True):
    """mask, state and carries of `case` after one launch equal the reference outside the near-tie margin; returns the
    reference tuple and the rows kept."""
    new_x, new_c, mask, acc, bad = ref.select(x, xp, lr, u, carries, primes)
    tie = ref.near_tie(lr, u) if lr is not None else np.zeros(x.shape[0], dtype=bool)
    keep = ~tie
    if cap:
        assert tie.sum() <= 0.001 * x.shape[0], 'too many near-ties: %d of %d' % (tie.sum(), x.shape[0])
    got_mask, got_x = case.got_mask(), case.state()
    np.testing.assert_array_equal(got_mask[keep], mask[keep].astype(np.uint8))
    assert got_x[keep].tobytes() == new_x[keep].tobytes()       # accepted rows are x', the others bitwise untouched
    for k, c in enumerate(case.carries):
        assert c.cpu().numpy()[keep].tobytes() == new_c[k][keep].tobytes(), 'carry %d' % k
    assert _canaries_intact(case.xbuf)
    return (new_x, new_c, mask, acc, bad), keep


def _check_totals(totals, want_sx, want_sx2, abs_sx, abs_sx2, rel):
    """|sum_x - want| <= rel * sum|x| and the same for the squares; returns the worst error / bound."""
    sx, sx2 = totals[0].numpy(), totals[1].numpy()
    r1 = np.abs(sx - want_sx) / (rel * abs_sx)
    r2 = np.abs(sx2 - want_sx2) / (rel * abs_sx2)
    assert (r1 <= 1.0).all() and (r2 <= 1.0).all(), (r1.max(), r2.max())
    return max(float(r1.max()), float(r2.max()))


def test_select_layouts():
    """The d list enters each of the nine select_kernel instantiations (host arithmetic of the dispatch)."""
    assert {ref.select_layout(d)[:2] for d in SELECT_DS} == {(4, 1), (4, 2), (4, 4), (4, 8), (4, 16), (4, 32), (4, 64),
                                                             (8, 64), (16, 64)}


@pytest.mark.parametrize('d', SELECT_DS)
def test_select(dev, d):
    """K6 at the tile edges of d's layout (rows per tile = 4 * (64 / LPC)): mask, kept rows and two carries equal the
    reference exactly, x offset by 100; counters exact; sum_x and sum_x2 are the fp64 sums of the fp32 values (and of their
    fp32 squares) to 1e-12, since each lane holds one row; a second call accumulates; statistics off changes nothing."""
    from nfmc_amd import hip
    rows = ref.select_layout(d)[2]
    worst, left_out, total = 0.0, 0, 0
    for i, n in enumerate((1, rows - 1, rows, rows + 1, 3 * rows + 2)):
        x, xp, lr, u, carries, primes = ref.select_inputs(n, d, 300 * d + i)
        stats = hip.DeviceStats(d, dev)
        case = _Select(hip, dev, x, xp, lr, u, carries, primes)
        hip.check(case.launch(stats=stats.struct()), 'select')
        (new_x, new_c, mask, acc, bad), keep = _assert_selected(case, x, xp, lr, u, carries, primes, cap=False)
        left_out, total = left_out + int((~keep).sum()), total + n
        if not keep.all():
            continue                                   # a near-tie may differ: the totals are then not comparable
        tot = stats.host_totals()
        assert tot[2].tolist()[:3] == [acc, n, bad] and tot[3].tolist()[:3] == [0, 0, 0]
        sx, sx2 = ref.moments_fp32sq(new_x)
        ax, ax2 = ref.abs_moments(new_x)
        worst = max(worst, _check_totals(tot, sx, sx2, ax, ax2, 1e-12))
        # the same launch again: accepted rows already hold x', the others reject again -> every total doubles
        hip.check(case.launch(stats=stats.struct()), 'select')
        tot = stats.host_totals()
        assert tot[2].tolist()[:3] == [2 * acc, 2 * n, 2 * bad]
        _check_totals(tot, 2 * sx, 2 * sx2, 2 * ax, 2 * ax2, 1e-12)
        assert case.state().tobytes() == new_x.tobytes()
        # statistics off: the same decisions and state from the same inputs
        off = _Select(hip, dev, x, xp, lr, u, carries, primes)
        hip.check(off.launch(), 'select')
        assert off.state().tobytes() == new_x.tobytes() and (off.got_mask() == mask).all()
    assert left_out <= 0.001 * total
    print('select d=%d (CPL, LPC, rows/tile = %s): worst statistics |err| / (1e-12 sum) = %.3g, near-ties left out: %d of %d'
          % (d, ref.select_layout(d), worst, left_out, total))


def test_select_shape_limit(dev):
    from nfmc_amd import hip
    x, xp, lr, u, _, _ = ref.select_inputs(4, 1025, 1, n_carry=0)
    assert _Select(hip, dev, x, xp, lr, u).launch() == hip.ESHAPE


@pytest.mark.parametrize('d,n', [(4, MAX_GRID * 256 + 5), (1024, MAX_GRID * 4 + 3)])
def test_select_grid_stride(dev, d, n):
    """More tiles than the grid: workgroup 0 takes two tiles, its lanes add two rows in fp32 before widening, so the sums
    are held to 2^-23 of sum|x| (sum x^2) instead of 1e-12.  Decisions, rows and counters stay exact."""
    from nfmc_amd import hip
    rows = ref.select_layout(d)[2]
    assert -(-n // rows) > MAX_GRID
    x, xp, lr, u, carries, primes = ref.select_inputs(n, d, 17 + d, n_carry=1)
    stats = hip.DeviceStats(d, dev)
    case = _Select(hip, dev, x, xp, lr, u, carries, primes)
    hip.check(case.launch(stats=stats.struct()), 'select')
    (new_x, _, _, acc, bad), keep = _assert_selected(case, x, xp, lr, u, carries, primes)
    tot = stats.host_totals()
    flips = int((~keep).sum())
    assert abs(int(tot[2][0]) - acc) <= flips and tot[2].tolist()[1:3] == [n, bad]
    if flips == 0:
        sx, sx2 = ref.moments_fp32sq(new_x)
        ax, ax2 = ref.abs_moments(new_x)
        worst = _check_totals(tot, sx, sx2, ax, ax2, 2.0 ** -23)
        print('select grid stride d=%d n=%d: worst statistics |err| / (2^-23 sum) = %.3g' % (d, n, worst))
    print('select grid stride d=%d n=%d: near-ties left out: %d' % (d, n, flips))


@pytest.mark.parametrize('d', [5, 300])
def test_select_log_ratio_edges(dev, d):
    """+inf accepts and counts as non-finite, -inf and NaN reject and count, 0 and 3.0e38 are ordinary; log_ratio = NULL
    accepts every row and counts nothing."""
    from nfmc_amd import hip
    n = 70
    x, xp, lr, u, carries, primes = ref.select_inputs(n, d, 23)
    lr = lr.copy()
    lr[[0, 9, 64]] = np.inf
    lr[[1, 65]] = -np.inf
    lr[[2, 66, 69]] = np.nan
    lr[3], lr[4], lr[5] = 0.0, 3.0e38, -3.0e38
    stats = hip.DeviceStats(d, dev)
    case = _Select(hip, dev, x, xp, lr, u, carries, primes)
    hip.check(case.launch(stats=stats.struct()), 'select')
    (_, _, mask, acc, bad), keep = _assert_selected(case, x, xp, lr, u, carries, primes, cap=False)
    assert keep.all() and bad == 8
    assert mask[[0, 9, 64, 4]].all() and not mask[[1, 65, 2, 66, 69, 5]].any()
    assert stats.host_totals()[2].tolist()[:3] == [acc, n, 8]
    stats = hip.DeviceStats(d, dev)
    case = _Select(hip, dev, x, xp, None, None, carries, primes)
    hip.check(case.launch(stats=stats.struct()), 'select')
    _assert_selected(case, x, xp, None, None, carries, primes)
    assert case.got_mask().all() and case.state().tobytes() == xp.tobytes()
    assert stats.host_totals()[2].tolist()[:3] == [n, n, 0]


@pytest.mark.parametrize('d', [5, 300])
@pytest.mark.parametrize('n_carry', [0, 1, 2])
def test_select_carries(dev, d, n_carry):
    """n_carry carried scalars follow the accepted rows; the carries beyond n_carry are not touched; no mask_out is fine."""
    from nfmc_amd import hip
    n = 133
    x, xp, lr, u, carries, primes = ref.select_inputs(n, d, 40 + n_carry)
    case = _Select(hip, dev, x, xp, lr, u, carries, primes)
    hip.check(case.launch(n_carry=n_carry, with_mask=False), 'select')
    new_x, new_c, mask, _, _ = ref.select(x, xp, lr, u, carries, primes, copy_carries=n_carry)
    assert not ref.near_tie(lr, u).any()
    assert case.state().tobytes() == new_x.tobytes() and (case.mask.cpu().numpy() == 7).all()
    for k in range(2):
        assert case.carries[k].cpu().numpy().tobytes() == new_c[k].tobytes(), 'carry %d' % k
        assert case.primes[k].cpu().numpy().tobytes() == primes[k].tobytes()
    assert 0 < mask.sum() < n


def test_select_native_uniforms(dev):
    """The kernel's own accept / jump stream at every packing position gives the decisions of oracle.philox's uniforms,
    and of the same uniforms replayed; 4096 rows, so the 0.1 % cap on near-ties is a real one."""
    from nfmc_amd import hip
    n, d, off = 4096, 13, 5000
    x, xp, lr, _, carries, primes = ref.select_inputs(n, d, 61, n_carry=1)
    left_out = 0
    for tag, fn in ((hip.TAG_ACCEPT, philox.accept_uniform), (hip.TAG_JUMP, philox.jump_uniform)):
        for step in (0, 1, 2, 3, 5):
            u = fn(SEED, _ids(off, n), step)
            rng = hip.make_rng(SEED, off, step)
            native = _Select(hip, dev, x, xp, lr, None, carries, primes)
            hip.check(native.launch(rng=rng, tag=tag), 'select')
            _, keep = _assert_selected(native, x, xp, lr, u, carries, primes)
            left_out += int((~keep).sum())
            replay = _Select(hip, dev, x, xp, lr, u, carries, primes)
            hip.check(replay.launch(rng=rng, tag=tag), 'select')
            assert (replay.got_mask() == native.got_mask()).all()      # the same uniforms, bit for bit: no margin
            assert replay.state().tobytes() == native.state().tobytes()
    print('select native uniforms: near-ties left out: %d of %d' % (left_out, 10 * n))


def test_select_argument_errors(dev):
    from nfmc_amd import hip
    n, d = 9, 5
    x, xp, lr, u, carries, primes = ref.select_inputs(n, d, 2)
    case = _Select(hip, dev, x, xp, lr, u, carries, primes)
    assert case.launch(n_carry=3) == hip.EINVAL
    assert case.launch(n_carry=-1) == hip.EINVAL
    st = case.args()
    st.carry[1] = None
    assert hip.lib().nfmc_mh_accept_select_f32(C.byref(st), hip.stream()) == hip.EINVAL
    st = case.args()
    st.carry_prime[0] = None
    assert hip.lib().nfmc_mh_accept_select_f32(C.byref(st), hip.stream()) == hip.EINVAL
    for tag in (0, 2, 4):
        assert case.launch(tag=tag) == hip.EINVAL
    assert case.launch(rng=hip.make_rng(SEED, 0, 0, rounds=7)) == hip.EUNSUPPORTED
    assert case.launch(rng=hip.make_rng(SEED, 0, 0, rounds=5)) == hip.EINVAL
    stats = hip.DeviceStats(d, dev)
    width = 2 * ref.padded_d(d) + 4
    small = stats._raw()
    small.scratch_bytes = 3 * width * 8 - 8          # n = 9 at d = 5 (128 rows per tile) is one workgroup: one slab
    assert case.launch(stats=small) == hip.OK
    small.scratch_bytes = width * 8 - 8
    assert case.launch(stats=small) == hip.ESCRATCH
    assert case.launch(stats=stats._raw(1, 1)) == hip.EINVAL                   # tail_slot is 0 or 2
    short = stats._raw(1, 0)
    short.scratch_bytes = int(hip.lib().nfmc_stats_scratch_bytes(d)) - 8      # deferred: the whole slab or nothing
    assert case.launch(stats=short) == hip.EINVAL
    fold = stats._raw()
    assert hip.lib().nfmc_stats_fold_f32(C.byref(fold), 1025, 0, None, 0, hip.stream()) == hip.ESHAPE
    assert case.state().tobytes() != x.tobytes()      # (the accepted launch above ran)


@pytest.mark.parametrize('d', [5, 64, 300])
def test_select_deferred_statistics(dev, d):
    """Three K6 calls on one DeviceStats, (a) folded per call, (b) deferred -- two with tail_slot 0, one with tail_slot 2
    -- and folded once by nfmc_stats_fold_f32, (c) deferred, immediate, deferred: the same sums (1e-12) and the same
    counters; the jump call's accepts land in jump_counters with its attempts; the scratch is all zero after the fold."""
    from nfmc_amd import hip
    n = 3 * ref.select_layout(d)[2] + 2
    x, xp, lr, u, _, _ = ref.select_inputs(n, d, 90 + d, n_carry=0)
    gen = torch.Generator().manual_seed(d)
    calls = []
    for k in range(3):
        xpk = (torch.randn(n, d, generator=gen) + 100).float().numpy()
        lrk = (-0.7 + 1.5 * torch.randn(n, generator=gen)).float().numpy()
        lrk[k] = np.nan                                    # one non-finite ratio per call
        calls.append((xpk, lrk, ref.replay_uniforms(n, gen)))
    # the reference chain of three transitions
    cur, accs, sx, sx2, ax, ax2 = x, [], 0.0, 0.0, 0.0, 0.0
    for xpk, lrk, uk in calls:
        assert not ref.near_tie(lrk, uk).any()
        cur, _, _, acc, bad = ref.select(cur, xpk, lrk, uk)
        assert bad == 1
        accs.append(acc)
        m, a = ref.moments_fp32sq(cur), ref.abs_moments(cur)
        sx, sx2, ax, ax2 = sx + m[0], sx2 + m[1], ax + a[0], ax2 + a[1]

    def run(modes):
        stats = hip.DeviceStats(d, dev)
        xs, buf = _guarded(n * d, dev)
        xs.copy_(_dv(x.reshape(-1), dev))
        for (xpk, lrk, uk), mode in zip(calls, modes):
            case = _Select(hip, dev, x, xpk, lrk, uk)
            case.x, case.xbuf = xs, buf
            st = stats.struct() if mode == 'now' else stats.struct(defer=True, attempted=n, jump=(mode == 'jump'))
            hip.check(case.launch(stats=st), 'select')
        assert xs.cpu().numpy().tobytes() == cur.tobytes() and _canaries_intact(buf)
        return stats

    worst = 0.0
    for modes in (('now', 'now', 'now'), ('defer', 'defer', 'jump'), ('defer', 'now', 'defer'), ('now', 'defer', 'jump')):
        stats = run(modes)
        if 'now' not in modes:
            assert stats._pending and int(stats._counters.cpu()[hip.CNT_ATTEMPTED]) == 0     # nothing folded yet
        tot = stats.host_totals()
        worst = max(worst, _check_totals(tot, sx, sx2, ax, ax2, 1e-12))
        if modes[2] == 'jump':
            assert tot[2].tolist()[:3] == [accs[0] + accs[1], 2 * n, 2]
            assert tot[3].tolist()[:3] == [accs[2], n, 1]
        else:
            assert tot[2].tolist()[:3] == [sum(accs), 3 * n, 3] and tot[3].tolist()[:3] == [0, 0, 0]
        assert not bool(stats.scratch.any()), 'the scratch is not all zero after the fold'
    print('select deferred statistics d=%d: worst |err| / (1e-12 sum) = %.3g' % (d, worst))


# ================================================================================================ K7
def _moments(hip, x_d, rows, d, st):
    return hip.lib().nfmc_moments_update_f32(hip.ptr(x_d), rows, d, C.byref(st), hip.stream())


@pytest.mark.parametrize('d', [1, 5, 255, 256, 257, 1024])
def test_moments_update(dev, d):
    """K7 accumulates in fp64: sum x and sum x^2 of x offset by 100 to 1e-13 of sum|x|, sum x^2; two calls add; the
    counters do not move."""
    from nfmc_amd import hip
    gen = torch.Generator().manual_seed(d)
    big = (torch.randn(3000, d, generator=gen) + 100).float()
    worst = 0.0
    for rows in (1, 3, 4, 5, 1023, 1024, 1025, 3000):
        x = big[3000 - rows:].contiguous().numpy()
        stats = hip.DeviceStats(d, dev)
        x_d = _dv(x, dev)
        hip.check(_moments(hip, x_d, rows, d, stats.struct()), 'moments')
        hip.check(_moments(hip, x_d, rows, d, stats.struct()), 'moments')
        tot = stats.host_totals()
        (sx, sx2), (ax, ax2) = ref.moments(x), ref.abs_moments(x)
        worst = max(worst, _check_totals(tot, 2 * sx, 2 * sx2, 2 * ax, 2 * ax2, 1e-13))
        assert tot[2].tolist() == [0, 0, 0, 0] and tot[3].tolist() == [0, 0, 0, 0]
        assert not bool(stats.scratch.any())
    print('moments_update d=%d: worst |err| / (1e-13 sum) = %.3g' % (d, worst))


def test_moments_update_argument_errors(dev):
    from nfmc_amd import hip
    d, rows = 5, 40
    x_d = torch.ones(rows, 1025, device=dev)
    stats = hip.DeviceStats(d, dev)
    assert _moments(hip, x_d, rows, d, stats._raw(1, 0)) == hip.EUNSUPPORTED
    assert _moments(hip, x_d, rows, 1025, stats._raw()) == hip.ESHAPE
    short = stats._raw()
    short.scratch_bytes = 10 * (2 * ref.padded_d(d) + 4) * 8 - 8       # 40 rows -> 10 workgroups
    assert _moments(hip, x_d, rows, d, short) == hip.ESCRATCH
    short.scratch_bytes += 8
    assert _moments(hip, x_d, rows, d, short) == hip.OK
    assert stats.host_totals()[0].tolist() == [40.0] * d


# ================================================================================================ rows_sample
def _rows_sample(hip, x_d, n, d, seed, first, out, m, idx):
    return hip.lib().nfmc_rows_sample_f32(hip.ptr(x_d), n, d, seed, first, hip.ptr(out),
                                          m, hip.ptr(idx, torch.int64) if idx is not None else None, hip.stream())


def _check_rows_sample(hip, dev, n, d, seed, first, m, with_index, x, x_d):
    out, buf = _guarded((m + 1) * d, dev)                        # one spare row before the canaries
    idx = torch.full((m + 4,), -7, dtype=torch.int64, device=dev) if with_index else None
    rc = _rows_sample(hip, x_d, n, d, seed, first, out, m, idx)
    if first + m > n:
        assert rc == hip.EINVAL
        return
    hip.check(rc, 'rows_sample')
    want = shuffle.permutation_prefix(n, seed, m, first=first)
    got = buf.cpu().numpy()
    assert got[:m * d].tobytes() == x[want].tobytes()
    assert (got[m * d:] == CANARY).all()                          # `out` past m rows is untouched
    if with_index:
        np.testing.assert_array_equal(idx.cpu().numpy()[:m], want)
        assert (idx.cpu().numpy()[m:] == -7).all()
    for i in (0, m // 2, m - 1) if m else ():
        assert hip.lib().nfmc_rows_sample_index(n, seed, first + i) == want[i]


@pytest.mark.parametrize('n,d', [(1, 1), (2, 3), (255, 64), (256, 65), (257, 130), (1665, 7)])
def test_rows_sample(dev, n, d):
    """Rows and indices are bitwise those of oracle.shuffle.permutation_prefix for every first / m / index_out, each index
    equals nfmc_rows_sample_index; first + m > n is EINVAL."""
    from nfmc_amd import hip
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=gen).float().numpy()
    x_d = _dv(x, dev)
    seed = 0x0123456789ABCDEF ^ n
    combos = {(first, m) for m in (0, 1, n) for first in (0, 5, n - m)}
    for first, m in sorted(combos):
        for with_index in (False, True):
            _check_rows_sample(hip, dev, n, d, seed, first, m, with_index, x, x_d)
    want = shuffle.permutation_prefix(n, seed, n)
    assert sorted(want.tolist()) == list(range(n))                # a permutation
    assert all(hip.lib().nfmc_rows_sample_index(n, seed, i) == want[i] for i in range(n))
    assert hip.lib().nfmc_rows_sample_index(n, seed, n) == -1


def test_rows_sample_grid_stride(dev):
    """m = 20000 > 4096 * 4 output rows: a wave gathers more than one row."""
    from nfmc_amd import hip
    n, d, m, first = 60000, 2, 20000, 5
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(3)).float().numpy()
    _check_rows_sample(hip, dev, n, d, 99, first, m, True, x, _dv(x, dev))


# ================================================================================================ blob copy
def _blob_case(k, dev, gen, big=False):
    """k pieces with padded strides, every fifth one transposed, every seventh one empty (rows or cols 0); `big`: the
    first piece has 300 000 elements.  Returns (params, layout rows (off, rows, cols, rs, cs), vector length)."""
    layout, params, cur = [], [], 3
    for i in range(k):
        rows, cols = int(torch.randint(1, 9, (), generator=gen)), int(torch.randint(1, 12, (), generator=gen))
        if big and i == 0:
            rows, cols = 300, 1000
        if i % 7 == 6:
            rows, cols = (0, cols) if i % 2 else (rows, 0)
        pad = int(torch.randint(0, 4, (), generator=gen))
        if i % 5 == 4:
            rs, cs, span = 1, rows + pad, (rows + pad) * cols        # transposed: vec_col_stride = rows_padded
        else:
            rs, cs, span = cols + pad, 1, rows * (cols + pad)        # padded rows
        layout.append((cur, rows, cols, rs, cs))
        params.append(torch.randn(rows, cols, generator=gen).float().to(dev))
        cur += span + int(torch.randint(0, 3, (), generator=gen))
    return params, layout, cur + 5


def _pieces(hip, params, layout):
    return (hip.NfmcBlobPiece * len(layout))(*[
        hip.NfmcBlobPiece(hip.ptr(p) if p.numel() else None, off, rows, cols, rs, cs)
        for p, (off, rows, cols, rs, cs) in zip(params, layout)])


@pytest.mark.parametrize('k,big', [(1, False), (16, False), (17, False), (33, False), (3, True)])
def test_blob_copy(dev, k, big):
    """Gather into a NaN-filled vector writes exactly the mapped elements; scatter into zeroed parameters round-trips
    bitwise and leaves the vector alone.  17 and 33 pieces take two and three launches; 300 000 elements grid-stride."""
    from nfmc_amd import hip
    gen = torch.Generator().manual_seed(1000 + k)
    params, layout, length = _blob_case(k, dev, gen, big)
    if big:
        assert params[0].numel() > 1024 * 256
    want = np.full(length, np.nan, dtype=np.float32)
    for p, (off, rows, cols, rs, cs) in zip(params, layout):
        r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
        idx = off + r * rs + c * cs
        assert np.isnan(want[idx]).all()                 # the case's pieces do not overlap
        want[idx] = p.cpu().numpy()
    assert np.isnan(want).any()
    vec = torch.full((length,), math.nan, dtype=torch.float32, device=dev)
    arr = _pieces(hip, params, layout)
    hip.check(hip.lib().nfmc_flow_blob_copy_f32(hip.ptr(vec), arr, k, 1, hip.stream()), 'blob gather')
    assert vec.cpu().numpy().tobytes() == want.tobytes()
    zeroed = [torch.zeros_like(p) for p in params]
    arr0 = _pieces(hip, zeroed, layout)
    hip.check(hip.lib().nfmc_flow_blob_copy_f32(hip.ptr(vec), arr0, k, 0, hip.stream()), 'blob scatter')
    for z, p in zip(zeroed, params):
        assert z.cpu().numpy().tobytes() == p.cpu().numpy().tobytes()
    assert vec.cpu().numpy().tobytes() == want.tobytes()


def test_blob_copy_argument_errors(dev):
    from nfmc_amd import hip
    vec = torch.zeros(64, device=dev)
    p = torch.ones(2, 3, device=dev)
    for bad in ((0, -1, 3, 3, 1), (0, 2, -3, 3, 1), (-1, 2, 3, 3, 1)):
        arr = _pieces(hip, [p], [bad])
        assert hip.lib().nfmc_flow_blob_copy_f32(hip.ptr(vec), arr, 1, 1, hip.stream()) == hip.EINVAL
    arr = (hip.NfmcBlobPiece * 1)(hip.NfmcBlobPiece(None, 0, 2, 3, 3, 1))
    assert hip.lib().nfmc_flow_blob_copy_f32(hip.ptr(vec), arr, 1, 1, hip.stream()) == hip.EINVAL
    assert hip.lib().nfmc_flow_blob_copy_f32(hip.ptr(vec), arr, -1, 1, hip.stream()) == hip.EINVAL
    assert not bool(vec.any())
