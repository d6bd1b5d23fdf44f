"""The three flow-proposal Metropolis kernels behind nfmc_flow_mh_steps_f32 that serve conditioners wider than 8 units,
row by row against the fp64 oracle (oracle.samplers.imh_sample on the same Philox streams), as the register kernel is
held by the per-target files:

  'mfma'  flow_mh_mfma_kernel (csrc/flow_mfma.hip): d = 64 / 128, 32 < n_hidden <= 128, 1 or 2 hidden layers;
  'wide'  flow_mh_wide_kernel (csrc/mfma_wide.hip): the other multiples of 32 from 32 to 512, the state streamed through
          the workspace the package's flow carries;
  'lane'  flow_mh_kernel<HP> (csrc/flow_kernels.hip): one chain per lane: n_hidden 9 .. 32 at any d, wider conditioners off
          the matrix-core shapes, spline couplings, NFMC_FLOW_NO_MFMA=1, NFMC_FLOW_TILE_PATH=1 (HP = 4 / 8).

Each copies the transition (the `adjusted` branch, the carry of U(x) and log q(x) on accept, the logq_cached read, the
replay reads, the statistics slabs, the sample store), so each is asked the same questions.  Every case asserts which
kernel took it (target_harness.flow_mh_kernel_of): a case that lands on another kernel fails.

Inputs: centred_flow_pair (flow seed 5) about laplace_fit, or local_fit(p, 0.3) at the starts for the funnel, and
centred starts (seed 3), so that the fp64 oracle accepts: the accept branch runs on most chains.  n = 150 chains (one full
128-chain matrix-core tile and 22 chains of the next: one full wave and 6 lanes; for 'lane' two wave tiles and 22 lanes)
and T = 4 transitions; one case per kernel at n = 1, where every inactive lane reads row n - 1 = 0.  Every adjusted case
holds, for the fp64 oracle alone, an acceptance of at least FLOOR = 0.25 and under CAP = 0.10 of its chains within
MARGIN = 1e-3 of a tie; tests/test_host_flow_mh_wide.py proves that on the CPU (FLOW_TESTS).

Tolerance: compare_flow_mh's row tolerance with c = affine_c(d) for affine couplings and spline_c for splines.  The
fp32-against-fp64 figure of the oracle flow at each affine case's own proposals (spline_c's measurement, CPU alone) is
1.6e-6 .. 1.1e-4, the largest at d = 512 where 4 x it is 4.3e-4 against affine_c = 1.6e-3; nowhere does 4 x the figure
exceed affine_c (the nearest: 1.9e-4 against 5e-4 for the funnel at d = 160), so C_FIGURES holds no entry and no case runs
at a wider c.  tests/test_host_flow_mh_wide.py measures the figures again and holds the table to them.

The n = 700, T = 3 statistics cases run 6 matrix-core tiles (11 wave tiles) on as many workgroups: the sums of several
workgroups' slabs.  No shape up to n = 700 gives one workgroup a second tile (the grids hold 2048 and 256 workgroups)."""
import collections
import functools

import numpy as np
import pytest
import torch

import target_harness as H

pytestmark = pytest.mark.gpu

N, T = 150, 4
SEED, FLOW_SEED, STARTS_SEED = 11, 5, 3
MARGIN, FLOOR, CAP = 1e-3, 0.25, 0.10
MOMENT_RTOL = 1e-12                     # tests/test_gpu_jump_pipeline.py: fp64 partial sums added in another order
STATS_BOUND = 64 * 2.0 ** -24           # sum_x, sum_x2 against the fp64 sums of the kept states, times sum |v|: 'lane' adds
#                                         64 rows in fp32 before it goes to fp64; the other two are fp64 throughout

# (case id) -> worst fp32-against-fp64 |log q| difference of the oracle flow at the case's own proposals, CPU alone, for the
# cases where 4 x it exceeds affine_c(d): none (measured 1.6e-6 .. 1.1e-4 over the affine cases below)
C_FIGURES = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple('Case', 'kernel target d nh hl cl spline scale env n')


def _case(kernel, target, d, nh, hl=2, cl=2, *, spline=False, scale=0.05, env=None, n=N):
    return Case(kernel, target, d, nh, hl, cl, spline, scale, env, n)


def _id(c):
    return '%s-%s-d%d-h%dx%d-c%d%s%s%s' % (c.kernel, c.target, c.d, c.nh, c.hl, c.cl, '-spline' if c.spline else '',
                                           '' if c.env is None else '-' + c.env, '' if c.n == N else '-n%d' % c.n)


# (d, n_hidden, hidden layers, couplings)
MFMA = [_case('mfma', 'sumsq', 64, 33, 1, 2),            # the narrowest width, padded to 64
        _case('mfma', 'sumsq', 64, 64, 2, 2),
        _case('mfma', 'sumsq', 128, 128, 2, 2),
        _case('mfma', 'sumsq', 128, 40, 1, 3),           # odd coupling count: `rev`
        _case('mfma', 'sumsq', 64, 128, 2, 1),
        _case('mfma', 'funnel', 64, 40, 2, 2, scale=0.1),
        _case('mfma', 'funnel', 128, 128, 1, 2, scale=0.05),
        _case('mfma', 'quadratic', 64, 64, 1, 2),
        _case('mfma', 'diagonal', 128, 40, 2, 2),
        _case('mfma', 'sumsq', 64, 64, 2, 2, n=1)]
WIDE = [_case('wide', 'sumsq', 32, 33, 1, 2),            # the smallest d
        _case('wide', 'sumsq', 96, 64, 2, 2),
        _case('wide', 'sumsq', 160, 100, 1, 3),
        _case('wide', 'sumsq', 256, 128, 2, 2),
        _case('wide', 'sumsq', 512, 128, 2, 2, scale=0.02),
        _case('wide', 'funnel', 96, 64, 1, 2, scale=0.1),
        _case('wide', 'funnel', 160, 100, 2, 2, scale=0.05),
        _case('wide', 'quadratic', 96, 64, 1, 2),
        _case('wide', 'diagonal', 32, 33, 2, 2),
        _case('wide', 'sumsq', 32, 33, 1, 2, n=1)]
# The LDS bound of 'lane' (csrc/flow_kernels.hip: flow_mh_tile_lds): two 64-row tiles at tile_stride(d) floats a row, and
# at n_hidden = 128 the activation buffer hbuf of 128 x 64 floats: 2 * 64 * 4 * stride + 128 * 64 * 4 = 512 stride + 32768
# bytes <= 160 KB = 163840 asks stride <= 256.  tile_stride(d) is d rounded up to 4, plus 4 when a quarter of that is
# even, so it is 4 x an odd number: 252 = 4 x 63 for d = 245 .. 252 (161792 bytes), 260 = 4 x 65 for d = 253 .. 260
# (165888 bytes).  The largest d that fits is 252, the first that does not 253; neither is a multiple of 32.
LDS_FITS, LDS_REFUSED = 252, 253
LANE = [_case('lane', 'sumsq', 7, 4, env='tile'),        # HP = 4 and 8: the register kernel's widths, sent here
        _case('lane', 'sumsq', 7, 8, env='tile'),
        _case('lane', 'sumsq', 50, 4, env='tile'),
        _case('lane', 'sumsq', 50, 8, env='tile'),
        _case('lane', 'sumsq', 50, 16),                  # HP = 16
        _case('lane', 'sumsq', 25, 32),                  # HP = 32
        _case('lane', 'sumsq', 25, 32, 2, 3),            # odd coupling count
        _case('lane', 'sumsq', 200, 32),
        _case('lane', 'sumsq', 33, 40),                  # HP = 64, with hbuf
        _case('lane', 'sumsq', 100, 100),                # HP = 128
        _case('lane', 'sumsq', 64, 64, env='no_mfma'),   # a matrix-core shape kept off the matrix cores
        _case('lane', 'sumsq', 50, 16, spline=True),
        _case('lane', 'sumsq', 13, 32, spline=True),
        _case('lane', 'funnel', 25, 32, scale=0.1),
        _case('lane', 'funnel', 33, 40, scale=0.1),
        _case('lane', 'quadratic', 25, 32),
        _case('lane', 'diagonal', 33, 40),
        _case('lane', 'sumsq', 25, 32, n=1),
        _case('lane', 'sumsq', LDS_FITS, 128, scale=0.02)]
CASES = MFMA + WIDE + LANE
BY_ID = {_id(c): c for c in CASES}
assert len(BY_ID) == len(CASES)


def _pick(*ids):
    return [BY_ID[i] for i in ids]


# two shapes per kernel, an odd coupling count among them (the reversed replay order), and a spline
SUBSET = _pick('mfma-sumsq-d64-h64x2-c2', 'mfma-sumsq-d128-h40x1-c3', 'wide-sumsq-d96-h64x2-c2', 'wide-sumsq-d160-h100x1-c3',
               'lane-sumsq-d33-h40x2-c2', 'lane-sumsq-d25-h32x2-c3', 'lane-sumsq-d13-h32x2-c2-spline')
ONE_PER_KERNEL = _pick('mfma-sumsq-d128-h40x1-c3', 'wide-sumsq-d96-h64x2-c2', 'lane-sumsq-d33-h40x2-c2')
THROUGH_IMH = _pick('mfma-sumsq-d64-h33x1-c2', 'mfma-funnel-d64-h40x2-c2', 'wide-sumsq-d256-h128x2-c2', 'wide-funnel-d96-h64x1-c2',
                    'lane-sumsq-d50-h16x2-c2', 'lane-sumsq-d50-h16x2-c2-spline', 'lane-funnel-d33-h40x2-c2')


def _problem(target, d, n):
    """A harness Problem with a target object of its own (laplace_fit and local_fit cache by id(p.target)): the package
    potential, and the fp64 oracle potential on the package's own fp32 parameters."""
    from nfmc_amd.potentials import DiagonalGaussian, Funnel, QuadraticPotential, SumOfSquares
    from oracle import potentials as opot
    if target == 'sumsq':
        pot = SumOfSquares((d,))
        ref = lambda x: opot.sum_squares(x)                                                      # noqa: E731
    elif target == 'funnel':
        pot, ref = Funnel((d,), 3.0), opot.funnel(3.0)
    elif target == 'quadratic':
        pot = QuadraticPotential((d,), torch.linspace(0.5, 2.0, d), torch.linspace(-1.0, 1.0, d))
        ref = opot.quadratic(pot.a, pot.b)
    else:
        pot = DiagonalGaussian((d,), mu=torch.linspace(-2.0, 2.0, d), sigma=torch.linspace(0.5, 1.5, d))
        ref = opot.quadratic(pot.a, pot.b)
    x0 = 0.7 * torch.randn(n, d, generator=torch.Generator().manual_seed(1000 * d + n))
    return H.Problem(pot, ref, ref, x0, d, '%s d=%d' % (target, d))


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """(problem at its centred starts, (package flow, fp64 oracle flow)) of a case; shared and read-only"""
    p = _problem(c.target, c.d, c.n)
    centre = H.local_fit(p, 0.3) if c.target == 'funnel' else None
    flows = H.centred_flow_pair(p, FLOW_SEED, c.nh, c.spline, c.cl, scale=c.scale, centre=centre, hidden_layers=c.hl)
    return H.centred(p, c.n, STARTS_SEED, centre), flows


@functools.lru_cache(maxsize=None)
def _oracle(c, steps=T, adjusted=True):
    from oracle import samplers as osamp
    q, (_f, of) = _inputs(c)
    return osamp.imh_sample(q.x0.double(), q.target, of, steps, noise=osamp.PhiloxNoise(SEED, dtype=torch.float64), adjusted=adjusted)


def _conditions(c, tr):
    """the conditions on a case's inputs, from the fp64 oracle alone; True when the caller is to stop there (the host file)"""
    H.oracle_inputs_ok(tr.flow_steps, _id(c), margin=MARGIN, floor=FLOOR, cap=CAP, skip_below_minus_50=c.target == 'funnel')
    return H._ORACLE_ONLY[0]


def _enter(dev, monkeypatch, c):
    """the case's environment, and the assertion that its kernel is the one that runs"""
    q, (f, _of) = _inputs(c)
    monkeypatch.delenv('NFMC_FLOW_TILE_PATH', raising=False)
    monkeypatch.delenv('NFMC_FLOW_NO_MFMA', raising=False)
    if c.env is not None:
        monkeypatch.setenv({'tile': 'NFMC_FLOW_TILE_PATH', 'no_mfma': 'NFMC_FLOW_NO_MFMA'}[c.env], '1')
    got = H.flow_mh_kernel_of(dev, q, f)
    assert got == c.kernel, (_id(c), got)
    return q, f


def _c(c, of, steps):
    if c.spline:
        return H.spline_c(c.d, of, steps)[0]
    return max(H.affine_c(c.d), H.SPLINE_C_FACTOR * C_FIGURES.get(_id(c), 0.0))


_base_runs = {}


def _base(dev, monkeypatch, c, steps=T):
    """The case's launch of `steps` transitions on the native streams with immediate statistics, once; the tests that
    compare another launch against it share it."""
    q, f = _enter(dev, monkeypatch, c)
    key = (c, steps)
    if key not in _base_runs:
        _base_runs[key] = H._direct_flow_mh(dev, q, f, steps, SEED, True, stats='immediate')
    return _base_runs[key]


def _check_stats(r, n, steps, what):
    st = r.stats
    assert st['accepted'] == int(r.masks.sum()), (what, st['accepted'], int(r.masks.sum()))
    assert st['attempted'] == n * steps, (what, st['attempted'])
    assert st['nonfinite'] == 0, (what, st['nonfinite'])
    kept = r.samples.double()
    for name, v in (('sum_x', kept), ('sum_x2', kept * kept)):
        want, bound = v.sum((0, 1)), STATS_BOUND * v.abs().sum((0, 1))
        err = (st[name].double() - want).abs()
        print('%s: %s worst error over bound %.3f' % (what, name, float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (what, name, float(err.max()))


def _follow_and_compare(c, r, tr):
    """decisions and log ratios, kept states of the chains that followed, the logq write-back; the worst ratio"""
    q, (_f, of) = _inputs(c)
    what, cc = _id(c), _c(c, of, tr.flow_steps)
    follows, ratio = H.compare_flow_mh(r.masks, r.log_ratios, tr.flow_steps, what, c=cc, margin=MARGIN, floor=FLOOR, cap=CAP,
                                       skip_below_minus_50=c.target == 'funnel')
    print('%s: worst log-ratio error over tolerance %.3f (c = %.1e)' % (what, ratio, cc))
    assert bool(follows.any()), what
    assert bool(torch.isfinite(r.samples).all()) and torch.equal(r.x, r.samples[-1]), what
    want = tr.stacked().float()
    np.testing.assert_allclose(r.samples[:, follows].numpy(), want[:, follows].numpy(), atol=3e-5 * max(1.0, c.d / 64), rtol=0,
                               err_msg=what)
    last = tr.flow_steps[-1]
    want_lq = torch.where(last.mask, last.f_xp, last.f_x).double()          # the log q the oracle carries out of the run
    tol = H.flow_mh_tolerance(tr.flow_steps, cc)[-1]
    err = (r.logq.double() - want_lq).abs()
    assert bool((err[follows] <= tol[follows]).all()), (what, 'logq', float(err[follows].max()))
    return ratio


# ------------------------------------------------------------------------------------------------ one launch
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_one_launch_follows_the_oracle_row_by_row(dev, monkeypatch, case):
    """T transitions of one nfmc_flow_mh_steps_f32 launch: every decision and log ratio, the kept states, the log q the
    launch writes back, and the immediate statistics (accepted = the kernel's own masks, attempted n T, no non-finite
    ratio, the sums of the kernel's own kept states)."""
    tr = _oracle(case)
    if _conditions(case, tr):
        return
    r = _base(dev, monkeypatch, case)
    _follow_and_compare(case, r, tr)
    _check_stats(r, case.n, T, _id(case))


@pytest.mark.parametrize('case', SUBSET, ids=_id)
def test_unadjusted_launch_keeps_every_proposal_and_carries_u_and_log_q(dev, monkeypatch, case):
    """adjusted = 0: every mask 1, the kept states the fp64 flow's samples at the same latents, and the log ratio of
    transition s + 1, which uses the U and log q carried from s, follows the oracle's on every row."""
    q, (_f, of) = _inputs(case)
    tr = _oracle(case, T, False)
    lr = torch.stack([js.log_alpha for js in tr.flow_steps])
    print('%s: unadjusted, log ratios %.1f .. %.1f' % (_id(case), float(lr.min()), float(lr.max())))
    assert bool(torch.isfinite(lr).all()), _id(case)
    if H._ORACLE_ONLY[0]:
        return
    q, f = _enter(dev, monkeypatch, case)
    got, got_m, got_lr = H._direct_flow_mh(dev, q, f, T, SEED, False)
    H.compare_flow_mh(got_m, got_lr, tr.flow_steps, _id(case), c=_c(case, of, tr.flow_steps), margin=0.0, adjusted=False)
    want = torch.stack([js.x_prime for js in tr.flow_steps]).float()
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=3e-5 * max(1.0, case.d / 64), rtol=0, err_msg=_id(case))


@pytest.mark.parametrize('case', SUBSET, ids=_id)
def test_cached_log_q_gives_the_uncached_launch(dev, monkeypatch, case):
    """logq_cached = 1 with log q of the starts from flow.log_prob: masks and kept states equal the uncached launch bit
    for bit, the log ratios agree to the row tolerance."""
    tr = _oracle(case)
    if _conditions(case, tr):
        return
    q, (_f, of) = _inputs(case)
    base = _base(dev, monkeypatch, case)
    q, f = _enter(dev, monkeypatch, case)
    with torch.no_grad():
        lq = f.log_prob(q.x0.to(dev)).detach().float()
    r = H._direct_flow_mh(dev, q, f, T, SEED, True, cached=lq)
    assert torch.equal(r.masks, base.masks) and torch.equal(r.samples, base.samples), _id(case)
    tol = H.flow_mh_tolerance(tr.flow_steps, _c(case, of, tr.flow_steps))
    err = (r.log_ratios.double() - base.log_ratios.double()).abs()
    assert bool((err <= tol).all()), (_id(case), float(err.max()))
    assert bool((r.logq.double() - base.logq.double()).abs().le(tol[-1]).all()), _id(case)


@pytest.mark.parametrize('case', SUBSET, ids=_id)
def test_replayed_noise_gives_the_native_launch(dev, monkeypatch, case):
    """The draws of the native streams handed in as replay_normals / replay_uniforms, under another seed: states, masks,
    log ratios and the written log q equal the native-stream launch bit for bit (an odd coupling count reads the latents
    in reversed order).  The uniforms are the oracle's recorded PhiloxNoise draws, which are the kernels' exactly.  Its
    recorded normals are not: oracle/philox.py rounds fp64 transcendentals once where the device uses its own, and says
    so (about 1e-6 absolute, not bitwise), so no launch on them can give the native launch's bits.  The latents of the
    bit-for-bit leg are therefore the device's own draws of the same stream (nfmc_philox_normals_f32, TAG_LATENT), held
    to the recorded ones to 1e-5; the recorded normals themselves are replayed too, and that launch is held to the oracle
    row by row like the native one."""
    import ctypes as C
    from nfmc_amd import hip
    from oracle import samplers as osamp
    tr = _oracle(case)
    if _conditions(case, tr):
        return
    q, (_f, of) = _inputs(case)
    rec = osamp.RecordingNoise(osamp.PhiloxNoise(SEED, dtype=torch.float64))
    osamp.imh_sample(q.x0.double(), q.target, of, T, noise=rec)
    recorded, uniforms = torch.stack(rec.normals).float(), torch.stack(rec.uniforms).float()
    base = _base(dev, monkeypatch, case)
    q, f = _enter(dev, monkeypatch, case)
    native = torch.empty(T, case.n, case.d, device=dev)
    for s in range(T):
        rng = hip.make_rng(SEED, 0, s)
        hip.check(hip.lib().nfmc_philox_normals_f32(C.byref(rng), hip.TAG_LATENT, case.n, case.d, hip.ptr(native[s]), hip.stream()),
                  'nfmc_philox_normals_f32')
    native = native.cpu()
    assert float((native - recorded).abs().max()) < 1e-5, _id(case)
    r = H._direct_flow_mh(dev, q, f, T, SEED + 1, True, replay=(native, uniforms))
    for name in ('samples', 'masks', 'log_ratios', 'logq', 'x'):
        assert torch.equal(getattr(r, name), getattr(base, name)), (_id(case), name)
    r = H._direct_flow_mh(dev, q, f, T, SEED + 1, True, replay=(recorded, uniforms))
    _follow_and_compare(case, r, tr)


@pytest.mark.parametrize('case', ONE_PER_KERNEL, ids=_id)
def test_deferred_statistics_fold_to_the_immediate_ones(dev, monkeypatch, case):
    """struct(defer=True) and the fold: the same counters and, against the launch's own kept states, the same bound."""
    tr = _oracle(case)
    if _conditions(case, tr):
        return
    base = _base(dev, monkeypatch, case)
    q, f = _enter(dev, monkeypatch, case)
    r = H._direct_flow_mh(dev, q, f, T, SEED, True, stats='deferred')
    assert torch.equal(r.samples, base.samples) and torch.equal(r.masks, base.masks), _id(case)
    _check_stats(r, case.n, T, _id(case) + ' deferred')


@pytest.mark.parametrize('case', ONE_PER_KERNEL, ids=_id)
def test_statistics_slabs_are_overwritten_at_once_and_added_to_when_deferred(dev, monkeypatch, case):
    """Every word of the statistics scratch set to 1 before the launch.  An immediate launch owns its slabs (the first
    transition of a workgroup writes, the later ones add; the fold that follows reads the launch's slabs alone): the totals
    are the clean launch's bit for bit.  A deferred launch adds to slabs that other launches of the run have written to,
    and the fold reads every slab: each total grows by the number of slabs, the counters of the launch's own tail slots
    (accepted, non-finite) too.  The sums are fp64 sums of the same terms and the slabs' ones in one fixed order: 1e-12 of
    their size covers the 2048 additions."""
    from nfmc_amd import hip
    tr = _oracle(case)
    if _conditions(case, tr):
        return
    base = _base(dev, monkeypatch, case)
    q, f = _enter(dev, monkeypatch, case)
    dp = 4
    while dp < case.d:
        dp *= 2                                                   # csrc/common.hpp: padded_d
    words = int(hip.lib().nfmc_stats_scratch_bytes(case.d)) // 8
    slabs, rest = divmod(words, 2 * dp + 4)
    assert rest == 0 and slabs >= 256, (words, dp)
    r = H._direct_flow_mh(dev, q, f, T, SEED, True, stats='immediate', prefill=1.0)
    assert r.stats['accepted'] == base.stats['accepted'] and r.stats['attempted'] == case.n * T and r.stats['nonfinite'] == 0
    assert torch.equal(r.stats['sum_x'], base.stats['sum_x']) and torch.equal(r.stats['sum_x2'], base.stats['sum_x2']), _id(case)
    r = H._direct_flow_mh(dev, q, f, T, SEED, True, stats='deferred', prefill=1.0)
    assert torch.equal(r.masks, base.masks) and torch.equal(r.samples, base.samples), _id(case)
    assert r.stats['accepted'] == base.stats['accepted'] + slabs and r.stats['nonfinite'] == slabs, (_id(case), r.stats['accepted'])
    assert r.stats['attempted'] == case.n * T
    for name in ('sum_x', 'sum_x2'):
        want = base.stats[name].double() + slabs
        assert bool(((r.stats[name].double() - want).abs() <= 1e-12 * (want.abs() + slabs)).all()), (_id(case), name)


@pytest.mark.parametrize('case', ONE_PER_KERNEL, ids=_id)
@pytest.mark.parametrize('mode', ['immediate', 'deferred'])
def test_statistics_over_several_workgroups(dev, monkeypatch, case, mode):
    """n = 700, T = 3: the totals are sums over the slabs of 6 (11 for 'lane') workgroups."""
    big = case._replace(n=700)
    tr = _oracle(big, 3)
    if _conditions(big, tr):
        return
    q, f = _enter(dev, monkeypatch, big)
    r = H._direct_flow_mh(dev, q, f, 3, SEED, True, stats=mode)
    _follow_and_compare(big, r, tr)
    _check_stats(r, 700, 3, '%s %s' % (_id(big), mode))


def _window(dense, thinning, max_samples):
    """MCMCSamples.add's rule (tests/test_gpu_configs.py: _reference_window)"""
    idx = [i for i in range(dense.shape[0]) if i % thinning == 0]
    return dense[idx[-max_samples:] if max_samples else idx]


@pytest.mark.parametrize('case', ONE_PER_KERNEL, ids=_id)
def test_thinned_windowed_store_is_the_dense_run_cut(dev, monkeypatch, case):
    """thinning = 3, max_samples = 2 over T = 7: the slab equals the dense run's transitions 3 and 6, bit for bit."""
    tr = _oracle(case, 7)
    if _conditions(case, tr):
        return
    dense = _base(dev, monkeypatch, case, 7)
    _follow_and_compare(case, dense, tr)
    q, f = _enter(dev, monkeypatch, case)
    r = H._direct_flow_mh(dev, q, f, 7, SEED, True, store=(3, 2))
    assert r.samples.shape == (2, case.n, case.d)
    assert torch.equal(r.samples, _window(dense.samples, 3, 2)), _id(case)
    assert torch.equal(r.masks, dense.masks) and torch.equal(r.x, dense.x) and torch.equal(r.logq, dense.logq), _id(case)


@pytest.mark.parametrize('case', ONE_PER_KERNEL, ids=_id)
def test_two_launches_of_the_same_arguments_give_the_same_bits(dev, monkeypatch, case):
    tr = _oracle(case)
    if _conditions(case, tr):
        return
    base = _base(dev, monkeypatch, case)
    q, f = _enter(dev, monkeypatch, case)
    r = H._direct_flow_mh(dev, q, f, T, SEED, True, stats='immediate')
    for name in ('samples', 'masks', 'log_ratios', 'logq', 'x'):
        assert torch.equal(getattr(r, name), getattr(base, name)), (_id(case), name)
    assert r.stats['accepted'] == base.stats['accepted'] and torch.equal(r.stats['sum_x'], base.stats['sum_x']) \
        and torch.equal(r.stats['sum_x2'], base.stats['sum_x2']), _id(case)


# ------------------------------------------------------------------------------------------------ through FixedIMH
def _compare_states(c):
    return lambda got, tr, what: H.compare_states(got, tr, what, margin=MARGIN, atol=3e-5 * max(1.0, c.d / 64), rtol=0.0)


@pytest.mark.parametrize('case', THROUGH_IMH, ids=_id)
def test_fixed_imh_on_the_kernel_follows_the_oracle(dev, monkeypatch, case):
    """FixedIMH (flow_mh_matches_oracle): the sampler's launches recorded, rows, kept states and counters."""
    q, flows = _inputs(case)
    if not H._ORACLE_ONLY[0]:
        _enter(dev, monkeypatch, case)
    H.flow_mh_matches_oracle(monkeypatch, q, flows, T=T, seed=SEED, spline=case.spline, what=_id(case), compare=_compare_states(case),
                             margin=MARGIN, skip_below_minus_50=case.target == 'funnel', floor=FLOOR)


def _without_workspace(monkeypatch, f):
    """the package flow presenting itself without the streamed kernels' workspace (NfmcRealNVP.scratch NULL)"""
    from nfmc_amd import hip
    packed = f.bijection.packed

    def bare(device, min_hidden=None):
        st, keep = packed(device, min_hidden)
        st = hip.NfmcRealNVP.from_buffer_copy(st)
        st.scratch, st.scratch_bytes = None, 0
        return st, keep
    monkeypatch.setattr(f.bijection, 'packed', bare)


def test_streamed_shape_without_a_workspace_is_refused_and_composed(dev, monkeypatch):
    """flow.scratch NULL at a shape of the streamed kernel: the probe answers NFMC_EUNSUPPORTED, FixedIMH composes every
    transition (split_flow_mh) and the kept states still follow the oracle."""
    case = BY_ID['wide-sumsq-d96-h64x2-c2']
    q, (_f, of) = _inputs(case)
    f = None
    if not H._ORACLE_ONLY[0]:
        from nfmc_amd.flows import Flow, RealNVP
        _enter(dev, monkeypatch, case)
        f = Flow(RealNVP((case.d,), n_layers=case.cl, conditioner_kwargs={'n_hidden': case.nh, 'n_layers': case.hl}))
        f.load_state_dict({k: v.float() for k, v in of.state_dict().items()})
        _without_workspace(monkeypatch, f)
        assert H.flow_mh_kernel_of(dev, q, f) is None
    H.flow_mh_matches_oracle(monkeypatch, q, (f, of), T=T, seed=SEED, spline=False, what=_id(case) + ' no workspace',
                             compare=_compare_states(case), margin=MARGIN, skip_below_minus_50=False, floor=FLOOR, refused=True, dev=dev)


def test_first_d_past_the_lds_bound_is_refused_and_composed(dev, monkeypatch):
    """d = 253 at width 128 (LDS_REFUSED: 165888 bytes of LDS): the probe refuses, the run is composed and still follows the
    oracle.  d = 252, the largest that fits, is a case of the matrix above."""
    case = _case('lane', 'sumsq', LDS_REFUSED, 128, scale=0.02)
    q, flows = _inputs(case)
    if not H._ORACLE_ONLY[0]:
        monkeypatch.delenv('NFMC_FLOW_TILE_PATH', raising=False)
        monkeypatch.delenv('NFMC_FLOW_NO_MFMA', raising=False)
        assert H.flow_mh_kernel_of(dev, q, flows[0]) is None
        fits = BY_ID['lane-sumsq-d%d-h128x2-c2' % LDS_FITS]
        assert H.flow_mh_kernel_of(dev, *(_inputs(fits)[0], _inputs(fits)[1][0])) == 'lane'
    H.flow_mh_matches_oracle(monkeypatch, q, flows, T=T, seed=SEED, spline=False, what=_id(case), compare=_compare_states(case),
                             margin=MARGIN, skip_below_minus_50=False, floor=FLOOR, refused=True, dev=dev)


# ------------------------------------------------------------------------------------------------ through the jump samplers
JUMPS = [('mala', BY_ID['mfma-sumsq-d64-h64x2-c2']), ('hmc', _case('wide', 'sumsq', 96, 64, 1, 2)), ('mala', BY_ID['lane-sumsq-d50-h16x2-c2'])]


@pytest.mark.parametrize('inner,case', JUMPS, ids=['%s-%s' % (k, _id(c)) for k, c in JUMPS])
def test_jump_sampler_jumps_on_the_kernel_follow_the_oracle(dev, monkeypatch, inner, case):
    """jump_mala / jump_hmc (L = 3), T = 3 outer iterations of K = 3 inner transitions, every jump a launch_flow_mh on the
    case's kernel.  Step sizes: U = sum x^2 has the Hessian 2 I, so h = 0.3 d^(-1/3) / 2 (MALA) and 0.5 d^(-1/4) / sqrt(2)
    (HMC), the per-target files' rule."""
    q, flows = _inputs(case)
    if not H._ORACLE_ONLY[0]:
        _enter(dev, monkeypatch, case)
    h = 0.3 * case.d ** (-1 / 3) / 2.0 if inner == 'mala' else 0.5 * case.d ** (-1 / 4) / 2.0 ** 0.5
    H.jump_matches_oracle(monkeypatch, q, inner, T=3, Kin=3, seed=SEED, h=h, imd=None, fuse_tail=False, spline=False, atol=1e-3,
                          rtol=1e-4, share=0.95, jump_slack=2, margin=MARGIN, skip_below_minus_50=False, L=3, flows=flows,
                          floor=FLOOR, tail_expected=False)


JUMP_COUNTERS = ('n_accepted_trajectories', 'n_attempted_trajectories', 'n_accepted_jumps', 'n_attempted_jumps',
                 'n_nonfinite_log_ratios', 'n_divergences', 'n_target_calls', 'n_target_gradient_calls')


@pytest.mark.parametrize('parts', [1, 2, 4])
def test_whole_run_call_without_a_register_jump_falls_back_to_one_part(dev, monkeypatch, parts):
    """jump_mala with store_samples=False and no progress bar on the (64, 64) flow goes through nfmc_jump_run_f32; the jump
    has no register kernel, so whatever jump_parts asks the call runs as one part: last states and counters equal the
    host loop's (time_kernels=True) bit for bit, the moments within MOMENT_RTOL."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    case = BY_ID['mfma-sumsq-d64-h64x2-c2']._replace(n=700)
    q, f = _enter(dev, monkeypatch, case)
    calls, real = [], jump.launch_jump_run
    monkeypatch.setattr(jump, 'launch_jump_run', lambda *a: calls.append(a[6:9]) or real(*a))
    outs = []
    for host_loop in (False, True):
        s = jump.JumpMALA((case.d,), q.pot, NFMCKernel((case.d,), flow=f), jump.JumpNFMCParameters(n_iterations=4, store_samples=False),
                          None, mcmc.LangevinParameters(n_iterations=3))
        s.seed, s.jump_parts = 424242, parts
        if host_loop:
            s.time_kernels = True
        out = s.sample(q.x0, show_progress=False)
        outs.append(out)
    assert calls == [(3, 3, parts)], calls                      # the first run alone took the whole-run call
    a, b = outs
    assert torch.equal(a.running_samples.last_sample, b.running_samples.last_sample)
    ca, cb = ({k: getattr(o.statistics, k) for k in JUMP_COUNTERS} for o in outs)
    assert ca == cb, (ca, cb)
    assert ca['n_attempted_jumps'] == 700 * 4 and 0 < ca['n_accepted_jumps'] < 700 * 4
    for name in ('first_moment', 'second_moment'):
        ea, eb = a.statistics.expectations[name], b.statistics.expectations[name]
        assert ea.n_seen == eb.n_seen == 700 * 4 * 4
        rel = float(((ea.total - eb.total).abs() / eb.total.abs()).max())
        print(name, 'relative difference', rel)
        assert rel <= MOMENT_RTOL, (name, rel)


# the tests whose inputs tests/test_host_flow_mh_wide.py runs through the fp64 oracle alone (probe_flow_inputs)
FLOW_TESTS = ('test_one_launch_follows_the_oracle_row_by_row', 'test_unadjusted_launch_keeps_every_proposal_and_carries_u_and_log_q',
              'test_cached_log_q_gives_the_uncached_launch', 'test_replayed_noise_gives_the_native_launch',
              'test_deferred_statistics_fold_to_the_immediate_ones', 'test_statistics_slabs_are_overwritten_at_once_and_added_to_when_deferred',
              'test_statistics_over_several_workgroups',
              'test_thinned_windowed_store_is_the_dense_run_cut', 'test_two_launches_of_the_same_arguments_give_the_same_bits',
              'test_fixed_imh_on_the_kernel_follows_the_oracle', 'test_streamed_shape_without_a_workspace_is_refused_and_composed',
              'test_first_d_past_the_lds_bound_is_refused_and_composed', 'test_jump_sampler_jumps_on_the_kernel_follow_the_oracle')
N_FLOW_CASES = len(CASES) + 3 * len(SUBSET) + 4 * len(ONE_PER_KERNEL) + 2 * len(ONE_PER_KERNEL) + len(THROUGH_IMH) + 2 + len(JUMPS)
