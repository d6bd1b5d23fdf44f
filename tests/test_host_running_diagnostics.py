"""CPU: the running diagnostics of runs that keep no states.  The stream algebra, restated in numpy
(running_fp64.py), against the fp64 oracle on the concatenated draws (diagnostics_fp64.py); the parameter's validation;
the planning arithmetic of the streaming store; an early end."""
import math
import re
import os

import numpy as np
import pytest
import torch

import diagnostics_fp64 as ref
import running_fp64 as stream
from nfmc_amd import diagnostics, hip
from nfmc_amd.containers import MCMCOutput, MCMCParameters, StreamingSampleStore, running_lags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ('sum_m', 'sum_m2', 'sum_mh', 'sum_mh2', 'sum_s2h', 'sum_mu', 'sum_mu2', 'sum_bt')


def agree(got, want, tol=1e-12):
    """Every row within `tol` of its own scale (the largest magnitude of the oracle's row, of lag 0 for the lags)."""
    for name in ROWS:
        scale = np.abs(want[name]).max() + 1e-300
        assert np.abs(got[name] - want[name]).max() <= tol * scale, name
    assert got['acov'].shape == want['acov'].shape
    assert np.abs(got['acov'] - want['acov']).max() <= tol * (np.abs(want['acov'][0]).max() + 1e-300)


CASES = [
    # K, n, d, L, blocks, mean, sd
    (37, 6, 3, 12, [1, 5, 13, 2, 16], 0.3, 1.5),      # a block of one, blocks shorter and longer than L, one across h = 18, odd K
    (300, 4, 2, 127, [32] * 9 + [12], 0.3, 1.5),
    (37, 6, 3, 0, [1, 5, 13, 2, 16], 0.3, 1.5),
    (5, 6, 3, 8, [1] * 5, 0.3, 1.5),                  # lags at or beyond K
    (37, 6, 3, 12, [1, 5, 13, 2, 16], 1000.0, 1.5),
]


@pytest.mark.parametrize('K,n,d,L,blocks,mean,sd', CASES)
def test_the_stream_algebra_agrees_with_the_oracle(K, n, d, L, blocks, mean, sd):
    x = ref.ar1(np.random.default_rng(K + L), K, n, d, 0.6, mean=mean, sd=sd)
    for group in (1, 2):
        got = stream.feed(x, blocks, L, group=group)
        agree(got, ref.sums(x, L, group))
        assert (got['acov'][K:] == 0).all()
    # the cut into blocks does not enter
    whole = stream.feed(x, [K], L)
    agree(stream.feed(x, blocks, L), whole, 1e-13)


def test_a_constant_coordinate_is_exact():
    x = ref.ar1(np.random.default_rng(2), 37, 6, 3, 0.6, mean=0.3, sd=1.5)
    x[:, :, 1] = 2.5
    got = stream.feed(x, [1, 5, 13, 2, 16], 12)
    assert (got['acov'][:, 1] == 0).all() and got['sum_s2h'][1] == 0 and got['sum_m'][1] == 6 * 2.5
    agree(got, ref.sums(x, 12))
    d = diagnostics.from_sums({k: torch.from_numpy(v) for k, v in got.items()}, 37, 6)
    assert math.isnan(d.rhat[1]) and not math.isnan(d.rhat[0])


def test_fp32_rounded_shifted_draws_stay_inside_the_autocovariance_bound():
    """The model with the shifted draws rounded to fp32 for products and rows, totals in fp64: what the kernel would give
    with exact sums inside a block."""
    x = ref.ar1(np.random.default_rng(5), 300, 4, 2, 0.9, mean=1000.0, sd=1.5)
    got = stream.feed(x, [32] * 9 + [12], 127, dtype=np.float32)
    want = ref.sums(x, 127)
    assert (np.abs(got['acov'] - want['acov']) / want['acov'][0]).max() <= 1.4e-6 / 4
    for name in ('sum_m', 'sum_mh', 'sum_s2h'):
        assert np.abs(got[name] - want[name]).max() <= 1e-12 * np.abs(want[name]).max()


def test_an_early_end_has_no_rhat_and_everything_else_of_the_draws_seen():
    x = ref.ar1(np.random.default_rng(7), 40, 6, 3, 0.6, mean=0.3, sd=1.5)
    got = stream.feed(x[:25], [7, 18], 12, n_planned=40, group=2)
    want = ref.sums(x[:25], 12, 2)
    for name in ('sum_mh', 'sum_mh2', 'sum_s2h'):
        assert np.isnan(got[name]).all()
        got[name] = want[name]
    agree(got, want)
    got.update({k: np.full(3, np.nan) for k in ('sum_mh', 'sum_mh2', 'sum_s2h')})
    d = diagnostics.from_sums({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in got.items()}, 25, 6, 2)
    w = ref.direct(x[:25], 12, 2)
    assert torch.isnan(d.rhat).all() and d.n_draws == 25
    for name in ('nested_rhat', 'ess', 'mcse_mean', 'mean', 'sd'):
        assert np.allclose(getattr(d, name).numpy(), w[name], rtol=1e-10, atol=0), name
    assert np.allclose(d.autocorrelation.numpy(), w['autocorrelation'], rtol=0, atol=1e-10)
    assert (d.truncated.numpy() == w['truncated']).all()


# ---- parameter validation
def test_the_parameter_is_validated():
    assert MCMCParameters().running_diagnostics is False and running_lags(MCMCParameters(), 100) is None
    with pytest.raises(ValueError, match='store_samples'):
        MCMCParameters(running_diagnostics=True)
    with pytest.raises(ValueError, match='store_samples'):
        MCMCParameters(running_diagnostics=0)                     # 0 lags is on
    for bad in (-1, 128, 3.5):
        with pytest.raises(ValueError, match='0 .. 127'):
            MCMCParameters(store_samples=False, running_diagnostics=bad)
    p = MCMCParameters(store_samples=False, running_diagnostics=True)
    assert running_lags(p, 2000) == 127 and running_lags(p, 37) == 36 and running_lags(p, 1) == 0
    assert running_lags(MCMCParameters(store_samples=False, running_diagnostics=12), 5) == 12
    assert running_lags(MCMCParameters(store_samples=False, running_diagnostics=0), 5) == 0
    p.store_samples = True                                         # changed after construction: refused when the run starts
    with pytest.raises(ValueError, match='store_samples'):
        running_lags(p, 10)


class FakeAccumulator:
    n, d, max_lag, n_seen, device = 4, 2, 12, 30, 'cpu'

    def sums(self, group=1):
        x = ref.ar1(np.random.default_rng(1), 30, 4, 2, 0.5)
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ref.sums(x, 12, group).items()}


def test_output_of_a_running_run():
    out = MCMCOutput((2,), store_samples=False, running=FakeAccumulator())
    with pytest.raises(ValueError, match='store_samples'):
        out.diagnostics(rank_normalized=True)
    with pytest.raises(ValueError, match='max_lag'):
        out.diagnostics(max_lag=13)
    with pytest.raises(ValueError):
        out.diagnostics(max_lag=-1)
    with pytest.raises(ValueError, match='superchains'):
        out.diagnostics(superchains=3)
    full = out.diagnostics(superchains=2)
    assert full.n_draws == 30 and full.n_chains == 4 and full.max_lag == 12 and full.nested_rhat is not None
    few = out.diagnostics(max_lag=5)
    assert few.max_lag == 5 and few.nested_rhat is None
    assert torch.equal(few.autocorrelation, full.autocorrelation[:6])
    short = FakeAccumulator()
    short.n_seen = 3
    with pytest.raises(ValueError, match='at least 4'):
        MCMCOutput((2,), store_samples=False, running=short).diagnostics()
    # without an accumulator nothing changed
    with pytest.raises(ValueError, match='run with store_samples=True'):
        MCMCOutput((2,), store_samples=False).diagnostics()


# ---- the streaming store's planning arithmetic
class Recorder:
    def __init__(self):
        self.blocks = []

    def update(self, ring, row, n_rows, first_draw):
        assert ring.shape[0] == 4 and 0 <= row < 4 and 1 <= n_rows <= 4
        rows = [(row + r) % 4 for r in range(n_rows)]
        self.blocks.append((first_draw, n_rows, [int(ring[r, 0, 0]) for r in rows]))


@pytest.mark.parametrize('thinning', [1, 3])
@pytest.mark.parametrize('launches', [[4, 4, 4, 4], [1, 3, 2, 4, 1, 1, 4], [3, 4, 2, 1, 4, 4, 1]])
def test_every_kept_draw_reaches_the_accumulator_once_and_in_order(thinning, launches):
    """A launch is simulated by writing the global transition index into the ring rows its plan names, as the kernels
    do (NfmcSampleStore: countdown, stride, row, ring_rows)."""
    launches = [k * thinning if i % 2 else max(1, k * thinning - 1) for i, k in enumerate(launches)]
    total = sum(launches)
    rec = Recorder()
    store = StreamingSampleStore(1, 1, 'cpu', total, thinning, stage_rows=4, acc=rec)
    assert store.rows == min(4, -(-total // thinning)) == 4 and store.max_offer == 4 * thinning
    done = 0
    for i, k in enumerate(launches):
        if i % 3 == 2:   # a host-driven path offers dense states
            store.add_dense(torch.arange(done, done + k, dtype=torch.float32).reshape(k, 1, 1))
        else:
            stride, countdown, ring_rows, row = store.plan(k)
            assert stride == thinning and ring_rows == 4
            for j in range(countdown, k, stride):
                assert (done + j) % thinning == 0
                store.buf[row, 0, 0] = done + j
                row = (row + 1) % ring_rows
        done += k
    store.flush()
    store.flush()   # nothing left: no empty block
    kept = list(range(0, total, thinning))
    firsts = [b[0] for b in rec.blocks]
    assert firsts == [sum(b[1] for b in rec.blocks[:i]) for i in range(len(rec.blocks))]   # first_draw counts up, no gap
    assert [v for b in rec.blocks for v in b[2]] == kept                                    # each kept index once, in order
    assert store.fed == len(kept) == store.planned


def test_a_launch_that_keeps_more_than_the_ring_holds_is_refused():
    store = StreamingSampleStore(1, 1, 'cpu', 100, 3, stage_rows=4, acc=Recorder())
    store.plan(12)
    with pytest.raises(RuntimeError, match='staging ring'):
        store.plan(13)
    big = StreamingSampleStore(1, 1, 'cpu', 100, 1, stage_rows=4, acc=Recorder())
    big.add_dense(torch.arange(11, dtype=torch.float32).reshape(11, 1, 1))   # dense offers are cut by the store itself
    big.flush()
    assert [v for b in big.acc.blocks for v in b[2]] == list(range(11))


# ---- the ABI
def test_the_abi_declares_the_stream_entry_points():
    names = {s[0] for s in hip.SYMBOLS}
    for fn in ('nfmc_diag_stream_state_bytes', 'nfmc_diag_stream_work_bytes', 'nfmc_diag_stream_reset_f32',
               'nfmc_diag_stream_update_f32', 'nfmc_diag_stream_sums_f32'):
        assert fn in names, fn
    src = open(os.path.join(ROOT, 'nfmc_amd', 'csrc', 'diag_stream.hpp')).read()
    assert not re.search(r'#include\s+"pot_', src)
    assert '#include "diag_stream.hpp"' in open(os.path.join(ROOT, 'nfmc_amd', 'csrc', 'misc_kernels.hip')).read()
