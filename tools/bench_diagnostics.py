"""Time nfmc_chain_diagnostics_f32 over a resident slab against the same sums composed from torch ops.

    python tools/bench_diagnostics.py [--shapes 100x65536x64,100x8192x512] [--max-lag 99] [--reps 5]

Per shape: median of `reps` calls after one warm-up, device events around the library call alone (buffers allocated
before); the bytes of the slab over that time next to the 6.3 TB/s streaming figure (the kernel reads the slab twice, so
half of it is its ceiling); and the torch composition -- centred draws, one elementwise product and reduction per lag
-- in the same process.  Prints one JSON line per shape.  Needs the GPU: there is no fallback.

    python tools/bench_diagnostics.py --rank [--shapes ...]

times the rank transform instead: the four series of nfmc_rank_series_f32 into one slab, and the whole
`diagnose(..., rank_normalized=True)` call (the plain sums, the four transforms, their four sums, the host part), each next
to the same results composed from torch ops on the device (torch.sort per coordinate, searchsorted, torch.special.ndtri,
and `torch_sums` for every series).

    python tools/bench_diagnostics.py --running [--shapes 65536x64,8192x512] [--lags 0,31,127] [--stage-rows 32,128]

times the running diagnostics of runs that keep no states: nfmc_diag_stream_update_f32 per kept draw (a block of
`stage_rows` draws from a resident ring, device events around the call, median of `reps`), and, with --through-sample,
whole `sample()` calls of jump_mala + RealNVP (d = 64, 65536 chains, 20 x 100 transitions; wall clock with a
synchronize, median of 3): the option on at thinning 1 and 10, off on the host loop, as an extra off as one native call, and
store_samples=True followed by diagnostics().
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nfmc_amd import diagnostics, hip  # noqa: E402

STREAM_TBS = 6.3   # measured float4 copy rate of the MI355X


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def torch_sums(x, max_lag, group):
    """What a user composes today: every sum of the kernel from torch ops on the device (fp32 centred draws, fp64 totals)."""
    K, n, d = x.shape
    h = K // 2
    m = x.mean(dim=0, dtype=torch.float64)
    c = (x - m).float()
    acov = torch.stack([(c[:K - l] * c[l:]).sum(dim=0).double().sum(dim=0) / K for l in range(max_lag + 1)])
    hx = torch.cat([c[:h], c[K - h:]], dim=1).double()
    mh = hx.mean(dim=0) + torch.cat([m, m])
    s2h = hx.var(dim=0, unbiased=True)
    mg = m.reshape(n // group, group, d)
    mu = mg.mean(dim=1)
    bt = mg.var(dim=1, unbiased=True) if group > 1 else torch.zeros_like(mu)
    head = [m.sum(0), (m * m).sum(0), mh.sum(0), (mh * mh).sum(0), s2h.sum(0), mu.sum(0), (mu * mu).sum(0), bt.sum(0)]
    return torch.cat([torch.stack(head), acov]).reshape(-1)


def torch_rank_series(x):
    """The four rank series composed from torch ops on the device: torch.sort per coordinate, searchsorted for the lower and
    upper bound of every value, torch.special.ndtri in fp64."""
    K, n, d = x.shape
    S = K * n
    v = x.reshape(S, d).t().contiguous()

    def scores(v):
        s = torch.sort(v, dim=1).values
        r = (torch.searchsorted(s, v) + torch.searchsorted(s, v, right=True) + 1).double() * 0.5
        return torch.special.ndtri((r - 0.375) / (S + 0.25)).float(), s

    bulk, s = scores(v)
    med = (s[:, (S - 1) // 2].double() + s[:, S // 2].double()) / 2
    folded, _ = scores((v.double() - med[:, None]).abs().float())
    low = (v <= s[:, (S - 1) // 20, None]).float()
    high = (v >= s[:, (19 * (S - 1) + 19) // 20, None]).float()
    return [t.t().reshape(K, n, d) for t in (bulk, folded, low, high)]


def bench_rank(a, dev):
    """--rank: the four-series transform (nfmc_rank_series_f32 four times into one slab) and the whole
    rank_normalized=True call, each next to the same results composed from torch ops."""
    for shape in a.shapes.split(','):
        K, n, d = (int(v) for v in shape.split('x'))
        L = min(a.max_lag, K - 1)
        torch.manual_seed(0)
        x = torch.randn(K, n, d, device=dev)
        x[1:] = 0.7 * x[:-1] + 0.5 * x[1:]
        rt = diagnostics._RankTransform(x)
        kinds = ('bulk', 'folded', 'tail_low', 'tail_high')

        def transform():
            for kind in kinds:
                rt.run(kind)

        def whole():
            return diagnostics.diagnose(x, max_lag=L, superchains=a.group, rank_normalized=True)

        def torch_whole():
            return [torch_sums(s.contiguous(), L, a.group).cpu() for s in [x] + torch_rank_series(x)]

        k_ms, k_all = timed(transform, a.reps)
        w_ms, w_all = timed(whole, a.reps)
        t_ms, t_all = timed(lambda: torch_rank_series(x), a.reps)
        tw_ms, tw_all = timed(torch_whole, a.reps)
        diff = {}
        for kind, want in zip(kinds, torch_rank_series(x)):
            diff[kind] = float((rt.run(kind) - want).abs().max())
        print(json.dumps({'shape': [K, n, d], 'max_lag': L, 'group': a.group, 'slab_gb': round(x.numel() * 4 / 1e9, 3),
                          'work_mb': round(rt.work.numel() * 8 / 1e6, 1),
                          'transform_ms': round(k_ms, 3), 'transform_ms_all': [round(v, 3) for v in k_all],
                          'torch_transform_ms': round(t_ms, 3), 'torch_transform_ms_all': [round(v, 3) for v in t_all],
                          'transform_speedup': round(t_ms / k_ms, 2),
                          'rank_normalized_call_ms': round(w_ms, 3), 'rank_normalized_call_ms_all': [round(v, 3) for v in w_all],
                          'torch_call_ms': round(tw_ms, 3), 'torch_call_ms_all': [round(v, 3) for v in tw_all],
                          'call_speedup': round(tw_ms / w_ms, 2), 'max_abs_diff_to_torch': diff}), flush=True)
        del x, rt


def bench_running(a, dev):
    lib = hip.lib()
    for shape in a.shapes.split(','):
        n, d = (int(v) for v in shape.split('x')[-2:])
        for L in (int(v) for v in a.lags.split(',')):
            for R in (int(v) for v in a.stage_rows.split(',')):
                torch.manual_seed(0)
                ring = torch.randn(R, n, d, device=dev)
                acc = diagnostics.RunningDiagnostics(n, d, dev, L, R * (a.reps + 1))

                def update():
                    acc.update(ring, 0, R, acc.n_seen)

                ms, ms_all = timed(update, a.reps)
                sums_ms, _ = timed(lambda: acc.sums(a.group), 1)
                state = int(lib.nfmc_diag_stream_state_bytes(n, d, L))
                print(json.dumps({'shape': [n, d], 'max_lag': L, 'stage_rows': R, 'update_us_per_draw': round(1e3 * ms / R, 2),
                                  'update_ms_all': [round(v, 4) for v in ms_all], 'state_gb': round(state / 1e9, 3),
                                  'state_as_kept_draws': round(state / (4.0 * n * d), 1),
                                  'sums_call_ms': round(sums_ms, 3)}), flush=True)
                del acc, ring
    if not a.through_sample:
        return
    import time
    from nfmc_amd import create_sampler
    from nfmc_amd.potentials import SumOfSquares
    n, d = 65536, 64
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(1))

    from nfmc_amd import containers

    def call(label, host_loop=False, diagnose=False, stage_rows=None, **params):
        torch.manual_seed(0)
        if stage_rows is not None:
            containers.RUNNING_STAGE_ROWS = stage_rows   # the ring of the runs below (StreamingSampleStore reads it per run)
            label += ', stage_rows %d' % stage_rows
        s = create_sampler(target=SumOfSquares((d,)), event_shape=(d,), strategy='jump_mala', flow='realnvp',
                           param_kwargs=dict(n_iterations=20, **params), inner_param_kwargs=dict(n_iterations=100))
        s.seed = 5
        if host_loop:
            s.host_loop = True   # JumpNFMC.sample: no whole-run call, the launches of every iteration from the host
        times = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = s.sample(x0, show_progress=False)
            if diagnose:
                out.diagnostics(superchains=a.group)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
            del out
        print(json.dumps({'sample': label, 'ms': round(statistics.median(times[1:]), 2),
                          'ms_all': [round(v, 2) for v in times]}), flush=True)

    call('off, one native call (extra: the default path of such a run)', store_samples=False)
    call('off, host loop', host_loop=True, store_samples=False)
    for thin in (1, 10):
        for R in (int(v) for v in a.stage_rows.split(',')):
            call('running, thinning %d' % thin, diagnose=True, stage_rows=R, store_samples=False, running_diagnostics=True,
                 thinning=thin)
            call('running L=31, thinning %d' % thin, diagnose=True, stage_rows=R, store_samples=False, running_diagnostics=31,
                 thinning=thin)
        call('stored + diagnostics(), thinning %d' % thin, diagnose=True, store_samples=True, thinning=thin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='100x65536x64,100x8192x512')
    ap.add_argument('--max-lag', type=int, default=99)
    ap.add_argument('--group', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rank', action='store_true', help='time the rank transform and the rank-normalised call instead')
    ap.add_argument('--running', action='store_true', help='time the running diagnostics instead')
    ap.add_argument('--lags', default='0,31,127')
    ap.add_argument('--stage-rows', default='32,128')
    ap.add_argument('--through-sample', action='store_true', help='with --running: whole sample() calls as well')
    a = ap.parse_args()
    dev = hip.require_gpu()
    lib = hip.lib()
    if a.running:
        if a.shapes == ap.get_default('shapes'):
            a.shapes = '65536x64,8192x512'
        bench_running(a, dev)
        return
    if a.rank:
        bench_rank(a, dev)
        return
    for shape in a.shapes.split(','):
        K, n, d = (int(v) for v in shape.split('x'))
        L = min(a.max_lag, K - 1)
        torch.manual_seed(0)
        x = torch.randn(K, n, d, device=dev)
        x[1:] = 0.7 * x[:-1] + 0.5 * x[1:]            # some autocorrelation; the values do not matter for the time
        sums = torch.empty(int(lib.nfmc_diag_sums_doubles(d, L)), dtype=torch.float64, device=dev)
        nbytes = int(lib.nfmc_diag_work_bytes(n, d, L))
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        args = hip.NfmcDiagArgs(hip.ptr(x), K, n, d, L, a.group, 0, hip.ptr(sums, torch.float64),
                                hip.ptr(work, torch.float64), nbytes)

        def kernel():
            hip.check(lib.nfmc_chain_diagnostics_f32(C.byref(args), hip.stream()), 'nfmc_chain_diagnostics_f32')

        k_ms, k_all = timed(kernel, a.reps)
        got = sums.clone()
        t_ms, t_all = timed(lambda: torch_sums(x, L, a.group), a.reps)
        want = torch_sums(x, L, a.group)
        scale = want.reshape(-1, d)[hip.DIAG_ACOV].abs().max()
        slab = x.numel() * 4
        print(json.dumps({'shape': [K, n, d], 'max_lag': L, 'group': a.group, 'kernel_ms': round(k_ms, 4),
                          'kernel_ms_all': [round(v, 4) for v in k_all], 'slab_gb': round(slab / 1e9, 3),
                          'slab_bytes_over_kernel_time_tbs': round(slab / (k_ms * 1e-3) / 1e12, 3),
                          'stream_tbs': STREAM_TBS, 'work_mb': round(nbytes / 1e6, 1),
                          'torch_ms': round(t_ms, 3), 'torch_ms_all': [round(v, 3) for v in t_all],
                          'speedup': round(t_ms / k_ms, 1),
                          'acov_max_diff_over_lag0': float(((got - want).reshape(-1, d)[hip.DIAG_ACOV:].abs().max() / scale))}),
              flush=True)
        del x, work, sums


if __name__ == '__main__':
    main()
