"""Shared host logic of the samplers: target resolution, run state on the device, noise bookkeeping."""
import ctypes as C
import math
import time
from typing import Optional

import torch

from .. import hip
from ..containers import DeviceSampleStore, StreamingSampleStore, running_lags
from ..flows import Flow
from ..potentials import Potential, recognize


def resolve_target(target, event_shape, fuse='auto', x0=None, family=None) -> Optional[Potential]:
    """A closed-form descriptor for `target`, or None (-> split path: torch autograd for U, grad U).
    fuse: 'auto' (default) probes plain callables (potentials.recognize; `x0` sets the radii the probes must also
    cover); False / 'never' keeps every plain callable on the split path.
    family: the launch family the descriptor is for (potentials.FAMILIES); a potential whose kind that family's kernels
    do not evaluate (`Potential.fused_in`) resolves to None there, like an arbitrary callable."""
    if isinstance(target, Potential):
        return target if family is None or target.fused_in(family) else None
    if fuse in (False, 'never'):
        return None
    x_scale = None
    if x0 is not None and x0.numel() > 0:
        x_scale = float(x0.detach().abs().max())
    return recognize(target, event_shape, x_scale=x_scale)


class Replay:
    """Recorded noise for parity tests: `normals` (T, n, d) and `uniforms` (T, n) on the device, consumed in
    transition order (one normal field and one uniform vector per transition; unadjusted transitions take
    no uniforms, exactly like the reference's draw order -- SURVEY.md App. A.3)."""

    def __init__(self, normals, uniforms, device):
        self.normals = torch.as_tensor(normals, dtype=torch.float32).to(device).contiguous()
        self.normals = self.normals.reshape(self.normals.shape[0], self.normals.shape[1], -1)
        self.uniforms = None
        if uniforms is not None and torch.as_tensor(uniforms).numel() > 0:
            self.uniforms = torch.as_tensor(uniforms, dtype=torch.float32).to(device).contiguous()
        self.i_n = 0
        self.i_u = 0

    def take_uniforms(self, k=1):
        """The uniforms of k transitions alone.  The split path draws them only once every target call of the step
        has returned, like the reference (langevin.py:106, hmc.py:112, jump.py:225): a step whose target raised never
        consumes its uniforms."""
        un = self.uniforms[self.i_u:self.i_u + k]
        assert un.shape[0] == k, 'replay uniforms exhausted'
        self.i_u += k
        return un

    def take(self, k, with_uniforms=True):
        nz = self.normals[self.i_n:self.i_n + k]
        assert nz.shape[0] == k, 'replay noise exhausted'
        self.i_n += k
        un = None
        if with_uniforms:
            un = self.uniforms[self.i_u:self.i_u + k]
            assert un.shape[0] == k, 'replay uniforms exhausted'
            self.i_u += k
        return nz, un


class Run:
    """Device-side state of one `sample()` call."""

    def __init__(self, sampler, x0):
        self.dev = hip.require_gpu()
        hip.lib()
        self.n = int(x0.shape[0])
        self.event_shape = tuple(x0.shape[1:])
        self.d = int(math.prod(self.event_shape)) if self.event_shape else 1
        self.sampler = sampler
        shard = sampler.shard
        self.shard = shard
        if shard is not None:
            lo, hi = shard.bounds(self.n)
            x0 = x0[lo:hi]
            self.chain_offset = lo
            self.n_global = self.n
            self.n = hi - lo
        else:
            self.chain_offset = 0
            self.n_global = self.n
        self.x = x0.detach().to(self.dev, torch.float32).reshape(self.n, self.d).contiguous().clone()
        # stats.struct() has side effects (it folds, or books `attempted` and defers): like `rng` below it is called
        # exactly once per launch, and only for a launch that runs; a probe takes hip.null_stats()
        self.stats = hip.DeviceStats(self.d, self.dev)
        if sampler.seed is None:
            seed = int(torch.randint(0, 2 ** 62, ()).item())
            if shard is not None:
                seed = shard.broadcast_int(seed)
        else:
            seed = int(sampler.seed)
        self.seed = seed
        # 10 (default) or 7: the opt-in Philox4x32-7 stream (NfmcRng.rounds).  Kernels without it answer
        # NFMC_EUNSUPPORTED, which surfaces as a ValueError: no launch silently falls back to the other stream.
        self.rounds = int(getattr(sampler, 'rng_rounds', 10) or 10)
        if self.rounds not in (7, 10):
            raise ValueError('rng_rounds must be 10 (Philox4x32-10) or 7 (Philox4x32-7)')
        self.replay = None
        if sampler.replay is not None:
            normals, uniforms = sampler.replay
            self.replay = Replay(normals, uniforms, self.dev)
        self.t0 = time.time()
        self.kernel_events = None   # bench.py: list of (label, start_event, end_event) when kernel timing is on
        tk = getattr(sampler, 'time_kernels', False)
        self.kernel_event_filter = tk if isinstance(tk, str) else None   # a label: time only that kernel
        if tk:
            self.kernel_events = []

    def timed(self, label):
        """Context manager recording HIP events on the launch stream around one kernel call."""
        return _Timed(self, label)

    def rng(self, step0, k=0, adjusted=True):
        """NfmcRng for a launch of k transitions starting at transition `step0`.  Replay order is draw order: with
        replayed noise this consumes k normal fields, and k uniform vectors only when `adjusted`, so it is called exactly
        once per launch, and only for a launch that runs (a `*_supported_f32` probe takes hip.make_rng instead)."""
        if self.replay is not None:
            nz, un = self.replay.take(k, with_uniforms=adjusted)
            self._keep = (nz, un)
            return hip.make_rng(self.seed, self.chain_offset, step0, nz, un, rounds=self.rounds)
        return hip.make_rng(self.seed, self.chain_offset, step0, rounds=self.rounds)

    def sync(self):
        torch.cuda.synchronize(self.dev)

    def time_is_up(self, t0, limit_seconds) -> bool:
        """The `time_limit_seconds` test of the sampling loops (mcmc/base.py:70-72).  With sharded chains rank 0's clock
        decides for everybody, so all ranks stop after the same number of steps (their later collectives -- the refit
        all-gather, the statistics all-reduce -- must see the same shapes)."""
        if limit_seconds is None:
            return False
        self.sync()
        up = time.time() - t0 >= limit_seconds
        if self.shard is not None and self.shard.world > 1:
            up = bool(self.shard.broadcast_int(1 if up else 0))
        return up

    def elapsed(self):
        self.sync()
        return time.time() - self.t0

    def launches(self, total, limit, t0, time_limit_seconds, bar):
        """The chunk loop of a sample() call whose transitions all run in launches of at most `limit`: yields
        (done, k) for the launch of transitions done .. done + k - 1, reads the clock (`time_is_up`) before each and
        moves `bar` after it; the bar is closed when the loop ends, however it ends.  `self.done` counts the
        transitions of the launches that returned."""
        self.done = done = 0
        limit = min(limit, self.launch_cap())
        clock = time_limit_seconds is not None   # without a limit nothing is read, and the stream is never waited for
        try:
            while done < total and not (clock and self.time_is_up(t0, time_limit_seconds)):
                k = min(limit, total - done)
                yield done, k
                self.done = done = done + k
                bar.update(k)
        finally:
            bar.close()

    def offer_state(self, sink):
        """The current state as the one transition a split-path step offers to `sink`: a sample store, a dense
        (1, n, d) view of a refit block, or None (nothing is kept)."""
        if sink is None:
            return
        if hasattr(sink, 'add_dense'):
            sink.add_dense(self.x[None])
        else:
            sink[0].copy_(self.x)

    def sample_store(self, offered):
        """The store of kept states for a run that offers `offered` of them (thinning and `max_samples` applied on the
        device), or None when the sampler keeps none."""
        p = self.sampler.params
        self.streaming = None
        if offered > 0 and not p.tuning:
            thinning = max(1, int(getattr(p, 'thinning', 1)))
            lags = running_lags(p, -(-int(offered) // thinning))
            if lags is not None:
                # no states are kept: the kept draws pass through a small ring into the running diagnostics
                self.streaming = StreamingSampleStore(self.n, self.d, self.dev, offered, thinning, lags)
                return self.streaming
        if not (p.store_samples and offered > 0):
            return None
        return DeviceSampleStore(self.n, self.d, self.dev, offered, getattr(p, 'thinning', 1),
                                 getattr(p, 'max_samples', None))

    def launch_cap(self, extra=0):
        """Transitions one launch may offer to the run's store, when the launch offers `extra` more than it is asked for
        (a jump tail): what one call takes, or what the staging ring of the running diagnostics holds."""
        streaming = getattr(self, 'streaming', None)
        if streaming is None:
            return hip.MAX_STEPS_PER_CALL
        return max(1, min(hip.MAX_STEPS_PER_CALL, streaming.max_offer - extra))

    def finish(self, out, t0, n_moments, store=None, **counters):
        """End of a sample() call: the final state, the statistics over `n_moments` (step, chain) pairs, the kept states
        of `store` and the kernel events into `out`, then the merge over the shards.  `counters` are MCMCStatistics
        counters; they override the device's accepted / attempted counts (and jump counts, where the class has them).

        The final-state copy and the statistics fold go out right behind the last kernel; the one device-to-host copy of
        the totals is the only synchronisation of the call (with a synchronize first, then the fold, then host work, then
        the clone, the stream sat idle ~110 us per call)."""
        last_sample = self.x.reshape(self.n, *self.event_shape).clone()
        sum_x, sum_x2, cnt, jc = self.stats.host_totals()
        st = out.statistics
        device = {'n_accepted_trajectories': int(cnt[hip.CNT_ACCEPTED]),
                  'n_attempted_trajectories': int(cnt[hip.CNT_ATTEMPTED])}
        if 'n_accepted_jumps' in st.COUNTERS:
            device.update(n_accepted_jumps=int(jc[hip.CNT_ACCEPTED]), n_attempted_jumps=int(jc[hip.CNT_ATTEMPTED]))
        st.update_counters(**{**device, **counters})
        # only jump launches book into the jump counters: they are zero for every other sampler
        st.n_nonfinite_log_ratios = int(cnt[hip.CNT_NONFINITE]) + int(jc[hip.CNT_NONFINITE])
        st.absorb_device_sums(sum_x.reshape(self.event_shape), sum_x2.reshape(self.event_shape), n_moments)
        if isinstance(store, StreamingSampleStore):
            store.flush()
            out.running = store.acc
        elif store is not None:
            out.running_samples.adopt_store(store, getattr(self.sampler.params, 'spill_to_host', False))
        out.running_samples.last_sample = last_sample
        st.update_elapsed_time(time.time() - t0)
        out.kernel_events = self.kernel_events
        if self.shard is not None:
            self.shard.merge_statistics(st)
        return out


class _Timed:
    def __init__(self, run, label):
        self.run, self.label = run, label

    def _on(self):
        sel = getattr(self.run, 'kernel_event_filter', None)
        return self.run.kernel_events is not None and (sel is None or sel == self.label)

    def __enter__(self):
        if self._on():
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self._on():
            self.e1.record(torch.cuda.current_stream())
            self.run.kernel_events.append((self.label, self.e0, self.e1))


def chunks(total, limit=hip.MAX_STEPS_PER_CALL):
    done = 0
    while done < total:
        k = min(limit, total - done)
        yield done, k
        done += k


def accept_select(run, step, x_prime, log_ratio, uniforms, tag, stats_struct, carry=None, mask_out=None):
    """The Metropolis test, the masked update of run.x and the moments of one split-path transition
    (nfmc_mh_accept_select_f32).  log_ratio None accepts every chain; uniforms None draws them on the native stream
    `tag` (hip.TAG_ACCEPT / TAG_JUMP) of transition `step`; carry = (per-chain values, their values at the proposal)
    is copied where a chain accepts; mask_out receives the uint8 mask."""
    st = hip.NfmcSelectArgs()
    st.x, st.x_prime, st.n, st.d = hip.ptr(run.x), hip.ptr(x_prime), run.n, run.d
    st.log_ratio = hip.ptr(log_ratio) if log_ratio is not None else None
    st.uniforms = hip.ptr(uniforms) if uniforms is not None else None
    st.n_carry = 0
    if carry is not None:
        st.n_carry = 1
        st.carry[0], st.carry_prime[0] = hip.ptr(carry[0]), hip.ptr(carry[1])
    st.rng = hip.make_rng(run.seed, run.chain_offset, step, rounds=run.rounds)
    st.rng_tag = tag
    st.stats = stats_struct
    st.mask_out = hip.ptr(mask_out, torch.uint8) if mask_out is not None else None
    hip.check(hip.lib().nfmc_mh_accept_select_f32(C.byref(st), hip.stream()), 'nfmc_mh_accept_select_f32')


def launch_limit(watched, show_progress, time_limit_seconds):
    """Transitions per launch of `Run.launches`: as many as one call takes when nobody watches the run, `watched` (a few,
    so that the bar moves and the clock is read) under a progress bar or a time limit."""
    return hip.MAX_STEPS_PER_CALL if time_limit_seconds is None and not show_progress else watched


def _refit(sampler, flow, x_train, x_val):
    """The in-run refit of JumpNFMC and DLMC (jump.py:201, dlmc.py:70: `flow.fit(x_train=..., x_val=...,
    **flow_fit_kwargs)`).  The build's own Flow takes `defer_check`: the run's kernels are enqueued and the divergence
    check (ValueError) is made when the next refit starts / when sampling ends, so that the next launch is queued behind
    the fit without a host round trip; a foreign flow object is called exactly as the reference calls it."""
    if isinstance(flow, Flow):
        return flow.fit(x_train=x_train, x_val=x_val, **{'defer_check': True, **sampler.params.flow_fit_kwargs})
    flow.fit(x_train=x_train, x_val=x_val, **sampler.params.flow_fit_kwargs)
    return None


def imd_tensor(kernel, dev):
    """inv_mass_diag on the device, or None when it is all ones (the kernels' scalar fast path)."""
    imd = kernel.inv_mass_diag
    if imd is None or bool((imd == 1).all()):
        return None
    return imd.detach().to(dev, torch.float32).contiguous()


class _NoBar:
    """Stands in for a disabled tqdm bar (constructing one costs ~15 us per sample() call even with disable=True)."""

    def __init__(self, iterable=None):
        self._it = iterable

    def __iter__(self):
        return iter(self._it)

    def update(self, n=1):
        pass

    def close(self):
        pass

    def set_postfix_str(self, s):
        pass


def progress(show, iterable=None, **kw):
    """tqdm when a progress bar is wanted, else a no-op with the same few methods."""
    if not show:
        return _NoBar(iterable)
    from tqdm import tqdm
    return tqdm(iterable, **kw) if iterable is not None else tqdm(**kw)
