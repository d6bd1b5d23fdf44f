"""ctypes binding of libnfmc_hip.so (include/nfmc_hip.h).  No torch types cross the boundary:
tensors are passed as raw device pointers (`tensor.data_ptr()`), work is enqueued on the
caller's current HIP stream.

The library is REQUIRED: importing a sampler on a machine where it cannot be loaded raises
(there is no CPU or eager-PyTorch fallback for the hot path).
"""
import ctypes as C
import os

import torch

from .abi import *  # noqa: F401,F403  the mirror of the header (constants, structs, SYMBOLS): hip.NAME for every name

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NFMC_LIB', os.path.join(HERE, 'libnfmc_hip.so'))


def padded_d(d):
    """The column count of a statistics slab for event size d (csrc/common.hpp: padded_d)."""
    p = 4
    while p < d:
        p <<= 1
    return p


def tune_shift_offset(d):
    """First word of the per-coordinate shift c in the tuning state: tuning launches accumulate x - c and (x - c)^2, the
    controller un-shifts in fp64 and moves c to the folded mean (include/nfmc_hip.h, NFMC_TUNE_WORDS)."""
    return TUNE_WORDS + 2 * padded_d(d) + STAT_TAIL


# Philox step of warmup transition 0: a warmup draws from its own half of the stream, so a sampling run that follows it
# with the same seed (steps from 0) never reuses a warmup draw
WARMUP_STEP0 = 1 << 31

_lib = None


def lib():
    """Load the library (once).  Raises if it is missing: the hot path has no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'nfmc_amd: %s is missing. Build it with `python -m nfmc_amd.build` (needs hipcc); the MI355X '
                'path has no CPU/eager fallback.' % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        # the structs below are ABI version NFMC_ABI_VERSION: a stale or side-built library (NFMC_LIB, tools/ab_*.sh
        # variants) under them would read pointers at the wrong offsets -- refuse it before binding anything else
        probe = getattr(handle, 'nfmc_limits', None)
        if probe is None:
            raise RuntimeError('nfmc_amd: %s does not export nfmc_limits (not an nfmc_hip library?)' % LIB_PATH)
        probe.restype, probe.argtypes = C.c_int, [C.POINTER(NfmcLimits)]
        lim = NfmcLimits()
        rc = probe(C.byref(lim))
        if rc != 0 or lim.abi_version != NFMC_ABI_VERSION:
            raise RuntimeError('nfmc_amd: %s has ABI version %d (status %d); this package binds version %d. Rebuild it '
                               'with `python -m nfmc_amd.build --force`.' % (LIB_PATH, lim.abi_version, rc, NFMC_ABI_VERSION))
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


class NfmcArgumentError(ValueError):
    """A negative status of the library (`code`): ValueError is the reference's only error channel."""

    def __init__(self, message, code):
        super().__init__(message)
        self.code = code

    @property
    def no_kernel(self):
        """The request is valid but no kernel covers it (shape / width beyond a fused kernel): callers that have a
        composed path take it."""
        return self.code in (EUNSUPPORTED, ESHAPE)


def check(rc, what):
    """Map a return code to the reference's error channels: ValueError for argument errors
    (the reference's only error type, langevin.py:111), RuntimeError for HIP errors."""
    if rc == 0:
        return
    msg = lib().nfmc_error_string(rc).decode()
    if rc < 0:
        raise NfmcArgumentError('%s: %s (code %d)' % (what, msg, rc), rc)
    raise RuntimeError('%s: HIP error %d: %s' % (what, rc, msg))


def supported(rc, what) -> bool:
    """The answer of a `*_supported_f32` dry-run query: False for a valid request no fused kernel covers
    (NfmcArgumentError.no_kernel), True for OK; any other status raises as `check` does."""
    if rc in (EUNSUPPORTED, ESHAPE):
        return False
    check(rc, what)
    return True


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError('nfmc_amd needs a ROCm GPU (MI355X / gfx950); torch.cuda.is_available() is False. '
                           'There is no CPU fallback for the hot path.')
    return torch.device('cuda', torch.cuda.current_device())


def ptr(t, dtype=torch.float32):
    """Device pointer of a contiguous CUDA tensor of `dtype` (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError('expected a GPU tensor')
    if t.dtype != dtype:
        raise ValueError('expected dtype %s, got %s' % (dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError('expected a contiguous tensor')
    return C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream():
    """torch's current stream on the current device as a hipStream_t (the raw binding: the public
    `torch.cuda.current_stream()` builds a Stream object, ~10 us per call, once per kernel launch)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def build_digest():
    """Source digest the loaded library was built from (nfmc_build_digest)."""
    return lib().nfmc_build_digest().decode()


def limits():
    out = NfmcLimits()
    check(lib().nfmc_limits(C.byref(out)), 'nfmc_limits')
    return out


class DeviceStats:
    """Device-resident accumulators behind NfmcStats (fp64 sums, u64 counters, scratch slabs).

    Deferred mode (`struct(defer=True, attempted=...)`): the sampling kernels only add their per-workgroup
    partials to the zeroed scratch and ONE fold (nfmc_stats_fold_f32) runs when the totals are read, instead
    of one fold kernel per launch.  `sum_x`, `sum_x2`, `counters` and `jump_counters` fold lazily, and a
    non-deferred `struct()` folds first, so the two modes can be mixed freely within a run.
    """

    def __init__(self, d, device):
        self.d = d
        self.device = device
        # one backing allocation (8-byte words), so the totals come back in ONE device-to-host copy (host_totals):
        # each separate .cpu() is ~30 us of latency at the end of every sample() call
        self._buf = torch.zeros(2 * d + 2 * CNT_WORDS, dtype=torch.float64, device=device)
        self._sum_x = self._buf[:d]
        self._sum_x2 = self._buf[d:2 * d]
        self._counters = self._buf[2 * d:2 * d + CNT_WORDS].view(torch.int64)
        self._jump_counters = self._buf[2 * d + CNT_WORDS:].view(torch.int64)
        nbytes = int(lib().nfmc_stats_scratch_bytes(d))
        self.scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=device)
        self._pending = False
        self._attempted = 0
        self._jump_attempted = 0

    def _raw(self, defer=0, tail_slot=0, counters=None):
        return NfmcStats(ptr(self._sum_x, torch.float64), ptr(self._sum_x2, torch.float64),
                         ptr(self._counters if counters is None else counters, torch.int64),
                         ptr(self.scratch, torch.float64), self.scratch.numel() * 8, defer, tail_slot)

    def struct(self, defer=False, attempted=0, jump=False, jump_attempted=0):
        """NfmcStats for one launch.  defer=True: `attempted` = chain-transitions this launch attempts (the fold
        books them; `jump_attempted` those of a jump fused behind it); jump=True: the launch is a jump (accept
        counts go to `jump_counters`).  NFMC_STATS_DEFER=0 turns deferral off (A/B measurements)."""
        if not defer or os.environ.get('NFMC_STATS_DEFER', '1') == '0':
            self.fold()
            return self._raw(counters=self._jump_counters if jump else None)
        self._pending = True
        if jump:
            self._jump_attempted += int(attempted)
        else:
            self._attempted += int(attempted)
            self._jump_attempted += int(jump_attempted)
        return self._raw(1, 2 if jump else 0)

    def fold(self):
        if not self._pending:
            return
        st = self._raw()
        check(lib().nfmc_stats_fold_f32(C.byref(st), self.d, self._attempted, ptr(self._jump_counters, torch.int64),
                                        self._jump_attempted, stream()), 'nfmc_stats_fold_f32')
        self._pending = False
        self._attempted = 0
        self._jump_attempted = 0

    @property
    def sum_x(self):
        self.fold()
        return self._sum_x

    @property
    def sum_x2(self):
        self.fold()
        return self._sum_x2

    @property
    def counters(self):
        self.fold()
        return self._counters

    @property
    def jump_counters(self):
        self.fold()
        return self._jump_counters

    def host_totals(self):
        """(sum_x, sum_x2, counters, jump_counters) as CPU tensors from one copy (synchronises the stream)."""
        self.fold()
        h = self._buf.cpu()
        d = self.d
        return (h[:d], h[d:2 * d], h[2 * d:2 * d + CNT_WORDS].view(torch.int64),
                h[2 * d + CNT_WORDS:].view(torch.int64))

    def zero_(self):
        self.fold()
        self._buf.zero_()


def dense_store(t):
    """NfmcSampleStore that keeps every transition of one call in the rows of `t` (k, n, d), in order (None: nothing)."""
    if t is None:
        return NfmcSampleStore(None, 1, 0, 1, 0)
    return NfmcSampleStore(ptr(t), 1, 0, int(t.shape[0]), 0)


def store_struct(samples, k):
    """NfmcSampleStore for a call that offers k transitions: `samples` is None (keep nothing), a
    containers.DeviceSampleStore (thinning / bounded window decided here, before the launch), or a dense (k, n, d)
    device tensor (every transition kept, in order)."""
    if samples is None:
        return dense_store(None)
    if hasattr(samples, 'struct'):
        return samples.struct(k)
    if int(samples.shape[0]) != int(k):
        raise ValueError('dense sample view has %d rows for %d transitions' % (samples.shape[0], k))
    return dense_store(samples)


def null_stats():
    return NfmcStats(None, None, None, None, 0, 0, 0)


def make_rng(seed, chain_offset, step0, replay_normals=None, replay_uniforms=None, rounds=0):
    """rounds: 0 / 10 = Philox4x32-10 (default stream), 7 = the opt-in Philox4x32-7 stream."""
    return NfmcRng(int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_offset), int(step0) & 0xFFFFFFFF, int(rounds),
                   ptr(replay_normals), ptr(replay_uniforms))
