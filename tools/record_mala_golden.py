"""Recordings of the exact-fit Gaussian MALA kernels (mala_kernel, FAST quadratic branch) for tests/test_gpu_mala_forms.py.

    python tools/record_mala_golden.py [--out tests/golden/mala_forms]        (on a GPU box)

Run it with the library of the commit whose bits are to be kept (NFMC_LIB selects a build), BEFORE the kernel is edited:
the test reruns every case through the public API and compares for equality, so a change of instruction forms in the step
loop is proven against what the parent computed and never against another instantiation of the changed code.

Every case is `create_sampler(SumOfSquares((64,)), strategy=...)` with a fixed seed and x0 from a seeded CPU generator.
Per case the manifest (cases.json) holds the SHA-256 of the bytes of `last_state`, `mean`, `second_moment` (float32), of
the integer counters (int64) and, where the run keeps its states, of `samples`; cases of at most RAW_MAX_CHAINS chains also
leave the arrays themselves in <id>.npz (the kept states excepted: hash only), so that a failing test can say where.

The cases (CASES below):
  chains       1, 37, 96: a partly filled wave, a partly filled tile (a tile is 32 chains at d = 64), three whole tiles
  transitions  1, 3, 4, 5, 33, 100 per launch: 33 crosses the refresh of the chain's 32 ln u; 3 and 5 leave a remainder
               of a group of four
  jump_mala    5 inner transitions x 3 outer iterations: the later launches start at steps 6 and 12, no multiples of 4
  rounds       Philox4x32-10 and the opt-in Philox4x32-7
  ula          no Metropolis test, no ln u
  kept states  store_samples=True runs the instantiation with per-step outputs, beside the lean one
  grid stride  65536 + 37 chains = 2050 tiles on at most 2048 workgroups: a workgroup walks two tiles, hashes only
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D = 64
SEED = 20240607
RAW_MAX_CHAINS = 96
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden', 'mala_forms')
FIELDS = ('last_state', 'mean', 'second_moment', 'counters', 'samples')


def _case(strategy, n, k, rounds=10, store=False, outer=None):
    cid = '%s_n%d_k%d_r%d%s%s' % (strategy, n, k, rounds, '_t%d' % outer if outer else '', '_kept' if store else '')
    return {'id': cid, 'strategy': strategy, 'n': n, 'k': k, 'rounds': rounds, 'store_samples': store, 'outer': outer}


def _cases():
    out = []
    for n in (1, 37, 96):
        for k in (1, 3, 4, 5, 33, 100):
            out.append(_case('mala', n, k))
    for k in (1, 3, 4, 5, 33, 100):
        out.append(_case('mala', 37, k, rounds=7))
    out += [_case('mala', 1, 33, rounds=7), _case('mala', 96, 33, rounds=7), _case('mala', 96, 100, rounds=7)]
    out += [_case('ula', 1, 5), _case('ula', 37, 33), _case('ula', 96, 5), _case('ula', 37, 5, rounds=7)]
    out += [_case('mala', 37, 5, store=True), _case('mala', 37, 33, store=True), _case('mala', 96, 100, store=True),
            _case('mala', 37, 33, rounds=7, store=True), _case('ula', 37, 5, store=True)]
    out += [_case('jump_mala', 37, 5, outer=3), _case('jump_mala', 96, 5, outer=3), _case('jump_mala', 1, 5, outer=3),
            _case('jump_mala', 37, 5, rounds=7, outer=3)]
    out += [_case('mala', 65536 + 37, 3), _case('mala', 65536 + 37, 3, rounds=7)]
    return out


CASES = _cases()


def x0_of(case):
    gen = torch.Generator().manual_seed(100003 * case['n'] + case['k'])
    return 0.7 * torch.randn(case['n'], D, generator=gen)


def run_case(case):
    """One case through the public API; {field: numpy array} (float32 states and moments, int64 counters)."""
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.sample import create_sampler
    st = case['strategy']
    if st == 'jump_mala':
        torch.manual_seed(1)   # the default-initialised RealNVP of the jump
        s = create_sampler(SumOfSquares((D,)), strategy=st, flow='realnvp',
                           param_kwargs={'n_iterations': case['outer'], 'store_samples': case['store_samples']},
                           inner_param_kwargs={'n_iterations': case['k']})
    else:
        s = create_sampler(SumOfSquares((D,)), strategy=st, flow=None,
                           param_kwargs={'n_iterations': case['k'], 'store_samples': case['store_samples']})
    s.seed = SEED
    s.rng_rounds = case['rounds']
    out = s.sample(x0_of(case), show_progress=False)
    stats = out.statistics
    names = tuple(stats.COUNTERS) + ('n_nonfinite_log_ratios',)
    res = {'last_state': out.running_samples.last_sample.reshape(-1, D).cpu().numpy(),
           'mean': out.mean.cpu().numpy(), 'second_moment': out.second_moment.cpu().numpy(),
           'counters': np.asarray([int(getattr(stats, c)) for c in names], dtype=np.int64)}
    if case['store_samples']:
        res['samples'] = out.samples.reshape(-1, case['n'], D).cpu().numpy()
    for name in ('last_state', 'mean', 'second_moment', 'samples'):
        if name in res:
            assert res[name].dtype == np.float32, (name, res[name].dtype)
            res[name] = np.ascontiguousarray(res[name])
    return res


def digests(res):
    return {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=GOLDEN_DIR)
    args = ap.parse_args()
    from nfmc_amd import hip
    assert torch.cuda.is_available(), 'the recorder needs the GPU'
    os.makedirs(args.out, exist_ok=True)
    manifest = {'library_digest': hip.build_digest(), 'd': D, 'seed': SEED, 'cases': []}
    for case in CASES:
        res = run_case(case)
        manifest['cases'].append(dict(case, sha256=digests(res)))
        if case['n'] <= RAW_MAX_CHAINS:
            np.savez(os.path.join(args.out, case['id'] + '.npz'), **{k: v for k, v in res.items() if k != 'samples'})
        print('%-28s acc %d / %d' % (case['id'], res['counters'][0], res['counters'][1]), flush=True)
    with open(os.path.join(args.out, 'cases.json'), 'w') as fh:
        json.dump(manifest, fh, indent=1)
        fh.write('\n')
    print('wrote %d cases to %s' % (len(CASES), args.out))


if __name__ == '__main__':
    main()
