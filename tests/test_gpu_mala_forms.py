"""The exact-fit Gaussian MALA kernels (mala_kernel, FAST quadratic branch) compute, bit for bit, what they computed before
their step loop was rewritten in cheaper instruction forms: the update on acceptance as moves under the accept mask, the
last reduction stage as one DPP add.  The cases also cover what two forms that were measured and not kept could have got
wrong (round keys in VGPRs, ln u of four transitions in one LDS read): they stay, for the next attempt at this loop.

The expected values are recordings of the parent commit's library (tools/record_mala_golden.py, which also lists what each
case is for): raw arrays for the runs of at most 96 chains, SHA-256 of the same bytes for all.  Equality, no tolerance: no
sum changes its order and the generator's stream is the same, so there is no rounding to allow for.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tools import record_mala_golden as rec   # noqa: E402  (the cases run exactly as they were recorded)

with open(os.path.join(rec.GOLDEN_DIR, 'cases.json')) as _fh:
    MANIFEST = json.load(_fh)


def test_manifest_covers_the_recorders_cases():
    assert [c['id'] for c in MANIFEST['cases']] == [c['id'] for c in rec.CASES]
    assert (MANIFEST['d'], MANIFEST['seed']) == (rec.D, rec.SEED)


@pytest.mark.parametrize('case', MANIFEST['cases'], ids=[c['id'] for c in MANIFEST['cases']])
def test_same_bits_as_the_parent(case):
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    params = {k: case[k] for k in ('id', 'strategy', 'n', 'k', 'rounds', 'store_samples', 'outer')}
    got = rec.run_case(params)
    assert sorted(got) == sorted(case['sha256'])
    raw = os.path.join(rec.GOLDEN_DIR, case['id'] + '.npz')
    assert os.path.exists(raw) == (case['n'] <= rec.RAW_MAX_CHAINS)
    if os.path.exists(raw):
        with np.load(raw) as z:
            for name in z.files:
                want = z[name]
                assert got[name].dtype == want.dtype and got[name].shape == want.shape, name
                # compared as bit patterns: -0.0 and NaN payloads count
                a, b = got[name].view(np.uint8), want.view(np.uint8)
                differing = np.flatnonzero(a != b)
                assert differing.size == 0, '%s: %d bytes differ, first at element %d' % (name, differing.size,
                                                                                       differing[0] // want.itemsize)
    assert rec.digests(got) == case['sha256']
