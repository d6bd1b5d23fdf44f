#!/usr/bin/env python
"""Generate tests/golden/spline_trained_*.npz: 'c-rqnsf' flows of the CPU restatement (oracle/flow.py) TRAINED on a
funnel-plus-two-modes sample, for the tests that hold the spline kernels to fp64 oracles where fitted splines live
(tests/spline_fixtures.py, tests/test_host_spline_trained.py, tests/test_gpu_spline_trained.py).  CPU only, this
repository's oracle only.

Run from the repo root:  python tests/golden/make_golden_spline.py [NAME...]

The recipe, per case: n = 1000 rows x = randn, x[:, 1:] *= exp(0.75 x[:, :1]) (a funnel in the first coordinate),
x[:n/2, -1] += 3 (two modes in the last); 800 training and 200 validation rows; oracle.flow.fit_run in fp64, 300 full-batch
AdamW epochs at lr = 0.05, the last weights kept.  The initial weights are torch's default Linear initialisation under
`init_seed`.  One thread, so that the sums (and with them every bit of the result) do not depend on the machine's core
count.  A fixture is data only: the state dict as float32 arrays ('flow/<key>'), the recipe and the shape as scalars, the
first and last losses of the run.  The archive is written with fixed member timestamps: the same bytes every time.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

N_ROWS, N_TRAIN, N_EPOCHS, LR, DATA_SEED = 1000, 800, 300, 0.05, 1
CASES = {  # name: d, n_hidden, hidden layers, coupling layers, seed of the initial weights
    'spline_trained_d8': (8, 4, 2, 2, 8),
    'spline_trained_d7': (7, 3, 1, 3, 7),
    'spline_trained_d24': (24, 8, 2, 2, 24),
    'spline_trained_d64': (64, 8, 2, 2, 64),
}


def recipe_rows(n, d, seed):
    """The training distribution: a funnel in coordinate 0, two modes in the last coordinate of the first half."""
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    x[:, 1:] *= torch.exp(0.75 * x[:, :1])
    x[:n // 2, -1] += 3.0
    return x


def write_npz(path, arrays):
    """np.savez_compressed with every member stamped 1980-01-01: regenerating gives the same file, byte for byte."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    from oracle import flow as oflow
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for name, (d, n_hidden, n_hl, n_coupling, init_seed) in CASES.items():
        if only and name not in only:
            continue
        x = recipe_rows(N_ROWS, d, DATA_SEED)
        torch.manual_seed(init_seed)
        flow = oflow.Flow(oflow.CRQNSF((d,), n_layers=n_coupling, conditioner_kwargs={'n_hidden': n_hidden, 'n_layers': n_hl}))
        tr = oflow.fit_run(flow, x[:N_TRAIN], x[N_TRAIN:], n_epochs=N_EPOCHS, lr=LR, keep_best_weights=False)
        arrays = {'flow/' + k: v.detach().to(torch.float32).numpy().copy() for k, v in tr.state.items()}
        arrays.update(d=np.int64(d), n_hidden=np.int64(n_hidden), n_hidden_layers=np.int64(n_hl), n_coupling=np.int64(n_coupling),
                      n_rows=np.int64(N_ROWS), n_train=np.int64(N_TRAIN), n_epochs=np.int64(N_EPOCHS), lr=np.float64(LR),
                      data_seed=np.int64(DATA_SEED), init_seed=np.int64(init_seed),
                      train_loss=np.array([tr.train[0], tr.train[-1]]), val_loss=np.array([tr.val[0], tr.val[-1]]))
        write_npz(os.path.join(OUT, name + '.npz'), arrays)
        n_floats = sum(v.size for k, v in arrays.items() if k.startswith('flow/'))
        print('wrote %s: %d floats, validation loss %.4f -> %.4f' % (name, n_floats, tr.val[0], tr.val[-1]))


if __name__ == '__main__':
    main()
