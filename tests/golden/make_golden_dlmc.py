#!/usr/bin/env python
"""Generate tests/golden/dlmc_*.npz by running the REFERENCE's DLMC (nfmc/algorithms/sampling/nfmc/dlmc.py), build
container only.  Same stand-ins, CPU flow (oracle/flow.py) and draw recorder as make_golden.py.

Run from the repo root:  python tests/golden/make_golden_dlmc.py

The flow's `fit` is a no-op, so the fixtures pin the transition arithmetic and the counters given fixed flow weights:
  dlmc_d6         the default gradient step  x <- x - eps grad_x [U(x) + log q(x)]
  dlmc_latent_d6  latent_updates=True        z = f(x), z <- z - eps (grad U(x) - z), x = f^-1(z)
Noise per iteration: one latent (n, d) field for the flow proposal, then one accept uniform per chain (the refit's
torch.randperm is recorded too and unused: the fit does nothing).  Fixtures are data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import DrawRecorder, _install_standins, flow_arrays, out_arrays, save  # noqa: E402


def main():
    _install_standins()
    from nfmc.algorithms.sampling.nfmc.dlmc import DLMC, DLMCKernel, DLMCParameters
    from oracle import flow as oflow
    from oracle import potentials as opot

    def nll(x):   # a likelihood different from the target, so the initial step is pinned to it
        return 0.5 * torch.sum((x - 0.25) ** 2, dim=-1)

    for name, latent, seed in [('dlmc_d6', False, 31), ('dlmc_latent_d6', True, 37)]:
        d, n, T = 6, 12, 4
        torch.manual_seed(seed)
        flow = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,))), seed + 100, 0.1, 0.7)
        flow.fit = lambda *a, **k: None
        torch.manual_seed(seed + 1)
        x0 = torch.randn(n, d)
        kern = DLMCKernel((d,), flow=flow, step_size=0.05)
        params = DLMCParameters(n_iterations=T, latent_updates=latent)
        s = DLMC((d,), opot.sum_squares, nll, kern, params)
        with DrawRecorder() as rec:
            out = s.sample(x0.clone(), show_progress=False)
        save(name, rec, x0=x0.numpy(), step_size=np.float64(kern.step_size), n_iterations=np.int64(T),
             latent_updates=np.int64(latent), nll_shift=np.float64(0.25), **flow_arrays(flow), **out_arrays(out))


if __name__ == '__main__':
    main()
