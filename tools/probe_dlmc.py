"""DLMC costs on the device (HIP events, best of 5): the grad_x log q kernel (nfmc_flow_logq_grad_f32), the fused step
(nfmc_dlmc_step_f32), the composed autograd route it replaces (forward_torch + autograd), one epoch of the resident flow
fit on the same rows (the fit's reverse sweep with its weight-gradient accumulators and AdamW: the other candidate layout
for the input gradient), and one whole DLMC outer iteration at the reference's defaults with the share of it in the refit.

    python tools/probe_dlmc.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nfmc_amd.flows import Flow, RealNVP  # noqa: E402
from nfmc_amd.potentials import SumOfSquares  # noqa: E402
from nfmc_amd.samplers import dlmc  # noqa: E402


def ev_ms(fn, reps=5):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def main():
    dev = torch.device('cuda', 0)
    for n, d in ((65536, 64), (32768, 256), (4096, 64)):
        torch.manual_seed(0)
        f = Flow(RealNVP((d,)))
        x = (0.7 * torch.randn(n, d)).to(dev)
        pot = SumOfSquares((d,))
        dlmc.logq_grad(f, x)   # pack + warm
        t_grad = ev_ms(lambda: dlmc.logq_grad(f, x))
        y = x.clone()
        t_step = ev_ms(lambda: dlmc.launch_step(f, y, 1e-6, pot=pot))
        f.to(dev)   # the composed route on the GPU (a fresh flow's parameters are on the host)
        t_auto = ev_ms(lambda: y.sub_(1e-6 * (dlmc._grad(pot, y, (d,)) + dlmc.logq_grad_torch(f, y, (d,)))))
        xf = x[:4096]
        f.fit(x_train=xf, n_epochs=2, early_stopping=False, show_progress=False)
        t_fit = ev_ms(lambda: f.fit(x_train=xf, n_epochs=20, early_stopping=False, show_progress=False)) / 20
        print('n=%6d d=%3d  logq_grad %.3f ms  fused step %.3f ms  composed autograd %.3f ms  fit epoch (4096 rows) %.3f ms'
              % (n, d, t_grad, t_step, t_auto, t_fit), flush=True)
    # one outer iteration at the defaults: refit (early stopping) + step + MH, kernel events per label
    for n, d in ((4096, 64), (32768, 64)):
        torch.manual_seed(0)
        s = dlmc.DLMC((d,), SumOfSquares((d,)), SumOfSquares((d,)), dlmc.DLMCKernel((d,)), dlmc.DLMCParameters(n_iterations=3))
        x0 = 0.7 * torch.randn(n, d)
        s.sample(x0, show_progress=False)
        T = 10
        s.params.n_iterations = T
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.sample(x0, show_progress=False)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) / T * 1e3
        s.time_kernels = True
        out = s.sample(x0, show_progress=False)
        torch.cuda.synchronize()
        per = {}
        for label, e0, e1 in out.kernel_events:
            per[label] = per.get(label, 0.0) + e0.elapsed_time(e1) / T
        orig = dlmc.DLMC._refit
        dlmc.DLMC._refit = lambda self, flow, xt, xv: None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.time_kernels = False
        s.sample(x0, show_progress=False)
        torch.cuda.synchronize()
        no_fit = (time.perf_counter() - t0) / T * 1e3
        dlmc.DLMC._refit = orig
        print('n=%6d d=%3d  DLMC iteration %.3f ms (wall), without the refit %.3f ms -> refit share %.0f %%; kernels %s'
              % (n, d, total, no_fit, 100 * (total - no_fit) / total, {k: round(v, 4) for k, v in per.items()}), flush=True)


if __name__ == '__main__':
    main()
