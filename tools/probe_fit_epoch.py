"""One epoch of the device fit at the refit shapes (profiles/r04_refit.txt): d, rows, validation rows -> microseconds per
epoch (gradient launch + fold launch, 200 epochs enqueued back to back, HIP events), the shuffled split of the refit buffer,
and a whole `Flow.fit(n_epochs=2)` call as the refit of jump.py:193-201 issues it.

    python tools/probe_fit_epoch.py spline {rkl24|ml64|ml256}

times one shape of the spline ('c-rqnsf') fit instead, in one process: the median epoch of the device path (gradient + fold
launch, HIP events around every epoch) and of the eager torch loop it replaces (flow_training._loop's epoch, wall clock with
the loop's own read of the loss), 60 epochs each after 5 warm ones (profiles/r08_spline_fit.txt)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nfmc_amd.flow_training import DeviceFit
from nfmc_amd.flows import Flow, RealNVP
from nfmc_amd.tuning import train_val_split


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


SPLINE_CASES = {  # d, batch rows, validation rows, reverse KL to SumOfSquares
    'rkl24': (24, 1000, 0, True),      # the IMH warmup's shape
    'ml64': (64, 1024, 1024, False),
    'ml256': (256, 4096, 4096, False),   # the C5 refit shape
}


def spline(case, warm=5, epochs=60):
    import statistics
    from nfmc_amd.flow_training import _base_log_prob, forward_torch, inverse_torch
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.util import create_flow_object
    d, n, nv, rkl = SPLINE_CASES[case]
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, d, generator=g) * 0.7071).to(dev)
    xv = (torch.randn(nv, d, generator=g) * 0.7071).to(dev) if nv else None
    pot = SumOfSquares((d,))
    # ---- device path
    torch.manual_seed(1)
    f = create_flow_object('c-rqnsf', (d,)).to(dev)
    assert DeviceFit.supported(f.bijection, dev)
    fit = DeviceFit.of(f.bijection, dev, n + nv, 0.01)
    if nv:
        fit.set_validation(xv)
    ctl = fit.control(1 << 20, False, 50, True)
    desc = pot.descriptor(dev) if rkl else None
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(warm + epochs + 1)]
    torch.cuda.synchronize()
    marks[0].record()
    for e in range(warm + epochs):
        rows = torch.randn(n, d, device=dev) if rkl else x
        fit.run_calls(ctl, rows, e, 1, pot_struct=desc)
        marks[e + 1].record()
    torch.cuda.synchronize()
    t_dev = statistics.median(marks[e].elapsed_time(marks[e + 1]) for e in range(warm, warm + epochs)) * 1e3
    st = fit.state_after(warm + epochs)
    # ---- the eager torch loop (flow_training._loop, one epoch at a time)
    torch.manual_seed(1)
    f = create_flow_object('c-rqnsf', (d,)).to(dev)
    opt = torch.optim.AdamW(f.parameters(), lr=0.01)

    def loss_fn(rows):
        if rkl:
            xs, ld = inverse_torch(f.bijection, rows)
            return (_base_log_prob(rows) - ld + pot(xs)).mean()
        z, ld = forward_torch(f.bijection, rows)
        return -(_base_log_prob(z) + ld).mean()
    times = []
    for e in range(warm + epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = loss_fn(torch.randn(n, d, device=dev) if rkl else x)
        assert torch.isfinite(loss)
        loss.backward()
        opt.step()
        with torch.no_grad():
            float(loss_fn(xv)) if nv else float(loss)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    t_torch = statistics.median(times[warm:])
    print('c-rqnsf %s d=%d H=%d rows=%d val=%d %s: device %.1f us per epoch, torch loop %.1f us, ratio %.1f (n_params %d, best loss %.4f)'
          % (case, d, f.bijection.n_hidden, n, nv, 'reverse KL' if rkl else 'max likelihood', t_dev, t_torch, t_torch / t_dev,
             fit.n_params, st[0]), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == 'spline':
        return spline(sys.argv[2])
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    for d, n, nv, H in ((256, 4096, 4096, None), (256, 2867, 1229, None), (64, 4096, 1024, None), (64, 1024, 0, None), (128, 4096, 4096, 16),
                        (128, 4096, 4096, 128), (128, 1024, 0, 128), (64, 1024, 0, 64)):
        torch.manual_seed(1)
        ck = {'conditioner_kwargs': {'n_hidden': H, 'n_layers': 2}} if H else {}
        f = Flow(RealNVP((d,), **ck)).to(dev)
        x = (torch.randn(n, d, generator=g) * 0.7071).to(dev)
        xv = (torch.randn(max(nv, 1), d, generator=g) * 0.7071).to(dev)
        fit = DeviceFit(f.bijection, dev, n + nv, lr=0.01)
        if nv:
            fit.set_validation(xv[:nv])
        ctl = fit.control(200, False, 50, True)
        fit.run_calls(ctl, x, 0, 5)
        per_epoch = ev_ms(lambda: fit.run_calls(ctl, x, 0, 200)) / 200
        print('d=%d H=%d rows=%d val=%d: %.1f us per epoch (n_params %d)' % (d, f.bijection.n_hidden, n, nv, per_epoch * 1e3,
                                                                                fit.n_params), flush=True)
    # C4's warmup: the variational fit of the 128 x 2 conditioner at d = 128 to the funnel, 1024 latents per epoch
    from nfmc_amd.potentials import Funnel
    pot = Funnel((128,), 3.0)
    for path in ('0', '1'):
        os.environ['NFMC_FIT_TORCH'] = path
        torch.manual_seed(1)
        f = Flow(RealNVP((128,), conditioner_kwargs={'n_hidden': 128, 'n_layers': 2})).to(dev)
        f.variational_fit(lambda v: -pot(v), n_epochs=3, lr=0.01, n_samples=1024, early_stopping=False, potential=pot)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.variational_fit(lambda v: -pot(v), n_epochs=200, lr=0.01, n_samples=1024, early_stopping=False, potential=pot)
        torch.cuda.synchronize()
        print('Flow.variational_fit, d=128, H=128x2, 200 epochs of 1024 latents (%s): %.1f ms' % (
            'eager torch loop' if path == '1' else 'device', 1e3 * (time.perf_counter() - t0)), flush=True)
    os.environ['NFMC_FIT_TORCH'] = '0'
    # the refit as the sampler issues it: split of a (5, 32768, 256) block + Flow.fit(2 epochs)
    d, K, nch = 256, 5, 32768
    torch.manual_seed(1)
    f = Flow(RealNVP((d,))).to(dev)
    buf = (torch.randn(K, nch, d, generator=g) * 0.7071).to(dev)
    xt, xv = train_val_split(buf, 0.7, 4096, 4096)
    f.fit(x_train=xt, x_val=xv, n_epochs=2, show_progress=False)
    print('train_val_split (5 x 32768 x 256 -> 4096 + 4096 rows): %.1f us' % (1e3 * ev_ms(lambda: train_val_split(buf, 0.7, 4096, 4096))))
    print('Flow.fit(n_epochs=2), 4096 + 4096 rows, GPU time: %.1f us' % (1e3 * ev_ms(lambda: f.fit(x_train=xt, x_val=xv, n_epochs=2, show_progress=False))))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        a, b = train_val_split(buf, 0.7, 4096, 4096)
        f.fit(x_train=a, x_val=b, n_epochs=2, show_progress=False)
    torch.cuda.synchronize()
    print('split + Flow.fit(n_epochs=2), wall per refit over 50: %.1f us' % ((time.perf_counter() - t0) / 50 * 1e6))


if __name__ == '__main__':
    main()
