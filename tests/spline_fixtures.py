"""Trained 'c-rqnsf' flows for the host and GPU tests (tests/golden/spline_trained_*.npz, written by
tests/golden/make_golden_spline.py): loaders into the CPU restatement (oracle/flow.py) and the device flow, the row makers,
the knot filter of the fit-gradient tests, and `floor`, the restatement's own fp32 error that every tolerance of
tests/test_gpu_spline_trained.py is derived from (bound = max(the near-identity test's bound, 12 x floor))."""
import copy
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ['spline_trained_d8', 'spline_trained_d7', 'spline_trained_d24', 'spline_trained_d64']
MARGIN = 12.0       # bound / floor: what tests/test_gpu_fit_spline.py documents between its bound and the fp32 floor
_cache = {}


def load(name):
    """(oracle flow in fp32, the fixture's scalars as a dict).  The flow is a fresh copy on every call."""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
            _cache[name] = {k: z[k] for k in z.files}
    fx = _cache[name]
    from oracle import flow as oflow
    meta = {k: v.item() for k, v in fx.items() if not k.startswith('flow/') and v.ndim == 0}
    ck = {'n_hidden': meta['n_hidden'], 'n_layers': meta['n_hidden_layers']}
    of = oflow.Flow(oflow.CRQNSF((meta['d'],), n_layers=meta['n_coupling'], conditioner_kwargs=ck))
    of.load_state_dict({k[len('flow/'):]: torch.from_numpy(v.copy()) for k, v in fx.items() if k.startswith('flow/')})
    return of, meta


def device_flow(of, meta):
    """The package's flow with the restatement's weights (still on the host: the caller moves it)."""
    from nfmc_amd.flows import CRQNSF, Flow
    ck = {'n_hidden': meta['n_hidden'], 'n_layers': meta['n_hidden_layers']}
    f = Flow(CRQNSF((meta['d'],), n_layers=meta['n_coupling'], conditioner_kwargs=ck))
    f.load_state_dict(of.state_dict())
    return f


def _generator():
    """tests/golden/make_golden_spline.py as a module: the one statement of the recipe (nothing runs on import)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_spline', os.path.join(GOLDEN, 'make_golden_spline.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


recipe_rows = _generator().recipe_rows       # the fixtures' training distribution: a funnel in coordinate 0, two modes in the last


def _spread(x, factor):
    x[:max(2, x.shape[0] // 20)] *= factor          # some coordinates of these rows leave [-B, B] = [-5, 5]
    return x


def data_rows(n, d, seed):
    """Rows of the training distribution, the first max(2, n // 20) three times as far out (identity tails)."""
    return _spread(recipe_rows(n, d, seed), 3.0)


def latent_rows(n, d, seed):
    """randn, the first max(2, n // 20) rows five times as far out."""
    return _spread(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)), 5.0)


ROWS = {'spline_trained_d8': 300, 'spline_trained_d7': 257, 'spline_trained_d24': 200, 'spline_trained_d64': 130}
ROW_SEEDS = {'spline_trained_d64': 5000}      # added to the rows' seeds: the draw with the lowest fit-gradient floors of six
POTENTIALS = ('sum', 'diag', 'funnel')          # the reverse-KL targets of the fit-gradient checks


def inputs(name):
    """(oracle flow, scalars, data rows, latent rows): the input set every check of the fixture `name` runs on."""
    of, meta = load(name)
    d = meta['d']
    return of, meta, data_rows(ROWS[name], d, 100 + d + ROW_SEEDS.get(name, 0)), latent_rows(ROWS[name], d, 200 + d + ROW_SEEDS.get(name, 0))


def knot_free(of, rows, inverse, tol=1e-4):
    """(rows kept, rows with a tail coordinate): fp64 walk of the restatement's layers in the direction of the sweep; a row
    goes when any spline input lies within `tol` of a knot of that direction (width knots forward, height knots inverse)."""
    from oracle import flow as oflow
    bij = copy.deepcopy(of.bijection).double()
    h = rows.double()
    keep = torch.ones(rows.shape[0], dtype=torch.bool)
    tail = torch.zeros(rows.shape[0], dtype=torch.bool)
    layers = list(bij.layers)
    with torch.no_grad():
        for layer in (reversed(layers) if inverse else layers):
            if isinstance(layer, oflow.RQSCoupling):
                v = h[:, layer.d_a:]
                cw, ch, _ = oflow.rqs_params(layer._raw(h[:, :layer.d_a]), layer.n_bins)
                knots = ch if inverse else cw
                keep &= ~((v[..., None] - knots).abs() < tol).any(-1).any(-1)
                tail |= (v.abs() > oflow.RQS_BOUND).any(-1)
            h, _ = layer.inverse(h) if inverse else layer.forward(h)
    return keep, tail


def filtered(of, rows, inverse, need_tail=True):
    keep, tail = knot_free(of, rows, inverse)
    assert float((~keep).float().mean()) <= 0.10, 'the knot filter removed more than 10 % of the rows'
    if need_tail:
        assert int((keep & tail).sum()) >= 2, 'fewer than two rows with a tail coordinate remain'
    return rows[keep].contiguous()


def regime(of, rows, inverse):
    """(max |raw conditioner output|, min and max interior derivative, min and max bin slope, narrowest bin) over an fp64
    walk of `rows` through the couplings in the direction of the sweep."""
    from oracle import flow as oflow
    bij = copy.deepcopy(of.bijection).double()
    h = rows.double()
    raw_max, d_lo, d_hi, s_lo, s_hi, w_lo = 0.0, float('inf'), 0.0, float('inf'), 0.0, float('inf')
    layers = list(bij.layers)
    with torch.no_grad():
        for layer in (reversed(layers) if inverse else layers):
            if isinstance(layer, oflow.RQSCoupling):
                raw = layer._raw(h[:, :layer.d_a])
                cw, ch, dv = oflow.rqs_params(raw, layer.n_bins)
                w, hh = cw[..., 1:] - cw[..., :-1], ch[..., 1:] - ch[..., :-1]
                raw_max = max(raw_max, float(raw.abs().max()))
                d_lo, d_hi = min(d_lo, float(dv[..., 1:-1].min())), max(d_hi, float(dv[..., 1:-1].max()))
                s_lo, s_hi = min(s_lo, float((hh / w).min())), max(s_hi, float((hh / w).max()))
                w_lo = min(w_lo, float(w.min()), float(hh.min()))
            h, _ = layer.inverse(h) if inverse else layer.forward(h)
    return raw_max, d_lo, d_hi, s_lo, s_hi, w_lo


# ------------------------------------------------------------------------------------------------------ rows at a knot
KNOT_FIXTURES = ['spline_trained_d8', 'spline_trained_d24']
KNOT_ROWS = 8
# (fixture, inverse) -> seed of the rows.  At many knots of a fitted spline the inverse is so ill-conditioned that the fp32
# restatement's own gradient error next to the knot exceeds the cap on the floor (test_host_spline_trained.py); these seeds
# draw rows whose floors stay under it.
KNOT_SEEDS = {('spline_trained_d8', False): 300, ('spline_trained_d8', True): 302,
              ('spline_trained_d24', False): 302, ('spline_trained_d24', True): 305}
KNOT_TOL = 2e-5      # the displaced rows keep this distance from every knot: delta is 1e-4 or more, fp32 rounding 5e-7


def knot_rows(of, inverse, seed, n=KNOT_ROWS, rel=1e-3, exact=False):
    """(rows, rows_minus, rows_plus): `n` fp32 rows whose source half is random (recipe rows for the maximum-likelihood
    sweep, randn for the reverse-KL sweep) and one of whose target coordinates is set so that the spline input of the FIRST
    coupling the sweep visits equals an interior knot once rounded to fp32: coupling 0, width knots, input
    exp(s0) x + t0 (forward); the last coupling, height knots, input (z - t1) exp(-s1) (inverse).  Knots in fp64.  The
    other two sets have that coordinate moved by -delta / +delta of the spline input, delta = `rel` of the narrower
    neighbouring bin; fp32 like the rows, or fp64 with `exact` (a delta below fp32 resolution: the one-sided limits).
    Rows are kept when their neighbours at rel = 1e-3 pass the knot filter in EVERY coupling, whatever `rel` is asked for:
    the same rows for every `rel`."""
    from oracle import flow as oflow
    bij = copy.deepcopy(of.bijection).double()
    d = of.event_shape[0]
    g = torch.Generator().manual_seed(seed)
    want, n = n, 4 * n       # candidates: the first `want` whose displaced rows the knot filter passes in EVERY coupling
    rows = (torch.randn(n, d, generator=g) if inverse else recipe_rows(n, d, seed)).double()
    layers = list(bij.layers)
    ea = layers[-1] if inverse else layers[0]
    cpl = [m for m in layers if isinstance(m, oflow.RQSCoupling)][-1 if inverse else 0]
    lo, hi, slo, shi = rows.clone(), rows.clone(), rows.clone(), rows.clone()
    with torch.no_grad():
        h = ea.inverse(rows)[0] if inverse else ea.forward(rows)[0].flip(-1)   # ReversePermutation sits before a coupling
        cw, ch, _ = oflow.rqs_params(cpl._raw(h[:, :cpl.d_a]), cpl.n_bins)
        knots = ch if inverse else cw
        for i in range(n):
            j = int(torch.randint(0, cpl.d_b, (), generator=g))                # target coordinate of the coupling
            k = int(torch.randint(1, cpl.n_bins, (), generator=g))             # interior knot
            col = cpl.d_a + j if inverse else d - 1 - (cpl.d_a + j)            # its index in the row
            width = float(min(knots[i, j, k] - knots[i, j, k - 1], knots[i, j, k + 1] - knots[i, j, k]))
            for t, v in ((rows, knots[i, j, k]), (lo, knots[i, j, k] - rel * width), (hi, knots[i, j, k] + rel * width),
                         (slo, knots[i, j, k] - 1e-3 * width), (shi, knots[i, j, k] + 1e-3 * width)):
                t[i, col] = v * torch.exp(ea.log_scale[col]) + ea.shift[col] if inverse else (v - ea.shift[col]) * torch.exp(-ea.log_scale[col])
    rows = rows.float()
    if not exact:
        lo, hi = lo.float(), hi.float()
    ok = knot_free(of, slo.float(), inverse, KNOT_TOL)[0] & knot_free(of, shi.float(), inverse, KNOT_TOL)[0]
    assert int(ok.sum()) >= want
    pick = ok.nonzero()[:want, 0]
    return rows[pick].contiguous(), lo[pick].contiguous(), hi[pick].contiguous()


def per_row_grads(of, loss_fn, rows):
    """fp64: {name: (n, *shape)} gradient of each row's share of `loss_fn` (a mean over rows), and the loss."""
    f = copy.deepcopy(of).double()
    rows = rows.double()
    n = rows.shape[0]
    out = {k: [] for k, _p in f.named_parameters()}
    total = 0.0
    for i in range(n):
        f.zero_grad()
        li = loss_fn(f, rows[i:i + 1]) / n
        li.backward()
        total += float(li.detach())
        for k, p in f.named_parameters():
            out[k].append(torch.zeros_like(p) if p.grad is None else p.grad.detach().clone())
    return {k: torch.stack(v) for k, v in out.items()}, total


KNOT_REACH = 1e-4    # of the narrower neighbouring bin: how far from a knot fp32 rounding can place a point that is ON it.
# A knot is 2B cumsum(w) - B in fp32: up to 8 additions near 1 (half an ulp, 6e-8, each), times 2B = 10, is 5e-6; the
# softmax's reciprocal and exponentials add a relative 2e-7 per width, 2e-6 over the interval; the input itself 5e-7.  1e-5
# in all, against bins that are 0.1 wide or more (test_host_spline_trained.py asserts it).


def knot_band(of, loss_fn, inverse, seed):
    """The gradients a correct fp32 evaluation of the at-a-knot rows can give: per row and entry, anything between the
    one-sided fp64 gradients AT the knot (displaced by 1e-9 of the bin, in fp64) and those KNOT_REACH away on either side,
    summed over rows.  A spline fitted to data bends so sharply at some knots (derivative 1e-3 against slopes of 20) that
    the gradient changes by more than its tensor's scale within 1e-3 of a bin: the one-sided gradients 1e-3 of a bin away
    do not bracket the gradient at the knot, where even the fp64 limits lie outside them by up to 13 times the scale."""
    sets = []
    for rel in (1e-9, KNOT_REACH):
        _rows, lo, hi = knot_rows(of, inverse, seed, rel=rel, exact=True)
        sets += [per_row_grads(of, loss_fn, lo)[0], per_row_grads(of, loss_fn, hi)[0]]
    stack = {k: torch.stack([g[k] for g in sets]) for k in sets[0]}            # (4, n, *shape)
    return {k: v.amin(0).sum(0) for k, v in stack.items()}, {k: v.amax(0).sum(0) for k, v in stack.items()}


def band_widths(band):
    """{name: the band's largest width over the largest |entry| of either edge of the tensor (at least 1e-3)}."""
    low, high = band
    return {k: float((high[k] - low[k]).max()) / max(float(low[k].abs().max()), float(high[k].abs().max()), 1e-3)
            for k in low if low[k].numel()}


def band_excess(grads, band):
    """How far `grads` lies outside the band, over the largest |entry| of either edge of the tensor (at least 1e-3)."""
    low, high = band
    worst = 0.0
    for k in low:
        if low[k].numel() == 0:
            continue
        g = grads[k].double().cpu()
        scale = max(float(low[k].abs().max()), float(high[k].abs().max()), 1e-3)
        worst = max(worst, float(torch.clamp(torch.maximum(low[k] - g, g - high[k]), min=0.0).max()) / scale)
    return worst


# ---------------------------------------------------------------------------------------------- errors and the floor
def max_abs(got, want):
    """Largest absolute difference; tuples of tensors give a tuple."""
    if isinstance(got, (tuple, list)):
        return tuple(max_abs(g, w) for g, w in zip(got, want))
    return float((torch.as_tensor(got).double().cpu() - torch.as_tensor(want).double().cpu()).abs().max())


def grad_err(got, want):
    """Dicts of gradients: the largest |difference| over the largest |entry| of the tensor (at least 1e-3), worst tensor;
    the normalisation of tests/test_gpu_fit_spline.py's gradient check."""
    worst = 0.0
    for name, w in want.items():
        if w is None or w.numel() == 0:
            continue
        w = w.double().cpu()
        worst = max(worst, float((got[name].double().cpu() - w).abs().max()) / max(float(w.abs().max()), 1e-3))
    return worst


def floor(fn, of, *inputs, err=max_abs):
    """The restatement's own fp32 error: `fn(flow, *inputs)` on the float flow against the same on its .double() copy
    with the inputs promoted exactly, measured by `err`, the normalisation the check itself uses."""
    lo = fn(copy.deepcopy(of).float(), *[t.float() if torch.is_tensor(t) and t.is_floating_point() else t for t in inputs])
    hi = fn(copy.deepcopy(of).double(), *[t.double() if torch.is_tensor(t) and t.is_floating_point() else t for t in inputs])
    return err(lo, hi)


def bound(existing, fl):
    """The tolerance rule: the bound the near-identity test of the same quantity uses, or 12 x the floor if larger."""
    return max(float(existing), MARGIN * float(fl))


# ------------------------------------------------------------------------------------- functions `floor` is taken of
def forward_fn(f, x):
    with torch.no_grad():
        return f.bijection.forward(x)


def inverse_fn(f, z):
    with torch.no_grad():
        return f.bijection.inverse(z)


def log_prob_fn(f, x):
    with torch.no_grad():
        return f.log_prob(x)


def round_trip_fn(f, x):
    with torch.no_grad():
        z, ld = f.bijection.forward(x)
        xb, ldb = f.bijection.inverse(z)
    return xb - x, ldb + ld


def log_q_fn(f, z):
    """log q of the proposal x = f^-1(z), as the flow-proposal Metropolis step computes it."""
    with torch.no_grad():
        _x, ld = f.bijection.inverse(z)
        return f.base_log_prob(z) - ld


def proposal_fn(target):
    """log q(x') + U(x') of the proposal x' = f^-1(z): everything a proposal adds to the Metropolis log-ratio."""
    def fn(f, z):
        with torch.no_grad():
            x, ld = f.bijection.inverse(z)
            return f.base_log_prob(z) - ld + target(x)
    return fn


def potential_cpu(kind, d, dtype=torch.float32):
    """Differentiable torch form of the reverse-KL targets 'sum', 'diag', 'funnel' in `dtype`."""
    if kind == 'sum':
        return lambda x: (x * x).sum(-1)
    if kind == 'diag':
        mu, sd = torch.linspace(-0.5, 0.5, d).to(dtype), torch.linspace(0.6, 1.7, d).to(dtype)
        return lambda x: 0.5 * (((x - mu) / sd) ** 2).sum(-1)
    from oracle import potentials as opot
    return opot.funnel(3.0)


def device_potential(kind, d):
    """The package's closed-form potentials behind the names of `potential_cpu`."""
    from nfmc_amd.potentials import DiagonalGaussian, Funnel, SumOfSquares
    if kind == 'sum':
        return SumOfSquares((d,))
    if kind == 'diag':
        return DiagonalGaussian((d,), torch.linspace(-0.5, 0.5, d), torch.linspace(0.6, 1.7, d))
    return Funnel((d,), 3.0)


def nll_loss(f, x):
    return -f.log_prob(x).mean()


def reverse_kl_loss(kind):
    def loss(f, z):
        x, ld = f.bijection.inverse(z)
        return (f.base_log_prob(z) - ld + potential_cpu(kind, z.shape[1], z.dtype)(x)).mean()
    return loss


def loss_and_grads(loss_fn):
    """fn for `floor`: (loss, {parameter name: gradient}) of `loss_fn(flow, rows)` by autograd."""
    def fn(f, rows):
        f.zero_grad()
        loss = loss_fn(f, rows)
        loss.backward()
        return loss.detach(), {k: p.grad.detach().clone() for k, p in f.named_parameters() if p.grad is not None}
    return fn


def loss_grad_err(got, want):
    """(relative-and-absolute loss error: |difference| / (1 + |loss|), gradient error as `grad_err`)."""
    (lg, gg), (lw, gw) = got, want
    return abs(float(lg) - float(lw)) / (1.0 + abs(float(lw))), grad_err(gg, gw)


# ------------------------------------------------------------------------------------------- the device fit's gradient
def check_gradient(fit, f, of, loss, dev, padded=True, loss_tol=3e-5, grad_tol=3e-4):
    """fit.m (beta1 = 0: the gradient) and the reported loss against `loss` of the restatement `of` and its autograd: the
    loss within `loss_tol` (relative and absolute), every entry within `grad_tol` of the largest entry of its tensor, the
    padding of the blob exactly zero.  Returns (loss error / (1 + |loss|), worst gradient error / scale)."""
    loss.backward()
    loss_gpu, applied, _val = (float(v) for v in fit.status.cpu())
    assert applied == 1.0
    print('loss device %.8g oracle %.8g' % (loss_gpu, float(loss.detach())))
    g = copy.deepcopy(f)
    fit.write_back(fit.m, bijection=g.bijection)                        # the gradient, laid out as parameters
    want = dict(of.named_parameters())
    worst = []
    for name, p in g.named_parameters():
        w = want[name].grad
        if w is None or w.numel() == 0:      # d = 1: the source half is empty, W1 has no entries
            continue
        scale = max(float(w.abs().max()), 1e-3)
        worst.append((float((p.detach().cpu() - w).abs().max()) / scale, name))
    print('worst gradient error / scale: %.3g (%s)' % max(worst))
    np.testing.assert_allclose(loss_gpu, float(loss.detach()), rtol=loss_tol, atol=loss_tol)
    for err, name in worst:
        assert err <= grad_tol, (name, err)
    if padded:
        # the padded entries of the blob (hidden units beyond n_hidden, alignment gaps) carry no gradient
        used = torch.zeros_like(fit.m, dtype=torch.bool)
        for _p, off, r, c, rs, cs in fit._layout(f.bijection):
            idx = off + torch.arange(r, device=dev)[:, None] * rs + torch.arange(c, device=dev)[None, :] * cs
            used[idx.reshape(-1)] = True
        assert int(used.sum()) > 0
        assert float(fit.m[~used].abs().max() if (~used).any() else 0.0) == 0.0
    lw = float(loss.detach())
    return abs(loss_gpu - lw) / (1.0 + abs(lw)), max(worst)[0]


def device_gradient(fit, f):
    """{parameter name: gradient on the host} of a DeviceFit step taken with beta1 = 0 (fit.m is the gradient)."""
    g = copy.deepcopy(f)
    fit.write_back(fit.m, bijection=g.bijection)
    return {name: p.detach().cpu() for name, p in g.named_parameters()}


# ------------------------------------------------------------------------------------------ flow-proposal Metropolis
MH_CHAINS, MH_STEPS, MH_SEED = 70, 5, 4242


def metropolis_oracle(of, meta, target):
    """The fp64 oracle run of the flow-proposal Metropolis checks (n = 70, T = 5, Philox seed 4242; target 'sumsq' or
    'funnel') and the floors of its log-ratios, all on the CPU.  A log-ratio is [-U(x') - log q(x')] - [-U(x) - log q(x)],
    x the state the chain carries.  Returns a dict:
      x0, trace, want_lr, want_m    the start, the oracle's trace, its log-ratios and decisions (T, n)
      fl_q                          the fp32 restatement's largest log q error over the oracle's proposals
      entry                         (T, n): the fp32 restatement's own error in log q + U (the two parts' absolute errors
                                    added) of that entry's proposal, plus that of the state its chain carries there
      fl_x                          the fp32 restatement's largest error of a proposal x'
      tol, ptol                     (T, n) bounds: max(existing bound, 12 max(fl_q, entry)); and, between two device kernels,
                                    max(0.2 existing bound, 12 entry)
    `entry` widens the bound only where it belongs: a proposal that passes a knot of derivative 1e-3 carries 6e-4 in x', which
    U multiplies by the target's gradient, in that entry and in those of a chain that accepted it."""
    from oracle import philox, potentials as opot, samplers as osamp
    d, n, T = meta['d'], MH_CHAINS, MH_STEPS
    u = opot.sum_squares if target == 'sumsq' else opot.funnel(3.0)
    of64 = copy.deepcopy(of).double()
    x0 = 0.7 * torch.randn(n, d, generator=torch.Generator().manual_seed(d + meta['n_hidden']))
    tr = osamp.imh_sample(x0.double(), u, of64, T, noise=osamp.PhiloxNoise(MH_SEED, dtype=torch.float64))
    want_lr, want_m = torch.stack(tr.log_ratios).numpy(), torch.stack(tr.masks).numpy()
    noise = osamp.PhiloxNoise(MH_SEED)
    zs = [noise.normal(n, (d,), t, philox.TAG_LATENT) for t in range(T)]
    fl_q = floor(log_q_fn, of, torch.cat(zs))
    fl_x = floor(inverse_fn, of, torch.cat(zs))[0]

    def parts(flow, z, dtype):
        with torch.no_grad():
            x, ld = flow.bijection.inverse(z.to(dtype))
            return (flow.base_log_prob(z.to(dtype)) - ld).double(), u(x).double()
    with torch.no_grad():
        carried = ((of.log_prob(x0).double() - of64.log_prob(x0.double())).abs() + (u(x0).double() - u(x0.double())).abs()).numpy()
    entry = np.zeros((T, n))
    for t in range(T):
        (q32, u32), (q64, u64) = parts(of, zs[t], torch.float32), parts(of64, zs[t], torch.float64)
        own = ((q32 - q64).abs() + (u32 - u64).abs()).numpy()
        entry[t] = own + carried
        carried = np.where(want_m[t], own, carried)
    existing = 3e-4 * max(1.0, d / 64) + 3e-5 * np.abs(want_lr)
    return dict(x0=x0, trace=tr, want_lr=want_lr, want_m=want_m, fl_q=fl_q, entry=entry, fl_x=fl_x,
                tol=np.maximum(existing, MARGIN * np.maximum(fl_q, entry)), ptol=np.maximum(0.2 * existing, MARGIN * entry))
