"""The shadowing harness (oracle/shadow.py) on the host: the fp32 oracle, standing in for a kernel, passes it, and the
kinds of error a kernel can make are flagged -- a harness that cannot fail tests nothing.

The stand-in run is C4-shaped but small: NeuTra HMC on the funnel, d = 16, conditioner 16 x 2, weights perturbed
until the conditioner pre-activations reach |a| ~ 6 (deep tanh saturation, as a fitted funnel flow has), L = 10,
h = 0.15 (acceptance ~0.93)."""
import copy

import pytest
import torch

from oracle import flow as oflow, potentials as opot, samplers as osamp, shadow

KAPPA = 8.0
D, N, T, L, H, SEED = 16, 64, 12, 10, 0.15, 7


def _flow():
    torch.manual_seed(5)
    return oflow.perturb_(oflow.Flow(oflow.RealNVP((D,), conditioner_kwargs={'n_hidden': 16, 'n_layers': 2})), 3, 0.5)


def _run(flow, h=H):
    z0 = torch.randn(N, D, generator=torch.Generator().manual_seed(0))
    tr = osamp.neutra_hmc_sample(z0, opot.funnel(3.0), flow, T, h, None, L, noise=osamp.PhiloxNoise(SEED))
    return torch.cat([z0[None], tr.stacked()]), tr


def _workload(flow):
    return shadow.Workload('neutra_hmc', opot.funnel(3.0), flow, H, L)


@pytest.fixture(scope='module')
def base():
    f = _flow()
    states, tr = _run(f)
    return f, states, tr, shadow.shadow(states, _workload(f), SEED)


def test_fp32_oracle_passes_the_harness(base):
    f, states, tr, rep = base
    assert rep.failures(KAPPA) == []
    s = rep.summary()
    assert s['transitions'] == T and s['clear_mismatches'] == 0
    assert abs(s['acceptance_inner'] - tr.n_accepted / (N * T)) < 1e-12   # changed rows == the oracle's accept count
    assert 0.8 < s['acceptance_inner'] < 1.0
    assert s['ratio_max'] == 1.0 and s['ratio_mean'] == 1.0                # the stand-in IS the fp32 yardstick
    # the regime the issue is about: conditioner pre-activations deep in tanh saturation on the visited states
    with torch.no_grad():
        pre = f.bijection.layers[2].conditioner[0](states[-1][:, :D // 2])
    assert float(pre.abs().max()) > 4


def test_output_bias_off_by_1e_3_is_flagged(base):
    f, _states, _tr, _rep = base
    g = copy.deepcopy(f)
    with torch.no_grad():
        g.bijection.layers[2].conditioner[-1].bias[D // 2] += 1e-3     # one shift of one coupling
    states, _ = _run(g)
    fails = shadow.shadow(states, _workload(f), SEED).failures(KAPPA)
    assert any(m.startswith('states') for m in fails), fails


def test_step_size_off_by_1e_4_relative_is_flagged(base):
    f, _states, _tr, _rep = base
    states, _ = _run(f, H * (1 + 1e-4))
    fails = shadow.shadow(states, _workload(f), SEED).failures(KAPPA)
    assert any(m.startswith('states') for m in fails), fails


def test_two_chains_swapped_after_one_transition_are_flagged(base):
    f, states, _tr, _rep = base
    s = states.clone()
    s[1, [3, 40]] = s[1, [40, 3]]
    fails = shadow.shadow(s, _workload(f), SEED).failures(KAPPA)
    assert fails, 'swap not flagged'


def test_one_flipped_accept_is_flagged(base):
    f, states, tr, rep = base
    t = T - 1
    acc = (states[t + 1] != states[t]).any(dim=1)
    lr, lu = tr.log_ratios[t], tr.uniforms[t]
    c = int(((lr - lu) * acc).argmax())                 # the accepted chain with the clearest margin
    assert acc[c] and float(lr[c] - lu[c]) > 0.1
    s = states.clone()
    s[t + 1, c] = s[t, c]                               # the kernel "rejected" it
    r = shadow.shadow(s, _workload(f), SEED)
    fails = r.failures(KAPPA)
    assert any('decisions differ' in m for m in fails), fails
    assert r.mismatches[0][:2] == (t, c)
    assert r.accepted_inner == tr.n_accepted - 1       # and the counter check would see it


def test_jump_and_imh_workloads_pass_with_the_fp32_oracle():
    """The jump (MALA inner + flow-proposal MH) and IMH kinds of the harness on the fp32 oracle's own runs; the IMH
    transition through `imh_sample(step0=...)` equals the harness's flow-proposal transition from the same pre-states."""
    d, n, K, seed = 8, 48, 3, 11
    torch.manual_seed(2)
    f = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,))), 4, 0.1, 0.7071)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(1))
    tr = osamp.jump_sample(x0, opot.sum_squares, f, 'langevin', 2, K, d ** (-1 / 3), noise=osamp.PhiloxNoise(seed))
    rep = shadow.shadow(torch.cat([x0[None], tr.stacked()]), shadow.Workload('jump_mala', opot.sum_squares, f, d ** (-1 / 3),
                                                                              n_inner=K), seed)
    assert rep.failures(KAPPA) == [] and rep.n_transitions == 2 * (K + 1)
    assert rep.accepted_inner == tr.n_accepted and rep.accepted_jumps == tr.n_accepted_jumps
    ti = osamp.imh_sample(x0, opot.sum_squares, f, 5, noise=osamp.PhiloxNoise(seed))
    states = torch.cat([x0[None], ti.stacked()])
    rep = shadow.shadow(states, shadow.Workload('imh', opot.sum_squares, f), seed)
    assert rep.failures(KAPPA) == [] and rep.accepted_jumps == ti.n_accepted
    for t in range(5):
        one = osamp.imh_sample(states[t], opot.sum_squares, f, 1, noise=osamp.PhiloxNoise(seed), step0=t)
        js = osamp.jump_transition(states[t].clone(), opot.sum_squares, f, t, osamp.PhiloxNoise(seed))
        assert torch.equal(one.last, js.x) and torch.equal(one.last, states[t + 1])


def test_fp64_oracle_transition_uses_the_fp32_draws():
    """The fp64 run draws the fp32 Philox values, promoted: the fp64 and fp32 transitions agree to fp32 rounding."""
    f = _flow()
    z = torch.randn(N, D, generator=torch.Generator().manual_seed(0))
    wl = _workload(f)
    a = shadow.one_transition(wl, z.double(), 3, osamp.PhiloxNoise(SEED, dtype=torch.float64), copy.deepcopy(f).double(),
                              opot.funnel(3.0))
    b = shadow.one_transition(wl, z, 3, osamp.PhiloxNoise(SEED), f, opot.funnel(3.0))
    assert a.x.dtype == torch.float64 and b.x.dtype == torch.float32
    same = a.mask == b.mask
    assert float(same.float().mean()) > 0.95
    assert float((a.x[same] - b.x[same].double()).abs().max()) < 1e-3
