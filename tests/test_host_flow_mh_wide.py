"""CPU: the inputs of every case of tests/test_gpu_flow_mh_wide.py hold their conditions for the fp64 oracle alone (an
acceptance of at least 0.25, under 10 % of the chains within 1e-3 of a tie, finite log ratios; the unadjusted cases:
finite log ratios), the arithmetic behind the two d at the LDS bound, and the figure behind the tolerance constant: the
oracle flow cast to fp32 against itself in fp64 at each affine case's own proposals."""
import torch

import target_harness as H
import test_gpu_flow_mh_wide as G


def test_every_gpu_case_holds_its_input_conditions_on_the_oracle_alone(monkeypatch, capsys):
    count = H.probe_flow_inputs(G, monkeypatch)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if 'oracle accepts' in ln or 'unadjusted' in ln]
    acc = [float(ln.split('oracle accepts ')[1].split()[0]) for ln in lines if 'oracle accepts' in ln]
    assert count == G.N_FLOW_CASES == 90, (count, G.N_FLOW_CASES)
    assert len(lines) >= count and min(acc) >= G.FLOOR
    print('\n'.join(lines))
    print('flow_mh_wide: proved the inputs of %d GPU cases, oracle acceptance %.3f .. %.3f' % (count, min(acc), max(acc)))


def test_case_matrix_reaches_every_kernel_and_bucket():
    assert {c.kernel for c in G.CASES} == {'mfma', 'wide', 'lane'}
    for kernel in ('mfma', 'wide', 'lane'):
        mine = [c for c in G.CASES if c.kernel == kernel]
        assert {'sumsq', 'funnel', 'quadratic', 'diagonal'} == {c.target for c in mine}
        assert any(c.n == 1 for c in mine) and any(c.cl % 2 for c in mine)
        assert {c.kernel for c in G.SUBSET} >= {kernel} and sum(c.kernel == kernel for c in G.ONE_PER_KERNEL) == 1
    assert all(c.d in (64, 128) and 32 < c.nh <= 128 and c.hl in (1, 2) for c in G.MFMA)
    assert all(c.d % 32 == 0 and c.d not in (64, 128) and 32 <= c.d <= 512 and 32 < c.nh <= 128 for c in G.WIDE)
    lane = [c for c in G.LANE if c.env is None and not c.spline]
    assert all(8 < c.nh <= 32 or c.d % 32 or c.d > 512 for c in lane)
    buckets = {4 if c.nh <= 4 else 8 if c.nh <= 8 else 16 if c.nh <= 16 else 32 if c.nh <= 32 else 64 if c.nh <= 64 else 128
               for c in G.LANE}
    assert buckets == {4, 8, 16, 32, 64, 128}
    assert all(c.n <= 700 for c in G.CASES)


def _tile_stride(d):
    s = (d + 3) & ~3                    # csrc/flow_device.hpp: tile_stride
    return s + 4 if (s >> 2) & 1 == 0 else s


def test_the_two_d_at_the_lds_bound():
    def lds(d):                         # csrc/flow_kernels.hip: flow_mh_tile_lds at n_hidden = 128
        return 2 * 64 * _tile_stride(d) * 4 + 128 * 64 * 4
    assert (_tile_stride(G.LDS_FITS), lds(G.LDS_FITS)) == (252, 161792) and lds(G.LDS_FITS) <= 160 * 1024
    assert (_tile_stride(G.LDS_REFUSED), lds(G.LDS_REFUSED)) == (260, 165888) and lds(G.LDS_REFUSED) > 160 * 1024
    assert G.LDS_REFUSED == G.LDS_FITS + 1 and all(lds(d) <= 160 * 1024 for d in range(2, G.LDS_FITS + 1))
    assert G.LDS_FITS % 32 and G.LDS_REFUSED % 32


def test_affine_c_covers_four_times_the_fp32_oracles_error_or_the_case_is_in_the_table(capsys):
    """spline_c's measurement on the affine cases: where 4 x the worst fp32-against-fp64 |log q| difference exceeds
    affine_c(d) the case must be in C_FIGURES with that figure (to 10 %); no other case may be."""
    worst_all = 0.0
    for c in G.CASES:
        if c.spline:
            continue
        _q, (_f, of) = G._inputs(c)
        _cc, worst = H.spline_c(c.d, of, G._oracle(c).flow_steps)
        worst_all = max(worst_all, worst)
        print('%s: fp32 oracle against fp64 %.2e, affine_c %.2e' % (G._id(c), worst, H.affine_c(c.d)))
        if H.SPLINE_C_FACTOR * worst > H.affine_c(c.d):
            assert G._id(c) in G.C_FIGURES and abs(G.C_FIGURES[G._id(c)] / worst - 1.0) < 0.1, (G._id(c), worst)
        else:
            assert G._id(c) not in G.C_FIGURES, G._id(c)
    print('worst over the affine cases %.2e' % worst_all)


def test_hidden_layer_count_reaches_both_flows():
    c = G.BY_ID['mfma-sumsq-d128-h40x1-c3']
    _q, (f, of) = G._inputs(c)
    assert f.bijection.n_hidden_layers == 1 and f.bijection.n_hidden == 40 and f.bijection.n_coupling == 3
    for k, v in f.state_dict().items():
        assert torch.equal(v.double(), of.state_dict()[k]), k
