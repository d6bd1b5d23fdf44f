"""CPU: what tests/test_gpu_neutra_hmc_wide.py rests on, from the fp64 oracle and the library's host functions alone.
Every oracle-backed run (G.RUNS) holds its input conditions (acceptance 0.30 .. 0.95, under 10 % of the chains within
their margin of a tie, finite log ratios); the figure table (the fp32 oracle against the fp64 one) is measured again and
held to 10 %; the case matrix reaches every template instance and every value of every axis on both kernels; the
arithmetic behind the second-tile n; and the two work-area formulas against nfmc_neutra_scratch_bytes."""
import torch

import target_harness as H
import test_gpu_neutra_hmc_wide as G


def test_every_oracle_backed_run_holds_its_input_conditions(capsys):
    accs = []
    for r in G.RUNS:
        acc, ties = G.conditions(r)
        if r.adjust:
            accs.append(acc)
            assert 0.30 <= acc <= 0.95 and ties < G.CAP, G._key(r)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if 'oracle accepts' in ln]
    assert len(lines) == len(accs) == len(G.RUNS) - 2            # the two unadjusted runs have no decision
    print('\n'.join(lines))
    print('neutra_hmc_wide: proved the inputs of %d runs, oracle acceptance %.3f .. %.3f' % (len(G.RUNS), min(accs), max(accs)))


def test_figure_table_is_the_fp32_oracles_error_to_ten_percent():
    """H.neutra_hmc_figures on every run's own inputs; no run without an entry, no entry without a run"""
    assert set(G.FIGURES) == set(G.RUN_OF)
    for r in G.RUNS:
        state, lr = G.measure(r)
        want_state, want_lr = G.FIGURES[G._key(r)]
        print('%s: fp32 oracle against fp64: states %.2e (table %.2e), log ratios %.2e (table %.2e)' % (G._key(r), state, want_state, lr, want_lr))
        assert abs(want_state / state - 1.0) < 0.1, (G._key(r), state, want_state)
        assert (lr == want_lr == 0.0) if not r.adjust else abs(want_lr / lr - 1.0) < 0.1, (G._key(r), lr, want_lr)


def test_case_matrix_reaches_every_kernel_instance_and_axis_value():
    assert 28 <= len(G.CASES) <= 32
    for kernel, cases, ds in (('mfma', G.MFMA, {64, 128}), ('wide', G.WIDE, {32, 96, 256, 512})):
        assert all(c.kernel == kernel == H.neutra_hmc_kernel_of(c.d, c.nh, c.hl) for c in cases)
        assert {c.d for c in cases} == ds
        th = lambda c: H._padded_hidden(H.neutra_presented_hidden(c.d, c.nh, c.hl)) // 16        # noqa: E731
        instances = {(c.d // 16 if kernel == 'mfma' else 0, th(c), c.hl) for c in cases}
        assert instances == {(td, t, nhl) for td in ({4, 8} if kernel == 'mfma' else {0}) for t in (4, 8) for nhl in (1, 2)}, instances
        assert {40, 100} <= {c.nh for c in cases}
        assert {c.cl for c in cases} == {1, 2, 3}
        assert {c.n for c in cases} == {150, 1}
        assert {c.target for c in cases} == {'sumsq', 'funnel', 'quadratic', 'diagonal'}
        assert {c.mass for c in cases} == {True, False}
        assert all(c.n <= 200 and c.L <= 4 for c in cases) and {c.L for c in cases} >= {1, 3, 4}
        assert G.ODD[kernel].cl % 2 == 1 and G.ODD[kernel].mass and G.EVEN[kernel].cl % 2 == 0 and G.SECOND[kernel].n == G.BIG
    assert any(c.d == 64 and c.nh == 6 for c in G.MFMA)
    assert H.neutra_presented_hidden(64, 6, 2) == 64 and H.neutra_hmc_kernel_of(64, 6, 2) == 'mfma'
    assert all(r.T <= 6 for r in G.RUNS)


def test_kernel_naming_follows_the_shape_rules():
    K = H.neutra_hmc_kernel_of
    assert [K(d, 64, 2) for d in (32, 64, 96, 128, 160, 256, 512)] == ['wide', 'mfma', 'wide', 'mfma', 'wide', 'wide', 'wide']
    assert K(64, 33, 1) == 'mfma' and K(64, 128, 2) == 'mfma' and K(64, 129, 2) is None and K(64, 64, 3) is None
    assert K(64, 8, 2) == 'mfma' and K(64, 8, 3) == 'valu' and K(96, 32, 2) == 'valu' and K(96, 33, 2) == 'wide'
    assert K(48, 64, 2) is None and K(544, 64, 2) is None and K(16, 64, 2) is None
    assert K(64, 64, 2, 8) == 'valu' and K(96, 16, 2, 8) == 'valu'


def test_second_tile_arithmetic():
    """n = 256 x 128 + 40: 257 tiles on kCkMaxGrid = 256 workgroup slots, so exactly one workgroup (slot 0) takes a second
    tile, the ragged one of 40 chains; the largest n of the suite so far, 32768, has exactly 256"""
    tiles = -(-G.BIG // H.MFMA_CHAINS)
    assert (H.MFMA_CHAINS, H.CK_MAX_GRID, tiles) == (128, 256, 257) and tiles > H.CK_MAX_GRID
    assert -(-32768 // H.MFMA_CHAINS) == H.CK_MAX_GRID
    assert G.BIG - (tiles - 1) * H.MFMA_CHAINS == 40 and G.TAIL == 128 + 40
    assert (tiles - 1) % H.CK_MAX_GRID == 0                       # tile 256 goes to the slot of tile 0
    assert G.BIG * 512 < 2 ** 31


def test_the_two_scratch_formulas_are_the_librarys():
    from nfmc_amd import hip
    lib = hip.lib()
    shapes = [(c.n, c.d, H.neutra_presented_hidden(c.d, c.nh, c.hl), c.hl, c.cl, c.kernel) for c in G.CASES + list(G.SECOND.values())]
    shapes += [(75, c.d, H.neutra_presented_hidden(c.d, c.nh, c.hl), c.hl, c.cl, c.kernel) for c in G.EVEN.values()]
    for n, d, hidden, hl, cl, kernel in shapes:
        got = int(lib.nfmc_neutra_scratch_bytes(n, d, hidden, hl, cl))
        mine = H.neutra_hmc_scratch_bytes(kernel, n, d, hidden, hl, cl)
        other = H.neutra_hmc_scratch_bytes('wide' if kernel == 'mfma' else 'mfma', n, d, hidden, hl, cl)
        assert got == mine and got != other, (n, d, hidden, hl, cl, kernel, got, mine, other)
    assert int(lib.nfmc_neutra_scratch_bytes(150, 64, 32, 2, 2)) == 0           # the one-chain-per-lane kernels take no work area
    assert int(lib.nfmc_realnvp_padded_hidden(33)) == int(lib.nfmc_realnvp_padded_hidden(64)) == 64 == H._padded_hidden(40)
    assert int(lib.nfmc_realnvp_padded_hidden(65)) == int(lib.nfmc_realnvp_padded_hidden(128)) == 128 == H._padded_hidden(100)


def test_flows_hold_the_same_weights_and_the_architecture_asked_for():
    c = G.BY_ID['mfma-sumsq-d128-h40x2-c3-L3']
    _p, f, of = G._inputs(c)
    assert (f.bijection.n_hidden_layers, f.bijection.n_hidden, f.bijection.n_coupling) == (2, 40, 3)
    for k, v in f.state_dict().items():
        assert torch.equal(v.double(), of.state_dict()[k]), k
