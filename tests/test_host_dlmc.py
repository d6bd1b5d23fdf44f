"""CPU: DLMC routing and defaults, and the fp64 oracle of the DLMC loop (oracle.samplers.dlmc_sample, dlmc.py:45-127)
reproducing the reference's fixtures (tests/golden/make_golden_dlmc.py).  The GPU tests (test_gpu_dlmc.py) compare
against the same oracle."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import golden_flow, load_golden  # noqa: E402


def _sumsq(x):
    return torch.sum(x ** 2, dim=-1)


def _nll(shift):
    return lambda x: 0.5 * torch.sum((x - shift) ** 2, dim=-1)


@pytest.mark.parametrize('name', ['dlmc_d6', 'dlmc_latent_d6'])
def test_restatement_reproduces_reference_fixture(name):
    from oracle import samplers as osamp
    fx = load_golden(name)
    flow = golden_flow(fx, 6)
    T = int(fx['n_iterations'])
    noise = osamp.ReplayNoise(torch.from_numpy(fx['noise/normals']).double(),
                              torch.from_numpy(fx['noise/uniforms']).double())
    tr = osamp.dlmc_sample(torch.from_numpy(fx['x0']), _sumsq, _nll(float(fx['nll_shift'])), flow, T,
                           float(fx['step_size']), latent=bool(fx['latent_updates']), noise=noise)
    assert np.allclose(tr.stacked().numpy(), fx['exp/samples'], atol=1e-5)
    c = fx['exp/counters']   # accepted, attempted, divergences, target calls, gradient calls
    n = fx['x0'].shape[0]
    assert (tr.n_accepted, tr.n_attempted, tr.n_divergences, tr.n_target_calls, tr.n_target_gradient_calls) == \
        tuple(int(v) for v in c)
    assert tr.n_attempted == n * T
    assert 0 < tr.n_accepted < n * T
    np.testing.assert_allclose(tr.moments.first.numpy(), fx['exp/first_moment'], atol=1e-5)
    np.testing.assert_allclose(tr.moments.second.numpy(), fx['exp/second_moment'], atol=1e-5)


def test_oracle_draws_the_flow_mh_stream_of_the_sampler():
    """Under PhiloxNoise iteration t of dlmc_sample draws the latents at step step0 + t with TAG_LATENT and the accept
    uniform with TAG_JUMP: the words DLMC.sample hands launch_flow_mh / split_flow_mh (step i, one transition)."""
    from oracle import flow as oflow, philox, samplers as osamp
    d, n, T, seed = 5, 7, 3, 123
    torch.manual_seed(0)
    of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,))), 4, 0.2, 0.8)
    x0 = torch.randn(n, d)
    rec = osamp.RecordingNoise(osamp.PhiloxNoise(seed, dtype=torch.float64))
    tr = osamp.dlmc_sample(x0, _sumsq, _nll(0.0), of, T, 0.05, noise=rec, step0=2)
    assert len(rec.normals) == len(rec.uniforms) == T
    ids = np.arange(n, dtype=np.uint32)
    for t in range(T):
        want_z = philox.normal_field(seed, ids, 2 + t, d, philox.TAG_LATENT)
        assert np.array_equal(rec.normals[t].numpy(), want_z.reshape(n, d).astype(np.float64))
        assert np.array_equal(rec.uniforms[t].numpy(), philox.jump_uniform(seed, ids, 2 + t).astype(np.float64))
    replay = osamp.dlmc_sample(x0, _sumsq, _nll(0.0), of, T, 0.05, noise=osamp.ReplayNoise(rec.normals, rec.uniforms))
    assert torch.equal(replay.stacked(), tr.stacked()) and replay.n_accepted == tr.n_accepted
    assert (tr.n_target_calls, tr.n_target_gradient_calls) == (n + 3 * n * T, n + n * T)


def test_create_sampler_routes_dlmc_with_reference_defaults():
    from nfmc_amd.sample import create_sampler
    from nfmc_amd.samplers.dlmc import DLMC, DLMCKernel, DLMCParameters
    nll = _nll(0.0)
    s = create_sampler(_sumsq, (5,), strategy='dlmc', negative_log_likelihood=nll, param_kwargs={'n_iterations': 7})
    assert isinstance(s, DLMC) and isinstance(s.kernel, DLMCKernel) and isinstance(s.params, DLMCParameters)
    assert s.negative_log_likelihood is nll and s.target is _sumsq
    assert s.kernel.step_size == 0.05 and s.params.latent_updates is False            # dlmc.py:14, 19
    assert s.params.n_iterations == 7
    assert (s.params.train_pct, s.params.max_train_size, s.params.max_val_size) == (0.7, 4096, 4096)
    fk = s.params.flow_fit_kwargs
    assert fk['early_stopping'] is True and fk['early_stopping_threshold'] == 50 and fk['batch_size'] == 'adaptive'
    assert len(s.kernel.flow.bijection.layers) == 6
    s2 = create_sampler(_sumsq, (5,), strategy='dlmc', flow='nice', negative_log_likelihood=nll,
                        kernel_kwargs={'step_size': 0.3}, param_kwargs={'latent_updates': True})
    assert s2.params.latent_updates is True


def test_direct_construction_like_reference():
    from nfmc_amd.samplers.dlmc import DLMC, DLMCKernel, DLMCParameters
    s = DLMC(event_shape=(5,), target=_sumsq, negative_log_likelihood=_sumsq)
    assert s.kernel.step_size == 0.05 and s.params.latent_updates is False and s.params.n_iterations == 100
    assert s.kernel.flow is not None and tuple(s.kernel.flow.event_shape) == (5,)
    k = DLMCKernel((5,), step_size=0.2)
    p = DLMCParameters(n_iterations=3, latent_updates=True)
    s = DLMC((5,), _sumsq, _sumsq, k, p)
    assert s.kernel is k and s.params is p


def test_dlmc_is_a_supported_strategy_and_needs_a_likelihood():
    from nfmc_amd.sample import create_sampler
    from nfmc_amd.util import get_supported_nfmc_samplers, get_supported_samplers
    assert 'dlmc' in get_supported_nfmc_samplers() and 'dlmc' in get_supported_samplers()
    with pytest.raises(ValueError, match='Negative log likelihood must be provided'):
        create_sampler(_sumsq, (4,), strategy='dlmc')
    with pytest.raises(ValueError, match='Unsupported sampling strategy'):
        create_sampler(_sumsq, (4,), strategy='dlmc', negative_log_likelihood=None)
    for other in ('ess', 'jump_ess', 'tess', 'nuts'):
        with pytest.raises(ValueError, match='Unsupported sampling strategy'):
            create_sampler(_sumsq, (4,), strategy=other, negative_log_likelihood=_sumsq)


def test_warmup_returns_x0_only():
    from nfmc_amd.samplers.dlmc import DLMC
    s = DLMC((3,), _sumsq, _sumsq)
    x0 = torch.randn(4, 3)
    out = s.warmup(x0, show_progress=False)
    assert torch.equal(out.running_samples.last_sample.cpu(), x0)


# ---- the launch geometry of csrc/dlmc_kernels.hip, restated for the GPU tests (test_gpu_dlmc.py) that pick shapes on
# both sides of every rows-per-wave switch and past the grid-stride threshold
LDS_BUDGET = 150 * 1024   # neutra_rows_per_wave (csrc/neutra_kernels.hpp)
DLMC_TILES = 3            # x, w and g wave tiles (dlmc_launch)
GRID_TILES = 4 * 2048     # 4 * kMaxGrid (csrc/common.hpp) workgroups per launch; more tiles grid-stride


def tile_stride(d):
    """tile_stride (csrc/flow_device.hpp): d rounded up to 4 floats, plus 4 when that is a multiple of 8."""
    s = (d + 3) & ~3
    return s + 4 if ((s >> 2) & 1) == 0 else s


def dlmc_rows_per_wave(d):
    for rpw in (64, 32, 16):
        if DLMC_TILES * rpw * tile_stride(d) * 4 <= LDS_BUDGET:
            return rpw
    return 0


def hp_bucket(n_hidden):
    return 4 if n_hidden <= 4 else 8


def test_launch_geometry_restated_from_the_kernel_source():
    """The restatement above against the source it restates, and the switch points it puts at 196 | 197 (64 -> 32
    rows) and 396 | 397 (32 -> 16 rows): a change to the formula fails here before it silently moves the GPU tests' shapes
    off the boundaries."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nfmc_amd', 'csrc')

    def src(name):
        with open(os.path.join(csrc, name)) as fh:
            return ' '.join(fh.read().split())
    dl, nk, fd, cm = (src(n) for n in ('dlmc_kernels.hip', 'neutra_kernels.hpp', 'flow_device.hpp', 'common.hpp'))
    assert 'const int rpw = neutra_rows_per_wave(f.d, 3);' in dl
    assert 'const size_t lds = (size_t)3 * rpw * tile_stride(f.d) * sizeof(float);' in dl
    assert 'const int grid = (int)(tiles < 4 * kMaxGrid ? tiles : 4 * kMaxGrid);' in dl
    assert 'const int hp = hp_bucket_n(f.n_hidden);' in dl
    assert ('for (int rpw = 64; rpw >= 16; rpw >>= 1) if ((size_t)tiles_of_d * rpw * tile_stride(d) * sizeof(float) '
            '<= 150 * 1024) return rpw;') in nk
    assert 'static int hp_bucket_n(int h) { return h <= 4 ? 4 : (h <= 8 ? 8' in nk
    assert 'int s = (d + 3) & ~3; if (((s >> 2) & 1) == 0) s += 4; return s;' in fd
    assert 'constexpr int kMaxGrid = 2048;' in cm
    assert [dlmc_rows_per_wave(d) for d in (2, 196, 197, 396, 397, 512)] == [64, 64, 32, 32, 16, 16]
    assert all(dlmc_rows_per_wave(d) == 64 for d in range(2, 197))
    assert all(dlmc_rows_per_wave(d) == 32 for d in range(197, 397))
    assert all(dlmc_rows_per_wave(d) == 16 for d in range(397, 513))
    assert [hp_bucket(h) for h in range(1, 9)] == [4, 4, 4, 4, 8, 8, 8, 8]
