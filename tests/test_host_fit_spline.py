"""The device fit's support predicate and workspace for spline couplings ('c-rqnsf'), answered by the library on the host:
conditioner width <= 8 at d <= 256 is covered, everything beyond keeps the torch loop, and the partial-gradient slabs of
the largest covered shape stay within 64 MiB."""
import ctypes as C

import pytest


def _struct(d, H, n_bins=8, n_coupling=2, n_hl=2):
    from nfmc_amd import hip
    return hip.NfmcRealNVP(d, n_coupling, H, n_hl, 0.001, n_bins, None, None, None, None, None, 0, 5.0, 0)


@pytest.mark.parametrize('d,H,want', [(1, 4, 1), (24, 4, 1), (255, 7, 1), (256, 8, 1), (257, 4, 0), (64, 9, 0), (64, 32, 0)])
def test_fit_supported_for_spline_couplings(d, H, want):
    from nfmc_amd import hip
    st = _struct(d, H)
    assert hip.lib().nfmc_flow_fit_supported_f32(C.byref(st)) == want


def test_affine_support_is_what_it_was():
    from nfmc_amd import hip
    for d, H, want in ((24, 4, 1), (128, 32, 1), (512, 7, 1), (300, 32, 0), (64, 128, 1)):
        assert hip.lib().nfmc_flow_fit_supported_f32(C.byref(_struct(d, H, n_bins=0))) == want, (d, H)


def test_partial_slabs_of_the_largest_spline_shape_stay_within_64_mib():
    from nfmc_amd import hip
    lib = hip.lib()
    d, H = 256, 8
    st = _struct(d, H)
    stride = (int(lib.nfmc_coupling_layer_floats(d, H, 2, 8)) + 3) // 4 * 4
    assert stride == 128 * 8 + 8 + 8 * 8 + 8 + 23 * 128 * 8 + 23 * 128
    n_params = 2 * stride + 4 * d
    nfl = C.c_int64(0)
    assert lib.nfmc_flow_fit_workspace(C.byref(st), 8192, 8192, n_params, C.byref(nfl)) == 0     # no other scratch
    assert 0 < nfl.value * 4 <= 64 << 20
    assert nfl.value % (n_params + 4) == 0 and nfl.value // (n_params + 4) >= 128                # still a wide launch
    # many coupling layers: fewer slabs, never more bytes
    st8 = _struct(d, H, n_coupling=8)
    lib.nfmc_flow_fit_workspace(C.byref(st8), 8192, 8192, 8 * stride + 4 * d, C.byref(nfl))
    assert 0 < nfl.value * 4 <= 64 << 20
    # beyond the kernel: no workspace
    assert lib.nfmc_flow_fit_workspace(C.byref(_struct(300, 6)), 100, 0, 10 ** 5, C.byref(nfl)) == 0 and nfl.value == 0
