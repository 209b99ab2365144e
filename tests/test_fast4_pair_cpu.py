"""CPU-only: the LDS budget of the STD128 blind rotation's two instances (tfhe_fast4_lds_bytes).  The pair
instance (two ciphertexts per wavefront) must fit three workgroups into a CU's 160 KiB; the default instance
keeps the size it had (four per CU).  No call touches a GPU."""
import pytest


@pytest.fixture(scope="module")
def lib():
    import tfhe_amd

    tfhe_amd.build()
    return tfhe_amd.lib()


def test_pair_instance_fits_three_workgroups_per_cu(lib):
    pair = lib.tfhe_fast4_lds_bytes(1)
    # tables (passes 1-3 twiddles both ways, monomials, pass-0 tables: 3360 words), four wavefronts' local regions
    # of 4 polynomials x 304 words, one cross area of 4 x 1152 words; no pass-4 table area
    assert pair == (3360 + 4 * 4 * 304 + 4 * 1152) * 4 == 51328
    assert 3 * pair <= 160 * 1024


def test_default_instance_lds_is_unchanged(lib):
    assert lib.tfhe_fast4_lds_bytes(0) == (4384 + 4 * 2 * 304 + 2 * 1152) * 4 == 36480
    assert 4 * lib.tfhe_fast4_lds_bytes(0) <= 160 * 1024


def test_pair_min_needs_a_context(lib):
    import ctypes

    v = ctypes.c_int32(-5)
    assert lib.tfhe_get_pair_min(None, ctypes.byref(v), None) != 0 and v.value == -5
    assert lib.tfhe_set_pair_min(None, 4) != 0
