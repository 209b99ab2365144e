"""Key generation / Encrypt / Decrypt entry points without a GPU: they are exported, bound, and every argument
error is TFHE_ERR_INVALID_ARGUMENT with a message, reported before any device call (so these pass on a machine
that has no GPU, where the first device call would be TFHE_ERR_DEVICE)."""
import ctypes as C

import pytest

import tfhe_amd
from tfhe_amd import capi

NEW = ["tfhe_keygen_device", "tfhe_setup_keygen", "tfhe_encrypt_device", "tfhe_decrypt_device", "tfhe_encrypt",
       "tfhe_decrypt"]
INVALID = 1  # TFHE_ERR_INVALID_ARGUMENT


def test_exported_and_bound():
    syms = tfhe_amd.exported_symbols()
    L = tfhe_amd.lib()
    for name in NEW:
        assert name in syms, name
        assert name in capi._SIGS, name
        assert getattr(L, name).argtypes == capi._SIGS[name][0]
    assert L.tfhe_abi_version() == capi.ABI_VERSION == 8  # new symbols only


def test_python_names():
    for name in ("from_keygen", "Encrypt", "Decrypt", "EncryptDevice", "DecryptDevice"):
        assert callable(getattr(tfhe_amd.BinFHEContextHIP, name)), name
    assert callable(tfhe_amd.keygen) and "keygen" in tfhe_amd.__all__


@pytest.fixture(scope="module")
def raw():
    """The library through a handle of its own, without the binding's argtypes: null pointers can be passed."""
    tfhe_amd.lib()
    L = C.CDLL(capi.library_path())
    L.tfhe_last_error.restype = C.c_char_p
    return L


def good_params():
    return tfhe_amd.params_from_set("TOY")


def bad_params():
    p = good_params()
    p.N = 500  # not a power of two: tfhe_params_finish rejects it
    return p


# A non-null value for every pointer: no call below may reach the point where it would be dereferenced.
BUF = (C.c_uint64 * 128)()
PTR = C.cast(BUF, C.c_void_p)
NULL = C.c_void_p(None)
u64, sz, i32 = C.c_uint64, C.c_size_t, C.c_int


def lwe_args(kind, p, sk=PTR, B=1, src=PTR, ptxt=4, mod=512, dst=PTR):
    """argument list of tfhe_encrypt(_device) / tfhe_decrypt(_device)"""
    head = [C.byref(p) if p is not None else NULL, i32(0), sk, sz(B), src, u64(ptxt), u64(mod)]
    if kind == "enc":
        return head + [u64(1), dst, NULL, NULL]  # seed, ct, seed_after (optional), stream
    return head + [dst, NULL]


LWE_FNS = [("tfhe_encrypt", "enc"), ("tfhe_encrypt_device", "enc"), ("tfhe_decrypt", "dec"), ("tfhe_decrypt_device", "dec")]
LWE_CASES = {
    "null params": dict(p=None),
    "rejected params": dict(p="bad"),
    "null sk": dict(sk=NULL),
    "null input": dict(src=NULL),
    "null output": dict(dst=NULL),
    "B = 0": dict(B=0),
    "mod = 0": dict(mod=0),
    "ptxt_mod = 0": dict(ptxt=0),
    "ptxt_mod > mod": dict(ptxt=1024, mod=512),
}


@pytest.mark.parametrize("fn,kind", LWE_FNS)
@pytest.mark.parametrize("case", list(LWE_CASES))
def test_lwe_argument_errors(raw, fn, kind, case):
    kw = dict(LWE_CASES[case])
    p = kw.pop("p", "good")
    p = {"good": good_params(), "bad": bad_params(), None: None}[p]
    assert getattr(raw, fn)(*lwe_args(kind, p, **kw)) == INVALID, case
    assert raw.tfhe_last_error(), case


KEYGEN_CASES = {
    "null params": lambda p: [NULL, u64(7), i32(0), PTR, NULL, NULL, NULL, NULL],
    "rejected params": lambda p: [C.byref(bad_params()), u64(7), i32(0), PTR, NULL, NULL, NULL, NULL],
    "null sk": lambda p: [C.byref(p), u64(7), i32(0), NULL, PTR, PTR, NULL, NULL],
}


@pytest.mark.parametrize("case", list(KEYGEN_CASES))
def test_keygen_device_argument_errors(raw, case):
    assert raw.tfhe_keygen_device(*KEYGEN_CASES[case](good_params())) == INVALID
    assert raw.tfhe_last_error()


def test_setup_keygen_argument_errors(raw):
    p, h = good_params(), C.c_void_p()
    cases = {
        "null out": [NULL, C.byref(p), u64(7), i32(1), PTR, NULL],
        "null sk_out": [C.byref(h), C.byref(p), u64(7), i32(1), NULL, NULL],
        "null params": [C.byref(h), NULL, u64(7), i32(1), PTR, NULL],
        "rejected params": [C.byref(h), C.byref(bad_params()), u64(7), i32(1), PTR, NULL],
    }
    for case, args in cases.items():
        assert raw.tfhe_setup_keygen(*args) == INVALID, case
        assert raw.tfhe_last_error(), case
        assert not h.value


def test_python_wrappers_check_shapes():
    cc = tfhe_amd.BinFHEContextHIP(good_params())
    with pytest.raises(ValueError):
        cc.Encrypt([0] * 3, [1])  # sk is not n words
    with pytest.raises(ValueError):
        cc.Encrypt([0] * 64, [])
    with pytest.raises(tfhe_amd.TfheError) as e:
        cc.Encrypt([0] * 64, [1], p=0)
    assert e.value.status == INVALID
