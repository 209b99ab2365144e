"""CPU-only checks of the C-ABI library: it loads, exports every symbol
include/tfhe_hip.h declares, its parameter selection agrees with the oracle and
the reference table, and its host-side number theory self-tests pass.
No compute call touches a GPU here."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def capi():
    import tfhe_amd

    tfhe_amd.build()
    return tfhe_amd


def test_library_exports_every_header_symbol(capi):
    lib = capi.lib()
    syms = capi.exported_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.tfhe_abi_version() == capi.capi.ABI_VERSION == 8


@pytest.mark.parametrize("name", ["TOY", "MEDIUM", "STD128", "STD128_OPT", "STD192", "STD192_OPT", "STD256",
                                  "STD128Q", "STD128Q_OPT", "STD192Q", "STD256Q", "SIGNED_MOD_TEST"])
def test_params_agree_with_oracle(capi, oracle, name):
    a = capi.params_from_set(name).as_dict()
    b = oracle.params_from_set(name).as_dict()
    for k in a:
        assert a[k] == b[k], (name, k)


@pytest.mark.parametrize("arb,logq,thr", [(True, 12, 1), (True, 12, 0), (False, 23, 1), (False, 11, 0),
                                          (True, 29, 0), (False, 17, 0)])
def test_logq_params_agree_with_oracle(capi, oracle, arb, logq, thr):
    a = capi.params_from_logq("STD128", arb, logq, 0, 0, thr).as_dict()
    b = oracle.params_from_logq("STD128", arb, logq, 0, 0, thr).as_dict()
    for k in a:
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("name", ["TOY", "STD128", "STD192", "STD128Q", "STD256Q"])
def test_host_selftest(capi, name):
    capi.host_selftest(capi.params_from_set(name))


def test_host_selftest_large_q(capi):
    capi.host_selftest(capi.params_from_logq("STD128", True, 12, 0, 0, 1))
    capi.host_selftest(capi.params_from_logq("STD128", False, 23, 0, 0, 1))


def test_errors_without_setup(capi):
    import numpy as np

    lib = capi.lib()
    a = np.zeros(4, dtype=np.uint64)
    st = lib.tfhe_eval_acc(None, 1, a, 1024, a)
    assert st == 3  # TFHE_ERR_NOT_SET_UP
    assert b"not set up" in lib.tfhe_last_error()
    assert lib.tfhe_status_string(2) == b"unsupported"
    bad = capi.params_from_set("STD128")
    bad.Q = 1000  # not prime / not 1 mod 2N
    assert lib.tfhe_params_finish(ctypes.byref(bad)) == 1
    assert lib.tfhe_host_selftest(ctypes.byref(bad)) == 1


def test_params_finish_rejects_zero_lwe_dimension(capi):
    """n = 0 (no blind-rotation round, no key-switch column, empty keys) is an invalid argument with a message,
    for tfhe_params_finish and for whatever finishes the caller's parameters itself; n = 1 is the smallest."""
    lib = capi.lib()
    p = capi.params_from_set("STD128")
    p.n = 0
    assert lib.tfhe_params_finish(ctypes.byref(p)) == 1  # TFHE_ERR_INVALID_ARGUMENT
    assert b"LWE dimension" in lib.tfhe_last_error()
    assert lib.tfhe_host_selftest(ctypes.byref(p)) == 1
    p.n = 1
    assert lib.tfhe_params_finish(ctypes.byref(p)) == 0
    assert (p.n, p.digitsG, p.dG2, p.dKS) == (1, 4, 8, 2)


def test_key_file_rejected_before_device_use(tmp_path):
    """tfhe_setup_from_key_file validates the header (magic, ABI, parameters, size,
    checksum) before any device call, so these checks run without a GPU."""
    import tfhe_amd
    from tfhe_amd import capi

    p = capi.params_from_set("TOY")
    bad = tmp_path / "bad.kimg"
    bad.write_bytes(b"NOTAKEY!" + b"\0" * 200)
    with pytest.raises(capi.TfheError, match="not a key image"):
        tfhe_amd.BinFHEContextHIP.from_key_file(p, str(bad))
    with pytest.raises(capi.TfheError, match="cannot open"):
        tfhe_amd.BinFHEContextHIP.from_key_file(p, str(tmp_path / "missing.kimg"))


def test_binding_rejects_malformed_shapes(capi):
    """The binding hands bare pointers to the C-ABI, so it checks every shape first
    (the reference throws 'input ciphertexts size unmatched', binfhe-base-scheme.cpp:607).
    The checks run before any library call, so an un-set-up context suffices."""
    import numpy as np

    p = capi.params_from_set("TOY")
    ctx = capi.BinFHEContextHIP(p)
    n, N, q = p.n, p.N, p.q
    ct = np.zeros((3, n + 1), dtype=np.uint64)
    with pytest.raises(ValueError, match="size unmatched"):
        ctx.EvalBinGate("NAND", ct, ct[:2])
    with pytest.raises(ValueError, match="expected shape"):
        ctx.EvalBinGate("NAND", ct[:, :n], ct)
    with pytest.raises(ValueError, match="expected shape"):
        ctx.EvalBinGate("NAND", ct, np.zeros((3, n + 2), dtype=np.uint64))
    with pytest.raises(ValueError, match="B\\*2\\*N"):
        ctx.EvalAcc(np.zeros((2, n), dtype=np.uint64), q, np.zeros((1, 2, N), dtype=np.uint64))
    with pytest.raises(ValueError, match="B\\*n"):
        ctx.EvalAcc(np.zeros(n + 1, dtype=np.uint64), q, np.zeros((1, 2, N), dtype=np.uint64))
    with pytest.raises(ValueError, match="LUT"):
        ctx.EvalFunc(ct, np.zeros(q - 1, dtype=np.uint64))
    with pytest.raises(ValueError, match="LUT"):
        ctx.EvalFunc(ct, np.zeros((2, q), dtype=np.uint64))
    with pytest.raises(ValueError, match="expected shape"):
        ctx.MKMSwitch(np.zeros((2, N), dtype=np.uint64), q)
    for fn in (lambda c: ctx.EvalFloor(c, 4 * q), lambda c: ctx.EvalSign(c, 4 * q),
               lambda c: ctx.EvalDecomp(c, 4 * q)):
        with pytest.raises(ValueError, match="expected shape"):
            fn(np.zeros((2, n), dtype=np.uint64))
    with pytest.raises(ValueError, match="expected shape"):
        ctx.CiphertextMulMatrix(np.zeros((2, n), dtype=np.uint64), np.zeros((2, 2), dtype=np.int64), 1 << 20)


def test_key_file_size_field_checked_before_allocation(tmp_path):
    """A header whose size field disagrees with the parameters is refused before the
    library allocates it (a hostile 2^62 must not reach std::vector::resize)."""
    import struct

    import tfhe_amd
    from tfhe_amd import capi

    p = capi.params_from_set("TOY")
    raw = bytes(p)  # tfhe_params as laid out by the C struct
    hdr = b"TFHEKIMG" + struct.pack("<II", capi.ABI_VERSION, 0) + raw + struct.pack("<QQ", 1 << 62, 0)
    f = tmp_path / "huge.kimg"
    f.write_bytes(hdr)
    with pytest.raises(capi.TfheError, match="size field"):
        tfhe_amd.BinFHEContextHIP.from_key_file(p, str(f))


def test_cpp_example_builds_and_links(capi, tmp_path):
    """examples/time_estimate.cpp (the reference's time-estimate.cpp against the C-ABI) compiles
    with the host compiler alone, links to libtfhe_hip.so and runs up to its first device call
    (no operation selected: it prints the ABI version and exits)."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "time_estimate"
    lib_dir = os.path.join(root, "tfhe-gpu_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "time_estimate.cpp"), "-L", lib_dir, "-ltfhe_hip",
                    f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "1", "none"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == f"C-ABI version {capi.capi.ABI_VERSION}"


def test_product_library_has_no_probe_builds(capi):
    """The fault-probe / timing-only builds of k_blind_rotate_f64w exist only in the test library
    (VERDICT r3 weak 7): the product library's symbol table carries the PROBE = 0 instances alone."""
    import re
    import subprocess

    def f64w_instances(path):
        out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
        return sorted(set(re.findall(r"k_blind_rotate_f64w<([^>]*)>", out)))

    def probe(inst):  # <RED, WRAP, LD, PROBE, RESCUE>
        return inst.split(", ")[3]

    prod = f64w_instances(capi.library_path())
    test = f64w_instances(capi.capi.TEST_LIB)
    assert prod and all(probe(i) == "0" for i in prod), prod
    assert set(prod) < set(test) and any(probe(i) != "0" for i in test), test
    assert "true, true, 1, 0, true" in prod  # the rescue form behind f64wduo ships


def test_knob_abi_mirrors_header(capi):
    """tfhe_knobs (include/tfhe_hip.h) and the ctypes mirror list the same fields in the same order."""
    import re

    txt = open(capi.capi.HEADER).read()
    body = re.search(r"typedef struct tfhe_knobs \{(.*?)\} tfhe_knobs;", txt, re.S).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert fields == [k for k, _ in capi.capi.Knobs._fields_]


@pytest.mark.parametrize("env, why", [({"TFHE_KS_CTS": "5"}, "ks_cts"), ({"TFHE_DUO": "-1"}, "duo"),
                                      ({"TFHE_F64W": "off"}, "not a whole number"),
                                      ({"TFHE_GENERIC": "3"}, "generic")])
def test_environment_knobs_are_validated(env, why):
    """A launch knob from the environment is range-checked like tfhe_set_knobs: setup fails
    before any device call, naming the variable."""
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, 'tfhe-gpu_amd'); import numpy as np, tfhe_amd\n"
            "from tfhe_amd import capi\n"
            "p = capi.params_from_set('TOY')\n"
            "try:\n"
            "    tfhe_amd.BinFHEContextHIP(p).GPUSetup(np.zeros(p.bsk_words(), np.uint64), np.zeros(p.ksk_words(), np.uint64))\n"
            "except capi.TfheError as e:\n"
            "    print('ERR', e)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **env))
    assert "ERR" in r.stdout and "launch knob from the environment" in r.stdout and why in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("kernel,product,probes", [("k_blind_rotate_sf2duo", [], ["0"]),
                                                    ("k_blind_rotate_f64wduo", ["0, false, false, 2", "0, true, true, 1"],
                                                     ["0, false, false, 2", "0, true, true, 1", "1, false, false, 2",
                                                      "1, true, true, 1", "2, true, true, 1", "3, true, true, 1",
                                                      "4, true, true, 1"]),
                                                    ("k_blind_rotate_sf2p", ["2, 0"], ["2, 0", "2, 1"]),
                                                    ("k_blind_rotate_sfduo", ["1, 0", "2, 0"],
                                                     ["1, 0", "1, 1", "1, 2", "2, 0", "2, 1", "2, 2"])])
def test_product_library_has_no_duo_probe(capi, kernel, product, probes):
    """The duo probes (1: a partner that never arrives; f64wduo 2: no hand-off, 3: broadcast factor rows,
    4: no D / C' exchange barrier; sf2p<2, 1>: broadcast factor rows; sfduo 2: no hand-off -- all timing only;
    sf2duo: the polynomial-split A/B form of the two-digit duo) are test-library instances only."""
    import re
    import subprocess

    def duo(path):
        out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
        return sorted(set(re.findall(kernel + r"<([\w, ]+)>", out)))

    assert duo(capi.library_path()) == product
    assert duo(capi.capi.TEST_LIB) == probes


def test_arithmetic_probes_exist_in_the_test_library_only(capi):
    """The arithmetic probes (csrc/arith_probes.hpp; tests/test_gpu_arith_units.py) -- one tfhe_test_arith_<family>
    entry point and one k_arith_<family> kernel per family -- are in lib/libtfhe_hip_test.so and not in the
    product library, and include/tfhe_hip.h does not declare them."""
    import re
    import subprocess

    families = {"dm", "kg", "g3", "sf", "f64", "fast4"}

    def names(path):
        dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        sym = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
        return set(re.findall(r"\btfhe_test_arith_(\w+)", dyn)), set(re.findall(r"\bk_arith_([a-z0-9]+)\b", sym))

    entry, kern = names(capi.capi.TEST_LIB)
    assert entry == families and kern >= families, (entry, kern)
    assert names(capi.library_path()) == (set(), set())
    assert not [s for s in capi.exported_symbols() if s.startswith("tfhe_test_")]
