"""ctypes declarations of include/tfhe_hip.h."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tfhe-gpu_amd/
_ROOT = os.path.dirname(_PKG)
_LIB = os.environ.get("TFHE_LIB", os.path.join(_PKG, "lib", "libtfhe_hip.so"))  # override: alternative builds
HEADER = os.path.join(_ROOT, "include", "tfhe_hip.h")
ABI_VERSION = 8  # TFHE_HIP_ABI_VERSION of include/tfhe_hip.h (3: tfhe_info.replicate_*; 4: row-pointer host arrays;
                 # 5: device-resident EvalFunc / EvalFloor / EvalSign; 6: knobs.duo, info.duo_timeouts;
                 # 7: knobs.split4; 8: knobs.ks40, tfhe_rccl_selftest)

# BINFHE_PARAMSET / BINGATE (binfhe-constants.h:46-101)
PARAMSETS = {"TOY": 0, "MEDIUM": 1, "STD128_AP": 2, "STD128_APOPT": 3, "STD128": 4, "STD128_OPT": 5, "STD192": 6,
             "STD192_OPT": 7, "STD256": 8, "STD256_OPT": 9, "STD128Q": 10, "STD128Q_OPT": 11, "STD192Q": 12,
             "STD192Q_OPT": 13, "STD256Q": 14, "STD256Q_OPT": 15, "SIGNED_MOD_TEST": 16}
BINGATE = {"OR": 0, "AND": 1, "NOR": 2, "NAND": 3, "XOR_FAST": 4, "XNOR_FAST": 5, "XOR": 6, "XNOR": 7}
CIRCUIT_OPS = dict(BINGATE, NOT=8, CONST0=9, CONST1=10)  # tfhe_gate + tfhe_circuit_op
FCIRCUIT_OPS = {"LIN": 0, "LUT": 1}  # tfhe_fcircuit_op


class TfheError(RuntimeError):
    def __init__(self, status: int, where: str, msg: str):
        super().__init__(f"{where}: status {status}: {msg}")
        self.status = status


class Params(C.Structure):
    _fields_ = [("n", C.c_uint32), ("N", C.c_uint32), ("q", C.c_uint64), ("Q", C.c_uint64), ("qKS", C.c_uint64),
                ("baseKS", C.c_uint32), ("baseG", C.c_uint32), ("numDigitsToThrow", C.c_uint32),
                ("digitsG", C.c_uint32), ("dKS", C.c_uint32), ("dG2", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def bsk_words(self):
        return self.n * 2 * self.dG2 * 2 * self.N

    def ksk_words(self):
        return self.N * self.baseKS * self.dKS * (self.n + 1)


class Info(C.Structure):
    _fields_ = [("num_devices", C.c_int), ("word_bits", C.c_int), ("bsk_device_bytes", C.c_uint64),
                ("ksk_device_bytes", C.c_uint64), ("bootstraps", C.c_uint64), ("key_image_bytes", C.c_uint64),
                ("br_kernel", C.c_int), ("replicate_method", C.c_int), ("replicate_ms", C.c_double),
                ("duo_timeouts", C.c_uint32)]


class Knobs(C.Structure):
    """tfhe_knobs: launch choices of a context (include/tfhe_hip.h), environment at setup, then tfhe_set_knobs."""
    _fields_ = [(k, C.c_int32) for k in ("ks_tiled_min", "ks_cts", "ks_split", "ks_pk", "host_parts", "wire",
                                         "acc_flags", "f64w", "sf2", "generic", "trace", "probe", "duo",
                                         "sf2p", "split4", "ks40")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CircuitGate(C.Structure):
    _fields_ = [("op", C.c_uint32), ("in0", C.c_uint32), ("in1", C.c_uint32)]


class CircuitInfo(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("num_inputs", "num_outputs", "num_gates", "bootstraps", "levels",
                                          "widest_level")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FuncNode(C.Structure):
    _fields_ = [("op", C.c_uint32), ("in0", C.c_uint32), ("in1", C.c_uint32), ("c0", C.c_int32), ("c1", C.c_int32),
                ("lut", C.c_uint32), ("k", C.c_uint64)]


class FuncCircuitInfo(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("num_inputs", "num_outputs", "num_nodes", "bootstraps", "levels",
                                          "widest_level", "num_luts", "negacyclic", "periodic", "arbitrary")] + \
               [("q", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Conv2d(C.Structure):
    """tfhe_conv2d: the geometry of a convolution (include/tfhe_hip.h)."""
    _fields_ = [(k, C.c_uint32) for k in ("c_in", "h", "w", "c_out", "kh", "kw", "stride_h", "stride_w", "pad_h",
                                          "pad_w", "groups")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Pool2d(C.Structure):
    """tfhe_pool2d: the geometry of a pooling window (include/tfhe_hip.h)."""
    _fields_ = [(k, C.c_uint32) for k in ("c", "h", "w", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CtMatMul(C.Structure):
    """tfhe_ct_matmul: the shape of a product of two encrypted tensors (include/tfhe_hip.h)."""
    _fields_ = [(k, C.c_uint32) for k in ("rows", "inner", "cols", "y_transposed", "y_shared")]

    def __init__(self, rows=0, inner=0, cols=0, y_transposed=0, y_shared=0):
        super().__init__(rows, inner, cols, int(y_transposed), int(y_shared))

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def y_shape(self, instances: int) -> tuple:
        """The shape of y without the n+1 axis."""
        kc = (self.cols, self.inner) if self.y_transposed else (self.inner, self.cols)
        return kc if self.y_shared else (instances,) + kc


u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
VP = C.c_void_p
SZ = C.c_size_t
U64 = C.c_uint64
P = C.POINTER(Params)

_SIGS = {
    "tfhe_abi_version": ([], C.c_int),
    "tfhe_set_kernel_variant": ([C.c_int], C.c_int),
    "tfhe_get_kernel_variant": ([], C.c_int),
    "tfhe_last_error": ([], C.c_char_p),
    "tfhe_status_string": ([C.c_int], C.c_char_p),
    "tfhe_params_from_set": ([C.c_int, P], C.c_int),
    "tfhe_params_from_logq": ([C.c_int, C.c_int, C.c_uint32, C.c_int64, C.c_uint32, C.c_uint32, P], C.c_int),
    "tfhe_params_finish": ([P], C.c_int),
    "tfhe_setup": ([C.POINTER(VP), P, u64p, u64p, C.c_int], C.c_int),
    "tfhe_setup_eval": ([C.POINTER(VP), P, u64p, u64p, C.c_int], C.c_int),
    "tfhe_clean": ([VP], C.c_int),
    "tfhe_eval_acc": ([VP, SZ, u64p, U64, u64p], C.c_int),
    "tfhe_shard_range": ([SZ, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
    "tfhe_host_shard_selftest": ([SZ, C.c_int, C.c_int, C.POINTER(C.c_size_t)], C.c_int),
    "tfhe_rccl_selftest": ([C.c_int, SZ, C.c_char_p, C.POINTER(C.c_int)], C.c_int),
    "tfhe_eval_acc_tv": ([VP, SZ, u64p, U64, u64p, C.c_uint32, u64p], C.c_int),
    "tfhe_mkm_switch": ([VP, SZ, u64p, U64, u64p], C.c_int),
    "tfhe_eval_acc_tv_rows": ([VP, SZ, VP, U64, u64p, C.c_uint32, VP], C.c_int),
    "tfhe_mkm_switch_rows": ([VP, SZ, VP, VP, U64, VP, VP], C.c_int),
    "tfhe_ciphertext_mul_matrix": ([VP, SZ, u64p, SZ, i64p, U64, u64p], C.c_int),
    "tfhe_lwe_gpu_setup": ([C.c_int], C.c_int),
    "tfhe_lwe_gpu_clean": ([], C.c_int),
    "tfhe_eval_bin_gate": ([VP, C.c_int, SZ, u64p, u64p, U64, u64p], C.c_int),
    "tfhe_eval_func": ([VP, SZ, u64p, U64, u64p, C.c_int, u64p], C.c_int),
    "tfhe_eval_floor": ([VP, SZ, u64p, U64, C.c_uint32, u64p], C.c_int),
    "tfhe_eval_sign": ([VP, SZ, u64p, U64, u64p], C.c_int),
    "tfhe_eval_decomp": ([VP, SZ, u64p, U64, C.c_uint32, u64p, u64p, C.POINTER(C.c_uint32)], C.c_int),
    "tfhe_eval_bin_gate_device": ([VP, C.c_int, SZ, VP, VP, U64, VP, VP], C.c_int),
    "tfhe_eval_acc_device": ([VP, SZ, VP, U64, VP, VP], C.c_int),
    "tfhe_mkm_switch_device": ([VP, SZ, VP, U64, VP, VP], C.c_int),
    "tfhe_eval_func_device": ([VP, SZ, VP, U64, VP, C.c_int, VP, VP], C.c_int),
    "tfhe_eval_floor_device": ([VP, SZ, VP, U64, C.c_uint32, VP, VP], C.c_int),
    "tfhe_eval_sign_device": ([VP, SZ, VP, U64, VP, VP], C.c_int),
    "tfhe_circuit_compile": ([C.POINTER(VP), C.c_uint32, VP, SZ, VP, SZ], C.c_int),
    "tfhe_circuit_free": ([VP], C.c_int),
    "tfhe_circuit_get_info": ([VP, C.POINTER(CircuitInfo)], C.c_int),
    "tfhe_circuit_level_widths": ([VP, VP, SZ], C.c_int),
    "tfhe_circuit_eval_plain": ([VP, SZ, VP, VP], C.c_int),
    "tfhe_eval_circuit_device": ([VP, VP, SZ, VP, U64, VP, VP], C.c_int),
    "tfhe_eval_circuit": ([VP, VP, SZ, u64p, U64, u64p], C.c_int),
    "tfhe_fcircuit_compile": ([C.POINTER(VP), C.c_uint32, VP, SZ, U64, VP, SZ, VP, SZ], C.c_int),
    "tfhe_fcircuit_free": ([VP], C.c_int),
    "tfhe_fcircuit_get_info": ([VP, C.POINTER(FuncCircuitInfo)], C.c_int),
    "tfhe_fcircuit_level_widths": ([VP, VP, SZ], C.c_int),
    "tfhe_fcircuit_eval_plain": ([VP, SZ, VP, VP], C.c_int),
    "tfhe_eval_fcircuit_device": ([VP, VP, SZ, VP, VP, VP], C.c_int),
    "tfhe_eval_fcircuit": ([VP, VP, SZ, u64p, u64p], C.c_int),
    "tfhe_ciphertext_mul_matrix_device": ([VP, SZ, SZ, VP, SZ, VP, VP, U64, VP, VP], C.c_int),
    "tfhe_eval_dense_device": ([VP, SZ, SZ, VP, SZ, VP, VP, U64, VP, VP, VP], C.c_int),
    "tfhe_eval_dense": ([VP, SZ, SZ, u64p, SZ, i64p, VP, U64, u64p, u64p], C.c_int),
    "tfhe_mm_tiles": ([C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], None),
    "tfhe_conv2d_shape": ([VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(SZ)], C.c_int),
    "tfhe_ciphertext_conv2d_device": ([VP, VP, SZ, VP, VP, VP, U64, VP, VP], C.c_int),
    "tfhe_eval_conv2d_device": ([VP, VP, SZ, VP, VP, VP, U64, VP, VP, VP], C.c_int),
    "tfhe_eval_conv2d": ([VP, VP, SZ, u64p, i64p, VP, U64, u64p, u64p], C.c_int),
    "tfhe_conv2d_tiles": ([C.POINTER(C.c_int)] * 4, None),
    "tfhe_pool2d_shape": ([VP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(SZ)], C.c_int),
    "tfhe_pool2d_eval_plain": ([VP, SZ, U64, VP, VP, VP], C.c_int),
    "tfhe_eval_pool2d_device": ([VP, VP, SZ, VP, U64, VP, VP, VP], C.c_int),
    "tfhe_eval_pool2d": ([VP, VP, SZ, u64p, U64, u64p, u64p], C.c_int),
    "tfhe_lut_tables_info": ([U64, VP, SZ, SZ, SZ, VP, C.POINTER(SZ), C.POINTER(U64)], C.c_int),
    "tfhe_eval_func_tables_device": ([VP, SZ, VP, U64, VP, SZ, SZ, VP, VP], C.c_int),
    "tfhe_eval_func_tables": ([VP, SZ, u64p, U64, u64p, SZ, SZ, u64p], C.c_int),
    "tfhe_eval_dense_tables_device": ([VP, SZ, SZ, VP, SZ, VP, VP, U64, VP, SZ, VP, VP], C.c_int),
    "tfhe_eval_dense_tables": ([VP, SZ, SZ, u64p, SZ, i64p, VP, U64, u64p, SZ, u64p], C.c_int),
    "tfhe_eval_conv2d_tables_device": ([VP, VP, SZ, VP, VP, VP, U64, VP, SZ, VP, VP], C.c_int),
    "tfhe_eval_conv2d_tables": ([VP, VP, SZ, u64p, i64p, VP, U64, u64p, SZ, u64p], C.c_int),
    "tfhe_eval_pool2d_tables_device": ([VP, VP, SZ, VP, U64, VP, SZ, VP, VP], C.c_int),
    "tfhe_eval_pool2d_tables": ([VP, VP, SZ, u64p, U64, u64p, SZ, u64p], C.c_int),
    "tfhe_ct_matmul_info": ([VP, SZ, U64, VP, C.POINTER(SZ), C.POINTER(U64)], C.c_int),
    "tfhe_ct_matmul_eval_plain": ([VP, SZ, U64, VP, VP, VP, VP], C.c_int),
    "tfhe_eval_ct_matmul_device": ([VP, VP, SZ, VP, VP, U64, VP, VP, VP], C.c_int),
    "tfhe_eval_ct_matmul": ([VP, VP, SZ, u64p, u64p, U64, u64p, u64p], C.c_int),
    "tfhe_keygen_device": ([P, U64, C.c_int, VP, VP, VP, C.POINTER(U64), VP], C.c_int),
    "tfhe_setup_keygen": ([C.POINTER(VP), P, U64, C.c_int, u64p, C.POINTER(U64)], C.c_int),
    "tfhe_encrypt_device": ([P, C.c_int, VP, SZ, VP, U64, U64, U64, VP, C.POINTER(U64), VP], C.c_int),
    "tfhe_decrypt_device": ([P, C.c_int, VP, SZ, VP, U64, U64, VP, VP], C.c_int),
    "tfhe_encrypt": ([P, C.c_int, u64p, SZ, i64p, U64, U64, U64, u64p, C.POINTER(U64), VP], C.c_int),
    "tfhe_decrypt": ([P, C.c_int, u64p, SZ, u64p, U64, U64, i64p, VP], C.c_int),
    "tfhe_export_key_image": ([VP, VP, SZ, VP], C.c_int),
    "tfhe_setup_from_key_image": ([C.POINTER(VP), P, VP, SZ, C.c_int], C.c_int),
    "tfhe_save_key_image": ([VP, C.c_char_p], C.c_int),
    "tfhe_setup_from_key_file": ([C.POINTER(VP), P, C.c_char_p, C.c_int], C.c_int),
    "tfhe_get_info": ([VP, C.POINTER(Info)], C.c_int),
    "tfhe_host_selftest": ([P], C.c_int),
    "tfhe_get_knobs": ([VP, C.POINTER(Knobs)], C.c_int),
    "tfhe_set_knobs": ([VP, C.POINTER(Knobs)], C.c_int),
    "tfhe_get_pair_min": ([VP, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)], C.c_int),
    "tfhe_set_pair_min": ([VP, C.c_int32], C.c_int),
    "tfhe_fast4_lds_bytes": ([C.c_int], SZ),
}


def library_path() -> str:
    return _LIB


def build(jobs: int = 8) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", _PKG, f"-j{jobs}"], check=True)
    return _LIB


def exported_symbols() -> list[str]:
    """Function names declared in include/tfhe_hip.h."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(tfhe_[a-z0-9_]+)\s*\(", txt)))


TEST_LIB = os.path.join(_PKG, "lib", "libtfhe_hip_test.so")  # + fault-probe / timing builds (tests only)
_libs = {}


def lib(path: str | None = None):
    """The product library (or `path`, e.g. TEST_LIB), loaded once per path."""
    path = path or _LIB
    L = _libs.get(path)
    if L is None:
        if not os.path.exists(path):
            raise TfheError(-1, "load", f"{path} missing: run tfhe_amd.build() (make -C tfhe-gpu_amd)")
        # One HIP runtime per process: torch wheels bundle libamdhip64/libhsa-runtime64
        # with the same sonames as /opt/rocm's but are NEEDED under unversioned names,
        # so loading ours first would put two HSA runtimes on one GPU and torch would
        # then see no devices.  Loading torch first makes ours bind to its runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name, None)  # an older build (TFHE_LIB A/B runs) may lack a newer entry point
            if fn is None:
                continue
            fn.argtypes = args
            fn.restype = res
        # the structs above mirror this ABI version.  A/B runs against the previous round's build
        # (tools/ab_lib.sh) may set TFHE_ABI_PREV=1 to admit ABI 6: its tfhe_knobs / tfhe_info are
        # prefixes of these, so reads and writes stay in bounds
        abi = L.tfhe_abi_version()
        if abi != ABI_VERSION and not (6 <= abi < ABI_VERSION and os.environ.get("TFHE_ABI_PREV") == "1"):
            raise TfheError(-1, "load", f"{path} has ABI {L.tfhe_abi_version()}, binding expects {ABI_VERSION}: "
                                        "rebuild (make -C tfhe-gpu_amd)")
        _libs[path] = L
    return L


def check(status: int, where: str, L=None):
    if status != 0:
        msg = (L or lib()).tfhe_last_error().decode(errors="replace")
        raise TfheError(status, where, msg)


def params_from_set(name: str) -> Params:
    p = Params()
    check(lib().tfhe_params_from_set(PARAMSETS[name], C.byref(p)), "tfhe_params_from_set")
    return p


def params_from_logq(name: str, arb_func: bool, logQ: int, N: int = 0, baseG: int = 0, throw: int = 0) -> Params:
    """GenerateBinFHEContext(set, arbFunc, logQ, N, GINX, false, baseG, numDigitsToThrow)."""
    p = Params()
    check(lib().tfhe_params_from_logq(PARAMSETS[name], int(arb_func), logQ, N, baseG, throw, C.byref(p)),
          "tfhe_params_from_logq")
    return p


def mm_tiles() -> tuple[int, int, int]:
    """(K-tile, column tile, threads per workgroup) of the matrix-product kernel (tfhe_mm_tiles)."""
    kt, ct, th = C.c_int(), C.c_int(), C.c_int()
    lib().tfhe_mm_tiles(C.byref(kt), C.byref(ct), C.byref(th))
    return kt.value, ct.value, th.value


def conv2d_tiles() -> tuple[int, int, int, int]:
    """(K-tile, output-plane tile, threads per workgroup, output positions per workgroup) of the convolution kernel
    (tfhe_conv2d_tiles)."""
    v = [C.c_int() for _ in range(4)]
    lib().tfhe_conv2d_tiles(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def conv2d_shape(desc: Conv2d) -> tuple[int, int, int]:
    """(oh, ow, K = (c_in / groups) kh kw) of a convolution; validates the descriptor (tfhe_conv2d_shape; no GPU)."""
    oh, ow, K = C.c_uint32(), C.c_uint32(), SZ()
    check(lib().tfhe_conv2d_shape(C.byref(desc), C.byref(oh), C.byref(ow), C.byref(K)), "tfhe_conv2d_shape")
    return oh.value, ow.value, K.value


def pool2d_shape(desc: Pool2d) -> tuple[int, int, int, int]:
    """(oh, ow, rounds of the longest tournament, pairs per plane) of a pooling window; validates the descriptor
    (tfhe_pool2d_shape; no GPU)."""
    oh, ow, rounds, pairs = C.c_uint32(), C.c_uint32(), C.c_uint32(), SZ()
    check(lib().tfhe_pool2d_shape(C.byref(desc), C.byref(oh), C.byref(ow), C.byref(rounds), C.byref(pairs)),
          "tfhe_pool2d_shape")
    return oh.value, ow.value, rounds.value, pairs.value


def pool2d_eval_plain(desc: Pool2d, values, lut, q: int):
    """The pooling tournament on clear values mod q: values[instances, c, h, w] (or [c, h, w]) and lut[q] ->
    [instances, c, oh, ow], op(a, b) = b + lut[a - b mod q] mod q (tfhe_pool2d_eval_plain; no GPU)."""
    x = np.ascontiguousarray(values, dtype=np.uint64)
    one = x.ndim == 3
    if one:
        x = x[None]
    if x.ndim != 4 or x.shape[1:] != (desc.c, desc.h, desc.w):
        raise ValueError(f"pool2d_eval_plain: expected shape (instances, {desc.c}, {desc.h}, {desc.w}), got {x.shape}")
    lut = np.ascontiguousarray(lut, dtype=np.uint64)
    if lut.shape != (q,):
        raise ValueError(f"pool2d_eval_plain: LUT must have shape ({q},), got {lut.shape}")
    oh, ow, _, _ = pool2d_shape(desc)
    x = np.ascontiguousarray(x)
    out = np.empty((x.shape[0], desc.c, oh, ow), dtype=np.uint64)
    check(lib().tfhe_pool2d_eval_plain(C.byref(desc), x.shape[0], q, C.c_void_p(lut.ctypes.data),
                                       C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data)),
          "tfhe_pool2d_eval_plain")
    return out[0] if one else out


def lut_tables_info(luts, q: int, inner: int = 1, B: int = 1):
    """(classes[T], per_class[3], bootstraps) of a batch of B ciphertexts under luts[T, q] and `inner`: ciphertext i
    uses table (i // inner) % T; class 0 negacyclic, 1 periodic, 2 arbitrary, each table classified on its own
    (tfhe_lut_tables_info; no GPU)."""
    t = np.ascontiguousarray(luts, dtype=np.uint64)
    if t.ndim != 2 or t.shape[1] != q:
        raise ValueError(f"lut_tables_info: tables must have shape (T, {q}), got {t.shape}")
    classes = np.zeros(t.shape[0], dtype=np.uint8)
    per = (SZ * 3)()
    boots = U64()
    check(lib().tfhe_lut_tables_info(q, C.c_void_p(t.ctypes.data), t.shape[0], inner, B,
                                     C.c_void_p(classes.ctypes.data), per, C.byref(boots)), "tfhe_lut_tables_info")
    return classes, (per[0], per[1], per[2]), boots.value


def lut_classes(luts, q: int):
    """The class of each table of luts[T, q] (0 negacyclic, 1 periodic, 2 arbitrary), as EvalFuncTables and the
    layers with one table per channel classify them (no GPU)."""
    return lut_tables_info(luts, q)[0]


def max_table(q: int, negacyclic: bool = False):
    """The table that makes the pooling step op(a, b) = b + EvalFunc(a - b) a maximum: ReLU of the signed difference.

    Default (arbitrary class, two bootstraps per pair): lut[x] = x for x < q/2, else 0; exact for differences in
    (-q/2, q/2).

    negacyclic=True (one bootstrap per pair), for inputs whose differences stay inside (-q/4, q/4), one more bit of
    headroom: lut[x] = x on [0, q/4), 0 on [q/4, q/2), and the upper half mirrored, lut[x + q/2] = q - lut[x].
    checkInputFunction compares lut[i] with q - lut[i + q/2], so a zero entry can never pass as negacyclic: the
    helper writes 1 for those zeros (lut[0] and [q/4, q/2)) and q - 1 for their mirrors.  A pair step then returns
    max(a, b) + 1 where a = b, max(a, b) - 1 where a < b and max(a, b) where a > b: one unit of the noise bits.

    On ciphertexts EvalFunc looks a table up at phase + beta (beta = 128), so under either table a pair step whose
    first operand wins or ties returns it beta higher: choose p with q / 2p above 128 per round plus the noise
    (DESIGN 3.11)."""
    if q < 8 or q & (q - 1):
        raise ValueError(f"max_table: q must be a power of two >= 8, got {q}")
    x = np.arange(q, dtype=np.uint64)
    if not negacyclic:
        return np.where(x < q // 2, x, 0).astype(np.uint64)
    half = np.where(x[:q // 2] < q // 4, x[:q // 2], 0)
    half[half == 0] = 1
    return np.concatenate([half, q - half]).astype(np.uint64)


def _pair_tables(who: str, luts, q: int):
    t = np.ascontiguousarray(luts, dtype=np.uint64)
    if t.shape != (2, q):
        raise ValueError(f"{who}: tables must have shape (2, {q}), got {t.shape}")
    return t


def ct_matmul_info(desc: CtMatMul, instances: int, luts, q: int) -> tuple[int, int]:
    """(products P = instances rows inner cols, bootstraps the call adds: P (b0 + b1), b = 1 for a negacyclic table
    and 2 otherwise) of a product of two encrypted tensors under luts[2, q] (tfhe_ct_matmul_info; no GPU)."""
    t = _pair_tables("ct_matmul_info", luts, q)
    products, boots = SZ(), U64()
    check(lib().tfhe_ct_matmul_info(C.byref(desc), instances, q, C.c_void_p(t.ctypes.data), C.byref(products),
                                    C.byref(boots)), "tfhe_ct_matmul_info")
    return products.value, boots.value


def ct_matmul_eval_plain(desc: CtMatMul, x, y, luts, q: int):
    """The pair form on clear values mod q: x[instances, rows, inner], y[instances, inner, cols] ([inner, cols] when
    desc.y_shared; the last two axes swapped when desc.y_transposed) and luts[2, q] -> [instances, rows, cols],
    out = sum_k luts[0][x + y mod q] - luts[1][x - y mod q] mod q (tfhe_ct_matmul_eval_plain; no GPU)."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    y = np.ascontiguousarray(y, dtype=np.uint64)
    if x.ndim != 3 or x.shape[1:] != (desc.rows, desc.inner):
        raise ValueError(f"ct_matmul_eval_plain: x: expected shape (instances, {desc.rows}, {desc.inner}), got {x.shape}")
    if y.shape != desc.y_shape(x.shape[0]):
        raise ValueError(f"ct_matmul_eval_plain: y: expected shape {desc.y_shape(x.shape[0])}, got {y.shape}")
    t = _pair_tables("ct_matmul_eval_plain", luts, q)
    out = np.empty((x.shape[0], desc.rows, desc.cols), dtype=np.uint64)
    check(lib().tfhe_ct_matmul_eval_plain(C.byref(desc), x.shape[0], q, C.c_void_p(t.ctypes.data),
                                          C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data),
                                          C.c_void_p(out.ctypes.data)), "tfhe_ct_matmul_eval_plain")
    return out


def product_tables(q: int, p: int, negacyclic: bool = False):
    """The two tables [2, q] (both rows equal) that make EvalCtMatMul / EvalCtMul a product of messages mod p, by the
    quarter-square identity x y = floor((x + y)^2 / 4) - floor((x - y)^2 / 4): with Delta = q / p and s the signed
    message of a step, the staircase Delta (floor(s^2 / 4) mod p).

    Default (arbitrary class, needs q <= N, 4 bootstraps per product): s in [-p/2, p/2).  Exact for messages with
    |x| + |y| <= p/2 -- the wrap at +-p/2 has the same square -- so messages in [0, p/4] or signed ones in
    [-p/4, p/4].

    negacyclic=True (2 bootstraps per product), for |x| + |y| < p/4, one more bit of headroom: on [0, q/4) the
    squares of s = 0 ... p/4 - 1, on [q/4, q/2) q minus the squares of s = h - p/2, and the upper half mirrored,
    lut[v + q/2] = q - lut[v], which gives negative s their positive square.  checkInputFunction compares lut[i]
    with q - lut[i + q/2], so a zero entry can never pass as negacyclic: the helper writes 1 for those zeros and
    q - 1 for their mirrors, as max_table does.  A product is then off by at most 2 units of the noise bits.

    On ciphertexts EvalFunc looks a table up at phase + beta (beta = 128).  The helper centres every step on that: it
    returns the staircase rotated by beta - Delta/2 places, so the look-up rounds at half a step, phase in
    [Delta s - Delta/2, Delta s + Delta/2) reads step s, for every Delta.  On clear values (ct_matmul_eval_plain)
    read the tables the same way, at Delta s + beta.  An output sums 2 inner bootstrap outputs: choose p with
    Delta/2 above their summed noise."""
    beta = 128
    if q < 8 or q & (q - 1):
        raise ValueError(f"product_tables: q must be a power of two >= 8, got {q}")
    if p < 4 or p & (p - 1) or 2 * p > q:
        raise ValueError(f"product_tables: p must be a power of two with 4 <= p <= q/2 = {q // 2}, got {p}")
    delta = q // p
    if not negacyclic:
        j = np.arange(q, dtype=np.int64) // delta
        s = np.where(j < p // 2, j, j - p)
        stairs = delta * ((s * s // 4) % p)
    else:
        h = np.arange(q // 2, dtype=np.int64) // delta
        s = np.where(h < p // 4, h, h - p // 2)
        sq = delta * ((s * s // 4) % p)
        half = np.where(h < p // 4, sq, (q - sq) % q)
        half[half == 0] = 1
        stairs = np.concatenate([half, q - half])
    lut = np.roll(stairs, beta - delta // 2).astype(np.uint64)
    return np.stack([lut, lut])


def host_selftest(p: Params):
    check(lib().tfhe_host_selftest(C.byref(p)), "tfhe_host_selftest")
