"""BinFHEContextHIP: the vector BinFHEContext surface (binfhecontext.cpp:316-365)
over the C-ABI.  Ciphertexts are numpy uint64 arrays of shape [B, n+1]
(a[0..n-1], b), keys are flat coefficient-form arrays (see include/tfhe_hip.h)."""
from __future__ import annotations

import ctypes as C
import os
from contextlib import contextmanager

import numpy as np

from .capi import (BINGATE, Conv2d, CtMatMul, Info, Knobs, Params, Pool2d, TfheError, check, conv2d_shape, lib, max_table,
                   pool2d_shape)


_M64 = (1 << 64) - 1


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _rows(x, width: int, what: str):
    """[B][width] view of a ciphertext batch (a single ciphertext becomes B = 1); the
    C-ABI takes bare pointers, so every shape is checked here before a call."""
    x = _u64(x)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2 or x.shape[1] != width:
        raise ValueError(f"{what}: expected shape (B, {width}), got {x.shape}")
    return x


def keygen(params: Params, seed: int, device: int = 0, want_bsk: bool = True, want_ksk: bool = True):
    """(sk, bsk_coeff, ksk): the keys of stream `seed` in the oracle's layouts (include/tfhe_hip.h), generated on
    `device` (tfhe_keygen_device) and copied to numpy arrays; a key that is not wanted is None.  keygen.seed_after
    holds the stream state behind the last call."""
    import torch

    dev = torch.device("cuda", device)

    def buf(words):
        return torch.empty(words, dtype=torch.int64, device=dev)

    d_sk = buf(params.n)
    d_bsk = buf(params.bsk_words()) if want_bsk else None
    d_ksk = buf(params.ksk_words()) if want_ksk else None
    after = C.c_uint64()
    torch.cuda.synchronize(dev)
    L = lib()
    check(L.tfhe_keygen_device(C.byref(params), seed & _M64, device, C.c_void_p(d_sk.data_ptr()),
                               C.c_void_p(d_bsk.data_ptr() if want_bsk else None),
                               C.c_void_p(d_ksk.data_ptr() if want_ksk else None), C.byref(after), None),
          "tfhe_keygen_device", L)
    keygen.seed_after = after.value

    def host(t):
        return None if t is None else t.cpu().numpy().view(np.uint64)

    return host(d_sk), host(d_bsk), host(d_ksk)


class BinFHEContextHIP:
    BETA = 128  # BinFHEContext::GetBeta, binfhecontext.h:348-350

    def __init__(self, params: Params, library: str | None = None):
        """library: another build of the C-ABI (capi.TEST_LIB: the test library with the fault probes)."""
        self.params = params
        self._h = C.c_void_p()
        self._L = lib(library)

    # -- GPUSetup / GPUClean (binfhecontext.cpp:349-365) --
    def GPUSetup(self, bsk_coeff, ksk, num_gpus: int = 1, bsk_format: str = "coefficient"):
        """bsk_format "coefficient" (tfhe_setup) or "evaluation": OpenFHE's NTT-domain
        values as KeyGen/BTKeyLoad leave them (tfhe_setup_eval, no host INTT)."""
        if bsk_format not in ("coefficient", "evaluation"):
            raise ValueError("bsk_format must be 'coefficient' or 'evaluation'")
        if self._h:
            self.GPUClean()
        p = self.params
        bsk = _u64(bsk_coeff).ravel()
        kk = _u64(ksk).ravel()
        if bsk.size != p.bsk_words() or kk.size != p.ksk_words():
            raise ValueError("key sizes do not match the parameters")
        fn = self._L.tfhe_setup if bsk_format == "coefficient" else self._L.tfhe_setup_eval
        self._check(fn(C.byref(self._h), C.byref(p), bsk, kk, num_gpus), fn.__name__)
        return self

    def _check(self, status, where):
        check(status, where, self._L)

    @classmethod
    def from_key_image(cls, params: Params, d_src: int, nbytes: int, device: int = 0, library: str | None = None):
        ctx = cls(params, library)
        ctx._check(ctx._L.tfhe_setup_from_key_image(C.byref(ctx._h), C.byref(params), C.c_void_p(d_src), nbytes, device),
                   "tfhe_setup_from_key_image")
        return ctx

    @classmethod
    def from_key_file(cls, params: Params, path: str, device: int = 0, library: str | None = None):
        """Adopt a key image saved by save_key_image (no host key conversion)."""
        ctx = cls(params, library)
        ctx._check(ctx._L.tfhe_setup_from_key_file(C.byref(ctx._h), C.byref(params), os.fsencode(path), device),
                   "tfhe_setup_from_key_file")
        return ctx

    @classmethod
    def from_keygen(cls, params: Params, seed: int, num_gpus: int = 1, library: str | None = None):
        """KeyGen + BTKeyGen on the device (tfhe_setup_keygen): the keys of stream `seed` are generated straight
        into the context's key arena.  Returns (context, sk); sk: n words mod qKS.  The stream is splitmix64
        (include/tfhe_hip.h): for tests, benchmarks and reproducible experiments, not a cryptographic generator."""
        ctx = cls(params, library)
        sk = np.empty(params.n, dtype=np.uint64)
        after = C.c_uint64()
        ctx._check(ctx._L.tfhe_setup_keygen(C.byref(ctx._h), C.byref(params), seed & _M64, num_gpus, sk,
                                            C.byref(after)), "tfhe_setup_keygen")
        ctx.seed_after = after.value
        return ctx, sk

    # -- Encrypt / Decrypt (binfhecontext.cpp:230-252) on the device; host arrays staged through `device` --
    def Encrypt(self, sk, m, p: int = 4, mod: int | None = None, seed: int = 0, device: int = 0):
        """m: B messages (negative and >= p are reduced mod p) -> ciphertexts [B, n+1] mod `mod` (default q).
        Ciphertext b reads the stream from seed + b (n + 2) draws; self.seed_after is the state behind the call."""
        msg = np.ascontiguousarray(np.atleast_1d(m), dtype=np.int64)
        if msg.ndim != 1 or msg.size == 0:
            raise ValueError(f"Encrypt: expected B >= 1 messages, got shape {msg.shape}")
        sk = self._sk(sk)
        ct = np.empty((msg.size, self.params.n + 1), dtype=np.uint64)
        after = C.c_uint64()
        self._check(self._L.tfhe_encrypt(C.byref(self.params), device, sk, msg.size, msg, p, mod or self.params.q,
                                         seed & _M64, ct.ravel(), C.byref(after), None), "tfhe_encrypt")
        self.seed_after = after.value
        return ct

    def Decrypt(self, sk, ct, p: int = 4, mod: int | None = None, device: int = 0):
        """ct [B, n+1] mod `mod` (default q) -> the B messages (a list of ints)."""
        ct, B = self._batch(ct, "Decrypt")
        if B == 0:
            raise ValueError("Decrypt: expected B >= 1 ciphertexts")
        out = np.empty(B, dtype=np.int64)
        self._check(self._L.tfhe_decrypt(C.byref(self.params), device, self._sk(sk), B, ct.ravel(), p,
                                         mod or self.params.q, out, None), "tfhe_decrypt")
        return [int(v) for v in out]

    def _sk(self, sk):
        sk = _u64(sk).ravel()
        if sk.size != self.params.n:
            raise ValueError(f"secret key: expected n = {self.params.n} words, got {sk.size}")
        return sk

    def EncryptDevice(self, B, d_sk, d_m, d_ct, p: int = 4, mod: int | None = None, seed: int = 0, device: int = 0,
                      stream=0):
        """d_sk[n] u64, d_m[B] i64 -> d_ct[B][n+1], device pointers; returns the stream state behind the call."""
        after = C.c_uint64()
        self._check(self._L.tfhe_encrypt_device(C.byref(self.params), device, C.c_void_p(d_sk), B, C.c_void_p(d_m), p,
                                                mod or self.params.q, seed & _M64, C.c_void_p(d_ct), C.byref(after),
                                                C.c_void_p(stream)), "tfhe_encrypt_device")
        return after.value

    def DecryptDevice(self, B, d_sk, d_ct, d_m, p: int = 4, mod: int | None = None, device: int = 0, stream=0):
        """d_ct[B][n+1] -> d_m[B] i64, device pointers."""
        self._check(self._L.tfhe_decrypt_device(C.byref(self.params), device, C.c_void_p(d_sk), B, C.c_void_p(d_ct), p,
                                                mod or self.params.q, C.c_void_p(d_m), C.c_void_p(stream)),
                    "tfhe_decrypt_device")

    def save_key_image(self, path: str):
        self._check(self._L.tfhe_save_key_image(self._h, os.fsencode(path)), "tfhe_save_key_image")

    def export_key_image(self, d_dst: int, nbytes: int, stream: int = 0):
        self._check(self._L.tfhe_export_key_image(self._h, C.c_void_p(d_dst), nbytes, C.c_void_p(stream)),
              "tfhe_export_key_image")

    def GPUClean(self):
        if self._h:
            self._check(self._L.tfhe_clean(self._h), "tfhe_clean")
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.GPUClean()
        except Exception:
            pass

    def info(self) -> Info:
        inf = Info()
        self._check(self._L.tfhe_get_info(self._h, C.byref(inf)), "tfhe_get_info")
        return inf

    @property
    def handle(self):
        return self._h

    # -- launch knobs (tfhe_knobs: environment at setup, then only these calls) --
    # pair_min has calls of its own (tfhe_knobs keeps its layout); here it is one more knob.  A library
    # without them (an earlier build in an A/B run) has no such knob.
    def knobs(self) -> dict:
        k = Knobs()
        self._check(self._L.tfhe_get_knobs(self._h, C.byref(k)), "tfhe_get_knobs")
        d = k.as_dict()
        if hasattr(self._L, "tfhe_get_pair_min"):
            v = C.c_int32()
            self._check(self._L.tfhe_get_pair_min(self._h, C.byref(v), None), "tfhe_get_pair_min")
            d["pair_min"] = v.value
        return d

    def pair_launches(self) -> int:
        """Blind rotations this context has launched on the pair instance (two ciphertexts per wavefront)."""
        n = C.c_uint64()
        self._check(self._L.tfhe_get_pair_min(self._h, None, C.byref(n)), "tfhe_get_pair_min")
        return n.value

    def set_knobs(self, **kw):
        kw = dict(kw)
        if "pair_min" in kw:
            self._check(self._L.tfhe_set_pair_min(self._h, int(kw.pop("pair_min"))), "tfhe_set_pair_min")
        k = Knobs()
        self._check(self._L.tfhe_get_knobs(self._h, C.byref(k)), "tfhe_get_knobs")
        for name, v in kw.items():
            if not hasattr(k, name):
                raise KeyError(f"unknown knob {name}")
            setattr(k, name, int(v))
        self._check(self._L.tfhe_set_knobs(self._h, C.byref(k)), "tfhe_set_knobs")

    @contextmanager
    def knobs_set(self, **kw):
        """Temporarily change knobs (tests, A/B runs); restored on exit."""
        old = self.knobs()
        self.set_knobs(**kw)
        try:
            yield self
        finally:
            self.set_knobs(**old)

    def GetBeta(self):
        return self.BETA

    def GetMaxPlaintextSpace(self):
        return self.params.q // self.BETA // 2

    # -- reference boundary calls --
    def EvalAcc(self, a, a_mod, acc):
        """EvalAcc_CUDA: a[B][n] mod a_mod, acc[B][2][N] -> new acc (acc0 transposed)."""
        n, N = self.params.n, self.params.N
        a = _u64(a)
        out = np.array(acc, dtype=np.uint64, copy=True, order="C")
        if a.size == 0 or a.size % n:
            raise ValueError(f"EvalAcc: a must hold B*n words (n = {n}), got {a.size}")
        B = a.size // n
        if out.size != B * 2 * N:
            raise ValueError(f"EvalAcc: acc must hold B*2*N = {B * 2 * N} words, got {out.size}")
        self._check(self._L.tfhe_eval_acc(self._h, B, a.ravel(), a_mod, out.ravel()), "tfhe_eval_acc")
        return out

    def MKMSwitch(self, ct_ext, fmod):
        ct_ext = _rows(ct_ext, self.params.N + 1, "MKMSwitch")
        B = ct_ext.shape[0]
        out = np.empty((B, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_mkm_switch(self._h, B, ct_ext.ravel(), fmod, out.ravel()), "tfhe_mkm_switch")
        return out

    def CiphertextMulMatrix(self, ct, matrix, modulus):
        ct = _rows(ct, self.params.n + 1, "CiphertextMulMatrix")
        m = np.ascontiguousarray(matrix, dtype=np.int64)
        if m.ndim != 2:
            raise ValueError("CiphertextMulMatrix: matrix must be 2-D [K][cols]")
        K, cols = m.shape
        if ct.size != K * (self.params.n + 1):  # lwe-operation.cu:66-69
            raise ValueError("The number of rows of the matrix must be equal to the number of input ciphertexts.")
        out = np.empty((cols, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_ciphertext_mul_matrix(self._h, K, ct.ravel(), cols, m.ravel(), modulus, out.ravel()),
              "tfhe_ciphertext_mul_matrix")
        return out

    @staticmethod
    def _layer_lut(who, lut, qq, channels):
        """A layer's table argument: (q,) one shared table, or (channels, q) one per channel -> (array, tabled)."""
        lut = _u64(lut)
        if lut.shape != (qq,) and lut.shape != (channels, qq):
            raise ValueError(f"{who}: LUT must have shape ({qq},) or ({channels}, {qq}), got {lut.shape}")
        return np.ascontiguousarray(lut), lut.ndim == 2

    # -- vector BinFHEContext surface --
    def _batch(self, ct, what="ciphertexts"):
        ct = _rows(ct, self.params.n + 1, what)
        return ct, ct.shape[0]

    def EvalBinGate(self, gate, ct1, ct2, q=None):
        ct1, B = self._batch(ct1, "EvalBinGate ct1")
        ct2, B2 = self._batch(ct2, "EvalBinGate ct2")
        if B != B2:  # binfhe-base-scheme.cpp:607
            raise ValueError(f"EvalBinGate: input ciphertexts size unmatched ({B} vs {B2})")
        g = BINGATE[gate] if isinstance(gate, str) else int(gate)
        out = np.empty((B, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_eval_bin_gate(self._h, g, B, ct1.ravel(), ct2.ravel(), q or self.params.q, out.ravel()),
              "tfhe_eval_bin_gate")
        return out

    def EvalFunc(self, ct, lut, q=None):
        ct, B = self._batch(ct, "EvalFunc")
        lut = _u64(lut)
        qq = q or self.params.q
        if not (lut.shape == (qq,) or lut.shape == (B, qq)):
            raise ValueError(f"EvalFunc: LUT must have shape ({qq},) or ({B}, {qq}), got {lut.shape}")
        out = np.empty((B, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_eval_func(self._h, B, ct.ravel(), qq, lut.ravel(), int(lut.ndim == 2),
                                   out.ravel()), "tfhe_eval_func")
        return out

    def EvalFuncTables(self, ct, luts, inner=1, q=None):
        """One table per channel: ct[B, n+1], luts[T, q]; ciphertext i uses table (i // inner) % T, every table
        classified on its own, each result bit for bit EvalFunc's with that table shared (tfhe_eval_func_tables)."""
        ct, B = self._batch(ct, "EvalFuncTables")
        luts = _u64(luts)
        qq = q or self.params.q
        if luts.ndim != 2 or luts.shape[0] == 0 or luts.shape[1] != qq:
            raise ValueError(f"EvalFuncTables: tables must have shape (T, {qq}), got {luts.shape}")
        out = np.empty((B, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_eval_func_tables(self._h, B, ct.ravel(), qq, luts.ravel(), luts.shape[0], inner,
                                                  out.ravel()), "tfhe_eval_func_tables")
        return out

    def EvalFloor(self, ct, mod, roundbits=0):
        ct, B = self._batch(ct, "EvalFloor")
        out = np.empty((B, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_eval_floor(self._h, B, ct.ravel(), mod, roundbits, out.ravel()), "tfhe_eval_floor")
        return out

    def EvalSign(self, ct, mod):
        ct, B = self._batch(ct, "EvalSign")
        out = np.empty((B, self.params.n + 1), dtype=np.uint64)
        self._check(self._L.tfhe_eval_sign(self._h, B, ct.ravel(), mod, out.ravel()), "tfhe_eval_sign")
        return out

    def EvalDecomp(self, ct, mod, max_digits=16):
        ct, B = self._batch(ct, "EvalDecomp")
        out = np.zeros((B, max_digits, self.params.n + 1), dtype=np.uint64)
        moduli = np.zeros(max_digits, dtype=np.uint64)
        nd = C.c_uint32()
        self._check(self._L.tfhe_eval_decomp(self._h, B, ct.ravel(), mod, max_digits, out.ravel(), moduli, C.byref(nd)),
              "tfhe_eval_decomp")
        d = nd.value
        return out[:, :d, :], [int(m) for m in moduli[:d]]

    # -- levelled Boolean circuits (tfhe_amd.Circuit): every level is one mixed batch --
    def EvalCircuit(self, circ, cts, q=None):
        """cts[num_inputs, instances, n+1] (or [num_inputs, n+1]: one instance) -> the outputs in the matching
        shape; host arrays staged through the context's first device."""
        inf, w = circ.info(), self.params.n + 1
        x = _u64(cts)
        one = x.ndim == 2
        if one:
            x = x[:, None, :]
        if x.ndim != 3 or x.shape[0] != inf["num_inputs"] or x.shape[2] != w or x.shape[1] == 0:
            raise ValueError(f"EvalCircuit: expected shape ({inf['num_inputs']}, instances, {w}), got {x.shape}")
        x = np.ascontiguousarray(x)
        out = np.empty((inf["num_outputs"], x.shape[1], w), dtype=np.uint64)
        self._check(self._L.tfhe_eval_circuit(self._h, circ.handle, x.shape[1], x.ravel(), q or self.params.q,
                                              out.ravel()), "tfhe_eval_circuit")
        return out[:, 0, :] if one else out

    def EvalCircuitDevice(self, circ, instances, d_in, d_out, q=None, stream=0):
        """d_in[num_inputs][instances][n+1] -> d_out[num_outputs][instances][n+1], device pointers."""
        self._check(self._L.tfhe_eval_circuit_device(self._h, circ.handle, instances, C.c_void_p(d_in),
                                                     q or self.params.q, C.c_void_p(d_out), C.c_void_p(stream)),
                    "tfhe_eval_circuit_device")

    # -- function circuits (tfhe_amd.FuncCircuit): linear forms and LUT bootstraps, every level one mixed batch --
    def EvalFuncCircuit(self, fc, cts):
        """cts[num_inputs, instances, n+1] mod the circuit's q (or [num_inputs, n+1]: one instance) -> the outputs
        in the matching shape; host arrays staged through the context's first device."""
        inf, w = fc.info(), self.params.n + 1
        x = _u64(cts)
        one = x.ndim == 2
        if one:
            x = x[:, None, :]
        if x.ndim != 3 or x.shape[0] != inf["num_inputs"] or x.shape[2] != w or x.shape[1] == 0:
            raise ValueError(f"EvalFuncCircuit: expected shape ({inf['num_inputs']}, instances, {w}), got {x.shape}")
        x = np.ascontiguousarray(x)
        out = np.empty((inf["num_outputs"], x.shape[1], w), dtype=np.uint64)
        self._check(self._L.tfhe_eval_fcircuit(self._h, fc.handle, x.shape[1], x.ravel(), out.ravel()),
                    "tfhe_eval_fcircuit")
        return out[:, 0, :] if one else out

    def EvalFuncCircuitDevice(self, fc, instances, d_in, d_out, stream=0):
        """d_in[num_inputs][instances][n+1] -> d_out[num_outputs][instances][n+1], device pointers."""
        self._check(self._L.tfhe_eval_fcircuit_device(self._h, fc.handle, instances, C.c_void_p(d_in),
                                                      C.c_void_p(d_out), C.c_void_p(stream)),
                    "tfhe_eval_fcircuit_device")

    # -- dense layers: y = f(W^T x + b), the matrix product then one shared-table EvalFunc, all on the device --
    def EvalDense(self, cts, matrix, lut, bias=None, q=None):
        """cts[instances, K, n+1] mod q (or [K, n+1]: one instance), matrix[K, cols] int64, lut[q], bias[cols] or None
        -> [instances, cols, n+1] (or [cols, n+1]); host arrays staged through the context's first device."""
        w, qq = self.params.n + 1, q or self.params.q
        x = _u64(cts)
        one = x.ndim == 2
        if one:
            x = x[None]
        m = np.ascontiguousarray(matrix, dtype=np.int64)
        if m.ndim != 2 or m.shape[0] == 0 or m.shape[1] == 0:
            raise ValueError(f"EvalDense: matrix must be 2-D [K][cols] and not empty, got {m.shape}")
        K, cols = m.shape
        if x.ndim != 3 or x.shape[0] == 0 or x.shape[1] != K or x.shape[2] != w:
            raise ValueError(f"EvalDense: expected shape (instances, {K}, {w}), got {x.shape}")
        lut, tabled = self._layer_lut("EvalDense", lut, qq, cols)
        b = None
        if bias is not None:
            b = _u64(bias)
            if b.shape != (cols,):
                raise ValueError(f"EvalDense: bias must have shape ({cols},), got {b.shape}")
        x = np.ascontiguousarray(x)
        out = np.empty((x.shape[0], cols, w), dtype=np.uint64)
        bp = C.c_void_p(b.ctypes.data if b is not None else None)
        if tabled:
            self._check(self._L.tfhe_eval_dense_tables(self._h, x.shape[0], K, x.ravel(), cols, m.ravel(), bp, qq,
                                                       lut.ravel(), cols, out.ravel()), "tfhe_eval_dense_tables")
        else:
            self._check(self._L.tfhe_eval_dense(self._h, x.shape[0], K, x.ravel(), cols, m.ravel(), bp, qq, lut,
                                                out.ravel()), "tfhe_eval_dense")
        return out[0] if one else out

    def EvalDenseDevice(self, instances, K, d_ct, cols, d_matrix, d_lut, d_out, d_bias=0, q=None, stream=0, num_luts=1):
        """d_ct[instances][K][n+1], d_matrix[K][cols] int64, d_lut[q], d_bias[cols] or 0 -> d_out[instances][cols][n+1],
        device pointers.  num_luts > 1: d_lut[num_luts = cols][q], one table per column."""
        if num_luts < 1:
            raise ValueError(f"EvalDenseDevice: num_luts must be at least 1, got {num_luts}")
        if num_luts > 1:
            self._check(self._L.tfhe_eval_dense_tables_device(self._h, instances, K, C.c_void_p(d_ct), cols,
                                                              C.c_void_p(d_matrix), C.c_void_p(d_bias),
                                                              q or self.params.q, C.c_void_p(d_lut), num_luts,
                                                              C.c_void_p(d_out), C.c_void_p(stream)),
                        "tfhe_eval_dense_tables_device")
            return
        self._check(self._L.tfhe_eval_dense_device(self._h, instances, K, C.c_void_p(d_ct), cols, C.c_void_p(d_matrix),
                                                   C.c_void_p(d_bias), q or self.params.q, C.c_void_p(d_lut),
                                                   C.c_void_p(d_out), C.c_void_p(stream)), "tfhe_eval_dense_device")

    def CiphertextMulMatrixDevice(self, instances, K, d_ct, cols, d_matrix, modulus, d_out, d_bias=0, stream=0):
        """d_ct[instances][K][n+1], d_matrix[K][cols] int64 (shared), d_bias[cols] or 0 -> d_out[instances][cols][n+1];
        no input is written."""
        self._check(self._L.tfhe_ciphertext_mul_matrix_device(self._h, instances, K, C.c_void_p(d_ct), cols,
                                                              C.c_void_p(d_matrix), C.c_void_p(d_bias), modulus,
                                                              C.c_void_p(d_out), C.c_void_p(stream)),
                    "tfhe_ciphertext_mul_matrix_device")

    # -- convolution layers: y = f(conv(x) + b), the gathered product then one shared-table EvalFunc --
    def EvalConv2d(self, cts, weight, lut, bias=None, stride=1, padding=0, groups=1, q=None):
        """cts[instances, C, H, W, n+1] mod q (or [C, H, W, n+1]: one instance), weight[C_out, C/groups, kh, kw] int64
        (OIHW), lut[q], bias[C_out] or None; stride and padding an int or a pair (rows, columns)
        -> [instances, C_out, oh, ow, n+1] (or [C_out, oh, ow, n+1]); host arrays staged through the first device."""
        w, qq = self.params.n + 1, q or self.params.q
        x = _u64(cts)
        one = x.ndim == 4
        if one:
            x = x[None]
        W = np.ascontiguousarray(weight, dtype=np.int64)
        if W.ndim != 4 or 0 in W.shape:
            raise ValueError(f"EvalConv2d: weight must be 4-D [C_out][C/groups][kh][kw] and not empty, got {W.shape}")
        if x.ndim != 5 or 0 in x.shape or x.shape[4] != w:
            raise ValueError(f"EvalConv2d: expected shape (instances, C, H, W, {w}), got {x.shape}")
        sh, sw = (stride, stride) if np.isscalar(stride) else stride
        ph, pw = (padding, padding) if np.isscalar(padding) else padding
        if groups < 1 or x.shape[1] != W.shape[1] * groups:
            raise ValueError(f"EvalConv2d: {x.shape[1]} input planes against weight {W.shape} with groups = {groups}")
        if min(sh, sw) < 1 or min(ph, pw) < 0:
            raise ValueError(f"EvalConv2d: stride {stride} must be >= 1 and padding {padding} >= 0")
        desc = Conv2d(x.shape[1], x.shape[2], x.shape[3], W.shape[0], W.shape[2], W.shape[3], sh, sw, ph, pw, groups)
        try:
            oh, ow, _ = conv2d_shape(desc)  # the descriptor's own rules, on the host; the message names the field
        except TfheError as e:
            raise ValueError(f"EvalConv2d: {e}") from None
        lut, tabled = self._layer_lut("EvalConv2d", lut, qq, W.shape[0])
        b = None
        if bias is not None:
            b = _u64(bias)
            if b.shape != (W.shape[0],):
                raise ValueError(f"EvalConv2d: bias must have shape ({W.shape[0]},), got {b.shape}")
        x = np.ascontiguousarray(x)
        out = np.empty((x.shape[0], W.shape[0], oh, ow, w), dtype=np.uint64)
        bp = C.c_void_p(b.ctypes.data if b is not None else None)
        if tabled:
            self._check(self._L.tfhe_eval_conv2d_tables(self._h, C.byref(desc), x.shape[0], x.ravel(), W.ravel(), bp, qq,
                                                        lut.ravel(), W.shape[0], out.ravel()), "tfhe_eval_conv2d_tables")
        else:
            self._check(self._L.tfhe_eval_conv2d(self._h, C.byref(desc), x.shape[0], x.ravel(), W.ravel(), bp, qq, lut,
                                                 out.ravel()), "tfhe_eval_conv2d")
        return out[0] if one else out

    def EvalConv2dDevice(self, desc, instances, d_ct, d_weight, d_lut, d_out, d_bias=0, q=None, stream=0, num_luts=1):
        """desc: tfhe_amd.Conv2d; d_ct[instances][c_in][h][w][n+1], d_weight[c_out][c_in/groups][kh][kw] int64, d_lut[q],
        d_bias[c_out] or 0 -> d_out[instances][c_out][oh][ow][n+1], device pointers.  num_luts > 1:
        d_lut[num_luts = c_out][q], one table per output plane."""
        if num_luts < 1:
            raise ValueError(f"EvalConv2dDevice: num_luts must be at least 1, got {num_luts}")
        if num_luts > 1:
            self._check(self._L.tfhe_eval_conv2d_tables_device(self._h, C.byref(desc), instances, C.c_void_p(d_ct),
                                                               C.c_void_p(d_weight), C.c_void_p(d_bias),
                                                               q or self.params.q, C.c_void_p(d_lut), num_luts,
                                                               C.c_void_p(d_out), C.c_void_p(stream)),
                        "tfhe_eval_conv2d_tables_device")
            return
        self._check(self._L.tfhe_eval_conv2d_device(self._h, C.byref(desc), instances, C.c_void_p(d_ct),
                                                    C.c_void_p(d_weight), C.c_void_p(d_bias), q or self.params.q,
                                                    C.c_void_p(d_lut), C.c_void_p(d_out), C.c_void_p(stream)),
                    "tfhe_eval_conv2d_device")

    def CiphertextConv2dDevice(self, desc, instances, d_ct, d_weight, modulus, d_out, d_bias=0, stream=0):
        """The gathered product alone at any modulus: d_ct[instances][c_in][h][w][n+1], d_weight (OIHW int64, shared),
        d_bias[c_out] or 0 -> d_out[instances][c_out][oh][ow][n+1]; no input is written."""
        self._check(self._L.tfhe_ciphertext_conv2d_device(self._h, C.byref(desc), instances, C.c_void_p(d_ct),
                                                          C.c_void_p(d_weight), C.c_void_p(d_bias), modulus,
                                                          C.c_void_p(d_out), C.c_void_p(stream)),
                    "tfhe_ciphertext_conv2d_device")

    # -- pooling layers: a windowed pair tournament, op(a, b) = b + EvalFunc(a - b) with one shared table --
    def EvalPool2d(self, cts, lut, kernel, stride=None, padding=0, q=None):
        """cts[instances, C, H, W, n+1] mod q (or [C, H, W, n+1]: one instance), lut[q]; kernel, stride and padding an
        int or a pair (rows, columns), stride defaulting to the kernel as in PyTorch -> [instances, C, oh, ow, n+1]
        (or [C, oh, ow, n+1]); host arrays staged through the first device.  With tfhe_amd.max_table(q) it is max
        pooling (EvalMaxPool2d); a tap in the padding is left out."""
        w, qq = self.params.n + 1, q or self.params.q
        x = _u64(cts)
        one = x.ndim == 4
        if one:
            x = x[None]
        if x.ndim != 5 or 0 in x.shape or x.shape[4] != w:
            raise ValueError(f"EvalPool2d: expected shape (instances, C, H, W, {w}), got {x.shape}")
        kh, kw = (kernel, kernel) if np.isscalar(kernel) else kernel
        sh, sw = (kh, kw) if stride is None else (stride, stride) if np.isscalar(stride) else stride
        ph, pw = (padding, padding) if np.isscalar(padding) else padding
        if min(kh, kw, sh, sw) < 1 or min(ph, pw) < 0:
            raise ValueError(f"EvalPool2d: kernel {kernel} and stride {stride} must be >= 1 and padding {padding} >= 0")
        desc = Pool2d(x.shape[1], x.shape[2], x.shape[3], kh, kw, sh, sw, ph, pw)
        try:
            oh, ow, _, _ = pool2d_shape(desc)  # the descriptor's own rules, on the host; the message names the field
        except TfheError as e:
            raise ValueError(f"EvalPool2d: {e}") from None
        lut, tabled = self._layer_lut("EvalPool2d", lut, qq, x.shape[1])
        x = np.ascontiguousarray(x)
        out = np.empty((x.shape[0], x.shape[1], oh, ow, w), dtype=np.uint64)
        if tabled:
            self._check(self._L.tfhe_eval_pool2d_tables(self._h, C.byref(desc), x.shape[0], x.ravel(), qq, lut.ravel(),
                                                        x.shape[1], out.ravel()), "tfhe_eval_pool2d_tables")
        else:
            self._check(self._L.tfhe_eval_pool2d(self._h, C.byref(desc), x.shape[0], x.ravel(), qq, lut, out.ravel()),
                        "tfhe_eval_pool2d")
        return out[0] if one else out

    def EvalMaxPool2d(self, cts, kernel, stride=None, padding=0, negacyclic=False, q=None):
        """Max pooling: EvalPool2d with tfhe_amd.max_table(q, negacyclic).  The default table takes two bootstraps per
        pair and differences in (-q/2, q/2); negacyclic=True takes one and differences in (-q/4, q/4)."""
        return self.EvalPool2d(cts, max_table(q or self.params.q, negacyclic), kernel, stride, padding, q)

    def EvalPool2dDevice(self, desc, instances, d_ct, d_lut, d_out, q=None, stream=0, num_luts=1):
        """desc: tfhe_amd.Pool2d; d_ct[instances][c][h][w][n+1], d_lut[q] -> d_out[instances][c][oh][ow][n+1], device
        pointers; no input word is written.  num_luts > 1: d_lut[num_luts = c][q], one table per plane."""
        if num_luts < 1:
            raise ValueError(f"EvalPool2dDevice: num_luts must be at least 1, got {num_luts}")
        if num_luts > 1:
            self._check(self._L.tfhe_eval_pool2d_tables_device(self._h, C.byref(desc), instances, C.c_void_p(d_ct),
                                                               q or self.params.q, C.c_void_p(d_lut), num_luts,
                                                               C.c_void_p(d_out), C.c_void_p(stream)),
                        "tfhe_eval_pool2d_tables_device")
            return
        self._check(self._L.tfhe_eval_pool2d_device(self._h, C.byref(desc), instances, C.c_void_p(d_ct),
                                                    q or self.params.q, C.c_void_p(d_lut), C.c_void_p(d_out),
                                                    C.c_void_p(stream)),
                    "tfhe_eval_pool2d_device")

    # -- products of two encrypted tensors: sum_k EvalFunc(x + y, luts[0]) - EvalFunc(x - y, luts[1]) --
    def EvalCtMatMul(self, x, y, luts, transposed=False, q=None):
        """x[instances, R, K, n+1] mod q times y[instances, K, C, n+1], or y[K, C, n+1] shared by every instance
        (encrypted weights); with transposed the K and C axes of y are swapped (Q K^T) -> [instances, R, C, n+1]:
        out[i, r, c] = sum_k EvalFunc(x[i, r, k] + y[i, k, c], luts[0]) - EvalFunc(x[i, r, k] - y[i, k, c], luts[1])
        mod q, luts[2, q].  With tfhe_amd.product_tables(q, p) it is the matrix product of the messages mod p.  Host
        arrays staged through the first device (tfhe_eval_ct_matmul)."""
        w, qq = self.params.n + 1, q or self.params.q
        x, y = _u64(x), _u64(y)
        if x.ndim != 4 or 0 in x.shape or x.shape[3] != w:
            raise ValueError(f"EvalCtMatMul: x: expected shape (instances, R, K, {w}), got {x.shape}")
        n, K = x.shape[0], x.shape[2]
        kc = f"C, {K}" if transposed else f"{K}, C"
        if y.ndim not in (3, 4) or 0 in y.shape or y.shape[-1] != w or y.shape[-2 if transposed else -3] != K or \
                (y.ndim == 4 and y.shape[0] != n):
            raise ValueError(f"EvalCtMatMul: y: expected shape ({n}, {kc}, {w}) or ({kc}, {w}), got {y.shape}")
        desc = CtMatMul(x.shape[1], K, y.shape[-3 if transposed else -2], transposed, y.ndim == 3)
        luts = _u64(luts)
        if luts.shape != (2, qq):
            raise ValueError(f"EvalCtMatMul: tables must have shape (2, {qq}), got {luts.shape}")
        out = np.empty((n, desc.rows, desc.cols, w), dtype=np.uint64)
        self._check(self._L.tfhe_eval_ct_matmul(self._h, C.byref(desc), n, x.ravel(), y.ravel(), qq, luts.ravel(),
                                                out.ravel()), "tfhe_eval_ct_matmul")
        return out

    def EvalCtMul(self, x, y, luts, q=None):
        """Elementwise on equal shapes [..., n+1]: out = EvalFunc(x + y, luts[0]) - EvalFunc(x - y, luts[1]) mod q;
        with tfhe_amd.product_tables(q, p) the product of the messages mod p.  EvalCtMatMul with R = K = C = 1 and
        one instance per element."""
        w = self.params.n + 1
        x, y = _u64(x), _u64(y)
        if x.ndim < 1 or x.shape[-1] != w or x.size == 0 or x.shape != y.shape:
            raise ValueError(f"EvalCtMul: expected two equal shapes (..., {w}), got {x.shape} and {y.shape}")
        out = self.EvalCtMatMul(x.reshape(-1, 1, 1, w), y.reshape(-1, 1, 1, w), luts, q=q)
        return out.reshape(x.shape)

    def EvalCtMatMulDevice(self, desc, instances, d_x, d_y, d_luts, d_out, q=None, stream=0):
        """desc: tfhe_amd.CtMatMul; d_x[instances][rows][inner][n+1], d_y[instances][inner][cols][n+1] (its axes as
        desc.y_transposed / desc.y_shared say), d_luts[2][q] -> d_out[instances][rows][cols][n+1], device pointers; no
        input word is written."""
        self._check(self._L.tfhe_eval_ct_matmul_device(self._h, C.byref(desc), instances, C.c_void_p(d_x),
                                                       C.c_void_p(d_y), q or self.params.q, C.c_void_p(d_luts),
                                                       C.c_void_p(d_out), C.c_void_p(stream)),
                    "tfhe_eval_ct_matmul_device")

    # -- device-resident (pointers are integers, e.g. torch tensor.data_ptr()) --
    def EvalBinGateDevice(self, gate, B, d_ct1, d_ct2, d_out, q=None, stream=0):
        g = BINGATE[gate] if isinstance(gate, str) else int(gate)
        self._check(self._L.tfhe_eval_bin_gate_device(self._h, g, B, C.c_void_p(d_ct1), C.c_void_p(d_ct2),
                                              q or self.params.q, C.c_void_p(d_out), C.c_void_p(stream)),
              "tfhe_eval_bin_gate_device")

    def EvalFuncDevice(self, B, d_ct, d_lut, d_out, q=None, per_ct_lut=False, stream=0):
        self._check(self._L.tfhe_eval_func_device(self._h, B, C.c_void_p(d_ct), q or self.params.q, C.c_void_p(d_lut),
                                          int(per_ct_lut), C.c_void_p(d_out), C.c_void_p(stream)),
              "tfhe_eval_func_device")

    def EvalFuncTablesDevice(self, B, d_ct, d_luts, num_luts, d_out, inner=1, q=None, stream=0):
        """d_ct[B][n+1], d_luts[num_luts][q] -> d_out[B][n+1], device pointers; ciphertext i uses table
        (i // inner) % num_luts."""
        self._check(self._L.tfhe_eval_func_tables_device(self._h, B, C.c_void_p(d_ct), q or self.params.q,
                                                         C.c_void_p(d_luts), num_luts, inner, C.c_void_p(d_out),
                                                         C.c_void_p(stream)), "tfhe_eval_func_tables_device")

    def EvalFloorDevice(self, B, d_ct, mod, d_out, roundbits=0, stream=0):
        self._check(self._L.tfhe_eval_floor_device(self._h, B, C.c_void_p(d_ct), mod, roundbits, C.c_void_p(d_out),
                                           C.c_void_p(stream)), "tfhe_eval_floor_device")

    def EvalSignDevice(self, B, d_ct, mod, d_out, stream=0):
        self._check(self._L.tfhe_eval_sign_device(self._h, B, C.c_void_p(d_ct), mod, C.c_void_p(d_out), C.c_void_p(stream)),
              "tfhe_eval_sign_device")
