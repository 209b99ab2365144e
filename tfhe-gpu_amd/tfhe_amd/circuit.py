"""Circuit: a compiled netlist of mixed gates (tfhe_circuit of include/tfhe_hip.h), evaluated level by
level on the device by BinFHEContextHIP.EvalCircuit / EvalCircuitDevice.  Compiling and eval_plain need
no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import CIRCUIT_OPS, CircuitGate, CircuitInfo, check, lib


class Circuit:
    """Wires 0 .. num_inputs-1 are the inputs; gates[g] = (op, in0, in1) defines wire num_inputs + g and
    reads only lower-numbered wires; op is a name ("AND", ..., "NOT", "CONST0", "CONST1") or an integer.
    in1 is ignored for NOT, both operands for the constants (they may be left out).  outputs names wires."""

    def __init__(self, num_inputs: int, gates, outputs, library: str | None = None):
        self._L = lib(library)
        self._h = C.c_void_p()
        rows = []
        for g in gates:
            op, *ins = g
            ins = list(ins) + [0] * (2 - len(ins))
            rows.append((CIRCUIT_OPS[op] if isinstance(op, str) else int(op), int(ins[0]), int(ins[1])))
        arr = (CircuitGate * max(1, len(rows)))(*rows)
        outs = np.ascontiguousarray(outputs, dtype=np.uint32).ravel()
        check(self._L.tfhe_circuit_compile(C.byref(self._h), int(num_inputs), C.cast(arr, C.c_void_p), len(rows),
                                           C.c_void_p(outs.ctypes.data if outs.size else None), outs.size),
              "tfhe_circuit_compile", self._L)
        self._info = self.info()

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        inf = CircuitInfo()
        check(self._L.tfhe_circuit_get_info(self._h, C.byref(inf)), "tfhe_circuit_get_info", self._L)
        return inf.as_dict()

    def level_widths(self) -> list[int]:
        w = np.zeros(max(1, self._info["levels"]), dtype=np.uint32)
        check(self._L.tfhe_circuit_level_widths(self._h, C.c_void_p(w.ctypes.data), w.size),
              "tfhe_circuit_level_widths", self._L)
        return [int(x) for x in w[:self._info["levels"]]]

    def eval_plain(self, bits):
        """The lowered plan on clear bits: bits[num_inputs, instances] (or [num_inputs]) -> uint8
        [num_outputs, instances] (or [num_outputs])."""
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        one = b.ndim == 1
        if one:
            b = b[:, None]
        ni, no = self._info["num_inputs"], self._info["num_outputs"]
        if b.ndim != 2 or b.shape[0] != ni:
            raise ValueError(f"eval_plain: expected shape ({ni}, instances), got {b.shape}")
        b = np.ascontiguousarray(b)
        out = np.zeros((no, b.shape[1]), dtype=np.uint8)
        check(self._L.tfhe_circuit_eval_plain(self._h, b.shape[1], C.c_void_p(b.ctypes.data if b.size else None),
                                              C.c_void_p(out.ctypes.data)), "tfhe_circuit_eval_plain", self._L)
        return out[:, 0] if one else out

    def free(self):
        if self._h:
            self._L.tfhe_circuit_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
