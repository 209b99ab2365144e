"""FuncCircuit: a compiled netlist of linear forms and LUT bootstraps over Z_q (tfhe_fcircuit of
include/tfhe_hip.h), evaluated level by level on the device by BinFHEContextHIP.EvalFuncCircuit /
EvalFuncCircuitDevice.  Compiling and eval_plain need no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import FCIRCUIT_OPS, FuncCircuitInfo, FuncNode, check, lib


def _term(t):
    """(wire, coefficient), or a bare wire (coefficient 1)."""
    if isinstance(t, (tuple, list)):
        return int(t[0]), int(t[1])
    return int(t), 1


def node_row(node):
    """("LIN", (in0, c0)[, (in1, c1)][, k]) or ("LUT", lut, (in0, c0)[, (in1, c1)][, k]) -> the fields of
    tfhe_fcircuit_node (op, in0, in1, c0, c1, lut, k).  The second term and k may be left out; k is told from
    a term by being a plain integer after the first term."""
    op, *rest = node
    code = FCIRCUIT_OPS[op] if isinstance(op, str) else int(op)
    lut = int(rest.pop(0)) if code == FCIRCUIT_OPS["LUT"] else 0
    if not rest:
        raise ValueError(f"node {node!r}: needs at least one term")
    in0, c0 = _term(rest.pop(0))
    in1, c1, k = 0, 0, 0
    if rest and isinstance(rest[0], (tuple, list)):
        in1, c1 = _term(rest.pop(0))
    if rest:
        k = int(rest.pop(0))
    if rest:
        raise ValueError(f"node {node!r}: too many fields")
    return code, in0, in1, c0, c1, lut, k


class FuncCircuit:
    """Wires 0 .. num_inputs-1 are the inputs; nodes[g] defines wire num_inputs + g as the linear form
    c0 w[in0] + c1 w[in1] + k mod q ("LIN") or as EvalFunc of that form under luts[lut] ("LUT"), and reads only
    lower-numbered wires.  luts is [num_luts, q]; outputs names wires."""

    def __init__(self, num_inputs: int, nodes, luts, outputs, q: int, library: str | None = None):
        self._L = lib(library)
        self._h = C.c_void_p()
        self._freed = False
        rows = [node_row(n) for n in nodes]
        arr = (FuncNode * max(1, len(rows)))(*rows)
        tables = np.ascontiguousarray(luts, dtype=np.uint64)
        if tables.size and (tables.ndim != 2 or tables.shape[1] != q):
            raise ValueError(f"FuncCircuit: luts must have shape (num_luts, {q}), got {tables.shape}")
        outs = np.ascontiguousarray(outputs, dtype=np.uint32).ravel()
        check(self._L.tfhe_fcircuit_compile(C.byref(self._h), int(num_inputs), C.cast(arr, C.c_void_p), len(rows), int(q),
                                            C.c_void_p(tables.ctypes.data if tables.size else None),
                                            tables.shape[0] if tables.size else 0,
                                            C.c_void_p(outs.ctypes.data if outs.size else None), outs.size),
              "tfhe_fcircuit_compile", self._L)
        self._info = self.info()

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        inf = FuncCircuitInfo()
        check(self._L.tfhe_fcircuit_get_info(self._h, C.byref(inf)), "tfhe_fcircuit_get_info", self._L)
        return inf.as_dict()

    def level_widths(self) -> list[int]:
        w = np.zeros(max(1, self._info["levels"]), dtype=np.uint32)
        check(self._L.tfhe_fcircuit_level_widths(self._h, C.c_void_p(w.ctypes.data), w.size),
              "tfhe_fcircuit_level_widths", self._L)
        return [int(x) for x in w[:self._info["levels"]]]

    def eval_plain(self, values):
        """The lowered plan on clear values mod q: values[num_inputs, instances] (or [num_inputs]) -> uint64
        [num_outputs, instances] (or [num_outputs])."""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        one = v.ndim == 1
        if one:
            v = v[:, None]
        ni, no = self._info["num_inputs"], self._info["num_outputs"]
        if v.ndim != 2 or v.shape[0] != ni:
            raise ValueError(f"eval_plain: expected shape ({ni}, instances), got {v.shape}")
        v = np.ascontiguousarray(v)
        out = np.zeros((no, v.shape[1]), dtype=np.uint64)
        check(self._L.tfhe_fcircuit_eval_plain(self._h, v.shape[1], C.c_void_p(v.ctypes.data if v.size else None),
                                               C.c_void_p(out.ctypes.data)), "tfhe_fcircuit_eval_plain", self._L)
        return out[:, 0] if one else out

    def free(self):
        """Releases the plan.  The library keeps a registry of live circuits, so a second free, or any use of the
        circuit afterwards, raises TfheError instead of following a dangling handle."""
        self._freed = True
        check(self._L.tfhe_fcircuit_free(self._h), "tfhe_fcircuit_free", self._L)

    def __del__(self):
        try:
            if not self._freed and self._h:
                self.free()
        except Exception:
            pass
