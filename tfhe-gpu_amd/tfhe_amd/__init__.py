"""tfhe_amd -- Python binding of the MI355X-native batched CGGI/GINX bootstrapping engine.

The engine is the C-ABI shared library built from ``tfhe-gpu_amd/csrc`` (see
``include/tfhe_hip.h``).  This package only marshals numpy arrays through ctypes
and mirrors the vector ``BinFHEContext`` surface of the reference
(binfhecontext.cpp:316-365): ``GPUSetup``, ``EvalBinGate``, ``EvalFunc``,
``EvalFloor``, ``EvalSign``, ``EvalDecomp``, plus the low-level
``EvalAcc``/``MKMSwitch`` boundary calls, ``Circuit`` / ``EvalCircuit``:
a netlist of mixed gates evaluated level by level on the device, and ``FuncCircuit`` / ``EvalFuncCircuit``: the
same for netlists of linear forms and LUT bootstraps over Z_q.  ``BinFHEContextHIP.from_keygen``, ``Encrypt``,
``Decrypt`` and ``keygen`` generate keys and ciphertexts on the device from a seeded splitmix64 stream (tests,
benchmarks, reproducible experiments -- not a cryptographic generator).  There is no CPU fallback: if the
library or a GPU is missing, calls raise.
"""
from .capi import (BINGATE, CIRCUIT_OPS, FCIRCUIT_OPS, PARAMSETS, TfheError, Params, lib, library_path, build, exported_symbols,
                   params_from_set, params_from_logq, host_selftest, mm_tiles, Conv2d, conv2d_shape, conv2d_tiles, Pool2d, pool2d_shape,
                   pool2d_eval_plain, max_table, lut_classes, lut_tables_info, CtMatMul, ct_matmul_info, ct_matmul_eval_plain,
                   product_tables)
from .circuit import Circuit
from .fcircuit import FuncCircuit
from .context import BinFHEContextHIP, keygen

__all__ = ["BINGATE", "CIRCUIT_OPS", "Circuit", "FCIRCUIT_OPS", "FuncCircuit", "PARAMSETS", "TfheError", "Params", "lib", "library_path", "build", "exported_symbols",
           "params_from_set", "params_from_logq", "host_selftest", "mm_tiles", "Conv2d", "conv2d_shape", "conv2d_tiles", "Pool2d", "pool2d_shape", "pool2d_eval_plain", "max_table", "lut_classes", "lut_tables_info", "CtMatMul", "ct_matmul_info", "ct_matmul_eval_plain", "product_tables", "BinFHEContextHIP", "keygen"]
