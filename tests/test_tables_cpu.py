"""No GPU: the host-only side of one table per channel: tfhe_lut_tables_info's classes against the class
a one-node FuncCircuit reports, its per-class and bootstrap counts against a count written out in numpy, its argument
errors, and the Python layers' refusal of a table array with the wrong number of channels."""
import ctypes as C

import numpy as np
import pytest

import tables_model
import tfhe_amd
from tfhe_amd import capi


@pytest.mark.parametrize("q", [8, 1 << 10, 1 << 12])
def test_classes_equal_the_function_circuits(q):
    kinds = ["negacyclic", "periodic", "arbitrary"] * 3
    luts = tables_model.tables(q, kinds)
    got = tfhe_amd.lut_classes(luts, q)
    assert got.tolist() == [tables_model.CLASS[k] for k in kinds]
    for t, lut in enumerate(luts):
        fc = tfhe_amd.FuncCircuit(1, [("LUT", 0, (0, 1))], lut[None], [1], q)
        inf = fc.info()
        assert [inf["negacyclic"], inf["periodic"], inf["arbitrary"]] == [int(got[t] == k) for k in range(3)], t
        fc.free()
    assert len({t.tobytes() for t in luts}) == 9  # three different tables of each class


@pytest.mark.parametrize("B,inner,T", [(13, 2, 3), (1, 1, 4), (70001, 5, 3), (3, 2, 5)])  # the last: T > B
def test_counts_equal_a_written_out_count(B, inner, T):
    q = 16
    kinds = [tables_model.KINDS[(t + 1) % 3] for t in range(T)]
    luts = tables_model.tables(q, kinds)
    classes, per, boots = tfhe_amd.lut_tables_info(luts, q, inner, B)
    want_per, want_boots = tables_model.counts(classes, B, inner)
    assert list(per) == want_per and sum(per) == B
    assert boots == want_boots


def _info(q, luts, T, inner, B, per=True, boots=True):
    p, b = (capi.SZ * 3)(), capi.U64()
    return capi.lib().tfhe_lut_tables_info(q, C.c_void_p(luts.ctypes.data if luts is not None else None), T, inner, B,
                                           None, p if per else None, C.byref(b) if boots else None)


def test_argument_errors_name_the_field():
    q = 16
    luts = tables_model.tables(q, ["negacyclic", "periodic"])
    assert _info(q, luts, 2, 1, 4) == 0  # classes may be NULL
    cases = [(lambda: _info(q, None, 2, 1, 4), "luts"), (lambda: _info(q, luts, 2, 1, 4, per=False), "per_class"),
             (lambda: _info(q, luts, 2, 1, 4, boots=False), "bootstraps"), (lambda: _info(q, luts, 2, 1, 0), "B"),
             (lambda: _info(q, luts, 0, 1, 4), "num_luts"), (lambda: _info(q, luts, 2, 0, 4), "inner"),
             (lambda: _info(4, luts, 2, 1, 4), "q"), (lambda: _info(24, luts, 2, 1, 4), "q"),
             (lambda: _info(1 << 62, luts, 8, 1, 4), "num_luts q"), (lambda: _info(q, luts, 2, 1 << 63, 4), "inner num_luts")]
    for call, field in cases:
        assert call() == 1, field  # TFHE_ERR_INVALID_ARGUMENT
        assert field in capi.lib().tfhe_last_error().decode(), field


def test_layers_refuse_a_table_array_of_the_wrong_channel_count():
    """The shape check comes before the library is asked for a device: a context object without keys is enough."""
    cp = tfhe_amd.params_from_set("STD128")
    ctx = tfhe_amd.BinFHEContextHIP(cp)
    q, w = cp.q, cp.n + 1
    lut = np.zeros(q, dtype=np.uint64)
    dense = np.zeros((1, 2, w), dtype=np.uint64), np.ones((2, 3), dtype=np.int64)
    conv = np.zeros((1, 1, 3, 3, w), dtype=np.uint64), np.ones((3, 1, 2, 2), dtype=np.int64)
    pool = np.zeros((1, 3, 2, 2, w), dtype=np.uint64)
    calls = [lambda t: ctx.EvalDense(dense[0], dense[1], t), lambda t: ctx.EvalConv2d(conv[0], conv[1], t),
             lambda t: ctx.EvalPool2d(pool, t, 2)]
    shapes = rf"\({q},\) or \(3, {q}\)"  # the message names both admitted shapes; channels = 3 in every layer
    for call in calls:
        for ch in (2, 4):
            with pytest.raises(ValueError, match=shapes):
                call(np.tile(lut, (ch, 1)))
        # (channels, q) passes the shape check: the call reaches the library, which refuses a context without keys
        with pytest.raises(tfhe_amd.TfheError):
            call(np.tile(lut, (3, 1)))


def test_device_wrappers_refuse_a_table_count_below_one():
    """num_luts = 1 is the shared-table entry and a larger value the tabled one; 0 or less is neither."""
    ctx = tfhe_amd.BinFHEContextHIP(tfhe_amd.params_from_set("STD128"))
    conv, pool = tfhe_amd.Conv2d(1, 3, 3, 3, 2, 2, 1, 1, 0, 0, 1), tfhe_amd.Pool2d(3, 2, 2, 2, 2, 2, 2, 0, 0)
    for n in (0, -1):
        with pytest.raises(ValueError, match="num_luts"):
            ctx.EvalDenseDevice(1, 2, 0, 3, 0, 0, 0, num_luts=n)
        with pytest.raises(ValueError, match="num_luts"):
            ctx.EvalConv2dDevice(conv, 1, 0, 0, 0, 0, num_luts=n)
        with pytest.raises(ValueError, match="num_luts"):
            ctx.EvalPool2dDevice(pool, 1, 0, 0, 0, num_luts=n)
