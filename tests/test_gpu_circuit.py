"""GPU: levelled Boolean circuits in one call (tfhe_eval_circuit / tfhe_eval_circuit_device): every level of a
compiled netlist runs as one mixed batch -- one preparation launch that gathers the operands by wire index and
builds each gate's own test vector, then the blind rotation, the extraction and the key switch once for the level.

The expected value is always the CPU oracle composed gate by gate in netlist order (circuit_nets.oracle_netlist:
orc.eval_bin_gate for the eight gates, NOT and the constants as the reference defines them), bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

import circuit_nets as nets
from helpers import random_cts

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)).to(torch.device("cuda", 0))


def run_device(ctx, circ, cts, q=None, stream=None):
    """EvalCircuitDevice on host arrays copied to cuda:0: cts[num_inputs, instances, n+1] -> numpy outputs."""
    import torch

    d_in = _dev(cts)
    inst, w = cts.shape[1], cts.shape[2]
    d_out = torch.zeros((circ.info()["num_outputs"], inst, w), dtype=torch.int64, device=d_in.device)
    torch.cuda.synchronize()
    ctx.EvalCircuitDevice(circ, inst, d_in.data_ptr(), d_out.data_ptr(), q=q,
                          stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().astype(np.uint64)


@pytest.fixture(scope="module")
def toy(oracle):
    """A context of its own on TOY parameters with valid keys (as smoke()): its scratch and wire store start empty."""
    import tfhe_amd

    op = oracle.params_from_set("TOY")
    rng = oracle.Rng(2025)
    sk, bsk, ksk = oracle.keygen(op, rng)
    cp = tfhe_amd.params_from_set("TOY")
    ctx = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    yield dict(op=op, cp=cp, ctx=ctx, orc=orc, sk=sk, rng=rng, keys=(bsk, ksk), tfhe=tfhe_amd, po=oracle)
    ctx.GPUClean()
    orc.close()


@pytest.fixture(scope="module")
def circuits():
    import tfhe_amd

    return dict(all_ops=tfhe_amd.Circuit(nets.ALL_OPS_INPUTS, nets.ALL_OPS, nets.ALL_OPS_OUTPUTS),
                mixed=tfhe_amd.Circuit(nets.MIXED_INPUTS, nets.MIXED, nets.MIXED_OUTPUTS))


@pytest.fixture(scope="module")
def toy_all_ops(toy, circuits):
    """The all-ops netlist on encrypted random bits, three instances: inputs, bits, the oracle composition (computed once)."""
    op, po = toy["op"], toy["po"]
    bits = np.random.default_rng(5).integers(0, 2, (nets.ALL_OPS_INPUTS, 3), dtype=np.uint8)
    cts = np.stack([np.stack([po.encrypt(op, toy["rng"], toy["sk"], int(m), 4, op.q) for m in row]) for row in bits])
    want = nets.oracle_netlist(toy["orc"], nets.ALL_OPS_INPUTS, nets.ALL_OPS, nets.ALL_OPS_OUTPUTS, cts, op.q)
    return dict(bits=bits, cts=cts, want=want)


def test_truth_on_real_keys(toy, circuits, toy_all_ops):
    op, po, ctx, circ = toy["op"], toy["po"], toy["ctx"], circuits["all_ops"]
    cts, want = toy_all_ops["cts"], toy_all_ops["want"]
    before = ctx.info().bootstraps
    got = ctx.EvalCircuit(circ, cts)
    assert ctx.info().bootstraps - before == circ.info()["bootstraps"] * 3
    assert got.shape == want.shape == (len(nets.ALL_OPS_OUTPUTS), 3, op.n + 1)
    assert np.array_equal(got, want)
    dec = np.array([[po.decrypt(op, toy["sk"], ct, 4, op.q) for ct in row] for row in got], dtype=np.uint8)
    assert np.array_equal(dec, circ.eval_plain(toy_all_ops["bits"]))
    # the device form, on a caller stream, equals the host form; one instance given as [num_inputs, n+1]
    import torch

    assert np.array_equal(run_device(ctx, circ, cts, stream=torch.cuda.Stream(torch.device("cuda", 0))), got)
    assert np.array_equal(ctx.EvalCircuit(circ, cts[:, 1]), got[:, 1])


@pytest.fixture(scope="module")
def mixed_reference(shared_kat):
    """Per parameter set: random input ciphertexts of the mixed netlist, three instances, and the oracle composition."""
    cache = {}

    def get(name):
        if name not in cache:
            s = shared_kat(name)
            cp = s["cp"]
            cts = np.stack([random_cts(np.random.default_rng(40 + i), 3, cp.n, cp.q) for i in range(nets.MIXED_INPUTS)])
            want = nets.oracle_netlist(s["orc"], nets.MIXED_INPUTS, nets.MIXED, nets.MIXED_OUTPUTS, cts, cp.q)
            cache[name] = (cts, want)
        return cache[name]

    return get


@pytest.mark.parametrize("name,knob", [("STD128", "split4"), ("STD128Q", "duo")])
def test_parity_on_the_production_kernels(shared_kat, circuits, mixed_reference, name, knob):
    ctx, circ = shared_kat(name)["ctx"], circuits["mixed"]
    assert circ.level_widths() == nets.MIXED_WIDTHS
    cts, want = mixed_reference(name)
    got3 = ctx.EvalCircuit(circ, cts)
    assert np.array_equal(got3, want)
    got1 = ctx.EvalCircuit(circ, cts[:, :1])
    assert np.array_equal(got1, want[:, :1])
    assert np.array_equal(run_device(ctx, circ, cts), want)  # the host form equals the device form
    assert ctx.knobs()[knob] > 0
    with ctx.knobs_set(**{knob: 0}):  # the one-workgroup / one-group forms of the same blind rotation
        assert np.array_equal(ctx.EvalCircuit(circ, cts), want)
        assert np.array_equal(ctx.EvalCircuit(circ, cts[:, :1]), want[:, :1])


def test_scratch_growth(toy):
    """A level of 5 * 205 = 1025 bootstraps, past the 1024-ciphertext scratch floor a small call leaves."""
    op, ctx, orc, tfhe = toy["op"], toy["ctx"], toy["orc"], toy["tfhe"]
    fresh = tfhe.BinFHEContextHIP(toy["cp"]).GPUSetup(*toy["keys"])  # its scratch starts empty
    try:
        rs = np.random.default_rng(7)
        small = tfhe.Circuit(2, [("OR", 0, 1)], [2])
        a = random_cts(rs, 2, op.n, op.q).reshape(2, 1, op.n + 1)
        assert np.array_equal(fresh.EvalCircuit(small, a)[0], orc.eval_bin_gate("OR", a[0], a[1]))
        inst = 205
        circ = tfhe.Circuit(10, [("NAND", 2 * g, 2 * g + 1) for g in range(5)], [10 + g for g in range(5)])
        assert circ.level_widths() == [5 * 1]
        cts = random_cts(rs, 10 * inst, op.n, op.q).reshape(10, inst, op.n + 1)
        got = fresh.EvalCircuit(circ, cts)
        x, y = cts[0::2].reshape(-1, op.n + 1), cts[1::2].reshape(-1, op.n + 1)  # the gathered operands, gate-major
        assert np.array_equal(got.reshape(-1, op.n + 1), fresh.EvalBinGate("NAND", x, y))
        idx = [0, 204, 205, 1024]
        assert np.array_equal(got.reshape(-1, op.n + 1)[idx], orc.eval_bin_gate("NAND", x[idx], y[idx]))
    finally:
        fresh.GPUClean()


def test_level_wider_than_the_device_chunk(shared_kat):
    """One gate, 65,539 instances: the level crosses max_chunk (65,536) and runs in two slices."""
    import tfhe_amd
    import torch

    s = shared_kat("STD128")
    cp, ctx, orc = s["cp"], s["ctx"], s["orc"]
    inst, w = 65536 + 3, cp.n + 1
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(9)
    d_in = torch.randint(0, cp.q, (2, inst, w), dtype=torch.int64, device=dev, generator=g)
    d_out = torch.zeros((1, inst, w), dtype=torch.int64, device=dev)
    d_ref = torch.zeros((inst, w), dtype=torch.int64, device=dev)
    circ = tfhe_amd.Circuit(2, [("NAND", 0, 1)], [2])
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalCircuitDevice(circ, inst, d_in.data_ptr(), d_out.data_ptr())
    ctx.EvalBinGateDevice("NAND", inst, d_in[0].data_ptr(), d_in[1].data_ptr(), d_ref.data_ptr())
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == 2 * inst
    assert torch.equal(d_out[0], d_ref)
    idx = [0, 65535, 65536, inst - 1]
    x, y = (d_in[k][idx].cpu().numpy().astype(np.uint64) for k in (0, 1))
    assert np.array_equal(d_out[0][idx].cpu().numpy().astype(np.uint64), orc.eval_bin_gate("NAND", x, y))


def test_reuse_of_plans_and_the_wire_store(toy, circuits, toy_all_ops):
    op, ctx = toy["op"], toy["ctx"]
    a, b = circuits["all_ops"], circuits["mixed"]
    cts_a, want_a = toy_all_ops["cts"], toy_all_ops["want"]
    cts_b = random_cts(np.random.default_rng(8), nets.MIXED_INPUTS * 3, op.n, op.q).reshape(nets.MIXED_INPUTS, 3, -1)
    want_b = nets.oracle_netlist(toy["orc"], nets.MIXED_INPUTS, nets.MIXED, nets.MIXED_OUTPUTS, cts_b, op.q)
    count = ctx.info().bootstraps
    for circ, cts, want in ((a, cts_a, want_a), (b, cts_b, want_b), (a, cts_a, want_a), (b, cts_b, want_b)):
        assert np.array_equal(run_device(ctx, circ, cts), want)
        count += circ.info()["bootstraps"] * 3
        assert ctx.info().bootstraps == count
    # fewer instances: another stride through the same (larger) wire store
    assert np.array_equal(run_device(ctx, a, cts_a[:, :2]), want_a[:, :2])
    assert np.array_equal(run_device(ctx, b, cts_b[:, 2:]), want_b[:, 2:])
    assert ctx.info().bootstraps == count + a.info()["bootstraps"] * 2 + b.info()["bootstraps"]


def test_trace_knob_reports_the_circuit_kernels(toy, circuits, toy_all_ops, capfd):
    """The trace knob times the preparation and output launches with event pairs (what tools/circuit_bench.py
    reads); the result does not change."""
    ctx, circ = toy["ctx"], circuits["all_ops"]
    capfd.readouterr()
    with ctx.knobs_set(trace=1):
        got = run_device(ctx, circ, toy_all_ops["cts"])
    err = capfd.readouterr().err
    assert np.array_equal(got, toy_all_ops["want"])
    assert "[tfhe] circuit: 14 bootstraps x 3 instances" in err and "9 prep launches" in err, err


def test_device_errors(toy, circuits):
    import torch

    op, ctx, tfhe, circ = toy["op"], toy["ctx"], toy["tfhe"], circuits["mixed"]
    L = tfhe.lib()
    w = op.n + 1
    d_in = torch.zeros((nets.MIXED_INPUTS, 1, w), dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros((len(nets.MIXED_OUTPUTS), 1, w), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def call(h, q, p_in, p_out):
        st = L.tfhe_eval_circuit_device(h, circ.handle, 1, C.c_void_p(p_in), q, C.c_void_p(p_out), None)
        return st, L.tfhe_last_error().decode()

    st, msg = call(ctx.handle, 1000, d_in.data_ptr(), d_out.data_ptr())  # 2N = 1024 for TOY
    assert st == 1 and "2N" in msg
    st, msg = call(ctx.handle, op.q, d_in.data_ptr(), None)
    assert st == 1 and "null" in msg
    # a context over two (logical) devices looks the output buffer up: host memory is on none of its devices
    os.environ["TFHE_LOGICAL_DEVICES"] = "2"
    try:
        multi = tfhe.BinFHEContextHIP(toy["cp"]).GPUSetup(*toy["keys"], num_gpus=2)
    finally:
        os.environ.pop("TFHE_LOGICAL_DEVICES", None)
    try:
        assert multi.info().num_devices == 2
        host = np.zeros((len(nets.MIXED_OUTPUTS), 1, w), dtype=np.uint64)
        st, msg = call(multi.handle, op.q, d_in.data_ptr(), host.ctypes.data)
        assert st == 1 and "device" in msg
        # and runs on the device that holds a real one
        cts = random_cts(np.random.default_rng(3), nets.MIXED_INPUTS, op.n, op.q).reshape(nets.MIXED_INPUTS, 1, w)
        assert np.array_equal(run_device(multi, circ, cts), run_device(ctx, circ, cts))
    finally:
        multi.GPUClean()
    torch.cuda.synchronize()
