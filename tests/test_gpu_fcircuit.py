"""GPU: function circuits in one call (tfhe_eval_fcircuit / tfhe_eval_fcircuit_device): every level of a compiled
netlist of linear forms and LUT bootstraps runs as one mixed batch -- one preparation launch that gathers each
record's folded form, applies its stage of EvalFunc and builds its own test vector, then ONE blind rotation at
a-modulus 2N for records at q and at 2q alike, one extraction, and the key switch once per output modulus.

The expected value is always the CPU oracle composed node by node in netlist order (fcircuit_nets.oracle_netlist:
numpy modular arithmetic for the linear forms, orc.eval_func for the LUT nodes), bit for bit; where stated, the
GPU's own EvalFuncDevice as well.
"""
import ctypes as C
import os

import numpy as np
import pytest

import fcircuit_nets as nets
from helpers import random_cts

pytestmark = pytest.mark.gpu

UNSUPPORTED = 2  # TFHE_ERR_UNSUPPORTED


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)).to(torch.device("cuda", 0))


def run_device(ctx, fc, cts, stream=None):
    """EvalFuncCircuitDevice on host arrays copied to cuda:0: cts[num_inputs, instances, n+1] -> numpy outputs."""
    import torch

    d_in = _dev(cts)
    inst, w = cts.shape[1], cts.shape[2]
    d_out = torch.zeros((fc.info()["num_outputs"], inst, w), dtype=torch.int64, device=d_in.device)
    torch.cuda.synchronize()
    ctx.EvalFuncCircuitDevice(fc, inst, d_in.data_ptr(), d_out.data_ptr(),
                              stream=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().astype(np.uint64)


@pytest.fixture(scope="module")
def toy(oracle):
    """A context of its own on the TOY logQ = 12 arbFunc parameters (n = 32, N = 2048, q = 2048) with valid keys."""
    import tfhe_amd

    op = oracle.params_from_logq("TOY", True, 12, 0, 0, 0)
    rng = oracle.Rng(41)
    sk, bsk, ksk = oracle.keygen(op, rng)
    cp = tfhe_amd.params_from_logq("TOY", True, 12, 0, 0, 0)
    ctx = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk)
    orc = oracle.Oracle(op, bsk, ksk)
    yield dict(op=op, cp=cp, ctx=ctx, orc=orc, sk=sk, rng=rng, keys=(bsk, ksk), tfhe=tfhe_amd, po=oracle)
    ctx.GPUClean()
    orc.close()


def compiled(net, q):
    import tfhe_amd

    ni, nodes, luts, outputs = net
    return tfhe_amd.FuncCircuit(ni, nodes, luts, outputs, q)


@pytest.fixture(scope="module")
def toy_adder(toy):
    """ADD4x3 on encrypted random digits, five instances: inputs, digits, the oracle composition (computed once)."""
    op, po = toy["op"], toy["po"]
    assert (op.n, op.N, op.q) == (32, 2048, 2048)
    net = nets.adder(3, op.q)
    digits = np.random.default_rng(6).integers(0, 4, (6, 5), dtype=np.uint64)
    cts = np.stack([np.stack([po.encrypt(op, toy["rng"], toy["sk"], int(m), 8, op.q) for m in row]) for row in digits])
    want = nets.oracle_netlist(toy["orc"], *net, op.q, cts)
    return dict(net=net, fc=compiled(net, op.q), digits=digits, cts=cts, want=want)


def test_adder_on_real_keys(toy, toy_adder):
    import torch

    op, po, ctx, fc = toy["op"], toy["po"], toy["ctx"], toy_adder["fc"]
    cts, want, digits = toy_adder["cts"], toy_adder["want"], toy_adder["digits"]
    assert fc.info()["bootstraps"] == 12
    before = ctx.info().bootstraps
    got = ctx.EvalFuncCircuit(fc, cts)
    assert ctx.info().bootstraps - before == 12 * 5
    assert got.shape == want.shape == (4, 5, op.n + 1)
    assert np.array_equal(got, want)
    dec = np.array([[po.decrypt(op, toy["sk"], ct, 8, op.q) for ct in row] for row in got], dtype=np.int64)
    x = sum(digits[d].astype(np.int64) << (2 * d) for d in range(3))
    y = sum(digits[3 + d].astype(np.int64) << (2 * d) for d in range(3))
    assert np.array_equal(dec, np.stack([(x + y) >> (2 * d) & 3 for d in range(4)]))  # zero wrong digits
    interval = np.uint64(op.q // 8)
    assert np.array_equal(dec.astype(np.uint64) * interval, fc.eval_plain(digits * interval))
    # the device form, on a caller's stream, equals the host form; one instance given as [num_inputs, n+1]
    assert np.array_equal(run_device(ctx, fc, cts, stream=torch.cuda.Stream(torch.device("cuda", 0))), got)
    assert np.array_equal(ctx.EvalFuncCircuit(fc, cts[:, 0]), got[:, 0])


@pytest.fixture(scope="module")
def all_classes_reference(shared_kat):
    """Per parameter set: random input ciphertexts of ALL_CLASSES, three instances, and the oracle composition."""
    cache = {}

    def get(name):
        if name not in cache:
            s = shared_kat(name)
            cp = s["cp"]
            net = nets.all_classes(cp.q)
            cts = np.stack([random_cts(np.random.default_rng(60 + i), 3, cp.n, cp.q) for i in range(net[0])])
            cache[name] = (compiled(net, cp.q), cts, nets.oracle_netlist(s["orc"], *net, cp.q, cts))
        return cache[name]

    return get


@pytest.mark.parametrize("name", ["STD128", "ARB12", "CHES18"])
def test_all_classes_on_the_production_kernels(shared_kat, all_classes_reference, name):
    """Negacyclic, periodic (both at q) and arbitrary (at 2q) records in one level, one blind rotation at
    a-modulus 2N: fast4 and its split form (STD128: q = N, so 2q = 2N), sf2 / sfduo (ARB12), three digits (CHES18)."""
    ctx = shared_kat(name)["ctx"]
    fc, cts, want = all_classes_reference(name)
    assert fc.level_widths() == nets.ALL_CLASSES_WIDTHS == [3, 3, 3, 2, 1]
    assert fc.info()["bootstraps"] == nets.ALL_CLASSES_BOOTSTRAPS == 12
    assert np.array_equal(ctx.EvalFuncCircuit(fc, cts), want)
    assert np.array_equal(ctx.EvalFuncCircuit(fc, cts[:, :1]), want[:, :1])
    with ctx.knobs_set(split4=0, duo=0):  # the one-workgroup forms of the same blind rotations
        assert np.array_equal(ctx.EvalFuncCircuit(fc, cts), want)
        assert np.array_equal(ctx.EvalFuncCircuit(fc, cts[:, :1]), want[:, :1])


def test_equals_the_vector_api_node_by_node(shared_kat):
    """ARB12, seven instances: EvalFuncDevice per LUT node with torch modular arithmetic in between."""
    import torch

    s = shared_kat("ARB12")
    cp, ctx = s["cp"], s["ctx"]
    q, w, inst = cp.q, cp.n + 1, 7
    ni, nodes, luts, outputs = net = nets.all_classes(q)
    fc = compiled(net, q)
    dev = torch.device("cuda", 0)
    d_in = torch.randint(0, q, (ni, inst, w), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    d_luts = _dev(luts)
    wires = [d_in[i] for i in range(ni)]
    for node in nodes:
        op, in0, in1, c0, c1, lut, k = nets.fields(node)
        v = c0 * wires[in0] + (c1 * wires[in1] if c1 else 0)
        v[:, -1] += k
        v = torch.remainder(v, q).contiguous()
        if op == "LUT":
            r = torch.empty_like(v)
            torch.cuda.synchronize()
            ctx.EvalFuncDevice(inst, v.data_ptr(), d_luts[lut].data_ptr(), r.data_ptr(), q=q)
            torch.cuda.synchronize()
            v = r
        wires.append(v)
    want = torch.stack([wires[o] for o in outputs])
    d_out = torch.zeros_like(want)
    torch.cuda.synchronize()
    ctx.EvalFuncCircuitDevice(fc, inst, d_in.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_out, want)


def test_arbitrary_tables_need_q_up_to_N(shared_kat):
    """LOGQ23: q = 4096 = 2N.  An arbitrary table would need modulus 2q: unsupported, nothing runs; negacyclic and
    periodic nodes run at q = 2N (mask scale 1)."""
    s = shared_kat("LOGQ23")
    cp, ctx, orc = s["cp"], s["ctx"], s["orc"]
    q = cp.q
    assert q > cp.N
    t = nets.tables(q)
    rs = np.random.default_rng(70)
    cts = np.stack([random_cts(rs, 2, cp.n, q) for _ in range(2)])
    arb = compiled((2, [("LUT", 0, (0, 1)), ("LUT", 1, (1, 1))], np.stack([t["neg1"], t["div4"]]), [2, 3]), q)
    before = ctx.info().bootstraps
    import tfhe_amd

    with pytest.raises(tfhe_amd.TfheError) as e:
        ctx.EvalFuncCircuit(arb, cts)
    assert e.value.status == UNSUPPORTED and "q <= N" in str(e.value)
    assert ctx.info().bootstraps == before
    net = (2, [("LUT", 0, (0, 1), (1, -1)), ("LUT", 1, (2, 1), (1, 2), q // 8), ("LIN", (3, 1), (2, 1)), ("LUT", 0, (4, 1))],
           np.stack([t["neg1"], t["mod4"]]), [2, 3, 5])
    fc = compiled(net, q)
    assert fc.level_widths() == [1, 1, 1, 1] and fc.info()["bootstraps"] == 4
    assert np.array_equal(ctx.EvalFuncCircuit(fc, cts), nets.oracle_netlist(orc, *net, q, cts))


def test_level_wider_than_the_device_chunk(shared_kat):
    """One arbitrary-class node, 65,539 instances on STD128: both of its levels cross max_chunk (65,536) and run in
    two slices, and its key switch ends at 2q."""
    import torch

    s = shared_kat("STD128")
    cp, ctx, orc = s["cp"], s["ctx"], s["orc"]
    q, inst, w = cp.q, 65536 + 3, cp.n + 1
    lut = nets.tables(q)["cube"]
    fc = compiled((1, [("LUT", 0, (0, 1))], lut[None, :], [1]), q)
    assert fc.level_widths() == [1, 1]
    dev = torch.device("cuda", 0)
    d_in = torch.randint(0, q, (1, inst, w), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(10))
    d_out = torch.zeros((1, inst, w), dtype=torch.int64, device=dev)
    d_ref = torch.zeros((inst, w), dtype=torch.int64, device=dev)
    d_lut = _dev(lut)
    torch.cuda.synchronize()
    before = ctx.info().bootstraps
    ctx.EvalFuncCircuitDevice(fc, inst, d_in.data_ptr(), d_out.data_ptr())
    ctx.EvalFuncDevice(inst, d_in[0].data_ptr(), d_lut.data_ptr(), d_ref.data_ptr())
    torch.cuda.synchronize()
    assert ctx.info().bootstraps - before == 4 * inst
    assert torch.equal(d_out[0], d_ref)
    idx = [0, 65535, inst - 1]
    x = d_in[0][idx].cpu().numpy().astype(np.uint64)
    assert np.array_equal(d_out[0][idx].cpu().numpy().astype(np.uint64), orc.eval_func(x, lut))


def test_reuse_growth_and_trace(toy, toy_adder, capfd):
    op, ctx, orc, tfhe = toy["op"], toy["ctx"], toy["orc"], toy["tfhe"]
    fc, cts, want = toy_adder["fc"], toy_adder["cts"], toy_adder["want"]
    net = nets.all_classes(op.q)
    other = compiled(net, op.q)
    cts_o = np.stack([random_cts(np.random.default_rng(80 + i), 2, op.n, op.q) for i in range(net[0])])
    want_o = nets.oracle_netlist(orc, *net, op.q, cts_o)
    count = ctx.info().bootstraps
    for c, x, y in ((fc, cts, want), (other, cts_o, want_o), (fc, cts, want), (other, cts_o, want_o)):
        assert np.array_equal(run_device(ctx, c, x), y)
        count += 12 * x.shape[1]
        assert ctx.info().bootstraps == count
    # fewer instances: another stride through the same (larger) wire store
    assert np.array_equal(run_device(ctx, fc, cts[:, 3:]), want[:, 3:])
    # a second context with the same keys, its wire store and scratch empty: small, then larger
    fresh = tfhe.BinFHEContextHIP(toy["cp"]).GPUSetup(*toy["keys"])
    try:
        assert np.array_equal(run_device(fresh, fc, cts[:, :1]), want[:, :1])
        assert np.array_equal(run_device(fresh, other, cts_o), want_o)
        assert np.array_equal(run_device(fresh, fc, cts), want)
    finally:
        fresh.GPUClean()
    # the trace knob prints the circuit line; the result does not change
    capfd.readouterr()
    with ctx.knobs_set(trace=1):
        got = run_device(ctx, fc, cts)
    err = capfd.readouterr().err
    assert np.array_equal(got, want)
    assert "[tfhe] circuit: 12 bootstraps x 5 instances" in err and "6 prep launches" in err, err


def test_device_errors(toy, toy_adder):
    import torch

    op, ctx, tfhe, fc = toy["op"], toy["ctx"], toy["tfhe"], toy_adder["fc"]
    L = tfhe.lib()
    w = op.n + 1
    d_in = torch.zeros((6, 1, w), dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros((4, 1, w), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    def call(h, circ, instances, p_in, p_out):
        st = L.tfhe_eval_fcircuit_device(h, circ.handle, instances, C.c_void_p(p_in), C.c_void_p(p_out), None)
        return st, L.tfhe_last_error().decode()

    wrong_q = compiled(nets.adder(3, 4 * op.N), 4 * op.N)  # 2N = 4096 here
    st, msg = call(ctx.handle, wrong_q, 1, d_in.data_ptr(), d_out.data_ptr())
    assert st == 1 and "2N" in msg
    st, msg = call(ctx.handle, fc, 1, d_in.data_ptr(), None)
    assert st == 1 and "null" in msg
    st, msg = call(ctx.handle, fc, 0, d_in.data_ptr(), d_out.data_ptr())
    assert st == 1 and "no instances" in msg
    st, msg = L.tfhe_eval_fcircuit_device(ctx.handle, None, 1, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), None), \
        L.tfhe_last_error().decode()
    assert st == 1 and "null" in msg
    # a context over two (logical) devices looks the output buffer up: host memory is on none of its devices
    os.environ["TFHE_LOGICAL_DEVICES"] = "2"
    try:
        multi = tfhe.BinFHEContextHIP(toy["cp"]).GPUSetup(*toy["keys"], num_gpus=2)
    finally:
        os.environ.pop("TFHE_LOGICAL_DEVICES", None)
    try:
        assert multi.info().num_devices == 2
        host = np.zeros((4, 1, w), dtype=np.uint64)
        st, msg = call(multi.handle, fc, 1, d_in.data_ptr(), host.ctypes.data)
        assert st == 1 and "device" in msg
        # and runs on the device that holds a real one
        assert np.array_equal(run_device(multi, fc, toy_adder["cts"][:, :1]), toy_adder["want"][:, :1])
    finally:
        multi.GPUClean()
    torch.cuda.synchronize()
