"""GPU: the tiled matrix product on device-resident buffers (tfhe_ciphertext_mul_matrix_device; mul_matrix.hip):
out[i][c] = sum_k matrix[k][c] ct[i][k] (+ bias[c] on the b word) mod m for `instances` input sets that share the
matrix.  Every word is compared against Python-integer arithmetic (tests/dense_model.product) at the kernel's tile
edges in K and cols, at every modulus class -- 2^k up to 2^32 (32-bit wrapping), 2^33 .. 2^63 (64-bit wrapping),
any other modulus (u128 sums; a modular add per term where K (m-1)^2 >= 2^128) -- and at the operands' extremes;
the inputs must come back untouched, and the call must order itself on the caller's stream."""
import numpy as np
import pytest

import dense_model

pytestmark = pytest.mark.gpu

MODULI = [1 << 12, 1 << 32, 1 << 33, 1 << 35, 1 << 63, (1 << 54) - 77823, (1 << 63) + 29, (1 << 64) - 59]
I64 = np.iinfo(np.int64)
U64MAX = np.iinfo(np.uint64).max


@pytest.fixture(scope="module")
def env(shared_kat):
    s = shared_kat("ARB12")  # the session's shared context (n = 1305: six blocks of 256 words, the last of 26)
    return s["op"], s["ctx"]


def _tiles():
    import tfhe_amd

    return tfhe_amd.mm_tiles()


def _dev(x):
    import torch

    x = np.ascontiguousarray(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _run(ctx, w, ct, mat, mod, bias=None, stream=0):
    """ct [instances][K][w], mat [K][cols] -> ([instances][cols][w] u64, the device tensors)"""
    import torch

    inst, K, cols = ct.shape[0], mat.shape[0], mat.shape[1]
    d_ct, d_m = _dev(ct), _dev(mat)
    d_b = _dev(bias) if bias is not None else None
    d_out = torch.full((inst, cols, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.CiphertextMulMatrixDevice(inst, K, d_ct.data_ptr(), cols, d_m.data_ptr(), mod, d_out.data_ptr(),
                                  d_bias=d_b.data_ptr() if d_b is not None else 0, stream=stream)
    torch.cuda.synchronize()
    return _host(d_out), (d_ct, d_m, d_b)


def _inputs(seed, inst, K, cols, w, mod):
    rs = np.random.default_rng(seed)
    ct = rs.integers(0, mod, (inst, K, w), dtype=np.uint64)
    mat = rs.integers(I64.min, I64.max, (K, cols), dtype=np.int64, endpoint=True)
    bias = rs.integers(0, mod, cols, dtype=np.uint64)
    return ct, mat, bias


# tile-edge sizes as functions of the kernel's tile (read from mm_tiles() when the test runs)
EDGES = {"1": lambda t: 1, "T-1": lambda t: t - 1, "T": lambda t: t, "T+1": lambda t: t + 1}
K_EDGES = dict(EDGES, **{"2T+3": lambda t: 2 * t + 3})
C_EDGES = dict(EDGES, **{"2T+1": lambda t: 2 * t + 1})
TILE_CASES = [(k, c, inst, 1 << 35) for k in K_EDGES for c in C_EDGES for inst in (1, 3)]  # every shape at 2^35
TILE_CASES += [("T+1", "T+1", inst, m) for m in MODULI if m != 1 << 35 for inst in (1, 3)]  # every modulus, +1 tails


@pytest.mark.parametrize("tile_case", TILE_CASES, ids=[f"K={k}-cols={c}-i{i}-m{m:#x}" for k, c, i, m in TILE_CASES])
def test_tile_edges(env, tile_case):
    op, ctx = env
    kt, ctl, _ = _tiles()
    K, cols, inst, mod = K_EDGES[tile_case[0]](kt), C_EDGES[tile_case[1]](ctl), tile_case[2], tile_case[3]
    w = op.n + 1
    ct, mat, bias = _inputs(K * 1000 + cols * 10 + inst, inst, K, cols, w, mod)
    got, _ = _run(ctx, w, ct, mat, mod, bias)
    assert np.array_equal(got, dense_model.product(ct, mat, mod, bias))


@pytest.mark.parametrize("mod", [1 << 12, 1 << 35, (1 << 54) - 77823, (1 << 63) + 29, (1 << 64) - 59],
                         ids=lambda m: f"{m:#x}")
def test_operand_edges(env, mod):
    """tests/test_gpu_mul_matrix.py::test_extreme_entries through the device form: columns of INT64_MIN, INT64_MAX
    and -1, a ciphertext row of 2^64 - 1 (an unreduced input), a bias entry >= modulus."""
    op, ctx = env
    w = op.n + 1
    rs = np.random.default_rng(10)
    K, cols = 9, 4
    ct = rs.integers(0, U64MAX, (2, K, w), dtype=np.uint64, endpoint=True)
    ct[0, 0, :] = U64MAX
    ct[1, K - 1, :] = U64MAX
    mat = rs.integers(I64.min, I64.max, (K, cols), dtype=np.int64, endpoint=True)
    mat[:, 0] = I64.min
    mat[:, 1] = I64.max
    mat[:, 2] = -1
    bias = np.array([mod - 1, mod, min(mod + 12345, int(U64MAX)), U64MAX], dtype=np.uint64)
    got, _ = _run(ctx, w, ct, mat, mod, bias)
    assert np.array_equal(got, dense_model.product(ct, mat, mod, bias))


@pytest.mark.parametrize("mod", [1 << 12, 1 << 35, (1 << 54) - 77823, (1 << 64) - 59], ids=lambda m: f"{m:#x}")
def test_inputs_untouched(env, mod):
    """d_ct, d_matrix and d_bias are bit-identical before and after, on every instance of the kernel -- with
    operands the pre-pass and the loads reduce (negative entries, words and bias above the modulus)."""
    import torch

    op, ctx = env
    w = op.n + 1
    kt, ctl, _ = _tiles()
    rs = np.random.default_rng(13)
    K, cols = kt + 1, ctl + 1
    ct = rs.integers(0, U64MAX, (2, K, w), dtype=np.uint64, endpoint=True)
    mat = rs.integers(I64.min, I64.max, (K, cols), dtype=np.int64, endpoint=True)
    bias = rs.integers(0, U64MAX, cols, dtype=np.uint64, endpoint=True)
    d_ct, d_m, d_b = _dev(ct), _dev(mat), _dev(bias)
    keep = [t.clone() for t in (d_ct, d_m, d_b)]
    d_out = torch.empty((2, cols, w), dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.CiphertextMulMatrixDevice(2, K, d_ct.data_ptr(), cols, d_m.data_ptr(), mod, d_out.data_ptr(),
                                  d_bias=d_b.data_ptr())
    torch.cuda.synchronize()
    for before, after in zip(keep, (d_ct, d_m, d_b)):
        assert torch.equal(before, after)
    assert np.array_equal(_host(d_out), dense_model.product(ct, mat, mod, bias))


def test_each_instance_equals_the_host_call(env):
    """Instance i of a 3-instance call equals the host CiphertextMulMatrix on instance i alone."""
    op, ctx = env
    w = op.n + 1
    ct, mat, _ = _inputs(14, 3, 37, 19, w, op.qKS)
    got, _ = _run(ctx, w, ct, mat, op.qKS)
    for i in range(3):
        assert np.array_equal(got[i], ctx.CiphertextMulMatrix(ct[i], mat, op.qKS)), i


def test_reference_fixture(env):
    """GEMM.cpp's configuration through the device form equals the reference's recorded output."""
    import refvec

    op, ctx = env
    data = refvec.load()
    c = refvec.case("mm_gemm", data)
    x = refvec.inputs(c, data["fixtures"])
    got, _ = _run(ctx, op.n + 1, x["in"][None], x["matrix"], c["args"]["modulus"])
    refvec.check(c, got.ravel(), {})


def test_stream_ordering(env):
    """A call on a non-default stream, then a dependent copy on the same stream with no synchronise in between."""
    import torch

    op, ctx = env
    w = op.n + 1
    ct, mat, bias = _inputs(15, 2, 40, 20, w, op.qKS)
    d_ct, d_m, d_b = _dev(ct), _dev(mat), _dev(bias)
    d_out = torch.full((2, 20, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(d_ct.device)
    ctx.CiphertextMulMatrixDevice(2, 40, d_ct.data_ptr(), 20, d_m.data_ptr(), op.qKS, d_out.data_ptr(),
                                  d_bias=d_b.data_ptr(), stream=s.cuda_stream)
    with torch.cuda.stream(s):
        copy = d_out.clone()
    s.synchronize()
    assert np.array_equal(_host(copy), dense_model.product(ct, mat, op.qKS, bias))


def test_errors_then_a_valid_call(env):
    import tfhe_amd as capi

    op, ctx = env
    w = op.n + 1
    ct, mat, _ = _inputs(16, 1, 3, 2, w, 1 << 12)
    d_ct, d_m, d_out = _dev(ct), _dev(mat), _dev(np.zeros((1, 2, w), dtype=np.uint64))
    P = (d_ct.data_ptr(), d_m.data_ptr(), d_out.data_ptr())
    bad = [
        dict(ct=0), dict(m=0), dict(out=0),                 # null pointers
        dict(inst=0), dict(K=0), dict(cols=0),              # zero sizes
        dict(mod=0),
        dict(inst=1 << 62), dict(K=1 << 62, cols=1 << 3),   # size products beyond size_t
    ]
    for b in bad:
        a = dict(inst=1, K=3, cols=2, ct=P[0], m=P[1], out=P[2], mod=1 << 12)
        a.update(b)
        with pytest.raises(capi.TfheError) as e:
            ctx.CiphertextMulMatrixDevice(a["inst"], a["K"], a["ct"], a["cols"], a["m"], a["mod"], a["out"])
        assert e.value.status == 1, b  # TFHE_ERR_INVALID_ARGUMENT
    got, _ = _run(ctx, w, ct, mat, 1 << 12)
    assert np.array_equal(got, dense_model.product(ct, mat, 1 << 12))
