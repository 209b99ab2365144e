"""GPU: Conv2d on device-resident ciphertexts with the gather inside the kernel (tfhe_ciphertext_conv2d_device;
conv2d.hip).  Every word is compared against the model of tests/conv_model.py (im2col in numpy, then Python-integer
arithmetic) at the kernel's tile edges in K, output planes per group and output positions, at every modulus class,
on shapes where nothing is square, with groups, and at the operands' extremes; against the composition a user had to
write before (a torch gather into an im2col buffer, CiphertextMulMatrixDevice, a permute); the inputs must come back
untouched, nothing may be written past the output, and the call must order itself on the caller's stream."""
import numpy as np
import pytest

import conv_model

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
U64MAX = np.iinfo(np.uint64).max
MODULI = [1 << 12, 1 << 32, 1 << 33, 1 << 63, (1 << 54) - 77823, (1 << 63) + 29, (1 << 64) - 59]


@pytest.fixture(scope="module")
def env(shared_kat):
    s = shared_kat("ARB12")  # the session's shared context (n = 1305: six blocks of 256 words, the last of 26)
    return s["op"], s["ctx"]


def _tiles():
    import tfhe_amd

    return tfhe_amd.conv2d_tiles()


def _dev(x):
    import torch

    x = np.ascontiguousarray(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _out_shape(d, inst, w):
    oh, ow, _ = conv_model.shape(d)
    return (inst, d.c_out, oh, ow, w)


def _run(ctx, w, d, ct, wt, mod, bias=None, stream=0):
    """ct [instances][c_in][h][w][w] -> ([instances][c_out][oh][ow][w] u64, the device tensors).  The output is
    pre-filled with -1 and followed by a guard row that must stay -1."""
    import torch

    import tfhe_amd

    shape = _out_shape(d, ct.shape[0], w)
    words = int(np.prod(shape))
    d_ct, d_w = _dev(ct), _dev(wt)
    d_b = _dev(bias) if bias is not None else None
    d_out = torch.full((words + w,), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    ctx.CiphertextConv2dDevice(tfhe_amd.Conv2d(*d), ct.shape[0], d_ct.data_ptr(), d_w.data_ptr(), mod, d_out.data_ptr(),
                               d_bias=d_b.data_ptr() if d_b is not None else 0, stream=stream)
    torch.cuda.synchronize()
    assert bool((d_out[words:] == -1).all()), "the guard row behind the output was written"
    return _host(d_out[:words]).reshape(shape), (d_ct, d_w, d_b)


def _inputs(seed, d, inst, w, mod, wide=False):
    """Ciphertexts below the modulus; weights over all of int64 (`wide`: the model then sums Python integers) or
    within 2^20 (K <= 127 at a modulus up to 2^35: every sum fits int64)."""
    rs = np.random.default_rng(seed)
    ct = rs.integers(0, mod, (inst, d.c_in, d.h, d.w, w), dtype=np.uint64)
    lo, hi = (I64.min, I64.max) if wide else (-(1 << 20), 1 << 20)
    wt = rs.integers(lo, hi, (d.c_out, d.c_in // d.groups, d.kh, d.kw), dtype=np.int64, endpoint=True)
    bias = rs.integers(0, mod, d.c_out, dtype=np.uint64)
    return ct, wt, bias


def _compose_on_device(ctx, w, d, d_ct, d_w, mod, d_b):
    """What a user had to do before: a torch gather into an im2col buffer [instances oh ow][K][w] per group,
    CiphertextMulMatrixDevice, and a permute to plane-major order."""
    import torch

    oh, ow, K = conv_model.shape(d)
    inst, Og, Cg = d_ct.shape[0], d.c_out // d.groups, d.c_in // d.groups
    xp = torch.nn.functional.pad(d_ct, (0, 0, d.pad_w, d.pad_w, d.pad_h, d.pad_h))
    win = xp.unfold(2, d.kh, d.stride_h).unfold(3, d.kw, d.stride_w)  # [inst, c_in, oh, ow, w, kh, kw]
    assert win.shape[2:4] == (oh, ow)
    out = torch.empty((inst, d.c_out, oh * ow, w), dtype=torch.int64, device=d_ct.device)
    for g in range(d.groups):
        cols = win[:, g * Cg:(g + 1) * Cg].permute(0, 2, 3, 1, 5, 6, 4).reshape(inst * oh * ow, K, w).contiguous()
        mat = d_w[g * Og:(g + 1) * Og].reshape(Og, K).t().contiguous()
        z = torch.empty((inst * oh * ow, Og, w), dtype=torch.int64, device=d_ct.device)
        torch.cuda.synchronize()
        ctx.CiphertextMulMatrixDevice(inst * oh * ow, K, cols.data_ptr(), Og, mat.data_ptr(), mod, z.data_ptr(),
                                      d_bias=d_b[g * Og:].data_ptr() if d_b is not None else 0)
        torch.cuda.synchronize()
        out[:, g * Og:(g + 1) * Og] = z.reshape(inst, oh * ow, Og, w).permute(0, 2, 1, 3)
    return _host(out).reshape(inst, d.c_out, oh, ow, w)


def _check(ctx, w, d, inst, mod, seed, wide=False, compose=False):
    ct, wt, bias = _inputs(seed, d, inst, w, mod, wide)
    got, (d_ct, d_w, d_b) = _run(ctx, w, d, ct, wt, mod, bias)
    assert np.array_equal(got, conv_model.conv2d(ct, wt, mod, d, bias))
    if compose:
        assert np.array_equal(got, _compose_on_device(ctx, w, d, d_ct, d_w, mod, d_b))


# tile-edge sizes as functions of the kernel's tile (read from conv2d_tiles() when the test runs)
EDGES = {"1": lambda t: 1, "T-1": lambda t: max(t - 1, 1), "T": lambda t: t, "T+1": lambda t: t + 1}
K_EDGES = dict(EDGES, **{"2T+3": lambda t: 2 * t + 3})
C_EDGES = dict(EDGES, **{"2T+1": lambda t: 2 * t + 1})
P_EDGES = dict(EDGES, **{"2T+1": lambda t: 2 * t + 1})
# K x planes at P + 1 positions and three instances; the positions at the +1 tails for both instance counts
SWEEP = [(k, c, "T+1", 3) for k in K_EDGES for c in C_EDGES]
SWEEP += [("T+1", "T+1", p, inst) for p in P_EDGES for inst in (1, 3) if (p, inst) != ("T+1", 3)]
SWEEP += [("1", "1", "1", 1)]


@pytest.mark.parametrize("case", SWEEP, ids=[f"K={k}-planes={c}-pos={p}-i{i}" for k, c, p, i in SWEEP])
def test_tile_edges_through_planes(env, case):
    """K reached through c_in with a 1 x 1 window (h = 1, w = positions), at 2^35."""
    op, ctx = env
    kt, ctl, _, pt = _tiles()
    K, planes, npos, inst = K_EDGES[case[0]](kt), C_EDGES[case[1]](ctl), P_EDGES[case[2]](pt), case[3]
    d = conv_model.desc(K, 1, npos, planes, 1, 1)
    _check(ctx, op.n + 1, d, inst, 1 << 35, K * 1000 + planes * 10 + npos)


@pytest.mark.parametrize("edge", list(K_EDGES))
def test_tile_edges_through_a_window(env, edge):
    """K reached through a 3 x 2 window: K = 6 c_in, so the edge is met from both sides by the multiples of 6 below
    and above it (K = 1 by c_in = 1: 6).  4 x 3 planes with padding (1, 0): 4 x 2 positions, padded taps in the
    first and last row of windows; planes per group = CT + 1."""
    op, ctx = env
    kt, ctl, _, _ = _tiles()
    target = K_EDGES[edge](kt)
    for c_in in sorted({max(target // 6, 1), -(-target // 6)}):
        d = conv_model.desc(c_in, 4, 3, ctl + 1, 3, 2, padding=(1, 0))
        assert conv_model.shape(d) == (4, 2, 6 * c_in)
        _check(ctx, op.n + 1, d, 2, 1 << 35, 7000 + c_in)


@pytest.mark.parametrize("inst", [1, 3])
@pytest.mark.parametrize("mod", MODULI, ids=lambda m: f"{m:#x}")
def test_every_modulus_at_the_tails(env, mod, inst):
    """K = KT + 1, CT + 1 planes, P + 1 positions at every modulus class (2^63 + 29 and 2^64 - 59 take GEN_TERM), with
    weights over all of int64."""
    op, ctx = env
    kt, ctl, _, pt = _tiles()
    d = conv_model.desc(kt + 1, 1, pt + 1, ctl + 1, 1, 1)
    _check(ctx, op.n + 1, d, inst, mod, 8000 + inst, wide=True)


NON_SQUARE = {
    # h = 5, w = 4, window 3 x 2, stride (2, 1), padding (1, 1): swapped axes would show; (5 + 2 - 3) % 2 == 0
    "swapped-axes": conv_model.desc(3, 5, 4, 5, 3, 2, stride=(2, 1), padding=(1, 1)),
    # padding (kh - 1, kw - 1): the corner windows hold a single real tap
    "full-padding": conv_model.desc(2, 3, 4, 3, 3, 2, padding=(2, 1)),
    # stride larger than the window: pixels no window reads
    "stride-beyond-window": conv_model.desc(2, 7, 9, 3, 2, 2, stride=(3, 4)),
    # (h + 2p - kh) % stride != 0 in both axes: (6 + 2 - 3) % 2 = 1, (7 + 0 - 2) % 3 = 2
    "inexact-division": conv_model.desc(2, 6, 7, 3, 3, 2, stride=(2, 3), padding=(1, 0)),
}


@pytest.mark.parametrize("name", list(NON_SQUARE))
@pytest.mark.parametrize("mod", [1 << 35, (1 << 54) - 77823], ids=lambda m: f"{m:#x}")
def test_non_square_everything(env, mod, name):
    op, ctx = env
    _check(ctx, op.n + 1, NON_SQUARE[name], 2, mod, 9000 + len(name), compose=True)


@pytest.mark.parametrize("groups", [1, 2, 4], ids=lambda g: f"groups={g}")
def test_groups(env, groups):
    """groups = 1, 2 and c_in (depthwise) with CT + 1 planes per group: a tile tail sits inside every group and must
    not spill into the next one.  Compared with the model and with the per-group composition on the device."""
    op, ctx = env
    ctl = _tiles()[1]
    d = conv_model.desc(4, 4, 3, groups * (ctl + 1), 2, 2, padding=(1, 0), groups=groups)
    _check(ctx, op.n + 1, d, 2, 1 << 35, 9100 + groups, compose=True)
    _check(ctx, op.n + 1, d, 2, (1 << 64) - 59, 9200 + groups, wide=True)


def test_one_by_one_window_equals_the_dense_product(env):
    """A 1 x 1 window, stride 1, no padding, groups = 1 is CiphertextMulMatrixDevice on the transposed layout."""
    import torch

    op, ctx = env
    w, mod = op.n + 1, op.qKS
    d = conv_model.desc(37, 3, 2, 19, 1, 1)
    ct, wt, bias = _inputs(9300, d, 2, w, mod)
    got, (d_ct, d_w, d_b) = _run(ctx, w, d, ct, wt, mod, bias)
    x = d_ct.permute(0, 2, 3, 1, 4).reshape(2 * 6, 37, w).contiguous()  # [instances h w][c_in][w]
    mat = d_w.reshape(19, 37).t().contiguous()
    z = torch.empty((2 * 6, 19, w), dtype=torch.int64, device=x.device)
    torch.cuda.synchronize()
    ctx.CiphertextMulMatrixDevice(2 * 6, 37, x.data_ptr(), 19, mat.data_ptr(), mod, z.data_ptr(), d_bias=d_b.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(got.reshape(2, 19, 6, w), _host(z.reshape(2, 6, 19, w).permute(0, 2, 1, 3).contiguous()))


@pytest.mark.parametrize("mod", [1 << 12, 1 << 35, (1 << 54) - 77823, (1 << 63) + 29, (1 << 64) - 59],
                         ids=lambda m: f"{m:#x}")
def test_operand_edges(env, mod):
    """Planes of INT64_MIN, INT64_MAX and -1 weights, ciphertext planes of 2^64 - 1 (unreduced inputs), bias entries
    >= modulus, with padding and two groups."""
    op, ctx = env
    w = op.n + 1
    d = conv_model.desc(4, 3, 3, 4, 2, 2, padding=(1, 1), groups=2)
    rs = np.random.default_rng(9400)
    ct = rs.integers(0, U64MAX, (2, 4, 3, 3, w), dtype=np.uint64, endpoint=True)
    ct[0, 0] = U64MAX
    ct[1, 3] = U64MAX
    wt = rs.integers(I64.min, I64.max, (4, 2, 2, 2), dtype=np.int64, endpoint=True)
    wt[0], wt[1], wt[2] = I64.min, I64.max, -1
    bias = np.array([mod - 1, mod, min(mod + 12345, int(U64MAX)), U64MAX], dtype=np.uint64)
    got, _ = _run(ctx, w, d, ct, wt, mod, bias)
    assert np.array_equal(got, conv_model.conv2d(ct, wt, mod, d, bias))


@pytest.mark.parametrize("mod", [1 << 12, 1 << 35, (1 << 54) - 77823, (1 << 64) - 59], ids=lambda m: f"{m:#x}")
def test_inputs_untouched(env, mod):
    """d_ct, d_weight and d_bias are bit-identical before and after, on every instance of the kernel -- with operands
    the pre-pass and the loads reduce (negative weights, words and bias above the modulus)."""
    op, ctx = env
    w = op.n + 1
    d = conv_model.desc(3, 3, 4, 3, 2, 3, padding=(1, 2))
    rs = np.random.default_rng(9500)
    ct = rs.integers(0, U64MAX, (2, 3, 3, 4, w), dtype=np.uint64, endpoint=True)
    wt = rs.integers(I64.min, I64.max, (3, 3, 2, 3), dtype=np.int64, endpoint=True)
    bias = rs.integers(0, U64MAX, 3, dtype=np.uint64, endpoint=True)
    got, tensors = _run(ctx, w, d, ct, wt, mod, bias)
    for before, after in zip((ct, wt.view(np.uint64), bias), tensors):
        assert np.array_equal(before, _host(after))
    assert np.array_equal(got, conv_model.conv2d(ct, wt, mod, d, bias))


def test_stream_ordering(env):
    """A call on a non-default stream, then a dependent copy on the same stream with no synchronise in between."""
    import torch

    import tfhe_amd

    op, ctx = env
    w = op.n + 1
    d = conv_model.desc(5, 6, 5, 20, 3, 3, padding=(1, 1))
    ct, wt, bias = _inputs(9600, d, 2, w, op.qKS)
    d_ct, d_w, d_b = _dev(ct), _dev(wt), _dev(bias)
    d_out = torch.full(_out_shape(d, 2, w), -1, dtype=torch.int64, device=d_ct.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(d_ct.device)
    ctx.CiphertextConv2dDevice(tfhe_amd.Conv2d(*d), 2, d_ct.data_ptr(), d_w.data_ptr(), op.qKS, d_out.data_ptr(),
                               d_bias=d_b.data_ptr(), stream=s.cuda_stream)
    with torch.cuda.stream(s):
        copy = d_out.clone()
    s.synchronize()
    assert np.array_equal(_host(copy), conv_model.conv2d(ct, wt, op.qKS, d, bias))


def test_errors_then_a_valid_call(env):
    import tfhe_amd

    op, ctx = env
    w = op.n + 1
    good = conv_model.desc(4, 5, 4, 6, 3, 2, stride=(2, 1), padding=(1, 1), groups=2)
    ct, wt, _ = _inputs(9700, good, 1, w, 1 << 12)
    d_ct, d_w, d_out = _dev(ct), _dev(wt), _dev(np.zeros(_out_shape(good, 1, w), dtype=np.uint64))
    bad = [
        (dict(ct=0), "ct"), (dict(wt=0), "weight"), (dict(out=0), "out"),       # null pointers
        (dict(inst=0), "instances"), (dict(mod=0), "modulus"),
        (dict(inst=1 << 62), "overflow"), (dict(desc=dict(c_in=1 << 31, c_out=1 << 31, groups=1 << 31, h=1 << 31)), "overflow"),
    ]
    bad += [(dict(desc={f: 0}), f) for f in good._fields if not f.startswith("pad")]
    bad += [(dict(desc=dict(c_in=3)), "c_in"), (dict(desc=dict(c_out=5)), "c_out"), (dict(desc=dict(pad_h=3)), "pad_h"),
            (dict(desc=dict(pad_w=2)), "pad_w"), (dict(desc=dict(h=1, kh=4, pad_h=1)), "kh"),
            (dict(desc=dict(w=1, kw=4, pad_w=1)), "kw")]
    for change, word in bad:
        a = dict(inst=1, ct=d_ct.data_ptr(), wt=d_w.data_ptr(), out=d_out.data_ptr(), mod=1 << 12, desc={})
        a.update(change)
        desc = tfhe_amd.Conv2d(*good._replace(**a["desc"]))
        with pytest.raises(tfhe_amd.TfheError) as e:
            ctx.CiphertextConv2dDevice(desc, a["inst"], a["ct"], a["wt"], a["mod"], a["out"])
        assert e.value.status == 1, change  # TFHE_ERR_INVALID_ARGUMENT
        assert word in str(e.value), (change, str(e.value))
    got, _ = _run(ctx, w, good, ct, wt, 1 << 12)
    assert np.array_equal(got, conv_model.conv2d(ct, wt, 1 << 12, good))
