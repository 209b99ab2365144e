"""CPU: the convolution model (tests/conv_model.py) that the GPU tests compare against, checked on its own -- against
sums of Python integers written out as six nested loops, against torch's float64 conv2d on small clear integers, and
by decryption through the oracle -- and the host-only calls of the library: tfhe_conv2d_shape and
tfhe_conv2d_tiles, which need no GPU."""
import itertools

import numpy as np
import pytest

import conv_model
from helpers import cube_lut

I64 = np.iinfo(np.int64)
U64MAX = np.iinfo(np.uint64).max


@pytest.mark.parametrize("mod", [1 << 12, (1 << 54) - 77823, (1 << 63) + 29, (1 << 64) - 59], ids=lambda m: f"{m:#x}")
def test_model_equals_python_integers(mod):
    """INT64_MIN / INT64_MAX weights, unreduced ciphertext words, a bias >= modulus, on a non-square shape with
    stride (2, 1), padding (1, 1) and two groups: every word against the definition, six nested loops."""
    rs = np.random.default_rng(41)
    d = conv_model.desc(4, 5, 4, 6, 3, 2, stride=(2, 1), padding=(1, 1), groups=2)
    oh, ow, K = conv_model.shape(d)
    assert (oh, ow, K) == (3, 5, 12)
    inst, width, Cg, Og = 2, 5, 2, 3
    ct = rs.integers(0, U64MAX, (inst, d.c_in, d.h, d.w, width), dtype=np.uint64, endpoint=True)
    ct[0, 0] = U64MAX
    wt = rs.integers(I64.min, I64.max, (d.c_out, Cg, d.kh, d.kw), dtype=np.int64, endpoint=True)
    wt[0], wt[1], wt[5] = I64.min, I64.max, -1
    bias = np.array([0, mod - 1, min(mod + 5, int(U64MAX)), U64MAX, 1, 2], dtype=np.uint64)
    got = conv_model.conv2d(ct, wt, mod, d, bias)
    assert got.shape == (inst, d.c_out, oh, ow, width) and got.dtype == np.uint64
    for i, o, oy, ox, j in itertools.product(range(inst), range(d.c_out), range(oh), range(ow), range(width)):
        g = o // Og
        want = int(bias[o]) if j == width - 1 else 0
        for ic in range(Cg):
            for ky in range(d.kh):
                for kx in range(d.kw):
                    iy, ix = oy * d.stride_h - d.pad_h + ky, ox * d.stride_w - d.pad_w + kx
                    if 0 <= iy < d.h and 0 <= ix < d.w:
                        want += int(wt[o, ic, ky, kx]) * int(ct[i, g * Cg + ic, iy, ix, j])
        assert int(got[i, o, oy, ox, j]) == want % mod, (i, o, oy, ox, j)
    # one instance keeps its shape; no bias is a zero bias
    assert np.array_equal(conv_model.conv2d(ct[0], wt, mod, d, bias), got[0])
    assert np.array_equal(conv_model.conv2d(ct, wt, mod, d), conv_model.conv2d(ct, wt, mod, d, np.zeros(6, np.uint64)))


@pytest.mark.parametrize("groups", [1, 2, 4], ids=lambda g: f"groups={g}")
@pytest.mark.parametrize("padding", [(0, 0), (1, 0), "full"], ids=str)
@pytest.mark.parametrize("stride", [(1, 1), (2, 1), (3, 2)], ids=str)
def test_model_equals_torch_conv2d_on_clear_integers(stride, padding, groups):
    """Small clear integers (|sums| far below 2^53) through the model at a modulus above every sum, against
    torch.nn.functional.conv2d in float64 on the CPU, which is exact there.  groups = C is depthwise."""
    import torch

    C, h, w, kh, kw, c_out = 4, 7, 6, 3, 2, 8
    pad = (kh - 1, kw - 1) if padding == "full" else padding
    d = conv_model.desc(C, h, w, c_out, kh, kw, stride=stride, padding=pad, groups=groups)
    rs = np.random.default_rng(42)
    x = rs.integers(0, 100, (2, C, h, w), dtype=np.int64)
    wt = rs.integers(-50, 50, (c_out, C // groups, kh, kw), dtype=np.int64)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), stride=stride,
                                     padding=pad, groups=groups).numpy()
    mod = 1 << 40
    got = conv_model.conv2d(x.astype(np.uint64)[..., None], wt, mod, d)[..., 0]
    assert got.shape == ref.shape == (2, c_out) + conv_model.shape(d)[:2]
    assert np.array_equal(got, ref.astype(np.int64) % mod)


def test_conv2d_shape_sweep_without_a_gpu():
    """tfhe_conv2d_shape from the library alone against the model's shape, over small descriptors -- among them
    (h + 2p - kh) % stride != 0, where the last rows are read by no window."""
    import tfhe_amd

    tfhe_amd.build()
    _lib_desc = lambda d: tfhe_amd.Conv2d(*d)
    inexact = 0
    for h, w, kh, kw, sh, sw, ph, pw in itertools.product((3, 5, 6), (4, 7), (1, 2, 3), (1, 2), (1, 2, 3), (1, 2),
                                                          (0, 1, 2), (0, 1)):
        if ph >= kh or pw >= kw or kh > h + 2 * ph or kw > w + 2 * pw:
            continue
        for c_in, c_out, groups in ((1, 1, 1), (4, 6, 2), (3, 3, 3)):
            d = conv_model.desc(c_in, h, w, c_out, kh, kw, stride=(sh, sw), padding=(ph, pw), groups=groups)
            assert tfhe_amd.conv2d_shape(_lib_desc(d)) == conv_model.shape(d), d
            inexact += (h + 2 * ph - kh) % sh != 0
    assert inexact > 0
    # stride beyond the window, and the extremes of one field
    assert tfhe_amd.conv2d_shape(_lib_desc(conv_model.desc(1, 9, 9, 1, 2, 2, stride=(4, 5)))) == (2, 2, 4)
    assert tfhe_amd.conv2d_shape(_lib_desc(conv_model.desc(1, 2**32 - 1, 1, 1, 1, 1))) == (2**32 - 1, 1, 1)


GOOD = dict(c_in=4, h=5, w=4, c_out=6, kh=3, kw=2, stride_h=2, stride_w=1, pad_h=1, pad_w=1, groups=2)
BAD_DESCRIPTORS = [(dict({f: 0}), f) for f in ("c_in", "h", "w", "c_out", "kh", "kw", "stride_h", "stride_w", "groups")]
BAD_DESCRIPTORS += [
    (dict(c_in=3), "c_in"), (dict(c_out=5), "c_out"),      # groups divides neither
    (dict(pad_h=3), "pad_h"), (dict(pad_w=2), "pad_w"),    # pad >= window
    (dict(h=1, kh=4, pad_h=1), "kh"), (dict(w=1, kw=4, pad_w=1), "kw"),  # window beyond the padded plane
]


@pytest.mark.parametrize("change,field", BAD_DESCRIPTORS, ids=[f"{c}" for c, _ in BAD_DESCRIPTORS])
def test_conv2d_shape_argument_errors(change, field):
    """Every descriptor error by status (TFHE_ERR_INVALID_ARGUMENT) and by a message that names the field."""
    import tfhe_amd

    tfhe_amd.build()
    assert tfhe_amd.conv2d_shape(tfhe_amd.Conv2d(**GOOD)) == (3, 5, 12)
    with pytest.raises(tfhe_amd.TfheError) as e:
        tfhe_amd.conv2d_shape(tfhe_amd.Conv2d(**dict(GOOD, **change)))
    assert e.value.status == 1
    assert field in str(e.value), str(e.value)


def test_conv2d_shape_null_arguments():
    """A null descriptor is an argument error; null result pointers are allowed."""
    import ctypes as C

    import tfhe_amd

    tfhe_amd.build()
    L = tfhe_amd.lib()
    assert L.tfhe_conv2d_shape(None, None, None, None) == 1
    assert b"descriptor" in L.tfhe_last_error()
    d = tfhe_amd.Conv2d(**GOOD)
    assert L.tfhe_conv2d_shape(C.byref(d), None, None, None) == 0
    K = C.c_size_t()
    assert L.tfhe_conv2d_shape(C.byref(d), None, None, C.byref(K)) == 0 and K.value == 12


def test_conv2d_tiles_without_a_gpu():
    """tfhe_conv2d_tiles: the kernel's tile sizes, from the library alone."""
    import tfhe_amd

    tfhe_amd.build()
    kt, ct, threads, positions = tfhe_amd.conv2d_tiles()
    assert kt > 0 and ct > 0 and threads > 0 and positions > 0
    assert threads % 64 == 0


def test_decrypting_layer_on_the_oracle(oracle):
    """conv_model.CONV_DECRYPT_CASE on the oracle alone: keygen, encrypt, the model's layer, decrypt -- every output is
    the clear-text layer's, and they are not constant.  Fixes the seeds tests/test_gpu_conv_layer.py reuses."""
    c = conv_model.CONV_DECRYPT_CASE
    d = c["desc"]
    msgs, weight, bias_msgs, f = conv_model.conv_decrypt_case()
    op = oracle.params_from_set(c["paramset"])
    p, q = c["p"], op.q
    rng = oracle.Rng(c["key_seed"])
    sk, bsk, ksk = oracle.keygen(op, rng)
    cts = np.stack([oracle.encrypt(op, rng, sk, int(m), p, q) for m in msgs.ravel()]).reshape(msgs.shape + (op.n + 1,))
    lut = cube_lut(q, p)  # v -> f(floor(v p / q)) q / p
    assert [int(lut[m * (q // p)]) // (q // p) for m in range(p)] == [f(m) for m in range(p)]
    bias = bias_msgs.astype(np.uint64) * np.uint64(q // p)
    orc = oracle.Oracle(op, bsk, ksk)
    try:
        out = conv_model.conv_layer(orc, cts, weight, lut, d, bias, q)
    finally:
        orc.close()
    oh, ow, _ = conv_model.shape(d)
    assert (oh, ow) == (4, 2) and out.shape == (1, d.c_out, oh, ow, op.n + 1)
    got = [oracle.decrypt(op, sk, row, p, q) for row in out.reshape(-1, op.n + 1)]
    want = conv_model.clear_conv(msgs, weight, bias_msgs, f, p, d)
    flat = [v for inst in want for plane in inst for row in plane for v in row]
    assert len(flat) == 16 and got == flat
    assert len(set(flat)) > 1, "the case must not be constant"
