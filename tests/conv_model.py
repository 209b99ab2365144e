"""The convolution layer y = f(conv(x) + b) in numpy and Python integers (no GPU): im2col, then the dense model's
exact matrix product per group (tests/dense_model.py), the bias on the b word, then the oracle's EvalFunc with one
shared table.  What tfhe_ciphertext_conv2d_device and tfhe_eval_conv2d* are compared against."""
from collections import namedtuple

import numpy as np

import dense_model

# the fields of tfhe_conv2d, in its order: tfhe_amd.Conv2d(*desc) is the library's descriptor
Desc = namedtuple("Desc", "c_in h w c_out kh kw stride_h stride_w pad_h pad_w groups")


def desc(c_in, h, w, c_out, kh, kw, stride=(1, 1), padding=(0, 0), groups=1):
    return Desc(c_in, h, w, c_out, kh, kw, stride[0], stride[1], padding[0], padding[1], groups)


def shape(d):
    """(oh, ow, K) of a valid descriptor."""
    oh = (d.h + 2 * d.pad_h - d.kh) // d.stride_h + 1
    ow = (d.w + 2 * d.pad_w - d.kw) // d.stride_w + 1
    return oh, ow, (d.c_in // d.groups) * d.kh * d.kw


def im2col(x, d):
    """x [instances, c_in, h, w, ...] -> [instances, oh ow, groups, K, ...]: row k = (ic kh + ky) kw + kx of group g
    at position oy ow + ox is x[i, g Cg + ic, oy sh - ph + ky, ox sw - pw + kx], zeros in the padding."""
    oh, ow, K = shape(d)
    Cg = d.c_in // d.groups
    xp = np.zeros(x.shape[:2] + (d.h + 2 * d.pad_h, d.w + 2 * d.pad_w) + x.shape[4:], dtype=x.dtype)
    xp[:, :, d.pad_h:d.pad_h + d.h, d.pad_w:d.pad_w + d.w] = x
    out = np.zeros((x.shape[0], oh * ow, d.groups, K) + x.shape[4:], dtype=x.dtype)
    for oy in range(oh):
        for ox in range(ow):
            win = xp[:, :, oy * d.stride_h:oy * d.stride_h + d.kh, ox * d.stride_w:ox * d.stride_w + d.kw]
            out[:, oy * ow + ox] = win.reshape((x.shape[0], d.groups, Cg * d.kh * d.kw) + x.shape[4:])
    return out


def conv2d(cts, weight, modulus, d, bias=None):
    """out[i][o][oy][ox][w] of the definition, exact at every modulus: cts [instances, c_in, h, w, n+1]
    (or [c_in, h, w, n+1]: one instance) u64, not necessarily reduced; weight [c_out, c_in/groups, kh, kw] int64;
    bias [c_out] u64 (any values) or None.  Returns u64 [instances, c_out, oh, ow, n+1] (or without instances)."""
    x = np.asarray(cts, dtype=np.uint64)
    one = x.ndim == 4
    if one:
        x = x[None]
    W = np.asarray(weight, dtype=np.int64)
    oh, ow, K = shape(d)
    Og = d.c_out // d.groups
    assert x.shape[1:4] == (d.c_in, d.h, d.w) and W.shape == (d.c_out, d.c_in // d.groups, d.kh, d.kw), (x.shape, W.shape)
    inst, width = x.shape[0], x.shape[4]
    cols = im2col(x, d)  # [inst, npos, groups, K, width]
    out = np.empty((inst, d.c_out, oh * ow, width), dtype=np.uint64)
    for g in range(d.groups):
        mat = W[g * Og:(g + 1) * Og].reshape(Og, K).T  # [K, Og]
        b = None if bias is None else np.asarray(bias, dtype=np.uint64)[g * Og:(g + 1) * Og]
        z = dense_model.product(cols[:, :, g].reshape(inst * oh * ow, K, width), mat, modulus, b)  # [inst npos, Og, width]
        out[:, g * Og:(g + 1) * Og] = z.reshape(inst, oh * ow, Og, width).transpose(0, 2, 1, 3)
    out = out.reshape(inst, d.c_out, oh, ow, width)
    return out[0] if one else out


def conv_layer(orc, cts, weight, lut, d, bias=None, q=None):
    """EvalFunc(conv2d(cts, weight, q, d, bias), lut) through the oracle `orc` (pyoracle.Oracle), shared table."""
    q = q or orc.p.q
    z = conv2d(cts, weight, q, d, bias)
    return orc.eval_func(z.reshape(-1, z.shape[-1]), lut, q).reshape(z.shape)


def clear_conv(msgs, weight, bias_msgs, f, p, d):
    """The layer on clear messages mod p: msgs [instances, c_in, h, w] -> nested lists [instances][c_out][oh][ow] of
    f((sum over the window + bias_msgs[o]) mod p)."""
    M = np.asarray(msgs, dtype=np.int64)
    if M.ndim == 3:
        M = M[None]
    z = conv2d(M.astype(np.uint64)[..., None] % np.uint64(p), weight, p, d)[..., 0].astype(np.int64)
    return [[[[f(int((z[i, o, y, x] + int(bias_msgs[o])) % p)) for x in range(z.shape[3])] for y in range(z.shape[2])]
             for o in range(z.shape[1])] for i in range(z.shape[0])]


# The decrypting case shared by tests/test_conv_cpu.py (oracle alone) and tests/test_gpu_conv_layer.py (device):
# STD128, plaintexts mod p = 4, c_in = 2, 3 x 3 planes, a 2 x 2 window, stride 1, padding (1, 0), c_out = 2, one
# instance: 4 x 2 positions per plane, 16 outputs.  Weights in {-1, 0, 1, 2}, a bias, and the arbitrary-class table
# v -> f(floor(v p / q)) q / p with f(m) = m^3 mod 4.  Worst-case noise: K = 8 taps of magnitude <= 2 scale the
# fresh ciphertexts' Gaussian (sigma 3.19) by at most sqrt(8 * 4) = sqrt(32): about 18, against EvalFunc's margin
# of beta = 128 (q / 2p) on either side, about 7 sigma.
CONV_DECRYPT_CASE = dict(paramset="STD128", p=4, key_seed=2029, data_seed=67,
                         desc=desc(2, 3, 3, 2, 2, 2, stride=(1, 1), padding=(1, 0)))


def conv_decrypt_case():
    """(msgs [1][2][3][3], weight [2][2][2][2], bias_msgs [2], f) of CONV_DECRYPT_CASE."""
    c = CONV_DECRYPT_CASE
    d = c["desc"]
    rs = np.random.default_rng(c["data_seed"])
    msgs = rs.integers(0, c["p"], (1, d.c_in, d.h, d.w), dtype=np.int64)
    weight = rs.integers(-1, 3, (d.c_out, d.c_in // d.groups, d.kh, d.kw), dtype=np.int64)  # {-1, 0, 1, 2}
    bias_msgs = rs.integers(0, c["p"], d.c_out, dtype=np.int64)
    return msgs, weight, bias_msgs, (lambda m: m ** 3 % 4)
