"""The pooling layer in numpy (no GPU): the windowed pair tournament, parameterised by the pair function,
so that one function serves clear integers, the host-array EvalFunc and the oracle.  What tfhe_pool2d_shape,
tfhe_pool2d_eval_plain and tfhe_eval_pool2d* are compared against.

Every (instance, plane, oy, ox) reduces the taps of its window inside the plane, in order t = ky kw + kx: round l
pairs neighbours, L[j] = pair(L[2j], L[2j+1]), an odd last element is carried, until one element is left.  All the
pairs of a round go through `pair` in one call."""
from collections import namedtuple

import numpy as np

# the fields of tfhe_pool2d, in its order: tfhe_amd.Pool2d(*desc) is the library's descriptor
Desc = namedtuple("Desc", "c h w kh kw stride_h stride_w pad_h pad_w")


def desc(c, h, w, kh, kw, stride=None, padding=(0, 0)):
    stride = (kh, kw) if stride is None else stride
    return Desc(c, h, w, kh, kw, stride[0], stride[1], padding[0], padding[1])


def taps(d, oy, ox):
    """The window's taps (y, x) inside the plane, in order t = ky kw + kx; a tap in the padding is left out."""
    out = []
    for ky in range(d.kh):
        for kx in range(d.kw):
            y, x = oy * d.stride_h - d.pad_h + ky, ox * d.stride_w - d.pad_w + kx
            if 0 <= y < d.h and 0 <= x < d.w:
                out.append((y, x))
    return out


def shape(d):
    """(oh, ow, rounds of the longest tournament, pairs per plane) of a valid descriptor."""
    oh = (d.h + 2 * d.pad_h - d.kh) // d.stride_h + 1
    ow = (d.w + 2 * d.pad_w - d.kw) // d.stride_w + 1
    valid = [len(taps(d, oy, ox)) for oy in range(oh) for ox in range(ow)]
    return oh, ow, max((v - 1).bit_length() for v in valid), sum(v - 1 for v in valid)


def pool2d(x, d, pair):
    """x [instances, c, h, w, ...] -> [instances, c, oh, ow, ...].
    pair(a, b): arrays [items, ...] -> [items, ...], one call per round over every pair of the round."""
    x = np.asarray(x)
    assert x.shape[1:4] == (d.c, d.h, d.w), (x.shape, d)
    oh, ow, _, _ = shape(d)
    tail = x.shape[4:]
    lists = [[x[:, :, y, xx] for y, xx in taps(d, oy, ox)] for oy in range(oh) for ox in range(ow)]
    while any(len(L) > 1 for L in lists):
        a = [L[2 * j] for L in lists for j in range(len(L) // 2)]
        b = [L[2 * j + 1] for L in lists for j in range(len(L) // 2)]
        r = pair(np.stack(a).reshape((-1,) + tail), np.stack(b).reshape((-1,) + tail))
        r = np.asarray(r).reshape((len(a),) + x.shape[:2] + tail)
        k = 0
        for i, L in enumerate(lists):
            n = len(L) // 2
            lists[i] = list(r[k:k + n]) + (L[-1:] if len(L) % 2 else [])  # an odd last element is carried
            k += n
    out = np.stack([L[0] for L in lists], axis=2)  # [instances, c, oh ow, ...]
    return out.reshape(x.shape[:2] + (oh, ow) + tail)


def plain_pair(lut, q):
    """op(a, b) = b + lut[a - b mod q] mod q on clear values."""
    lut = np.asarray(lut, dtype=np.uint64)
    m = np.uint64(q - 1)
    return lambda a, b: (b + lut[((a - b) & m).astype(np.int64)]) & m


def func_pair(eval_func, lut, q):
    """op(a, b) = b + EvalFunc(a - b mod q, lut) mod q on ciphertext rows; eval_func(cts[B, n+1], lut, q) is the
    host-array EvalFunc of a context or of the oracle."""
    m = np.uint64(q - 1)
    return lambda a, b: (b + np.asarray(eval_func(np.ascontiguousarray((a - b) & m), lut, q), dtype=np.uint64)) & m


# The decrypting cases shared by tests/test_pool_cpu.py (oracle alone, 8 key seeds) and tests/test_gpu_pool2d.py (a
# from_keygen context).  EvalFunc looks its table up at phase + beta (beta = 128), so with lut[x] = x a pair step
# whose first operand wins returns it 128 higher: a result is off by up to 128 per round plus the noise (DESIGN
# 3.11).  A usable p needs q / 2p above that and the differences inside the table's range.  STD128 (q = 1024)
# admits none for either table -- the best, p = 3 with the arbitrary table, failed 2 of 8 seeds (worst error 180
# against 170) -- so both run on the logQ = 12 context (q = 2048) over one round, a 1 x 2 window:
#   arbitrary:  p = 4, messages {0, 1}: worst error 151 against q / 2p = 256;
#   negacyclic: p = 6, messages {0, 1}: worst error 147 against q / 2p = 170, differences up to 341 + 147 < q / 4.
POOL_DECRYPT_LOGQ = ("STD128", True, 12, 0, 0, 1)  # params_from_logq's arguments
POOL_DECRYPT_CASES = {
    "arbitrary": dict(p=4, hi=2, negacyclic=False),
    "negacyclic": dict(p=6, hi=2, negacyclic=True),
}
POOL_DECRYPT_DESC = desc(1, 1, 3, 1, 2, stride=(1, 1))  # one row of 3: 2 positions of 2 taps, one round
POOL_DECRYPT_SEEDS = tuple(range(3001, 3009))


def pool_decrypt_msgs(kind, seed):
    d = POOL_DECRYPT_DESC
    return np.random.default_rng(seed).integers(0, POOL_DECRYPT_CASES[kind]["hi"], (1, d.c, d.h, d.w), dtype=np.int64)


def clear_max(msgs, d):
    """Max pooling of clear integers [instances, c, h, w] -> [instances, c, oh, ow], padding left out."""
    return pool2d(np.asarray(msgs, dtype=np.int64), d, np.maximum)


# The network of the decrypting GPU case, pinned on the oracle by tests/test_pool_cpu.py: one plane of 3 x 3 mod
# p = 4 -> a 2 x 2 convolution (weights in {0, 1}) with the periodic table m -> m mod 2 -> two planes of 2 x 2 with
# values {0, 1} -> max pooling by a 1 x 2 window (one round, the arbitrary table) -> 2 x 2 x 1 outputs.
NET_CASE = dict(p=4, key_seed=POOL_DECRYPT_SEEDS[0], data_seed=71)


def parity_lut(q, p):
    """v -> (floor(v p / q) mod 2) q / p: a periodic-class table."""
    return np.array([(x // (q // p)) % 2 * (q // p) for x in range(q)], dtype=np.uint64)


def net_case():
    """(msgs [1][1][3][3], weight [2][1][2][2], want [1][2][2][1]) of NET_CASE."""
    rs = np.random.default_rng(NET_CASE["data_seed"])
    msgs = rs.integers(0, NET_CASE["p"], (1, 1, 3, 3), dtype=np.int64)
    weight = rs.integers(0, 2, (2, 1, 2, 2), dtype=np.int64)
    z = np.zeros((1, 2, 2, 2), dtype=np.int64)
    for o in range(2):
        for y in range(2):
            for x in range(2):
                z[0, o, y, x] = int((weight[o, 0] * msgs[0, 0, y:y + 2, x:x + 2]).sum()) % NET_CASE["p"] % 2
    return msgs, weight, clear_max(z, desc(2, 2, 2, 1, 2))
