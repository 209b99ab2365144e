"""The key switch in Python integers, and the edge contexts, KSK fills and extract rows of the key-switch edge tests
(tests/test_ks_model_cpu.py, tests/test_gpu_keyswitch_edges.py).

Straight from the definition (ks_tiled.hip:4-6; lwe-pke.cpp:204-215, 299-321):

    x_i     = RoundqQ(ext[i], qKS, Q)                         i <= N
    d_j(i)  = the j-th base-baseKS digit of x_i, least significant first, j < dKS
    sum_k   = sum over i < N, j < dKS of KSK[i][d_j(i)][j][k]   exactly, no reduction, k <= n
    out[k]  = RoundqQ((0 - sum_k) mod qKS, fmod, qKS)         k < n
    out[n]  = RoundqQ((x_N - sum_n) mod qKS, fmod, qKS)

RoundqQ is the reference's double formula (lwe-pke.cpp:41-46) in Python floats, the one test_round_qQ uses.  The
column sums are exact: the selected rows' 32-bit halves are added in uint64 (N dKS 2^32 < 2^64, asserted) and joined
as Python integers.  Nothing here is shared with the oracle (oracle/tfhe_oracle.c mkm_one, which subtracts mod qKS
row by row) or with the device code.
"""
import math

import numpy as np


def round_qQ(v, q, Q):
    return int(math.floor(0.5 + float(v) * float(q) / float(Q))) % q


def ks_sums(p, ksk, row):
    """(exact column sums [n + 1] as Python integers, x_N) for one extract row; ksk: the flat caller's-layout key."""
    N, n, bks, dks, qks, Q = p.N, p.n, p.baseKS, p.dKS, int(p.qKS), int(p.Q)
    assert N * dks < (1 << 31)
    K = np.asarray(ksk, dtype=np.uint64).reshape(N, bks, dks, n + 1)
    x = [round_qQ(int(v), qks, Q) for v in row]
    dig = np.empty((N, dks), dtype=np.int64)
    for i in range(N):
        t = x[i]
        for j in range(dks):
            dig[i, j] = t % bks
            t //= bks
    rows = K[np.arange(N)[:, None], dig, np.arange(dks)[None, :]].reshape(N * dks, n + 1)
    lo = (rows & np.uint64(0xFFFFFFFF)).sum(axis=0, dtype=np.uint64)
    hi = (rows >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
    return [int(l) + (int(h) << 32) for l, h in zip(lo, hi)], x[N]


def ks_finish(p, sums, xN, fmod):
    n, qks = p.n, int(p.qKS)
    out = [round_qQ((0 - s) % qks, fmod, qks) for s in sums[:n]]
    out.append(round_qQ((xN - sums[n]) % qks, fmod, qks))
    return np.array(out, dtype=np.uint64)


def key_switch(p, ksk, ext, fmod):
    """[B][n + 1] for ext[B][N + 1]."""
    ext = np.atleast_2d(ext)
    return np.stack([ks_finish(p, *ks_sums(p, ksk, row), fmod) for row in ext])


# ---------------------------------------------------------------------------------------------------------------
# The edge contexts.  base: a set name or a params_from_logq argument tuple; qKS / baseKS None: as the set.
# star: also at n = 32 and 47.  Expected launch form of the tiled key switch: kb key bytes (with ks40 = 0: kb0),
# sum: sum width in bits with packed sums / without; tiled False: the tiled form declines the shape.
# ---------------------------------------------------------------------------------------------------------------
ARB12 = ("STD128", True, 12, 0, 0, 1)
LOGQ23 = ("STD128", False, 23, 0, 0, 1)

CONTEXTS = {
    # PK form (packed u16 pairs mod 2^16), CTS 1 / 2 / 4
    "u16-packed": dict(base="STD128", qKS=1 << 14, baseKS=128, star=True, kb=2, sums=(16, 32), pk=True),
    # the largest u16 key word; packed sums wrap mod 2^16 = qKS; the boundary of ksk_bits_for
    "u16-top": dict(base="STD128", qKS=1 << 16, kb=2, sums=(16, 32), pk=True),
    # u16 keys, exact u32 sums, no PK whatever the knob says
    "u16-npot": dict(base="STD128", qKS=(1 << 16) - 1, kb=2, sums=(32, 32)),
    # the smallest u32-key modulus: u32 keys, exact u32 sums (acc32 holds) and a qKS that is no power of two, the
    # only context whose u32 / u32 build finishes with a real `colsum % qKS`.  With STD128's baseKS = 128 the rows of
    # u32 words exceed the tiled form's LDS stage (2 x 4 x 128 x 144 B > 80 KiB, launch_tiled), so the tiled form
    # runs at the nearest base it admits, 32 (dKS = 4), and baseKS = 128 stays as the declined shape: the gather
    # serves every batch and no `[ks]` line may appear
    "u32-first": dict(base="STD128", qKS=(1 << 16) + 1, baseKS=32, kb=4, sums=(32, 32)),
    "u32-first-b128": dict(base="STD128", qKS=(1 << 16) + 1, kb=4, sums=(32, 32), tiled=False),
    # exact u32 sums reaching N dKS (qKS - 1) = 2^32 - 8192
    "u32-bound": dict(base="STD192", star=True, kb=4, sums=(32, 32), bound=(1 << 32) - 8192),
    # N dKS (qKS - 1) = 2^32 + 16384: must take u64 sums
    "u32-past": dict(base="STD192", qKS=(1 << 19) + 3, kb=4, sums=(64, 64), bound=(1 << 32) + 16384),
    # u32 sums wrapping mod 2^32
    "u32-wrap": dict(base="STD128Q", kb=4, sums=(32, 32)),
    # the largest u32 key word
    "u32-top": dict(base="STD128Q", qKS=1 << 32, kb=4, sums=(32, 32)),
    # split-word records, byte fields of width b = 1, 3, 5; ks40 = 0: the u64 words
    "split-b1": dict(base=ARB12, qKS=1 << 33, kb=5, kb0=8, sums=(64, 64)),
    "split-b3": dict(base=ARB12, qKS=1 << 35, star=True, kb=5, kb0=8, sums=(64, 64)),
    "split-b5": dict(base=ARB12, qKS=1 << 37, kb=5, kb0=8, sums=(64, 64)),
    # ks40_hbits = 0: the u64 words serve, though records could be packed
    "u64-2^38": dict(base=ARB12, qKS=1 << 38, kb=8, sums=(64, 64)),
    "u64-npot": dict(base=ARB12, qKS=(1 << 35) - 1, kb=8, sums=(64, 64)),
    # the sweep of small LWE dimensions only (small_cases): logQ = 23, q = 2N beside ARB12's q = N
    "split-b3-q2N": dict(base=LOGQ23, kb=5, kb0=8, sums=(64, 64), small_only=True),
}

FILLS = ("max", "even", "odd", "random")
N_STAR = (32, 33, 47)  # a full last column tile, one column into a new tile, one short of full; n_pad > n at every width
N_PLAIN = (33,)
# Small LWE dimensions (tests/test_lwe_dimension_cpu.py, tests/test_gpu_lwe_dimension.py): one column, two, one short
# of the 8 words of a u16 piece, exactly 8, one past.  n_pad (n rounded up to a 16-byte piece: 8 u16, 4 u32, 2 u64
# words) is smaller than one column tile at every width, so every piece past it is a clamped one.
N_SMALL = (1, 2, 7, 8, 9)
SMALL = ("u16-packed", "u32-bound", "split-b3", "split-b3-q2N")  # each base set's own qKS and baseKS


def cases():
    """(context name, n) of every edge context."""
    return [(name, n) for name, c in CONTEXTS.items() if not c.get("small_only")
            for n in (N_STAR if c.get("star") else N_PLAIN)]


def small_cases(names=SMALL):
    """(context name, n) of the small-n sweep."""
    return [(name, n) for name in names for n in N_SMALL]


def dks_for(qKS, baseKS):
    """dKS as params_finish derives it (lwe-pke.cpp:305: natural-log ratio)."""
    return int(math.ceil(math.log(float(qKS)) / math.log(float(baseKS))))


def edge_params(module, name, n):
    """Parameters of edge context `name` at LWE dimension n from `module` (pyoracle or tfhe_amd): the base set
    with n, qKS and baseKS overwritten and dKS recomputed."""
    c = CONTEXTS[name]
    p = module.params_from_set(c["base"]) if isinstance(c["base"], str) else module.params_from_logq(*c["base"])
    p.n = n
    if c.get("qKS"):
        p.qKS = c["qKS"]
    if c.get("baseKS"):
        p.baseKS = c["baseKS"]
    p.dKS = dks_for(p.qKS, p.baseKS)
    if "bound" in c:
        assert p.N * p.dKS * (p.qKS - 1) == c["bound"], (name, p.N, p.dKS, p.qKS)
    return p


def ksk_words(p):
    return p.N * p.baseKS * p.dKS * (p.n + 1)


def make_ksk(p, fill, seed=0):
    """KSK [N][baseKS][dKS][n + 1] (flat) of one fill: every entry qKS - 1; even columns qKS - 1 and odd columns 0
    (the B entry, column n, follows its parity) and the reverse, so a carry out of a packed half or a byte field
    lands in a zero column and shows; seeded random."""
    n, top = p.n, int(p.qKS) - 1
    if fill == "random":
        return np.random.default_rng(1000 + seed).integers(0, int(p.qKS), ksk_words(p), dtype=np.uint64)
    row = np.full(n + 1, top, dtype=np.uint64)
    if fill == "even":
        row[1::2] = 0
    elif fill == "odd":
        row[0::2] = 0
    else:
        assert fill == "max"
    return np.tile(row, p.N * p.baseKS * p.dKS)


def preimage(t, q, Q):
    """A v < Q with RoundqQ(v, q, Q) = t (the middle of t's interval)."""
    v = (t * Q) // q
    for d in (0, 1, -1, 2, -2):
        if 0 <= v + d < Q and round_qQ(v + d, q, Q) == t:
            return v + d
    raise AssertionError((t, q, Q))


EDGE_ROWS = 4  # rows r with r % ROW_PERIOD < EDGE_ROWS are edge rows of kind r % ROW_PERIOD
ROW_PERIOD = 7


def make_ext(p, B, seed=0):
    """Extract rows [B][N + 1] mod Q; row r is of kind r % 7: 0 all 0; 1 all Q - 1; 2 every coefficient rounds to
    qKS - 1 (every digit at its largest, the partial top digit too); 3 cycles through the values that round to
    baseKS^j - 1 and baseKS^j (j = 0 .. dKS, those below qKS: a digit at its largest next to the carry into the next
    one); 4, 5, 6 random.  A batch of B rows is the first B of these, so every batch from 4 up holds the four edge
    kinds and the tile edges 256 / 512 / 1024 / 2048 fall on different kinds."""
    N, Q, qks, bks = p.N, int(p.Q), int(p.qKS), p.baseKS
    ext = np.random.default_rng(2000 + seed).integers(0, Q, (B, N + 1), dtype=np.uint64)
    top = preimage(qks - 1, qks, Q)
    cyc = sorted({t for j in range(p.dKS + 1) for t in (bks ** j - 1, bks ** j) if 0 <= t < qks})
    cyc = np.array([preimage(t, qks, Q) for t in cyc], dtype=np.uint64)
    ext[0::ROW_PERIOD] = 0
    ext[1::ROW_PERIOD] = Q - 1
    ext[2::ROW_PERIOD] = top
    ext[3::ROW_PERIOD] = cyc[np.arange(N + 1) % len(cyc)]
    return ext
