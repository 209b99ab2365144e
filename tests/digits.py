"""The gadget digits' boundaries: what tests/test_digit_boundaries_cpu.py and
tests/test_gpu_digit_boundaries.py share -- the reference's carry loop on Python integers, the accumulator values
at which a digit jumps, accumulators tiled from them, and bootstrapping keys that keep them there.

Every round of a blind rotation cuts each accumulator coefficient c (centred: c < Q >> 1 ? c : c - Q) into digitsG
signed digits of logG bits (rgsw-acc.cpp:57-111): r = the low logG bits sign-extended, c = (c - r) >> logG; the
first numDigitsToThrow digits are dropped.  In closed form digit l is the window of logG bits at bit logG l of
c + K_l, K_l = (B/2)(B^l - 1)/(B - 1), B = 2^logG, and what is left after the last digit is floor((c + K_D) / B^D),
D = digitsG.  The kernels restate one or the other; both jump at c + K_l = 0 mod B^l.

Two synthetic round keys, in the BSK layout [n][2 keys][dG2 rows][2 polys][N]:
  ZERO      every row 0: the round adds nothing;
  IDENTITY  the trivial RGSW encryption of 1 in the + key (row j + 2 l, polynomial j = the constant B^(l + thr)) and
            0 in the - key: acc (.) key = R(acc), R(c) = sum_l d_l(c) B^(l + thr) mod Q per coefficient, and the
            round is acc <- acc + (X^m - 1) R(acc), m = ((amod - a_i) mod amod) 2N / amod.  Where the digits
            reconstruct c this is acc <- X^m acc: boundary values are rotated and negated and stay boundary values.
"""
import numpy as np

import lwe_dim as ld

N_ROUNDS = 3  # both round parities; a first, a middle and a last round
CLASSES = ("centre", "window", "residual", "ripple")


# ---------------------------------------------------------------------------------------------------------------
# the integer model
# ---------------------------------------------------------------------------------------------------------------
def shape(p):
    """(Q, logG, digitsG, thr) of an oracle or engine parameter struct."""
    return int(p.Q), int(p.baseG).bit_length() - 1, int(p.digitsG), int(p.numDigitsToThrow)


def digits(c, Q, logG, digitsG, thr):
    """(kept signed digits, residual) of the residue c: the reference's carry loop."""
    assert 0 <= c < Q
    B = 1 << logG
    d = c if c < (Q >> 1) else c - Q
    out = []
    for _ in range(digitsG):
        r = d & (B - 1)
        if r >= B >> 1:
            r -= B
        d = (d - r) >> logG
        out.append(r)
    return out[thr:], d


def recon(c, Q, logG, digitsG, thr):
    """R(c) = sum_l d_l(c) B^(l + thr) mod Q."""
    kept, _ = digits(c, Q, logG, digitsG, thr)
    return sum(d << (logG * (l + thr)) for l, d in enumerate(kept)) % Q


def digit_words(acc, Q, logG, digitsG, thr):
    """acc[B][2][N] -> [B][dG2][N]: row j + 2 l = digit l of polynomial j as a residue mod Q, the layout of
    or_signed_digit_decompose."""
    acc = np.asarray(acc, dtype=np.uint64)
    u, inv = np.unique(acc, return_inverse=True)
    rows = np.array([[d % Q for d in digits(int(c), Q, logG, digitsG, thr)[0]] for c in u], dtype=np.uint64)
    d = rows[inv.ravel()].reshape(acc.shape + (digitsG - thr,))  # [B][2][N][l]
    return np.ascontiguousarray(d.transpose(0, 3, 1, 2)).reshape(acc.shape[0], 2 * (digitsG - thr), acc.shape[2])


def exponents(a, amod, N):
    """m[B][n] = ((amod - a) mod amod) 2N / amod (rgsw-acc-cggi.cpp:153)."""
    a = np.asarray(a, dtype=np.uint64).astype(np.int64)
    assert (2 * N) % amod == 0
    return ((amod - a % amod) % amod) * (2 * N // amod)


def identity_round(acc, m, Q, logG, digitsG, thr):
    """One IDENTITY round: acc[B][2][N] + (X^m[b] - 1) R(acc) mod Q, canonical residues."""
    acc = np.asarray(acc, dtype=np.uint64)
    assert Q < 1 << 61
    N = acc.shape[-1]
    u, inv = np.unique(acc, return_inverse=True)
    Ru = np.array([recon(int(c), Q, logG, digitsG, thr) for c in u], dtype=np.int64)
    R = Ru[inv.ravel()].reshape(acc.shape)
    out = acc.astype(np.int64)
    for b, mb in enumerate(np.asarray(m).ravel()):
        mb = int(mb)
        assert 0 <= mb < 2 * N
        if mb == 0:
            continue
        s = mb % N
        rot = np.roll(R[b], s, axis=-1)  # X^s R: coefficient k moves to k + s, the wrapped ones negated
        rot[:, :s] = -rot[:, :s]
        if mb >= N:
            rot = -rot
        out[b] = (out[b] - R[b] + rot) % Q
    return out.astype(np.uint64)


def identity_states(a, amod, acc, Q, logG, digitsG, thr, rounds=None):
    """[acc before round 0, after round 0, ...] of IDENTITY rounds over a[:, :rounds]."""
    a = np.asarray(a)
    m = exponents(a, amod, np.asarray(acc).shape[-1])
    out = [np.asarray(acc, dtype=np.uint64)]
    for i in range(a.shape[1] if rounds is None else rounds):
        out.append(identity_round(out[-1], m[:, i], Q, logG, digitsG, thr))
    return out


def identity_model(a, amod, acc, Q, logG, digitsG, thr):
    """EvalAcc under IDENTITY keys in every round: the rounds, then the extraction transpose."""
    return ld.transpose0(identity_states(a, amod, acc, Q, logG, digitsG, thr)[-1], Q)


# ---------------------------------------------------------------------------------------------------------------
# the values
# ---------------------------------------------------------------------------------------------------------------
def boundary_values(Q, logG, digitsG, thr):
    """(values, classes): canonical residues whose centred value lies in [floor(Q/2) - Q, floor(Q/2)), sorted by
    centred value, and for each the tuple of CLASSES that produced it.

      centre    0, +-1, +-2 and the three values at each end of the centred range;
      window    c + K_l = m B^l + e, e in -2 .. 1, for l = 1 .. digitsG - 1 (thrown digits counted): the floor
                boundary of digit l's window, digit l - 1 on its tie; m in {0, +-1, 2}, the smallest and largest m
                the range admits with their inner neighbours, and {B/2 - 1, B/2, B/2 + 1, -B/2}, which put digit l
                on its own tie;
      residual  the same at l = digitsG (m without the last four): the first value whose digits leave a residual
                and the one below it;
      ripple    sum_{l < t} (B/2 - 1) B^l, one below and one above, for t = 1 .. digitsG: a carry through t digits.

    The list is then closed under negation mod Q (a negated value keeps its classes): an IDENTITY round rotates
    and negates, so a closed list stays a list."""
    B = 1 << logG
    hi = Q >> 1
    lo = hi - Q
    found = {}

    def add(c, cls):
        if lo <= c < hi:
            found.setdefault(c, set()).add(cls)

    for c in (0, 1, -1, 2, -2, lo, lo + 1, lo + 2, hi - 1, hi - 2, hi - 3):
        add(c, "centre")
    for l in range(1, digitsG + 1):
        Bl = B ** l
        K = (B >> 1) * (Bl - 1) // (B - 1)
        m_min = -((-(lo + K - 1)) // Bl)   # the smallest m with m B^l + 1 - K >= lo
        m_max = (hi - 1 + K + 2) // Bl     # the largest m with m B^l - 2 - K < hi
        ms = {0, 1, -1, 2, m_min, m_min + 1, m_max - 1, m_max}
        if l < digitsG:
            ms |= {(B >> 1) - 1, B >> 1, (B >> 1) + 1, -(B >> 1)}
        for m in ms:
            for e in (-2, -1, 0, 1):
                add(m * Bl + e - K, "window" if l < digitsG else "residual")
    for t in range(1, digitsG + 1):
        v = sum(((B >> 1) - 1) * B ** l for l in range(t))
        for c in (v - 1, v, v + 1, -v + 1, -v, -v - 1, -v - 2):
            add(c, "ripple")
    for c, cls in list(found.items()):
        neg = (-c) % Q
        neg = neg if neg < hi else neg - Q
        found.setdefault(neg, set()).update(cls)
    order = sorted(found)
    return [c % Q for c in order], [tuple(k for k in CLASSES if k in found[c]) for c in order]


def has_residual(Q, logG, digitsG, thr):
    """Whether some value of the centred range leaves a residual (the residual is monotone in c)."""
    hi = Q >> 1
    return any(digits(c % Q, Q, logG, digitsG, thr)[1] != 0 for c in (hi - 1, hi - Q))


def reconstructs(values, Q, logG, digitsG, thr):
    """Whether R(c) = c for every value: then IDENTITY rounds only rotate and negate the list."""
    return all(recon(c, Q, logG, digitsG, thr) == c for c in values)


def tile(values, N, B, Q, seed=0):
    """acc[B][2][N]: rows 0 .. B - 2 from the list, the last row random.  The list is padded to an odd length
    (coprime to the power-of-two lane and register strides).  Coefficient k = 8 g + r of polynomial j of row b
    holds values[(g + (N / 8) b + 37 r + 3 j) mod len]: for each r the B - 1 rows cover (B - 1) N / 8 consecutive
    list positions, so every value meets every residue of k mod 8 in each polynomial (positions())."""
    vals = list(values) + ([values[0]] if len(values) % 2 == 0 else [])
    L = len(vals)
    assert N % 8 == 0 and (B - 1) * (N >> 3) >= L, (N, B, L)
    v = np.array(vals, dtype=np.uint64)
    k = np.arange(N)
    acc = np.random.default_rng(seed).integers(0, Q, (B, 2, N), dtype=np.uint64)
    for b in range(B - 1):
        for j in range(2):
            acc[b, j] = v[((k >> 3) + (N >> 3) * b + 37 * (k & 7) + 3 * j) % L]
    return acc


def positions(acc, values):
    """tile's condition: {(polynomial, value): the residues mod 8 of the coefficient indices at which rows
    0 .. B - 2 hold the value}."""
    acc = np.asarray(acc)
    out = {}
    for j in range(2):
        for v in set(values):
            out[j, v] = set(int(x) & 7 for x in np.nonzero(acc[:-1, j] == np.uint64(v))[1])
    return out


def list_share(acc, values):
    """The share of the words of rows 0 .. B - 2 that are list values."""
    rows = np.asarray(acc)[:-1]
    return float(np.isin(rows, np.array(sorted(set(values)), dtype=np.uint64)).mean())


# ---------------------------------------------------------------------------------------------------------------
# the keys and the rotations
# ---------------------------------------------------------------------------------------------------------------
def identity_rows(p):
    """One IDENTITY round [2][dG2][2][N]."""
    Q, logG, digitsG, thr = shape(p)
    assert p.dG2 == 2 * (digitsG - thr)
    rows = np.zeros((2, p.dG2, 2, p.N), dtype=np.uint64)
    for l in range(digitsG - thr):
        for j in range(2):
            rows[0, j + 2 * l, j, 0] = (1 << (logG * (l + thr))) % Q
    return rows


def mixed_keys(oracle, seed, prefix, last=True):
    """keys(cp, op) -> (bsk, ksk): the seeded random keys of lwe_dim.kat_edge_keys with the rounds before the last
    (last = False: every round) replaced by `prefix` rounds, "zero" or "identity"."""
    assert prefix in ("zero", "identity")

    def keys(cp, op):
        bsk, ksk = ld.kat_edge_keys(oracle, seed)(cp, op)
        rounds = bsk.reshape(op.n, 2, op.dG2, 2, op.N)
        rounds[: op.n - 1 if last else op.n] = 0 if prefix == "zero" else identity_rows(op)
        return bsk, ksk

    return keys


def zero_keys(oracle, seed):
    return mixed_keys(oracle, seed, "zero", last=False)


def identity_keys(oracle, seed):
    return mixed_keys(oracle, seed, "identity", last=False)


def rotations(amod, n, B, N, seed=0):
    """a[B][n] without a zero entry: row 0 every m = N (a = amod / 2: X^N = -1, the IDENTITY round is acc - 2 R);
    row 1 every a = amod - 1, the smallest step forwards (m = 2N / amod: every m = 1 where amod = 2N); row 2 every
    a = 1, the same step backwards (m = 2N - 2N / amod); the rest random."""
    assert B >= 4 and amod % 2 == 0 and amod > 2
    a = np.random.default_rng(seed).integers(1, amod, (B, n), dtype=np.uint64)
    a[0] = amod >> 1
    a[1] = amod - 1
    a[2] = 1
    assert a.all() and (a < amod).all()
    return a


# ---------------------------------------------------------------------------------------------------------------
# the recipes of the GPU module: name -> (keys, what it reaches)
# ---------------------------------------------------------------------------------------------------------------
RECIPES = ("first", "identity", "zero-carried", "identity-carried")


def recipe_keys(oracle, recipe, seed):
    return {"first": lambda: ld.kat_edge_keys(oracle, seed),
            "identity": lambda: identity_keys(oracle, seed),
            "zero-carried": lambda: mixed_keys(oracle, seed, "zero"),
            "identity-carried": lambda: mixed_keys(oracle, seed, "identity")}[recipe]()


def inputs(op, seed=0, B=ld.B):
    """(values, [(what, a, amod, acc)]) of one context: tile accumulators and rotations at both a-moduli."""
    Q, logG, digitsG, thr = shape(op)
    values, _ = boundary_values(Q, logG, digitsG, thr)
    acc = tile(values, op.N, B, Q, seed)
    calls = [(f"a mod {amod}", rotations(amod, op.n, B, op.N, seed + amod), amod, acc)
             for amod in sorted({int(op.q), 2 * op.N})]
    return values, calls
