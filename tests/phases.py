"""Phase sweeps: ciphertexts of a chosen phase, and the plain rule each op applies to it.

Which test-vector entry a bootstrap selects depends on the ciphertext's phase b - <a, s> and on nothing else, and
with q | 2N the blind rotation reads the test vector exactly at that phase.  With valid keys a ciphertext of any
phase phi is `a` uniform, b = <a, s> + phi, so every phase of [0, q) can be driven through the device's three
test-vector builders (k_build_testvector, k_circuit_prep, k_fcircuit_prep) and the result compared with

  * the plain models below: integer-only numpy functions of the phase, each restating a rule of the reference
    (binfhe-base-scheme.cpp, cited by line at each function), and
  * the CPU oracle, bit for bit.

The contexts run at LWE dimension n = 32 (keys of a few MB, 2.5-3.5 ms per oracle bootstrap); the test vector,
the ring dimension, the moduli and the key-switch base are the base set's own.

Distances and windows.  A boundary b of a rule is a phase at which the rule's value may change between b - 1 and
b.  dist(phi) is 1 at b - 1 and at b, 2 at b - 2 and b + 1, ...; a window of half-width W excludes the 2 W
phases with dist <= W.  The two-stage ops (periodic and arbitrary EvalFunc, EvalFloor and what is built on it)
read their second test vector at the phase plus the first bootstrap's noise, so next to a boundary the noise
decides the result; tests/test_phase_model_cpu.py measures how far (d_max) and fixes W = window(d_max).
"""
import ctypes as C

import numpy as np

N32 = 32    # the lowered LWE dimension
SEED = 5    # or_keygen stream of every sweep context
BETA = 128  # BinFHEContext::GetBeta, binfhecontext.h:348-350

# The three contexts of tests/test_gpu_phase_sweep.py (a set name or a params_from_logq argument tuple) and the
# kernel family each must route to (tfhe_info.br_kernel: 1 fast4, 5 sf)
BASE_G = "STD128"                          # N = 1024, q = 1024
BASE_F = ("STD128", True, 12, 0, 0, 1)     # logQ = 12 arbFunc, throw 1: N = q = 2048
BASE_S = ("STD128", False, 23, 0, 0, 1)    # logQ = 23, throw 1: N = 2048, q = 4096
BR_KERNEL = {"G": 1, "F": 5, "S": 5}

# The windows of the two-stage ops.  tests/test_phase_model_cpu.py measures d_max, the largest dist at which the
# oracle departs from the plain model, per op with SEED (1 to 3: DESIGN 2.2), and asserts that window(d_max) is
# the value here.  The single-bootstrap ops (the six gates, the negacyclic LUT) depart nowhere.
W = {"periodic": 8, "arbitrary": 8, "sign": 8, "floor": 8}


def window(d_max):
    """W = max(8, 2 d_max) rounded up to a power of two.  The factor 2: d_max is a sample maximum of Gaussian
    noise, and another seed or key must not turn the window's edge into a flaky test."""
    w = max(8, 2 * int(d_max))
    return 1 << (w - 1).bit_length()


def lowered_params(oracle, base, n=N32, Q=None, baseG_log=None):
    """(cp, op): the engine's and the oracle's parameters of `base` (a set name or a params_from_logq argument
    tuple) at LWE dimension n, with Q / baseG overwritten where given: tfhe_params_finish through the C-ABI, the
    fields it derives mirrored into the oracle's Params."""
    import tfhe_amd
    from tfhe_amd import capi as raw

    if isinstance(base, str):
        cp, op = tfhe_amd.params_from_set(base), oracle.params_from_set(base)
    else:
        cp, op = tfhe_amd.params_from_logq(*base), oracle.params_from_logq(*base)
    cp.n = n
    if Q is not None:
        cp.Q = Q
    if baseG_log is not None:
        cp.baseG = 1 << baseG_log
    cp.digitsG = cp.dG2 = 0
    raw.check(raw.lib().tfhe_params_finish(C.byref(cp)), "tfhe_params_finish")
    for k in ("n", "Q", "baseG", "digitsG", "dG2", "numDigitsToThrow"):
        setattr(op, k, getattr(cp, k))
    op.logG = cp.baseG.bit_length() - 1
    assert (op.N, op.q, op.qKS, op.baseKS, op.dKS) == (cp.N, cp.q, cp.qKS, cp.baseKS, cp.dKS)
    return cp, op


def sweep_context(oracle, base, gpu=True, seed=SEED, n=N32):
    """(orc, ctx, s): the oracle context, the GPU context (None without `gpu`) and the centred secret (int64,
    ternary) of `base` with n lowered (32 unless given): lowered_params, and *valid* keys: or_keygen(seed), a real
    KSK."""
    import tfhe_amd

    cp, op = lowered_params(oracle, base, n)
    sk, bsk, ksk = oracle.keygen(op, oracle.Rng(seed))
    # or_keygen writes s as ternary words mod qKS
    s = np.where(sk > np.uint64(op.qKS // 2), sk.astype(np.int64) - np.int64(op.qKS), sk.astype(np.int64))
    assert set(np.unique(s)) <= {-1, 0, 1}
    assert n < N32 or (np.any(s == 1) and np.any(s == -1))  # (a key of a few words may miss a value)
    orc = oracle.Oracle(op, bsk, ksk)
    ctx = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(bsk, ksk) if gpu else None
    return orc, ctx, s


def with_phase(rs, s, phases, mod, fixed=None):
    """[B + 3, n+1] ciphertexts mod `mod`: row i < B has `a` uniform and b = <a, s> + phases[i]; then three
    fixed rows of the phases `fixed` (default: the first, the middle and the last of `phases`): a = 0; every
    a_i = mod - 1; and b = 0 with one nonzero a_i, on the first key coefficient +-1, solved for the phase."""
    s = np.asarray(s, dtype=np.int64)
    ph = np.asarray(phases, dtype=np.int64).ravel() % mod
    B, n = ph.size, s.size
    f0, f1, f2 = (int(f) % mod for f in (fixed if fixed is not None else (ph[0], ph[B // 2], ph[-1])))
    a = np.zeros((B + 3, n), dtype=np.int64)
    a[:B] = rs.integers(0, mod, (B, n), dtype=np.int64)
    a[B + 1] = mod - 1
    i = int(np.flatnonzero(s)[0])
    a[B + 2, i] = (-f2 * s[i]) % mod  # 0 - a_i s_i = f2 s_i^2 = f2
    b = (a @ s + np.concatenate([ph, [f0, f1, 0]])) % mod
    b[B + 2] = 0
    ct = np.concatenate([a, b[:, None]], axis=1).astype(np.uint64)
    assert np.array_equal(phase_of(ct, s, mod), np.concatenate([ph, [f0, f1, f2]]))
    return ct


def phase_of(ct, s, mod):
    """b - <a, s> mod `mod` of ct[..., n+1], int64."""
    ct = np.asarray(ct).astype(np.int64)
    return (ct[..., -1] - ct[..., :-1] @ np.asarray(s, dtype=np.int64)) % mod


def decrypt(ct, s, p, mod):
    """LWEEncryptionScheme::Decrypt (lwe-pke.cpp:92-130) of ct[..., n+1]: floor(p (phase + mod / (2 p)) / mod)."""
    r = (phase_of(ct, s, mod) + mod // (2 * p)) % mod
    return r * p // mod


def lwe_error(ct, s, want, mod):
    """|phase - want| mod `mod`, centred."""
    d = (phase_of(ct, s, mod) - np.asarray(want, dtype=np.int64)) % mod
    return np.minimum(d, mod - d)


def dist(phi, boundaries, mod):
    """Distance of each phase to the nearest boundary (module docstring), cyclic mod `mod`."""
    phi = np.asarray(phi, dtype=np.int64)
    d = np.full(phi.shape, mod, dtype=np.int64)
    for b in boundaries:
        d = np.minimum(d, np.minimum((phi - b) % mod + 1, (b - phi) % mod))
    return d


# ---------------------------------------------------------------------------------------------------------------
# plain models
# ---------------------------------------------------------------------------------------------------------------
# gate constants q1 = k q / 8 (rgsw-cryptoparameters.h:130-137), in BINGATE order OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST
GATE_K = {"OR": 5, "AND": 7, "NOR": 1, "NAND": 3, "XOR_FAST": 5, "XNOR_FAST": 1}


def gate_phase(gate, phi1, phi2, q):
    """The phase of the prepared ciphertext: ct1 + ct2, or 2 (ct1 - ct2) for the FAST gates
    (binfhe-base-scheme.cpp:642-655)."""
    phi1, phi2 = np.asarray(phi1, dtype=np.int64), np.asarray(phi2, dtype=np.int64)
    return (2 * (phi1 - phi2) if gate.endswith("_FAST") else phi1 + phi2) % q


def gate_model(gate, phi, q):
    """The bit a bootstrapped gate returns for a prepared ciphertext of phase phi.  BootstrapGateCore
    (binfhe-base-scheme.cpp:1116-1129): q1 = the gate constant, q2 = q1 + q/2 mod q; the test vector is -Q/8 for a
    phase in [q1, q2) if q1 < q2, and +Q/8 for a phase in [q2, q1) otherwise (the opposite sign elsewhere);
    the extraction adds Q/8 + 1 (:664-672), so the output encodes 0 where the entry is -Q/8 and Q/4, bit 1,
    where it is +Q/8."""
    phi = np.asarray(phi, dtype=np.int64)
    q1 = GATE_K[gate] * (q >> 3)
    q2 = (q1 + (q >> 1)) % q
    if q1 < q2:
        return np.where((phi >= q1) & (phi < q2), 0, 1)
    return np.where((phi >= q2) & (phi < q1), 1, 0)


def not_phase(phi, q):
    """EvalNOT (binfhe-base-scheme.cpp:147-159): a -> -a, b -> q/4 - b."""
    return (q // 4 - np.asarray(phi, dtype=np.int64)) % q


def xor_model(gate, phi1, phi2, q):
    """XOR / XNOR as the reference composes them (binfhe-base-scheme.cpp:620-640): OR(AND(ct1, NOT ct2),
    AND(NOT ct1, ct2)), negated for XNOR.  The two ANDs follow the range rule at their exact phases; the OR reads
    (t1 + t2) q/4 plus the ANDs' output noise, q/8 away from its range's ends."""
    t1 = gate_model("AND", gate_phase("AND", phi1, not_phase(phi2, q), q), q)
    t2 = gate_model("AND", gate_phase("AND", not_phase(phi1, q), phi2, q), q)
    r = gate_model("OR", (t1 + t2) * (q // 4) % q, q)
    return r if gate == "XOR" else 1 - r


def bin_gate_model(gate, phi1, phi2, q):
    """Any of the eight gates on operand phases."""
    if gate in ("XOR", "XNOR"):
        return xor_model(gate, phi1, phi2, q)
    return gate_model(gate, gate_phase(gate, phi1, phi2, q), q)


def lut_model(lut, phi, q):
    """EvalFunc (binfhe-base-scheme.cpp:679-789): the table entry at (phi + beta) mod q, for all three classes
    (negacyclic :701-713 reads it in one bootstrap; periodic :767-789 and arbitrary :722-765 first clear the top bit).
    lut[q], or [B, q] with phi[B]: row i reads its own table (:791-924)."""
    lut = np.asarray(lut).astype(np.int64)
    x = (np.asarray(phi, dtype=np.int64) + BETA) % q
    return lut[x] if lut.ndim == 1 else lut[np.arange(lut.shape[0]), x]


def lut_boundaries(q, p=8):
    """Phases at which a table over p messages (entry i = f(i // (q / p)) q / p) changes: phi + beta = 0 mod q / p."""
    return [(k * (q // p) - BETA) % q for k in range(p)]


def sign_model(phi, Qin):
    """EvalSign (binfhe-base-scheme.cpp:989-1037): the floors leave the top bits of phi + beta (one beta per
    floor, each absorbed by the next), f3 (:1029-1031) returns +Q/4 below half the last modulus and -Q/4 from
    it, and q/4 comes off: the result decrypts (p = 2) to [(phi + beta) mod Qin >= Qin / 2]."""
    return ((np.asarray(phi, dtype=np.int64) + BETA) % Qin >= Qin // 2).astype(np.int64)


def sign_boundaries(Qin, q):
    """phi + beta = 0 mod Qin / 2, where the rule steps, and q / 2 below: there the first floor is at its own
    boundary (floor_boundaries), and a floor that comes out one q too high carries into the top bit."""
    return [(v - BETA) % Qin for v in (0, Qin // 2, Qin - q // 2, Qin // 2 - q // 2)]


def floor_model(phi, Qin, qf):
    """EvalFloor (binfhe-base-scheme.cpp:926-987): ct + beta, then f1 (:954-959) moves phase mod qf into
    [qf/4, 3 qf/4) and f2 (:973-980) subtracts it: what is left is the multiple of qf below phi + beta.  The
    return value is its decryption at plaintext modulus Qin / qf.  UnitTestFunc.cpp:71-93 is the case Qin = q,
    qf = 512 (roundbits = 1), phi = m q / p + e with q / p = 256: (m 256 + e + 128) // 512 = m // 2 for |e| < beta."""
    return (np.asarray(phi, dtype=np.int64) + BETA) % Qin // qf


def floor_boundaries(phis, Qin, qf):
    """The boundaries of EvalFloor next to the given phases: phi + beta = 0 mod qf / 2 (at 0 mod qf the result
    steps; at qf / 2 f1's noise can carry the phase out of f2's linear range, :973-980)."""
    h = qf // 2
    k = np.unique((np.asarray(phis, dtype=np.int64) + BETA) // h)
    return sorted({int(v * h - BETA) % Qin for v in np.concatenate([k, k + 1])})


def decomp_model(phi, Qin, q):
    """EvalDecomp (binfhe-base-scheme.cpp:1039-1085) at decrypt level, as UnitTestFunc.cpp:198-264 asserts it:
    [(digit values, plaintext modulus, ciphertext modulus)].  Digit 0 is the input mod q (p = q / 2 beta slots);
    each floor and ModSwitch (mod -> mod / q * 2 beta) moves the next p-ary digit of (phi + beta) // 2 beta down; the
    last digit keeps the modulus the floors left and the slots that remain.  UnitTestFunc's messages P/2 - 3 ..
    P/2 + 4 are phi = m 2 beta + e: digit 0 = 13 .. 15, 0 .. 4, the middle digits 15 or 0, the last 0 or 1."""
    phi = np.asarray(phi, dtype=np.int64)
    M = (phi + BETA) % Qin // (2 * BETA)
    p = q // (2 * BETA)
    out, mod = [], Qin
    while mod > q:
        out.append((M % p, p, q))
        M = M // p
        mod = mod // q * 2 * BETA
    out.append((M, mod // (2 * BETA), mod))
    return out
