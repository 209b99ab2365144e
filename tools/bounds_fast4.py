"""Per-index worst-case magnitude bounds for the 4-wavefront fast kernel's transforms
(blind_rotate_fast4.hip): radix-4 passes over index bit pairs (b9 b8), (b7 b6), ... (b1 b0)
(forward, Cooley-Tukey) and the reverse (inverse, Gentleman-Sande), signed Montgomery
products (|smul(y, w)| <= |y| (Q/2) / 2^32 + Q/2).  RED lists, per inverse pass, which stage's
sum outputs are reduced (smul by R mod Q).  Asserts every 32-bit value < 2^31, the external
product row sums < 2^63, and the accumulator update window, for every digit shape the kernel is
built for.  Run: python3 tools/bounds_fast4.py [Q]"""
import sys

Q = int(sys.argv[1]) if len(sys.argv) > 1 else 134215681
Qh = Q // 2
LIM = 2 ** 31
RED = {0: None, 1: "B", 2: None, 3: "B", 4: None}   # inverse pass (L5, L4, L3, L2, L1) -> reduced stage


def smul_b(y):
    assert y < LIM, f"smul input {y / Q:.2f}Q"
    return y * Qh / 2 ** 32 + LIM * Q / 2 ** 32


def fwd(b_in, small=False):
    b = list(b_in)
    if small:  # pass 0 from the lookup tables: x0 + T1[x2] +- (T2[x1] + T21[x3]), tables reduced (<= Q/2)
        b = [max(b_in) + 3 * (Qh + 1)] * 1024
    for p in range(1 if small else 0, 5):
        for bit in (9 - 2 * p, 8 - 2 * p):
            m = 1 << bit
            nb = list(b)
            for i in range(1024):
                if not i & m:
                    j = i | m
                    v = smul_b(b[j])
                    nb[i] = nb[j] = b[i] + v
                    assert nb[i] < LIM
            b = nb
    return b


def inv(b_in):
    b = list(b_in)
    for p in range(5):
        for s, bit in enumerate((2 * p, 2 * p + 1)):
            m = 1 << bit
            nb = list(b)
            red = RED[p] == "AB"[s]
            for i in range(1024):
                if not i & m:
                    j = i | m
                    t = b[i] + b[j]
                    assert t < LIM, f"inverse pass {p} stage {s}: {t / Q:.2f}Q"
                    nb[i] = smul_b(t) if red else t
                    nb[j] = smul_b(t)
            b = nb
    return b




def check(dig, logg, fold, split=False):
    """DIG digits of base 2^logg per polynomial; fold = top digit eliminated (C rows); split = the SPLIT
    form: each group reduces its own polynomial's half of the row sum, and A is the sum of two such"""
    dmax = 1 << (logg - 1)
    F = max(fwd([dmax] * 1024))
    if logg <= 7:  # pass 0 from the lookup tables (digits in [-64, 64))
        F = max(F, max(fwd([dmax] * 1024, small=True)))
    nt = dig - 1 if fold else dig          # transformed digits
    rowsum = 2 * nt * F * Qh + (2 * F * Qh if fold else 0)  # C rows kept <= F
    assert rowsum < 2 ** 63
    A = rowsum / 2 ** 32 + Qh                 # sredc of the row sum
    if split:
        A = 2 * (rowsum / 2 / 2 ** 32 + Qh)   # two sredc'd half sums
        assert A < LIM
    S = (2 * A * Qh) / 2 ** 32 + Qh           # monomial combination
    msg = ""
    if fold:
        C0 = smul_b(max(fwd([Qh + 1] * 1024)))    # C = N^-1 NTT(acc)
        Cred = smul_b(C0 + 8 * S)
        assert max(C0, Cred) + 7 * S <= F
        msg = f", C {(max(C0, Cred) + 7 * S) / Q:.3f}Q"
    out = max(inv([S] * 1024))
    assert out < 3 * Q, f"inverse output {out / Q:.3f}Q"
    print(f"Q={Q} dig={dig} logG={logg} fold={fold}{' split' if split else ''}: fwd {F / Q:.3f}Q{msg}, S {S / Q:.3f}Q, "
          f"row sums 2^{rowsum.bit_length() if isinstance(rowsum, int) else __import__('math').log2(rowsum):.1f}, "
          f"inverse out {out / Q:.3f}Q (reductions {RED})  OK")


# the shapes blind_rotate_fast4.hip instantiates (fast4_shape_supported)
for shape in ((4, 7, True), (6, 5, True), (5, 5, False), (3, 9, False)):
    check(*shape)
check(4, 7, True, split=True)  # the SPLIT form (STD128 shape only)


# ---- fused radix-4 groups (fwd4f / inv4f, template parameter FU) ----
# A fused group reduces the sum of the two products that meet in its second stage once:
#   forward  t = smul(x2 w1); c = sredc(x1 w2 + x3 p21), d = sredc(x1 w3 + x3 n31); y = x0 +- t +- c|d
#   inverse  y1 = sredc(e wa + f wb), y3 = sredc(e pa + f pb), y2 = smul((s0 - s2) w1), y0 = s0 + s2 (RED: reduced)
# with e = x0 - x1, f = x2 - x3, s0 = x0 + x1, s2 = x2 + x3 and every twiddle and product |.| <= Q/2.
FU_ALL = (frozenset(range(5)), frozenset(range(5)))          # (forward passes, inverse passes) run fused
FU_PAIR = (frozenset((0, 1, 2, 3)), frozenset(range(5)))     # the pair instance's build: forward pass 4 plain


def sred2_b(y, z):
    """|sredc(y w + z v)| for |w|, |v| <= Q/2: the 64-bit sum stays far below 2^63 for 32-bit y, z"""
    assert y < LIM and z < LIM
    assert (y + z) * Qh < 2 ** 63 - 2 ** 58
    return (y + z) * Qh / 2 ** 32 + LIM * Q / 2 ** 32


def fwd_fused(b_in, fused, small=False):
    b = list(b_in)
    if small:
        b = [max(b_in) + 3 * (Qh + 1)] * 1024
    for p in range(1 if small else 0, 5):
        hi, lo = 1 << (9 - 2 * p), 1 << (8 - 2 * p)
        nb = list(b)
        for i in range(1024):
            if i & (hi | lo):
                continue
            x0, x1, x2, x3 = b[i], b[i | lo], b[i | hi], b[i | hi | lo]
            if p in fused:
                a = x0 + smul_b(x2)
                c = sred2_b(x1, x3)
                y = [a + c] * 4
            else:
                a0, a1 = x0 + smul_b(x2), x1 + smul_b(x3)
                assert max(a0, a1) < LIM
                y = [a0 + smul_b(a1)] * 4
            assert max(y) < LIM
            nb[i], nb[i | lo], nb[i | hi], nb[i | hi | lo] = y
        b = nb
    return b


def inv_fused(b_in, fused, red=RED):
    b = list(b_in)
    for p in range(5):
        lo, hi = 1 << (2 * p), 1 << (2 * p + 1)
        nb = list(b)
        for i in range(1024):
            if i & (hi | lo):
                continue
            x0, x1, x2, x3 = b[i], b[i | lo], b[i | hi], b[i | hi | lo]
            s0, s2 = x0 + x1, x2 + x3          # also |e|, |f|
            assert s0 + s2 < LIM, f"inverse pass {p}: {(s0 + s2) / Q:.2f}Q"
            if p in fused:
                y0 = smul_b(s0 + s2) if red[p] == "B" else s0 + s2
                y13 = sred2_b(s0, s2)
                y = [y0, y13, smul_b(s0 + s2), y13]
            else:
                u0, u1 = (smul_b(s0), smul_b(s2)) if red[p] == "A" else (s0, s2)
                v0, v1 = smul_b(s0), smul_b(s2)
                t0, t1 = u0 + u1, v0 + v1
                assert max(t0, t1) < LIM
                y = [smul_b(t0) if red[p] == "B" else t0, smul_b(t1) if red[p] == "B" else t1, smul_b(t0), smul_b(t1)]
            nb[i], nb[i | lo], nb[i | hi], nb[i | hi | lo] = y
        b = nb
    return b


def check_fused(fu=FU_ALL, quiet=False):
    """The STD128 shape (4 digits of 7 bits, folded) with the passes of fu fused: every 32-bit value < 2^31 (the
    asserts above), row sums < 2^63, the C bound and its eight-round reduction, the accumulator update window.
    Returns the proven magnitudes {F: transform outputs, S: inverse inputs, out: inverse outputs}."""
    ff, fi = fu
    dmax = 1 << 6
    F = max(max(fwd_fused([dmax] * 1024, ff)), max(fwd_fused([dmax] * 1024, ff, small=True)))
    rowsum = 2 * 3 * F * Qh + 2 * F * Qh
    assert rowsum < 2 ** 63
    A = rowsum / 2 ** 32 + Qh
    S = (2 * A * Qh) / 2 ** 32 + Qh
    C0 = smul_b(max(fwd_fused([Qh + 1] * 1024, ff)))
    Cred = smul_b(C0 + 8 * S)
    assert max(C0, Cred) + 7 * S <= F
    out = max(inv_fused([S] * 1024, fi))
    assert out < 3 * Q, f"inverse output {out / Q:.3f}Q"
    # no RED stage can go: without either one the inverse leaves the update window (or 32 bits)
    for p in (1, 3):
        try:
            o = max(inv_fused([S] * 1024, fi, {**RED, p: None}))
        except AssertionError:
            o = float("inf")
        assert o >= 3 * Q, f"RED of inverse pass {p} has become unnecessary"
    if not quiet:
        print(f"Q={Q} fused fwd {sorted(ff)} inv {sorted(fi)}: fwd {F / Q:.3f}Q, C {(max(C0, Cred) + 7 * S) / Q:.3f}Q, "
              f"S {S / Q:.3f}Q, inverse out {out / Q:.3f}Q (both reductions still needed)  OK")
    return {"F": F, "S": S, "out": out}


if __name__ == "__main__":
    check_fused(FU_ALL)
    check_fused(FU_PAIR)
