"""One table per channel in numpy (no GPU): the index rule t(i) = (i // inner) % T, three different tables
of each class of checkInputFunction, and the composition the tabled calls are compared against: the shared-table
EvalFunc once per table, on that table's ciphertexts."""
import numpy as np

from helpers import cube_lut

KINDS = ["negacyclic", "periodic", "arbitrary"]
CLASS = {"negacyclic": 0, "periodic": 1, "arbitrary": 2}
BOOTSTRAPS = np.array([1, 2, 2])  # per ciphertext, by class


def luts3(q):
    """kind -> three different tables of that class: tests/test_gpu_dense.py's constructions, and the same with
    other multipliers (x^2 mod q/2; another plaintext modulus for the cube, and x^3 + 1), so that a wrong table of the right
    class shows."""
    h = q // 2

    def neg(k):  # lut[i] == q - lut[h + i] for every i < h
        return np.array([1 + (k * x) % (q - 1) if x < h else q - 1 - (k * (x - h)) % (q - 1) for x in range(q)],
                        dtype=np.uint64)

    def per(k):
        return np.array([(x * k) % h for x in range(q)], dtype=np.uint64)

    per2 = np.array([(x * x) % h for x in range(q)], dtype=np.uint64)  # (x + h)^2 = x^2 mod h
    arb3 = np.array([(x * x * x + 1) % q for x in range(q)], dtype=np.uint64)
    return {"negacyclic": [neg(3), neg(5), neg(7)], "periodic": [per(5), per(7), per2],
            "arbitrary": [cube_lut(q), cube_lut(q, 4), arb3]}


def tables(q, kinds):
    """[len(kinds), q]: table k is of class kinds[k]; a class that appears again gets its next table (of three)."""
    three, seen, out = luts3(q), {}, []
    for k in kinds:
        out.append(three[k][seen.get(k, 0) % 3])
        seen[k] = seen.get(k, 0) + 1
    return np.stack(out)


def table_of(B, inner, T):
    """t(i) for i < B."""
    return (np.arange(B) // inner) % T


def counts(classes, B, inner):
    """(per_class[3], bootstraps) of a batch of B, written out: one pass over the ciphertexts."""
    c = np.asarray(classes)[table_of(B, inner, len(classes))]
    per = [int((c == k).sum()) for k in range(3)]
    return per, int(BOOTSTRAPS[c].sum())


def compose(eval_func, cts, luts, inner, q):
    """out[i] = eval_func(cts[i], luts[t(i)]): one shared-table call per table, on the rows of that table."""
    cts = np.asarray(cts, dtype=np.uint64)
    t = table_of(cts.shape[0], inner, len(luts))
    out = np.empty_like(cts)
    for k in range(len(luts)):
        rows = np.flatnonzero(t == k)
        if rows.size:
            out[rows] = eval_func(np.ascontiguousarray(cts[rows]), luts[k], q)
    return out
