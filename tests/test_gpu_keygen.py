"""Key generation, encryption and decryption on the device against the oracle's or_keygen /
or_encrypt / or_decrypt, which draw from the same splitmix64 stream (include/tfhe_hip.h "The stream").

Everything except the words that carry a Gaussian must be identical.  A Gaussian is llround(3.19 z) with z from
log / cos / sqrt in double; host and device libraries may round log or cos differently in the last place, which
moves llround only when 3.19 z lies within ~1e-16 relative of a half-integer: about 1e-15 per draw.  The cap
(GAUSS_PER_DIFF): at most one differing Gaussian-carrying word per 2^24 of them, each by exactly +-1 mod its
modulus.  Every array compared here holds fewer than 2^24 such words except the BSK of STD128Q / LOGQ23 (2^24 and
1.3 * 2^24), so the cap is zero differences nearly everywhere; DESIGN 3.8 records the observed count.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import cube_lut, random_cts

pytestmark = pytest.mark.gpu

TRUTH = {"AND": lambda x, y: x & y, "OR": lambda x, y: x | y, "NAND": lambda x, y: 1 - (x & y),
         "NOR": lambda x, y: 1 - (x | y), "XOR": lambda x, y: x ^ y, "XNOR": lambda x, y: 1 - (x ^ y),
         "XOR_FAST": lambda x, y: x ^ y, "XNOR_FAST": lambda x, y: 1 - (x ^ y)}  # UnitTestFHEW.cpp truth tables

CONTEXTS = {
    "TOY": ("set", "TOY"),                          # N = 512, generic v1, qKS = Q (not a power of two), u32 KSK
    "STD128": ("set", "STD128"),                    # fast4, u16 KSK
    "STD128Q": ("set", "STD128Q"),                  # FP64 class, 64-bit words, u32 KSK
    "LOGQ23": ("logq", "STD128", False, 23, 0, 0, 1),  # 54-bit special form, qKS = 2^35 (u64 KSK)
}
ARB12 = ("logq", "STD128", True, 12, 0, 0, 1)
SEED = 7
GAUSS_PER_DIFF = 1 << 24


def make_params(module, spec):
    return module.params_from_set(spec[1]) if spec[0] == "set" else module.params_from_logq(*spec[1:])


def gauss_diffs(got, want, mod, what):
    """Number of differing Gaussian-carrying words; asserts the cap and that each differs by +-1 mod `mod`."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    idx = np.flatnonzero(got != want)
    print(f"{what}: {idx.size} of {got.size} Gaussian-carrying words differ")
    assert idx.size * GAUSS_PER_DIFF <= got.size, f"{what}: {idx.size} differing words of {got.size}"
    for i in idx:
        d = (int(got[i]) - int(want[i])) % mod
        assert d in (1, mod - 1), f"{what}[{i}]: {got[i]} vs {want[i]}"
    return idx.size


@pytest.fixture(scope="module", params=list(CONTEXTS))
def keys(request, oracle):
    """One context at a time (module-scoped parameter: the tests of a context run together): its parameters and
    the oracle's keys of SEED, computed once."""
    import tfhe_amd

    spec = CONTEXTS[request.param]
    op, cp = make_params(oracle, spec), make_params(tfhe_amd, spec)
    rng = oracle.Rng(SEED)
    sk, bsk, ksk = oracle.keygen(op, rng)
    for a in (sk, bsk, ksk):
        a.setflags(write=False)
    return dict(name=request.param, op=op, cp=cp, sk=sk, bsk=bsk, ksk=ksk, seed_after=rng.s, diffs={})


def test_keys_equal_oracle(keys):
    import tfhe_amd

    cp = keys["cp"]
    sk, bsk, ksk = tfhe_amd.keygen(cp, SEED)
    assert tfhe_amd.keygen.seed_after == keys["seed_after"]
    assert np.array_equal(sk, keys["sk"])
    k_got, k_want = ksk.reshape(-1, cp.n + 1), keys["ksk"].reshape(-1, cp.n + 1)
    assert np.array_equal(k_got[:, :cp.n], k_want[:, :cp.n]), "KSK A words"
    b_got, b_want = bsk.reshape(-1, 2, cp.N), keys["bsk"].reshape(-1, 2, cp.N)
    assert np.array_equal(b_got[:, 0], b_want[:, 0]), "BSK a polynomials"
    keys["diffs"]["ksk"] = gauss_diffs(k_got[:, cp.n], k_want[:, cp.n], cp.qKS, f"{keys['name']} KSK B")
    keys["diffs"]["bsk"] = gauss_diffs(b_got[:, 1], b_want[:, 1], cp.Q, f"{keys['name']} BSK b")


def test_arena_path_equals_host_path(keys):
    """tfhe_setup_keygen's context against tfhe_setup on the oracle's keys of the same seed: the same key image,
    byte for byte, and the same gate outputs (the derived key forms)."""
    import torch

    import tfhe_amd

    # the images can only be compared where the keys agree exactly (test_keys_equal_oracle's count, when it ran)
    assert not any(keys["diffs"].values()), "a +-1 Gaussian word at this seed: compare at another seed"
    cp = keys["cp"]
    A, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, SEED)
    assert A.seed_after == keys["seed_after"]
    assert np.array_equal(sk, keys["sk"])
    B = tfhe_amd.BinFHEContextHIP(cp).GPUSetup(keys["bsk"], keys["ksk"])
    try:
        nbytes = A.info().key_image_bytes
        assert nbytes == B.info().key_image_bytes
        imgs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
        A.export_key_image(imgs[0].data_ptr(), nbytes)
        B.export_key_image(imgs[1].data_ptr(), nbytes)
        torch.cuda.synchronize()
        assert torch.equal(imgs[0], imgs[1]), "key images differ"
        del imgs
        rs = np.random.default_rng(11)
        for batch in (3, 5) if keys["name"] == "TOY" else (3,):
            c1, c2 = random_cts(rs, batch, cp.n, cp.q), random_cts(rs, batch, cp.n, cp.q)
            for gate in ("NAND", "XOR"):
                assert np.array_equal(A.EvalBinGate(gate, c1, c2), B.EvalBinGate(gate, c1, c2)), gate
    finally:
        A.GPUClean()
        B.GPUClean()


@pytest.fixture(scope="module")
def q128(oracle):
    import tfhe_amd

    op, cp = oracle.params_from_set("STD128Q"), tfhe_amd.params_from_set("STD128Q")
    s = np.random.default_rng(5).integers(-1, 2, cp.n)
    sk = np.where(s < 0, cp.qKS - 1, s).astype(np.uint64)
    return op, cp, sk, tfhe_amd.BinFHEContextHIP(cp)


def messages(B, p):
    """negative, >= p and in-range messages"""
    base = [-3, p, 1, -p - 3, 2 * p + 1, 0, -1, p - 1]
    return [base[i % len(base)] + (i // len(base)) for i in range(B)]


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("pm", [(4, None), (1 << 15, 1 << 23)], ids=["p4_q", "p2^15_2^23"])
def test_encrypt_decrypt_equal_oracle(oracle, q128, B, pm):
    op, cp, sk, cc = q128
    p, mod = pm[0], pm[1] or cp.q
    seed = 100 + B
    msgs = messages(B, p)
    rng = oracle.Rng(seed)
    want = np.stack([oracle.encrypt(op, rng, sk, m, p, mod) for m in msgs])
    got = cc.Encrypt(sk, msgs, p=p, mod=mod, seed=seed)
    assert cc.seed_after == rng.s
    assert got.shape == (B, cp.n + 1)
    assert np.array_equal(got[:, :cp.n], want[:, :cp.n])
    gauss_diffs(got[:, cp.n], want[:, cp.n], mod, "ciphertext b")
    rand = random_cts(np.random.default_rng(B), B, cp.n, mod)
    for cts in (got, rand):
        assert cc.Decrypt(sk, cts, p=p, mod=mod) == [oracle.decrypt(op, sk, c, p, mod) for c in cts]
    assert cc.Decrypt(sk, got, p=p, mod=mod) == [m % p for m in msgs]


def test_encrypt_decrypt_device_pointers(q128):
    import torch

    _, cp, sk, cc = q128
    B, p, mod, seed = 5, 1 << 15, 1 << 23, 321
    msgs = messages(B, p)
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_m = torch.tensor(msgs, dtype=torch.int64, device="cuda")
    d_ct = torch.zeros(B * (cp.n + 1), dtype=torch.int64, device="cuda")
    d_out = torch.zeros(B, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    after = cc.EncryptDevice(B, d_sk.data_ptr(), d_m.data_ptr(), d_ct.data_ptr(), p=p, mod=mod, seed=seed)
    cc.DecryptDevice(B, d_sk.data_ptr(), d_ct.data_ptr(), d_out.data_ptr(), p=p, mod=mod)
    torch.cuda.synchronize()
    host = cc.Encrypt(sk, msgs, p=p, mod=mod, seed=seed)
    assert after == cc.seed_after
    assert np.array_equal(d_ct.cpu().numpy().view(np.uint64).reshape(B, -1), host)
    assert d_out.cpu().tolist() == [m % p for m in msgs]


@pytest.mark.parametrize("name", ["TOY", "STD128"])
def test_gates_end_to_end_device_keys(name):
    """test_paramset_gates_decrypt with keys, ciphertexts and decryption from the device alone."""
    import tfhe_amd

    cc, sk = tfhe_amd.BinFHEContextHIP.from_keygen(tfhe_amd.params_from_set(name), seed=31)
    m1, m2 = [0, 0, 1, 1], [0, 1, 0, 1]
    c1 = cc.Encrypt(sk, m1, p=4, seed=1000)
    c2 = cc.Encrypt(sk, m2, p=4, seed=cc.seed_after)
    for gate, f in TRUTH.items():
        assert cc.Decrypt(sk, cc.EvalBinGate(gate, c1, c2), p=4) == [f(x, y) for x, y in zip(m1, m2)], gate
    cc.GPUClean()


def test_eval_func_end_to_end_device_keys():
    import tfhe_amd

    cp = make_params(tfhe_amd, ARB12)
    cc, sk = tfhe_amd.BinFHEContextHIP.from_keygen(cp, seed=47)
    ms = list(range(8))
    out = cc.EvalFunc(cc.Encrypt(sk, ms, p=8, seed=5), cube_lut(cp.q))
    assert cc.Decrypt(sk, out, p=8) == [m ** 3 % 8 for m in ms]
    cc.GPUClean()


def test_keygen_device_optional_keys_and_bounds():
    """TOY: with d_bsk_coeff or d_ksk NULL the other key is written identically, and nothing is written behind
    the end of sk, BSK or KSK (guard words keep their pattern)."""
    import torch

    import tfhe_amd

    cp = tfhe_amd.params_from_set("TOY")
    L, guard, fill = tfhe_amd.lib(), 4096, 0x5A5A5A5A5A5A5A5A

    def run(want_bsk, want_ksk):
        sizes = dict(sk=cp.n, bsk=cp.bsk_words() if want_bsk else 0, ksk=cp.ksk_words() if want_ksk else 0)
        bufs = {k: torch.full((w + guard,), fill, dtype=torch.int64, device="cuda") for k, w in sizes.items()}
        torch.cuda.synchronize()
        ptr = {k: C.c_void_p(bufs[k].data_ptr() if sizes[k] else None) for k in bufs}
        after = C.c_uint64()
        tfhe_amd.capi.check(L.tfhe_keygen_device(C.byref(cp), SEED, 0, ptr["sk"], ptr["bsk"], ptr["ksk"],
                                                 C.byref(after), None), "tfhe_keygen_device")
        out = {}
        for k, w in sizes.items():
            h = bufs[k].cpu().numpy()
            assert (h[w:] == fill).all(), f"{k}: guard words overwritten"
            out[k] = h[:w]
        return out, after.value

    both, after = run(True, True)
    only_ksk, after_k = run(False, True)
    only_bsk, after_b = run(True, False)
    assert after == after_k == after_b
    assert np.array_equal(both["ksk"], only_ksk["ksk"]) and np.array_equal(both["bsk"], only_bsk["bsk"])
    assert np.array_equal(both["sk"], only_ksk["sk"]) and np.array_equal(both["sk"], only_bsk["sk"])
    assert not (both["bsk"] == fill).all() and not (both["ksk"] == fill).all()
