"""The shared twiddle table of the 4-wavefront kernel's fused passes 1-3 in LDS (blind_rotate_fast4.hip, FU_L):
84 blocks [w1, w2, w3, p21] (pass 1: 4 blocks, pass 2: 16, pass 3: 64) followed by the 84 n31 words, one per block,
420 words inside the 672 the forward and inverse tables occupy otherwise.  Pass 3's blocks stand in the order of
the lanes that read them (k_pack_tables4), which mirrors like the block index: lane l's inverse block is lane
63 - l's.  A lane reads its block with one ds_read_b128 and its n31 word with one ds_read_b32; the forward pass
reads block c, the inverse block m - 1 - c.
Checks that every read stays inside the table and is conflict-free: ds_read_b128 in its four 16-lane groups over
64 banks, ds_read_b32 in two 32-lane groups over 32 banks (lanes reading the same address share one access).
Run: python3 tools/lds_tables4.py"""
from lds_layouts4 import elem

BLK_WORDS, N31_AT, AREA = 4 * 84, 4 * 84, 672
# pass: (layout the pass runs in, index bits above the pass's pair, first block, blocks)
PASSES = {1: (2, 8, 0, 4), 2: (3, 6, 4, 16), 3: (4, 4, 20, 64)}
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]
B32_GROUPS = [list(range(32)), list(range(32, 64))]


def conflicts(groups, addr, words, banks):
    """worst number of distinct addresses of one group that meet in a bank"""
    worst = 0
    for g in groups:
        hit = {}
        for lane in g:
            for k in range(words):
                hit.setdefault((addr[lane] + k) % banks, set()).add(addr[lane] + k)
        worst = max(worst, max(len(s) for s in hit.values()))
    return worst


def check():
    assert N31_AT + 84 <= AREA
    for p, (L, shift, first, m) in PASSES.items():
        for inverse in (False, True):
            worst128 = worst32 = 0
            for w in range(4):
                c = [elem(L, w, lane, 0) >> shift for lane in range(64)]
                assert all(0 <= v < m for v in c) and all(elem(L, w, lane, r) >> shift == c[lane]
                                                          for lane in range(64) for r in range(4))
                if p == 3:  # lane order: position = the lane that holds block c in a forward pass
                    pos = {v: lane for lane, v in enumerate(c)}
                    assert sorted(pos) == list(range(64)) and all(pos[63 - v] == 63 - pos[v] for v in c)
                    assert all(v == (q & 7) | ((q & 8) << 1) | ((q & 16) << 1) | ((q & 32) >> 2) for v, q in pos.items())
                    c = [pos[v] for v in c]
                blk = [first + (m - 1 - v if inverse else v) for v in c]
                assert all(first <= b < first + m for b in blk)
                worst128 = max(worst128, conflicts(B128_GROUPS, [4 * b for b in blk], 4, 64))
                worst32 = max(worst32, conflicts(B32_GROUPS, [N31_AT + b for b in blk], 1, 32))
            print(f"pass {p} {'inverse' if inverse else 'forward'}: {m} blocks, ds_read_b128 max {worst128}-way, "
                  f"ds_read_b32 (n31) max {worst32}-way")
            assert worst128 == 1 and worst32 == 1
    print(f"shared table: {N31_AT + 84} of {AREA} words")


if __name__ == "__main__":
    check()
