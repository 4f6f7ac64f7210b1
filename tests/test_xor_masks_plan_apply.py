"""CPU: the decode table of ecamd_xor_decode_masks, loaded through ctypes from libecamd_host.so
(ecamd_xor_decode_masks_plan), applied in numpy the way xor_decode_masks_kernel applies it -- the entry at
the rank of the mask, output r = XOR of the fragments in source mask r, the outputs >= k skipped without
decode_parity -- to random INCONSISTENT buffers with the lost slots zeroed, and compared over every buffer
with oracle/xor_oracle.py's decode of the same stripe.  On inconsistent buffers a wrong choice of parity
shows.  Every pattern of (3,3,3), (10,5,3) and (10,6,4), and 300 seeded patterns of (20,6,4)."""
import ctypes as C
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import xor_oracle as XO  # noqa: E402

ENTRY = np.dtype([("n_out", "u1"), ("out", "u1", 3), ("src", "<u4", 3)])
BS = 24


def table(k, m, hd):
    from liberasurecode_amd import _lib
    h = _lib.host()
    count = h.ecamd_xor_decode_masks_plan(k, m, hd, None, 0)
    assert count == sum(math.comb(k + m, t) for t in range(hd))
    raw = np.full((count + 1) * ENTRY.itemsize, 0xEE, np.uint8)
    assert h.ecamd_xor_decode_masks_plan(k, m, hd, raw.ctypes.data_as(C.c_void_p), count) == count
    assert (raw[count * ENTRY.itemsize:] == 0xEE).all()
    return raw[:count * ENTRY.itemsize].view(ENTRY)


def rank(n, lost):
    """offset[t] + C(f0,1) + C(f1,2) + C(f2,3) for the ascending list."""
    t = len(lost)
    return sum(math.comb(n, i) for i in range(t)) + sum(math.comb(f, i + 1) for i, f in enumerate(lost))


def every_pattern(n, hd):
    return [list(c) for t in range(hd) for c in itertools.combinations(range(n), t)]


def check_patterns(k, m, hd, patterns, seed):
    n = k + m
    tab = table(k, m, hd)
    code = XO.XorCode(k, m, hd)
    rng = np.random.default_rng(seed)
    for lost in patterns:
        before = rng.integers(0, 256, size=(n, BS), dtype=np.uint8)
        before[lost] = 0
        e = tab[rank(n, lost)]
        assert int(e["n_out"]) == len(lost) and [int(f) for f in e["out"][:len(lost)]] == lost, (lost, e)
        for dp in (1, 0):
            want = [np.array(x) for x in before]
            assert code.decode(want, lost, dp) == 0, lost
            got = before.copy()
            for r in range(int(e["n_out"])):
                f, src = int(e["out"][r]), int(e["src"][r])
                if not dp and f >= k:
                    continue
                assert src and not any(src >> x & 1 for x in lost) and src >> n == 0, (lost, hex(src))
                acc = np.zeros(BS, np.uint8)
                for x in range(n):
                    if src >> x & 1:
                        acc ^= before[x]
                got[f] = acc
            assert (got == np.stack(want)).all(), (lost, dp)


@pytest.mark.parametrize("k,m,hd,count", [(3, 3, 3, 22), (10, 5, 3, 121), (10, 6, 4, 697)])
def test_every_pattern(k, m, hd, count):
    patterns = every_pattern(k + m, hd)
    assert len(patterns) == count
    assert sorted(rank(k + m, p) for p in patterns) == list(range(count))
    check_patterns(k, m, hd, patterns, 4100 + k)


def test_300_seeded_patterns_of_20_6_4():
    k, m, hd = 20, 6, 4
    rng = np.random.default_rng(2064)
    patterns = [sorted(int(f) for f in rng.choice(k + m, size=int(rng.integers(1, hd)), replace=False)) for _ in range(300)]
    assert {len(p) for p in patterns} == {1, 2, 3}
    assert len(table(k, m, hd)) == 2952
    check_patterns(k, m, hd, patterns, 4120)


def test_a_rejected_code_has_no_table():
    from liberasurecode_amd import _lib
    for k, m, hd in ((10, 4, 3), (21, 6, 4), (10, 6, 5), (0, 6, 4), (12, 5, 4)):
        assert _lib.host().ecamd_xor_decode_masks_plan(k, m, hd, None, 0) == -1
