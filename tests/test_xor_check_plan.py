"""CPU: the flat XOR check / locate plan (ecamd_xor_check_plan, include/ecamd_host.h).

The signatures are compared with the ones derived from the parity bitmaps (xor_util.tables), and the
locate rule they define -- per 16-bit word, fragment f explains the word iff all its non-zero
syndromes are equal and the set of rows with a non-zero syndrome is sig[f]; a stripe's suspects are
the AND over its dirty words -- is run as a numpy model against oracle/xor_oracle.py (through the
definitions of test_gpu_locate_sweep).  No device is needed: the fused kernel and the GPU tests take
`sig` from this one function."""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_gpu_locate_sweep as SW
import xor_util as X
from liberasurecode_amd import _lib

XO = SW.XO


def plan(k, m, hd):
    sig = (C.c_uint * (k + m))(*([0xDEAD] * (k + m)))
    rc = _lib.host().ecamd_xor_check_plan(k, m, hd, sig)
    return rc, [int(x) for x in sig]


def derived(k, m, hd):
    pb, _ = X.tables(k, m, hd)
    return [sum(1 << p for p in range(m) if pb[p] >> j & 1) for j in range(k)] + [1 << p for p in range(m)]


def sum_triple(sig):
    """The first (f1, f2, f3) with sig[f1] ^ sig[f2] == sig[f3], or None."""
    for f1, f2 in itertools.combinations(range(len(sig)), 2):
        for f3 in range(len(sig)):
            if f3 not in (f1, f2) and sig[f1] ^ sig[f2] == sig[f3]:
                return f1, f2, f3
    return None


def model_locate(k, m, hd, sig, held):
    """(status, suspects) of (S, k+m, bs) stripes by the rule alone, bs even."""
    pb, _ = X.tables(k, m, hd)
    nS, n, bs = held.shape
    words = np.ascontiguousarray(held).view("<u2")  # (S, n, bs / 2)
    status = np.zeros(nS, np.uint32)
    suspects = np.zeros(nS, np.uint32)
    for s in range(nS):
        syn = np.array(words[s, k:])
        for p in range(m):
            for j in range(k):
                if pb[p] >> j & 1:
                    syn[p] ^= words[s, j]
        keep = (1 << n) - 1
        for w in np.nonzero(syn.any(axis=0))[0]:
            col = [int(x) for x in syn[:, w]]
            rows = sum(1 << p for p in range(m) if col[p])
            status[s] |= np.uint32(rows << k)
            equal = len({x for x in col if x}) == 1
            keep &= sum(1 << f for f in range(n) if equal and sig[f] == rows)
        suspects[s] = keep if status[s] else 0
    return status, suspects


def test_all_38_codes_match_the_bitmaps_and_are_distinct():
    assert len(X.XOR_CODES) == 38
    for k, m, hd in X.XOR_CODES:
        rc, sig = plan(k, m, hd)
        assert rc == 0 and sig == derived(k, m, hd), (k, m, hd)
        assert all(sig) and len(set(sig)) == k + m, (k, m, hd, sig)
        assert m in (3, 5, 6) and k <= 20 and max(sig) < 1 << m


@pytest.mark.parametrize("k,m,hd", [(10, 4, 9), (10, 6, 5), (21, 6, 4), (3, 3, 4), (4, 3, 3), (0, 6, 3)])
def test_rejected_code(k, m, hd):
    sig = (C.c_uint * 32)(*([0xDEAD] * 32))
    assert _lib.host().ecamd_xor_check_plan(k, m, hd, sig) == -1
    assert all(x == 0xDEAD for x in sig)


def test_3_3_3_has_a_pair_that_reads_as_a_third():
    rc, sig = plan(3, 3, 3)
    assert rc == 0
    t = sum_triple(sig)
    assert t is not None
    f1, f2, f3 = t
    assert len({f1, f2, f3}) == 3 and sig[f1] ^ sig[f2] == sig[f3]


@pytest.mark.parametrize("k,m,hd", [(10, 6, 4), (3, 3, 3), (20, 6, 4)])
def test_rule_finds_every_single_and_agrees_with_the_oracle_on_same_word_pairs(k, m, hd):
    n, bs = k + m, 32
    rc, sig = plan(k, m, hd)
    assert rc == 0
    rng = np.random.default_rng(77 + k)
    pairs = list(itertools.combinations(range(n), 2))
    if len(pairs) > 15:
        pairs = [pairs[i] for i in rng.choice(len(pairs), 15, replace=False)]
    t = sum_triple(sig)
    if t and (t[0], t[1]) not in pairs:
        pairs.append((t[0], t[1]))
    nS = 1 + n + 2 * len(pairs)
    good = np.empty((nS, n, bs), np.uint8)
    for s in range(nS):
        good[s, :k] = rng.integers(0, 256, size=(k, bs), dtype=np.uint8)
        good[s, k:] = XO.encode_bytes(k, m, hd, good[s, :k])
    bad = good.copy()
    for f in range(n):  # stripe 1 + f: fragment f alone, two different words
        for w in rng.choice(bs // 2, 2, replace=False):
            SW.xor_word(bad, 1 + f, f, 2 * int(w), int(rng.integers(1, 0x10000)))
    same = {}
    for i, (f1, f2) in enumerate(pairs):  # one word: the same error in both, then different errors
        s, p, v = 1 + n + 2 * i, 2 * int(rng.integers(0, bs // 2)), int(rng.integers(1, 0x10000))
        SW.xor_word(bad, s, f1, p, v)
        SW.xor_word(bad, s, f2, p, v)
        same[s] = (f1, f2)
        SW.xor_word(bad, s + 1, f1, p, v)
        SW.xor_word(bad, s + 1, f2, p, v ^ int(rng.integers(1, 0x10000)))
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, bad)
    st, su = model_locate(k, m, hd, sig, bad)
    assert (st == want_st).all() and (su == want_su).all(), [(int(s), hex(int(su[s])), hex(int(want_su[s])))
                                                             for s in np.nonzero(su != want_su)[0][:6]]
    assert not st[0] and not su[0]
    for f in range(n):
        assert st[1 + f] and su[1 + f] == 1 << f, (f, hex(int(su[1 + f])))
    for s, (f1, f2) in same.items():  # a same-word pair reads as f3 exactly where the signatures add up
        third = [f for f in range(n) if sig[f] == sig[f1] ^ sig[f2]]
        assert su[s] == sum(1 << f for f in third), (f1, f2, hex(int(su[s])))
