"""CPU: the flat XOR check plan for stripes with fragments missing (ecamd_xor_check_plan_degraded,
include/ecamd_host.h).

Expected values never come from the code under test: `reduce` restates the header's reduction rule from
the parity_bms of tests/golden/xor_codes.json, and the rule-independent properties (no missing fragment
in a surviving row, every surviving row in the row space of the original ones, the survivor count by
rank, the owner parity in its row) are checked with plain GF(2) elimination on integers.  Swept: all 38
codes, every missing set of size 0, 1 and 2 and a seeded sample of 50 sets of each size 3..m."""
import ctypes as C
import itertools
import json
import os
import random

import pytest

from liberasurecode_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "xor_codes.json")) as fh:
    CODES = [(c["k"], c["m"], c["hd"], [int(x) for x in c["parity_bms"]]) for c in json.load(fh)]
CANARY = 0xDEAD


def reduce(k, m, pb, missing):
    """The header's rule: (rows, sig, covered, survivors)."""
    rows = [pb[p] | 1 << (k + p) for p in range(m)]
    live = [True] * m
    for f in sorted(missing):
        have = [p for p in range(m) if live[p] and rows[p] >> f & 1]
        if not have:
            continue
        for p in have[1:]:
            rows[p] ^= rows[have[0]]
        live[have[0]] = False
    rows = [rows[p] if live[p] else 0 for p in range(m)]
    sig = [sum(1 << p for p in range(m) if rows[p] >> f & 1) for f in range(k + m)]
    return rows, sig, sum(1 << f for f in range(k + m) if sig[f]), sum(live)


def plan(k, m, hd, missing, null=False):
    """(rc, rows, sig, covered) of the library, every output canary-filled first."""
    rows = (C.c_uint * 32)(*([CANARY] * 32))
    sig = (C.c_uint * 32)(*([CANARY] * 32))
    covered = C.c_uint(CANARY)
    lst = None if null else _lib.ints(list(missing) + [-1])
    rc = _lib.host().ecamd_xor_check_plan_degraded(k, m, hd, lst, rows, sig, C.byref(covered))
    return rc, [int(x) for x in rows], [int(x) for x in sig], int(covered.value)


def rank(vectors):
    """Rank over GF(2) of integers taken as bit vectors."""
    basis = []
    for v in vectors:
        for b in basis:
            v = min(v, v ^ b)
        if v:
            basis.append(v)
    return len(basis)


def missing_sets(k, m, seed):
    n = k + m
    sets = [list(c) for r in (0, 1, 2) for c in itertools.combinations(range(n), r)]
    rnd = random.Random(seed)
    for r in range(3, m + 1):
        sets += [sorted(rnd.sample(range(n), r)) for _ in range(50)]
    return sets


def test_golden_file_has_the_38_codes():
    assert len(CODES) == 38 and len({c[:3] for c in CODES}) == 38


@pytest.mark.parametrize("k,m,hd,pb", CODES, ids=["%d_%d_%d" % c[:3] for c in CODES])
def test_plan_equals_the_rule_and_has_its_properties(k, m, hd, pb):
    n = k + m
    full = [pb[p] | 1 << (k + p) for p in range(m)]
    for i, missing in enumerate(missing_sets(k, m, 100 * k + 10 * m + hd)):
        listed = missing[::-1] if i % 3 == 1 else missing  # the order of the list does not matter
        rc, rows, sig, covered = plan(k, m, hd, listed)
        want_rows, want_sig, want_cov, want_rc = reduce(k, m, pb, missing)
        assert (rc, rows[:m], sig[:n], covered) == (want_rc, want_rows, want_sig, want_cov), (k, m, hd, missing)
        assert all(x == CANARY for x in rows[m:] + sig[n:]), "written past m rows / k+m signatures"
        lost = sum(1 << f for f in missing)
        alive = [p for p in range(m) if rows[p]]
        # rule-independent
        assert len(alive) == rc == m - rank([sum((full[p] >> f & 1) << p for p in range(m)) for f in missing]), missing
        for p in alive:
            assert not rows[p] & lost and rows[p] >> (k + p) & 1, (missing, p)
            assert rank(full + [rows[p]]) == m, (missing, p)  # in the row space of the original rows
        assert rank([rows[p] for p in alive]) == len(alive)
        for f in range(n):
            assert sig[f] == sum(1 << p for p in range(m) if rows[p] >> f & 1)
            assert not (lost >> f & 1 and sig[f])
        assert covered == sum(1 << f for f in range(n) if sig[f]) and not covered & lost
        if len(missing) <= hd - 2:
            assert covered == (1 << n) - 1 - lost, (k, m, hd, missing, hex(covered))
        if hd == 4 and len(missing) == 1:
            avail = [sig[f] for f in range(n) if f not in missing]
            assert len(set(avail)) == len(avail), (k, m, hd, missing)


@pytest.mark.parametrize("k,m,hd,pb", CODES, ids=["%d_%d_%d" % c[:3] for c in CODES])
def test_nothing_missing_is_the_full_plan(k, m, hd, pb):
    full = (C.c_uint * (k + m))()
    assert _lib.host().ecamd_xor_check_plan(k, m, hd, full) == 0
    for null in (False, True):
        rc, rows, sig, covered = plan(k, m, hd, [], null)
        assert rc == m and rows[:m] == [pb[p] | 1 << (k + p) for p in range(m)]
        assert sig[:k + m] == [int(x) for x in full] and covered == (1 << (k + m)) - 1


def test_covered_may_be_null():
    k, m, hd = 10, 6, 4
    rows, sig = (C.c_uint * m)(), (C.c_uint * (k + m))()
    assert _lib.host().ecamd_xor_check_plan_degraded(k, m, hd, _lib.ints([3, -1]), rows, sig, None) == m - 1
    assert [int(x) for x in rows] == reduce(k, m, dict((c[:3], c[3]) for c in CODES)[(k, m, hd)], [3])[0]


def test_too_many_lost_leaves_fragments_uncovered_and_can_leave_no_row():
    k, m, hd = 3, 3, 3
    rc, rows, sig, covered = plan(k, m, hd, [3, 4, 5])  # every parity lost: every row is retired
    assert rc == 0 and rows[:m] == [0, 0, 0] and sig[:k + m] == [0] * 6 and covered == 0
    rc, rows, sig, covered = plan(k, m, hd, [0, 1, 2])  # every data fragment lost: the parities still sum to zero
    assert rc == 1 and covered == 0b111000 and sorted(rows[:m]) == [0, 0, 0b111000]
    k, m, hd = 10, 6, 4
    rc, rows, sig, covered = plan(k, m, hd, [0, 1, 2])  # hd - 1 lost: some available fragment is in no check
    assert rc == 3 and covered != (1 << 16) - 1 - 0b111


@pytest.mark.parametrize("k,m,hd,missing", [
    (10, 6, 4, [16]),               # out of range
    (10, 6, 4, [3, 400]),
    (10, 6, 4, [3, 5, 3]),          # repeated
    (10, 6, 4, [0, 1, 2, 3, 4, 5, 6]),  # more than m entries
    (3, 3, 3, [0, 1, 2, 3]),
    (10, 4, 9, [1]),                # codes init_xor_hd_code rejects
    (21, 6, 4, []),
    (3, 3, 4, [0]),
    (0, 6, 3, []),
])
def test_rejects_leave_the_outputs_untouched(k, m, hd, missing):
    rc, rows, sig, covered = plan(k, m, hd, missing)
    assert rc == -1
    assert all(x == CANARY for x in rows + sig) and covered == CANARY
