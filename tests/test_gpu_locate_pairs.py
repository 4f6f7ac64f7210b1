"""GPU: two bad fragments per stripe (ecamd_rs_locate_pairs / ecamd_rs_scrub_pairs, include/ecamd.h).

Expected values never come from the code under test.  Stripes are the reference encode's
(test_gpu_check.stripes); the damaged pair of a stripe is known by construction, and for a sample the
reference codec confirms it: {a, b} is the pair iff replacing a and b by the reference's decode with
both listed as missing makes test_gpu_check.oracle_status zero, and no other pair does.  d_status and
d_suspects must be what ecamd_rs_locate writes for the same data, word for word."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle_lib as orc
import test_gpu_check as TC
from test_gpu_check import D, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
TAIL = TC.TAIL
EINVAL = -22
CANARY = 0xA5
CANARY32 = CANARY * 0x01010101


def bits(*frags):
    return sum(1 << f for f in frags)


def hexes(x):
    return [hex(int(v)) for v in x]


def damage_pair(stripe, a, b, placement, tile):
    """Two damaged fragments in one of four placements: the same 16-bit word; two tiles; a tile against
    the tail; a high-byte-only against a low-byte-only error (of one word)."""
    w = 2 * (37 + 5 * a + b)
    if placement == 0:
        stripe[a, w] ^= 0x11
        stripe[a, w + 1] ^= 0x80
        stripe[b, w] ^= 0x02
        stripe[b, w + 1] ^= 0x3C
    elif placement == 1:
        stripe[a, w] ^= 0x40
        stripe[b, tile + w + 1] ^= 0x07
    elif placement == 2:
        stripe[a, tile + w] ^= 0x01
        stripe[b, 2 * tile + 2 * (b % 24)] ^= 0x99
    else:
        stripe[a, w + 1] ^= 0x20
        stripe[b, w] ^= 0x04


_batch = {}


def batch_10_4():
    """(held, want_pairs, want_suspects): the 91 pairs of (10,4), a clean stripe, 14 single-damaged."""
    if not _batch:
        k, m = 10, 4
        bs = 2 * TC.tile_of(m) + TAIL
        full = TC.stripes(k, m, bs)
        pairs = list(itertools.combinations(range(k + m), 2))
        n = len(pairs) + 1 + k + m
        held = np.stack([full[s % TC.S] for s in range(n)])
        want_pairs, want_suspects = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        for i, (a, b) in enumerate(pairs):
            damage_pair(held[i], a, b, i % 4, TC.tile_of(m))
            want_pairs[i] = bits(a, b)
        for f in range(k + m):
            s = len(pairs) + 1 + f
            held[s, f, 100 + 3 * f] ^= 0x5A
            held[s, f, bs - 1 - f] ^= 0x01
            want_suspects[s] = 1 << f
        held.setflags(write=False)
        _batch["v"] = (held, want_pairs, want_suspects)
    return _batch["v"]


def upload(D, held):
    lay = D.Layout.alloc(held.shape[1], held.shape[2], held.shape[0])
    lay.upload_stripes(np.ascontiguousarray(held))
    return lay


def locate_pairs_and_locate(D, k, m, held, missing=()):
    """rs_locate_pairs of the stripes, checked against rs_locate of the same data: (status, suspects, pairs)."""
    lay = upload(D, held)
    try:
        st, su, pr, checked = D.rs_locate_pairs(k, m, lay, missing)
        st0, su0, checked0 = D.rs_locate(k, m, lay, missing)
    finally:
        lay.buf.free()
    assert checked == checked0
    assert st.tobytes() == st0.tobytes() and su.tobytes() == su0.tobytes(), (hexes(st), hexes(st0), hexes(su), hexes(su0))
    return st, su, pr


def raw_pairs(dev, D, k, m, missing, base, stripe_stride, frag_stride, bs, nstripes, null_pairs=False, extra=2):
    """ecamd_rs_locate_pairs on explicit pointers into canary-filled arrays of nstripes + extra words."""
    from liberasurecode_amd import _lib
    n = nstripes + extra
    arrs = [D.DeviceBuffer(4 * n) for _ in range(3)]
    for a in arrs:
        dev.ecamd_memset(a.ptr, CANARY, a.nbytes)
    checked = C.c_uint32(0xFFFFFFFF)
    rc = dev.ecamd_rs_locate_pairs(k, m, _lib.ints(list(missing) + [-1]), base, stripe_stride, frag_stride, bs, nstripes,
                                   arrs[0].ptr, arrs[1].ptr, None if null_pairs else arrs[2].ptr, C.byref(checked), None)
    dev.ecamd_synchronize()
    out = [a.download().view(np.uint32).copy() for a in arrs]
    for a in arrs:
        a.free()
    return (rc, *out, checked.value)


@pytest.mark.parametrize("k,m", [(10, 4), (20, 8)])
def test_clean_batch_writes_zeros_and_nothing_past_nstripes(D, dev, k, m):
    bs = 2 * TC.tile_of(m) + TAIL
    lay = upload(D, np.array(TC.stripes(k, m, bs)))
    try:
        n0 = dev.ecamd_locate_pairs_launches()
        rc, st, su, pr, checked = raw_pairs(dev, D, k, m, [], lay.buf.ptr, lay.stripe_stride, lay.frag_stride, bs, TC.S)
        assert dev.ecamd_locate_pairs_launches() == n0 + 1  # launched; its workgroups find nothing to do
    finally:
        lay.buf.free()
    assert rc == 0 and checked == bits(*range(k, k + m))
    for a in (st, su, pr):
        assert not a[:TC.S].any() and (a[TC.S:] == CANARY32).all(), hexes(a)


def test_every_pair_of_10_4(D, dev):
    k, m = 10, 4
    held, want_pairs, want_suspects = batch_10_4()
    st, su, pr = locate_pairs_and_locate(D, k, m, held)
    assert (su == want_suspects).all(), (hexes(su), hexes(want_suspects))
    assert (pr == want_pairs).all(), [(s, hex(int(pr[s])), hex(int(want_pairs[s]))) for s in np.nonzero(pr != want_pairs)[0]]
    assert ((st != 0) == ((want_pairs | want_suspects) != 0)).all()


def test_oracle_by_repair(D, dev):
    """Eight stripes of the batch, two of each placement: exactly the reported pair repairs the stripe."""
    k, m = 10, 4
    held, want_pairs, _ = batch_10_4()
    lay = upload(D, held)
    try:
        _, _, pr, _ = D.rs_locate_pairs(k, m, lay)
    finally:
        lay.buf.free()
    for s in (0, 1, 2, 3, 36, 57, 78, 87):
        repairs = 0
        for c, d in itertools.combinations(range(k + m), 2):
            frags = [np.array(x) for x in held[s]]
            assert orc.decode(k, m, frags, [c, d]) == 0
            trial = np.stack(frags)[None]
            if not TC.oracle_status(k, m, trial, [])[0][0]:
                repairs |= bits(c, d)
                assert bits(c, d) == want_pairs[s], (s, c, d)
        assert repairs == want_pairs[s] == pr[s], (s, hex(repairs), hex(int(pr[s])))


def test_20_8_full_degraded_and_three_bad_fragments(D, dev):
    k, m = 20, 8
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    full = TC.stripes(k, m, bs)
    # input + input, input + parity, parity + parity, rows of the second 4-row half
    cases = [(0, 5), (3, 20), (21, 23), (7, 26), (19, 27), (24, 25)]
    held = np.stack([full[s % TC.S] for s in range(len(cases) + 3)])
    want = np.zeros(len(held), np.uint32)
    for i, (a, b) in enumerate(cases):
        damage_pair(held[i], a, b, i % 4, t)
        want[i] = bits(a, b)
    s3 = len(cases)  # three bad fragments in one word, and in three words: R >= 5 leaves no pair
    for f in (2, 11, 22):
        held[s3, f, 2 * 400] ^= 0x10 + f
        held[s3 + 1, f, 2 * 500 + 64 * f] ^= 0x01
    st, su, pr = locate_pairs_and_locate(D, k, m, held)
    assert (pr == want).all() and not su.any(), (hexes(pr), hexes(want), hexes(su))
    assert st[s3] and st[s3 + 1] and not st[s3 + 2]
    # degraded: fragments 3 and 25 lost, R = 6; fragment 20 is an input now
    missing = [3, 25]
    dev.ecamd_tune(b"bitslice", 0)  # the generic stage: no kernel of this map to compile
    cases = [(0, 4), (20, 21), (26, 27)]
    held = TC.held_of(np.stack([full[s % TC.S] for s in range(len(cases) + 1)]), missing)
    want = np.zeros(len(held), np.uint32)
    for i, (a, b) in enumerate(cases):
        damage_pair(held[i], a, b, i + 1, t)
        want[i] = bits(a, b)
    st, su, pr = locate_pairs_and_locate(D, k, m, held, missing)
    assert (pr == want).all() and not su.any() and not st[len(cases)], (hexes(pr), hexes(want), hexes(su))


@pytest.mark.parametrize("k,m,missing", [(10, 4, [2]), (4, 2, [])])
def test_fewer_than_four_checked_fragments_leave_pairs_zero(D, dev, k, m, missing):
    bs = 2 * 4096 + TAIL
    held = TC.held_of(TC.stripes(k, m, bs), missing)
    held[1, 0, 10] ^= 0x01
    held[1, k + m - 1, 4096 + 11] ^= 0x80
    held[2, 1, 77] ^= 0x08
    n0 = dev.ecamd_locate_pairs_launches()
    st, su, pr = locate_pairs_and_locate(D, k, m, held, missing)
    assert st[1] and st[2] and su[2] == 1 << 1 and not pr.any(), (hexes(st), hexes(su), hexes(pr))
    assert dev.ecamd_locate_pairs_launches() == n0


def test_knob_bitslice_changes_nothing(D, dev):
    k, m = 10, 4
    held, want_pairs, _ = batch_10_4()
    got = []
    for mode in (2, 0):
        dev.ecamd_tune(b"bitslice", mode)
        n0 = dev.ecamd_locate_fused_launches()
        got.append(locate_pairs_and_locate(D, k, m, held))
        assert (dev.ecamd_locate_fused_launches() > n0) == (mode == 2)
    for x, y in zip(*got):
        assert x.tobytes() == y.tobytes()
    assert (got[0][2] == want_pairs).all()


def test_grid_loops(D, dev):
    """Knob pairs_grid 2: two chunks and two stripe slots, so the chunk loop (16396 units: 33 passes of
    2 x 256) and the stripe loop (8 stripes) both iterate; the same words as with the default grid."""
    k, m = 10, 4
    bs = 65536 + TAIL
    full = TC.stripes(k, m, bs)
    cases = [(0, 1), (2, 13), (10, 11), None, (5, 9), (12, 13), (3, 10), (4, 7)]
    held = np.stack([full[s % TC.S] for s in range(len(cases))])
    want = np.zeros(len(cases), np.uint32)
    for i, c in enumerate(cases):
        if c:
            a, b = c
            held[i, a, (9000 * i + 2 * a) % bs] ^= 0x21  # anywhere in the fragment, the tail included
            held[i, b, bs - 2 - 2 * i] ^= 0x40
            held[i, b, 4096 * i + 1] ^= 0x02
            want[i] = bits(a, b)
    try:
        got = []
        for grid in (0, 2):
            dev.ecamd_tune(b"pairs_grid", grid)
            got.append(locate_pairs_and_locate(D, k, m, held))
    finally:
        dev.ecamd_tune(b"pairs_grid", 0)
    for x, y in zip(*got):
        assert x.tobytes() == y.tobytes()
    assert (got[0][2] == want).all(), (hexes(got[0][2]), hexes(want))


def test_scrub_pairs_repairs_singles_and_pairs(D, dev):
    k, m = 10, 4
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    full = TC.stripes(k, m, bs)
    good = np.stack([full[s % TC.S] for s in range(7)])
    bad = good.copy()
    bad[1, 3, 5000:5040] ^= 0x5A        # one data fragment
    damage_pair(bad[2], 2, 7, 1, t)     # two data fragments
    damage_pair(bad[3], 6, 12, 2, t)    # data and parity, one of them in the tail
    damage_pair(bad[4], 10, 13, 0, t)   # two parity fragments, the same word
    bad[5, k + 1, 17] ^= 0x01           # one parity fragment
    for f in (0, 4, 11):                # three fragments, the same word
        bad[6, f, 2 * 123] ^= 0x03 + f
    lay = upload(D, bad)
    try:
        st, su, pr, counts = D.rs_scrub_pairs(k, m, lay)
        after = lay.download_stripes()
        again, _ = D.rs_check(k, m, lay)
    finally:
        lay.buf.free()
    assert list(su) == [0, 1 << 3, 0, 0, 0, 1 << (k + 1), 0], hexes(su)
    assert list(pr[:6]) == [0, 0, bits(2, 7), bits(6, 12), bits(10, 13), 0], hexes(pr)
    # R == 4: three bad fragments can in principle read as a pair; otherwise the stripe is not written
    triple_taken = int(pr[6] != 0)
    assert counts == (1, 2, 3 + triple_taken, 1 - triple_taken), counts
    for s in range(6):
        assert (after[s] == good[s]).all(), s
        assert not again[s]
    if not triple_taken:
        assert (after[6] == bad[6]).all() and again[6] and st[6]


def test_scrub_pairs_20_8(D, dev):
    k, m = 20, 8
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    good = np.array(TC.stripes(k, m, bs))
    bad = good.copy()
    damage_pair(bad[1], 4, 25, 2, t)
    lay = upload(D, bad)
    try:
        st, su, pr, counts = D.rs_scrub_pairs(k, m, lay)
        after = lay.download_stripes()
    finally:
        lay.buf.free()
    assert counts == (2, 0, 1, 0) and list(pr) == [0, bits(4, 25), 0] and not su.any()
    assert (after == good).all()


def test_errors_leave_the_arrays_untouched(D, dev):
    k, m = 10, 4
    lay = D.Layout.alloc(k + m, 4096, TC.S)
    try:
        args = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride)
        for bs, null_pairs in ((4095, False), (4096, True)):  # odd blocksize; null d_pairs
            rc, st, su, pr, _ = raw_pairs(dev, D, k, m, [], *args, bs, TC.S, null_pairs=null_pairs)
            assert rc == EINVAL, (bs, null_pairs)
            assert (st == CANARY32).all() and (su == CANARY32).all() and (pr == CANARY32).all()
        rc, st, su, pr, _ = raw_pairs(dev, D, k, m, [0, 1, 2, 3, 4], *args, 4096, TC.S)
        assert rc == EINVAL and (st == CANARY32).all() and (su == CANARY32).all() and (pr == CANARY32).all()
        arrs = [D.DeviceBuffer(4 * TC.S) for _ in range(3)]
        for a in arrs:
            dev.ecamd_memset(a.ptr, CANARY, a.nbytes)
        counts = [C.c_int(-3) for _ in range(4)]
        # a pair repair needs four checks: (10, 3) is refused before anything runs
        assert dev.ecamd_rs_scrub_pairs(10, 3, *args, 4096, TC.S, *[a.ptr for a in arrs], *[C.byref(c) for c in counts],
                                        None) == EINVAL
        dev.ecamd_synchronize()
        for a in arrs:
            assert (a.download().view(np.uint32) == CANARY32).all()
            a.free()
        assert [c.value for c in counts] == [-3] * 4
    finally:
        lay.buf.free()
