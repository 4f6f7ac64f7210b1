"""GPU: correction of located fragments on the device (ecamd_rs_correct / ecamd_xor_correct,
include/ecamd.h).

Expected bytes never come from the code under test: good stripes are the reference encode's
(test_gpu_check.stripes, xor_oracle through test_gpu_xor_scrub.encoded) and a corrected stripe must
equal its good stripe.  The per-stripe words must be what ecamd_rs_locate_pairs / ecamd_rs_locate /
ecamd_xor_locate write for a fresh upload of the same data, and d_counts the tallies of those words.
Missing slots hold 0x5A and must still hold it afterwards."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_check as TC
import test_gpu_locate_pairs as LP
import test_gpu_locate_sweep as SW
import test_gpu_xor_scrub as XS
import test_xor_check_plan as TP
from test_gpu_check import D, dev  # noqa: F401  (fixtures)
from test_gpu_locate_pairs import bits, damage_pair, hexes, upload

pytestmark = pytest.mark.gpu
TAIL = TC.TAIL
EINVAL = -22
CANARY = 0xA5
CANARY32 = CANARY * 0x01010101


def tallies(st, su, pr):
    """(clean, one suspect, pair, dirty and neither) of the words, as d_counts must hold them."""
    pr = np.zeros_like(st) if pr is None else pr
    one = (st != 0) & (su != 0) & ((su & (su - 1)) == 0)
    two = (st != 0) & (su == 0) & (np.array([bin(int(v)).count("1") for v in pr]) == 2)
    return (int((st == 0).sum()), int(one.sum()), int(two.sum()), int(((st != 0) & ~one & ~two).sum()))


def correct(D, k, m, held, missing=(), pairs=True):
    """rs_correct of an upload of the stripes: (bytes afterwards, status, suspects, pairs, counts)."""
    lay = upload(D, held)
    try:
        st, su, pr, counts = D.rs_correct(k, m, lay, missing, pairs)
        return lay.download_stripes(), st, su, pr, counts
    finally:
        lay.buf.free()


def located(D, k, m, held, missing=(), pairs=True):
    """The locate's words for a fresh upload of the same stripes."""
    lay = upload(D, held)
    try:
        if pairs:
            return D.rs_locate_pairs(k, m, lay, missing)[:3]
        return D.rs_locate(k, m, lay, missing)[:2] + (None,)
    finally:
        lay.buf.free()


def same_words(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == np.uint32 and g.tobytes() == w.tobytes(), (hexes(g), hexes(w))


def test_every_culprit_and_every_pair_of_10_4_in_one_batch(D, dev):
    k, m = 10, 4
    held, want_pairs, want_suspects = LP.batch_10_4()
    n = len(held)
    bs = held.shape[2]
    full = TC.stripes(k, m, bs)
    good = np.stack([full[s % TC.S] for s in range(n + 1)])
    bad = np.concatenate([held, good[n:]])
    for f in (0, 4, 11):  # three bad fragments in one word
        bad[n, f, 2 * 123] ^= 0x03 + f
    n0 = dev.ecamd_correct_launches()
    after, st, su, pr, counts = correct(D, k, m, bad)
    assert dev.ecamd_correct_launches() == n0 + 1
    same_words((st, su, pr), located(D, k, m, bad))
    assert (su[:n] == want_suspects).all() and (pr[:n] == want_pairs).all()
    assert counts == tallies(st, su, pr), (counts, tallies(st, su, pr))
    assert counts[1] == k + m and counts[2] >= 91 and counts[0] == 1
    for s in range(n):
        assert (after[s] == good[s]).all(), (s, hex(int(su[s])), hex(int(pr[s])))
    # R == 4: three bad fragments can in principle read as a pair; otherwise the stripe is not written
    assert st[n] and not su[n]
    assert bool((after[n] == bad[n]).all()) == (pr[n] == 0)


def scrub_batch(k, m):
    """The batch of test_gpu_locate_pairs.test_scrub_pairs_repairs_singles_and_pairs."""
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    full = TC.stripes(k, m, bs)
    good = np.stack([full[s % TC.S] for s in range(7)])
    bad = good.copy()
    bad[1, 3, 5000:5040] ^= 0x5A
    damage_pair(bad[2], 2, 7, 1, t)
    damage_pair(bad[3], 6, 12, 2, t)
    damage_pair(bad[4], 10, 13, 0, t)
    bad[5, k + 1, 17] ^= 0x01
    for f in (0, 4, 11):
        bad[6, f, 2 * 123] ^= 0x03 + f
    return good, bad


def test_the_same_bytes_as_the_scrub(D, dev):
    k, m = 10, 4
    good, bad = scrub_batch(k, m)
    after, st, su, pr, counts = correct(D, k, m, bad)
    lay = upload(D, bad)
    try:
        st1, su1, pr1, counts1 = D.rs_scrub_pairs(k, m, lay)
        scrubbed = lay.download_stripes()
    finally:
        lay.buf.free()
    same_words((st, su, pr), (st1, su1, pr1))
    assert counts == counts1
    assert after.tobytes() == scrubbed.tobytes()
    for s in range(6):
        assert (after[s] == good[s]).all(), s


def test_singles_only_leaves_pair_stripes_untouched(D, dev):
    k, m = 10, 4
    good, bad = scrub_batch(k, m)
    n0 = dev.ecamd_locate_pairs_launches()
    after, st, su, pr, counts = correct(D, k, m, bad, pairs=False)
    assert dev.ecamd_locate_pairs_launches() == n0 and pr is None
    same_words((st, su, None), located(D, k, m, bad, pairs=False))
    assert list(su) == [0, 1 << 3, 0, 0, 0, 1 << (k + 1), 0] and counts == (1, 2, 0, 4), (hexes(su), counts)
    for s in (0, 1, 5):
        assert (after[s] == good[s]).all(), s
    for s in (2, 3, 4, 6):
        assert (after[s] == bad[s]).all(), s


def test_20_8_pairs_and_singles(D, dev):
    k, m = 20, 8
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    full = TC.stripes(k, m, bs)
    cases = [(0, 5), (3, 20), (21, 23), (7, 26), (19, 27), (24, 25)]
    singles = [0, 19, 20, 27]
    good = np.stack([full[s % TC.S] for s in range(len(cases) + len(singles) + 1)])
    bad = good.copy()
    want_pr, want_su = np.zeros(len(bad), np.uint32), np.zeros(len(bad), np.uint32)
    for i, (a, b) in enumerate(cases):
        damage_pair(bad[i], a, b, i % 4, t)
        want_pr[i] = bits(a, b)
    for i, f in enumerate(singles):
        s = len(cases) + i
        bad[s, f, 2 * (300 + 7 * f)] ^= 0x81
        bad[s, f, bs - 1 - 2 * i] ^= 0x10  # in the tail
        want_su[s] = 1 << f
    after, st, su, pr, counts = correct(D, k, m, bad)
    assert (su == want_su).all() and (pr == want_pr).all(), (hexes(su), hexes(pr))
    assert counts == (1, len(singles), len(cases), 0) == tallies(st, su, pr)
    assert (after == good).all(), [int(s) for s in np.nonzero((after != good).any(axis=(1, 2)))[0]]


def test_degraded_10_4_one_missing(D, dev):
    """R = 3: every participating fragment damaged in turn, a word in the tail included; a non-NULL
    d_pairs with R < 4 is zeroed and singles are still corrected."""
    k, m, missing = 10, 4, [2]
    bs = 2 * TC.tile_of(m) + TAIL
    full = TC.stripes(k, m, bs)
    part = [f for f in range(k + m) if f not in missing]
    good = TC.held_of(np.stack([full[s % TC.S] for s in range(len(part) + 1)]), missing)
    bad = good.copy()
    for i, f in enumerate(part):
        bad[i, f, 2 * (50 + 11 * f)] ^= 0x5A
        bad[i, f, bs - 1 - 2 * (i % 8)] ^= 0x01  # the tail
    n0 = dev.ecamd_locate_pairs_launches()
    after, st, su, pr, counts = correct(D, k, m, bad, missing)
    assert dev.ecamd_locate_pairs_launches() == n0 and not pr.any()
    assert list(su) == [1 << f for f in part] + [0], hexes(su)
    assert counts == (1, len(part), 0, 0)
    assert (after == good).all() and (after[:, missing] == TC.FILL).all()


def test_degraded_20_8_two_missing_pairs(D, dev):
    k, m, missing = 20, 8, [3, 25]
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    full = TC.stripes(k, m, bs)
    dev.ecamd_tune(b"bitslice", 0)  # the generic stage: no kernel of this map to compile
    cases = [(0, 4), (20, 21), (26, 27)]
    good = TC.held_of(np.stack([full[s % TC.S] for s in range(len(cases) + 1)]), missing)
    bad = good.copy()
    for i, (a, b) in enumerate(cases):
        damage_pair(bad[i], a, b, i + 1, t)
    after, st, su, pr, counts = correct(D, k, m, bad, missing)
    assert list(pr) == [bits(a, b) for a, b in cases] + [0] and not su.any(), (hexes(pr), hexes(su))
    assert counts == (1, 0, len(cases), 0)
    assert (after == good).all() and (after[:, missing] == TC.FILL).all()


def test_4_2_two_checks_generic_path(D, dev):
    k, m = 4, 2
    bs = 2 * 4096 + TAIL
    full = TC.stripes(k, m, bs)
    good = np.stack([full[s % TC.S] for s in range(k + m + 1)])
    bad = good.copy()
    for f in range(k + m):
        bad[f, f, 2 * (40 + f)] ^= 0x21
        bad[f, f, 4096 + 2 * f + 1] ^= 0x80
        bad[f, f, bs - 2 - 2 * f] ^= 0x07
    n0 = dev.ecamd_locate_fused_launches()
    after, st, su, pr, counts = correct(D, k, m, bad)
    assert dev.ecamd_locate_fused_launches() == n0
    assert list(su) == [1 << f for f in range(k + m)] + [0] and not pr.any()
    assert counts == (1, k + m, 0, 0)
    assert (after == good).all()


def raw_correct(dev, D, k, m, missing, base, stripe_stride, frag_stride, bs, nstripes, pairs=True, null=(), extra=3,
                stream=None):
    """ecamd_rs_correct on explicit pointers: arrays of nstripes + extra canary words and a d_counts of 8."""
    from liberasurecode_amd import _lib
    arrs = [D.DeviceBuffer(4 * (nstripes + extra)) for _ in range(3)] + [D.DeviceBuffer(32)]
    for a in arrs:
        dev.ecamd_memset(a.ptr, CANARY, a.nbytes)
    ptrs = [None if i in null or (i == 2 and not pairs) else a.ptr for i, a in enumerate(arrs)]
    checked = C.c_uint32(0xFFFFFFFF)
    rc = dev.ecamd_rs_correct(k, m, _lib.ints(list(missing) + [-1]), base, stripe_stride, frag_stride, bs, nstripes, *ptrs,
                              C.byref(checked), stream)
    dev.ecamd_synchronize()
    out = [a.download().view(np.uint32).copy() for a in arrs]
    for a in arrs:
        a.free()
    return (rc, *out, checked.value)


def run_layout(dev, D, k, m, host, good_host, base_off, stripe_stride, frag_stride, bs, nS, want_su, want_pr):
    """ecamd_rs_correct on `host` uploaded at base_off of a buffer with a canary line on either side: the
    whole buffer must end as good_host in the same frame -- the canaries between blocksize and the strides
    and around the batch included -- and nothing past nstripes words / 4 counts is written."""
    pad = 256
    frame = np.full(pad + base_off + host.size + pad, CANARY, np.uint8)
    want = frame.copy()
    frame[pad + base_off:pad + base_off + host.size] = host.reshape(-1)
    want[pad + base_off:pad + base_off + host.size] = good_host.reshape(-1)
    buf = D.DeviceBuffer(frame.nbytes)
    try:
        buf.upload(frame)
        rc, st, su, pr, cn, _ = raw_correct(dev, D, k, m, [], buf.ptr + pad + base_off, stripe_stride, frag_stride, bs, nS)
        got = buf.download()
    finally:
        buf.free()
    assert rc == 0
    assert list(su[:nS]) == want_su and list(pr[:nS]) == want_pr, (hexes(su), hexes(pr))
    for a in (st, su, pr):
        assert (a[nS:] == CANARY32).all()
    assert tuple(int(c) for c in cn[:4]) == tallies(st[:nS], su[:nS], pr[:nS]) and (cn[4:] == CANARY32).all()
    assert (got == want).all(), np.nonzero(got != want)[0][:8]


def test_layouts_bounds_and_a_partial_last_unit(D, dev):
    k, m, nS = 10, 4, 4
    n, bs = k + m, 4096 + 50  # 4146 = 4 * 1036 + 2: the last unit holds one word
    assert bs % 4 == 2
    full = TC.stripes(k, m, bs)
    good = np.stack([full[s % TC.S] for s in range(nS)])
    bad = good.copy()
    bad[1, 3, bs - 2] ^= 0x11   # the last word of an input
    bad[1, 3, bs - 1] ^= 0x80
    bad[2, 1, 2 * 77] ^= 0x40   # a pair, one of them in the last word
    bad[2, 12, bs - 1] ^= 0x09
    bad[3, 13, bs - 2] ^= 0x01  # the last word of a parity
    want_su = [0, 1 << 3, 0, 1 << 13]
    want_pr = [0, 0, bits(1, 12), 0]
    F = (bs + 15) // 16 * 16
    # a padded frag_stride, the padding a canary after each fragment
    fs = F + 48
    host, ghost = np.full((nS, n, fs), CANARY, np.uint8), np.full((nS, n, fs), CANARY, np.uint8)
    host[:, :, :bs], ghost[:, :, :bs] = bad, good
    run_layout(dev, D, k, m, host, ghost, 0, fs * n, fs, bs, nS, want_su, want_pr)
    run_layout(dev, D, k, m, host, ghost, 48, fs * n, fs, bs, nS, want_su, want_pr)
    # fragment-major: [k+m][S][F]
    host, ghost = np.full((n, nS, F), CANARY, np.uint8), np.full((n, nS, F), CANARY, np.uint8)
    host[:, :, :bs], ghost[:, :, :bs] = bad.transpose(1, 0, 2), good.transpose(1, 0, 2)
    run_layout(dev, D, k, m, host, ghost, 16, F, nS * F, bs, nS, want_su, want_pr)


def test_both_grid_loops(D, dev):
    """Knob pairs_grid 2 (it caps correct_kernel's grid as well as locate_pairs_kernel's) on the shape of test_gpu_locate_pairs.test_grid_loops: two chunks and two
    stripe slots, so the chunk loop and the stripe loop both iterate; the same bytes and words."""
    k, m = 10, 4
    bs = 65536 + TAIL
    full = TC.stripes(k, m, bs)
    cases = [(0, 1), (2, 13), (10, 11), None, (5, 9), (12, 13), (3, 10), (4,)]
    good = np.stack([full[s % TC.S] for s in range(len(cases))])
    bad = good.copy()
    for i, c in enumerate(cases):
        if c:
            a, b = c[0], c[-1]
            bad[i, a, (9000 * i + 2 * a) % bs] ^= 0x21  # anywhere in the fragment, the tail included
            bad[i, b, bs - 2 - 2 * i] ^= 0x40
            bad[i, b, 4096 * i + 1] ^= 0x02
    got = []
    try:
        for grid in (0, 2):
            dev.ecamd_tune(b"pairs_grid", grid)
            got.append(correct(D, k, m, bad))
    finally:
        dev.ecamd_tune(b"pairs_grid", 0)
    assert got[0][0].tobytes() == got[1][0].tobytes()
    same_words(got[0][1:4], got[1][1:4])
    assert got[0][4] == got[1][4] == (1, 1, 6, 0)
    assert list(got[0][3]) == [bits(*c) if c and len(c) == 2 else 0 for c in cases]
    assert (got[1][0] == good).all()


def test_knob_bitslice_changes_nothing(D, dev):
    k, m = 10, 4
    good, bad = scrub_batch(k, m)
    got = []
    for mode in (2, 0):
        dev.ecamd_tune(b"bitslice", mode)
        n0 = dev.ecamd_locate_fused_launches()
        got.append(correct(D, k, m, bad))
        assert (dev.ecamd_locate_fused_launches() > n0) == (mode == 2)
    assert got[0][0].tobytes() == got[1][0].tobytes()
    same_words(got[0][1:4], got[1][1:4])
    assert got[0][4] == got[1][4]
    assert (got[0][0][:6] == good[:6]).all()


# ---- flat XOR -----------------------------------------------------------------------------------

def xor_correct(D, k, m, hd, held):
    lay = D.Layout.alloc(k + m, held.shape[2], held.shape[0])
    try:
        lay.upload_stripes(held)
        st, su, pr, counts = D.xor_correct(k, m, hd, lay)
        assert pr is None
        return lay.download_stripes(), st, su, counts, D.xor_check(k, m, hd, lay)
    finally:
        lay.buf.free()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("k,m,hd", [(10, 6, 4), (3, 3, 3)])
def test_xor_every_culprit(D, knobs, k, m, hd, fused):
    """The batch of test_gpu_xor_scrub.test_scrub_repairs_every_located_fragment_and_leaves_the_rest."""
    dev = knobs
    n, bs = k + m, 4096 + TAIL
    nS = 2 + n + 2
    good = XS.encoded(7000 + k, k, m, hd, nS, bs)
    bad = good.copy()
    rng = np.random.default_rng(7100 + k)
    for f in range(n):
        lo, hi = (4096, bs) if f % 3 == 2 else (0, 4096)
        SW.xor_word(bad, 1 + f, f, int(rng.integers(lo // 2, hi // 2)) * 2, int(rng.integers(1, 0x10000)))
        SW.xor_word(bad, 1 + f, f, int(rng.integers(0, bs // 2)) * 2, 0x8000)
    pairs = [1 + n, 2 + n]
    SW.xor_word(bad, pairs[0], 0, 10, 0x0101)
    SW.xor_word(bad, pairs[0], 2, 2000, 0x0440)
    SW.xor_word(bad, pairs[1], 1, 300, 0x0003)
    SW.xor_word(bad, pairs[1], k + 1, 4096 + 20, 0x3000)
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, bad)
    assert [int(v) for v in want_su[1:1 + n]] == [1 << f for f in range(n)] and not want_su[pairs].any()
    dev.ecamd_tune(b"xor_check_fused", fused)
    c0, n0 = XS.counters(dev), dev.ecamd_correct_launches()
    after, st, su, counts, again = xor_correct(D, k, m, hd, bad)
    assert (XS.counters(dev)[1] > c0[1]) == bool(fused) and dev.ecamd_correct_launches() == n0 + 1
    assert (st == want_st).all() and (su == want_su).all(), (hexes(st), hexes(su))
    assert counts == (2, n, 0, 2) == tallies(st, su, None)
    for s in range(nS):
        assert (after[s] == (bad[s] if s in pairs else good[s])).all(), s
    assert list(np.nonzero(again)[0]) == pairs


@pytest.fixture()
def knobs(dev):
    yield dev
    for key, value in ((b"xor_check_fused", -1), (b"xor_check_threads", 0)):
        dev.ecamd_tune(key, value)


def test_xor_pair_that_reads_as_a_third_fragment_ends_as_the_scrub_leaves_it(D, dev):
    k, m, hd, bs, nS = 3, 3, 3, 4096 + TAIL, 2
    rc, sig = TP.plan(k, m, hd)
    assert rc == 0
    f1, f2, f3 = TP.sum_triple(sig)
    good = XS.encoded(7500, k, m, hd, nS, bs)
    bad = good.copy()
    SW.xor_word(bad, 1, f1, 1234, 0x5AA5)
    SW.xor_word(bad, 1, f2, 1234, 0x5AA5)
    after, st, su, counts, again = xor_correct(D, k, m, hd, bad)
    assert st[1] and su[1] == 1 << f3 and counts == (1, 1, 0, 0) and not again.any()
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.upload_stripes(bad)
        D.xor_scrub(k, m, hd, lay)
        scrubbed = lay.download_stripes()
    finally:
        lay.buf.free()
    assert after.tobytes() == scrubbed.tobytes()
    assert (after[0] == good[0]).all() and (after[1, f3] != bad[1, f3]).any()


# ---- framed, stream order, errors -----------------------------------------------------------------

def test_framed_fragments_at_the_payload(D, dev):
    from liberasurecode_amd import frame as F
    k, m, nS = 10, 4, 3
    obj_size = 10 * 1000
    fb = F.FrameBatch(F.RS_VAND, k, m, obj_size, nS, checksum=F.CHKSUM_CRC32)
    bs = fb.blocksize
    assert bs % 2 == 0 and bs >= 64
    objs = np.random.default_rng(9100).integers(0, 256, size=nS * fb.obj_stride, dtype=np.uint8)
    d_obj = D.DeviceBuffer(objs.nbytes)
    try:
        d_obj.upload(objs)
        fb.encode(d_obj)
        dev.ecamd_synchronize()
        frags = fb.fragments()
        assert not fb.verify()[0].any()
        hurt = frags.copy()
        hurt[1, 5, F.HEADER + 40] ^= 0x77
        hurt[1, 5, F.HEADER + bs - 1] ^= 0x01
        fb.upload_fragments(hurt)
        status = fb.verify()[0]
        want = np.zeros_like(status)
        want[1, 5] = 1 << 4
        assert (status == want).all(), status
        rc, st, su, pr, cn, checked = raw_correct(dev, D, k, m, [], fb.base + F.HEADER, fb.stripe_stride, fb.frag_stride, bs, nS)
        assert rc == 0 and list(su[:nS]) == [0, 1 << 5, 0] and tuple(cn[:4]) == (2, 1, 0, 0)
        assert not fb.verify()[0].any()
        assert (fb.fragments() == frags).all()
    finally:
        d_obj.free()
        fb.buf.free()


def test_stream_order_with_one_synchronise_at_the_end(D, dev):
    """Upload, correct and download enqueued back to back on one stream; one wait at the end."""
    k, m = 10, 4
    good, bad = scrub_batch(k, m)
    nS, bs = bad.shape[0], bad.shape[2]
    lay = D.Layout.alloc(k + m, bs, nS)
    nbytes = lay.stripe_stride * nS
    words = D.DeviceBuffer(4 * (3 * nS + 4))
    pin = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    sizes = [nbytes, nbytes, words.nbytes]
    stream = D.Stream()
    try:
        for p, size in zip(pin, sizes):
            assert dev.ecamd_host_alloc(C.byref(p), size) == 0
        h_in, h_out, h_words = (np.ctypeslib.as_array((C.c_uint8 * size).from_address(p.value)) for p, size in zip(pin, sizes))
        view = h_in.reshape(nS, k + m, lay.frag_stride)
        view[...] = 0
        view[:, :, :bs] = bad
        h_out[...] = 0
        h_words[...] = 0
        s = stream.handle
        assert dev.ecamd_memcpy_async(lay.buf.ptr, pin[0], nbytes, 0, s) == 0
        assert dev.ecamd_rs_correct(k, m, None, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, bs, nS, words.ptr,
                                    words.ptr + 4 * nS, words.ptr + 8 * nS, words.ptr + 12 * nS, None, s) == 0
        assert dev.ecamd_memcpy_async(pin[1], lay.buf.ptr, nbytes, 1, s) == 0
        assert dev.ecamd_memcpy_async(pin[2], words.ptr, words.nbytes, 1, s) == 0
        stream.synchronize()
        after = h_out.reshape(nS, k + m, lay.frag_stride)[:, :, :bs].copy()
        w = h_words.view(np.uint32).copy()
    finally:
        for p in pin:
            if p.value:
                dev.ecamd_host_free(p)
        stream.destroy()
        words.free()
        lay.buf.free()
    st, su, pr, cn = w[:nS], w[nS:2 * nS], w[2 * nS:3 * nS], w[3 * nS:]
    assert list(su) == [0, 1 << 3, 0, 0, 0, 1 << (k + 1), 0], hexes(su)
    assert list(pr[:6]) == [0, 0, bits(2, 7), bits(6, 12), bits(10, 13), 0], hexes(pr)
    assert tuple(int(c) for c in cn) == tallies(st, su, pr)
    assert (after[:6] == good[:6]).all()


def test_errors_leave_everything_untouched(D, dev):
    k, m, nS, bs = 10, 4, TC.S, 4096
    host = np.random.default_rng(9200).integers(0, 256, size=32 * bs * nS, dtype=np.uint8)
    buf = D.DeviceBuffer(host.nbytes)

    def untouched(res):
        rc, st, su, pr, cn = res[:5]
        assert rc == EINVAL
        for a in (st, su, pr, cn):
            assert (a == CANARY32).all()
        assert (buf.download() == host).all()

    try:
        buf.upload(host)
        args = (buf.ptr, 32 * bs, bs)
        untouched(raw_correct(dev, D, k, m, [], *args, bs - 1, nS))             # odd blocksize
        untouched(raw_correct(dev, D, k, m, [], *args, bs, nS, null=(0,)))      # null d_status
        untouched(raw_correct(dev, D, k, m, [], *args, bs, nS, null=(1,)))      # null d_suspects
        untouched(raw_correct(dev, D, k, m, [0, 1, 2, 3, 4], *args, bs, nS))    # m + 1 missing
        untouched(raw_correct(dev, D, 28, 5, [], *args, bs, nS))                # k + m > 32
        # flat XOR with a code init_xor_hd_code rejects, and an odd blocksize
        for kk, mm, hd, size in ((10, 4, 9, bs), (10, 6, 4, bs - 1)):
            arrs = [D.DeviceBuffer(4 * nS) for _ in range(2)] + [D.DeviceBuffer(32)]
            for a in arrs:
                dev.ecamd_memset(a.ptr, CANARY, a.nbytes)
            rc = dev.ecamd_xor_correct(kk, mm, hd, buf.ptr, 32 * bs, bs, size, nS, *[a.ptr for a in arrs], None)
            dev.ecamd_synchronize()
            out = [a.download().view(np.uint32).copy() for a in arrs]
            for a in arrs:
                a.free()
            untouched((rc, out[0], out[1], out[0], out[2]))
        # an empty batch returns 0 and writes nothing
        n0 = dev.ecamd_correct_launches()
        rc, st, su, pr, cn, _ = raw_correct(dev, D, k, m, [], *args, bs, 0)
        assert rc == 0 and dev.ecamd_correct_launches() == n0
        for a in (st, su, pr, cn):
            assert (a == CANARY32).all()
        assert (buf.download() == host).all()
    finally:
        buf.free()
