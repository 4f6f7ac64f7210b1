"""GPU: check, locate and correct of flat XOR stripes with fragments missing (ecamd_xor_check_degraded,
ecamd_xor_locate_degraded, ecamd_xor_correct_degraded, include/ecamd.h).

Expected values never come from the code under test.  Status and suspects are `oracle` below: the
reduction rule restated in test_xor_degraded_plan.reduce (from the golden parity bitmaps) applied to the
stored bytes word by word.  Corrected bytes are compared with the reference-encoded originals.  The
clean / dirty split is cross-checked against the reference itself: rebuild the missing fragments with
its decode, then judge the full stripe with test_gpu_locate_sweep.xor_status.  Missing slots hold a
canary before upload and must still hold it afterwards.

Shapes as test_gpu_xor_scrub: bs = 2 * 2048 + TAIL gives whole tiles of both tile forms (knob
xor_check_threads 256 / 64) and a tail for the generic stage; knob xor_check_fused 0 sends everything
through the generic stage, whose words must be the same."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_check as TC
import test_gpu_locate_sweep as SW
import test_gpu_xor_scrub as XS
import test_xor_degraded_plan as P
from test_gpu_check import D, dev  # noqa: F401  (fixtures)
from test_gpu_xor_scrub import knobs  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
XO = TC.XO
TAIL = TC.TAIL
EINVAL = -22
CANARY = XS.CANARY
CANARY32 = XS.CANARY32
GUARD = XS.GUARD
FORMS = XS.FORMS
TILE = 2048
BS = 2 * TILE + TAIL
PB = {c[:3]: c[3] for c in P.CODES}
CASES = [(10, 6, 4, [3]), (10, 6, 4, [12]), (10, 6, 4, [3, 12]), (10, 6, 4, [0, 1, 2]),
         (3, 3, 3, [0]), (3, 3, 3, [4]), (20, 6, 4, [19]), (20, 6, 4, [0, 25])]


def bits_of(mask):
    return [f for f in range(32) if mask >> f & 1]


def oracle(k, m, hd, missing, held):
    """(status, suspects, covered) of (S, k+m, bs) stored stripes by the rule alone; the missing slots
    are never looked at."""
    rows, sig, covered, _ = P.reduce(k, m, PB[(k, m, hd)], missing)
    alive = [p for p in range(m) if rows[p]]
    words = np.ascontiguousarray(held).view("<u2")
    nS = held.shape[0]
    status, suspects = np.zeros(nS, np.uint32), np.zeros(nS, np.uint32)
    for s in range(nS):
        syn = np.zeros((len(alive), words.shape[2]), np.uint16)
        for i, p in enumerate(alive):
            for f in bits_of(rows[p]):
                syn[i] ^= words[s, f]
        keep = covered
        for w in np.nonzero(syn.any(axis=0))[0]:
            col = [int(x) for x in syn[:, w]]
            nz = sum(1 << alive[i] for i in range(len(alive)) if col[i])
            status[s] |= np.uint32(nz << k)
            equal = len({x for x in col if x}) == 1
            keep &= sum(1 << f for f in bits_of(covered) if equal and sig[f] == nz)
        suspects[s] = keep if status[s] else 0
    return status, suspects, covered


def reference_dirty(k, m, hd, missing, held):
    """Per stripe, whether the reference finds the stripe inconsistent once its decode has rebuilt the
    missing fragments; None for a pattern it cannot decode."""
    code = XO.XorCode(k, m, hd)
    out = np.zeros(held.shape[0], bool)
    for s in range(held.shape[0]):
        bufs = [np.array(x) for x in held[s]]
        for f in missing:
            bufs[f][:] = 0
        if code.decode(bufs, list(missing), 1) != 0:
            return None
        out[s] = SW.xor_status(k, m, hd, np.stack(bufs)[None])[0] != 0
    return out


def tallies(st, su):
    one = (st != 0) & (su != 0) & ((su & (su - 1)) == 0)
    return (int((st == 0).sum()), int(one.sum()), 0, int(((st != 0) & ~one).sum()))


def raw(dev, D, what, k, m, hd, missing, base, stripe_stride, frag_stride, bs, nS, null=()):
    """The three degraded calls on explicit pointers, every array canary-filled with GUARD words on either
    side (test_gpu_xor_scrub.raw's pattern): (rc, status, suspects, counts, covered).  status / suspects /
    counts are None where the call left every word untouched, covered is None where it was not set."""
    from liberasurecode_amd import _lib
    n = nS + 2 * GUARD
    st, su, cn = D.DeviceBuffer(4 * n), D.DeviceBuffer(4 * n), D.DeviceBuffer(4 * (4 + 2 * GUARD))
    for a in (st, su, cn):
        dev.ecamd_memset(a.ptr, CANARY, a.nbytes)
    covered = C.c_uint32(CANARY32)
    lst = None if missing is None else _lib.ints(list(missing) + [-1])
    d_st = None if "status" in null else st.ptr + 4 * GUARD
    d_su = None if "suspects" in null else su.ptr + 4 * GUARD
    args = (k, m, hd, lst, base, stripe_stride, frag_stride, bs, nS, d_st)
    if what == "check":
        rc = dev.ecamd_xor_check_degraded(*args, C.byref(covered), None)
    elif what == "locate":
        rc = dev.ecamd_xor_locate_degraded(*args, d_su, C.byref(covered), None)
    else:
        rc = dev.ecamd_xor_correct_degraded(*args, d_su, cn.ptr + 4 * GUARD, C.byref(covered), None)
    dev.ecamd_synchronize()
    a, b, c = (x.download().view(np.uint32).copy() for x in (st, su, cn))
    for x in (st, su, cn):
        x.free()
    for arr, used in ((a, nS), (b, nS), (c, 4)):
        assert (arr[:GUARD] == CANARY32).all() and (arr[GUARD + used:] == CANARY32).all(), what
    if what == "check":
        assert (b == CANARY32).all()
    if what != "correct":
        assert (c == CANARY32).all()
    a, b, c = a[GUARD:GUARD + nS], b[GUARD:GUARD + nS], c[GUARD:GUARD + 4]
    return (rc, None if nS and (a == CANARY32).all() else a, None if nS and (b == CANARY32).all() else b,
            None if (c == CANARY32).all() else tuple(int(x) for x in c),
            None if covered.value == CANARY32 else covered.value)


def held_of(bad, missing):
    held = np.array(bad)
    held[:, list(missing)] = CANARY
    return held


_batches = {}


def batch(k, m, hd, missing, dense=True):
    """damaged_batch over the covered fragments, the missing slots canary-filled, with the oracle's words:
    (good, held, singles, status, suspects, covered), once per case."""
    key = (k, m, hd, tuple(missing), dense)
    if key not in _batches:
        covered = P.reduce(k, m, PB[(k, m, hd)], missing)[2]
        good, bad, singles, pairs, clean = SW.damaged_batch(9000 + 31 * k + sum(missing), k, k + m, BS, TILE, bits_of(covered),
                                                            XS.encoder(k, m, hd), dense=dense)
        held = held_of(bad, missing)
        st, su, cov = oracle(k, m, hd, missing, held)
        assert cov == covered and not st[clean].any() and st[list(singles)].all() and st[pairs].all()
        for a in (good, held, st, su):
            a.setflags(write=False)
        _batches[key] = (good, held, singles, st, su, covered)
    return _batches[key]


def upload(D, held):
    lay = D.Layout.alloc(held.shape[1], held.shape[2], held.shape[0])
    lay.upload_stripes(held)
    return lay


def check_corrected(after, good, held, missing, want_st, want_su, singles):
    """A stripe with exactly one suspect is the reference-encoded original again in every available
    fragment, every other stripe is byte-identical, and every missing slot still holds the canary."""
    avail = [f for f in range(held.shape[1]) if f not in missing]
    assert (after[:, list(missing)] == CANARY).all()
    for s in range(held.shape[0]):
        su = int(want_su[s])
        if want_st[s] and su and not su & (su - 1):
            assert singles.get(s) == su.bit_length() - 1, (s, hex(su))
            assert (after[s, avail] == good[s, avail]).all(), s
        else:
            assert (after[s] == held[s]).all(), s


@pytest.mark.parametrize("k,m,hd,missing", CASES, ids=["%d_%d_%d_%s" % (k, m, hd, "-".join(map(str, x))) for k, m, hd, x in CASES])
def test_every_covered_culprit_on_every_path(D, knobs, k, m, hd, missing):
    dev = knobs
    good, held, singles, want_st, want_su, covered = batch(k, m, hd, missing)
    nS = held.shape[0]
    ref = reference_dirty(k, m, hd, missing, held)
    if ref is not None:  # a pattern the reference decodes: the same clean / dirty split
        assert ((want_st != 0) == ref).all(), np.nonzero((want_st != 0) != ref)[0]
    got = []
    for threads, form_tile in FORMS:
        assert BS // form_tile >= 1 and BS % form_tile == TAIL
        dev.ecamd_tune(b"xor_check_threads", threads)
        for fused in (1, 0):
            dev.ecamd_tune(b"xor_check_fused", fused)
            lay = upload(D, held)
            try:
                where = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, BS, nS)
                c0 = XS.counters(dev)
                rc, chk, _, _, cov = raw(dev, D, "check", k, m, hd, missing, *where)
                c1 = XS.counters(dev)
                assert rc == 0 and cov == covered
                assert (c1[0] > c0[0], c1[1] > c0[1]) == (bool(fused), False) and c1[2:] == c0[2:], (fused, c0, c1)
                rc, st, su, _, cov = raw(dev, D, "locate", k, m, hd, missing, *where)
                c2 = XS.counters(dev)
                assert rc == 0 and cov == covered
                assert (c2[0] > c1[0], c2[1] > c1[1]) == (False, bool(fused)) and c2[2:] == c1[2:], (fused, c1, c2)
                wrong = np.nonzero((st != want_st) | (su != want_su) | (chk != want_st))[0]
                assert not len(wrong), (threads, fused, [(int(s), hex(int(st[s])), hex(int(su[s])), hex(int(chk[s])),
                                                          hex(int(want_st[s])), hex(int(want_su[s]))) for s in wrong[:6]])
                assert (lay.download_stripes() == held).all()
                n0 = dev.ecamd_correct_launches()
                rc, st2, su2, counts, cov = raw(dev, D, "correct", k, m, hd, missing, *where)
                assert rc == 0 and cov == covered and dev.ecamd_correct_launches() == n0 + 1
                assert st2.tobytes() == st.tobytes() and su2.tobytes() == su.tobytes()
                assert counts == tallies(want_st, want_su), (counts, tallies(want_st, want_su))
                check_corrected(lay.download_stripes(), good, held, missing, want_st, want_su, singles)
                got.append((st, su, chk))
            finally:
                lay.buf.free()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.dtype == np.uint32 and a.tobytes() == b.tobytes()


def test_every_single_loss_of_10_6_4_locates_and_corrects_every_fragment(D, knobs):
    dev = knobs
    k, m, hd = 10, 6, 4
    for lost in range(k + m):
        good, held, singles, want_st, want_su, covered = batch(k, m, hd, [lost], dense=False)
        assert covered == (1 << (k + m)) - 1 - (1 << lost)
        for s, f in singles.items():  # hd 4 with one lost: the signatures are distinct
            assert want_su[s] == 1 << f, (lost, s, f, hex(int(want_su[s])))
        lay = upload(D, held)
        try:
            st, su, pr, counts, cov = D.xor_correct(k, m, hd, lay, missing=[lost])
            after = lay.download_stripes()
        finally:
            lay.buf.free()
        assert pr is None and cov == covered
        assert (st == want_st).all() and (su == want_su).all(), (lost, [hex(int(x)) for x in su])
        assert counts == tallies(want_st, want_su) and counts[1] == len(singles)
        check_corrected(after, good, held, [lost], want_st, want_su, singles)


def test_fragments_that_share_a_signature_come_back_together_and_are_not_written(D, knobs):
    k, m, hd, missing = 3, 3, 3, [0]
    rows, sig, covered, alive = P.reduce(k, m, PB[(k, m, hd)], missing)
    classes = [[f for f in bits_of(covered) if sig[f] == v] for v in sorted({sig[f] for f in bits_of(covered)})]
    shared = [c for c in classes if len(c) > 1]
    assert shared and alive == 2
    nS = 1 + sum(len(c) for c in shared)
    held = held_of(XS.encoded(9500, k, m, hd, nS, BS), missing)
    want = np.zeros(nS, np.uint32)
    s = 1
    for c in shared:
        for f in c:  # one word in a tile, one in the tail
            SW.xor_word(held, s, f, 2 * (100 + 7 * f), 0x1234 + f)
            SW.xor_word(held, s, f, BS - 2 - 2 * f, 0x8001)
            want[s] = sum(1 << x for x in c)
            s += 1
    want_st, want_su, _ = oracle(k, m, hd, missing, held)
    assert (want_su == want).all() and want_st[1:].all() and not want_st[0]
    lay = upload(D, held)
    try:
        st, su, cov = D.xor_locate(k, m, hd, lay, missing=missing)
        assert cov == covered and (st == want_st).all() and (su == want).all(), [hex(int(x)) for x in su]
        st, su, pr, counts, cov = D.xor_correct(k, m, hd, lay, missing=missing)
        assert (su == want).all() and counts == (1, 0, 0, nS - 1)
        assert (lay.download_stripes() == held).all()
        chk, cov = D.xor_check(k, m, hd, lay, missing=missing)
        assert (chk == want_st).all() and cov == covered
    finally:
        lay.buf.free()


def test_one_surviving_row_and_no_surviving_row(D, knobs):
    k, m, hd, nS = 3, 3, 3, 3
    full = XS.encoded(9600, k, m, hd, nS, BS)
    # every data fragment lost: one row is left, the three parities, and every one of them is a suspect
    missing = [0, 1, 2]
    rows, sig, covered, alive = P.reduce(k, m, PB[(k, m, hd)], missing)
    assert alive == 1 and covered == 0b111000
    held = held_of(full, missing)
    SW.xor_word(held, 1, 4, 64, 0x00FF)
    SW.xor_word(held, 2, 5, BS - 2, 0x0100)
    want_st, want_su, _ = oracle(k, m, hd, missing, held)
    assert list(want_su) == [0, covered, covered] and not want_st[0]
    lay = upload(D, held)
    try:
        where = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, BS, nS)
        rc, st, su, counts, cov = raw(knobs, D, "correct", k, m, hd, missing, *where)
        assert rc == 0 and cov == covered and (st == want_st).all() and (su == want_su).all() and counts == (1, 0, 0, 2)
        assert (lay.download_stripes() == held).all()
        # every parity lost: no row is left; all-zero words, nothing covered, whatever the data holds
        missing = [3, 4, 5]
        assert P.reduce(k, m, PB[(k, m, hd)], missing)[2:] == (0, 0)
        n0 = knobs.ecamd_correct_launches()
        for what in ("check", "locate", "correct"):
            rc, st, su, counts, cov = raw(knobs, D, what, k, m, hd, missing, *where)
            assert rc == 0 and cov == 0 and not st.any()
            assert what == "check" or not su.any()
            assert counts == ((nS, 0, 0, 0) if what == "correct" else None)
        assert knobs.ecamd_correct_launches() == n0
        assert (lay.download_stripes() == held).all()
    finally:
        lay.buf.free()


def test_fragment_major_layout_with_a_padded_frag_stride(D, knobs):
    """[k+m][S][F] with frag_stride = S * F + 48: the whole buffer -- the padding after every fragment,
    the gap after every fragment row and the missing slots included -- ends as the good one."""
    dev = knobs
    k, m, hd, missing, nS = 10, 6, 4, [3], 4
    n = k + m
    good = held_of(XS.encoded(9700, k, m, hd, nS, BS), missing)
    bad = good.copy()
    SW.xor_word(bad, 1, 7, 64, 0x1234)
    SW.xor_word(bad, 2, n - 1, BS - 2, 0x00FF)
    SW.xor_word(bad, 3, 0, 8, 0x8001)
    SW.xor_word(bad, 3, k, 2000, 0x0180)
    want_st, want_su, covered = oracle(k, m, hd, missing, bad)
    assert list(want_su) == [0, 1 << 7, 1 << (n - 1), 0] and want_st[3]
    good[3] = bad[3]  # two bad fragments: not written
    F = (BS + 15) // 16 * 16 + 32
    fs = nS * F + 48
    pad, base_off = 256, 16
    host, ghost = np.full((n, fs), CANARY, np.uint8), np.full((n, fs), CANARY, np.uint8)
    for arr, src in ((host, bad), (ghost, good)):
        for s in range(nS):
            arr[:, s * F:s * F + BS] = src[s]
    frame = np.full(pad + base_off + host.size + pad, CANARY, np.uint8)
    want = frame.copy()
    frame[pad + base_off:pad + base_off + host.size] = host.reshape(-1)
    want[pad + base_off:pad + base_off + host.size] = ghost.reshape(-1)
    buf = D.DeviceBuffer(frame.nbytes)
    try:
        buf.upload(frame)
        where = (buf.ptr + pad + base_off, F, fs, BS, nS)
        c0 = XS.counters(dev)
        rc, chk, _, _, cov = raw(dev, D, "check", k, m, hd, missing, *where)
        assert rc == 0 and cov == covered and (chk == want_st).all()
        rc, st, su, _, _ = raw(dev, D, "locate", k, m, hd, missing, *where)
        assert rc == 0 and (st == want_st).all() and (su == want_su).all(), [hex(int(x)) for x in su]
        c1 = XS.counters(dev)
        assert c1[0] > c0[0] and c1[1] > c0[1] and c1[2:] == c0[2:]
        assert (buf.download() == frame).all()
        rc, st, su, counts, _ = raw(dev, D, "correct", k, m, hd, missing, *where)
        assert rc == 0 and (su == want_su).all() and counts == (1, 2, 0, 1)
        got = buf.download()
        assert (got == want).all(), np.nonzero(got != want)[0][:8]
    finally:
        buf.free()


def test_errors_and_an_empty_batch_leave_everything_untouched(D, knobs):
    dev = knobs
    k, m, hd, nS, bs = 10, 6, 4, 3, 4096
    host = np.full(16 * bs * nS, CANARY, np.uint8)
    buf = D.DeviceBuffer(host.nbytes + 16)
    try:
        buf.upload(host)

        def untouched(what, res):
            rc, st, su, counts, cov = res
            assert rc == EINVAL and st is None and su is None and counts is None and cov is None, (what, res)
            assert (buf.download(host.nbytes) == host).all()

        good = (buf.ptr, 16 * bs, bs, bs, nS)
        for what in ("check", "locate", "correct"):
            # what the plan rejects: out of range, repeated, more than m entries, a code nobody accepts
            untouched(what, raw(dev, D, what, k, m, hd, [16], *good))
            untouched(what, raw(dev, D, what, k, m, hd, [3, 3], *good))
            untouched(what, raw(dev, D, what, k, m, hd, [0, 1, 2, 3, 4, 5, 6], *good))
            untouched(what, raw(dev, D, what, 10, 4, 9, [1], *good))
            # the layout errors of the full-stripe calls
            untouched(what, raw(dev, D, what, k, m, hd, [3], buf.ptr + 8, 16 * bs, bs, bs, nS))
            untouched(what, raw(dev, D, what, k, m, hd, [3], buf.ptr, 16 * bs, bs - 16, bs, nS))
            untouched(what, raw(dev, D, what, k, m, hd, [3], buf.ptr, 16 * bs + 8, bs, bs, nS))
            untouched(what, raw(dev, D, what, k, m, hd, [3], None, 16 * bs, bs, bs, nS))
            untouched(what, raw(dev, D, what, k, m, hd, [3], *good, null=("status",)))
            if what != "check":
                untouched(what, raw(dev, D, what, k, m, hd, [3], *good, null=("suspects",)))
                untouched(what, raw(dev, D, what, k, m, hd, [3], buf.ptr, 16 * bs, bs, bs - 1, nS))  # odd blocksize
        # an odd blocksize is fine for the check
        rc, st, _, _, cov = raw(dev, D, "check", k, m, hd, [3], buf.ptr, 16 * bs, bs, bs - 1, nS)
        assert rc == 0 and st is not None and cov == (1 << 16) - 1 - (1 << 3)
        # an empty batch returns 0 and writes nothing
        c0, n0 = XS.counters(dev), dev.ecamd_correct_launches()
        for what in ("check", "locate", "correct"):
            rc, st, su, counts, cov = raw(dev, D, what, k, m, hd, [3], buf.ptr, 16 * bs, bs, bs, 0)
            assert rc == 0 and not len(st) and not len(su) and counts is None
        assert XS.counters(dev) == c0 and dev.ecamd_correct_launches() == n0
        assert (buf.download(host.nbytes) == host).all()
    finally:
        buf.free()


def test_an_empty_missing_list_keeps_todays_calls_and_tuples(D, knobs):
    k, m, hd = 10, 6, 4
    held = XS.encoded(9800, k, m, hd, 2, BS)
    SW.xor_word(held, 1, 5, 100, 0x4242)
    lay = upload(D, held)
    try:
        out = D.xor_locate(k, m, hd, lay, missing=())
        assert len(out) == 2 and list(out[1]) == [0, 1 << 5]
        chk = D.xor_check(k, m, hd, lay, missing=[])
        assert isinstance(chk, np.ndarray) and chk.tobytes() == out[0].tobytes()
        # and the degraded entry point with nothing missing gives the full-stripe words
        rc, st, su, _, cov = raw(knobs, D, "locate", k, m, hd, [], lay.buf.ptr, lay.stripe_stride, lay.frag_stride, BS, 2)
        assert rc == 0 and cov == (1 << 16) - 1 and st.tobytes() == out[0].tobytes() and su.tobytes() == out[1].tobytes()
        rc, st, su, _, cov = raw(knobs, D, "locate", k, m, hd, None, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, BS, 2)
        assert rc == 0 and st.tobytes() == out[0].tobytes() and su.tobytes() == out[1].tobytes()
        assert len(D.xor_correct(k, m, hd, lay, missing=())) == 4
    finally:
        lay.buf.free()
