"""GPU: the fused flat XOR check / locate kernel and ecamd_xor_scrub (include/ecamd.h).

Expected values never come from the code under test: statuses and suspects are
test_gpu_locate_sweep.xor_status / xor_oracle_locate over oracle/xor_oracle.py, repaired bytes are
compared with the reference-encoded originals.  ecamd_xor_check_fused_launches /
ecamd_xor_locate_fused_launches pin which path ran; knob xor_check_fused 0 gives the generic
compute-and-compare path, whose words must be byte-identical.  Knob xor_check_threads reaches both tile
forms (256 lanes on 4 KiB tiles, one wave on 1 KiB tiles) at a few KiB.

damaged_batch refuses a `tile` below 1024 + 64 (its "lanes" item writes at offset 1000 of a tile), so
the one-wave form runs it with tile 2048 -- two of its tiles -- and bs = 2 * 2048 + TAIL: four whole
1 KiB tiles and the tail, the "lanes" pair still inside one 1 KiB tile on lanes 0 and 62."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_check as TC
import test_gpu_locate_sweep as SW
import test_xor_check_plan as TP
from test_gpu_check import D, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
XO = TC.XO
TAIL = TC.TAIL
EINVAL = -22
CANARY = 0xA5
CANARY32 = CANARY * 0x01010101
GUARD = 2  # canary words on either side of the status and suspects arrays
CODES = [(10, 6, 4), (3, 3, 3), (20, 6, 4)]
FORMS = [(256, 4096), (64, 1024)]  # knob xor_check_threads, the form's tile


@pytest.fixture()
def knobs(dev):
    """The flat XOR check knobs back at their defaults afterwards."""
    yield dev
    for key, value in ((b"xor_check_fused", -1), (b"xor_check_threads", 0), (b"xor_tiles_per_slot", -1), (b"xor_wgs", 0)):
        dev.ecamd_tune(key, value)


def counters(dev):
    return (dev.ecamd_xor_check_fused_launches(), dev.ecamd_xor_locate_fused_launches(),
            dev.ecamd_check_fused_launches(), dev.ecamd_locate_fused_launches())


def encoder(k, m, hd):
    return lambda d: XO.encode_bytes(k, m, hd, d)


def encoded(seed, k, m, hd, nS, bs):
    """(nS, k+m, bs) reference-encoded stripes (XOR is bytewise: one encode of the stripes end to end)."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(k, nS * bs), dtype=np.uint8)
    full = np.concatenate([data, XO.encode_bytes(k, m, hd, data)])
    return np.ascontiguousarray(full.reshape(k + m, nS, bs).transpose(1, 0, 2))


def raw(dev, D, what, k, m, hd, base, stripe_stride, frag_stride, bs, nS):
    """ecamd_xor_check / _locate / _scrub on explicit pointers, both arrays canary-filled with GUARD
    words on either side: (rc, status, suspects, counts) with the canaries checked; status / suspects
    are None where the call left all nS words untouched."""
    n = nS + 2 * GUARD
    st, su = D.DeviceBuffer(4 * n), D.DeviceBuffer(4 * n)
    dev.ecamd_memset(st.ptr, CANARY, st.nbytes)
    dev.ecamd_memset(su.ptr, CANARY, su.nbytes)
    counts = [C.c_int(-3) for _ in range(3)]
    args = (k, m, hd, base, stripe_stride, frag_stride, bs, nS, st.ptr + 4 * GUARD)
    if what == "check":
        rc = dev.ecamd_xor_check(*args, None)
    elif what == "locate":
        rc = dev.ecamd_xor_locate(*args, su.ptr + 4 * GUARD, None)
    else:
        rc = dev.ecamd_xor_scrub(*args, su.ptr + 4 * GUARD, *[C.byref(c) for c in counts], None)
    dev.ecamd_synchronize()
    a, b = st.download().view(np.uint32).copy(), su.download().view(np.uint32).copy()
    st.free()
    su.free()
    for arr in (a, b):
        assert (arr[:GUARD] == CANARY32).all() and (arr[GUARD + nS:] == CANARY32).all(), what
    if what == "check":
        assert (b == CANARY32).all()
    a, b = a[GUARD:GUARD + nS], b[GUARD:GUARD + nS]
    return (rc, None if nS and (a == CANARY32).all() else a, None if nS and (b == CANARY32).all() else b,
            tuple(c.value for c in counts))


_batches = {}


def batch(k, m, hd, tile):
    """damaged_batch and the oracle's words for it, once per (code, tile)."""
    key = (k, m, hd, tile)
    if key not in _batches:
        n, bs = k + m, 2 * tile + TAIL
        good, bad, singles, pairs, clean = SW.damaged_batch(3000 + k + tile, k, n, bs, tile, list(range(n)), encoder(k, m, hd))
        want_st, want_su = SW.xor_oracle_locate(k, m, hd, bad)
        SW.assert_located(want_st, want_su, singles, pairs, clean, True)
        bad.setflags(write=False)
        _batches[key] = (bad, want_st, want_su)
    return _batches[key]


@pytest.mark.parametrize("threads,form_tile", FORMS)
@pytest.mark.parametrize("k,m,hd", CODES)
def test_every_culprit_fused_and_generic(D, knobs, k, m, hd, threads, form_tile):
    dev = knobs
    tile = max(form_tile, 2048)  # see the module docstring
    bad, want_st, want_su = batch(k, m, hd, tile)
    assert bad.shape[2] // form_tile >= 2 and bad.shape[2] % form_tile == TAIL
    lay = D.Layout.alloc(k + m, bad.shape[2], bad.shape[0])
    got = {}
    try:
        lay.upload_stripes(bad)
        dev.ecamd_tune(b"xor_check_threads", threads)
        for fused in (1, 0):
            dev.ecamd_tune(b"xor_check_fused", fused)
            c0 = counters(dev)
            st, su = D.xor_locate(k, m, hd, lay)
            chk = D.xor_check(k, m, hd, lay)
            c1 = counters(dev)
            assert (c1[0] > c0[0], c1[1] > c0[1]) == (bool(fused), bool(fused)), (fused, c0, c1)
            assert c1[2:] == c0[2:]
            wrong = np.nonzero((st != want_st) | (su != want_su) | (chk != want_st))[0]
            assert not len(wrong), (fused, [(int(s), hex(int(st[s])), hex(int(su[s])), hex(int(chk[s])), hex(int(want_st[s])),
                                             hex(int(want_su[s]))) for s in wrong[:6]])
            got[fused] = (st, su, chk)
        assert (lay.download_stripes() == bad).all()
    finally:
        lay.buf.free()
    for a, b in zip(got[1], got[0]):
        assert a.dtype == np.uint32 and a.tobytes() == b.tobytes()


def small_case(k, m, hd, bs, nS=4):
    """nS stripes of (k, m, hd): stripe 1 a data fragment in tile 0, stripe 2 a parity near the end,
    stripe 3 two fragments in different words; stripe 0 clean.  With the oracle's words."""
    held = encoded(4000 + bs, k, m, hd, nS, bs)
    SW.xor_word(held, 1, 4 % k, 64, 0x1234)
    SW.xor_word(held, 2, k + m - 1, (bs - 2) // 2 * 2, 0x00FF)
    SW.xor_word(held, 3, 0, 8, 0x8001)
    SW.xor_word(held, 3, k, (bs // 2) // 2 * 2, 0x0180)
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, held)
    assert not want_st[0] and want_su[1] == 1 << (4 % k) and want_su[2] == 1 << (k + m - 1) and want_st[3]
    return held, want_st, want_su


def run_layout(dev, D, k, m, hd, host, base_off, stripe_stride, frag_stride, bs, nS, want_st, want_su):
    """Check and locate on `host` uploaded at base_off of a buffer with a canary line on either side:
    the oracle's words, the fused path, and not one byte of the buffer changed."""
    pad = 256
    raw_host = np.full(pad + base_off + host.size + pad, CANARY, np.uint8)
    raw_host[pad + base_off:pad + base_off + host.size] = host.reshape(-1)
    buf = D.DeviceBuffer(raw_host.nbytes)
    try:
        buf.upload(raw_host)
        base = buf.ptr + pad + base_off
        assert base % 16 == 0 and (base % 128 == 0) == (base_off % 128 == 0)
        c0 = counters(dev)
        rc, st, _, _ = raw(dev, D, "check", k, m, hd, base, stripe_stride, frag_stride, bs, nS)
        assert rc == 0 and (st == want_st).all(), [hex(int(x)) for x in st]
        rc, st, su, _ = raw(dev, D, "locate", k, m, hd, base, stripe_stride, frag_stride, bs, nS)
        assert rc == 0 and (st == want_st).all() and (su == want_su).all(), [hex(int(x)) for x in su]
        c1 = counters(dev)
        assert c1[0] > c0[0] and c1[1] > c0[1] and c1[2:] == c0[2:]
        assert (buf.download() == raw_host).all()
    finally:
        buf.free()


@pytest.mark.parametrize("threads,tile", FORMS)
def test_layouts_and_canaries(D, knobs, threads, tile):
    dev = knobs
    k, m, hd, nS = 10, 6, 4, 4
    n, bs = k + m, 4096 + TAIL  # one 4 KiB tile or four 1 KiB tiles, and the tail
    assert bs // tile >= 1 and bs % tile == TAIL
    dev.ecamd_tune(b"xor_check_threads", threads)
    held, want_st, want_su = small_case(k, m, hd, bs)
    F = (bs + 15) // 16 * 16
    # a padded frag_stride, the padding a canary after each fragment; the base 128-aligned
    fs = F + 48
    host = np.full((nS, n, fs), CANARY, np.uint8)
    host[:, :, :bs] = held
    run_layout(dev, D, k, m, hd, host, 0, fs * n, fs, bs, nS, want_st, want_su)
    # the same at a base that is 16-aligned but not 128-aligned
    run_layout(dev, D, k, m, hd, host, 48, fs * n, fs, bs, nS, want_st, want_su)
    # fragment-major: [k+m][S][F]
    host = np.full((n, nS, F), CANARY, np.uint8)
    host[:, :, :bs] = held.transpose(1, 0, 2)
    run_layout(dev, D, k, m, hd, host, 16, F, nS * F, bs, nS, want_st, want_su)


@pytest.mark.parametrize("threads,tile", FORMS)
def test_sizes_around_one_tile(D, knobs, threads, tile):
    dev = knobs
    k, m, hd, nS = 10, 6, 4, 4
    dev.ecamd_tune(b"xor_check_threads", threads)

    def run(what, held):
        lay = D.Layout.alloc(k + m, held.shape[2], nS)
        try:
            lay.upload_stripes(held)
            c0 = counters(dev)
            out = raw(dev, D, what, k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, held.shape[2], nS)
            c1 = counters(dev)
            assert c1[2:] == c0[2:]
            return out, (c1[0] - c0[0], c1[1] - c0[1])
        finally:
            lay.buf.free()

    # a fragment shorter than a tile: nothing is fused
    held, want_st, want_su = small_case(k, m, hd, tile - 16)
    (rc, st, _, _), ran = run("check", held)
    assert rc == 0 and (st == want_st).all() and ran == (0, 0)
    (rc, st, su, _), ran = run("locate", held)
    assert rc == 0 and (st == want_st).all() and (su == want_su).all() and ran == (0, 0)
    # exactly one tile: all of it is fused, one launch, no tail for the generic path
    held, want_st, want_su = small_case(k, m, hd, tile)
    (rc, st, _, _), ran = run("check", held)
    assert rc == 0 and (st == want_st).all() and ran == (1, 0)
    (rc, st, su, _), ran = run("locate", held)
    assert rc == 0 and (st == want_st).all() and (su == want_su).all() and ran == (0, 1)
    # a tile and a 10-byte tail (tile + 10 is even, so locate runs too): a flip in the very last byte
    bs = tile + 10
    held = encoded(4100 + tile, k, m, hd, nS, bs)
    held[2, 7, bs - 1] ^= 0x80
    held[3, k + 1, tile - 1] ^= 0x01
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, held)
    assert want_su[2] == 1 << 7 and want_st[3] == want_su[3] == 1 << (k + 1) and not want_st[0] and not want_st[1]
    (rc, st, _, _), ran = run("check", held)
    assert rc == 0 and (st == want_st).all() and ran == (1, 0)
    (rc, st, su, _), ran = run("locate", held)
    assert rc == 0 and (st == want_st).all() and (su == want_su).all() and ran == (0, 1)
    # an odd size, tile + 11: the check as before, locate refuses and touches neither array
    bs = tile + 11
    held = encoded(4200 + tile, k, m, hd, nS, bs)
    held[2, 7, bs - 1] ^= 0x80
    want_st = SW.xor_status(k, m, hd, held)
    assert want_st[2] and not want_st[[0, 1, 3]].any()
    (rc, st, _, _), ran = run("check", held)
    assert rc == 0 and (st == want_st).all() and ran == (1, 0)
    (rc, st, su, _), ran = run("locate", held)
    assert rc == EINVAL and st is None and su is None and ran == (0, 0)


def test_launch_split_advances_every_pointer(D, knobs):
    """Knob xor_tiles_per_slot 1 with 3 slots per CU (knob xor_wgs): a launch takes at most 3 * CUs
    4 KiB tiles, so 2 * 3 * CUs + 1 one-tile stripes take exactly 3 launches."""
    import torch
    dev = knobs
    k, m, hd, bs = 3, 3, 3, 4096
    slots = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    nS = 2 * slots + 1
    held = encoded(5000, k, m, hd, nS, bs)
    first, mid, last = 1, slots + 5, nS - 1  # one damaged stripe in each launch's range
    SW.xor_word(held, first, 1, 100, 0x4242)
    SW.xor_word(held, mid, k + 2, 4000, 0x0001)
    SW.xor_word(held, last, 2, 2048, 0xFFFF)
    dirty = [first, mid, last]
    st3, su3 = SW.xor_oracle_locate(k, m, hd, held[dirty])
    assert list(su3) == [1 << 1, 1 << (k + 2), 1 << 2]
    want_st, want_su = np.zeros(nS, np.uint32), np.zeros(nS, np.uint32)  # the others are the reference's encode
    want_st[dirty], want_su[dirty] = st3, su3
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.upload_stripes(held)
        for key, value in ((b"xor_check_threads", 256), (b"xor_wgs", 3), (b"xor_tiles_per_slot", 1)):
            dev.ecamd_tune(key, value)
        c0 = counters(dev)
        st, su = D.xor_locate(k, m, hd, lay)
        chk = D.xor_check(k, m, hd, lay)
        c1 = counters(dev)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (3, 3) and c1[2:] == c0[2:]
        for got, want in ((st, want_st), (su, want_su), (chk, want_st)):
            assert (got == want).all(), (np.nonzero(got != want)[0][:8], [hex(int(x)) for x in got[dirty]])
    finally:
        lay.buf.free()


@pytest.mark.parametrize("threads,tile", FORMS)
def test_two_lanes_of_one_tile_and_one_fragment_in_two_tiles(D, knobs, threads, tile):
    dev = knobs
    k, m, hd, nS = 10, 6, 4, 3
    bs = 2 * tile
    held = encoded(6000 + tile, k, m, hd, nS, bs)
    # two different fragments in one tile, 16-byte chunks 0 and 62: lanes 0 and 62 of one wave, each
    # of which finds a culprit of its own -- only the AND across the wave leaves none
    SW.xor_word(held, 0, 2, tile + 10, 0x0101)
    SW.xor_word(held, 0, 5, tile + 1000, 0x7000)
    # the same fragment in two tiles
    SW.xor_word(held, 1, 3, 10, 0x0101)
    SW.xor_word(held, 1, 3, tile + 500, 0x0220)
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, held)
    assert want_st[0] and want_su[0] == 0 and want_su[1] == 1 << 3 and not want_st[2]
    dev.ecamd_tune(b"xor_check_threads", threads)
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.upload_stripes(held)
        c0 = counters(dev)
        st, su = D.xor_locate(k, m, hd, lay)
        assert counters(dev)[1] == c0[1] + 1
        assert (st == want_st).all() and (su == want_su).all(), ([hex(int(x)) for x in st], [hex(int(x)) for x in su])
    finally:
        lay.buf.free()


@pytest.mark.parametrize("k,m,hd", [(10, 6, 4), (3, 3, 3)])
def test_scrub_repairs_every_located_fragment_and_leaves_the_rest(D, knobs, k, m, hd):
    dev = knobs
    n, bs = k + m, 4096 + TAIL
    nS = 2 + n + 2
    good = encoded(7000 + k, k, m, hd, nS, bs)
    bad = good.copy()
    rng = np.random.default_rng(7100 + k)
    for f in range(n):  # stripe 1 + f: fragment f, in the tile or (every third) in the tail
        lo, hi = (4096, bs) if f % 3 == 2 else (0, 4096)
        SW.xor_word(bad, 1 + f, f, int(rng.integers(lo // 2, hi // 2)) * 2, int(rng.integers(1, 0x10000)))
        SW.xor_word(bad, 1 + f, f, int(rng.integers(0, bs // 2)) * 2, 0x8000)
    pairs = [1 + n, 2 + n]  # unrelated pairs: different fragments, different words
    SW.xor_word(bad, pairs[0], 0, 10, 0x0101)
    SW.xor_word(bad, pairs[0], 2, 2000, 0x0440)
    SW.xor_word(bad, pairs[1], 1, 300, 0x0003)
    SW.xor_word(bad, pairs[1], k + 1, 4096 + 20, 0x3000)
    clean = [0, nS - 1]
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, bad)
    for f in range(n):
        assert want_su[1 + f] == 1 << f
    assert not want_st[clean].any() and want_st[pairs].all() and not want_su[pairs].any()
    lay = D.Layout.alloc(n, bs, nS)
    try:
        lay.upload_stripes(bad)
        st0, su0 = D.xor_locate(k, m, hd, lay)
        assert (st0 == want_st).all() and (su0 == want_su).all()
        assert (lay.download_stripes() == bad).all()
        c0 = counters(dev)
        st, su, counts = D.xor_scrub(k, m, hd, lay)
        assert counters(dev)[1] > c0[1]
        assert counts == (2, n, 2), counts
        assert st.tobytes() == st0.tobytes() and su.tobytes() == su0.tobytes()
        after = lay.download_stripes()
        for s in range(nS):
            assert (after[s] == (bad[s] if s in pairs else good[s])).all(), s
        again = D.xor_check(k, m, hd, lay)
        assert list(np.nonzero(again)[0]) == pairs
    finally:
        lay.buf.free()


def test_scrub_of_a_pair_that_reads_as_a_third_fragment(D, knobs):
    """flat_xor_hd is not MDS: in (3,3,3) the same error in the same word of f1 and f2 is the syndrome
    of f3 alone.  Scrub names f3, counts the stripe repaired and leaves it consistent."""
    k, m, hd, bs, nS = 3, 3, 3, 4096 + TAIL, 2
    rc, sig = TP.plan(k, m, hd)
    assert rc == 0
    f1, f2, f3 = TP.sum_triple(sig)
    good = encoded(7500, k, m, hd, nS, bs)
    bad = good.copy()
    SW.xor_word(bad, 1, f1, 1234, 0x5AA5)
    SW.xor_word(bad, 1, f2, 1234, 0x5AA5)
    want_st, want_su = SW.xor_oracle_locate(k, m, hd, bad)
    assert want_st[1] and want_su[1] == 1 << f3 and not want_st[0]
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.upload_stripes(bad)
        st, su, counts = D.xor_scrub(k, m, hd, lay)
        assert (st == want_st).all() and (su == want_su).all() and counts == (1, 1, 0), (counts, hex(int(su[1])))
        assert not D.xor_check(k, m, hd, lay).any()
        after = lay.download_stripes()
        assert (after[0] == good[0]).all()
        others = [f for f in range(k + m) if f != f3]
        assert (after[1, others] == bad[1, others]).all() and (after[1, f3] != bad[1, f3]).any()
    finally:
        lay.buf.free()


def test_scrub_errors_and_empty_batch(D, knobs):
    dev = knobs
    nS, bs = 3, 4096
    host = np.random.default_rng(8000).integers(0, 256, size=16 * bs * nS, dtype=np.uint8)
    buf = D.DeviceBuffer(host.nbytes)
    try:
        buf.upload(host)
        for k, m, hd, size in ((10, 4, 9, bs), (10, 6, 4, bs - 1)):
            rc, st, su, counts = raw(dev, D, "scrub", k, m, hd, buf.ptr, 16 * bs, bs, size, nS)
            assert rc == EINVAL and st is None and su is None, (k, m, hd, size)
        assert (buf.download() == host).all()
        rc, st, su, counts = raw(dev, D, "scrub", 10, 6, 4, buf.ptr, 16 * bs, bs, bs, 0)
        assert rc == 0 and counts == (0, 0, 0) and not len(st) and not len(su)
        assert (buf.download() == host).all()
    finally:
        buf.free()
