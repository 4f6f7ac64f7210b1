"""GPU: the generic path's chunk loops, and scrub on (20,8) and (4,2).

check_generic (csrc/hip/ecamd_check.hip) walks a batch in stripe chunks over the shared scratch of
kCheckScratchBytes and a long fragment in byte ranges, with a clamp of its own at 65535 stripes for the
grid's y / z limit.  The tests here are sized so that each loop iterates twice: data are made on the
device (fill_splitmix + encode), damaged with a few small uploads, and the expected words of the damaged
stripes come from the oracles of test_gpu_locate / test_gpu_check on downloaded bytes -- whole stripes
where they are small, 4 KiB-aligned windows of every fragment around each damaged byte where they are
not (the codes are word-wise, and the rest of the stripe is encode output, which test_gpu_parity holds to
the reference).  Every other word must be 0 and the canary words past nstripes intact."""
import os
import re

import numpy as np
import pytest

import gfnp
import oracle_lib as orc
import test_gpu_check as TC
import test_gpu_locate as TL
import test_gpu_locate_sweep as SW
from ecdata import stripe_fragments
from test_gpu_check import D, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
TAIL = TC.TAIL
CANARY = TL.CANARY
CANARY32 = TL.CANARY32
EXTRA = 2
INTERNAL = os.path.join(TC.ROOT, "liberasurecode_amd", "csrc", "hip", "ecamd_internal.hpp")


def scratch_cap():
    text = open(INTERNAL).read()
    mo = re.search(r"constexpr\s+size_t\s+kCheckScratchBytes\s*=\s*size_t\((\d+)\)\s*<<\s*(\d+)\s*;", text)
    assert mo, "kCheckScratchBytes not found in ecamd_internal.hpp"
    return int(mo.group(1)) << int(mo.group(2))


def passes(nrows, bs, nstripes, start=0):
    """check_generic's plan restated: [(f0, len, stripes per pass)] for bytes [start, bs) of nrows rows."""
    cap = scratch_cap()
    seg = max(65536, cap // nrows // 65536 * 65536)
    out = []
    for f0 in range(start, bs, seg):
        ln = min(seg, bs - f0)
        pitch = (ln + 255) & ~255
        out.append((f0, ln, min(min(max(cap // (pitch * nrows), 1), 65535), nstripes)))
    return out


def canaried(dev, D, n):
    buf = D.DeviceBuffer(4 * (n + EXTRA))
    dev.ecamd_memset(buf.ptr, CANARY, buf.nbytes)
    return buf


def words_of(buf):
    w = buf.download().view(np.uint32).copy()
    buf.free()
    return w


def run_check_locate(dev, D, code, lay, missing=()):
    """(check status, locate status, suspects) of the layout, each nstripes + EXTRA words of which only
    the first nstripes may have been written.  code: (k, m) or (k, m, hd)."""
    from liberasurecode_amd import _lib
    n = lay.nstripes
    args = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, n)
    chk, st, su = canaried(dev, D, n), canaried(dev, D, n), canaried(dev, D, n)
    if len(code) == 2:
        miss = _lib.ints(list(missing) + [-1])
        _lib.check(dev.ecamd_rs_check(*code, miss, *args, chk.ptr, None, None), "rs_check")
        _lib.check(dev.ecamd_rs_locate(*code, miss, *args, st.ptr, su.ptr, None, None), "rs_locate")
    else:
        _lib.check(dev.ecamd_xor_check(*code, *args, chk.ptr, None), "xor_check")
        _lib.check(dev.ecamd_xor_locate(*code, *args, st.ptr, su.ptr, None), "xor_locate")
    _lib.check(dev.ecamd_synchronize(), "synchronize")
    out = [words_of(b) for b in (chk, st, su)]
    for w in out:
        assert (w[n:] == CANARY32).all(), TL.hexes(w[n:])
    return out


def stripe_bytes(lay, s, lo=0, hi=None):
    """Bytes [lo, hi) of every fragment of stripe s: (nfrags, hi - lo)."""
    hi = lay.blocksize if hi is None else hi
    if hi - lo == lay.blocksize and lay.stripe_stride == lay.frag_stride * lay.nfrags:
        raw = lay.buf.download(lay.stripe_stride, s * lay.stripe_stride).reshape(lay.nfrags, lay.frag_stride)
        return np.ascontiguousarray(raw[:, :lay.blocksize])
    return np.stack([lay.buf.download(hi - lo, s * lay.stripe_stride + f * lay.frag_stride + lo)
                     for f in range(lay.nfrags)])


def damage(lay, s, f, p, v):
    """XOR the 16-bit word at even offset p of fragment f of stripe s on the device."""
    at = s * lay.stripe_stride + f * lay.frag_stride + p
    w = lay.buf.download(2, at)
    w[0] ^= v & 0xFF
    w[1] ^= v >> 8
    lay.buf.upload(w, at)


def judge(code, held):
    """(status, suspects) of the stripes in held from the oracles alone."""
    if len(code) == 2:
        return TL.oracle_locate(*code, held, [])
    return SW.xor_oracle_locate(*code, held)


def expect(got, n, want):
    """got[:n] is zero but for the words of want {stripe: value}."""
    full = np.zeros(n, np.uint32)
    for s, v in want.items():
        full[s] = v
    bad = np.nonzero(got[:n] != full)[0]
    assert not len(bad), [(int(s), hex(int(got[s])), hex(int(full[s]))) for s in bad[:8]]


def test_stripe_chunks_of_4_2_and_scrub(D, dev):
    """(4,2) takes the generic path alone; 140 stripes of 256 KiB + 48 go in two passes over the scratch."""
    k, m, nS = 4, 2, 140
    bs = 256 * 1024 + TAIL
    plan = passes(m, bs, nS)
    assert len(plan) == 1
    per = plan[0][2]
    assert per < nS <= 2 * per  # two passes (127 + 13 with a 64 MiB scratch)
    dev.ecamd_tune(b"bitslice", 0)
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.fill_splitmix(nfrags=k, stripe0=5)
        D.rs_encode(k, m, lay)
        # the first stripe, the last of pass 1, the first of pass 2, the last: a culprit each, one of them two
        hits = {0: [(1, 20, 0x0100)], per - 1: [(k + 1, bs - 2, 0xFFFF)], per: [(3, 70000, 0x8001)],
                nS - 1: [(0, 4, 0x0040), (k, bs - 30, 0x2000)]}
        good = {s: stripe_bytes(lay, s) for s in hits}
        for s, hs in hits.items():
            for f, p, v in hs:
                damage(lay, s, f, p, v)
        bad = {s: stripe_bytes(lay, s) for s in hits}
        order = sorted(hits)
        want_st, want_su = judge((k, m), np.stack([bad[s] for s in order]))
        want_st, want_su = dict(zip(order, want_st)), dict(zip(order, want_su))
        for s in order:  # conditions on the inputs: one culprit is located, two in different words are not
            assert want_st[s]
            assert want_su[s] == (1 << hits[s][0][0] if len(hits[s]) == 1 else 0), (s, hex(int(want_su[s])))
        n0 = dev.ecamd_locate_fused_launches() + dev.ecamd_check_fused_launches()
        chk, st, su = run_check_locate(dev, D, (k, m), lay)
        expect(chk, nS, want_st)
        expect(st, nS, want_st)
        expect(su, nS, want_su)
        st, su, counts = D.rs_scrub(k, m, lay)
        assert counts == (nS - 4, 3, 1), counts
        expect(st, nS, want_st)
        expect(su, nS, want_su)
        for s in order:
            after = stripe_bytes(lay, s)
            assert (after == (good[s] if len(hits[s]) == 1 else bad[s])).all(), s
        again, _ = D.rs_check(k, m, lay)
        expect(again, nS, {nS - 1: want_st[nS - 1]})
        assert dev.ecamd_locate_fused_launches() + dev.ecamd_check_fused_launches() == n0
    finally:
        lay.buf.free()


@pytest.mark.parametrize("code", [(10, 4), (3, 3, 3)])
def test_more_stripes_than_one_grid_holds(D, dev, code):
    """65540 stripes of 32 bytes fit the scratch at once; the grid's y / z limit does not hold them."""
    k, m = code[:2]
    bs, nS = 32, 65540
    plan = passes(m, bs, nS)
    assert len(plan) == 1 and plan[0][2] == 65535 < nS
    dev.ecamd_tune(b"bitslice", 0)
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.fill_splitmix(nfrags=k, stripe0=9)
        if len(code) == 2:
            D.rs_encode(k, m, lay)
        else:
            D.xor_encode(*code, lay)
        hits = {0: (k - 1, 30, 0x00FF), 65534: (k + m - 1, 0, 0x0001), 65535: (0, 16, 0xFF00), 65539: (k, 14, 0x1234)}
        for s, (f, p, v) in hits.items():
            damage(lay, s, f, p, v)
        order = sorted(hits)
        want_st, want_su = judge(code, np.stack([stripe_bytes(lay, s) for s in order]))
        want_st, want_su = dict(zip(order, want_st)), dict(zip(order, want_su))
        for s in order:
            assert want_st[s] and want_su[s] == 1 << hits[s][0], (s, hex(int(want_su[s])))
        chk, st, su = run_check_locate(dev, D, code, lay)
        expect(chk, nS, want_st)
        expect(st, nS, want_st)
        expect(su, nS, want_su)
    finally:
        lay.buf.free()


def test_byte_ranges_of_20_8(D, dev):
    """(20,8) with fragments of 8 MiB + 64 KiB + 48: eight rows leave 8 MiB of scratch each, one stripe per
    pass, so every stripe goes in two byte ranges -- and the suspects must AND across the launches."""
    k, m, nS = 20, 8, 2
    bs = (8 << 20) + (64 << 10) + TAIL
    plan = passes(m, bs, nS)
    assert len(plan) == 2 and plan[0][2] == 1 < nS, plan  # both loops iterate
    r1 = plan[1][0]  # first byte of range 1
    a, b = 6, 17
    # stripe 0: one fragment in range 0 and in the 48-byte tail of the last range; stripe 1: a in range 0, b in range 1
    hits = {0: [(a, 5000, 0x0180), (a, bs - 20, 0x8000)], 1: [(a, 123456, 0x00F0), (b, r1 + 1000, 0x0F00)]}
    checked = sum(1 << f for f in range(k, k + m))
    dev.ecamd_tune(b"bitslice", 0)
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.fill_splitmix(nfrags=k, stripe0=3)
        D.rs_encode(k, m, lay)
        for s, hs in hits.items():
            for f, p, v in hs:
                damage(lay, s, f, p, v)
        held = []
        for s in sorted(hits):  # the damaged words' 4 KiB windows of every fragment, side by side
            wins = [stripe_bytes(lay, s, p & ~4095, min((p & ~4095) + 4096, bs)) for _, p, _ in hits[s]]
            wins[-1] = np.pad(wins[-1], ((0, 0), (0, 4096 - wins[-1].shape[1])))  # zeros encode to zeros
            held.append(np.concatenate(wins, axis=1))
        want_st, want_su = TL.oracle_locate(k, m, np.stack(held), [])
        assert list(want_st) == [checked, checked] and list(want_su) == [1 << a, 0], (TL.hexes(want_st), TL.hexes(want_su))
        n0 = dev.ecamd_locate_fused_launches(), dev.ecamd_check_fused_launches()
        generic = run_check_locate(dev, D, (k, m), lay)
        assert (dev.ecamd_locate_fused_launches(), dev.ecamd_check_fused_launches()) == n0
        for got, want in zip(generic, (want_st, want_st, want_su)):
            expect(got, nS, dict(enumerate(want)))
        # the fused tiles plus the generic 48-byte tail give the same words
        dev.ecamd_tune(b"bitslice", 2)
        fused = run_check_locate(dev, D, (k, m), lay)
        assert dev.ecamd_locate_fused_launches() > n0[0] and dev.ecamd_check_fused_launches() > n0[1]
        for x, y in zip(generic, fused):
            assert x.tobytes() == y.tobytes(), (TL.hexes(x), TL.hexes(y))
    finally:
        lay.buf.free()


def gf_mul(x, y):
    return int(gfnp.EXP[gfnp.LOG[x] + gfnp.LOG[y]]) if x and y else 0


def gf_div(x, y):
    return int(gfnp.EXP[gfnp.LOG[x] - gfnp.LOG[y] + 65535]) if x else 0


def mimic(k, m, f1, f2, f3, c):
    """Errors (e1, e2) in one word of data fragments f1 and f2 of an m = 2 code whose syndrome is that
    of the error c in data fragment f3 alone."""
    G = orc.generator(k, m)
    A = [[G[(k + r) * k + j] for j in range(k)] for r in range(m)]
    v = [gf_mul(c, A[0][f3]), gf_mul(c, A[1][f3])]
    det = gf_mul(A[0][f1], A[1][f2]) ^ gf_mul(A[0][f2], A[1][f1])
    assert det
    e1 = gf_div(gf_mul(v[0], A[1][f2]) ^ gf_mul(A[0][f2], v[1]), det)
    e2 = gf_div(gf_mul(A[0][f1], v[1]) ^ gf_mul(v[0], A[1][f1]), det)
    return e1, e2


@pytest.mark.parametrize("k,m", [(20, 8), (4, 2)])
def test_scrub_on_the_other_codes(D, dev, k, m):
    """test_gpu_locate's scrub scheme on (20,8) -- 16 KiB tiles, decode_multi with k = 20 -- and on (4,2),
    which is generic-only and, with two checked fragments, may name a wrong fragment when two are bad: the
    header documents that such a stripe is repaired to a consistent one, and the oracle says which."""
    tile = TC.tile_of(m)
    bs = 2 * tile + TAIL
    nS = 7
    good = np.empty((nS, k + m, bs), np.uint8)
    for s in range(nS):
        good[s, :k] = stripe_fragments(800 + s, k, bs)
        good[s, k:] = orc.encode(k, m, good[s, :k])
    bad = good.copy()
    bad[1, 3, tile + 900:tile + 940] ^= 0x5A      # a data fragment
    bad[2, k + m - 1, 17] ^= 0x01                 # a parity fragment
    bad[3, k - 1, 2 * tile + 30] ^= 0x80          # a byte of the tail
    bad[4, 0, 100] ^= 0x01                        # two bad fragments, different tiles
    bad[4, 2, tile + 100] ^= 0x01
    if m == 2:  # two bad fragments in one word that read as a third fragment's error
        e1, e2 = mimic(k, m, 0, 1, 2, 0x1D2C)
        SW.xor_word(bad, 5, 0, 4000, e1)
        SW.xor_word(bad, 5, 1, 4000, e2)
    else:       # m = 8 tells them apart
        SW.xor_word(bad, 5, 0, 4000, 0x0102)
        SW.xor_word(bad, 5, 1, 4000, 0x0201)
    want_st, want_su = TL.oracle_locate(k, m, bad, [])
    assert list(want_su[:5]) == [0, 1 << 3, 1 << (k + m - 1), 1 << (k - 1), 0] and want_st[1:6].all() and not want_st[6]
    assert want_su[5] == (1 << 2 if m == 2 else 0), hex(int(want_su[5]))
    after_want = bad.copy()
    after_want[1:4] = good[1:4]
    if m == 2:  # "repaired": the reference decode of the stripe with the named fragment listed as missing
        frags = [np.array(x) for x in bad[5]]
        assert orc.decode(k, m, frags, [2], 1) == 0
        after_want[5] = np.stack(frags)
        assert (after_want[5] != good[5]).any() and not TC.oracle_status(k, m, after_want[5:6], [])[0][0]
    located = 4 if m == 2 else 3
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.upload_stripes(bad)
        st, su, counts = D.rs_scrub(k, m, lay)
        assert counts == (2, located, 5 - located), counts
        assert (st == want_st).all() and (su == want_su).all(), (TL.hexes(st), TL.hexes(su), TL.hexes(want_su))
        after = lay.download_stripes()
        for s in range(nS):
            assert (after[s] == after_want[s]).all(), s
        again, _ = D.rs_check(k, m, lay)
        want_again, _ = TC.oracle_status(k, m, after_want, [])
        assert (again == want_again).all() and list(want_again != 0) == [s in (4, 5) and not (s == 5 and m == 2)
                                                                         for s in range(nS)]
        # an all-clean batch: nothing to repair, no byte written
        lay.upload_stripes(good)
        before = lay.buf.download()
        st, su, counts = D.rs_scrub(k, m, lay)
        assert counts == (nS, 0, 0) and not st.any() and not su.any()
        assert lay.buf.download().tobytes() == before.tobytes()
    finally:
        lay.buf.free()
