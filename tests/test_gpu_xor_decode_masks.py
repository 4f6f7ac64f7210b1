"""GPU: decode of flat_xor_hd stripes whose lost fragments are named by masks in device memory
(ecamd_xor_decode_masks; include/ecamd.h).

T = 4096 bytes is the data kernel's tile (256 lanes of one 16-byte chunk).

Expected bytes never come from the code under test: they are oracle/xor_oracle.py's decode of the stripe
with zeroed lost slots, on random INCONSISTENT buffers, so a wrong choice of parity shows.  A lost slot
holds 0x5A before the call, the bytes between blocksize and frag_stride hold 0xA5, and the result and
count arrays are followed by canary words.  Everything the call must not write -- survivors, lost parity
without decode_parity, every slot of an unrecoverable stripe, the gaps -- must be byte-identical to before,
so every comparison is over the whole buffer."""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_gpu_check as TC
from test_gpu_check import D  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
XO = TC.XO
T = 4096
FILL = 0x5A
GAP = 0xA5
CANARY32 = 0xA5A5A5A5
EINVAL = -22
UNRECOVERABLE = 0x80000000


@pytest.fixture()
def dev(D):
    from liberasurecode_amd import _lib
    d = _lib.dev()
    yield d
    d.ecamd_tune(b"pairs_grid", 0)


def bits(*frags):
    return sum(1 << f for f in frags)


def lost_of(mask):
    return [f for f in range(32) if (mask >> f) & 1]


def recoverable(n, hd, mask):
    return mask != 0 and mask >> n == 0 and len(lost_of(mask)) < hd


def want_result(k, m, hd, mask, dp):
    if mask == 0:
        return 0
    if not recoverable(k + m, hd, mask):
        return UNRECOVERABLE | len(lost_of(mask))
    return sum(1 for f in lost_of(mask) if f < k or dp)


def want_counts(results):
    r = np.asarray(results, np.uint32)
    return (int((r == 0).sum()), int(((r != 0) & (r < UNRECOVERABLE)).sum()), int((r >= UNRECOVERABLE).sum()))


def every_mask(n, hd):
    return [bits(*c) for t in range(hd) for c in itertools.combinations(range(n), t)]


_batches = {}


def batch(k, m, hd, bs, masks, seed):
    """(held, rebuilt): held[s] is a random inconsistent stripe [k+m][bs]; rebuilt[s][f] is what the oracle's
    decode (decode_parity 1) of held[s] with the lost slots zeroed leaves in lost slot f.  The data rows do
    not depend on decode_parity: xor_hd_decode touches parity last, and only with the flag.  Computed once
    per batch and never modified."""
    key = (k, m, hd, bs, tuple(masks), seed)
    if key not in _batches:
        n = k + m
        held = np.random.default_rng(seed).integers(0, 256, size=(len(masks), n, bs), dtype=np.uint8)
        code = XO.XorCode(k, m, hd)
        rebuilt = []
        for s, mask in enumerate(masks):
            lost = lost_of(mask)
            if not recoverable(n, hd, mask):
                rebuilt.append({})
                continue
            bufs = [np.array(x) for x in held[s]]
            for f in lost:
                bufs[f][:] = 0
            for dp in (0, 1):  # decode_parity 0 first: its data rows must be those of decode_parity 1
                mine = [np.array(x) for x in bufs]
                assert code.decode(mine, lost, dp) == 0
                if dp == 0:
                    data_rows = {f: mine[f] for f in lost if f < k}
            assert all((mine[f] == data_rows[f]).all() for f in data_rows)
            rebuilt.append({f: mine[f] for f in lost})
        held.setflags(write=False)
        _batches[key] = (held, rebuilt)
    return _batches[key]


def images(k, m, hd, held, rebuilt, masks, dp, gap=16, fill=FILL):
    """(before, after) host images [S][k+m][frag_stride]: 0xA5 between blocksize and frag_stride, `fill` in
    every lost slot before; after, the oracle's bytes in every slot the call must rebuild, nothing else
    changed."""
    nS, n, bs = held.shape
    fs = (bs + 15) // 16 * 16 + gap
    before = np.full((nS, n, fs), GAP, np.uint8)
    before[:, :, :bs] = held
    for s, mask in enumerate(masks):
        for f in lost_of(mask):
            if f < n:
                before[s, f, :bs] = fill
    after = before.copy()
    for s, mask in enumerate(masks):
        for f, want in rebuilt[s].items():
            if f < k or dp:
                after[s, f, :bs] = want
    return before, after


def raw_masks(dev, D, k, m, hd, d_lost, dp, base, stripe_stride, frag_stride, bs, nS, stream=None, extra=3):
    """ecamd_xor_decode_masks on explicit pointers: (rc, d_result of nS + extra canary words, d_counts of 8)."""
    res, cnt = D.DeviceBuffer(4 * (max(nS, 0) + extra)), D.DeviceBuffer(32)
    for a in (res, cnt):
        dev.ecamd_memset(a.ptr, GAP, a.nbytes)
    rc = dev.ecamd_xor_decode_masks(k, m, hd, d_lost, dp, base, stripe_stride, frag_stride, bs, nS, res.ptr, cnt.ptr, stream)
    dev.ecamd_synchronize()
    out = [a.download().view(np.uint32).copy() for a in (res, cnt)]
    for a in (res, cnt):
        a.free()
    return (rc, *out)


def run(dev, D, k, m, hd, before, masks, dp, bs):
    """The call on an upload of `before`: (image afterwards, result words, counts)."""
    nS, n, fs = before.shape
    buf, lost = D.DeviceBuffer(before.nbytes), D.DeviceBuffer(4 * nS)
    try:
        buf.upload(before)
        lost.upload(np.asarray(masks, np.uint32))
        rc, res, cnt = raw_masks(dev, D, k, m, hd, lost.ptr, int(dp), buf.ptr, n * fs, fs, bs, nS)
        assert rc == 0
        assert (res[nS:] == CANARY32).all() and (cnt[3:] == CANARY32).all()
        return buf.download().reshape(before.shape), res[:nS], tuple(int(c) for c in cnt[:3])
    finally:
        buf.free()
        lost.free()


def check_batch(dev, D, k, m, hd, bs, masks, dp, seed):
    held, rebuilt = batch(k, m, hd, bs, masks, seed)
    before, after = images(k, m, hd, held, rebuilt, masks, dp)
    got, res, cnt = run(dev, D, k, m, hd, before, masks, dp, bs)
    want = [want_result(k, m, hd, mask, dp) for mask in masks]
    assert [int(r) for r in res] == want, [hex(int(r)) for r in res][:16]
    assert cnt == want_counts(want), (cnt, want_counts(want))
    bad = np.nonzero((got != after).any(axis=2))
    assert not len(bad[0]), [(int(s), int(f), hex(masks[s])) for s, f in zip(*bad)][:8]
    return got


def cache_entries(dev):
    e, b, lim = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert dev.ecamd_map_cache_stats(C.byref(e), C.byref(b), C.byref(lim)) == 0
    return e.value


@pytest.mark.parametrize("dp", [1, 0])
def test_every_pattern_of_10_6_4_in_one_batch(D, dev, dp):
    k, m, hd, bs = 10, 6, 4, T + 18
    masks = every_mask(k + m, hd)
    assert len(masks) == 697 and len(set(masks)) == 697
    n0, x0, e0 = dev.ecamd_xor_decode_masks_launches(), dev.ecamd_xor_stream_launches(), cache_entries(dev)
    got = check_batch(dev, D, k, m, hd, bs, masks, dp, 6400)
    assert dev.ecamd_xor_decode_masks_launches() == n0 + 1
    assert dev.ecamd_xor_stream_launches() == x0 and cache_entries(dev) == e0
    if not dp:  # lost parity slots still hold 0x5A
        for s, mask in enumerate(masks):
            for f in lost_of(mask):
                if f >= k:
                    assert (got[s, f, :bs] == FILL).all(), (s, f)


def test_every_pattern_of_20_6_4(D, dev):
    """2952 stripes of one partial tile."""
    k, m, hd = 20, 6, 4
    masks = every_mask(k + m, hd)
    assert len(masks) == 2952
    check_batch(dev, D, k, m, hd, 274, masks, 1, 6401)


@pytest.mark.parametrize("k,m,hd,count", [(3, 3, 3, 22), (10, 5, 3, 121), (15, 6, 3, 232)])
def test_every_pattern_of_the_hd_3_codes(D, dev, k, m, hd, count):
    masks = every_mask(k + m, hd)
    assert len(masks) == count
    for dp in (1, 0):
        check_batch(dev, D, k, m, hd, T + 18, masks, dp, 6402 + k)


SIZES = [1, 2, 15, 16, 17, T - 1, T, T + 1, 3 * T + 18, 17 * T + 2]  # the last: a second tile column
SIZE_MASKS = [0, bits(3), bits(11), bits(0, 5, 12), bits(1, 11, 13), bits(2, 4, 6, 8)]


@pytest.mark.parametrize("bs", SIZES)
def test_sizes(D, dev, bs):
    k, m, hd = 10, 6, 4
    for dp in (1, 0):
        check_batch(dev, D, k, m, hd, bs, SIZE_MASKS, dp, 6410)


def test_unrecoverable_stripes_are_left_as_they_were(D, dev):
    k, m, hd, bs = 10, 6, 4, T + 18
    masks = [bits(0, 1, 2, 3), bits(12, 13, 14, 15), bits(0, 9, 10, 15), bits(16), bits(3, 16), bits(31), 0xFFFFFFFF,
             bits(*range(16)), bits(5)]
    held, rebuilt = batch(k, m, hd, bs, masks, 6420)
    before, _ = images(k, m, hd, held, rebuilt, masks, 1)
    got = check_batch(dev, D, k, m, hd, bs, masks, 1, 6420)
    assert (got[:8] == before[:8]).all() and not (got[8] == before[8]).all()
    # (10,5,3): exactly hd = 3 lost is one too many there, though it is a pattern of (10,6,4)
    masks3 = [bits(0, 5, 12), bits(0, 5), bits(15), bits(14)]
    held, rebuilt = batch(10, 5, 3, bs, masks3, 6421)
    before, _ = images(10, 5, 3, held, rebuilt, masks3, 1)
    got = check_batch(dev, D, 10, 5, 3, bs, masks3, 1, 6421)
    assert (got[0] == before[0]).all() and (got[2] == before[2]).all()


def test_the_same_bytes_as_decode_multi(D, dev):
    """Every pattern of (10,6,4) on an upload whose lost slots are zeroed, and a second upload of it through
    ecamd_xor_decode_multi with the ascending lists: the whole buffers are equal, for both flags."""
    k, m, hd, bs = 10, 6, 4, T + 18
    masks = every_mask(k + m, hd)
    held, rebuilt = batch(k, m, hd, bs, masks, 6400)
    for dp in (1, 0):
        before, _ = images(k, m, hd, held, rebuilt, masks, dp, fill=0)
        got, _, _ = run(dev, D, k, m, hd, before, masks, dp, bs)
        nS, n, fs = before.shape
        buf = D.DeviceBuffer(before.nbytes)
        try:
            buf.upload(before)
            D.xor_decode_multi(k, m, hd, [lost_of(mask) for mask in masks], D.Layout(buf, n, bs, nS, fs, n * fs), decode_parity=dp)
            D.synchronize()
            multi = buf.download().reshape(before.shape)
        finally:
            buf.free()
        assert got.tobytes() == multi.tobytes()


def test_pairs_grid_1_walks_both_grid_loops(D, dev):
    """One workgroup: the tile loop and the stripe loop both iterate; the same bytes."""
    got = []
    for grid in (0, 1):
        dev.ecamd_tune(b"pairs_grid", grid)
        got.append(check_batch(dev, D, 10, 6, 4, 3 * T + 18, SIZE_MASKS, 1, 6410))
    assert got[0].tobytes() == got[1].tobytes()


def test_stream_order_with_one_synchronise_at_the_end(D, dev):
    """The masks copied from pinned host memory on a created stream, the call enqueued right behind the
    copy, one wait at the end."""
    k, m, hd, bs = 10, 6, 4, T + 18
    masks = SIZE_MASKS + [bits(15), bits(0, 1, 2)]
    nS = len(masks)
    held, rebuilt = batch(k, m, hd, bs, masks, 6430)
    before, after = images(k, m, hd, held, rebuilt, masks, 1)
    _, n, fs = before.shape
    buf, d_lost, words = D.DeviceBuffer(before.nbytes), D.DeviceBuffer(4 * nS), D.DeviceBuffer(4 * nS + 12)
    pin = C.c_void_p()
    stream = D.Stream()
    try:
        assert dev.ecamd_host_alloc(C.byref(pin), 4 * nS) == 0
        np.ctypeslib.as_array((C.c_uint32 * nS).from_address(pin.value))[...] = masks
        buf.upload(before)
        dev.ecamd_memset(d_lost.ptr, 0xFF, 4 * nS)  # unrecoverable everywhere unless the copy comes first
        s = stream.handle
        assert dev.ecamd_memcpy_async(d_lost.ptr, pin, 4 * nS, 0, s) == 0
        assert dev.ecamd_xor_decode_masks(k, m, hd, d_lost.ptr, 1, buf.ptr, n * fs, fs, bs, nS, words.ptr, words.ptr + 4 * nS, s) == 0
        stream.synchronize()
        got = buf.download().reshape(before.shape)
        w = words.download().view(np.uint32)
    finally:
        if pin.value:
            dev.ecamd_host_free(pin)
        stream.destroy()
        for a in (buf, d_lost, words):
            a.free()
    want = [want_result(k, m, hd, mask, 1) for mask in masks]
    assert [int(r) for r in w[:nS]] == want and tuple(int(c) for c in w[nS:]) == want_counts(want)
    assert (got == after).all()


def test_framed_chain_verify_masks_decode(D, dev):
    """Backend 3: verify -> status_masks(bit 4) -> xor_decode_masks at the payload, one stream, one wait:
    payload damage in 0..3 fragments per stripe is healed and the second audit is clean."""
    from liberasurecode_amd import frame as F
    k, m, hd, nS = 10, 6, 4, 8
    n = k + m
    fb = F.FrameBatch(F.FLAT_XOR_HD, k, m, 10 * 1000, nS, hd=hd, checksum=F.CHKSUM_CRC32)
    bs = fb.blocksize
    assert bs >= 64
    rng = np.random.default_rng(9310)
    objs = rng.integers(0, 256, size=nS * fb.obj_stride, dtype=np.uint8)
    d_obj = D.DeviceBuffer(objs.nbytes)
    arrs = [D.DeviceBuffer(4 * nS * n), D.DeviceBuffer(4 * nS * n), D.DeviceBuffer(4 * nS), D.DeviceBuffer(4 * nS + 12)]
    stream = D.Stream()
    try:
        d_obj.upload(objs)
        fb.encode(d_obj)
        dev.ecamd_synchronize()
        frags = fb.fragments()
        hurt = frags.copy()
        want_masks = []
        for s in range(nS):
            bad = [int(f) for f in rng.choice(n, size=s % 4, replace=False)]
            want_masks.append(bits(*bad))
            for f in bad:
                hurt[s, f, F.HEADER + int(rng.integers(0, bs))] ^= 0x41
                hurt[s, f, F.HEADER + bs - 1] ^= 0x80
        fb.upload_fragments(hurt)
        d_status, d_crc, d_masks, d_words = (a.ptr for a in arrs)
        h = stream.handle
        assert dev.ecamd_frame_verify(n, bs, 0, fb.base, fb.stripe_stride, fb.frag_stride, nS, d_status, d_crc, h) == 0
        assert dev.ecamd_frame_status_masks(n, d_status, 1 << 4, nS, d_masks, h) == 0
        assert dev.ecamd_xor_decode_masks(k, m, hd, d_masks, 1, fb.base + F.HEADER, fb.stripe_stride, fb.frag_stride, bs, nS,
                                          d_words, d_words + 4 * nS, h) == 0
        stream.synchronize()
        assert [int(v) for v in arrs[2].download().view(np.uint32)] == want_masks
        w = arrs[3].download().view(np.uint32)
        want = [s % 4 for s in range(nS)]
        assert [int(r) for r in w[:nS]] == want and tuple(int(c) for c in w[nS:]) == want_counts(want)
        assert (fb.fragments() == frags).all()
        assert not fb.verify()[0].any()
    finally:
        stream.destroy()
        for a in arrs + [d_obj, fb.buf]:
            a.free()


def test_device_py_returns_result_and_counts(D, dev):
    k, m, hd, bs = 10, 6, 4, 274
    masks = SIZE_MASKS
    held, rebuilt = batch(k, m, hd, bs, masks, 6440)
    lay = D.Layout.alloc(k + m, bs, len(masks))
    try:
        want_frags = np.array(held)
        for s, mask in enumerate(masks):
            for f in lost_of(mask):
                want_frags[s, f] = rebuilt[s].get(f, FILL)
        start = np.array(held)
        for s, mask in enumerate(masks):
            start[s, lost_of(mask)] = FILL
        lay.upload_stripes(start)
        res, cnt = D.xor_decode_masks(k, m, hd, masks, lay)
        want = [want_result(k, m, hd, mask, 1) for mask in masks]
        assert [int(r) for r in res] == want and cnt == want_counts(want)
        assert (lay.download_stripes() == want_frags).all()
    finally:
        lay.buf.free()


def test_rejections_leave_everything_untouched(D, dev):
    k, m, hd, nS, bs = 10, 6, 4, 3, 4096
    host = np.random.default_rng(9210).integers(0, 256, size=32 * bs * nS, dtype=np.uint8)
    buf, lost = D.DeviceBuffer(host.nbytes), D.DeviceBuffer(4 * nS)

    def untouched(res, rc=EINVAL):
        assert res[0] == rc
        assert (res[1] == CANARY32).all() and (res[2] == CANARY32).all()
        assert (buf.download() == host).all()

    try:
        buf.upload(host)
        lost.upload(np.full(nS, bits(0, 1), np.uint32))
        n0 = dev.ecamd_xor_decode_masks_launches()
        args = (buf.ptr, 32 * bs, bs)
        untouched(raw_masks(dev, D, k, m, hd, None, 1, *args, bs, nS))                        # null d_lost
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, None, 32 * bs, bs, bs, nS))        # null base
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, buf.ptr + 8, 32 * bs, bs, bs, nS))  # base not 16-byte aligned
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, buf.ptr, 32 * bs + 8, bs, bs, nS))  # stripe_stride
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, buf.ptr, 32 * bs, bs + 8, bs, nS))  # frag_stride
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, buf.ptr, 32 * bs, bs - 16, bs, nS))  # frag_stride < blocksize
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, *args, 0, nS))                      # blocksize 0
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, *args, bs, -1))                     # nstripes < 0
        for code in ((10, 4, 3), (21, 6, 4), (10, 6, 5), (10, 6, 2), (0, 6, 4), (10, 0, 4), (28, 6, 4)):
            untouched(raw_masks(dev, D, *code, lost.ptr, 1, *args, bs, nS))                    # not a code of init_xor_hd_code
        untouched(raw_masks(dev, D, k, m, hd, lost.ptr, 1, *args, bs, 0), rc=0)                # an empty batch: 0, nothing written
        assert dev.ecamd_xor_decode_masks_launches() == n0
    finally:
        buf.free()
        lost.free()
