"""GPU: decode of stripes whose lost fragments are named by masks in device memory
(ecamd_rs_decode_masks, ecamd_frame_status_masks; include/ecamd.h).

T = 4096 bytes is the data kernel's tile (256 lanes of one 16-byte chunk).

Expected bytes never come from the code under test: good stripes are the reference encode's
(test_gpu_check.stripes), a lost slot holds 0x5A before the call and a rebuilt fragment must equal the good
one.  Everything else -- survivors, lost slots that are not rebuilt, the 0xA5 between blocksize and
frag_stride -- must be byte-identical to before, so every comparison is over the whole buffer."""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_gpu_check as TC
from test_gpu_check import D  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
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
    d.ecamd_tune(b"bitslice", 1)


def bits(*frags):
    return sum(1 << f for f in frags)


def lost_of(mask):
    return [f for f in range(32) if (mask >> f) & 1]


def recoverable(k, m, mask):
    return mask != 0 and mask >> (k + m) == 0 and len(lost_of(mask)) <= m


def want_result(k, m, mask, rp):
    if mask == 0:
        return 0
    if not recoverable(k, m, mask):
        return UNRECOVERABLE | len(lost_of(mask))
    return sum(1 for f in lost_of(mask) if f < k or rp)


def want_counts(results):
    r = np.asarray(results, np.uint32)
    return (int((r == 0).sum()), int(((r != 0) & (r < UNRECOVERABLE)).sum()), int((r >= UNRECOVERABLE).sum()))


def good_stripes(k, m, bs, n):
    full = TC.stripes(k, m, bs)
    return np.stack([full[s % TC.S] for s in range(n)])


def images(k, m, good, masks, rp, gap=16):
    """(before, after) host images [S][k+m][frag_stride]: 0xA5 between blocksize and frag_stride, 0x5A in
    every lost slot before; after, the good bytes in every slot the call must rebuild and nothing else
    changed."""
    nS, n, bs = good.shape
    fs = (bs + 15) // 16 * 16 + gap
    before = np.full((nS, n, fs), GAP, np.uint8)
    before[:, :, :bs] = good
    for s, mask in enumerate(masks):
        for f in lost_of(mask):
            if f < n:
                before[s, f, :bs] = FILL
    after = before.copy()
    for s, mask in enumerate(masks):
        if recoverable(k, m, mask):
            for f in lost_of(mask):
                if f < k or rp:
                    after[s, f, :bs] = good[s, f]
    return before, after


def raw_masks(dev, D, k, m, d_lost, rp, base, stripe_stride, frag_stride, bs, nS, stream=None, extra=3):
    """ecamd_rs_decode_masks on explicit pointers: (rc, d_result of nS + extra canary words, d_counts of 8)."""
    res, cnt = D.DeviceBuffer(4 * (max(nS, 0) + extra)), D.DeviceBuffer(32)
    for a in (res, cnt):
        dev.ecamd_memset(a.ptr, GAP, a.nbytes)
    rc = dev.ecamd_rs_decode_masks(k, m, d_lost, rp, base, stripe_stride, frag_stride, bs, nS, res.ptr, cnt.ptr, stream)
    dev.ecamd_synchronize()
    out = [a.download().view(np.uint32).copy() for a in (res, cnt)]
    for a in (res, cnt):
        a.free()
    return (rc, *out)


def run(dev, D, k, m, before, masks, rp, bs):
    """The call on an upload of `before`: (image afterwards, result words, counts)."""
    nS, n, fs = before.shape
    buf, lost = D.DeviceBuffer(before.nbytes), D.DeviceBuffer(4 * nS)
    try:
        buf.upload(before)
        lost.upload(np.asarray(masks, np.uint32))
        rc, res, cnt = raw_masks(dev, D, k, m, lost.ptr, int(rp), buf.ptr, n * fs, fs, bs, nS)
        assert rc == 0
        assert (res[nS:] == CANARY32).all() and (cnt[3:] == CANARY32).all()
        return buf.download().reshape(before.shape), res[:nS], tuple(int(c) for c in cnt[:3])
    finally:
        buf.free()
        lost.free()


def check_batch(dev, D, k, m, good, masks, rp):
    bs = good.shape[2]
    before, after = images(k, m, good, masks, rp)
    got, res, cnt = run(dev, D, k, m, before, masks, rp, bs)
    want = [want_result(k, m, mask, rp) for mask in masks]
    assert [int(r) for r in res] == want, [hex(int(r)) for r in res]
    assert cnt == want_counts(want), (cnt, want_counts(want))
    bad = np.nonzero((got != after).any(axis=2))
    assert not len(bad[0]), [(int(s), int(f), hex(masks[s])) for s, f in zip(*bad)][:8]
    return got


def cache_entries(dev):
    e, b, lim = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert dev.ecamd_map_cache_stats(C.byref(e), C.byref(b), C.byref(lim)) == 0
    return e.value


_every = {}


def every_pattern_10_4():
    """(good, masks): (10,4), blocksize T + 18, one stripe per pattern of at most 4 lost -- 1471 of them."""
    if not _every:
        k, m = 10, 4
        masks = [bits(*c) for r in range(m + 1) for c in itertools.combinations(range(k + m), r)]
        assert len(masks) == 1471 and len(set(masks)) == 1471
        _every["x"] = (good_stripes(k, m, T + 18, len(masks)), masks)
    return _every["x"]


@pytest.mark.parametrize("rp", [1, 0])
def test_every_pattern_of_10_4_in_one_batch(D, dev, rp):
    k, m = 10, 4
    good, masks = every_pattern_10_4()
    n0, b0, e0 = dev.ecamd_decode_masks_launches(), dev.ecamd_bitslice_launches(), cache_entries(dev)
    got = check_batch(dev, D, k, m, good, masks, rp)
    assert dev.ecamd_decode_masks_launches() == n0 + 1
    assert dev.ecamd_bitslice_launches() == b0 and cache_entries(dev) == e0
    if not rp:  # lost parity slots still hold 0x5A
        bs = good.shape[2]
        for s, mask in enumerate(masks):
            for f in lost_of(mask):
                if f >= k:
                    assert (got[s, f, :bs] == FILL).all(), (s, f)


SIZES = [2, 14, 16, 18, T - 2, T, T + 2, 3 * T + 18]
SIZE_MASKS = [0, bits(3), bits(11), bits(0, 5, 10, 13), bits(1, 2, 6, 9, 12)]


@pytest.mark.parametrize("bs", SIZES)
def test_sizes(D, dev, bs):
    k, m = 10, 4
    good = good_stripes(k, m, bs, len(SIZE_MASKS))
    before, _ = images(k, m, good, SIZE_MASKS, 1)
    got = check_batch(dev, D, k, m, good, SIZE_MASKS, 1)
    assert (got[4] == before[4]).all()  # five lost: byte-identical, result 0x80000005 (check_batch)


C5_LOST = [bits(*range(8)), bits(0, 2, 4, 6, 20, 22, 24, 26)]


def batch_20_8():
    return good_stripes(20, 8, T + 18, 3), C5_LOST + [bits(7)]


def test_20_8_both_c5_patterns_and_one_loss(D, dev):
    good, masks = batch_20_8()
    for rp in (1, 0):
        check_batch(dev, D, 20, 8, good, masks, rp)


def test_4_2_every_pattern(D, dev):
    k, m = 4, 2
    masks = [bits(*c) for r in range(m + 1) for c in itertools.combinations(range(k + m), r)]
    assert len(masks) == 22
    for rp in (1, 0):
        check_batch(dev, D, k, m, good_stripes(k, m, T + 18, len(masks)), masks, rp)


def test_24_8_eight_lost(D, dev):
    k, m = 24, 8
    rng = np.random.default_rng(24008)
    masks = [bits(*(int(f) for f in rng.choice(k + m, size=8, replace=False))) for _ in range(3)]
    check_batch(dev, D, k, m, good_stripes(k, m, T + 18, len(masks)), masks, 1)


def test_the_same_bytes_as_decode_multi(D, dev):
    """A second upload of the every-pattern batch through ecamd_rs_decode_multi (knob bitslice 0: its
    LDS-table kernels, so 1470 patterns start no compile): the whole buffers are equal."""
    k, m = 10, 4
    good, masks = every_pattern_10_4()
    bs = good.shape[2]
    before, _ = images(k, m, good, masks, 1)
    got, _, _ = run(dev, D, k, m, before, masks, 1, bs)
    nS, n, fs = before.shape
    buf = D.DeviceBuffer(before.nbytes)
    try:
        buf.upload(before)
        dev.ecamd_tune(b"bitslice", 0)
        D.rs_decode_multi(k, m, [lost_of(mask) for mask in masks], D.Layout(buf, n, bs, nS, fs, n * fs))
        D.synchronize()
        multi = buf.download().reshape(before.shape)
    finally:
        buf.free()
    assert got.tobytes() == multi.tobytes()


def test_pairs_grid_1_walks_both_grid_loops(D, dev):
    """One workgroup: the tile loop and the stripe loop both iterate; the same bytes."""
    cases = [(10, 4, good_stripes(10, 4, 3 * T + 18, len(SIZE_MASKS)), SIZE_MASKS), (20, 8, *batch_20_8())]
    for k, m, good, masks in cases:
        got = []
        for grid in (0, 1):
            dev.ecamd_tune(b"pairs_grid", grid)
            got.append(check_batch(dev, D, k, m, good, masks, 1))
        assert got[0].tobytes() == got[1].tobytes()


def test_stream_order_with_one_synchronise_at_the_end(D, dev):
    """The masks copied from pinned host memory on a created stream, the call enqueued right behind the
    copy, one wait at the end."""
    k, m = 10, 4
    masks = SIZE_MASKS + [bits(13), bits(0, 1, 2, 3)]
    nS, bs = len(masks), T + 18
    good = good_stripes(k, m, bs, nS)
    before, after = images(k, m, good, masks, 1)
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
        assert dev.ecamd_rs_decode_masks(k, m, d_lost.ptr, 1, buf.ptr, n * fs, fs, bs, nS, words.ptr, words.ptr + 4 * nS, s) == 0
        stream.synchronize()
        got = buf.download().reshape(before.shape)
        w = words.download().view(np.uint32)
    finally:
        if pin.value:
            dev.ecamd_host_free(pin)
        stream.destroy()
        for a in (buf, d_lost, words):
            a.free()
    want = [want_result(k, m, mask, 1) for mask in masks]
    assert [int(r) for r in w[:nS]] == want and tuple(int(c) for c in w[nS:]) == want_counts(want)
    assert (got == after).all()


def test_framed_chain_verify_masks_decode(D, dev):
    """verify -> status_masks(bit 4) -> decode_masks at the payload, one stream, one wait: payload damage in
    0..4 fragments per stripe is healed and the second audit is clean."""
    from liberasurecode_amd import frame as F
    k, m, nS = 10, 4, 8
    n = k + m
    fb = F.FrameBatch(F.RS_VAND, k, m, 10 * 1000, nS, checksum=F.CHKSUM_CRC32)
    bs = fb.blocksize
    assert bs % 2 == 0 and bs >= 64
    rng = np.random.default_rng(9300)
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
            bad = [int(f) for f in rng.choice(n, size=s % 5, replace=False)]
            want_masks.append(bits(*bad))
            for f in bad:
                hurt[s, f, F.HEADER + int(rng.integers(0, bs))] ^= 0x41
                hurt[s, f, F.HEADER + bs - 1] ^= 0x80
        fb.upload_fragments(hurt)
        d_status, d_crc, d_masks, d_words = (a.ptr for a in arrs)
        h = stream.handle
        assert dev.ecamd_frame_verify(n, bs, 0, fb.base, fb.stripe_stride, fb.frag_stride, nS, d_status, d_crc, h) == 0
        assert dev.ecamd_frame_status_masks(n, d_status, 1 << 4, nS, d_masks, h) == 0
        assert dev.ecamd_rs_decode_masks(k, m, d_masks, 1, fb.base + F.HEADER, fb.stripe_stride, fb.frag_stride, bs, nS,
                                         d_words, d_words + 4 * nS, h) == 0
        stream.synchronize()
        assert [int(v) for v in arrs[2].download().view(np.uint32)] == want_masks
        w = arrs[3].download().view(np.uint32)
        want = [s % 5 for s in range(nS)]
        assert [int(r) for r in w[:nS]] == want and tuple(int(c) for c in w[nS:]) == want_counts(want)
        assert (fb.fragments() == frags).all()
        assert not fb.verify()[0].any()
    finally:
        stream.destroy()
        for a in arrs + [d_obj, fb.buf]:
            a.free()


def test_status_masks_takes_any_of_the_bits(D, dev):
    nfrag, nS = 14, 300
    rng = np.random.default_rng(9400)
    status = (rng.integers(0, 32, size=(nS, nfrag)) * (rng.random((nS, nfrag)) < 0.2)).astype(np.uint32)
    st, out = D.DeviceBuffer(status.nbytes), D.DeviceBuffer(4 * nS + 8)
    try:
        st.upload(status)
        for which in (1 << 4, 0x0F, 0x1F):
            dev.ecamd_memset(out.ptr, GAP, out.nbytes)
            assert dev.ecamd_frame_status_masks(nfrag, st.ptr, which, nS, out.ptr, None) == 0
            dev.ecamd_synchronize()
            got = out.download().view(np.uint32)
            want = [bits(*[f for f in range(nfrag) if status[s, f] & which]) for s in range(nS)]
            assert [int(v) for v in got[:nS]] == want and (got[nS:] == CANARY32).all()
        for bad in ((0, st.ptr, out.ptr), (33, st.ptr, out.ptr), (nfrag, None, out.ptr), (nfrag, st.ptr, None)):
            dev.ecamd_memset(out.ptr, GAP, out.nbytes)
            assert dev.ecamd_frame_status_masks(bad[0], bad[1], 1, nS, bad[2], None) == EINVAL
            dev.ecamd_synchronize()
            assert (out.download().view(np.uint32) == CANARY32).all()
    finally:
        st.free()
        out.free()


def test_rejections_leave_everything_untouched(D, dev):
    k, m, nS, bs = 10, 4, TC.S, 4096
    host = np.random.default_rng(9200).integers(0, 256, size=32 * bs * nS, dtype=np.uint8)
    buf, lost = D.DeviceBuffer(host.nbytes), D.DeviceBuffer(4 * nS)

    def untouched(res, rc=EINVAL):
        assert res[0] == rc
        assert (res[1] == CANARY32).all() and (res[2] == CANARY32).all()
        assert (buf.download() == host).all()

    try:
        buf.upload(host)
        lost.upload(np.full(nS, bits(0, 1), np.uint32))
        n0 = dev.ecamd_decode_masks_launches()
        args = (buf.ptr, 32 * bs, bs)
        untouched(raw_masks(dev, D, k, m, None, 1, *args, bs, nS))                        # null d_lost
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, None, 32 * bs, bs, bs, nS))        # null base
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, buf.ptr + 8, 32 * bs, bs, bs, nS))  # base not 16-byte aligned
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, buf.ptr, 32 * bs + 8, bs, bs, nS))  # stripe_stride
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, buf.ptr, 32 * bs, bs + 8, bs, nS))  # frag_stride
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, buf.ptr, 32 * bs, bs - 16, bs, nS))  # frag_stride < blocksize
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, *args, 0, nS))                      # blocksize 0
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, *args, bs, -1))                     # nstripes < 0
        untouched(raw_masks(dev, D, 28, 5, lost.ptr, 1, *args, bs, nS))                    # k + m > 32
        untouched(raw_masks(dev, D, 10, 9, lost.ptr, 1, *args, bs, nS))                    # m > 8
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, *args, bs - 1, nS))                 # odd blocksize
        untouched(raw_masks(dev, D, k, m, lost.ptr, 1, *args, bs, 0), rc=0)                # an empty batch: 0, nothing written
        assert dev.ecamd_decode_masks_launches() == n0
    finally:
        buf.free()
        lost.free()
