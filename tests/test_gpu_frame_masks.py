"""GPU: whole framed fragments, headers included, rebuilt from masks in device memory
(ecamd_frame_reconstruct_masks, FrameBatch.reconstruct_masks / heal; include/ecamd.h).

Every expected byte comes from test_gpu_frame.expected_stripe (oracle parity plus ec_api.expected_header),
never from the code under test; stripe s of a batch holds object s % 8.  Before the call every lost slot,
header and payload, holds 0x5A and every gap -- fragment_len .. frag_stride of each slot and the `head`
bytes in front -- holds 0xA5.  After it the WHOLE device image must equal the expected image: that one
comparison covers "rebuilt right", "survivors untouched", "gaps untouched" and "unrecoverable stripes
untouched".

Flat XOR payloads are multiples of 4 bytes (get_aligned_data_size pads an object to k * 4), so no object
size gives a blocksize of 1 or 4097: the smallest and the "one tile plus a word" XOR shapes here are 4 and
4100 bytes."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ec_api
import test_gpu_frame as TF
from test_gpu_frame import F  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
FILL = 0x5A
GAP = 0xA5
CANARY32 = 0xA5A5A5A5
EINVAL = -22
UNRECOVERABLE = 0x80000000
CRC32, NONE, MD5 = ec_api.CHKSUM_CRC32, ec_api.CHKSUM_NONE, ec_api.CHKSUM_MD5
NOBJ = 8


@pytest.fixture()
def dev(F):
    from liberasurecode_amd import _lib
    d = _lib.dev()
    yield d
    for key, default in ((b"crc_bits", 0), (b"crc_pos", 1), (b"crc_span_kib", 0), (b"crc_gap_bits", 0),
                         (b"pairs_grid", 0)):
        d.ecamd_tune(key, default)


def bits(*frags):
    return sum(1 << f for f in frags)


def lost_of(mask):
    return [f for f in range(32) if (mask >> f) & 1]


def recoverable(name, k, m, hd, mask):
    """The issue's rule, restated: no bit at or past k+m, at most m bits (rs_vand), fewer than hd (flat XOR)."""
    n = len(lost_of(mask))
    return mask != 0 and mask >> (k + m) == 0 and (n <= m if name == "rs" else n < hd)


def want_result(name, k, m, hd, mask):
    if mask == 0:
        return 0
    return len(lost_of(mask)) if recoverable(name, k, m, hd, mask) else UNRECOVERABLE | len(lost_of(mask))


def want_counts(results):
    r = np.asarray(results, np.uint32)
    return (int((r == 0).sum()), int(((r != 0) & (r < UNRECOVERABLE)).sum()), int((r >= UNRECOVERABLE).sum()))


def masks_up_to(n, t):
    """0, then every mask of 1..t of n fragments."""
    return [0] + [bits(*c) for i in range(1, t + 1) for c in itertools.combinations(range(n), i)]


@functools.lru_cache(maxsize=None)
def good_stripe(name, k, m, hd, size, ct, legacy, o):
    """(k+m, fragment_len) uint8: the fragments liberasurecode_encode returns for object o (restated)."""
    obj = np.random.default_rng([size, o, k, m]).integers(0, 256, size, dtype=np.uint8).tobytes()
    frags = TF.expected_stripe(TF._backend(name), k, m, hd, obj, ct, legacy=legacy)
    out = np.stack([np.frombuffer(f, dtype=np.uint8) for f in frags])
    out.setflags(write=False)
    return out


def batch(F, name, k, m, hd, size, masks, ct=CRC32, legacy=False, align=128):
    """(FrameBatch, good[S][k+m][fragment_len], image before, image after) for one mask per stripe."""
    n, S = k + m, len(masks)
    fb = F.FrameBatch(TF._backend(name), k, m, size, S, hd=hd or 3, checksum=ct, align=align)
    good = np.stack([good_stripe(name, k, m, hd, size, ct, legacy, s % NOBJ) for s in range(S)])
    assert good.shape == (S, n, fb.fragment_len)
    before = np.full(fb.nbytes, GAP, np.uint8)
    view = fb._view(before)
    view[...] = good
    for s, mask in enumerate(masks):
        for f in lost_of(mask):
            if f < n:
                view[s, f, :] = FILL
    after = before.copy()
    view = fb._view(after)
    for s, mask in enumerate(masks):
        if recoverable(name, k, m, hd, mask):
            for f in lost_of(mask):
                view[s, f, :] = good[s, f]
    return fb, good, before, after


def where(fb, got, want):
    """The first differing byte of two images as (stripe, fragment, offset in the slot), for the message."""
    at = int(np.flatnonzero(got != want)[0])
    if at < fb.head:
        return ("head", at)
    s, r = divmod(at - fb.head, fb.stripe_stride)
    return (s, r // fb.frag_stride, r % fb.frag_stride, hex(int(got[at])), hex(int(want[at])))


def assert_image(fb, after):
    got = fb.buf.download(fb.nbytes)
    assert np.array_equal(got, after), where(fb, got, after)


def check_batch(F, name, k, m, hd, size, masks, ct=CRC32, legacy=False, align=128, verify=True):
    fb, good, before, after = batch(F, name, k, m, hd, size, masks, ct, legacy, align)
    fb.buf.upload(before)
    res, cnt = fb.reconstruct_masks(masks)
    want = [want_result(name, k, m, hd, mask) for mask in masks]
    assert [int(r) for r in res] == want, [hex(int(r)) for r in res][:16]
    assert cnt == want_counts(want), (cnt, want_counts(want))
    assert_image(fb, after)
    if verify and ct == CRC32:
        st, _ = fb.verify(legacy=legacy)
        ok = [s for s, mask in enumerate(masks) if mask == 0 or recoverable(name, k, m, hd, mask)]
        assert not st[ok].any(), np.argwhere(st[ok] != 0)[:8]
    return fb


# ---- 1. sizes ----

# the two masks with a bit at or past k+m on a middle stripe AND on the last one: a stamp indexed past
# k+m from a middle stripe lands inside the compared image
SIZE_MASKS = [0, bits(3), 0xFFFFFFFF, bits(14), bits(11), bits(0, 5, 10, 13), bits(1, 2, 6, 9, 12), bits(13),
              0xFFFFFFFF, bits(14)]
# blocksize 2; tail bytes only, exactly one chunk, one chunk plus tail; the decode tile's edge; 16 KiB and
# 18 bytes, 48 KiB and 6 bytes (one span each under the default crc_span_kib of 128: test_knobs runs 16402
# bytes as five spans of 4 KiB); and the smallest shape that takes two spans by default
BLOCKSIZES = [2, 14, 16, 18, 4094, 4096, 4098, 16402, 3 * 16384 + 6, 128 * 1024 + 18]


@pytest.mark.parametrize("bs", BLOCKSIZES)
def test_sizes(F, dev, bs):
    fb = check_batch(F, "rs", 10, 4, 0, 10 * bs - 1, SIZE_MASKS)
    assert fb.blocksize == bs


# ---- 2. every pattern of (10,4) in one batch ----

def test_every_pattern_10_4(F, dev):
    masks = masks_up_to(14, 4)
    assert len(masks) == 1471
    check_batch(F, "rs", 10, 4, 0, 10 * 1000, masks)


def test_every_pattern_10_4_without_checksum(F, dev):
    """CHKSUM_NONE: the header has no CRC, no span kernel runs, and the stamp kernel is counted."""
    masks = masks_up_to(14, 4)
    n0 = dev.ecamd_frame_reconstruct_masks_launches()
    check_batch(F, "rs", 10, 4, 0, 10 * 1000, masks, ct=NONE)
    assert dev.ecamd_frame_reconstruct_masks_launches() == n0 + 1


# ---- 3. other codes ----

def test_rs_4_2_every_pattern(F, dev):
    masks = masks_up_to(6, 2) + [bits(0, 1, 2), bits(6), 0xFFFFFFFF]
    for size in (4 * 1000 - 3, 4 * 4098):
        check_batch(F, "rs", 4, 2, 0, size, masks)


C5_LOST = [bits(*range(8)), bits(0, 2, 4, 6, 20, 22, 24, 26)]


def test_rs_20_8_c5_patterns(F, dev):
    masks = C5_LOST + [bits(7), bits(1, 3, 5, 9, 19, 21, 25, 27), bits(*range(9)), bits(28), 0]
    check_batch(F, "rs", 20, 8, 0, 20 * 4114 - 7, masks)


def test_rs_1_1(F, dev):
    masks = [0, bits(0), bits(1), bits(0, 1), bits(2)]
    for size in (1, 4099):
        check_batch(F, "rs", 1, 1, 0, size, masks)


@pytest.mark.parametrize("k,m,hd", [(3, 3, 3), (10, 5, 3), (10, 6, 4)])
def test_xor_every_pattern(F, dev, k, m, hd):
    """Every mask of fewer than hd bits, and masks of exactly hd bits -- refused, left untouched."""
    n = k + m
    refused = [bits(*c) for c in itertools.islice(itertools.combinations(range(n), hd), 0, None, 7)]
    masks = masks_up_to(n, hd - 1) + refused + [bits(n), 0xFFFFFFFF]
    assert check_batch(F, "xor", k, m, hd, 1, masks).blocksize == 4
    # one tile and a word: every 9th mask keeps the image small
    assert check_batch(F, "xor", k, m, hd, k * 4100 - 3, masks[::9] + masks[-2:]).blocksize == 4100


def test_xor_20_6_4_sample(F, dev):
    n = 26
    rng = np.random.default_rng(2064)
    masks = [bits(f) for f in range(n)]
    while len(masks) < n + 256:
        t = int(rng.integers(1, 5))  # 1..4 lost: 4 is refused
        masks.append(bits(*rng.choice(n, size=t, replace=False).tolist()))
    check_batch(F, "xor", 20, 6, 4, 20 * 1000, masks)


# ---- 4. the same bytes as the existing calls ----

@pytest.mark.parametrize("name,k,m,hd,lost", [("rs", 10, 4, 0, [3, 11]), ("rs", 10, 4, 0, [0, 5, 10, 13]),
                                              ("rs", 20, 8, 0, list(range(8))), ("xor", 10, 6, 4, [2, 5, 12]),
                                              ("xor", 3, 3, 3, [0, 3])])
def test_same_bytes_as_reconstruct_and_decode_masks(F, dev, name, k, m, hd, lost):
    from liberasurecode_amd.device import DeviceBuffer
    S, size = 3, k * 4100 - 3
    masks = [bits(*lost)] * S
    fb, good, before, after = batch(F, name, k, m, hd, size, masks)
    fb.buf.upload(before)
    fb.reconstruct_masks(masks)
    mine = fb.fragments()
    # ecamd_frame_reconstruct, one call per destination
    for dest in lost:
        fb.buf.upload(before)
        fb.reconstruct(lost, dest)
        assert np.array_equal(fb.fragments()[:, dest], mine[:, dest]), dest
    # ecamd_*_decode_masks at the payloads
    fb.buf.upload(before)
    d_lost = DeviceBuffer(4 * S)
    d_lost.upload(np.asarray(masks, np.uint32))
    if name == "rs":
        rc = dev.ecamd_rs_decode_masks(k, m, d_lost.ptr, 1, fb.base + 80, fb.stripe_stride, fb.frag_stride, fb.blocksize,
                                       S, None, None, None)
    else:
        rc = dev.ecamd_xor_decode_masks(k, m, hd, d_lost.ptr, 1, fb.base + 80, fb.stripe_stride, fb.frag_stride,
                                        fb.blocksize, S, None, None, None)
    assert rc == 0 and dev.ecamd_synchronize() == 0
    assert np.array_equal(fb.fragments()[:, :, 80:], mine[:, :, 80:])
    d_lost.free()


# ---- 5. knobs and variants ----

KNOBS = [(b, p, 4, 1, 0) for b in (4, 5, 6, 7, 8) for p in (0, 1)] + [(4, 0, 0, 0, 4), (5, 1, 0, 1, 0), (8, 0, 8, 0, 0)]


@pytest.mark.parametrize("crc_bits,crc_pos,span_kib,pairs_grid,gap_bits", KNOBS)
def test_knobs(F, dev, crc_bits, crc_pos, span_kib, pairs_grid, gap_bits):
    """Every form of the span kernel, spans of 4 KiB (five of them, the first one partial), and grids of one
    workgroup (grid-stride loops in the decode and in the masked span kernel): the same bytes."""
    for key, v in ((b"crc_bits", crc_bits), (b"crc_pos", crc_pos), (b"crc_span_kib", span_kib),
                   (b"pairs_grid", pairs_grid), (b"crc_gap_bits", gap_bits)):
        assert dev.ecamd_tune(key, v) == 0
    check_batch(F, "rs", 10, 4, 0, 10 * 16402 - 1, SIZE_MASKS)
    check_batch(F, "xor", 10, 6, 4, 10 * 4100 - 3, [bits(0, 1, 2), 0, bits(15), bits(3, 4, 5, 6), bits(9, 12)], verify=False)


def test_legacy_crc(F, dev, monkeypatch):
    monkeypatch.setenv("LIBERASURECODE_WRITE_LEGACY_CRC", "1")
    check_batch(F, "rs", 10, 4, 0, 10 * 4098 - 1, SIZE_MASKS, legacy=True)
    check_batch(F, "xor", 10, 5, 3, 10 * 1000, [bits(9, 12), bits(0), 0, bits(1, 2, 3)], legacy=True)


def test_md5_type_stored_not_computed(F, dev):
    check_batch(F, "rs", 4, 2, 0, 5000, [bits(0, 5), 0, bits(3), bits(0, 1, 2)], ct=MD5)


def test_packed_fragments(F, dev):
    """align 16: no head in front, the gap after a payload that is no multiple of 16 is its padding alone."""
    check_batch(F, "rs", 10, 4, 0, 10 * 4098 - 1, SIZE_MASKS, align=16)


# ---- 6. the chain ----

def damaged(F, nS=8):
    """8 encoded (10,4) stripes' worth of expected fragments, 0..4 whole fragments per stripe overwritten with
    0x5A (headers included) and one payload byte flipped in another fragment of two stripes: (batch, image
    before, image after, masks)."""
    whole = [[], [3], [0, 13], [1, 2, 12], [0, 5, 10, 13], [11], [4, 9], []]
    flips = {2: 6, 7: 8}  # stripe -> fragment with one payload byte flipped
    masks = [bits(*w) | (bits(flips[s]) if s in flips else 0) for s, w in enumerate(whole)]
    fb, good, before, after = batch(F, "rs", 10, 4, 0, 10 * 5000 - 3, [bits(*w) for w in whole])
    for img in (before,):
        v = fb._view(img)
        for s, f in flips.items():
            v[s, f, 80 + 1234] ^= 0x40
    return fb, before, after, masks


def test_chain_raw_calls_one_stream(F, dev):
    from liberasurecode_amd.device import DeviceBuffer, Stream
    fb, before, after, masks = damaged(F)
    nS, n = fb.nstripes, 14
    st, crc, words = DeviceBuffer(4 * nS * n), DeviceBuffer(4 * nS * n), DeviceBuffer(8 * nS + 12)
    stream = Stream()
    try:
        fb.buf.upload(before)
        s = stream.handle
        assert dev.ecamd_frame_verify(n, fb.blocksize, 0, fb.base, fb.stripe_stride, fb.frag_stride, nS, st.ptr, crc.ptr, s) == 0
        assert dev.ecamd_frame_status_masks(n, st.ptr, 0x1F, nS, words.ptr, s) == 0
        assert dev.ecamd_frame_reconstruct_masks(6, 10, 4, 0, CRC32, words.ptr, fb.base, fb.stripe_stride, fb.frag_stride,
                                                 fb.obj_size, nS, words.ptr + 4 * nS, words.ptr + 8 * nS, s) == 0
        stream.synchronize()
        w = words.download().view(np.uint32)
    finally:
        stream.destroy()
        for a in (st, crc, words):
            a.free()
    assert [int(x) for x in w[:nS]] == masks
    want = [len(lost_of(mask)) for mask in masks]
    assert [int(x) for x in w[nS:2 * nS]] == want and tuple(int(c) for c in w[2 * nS:]) == want_counts(want)
    assert_image(fb, after)
    assert not fb.verify()[0].any()


def test_chain_heal(F, dev):
    from liberasurecode_amd.device import Stream
    fb, before, after, masks = damaged(F)
    fb.buf.upload(before)
    stream = Stream()
    try:
        got_masks, res, cnt = fb.heal(stream=stream)
    finally:
        stream.destroy()
    want = [len(lost_of(mask)) for mask in masks]
    assert got_masks.tolist() == masks and res.tolist() == want and cnt == want_counts(want)
    assert_image(fb, after)
    assert not fb.verify()[0].any()
    # nothing left to heal: every mask empty, nothing written
    got_masks, res, cnt = fb.heal()
    assert not got_masks.any() and not res.any() and cnt == (fb.nstripes, 0, 0)
    assert_image(fb, after)


# ---- 7. stream order ----

def test_stream_order_with_one_synchronise_at_the_end(F, dev):
    """The masks copied from pinned host memory on a created stream right in front of the call; d_result NULL:
    the stamp stage reads the decode's words from library scratch."""
    from liberasurecode_amd.device import DeviceBuffer, Stream
    masks = SIZE_MASKS
    fb, good, before, after = batch(F, "rs", 10, 4, 0, 10 * 4114 - 1, masks)
    nS = len(masks)
    d_lost, cnt = DeviceBuffer(4 * nS), DeviceBuffer(32)
    pin = C.c_void_p()
    stream = Stream()
    try:
        assert dev.ecamd_host_alloc(C.byref(pin), 4 * nS) == 0
        np.ctypeslib.as_array((C.c_uint32 * nS).from_address(pin.value))[...] = masks
        fb.buf.upload(before)
        dev.ecamd_memset(d_lost.ptr, 0xFF, 4 * nS)  # unrecoverable everywhere unless the copy comes first
        dev.ecamd_memset(cnt.ptr, GAP, 32)
        s = stream.handle
        assert dev.ecamd_memcpy_async(d_lost.ptr, pin, 4 * nS, 0, s) == 0
        assert dev.ecamd_frame_reconstruct_masks(6, 10, 4, 0, CRC32, d_lost.ptr, fb.base, fb.stripe_stride, fb.frag_stride,
                                                 fb.obj_size, nS, None, cnt.ptr, s) == 0
        stream.synchronize()
        c = cnt.download().view(np.uint32)
    finally:
        if pin.value:
            dev.ecamd_host_free(pin)
        stream.destroy()
        d_lost.free()
        cnt.free()
    assert tuple(int(x) for x in c[:3]) == want_counts([want_result("rs", 10, 4, 0, mask) for mask in masks])
    assert (c[3:] == CANARY32).all()
    assert_image(fb, after)


# ---- 8. rejections ----

def test_rejections_leave_everything_untouched(F, dev):
    from liberasurecode_amd.device import DeviceBuffer
    masks = [bits(3), bits(0, 13), 0]
    fb, good, before, after = batch(F, "rs", 10, 4, 0, 10 * 1000, masks)
    nS = len(masks)
    d_lost, words = DeviceBuffer(4 * nS), DeviceBuffer(4 * nS + 32)
    d_lost.upload(np.asarray(masks, np.uint32))
    fb.buf.upload(before)
    dev.ecamd_memset(words.ptr, GAP, words.nbytes)
    ss, fs, size = fb.stripe_stride, fb.frag_stride, fb.obj_size

    def call(backend=6, k=10, m=4, hd=0, lost=d_lost.ptr, base=fb.base, ss=ss, fs=fs, n=nS):
        return dev.ecamd_frame_reconstruct_masks(backend, k, m, hd, CRC32, lost, base, ss, fs, size, n, words.ptr,
                                                 words.ptr + 4 * nS, None)

    bad = [call(lost=None), call(base=None), call(base=fb.base + 8), call(ss=ss + 8), call(fs=fs + 8),
           call(fs=80 + 992), call(k=10, m=9), call(k=25, m=8), call(backend=3, k=4, m=3, hd=3), call(backend=1),
           call(n=-1)]
    assert bad == [EINVAL] * len(bad), bad
    assert dev.ecamd_synchronize() == 0
    assert (words.download().view(np.uint32) == CANARY32).all()
    got = fb.buf.download(fb.nbytes)
    assert np.array_equal(got, before), where(fb, got, before)
    # nstripes 0: success, nothing written
    assert call(n=0) == 0 and dev.ecamd_synchronize() == 0
    assert (words.download().view(np.uint32) == CANARY32).all()
    assert np.array_equal(fb.buf.download(fb.nbytes), before)
    # and the batch is still healable
    res, cnt = fb.reconstruct_masks(masks)
    assert res.tolist() == [1, 2, 0] and cnt == (1, 2, 0)
    assert_image(fb, after)
    d_lost.free()
    words.free()
