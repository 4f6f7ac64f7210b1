"""Device-resident batched erasure coding on MI355X (Python face of include/ecamd.h).

Buffers are plain HBM allocations made by libecamd (no torch types); a batch of S stripes is a
strided layout where fragment f of stripe s lives at base + s*stripe_stride + f*frag_stride.
"""
import ctypes as C

import numpy as np

from ._lib import check, dev, i64s, ints, u32s


def available() -> bool:
    try:
        return dev().ecamd_init() == 0
    except Exception:
        return False


class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(dev().ecamd_malloc(C.byref(p), self.nbytes), "ecamd_malloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            dev().ecamd_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        check(dev().ecamd_memcpy_h2d(self.ptr + offset, arr.ctypes.data, arr.nbytes), "h2d")

    def download(self, nbytes=None, offset: int = 0) -> np.ndarray:
        n = self.nbytes - offset if nbytes is None else int(nbytes)
        out = np.empty(n, dtype=np.uint8)
        check(dev().ecamd_memcpy_d2h(out.ctypes.data, self.ptr + offset, n), "d2h")
        return out

    def zero(self):
        check(dev().ecamd_memset(self.ptr, 0, self.nbytes), "memset")


class Stream:
    def __init__(self):
        p = C.c_void_p()
        check(dev().ecamd_stream_create(C.byref(p)), "stream")
        self.handle = p.value

    def synchronize(self):
        check(dev().ecamd_stream_synchronize(self.handle), "stream sync")

    def destroy(self):
        """ecamd_stream_destroy: the stream and the library's context for it."""
        if self.handle:
            check(dev().ecamd_stream_destroy(self.handle), "stream destroy")
            self.handle = None


class Event:
    def __init__(self):
        p = C.c_void_p()
        check(dev().ecamd_event_create(C.byref(p)), "event")
        self.handle = p.value

    def record(self, stream=None):
        check(dev().ecamd_event_record(self.handle, stream.handle if stream else None), "record")

    def elapsed_ms(self, end: "Event") -> float:
        ms = C.c_float()
        check(dev().ecamd_event_elapsed_ms(self.handle, end.handle, C.byref(ms)), "elapsed")
        return ms.value


def _s(stream):
    return stream.handle if stream is not None else None


class Layout:
    """Strided batch layout of S stripes x F fragments of `blocksize` bytes."""

    def __init__(self, buf: DeviceBuffer, nfrags: int, blocksize: int, nstripes: int,
                 frag_stride=None, stripe_stride=None):
        self.buf = buf
        self.nfrags = nfrags
        self.blocksize = blocksize
        self.nstripes = nstripes
        self.frag_stride = frag_stride or (blocksize + 15) // 16 * 16
        self.stripe_stride = stripe_stride or self.frag_stride * nfrags

    @classmethod
    def alloc(cls, nfrags, blocksize, nstripes):
        fs = (blocksize + 15) // 16 * 16
        buf = DeviceBuffer(fs * nfrags * nstripes)
        return cls(buf, nfrags, blocksize, nstripes, fs, fs * nfrags)

    def upload_stripes(self, frags: np.ndarray):
        """frags: (S, F, blocksize) uint8."""
        S, F, bs = frags.shape
        host = np.zeros((S, self.stripe_stride), dtype=np.uint8)
        for f in range(F):
            host[:, f * self.frag_stride:f * self.frag_stride + bs] = frags[:, f]
        self.buf.upload(host)

    def download_stripes(self) -> np.ndarray:
        raw = self.buf.download(self.stripe_stride * self.nstripes).reshape(self.nstripes,
                                                                             self.stripe_stride)
        out = np.empty((self.nstripes, self.nfrags, self.blocksize), dtype=np.uint8)
        for f in range(self.nfrags):
            out[:, f] = raw[:, f * self.frag_stride:f * self.frag_stride + self.blocksize]
        return out

    def fill_splitmix(self, nfrags=None, stripe0=0, seed_base=0xEC0DE, stream=None):
        check(dev().ecamd_fill_splitmix(self.buf.ptr, self.stripe_stride, self.frag_stride,
                                        nfrags or self.nfrags, self.blocksize, self.nstripes,
                                        stripe0, seed_base, _s(stream)), "fill")


def rs_encode(k, m, lay: Layout, stream=None):
    check(dev().ecamd_rs_encode(k, m, lay.buf.ptr, lay.stripe_stride, lay.frag_stride,
                                lay.blocksize, lay.nstripes, _s(stream)), "rs_encode")


def rs_decode(k, m, missing, lay: Layout, rebuild_parity=True, stream=None):
    check(dev().ecamd_rs_decode(k, m, ints(list(missing) + [-1]), int(rebuild_parity), lay.buf.ptr,
                                lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes,
                                _s(stream)), "rs_decode")


def rs_decode_multi(k, m, missing_per_stripe, lay: Layout, rebuild_parity=True, stream=None):
    """One erasure list per stripe; stripes are grouped by pattern on the host."""
    width = m + 1
    flat = []
    for pat in missing_per_stripe:
        row = list(pat)[:m] + [-1] * (width - min(len(pat), m))
        flat += row
    check(dev().ecamd_rs_decode_multi(k, m, ints(flat), width, int(rebuild_parity), lay.buf.ptr,
                                      lay.stripe_stride, lay.frag_stride, lay.blocksize,
                                      lay.nstripes, _s(stream)), "rs_decode_multi")


def rs_reconstruct(k, m, missing, dest, lay: Layout, stream=None):
    check(dev().ecamd_rs_reconstruct(k, m, ints(list(missing) + [-1]), dest, lay.buf.ptr,
                                     lay.stripe_stride, lay.frag_stride, lay.blocksize,
                                     lay.nstripes, _s(stream)), "rs_reconstruct")


def _status(call, lay, stream, what):
    """Run call(d_status) and return the nstripes status words (waits for `stream`)."""
    buf = DeviceBuffer(4 * max(lay.nstripes, 1))
    try:
        check(call(buf.ptr), what)
        if stream is not None:
            stream.synchronize()
        return buf.download(4 * lay.nstripes).view(np.uint32).copy()
    finally:
        buf.free()


def rs_check(k, m, lay: Layout, missing=(), stream=None):
    """ecamd_rs_check: (status, checked_mask).  status[s] has bit f set when available fragment f of
    stripe s -- one that is not among the first k available, the inputs -- differs from what the
    inputs imply; checked_mask has the bits of the fragments that were checked."""
    checked = C.c_uint32(0)
    status = _status(lambda d: dev().ecamd_rs_check(
        k, m, ints(list(missing) + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
        lay.nstripes, d, C.byref(checked), _s(stream)), lay, stream, "rs_check")
    return status, checked.value


def xor_check(k, m, hd, lay: Layout, stream=None, missing=()):
    """ecamd_xor_check: status[s] has bit k + p set when stored parity p of stripe s differs from the
    XOR its parity bitmap names.  With a non-empty `missing`, ecamd_xor_check_degraded: (status,
    covered_mask) -- bit k + p for the surviving check row parity p owns (ecamd_xor_check_plan_degraded),
    covered_mask the fragments some surviving row contains; missing slots are never read."""
    missing = list(missing)
    if missing:
        covered = C.c_uint32(0)
        status = _status(lambda d: dev().ecamd_xor_check_degraded(
            k, m, hd, ints(missing + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
            lay.nstripes, d, C.byref(covered), _s(stream)), lay, stream, "xor_check_degraded")
        return status, covered.value
    return _status(lambda d: dev().ecamd_xor_check(
        k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes, d,
        _s(stream)), lay, stream, "xor_check")


def _status_suspects(call, lay, stream, what):
    """Run call(d_status, d_suspects) and return both arrays of nstripes words (waits for `stream`)."""
    n = max(lay.nstripes, 1)
    buf = DeviceBuffer(8 * n)
    try:
        check(call(buf.ptr, buf.ptr + 4 * n), what)
        if stream is not None:
            stream.synchronize()
        words = buf.download(8 * n).view(np.uint32)
        return words[:lay.nstripes].copy(), words[n:n + lay.nstripes].copy()
    finally:
        buf.free()


def rs_locate(k, m, lay: Layout, missing=(), stream=None):
    """ecamd_rs_locate: (status, suspects, checked_mask).  status as rs_check; suspects[s] is 0 on a
    consistent stripe, else the mask of fragments that alone explain every disagreement of stripe s:
    one bit -- located; zero -- more than one fragment is bad.  blocksize must be even."""
    checked = C.c_uint32(0)
    status, suspects = _status_suspects(lambda d, u: dev().ecamd_rs_locate(
        k, m, ints(list(missing) + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
        lay.nstripes, d, u, C.byref(checked), _s(stream)), lay, stream, "rs_locate")
    return status, suspects, checked.value


def xor_locate(k, m, hd, lay: Layout, stream=None, missing=()):
    """ecamd_xor_locate: (status, suspects) of full flat_xor_hd stripes.  With a non-empty `missing`,
    ecamd_xor_locate_degraded: (status, suspects, covered_mask); fragments that share a signature come
    back together, several bits in one word."""
    missing = list(missing)
    if missing:
        covered = C.c_uint32(0)
        status, suspects = _status_suspects(lambda d, u: dev().ecamd_xor_locate_degraded(
            k, m, hd, ints(missing + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
            lay.nstripes, d, u, C.byref(covered), _s(stream)), lay, stream, "xor_locate_degraded")
        return status, suspects, covered.value
    return _status_suspects(lambda d, u: dev().ecamd_xor_locate(
        k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes, d, u,
        _s(stream)), lay, stream, "xor_locate")


def rs_scrub(k, m, lay: Layout, stream=None):
    """ecamd_rs_scrub on full stripes (m >= 2): locate, then repair in place every stripe with exactly
    one suspect.  Returns (status, suspects, (n_clean, n_repaired, n_unlocated)); waits for `stream`, so
    the repairs are complete on return."""
    counts = [C.c_int(0), C.c_int(0), C.c_int(0)]
    status, suspects = _status_suspects(lambda d, u: dev().ecamd_rs_scrub(
        k, m, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes, d, u,
        C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2]), _s(stream)), lay, stream, "rs_scrub")
    if stream is None:
        check(dev().ecamd_synchronize(), "synchronize")
    return status, suspects, tuple(c.value for c in counts)


def _status_suspects_pairs(call, lay, stream, what):
    """Run call(d_status, d_suspects, d_pairs) and return the three arrays of nstripes words (waits
    for `stream`)."""
    n = max(lay.nstripes, 1)
    buf = DeviceBuffer(12 * n)
    try:
        check(call(buf.ptr, buf.ptr + 4 * n, buf.ptr + 8 * n), what)
        if stream is not None:
            stream.synchronize()
        words = buf.download(12 * n).view(np.uint32)
        return tuple(words[i * n:i * n + lay.nstripes].copy() for i in range(3))
    finally:
        buf.free()


def rs_locate_pairs(k, m, lay: Layout, missing=(), stream=None):
    """ecamd_rs_locate_pairs: (status, suspects, pairs, checked_mask).  status, suspects and the mask
    as rs_locate; pairs[s] has exactly the two bits {a, b} when stripe s is dirty, has no suspect, at
    least 4 fragments were checked and {a, b} is the one pair of fragments that explains every dirty
    word, else 0."""
    checked = C.c_uint32(0)
    status, suspects, pairs = _status_suspects_pairs(lambda d, u, p: dev().ecamd_rs_locate_pairs(
        k, m, ints(list(missing) + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
        lay.nstripes, d, u, p, C.byref(checked), _s(stream)), lay, stream, "rs_locate_pairs")
    return status, suspects, pairs, checked.value


def rs_scrub_pairs(k, m, lay: Layout, stream=None):
    """ecamd_rs_scrub_pairs on full stripes (m >= 4): locate, then repair in place every stripe with
    exactly one suspect and every stripe with a pair.  Returns (status, suspects, pairs, (n_clean,
    n_repaired, n_repaired_pairs, n_unlocated)); waits for `stream`, so the repairs are complete on
    return."""
    counts = [C.c_int(0) for _ in range(4)]
    status, suspects, pairs = _status_suspects_pairs(lambda d, u, p: dev().ecamd_rs_scrub_pairs(
        k, m, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes, d, u, p,
        *[C.byref(c) for c in counts], _s(stream)), lay, stream, "rs_scrub_pairs")
    if stream is None:
        check(dev().ecamd_synchronize(), "synchronize")
    return status, suspects, pairs, tuple(c.value for c in counts)


def _correct(call, lay, stream, what, pairs):
    """Run call(d_status, d_suspects, d_pairs or None, d_counts), wait for `stream` (or the device) and
    return (status, suspects, pairs or None, counts)."""
    n = max(lay.nstripes, 1)
    buf = DeviceBuffer(12 * n + 16)
    try:
        check(dev().ecamd_memset(buf.ptr, 0, 12 * n + 16), "memset")
        check(call(buf.ptr, buf.ptr + 4 * n, buf.ptr + 8 * n if pairs else None, buf.ptr + 12 * n), what)
        if stream is not None:
            stream.synchronize()
        else:
            check(dev().ecamd_synchronize(), "synchronize")
        words = buf.download(12 * n + 16).view(np.uint32)
        status, suspects, pr = (words[i * n:i * n + lay.nstripes].copy() for i in range(3))
        return status, suspects, pr if pairs else None, tuple(int(c) for c in words[3 * n:3 * n + 4])
    finally:
        buf.free()


def rs_correct(k, m, lay: Layout, missing=(), pairs=True, stream=None):
    """ecamd_rs_correct: locate (with `pairs`, two bad fragments too) and correct the located words in
    place, all on the stream with no host wait inside the call.  Returns (status, suspects, pairs,
    counts): the words as rs_locate_pairs / rs_locate write them (pairs None without `pairs`) and counts
    = (clean, corrected from one suspect, corrected from a pair, dirty and not corrected), after this
    function's own synchronise.  `missing` fragments' slots are neither read nor written."""
    return _correct(lambda d, u, p, c: dev().ecamd_rs_correct(
        k, m, ints(list(missing) + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
        lay.nstripes, d, u, p, c, None, _s(stream)), lay, stream, "rs_correct", pairs)


def xor_correct(k, m, hd, lay: Layout, stream=None, missing=()):
    """ecamd_xor_correct on full flat_xor_hd stripes: (status, suspects, None, counts) as rs_correct.
    With a non-empty `missing`, ecamd_xor_correct_degraded: (status, suspects, None, counts,
    covered_mask); only a stripe with exactly one suspect is written, never a missing slot."""
    missing = list(missing)
    if missing:
        covered = C.c_uint32(0)
        out = _correct(lambda d, u, p, c: dev().ecamd_xor_correct_degraded(
            k, m, hd, ints(missing + [-1]), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
            lay.nstripes, d, u, c, C.byref(covered), _s(stream)), lay, stream, "xor_correct_degraded", False)
        return out + (covered.value,)
    return _correct(lambda d, u, p, c: dev().ecamd_xor_correct(
        k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes, d, u, c,
        _s(stream)), lay, stream, "xor_correct", False)


def _decode_masks(call, lost_masks, lay, stream, what):
    """call(d_lost, d_result, d_counts) on an upload of lost_masks, then a synchronise: (result, counts)."""
    n = max(lay.nstripes, 1)
    masks = np.ascontiguousarray(np.asarray(lost_masks, dtype=np.uint32).reshape(-1))
    if masks.size != lay.nstripes:
        raise ValueError("one mask per stripe: %d masks, %d stripes" % (masks.size, lay.nstripes))
    buf = DeviceBuffer(8 * n + 16)
    try:
        check(dev().ecamd_memset(buf.ptr, 0, 8 * n + 16), "memset")
        if lay.nstripes:
            buf.upload(masks)
        check(call(buf.ptr, buf.ptr + 4 * n, buf.ptr + 8 * n), what)
        if stream is not None:
            stream.synchronize()
        else:
            check(dev().ecamd_synchronize(), "synchronize")
        words = buf.download(8 * n + 16).view(np.uint32)
        return words[n:n + lay.nstripes].copy(), tuple(int(c) for c in words[2 * n:2 * n + 3])
    finally:
        buf.free()


def rs_decode_masks(k, m, lost_masks, lay: Layout, rebuild_parity=True, stream=None):
    """ecamd_rs_decode_masks: rebuild in place the fragments each stripe lost, lost_masks[s] the mask of
    stripe s (bit f: fragment f is lost).  The masks are uploaded to device memory, where the call reads
    them; there is no host wait inside the call.  Returns (result, counts) after this function's own
    synchronise: result[s] = fragments rebuilt, 0 for an empty mask, 0x80000000 | popcount for a mask that
    cannot be recovered (that stripe is not written); counts = (left alone, rebuilt, unrecoverable).
    blocksize must be even, m <= 8."""
    return _decode_masks(lambda lost, res, cnt: dev().ecamd_rs_decode_masks(
        k, m, lost, int(rebuild_parity), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes,
        res, cnt, _s(stream)), lost_masks, lay, stream, "rs_decode_masks")


def xor_decode_masks(k, m, hd, lost_masks, lay: Layout, decode_parity=True, stream=None):
    """ecamd_xor_decode_masks: the same for a flat_xor_hd code.  A mask of hd or more fragments cannot be
    recovered (the reference refuses it); a rebuilt fragment holds what xor_hd_decode leaves when the lost
    slots were zero-filled, as after xor_decode_multi; any blocksize >= 1.  Returns (result, counts) as
    rs_decode_masks."""
    return _decode_masks(lambda lost, res, cnt: dev().ecamd_xor_decode_masks(
        k, m, hd, lost, int(decode_parity), lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes,
        res, cnt, _s(stream)), lost_masks, lay, stream, "xor_decode_masks")


def frame_status_masks(nfrag, d_frag_status, bits, nstripes, d_masks, stream=None):
    """ecamd_frame_status_masks: d_masks[s] (device address) gets bit f when word s*nfrag + f of
    d_frag_status (device address, as ecamd_frame_verify writes it) has any of `bits`.  Asynchronous on
    `stream`: the masks are meant for ecamd_rs_decode_masks (rs_vand) or ecamd_xor_decode_masks
    (flat_xor_hd) on the same stream."""
    check(dev().ecamd_frame_status_masks(nfrag, d_frag_status, bits, nstripes, d_masks, _s(stream)),
          "frame_status_masks")


def xor_scrub(k, m, hd, lay: Layout, stream=None):
    """ecamd_xor_scrub on full flat_xor_hd stripes: locate, then repair in place every stripe with
    exactly one suspect.  Returns (status, suspects, (n_clean, n_repaired, n_unlocated)) as rs_scrub;
    waits for `stream`, so the repairs are complete on return.  flat_xor_hd is not MDS: two bad
    fragments can read as a third, which is then "repaired" (include/ecamd.h)."""
    counts = [C.c_int(0), C.c_int(0), C.c_int(0)]
    status, suspects = _status_suspects(lambda d, u: dev().ecamd_xor_scrub(
        k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize, lay.nstripes, d, u,
        C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2]), _s(stream)), lay, stream, "xor_scrub")
    if stream is None:
        check(dev().ecamd_synchronize(), "synchronize")
    return status, suspects, tuple(c.value for c in counts)


class GF16Map:
    """An arbitrary R x K GF(2^16) fragment map prepared on the device."""

    def __init__(self, coeff):
        coeff = np.asarray(coeff, dtype=np.int64)
        self.R, self.K = coeff.shape
        p = C.c_void_p()
        check(dev().ecamd_map_create(ints(coeff.reshape(-1).tolist()), self.R, self.K, C.byref(p)),
              "map_create")
        self.handle = p.value

    def __del__(self):
        try:
            dev().ecamd_map_destroy(self.handle)
        except Exception:
            pass

    def apply(self, lay: Layout, inputs, outputs, stream=None, out_layout: Layout = None):
        out_layout = out_layout or lay
        check(dev().ecamd_map_apply_strided(
            self.handle, lay.buf.ptr, lay.stripe_stride,
            i64s([i * lay.frag_stride for i in inputs]), out_layout.buf.ptr,
            out_layout.stripe_stride, i64s([o * out_layout.frag_stride for o in outputs]),
            lay.blocksize, lay.nstripes, _s(stream)), "map_apply")


def xor_encode(k, m, hd, lay: Layout, stream=None):
    """flat_xor_hd encode of a strided batch in place (ecamd_xor_encode)."""
    check(dev().ecamd_xor_encode(k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride,
                                 lay.blocksize, lay.nstripes, _s(stream)), "xor_encode")


def xor_decode(k, m, hd, missing, lay: Layout, decode_parity=True, stream=None):
    """xor_hd_decode replayed on every stripe (missing slots read as zero)."""
    check(dev().ecamd_xor_decode(k, m, hd, ints(list(missing) + [-1]), int(decode_parity),
                                 lay.buf.ptr, lay.stripe_stride, lay.frag_stride, lay.blocksize,
                                 lay.nstripes, _s(stream)), "xor_decode")


def xor_reconstruct(k, m, hd, missing, dest, lay: Layout, stream=None):
    """xor_reconstruct_one of fragment `dest` on every stripe."""
    check(dev().ecamd_xor_reconstruct(k, m, hd, ints(list(missing) + [-1]), dest, lay.buf.ptr,
                                      lay.stripe_stride, lay.frag_stride, lay.blocksize,
                                      lay.nstripes, _s(stream)), "xor_reconstruct")


def xor_decode_multi(k, m, hd, missing_per_stripe, lay: Layout, decode_parity=True, stream=None):
    """One erasure list per stripe; stripes with identical lists share a launch."""
    width = k + m + 1
    flat = []
    for pat in missing_per_stripe:
        flat += list(pat)[:width - 1] + [-1] * (width - min(len(pat), width - 1))
    check(dev().ecamd_xor_decode_multi(k, m, hd, ints(flat), width, int(decode_parity), lay.buf.ptr,
                                       lay.stripe_stride, lay.frag_stride, lay.blocksize,
                                       lay.nstripes, _s(stream)), "xor_decode_multi")


def xor_apply(masks, lay: Layout, inputs, outputs, stream=None):
    check(dev().ecamd_xor_apply_strided(
        u32s(masks), len(outputs), len(inputs), lay.buf.ptr, lay.stripe_stride,
        i64s([i * lay.frag_stride for i in inputs]), lay.buf.ptr, lay.stripe_stride,
        i64s([o * lay.frag_stride for o in outputs]), lay.blocksize, lay.nstripes, _s(stream)),
        "xor_apply")


def synchronize():
    check(dev().ecamd_synchronize(), "synchronize")
