"""GPU: the output store policy of the plain one-wave bitsliced kernel (knob bs_store_through; hip/ecamd_device.hip
bs_form, host/bitslice.cpp BitsliceStyle::opts) and its timeline form change how and when a tile is stored,
never what is stored: every operation byte-exact against the CPU oracle with write-through stores off, on and
chosen by shape, the launch counter proving the bitsliced kernel ran, every other fragment untouched.

A launch here has 1 tile (1 stripe x 4 KiB) or 6 (3 stripes x (2 tiles + 48 bytes, the tail on the LDS-table
kernel))."""
import ctypes

import numpy as np
import pytest

import oracle_lib as orc
from ecdata import stripe_fragments
from liberasurecode_amd import _lib
from liberasurecode_amd import device as D

pytestmark = pytest.mark.gpu

K, M = 10, 4
SIZES = {"1x1tile": (4096, 1), "3x2tiles+48": (2 * 4096 + 48, 3)}
SETTINGS = [0, 1, -1]  # bs_store_through: never (the kernel as it was), always, by shape (the default)
OPS = {"encode": None, "decode0123": [0, 1, 2, 3], "decode_0_5_10_13": [0, 5, 10, 13], "reconstruct3": [3]}


def _launches():
    f = _lib.dev().ecamd_bitslice_launches
    f.restype = ctypes.c_longlong
    return f()


_want = {}


def want_of(size, S=None):
    bs, s_default = SIZES[size]
    S = S or s_default
    if (size, S) not in _want:
        w = np.stack([np.concatenate([stripe_fragments(31 + s, K, bs), orc.encode(K, M, stripe_fragments(31 + s, K, bs))])
                      for s in range(S)])
        w.setflags(write=False)
        _want[(size, S)] = w
    return _want[(size, S)]


@pytest.fixture
def knobs():
    d = _lib.dev()
    assert d.ecamd_tune(b"bitslice", 2) == 0  # wait for each compile: every launch takes the bitsliced kernel
    assert d.ecamd_tune(b"small_chunks", 0) == 0  # small batches would otherwise take the small-launch kernel

    def set_through(v):
        assert d.ecamd_tune(b"bs_store_through", v) == 0

    yield set_through
    set_through(-1)
    d.ecamd_tune(b"small_chunks", -1)
    d.ecamd_tune(b"bitslice", 1)


@pytest.mark.parametrize("lost,by_shape", [([1, 6], True), ([7], False)], ids=["2outputs", "1output"])
def test_knob_selects_the_kernel_form(knobs, lost, by_shape):
    """The knob reaches the kernel: the write-through form is a kernel of its own in the process's cache
    (ecamd_bitslice_entries), loaded the first time a setting asks for it -- under the default for the 2-output
    map, which takes it by shape, and only under `always` for the 1-output map, which keeps nt.  (Patterns no
    other test of this module runs, so their entries are new here.)"""
    d = _lib.dev()
    bs, S = SIZES["1x1tile"]
    want = want_of("1x1tile")
    lay = D.Layout.alloc(K + M, bs, S)
    assert d.ecamd_tune(b"bitslice_entries", 4096) == 0  # a full cache would evict one entry per new one
    try:
        grew = {}
        for setting in (0, -1, 1):
            knobs(setting)
            host = want.copy()
            host[:, lost] = 0x5A
            lay.upload_stripes(host)
            e0, n0 = d.ecamd_bitslice_entries(), _launches()
            if len(lost) == 1:
                D.rs_reconstruct(K, M, lost, lost[0], lay)
            else:
                D.rs_decode(K, M, lost, lay)
            assert (lay.download_stripes() == want).all(), setting
            assert _launches() > n0, setting
            grew[setting] = d.ecamd_bitslice_entries() - e0
        assert grew == ({0: 1, -1: 1, 1: 0} if by_shape else {0: 1, -1: 0, 1: 1}), grew
    finally:
        d.ecamd_tune(b"bitslice_entries", 0)
        lay.buf.free()


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("op", sorted(OPS))
def test_operation_exact_under_every_setting(knobs, op, size):
    bs, S = SIZES[size]
    want = want_of(size)
    lost = OPS[op]
    lay = D.Layout.alloc(K + M, bs, S)
    try:
        for setting in SETTINGS:
            knobs(setting)
            host = want.copy()
            if lost is None:
                host[:, K:] = 0xA5
            else:
                host[:, lost] = 0x5A
            lay.upload_stripes(host)
            n0 = _launches()
            if lost is None:
                D.rs_encode(K, M, lay)
            elif op.startswith("reconstruct"):
                D.rs_reconstruct(K, M, lost, lost[0], lay)
            else:
                D.rs_decode(K, M, lost, lay)
            got = lay.download_stripes()
            assert _launches() > n0, setting
            assert (got == want).all(), (setting, np.argwhere(got != want)[:4])  # outputs exact, the rest untouched
    finally:
        lay.buf.free()


def test_timeline_form_same_bytes_and_one_record_per_tile(knobs):
    """The measurement form (ecamd_bitslice_timeline): the encode's bytes as ever, and tile t's record at
    32 t -- its own number, an end no earlier than its start, an XCC id below 8 -- with nothing written
    past the records the caller allowed."""
    d = _lib.dev()
    size = "3x2tiles+48"
    bs, S = SIZES[size]
    want = want_of(size)
    ntiles = S * 2
    lay = D.Layout.alloc(K + M, bs, S)
    buf = D.DeviceBuffer((ntiles + 1) * 32)
    try:
        for allowed in (ntiles, ntiles - 1):
            buf.upload(np.full((ntiles + 1) * 32, 0xEE, np.uint8))
            host = want.copy()
            host[:, K:] = 0xA5
            lay.upload_stripes(host)
            assert d.ecamd_bitslice_timeline(buf.ptr, allowed) == 0
            n0 = _launches()
            D.rs_encode(K, M, lay)
            got = lay.download_stripes()
            assert d.ecamd_bitslice_timeline(None, 0) == 0
            assert _launches() > n0
            assert (got == want).all()
            rec = buf.download().view(np.uint32).reshape(ntiles + 1, 8)
            assert (rec[allowed:] == 0xEEEEEEEE).all()
            r = rec[:allowed].astype(np.int64)
            start, end = r[:, 0] | (r[:, 1] << 32), r[:, 2] | (r[:, 3] << 32)
            assert (r[:, 4] == np.arange(allowed)).all() and (end >= start).all() and ((r[:, 5] & 15) < 8).all()
            assert (end - start < 100_000).all()  # a tile lives microseconds; the clock ticks at 100 MHz
    finally:
        d.ecamd_bitslice_timeline(None, 0)
        buf.free()
        lay.buf.free()


def test_decode_multi_stripe_lists_exact_under_every_setting(knobs):
    """One ecamd_rs_decode_multi call: two patterns, so each launch takes its 3 stripes from a stripe list."""
    size, S = "3x2tiles+48", 6
    bs = SIZES[size][0]
    want = want_of(size, S)
    per = [[0, 1, 2, 3] if s % 2 == 0 else [0, 5, 10, 13] for s in range(S)]
    lay = D.Layout.alloc(K + M, bs, S)
    try:
        for setting in SETTINGS:
            knobs(setting)
            host = want.copy()
            for s, p in enumerate(per):
                host[s, p] = 0xC3
            lay.upload_stripes(host)
            n0 = _launches()
            D.rs_decode_multi(K, M, per, lay)
            got = lay.download_stripes()
            assert _launches() - n0 >= 2, setting
            assert (got == want).all(), (setting, np.argwhere(got != want)[:4])
    finally:
        lay.buf.free()
