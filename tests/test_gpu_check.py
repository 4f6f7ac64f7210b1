"""GPU: the on-device stripe consistency check (ecamd_rs_check / ecamd_xor_check, include/ecamd.h).

Expected statuses never come from the code under test: stripes are built with the reference encode
(oracle_lib / xor_oracle), and for a pattern with missing fragments bit f is expected iff the stored
fragment f differs anywhere from the reference's reconstruct of f.  Missing slots hold 0x5A.  The
fused-launch counter pins which path ran: the check form of the bitsliced kernel for whole tiles of
(10,4) and (20,8), the generic compute-and-compare path for (4,2), tails, knob bitslice 0 and flat XOR."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
import xor_util as X
from ecdata import stripe_fragments

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import xor_oracle as XO  # noqa: E402

S = 3
FILL = 0x5A
TAIL = 48
EINVAL = -22
CANARY = 0xA5


def tile_of(rows):
    return 4096 if rows <= 4 else 16384


@pytest.fixture(scope="module")
def D():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from liberasurecode_amd import device
    return device


@pytest.fixture()
def dev(D):
    """libecamd with knob bitslice 2 (wait for compiles); the default comes back afterwards."""
    from liberasurecode_amd import _lib
    d = _lib.dev()
    d.ecamd_tune(b"bitslice", 2)
    yield d
    d.ecamd_tune(b"bitslice", 1)
    d.ecamd_tune(b"bs_tiles_per_slot", -1)


_stripes = {}


def stripes(k, m, bs):
    """(S, k+m, bs) reference-encoded stripes, computed once per shape and never modified."""
    key = (k, m, bs)
    if key not in _stripes:
        full = np.empty((S, k + m, bs), np.uint8)
        for s in range(S):
            full[s, :k] = stripe_fragments(300 + 7 * k + s, k, bs)
            full[s, k:] = orc.encode(k, m, full[s, :k])
        full.setflags(write=False)
        _stripes[key] = full
    return _stripes[key]


def oracle_status(k, m, held, missing):
    """Per stripe: bit f for every checked fragment f (available, not among the first k available)
    whose stored bytes differ from the reference's reconstruct of f; and the checked mask."""
    avail = [f for f in range(k + m) if f not in missing]
    checked = avail[k:]
    out = np.zeros(held.shape[0], np.uint32)
    for s in range(held.shape[0]):
        for f in checked:
            frags = [np.array(x) for x in held[s]]
            assert orc.reconstruct(k, m, frags, list(missing), f) == 0
            if (frags[f] != held[s, f]).any():
                out[s] |= np.uint32(1 << f)
    return out, sum(1 << f for f in checked)


def held_of(full, missing):
    held = np.array(full)
    if missing:
        held[:, list(missing)] = FILL
    return held


def run_check(D, k, m, held, missing=()):
    lay = D.Layout.alloc(k + m, held.shape[2], held.shape[0])
    try:
        lay.upload_stripes(held)
        return D.rs_check(k, m, lay, missing)
    finally:
        lay.buf.free()


def raw_check(dev, D, k, m, missing, base, stripe_stride, frag_stride, bs, nstripes):
    """ecamd_rs_check on explicit pointers: (rc, status words as left in a canary-filled buffer, checked)."""
    from liberasurecode_amd import _lib
    st = D.DeviceBuffer(4 * max(nstripes, 1))
    dev.ecamd_memset(st.ptr, CANARY, st.nbytes)
    checked = C.c_uint32(0xFFFFFFFF)
    rc = dev.ecamd_rs_check(k, m, _lib.ints(list(missing) + [-1]), base, stripe_stride, frag_stride, bs, nstripes,
                            st.ptr, C.byref(checked), None)
    dev.ecamd_synchronize()
    words = st.download().view(np.uint32).copy()
    st.free()
    return rc, words, checked.value


@pytest.mark.parametrize("k,m,fused", [(10, 4, True), (20, 8, True), (4, 2, False)])
def test_clean_stripes_and_which_path(D, dev, k, m, fused):
    bs = 2 * tile_of(m) + TAIL
    n0 = dev.ecamd_check_fused_launches()
    status, checked = run_check(D, k, m, np.array(stripes(k, m, bs)))
    assert checked == sum(1 << f for f in range(k, k + m))
    assert status.dtype == np.uint32 and status.shape == (S,) and not status.any()
    assert (dev.ecamd_check_fused_launches() > n0) == fused


def flips(k, m, bs):
    t = tile_of(m)
    pos = [0, 2 * t - 1, 2 * t + 20]  # first byte of tile 0, last byte of tile 1, in the 48-byte tail
    out = [(f, p) for p in pos for f in (3, k + m - 1)]
    if m > 4:
        out.append((k + 5, t + 1000))  # a row of the second 4-row half
    return out


@pytest.mark.parametrize("k,m", [(10, 4), (20, 8), (4, 2)])
def test_one_bit_flips_match_the_oracle(D, dev, k, m):
    bs = 2 * tile_of(m) + TAIL
    full = stripes(k, m, bs)
    for f, p in flips(k, m, bs):
        held = np.array(full)
        held[1, f, p] ^= 0x04
        want, _ = oracle_status(k, m, held, [])
        assert want[1] and not want[0] and not want[2]
        got, _ = run_check(D, k, m, held)
        assert (got == want).all(), (f, p, [hex(x) for x in got], [hex(x) for x in want])


# rs_vand (8, 12): R = 12 checked fragments in two row groups.  At this size group 0 (8 rows, 16 KiB
# tiles) covers 16384 bytes and group 1 (4 rows, one-wave 4 KiB tiles) 20480; the generic stage redoes
# everything past the SMALLER cover for all rows, so bytes [16384, 20480) of group 1's rows are seen
# by both stages.  (fragment, byte) of the flip in stripe 1: none, an input, a row of each group, one
# where the stages overlap, one in the 48-byte tail.
WIDE = (8, 12, 16384 + 4096 + TAIL)
WIDE_FLIPS = [None, (3, 5000), (9, 100), (17, 16384 + 1000), (12, 16384 + 4096 + 20)]


def test_twelve_checked_fragments_in_two_row_groups(D, dev):
    """Judged by the statuses alone: a group whose network is declined goes the generic way, which
    must be just as right."""
    k, m, bs = WIDE
    full = stripes(k, m, bs)
    n0 = dev.ecamd_check_fused_launches()
    for flip in WIDE_FLIPS:
        held = np.array(full)
        if flip:
            held[1, flip[0], flip[1]] ^= 0x04
        want, mask = oracle_status(k, m, held, [])
        assert mask == 0xFFF << k and not want[0] and not want[2]
        assert want[1] == (0 if not flip else mask if flip[0] < k else 1 << flip[0])
        got, checked = run_check(D, k, m, held)
        assert checked == mask
        assert (got == want).all(), (flip, [hex(x) for x in got], [hex(x) for x in want])
    print("ecamd_check_fused_launches rose by", dev.ecamd_check_fused_launches() - n0, "over", len(WIDE_FLIPS), "checks")


@pytest.mark.parametrize("missing", [[2, 7], [0]])
def test_missing_fragments(D, dev, missing):
    k, m = 10, 4
    bs = 2 * 4096 + TAIL
    full = stripes(k, m, bs)
    avail = [f for f in range(k + m) if f not in missing]
    n0 = dev.ecamd_check_fused_launches()
    held = held_of(full, missing)
    want, mask = oracle_status(k, m, held, missing)
    got, checked = run_check(D, k, m, held, missing)
    assert checked == mask == sum(1 << f for f in avail[k:])
    assert not want.any() and (got == want).all()
    assert dev.ecamd_check_fused_launches() > n0  # [2, 7]: compiled at run time (knob 2 waits)
    # an input, a checked fragment, and a missing slot (which may hold anything: nothing shows)
    for f, p, silent in ((avail[4], 4096 + 5, False), (avail[k], 77, False), (missing[0], 4095, True)):
        held = held_of(full, missing)
        held[1, f, p] ^= 0x80
        want, _ = oracle_status(k, m, held, missing)
        assert bool(want.any()) != silent
        got, _ = run_check(D, k, m, held, missing)
        assert (got == want).all(), (missing, f, [hex(x) for x in got], [hex(x) for x in want])
        assert not (got & sum(1 << i for i in list(missing) + avail[:k])).any()


def test_exactly_m_missing_checks_nothing(D, dev):
    k, m = 10, 4
    held = held_of(stripes(k, m, 4096 + TAIL), [1, 4, 11, 13])
    held[2, 0, 9] ^= 1
    got, checked = run_check(D, k, m, held, [1, 4, 11, 13])
    assert checked == 0 and not got.any()


def padded(D, held, pad, seed):
    """The stripes in a layout whose fragment slots are `pad` bytes longer than round_up(bs, 16),
    every byte outside the fragments' own blocksize bytes random."""
    nS, n, bs = held.shape
    fs = (bs + 15) // 16 * 16 + pad
    host = np.random.default_rng(seed).integers(0, 256, size=(nS, n, fs), dtype=np.uint8)
    host[:, :, :bs] = held
    buf = D.DeviceBuffer(host.nbytes)
    buf.upload(host)
    return D.Layout(buf, n, bs, nS, fs, fs * n)


@pytest.mark.parametrize("bs", [1, 15, 100, 4095, 4096 + 7, 8192 + 48])
def test_generic_path_alone(D, dev, bs):
    k, m = 10, 4
    full = stripes(k, m, bs)
    dev.ecamd_tune(b"bitslice", 0)
    n0 = dev.ecamd_check_fused_launches()
    results = []
    for f in (None, 3, k + m - 1):  # clean; a flip in the LAST byte of a data / the last parity fragment
        held = np.array(full)
        if f is not None:
            held[1, f, bs - 1] ^= 0x01
        want, _ = oracle_status(k, m, held, [])
        assert bool(want.any()) == (f is not None)
        lay = padded(D, held, 16, 5 + bs)  # garbage between blocksize and frag_stride never flags
        got, _ = D.rs_check(k, m, lay)
        lay.buf.free()
        assert (got == want).all(), (bs, f, [hex(x) for x in got], [hex(x) for x in want])
        results.append((held, got))
    assert dev.ecamd_check_fused_launches() == n0
    if bs == 8192 + 48:  # byte-identical to the fused run
        dev.ecamd_tune(b"bitslice", 2)
        for held, got in results:
            fused, _ = run_check(D, k, m, held)
            assert fused.tobytes() == got.tobytes()
        assert dev.ecamd_check_fused_launches() > n0


def test_split_launch_advances_the_status_words(D, dev):
    """bs_tiles_per_slot 1 splits a long pass into several launches, each over its own stripe range:
    the status words must follow the stripes."""
    import torch
    k, m, bs = 10, 4, 4096
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nS = 16 * cus + 37  # one launch takes 16 one-wave tiles per CU (4 waves per SIMD x 4 SIMDs)
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.fill_splitmix(nfrags=k, stripe0=1)
        D.rs_encode(k, m, lay)
        at = (nS - 1) * lay.stripe_stride + (k + 2) * lay.frag_stride + 1234
        byte = lay.buf.download(1, at)
        byte[0] ^= 0x20
        lay.buf.upload(byte, at)
        dev.ecamd_tune(b"bs_tiles_per_slot", 1)
        n0 = dev.ecamd_check_fused_launches()
        got, _ = D.rs_check(k, m, lay)
        assert dev.ecamd_check_fused_launches() - n0 >= 2
        assert got[nS - 1] == 1 << 12 and not got[:nS - 1].any(), np.nonzero(got)[0][:8]
    finally:
        lay.buf.free()


def test_fragment_major_strides(D, dev):
    k, m = 10, 4
    bs = 2 * 4096 + TAIL
    F = (bs + 15) // 16 * 16
    held = np.array(stripes(k, m, bs))
    held[1, k + 1, 4097] ^= 0x40
    held[2, 6, 8200] ^= 0x02
    want, _ = oracle_status(k, m, held, [])
    host = np.zeros((k + m, S, F), np.uint8)  # [k+m][S][F]
    host[:, :, :bs] = held.transpose(1, 0, 2)
    buf = D.DeviceBuffer(host.nbytes)
    buf.upload(host)
    n0 = dev.ecamd_check_fused_launches()
    got, _ = D.rs_check(k, m, D.Layout(buf, k + m, bs, S, frag_stride=S * F, stripe_stride=F))
    buf.free()
    assert dev.ecamd_check_fused_launches() > n0
    assert (got == want).all() and want[1] == 1 << (k + 1) and want[2] == 0xF << k


def test_framed_fragments_at_payload_offset(D, dev):
    from liberasurecode_amd import _lib, frame
    k, m = 10, 4
    size = k * (8192 + 64) - 6
    fb = frame.FrameBatch(frame.RS_VAND, k, m, size, S)
    obj = D.DeviceBuffer(fb.obj_stride * S)
    _lib.check(dev.ecamd_fill_splitmix(obj.ptr, fb.obj_stride, 0, 1, size, S, 0, 0x99, None), "fill")
    fb.encode(obj)
    args = (fb.base + frame.HEADER, fb.stripe_stride, fb.frag_stride, fb.blocksize, S)
    rc, got, checked = raw_check(dev, D, k, m, [], *args)
    assert rc == 0 and checked == 0xF << k and not got.any()
    frags = fb.fragments()
    frags[2, 4, frame.HEADER + 5000] ^= 0x08  # a payload byte of data fragment 4, stripe 2
    fb.upload_fragments(frags)
    want, _ = oracle_status(k, m, np.ascontiguousarray(frags[:, :, frame.HEADER:frame.HEADER + fb.blocksize]), [])
    rc, got, _ = raw_check(dev, D, k, m, [], *args)
    assert rc == 0 and want[2] and (got == want).all()
    obj.free()
    fb.buf.free()


@pytest.mark.parametrize("k,m,hd", [(10, 6, 4), (3, 3, 3)])
def test_flat_xor(D, dev, k, m, hd):
    bs = 4096 + 10
    pb, _ = X.tables(k, m, hd)
    full = np.empty((S, k + m, bs), np.uint8)
    for s in range(S):
        full[s, :k] = stripe_fragments(900 + s, k, bs)
        full[s, k:] = XO.encode_bytes(k, m, hd, full[s, :k])

    def run(held):
        lay = padded(D, held, 16, 77)
        try:
            return D.xor_check(k, m, hd, lay)
        finally:
            lay.buf.free()

    n0 = dev.ecamd_check_fused_launches()
    assert not run(full).any()
    for d in (0, k - 1):  # a data flip: exactly the parities whose bitmap contains d
        held = full.copy()
        held[1, d, bs - 1] ^= 0x10
        want = sum(1 << (k + p) for p in range(m) if pb[p] >> d & 1)
        assert want
        got = run(held)
        assert got[1] == want and not got[0] and not got[2], (d, hex(got[1]), hex(want))
    for p in (0, m - 1):  # a parity flip: that parity alone
        held = full.copy()
        held[2, k + p, 0] ^= 0x01
        got = run(held)
        assert got[2] == 1 << (k + p) and not got[0] and not got[1]
    assert dev.ecamd_check_fused_launches() == n0


def test_errors_leave_the_status_untouched(D, dev):
    lay = D.Layout.alloc(34, 4096, S)
    try:
        canary = np.full(S, CANARY * 0x01010101, np.uint32)
        rc, got, _ = raw_check(dev, D, 30, 4, [], lay.buf.ptr, lay.stripe_stride, lay.frag_stride, 4096, S)
        assert rc == EINVAL and (got == canary).all()
        rc, got, _ = raw_check(dev, D, 10, 4, [0, 1, 2, 3, 4], lay.buf.ptr, lay.stripe_stride, lay.frag_stride, 4096, S)
        assert rc == EINVAL and (got == canary).all()
        st = D.DeviceBuffer(4 * S)
        dev.ecamd_memset(st.ptr, CANARY, st.nbytes)
        assert dev.ecamd_xor_check(10, 4, 9, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, 4096, S, st.ptr,
                                   None) == EINVAL
        assert (st.download().view(np.uint32) == canary).all()
        st.free()
    finally:
        lay.buf.free()


def test_check_maps_count_in_the_map_cache(D, dev):
    k, m = 10, 4
    entries = [C.c_int64(), C.c_int64()]
    held = held_of(stripes(k, m, 4096 + TAIL), [9])
    for e in entries:  # the first check of a pattern adds its map, the second finds it
        run_check(D, k, m, held, [9])
        assert dev.ecamd_map_cache_stats(C.byref(e), None, None) == 0
    run_check(D, k, m, held_of(stripes(k, m, 4096 + TAIL), [9, 11]), [9, 11])
    after = C.c_int64()
    assert dev.ecamd_map_cache_stats(C.byref(after), None, None) == 0
    assert entries[0].value == entries[1].value and after.value == entries[1].value + 1


def test_fresh_process_runs_shipped_check_kernels_at_first_call(tmp_path):
    """Empty $ECAMD_JIT_CACHE, default knob (bitslice 1: never waits for a compile): the first check of
    (10,4), full stripe and with fragment 5 missing, runs fused -- its code object came from lib/jit/."""
    cache = tmp_path / "jitcache"
    cache.mkdir(mode=0o700)
    env = dict(os.environ, ECAMD_JIT_CACHE=str(cache))
    r = subprocess.run([sys.executable, os.path.join(HERE, "check_shipped_run.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for name in ("full", "lost5"):
        assert out[name + "_fused_launches"] > 0, out
        assert out[name + "_clean"] and out[name + "_flagged"], out
    assert out["cache_objects"] == 0, out
