"""GPU: locate and scrub (ecamd_rs_locate / ecamd_xor_locate / ecamd_rs_scrub, include/ecamd.h).

Expected values never come from the code under test.  Stripes are built with the reference encode
(oracle_lib / xor_oracle); statuses follow test_gpu_check.oracle_status; fragment f is an expected
suspect of a dirty stripe iff replacing the stored f by the reference's reconstruct of f (f added to
the missing list) makes the oracle status of the stripe zero.  The fused-launch counter pins which
path ran: the locate form of the bitsliced kernel for whole tiles of (10,4) and (20,8), the generic
compute-and-compare path for (4,2), tails, knob bitslice 0 and flat XOR."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
import test_gpu_check as TC
import xor_util as X
from ecdata import stripe_fragments
from test_gpu_check import D, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
XO = TC.XO
S = TC.S
TAIL = TC.TAIL
EINVAL = -22
CANARY = 0xA5
CANARY32 = CANARY * 0x01010101


def oracle_locate(k, m, held, missing):
    """(status, suspects) per stripe from the reference codec alone."""
    missing = list(missing)
    avail = [f for f in range(k + m) if f not in missing]
    status, _ = TC.oracle_status(k, m, held, missing)
    suspects = np.zeros(held.shape[0], np.uint32)
    for s in np.nonzero(status)[0]:
        for f in avail:
            frags = [np.array(x) for x in held[s]]
            assert orc.reconstruct(k, m, frags, sorted(missing + [f]), f) == 0
            trial = np.array(held[s:s + 1])
            trial[0, f] = frags[f]
            if not TC.oracle_status(k, m, trial, missing)[0][0]:
                suspects[s] |= np.uint32(1 << f)
    return status, suspects


def run_locate(D, k, m, held, missing=()):
    lay = D.Layout.alloc(k + m, held.shape[2], held.shape[0])
    try:
        lay.upload_stripes(held)
        return D.rs_locate(k, m, lay, missing)
    finally:
        lay.buf.free()


def raw_locate(dev, D, k, m, missing, base, stripe_stride, frag_stride, bs, nstripes, extra=2):
    """ecamd_rs_locate on explicit pointers into canary-filled arrays of nstripes + extra words:
    (rc, status, suspects, checked), the arrays whole."""
    from liberasurecode_amd import _lib
    n = nstripes + extra
    st, su = D.DeviceBuffer(4 * n), D.DeviceBuffer(4 * n)
    dev.ecamd_memset(st.ptr, CANARY, st.nbytes)
    dev.ecamd_memset(su.ptr, CANARY, su.nbytes)
    checked = C.c_uint32(0xFFFFFFFF)
    rc = dev.ecamd_rs_locate(k, m, _lib.ints(list(missing) + [-1]), base, stripe_stride, frag_stride, bs, nstripes,
                             st.ptr, su.ptr, C.byref(checked), None)
    dev.ecamd_synchronize()
    a, b = st.download().view(np.uint32).copy(), su.download().view(np.uint32).copy()
    st.free()
    su.free()
    return rc, a, b, checked.value


def hexes(x):
    return [hex(int(v)) for v in x]


@pytest.mark.parametrize("k,m,fused", [(10, 4, True), (20, 8, True), (4, 2, False)])
def test_clean_stripes_and_which_path(D, dev, k, m, fused):
    bs = 2 * TC.tile_of(m) + TAIL
    held = np.array(TC.stripes(k, m, bs))
    n0 = dev.ecamd_locate_fused_launches()
    status, suspects, checked = run_locate(D, k, m, held)
    assert checked == sum(1 << f for f in range(k, k + m))
    assert status.shape == suspects.shape == (S,) and not status.any() and not suspects.any()
    assert (dev.ecamd_locate_fused_launches() > n0) == fused
    # only nstripes words of each array are written
    lay = D.Layout.alloc(k + m, bs, S)
    lay.upload_stripes(held)
    rc, st, su, _ = raw_locate(dev, D, k, m, [], lay.buf.ptr, lay.stripe_stride, lay.frag_stride, bs, S)
    lay.buf.free()
    assert rc == 0 and not st[:S].any() and not su[:S].any()
    assert (st[S:] == CANARY32).all() and (su[S:] == CANARY32).all()


@pytest.mark.parametrize("k,m", [(10, 4), (20, 8), (4, 2)])
def test_one_flip_is_located(D, dev, k, m):
    bs = 2 * TC.tile_of(m) + TAIL
    full = TC.stripes(k, m, bs)
    for f, p in TC.flips(k, m, bs):
        held = np.array(full)
        held[1, f, p] ^= 0x04
        want_st, want_su = oracle_locate(k, m, held, [])
        assert want_su[1] == 1 << f and not want_su[0] and not want_su[2]
        st, su, _ = run_locate(D, k, m, held)
        assert (st == want_st).all(), (f, p, hexes(st), hexes(want_st))
        assert (su == want_su).all(), (f, p, hexes(su), hexes(want_su))


@pytest.mark.parametrize("k,m", [(10, 4), (20, 8)])
def test_two_flips_in_one_fragment_and_in_two(D, dev, k, m):
    t = TC.tile_of(m)
    bs = 2 * t + TAIL
    full = TC.stripes(k, m, bs)
    # the same fragment in different tiles: still that fragment
    for f in (2, k + 1):
        held = np.array(full)
        held[1, f, 10] ^= 0x01
        held[1, f, t + 11] ^= 0x80
        st, su, _ = run_locate(D, k, m, held)
        assert su[1] == 1 << f and not su[0] and not su[2], (f, hexes(su))
    # two different fragments: different tiles (fails if waves OR where they must AND), the same
    # word, and a whole tile against the tail (where the fused and the generic path meet in one word)
    for (f1, p1), (f2, p2) in ((((2, 10)), (5, t + 10)), ((2, 10), (k + 1, t + 300)), ((3, 2000), (7, 2000)),
                               ((3, 2001), (k, 2000)), ((4, 100), (6, 2 * t + 20)), ((k + 2, t + 1), (1, 2 * t + 3))):
        held = np.array(full)
        held[1, f1, p1] ^= 0x10
        held[1, f2, p2] ^= 0x02
        want_st, want_su = oracle_locate(k, m, held, [])
        assert not want_su.any()  # m >= 3 checked fragments: two bad fragments leave no candidate
        st, su, _ = run_locate(D, k, m, held)
        assert (st == want_st).all() and st[1] and not su.any(), ((f1, p1), (f2, p2), hexes(st), hexes(su))


def test_twelve_checked_fragments_take_the_generic_path_alone(D, dev):
    """rs_vand (8, 12), R = 12: the fused locate needs every row's syndrome in one wave, so more than
    8 rows go through the compare kernel alone (the cases of test_gpu_check.WIDE_FLIPS)."""
    k, m, bs = TC.WIDE
    full = TC.stripes(k, m, bs)
    n0 = dev.ecamd_locate_fused_launches()
    for flip in TC.WIDE_FLIPS:
        held = np.array(full)
        if flip:
            held[1, flip[0], flip[1]] ^= 0x04
        want_st, want_su = oracle_locate(k, m, held, [])
        assert want_su[1] == (1 << flip[0] if flip else 0) and not want_su[0] and not want_su[2]
        st, su, checked = run_locate(D, k, m, held)
        assert checked == 0xFFF << k
        assert (st == want_st).all(), (flip, hexes(st), hexes(want_st))
        assert (su == want_su).all(), (flip, hexes(su), hexes(want_su))
    assert dev.ecamd_locate_fused_launches() == n0


@pytest.mark.parametrize("missing", [[0], [2, 7]])
def test_missing_fragments(D, dev, missing):
    k, m = 10, 4
    bs = 2 * 4096 + TAIL
    full = TC.stripes(k, m, bs)
    avail = [f for f in range(k + m) if f not in missing]
    n0 = dev.ecamd_locate_fused_launches()
    st, su, checked = run_locate(D, k, m, TC.held_of(full, missing), missing)
    assert checked == sum(1 << f for f in avail[k:]) and not st.any() and not su.any()
    assert dev.ecamd_locate_fused_launches() > n0
    never = sum(1 << f for f in missing) | (0xFFFFFFFF & ~((1 << (k + m)) - 1))
    for f, p, silent in ((avail[4], 4096 + 5, False), (avail[k], 77, False), (avail[k + 1], 8192 + 9, False),
                         (missing[0], 4095, True)):
        held = TC.held_of(full, missing)
        held[1, f, p] ^= 0x80
        want_st, want_su = oracle_locate(k, m, held, missing)
        assert bool(want_st.any()) != silent
        if not silent:
            assert want_su[1] == 1 << f
        st, su, _ = run_locate(D, k, m, held, missing)
        assert (st == want_st).all() and (su == want_su).all(), (missing, f, hexes(st), hexes(su), hexes(want_su))
        assert not (su & never).any()


def test_one_checked_fragment_suspects_every_participant_and_none_checked_nothing(D, dev):
    k, m = 10, 4
    bs = 4096 + TAIL
    missing = [1, 4, 11]  # R = 1
    avail = [f for f in range(k + m) if f not in missing]
    for f, p in ((0, 9), (13, 4096 + 3)):
        held = TC.held_of(TC.stripes(k, m, bs), missing)
        held[2, f, p] ^= 1
        want_st, want_su = oracle_locate(k, m, held, missing)
        assert want_su[2] == sum(1 << a for a in avail)
        st, su, checked = run_locate(D, k, m, held, missing)
        assert checked == 1 << 13 and (st == want_st).all() and (su == want_su).all(), (hexes(st), hexes(su))
    missing = [1, 4, 11, 13]  # R = 0
    held = TC.held_of(TC.stripes(k, m, bs), missing)
    held[2, 0, 9] ^= 1
    st, su, checked = run_locate(D, k, m, held, missing)
    assert checked == 0 and not st.any() and not su.any()


@pytest.mark.parametrize("bs", [2, 16, 100, 4096 + 6, 8192 + 48])
def test_generic_path_alone(D, dev, bs):
    k, m = 10, 4
    full = TC.stripes(k, m, bs)
    dev.ecamd_tune(b"bitslice", 0)
    n0 = dev.ecamd_locate_fused_launches()
    results = []
    cases = [(), ((3, bs - 1),), ((k + m - 1, bs - 1),), ((k, 0),), ((3, 0), (3, bs - 1)), ((3, bs - 1), (6, bs - 2)),
             ((4, 1), (k + 1, bs - 1))]
    for case in cases:
        held = np.array(full)
        for f, p in case:
            held[1, f, p] ^= 0x21
        want_st, want_su = oracle_locate(k, m, held, [])
        lay = TC.padded(D, held, 16, 5 + bs)  # garbage between blocksize and frag_stride changes nothing
        st, su, _ = D.rs_locate(k, m, lay)
        lay.buf.free()
        assert (st == want_st).all() and (su == want_su).all(), (bs, case, hexes(st), hexes(su), hexes(want_su))
        results.append((held, st, su))
    assert dev.ecamd_locate_fused_launches() == n0
    if bs == 8192 + 48:  # byte-identical to the fused run
        dev.ecamd_tune(b"bitslice", 2)
        for held, st, su in results:
            fst, fsu, _ = run_locate(D, k, m, held)
            assert fst.tobytes() == st.tobytes() and fsu.tobytes() == su.tobytes()
        assert dev.ecamd_locate_fused_launches() > n0


def test_generic_path_of_20_8_and_4_2_pairs(D, dev):
    """(20,8) through the compare kernel alone, and (4,2) -- R = 2, which locates one bad fragment."""
    dev.ecamd_tune(b"bitslice", 0)
    for k, m, bs in ((20, 8, 512 + 6), (4, 2, 4096 + 6)):
        full = TC.stripes(k, m, bs)
        for f, p in ((0, 0), (k - 1, bs - 1), (k, 100), (k + m - 1, bs - 2)):
            held = np.array(full)
            held[1, f, p] ^= 0x40
            want_st, want_su = oracle_locate(k, m, held, [])
            assert want_su[1] == 1 << f
            st, su, _ = run_locate(D, k, m, held)
            assert (st == want_st).all() and (su == want_su).all(), (k, m, f, hexes(st), hexes(su))


def test_errors_leave_both_arrays_untouched(D, dev):
    lay = D.Layout.alloc(34, 4096, S)
    try:
        args = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride)
        for k, m, missing, bs in ((10, 4, [], 4095), (10, 4, [], 1), (30, 4, [], 4096), (10, 4, [0, 1, 2, 3, 4], 4096)):
            rc, st, su, _ = raw_locate(dev, D, k, m, missing, *args, bs, S)
            assert rc == EINVAL, (k, m, missing, bs)
            assert (st == CANARY32).all() and (su == CANARY32).all()
        st, su = D.DeviceBuffer(4 * S), D.DeviceBuffer(4 * S)
        for hd, bs in ((9, 4096), (4, 4095)):
            dev.ecamd_memset(st.ptr, CANARY, st.nbytes)
            dev.ecamd_memset(su.ptr, CANARY, su.nbytes)
            assert dev.ecamd_xor_locate(10, 6, hd, *args, bs, S, st.ptr, su.ptr, None) == EINVAL
            assert (st.download().view(np.uint32) == CANARY32).all() and (su.download().view(np.uint32) == CANARY32).all()
        counts = [C.c_int(-3) for _ in range(3)]
        assert dev.ecamd_rs_scrub(10, 1, *args, 4096, S, st.ptr, su.ptr, *[C.byref(c) for c in counts], None) == EINVAL
        assert (st.download().view(np.uint32) == CANARY32).all() and (su.download().view(np.uint32) == CANARY32).all()
        st.free()
        su.free()
    finally:
        lay.buf.free()


def test_split_launch_advances_both_arrays(D, dev):
    import torch
    k, m, bs = 10, 4, 4096
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nS = 16 * cus + 37
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.fill_splitmix(nfrags=k, stripe0=1)
        D.rs_encode(k, m, lay)
        at = (nS - 1) * lay.stripe_stride + 6 * lay.frag_stride + 1234
        byte = lay.buf.download(1, at)
        byte[0] ^= 0x20
        lay.buf.upload(byte, at)
        dev.ecamd_tune(b"bs_tiles_per_slot", 1)
        n0 = dev.ecamd_locate_fused_launches()
        st, su, _ = D.rs_locate(k, m, lay)
        assert dev.ecamd_locate_fused_launches() - n0 >= 2
        assert st[nS - 1] == 0xF << k and not st[:nS - 1].any(), np.nonzero(st)[0][:8]
        assert su[nS - 1] == 1 << 6 and not su[:nS - 1].any(), np.nonzero(su)[0][:8]
    finally:
        lay.buf.free()


def test_fragment_major_strides(D, dev):
    k, m = 10, 4
    bs = 2 * 4096 + TAIL
    F = (bs + 15) // 16 * 16
    held = np.array(TC.stripes(k, m, bs))
    held[1, k + 1, 4097] ^= 0x40
    held[2, 6, 8200] ^= 0x02
    want_st, want_su = oracle_locate(k, m, held, [])
    host = np.zeros((k + m, S, F), np.uint8)  # [k+m][S][F]
    host[:, :, :bs] = held.transpose(1, 0, 2)
    buf = D.DeviceBuffer(host.nbytes)
    buf.upload(host)
    n0 = dev.ecamd_locate_fused_launches()
    st, su, _ = D.rs_locate(k, m, D.Layout(buf, k + m, bs, S, frag_stride=S * F, stripe_stride=F))
    buf.free()
    assert dev.ecamd_locate_fused_launches() > n0
    assert (st == want_st).all() and (su == want_su).all()
    assert su[1] == 1 << (k + 1) and su[2] == 1 << 6 and not su[0]


def test_framed_fragments_at_payload_offset(D, dev):
    from liberasurecode_amd import _lib, frame
    k, m = 10, 4
    size = k * (8192 + 64) - 6
    fb = frame.FrameBatch(frame.RS_VAND, k, m, size, S)
    obj = D.DeviceBuffer(fb.obj_stride * S)
    _lib.check(dev.ecamd_fill_splitmix(obj.ptr, fb.obj_stride, 0, 1, size, S, 0, 0x99, None), "fill")
    fb.encode(obj)
    assert fb.blocksize % 2 == 0
    args = (fb.base + frame.HEADER, fb.stripe_stride, fb.frag_stride, fb.blocksize, S)
    rc, st, su, checked = raw_locate(dev, D, k, m, [], *args)
    assert rc == 0 and checked == 0xF << k and not st[:S].any() and not su[:S].any()
    frags = fb.fragments()
    frags[2, 4, frame.HEADER + 5000] ^= 0x08  # a payload byte of data fragment 4, stripe 2
    fb.upload_fragments(frags)
    payload = np.ascontiguousarray(frags[:, :, frame.HEADER:frame.HEADER + fb.blocksize])
    want_st, want_su = oracle_locate(k, m, payload, [])
    rc, st, su, _ = raw_locate(dev, D, k, m, [], *args)
    assert rc == 0 and want_su[2] == 1 << 4 and (st[:S] == want_st).all() and (su[:S] == want_su).all()
    obj.free()
    fb.buf.free()


@pytest.mark.parametrize("k,m,hd", [(10, 6, 4), (3, 3, 3)])
def test_flat_xor(D, dev, k, m, hd):
    bs = 4096 + 10
    full = np.empty((S, k + m, bs), np.uint8)
    for s in range(S):
        full[s, :k] = stripe_fragments(900 + s, k, bs)
        full[s, k:] = XO.encode_bytes(k, m, hd, full[s, :k])
    pb, _ = X.tables(k, m, hd)

    def run(held):
        lay = TC.padded(D, held, 16, 77)
        try:
            return D.xor_locate(k, m, hd, lay)
        finally:
            lay.buf.free()

    n0 = dev.ecamd_locate_fused_launches()
    st, su = run(full)
    assert not st.any() and not su.any()
    for d in (0, k - 1):  # a data flip: status as the check's, that data bit alone
        held = full.copy()
        held[1, d, bs - 1] ^= 0x10
        st, su = run(held)
        assert st[1] == sum(1 << (k + p) for p in range(m) if pb[p] >> d & 1)
        assert su[1] == 1 << d and not su[0] and not su[2], (d, hexes(su))
    for p in (0, m - 1):  # a parity flip: that parity alone
        held = full.copy()
        held[2, k + p, 0] ^= 0x01
        st, su = run(held)
        assert st[2] == 1 << (k + p) and su[2] == 1 << (k + p) and not su[0] and not su[1]
    # two fragments whose syndromes no single fragment produces: different words of two data
    # fragments, and a data fragment with a parity that does not contain it
    held = full.copy()
    held[1, 0, 7] ^= 0x01
    held[1, 1, 2001] ^= 0x01
    st, su = run(held)
    assert st[1] and not su.any(), hexes(su)
    out = [p for p in range(m) if not pb[p] >> 0 & 1]
    if out:
        held = full.copy()
        held[1, 0, 7] ^= 0x01
        held[1, k + out[0], 7] ^= 0x01
        st, su = run(held)
        assert st[1] and not su.any(), hexes(su)
    assert dev.ecamd_locate_fused_launches() == n0


def test_scrub_repairs_located_stripes_and_leaves_the_rest(D, dev):
    k, m, nS = 10, 4, 6
    bs = 2 * 4096 + TAIL
    good = np.empty((nS, k + m, bs), np.uint8)
    for s in range(nS):
        good[s, :k] = stripe_fragments(700 + s, k, bs)
        good[s, k:] = orc.encode(k, m, good[s, :k])
    bad = good.copy()
    bad[1, 3, 5000:5040] ^= 0x5A       # a data fragment
    bad[2, k + 2, 17] ^= 0x01          # a parity fragment
    bad[3, 8, 2 * 4096 + 30] ^= 0x80   # a byte of the tail
    bad[4, 0, 100] ^= 0x01             # two bad fragments
    bad[4, 9, 4096 + 100] ^= 0x01
    lay = D.Layout.alloc(k + m, bs, nS)
    try:
        lay.upload_stripes(bad)
        n0 = dev.ecamd_bitslice_launches()
        st, su, counts = D.rs_scrub(k, m, lay)
        assert counts == (2, 3, 1), counts
        assert list(su) == [0, 1 << 3, 1 << (k + 2), 1 << 8, 0, 0], hexes(su)
        assert st[4] and not st[0] and not st[5]
        after = lay.download_stripes()
        for s in (0, 1, 2, 3, 5):
            assert (after[s] == good[s]).all(), s
        assert (after[4] == bad[4]).all()
        again, _ = D.rs_check(k, m, lay)
        assert list(again != 0) == [False, False, False, False, True, False]
        assert dev.ecamd_bitslice_launches() > n0
    finally:
        lay.buf.free()


def test_fresh_process_runs_shipped_locate_kernels_at_first_call(tmp_path):
    """Empty $ECAMD_JIT_CACHE, default knob (bitslice 1: never waits for a compile): the first locate of
    (10,4), full stripe and with fragment 5 missing, runs fused -- its code object came from lib/jit/."""
    cache = tmp_path / "jitcache"
    cache.mkdir(mode=0o700)
    env = dict(os.environ, ECAMD_JIT_CACHE=str(cache))
    r = subprocess.run([sys.executable, os.path.join(HERE, "locate_shipped_run.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for name in ("full", "lost5"):
        assert out[name + "_fused_launches"] > 0, out
        assert out[name + "_clean"] and out[name + "_located"], out
    assert out["cache_objects"] == 0, out
