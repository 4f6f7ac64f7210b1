"""GPU: check and locate over every shipped pattern, every culprit and whole-word errors.

test_gpu_locate.py pins paths, strides and canaries on a handful of one-bit flips.  Here the data the
kernels decide from is swept: for every pattern of prebuild.LOCATE_OPS (each one a fused kernel of its
own, generated from its own syndrome map and ratio matrix), a few that compile at run time and two flat
XOR codes, one batch damages every participating fragment in turn with whole 16-bit words of random
value -- a few words, and again with two dozen, so every input candidate's network and every plane of
it decides something -- and adds the two-fragment stripes, among them two fragments in one tile on different lanes, which only the
wave-wide reduction of each candidate's verdict tells from a located stripe.

Expected values never come from the code under test: test_gpu_locate.oracle_locate and
test_gpu_check.oracle_status judge rs_vand, the same definitions over oracle/xor_oracle.py judge flat
XOR.  Each pattern runs with knob bitslice 2 and 0; the fused-launch counters pin the path and the two
paths must agree byte for byte."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
import test_gpu_check as TC
import test_gpu_locate as TL
from liberasurecode_amd import prebuild
from test_gpu_check import D, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
XO = TC.XO
TAIL = TC.TAIL
FILL = TC.FILL

RS_PATTERNS = [(k, m, list(miss)) for k, m, miss in prebuild.LOCATE_OPS]
SHIPPED = len(RS_PATTERNS)
# compiled at run time (knob 2 waits): one loss of (20,8), R = 2 of (20,8) and (10,4), a code nobody ships
RS_PATTERNS += [(20, 8, [3]), (20, 8, [0, 5, 9, 21, 22, 27]), (10, 4, [2, 7]), (6, 3, [])]
XOR_CODES = [(10, 6, 4), (3, 3, 3)]


def xor_status(k, m, hd, held):
    """TC.oracle_status for flat XOR: bit k + p iff stored parity p differs from the reference encode
    of the stored data."""
    out = np.zeros(held.shape[0], np.uint32)
    for s in range(held.shape[0]):
        par = XO.encode_bytes(k, m, hd, held[s, :k])
        for p in range(m):
            if (par[p] != held[s, k + p]).any():
                out[s] |= np.uint32(1 << (k + p))
    return out


def xor_oracle_locate(k, m, hd, held):
    """TL.oracle_locate for flat XOR: f is a suspect of a dirty stripe iff replacing the stored f by the
    reference's reconstruct of f makes the stripe's status zero."""
    code = XO.XorCode(k, m, hd)
    status = xor_status(k, m, hd, held)
    suspects = np.zeros(held.shape[0], np.uint32)
    for s in np.nonzero(status)[0]:
        for f in range(k + m):
            bufs = [np.array(x) for x in held[s]]
            assert code.reconstruct_one(bufs, [f], f) == 0
            trial = np.array(held[s:s + 1])
            trial[0, f] = bufs[f]
            if not xor_status(k, m, hd, trial)[0]:
                suspects[s] |= np.uint32(1 << f)
    return status, suspects


def xor_word(held, s, f, p, v):
    """XOR the 16-bit word at even byte offset p of fragment f (low byte first, as the kernels read it)."""
    assert p % 2 == 0 and 0 < v <= 0xFFFF
    held[s, f, p] ^= v & 0xFF
    held[s, f, p + 1] ^= v >> 8


DENSE = 24


def damaged_batch(seed, k, n, bs, tile, avail, encode, dense=True):
    """Reference-encoded stripes with whole-word damage: (good, bad, singles {stripe: f}, pairs [stripe],
    clean [stripe]).  One stripe per participating fragment (1-3 words at random even offsets; the first
    word's region cycles over tile 0, tile 1 and the tail, and fragments 0, 1, 2 of the list get an
    all-ones, a high-byte-only and a low-byte-only error); with `dense` a second stripe per fragment with
    DENSE random words (a candidate's network with two planes swapped passes one random word with
    probability 1/2, DENSE of them with 2^-DENSE); four two-fragment stripes; three clean ones first, in
    the middle and last."""
    rng = np.random.default_rng(seed)
    assert bs - 2 * tile >= 2 and tile >= 1024 + 64
    items = [("single", f) for f in avail] + ([("dense", f) for f in avail] if dense else [])
    half = len(items) // 2
    order = [("clean", -1)] + items[:half] + [("clean", -1)] + items[half:]
    order += [(what, -1) for what in ("lanes", "word", "tiles", "tail", "clean")]
    nS = len(order)
    good = np.empty((nS, n, bs), np.uint8)
    for s in range(nS):
        good[s, :k] = rng.integers(0, 256, size=(k, bs), dtype=np.uint8)
        good[s, k:] = encode(good[s, :k])
    bad = good.copy()
    singles, pairs, clean = {}, [], []

    def value():
        return int(rng.integers(1, 0x10000))

    def even(lo, hi):
        return int(rng.integers(lo // 2, hi // 2)) * 2

    regions = ((0, tile), (tile, 2 * tile), (2 * tile, bs))
    for s, (what, f) in enumerate(order):
        if what == "clean":
            clean.append(s)
        elif what == "single":
            i = list(avail).index(f)
            words = {even(*regions[i % 3])}
            for _ in range(int(rng.integers(0, 3))):
                words.add(even(0, bs))
            for j, p in enumerate(sorted(words)):
                v = value()
                if j == 0 and i < 3:
                    v = (0xFFFF, (v & 0xFF00) or 0x8000, (v & 0x00FF) or 0x01)[i]
                xor_word(bad, s, f, p, v)
            singles[s] = f
        elif what == "dense":
            for p in {even(0, bs) for _ in range(DENSE)}:
                xor_word(bad, s, f, p, value())
            singles[s] = f
        else:
            f1, f2 = (int(x) for x in rng.choice(avail[:k] if what == "lanes" else avail, 2, replace=False))
            v1 = value()
            v2 = v1 ^ value()  # never the same error in both
            t0 = tile * int(rng.integers(0, 2))
            if what == "lanes":  # one tile, 16-byte chunks 0 and 62: different lanes whatever the lane's share
                p1, p2 = t0 + 10, t0 + 1000
            elif what == "word":
                p1 = p2 = even(0, bs)
            elif what == "tiles":
                p1, p2 = even(0, tile), even(tile, 2 * tile)
            else:
                p1, p2 = even(0, 2 * tile), even(2 * tile, bs)
            xor_word(bad, s, f1, p1, v1)
            xor_word(bad, s, f2, p2, v2)
            pairs.append(s)
    return good, bad, singles, pairs, clean


def assert_located(want_st, want_su, singles, pairs, clean, definite):
    """The condition on the inputs: clean stripes clean, dirty ones dirty and, where the code can tell
    (`definite`: three checked fragments or more), every single located and no pair."""
    assert not want_st[clean].any() and not want_su[clean].any()
    assert want_st[list(singles)].all() and want_st[pairs].all()
    if definite:
        for s, f in singles.items():
            assert want_su[s] == 1 << f, (s, f, hex(int(want_su[s])))
        assert not want_su[pairs].any(), TL.hexes(want_su[pairs])


def prebuilt(fn, k, m, missing, shipped, tmp):
    """ecamd_check_prebuild / ecamd_locate_prebuild's answer.  A shipped pattern is asked against lib/jit/,
    where its object already lies, so nothing is compiled (and nothing may appear there)."""
    arr = (C.c_int * (len(missing) + 1))(*(list(missing) + [-1]))
    if not shipped:
        # asked after the knob 2 run, against the run time's own cache: the object it compiled there has
        # the prebuild's name, so this compiles nothing either (and only compiles again if it does not)
        cache = os.environ.get("ECAMD_JIT_CACHE") or "/tmp/ecamd-jit-%d" % os.getuid()
        return fn(k, m, C.cast(arr, C.c_void_p), b"gfx950", (cache if os.path.isdir(cache) else str(tmp)).encode())
    before = sorted(os.listdir(prebuild.JIT_DIR))
    rc = fn(k, m, C.cast(arr, C.c_void_p), b"gfx950", prebuild.JIT_DIR.encode())
    assert sorted(os.listdir(prebuild.JIT_DIR)) == before, "a shipped check / locate object was missing from lib/jit/"
    return rc


def both_paths(dev, run, fused, want_st, want_su):
    """run() -> (locate status, suspects, check status) with knob bitslice 2, then 0; fused() -> whether
    the pattern has a fused (locate, check) form."""
    got = {}
    for knob in (2, 0):
        dev.ecamd_tune(b"bitslice", knob)
        l0, c0 = dev.ecamd_locate_fused_launches(), dev.ecamd_check_fused_launches()
        st, su, chk = run()
        ran = (dev.ecamd_locate_fused_launches() > l0, dev.ecamd_check_fused_launches() > c0)
        assert ran == (fused() if knob == 2 else (False, False)), (knob, ran)
        bad = np.nonzero((st != want_st) | (su != want_su) | (chk != want_st))[0]
        assert not len(bad), (knob, [(int(s), hex(int(st[s])), hex(int(su[s])), hex(int(chk[s])), hex(int(want_st[s])),
                                     hex(int(want_su[s]))) for s in bad[:6]])
        got[knob] = (st, su, chk)
    for a, b in zip(got[2], got[0]):
        assert a.dtype == np.uint32 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("index", range(len(RS_PATTERNS)), ids=["%d_%d_%s" % (k, m, "-".join(map(str, miss)) or "full")
                                                                 for k, m, miss in RS_PATTERNS])
def test_rs_every_culprit_whole_words(D, dev, tmp_path, index):
    k, m, missing = RS_PATTERNS[index]
    n = k + m
    tile = TC.tile_of(m)  # by the code, not by the pattern: 16 KiB for every (20,8) pattern, whatever R is
    bs = 2 * tile + TAIL
    avail = [f for f in range(n) if f not in missing]
    R = len(avail) - k
    # the dense stripes double the oracle's work: left out where that is seconds, the (20,8) patterns that
    # compile at run time on top
    good, bad, singles, pairs, clean = damaged_batch(1000 + index, k, n, bs, tile, avail, lambda d: orc.encode(k, m, d),
                                                     dense=index < SHIPPED or tile == 4096)
    held = TC.held_of(bad, missing)
    want_st, want_su = TL.oracle_locate(k, m, held, missing)
    assert_located(want_st, want_su, singles, pairs, clean, R >= 3)
    never = sum(1 << f for f in missing) | (0xFFFFFFFF & ~((1 << n) - 1))
    assert not (want_su & never).any()

    def fused():
        fused_locate = prebuilt(dev.ecamd_locate_prebuild, k, m, missing, index < SHIPPED, tmp_path)
        fused_check = prebuilt(dev.ecamd_check_prebuild, k, m, missing, index < SHIPPED, tmp_path)
        assert fused_locate >= 0 and fused_check >= 0
        if index < SHIPPED:  # every shipped object is a fused kernel that runs here; (4,2) ships none
            assert (fused_locate > 0) == (fused_check > 0) == ((k, m) != (4, 2))
        return fused_locate > 0, fused_check > 0

    lay = D.Layout.alloc(n, bs, held.shape[0])
    try:
        lay.upload_stripes(held)
        mask = sum(1 << f for f in avail[k:])

        def run():
            st, su, checked = D.rs_locate(k, m, lay, missing)
            chk, checked2 = D.rs_check(k, m, lay, missing)
            assert checked == checked2 == mask
            return st, su, chk

        both_paths(dev, run, fused, want_st, want_su)
    finally:
        lay.buf.free()


@pytest.mark.parametrize("k,m,hd", XOR_CODES)
def test_flat_xor_every_culprit_whole_words(D, dev, k, m, hd):
    n = k + m
    tile = 4096
    bs = 2 * tile + TAIL
    good, bad, singles, pairs, clean = damaged_batch(2000 + k, k, n, bs, tile, list(range(n)),
                                                     lambda d: XO.encode_bytes(k, m, hd, d))
    want_st, want_su = xor_oracle_locate(k, m, hd, bad)
    assert_located(want_st, want_su, singles, pairs, clean, True)
    lay = D.Layout.alloc(n, bs, bad.shape[0])
    try:
        lay.upload_stripes(bad)

        def run():
            st, su = D.xor_locate(k, m, hd, lay)
            return st, su, D.xor_check(k, m, hd, lay)

        both_paths(dev, run, lambda: (False, False), want_st, want_su)
    finally:
        lay.buf.free()


def test_fresh_process_runs_every_shipped_check_and_locate_object(tmp_path):
    """Empty $ECAMD_JIT_CACHE, default knob (bitslice 1: never waits for a compile): the first check and
    the first locate of every pattern of CHECK_OPS / LOCATE_OPS run fused wherever the prebuild has a
    fused form -- each from its own object in lib/jit/ -- give the right words, and nothing is compiled."""
    cache = tmp_path / "jitcache"
    cache.mkdir(mode=0o700)
    env = dict(os.environ, ECAMD_JIT_CACHE=str(cache))
    r = subprocess.run([sys.executable, os.path.join(HERE, "locate_all_shipped_run.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    want = []
    for op, ops in (("check", prebuild.CHECK_OPS), ("locate", prebuild.LOCATE_OPS)):
        want += [(op, k, m, list(miss)) for k, m, miss in ops]
    got = {(x["op"], x["k"], x["m"], tuple(x["missing"])): x for x in lines[:-1]}
    assert sorted(got) == sorted((op, k, m, tuple(miss)) for op, k, m, miss in want)
    for key, x in got.items():
        assert x["prebuilt"] >= 0, x
        assert (x["fused_launches"] > 0) == (x["prebuilt"] > 0), x
        assert (x["prebuilt"] > 0) == (key[1:3] != (4, 2)), x
        assert x["clean"] and x["input_found"] and x["checked_found"], x
    assert lines[-1] == {"cache_objects": 0}, lines[-1]
