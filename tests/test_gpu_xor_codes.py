"""GPU: every flat XOR device kernel on all 38 codes of tests/golden/xor_codes.json.

The kernels are specialised by the shape of the code -- xor_check_kernel<KG, LOCATE, Args> by its load
groups (KG = (k + m + 3) / 4 for full stripes, (participants + 3) / 4 for the slot form) with a row loop
that ends at the surviving rows, xor_stream_kernel<KG, COPY> by (inputs + 3) / 4 -- and the suites that
pin paths, layouts and canaries (test_gpu_xor_scrub, test_gpu_locate_sweep, test_gpu_correct,
test_gpu_xor_degraded, test_gpu_xor_batch) run them on two to five codes.  Here each section runs one
batch of theirs on every code:

  a. check and locate of full stripes, both tile forms, fused and generic;
  b. correct and scrub of full stripes;
  c. check, locate and correct with one, two and (hd 4) three fragments missing;
  d. encode, decode, reconstruct and decode_multi at a size that xor_small_kernel cannot take, which
     ecamd_xor_stream_launches proves.

Expected values never come from the code under test: status and suspects are
test_gpu_locate_sweep.xor_oracle_locate (full stripes) and test_gpu_xor_degraded.oracle (the reduction
rule of test_xor_degraded_plan.reduce over the golden parity bitmaps), bytes are oracle/xor_oracle.py's.
Every comparison is byte-exact.  The helpers and their cached batches are those suites' own."""
import json
import os

import numpy as np
import pytest

import test_gpu_check as TC
import test_gpu_locate_sweep as SW
import test_gpu_xor_batch as XB
import test_gpu_xor_degraded as XD
import test_gpu_xor_scrub as XS
import test_xor_degraded_plan as P
from test_gpu_check import D, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
XO = TC.XO
TAIL = TC.TAIL
CODES = [c[:3] for c in P.CODES]
IDS = ["%d_%d_%d" % c for c in CODES]
TILE = 2048  # test_gpu_xor_scrub's: bs = 2 * 2048 + TAIL, four 1 KiB tiles or one 4 KiB tile, and a tail
with open(os.path.join(TC.HERE, "golden", "tune_rules.json")) as fh:
    SMALL_CHUNKS = json.load(fh)["knobs"]["small_chunks"]["default"]
STREAM_BS, STREAM_S = 2 * 4096 + 10, 9  # two 4 KiB or eight 1 KiB tiles and a ragged tail; 513 * 9 chunks
STREAM_THREADS = [256, 64]  # knob xor_threads: the 4 KiB and the 1 KiB tile form

# The (load groups, surviving rows) classes of the slot form that section c must reach.
SLOT_CLASSES = {(1, 1), (2, 2), (2, 3), (3, 2), (3, 3), (3, 4), (3, 5), (4, 3), (4, 4), (4, 5), (5, 3), (5, 4), (5, 5),
                (6, 3), (6, 4), (6, 5), (7, 5)}
# (KG, rows): codes, of the full form.
FULL_CLASSES = {(2, 3): 1, (3, 5): 6, (3, 6): 2, (4, 5): 6, (4, 6): 8, (5, 6): 8, (6, 6): 5, (7, 6): 2}


@pytest.fixture()
def knobs(dev):
    """Every knob this file sets back at its default afterwards."""
    yield dev
    for key, value in ((b"xor_check_fused", -1), (b"xor_check_threads", 0), (b"xor_threads", 0)):
        dev.ecamd_tune(key, value)


def missing_lists(k, m, hd):
    return [[k // 2], [k + m - 1], [0, k]] + ([[1, k - 1, k + 1]] if hd == 4 else [])


DEGRADED = [(k, m, hd, miss) for k, m, hd in CODES for miss in missing_lists(k, m, hd)]


def test_the_golden_file_has_38_codes_and_they_fall_into_the_known_classes():
    assert len(CODES) == 38 and len(set(CODES)) == 38
    full = {}
    for k, m, hd in CODES:
        full[((k + m + 3) // 4, m)] = full.get(((k + m + 3) // 4, m), 0) + 1
    assert full == FULL_CLASSES
    assert sorted({(k + 3) // 4 for k, m, hd in CODES}) == [1, 2, 3, 4, 5]  # stream KG 1, 2, 3, 4 and (5 ->) 8
    reached = set()
    for k, m, hd, missing in DEGRADED:
        assert len(set(missing)) == len(missing) and all(0 <= f < k + m for f in missing)
        rows, sig, covered, alive = P.reduce(k, m, XD.PB[(k, m, hd)], missing)
        reached.add(((bin(covered).count("1") + 3) // 4, alive))
    assert SLOT_CLASSES <= reached, sorted(SLOT_CLASSES - reached)


# ---- a, b: full stripes ---------------------------------------------------------------------------

_full = {}


def full_batch(k, m, hd):
    """test_gpu_xor_scrub.batch(k, m, hd, TILE) with the reference-encoded originals: (good, bad, status,
    suspects).  The condition on the inputs: every single located uniquely, no pair, the clean clean."""
    key = (k, m, hd)
    if key not in _full:
        bad, want_st, want_su = XS.batch(k, m, hd, TILE)
        n, bs = k + m, 2 * TILE + TAIL
        good, again, singles, pairs, clean = SW.damaged_batch(3000 + k + TILE, k, n, bs, TILE, list(range(n)),
                                                              XS.encoder(k, m, hd))
        assert again.shape == bad.shape == (3 + 2 * n + 4, n, bs) and (again == bad).all()
        SW.assert_located(want_st, want_su, singles, pairs, clean, True)
        good.setflags(write=False)
        _full[key] = (good, bad, want_st, want_su)
    return _full[key]


def one_bit(word):
    word = int(word)
    return word != 0 and not word & (word - 1)


@pytest.mark.parametrize("k,m,hd", CODES, ids=IDS)
def test_check_and_locate_of_full_stripes(D, knobs, k, m, hd):
    """test_gpu_xor_scrub.test_every_culprit_fused_and_generic on every code, the four forms in one case."""
    dev = knobs
    good, bad, want_st, want_su = full_batch(k, m, hd)
    bs = bad.shape[2]
    lay = D.Layout.alloc(k + m, bs, bad.shape[0])
    got = {}
    try:
        lay.upload_stripes(bad)
        for threads, form_tile in XS.FORMS:
            assert bs // form_tile >= 1 and bs % form_tile == TAIL
            dev.ecamd_tune(b"xor_check_threads", threads)
            for fused in (1, 0):
                dev.ecamd_tune(b"xor_check_fused", fused)
                c0 = XS.counters(dev)
                st, su = D.xor_locate(k, m, hd, lay)
                chk = D.xor_check(k, m, hd, lay)
                c1 = XS.counters(dev)
                assert (c1[0] > c0[0], c1[1] > c0[1]) == (bool(fused), bool(fused)), (threads, fused, c0, c1)
                assert c1[2:] == c0[2:]
                wrong = np.nonzero((st != want_st) | (su != want_su) | (chk != want_st))[0]
                assert not len(wrong), (threads, fused, [(int(s), hex(int(st[s])), hex(int(su[s])), hex(int(chk[s])),
                                                          hex(int(want_st[s])), hex(int(want_su[s]))) for s in wrong[:6]])
                got[(threads, fused)] = (st, su, chk)
        assert (lay.download_stripes() == bad).all()
    finally:
        lay.buf.free()
    assert len(got) == 4
    first = got[(XS.FORMS[0][0], 1)]
    for other in got.values():
        for a, b in zip(first, other):
            assert a.dtype == np.uint32 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k,m,hd", CODES, ids=IDS)
def test_correct_and_scrub_of_full_stripes(D, knobs, k, m, hd):
    dev = knobs
    good, bad, want_st, want_su = full_batch(k, m, hd)
    nS = bad.shape[0]
    clean, one, _, rest = XD.tallies(want_st, want_su)
    assert clean == 3 and one == 2 * (k + m) and rest == 4
    for what in ("correct", "scrub"):
        lay = D.Layout.alloc(k + m, bad.shape[2], nS)
        try:
            lay.upload_stripes(bad)
            n0 = dev.ecamd_correct_launches()
            if what == "correct":
                st, su, pr, counts = D.xor_correct(k, m, hd, lay)
                assert pr is None and counts == (clean, one, 0, rest), counts
                assert dev.ecamd_correct_launches() == n0 + 1
            else:
                st, su, counts = D.xor_scrub(k, m, hd, lay)
                assert counts == (clean, one, rest), counts
            after = lay.download_stripes()
        finally:
            lay.buf.free()
        wrong = np.nonzero((st != want_st) | (su != want_su))[0]
        assert not len(wrong), (what, [(int(s), hex(int(st[s])), hex(int(su[s])), hex(int(want_st[s])), hex(int(want_su[s])))
                                       for s in wrong[:6]])
        for s in range(nS):
            want = good[s] if one_bit(want_su[s]) else bad[s]
            assert (after[s] == want).all(), (what, s, hex(int(want_su[s])))


# ---- c: fragments missing -------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,hd,missing", DEGRADED, ids=["%d_%d_%d-%s" % (k, m, hd, "-".join(map(str, x))) for k, m, hd, x in DEGRADED])
def test_check_locate_and_correct_with_fragments_missing(D, knobs, k, m, hd, missing):
    """test_gpu_xor_degraded.test_every_covered_culprit_on_every_path on every code, without the dense
    stripes; every pattern here is one the reference decodes."""
    dev = knobs
    good, held, singles, want_st, want_su, covered = XD.batch(k, m, hd, missing, dense=False)
    nS, BS = held.shape[0], XD.BS
    assert held.shape[2] == BS == 2 * TILE + TAIL
    ref = XD.reference_dirty(k, m, hd, missing, held)
    assert ref is not None
    assert ((want_st != 0) == ref).all(), np.nonzero((want_st != 0) != ref)[0]
    alive = P.reduce(k, m, XD.PB[(k, m, hd)], missing)[3]
    assert alive >= 1
    got = []
    for threads, form_tile in XS.FORMS:
        assert BS // form_tile >= 1 and BS % form_tile == TAIL
        dev.ecamd_tune(b"xor_check_threads", threads)
        for fused in (1, 0):
            dev.ecamd_tune(b"xor_check_fused", fused)
            # which fused counter a locate moves: one surviving row tells no fragment of it from another, so
            # the locate runs the check form and names the whole row (the degraded driver)
            locate_form = (False, bool(fused)) if alive >= 2 else (bool(fused), False)
            lay = XD.upload(D, held)
            try:
                where = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, BS, nS)
                c0 = XS.counters(dev)
                rc, chk, _, _, cov = XD.raw(dev, D, "check", k, m, hd, missing, *where)
                c1 = XS.counters(dev)
                assert rc == 0 and cov == covered
                assert (c1[0] > c0[0], c1[1] > c0[1]) == (bool(fused), False) and c1[2:] == c0[2:], (threads, fused, c0, c1)
                rc, st, su, _, cov = XD.raw(dev, D, "locate", k, m, hd, missing, *where)
                c2 = XS.counters(dev)
                assert rc == 0 and cov == covered
                assert (c2[0] > c1[0], c2[1] > c1[1]) == locate_form and c2[2:] == c1[2:], (threads, fused, c1, c2)
                wrong = np.nonzero((st != want_st) | (su != want_su) | (chk != want_st))[0]
                assert not len(wrong), (threads, fused, [(int(s), hex(int(st[s])), hex(int(su[s])), hex(int(chk[s])),
                                                          hex(int(want_st[s])), hex(int(want_su[s]))) for s in wrong[:6]])
                assert (lay.download_stripes() == held).all()
                n0 = dev.ecamd_correct_launches()
                rc, st2, su2, counts, cov = XD.raw(dev, D, "correct", k, m, hd, missing, *where)
                assert rc == 0 and cov == covered and dev.ecamd_correct_launches() == n0 + 1
                assert st2.tobytes() == st.tobytes() and su2.tobytes() == su.tobytes()
                assert counts == XD.tallies(want_st, want_su), (counts, XD.tallies(want_st, want_su))
                XD.check_corrected(lay.download_stripes(), good, held, missing, want_st, want_su, singles)
                got.append((st, su, chk))
            finally:
                lay.buf.free()
    assert len(got) == 4
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.dtype == np.uint32 and a.tobytes() == b.tobytes()


# ---- d: the stream kernel -------------------------------------------------------------------------

def stream_case(k, m, hd):
    """Random (inconsistent) stripes and what the reference makes of them: the host batch and a list of
    (op, argument, expected stripes, fragments to compare)."""
    n = k + m
    oc = XO.XorCode(k, m, hd)
    host = np.random.default_rng(11000 + 100 * k + 10 * m + hd).integers(0, 256, size=(STREAM_S, n, STREAM_BS), dtype=np.uint8)
    host.setflags(write=False)
    pats = XB._recoverable(k, m, hd, 31 + k, 3)
    assert len(pats) == 3 and all(pats)

    def expect(fn, lost_of):
        out = np.empty_like(host)
        for s in range(STREAM_S):
            bufs = XB._zeroed(host[s], lost_of(s))
            fn(bufs, s)
            out[s] = np.stack(bufs)
        return out

    def decode(p):
        def fn(bufs, s):
            assert oc.decode(bufs, p, 1) == 0
        return fn

    def reconstruct(p):
        def fn(bufs, s):
            assert oc.reconstruct_one(bufs, p, p[0]) == 0
        return fn

    per = [pats[s % 3] for s in range(STREAM_S)]
    per[3] = []

    def multi(bufs, s):
        assert not per[s] or oc.decode(bufs, per[s], 1) == 0

    everything = list(range(n))
    ops = [("encode", None, expect(lambda bufs, s: oc.encode(bufs), lambda s: range(k, n)), everything)]
    for p in pats:
        ops.append(("decode", p, expect(decode(p), lambda s: p), everything))
        # ecamd_xor_reconstruct promises fragment p[0] alone; the survivors must stay as they were
        ops.append(("reconstruct", p, expect(reconstruct(p), lambda s: p), [f for f in everything if f not in p[1:]]))
    ops.append(("decode_multi", per, expect(multi, lambda s: per[s]), everything))
    return host, ops


@pytest.mark.parametrize("k,m,hd", CODES, ids=IDS)
def test_encode_decode_and_reconstruct_on_the_stream_kernel(D, knobs, k, m, hd):
    dev = knobs
    chunks = (STREAM_BS + 15) // 16 * STREAM_S
    assert chunks == 513 * 9 > SMALL_CHUNKS == 4096  # no pass of this batch is small_launch's
    host, ops = stream_case(k, m, hd)
    for threads in STREAM_THREADS:
        assert STREAM_BS // (16 * threads) >= 2 and STREAM_BS % (16 * threads) == 10
        dev.ecamd_tune(b"xor_threads", threads)
        for op, arg, want, compare in ops:
            lay = D.Layout.alloc(k + m, STREAM_BS, STREAM_S)
            try:
                lay.upload_stripes(host)
                n0 = dev.ecamd_xor_stream_launches()
                if op == "encode":
                    D.xor_encode(k, m, hd, lay)
                elif op == "decode":
                    D.xor_decode(k, m, hd, arg, lay, decode_parity=True)
                elif op == "reconstruct":
                    D.xor_reconstruct(k, m, hd, arg, arg[0], lay)
                else:
                    D.xor_decode_multi(k, m, hd, arg, lay, decode_parity=True)
                ran = dev.ecamd_xor_stream_launches() - n0
                got = lay.download_stripes()
            finally:
                lay.buf.free()
            assert ran > 0, (threads, op, arg)
            wrong = [(s, f) for s in range(STREAM_S) for f in compare if (got[s, f] != want[s, f]).any()]
            assert not wrong, (threads, op, arg, wrong[:8])


def test_a_small_encode_leaves_the_stream_counter_alone(D, knobs):
    dev = knobs
    k, m, hd, bs = 3, 3, 3, 48
    assert (bs + 15) // 16 <= SMALL_CHUNKS
    host = np.random.default_rng(12000).integers(0, 256, size=(1, k + m, bs), dtype=np.uint8)
    lay = D.Layout.alloc(k + m, bs, 1)
    try:
        lay.upload_stripes(host)
        n0 = dev.ecamd_xor_stream_launches()
        D.xor_encode(k, m, hd, lay)
        got = lay.download_stripes()
        assert dev.ecamd_xor_stream_launches() == n0
    finally:
        lay.buf.free()
    assert (got[0, :k] == host[0, :k]).all() and (got[0, k:] == XO.encode_bytes(k, m, hd, host[0, :k])).all()
