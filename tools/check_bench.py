#!/usr/bin/env python3
"""Cost of the stripe consistency check (ecamd_rs_check) against the encode it mirrors, at the C3
layout bench.py times (k=10 m=4, 1 MiB fragments, 256 stripes) and at C5 (k=20 m=8, 4 MiB):
HIP events around single launches on one stream, a clock-settling warm-up, then `--reps` alternating
repetitions of (a) ecamd_rs_encode, (b) the fused check (knob bitslice 2), (c) the generic check (knob
bitslice 0; C3 only) -- each repetition the mean of `--n` back-to-back calls.  (b) moves the encode's
14 MiB per stripe and stores nothing; both are rated on those algorithmic bytes against 8 TB/s.
`--per-cu LIST` repeats (b) with knob check_per_cu at each value (resident one-wave workgroups per
CU; -1 the default policy).  `--parent-encode-ms X` records the yardstick: the encode pass time of a
bench.py run of the parent commit in the same session.  One JSON document on stdout, also written to
`--out`.

`--locate` measures ecamd_rs_locate instead (C3 only): alternating repetitions of (a) the fused check and
the fused locate on a clean batch -- the same loads and network; locate adds one memset and the finalize
launch -- and (b) both on an all-dirty batch, fragment 3 of every stripe rewritten with other data so
that every wave of every tile takes the second stage.  The VGPR and scratch figures of the shipped
(10,4) and (20,8) locate objects are read from freshly built code objects when llvm-readelf is there.
`--parent-check-ms X` records the parent commit's fused check time of the same session.

`--xor` measures flat XOR instead, per shape of `--xor-shapes` ((10,6,4) at 1 MiB x 256 stripes and
(3,3,3) at 4 KiB x 131072 by default): alternating repetitions of (a) ecamd_xor_encode and ecamd_xor_check /
ecamd_xor_locate on (b) the generic path (knob xor_check_fused 0, which is what ran before the fused
kernel existed) and (c) each tile form of the fused kernel (knob xor_check_threads 256, 64 and 0, the
default), on clean data and then on an all-dirty batch (data fragment 1 of every stripe rewritten).
The bar for (c) on clean data is (a)'s mean plus the spread of (a)'s own repetitions.  `--tree DIR` runs
the tool against the package and built libraries of another checkout: with the parent commit's, `--xor`
gives (a) and (b) as that commit runs them (it has the generic path alone).  `--xor --missing LIST`
measures the degraded calls instead, on the first shape, clean data and default knobs: ecamd_xor_check
against ecamd_xor_check_degraded with LIST lost (and the two locates), alternating; the bar for the
degraded form is the full-stripe mean plus the larger spread of the two series.

`--pairs` measures ecamd_rs_locate_pairs (C3 only) against ecamd_rs_locate, alternating: (a) on a clean
batch -- the pair stage adds one memset, one launch whose workgroups all end after two loads, and one
finalize --, (b) with one stripe of 256 holding two damaged words, (c) with two fragments of every
stripe rewritten, so that every word needs the pair.  With `--tree DIR` of the parent commit it times
ecamd_rs_locate alone (`--locate-only`: the same on this commit); `--pairs-merge THIS,BEFORE,AFTER` joins this commit's document with two such
runs of the same session, before and after it: their spread is the margin for (a).

`--correct` measures ecamd_rs_correct (C3 only).  (a) clean batch, HIP events: ecamd_rs_locate_pairs
against ecamd_rs_correct with pairs (without and with d_counts), alternating.  (b) one stripe of 256 with
two damaged words and (c) fragments 3 and 12 of every stripe rewritten: ecamd_rs_scrub_pairs against
ecamd_rs_correct, a host wall clock around call plus stream synchronise -- the scrub's cost includes its
host half --, the damaged batch copied back from a second device buffer outside the timed region before
every call.  With `--tree DIR` of the parent commit it times ecamd_rs_locate_pairs and
ecamd_rs_scrub_pairs alone; `--correct-merge THIS,BEFORE,AFTER` joins this commit's document with two
such runs of the same session, and `--added-launch-us X` (from a kernel trace of this commit on a clean
batch) completes the bar of (a): the parent's larger mean, plus the spread between its two runs, plus X."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:  # the package and libraries of another built checkout (before the imports below)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401

from liberasurecode_amd import _lib  # noqa: E402
from liberasurecode_amd import device as D  # noqa: E402

PEAK = 8e12  # bytes/s


def timed(st, fn, n):
    a, b = D.Event(), D.Event()
    a.record(st)
    for _ in range(n):
        fn()
    b.record(st)
    st.synchronize()
    return a.elapsed_ms(b) / n


def series(ms, algo):
    mean = sum(ms) / len(ms)
    return {"ms": [round(x, 4) for x in ms], "mean_ms": round(mean, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "tb_s": round(algo / (mean * 1e-3) / 1e12, 3), "frac_8tbs": round(algo / (mean * 1e-3) / PEAK, 4)}


def run(d, st, k, m, F, S, reps, n, generic, per_cu):
    lay = D.Layout.alloc(k + m, F, S)
    lay.fill_splitmix(nfrags=k, stream=st)
    status = D.DeviceBuffer(4 * S)
    checked = _lib.u32s([0])

    def encode():
        D.rs_encode(k, m, lay, stream=st)

    def check():
        _lib.check(d.ecamd_rs_check(k, m, None, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, F, S, status.ptr,
                                    checked, st.handle), "rs_check")

    d.ecamd_tune(b"bitslice", 2)
    encode()
    n0 = d.ecamd_check_fused_launches()
    check()
    st.synchronize()
    fused_launches = d.ecamd_check_fused_launches() - n0
    assert fused_launches > 0, "the fused check kernel did not run"
    assert not status.download().any(), "encoded stripes must check clean"
    for _ in range(60):  # settle the clocks
        encode()
    st.synchronize()
    ms = {"encode": [], "check_fused": [], "check_generic": []}
    caps = {c: [] for c in per_cu}
    for _ in range(reps):
        ms["encode"].append(timed(st, encode, n))
        ms["check_fused"].append(timed(st, check, n))
        for c in per_cu:
            d.ecamd_tune(b"check_per_cu", c)
            caps[c].append(timed(st, check, n))
        d.ecamd_tune(b"check_per_cu", -1)
        if generic:
            d.ecamd_tune(b"bitslice", 0)
            check()  # (its scratch is allocated outside the timing)
            ms["check_generic"].append(timed(st, check, max(2, n // 4)))
            d.ecamd_tune(b"bitslice", 2)
    assert not status.download().any()
    algo = S * (k + m) * F
    out = {"k": k, "m": m, "fragment_bytes": F, "stripes": S, "algorithmic_bytes": algo,
           "fused_launches_per_call": fused_launches,
           "encode": series(ms["encode"], algo), "check_fused": series(ms["check_fused"], algo)}
    if generic:
        out["check_generic"] = series(ms["check_generic"], algo)
        out["fused_over_generic"] = round(out["check_fused"]["mean_ms"] / out["check_generic"]["mean_ms"], 4)
    if per_cu:
        out["check_fused_per_cu"] = {str(c): series(v, algo) for c, v in caps.items()}
    out["check_over_encode"] = round(out["check_fused"]["mean_ms"] / out["encode"]["mean_ms"], 4)
    lay.buf.free()
    status.free()
    return out


def object_figures(d, k, m):
    """VGPRs, scratch bytes and size of the locate code object of (k, m), built into a temporary directory."""
    import re
    import subprocess
    import tempfile
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    with tempfile.TemporaryDirectory() as tmp:
        if d.ecamd_locate_prebuild(k, m, None, b"gfx950", tmp.encode()) != 1 or not os.path.exists(readelf):
            return None
        co = [n for n in os.listdir(tmp) if n.endswith(".co")][0]
        notes = subprocess.run([readelf, "--notes", os.path.join(tmp, co)], capture_output=True, text=True).stdout
        fig = {key: int(re.search(r"\." + key + r":\s+(\d+)", notes).group(1))
               for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
        fig["object_bytes"] = os.path.getsize(os.path.join(tmp, co))
        return fig


def run_locate(d, st, reps, n):
    k, m, F, S = 10, 4, 1 << 20, 256
    lay = D.Layout.alloc(k + m, F, S)
    lay.fill_splitmix(nfrags=k, stream=st)
    words = D.DeviceBuffer(8 * S)
    checked = _lib.u32s([0])
    args = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, F, S)

    def check():
        _lib.check(d.ecamd_rs_check(k, m, None, *args, words.ptr, checked, st.handle), "rs_check")

    def locate():
        _lib.check(d.ecamd_rs_locate(k, m, None, *args, words.ptr, words.ptr + 4 * S, checked, st.handle), "rs_locate")

    d.ecamd_tune(b"bitslice", 2)
    D.rs_encode(k, m, lay, stream=st)
    n0 = d.ecamd_locate_fused_launches()
    locate()
    st.synchronize()
    fused_launches = d.ecamd_locate_fused_launches() - n0
    assert fused_launches > 0, "the fused locate kernel did not run"
    assert not words.download().any(), "encoded stripes must read clean"
    for _ in range(60):  # settle the clocks
        check()
    st.synchronize()
    algo = S * (k + m) * F
    ms = {"check_clean": [], "locate_clean": [], "check_dirty": [], "locate_dirty": []}
    for _ in range(reps):
        ms["check_clean"].append(timed(st, check, n))
        ms["locate_clean"].append(timed(st, locate, n))
    # all-dirty: fragment 3 of every stripe holds other data, so every word of every tile disagrees
    _lib.check(d.ecamd_fill_splitmix(lay.buf.ptr + 3 * lay.frag_stride, lay.stripe_stride, lay.frag_stride, 1, F, S, 0,
                                     0x5EED, st.handle), "fill")
    locate()
    st.synchronize()
    got = words.download().view("uint32")
    assert (got[:S] == 0xF << k).all() and (got[S:] == 1 << 3).all(), "every stripe must name fragment 3"
    for _ in range(reps):
        ms["check_dirty"].append(timed(st, check, n))
        ms["locate_dirty"].append(timed(st, locate, n))
    out = {"k": k, "m": m, "fragment_bytes": F, "stripes": S, "algorithmic_bytes": algo,
           "fused_launches_per_call": fused_launches}
    out.update({name: series(v, algo) for name, v in ms.items()})
    c, l = out["check_clean"], out["locate_clean"]
    out["clean_locate_minus_check_ms"] = round(l["mean_ms"] - c["mean_ms"], 4)
    out["clean_within_check_spread"] = bool(l["mean_ms"] <= c["max_ms"])
    out["dirty_locate_over_clean_locate"] = round(out["locate_dirty"]["mean_ms"] / l["mean_ms"], 4)
    out["objects"] = {"10,4": object_figures(d, 10, 4), "20,8": object_figures(d, 20, 8)}
    lay.buf.free()
    words.free()
    return out


def run_pairs(d, st, reps, n, locate_only=False):
    """C3, ecamd_rs_locate against ecamd_rs_locate_pairs, alternating: (a) a clean batch, (b) one stripe
    of 256 with two damaged words, (c) fragments 3 and 12 of every stripe rewritten.  A tree from before
    the pair stage (--tree) has ecamd_rs_locate alone: its rows are the yardstick of (a)."""
    k, m, F, S = 10, 4, 1 << 20, 256
    has_pairs = hasattr(d, "ecamd_rs_locate_pairs") and not locate_only
    lay = D.Layout.alloc(k + m, F, S)
    words = D.DeviceBuffer(12 * S)
    checked = _lib.u32s([0])
    args = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, F, S)

    def locate():
        _lib.check(d.ecamd_rs_locate(k, m, None, *args, words.ptr, words.ptr + 4 * S, checked, st.handle), "rs_locate")

    def pairs():
        _lib.check(d.ecamd_rs_locate_pairs(k, m, None, *args, words.ptr, words.ptr + 4 * S, words.ptr + 8 * S, checked,
                                           st.handle), "rs_locate_pairs")

    def fresh():
        lay.fill_splitmix(nfrags=k, stream=st)
        D.rs_encode(k, m, lay, stream=st)

    def result():
        (pairs if has_pairs else locate)()
        st.synchronize()
        got = words.download().view("uint32")
        return got[:S], got[S:2 * S], got[2 * S:]

    def rounds(ms, suffix):
        for _ in range(reps):
            ms["locate_" + suffix].append(timed(st, locate, n))
            if has_pairs:
                ms["pairs_" + suffix].append(timed(st, pairs, n))

    d.ecamd_tune(b"bitslice", 2)
    fresh()
    status, suspects, prs = result()
    assert not status.any() and not suspects.any() and (not has_pairs or not prs.any()), "encoded stripes must read clean"
    for _ in range(60):  # settle the clocks
        locate()
    st.synchronize()
    algo = S * (k + m) * F
    ms = {"%s_%s" % (op, case): [] for op in ("locate", "pairs") for case in ("clean", "one_dirty", "all_dirty")}
    rounds(ms, "clean")
    # (b) stripe 77: one word of fragment 2 and one of fragment 11
    for f, at in ((2, 123456), (11, 987654)):
        pos = 77 * lay.stripe_stride + f * lay.frag_stride + at
        two = lay.buf.download(2, pos)
        two[0] ^= 0x5A
        two[1] ^= 0x01
        lay.buf.upload(two, pos)
    status, suspects, prs = result()
    assert status[77] and not suspects.any() and sum(1 for x in status if x) == 1
    assert not has_pairs or (prs[77] == (1 << 2 | 1 << 11) and sum(1 for x in prs if x) == 1), "stripe 77 must name {2, 11}"
    rounds(ms, "one_dirty")
    # (c) fragments 3 and 12 of every stripe hold other data, so every word of every stripe needs the pair
    fresh()
    for f, seed in ((3, 0x5EED), (12, 0xBEEF)):
        _lib.check(d.ecamd_fill_splitmix(lay.buf.ptr + f * lay.frag_stride, lay.stripe_stride, lay.frag_stride, 1, F, S, 0,
                                         seed, st.handle), "fill")
    status, suspects, prs = result()
    assert status.all() and not suspects.any()
    assert not has_pairs or (prs == (1 << 3 | 1 << 12)).all(), "every stripe must name {3, 12}"
    rounds(ms, "all_dirty")
    out = {"k": k, "m": m, "fragment_bytes": F, "stripes": S, "algorithmic_bytes": algo, "pair_stage": has_pairs}
    out.update({name: series(v, algo) for name, v in ms.items() if v})
    if has_pairs:
        out["clean_pairs_minus_locate_ms"] = round(out["pairs_clean"]["mean_ms"] - out["locate_clean"]["mean_ms"], 4)
        out["all_dirty_pairs_over_locate"] = round(out["pairs_all_dirty"]["mean_ms"] / out["locate_all_dirty"]["mean_ms"], 3)
    lay.buf.free()
    words.free()
    return out


def run_correct(d, st, reps, n):
    """C3: (a) clean, events: locate_pairs / correct / correct with counts; (b), (c) wall clock around call
    plus synchronise, the damaged batch restored before every call: scrub_pairs / correct."""
    k, m, F, S = 10, 4, 1 << 20, 256
    has_correct = hasattr(d, "ecamd_rs_correct")
    lay = D.Layout.alloc(k + m, F, S)
    saved = D.DeviceBuffer(lay.buf.nbytes)
    words = D.DeviceBuffer(12 * S + 16)
    checked = _lib.u32s([0])
    host_counts = [_lib.C.c_int(0) for _ in range(4)]
    args = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, F, S)
    w = (words.ptr, words.ptr + 4 * S, words.ptr + 8 * S)

    def pairs():
        _lib.check(d.ecamd_rs_locate_pairs(k, m, None, *args, *w, checked, st.handle), "rs_locate_pairs")

    def correct(counts=False):
        _lib.check(d.ecamd_rs_correct(k, m, None, *args, *w, words.ptr + 12 * S if counts else None, checked, st.handle),
                   "rs_correct")

    def scrub():
        _lib.check(d.ecamd_rs_scrub_pairs(k, m, *args, *w, *[_lib.C.byref(c) for c in host_counts], st.handle), "rs_scrub_pairs")

    def fresh():
        lay.fill_splitmix(nfrags=k, stream=st)
        D.rs_encode(k, m, lay, stream=st)

    def keep():
        _lib.check(d.ecamd_memcpy_async(saved.ptr, lay.buf.ptr, lay.buf.nbytes, 2, st.handle), "keep")
        st.synchronize()

    def restore():
        _lib.check(d.ecamd_memcpy_async(lay.buf.ptr, saved.ptr, lay.buf.nbytes, 2, st.handle), "restore")
        st.synchronize()

    def wall(fn):
        """Mean ms of n calls, each on the restored damaged batch: clock around call plus synchronise."""
        total = 0.0
        for _ in range(n):
            restore()
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            total += time.perf_counter() - t0
        return total * 1e3 / n

    def repaired(what):
        st.synchronize()
        _lib.check(d.ecamd_rs_locate_pairs(k, m, None, *args, *w, checked, st.handle), "rs_locate_pairs")
        st.synchronize()
        assert not words.download(4 * S).any(), "%s must leave every stripe consistent" % what

    d.ecamd_tune(b"bitslice", 2)
    fresh()
    (correct if has_correct else pairs)()
    st.synchronize()
    assert not words.download(12 * S).any(), "encoded stripes must read clean"
    for _ in range(60):  # settle the clocks
        pairs()
    st.synchronize()
    algo = S * (k + m) * F
    ms = {}
    for _ in range(reps):
        ms.setdefault("pairs_clean", []).append(timed(st, pairs, n))
        if has_correct:
            ms.setdefault("correct_clean", []).append(timed(st, correct, n))
            ms.setdefault("correct_counts_clean", []).append(timed(st, lambda: correct(True), n))
    # (b) stripe 77: one word of fragment 2 and one of fragment 11
    for f, at in ((2, 123456), (11, 987654)):
        pos = 77 * lay.stripe_stride + f * lay.frag_stride + at
        two = lay.buf.download(2, pos)
        two[0] ^= 0x5A
        two[1] ^= 0x01
        lay.buf.upload(two, pos)
    keep()
    for suffix in ("one_dirty", "all_dirty"):
        if suffix == "all_dirty":
            # (c) fragments 3 and 12 of every stripe hold other data, so every word of every stripe needs the pair
            fresh()
            for f, seed in ((3, 0x5EED), (12, 0xBEEF)):
                _lib.check(d.ecamd_fill_splitmix(lay.buf.ptr + f * lay.frag_stride, lay.stripe_stride, lay.frag_stride, 1, F,
                                                 S, 0, seed, st.handle), "fill")
            keep()
        scrub()  # both paths once: results, and everything they allocate or compile outside the timing
        repaired("scrub_pairs")
        if has_correct:
            restore()
            correct(True)
            st.synchronize()
            got = words.download().view("uint32")
            want = (S - 1, 0, 1, 0) if suffix == "one_dirty" else (0, 0, S, 0)
            assert tuple(int(c) for c in got[3 * S:3 * S + 4]) == want, (suffix, got[3 * S:3 * S + 4])
            repaired("correct")
        for _ in range(reps):
            ms.setdefault("scrub_pairs_" + suffix, []).append(wall(scrub))
            if has_correct:
                ms.setdefault("correct_" + suffix, []).append(wall(correct))
    out = {"k": k, "m": m, "fragment_bytes": F, "stripes": S, "algorithmic_bytes": algo, "correct": has_correct,
           "clean_timer": "HIP events around %d calls" % n,
           "dirty_timer": "host wall clock around call plus stream synchronise, batch restored before each call"}
    out.update({name: series(v, algo) for name, v in ms.items()})
    if has_correct:
        out["clean_correct_minus_pairs_ms"] = round(out["correct_clean"]["mean_ms"] - out["pairs_clean"]["mean_ms"], 4)
        for suffix in ("one_dirty", "all_dirty"):
            out["%s_scrub_over_correct" % suffix] = round(out["scrub_pairs_" + suffix]["mean_ms"] /
                                                          out["correct_" + suffix]["mean_ms"], 3)
    lay.buf.free()
    saved.free()
    words.free()
    return out


XOR_FORMS = (("generic", 0, 0), ("fused_4k", 1, 256), ("fused_1k", 1, 64), ("fused_default", 1, 0))


def run_xor(d, st, k, m, hd, F, S, reps, n):
    """One flat XOR shape: (a) ecamd_xor_encode, then check and locate on the generic path and on each
    tile form of the fused kernel, alternating; then the same on an all-dirty batch.  A tree from before
    the fused kernel (--tree) has the generic path alone: its rows are (a) and (b)."""
    fused_tree = hasattr(d, "ecamd_xor_check_fused_launches")
    forms = XOR_FORMS if fused_tree else XOR_FORMS[:1]
    lay = D.Layout.alloc(k + m, F, S)
    lay.fill_splitmix(nfrags=k, stream=st)
    words = D.DeviceBuffer(8 * S)
    args = (k, m, hd, lay.buf.ptr, lay.stripe_stride, lay.frag_stride, F, S)

    def encode():
        D.xor_encode(k, m, hd, lay, stream=st)

    def check():
        _lib.check(d.ecamd_xor_check(*args, words.ptr, st.handle), "xor_check")

    def locate():
        _lib.check(d.ecamd_xor_locate(*args, words.ptr, words.ptr + 4 * S, st.handle), "xor_locate")

    def form(fused, threads):
        if not fused_tree:
            return
        d.ecamd_tune(b"xor_check_fused", fused)
        d.ecamd_tune(b"xor_check_threads", threads)

    def round_of(ms, suffix):
        for name, fused, threads in forms:
            form(fused, threads)
            count = (lambda: (d.ecamd_xor_check_fused_launches(), d.ecamd_xor_locate_fused_launches())) if fused_tree \
                else (lambda: (0, 0))
            c0, l0 = count()
            few = n if fused else max(2, n // 4)
            ms.setdefault("check_%s_%s" % (name, suffix), []).append(timed(st, check, few))
            ms.setdefault("locate_%s_%s" % (name, suffix), []).append(timed(st, locate, few))
            c1, l1 = count()
            assert (c1 > c0, l1 > l0) == (bool(fused), bool(fused)), (name, c1 - c0, l1 - l0)

    encode()
    for name, fused, threads in forms:  # every path once: results, and the scratch allocated outside the timing
        form(fused, threads)
        locate()
        st.synchronize()
        assert not words.download().any(), "encoded stripes must read clean (%s)" % name
    for _ in range(60):  # settle the clocks
        encode()
    st.synchronize()
    algo = S * (k + m) * F
    ms = {"encode": []}
    for _ in range(reps):
        ms["encode"].append(timed(st, encode, n))
        round_of(ms, "clean")
    # all-dirty: data fragment 1 of every stripe holds other data, so every word of every tile disagrees
    _lib.check(d.ecamd_fill_splitmix(lay.buf.ptr + lay.frag_stride, lay.stripe_stride, lay.frag_stride, 1, F, S, 0,
                                     0x5EED, st.handle), "fill")
    pb = (_lib.C.c_uint * m)()
    assert _lib.host().ecamd_xor_code_tables(k, m, hd, pb, None) == 0
    rows = sum(1 << p for p in range(m) if pb[p] >> 1 & 1)  # the parities that contain data fragment 1
    for name, fused, threads in forms:
        form(fused, threads)
        locate()
        st.synchronize()
        got = words.download().view("uint32")
        assert (got[:S] == rows << k).all() and (got[S:] == 1 << 1).all(), "every stripe must name fragment 1 (%s)" % name
    for _ in range(reps):
        round_of(ms, "dirty")
    form(-1, 0)
    out = {"k": k, "m": m, "hd": hd, "fragment_bytes": F, "stripes": S, "algorithmic_bytes": algo}
    out.update({name: series(v, algo) for name, v in ms.items()})
    enc = out["encode"]
    out["bar_ms"] = round(enc["mean_ms"] + enc["spread_ms"], 4)  # (a) plus the spread of its own repetitions
    for name in [f[0] for f in forms[1:]]:
        for op in ("check", "locate"):
            c = out["%s_%s_clean" % (op, name)]
            g = out["%s_generic_clean" % op]
            out["%s_%s_clean_within_bar" % (op, name)] = bool(c["mean_ms"] <= out["bar_ms"])
            out["%s_%s_clean_over_generic" % (op, name)] = round(c["mean_ms"] / g["mean_ms"], 4)
    lay.buf.free()
    words.free()
    return out


def run_xor_degraded(d, st, k, m, hd, F, S, missing, reps, n):
    """One flat XOR shape on clean data, default knobs: ecamd_xor_check on the full stripes against
    ecamd_xor_check_degraded with `missing` lost, alternating -- the same launches over one load group
    slot fewer per lost or uncovered fragment -- and the same pair for the locate."""
    lay = D.Layout.alloc(k + m, F, S)
    lay.fill_splitmix(nfrags=k, stream=st)
    words = D.DeviceBuffer(8 * S)
    where = (lay.buf.ptr, lay.stripe_stride, lay.frag_stride, F, S)
    lost = _lib.ints(list(missing) + [-1])
    covered = _lib.C.c_uint32(0)
    calls = {
        "check_full": lambda: _lib.check(d.ecamd_xor_check(k, m, hd, *where, words.ptr, st.handle), "xor_check"),
        "check_degraded": lambda: _lib.check(d.ecamd_xor_check_degraded(
            k, m, hd, lost, *where, words.ptr, _lib.C.byref(covered), st.handle), "xor_check_degraded"),
        "locate_full": lambda: _lib.check(d.ecamd_xor_locate(k, m, hd, *where, words.ptr, words.ptr + 4 * S, st.handle),
                                          "xor_locate"),
        "locate_degraded": lambda: _lib.check(d.ecamd_xor_locate_degraded(
            k, m, hd, lost, *where, words.ptr, words.ptr + 4 * S, _lib.C.byref(covered), st.handle), "xor_locate_degraded"),
    }
    D.xor_encode(k, m, hd, lay, stream=st)
    for name, call in calls.items():  # every path once: results, launch counters, scratch outside the timing
        c0 = (d.ecamd_xor_check_fused_launches(), d.ecamd_xor_locate_fused_launches())
        call()
        st.synchronize()
        c1 = (d.ecamd_xor_check_fused_launches(), d.ecamd_xor_locate_fused_launches())
        assert (c1[0] > c0[0], c1[1] > c0[1]) == (name.startswith("check"), name.startswith("locate")), (name, c0, c1)
        assert not words.download().any(), "encoded stripes must read clean (%s)" % name
    for _ in range(60):  # settle the clocks
        D.xor_encode(k, m, hd, lay, stream=st)
    st.synchronize()
    ms = {}
    for _ in range(reps):
        for name, call in calls.items():
            ms.setdefault(name, []).append(timed(st, call, n))
    participants = bin(covered.value).count("1")
    out = {"k": k, "m": m, "hd": hd, "fragment_bytes": F, "stripes": S, "missing": list(missing),
           "covered_mask": covered.value, "fragments_loaded_full": k + m, "fragments_loaded_degraded": participants,
           "load_groups_full": (k + m + 3) // 4, "load_groups_degraded": (participants + 3) // 4}
    out.update({name: series(v, S * (k + m if name.endswith("full") else participants) * F) for name, v in ms.items()})
    for op in ("check", "locate"):
        full, deg = out[op + "_full"], out[op + "_degraded"]
        spread = max(full["spread_ms"], deg["spread_ms"])  # the run-to-run spread this run shows
        out[op + "_spread_ms"] = spread
        out[op + "_degraded_minus_full_ms"] = round(deg["mean_ms"] - full["mean_ms"], 4)
        out[op + "_degraded_within_spread_of_full"] = bool(deg["mean_ms"] <= full["mean_ms"] + spread)
    lay.buf.free()
    words.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--locate", action="store_true", help="measure ecamd_rs_locate at C3 instead")
    ap.add_argument("--xor", action="store_true", help="measure ecamd_xor_check / ecamd_xor_locate instead")
    ap.add_argument("--pairs", action="store_true", help="measure ecamd_rs_locate_pairs at C3 instead")
    ap.add_argument("--locate-only", action="store_true", help="with --pairs: time ecamd_rs_locate alone, as --tree PARENT does")
    ap.add_argument("--pairs-merge", default=None,
                    help="THIS,BEFORE,AFTER: --pairs documents of this commit and of two runs of the parent's tree")
    ap.add_argument("--correct", action="store_true", help="measure ecamd_rs_correct at C3 instead")
    ap.add_argument("--correct-merge", default=None,
                    help="THIS,BEFORE,AFTER: --correct documents of this commit and of two runs of the parent's tree")
    ap.add_argument("--added-launch-us", type=float, default=None,
                    help="with --correct-merge: traced duration of the launches ecamd_rs_correct adds on a clean batch")
    ap.add_argument("--xor-shapes", default="10,6,4,1048576,256;3,3,3,4096,131072",
                    help="k,m,hd,fragment bytes,stripes; ...")
    ap.add_argument("--missing", default=None,
                    help="with --xor: comma-separated lost fragments; time ecamd_xor_check_degraded / _locate_degraded "
                         "against the full-stripe calls on the first shape instead")
    ap.add_argument("--tree", default=None, help="run against the package and libraries of another built checkout")
    ap.add_argument("--parent-check-ms", type=float, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--per-cu", default="", help="comma-separated check_per_cu values to A/B at C3")
    ap.add_argument("--parent-encode-ms", type=float, default=None)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 alternating repetitions"
    if a.pairs_merge:
        # this commit's --pairs document with the yardstick of (a): the parent commit's clean
        # ecamd_rs_locate of the same session, run before and after it (--pairs --tree PARENT)
        docs = []
        for path in a.pairs_merge.split(","):
            with open(path) as f:
                docs.append(json.load(f))
        doc, before, after = docs
        b, c = before["c3"]["locate_clean"]["mean_ms"], after["c3"]["locate_clean"]["mean_ms"]
        mean = doc["c3"]["pairs_clean"]["mean_ms"]
        doc["yardstick"] = {"parent_locate_clean_ms": [b, c], "margin_ms": round(abs(b - c), 4), "pairs_clean_mean_ms": mean,
                            "within": bool(mean <= max(b, c) + abs(b - c)),
                            "parent_before": before["c3"], "parent_after": after["c3"]}
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    if a.correct_merge:
        # the bar of (a): the parent's larger clean ecamd_rs_locate_pairs mean of the same session (run before
        # and after this commit, --correct --tree PARENT), plus the spread between those two runs, plus the
        # traced duration of the added launches
        docs = []
        for path in a.correct_merge.split(","):
            with open(path) as f:
                docs.append(json.load(f))
        doc, before, after = docs
        b, c = before["c3"]["pairs_clean"]["mean_ms"], after["c3"]["pairs_clean"]["mean_ms"]
        added = (a.added_launch_us or 0.0) / 1e3
        mean = doc["c3"]["correct_clean"]["mean_ms"]
        bar = max(b, c) + abs(b - c) + added
        doc["yardstick"] = {"parent_pairs_clean_ms": [b, c], "parent_spread_ms": round(abs(b - c), 4),
                            "added_launch_ms": round(added, 4), "bar_ms": round(bar, 4), "correct_clean_mean_ms": mean,
                            "within": bool(mean <= bar), "over_by_ms": round(max(0.0, mean - bar), 4),
                            "parent_before": before["c3"], "parent_after": after["c3"]}
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    d = _lib.dev()
    st = D.Stream()
    per_cu = [int(x) for x in a.per_cu.split(",") if x.strip()]
    if a.xor and a.missing:
        k, m, hd, F, S = (int(x) for x in a.xor_shapes.split(";")[0].split(","))
        missing = [int(x) for x in a.missing.split(",")]
        doc = {"tool": "tools/check_bench.py --xor --missing " + a.missing, "reps": a.reps, "calls_per_rep": a.n,
               "shape": run_xor_degraded(d, st, k, m, hd, F, S, missing, a.reps, a.n)}
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    if a.xor:
        doc = {"tool": "tools/check_bench.py --xor", "fused_kernel": hasattr(d, "ecamd_xor_check_fused_launches"), "reps": a.reps, "calls_per_rep": a.n, "shapes": []}
        for shape in a.xor_shapes.split(";"):
            k, m, hd, F, S = (int(x) for x in shape.split(","))
            doc["shapes"].append(run_xor(d, st, k, m, hd, F, S, a.reps, a.n))
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    if a.correct:
        doc = {"tool": "tools/check_bench.py --correct", "reps": a.reps, "calls_per_rep": a.n,
               "c3": run_correct(d, st, a.reps, a.n)}
        d.ecamd_tune(b"bitslice", 1)
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    if a.pairs:
        doc = {"tool": "tools/check_bench.py --pairs", "reps": a.reps, "calls_per_rep": a.n,
               "c3": run_pairs(d, st, a.reps, a.n, a.locate_only)}
        d.ecamd_tune(b"bitslice", 1)
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    if a.locate:
        doc = {"tool": "tools/check_bench.py --locate", "reps": a.reps, "calls_per_rep": a.n,
               "c3": run_locate(d, st, a.reps, a.n)}
        if a.parent_check_ms is not None:
            doc["yardstick"] = {"parent_check_fused_ms": a.parent_check_ms}
        d.ecamd_tune(b"bitslice", 1)
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    doc = {"tool": "tools/check_bench.py", "reps": a.reps, "calls_per_rep": a.n,
           "c3": run(d, st, 10, 4, 1 << 20, 256, a.reps, a.n, True, per_cu)}
    if not a.no_c5:
        doc["c5"] = run(d, st, 20, 8, 4 << 20, 32, a.reps, max(4, a.n // 2), False, [])
    if a.parent_encode_ms is not None:
        enc = doc["c3"]["encode"]
        chk = doc["c3"]["check_fused"]["mean_ms"]
        doc["yardstick"] = {"parent_encode_pass_ms": a.parent_encode_ms, "margin_ms": enc["spread_ms"],
                            "check_fused_mean_ms": chk,
                            "within": bool(chk <= a.parent_encode_ms + enc["spread_ms"])}
    d.ecamd_tune(b"bitslice", 1)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
