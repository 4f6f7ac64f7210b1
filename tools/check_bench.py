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
`--out`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--per-cu", default="", help="comma-separated check_per_cu values to A/B at C3")
    ap.add_argument("--parent-encode-ms", type=float, default=None)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 alternating repetitions"
    d = _lib.dev()
    st = D.Stream()
    per_cu = [int(x) for x in a.per_cu.split(",") if x.strip()]
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
