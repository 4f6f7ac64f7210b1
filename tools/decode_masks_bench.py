#!/usr/bin/env python3
"""ecamd_rs_decode_masks against ecamd_rs_decode_multi at the C3 shape -- (10,4), 1 MiB fragments, 256
stripes -- in one process, the same build, profiler off (development tool; DESIGN.md "Decode from device
masks").

Batches: (a) every stripe loses {0,1,2,3}; (b) one stripe of 256 loses one fragment; (c) 256 distinct
seeded patterns of 1-4 lost; (d) batch (c) as the FIRST call of a fresh child process (host wall clock
around the call and a stream synchronise; one child per call).  (a)-(c): after a warm-up of both calls,
`--reps` repetitions alternate the two calls, each timed by HIP events around `--calls` calls on one
stream; the spread is max - min over the repetitions.  A decode is idempotent -- the lost slots are outputs
only -- so nothing is restored between calls.  The masks sit in device memory (that is the call's input);
decode_multi takes its lists from the host, as it must.

  python tools/decode_masks_bench.py --out profiles/decode_masks_c3.json
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/decode_masks_bench.py --trace
  python tools/decode_masks_bench.py --trace-merge OUT --out profiles/decode_masks_c3.json   (adds the kernel times)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, M, F, S = 10, 4, 1 << 20, 256
TRACE_CALLS = 5


def batches():
    import numpy as np
    rng = np.random.default_rng(1004)
    distinct = set()
    while len(distinct) < S:
        distinct.add(tuple(sorted(int(f) for f in rng.choice(K + M, size=int(rng.integers(1, M + 1)), replace=False))))
    return {"a_all_lose_0123": [(0, 1, 2, 3)] * S,
            "b_one_stripe_one_fragment": [()] * 100 + [(5,)] + [()] * (S - 101),
            "c_256_distinct_patterns": sorted(distinct)}


def algorithmic_bytes(pats):
    """Fragments a decode must read and write: k inputs and the lost fragments of every stripe with a loss."""
    return sum((K + len(p)) * F for p in pats if p)


def setup():
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from liberasurecode_amd import _lib
    from liberasurecode_amd import device as D
    d = _lib.dev()
    lay = D.Layout.alloc(K + M, F, S)
    st = D.Stream()
    lay.fill_splitmix(nfrags=K, stream=st)
    D.rs_encode(K, M, lay, stream=st)
    st.synchronize()
    words = D.DeviceBuffer(4 * S * 2 + 16)

    def masks_call(pats):
        masks = np.array([sum(1 << f for f in p) for p in pats], np.uint32)
        words.upload(masks)
        return lambda: _lib.check(d.ecamd_rs_decode_masks(K, M, words.ptr, 1, lay.buf.ptr, lay.stripe_stride, lay.frag_stride,
                                                          F, S, words.ptr + 4 * S, words.ptr + 8 * S, st.handle), "decode_masks")

    def multi_call(pats):
        return lambda: D.rs_decode_multi(K, M, pats, lay, stream=st)

    return d, D, lay, st, masks_call, multi_call


def spread(ms, nbytes):
    mean = sum(ms) / len(ms)
    return {"ms": [round(v, 4) for v in ms], "mean_ms": round(mean, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "tb_s": round(nbytes / mean / 1e9, 3), "frac_8tbs": round(nbytes / mean / 1e9 / 8.0, 4)}


def measure(reps, calls):
    d, D, lay, st, masks_call, multi_call = setup()
    a, b = D.Event(), D.Event()
    out = {}
    for name, pats in batches().items():
        fns = {"decode_masks": masks_call(pats), "decode_multi": multi_call(pats)}
        # 256 patterns that are not shipped: with the default knob decode_multi would queue 256 compiles (two
        # at a time, minutes in all) and change kernels under the timed window as they finish, so it is
        # timed on its LDS-table kernels -- the state a node is in while it meets new patterns.
        knob = 0 if len(set(pats)) > 8 else 1
        d.ecamd_tune(b"bitslice", knob)
        for fn in fns.values():  # warm-up: code objects, maps, the scratch
            for _ in range(3):
                fn()
        st.synchronize()
        bs0 = d.ecamd_bitslice_launches()
        ms = {key: [] for key in fns}
        for _ in range(reps):
            for key, fn in fns.items():
                a.record(st)
                for _ in range(calls):
                    fn()
                b.record(st)
                st.synchronize()
                ms[key].append(a.elapsed_ms(b) / calls)
        d.ecamd_tune(b"bitslice", 1)
        nbytes = algorithmic_bytes(pats)
        out[name] = {"decode_multi_knob_bitslice": knob, "distinct_patterns": len({p for p in pats if p}), "stripes_with_a_loss": sum(1 for p in pats if p),
                     "algorithmic_bytes": nbytes, "bitsliced_launches_in_window": int(d.ecamd_bitslice_launches() - bs0),
                     **{key: spread(v, nbytes) for key, v in ms.items()}}
        out[name]["multi_over_masks"] = round(out[name]["decode_multi"]["mean_ms"] / out[name]["decode_masks"]["mean_ms"], 3)
        print(json.dumps({name: out[name]}), flush=True)
    lay.buf.free()
    return out


def child(which):
    """Batch (c) as the first call of this process: wall clock around the call plus a stream synchronise."""
    d, D, lay, st, masks_call, multi_call = setup()
    pats = batches()["c_256_distinct_patterns"]
    fn = masks_call(pats) if which == "decode_masks" else multi_call(pats)
    st.synchronize()
    t0 = time.perf_counter()
    fn()
    st.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    fn()
    st.synchronize()
    second = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"child": which, "first_call_ms": round(first, 4), "second_call_ms": round(second, 4)}), flush=True)
    lay.buf.free()


def fresh(reps):
    out = {"decode_masks": [], "decode_multi": []}
    for _ in range(reps):
        for which in out:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], capture_output=True, text=True,
                               timeout=300, check=True)
            out[which].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"child"')][-1]))
    res = {"timer": "host wall clock around the call plus a stream synchronise; a fresh process per figure",
           "algorithmic_bytes": algorithmic_bytes(batches()["c_256_distinct_patterns"])}
    for which, rows in out.items():
        first = [r["first_call_ms"] for r in rows]
        res[which] = {"first_call_ms": first, "second_call_ms": [r["second_call_ms"] for r in rows],
                      "first_mean_ms": round(sum(first) / len(first), 4), "first_spread_ms": round(max(first) - min(first), 4)}
    res["multi_over_masks_first_call"] = round(res["decode_multi"]["first_mean_ms"] / res["decode_masks"]["first_mean_ms"], 3)
    print(json.dumps({"d_first_call_of_a_fresh_process": res}), flush=True)
    return res


def trace():
    """For a kernel trace (a run of its own): TRACE_CALLS calls of ecamd_rs_decode_masks per batch, in order."""
    d, D, lay, st, masks_call, _ = setup()
    for pats in batches().values():
        fn = masks_call(pats)
        for _ in range(TRACE_CALLS):
            fn()
        st.synchronize()
    lay.buf.free()


def trace_merge(outdir):
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    res = {"note": "rocprofv3 --kernel-trace, a run of its own: %d calls of ecamd_rs_decode_masks per batch" % TRACE_CALLS}
    for kernel in ("masks_plan_kernel", "decode_masks_kernel", "masks_counts_kernel"):
        us = [t for _, name, t in rows if kernel in name]
        if len(us) != TRACE_CALLS * 3:
            raise SystemExit("%s: %d dispatches in the trace, %d expected" % (kernel, len(us), TRACE_CALLS * 3))
        for i, name in enumerate(batches()):
            part = us[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]
            res.setdefault(name, {})[kernel + "_us"] = {"avg": round(sum(part) / len(part), 2), "min": round(min(part), 2),
                                                        "max": round(max(part), 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-merge", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.trace:
        return trace()
    if args.trace_merge:
        doc = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        doc["kernel_trace"] = trace_merge(args.trace_merge)
    else:
        if args.reps < 5:
            raise SystemExit("at least five repetitions")
        doc = {"tool": "tools/decode_masks_bench.py", "reps": args.reps, "calls_per_rep": args.calls,
               "timer": "HIP events around calls_per_rep calls on one stream, the two calls alternating",
               "c3": {"k": K, "m": M, "fragment_bytes": F, "stripes": S}}
        doc["c3"].update(measure(args.reps, args.calls))
        doc["c3"]["d_first_call_of_a_fresh_process"] = fresh(args.reps)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
