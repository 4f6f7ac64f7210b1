#!/usr/bin/env python3
"""ecamd_xor_decode_masks against ecamd_xor_decode_multi -- flat_xor_hd (10,6,4), 1 MiB fragments, 256
stripes -- in one process, the same build, profiler off (development tool; DESIGN.md "Decode from device
masks").

Batches: (a) every stripe loses {0,1,2}; (b) one stripe of 256 loses one fragment; (c) 256 distinct seeded
patterns of 1-3 lost; (d) batch (c) as the FIRST call of a fresh child process (host wall clock around the
call and a stream synchronise; one child per call).  (a)-(c): after a warm-up of both calls, `--reps`
repetitions alternate the two calls, each timed by HIP events around `--calls` calls on one stream; the
spread is max - min over the repetitions.  The masks sit in device memory (that is the call's input);
decode_multi takes its lists from the host, as it must.  Only time is compared here (the bytes:
tests/test_gpu_xor_decode_masks.py): decode_multi reads a lost parity's own slot, which a repeated call
finds rebuilt and not zero-filled, and that changes its bytes, not its traffic.

  python tools/xor_decode_masks_bench.py --out profiles/xor_decode_masks.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, M, HD, F, S = 10, 6, 4, 1 << 20, 256


def batches():
    import numpy as np
    rng = np.random.default_rng(1064)
    distinct = set()
    while len(distinct) < S:
        distinct.add(tuple(sorted(int(f) for f in rng.choice(K + M, size=int(rng.integers(1, HD)), replace=False))))
    return {"a_all_lose_012": [(0, 1, 2)] * S,
            "b_one_stripe_one_fragment": [()] * 100 + [(5,)] + [()] * (S - 101),
            "c_256_distinct_patterns": sorted(distinct)}


def algorithmic_bytes(pats):
    """Fragments the masks call reads and writes: |U| + n_out of every stripe with a loss, U the union of the
    sources of the pattern's entry in the code's decode table (ecamd_xor_decode_masks_plan)."""
    import math
    import numpy as np
    from liberasurecode_amd import _lib
    entry = np.dtype([("n_out", "u1"), ("out", "u1", 3), ("src", "<u4", 3)])
    count = _lib.host().ecamd_xor_decode_masks_plan(K, M, HD, None, 0)
    raw = np.zeros(count * entry.itemsize, np.uint8)
    assert _lib.host().ecamd_xor_decode_masks_plan(K, M, HD, raw.ctypes.data_as(C.c_void_p), count) == count
    tab = raw.view(entry)
    total = 0
    for p in pats:
        if p:
            e = tab[sum(math.comb(K + M, i) for i in range(len(p))) + sum(math.comb(f, i + 1) for i, f in enumerate(p))]
            union = 0
            for r in range(int(e["n_out"])):
                union |= int(e["src"][r])
            total += (bin(union).count("1") + int(e["n_out"])) * F
    return total


def setup():
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from liberasurecode_amd import _lib
    from liberasurecode_amd import device as D
    d = _lib.dev()
    lay = D.Layout.alloc(K + M, F, S)
    st = D.Stream()
    lay.fill_splitmix(nfrags=K, stream=st)
    D.xor_encode(K, M, HD, lay, stream=st)
    st.synchronize()
    words = D.DeviceBuffer(4 * S * 2 + 16)

    def masks_call(pats):
        masks = np.array([sum(1 << f for f in p) for p in pats], np.uint32)
        words.upload(masks)
        return lambda: _lib.check(d.ecamd_xor_decode_masks(K, M, HD, words.ptr, 1, lay.buf.ptr, lay.stripe_stride, lay.frag_stride,
                                                           F, S, words.ptr + 4 * S, words.ptr + 8 * S, st.handle), "xor_decode_masks")

    def multi_call(pats):
        return lambda: D.xor_decode_multi(K, M, HD, pats, lay, stream=st)

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
        for fn in fns.values():  # warm-up: code objects, the table, decode_multi's maps
            for _ in range(3):
                fn()
        st.synchronize()
        x0, m0 = d.ecamd_xor_stream_launches(), d.ecamd_xor_decode_masks_launches()
        ms = {key: [] for key in fns}
        for _ in range(reps):
            for key, fn in fns.items():
                a.record(st)
                for _ in range(calls):
                    fn()
                b.record(st)
                st.synchronize()
                ms[key].append(a.elapsed_ms(b) / calls)
        nbytes = algorithmic_bytes(pats)
        out[name] = {"distinct_patterns": len({p for p in pats if p}), "stripes_with_a_loss": sum(1 for p in pats if p),
                     "algorithmic_bytes": nbytes,
                     "xor_stream_launches_per_multi_call": (d.ecamd_xor_stream_launches() - x0) / (reps * calls),
                     "data_launches_per_masks_call": (d.ecamd_xor_decode_masks_launches() - m0) / (reps * calls),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if args.reps < 5:
        raise SystemExit("at least five repetitions")
    doc = {"tool": "tools/xor_decode_masks_bench.py", "reps": args.reps, "calls_per_rep": args.calls,
           "timer": "HIP events around calls_per_rep calls on one stream, the two calls alternating",
           "shape": {"k": K, "m": M, "hd": HD, "fragment_bytes": F, "stripes": S}}
    doc["shape"].update(measure(args.reps, args.calls))
    doc["shape"]["d_first_call_of_a_fresh_process"] = fresh(args.reps)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
