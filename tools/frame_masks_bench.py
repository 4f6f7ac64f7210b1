#!/usr/bin/env python3
"""ecamd_frame_reconstruct_masks at the framed C3 shape -- (10,4), 10 MiB objects (1 MiB payloads), 256
stripes, CRC32 checksums, 128-byte-aligned slots -- in one process, the same build, profiler off
(development tool; DESIGN.md "Whole fragments from device masks").

Batches: (a) every stripe loses {0,1,2,3}; (b) one stripe of 256 loses one fragment; (c) 256 distinct
seeded patterns of 1-4 lost.  Each batch is measured against
  decode_masks      ecamd_rs_decode_masks alone on the same masks, at the payloads: the difference is what
                    the stamp stage costs (its algorithmic traffic: the rebuilt payloads read once, plus 80
                    bytes each);
  reconstruct_loop  what a caller must do without the call: ecamd_frame_reconstruct once per (pattern,
                    destination), on the sub-batch of stripes that share the pattern.
After a warm-up of all three, `--reps` repetitions alternate them, each timed by HIP events around
`--calls` calls on one stream; the spread is max - min over the repetitions.  A rebuild is idempotent -- the
lost slots are outputs only -- so nothing is restored between calls.

  python tools/frame_masks_bench.py --out profiles/frame_masks_c3.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, M, S = 10, 4, 256
OBJ = 10 << 20
HEADER = 80


def batches():
    import numpy as np
    rng = np.random.default_rng(1004)
    distinct = set()
    while len(distinct) < S:
        distinct.add(tuple(sorted(int(f) for f in rng.choice(K + M, size=int(rng.integers(1, M + 1)), replace=False))))
    return {"a_all_lose_0123": [(0, 1, 2, 3)] * S,
            "b_one_stripe_one_fragment": [()] * 100 + [(5,)] + [()] * (S - 101),
            "c_256_distinct_patterns": sorted(distinct)}


def runs_of(pats):
    """(first stripe, stripes, pattern) of every run of consecutive stripes that lost the same fragments."""
    out, s = [], 0
    while s < len(pats):
        e = s
        while e < len(pats) and pats[e] == pats[s]:
            e += 1
        if pats[s]:
            out.append((s, e - s, pats[s]))
        s = e
    return out


def setup():
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    from liberasurecode_amd import _lib
    from liberasurecode_amd import device as D
    from liberasurecode_amd import frame as F
    d = _lib.dev()
    fb = F.FrameBatch(F.RS_VAND, K, M, OBJ, S, checksum=F.CHKSUM_CRC32, align=128)
    st = D.Stream()
    d_obj = D.DeviceBuffer(fb.obj_stride * S)
    D.Layout(d_obj, 1, OBJ, S, fb.obj_stride, fb.obj_stride).fill_splitmix(stream=st)
    fb.encode(d_obj, stream=st)
    st.synchronize()
    d_obj.free()
    words = D.DeviceBuffer(4 * S * 2 + 16)

    def upload(pats):
        words.upload(np.array([sum(1 << f for f in p) for p in pats], np.uint32))

    def reconstruct_masks(pats):
        return lambda: _lib.check(d.ecamd_frame_reconstruct_masks(
            F.RS_VAND, K, M, 0, F.CHKSUM_CRC32, words.ptr, fb.base, fb.stripe_stride, fb.frag_stride, OBJ, S,
            words.ptr + 4 * S, words.ptr + 8 * S, st.handle), "frame_reconstruct_masks")

    def decode_masks(pats):
        return lambda: _lib.check(d.ecamd_rs_decode_masks(
            K, M, words.ptr, 1, fb.base + HEADER, fb.stripe_stride, fb.frag_stride, fb.blocksize, S, words.ptr + 4 * S,
            words.ptr + 8 * S, st.handle), "rs_decode_masks")

    def reconstruct_loop(pats):
        calls = [(_lib.ints(list(p) + [-1]), dest, fb.base + s0 * fb.stripe_stride, n)
                 for s0, n, p in runs_of(pats) for dest in p]

        def run():
            for missing, dest, base, n in calls:
                _lib.check(d.ecamd_frame_reconstruct(F.RS_VAND, K, M, 0, F.CHKSUM_CRC32, missing, dest, base, fb.stripe_stride,
                                                     fb.frag_stride, OBJ, n, st.handle), "frame_reconstruct")
        run.calls = len(calls)
        return run

    return d, D, fb, st, upload, {"reconstruct_masks": reconstruct_masks, "decode_masks": decode_masks,
                                  "reconstruct_loop": reconstruct_loop}


def spread(ms):
    mean = sum(ms) / len(ms)
    return {"ms": [round(v, 4) for v in ms], "mean_ms": round(mean, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def measure(reps, calls):
    d, D, fb, st, upload, makers = setup()
    a, b = D.Event(), D.Event()
    out = {}
    for name, pats in batches().items():
        upload(pats)
        fns = {key: make(pats) for key, make in makers.items()}
        # 256 patterns that are not shipped: with the default knob the per-pattern loop would queue hundreds of
        # compiles and change kernels under the timed window as they finish, so it is timed on its LDS-table
        # kernels -- the state a node is in while it meets new patterns (as tools/decode_masks_bench.py)
        knob = 0 if len(set(pats)) > 8 else 1
        d.ecamd_tune(b"bitslice", knob)
        for fn in fns.values():  # warm-up: code objects, maps, images, the scratch
            for _ in range(3):
                fn()
        st.synchronize()
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
        rebuilt = sum(len(p) for p in pats)
        row = {"reconstruct_loop_knob_bitslice": knob, "distinct_patterns": len({p for p in pats if p}),
               "stripes_with_a_loss": sum(1 for p in pats if p), "fragments_rebuilt": rebuilt,
               "reconstruct_loop_calls": fns["reconstruct_loop"].calls,
               "stamp_algorithmic_bytes": rebuilt * (fb.blocksize + HEADER),
               **{key: spread(v) for key, v in ms.items()}}
        stamp = row["reconstruct_masks"]["mean_ms"] - row["decode_masks"]["mean_ms"]
        row["stamp_stage_ms"] = round(stamp, 4)
        row["stamp_stage_tb_s"] = round(row["stamp_algorithmic_bytes"] / stamp / 1e9, 3) if stamp > 0 else None
        row["loop_over_masks"] = round(row["reconstruct_loop"]["mean_ms"] / row["reconstruct_masks"]["mean_ms"], 3)
        out[name] = row
        print(json.dumps({name: row}), flush=True)
    status, _ = fb.verify(stream=st)
    out["audit_after_all_zero"] = bool(not status.any())
    fb.buf.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least five repetitions")
    doc = {"tool": "tools/frame_masks_bench.py", "reps": args.reps, "calls_per_rep": args.calls,
           "timer": "HIP events around calls_per_rep calls on one stream, the three calls alternating",
           "c3_framed": {"k": K, "m": M, "object_bytes": OBJ, "stripes": S, "checksum": "crc32", "slot_align": 128}}
    doc["c3_framed"].update(measure(args.reps, args.calls))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
