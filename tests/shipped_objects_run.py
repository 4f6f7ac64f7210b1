"""Child process of tests/test_gpu_shipped_objects.py: one fresh process, an empty $ECAMD_JIT_CACHE, knob
"bitslice" at its default (1: never waits for a compile), so only the code objects shipped in lib/jit/
can run bitsliced.  Runs every op of one slice (shipped_ops.slices) on the GPU and compares it with the
reference digests of tests/golden/rs_shipped.json; then the slice's (10,4) decode patterns 16 at a time
through one interleaved rs_decode_multi call; then, for a slice longer than the kernel cache, its first
ops again.  Prints one JSON line.

usage: shipped_objects_run.py SLICE"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import oracle_lib as orc  # noqa: E402
import shipped_ops as so  # noqa: E402
from ecdata import stripe_fragments  # noqa: E402
from liberasurecode_amd import _lib  # noqa: E402
from liberasurecode_amd import device as D  # noqa: E402

TABLES, BITSLICED = 0, 1
MULTI_RUN, MULTI_STRIPES = 16, 32
LRU_ENTRIES, LRU_RERUN = 256, 8
MAX_LISTED = 20


def first_difference(got, want):
    """(stripe, fragment, offset) of the first byte that differs, or None."""
    ne = np.argwhere(got != want)
    return [int(v) for v in ne[0]] if len(ne) else None


class Runner:
    def __init__(self):
        self.d = _lib.dev()
        self.layouts = {}
        self.bad = []
        self.bitsliced = 0

    def layout(self, n, bs, S):
        if (n, bs, S) not in self.layouts:
            self.layouts[n, bs, S] = D.Layout.alloc(n, bs, S)
        return self.layouts[n, bs, S]

    def fail(self, **what):
        if len(self.bad) < MAX_LISTED:
            self.bad.append(what)
        else:
            self.bad[-1]["more"] = self.bad[-1].get("more", 0) + 1

    def run_op(self, i, op, gold, stage):
        d = self.d
        k, m, miss, dest, rebuild = op
        bs = so.blocksize(op)
        assert bs == gold[1], (op, bs, gold[1])
        expect = so.expected_bitsliced(op)
        arr = _lib.ints(list(miss) + [-1]) if miss is not None else None
        form = d.ecamd_rs_kernel_form(k, m, arr, dest, rebuild, bs)
        if form != (BITSLICED if expect else TABLES):
            self.fail(op=op, stage=stage, form=form, expected_bitsliced=expect)
        full, erased = so.op_inputs(i, op, orc.encode)
        lay = self.layout(k + m, bs, so.S)
        lay.upload_stripes(erased)
        n0 = d.ecamd_bitslice_launches()
        if miss is None:
            D.rs_encode(k, m, lay)
        elif dest < 0:
            D.rs_decode(k, m, miss, lay, rebuild_parity=bool(rebuild))
        else:
            D.rs_reconstruct(k, m, miss, dest, lay)
        got = lay.download_stripes()
        ran = d.ecamd_bitslice_launches() - n0
        if (ran >= 1) != expect:
            self.fail(op=op, stage=stage, bitsliced_launches=ran, expected_bitsliced=expect)
        self.bitsliced += 1 if ran >= 1 else 0
        if so.digest(op, got) != gold[2]:
            want = so.run_host(op, erased, orc)
            outs = so.outputs(op)
            at = first_difference(got[:, outs], want[:, outs])
            if at:
                at[1] = outs[at[1]]
            self.fail(op=op, stage=stage, digest=so.digest(op, got), golden=gold[2],
                      oracle_digest=so.digest(op, want), first_difference_vs_oracle=at)
        rest = [f for f in range(k + m) if f not in so.outputs(op)]
        if not (got[:, rest] == erased[:, rest]).all():
            at = first_difference(got[:, rest], erased[:, rest])
            at[1] = rest[at[1]]
            self.fail(op=op, stage=stage, input_fragment_changed=at)

    def run_multi(self, run_index, run_ops):
        """One rs_decode_multi over 32 stripes of 16 interleaved patterns: the host's grouping by
        pattern and the kernels' stripe lists."""
        d = self.d
        k, m = 10, 4
        bs = 2 * so.TILE_WAVE + so.TAIL
        assert all(so.blocksize(op) == bs for op in run_ops)
        full = np.empty((MULTI_STRIPES, k + m, bs), np.uint8)
        for s in range(MULTI_STRIPES):
            full[s, :k] = stripe_fragments(500000 + run_index * MULTI_STRIPES + s, k, bs)
            full[s, k:] = orc.encode(k, m, full[s, :k])
        erased = full.copy()
        pats = [run_ops[s % MULTI_RUN][2] for s in range(MULTI_STRIPES)]
        for s, p in enumerate(pats):
            erased[s, p] = so.FILL
        want = erased.copy()
        for s, p in enumerate(pats):
            want[s] = so.run_host((k, m, p, -1, 1), erased[s:s + 1], orc)[0]
        lay = self.layout(k + m, bs, MULTI_STRIPES)
        lay.upload_stripes(erased)
        n0 = d.ecamd_bitslice_launches()
        D.rs_decode_multi(k, m, pats, lay)
        got = lay.download_stripes()
        ran = d.ecamd_bitslice_launches() - n0
        if ran < MULTI_RUN:
            self.fail(stage="multi", run=run_index, bitsliced_launches=ran)
        if not (got == want).all():
            at = first_difference(got, want)
            self.fail(stage="multi", run=run_index, pattern=pats[at[0]], first_difference_vs_oracle=at)


def main():
    name = sys.argv[1]
    ops = so.ops()
    gold = so.golden_for(ops)
    indices = so.slices(ops)[name]
    r = Runner()
    d = r.d
    assert D.available(), "no HIP device"
    d.ecamd_tune(b"small_chunks", 0)  # these short fragments are not for gf16_small_kernel
    t0 = time.perf_counter()
    for i in indices:
        r.run_op(i, ops[i], gold[i], "first")
    t_ops = time.perf_counter() - t0
    out = {"slice": name, "ops": len(indices), "bitsliced": r.bitsliced,
           "expected_bitsliced": sum(so.expected_bitsliced(ops[i]) for i in indices)}
    dec = [ops[i] for i in indices if so.is_decode_10_4(ops[i])]
    runs = [dec[p:p + MULTI_RUN] for p in range(0, len(dec) - MULTI_RUN + 1, MULTI_RUN)]
    for j, run_ops in enumerate(runs):
        r.run_multi(j, run_ops)
    out["multi_runs"] = len(runs)
    if len(indices) > LRU_ENTRIES:  # the first ops' kernels were evicted: they load again
        n = r.bitsliced
        for i in indices[:LRU_RERUN]:
            r.run_op(i, ops[i], gold[i], "again")
        out["rerun"] = LRU_RERUN
        out["rerun_bitsliced"] = r.bitsliced - n
    out["entries"] = d.ecamd_bitslice_entries()
    out["mismatches"] = r.bad
    out["seconds_ops"] = round(t_ops, 2)
    out["seconds"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
