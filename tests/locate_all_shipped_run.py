"""Child process of tests/test_gpu_locate_sweep.py: one fresh process, knob "bitslice" at its default (1:
never waits for a compile), an empty $ECAMD_JIT_CACHE.  For every pattern of prebuild.CHECK_OPS the FIRST
ecamd_rs_check, and for every pattern of prebuild.LOCATE_OPS the FIRST ecamd_rs_locate, on four stripes:
clean, an input fragment damaged, a checked fragment damaged, clean.  One JSON line per call: what the
prebuild answers for the pattern (asked against lib/jit/, where the object lies: nothing is compiled),
how often the fused kernel ran, whether the clean stripes read clean and whether each damaged fragment was
found (check: an input flags every checked fragment, a checked one itself; locate: the suspect is that
fragment); a last line counts the code objects in the cache directory (none: nothing was compiled)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402,F401

import numpy as np  # noqa: E402

import oracle_lib as orc  # noqa: E402
from ecdata import stripe_fragments  # noqa: E402
from liberasurecode_amd import _lib, prebuild  # noqa: E402
from liberasurecode_amd import device as D  # noqa: E402

S = 4


def main():
    d = _lib.dev()
    full = {}
    for k, m, _ in prebuild.CHECK_OPS + prebuild.LOCATE_OPS:
        if (k, m) not in full:
            tile = 4096 if m <= 4 else 16384
            bs = 2 * tile + 48
            a = np.empty((S, k + m, bs), np.uint8)
            for s in range(S):
                a[s, :k] = stripe_fragments(40 + s, k, bs)
                a[s, k:] = orc.encode(k, m, a[s, :k])
            full[(k, m)] = (tile, a)
    jit = prebuild.JIT_DIR.encode()
    for op, ops in (("check", prebuild.CHECK_OPS), ("locate", prebuild.LOCATE_OPS)):
        ask = d.ecamd_check_prebuild if op == "check" else d.ecamd_locate_prebuild
        count = d.ecamd_check_fused_launches if op == "check" else d.ecamd_locate_fused_launches
        for k, m, miss in ops:
            tile, a = full[(k, m)]
            avail = [f for f in range(k + m) if f not in miss]
            fin, fchk = avail[k // 2], avail[-1]  # an input and a checked fragment of this pattern
            held = a.copy()
            held[:, list(miss)] = 0x5A
            held[1, fin, tile + 100] ^= 0xC3  # both in whole tiles: the fused kernel decides
            held[2, fchk, 50] ^= 0x01
            lay = D.Layout.alloc(k + m, held.shape[2], S)
            lay.upload_stripes(held)
            arr = (C.c_int * (len(miss) + 1))(*(list(miss) + [-1]))
            out = {"op": op, "k": k, "m": m, "missing": list(miss),
                   "prebuilt": ask(k, m, C.cast(arr, C.c_void_p), b"gfx950", jit)}
            n0 = count()
            if op == "check":
                status, mask = D.rs_check(k, m, lay, miss)
                out["input_found"] = int(status[1]) == mask
                out["checked_found"] = int(status[2]) == 1 << fchk
            else:
                status, suspects, mask = D.rs_locate(k, m, lay, miss)
                out["input_found"] = int(status[1]) == mask and int(suspects[1]) == 1 << fin
                out["checked_found"] = int(status[2]) == 1 << fchk and int(suspects[2]) == 1 << fchk
                out["clean"] = not suspects[[0, 3]].any()
            out["fused_launches"] = count() - n0
            out["clean"] = bool(out.get("clean", True) and not status[[0, 3]].any() and mask == sum(1 << f for f in avail[k:]))
            lay.buf.free()
            print(json.dumps(out))
    cache = os.environ["ECAMD_JIT_CACHE"]
    print(json.dumps({"cache_objects": len([n for n in os.listdir(cache) if n.endswith(".co")])}))


if __name__ == "__main__":
    main()
