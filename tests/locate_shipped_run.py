"""Child process of tests/test_gpu_locate.py: one fresh process, knob "bitslice" at its default (1: never
waits for a compile), an empty $ECAMD_JIT_CACHE.  Reports whether the FIRST ecamd_rs_locate of RS(10,4)
-- full stripe, and with fragment 5 missing -- ran the fused kernel (ecamd_locate_fused_launches),
whether clean stripes read clean and a flipped byte of an input fragment is located, and how many code
objects the cache directory holds afterwards (none: the kernels came from lib/jit/, nothing was
compiled)."""
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
from liberasurecode_amd import _lib  # noqa: E402
from liberasurecode_amd import device as D  # noqa: E402


def main():
    d = _lib.dev()
    k, m, bs, S = 10, 4, 2 * 4096 + 48, 3
    full = np.empty((S, k + m, bs), np.uint8)
    for s in range(S):
        full[s, :k] = stripe_fragments(60 + s, k, bs)
        full[s, k:] = orc.encode(k, m, full[s, :k])
    out = {}
    lay = D.Layout.alloc(k + m, bs, S)
    for name, miss in (("full", []), ("lost5", [5])):
        held = full.copy()
        held[:, miss] = 0x5A
        lay.upload_stripes(held)
        n0 = d.ecamd_locate_fused_launches()
        status, suspects, _ = D.rs_locate(k, m, lay, miss)
        out[name + "_fused_launches"] = d.ecamd_locate_fused_launches() - n0
        out[name + "_clean"] = not status.any() and not suspects.any()
        held[1, 7, 4096 + 100] ^= 0x01  # fragment 7 is an input in both patterns
        lay.upload_stripes(held)
        status, suspects, _ = D.rs_locate(k, m, lay, miss)
        out[name + "_located"] = [int(x) for x in suspects] == [0, 1 << 7, 0] and bool(status[1])
    cache = os.environ["ECAMD_JIT_CACHE"]
    out["cache_objects"] = len([n for n in os.listdir(cache) if n.endswith(".co")])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
