"""Child process of tests/test_gpu_check.py: one fresh process, knob "bitslice" at its default (1: never
waits for a compile), an empty $ECAMD_JIT_CACHE.  Reports whether the FIRST ecamd_rs_check of RS(10,4)
-- full stripe, and with fragment 5 missing -- ran the fused kernel (ecamd_check_fused_launches), whether
clean stripes read clean and a flipped parity byte is flagged, and how many code objects the cache
directory holds afterwards (none: the kernels came from lib/jit/, nothing was compiled)."""
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
        n0 = d.ecamd_check_fused_launches()
        status, _ = D.rs_check(k, m, lay, miss)
        out[name + "_fused_launches"] = d.ecamd_check_fused_launches() - n0
        out[name + "_clean"] = not status.any()
        held[1, k + 3, 100] ^= 0x01  # the last parity is checked in both patterns
        lay.upload_stripes(held)
        status, _ = D.rs_check(k, m, lay, miss)
        out[name + "_flagged"] = [int(x) for x in status] == [0, 1 << (k + 3), 0]
    cache = os.environ["ECAMD_JIT_CACHE"]
    out["cache_objects"] = len([n for n in os.listdir(cache) if n.endswith(".co")])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
