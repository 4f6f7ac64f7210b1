#!/usr/bin/env python3
"""Generate tests/golden/rs_shipped.json from the REFERENCE itself: one digest per operation whose
bitsliced kernel build() ships (tests/shipped_ops.py: prebuild.all_ops(full=True)).

Runs on the build machine only: `make -C oracle ref` compiles the reference's
liberasurecode_rs_vand.so.1 into oracle/_ref/, and this script drives it through ctypes (load_rs and
the call shapes of make_golden.py) on the inputs of shipped_ops.op_inputs -- splitmix64 data, the
reference's own parity, every missing slot filled with 0x5A.  The committed JSON holds only data:
per op [k, m, missing, dest, rebuild_parity, blocksize, digest].  Deterministic: two runs give the
same bytes."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import shipped_ops as so  # noqa: E402
from make_golden import Bufs, as_ip, gen_matrix, load_rs  # noqa: E402


class RefCodec:
    """liberasurecode_rs_vand_{encode,decode,reconstruct} behind oracle_lib's call shapes."""

    def __init__(self):
        self.lib = load_rs()
        self.G = {}

    def gen(self, k, m):
        if (k, m) not in self.G:
            self.G[k, m] = gen_matrix(self.lib, k, m)
        return as_ip(self.G[k, m])

    def encode(self, k, m, data):
        bs = data.shape[1]
        bufs = Bufs(list(data) + list(np.zeros((m, bs), np.uint8)))
        self.lib.liberasurecode_rs_vand_encode(self.gen(k, m), bufs.array(0, k), bufs.array(k, k + m), k, m, bs)
        return np.stack(bufs.arrs[k:])

    def decode(self, k, m, frags, missing, rebuild_parity=1):
        bufs = Bufs(frags)
        assert all(b is f for b, f in zip(bufs.arrs, frags))  # in place
        return self.lib.liberasurecode_rs_vand_decode(self.gen(k, m), bufs.array(0, k), bufs.array(k, k + m), k, m,
                                                      as_ip(list(missing) + [-1]), frags[0].shape[0], rebuild_parity)

    def reconstruct(self, k, m, frags, missing, dest):
        bufs = Bufs(frags)
        assert all(b is f for b, f in zip(bufs.arrs, frags))
        return self.lib.liberasurecode_rs_vand_reconstruct(self.gen(k, m), bufs.array(0, k), bufs.array(k, k + m), k,
                                                           m, as_ip(list(missing) + [-1]), dest, frags[0].shape[0])


def main():
    ref = RefCodec()
    rows = []
    for i, op in enumerate(so.ops()):
        _, erased = so.op_inputs(i, op, ref.encode)
        rows.append(list(op) + [so.blocksize(op), so.digest(op, so.run_host(op, erased, ref))])
    text = '{"stripes":%d,"fill":%d,"ops":[\n' % (so.S, so.FILL)
    text += ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n"
    with open(so.GOLDEN, "w") as f:
        f.write(text)
    print("rs_shipped.json:", len(rows), "ops,", len(text), "bytes")


if __name__ == "__main__":
    main()
