"""The operations whose bitsliced kernels build() ships in lib/jit/ (liberasurecode_amd/prebuild.py),
their test inputs and their digests -- shared by tests/golden/make_shipped_golden.py (reference), the
CPU tests (oracle, networks) and tests/shipped_objects_run.py (GPU).

An op is prebuild's tuple (k, m, missing | None, dest, rebuild_parity): encode (missing None), decode
(dest < 0) or the single-destination reconstruct of `dest`.  Everything here is stated from the map's
shape and the documented defaults, never read back from the library under test."""
import hashlib
import json
import os

import numpy as np

from ecdata import stripe_fragments

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rs_shipped.json")

S = 3                     # stripes per op: the stripe stride matters
FILL = 0x5A               # what every missing slot holds before the operation
TAIL = 48                 # bytes past the last whole tile: handed over to the table kernels
TILE_WAVE = 4096          # one-wave tiles: row groups of up to 4 outputs
TILE = 16384              # 4-wave tiles: 5..8 outputs
NARROW_MIN_K = 8          # default of knob bs_narrow_min_k
N_DECODES_10_4 = 1470     # sum of C(14, r), r = 1..4


def ops():
    from liberasurecode_amd import prebuild
    out = [(k, m, list(miss) if miss is not None else None, dest, rebuild)
           for k, m, miss, dest, rebuild in prebuild.all_ops(full=True)]
    check_ops(out)
    return out


def is_decode_10_4(op):
    k, m, miss, dest, _ = op
    return (k, m) == (10, 4) and dest < 0 and bool(miss)


def check_ops(lst):
    """The list must keep every 1- to 4-loss pattern of RS(10,4): it cannot shrink unnoticed."""
    dec = [tuple(op[2]) for op in lst if is_decode_10_4(op)]
    assert len(dec) == N_DECODES_10_4 and len(set(dec)) == N_DECODES_10_4, len(dec)
    assert all(1 <= len(p) <= 4 and list(p) == sorted(set(p)) and 0 <= p[0] and p[-1] < 14 for p in dec)


def kind(op):
    return "encode" if op[2] is None else "decode" if op[3] < 0 else "reconstruct"


def outputs(op):
    """Fragment indices the operation writes, ascending."""
    k, m, miss, dest, _ = op
    if miss is None:
        return list(range(k, k + m))
    return sorted(miss) if dest < 0 else [dest]


def plan(op):
    """(inputs, coefficient rows R x K) of the op's fragment map from the host planner."""
    import ctypes as C

    from liberasurecode_amd import _lib
    k, m, miss, dest, rebuild = op
    h = _lib.host()
    G = (C.c_int * ((k + m) * k))()
    assert h.ecamd_rs_generator(k, m, G) == 0
    if miss is None:
        return list(range(k)), [[G[(k + r) * k + j] for j in range(k)] for r in range(m)]
    ml = _lib.ints(list(miss) + [-1])
    inputs = (C.c_int * (k + m))()
    n = C.c_int()
    if dest < 0:
        outs = (C.c_int * (k + m))()
        coeff = (C.c_int * ((k + m) * k))()
        assert h.ecamd_rs_decode_map(G, k, m, ml, rebuild, inputs, outs, coeff, C.byref(n)) == 0
        R = n.value
        assert sorted(outs[:R]) == outputs(op), (op, list(outs[:R]))
        # rows in ascending output order, as outputs() lists them
        order = sorted(range(R), key=lambda r: outs[r])
        return list(inputs[:k]), [[coeff[r * k + j] for j in range(k)] for r in order]
    coeff = (C.c_int * (k + m))()
    assert h.ecamd_rs_reconstruct_map(G, k, m, ml, dest, inputs, C.byref(n), coeff) == 0
    return list(inputs[:n.value]), [list(coeff[:n.value])]


_shapes = {}


def shape(op):
    """(R outputs, K inputs) of the op's map."""
    key = (op[0], op[1], tuple(op[2]) if op[2] is not None else None, op[3], op[4])
    if key not in _shapes:
        inputs, rows = plan(op)
        _shapes[key] = (len(rows), len(inputs))
    return _shapes[key]


def expected_bitsliced(op):
    """By the map's shape (R outputs over K inputs) under the default knobs: 3..8 outputs always,
    1..2 outputs when the map has at least bs_narrow_min_k inputs; the LDS tables otherwise."""
    R, K = shape(op)
    return 3 <= R <= 8 or (1 <= R <= 2 and K >= NARROW_MIN_K)


def blocksize(op):
    """Two whole tiles of the op's kernel form and a 48-byte tail."""
    R, _ = shape(op)
    return 2 * (TILE_WAVE if R <= 4 else TILE) + TAIL


def op_inputs(index, op, encode):
    """(full, erased): (S, k+m, bs) uint8 -- the whole stripes (data of seeds 1000 + 4*index + s,
    parity by `encode(k, m, data)`), and the same with every missing slot filled with FILL."""
    k, m, miss, _, _ = op
    bs = blocksize(op)
    full = np.empty((S, k + m, bs), np.uint8)
    for s in range(S):
        full[s, :k] = stripe_fragments(1000 + index * 4 + s, k, bs)
        full[s, k:] = encode(k, m, full[s, :k])
    erased = full.copy()
    if miss is None:
        erased[:, k:] = FILL
    else:
        erased[:, list(miss)] = FILL
    return full, erased


def digest(op, frags):
    """frags: (S, k+m, bs) after the operation.  SHA-256 over the outputs, stripe by stripe and in
    ascending fragment order; the first 32 hex characters."""
    h = hashlib.sha256()
    for s in range(frags.shape[0]):
        for f in outputs(op):
            h.update(np.ascontiguousarray(frags[s, f]).tobytes())
    return h.hexdigest()[:32]


def run_host(op, erased, codec):
    """The operation on host fragments through a codec with oracle_lib's encode / decode / reconstruct
    call shapes; returns the (S, k+m, bs) result."""
    k, m, miss, dest, rebuild = op
    out = erased.copy()
    for s in range(out.shape[0]):
        if miss is None:
            out[s, k:] = codec.encode(k, m, out[s, :k])
            continue
        frags = [np.ascontiguousarray(out[s, f]) for f in range(k + m)]
        if dest < 0:
            assert codec.decode(k, m, frags, miss, rebuild) == 0
        else:
            assert codec.reconstruct(k, m, frags, miss, dest) == 0
        out[s] = np.stack(frags)
    return out


def load_golden():
    """[(op, bs, digest)] in all_ops(full=True) order."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    return [((k, m, miss, dest, rebuild), bs, dg) for k, m, miss, dest, rebuild, bs, dg in doc["ops"]]


def golden_for(lst):
    """The golden rows of the op list, checked to describe exactly these ops."""
    gold = load_golden()
    assert [g[0] for g in gold] == [tuple(op) for op in lst], "rs_shipped.json is not of this op list"
    return gold


def slices(lst):
    """Op indices per GPU child process: A (everything that is not a 2..4-loss (10,4) decode), the 91
    2-loss, the 364 3-loss and the 1,001 4-loss decodes in three parts."""
    def losses(i):
        return len(lst[i][2]) if is_decode_10_4(lst[i]) else 0
    idx = range(len(lst))
    four = [i for i in idx if losses(i) == 4]
    third = (len(four) + 2) // 3
    out = {"A": [i for i in idx if losses(i) < 2],
           "loss2": [i for i in idx if losses(i) == 2],
           "loss3": [i for i in idx if losses(i) == 3]}
    for p in range(3):
        out[f"loss4_{p}"] = four[p * third:(p + 1) * third]
    assert sorted(sum(out.values(), [])) == list(idx)
    assert (len(out["loss2"]), len(out["loss3"]), len(four)) == (91, 364, 1001)
    return out
