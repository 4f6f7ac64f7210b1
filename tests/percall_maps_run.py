"""Child process of tests/test_gpu_percall_maps.py: ecamd_host_map_apply (the per-call path under
liberasurecode_rs_vand.so.1) called directly with ARBITRARY coefficient matrices, several of one shape on
the same caller buffers, every output compared byte for byte with tests/gfnp.apply_map (the numpy
GF(2^16) model: neither the product nor the C oracle).  Inputs are ecdata's splitmix streams, matrices are
drawn from the same generator.  The parent sets PERCALL_MAPS_MODE and the ECAMD_PERCALL_* environment (read
once per process); one JSON line comes out: {"ok", "bad": the first mismatches, "calls", "seconds", the
resident small server's counters before/after as deltas, ...}.  Mismatches are collected, not raised, so a
failing run still reports its counters.

Modes: A same shape, different matrix, shapes interleaved; B map-cache eviction and table-address reuse
(ECAMD_PERCALL_MAP_CACHE=2); B_crc the same through the frontend with CHKSUM_CRC32 (the fused checksum
form); C the default cache limit walked through once; fail an injected failed wait for a served request."""
import ctypes as C
import errno
import itertools
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's)

import gfnp  # noqa: E402
from ecdata import splitmix_bytes, stripe_fragments  # noqa: E402
from liberasurecode_amd import _lib  # noqa: E402

COUNTERS = (("posts", "ecamd_small_server_posts"), ("server_launches", "ecamd_small_server_launches"),
            ("rewrites", "ecamd_small_server_rewrites"), ("stale_hits", "ecamd_small_server_stale_hits"),
            ("crc_launches", "ecamd_small_crc_launches"))


def counters():
    d = _lib.dev()
    out = {}
    for key, name in COUNTERS:
        fn = getattr(d, name)
        fn.restype = C.c_longlong
        out[key] = fn()
    return out


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


def random_matrix(seed, R, K):
    """R x K coefficients from the full 16-bit range."""
    return splitmix_bytes(0xC0EFF ^ (seed << 12) ^ (R << 6) ^ K, 2 * R * K).view("<u2").astype(np.int64).reshape(R, K)


def edge_matrix(seed, R, K, idx):
    """random_matrix plus what generator-derived matrices never hold, as far as the shape has room: the
    elements 0, 1 and 0xFFFF, an all-zero row and two equal rows.  R >= 3: all of them in every matrix.
    R = 2: matrix 0 has two equal rows, matrix 1 a zero row.  R = 1: matrix 1 is the zero row.  K < 3: the
    elements that fit (1 and 0xFFFF first; the zero row supplies the 0), one fewer in matrix 2 so that the
    three stay distinct."""
    m = random_matrix(seed, R, K)
    vals = [1, 0xFFFF, 0][:K] if K > 1 else [(1, 0xFFFF)[idx & 1]]
    if K < 3 and idx == 2:
        vals = vals[:-1]
    for j, v in enumerate(vals):
        m[0, (j + idx) % K] = v
    if R >= 3:
        m[1 + idx % (R - 1)] = 0  # never row 0
        free = [r for r in range(1, R) if r != 1 + idx % (R - 1)]
        m[free[0]] = m[0]
    elif R == 2 and idx % 3 == 0:
        m[1] = m[0]
    elif idx % 3 == 1:
        m[R - 1] = 0
    return m


class Caller:
    """One set of caller buffers for a (R, K, bs) shape: K inputs (splitmix) and R outputs."""

    def __init__(self, R, K, bs, stripe):
        self.R, self.K, self.bs = R, K, bs
        self.ins = stripe_fragments(stripe, K, bs)
        self.outs = np.zeros((R, bs), dtype=np.uint8)
        self.inp = (C.c_void_p * K)(*[self.ins[j].ctypes.data for j in range(K)])
        self.outp = (C.c_void_p * R)(*[self.outs[r].ctypes.data for r in range(R)])
        self.fn = _lib.dev().ecamd_host_map_apply

    def want(self, m):
        return np.stack(gfnp.apply_map(m.tolist(), [self.ins[j] for j in range(self.K)]))

    def call(self, cm):
        self.outs[:] = 0xA5  # a call that wrote nothing does not pass on the previous call's bytes
        return self.fn(cm, self.R, self.K, self.inp, self.outp, self.bs)

    def check(self, cm, want, bad, tag):
        rc = self.call(cm)
        if rc != 0 or not np.array_equal(self.outs, want):
            rows = [r for r in range(self.R) if not np.array_equal(self.outs[r], want[r])]
            if len(bad) < 8:
                bad.append([tag, rc, rows])
            return False
        return True


def cints(m):
    return _lib.ints(int(v) for v in m.reshape(-1))


# ---- A: same shape, different matrix, no eviction ----
A_BS = (2, 1024, 30, 1026, 510, 1023, 512, 4098, 514, 16384, 16386)  # 2-byte lanes up to 512, then 4-byte
A_R = (1, 3, 5, 2, 4, 8)  # W = 2, 4, 8, 2, 4, 8: the server's kernel key changes with every group
A_K = (1, 2, 10, 20)
A_ORDER = (0, 1, 0, 2, 2, 1, 0, 0)


def a_groups():
    groups = []
    for bi, bs in enumerate(A_BS):
        for ri, R in enumerate(A_R):
            for t in range(2):  # two of the four K per (bs, R); every K meets every R and every bs
                groups.append((R, A_K[(bi + ri + 2 * t) % 4], bs))
    groups.insert(len(groups) // 2, (9, 3, 1024))  # two row passes: not one launch
    for bs in (2, 1024, 16384):  # one pass of 160 KiB of tables: no room to stage inputs beside them
        if (8, 20, bs) not in groups:
            groups.append((8, 20, bs))
    return groups


def served_shape(R, K, bs):
    """Whether the server takes the call (launch_small / server_post): one pass, its tables and the staged
    inputs of one workgroup within the LDS, at most 16 workgroups."""
    W = 2 if R <= 2 else 4 if R <= 4 else 8
    lane = 2 if (bs + 1) // 2 <= 256 else 4
    wgs = ((bs + lane - 1) // lane + 255) // 256
    return R <= 8 and K * 1024 * W + K * 256 * lane <= 159 * 1024 and wgs <= 16, W | lane << 4


def mode_a():
    bad, calls, posted, key_changes, last_key = [], 0, 0, 0, None
    unposted_bad = []
    groups = a_groups()
    t0 = time.time()
    c0 = counters()
    for gi, (R, K, bs) in enumerate(groups):
        cal = Caller(R, K, bs, stripe=100 + gi)
        mats = [edge_matrix(gi, R, K, i) for i in range(3)]
        assert len({m.tobytes() for m in mats}) == 3, (R, K, bs)
        cms = [cints(m) for m in mats]
        wants = [cal.want(m) for m in mats]
        served, key = served_shape(R, K, bs)
        if served and key != last_key:
            key_changes += last_key is not None
            last_key = key
        for n, i in enumerate(A_ORDER):
            p0 = counters()["posts"]
            cal.check(cms[i], wants[i], bad, ["A", R, K, bs, n, i])
            dp = counters()["posts"] - p0
            calls += 1
            posted += dp
            if (bs == 16386 or R == 9) and dp != 0:
                unposted_bad.append([R, K, bs, n, dp])
    out = delta(counters(), c0)
    out.update(ok=not bad and not unposted_bad, bad=bad, unposted_bad=unposted_bad[:8], calls=calls, groups=len(groups),
               posted=posted, key_changes=key_changes, seconds=round(time.time() - t0, 2))
    return out


# ---- B: eviction and address reuse ----
def mode_b():
    R, K, bs, nmat, cap = 4, 10, 1024, 64, 4096
    cal = Caller(R, K, bs, stripe=7)
    mats = [random_matrix(1000 + i, R, K) for i in range(nmat)]
    assert len({m.tobytes() for m in mats}) == nmat
    cms = [cints(m) for m in mats]
    wants = [cal.want(m) for m in mats]
    bad, calls, nbad, must_rewrite = [], 0, 0, 0
    slots, last = [None, None], 0  # the matrices the server's two slots hold, as server_post fills them
    t0 = time.time()
    c0 = counters()
    for n in range(cap):
        i = n % nmat
        nbad += not cal.check(cms[i], wants[i], bad, ["B", n, i])
        calls += 1
        if i in slots:
            last = slots.index(i)
        else:
            must_rewrite += 1
            last ^= 1
            slots[last] = i
        if counters()["stale_hits"] - c0["stale_hits"] >= 8:
            break
    out = delta(counters(), c0)
    out.update(ok=not bad, bad=bad, mismatched_calls=nbad, calls=calls, must_rewrite=must_rewrite,
               seconds=round(time.time() - t0, 2))
    return out


def mode_b_crc():
    """RS(10,4) with CHKSUM_CRC32 through the frontend, 20 KiB objects (2 KiB fragments: above the fused
    checksum's 16 KiB-of-fragments threshold), 16 distinct 4-loss patterns round-robin: a decode (4 x 10 map)
    and a reconstruct of the first lost fragment (1 x 10 map, the call the frontend arms the checksums for)
    per visit, every map evicted before its pattern comes round again."""
    import ec_api as E
    from test_gpu_frontend import payload_bytes, rs_expected
    k, m, size, rounds = 10, 4, 20480, 8
    desc = E.create(E.EC_BACKEND_LIBERASURECODE_RS_VAND, k, m, hd=m, ct=E.CHKSUM_CRC32)
    assert desc > 0, desc
    data = payload_bytes(size, 20480)
    want = rs_expected(k, m, data, E.CHKSUM_CRC32)
    rc, dp, pp, flen = E.encode(desc, data)
    assert rc == 0, rc
    frags = E.fragments(dp, k, flen) + E.fragments(pp, m, flen)
    E.lib().liberasurecode_encode_cleanup(desc, dp, pp)
    bad = [] if frags == want else [["B_crc", "encode"]]
    # every pattern loses data fragment p % 10 (the decode needs the codec) and three more
    pats = []
    for p, rest in zip(range(16), itertools.combinations(range(k + m - 1), 3)):
        lost = sorted({p % k} | set((p % k + 1 + r) % (k + m) for r in rest))
        assert len(lost) == 4 and lost not in pats, lost
        pats.append(lost)
    calls = 0
    t0 = time.time()
    c0 = counters()
    for rnd in range(rounds):
        for lost in pats:
            avail = [f for i, f in enumerate(frags) if i not in lost]
            rc, out = E.decode(desc, avail, flen, force=1)
            if (rc != 0 or out != data) and len(bad) < 8:
                bad.append(["B_crc", "decode", rnd, lost, rc])
            rc, rec = E.reconstruct(desc, avail, flen, lost[0])
            if (rc != 0 or rec != want[lost[0]]) and len(bad) < 8:
                bad.append(["B_crc", "reconstruct", rnd, lost, rc])
            calls += 2
    out = delta(counters(), c0)
    assert E.lib().liberasurecode_instance_destroy(desc) == 0
    out.update(ok=not bad, bad=bad, calls=calls, seconds=round(time.time() - t0, 2))
    return out


# ---- C: the default cache limit ----
def mode_c():
    bad, calls = [], 0
    t0 = time.time()
    c0 = counters()
    n1 = 4100
    cal = Caller(1, 2, 64, stripe=9)
    for i in range(n1):
        m = np.array([[i + 1, 0x9C3B]], dtype=np.int64)
        if i % 64 == 0 or i >= n1 - 3:
            cal.check(cints(m), cal.want(m), bad, ["C", i])
        elif cal.call(cints(m)) != 0 and len(bad) < 8:
            bad.append(["C", i, "rc"])
        calls += 1
    cal = Caller(4, 10, 1024, stripe=10)
    mats = [random_matrix(5000 + i, 4, 10) for i in range(2)]
    wants = [cal.want(m) for m in mats]
    for n in range(10):
        cal.check(cints(mats[n & 1]), wants[n & 1], bad, ["C", "alt", n])
        calls += 1
    out = delta(counters(), c0)
    out.update(ok=not bad, bad=bad, calls=calls, seconds=round(time.time() - t0, 2))
    return out


# ---- a failed wait for a served request ----
def mode_fail():
    import ec_api as E
    from test_gpu_frontend import payload_bytes
    d = _lib.dev()
    bad = []
    t0 = time.time()
    # through the frontend: -EIO and no fragments (as tests/test_gpu_errors.py for the staging site)
    k, m = 10, 4
    desc = E.create(E.EC_BACKEND_LIBERASURECODE_RS_VAND, k, m, hd=m, ct=E.CHKSUM_NONE)
    assert desc > 0, desc
    data = payload_bytes(4096 * k, 3)
    rc, dp, pp, flen = E.encode(desc, data)  # served (tests/test_gpu_percall_env.py pins that it is)
    assert rc == 0, rc
    first = E.fragments(dp, k, flen) + E.fragments(pp, m, flen)
    E.lib().liberasurecode_encode_cleanup(desc, dp, pp)
    assert d.ecamd_fault_inject(b"server_wait", 1) == 0
    rc, dp, pp, flen2 = E.encode(desc, data)
    frontend = {"rc": rc, "fragments": bool(dp) or bool(pp)}
    assert d.ecamd_fault_inject(b"server_wait", 0) == 0
    rc, dp, pp, flen2 = E.encode(desc, data)
    if rc == 0:
        if E.fragments(dp, k, flen) + E.fragments(pp, m, flen) != first:
            bad.append(["fail", "encode after the failure", "bytes"])
        E.lib().liberasurecode_encode_cleanup(desc, dp, pp)
    else:
        bad.append(["fail", "encode after the failure", rc])
    assert E.lib().liberasurecode_instance_destroy(desc) == 0
    # directly: two matrices cached in the server's two slots, then the failure
    cal = Caller(4, 10, 1024, stripe=11)
    mats = [random_matrix(7000 + i, 4, 10) for i in range(2)]
    cms = [cints(x) for x in mats]
    wants = [cal.want(x) for x in mats]
    for n in range(4):
        cal.check(cms[n & 1], wants[n & 1], bad, ["fail", "before", n])
    r_cached = counters()["rewrites"]
    cal.check(cms[0], wants[0], bad, ["fail", "cached", 0])
    cached_rewrites = counters()["rewrites"] - r_cached  # 0: the block was served from its slot
    d.ecamd_percall_reset()
    assert d.ecamd_fault_inject(b"server_wait", 1) == 0
    direct = {"rc": cal.call(cms[1]), "status": d.ecamd_percall_status()}
    assert d.ecamd_fault_inject(b"server_wait", 0) == 0
    d.ecamd_percall_reset()
    c0 = counters()
    first_rewrites = None
    for n in range(20):
        cal.check(cms[n & 1], wants[n & 1], bad, ["fail", "after", n])
        if n == 0:
            first_rewrites = counters()["rewrites"] - c0["rewrites"]
    out = delta(counters(), c0)
    out.update(ok=not bad, bad=bad, frontend=frontend, direct=direct, cached_rewrites=cached_rewrites,
               first_rewrites=first_rewrites, status_after=d.ecamd_percall_status(), eio=-errno.EIO,
               seconds=round(time.time() - t0, 2))
    return out


def main():
    mode = os.environ["PERCALL_MAPS_MODE"]
    out = {"A": mode_a, "B": mode_b, "B_crc": mode_b_crc, "C": mode_c, "fail": mode_fail}[mode]()
    print(json.dumps(dict(out, mode=mode)))


if __name__ == "__main__":
    main()
