#!/usr/bin/env python3
"""Where a launch of the one-wave bitsliced kernel spends its time (DESIGN.md §4 "Per-launch cost").

  timeline  the kernel's timeline form (ecamd_bitslice_timeline: every tile writes its start and end wall
            clock, XCC and hardware id) on C3 encode and decode {0,1,2,3}, 64 and 256 stripes, 7 and 8
            resident workgroups per CU.  Per launch: bytes per 10 us bin, the time for the rate to reach 95%
            of its plateau, the idle slot-time after the last tile is handed out, the gap between a tile's end
            and the next tile's start on a CU, and the launch's span against its event-timed cost in a
            back-to-back chain (the difference is what a launch costs outside its tiles).
  ab        knob settings against a base (default: write-through output stores against nt, knob
            bs_store_through): interleaved rounds of timed steps (one encode + one decode {0,1,2,3}, as
            bench.py's), one event pair around each round, 64 and 256 stripes.
  other     the same variants on other maps that take the same kernel form (mixed decode, 1- and 2-output
            maps, a 21-fragment tile).
  split     1,024 stripes as 1 / 2 / 4 launches (bs_tiles_per_slot 0 / 32 / 16).

usage: launch_timeline.py timeline|ab|other|split OUT.json [variant=key:value,key:value ...]
(the first variant given is the base the others are compared with)
The wall clock is s_memrealtime's: 100 MHz, one tick = 10 ns."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from liberasurecode_amd import _lib  # noqa: E402
from liberasurecode_amd import device as D  # noqa: E402

K, M, F = 10, 4, 1 << 20
TILE = 4096
TICK_US = 0.01
OPS = {"encode": None, "decode0123": [0, 1, 2, 3]}
LAUNCH_KNOBS = {"bs_store_through": -1, "bs_tiles_per_slot": -1, "bs_wave_per_cu": -1}


def tune(d, knobs):
    for k, v in {**LAUNCH_KNOBS, **knobs}.items():
        assert d.ecamd_tune(k.encode(), v) == 0, k


def run_op(lost, lay, st):
    if lost is None:
        D.rs_encode(K, M, lay, stream=st)
    else:
        D.rs_decode(K, M, lost, lay, stream=st)


def chain_us(lost, lay, st, n=20):
    """Event-timed cost per launch of n back-to-back launches."""
    a, b = D.Event(), D.Event()
    a.record(st)
    for _ in range(n):
        run_op(lost, lay, st)
    b.record(st)
    st.synchronize()
    return a.elapsed_ms(b) * 1e3 / n


def analyse(rec, nfrag_bytes, cap):
    """rec: (ntiles, 8) uint32 records of one launch."""
    start = (rec[:, 0].astype(np.int64) | (rec[:, 1].astype(np.int64) << 32))
    end = (rec[:, 2].astype(np.int64) | (rec[:, 3].astype(np.int64) << 32))
    assert (end >= start).all() and (rec[:, 4] == np.arange(len(rec))).all(), "records missing or torn"
    t0 = start.min()
    start, end = (start - t0) * TICK_US, (end - t0) * TICK_US
    span = float(end.max())
    xcc = rec[:, 5] & 15
    cu = (xcc.astype(np.int64) << 16) | (rec[:, 6] & 0xff00)  # XCC, SE, SH, CU of HW_ID
    nbins = int(span // 10) + 1
    bins = np.bincount((end // 10).astype(np.int64), minlength=nbins) * nfrag_bytes
    mid = bins[nbins // 4: max(nbins // 4 + 1, 3 * nbins // 4)]
    plateau = float(np.median(mid))
    ramp = next((10.0 * (i + 1) for i, b in enumerate(bins) if b >= 0.95 * plateau), None)
    last_handout = float(start.max())
    # per CU: what its slots idle between the last hand-out of the launch and the launch's end, and the gap
    # between the i-th tile to end and the (cap + i)-th to start there
    idle, gaps, per_cu = 0.0, [], []
    for c in np.unique(cu):
        sel = cu == c
        s_, e_ = np.sort(start[sel]), np.sort(end[sel])
        per_cu.append(int(sel.sum()))
        # slots in use there: the most tiles alive at once; each slot's last tile is among the last to end
        resident = int(max(((s_[:, None] >= start[sel][None, :]) & (s_[:, None] < end[sel][None, :])).sum(axis=1)))
        idle += float((span - np.maximum(e_[-resident:], last_handout)).sum())
        n = len(s_) - resident
        if n > 0:
            gaps.extend((s_[resident:] - e_[:n]).tolist())
    life = end - start
    return {
        "tiles": int(len(rec)), "span_us": round(span, 2), "bytes_per_10us_bin": [int(b) for b in bins],
        "plateau_gb_per_s": round(plateau / 10e-6 / 1e9, 1),
        "mean_gb_per_s": round(len(rec) * nfrag_bytes / (span * 1e-6) / 1e9, 1),
        "ramp_to_95pct_us": ramp, "last_handout_us": round(last_handout, 2),
        "tail_us": round(span - last_handout, 2),
        "idle_slot_us_after_last_handout": round(idle, 1), "cus_seen": int(len(per_cu)),
        "idle_per_slot_us": round(idle / max(1, len(per_cu) * cap), 2),
        "tile_life_us": {"median": round(float(np.median(life)), 2), "p95": round(float(np.percentile(life, 95)), 2),
                         "first_generation_median": round(float(np.median(life[start < 1.0])), 2)},
        "refill_gap_us": {"median": round(float(np.median(gaps)), 3), "mean": round(float(np.mean(gaps)), 3),
                          "p95": round(float(np.percentile(gaps, 95)), 3)} if gaps else None,
        "first_start_by_xcc_us": {int(x): round(float(start[xcc == x].min()), 2) for x in np.unique(xcc)},
        "tiles_per_cu": {"min": min(per_cu), "max": max(per_cu)},
    }


def timeline(out):
    d = _lib.dev()
    d.ecamd_tune(b"bitslice", 2)
    st = D.Stream()
    res = {"clock": "s_memrealtime, 100 MHz", "workload": "C3 k=10 m=4, 1 MiB fragments", "launches": []}
    for S in (64, 256):
        lay = D.Layout.alloc(K + M, F, S)
        lay.fill_splitmix(nfrags=K, stream=st)
        D.rs_encode(K, M, lay, stream=st)
        st.synchronize()
        ntiles = S * F // TILE
        buf = D.DeviceBuffer(ntiles * 32)
        for _ in range(60):  # settle the clocks (bench.py)
            run_op(None, lay, st)
        st.synchronize()
        for cap in (7, 8):
            for name, lost in OPS.items():
                tune(d, {"bs_wave_per_cu": cap})
                plain_us = statistics.median(chain_us(lost, lay, st) for _ in range(5))
                buf.zero()
                assert d.ecamd_bitslice_timeline(buf.ptr, ntiles) == 0
                form_us = statistics.median(chain_us(lost, lay, st) for _ in range(5))  # the last launch's records stay
                assert d.ecamd_bitslice_timeline(None, 0) == 0
                rec = buf.download().view(np.uint32).reshape(ntiles, 8)
                nfrag = K + (M if lost is None else len(lost))
                a = analyse(rec, nfrag * TILE, cap)
                a.update({"op": name, "stripes": S, "per_cu": cap, "plain_launch_us_in_chain": round(plain_us, 2),
                          "timeline_form_launch_us_in_chain": round(form_us, 2),
                          "outside_tiles_us": round(form_us - a["span_us"], 2)})
                res["launches"].append(a)
                print(json.dumps({k: v for k, v in a.items() if k != "bytes_per_10us_bin"}), flush=True)
        tune(d, {})
        buf.free()
        lay.buf.free()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def c3_step(lay, st):
    run_op(None, lay, st)
    run_op(OPS["decode0123"], lay, st)


def step_ms(step, lay, st, steps=20):
    a, b = D.Event(), D.Event()
    a.record(st)
    for _ in range(steps):
        step(lay, st)
    b.record(st)
    st.synchronize()
    return a.elapsed_ms(b) / steps


def ab(out, variants, sizes=(64, 256), rounds=7, shape=(K, M, F), step=c3_step, what="C3 step = encode + decode {0,1,2,3}"):
    d = _lib.dev()
    d.ecamd_tune(b"bitslice", 2)
    st = D.Stream()
    res = {"workload": what + ", ms per step, interleaved rounds", "sizes": {}}
    k, m, f = shape
    base_name = next(iter(variants))
    for S in sizes:
        lay = D.Layout.alloc(k + m, f, S)
        lay.fill_splitmix(nfrags=k, stream=st)
        D.rs_encode(k, m, lay, stream=st)
        st.synchronize()
        for knobs in variants.values():  # compile every form first
            tune(d, knobs)
            step_ms(step, lay, st, 2)
        for _ in range(60):
            step_ms(step, lay, st, 1)
        ms = {v: [] for v in variants}
        for _ in range(rounds):
            for v, knobs in variants.items():
                tune(d, knobs)
                step_ms(step, lay, st, 3)
                ms[v].append(round(step_ms(step, lay, st), 5))
        tune(d, {})
        base = statistics.median(ms[base_name])
        res["sizes"][S] = {v: {"ms": x, "median_ms": statistics.median(x), "vs_base": round(base / statistics.median(x), 4),
                               "knobs": variants[v]} for v, x in ms.items()}
        for v, r in res["sizes"][S].items():
            print(S, v, r["median_ms"], r["vs_base"], min(r["ms"]), max(r["ms"]), flush=True)
        lay.buf.free()
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return res


# other maps of the same kernel form: the mixed decode, 1- and 2-output maps, a 21-fragment tile (C5)
OTHER = {"c3_decode_0_5_10_13": ((10, 4, 1 << 20), 256, lambda lay, st: D.rs_decode(10, 4, [0, 5, 10, 13], lay, stream=st)),
         "c3_reconstruct_3": ((10, 4, 1 << 20), 256, lambda lay, st: D.rs_reconstruct(10, 4, [3], 3, lay, stream=st)),
         "c3_decode_0_11": ((10, 4, 1 << 20), 256, lambda lay, st: D.rs_decode(10, 4, [0, 11], lay, stream=st)),
         "c5_reconstruct_x8_d5": ((20, 8, 4 << 20), 32,
                                  lambda lay, st: D.rs_reconstruct(20, 8, list(range(8)), 5, lay, stream=st))}


AB_DEFAULT = {"nt": {"bs_store_through": 0}, "through": {"bs_store_through": 1}}
SPLIT = {"launches4": {"bs_tiles_per_slot": 16}, "launches2": {"bs_tiles_per_slot": 32}, "launches1": {"bs_tiles_per_slot": 0}}

if __name__ == "__main__":
    mode, out = sys.argv[1], sys.argv[2]
    given = {a.split("=")[0]: {kv.split(":")[0]: int(kv.split(":")[1]) for kv in a.split("=")[1].split(",") if kv}
             for a in sys.argv[3:]}
    assert D.available(), "no HIP device"
    if mode == "timeline":
        timeline(out)
    elif mode == "ab":
        ab(out, given or AB_DEFAULT)
    elif mode == "other":
        res = {name: ab(out, given or AB_DEFAULT, sizes=(S,), rounds=5, shape=shape, step=fn, what=name)
               for name, (shape, S, fn) in OTHER.items()}
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)
    elif mode == "split":
        ab(out, SPLIT, sizes=(1024,), rounds=5)
    else:
        raise SystemExit(__doc__)
