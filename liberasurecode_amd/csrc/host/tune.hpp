// tune.hpp -- the ecamd_tune() knobs: struct Tuning (one member per knob), the table of their names,
// defaults and normalising rules, set-by-name and the $ECAMD_TUNE parser.  The knobs themselves are
// listed once, in tune_knobs.def.  Plain C++17, linked into libecamd.so only.
#pragma once
#include <atomic>
#include <cstddef>
#include <optional>

namespace ecamd {

// Launch-geometry knobs (0 = automatic).  Set through ecamd_tune() for sweeps; defaults are the
// measured best on MI355X ("Tuning").
// A launch knob: written by ecamd_tune from any thread, read by launches on others (each launch
// reads each knob once; every setting gives bit-identical results, only the launch shape changes).
// gf16_small_kernel for launches up to 4096 chunks (64 KiB per fragment, one stripe):
// DESIGN.md §6 (per-call objects of a few KiB).
constexpr int kSmallChunksDefault = 4096;
constexpr int kMultiStreamsMax = 4;  // decode_multi fan-out: the caller's stream + 3 pool streams

struct Knob {
    std::atomic<int> v;
    explicit Knob(int x) : v(x) {}
    operator int() const { return v.load(std::memory_order_relaxed); }
    Knob& operator=(int x)
    {
        v.store(x, std::memory_order_relaxed);
        return *this;
    }
};

constexpr int kFrameCrcNibDefault = 0;
constexpr int kFrameCrcBsDefault = 1;
// 1-2-output maps of at least 8 inputs take the one-wave bitsliced kernel: C3 (k = 10) single
// reconstruct of a data / parity fragment 0.685 / 0.690 -> 0.750 / 0.774 of 8 TB/s, decode of 1 / 2
// lost 0.687 / 0.688 -> 0.770 / 0.750; C5 (k = 20) reconstruct 0.692 -> 0.806; C2 (k = 4) keeps its
// 8 KiB tables (0.80 against 0.70 bitsliced) (tools/bs_wave_ab.py c3ncap c5ncap2 c2n,
// profiles/r05_ab_ncap.log, r05_ab_narrow.log)
constexpr int kBsNarrowMinKDefault = 8;

// Defaults of the one-wave crc form's knobs (frame_crc_wave*).
struct CrcWaveDefaults {
    int w, pos, per, pf, big;
};
// 4 waves per workgroup, 2 position sets (68 KiB of LDS: 2 workgroups, 8 waves per CU), one tile per
// wave, the next input's 4 chunks prefetched: against the 16 KiB-tile crc variant in the same runs
// C3 0.687 -> 0.704, Swift segments 0.591 -> 0.638, C5 0.599 -> 0.674 (profiles/r05_ab_crcwave_c5b.log;
// 12 waves per CU, 1 or 4 position sets and longer runs per wave all lose: r05_ab_crcwave_*.log)
constexpr CrcWaveDefaults kCrcWave{4, 2, 1, 4, 0};

struct Tuning {
#define KNOB(name, def, ...) Knob name{def};
#include "tune_knobs.def"
#undef KNOB
};
extern Tuning g_tune;  // the process's knobs (local to libecamd.so: abi/ecamd.map)

// One knob of the table: rule(value, def) is the value ecamd_tune stores, or nothing for a value it
// rejects -- `must` then completes the error text "<name> must be <must>".
struct TuneKnob {
    const char* name;
    Knob Tuning::*knob;
    int def;
    std::optional<int> (*rule)(int value, int def);
    const char* must = nullptr;
};
extern const TuneKnob kTuneKnobs[];
extern const size_t kTuneKnobCount;

// Sets knob `key` of `t` to its rule's reading of `value`.  knob: null for an unknown key; stored:
// false when the rule rejected the value (the knob keeps what it held).
struct TuneSet {
    const TuneKnob* knob;
    bool stored;
};
TuneSet tune_set(Tuning& t, const char* key, int value);

// $ECAMD_TUNE="key=value,key=value": knobs applied once, before the first call touches a device --
// so a profiler or an A/B can run an unmodified command (bench.py) with other launch shapes.
void tune_from_env();

}  // namespace ecamd
