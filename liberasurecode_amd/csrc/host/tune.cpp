// tune.cpp -- the table of ecamd_tune() knobs (tune_knobs.def), set-by-name and $ECAMD_TUNE.
#include "tune.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

namespace ecamd {

Tuning g_tune;

namespace {

// The normalising rules: (value asked for, the knob's default) -> value stored.
using Norm = std::optional<int>;

Norm raw(int v, int) { return v; }                  // 0 off, anything else on, or the launcher's reading
Norm on_off(int v, int) { return v != 0 ? 1 : 0; }
Norm positive(int v, int) { return v > 0 ? 1 : 0; }
template <int lo, int hi>
Norm clamp_to(int v, int)
{
    return std::max(lo, std::min(v, hi));
}
template <int lo, int hi>
Norm in_range(int v, int d)  // anything outside [lo, hi] restores the default
{
    return v >= lo && v <= hi ? v : d;
}
template <int... allowed>
Norm one_of(int v, int d)  // anything else restores the default
{
    return ((v == allowed) || ...) ? v : d;
}
template <int hi = INT_MAX>
Norm neg_default_max(int v, int d)  // < 0: the default
{
    return v < 0 ? d : std::min(v, hi);
}
Norm neg_default_on_off(int v, int d) { return v < 0 ? d : v != 0 ? 1 : 0; }
template <int hi>
Norm nonpos_default_max(int v, int d)  // <= 0: the default
{
    return v <= 0 ? d : std::min(v, hi);
}
Norm nonpos_default_1_2_4(int v, int d) { return v <= 0 ? d : v >= 4 ? 4 : v >= 2 ? 2 : 1; }
Norm step_0_2_4(int v, int) { return v >= 4 ? 4 : v >= 2 ? 2 : 0; }

}  // namespace

const TuneKnob kTuneKnobs[] = {
#define KNOB(name, def, ...) {#name, &Tuning::name, def, __VA_ARGS__},
#include "tune_knobs.def"
#undef KNOB
};
const size_t kTuneKnobCount = sizeof(kTuneKnobs) / sizeof(kTuneKnobs[0]);

TuneSet tune_set(Tuning& t, const char* key, int value)
{
    for (const TuneKnob& k : kTuneKnobs) {
        if (std::strcmp(k.name, key) != 0) continue;
        const std::optional<int> v = k.rule(value, k.def);
        if (v) t.*k.knob = *v;
        return {&k, v.has_value()};
    }
    return {nullptr, false};
}

void tune_from_env()
{
    const char* env = std::getenv("ECAMD_TUNE");
    if (!env) return;
    std::string all(env);
    size_t pos = 0;
    while (pos < all.size()) {
        size_t end = all.find(',', pos);
        if (end == std::string::npos) end = all.size();
        const std::string kv = all.substr(pos, end - pos);
        const size_t eq = kv.find('=');
        if (eq != std::string::npos && eq > 0)
            (void)tune_set(g_tune, kv.substr(0, eq).c_str(), std::atoi(kv.c_str() + eq + 1));
        pos = end + 1;
    }
}

}  // namespace ecamd
