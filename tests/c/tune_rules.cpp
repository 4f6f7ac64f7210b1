// tune_rules.cpp -- stand-alone check of the ecamd_tune() knob table (csrc/host/tune.cpp, linked directly: no
// library, no GPU).  argv[1] is tests/golden/tune_rules.json: for every knob its default and, for a fixed list
// of values applied in order to a freshly constructed Tuning, ecamd_tune's return code and the value stored
// afterwards, as recorded from the hand-written setter this table replaced.
//   1. replay: the table gives the same return codes, stored values, defaults and set of names;
//   2. table integrity: unique names, one entry per Tuning member, listed default == constructed value;
//   3. $ECAMD_TUNE: valid entries applied, malformed and unknown ones skipped.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "tune.hpp"

using namespace ecamd;

namespace {

constexpr int kEinval = -22;  // ECAMD_EINVAL (include/ecamd.h)
int g_failures = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            g_failures++;                         \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
        }                                         \
    } while (0)

// The return code ecamd_tune() makes of a tune_set result (ecamd_runtime.hip).
int rc_of(const TuneSet& r) { return r.knob && r.stored ? 0 : kEinval; }

struct KnobRecord {
    int def = 0;
    std::vector<int> rc, stored;
};
struct Fixture {
    std::vector<int> values;
    int unknown_key_rc = 0, null_key_rc = 0;
    std::map<std::string, KnobRecord> knobs;
};

// Just enough JSON for the fixture: objects, arrays of integers, strings without escapes, integers.
struct Reader {
    const char* p;
    [[noreturn]] void die(const char* what)
    {
        std::fprintf(stderr, "fixture: expected %s at \"%.20s\"\n", what, p);
        std::exit(2);
    }
    void ws()
    {
        while (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t') p++;
    }
    bool eat(char c)
    {
        ws();
        if (*p != c) return false;
        p++;
        return true;
    }
    void expect(char c)
    {
        const char what[2] = {c, 0};
        if (!eat(c)) die(what);
    }
    std::string str()
    {
        expect('"');
        const char* e = std::strchr(p, '"');
        if (!e) die("closing quote");
        std::string s(p, e);
        p = e + 1;
        return s;
    }
    int num()
    {
        ws();
        char* e = nullptr;
        const long v = std::strtol(p, &e, 10);
        if (e == p) die("integer");
        p = e;
        return static_cast<int>(v);
    }
    std::vector<int> ints()
    {
        std::vector<int> v;
        expect('[');
        if (eat(']')) return v;
        do v.push_back(num());
        while (eat(','));
        expect(']');
        return v;
    }
    // calls member(key) for each "key": of an object, the callback consumes the value
    template <class F>
    void object(F member)
    {
        expect('{');
        if (eat('}')) return;
        do {
            const std::string key = str();
            expect(':');
            member(key);
        } while (eat(','));
        expect('}');
    }
};

Fixture load(const char* path)
{
    std::ifstream in(path);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    Fixture f;
    Reader r{text.c_str()};
    r.object([&](const std::string& key) {
        if (key == "values") f.values = r.ints();
        else if (key == "unknown_key_rc") f.unknown_key_rc = r.num();
        else if (key == "null_key_rc") f.null_key_rc = r.num();
        else if (key == "knobs")
            r.object([&](const std::string& name) {
                KnobRecord& k = f.knobs[name];
                r.object([&](const std::string& field) {
                    if (field == "default") k.def = r.num();
                    else if (field == "rc") k.rc = r.ints();
                    else if (field == "stored") k.stored = r.ints();
                    else r.die("default, rc or stored");
                });
            });
        else r.die("a known top-level key");
    });
    return f;
}

void test_table(const Fixture& f)
{
    CHECK(kTuneKnobCount == sizeof(Tuning) / sizeof(Knob), "table %zu entries, Tuning %zu members", kTuneKnobCount,
          sizeof(Tuning) / sizeof(Knob));
    CHECK(kTuneKnobCount == f.knobs.size(), "table %zu entries, fixture %zu knobs", kTuneKnobCount, f.knobs.size());
    std::set<std::string> names;
    std::set<const void*> members;
    Tuning fresh;
    for (size_t i = 0; i < kTuneKnobCount; i++) {
        const TuneKnob& k = kTuneKnobs[i];
        CHECK(names.insert(k.name).second, "%s listed twice", k.name);
        CHECK(members.insert(&(fresh.*k.knob)).second, "%s shares its member", k.name);
        CHECK(static_cast<int>(fresh.*k.knob) == k.def, "%s: listed default %d, constructed %d", k.name, k.def,
              static_cast<int>(fresh.*k.knob));
        CHECK(f.knobs.count(k.name) == 1, "%s is not in the fixture", k.name);
    }
    for (const auto& kv : f.knobs) CHECK(names.count(kv.first) == 1, "%s is not in the table", kv.first.c_str());
}

void test_replay(const Fixture& f)
{
    CHECK(f.values.size() == 45, "%zu values", f.values.size());
    for (size_t i = 0; i < kTuneKnobCount; i++) {
        const TuneKnob& k = kTuneKnobs[i];
        const auto it = f.knobs.find(k.name);
        if (it == f.knobs.end()) continue;  // reported by test_table
        const KnobRecord& want = it->second;
        CHECK(k.def == want.def, "%s: default %d, recorded %d", k.name, k.def, want.def);
        CHECK(want.rc.size() == f.values.size() && want.stored.size() == f.values.size(), "%s: short record", k.name);
        if (want.rc.size() != f.values.size() || want.stored.size() != f.values.size()) continue;
        {
            Tuning t;
            const TuneSet r = tune_set(t, k.name, k.def);
            CHECK(r.knob == &k && r.stored && static_cast<int>(t.*k.knob) == k.def,
                  "%s: the default %d is not a fixed point of its rule (stored %d)", k.name, k.def,
                  static_cast<int>(t.*k.knob));
        }
        Tuning t;
        for (size_t j = 0; j < f.values.size(); j++) {
            const TuneSet r = tune_set(t, k.name, f.values[j]);
            CHECK(r.knob == &k, "%s: looked up another entry", k.name);
            const int got = t.*k.knob;
            CHECK(rc_of(r) == want.rc[j] && got == want.stored[j], "%s = %d: rc %d stored %d, recorded rc %d stored %d",
                  k.name, f.values[j], rc_of(r), got, want.rc[j], want.stored[j]);
            if (r.knob && !r.stored) {
                CHECK(r.knob->must != nullptr, "%s rejects %d without a text", k.name, f.values[j]);
                char msg[256];
                std::snprintf(msg, sizeof(msg), "%s must be %s", k.name, r.knob->must ? r.knob->must : "");
                CHECK(std::strcmp(msg, "threads must be a multiple of 64 in [64,1024]") == 0, "error text \"%s\"", msg);
            }
        }
        for (size_t o = 0; o < kTuneKnobCount; o++)  // a knob's setter touches that knob alone
            if (o != i)
                CHECK(static_cast<int>(t.*kTuneKnobs[o].knob) == kTuneKnobs[o].def, "%s changed %s", k.name,
                      kTuneKnobs[o].name);
    }
    Tuning t;
    const TuneSet unknown = tune_set(t, "no_such_knob", 1);
    CHECK(unknown.knob == nullptr && !unknown.stored && rc_of(unknown) == f.unknown_key_rc, "unknown key: rc %d",
          rc_of(unknown));
    // a null key never reaches the table: ecamd_tune() answers it first, with the same code
    CHECK(f.null_key_rc == kEinval, "recorded null-key rc %d", f.null_key_rc);
}

// $ECAMD_TUNE = env, then tune_from_env() on g_tune at its defaults: exactly the knobs in `want` differ.
void env_case(const char* env, const std::map<std::string, int>& want)
{
    for (size_t i = 0; i < kTuneKnobCount; i++) g_tune.*kTuneKnobs[i].knob = kTuneKnobs[i].def;
    if (env) setenv("ECAMD_TUNE", env, 1);
    else unsetenv("ECAMD_TUNE");
    tune_from_env();
    for (size_t i = 0; i < kTuneKnobCount; i++) {
        const TuneKnob& k = kTuneKnobs[i];
        const auto it = want.find(k.name);
        const int expect = it == want.end() ? k.def : it->second;
        CHECK(static_cast<int>(g_tune.*k.knob) == expect, "ECAMD_TUNE=\"%s\": %s is %d, expected %d", env ? env : "(unset)",
              k.name, static_cast<int>(g_tune.*k.knob), expect);
    }
}

void test_env()
{
    env_case(nullptr, {});
    env_case("", {});
    env_case("bitslice=2,xor_threads=64", {{"bitslice", 2}, {"xor_threads", 64}});
    env_case("bitslice,xor_threads=128", {{"xor_threads", 128}});                 // an entry without '='
    env_case("=5,xor_threads=128", {{"xor_threads", 128}});                       // ... and one without a key
    env_case("bitslice=0,no_such_knob=3,xor_threads=256", {{"bitslice", 0}, {"xor_threads", 256}});
    env_case("bitslice=2,", {{"bitslice", 2}});                                   // trailing comma
    env_case("threads=100,bs_copy_per_cu=-1", {});  // a rejected value and a rule that restores the default
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s tests/golden/tune_rules.json\n", argv[0]);
        return 2;
    }
    const Fixture f = load(argv[1]);
    test_table(f);
    test_replay(f);
    test_env();
    if (g_failures) {
        std::fprintf(stderr, "tune_rules: %d failures\n", g_failures);
        return 1;
    }
    std::printf("tune_rules: ok (%zu knobs x %zu values)\n", kTuneKnobCount, f.values.size());
    return 0;
}
