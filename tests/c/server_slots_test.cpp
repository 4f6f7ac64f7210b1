// The resident small server's slot decision (liberasurecode_amd/csrc/hip/ecamd_server_slots.hpp) on the
// CPU: which cached argument slot a request takes and whether its block is rewritten.  Stand-alone (no HIP);
// tests/test_server_slots.py compiles and runs it, with and without sanitizers.  Exit status 0 and
// "server_slots: ok" when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ecamd_server_slots.hpp"

namespace {

// the fields of SmallArgs (ecamd_kernels.hpp) that matter here: addresses, sizes, shape, the flag and its value
struct Args {
    const uint8_t* tables;
    const uint8_t* in;
    uint8_t* out;
    int64_t in_pitch, out_pitch, bs;
    int ncols, nrows;
    uint32_t masks[8];
    uint32_t* done;
    uint32_t done_val;
};

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                    \
        }                                                                  \
    } while (0)

Args request(uintptr_t tables, int64_t bs, uint32_t done_val)
{
    Args a;
    std::memset(&a, 0, sizeof(a));  // padding too: the comparison is bytewise
    a.tables = reinterpret_cast<const uint8_t*>(tables);
    a.in = reinterpret_cast<const uint8_t*>(uintptr_t(0x10000));
    a.out = reinterpret_cast<uint8_t*>(uintptr_t(0x20000));
    a.in_pitch = a.out_pitch = 1024;
    a.bs = bs;
    a.ncols = 10;
    a.nrows = 4;
    a.done = reinterpret_cast<uint32_t*>(uintptr_t(0x30000));
    a.done_val = done_val;
    return a;
}

struct Server {
    ecamd::ServerSlotEntry<Args> cached[2];
    int last_slot = 0;
    long rewrites = 0, stale = 0;
    ecamd::ServerSlotChoice post(const Args& a, uint32_t variant, uint64_t serial)
    {
        const ecamd::ServerSlotChoice c = ecamd::server_slot_choose(a, variant, serial, cached, last_slot);
        rewrites += c.rewrite;
        stale += c.stale;
        ecamd::server_slot_note(c, a, variant, serial, cached, last_slot);
        return c;
    }
    void relaunch() { cached[0].have = cached[1].have = false; }  // a new server instance holds no block
};

constexpr uint32_t kVariant = 4 | (4 << 4);

}  // namespace

int main()
{
    {  // nothing cached: the slot not used last, rewritten; then equal arguments and serial reuse it
        Server s;
        auto c = s.post(request(0x1000, 1024, 1), kVariant, 7);
        CHECK(c.slot == 1 && c.rewrite && !c.stale);
        c = s.post(request(0x1000, 1024, 2), kVariant, 7);  // done_val is ignored
        CHECK(c.slot == 1 && !c.rewrite && !c.stale);
        c = s.post(request(0x1000, 1024, 0xffffffffu), kVariant, 7);
        CHECK(c.slot == 1 && !c.rewrite && !c.stale);
        CHECK(s.rewrites == 1 && s.stale == 0);
    }
    {  // equal arguments, another serial (a new map at a recycled address): rewrites the slot not used last
        Server s;
        s.post(request(0x1000, 1024, 1), kVariant, 7);  // slot 1
        auto c = s.post(request(0x1000, 1024, 2), kVariant, 8);
        CHECK(c.slot == 0 && c.rewrite && c.stale);
        // both slots now hold the address with different serials: each serial finds its own
        c = s.post(request(0x1000, 1024, 3), kVariant, 7);
        CHECK(c.slot == 1 && !c.rewrite && !c.stale);
        c = s.post(request(0x1000, 1024, 4), kVariant, 8);
        CHECK(c.slot == 0 && !c.rewrite && !c.stale);
        // a third serial matches neither: the slot not used last (1), counted once
        c = s.post(request(0x1000, 1024, 5), kVariant, 9);
        CHECK(c.slot == 1 && c.rewrite && c.stale);
        CHECK(s.stale == 2 && s.rewrites == 3);
        // serial 0 (a request without tables) is a serial like any other
        c = s.post(request(0x1000, 1024, 6), kVariant, 0);
        CHECK(c.rewrite && c.stale);
    }
    {  // another variant, or any differing field, rewrites and is no stale hit
        Server s;
        s.post(request(0x1000, 1024, 1), kVariant, 7);
        auto c = s.post(request(0x1000, 1024, 2), kVariant | 256u, 7);
        CHECK(c.slot == 0 && c.rewrite && !c.stale);
        Args a = request(0x1000, 1024, 3);
        a.bs = 1026;
        c = s.post(a, kVariant, 7);
        CHECK(c.rewrite && !c.stale);
        a = request(0x2000, 1024, 4);  // other tables
        CHECK(s.post(a, kVariant, 7).rewrite);
        a = request(0x2000, 1024, 5);
        a.in += 128;
        CHECK(s.post(a, kVariant, 7).rewrite);
        a = request(0x2000, 1024, 6);
        a.out += 128;
        CHECK(s.post(a, kVariant, 7).rewrite);
        a = request(0x2000, 1024, 7);
        a.nrows = 3;
        CHECK(s.post(a, kVariant, 7).rewrite);
        a = request(0x2000, 1024, 8);
        a.masks[7] = 1;
        CHECK(s.post(a, kVariant, 7).rewrite);
        a = request(0x2000, 1024, 9);
        a.done += 1;
        CHECK(s.post(a, kVariant, 7).rewrite);
        CHECK(s.stale == 0);
    }
    {  // an alternating pair stays cached in the two slots
        Server s;
        const Args enc = request(0x1000, 1024, 0), dec = request(0x5000, 1024, 0);
        for (uint32_t i = 0; i < 1000; i++) {
            Args a = (i & 1) ? dec : enc;
            a.done_val = i + 1;
            const auto c = s.post(a, kVariant, (i & 1) ? 12 : 11);
            CHECK(c.rewrite == (i < 2) && c.slot == ((i & 1) ? 0 : 1));
        }
        CHECK(s.rewrites == 2 && s.stale == 0);
        // a third request takes the slot not used last (the pair's older one), the other survives
        auto c = s.post(request(0x9000, 1024, 1), kVariant, 13);
        CHECK(c.slot == 1 && c.rewrite);
        CHECK(!s.post(dec, kVariant, 12).rewrite);
        // after a relaunch nothing matches, whatever the entries still say
        s.relaunch();
        c = s.post(dec, kVariant, 12);
        CHECK(c.rewrite && !c.stale);
        c = s.post(request(0x9000, 1024, 2), kVariant, 13);
        CHECK(c.rewrite && !c.stale);
        CHECK(!s.post(dec, kVariant, 12).rewrite);
    }
    if (g_failed) {
        std::printf("server_slots: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("server_slots: ok\n");
    return 0;
}
