// ecamd_server_slots.hpp -- which of the resident small server's two cached argument slots a request
// takes (server_post in ecamd_small.hip).  Host logic only, no HIP: tests/c/server_slots_test.cpp
// runs it on the CPU.
#pragma once
#include <cstdint>
#include <cstring>

namespace ecamd {

// What the host remembers of one mailbox slot: the argument block it last wrote there, its kernel variant
// and the serial of the map whose tables the block points to (ecamd_map::serial; 0: the request carries
// no tables, the flat-XOR form has its masks in the block).
template <class Args>
struct ServerSlotEntry {
    bool have = false;  // written since this server instance was launched
    Args args{};
    uint32_t variant = 0;
    uint64_t serial = 0;
};

struct ServerSlotChoice {
    int slot;      // the slot the request is posted with
    bool rewrite;  // its block must be written there (a new generation: the server reads it and stages its tables again)
    bool stale;    // a cached block matched in everything but the serial: another map at a recycled address
};

// A request reuses a slot only when its variant, every argument but the completion-flag value (done_val)
// and the map's serial equal the cached ones: a device address alone does not identify a map, a freed
// table image's address comes back from the allocator for the next map of that shape.  Anything else
// rewrites the slot not used last, so two alternating requests both stay cached.
template <class Args>
ServerSlotChoice server_slot_choose(const Args& req, uint32_t variant, uint64_t serial,
                                    const ServerSlotEntry<Args> (&cached)[2], int last_slot)
{
    bool stale = false;
    for (int i = 0; i < 2; i++) {
        if (!cached[i].have || cached[i].variant != variant) continue;
        Args cmp = req;
        cmp.done_val = cached[i].args.done_val;
        if (std::memcmp(&cmp, &cached[i].args, sizeof(Args)) != 0) continue;
        if (cached[i].serial == serial) return {i, false, false};
        stale = true;
    }
    return {(last_slot ^ 1) & 1, true, stale};
}

// Records the choice: a rewritten slot now holds the request.
template <class Args>
void server_slot_note(const ServerSlotChoice& c, const Args& req, uint32_t variant, uint64_t serial,
                      ServerSlotEntry<Args> (&cached)[2], int& last_slot)
{
    if (c.rewrite) {
        cached[c.slot].have = true;
        cached[c.slot].args = req;
        cached[c.slot].variant = variant;
        cached[c.slot].serial = serial;
    }
    last_slot = c.slot;
}

}  // namespace ecamd
