// summary_ring_host.h -- the host side of the ring in which the class-table builds publish their counts (kfx_sdf_summary,
// kfx_device.h; summary.hip writes it, raycast.hip class_view and debug.hip read it).  Host-only and free of HIP, so that
// scripts/summary_ring_host_check.cpp can run it under the host sanitizers on a machine without a device.
//
// A slot is one 64-bit word {stamp, count}: the count of 32^3-cell entries of class != 0 in the low half, and in the high half
// the stamp of the build that wrote it -- its build number + 1 folded into [1, 2^32 - 1], so that a slot nobody has written
// (zero) carries no build's stamp.  Build b writes slot b % KFX_SUMMARY_RING with one 64-bit store; a reader that wants build
// b's count looks at that slot until it carries b's stamp.  The slot's previous writer was build b - KFX_SUMMARY_RING and its
// next one is b + KFX_SUMMARY_RING: their stamps differ from b's (the fold repeats after 2^32 - 1 builds only), so a count is
// never taken for another build's.
#pragma once
#include <cstdint>

#define KFX_SUMMARY_RING 8

namespace kfx {

inline unsigned summary_ring_index(unsigned build) { return build % KFX_SUMMARY_RING; }
inline uint32_t summary_ring_stamp(unsigned build) { return build % 0xffffffffu + 1u; }   // never 0
inline uint64_t summary_ring_pack(uint32_t stamp, int count) { return ((uint64_t)stamp << 32) | (uint32_t)count; }
inline uint32_t summary_ring_slot_stamp(uint64_t slot) { return (uint32_t)(slot >> 32); }
inline int summary_ring_slot_count(uint64_t slot) { return (int)(uint32_t)slot; }

// The bounded wait for build `build`'s count.  poll() returns the present value of slot summary_ring_index(build); fallback()
// is what makes the build finish for certain (a synchronisation of its stream).  At most max_polls looks, then the fallback and
// one more look.  Returns 0 (seen while polling) or 1 (seen after the fallback) with *count set, or -1: the slot does not carry
// the build's stamp even now, *count is untouched and nothing was read out of the slot.
template <typename POLL, typename FALLBACK>
inline int summary_ring_wait(unsigned build, unsigned long long max_polls, POLL poll, FALLBACK fallback, int* count)
{
    const uint32_t want = summary_ring_stamp(build);
    for (unsigned long long i = 0; i < max_polls; ++i) {
        const uint64_t v = poll();
        if (summary_ring_slot_stamp(v) == want) { *count = summary_ring_slot_count(v); return 0; }
    }
    fallback();
    const uint64_t v = poll();
    if (summary_ring_slot_stamp(v) == want) { *count = summary_ring_slot_count(v); return 1; }
    return -1;
}

} // namespace kfx
