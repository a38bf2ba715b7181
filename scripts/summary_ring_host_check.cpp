// summary_ring_host_check.cpp -- the host side of the ring in which the class-table builds publish their counts
// (kangaroo_amd/csrc/summary_ring_host.h) under the host sanitizers, on a machine without a device: the packing of a slot, the
// stamp of a build and its slot of the ring, and the bounded wait that raycast.hip's class_view steers by.  A host array of
// exactly KFX_SUMMARY_RING slots plays the pinned ring (an index slip is an out-of-bounds access the address sanitizer reports),
// a model of the builds writes it, and the poll and the fallback are functors that count their calls.  Covered: slots never
// written; ring wrap-around; build numbers past 2^31 and across the wrap of the 32-bit build counter; a stamp from
// KFX_SUMMARY_RING builds ago (or ahead) not being taken for the expected one; the wait falling through to the fallback and to
// the error.  The kernels' store and the host's atomic load are not covered here (tests/test_gpu_class_build_one_launch.py,
// tests/test_gpu_summary.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/summary_ring_host_check.cpp -o summary_ring_host_check
//   ./summary_ring_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../kangaroo_amd/csrc/summary_ring_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;

// the ring as the builds write it: build b stores {stamp(b), count} in slot b % KFX_SUMMARY_RING
struct Ring {
    std::vector<uint64_t> slots = std::vector<uint64_t>(KFX_SUMMARY_RING, 0);
    void publish(unsigned build, int count) { slots.at(summary_ring_index(build)) = summary_ring_pack(summary_ring_stamp(build), count); }
    uint64_t look(unsigned build) const { return slots.at(summary_ring_index(build)); }
};

// a wait for `build` on `ring`: the poll reads the slot; `arrives_at` (> 0): the build publishes `count` just before that look;
// `fallback_publishes`: the fallback does.  Returns the wait's verdict; *polls and *fallbacks count the calls.
static int wait_on(Ring& ring, unsigned build, unsigned long long max_polls, unsigned long long arrives_at, bool fallback_publishes, int count, int* got,
                   unsigned long long* polls, int* fallbacks)
{
    *polls = 0; *fallbacks = 0;
    return summary_ring_wait(
        build, max_polls,
        [&]() {
            *polls += 1;
            if (arrives_at && *polls == arrives_at) ring.publish(build, count);
            return ring.look(build);
        },
        [&]() {
            *fallbacks += 1;
            if (fallback_publishes) ring.publish(build, count);
        },
        got);
}

int main()
{
    int n = 0;
    const int untouched = -12345;
    unsigned long long polls;
    int fallbacks, got;
    {   // packing: stamp and count come back as they went in, for every count a table can have (and the extremes of an int)
        for (const uint32_t stamp : {1u, 2u, 8u, 0x7fffffffu, 0x80000000u, 0xffffffffu})
            for (const int count : {0, 1, 4095, 4096, 0x7fffffff, -1}) {
                const uint64_t v = summary_ring_pack(stamp, count);
                CHECK(summary_ring_slot_stamp(v) == stamp && summary_ring_slot_count(v) == count);
                ++n;
            }
        CHECK(summary_ring_slot_stamp(0) == 0);   // an unwritten slot carries no build's stamp ...
    }
    {   // ... because no build's stamp is zero: the first builds, 2^31 and its neighbours, the end of the 32-bit counter
        const unsigned builds[] = {0u, 1u, 7u, 8u, 9u, 0x7ffffff8u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffff0u, 0xfffffffeu, 0xffffffffu};
        for (const unsigned b : builds) {
            CHECK(summary_ring_stamp(b) != 0u);
            CHECK(summary_ring_index(b) < KFX_SUMMARY_RING && summary_ring_index(b) == b % KFX_SUMMARY_RING);
            // the builds that share b's slot within several turns of the ring, before and after (the counter wraps): other stamps
            for (unsigned k = 1; k <= 4; ++k) {
                const unsigned before = b - k * KFX_SUMMARY_RING, after = b + k * KFX_SUMMARY_RING;
                CHECK(summary_ring_index(before) == summary_ring_index(b) && summary_ring_index(after) == summary_ring_index(b));
                CHECK(summary_ring_stamp(before) != summary_ring_stamp(b) && summary_ring_stamp(after) != summary_ring_stamp(b));
            }
            // and its neighbours sit in other slots
            for (unsigned k = 1; k < KFX_SUMMARY_RING; ++k) CHECK(summary_ring_index(b + k) != summary_ring_index(b));
            ++n;
        }
    }
    {   // slots never written: every look fails, the fallback runs once, the error comes back and nothing is read out
        Ring ring;
        for (const unsigned b : {0u, 3u, 7u, 8u, 0x80000000u, 0xffffffffu})
            for (const unsigned long long max_polls : {0ull, 1ull, 5ull, 1000ull}) {
                got = untouched;
                CHECK(wait_on(ring, b, max_polls, 0, false, 0, &got, &polls, &fallbacks) == -1);
                CHECK(got == untouched && polls == max_polls + 1 && fallbacks == 1);
                ++n;
            }
    }
    {   // a stream of builds over several turns of the ring, from three starting points (0; across 2^31; across the counter's
        // wrap): the steer's build (three behind the one just issued) is seen at the first look with its own count, without the
        // fallback; a build not issued yet, whose slot holds the stamp of KFX_SUMMARY_RING builds earlier, is not
        for (const unsigned start : {0u, 0x7ffffff0u, 0xfffffff0u}) {
            Ring ring;
            for (unsigned i = 0; i < 5 * KFX_SUMMARY_RING; ++i) {
                const unsigned b = start + i;   // (wraps)
                ring.publish(b, (int)(i * 7 + 1));
                if (i >= 2) {
                    got = untouched;
                    CHECK(wait_on(ring, b - 2, 1000, 0, false, 0, &got, &polls, &fallbacks) == 0);
                    CHECK(got == (int)((i - 2) * 7 + 1) && polls == 1 && fallbacks == 0);
                }
                // the build after this one: its slot holds build b + 1 - KFX_SUMMARY_RING's word (or nothing): never taken
                got = untouched;
                CHECK(wait_on(ring, b + 1, 3, 0, false, 0, &got, &polls, &fallbacks) == -1 && got == untouched && polls == 4 && fallbacks == 1);
                // a build overwritten since (KFX_SUMMARY_RING ago): its count is gone, and the present one is not taken for it
                if (i >= KFX_SUMMARY_RING) {
                    got = untouched;
                    CHECK(wait_on(ring, b - KFX_SUMMARY_RING, 3, 0, false, 0, &got, &polls, &fallbacks) == -1 && got == untouched);
                }
                ++n;
            }
        }
    }
    {   // the build arrives while the host looks: at the first, a middle and the last allowed look -- seen there, no fallback
        for (const unsigned long long at : {1ull, 2ull, 500ull, 1000ull}) {
            Ring ring;
            ring.publish(0x80000005u - KFX_SUMMARY_RING, 99);   // the slot's previous tenant
            got = untouched;
            CHECK(wait_on(ring, 0x80000005u, 1000, at, false, 42, &got, &polls, &fallbacks) == 0);
            CHECK(got == 42 && polls == at && fallbacks == 0);
            ++n;
        }
    }
    {   // it arrives only with the fallback (the stream synchronised): seen at the one look after it, verdict 1
        Ring ring;
        ring.publish(13u - KFX_SUMMARY_RING, 99);
        got = untouched;
        CHECK(wait_on(ring, 13u, 10, 0, true, 7, &got, &polls, &fallbacks) == 1);
        CHECK(got == 7 && polls == 11 && fallbacks == 1);
        // a wait without any look before the fallback
        Ring other;
        got = untouched;
        CHECK(wait_on(other, 2u, 0, 0, true, 3, &got, &polls, &fallbacks) == 1 && got == 3 && polls == 1 && fallbacks == 1);
        // arriving one look too late for the polling: the look after the fallback is that look
        Ring late;
        got = untouched;
        CHECK(wait_on(late, 5u, 10, 11, false, 9, &got, &polls, &fallbacks) == 1 && got == 9 && polls == 11 && fallbacks == 1);
        // and two looks too late: the error
        Ring never;
        got = untouched;
        CHECK(wait_on(never, 5u, 10, 12, false, 9, &got, &polls, &fallbacks) == -1 && got == untouched && polls == 11 && fallbacks == 1);
        n += 4;
    }
    printf("summary_ring_host_check: ok (%d cases)\n", n);
    return 0;
}
