// nr_key_records.h — the size rules of a key cache's record store (nr_common.h Schedule::krec).  Plain C++ with
// no HIP dependency: tests/test_key_records_policy.py compiles it with the host compiler.
//
// The store holds, for each cached slot in dense order, the 16-double Gouraud shading record of every distinct
// winner of the slot's tile; roff[s] is the number of records before slot s (an exclusive prefix sum of the
// slots' distinct counts, in records), roff[slots] the total.
//   bytes   what the store holds: 128 bytes per record.
//   room    what is allocated: the records and a tail of TAIL more.  The steady kernel's loads are unconditional:
//           a slot without winners -- the last one may start at the total -- still reads its "first" record.
//   fits    the cap: a store is built only if it is no larger than the context's f64 framebuffer (W * H * ipp
//           doubles).  A condition, not a tuned number: a scene whose tiles have so many winners that their
//           records outweigh the framebuffer stays on the key index.
#pragma once

#include <cstddef>
#include <cstdint>

namespace nrkrec {

constexpr unsigned REC_DOUBLES = 16;
constexpr std::uint64_t REC_BYTES = REC_DOUBLES * sizeof(double);

inline std::uint64_t bytes(std::uint64_t records) { return records * REC_BYTES; }

constexpr unsigned TAIL = 1;
inline std::uint64_t room_doubles(std::uint64_t records) { return (records + TAIL) * REC_DOUBLES; }

inline bool fits(std::uint64_t records, std::int64_t W, std::int64_t H, int ipp) {
    if (W <= 0 || H <= 0 || ipp <= 0) return false;
    const std::uint64_t fb = (std::uint64_t)W * (std::uint64_t)H * (std::uint64_t)ipp * sizeof(double);
    return bytes(records) <= fb;
}

// The exclusive prefix sum the scan kernel writes, on the host (the reference of its test): roff has n + 1
// entries; returns the total.
inline std::uint64_t offsets(const std::uint32_t* distinct, std::size_t n, std::uint32_t* roff) {
    std::uint64_t sum = 0;
    for (std::size_t s = 0; s < n; ++s) {
        roff[s] = (std::uint32_t)sum;
        sum += distinct[s];
    }
    roff[n] = (std::uint32_t)sum;
    return sum;
}

}  // namespace nrkrec
