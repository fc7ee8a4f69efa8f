// Work unit -> (quadrant pixel, sample in chunk, sample-buffer slot): the one statement of how a trace work item's units are laid out,
// called by the cycle unit's deal (ptk_trace_cycle.h) and by the host-side sweep (tests/cpp/unit_map_fuzz.cpp).  Plain C++: no HIP
// header, so a host compiler takes it as it stands.
//
// A work item is (an 8x8 quadrant, a chunk of samples); its units are numbered sample-major over the quadrant's LIVE pixels:
//   unit u = s * n_live + r,   s = sample in the chunk (0 .. s_count-1),   r = rank of the pixel among the live ones (0 .. n_live-1)
// and the sample goes to slot  out_base + s * 64 + q  of the sample buffer, q = 0 .. 63 the pixel's place in the quadrant (row * 8 +
// column) - pixel_of_rank[r], the table acquire_work_item leaves in LDS.  u / n_live is a multiply-high by magic = ceil(2^32 / n_live),
// exact while u * n_live < 2^32 (u < 64 * chunk and n_live <= 64: far below); for n_live = 1 the magic does not fit 32 bits and s = u.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTK_UNIT_MAP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PTK_UNIT_MAP_FN inline
#endif

namespace ptk {

struct UnitPlace { uint32_t q, s, slot; };          // quadrant pixel, sample in the chunk, sample-buffer slot

// ceil(2^32 / n_live) as acquire_work_item stores it (IT_NLIVE_MAGIC): truncated to 32 bits, so 0 for n_live = 1
PTK_UNIT_MAP_FN uint32_t unit_magic(uint32_t n_live) { return (uint32_t)((0x100000000ull + n_live - 1u) / n_live); }

// Table: anything indexable by rank that yields the pixel's place 0 .. 63 (an LDS byte array on the device, a plain array on the host)
template <class Table>
PTK_UNIT_MAP_FN UnitPlace unit_place(uint32_t u, uint32_t n_live, uint32_t magic, const Table& pixel_of_rank, uint32_t out_base)
{
    UnitPlace p;
    p.s = n_live == 1u ? u : (uint32_t)(((uint64_t)u * magic) >> 32);
    p.q = (uint32_t)pixel_of_rank[u - p.s * n_live];
    p.slot = out_base + p.s * 64u + p.q;
    return p;
}

// ... and the pixel's row-major index in the frame (rows from the top), from the quadrant's origin as one word: base = y0 * width + x0
PTK_UNIT_MAP_FN uint32_t unit_pixel(uint32_t q, uint32_t base, uint32_t width) { return base + (q >> 3) * width + (q & 7u); }

}  // namespace ptk
