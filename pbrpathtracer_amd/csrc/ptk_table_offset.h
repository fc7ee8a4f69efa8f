// When the cycle unit's kernels may be launched: its shade block reads its tables at a wave-uniform base plus a 32-BIT byte offset
// (ptk_device_fn.h ldg_at), so every table it reads that way must be smaller than 2^32 bytes.  Plain C++, the one statement of the
// rule: run_passes (ptk_api.hip) asks it per render and launches the pair unit's kernel - the same pass and shade block with 64-bit
// addressing, bit-identical samples - when it says no; tests/cpp/table_offset_edge.cpp holds it at its edge.
//   per pixel:     pixel_rng 8 bytes, primary_hit and primary_rd 16 bytes - the largest, width * height * 16
//   per material:  96 bytes (MAT_F4 float4s); the caller passes the table's length in float4s
//   per triangle:  shade records, frames and lights of a FLAT scene, at most 16 triangles: a few KiB, nothing to ask
// The sample buffer is NOT among them: its store keeps 64-bit addressing.
#pragma once
#include <stdint.h>

namespace ptk {

inline bool cycle_unit_tables_fit(int width, int height, uint64_t mats_float4s)
{
    if (width <= 0 || height <= 0) return false;
    const uint64_t limit = 1ull << 32;
    return (uint64_t)width * (uint64_t)height < limit / 16ull && mats_float4s < limit / 16ull;       // (no product that could wrap)
}

}  // namespace ptk
