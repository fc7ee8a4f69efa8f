// The rule that keeps the cycle unit away from tables of 2^32 bytes or more (csrc/ptk_table_offset.h cycle_unit_tables_fit, asked
// by run_passes) at its edge: width * height * 16 is the largest per-pixel table, MAT_F4 * 16 = 96 bytes a material.
#include <stdint.h>
#include <stdio.h>

#include "ptk_table_offset.h"

static int bad = 0;
static void expect(bool got, bool want, const char* what)
{
    if (got != want) { printf("WRONG: %s: %d, expected %d\n", what, (int)got, (int)want); bad++; }
}

int main()
{
    using ptk::cycle_unit_tables_fit;
    // 2^28 pixels make 2^32 bytes: the largest frame that passes has 2^28 - 1 pixels or fewer
    expect(cycle_unit_tables_fit(16384, 16384, 0), false, "16384 x 16384 (2^28 pixels, 2^32 bytes)");
    expect(cycle_unit_tables_fit(16384, 16383, 0), true, "16384 x 16383");
    expect(cycle_unit_tables_fit(16383, 16384, 0), true, "16383 x 16384");
    expect(cycle_unit_tables_fit(268435455, 1, 0), true, "(2^28 - 1) x 1: the last byte offset is 2^32 - 32");
    expect(cycle_unit_tables_fit(268435456, 1, 0), false, "2^28 x 1");
    expect(cycle_unit_tables_fit(1, 268435455, 0), true, "1 x (2^28 - 1)");
    expect(cycle_unit_tables_fit(1, 268435456, 0), false, "1 x 2^28");
    expect(cycle_unit_tables_fit(2147483647, 2147483647, 0), false, "INT_MAX x INT_MAX (no 32-bit overflow in the rule itself)");
    expect(cycle_unit_tables_fit(65536, 65536, 0), false, "65536 x 65536 (2^32 pixels: zero in 32 bits)");
    expect(cycle_unit_tables_fit(1280, 720, 36), true, "bench config C2");
    expect(cycle_unit_tables_fit(0, 720, 0), false, "no frame");
    expect(cycle_unit_tables_fit(1280, -1, 0), false, "negative height");
    // the material table, in float4s
    expect(cycle_unit_tables_fit(64, 64, (1ull << 28) - 1), true, "2^28 - 1 float4s of materials");
    expect(cycle_unit_tables_fit(64, 64, 1ull << 28), false, "2^28 float4s of materials");
    expect(cycle_unit_tables_fit(64, 64, 1ull << 60), false, "2^60 float4s (no 64-bit overflow in the rule itself)");
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
