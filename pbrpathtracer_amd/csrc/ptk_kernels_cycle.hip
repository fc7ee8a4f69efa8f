// The exact build's PLAIN trace kernels a third time: trace_kernel_cycle<false, true, true, false> and <false, true, true, true>, and
// their launcher (ptk::launch_trace_cycle), as a translation unit of their own.  The kernel text is ptk_kernels.hip's, included under
// PTK_PLAIN_UNIT and PTK_RECT_UNIT - the kernel template with the pair pass and a launcher, nothing else of that file - and
// PTK_CYCLE_UNIT, which replaces the template's voted main loop by ptk_trace_cycle.h: a fixed deal / shade / pass cycle with no block
// vote, units dealt from scalar registers (ptk_unit_map.h), and the launch constants the loop reads held in SGPRs.  The pass
// (ptk_trace_pass.h) and the shade block (ptk_trace_shade.h) are the text the other units include: everything that reaches the image
// is theirs, so the samples are the pair unit's bit for bit.  Two forms in the shade block are this unit's own (PTK_SHADE32,
// ptk_device_fn.h): its table reads go by 32-bit byte offsets from scalar bases (ldg_at; the host launches the unit only while those
// tables are below 2^32 bytes, ptk_table_offset.h) and the hemisphere angle is computed in float (ptk_angle_f32.h: the same bits for
// every draw, swept on the host).  Neither changes a floating-point operation the oracle defines.  Its square roots are its own as well: they
// come from v_rsq_f32 (sqrt_ieee_rsq, ptk_device_fn.h: sqrtf's bits for every input, enumerated on the GPU); the pair unit keeps the
// neighbour-test form.
// csrc/Makefile compiles this unit with the PLAIN unit's flags (CYCLE_UNIT_FLAGS adds to them; empty by default: the pair unit's module
// inliner is not used here, kinds 1, 3 and 5 of the pair loop keep one v_mul_f32 more); launch_trace picks it when
// RenderParams::plain is 3 (the flat_cycle option on top of flat_rect_pairs).  ptk_kernels_plain.hip and ptk_kernels_rect.hip are not
// touched by any of this and keep their machine code.
#include "ptk_unit_map.h"
#define PTK_PLAIN_UNIT 1
#define PTK_RECT_UNIT 1
#define PTK_CYCLE_UNIT 1
#define trace_kernel trace_kernel_cycle
#include "ptk_kernels.hip"
