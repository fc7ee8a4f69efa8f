// The exact build's PLAIN trace kernels once more, with the pair pass: trace_kernel_rect<false, true, true, false> and
// <false, true, true, true>, and their launcher (ptk::launch_trace_rect), as a translation unit of their own.  The kernel text is
// ptk_kernels.hip's, included under PTK_PLAIN_UNIT - the kernel template and a launcher, nothing else of that file - and
// PTK_RECT_UNIT, which puts a counted loop in front of the pass's record loop: the prefix of the flat list that consists of
// fan-split axis-aligned rectangles (classify_flat_kernel's pair word, ptk_flat_mt.h flat_rect_pair) is tested one pair of records
// at a time, the second record's words named as the first's, so that the compiler's common-subexpression elimination removes what
// the two tests share - s, the determinant and its reciprocal, t, half of the accept tests (the pair lemma).
// csrc/Makefile compiles this unit with the PLAIN unit's flags and the module inliner (RECT_UNIT_FLAGS: both copies of the test are
// in the kernel before either is simplified, or three kinds keep one product twice, once negated); launch_trace picks it when RenderParams::plain is 2 (the
// flat_rect_pairs option).  ptk_kernels_plain.hip is not touched by any of this and keeps its machine code.
#define PTK_PLAIN_UNIT 1
#define PTK_RECT_UNIT 1
#define trace_kernel trace_kernel_rect
#include "ptk_kernels.hip"
