// The exact build's PLAIN trace kernels, trace_kernel<false, true, true, false> and <false, true, true, true>, and their launcher
// (ptk::launch_trace_plain), as a translation unit of their own.  The kernel text is ptk_kernels.hip's, included under
// PTK_PLAIN_UNIT, which leaves out everything else of that file; csrc/Makefile compiles this unit - and only this one - with
//   -mllvm -structurizecfg-skip-uniform-regions=1
// Their pass switches wave-uniformly over sixteen zero classes per triangle.  Without the option the backend rewrites that uniform
// branch tree into structured form: each subtree sets a 64-bit flag and each level is left through a flag test and a taken branch,
// two to five hops per triangle between a body and the accept chain.  With it the bodies branch straight to the accept chain
// (DESIGN 4.1 "The pass", 5; tests/test_plain_dispatch_isa_cpu.py holds the assembly to that).  The option acts on a whole unit and
// raises the BVH STATS kernel's spills, so the other kernels stay in ptk_kernels.hip on the common command line.
#define PTK_PLAIN_UNIT 1
#include "ptk_kernels.hip"
