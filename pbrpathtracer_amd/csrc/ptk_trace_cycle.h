// The cycle unit's main loop (ptk_kernels_cycle.hip; included by ptk_kernels.hip's kernel template under PTK_CYCLE_UNIT, in place of
// the voted loop): TEXT inside the kernel, behind its prologue and the PTK_FINISH_PATH / PTK_WALK_DONE macros.
//
// Fixed cycle.  A PLAIN kernel has two blocks, the shade block and the pass, and a FLAT wave in such a scene alternates them
// strictly; the voted loop nevertheless counts five states twice per cycle, weighs them, and decides a deal it then repeats the
// ballots for.  Here one turn is: deal - leave if nothing is live - shade - pass.  There is no vote and no ST_GEN.
//   * At the top of a turn no lane is in TRAV: the pass leaves every lane that ran it in NEED (miss, or a hit that would be the
//     terminal interaction: PTK_WALK_DONE) or in SHADE (hit), and FLAT lanes never re-enter the walk from it (W.occl_tri stays -1:
//     the shadow ray lives in WS).  So the states up there are NEED, SHADE and DONE.
//   * The deal turns every NEED lane into SHADE (a unit; depth < 0 marks the path start, which the shade block performs) or, when
//     every queue is empty, into DONE.  A lane whose path ended in the shade block (roulette, the terminal rule) is in NEED during
//     the pass of that turn and sits it out, as it does under the vote.
// Termination.  `dry` is set by the one deal that found every queue empty (acquire_work_item returned 0; it returns 0 ever after:
// IT_STEAL = 8, IT_LO = IT_HI = 0, and a used-up quota stays used up), and DONE is only ever assigned behind it.  The exit test
// follows the deal directly and is "no lane in SHADE": behind a deal no lane is in NEED or TRAV, so it says every lane is DONE - seen
// only after a deal that found the queues empty, with nothing undealt (next_unit == total_units whenever acquire_item is called).
// Every turn that does not leave runs the shade block with at least one lane, each of which either ends its path or goes through the
// pass: a path ends after at most max_depth interactions, a turn deals at most 64 units and the launch has finitely many, so the
// loop ends.  The deal's inner loop (entered only when the item has fewer units left than lanes want) ends because each round either
// breaks or uses the item up and deals to at least one lane (m_need loses bits) before it acquires the next of finitely many items.
//
// Scalar deal.  next_unit, total_units and the item's constants are wave-uniform and held in SGPRs: LDS reads are divergent values
// to the compiler, so everything that comes from lds_item or from acquire_item() passes through readfirstlane once per ACQUIRED
// ITEM, behind acquire_work_item's closing barrier, and the deal loop's control is s_cmp / s_cbranch.  Per round a needy lane
// computes its rank among the needy (mbcnt), the multiply-high by the item's magic, one LDS read of lds_pixel_of_rank and the three
// results (ptk_unit_map.h unit_place / unit_pixel, the function tests/cpp/unit_map_fuzz.cpp sweeps).  The queues, the stealing,
// one-item-per-wave launches and the multi-GPU quota stay in acquire_work_item and see the same calls in the same order.
//
// Launch constants.  In SGPRs for the kernel's life: the sample buffer (samples_u, as before), max_depth (max_depth_u, read by
// PTK_WALK_DONE), the frame's width, the flat table's address and its record count.  NOT hoisted: the shade block's table pointers
// (pixel_rng, primary_hit, primary_rd, shade, mats, lights, first_sample, num_lights) - sixteen more registers than the budget has.
    static_assert(PLAIN && !STATS && FLAT, "the cycle unit holds the exact PLAIN kernels only");
    (void)camRight; (void)camUp;        // (the camera-ray block's: a PLAIN path starts at its cached first hit)
    {
        const uint32_t width_u = (uint32_t)__builtin_amdgcn_readfirstlane(P.width);
        const float4* const flat_tris_u = uniform_ptr(P.flat_tris);
        const int flat_count_u = __builtin_amdgcn_readfirstlane(P.flat_count);
#define PTK_U_FLAT_TRIS flat_tris_u
#define PTK_U_FLAT_COUNT flat_count_u
        // the current item, wave-uniform (SGPRs): live pixels, their magic, y0 * width + x0, first sample of the chunk, first slot
        uint32_t it_nlive = 1u, it_magic = 0u, it_pixbase = 0u, it_sbegin = 0u, it_outbase = 0u;
        uint32_t dry = 0u;              // 1: every queue has been seen empty (or this wave's quota is used up).  (A word, not a bool: a
                                        // loop-carried uniform bool is lowered to a lane mask and tested through two VALU instructions)
        // a lane's unit -> its pixel, sample and slot (ptk_unit_map.h)
        auto take_unit = [&](uint32_t u)
        {
            const UnitPlace up = unit_place(u, it_nlive, it_magic, lds_pixel_of_rank, it_outbase);
            pix = unit_pixel(up.q, it_pixbase, width_u);
            sample_abs = it_sbegin + up.s;
            out_idx = up.slot;
            st = ST_SHADE;      // (the path starts at its first surface interaction: the shade block sets it up, depth < 0 marks it)
            depth = -1;
        };
        for (;;)
        {
            // ---- 1. deal to the lanes that need a unit ----
            unsigned long long m_need = __ballot(st == ST_NEED);
            if (m_need)
            {
                uint32_t wanted = (uint32_t)__popcll(m_need);
                if (wanted > total_units - next_unit)
                {
                    // the item has fewer units left than lanes want (or there is no item yet): hand out what it has, take the next one.
                    // About one deal in eight at 8 samples per chunk; the common deal below is straight-line code
                    for (;;)
                    {
                        if (next_unit >= total_units)
                        {
                            next_unit = 0u;
                            total_units = dry ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)acquire_item());
                            if (total_units == 0u)
                            {
                                dry = 1u;
                                if (__builtin_amdgcn_inverse_ballot_w64(m_need)) st = ST_DONE;
                                wanted = 0u;
                                break;
                            }
                            it_nlive = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[IT_NLIVE]);
                            it_magic = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[IT_NLIVE_MAGIC]);
                            it_pixbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[IT_Y0]) * width_u + (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[IT_X0]);
                            it_sbegin = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[IT_SBEGIN]);
                            it_outbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[IT_OUTBASE]);
                        }
                        const uint32_t avail = total_units - next_unit;            // > 0
                        if (wanted <= avail) break;                                 // the common deal finishes
                        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m_need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_need, 0u));
                        if (__builtin_amdgcn_inverse_ballot_w64(m_need) && rank < avail) take_unit(next_unit + rank);
                        next_unit = total_units;
                        m_need = __ballot(st == ST_NEED);
                        wanted = (uint32_t)__popcll(m_need);                        // > 0: wanted - avail
                    }
                }
                if (wanted)
                {
                    // every needy lane takes a unit of the current item: its rank among the needy names it
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m_need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_need, 0u));
                    if (__builtin_amdgcn_inverse_ballot_w64(m_need)) take_unit(next_unit + rank);
                    next_unit += wanted;
                }
            }
            // ---- 2. leave if no lane is live (behind a deal: every lane is in SHADE or DONE) ----
            if (__ballot(st == ST_SHADE) == 0ull) break;
            // ---- 3. the shade block, for the lanes that have a hit (a path start is a cached camera-ray hit) ----
            if (st == ST_SHADE)
            {
#include "ptk_trace_shade.h"
            }
            // ---- 4. the pass, for the lanes that have a ray ----
            if (st == ST_TRAV)
            {
#include "ptk_trace_pass.h"
            }
        }
#undef PTK_U_FLAT_TRIS
#undef PTK_U_FLAT_COUNT
    }
