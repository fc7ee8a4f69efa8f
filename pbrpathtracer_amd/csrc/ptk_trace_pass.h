// The FLAT pass of the trace kernels as TEXT: the body of `if (st == ST_TRAV) { ... }`, included by ptk_kernels.hip's main loop and by
// the fixed-cycle loop of the cycle unit (ptk_trace_cycle.h), so that there is one copy of it.  Not a header in the usual sense: it
// reads the kernel's locals (P, W, WS, L, Tdi, ray, rng, cnt, depth, iter, st ...) and its macros (PTK_WALK_DONE).
// PTK_U_FLAT_TRIS / PTK_U_FLAT_COUNT: where the flat table's address and length come from - the parameter block (an s_load per pass)
// unless the including unit holds them in registers of its own.
#ifndef PTK_U_FLAT_TRIS
#define PTK_U_FLAT_TRIS P.flat_tris
#endif
#ifndef PTK_U_FLAT_COUNT
#define PTK_U_FLAT_COUNT P.flat_count
#endif
                    typedef float f4v __attribute__((ext_vector_type(4)));
                    typedef const __attribute__((address_space(4))) f4v* cf4;        // constant address space -> s_load
                    const cf4 ct = (cf4)(uintptr_t)PTK_U_FLAT_TRIS;        // the scene's triangles in ascending index order
                    // both rays of a diffuse bounce in one pass over the triangles: the shadow ray
                    // (ray number `ray`) and the sampled bounce (`ray + 1`), pathtracer.cpp:638 / :724
                    const bool shadow = WS.occl_tri >= 0;
                    const uint32_t bounce_ray = shadow ? ray + 1u : ray;
                    RayPair R;
                    R.ox = f2{ W.ro.x, WS.ro.x }; R.oy = f2{ W.ro.y, WS.ro.y }; R.oz = f2{ W.ro.z, WS.ro.z };
                    R.dx = f2{ W.rd.x, WS.rd.x }; R.dy = f2{ W.rd.y, WS.rd.y }; R.dz = f2{ W.rd.z, WS.rd.z };
                    // exact PLAIN pass: one 4-bit class per record (classify_flat_kernel, ptk_frame.hip) names the edge words stored
                    // as zeros, and the record goes to the body with those operations deleted (ptk_flat_mt.h; DESIGN 4.1: same hits,
                    // same bits of t).  The class word is one scalar load per pass, the switch is wave-uniform, the order ascending.
                    constexpr bool ZERO_CLASSES = PLAIN && !STATS && !PTK_CONTRACT;
                    typedef const __attribute__((address_space(4))) unsigned long long* cu64;
                    const unsigned long long classes = ZERO_CLASSES ? *(cu64)(uintptr_t)(PTK_U_FLAT_TRIS + FLAT_CLASSES_AT) : 0ull;
#ifdef PTK_RECT_UNIT
                    // The pair pass (this unit only): the list's prefix of fan-split axis-aligned rectangles, one pair of records per
                    // turn of a counted loop - one wave-uniform switch over the six kinds, the arithmetic of both records with B's
                    // words named as A's (ptk_flat_mt.h mt_rect_pair), one shared accept, the hit moves (the pair lemma).
                    // Only a prefix is paired, so the order stays ascending; the loop below goes on from record 2m.
                    static_assert(ZERO_CLASSES, "the pair unit holds the exact PLAIN kernels only");
                    const unsigned long long pairs = *(cu64)(uintptr_t)(PTK_U_FLAT_TRIS + FLAT_PAIRS_AT);
                    const int n_pairs = (int)(pairs >> 32) & 15;
                    for (int j = 0; j < n_pairs; j++)
                    {
                        // of the pair's six float4s, record A's three: v0, e2 (e1(A), e1(B), e2(B) are words of e2(A) or zeros) and the index,
                        // which B's follows (the classifier pairs no other records)
                        const f4v a0 = ct[j * 2 * TRI_F4], a1 = ct[j * 2 * TRI_F4 + 1], a2 = ct[j * 2 * TRI_F4 + 2];
                        f2 aA, uA, vA, tA, aB, uB, vB, tB;
#define PTK_RECT_KIND(c) tri_math_rect<c>(W, R, a0.x, a0.y, a0.z, a1.z, a1.w, a2.x, aA, uA, vA, tA, aB, uB, vB, tB); break;
                        switch ((unsigned)(pairs >> (j * 4)) & 15u)
                        {
                            case 1: PTK_RECT_KIND(1) case 2: PTK_RECT_KIND(2) case 3: PTK_RECT_KIND(3) case 4: PTK_RECT_KIND(4) case 5: PTK_RECT_KIND(5)
                            default: PTK_RECT_KIND(6)           // (the classifier writes 1..6 inside the prefix)
                        }
#undef PTK_RECT_KIND
                        tri_accept_rect(W, WS, shadow, aA, tA, uA, vA, uB, vB, __float_as_int(a2.y));
                    }
                    for (int k = n_pairs * 2; k < PTK_U_FLAT_COUNT; k++)
#else
                    for (int k = 0; k < PTK_U_FLAT_COUNT; k++)
#endif
                    {
                        const f4v a0 = ct[k * TRI_F4], a1 = ct[k * TRI_F4 + 1], a2 = ct[k * TRI_F4 + 2];
                        const float4 t0 = make_float4(a0.x, a0.y, a0.z, a0.w), t1 = make_float4(a1.x, a1.y, a1.z, a1.w),
                                     t2 = make_float4(a2.x, a2.y, a2.z, a2.w);
#define PTK_ZERO_CLASS(c) case c: tri_math_pair<ZERO_CLASSES ? ptk_mt::flat_zero_mask(c) : 0u>(W, R, t0, t1, t2, ma, mu, mv, mt); break;
                        if (ZERO_CLASSES)
                        {
                            // (only the arithmetic is switched: the accept chain and the hit records follow once, for all classes)
                            f2 ma, mu, mv, mt;
                            switch ((unsigned)(classes >> (k * 4)) & 15u)
                            {
                                PTK_ZERO_CLASS(1) PTK_ZERO_CLASS(2) PTK_ZERO_CLASS(3) PTK_ZERO_CLASS(4) PTK_ZERO_CLASS(5)
                                PTK_ZERO_CLASS(6) PTK_ZERO_CLASS(7) PTK_ZERO_CLASS(8) PTK_ZERO_CLASS(9) PTK_ZERO_CLASS(10)
                                PTK_ZERO_CLASS(11) PTK_ZERO_CLASS(12) PTK_ZERO_CLASS(13) PTK_ZERO_CLASS(14) PTK_ZERO_CLASS(15)
                                default: tri_math_pair<0u>(W, R, t0, t1, t2, ma, mu, mv, mt); break;
                            }
                            (void)tri_accept_pair<STATS, PLAIN>(P, W, WS, shadow, ma, mu, mv, mt, t2, rng, bounce_ray, ray, cnt);
                        }
                        else
                            (void)tri_test_pair<STATS, PLAIN>(P, W, WS, R, shadow, t0, t1, t2, rng, bounce_ray, ray, cnt);
#undef PTK_ZERO_CLASS
                    }
                    if (shadow)
                    {
                        // DirectIllumimation visibility (pathtracer.cpp:522-526): lit unless something else is closest
                        if (STATS) { cnt.rays++; cnt.shadow++; }
                        if (!(WS.best.tri != PTK_NOHIT && WS.best.tri != WS.occl_tri)) L = add(L, Tdi);
                        WS.occl_tri = -1;
                        ray++;
                    }
                    W.node = NODE_EXIT;
                    PTK_WALK_DONE();
