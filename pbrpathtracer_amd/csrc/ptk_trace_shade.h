// The shade block of the trace kernels as TEXT: the body of `if (st == ST_SHADE) { ... }` - the start of a path whose cached camera
// ray hit (depth < 0) and one surface interaction - included by ptk_kernels.hip's main loop and by the fixed-cycle loop of the cycle
// unit (ptk_trace_cycle.h), so that there is one copy of it.  Like ptk_trace_pass.h it reads the kernel's locals and macros.
                if (depth < 0)
                {
                    // a path dealt since the last shade block.  Pinhole camera, no stochastic opacity: every sample of this
                    // pixel shoots the same camera ray, so its direction and closest hit were computed once (primary_hits_kernel)
                    // and the path starts at its first surface interaction (pixels whose camera ray misses are never dealt).
                    // The stream is set up as in the camera-ray block below, and the two SampleCircle draws a pinhole frame
                    // still consumes (pathtracer.cpp:787, always two) only advance it - two LCG steps in one:
                    //   s2 = (s * a + inc) * a + inc = s * a^2 + inc * (a + 1)      (mod 2^32: the identical state)
#if PTK_SHADE32
                    // (the cycle unit: 32-bit byte offsets from the three wave-uniform bases, ldg_at - the host launches this unit
                    // only for frames whose tables stay below 2^32 bytes)
                    const uint2 pr = ldg_at(P.pixel_rng, pix * 8u);
                    const float4 c = ldg_at(P.primary_hit, pix * 16u), r = ldg_at(P.primary_rd, pix * 16u);
#else
                    const uint2 pr = P.pixel_rng[pix];
                    const float4 c = P.primary_hit[pix], r = P.primary_rd[pix];
#endif
                    rng.inc = pr.y;
                    rng.state = hash32(P.first_sample + sample_abs + pr.x);
                    rng.key = rng.state;
                    rng.state = rng.state * (747796405u * 747796405u) + rng.inc * (747796405u + 1u);
                    L = V(0.0f, 0.0f, 0.0f); T = V(1.0f, 1.0f, 1.0f);
                    depth = 0; iter = 0; inside = false; ray = 1;
                    W.occl_tri = -1;
                    if (STATS) cnt.started++;
                    W.ro = camPos0; W.rd = V(r.x, r.y, r.z);
                    W.best.tri = __float_as_int(c.x); W.best.t = c.y; W.best.u = c.z; W.best.v = c.w;
                    W.node = NODE_EXIT; W.top = stack; W.tri_left = 0;
                }
                // ---- one surface interaction of PathTracer::Trace, pathtracer.cpp:551-727 ----
                const bool ended = shade_interaction<STATS, FLAT, PLAIN, LAMBERT>(P, W, WS, stack, rng, L, T, Tdi, nextDir, depth, iter, inside, ray, cnt);
                if (ended) PTK_FINISH_PATH();
                else st = ST_TRAV;
