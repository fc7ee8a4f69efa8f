// The text of rays_kernel (ptk_rays.hip), included once per variant: PTK_RAYS_KERNEL names the kernel, PTK_RAYS_KEYED says where
// a ray's RNG pixel comes from - 0: R.key_base + the ray's index (ptk_trace_rays), 1: R.keys[index] (a lightmap's texel index,
// ptk_bake_lightmap).  Two kernels from one text rather than a template, so that rays_kernel keeps its name and machine code.
#if PTK_RAYS_KEYED
#define PTK_RAYS_KEY(i) keys_u[i]
#else
#define PTK_RAYS_KEY(i) (R.key_base + (i))
#endif

__global__ __launch_bounds__(PTK_RAYS_BLOCK, PTK_RAYS_WAVES) void PTK_RAYS_KERNEL(RaysBlock* __restrict__ block)
{
    typedef const __attribute__((address_space(4))) RenderParams ConstParams;
    typedef const __attribute__((address_space(4))) RaysParams ConstRays;
    ConstParams& P = *(ConstParams*)(uintptr_t)&block->p;
    ConstRays& R = *(ConstRays*)(uintptr_t)&block->r;
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_RAYS_BLOCK];
    __shared__ uint32_t lds_item[RI_WORDS];
    static_assert(PTK_RAYS_BLOCK == 64, "one wave per workgroup");

    const int lane = threadIdx.x;
    int* stack = lds_stack + lane;
    unsigned* const counter = &block->counter;

    // takes the next item off the counter (-> lds_item); returns its unit count, 0 when none is left.  Wave-uniform.
    auto acquire_item = [&]() -> uint32_t {
        __syncthreads();                    // every lane is done with the previous item's words
        if (lane == 0)
        {
            const uint32_t item = atomicAdd(counter, 1u);
            uint32_t units = 0;
            if (item < (uint32_t)P.num_items)
            {
                const uint32_t group = item / (uint32_t)P.num_chunks, chunk_id = item - group * (uint32_t)P.num_chunks;
                const uint32_t ray0 = group * 64u, n = min(64u, (uint32_t)R.num_rays - ray0);      // host: group * 64 < num_rays
                const uint32_t s_begin = chunk_id * (uint32_t)P.chunk, s_count = min((uint32_t)P.chunk, P.spp - s_begin);   // host: s_begin < spp
                lds_item[RI_N] = n; lds_item[RI_MAGIC] = (uint32_t)((0x100000000ull + n - 1u) / n);
                lds_item[RI_RAY0] = ray0; lds_item[RI_SBEGIN] = s_begin;
                lds_item[RI_OUTBASE] = item * (uint32_t)P.chunk * 64u;
                units = n * s_count;
            }
            lds_item[RI_UNITS] = units;
        }
        __syncthreads();
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_item[RI_UNITS]);
    };

    bool more = true;                           // wave-uniform: the counter has not been seen past the last item yet
    uint32_t total_units = 0, next_unit = 0;    // wave-uniform
    // per-lane: the unit this lane is tracing
    uint32_t ray_i = 0, sample_abs = 0, out_idx = 0;

    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    Rng rng;
    rng.inc = 1u; rng.state = 0; rng.key = 0;
    Walk W;
    W.begin(V(0.0f, 0.0f, 0.0f), V(0.0f, 0.0f, 1.0f), 0, stack, 0.0f);
    W.occl_tri = -1;
    v3 L = V(0.0f, 0.0f, 0.0f), T = V(1.0f, 1.0f, 1.0f);
    v3 Tdi = V(0.0f, 0.0f, 0.0f), nextDir = V(0.0f, 0.0f, 1.0f);
    int depth = 0, iter = 0;
    bool inside = false;
    uint32_t ray = 0;
    int st = ST_NEED;

    float4* const samples_u = uniform_ptr(P.samples);
    const float* const origins_u = uniform_ptr(R.origins);
    const float* const dirs_u = uniform_ptr(R.dirs);
#if PTK_RAYS_KEYED
    const uint32_t* const keys_u = uniform_ptr(R.keys);
#endif
    const int num_nodes_u = __builtin_amdgcn_readfirstlane(P.num_nodes);
    const float scene_bound_u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.scene_bound)));

    // a finished path: its radiance goes to the sample buffer, the lane waits for its next unit (or is done: the counter ran dry)
#define PTK_FINISH_PATH()                                                                         \
    do {                                                                                          \
        samples_u[out_idx] = make_float4(L.x, L.y, L.z, 0.0f);                                    \
        st = more ? ST_NEED : ST_DONE;                                                            \
    } while (0)
    // a finished walk, as in trace_kernel: a shadow ray resolves DirectIllumimation's visibility and rolls into the sampled bounce;
    // a bounce ray (or the caller's ray) ends the path on a miss or queues for shading
#define PTK_WALK_DONE()                                                                           \
    do {                                                                                          \
        ray++;                                                                                    \
        const bool hit_ = W.best.tri != PTK_NOHIT;                                                \
        if (W.occl_tri >= 0)                                                                      \
        {                                                                                         \
            if (!(hit_ && W.best.tri != W.occl_tri)) L = add(L, Tdi);     /* pathtracer.cpp:522-526 */  \
            W.occl_tri = -1;                                                                      \
            W.begin(W.ro, nextDir, num_nodes_u, stack, scene_bound_u);                            \
        }                                                                                         \
        else if (!hit_) PTK_FINISH_PATH();                                /* :550 miss -> black */ \
        else st = ST_SHADE;                                                                       \
    } while (0)

    int debt_shade = 0, debt_need = 0;     // wave-uniform: lane-iterations wasted by lanes that wait for shading / for a unit
    for (;;)
    {
        // deal the next work units to the lanes that need one (wave-uniform code)
        unsigned long long m_need = __ballot(st == ST_NEED);
        while (m_need)
        {
            if (next_unit >= total_units)
            {
                next_unit = 0;
                total_units = more ? acquire_item() : 0u;
                if (total_units == 0) { more = false; if (st == ST_NEED) st = ST_DONE; break; }
            }
            const uint32_t n = lds_item[RI_N];
            const uint32_t u = next_unit + (uint32_t)__popcll(m_need & ((1ull << lane) - 1ull));
            if (st == ST_NEED && u < total_units)
            {
                const uint32_t s_in_chunk = n == 1u ? u : __umulhi(u, lds_item[RI_MAGIC]);      // = u / n
                const uint32_t r = u - s_in_chunk * n;
                ray_i = lds_item[RI_RAY0] + r;
                sample_abs = lds_item[RI_SBEGIN] + s_in_chunk;
                out_idx = lds_item[RI_OUTBASE] + s_in_chunk * 64u + r;
                st = ST_TRAV;
                depth = -1;                 // set up below, once for all the lanes this deal served
            }
            next_unit = min(total_units, next_unit + (uint32_t)__popcll(m_need));
            m_need = __ballot(st == ST_NEED);
        }
        if (depth < 0)
        {
            // a new path: the caller's ray is its ray 0; its stream is that of (seed, key_base + ray, sample) - rng_init of the
            // oracle -, under PTK_RAYS_LENS_DRAWS advanced past the two SampleCircle draws of a camera ray, two LCG steps in one
            // (trace_kernel's cached-camera start)
            const float* o = origins_u + (size_t)ray_i * 3, * d = dirs_u + (size_t)ray_i * 3;
            const v3 ro = V(o[0], o[1], o[2]), rd = V(d[0], d[1], d[2]);
            const uint32_t pkey = pixel_key(P.seed_lo, P.seed_hi, PTK_RAYS_KEY(ray_i));
            rng.inc = (hash32(pkey ^ 0x9E3779B9u) << 1) | 1u;
            rng.state = hash32(P.first_sample + sample_abs + pkey);
            rng.key = rng.state;
            if (R.lens_draws) rng.state = rng.state * (747796405u * 747796405u) + rng.inc * (747796405u + 1u);
            L = V(0.0f, 0.0f, 0.0f); T = V(1.0f, 1.0f, 1.0f);
            depth = 0; iter = 0; inside = false; ray = 0;
            W.occl_tri = -1;
            W.begin(ro, rd, P.num_nodes, stack, P.scene_bound);
        }
        const int n_trav = __popcll(__ballot(st == ST_TRAV)), n_shade = __popcll(__ballot(st == ST_SHADE));
        if (n_trav + n_shade == 0) break;

        // Block choice: trace_kernel's ski-rental rule.  The walk keeps stepping until the lane-iterations wasted by the lanes
        // parked for shading (or waiting for a unit) outweigh lambda x the lanes that running their block would leave idle.
        if (n_trav > 0)
        {
            int ds = __builtin_amdgcn_readfirstlane(debt_shade), dn = __builtin_amdgcn_readfirstlane(debt_need);
            unsigned long long m_tq = __ballot(W.tri_left > 0), m_nr = __ballot(W.node >= 0);
            bool want_shade = false, want_deal = false;
            const WalkParams WP = walk_params(P);          // the loop's share of the parameters, in SGPRs
            NodeRec nrec;
            request_node(WP, W, nrec);                     // one node record in flight across iterations (walk_step)
            do
            {
                const int n_tq = __popcll(m_tq), n_nr = __popcll(m_nr);
                const bool run_tri_arm = (n_tq > 0) & ((n_nr == 0) | (n_tq * 8 >= WP.tri_thr * n_nr));
                if (st == ST_TRAV)
                {
                    walk_step<false, PTK_RAYS_BLOCK, true>(WP, W, rng, ray, stack, cnt, run_tri_arm, &nrec);
                    if (W.done()) PTK_WALK_DONE();
                }
                m_tq = __ballot(W.tri_left > 0); m_nr = __ballot(W.node >= 0);
                const int nt = __popcll(m_tq | m_nr);
                const int ns = __popcll(__ballot(st == ST_SHADE));
                // (once the counter has run dry a finished path leaves its lane DONE, not in NEED: no debt)
                const int nn = __popcll(__ballot(st == ST_NEED));
                const int nl = nt + ns + nn;
                ds += ns; dn += nn;
                want_shade = (ns > 0) & (ds * 8 >= WP.shade_thr * (nl - ns));
                want_deal = (nn > 0) & (dn * 8 >= WP.gen_thr * (nl - nn));
                if (want_shade | want_deal | (nt == 0)) break;
            } while (true);
            debt_shade = ds; debt_need = dn;
            if (!want_shade)
            {
                // the lanes in NEED are dealt at the top of the loop, whichever exit it was
                debt_need = 0;
                continue;
            }
        }
        debt_shade = 0;
        if (st == ST_SHADE)
        {
            // ---- one surface interaction of PathTracer::Trace, pathtracer.cpp:551-727 ----
            const bool ended = shade_interaction<false, false, false, false>(P, W, W, stack, rng, L, T, Tdi, nextDir, depth, iter, inside, ray, cnt);
            if (ended) PTK_FINISH_PATH();
            else st = ST_TRAV;
        }
    }
#undef PTK_WALK_DONE
#undef PTK_FINISH_PATH
}
#undef PTK_RAYS_KEY
