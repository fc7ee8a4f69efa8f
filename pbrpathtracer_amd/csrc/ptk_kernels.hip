// HIP kernels for gfx950 (CDNA4, wave64): the per-pixel render loop of the reference
//   PathTracer::RenderFrame -> Trace -> Hit -> {IntersectTriangle, Image::tex2D, DirectIllumimation}
//   (reference PathTracing/src/pathtracer.cpp:367-822, mesh.cpp:48-59, image.cpp:63-86)
// as a path-tracing kernel of persistent waves (trace_kernel: one path per lane) followed by a streaming
// accumulate_kernel.  This file holds what is compiled once per arithmetic level (below): the trace kernels, what only they use,
// the queue set-up, probe_math_kernel.  The shared device functions (v3, the exact arithmetic, the RNG, tex2d, the walk) are in
// ptk_device_fn.h; accumulate_kernel and the other kernels that exist once are in ptk_frame.hip.
//
// Design (not a translation of the reference's recursion):
//   * Trace is iterative: L += T*e; L += T*direct; T *= weight, with the reference's two counters
//     (depth arms Russian roulette, iter is the hard stop) and its quirks kept.
//   * Work item = (8x8 pixel quadrant, chunk of samples); work unit = (live pixel of it, sample): parallel over
//     pixels AND samples, so a frame with few non-trivial pixels still fills 256 CUs.  Units are dealt to
//     whichever lane needs work; the waves are persistent and pull items from per-XCD queues built over a
//     device-side list of the quadrants that have live pixels (live_mask_kernel / live_compact_kernel), so all
//     64 lanes of every wave trace until the launch runs dry.  Each finished path stores its radiance as one
//     float4 into a sample buffer in HBM; accumulate_kernel then folds the samples of a pixel into the float
//     accumulator strictly in sample order (the reference's one-add-per-RenderFrame semantics,
//     pathtracer.cpp:798-800) and writes the RGB8 resolve.
//   * A lane is a state machine {NEED, GEN, TRAV, SHADE, DONE}.  Every wave iteration takes a 64-bit ballot per
//     state and runs one block: the BVH walk keeps stepping (node arm every iteration, triangle arm when enough
//     lanes hold a leaf; bounce and shadow rays share the walk; a finished shadow ray rolls straight into the
//     bounce ray) until the lane-iterations wasted by lanes parked for shading / a camera ray outweigh the
//     lanes that block would leave idle.  Divergent blocks therefore run with full-ish EXEC masks instead of
//     once per ray.  Scenes of <= 16 triangles skip the hierarchy (FLAT: scalar triangle loads, shadow and
//     bounce ray in one pass).
//   * Closest hit: 4-wide BVH, one 64-byte record per node holding the four child boxes quantised OUTWARD to 8 bits on
//     the node's own grid (t = fma(q, A, B) per plane), nearest child first, the others on a per-lane stack in LDS laid
//     out [level][lane] (conflict-free ds_read/write_b32); the node record is requested before the triangle arm runs.
//     Result = min over accepted triangles with an order-independent tie rule, so it does not depend on the tree (the
//     reference's own tree is random, mesh.cpp:171-172).  Box tests are acceleration only, so they use v_rcp and fused
//     multiply-adds - but they are CONSERVATIVE for any ray origin and triangle size (explicit slack for the slab
//     arithmetic's absolute error and for Moeller-Trumbore's own error in t, see walk_step); everything that reaches the
//     image (Moeller-Trumbore, shading, samplers) is IEEE and in the reference's order, with 1/x and sqrt as short
//     sequences proven bit-identical by enumeration (rcp_ieee, sqrt_ieee).
//   * Shadow rays keep the reference's closest-hit + identity test (pathtracer.cpp:522-526): the light triangle is
//     tested first (its record comes with the light sample), then any hit the closest-hit rule accepts is nearer and
//     ends the walk (Walk::occl_tri).
//   * Pinhole cameras without opacity textures: the camera ray's hit is cached per pixel, pixels whose camera ray
//     misses are never traced, and a new path starts directly in the SHADE block.
//   * RNG: PCG-RXS-M-XS-32 per path, keyed on (seed, pixel, sample) - never on lane/block/GPU.
//
// Float arithmetic is written operation by operation in the reference's order and this file is
// compiled with -ffp-contract=off: results are reproducible against the CPU oracle bit for bit.
//
// This file is compiled THREE times into libptk.so.  PTK_CONTRACT 0 (default): -ffp-contract=off, the bit-exact product kernels
// in namespace ptk.  PTK_CONTRACT 1: the same trace kernels in namespace ptk::fma, built with -ffp-contract=fast (the compiler
// fuses a * b + c into v_fma_f32 wherever it appears: Moeller-Trumbore, dot products, normalisations, shading) for the
// "contract" option of ptk_set_option; PTK_CONTRACT 2 (ptk::fast) also takes 1 / x, sqrt and 1 / sqrt straight from the
// hardware's v_rcp / v_sqrt / v_rsq (within 1 ulp of the correctly rounded result, tests/test_gpu_exact_math.py).  No longer
// bit-identical to the oracle, but held to it sample by sample (tests/test_gpu_contract_samples.py: nearly every sample within
// 1e-4 relative of the exact kernels' and no bias among those; the rest took another branch or texel) and to the mean image's
// tolerance (tests/test_gpu_contract.py); and still reproducible bit for bit, whatever the work distribution, passes or tiles.
// Each build has its own probe_math_kernel (ptk_probe_math follows the option).  (The header defaults PTK_CONTRACT to 0.)
// A fourth time, through ptk_kernels_plain.hip, for the exact build's two PLAIN instantiations alone (PTK_PLAIN_UNIT, below the kernel),
// and a fifth, through ptk_kernels_rect.hip, for the same two with the pair pass in front of the record loop (PTK_RECT_UNIT),
// and a sixth, through ptk_kernels_cycle.hip, for those two around another main loop (PTK_CYCLE_UNIT, ptk_trace_cycle.h).

#include "ptk_device_fn.h"
#include "ptk_flat_mt.h"

namespace ptk {
#if PTK_CONTRACT >= 2
namespace fast {
#elif PTK_CONTRACT
namespace fma {
#endif

#define PTK_TRACE_BLOCK 64          // trace_kernel: one wave per workgroup -> finest-grained dispatch
#ifndef PTK_TRACE_WAVES
#define PTK_TRACE_WAVES 5           // waves per SIMD the register allocator must allow, FLAT variant: 96 VGPRs (4 spilled) since the parameters
                                    // are read through the constant address space; C2 +3.4-4.5 %, C1 +4 % over four waves (six: 80 VGPRs, 37 spilled, -6 %)
#endif
#ifndef PTK_TRACE_WAVES_PLAIN
#define PTK_TRACE_WAVES_PLAIN 5     // ... its PLAIN variant: 72 VGPRs and nothing spilled at five, six and seven alike.  Seven make an isolated C2 launch
                                    // 3 % shorter and leave ms_per_step where it is (consecutive launches share the chip either way): five stay
#endif
#ifndef PTK_TRACE_WAVES_BVH
#define PTK_TRACE_WAVES_BVH 4       // ... BVH variant
#endif

// FLAT pass, both rays of a lane against one triangle in PACKED f32: x = the bounce ray (W), y = the shadow ray (WS).
// Every Moeller-Trumbore operation is the same IEEE mul / add / sub as in tri_test, on two values at once
// (v_pk_mul_f32 / v_pk_add_f32 run at the rate of their scalar forms; the triangle's words come from SGPRs), which
// nearly halves the instructions of the hottest loop of the Cornell configs.  No early returns: all quantities are
// computed and the reference's tests AND-ed in their negated form, exactly as tri_test does.  Returns true when the
// shadow ray has been decided by an occluder.
// (ox, oy, oz are not read - both rays leave W.ro, see tri_test_pair - but dropping them reorders a few moves of the kernels)
struct RayPair { f2 ox, oy, oz, dx, dy, dz; };

// The arithmetic of the test for both rays: ptk_flat_mt.h's mt_pair (shared with the host-side check of the masks) on the packed pair.
// ZM (exact PLAIN pass only): the record's edge words that are known to be stored zeros, whose operations are deleted; ZM = 0 is
// the full text.  u, v of a hit may then differ from the full test's in the sign of a zero, and nothing of a PLAIN scene reads them.
template <unsigned ZM>
__device__ __forceinline__ void tri_math_pair(const Walk& W, const RayPair& R, float4 t0, float4 t1, float4 t2, f2& a, f2& u, f2& v, f2& t)
{
    ptk_mt::mt_pair<ZM>(R.dx, R.dy, R.dz, W.ro.x, W.ro.y, W.ro.z, t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x,
                        [](const f2& x) { return f2{ rcp_ieee(x.x), rcp_ieee(x.y) }; }, a, u, v, t);
}

// ... and what follows it: the reference's tests, the closest-hit rule, stochastic opacity, the hit records.
// PLAIN (trace_kernel): no triangle of the scene has an opacity texture, so the opacity branch is dead code.
template <bool STATS, bool PLAIN, class PT>
__device__ __forceinline__ bool tri_accept_pair(const PT& P, Walk& W, Walk& WS, const bool shadow_live, const f2 a, const f2 u, const f2 v, const f2 t,
                                                float4 t2, const Rng& rng, uint32_t ray_bounce, uint32_t ray_shadow, Counters& cnt)
{
    const f2 uv = u + v;
    const int tri = __float_as_int(t2.y);
    const int otex = __float_as_int(t2.z);
    bool okb = ptk_mt::mt_accept(a.x, u.x, v.x, uv.x, t.x, PTK_EPS);
    bool oks = ptk_mt::mt_accept(a.y, u.y, v.y, uv.y, t.y, PTK_EPS);
    // the flat list is in ascending triangle index, so the tie rule's "equal t and smaller index" can never hold for a
    // later record: nearer-than-best is the whole rule
    okb = okb & (t.x < W.best.t);
    oks = oks & shadow_live & (t.y < WS.best.t);
    if (!PLAIN && (okb | oks) && otex >= 0)
    {
        // stochastic opacity, pathtracer.cpp:469-476 (GetUV :533-536); rare: skipped with s_cbranch_execz
        const float4* sp4 = P.shade + (size_t)tri * SHADE_F4;
        const float4 s1 = ldg4(sp4 + 1), s2 = ldg4(sp4 + 2);
        if (okb)
        {
            const float w = 1.0f - u.x - v.x;
            const float op = tex2d_r(P, otex, w * s1.x + u.x * s1.z + v.x * s2.x, w * s1.y + u.x * s1.w + v.x * s2.y);
            if (STATS) cnt.tex++;
            okb = rng.opacity(ray_bounce, (uint32_t)tri) < op;
        }
        if (oks)
        {
            const float w = 1.0f - u.y - v.y;
            const float op = tex2d_r(P, otex, w * s1.x + u.y * s1.z + v.y * s2.x, w * s1.y + u.y * s1.w + v.y * s2.y);
            if (STATS) cnt.tex++;
            oks = rng.opacity(ray_shadow, (uint32_t)tri) < op;
        }
    }
    // (exec-masked moves - full rate - instead of four half-rate selects per ray; skipped outright when no lane accepts.
    // C2 +1 %; the same in the BVH walk's tri_test measured +-0, so that one keeps its selects)
    if (okb) { W.best.tri = tri; W.best.t = t.x; W.best.u = u.x; W.best.v = v.x; asm volatile("" : "+v"(W.best.t), "+v"(W.best.u), "+v"(W.best.v)); }
    if (oks) { WS.best.tri = tri; WS.best.t = t.y; WS.best.u = u.y; WS.best.v = v.y; asm volatile("" : "+v"(WS.best.t), "+v"(WS.best.u), "+v"(WS.best.v)); }
    return oks & (tri != WS.occl_tri);
}

#ifdef PTK_RECT_UNIT
// The pair pass of ptk_kernels_rect.hip: both records of a fan-split axis-aligned rectangle of kind KIND from v0 and e2 of the first
// (ptk_flat_mt.h mt_rect_pair: the same arithmetic, B's words named as A's, the sharing left to the compiler) ...
template <int KIND>
__device__ __forceinline__ void tri_math_rect(const Walk& W, const RayPair& R, float v0x, float v0y, float v0z, float e2x, float e2y, float e2z,
                                              f2& aA, f2& uA, f2& vA, f2& tA, f2& aB, f2& uB, f2& vB, f2& tB)
{
    ptk_mt::mt_rect_pair<KIND>(R.dx, R.dy, R.dz, W.ro.x, W.ro.y, W.ro.z, v0x, v0y, v0z, e2x, e2y, e2z,
                               [](const f2& x) { return f2{ rcp_ieee(x.x), rcp_ieee(x.y) }; }, aA, uA, vA, tA, aB, uB, vB, tB);
}
// ... and the accept of the two of them for one ray (PLAIN: no opacity), ptk_flat_mt.h mt_rect_accept_once: the nine predicates as WAVE
// MASKS - one compare each, straight into a scalar register pair, joined with scalar and / or.  Written as `bool & bool` on lane values the
// compiler folds each pair of sign tests into v_max, v_max, v_min and one compare (four half-rate instructions for two), and the two
// records' accepts into two masked regions per ray where one does.  The predicates keep their NaN behaviour: !(x < y) is the compare
// "unordered or >=" (v_cmp_nlt_f32), !(x > y) "unordered or <=" (v_cmp_ngt_f32), t > eps and t < best the ordered ones.
// The caller stands inside `if (st == ST_TRAV)`: a mask compare returns bits for the lanes that execute it only, so every mask here is
// a subset of exec, the same value in every lane, and the inverse ballot - which takes a wave-uniform mask - turns it back into a lane
// condition whose region closes as any `if` does.
#define PTK_MASK_NLT(x, y) __builtin_amdgcn_fcmpf(x, y, 11)          // FCMP_UGE
#define PTK_MASK_NGT(x, y) __builtin_amdgcn_fcmpf(x, y, 13)          // FCMP_ULE
#define PTK_MASK_GT(x, y) __builtin_amdgcn_fcmpf(x, y, 2)            // FCMP_OGT
#define PTK_MASK_LT(x, y) __builtin_amdgcn_fcmpf(x, y, 4)            // FCMP_OLT
__device__ __forceinline__ void rect_accept_masks(float a, float t, float uA, float vA, float uvA, float uB, float vB, float uvB, float best_t,
                                                  unsigned long long& hit, unsigned long long& first)
{
    const unsigned long long X = PTK_MASK_NLT(__builtin_fabsf(a), PTK_EPS) & PTK_MASK_GT(t, PTK_EPS) & PTK_MASK_LT(t, best_t);
    const unsigned long long inA = PTK_MASK_NLT(uA, 0.0f) & PTK_MASK_NLT(vA, 0.0f) & PTK_MASK_NGT(uvA, 1.0f);
    const unsigned long long inB = PTK_MASK_NLT(uB, 0.0f) & PTK_MASK_NLT(vB, 0.0f) & PTK_MASK_NGT(uvB, 1.0f);
    hit = X & (inA | inB);
    first = inA;
}
#undef PTK_MASK_NLT
#undef PTK_MASK_NGT
#undef PTK_MASK_GT
#undef PTK_MASK_LT
// One update per ray: A and B share t and B is accepted only when A is not, so best.t = t and the index is A's or B's by inA - B's is
// A's + 1 (the classifier pairs no other records), so it is B's minus the lane's bit of inA: a 0 / 1 select and a subtraction, where
// choosing between two scalar indices takes two moves first.  (u, v of the hit are not kept: nothing of a PLAIN scene reads them.)
// The empty asm makes the update a masked move and not a select.
__device__ __forceinline__ void tri_accept_rect(Walk& W, Walk& WS, const bool shadow_live, const f2 a, const f2 t, const f2 uA, const f2 vA,
                                                const f2 uB, const f2 vB, const int triA)
{
    const f2 uvA = uA + vA, uvB = uB + vB;
    const int triB = triA + 1;
    unsigned long long hb, fb, hs, fs;
    rect_accept_masks(a.x, t.x, uA.x, vA.x, uvA.x, uB.x, vB.x, uvB.x, W.best.t, hb, fb);
    rect_accept_masks(a.y, t.y, uA.y, vA.y, uvA.y, uB.y, vB.y, uvB.y, WS.best.t, hs, fs);
    if (__builtin_amdgcn_inverse_ballot_w64(hb))
    {
        W.best.tri = triB - (int)__builtin_amdgcn_inverse_ballot_w64(fb); W.best.t = t.x;
        asm volatile("" : "+v"(W.best.t));
    }
    if (__builtin_amdgcn_inverse_ballot_w64(hs) & shadow_live)
    {
        WS.best.tri = triB - (int)__builtin_amdgcn_inverse_ballot_w64(fs); WS.best.t = t.y;
        asm volatile("" : "+v"(WS.best.t));
    }
}
#endif

template <bool STATS, bool PLAIN, class PT>
__device__ __forceinline__ bool tri_test_pair(const PT& P, Walk& W, Walk& WS, const RayPair& R, const bool shadow_live, float4 t0, float4 t1,
                                              float4 t2, const Rng& rng, uint32_t ray_bounce, uint32_t ray_shadow, Counters& cnt)
{
    if (STATS) cnt.tris += shadow_live ? 2u : 1u;
    f2 a, u, v, t;
    tri_math_pair<0u>(W, R, t0, t1, t2, a, u, v, t);
    return tri_accept_pair<STATS, PLAIN>(P, W, WS, shadow_live, a, u, v, t, t2, rng, ray_bounce, ray_shadow, cnt);
}

// ---- work distribution shared by the persistent trace kernels -------------------------------------------------------
// the current item: read only when units are dealt, so it lives in LDS, not in registers the hot loops want
enum { IT_NLIVE = 0, IT_X0, IT_Y0, IT_SBEGIN, IT_OUTBASE,
       IT_STEAL,                // queues (group + steal) & 7 ... are the ones not yet seen empty; 8 = none left
       IT_LO, IT_HI, IT_G,      // slots [lo, hi) of queue g this wave has popped and not yet used
       IT_REMAIN,               // slots that queue had left after that pop (sizes the next batch)
       IT_TAKEN,                // items this wave has traced so far (against the launch's per-wave quota, if any)
       IT_NLIVE_MAGIC,          // ceil(2^32 / live pixels): unit / live pixels = mulhi(unit, magic), exact while unit * live pixels < 2^32
       IT_WORDS };

// Takes the next non-empty work item from the per-XCD queues (-> lds_item, lds_pixel_of_rank); returns its unit count, 0
// when every queue is empty (or this wave's quota of a multi-generation launch is used up).  Wave-uniform; one wave per
// workgroup.
template <class PT>
__device__ __forceinline__ uint32_t acquire_work_item(const PT& P, uint32_t* lds_item, unsigned char* lds_pixel_of_rank, const int lane)
{
    // the launch geometry is re-read from the queue block (one coalesced load, fields broadcast with
    // v_readlane) instead of living in SGPRs across the hot loops, where it forced spills
    const int geo = ((const int*)(P.queues + 8 * PTK_QUEUE_STRIDE))[lane & 15];
    const int num_chunks = __builtin_amdgcn_readlane(geo, QG_NUM_CHUNKS), world = __builtin_amdgcn_readlane(geo, QG_WORLD);
    const int rank = __builtin_amdgcn_readlane(geo, QG_RANK);
    const int tiles_x = __builtin_amdgcn_readlane(geo, QG_TILES_X), chunk = __builtin_amdgcn_readlane(geo, QG_CHUNK);
    const uint32_t spp = (uint32_t)__builtin_amdgcn_readlane(geo, QG_SPP);
    const int slots_per_queue = __builtin_amdgcn_readlane(geo, QG_SLOTS), live_count = __builtin_amdgcn_readlane(geo, QG_LIVE_COUNT);
    // multi-GPU runs launch several generations of waves, each retiring after its quota of items, so that the
    // kernels of the exchange step (RCCL, on another stream) find free wave slots while this kernel is running
    const uint32_t quota = (uint32_t)__builtin_amdgcn_readlane(geo, QG_QUOTA);
    const int my_group = (int)blockIdx.x & 7;
    int steal = (int)lds_item[IT_STEAL];
    int lo = (int)lds_item[IT_LO], hi = (int)lds_item[IT_HI], cur_g = (int)lds_item[IT_G];
    uint32_t remain = lds_item[IT_REMAIN];
    const int pullers = max(1, (int)gridDim.x >> 3);           // waves that share one queue
    if (quota != 0u && lds_item[IT_TAKEN] >= quota && lo >= hi) steal = 8;
    for (;;)
    {
        while (lo >= hi && steal < 8)
        {
            // pop the next slot(s).  P.max_batch > 1 pops guided batches (a share of what is left per puller,
            // shrinking towards the end); measured slower on every config - consecutive slots are the chunks of
            // ONE quadrant, which are better traced by several waves at the same time - so the default is 1
            const int g = (my_group + steal) & 7;
            // (what the queue had left after this wave's previous pop has roughly halved since: the other
            // pullers popped meanwhile)
            const uint32_t left = g == cur_g && remain != 0xffffffffu ? remain / 2u : (uint32_t)slots_per_queue;
            const int want = max(1, min(P.max_batch, (int)(left / (4u * (uint32_t)pullers))));
            int old = 0;
            if (lane == 0) old = (int)atomicAdd(&P.queues[g * PTK_QUEUE_STRIDE], (unsigned)want);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old < slots_per_queue)
            {
                lo = old; hi = min(slots_per_queue, old + want); cur_g = g;
                remain = (uint32_t)(slots_per_queue - hi);
                break;
            }
            // this queue is empty: look at all eight counters at once (one load) and move on to the next
            // one that still has items, instead of finding each of them empty with an atomic of its own
            unsigned seen = ~0u;
            if (lane < 8) seen = __hip_atomic_load(&P.queues[((my_group + lane) & 7) * PTK_QUEUE_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned avail = (unsigned)__ballot(seen < (unsigned)slots_per_queue) & 0xffu & (0xffu << (steal + 1));
            steal = avail ? __builtin_ctz(avail) : 8;
            if (steal < 8)
            {
                // size the first pop from the victim by what it was just seen to have left
                cur_g = (my_group + steal) & 7;
                remain = 2u * ((uint32_t)slots_per_queue - (uint32_t)__builtin_amdgcn_readlane((int)seen, steal));
            }
        }
        if (lo >= hi) break;
        const int slot = lo++;
        if (slot >= slots_per_queue) continue;                             // (one-item-per-wave mode: surplus block)
        // slot -> (entry of the live list, chunk): a queue holds runs of four consecutive entries - the
        // quadrants of one tile, as a rule - so that tile is traced within one XCD
        const int e = slot / num_chunks, chunk_id = slot - e * num_chunks;
        const int v = ((e >> 2) * 8 + cur_g) * 4 + (e & 3);
        if (v >= live_count) continue;                                     // padding of the last runs
        const int subtile = (int)P.live_list[v];                           // (owned tile) * 4 + quadrant
        const unsigned long long live_mask = P.live_mask[subtile];         // its pixels that need tracing
        const int item = subtile * num_chunks + chunk_id;
        const int owned = subtile >> 2, quad = subtile & 3;
        const int tile = owned * world + rank;
        int tx, ty; tile_origin(tile, tiles_x, tx, ty);
        const int x0 = tx * PTK_TILE + (quad & 1) * 8, y0 = ty * PTK_TILE + (quad >> 1) * 8;
        const uint32_t s_begin = (uint32_t)chunk_id * (uint32_t)chunk;
        const uint32_t s_count = min((uint32_t)chunk, spp - s_begin);      // host guarantees s_begin < spp
        const uint32_t n_live = (uint32_t)__popcll(live_mask);
        if (n_live == 0) continue;
        __syncthreads();                    // every lane is done with the previous item's table
        if ((live_mask >> lane) & 1ull) lds_pixel_of_rank[__popcll(live_mask & ((1ull << lane) - 1ull))] = (unsigned char)lane;
        if (lane == 0)
        {
            lds_item[IT_NLIVE] = n_live; lds_item[IT_NLIVE_MAGIC] = (uint32_t)((0x100000000ull + n_live - 1u) / n_live); lds_item[IT_X0] = (uint32_t)x0; lds_item[IT_Y0] = (uint32_t)y0;
            lds_item[IT_SBEGIN] = s_begin; lds_item[IT_STEAL] = (uint32_t)steal; lds_item[IT_TAKEN] += 1u;
            lds_item[IT_LO] = (uint32_t)lo; lds_item[IT_HI] = (uint32_t)hi; lds_item[IT_G] = (uint32_t)cur_g; lds_item[IT_REMAIN] = remain;
            lds_item[IT_OUTBASE] = (uint32_t)item * (uint32_t)chunk * 64u;   // sample s of quadrant pixel q: P.samples[base + s * 64 + q]
        }
        __syncthreads();
        return n_live * s_count;
    }
    if (lane == 0) { lds_item[IT_STEAL] = 8u; lds_item[IT_LO] = lds_item[IT_HI] = 0u; }
    __syncthreads();
    return 0u;
}

// (the two states that wait for a camera ray - no unit yet, unit dealt - are the two smallest: one compare counts both)
enum : int { ST_NEED = 0, ST_GEN = 1, ST_TRAV = 2, ST_SHADE = 3, ST_DONE = 4 };

// FLAT = the scene has so few triangles (P.flat_count <= 16) that no hierarchy is walked: a traversing
// lane tests every triangle, the records are fetched with SCALAR loads (one s_load per triangle per
// wave, operands broadcast from SGPRs, no vector memory traffic and no LDS stack), and the whole walk
// is one block of the state machine, so lanes re-synchronise by themselves.
// PLAIN = a FLAT scene that is also opaque, untextured, flat-shaded, without opacity textures and seen through a cached pinhole
// camera (ptk_api.hip decides, see RenderParams::plain): the same text with everything such a scene cannot reach compiled out -
// textures, UVs, smoothed / mapped normals, stochastic opacity and its two keys per pass, the glass branch, the camera-ray block.
// The route it does take is untouched, so its samples are bit-identical to the generic kernel's.
// LAMBERT = a PLAIN scene in which no material has reflectiveness > 0 (RenderParams::lambert): the specular draw can never succeed,
// so shade_interaction keeps its advance of the stream and the diffuse route alone, and `iter`, equal to `depth`, is not carried.
template <bool STATS, bool FLAT, bool PLAIN, bool LAMBERT = false>
__global__ __launch_bounds__(PTK_TRACE_BLOCK, (PLAIN ? PTK_TRACE_WAVES_PLAIN : FLAT ? PTK_TRACE_WAVES : PTK_TRACE_WAVES_BVH)) void trace_kernel(const RenderParams* __restrict__ Pp)
{
    // the parameters live in the launch's queue block, in the constant address space: fields are s_load-ed where they are
    // used instead of being preloaded whole into SGPRs (ptk_device.h: 30 / 42 SGPR spills -> 0)
    typedef const __attribute__((address_space(4))) RenderParams ConstParams;
    ConstParams& P = *(ConstParams*)(uintptr_t)Pp;
    static_assert(FLAT || !PLAIN, "PLAIN is a variant of the FLAT kernel");
    static_assert((PLAIN && !STATS) || !LAMBERT, "LAMBERT is a level of the PLAIN kernel; the STATS kernels count the generic route");
    __shared__ int lds_stack[FLAT ? 1 : PTK_STACK_ROWS * PTK_TRACE_BLOCK];
    if (P.exit_flag && __hip_atomic_load(P.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.exit_gen) return;     // an Exit() named this render or a later one

    const int tid = threadIdx.x;
    int* stack = lds_stack + tid;
    const int lane = tid & 63;
    // ---- work distribution -------------------------------------------------------------------------
    // Work item = (owned 16x16 tile, 8x8 quadrant, chunk of samples); its work UNITS = (live pixel of the
    // quadrant, sample of the chunk), sample-major.  Units are dealt to whichever lane needs work next, NOT
    // pinned pixel-to-lane, and the waves are PERSISTENT: a wave that has dealt the last unit of its item
    // takes the next item from a queue while its other lanes are still finishing paths of the previous one,
    // so all 64 lanes keep tracing until the whole launch runs dry (a lane's state carries its own pixel,
    // sample and output slot).  A pixel-per-lane mapping idled the wave while its unluckiest pixel finished
    // its samples, and a wave per item left a tail at the end of every item.
    //
    // XCD-aware queues: workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one), each
    // with its own L2.  There is one queue per XCD group, holding whole 16x16 tiles (runs of 4 x num_chunks
    // items) tile by tile round-robin, so the waves that trace the same pixels - the same BVH nodes and
    // triangles - share an L2; a group whose queue is empty steals from the others.  (One contiguous eighth
    // of the frame per XCD was 2x slower when the dispatcher dealt the items: cheap and dear regions.)
    static_assert(PTK_TRACE_BLOCK == 64, "one wave per workgroup");
    __shared__ unsigned char lds_pixel_of_rank[64];
    __shared__ uint32_t lds_item[IT_WORDS];
    if (lane == 0)
    {
        // small launches (P.persistent == 0: few items per wave slot) run one item per wave, named by blockIdx,
        // with no queue traffic at all - the hardware dispatcher balances those better than 4096 waves
        // contending for eight counters could
        lds_item[IT_STEAL] = P.persistent ? 0u : 8u;
        lds_item[IT_LO] = P.persistent ? 0u : (uint32_t)blockIdx.x >> 3;
        lds_item[IT_HI] = P.persistent ? 0u : ((uint32_t)blockIdx.x >> 3) + 1u;
        lds_item[IT_G] = (uint32_t)blockIdx.x & 7u;
        lds_item[IT_REMAIN] = 0xffffffffu;      // "unknown": the first pop is sized from the whole queue
        lds_item[IT_TAKEN] = 0u;
    }
    __syncthreads();
    uint32_t total_units = 0, next_unit = 0;    // wave-uniform
    // per-lane: the unit this lane is tracing
    uint32_t pix = 0;               // row-major pixel index from the top
    uint32_t sample_abs = 0;        // sample index inside this launch (chunk start + index in the chunk)
    uint32_t out_idx = 0;           // its slot in the sample buffer

    // takes the next non-empty item (-> lds_item, lds_pixel_of_rank); returns its unit count, 0 when every queue is empty
    auto acquire_item = [&]() -> uint32_t { return acquire_work_item(P, lds_item, lds_pixel_of_rank, lane); };

    const v3 camPos0 = V(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    const v3 camRight = V(P.cam_right[0], P.cam_right[1], P.cam_right[2]);
    const v3 camUp = V(P.cam_up[0], P.cam_up[1], P.cam_up[2]);

    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    Rng rng;
    rng.inc = 1u; rng.state = 0; rng.key = 0;

    // per-lane path state
    Walk W;
    W.begin(camPos0, V(0.0f, 0.0f, 1.0f), 0, stack, 0.0f);
    W.occl_tri = -1;
    Walk WS;                        // FLAT only: the shadow ray, tested in the same pass as the bounce ray
    WS.begin(camPos0, V(0.0f, 0.0f, 1.0f), 0, stack, 0.0f);
    WS.occl_tri = -1;
    v3 L = V(0.0f, 0.0f, 0.0f), T = V(1.0f, 1.0f, 1.0f);
    v3 Tdi = V(0.0f, 0.0f, 0.0f), nextDir = V(0.0f, 0.0f, 1.0f);
    int depth = 0, iter = 0;
    bool inside = false;
    uint32_t ray = 0;
    int st = ST_NEED;               // every lane works, whatever its own pixel is

    // (what the walk loop's exits read of the parameters, in SGPRs for the kernel's life: see WalkParams)
    float4* const samples_u = uniform_ptr(P.samples);
    const int num_nodes_u = __builtin_amdgcn_readfirstlane(P.num_nodes);
    const float scene_bound_u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.scene_bound)));
    // (the cycle unit, ptk_kernels_cycle.hip, holds more of them there: see ptk_trace_cycle.h)
#ifdef PTK_CYCLE_UNIT
    const int max_depth_u = __builtin_amdgcn_readfirstlane(P.max_depth);
#define PTK_U_MAX_DEPTH max_depth_u
#else
#define PTK_U_MAX_DEPTH P.max_depth
#endif
    // a finished path: its radiance goes to the sample buffer, the lane moves to its next sample
#define PTK_FINISH_PATH()                                                                         \
    do {                                                                                          \
        samples_u[out_idx] = make_float4(L.x, L.y, L.z, 0.0f);                                    \
        st = ST_NEED;                                                                             \
    } while (0)

    // a finished walk: shadow rays resolve DirectIllumimation's visibility and roll into the sampled
    // bounce; bounce rays end the path on a miss or queue for shading.
    // FLAT: a hit whose interaction would be the terminal one (pathtracer.cpp:571, `iter` does not change between
    // shade_interaction and here) ends the path like a miss: that interaction sets `ended` before any draw, any
    // emission, any write to L, and the pass has folded the shadow ray into L already.  Parked in SHADE instead,
    // the lane took a slot of a shade block for nothing, was dealt its next unit after that block and sat out
    // the whole following pass.  (The STATS kernels keep the parked route: their shade_lanes counts executed
    // interactions and equals hits_shaded, which includes the terminal one.)
#define PTK_WALK_DONE()                                                                           \
    do {                                                                                          \
        if (STATS) { cnt.rays++; cnt.max_nodes = max(cnt.max_nodes, cnt.cur_nodes); cnt.cur_nodes = 0; }     \
        ray++;                                                                                    \
        const bool hit_ = W.best.tri != PTK_NOHIT;                                                \
        if (W.occl_tri >= 0)                                                                      \
        {                                                                                         \
            /* pathtracer.cpp:522-526: lit unless something else is closest */                    \
            if (STATS) cnt.shadow++;                                                              \
            if (!(hit_ && W.best.tri != W.occl_tri)) L = add(L, Tdi);                             \
            W.occl_tri = -1;                                                                      \
            W.begin(W.ro, nextDir, num_nodes_u, stack, scene_bound_u);                                   \
        }                                                                                         \
        else if (!hit_ || (FLAT && !STATS && !((LAMBERT ? depth : iter) < PTK_U_MAX_DEPTH))) PTK_FINISH_PATH();     /* :550 miss -> black */  \
        else st = ST_SHADE;                                                                       \
    } while (0)

#ifdef PTK_CYCLE_UNIT
    // the cycle unit's main loop: a fixed shade / pass cycle around the same two blocks, units dealt from scalar registers
#include "ptk_trace_cycle.h"
#else
    int debt_shade = 0, debt_gen = 0;      // wave-uniform: lane-iterations wasted by parked lanes
    for (;;)
    {
        // deal the next work units to the lanes that need one (wave-uniform code)
        // FLAT: deal lazily.  The kernel runs in lock-step - shade (all lanes), pass (all but the few whose path just ended),
        // shade ... - and a lane dealt after the shade block only waits in SHADE / GEN for the block after the pass, in front
        // of which the lanes that missed are dealt anyway.  So the deal is skipped while it cannot change the vote below:
        // the pass wins even if every NEED lane is counted for its strongest rival.  A dealt lane lands in SHADE, GEN or DONE,
        // so with the deal the pass would have run with the same lanes; only which lane picks up which unit differs.
        // Termination: a skipped iteration has n_trav > 0 and runs the pass (weights are >= 1: the skip test implies the vote),
        // after which no lane of it is in TRAV, so two skips never follow each other and no skip reaches the `break` below
        // (n_live >= n_trav > 0).  With n_trav == 0 the deal always runs, and it leaves no lane in NEED (each gets a unit
        // or, when every queue is empty, DONE): n_live == 0 is only ever seen right after such a deal, with nothing undealt.
        // One-item-per-wave launches and the quota of a multi-GPU share live in acquire_item and see the same calls.
        bool deal = true;
        if (FLAT)
        {
            const int n_need = __popcll(__ballot(st == ST_NEED)), nt = __popcll(__ballot(st == ST_TRAV));
            const int ns = __popcll(__ballot(st == ST_SHADE)), ng = PLAIN ? 0 : __popcll(__ballot(st == ST_GEN));
            deal = nt == 0 || nt * 8 < (ns + n_need) * P.flat_shade_w || (!PLAIN && nt * 8 < (ng + n_need) * P.flat_gen_w);
        }
        if (!FLAT || deal)
        {
            unsigned long long m_need = __ballot(st == ST_NEED);
            while (m_need)
            {
                if (next_unit >= total_units)
                {
                    next_unit = 0;
                    total_units = (lds_item[IT_STEAL] < 8u || lds_item[IT_LO] < lds_item[IT_HI]) ? acquire_item() : 0u;
                    if (total_units == 0) { if (st == ST_NEED) st = ST_DONE; break; }
                }
                const uint32_t n_live = lds_item[IT_NLIVE];
                const uint32_t u = next_unit + (uint32_t)__popcll(m_need & ((1ull << lane) - 1ull));
                if (st == ST_NEED && u < total_units)
                {
                    const uint32_t s_in_chunk = n_live == 1u ? u : __umulhi(u, lds_item[IT_NLIVE_MAGIC]);   // = u / n_live without the integer-division expansion
                    const uint32_t q = lds_pixel_of_rank[u - s_in_chunk * n_live];
                    pix = (lds_item[IT_Y0] + (q >> 3)) * (uint32_t)P.width + lds_item[IT_X0] + (q & 7u);
                    sample_abs = lds_item[IT_SBEGIN] + s_in_chunk;
                    out_idx = lds_item[IT_OUTBASE] + s_in_chunk * 64u + q;
                    // cached camera rays (pinhole, no stochastic opacity): the path starts at its first surface
                    // interaction, so the lane queues for the SHADE block directly and sets its path up there (depth < 0
                    // marks it) - one voted block less to wait for per path, and bigger shading batches
                    st = (PLAIN || P.primary_hit) ? ST_SHADE : ST_GEN;
                    depth = -1;
                }
                next_unit = min(total_units, next_unit + (uint32_t)__popcll(m_need));
                m_need = __ballot(st == ST_NEED);
            }
        }
        const unsigned long long m_trav = __ballot(st == ST_TRAV);
        const unsigned long long m_shade = __ballot(st == ST_SHADE);
        const unsigned long long m_gen = PLAIN ? 0ull : __ballot(st == ST_GEN);      // (PLAIN: no lane is ever in GEN)
        const int n_trav = __popcll(m_trav), n_shade = __popcll(m_shade), n_gen = __popcll(m_gen);
        const int n_live = n_trav + n_shade + n_gen;
        if (n_live == 0) break;

        // Block choice ("ski rental"): a lane parked in SHADE / GEN wastes one lane-iteration for
        // every walk iteration it sits out, while running its block now wastes the lanes that are not
        // parked there.  The walk keeps stepping until the lane-iterations wasted by the parked lanes
        // (debt, accumulated per walk iteration) exceed lambda x the lanes the block would leave idle,
        // with lambda ~ cost(block) / cost(walk step) (P.shade_thr, P.gen_thr in eighths).  Short walks
        // (a bare Cornell box) thus batch ~3/4 of a wave per shade call, deep trees with straggling
        // rays shade small batches early instead of idling - measured optimum in both regimes.
        bool run_shade = n_trav == 0 && n_shade >= n_gen && n_shade > 0;
        bool run_gen = n_trav == 0 && !run_shade;
        if (FLAT)
        {
            // every block is one complete unit of work for a lane: run the one most lanes wait for
            // (weights in eighths: a cheap block may run with fewer lanes than an expensive one)
            const int sc_trav = n_trav * 8, sc_shade = n_shade * P.flat_shade_w, sc_gen = n_gen * P.flat_gen_w;
            if (n_trav > 0 && sc_trav >= sc_shade && sc_trav >= sc_gen)
            {
                if (STATS && lane == 0) { cnt.walk_iters++; cnt.walk_lanes += (uint32_t)n_trav; }
                if (st == ST_TRAV)
                {
#include "ptk_trace_pass.h"
                }
                continue;
            }
            run_shade = n_shade > 0 && (sc_shade >= sc_gen || n_gen == 0);
            run_gen = !run_shade;
        }
        else if (n_trav > 0)
        {
            // ---- BVH walk ----
            // The loop's bookkeeping is wave-uniform and kept to four ballots per iteration: a lane is walking exactly when
            // its walk has a leaf triangle pending or a node to visit (W is `done` in every other state, from W.begin's
            // initial call on), so the two masks that vote the triangle arm also count the walking lanes.
            int ds = __builtin_amdgcn_readfirstlane(debt_shade), dg = __builtin_amdgcn_readfirstlane(debt_gen);
            unsigned long long m_tq = __ballot(W.tri_left > 0), m_nr = __ballot(W.node >= 0);
            bool want_shade = false, want_gen = false;
            const WalkParams WP = walk_params(P);          // the loop's share of the parameters, in SGPRs
            NodeRec nrec;
            request_node(WP, W, nrec);                     // the walk keeps one node record in flight across iterations (walk_step)
            do
            {
                if (STATS) { const uint32_t nt = (uint32_t)__popcll(__ballot(st == ST_TRAV)); if (lane == 0) { cnt.walk_iters++; cnt.walk_lanes += nt; } }
                // arm A (triangles) is voted: about one triangle is tested per four nodes visited, so run
                // every iteration it would execute with ~1/7 of the lanes.  A lane parks its leaf and walks
                // on until it reaches the next leaf; the arm runs once enough lanes wait for it (P.tri_thr
                // eighths of the lanes that still have a node to visit) or nobody can walk on.  Deferring
                // only delays t-max tightening: the closest hit is order-independent.  (Measured: waiting
                // for half of the walking lanes, thr 4, is the optimum - beyond that the rays whose walk
                // is finished but for the parked leaf idle too long; a 4-deep leaf ring per lane made
                // that worse, not better.)
                const int n_tq = __popcll(m_tq), n_nr = __popcll(m_nr);
                const bool run_tri_arm = (n_tq > 0) & ((n_nr == 0) | (n_tq * 8 >= WP.tri_thr * n_nr));      // (bitwise: no scalar branches)
                if (STATS && lane == 0 && run_tri_arm) { cnt.tri_execs++; cnt.tri_lanes += (uint32_t)n_tq; }
                if (st == ST_TRAV)
                {
                    walk_step<STATS, PTK_TRACE_BLOCK, true>(WP, W, rng, ray, stack, cnt, run_tri_arm, &nrec);
                    if (W.done()) PTK_WALK_DONE();
                }
                m_tq = __ballot(W.tri_left > 0); m_nr = __ballot(W.node >= 0);
                const int nt = __popcll(m_tq | m_nr);
                const int ns = __popcll(__ballot(st == ST_SHADE));
                // a lane whose path ended in the walk (its ray left the scene) waits in NEED for a new unit: it runs
                // up the same debt as a lane waiting for the camera-ray block, and is dealt its unit first
                const int ng = __popcll(__ballot(st < ST_TRAV));
                const int nl = nt + ns + ng;
                ds += ns; dg += ng;
                // one exit test per iteration, which exit it was is sorted out after the loop
                want_shade = (ns > 0) & (ds * 8 >= WP.shade_thr * (nl - ns));
                want_gen = (ng > 0) & (dg * 8 >= WP.gen_thr * (nl - ng));
                if (want_shade | want_gen | (nt == 0)) break;
            } while (true);
            if (want_shade) run_shade = true;
            else if (want_gen) run_gen = __ballot(st == ST_NEED) == 0ull;      // NEED lanes: re-vote via the top of the loop
            debt_shade = ds; debt_gen = dg;
            if (!run_shade && !run_gen) continue;        // the walk ran dry: re-vote
        }
        if (run_shade) debt_shade = 0; else debt_gen = 0;
        if (run_shade)
        {
            if (STATS) { const uint32_t nsx = (uint32_t)__popcll(__ballot(st == ST_SHADE)); if (lane == 0) { cnt.shade_execs++; cnt.shade_lanes += nsx; } }
            if (st == ST_SHADE)
            {
#include "ptk_trace_shade.h"
            }
        }
        else if (!PLAIN)
        {
            if (STATS) { const uint32_t ngx = (uint32_t)__popcll(__ballot(st == ST_GEN)); if (lane == 0) { cnt.gen_execs++; cnt.gen_lanes += ngx; } }
            if (st == ST_GEN)
            {
                // ---- camera ray with thin-lens DOF, pathtracer.cpp:785-791 + SampleCircle :734-739 ----
                // (uncached cameras only: a cached camera ray's path starts in the shade block)
                // the pixel's RNG stream constants (pixel_key, increment) come from a per-frame table: they depend on
                // (seed, pixel) only, and four of the five hashes of a path's start went into them
                const uint2 pr = P.pixel_rng[pix];
                const uint32_t pkey = pr.x;
                rng.inc = pr.y;
                rng.state = hash32(P.first_sample + sample_abs + pkey);
                rng.key = rng.state;
                L = V(0.0f, 0.0f, 0.0f); T = V(1.0f, 1.0f, 1.0f);
                depth = 0; iter = 0; inside = false; ray = 0;
                W.occl_tri = -1;
                if (STATS) cnt.started++;
                // per-pixel constants are re-read here (L1/L2 hits) instead of living in registers
                const float4 d0 = P.primary[pix];
                const v3 dir0 = V(d0.x, d0.y, d0.z);
                v3 focalPoint = add(camPos0, muls(dir0, P.focal_dist));
                float r1 = rng.next(), r2 = rng.next();          // always two draws, even with a pinhole
                v3 ro = camPos0;
                if (P.aperture != 0.0f)
                {
                    float angle = (float)((double)r1 * 2. * PTK_PI_D);
                    float radius = sqrt_ieee(r2);
                    float sn, cs;
                    sincos_2pi(angle, sn, cs);
                    float offx = (cs * radius) * P.aperture, offy = (sn * radius) * P.aperture;
                    ro = add(camPos0, add(muls(camRight, offx), muls(camUp, offy)));
                }
                v3 rd = normalize(sub(focalPoint, ro));
                W.begin(ro, rd, P.num_nodes, stack, P.scene_bound);
                st = ST_TRAV;
            }
        }
    }
#endif  // !PTK_CYCLE_UNIT
#undef PTK_WALK_DONE
#undef PTK_FINISH_PATH
#undef PTK_U_MAX_DEPTH
    if (STATS)
    {
        atomicAdd(&P.stats[0], (unsigned long long)cnt.started);
        atomicAdd(&P.stats[1], (unsigned long long)cnt.rays);
        atomicAdd(&P.stats[2], (unsigned long long)cnt.shadow);
        atomicAdd(&P.stats[3], (unsigned long long)cnt.nodes);
        atomicAdd(&P.stats[4], (unsigned long long)cnt.tris);
        atomicAdd(&P.stats[5], (unsigned long long)cnt.shaded);
        atomicAdd(&P.stats[6], (unsigned long long)cnt.tex);
        atomicMax(&P.stats[15], (unsigned long long)cnt.max_nodes);
        if (lane == 0)
        {
            atomicAdd(&P.stats[7], (unsigned long long)cnt.walk_iters);
            atomicAdd(&P.stats[8], (unsigned long long)cnt.walk_lanes);
            atomicAdd(&P.stats[9], (unsigned long long)cnt.shade_execs);
            atomicAdd(&P.stats[10], (unsigned long long)cnt.shade_lanes);
            atomicAdd(&P.stats[11], (unsigned long long)cnt.gen_execs);
            atomicAdd(&P.stats[12], (unsigned long long)cnt.gen_lanes);
            atomicAdd(&P.stats[13], (unsigned long long)cnt.tri_execs);
            atomicAdd(&P.stats[14], (unsigned long long)cnt.tri_lanes);
        }
    }
}

// The exact build's two PLAIN instantiations (generic level and LAMBERT) are emitted by a unit of their own, ptk_kernels_plain.hip:
// this text once more under PTK_PLAIN_UNIT, which leaves only the kernel template and this launcher, compiled with
// -mllvm -structurizecfg-skip-uniform-regions=1 (csrc/Makefile) so that the pass's wave-uniform class switch stays a branch tree whose
// bodies jump straight to the accept chain (DESIGN 4.1 "The pass").  Every other kernel keeps the common command line.
#if !PTK_CONTRACT
void launch_trace_plain(bool lambert, int blocks, hipStream_t stream, const RenderParams* dp);
// ... and once more by ptk_kernels_rect.hip (PTK_RECT_UNIT on top of PTK_PLAIN_UNIT, the same flags): the same two instantiations under
// the name trace_kernel_rect, whose pass tests the list's prefix of fan-split rectangles pair by pair (RenderParams::plain == 2)
void launch_trace_rect(bool lambert, int blocks, hipStream_t stream, const RenderParams* dp);
// ... and by ptk_kernels_cycle.hip (PTK_CYCLE_UNIT on top of both, the PLAIN unit's flags): the pair unit's pass and shade block under
// the name trace_kernel_cycle, in a fixed shade / pass cycle with a scalar unit deal (RenderParams::plain == 3, the flat_cycle option)
void launch_trace_cycle(bool lambert, int blocks, hipStream_t stream, const RenderParams* dp);
#endif
#ifdef PTK_PLAIN_UNIT
#if PTK_CONTRACT
#error "the PLAIN unit belongs to the exact build: the contracted builds keep their PLAIN kernels in ptk_kernels.hip"
#endif
#if defined(PTK_CYCLE_UNIT)
void launch_trace_cycle(bool lambert, int blocks, hipStream_t stream, const RenderParams* dp)
#elif defined(PTK_RECT_UNIT)
void launch_trace_rect(bool lambert, int blocks, hipStream_t stream, const RenderParams* dp)
#else
void launch_trace_plain(bool lambert, int blocks, hipStream_t stream, const RenderParams* dp)
#endif
{
    if (lambert) hipLaunchKernelGGL((trace_kernel<false, true, true, true>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
    else hipLaunchKernelGGL((trace_kernel<false, true, true>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
}
#else

// Probe of the arithmetic helpers as THIS build compiles them (op 0: rcp_ieee, 1: rcp_ieee_any, 2: sqrt_ieee, 3: inv_length,
// the normalisation's factor, 4 / 5: sin / cos of sincos_2pi, 6: sqrt_ieee_rsq, 7: inv_length over it - the two as the cycle
// unit's shade block compiles sqrt_ieee and inv_length): the tests hold the exact build against the host's IEEE results
// and the oracle, the contracted builds against float64 within their documented error.
__global__ __launch_bounds__(PTK_BLOCK) void probe_math_kernel(int op, const float* __restrict__ in, float* __restrict__ out, int n)
{
    const int i = blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    float r;
    if (op == 0) r = rcp_ieee(x);
    else if (op == 1) r = rcp_ieee_any(x);
    else if (op == 2) r = sqrt_ieee(x);
    else if (op == 3) r = inv_length(x);
    else if (op == 6) r = sqrt_ieee_rsq(x);
    else if (op == 7) r = inv_length_rsq(x);
    else {
        float sn, cs;
        sincos_2pi(x, sn, cs);
        r = op == 4 ? sn : cs;
    }
    out[i] = r;
}
void launch_probe_math(int op, const float* d_in, float* d_out, int n, hipStream_t stream)
{
    if (n > 0) hipLaunchKernelGGL(probe_math_kernel, dim3((n + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, op, d_in, d_out, n);
}

struct QueueGeometry { int w[QG_WORDS]; };
static_assert(sizeof(RenderParams) % 4 == 0, "copied word by word");
__device__ __forceinline__ RenderParams* queue_block_params_dev(unsigned* block)
{
    return (RenderParams*)((char*)block + ((8 * PTK_QUEUE_STRIDE + QG_WORDS) * sizeof(unsigned) + 63) / 64 * 64);
}
__global__ void queue_init_kernel(unsigned* block, const QueueGeometry geo, const unsigned* live_count, const RenderParams params)
{
    const int t = threadIdx.x;
    // the launch's parameter block, which the trace kernel reads through the constant address space
    {
        const uint32_t* src = (const uint32_t*)&params;
        uint32_t* dst = (uint32_t*)queue_block_params_dev(block);
        for (int i = t; i < (int)(sizeof(RenderParams) / 4); i += 64) dst[i] = src[i];
    }
    if (t < 8) block[t * PTK_QUEUE_STRIDE] = 0u;
    int w = t < QG_WORDS ? geo.w[t] : 0;
    const int n = (int)*live_count;
    if (t == QG_LIVE_COUNT) w = n;
    if (t == QG_SLOTS) w = (n + 31) / 32 * 4 * geo.w[QG_NUM_CHUNKS];      // per queue: runs of 4 entries, 8 queues
    if (t == QG_QUOTA && w > 0) w = (n * geo.w[QG_NUM_CHUNKS] + w - 1) / w;  // in: blocks of a multi-generation launch; out: items per block
    if (t < QG_WORDS) ((int*)(block + 8 * PTK_QUEUE_STRIDE))[t] = w;
}

void launch_trace(const RenderParams& p0, int num_subtiles, int resident_waves, hipStream_t stream, bool stats)
{
    if (num_subtiles <= 0) return;
#if PTK_CONTRACT
    stats = false;                  // the counters belong to the exact build
#endif
    RenderParams p = p0;
    // the items = (entry of the live list, chunk) go into 8 queues (one per XCD group) in runs of four entries; the
    // host only knows an upper bound of the list's length (every quadrant live), the device the real one
    const int padded = (num_subtiles + 31) / 32 * 32 * p.num_chunks;
    // queue block = 8 zeroed slot counters (one per 128-B line) followed by the launch geometry the item set-up reads;
    // written by a one-wave kernel from its own arguments (stream-ordered, nothing for the host to wait on)
    QueueGeometry geo = {};
    geo.w[QG_NUM_CHUNKS] = p.num_chunks; geo.w[QG_WORLD] = p.world; geo.w[QG_RANK] = p.rank;
    geo.w[QG_TILES_X] = p.tiles_x; geo.w[QG_CHUNK] = p.chunk; geo.w[QG_SPP] = (int)p.spp;
    // big launches: persistent waves, as many one-wave workgroups as the chip holds at once, each pulling items until
    // none is left; small ones: a wave per (possible) item, the dispatcher balances those better
    if (!(p.flat_count > 0) && PTK_TRACE_WAVES_BVH != 4) resident_waves = resident_waves / 16 * 4 * PTK_TRACE_WAVES_BVH;
    if (p.flat_count > 0 && PTK_TRACE_WAVES != 4) resident_waves = resident_waves / 16 * 4 * ((p.plain && !stats) ? PTK_TRACE_WAVES_PLAIN : PTK_TRACE_WAVES);
    if (p.persistent < 0) p.persistent = padded > 4 * resident_waves ? 1 : 0;
    const int generations = p.persistent ? std::max(1, std::min(p.generations, padded / resident_waves)) : 1;
    const int blocks = p.persistent ? resident_waves * generations : padded;
    geo.w[QG_QUOTA] = generations > 1 ? blocks : 0;
    hipLaunchKernelGGL(queue_init_kernel, dim3(1), dim3(64), 0, stream, p.queues, geo, p.live_count, p);
    const RenderParams* dp = queue_block_params(p.queues);
    const bool flat = p.flat_count > 0;
#if !PTK_CONTRACT
    if (stats && flat) hipLaunchKernelGGL((trace_kernel<true, true, false>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
    else if (stats) hipLaunchKernelGGL((trace_kernel<true, false, false>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
    else if (flat && p.plain == 3) launch_trace_cycle(p.lambert != 0, blocks, stream, dp); // (the cycle unit: the flat_cycle option on top of flat_rect_pairs)
    else if (flat && p.plain == 2) launch_trace_rect(p.lambert != 0, blocks, stream, dp);  // (the pair-pass unit: the flat_rect_pairs option)
    else if (flat && p.plain) launch_trace_plain(p.lambert != 0, blocks, stream, dp);      // (the unit built for the class switch, above)
    else
#else
    if (flat && p.plain && p.lambert) hipLaunchKernelGGL((trace_kernel<false, true, true, true>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
    else if (flat && p.plain) hipLaunchKernelGGL((trace_kernel<false, true, true>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
    else
#endif
    if (flat) hipLaunchKernelGGL((trace_kernel<false, true, false>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
    else hipLaunchKernelGGL((trace_kernel<false, false, false>), dim3(blocks), dim3(PTK_TRACE_BLOCK), 0, stream, dp);
}

#endif  // !PTK_PLAIN_UNIT

#if PTK_CONTRACT
}  // namespace fma / fast
#endif
}  // namespace ptk
