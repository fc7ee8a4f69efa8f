// HIP kernels for gfx950 that exist ONCE in libptk.so, in the exact build (-ffp-contract=off, namespace ptk), and their launchers:
// what a frame needs around the trace kernels of ptk_kernels.hip - primary rays and the primary-hit cache, the live mask and the
// ordered list of live quadrants, the per-pixel RNG keys, accumulate_kernel (the fold of the sample buffer, the 8-bit resolve, the
// hand-off), the packed form of the multi-GPU exchange - and the parity probes.  Built from ptk_device_fn.h's device functions.
#include "ptk_device_fn.h"
#include "ptk_adaptive.h"
#include "ptk_flat_mt.h"

namespace ptk {

// The hemisphere sampler's tangent frame (sample_basis) about an unsmoothed, unmapped triangle's shading normal takes two values:
// one for the stored normal, one for its negation (shade_interaction's flip test).  They are tabulated here for the FLAT scenes'
// triangles, by the device function and with the arguments the shade block would use - the negated normal's frame is computed from
// the negated normal, not by negating the other (the signs of zeros differ) - so the PLAIN kernel reads the bits it used to compute.
// One thread per (triangle, side); a degenerate triangle's NaN normal gives the NaN frame it always gave.
__global__ __launch_bounds__(64) void fill_flat_frames_kernel(const float4* __restrict__ shade, float4* __restrict__ flat_tris, int first, int count)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count * 2) return;
    const int tri = first + (j >> 1), side = j & 1;
    const float4 s0 = shade[(size_t)tri * SHADE_F4];
    v3 n = V(s0.x, s0.y, s0.z);
    if (side) n = neg(n);
    v3 u, v;
    sample_basis(n, 1.0f - PTK_EPS, n, u, v);
    float4* f = flat_tris + FLAT_FRAMES_AT + tri * FLAT_FRAME_F4 + side * 2;
    f[0] = make_float4(u.x, u.y, u.z, 0.0f);
    f[1] = make_float4(v.x, v.y, v.z, 0.0f);
}
void launch_flat_frames(const float4* d_shade, float4* d_flat_tris, int first, int count, hipStream_t stream)
{
    if (count > 0) hipLaunchKernelGGL(fill_flat_frames_kernel, dim3((count * 2 + 63) / 64), dim3(64), 0, stream, d_shade, d_flat_tris, first, count);
}

// The class table behind the frame table (ptk_device.h FLAT_CLASSES_AT): lane k classifies record k by its six stored edge words
// (ptk_flat_mt.h flat_zero_class, the rule ptk_flat_zero_class exports), lane 0 gathers the nibbles and writes both words.
// One wave; classifies all records anew, whichever of them changed.
// The pair word behind it (FLAT_PAIRS_AT): lane k < 8 takes records 2k, 2k + 1 to ptk_flat_mt.h flat_rect_pair (the rule
// ptk_flat_rect_pair exports); lane 0 keeps the kinds of the longest prefix of pairs and its length.
__global__ __launch_bounds__(64) void classify_flat_kernel(float4* __restrict__ flat_tris, int num_tris, int use, int use_pairs)
{
    const int k = threadIdx.x;
    int cls = 0, kind = 0;
    if (k < num_tris && k < FLAT_MAX_TRIS)
    {
        const float4 t0 = flat_tris[k * TRI_F4], t1 = flat_tris[k * TRI_F4 + 1], t2 = flat_tris[k * TRI_F4 + 2];
        const float e[6] = { t0.w, t1.x, t1.y, t1.z, t1.w, t2.x };
        cls = ptk_mt::flat_zero_class(e);
    }
    if (2 * k + 1 < num_tris && 2 * k + 1 < FLAT_MAX_TRIS)
    {
        float rec[2][9];
        int index[2];
        for (int r = 0; r < 2; r++)
        {
            const float4* q = flat_tris + (2 * k + r) * TRI_F4;
            const float4 t0 = q[0], t1 = q[1], t2 = q[2];
            rec[r][0] = t0.x; rec[r][1] = t0.y; rec[r][2] = t0.z; rec[r][3] = t0.w; rec[r][4] = t1.x; rec[r][5] = t1.y;
            rec[r][6] = t1.z; rec[r][7] = t1.w; rec[r][8] = t2.x;
            index[r] = __float_as_int(t2.y);
        }
        // (the pair pass takes B's triangle index to be A's + 1, as the flat list's order has it)
        kind = index[1] == index[0] + 1 ? ptk_mt::flat_rect_pair(rec[0], rec[1]) : 0;
    }
    unsigned long long word = 0ull, pairs = 0ull;
    for (int j = 0; j < FLAT_MAX_TRIS; j++) word |= (unsigned long long)(__shfl(cls, j) & 15) << (j * 4);
    int m = 0;
    for (int j = 0; j < FLAT_MAX_TRIS / 2; j++)
    {
        const int kj = __shfl(kind, j);
        if (m == j && kj != 0) { pairs |= (unsigned long long)kj << (j * 4); m = j + 1; }
    }
    pairs |= (unsigned long long)m << 32;
    if (k == 0)
    {
        unsigned long long* out = (unsigned long long*)(flat_tris + FLAT_CLASSES_AT);
        out[0] = use ? word : 0ull;
        out[1] = word;
        unsigned long long* outp = (unsigned long long*)(flat_tris + FLAT_PAIRS_AT);
        outp[0] = use_pairs ? pairs : 0ull;
        outp[1] = pairs;
    }
}
void launch_flat_classes(float4* d_flat_tris, int num_tris, int use, int use_pairs, hipStream_t stream)
{
    hipLaunchKernelGGL(classify_flat_kernel, dim3(1), dim3(64), 0, stream, d_flat_tris, num_tris, use, use_pairs);
}

// Streaming fold of the sample buffer into the float accumulator, strictly in sample order
// (`mTotalImg[px] += color` once per RenderFrame(), pathtracer.cpp:798-800), plus the 8-bit resolve
// (pathtracer.cpp:802-812).  One thread per pixel; each sample read is a coalesced 1 KiB per wave.
__global__ __launch_bounds__(PTK_BLOCK) void accumulate_kernel(const RenderParams P)
{
    // an aborted pass adds nothing: trace waves that saw the exit flag returned without writing their samples, so the
    // sample buffer may hold another pass's values (the reference adds nothing for the rows it skips, pathtracer.cpp:779-780)
    if (P.exit_flag && __hip_atomic_load(P.exit_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.exit_gen) return;     // an Exit() named this render or a later one
    const int tid = threadIdx.x;
    const int lane = tid & 63, quad = tid >> 6;
    const int owned = blockIdx.x;
    const int tile = owned * P.world + P.rank;
    if (tile >= P.num_tiles) return;
    int tx, ty; tile_origin(tile, P.tiles_x, tx, ty);
    // (quadrant_pixel written out: through the helper the shifts of tid fold in another order, and this kernel keeps its machine code)
    const int px = tx * PTK_TILE + (quad & 1) * 8 + (lane & 7);
    const int py = ty * PTK_TILE + (quad >> 1) * 8 + (lane >> 3);
    if (px >= P.width || py >= P.height) return;
    const size_t accidx = ((size_t)(P.height - 1 - py) * P.width + px) * 3;   // bottom-up (pathtracer.cpp:796)
    v3 acc = V(P.accum[accidx], P.accum[accidx + 1], P.accum[accidx + 2]);
    const size_t subtile = (size_t)owned * 4 + quad;
    // (a pixel that is not in its quadrant's live mask - cached camera ray misses, or no lens ray reaches the scene - was not
    // traced: nothing was stored for it and it receives nothing)
    const bool black = ((P.live_mask[subtile] >> lane) & 1ull) == 0ull;
    if (!black)
    {
        // the samples of one pixel are a strided array (chunk after chunk of its quadrant's items): sample s sits at
        // in[s * 64].  Eight loads in flight per lane, added strictly in sample order.
        const float4* in = P.samples + (subtile * P.num_chunks * P.chunk) * 64 + lane;
        uint32_t s = 0;
        for (; s + 8 <= P.spp; s += 8)
        {
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = in[(size_t)(s + k) * 64];
#pragma unroll
            for (int k = 0; k < 8; k++) acc = add(acc, V(v[k].x, v[k].y, v[k].z));
        }
        for (; s < P.spp; s++)
        {
            const float4 col = in[(size_t)s * 64];
            acc = add(acc, V(col.x, col.y, col.z));
        }
    }
    P.accum[accidx] = acc.x; P.accum[accidx + 1] = acc.y; P.accum[accidx + 2] = acc.z;
    float c3[3] = { acc.x / P.resolve_samples, acc.y / P.resolve_samples, acc.z / P.resolve_samples };
    uint8_t b3[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        b3[k] = resolve8(c3[k]);
        P.rgb8[accidx + k] = b3[k];
    }
    if (P.rgb8_host)
    {
        // The hand-off: straight into the caller's page-locked buffer, over PCIe.  A pixel that receives nothing AND holds
        // nothing resolves to 0 whatever the sample count - it was written when the buffer was bound / reset and is
        // skipped (four fifths of the C2 frame); one that holds light from before a camera move keeps dimming and is
        // written.  Byte stores of single pixels crawl over the link (measured: 0.5 MB in 70 us), so a row of the quadrant
        // - 8 pixels, 24 contiguous bytes - is gathered with lane shuffles and leaves as six dwords.
        const bool skip_host = black && acc.x == 0.0f && acc.y == 0.0f && acc.z == 0.0f && !P.rgb8_host_full;
        const uint32_t mine = (uint32_t)b3[0] | ((uint32_t)b3[1] << 8) | ((uint32_t)b3[2] << 16);
        const unsigned long long row_live = (__ballot(!skip_host) >> (lane & ~7)) & 0xffull;     // this row's pixels that must be written
        // dword d (0..5) of the row holds bytes 4d..4d+3 = pixels (4d)/3 .. (4d+3)/3; lanes 0..5 of each row write one each
        const int d = lane & 7;
        const int p0 = (4 * d) / 3, p1 = min(7, (4 * d + 3) / 3), sh = (4 * d) % 3;          // first pixel, last pixel, byte offset in the first
        const uint32_t w0 = (uint32_t)__shfl((int)mine, (lane & ~7) + min(p0, 7)), w1 = (uint32_t)__shfl((int)mine, (lane & ~7) + p1);
        // bytes of pixel p0 from offset sh, then pixel p0 + 1 (= p1 unless the dword lies within one pixel... it never does: 4 > 3)
        const uint32_t word = (w0 >> (8 * sh)) | (w1 << (8 * (3 - sh)));
        const bool aligned = (((size_t)P.width * 3) & 3) == 0 && (((uintptr_t)P.rgb8_host) & 3) == 0;
        const int row_px = min(8, P.width - (px - (lane & 7)));                                // pixels of this row on the image (>= 1 here)
        if (aligned && row_px == 8)
        {
            if (d < 6 && row_live != 0ull) *(uint32_t*)(P.rgb8_host + accidx - (size_t)(lane & 7) * 3 + d * 4) = word;
        }
        else if (!skip_host)
        {
            P.rgb8_host[accidx] = b3[0]; P.rgb8_host[accidx + 1] = b3[1]; P.rgb8_host[accidx + 2] = b3[2];
        }
    }
}

// Primary ray directions before DOF: one thread per image row walks the row with the reference's
// incremental `pixel += camRight * deltaX` (pathtracer.cpp:782-785, :814), so every direction is
// the value the reference computes.  Runs once per camera / resolution change.
__global__ void primary_dirs_kernel(const PrimaryParams P)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.height) return;
    v3 up = V(P.cam_up[0], P.cam_up[1], P.cam_up[2]);
    v3 right = V(P.cam_right[0], P.cam_right[1], P.cam_right[2]);
    v3 pos = V(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    v3 pixel = sub(V(P.top_left[0], P.top_left[1], P.top_left[2]), muls(up, (float)i * P.delta_y));
    v3 step = muls(right, P.delta_x);
    float4* row = P.primary + (size_t)i * P.width;
    for (int j = 0; j < P.width; j++)
    {
        v3 d = normalize(sub(pixel, pos));
        row[j] = make_float4(d.x, d.y, d.z, 0.0f);
        pixel = add(pixel, step);
    }
}

// Primary-visibility cache for pinhole cameras (aperture == 0) in scenes without opacity textures: the
// camera ray of a pixel is the same for every sample (pathtracer.cpp:785-791 with a zero lens offset),
// so its closest hit is found once per camera / scene change instead of once per sample.
__global__ __launch_bounds__(PTK_BLOCK) void primary_hits_kernel(const RenderParams P, float4* out, float4* out_rd)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_BLOCK];
    const int i = blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (i >= P.width * P.height) return;
    Rng rng; rng.inc = 1u; rng.state = 0u; rng.key = 0u;            // no opacity draws can occur here
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    float4 d = P.primary[i];
    const v3 camPos0 = V(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    v3 focalPoint = add(camPos0, muls(V(d.x, d.y, d.z), P.focal_dist));
    v3 rd = normalize(sub(focalPoint, camPos0));
    Walk W;
    W.occl_tri = -1;
    W.begin(camPos0, rd, P.num_nodes, lds_stack + threadIdx.x, P.scene_bound);
    while (!W.done()) walk_step<false, PTK_BLOCK>(P, W, rng, 0u, lds_stack + threadIdx.x, cnt);
    out[i] = make_float4(__int_as_float(W.best.tri), W.best.t, W.best.u, W.best.v);
    out_rd[i] = make_float4(rd.x, rd.y, rd.z, 0.0f);           // the very floats the camera-ray block computes for a zero lens offset
}

// Parity probe: closest hit for a list of rays (no opacity draws differ: key 0, ray 0).
__global__ __launch_bounds__(PTK_BLOCK) void probe_hits_kernel(const ProbeParams P)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_BLOCK];
    int i = blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (i >= P.n) return;
    Rng rng; rng.inc = (hash32(0u ^ 0x9E3779B9u) << 1) | 1u; rng.state = hash32(0u); rng.key = rng.state;
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    v3 ro = V(P.ro[i * 3], P.ro[i * 3 + 1], P.ro[i * 3 + 2]);
    v3 rd = V(P.rd[i * 3], P.rd[i * 3 + 1], P.rd[i * 3 + 2]);
    Walk W;
    W.occl_tri = -1;
    W.begin(ro, rd, P.num_nodes, lds_stack + threadIdx.x, P.scene_bound);
    while (!W.done()) walk_step<false, PTK_BLOCK>(P, W, rng, 0u, lds_stack + threadIdx.x, cnt);
    bool hit = W.best.tri != PTK_NOHIT;
    P.tri[i] = hit ? W.best.tri : -1;
    P.tuv[i * 3] = hit ? W.best.t : 0.0f; P.tuv[i * 3 + 1] = hit ? W.best.u : 0.0f; P.tuv[i * 3 + 2] = hit ? W.best.v : 0.0f;
}

// Parity probe of DirectIllumimation (pathtracer.cpp:505-531) with its three draws on tape: the sampling half above, then the
// shadow walk and the visibility rule exactly as trace_kernel applies them (PTK_WALK_DONE).
__global__ __launch_bounds__(PTK_BLOCK) void probe_direct_kernel(const ProbeParams P, const float* __restrict__ pts, const float* __restrict__ nrm,
                                                                 const float* __restrict__ dif, const float* __restrict__ tape, float* __restrict__ out)
{
    __shared__ int lds_stack[PTK_STACK_ROWS * PTK_BLOCK];
    const int i = blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (i >= P.n) return;
    Rng rng; rng.inc = (hash32(0u ^ 0x9E3779B9u) << 1) | 1u; rng.state = hash32(0u); rng.key = rng.state;
    Counters cnt = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const v3 p = V(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]), n = V(nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2]);
    const v3 diffuse = V(dif[i * 3], dif[i * 3 + 1], dif[i * 3 + 2]);
    v3 l, di, res = V(0.0f, 0.0f, 0.0f);
    int light_tri;
    float4 lt0, lt1, lt2;
    if (P.num_lights > 0 && sample_direct_light(P, p, n, diffuse, tape[i * 3], tape[i * 3 + 1], tape[i * 3 + 2], l, di, light_tri, lt0, lt1, lt2))
    {
        Walk W;
        W.begin(p, l, P.num_nodes, lds_stack + threadIdx.x, P.scene_bound);
        W.occl_tri = light_tri;
        (void)tri_test<false>(P, W, lt0, lt1, lt2, rng, 0u, cnt);
        while (!W.done()) walk_step<false, PTK_BLOCK>(P, W, rng, 0u, lds_stack + threadIdx.x, cnt);
        if (!(W.best.tri != PTK_NOHIT && W.best.tri != W.occl_tri)) res = di;        // :522-526: lit unless something else is closest
    }
    out[i * 3] = res.x; out[i * 3 + 1] = res.y; out[i * 3 + 2] = res.z;
}
void launch_probe_direct(const ProbeParams& p, const float* pts, const float* nrm, const float* dif, const float* tape, float* out, hipStream_t stream)
{
    if (p.n > 0) hipLaunchKernelGGL(probe_direct_kernel, dim3((p.n + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, p, pts, nrm, dif, tape, out);
}

// Uncached cameras (thin lens; pinhole with opacity textures): can ANY camera ray of this pixel reach the scene?  Every lens ray
// of a pixel starts inside the aperture square around the camera position and passes through the pixel's focal point
// (pathtracer.cpp:785-791; the camera-ray block of trace_kernel): origin o = cam + x right + y up with |x|, |y| <= aperture,
// direction parallel to F - o.  Per axis that is o_k in [cam_k - h_k, cam_k + h_k], d_k in [F_k - cam_k - h_k, F_k - cam_k + h_k]
// with h_k = aperture (|right_k| + |up_k|); taking the two intervals as independent (a superset of the bundle), the ray
// parameters t >= 0 at which SOME such ray is inside the scene's bounding box on axis k form an interval given by two linear
// inequalities; the pixel is dead - black for every sample, never traced, nothing stored - when the three intervals have no
// common point.  Conservative by construction and by margin: the box is padded by 1e-4 of the scene's size and of the camera's
// distance (Moeller-Trumbore accepts nothing measurably outside a triangle, and every triangle lies in the box), the intervals by
// the float rounding of o, F and the normalised direction; evaluated in double, once per camera / frame / scene change.
// Exact: bit-identical images with the cull on and off (tests/test_gpu_host_api.py::test_lens_cull_is_exact).
__device__ bool lens_rays_may_reach_scene(const RenderParams& P, const float4 d0)
{
    double ext = 0.0, far_ = 0.0;
    for (int k = 0; k < 3; k++)
    {
        ext = fmax(ext, (double)P.scene_hi[k] - (double)P.scene_lo[k]);
        far_ = fmax(far_, fmax(fabs((double)P.scene_lo[k] - (double)P.cam_pos[k]), fabs((double)P.scene_hi[k] - (double)P.cam_pos[k])));
    }
    const double pad = 1e-4 * (ext + far_) + 1e-5;
    const double ap = fabs((double)P.aperture) * 1.0001;
    const float dir0[3] = { d0.x, d0.y, d0.z };
    double tlo = 0.0, thi = 1e300;
    bool feasible = true;
    for (int k = 0; k < 3; k++)
    {
        const float Ff = P.cam_pos[k] + dir0[k] * P.focal_dist;            // the focal point as the camera-ray block computes it
        const double oc = (double)P.cam_pos[k], F = (double)Ff;
        const double h = ap * (fabs((double)P.cam_right[k]) + fabs((double)P.cam_up[k])) + 1e-6 * fabs(oc);
        const double dc = F - oc, hd = h + 1e-6 * (fabs(F) + fabs(oc) + fabs(dc));
        const double lo = (double)P.scene_lo[k] - pad, hi = (double)P.scene_hi[k] + pad;
        // the smallest coordinate any ray of the bundle has at parameter t must not exceed hi, the largest not fall short of lo
        const double a1 = (oc - h) - hi, b1 = dc - hd;                     // a1 + t b1 <= 0
        const double a2 = lo - (oc + h), b2 = -(dc + hd);                  // a2 + t b2 <= 0
        if (b1 > 0.0) thi = fmin(thi, -a1 / b1); else if (b1 < 0.0) tlo = fmax(tlo, -a1 / b1); else if (a1 > 0.0) feasible = false;
        if (b2 > 0.0) thi = fmin(thi, -a2 / b2); else if (b2 < 0.0) tlo = fmax(tlo, -a2 / b2); else if (a2 > 0.0) feasible = false;
    }
    return feasible && tlo <= thi * (1.0 + 1e-9) + 1e-12;
}

// Which pixels of every owned 8x8 quadrant need tracing: on the image, and - when the camera ray's closest hit is
// cached - not a miss (pathtracer.cpp:550: such a pixel is black for every sample); uncached cameras: not a pixel whose
// lens rays all miss the scene's bounds (above).  One wave per quadrant.
__global__ __launch_bounds__(PTK_BLOCK) void live_mask_kernel(const RenderParams P, unsigned long long* mask, int num_subtiles)
{
    const int subtile = blockIdx.x * (PTK_BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (subtile >= num_subtiles) return;
    const int owned = subtile >> 2, quad = subtile & 3;
    const int tile = owned * P.world + P.rank;
    bool live = false;
    if (tile < P.num_tiles)
    {
        int tx, ty, px, py; tile_origin(tile, P.tiles_x, tx, ty);
        quadrant_pixel(tx, ty, quad, lane, px, py);
        live = px < P.width && py < P.height;
        if (live && P.primary_hit) live = __float_as_int(P.primary_hit[(size_t)py * P.width + px].x) != PTK_NOHIT;
        else if (live && P.lens_cull) live = lens_rays_may_reach_scene(P, P.primary[(size_t)py * P.width + px]);
    }
    const unsigned long long m = __ballot(live);
    if (lane == 0) mask[subtile] = m;
}

// Ordered list of the quadrants that have live pixels (single workgroup: a few hundred thousand quadrants at most).
__global__ __launch_bounds__(1024) void live_compact_kernel(const unsigned long long* mask, int num_subtiles, unsigned* list, unsigned* count)
{
    __shared__ unsigned wave_total[16];
    __shared__ unsigned base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) base = 0;
    __syncthreads();
    for (int s0 = 0; s0 < num_subtiles; s0 += 1024)
    {
        const int sidx = s0 + t;
        const bool live = sidx < num_subtiles && mask[sidx] != 0ull;
        const unsigned long long b = __ballot(live);
        if (lane == 0) wave_total[wave] = (unsigned)__popcll(b);
        __syncthreads();
        unsigned before = base;
        for (int w = 0; w < wave; w++) before += wave_total[w];
        if (live) list[before + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = (unsigned)sidx;
        __syncthreads();
        if (t == 0) { unsigned sum = 0; for (int w = 0; w < 16; w++) sum += wave_total[w]; base += sum; }
        __syncthreads();
    }
    if (t == 0) *count = base;
}

__global__ __launch_bounds__(PTK_BLOCK) void pixel_rng_kernel(uint32_t seed_lo, uint32_t seed_hi, int n, uint2* out)
{
    const int i = blockIdx.x * PTK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pkey = pixel_key(seed_lo, seed_hi, (uint32_t)i);
    out[i] = make_uint2(pkey, (hash32(pkey ^ 0x9E3779B9u) << 1) | 1u);
}
void launch_pixel_rng(uint32_t seed_lo, uint32_t seed_hi, int n, uint2* out, hipStream_t stream)
{
    if (n > 0) hipLaunchKernelGGL(pixel_rng_kernel, dim3((n + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, seed_lo, seed_hi, n, out);
}

void launch_compact_list(const unsigned long long* mask, int num_subtiles, unsigned* list, unsigned* count, hipStream_t stream)
{
    if (num_subtiles > 0) hipLaunchKernelGGL(live_compact_kernel, dim3(1), dim3(1024), 0, stream, mask, num_subtiles, list, count);
}
void launch_live_list(const RenderParams& p, int num_subtiles, unsigned long long* mask, unsigned* list, unsigned* count, hipStream_t stream)
{
    if (num_subtiles <= 0) return;
    const int per_block = PTK_BLOCK / 64;
    hipLaunchKernelGGL(live_mask_kernel, dim3((num_subtiles + per_block - 1) / per_block), dim3(PTK_BLOCK), 0, stream, p, mask, num_subtiles);
    launch_compact_list(mask, num_subtiles, list, count, stream);
}

// ---- multi-GPU exchange step: packed form of the float accumulator ---------------------------------
// Packed layout of rank r of `world` (include/ptk.h ptk_packed_layout): its owned tiles in ascending tile order, 768
// floats each = the tile's 16 x 16 pixels row-major from the tile's top-left, RGB; pixels off the image hold 0.
// pack: accumulator -> packed (one workgroup per owned tile, 768 B contiguous per wave-store);
// unpack: the packed buffers of ALL ranks (rank r's starts at float offset base[r]) -> full image, one workgroup per tile.
struct ExchangeBases { long long base[PTK_MAX_RANKS]; };

__global__ __launch_bounds__(PTK_BLOCK) void pack_owned_kernel(const float* __restrict__ accum, float* __restrict__ packed, int width, int height,
                                                               int tiles_x, int num_tiles, int rank, int world)
{
    const int owned = blockIdx.x, tile = owned * world + rank;
    if (tile >= num_tiles) return;
    int tx, ty; tile_origin(tile, tiles_x, tx, ty);
    const int p = threadIdx.x, px = tx * PTK_TILE + (p & 15), py = ty * PTK_TILE + (p >> 4);
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (px < width && py < height)
    {
        const size_t a = ((size_t)(height - 1 - py) * width + px) * 3;
        r = accum[a]; g = accum[a + 1]; b = accum[a + 2];
    }
    float* o = packed + (size_t)owned * (PTK_BLOCK * 3) + p * 3;
    o[0] = r; o[1] = g; o[2] = b;
}

__global__ __launch_bounds__(PTK_BLOCK) void unpack_all_kernel(const float* __restrict__ packed, const ExchangeBases bases, float* __restrict__ image,
                                                               int width, int height, int tiles_x, int num_tiles, int world)
{
    const int tile = blockIdx.x;
    if (tile >= num_tiles) return;
    const int rank = tile % world, owned = tile / world;
    int tx, ty; tile_origin(tile, tiles_x, tx, ty);
    const int p = threadIdx.x, px = tx * PTK_TILE + (p & 15), py = ty * PTK_TILE + (p >> 4);
    if (px >= width || py >= height) return;
    const float* in = packed + bases.base[rank] + (size_t)owned * (PTK_BLOCK * 3) + p * 3;
    const size_t a = ((size_t)(height - 1 - py) * width + px) * 3;
    image[a] = in[0]; image[a + 1] = in[1]; image[a + 2] = in[2];
}

void launch_pack_owned(const float* accum, float* packed, int width, int height, int rank, int world, hipStream_t stream)
{
    const int tiles_x = (width + PTK_TILE - 1) / PTK_TILE, num_tiles = tiles_x * ((height + PTK_TILE - 1) / PTK_TILE);
    const int owned = num_tiles <= rank ? 0 : (num_tiles - rank + world - 1) / world;
    if (owned > 0) hipLaunchKernelGGL(pack_owned_kernel, dim3(owned), dim3(PTK_BLOCK), 0, stream, accum, packed, width, height, tiles_x, num_tiles, rank, world);
}
void launch_unpack_all(const float* packed, const long long* bases, float* image, int width, int height, int world, hipStream_t stream)
{
    const int tiles_x = (width + PTK_TILE - 1) / PTK_TILE, num_tiles = tiles_x * ((height + PTK_TILE - 1) / PTK_TILE);
    ExchangeBases b = {};
    for (int r = 0; r < world && r < PTK_MAX_RANKS; r++) b.base[r] = bases[r];
    hipLaunchKernelGGL(unpack_all_kernel, dim3(num_tiles), dim3(PTK_BLOCK), 0, stream, packed, b, image, width, height, tiles_x, num_tiles, world);
}

void launch_accumulate(const RenderParams& p, int owned_tiles, hipStream_t stream)
{
    if (owned_tiles <= 0) return;
    hipLaunchKernelGGL(accumulate_kernel, dim3(owned_tiles), dim3(PTK_BLOCK), 0, stream, p);
}
void launch_primary_hits(const RenderParams& p, float4* out, float4* out_rd, hipStream_t stream)
{
    int n = p.width * p.height;
    hipLaunchKernelGGL(primary_hits_kernel, dim3((n + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, p, out, out_rd);
}
void launch_primary(const PrimaryParams& p, hipStream_t stream)
{
    int threads = 64;
    hipLaunchKernelGGL(primary_dirs_kernel, dim3((p.height + threads - 1) / threads), dim3(threads), 0, stream, p);
}
void launch_probe(const ProbeParams& p, hipStream_t stream)
{
    if (p.n <= 0) return;
    hipLaunchKernelGGL(probe_hits_kernel, dim3((p.n + PTK_BLOCK - 1) / PTK_BLOCK), dim3(PTK_BLOCK), 0, stream, p);
}

}  // namespace ptk
