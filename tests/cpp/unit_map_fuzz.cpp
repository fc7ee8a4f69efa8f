// The cycle unit's work-unit mapping without a device: csrc/ptk_unit_map.h unit_place / unit_pixel / unit_magic - the functions the
// kernel's deal calls (csrc/ptk_trace_cycle.h) - swept over every item shape a launch can produce.
//   unit_map_fuzz <masks per live count> [seed]
// For every live-pixel count 1 .. 64, <masks> random live masks of that count, chunk sizes 4 and 8 (and a short last chunk of each),
// and every deal width 1 .. 64: the item's units are dealt as the kernel deals them - rounds of `width` needy lanes, lane of rank r
// taking unit next + r while that is below the item's total, the last round partial - and
//   * every unit (live pixel, sample) of the item is dealt exactly once, no dead pixel ever;
//   * its slot is base + s * 64 + q;
//   * s is u / n_live by true division, q the pixel of rank u % n_live in ascending lane order;
//   * its pixel is what the voted kernels' deal computes: (y0 + (q >> 3)) * width + x0 + (q & 7), with s from their own expression
//     n_live == 1 ? u : __umulhi(u, magic) and the table acquire_work_item writes.
// Exit status 0 and a last line "ok" when all of it holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ptk_unit_map.h"

static int popc64(uint64_t x) { return __builtin_popcountll(x); }

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: unit_map_fuzz <masks per live count> [seed]\n"); return 2; }
    const int masks = std::atoi(argv[1]);
    std::mt19937_64 gen(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 20240607ull);
    unsigned long long calls = 0, mismatches = 0, items = 0, partial_rounds = 0, single_pixel_items = 0;
    std::vector<int> dealt(8 * 64);
    for (uint32_t n_live = 1; n_live <= 64; n_live++)
        for (int m = 0; m < masks; m++)
        {
            // a random mask with exactly n_live bits (the first of each count: the lowest / the highest bits, then random ones)
            uint64_t mask = 0;
            if (m == 0) mask = n_live == 64 ? ~0ull : ((1ull << n_live) - 1ull);
            else if (m == 1) mask = n_live == 64 ? ~0ull : ~((1ull << (64 - n_live)) - 1ull);
            else while ((uint32_t)popc64(mask) < n_live) mask |= 1ull << (gen() & 63);
            // the table as acquire_work_item writes it, and the item's constants
            unsigned char pixel_of_rank[64];
            std::memset(pixel_of_rank, 0xff, sizeof(pixel_of_rank));
            for (int lane = 0; lane < 64; lane++)
                if ((mask >> lane) & 1ull) pixel_of_rank[popc64(mask & ((1ull << lane) - 1ull))] = (unsigned char)lane;
            const uint32_t magic = (uint32_t)((0x100000000ull + n_live - 1u) / n_live);        // IT_NLIVE_MAGIC
            if (magic != ptk::unit_magic(n_live)) { mismatches++; std::printf("magic of %u\n", n_live); }
            const uint32_t width = 8u + (uint32_t)(gen() % 8185u), x0 = (uint32_t)(gen() % (width / 8u)) * 8u, y0 = (uint32_t)(gen() % 1024u) * 8u;
            const uint32_t pixbase = y0 * width + x0;
            for (uint32_t chunk : { 4u, 8u })
                for (uint32_t s_count : { chunk, chunk - 1u - (uint32_t)(gen() % (chunk - 1u)) })      // a full chunk and a short last one
                {
                    const uint32_t out_base = (uint32_t)(gen() % 100000u) * chunk * 64u, s_begin = (uint32_t)(gen() % 64u) * chunk;
                    const uint32_t total = n_live * s_count;
                    items++; single_pixel_items += n_live == 1u;
                    for (uint32_t deal_width = 1; deal_width <= 64; deal_width++)
                    {
                        std::fill(dealt.begin(), dealt.end(), 0);
                        uint32_t next = 0;
                        while (next < total)
                        {
                            if (total - next < deal_width) partial_rounds++;
                            for (uint32_t rank = 0; rank < deal_width; rank++)
                            {
                                const uint32_t u = next + rank;
                                if (!(u < total)) continue;                 // (the deal's `rank < avail`)
                                const ptk::UnitPlace p = ptk::unit_place(u, n_live, magic, pixel_of_rank, out_base);
                                const uint32_t pix = ptk::unit_pixel(p.q, pixbase, width), sample_abs = s_begin + p.s;
                                calls++;
                                // the voted kernels' own expressions (csrc/ptk_kernels.hip, the deal of the main loop)
                                const uint32_t s_ref = n_live == 1u ? u : (uint32_t)(((uint64_t)u * magic) >> 32);
                                const uint32_t q_ref = pixel_of_rank[u - s_ref * n_live];
                                const uint32_t pix_ref = (y0 + (q_ref >> 3)) * width + x0 + (q_ref & 7u);
                                const uint32_t out_ref = out_base + s_ref * 64u + q_ref;
                                bool ok = p.s == u / n_live && p.s < s_count && p.q < 64u && ((mask >> p.q) & 1ull) != 0ull;
                                ok = ok && p.q == pixel_of_rank[u % n_live] && p.slot == out_base + p.s * 64u + p.q;
                                ok = ok && p.s == s_ref && p.q == q_ref && pix == pix_ref && p.slot == out_ref && sample_abs == s_begin + s_ref;
                                if (!ok)
                                {
                                    if (mismatches++ < 10) std::printf("n_live %u mask %016llx chunk %u count %u width %u unit %u: s %u q %u slot %u pix %u\n", n_live,
                                                                       (unsigned long long)mask, chunk, s_count, deal_width, u, p.s, p.q, p.slot, pix);
                                    continue;
                                }
                                dealt[p.s * 64u + p.q]++;
                            }
                            next = next + deal_width < total ? next + deal_width : total;
                        }
                        for (uint32_t s = 0; s < 8u; s++)
                            for (uint32_t q = 0; q < 64u; q++)
                                if (dealt[s * 64u + q] != (s < s_count && ((mask >> q) & 1ull) ? 1 : 0)) mismatches++;
                    }
                }
        }
    std::printf("items %llu (with one live pixel: %llu), units placed %llu, partial last rounds %llu\n", items, single_pixel_items, calls, partial_rounds);
    std::printf("mismatches %llu\n", mismatches);
    if (mismatches || !single_pixel_items || !partial_rounds) return 1;
    std::printf("ok\n");
    return 0;
}
