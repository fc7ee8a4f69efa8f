// CPU test of the staging layout (pbrpathtracer_amd/csrc/ptk_stage.h, the HIP-free half): where the parts of a host entry's one
// staging allocation lie.  Offsets follow the order of declaration and never overlap, every present part starts on a 16-byte
// boundary - also behind a part of an odd number of bytes -, absent and empty parts take no space and say so, the total is the end
// of the last present part, and a layout without present parts has total 0.  Built and run by tests/test_host_cpu.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#define PTK_STAGE_LAYOUT_ONLY
#include "ptk_stage.h"

using ptk::StageLayout;

struct Want { size_t elem, count; bool present; };

static int check(const std::vector<Want>& parts, const char* name)
{
    StageLayout l;
    size_t end = 0;                              // end of the last present part so far
    int present = 0;
    for (size_t i = 0; i < parts.size(); i++)
    {
        const Want& w = parts[i];
        const size_t before = l.total, at = l.add(w.elem, w.count, w.present);
        if (!w.present || w.count == 0)
        {
            if (at != StageLayout::kAbsent) { std::printf("FAIL %s: part %zu is absent but got offset %zu\n", name, i, at); return 1; }
            if (l.total != before) { std::printf("FAIL %s: absent part %zu took %zu bytes\n", name, i, l.total - before); return 1; }
            continue;
        }
        present++;
        if (at == StageLayout::kAbsent) { std::printf("FAIL %s: present part %zu reported absent\n", name, i); return 1; }
        if (at % 16 != 0) { std::printf("FAIL %s: part %zu at %zu is not 16-byte aligned\n", name, i, at); return 1; }
        if (at < end) { std::printf("FAIL %s: part %zu at %zu overlaps or precedes the part before it (ends at %zu)\n", name, i, at, end); return 1; }
        if (at - end >= 16) { std::printf("FAIL %s: %zu bytes of padding before part %zu\n", name, at - end, i); return 1; }
        end = at + w.elem * w.count;
        if (l.total != end) { std::printf("FAIL %s: total %zu after part %zu, which ends at %zu\n", name, l.total, i, end); return 1; }
    }
    if (l.total != end) { std::printf("FAIL %s: total %zu, last present part ends at %zu\n", name, l.total, end); return 1; }
    if (present == 0 && l.total != 0) { std::printf("FAIL %s: all parts absent, total %zu\n", name, l.total); return 1; }
    return 0;
}

int main()
{
    int bad = 0;
    bad += check({}, "empty");
    bad += check({ { 4, 10, false }, { 1, 7, false }, { 4, 0, true }, { 1, 0, true } }, "all absent");
    // a part of odd byte size in front, in the middle and at the end: what follows is aligned all the same
    for (size_t n : { (size_t)1, (size_t)63, (size_t)65 })
    {
        bad += check({ { 1, n, true }, { 4, 3 * n, true }, { 4, n, true } }, "bytes first");
        bad += check({ { 4, 3 * n, true }, { 1, n, true }, { 4, 2 * n, true }, { 1, n, true }, { 4, n, true } }, "bytes between");
        bad += check({ { 4, 3 * n, true }, { 4, 3 * n, true }, { 4, n, false }, { 4, n, true }, { 4, 2 * n, false }, { 1, n, true } }, "a ray query");
        bad += check({ { 1, n, true }, { 1, n, true }, { 1, n, true } }, "bytes only");
        bad += check({ { 4, n, false }, { 1, n, true }, { 4, 0, true }, { 8, n, true } }, "absent first, empty between");
    }
    // sizes are size_t: parts beyond 4 GiB
    {
        StageLayout l;
        const size_t a = l.add(4, (size_t)3 << 30), b = l.add(1, 5), c = l.add(16, (size_t)1 << 30);
        if (a != 0 || b != (size_t)12 << 30 || c != ((size_t)12 << 30) + 16 || l.total != c + ((size_t)16 << 30))
        { std::printf("FAIL large: %zu %zu %zu total %zu\n", a, b, c, l.total); bad++; }
    }
    if (bad) return 1;
    std::printf("stage layout OK\n");
    return 0;
}
