// The refit rule of csrc/ptk_refit.hip (refit_kernel + bvh_quantise.h emit_wide_node) restated in host code and held against the
// host builder: refitting a tree over the vertices it was built from must reproduce every node record bit for bit, and
// refitting over moved vertices must keep the links and enclose every leaf's triangles.
#include "bvh_build.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace ptk;

static bool refit(const BuiltBvh& b, const std::vector<float>& v, std::vector<float>& out)
{
    float vmax = 0.0f;
    for (float x : v) vmax = std::max(vmax, std::fabs(x));
    const float pad = 1e-5f * std::max(vmax, 1.0f);
    const int nn = b.num_nodes;
    std::vector<int> level(nn, -1);
    level[0] = 0;
    int levels = 1;
    for (int id = 0; id < nn; id++)
    {
        if (level[id] < 0) { std::printf("node %d has no parent\n", id); return false; }
        int32_t l[4]; std::memcpy(l, &b.nodes[(size_t)id * 16 + 6], 16);
        for (int k = 0; k < 4; k++)
            if (l[k] >= 0)
            {
                if (l[k] <= id || l[k] >= nn) { std::printf("link of node %d does not point forward\n", id); return false; }
                level[l[k]] = level[id] + 1; levels = std::max(levels, level[l[k]] + 1);
            }
    }
    std::vector<float> side((size_t)nn * 6);
    out.assign(b.nodes.size(), 0.0f);
    for (int L = levels - 1; L >= 0; L--)
        for (int id = 0; id < nn; id++)
        {
            if (level[id] != L) continue;
            int32_t link[4]; std::memcpy(link, &b.nodes[(size_t)id * 16 + 6], 16);
            int nc = 0;
            while (nc < 4 && link[nc] != INT32_MIN) nc++;
            for (int k = nc; k < 4; k++) if (link[k] != INT32_MIN) { std::printf("node %d: slots not filled from the first\n", id); return false; }
            float cmn[4][3], cmx[4][3], umn[3] = { INFINITY, INFINITY, INFINITY }, umx[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (int k = 0; k < nc; k++)
            {
                if (link[k] < 0)
                {
                    const int code = ~link[k], first = code >> 3, cnt = (code & 7) + 1;
                    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
                    for (int j = 0; j < cnt; j++)
                    {
                        const float* p = &v[(size_t)b.order[first + j] * 9];
                        for (int c = 0; c < 9; c++) { mn[c % 3] = std::min(mn[c % 3], p[c]); mx[c % 3] = std::max(mx[c % 3], p[c]); }
                    }
                    for (int a = 0; a < 3; a++) { cmn[k][a] = mn[a] - pad; cmx[k][a] = mx[a] + pad; }
                }
                else for (int a = 0; a < 3; a++) { cmn[k][a] = side[(size_t)link[k] * 6 + a]; cmx[k][a] = side[(size_t)link[k] * 6 + 3 + a]; }
                for (int a = 0; a < 3; a++) { umn[a] = std::min(umn[a], cmn[k][a]); umx[a] = std::max(umx[a], cmx[k][a]); }
            }
            float scale[3]; uint32_t lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
            for (int a = 0; a < 3; a++)
            {
                const double ext = (double)umx[a] - (double)umn[a];
                float s = (float)(ext / 255.0 * (1.0 + 1e-6));
                if (!(s > 1e-30f)) s = 1e-30f;
                while ((double)umn[a] + 255.0 * (double)s < (double)umx[a]) s = std::nextafter(s, INFINITY);
                scale[a] = s;
                for (int k = 0; k < 4; k++)
                {
                    if (k >= nc) { lo[a] |= 255u << (8 * k); continue; }
                    const double o = umn[a], sd = s;
                    int ql = (int)std::floor(((double)cmn[k][a] - o) / sd), qh = (int)std::ceil(((double)cmx[k][a] - o) / sd);
                    ql = std::min(std::max(ql, 0), 255); qh = std::min(std::max(qh, 0), 255);
                    while (ql > 0 && o + ql * sd > (double)cmn[k][a]) ql--;
                    while (qh < 255 && o + qh * sd < (double)cmx[k][a]) qh++;
                    lo[a] |= (uint32_t)ql << (8 * k); hi[a] |= (uint32_t)qh << (8 * k);
                    // the quantised planes enclose the child's float box
                    if (o + ql * sd > (double)cmn[k][a] || o + qh * sd < (double)cmx[k][a]) { std::printf("node %d: a plane inside its child's box\n", id); return false; }
                }
            }
            float* q = &out[(size_t)id * 16];
            q[0] = umn[0]; q[1] = umn[1]; q[2] = umn[2]; q[3] = scale[0]; q[4] = scale[1]; q[5] = scale[2];
            std::memcpy(&q[6], link, 16); std::memcpy(&q[10], lo, 12); std::memcpy(&q[13], hi, 12);
            for (int a = 0; a < 3; a++) { side[(size_t)id * 6 + a] = umn[a]; side[(size_t)id * 6 + 3 + a] = umx[a]; }
        }
    return true;
}

int main()
{
    for (int n : { 5, 12, 16, 300, 5000, 40000 })
    {
        std::mt19937 g(n);
        std::uniform_real_distribution<float> U(-1, 1);
        std::vector<float> v((size_t)n * 9);
        for (int i = 0; i < n; i++)
        {
            const float c[3] = { U(g) * 3, U(g), U(g) };
            for (int k = 0; k < 9; k++) v[(size_t)i * 9 + k] = c[k % 3] + 0.05f * U(g);
        }
        BuiltBvh b;
        if (!build_bvh(v.data(), n, 32, 4, b)) { std::printf("n=%d: build failed\n", n); return 1; }
        std::vector<float> out;
        if (!refit(b, v, out)) return 1;
        if (std::memcmp(out.data(), b.nodes.data(), out.size() * sizeof(float)) != 0) { std::printf("n=%d: a refit of the unmoved scene differs from the built tree\n", n); return 1; }
        for (float& x : v) x = x * 1.7f + 0.3f * U(g);
        if (!refit(b, v, out)) return 1;
        for (int id = 0; id < b.num_nodes; id++)
            if (std::memcmp(&out[(size_t)id * 16 + 6], &b.nodes[(size_t)id * 16 + 6], 16) != 0) { std::printf("n=%d: links changed\n", n); return 1; }
        std::printf("n=%d: %d nodes, identical\n", n, b.num_nodes);
    }
    return 0;
}
