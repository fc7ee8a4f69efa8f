// The host BVH builder (pbrpathtracer_amd/csrc/bvh_build.cpp) as a stand-alone program, for the tests that need a tree without a
// GPU (tests/test_walker_limits_cpu.py):   bvh_dump <verts.f32> <leaf_max> <nodes.f32> <order.i32>
// reads n x 9 float32 vertices, builds the tree the way ptk_upload_scene's host path does (stack bound 32, leaf size 4 unless
// "bvh_leaf_max" says otherwise) and writes the 16-float node records and the leaf order.  Prints "nodes depth stack_need".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bvh_build.h"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: bvh_dump verts.f32 leaf_max nodes.f32 order.i32\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 36 != 0) { std::fprintf(stderr, "%s: not a whole number of triangles\n", argv[1]); return 2; }
    std::vector<float> verts((size_t)bytes / 4);
    if (std::fread(verts.data(), 1, (size_t)bytes, f) != (size_t)bytes) { std::fprintf(stderr, "%s: short read\n", argv[1]); return 2; }
    std::fclose(f);
    ptk::g_bvh_tuning.leaf_max = std::atoi(argv[2]);
    ptk::BuiltBvh b;
    if (!ptk::build_bvh(verts.data(), (int32_t)(bytes / 36), 32, 4, b)) { std::fprintf(stderr, "build_bvh failed\n"); return 1; }
    std::FILE* fn = std::fopen(argv[3], "wb");
    std::FILE* fo = std::fopen(argv[4], "wb");
    if (!fn || !fo) { std::perror("output"); return 2; }
    const bool ok = std::fwrite(b.nodes.data(), 4, b.nodes.size(), fn) == b.nodes.size() &&
                    std::fwrite(b.order.data(), 4, b.order.size(), fo) == b.order.size();
    if (std::fclose(fn) != 0 || std::fclose(fo) != 0 || !ok) { std::fprintf(stderr, "write failed\n"); return 2; }
    std::printf("%d %d %d\n", (int)b.num_nodes, (int)b.depth, (int)b.stack_need);
    return 0;
}
