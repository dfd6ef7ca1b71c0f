// skin_check.cpp -- the arithmetic and the checks of linear-blend skinning (toyraygun_amd/csrc/trg_skin_math.h) run on the host, the way
// trg_skin_bind and the skin kernel of trg_refit.hip apply them.  A program of its own (host sanitizers welcome):
//
//   skin_check <input>      input: uint32 n_verts, n_tris, n_bones, has_normals; float positions[3 n_verts]; float normals[9 n_tris] (if any);
//                           uint32 indices[3 n_tris]; uint32 ids[4 n_verts]; float weights[4 n_verts]; float bones[12 n_bones]
//
// prints what the two checks say and -- for a binding that passes -- the skinned bits:
//   ids ok | ids refused vertex <v> slot <j>
//   weights ok | weights refused <weight|sum> vertex <v>
//   P <x> <y> <z>                        per vertex, hex words
//   N <x> <y> <z>                        per corner, hex words
#include <cstdio>
#include <cstring>
#include <vector>

#include "trg_skin_math.h"

using namespace trg;

namespace {
template <typename T>
bool read_n(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: skin_check <input>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n_verts = head[0], n_tris = head[1], n_bones = head[2];
    const bool has_nrm = head[3] != 0;
    std::vector<float> pos, nrm, weights, bones;
    std::vector<uint32_t> idx, ids;
    if (!read_n(f, pos, (size_t)n_verts * 3) || !read_n(f, nrm, has_nrm ? (size_t)n_tris * 9 : 0) || !read_n(f, idx, (size_t)n_tris * 3) ||
        !read_n(f, ids, (size_t)n_verts * 4) || !read_n(f, weights, (size_t)n_verts * 4) || !read_n(f, bones, (size_t)n_bones * 12)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);
    for (size_t k = 0; k < idx.size(); ++k)
        if (idx[k] >= n_verts) { fprintf(stderr, "index out of range\n"); return 2; }

    uint32_t vert = 0, slot = 0;
    if (skin::ids_check(ids.data(), n_verts, n_bones, &vert, &slot) != skin::kSkinOk) { printf("ids refused vertex %u slot %u\n", vert, slot); return 0; }
    printf("ids ok\n");
    const int w = skin::weights_check(weights.data(), n_verts, &vert, &slot);
    if (w != skin::kSkinOk) { printf("weights refused %s vertex %u\n", w == skin::kSkinWeight ? "weight" : "sum", vert); return 0; }
    printf("weights ok\n");
    float M[12], q[3];
    for (uint32_t v = 0; v < n_verts; ++v) {
        skin::blend(bones.data(), &ids[(size_t)v * 4], &weights[(size_t)v * 4], M);
        pose::point(M, &pos[(size_t)v * 3], q);
        printf("P %08x %08x %08x\n", bits(q[0]), bits(q[1]), bits(q[2]));
    }
    for (size_t k = 0; has_nrm && k < (size_t)n_tris * 3; ++k) {
        const uint32_t v = idx[k];                                          // the corner's own vertex
        skin::blend(bones.data(), &ids[(size_t)v * 4], &weights[(size_t)v * 4], M);
        pose::normal(M, &nrm[k * 3], q);
        printf("N %08x %08x %08x\n", bits(q[0]), bits(q[1]), bits(q[2]));
    }
    return 0;
}
