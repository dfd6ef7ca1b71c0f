// pose_check.cpp -- the arithmetic and the maps of a pose (toyraygun_amd/csrc/trg_pose_math.h) run on the host, the way trg_pose_bind and the pose
// kernel of trg_refit.hip apply them.  A program of its own (host sanitizers welcome):
//
//   pose_check <input>      input: uint32 n_verts, n_tris, n_objects, has_normals; float positions[3 n_verts]; float normals[9 n_tris] (if any);
//                           uint32 indices[3 n_tris]; uint32 first[n_objects + 1]; float xforms[12 n_objects]
//
// prints what the table check and the vertex map say and -- for a table that passes -- the two maps and the posed bits:
//   table ok | table refused <kind> object <j>
//   vertices ok | vertices refused <kind> triangle <t> vertex <v>
//   T <object of triangle> ...           one line
//   V <object of vertex, or ffffffff> ...  one line
//   P <x> <y> <z>                        per vertex, hex words
//   N <x> <y> <z>                        per corner, hex words
#include <cstdio>
#include <cstring>
#include <vector>

#include "trg_pose_math.h"

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
    if (argc != 2) { fprintf(stderr, "usage: pose_check <input>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n_verts = head[0], n_tris = head[1], n_objects = head[2];
    const bool has_nrm = head[3] != 0;
    std::vector<float> pos, nrm, xf;
    std::vector<uint32_t> idx, first;
    if (!read_n(f, pos, (size_t)n_verts * 3) || !read_n(f, nrm, has_nrm ? (size_t)n_tris * 9 : 0) || !read_n(f, idx, (size_t)n_tris * 3) ||
        !read_n(f, first, (size_t)n_objects + 1) || !read_n(f, xf, (size_t)n_objects * 12)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);

    static const char *const table_kind[] = { "ok", "first", "order", "end" }, *const verts_kind[] = { "ok", "index", "shared" };
    uint32_t obj = 0, tri = 0, vert = 0;
    const int t = pose::table_check(first.data(), n_objects, n_tris, &obj);
    if (t != pose::kTableOk) { printf("table refused %s object %u\n", table_kind[t], obj); return 0; }
    printf("table ok\n");
    std::vector<uint32_t> tri_obj(n_tris), vtx_obj(n_verts);
    pose::triangle_objects(first.data(), n_objects, tri_obj.data());
    const int v = pose::vertex_objects(idx.data(), n_verts, n_tris, tri_obj.data(), vtx_obj.data(), &tri, &vert);
    if (v != pose::kVertsOk) { printf("vertices refused %s triangle %u vertex %u\n", verts_kind[v], tri, vert); return 0; }
    printf("vertices ok\n");
    printf("T");
    for (uint32_t k = 0; k < n_tris; ++k) printf(" %x", tri_obj[k]);
    printf("\nV");
    for (uint32_t k = 0; k < n_verts; ++k) printf(" %x", vtx_obj[k]);
    printf("\n");
    for (uint32_t k = 0; k < n_verts; ++k) {
        float q[3] = { pos[(size_t)k * 3], pos[(size_t)k * 3 + 1], pos[(size_t)k * 3 + 2] };
        if (vtx_obj[k] != pose::kNoObject) pose::point(&xf[(size_t)vtx_obj[k] * 12], &pos[(size_t)k * 3], q);
        printf("P %08x %08x %08x\n", bits(q[0]), bits(q[1]), bits(q[2]));
    }
    for (size_t k = 0; has_nrm && k < (size_t)n_tris * 3; ++k) {
        float q[3];
        pose::normal(&xf[(size_t)tri_obj[k / 3] * 12], &nrm[k * 3], q);
        printf("N %08x %08x %08x\n", bits(q[0]), bits(q[1]), bits(q[2]));
    }
    return 0;
}
