// morph_check.cpp -- the arithmetic, the checks and the transposition of blend shapes (toyraygun_amd/csrc/trg_morph_math.h) run on the host, the way
// trg_morph_bind and the morph kernel of trg_refit.hip apply them.  A program of its own (host sanitizers welcome):
//
//   morph_check <input>     input: uint32 n_verts, n_tris, n_targets, n_entries, n_bones, has_normals, has_normal_deltas, list_records;
//                           float positions[3 n_verts]; float normals[9 n_tris] (if any); uint32 indices[3 n_tris]; uint32 target_first[n_targets + 1];
//                           uint32 entry_vertex[n_entries]; float dpos[3 n_entries]; float dnrm[3 n_entries] (if any); float target_weights[n_targets];
//                           uint32 ids[4 n_verts]; float weights[4 n_verts]; float bones[12 n_bones] (the last three if n_bones)
//
// prints what the two checks say and -- for targets that pass -- the transposed records (list_records) and the morphed bits:
//   targets ok | targets refused <first|order|end> target <k>
//   entries ok | entries refused <vertex|order|delta|normal-delta> target <k> entry <e>
//   F <vfirst[v]>                        per vertex and one more, decimal
//   R <target> <dx> <dy> <dz>            per position record, the target decimal, the delta as hex words
//   Q <target> <dx> <dy> <dz>            per normal record
//   P <x> <y> <z>                        per vertex, hex words
//   N <x> <y> <z>                        per corner, hex words
#include <cstdio>
#include <cstring>
#include <vector>

#include "trg_morph_math.h"

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
    if (argc != 2) { fprintf(stderr, "usage: morph_check <input>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[8];
    if (fread(head, 4, 8, f) != 8) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n_verts = head[0], n_tris = head[1], n_targets = head[2], n_entries = head[3], n_bones = head[4];
    const bool has_nrm = head[5] != 0, has_dnrm = head[6] != 0, list_records = head[7] != 0;
    std::vector<float> pos, nrm, dpos, dnrm, tw, weights, bones;
    std::vector<uint32_t> idx, first, ev, ids;
    // the entry arrays are read as long as the file says: a table with a wrong end is refused before anything indexes them
    if (!read_n(f, pos, (size_t)n_verts * 3) || !read_n(f, nrm, has_nrm ? (size_t)n_tris * 9 : 0) || !read_n(f, idx, (size_t)n_tris * 3) ||
        !read_n(f, first, (size_t)n_targets + 1) || !read_n(f, ev, n_entries) || !read_n(f, dpos, (size_t)n_entries * 3) ||
        !read_n(f, dnrm, has_dnrm ? (size_t)n_entries * 3 : 0) || !read_n(f, tw, n_targets) || !read_n(f, ids, n_bones ? (size_t)n_verts * 4 : 0) ||
        !read_n(f, weights, n_bones ? (size_t)n_verts * 4 : 0) || !read_n(f, bones, (size_t)n_bones * 12)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);
    if (n_targets == 0 || (has_dnrm && !has_nrm)) { fprintf(stderr, "no targets, or normal deltas without normals\n"); return 2; }
    for (size_t k = 0; k < idx.size(); ++k)
        if (idx[k] >= n_verts) { fprintf(stderr, "index out of range\n"); return 2; }

    uint32_t target = 0, entry = 0;
    const int t = morph::targets_check(first.data(), n_targets, n_entries, &target);
    if (t != morph::kTargetsOk) {
        printf("targets refused %s target %u\n", t == morph::kTargetsFirst ? "first" : t == morph::kTargetsOrder ? "order" : "end", target);
        return 0;
    }
    printf("targets ok\n");
    const int e = morph::entries_check(first.data(), n_targets, ev.data(), n_verts, dpos.data(), has_dnrm ? dnrm.data() : nullptr, &target, &entry);
    if (e != morph::kEntriesOk) {
        printf("entries refused %s target %u entry %u\n",
               e == morph::kEntriesVertex ? "vertex" : e == morph::kEntriesOrder ? "order" : e == morph::kEntriesDelta ? "delta" : "normal-delta", target, entry);
        return 0;
    }
    printf("entries ok\n");
    if (n_bones) {
        uint32_t vert = 0, slot = 0;
        if (skin::ids_check(ids.data(), n_verts, n_bones, &vert, &slot) != skin::kSkinOk || skin::weights_check(weights.data(), n_verts, &vert, &slot) != skin::kSkinOk) {
            printf("skin refused vertex %u\n", vert);
            return 0;
        }
    }
    // exactly as large as the unit makes them: the sanitizer sees an index one past either end
    std::vector<uint32_t> vfirst((size_t)n_verts + 1), cursor(n_verts);
    std::vector<morph::Rec> pos_recs(n_entries), nrm_recs(has_dnrm ? n_entries : 0);
    morph::transpose(first.data(), n_targets, ev.data(), dpos.data(), has_dnrm ? dnrm.data() : nullptr, n_verts, vfirst.data(), cursor.data(), pos_recs.data(),
                     has_dnrm ? nrm_recs.data() : nullptr);
    if (list_records) {
        for (uint32_t v = 0; v <= n_verts; ++v) printf("F %u\n", vfirst[v]);
        for (const morph::Rec &r : pos_recs) printf("R %u %08x %08x %08x\n", r.target, bits(r.d[0]), bits(r.d[1]), bits(r.d[2]));
        for (const morph::Rec &r : nrm_recs) printf("Q %u %08x %08x %08x\n", r.target, bits(r.d[0]), bits(r.d[1]), bits(r.d[2]));
    }
    float q[3];
    for (uint32_t v = 0; v < n_verts; ++v) {
        morph::vertex(&pos[(size_t)v * 3], vfirst.data(), pos_recs.data(), tw.data(), v, n_bones ? &ids[(size_t)v * 4] : nullptr, n_bones ? &weights[(size_t)v * 4] : nullptr,
                      n_bones ? bones.data() : nullptr, q);
        printf("P %08x %08x %08x\n", bits(q[0]), bits(q[1]), bits(q[2]));
    }
    for (size_t k = 0; has_nrm && k < (size_t)n_tris * 3; ++k) {
        const uint32_t v = idx[k];                                          // the corner's own vertex
        morph::corner(&nrm[k * 3], vfirst.data(), has_dnrm ? nrm_recs.data() : nullptr, tw.data(), v, n_bones ? &ids[(size_t)v * 4] : nullptr,
                      n_bones ? &weights[(size_t)v * 4] : nullptr, n_bones ? bones.data() : nullptr, q);
        printf("N %08x %08x %08x\n", bits(q[0]), bits(q[1]), bits(q[2]));
    }
    return 0;
}
