#include "bvh_build.h"
#include "q4node.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <random>
using namespace trg;
// a cube's 36 vertices (12 triangles, 6 quads, the (a,b,c)(a,c,d) pattern)
static void add_cube(std::vector<float> &pos, std::vector<uint32_t> &idx, std::vector<uint32_t> &mat, float cx, float cy, float cz, float h) {
    const float c[8][3] = { {-1,-1,-1},{1,-1,-1},{1,1,-1},{-1,1,-1},{-1,-1,1},{1,-1,1},{1,1,1},{-1,1,1} };
    const int f[6][4] = { {0,1,2,3},{5,4,7,6},{4,0,3,7},{1,5,6,2},{3,2,6,7},{4,5,1,0} };
    for (int q = 0; q < 6; ++q) {
        const int t[6] = { f[q][0], f[q][1], f[q][2], f[q][0], f[q][2], f[q][3] };
        for (int k = 0; k < 6; ++k) { idx.push_back((uint32_t)(pos.size() / 3)); pos.push_back(cx + h * c[t[k]][0]); pos.push_back(cy + h * c[t[k]][1]); pos.push_back(cz + h * c[t[k]][2]); }
        mat.push_back(1); mat.push_back(1);
    }
}
// The highest stack level a traversal of a quantised 4-wide tree (16 dwords per node, children in words 12..15) can write, and the tree's depth in
// levels of inner nodes.  trg_device.h wide_select: level 0 holds the sentinel; a node entered with `pending` entries above it stores its three
// candidates at levels pending + 1 .. pending + 3 whether it keeps them or not, keeps one per further child the ray enters, and ANY child may be
// the nearest: an inner child of a node with m children is entered with up to pending + m - 1 entries pending.  Leaves store nothing.
static bool worst_stack_level(const std::vector<uint32_t> &q, uint32_t n_nodes, uint32_t &top, uint32_t &depth) {
    struct Item { uint32_t node, pending, d; };
    std::vector<Item> st;
    top = 0; depth = 0;
    if (n_nodes) st.push_back({ 0u, 0u, 1u });
    size_t visited = 0;
    while (!st.empty()) {
        const Item it = st.back(); st.pop_back();
        if (++visited > n_nodes) return false;   // (a cycle or a node with two parents)
        top = std::max(top, it.pending + 3u); depth = std::max(depth, it.d);
        const uint32_t *w = &q[(size_t)it.node * 16];
        uint32_t m = 0;
        for (int k = 0; k < 4; ++k) m += (int32_t)w[12 + k] != (int32_t)0x80000000;
        for (int k = 0; k < 4; ++k) {
            const int32_t c = (int32_t)w[12 + k];
            if (c >= 0) { if ((uint32_t)c >= n_nodes) return false; st.push_back({ (uint32_t)c, it.pending + m - 1u, it.d + 1u }); }
        }
    }
    return true;
}
// both collapses of a scene against the levels the host allots (bvh_build.h wide_stack_levels of the deeper of the two: trg_capi.cpp build_host_scene)
static int deeper_box_flavours = 0;
static bool stack_fits(const Bvh &b, const char *what) {
    uint32_t top = 0, depth = 0, top_box = 0, depth_box = 0;
    if (!worst_stack_level(b.nodes4q, b.n_nodes4, top, depth) || !worst_stack_level(b.nodes4q_box, b.n_nodes4_box, top_box, depth_box)) { printf("%s: bad tree\n", what); return false; }
    if (depth != b.depth4 || depth_box != b.depth4_box) { printf("%s: depth4 %u/%u, walked %u/%u\n", what, b.depth4, b.depth4_box, depth, depth_box); return false; }
    const uint32_t levels = wide_stack_levels(std::max(b.depth4, b.depth4_box));
    if (b.depth4_box > b.depth4) { ++deeper_box_flavours; printf("%s: the box flavour is DEEPER than the plain collapse, %u > %u\n", what, b.depth4_box, b.depth4); }
    // (what the parent of this check sized the stack by -- the plain collapse alone -- must be said when it would not have been enough)
    if (top_box + 1u > wide_stack_levels(b.depth4)) printf("%s: the box flavour writes level %u, the plain collapse's %u levels would not hold it\n", what, top_box, wide_stack_levels(b.depth4));
    if (top + 1u > levels || top_box + 1u > levels) { printf("%s: stack levels written %u / %u, allotted %u\n", what, top, top_box, levels); return false; }
    return true;
}
int main() {
    std::mt19937 rng(5);
    // where the two collapses could part: cubes nested in cubes (every box's subtree root sits inside the next one's bounds), long rows of touching
    // cubes (a spine of a tree), both beside a cloud of small ones, and random clouds of every size -- the stack check alone
    {
        int scenes = 0;
        std::uniform_real_distribution<float> U(-5.f, 5.f);
        for (int kind = 0; kind < 4; ++kind) for (int n : { 2, 3, 5, 8, 13, 21, 34, 55, 89, 144 }) for (int rep = 0; rep < (kind == 3 ? 12 : 2); ++rep) {
            std::vector<float> pos; std::vector<uint32_t> idx, mat;
            if (kind == 0 || kind == 2) for (int i = 0; i < n; ++i) add_cube(pos, idx, mat, 0.f, 0.f, 0.f, 0.05f * (float)(i + 1));           // nested
            if (kind == 1 || kind == 2) for (int i = 0; i < n; ++i) add_cube(pos, idx, mat, 8.f + 0.2f * (float)i, 0.f, 0.f, 0.1f);            // a row, face to face
            if (kind >= 2) for (int i = 0; i < (kind == 3 ? n : n / 2 + rep); ++i) add_cube(pos, idx, mat, U(rng), U(rng), U(rng), kind == 3 ? 0.02f * (float)(1 + i % 17) : 0.1f);
            if (rep) { for (int k = 0; k < 3; ++k) { idx.push_back((uint32_t)(pos.size() / 3)); pos.push_back(U(rng)); pos.push_back(U(rng)); pos.push_back(U(rng)); } mat.push_back(1); }
            Bvh b;
            build_bvh(pos.data(), idx.data(), mat.data(), (uint32_t)mat.size(), b, false, true);
            char what[64]; snprintf(what, sizeof what, "kind %d n %d rep %d", kind, n, rep);
            if (!stack_fits(b, what)) return 1;
            ++scenes;
        }
        printf("stack: %d scenes of nested, touching and random cubes fit the levels allotted; box flavour deeper than the plain collapse in %d\n", scenes, deeper_box_flavours);
    }
    for (int n : { 1, 2, 7, 300, 9000 }) {
        std::vector<float> pos; std::vector<uint32_t> idx, mat;
        std::uniform_real_distribution<float> U(-5.f, 5.f);
        for (int i = 0; i < n; ++i) add_cube(pos, idx, mat, U(rng), U(rng), U(rng), 0.1f);
        // a lone triangle and two lone quads too (the quads become boxes of no thickness in the box flavour)
        for (int k = 0; k < 3; ++k) { idx.push_back((uint32_t)(pos.size() / 3)); pos.push_back(U(rng)); pos.push_back(U(rng)); pos.push_back(U(rng)); }
        mat.push_back(1);
        for (int q = 0; q < 2; ++q) {
            const float a[3] = { U(rng), U(rng), U(rng) }, e1[3] = { 1.f, 0.25f, 0.f }, e2[3] = { 0.f, 0.5f, 2.f };
            const float v[4][3] = { { a[0], a[1], a[2] }, { a[0] + e1[0], a[1] + e1[1], a[2] + e1[2] }, { a[0] + e1[0] + e2[0], a[1] + e1[1] + e2[1], a[2] + e1[2] + e2[2] }, { a[0] + e2[0], a[1] + e2[1], a[2] + e2[2] } };
            const int t[6] = { 0, 1, 2, 0, 2, 3 };
            for (int k = 0; k < 6; ++k) { idx.push_back((uint32_t)(pos.size() / 3)); for (int c = 0; c < 3; ++c) pos.push_back(v[t[k]][c]); }
            mat.push_back(1); mat.push_back(1);
        }
        Bvh b;
        build_bvh(pos.data(), idx.data(), mat.data(), (uint32_t)mat.size(), b, false, true);
        if (n == 7) {
            // hostile cubes: the same scene again with cubes of no size, of no thickness, at 1e30, with a NaN / an infinite corner, with two materials,
            // and one whose corner is off by 1e-3 -- none of them may be taken for a box (or crash the builder); the seven good ones still are
            std::vector<float> p2 = pos; std::vector<uint32_t> i2 = idx, m2 = mat;
            const size_t v0 = p2.size() / 3;
            auto cube_at = [&](float h, float cx) { add_cube(p2, i2, m2, cx, 8.f, 8.f, h); return p2.size() / 3 - 36; };
            cube_at(0.f, 1.f);                                                         // a point
            { const size_t c = cube_at(0.1f, 2.f); for (size_t v = c; v < c + 36; ++v) p2[v * 3 + 2] = 8.f; }          // flat
            { const size_t c = cube_at(0.1f, 3.f); for (size_t v = c; v < c + 36; ++v) for (int a = 0; a < 3; ++a) p2[v * 3 + a] *= 1e30f; }
            { const size_t c = cube_at(0.1f, 4.f); p2[c * 3] = std::nanf(""); }
            { const size_t c = cube_at(0.1f, 5.f); p2[(c + 7) * 3 + 1] = INFINITY; }
            { cube_at(0.1f, 6.f); m2[m2.size() - 1] = 2; }
            { const size_t c = cube_at(0.1f, 7.f); p2[(c + 2) * 3] += 1e-3f; }
            (void)v0;
            Bvh h;
            build_bvh(p2.data(), i2.data(), m2.data(), (uint32_t)m2.size(), h, false, true);
            if (h.n_boxes_real != 7u) { printf("hostile cubes: %u boxes\n", h.n_boxes_real); return 1; }
            printf("hostile cubes: none taken for a box\n");
        }
        const uint32_t nrec = (uint32_t)(b.tris.size() / 3);
        std::vector<int> seen(nrec, 0);
        size_t box_refs = 0;
        for (uint32_t i = 0; i < b.n_nodes4_box; ++i) {
            const uint32_t *w = &b.nodes4q_box[(size_t)i * 16];
            for (int k = 0; k < 4; ++k) {
                const int32_t c = (int32_t)w[12 + k];
                if (c == (int32_t)0x80000000) continue;
                if (c >= 0) { if ((uint32_t)c >= b.n_nodes4_box) { printf("bad inner %d\n", c); return 1; } continue; }
                const uint32_t code = (uint32_t)~c, first = code >> 3, cnt = code & 7u;
                if (cnt == kLeafBox) {
                    if (first < nrec || first - nrec >= b.boxes.size()) { printf("bad box %u\n", first); return 1; }
                    const uint32_t first = (code >> 3) - nrec;      // (a box is addressed like a record behind the records)
                    ++box_refs;
                    for (uint32_t r = 0; r < (b.boxes[first].node == ~0u ? 2u : 12u); ++r) seen[b.boxes[first].first_rec + r]++;
                } else {
                    const uint32_t m = leaf_count(code);
                    if (first + m > nrec) { printf("bad leaf\n"); return 1; }
                    for (uint32_t r = 0; r < m; ++r) seen[first + r]++;
                }
            }
        }
        bool ok = true;
        if (b.n_nodes4_box) for (uint32_t r = 0; r < nrec; ++r) ok = ok && seen[r] == 1;
        if (b.n_boxes_real != (uint32_t)n || (b.n_nodes4_box && b.boxes.size() != (size_t)n + 2)) { printf("box counts: %u real, %zu all\n", b.n_boxes_real, b.boxes.size()); return 1; }
        printf("n=%d tris=%zu boxes=%zu nodes4=%u nodes4_box=%u box_refs=%zu depth4 %u/%u every record once: %s\n", n, mat.size(), b.boxes.size(), b.n_nodes4, b.n_nodes4_box, box_refs, b.depth4, b.depth4_box, ok ? "yes" : "NO");
        if (!ok || box_refs != (b.n_nodes4_box ? b.boxes.size() : 0)) return 1;
        if (!stack_fits(b, "cloud")) return 1;
    }
    printf("stack: every scene fits; box flavour deeper than the plain collapse in %d\n", deeper_box_flavours);
    return 0;
}
