// refit_check.cpp -- the arithmetic of a refit (toyraygun_amd/csrc/trg_refit_math.h) evaluated on the host, the way trg_refit.hip's kernels apply it:
// leaf boxes, bottom-up ping-pong passes, quantisation, records, box frames.
//   * as a program (with bvh_build.cpp; host sanitizers welcome): scenes of cubes, lone quads and triangles are built, moved and refitted, and checked
//     against a fresh build of the moved geometry -- and every triangle against the decoded box of every ancestor, in both node flavours;
//   * as a shared object (-DREFIT_SHARED, without bvh_build.cpp): the same steps behind a C interface, for tests that hold the arrays of the
//     trg_debug_* entry points.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "trg_refit_math.h"

using namespace trg;
using refit::Geo;

namespace {

struct BoxRef { uint32_t first, count; };   // the records behind a box code of the box flavour

// rf_leaf_kernel + rf_pass_kernel x passes + rf_quantize_kernel for one node array.  Returns false when the passes had not settled.
bool refit_array(const Geo &g, const uint32_t *in, uint32_t n, const uint32_t *rec_prim, uint32_t n_rec, const BoxRef *boxes, uint32_t n_boxes, uint32_t passes, float pad,
                 uint32_t *out, uint8_t *quadx) {
    const float inf = INFINITY;
    std::vector<float> childbox((size_t)n * 24), leaf((size_t)n * 6), a, b;
    for (uint32_t i = 0; i < n; ++i) {
        float L[6] = { inf, inf, inf, -inf, -inf, -inf };
        for (int k = 0; k < 4; ++k) {
            float bx[6] = { inf, inf, inf, -inf, -inf, -inf };
            const int32_t c = (int32_t)in[(size_t)i * 16 + 12 + k];
            if (c < 0 && c != kQ4Empty) {
                const uint32_t code = (uint32_t)~c;
                uint32_t first = code >> 3, count;
                if ((code & 7u) == refit::kCodeBox) { const uint32_t bi = first - n_rec; if (bi >= n_boxes) return false; first = boxes[bi].first; count = boxes[bi].count; }
                else count = refit::code_records(code);
                if (first + count > n_rec) return false;
                for (uint32_t r = first; r < first + count; ++r) refit::grow_tri(g, rec_prim[r], bx, bx + 3);
                if (quadx && (code & 7u) == refit::kCodeQuad) quadx[first] = 1;
            }
            memcpy(&childbox[((size_t)i * 4 + k) * 6], bx, 24);
            for (int x = 0; x < 3; ++x) { L[x] = fminf(L[x], bx[x]); L[3 + x] = fmaxf(L[3 + x], bx[3 + x]); }
        }
        memcpy(&leaf[(size_t)i * 6], L, 24);
    }
    a = leaf; b.resize(a.size());
    auto pass = [&](const std::vector<float> &src, std::vector<float> &dst) {
        for (uint32_t i = 0; i < n; ++i) {
            float bx[6];
            memcpy(bx, &leaf[(size_t)i * 6], 24);
            for (int k = 0; k < 4; ++k) {
                const int32_t c = (int32_t)in[(size_t)i * 16 + 12 + k];
                if (c < 0 || (uint32_t)c >= n) continue;
                for (int x = 0; x < 3; ++x) { bx[x] = fminf(bx[x], src[(size_t)c * 6 + x]); bx[3 + x] = fmaxf(bx[3 + x], src[(size_t)c * 6 + 3 + x]); }
            }
            memcpy(&dst[(size_t)i * 6], bx, 24);
        }
    };
    for (uint32_t p = 0; p < passes; ++p) { pass(a, b); a.swap(b); }
    pass(a, b);
    const bool settled = memcmp(a.data(), b.data(), a.size() * 4) == 0;
    for (uint32_t i = 0; i < n; ++i) {
        float cb[24], f32[32];
        uint32_t child[4];
        for (int k = 0; k < 4; ++k) {
            child[k] = in[(size_t)i * 16 + 12 + k];
            const int32_t c = (int32_t)child[k];
            memcpy(cb + k * 6, c >= 0 ? &a[(size_t)c * 6] : &childbox[((size_t)i * 4 + k) * 6], 24);
        }
        refit::node_floats(cb, child, pad, f32);
        quantize_node4(f32, out + (size_t)i * 16);
    }
    return settled;
}

// every triangle inside the decoded box of every ancestor
bool contained(const Geo &g, const uint32_t *nodes, uint32_t n, const uint32_t *rec_prim, uint32_t n_rec, const BoxRef *boxes, uint32_t n_boxes, size_t *leaves_seen, bool report = true) {
    struct Item { uint32_t node; double lo[3], hi[3]; };
    std::vector<Item> st;
    Item root{ 0u, { -INFINITY, -INFINITY, -INFINITY }, { INFINITY, INFINITY, INFINITY } };
    st.push_back(root);
    size_t visited = 0;
    while (!st.empty()) {
        const Item it = st.back(); st.pop_back();
        if (++visited > n) return false;
        for (int k = 0; k < 4; ++k) {
            const int32_t c = (int32_t)nodes[(size_t)it.node * 16 + 12 + k];
            if (c == kQ4Empty) continue;
            Item ch{ 0u, {}, {} };
            refit::decode_child(&nodes[(size_t)it.node * 16], k, ch.lo, ch.hi);
            for (int a = 0; a < 3; ++a) { ch.lo[a] = std::max(ch.lo[a], it.lo[a]); ch.hi[a] = std::min(ch.hi[a], it.hi[a]); }   // inside this box AND every ancestor's
            if (c >= 0) { if ((uint32_t)c >= n) return false; ch.node = (uint32_t)c; st.push_back(ch); continue; }
            const uint32_t code = (uint32_t)~c;
            uint32_t first = code >> 3, count;
            if ((code & 7u) == refit::kCodeBox) { const uint32_t bi = first - n_rec; if (bi >= n_boxes) return false; first = boxes[bi].first; count = boxes[bi].count; }
            else count = refit::code_records(code);
            ++*leaves_seen;
            for (uint32_t r = first; r < first + count; ++r)
                for (int j = 0; j < 3; ++j) {
                    const float *p = refit::vtx(g, rec_prim[r], j);
                    for (int a = 0; a < 3; ++a)
                        if (!((double)p[a] >= ch.lo[a] && (double)p[a] <= ch.hi[a])) {
                            if (report) printf("triangle %u vertex %d axis %d: %.9g outside [%.9g, %.9g] (node %u child %d)\n", rec_prim[r], j, a, p[a], ch.lo[a], ch.hi[a], it.node, k);
                            return false;
                        }
                }
        }
    }
    return true;
}

}  // namespace

extern "C" {

// bounds, centre and padding of the indexed vertices
void rf_host_bounds(const float *pos, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, float *lo3, float *hi3, float *center3, float *pad) {
    const Geo g{ pos, idx, n_verts, n_tris };
    for (int a = 0; a < 3; ++a) { lo3[a] = INFINITY; hi3[a] = -INFINITY; }
    for (uint32_t t = 0; t < n_tris; ++t) refit::grow_tri(g, t, lo3, hi3);
    refit::scene_center(lo3, hi3, center3);
    *pad = refit::scene_pad(lo3, hi3);
}
// rf_records_kernel: the rows of the strict records (32 floats each, in place) and the 12 plane floats per record; quadx from rf_host_nodes
void rf_host_records(const float *pos, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, float *records32, uint32_t n_rec, const uint8_t *quadx, const float *center3,
                     float *planes12) {
    const Geo g{ pos, idx, n_verts, n_tris };
    for (uint32_t r = 0; r < n_rec; ++r) {
        float *mt = records32 + (size_t)r * 32, rows[12], yrows[12];
        refit::tri_rows(g, refit::f2u(mt[3]), rows);
        const float *e2row = rows + 8;
        if (quadx[r] && r + 1u < n_rec) { refit::tri_rows(g, refit::f2u(mt[32 + 3]), yrows); e2row = yrows + 8; }
        refit::plane_rows(rows, e2row, center3, planes12 + (size_t)r * 12);
        for (int k = 0; k < 3; ++k) { mt[k] = rows[k]; mt[4 + k] = rows[4 + k]; mt[8 + k] = rows[8 + k]; }
    }
}
// a plain node array (16 dwords per node) refitted; rec_prim = the original index of every record.  1: the passes settled
int rf_host_nodes(const float *pos, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, const uint32_t *nodes_in, uint32_t n_nodes, const uint32_t *rec_prim, uint32_t n_rec,
                  uint32_t passes, float pad, uint32_t *nodes_out, uint8_t *quadx) {
    const Geo g{ pos, idx, n_verts, n_tris };
    memset(quadx, 0, n_rec);
    return refit_array(g, nodes_in, n_nodes, rec_prim, n_rec, nullptr, 0, passes, pad, nodes_out, quadx) ? 1 : 0;
}
int rf_host_contained(const float *pos, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, const uint32_t *nodes, uint32_t n_nodes, const uint32_t *rec_prim, uint32_t n_rec) {
    const Geo g{ pos, idx, n_verts, n_tris };
    size_t leaves = 0;
    return contained(g, nodes, n_nodes, rec_prim, n_rec, nullptr, 0, &leaves, false) ? 1 : 0;
}
// the frame of the box whose twelve triangles begin at k0: centre (3), rows a_k (9), and the rows (a_k, d_k) of the box record (12).  1: still a box
int rf_host_box(const float *pos, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, uint32_t k0, const float *scene_center3, float *frame12, float *rows12) {
    const Geo g{ pos, idx, n_verts, n_tris };
    refit::Frame fr;
    uint32_t fq[6];
    if (!refit::box_group_pos(g, k0, fr, fq)) return 0;
    memcpy(frame12, fr.center, 12); memcpy(frame12 + 3, fr.axis, 36);
    refit::frame_rows(fr, scene_center3, rows12);
    return 1;
}
int rf_host_quad_still(const float *pos, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, uint32_t x, uint32_t y) {
    const Geo g{ pos, idx, n_verts, n_tris };
    return refit::quad_still(g, x, y) ? 1 : 0;
}
double rf_host_area(const uint32_t *nodes, uint32_t n_nodes) {
    double s = 0.0;
    for (uint32_t i = 0; i < n_nodes; ++i) s += refit::node_half_area(nodes + (size_t)i * 16);
    return s;
}
// the same sum in the order rf_area_kernel and rf_area_final_kernel add it: at most 1,024 blocks of 256 threads, every thread its strided share, the
// tree over a block's 256 partial sums, then the blocks in order (doubles: the order decides the last bits)
double rf_host_area_blocks(const uint32_t *nodes, uint32_t n_nodes) {
    const uint32_t kT = 256, nb = std::min<uint32_t>(1024u, (n_nodes + kT - 1) / kT);
    double total = 0.0;
    for (uint32_t b = 0; b < nb; ++b) {
        double sh[kT];
        for (uint32_t t = 0; t < kT; ++t) {
            sh[t] = 0.0;
            for (uint64_t i = (uint64_t)b * kT + t; i < n_nodes; i += (uint64_t)nb * kT) {
                const uint32_t *nd = nodes + (size_t)i * 16;
                if ((nd[12] | nd[13] | nd[14] | nd[15]) != 0u) sh[t] += refit::node_half_area(nd);
            }
        }
        for (uint32_t s = kT / 2; s > 0; s >>= 1)
            for (uint32_t t = 0; t < s; ++t) sh[t] += sh[t + s];
        total += sh[0];
    }
    return total;
}

}  // extern "C"

#ifndef REFIT_SHARED
#include "bvh_build.h"

namespace {
struct Mesh { std::vector<float> pos; std::vector<uint32_t> idx, mat; std::vector<int> cube_of_vertex; int cubes = 0; };
// a cube's 36 vertices (12 triangles, 6 quads, the (a,b,c)(a,c,d) pattern)
void add_cube(Mesh &m, float cx, float cy, float cz, float h) {
    const float c[8][3] = { {-1,-1,-1},{1,-1,-1},{1,1,-1},{-1,1,-1},{-1,-1,1},{1,-1,1},{1,1,1},{-1,1,1} };
    const int f[6][4] = { {0,1,2,3},{5,4,7,6},{4,0,3,7},{1,5,6,2},{3,2,6,7},{4,5,1,0} };
    for (int q = 0; q < 6; ++q) {
        const int t[6] = { f[q][0], f[q][1], f[q][2], f[q][0], f[q][2], f[q][3] };
        for (int k = 0; k < 6; ++k) {
            m.idx.push_back((uint32_t)(m.pos.size() / 3)); m.cube_of_vertex.push_back(m.cubes);
            m.pos.push_back(cx + h * c[t[k]][0]); m.pos.push_back(cy + h * c[t[k]][1]); m.pos.push_back(cz + h * c[t[k]][2]);
        }
        m.mat.push_back(1); m.mat.push_back(1);
    }
    ++m.cubes;
}
void add_tri(Mesh &m, const float v[3][3]) {
    for (int k = 0; k < 3; ++k) { m.idx.push_back((uint32_t)(m.pos.size() / 3)); m.cube_of_vertex.push_back(-1); for (int c = 0; c < 3; ++c) m.pos.push_back(v[k][c]); }
    m.mat.push_back(1);
}
void add_quad(Mesh &m, const float a[3], const float e1[3], const float e2[3]) {
    float v[4][3];
    for (int c = 0; c < 3; ++c) { v[0][c] = a[c]; v[1][c] = a[c] + e1[c]; v[2][c] = a[c] + e1[c] + e2[c]; v[3][c] = a[c] + e2[c]; }
    const float t0[3][3] = { { v[0][0], v[0][1], v[0][2] }, { v[1][0], v[1][1], v[1][2] }, { v[2][0], v[2][1], v[2][2] } };
    const float t1[3][3] = { { v[0][0], v[0][1], v[0][2] }, { v[2][0], v[2][1], v[2][2] }, { v[3][0], v[3][1], v[3][2] } };
    add_tri(m, t0); add_tri(m, t1);
}
// per cube a rigid-plus-shear map about the origin of the scene (in double, rounded once); everything else moves as one body by another such map
std::vector<float> moved(const Mesh &m, std::mt19937 &rng, double amount) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<std::array<double, 12>> maps((size_t)m.cubes + 1);
    for (auto &M : maps) {
        const double ang = amount * U(rng), c = std::cos(ang), s = std::sin(ang), sh = amount * U(rng);
        const double R[3][3] = { { c, 0, s }, { 0, 1, 0 }, { -s, 0, c } }, S[3][3] = { { 1, sh, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double v = 0; for (int k = 0; k < 3; ++k) v += R[i][k] * S[k][j]; M[(size_t)i * 3 + j] = v; }
        for (int i = 0; i < 3; ++i) M[9 + (size_t)i] = amount * U(rng);
    }
    std::vector<float> out(m.pos.size());
    for (size_t v = 0; v < m.pos.size() / 3; ++v) {
        const auto &M = maps[(size_t)(m.cube_of_vertex[v] + 1)];
        for (int i = 0; i < 3; ++i) out[v * 3 + i] = (float)(M[(size_t)i * 3] * m.pos[v * 3] + M[(size_t)i * 3 + 1] * m.pos[v * 3 + 1] + M[(size_t)i * 3 + 2] * m.pos[v * 3 + 2] + M[9 + (size_t)i]);
    }
    return out;
}
// the same triangles as an INDEXED mesh: every corner of a body stored once, two vertices that no triangle names (one far outside the scene), and the
// vertex buffer shuffled
Mesh indexed_copy(const Mesh &m, std::mt19937 &rng) {
    std::map<std::array<float, 4>, uint32_t> seen;
    std::vector<std::array<float, 3>> verts;
    std::vector<int> body;
    std::vector<uint32_t> idx;
    for (uint32_t i : m.idx) {
        const std::array<float, 4> key = { (float)m.cube_of_vertex[i], m.pos[(size_t)i * 3], m.pos[(size_t)i * 3 + 1], m.pos[(size_t)i * 3 + 2] };
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (uint32_t)verts.size()).first;
            verts.push_back({ key[1], key[2], key[3] }); body.push_back(m.cube_of_vertex[i]);
        }
        idx.push_back(it->second);
    }
    verts.push_back({ 1e6f, -1e6f, 1e6f }); body.push_back(-1);
    verts.push_back({ 0.5f, 0.5f, 0.5f }); body.push_back(-1);
    std::vector<uint32_t> perm(verts.size());
    for (size_t v = 0; v < perm.size(); ++v) perm[v] = (uint32_t)v;
    std::shuffle(perm.begin(), perm.end(), rng);
    Mesh o;
    o.mat = m.mat; o.cubes = m.cubes;
    o.pos.resize(verts.size() * 3); o.cube_of_vertex.resize(verts.size());
    for (size_t v = 0; v < verts.size(); ++v) {
        for (int c = 0; c < 3; ++c) o.pos[(size_t)perm[v] * 3 + c] = verts[v][c];
        o.cube_of_vertex[perm[v]] = body[v];
    }
    for (uint32_t i : idx) o.idx.push_back(perm[i]);
    return o;
}
struct Arrays { std::vector<uint32_t> rec_prim; std::vector<BoxRef> boxes; };
Arrays arrays_of(const Bvh &b) {
    Arrays a;
    for (size_t r = 0; r < b.tris.size() / 3; ++r) a.rec_prim.push_back(refit::f2u(b.tris[r * 3].w));
    for (const BoxLeaf &bl : b.boxes) a.boxes.push_back(BoxRef{ bl.first_rec, bl.node == ~0u ? 2u : 12u });
    return a;
}
size_t words_differing(const std::vector<uint32_t> &x, const uint32_t *y) { size_t d = 0; for (size_t i = 0; i < x.size(); ++i) d += x[i] != y[i]; return d; }
}  // namespace

int main() {
    std::mt19937 rng_plain(11);
    std::uniform_real_distribution<float> U(-5.f, 5.f);
    bool all_ok = true;
    double worst_frame = 0.0;
    std::mt19937 rng_indexed(12);   // (the indexed scene draws from a generator of its own: the other scenes are the ones they always were)
    struct Case { int n; bool indexed; };
    for (const Case cs : { Case{ 1, false }, Case{ 2, false }, Case{ 7, false }, Case{ 60, false }, Case{ 60, true }, Case{ 700, false } }) {
        const int n = cs.n;
        std::mt19937 &rng = cs.indexed ? rng_indexed : rng_plain;
        Mesh m;
        const float fa[3] = { -6.f, -6.f, -6.f }, fe1[3] = { 12.f, 0.f, 0.f }, fe2[3] = { 0.f, 0.f, 12.f };
        add_quad(m, fa, fe1, fe2);                                        // a floor
        for (int i = 0; i < n; ++i) add_cube(m, U(rng), U(rng), U(rng), 0.1f + 0.02f * (float)(i % 9));
        for (int i = 0; i < 3 + n / 2; ++i) { float v[3][3]; for (auto &p : v) for (float &c : p) c = U(rng); add_tri(m, v); }
        for (int q = 0; q < 2; ++q) { const float a[3] = { U(rng), U(rng), U(rng) }, e1[3] = { 1.f, 0.25f, 0.f }, e2[3] = { 0.f, 0.5f, 2.f }; add_quad(m, a, e1, e2); }
        if (cs.indexed) {
            const size_t corners = m.pos.size() / 3;
            m = indexed_copy(m, rng);
            printf("indexed n %d: %zu corners are %zu vertices, two of them named by no triangle\n", n, corners, m.pos.size() / 3);
            if (m.pos.size() / 3 >= corners) all_ok = false;
        }
        const uint32_t nt = (uint32_t)m.mat.size(), nv = (uint32_t)(m.pos.size() / 3);
        Bvh b0;
        build_bvh(m.pos.data(), m.idx.data(), m.mat.data(), nt, b0, false, true);
        const Arrays A = arrays_of(b0);
        const uint32_t n_rec = (uint32_t)A.rec_prim.size(), passes = std::max(b0.depth4, b0.depth4_box);
        for (int motion = 0; motion < 3; ++motion) {   // 0: identity, 1: small, 2: large
            const std::vector<float> pos = motion == 0 ? m.pos : moved(m, rng, motion == 1 ? 0.02 : 0.8);
            const Geo g{ pos.data(), m.idx.data(), nv, nt };
            float lo[3], hi[3], center[3], pad;
            rf_host_bounds(pos.data(), m.idx.data(), nv, nt, lo, hi, center, &pad);
            float ilo[3] = { INFINITY, INFINITY, INFINITY }, ihi[3] = { -INFINITY, -INFINITY, -INFINITY };   // the bounds are those of the vertices the triangles name
            for (uint32_t i : m.idx) for (int a = 0; a < 3; ++a) { ilo[a] = std::min(ilo[a], pos[(size_t)i * 3 + a]); ihi[a] = std::max(ihi[a], pos[(size_t)i * 3 + a]); }
            if (memcmp(lo, ilo, 12) || memcmp(hi, ihi, 12)) { printf("n %d motion %d: the bounds are not those of the indexed vertices\n", n, motion); all_ok = false; }
            std::vector<uint32_t> plain((size_t)b0.n_nodes4 * 16), boxf((size_t)b0.n_nodes4_box * 16);
            std::vector<uint8_t> quadx(n_rec, 0);
            bool ok = refit_array(g, b0.nodes4q.data(), b0.n_nodes4, A.rec_prim.data(), n_rec, nullptr, 0, passes, pad, plain.data(), quadx.data());
            if (b0.n_nodes4_box) ok = refit_array(g, b0.nodes4q_box.data(), b0.n_nodes4_box, A.rec_prim.data(), n_rec, A.boxes.data(), (uint32_t)A.boxes.size(), passes, pad, boxf.data(), nullptr) && ok;
            if (!ok) { printf("n %d motion %d: the passes did not settle in %u\n", n, motion, passes); all_ok = false; }
            // the quad marks are the builder's
            for (uint32_t r = 0; r < n_rec; ++r) if ((quadx[r] != 0) != (b0.quad[r] != 0)) { printf("n %d: quad mark of record %u differs\n", n, r); all_ok = false; break; }
            for (uint32_t r = 0; r < n_rec; ++r)
                if (quadx[r] && !refit::quad_still(g, A.rec_prim[r], A.rec_prim[r + 1])) { printf("n %d motion %d: quad at record %u refused\n", n, motion, r); all_ok = false; break; }
            if (motion == 0) {
                const size_t dp = words_differing(b0.nodes4q, plain.data()), db = words_differing(b0.nodes4q_box, boxf.data());
                printf("identity n %d: plain nodes differ in %zu of %zu words, box flavour in %zu of %zu\n", n, dp, b0.nodes4q.size(), db, b0.nodes4q_box.size());
                if (dp || db) all_ok = false;
            }
            // a fresh build of the moved geometry: records by primitive index, frames by first triangle
            Bvh b1;
            build_bvh(pos.data(), m.idx.data(), m.mat.data(), nt, b1, false, true);
            std::vector<const F4 *> fresh(nt, nullptr);
            for (size_t r = 0; r < b1.tris.size() / 3; ++r) fresh[refit::f2u(b1.tris[r * 3].w)] = &b1.tris[r * 3];
            for (uint32_t r = 0; r < n_rec; ++r) {
                float rows[12];
                refit::tri_rows(g, A.rec_prim[r], rows);
                const F4 *f = fresh[A.rec_prim[r]];
                if (!f || memcmp(rows, &f[0], 12) || memcmp(rows + 4, &f[1], 12) || memcmp(rows + 8, &f[2], 12)) { printf("n %d motion %d: strict rows of triangle %u differ\n", n, motion, A.rec_prim[r]); all_ok = false; break; }
            }
            if (b1.boxes.size() != b0.boxes.size()) { printf("n %d motion %d: %zu boxes, the fresh build finds %zu\n", n, motion, b0.boxes.size(), b1.boxes.size()); all_ok = false; }
            for (const BoxLeaf &bl : b0.boxes) {
                uint32_t k0 = ~0u;
                for (uint32_t r = 0; r < (bl.node == ~0u ? 2u : 12u); ++r) k0 = std::min(k0, A.rec_prim[bl.first_rec + r]);
                refit::Frame fr;
                bool okb;
                if (bl.node == ~0u) {
                    float xr[12], yr[12];
                    refit::tri_rows(g, A.rec_prim[bl.first_rec], xr); refit::tri_rows(g, A.rec_prim[bl.first_rec + 1], yr);
                    okb = refit::lone_quad_frame(xr, yr + 8, fr);
                } else {
                    uint32_t fq[6];
                    okb = refit::box_group_pos(g, k0, fr, fq);
                }
                const BoxLeaf *match = nullptr;
                for (const BoxLeaf &c : b1.boxes) {
                    uint32_t k1 = ~0u;
                    for (uint32_t r = 0; r < (c.node == ~0u ? 2u : 12u); ++r) k1 = std::min(k1, refit::f2u(b1.tris[(size_t)(c.first_rec + r) * 3].w));
                    if (k1 == k0 && (c.node == ~0u) == (bl.node == ~0u)) match = &c;
                }
                if (!okb || !match) { printf("n %d motion %d: box at triangle %u: refit %d, fresh %d\n", n, motion, k0, (int)okb, match != nullptr); all_ok = false; continue; }
                for (int a = 0; a < 3; ++a) {
                    worst_frame = std::max(worst_frame, (double)std::fabs(fr.center[a] - match->center[a]));
                    for (int k = 0; k < 3; ++k) {
                        const double scale = std::max(1e-30, (double)std::fabs(match->axis[k][a]));
                        if (bl.node != ~0u || k < 2 || std::fabs(match->axis[k][a]) > 0) worst_frame = std::max(worst_frame, std::fabs((double)fr.axis[k][a] - (double)match->axis[k][a]) / std::max(scale, 1.0));
                    }
                }
            }
            size_t leaves = 0;
            if (!contained(g, plain.data(), b0.n_nodes4, A.rec_prim.data(), n_rec, nullptr, 0, &leaves)) { printf("n %d motion %d: plain flavour does not contain its triangles\n", n, motion); all_ok = false; }
            if (b0.n_nodes4_box && !contained(g, boxf.data(), b0.n_nodes4_box, A.rec_prim.data(), n_rec, A.boxes.data(), (uint32_t)A.boxes.size(), &leaves)) { printf("n %d motion %d: box flavour does not contain its triangles\n", n, motion); all_ok = false; }
            printf("n %d motion %d: %u records, %zu boxes, %zu leaves walked, area ratio %.4f / %.4f\n", n, motion, n_rec, b0.boxes.size(), leaves,
                   rf_host_area(plain.data(), b0.n_nodes4) / rf_host_area(b0.nodes4q.data(), b0.n_nodes4),
                   b0.n_nodes4_box ? rf_host_area(boxf.data(), b0.n_nodes4_box) / rf_host_area(b0.nodes4q_box.data(), b0.n_nodes4_box) : 0.0);
        }
    }
    printf("box frames against the fresh build: worst difference %.3g\n", worst_frame);
    printf(all_ok ? "refit check: every scene passed\n" : "refit check: FAILED\n");
    return all_ok ? 0 : 1;
}
#endif
