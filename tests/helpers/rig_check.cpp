// rig_check.cpp -- the arithmetic, the checks and the level table of a rig (toyraygun_amd/csrc/trg_rig_math.h) run on the host, the way
// trg_rig_bind and the rig kernel of trg_refit.hip apply them, on arrays of exactly the stated sizes.  A program of its own (host sanitizers
// welcome):
//
//   rig_check <input>       input: uint32 n_joints, n_keys, n_clocks, has_inv_bind, n_clock_vectors; uint32 parent[n_joints];
//                           uint32 key_first[n_joints + 1]; float keys[12 n_keys]; uint32 clock_of[n_joints]; float inv_bind[12 n_joints] (if any);
//                           float clocks[n_clock_vectors][n_clocks]
//
// prints what the checks say and -- for a rig that passes -- the level table and, per clock vector, the bits of every matrix:
//   check ok | check refused <code> joint <j> key <k>         code: the number of trg::rig's enum
//   levels <n>                                                 then  L <level> <first> <count>   and   O <the joints in launch order>
//   depth refused joint <j>
//   V <vector>   then per joint   B <12 hex words>   and   W <12 hex words>
//   F <4 hex words>  twice: the sampling fallback on a pair of zero length, and on one whose length overflows
#include <cstdio>
#include <cstring>
#include <vector>

#include "trg_rig_math.h"

using namespace trg;

namespace {
template <typename T>
bool read_n(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
void row(const char *tag, const float *m, int n) {
    printf("%s", tag);
    for (int k = 0; k < n; ++k) printf(" %08x", bits(m[k]));
    printf("\n");
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: rig_check <input>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5];
    if (fread(head, 4, 5, f) != 5) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n_joints = head[0], n_keys = head[1], n_clocks = head[2], n_vectors = head[4];
    const bool has_inv = head[3] != 0;
    std::vector<uint32_t> parent, kfirst, clock_of;
    std::vector<float> keys, inv_bind, clocks;
    if (!read_n(f, parent, n_joints) || !read_n(f, kfirst, (size_t)n_joints + 1) || !read_n(f, keys, (size_t)n_keys * 12) || !read_n(f, clock_of, n_joints) ||
        !read_n(f, inv_bind, has_inv ? (size_t)n_joints * 12 : 0) || !read_n(f, clocks, (size_t)n_vectors * n_clocks)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    // the fallback of the normalised lerp: a length of zero, and one that is not finite -- the first rotation comes back, bits and all
    const float zero[4] = { 0.f, -0.f, 0.f, 0.f }, big[4] = { 3e38f, 3e38f, -3e38f, 1.f };
    float q[4];
    rig::nlerp(zero, zero, 0.5f, q);
    row("F", q, 4);
    rig::nlerp(big, big, 0.5f, q);
    row("F", q, 4);

    uint32_t joint = 0, key = 0;
    const int what = rig::check(parent.data(), n_joints, kfirst.data(), keys.data(), n_keys, clock_of.data(), n_clocks, has_inv ? inv_bind.data() : nullptr, &joint, &key);
    if (what != rig::kRigOk) { printf("check refused %d joint %u key %u\n", what, joint, key); return 0; }
    printf("check ok\n");
    std::vector<uint32_t> depth(n_joints), order(n_joints), level_first(rig::kMaxLevels + 1);
    uint32_t n_levels = 0;
    if (rig::levels(parent.data(), n_joints, depth.data(), order.data(), level_first.data(), &n_levels, &joint) != rig::kRigOk) { printf("depth refused joint %u\n", joint); return 0; }
    printf("levels %u\n", n_levels);
    for (uint32_t l = 0; l < n_levels; ++l) printf("L %u %u %u\n", l, level_first[l], level_first[l + 1] - level_first[l]);
    printf("O");
    for (uint32_t k = 0; k < n_joints; ++k) printf(" %u", order[k]);
    printf("\n");
    std::vector<float> world((size_t)n_joints * 12), bones((size_t)n_joints * 12);
    for (uint32_t v = 0; v < n_vectors; ++v) {
        rig::evaluate(parent.data(), kfirst.data(), keys.data(), clock_of.data(), has_inv ? inv_bind.data() : nullptr, clocks.data() + (size_t)v * n_clocks, order.data(),
                      level_first.data(), n_levels, world.data(), bones.data());
        printf("V %u\n", v);
        for (uint32_t j = 0; j < n_joints; ++j) { row("B", &bones[(size_t)j * 12], 12); row("W", &world[(size_t)j * 12], 12); }
    }
    return 0;
}
