// trg_ctx.h -- the one definition of the render context (private: include/trg.h only names the type).  trg_capi.cpp owns the context;
// trg_denoise.hip and trg_refit.hip read it and hang their per-context state on it.  Part of the kernel-source hash (srchash.py): launch
// planning reads these fields.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/trg.h"
#include "trg_kernels.h"

namespace trg {
struct DenoiseState;   // trg_denoise.hip
struct RefitState;     // trg_refit.hip
}  // namespace trg

struct trg_ctx {
    int device = 0;
    uint32_t w = 0, h = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t fence[8] = {};
    bool fence_set[8] = {};
    float *accum_own = nullptr, *accum = nullptr;
    uint32_t *offsets = nullptr;
    unsigned long long *counters = nullptr;
    unsigned char *blob = nullptr;
    unsigned char *tex_mem = nullptr;   // uv | ids | table | texels (trg_load_textures)
    trg::TexDesc tex{};
    // global overflow levels of the traversal stacks (grow-only), one buffer per launch the caller keeps in flight
    // (TRG_OPT_LAUNCHES_IN_FLIGHT): launch k uses slot k mod in_flight, so overlapping launches never share one
    static constexpr int kScratchSlots = 16;
    hipStream_t slot_stream[kScratchSlots] = {};   // which stream owns scratch slot k (slot 0 = the context's own stream)
    int slots_used = 1;
    int *stack_scratch[kScratchSlots] = {};
    size_t stack_scratch_bytes[kScratchSlots] = {};
    // wavefront schedule: path state + ray queues of one batch, one set per launch in flight (grow-only)
    unsigned char *wf_mem[kScratchSlots] = {};
    size_t wf_bytes[kScratchSlots] = {};
    int cu_count = 256;
    uint32_t *xq = nullptr;   // kScratchSlots x 8 job-queue heads of the persistent regeneration launches (TRG_OPT_TILE_ORDER 64 + n), one set per stream
    uint32_t bvh_depth4 = 0, bvh_nodes4 = 0;
    trg::SceneDesc sc{};
    bool scene_loaded = false, have_uniforms = false, have_offsets = false;
    trg_uniforms u{};
    bool opt_strict = false, opt_counters = false, opt_force_global = false, opt_timing = true;
    int opt_kernel = TRG_KERNEL_AUTO;
    uint32_t last_kernel = TRG_KERNEL_DIRECT;
    uint32_t last_tail_k = 0;
    int opt_gpu_build = 0;   // TRG_OPT_GPU_BUILD: 0 host SAH, 1 device binned SAH, 2 device LBVH (Karras), 3 device PLOC
    int opt_fsplit = 0;  // 0 = auto
    int opt_tail = -1;   // TRG_OPT_TAIL_BOUNCE: -1 auto, 0 off, K
    int opt_regen = -1;        // TRG_OPT_REGEN: 1 = path regeneration for HBM-resident scenes (direct kernel, frame-serial), -1 = from 32,768 triangles on, 0 = the lock-step kernel
    uint32_t last_regen = 0;
    int opt_tail_levels = 0;   // TRG_OPT_TAIL_LEVELS: 0 = re-compact every second bounce after K, 1 = once at K only
    int opt_in_flight = 1;  // launches of this context the caller keeps in flight (TRG_OPT_LAUNCHES_IN_FLIGHT)
    int opt_stack_levels = (int)TRG_STACK_LDS_LEVELS;   // TRG_OPT_STACK_LDS_LEVELS
    int opt_tail_sort = 0;     // TRG_OPT_TAIL_SORT: 0 off, 1 direction octant, 2 / 3 octant + origin cell of a 2^3 / 4^3 grid
    int opt_tail_refill = -1;  // TRG_OPT_TAIL_REFILL: 1 = the tail launches run ONE bounce each with in-wave refill (render_rtail_kernel); -1 = the library's choice
    float scene_lo[3] = { 0.f, 0.f, 0.f }, scene_hi[3] = { 1.f, 1.f, 1.f };   // bounds of the loaded scene (tail sort: the origin grid)
    int opt_tile_order = -1;   // TRG_OPT_TILE_ORDER: -1 auto, 0 image columns centre-out, 1 / 2 / 4 / 8 XCD regions with that many column strips
    uint32_t last_xcd_cols = 0;
    double last_build_ms = 0.0;
    bool gpu_built = false;
    uint32_t bvh_nodes = 0, bvh_depth = 0, bvh_leaves = 0, bvh_quads = 0, bvh_boxes = 0;
    uint32_t bvh_room = 0, bvh_walk_depth = 0;   // the room of an LDS-resident scene: its faces (0 = none), and the depth of the part the shipped build walks behind it
    float room_center[3] = { 0.f, 0.f, 0.f }, room_axis[3][3] = {};   // its frame: l_k = room_axis[k] . (P - room_center), the room is |l_k| <= 1 (render_impl: is the light inside?)
    double last_ms = 0.0, total_ms = 0.0;
    uint32_t renders = 0;
    uint32_t last_fsplit = 1;
    uint32_t launches = 0;   // trg_render launches since create (never reset: picks the scratch slot)
    std::string err;
    // what the denoiser and the refit unit keep for this context (created on first use; trg_destroy frees them: trg_internal.h)
    trg::DenoiseState *denoise = nullptr;
    trg::RefitState *refit = nullptr;
};
