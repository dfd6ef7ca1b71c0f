/* trg_refit.h -- refit a loaded scene from new vertex positions, on the device.
 *
 * What the interfaces this backend stands in for call `refit` (MPS) or an ALLOW_UPDATE build (DXR): the scene keeps its TOPOLOGY -- triangle k
 * stays triangle k, with its colours, its material id and its texture coordinates -- and its acceleration structure keeps its shape; everything
 * that depends on where the vertices are is derived again.  A unit of its own beside the render path (like trg_denoise.h): include/trg.h names
 * none of it.
 *
 * Two paths, reported by trg_refit_last:
 *
 *  TRG_REFIT_DEVICE   a scene traversed from HBM (every device-built scene, every host-built one too large for the LDS tier).  On the context's
 *                     stream: the new buffers are uploaded into grow-only scratch; the scene bounds, the centre and the builders' padding
 *                     max(2e-5 x extent, 4e-6 x max|coord|) are reduced exactly as trg_load_scene computes them; every input is checked --
 *                     indices in range, coordinates finite, every pair of triangles the loaded tree holds as a QUAD leaf still a parallelogram
 *                     by the builder's own rule, every BOX record still a parallelepiped to 1e-5 --; the per-node boxes are recomputed bottom-up
 *                     in ping-pong passes (no atomics on floats, no parent array) and quantised by the rule of the builders (power-of-two scale,
 *                     low planes rounded down, high planes up: a decoded box contains its float box) into scratch.  Then the host reads the
 *                     bounds and the flag words -- the call's ONE wait -- and only a scene that passed is written: the strict 128-byte records
 *                     (v0, e1, e2), the plane-form records (in double, relative to the new centre; the X record of a quad carries the
 *                     parallelogram), the nine normal floats of both when normals are given, the frames of the box records, and both node arrays
 *                     (child codes and unused slots do not change).  A refused call leaves the loaded scene bit for bit what it was.
 *  TRG_REFIT_REBUILD  a scene small enough for the LDS tier (about 170 triangles at most): microseconds of host build, and a rebuilt tree beats
 *                     a refitted one.  Colours and material ids are read back from the device.
 *
 * Loaded textures survive both paths.  The call is SYNCHRONOUS like trg_load_scene (it waits once, for the checks), and like it must not run
 * while a render of the same context is in flight on another stream.
 *
 * Out of scope: changed topology, colours or material ids (the caller reloads); refitting the LDS layouts in place; deciding for the caller when a
 * refitted tree has grown too loose -- trg_refit_info::area_ratio is there for that decision.
 */
#ifndef TRG_REFIT_H
#define TRG_REFIT_H

#include "trg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRG_REFIT_NONE 0u     /* no refit since the context was created (or since trg_refit_release) */
#define TRG_REFIT_DEVICE 1u
#define TRG_REFIT_REBUILD 2u

typedef struct trg_refit_info {
    uint32_t path;            /* TRG_REFIT_* of the last successful call */
    uint32_t n_records;       /* leaf records rewritten (both forms) */
    uint32_t n_quads;         /* quad leaves whose parallelogram was checked and re-derived */
    uint32_t n_boxes;         /* box records re-derived (parallelepipeds and lone quads dressed as boxes) */
    uint32_t n_nodes;         /* quantised 4-wide nodes rewritten, plain array */
    uint32_t n_nodes_box;     /* ... and box-leaf flavour (0: the scene has none) */
    uint32_t passes;          /* bottom-up passes over the node array */
    uint32_t reserved;
    float lo[3], hi[3];       /* bounds of the moved triangles */
    float pad;                /* the padding of every child box */
    float reserved_f;
    double ms;                /* host time of the call, its one wait included (the writes that follow it are enqueued, not waited for) */
    double area_ratio;        /* sum of the half areas of all decoded child boxes of the plain node array, over the same sum of the tree as loaded */
    double area_ratio_box;    /* the same for the box-leaf flavour (0: none) */
} trg_refit_info;

/* same topology as the loaded scene: triangle k stays triangle k; colours, material ids and textures stay.  normals3 (9 floats per triangle,
 * like trg_load_scene) may be NULL: the loaded normals stay.  n_tris must be the loaded scene's.  TRG_ERR_INVALID: bad arguments, an index out of
 * range, a non-finite coordinate, an 8-wide experiments build; TRG_ERR_RANGE: a quad leaf or a box record of the loaded tree that the moved
 * vertices no longer form.  trg_last_error names the first offending triangle. */
TRG_API int trg_refit_scene(trg_ctx *ctx, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris);
TRG_API int trg_refit_last(trg_ctx *ctx, trg_refit_info *out);
/* frees the unit's scratch of this context early (trg_destroy frees it too) */
TRG_API int trg_refit_release(trg_ctx *ctx);
/* every context of the group refits its own copy; the first failure is returned (trg_last_error of that context has the text) */
TRG_API int trg_group_refit_scene(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris);

#ifdef __cplusplus
}
#endif
#endif /* TRG_REFIT_H */
