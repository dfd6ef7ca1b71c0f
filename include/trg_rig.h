/* trg_rig.h -- animate a loaded scene on the device: a keyframed joint forest makes the bones, and the bones never leave the device.
 *
 * trg_skin_apply and trg_morph_apply (trg_skin.h, trg_morph.h) take 48 bytes per bone from the host on every call, and before that the caller has
 * sampled keyframes, composed every joint with its parent and multiplied by the inverse bind matrix on the CPU.  What changes per call is a time.
 * A RIG is bound once -- the joint forest, its keyframed translation / rotation / scale tracks, its inverse bind matrices -- and evaluated on the
 * device into bone matrices that feed the skin and morph bindings where they are.  Per call: one float per CLOCK (one clock is one character's
 * time; a crowd of a thousand characters is 4 KB).  A unit of its own beside the render path (include/trg.h names none of it).
 *
 *  bind      n_joints joints; joint j is bone j.  parent[j] is 0xFFFFFFFF (a root; several are legal) or < j.  Joint j's keys are the records
 *            key_first[j] .. key_first[j + 1] - 1 of keys12, 12 floats each: { time, Tx, Ty, Tz | Rx, Ry, Rz, Rw | Sx, Sy, Sz, 0 }; at least one
 *            per joint, times strictly ascending within a joint.  clock_of[j] < n_clocks.  inv_bind12: n_joints x 12 floats, row-major [A | t], or
 *            NULL: the bone is then the joint's world matrix.  Checked on the host, in this order, the first offender named in trg_last_error
 *            (TRG_ERR_INVALID): counts non-zero and no null table; the parent rule; the key table (begins at 0, strictly ascending, ends at
 *            n_keys); times finite and ascending; T and S finite; rotations finite with | len^2 - 1 | <= 1e-3, the length formed in double;
 *            clock_of in range; inv_bind finite.  Last: a forest deeper than TRG_RIG_MAX_LEVELS is TRG_ERR_RANGE.  A bind refused by one
 *            of these checks leaves an earlier rig as it was (one that fails later, allocating or copying -- TRG_ERR_NOMEM, TRG_ERR_DEVICE --,
 *            leaves NO rig bound).  A rig holds no geometry and is independent of the loaded scene: it SURVIVES trg_load_scene.
 *  evaluate  n_clocks floats on the host, finite (else TRG_ERR_INVALID, nothing enqueued).  One kernel launch per level of the forest on the
 *            context's stream -- at most TRG_RIG_MAX_LEVELS --, one thread per joint: sample, local matrix, compose with the parent's world, which
 *            the launch before wrote, compose with the inverse bind.  The call does not wait.  World and bone matrices stay on the device.
 *  read / buffers   of the last evaluation: n_joints x 12 floats each to the host (either may be NULL; waits; refused before the first
 *            evaluation) / their device addresses, 16-byte aligned, valid from bind until the next bind or release, their contents
 *            undefined until the first evaluation.
 *  skin_apply / morph_apply   evaluate, then the context's skin (morph) binding is applied from the rig's bones: a device-to-device copy on the
 *            stream takes the place of trg_skin_apply's upload, everything after it is trg_skin_apply (trg_morph_apply): same kernel, same refit,
 *            same rotation of the copies, same refusals.  The rig needs as many joints as the binding has bones; a morph binding needs bones.
 *  skin_apply_device / morph_apply_device   the same from bones the CALLER holds in device memory (torch, a physics step): n_bones x 12 floats
 *            on the context's device, any alignment, copied on the stream.  No rig is needed.  The pointer is checked against the device
 *            runtime's records as trg_refit_scene_device's are (memory of this device, inside one allocation; the SIZE half of that check is best
 *            effort: a sub-allocating pool vouches for its whole block); a pointer that fails is refused with nothing enqueued.  The copy is
 *            ordered on the CONTEXT's stream only: whatever stream of the caller's wrote the bones must have finished before the call.
 *  group     every context of the group binds / applies its own copy; the first failure is returned.
 *
 * A BONE THAT IS NOT FINITE cannot be refused on the host any more -- the host never sees it.  It is caught where every coordinate that is not
 * finite already is: by the refit's bounds pass (a scene of the LDS tier: the rebuild's host check) before anything of the scene is written,
 * TRG_ERR_INVALID.  As after every refused apply, the scene, the current and the previous pose are then bit for bit what they were.
 *
 * The arithmetic, operation by operation, is toyraygun_amd/csrc/trg_rig_math.h: normalised lerp on the short path for rotations, lerp for
 * translation and scale, clamped outside a track.  Host, device and a numpy float32 restatement agree bit for bit.
 *
 * Out of scope: spherical interpolation (sinf and acosf are not correctly rounded on either side: its bits could not be pinned); cubic or step
 * keys; blending of clips; inverse kinematics; forests deeper than 64 levels; the 8-wide experiments build, which refuses these calls.
 */
#ifndef TRG_RIG_H
#define TRG_RIG_H

#include "trg_morph.h"
#include "trg_skin.h"

#define TRG_RIG_MAX_LEVELS 64

#ifdef __cplusplus
extern "C" {
#endif

TRG_API int trg_rig_bind(trg_ctx *ctx, const uint32_t *parent, uint32_t n_joints, const uint32_t *key_first, const float *keys12, uint32_t n_keys,
                         const uint32_t *clock_of, uint32_t n_clocks, const float *inv_bind12);
TRG_API int trg_rig_evaluate(trg_ctx *ctx, const float *clocks);
/* world and bone matrices of the last evaluation, n_joints x 12 floats each; either may be NULL; waits */
TRG_API int trg_rig_read(trg_ctx *ctx, float *bones12_host, float *world12_host);
/* their device addresses; either out pointer may be NULL.  Valid from bind on; the contents are undefined until the first evaluation */
TRG_API int trg_rig_buffers(trg_ctx *ctx, void **bones_dev, void **world_dev);
/* frees the rig only (trg_refit_release and trg_destroy free it too) */
TRG_API int trg_rig_release(trg_ctx *ctx);
TRG_API int trg_rig_skin_apply(trg_ctx *ctx, const float *clocks);
TRG_API int trg_rig_morph_apply(trg_ctx *ctx, const float *target_weights, const float *clocks);
TRG_API int trg_rig_skin_apply_device(trg_ctx *ctx, const void *bones12_dev);
TRG_API int trg_rig_morph_apply_device(trg_ctx *ctx, const float *target_weights, const void *bones12_dev);
TRG_API int trg_group_rig_bind(trg_group *g, const uint32_t *parent, uint32_t n_joints, const uint32_t *key_first, const float *keys12, uint32_t n_keys,
                               const uint32_t *clock_of, uint32_t n_clocks, const float *inv_bind12);
TRG_API int trg_group_rig_skin_apply(trg_group *g, const float *clocks);
TRG_API int trg_group_rig_morph_apply(trg_group *g, const float *target_weights, const float *clocks);

#ifdef __cplusplus
}
#endif
#endif /* TRG_RIG_H */
