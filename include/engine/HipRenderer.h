// engine/HipRenderer.h -- the MI355X backend: a toyraygun::Renderer whose loadScene/renderFrame drive the
// gfx950 megakernel through the C ABI of include/trg.h.  Takes the place of MetalRenderer
// (reference src/engine/Metal/MetalRenderer.h:16-29, MetalRenderer.mm:557-597) / D3D12Renderer.
#pragma once
#include <stdint.h>

#include <vector>

#include "engine/Renderer.h"

struct trg_ctx;
struct trg_group;

namespace toyraygun {

class HipRenderer : public Renderer {
public:
    HipRenderer();
    ~HipRenderer() override;

    bool init() override;                   // creates the device context; false (+message on stdout) on failure
    void destroy() override;
    void loadScene(Scene *scene) override;  // uploads the five Scene vectors, builds the BVH
    // The same scene with its geometry MOVED: uploads like loadScene.  In temporal mode (setDenoise), when the triangle count is the one of the
    // scene uploaded last (and neither scene has textures), the history is KEPT: the vectors uploaded last are handed to
    // trg_temporal_set_previous_scene (include/trg_denoise.h) -- triangle k of `scene` is the surface triangle k was -- and the next step looks
    // for every pixel's history where its surface was.  In every other case it is loadScene.
    void updateScene(Scene *scene);
    // Off by default.  On: updateScene REFITS the loaded scene (trg_refit_scene, include/trg_refit.h) where it called loadScene, when the triangle
    // count is the one of the scene uploaded last: the tree keeps its shape, the records, box frames and node boxes follow the vertices, colours,
    // material ids and textures stay.  A refit the library refuses (a quad or a box of the loaded tree that the moved vertices no longer form) falls
    // back to loadScene and says so on stdout.  The temporal hand-over above is the same either way.
    void setRefit(bool on) { m_refit = on; }
    bool getRefit() const { return m_refit; }
    unsigned int getRefitCount() const { return m_refits; }    // updateScene calls that were served by a refit
    // Poses (include/trg_pose.h): the loaded scene as OBJECTS that move by a matrix each, without a new Scene and without an upload of vertices.
    // bindObjects, after loadScene of the same `scene`: object j is triangles [firstTri[j], firstTri[j + 1]) -- nObjects + 1 entries, ascending from
    // 0 to the triangle count; no vertex may belong to two objects.  poseObjects: nObjects x 12 floats, row-major [A | t] per object, applied to the
    // geometry AS BOUND (not to the last pose); the loaded tree is refitted on the device.  In temporal mode on one device the pose before this one
    // is handed to trg_temporal_set_previous_scene_device from the pose unit's own buffers: the history follows without a host copy.  A pose the
    // library refuses (no binding, a loadScene since, a quad or a box of the loaded tree that the posed vertices no longer form) says so on stdout
    // and changes nothing.  Both return false when refused.
    bool bindObjects(Scene *scene, const uint32_t *firstTri, unsigned int nObjects);
    bool poseObjects(const float *xforms12);
    unsigned int getPoseCount() const { return m_poses; }      // poseObjects calls that succeeded
    // Skinning (include/trg_skin.h): the loaded scene as a mesh that BENDS -- every vertex follows a blend of up to four bone matrices.  bindSkin,
    // after loadScene of the same `scene`: per vertex four bone ids (< nBones) and four weights (>= 0, summing to 1; they are not normalised here).
    // poseSkin: nBones x 12 floats, row-major [A | t] per bone, applied to the geometry AS BOUND; the loaded tree is refitted on the device.  In
    // temporal mode on one device the pose before this one goes to trg_temporal_set_previous_scene_device from the skin unit's own buffers.  A call
    // the library refuses says so on stdout, changes nothing and arms nothing.  Both return false when refused.
    bool bindSkin(Scene *scene, const uint32_t *boneIds4, const float *weights4, unsigned int nBones);
    bool poseSkin(const float *bones12);
    unsigned int getSkinCount() const { return m_skins; }      // poseSkin calls that succeeded
    // Blend shapes (include/trg_morph.h), in front of an optional skin.  bindMorph, after loadScene of the same `scene`: target k owns the entries
    // [targetFirst[k], targetFirst[k + 1]), each a vertex, a position delta and -- entryDnrm3 may be null -- a normal delta; boneIds4, boneWeights4
    // and nBones as bindSkin takes them, or null, null, 0.  poseMorph: nTargets weights and (exactly when bones were bound) nBones x 12 floats,
    // applied to the geometry AS BOUND -- morph first, then skin; the loaded tree is refitted on the device.  In temporal mode on one device the
    // pose before this one goes to trg_temporal_set_previous_scene_device from the morph unit's own buffers.  A call the library refuses says so
    // on stdout, changes nothing and arms nothing.  Both return false when refused.
    bool bindMorph(Scene *scene, unsigned int nTargets, const uint32_t *targetFirst, const uint32_t *entryVertex, const float *entryDpos3,
                   const float *entryDnrm3, const uint32_t *boneIds4, const float *boneWeights4, unsigned int nBones);
    bool poseMorph(const float *targetWeights, const float *bones12);
    unsigned int getMorphCount() const { return m_morphs; }    // poseMorph calls that succeeded
    // Rigs (include/trg_rig.h): the bones themselves made on the device, from a keyframed joint forest.  bindRig, any time after create (a rig holds
    // no geometry and survives loadScene): joint j is bone j; parent[j] is 0xFFFFFFFF or < j; joint j's keys are the 12-float records
    // [keyFirst[j], keyFirst[j + 1]) of keys12, {time, T | R | S, 0}; clockOf[j] < nClocks; invBind12 nJoints x 12 floats or null.  animateSkin:
    // nClocks floats -- the rig is evaluated and the skin binding (bindSkin, as many bones as the rig has joints) is applied from its bones, which
    // never leave the device.  animateMorph: the same for the morph binding (bound with bones), with its target weights.  The temporal hand-over
    // is poseSkin's and poseMorph's.  A call the library refuses says so on stdout, changes nothing and arms nothing.  All return false when refused.
    bool bindRig(const uint32_t *parent, unsigned int nJoints, const uint32_t *keyFirst, const float *keys12, const uint32_t *clockOf, unsigned int nClocks,
                 const float *invBind12);
    bool animateSkin(const float *clocks);
    bool animateMorph(const float *targetWeights, const float *clocks);
    unsigned int getRigCount() const { return m_rigs; }        // animateSkin and animateMorph calls that succeeded
    // One more sample per pixel into the running average.  ASYNCHRONOUS like the reference's (MetalRenderer.mm:373-552: encode,
    // commit, return; three frames in flight behind a semaphore, :33,377,385-387): the call never waits for the GPU to finish
    // a frame.  It takes a snapshot of the uniforms and either launches at once (GPU idle) or -- while earlier launches are
    // still running -- lets consecutive frames with identical uniforms ride in ONE later launch (the megakernel renders any
    // number of frames per launch, bit for bit what one launch per frame gives).  At most kFramesInFlight launches are queued
    // on the device; only readAccumulation / savePNG / getRayCount / destroy wait for it.
    void renderFrame() override;

    // ---- beyond the reference: several GPUs of one node.  Call before init(): the frame is then sharded by row bands over the
    //      devices (trg_group_*, include/trg.h) and gathered on the first one, which presents / reads back / writes the PNG.
    //      One device is a group of one (the same calls, nothing to exchange).
    bool setDevices(const int *devices, int count);
    int getDeviceCount() const { return m_deviceCount; }

    // ---- the acceleration structure: the reference rebuilds it on the GPU at loadScene (MPSTriangleAccelerationStructure rebuild,
    //      MetalRenderer.mm:272-279).  0 (default): the host's binned-SAH builder; 1: the same split rule on the device, level by
    //      level (a million triangles in ~20 ms); 2: Karras LBVH; 3: PLOC (TRG_OPT_GPU_BUILD, include/trg.h).  Scenes small enough
    //      to be staged in LDS are always built on the host.  Takes effect at the next loadScene().
    bool setDeviceBuild(int builder);
    int getDeviceBuild() const { return m_deviceBuild; }

    // ---- beyond the reference: batch rendering and read-back for headless use ----
    void setBounces(unsigned int bounces);              // reference hard-codes 3 (MetalRenderer.mm:426)
    unsigned int getBounces() const { return m_bounces; }
    void setOffsetSeed(uint32_t seed);                  // per-pixel Halton offset seed (default 0x5EED0001)
    bool renderFrames(unsigned int frames);             // `frames` samples in ONE kernel launch (asynchronous too)
    bool flush();                                       // launch whatever renderFrame() has queued; does not wait
    bool finish();                                      // flush, then wait until the device has finished every frame
    void setSynchronous(bool on);                       // true: every launch is timed with HIP events and waited for (getLastRenderMs)
    unsigned int getLaunchCount() const { return m_launches; }   // kernel launches so far (progressive loops coalesce frames)
    static const int kFramesInFlight = 3;               // MetalRenderer.mm:33 kMaxFramesInFlight
    bool readAccumulation(float *rgbaOut);              // width*height*4 floats, row 0 = scene bottom
    bool savePNG(const char *path);                     // ACES + sRGB (PostProcessing.metal:44-57), top row first
    // ---- denoising (include/trg_denoise.h).  0 (default): off, nothing changes.  1..6: the image handed to post-processing (savePNG) is an
    //      edge-avoiding a-trous filtered COPY of the accumulation buffer, guided by the first hits of frame 0 under the current camera; the
    //      accumulation itself goes on undisturbed.  One device only: a device group ignores it.
    //      varianceGuided: savePNG instead renders the frames so far AGAIN as two independent halves (trg_render_denoised_variance; one more
    //      frame when their number is odd, and it says so) and filters their mean, guided by the halves' difference; the accumulation buffer is
    //      not touched, the ray count includes the second rendering.
    //      temporal (not together with varianceGuided; one device only -- false with a device group or after setDevices()): every renderFrame() / renderFrames() batch is a step of
    //      trg_render_temporal_own -- rendered into an image of the denoise state, blended with the history reprojected from the previous
    //      batches' camera, filtered with the temporal variance -- and savePNG writes the last step's output.  The accumulation buffer is not
    //      written in this mode (readAccumulation returns what it held before), batches are never coalesced, and loadScene() forgets the history.
    bool setDenoise(int iterations, bool varianceGuided = false, bool temporal = false);
    int getDenoise() const { return m_denoise; }
    bool getDenoiseVarianceGuided() const { return m_denoiseVar; }
    bool getDenoiseTemporal() const { return m_denoiseTemporal; }
    // ---- changing light (trg_temporal_set_lag_correction): gate >= 0 switches the gated lag correction of the temporal steps on (3 is the
    //      library's suggestion, TRG_TEMPORAL_LAG_GATE_DEFAULT), a negative gate off (the default).  Effective in temporal mode on one device;
    //      it may be set before init() and survives loadScene.  False for a NaN, or when the library refuses.
    bool setLagCorrection(float gate);
    float getLagCorrection() const { return m_lagGate; }
    // ---- a long history (trg_temporal_set_variance_of_mean): the temporal steps carry the variance of the ACCUMULATED colour through the
    //      history and hand that to the filter, which narrows as the history grows.  Off by default.  Effective in temporal mode on one device;
    //      it may be set before init() and survives loadScene.  A change forgets the temporal history.  False when the library refuses.
    bool setVarianceOfMean(bool on);
    bool getVarianceOfMean() const { return m_varianceOfMean; }
    // ---- pixel footprints (trg_temporal_set_coverage): the temporal steps take their guides from the pixel centres, accumulate how often the
    //      frame's jittered ray agrees with them, and keep a pixel whose agreement is below covMin out of the filter (it shows its accumulated
    //      colour).  0 <= covMin < 1: on; < 0: off, the default.  Effective in temporal mode on one device; it may be set before init() and
    //      survives loadScene.  A change forgets the temporal history.  False for a NaN or covMin >= 1, or when the library refuses.
    bool setCoverage(float covMin);
    float getCoverage() const { return m_coverageMin; }
    int getFrameIndex() const { return m_frameIndex; }
    double getLastRenderMs() const;
    uint64_t getRayCount() const;                       // primary + bounce + shadow rays traced so far
    const char *getLastError() const;
    trg_ctx *context() { return m_ctx; }
    void fillUniforms(Uniforms *out);                   // MetalRenderer.mm:340-371 updateUniforms

protected:
    trg_ctx *m_ctx;              // the context (of the first device when a group is used)
    trg_group *m_group;          // non-null when rendering on several devices
    int m_devices[16];
    int m_deviceCount;
    unsigned int m_bounces;
    int m_deviceBuild;
    uint32_t m_offsetSeed;
    bool m_sceneLoaded;
    bool m_synchronous;
    unsigned int m_pending;      // frames renderFrame() has accepted but not launched yet
    int m_pendingFirst;          // frame index of the first of them
    Uniforms m_pendingUniforms;  // their uniforms (frameIndex zeroed)
    unsigned int m_launches;
    int m_denoise;               // a-trous iterations of the image handed to post-processing; 0 = off
    bool m_denoiseVar;           // ... by the variance-guided filter from two half-sample buffers
    bool m_denoiseTemporal;      // ... or every batch a temporal step (trg_render_temporal_own)
    void *m_temporalOut;         // the last temporal step's output image (owned by the denoise state); null before the first
    float m_lagGate;             // the gate of the lag correction of the temporal steps; < 0 = off
    bool m_varianceOfMean;       // the temporal steps track the variance of the accumulated colour
    float m_coverageMin;         // cov_min of the coverage history of the temporal steps; < 0 = off
    // updateScene: the positions, normals and indices uploaded last (temporal mode, one device; else empty), whether they came with textures,
    // and whether the loadScene in progress keeps the temporal history
    std::vector<float> m_lastPositions, m_lastNormals;
    std::vector<uint32_t> m_lastIndices;
    bool m_lastTextured;
    bool m_keepHistory;
    // setRefit; whether the loadScene in progress may refit; the triangle count uploaded last; refits done
    bool m_refit = false, m_refitNow = false;
    size_t m_loadedTris = 0;
    unsigned int m_refits = 0;
    unsigned int m_poses = 0;    // poses applied
    uint32_t m_poseVerts = 0;    // the vertex count bound by bindObjects
    unsigned int m_skins = 0;    // skins applied
    uint32_t m_skinVerts = 0;    // the vertex count bound by bindSkin
    unsigned int m_morphs = 0;   // morphs applied
    uint32_t m_morphVerts = 0;   // the vertex count bound by bindMorph
    unsigned int m_rigs = 0;     // rigs applied
    void afterPose(int (*buffers)(trg_ctx *, void **, void **, void **, void **, void **), uint32_t nVerts);   // the history follows an apply
};

}  // namespace toyraygun
