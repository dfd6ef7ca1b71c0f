// HipRenderer.cpp -- toyraygun::Renderer backend for MI355X (see include/engine/HipRenderer.h).
// Everything that touches the GPU goes through the C ABI of include/trg.h.
#include "engine/HipRenderer.h"

#include <stdio.h>
#include <string.h>

#include <vector>

#include "png_writer.h"
#include "trg.h"
#include "trg_denoise.h"
#include "trg_morph.h"
#include "trg_pose.h"
#include "trg_rig.h"
#include "trg_skin.h"
#include "trg_refit.h"

namespace toyraygun {

HipRenderer::HipRenderer()
    : m_ctx(nullptr), m_group(nullptr), m_deviceCount(0), m_bounces(3), m_deviceBuild(0), m_offsetSeed(0x5EED0001u), m_sceneLoaded(false), m_synchronous(false), m_pending(0), m_pendingFirst(0),
      m_launches(0), m_denoise(0), m_denoiseVar(false), m_denoiseTemporal(false), m_temporalOut(nullptr), m_lagGate(-1.0f), m_varianceOfMean(false), m_coverageMin(-1.0f), m_lastTextured(false), m_keepHistory(false) {
    memset(&m_pendingUniforms, 0, sizeof(m_pendingUniforms));
}
HipRenderer::~HipRenderer() { destroy(); }

bool HipRenderer::setDevices(const int *devices, int count) {
    if (m_ctx || !devices || count < 1 || count > 16) return false;   // before init() only
    for (int i = 0; i < count; ++i) m_devices[i] = devices[i];
    m_deviceCount = count;
    return true;
}

bool HipRenderer::init() {
    Renderer::init();  // width/height/aspect from the Engine (Renderer.cpp:18-27)
    destroy();
    if (m_deviceCount >= 1) {   // setDevices() was called: a device group, also for one device (same calls, nothing to exchange)
        const int rc = trg_group_create(&m_group, m_devices, m_deviceCount, (uint32_t)m_width, (uint32_t)m_height);
        if (rc != TRG_OK) {
            printf("HipRenderer: %s\n", trg_group_last_error(nullptr));
            m_group = nullptr;
            return false;
        }
        m_ctx = trg_group_ctx(m_group, 0);
        if (trg_group_set_pixel_offsets_seed(m_group, m_offsetSeed) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_group_last_error(m_group));
            return false;
        }
    } else {
        const int dev = Engine::instance()->getDevice();
        const int rc = trg_create(&m_ctx, dev, (uint32_t)m_width, (uint32_t)m_height);
        if (rc != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(nullptr));
            m_ctx = nullptr;
            return false;
        }
        // the reference creates the random-offset texture in resize() (MetalRenderer.mm:323-335)
        if (trg_set_pixel_offsets_seed(m_ctx, m_offsetSeed) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(m_ctx));
            return false;
        }
        // (the setting lives in the context's denoise state, which destroy() released)
        if (m_lagGate >= 0.0f && trg_temporal_set_lag_correction(m_ctx, m_lagGate) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(m_ctx));
            return false;
        }
        if (m_varianceOfMean && trg_temporal_set_variance_of_mean(m_ctx, 1) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(m_ctx));
            return false;
        }
        if (m_coverageMin >= 0.0f && trg_temporal_set_coverage(m_ctx, m_coverageMin) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(m_ctx));
            return false;
        }
    }
    m_frameIndex = 0;  // MetalRenderer.mm:337
    m_sceneLoaded = false;
    m_pending = 0; m_launches = 0;
    // asynchronous launches: nothing waits per frame
    if (m_group) trg_group_set_option(m_group, TRG_OPT_TIMING, m_synchronous ? 1 : 0);
    else trg_set_option(m_ctx, TRG_OPT_TIMING, m_synchronous ? 1 : 0);
    return true;
}

void HipRenderer::destroy() {
    if (m_ctx) flush();
    if (m_group) trg_group_destroy(m_group);   // owns every context, m_ctx included
    else if (m_ctx) trg_destroy(m_ctx);
    m_group = nullptr;
    m_ctx = nullptr;
    m_sceneLoaded = false;
    m_temporalOut = nullptr;   // (it pointed into the denoise state)
}

void HipRenderer::loadScene(Scene *scene) {
    if (!m_ctx || !scene) return;
    flush();   // frames queued for the old scene are rendered with it
    static_assert(sizeof(bx::Vec3) == 12, "bx::Vec3 must be 3 packed floats");
    const uint32_t nTris = (uint32_t)scene->m_materialIDBuffer.size();
    const uint32_t nVerts = (uint32_t)scene->m_vertexBuffer.size();
    const float *pos = nVerts ? &scene->m_vertexBuffer[0].x : nullptr;
    const float *nrm = nVerts ? &scene->m_normalBuffer[0].x : nullptr;
    const float *col = nVerts ? &scene->m_colorBuffer[0].x : nullptr;
    const uint32_t *idx = nVerts ? &scene->m_indexBuffer[0] : nullptr;
    const uint32_t *mat = nTris ? &scene->m_materialIDBuffer[0] : nullptr;
    // a device-built tree is traversed in HBM: scenes of a few hundred triangles are staged in LDS and keep the host builder
    const int builder = nTris >= 1024u ? m_deviceBuild : 0;
    // updateScene with setRefit(true): the loaded tree follows the vertices; what the library refuses is loaded instead
    bool refitted = false;
    if (m_refitNow) {
        const int rrc = m_group ? trg_group_refit_scene(m_group, pos, nrm, idx, nVerts, nTris) : trg_refit_scene(m_ctx, pos, nrm, idx, nVerts, nTris);
        refitted = rrc == TRG_OK;
        if (refitted) ++m_refits;
        else { printf("HipRenderer: refit refused (%s); loading the scene\n", trg_last_error(m_ctx)); fflush(stdout); }
    }
    if (!refitted) {
        if (m_group) trg_group_set_option(m_group, TRG_OPT_GPU_BUILD, builder);
        else trg_set_option(m_ctx, TRG_OPT_GPU_BUILD, builder);
    }
    const int rc = refitted ? TRG_OK
                 : m_group  ? trg_group_load_scene(m_group, pos, nrm, col, idx, mat, nVerts, nTris)
                            : trg_load_scene(m_ctx, pos, nrm, col, idx, mat, nVerts, nTris);
    if (rc != TRG_OK) {
        printf("HipRenderer: %s\n", m_group ? trg_group_last_error(m_group) : trg_last_error(m_ctx));
        m_sceneLoaded = false;
        return;
    }
    m_sceneLoaded = true;
    m_loadedTris = nTris;
    // the temporal history belongs to the old scene (the library does not notice a changed one) -- unless updateScene vouches for it
    if (m_denoiseTemporal && !m_keepHistory) {
        if (trg_temporal_reset(m_ctx) != TRG_OK) printf("HipRenderer: %s\n", trg_last_error(m_ctx));
        m_temporalOut = nullptr;
    }
    // what updateScene hands to trg_temporal_set_previous_scene when this geometry moves
    m_lastPositions.clear(); m_lastNormals.clear(); m_lastIndices.clear();
    m_lastTextured = !scene->m_textures.empty();
    if (m_denoiseTemporal && !m_group && nVerts) {
        m_lastPositions.assign(pos, pos + (size_t)nVerts * 3);
        m_lastNormals.assign(nrm, nrm + (size_t)nVerts * 3);
        m_lastIndices.assign(idx, idx + (size_t)nVerts);
    }
    // albedo textures of the scene (Scene::addMesh with a Texture): expanded to RGBA8 and uploaded with the texture coordinates
    if (!scene->m_textures.empty() && nTris && !refitted) {   // (a refitted scene keeps the textures it was loaded with)
        std::vector<float> uv(scene->m_uvBuffer);
        std::vector<uint32_t> ids(scene->m_textureIDBuffer);
        uv.resize((size_t)nVerts * 2, 0.0f);       // triangles added after the last textured mesh
        ids.resize(nTris, 0u);
        std::vector<std::vector<uint8_t> > rgba(scene->m_textures.size());
        std::vector<const uint8_t *> ptrs;
        std::vector<uint32_t> ws, hs;
        for (size_t k = 0; k < scene->m_textures.size(); ++k) {
            Texture *t = scene->m_textures[k];
            const int w = t->getWidth(), h = t->getHeight(), ch = t->getChannels();
            const uint8_t *src = t->getBufferPointer();
            rgba[k].resize((size_t)w * h * 4);
            for (size_t i = 0; i < (size_t)w * h; ++i) {
                const uint8_t *p = src + i * ch;
                uint8_t *q = &rgba[k][i * 4];
                if (ch >= 3) { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = ch == 4 ? p[3] : 255; }
                else { q[0] = q[1] = q[2] = p[0]; q[3] = ch == 2 ? p[1] : 255; }
            }
            ptrs.push_back(rgba[k].data()); ws.push_back((uint32_t)w); hs.push_back((uint32_t)h);
        }
        const int rc = m_group ? trg_group_load_textures(m_group, uv.data(), ids.data(), nTris, ptrs.data(), ws.data(), hs.data(), (uint32_t)ptrs.size())
                               : trg_load_textures(m_ctx, uv.data(), ids.data(), nTris, ptrs.data(), ws.data(), hs.data(), (uint32_t)ptrs.size());
        if (rc != TRG_OK) {
            printf("HipRenderer: %s\n", m_group ? trg_group_last_error(m_group) : trg_last_error(m_ctx));
            m_sceneLoaded = false;
            return;
        }
    }
}

void HipRenderer::updateScene(Scene *scene) {
    if (!m_ctx || !scene) return;
    const size_t nTris = scene->m_materialIDBuffer.size();
    const bool keep = m_denoiseTemporal && !m_group && m_sceneLoaded && nTris != 0 && m_lastIndices.size() == nTris * 3 && !m_lastTextured &&
                      scene->m_textures.empty();
    m_refitNow = m_refit && m_sceneLoaded && nTris != 0 && nTris == m_loadedTris;
    if (!keep) { loadScene(scene); m_refitNow = false; return; }
    std::vector<float> positions, normals;
    std::vector<uint32_t> indices;
    positions.swap(m_lastPositions); normals.swap(m_lastNormals); indices.swap(m_lastIndices);
    m_keepHistory = true;
    loadScene(scene);
    m_keepHistory = false;
    m_refitNow = false;
    if (!m_sceneLoaded) return;
    if (trg_temporal_set_previous_scene(m_ctx, positions.data(), normals.data(), indices.data(), (uint32_t)(positions.size() / 3), (uint32_t)nTris) != TRG_OK) {
        printf("HipRenderer: %s\n", trg_last_error(m_ctx));
        trg_temporal_reset(m_ctx);   // the history cannot be followed: start over, as loadScene does
        m_temporalOut = nullptr;
    }
}

// a pose call on the one context, or on every context of the group in turn (what trg_group_pose_* do, after the same wait) -- done here so that
// the text reported is that of the context which refused THIS call, not an older one another context still holds
template <typename Call>
static int poseEach(trg_group *group, trg_ctx *ctx, Call call, const char **text) {
    *text = "";
    if (!group) {
        const int rc = call(ctx);
        if (rc != TRG_OK) *text = trg_last_error(ctx);
        return rc;
    }
    int rc = trg_group_sync(group);
    if (rc != TRG_OK) { *text = trg_group_last_error(group); return rc; }
    for (int r = 0; r < trg_group_size(group); ++r) {
        trg_ctx *c = trg_group_ctx(group, r);
        if (!c) return TRG_ERR_INVALID;
        if ((rc = call(c)) != TRG_OK) { *text = trg_last_error(c); return rc; }
    }
    return TRG_OK;
}

// a Scene's arrays and counts as a bind takes them; false: there is nothing to bind
struct BindGeometry {
    const float *pos, *nrm;
    const uint32_t *idx;
    uint32_t nVerts, nTris;
};
static bool bindGeometry(Scene *scene, BindGeometry *g) {
    g->nTris = (uint32_t)scene->m_materialIDBuffer.size();
    g->nVerts = (uint32_t)scene->m_vertexBuffer.size();
    if (!g->nVerts || !g->nTris || scene->m_indexBuffer.size() != (size_t)g->nTris * 3) return false;
    // (a scene without a normal per corner is bound without normals: the loaded ones stay, and a morph's normal deltas are then refused)
    g->pos = &scene->m_vertexBuffer[0].x;
    g->nrm = scene->m_normalBuffer.size() == (size_t)g->nTris * 3 ? &scene->m_normalBuffer[0].x : nullptr;
    g->idx = &scene->m_indexBuffer[0];
    return true;
}

// after an apply of any unit that succeeded: `buffers` is the unit's trg_*_buffers, nVerts what its bind bound
void HipRenderer::afterPose(int (*buffers)(trg_ctx *, void **, void **, void **, void **, void **), uint32_t nVerts) {
    // (updateScene's remembered vectors are no longer what the device holds: its next call loads)
    m_lastPositions.clear(); m_lastNormals.clear(); m_lastIndices.clear();
    if (!m_denoiseTemporal || m_group) return;
    // what was current is the unit's PREVIOUS pose now, and stays untouched through the next apply: the history is told where every triangle was
    void *prevPos = nullptr, *prevNrm = nullptr, *idx = nullptr;
    if (buffers(m_ctx, nullptr, nullptr, &idx, &prevPos, &prevNrm) != TRG_OK ||
        trg_temporal_set_previous_scene_device(m_ctx, prevPos, prevNrm, idx, nVerts, (uint32_t)m_loadedTris) != TRG_OK) {
        printf("HipRenderer: %s\n", trg_last_error(m_ctx));
        trg_temporal_reset(m_ctx);   // the history cannot be followed: start over, as loadScene does
        m_temporalOut = nullptr;
    }
}

bool HipRenderer::bindObjects(Scene *scene, const uint32_t *firstTri, unsigned int nObjects) {
    if (!m_ctx || !scene || !m_sceneLoaded || !firstTri) return false;
    flush();
    BindGeometry g;
    if (!bindGeometry(scene, &g)) return false;
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_pose_bind(c, g.pos, g.nrm, g.idx, g.nVerts, g.nTris, firstTri, nObjects); }, &text);
    if (rc != TRG_OK) { printf("HipRenderer: objects not bound (%s)\n", text); fflush(stdout); }
    else m_poseVerts = g.nVerts;
    return rc == TRG_OK;
}

bool HipRenderer::poseObjects(const float *xforms12) {
    if (!m_ctx || !m_sceneLoaded || !xforms12) return false;
    flush();   // frames queued so far are rendered with the pose they were queued under
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_pose_apply(c, xforms12); }, &text);
    if (rc != TRG_OK) {
        printf("HipRenderer: pose refused (%s); nothing changed\n", text);
        fflush(stdout);
        return false;
    }
    ++m_poses;
    afterPose(trg_pose_buffers, m_poseVerts);
    return true;
}

bool HipRenderer::bindSkin(Scene *scene, const uint32_t *boneIds4, const float *weights4, unsigned int nBones) {
    if (!m_ctx || !scene || !m_sceneLoaded || !boneIds4 || !weights4) return false;
    flush();
    BindGeometry g;
    if (!bindGeometry(scene, &g)) return false;
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_skin_bind(c, g.pos, g.nrm, g.idx, g.nVerts, g.nTris, boneIds4, weights4, nBones); }, &text);
    if (rc != TRG_OK) { printf("HipRenderer: skin not bound (%s)\n", text); fflush(stdout); }
    else m_skinVerts = g.nVerts;
    return rc == TRG_OK;
}

bool HipRenderer::poseSkin(const float *bones12) {
    if (!m_ctx || !m_sceneLoaded || !bones12) return false;
    flush();   // frames queued so far are rendered with the pose they were queued under
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_skin_apply(c, bones12); }, &text);
    if (rc != TRG_OK) {
        printf("HipRenderer: skin refused (%s); nothing changed\n", text);
        fflush(stdout);
        return false;
    }
    ++m_skins;
    afterPose(trg_skin_buffers, m_skinVerts);
    return true;
}

bool HipRenderer::bindMorph(Scene *scene, unsigned int nTargets, const uint32_t *targetFirst, const uint32_t *entryVertex, const float *entryDpos3,
                            const float *entryDnrm3, const uint32_t *boneIds4, const float *boneWeights4, unsigned int nBones) {
    if (!m_ctx || !scene || !m_sceneLoaded || !nTargets || !targetFirst) return false;
    flush();
    BindGeometry g;
    if (!bindGeometry(scene, &g)) return false;
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) {
        return trg_morph_bind(c, g.pos, g.nrm, g.idx, g.nVerts, g.nTris, nTargets, targetFirst, targetFirst[nTargets], entryVertex, entryDpos3, entryDnrm3, boneIds4, boneWeights4, nBones);
    }, &text);
    if (rc != TRG_OK) { printf("HipRenderer: morph not bound (%s)\n", text); fflush(stdout); }
    else m_morphVerts = g.nVerts;
    return rc == TRG_OK;
}

bool HipRenderer::poseMorph(const float *targetWeights, const float *bones12) {
    if (!m_ctx || !m_sceneLoaded || !targetWeights) return false;
    flush();   // frames queued so far are rendered with the pose they were queued under
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_morph_apply(c, targetWeights, bones12); }, &text);
    if (rc != TRG_OK) {
        printf("HipRenderer: morph refused (%s); nothing changed\n", text);
        fflush(stdout);
        return false;
    }
    ++m_morphs;
    afterPose(trg_morph_buffers, m_morphVerts);
    return true;
}

bool HipRenderer::bindRig(const uint32_t *parent, unsigned int nJoints, const uint32_t *keyFirst, const float *keys12, const uint32_t *clockOf, unsigned int nClocks,
                          const float *invBind12) {
    if (!m_ctx || !parent || !keyFirst || !keys12 || !clockOf || !nJoints) return false;
    flush();
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_rig_bind(c, parent, nJoints, keyFirst, keys12, keyFirst[nJoints], clockOf, nClocks, invBind12); }, &text);
    if (rc != TRG_OK) { printf("HipRenderer: rig not bound (%s)\n", text); fflush(stdout); }
    return rc == TRG_OK;
}

bool HipRenderer::animateSkin(const float *clocks) {
    if (!m_ctx || !m_sceneLoaded || !clocks) return false;
    flush();   // frames queued so far are rendered with the pose they were queued under
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_rig_skin_apply(c, clocks); }, &text);
    if (rc != TRG_OK) {
        printf("HipRenderer: rig refused (%s); nothing changed\n", text);
        fflush(stdout);
        return false;
    }
    ++m_rigs;
    afterPose(trg_skin_buffers, m_skinVerts);
    return true;
}

bool HipRenderer::animateMorph(const float *targetWeights, const float *clocks) {
    if (!m_ctx || !m_sceneLoaded || !targetWeights || !clocks) return false;
    flush();   // frames queued so far are rendered with the pose they were queued under
    const char *text = "";
    const int rc = poseEach(m_group, m_ctx, [&](trg_ctx *c) { return trg_rig_morph_apply(c, targetWeights, clocks); }, &text);
    if (rc != TRG_OK) {
        printf("HipRenderer: rig refused (%s); nothing changed\n", text);
        fflush(stdout);
        return false;
    }
    ++m_rigs;
    afterPose(trg_morph_buffers, m_morphVerts);
    return true;
}

// MetalRenderer.mm:340-371: inverse view-projection, fixed ceiling light, frame index.
void HipRenderer::fillUniforms(Uniforms *u) {
    memset(u, 0, sizeof(*u));
    float viewProj[16], invViewProj[16];
    getViewProjMtx(viewProj);
    bx::mtxInverse(invViewProj, viewProj);
    u->camera.position.set(getCameraPosition());
    u->camera.invViewProjMtx.set(invViewProj);
    u->light.position.set(bx::Vec3(0.0f, 1.98f, 0.0f));
    u->light.forward.set(bx::Vec3(0.0f, -1.0f, 0.0f));
    u->light.right.set(bx::Vec3(0.25f, 0.0f, 0.0f));
    u->light.up.set(bx::Vec3(0.0f, 0.0f, 0.25f));
    u->light.color.set(bx::Vec3(1.0f, 1.0f, 1.0f));
    u->width = (unsigned int)m_width;
    u->height = (unsigned int)m_height;
    u->frameIndex = (unsigned int)m_frameIndex;
}

// Launch the queued frames [m_pendingFirst, m_pendingFirst + m_pending) in one megakernel launch.  A semaphore of
// kFramesInFlight launches (MetalRenderer.mm:377: dispatch_semaphore_wait before encoding) bounds what is queued on the device.
bool HipRenderer::flush() {
    if (!m_ctx || m_pending == 0) return true;
    const unsigned int frames = m_pending;
    m_pending = 0;
    if (!m_sceneLoaded) return false;
    static_assert(sizeof(Uniforms) == sizeof(trg_uniforms), "Uniforms / trg_uniforms layout mismatch");
    const int slot = (int)(m_launches % (unsigned int)kFramesInFlight);
    if (m_group) {   // row bands over the devices, gathered on the first one (which presents); the same bound on launches in flight
        if (trg_group_fence_wait(m_group, slot) != TRG_OK ||
            trg_group_set_uniforms(m_group, reinterpret_cast<const trg_uniforms *>(&m_pendingUniforms)) != TRG_OK ||
            trg_group_render(m_group, (uint32_t)m_pendingFirst, frames, m_bounces, TRG_GATHER_ROOT, 0) != TRG_OK ||
            trg_group_fence_record(m_group, slot) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_group_last_error(m_group));
            return false;
        }
        ++m_launches;
        return true;
    }
    if (m_denoiseTemporal) {
        // the batch as one temporal step: rendered into an image of the denoise state, reprojected history blended in, filtered; the
        // accumulation buffer is not touched
        trg_temporal_params tp;
        trg_temporal_default_params(&tp);
        tp.iterations = m_denoise;
        if (trg_fence_wait(m_ctx, slot) != TRG_OK ||
            trg_set_uniforms(m_ctx, reinterpret_cast<const trg_uniforms *>(&m_pendingUniforms)) != TRG_OK ||
            trg_render_temporal_own(m_ctx, (uint32_t)m_pendingFirst, frames, m_bounces, &tp, &m_temporalOut) != TRG_OK ||
            trg_fence_record(m_ctx, slot) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(m_ctx));
            return false;
        }
        ++m_launches;
        return true;
    }
    if (trg_fence_wait(m_ctx, slot) != TRG_OK ||
        trg_set_uniforms(m_ctx, reinterpret_cast<const trg_uniforms *>(&m_pendingUniforms)) != TRG_OK ||
        trg_render(m_ctx, (uint32_t)m_pendingFirst, frames, m_bounces, 0, (uint32_t)m_height) != TRG_OK ||
        trg_fence_record(m_ctx, slot) != TRG_OK) {
        printf("HipRenderer: %s\n", trg_last_error(m_ctx));
        return false;
    }
    ++m_launches;
    return true;
}

// Accept `frames` more frames with the CURRENT uniforms.  Frames whose uniforms differ from the queued ones cannot share a launch.
static bool sameUniforms(const Uniforms &a, const Uniforms &b) { return memcmp(&a, &b, sizeof(Uniforms)) == 0; }
bool HipRenderer::renderFrames(unsigned int frames) {
    if (!m_ctx || !m_sceneLoaded || frames == 0) return false;
    Uniforms u;
    fillUniforms(&u);
    u.frameIndex = 0;   // trg_render iterates its own frame range (uniforms->frameIndex = _frameIndex++, MetalRenderer.mm:363)
    if (m_pending && !sameUniforms(u, m_pendingUniforms) && !flush()) return false;
    if (m_pending == 0) { m_pendingUniforms = u; m_pendingFirst = m_frameIndex; }
    m_pending += frames;
    m_frameIndex += (int)frames;
    // launch now if the device has nothing to do (or we are asked to be synchronous, or a lot has piled up); otherwise the
    // frames wait for the next call and share its launch
    // (temporal mode: every call is a step of its own, whatever the device is doing -- how the frames are batched decides the picture)
    if (m_synchronous || m_denoiseTemporal || frames > 1 || m_pending >= 64u || trg_stream_idle(m_ctx) != 0) return flush();
    return true;
}

void HipRenderer::renderFrame() { renderFrames(1); }

void HipRenderer::setSynchronous(bool on) {
    flush();
    m_synchronous = on;
    if (m_group) trg_group_set_option(m_group, TRG_OPT_TIMING, on ? 1 : 0);
    else if (m_ctx) trg_set_option(m_ctx, TRG_OPT_TIMING, on ? 1 : 0);
}

void HipRenderer::setBounces(unsigned int bounces) { flush(); m_bounces = bounces; }
bool HipRenderer::setDeviceBuild(int builder) {
    if (builder < 0 || builder > 3) return false;
    m_deviceBuild = builder;
    return true;
}
bool HipRenderer::finish() { return m_ctx && flush() && (m_group ? trg_group_sync(m_group) : trg_sync(m_ctx)) == TRG_OK; }
void HipRenderer::setOffsetSeed(uint32_t seed) {
    flush();
    m_offsetSeed = seed;
    if (m_group) trg_group_set_pixel_offsets_seed(m_group, seed);
    else if (m_ctx) trg_set_pixel_offsets_seed(m_ctx, seed);
}
bool HipRenderer::readAccumulation(float *rgbaOut) {
    if (!m_ctx || !flush()) return false;
    if (m_group) return trg_group_read_accum(m_group, 0, rgbaOut) == TRG_OK;   // waits for the gather onto device 0 (and the unpack of interleaved bands)
    return trg_read_accum(m_ctx, rgbaOut) == TRG_OK;
}
bool HipRenderer::setDenoise(int iterations, bool varianceGuided, bool temporal) {
    if (iterations < 0 || iterations > TRG_DENOISE_MAX_ITERATIONS || (varianceGuided && temporal)) return false;
    const bool on = temporal && iterations > 0;
    if (on && (m_group || m_deviceCount >= 1)) return false;   // one device only: a device group (created, or asked for by setDevices) has no temporal mode
    if (on != m_denoiseTemporal) {
        flush();   // frames queued so far keep the mode they were queued in
        if (m_ctx && trg_temporal_reset(m_ctx) != TRG_OK) printf("HipRenderer: %s\n", trg_last_error(m_ctx));
        m_temporalOut = nullptr;
    }
    m_denoise = iterations;
    m_denoiseVar = varianceGuided && iterations > 0;
    m_denoiseTemporal = on;
    return true;
}
bool HipRenderer::setLagCorrection(float gate) {
    if (gate != gate) return false;
    if (m_ctx && !m_group) {
        flush();   // frames queued so far keep the setting they were queued under
        if (trg_temporal_set_lag_correction(m_ctx, gate) != TRG_OK) { printf("HipRenderer: %s\n", trg_last_error(m_ctx)); return false; }
    }
    m_lagGate = gate;
    return true;
}
bool HipRenderer::setVarianceOfMean(bool on) {
    if (m_ctx && !m_group) {
        flush();   // frames queued so far keep the setting they were queued under
        if (trg_temporal_set_variance_of_mean(m_ctx, on ? 1 : 0) != TRG_OK) { printf("HipRenderer: %s\n", trg_last_error(m_ctx)); return false; }
    }
    m_varianceOfMean = on;
    return true;
}
bool HipRenderer::setCoverage(float covMin) {
    if (!(covMin < 1.0f)) return false;   // (NaN too)
    if (m_ctx && !m_group) {
        flush();   // frames queued so far keep the setting they were queued under
        if (trg_temporal_set_coverage(m_ctx, covMin) != TRG_OK) { printf("HipRenderer: %s\n", trg_last_error(m_ctx)); return false; }
    }
    m_coverageMin = covMin;
    return true;
}
bool HipRenderer::savePNG(const char *path) {
    if (!m_ctx || !flush()) return false;
    std::vector<uint8_t> rgba((size_t)m_width * m_height * 4);
    if (m_denoise > 0 && !m_group) {
        // tone-map a denoised copy: filter the accumulation buffer into the denoise state's image, bind that image as the accumulation
        // buffer for the post-processing pass, and bind the renderer's own buffer back (everything on the context's one stream)
        trg_denoise_params dp;
        trg_denoise_default_params(&dp);
        dp.iterations = m_denoise;
        void *denoised = nullptr;
        int drc;
        if (m_denoiseTemporal) {
            // the last temporal step's output is the picture
            denoised = m_temporalOut;
            drc = denoised ? TRG_OK : TRG_ERR_INVALID;
            if (!denoised) { printf("HipRenderer: temporal denoising is on and no frame has been rendered\n"); return false; }
        } else if (m_denoiseVar) {
            // the frames so far once more, as two independent halves whose difference guides the filter (the uniforms are those of the last launch)
            unsigned int n = m_frameIndex > 0 ? (unsigned int)m_frameIndex : 2u;
            if (n & 1u) {
                printf("HipRenderer: the variance-guided denoiser needs an even sample count: rendering %u samples, not %u\n", n + 1u, n);
                ++n;
            }
            trg_denoise_var_params vp;
            trg_denoise_var_default_params(&vp);
            vp.iterations = m_denoise;
            drc = trg_render_denoised_variance_own(m_ctx, 0u, n, m_bounces, &vp, &denoised);
        } else {
            drc = trg_denoise_accum(m_ctx, 0u, &dp, &denoised);
        }
        if (drc != TRG_OK || trg_bind_accum(m_ctx, denoised) != TRG_OK) {
            printf("HipRenderer: %s\n", trg_last_error(m_ctx));
            return false;
        }
        const int rc = trg_postprocess(m_ctx, rgba.data(), 1);
        trg_bind_accum(m_ctx, nullptr);
        if (rc != TRG_OK) return false;
        return trg_host::write_png_rgba8(path, rgba.data(), m_width, m_height);
    }
    if ((m_group ? trg_group_postprocess(m_group, 0, rgba.data(), 1) : trg_postprocess(m_ctx, rgba.data(), 1)) != TRG_OK) return false;
    return trg_host::write_png_rgba8(path, rgba.data(), m_width, m_height);
}
double HipRenderer::getLastRenderMs() const {
    trg_stats st;
    return (m_ctx && trg_get_stats(m_ctx, &st) == TRG_OK) ? st.last_render_ms : 0.0;
}
uint64_t HipRenderer::getRayCount() const {
    const_cast<HipRenderer *>(this)->flush();
    trg_stats st;
    if (m_group) return trg_group_get_stats(m_group, &st) == TRG_OK ? st.primary_rays + st.bounce_rays + st.shadow_rays : 0;
    return (m_ctx && trg_get_stats(m_ctx, &st) == TRG_OK) ? st.primary_rays + st.bounce_rays + st.shadow_rays : 0;
}
const char *HipRenderer::getLastError() const { return trg_last_error(m_ctx); }

}  // namespace toyraygun
