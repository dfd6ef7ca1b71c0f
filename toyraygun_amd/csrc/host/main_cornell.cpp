// main_cornell.cpp -- headless demo following the reference app's call order (reference src/main.cpp:16-98):
// engine init -> three shaders -> renderer init -> camera -> Cornell box -> frame loop; then writes a PNG.
//   toyraygun_cornell [width height frames bounces out.png [denoise=N[,var|,temporal[,lag[=G]][,vmean][,cover[=C]]]] [orbit=DEG] [slide=D] [twist=DEG] [bulge=W] [bend=DEG] [refit|pose|skin|morph|rig]]
//     denoise=N    a-trous iterations of the written image, 0 = off (default)
//     ,var         the variance-guided filter from two half-sample buffers
//     ,temporal    the frames are rendered as `frames` calls of 1 spp, each a temporal step (reprojected history, temporal variance); the
//                  picture is the last step's
//     ,lag[=G]     (behind ,temporal) the gated lag correction of the accumulated colour at gate G (default 3): a moved shadow or a changed
//                  light no longer waits for the history to fade (HipRenderer::setLagCorrection)
//     ,vmean       (behind ,temporal, before or after ,lag) the steps track the variance of the ACCUMULATED colour and filter by that: the
//                  filter narrows as the history grows (HipRenderer::setVarianceOfMean)
//     ,cover[=C]   (behind ,temporal, in any order with the other two) guides from the pixel centres and a coverage history: a pixel whose footprint
//                  holds two surfaces (accumulated agreement below C, default 0.9, 0 <= C < 1) stays out of the filter (HipRenderer::setCoverage)
//     orbit=DEG    the eye turns about the look-at point (about the vertical axis) by DEG degrees per call
//     slide=D      before call k the box is rebuilt with the short box moved by k * D along x and handed to HipRenderer::updateScene: with
//                  ,temporal the history follows the moving box (trg_temporal_set_previous_scene), otherwise it is a plain loadScene
//     refit        (with slide=D) HipRenderer::setRefit(true): updateScene refits the loaded scene from the moved vertices (trg_refit_scene,
//                  include/trg_refit.h) instead of loading it again; the last line of output counts the refits
//     pose         (with slide=D, not with refit) the box is bound once with the short box as an object of its own (HipRenderer::bindObjects) and
//                  before call k the short box is moved by k * D through HipRenderer::poseObjects (include/trg_pose.h): 96 bytes go to the device,
//                  not a scene; with ,temporal the history follows from the pose unit's own buffers.  The last line of output counts the poses
//     skin         (with twist=DEG, not with refit or pose) the box is bound once with two bones (HipRenderer::bindSkin): bone 0 is the identity,
//                  bone 1 a rotation about the short box's vertical axis, and the short box's corners are weighted to bone 1 by their height within
//                  the box -- everything else has weight 1 on bone 0.  Before call k bone 1 turns by k * DEG degrees (HipRenderer::poseSkin,
//                  include/trg_skin.h): the box twists (twist=0, like slide=0 under pose, applies nothing).  The last line of output counts the skins applied
//     morph        (with bulge=W, optionally twist=DEG; not with refit, pose or skin) the box is bound once with one blend-shape target
//                  (HipRenderer::bindMorph): the copies of the short box's four top corners, each delta the corner's offset from the box's vertical
//                  axis -- and, with twist=DEG, with the two bones of the skin option behind it.  Before call k the target gets the weight k * W
//                  and bone 1 turns by k * DEG degrees (HipRenderer::poseMorph, include/trg_morph.h): the top of the box bulges, and twists.
//                  bulge=0 without a twist applies nothing.  The last line of output counts the morphs applied
//     rig          (with bend=DEG; not with refit, pose, skin or morph) the short box is bound to a chain of three joints up its vertical axis -- at
//                  its foot, half way up and at its top, each the child of the one below; a corner leans on joint k by max(0, 1 - |2 h - k|), h
//                  its height within the box -- and everything else to a fourth joint that rests (HipRenderer::bindSkin, four bones).  The clip
//                  (HipRenderer::bindRig, include/trg_rig.h) has two keys per chain joint: rest at time 0, and at time 1 every joint turned by
//                  DEG x (calls - 1) degrees about the x axis through its origin.  Before call k the clock is k / (calls - 1)
//                  (HipRenderer::animateSkin): 4 bytes go to the device and the box bends over.  bend=0 applies nothing.  Not with slide=D: a
//                  slid box is a reloaded scene, and the skin binding would be stale.  The last line of output
//                  counts the rigs applied
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <vector>

#include "cornellBox.h"
#include "engine/Engine.h"
#include "engine/HipRenderer.h"
#include "engine/Renderer.h"
#include "engine/Shader.h"
#include "trg_denoise.h"

using namespace toyraygun;

// the Cornell box (cornellBox.h) with the short box moved by dx along x
static Scene *createSlidCornellBox(float dx) {
    Scene *scene = new Scene();
    int n = 0;
    const toyraygun_scenes::Placement *p = toyraygun_scenes::cornellPlacements(&n);
    float m[16];
    for (int i = 0; i < n; ++i) {
        bx::mtxSRT(m, p[i].scale[0], p[i].scale[1], p[i].scale[2], p[i].rot[0], p[i].rot[1], p[i].rot[2], p[i].pos[0] + (i == 0 ? dx : 0.0f), p[i].pos[1], p[i].pos[2]);
        const bx::Vec3 color(p[i].color[0], p[i].color[1], p[i].color[2]);
        if (p[i].kind == 'c') scene->addCube(color, m);
        else if (p[i].kind == 'p') scene->addPlane(color, m);
        else scene->addAreaLight(color, m);
    }
    return scene;
}

static Shader *loadShader(const char *name, ShaderType type, const char *const *fns, const ShaderFunctionType *types, int n) {
    Shader *s = Engine::createShader();
    if (!s->load(name)) { std::cout << "Failed to load " << name << " shader." << std::endl; return nullptr; }
    for (int i = 0; i < n; ++i) s->addFunction(fns[i], types[i]);
    if (!s->compile(type)) { std::cout << "Failed to compile " << name << " shader." << std::endl; return nullptr; }
    return s;
}

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 1024, height = argc > 2 ? atoi(argv[2]) : 768;
    const int frames = argc > 3 ? atoi(argv[3]) : 64, bounces = argc > 4 ? atoi(argv[4]) : 3;
    const char *out = argc > 5 ? argv[5] : "cornell.png";
    int denoise = 0;
    bool denoiseVar = false, denoiseTemporal = false, varianceOfMean = false;
    double orbit = 0.0, slide = 0.0, lagGate = -1.0, coverMin = -1.0;
    double twist = 0.0, bulge = 0.0, bend = 0.0;
    bool refit = false, pose = false, skin = false, morph = false, rig = false;
    const char *usage = "usage: toyraygun_cornell [width height frames bounces out.png [denoise=N[,var|,temporal[,lag[=G]][,vmean][,cover[=C]]]] [orbit=DEG] [slide=D] [twist=DEG] [bulge=W] [bend=DEG] [refit|pose|skin|morph|rig]]";
    for (int a = 6; a < argc; ++a) {
        if (strncmp(argv[a], "slide=", 6) == 0) {
            char *end = nullptr;
            slide = strtod(argv[a] + 6, &end);
            if (end == argv[a] + 6 || *end != 0) { std::cout << usage << std::endl; return -1; }
            continue;
        }
        if (strcmp(argv[a], "refit") == 0) { refit = true; continue; }
        if (strcmp(argv[a], "pose") == 0) { pose = true; continue; }
        if (strcmp(argv[a], "skin") == 0) { skin = true; continue; }
        if (strcmp(argv[a], "morph") == 0) { morph = true; continue; }
        if (strcmp(argv[a], "rig") == 0) { rig = true; continue; }
        if (strncmp(argv[a], "bend=", 5) == 0) {
            char *end = nullptr;
            bend = strtod(argv[a] + 5, &end);
            if (end == argv[a] + 5 || *end != 0) { std::cout << usage << std::endl; return -1; }
            continue;
        }
        if (strncmp(argv[a], "bulge=", 6) == 0) {
            char *end = nullptr;
            bulge = strtod(argv[a] + 6, &end);
            if (end == argv[a] + 6 || *end != 0) { std::cout << usage << std::endl; return -1; }
            continue;
        }
        if (strncmp(argv[a], "twist=", 6) == 0) {
            char *end = nullptr;
            twist = strtod(argv[a] + 6, &end);
            if (end == argv[a] + 6 || *end != 0) { std::cout << usage << std::endl; return -1; }
            continue;
        }
        if (strncmp(argv[a], "orbit=", 6) == 0) {
            char *end = nullptr;
            orbit = strtod(argv[a] + 6, &end);
            if (end == argv[a] + 6 || *end != 0) { std::cout << usage << std::endl; return -1; }
            continue;
        }
        if (strncmp(argv[a], "denoise=", 8) != 0) { std::cout << usage << std::endl; return -1; }
        denoise = atoi(argv[a] + 8);
        const char *comma = strchr(argv[a] + 8, ',');
        if (comma) {
            if (strcmp(comma, ",var") == 0) denoiseVar = true;
            else if (strncmp(comma, ",temporal", 9) == 0 && (comma[9] == 0 || comma[9] == ',')) {
                denoiseTemporal = true;
                // behind ,temporal: ,lag[=G], ,vmean and ,cover[=C], each at most once, in any order
                const char *tok = comma + 9;
                bool sawLag = false, sawCover = false;
                while (*tok) {
                    const char *next = strchr(tok + 1, ',');
                    const size_t len = next ? (size_t)(next - tok) : strlen(tok);
                    if (len == 6 && strncmp(tok, ",vmean", 6) == 0 && !varianceOfMean) varianceOfMean = true;
                    else if (len == 4 && strncmp(tok, ",lag", 4) == 0 && !sawLag) { sawLag = true; lagGate = TRG_TEMPORAL_LAG_GATE_DEFAULT; }
                    else if (len > 5 && strncmp(tok, ",lag=", 5) == 0 && !sawLag) {
                        char *end = nullptr;
                        lagGate = strtod(tok + 5, &end);
                        if (end != tok + len || !(lagGate >= 0.0)) { std::cout << usage << std::endl; return -1; }
                        sawLag = true;
                    }
                    else if (len == 6 && strncmp(tok, ",cover", 6) == 0 && !sawCover) { sawCover = true; coverMin = TRG_TEMPORAL_COVERAGE_MIN_DEFAULT; }
                    else if (len > 7 && strncmp(tok, ",cover=", 7) == 0 && !sawCover) {
                        char *end = nullptr;
                        coverMin = strtod(tok + 7, &end);
                        if (end != tok + len || !(coverMin >= 0.0 && coverMin < 1.0)) { std::cout << usage << std::endl; return -1; }
                        sawCover = true;
                    }
                    else { std::cout << usage << std::endl; return -1; }
                    tok += len;
                }
            }
            else { std::cout << usage << std::endl; return -1; }
        }
    }

    if ((pose && refit) || (skin && (pose || refit)) || (morph && (pose || refit || skin)) || (rig && (pose || refit || skin || morph || slide != 0.0))) { std::cout << usage << std::endl; return -1; }

    Engine *engine = Engine::instance();
    engine->init(width, height);
    engine->setFrameBudget(frames);

    const char *rtFns[] = { "raygen", "primaryHit", "primaryMiss", "shadowHit", "shadowMiss" };
    const ShaderFunctionType rtTypes[] = { ShaderFunctionType::RayGen, ShaderFunctionType::ClosestHit, ShaderFunctionType::Miss,
                                           ShaderFunctionType::ShadowHit, ShaderFunctionType::ShadowMiss };
    const char *accFns[] = { "accumulate" };
    const ShaderFunctionType accTypes[] = { ShaderFunctionType::Compute };
    const char *ppFns[] = { "vert", "frag" };
    const ShaderFunctionType ppTypes[] = { ShaderFunctionType::Vertex, ShaderFunctionType::Fragment };
    Shader *rt = loadShader("Raytracing", ShaderType::Raytrace, rtFns, rtTypes, 5);
    Shader *acc = loadShader("Accumulate", ShaderType::Compute, accFns, accTypes, 1);
    Shader *pp = loadShader("PostProcessing", ShaderType::Graphics, ppFns, ppTypes, 2);
    if (!rt || !acc || !pp) return -1;

    Renderer *renderer = Engine::createRenderer();
    if (!renderer->init()) { std::cout << "Renderer failed to initialize." << std::endl; return -1; }
    renderer->addShader(rt);
    renderer->addShader(acc);
    renderer->addShader(pp);
    renderer->setCameraPosition(bx::Vec3(0.0f, 1.0f, 3.38f));
    renderer->setCameraLookAt(bx::Vec3(0.0f, 1.0f, -1.0f));

    // (the denoise mode first: in temporal mode the renderer remembers the geometry it uploads, for updateScene)
    HipRenderer *hip = static_cast<HipRenderer *>(renderer);
    if (!hip->setDenoise(denoise, denoiseVar, denoiseTemporal)) { std::cout << "denoise must be 0.." << 6 << std::endl; return -1; }
    if (lagGate >= 0.0 && !hip->setLagCorrection((float)lagGate)) { std::cout << "the lag correction was refused" << std::endl; return -1; }
    if (coverMin >= 0.0 && !hip->setCoverage((float)coverMin)) { std::cout << "the coverage history was refused" << std::endl; return -1; }
    if (varianceOfMean && !hip->setVarianceOfMean(true)) { std::cout << "the variance of the mean was refused" << std::endl; return -1; }
    hip->setRefit(refit);
    Scene *scene = createCornellBoxScene();
    renderer->loadScene(scene);
    hip->setBounces((unsigned int)bounces);
    // pose: the short box (the first cube the scene adds: triangles 0 .. 11) is one object, everything else the other
    const uint32_t firstTri[3] = { 0u, 12u, (uint32_t)scene->m_materialIDBuffer.size() };
    if (pose && !hip->bindObjects(scene, firstTri, 2)) { std::cout << "the objects were refused" << std::endl; return -1; }
    // skin: the short box's 36 corners (the first cube the scene adds) lean on bone 1 by their height within the box, the rest on bone 0
    // morph: one target, the copies of the short box's four top corners, each moved away from the box's vertical axis; behind it, with a twist, the
    // skin's two bones
    double axisX = 0.0, axisZ = 0.0;
    if (skin || morph) {
        const size_t nVerts = scene->m_vertexBuffer.size();
        if (nVerts < 36) { std::cout << (skin ? "the skin was refused" : "the morph was refused") << std::endl; return -1; }
        float lo = scene->m_vertexBuffer[0].y, hi = lo;
        for (size_t v = 0; v < 36; ++v) {
            lo = fminf(lo, scene->m_vertexBuffer[v].y); hi = fmaxf(hi, scene->m_vertexBuffer[v].y);
            axisX += (double)scene->m_vertexBuffer[v].x / 36.0; axisZ += (double)scene->m_vertexBuffer[v].z / 36.0;
        }
        std::vector<uint32_t> ids(nVerts * 4, 0u);
        std::vector<float> weights(nVerts * 4, 0.0f);
        for (size_t v = 0; v < nVerts; ++v) {
            const float w1 = v < 36 && hi > lo ? (scene->m_vertexBuffer[v].y - lo) / (hi - lo) : 0.0f;
            ids[v * 4 + 1] = 1u;
            weights[v * 4] = 1.0f - w1; weights[v * 4 + 1] = w1;
        }
        if (skin && !hip->bindSkin(scene, ids.data(), weights.data(), 2)) { std::cout << "the skin was refused" << std::endl; return -1; }
        if (morph) {
            std::vector<uint32_t> entryVertex;
            std::vector<float> dpos;
            for (uint32_t v = 0; v < 36; ++v)
                if (scene->m_vertexBuffer[v].y == hi) {
                    entryVertex.push_back(v);
                    dpos.push_back(scene->m_vertexBuffer[v].x - (float)axisX); dpos.push_back(0.0f); dpos.push_back(scene->m_vertexBuffer[v].z - (float)axisZ);
                }
            const uint32_t targetFirst[2] = { 0u, (uint32_t)entryVertex.size() };
            const bool bones = twist != 0.0;
            if (!hip->bindMorph(scene, 1, targetFirst, entryVertex.data(), dpos.data(), nullptr, bones ? ids.data() : nullptr, bones ? weights.data() : nullptr, bones ? 2 : 0)) {
                std::cout << "the morph was refused" << std::endl;
                return -1;
            }
        }
    }
    // rig: joints 0, 1, 2 up the short box's vertical axis, joint 3 at rest for everything else; two keys per chain joint
    if (rig) {
        const size_t nVerts = scene->m_vertexBuffer.size();
        if (nVerts < 36) { std::cout << "the rig was refused" << std::endl; return -1; }
        double lo = scene->m_vertexBuffer[0].y, hi = lo, x0 = scene->m_vertexBuffer[0].x, x1 = x0, z0 = scene->m_vertexBuffer[0].z, z1 = z0;
        for (size_t v = 0; v < 36; ++v) {
            lo = fmin(lo, (double)scene->m_vertexBuffer[v].y); hi = fmax(hi, (double)scene->m_vertexBuffer[v].y);
            x0 = fmin(x0, (double)scene->m_vertexBuffer[v].x); x1 = fmax(x1, (double)scene->m_vertexBuffer[v].x);
            z0 = fmin(z0, (double)scene->m_vertexBuffer[v].z); z1 = fmax(z1, (double)scene->m_vertexBuffer[v].z);
        }
        double origin[4][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
        for (int k = 0; k < 3; ++k) { origin[k][0] = (x0 + x1) / 2; origin[k][1] = lo + (hi - lo) * (double)k / 2; origin[k][2] = (z0 + z1) / 2; }
        std::vector<uint32_t> ids(nVerts * 4);
        std::vector<float> weights(nVerts * 4, 0.0f);
        for (size_t v = 0; v < nVerts; ++v) {
            for (uint32_t k = 0; k < 4; ++k) ids[v * 4 + k] = k;
            if (v >= 36 || !(hi > lo)) { weights[v * 4 + 3] = 1.0f; continue; }
            const double h = ((double)scene->m_vertexBuffer[v].y - lo) / (hi - lo);
            for (int k = 0; k < 3; ++k) weights[v * 4 + k] = (float)fmax(0.0, 1.0 - fabs(2.0 * h - (double)k));
        }
        const double a = bend * (double)(frames - 1) * 3.14159265358979323846 / 180.0;
        const uint32_t parent[4] = { 0xFFFFFFFFu, 0u, 1u, 0xFFFFFFFFu }, keyFirst[5] = { 0u, 2u, 4u, 6u, 7u }, clockOf[4] = { 0u, 0u, 0u, 0u };
        float keys[7 * 12] = { 0 }, invBind[4 * 12] = { 0 };
        for (int k = 0; k < 4; ++k) {
            for (int i = 0; i < (k < 3 ? 2 : 1); ++i) {
                float *key = keys + (keyFirst[k] + i) * 12;
                key[0] = (float)i;
                for (int e = 0; e < 3; ++e) key[1 + e] = k < 3 ? (float)(origin[k][e] - (k ? origin[k - 1][e] : 0.0)) : 0.0f;
                key[4] = i ? (float)sin(a / 2) : 0.0f;
                key[7] = i ? (float)cos(a / 2) : 1.0f;
                key[8] = key[9] = key[10] = 1.0f;
            }
            invBind[k * 12] = invBind[k * 12 + 5] = invBind[k * 12 + 10] = 1.0f;
            for (int e = 0; e < 3; ++e) invBind[k * 12 + 4 * e + 3] = (float)-origin[k][e];
        }
        if (!hip->bindSkin(scene, ids.data(), weights.data(), 4) || !hip->bindRig(parent, 4, keyFirst, keys, clockOf, 1, invBind)) {
            std::cout << "the rig was refused" << std::endl;
            return -1;
        }
    }
    const bx::Vec3 eye0(0.0f, 1.0f, 3.38f), at(0.0f, 1.0f, -1.0f);
    int call = 0;
    while (!engine->hasQuit()) {
        engine->pollEvents();
        if (engine->hasQuit()) break;
        if (orbit != 0.0) {   // the eye of call k: turned by k * orbit degrees about the vertical axis through the look-at point
            const double t = orbit * (double)call * 3.14159265358979323846 / 180.0;
            const double dx = (double)eye0.x - (double)at.x, dz = (double)eye0.z - (double)at.z;
            renderer->setCameraPosition(bx::Vec3((float)((double)at.x + dx * cos(t) + dz * sin(t)), eye0.y, (float)((double)at.z - dx * sin(t) + dz * cos(t))));
        }
        if ((skin || morph) && (twist != 0.0 || (morph && bulge != 0.0)) && call > 0) {
            // bone 1: x' = R (x - axis) + axis, R a turn by call * twist degrees about the vertical through (axisX, axisZ)
            const double t = twist * (double)call * 3.14159265358979323846 / 180.0, cs = cos(t), sn = sin(t);
            float bones[24] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
            bones[12] = (float)cs; bones[14] = (float)sn; bones[15] = (float)(axisX - cs * axisX - sn * axisZ);
            bones[20] = (float)-sn; bones[22] = (float)cs; bones[23] = (float)(axisZ + sn * axisX - cs * axisZ);
            const float weight = (float)call * (float)bulge;
            if (skin) hip->poseSkin(bones);
            else hip->poseMorph(&weight, twist != 0.0 ? bones : nullptr);
        } else if (rig && bend != 0.0 && call > 0 && frames > 1) {
            const float clock = (float)((double)call / (double)(frames - 1));
            hip->animateSkin(&clock);
        } else if (pose && slide != 0.0 && call > 0) {
            float x[24] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
            x[3] = (float)((double)call * slide);
            hip->poseObjects(x);
        } else if (slide != 0.0 && call > 0) {
            Scene *moved = createSlidCornellBox((float)((double)call * slide));
            hip->updateScene(moved);
            delete moved;   // (the renderer borrows the scene for the call only)
        }
        renderer->renderFrame();
        ++call;
    }
    printf("%d frames, %llu rays, last frame %.3f ms\n", hip->getFrameIndex(), (unsigned long long)hip->getRayCount(), hip->getLastRenderMs());
    if (refit) printf("%u scene updates served by a refit\n", hip->getRefitCount());
    if (!hip->savePNG(out)) { std::cout << "Failed to write " << out << std::endl; return -1; }
    printf("wrote %s\n", out);
    if (pose) printf("%u poses applied\n", hip->getPoseCount());
    if (skin) printf("%u skins applied\n", hip->getSkinCount());
    if (morph) printf("%u morphs applied\n", hip->getMorphCount());
    if (rig) printf("%u rigs applied\n", hip->getRigCount());
    return 0;
}
