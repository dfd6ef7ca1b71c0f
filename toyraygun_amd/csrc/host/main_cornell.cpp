// main_cornell.cpp -- headless demo following the reference app's call order (reference src/main.cpp:16-98):
// engine init -> three shaders -> renderer init -> camera -> Cornell box -> frame loop; then writes a PNG.
//   toyraygun_cornell [width height frames bounces out.png [denoise=N[,var|,temporal]] [orbit=DEG]]
//     denoise=N    a-trous iterations of the written image, 0 = off (default)
//     ,var         the variance-guided filter from two half-sample buffers
//     ,temporal    the frames are rendered as `frames` calls of 1 spp, each a temporal step (reprojected history, temporal variance); the
//                  picture is the last step's
//     orbit=DEG    the eye turns about the look-at point (about the vertical axis) by DEG degrees per call
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>

#include "cornellBox.h"
#include "engine/Engine.h"
#include "engine/HipRenderer.h"
#include "engine/Renderer.h"
#include "engine/Shader.h"

using namespace toyraygun;

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
    bool denoiseVar = false, denoiseTemporal = false;
    double orbit = 0.0;
    const char *usage = "usage: toyraygun_cornell [width height frames bounces out.png [denoise=N[,var|,temporal]] [orbit=DEG]]";
    for (int a = 6; a < argc; ++a) {
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
            else if (strcmp(comma, ",temporal") == 0) denoiseTemporal = true;
            else { std::cout << usage << std::endl; return -1; }
        }
    }

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

    Scene *scene = createCornellBoxScene();
    renderer->loadScene(scene);

    HipRenderer *hip = static_cast<HipRenderer *>(renderer);
    hip->setBounces((unsigned int)bounces);
    if (!hip->setDenoise(denoise, denoiseVar, denoiseTemporal)) { std::cout << "denoise must be 0.." << 6 << std::endl; return -1; }
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
        renderer->renderFrame();
        ++call;
    }
    printf("%d frames, %llu rays, last frame %.3f ms\n", hip->getFrameIndex(), (unsigned long long)hip->getRayCount(), hip->getLastRenderMs());
    if (!hip->savePNG(out)) { std::cout << "Failed to write " << out << std::endl; return -1; }
    printf("wrote %s\n", out);
    return 0;
}
