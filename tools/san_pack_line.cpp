// Sanitizer driver for the host mirror's line-light packing (LightingRenderer::PackLineLight): 2 000 lights, among them Opacity <= 0,
// coincident ends, positions of 3e38 and NaN, infinite colours, a missing falloff and every RampMode.
// A stand-alone program; build and run from the repository root (the library must be built: the mirror links against it):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iilluminant_amd/host -Iinclude \
//       tools/san_pack_line.cpp illuminant_amd/host/illuminant_host.cpp -Lilluminant_amd/lib -lilluminant_hip \
//       -Wl,-rpath,$PWD/illuminant_amd/lib -o /tmp/san_pack_line && /tmp/san_pack_line
// Prints "packed 1600 of 2000" and exits 0 when neither sanitizer reports anything (400 lights have Opacity <= 0 and are skipped).
#include "illuminant_host.hpp"
#include <cstdio>
#include <cmath>
#include <limits>
using namespace Squared::Illuminant;
using namespace Squared::Illuminant::Lighting;
int main() {
    int packed = 0;
    double sum = 0;
    for (int k = 0; k < 2000; k++) {
        LineLightSource l;
        l.StartPosition = { 3.0f * k, -2.0f * k, (k % 7 == 0) ? 3e38f : 10.0f };
        l.EndPosition = (k % 9 == 0) ? l.StartPosition : Vector3{ -1.5f * k, 4.0f, (k % 13 == 0) ? std::numeric_limits<float>::quiet_NaN() : 30.0f };
        l.Radius = (k % 4 == 0) ? 0.0f : 0.5f * (k % 11);
        l.RampMode = (LightSourceRampMode)(k % 3);
        if (k % 6 == 0) l.SetColor(Vector4{ 1e30f * k, 0.5f, 0.25f, std::numeric_limits<float>::infinity() });
        else { l.StartColor = { 1, 0.5f, 0.25f, 0.9f }; l.EndColor = { 0.1f, 0.2f, 0.3f, 0.01f * k }; }
        l.Opacity = (k % 5 == 0) ? ((k % 10 == 0) ? 0.0f : -1.0f) : 0.001f * k;
        l.CastsShadows = k % 2;
        if (k % 3) l.ShadowDistanceFalloff = 2.0f;
        l.AmbientOcclusionRadius = 1.0f * (k % 8); l.AmbientOcclusionOpacity = 0.125f * (k % 8); l.FalloffYFactor = 1.0f + (k % 3);
        l.RampOffset = 0.1f * k; l.RampRate = (k % 17 == 0) ? 0.0f : 2.0f;
        IlmLightVertex v;
        if (LightingRenderer::PackLineLight(l, 1.0f + k, k % 3 == 0, v)) {
            packed++;
            if (v.LightProperties.y != 0 || v.LightProperties.w != ((k % 2) && (k % 3 == 0) ? 1.0f : 0.0f)) return 2;
            const float* f = reinterpret_cast<const float*>(&v);
            for (int i = 0; i < 32; i++) if (f[i] == f[i] && std::isfinite(f[i])) sum += f[i];      // every member was written
        }
    }
    std::printf("packed %d of 2000 (checksum %.6g)\n", packed, sum);
    return packed == 1600 ? 0 : 1;
}
