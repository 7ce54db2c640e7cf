// Sanitizer driver for the host mirror's volumetric-light packing (LightingRenderer::PackVolumetricLight): 2 100 lights over the three
// shapes and an unknown one, among them Opacity <= 0, coincident corners, positions of 3e38 and NaN, infinite colours, a missing direction
// and falloff and every RampMode.
// A stand-alone program; build and run from the repository root (the library must be built: the mirror links against it):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iilluminant_amd/host -Iinclude \
//       tools/san_pack_volumetric.cpp illuminant_amd/host/illuminant_host.cpp -Lilluminant_amd/lib -lilluminant_hip \
//       -Wl,-rpath,$PWD/illuminant_amd/lib -o /tmp/san_pack_volumetric && /tmp/san_pack_volumetric
// Prints "packed 1260 of 2100" and exits 0 when neither sanitizer reports anything (420 lights have Opacity <= 0 and 525 the unknown
// shape 3; 105 have both).
#include "illuminant_host.hpp"
#include <cstdio>
#include <cmath>
#include <limits>
using namespace Squared::Illuminant;
using namespace Squared::Illuminant::Lighting;
int main() {
    int packed = 0;
    double sum = 0;
    for (int k = 0; k < 2100; k++) {
        VolumetricLightSource l;
        l.Shape = (VolumetricLightShape)(k % 4);
        l.StartPosition = { 3.0f * k, -2.0f * k, (k % 7 == 0) ? 3e38f : 10.0f };
        l.EndPosition = (k % 9 == 0) ? l.StartPosition : Vector3{ -1.5f * k, 4.0f, (k % 13 == 0) ? std::numeric_limits<float>::quiet_NaN() : 30.0f };
        if (k % 2) l.LightDirection = Vector3{ 0.1f * (k % 5), -0.2f, (k % 11 == 0) ? std::numeric_limits<float>::infinity() : -0.9f };
        l.StartRadius = 0.5f * (k % 11); l.EndRadius = (k % 4 == 0) ? 0.0f : 2.0f;
        l.RampMode = (LightSourceRampMode)(k % 3);
        l.Color = (k % 6 == 0) ? Vector4{ 1e30f * k, 0.5f, 0.25f, std::numeric_limits<float>::infinity() } : Vector4{ 1, 0.5f, 0.25f, 0.9f };
        l.Opacity = (k % 5 == 0) ? ((k % 10 == 0) ? 0.0f : -1.0f) : 0.001f * k;
        l.CastsShadows = k % 2;
        if (k % 3) l.ShadowDistanceFalloff = 2.0f;
        l.AmbientOcclusionRadius = 1.0f * (k % 8); l.AmbientOcclusionOpacity = 0.125f * (k % 8); l.FalloffYFactor = 1.0f + (k % 3);
        l.Volumetricity = 0.25f * (k % 6); l.RampLength = 0.5f * (k % 9); l.RampPower = 0.5f * (k % 5); l.BlowoutFactor = 0.1f * (k % 4);
        l.DistanceAttenuation = 0.5f + (k % 3);
        IlmLightVertex v;
        if (LightingRenderer::PackVolumetricLight(l, 1.0f + k, k % 3 == 0, v)) {
            packed++;
            if (v.EvenMoreLightProperties.w != (float)(k % 4) || v.LightProperties.w != ((k % 2) && (k % 3 == 0) ? 1.0f : 0.0f)) return 2;
            if ((k % 4 != 1) && !(v.LightPosition2.x >= 0 || v.LightPosition2.x != v.LightPosition2.x)) return 3;      // half-extents are absolute values
            const float* f = reinterpret_cast<const float*>(&v);
            for (int i = 0; i < 32; i++) if (f[i] == f[i] && std::isfinite(f[i])) sum += f[i];      // every member was written
        }
    }
    std::printf("packed %d of 2100 (checksum %.6g)\n", packed, sum);
    return packed == 1260 ? 0 : 1;
}
