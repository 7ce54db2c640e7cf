// Sanitizer driver for the host mirror's projector packing (LightingRenderer::PackProjectorLight and the Matrix operations under it):
// 2 000 lights, among them singular and perspective transforms, zero scales, positions of 3e38, rotations and missing textures.
// A stand-alone program; build and run from the repository root (the library must be built: the mirror links against it):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iilluminant_amd/host -Iinclude \
//       tools/san_pack_projector.cpp illuminant_amd/host/illuminant_host.cpp -Lilluminant_amd/lib -lilluminant_hip \
//       -Wl,-rpath,$PWD/illuminant_amd/lib -o /tmp/san_pack_projector && /tmp/san_pack_projector
// Prints "packed 1714 of 2000" and exits 0 when neither sanitizer reports anything (286 lights have no texture and are skipped).
#include "illuminant_host.hpp"
#include <cstdio>
#include <cmath>
using namespace Squared::Illuminant;
using namespace Squared::Illuminant::Lighting;
int main() {
    auto tex = std::make_shared<RampTexture>();
    tex->Width = 5; tex->Height = 3; tex->Texels.resize(15);
    int packed = 0;
    for (int k = 0; k < 2000; k++) {
        ProjectorLightSource l;
        l.TextureRef = (k % 7 == 0) ? nullptr : tex;
        const float a = 0.01f * k;
        l.Transform.M[0][0] = std::cos(a); l.Transform.M[0][1] = std::sin(a); l.Transform.M[1][0] = -std::sin(a); l.Transform.M[1][1] = std::cos(a);
        if (k % 11 == 0) l.Transform.M[2][2] = 0;             // singular
        if (k % 13 == 0) l.Transform.M[0][3] = 0.01f;         // perspective
        l.Scale = { 0.25f + 0.1f * (k % 9), (k % 17 == 0) ? 0.0f : 1.5f };
        l.Position = { 3.0f * k, -2.0f * k, (k % 5 == 0) ? 3e38f : 1.0f };
        if (k % 3) l.Rotation = { 0, 0, std::sin(a / 2), std::cos(a / 2) };
        if (k % 4) l.Origin = Vector3{ 1, 2, 3 };
        if (k % 6) l.Depth = 64.0f;
        l.Wrap = k % 2;
        IlmLightVertex v;
        if (LightingRenderer::PackProjectorLight(l, 1.0f + k, k % 2, 128.0f, Vector2{ 1.0f, (k % 19 == 0) ? 0.0f : 2.0f }, -0.33f, v)) packed++;
    }
    std::printf("packed %d of 2000\n", packed);
    return packed == 2000 - 286 ? 0 : 1;
}
