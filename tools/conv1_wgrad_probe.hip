// tools only (round 6): where does conv1's weight gradient spend its time?  The fp32-boundary kernel (conv1_wgrad_tr2_kernel, 263 us in the step for 983 MB of frames
// + 315 MB of dY) and round 5's uint8 one (raw rows through LDS, since removed: 246 MB of frames) took about the SAME time — so the 4 x smaller input bought nothing and the bound had to be
// a phase they share.  Phase ablation on 2048 static-camera frames: full | no multiply loop | no prefetch of the next band | neither.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DHULC_W1_PROBE tools/conv1_wgrad_probe.hip -o tools/bin/conv1_wgrad_probe && tools/bin/conv1_wgrad_probe
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cstring>
#include <vector>
#include <algorithm>
#include <cmath>
#include "../hulc_amd/csrc/conv_wgrad.h"
void hulc_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
using namespace hulc_bf16;
int main() {
    for (int cam = 0; cam < 2; ++cam) {
        const int Nf = 2048, IH = cam ? 84 : 200, OH = (IH - 8) / 4 + 1;
        float* x32; unsigned char* x8; h16_t* dy; float *part, *bias;
        const size_t nx = (size_t)Nf * 3 * IH * IH, ny = (size_t)Nf * OH * OH * 32;
        hipMalloc(&x32, nx * 4); hipMalloc(&x8, nx); hipMalloc(&dy, ny * 2); hipMalloc(&part, sizeof(float) * 512ll * 32 * 192); hipMalloc(&bias, sizeof(float) * 512 * 64);
        {   std::vector<float> h(nx); unsigned s = 1; for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 9) - (1 << 22)) * (1.f / (1 << 22)); }
            hipMemcpy(x32, h.data(), nx * 4, hipMemcpyHostToDevice);
            std::vector<unsigned char> b(nx); for (auto& v : b) { s = s * 1664525u + 1013904223u; v = (unsigned char)(s >> 24); }
            hipMemcpy(x8, b.data(), nx, hipMemcpyHostToDevice);
            std::vector<h16_t> g(ny); for (auto& v : g) { s = s * 1664525u + 1013904223u; const float f = ((int)(s >> 9) - (1 << 22)) * (0.01f / (1 << 22)); unsigned u; memcpy(&u, &f, 4); v = (h16_t)((u + 0x8000u) >> 16); }
            hipMemcpy(dy, g.data(), ny * 2, hipMemcpyHostToDevice); }
        int* ctr; hipMalloc(&ctr, 256);
        int* shifts; hipMalloc(&shifts, Nf * 2 * sizeof(int));
        {   std::vector<int> h(Nf * 2); unsigned s2 = 7; const int pad = cam ? 4 : 10; for (auto& v : h) { s2 = s2 * 1664525u + 1013904223u; v = (int)((s2 >> 8) % (2 * pad + 1)); }
            hipMemcpy(shifts, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice); }
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        for (int u8 : {0, 2, 3}) {                                // 0: fp32 boundary, 2: uint8 converted from the prefetch registers (round 6), 3: the same with interior / row-end slots
            g_conv1_wgrad_u8reg = u8 ? u8 - 1 : -1;
            Conv1Src src{}; src.X = u8 ? (const void*)x8 : (const void*)x32; src.u8 = u8 != 0; src.fold = u8 != 0;
            if (u8) { src.shift = shifts; src.pad = cam ? 4 : 10; }      // RandomShiftsAug draws as in bench.py --ingest u8
            float t[32];
            for (int d = 0; d < 32; ++d) t[d] = 1e30f;
            for (int round = 0; round < 4; ++round)               // alternating rounds, minimum per arm: one arm's 10 launches in a row pick up the box's drift
            for (int dbg : {0, 1, 2, 3, 11, 19, 27}) {
                hipMemcpyToSymbol(HIP_SYMBOL(g_w1_probe), &dbg, sizeof(int));
                auto launch = [&]() { hipMemsetAsync(ctr, 0, 256, 0); launch_conv1_wgrad_tr(0, src, dy, part, bias, Nf, IH, IH, OH, OH, 512, ctr); };
                for (int i = 0; i < 2; ++i) launch();
                hipDeviceSynchronize(); hipEventRecord(e0);
                for (int i = 0; i < 8; ++i) launch();
                hipEventRecord(e1); hipDeviceSynchronize();
                float ms; hipEventElapsedTime(&ms, e0, e1); t[dbg] = std::min(t[dbg], ms * 125.f);
            }
            if (u8) {                                             // the two uint8 forms must produce the same slabs (same products, same order): compare after a full launch
                int z = 0; hipMemcpyToSymbol(HIP_SYMBOL(g_w1_probe), &z, sizeof(int));
                hipMemsetAsync(ctr, 0, 256, 0); hipMemsetAsync(bias, 0, sizeof(float) * 512 * 64, 0);
                const int grid = launch_conv1_wgrad_tr(0, src, dy, part, bias, Nf, IH, IH, OH, OH, 512, nullptr);      // static frame order: slabs comparable
                std::vector<float> h((size_t)grid * 32 * 192); hipMemcpy(h.data(), part, h.size() * 4, hipMemcpyDeviceToHost);
                static std::vector<float> ref;
                if (u8 == 2) ref = h;
                else { double dmax = 0, n = 0; for (size_t i = 0; i < h.size(); ++i) { dmax = std::max(dmax, (double)fabsf(h[i] - ref[i])); n = std::max(n, (double)fabsf(ref[i])); }
                       printf("         u8spl vs u8reg slabs: max |diff| %.3g (max |value| %.3g, %d slabs)\n", dmax, n, grid); }
            }
            const double mb = (double)Nf * (3.0 * IH * IH * (u8 ? 1 : 4) + OH * OH * 32 * 2.0) / 1e6;
            printf("%-8s %-5s full %6.1f us (%4.2f TB/s of %4.0f MB)  no-multiply %6.1f  no-prefetch %6.1f  neither %6.1f", cam ? "gripper" : "static", u8 == 0 ? "fp32" : (u8 == 2 ? "u8reg" : "u8spl"), t[0], mb / t[0], mb, t[1], t[2], t[3]);
            if (u8 >= 2) printf("  | of 'neither': without the conversion %6.1f  without the dY staging %6.1f  without both (barriers + band bookkeeping) %6.1f", t[11], t[19], t[27]);
            printf("\n");
        }
    }
    return 0;
}
