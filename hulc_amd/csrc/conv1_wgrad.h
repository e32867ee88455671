// hulc_amd/csrc/conv1_wgrad.h — conv1's weight gradient from the boundary frames (fp32 NCHW or uint8 NHWC through conv1_stage.h): three kernel forms, the plan that
// picks form and band height (conv1_wgrad_plan) and the one launcher, launch_conv1_wgrad_jobs (up to four jobs per launch).
#pragma once
#include <algorithm>
#include "conv1_stage.h"

namespace HULC_NS {

// ---------------------------------------------------------------------------------------------------------------------
// conv1 (8x8 stride 4, 3 -> 32 channels) weight gradient straight from the fp32 NCHW boundary frames.
//   dW[co][(c,kh,kw)] = sum dY[n][oh][ow][co] * X[n][c][oh*4+kh][ow*4+kw]
// The X band is converted to bf16 while it is staged ([c][row][iw] image), dY is staged as [pix][32]; an n-tile of 16 packed
// columns = (c, two kernel rows kh, 8 kw): lane chunk q covers kh = kh_lo + q/2, kw = (q&1)*4..+3 -> 4 contiguous bf16 in a row.
// ---------------------------------------------------------------------------------------------------------------------
struct Wgrad1Cfg {
    static constexpr int CO = 32, KH = 8, KW = 8, S = 4, C = 3;
    static constexpr int DYS = CO * 2 + 32;     // 96 B = 32 x odd: the 4 pixel rows x 4 chunks of a tr-read group fall on distinct bank pairs (80 B pitched pixel 3 onto pixel 0: 44 % conflict cycles, tools/pmc_sq.sh)
    static size_t lds_bytes(int R, int IW, int OW, bool u8 = false) {
        const int OWp = (OW + 7) / 8 * 8;
        const int XR = (R - 1) * S + KH;
        return (size_t)C * XR * (IW * 2 + 16) + 512 + (size_t)(R * OWp + 8) * DYS + (u8 ? (size_t)XR * conv1_raw_pitch(IW) + 16 : 0);   // + raw uint8 rows
    }
};

// One conv1 weight-gradient job of a launch (the two cameras' frames, or the two frame sources of a camera in the paired pass): the arguments the kernels below took
// one by one.  A workgroup belongs to ONE job for its life: the job whose block range [blk0, next blk0) holds blockIdx.x; the body sees its index within the job (bid)
// and the job's workgroup count (nwg) where a one-job launch has blockIdx.x and gridDim.x.  part = the job's own slab area, work_ctr its own claim counter.
struct Wgrad1Job { Conv1Src S; int* work_ctr; const h16_t* dY; float* part; float* bias_part; int Nf, IH, IW, OH, OW, R, nbands, blk0; };
struct Wgrad1Batch { Wgrad1Job j[4]; int n; };
#define WGRAD1_PICK_JOB(bt)                                                                       \
    int jk = 0;                                                                                   \
    while (jk + 1 < bt.n && (int)blockIdx.x >= bt.j[jk + 1].blk0) ++jk;                           \
    const Wgrad1Job& J = bt.j[jk];                                                                \
    const int bid = (int)blockIdx.x - J.blk0, nwg = (jk + 1 < bt.n ? bt.j[jk + 1].blk0 : (int)gridDim.x) - J.blk0;

DEVI void conv1_wgrad_tr_body(const Conv1Src& X, int* __restrict__ work_ctr, const h16_t* __restrict__ dY, float* __restrict__ part,
                              float* __restrict__ bias_part, int Nf, int IH, int IW, int OH, int OW, int R, const int bid, const int nwg) {
    using C = Wgrad1Cfg;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OWp = (OW + 7) & ~7, U = OWp >> 3;
    const int XR = (R - 1) * C::S + C::KH;
    const int XRS = IW * 2 + 16;                                  // bytes per staged input row
    const int xbytes = C::C * XR * XRS + 512;
    const int dypix = R * OWp + 8;
    lds_char* ximg = (lds_char*)smem;
    lds_char* dyimg = ximg + xbytes;
    for (int i = tid * 16; i < xbytes + dypix * C::DYS; i += 256 * 16) *(lds_u32x4*)((lds_char*)smem + i) = u32x4_t{0u, 0u, 0u, 0u};
    __syncthreads();

    f32x4 acc[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2, q = a & 3;
    const int ccolA = q * 8;
    const int nt0 = wave * 3;
    const int W4 = IW >> 2;                                       // float4 per input row (IW % 4 == 0)
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    __shared__ int s_nextf[2];
    int fiter = 0;
    for (int f = bid; f < Nf;) {
        if (work_ctr && tid == 0) s_nextf[fiter & 1] = nwg + atomicAdd(work_ctr, 1);   // next frame claimed dynamically (see ConvTileP::work_ctr)
        for (int oh0 = 0; oh0 < OH; oh0 += R) {
            __syncthreads();
            {   // dY band, one row per wave pass
                for (int r = wave; r < R; r += 4) {
                    const bool in = oh0 + r < OH;
                    const h16_t* src = dY + ((long long)f * OH + min(oh0 + r, OH - 1)) * OW * C::CO;
                    for (int i = lane; i < OW * 4; i += 64) {
                        u32x4_t v = *reinterpret_cast<const u32x4_t*>(src + i * 8);
                        if (!in) v = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                        for (int e = 0; e < 4; ++e) { bsum[2 * e] += h2f_lo(v[e]); bsum[2 * e + 1] += h2f_hi(v[e]); }
                        *(lds_u32x4*)(dyimg + (r * OWp + (i >> 2)) * C::DYS + (i & 3) * 16) = v;
                    }
                }
            }
            {   // X band -> bf16 [c][row][iw]
                const int ih0 = oh0 * C::S;
                conv1_stage_band(X, f, ih0, min(XR, IH - ih0), IH, IW, ximg, XR, XRS, tid, dyimg + dypix * C::DYS);
            }
            __syncthreads();
            const int units = R * U;
            for (int u0 = 0; u0 < units; u0 += 4) {
                const int u = u0 + g;
                const bool valid = u < units;
                const int r = valid ? u / U : 0, ow0 = valid ? (u % U) * 8 : 0;
                const int pixA = valid ? r * OWp + ow0 : R * OWp;
                lds_char* abase = dyimg + (pixA + prow) * C::DYS + ccolA;
                h16x8_t af[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) af[c] = tr_read8(abase + c * 32, abase + 4 * C::DYS + c * 32);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int nt = nt0 + j;
                    const int ch = nt >> 2, kh = (nt & 3) * 2 + (q >> 1);
                    lds_char* bbase = ximg + (ch * XR + r * C::S + kh) * XRS + ((ow0 + prow) * C::S + (q & 1) * 4) * 2;
                    const h16x8_t bf = tr_read8(bbase, bbase + 4 * C::S * 2);
#pragma unroll
                    for (int c = 0; c < 2; ++c) acc[j][c] = MFMA_16x16x32_H(af[c], bf, acc[j][c], 0, 0, 0);
                }
            }
        }
        f = work_ctr ? s_nextf[fiter & 1] : f + nwg;   // written >= 2 barriers ago; the other slot is the one tid 0 writes next
        ++fiter;
    }
    float* out = part + (long long)bid * C::CO * 192;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long long)(c * 16 + g * 4 + r) * 192 + (nt0 + j) * 16 + a] = acc[j][c][r];
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < C::CO) {
        const int cgrp = tid >> 3, e = tid & 7;
        float s = 0.f;
        for (int t = cgrp; t < 256; t += 4) s += red[t * 8 + e];
        if (bias_part) unsafeAtomicAdd(bias_part + tid, s);
    }
}
__global__ void __launch_bounds__(256, 2) conv1_wgrad_tr_kernel(Wgrad1Batch bt) {
    WGRAD1_PICK_JOB(bt)
    conv1_wgrad_tr_body(J.S, J.work_ctr, J.dY, J.part, J.bias_part, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, bid, nwg);
}

// ---------------------------------------------------------------------------------------------------------------------
// v2 of the kernel above for the fp32 NCHW boundary (the headline configuration): 8 waves, 2 workgroups per CU, and the NEXT band's
// frames + dY rows prefetched into registers while the current band multiplies.
//   v1 runs 4 workgroups per CU that each stage a band (loads -> wait -> convert -> LDS) and then multiply it; the HBM stream stalls
//   whenever the resident workgroups are all converting / multiplying, the bands are 3 output rows tall (39 KB of LDS each), so every
//   band re-stages 4 of its 16 input rows (33 % over-fetch) and pays its barriers for 12 new rows.  It moved 1.53 GB in 370 us (3.6 of
//   the ~6.3 TB/s a streaming copy reaches).
//   v2: bands of 7 output rows (32 input rows: 14 % over-fetch, 7 bands per 49-row frame), 13 x 16 B per thread in flight for the whole
//   multiply phase of the previous band (106 KB per workgroup), zero rows applied at the commit, the two wave halves split the pixel
//   units and are summed through LDS at the end.
// ---------------------------------------------------------------------------------------------------------------------
template <int PFX, int PFY>
DEVI void conv1_wgrad_tr2_body(const float* __restrict__ X, int* __restrict__ work_ctr, const h16_t* __restrict__ dY, float* __restrict__ part,
                               float* __restrict__ bias_part, int Nf, int IH, int IW, int OH, int OW, int R, int nbands, const int bid, const int nwg) {
    using C = Wgrad1Cfg;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OWp = (OW + 7) & ~7, U = OWp >> 3;
    const int XR = (R - 1) * C::S + C::KH;
    const int XRS = IW * 2 + 16;
    const int xbytes = C::C * XR * XRS + 512;
    const int dypix = R * OWp + 8;
    lds_char* ximg = (lds_char*)smem;
    lds_char* dyimg = ximg + xbytes;
    for (int i = tid * 16; i < xbytes + dypix * C::DYS; i += 512 * 16) *(lds_u32x4*)((lds_char*)smem + i) = u32x4_t{0u, 0u, 0u, 0u};
    const int W4 = IW >> 2;
    const int nx = C::C * XR * W4, ny = R * OW * 4;               // 16-byte chunks of a band: fp32 frame quads, dY channel quarters
    // band-invariant slot descriptors, one register each: frame slots (channel << 16 | row << 8 | float4 column), dY slots (row << 16 | chunk)
    int xd[PFX], yd[PFY];
#pragma unroll
    for (int k = 0; k < PFX; ++k) {
        const int e = min(tid + k * 512, nx - 1);
        const int c = e / (XR * W4), rem = e - c * (XR * W4), r = rem / W4, q4 = rem - r * W4;
        xd[k] = (c << 16) | (r << 8) | q4;
    }
#pragma unroll
    for (int k = 0; k < PFY; ++k) {
        const int e = min(tid + k * 512, ny - 1);
        const int r = e / (OW * 4), i = e - r * (OW * 4);
        yd[k] = (r << 16) | i;
    }
    f32x4 acc[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2, q = a & 3;
    const int ccolA = q * 8;
    const int nt0 = (wave & 3) * 3, uh = wave >> 2;
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 px[PFX];
    u32x4_t py[PFY];
    int xrows = 0, yrows = 0;                                     // rows of the prefetched band inside the frame (others are zeros)
    const int nitems = Nf * nbands;
    auto prefetch = [&](int item) {
        const int f = item / nbands, oh0 = (item % nbands) * R;
        const int ih0 = oh0 * C::S;
        xrows = min(XR, IH - ih0); yrows = min(R, OH - oh0);
        const float* xb = X + ((long long)f * C::C * IH + ih0) * IW;
        const h16_t* yb = dY + ((long long)f * OH + oh0) * OW * C::CO;
#pragma unroll
        for (int k = 0; k < PFX; ++k) {
            const int c = xd[k] >> 16, r = (xd[k] >> 8) & 0xff, q4 = xd[k] & 0xff;
            px[k] = *reinterpret_cast<const float4*>(xb + (c * IH + min(r, xrows - 1)) * IW + q4 * 4);       // rows below the frame: re-read a valid row (zeroed at the commit)
        }
#pragma unroll
        for (int k = 0; k < PFY; ++k) {
            const int r = yd[k] >> 16, i = yd[k] & 0xffff;
            py[k] = *reinterpret_cast<const u32x4_t*>(yb + (min(r, yrows - 1) * OW) * C::CO + i * 8);
        }
    };
    // A workgroup walks the bands of ONE frame back to back (work unit = frame, claimed dynamically): the (KH - S) input rows two
    // consecutive bands share are then re-read by the same CU a few microseconds later and come from L2 instead of HBM (with the bands of
    // a frame dealt to different workgroups the PMC counters showed 27 % more HBM bytes than the frames hold).
    __shared__ int s_next[2];
    int frame = bid, fiter = 0, band = 0;
    int item = frame * nbands;
    if (frame < Nf) prefetch(item);
    while (frame < Nf) {
        if (band == 0 && work_ctr && tid == 0) s_next[fiter & 1] = nwg + atomicAdd(work_ctr, 1);
        __syncthreads();                                          // previous band consumed (first pass: zero fill visible)
        const int cxr = xrows, cyr = yrows;
#pragma unroll
        for (int k = 0; k < PFX; ++k)
            if (tid + k * 512 < nx) {
                const int c = xd[k] >> 16, r = (xd[k] >> 8) & 0xff, q4 = xd[k] & 0xff;
                const bool in = r < cxr;
                u32x2_t o;
                o[0] = in ? pack2h(px[k].x, px[k].y) : 0u;
                o[1] = in ? pack2h(px[k].z, px[k].w) : 0u;
                *(__attribute__((address_space(3))) u32x2_t*)(ximg + (c * XR + r) * XRS + q4 * 8) = o;
            }
#pragma unroll
        for (int k = 0; k < PFY; ++k)
            if (tid + k * 512 < ny) {
                const int r = yd[k] >> 16, i = yd[k] & 0xffff;
                const u32x4_t v = r < cyr ? py[k] : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 4; ++e) { bsum[2 * e] += h2f_lo(v[e]); bsum[2 * e + 1] += h2f_hi(v[e]); }
                *(lds_u32x4*)(dyimg + (r * OWp + (i >> 2)) * C::DYS + (i & 3) * 16) = v;
            }
        __syncthreads();
        if (++band == nbands) {                                   // next frame (its claim was written at the frame's first band: >= 1 barrier ago)
            band = 0;
            frame = work_ctr ? s_next[fiter & 1] : frame + nwg;
            ++fiter;
        }
        item = frame * nbands + band;
        if (frame < Nf) prefetch(item);      // in flight during the MFMAs below
        const int units = R * U;
        // run u = u0 + g -> (row ur, run uo of the row) advanced by adds (8 runs per step): a runtime division per step stood next to 6 MFMAs
        int joff[3];                                   // per n-tile: (channel, kernel row) of this lane's B rows + its column half
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int nt = nt0 + j; joff[j] = ((nt >> 2) * XR + (nt & 3) * 2 + (q >> 1)) * XRS + (q & 1) * 8; }
        const int q8 = 8 / U, r8 = 8 - q8 * U;
        int ur, uo;
        { const int u = uh * 4 + g; ur = u / U; uo = u - ur * U; }
#pragma unroll 1
        for (int u0 = uh * 4; u0 < units; u0 += 8) {
            const int u = u0 + g;
            const bool valid = u < units;
            const int r = valid ? ur : 0, ow0 = valid ? uo * 8 : 0;
            ur += q8; uo += r8;
            if (uo >= U) { uo -= U; ++ur; }
            const int pixA = valid ? r * OWp + ow0 : R * OWp;
            lds_char* abase = dyimg + (pixA + prow) * C::DYS + ccolA;
            h16x8_t af[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) af[c] = tr_read8(abase + c * 32, abase + 4 * C::DYS + c * 32);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lds_char* bbase = ximg + joff[j] + (r * C::S) * XRS + (ow0 + prow) * C::S * 2;
                const h16x8_t bf = tr_read8(bbase, bbase + 4 * C::S * 2);
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[j][c] = MFMA_16x16x32_H(af[c], bf, acc[j][c], 0, 0, 0);
            }
        }
    }
    // ---- the two unit halves (waves w and w + 4) are summed through LDS, then one slab per workgroup
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    if (uh == 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 2; ++c) red[((wave & 3) * 6 + j * 2 + c) * 64 + lane] = acc[j][c];
    }
    __syncthreads();
    if (uh == 0) {
        float* out = part + (long long)bid * C::CO * 192;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const f32x4 v = acc[j][c] + red[((wave & 3) * 6 + j * 2 + c) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(long long)(c * 16 + g * 4 + r) * 192 + (nt0 + j) * 16 + a] = v[r];
            }
    }
    __syncthreads();
    float* redf = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) redf[tid * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < C::CO) {
        const int cgrp = tid >> 3, e = tid & 7;
        float sacc = 0.f;
        for (int t = cgrp; t < 512; t += 4) sacc += redf[t * 8 + e];
        if (bias_part) unsafeAtomicAdd(bias_part + tid, sacc);
    }
}
template <int PFX, int PFY>
__global__ void __launch_bounds__(512, 4) conv1_wgrad_tr2_kernel(Wgrad1Batch bt) {
    WGRAD1_PICK_JOB(bt)
    conv1_wgrad_tr2_body<PFX, PFY>(reinterpret_cast<const float*>(J.S.X), J.work_ctr, J.dY, J.part, J.bias_part, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, J.nbands, bid, nwg);
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 6: the v2 structure for the uint8 (.., H, W, C) boundary with the conversion done FROM THE PREFETCH REGISTERS (round 5 prefetched the next band as raw bytes and
// converted them in LDS; profiles/r06_conv1_wgrad_probe.txt: commit + conversion were 119 of that kernel's 251 us — raw rows into LDS, margins, a barrier, a second pass that reads them back — and the 4 x smaller frames bought nothing over the fp32 boundary's 261 us).  A prefetch slot is
// the aligned 16-byte window around a 4-pixel group's 12 bytes (one dwordx4 load; 33 % more bytes requested, the overlaps hit in L2); the column shift and the replicate
// pad are resolved per pixel from the window at the commit.  One barrier per band less, no raw rows in LDS.
// ---------------------------------------------------------------------------------------------------------------------
// SPLIT (round 6, second pass): slots 0 .. PFX - 2 hold INTERIOR groups only (conv1_interior_groups: no clamp, no per-pixel select, one alignbyte shift per frame),
// slot PFX - 1 the few groups next to the row ends (threads [0, XR * edge groups per row)) with the general conversion — the slot index is an unrolled compile-time
// constant, so no wave pays the slow path for its interior lanes.  Same LDS image, same slabs.
template <int PFX, int PFY, bool SPLIT = false>
DEVI void conv1_wgrad_tr2r_body(const Conv1Src& S, int* __restrict__ work_ctr, const h16_t* __restrict__ dY, float* __restrict__ part,
                                float* __restrict__ bias_part, int Nf, int IH, int IW, int OH, int OW, int R, int nbands, const int bid, const int nwg) {
    using C = Wgrad1Cfg;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OWp = (OW + 7) & ~7, U = OWp >> 3;
    const int XR = (R - 1) * C::S + C::KH;
    const int XRS = IW * 2 + 16;
    const int xbytes = C::C * XR * XRS + 512;
    const int dypix = R * OWp + 8;
    lds_char* ximg = (lds_char*)smem;
    lds_char* dyimg = ximg + xbytes;
    for (int i = tid * 16; i < xbytes + dypix * C::DYS; i += 512 * 16) *(lds_u32x4*)((lds_char*)smem + i) = u32x4_t{0u, 0u, 0u, 0u};
    const int W4 = IW >> 2;
    const int RB = IW * 3, n4 = RB >> 2;                          // bytes / 4-byte chunks per source row
    const int nx = XR * W4, ny = R * OW * 4;                       // 4-pixel groups of a band (one 16-byte slot each), dY channel quarters
    const unsigned char* Xb = reinterpret_cast<const unsigned char*>(S.X);
    // raw slot k of this thread = chunk tid + 512 k of the [XR][n4] grid: (row, chunk) advanced incrementally from slot 0's — twelve
    // descriptor registers next to twelve slots of in-flight data spilled 17 registers at the 128-VGPR budget and serialised the prefetch
    // ... and the compiler hoists whatever is band-invariant out of the band loop and spills it just the same (a scratch reload in front of
    // every prefetch load waits for the loads issued before it): slot 0's (row, chunk) is recomputed per band behind an opaque copy of tid
    const int xdq = 512 / W4, xdr = 512 - xdq * W4;                // slot k of this thread = group tid + 512 k of the [XR][W4] grid, advanced by adds
    // SPLIT: interior groups [cl, cl + WI) of every row in slots 0 .. PFX - 2 ([XR][WI] grid), the WE = W4 - WI others in slot PFX - 1 ([XR][WE] grid)
    int cl = 0, WI = 0;
    if (SPLIT) conv1_interior_groups(IW, S.pad, ((PFX - 1) * 512) / XR, cl, WI);
    const int WE = W4 - WI, ni = XR * WI, ne = XR * WE;
    const int idq = SPLIT ? 512 / max(WI, 1) : 0, idr = 512 - idq * WI;
    const float invWI = 1.f / (float)max(WI, 1), invWE = 1.f / (float)max(WE, 1);
    int yd[PFY];
#pragma unroll
    for (int k = 0; k < PFY; ++k) {
        const int e = min(tid + k * 512, ny - 1);
        const int r = e / (OW * 4), i = e - r * (OW * 4);
        yd[k] = (r << 16) | i;
    }
    f32x4 acc[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2, q = a & 3;
    const int ccolA = q * 8;
    const int nt0 = (wave & 3) * 3, uh = wave >> 2;
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    u32x4_t px[PFX];                                              // slot = the aligned 16-byte window that holds a group's 12 bytes
    u32x4_t py[PFY];
    int xrows = 0, yrows = 0, pdx = 0;
    auto prefetch = [&](int item) {
        const int f = item / nbands, oh0 = (item % nbands) * R;
        const int ih0 = oh0 * C::S;
        xrows = min(XR, IH - ih0); yrows = min(R, OH - oh0);
        int dy = 0;
        pdx = 0;
        S.offsets(f, pdx, dy);
        const unsigned char* fb = Xb + S.frame(f) * IH * RB;
        const h16_t* yb = dY + ((long long)f * OH + oh0) * OW * C::CO;
        if constexpr (SPLIT) {
            int t = tid;
            asm volatile("" : "+v"(t));
            const int rmax = min(XR, xrows) - 1;
            int r = wg_fdiv(t, invWI), ci = t - r * WI;
            const int off0 = 12 * cl + 3 * pdx;                      // 3 (4 c + dx) = the group's first byte in its row
#pragma unroll
            for (int k = 0; k < PFX - 1; ++k) {
                px[k] = *reinterpret_cast<const u32x4_t*>(fb + (long long)min(max(ih0 + min(r, rmax) + dy, 0), IH - 1) * RB + ((off0 + 12 * ci) & ~3));
                ci += idr; r += idq; if (ci >= WI) { ci -= WI; ++r; }
            }
            const int re = wg_fdiv(t, invWE), ce = t - re * WE, c = ce < cl ? ce : ce + WI;
            px[PFX - 1] = *reinterpret_cast<const u32x4_t*>(fb + (long long)min(max(ih0 + min(re, rmax) + dy, 0), IH - 1) * RB + conv1_window_off(c, pdx, IW, RB));
        } else {
            int t = tid;
            asm volatile("" : "+v"(t));
            int r = t / W4, c = t - r * W4;
#pragma unroll
            for (int k = 0; k < PFX; ++k) {
                const int rr = min(r, min(XR, xrows) - 1);            // slots past the band / rows below the frame: a valid row (dropped / zeroed at the commit)
                px[k] = *reinterpret_cast<const u32x4_t*>(fb + (long long)min(max(ih0 + rr + dy, 0), IH - 1) * RB + conv1_window_off(c, pdx, IW, RB));
                c += xdr; r += xdq; if (c >= W4) { c -= W4; ++r; }
            }
        }
#pragma unroll
        for (int k = 0; k < PFY; ++k) {
            const int r = yd[k] >> 16, i = yd[k] & 0xffff;
            py[k] = *reinterpret_cast<const u32x4_t*>(yb + (min(r, yrows - 1) * OW) * C::CO + i * 8);
        }
    };
    __shared__ int s_next[2];
    int frame = bid, fiter = 0, band = 0;
    int item = frame * nbands;
    if (frame < Nf) prefetch(item);
    while (frame < Nf) {
        if (band == 0 && work_ctr && tid == 0) s_next[fiter & 1] = nwg + atomicAdd(work_ctr, 1);
        __syncthreads();                                          // previous band consumed (first pass: zero fill visible)
        const int cxr = xrows, cyr = yrows, dx = pdx;
        {
            // the band's 4-pixel groups straight from the prefetch registers into the 16-bit [c][row][iw] image (no raw rows in LDS, no margin fill, no barrier
            // between a raw commit and a conversion pass): window -> the 12 bytes of pixels qp .. qp + 3 -> for output pixel k of the group the source pixel
            // clamp(c 4 + k + dx) - qp (= k everywhere but at the row ends, where RandomShiftsAug's replicate pad repeats the edge pixel)
            auto commit_x = [&](auto FOLD_) __attribute__((always_inline)) {      // the folded path (production) converts the byte as it is: no multiply-add
            constexpr bool FOLD = decltype(FOLD_)::value;
            int t = tid;
            asm volatile("" : "+v"(t));
            if constexpr (SPLIT) {
                const int shu = (3 * dx) & 3;
                int r = wg_fdiv(t, invWI), ci = t - r * WI;
#pragma unroll
                for (int k = 0; k < PFX - 1; ++k) {
                    if (t + k * 512 < ni) {
                        u32x2_t ov[3] = {u32x2_t{0u, 0u}, u32x2_t{0u, 0u}, u32x2_t{0u, 0u}};
                        if (r < cxr) {
                            unsigned lo[3], hi[3];
                            conv1_window_group_interior<FOLD>(px[k], shu, lo, hi);
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) { ov[ch][0] = lo[ch]; ov[ch][1] = hi[ch]; }
                        }
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) *(__attribute__((address_space(3))) u32x2_t*)(ximg + (ch * XR + r) * XRS + (cl + ci) * 8) = ov[ch];
                    }
                    ci += idr; r += idq; if (ci >= WI) { ci -= WI; ++r; }
                }
                if (t < ne) {
                    const int re = wg_fdiv(t, invWE), ce = t - re * WE, c = ce < cl ? ce : ce + WI;
                    u32x2_t ov[3] = {u32x2_t{0u, 0u}, u32x2_t{0u, 0u}, u32x2_t{0u, 0u}};
                    if (re < cxr) {
                        unsigned lo[3], hi[3];
                        conv1_window_group<FOLD>(px[PFX - 1], c, dx, IW, RB, lo, hi);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) { ov[ch][0] = lo[ch]; ov[ch][1] = hi[ch]; }
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) *(__attribute__((address_space(3))) u32x2_t*)(ximg + (ch * XR + re) * XRS + c * 8) = ov[ch];
                }
                return;
            }
            int r = t / W4, c = t - r * W4;
#pragma unroll
            for (int k = 0; k < PFX; ++k) {
                if (t + k * 512 < nx) {
                    u32x2_t ov[3] = {u32x2_t{0u, 0u}, u32x2_t{0u, 0u}, u32x2_t{0u, 0u}};
                    if (r < cxr) {                                // rows below the frame stay zero
                        unsigned lo[3], hi[3];
                        conv1_window_group<FOLD>(px[k], c, dx, IW, RB, lo, hi);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) { ov[ch][0] = lo[ch]; ov[ch][1] = hi[ch]; }
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) *(__attribute__((address_space(3))) u32x2_t*)(ximg + (ch * XR + r) * XRS + c * 8) = ov[ch];
                }
                c += xdr; r += xdq; if (c >= W4) { c -= W4; ++r; }
            }
            };
            if (S.fold) commit_x(std::true_type{}); else commit_x(std::false_type{});
        }
#pragma unroll
        for (int k = 0; k < PFY; ++k)
            if (tid + k * 512 < ny) {
                const int r = yd[k] >> 16, i = yd[k] & 0xffff;
                const u32x4_t v = r < cyr ? py[k] : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 4; ++e) { bsum[2 * e] += h2f_lo(v[e]); bsum[2 * e + 1] += h2f_hi(v[e]); }
                *(lds_u32x4*)(dyimg + (r * OWp + (i >> 2)) * C::DYS + (i & 3) * 16) = v;
            }
        __syncthreads();
        if (++band == nbands) {
            band = 0;
            frame = work_ctr ? s_next[fiter & 1] : frame + nwg;
            ++fiter;
        }
        item = frame * nbands + band;
        if (frame < Nf) prefetch(item);      // in flight during the MFMAs below
        const int units = R * U;
        // run u = u0 + g -> (row ur, run uo of the row) advanced by adds (8 runs per step): a runtime division per step stood next to 6 MFMAs
        int joff[3];                                   // per n-tile: (channel, kernel row) of this lane's B rows + its column half
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int nt = nt0 + j; joff[j] = ((nt >> 2) * XR + (nt & 3) * 2 + (q >> 1)) * XRS + (q & 1) * 8; }
        const int q8 = 8 / U, r8 = 8 - q8 * U;
        int ur, uo;
        { const int u = uh * 4 + g; ur = u / U; uo = u - ur * U; }
#pragma unroll 1
        for (int u0 = uh * 4; u0 < units; u0 += 8) {
            const int u = u0 + g;
            const bool valid = u < units;
            const int r = valid ? ur : 0, ow0 = valid ? uo * 8 : 0;
            ur += q8; uo += r8;
            if (uo >= U) { uo -= U; ++ur; }
            const int pixA = valid ? r * OWp + ow0 : R * OWp;
            lds_char* abase = dyimg + (pixA + prow) * C::DYS + ccolA;
            h16x8_t af[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) af[c] = tr_read8(abase + c * 32, abase + 4 * C::DYS + c * 32);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lds_char* bbase = ximg + joff[j] + (r * C::S) * XRS + (ow0 + prow) * C::S * 2;
                const h16x8_t bf = tr_read8(bbase, bbase + 4 * C::S * 2);
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[j][c] = MFMA_16x16x32_H(af[c], bf, acc[j][c], 0, 0, 0);
            }
        }
    }
    // ---- the bias partial of this workgroup first (Conv1Src::fold needs it for the slab), then the two unit halves (waves w and w + 4) are summed
    // through LDS and one slab per workgroup is written
    __syncthreads();
    float* redf = reinterpret_cast<float*>(smem);
    float* dbw = redf + 6144;                                    // [CO]: this workgroup's bias-gradient partial (24 KB in: behind redf's 16 KB and red's 24 KB)
#pragma unroll
    for (int e = 0; e < 8; ++e) redf[tid * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < C::CO) {
        const int cgrp = tid >> 3, e = tid & 7;
        float sacc = 0.f;
        for (int t = cgrp; t < 512; t += 4) sacc += redf[t * 8 + e];
        if (bias_part) unsafeAtomicAdd(bias_part + tid, sacc);
        dbw[tid] = sacc;
    }
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    if (uh == 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 2; ++c) red[((wave & 3) * 6 + j * 2 + c) * 64 + lane] = acc[j][c];
    }
    __syncthreads();
    if (uh == 0) {
        float* out = part + (long long)bid * C::CO * 192;
        const float fsc = S.fold ? CONV1_FOLD_SCALE : 1.f;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const f32x4 v = acc[j][c] + red[((wave & 3) * 6 + j * 2 + c) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = c * 16 + g * 4 + r;
                    out[(long long)co * 192 + (nt0 + j) * 16 + a] = S.fold ? fmaf(v[r], fsc, -dbw[co]) : v[r];      // dW = (2/255) (dY * u) - db (x) 1
                }
            }
    }
}
template <int PFX, int PFY, bool SPLIT = false>
__global__ void __launch_bounds__(512, 4) conv1_wgrad_tr2r_kernel(Wgrad1Batch bt) {
    WGRAD1_PICK_JOB(bt)
    conv1_wgrad_tr2r_body<PFX, PFY, SPLIT>(J.S, J.work_ctr, J.dY, J.part, J.bias_part, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, J.nbands, bid, nwg);
}

// Kernel form and band height of one conv1 weight-gradient job: 1 = conv1_wgrad_tr2_kernel<6, 2> (fp32 frames), 2 = conv1_wgrad_tr2r_kernel<3, 2, true>,
// 3 = conv1_wgrad_tr2r_kernel<4, 2> (uint8 frames), 5 = conv1_wgrad_tr_kernel (any shape).  u8form: which uint8 form is tried first — 2 (the engine's) or 1, the
// general-slot form 3 that hulc_k_conv1_wgrad_u8 can ask for
static inline int conv1_wgrad_plan(const Conv1Src& X, int IH, int IW, int OH, int OW, int& R_out, int& nb_out, size_t& lds_out, int u8form = 2) {
    auto balanced = [&](int R) { const int nb = (OH + R - 1) / R; nb_out = nb; R_out = (OH + nb - 1) / nb; };
    if (!X.u8 && (IW % 4) == 0) {
        // tallest band whose images fit 2 workgroups per CU and whose chunks fit the prefetch slots (8 frame + 2 dY registers of 16 B per thread:
        // 10 + 3 slots spilled 46 registers of in-flight data at the 128-VGPR budget of 2 x 8 waves per CU, which serialised the prefetch)
        int R = OH;
        auto fits = [&](int r) {
            const int XR = (r - 1) * Wgrad1Cfg::S + Wgrad1Cfg::KH;
            return Wgrad1Cfg::lds_bytes(r, IW, OW) <= (size_t)79 * 1024 && (long long)3 * XR * (IW / 4) <= 6 * 512 && (long long)r * OW * 4 <= 2 * 512 && XR < 128 && r < 128;
        };
        while (R > 1 && !fits(R)) --R;
        if (fits(R)) {
            balanced(R);
            lds_out = std::max<size_t>(Wgrad1Cfg::lds_bytes(R_out, IW, OW), 512 * 8 * sizeof(float));
            return 1;
        }
    }
    // uint8 forms: 2 = conversion from the prefetch registers with interior / row-end slots (conv1_wgrad_tr2r_kernel<3, 2, true>), 1 = one general slot kind
    if (X.u8 && (IW % 4) == 0 && IW >= 8 && u8form >= 2) {
        // round 6, second pass: 2 slots of interior groups (fast conversion) + 1 slot of row-end groups + 2 dY slots per thread (conv1_wgrad_tr2r_kernel<3, 2, true>)
        int R = OH;
        auto fits = [&](int r) {
            const int XR = (r - 1) * Wgrad1Cfg::S + Wgrad1Cfg::KH;
            int cl, wi;
            conv1_interior_groups(IW, X.pad, (2 * 512) / XR, cl, wi);
            return Wgrad1Cfg::lds_bytes(r, IW, OW, false) <= (size_t)79 * 1024 && wi >= 1 && (long long)XR * wi <= 2 * 512 && (long long)XR * (IW / 4 - wi) <= 512 &&
                   (long long)r * OW * 4 <= 2 * 512 && r < 128;
        };
        while (R > 1 && !fits(R)) --R;
        if (fits(R)) {
            balanced(R);
            lds_out = std::max<size_t>(Wgrad1Cfg::lds_bytes(R_out, IW, OW, false), 32 * 1024);
            return 2;
        }
    }
    if (X.u8 && (IW % 4) == 0 && IW >= 8) {
        // uint8 boundary, round 6: 4 window slots of 16 bytes + 2 dY slots per thread, converted from the registers (conv1_wgrad_tr2r_kernel); no raw rows in LDS
        int R = OH;
        auto fits = [&](int r) {
            const int XR = (r - 1) * Wgrad1Cfg::S + Wgrad1Cfg::KH;
            return Wgrad1Cfg::lds_bytes(r, IW, OW, false) <= (size_t)79 * 1024 && (long long)XR * (IW / 4) <= 4 * 512 && (long long)r * OW * 4 <= 2 * 512 && r < 128;
        };
        while (R > 1 && !fits(R)) --R;
        if (fits(R)) {
            balanced(R);
            lds_out = std::max<size_t>(Wgrad1Cfg::lds_bytes(R_out, IW, OW, false), 32 * 1024);      // (>= the epilogue's reduction areas: 24.6 KB)
            return 3;
        }
    }
    constexpr int lds_kb = 39;   // 4 workgroups per CU (0.44 vs 0.50 ms/step at 2 per CU with 78 KB bands)
    int R = OH;
    while (R > 1 && Wgrad1Cfg::lds_bytes(R, IW, OW, X.u8) > (size_t)lds_kb * 1024) --R;
    R_out = R; nb_out = (OH + R - 1) / R;
    lds_out = Wgrad1Cfg::lds_bytes(R, IW, OW, X.u8);
    return 5;
}
// conv1's weight gradient for up to four jobs as ONE launch: the two cameras' frames (and, in the paired pass, each camera's two frame sources).  Every job must
// take the same kernel form (else false: nothing launched); each job's band height is its own, the dynamic LDS the largest.  The launch's workgroups — as many as
// one launch of the largest job would start — are divided over the jobs by camera_split on frames x bands x (multiply steps of 8 eight-pixel runs + 1), no job
// more than its frames (work unit = frame); wg != nullptr: the counts as given (tests).  j[0].part = the slab area: job k's slabs lie behind job k - 1's
// (part of the later jobs is set here).  ns[k] = slabs (= workgroups) of job k.
static inline bool launch_conv1_wgrad_jobs(hipStream_t st, Wgrad1Job* j, int n, int max_blocks, const int* wg, int* ns, int u8form = 2) {
    if (n < 1 || n > 4) return false;
    int form = 0; size_t lds = 0; double w[4]; int cap = 0;
    for (int k = 0; k < n; ++k) {
        size_t l = 0;
        const int f = conv1_wgrad_plan(j[k].S, j[k].IH, j[k].IW, j[k].OH, j[k].OW, j[k].R, j[k].nbands, l, u8form);
        if (k && f != form) return false;
        if (j[k].Nf < 1) return false;
        form = f; lds = std::max(lds, l);
        const int U = (j[k].OW + 7) / 8;
        w[k] = (double)j[k].Nf * j[k].nbands * ((j[k].R * U + 7) / 8 + 1);
        cap = std::max(cap, j[k].Nf);
    }
    const int grid = std::min(form == 5 ? cap : std::min(cap, 512), max_blocks);
    long long total = 0;
    for (int k = 0; k < n; ++k) total += j[k].Nf;
    if (wg) { for (int k = 0; k < n; ++k) ns[k] = std::min(std::max(wg[k], 1), j[k].Nf); }
    else if (n == 1) ns[0] = grid;
    else if (total <= std::min(form == 5 ? (int)total : 512, max_blocks)) { for (int k = 0; k < n; ++k) ns[k] = j[k].Nf; }      // (small calls) one frame per workgroup, as in separate launches
    else {
        if (grid < n) return false;
        int left = grid; double wl = 0;
        for (int k = 0; k < n; ++k) wl += w[k];
        for (int k = n - 1; k > 0; --k) {          // job k against the jobs before it; those keep at least one workgroup each
            int a, b;
            camera_split(left, wl - w[k], w[k], a, b);
            b = std::min(std::min(b, left - k), j[k].Nf);
            ns[k] = b; left -= b; wl -= w[k];
        }
        ns[0] = std::min(left, j[0].Nf);
    }
    Wgrad1Batch bt{}; bt.n = n;
    int blk = 0;
    for (int k = 0; k < n; ++k) {
        if (k) j[k].part = j[k - 1].part + (long long)ns[k - 1] * Wgrad1Cfg::CO * 192;
        j[k].blk0 = blk; blk += ns[k];
        bt.j[k] = j[k];
    }
    if (form == 1) {
        max_dyn_lds_once<&conv1_wgrad_tr2_kernel<6, 2>>(80 * 1024);
        hipLaunchKernelGGL((conv1_wgrad_tr2_kernel<6, 2>), dim3(blk), dim3(512), lds, st, bt);
    } else if (form == 2) {
        max_dyn_lds_once<&conv1_wgrad_tr2r_kernel<3, 2, true>>(80 * 1024);
        hipLaunchKernelGGL((conv1_wgrad_tr2r_kernel<3, 2, true>), dim3(blk), dim3(512), lds, st, bt);
    } else if (form == 3) {
        max_dyn_lds_once<&conv1_wgrad_tr2r_kernel<4, 2>>(80 * 1024);
        hipLaunchKernelGGL((conv1_wgrad_tr2r_kernel<4, 2>), dim3(blk), dim3(512), lds, st, bt);
    } else {
        for (int k = 0; k < n; ++k) bt.j[k].S.fold = 0;      // this (fallback) kernel writes the plain slab: it stages x itself
        max_dyn_lds_once<&conv1_wgrad_tr_kernel>(160 * 1024 - 64);
        hipLaunchKernelGGL(conv1_wgrad_tr_kernel, dim3(blk), dim3(256), lds, st, bt);
    }
    return true;
}
static inline int launch_conv1_wgrad_tr(hipStream_t st, const Conv1Src& X, const h16_t* dY, float* part, float* bias_part, int Nf, int IH, int IW, int OH,
                                        int OW, int max_blocks, int* work_ctr = nullptr, int u8form = 2) {
    Wgrad1Job q{}; q.S = X; q.work_ctr = work_ctr; q.dY = dY; q.part = part; q.bias_part = bias_part; q.Nf = Nf; q.IH = IH; q.IW = IW; q.OH = OH; q.OW = OW;
    int ns = 0;
    return launch_conv1_wgrad_jobs(st, &q, 1, max_blocks, nullptr, &ns, u8form) ? ns : 0;
}

}  // namespace HULC_NS
