// hulc_amd/csrc/conv_wgrad.h — convolution weight gradients for NHWC bf16 activations on gfx950.
//
//   dW[co][(kh,kw,ci)] = sum_{n,oh,ow} dY[n][oh][ow][co] * X[n][oh*S+kh][ow*S+kw][ci]
//
// Both MFMA operands are reduction-strided in memory (the reduction runs over pixels, the layouts are channel-fastest),
// which is exactly what ds_read_b64_tr_b16 exists for: the RAW tiles — a band of dY rows and the band of X rows under it —
// are copied once into LDS in their natural [pixel][channel] order, and every operand fragment is produced by transposing
// LDS reads.  No im2col: the (kh,kw) taps are address offsets into the X image, so each input element is fetched from HBM
// once per band instead of KH*KW times.  The reduction unit is an 8-pixel run inside one output row (rows are padded to a
// multiple of 8 with zero dY pixels), so each 16-lane group of an MFMA (k = 32 = 4 groups x 8) can address its own run.
//
// tr-read semantics (probed on MI355X, tools/probe_trread.py): within a 16-lane group, lane i receives element (i & 3) of the
// 8-byte chunks addressed by lanes (j*4 + (i >> 2)), j = 0..3.  So lane a addresses chunk [k-row = a >> 2][cols (a & 3)*4 ..+3]
// and lane i ends up with column i of the 4 x 16 block, rows 0..3 — the K-contiguous fragment the bf16 MFMA wants.
//
// Work split: persistent workgroups (4 waves) loop over frames and row bands, keep the whole CO x (KH*KW*CI) gradient in
// accumulator registers (wave w owns a quarter of the n-tiles), and write one fp32 partial slab each at the end; the existing
// deterministic slab reduction (unpack_conv_wgrad_kernel) finishes the job.
#pragma once
#include <algorithm>
#include "lds_types.h"

namespace HULC_NS {

template <int CI, int CO, int KH, int KW, int S>
struct WgradCfg {
    // LDS bytes per pixel.  A ds_read_b64_tr_b16 is served in two 32-lane halves; with the k <-> pixel assignment of the v2 kernel
    // a half reads 8 pixels (stride S) x 32 B, which tiles the 64 banks exactly iff pitch * S = 32 * odd bytes
    // (SQ_LDS_BANK_CONFLICT: 45 % of the LDS cycles with the old +16 pitch at S = 1, 0 with this one)
    static constexpr int XS = (S == 1) ? ((CI * 2 / 32) | 1) * 32 : CI * 2 + 16;
    static constexpr int DYS = ((CO * 2 / 32) | 1) * 32;
    static constexpr int CGN = CI / 16;             // channel groups per tap
    static constexpr int NT = KH * KW * CGN;        // n-tiles (16 columns of the packed K dimension each)
    static constexpr int NTW = NT / 4;              // n-tiles per wave
    static constexpr int CT = CO / 16;              // co-tiles
    static_assert(NT % 4 == 0, "n-tiles must split over 4 waves");
    static size_t lds_bytes(int R, int IW, int OW) {
        const int OWp = (OW + 7) / 8 * 8;
        const int XR = (R - 1) * S + KH;
        return (size_t)(XR * IW + 8 * S + KW) * XS + (size_t)(R * OWp + 8) * DYS;
    }
};

template <int CI, int CO, int KH, int KW, int S>
__global__ void __launch_bounds__(256, 2) conv_wgrad_tr_kernel(const h16_t* __restrict__ X, const h16_t* __restrict__ dY, float* __restrict__ part,
                                                            float* __restrict__ bias_part, int Nf, int IH, int IW, int OH, int OW, int R) {
    using C = WgradCfg<CI, CO, KH, KW, S>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OWp = (OW + 7) & ~7, U = OWp >> 3;
    const int XR = (R - 1) * S + KH;
    const int xpix = XR * IW + 8 * S + KW;          // incl. zero tail read by the padded pixels of the last row
    const int dypix = R * OWp + 8;                  // last 8 pixels: permanent zeros (target of idle lane groups)
    lds_char* ximg = (lds_char*)smem;
    lds_char* dyimg = ximg + xpix * C::XS;
    // zero everything once: pads must be finite (0 * NaN would poison the sum) and dY pads must be 0
    for (int i = tid * 16; i < xpix * C::XS + dypix * C::DYS; i += 256 * 16) *(lds_u32x4*)((lds_char*)smem + i) = u32x4_t{0u, 0u, 0u, 0u};
    __syncthreads();

    f32x4 acc[C::NTW][C::CT];
#pragma unroll
    for (int j = 0; j < C::NTW; ++j)
#pragma unroll
        for (int c = 0; c < C::CT; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2;                         // pixel (k-row) this lane addresses inside an 8-pixel run: prow, prow + 4
    const int ccol = (a & 3) * 8;                    // byte offset of this lane's 4-channel chunk inside a 16-channel group
    const int nt0 = wave * C::NTW;
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // bias gradient: this lane's 8 channels (chunk lane % CH) of every dY pixel it stages

    for (int f = blockIdx.x; f < Nf; f += gridDim.x) {
        for (int oh0 = 0; oh0 < OH; oh0 += R) {
            __syncthreads();                         // previous band fully consumed
            // ---- stage dY band [R][OWp][CO] (rows outside the frame -> zeros): one band row per wave pass, no per-chunk division
            {
                constexpr int CH = CO / 8;           // 16-byte chunks per pixel
                for (int r = wave; r < R; r += 4) {
                    const bool in = oh0 + r < OH;
                    const h16_t* src = dY + ((long long)f * OH + min(oh0 + r, OH - 1)) * OW * CO;
                    for (int i = lane; i < OW * CH; i += 64) {
                        u32x4_t v = *reinterpret_cast<const u32x4_t*>(src + i * 8);
                        if (!in) v = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
                        for (int e = 0; e < 4; ++e) { bsum[2 * e] += h2f_lo(v[e]); bsum[2 * e + 1] += h2f_hi(v[e]); }
                        *(lds_u32x4*)(dyimg + (r * OWp + i / CH) * C::DYS + (i % CH) * 16) = v;
                    }
                }
            }
            // ---- stage X band [XR][IW][CI] (rows below the frame keep stale finite data: they only meet zero dY rows)
            {
                constexpr int CH = CI / 8;
                const int ih0 = oh0 * S;
                const int rows = min(XR, IH - ih0);
                const int total = rows * IW * CH;
                const h16_t* src = X + ((long long)f * IH + ih0) * IW * CI;
                for (int i0 = tid; i0 < total; i0 += 256 * 8) {          // 8 independent 16-byte loads in flight per thread
                    u32x4_t v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {                           // unconditional (clamped) loads: no branch, no per-load wait
                        const int i = min(i0 + u * 256, total - 1);
                        v[u] = *reinterpret_cast<const u32x4_t*>(src + (long long)(i / CH) * CI + (i % CH) * 8);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + u * 256;
                        if (i < total) *(lds_u32x4*)(ximg + (i / CH) * C::XS + (i % CH) * 16) = v[u];
                    }
                }
            }
            __syncthreads();
            // ---- MFMA over the band: 4 eight-pixel runs (one per lane group) per step
            const int units = R * U;
            for (int u0 = 0; u0 < units; u0 += 4) {
                const int u = u0 + g;
                const bool valid = u < units;
                const int r = valid ? u / U : 0, ow0 = valid ? (u % U) * 8 : 0;
                const int pixA = valid ? r * OWp + ow0 : R * OWp;      // idle groups read the permanent zero pixels
                lds_char* abase = dyimg + (pixA + prow) * C::DYS + ccol;
                h16x8_t af[C::CT];
#pragma unroll
                for (int c = 0; c < C::CT; ++c) af[c] = tr_read8(abase + c * 32, abase + 4 * C::DYS + c * 32);
                const int pixB0 = (r * S) * IW + ow0 * S;
#pragma unroll
                for (int j = 0; j < C::NTW; ++j) {
                    const int nt = nt0 + j;
                    const int tap = nt / C::CGN, cg = nt % C::CGN;
                    const int kh = tap / KW, kw = tap % KW;
                    lds_char* bbase = ximg + (pixB0 + kh * IW + kw + prow * S) * C::XS + cg * 32 + ccol;
                    const h16x8_t bf = tr_read8(bbase, bbase + 4 * S * C::XS);
#pragma unroll
                    for (int c = 0; c < C::CT; ++c) acc[j][c] = MFMA_16x16x32_H(af[c], bf, acc[j][c], 0, 0, 0);
                }
            }
        }
    }
    // ---- partial slab: part[block][co][nt*16 + n], D layout: row (co) = (lane>>4)*4 + r, col (n) = lane & 15
    constexpr int KC = KH * KW * CI;
    float* out = part + (long long)blockIdx.x * CO * KC;
#pragma unroll
    for (int j = 0; j < C::NTW; ++j)
#pragma unroll
        for (int c = 0; c < C::CT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long long)(c * 16 + g * 4 + r) * KC + (nt0 + j) * 16 + a] = acc[j][c][r];
    // ---- bias-gradient slab: channel c = 8*(tid % CH) + e is spread over the threads with the same tid % CH
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < CO) {
        constexpr int CH = CO / 8;
        const int cgrp = tid >> 3, e = tid & 7;
        float s = 0.f;
        for (int t = cgrp; t < 256; t += CH) s += red[t * 8 + e];
        if (bias_part) unsafeAtomicAdd(bias_part + tid, s);          // bias_part = the bias gradient itself (<= gridDim.x adds per channel); null: the caller sums dY's columns itself (reproducible mode)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// v2 of the kernel above: ONE 8-wave workgroup per CU instead of two 4-wave ones.
//   * wave = (n-quarter q, co-half h): 2 co-tiles x NT/4 n-tiles of accumulators (72 VGPRs at conv3 instead of 144), which
//     leaves room for
//   * a register prefetch of the NEXT band (dY rows + X rows, 16 x 16 B per thread) that is in flight during the MFMAs of the
//     current one — the two-workgroup version had nothing in flight while it multiplied and nothing multiplying while it staged;
//   * whole-frame bands where the frame fits (conv3: 152 KB of LDS), balanced bands otherwise (no 1-row tail band).
// Chunk k of a thread is (dY or X, LDS offset, global offset) packed in one register; loads are unconditional (clamped).
// ---------------------------------------------------------------------------------------------------------------------
// One weight-gradient job of a launch (conv_wgrad_tr8_body / conv_wgrad_dma_body): the operands and band geometry the kernels used to take as separate arguments.
// part = the job's OWN slab area (slab index = the workgroup's index within the job), work_ctr its own claim counter.
struct WgradJob {
    const h16_t* X; const h16_t* dY; float* part; float* bias_part; const h16_t* zeros;
    int Nf, IH, IW, OH, OW, R, nbands; int* work_ctr; int FPB;
};
// bid / nwg: index of this workgroup within its job and the job's workgroup count (blockIdx.x / gridDim.x of a one-job launch)
template <int CI, int CO, int KH, int KW, int S, int NWV, int D = 3, int IWC = 0>      // IWC: compile-time image width (0: run time), see conv_wgrad_dma_kernel
DEVI void conv_wgrad_tr8_body(const WgradJob& J, const int bid, const int nwg) {
    const h16_t* __restrict__ const X = J.X; const h16_t* __restrict__ const dY = J.dY; float* __restrict__ const part = J.part; float* __restrict__ const bias_part = J.bias_part;
    const int Nf = J.Nf, IH = J.IH, IW = J.IW, OH = J.OH, OW = J.OW, R = J.R, nbands = J.nbands, FPB = J.FPB;
    int* __restrict__ const work_ctr = J.work_ctr;
    // FPB > 1 (small frames, nbands == 1): FPB frames are stacked to one band.  X rows of consecutive frames are contiguous in memory; dY is staged
    // with a pitch of VP = IH / S rows per frame, its OH real rows followed by rows that stay zero from the initial LDS fill, so that dY row v still
    // sits over X row v * S and the pixel runs that cross into the next frame multiply zeros.  R = (FPB - 1) * VP + OH virtual rows.
    using C = WgradCfg<CI, CO, KH, KW, S>;
    constexpr int NTH = NWV * 64, PF = 8192 / NTH, CTH = C::CT / (NWV / 4), CHY = CO / 8, CHX = CI / 8;   // NWV = 8 or 16 waves
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OWp = (OW + 7) & ~7, U = OWp >> 3;
    const int XR = (R - 1) * S + KH;
    const int xpix = XR * IW + 8 * S + KW;
    const int dypix = R * OWp + 8;
    lds_char* ximg = (lds_char*)smem;
    lds_char* dyimg = ximg + xpix * C::XS;
    for (int i = tid * 16; i < xpix * C::XS + dypix * C::DYS; i += NTH * 16) *(lds_u32x4*)((lds_char*)smem + i) = u32x4_t{0u, 0u, 0u, 0u};

    // ---- this thread's chunks: index ci = tid + k*512 over [dY band chunks | X band chunks]
    const bool stacked = FPB > 1;
    const int VP = IH / S;
    const int ndy = (stacked ? FPB * OH : R) * OW * CHY, nx = XR * IW * CHX, nch = ndy + nx;
    unsigned pk[PF];                               // bit 31: X chunk; bits 17..30: LDS offset / 16; bits 0..16: global element offset / 8
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int ci = min(tid + k * NTH, nch - 1);
        if (ci < ndy) {
            const int pix = ci / CHY, c = ci % CHY;
            int r = pix / OW;
            const int ow = pix % OW;
            if (stacked) r = (r / OH) * VP + r % OH;      // memory row (frame, row) -> virtual row of the stacked band
            pk[k] = ((unsigned)((xpix * C::XS + (r * OWp + ow) * C::DYS + c * 16) >> 4) << 17) | (unsigned)ci;
        } else {
            const int cx = ci - ndy;
            const int pix = cx / CHX, c = cx % CHX;
            pk[k] = 0x80000000u | ((unsigned)((pix * C::XS + c * 16) >> 4) << 17) | (unsigned)cx;
        }
    }
    const int q = wave & 3, h = wave >> 2;
    f32x4 acc[C::NTW][CTH];
#pragma unroll
    for (int j = 0; j < C::NTW; ++j)
#pragma unroll
        for (int c = 0; c < CTH; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2;
    const int ccol = (a & 3) * 8;
    // n-tile <-> wave as in conv_wgrad_dma_kernel: quarter q = (tap group tg, channel group cgq); tile j of a wave is tap tg * TPG + j, its LDS offset splits into a
    // wave part (added to the image pointer) and a j part that is the same for every wave (an immediate when IW is a compile-time constant)
    constexpr int NTG = 4 / C::CGN, TPG = KH * KW / NTG;
    static_assert(C::CGN <= 4 && 4 % C::CGN == 0 && (KH * KW) % NTG == 0 && TPG == C::NTW && (NTG == 1 || TPG % KW == 0), "n-tile assignment");
    const int IWk = IWC ? IWC : IW;
    const int cgq = q % C::CGN, tg = q / C::CGN;
    const int qoff = ((tg * TPG / KW) * IWk) * C::XS + cgq * 32;
    int toff[C::NTW];
#pragma unroll
    for (int j = 0; j < C::NTW; ++j) toff[j] = ((j / KW) * IWk + j % KW) * C::XS;
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    u32x4_t pf[PF];
    const int nitems = stacked ? (Nf + FPB - 1) / FPB : Nf * nbands;
    unsigned zmask = 0, zmask_cur = 0;
    auto prefetch = [&](int item) {
        zmask = 0;
        const int f = stacked ? item * FPB : item / nbands, oh0 = stacked ? 0 : (item % nbands) * R;
        const int nfr = stacked ? min(FPB, Nf - f) : 1;         // the last stacked band may be short: its missing frames stage as zero dY
        const h16_t* ybase = dY + ((long long)f * OH + oh0) * OW * CO;
        const h16_t* xbase = X + ((long long)f * IH + oh0 * S) * IW * CI;
        const int yrows = stacked ? nfr * OH : min(R, OH - oh0), xrows = stacked ? min(XR, nfr * IH) : min(XR, IH - oh0 * S);
        const int ylim = yrows * OW * CHY - 1, xlim = xrows * IW * CHX - 1;   // last in-frame chunk
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const bool isx = (pk[k] >> 31) != 0;
            const int go = (int)(pk[k] & 0x1ffffu);
            const h16_t* src = isx ? xbase + (long long)min(go, xlim) * 8 : ybase + (long long)min(go, ylim) * 8;
            pf[k] = *reinterpret_cast<const u32x4_t*>(src);           // value untouched here: no wait at the issue point
            if (!isx && go > ylim) zmask |= 1u << k;                  // dY rows below the frame become zeros at the LDS write
        }
    };
    __shared__ int s_next[2];
    int item = bid, iter = 0;
    if (item < nitems) prefetch(item);
    while (item < nitems) {
        if (work_ctr && tid == 0) s_next[iter & 1] = nwg + atomicAdd(work_ctr, 1);   // dynamic claim (see ConvTileP::work_ctr)
        __syncthreads();                               // previous band fully consumed (first pass: zero fill visible)
        zmask_cur = zmask;
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            if (tid + k * NTH < nch) {
                const u32x4_t v = ((zmask_cur >> k) & 1u) ? u32x4_t{0u, 0u, 0u, 0u} : pf[k];
                if (!(pk[k] >> 31)) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { bsum[2 * e] += h2f_lo(v[e]); bsum[2 * e + 1] += h2f_hi(v[e]); }
                }
                *(lds_u32x4*)((lds_char*)smem + (((pk[k] >> 17) & 0x3fffu) << 4)) = v;
            }
        }
        __syncthreads();
        item = work_ctr ? s_next[iter & 1] : item + nwg;
        ++iter;
        if (item < nitems) prefetch(item);             // in flight during the MFMAs below
        const int units = R * U;
        // k <-> pixel assignment of a 32-pixel step (4 runs of 8): k = g*8 + e; e < 4 (first tr-read): run g>>1, pixel (g&1)*4 + e;
        // e >= 4 (second tr-read): run 2 + (g>>1), pixel (g&1)*4 + e - 4.  A 32-lane half of one read then covers 8 consecutive
        // pixels of ONE run -> conflict-free with the pitches of WgradCfg.
        const int px = (g & 1) * 4 + prow;
        // run u = u0 + hh * 2 + (g >> 1) of the band = (row r, 8-pixel run uo of the row).  Its dY pixel is 8 u (OWp = 8 U); its X pixel offset follows
        // (r, uo) by adds: + step4 per step, + wrapd whenever uo passes U.  (A runtime u / U and u % U per run and step were ~100 VALU instructions
        // next to the step's 18 MFMAs: conv2 / conv3 weight gradients 372 -> 340 us per step.)
        const int q4 = 4 / U, r4 = 4 - q4 * U;
        const int step4 = (q4 * S * IW + r4 * 8 * S) * C::XS, wrapd = (S * IW - U * 8 * S) * C::XS;
        int uo[2], pbv[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int u = hh * 2 + (g >> 1), r = u / U;
            uo[hh] = u - r * U;
            pbv[hh] = ((r * S) * IW + (uo[hh] * 8 + px) * S) * C::XS + ccol;
        }
        const int abase = px * C::DYS + ccol + h * CTH * 32, pb_idle = (px * S) * C::XS + ccol;
#pragma unroll 1
        for (int u0 = 0; u0 < units; u0 += 4) {
            lds_char* ab[2];
            int pb[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int u = u0 + hh * 2 + (g >> 1);
                const bool valid = u < units;
                ab[hh] = dyimg + (valid ? u * 8 : R * OWp) * C::DYS + abase;      // idle runs read the permanent zero pixels
                pb[hh] = valid ? pbv[hh] : pb_idle;
                pbv[hh] += step4; uo[hh] += r4;
                if (uo[hh] >= U) { uo[hh] -= U; pbv[hh] += wrapd; }
            }
            auto bfrag = [&](int j) { return tr_read8(ximg + qoff + pb[0] + toff[j], ximg + qoff + pb[1] + toff[j]); };
            // B fragments run D n-tiles ahead of their MFMAs; A fragments first
            h16x8_t ring[D];
            h16x8_t af[CTH];
#pragma unroll
            for (int c = 0; c < CTH; ++c) af[c] = tr_read8(ab[0] + c * 32, ab[1] + c * 32);
#pragma unroll
            for (int j = 0; j < D && j < C::NTW; ++j) ring[j] = bfrag(j);
            __builtin_amdgcn_sched_barrier(0);          // keep the reads this far ahead: the scheduler otherwise sinks them next to their use
#pragma unroll
            for (int j = 0; j < C::NTW; ++j) {
                const h16x8_t bf = ring[j % D];
#pragma unroll
                for (int c = 0; c < CTH; ++c) acc[j][c] = MFMA_16x16x32_H(af[c], bf, acc[j][c], 0, 0, 0);
                if (j + D < C::NTW) ring[j % D] = bfrag(j + D);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    constexpr int KC = KH * KW * CI;
    float* out = part + (long long)bid * CO * KC;
#pragma unroll
    for (int j = 0; j < C::NTW; ++j)
#pragma unroll
        for (int c = 0; c < CTH; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long long)((h * CTH + c) * 16 + g * 4 + r) * KC + ((tg * TPG + j) * C::CGN + cgq) * 16 + a] = acc[j][c][r];
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < CO) {
        const int cgrp = tid >> 3, e = tid & 7;
        float s = 0.f;
        for (int t = cgrp; t < NTH; t += CHY) s += red[t * 8 + e];
        if (bias_part) unsafeAtomicAdd(bias_part + tid, s);
    }
}
template <int CI, int CO, int KH, int KW, int S, int NWV, int D = 3, int IWC = 0>
__global__ void __launch_bounds__(NWV * 64) conv_wgrad_tr8_kernel(const h16_t* __restrict__ X, const h16_t* __restrict__ dY, float* __restrict__ part,
                                                            float* __restrict__ bias_part, int Nf, int IH, int IW, int OH, int OW, int R, int nbands,
                                                            int* __restrict__ work_ctr, int FPB) {
    const WgradJob J{X, dY, part, bias_part, nullptr, Nf, IH, IW, OH, OW, R, nbands, work_ctr, FPB};
    conv_wgrad_tr8_body<CI, CO, KH, KW, S, NWV, D, IWC>(J, (int)blockIdx.x, (int)gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// v3 (round 4): the v2 multiply loop fed by LDS-DMA into TWO band buffers.
//   v2 stages a band through 16 prefetch registers per thread and a commit phase (ds_write_b128 + the bias sums), behind two barriers per band;
//   measured on 2048 static-camera frames (rocprofv3): whole kernel 129 / 137 us (conv3 / conv2), without the MFMA loop 71 / 96,
//   without the global loads 101 / 100, with neither 37 / 42 — per band: 2.5 us of commit + barriers, ~3.5 us of load latency that the MFMA loop of
//   ONE resident band cannot cover (the next band's registers are only free after the commit), ~8 us of multiply loop.
//   Here a band = X rows + dY rows of R output rows as ONE contiguous LDS image (same pitches, same tr-read fragments as v2), filled by
//   global_load_lds_dwordx4 in 1 KB pieces (8 waves x 64 lanes x 16 B; a lane decodes its 16-byte slot -> (pixel, chunk) -> global address; pad
//   slots, dY columns >= OW, rows beyond the frame and the trailing zero pixels come from a zero page), the NEXT band's DMA is issued right after the
//   band barrier into the other buffer and lands under the multiply loop; no staging registers (64 VGPRs back), no commit, ONE barrier per band.  The
//   bias gradient (column sums of dY) is read back from LDS (3 x 16 B per thread and band).  Bands are smaller (two must fit: R = 7 rows for
//   conv3, 6 for conv2), which costs 6 - 11 % more multiply steps (partially filled last step of a band).
// Static-camera shapes only; small frames keep v2's stacked bands.
// ---------------------------------------------------------------------------------------------------------------------
// One LDS-DMA piece (64 lanes x 16 B -> 1 KB at the wave-uniform LDS address `dst`), issued as inline assembly.  Reason: the tr-read builtin
// (ds_read_b64_tr_b16) carries no memory operand, so LLVM's waitcnt pass must assume it may read what a pending
// __builtin_amdgcn_global_load_lds is still writing and puts `s_waitcnt vmcnt(0)` in front of the first tr-read after the DMA — the multiply
// loop then waits for the whole next band (measured: whole = DMA + MFMA exactly).  Hidden from the pass, the DMA is ordered by this kernel's
// own `s_waitcnt vmcnt(0)` + barrier only.  (Compiler-inserted vmcnt waits stay safe: unknown extra operations can only make them wait longer.)
DEVI void wg_lds_dma16(const void* src, lds_char* dst) {
    const unsigned a = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)dst);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(src), "s"(a) : "memory", "m0");
}
template <int CI, int CO, int KH, int KW, int S, int IWC = 0>      // IWC: the image width at compile time (0: run time) — the tap offsets of the B fragments become ds_read immediates
DEVI void conv_wgrad_dma_body(const WgradJob& J, const int bid, const int nwg) {
    const h16_t* __restrict__ const X = J.X; const h16_t* __restrict__ const dY = J.dY; float* __restrict__ const part = J.part; float* __restrict__ const bias_part = J.bias_part;
    const h16_t* __restrict__ const zeros = J.zeros;
    const int Nf = J.Nf, IH = J.IH, IW = J.IW, OH = J.OH, OW = J.OW, R = J.R, nbands = J.nbands;
    int* __restrict__ const work_ctr = J.work_ctr;
    using C = WgradCfg<CI, CO, KH, KW, S>;
    constexpr int NWV = 8, NTH = NWV * 64, CTH = C::CT / (NWV / 4), CHY = CO / 8, CHX = CI / 8, XSS = C::XS / 16, YSS = C::DYS / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OWp = (OW + 7) & ~7, U = OWp >> 3;
    const int XR = (R - 1) * S + KH;
    const int xpix = XR * IW + 8 * S + KW;
    const int dypix = R * OWp + 8;
    const int xslots = xpix * XSS, yslots = dypix * YSS;
    const int bbytes = ((xslots + yslots) * 16 + 1023) & ~1023;      // one band buffer: [X image | dY image], whole 1 KB DMA pieces
    const int npieces = bbytes >> 10;
    lds_char* const lbase = (lds_char*)smem;
    const int nitems = Nf * nbands;
    const float invXSS = 1.f / (float)XSS, invYSS = 1.f / (float)YSS, invIW = 1.f / (float)IW, invOWp = 1.f / (float)OWp, invOW = 1.f / (float)OW;
    // a lane's slot of piece k is the same (pixel, chunk) in every band: decoded ONCE into pk[k] — bit 31: X image, bit 30: a real chunk of a
    // pixel that can lie inside the frame, bits 24..29: its band row, bits 0..23: element offset / 8 from the band's first row — so that issuing a
    // band costs a handful of VALU operations per piece (decoding per band made the issue phase 1.6 us of a 4.3 us band)
    constexpr int PFM = 10;
    unsigned pk[PFM];
#pragma unroll
    for (int k = 0; k < PFM; ++k) {
        int q = (k * NWV + wave) * 64 + lane;
        unsigned v = 0;
        if (q < xslots) {
            const int px = wg_fdiv(q, invXSS), ch = q - px * XSS;
            const int r = wg_fdiv(px, invIW), c = px - r * IW;
            if (ch < CHX && r < XR) v = 0xC0000000u | ((unsigned)r << 24) | (unsigned)(((r * IW + c) * CI + ch * 8) >> 3);
        } else {
            q -= xslots;
            const int px = wg_fdiv(q, invYSS), ch = q - px * YSS;
            const int r = wg_fdiv(px, invOWp), c = px - r * OWp;
            if (ch < CHY && r < R && c < OW) v = 0x40000000u | ((unsigned)r << 24) | (unsigned)(((r * OW + c) * CO + ch * 8) >> 3);
        }
        pk[k] = v;
    }
    auto dma = [&](int item, int buf) {
        const int f = item / nbands, oh0 = (item - f * nbands) * R, ih0 = oh0 * S;
        const int yrows = min(R, OH - oh0), xrows = min(XR, IH - ih0);
        const h16_t* xsrc = X + ((long long)f * IH + ih0) * IW * CI;
        const h16_t* ysrc = dY + ((long long)f * OH + oh0) * OW * CO;
        lds_char* dst = lbase + buf * bbytes + wave * 1024;
#pragma unroll
        for (int k = 0; k < PFM; ++k) {
            if (k * NWV + wave >= npieces) break;                     // wave-uniform
            const unsigned v = pk[k];
            const bool isx = (v >> 31) != 0;
            const int r = (int)((v >> 24) & 63u);
            const bool ok = ((v >> 30) & 1u) && r < (isx ? xrows : yrows);
            const h16_t* src = ok ? (isx ? xsrc : ysrc) + (long long)(v & 0xffffffu) * 8 : zeros;
            wg_lds_dma16(src, dst + k * NWV * 1024);
        }
    };
    const int q = wave & 3, h = wave >> 2;
    f32x4 acc[C::NTW][CTH];
#pragma unroll
    for (int j = 0; j < C::NTW; ++j)
#pragma unroll
        for (int c = 0; c < CTH; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2;
    const int ccol = (a & 3) * 8;
    // n-tile <-> wave (round 5): wave quarter q owns channel group q % CGN of the taps [tg * TPG, (tg + 1) * TPG), tg = q / CGN — its n-tile j is tap tg * TPG + j.
    // The LDS offset of tile j is then (wave part) + (j part): ((tg * TPG / KW) * IW) * XS + cgq * 32 goes into the band's base pointer once, and
    // ((j / KW) * IW + j % KW) * XS is the same for every wave — an immediate of the ds_read when IW is a compile-time constant (IWC): 18 VALU adds per multiply step
    // and wave gone.  (Before: tiles q * NTW .. + NTW - 1 in (tap, channel group) order: a different offset list per wave, added with VALU.)
    constexpr int NTG = 4 / C::CGN, TPG = KH * KW / NTG;
    static_assert(C::CGN <= 4 && 4 % C::CGN == 0 && (KH * KW) % NTG == 0 && TPG == C::NTW && (NTG == 1 || TPG % KW == 0), "n-tile assignment");
    const int IWk = IWC ? IWC : IW;
    const int cgq = q % C::CGN, tg = q / C::CGN;
    const int qoff = ((tg * TPG / KW) * IWk) * C::XS + cgq * 32;          // this wave's part of every B-fragment offset
    int toff[C::NTW];
#pragma unroll
    for (int j = 0; j < C::NTW; ++j) toff[j] = ((j / KW) * IWk + j % KW) * C::XS;
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    __shared__ int s_next[2];
    int item = bid, iter = 0, nb = 0;
    if (item < nitems) dma(item, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int px = (g & 1) * 4 + prow;
    const int q4 = 4 / U, r4 = 4 - q4 * U;
    const int step4 = (q4 * S * IW + r4 * 8 * S) * C::XS, wrapd = (S * IW - U * 8 * S) * C::XS;
    while (item < nitems) {
        if (work_ctr && tid == 0) s_next[iter & 1] = nwg + atomicAdd(work_ctr, 1);   // dynamic claim (see ConvTileP::work_ctr)
        __syncthreads();                               // this band has landed (every wave waited for its own pieces) and nobody reads the other buffer any more
        const int cur = item;
        item = work_ctr ? s_next[iter & 1] : item + nwg;
        ++iter;
        lds_char* const ximg0 = lbase + nb * bbytes;
        lds_char* const dyimg = ximg0 + xslots * 16;
        lds_char* const ximg = ximg0 + qoff;              // B fragments only
        nb ^= 1;
        // the next band streams in under the bias sums and the MFMAs below.  Waves 0-3 issue their pieces now, waves 4-7 (the second wave of each
        // SIMD) after their first multiply step, so that one wave per SIMD multiplies while the other spends its issue time
        bool pend = item < nitems;
        if (pend && wave < 4) { dma(item, nb); pend = false; }
        {                                              // bias gradient: column sums of the band's real dY pixels, from LDS
            const int f = cur / nbands, oh0 = (cur - f * nbands) * R;
            const int nchunk = min(R, OH - oh0) * OW * CHY;
            for (int i = tid; i < nchunk; i += NTH) {  // i % CHY == tid % CHY: a thread keeps one channel group
                const int pix = i / CHY, r = wg_fdiv(pix, invOW), c = pix - r * OW;
                const u32x4_t v = *(lds_u32x4*)(dyimg + (r * OWp + c) * C::DYS + (tid % CHY) * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) { bsum[2 * e] += h2f_lo(v[e]); bsum[2 * e + 1] += h2f_hi(v[e]); }
            }
        }
        const int units = R * U;
        int uo[2], pbv[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int u = hh * 2 + (g >> 1), r = u / U;
            uo[hh] = u - r * U;
            pbv[hh] = ((r * S) * IW + (uo[hh] * 8 + px) * S) * C::XS + ccol;
        }
        const int abase = px * C::DYS + ccol + h * CTH * 32, pb_idle = (px * S) * C::XS + ccol;
        // (measured and not kept: all fragments of step s + 1 requested before the MFMAs of step s, two register sets — 94 vs 97 us for the multiply
        //  phase alone, 239 VGPRs; and with ONE B-fragment read per step instead of nine the phase still takes 94 us: the loop is not waiting on LDS)
        auto mstep = [&](const int u0) {
            lds_char* ab[2];
            int pb[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int u = u0 + hh * 2 + (g >> 1);
                const bool valid = u < units;
                ab[hh] = dyimg + (valid ? u * 8 : R * OWp) * C::DYS + abase;      // idle runs read the zero pixels behind the band
                pb[hh] = valid ? pbv[hh] : pb_idle;
                pbv[hh] += step4; uo[hh] += r4;
                if (uo[hh] >= U) { uo[hh] -= U; pbv[hh] += wrapd; }
            }
            auto bfrag = [&](int j) { return tr_read8(ximg + pb[0] + toff[j], ximg + pb[1] + toff[j]); };
            constexpr int D = 3;
            h16x8_t ring[D];
            h16x8_t af[CTH];
#pragma unroll
            for (int c = 0; c < CTH; ++c) af[c] = tr_read8(ab[0] + c * 32, ab[1] + c * 32);
#pragma unroll
            for (int j = 0; j < D && j < C::NTW; ++j) ring[j] = bfrag(j);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < C::NTW; ++j) {
                const h16x8_t bf = ring[j % D];
#pragma unroll
                for (int c = 0; c < CTH; ++c) acc[j][c] = MFMA_16x16x32_H(af[c], bf, acc[j][c], 0, 0, 0);
                if (j + D < C::NTW) ring[j % D] = bfrag(j + D);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (units > 0) mstep(0);                       // first step peeled: the second wave of a SIMD issues its DMA pieces behind it, and the loop body stays free of that code
        if (pend) { dma(item, nb); pend = false; }
#pragma unroll 1
        for (int u0 = 4; u0 < units; u0 += 4) mstep(u0);
        if (pend) dma(item, nb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of the next band have landed
    }
    constexpr int KC = KH * KW * CI;
    float* out = part + (long long)bid * CO * KC;
#pragma unroll
    for (int j = 0; j < C::NTW; ++j)
#pragma unroll
        for (int c = 0; c < CTH; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long long)((h * CTH + c) * 16 + g * 4 + r) * KC + ((tg * TPG + j) * C::CGN + cgq) * 16 + a] = acc[j][c][r];
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < CO) {
        const int cgrp = tid >> 3, e = tid & 7;
        float s = 0.f;
        for (int t = cgrp; t < NTH; t += CHY) s += red[t * 8 + e];
        if (bias_part) unsafeAtomicAdd(bias_part + tid, s);
    }
}
template <int CI, int CO, int KH, int KW, int S, int IWC = 0>
__global__ void __launch_bounds__(512) conv_wgrad_dma_kernel(const h16_t* __restrict__ X, const h16_t* __restrict__ dY, float* __restrict__ part,
                                                             float* __restrict__ bias_part, const h16_t* __restrict__ zeros, int Nf, int IH, int IW, int OH, int OW,
                                                             int R, int nbands, int* __restrict__ work_ctr) {
    const WgradJob J{X, dY, part, bias_part, zeros, Nf, IH, IW, OH, OW, R, nbands, work_ctr, 1};
    conv_wgrad_dma_body<CI, CO, KH, KW, S, IWC>(J, (int)blockIdx.x, (int)gridDim.x);
}
// The weight gradient of one stage for BOTH cameras in one launch: the static camera's job on the LDS-DMA body (IWS = its map width), the gripper camera's on the
// stacked-band body (IWG).  A workgroup belongs to one job for its life: blockIdx.x < wgA -> job A.  Neither multiply loop changes; both bodies are 512 threads.
template <int CI, int CO, int KH, int KW, int S, int IWS, int IWG>
__global__ void __launch_bounds__(512) conv_wgrad_pair_kernel(WgradJob A, WgradJob B, int wgA) {
    if ((int)blockIdx.x < wgA) conv_wgrad_dma_body<CI, CO, KH, KW, S, IWS>(A, (int)blockIdx.x, wgA);
    else conv_wgrad_tr8_body<CI, CO, KH, KW, S, 8, 3, IWG>(B, (int)blockIdx.x - wgA, (int)gridDim.x - wgA);
}
// band height for v3: among the heights of which two bands fit the LDS, the one with the fewest multiply steps per frame — a band of r rows is
// ceil(r U / 4) steps of four 8-pixel runs (U = OWp / 8 runs per row; a partially filled last step multiplies zeros) plus about one step's worth of
// barrier / issue overhead.  conv3 (21 rows, U = 3): 8 + 8 + 5 rows = 6 + 6 + 4 steps; conv2 (23 rows): 6 + 6 + 6 + 5.  0 = shape not covered
template <int CI, int CO, int KH, int KW, int S>
static inline int conv_wgrad_dma_rows(int IH, int IW, int OH, int OW, int* nbands_out, size_t* lds_out) {
    using C = WgradCfg<CI, CO, KH, KW, S>;
    const int OWp = (OW + 7) / 8 * 8, U = OWp / 8;
    int bestR = 0, bestc = 1 << 30;
    for (int R = OH; R >= 1; --R) {
        const int XR = (R - 1) * S + KH;
        const size_t band = (((size_t)(XR * IW + 8 * S + KW) * C::XS + (size_t)(R * OWp + 8) * C::DYS) + 1023) / 1024 * 1024;
        const size_t lds = std::max<size_t>(2 * band, 512 * 8 * sizeof(float));
        if (lds > 160 * 1024 - 128 || band > 80 * 1024 || R > 63) continue;      // <= 10 pieces per wave (pk[] in registers), 6 bits of band row in pk
        const int nb = (OH + R - 1) / R, last = OH - (nb - 1) * R;
        const int cost = (nb - 1) * ((R * U + 3) / 4 + 1) + (last * U + 3) / 4 + 1;
        if (cost < bestc) { bestc = cost; bestR = R; *nbands_out = nb; *lds_out = lds; }
    }
    return bestR;
}

// the map widths of the two cameras at conv3 / conv2 (200 x 200 and 84 x 84 frames): the compile-time-width instances of the kernels
template <int CI, int KH> struct WgradCamW {
    static constexpr int fixed = (CI == 64 && KH == 3) ? 1 : ((CI == 32 && KH == 4) ? 2 : 0);
    static constexpr int stat = fixed == 1 ? 23 : (fixed == 2 ? 49 : 0), gripper = fixed == 1 ? 9 : (fixed == 2 ? 20 : 0);
};
// band / stack geometry of the stacked-band kernel (conv_wgrad_tr8_kernel) for a job that runs on `wgs` workgroups; false = shape not covered
template <int CI, int CO, int KH, int KW, int S>
static inline bool conv_wgrad_tr8_plan(int Nf, int IH, int IW, int OH, int OW, int wgs, int& R_out, int& nb_out, int& fpb_out, size_t& lds_out) {
    using C = WgradCfg<CI, CO, KH, KW, S>;
    constexpr int NWV = 8;
    // fewest balanced bands whose chunks fit the 16 x 512 prefetch slots and whose images fit in 160 KB (16 KB kept for the bias reduction)
    for (int nb = 1; nb <= OH; ++nb) {
        int R = (OH + nb - 1) / nb, XR = (R - 1) * S + KH;
        long long chunks = (long long)R * OW * (CO / 8) + (long long)XR * IW * (CI / 8);
        size_t lds = std::max<size_t>(C::lds_bytes(R, IW, OW), NWV * 64 * 8 * sizeof(float));
        if (chunks > 16 * 512 || lds > 160 * 1024 - 64 || (long long)XR * IW * CI >= (1 << 20)) continue;
        // small frames (whole frame per band): stack FPB frames to a band — the two barriers, the staging and the exposed load latency of a band
        // (~5 us, against ~0.5 us of MFMAs for a 7x7 gripper map) are then paid once per FPB frames.  Largest FPB that fits LDS and the prefetch
        // slots and still leaves every workgroup OF THIS JOB two bands (the second one's loads fly under the first one's MFMAs).
        int fpb = 1;
        if (nb == 1 && IH % S == 0) {
            for (int f = 2; f <= 16; ++f) {
                const int Rf = (f - 1) * (IH / S) + OH, XRf = (Rf - 1) * S + KH;
                const long long ch = (long long)f * OH * OW * (CO / 8) + (long long)XRf * IW * (CI / 8);
                const size_t l = std::max<size_t>(C::lds_bytes(Rf, IW, OW), NWV * 64 * 8 * sizeof(float));
                if (ch > 16 * 512 || l > 160 * 1024 - 64 || (long long)XRf * IW * CI >= (1 << 20)) break;
                if ((Nf + f - 1) / f < 2 * wgs) break;
                fpb = f; R = Rf; XR = XRf; chunks = ch; lds = l;
            }
        }
        R_out = R; nb_out = nb; fpb_out = fpb; lds_out = lds;
        return true;
    }
    return false;
}

// band plan of the LDS-DMA body (conv_wgrad_dma_body) for job J: frames large enough that v2 would not stack them (>= 2 bands of multiply work per frame), at least
// min_nf of them, element offsets inside 31 bits.  Fills J.R / nbands / FPB and the launch's dynamic LDS bytes; false (J untouched) = the job does not run on that body
template <int CI, int CO, int KH, int KW, int S>
static inline bool conv_wgrad_dma_plan(WgradJob& J, int min_nf, size_t& lds) {
    if (!J.zeros || J.OH * J.OW < 256 || J.Nf < min_nf || (long long)J.Nf * J.IH * J.IW * CI >= (1ll << 31)) return false;
    int nb = 0;
    const int R = conv_wgrad_dma_rows<CI, CO, KH, KW, S>(J.IH, J.IW, J.OH, J.OW, &nb, &lds);
    if (R <= 0) return false;
    J.R = R; J.nbands = nb; J.FPB = 1;
    return true;
}

// One job as one launch.  The caller fills J's operands, geometry, part, bias_part, work_ctr and zeros (null: never the LDS-DMA body); R / nbands / FPB are planned
// here.  Returns the number of partial slabs written (= workgroups)
template <int CI, int CO, int KH, int KW, int S>
static inline int launch_conv_wgrad_tr(hipStream_t st, WgradJob J, int max_blocks) {
    using C = WgradCfg<CI, CO, KH, KW, S>;
    size_t lds = 0;
    // v3 (LDS-DMA, two band buffers)
    if (conv_wgrad_dma_plan<CI, CO, KH, KW, S>(J, 2, lds)) {
        constexpr int IWS = WgradCamW<CI, KH>::stat;      // the static camera's maps (200 x 200 frames): conv3 reads 23 x 23, conv2 49 x 49
        const int grid = std::min(std::min(J.Nf * J.nbands, 256), max_blocks);
        if (IWS && J.IW == IWS) {
            max_dyn_lds_once<&conv_wgrad_dma_kernel<CI, CO, KH, KW, S, IWS>>(160 * 1024 - 64);
            hipLaunchKernelGGL((conv_wgrad_dma_kernel<CI, CO, KH, KW, S, IWS>), dim3(grid), dim3(512), lds, st, J.X, J.dY, J.part, J.bias_part, J.zeros, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, J.nbands, J.work_ctr);
        } else {
            max_dyn_lds_once<&conv_wgrad_dma_kernel<CI, CO, KH, KW, S, 0>>(160 * 1024 - 64);
            hipLaunchKernelGGL((conv_wgrad_dma_kernel<CI, CO, KH, KW, S, 0>), dim3(grid), dim3(512), lds, st, J.X, J.dY, J.part, J.bias_part, J.zeros, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, J.nbands, J.work_ctr);
        }
        return grid;
    }
    constexpr int NWV = 8;                                   // 16 waves (one co-tile each, 4 waves per SIMD) measured slower: 0.43 vs 0.40 ms/step
    if (conv_wgrad_tr8_plan<CI, CO, KH, KW, S>(J.Nf, J.IH, J.IW, J.OH, J.OW, std::min(256, max_blocks), J.R, J.nbands, J.FPB, lds)) {
        const int items = J.FPB > 1 ? (J.Nf + J.FPB - 1) / J.FPB : J.Nf * J.nbands;
        const int grid = std::min(std::min(items, 256), max_blocks);
        // the gripper camera's maps (84 x 84 frames): conv3 reads 9 x 9, conv2 20 x 20 — the compile-time-width instance (tap offsets as ds_read immediates)
        constexpr int IWG = WgradCamW<CI, KH>::gripper;
        if (IWG && J.IW == IWG) {
            max_dyn_lds_once<&conv_wgrad_tr8_kernel<CI, CO, KH, KW, S, NWV, 3, IWG>>(160 * 1024 - 64);
            hipLaunchKernelGGL((conv_wgrad_tr8_kernel<CI, CO, KH, KW, S, NWV, 3, IWG>), dim3(grid), dim3(NWV * 64), lds, st, J.X, J.dY, J.part, J.bias_part, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, J.nbands, J.work_ctr, J.FPB);
        } else {
            max_dyn_lds_once<&conv_wgrad_tr8_kernel<CI, CO, KH, KW, S, NWV>>(160 * 1024 - 64);
            hipLaunchKernelGGL((conv_wgrad_tr8_kernel<CI, CO, KH, KW, S, NWV>), dim3(grid), dim3(NWV * 64), lds, st, J.X, J.dY, J.part, J.bias_part, J.Nf, J.IH, J.IW, J.OH, J.OW, J.R, J.nbands, J.work_ctr, J.FPB);
        }
        return grid;
    }
    int R = J.OH;                                            // largest band that keeps two workgroups per CU (<= 78 KB)
    while (R > 1 && C::lds_bytes(R, J.IW, J.OW) > 78 * 1024) --R;
    const int nbands = (J.OH + R - 1) / R;
    R = (J.OH + nbands - 1) / nbands;                        // balanced (no short tail band)
    lds = C::lds_bytes(R, J.IW, J.OW);
    const int grid = J.Nf < max_blocks ? J.Nf : max_blocks;
    max_dyn_lds_once<&conv_wgrad_tr_kernel<CI, CO, KH, KW, S>>(160 * 1024);
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<CI, CO, KH, KW, S>), dim3(grid), dim3(256), lds, st, J.X, J.dY, J.part, J.bias_part, J.Nf, J.IH, J.IW, J.OH, J.OW, R);
    return grid;                                             // = number of partial slabs written
}

// Both cameras' weight gradient of conv3 or conv2 as ONE launch (conv_wgrad_pair_kernel): A = the static camera's job (LDS-DMA body), B = the gripper camera's
// (stacked-band body, its stack sized for its own workgroups).  The launch's min(256, max_blocks) workgroups are divided by camera_split over the jobs' multiply
// steps (bands x (steps of four 8-pixel runs + 1), the cost model of conv_wgrad_dma_rows); wg != nullptr: the two counts as given (tests).  A.part = the slab area:
// A's slabs first, B's right behind them (B.part is set here).  Returns false (nothing launched) for shapes that are not the two cameras' maps; ns = slabs per job.
template <int CI, int CO, int KH, int KW, int S>
static inline bool launch_conv_wgrad_pair(hipStream_t st, WgradJob A, WgradJob B, int max_blocks, const int* wg, int ns[2]) {
    using W = WgradCamW<CI, KH>;
    if constexpr (W::fixed == 0) return false;
    else {
        constexpr int IWS = W::stat, IWG = W::gripper;
        if (A.IW != IWS || A.IH != IWS || B.IW != IWG || B.IH != IWG || B.Nf < 1) return false;
        size_t ldsA = 0;
        if (!conv_wgrad_dma_plan<CI, CO, KH, KW, S>(A, 1, ldsA)) return false;
        const int nbA = A.nbands;
        const int grid = std::min(256, max_blocks);
        if (grid < 2) return false;
        auto steps = [](int rows, int OW) { return (rows * ((OW + 7) / 8) + 3) / 4 + 1; };
        const int itemsA = A.Nf * nbA;
        const double wA = (double)A.Nf * ((nbA - 1) * steps(A.R, A.OW) + steps(A.OH - (nbA - 1) * A.R, A.OW));
        size_t ldsB = 0; int itemsB = 0;
        auto planB = [&](int wgs) {
            if (!conv_wgrad_tr8_plan<CI, CO, KH, KW, S>(B.Nf, B.IH, B.IW, B.OH, B.OW, wgs, B.R, B.nbands, B.FPB, ldsB)) return false;
            itemsB = B.FPB > 1 ? (B.Nf + B.FPB - 1) / B.FPB : B.Nf * B.nbands;
            return true;
        };
        int nA, nB;
        if (wg) { nA = std::max(wg[0], 1); nB = std::max(wg[1], 1); if (!planB(nB)) return false; }
        else {
            if (!planB(grid)) return false;
            if (itemsA + itemsB <= grid) { nA = itemsA; nB = itemsB; }      // (small calls) one item per workgroup, as in two launches
            else {
                camera_split(grid, wA, (double)itemsB * steps(B.R, B.OW), nA, nB);
                if (nA > itemsA) { nB = std::min(itemsB, nB + nA - itemsA); nA = itemsA; }
                if (nB > itemsB) { nA = std::min(itemsA, nA + nB - itemsB); nB = itemsB; }
                if (!planB(nB)) return false;
            }
        }
        nA = std::min(nA, itemsA); nB = std::min(nB, itemsB);
        B.part = A.part + (long long)nA * CO * (KH * KW * CI);
        max_dyn_lds_once<&conv_wgrad_pair_kernel<CI, CO, KH, KW, S, IWS, IWG>>(160 * 1024 - 64);
        hipLaunchKernelGGL((conv_wgrad_pair_kernel<CI, CO, KH, KW, S, IWS, IWG>), dim3(nA + nB), dim3(512), std::max(ldsA, ldsB), st, A, B, nA);
        ns[0] = nA; ns[1] = nB;
        return true;
    }
}

}  // namespace HULC_NS
