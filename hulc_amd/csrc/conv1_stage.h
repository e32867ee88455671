// hulc_amd/csrc/conv1_stage.h — conv1's input side, shared by its forward (conv_tile.h) and its weight gradient (conv1_wgrad.h): the frame source (Conv1Src: fp32
// NCHW, uint8 NHWC, frame store), raw-row pitches, the 16-byte window conversion of uint8 4-pixel groups and its interior groups, the band staging into a 16-bit
// [c][row][iw] LDS image, the folded bias and the fp32 materialisation of the uint8 transform.
#pragma once
#include "lds_types.h"

namespace HULC_NS {

// ---------------------------------------------------------------------------------------------------------------------
// conv1 input band staging, shared by conv1_fwd_kernel and conv1_wgrad_tr_kernel: rows [ih0, ih0+rows) of frame f as a bf16
// [c][row][iw] LDS image.  Two boundary formats:
//   * fp32 NCHW frames already transformed by the reference's dataloader (hulc.py:395-414) — the reference boundary;
//   * uint8 (.., H, W, C) frames straight from the dataset: ScaleImageTensor (x/255), Normalize(0.5, 0.5)
//     and RandomShiftsAug (hulc/utils/transforms.py:8-29: replicate-pad by `pad`, one integer shift per frame; the bilinear
//     grid_sample lands on pixel centres, i.e. out[y][x] = in[clamp(y + sy - pad)][clamp(x + sx - pad)]) are fused into this load —
//     4x fewer input bytes and no fp32 copy of the frames ever exists.
// ---------------------------------------------------------------------------------------------------------------------
#define CONV1_RAW_MARGIN 16          // replicated edge pixels each side of a raw uint8 row (>= the largest RandomShiftsAug pad; 48 bytes)
static inline __host__ __device__ int conv1_raw_pitch16(int IW) { return (((IW + 2 * CONV1_RAW_MARGIN) * 3 + 8 + 7) & ~7) + 15 & ~15; }   // the same rounded to the LDS-DMA path's 16-byte slots
static inline __host__ __device__ int conv1_raw_pitch(int IW) { return ((IW + 2 * CONV1_RAW_MARGIN) * 3 + 8 + 7) & ~7; }   // bytes per raw row (+8: the 16-byte read window)
struct Conv1Src {
    const void* X;         // fp32 NCHW (u8 == 0) or uint8 NHWC (u8 == 1)
    const int* shift;      // u8 only: [Nf][2] = (sx, sy) in [0, 2*pad], or null (no augmentation)
    int u8, pad;
    // fold (round 5; u8 only, 16-bit engines): the affine x = u (2/255) - 1 of ScaleImageTensor + Normalize is taken OUT of the data path.
    // conv1 has no zero padding (RandomShiftsAug pads by replication), so  conv(W, x) + b = (2/255) conv(W, u) + (b - sum_k W[.,k])  and
    // dW = dY * x = (2/255) (dY * u) - db (x) 1:  the MFMA operand is the EXACT 16-bit value of the byte (0..255 are representable: one v_cvt_f32_ubyteN
    // per value instead of extract + convert + fma, and no rounding of the input at all), the scale and the folded bias move into the fp32 epilogue
    // (bias = bias_fold, computed by conv1_bias_fold_kernel from the 16-bit weights), the weight-gradient kernels scale their slab and subtract their
    // own bias partial before they write it.  fold == 0: the value x itself is staged (round 2 - 4).
    int fold;
    // frame store (round 6; u8 only): X is not this batch's (Nf,H,W,C) frames but a device-resident STORE of nstore frames (whole episodes), and the
    // batch's frame f = window f / S, step f % S lives at store index wstart[f / S] + f % S — conv1's forward and weight gradient GATHER their bands by index,
    // no (B,S,H,W,C) tensor is materialised and nothing crosses PCIe per step (include/hulc_hip.h hulc_batch::window_start).  A start outside [0, nstore - S]
    // is clamped (never an out-of-bounds read); shift[] stays indexed by the batch frame f.
    const long long* wstart = nullptr;
    int S = 1;
    long long nstore = 0;
    DEVI long long frame(int f) const {
        if (!wstart) return f;
        const int b = f / S;
        const long long s0 = min(max(wstart[b], 0ll), nstore - (long long)S);
        return s0 + (f - b * S);
    }
    DEVI long long frames_total(int Nf) const { return wstart ? nstore : (long long)Nf; }
    // frame f's RandomShiftsAug offsets (dx, dy) = shift - pad; a column shift outside the contract's [0, 2 pad] is clamped (every uint8 kernel, forward and backward alike: the
    // staged replicate margins / the interior groups of the register kernels assume |dx| <= pad); rows are clamped per row, any dy is safe
    DEVI void offsets(int f, int& dx, int& dy) const {
        dx = dy = 0;
        if (shift) { dx = min(max(shift[2 * f] - pad, -pad), pad); dy = shift[2 * f + 1] - pad; }
    }
};
#define CONV1_FOLD_SCALE (2.f / 255.f)
// bias_fold[o] = b[o] - sum_k W16[o][k] over the packed 16-bit conv1 weights [32][192] (what the MFMAs multiply); one wave per output channel
__global__ void __launch_bounds__(64) conv1_bias_fold_kernel(const h16_t* __restrict__ W, const float* __restrict__ b, float* __restrict__ out) {
    const int o = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int k = lane; k < 192; k += 64) s += h2f(W[o * 192 + k]);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) out[o] = b[o] - s;
}
DEVI float u8_to_unit(unsigned char b) { return ((float)b / 255.f - 0.5f) / 0.5f; }    // ScaleImageTensor then Normalize(mean .5, std .5)
// element e = tid + m*256 of a [rows][n] grid, m = 0, 1, ...: (row, col) advanced incrementally — a runtime integer division per
// element (~35 VALU instructions) made the staging VALU-bound (one division per load AND per store, 3 channels, every band)
struct RowCol { int r, c; };
struct Step256 {
    int n, dq, dr;
    DEVI explicit Step256(int n_) : n(n_), dq(256 / n_), dr(256 % n_) {}
    DEVI void adv(RowCol& p) const { p.c += dr; p.r += dq; if (p.c >= n) { p.c -= n; ++p.r; } }
};
// ---- uint8 frames converted FROM REGISTERS (round 6): a 4-pixel group (12 bytes of an interleaved RGB row at a shift-dependent byte offset) is fetched as the aligned
// 16-byte WINDOW around it — conv1_window_off gives the window's byte offset in the source row, clamped so that it stays inside the row (the frame buffer's last row
// included) — and conv1_window_group turns the window into the group's three 4-value planes: window -> the 12 bytes of source pixels qp .. qp + 3 -> for output pixel k
// the source pixel clamp(c 4 + k + dx, 0, IW - 1) - qp (= k everywhere but at the row ends, where RandomShiftsAug's replicate pad repeats the edge pixel).
DEVI int conv1_window_off(int c, int dx, int IW, int RB) {
    const int qp = min(max(c * 4 + dx, 0), IW - 4);
    return min((qp * 3) & ~3, RB - 16);
}
template <bool FOLD>
DEVI void conv1_window_group(const u32x4_t& w, int c, int dx, int IW, int RB, unsigned (&lo)[3], unsigned (&hi)[3]) {
    const float sc = 2.f / 255.f, of = -1.f;
    const int p0 = c * 4 + dx, qp = min(max(p0, 0), IW - 4);
    const int a0 = min((qp * 3) & ~3, RB - 16), sh = qp * 3 - a0;      // 0 .. 4
    const bool s4 = sh == 4;
    const unsigned w0 = s4 ? w[1] : w[0], w1 = s4 ? w[2] : w[1], w2 = s4 ? w[3] : w[2], w3 = w[3];
    const unsigned d0 = __builtin_amdgcn_alignbyte(w1, w0, sh & 3), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh & 3), d2 = __builtin_amdgcn_alignbyte(w3, w2, sh & 3);
    const unsigned P[4] = {d0, __builtin_amdgcn_alignbyte(d1, d0, 3), __builtin_amdgcn_alignbyte(d2, d1, 2), d2 >> 8};      // the four source pixels as 24-bit words
    float v[12];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int si = min(max(p0 + kk, 0), IW - 1) - qp;       // 0 .. 3
        const unsigned pw = si == 0 ? P[0] : (si == 1 ? P[1] : (si == 2 ? P[2] : P[3]));
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { const float x = (float)((pw >> (8 * ch)) & 0xffu); v[kk * 3 + ch] = FOLD ? x : fmaf(x, sc, of); }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { lo[ch] = pack2h(v[ch], v[3 + ch]); hi[ch] = pack2h(v[6 + ch], v[9 + ch]); }
}
// The same for a group that no shift can push against a row end (conv1_interior_groups): source pixel k of the group is pixel qp + k, qp = 4 c + dx, the window starts at
// (3 qp) & ~3 and the group's 12 bytes at offset sh = (3 qp) & 3 = (3 dx) & 3 of it — ONE value per frame.  3 alignbyte + 12 byte conversions + 6 packs against the ~ 80
// instructions of the clamps and per-pixel selects above (the conversion was VALU-bound: profiles/r06_conv1_wgrad_probe.txt).
template <bool FOLD>
DEVI void conv1_window_group_interior(const u32x4_t& w, int sh, unsigned (&lo)[3], unsigned (&hi)[3]) {
    const float sc = 2.f / 255.f, of = -1.f;
    const unsigned d[3] = {__builtin_amdgcn_alignbyte(w[1], w[0], sh), __builtin_amdgcn_alignbyte(w[2], w[1], sh), __builtin_amdgcn_alignbyte(w[3], w[2], sh)};
    float v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { const float x = (float)((d[i >> 2] >> (8 * (i & 3))) & 0xffu); v[i] = FOLD ? x : fmaf(x, sc, of); }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { lo[ch] = pack2h(v[ch], v[3 + ch]); hi[ch] = pack2h(v[6 + ch], v[9 + ch]); }
}
// groups [cl, cl + wi) of a row's IW / 4 are interior for every shift |dx| <= pad: 4 c - pad >= 0 and 4 c + pad <= IW - 6 (all four pixels inside the row, the window
// not clamped at the row's last 16 bytes); at most `cap` of them, centred.  wi <= 0: no interior (tiny frames).
static inline __host__ __device__ void conv1_interior_groups(int IW, int pad, int cap, int& cl, int& wi) {
    const int lo = (pad + 3) >> 2, hi = (IW - 6 - pad) >= 0 ? (IW - 6 - pad) / 4 + 1 : 0;      // [lo, hi)
    wi = hi - lo < cap ? hi - lo : cap;
    cl = wi > 0 ? lo + (hi - lo - wi) / 2 : 0;
    if (wi < 0) wi = 0;
}
template <bool REGCONV = false>      // compile-time: the window path must not sit (as dead code with live registers) inside the 128-VGPR fp32 forward kernel — it cost that kernel 16 more spills
DEVI void conv1_stage_band(const Conv1Src& s, int f, int ih0, int rows, int IH, int IW, lds_char* ximg, int XR, int XRS, int tid, lds_char* raw) {
    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
    const int W4 = IW >> 2;                                           // 4-pixel groups per row
    const Step256 sq(W4);
    const RowCol q0{tid / W4, tid % W4};
    if (!s.u8) {
        // all three channel planes of the band in ONE pass: element e of the [3][rows][W4] grid of 16-byte quads, NU quads in flight per thread.
        // (A pass per channel had ~3 useful loads in flight per thread for a 16-row band — its other unrolled slots re-read a clamped element —
        // and exposed the load latency three times per band.)
        const float* X = reinterpret_cast<const float*>(s.X);
        const float* src0 = X + ((long long)f * 3 * IH + ih0) * IW;
        const int per = rows * W4, tot = 3 * per;
        const float inv_per = 1.f / (float)per, inv_w4 = 1.f / (float)W4;
        constexpr int NU = 6;       // conv1_fwd_kernel<4> runs at 128 VGPRs next to 48 registers of weight fragments: 10 in flight spilled 38
        for (int e0 = tid; e0 < tot; e0 += 256 * NU) {
            float4 v[NU];
            int pk[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int e = min(e0 + u * 256, tot - 1);
                const int c = (int)(((float)e + 0.5f) * inv_per), rem = e - c * per;
                const int r = (int)(((float)rem + 0.5f) * inv_w4), q4 = rem - r * W4;
                pk[u] = (c << 20) | (r << 8) | q4;
                v[u] = *reinterpret_cast<const float4*>(src0 + ((long long)c * IH + r) * IW + q4 * 4);
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (e0 + u * 256 < tot) {
                    const int c = pk[u] >> 20, r = (pk[u] >> 8) & 0xfff, q4 = pk[u] & 0xff;
                    u32x2_t o;
                    o[0] = pack2h(v[u].x, v[u].y);
                    o[1] = pack2h(v[u].z, v[u].w);
                    *(__attribute__((address_space(3))) u32x2_t*)(ximg + (c * XR + r) * XRS + q4 * 8) = o;
                }
            }
        }
        return;
    }
    // uint8: (A) the band's source rows (row clamp of the replicate pad applied) are copied with 8- or 4-byte loads into `raw`, each
    // row behind a margin of CONV1_RAW_MARGIN replicated edge pixels — byte-wide global loads cost a full wave instruction per
    // 64 bytes and made a first version as slow as the 4x larger fp32 path; (B) a 4-pixel group is 12 contiguous bytes of a raw row
    // at a (shift-dependent) unaligned offset: four aligned LDS dwords, v_alignbyte, v_cvt_f32_ubyteN, one FMA per value
    // (b * 2/255 - 1: within one fp32 ulp of the reference's (b/255 - .5)/.5, which the fp32-mode ingest_u8_kernel keeps exactly).
    const unsigned char* base = reinterpret_cast<const unsigned char*>(s.X) + s.frame(f) * IH * IW * 3;
    int dx = 0, dy = 0;
    s.offsets(f, dx, dy);
    const int RB = IW * 3;                                            // bytes per source row (multiple of 4: IW % 4 == 0)
    if constexpr (REGCONV) {
        // one pass: NU windows in flight per thread, converted from the registers into the [c][row][iw] image (no raw rows in LDS, no margins, no barrier in between)
        constexpr int NU = 6;
        // interior groups first (conv1_interior_groups: no clamp, no per-pixel select, one alignbyte shift per frame — see conv1_wgrad_tr2r_kernel), then the row ends
        int cl, WI;
        conv1_interior_groups(IW, s.pad, W4, cl, WI);
        if (WI > 0 && dx >= -s.pad && dx <= s.pad) {
            const Step256 si(WI);
            const int shu = (3 * dx) & 3, off0 = 12 * cl + 3 * dx;
            RowCol p{tid / WI, tid % WI};
            while (p.r < rows) {
                RowCol e[NU];
                u32x4_t w[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    e[u] = p; si.adv(p);
                    const bool in = e[u].r < rows;
                    w[u] = *reinterpret_cast<const u32x4_t*>(base + (long long)min(max(ih0 + (in ? e[u].r : rows - 1) + dy, 0), IH - 1) * RB + ((off0 + 12 * (in ? e[u].c : 0)) & ~3));
                }
#pragma unroll
                for (int u = 0; u < NU; ++u)
                    if (e[u].r < rows) {
                        unsigned lo[3], hi[3];
                        if (s.fold) conv1_window_group_interior<true>(w[u], shu, lo, hi); else conv1_window_group_interior<false>(w[u], shu, lo, hi);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) *(__attribute__((address_space(3))) u32x2_t*)(ximg + (ch * XR + e[u].r) * XRS + (cl + e[u].c) * 8) = u32x2_t{lo[ch], hi[ch]};
                    }
            }
            const int WE = W4 - WI;
            for (int i = tid; i < rows * WE; i += 256) {
                const int r = i / WE, ce = i - r * WE, c = ce < cl ? ce : ce + WI;
                const u32x4_t w = *reinterpret_cast<const u32x4_t*>(base + (long long)min(max(ih0 + r + dy, 0), IH - 1) * RB + conv1_window_off(c, dx, IW, RB));
                unsigned lo[3], hi[3];
                if (s.fold) conv1_window_group<true>(w, c, dx, IW, RB, lo, hi); else conv1_window_group<false>(w, c, dx, IW, RB, lo, hi);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) *(__attribute__((address_space(3))) u32x2_t*)(ximg + (ch * XR + r) * XRS + c * 8) = u32x2_t{lo[ch], hi[ch]};
            }
            return;
        }
        RowCol p = q0;
        while (p.r < rows) {
            RowCol e[NU];
            u32x4_t w[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                e[u] = p; sq.adv(p);
                const bool in = e[u].r < rows;
                w[u] = *reinterpret_cast<const u32x4_t*>(base + (long long)min(max(ih0 + (in ? e[u].r : rows - 1) + dy, 0), IH - 1) * RB + conv1_window_off(in ? e[u].c : 0, dx, IW, RB));
            }
#pragma unroll
            for (int u = 0; u < NU; ++u)
                if (e[u].r < rows) {
                    unsigned lo[3], hi[3];
                    if (s.fold) conv1_window_group<true>(w[u], e[u].c, dx, IW, RB, lo, hi); else conv1_window_group<false>(w[u], e[u].c, dx, IW, RB, lo, hi);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) *(__attribute__((address_space(3))) u32x2_t*)(ximg + (ch * XR + e[u].r) * XRS + e[u].c * 8) = u32x2_t{lo[ch], hi[ch]};
                }
        }
        return;
    }
    const int RP = conv1_raw_pitch(IW);
    constexpr int LM = CONV1_RAW_MARGIN * 3;                          // byte offset of pixel 0 in a raw row (multiple of 8)
    if ((RB & 7) == 0 && ((uintptr_t)base & 7) == 0) {
        typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));
        constexpr int NU = 10;                                        // the whole band in one round of loads per thread
        const int n8 = RB >> 3;
        const Step256 s8(n8);
        RowCol p{tid / n8, tid % n8};
        while (p.r < rows) {
            RowCol e[NU];
            u32x2v v[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                e[u] = p; s8.adv(p);
                const bool in = e[u].r < rows;
                v[u] = *reinterpret_cast<const u32x2v*>(base + (long long)min(max(ih0 + (in ? e[u].r : rows - 1) + dy, 0), IH - 1) * RB + (in ? e[u].c : 0) * 8);
            }
#pragma unroll
            for (int u = 0; u < NU; ++u)
                if (e[u].r < rows) *(__attribute__((address_space(3))) u32x2v*)(raw + e[u].r * RP + LM + e[u].c * 8) = v[u];
        }
    } else {
        constexpr int NU = 8;
        const int n4 = RB >> 2;
        const Step256 s4(n4);
        RowCol p{tid / n4, tid % n4};
        while (p.r < rows) {
            RowCol e[NU];
            unsigned v[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                e[u] = p; s4.adv(p);
                const bool in = e[u].r < rows;
                v[u] = *reinterpret_cast<const unsigned*>(base + (long long)min(max(ih0 + (in ? e[u].r : rows - 1) + dy, 0), IH - 1) * RB + (in ? e[u].c : 0) * 4);
            }
#pragma unroll
            for (int u = 0; u < NU; ++u)
                if (e[u].r < rows) *(__attribute__((address_space(3))) unsigned*)(raw + e[u].r * RP + LM + e[u].c * 4) = v[u];
        }
    }
    if (dx != 0) {                                                    // replicate margins (F.pad(..., "replicate")): one thread per (row, side)
        for (int i = tid; i < rows * 2; i += 256) {
            const int rr = i >> 1, side = i & 1;
            const unsigned char* rp = base + (long long)min(max(ih0 + rr + dy, 0), IH - 1) * RB;
            const unsigned w = *reinterpret_cast<const unsigned*>(rp + (side ? RB - 4 : 0));
            const unsigned px = side ? (w >> 8) : (w & 0xffffffu);    // the edge pixel's 3 bytes
            lds_char* dst = raw + rr * RP + (side ? LM + RB : 0);
            for (int k = 0; k < CONV1_RAW_MARGIN; ++k) {
                dst[k * 3 + 0] = (char)(px & 0xff); dst[k * 3 + 1] = (char)((px >> 8) & 0xff); dst[k * 3 + 2] = (char)((px >> 16) & 0xff);
            }
        }
    }
    __syncthreads();
    const float sc = s.fold ? 1.f : 2.f / 255.f, of = s.fold ? 0.f : -1.f;      // fold: the exact value of the byte (Conv1Src::fold)
    for (RowCol p = q0; p.r < rows; sq.adv(p)) {
        const int o = p.r * RP + LM + (p.c * 4 + dx) * 3;             // |dx| <= pad <= CONV1_RAW_MARGIN: stays inside the margins
        const int sh = o & 3;
        const __attribute__((address_space(3))) unsigned* wp = (const __attribute__((address_space(3))) unsigned*)(raw + (o & ~3));
        const unsigned w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
        const unsigned d[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh)};
        float v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = fmaf((float)((d[k >> 2] >> (8 * (k & 3))) & 0xffu), sc, of);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u32x2_t ov;
            ov[0] = pack2h(v[c], v[3 + c]);
            ov[1] = pack2h(v[6 + c], v[9 + c]);
            *(__attribute__((address_space(3))) u32x2_t*)(ximg + (c * XR + p.r) * XRS + p.c * 8) = ov;
        }
    }
}
// the same transform materialised as fp32 NCHW frames (fp32 parity mode, tests): out[f][c][y][x]
__global__ void ingest_u8_kernel(const unsigned char* __restrict__ in, const int* __restrict__ shift, int pad, int Nf, int IH, int IW, float* __restrict__ out, Conv1Src src = Conv1Src{}) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)Nf * 3 * IH * IW) return;
    const int x = (int)(idx % IW), y = (int)((idx / IW) % IH), c = (int)((idx / ((long long)IW * IH)) % 3), f = (int)(idx / ((long long)3 * IW * IH));
    int dx = 0, dy = 0;
    if (shift) { dx = min(max(shift[2 * f] - pad, -pad), pad); dy = shift[2 * f + 1] - pad; }      // as Conv1Src::offsets
    const int sy = min(max(y + dy, 0), IH - 1), sx = min(max(x + dx, 0), IW - 1);
    out[idx] = u8_to_unit(in[((src.frame(f) * IH + sy) * IW + sx) * 3 + c]);       // src: only its frame-store fields are used (frame(f) = f without a store)
}

}  // namespace HULC_NS
