// hulc_amd/csrc/lin_bwd.h — weight / bias gradients of the Linear layers: the M <= 64 body (single and batched launch) and the streaming row-walking body with its
// job list (LinStreamBatch), which the engine's backward queue flushes.
#pragma once
#include "lds_types.h"

namespace HULC_NS {

// One workgroup's 64 (n) x 128 (k) fp32 tile of dW leaves the accumulators (shared by lin_bwd_smallm_body and lin_bwd_stream_body).  A wave holds two halves h of
// 16 (n) x 64 (k): half h starts at row r0[h], column c0[h] of dW and is fragments acc[4 h .. 4 h + 3], 16 columns each (lin_bwd_smallm_body: the wave's 16 rows x
// both column halves; lin_bwd_stream_body: two row groups x the wave's 64 columns).  vec_ok: whole tile inside K and 16-byte aligned -> row-shaped float4 stores through a per-wave LDS image at `smem` (the
// caller's operand images must be dead: this function starts with a barrier), added to the `oldw` quads fetched before the multiply; else per-fragment stores / atomics
DEVI void lin_bwd_tile_out(const f32x4 (&acc)[8], const float4 (&oldw)[8], const bool vec_ok, const bool atomic, const int store, float* __restrict__ dW, const long long lddw,
                           const int N, const int K, const int (&r0)[2], const int (&c0)[2], char* smem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, a = lane & 15;
    const int orow = lane >> 4, ocol = (lane & 15) * 4;
    if (vec_ok) {
        constexpr int OP = 64 * 4 + 16;                          // pitch of one row's 64 fp32 columns in the wave's image
        __syncthreads();                                         // every wave is past its last read of the operand images (and of the bias sums)
        lds_char* const tb = (lds_char*)smem + wave * (16 * OP);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) *(__attribute__((address_space(3))) f32x4*)(tb + a * OP + jj * 64 + g * 16) = acc[h * 4 + jj];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const f32x4 v = *(__attribute__((address_space(3))) f32x4*)(tb + (it * 4 + orow) * OP + ocol * 4);
                const int nr = r0[h] + it * 4 + orow;
                float4 o = oldw[h * 4 + it];
                o.x += v[0]; o.y += v[1]; o.z += v[2]; o.w += v[3];
                if (nr < N) *reinterpret_cast<float4*>(dW + (long long)nr * lddw + c0[h] + ocol) = o;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = r0[j >> 2] + a, k = c0[j >> 2] + (j & 3) * 16 + g * 4;
            if (n >= N) continue;
            float* p = dW + (long long)n * lddw + k;
            if (atomic) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k + r < K) unsafeAtomicAdd(p + r, acc[j][r]);
            } else if (k + 3 < K && ((((uintptr_t)p) & 15) == 0)) {
                // store mode (slabs are never zeroed; first backward after zero_grads): the ragged last k-tile must STORE too, not add to what lies there
                float4 o = store ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<float4*>(p);
                o.x += acc[j][0]; o.y += acc[j][1]; o.z += acc[j][2]; o.w += acc[j][3];
                *reinterpret_cast<float4*>(p) = o;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k + r < K) p[r] = store ? acc[j][r] : p[r] + acc[j][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Linear-layer backward for M <= 64 rows (every M = B MLP layer): dW[N][K] += dY^T X and db[N] += colsum(dY) in ONE launch.
// (More rows are walked 64 at a time by the one workgroup of a tile; the many-row layers run lin_bwd_stream_body below.)
// Both operands are reduction(M)-major in memory; their tiles are staged in LDS as they lie ([m][n] and [m][k]) and the MFMA
// fragments come from transposing reads, so no transposed activation copies (and no separate column-sum launches) are needed.
// Orientation: A = X fragment (rows k), B = dY fragment (cols n)  ->  a lane owns dW[n][k..k+3]: float4 read-modify-write.
// ---------------------------------------------------------------------------------------------------------------------
DEVI void lin_bwd_smallm_body(const h16_t* __restrict__ dY, long long ldy, const h16_t* __restrict__ X, long long ldx,
                              int M, int N, int K, float* __restrict__ dW, long long lddw, float* __restrict__ db,
                              float* __restrict__ db2, int store, const int bx, const int by, char* smem) {
    // store != 0: dW is known to be all zeros (first backward after hulc_zero_grads): the tile is stored instead of read, added and written
    constexpr int TN = 64, TK = 128, YS = TN * 2 + 16, XS = TK * 2 + 16;
    lds_char* yimg = (lds_char*)smem;
    lds_char* ximg = yimg + 64 * YS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = bx * TN, k0 = by * TK;
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2, ccol = (a & 3) * 8;
    // wave w: n-tile w (16 columns of dY) x 8 k-tiles
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    // the 8 dW quads this lane accumulates into are fetched NOW (single launch over M: plain read-modify-write), so their latency hides
    // under the staging / MFMA phase instead of serialising as 8 dependent load-add-store rounds at the end
    // Whole-tile output path (wave-uniform condition): the accumulators leave in ROW shape, not in fragment shape.  A fragment-shaped store puts 16
    // different dW rows on 16 adjacent lanes — 64 separate 16-byte accesses per wave instruction, 64 contiguous bytes per row; the launches that
    // write the M <= 64 Linear layers' fp32 gradients ran at ~3 TB/s that way.  Each wave turns its 16 x 128 tile through a private LDS image (the
    // operand images are dead by then) so that an instruction writes 4 rows x 256 contiguous bytes; the old values are read in the same shape.
    const bool vec_ok = (lddw & 3) == 0 && ((reinterpret_cast<uintptr_t>(dW) & 15) == 0) && k0 + TK <= K;
    const int orow = lane >> 4, ocol = (lane & 15) * 4;          // output shape: row 4 it + orow of the wave's 16, columns 64 h + ocol .. + 3
    float4 oldw[8];
    if (vec_ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int nr = n0 + wave * 16 + (j & 3) * 4 + orow;
            oldw[j] = (store || nr >= N) ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(dW + (long long)nr * lddw + k0 + (j >> 2) * 64 + ocol);
        }
    }
    // the next 64-row chunk's tiles are requested into registers before the MFMAs of the current one (2 + 4 x 16 bytes per thread)
    u32x4_t ry[2], rx[4];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * 256, m = i / (TN / 8), c = i % (TN / 8);
            h16_t v[8];
            if (m0 + m < M && n0 + c * 8 < N) load8_guard<h16_t>(dY + (long long)(m0 + m) * ldy + n0 + c * 8, N - (n0 + c * 8), v);
            else zero8<h16_t>(v);
            ry[u] = *reinterpret_cast<const u32x4_t*>(v);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = tid + u * 256, m = i / (TK / 8), c = i % (TK / 8);
            h16_t v[8];
            if (m0 + m < M && k0 + c * 8 < K) load8_guard<h16_t>(X + (long long)(m0 + m) * ldx + k0 + c * 8, K - (k0 + c * 8), v);
            else zero8<h16_t>(v);
            rx[u] = *reinterpret_cast<const u32x4_t*>(v);
        }
    };
    fetch(0);
    for (int m0 = 0; m0 < M; m0 += 64) {
        if (m0 > 0) __syncthreads();
        // stage dY[m0:m0+64][n0:n0+64] and X[m0:m0+64][k0:k0+128] (rows >= M and columns past the edge -> zeros)
#pragma unroll
        for (int u = 0; u < 2; ++u) { const int i = tid + u * 256; *(lds_u32x4*)(yimg + (i / (TN / 8)) * YS + (i % (TN / 8)) * 16) = ry[u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = tid + u * 256; *(lds_u32x4*)(ximg + (i / (TK / 8)) * XS + (i % (TK / 8)) * 16) = rx[u]; }
        __syncthreads();
        if (m0 + 64 < M) fetch(m0 + 64);
#pragma unroll
        for (int ms = 0; ms < 2; ++ms) {                        // reduction over m: 2 x 32
            const int mrow = ms * 32 + g * 8 + prow;
            lds_char* yb = yimg + mrow * YS + wave * 32 + ccol;
            const h16x8_t yf = tr_read8(yb, yb + 4 * YS);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lds_char* xb = ximg + mrow * XS + j * 32 + ccol;
                const h16x8_t xf = tr_read8(xb, xb + 4 * XS);
                acc[j] = MFMA_16x16x32_H(xf, yf, acc[j], 0, 0, 0);   // D[row = k][col = n]
            }
        }
        if (db && by == 0) {                                    // column sums of dY: wave w adds rows 16 w .. 16 w + 15 of column `lane`
#pragma unroll 16
            for (int m = 0; m < 16; ++m) bsum += h2f(*(__attribute__((address_space(3))) h16_t*)(yimg + (wave * 16 + m) * YS + lane * 2));
        }
    }
    if (db && by == 0) {                                        // the four waves' partial column sums meet in LDS (the tiles are dead)
        __syncthreads();
        *(__attribute__((address_space(3))) float*)(yimg + (wave * 64 + lane) * 4) = bsum;
        __syncthreads();
        if (tid < TN) {
            bsum = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) bsum += *(__attribute__((address_space(3))) float*)(yimg + (w * 64 + tid) * 4);
        }
    }
    const int r0[2] = {n0 + wave * 16, n0 + wave * 16}, c0[2] = {k0, k0 + 64};
    lin_bwd_tile_out(acc, oldw, vec_ok, false, store, dW, lddw, N, K, r0, c0, smem);
    if (db && by == 0 && tid < TN && n0 + tid < N) { db[n0 + tid] += bsum; if (db2) db2[n0 + tid] += bsum; }
}

constexpr int LBS_LDS = 64 * (64 * 2 + 16) + 64 * (128 * 2 + 16);
__global__ void __launch_bounds__(256) lin_bwd_smallm_kernel(const h16_t* __restrict__ dY, long long ldy, const h16_t* __restrict__ X, long long ldx,
                                                             int M, int N, int K, float* __restrict__ dW, long long lddw, float* __restrict__ db,
                                                             float* __restrict__ db2, int store = 0) {
    __shared__ __attribute__((aligned(16))) char smem[LBS_LDS];
    lin_bwd_smallm_body(dY, ldy, X, ldx, M, N, K, dW, lddw, db, db2, store, blockIdx.x, blockIdx.y, smem);
}
// the weight / bias gradients of up to LBS_MAX_JOBS M <= 64 Linear layers in ONE launch (the layers of the MLPs' backward: each was a ~9 us launch
// behind its own data-gradient GEMM); problem = the one whose block range holds blockIdx.x.  store: per job, as lin_bwd_smallm_body takes it
struct LinBwdJob { const h16_t* dY; const h16_t* X; float* dW; float* db; long long ldx, lddw; int M, N, K, nx, blk0, store; };
constexpr int LBS_MAX_JOBS = 32;
struct LinBwdBatch { LinBwdJob j[LBS_MAX_JOBS]; int n; };
__global__ void __launch_bounds__(256) lin_bwd_smallm_batched_kernel(LinBwdBatch bt) {
    __shared__ __attribute__((aligned(16))) char smem[LBS_LDS];
    int k = 0;
    while (k + 1 < bt.n && (int)blockIdx.x >= bt.j[k + 1].blk0) ++k;
    const LinBwdJob J = bt.j[k];
    const int b = blockIdx.x - J.blk0;
    lin_bwd_smallm_body(J.dY, (long long)J.N, J.X, J.ldx, J.M, J.N, J.K, J.dW, J.lddw, J.db, nullptr, J.store, b % J.nx, b / J.nx, smem);
}

// ---------------------------------------------------------------------------------------------------------------------
// The same product for MANY rows (token-major layers: M = B S): a workgroup owns one 64 (n) x 128 (k) tile of dW and WALKS a long row range [mbeg, mend) in
// 64-row steps.  lin_bwd_smallm_body's one-deep pipeline (register prefetch, two __syncthreads and an LDS commit per step) exposes the global-load latency on every
// step, so its launches split the rows into 256-row chunks over many short-lived workgroups, each writing a full fp32 slab that a second launch reads back.  Here the
// row steps arrive by LDS-DMA (lds_dma16, common.h) in a ring of LBT_NST stages: LBT_NST - 2 steps in flight while another is multiplied, counted vmcnt, ONE barrier
// per step, as gemm_glds_body does along K.  (Depth: three and six stages ran the benchmark's launches in the same time, 34.4 and 35.5 us,
// profiles/lin_wgrad_flush.txt — a row step costs ~1 us per workgroup either way — so the ring stays at three: 72 KB, two workgroups per CU.)  With the rows of a job in one or two ranges the slabs (and the launch that sums them) go away.
//   * stage = dY rows [64][128 B] + X rows [64][256 B], unpadded (a DMA instruction writes 1 KB linearly: lane i at base + 16 i).  Wave w fills dY rows 16 w .. 16 w + 15
//     (two pieces of 8 rows) and X rows 16 w .. 16 w + 15 (four pieces of 4 rows): 6 DMA instructions per wave and stage.
//   * the transposing fragment reads stay conflict-free through a swizzle of the 16-byte slots on the SOURCE side: a 32-lane half of ds_read_b64_tr_b16 reads rows
//     {p, p + 8} x 32 B (p = 0 .. 3); slot = chunk ^ sw(row) sends those eight rows to eight different 32-byte bank windows (lbt_swx / lbt_swy).
//   * edges: a 16-byte chunk that is not wholly inside the matrix (rows >= mend, columns >= N / K) is fetched from a 16-byte ZERO page instead, so every slot of the
//     stage is rewritten by every step (never stale); the valid elements of a chunk that straddles the column edge (N or K not a multiple of 8) are patched into the
//     zero slot by the lane that fetched it, behind its own vmcnt wait and before the step's barrier.  Rows start 8-byte aligned (N, ldx multiples of 4: lin_stream_ok).
//   * output as in lin_bwd_smallm_body (lin_bwd_tile_out): store / read-add-write of the tile, or atomics when several row ranges share dW without slabs; the column
//     sums of dY (bias gradient) are taken from the staged rows by the k-tile-0 workgroups.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LBT_NST = 3, LBT_YB = 64 * 128, LBT_STAGE = LBT_YB + 64 * 256, LBT_LDS = LBT_NST * LBT_STAGE;
__device__ __attribute__((aligned(16))) unsigned int lbt_zero16[4] = {0u, 0u, 0u, 0u};
DEVI int lbt_swy(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }      // dY rows are 128 B: rows r, r + 1 already lie in different halves of the 64 banks
DEVI int lbt_swx(int row) { return ((row & 7) << 1) ^ (row & 8); }
DEVI void lin_bwd_stream_body(const h16_t* __restrict__ dY, long long ldy, const h16_t* __restrict__ X, long long ldx, const int mbeg, const int mend, const int N, const int K,
                              float* __restrict__ dW, long long lddw, float* __restrict__ db, const int store, const bool atomic, const bool atomic_b, const int bx, const int by,
                              char* smem) {
    lds_char* const ring = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = bx * 64, k0 = by * 128;
    const int g = lane >> 4, a = lane & 15;
    const int prow = a >> 2, ccol = (a & 3) * 8;
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const bool vec_ok = !atomic && (lddw & 3) == 0 && ((reinterpret_cast<uintptr_t>(dW) & 15) == 0) && k0 + 128 <= K;
    const int orow = lane >> 4, ocol = (lane & 15) * 4;
    // wave tile 32 (n) x 64 (k): two dY fragments x four X fragments per 32 rows = 12 transposing reads for 8 MFMAs (16 x 128, lin_bwd_smallm_body's, needs 18)
    const int wn = wave & 1, wk = wave >> 1;
    const int r0[2] = {n0 + wn * 32, n0 + wn * 32 + 16}, c0[2] = {k0 + wk * 64, k0 + wk * 64};
    float4 oldw[8];
    if (vec_ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int nr = r0[j >> 2] + (j & 3) * 4 + orow;
            oldw[j] = (store || nr >= N) ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(dW + (long long)nr * lddw + c0[j >> 2] + ocol);
        }
    }
    // this lane's six slots of a stage: u = 0, 1 -> dY piece 2 w + u (row 8 (2 w + u) + lane / 8, slot lane % 8); u = 2 .. 5 -> X piece 4 w + u - 2 (row 4 (4 w + u - 2) + lane / 16,
    // slot lane % 16).  src[u] = the chunk's address in row 0 of the tile's rows (advanced by m ld per step); col[u] = its first column; lim = N or K
    const h16_t* src[6];
    int srow[6], scol[6];
    unsigned full = 0, part = 0;      // bit u: the chunk lies wholly inside / straddles the column edge
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const bool y = u < 2;
        const int row = y ? (wave * 2 + u) * 8 + (lane >> 3) : (wave * 4 + u - 2) * 4 + (lane >> 4);
        const int slot = y ? (lane & 7) : (lane & 15);
        const int c = slot ^ (y ? lbt_swy(row) : lbt_swx(row));
        const int col = (y ? n0 : k0) + c * 8, lim = y ? N : K;
        srow[u] = row; scol[u] = col;
        src[u] = (y ? dY : X) + (long long)row * (y ? ldy : ldx) + col;
        if (col + 8 <= lim) full |= 1u << u;
        else if (col < lim) part |= 1u << u;
    }
    const bool any_part = __any((int)part) != 0;      // wave-uniform
    const int nk = mend > mbeg ? (mend - mbeg + 63) >> 6 : 0;
    auto issue = [&](int kt, int buf) {
        const int m0 = mbeg + kt * 64;
        lds_char* const st = ring + buf * LBT_STAGE;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const bool ok = ((full >> u) & 1u) && m0 + srow[u] < mend;
            const void* s = ok ? (const void*)(src[u] + (long long)m0 * (u < 2 ? ldy : ldx)) : (const void*)lbt_zero16;
            lds_dma16(s, (unsigned)(size_t)(st + (u < 2 ? (wave * 2 + u) * 1024 : LBT_YB + (wave * 4 + u - 2) * 1024)));
        }
    };
    // the valid elements of the chunks that straddle N / K (their slots hold the zero page's bytes: this wave's own DMA, waited for by the caller)
    auto patch = [&](int kt, int buf) {
        const int m0 = mbeg + kt * 64;
        lds_char* const st = ring + buf * LBT_STAGE;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            if (!((part >> u) & 1u) || m0 + srow[u] >= mend) continue;
            const h16_t* s = src[u] + (long long)m0 * (u < 2 ? ldy : ldx);
            lds_char* d = st + (u < 2 ? (wave * 2 + u) * 1024 : LBT_YB + (wave * 4 + u - 2) * 1024) + lane * 16;
            const int nv = (u < 2 ? N : K) - scol[u];
#pragma unroll
            for (int e = 0; e < 7; ++e)
                if (e < nv) *(__attribute__((address_space(3))) h16_t*)(d + e * 2) = s[e];
        }
    };
#pragma unroll
    for (int j = 0; j < LBT_NST - 1; ++j)
        if (j < nk) issue(j, j);
    int buf = 0;
#pragma unroll 1
    for (int kt = 0; kt < nk; ++kt) {
        // Ordering.  (1) vmcnt: a wave's DMA instructions complete in issue order, stage kt's six were issued before those of stage kt + 1 (the only younger ones, when
        // there is a stage kt + 1), so vmcnt(6) — vmcnt(0) in the last step — leaves THIS wave's share of stage kt landed (older plain loads — the oldw quads — only make the wait longer).  (2) the patch
        // writes go to slots this wave's own DMA has filled, so they cannot be overtaken by a DMA.  (3) lgkmcnt(0) + s_barrier: behind the barrier every wave's share
        // and patches of stage kt are in LDS — a wave reads only bytes that every wave's DMA has landed — and every wave has finished its fragment reads of stage
        // kt - 1 (lgkmcnt(0) retires them before it arrives), whose buffer the DMA issued right below overwrites.  Stage kt + 1's buffer is never read before the
        // barrier of step kt + 1.
        static_assert(LBT_NST == 3, "one counted wait per number of younger stages in flight: 0 or 1");
        if (nk - 1 - kt >= 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (any_part) patch(kt, buf);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + LBT_NST - 1 < nk) issue(kt + LBT_NST - 1, buf == 0 ? LBT_NST - 1 : buf - 1);
        lds_char* const yimg = ring + buf * LBT_STAGE;
        lds_char* const ximg = yimg + LBT_YB;
#pragma unroll
        for (int ms = 0; ms < 2; ++ms) {                        // reduction over m: 2 x 32
            const int mrow = ms * 32 + g * 8 + prow;            // (bit 2 clear: mrow + 4 has the same lbt_swy and lbt_swx ^ 8)
            const int sy = lbt_swy(mrow), sx = lbt_swx(mrow);
            h16x8_t yf[2], xf[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                lds_char* yb = yimg + mrow * 128 + (((wn * 4 + i * 2 + (ccol >> 4)) ^ sy) << 4) + (ccol & 15);
                yf[i] = tr_read8(yb, yb + 4 * 128);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int c = wk * 8 + jj * 2 + (ccol >> 4);
                xf[jj] = tr_read8(ximg + mrow * 256 + ((c ^ sx) << 4) + (ccol & 15), ximg + (mrow + 4) * 256 + ((c ^ sx ^ 8) << 4) + (ccol & 15));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[i * 4 + jj] = MFMA_16x16x32_H(xf[jj], yf[i], acc[i * 4 + jj], 0, 0, 0);   // D[row = k][col = n]
        }
        if (db && by == 0) {                                    // column sums of dY: wave w adds rows 16 w .. 16 w + 15 of column `lane`
#pragma unroll 16
            for (int m = 0; m < 16; ++m) {
                const int r = wave * 16 + m;
                bsum += h2f(*(__attribute__((address_space(3))) h16_t*)(yimg + r * 128 + (((lane >> 3) ^ lbt_swy(r)) << 4) + (lane & 7) * 2));
            }
        }
        buf = buf == LBT_NST - 1 ? 0 : buf + 1;
    }
    // no DMA is in flight here (the last step waited vmcnt(0); nk == 0 issued none): plain barriers from here on
    if (db && by == 0) {                                        // the four waves' partial column sums meet in LDS
        __syncthreads();
        *(__attribute__((address_space(3))) float*)(ring + (wave * 64 + lane) * 4) = bsum;
        __syncthreads();
        if (tid < 64) {
            bsum = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) bsum += *(__attribute__((address_space(3))) float*)(ring + (w * 64 + tid) * 4);
        }
    }
    lin_bwd_tile_out(acc, oldw, vec_ok, atomic, store, dW, lddw, N, K, r0, c0, smem);
    if (db && by == 0 && tid < 64 && n0 + tid < N) {
        if (atomic_b) unsafeAtomicAdd(db + n0 + tid, bsum);
        else db[n0 + tid] += bsum;
    }
}
// Up to LBT_MAX_JOBS Linear layers' weight / bias gradients in ONE launch of the streaming body.  Job j owns blocks [blk0, blk0 + tiles nsplit): block b - blk0 = z tiles + t is
// row range z (rows [z mchunk, (z + 1) mchunk), mchunk a multiple of 64) of tile t.  part != null: range z STORES its own slab part + z N K (pitch K; summed in index
// order by the caller's unpack launch — also with nsplit = 1, for gradients that are re-packed on the way); part == null: dW directly — nsplit = 1 stores (store != 0)
// or reads, adds and writes; nsplit > 1 adds with fp32 atomics.  db (may be null) is added to: plainly (nsplit = 1) or with atomics.
struct LinStreamJob { const h16_t* dY; const h16_t* X; float* dW; float* db; float* part; long long ldx, lddw; int M, N, K, nx, blk0, nsplit, mchunk, store; };
constexpr int LBT_MAX_JOBS = 32;
struct LinStreamBatch { LinStreamJob j[LBT_MAX_JOBS]; int n; };
__global__ void __launch_bounds__(256) lin_bwd_stream_kernel(LinStreamBatch bt) {
    extern __shared__ __attribute__((aligned(16))) char lbt_smem[];
    int k = 0;
    while (k + 1 < bt.n && (int)blockIdx.x >= bt.j[k + 1].blk0) ++k;
    const LinStreamJob J = bt.j[k];
    const int tiles = J.nx * ((J.K + 127) >> 7);
    const int b = blockIdx.x - J.blk0, z = b / tiles, t = b % tiles;
    const int mbeg = z * J.mchunk, mend = min(J.M, mbeg + J.mchunk);
    lin_bwd_stream_body(J.dY, (long long)J.N, J.X, J.ldx, mbeg, mend, J.N, J.K, J.part ? J.part + (long long)z * J.N * J.K : J.dW, J.part ? (long long)J.K : J.lddw, J.db,
                        J.part ? 1 : J.store, !J.part && J.nsplit > 1, J.nsplit > 1, t % J.nx, t / J.nx, lbt_smem);
}
// what the streaming body fetches by DMA: rows that start 8-byte aligned (the instruction takes 4-byte aligned sources; 8 is what the model's shapes and the tests reach)
static inline bool lin_stream_ok(const void* dY, const void* X, long long ldx, int N) { return (N & 3) == 0 && (ldx & 3) == 0 && (((uintptr_t)dY | (uintptr_t)X) & 7) == 0; }
// appends a job (rows split into nsplit ranges) and returns its number of workgroups; blocks = the batch's running block count
static inline int lin_stream_add(LinStreamBatch& bt, int& blocks, const h16_t* dY, const h16_t* X, long long ldx, int M, int N, int K, float* dW, long long lddw, float* db,
                                 float* part, int nsplit, int store) {
    LinStreamJob& J = bt.j[bt.n++];
    J.dY = dY; J.X = X; J.dW = dW; J.db = db; J.part = part; J.ldx = ldx; J.lddw = lddw; J.M = M; J.N = N; J.K = K; J.nx = (N + 63) / 64; J.blk0 = blocks;
    J.nsplit = nsplit; J.mchunk = ((M + nsplit - 1) / nsplit + 63) / 64 * 64; J.store = store;
    const int wg = J.nx * ((K + 127) / 128) * nsplit;
    blocks += wg;
    return wg;
}
static inline void launch_lin_stream(hipStream_t st, const LinStreamBatch& bt, int blocks) {
    if (bt.n < 1 || blocks < 1) return;
    max_dyn_lds_once<&lin_bwd_stream_kernel>(LBT_LDS);
    hipLaunchKernelGGL(lin_bwd_stream_kernel, dim3(blocks), dim3(256), LBT_LDS, st, bt);
}

}  // namespace HULC_NS
