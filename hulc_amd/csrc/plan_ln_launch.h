// hulc_amd/csrc/plan_ln_launch.h — the launch decisions of the LayerNorm family and of the plan scatter as free functions of the stream (and, for the fp32
// LayerNorm backward, the column-sum scratch), so that the engine (engine.h ln_fwd / ln_bwd, engine_backward.inc) and the per-kernel test entries
// (k_entries.h) run the same arithmetic: block shape and rows per block of the fused backward, the row split of the fp32 pair, w4 over lds for the scatter.
#pragma once
#include <algorithm>
#include <type_traits>
#include "kernels.h"

namespace HULC_NS {

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

template <typename T>
inline void launch_ln_fwd(hipStream_t st, const float* x, long long ldx, int rows, int n, const float* g, const float* b, T* out, long long ldo, float* outf,
                          long long ldf, float* stats) {
    hipLaunchKernelGGL((layernorm_fwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, st, x, ldx, rows, n, g, b, out, ldo, outf, ldf, stats);
}
// the fused backward serves the 16-bit types only; its broadcast / partial-sum forms of dy exist nowhere else
template <typename T> constexpr bool ln_bwd_fused() { return std::is_same<T, h16_t>::value; }
inline int ln_bwd_rows_per_block(int rows) { return rows >= 1024 ? 16 : 4; }          // fused: 16 rows and 16 waves per block from 1024 rows on
inline int ln_bwd_nsplit(int rows) { return std::max(1, std::min(64, cdiv(rows, 64))); }          // fp32 pair: row chunks of the parameter gradients
inline long long ln_bwd_scratch_floats(int rows, int n) { return 2ll * ln_bwd_nsplit(rows) * n; }          // [2][nsplit][n] partial sums (fp32 pair only)
// bcast_rows > 0 (fused kernel only): dy holds one row per WINDOW, broadcast over its bcast_rows rows and divided by bcast_div
template <typename T>
inline void launch_ln_bwd(hipStream_t st, float* scratch, const float* dy, long long lddy, const float* x, long long ldx, const float* stats, const float* g, int rows,
                          int n, float* dxf, long long ldd, int acc, T* dxt, long long ldt, float* dg, float* db, float drop_p = 0.f, unsigned long long drop_seed = 0,
                          int bcast_rows = 0, float bcast_div = 1.f, int dy_parts = 1, long long dy_part_stride = 0, bool fixed_order = false) {
    if constexpr (ln_bwd_fused<T>()) {
        const int rpb = ln_bwd_rows_per_block(rows);
        const int nblk = cdiv(rows, rpb);
        // fixed_order (reproducible mode): the blocks store their gamma / beta partials in `scratch` ([2][nblk][n]) and the fp32 pair's second stage adds them in block order
        const bool slab = fixed_order && dg && nblk > 1;
        hipLaunchKernelGGL((layernorm_bwd_fused_kernel<T>), dim3(nblk), dim3(rpb == 16 ? 1024 : 256), 0, st, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, dxt, ldt,
                           drop_p, drop_seed, rpb, dg, db, bcast_rows, bcast_div, dy_parts, dy_part_stride, slab ? scratch : (float*)nullptr);
        if (slab) {
            hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch, nblk, n, dg, (float*)nullptr, 1.f);
            hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch + (long long)nblk * n, nblk, n, db, (float*)nullptr, 1.f);
        }
    } else {        // fp32 (parity) mode: unfused and deterministic
        if ((drop_p > 0.f || drop_seed != 0) && dxt && dxf) {       // dx first, its copy through the dropout mask in a second launch
            hipLaunchKernelGGL((layernorm_bwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, st, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, (T*)nullptr, 0);
            hipLaunchKernelGGL((dropout_apply_kernel<T>), dim3(cdiv((long long)rows * n, 256)), dim3(256), 0, st, dxf, (float*)nullptr, dxt, (long long)rows * n, drop_p, drop_seed);
        } else
            hipLaunchKernelGGL((layernorm_bwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, st, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, dxt, ldt);
        const int nsplit = ln_bwd_nsplit(rows);
        hipLaunchKernelGGL(layernorm_param_grad_kernel, dim3(cdiv(n, 64), nsplit), dim3(256), 0, st, dy, lddy, x, ldx, stats, rows, n, cdiv(rows, nsplit), scratch, (float*)nullptr, (float*)nullptr);
        hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch, nsplit, n, dg, (float*)nullptr, 1.f);
        hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(n, 64)), dim3(256), 0, st, scratch + (long long)nsplit * n, nsplit, n, db, (float*)nullptr, 1.f);
    }
}

// 16-bit engines: four waves per tile (and stores into a fresh buffer); the fp32 engine keeps the serial sum order.  Both kernels hold NCLS <= 32 rows in LDS.
template <typename T> inline bool plan_scatter_w4(int NCLS) { return !std::is_same<T, float>::value && NCLS <= 32; }
template <typename T>
inline void launch_plan_scatter_grad(hipStream_t st, bool w4, const T* dC, const int* idx, int B, int NCAT, int NCLS, int H, int KIN, float* dw, int store) {
    if (w4) hipLaunchKernelGGL((plan_scatter_grad_w4_kernel<T>), dim3(NCAT, cdiv(H, 64)), dim3(256), 0, st, dC, idx, B, NCAT, NCLS, H, KIN, dw, store);
    else hipLaunchKernelGGL((plan_scatter_grad_lds_kernel<T>), dim3(NCAT, cdiv(H, 64)), dim3(64), 0, st, dC, idx, B, NCAT, NCLS, H, KIN, dw);
}

}  // namespace HULC_NS
