// hulc_amd/csrc/repro_sites.h — the audited launch sites whose summation order depends on scheduling ("Reproducible mode").  One bit per site
// in hulc_get_option "nondeterministic_sites": the HOST launch code sets it whenever it issues a float-atomic form with two or more contributors per
// destination, or a dynamic-claim form whose accumulator spans claims.  With hulc_set_option "reproducible" 1 no launch sets a bit.
#pragma once
enum ReproSite : unsigned {
    ND_GEMM_SPLITK = 1u << 0,        // gemm.h epi_store ep.atomic: split-K weight gradients (Engine::gemm_wgrad)
    ND_TRANSPOSE_COLSUM = 1u << 1,   // kernels.h transpose_tile64_store: bias gradients riding on the dY transpose (more than one row tile)
    ND_COLSUM_ROWS = 1u << 2,        // kernels.h colsum_kernel direct_accumulate == 2 (more than one row chunk)
    ND_CONV_UNPACK_SPLIT = 1u << 3,  // kernels.h unpack_conv_wgrad(_batched)_kernel: slab range split over grid.y
    ND_LN_PARAM = 1u << 4,           // kernels.h layernorm_bwd_fused_kernel: gamma / beta gradients (more than one workgroup)
    ND_POS_EMB = 1u << 5,            // kernels.h pr_input_bwd_kernel: position-embedding gradient (more than one window chunk)
    ND_VAL_METRICS = 1u << 6,        // kernels.h logistic_sample_kernel / det_head.h det_head_act_kernel: validation MAE / gripper metrics
    ND_TR_FFN_FWD = 1u << 7,         // tr_fused.h forward: y2 accumulated by the four hidden quarters
    ND_TR_LN_BWD = 1u << 8,          // tr_fused.h backward: norm1 / norm2 gamma / beta gradients (more than one window)
    ND_ENC_TAIL_LN = 1u << 9,        // enc_tail.h enc_tail_bwd_kernel: LayerNorm gamma / beta gradients (more than 16 frames)
    ND_CONV_BIAS = 1u << 10,         // conv_wgrad.h, conv1_wgrad.h: conv bias gradients of the weight-gradient kernels (more than one workgroup)
    ND_LIN_BWD_ROWS = 1u << 11,      // lin_bwd.h lin_bwd_smallm_body: row-split bias (and slab-less weight) gradients
    ND_CONV_CLAIM = 1u << 12,        // conv_wgrad.h, conv1_wgrad.h work_ctr: items claimed dynamically under a per-workgroup slab accumulator
};
