// hulc_amd/csrc/engine.h — host-side orchestration of one HULC / GCBC training step on one MI355X.
// Engine<T> owns the workspace (saved activations, packed/transposed weight copies) and enqueues the kernels of
// forward+loss, backward and Adam on one HIP stream.  T = float (parity mode) or h16_t (bench mode).
// Reference call stack restated here: SURVEY.md §3.2 (hulc/models/hulc.py:390-537).
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "iengine.h"
#include "repro_sites.h"
#include "trainable_plan.h"
#include "gemm.h"
#include "kernels.h"
#include "plan_ln_launch.h"
#include "conv_wgrad.h"
#include "conv1_stage.h"
#include "window_rows.h"
#include "conv1_wgrad.h"
#include "lin_bwd.h"
#include "conv_tile.h"
#include "conv_reg.h"
#include "tr_fused.h"
#include "rnn_persist.h"
#include "enc_tail.h"
#include "rollout_step.h"
#include "aux_heads.h"
#include "aux_rows.h"
#include "det_head.h"

namespace HULC_NS {

#define HIP_CHECK_VOID(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { hulc_set_error("%s:%d %s", __FILE__, __LINE__, hipGetErrorString(e_)); } } while (0)

template <typename T>
struct Engine : IEngine {
    hulc_config cfg;
    // ---- model dims
    static constexpr int EMB = 128, VF = 64, GOAL = 32, LANG = 384, HID = 2048, NCAT = 32, NCLS = 32, NH = 8, FF = 2048,
                         FCH = 4096, NMIX = LL_NMIX;
    // per model kind: PLAN = width of the two fc_state outputs (32x32 logits; mcil: mean|var of a 256-d Normal), NDIM = mixture
    // dimensions (6 + discrete gripper head; mcil: 7, no gripper head), NHEAD = packed head columns (16-aligned), DE = decoder's slice
    // of the perceptual embedding (perceptual_emb_slice [64,128]; mcil: all 128)
    int PLAN, NDIM, NHEAD, NO, DE;
    bool mcil, gru = false;       // gru: mcil with plan_recognition.rnn_type = nn.GRU (3 gate blocks per BiRNN weight)
    int dec_plan, KIN;
    int maxB, maxS, maxN;
    // ---- bound flat buffers
    float *P = nullptr, *G = nullptr, *AM = nullptr, *AV = nullptr;
    int64_t numel = 0;
    struct Ref { int64_t off, n; };
    std::map<std::string, Ref> tab;
    // ---- arena
    std::vector<void*> allocs;
    int64_t ws_bytes = 0;
    struct Named { void* p; int64_t n; int kind; };   // kind 0: f32, 1: T, 2: int32
    std::map<std::string, Named> named;

    template <typename U> U* alloc(int64_t n, const char* name = nullptr, int kind = -1) {
        void* p = nullptr;
        int64_t bytes = ((n * (int64_t)sizeof(U) + 255) / 256) * 256 + 256;
        if (hipMalloc(&p, bytes) != hipSuccess) { alloc_failed = true; return nullptr; }
        hipMemsetAsync(p, 0, bytes, st);
        allocs.push_back(p);
        ws_bytes += bytes; alloc_sz[p] = bytes;
        if (name) named[name] = Named{p, n, kind >= 0 ? kind : (std::is_same<U, float>::value ? 0 : (std::is_same<U, int>::value ? 2 : 1))};
        return (U*)p;
    }
    bool alloc_failed = false;
    std::map<void*, int64_t> alloc_sz;      // bytes of every block of the arena (release() gives a block back)

    // ---- weights
    struct LinW {
        const float* W32 = nullptr; const float* b32 = nullptr; float* dW = nullptr; float* db = nullptr;
        T* W = nullptr; T* Wt = nullptr; int N = 0, K = 0; bool own_w = false;
        T* Wfr = nullptr; T* Wtfr = nullptr;      // fragment-ordered copies of W / Wt (add_frag; gemm.h: frag_pack_kernel)
    };
    struct ConvW {
        const float* W32 = nullptr; const float* b32 = nullptr; float* dW = nullptr; float* db = nullptr;
        T* Wf = nullptr; T* Wd = nullptr; int O = 0, I = 0, KH = 0, KW = 0, S = 0; int nhwc = 0;   // nhwc: packed (kh,kw,ci) order (conv2/3)
    };
    struct EncW { ConvW c1, c2, c3; LinW fc7, fc1, fc2; const float *lng = nullptr, *lnb = nullptr; float *dlng = nullptr, *dlnb = nullptr; bool gripper = false; int IH = 0; int H1 = 0, H2 = 0, H3 = 0; };
    EncW encS, encG;
    LinW pp[5], vg[3], lg[3], tr_in[2], tr_out[2], tr_l1[2], tr_l2[2], pr_fc, pr_fs, whh0, wih1, whh1, cl_im0, cl_im2, cl_la0, cl_la2;
    // mcil plan recognition (plan_recognition_net.py:14-42): 2-layer bidirectional tanh RNN; [layer][direction]
    LinW bw_ih[2][2], bw_hh[2][2];
    const float *bb_ih[2][2], *bb_hh[2][2]; float *dbb_ih[2][2], *dbb_hh[2][2];
    T* gcarB2 = nullptr;      // second direct-path buffer of the paired BiGRU BPTT
    T *bZ0[2] = {nullptr, nullptr}, *bH0[2], *bZ1, *bH1, *bh1b, *bxcat, *bdx, *bdH0[2], *bdZ0[2], *bdZ1, *bdz1b, *plan_t;
    float *plan_f, *plan_eps, *plan_eps_in, *klel;
    // GRU variant: per recurrence c (0: layer 0 fwd, 1: layer 0 reverse, 2: layer 1 fwd; 3: the single evaluated step of layer 1 reverse)
    struct GruBuf { T *Zx, *H, *R, *Z, *N, *GN, *dZx, *dG; } gb[4];
    float* gGf = nullptr; T *gcarA = nullptr, *gcarB = nullptr;
    const float *ln_vg_g, *ln_vg_b, *ln_lg_g, *ln_lg_b, *tr_n1g[2], *tr_n1b[2], *tr_n2g[2], *tr_n2b[2], *pos32, *logit_scale;
    float *d_ln_vg_g, *d_ln_vg_b, *d_ln_lg_g, *d_ln_lg_b, *d_tr_n1g[2], *d_tr_n1b[2], *d_tr_n2g[2], *d_tr_n2b[2], *dpos, *dlogit_scale;
    // decoder input weights W_ih0 [HID][KIN] (sub-blocked) + packed heads
    const float *wih0_32, *bih0, *bhh0, *bih1, *bhh1;
    float *dwih0, *dbih0, *dbhh0, *dbih1, *dbhh1;
    T *wih0 = nullptr, *wih0T = nullptr;
    T *wheads = nullptr, *wheadsT = nullptr; float* bheads = nullptr; float *dwheads_tmp = nullptr, *dbheads_tmp = nullptr;
    const float *head_w32[4], *head_b32[4]; float *head_dw[4], *head_db[4]; int head_rows[4] = {60, 60, 60, 2};
    float* dw7_tmp = nullptr;
    bool bound = false;
    T* wshadow = nullptr;                 // bf16 mode: flat compute copy of all parameters (written by the Adam kernel)
    std::vector<TrDesc> trdesc; TrDesc* trdesc_dev = nullptr; int tr_blocks = 0; unsigned short* blk2desc_dev = nullptr;
    // round 5: Adam writes the transposed copies of the Linear weights itself (kernels.h adam_tiled_kernel).  Two sub-tables of `trdesc`: the matrices that are plain
    // views of the 16-bit shadow (tiled by the optimizer) and the rest (packed sources: the permuted fc7, the decoder heads — still transposed by prepare_weights)
    struct TrTable { TrDesc* desc = nullptr; unsigned short* b2d = nullptr; int blocks = 0, n = 0; };
    TrTable tr_adam, tr_rest;
    long long* adam_chunk_start = nullptr; int* adam_chunk_n = nullptr; int adam_chunks = 0;
    bool adam_fuse_tr = true;               // hulc_set_option "adam_fused_transposes"
    void set_adam_fuse(bool on) override { adam_fuse_tr = on; }
    bool frag_by_adam = false;              // every fragment-ordered weight copy is written by adam_tiled_kernel (TrDesc::fr / frT)
    bool rest_by_pack = false;              // weight_pack_kernel also writes the transposed copies of every matrix in tr_rest
    bool tr_fresh = false;                  // set by optim(): the shadow-sourced transposed copies are those of the current parameters
    void tr_table_free(TrTable& t) { if (t.desc) hipFree(t.desc); if (t.b2d) hipFree(t.b2d); t = TrTable{}; }
    bool tr_table_build(TrTable& t, std::vector<TrDesc> v) {
        tr_table_free(t);
        int blk = 0;
        for (TrDesc& d : v) { d.blk0 = blk; blk += d.tiles_x * cdiv(d.R, TRT); }
        t.blocks = blk; t.n = (int)v.size();
        if (v.empty()) return true;
        std::vector<unsigned short> b2d((size_t)blk);
        for (size_t i = 0; i < v.size(); ++i) { const int end = i + 1 < v.size() ? v[i + 1].blk0 : blk; for (int b = v[i].blk0; b < end; ++b) b2d[b] = (unsigned short)i; }
        if (hipMalloc((void**)&t.desc, sizeof(TrDesc) * v.size()) != hipSuccess || hipMalloc((void**)&t.b2d, sizeof(unsigned short) * b2d.size()) != hipSuccess) return false;
        hipMemcpy(t.desc, v.data(), sizeof(TrDesc) * v.size(), hipMemcpyHostToDevice);
        hipMemcpy(t.b2d, b2d.data(), sizeof(unsigned short) * b2d.size(), hipMemcpyHostToDevice);
        return true;
    }
    // the optimizer's tile / chunk tables: matrices of `trdesc` whose source is a contiguous [R][C] view of the shadow with 4-element alignment are tiled; the chunk
    // list covers the rest of [0, numel)
    void adam_tables_build() {
        tr_table_free(tr_adam); tr_table_free(tr_rest); rest_by_pack = false; frag_by_adam = false;
        if (adam_chunk_start) { hipFree(adam_chunk_start); adam_chunk_start = nullptr; } if (adam_chunk_n) { hipFree(adam_chunk_n); adam_chunk_n = nullptr; }
        adam_chunks = 0; tr_fused_host.clear(); tr_rest_host.clear();
        if (std::is_same<T, float>::value || !wshadow || (numel & 3)) return;
        std::vector<TrDesc> fused, rest;
        std::vector<std::pair<long long, long long>> rng;
        for (const TrDesc& d : trdesc) {
            const T* src = (const T*)d.src;
            const long long off = src - wshadow;
            const bool in = src >= wshadow && off + (long long)d.R * d.C <= numel && d.lds == d.C && (d.C & 3) == 0 && (off & 3) == 0 && !d.cs;
            if (in) { fused.push_back(d); rng.emplace_back(off, off + (long long)d.R * d.C); } else rest.push_back(d);
        }
        std::sort(rng.begin(), rng.end());
        for (size_t i = 0; i + 1 < rng.size(); ++i) if (rng[i].second > rng[i + 1].first) return;       // overlapping views: keep the flat kernel
        if (fused.empty() || fused.size() > 65535) return;
        std::vector<long long> cs; std::vector<int> cn;
        long long pos = 0;
        auto cover = [&](long long lo, long long hi) { for (long long x = lo; x < hi; x += ADAM_CHUNK) { cs.push_back(x); cn.push_back((int)std::min<long long>(ADAM_CHUNK, hi - x)); } };
        for (auto& r : rng) { cover(pos, r.first); pos = r.second; }
        cover(pos, numel);
        if (!tr_table_build(tr_adam, fused) || !tr_table_build(tr_rest, rest)) { tr_table_free(tr_adam); tr_table_free(tr_rest); return; }
        tr_fused_host = fused; tr_rest_host = rest;      // hulc_trainable_set filters them (engine_trainable.inc)
        // every transpose the optimizer does not write comes from a matrix weight_pack_kernel packs (the permuted fc7, the decoder heads): it writes their transposed copies as well
        { int lf = 0; for (const TrDesc& d : fused) if (d.fr && d.frT) ++lf; frag_by_adam = fragbatch.n > 0 && 2 * lf == fragbatch.n && lf == frag_linked; }
        rest_by_pack = true;
        for (const TrDesc& d : rest) {
            const bool f7 = d.src == (const void*)encG.fc7.W && d.dst == (void*)encG.fc7.Wt && d.R == 128 && d.C == 3136 && d.ldt == 128;
            const bool hd = d.src == (const void*)wheads && d.dst == (void*)wheadsT && d.R == NHEAD && d.C == HID && d.ldt == NHEAD;
            if (!f7 && !hd) rest_by_pack = false;
        }
        adam_chunks = (int)cs.size();
        if (adam_chunks) {
            if (hipMalloc((void**)&adam_chunk_start, sizeof(long long) * cs.size()) != hipSuccess || hipMalloc((void**)&adam_chunk_n, sizeof(int) * cn.size()) != hipSuccess) { tr_table_free(tr_adam); tr_table_free(tr_rest); adam_chunks = 0; tr_fused_host.clear(); tr_rest_host.clear(); return; }
            hipMemcpy(adam_chunk_start, cs.data(), sizeof(long long) * cs.size(), hipMemcpyHostToDevice);
            hipMemcpy(adam_chunk_n, cn.data(), sizeof(int) * cn.size(), hipMemcpyHostToDevice);
        }
    }

    // ---- workspace (per modality pass)
    // per camera: the activations, and the gradients of a1..a3, f1, f2 and of the tail's input (ss of the static camera: d_ss, fp32; g0 of the gripper camera: d_g0), set once
    // in alloc_all.  16-bit engines: each camera has its own gradient buffers (a stage runs for both cameras in one launch, both cameras' gradients are alive at once);
    // fp32 engine: the cameras run one after the other and point to the same buffers
    struct EncA {
        T *a1, *a2, *a3, *ss, *g0, *f1; float *ssstats, *f2, *lnst; unsigned* m1bits = nullptr; unsigned* m2bits = nullptr;
        T *dact1 = nullptr, *dact2 = nullptr, *dact3 = nullptr, *d_f1 = nullptr, *d_f2t = nullptr, *d_g0 = nullptr; float* d_ss = nullptr;
    } aS, aG;
    T *emb, *lang_t, *gl1, *gl2, *goal_t, *ppx, *ppa[4], *xm, *seqf_t, *embg, *Cb, *Zx0, *Zx1, *H0, *H1, *dheads, *dH1, *dZ1, *dH0, *dZ0, *dC;
    float *gl3, *goal_st, *pp_logits, *seqf, *pr_logits, *probs, *klcat, *dpp_kl, *dpr_kl, *Cplan, *heads, *rowloss, *a_tcp;
    int* pidx; int* pidx_in;
    T *xt[3], *qkv[2], *ao[2], *x1t[2], *hff[2];
    float *xf[3], *Pat[2], *y1[2], *st1[2], *x1f[2], *y2[2], *st2[2];
    float* zero_arena = nullptr; int64_t zero_n = 0; bool arena_clean = false;   // arena_clean: the forward's last launch has cleared it (only a backward writes it)
    int* work_ctrs = nullptr; int work_ctr_next = 0;
    int* next_ctr() { return work_ctrs ? work_ctrs + (work_ctr_next++ & 63) : nullptr; }
    // ---- reproducible mode (iengine.h "reproducible", repro_sites.h).  repro is the LATCHED option: a forward and its backward run the same routing.
    // Every scheduling-dependent launch site reports itself through nd(); the reproducible routing of a site never does.
    bool repro = false;
    unsigned long long nd_sites = 0;
    void nd(unsigned bit) { nd_sites |= bit; }
    void repro_latch() { repro = repro_opt != 0; }
    // claim counter of a launch whose workgroups ACCUMULATE over the items they claim (the weight-gradient kernels): null = the strided assignment
    int* claim_ctr(bool contended) { if (repro) return nullptr; int* c = next_ctr(); if (c && contended) nd(ND_CONV_CLAIM); return c; }
    bool trf_on() const { return tr_fused_mode && !repro; }      // the fused transformer launches sum with float atomics (tr_fused.h): reproducible mode runs the unfused layer
    float *demb, *dgoal, *dseqf, *dplan, *dprl, *dppx, *dxa, *dxb, *dy_f, *dxm;
    T *dprl_t, *dppl_t, *dseq_t, *dt_a, *dt_b, *dt_c, *dgl3_t;
    T *tA, *tB; int64_t tcap;
    bool h0t_valid = false;                 // tB2 holds H0^T of the current backward (16-bit engines)
    T* tB2 = nullptr;                       // second transposed-operand buffer (H0^T, transposed once next to dZ1^T and H1^T: read by dW_ih1 and again by dW_hh0)
    float *part; int64_t partcap; float* cspart;
    // clip
    int* auxrows; T *sf_m, *im1, *g_m, *la1, *img_t, *txt_t; float *img, *txt, *dimg, *dtxt, *dsf_m, *dg_m; T *dimg_t, *dtxt_t, *dim1, *dla1;
    float* losses;   // [8]: 0 action, 1 kl(sum klcat), 2 clip
    // BC-Z / MIA language auxiliary heads (aux_heads.h; hulc_aux_heads_enable): off unless enabled before the bind — then nothing below is allocated, bound or launched
    bool aux_bcz = false, aux_mia = false;
    float aux_w_bcz = 1.f, aux_w_mia = 1.f;
    LinW bz0, bz2;                                            // bc_z_lang_decoder.mlp.0 (4096 -> 512, ReLU), .mlp.2 (512 -> 384)
    const float *mia_w0 = nullptr, *mia_b0 = nullptr, *mia_w1 = nullptr, *mia_b1 = nullptr;      // mia_lang_discriminator.mlp.0 (64 -> 512), .mlp.3 (512 -> 1): read as fp32 by mia_head_kernel
    float *d_mia_w0 = nullptr, *d_mia_b0 = nullptr, *d_mia_w1 = nullptr, *d_mia_b1 = nullptr;
    T *bz1 = nullptr, *dbz1 = nullptr, *bz_dpred_t = nullptr; float *bz_pred = nullptr, *bz_tgt = nullptr, *bz_dpred = nullptr;
    float* aux_loss = nullptr;                               // device [4]: 0 bc_z, 1 mia (unweighted)
    int bcz_n = 0, mia_n = 0;                                // rows the heads of the last forward ran on (0: not launched, loss 0)
    float *clip_rows_ws = nullptr, *mia_rows_ws = nullptr;   // aux_rows.h workspaces of the n > 64 kernels: only a context with max_batch > 64 has them
    int aux_rows_last = 0;                                   // rows of the last forward / validate, for hulc_aux_losses_get
    // deterministic action decoder (det_head.h; hulc_decoder_select): off unless selected before the bind — then the packed mixture heads are neither allocated,
    // bound nor launched, and action_decoder.actions.0.* is read straight from the bound parameters (16-bit engines: from their shadow)
    bool det = false, dec_selected = false; int det_crit = HULC_CRIT_HUBER;
    const float *det_w32 = nullptr, *det_b32 = nullptr; float *det_dw = nullptr, *det_db = nullptr;
    const T* det_w = nullptr;
    float* dpre = nullptr;                                   // [S B][8]: gradient of the head's pre-activation
    // feed-forward decoder body (hulc_decoder_body_select, rnn_model = mlp_decoder): off unless selected before the bind.  Layer 0 keeps the recurrence's
    // decomposition (wih0 / bih0 are rnn.0.*, the second bias reads a zero vector and has no gradient), layers 1 / 2 are mlp1 / mlp2.  a0 lives in H0, a1 in H1, y in
    // Zx1, dy in dH1 and the two masked data gradients in dZ1 / dZ0; Zx0 and dH0 are released, the recurrences (engine_recurrent.inc) are never launched
    bool mlp = false, body_selected = false;
    LinW mlp1, mlp2;
    float* zbias = nullptr;                                  // [HID] zeros
    // ---- state of the last forward
    hulc_batch cur{}; float cur_lw = 0, cur_cw = 0; bool have_fwd = false;

    // =====================================================================================================
    Engine(const hulc_config& c) : cfg(c) {
        memset(&cur2, 0, sizeof(cur2));
        mcil = cfg.kind == HULC_KIND_MCIL || cfg.kind == HULC_KIND_MCIL_GRU;
        gru = cfg.kind == HULC_KIND_MCIL_GRU;
        PLAN = mcil ? 512 : 1024; NDIM = mcil ? 7 : 6; NO = NMIX * NDIM; NHEAD = mcil ? 224 : 192; DE = mcil ? EMB : 64;
        if (mcil) { head_rows[0] = head_rows[1] = head_rows[2] = NO; head_rows[3] = 0; }
        dec_plan = cfg.kind == HULC_KIND_GCBC ? 0 : (mcil ? PLAN / 2 : PLAN);
        KIN = dec_plan + DE + GOAL;
        maxB = cfg.max_batch; maxS = cfg.max_seq; maxN = maxB * maxS;
    }
    ~Engine() override { for (void* p : allocs) hipFree(p); if (rp_err_host) hipHostFree((void*)rp_err_host); if (blk2desc_dev) hipFree(blk2desc_dev); if (trdesc_dev) hipFree(trdesc_dev); tr_table_free(tr_adam); tr_table_free(tr_rest); if (adam_chunk_start) hipFree(adam_chunk_start); if (adam_chunk_n) hipFree(adam_chunk_n); gn_free(); tm_free(); if (clip_state) hipFree(clip_state); if (env_rows_host) hipHostFree(env_rows_host); }
    int64_t workspace_bytes() const override { return ws_bytes; }
    void set_kl_beta(float b) override { cfg.kl_beta = b; }
    void set_dropout(float p) override { cfg.dropout_p = p; }

    uint64_t site_seed(int site) const {
        uint64_t z = cfg.seed + 0x9E3779B97F4A7C15ull * (cur.step * 64 + (cur.is_lang ? 32 : 0) + site + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
    }

    // ---------------------------------------------------------------- allocation
    void alloc_enc(EncA& a, int IH, bool gripper, const char* pre) {
        const int H1 = (IH - 8) / 4 + 1, H2 = (H1 - 4) / 2 + 1, H3 = H2 - 2;
        std::string s(pre);
        a.a1 = alloc<T>((int64_t)maxN * H1 * H1 * 32, (s + "a1").c_str());
        a.m1bits = std::is_same<T, h16_t>::value ? alloc<unsigned>((int64_t)maxN * H1 * H1) : nullptr;   // ReLU bitmask of a1 (conv2 dgrad)
        a.a2 = alloc<T>((int64_t)maxN * H2 * H2 * 64, (s + "a2").c_str());
        a.m2bits = std::is_same<T, h16_t>::value ? alloc<unsigned>((int64_t)maxN * H2 * H2 * 2) : nullptr;   // ReLU bitmask of a2 (conv3 dgrad), emitted by conv2's forward
        a.a3 = alloc<T>((int64_t)maxN * H3 * H3 * 64, (s + "a3").c_str());
        a.ss = gripper ? nullptr : alloc<T>((int64_t)maxN * 128, (s + "ss").c_str());
        a.ssstats = gripper ? nullptr : alloc<float>((int64_t)maxN * 64 * 4);
        a.g0 = gripper ? alloc<T>((int64_t)maxN * 128, (s + "g0").c_str()) : nullptr;
        a.f1 = alloc<T>((int64_t)maxN * 512, (s + "f1").c_str());
        a.f2 = alloc<float>((int64_t)maxN * 64, (s + "f2").c_str());
        a.lnst = alloc<float>((int64_t)maxN * 2);
    }
    int alloc_all() {
        const int64_t N = maxN, B = maxB, S = maxS, SB = (int64_t)maxS * maxB;
        alloc_enc(aS, 200, false, "s_");
        alloc_enc(aG, 84, true, "g_");
        aS.dact1 = alloc<T>(N * 49 * 49 * 32, "dact1"); aS.dact2 = alloc<T>(N * 23 * 23 * 64, "dact2"); aS.dact3 = alloc<T>(N * 21 * 21 * 64, "dact3");
        aG.d_g0 = alloc<T>(N * 128); aS.d_f1 = alloc<T>(N * 512); aS.d_f2t = alloc<T>(N * 64); aS.d_ss = alloc<float>(N * 128, "d_ss");
        if constexpr (std::is_same<T, h16_t>::value) {
            aG.d_f1 = alloc<T>(N * 512); aG.d_f2t = alloc<T>(N * 64);
            aG.dact1 = alloc<T>(N * 20 * 20 * 32, "g_dact1"); aG.dact2 = alloc<T>(N * 9 * 9 * 64, "g_dact2"); aG.dact3 = alloc<T>(N * 7 * 7 * 64, "g_dact3");      // 42 KB per frame (87 MB at 2048 frames)
        } else {
            aG.d_f1 = aS.d_f1; aG.d_f2t = aS.d_f2t; aG.dact1 = aS.dact1; aG.dact2 = aS.dact2; aG.dact3 = aS.dact3;
        }
        emb = alloc<T>(N * EMB, "emb"); lang_t = alloc<T>(B * LANG); gl1 = alloc<T>(B * HID); gl2 = alloc<T>(B * HID);
        gl3 = alloc<float>(B * GOAL, "goal_pre"); goal_t = alloc<T>(B * GOAL, "goal"); goal_st = alloc<float>(B * 2);
        ppx = alloc<T>(B * (EMB + GOAL)); for (int i = 0; i < 4; ++i) ppa[i] = alloc<T>(B * HID);
        pp_logits = alloc<float>(B * PLAN, "pp_logits");
        for (int l = 0; l < 3; ++l) { xt[l] = alloc<T>(N * EMB); xf[l] = alloc<float>(N * EMB, l == 2 ? "pr_x_final" : (l == 0 ? "pr_x0" : "pr_x1")); }
        for (int l = 0; l < 2; ++l) {
            qkv[l] = alloc<T>(N * 3 * EMB); Pat[l] = alloc<float>(B * NH * S * S, l ? "attn_p1" : "attn_p0"); ao[l] = alloc<T>(N * EMB);
            y1[l] = alloc<float>(N * EMB); st1[l] = alloc<float>(N * 2); x1t[l] = alloc<T>(N * EMB); x1f[l] = alloc<float>(N * EMB);
            hff[l] = alloc<T>(N * FF); y2[l] = alloc<float>(N * EMB); st2[l] = alloc<float>(N * 2);
        }
        xm = alloc<T>(B * EMB); seqf = alloc<float>(B * FCH, "seq_feat"); seqf_t = alloc<T>(B * FCH); pr_logits = alloc<float>(B * PLAN, "pr_logits");
        probs = alloc<float>(B * PLAN, "pr_probs"); klcat = alloc<float>(B * NCAT); dpp_kl = alloc<float>(B * PLAN); dpr_kl = alloc<float>(B * PLAN);
        pidx = alloc<int>(B * NCAT, "plan_idx"); pidx_in = alloc<int>(B * NCAT);
        embg = alloc<T>(SB * DE); Cplan = alloc<float>(B * HID); Cb = alloc<T>(B * HID, "dec_cb");
        Zx0 = alloc<T>(SB * HID); Zx1 = alloc<T>(SB * HID); H0 = alloc<T>(SB * HID, "dec_h0"); H1 = alloc<T>(SB * HID, "dec_h1");
        heads = alloc<float>(SB * NHEAD, "heads"); dheads = alloc<T>(SB * NHEAD, "dheads"); rowloss = alloc<float>(SB * 8); a_tcp = alloc<float>(SB * 7, "a_tcp");
        dH1 = alloc<T>(SB * HID); dZ1 = alloc<T>(SB * HID, "dec_dz1"); dH0 = alloc<T>(SB * HID); dZ0 = alloc<T>(SB * HID, "dec_dz0"); dC = alloc<T>(B * HID);
        // backward scratch that must start at zero lives in ONE arena -> a single memset per backward
        {
            auto r64 = [](int64_t n) { return (n + 63) / 64 * 64; };
            zero_n = r64(N * EMB) + r64(B * GOAL) + r64(B * FCH) + r64((int64_t)NHEAD * HID) + r64(NHEAD) + r64(128 * 3136) + 64;
            zero_arena = alloc<float>(zero_n);
            float* q = zero_arena;
            demb = q; q += r64(N * EMB); dgoal = q; q += r64(B * GOAL); dseqf = q; q += r64(B * FCH);
            dwheads_tmp = q; q += r64((int64_t)NHEAD * HID); dbheads_tmp = q; q += r64(NHEAD); dw7_tmp = q; q += r64(128 * 3136);
            work_ctrs = reinterpret_cast<int*>(q);      // 64 zeroed counters per backward: dynamic work claiming of the persistent encoder-backward kernels
            named["demb"] = Named{demb, N * EMB, 0}; named["dgoal"] = Named{dgoal, B * GOAL, 0}; named["dseq_feat"] = Named{dseqf, B * FCH, 0};
        }
        dplan = alloc<float>(B * PLAN, "dplan"); dprl = alloc<float>(B * PLAN, "dpr_logits"); dppx = alloc<float>(B * (EMB + GOAL));
        dxa = alloc<float>(N * EMB, "tr_dx"); dxb = alloc<float>(N * EMB); dy_f = alloc<float>(N * EMB, "tr_dy1"); dxm = alloc<float>(B * EMB);
        dprl_t = alloc<T>(B * PLAN); dppl_t = alloc<T>(B * PLAN); dseq_t = alloc<T>(B * FCH);
        dt_a = alloc<T>(std::max<int64_t>(N * FF, 2 * B * HID)); dt_b = alloc<T>(N * 3 * EMB); dt_c = alloc<T>(N * EMB); dgl3_t = alloc<T>(B * GOAL);
        tcap = std::max<int64_t>(3136 * ((N + 7) / 8 * 8), std::max<int64_t>((gru ? 3 : 1) * HID * ((SB + 7) / 8 * 8), FCH * ((B + 7) / 8 * 8))) + 4096;
        tA = alloc<T>(tcap); tB = alloc<T>(tcap);
        // conv weight-gradient slabs: the 16-bit engines keep the slabs of ALL convolutions of a backward (one batched unpack launch at its end)
        partcap = std::is_same<T, h16_t>::value ? 96ll * 1024 * 1024 : 1024ll * 64 * 576; part = alloc<float>(partcap); cspart = alloc<float>(1024 * 2048);
        auxrows = alloc<int>(B); sf_m = alloc<T>(B * FCH); im1 = alloc<T>(B * 128); g_m = alloc<T>(B * GOAL); la1 = alloc<T>(B * 128);
        img = alloc<float>(B * GOAL, "clip_img"); txt = alloc<float>(B * GOAL, "clip_txt"); img_t = alloc<T>(B * GOAL); txt_t = alloc<T>(B * GOAL);
        dimg = alloc<float>(B * GOAL); dtxt = alloc<float>(B * GOAL); dimg_t = alloc<T>(B * GOAL); dtxt_t = alloc<T>(B * GOAL);
        dim1 = alloc<T>(B * 128); dla1 = alloc<T>(B * 128); dsf_m = alloc<float>(B * FCH); dg_m = alloc<float>(B * GOAL);
        losses = alloc<float>(8);
        if (B > AUX_ROWS_SINGLE && cfg.use_clip) clip_rows_ws = alloc<float>(clip_rows_ws_floats(B));
        if (gru) {
            for (int c = 0; c < 4; ++c) {
                const int64_t rows = c < 3 ? SB : B;
                gb[c].Zx = alloc<T>(rows * 3 * HID); gb[c].R = alloc<T>(rows * HID); gb[c].Z = alloc<T>(rows * HID); gb[c].N = alloc<T>(rows * HID);
                gb[c].GN = alloc<T>(rows * HID); gb[c].dZx = alloc<T>(rows * 3 * HID); gb[c].dG = alloc<T>(rows * 3 * HID);
            }
            gGf = alloc<float>(B * 3 * HID); gcarA = alloc<T>(B * HID); gcarB = alloc<T>(B * HID);
        }
        if (mcil) {
            for (int d = 0; d < 2; ++d) { bZ0[d] = alloc<T>(SB * HID); bH0[d] = alloc<T>(SB * HID, d ? "birnn_h0_rev" : "birnn_h0"); bdH0[d] = alloc<T>(SB * HID); bdZ0[d] = alloc<T>(SB * HID); }
            bZ1 = alloc<T>(SB * HID); bH1 = alloc<T>(SB * HID, "birnn_h1"); bh1b = alloc<T>(B * HID); bxcat = alloc<T>(B * 2 * HID, "birnn_x"); bdx = alloc<T>(B * 2 * HID);
            bdZ1 = alloc<T>(SB * HID); bdz1b = alloc<T>(B * HID);
            plan_t = alloc<T>(B * PLAN / 2); plan_f = alloc<float>(B * PLAN / 2, "plan"); plan_eps = alloc<float>(B * PLAN / 2); plan_eps_in = alloc<float>(B * PLAN / 2);
            klel = alloc<float>(B * PLAN / 2);
        }
        bheads = alloc<float>(NHEAD); wheads = alloc<T>((int64_t)NHEAD * HID); wheadsT = alloc<T>((int64_t)HID * NHEAD);
        if (alloc_failed) { hulc_set_error("hipMalloc failed while sizing the workspace (B=%d S=%d)", maxB, maxS); return 1; }
#ifdef HULC_HALF_F16
        if (!std::is_same<T, float>::value) return scaler_enable(65536.f, 2.f, 0.5f, 2000);      // torch.cuda.amp.GradScaler() defaults
#endif
        return 0;
    }

    // ---------------------------------------------------------------- BC-Z / MIA language auxiliary heads (include/hulc_hip.h: hulc_aux_heads_enable)
    int aux_heads_enable(int bc_z, int mia) override {
        if (bound) { hulc_set_error("hulc_aux_heads_enable after hulc_bind_params (the heads' tensors are bound by name: enable them first)"); return 1; }
        if (mcil) { hulc_set_error("hulc_aux_heads_enable: HULC_KIND_MCIL has no proj_vis_lang and trains without the language auxiliary losses (conf/model/mcil.yaml)"); return 1; }
        if (aux_bcz || aux_mia) { hulc_set_error("hulc_aux_heads_enable: the heads of this context are already enabled"); return 1; }
        if (!bc_z && !mia) return 0;
        const int64_t B = maxB;
        if (bc_z) {
            bz1 = alloc<T>(B * 512); dbz1 = alloc<T>(B * 512); bz_dpred_t = alloc<T>(B * LANG);
            bz_pred = alloc<float>(B * LANG, "bcz_pred"); bz_tgt = alloc<float>(B * LANG); bz_dpred = alloc<float>(B * LANG);
        }
        aux_loss = alloc<float>(4);
        if (mia && B > AUX_ROWS_SINGLE) mia_rows_ws = alloc<float>(mia_rows_ws_floats(B));
        if (alloc_failed) { hulc_set_error("hulc_aux_heads_enable: workspace allocation failed"); return 1; }
        aux_bcz = bc_z != 0; aux_mia = mia != 0;
        return 0;
    }
    // ---------------------------------------------------------------- deterministic action decoder (include/hulc_hip.h: hulc_decoder_select)
    template <typename U> void release(U*& p) {
        if (!p) return;
        for (auto it = named.begin(); it != named.end();) { if (it->second.p == (void*)p) it = named.erase(it); else ++it; }
        allocs.erase(std::remove(allocs.begin(), allocs.end(), (void*)p), allocs.end());
        ws_bytes -= alloc_sz[(void*)p]; alloc_sz.erase((void*)p);
        hipFree((void*)p); p = nullptr;
    }
    int decoder_select(int decoder, int criterion) override {
        if (bound) { hulc_set_error("hulc_decoder_select after hulc_bind_params (the head's tensors are bound by name: select the decoder first)"); return 1; }
        if (decoder != HULC_DECODER_LOGISTIC && decoder != HULC_DECODER_DETERMINISTIC) { hulc_set_error("hulc_decoder_select: unknown decoder %d", decoder); return 1; }
        if (dec_selected) { hulc_set_error("hulc_decoder_select: the decoder of this context is already selected"); return 1; }
        if (decoder == HULC_DECODER_LOGISTIC) { dec_selected = true; return 0; }
        if (cfg.kind == HULC_KIND_GCBC) { hulc_set_error("hulc_decoder_select: HULC_KIND_GCBC with the deterministic decoder has no reference behaviour (GCBC.forward raises: torch.cat of a (B,0) plan with (B,S,.) tensors)"); return 1; }
        if (mcil) { hulc_set_error("hulc_decoder_select: the deterministic decoder is not built for HULC_KIND_MCIL* (gripper_control false, 128-wide embedding slice)"); return 1; }
        if (mlp) { hulc_set_error("hulc_decoder_select: the deterministic decoder is not built on the feed-forward body (HULC_BODY_MLP is selected)"); return 1; }
        if (criterion != HULC_CRIT_HUBER && criterion != HULC_CRIT_MSE) { hulc_set_error("hulc_decoder_select: criterion %d (HULC_CRIT_HUBER or HULC_CRIT_MSE)", criterion); return 1; }
        static_assert(HID == DET_HID, "det_head.h is built for the 2048-wide decoder");
        HIP_CHECK(hipStreamSynchronize(st));      // the buffers' clearing memsets
        const int64_t SB = (int64_t)maxS * maxB;
        release(heads); release(dheads); release(wheads); release(wheadsT);
        dpre = alloc<float>(SB * DET_LD, "det_dpre");
        if (alloc_failed) { hulc_set_error("hulc_decoder_select: workspace allocation failed"); return 1; }
        for (int i = 0; i < 4; ++i) head_rows[i] = 0;
        det = true; det_crit = criterion; dec_selected = true;
        return 0;
    }
    // ---------------------------------------------------------------- feed-forward decoder body (include/hulc_hip.h: hulc_decoder_body_select)
    int decoder_body_select(int body) override {
        if (bound) { hulc_set_error("hulc_decoder_body_select after hulc_bind_params (the body's tensors are bound by name: select the body first)"); return 1; }
        if (body != HULC_BODY_RNN && body != HULC_BODY_MLP) { hulc_set_error("hulc_decoder_body_select: unknown body %d", body); return 1; }
        if (body_selected) { hulc_set_error("hulc_decoder_body_select: the decoder body of this context is already selected"); return 1; }
        if (body == HULC_BODY_RNN) { body_selected = true; return 0; }
        if (mcil) { hulc_set_error("hulc_decoder_body_select: the feed-forward body is not built for HULC_KIND_MCIL* (continuous plan, 128-wide embedding slice)"); return 1; }
        if (det) { hulc_set_error("hulc_decoder_body_select: the feed-forward body is not built under the deterministic decoder (HULC_DECODER_DETERMINISTIC is selected)"); return 1; }
        HIP_CHECK(hipStreamSynchronize(st));      // the buffers' clearing memsets
        release(Zx0); release(dH0);
        zbias = alloc<float>(HID);
        if (alloc_failed) { hulc_set_error("hulc_decoder_body_select: workspace allocation failed"); return 1; }
        const int64_t n = (int64_t)maxS * maxB * HID;
        named["dec_a0"] = Named{H0, n, 1}; named["dec_a1"] = Named{H1, n, 1}; named["dec_y"] = Named{Zx1, n, 1};
        named["dec_dy"] = Named{dH1, n, 1}; named["dec_da1"] = Named{dZ1, n, 1}; named["dec_da0"] = Named{dZ0, n, 1};
        mlp = true; body_selected = true;
        return 0;
    }
    int aux_weights_set(float bc_z_weight, float mia_weight) override { aux_w_bcz = bc_z_weight; aux_w_mia = mia_weight; return 0; }
    // [bc_z, mia, rows, 0] of the last forward / validate, unweighted; a head that did not run (not enabled, no flagged row, no forward yet) reads 0
    int aux_losses_get(float* out_host) override {
        if (!out_host) { hulc_set_error("hulc_aux_losses_get: null output"); return 1; }
        float h[4] = {0.f, 0.f, 0.f, 0.f};
        if (bcz_n > 0 || mia_n > 0) HIP_CHECK(hipMemcpyAsync(h, aux_loss, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        out_host[0] = bcz_n > 0 ? h[0] : 0.f; out_host[1] = mia_n > 0 ? h[1] : 0.f; out_host[2] = (float)aux_rows_last; out_host[3] = 0.f;
        return 0;
    }
    // the heads' forward on the n gathered rows (auxrows uploaded); `shared` = the CLIP block of this pass already gathered sf_m / g_m and projected img / txt.
    // train: gradients of the losses w.r.t. img / txt / pred are left for the backward, the discriminator's own gradients are added by its kernel
    int aux_heads_fwd(const hulc_batch* b, int n, bool shared, bool train, int lang_row0) {
        if (!shared) hipLaunchKernelGGL((gather_rows_kernel<T, T>), dim3(cdiv(n * FCH, 256)), dim3(256), 0, st, seqf_t, (long long)FCH, auxrows, n, FCH, sf_m);
        if (aux_mia) {
            if (!shared) {
                hipLaunchKernelGGL((gather_rows_kernel<T, T>), dim3(cdiv(n * GOAL, 256)), dim3(256), 0, st, goal_t, (long long)GOAL, auxrows, n, GOAL, g_m);
                { EpiP ep = epi(im1, false); ep.relu = 1; lin_fwd(sf_m, FCH, n, cl_im0, ep, 128); }
                { EpiP ep = epi(img, true); lin_fwd(im1, 128, n, cl_im2, ep, GOAL); }
                { EpiP ep = epi(la1, false); ep.relu = 1; lin_fwd(g_m, GOAL, n, cl_la0, ep, 128); }
                { EpiP ep = epi(txt, true); lin_fwd(la1, 128, n, cl_la2, ep, GOAL); }
            }
            static_assert(GOAL == MIA_D, "mia_head_kernel is built for 32-wide projections");
            const bool ok = train ? launch_mia_head(st, img, txt, n, mia_w0, mia_b0, mia_w1, mia_b1, aux_w_mia, aux_loss + 1, dimg, dtxt, shared ? 1 : 0, d_mia_w0, d_mia_b0, d_mia_w1,
                                                    d_mia_b1, lscale(), mia_rows_ws)
                                  : launch_mia_head(st, img, txt, n, mia_w0, mia_b0, mia_w1, mia_b1, 0.f, aux_loss + 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                    mia_rows_ws);
            if (!ok) { hulc_set_error("MIA head: n=%d rows not covered by this context's workspace (max_batch=%d)", n, maxB); return 1; }
            mia_n = n;
        }
        if (aux_bcz) {
            // lang[rows]: the batch's fp32 embeddings; the paired pass numbers the lang rows from Bv
            hipLaunchKernelGGL((gather_rows_kernel<float, float>), dim3(cdiv(n * LANG, 256)), dim3(256), 0, st, b->lang - (long long)lang_row0 * LANG, (long long)LANG, auxrows, n, LANG, bz_tgt);
            { EpiP ep = epi(bz1, false); ep.relu = 1; lin_fwd(sf_m, FCH, n, bz0, ep, 512); }
            { EpiP ep = epi(bz_pred, true); lin_fwd(bz1, 512, n, bz2, ep, LANG); }
            hipLaunchKernelGGL(cosine_dist_loss_kernel, dim3(1), dim3(1024), 0, st, bz_pred, bz_tgt, n, LANG, train ? aux_w_bcz : 0.f, aux_loss + 0, train ? bz_dpred : (float*)nullptr,
                               train ? lscale() : (const float*)nullptr);
            bcz_n = n;
        }
        return 0;
    }

    // ---------------------------------------------------------------- binding
    bool has(const std::string& n) const { return tab.count(n) > 0; }
    const float* pw(const std::string& n) { return P + tab.at(n).off; }
    float* gw(const std::string& n) { return G + tab.at(n).off; }
    void bind_lin(LinW& L, const std::string& name, int N, int K, bool bias_suffix = true) {
        L.W32 = pw(name + (bias_suffix ? ".weight" : "")); L.dW = gw(name + (bias_suffix ? ".weight" : ""));
        if (bias_suffix) { L.b32 = pw(name + ".bias"); L.db = gw(name + ".bias"); }
        L.N = N; L.K = K;
        if (std::is_same<T, float>::value) L.W = (T*)L.W32;
        else L.W = wshadow + (L.W32 - P);
        L.own_w = false;
        if (!L.Wt) L.Wt = alloc<T>((int64_t)N * K);
        add_tr(L.W32, L.W, L.Wt, N, K);
    }
    // fragment-ordered weight copies (gemm.h: frag_pack_kernel): the recurrent weights of the GRU plan encoder and the plan-recognition transformer's
    // weights, whose kernels read MFMA fragments straight from global memory.  Jobs are collected at bind time, one batched launch in prepare_weights
    FragPackBatch fragbatch{};
    int frag_blocks = 0;
    void add_frag(LinW& L) {
        if constexpr (std::is_same<T, h16_t>::value) {
            if (!L.Wfr) L.Wfr = alloc<T>((int64_t)L.N * L.K);
            if (!L.Wtfr) L.Wtfr = alloc<T>((int64_t)L.N * L.K);
            if (fragbatch.n + 2 > FRAG_PACK_MAX) return;
            FragPackBatch& fb = fragbatch;
            fb.src[fb.n] = L.W; fb.dst[fb.n] = L.Wfr; fb.N[fb.n] = L.N; fb.K[fb.n] = L.K; fb.blk0[fb.n] = frag_blocks; frag_blocks += frag_pack_blocks(L.N, L.K); ++fb.n;
            fb.src[fb.n] = L.Wt; fb.dst[fb.n] = L.Wtfr; fb.N[fb.n] = L.K; fb.K[fb.n] = L.N; fb.blk0[fb.n] = frag_blocks; frag_blocks += frag_pack_blocks(L.K, L.N); ++fb.n;
            fb.blk0[fb.n] = frag_blocks;
            // the optimizer's tile pass can write both copies (kernels.h adam_tiled_kernel): remember them on the weight's transpose descriptor
            for (TrDesc& d : trdesc)
                if (d.dst == (void*)L.Wt && d.R == L.N && d.C == L.K && (L.N % 32) == 0 && (L.K % 32) == 0) { d.fr = L.Wfr; d.frT = L.Wtfr; ++frag_linked; }
        }
    }
    int frag_linked = 0;                    // weights whose fragment-ordered copies ride on their transpose descriptor (2 frag jobs each)
    static constexpr int TRT = std::is_same<T, float>::value ? 32 : 64;     // transpose tile (bf16: 64x64, 16-byte accesses)
    void add_tr(const float* w32, const T* w, T* wt, int R, int C) {
        TrDesc d; d.src = std::is_same<T, float>::value ? (const void*)w32 : (const void*)w; d.dst = wt; d.lds = C; d.ldt = R; d.R = R; d.C = C;
        d.tiles_x = cdiv(C, TRT); d.blk0 = tr_blocks; tr_blocks += d.tiles_x * cdiv(R, TRT);
        trdesc.push_back(d);
    }
    // a transpose whose source is a packed compute-type buffer of this engine (not a parameter): T -> T in both engine kinds
    void add_tr_packed(const T* src, T* wt, int R, int C) {
        TrDesc d; d.src = src; d.dst = wt; d.lds = C; d.ldt = R; d.R = R; d.C = C;
        d.tiles_x = cdiv(C, TRT); d.blk0 = tr_blocks; tr_blocks += d.tiles_x * cdiv(R, TRT);
        trdesc.push_back(d);
    }
    void bind_conv(ConvW& c, const std::string& name, int O, int I, int K, int S, int nhwc) {
        c.W32 = pw(name + ".weight"); c.b32 = pw(name + ".bias"); c.dW = gw(name + ".weight"); c.db = gw(name + ".bias");
        c.O = O; c.I = I; c.KH = c.KW = K; c.S = S; c.nhwc = nhwc;
        if (!c.Wf) c.Wf = alloc<T>((int64_t)O * I * K * K);
        if (nhwc && !c.Wd) c.Wd = alloc<T>((int64_t)O * I * K * K);
    }
    void bind_enc(EncW& e, const std::string& pre, bool gripper, int IH) {
        e.gripper = gripper; e.IH = IH; e.H1 = (IH - 8) / 4 + 1; e.H2 = (e.H1 - 4) / 2 + 1; e.H3 = e.H2 - 2;
        bind_conv(e.c1, pre + "conv_model.0", 32, 3, 8, 4, 0);
        bind_conv(e.c2, pre + "conv_model.2", 64, 32, 4, 2, 1);
        bind_conv(e.c3, pre + "conv_model.4", 64, 64, 3, 1, 1);
        if (gripper) {
            // fc7 consumes the NHWC flatten: keep packed copies (W, Wt own storage even in fp32 mode)
            e.fc7.W32 = pw(pre + "conv_model.7.weight"); e.fc7.b32 = pw(pre + "conv_model.7.bias");
            e.fc7.dW = gw(pre + "conv_model.7.weight"); e.fc7.db = gw(pre + "conv_model.7.bias");
            e.fc7.N = 128; e.fc7.K = 3136;
            if (!e.fc7.W) { e.fc7.W = alloc<T>(128 * 3136); e.fc7.Wt = alloc<T>(128 * 3136); e.fc7.own_w = true; }
            add_tr_packed(e.fc7.W, e.fc7.Wt, 128, 3136);      // transposed copy of the PERMUTED weight (weight_pack_kernel writes it just before the batched transpose)
        }
        bind_lin(e.fc1, pre + "fc1.0", 512, 128);
        bind_lin(e.fc2, pre + "fc2", 64, 512);
        e.lng = pw(pre + "ln.weight"); e.lnb = pw(pre + "ln.bias"); e.dlng = gw(pre + "ln.weight"); e.dlnb = gw(pre + "ln.bias");
    }
    int bind(float* p, float* g, float* m, float* v, int64_t n_, int n, const char* const* names, const int64_t* offs,
             const int64_t* numels) override {
        P = p; G = g; AM = m; AV = v; numel = n_;
        tab.clear(); trdesc.clear(); tr_blocks = 0; fragbatch = FragPackBatch{}; frag_blocks = 0; frag_linked = 0;
        if (!std::is_same<T, float>::value && !wshadow) wshadow = alloc<T>(numel, "wshadow");      // named: hulc_get_tensor reads the 16-bit shadow back (tests)
        for (int i = 0; i < n; ++i) tab[names[i]] = Ref{offs[i], numels[i]};
        gn_tens.clear(); gn_built = false; gn_have = false;      // the gradient-norm tables follow the tensor table (rebuilt at the end of this bind if clipping by norm / tracking is configured)
        for (int i = 0; i < n; ++i) gn_tens.push_back(Ref{offs[i], numels[i]});
        tm_reset(); tm_names.clear();      // a new tensor table: every tensor trainable until hulc_trainable_set says otherwise
        ema = nullptr; ema_swapped = false;      // ... and no average: its buffer was borrowed for the old table (hulc_ema_enable again)
        for (int i = 0; i < n; ++i) tm_names.push_back(names[i]);
        tab_order.assign(tab.begin(), tab.end());
        std::sort(tab_order.begin(), tab_order.end(), [](const std::pair<std::string, Ref>& a, const std::pair<std::string, Ref>& b) { return a.second.off < b.second.off; });
        // data parallelism: the "this step's gradients are garbage" vote rides in an alignment-padding element of the LAST bucket (see skip_vote_put)
        lazy.clear();
        skip_pad = -1;
        // (only a REAL padding element qualifies — hulc_bind_params accepts any 4-aligned layout, so the element behind a tensor is
        //  padding only if the next tensor of the table starts later; a tightly packed layout has no vote word and the vote falls back to skip_pad = -1)
        for (size_t i = 0; i < tab_order.size(); ++i) {
            const auto& kv = tab_order[i];
            const int64_t end = kv.second.off + kv.second.n, nxt = i + 1 < tab_order.size() ? tab_order[i + 1].second.off : numel;
            if (kv.first.compare(0, 19, "perceptual_encoder.") == 0 && end < nxt && end < numel) { skip_pad = end; break; }
        }
        try {
            bind_enc(encS, "perceptual_encoder.rgb_static_encoder.", false, 200);
            bind_enc(encG, "perceptual_encoder.rgb_gripper_encoder.", true, 84);
            const char* ppn[5] = {"plan_proposal.fc_model.0", "plan_proposal.fc_model.2", "plan_proposal.fc_model.4", "plan_proposal.fc_model.6",
                                  "plan_proposal.fc_state.0"};
            const int ppN[5] = {HID, HID, HID, HID, PLAN}, ppK[5] = {EMB + GOAL, HID, HID, HID, HID};
            for (int i = 0; i < 5; ++i) bind_lin(pp[i], ppn[i], ppN[i], ppK[i]);
            const char* vgn[3] = {"visual_goal.mlp.0", "visual_goal.mlp.2", "visual_goal.mlp.4"};
            const char* lgn[3] = {"language_goal.mlp.1", "language_goal.mlp.3", "language_goal.mlp.5"};
            const int gN[3] = {HID, HID, GOAL};
            const int vK[3] = {EMB, HID, HID}, lK[3] = {LANG, HID, HID};
            for (int i = 0; i < 3; ++i) { bind_lin(vg[i], vgn[i], gN[i], vK[i]); bind_lin(lg[i], lgn[i], gN[i], lK[i]); }
            ln_vg_g = pw("visual_goal.ln.weight"); ln_vg_b = pw("visual_goal.ln.bias"); d_ln_vg_g = gw("visual_goal.ln.weight"); d_ln_vg_b = gw("visual_goal.ln.bias");
            ln_lg_g = pw("language_goal.ln.weight"); ln_lg_b = pw("language_goal.ln.bias"); d_ln_lg_g = gw("language_goal.ln.weight"); d_ln_lg_b = gw("language_goal.ln.bias");
            const std::string pr = "plan_recognition.";
            if (mcil) {
                for (int l = 0; l < 2; ++l)
                    for (int d = 0; d < 2; ++d) {
                        const std::string sfx = "_l" + std::to_string(l) + (d ? "_reverse" : "");
                        const std::string bp = pr + "birnn_model.";
                        bind_lin(bw_ih[l][d], bp + "weight_ih" + sfx, (gru ? 3 : 1) * HID, l ? 2 * HID : EMB, false);
                        bind_lin(bw_hh[l][d], bp + "weight_hh" + sfx, (gru ? 3 : 1) * HID, HID, false);
                        if (gru) add_frag(bw_hh[l][d]);
                        bb_ih[l][d] = pw(bp + "bias_ih" + sfx); bb_hh[l][d] = pw(bp + "bias_hh" + sfx);
                        dbb_ih[l][d] = gw(bp + "bias_ih" + sfx); dbb_hh[l][d] = gw(bp + "bias_hh" + sfx);
                    }
            } else {
            pos32 = pw(pr + "position_embeddings.weight"); dpos = gw(pr + "position_embeddings.weight");
            for (int l = 0; l < 2; ++l) {
                const std::string L = pr + "transformer_encoder.layers." + std::to_string(l) + ".";
                tr_in[l].W32 = pw(L + "self_attn.in_proj_weight"); tr_in[l].dW = gw(L + "self_attn.in_proj_weight");
                tr_in[l].b32 = pw(L + "self_attn.in_proj_bias"); tr_in[l].db = gw(L + "self_attn.in_proj_bias");
                tr_in[l].N = 3 * EMB; tr_in[l].K = EMB;
                tr_in[l].W = std::is_same<T, float>::value ? (T*)tr_in[l].W32 : wshadow + (tr_in[l].W32 - P);
                if (!tr_in[l].Wt) tr_in[l].Wt = alloc<T>(3 * EMB * EMB);
                add_tr(tr_in[l].W32, tr_in[l].W, tr_in[l].Wt, 3 * EMB, EMB);
                bind_lin(tr_out[l], L + "self_attn.out_proj", EMB, EMB);
                bind_lin(tr_l1[l], L + "linear1", FF, EMB);
                bind_lin(tr_l2[l], L + "linear2", EMB, FF);
                for (LinW* w : {&tr_in[l], &tr_out[l], &tr_l1[l], &tr_l2[l]}) add_frag(*w);      // the fused layer kernels (tr_fused.h) read these
                tr_n1g[l] = pw(L + "norm1.weight"); tr_n1b[l] = pw(L + "norm1.bias"); d_tr_n1g[l] = gw(L + "norm1.weight"); d_tr_n1b[l] = gw(L + "norm1.bias");
                tr_n2g[l] = pw(L + "norm2.weight"); tr_n2b[l] = pw(L + "norm2.bias"); d_tr_n2g[l] = gw(L + "norm2.weight"); d_tr_n2b[l] = gw(L + "norm2.bias");
            }
            bind_lin(pr_fc, pr + "fc", FCH, EMB);
            }
            bind_lin(pr_fs, pr + "fc_state.0", PLAN, FCH);
            const std::string ad = "action_decoder.";
            if (mlp) {      // rnn.0 takes the place of weight_ih_l0 / bias_ih_l0; there is no second bias (zbias) and nothing recurrent
                wih0_32 = pw(ad + "rnn.0.weight"); dwih0 = gw(ad + "rnn.0.weight");
                bih0 = pw(ad + "rnn.0.bias"); dbih0 = gw(ad + "rnn.0.bias"); bhh0 = zbias; dbhh0 = nullptr;
                bih1 = bhh1 = nullptr; dbih1 = dbhh1 = nullptr;
                for (const char* l : {"rnn.2", "rnn.4"})
                    if (tab.at(ad + l + ".weight").n != (int64_t)HID * HID || tab.at(ad + l + ".bias").n != HID) {
                        hulc_set_error("hulc_bind_params: action_decoder.%s must be Linear(2048, 2048)", l); return 1; }
                if (tab.at(ad + "rnn.0.weight").n != (int64_t)HID * KIN || tab.at(ad + "rnn.0.bias").n != HID) {
                    hulc_set_error("hulc_bind_params: action_decoder.rnn.0 must be Linear(%d, 2048)", KIN); return 1; }
            } else {
            wih0_32 = pw(ad + "rnn.weight_ih_l0"); dwih0 = gw(ad + "rnn.weight_ih_l0");
            bih0 = pw(ad + "rnn.bias_ih_l0"); bhh0 = pw(ad + "rnn.bias_hh_l0"); bih1 = pw(ad + "rnn.bias_ih_l1"); bhh1 = pw(ad + "rnn.bias_hh_l1");
            dbih0 = gw(ad + "rnn.bias_ih_l0"); dbhh0 = gw(ad + "rnn.bias_hh_l0"); dbih1 = gw(ad + "rnn.bias_ih_l1"); dbhh1 = gw(ad + "rnn.bias_hh_l1");
            }
            wih0 = std::is_same<T, float>::value ? (T*)wih0_32 : wshadow + (wih0_32 - P);
            if (!wih0T) wih0T = alloc<T>((int64_t)HID * KIN);
            add_tr(wih0_32, wih0, wih0T, HID, KIN);
            if (mlp) {
                bind_lin(mlp1, ad + "rnn.2", HID, HID);
                bind_lin(mlp2, ad + "rnn.4", HID, HID);
            } else {
            bind_lin(whh0, ad + "rnn.weight_hh_l0", HID, HID, false);
            bind_lin(wih1, ad + "rnn.weight_ih_l1", HID, HID, false);
            bind_lin(whh1, ad + "rnn.weight_hh_l1", HID, HID, false);
            }
            if (!det) add_tr_packed(wheads, wheadsT, NHEAD, HID);      // the packed heads' transposed copy rides on the batched transpose as well
            const char* hn[4] = {"prob_fc", "mean_fc", "log_scale_fc", "gripper_fc"};
            for (int i = 0; i < 4; ++i) { head_w32[i] = head_b32[i] = nullptr; head_dw[i] = head_db[i] = nullptr; }
            if (det) {
                det_w32 = pw(ad + "actions.0.weight"); det_b32 = pw(ad + "actions.0.bias"); det_dw = gw(ad + "actions.0.weight"); det_db = gw(ad + "actions.0.bias");
                if (tab.at(ad + "actions.0.weight").n != (int64_t)DET_OUT * HID || tab.at(ad + "actions.0.bias").n != DET_OUT) {
                    hulc_set_error("hulc_bind_params: action_decoder.actions.0 must be Linear(2048, 7)"); return 1; }
                det_w = std::is_same<T, float>::value ? (const T*)det_w32 : (const T*)(wshadow + (det_w32 - P));
            }
            for (int i = 0; i < (det ? 0 : (mcil ? 3 : 4)); ++i) {
                head_w32[i] = pw(ad + hn[i] + ".weight"); head_b32[i] = pw(ad + hn[i] + ".bias");
                head_dw[i] = gw(ad + hn[i] + ".weight"); head_db[i] = gw(ad + hn[i] + ".bias");
            }
            if (cfg.use_clip || aux_mia) {      // the MIA head scores the same projections (hulc.py:621): proj_vis_lang.* without logit_scale when the CLIP loss is off
                bind_lin(cl_im0, "proj_vis_lang.mlp_im.0", 128, FCH); bind_lin(cl_im2, "proj_vis_lang.mlp_im.2", GOAL, 128);
                bind_lin(cl_la0, "proj_vis_lang.mlp_lang.0", 128, GOAL); bind_lin(cl_la2, "proj_vis_lang.mlp_lang.2", GOAL, 128);
            }
            if (cfg.use_clip) { logit_scale = pw("logit_scale"); dlogit_scale = gw("logit_scale"); }
            if (aux_bcz) { bind_lin(bz0, "bc_z_lang_decoder.mlp.0", 512, FCH); bind_lin(bz2, "bc_z_lang_decoder.mlp.2", LANG, 512); }
            if (aux_mia) {
                const std::string md = "mia_lang_discriminator.mlp.";
                mia_w0 = pw(md + "0.weight"); mia_b0 = pw(md + "0.bias"); mia_w1 = pw(md + "3.weight"); mia_b1 = pw(md + "3.bias");
                d_mia_w0 = gw(md + "0.weight"); d_mia_b0 = gw(md + "0.bias"); d_mia_w1 = gw(md + "3.weight"); d_mia_b1 = gw(md + "3.bias");
                if (tab.at(md + "0.weight").n != (int64_t)MIA_H * MIA_IN || tab.at(md + "0.bias").n != MIA_H || tab.at(md + "3.weight").n != MIA_H || tab.at(md + "3.bias").n != 1) {
                    hulc_set_error("hulc_bind_params: mia_lang_discriminator.* must be Linear(64, 512) and Linear(512, 1)"); return 1; }
            }
        } catch (const std::out_of_range&) {
            hulc_set_error("hulc_bind_params: a required parameter name is missing from the table");
            return 1;
        }
        // the weight gradients every writer of which can STORE (see LazyG): the M = B MLPs and the decoder's 2048^2 recurrent / layer-1 input weights
        for (int i = 0; i < 5; ++i) lazy_register(pp[i]);
        for (int i = 0; i < 3; ++i) { lazy_register(vg[i]); lazy_register(lg[i]); }
        lazy_register(pr_fs); lazy_register(whh0); lazy_register(whh1); lazy_register(wih1);      // feed-forward body: the three are unbound (dW null) and lazy_register skips them
        if (mlp) { lazy_register(mlp1); lazy_register(mlp2); }      // their only writer is lin_wgrad
        std::sort(lazy.begin(), lazy.end(), [](const LazyG& a, const LazyG& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < lazy.size(); ++i) if (lazy[i].off + lazy[i].n > lazy[i + 1].off) { lazy.clear(); break; }      // overlapping views: no lazy set
        if (blk2desc_dev) { hipFree(blk2desc_dev); blk2desc_dev = nullptr; }
        {
            std::vector<unsigned short> b2d((size_t)std::max(tr_blocks, 1));
            for (size_t i = 0; i < trdesc.size(); ++i) {
                const int end = i + 1 < trdesc.size() ? trdesc[i + 1].blk0 : tr_blocks;
                for (int b = trdesc[i].blk0; b < end; ++b) b2d[b] = (unsigned short)i;
            }
            if (hipMalloc((void**)&blk2desc_dev, b2d.size() * sizeof(unsigned short)) != hipSuccess) alloc_failed = true;
            else hipMemcpy(blk2desc_dev, b2d.data(), b2d.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
        }
        if (trdesc_dev) { hipFree(trdesc_dev); trdesc_dev = nullptr; }
        if (hipMalloc((void**)&trdesc_dev, sizeof(TrDesc) * trdesc.size()) != hipSuccess) alloc_failed = true;
        else hipMemcpy(trdesc_dev, trdesc.data(), sizeof(TrDesc) * trdesc.size(), hipMemcpyHostToDevice);
        adam_tables_build();
        if (alloc_failed) { hulc_set_error("hipMalloc failed while allocating weight copies"); return 1; }
        if ((clip_algo == HULC_CLIP_NORM || clip_track) && gn_build()) return 1;      // the norm pass's chunk table belongs to this tensor table
        bound = true;
        return prepare_weights();
    }

    HeadPack head_pack() const {
        HeadPack hp;
        for (int i = 0; i < 4; ++i) { hp.w[i] = head_w32[i]; hp.b[i] = head_b32[i]; hp.dw[i] = head_dw[i]; hp.db[i] = head_db[i]; hp.rows[i] = head_rows[i]; }
        return hp;
    }
    // ---------------------------------------------------------------- small launch helpers
    template <typename TS, typename TD>
    void cast_tr(const TS* src, long long lds_, TD* dst, long long ldd, TD* dstT, long long ldt, int R, int C) {
        dim3 grid(cdiv(C, 32), cdiv(R, 32));
        hipLaunchKernelGGL((cast_transpose_kernel<TS, TD>), grid, dim3(256), 0, st, src, lds_, dst, ldd, dstT, ldt, R, C);
    }
    static int ldpad(int m) { return (m + 7) / 8 * 8; }
    // dstA[c][r] = srcA[r][c] and dstB likewise, one launch
    void transpose_pair(const T* a, long long lda, T* at, int Ra, int Ca, const T* b, long long ldb, T* bt, int Rb, int Cb, long long ldt,
                        float* cs = nullptr, float* cs2 = nullptr) {
        TrPair p;
        p.d[0].cs = cs; p.d[0].cs2 = cs2;
        if (cs && Ra > TRT) nd(ND_TRANSPOSE_COLSUM);
        p.d[0].src = a; p.d[0].dst = at; p.d[0].lds = lda; p.d[0].ldt = ldt; p.d[0].R = Ra; p.d[0].C = Ca; p.d[0].tiles_x = cdiv(Ca, TRT); p.d[0].blk0 = 0;
        const int n0 = p.d[0].tiles_x * cdiv(Ra, TRT);
        p.d[1].src = b; p.d[1].dst = bt; p.d[1].lds = ldb; p.d[1].ldt = ldt; p.d[1].R = Rb; p.d[1].C = Cb; p.d[1].tiles_x = cdiv(Cb, TRT); p.d[1].blk0 = n0;
        const dim3 grid(n0 + p.d[1].tiles_x * cdiv(Rb, TRT));
        if constexpr (std::is_same<T, float>::value) hipLaunchKernelGGL((pair_transpose_kernel<T>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL(pair_transpose64_kernel, grid, dim3(256), 0, st, p);
    }
    // 16-bit engines: three transposes, one launch (dst leading dimension ldt for all; cs / cs2 = fused column sums of the FIRST source)
    void transpose_triple(const T* a, long long lda, T* at, int Ra, int Ca, const T* b, long long ldb, T* bt, int Rb, int Cb, const T* c, long long ldc, T* ct, int Rc, int Cc,
                          long long ldt, float* cs = nullptr, float* cs2 = nullptr) {
        if constexpr (!std::is_same<T, float>::value) {
            TrMulti m{}; m.n = 3;
            const T* src[3] = {a, b, c}; T* dst[3] = {at, bt, ct}; const long long ld[3] = {lda, ldb, ldc}; const int R[3] = {Ra, Rb, Rc}, C[3] = {Ca, Cb, Cc};
            int blk = 0;
            for (int i = 0; i < 3; ++i) {
                m.d[i].src = src[i]; m.d[i].dst = dst[i]; m.d[i].lds = ld[i]; m.d[i].ldt = ldt; m.d[i].R = R[i]; m.d[i].C = C[i]; m.d[i].tiles_x = cdiv(C[i], TRT); m.d[i].blk0 = blk;
                blk += m.d[i].tiles_x * cdiv(R[i], TRT);
            }
            m.d[0].cs = cs; m.d[0].cs2 = cs2;
            if (cs && Ra > TRT) nd(ND_TRANSPOSE_COLSUM);
            hipLaunchKernelGGL(multi_transpose64_kernel, dim3(blk), dim3(256), 0, st, m);
        }
    }
    template <typename TS, typename TD>
    void copy2d(const TS* src, long long lds_, TD* dst, long long ldd, int R, int C, int acc, float scale = 1.f) {
        hipLaunchKernelGGL((copy2d_kernel<TS, TD>), dim3(cdiv((long long)R * C, 256)), dim3(256), 0, st, src, lds_, dst, ldd, R, C, acc, scale);
    }
    void colsum(const T* x, long long ld, int M, int N, float* out, float* out2 = nullptr, float scale = 1.f) {
        if (ld == N && (N == 32 || N == 64) && M >= 4096) {          // conv bias grads: flat 16-byte streaming
            const int nblk = 256;
            hipLaunchKernelGGL((colsum_flat_kernel<T>), dim3(nblk), dim3(256), 0, st, x, (long long)M * N, N, cspart);
            hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(N, 64)), dim3(256), 0, st, cspart, nblk, N, out, out2, scale);
            return;
        }
        const int nsplit = std::max(1, std::min(256, cdiv(M, 256)));
        const int rps = cdiv(M, nsplit);
        if (std::is_same<T, float>::value || repro) {
            // fp32 (parity) mode and the reproducible mode: two-stage, fixed order
            hipLaunchKernelGGL((colsum_kernel<T>), dim3(cdiv(N, 64), nsplit), dim3(256), 0, st, x, ld, M, N, cspart, rps, 0, 1.f, (float*)nullptr);
            hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(N, 64)), dim3(256), 0, st, cspart, nsplit, N, out, out2, scale);
        } else {
            // bf16 (bench) mode: one launch, each row chunk adds its column sums with fp32 atomics
            if (nsplit > 1) nd(ND_COLSUM_ROWS);
            hipLaunchKernelGGL((colsum_kernel<T>), dim3(cdiv(N, 64), nsplit), dim3(256), 0, st, x, ld, M, N, out, rps, 2, scale, out2);
        }
    }
    // dense NT GEMM with tile selection
    void gemm(const DenseLoader<T>& a, const DenseLoader<T>& b, const DenseOut& om, const EpiP& ep, int M, int N, int K) {
        const double fl = 2.0 * M * N * K, by = ((double)M * K + (double)N * K + (double)M * N) * sizeof(T);
        const GemmPick pick = gemm_pick<T>(a, b, ep, M, N, K);      // gemm.h: the tile and kernel decision
        if (pick == GEMM_PICK_SKINNY) {
            // two roles share the skinny kernels: M <= 64 layers stream a whole weight matrix per launch (weight-bound), many-row GEMMs
            // (small-N heads / weight gradients with K = 2048) stream activations
            TimerScope ts(this, M <= 64 ? "skinny_gemm_m64" : "skinny_gemm_rows", "hbm", fl, by);
            gemm_launch_picked<T>(st, pick, a, b, om, ep, M, N, K);
        } else if (gemm_pick_tile(pick) == 128) {
            TimerScope ts(this, "gemm_128x128", "mfma", fl, by);
            gemm_launch_picked<T>(st, pick, a, b, om, ep, M, N, K);
        } else gemm_launch_picked<T>(st, pick, a, b, om, ep, M, N, K);
    }
    // dW[M][N] += A[M][K] B[N][K]^T with fp32 accumulate; few output tiles + long K -> split K across workgroups (atomics)
    void gemm_wgrad(const DenseLoader<T>& a, const DenseLoader<T>& b, float* dW, long long lddw, int M, int N, int K) {
        EpiP ep = epi(dW, true); ep.accumulate = 1;
        if constexpr (std::is_same<T, h16_t>::value) {
            if (a.R1 == 0x7fffffff && b.R1 == 0x7fffffff && skinny_ok(M, N, K, a.s1, b.s1, a.p, b.p)) { gemm(a, b, dense_out(lddw), ep, M, N, K); return; }
        }
        bool big = false;
        const int nsplit = gemm_wgrad_nsplit<T>(M, N, K, &big);      // gemm.h
        if (nsplit <= 1) { gemm(a, b, dense_out(lddw), ep, M, N, K); return; }
        if (repro) {
            // the same K split, but every slice stores its own fp32 slab [M][N] (gemm_kernel's z_stride form) in the idle part of the slab arena and one
            // launch adds the slabs to dW in slice order; without room for the slabs the product runs unsplit
            const long long zs = ((long long)M * N + 3) / 4 * 4;
            if (part_cur + zs * nsplit > this->partcap) { gemm(a, b, dense_out(lddw), ep, M, N, K); return; }
            float* const slabs = this->part + part_cur;
            EpiP es = epi(slabs, true); es.z_stride = zs;
            TimerScope ts(this, big ? "gemm_128x128" : "gemm_64x64_splitk", "mfma", 2.0 * M * N * K, ((double)M * K + (double)N * K) * sizeof(T) + 4.0 * M * N * nsplit);
            if (big) launch_gemm<T, 128, 128>(st, a, b, dense_out(N), es, M, N, K, 1, nsplit);
            else launch_gemm<T, 64, 64>(st, a, b, dense_out(N), es, M, N, K, 1, nsplit);
            const int vec = (N & 3) == 0 && (lddw & 3) == 0 && ((uintptr_t)slabs & 15) == 0 && ((uintptr_t)dW & 15) == 0;
            hipLaunchKernelGGL(slab_sum_kernel, dim3(cdiv((long long)M * N, vec ? 1024 : 256)), dim3(256), 0, st, (const float*)slabs, nsplit, zs, M, N, dW, lddw, vec);
            return;
        }
        nd(ND_GEMM_SPLITK);
        ep.atomic = 1;
        TimerScope ts(this, big ? "gemm_128x128" : "gemm_64x64_splitk", "mfma", 2.0 * M * N * K, ((double)M * K + (double)N * K) * sizeof(T) + 4.0 * M * N);
        if (big) launch_gemm<T, 128, 128>(st, a, b, dense_out(lddw), ep, M, N, K, 1, nsplit);
        else launch_gemm<T, 64, 64>(st, a, b, dense_out(lddw), ep, M, N, K, 1, nsplit);
    }
    EpiP epi(void* out, bool f32) const { EpiP e; e.out = out; e.out_f32 = f32 ? 1 : 0; e.generic_only = epilogue_fast ? 0 : 1; return e; }

    // Y[M][N] = X[M][K] W^T (+bias) ...
    void lin_fwd(const T* X, long long ldx, int M, const LinW& L, EpiP ep, long long ldo) {
        if (!ep.bias) ep.bias = L.b32;
        gemm(dense<T>(X, M, ldx), dense<T>(L.W, L.N, L.K), dense_out(ldo), ep, M, L.N, L.K);
    }
    // weight + bias grads of Y = X W^T: dW[N][K] += dY^T X ; db += colsum(dY).  dY [M][N] dense, X [M][K] (ldx)
    void lin_wgrad(const T* dY, const T* X, long long ldx, int M, int N, int K, float* dW, long long lddw, float* db, float* db2 = nullptr) {
        if constexpr (std::is_same<T, h16_t>::value) {
            if (M <= 64) {          // one fused launch: tr-read wgrad + bias grad, no transposed copies
                hipLaunchKernelGGL(lin_bwd_smallm_kernel, dim3(cdiv(N, 64), cdiv(K, 128)), dim3(256), 0, st, dY, (long long)N, X, ldx, M, N, K, dW, lddw, db, db2, grad_first(dW) ? 1 : 0);
                return;
            }
            grad_ensure_zero(dW);      // the paths below accumulate
        }
        const int mp = ldpad(M);
        const bool fuse_cs = std::is_same<T, h16_t>::value && !repro;     // bf16 (bench) mode: the dY transpose also adds its column sums into db (atomics)
        transpose_pair(dY, N, tA, M, N, X, ldx, tB, M, K, mp, fuse_cs ? db : nullptr, fuse_cs ? db2 : nullptr);
        gemm_wgrad(dense<T>(tA, N, mp), dense<T>(tB, K, mp), dW, lddw, N, K, M);
        if (db && !fuse_cs) colsum(dY, N, M, N, db, db2);
    }
    // dX[M][K] = dY[M][N] W   (via the transposed copy Wt [K][N])
    void lin_dgrad(const T* dY, int M, const LinW& L, EpiP ep, const DenseOut& om) {
        gemm(dense<T>(dY, M, L.N), dense<T>(L.Wt, L.K, L.N), om, ep, M, L.K, L.N);
    }
    // the LayerNorm launches and their decisions live in plan_ln_launch.h (shared with the test entries of k_entries.h), like every other kernels.h launch helper
    void ln_fwd(const float* x, long long ldx, int rows, int n, const float* g, const float* b, T* out, long long ldo, float* outf, long long ldf,
                float* stats) {
        launch_ln_fwd<T>(st, x, ldx, rows, n, g, b, out, ldo, outf, ldf, stats);
    }
    // bcast_rows > 0 (fused kernel only, see ln_bwd_can_bcast): dy holds one row per WINDOW, broadcast over its bcast_rows rows and divided by bcast_div
    static constexpr bool ln_bwd_can_bcast = ln_bwd_fused<T>();
    void ln_bwd(const float* dy, long long lddy, const float* x, long long ldx, const float* stats, const float* g, int rows, int n, float* dxf,
                long long ldd, int acc, T* dxt, long long ldt, float* dg, float* db, float drop_p = 0.f, unsigned long long drop_seed = 0,
                int bcast_rows = 0, float bcast_div = 1.f, int dy_parts = 1, long long dy_part_stride = 0) {
        if (ln_bwd_fused<T>() && !repro && dg && cdiv(rows, ln_bwd_rows_per_block(rows)) > 1) nd(ND_LN_PARAM);
        launch_ln_bwd<T>(st, cspart, dy, lddy, x, ldx, stats, g, rows, n, dxf, ldd, acc, dxt, ldt, dg, db, drop_p, drop_seed, bcast_rows, bcast_div, dy_parts, dy_part_stride, repro);
    }

    // ---------------------------------------------------------------- weight preparation
    // compute-precision copies: (bf16) flat shadow cast, ONE batched launch for every transposed Linear weight, conv packs, the
    // NHWC-permuted gripper fc and the packed decoder heads
    int prepare_weights(bool shadow_fresh = false) override {
        if (!bound) { hulc_set_error("hulc_prepare_weights before hulc_bind_params"); return 1; }
        // under a trainable mask the refresh behind an optimizer step leaves every copy of a frozen tensor alone (an explicit hulc_prepare_weights refreshes all)
        const bool masked = shadow_fresh && tm_active;
        if (masked && tm_ntrain == 0) return 0;
        c1_bias_fold_valid = false;
        if constexpr (!std::is_same<T, float>::value) {
            if (!shadow_fresh) hipLaunchKernelGGL((cast_kernel<float, T>), dim3(2048), dim3(256), 0, st, P, wshadow, (long long)numel);
        }
        {      // the six conv weight packs, the gripper fc7's NHWC column permutation and the packed decoder heads: one launch (weight_pack_kernel) ...
            ConvPackBatch d;
            int k = 0, blk = 0;
            for (EncW* e : {&encS, &encG})
                for (ConvW* c : {&e->c1, &e->c2, &e->c3}) {
                    d.w[k] = c->W32; d.wf[k] = c->Wf; d.wd[k] = c->nhwc ? c->Wd : nullptr; d.O[k] = (masked && !tm_trainable_w(c->W32)) ? 0 : c->O; d.I[k] = c->I; d.K[k] = c->KH; d.S[k] = c->S; d.nhwc[k] = c->nhwc;
                    d.blk0[k] = blk; blk += cdiv(c->O * c->I * c->KH * c->KW, 256); ++k;
                }
            d.blk0[6] = blk;
            const int blkA = blk, blkB = blkA + cdiv(128 * 3136, 256);
            // packed heads [192][2048]: prob | mean | log_scale | gripper | zero pad
            HeadPack hp = head_pack();
            const int rows = head_rows[0] + head_rows[1] + head_rows[2] + head_rows[3];
            const int r7 = (masked && !tm_trainable_w(encG.fc7.W32)) ? 0 : 128;      // zero rows: the blocks of a frozen job return without a store
            if (masked && !heads_trainable()) for (int i = 0; i < 4; ++i) hp.rows[i] = 0;
            // 16-bit engines: the transposed copies of the two packed matrices are written by this launch too (rest_by_pack: then no transpose launch is left behind Adam)
            T* const f7t = rest_by_pack ? encG.fc7.Wt : (T*)nullptr;
            T* const wht = rest_by_pack ? wheadsT : (T*)nullptr;
            hipLaunchKernelGGL((weight_pack_kernel<T>), dim3(blkB + cdiv((long long)rows * HID, 256)), dim3(256), 0, st, d, blkA, encG.fc7.W32, encG.fc7.W, r7, 64, 49, blkB, hp,
                               wheads, bheads, HID, f7t, wht, NHEAD);
        }
        // ... then every transposed copy — the Linear weights, the permuted fc7 and the packed heads — in ONE batched launch
        if (masked) {
            if (std::is_same<T, float>::value) { if (tm_tr_all.blocks) hipLaunchKernelGGL((batched_transpose_kernel<float, T>), dim3(tm_tr_all.blocks), dim3(256), 0, st, (const TrDesc*)tm_tr_all.desc, tm_tr_all.n); }
            else if (tr_fresh) { if (tm_tr_rest.blocks && !rest_by_pack) hipLaunchKernelGGL(batched_transpose64_kernel, dim3(tm_tr_rest.blocks), dim3(256), 0, st, (const TrDesc*)tm_tr_rest.desc, tm_tr_rest.n, (const unsigned short*)tm_tr_rest.b2d); }
            else if (tm_tr_all.blocks) hipLaunchKernelGGL(batched_transpose64_kernel, dim3(tm_tr_all.blocks), dim3(256), 0, st, (const TrDesc*)tm_tr_all.desc, tm_tr_all.n, (const unsigned short*)tm_tr_all.b2d);
        }
        else if (std::is_same<T, float>::value) hipLaunchKernelGGL((batched_transpose_kernel<float, T>), dim3(tr_blocks), dim3(256), 0, st, trdesc_dev, (int)trdesc.size());
        else if (tr_fresh && tr_adam.n) {      // the optimizer wrote the shadow-sourced transposed copies (adam_tiled_kernel): only the packed sources are left
            if (tr_rest.blocks && !rest_by_pack) hipLaunchKernelGGL(batched_transpose64_kernel, dim3(tr_rest.blocks), dim3(256), 0, st, tr_rest.desc, tr_rest.n, (const unsigned short*)tr_rest.b2d);
        }
        else hipLaunchKernelGGL(batched_transpose64_kernel, dim3(tr_blocks), dim3(256), 0, st, trdesc_dev, (int)trdesc.size(), (const unsigned short*)blk2desc_dev);
        const bool was_fresh = tr_fresh && tr_adam.n;
        tr_fresh = false;
        if constexpr (std::is_same<T, h16_t>::value) {
            // (the optimizer's tile pass wrote them when every frag job is linked to a tiled descriptor: frag_by_adam)
            if (masked) { if (tm_frag.n && !(was_fresh && frag_by_adam)) hipLaunchKernelGGL(frag_pack_kernel, dim3(tm_frag_blocks), dim3(256), 0, st, tm_frag); }
            else if (fragbatch.n && !(was_fresh && frag_by_adam)) hipLaunchKernelGGL(frag_pack_kernel, dim3(frag_blocks), dim3(256), 0, st, fragbatch);
        }
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in prepare_weights"); return 1; }
        return 0;
    }
    // grads_fresh: the gradient buffer is all zeros (hulc_zero_grads was the last thing that touched it).  The first backward after it may STORE
    // the weight gradients that have a single whole-tensor contribution instead of reading the zeros back and adding (200 MB of reads per step):
    // 0 + x == x exactly, so the result is bit-identical.  A second backward before the next zero_grads (one pass per modality) accumulates.
    // ---- deferred Linear weight / bias gradients (16-bit engines).  Nothing in a backward reads a weight gradient before its all-reduce bucket, the end of the
    // backward or the optimizer, so part 0 only QUEUES them (wq_add: the decoder heads, every M = B MLP layer, fc_state / fc of the plan recognition, the eight
    // transformer Linears) and wq_flush runs the queue as two launches at the end of part 0 — the M <= 64 jobs in lin_bwd_smallm_batched_kernel (one row step,
    // write-bound), the many-row jobs in lin_bwd_stream_kernel — instead of seven dependent launches behind their data-gradient GEMMs plus two slab sums.  dY and X
    // of a queued job must stay untouched until the flush: forward activations and gradient buffers of their own (trb_*, mlp_dy sets, dheads, dprl_t, dseq_t, ...).
    // With a collective armed (ar_dtype >= 0) bucket_ready flushes before it puts a bucket on the wire.  The lazy-zero state of a target (grad_first) is read at
    // flush time, when the launch that stores or adds is actually enqueued.
    T *trb_c[2] = {nullptr, nullptr}, *trb_a[2] = {nullptr, nullptr}, *trb_d[2] = {nullptr, nullptr}, *trb_b[2] = {nullptr, nullptr};
    struct WqJob { const T* dY; const T* X; long long ldx, lddw; int M, N, K; float* dW; float* db; bool heads; };
    std::vector<WqJob> wq;
    // row ranges of a many-row job: one (no slab, the workgroup writes dW itself) when the launch has at least a workgroup for every second CU anyway, else two
    static int lin_stream_nsplit(int tiles, int M) { return (M > 256 && tiles < 128) ? 2 : 1; }
    // the M = B layers outside the MLP helper join the queue in the row range their one-launch form (lin_wgrad) covers; more rows keep lin_wgrad's transposed GEMM
    bool wq_small(int M) const { return std::is_same<T, h16_t>::value && M <= 64; }
    void wq_add(const T* dY, const T* X, long long ldx, int M, int N, int K, float* dW, long long lddw, float* db, bool heads = false) {
        wq.push_back(WqJob{dY, X, ldx, lddw, M, N, K, dW, db, heads});
    }
    void wq_add(const T* dY, const T* X, int M, const LinW& L) {
        if constexpr (std::is_same<T, h16_t>::value) {
            if (M <= 64 || lin_stream_ok(dY, X, L.K, L.N)) { wq_add(dY, X, L.K, M, L.N, L.K, L.dW, L.K, L.db); return; }
        }
        lin_wgrad(dY, X, L.K, M, L.N, L.K, L.dW, L.K, L.db);      // rows the streaming body's DMA cannot fetch: the transposed GEMM, at once
    }
    void wq_flush() {
        if constexpr (std::is_same<T, h16_t>::value) {
            if (wq.empty()) return;
            int tiles = 0;
            for (const WqJob& q : wq) if (q.M > 64) tiles += cdiv(q.N, 64) * cdiv(q.K, 128);
            LinBwdBatch ob{}; int oblk = 0;
            LinStreamBatch sb{}; int sblk = 0;
            auto run_one = [&]() { if (ob.n) hipLaunchKernelGGL(lin_bwd_smallm_batched_kernel, dim3(oblk), dim3(256), 0, st, ob); ob.n = 0; oblk = 0; };
            auto run_str = [&]() { launch_lin_stream(st, sb, sblk); sb.n = 0; sblk = 0; };
            const WqJob* hj = nullptr; int hsplit = 1; bool hcolsum = false;
            for (const WqJob& q : wq) {
                if (q.M <= 64) {
                    if (ob.n == LBS_MAX_JOBS) run_one();
                    LinBwdJob& J = ob.j[ob.n++];
                    J.dY = q.dY; J.X = q.X; J.dW = q.dW; J.db = q.db; J.ldx = q.ldx; J.lddw = q.lddw; J.M = q.M; J.N = q.N; J.K = q.K; J.nx = cdiv(q.N, 64); J.blk0 = oblk;
                    J.store = grad_first(q.dW) ? 1 : 0;
                    oblk += J.nx * cdiv(q.K, 128);
                    continue;
                }
                if (sb.n == LBT_MAX_JOBS) run_str();
                if (q.heads) {      // the packed heads: slab(s) at the start of the (idle) convolution slab arena, re-packed into the four tensors by unpack_heads_grad_kernel below
                    hj = &q; hsplit = lin_stream_nsplit(tiles, q.M);
                    if (part_cur + (int64_t)hsplit * q.N * q.K > this->partcap) hsplit = 1;      // (room for one slab was checked when the job was queued)
                    hcolsum = repro && hsplit > 1;      // reproducible mode: the two ranges' bias sums would land with atomics -> two-stage column sum instead
                    if (hsplit > 1 && !repro) nd(ND_LIN_BWD_ROWS);
                    lin_stream_add(sb, sblk, (const h16_t*)q.dY, (const h16_t*)q.X, q.ldx, q.M, q.N, q.K, nullptr, q.lddw, hcolsum ? nullptr : q.db, this->part + part_cur, hsplit, 1);
                } else lin_stream_add(sb, sblk, (const h16_t*)q.dY, (const h16_t*)q.X, q.ldx, q.M, q.N, q.K, q.dW, q.lddw, q.db, nullptr, 1, grad_first(q.dW) ? 1 : 0);
            }
            run_one(); run_str();
            if (hj) {
                if (hcolsum) colsum(hj->dY, hj->N, hj->M, hj->N, hj->db);
                const HeadPack hp = head_pack();
                const int rows = head_rows[0] + head_rows[1] + head_rows[2] + head_rows[3];
                hipLaunchKernelGGL(unpack_heads_grad_kernel, dim3(cdiv((long long)rows * HID, 256)), dim3(256), 0, st, hp, (const float*)(this->part + part_cur), (const float*)hj->db, HID, hsplit, (long long)hj->N * hj->K);
            }
            wq.clear();
        }
    }
    float* dparts = nullptr;                // fused FFN backward: the four hidden-quarter partials of the gradient entering norm1
    h16_t* dump_page = nullptr;             // conv_reg.h EPI form: scratch that receives the stores of pixels which must not be written
    bool grads_fresh = false;
    int wacc() const { return grads_fresh ? 0 : 1; }
    // ---- lazily zeroed weight gradients (round 5, VERDICT r4 #8 ii; 16-bit engines).  hulc_zero_grads used to memset all 188 MB (24.5 us) although the
    // first backward STORES the large Linear weight gradients (0 + x == x).  Now the tensors whose every writer can store (`lazy`: the M = B MLPs'
    // weights through lin_wgrad / mlp_bwd, the decoder's recurrent / layer-1 input weights through their 2048^3 GEMMs) are only MARKED stale by
    // zero_grads and everything else is zeroed by one multi-range launch.  A stale tensor is made valid by whoever touches it first:
    //   * a store-capable site asks grad_first(dW): stale -> it stores (and the mark is cleared); not stale -> it accumulates as before;
    //   * an accumulate-only path calls grad_ensure_zero(dW) first;
    //   * what is still stale when its all-reduce bucket is issued, at the end of the backward, or when the optimizer / a whole-buffer all-reduce
    //     runs (a tensor the step never touched: language_goal.* in a vision-only step) is zeroed then (lazy_sweep).
    // So the buffer the caller sees after hulc_backward is exactly what the full memset produced; between hulc_zero_grads and the next backward the
    // lazy tensors hold the previous step's values (hulc_set_option "lazy_zero_grads" 0 restores the plain memset).
    struct LazyG { int64_t off, n; bool stale; };
    std::vector<LazyG> lazy;
    void lazy_register(const LinW& L) {
        if (!std::is_same<T, h16_t>::value || !L.dW || (int64_t)L.N * L.K < 65536) return;
        const int64_t off = L.dW - G, exact = (int64_t)L.N * L.K;
        int64_t n = (exact + 63) / 64 * 64;
        // the rounded range may cover alignment padding only: never the first elements of the next tensor of a tightly packed layout
        for (const auto& kv : tab_order) if (kv.second.off > off && kv.second.off < off + n) n = exact;
        if (off + n > numel) n = exact;
        if (n % 4 || off % 4) return;      // multi_zero_kernel clears 16-byte pieces
        for (const LazyG& z : lazy) if (z.off == off) return;
        if (lazy.size() < 30 && off >= 0 && off + n <= numel) lazy.push_back(LazyG{off, n, false});
    }
    int lazy_find(const float* dW) const { const int64_t off = dW - G; for (size_t i = 0; i < lazy.size(); ++i) if (lazy[i].off == off) return (int)i; return -1; }
    // store-capable writer of dW: true = STORE
    bool grad_first(const float* dW) {
        const int i = lazy_find(dW);
        if (i < 0) return grads_fresh;
        const bool s = lazy[i].stale;
        lazy[i].stale = false;
        return s;
    }
    void grad_ensure_zero(const float* dW) {
        const int i = lazy_find(dW);
        if (i >= 0 && lazy[i].stale) { hipMemsetAsync(G + lazy[i].off, 0, sizeof(float) * lazy[i].n, st); lazy[i].stale = false; }
    }
    void lazy_sweep(int64_t lo, int64_t hi, hipStream_t s) {
        MultiZero mz{}; int k = 0; long long mx = 0;
        for (LazyG& z : lazy)
            if (z.stale && z.off >= lo && z.off + z.n <= hi) { mz.p[k] = G + z.off; mz.n[k] = z.n; mx = std::max<long long>(mx, z.n); ++k; z.stale = false; }
        if (k) hipLaunchKernelGGL(multi_zero_kernel, dim3((unsigned)std::min<long long>(256, cdiv(mx, 4 * 256 * 8)), k), dim3(256), 0, s, mz);
    }
    int flush_grads() override {
        if (!bound) { hulc_set_error("hulc_flush_grads before hulc_bind_params"); return 1; }
        lazy_sweep(0, numel, st);
        return 0;
    }
    int zero_grads() override {
        if (!bound) { hulc_set_error("hulc_zero_grads before hulc_bind_params"); return 1; }
        if (!have_fwd) repro_latch();      // a pending forward keeps its routing for its backward
        if (lazy.empty() || !lazy_zero_mode) {
            HIP_CHECK(hipMemsetAsync(G, 0, numel * sizeof(float), st));
            for (LazyG& z : lazy) z.stale = false;
        } else {
            // the complement of the lazy tensors, as <= 31 ranges in one launch
            MultiZero mz{}; int k = 0; long long mx = 0; int64_t cur = 0;
            auto add = [&](int64_t lo, int64_t hi) { if (hi > lo) { mz.p[k] = G + lo; mz.n[k] = hi - lo; mx = std::max<long long>(mx, hi - lo); ++k; } };
            for (LazyG& z : lazy) { add(cur, z.off); cur = z.off + z.n; z.stale = true; }
            add(cur, numel / 4 * 4);
            if (numel % 4) HIP_CHECK(hipMemsetAsync(G + numel / 4 * 4, 0, sizeof(float) * (numel % 4), st));
            if (k) hipLaunchKernelGGL(multi_zero_kernel, dim3((unsigned)std::min<long long>(256, cdiv(mx, 4 * 256 * 8)), k), dim3(256), 0, st, mz);
        }
        grads_fresh = true; bwd_since_opt = false;
        return 0;
    }

#include "engine_encoders.inc"      // the perceptual encoders: conv1 sources (fp32 / uint8 / frame store), conv2 / conv3 forward, data and weight gradients, spatial softmax, the fc tails
#include "engine_forward.inc"      // MLP helper, the forward pieces shared by training / validation / rollout, hulc_forward_loss and hulc_forward_loss_pair
#include "engine_inference.inc"      // validation forward (a20), the CLIP ground-truth metric, the stateful rollout
#include "engine_rollout_envs.inc"      // the batched multi-environment rollout: max_envs policy slots per context (rollout_step.h)
#include "engine_recurrent.inc"      // the 2048-wide recurrences: persistent launches (rnn_persist.h) with their probe / fallback protocol, the mcil BiRNN and BiGRU plan encoders (a12, a19)
#include "engine_trainable.inc"      // the per-tensor trainable mask: hulc_trainable_set / _get / _steps_set and the optimizer / refresh tables without the frozen tensors
#include "engine_ema.inc"      // the averaged weights: hulc_ema_enable / _state_get / _state_set / _swap, the update pass behind the optimizer kernel
#include "engine_backward.inc"      // gradient all-reduce buckets + the job-wide skip vote (comm.h), hulc_backward / hulc_backward_part / hulc_backward_allreduce (a16-a17)
    // ---------------------------------------------------------------- dynamic loss scaling (kernels.h: ScalerState)
    ScalerState* scaler = nullptr;          // device; null = off (fp32 / bf16 default)
    const float* lscale() const { return scaler ? &scaler->scale : nullptr; }
    int scaler_enable(float init_scale, float growth, float backoff, int interval) override {
        if (!(init_scale > 0.f)) { scaler = nullptr; return 0; }          // <= 0: off
        if (!(growth >= 1.f) || !(backoff > 0.f && backoff <= 1.f) || interval < 1) { hulc_set_error("hulc_scaler_enable: need growth >= 1, 0 < backoff <= 1, interval >= 1"); return 1; }
        if (!scaler_mem) { scaler_mem = alloc<ScalerState>(1); if (alloc_failed) { hulc_set_error("hulc_scaler_enable: allocation failed"); return 1; } }
        ScalerState h; memset(&h, 0, sizeof(h));
        h.scale = init_scale; h.growth = growth; h.backoff = backoff; h.interval = interval;
        HIP_CHECK(hipMemcpyAsync(scaler_mem, &h, sizeof(h), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        scaler = scaler_mem;
        return 0;
    }
    ScalerState* scaler_mem = nullptr;
    int scaler_get(float* scale, int32_t* tracker, int64_t* skipped, int32_t* last_inf, int64_t* taken) override {
        if (!scaler) { if (scale) *scale = 1.f; if (tracker) *tracker = 0; if (skipped) *skipped = 0; if (last_inf) *last_inf = 0; if (taken) *taken = 0; return 0; }
        ScalerState h;
        HIP_CHECK(hipMemcpyAsync(&h, scaler, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (scale) *scale = h.scale; if (tracker) *tracker = h.growth_tracker; if (skipped) *skipped = h.skipped; if (last_inf) *last_inf = h.last_found_inf; if (taken) *taken = h.steps;
        return 0;
    }
    // taken >= 0 also restores the count of optimizer steps actually taken — Adam's bias corrections run on it in fp16 mode (adam_kernel), so a
    // resumed run must get it back (torch keeps it as the optimizer state's `step`, which GradScaler.step never advances on a skipped step)
    int scaler_set(float scale, int32_t tracker, int64_t taken) override {
        if (!scaler) { hulc_set_error("hulc_scaler_set: the loss scaler is off (hulc_scaler_enable first)"); return 1; }
        if (!(scale > 0.f) || tracker < 0) { hulc_set_error("hulc_scaler_set: need scale > 0, growth_tracker >= 0"); return 1; }
        ScalerState h;
        HIP_CHECK(hipMemcpyAsync(&h, scaler, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        h.scale = scale; h.growth_tracker = tracker;
        if (taken >= 0) h.steps = (int)taken;
        HIP_CHECK(hipMemcpyAsync(scaler, &h, sizeof(h), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    // ---------------------------------------------------------------- gradient clipping / gradient norms (kernels.h: ClipState, grad_sumsq_kernel)
    std::vector<Ref> gn_tens;               // the bound tensors in bind order
    bool gn_built = false, gn_have = false; // tables match gn_tens / the last optimizer step computed norms
    int gn_chunks = 0;
    long long* gn_chunk_start = nullptr; int* gn_chunk_n = nullptr; int* gn_tfirst = nullptr; float* gn_partial = nullptr; double* gn_tsq = nullptr; float* gn_tnorm = nullptr;
    ClipState* clip_state = nullptr;        // device
    int clip_algo = HULC_CLIP_OFF; float clip_limit = 0.f; bool clip_track = false;
    void gn_free() {
        for (void* p : {(void*)gn_chunk_start, (void*)gn_chunk_n, (void*)gn_tfirst, (void*)gn_partial, (void*)gn_tsq, (void*)gn_tnorm}) if (p) hipFree(p);
        gn_chunk_start = nullptr; gn_chunk_n = nullptr; gn_tfirst = nullptr; gn_partial = nullptr; gn_tsq = nullptr; gn_tnorm = nullptr; gn_chunks = 0; gn_built = false;
    }
    // chunk table of the norm pass: every bound tensor cut into GN_CHUNK pieces; only listed elements, never the padding between tensors.  Built off the
    // step path: by hulc_bind_params when clipping by norm / tracking is already configured, else by the hulc_grad_clip_set that configures it
    int gn_build() {
        gn_free();
        std::vector<long long> cs; std::vector<int> cn, tf;
        for (size_t t = 0; t < gn_tens.size(); ++t) {
            const Ref& r = gn_tens[t];
            if (r.off < 0 || r.n < 0 || (r.off & 3) || r.off + r.n > numel) { hulc_set_error("gradient norm: tensor at offset %lld (%lld elements) is misaligned or outside the bound buffer", (long long)r.off, (long long)r.n); return 1; }
            tf.push_back((int)cs.size());
            if (tm_active && !tm_mask[t]) continue;      // a frozen tensor has no chunk: it is not read, adds nothing to the total and reports 0
            for (int64_t x = 0; x < r.n; x += GN_CHUNK) { cs.push_back(r.off + x); cn.push_back((int)std::min<int64_t>(GN_CHUNK, r.n - x)); }
        }
        tf.push_back((int)cs.size());
        if (cs.empty() && !tm_active) { hulc_set_error("gradient norm: no bound tensors"); return 1; }
        if (cs.empty()) { cs.push_back(0); cn.push_back(0); }      // every tensor frozen: one empty chunk behind the table (the step launches nothing)
        const size_t nc = cs.size(), nt = gn_tens.size();
        if (hipMalloc((void**)&gn_chunk_start, sizeof(long long) * nc) != hipSuccess || hipMalloc((void**)&gn_chunk_n, sizeof(int) * nc) != hipSuccess ||
            hipMalloc((void**)&gn_tfirst, sizeof(int) * (nt + 1)) != hipSuccess || hipMalloc((void**)&gn_partial, sizeof(float) * nc) != hipSuccess ||
            hipMalloc((void**)&gn_tsq, sizeof(double) * nt) != hipSuccess || hipMalloc((void**)&gn_tnorm, sizeof(float) * nt) != hipSuccess) {
            gn_free(); hulc_set_error("gradient norm: allocation failed"); return 1;
        }
        HIP_CHECK(hipMemcpy(gn_chunk_start, cs.data(), sizeof(long long) * nc, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(gn_chunk_n, cn.data(), sizeof(int) * nc, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(gn_tfirst, tf.data(), sizeof(int) * (nt + 1), hipMemcpyHostToDevice));
        gn_chunks = tf.back(); gn_built = true;
        return 0;
    }
    int clip_state_write(float total, float coef) {
        if (!clip_state && hipMalloc((void**)&clip_state, sizeof(ClipState)) != hipSuccess) { clip_state = nullptr; hulc_set_error("hulc_grad_clip_set: allocation failed"); return 1; }
        const ClipState h{total, coef, clip_algo, clip_limit};
        HIP_CHECK(hipMemcpyAsync(clip_state, &h, sizeof(h), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));          // `h` lives on this frame
        return 0;
    }
    int grad_clip_set(int32_t algo, float limit, int32_t track) override {
        if (algo != HULC_CLIP_OFF && algo != HULC_CLIP_NORM && algo != HULC_CLIP_VALUE) { hulc_set_error("hulc_grad_clip_set: unknown algorithm %d", (int)algo); return 1; }
        if (!(limit > 0.f)) algo = HULC_CLIP_OFF;      // Lightning: gradient_clip_val None / 0 = no clipping
        if ((algo == HULC_CLIP_NORM || track != 0) && bound && !gn_built && gn_build()) return 1;      // before a bind: hulc_bind_params builds the table
        clip_algo = algo; clip_limit = algo == HULC_CLIP_OFF ? 0.f : limit; clip_track = track != 0;
        gn_have = false;
        if (clip_algo == HULC_CLIP_OFF && !clip_track) return 0;
        return clip_state_write(0.f, 1.f);
    }
    int grad_norm_get(float* total, float* coef, float* per_tensor, int64_t cap) override {
        if (!gn_have) { hulc_set_error("hulc_grad_norm_get: no optimizer step has computed gradient norms (hulc_grad_clip_set with HULC_CLIP_NORM or track != 0 first)"); return 1; }
        if (per_tensor && cap < (int64_t)gn_tens.size()) { hulc_set_error("hulc_grad_norm_get: per-tensor buffer holds %lld values, %lld tensors are bound", (long long)cap, (long long)gn_tens.size()); return 1; }
        ClipState h;
        HIP_CHECK(hipMemcpyAsync(&h, clip_state, sizeof(h), hipMemcpyDeviceToHost, st));
        if (per_tensor) HIP_CHECK(hipMemcpyAsync(per_tensor, gn_tnorm, sizeof(float) * gn_tens.size(), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (total) *total = h.total_norm;
        if (coef) *coef = h.coef;
        return 0;
    }

    int optim(const hulc_optim& o) override {
        if (!bound) { hulc_set_error("hulc_optimizer_step before hulc_bind_params"); return 1; }
        if (ema_refuse("hulc_optimizer_step")) return 1;
        const bool want_norm = clip_algo == HULC_CLIP_NORM || clip_track;
        if (want_norm && !gn_built) { hulc_set_error("hulc_optimizer_step: the gradient-norm tables are missing (hulc_bind_params / hulc_grad_clip_set build them)"); return 1; }      // before the step tag advances
        // trainable mask: per-group numbers of this step (kernels.h OptGroups) — a tensor that sat out k steps is at its own step o.step - k
        OptGroups og{};
        if (tm_active && o.step >= 1) {
            for (int g = 0; g < tm_ngroups; ++g) {
                const int64_t own = o.step - tm_goff[g];
                if (!scaler && own < 1) { hulc_set_error("hulc_optimizer_step: step %lld, but a trainable tensor sat out %lld steps (hulc_trainable_steps_set)", (long long)o.step, (long long)tm_goff[g]); return 1; }
                og.bc1[g] = (float)(1.0 - pow((double)o.beta1, (double)own)); og.bc2_sqrt[g] = (float)sqrt(1.0 - pow((double)o.beta2, (double)own));
                og.off[g] = (int)tm_goff[g]; og.first[g] = own == 1;
            }
        }
        persist_check("hulc_optimizer_step", false);
        lazy_sweep(0, numel, st);            // an optimizer step without a backward behind hulc_zero_grads: the lazily zeroed tensors become zeros now
        bwd_since_opt = false;
        const unsigned tag = ++opt_seq;
        if (o.kind != HULC_OPT_ADAM && o.kind != HULC_OPT_ADAMW && o.kind != HULC_OPT_SGD) { hulc_set_error("hulc_optimizer_step: unknown optimizer kind %d", (int)o.kind); return 1; }
        if (o.step < 1) { hulc_set_error("hulc_optimizer_step: step counts from 1 (got %lld)", (long long)o.step); return 1; }
        const float lr = o.lr, b1 = o.beta1, b2 = o.beta2, eps = o.eps, gscale = o.grad_scale;
        const int64_t step = o.step;
        const double bc1d = 1.0 - pow((double)b1, (double)step), bc2d = 1.0 - pow((double)b2, (double)step);
        h16_t* const shadow = std::is_same<T, float>::value ? (h16_t*)nullptr : (h16_t*)wshadow;
        // after the all-reduce, whoever performed it: every rank sees the same flag and derives the same clipping coefficient from the same reduced buffer
        const ClipState* const cs = clip_algo != HULC_CLIP_OFF ? clip_state : nullptr;
        tm_last_step = step;      // what hulc_trainable_set converts a tensor's sat-out count and its own step count with
        if (tm_active) {
            if (tm_ntrain == 0) return 0;      // every tensor frozen: nothing is read, written or launched
            if (want_norm) {
                hipLaunchKernelGGL(grad_sumsq_kernel, dim3(gn_chunks), dim3(256), 0, st, (const float*)G, (const long long*)gn_chunk_start, (const int*)gn_chunk_n, gn_partial, scaler);
                hipLaunchKernelGGL(grad_norm_combine_kernel, dim3(1), dim3(1024), 0, st, (const float*)gn_partial, (const int*)gn_tfirst, (int)gn_tens.size(), gscale, (const ScalerState*)scaler,
                                   clip_state, gn_tsq, gn_tnorm);
                gn_have = true;
            } else if (scaler)      // the non-finite check reads the gradients the step will read, no others: the norm pass's chunk walk over the trainable tensors (its sums are not used)
                hipLaunchKernelGGL(grad_sumsq_kernel, dim3(gn_chunks), dim3(256), 0, st, (const float*)G, (const long long*)gn_chunk_start, (const int*)gn_chunk_n, gn_partial, scaler);
            if (o.kind == HULC_OPT_SGD)
                hipLaunchKernelGGL(sgd_grouped_kernel, dim3(tm_flat.chunks), dim3(256), 0, st, P, (const float*)G, AM, (const long long*)tm_flat.start, (const int*)tm_flat.n, (const unsigned char*)tm_flat.gid, og,
                                   lr, o.momentum, o.dampening, o.weight_decay, (int)(o.nesterov != 0), gscale, shadow, (const ScalerState*)scaler, (const unsigned*)rp_skip, tag, cs);
            else {
                const bool tiles = adam_fuse_tr && tm_tile_ok && tm_tiles.n && shadow;
                const ChunkTable& ct = tiles ? tm_comp : tm_flat;
                AdamArgs a{P, G, AM, AV, lr, b1, b2, eps, 1.f, 1.f, gscale, o.weight_decay, (int)(o.kind == HULC_OPT_ADAMW), shadow, (const ScalerState*)scaler, (const unsigned*)rp_skip, tag, cs};
                hipLaunchKernelGGL(adam_grouped_kernel, dim3((tiles ? tm_tiles.blocks : 0) + ct.chunks), dim3(256), 0, st, a, (const TrDesc*)(tiles ? tm_tiles.desc : nullptr),
                                   (const unsigned short*)(tiles ? tm_tiles.b2d : nullptr), (const unsigned char*)(tiles ? tm_tile_gid : nullptr), tiles ? tm_tiles.blocks : 0,
                                   (const long long*)ct.start, (const int*)ct.n, (const unsigned char*)ct.gid, og);
                if (tiles) tr_fresh = true;
            }
            if (ema) ema_step(tag);
            if (scaler) hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(1), 0, st, scaler, (const unsigned*)rp_skip, tag);
            if (hipGetLastError() != hipSuccess) { hulc_set_error("optimizer launch failed"); return 1; }
            return prepare_weights(true);
        }
        if (want_norm) {        // one read of G: the norm pass raises found_inf itself (fp16), the separate check is skipped
            hipLaunchKernelGGL(grad_sumsq_kernel, dim3(gn_chunks), dim3(256), 0, st, (const float*)G, (const long long*)gn_chunk_start, (const int*)gn_chunk_n, gn_partial, scaler);
            hipLaunchKernelGGL(grad_norm_combine_kernel, dim3(1), dim3(1024), 0, st, (const float*)gn_partial, (const int*)gn_tfirst, (int)gn_tens.size(), gscale, (const ScalerState*)scaler,
                               clip_state, gn_tsq, gn_tnorm);
            gn_have = true;
        } else if (scaler) hipLaunchKernelGGL(nonfinite_check_kernel, dim3(2048), dim3(256), 0, st, G, (long long)numel, scaler);
        if (o.kind == HULC_OPT_SGD)
            hipLaunchKernelGGL(sgd_kernel, dim3(2048), dim3(256), 0, st, P, G, AM, (long long)numel, lr, o.momentum, o.dampening, o.weight_decay, (int)(o.nesterov != 0),
                               (int)(step == 1), gscale, shadow, (const ScalerState*)scaler, (const unsigned*)rp_skip, tag, cs);
        else if (adam_fuse_tr && tr_adam.n && shadow) {
            AdamArgs a{P, G, AM, AV, lr, b1, b2, eps, (float)bc1d, (float)sqrt(bc2d), gscale, o.weight_decay, (int)(o.kind == HULC_OPT_ADAMW), shadow, (const ScalerState*)scaler, (const unsigned*)rp_skip, tag, cs};
            hipLaunchKernelGGL(adam_tiled_kernel, dim3(tr_adam.blocks + adam_chunks), dim3(256), 0, st, a, (const TrDesc*)tr_adam.desc, (const unsigned short*)tr_adam.b2d, tr_adam.blocks,
                               (const long long*)adam_chunk_start, (const int*)adam_chunk_n);
            tr_fresh = true;
        } else
            hipLaunchKernelGGL(adam_kernel, dim3(2048), dim3(256), 0, st, P, G, AM, AV, (long long)numel, lr, b1, b2, eps, (float)bc1d, (float)sqrt(bc2d), gscale,
                               shadow, (const ScalerState*)scaler, o.weight_decay, (int)(o.kind == HULC_OPT_ADAMW), (const unsigned*)rp_skip, tag, cs);
        if (ema) ema_step(tag);      // the averaged weights follow the step under the step's own skip conditions (engine_ema.inc)
        if (scaler) hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(1), 0, st, scaler, (const unsigned*)rp_skip, tag);
        if (hipGetLastError() != hipSuccess) { hulc_set_error("adam launch failed"); return 1; }
        return prepare_weights(true);
    }

    int get_tensor(const char* name, float* out, int64_t cap, int64_t* n) override {
        auto it = named.find(name);
        if (it == named.end()) { hulc_set_error("hulc_get_tensor: unknown tensor '%s'", name); return 1; }
        const Named& t = it->second;
        int64_t cnt = std::min<int64_t>(cap, t.n);
        *n = cnt;
        HIP_CHECK(hipStreamSynchronize(st));
        if (t.kind == 0) { HIP_CHECK(hipMemcpy(out, t.p, cnt * sizeof(float), hipMemcpyDeviceToHost)); }
        else if (t.kind == 1) {
            std::vector<T> tmp(cnt);
            HIP_CHECK(hipMemcpy(tmp.data(), t.p, cnt * sizeof(T), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < cnt; ++i) out[i] = host_to_f(tmp[i]);
        } else {
            std::vector<int> tmp(cnt);
            HIP_CHECK(hipMemcpy(tmp.data(), t.p, cnt * sizeof(int), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < cnt; ++i) out[i] = (float)tmp[i];
        }
        return 0;
    }
    static float host_to_f(float x) { return x; }
#ifdef HULC_HALF_F16
    static float host_to_f(h16_t x) {      // IEEE binary16 -> float on the host
        const uint32_t sgn = (uint32_t)(x >> 15) << 31, ex = (x >> 10) & 31, man = x & 1023;
        uint32_t u;
        if (ex == 0) { float f = ldexpf((float)man, -24); memcpy(&u, &f, 4); u |= sgn; }
        else if (ex == 31) u = sgn | 0x7f800000u | (man << 13);
        else u = sgn | ((ex + 112) << 23) | (man << 13);
        float f; memcpy(&f, &u, 4); return f;
    }
#else
    static float host_to_f(h16_t x) { uint32_t u = ((uint32_t)x) << 16; float f; memcpy(&f, &u, 4); return f; }
#endif
    int get_plan_idx(int32_t* out, int64_t cap) override {
        HIP_CHECK(hipStreamSynchronize(st));
        int64_t cnt = std::min<int64_t>(cap, (int64_t)cur.B * NCAT);
        HIP_CHECK(hipMemcpy(out, pidx, cnt * sizeof(int), hipMemcpyDeviceToHost));
        return 0;
    }
};

// per-kernel test entry (hulc_k_gemm_nt): C (fp32) = relu?(A B^T + bias) through the production GEMM kernels of this translation unit's
// 16-bit type (or fp32 when is_f32; bf16 unit only).  relu bit 2 (value 4): force the register-staged kernel instead of the LDS-DMA one.
int k_gemm_nt(int is_f32, const void* A, const void* B, float* C, int M, int N, int K, long long lda, long long ldb, long long ldc, const float* bias, int relu,
              void* stream) {
    hipStream_t st = (hipStream_t)stream;
    EpiP ep; ep.out = C; ep.out_f32 = 1; ep.bias = bias; ep.relu = relu & 1;
    if (!is_f32 && !(relu & 4) && M >= 512 && N >= 128) {
        const DenseLoader<h16_t> a = dense<h16_t>((const h16_t*)A, M, lda), b = dense<h16_t>((const h16_t*)B, N, ldb);
        if (gemm_glds_ok(a, b, ep, M, N, K)) {
            launch_gemm_glds(st, a, b, dense_out(ldc), ep, M, N, K);
            if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_gemm_nt: launch failed"); return 1; }
            return 0;
        }
    }
    if (is_f32) {
#ifdef HULC_HALF_F16
        hulc_set_error("hulc_k_gemm_nt: the fp32 kernels live in the bf16 translation unit"); return 1;
#else
        if (M >= 512 && N >= 128) launch_gemm<float, 128, 128>(st, dense<float>((const float*)A, M, lda), dense<float>((const float*)B, N, ldb), dense_out(ldc), ep, M, N, K);
        else launch_gemm<float, 64, 64>(st, dense<float>((const float*)A, M, lda), dense<float>((const float*)B, N, ldb), dense_out(ldc), ep, M, N, K);
#endif
    } else {
        if (M >= 512 && N >= 128) launch_gemm<h16_t, 128, 128>(st, dense<h16_t>((const h16_t*)A, M, lda), dense<h16_t>((const h16_t*)B, N, ldb), dense_out(ldc), ep, M, N, K);
        else launch_gemm<h16_t, 64, 64>(st, dense<h16_t>((const h16_t*)A, M, lda), dense<h16_t>((const h16_t*)B, N, ldb), dense_out(ldc), ep, M, N, K);
    }
    if (hipGetLastError() != hipSuccess) { hulc_set_error("hulc_k_gemm_nt: launch failed"); return 1; }
    return 0;
}

// factory of this translation unit (iengine.h): fp32 + bf16 engines in capi.hip, the fp16 engine in engine_f16.hip
IEngine* make_engine(const hulc_config& cfg, int* rc) {
#ifdef HULC_HALF_F16
    auto* e = new Engine<h16_t>(cfg); *rc = e->alloc_all(); return e;
#else
    if (cfg.dtype == HULC_DTYPE_F32) { auto* e = new Engine<float>(cfg); *rc = e->alloc_all(); return e; }
    auto* e = new Engine<h16_t>(cfg); *rc = e->alloc_all(); return e;
#endif
}

}  // namespace HULC_NS

#include "k_entries.h"      // test entries of the 16-bit encoder head and the action loss (hulc_k_spatial_softmax64, hulc_k_enc_tail_*, hulc_k_logistic_loss)
