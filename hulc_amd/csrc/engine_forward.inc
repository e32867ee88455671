// hulc_amd/csrc/engine_forward.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body: MLP helper, the forward pieces shared by training / validation / rollout, hulc_forward_loss and hulc_forward_loss_pair (SURVEY 8 a1, a2, a7-a15).
// Split out of engine.h in round 6 (VERDICT r5 weak #12: one 224 KB header); no code changed by the move.  Not a standalone header.
    // ---------------------------------------------------------------- MLP helper (ReLU between layers, none after last)
    // acts[i] = output of layer i (T) ; last layer output fp32 (outf)
    void mlp_fwd(const T* x, long long ldx, int M, LinW* L, int n, T** acts, float* outf, T* outt) {
        const T* in = x; long long ld = ldx;
        for (int i = 0; i < n; ++i) {
            if (i < n - 1) { EpiP ep = epi(acts[i], false); ep.relu = 1; lin_fwd(in, ld, M, L[i], ep, L[i].N); in = acts[i]; ld = L[i].N; }
            else {
                if (outf) { EpiP ep = epi(outf, true); lin_fwd(in, ld, M, L[i], ep, L[i].N); }
                if (outt) { EpiP ep = epi(outt, false); lin_fwd(in, ld, M, L[i], ep, L[i].N); }
            }
        }
    }
    // dy: T [M][N_last]; x: first-layer input (ldx). dxf: optional fp32 output (accumulating) with map
    // 16-bit engines, M <= 64: the weight / bias gradients are queued (wq_add) and read every layer's incoming gradient at the flush, so each mlp_bwd call of a backward
    // keeps its chain in a buffer set of its own (mlp_dy_next counts the calls; reset when a backward starts).  A set = 7 x 64 x 2048 values of T
    static constexpr int MLP_DY_SETS = 4;
    T* mlp_dy[MLP_DY_SETS][8] = {};
    int mlp_dy_next = 0;
    void mlp_bwd(const T* dy, const T* x, long long ldx, int M, LinW* L, int n, T** acts, T* s0, T* s1, float* dxf, const DenseOut* om, int dx_acc) {
        const T* d = dy;
        if constexpr (std::is_same<T, h16_t>::value) {
            // M <= 64 (every M = B MLP): the data-gradient chain runs here, every layer's incoming gradient kept in its own buffer; the weight / bias gradients of
            // all layers join the backward's one batched launch (wq_flush) instead of one ~9 us launch per layer.  Store or add is decided per tensor at the flush
            if (M <= 64 && n <= 8 && mlp_dy_next < MLP_DY_SETS) {
                T** const set = mlp_dy[mlp_dy_next++];
                for (int i = n - 1; i >= 0; --i) {
                    const T* in = i > 0 ? acts[i - 1] : x;
                    const long long ld = i > 0 ? L[i - 1].N : ldx;
                    wq_add(d, in, ld, M, L[i].N, L[i].K, L[i].dW, L[i].K, L[i].db);
                    if (i > 0) {
                        if (!set[i]) set[i] = alloc<T>((int64_t)64 * 2048);
                        T* o = L[i].K <= 2048 ? set[i] : (T*)nullptr;
                        if (!o) { hulc_set_error("mlp_bwd: hidden width %d exceeds the per-layer gradient buffers", L[i].K); return; }
                        EpiP ep = epi(o, false); ep.mask = acts[i - 1];
                        lin_dgrad(d, M, L[i], ep, dense_out(L[i].K));
                        d = o;
                    } else if (dxf) {
                        EpiP ep = epi(dxf, true); ep.accumulate = dx_acc;
                        lin_dgrad(d, M, L[i], ep, *om);
                    }
                }
                return;
            }
        }
        T* scratch[2] = {s0, s1};
        for (int i = n - 1; i >= 0; --i) {
            const T* in = i > 0 ? acts[i - 1] : x;
            const long long ld = i > 0 ? L[i - 1].N : ldx;
            lin_wgrad(d, in, ld, M, L[i].N, L[i].K, L[i].dW, L[i].K, L[i].db);
            if (i > 0) {
                T* o = scratch[i & 1];
                EpiP ep = epi(o, false); ep.mask = acts[i - 1];
                lin_dgrad(d, M, L[i], ep, dense_out(L[i].K));
                d = o;
            } else if (dxf) {
                EpiP ep = epi(dxf, true); ep.accumulate = dx_acc;
                lin_dgrad(d, M, L[i], ep, *om);
            }
        }
    }

    // ---------------------------------------------------------------- forward pieces (shared by training, validation and rollout)
    // perceptual encoders + goal encoder + plan proposal MLP
    void trunk_fwd(const hulc_batch* b, float dp) {
        const int B = b->B, S = b->S, N = B * S;
        const bool hulc = cfg.kind == HULC_KIND_HULC;
        bool ppx_packed = false;
        // ---- perceptual encoders (concat_encoders.py:59-109): static -> emb[..., 0:64], gripper -> emb[..., 64:128]
        {
            const Conv1Src src[2] = {conv1_src(*b, false), conv1_src(*b, true)}, src2[2] = {conv1_src(cur2, false), conv1_src(cur2, true)};
            const bool tail_fused = enc_tail_fusable();
            // ragged pass (window_len_host): the encoders run on the N' real frames and write compact rows, which are then expanded to the (B,S,EMB) rows everything
            // below reads; the transformer input is a function of the batch row, so pr_fwd writes it with its own launch (x0_done stays false)
            const int Nenc = enc_frames(N);
            enc_fwd_both(src, pair ? src2 : nullptr, Nenc, tail_fused);
            x0_done = false;
            if (tail_fused) enc_tail_fwd_both(Nenc, !ragged() && !mcil && trf_on() && S <= 64 && EMB == 128, S, dp);
            if (ragged()) launch_rows_expand<T>(st, emb_c, rg_lens(), rg_off(), B, S, EMB, emb);
            enc_frames_last = Nenc;
        }
        // ---- goal encoder (goal_encoders.py:31-36 / 64-69)
        if (pair) {       // rows [0, Bv): visual goal = emb[:, -1]; rows [Bv, B): language goal
            const int Bv = pairBv, Bl = B - pairBv;
            T* av[2] = {gl1, gl2};
            T* al[2] = {gl1 + (long long)Bv * HID, gl2 + (long long)Bv * HID};
            mlp_fwd(emb + (long long)(S - 1) * EMB, (long long)S * EMB, Bv, vg, 3, av, gl3, nullptr);
            ln_fwd(gl3, GOAL, Bv, GOAL, ln_vg_g, ln_vg_b, goal_t, GOAL, nullptr, 0, goal_st);
            hipLaunchKernelGGL((cast_kernel<float, T>), dim3(cdiv(Bl * LANG, 256)), dim3(256), 0, st, b->lang, lang_t, (long long)Bl * LANG);
            mlp_fwd(lang_t, LANG, Bl, lg, 3, al, gl3 + Bv * GOAL, nullptr);
            ln_fwd(gl3 + Bv * GOAL, GOAL, Bl, GOAL, ln_lg_g, ln_lg_b, goal_t + Bv * GOAL, GOAL, nullptr, 0, goal_st + 2 * Bv);
        } else {
            T* acts[2] = {gl1, gl2};
            // hulc / mcil: the LayerNorm launch also packs the plan proposal's input rows [emb[:,0,:] | goal] (goal_ln_concat_kernel)
            auto goal_ln = [&](const float* g_, const float* b_) {
                if (hulc || mcil) {
                    hipLaunchKernelGGL((goal_ln_concat_kernel<T>), dim3(cdiv(B, 4) + cdiv(B * EMB, 256)), dim3(256), 0, st, gl3, B, GOAL, g_, b_, goal_t, goal_st, emb, (long long)S * EMB, EMB, ppx);
                    ppx_packed = true;
                } else ln_fwd(gl3, GOAL, B, GOAL, g_, b_, goal_t, GOAL, nullptr, 0, goal_st);
            };
            if (b->is_lang) {
                hipLaunchKernelGGL((cast_kernel<float, T>), dim3(cdiv(B * LANG, 256)), dim3(256), 0, st, b->lang, lang_t, (long long)B * LANG);
                mlp_fwd(lang_t, LANG, B, lg, 3, acts, gl3, nullptr);
                goal_ln(ln_lg_g, ln_lg_b);
            } else {
                mlp_fwd(emb + (long long)(S - 1) * EMB, (long long)S * EMB, B, vg, 3, acts, gl3, nullptr);
                goal_ln(ln_vg_g, ln_vg_b);
            }
        }
        // ---- plan proposal (plan_proposal_net.py:42-47)
        if (hulc || mcil) {
            if (!ppx_packed) hipLaunchKernelGGL((concat_pp_kernel<T>), dim3(cdiv(B * (EMB + GOAL), 256)), dim3(256), 0, st, emb, (long long)S * EMB, EMB, goal_t, GOAL, B, ppx);
            mlp_fwd(ppx, EMB + GOAL, B, pp, 5, ppa, pp_logits, nullptr);
        }
    }
    // plan recognition transformer -> seq_feat, pr_logits
    void pr_fwd(int B, int S, float dp) {
        const int N = B * S;
        // ---- plan recognition transformer (plan_recognition_net.py:94-117)
        bool fused = false;
        if constexpr (std::is_same<T, h16_t>::value) {
            fused = trf_on() && S <= 64;          // 32 < S <= 64 (config 5): two 32-row halves per window, tr_fused.h WIDE
        }
        if (!(fused && x0_done))
        hipLaunchKernelGGL((posadd_kernel<T>), dim3(cdiv((long long)N * EMB, 256)), dim3(256), 0, st, emb, pos32, B, S, EMB, xf[0], xt[0], dp, site_seed(0),
                           fused ? y2[0] : (float*)nullptr, fused ? y2[1] : (float*)nullptr);
        x0_done = false;
        if constexpr (std::is_same<T, h16_t>::value) {
            if (fused) {        // one launch per encoder layer (tr_fused.h); norm2 of layer 0 is the first step of layer 1's launch, the last norm2 a LayerNorm launch
                for (int l = 0; l < 2; ++l) {
                    TrLayerP q{};
                    q.xin = l ? y2[0] : xf[0]; q.ln_in = l; q.ln_g = tr_n2g[0]; q.ln_b = tr_n2b[0]; q.xf_out = xf[1]; q.xt_out = xt[1]; q.st_out = st2[0];
                    q.Wqkv = tr_in[l].Wfr; q.Wo = tr_out[l].Wfr; q.W1 = tr_l1[l].Wfr; q.W2 = tr_l2[l].Wfr;
                    q.bqkv = tr_in[l].b32; q.bo = tr_out[l].b32; q.b1 = tr_l1[l].b32; q.b2 = tr_l2[l].b32; q.n1g = tr_n1g[l]; q.n1b = tr_n1b[l];
                    q.qkv = qkv[l]; q.Pat = Pat[l]; q.ao = ao[l]; q.y1 = y1[l]; q.st1 = st1[l]; q.x1t = x1t[l]; q.x1f = x1f[l]; q.hff = hff[l]; q.y2 = y2[l];
                    q.B = B; q.S = S; q.dp = dp;
                    q.seed_att = site_seed(1 + 4 * l); q.seed_o = site_seed(2 + 4 * l); q.seed_h = site_seed(3 + 4 * l); q.seed_y = site_seed(4 + 4 * l);
                    // per token: QKV 3 x 128 x 128, out projection 128 x 128, FFN 2 x 128 x 2048, attention 2 x S x 128 MACs (SURVEY §8(d))
                    TimerScope ts(this, "transformer_fused", "mfma", 2.0 * N * (4.0 * EMB * EMB + 2.0 * EMB * FF + 2.0 * S * EMB), (double)N * (4 * EMB + FF) * sizeof(T));
                    nd(ND_TR_FFN_FWD);      // y2: four hidden quarters per element
                    launch_tr_layer_fwd(st, q);
                }
                // the last norm2 and the mean over the window in one launch (the normalised rows are kept for tests only)
                launch_ln_mean<T>(st, y2[1], B, S, EMB, tr_n2g[1], tr_n2b[1], st2[1], xm, xf[2]);
            }
        }
        for (int l = 0; l < 2 && !fused; ++l) {
            { EpiP ep = epi(qkv[l], false); lin_fwd(xt[l], EMB, N, tr_in[l], ep, 3 * EMB); }
            launch_attention_fwd<T>(st, attention_s64(S), qkv[l], B, S, EMB, NH, Pat[l], ao[l], dp, site_seed(1 + 4 * l));
            { EpiP ep = epi(y1[l], true); ep.res = xf[l]; ep.res_f32 = 1; ep.res_ld = EMB; ep.res_late = 1; ep.drop_p = dp; ep.drop_seed = site_seed(2 + 4 * l);
              lin_fwd(ao[l], EMB, N, tr_out[l], ep, EMB); }
            ln_fwd(y1[l], EMB, N, EMB, tr_n1g[l], tr_n1b[l], x1t[l], EMB, x1f[l], EMB, st1[l]);
            { EpiP ep = epi(hff[l], false); ep.relu = 1; ep.drop_p = dp; ep.drop_seed = site_seed(3 + 4 * l); lin_fwd(x1t[l], EMB, N, tr_l1[l], ep, FF); }
            { EpiP ep = epi(y2[l], true); ep.res = x1f[l]; ep.res_f32 = 1; ep.res_ld = EMB; ep.res_late = 1; ep.drop_p = dp; ep.drop_seed = site_seed(4 + 4 * l);
              lin_fwd(hff[l], FF, N, tr_l2[l], ep, EMB); }
            ln_fwd(y2[l], EMB, N, EMB, tr_n2g[l], tr_n2b[l], xt[l + 1], EMB, xf[l + 1], EMB, st2[l]);
        }
        // mean over S commutes with the affine fc (:113-114): seq_feat = fc(mean_t x)
        if (!fused) hipLaunchKernelGGL((mean_over_s_kernel<T>), dim3(cdiv(B * EMB, 256)), dim3(256), 0, st, xf[2], B, S, EMB, xm);
        { EpiP ep = epi(seqf, true); ep.out2 = seqf_t; ep.out2_lo = 0; ep.out2_hi = (long long)B * FCH;      // the 16-bit copy the next GEMM reads: a second store of the epilogue
          lin_fwd(xm, EMB, B, pr_fc, ep, FCH); }
        { EpiP ep = epi(pr_logits, true); lin_fwd(seqf_t, FCH, B, pr_fs, ep, PLAN); }
    }
    // action decoder up to the packed heads [S*B][NHEAD] (logistic_decoder_rnn.py:260-287); plan/goal terms hoisted out of the time loop.
    // h0_0 / h0_1: previous hidden states [B][HID] of the two layers (stateful rollout, :107-111) or null (h0 = 0).
    void dec_fwd(const int* plan_idx, int B, int S, const T* h0_0, const T* h0_1) {
        const int SB = S * B;
        const bool hulc = cfg.kind == HULC_KIND_HULC;
        // 16-bit engines (hulc / gcbc): the goal term of the time-invariant decoder input is added inside the plan-gather launch; the fp32 (parity)
        // engine and mcil (whose plan term is a GEMM already) keep the K = 32 GEMM and its summation order
        const bool cb_fused = !mcil && !std::is_same<T, float>::value;
            // time-major copy of the gripper half of emb: embg[t*B+b][0:64] = emb[b][t][64:128]
            if (mcil) {      // continuous plan (B,256): a GEMM against the plan columns of W_ih0 instead of the one-hot column gather
                hipLaunchKernelGGL((gather_embg_kernel<T>), dim3(cdiv(SB * DE, 256)), dim3(256), 0, st, emb, embg, B, S, DE);
                EpiP ep = epi(Cplan, true); ep.bias = bih0; ep.bias2 = bhh0;
                gemm(dense<T>(plan_t, B, dec_plan), dense<T>(wih0, HID, KIN), dense_out(HID), ep, B, HID, dec_plan);
            } else      // the one-hot plan gather and the time-major embedding copy are independent: one launch
            launch_plan_gather<T>(st, wih0T, plan_idx, B, hulc ? NCAT : 0, NCLS, HID, bih0, bhh0, Cplan, emb, embg, S, DE, goal_t, GOAL, dec_plan + DE, cb_fused ? Cb : (T*)nullptr);
            if (!cb_fused) { EpiP ep = epi(Cb, false); ep.res = Cplan; ep.res_f32 = 1; ep.res_ld = HID;
              gemm(dense<T>(goal_t, B, GOAL), dense<T>(wih0 + dec_plan + DE, HID, KIN), dense_out(HID), ep, B, HID, GOAL); }
            if (mlp) {      // feed-forward body (rnn.py mlp_decoder): a0 = relu(W0 x + b0) with the time-invariant term as the broadcast residual, a1 = relu(W1 a0 + b1), y = W2 a1 + b2
                { EpiP ep = epi(H0, false); ep.res = Cb; ep.res_ld = HID; ep.res_rowmod = B; ep.relu = 1;
                  gemm(dense<T>(embg, SB, DE), dense<T>(wih0 + dec_plan, HID, KIN), dense_out(HID), ep, SB, HID, DE); }
                { EpiP ep = epi(H1, false); ep.relu = 1; lin_fwd(H0, HID, SB, mlp1, ep, HID); }
                { EpiP ep = epi(Zx1, false); lin_fwd(H1, HID, SB, mlp2, ep, HID); }
                { EpiP ep = epi(heads, true); ep.bias = bheads;
                  gemm(dense<T>(Zx1, SB, HID), dense<T>(wheads, NHEAD, HID), dense_out(NHEAD), ep, SB, NHEAD, HID); }
                return;
            }
            const long long BH = (long long)B * HID;
            { EpiP ep = epi(Zx0, false); ep.res = Cb; ep.res_ld = HID; ep.res_rowmod = B;
              if (!h0_0) { ep.out2 = H0; ep.out2_lo = 0; ep.out2_hi = BH; ep.out2_relu = 1; }      // h_{-1} = 0: H0[0] = relu(Zx0[0]) written here
              gemm(dense<T>(embg, SB, DE), dense<T>(wih0 + dec_plan, HID, KIN), dense_out(HID), ep, SB, HID, DE); }
            rnn_fwd(Zx0, H0, whh0, B, S, h0_0, 1, false, !h0_0);
            { EpiP ep = epi(Zx1, false); ep.bias = bih1; ep.bias2 = bhh1;
              if (!h0_1) { ep.out2 = H1; ep.out2_lo = 0; ep.out2_hi = BH; ep.out2_relu = 1; }
              gemm(dense<T>(H0, SB, HID), dense<T>(wih1.W, HID, HID), dense_out(HID), ep, SB, HID, HID); }
            rnn_fwd(Zx1, H1, whh1, B, S, h0_1, 1, false, !h0_1);
            if (det) return;      // the deterministic head reads H1 itself (det_head.h): no heads GEMM
            { EpiP ep = epi(heads, true); ep.bias = bheads;
              gemm(dense<T>(H1, SB, HID), dense<T>(wheads, NHEAD, HID), dense_out(NHEAD), ep, SB, NHEAD, HID); }
    }

    // ---------------------------------------------------------------- forward
    int forward(const hulc_batch* b, float lw, float cw, float* out, int on_host) override {
        pair = false;
        int rc = forward_impl(b, lw, cw, out, on_host);
        // a persistent recurrence of THIS forward timed out and the stream is drained (losses read back): run it again, one launch per step
        if (!rc && out && on_host && persist_check("hulc_forward_loss", true)) rc = forward_impl(b, lw, cw, out, on_host);
        return rc;
    }
    // vis + lang windows of one step as ONE pass over Bv + Bl windows (hulc.py:433-469 runs them one after the other): the encoders, plan
    // networks and the decoder are shared, only the goal encoder (rows [0,Bv): visual, [Bv,B): language) and the CLIP rows differ.  The
    // latency-bound part of the step (recurrent steps, M <= 64 GEMMs, transformer) then runs once at 2B rows instead of twice at B.
    // Needs Bv == Bl (the per-modality means then share one gradient scale).  out: [total, kl, action, clip] of vis, then of lang.
    std::vector<int> aux_host;
    int* pidx_j = nullptr;
    int forward_pair(const hulc_batch* vb, const hulc_batch* lb, float lw, float cw, float* out, int on_host) override {
        if (!bound) { hulc_set_error("hulc_forward_loss_pair before hulc_bind_params"); return 1; }
        if (vb->is_lang || !lb->is_lang || !lb->lang) { hulc_set_error("hulc_forward_loss_pair: first batch must be the vis modality, second the lang modality with embeddings"); return 1; }
        if (vb->B != lb->B || vb->S != lb->S) { hulc_set_error("hulc_forward_loss_pair: both modalities need the same B and S (got %dx%d and %dx%d)", vb->B, vb->S, lb->B, lb->S); return 1; }
        for (const hulc_batch* b : {vb, lb})
            if (ingest_args_bad(b)) return 1;
        if ((vb->window_len_host != nullptr) != (lb->window_len_host != nullptr)) {
            hulc_set_error("hulc_forward_loss_pair: window_len_host (ragged encoder pass) must be given for both modalities or for neither"); return 1; }
        if (vb->frames_u8 != lb->frames_u8 || vb->actions_absolute != lb->actions_absolute || vb->max_rel_pos != lb->max_rel_pos || vb->max_rel_orn != lb->max_rel_orn) {
            hulc_set_error("hulc_forward_loss_pair: both modalities must use the same ingest options"); return 1; }
        if ((vb->plan_idx != nullptr) != (lb->plan_idx != nullptr) || (vb->plan_eps != nullptr) != (lb->plan_eps != nullptr)) {
            hulc_set_error("hulc_forward_loss_pair: inject the plan draw for both modalities or for neither"); return 1; }
        const int Bv = vb->B, B = 2 * Bv, S = vb->S;
        if (B > maxB) { hulc_set_error("hulc_forward_loss_pair: %d + %d windows exceed max_batch=%d", Bv, Bv, maxB); return 1; }
        if (!act_j) {
            act_j = alloc<float>((int64_t)maxN * 7); ro_j = alloc<float>((int64_t)maxN * 15); eps_j = alloc<float>((int64_t)maxB * 256);
            pidx_j = alloc<int>((int64_t)maxB * NCAT); losses2 = alloc<float>(8);
            if (alloc_failed) { hulc_set_error("hulc_forward_loss_pair: workspace allocation failed"); return 1; }
        }
        const size_t na = sizeof(float) * Bv * S * 7, nr = sizeof(float) * Bv * S * 15;
        MultiCopy mc{}; int nseg = 0;          // the joins of the two modalities' actions / robot_obs (device memory by the hulc_batch contract): one launch
        auto seg = [&](void* dst, const void* src, size_t bytes) { mc.dst[nseg] = (unsigned*)dst; mc.src[nseg] = (const unsigned*)src; mc.words[nseg] = (int)(bytes / 4); ++nseg; };
        seg(act_j, vb->actions, na); seg((char*)act_j + na, lb->actions, na);
        seg(ro_j, vb->robot_obs, nr); seg((char*)ro_j + nr, lb->robot_obs, nr);
        hulc_batch jb = *vb;
        jb.B = B; jb.actions = act_j; jb.robot_obs = ro_j; jb.lang = lb->lang; jb.is_lang = 0;
        hipLaunchKernelGGL(multi_copy_kernel, dim3(16, nseg), dim3(256), 0, st, mc);
        if (vb->plan_idx) {                    // injected draws (parity tests) may live in host memory: plain copies
            HIP_CHECK(hipMemcpyAsync(pidx_j, vb->plan_idx, sizeof(int) * Bv * NCAT, hipMemcpyDefault, st));
            HIP_CHECK(hipMemcpyAsync(pidx_j + Bv * NCAT, lb->plan_idx, sizeof(int) * Bv * NCAT, hipMemcpyDefault, st));
            jb.plan_idx = pidx_j;
        }
        if (vb->plan_eps) {
            const size_t ne = sizeof(float) * Bv * (PLAN / 2);
            HIP_CHECK(hipMemcpyAsync(eps_j, vb->plan_eps, ne, hipMemcpyDefault, st)); HIP_CHECK(hipMemcpyAsync((char*)eps_j + ne, lb->plan_eps, ne, hipMemcpyDefault, st));
            jb.plan_eps = eps_j;
        }
        aux_host.assign(lb->aux_rows ? lb->aux_rows : nullptr, lb->aux_rows ? lb->aux_rows + lb->n_aux : nullptr);
        for (int& r : aux_host) r += Bv;
        jb.aux_rows = aux_host.data(); jb.n_aux = lb->aux_rows ? lb->n_aux : 0;
        pair = true; pairBv = Bv; cur2 = *lb;
        int rc = forward_impl(&jb, lw, cw, out, on_host);
        if (!rc && out && on_host && persist_check("hulc_forward_loss_pair", true)) rc = forward_impl(&jb, lw, cw, out, on_host);
        return rc;
    }
    // An injected categorical sample (host or device memory) is a row of the plan gather's weight and of the plan scatter's LDS tile, unchecked in both kernels:
    // it is read back and refused on the host when any class lies outside [0, NCLS) — nothing is launched with it (the rollout paths clamp theirs on the device)
    int plan_idx_bad(const int* src, int count, const char* who) {
        std::vector<int> h((size_t)count);
        HIP_CHECK(hipMemcpyAsync(h.data(), src, sizeof(int) * (size_t)count, hipMemcpyDefault, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < count; ++i)
            if (h[i] < 0 || h[i] >= NCLS) { hulc_set_error("%s: injected plan index %d (window %d, category %d) is outside [0, %d)", who, h[i], i / NCAT, i % NCAT, NCLS); return 1; }
        return 0;
    }
    // the frame-store and RandomShiftsAug arguments of one batch
    static bool ingest_args_bad(const hulc_batch* b) {
        if (store_args_bad(b)) return true;
        if (b->frames_u8 && (b->shift_static || b->shift_gripper) && (b->pad_static < 0 || b->pad_static > CONV1_RAW_MARGIN || b->pad_gripper < 0 || b->pad_gripper > CONV1_RAW_MARGIN)) { hulc_set_error("RandomShiftsAug pads must lie in [0, %d] (the staged rows' replicate margin); got pad_static=%d, pad_gripper=%d", CONV1_RAW_MARGIN, b->pad_static, b->pad_gripper); return true; }
        return false;
    }
    // what a training forward and a validation forward ask of their batch's shape and modality (its ingest arguments: ingest_args_bad, which validation checks later)
    bool batch_args_bad(const hulc_batch* b) {
        if (b->B < 1 || b->S < 1 || b->B > maxB || b->S > maxS || b->S > cfg.max_window || b->S > 64) { hulc_set_error("batch (B=%d,S=%d) exceeds workspace (max_batch=%d,max_seq=%d,max_window=%d)", b->B, b->S, maxB, maxS, cfg.max_window); return true; }
        if (b->is_lang && !b->lang) { hulc_set_error("lang modality batch without language embeddings (hulc.py:440 KeyError 'lang')"); return true; }
        if (b->actions_absolute && !(b->max_rel_pos > 0.f && b->max_rel_orn > 0.f)) { hulc_set_error("actions_absolute needs max_rel_pos > 0 and max_rel_orn > 0 (RelativeActions, transforms.py:35-37)"); return true; }
        return false;
    }
    // gather the flagged rows of seqf_t and goal_t, then the two CLIP projections (hulc.py:650-695): img, txt [n][GOAL] fp32.  auxrows holds the n row indices
    void clip_proj_fwd(int n) {
        hipLaunchKernelGGL((gather_rows_kernel<T, T>), dim3(cdiv(n * FCH, 256)), dim3(256), 0, st, seqf_t, (long long)FCH, auxrows, n, FCH, sf_m);
        hipLaunchKernelGGL((gather_rows_kernel<T, T>), dim3(cdiv(n * GOAL, 256)), dim3(256), 0, st, goal_t, (long long)GOAL, auxrows, n, GOAL, g_m);
        { EpiP ep = epi(im1, false); ep.relu = 1; lin_fwd(sf_m, FCH, n, cl_im0, ep, 128); }
        { EpiP ep = epi(img, true); lin_fwd(im1, 128, n, cl_im2, ep, GOAL); }
        { EpiP ep = epi(la1, false); ep.relu = 1; lin_fwd(g_m, GOAL, n, cl_la0, ep, 128); }
        { EpiP ep = epi(txt, true); lin_fwd(la1, 128, n, cl_la2, ep, GOAL); }
    }
    int forward_impl(const hulc_batch* b, float lw, float cw, float* out, int on_host) {
        if (!bound) { hulc_set_error("hulc_forward_loss before hulc_bind_params"); return 1; }
        persist_check("hulc_forward_loss", false);
        repro_latch();
        if (batch_args_bad(b) || ingest_args_bad(b)) return 1;
        if (cfg.kind == HULC_KIND_HULC && b->plan_idx && plan_idx_bad(b->plan_idx, b->B * NCAT, "hulc_forward_loss")) return 1;
        cur = *b; cur_lw = lw; cur_cw = cw; have_fwd = false; val_clip_n = 0;
        if (window_tables(*b, pair ? pairBv : b->B, pair ? &cur2 : nullptr)) return 1;
        const int B = b->B, S = b->S, N = B * S, SB = S * B;
        const bool hulc = cfg.kind == HULC_KIND_HULC;
        const float dp = cfg.dropout_p;
        const int Bm = pair ? pairBv : B;                    // windows per modality: the reference's means (and so the gradient scales) are per modality
        const float* kl_src = nullptr; int kl_n = 0;
        if constexpr (std::is_same<T, h16_t>::value) {      // cleared by the first conv1 launch of trunk_fwd (nothing accumulates a loss before the encoders are done)
            pend_zero[0] = losses; pend_zero[1] = pair ? losses2 : nullptr;
        } else {
            HIP_CHECK(hipMemsetAsync(losses, 0, 8 * sizeof(float), st));
            if (pair) HIP_CHECK(hipMemsetAsync(losses2, 0, 8 * sizeof(float), st));
        }
        trunk_fwd(b, dp);
        if (pend_zero[0]) { hulc_set_error("forward: the loss accumulators were not cleared (no conv1 launch took them)"); return 1; }
        // ---- sample + KL (hulc.py:289-296, 539-561); mcil: the reparametrised Normal sample
        const float wpp = lw * cfg.kl_beta * cfg.kl_balancing_mix / Bm, wpr = lw * cfg.kl_beta * (1.f - cfg.kl_balancing_mix) / Bm;
        if (mcil) {
            if (gru) bigru_fwd(B, S); else birnn_fwd(B, S);
            const int n = PLAN / 2;
            const float* eps = nullptr;
            if (b->plan_eps) { HIP_CHECK(hipMemcpyAsync(plan_eps_in, b->plan_eps, sizeof(float) * B * n, hipMemcpyDefault, st)); eps = plan_eps_in; }
            launch_normal_kl_sample<T>(st, pr_logits, pp_logits, B, n, eps, plan_eps, plan_f, plan_t, klel, dpp_kl, dpr_kl, wpp, wpr, site_seed(20), lscale());
            kl_src = klel; kl_n = Bm * n;
        } else pr_fwd(B, S, dp);
        if (hulc) {
            const int* idx_in = nullptr;
            if (b->plan_idx) { HIP_CHECK(hipMemcpyAsync(pidx_in, b->plan_idx, sizeof(int) * B * NCAT, hipMemcpyDefault, st)); idx_in = pidx_in; }
            launch_plan_kl_sample(st, pr_logits, pp_logits, B, NCAT, NCLS, idx_in, pidx, probs, klcat, dpp_kl, dpr_kl, wpp, wpr, site_seed(20), lscale());
            kl_src = klcat; kl_n = Bm * NCAT;
        }
        if (pair && kl_src) {      // per-modality KL sums; one modality: summed by finish_losses_kernel at the end of the forward
            launch_sum_reduce(st, kl_src, kl_n, cfg.kl_beta / Bm, losses + 1);
            launch_sum_reduce(st, kl_src + kl_n, kl_n, cfg.kl_beta / Bm, losses2 + 1);
        }
        // ---- action decoder (logistic_decoder_rnn.py:260-287): plan/goal terms hoisted out of the time loop
        {
            dec_fwd(pidx, B, S, nullptr, nullptr);
            // mcil_default.yaml: gripper_control false (no tcp-frame transform), discrete_gripper false (7th mixture dimension instead of the CE head)
            if (det)      // tanh head + Huber / MSE against the world-frame actions (deterministic_decoder.py:82-94) + the pre-activation gradient, one launch
                launch_det_head_loss<T>(st, H1, det_w, det_b32, actions_of(*b), b->robot_obs, B, S, det_crit, 0, lw / (float)(S * Bm), lscale(), rowloss, 8, nullptr, dpre);
            else      // the wide kernel on the 16-bit engines, the serial one on the fp32 parity engine (plan_ln_launch.h)
                launch_logistic_loss<T>(st, logistic_loss_wide<T>(NMIX, NDIM), heads, NHEAD, actions_of(*b), b->robot_obs, B, S, NMIX, NDIM, cfg.num_classes, cfg.log_scale_min,
                                        cfg.gripper_alpha, mcil ? 0 : 1, mcil ? 0 : 1, lw / (float)(S * Bm), lscale(), rowloss, a_tcp, dheads);
            if (pair) hipLaunchKernelGGL(sum_rows_pair_kernel, dim3(1), dim3(256), 0, st, rowloss, SB, B, pairBv, 1.f / (S * Bm), losses + 0, losses2 + 0);
            // one modality: the action-loss sum, the KL sum, the packing and the copy to a device `out` are ONE launch at the end (finish_losses_kernel)
        }
        // ---- CLIP auxiliary loss (hulc.py:650-695), lang modality, masked rows
        clip_n = 0;
        if ((b->is_lang || pair) && cfg.use_clip && b->n_aux > 0) {
            const int n = b->n_aux;
            if (n > B) { hulc_set_error("clip aux rows n=%d unsupported (<= B=%d)", n, B); return 1; }
            clip_n = n;
            HIP_CHECK(hipMemcpyAsync(auxrows, b->aux_rows, sizeof(int) * n, hipMemcpyHostToDevice, st));
            clip_proj_fwd(n);
            static_assert(GOAL == CLIP_D, "the CLIP loss kernels are built for 32-wide projections");
            // n <= 64: one workgroup (the 1024-thread form on the 16-bit engines, the serial one on the fp32 parity engine); above: the tiled launches of aux_rows.h
            if (!launch_clip_loss(st, !std::is_same<T, float>::value, img, txt, n, logit_scale, cw, (pair ? losses2 : losses) + 2, dimg, dtxt, dlogit_scale, lscale(), clip_rows_ws)) {
                hulc_set_error("clip loss: n=%d rows not covered by this context's workspace (max_batch=%d)", n, maxB); return 1; }
        }
        // ---- BC-Z / MIA auxiliary losses (hulc.py:567-648) on the same rows; the MIA head shares the CLIP projections
        bcz_n = mia_n = 0; aux_rows_last = 0;
        if ((aux_bcz || aux_mia) && (b->is_lang || pair) && b->n_aux > 0) {
            const int n = b->n_aux;
            if (n > B) { hulc_set_error("auxiliary-loss rows n=%d unsupported (<= B=%d)", n, B); return 1; }
            if (!clip_n) HIP_CHECK(hipMemcpyAsync(auxrows, b->aux_rows, sizeof(int) * n, hipMemcpyHostToDevice, st));
            if (aux_heads_fwd(b, n, clip_n > 0, true, pair ? pairBv : 0)) return 1;
            aux_rows_last = n;
        }
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in forward"); return 1; }
        have_fwd = true;
        // [total_mod, kl, action, clip]; a device `out` is written by the kernels themselves
        float* const dev_out = (out && !on_host) ? out : nullptr;
        if (!pair) {     // + the backward's zero arena (4 MB), cleared by 255 more blocks of the same launch instead of a memset at the head of the backward
            hipLaunchKernelGGL(finish_losses_kernel, dim3(256), dim3(256), 0, st, rowloss, SB * 8, 1.f / SB, kl_src, kl_n, cfg.kl_beta / Bm, losses, dev_out,
                               reinterpret_cast<float4*>(zero_arena), (long long)(zero_n / 4));
            arena_clean = true;
        }
        else if (out) {
            hipLaunchKernelGGL(pack_losses_kernel, dim3(1), dim3(1), 0, st, losses, dev_out);
            hipLaunchKernelGGL(pack_losses_kernel, dim3(1), dim3(1), 0, st, losses2, dev_out ? dev_out + 4 : (float*)nullptr);
        }
        if (out && on_host) {
            HIP_CHECK(hipMemcpyAsync(out, losses + 4, 4 * sizeof(float), hipMemcpyDeviceToHost, st));
            if (pair) HIP_CHECK(hipMemcpyAsync(out + 4, losses2 + 4, 4 * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        return 0;
    }
    int clip_n = 0;

