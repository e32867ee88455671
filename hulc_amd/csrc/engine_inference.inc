// hulc_amd/csrc/engine_inference.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body: validation forward (a20), the CLIP ground-truth metric, the stateful rollout.
// Split out of engine.h in round 6 (VERDICT r5 weak #12: one 224 KB header); no code changed by the move.  Not a standalone header.
    // ---------------------------------------------------------------- validation forward (SURVEY §8 a20; hulc.py:301-388, 770-797)
    float* valm = nullptr;            // [32]: 0 loss_pp, 1 loss_pr, 2 kl; 8..14 pp (mae[6], sr); 16..22 pr
    float *pred_pp = nullptr, *pred_pr = nullptr, *nz_mix = nullptr, *nz_act = nullptr;
    int* pidx_pp = nullptr;
    void val_alloc() {
        if (valm) return;
        valm = alloc<float>(32); pred_pp = alloc<float>((int64_t)maxB * maxS * 7); pred_pr = alloc<float>((int64_t)maxB * maxS * 7);
        nz_mix = alloc<float>((int64_t)maxB * maxS * NDIM * NMIX); nz_act = alloc<float>((int64_t)maxB * maxS * NDIM);
        pidx_pp = alloc<int>((int64_t)maxB * NCAT);
    }
    // mcil: plan ~ N(mean, std) of `state` (B, PLAN) into plan_f / plan_t, or the injected (B, PLAN/2) draw; with kl_with the per-element
    // KL(state || kl_with) lands in klel (no gradient weights)
    void sample_cont(const float* state, const float* kl_with, const float* inject, int B, uint64_t seed) {
        const int n = PLAN / 2;
        launch_normal_kl_sample<T>(st, state, kl_with, B, n, nullptr, plan_eps, plan_f, plan_t, klel, dpp_kl, dpr_kl, 0.f, 0.f, seed, nullptr);
        if (inject) {
            hipMemcpyAsync(plan_f, inject, sizeof(float) * B * n, hipMemcpyDefault, st);
            hipLaunchKernelGGL((cast_kernel<float, T>), dim3(cdiv(B * n, 256)), dim3(256), 0, st, plan_f, plan_t, (long long)B * n);
        }
    }
    int validate(const hulc_batch* b, const hulc_val_noise* nz, float* out17, int32_t* plan_pp_out, int32_t* plan_pr_out, float* pred_pp_out,
                 float* pred_pr_out) override {
        persist_check("hulc_validate", false);
        int rc = validate_impl(b, nz, out17, plan_pp_out, plan_pr_out, pred_pp_out, pred_pr_out);
        // validate ends with a stream synchronisation: a timed-out persistent recurrence is visible here -> the metrics are recomputed on the per-step path
        if (!rc && persist_check("hulc_validate", true)) rc = validate_impl(b, nz, out17, plan_pp_out, plan_pr_out, pred_pp_out, pred_pr_out);
        return rc;
    }
    int validate_impl(const hulc_batch* b, const hulc_val_noise* nz, float* out17, int32_t* plan_pp_out, int32_t* plan_pr_out, float* pred_pp_out,
                      float* pred_pr_out) {
        if (!bound) { hulc_set_error("hulc_validate before hulc_bind_params"); return 1; }
        if (batch_args_bad(b)) return 1;
        const bool hulc = cfg.kind == HULC_KIND_HULC;     // GCBC (gcbc.py:214-246): one decoder pass without a plan, reported in the "pp" slots
        val_alloc();
        if (alloc_failed) { hulc_set_error("hulc_validate: workspace allocation failed"); return 1; }
        repro_latch();
        if (ingest_args_bad(b)) return 1;
        static const hulc_val_noise none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (!nz) nz = &none;
        if (hulc && ((nz->plan_idx_pr && plan_idx_bad(nz->plan_idx_pr, b->B * NCAT, "hulc_validate (plan_idx_pr)")) ||
                     (nz->plan_idx_pp && plan_idx_bad(nz->plan_idx_pp, b->B * NCAT, "hulc_validate (plan_idx_pp)")))) return 1;
        cur = *b; have_fwd = false; pair = false; val_clip_n = 0;
        if (window_tables(*b, b->B, nullptr)) return 1;
        const int B = b->B, S = b->S, SB = S * B;
        HIP_CHECK(hipMemsetAsync(valm, 0, 32 * sizeof(float), st));
        trunk_fwd(b, 0.f);
        if (gru) bigru_fwd(B, S); else if (mcil) birnn_fwd(B, S); else pr_fwd(B, S, 0.f);
        // KL (beta-scaled) + recognition sample, then the proposal sample (no KL terms: second logits pointer null)
        const int* in_pr = nullptr;
        if (hulc) {
        if (nz->plan_idx_pr) { HIP_CHECK(hipMemcpyAsync(pidx_in, nz->plan_idx_pr, sizeof(int) * B * NCAT, hipMemcpyDefault, st)); in_pr = pidx_in; }
        launch_plan_kl_sample(st, pr_logits, pp_logits, B, NCAT, NCLS, in_pr, pidx, probs, klcat, dpp_kl, dpr_kl, 0.f, 0.f, site_seed(40), nullptr);
        launch_sum_reduce(st, klcat, B * NCAT, cfg.kl_beta / B, valm + 2);
        const int* in_pp = nullptr;
        if (nz->plan_idx_pp) { HIP_CHECK(hipMemcpyAsync(pidx_in, nz->plan_idx_pp, sizeof(int) * B * NCAT, hipMemcpyDefault, st)); in_pp = pidx_in; }
        launch_plan_kl_sample(st, pp_logits, nullptr, B, NCAT, NCLS, in_pp, pidx_pp, probs, klcat, dpp_kl, dpr_kl, 0.f, 0.f, site_seed(41), nullptr);
        }
        const float* acts = actions_of(*b);
        for (int pass = 0; pass < ((hulc || mcil) ? 2 : 1); ++pass) {          // 0: plan proposal, 1: plan recognition (loss_and_act, logistic_decoder_rnn.py:85-100)
            if (mcil) {      // continuous plan: Independent(Normal).sample() (distributions.py:37-38) or the injected draw (B,256) fp32
                sample_cont(pass == 0 ? pp_logits : pr_logits, pass == 0 ? nullptr : pp_logits, reinterpret_cast<const float*>(pass == 0 ? nz->plan_idx_pp : nz->plan_idx_pr),
                            B, site_seed(41 - pass));
                if (pass == 1) launch_sum_reduce(st, klel, B * (PLAN / 2), cfg.kl_beta / B, valm + 2);
                int32_t* po = pass == 0 ? plan_pp_out : plan_pr_out;
                if (po) HIP_CHECK(hipMemcpyAsync(po, plan_f, sizeof(float) * B * (PLAN / 2), hipMemcpyDefault, st));
            }
            dec_fwd(pass == 0 ? pidx_pp : pidx, B, S, nullptr, nullptr);
            // metrics: one atomic per row and component; reproducible mode sums the stored predictions in a fixed order instead (val_metrics_kernel)
            float *const pred = pass == 0 ? pred_pp : pred_pr, *const metrics = valm + 8 + 8 * pass;
            if (!repro && SB > 1) nd(ND_VAL_METRICS);
            // loss_and_act; det (deterministic_decoder.py:63-80): criterion in the tcp frame, prediction in the world frame, no noise; mixture head: the serial loss kernel on every engine
            if (det) launch_det_head_loss<T>(st, H1, det_w, det_b32, acts, b->robot_obs, B, S, det_crit, 1, 0.f, nullptr, rowloss, 8, nullptr, dpre);
            else launch_logistic_loss<T>(st, false, heads, NHEAD, acts, b->robot_obs, B, S, NMIX, NDIM, cfg.num_classes, cfg.log_scale_min, cfg.gripper_alpha, mcil ? 0 : 1, mcil ? 0 : 1,
                                         0.f, nullptr, rowloss, a_tcp, dheads);
            launch_sum_reduce(st, rowloss, SB * 8, 1.f / SB, valm + pass);
            if (det) launch_det_head_act<T>(st, H1, nullptr, 0, det_w, det_b32, b->robot_obs, acts, B, S, pred, repro ? nullptr : metrics);
            else {
                const float* um = pass == 0 ? nz->u_mix_pp : nz->u_mix_pr;
                const float* ua = pass == 0 ? nz->u_act_pp : nz->u_act_pr;
                if (um) { HIP_CHECK(hipMemcpyAsync(nz_mix, um, sizeof(float) * SB * NDIM * NMIX, hipMemcpyDefault, st)); um = nz_mix; }
                if (ua) { HIP_CHECK(hipMemcpyAsync(nz_act, ua, sizeof(float) * SB * NDIM, hipMemcpyDefault, st)); ua = nz_act; }
                launch_logistic_sample(st, heads, NHEAD, b->robot_obs, acts, um, ua, B, S, NMIX, NDIM, cfg.log_scale_min, mcil ? 0 : 1, mcil ? 0 : 1, site_seed(42 + pass), pred,
                                       repro ? nullptr : metrics);
            }
            if (repro) hipLaunchKernelGGL(val_metrics_kernel, dim3(1), dim3(256), 0, st, (const float*)pred, acts, SB, metrics);
        }
        // val/val_pred_clip_loss (hulc.py:804-808): the CLIP auxiliary loss of the lang modality on the masked rows, forward only
        if (b->is_lang && cfg.use_clip && b->n_aux > 0) {
            const int n = b->n_aux;
            if (n > B) { hulc_set_error("clip aux rows n=%d unsupported (<= B=%d)", n, B); return 1; }
            HIP_CHECK(hipMemcpyAsync(auxrows, b->aux_rows, sizeof(int) * n, hipMemcpyHostToDevice, st));
            clip_proj_fwd(n);
            const bool one_wg = n <= AUX_ROWS_SINGLE;          // the single-workgroup kernel also writes gradients (times 0, into scratch); above 64 rows: loss only
            if (!launch_clip_loss(st, false, img, txt, n, logit_scale, 0.f, valm + 3, one_wg ? dimg : nullptr, one_wg ? dtxt : nullptr, one_wg ? valm + 31 : nullptr, nullptr, clip_rows_ws)) {
                hulc_set_error("clip loss: n=%d rows not covered by this context's workspace (max_batch=%d)", n, maxB); return 1; }
            val_clip_n = n;
        }
        // val/lang_pred_loss, val/lang_contrastive_loss (hulc.py:798-813): the BC-Z / MIA losses of the masked lang rows, forward only (hulc_aux_losses_get)
        bcz_n = mia_n = 0; aux_rows_last = 0;
        if ((aux_bcz || aux_mia) && b->is_lang && b->n_aux > 0) {
            const int n = b->n_aux;
            if (n > B) { hulc_set_error("auxiliary-loss rows n=%d unsupported (<= B=%d)", n, B); return 1; }
            if (!val_clip_n) HIP_CHECK(hipMemcpyAsync(auxrows, b->aux_rows, sizeof(int) * n, hipMemcpyHostToDevice, st));
            if (aux_heads_fwd(b, n, val_clip_n > 0, false, 0)) return 1;
            aux_rows_last = n;
        }
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in validate"); return 1; }
        if (plan_pp_out && hulc) HIP_CHECK(hipMemcpyAsync(plan_pp_out, pidx_pp, sizeof(int) * B * NCAT, hipMemcpyDefault, st));
        if (plan_pr_out && hulc) HIP_CHECK(hipMemcpyAsync(plan_pr_out, pidx, sizeof(int) * B * NCAT, hipMemcpyDefault, st));
        if (pred_pp_out) HIP_CHECK(hipMemcpyAsync(pred_pp_out, pred_pp, sizeof(float) * SB * 7, hipMemcpyDefault, st));
        if (pred_pr_out && (hulc || mcil)) HIP_CHECK(hipMemcpyAsync(pred_pr_out, pred_pr, sizeof(float) * SB * 7, hipMemcpyDefault, st));
        float h[32];
        HIP_CHECK(hipMemcpyAsync(h, valm, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (out17) {
            out17[0] = h[0]; out17[1] = h[1]; out17[2] = h[2]; out17[3] = h[14]; out17[4] = h[22];
            for (int i = 0; i < 6; ++i) { out17[5 + i] = h[8 + i]; out17[11 + i] = h[16 + i]; }
            out17[17] = h[3];
        }
        return 0;
    }

    // ---------------------------------------------------------------- CLIP ground-truth metric (hulc.py:967-974, 980-1043)
    // encode: language_goal(lang_emb) then proj_vis_lang.mlp_lang, kept as fp32 (m, GOAL) in `slot` (0: training instructions, 1: validation
    // instructions) until the next encode of that slot.  scores: exp(logit_scale) * normalised image projections of the masked rows of the LAST
    // hulc_validate (lang modality) times the normalised slot rows -> (n, m) on the host.  Both overwrite goal-encoder activations: not between a
    // forward and its backward.
    int val_clip_n = 0;
    float* gt_txt[2] = {nullptr, nullptr}; int gt_m[2] = {0, 0}, gt_cap[2] = {0, 0};
    float *gt_in = nullptr, *gt_out = nullptr; int64_t gt_in_cap = 0, gt_out_cap = 0;
    template <typename U> bool gt_grow(U*& p, int64_t& cap, int64_t n) {
        if (n <= cap) return true;
        void* q = nullptr;
        if (hipMalloc(&q, n * sizeof(U) + 256) != hipSuccess) return false;
        allocs.push_back(q);       // the old block stays until the engine goes: kernels in flight may still read it
        p = (U*)q; cap = n;
        return true;
    }
    int clip_gt_encode(const float* lang_emb, int m, int slot) override {
        if (!bound) { hulc_set_error("hulc_clip_gt_encode before hulc_bind_params"); return 1; }
        if (!cfg.use_clip || cfg.kind != HULC_KIND_HULC) { hulc_set_error("hulc_clip_gt_encode: the context has no CLIP head (use_clip_auxiliary_loss, hulc.py:703)"); return 1; }
        if (have_fwd) { hulc_set_error("hulc_clip_gt_encode between a forward and its backward"); return 1; }
        if (slot < 0 || slot > 1 || m < 1 || !lang_emb) { hulc_set_error("hulc_clip_gt_encode: slot %d, m %d", slot, m); return 1; }
        int64_t capi = gt_cap[slot];
        if (!gt_grow(gt_txt[slot], capi, (int64_t)m * GOAL) || !gt_grow(gt_in, gt_in_cap, (int64_t)m * LANG)) { hulc_set_error("hulc_clip_gt_encode: allocation failed"); return 1; }
        gt_cap[slot] = (int)capi;
        HIP_CHECK(hipMemcpyAsync(gt_in, lang_emb, sizeof(float) * (int64_t)m * LANG, hipMemcpyDefault, st));
        T* acts[2] = {gl1, gl2};
        for (int r0 = 0; r0 < m; r0 += maxB) {
            const int rows = std::min(maxB, m - r0);
            hipLaunchKernelGGL((cast_kernel<float, T>), dim3(cdiv(rows * LANG, 256)), dim3(256), 0, st, gt_in + (int64_t)r0 * LANG, lang_t, (long long)rows * LANG);
            mlp_fwd(lang_t, LANG, rows, lg, 3, acts, gl3, nullptr);
            ln_fwd(gl3, GOAL, rows, GOAL, ln_lg_g, ln_lg_b, goal_t, GOAL, nullptr, 0, goal_st);
            { EpiP ep = epi(la1, false); ep.relu = 1; lin_fwd(goal_t, GOAL, rows, cl_la0, ep, 128); }
            { EpiP ep = epi(gt_txt[slot] + (int64_t)r0 * GOAL, true); lin_fwd(la1, 128, rows, cl_la2, ep, GOAL); }
        }
        gt_m[slot] = m;
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in hulc_clip_gt_encode"); return 1; }
        HIP_CHECK(hipStreamSynchronize(st));          // lang_emb may be a host buffer the caller frees
        return 0;
    }
    int clip_gt_scores(int slot, float* out_host, int64_t cap, int32_t* n_out, int32_t* m_out) override {
        if (slot < 0 || slot > 1 || gt_m[slot] < 1) { hulc_set_error("hulc_clip_gt_scores: slot %d holds no encoded instructions", slot); return 1; }
        if (val_clip_n < 1) { hulc_set_error("hulc_clip_gt_scores: the last hulc_validate had no masked lang rows (hulc.py:988-989 returns early)"); return 1; }
        const int n = val_clip_n, m = gt_m[slot];
        if (n_out) *n_out = n;
        if (m_out) *m_out = m;
        if (!out_host && cap == 0) return 0;                                   // shape query
        if (!out_host || cap < (int64_t)n * m) { hulc_set_error("hulc_clip_gt_scores: buffer of %lld floats, need %lld", (long long)cap, (long long)n * m); return 1; }
        if (!gt_grow(gt_out, gt_out_cap, (int64_t)n * m)) { hulc_set_error("hulc_clip_gt_scores: allocation failed"); return 1; }
        hipLaunchKernelGGL(clip_gt_scores_kernel, dim3(cdiv(m, 64), n), dim3(64), 0, st, img, gt_txt[slot], n, m, GOAL, logit_scale, gt_out);
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in hulc_clip_gt_scores"); return 1; }
        HIP_CHECK(hipMemcpyAsync(out_host, gt_out, sizeof(float) * (int64_t)n * m, hipMemcpyDefault, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }

    // ---------------------------------------------------------------- rollout (hulc.py:843-957), B = 1
    int* roll_plan = nullptr; T* roll_plan_c = nullptr; T *roll_goal = nullptr, *roll_h0 = nullptr, *roll_h1 = nullptr;
    float *roll_fs = nullptr, *roll_fg = nullptr, *roll_ro = nullptr, *roll_pred = nullptr, *roll_pred_goal = nullptr;
    bool roll_has_h = false, roll_has_plan = false;
    uint64_t roll_counter = 0;
    void roll_alloc() {
        if (roll_plan) return;
        val_alloc();
        roll_plan = alloc<int>(NCAT); roll_plan_c = alloc<T>(PLAN); roll_goal = alloc<T>(GOAL);
        if (!mlp) { roll_h0 = alloc<T>(HID); roll_h1 = alloc<T>(HID); }
        roll_fs = alloc<float>(2ll * 3 * encS.IH * encS.IH); roll_fg = alloc<float>(2ll * 3 * encG.IH * encG.IH);
        roll_ro = alloc<float>(16); roll_pred = alloc<float>(8); roll_pred_goal = alloc<float>(GOAL);
    }
    int rollout_reset() override { roll_has_h = false; roll_has_plan = false; roll_counter = 0; return 0; }
    int rollout_plan(const hulc_rollout_obs* obs, const float* goal_static, const float* goal_gripper, const float* goal_lang, const int32_t* plan_inject,
                     int32_t* plan_out) override {
        if (!bound) { hulc_set_error("hulc_rollout_plan before hulc_bind_params"); return 1; }
        const bool gcbc = cfg.kind == HULC_KIND_GCBC;      // gcbc.py:286-320: only the latent goal is encoded (once per rollout), the decoder acts without a plan
        if ((goal_lang != nullptr) == (goal_static != nullptr && goal_gripper != nullptr)) {
            hulc_set_error("hulc_rollout_plan: give either the two goal images or the language embedding");
            return 1;
        }
        if (maxS < 2 && !goal_lang) { hulc_set_error("hulc_rollout_plan: a visual goal needs max_seq >= 2 (obs + goal frame form one window, hulc.py:917-919)"); return 1; }
        roll_alloc();
        if (alloc_failed) { hulc_set_error("hulc_rollout_plan: workspace allocation failed"); return 1; }
        have_fwd = false; pair = false;
        hulc_batch bb; memset(&bb, 0, sizeof(bb));
        bb.B = 1; bb.step = roll_counter;
        if (goal_lang) {
            bb.S = 1; bb.is_lang = 1; bb.rgb_static = obs->rgb_static; bb.rgb_gripper = obs->rgb_gripper; bb.lang = goal_lang;
        } else {
            const size_t ns = sizeof(float) * 3 * encS.IH * encS.IH, ng = sizeof(float) * 3 * encG.IH * encG.IH;
            HIP_CHECK(hipMemcpyAsync(roll_fs, obs->rgb_static, ns, hipMemcpyDefault, st));
            HIP_CHECK(hipMemcpyAsync((char*)roll_fs + ns, goal_static, ns, hipMemcpyDefault, st));
            HIP_CHECK(hipMemcpyAsync(roll_fg, obs->rgb_gripper, ng, hipMemcpyDefault, st));
            HIP_CHECK(hipMemcpyAsync((char*)roll_fg + ng, goal_gripper, ng, hipMemcpyDefault, st));
            bb.S = 2; bb.is_lang = 0; bb.rgb_static = roll_fs; bb.rgb_gripper = roll_fg;
        }
        cur = bb;
        trunk_fwd(&bb, 0.f);
        const int* inj = nullptr;
        if (mcil) {     // continuous plan (256) fp32: sampled from the proposal Normal or injected; kept in roll_plan_c for the following act() calls
            sample_cont(pp_logits, nullptr, reinterpret_cast<const float*>(plan_inject), 1, site_seed(50));
            HIP_CHECK(hipMemcpyAsync(roll_plan_c, plan_t, sizeof(T) * (PLAN / 2), hipMemcpyDeviceToDevice, st));
            if (plan_out) HIP_CHECK(hipMemcpyAsync(plan_out, plan_f, sizeof(float) * (PLAN / 2), hipMemcpyDefault, st));
        } else if (!gcbc) {
        if (plan_inject) { HIP_CHECK(hipMemcpyAsync(pidx_in, plan_inject, sizeof(int) * NCAT, hipMemcpyDefault, st)); inj = pidx_in; }
        launch_plan_kl_sample(st, pp_logits, nullptr, 1, NCAT, NCLS, inj, roll_plan, probs, klcat, dpp_kl, dpr_kl, 0.f, 0.f, site_seed(50), nullptr);
        }
        HIP_CHECK(hipMemcpyAsync(roll_goal, goal_t, sizeof(T) * GOAL, hipMemcpyDeviceToDevice, st));
        if (!gcbc) roll_has_h = false;                 // action_decoder.clear_hidden_state() (hulc.py:925 / :946); GCBC.step never clears it (gcbc.py:286-320)
        roll_has_plan = true;
        if (plan_out && !mcil && !gcbc) HIP_CHECK(hipMemcpyAsync(plan_out, roll_plan, sizeof(int) * NCAT, hipMemcpyDefault, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in rollout_plan"); return 1; }
        return 0;
    }
    // the latent goal / plan of a rollout as VALUES (hulc.py:881-948: predict_with_plan / get_pp_plan_* take and return them)
    int rollout_get_goal(float* latent_goal_out) override {
        if (!roll_has_plan) { hulc_set_error("hulc_rollout_get_goal before hulc_rollout_plan"); return 1; }
        hipLaunchKernelGGL((cast_kernel<T, float>), dim3(1), dim3(64), 0, st, roll_goal, roll_pred_goal, (long long)GOAL);
        HIP_CHECK(hipMemcpyAsync(latent_goal_out, roll_pred_goal, sizeof(float) * GOAL, hipMemcpyDefault, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    int rollout_set_state(const void* plan, const float* latent_goal) override {
        if (!bound) { hulc_set_error("hulc_rollout_set_state before hulc_bind_params"); return 1; }
        const bool gcbc = cfg.kind == HULC_KIND_GCBC;
        if (!gcbc && !plan) { hulc_set_error("hulc_rollout_set_state: null plan"); return 1; }
        roll_alloc();
        if (alloc_failed) { hulc_set_error("hulc_rollout_set_state: workspace allocation failed"); return 1; }
        HIP_CHECK(hipMemcpyAsync(roll_pred_goal, latent_goal, sizeof(float) * GOAL, hipMemcpyDefault, st));
        hipLaunchKernelGGL((cast_kernel<float, T>), dim3(1), dim3(64), 0, st, roll_pred_goal, roll_goal, (long long)GOAL);
        if (mcil) {
            HIP_CHECK(hipMemcpyAsync(plan_f, plan, sizeof(float) * (PLAN / 2), hipMemcpyDefault, st));
            hipLaunchKernelGGL((cast_kernel<float, T>), dim3(1), dim3(256), 0, st, plan_f, roll_plan_c, (long long)(PLAN / 2));
        } else if (!gcbc) {
            HIP_CHECK(hipMemcpyAsync(roll_plan, plan, sizeof(int) * NCAT, hipMemcpyDefault, st));
            // a caller-supplied class index is a column of the plan embedding gather in dec_fwd: keep it inside [0, NCLS) (ADVICE r5)
            hipLaunchKernelGGL(clamp_index_kernel, dim3(1), dim3(64), 0, st, roll_plan, NCAT, NCLS);
        }
        HIP_CHECK(hipStreamSynchronize(st));
        roll_has_plan = true;
        return 0;
    }
    int rollout_act(const hulc_rollout_obs* obs, const float* u_mix, const float* u_act, float* action_out) override {
        if (!roll_has_plan) { hulc_set_error("hulc_rollout_act before hulc_rollout_plan (Hulc.step replans at rollout_step_counter %% replan_freq == 0)"); return 1; }
        have_fwd = false;
        hulc_batch bb; memset(&bb, 0, sizeof(bb));
        bb.B = 1; bb.S = 1; bb.step = roll_counter++;
        cur = bb;
        const Conv1Src src[2] = {conv1_src_f32(obs->rgb_static), conv1_src_f32(obs->rgb_gripper)};
        enc_fwd_both(src, nullptr, 1, false);
        HIP_CHECK(hipMemcpyAsync(goal_t, roll_goal, sizeof(T) * GOAL, hipMemcpyDeviceToDevice, st));
        if (mcil) HIP_CHECK(hipMemcpyAsync(plan_t, roll_plan_c, sizeof(T) * (PLAN / 2), hipMemcpyDeviceToDevice, st));
        if (mlp) dec_fwd(roll_plan, 1, 1, nullptr, nullptr);      // feed-forward body: h_n is None (rnn.py mlp_decoder), nothing is kept between steps
        else {
        dec_fwd(roll_plan, 1, 1, roll_has_h ? roll_h0 : nullptr, roll_has_h ? roll_h1 : nullptr);
        HIP_CHECK(hipMemcpyAsync(roll_h0, H0, sizeof(T) * HID, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemcpyAsync(roll_h1, H1, sizeof(T) * HID, hipMemcpyDeviceToDevice, st));
        roll_has_h = true;
        }
        HIP_CHECK(hipMemcpyAsync(roll_ro, obs->robot_obs_raw, sizeof(float) * 15, hipMemcpyDefault, st));
        if (det) { u_mix = u_act = nullptr; launch_det_head_act<T>(st, H1, nullptr, 0, det_w, det_b32, roll_ro, nullptr, 1, 1, roll_pred, nullptr); }      // deterministic head: the noise is ignored
        if (u_mix) { HIP_CHECK(hipMemcpyAsync(nz_mix, u_mix, sizeof(float) * NDIM * NMIX, hipMemcpyDefault, st)); u_mix = nz_mix; }
        if (u_act) { HIP_CHECK(hipMemcpyAsync(nz_act, u_act, sizeof(float) * NDIM, hipMemcpyDefault, st)); u_act = nz_act; }
        if (!det) launch_logistic_sample(st, heads, NHEAD, roll_ro, nullptr, u_mix, u_act, 1, 1, NMIX, NDIM, cfg.log_scale_min, mcil ? 0 : 1, mcil ? 0 : 1, site_seed(51), roll_pred, nullptr);
        HIP_CHECK(hipMemcpyAsync(action_out, roll_pred, sizeof(float) * 7, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in rollout_act"); return 1; }
        return 0;
    }

