// hulc_amd/csrc/engine_rollout_envs.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body: the batched
// multi-environment rollout (hulc_rollout_envs_*): max_envs independent policy slots per context, n of them planned / stepped by one call.  Kernels and the
// state layout: rollout_step.h.  Separate from the B = 1 rollout state (engine_inference.inc: roll_*): neither family reads or writes the other's state;
// both use the forward workspace (emb, goal_t, heads ...) as scratch within a call.  Not a standalone header.
    int env_max = 0, env_cap = 0;
    std::vector<unsigned char> env_has_plan, env_par;       // host mirrors: arguments are validated before the first launch; env_par = which hidden-state buffer is current
    std::vector<int> env_desc;                              // the call's row descriptors, slot | parity << 16
    int *env_plan_i = nullptr, *env_rows = nullptr, *env_pidx = nullptr; int* env_rows_host = nullptr;
    float *env_plan_f = nullptr, *env_cache = nullptr, *env_ro = nullptr, *env_pred = nullptr, *env_goal_f = nullptr, *env_fs = nullptr, *env_fg = nullptr;
    T *env_goal = nullptr, *env_h0 = nullptr, *env_h1 = nullptr, *env_ha = nullptr, *env_hb = nullptr;
    uint64_t env_counter = 0;
    int env_pc() const { return mcil ? PLAN / 2 : 0; }
    int env_ncat() const { return cfg.kind == HULC_KIND_HULC ? NCAT : 0; }

    int rollout_envs_init(int max_envs) override {
        if (!bound) { hulc_set_error("hulc_rollout_envs_init before hulc_bind_params"); return 1; }
        if (max_envs < 1 || max_envs > maxB || max_envs > ENV_MAX_ROWS) {
            hulc_set_error("hulc_rollout_envs_init: max_envs %d outside [1, min(max_batch = %d, %d)]", max_envs, maxB, ENV_MAX_ROWS);
            return 1;
        }
        val_alloc();
        if (max_envs > env_cap) {       // a larger table: new blocks (the old ones stay until the engine goes, like every workspace block)
            const int64_t S = max_envs;
            env_plan_i = alloc<int>(S * NCAT); env_plan_f = alloc<float>(S * 256); env_goal = alloc<T>(S * GOAL);
            if (!mlp) { env_h0 = alloc<T>(2 * S * HID); env_h1 = alloc<T>(2 * S * HID); }      // the feed-forward body has no per-slot hidden state
            env_cache = alloc<float>(S * HID);
            env_rows = alloc<int>(S); env_pidx = alloc<int>(S * NCAT); env_ro = alloc<float>(S * 16); env_pred = alloc<float>(S * 8); env_goal_f = alloc<float>(S * GOAL);
            if (std::is_same<T, float>::value && !mlp) { env_ha = alloc<T>(S * HID); env_hb = alloc<T>(S * HID); }
            if (maxS >= 2) { env_fs = alloc<float>(2 * S * 3 * encS.IH * encS.IH); env_fg = alloc<float>(2 * S * 3 * encG.IH * encG.IH); }
            if (env_rows_host) { hipHostFree(env_rows_host); env_rows_host = nullptr; }
            if (hipHostMalloc((void**)&env_rows_host, sizeof(int) * S, hipHostMallocDefault) != hipSuccess) alloc_failed = true;
            if (alloc_failed) { env_cap = env_max = 0; hulc_set_error("hulc_rollout_envs_init: workspace allocation failed"); return 1; }
            env_cap = max_envs;
        }
        env_max = max_envs;
        env_has_plan.assign(env_max, 0); env_par.assign(env_max, 0);
        if (!mlp) {
        HIP_CHECK(hipMemsetAsync(env_h0, 0, sizeof(T) * 2 * env_cap * HID, st));
        HIP_CHECK(hipMemsetAsync(env_h1, 0, sizeof(T) * 2 * env_cap * HID, st));
        }
        env_counter = 0;
        return 0;
    }
    // the checks every call shares; fills env_desc (no state is touched).  slots == nullptr: rows 0..n-1 (reset: every slot, n ignored)
    int env_check(const char* fn, int n, const int32_t* slots, bool all_if_null, bool need_plan) {
        if (env_max < 1) { hulc_set_error("%s before hulc_rollout_envs_init", fn); return 1; }
        if (!slots && all_if_null) n = env_max;
        if (n < 1 || n > env_max) { hulc_set_error("%s: n = %d outside [1, max_envs = %d]", fn, n, env_max); return 1; }
        env_desc.assign(n, 0);
        unsigned long long seen = 0;       // max_envs <= 64
        for (int r = 0; r < n; ++r) {
            const int s = slots ? slots[r] : r;
            if (s < 0 || s >= env_max) { hulc_set_error("%s: row %d names slot %d outside [0, max_envs = %d)", fn, r, s, env_max); return 1; }
            if (seen >> s & 1ull) { hulc_set_error("%s: slot %d is named more than once", fn, s); return 1; }
            seen |= 1ull << s;
            if (need_plan && !env_has_plan[s]) { hulc_set_error("%s: slot %d has no plan (hulc_rollout_envs_plan / hulc_rollout_envs_set_state first)", fn, s); return 1; }
            env_desc[r] = s | ((int)env_par[s] << 16);
        }
        return 0;
    }
    // one host -> device copy of the row descriptors per call (through a pinned staging block: every call ends in a stream synchronisation before the next refill)
    int env_upload_rows() {
        const int n = (int)env_desc.size();
        memcpy(env_rows_host, env_desc.data(), sizeof(int) * n);
        HIP_CHECK(hipMemcpyAsync(env_rows, env_rows_host, sizeof(int) * n, hipMemcpyHostToDevice, st));
        return 0;
    }
    // plan / goal rows of the call (pidx or plan_f, goal_t) -> their slots (+ the cached decoder input term of the 16-bit engines)
    void env_store(int n, const int* pidx_rows, const float* planf_rows, bool zero_hidden) {
        EnvStoreP q{};
        q.rowdesc = env_rows; q.n = n; q.max_envs = env_cap; q.pidx = env_ncat() ? pidx_rows : nullptr; q.plan_f = mcil ? planf_rows : nullptr; q.goal = goal_t;
        q.NCAT = env_ncat(); q.NCLS = NCLS; q.PC = env_pc(); q.s_plan_i = env_plan_i; q.s_plan_f = env_plan_f; q.s_goal = env_goal;
        q.wT = std::is_same<T, float>::value ? nullptr : (const void*)wih0T; q.grow0 = dec_plan + DE; q.b1 = bih0; q.b2 = bhh0; q.s_cache = env_cache;
        q.h0 = env_h0; q.h1 = env_h1; q.zero_hidden = zero_hidden ? 1 : 0;
        hipLaunchKernelGGL((env_plan_store_kernel<T>), dim3(HID / 256, n), dim3(256), 0, st, q);
    }
    int rollout_envs_reset(int n, const int32_t* slots, int clear_hidden) override {
        if (env_check("hulc_rollout_envs_reset", n, slots, true, false)) return 1;
        n = (int)env_desc.size();
        const bool zero = !mlp && (cfg.kind != HULC_KIND_GCBC || clear_hidden != 0);      // feed-forward body: only the plans are dropped      // GCBC.reset drops the goal only (gcbc.py:281-285)
        if (zero) {
            if (env_upload_rows()) return 1;
            hipLaunchKernelGGL((env_zero_hidden_kernel<T>), dim3(n), dim3(256), 0, st, env_rows, env_cap, env_h0, env_h1);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        for (int r = 0; r < n; ++r) env_has_plan[env_desc[r] & 0xffff] = 0;
        return 0;
    }
    int rollout_envs_plan(const hulc_rollout_envs_obs* obs, const float* goal_static, const float* goal_gripper, const float* goal_lang, const void* plan_inject,
                          void* plan_out, float* latent_goal_out) override {
        const char* fn = "hulc_rollout_envs_plan";
        if (env_check(fn, obs->n, obs->slots, false, false)) return 1;
        if ((goal_lang != nullptr) == (goal_static != nullptr && goal_gripper != nullptr) || (goal_lang && (goal_static || goal_gripper))) {
            hulc_set_error("%s: give either the two goal images or the language embeddings (exactly one goal kind per call)", fn);
            return 1;
        }
        if (maxS < 2 && !goal_lang) { hulc_set_error("%s: a visual goal needs max_seq >= 2 (obs + goal frame form one window, hulc.py:917-919)", fn); return 1; }
        const bool gcbc = cfg.kind == HULC_KIND_GCBC;
        const int n = obs->n;
        if (env_upload_rows()) return 1;
        have_fwd = false; pair = false;
        hulc_batch bb; memset(&bb, 0, sizeof(bb));
        bb.B = n; bb.step = env_counter++;
        if (goal_lang) {
            bb.S = 1; bb.is_lang = 1; bb.rgb_static = obs->rgb_static; bb.rgb_gripper = obs->rgb_gripper; bb.lang = goal_lang;
        } else {          // (obs, goal) 2-frame windows, interleaved per row: four strided copies whatever n is
            const size_t ns = sizeof(float) * 3 * encS.IH * encS.IH, ng = sizeof(float) * 3 * encG.IH * encG.IH;
            HIP_CHECK(hipMemcpy2DAsync(env_fs, 2 * ns, obs->rgb_static, ns, ns, n, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpy2DAsync((char*)env_fs + ns, 2 * ns, goal_static, ns, ns, n, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpy2DAsync(env_fg, 2 * ng, obs->rgb_gripper, ng, ng, n, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpy2DAsync((char*)env_fg + ng, 2 * ng, goal_gripper, ng, ng, n, hipMemcpyDeviceToDevice, st));
            bb.S = 2; bb.is_lang = 0; bb.rgb_static = env_fs; bb.rgb_gripper = env_fg;
        }
        cur = bb;
        trunk_fwd(&bb, 0.f);
        if (mcil) sample_cont(pp_logits, nullptr, reinterpret_cast<const float*>(plan_inject), n, site_seed(52));
        else if (!gcbc) {
            const int* inj = nullptr;
            if (plan_inject) { HIP_CHECK(hipMemcpyAsync(pidx_in, plan_inject, sizeof(int) * n * NCAT, hipMemcpyDefault, st)); inj = pidx_in; }
            launch_plan_kl_sample(st, pp_logits, nullptr, n, NCAT, NCLS, inj, env_pidx, probs, klcat, dpp_kl, dpr_kl, 0.f, 0.f, site_seed(52), nullptr);
        }
        env_store(n, env_pidx, mcil ? plan_f : nullptr, !gcbc && !mlp);       // action_decoder.clear_hidden_state() per planned slot (hulc.py:925 / :946); GCBC.step never clears it
        if (plan_out && mcil) HIP_CHECK(hipMemcpyAsync(plan_out, plan_f, sizeof(float) * n * (PLAN / 2), hipMemcpyDefault, st));
        if (plan_out && !mcil && !gcbc) {      // what the slots hold (an injected index comes back clamped into [0, NCLS))
            EnvGatherP g{}; g.rowdesc = env_rows; g.n = n; g.max_envs = env_cap; g.NCAT = NCAT; g.s_plan_i = env_plan_i; g.s_goal = env_goal; g.pidx = env_pidx;
            hipLaunchKernelGGL((env_gather_kernel<T>), dim3(n), dim3(256), 0, st, g);
            HIP_CHECK(hipMemcpyAsync(plan_out, env_pidx, sizeof(int) * n * NCAT, hipMemcpyDefault, st));
        }
        if (latent_goal_out) {
            hipLaunchKernelGGL((cast_kernel<T, float>), dim3(cdiv(n * GOAL, 256)), dim3(256), 0, st, goal_t, env_goal_f, (long long)n * GOAL);
            HIP_CHECK(hipMemcpyAsync(latent_goal_out, env_goal_f, sizeof(float) * n * GOAL, hipMemcpyDefault, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in %s", fn); return 1; }
        for (int r = 0; r < n; ++r) env_has_plan[env_desc[r] & 0xffff] = 1;
        return 0;
    }
    int rollout_envs_get_state(int n, const int32_t* slots, void* plan_out, float* latent_goal_out) override {
        if (env_check("hulc_rollout_envs_get_state", n, slots, false, true)) return 1;
        if (env_upload_rows()) return 1;
        EnvGatherP g{}; g.rowdesc = env_rows; g.n = n; g.max_envs = env_cap; g.NCAT = env_ncat(); g.PC = env_pc();
        g.s_plan_i = env_plan_i; g.s_plan_f = env_plan_f; g.s_goal = env_goal; g.pidx = env_ncat() ? env_pidx : nullptr; g.plan_f = mcil ? plan_f : nullptr; g.goal_f = env_goal_f;
        hipLaunchKernelGGL((env_gather_kernel<T>), dim3(n), dim3(256), 0, st, g);
        if (plan_out && mcil) HIP_CHECK(hipMemcpyAsync(plan_out, plan_f, sizeof(float) * n * (PLAN / 2), hipMemcpyDefault, st));
        if (plan_out && env_ncat()) HIP_CHECK(hipMemcpyAsync(plan_out, env_pidx, sizeof(int) * n * NCAT, hipMemcpyDefault, st));
        if (latent_goal_out) HIP_CHECK(hipMemcpyAsync(latent_goal_out, env_goal_f, sizeof(float) * n * GOAL, hipMemcpyDefault, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    int rollout_envs_set_state(int n, const int32_t* slots, const void* plan, const float* latent_goal) override {
        const char* fn = "hulc_rollout_envs_set_state";
        if (env_check(fn, n, slots, false, false)) return 1;
        if (cfg.kind != HULC_KIND_GCBC && !plan) { hulc_set_error("%s: null plan", fn); return 1; }
        if (env_upload_rows()) return 1;
        HIP_CHECK(hipMemcpyAsync(env_goal_f, latent_goal, sizeof(float) * n * GOAL, hipMemcpyDefault, st));
        hipLaunchKernelGGL((cast_kernel<float, T>), dim3(cdiv(n * GOAL, 256)), dim3(256), 0, st, env_goal_f, goal_t, (long long)n * GOAL);
        if (mcil) HIP_CHECK(hipMemcpyAsync(plan_f, plan, sizeof(float) * n * (PLAN / 2), hipMemcpyDefault, st));
        else if (env_ncat()) HIP_CHECK(hipMemcpyAsync(env_pidx, plan, sizeof(int) * n * NCAT, hipMemcpyDefault, st));
        env_store(n, env_pidx, mcil ? plan_f : nullptr, false);       // like hulc_rollout_set_state: the hidden state is not touched
        HIP_CHECK(hipStreamSynchronize(st));
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in %s", fn); return 1; }
        for (int r = 0; r < n; ++r) env_has_plan[env_desc[r] & 0xffff] = 1;
        return 0;
    }
    // 16-bit engines: heads GEMM + sampler over the new layer-1 state of every row's slot (byrow: over rows 0..n-1 of the feed-forward body's row buffer; never mcil)
    void env_heads_sample(int n, const T* h1, bool byrow, const float* u_mix, const float* u_act) {
        EnvHeadsP hp{};
        hp.rowdesc = env_rows; hp.n = n; hp.max_envs = env_cap; hp.h1 = h1; hp.W = wheads; hp.bias = bheads; hp.robot_obs = env_ro; hp.u_mix = u_mix; hp.u_act = u_act;
        hp.NMIX = NMIX; hp.NDIM = NDIM; hp.log_scale_min = cfg.log_scale_min; hp.gripper_control = mcil ? 0 : 1; hp.discrete_gripper = mcil ? 0 : 1;
        hp.seed = site_seed(53); hp.pred = env_pred;
        launch_env_heads_sample(st, hp, NHEAD, byrow);
    }
    int rollout_envs_act(const hulc_rollout_envs_obs* obs, const float* u_mix, const float* u_act, float* actions_out) override {
        const char* fn = "hulc_rollout_envs_act";
        if (env_check(fn, obs->n, obs->slots, false, true)) return 1;
        const int n = obs->n;
        if (env_upload_rows()) return 1;
        have_fwd = false; pair = false;
        hulc_batch bb; memset(&bb, 0, sizeof(bb));
        bb.B = n; bb.S = 1; bb.step = env_counter++;
        cur = bb;
        HIP_CHECK(hipMemcpyAsync(env_ro, obs->robot_obs_raw, sizeof(float) * 15 * n, hipMemcpyDefault, st));
        if (det) u_mix = u_act = nullptr;      // deterministic head: the noise is ignored
        if (u_mix) { HIP_CHECK(hipMemcpyAsync(nz_mix, u_mix, sizeof(float) * n * NDIM * NMIX, hipMemcpyDefault, st)); u_mix = nz_mix; }
        if (u_act) { HIP_CHECK(hipMemcpyAsync(nz_act, u_act, sizeof(float) * n * NDIM, hipMemcpyDefault, st)); u_act = nz_act; }
        const Conv1Src src[2] = {conv1_src_f32(obs->rgb_static), conv1_src_f32(obs->rgb_gripper)};
        enc_fwd_both(src, nullptr, n, false);
        if (mlp && std::is_same<T, h16_t>::value) {
            if constexpr (std::is_same<T, h16_t>::value) {
            // feed-forward body, 16 bit: embedding -> actions in four launches, the recurrence-free forms of the row kernels (rollout_step.h).  a0 / a1 / y are rows
            // 0..n-1 of the decoder's forward workspace (H0 / H1 / Zx1, n <= max_batch rows); nothing goes back to the slots and no parity is read
            auto a16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
            EnvLayerP l{};
            l.rowdesc = env_rows; l.n = n; l.max_envs = env_cap; l.x = emb + (EMB - DE); l.x_ld = EMB; l.Kx = DE;
            l.Wx = wih0 + dec_plan; l.wx_ld = KIN; l.h = H0; l.ctab = env_cache; l.w16 = a16(l.Wx) && (KIN % 8) == 0;
            hipLaunchKernelGGL((env_rnn_layer_kernel<false, true>), dim3(HID / ENV_COLS), dim3(ENV_WAVES * 64), 0, st, l);
            l.x = H0; l.x_ld = HID; l.Kx = HID; l.Wx = mlp1.W; l.wx_ld = HID; l.h = H1; l.ctab = nullptr; l.b1 = mlp1.b32; l.w16 = a16(l.Wx);
            hipLaunchKernelGGL((env_rnn_layer_kernel<false, true>), dim3(HID / ENV_COLS), dim3(ENV_WAVES * 64), 0, st, l);
            l.x = H1; l.Wx = mlp2.W; l.h = Zx1; l.b1 = mlp2.b32; l.w16 = a16(l.Wx);
            hipLaunchKernelGGL((env_rnn_layer_kernel<false, false>), dim3(HID / ENV_COLS), dim3(ENV_WAVES * 64), 0, st, l);
            env_heads_sample(n, Zx1, true, u_mix, u_act);
            }
        } else if (mlp) {
            // feed-forward body, fp32 engine: slot plan / goal -> rows, dec_fwd at B = n, S = 1, the validation sampler; no state goes back to the slots
            EnvGatherP g{}; g.rowdesc = env_rows; g.n = n; g.max_envs = env_cap; g.NCAT = env_ncat(); g.PC = 0;
            g.s_plan_i = env_plan_i; g.s_plan_f = env_plan_f; g.s_goal = env_goal; g.pidx = env_ncat() ? env_pidx : nullptr; g.goal_t = goal_t;
            hipLaunchKernelGGL((env_gather_kernel<T>), dim3(n), dim3(256), 0, st, g);
            dec_fwd(env_pidx, n, 1, nullptr, nullptr);
            launch_logistic_sample(st, heads, NHEAD, env_ro, nullptr, u_mix, u_act, n, 1, NMIX, NDIM, cfg.log_scale_min, 1, 1, site_seed(53), env_pred, nullptr);
        } else if constexpr (std::is_same<T, h16_t>::value) {
            // embedding -> actions: three launches, no copy (rollout_step.h)
            auto a16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
            EnvLayerP l0{};
            l0.rowdesc = env_rows; l0.n = n; l0.max_envs = env_cap; l0.x = emb + (EMB - DE); l0.x_ld = EMB; l0.x_by_slot = 0; l0.Kx = DE;
            l0.Wx = wih0 + dec_plan; l0.wx_ld = KIN; l0.Whh = whh0.W; l0.h = env_h0; l0.ctab = env_cache;
            l0.w16 = a16(l0.Wx) && a16(l0.Whh) && (KIN % 8) == 0;
            hipLaunchKernelGGL((env_rnn_layer_kernel<true, true>), dim3(HID / ENV_COLS), dim3(ENV_WAVES * 64), 0, st, l0);
            EnvLayerP l1{};
            l1.rowdesc = env_rows; l1.n = n; l1.max_envs = env_cap; l1.x = env_h0; l1.x_ld = HID; l1.x_by_slot = 1; l1.Kx = HID;
            l1.Wx = wih1.W; l1.wx_ld = HID; l1.Whh = whh1.W; l1.h = env_h1; l1.ctab = nullptr; l1.b1 = bih1; l1.b2 = bhh1;
            l1.w16 = a16(l1.Wx) && a16(l1.Whh);
            hipLaunchKernelGGL((env_rnn_layer_kernel<true, true>), dim3(HID / ENV_COLS), dim3(ENV_WAVES * 64), 0, st, l1);
            if (det) launch_det_head_act<T>(st, env_h1, env_rows, env_cap, det_w, det_b32, env_ro, nullptr, n, 1, env_pred, nullptr);      // the new layer-1 state of every row's slot
            else env_heads_sample(n, env_h1, false, u_mix, u_act);
        } else {
            // the fp32 parity engine composes the generic path: slot state -> rows, dec_fwd at B = n, S = 1, rows -> slots, the validation sampler
            EnvGatherP g{}; g.rowdesc = env_rows; g.n = n; g.max_envs = env_cap; g.NCAT = env_ncat(); g.PC = env_pc();
            g.s_plan_i = env_plan_i; g.s_plan_f = env_plan_f; g.s_goal = env_goal; g.h0 = env_h0; g.h1 = env_h1;
            g.pidx = env_ncat() ? env_pidx : nullptr; g.plan_t = mcil ? (void*)plan_t : nullptr; g.goal_t = goal_t; g.ha = env_ha; g.hb = env_hb;
            hipLaunchKernelGGL((env_gather_kernel<T>), dim3(n), dim3(256), 0, st, g);
            dec_fwd(env_pidx, n, 1, env_ha, env_hb);
            hipLaunchKernelGGL((env_scatter_hidden_kernel<T>), dim3(n), dim3(256), 0, st, env_rows, env_cap, H0, H1, env_h0, env_h1);
            if (det) launch_det_head_act<T>(st, H1, nullptr, 0, det_w, det_b32, env_ro, nullptr, n, 1, env_pred, nullptr);
            else launch_logistic_sample(st, heads, NHEAD, env_ro, nullptr, u_mix, u_act, n, 1, NMIX, NDIM, cfg.log_scale_min, mcil ? 0 : 1, mcil ? 0 : 1, site_seed(53), env_pred, nullptr);
        }
        HIP_CHECK(hipMemcpyAsync(actions_out, env_pred, sizeof(float) * 7 * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (hipGetLastError() != hipSuccess) { hulc_set_error("kernel launch failed in %s", fn); return 1; }
        for (int r = 0; r < n; ++r) env_par[env_desc[r] & 0xffff] ^= 1;       // the stepped slots' new state is in the other buffer
        return 0;
    }
