"""GPU (-m gpu): the CLIP, MIA and BC-Z language auxiliary losses on MORE than 64 flagged rows (csrc/aux_rows.h): the three kernels alone against float64
restatements of their own fp32 inputs, the fp32 step against the one reference fixture with 66 flagged rows (tests/golden/clip_rows72.npz,
tools/gen_golden_rows.py) and against the oracle around the 64-row tile edge, the paired pass, the MIA / BC-Z heads against torch restatements, the
16-bit engines, validation with the CLIP ground-truth scores, and the error paths.  Every gate is one an existing test of the same quantity uses; the
kernel-level gate is measured in the test itself, output by output, on the n = 64 call, which runs the single-workgroup kernels."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hulc_oracle as O  # noqa: E402
from aux_golden_util import IM0, SCALES  # noqa: E402
from aux_rows_util import (CLIP_BETA, bcz_restated, clip_loss64, cosine_dist64, flag_rule, grads_np, kernel_rows, load_rows_case, mia_head64,  # noqa: E402
                           mia_restated, run_step, to_dev)
from golden_util import adam_close, check_grads64, grad_entries, rel_l2, sample_idx  # noqa: E402
from hulc_amd import lib as L  # noqa: E402
from hulc_amd import spec  # noqa: E402
from hulc_amd.utils import synthetic  # noqa: E402

HEADS = ("bc_z_lang_decoder.", "mia_lang_discriminator.", "proj_vis_lang.")
NS = (64, 65, 127, 128, 129, 300)


def _engine(dims, B, S, dtype, **kw):
    from hulc_amd.engine import StepEngine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible — the product path has no CPU fallback")
    return StepEngine(dims, B, S, dtype=dtype, dropout_p=0.0, **kw)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _err(got, ref):
    """rel-L2 of an array, relative error of a scalar."""
    return rel_l2(np.asarray(got, np.float64), np.asarray(ref, np.float64))


FP32_FLOOR = 2.0 ** -24


def _gate_against_n64(label, errs):
    """errs: {n: {output: error}}, rel-L2 for an array and relative error for a scalar, against float64 of the same fp32 inputs.
    Every output has its own yardstick: e64 = its error in the n = 64 call, i.e. in the single-workgroup kernel the project already accepts, and at a
    larger n it may have 2 x e64 x n / 64 (n / 64: linear worst-case growth of an fp32 sum of n terms; 2: the different reduction order).
    One floor: e64 is taken as at least 2^-24 = 6e-8, the representation error an fp32 output carries whatever computed it.  Without it the gate asks
    for the impossible where the n = 64 result happens to land closer to float64 than one rounding (the single-workgroup CLIP loss measures 1.1e-8 on
    one of the inputs here); it changes nothing for an output whose n = 64 error is above one rounding.  The recorded figures: profiles/aux_rows.txt."""
    for n in NS:
        for k, e in errs[n].items():
            e64 = max(errs[64][k], FP32_FLOOR)
            print(f"AUXROWS {label} n={n} {k}: error {e:.3e}" + (f"  (e64; floored to {e64:.3e})" if n == 64 and e64 != e else "  (e64)" if n == 64 else f"  gate {2 * e64 * n / 64:.3e}"))
    for n in NS[1:]:
        for k, e in errs[n].items():
            assert e <= 2 * max(errs[64][k], FP32_FLOOR) * n / 64, (label, n, k, e, errs[64][k])


# ---------------------------------------------------------------------------------------------------------------- 1. the kernels alone
def _clip_call(entry, img, txt, ls, w):
    n = img.shape[0]
    d = dict(loss=torch.zeros(1, device="cuda"), dimg=torch.full((n, 32), 7.0, device="cuda"), dtxt=torch.full((n, 32), 7.0, device="cuda"), dls=torch.zeros(1, device="cuda"))
    a, b, s = _cu(img), _cu(txt), _cu([ls])          # kept alive over the call
    L.check(getattr(L.load(), entry)(a.data_ptr(), b.data_ptr(), n, s.data_ptr(), w, d["loss"].data_ptr(), d["dimg"].data_ptr(), d["dtxt"].data_ptr(), d["dls"].data_ptr(), None))
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("entry", ["hulc_k_clip_loss", "hulc_k_clip_loss_fp32"])
@pytest.mark.parametrize("ls", [math.log(1 / 0.07), math.log(100.0)])
def test_clip_kernel_against_float64(entry, ls):
    w, errs = 3.0, {}
    for n in NS:
        img, txt = kernel_rows(n, 100 + n)
        got = _clip_call(entry, img, txt, np.float32(ls), w)
        loss, dimg, dtxt, dls = clip_loss64(img, txt, np.float32(ls), w)
        errs[n] = dict(loss=_err(got["loss"][0], loss), dimg=_err(got["dimg"], dimg), dtxt=_err(got["dtxt"], dtxt), dlogit_scale=_err(got["dls"][0], dls))
        assert np.isfinite(got["dimg"]).all() and np.isfinite(got["dtxt"]).all()
        if n in (129, 300):          # no atomics, fixed reduction order: two runs give the same bits
            again = _clip_call(entry, img, txt, np.float32(ls), w)
            assert all(np.array_equal(got[k], again[k]) for k in got), n
    _gate_against_n64(f"{entry} logit_scale={ls:.4f}", errs)


def _mia_params(seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((512, 64)) / 8).astype(np.float32), (0.1 * rng.standard_normal(512)).astype(np.float32),
            (rng.standard_normal((1, 512)) / 16).astype(np.float32), np.array([0.05], np.float32))


def _mia_call(img, txt, prm, w, accum):
    n = img.shape[0]
    d = dict(loss=torch.zeros(1, device="cuda"), dimg=torch.full((n, 32), 0.5 if accum else 7.0, device="cuda"), dtxt=torch.full((n, 32), -0.25 if accum else 7.0, device="cuda"),
             dW0=torch.zeros(512, 64, device="cuda"), db0=torch.zeros(512, device="cuda"), dW1=torch.zeros(1, 512, device="cuda"), db1=torch.zeros(1, device="cuda"))
    p = [_cu(x) for x in prm] + [_cu(img), _cu(txt)]          # kept alive over the call
    L.check(L.load().hulc_k_mia_head(p[4].data_ptr(), p[5].data_ptr(), n, p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(), w, d["loss"].data_ptr(),
                                     d["dimg"].data_ptr(), d["dtxt"].data_ptr(), int(accum), d["dW0"].data_ptr(), d["db0"].data_ptr(), d["dW1"].data_ptr(), d["db1"].data_ptr(), None))
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_mia_kernel_against_float64():
    w, errs, prm = 1.5, {}, _mia_params(3)
    for n in NS:
        img, txt = kernel_rows(n, 200 + n)
        got = _mia_call(img, txt, prm, w, False)
        ref = dict(zip(("loss", "dimg", "dtxt", "dW0", "db0", "dW1", "db1"), mia_head64(img, txt, *prm, w)))
        errs[n] = {k: _err(got[k].reshape(-1)[0] if k in ("loss", "db1") else got[k], ref[k].reshape(-1)[0] if k in ("loss", "db1") else ref[k]) for k in ref}
        # the other roll direction pairs every txt row with another image: its dtxt is a different tensor altogether (the rolled pairs span all n rows)
        assert _err(got["dtxt"], mia_head64(img, txt, *prm, w, shift=-1)[2]) > 0.1
        acc = _mia_call(img, txt, prm, w, True)          # accum: added to what dimg / dtxt held
        assert np.abs(acc["dimg"] - (got["dimg"] + np.float32(0.5))).max() <= 1e-6 * max(1.0, np.abs(got["dimg"]).max())
        assert np.abs(acc["dtxt"] - (got["dtxt"] - np.float32(0.25))).max() <= 1e-6 * max(1.0, np.abs(got["dtxt"]).max())
        if n in (129, 300):
            again = _mia_call(img, txt, prm, w, False)
            assert all(np.array_equal(got[k], again[k]) for k in got), n
    _gate_against_n64("hulc_k_mia_head", errs)
    # loss only (validation): no gradient pointer
    img, txt = kernel_rows(130, 5)
    loss = torch.zeros(1, device="cuda")
    p = [_cu(x) for x in prm] + [_cu(img), _cu(txt)]
    L.check(L.load().hulc_k_mia_head(p[4].data_ptr(), p[5].data_ptr(), 130, p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(), 0.0, loss.data_ptr(),
                                     None, None, 0, None, None, None, None, None))
    assert abs(float(loss[0]) - mia_head64(img, txt, *prm, 1.0)[0]) <= 1e-5


def test_cosine_dist_kernel_against_float64():
    w, errs, D = 2.0, {}, 384
    for n in NS:
        rng = np.random.default_rng(300 + n)
        pred, tgt = (rng.standard_normal((n, D)) * 10.0 ** rng.uniform(-1, 1, (n, 1)) for _ in range(2))
        pred[n - 2] = tgt[n - 2] * 1.001 + 1e-4 * rng.standard_normal(D)          # a nearly parallel pair: 1 - cos cancels
        pred, tgt = pred.astype(np.float32), tgt.astype(np.float32)

        def call():
            loss, dp, a, b = torch.zeros(1, device="cuda"), torch.full((n, D), 7.0, device="cuda"), _cu(pred), _cu(tgt)
            L.check(L.load().hulc_k_cosine_dist(a.data_ptr(), b.data_ptr(), n, D, w, loss.data_ptr(), dp.data_ptr(), None))
            return loss.cpu().numpy(), dp.cpu().numpy()

        got = call()
        ref = cosine_dist64(pred, tgt, w)
        errs[n] = dict(loss=_err(got[0][0], ref[0]), dpred=_err(got[1], ref[1]))
        if n in (129, 300):
            again = call()
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    _gate_against_n64("hulc_k_cosine_dist", errs)


# ---------------------------------------------------------------------------------------------------------------- 2. fp32 step vs the reference fixture
@functools.lru_cache(maxsize=None)
def _rows_case_oracle():
    dims, P, batch, fx = load_rows_case()
    losses, G = O.training_step(P, dims, batch)
    return dims, P, batch, fx, losses, G


def test_fp32_step_matches_the_reference_on_66_flagged_rows():
    """The gates of test_gpu_parity.py::test_fp32_step_matches_oracle_and_reference: loss 1e-3 of the reference and 2e-5 of the oracle, every gradient tensor
    1e-3 (5e-3 the conv sums) of the reference's float64 gradients, the parameters after one Adam step."""
    dims, P, batch, fx, losses_o, G = _rows_case_oracle()
    rows = np.nonzero(batch["lang"]["use_for_aux"])[0]
    assert len(rows) == 66
    eng = _engine(dims, 72, 2, "fp32")
    eng.load_numpy(P)
    tot, per = run_step(eng, batch)
    ref = float(fx["loss_total"])
    print(f"[clip_rows72] total: engine {tot:.6f} reference {ref:.6f} oracle {float(losses_o['total']):.6f}; clip x beta: engine {CLIP_BETA * per['lang']['clip']:.6f} "
          f"reference {float(fx['log/train/lang_clip_loss']):.6f}")
    assert abs(tot - ref) <= 1e-3 * abs(ref), (tot, ref)
    assert abs(tot - float(losses_o["total"])) <= 2e-5 * abs(ref)
    clip_ref = float(fx["log/train/lang_clip_loss"])
    assert abs(CLIP_BETA * per["lang"]["clip"] - clip_ref) <= 1e-3 * abs(clip_ref)
    assert abs(CLIP_BETA * per["lang"]["clip"] - float(losses_o["clip"])) <= 2e-5 * abs(float(losses_o["clip"]))          # the oracle's slot holds beta x clip
    Gg = grads_np(eng)
    w64, wn64 = check_grads64(Gg, fx, label="clip_rows72")
    print(f"[clip_rows72] grads vs fp64 reference: worst {w64[0]:.2e} ({w64[1]}) conv sums {wn64[0]:.2e} ({wn64[1]})")
    eng.adam_step()
    pv = eng.views(eng.flat_params)
    for key in fx.files:
        if key.startswith("adam1/"):
            n = key[len("adam1/"):]
            flat = pv[n].detach().cpu().numpy().reshape(-1)
            got = flat if flat.size <= 4096 else flat[sample_idx(n, flat.size)]
            assert adam_close(got, fx[key], grad_entries(fx, n)), n
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 3. shapes around the tile edge vs the oracle
@pytest.mark.parametrize("kind,Bv,Bl,S,rule", [("hulc", 1, 65, 2, "all"), ("gcbc", 1, 130, 2, "mod12"), ("hulc", 2, 128, 2, "all")])
def test_rows_around_the_tile_edge_match_oracle(kind, Bv, Bl, S, rule):
    """In the manner of test_gpu_shapes.py::test_ragged_shapes_match_oracle, same gates."""
    dims = spec.ModelDims(kind=kind, max_window=32, use_clip=True)
    P = spec.init_all(dims, seed=100 + Bl, ln_jitter=True)
    batch = synthetic.make_batch(Bv, Bl, S, seed=100 + Bl, edge_frac=0.1, aux_mask="all")
    if rule == "mod12":
        batch["lang"]["use_for_aux"] = flag_rule(Bl)
    n_rows = int(batch["lang"]["use_for_aux"].sum())
    assert n_rows > 64
    losses_o, G = O.training_step(P, dims, batch)
    for dtype, tol_loss, tol_cos in (("fp32", 2e-5, 0.99999), ("bf16", 5e-3, 0.99)):
        eng = _engine(dims, max(Bv, Bl), S, dtype, num_classes=dims.mix_classes)
        eng.load_numpy(P)
        tot, per = run_step(eng, batch)
        eng.flush_grads()
        ref = float(losses_o["total"])
        Gg = grads_np(eng)
        a = np.concatenate([Gg[n].reshape(-1) for n in G]).astype(np.float64)
        b = np.concatenate([G[n].reshape(-1) for n in G]).astype(np.float64)
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        print(f"[{kind} Bl={Bl} rows={n_rows} {dtype}] total {tot:.6f} oracle {ref:.6f} cosine {cos:.6f} norm ratio {np.linalg.norm(a) / np.linalg.norm(b):.6f}")
        assert abs(tot - ref) <= tol_loss * abs(ref), (dtype, tot, ref)
        assert cos > tol_cos, (dtype, cos)
        assert abs(np.linalg.norm(a) / np.linalg.norm(b) - 1) < (1e-4 if dtype == "fp32" else 0.05)
        if dtype == "fp32":          # the aux block's own tensors, one by one (the concatenated cosine is dominated by the decoder)
            for n in G:
                if n.startswith("proj_vis_lang.") or n == "logit_scale":
                    assert rel_l2(Gg[n], G[n]) < 1e-3, (n, rel_l2(Gg[n], G[n]))
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- 4. paired pass
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_paired_pass_with_66_rows_equals_two_modality_passes(dtype):
    """Bv = Bl = 66, every lang row flagged: the aux rows are numbered from Bv in the 132-window pass.  Gates of
    test_gpu_parity.py::test_paired_pass_equals_two_modality_passes (fp32: every gradient tensor within 2e-5; bf16: losses 2e-3, gradient cosine 0.999)."""
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
    P = spec.init_all(dims, seed=66, ln_jitter=True)
    batch = synthetic.make_batch(66, 66, 2, seed=66, edge_frac=0.05, aux_mask="all")
    kw = dict(num_classes=dims.mix_classes)
    eng = _engine(dims, 66, 2, dtype, **kw)
    eng.load_numpy(P)
    rng = np.random.default_rng(1)
    for mb in batch.values():
        mb["plan_idx"] = rng.integers(0, 32, (66, 32))
    tot, per = run_step(eng, batch)
    eng.flush_grads()
    g_seq = eng.flat_grads.clone()
    eng.close()
    eng = _engine(dims, 132, 2, dtype, **kw)
    eng.load_numpy(P)
    eng.zero_grads()
    lv, ll = eng.forward_loss_pair(to_dev(batch["vis"]), to_dev(batch["lang"]), 0.5, CLIP_BETA, step=0)
    eng.backward()
    eng.flush_grads()
    torch.cuda.synchronize()
    tol = 2e-5 if dtype == "fp32" else 2e-3
    for got, sc in ((lv, "vis"), (ll, "lang")):
        for k in ("total_mod", "kl", "action", "clip"):
            print(f"   [{dtype}] {sc} {k}: pair {got[k]:.6f} single {per[sc][k]:.6f}")
            assert abs(got[k] - per[sc][k]) <= tol * max(1.0, abs(per[sc][k])), (sc, k, got[k], per[sc][k])
    g_pair = eng.flat_grads
    if dtype == "fp32":
        va, vb = eng.views(g_seq), eng.views(g_pair)
        worst = max((rel_l2(vb[n].cpu().numpy(), va[n].cpu().numpy()), n) for n in va if float(va[n].abs().max()) > 1e-7)
        print(f"   paired vs single gradients: worst {worst[0]:.2e} ({worst[1]})")
        assert worst[0] < 2e-5, worst
    else:
        cos = float((g_seq.double() @ g_pair.double()) / (g_seq.double().norm() * g_pair.double().norm()))
        assert cos > 0.999, cos
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 5. MIA and BC-Z above 64 rows
def _three_head_case(n, distinct=False):
    """hulc with the CLIP, BC-Z and MIA losses on n lang windows of 2 frames, all flagged.  Default-initialised parameters cannot tell one pairing of the rows
    from another (aux_golden_util.SCALES), so the case takes those multiples and the image gain 8 of the committed MIA fixtures, with the first image
    projection's bias moved by -(gain - 1) W mean(seq_feat[rows]) — seq_feat read from an fp32 engine, as the fixtures read it from the reference.
    The MIA loss is a MEAN over the scored pairs: over n independent rows the two roll directions differ by O(n^-1/2) of an already small interaction term
    (1e-4 of the loss at n = 130, whatever the scales), so no parameter choice separates them on random rows.  The rows therefore repeat three distinct
    windows (row i = window i mod 3): roll(+1) pairs image class c with text class c - 1 in every rolled pair, roll(-1) with c + 1, and the difference of
    the two losses no longer shrinks with n.  Seed 506 is the first of 500 .. 511 whose float64 restatement on the ORACLE's seq_feat / goal separates the
    two by more than 4 % of the loss at gain 8 (the gate asks for 1 %); the engine's own output played no part in the choice.
    distinct=True: n independent windows instead (the 16-bit test).  The gain is a cancellation that 16-bit operands resolve to their mantissa only
    (aux_golden_util.SCALES); over three repeated windows that rounding error repeats 43 times instead of averaging out, and rounding the projections'
    operands to bf16 in a float64 restatement alone puts the head-gradient cosine at 0.977 there (0.998 on independent windows) — the committed 16-bit
    cases run on independent windows too."""
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=True, use_bc_z=True, use_mia=True)
    P = spec.init_all(dims, seed=506, ln_jitter=True)
    for name, f in SCALES.items():
        P[name] = (P[name] * np.float32(f)).astype(np.float32)
    three = synthetic.make_batch(0, 3, 2, seed=506, edge_frac=0.05, aux_mask="all")["lang"]
    lang = {k: np.ascontiguousarray(v[np.arange(n) % 3]) for k, v in three.items()}
    if distinct:
        lang = synthetic.make_batch(0, n, 2, seed=506, edge_frac=0.05, aux_mask="all")["lang"]
    lang["plan_idx"] = np.random.default_rng(n).integers(0, 32, (n, 32))
    eng = _engine(dims, n, 2, "fp32")
    eng.load_numpy(P)
    eng.zero_grads()
    eng.forward_loss(to_dev(lang), True, 1.0, CLIP_BETA, step=0)
    eng.backward()
    sf = eng.get_tensor("seq_feat", n * 4096).reshape(n, 4096)
    eng.close()
    gain = 8.0
    W = P[IM0 + ".weight"].astype(np.float64)
    P[IM0 + ".bias"] = (P[IM0 + ".bias"].astype(np.float64) - (gain - 1.0) * (W @ sf.astype(np.float64).mean(0))).astype(np.float32)
    P[IM0 + ".weight"] = (P[IM0 + ".weight"] * np.float32(gain)).astype(np.float32)
    return dims, P, lang


@functools.lru_cache(maxsize=None)
def _three_head_fp32(n, distinct=False):
    """The fp32 engine on the three-head case: one lang-only step per (bc_z weight, mia weight) of [(0,0), (0,0), (1,0), (0,1), (1,1)], and a sixth with the
    BC-Z loss alone (modality and CLIP weights 0: every other gradient source is multiplied by zero)."""
    dims, P, lang = _three_head_case(n, distinct)
    eng = _engine(dims, n, 2, "fp32")
    eng.load_numpy(P)
    mb = to_dev(lang)
    runs = []
    for wb, wm, lw, cw in [(0.0, 0.0, 1.0, CLIP_BETA), (0.0, 0.0, 1.0, CLIP_BETA), (1.0, 0.0, 1.0, CLIP_BETA), (0.0, 1.0, 1.0, CLIP_BETA), (1.0, 1.0, 1.0, CLIP_BETA),
                           (1.0, 0.0, 0.0, 0.0)]:
        eng.set_aux_weights(wb, wm)
        eng.zero_grads()
        l = eng.forward_loss(mb, True, lw, cw, step=0)
        eng.backward()
        runs.append((l, grads_np(eng)))
    sf = eng.get_tensor("seq_feat", n * 4096).reshape(n, 4096)
    goal = eng.get_tensor("goal", n * 32).reshape(n, 32)
    eng.close()
    return dims, P, lang, runs, sf, goal


def _upstream_gate(name, d, ref, noise):
    gate = max(1e-4 * np.linalg.norm(ref), 10.0 * noise)
    err = np.linalg.norm(d - ref)
    print(f"   {name}: |d - ref| {err:.3e}  |ref| {np.linalg.norm(ref):.3e}  run-to-run noise of two weight-0 runs {noise:.3e}  gate {gate:.3e}")
    assert np.linalg.norm(ref) > 0, name
    assert err <= gate, (name, err, gate)


@pytest.mark.parametrize("n", [65, 130])
def test_mia_and_bcz_above_64_rows_match_torch(n):
    """Gates of test_gpu_aux_losses.py::test_mia_matches_torch_roll_direction_and_one_row and ::test_bcz_partial_mask_...: loss slots 1e-5, the heads' own
    gradients 1e-4 rel-L2 against autograd, the projections' and the upstream gradients (read off plan_recognition.fc.bias = sum_rows dL/dseq_feat and
    language_goal.ln.bias = sum_rows dL/dgoal) at max(1e-4 |ref|, 10 x the run-to-run noise of two weight-0 runs); at n = 130 the restatement rolled the
    other way must miss the engine's loss by more than 10 x 1e-3 |ref|.  The rows repeat three windows (see _three_head_case), so this shows the DIRECTION
    of the roll through the engine; a roll confined to 64-row blocks would change only the pairs at the block edges and is not what it detects — that the
    rolled pairs span all n rows is shown by test_mia_kernel_against_float64 (random rows, every output against float64)."""
    dims, P, lang, runs, sf, goal = _three_head_fp32(n)
    (l0, g0), (l0b, g0b), (lb, gb), (lm, gm), (l1, g1), (lz, gz) = runs
    noise = lambda k: float(np.linalg.norm(g0b[k].astype(np.float64) - g0[k]))
    assert l1["aux_rows"] == n
    # ---- MIA
    loss, T, sfl, gl = mia_restated(P, sf, goal, 1)
    loss.backward()
    got, ref = lm["mia"], float(loss)
    print(f"[mia n={n}] loss slot {got:.7f} torch roll(+1) {ref:.7f}")
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)) and l0["mia"] == lm["mia"] == l1["mia"]
    assert abs(ref - math.log(2.0)) > 1e-3
    if n == 130:
        minus = float(mia_restated(P, sf, goal, -1)[0])
        print(f"   roll(-1) {minus:.7f}: engine misses it by {abs(got - minus):.3e} (gate {1e-3 * abs(ref):.3e})")
        assert abs(got - minus) > 10 * 1e-3 * abs(ref)
    for name, t in T.items():
        d = (gm[name] - g0[name]).astype(np.float64)
        if name.startswith("mia_lang_discriminator."):
            e = rel_l2(d, t.grad.numpy())
            print(f"   {name}: rel-L2 {e:.2e}")
            assert e <= 1e-4, (name, e)
            assert not np.any(g0[name]), name
        else:          # the CLIP loss shares the projections: the difference of the two runs is the MIA share
            _upstream_gate(name, d.reshape(-1), t.grad.numpy().reshape(-1), noise(name))
    for key, ref_up in (("plan_recognition.fc.bias", sfl.grad.numpy().sum(0)), ("language_goal.ln.bias", gl.grad.numpy().sum(0))):
        _upstream_gate(key, (gm[key] - g0[key]).astype(np.float64), ref_up, noise(key))
    # ---- BC-Z
    loss, T, sfl = bcz_restated(P, sf, lang["lang"])
    loss.backward()
    print(f"[bcz n={n}] loss slot {lb['bc_z']:.7f} torch {float(loss):.7f}")
    assert abs(lb["bc_z"] - float(loss)) <= 1e-5 and l0["bc_z"] == lb["bc_z"] == l1["bc_z"]
    for name, t in T.items():
        e = rel_l2(gb[name], t.grad.numpy())
        print(f"   {name}: rel-L2 {e:.2e}")
        assert e <= 1e-4, (name, e)
        assert not np.any(g0[name]), name
    # The BC-Z share of d seq_feat (read off plan_recognition.fc.bias) is 1e-3 of the tensor's whole gradient here, so the difference of two fp32 steps
    # resolves it to the rounding of the WHOLE gradient (printed), not to 1e-4 of the share.  It is therefore measured without the subtraction, in the
    # step whose only gradient source is the BC-Z loss, at the unchanged gate.
    key = "plan_recognition.fc.bias"
    ref_up = sfl.grad.numpy().sum(0)
    print(f"   {key}: |whole gradient| {np.linalg.norm(g0[key]):.3e}, its fp32 resolution ~ {6e-8 * np.linalg.norm(g0[key]):.1e}; difference of two steps misses the BC-Z share by "
          f"{np.linalg.norm((gb[key] - g0[key]).astype(np.float64) - ref_up):.3e}")
    assert lz["bc_z"] == lb["bc_z"]
    _upstream_gate(key, gz[key].astype(np.float64), ref_up, 0.0)


# ---------------------------------------------------------------------------------------------------------------- 6. 16-bit engines
def _head_cosine(Gg, ref_of, names, scale):
    a = np.concatenate([Gg[n].reshape(-1).astype(np.float64) / scale if ref_of(n).size == Gg[n].size else Gg[n].reshape(-1)[sample_idx(n, Gg[n].size)].astype(np.float64) / scale
                        for n in names])
    b = np.concatenate([ref_of(n).reshape(-1).astype(np.float64) for n in names])
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_step_on_66_flagged_rows_close_to_the_reference(dtype):
    """Measures and gates of test_gpu_aux_losses.py::test_16bit_step_close_to_the_reference on clip_rows72: the step's loss within 5e-3 of the reference, the
    head tensors' gradients at cosine > 0.99 against its float64 gradients; fp16: the loss scale must cancel and stay."""
    dims, P, batch, fx = load_rows_case()
    eng = _engine(dims, 72, 2, dtype)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
    eng.load_numpy(P)
    tot, per = run_step(eng, batch)
    eng.flush_grads()
    ref = float(fx["loss_total"])
    scale = eng.scaler_state()["scale"] if dtype == "fp16" else 1.0
    Gg = grads_np(eng)
    names = [k[len("gradnorm64/"):] for k in fx.files if k.startswith("gradnorm64/") and k[len("gradnorm64/"):].startswith(HEADS)]
    cos = _head_cosine(Gg, lambda n: fx["grad64/" + n] if "grad64/" + n in fx.files else fx["gradsamp64/" + n], names, scale)
    print(f"[clip_rows72 {dtype}] total: engine {tot:.6f} reference {ref:.6f}; head-gradient cosine {cos:.5f}; loss scale {scale}")
    assert abs(tot - ref) <= 5e-3 * abs(ref), (tot, ref)
    if dtype == "fp16":
        assert scale == 256.0
    assert cos > 0.99, cos
    eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_three_head_step_on_130_rows(dtype):
    """The same two measures on a three-head case of 130 independent windows (see _three_head_case, distinct=True).  No reference fixture exists above 64
    rows for MIA / BC-Z; the fp32 engine on these same 130 windows stands in for it: loss within 5e-3, head-gradient cosine > 0.99.  The fp32 engine's heads
    are held to torch autograd at 1e-4 by test_mia_and_bcz_above_64_rows_match_torch on the repeated-window case of the same size, and the fp32 step
    to the reference fixture and the oracle by the tests above; this case itself is checked against nothing but the fp32 engine."""
    n = 130
    dims, P, lang, runs, sf, goal = _three_head_fp32(n, True)
    l32, g32 = runs[4]
    ref = l32["total_mod"] + CLIP_BETA * l32["clip"] + l32["bc_z"] + l32["mia"]
    eng = _engine(dims, n, 2, dtype)
    if dtype == "fp16":
        eng.scaler_enable(init_scale=256.0)
    eng.load_numpy(P)
    eng.zero_grads()
    l = eng.forward_loss(to_dev(lang), True, 1.0, CLIP_BETA, step=0)
    eng.backward()
    eng.flush_grads()
    tot = l["total_mod"] + CLIP_BETA * l["clip"] + l["bc_z"] + l["mia"]
    scale = eng.scaler_state()["scale"] if dtype == "fp16" else 1.0
    Gg = grads_np(eng)
    names = [k for k in g32 if k.startswith(HEADS)]
    cos = _head_cosine(Gg, lambda k: g32[k], names, scale)
    print(f"[three heads n={n} {dtype}] total: engine {tot:.6f} fp32 engine {ref:.6f}; clip {l['clip']:.6f}/{l32['clip']:.6f} bc_z {l['bc_z']:.6f}/{l32['bc_z']:.6f} "
          f"mia {l['mia']:.6f}/{l32['mia']:.6f}; head-gradient cosine {cos:.5f}; loss scale {scale}")
    assert l["aux_rows"] == n
    assert abs(tot - ref) <= 5e-3 * abs(ref), (tot, ref)
    if dtype == "fp16":
        assert scale == 256.0
    assert cos > 0.99, cos
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 7. validation
def test_validate_and_clip_gt_scores_on_66_flagged_rows():
    """val_pred_clip_loss against the oracle at the fp32 gate of test_gpu_val.py (1e-3); hulc_clip_gt_scores returns (66, m) and matches the numpy restatement
    at the gate of test_clip_groundtruth.py::test_encode_in_chunks_and_argument_errors (3e-4 of the largest score)."""
    dims, P, batch, fx = load_rows_case()
    mb = batch["lang"]
    mask = mb["use_for_aux"].astype(bool)
    rows = np.nonzero(mask)[0].astype(np.int32)
    B, S = mb["actions"].shape[:2]
    eng = _engine(dims, B, S, "fp32", num_classes=dims.mix_classes)
    eng.load_numpy(P)
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((37, 384)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=-1, keepdims=True)
    eng.clip_gt_encode(emb, 0)
    dev = {k: torch.from_numpy(np.ascontiguousarray(mb[k], np.float32)).cuda() for k in ("rgb_static", "rgb_gripper", "actions", "robot_obs", "lang")}
    dev["aux_rows"] = rows
    o = eng.validate(dev, True)
    got = eng.clip_gt_scores(0)
    eng.close()
    emb_o = O.encode(P, mb["rgb_static"], mb["rgb_gripper"])
    goal = O.goal_encode(P, mb["lang"], True)
    _, seq_feat, _ = O.plan_recognition_fwd(P, emb_o, dims.heads)
    ref = float(O.clip_loss(P, seq_feat, goal, mask)[0])
    print(f"[validate 66 rows] val_pred_clip_loss engine {o['val_pred_clip_loss']:.6f} oracle {ref:.6f}")
    assert abs(o["val_pred_clip_loss"] - ref) <= 1e-3 * abs(ref)
    _, _, want = O.clip_gt_loss(P, seq_feat[mask], O.goal_encode(P, emb, True), np.zeros(37, np.int64), np.zeros(66, np.int64))
    assert got.shape == (66, 37)
    assert np.abs(got - want).max() <= 3e-4 * np.abs(want).max(), np.abs(got - want).max()


# ---------------------------------------------------------------------------------------------------------------- 8. error paths, n <= 64 untouched
def test_more_rows_than_windows_is_an_error_and_64_rows_take_the_single_workgroup_kernel():
    dims = spec.ModelDims(kind="hulc", max_window=32, use_clip=True)
    P = spec.init_all(dims, seed=64, ln_jitter=True)
    lang = synthetic.make_batch(0, 64, 2, seed=64, edge_frac=0.05, aux_mask="all")["lang"]
    lang["plan_idx"] = np.random.default_rng(64).integers(0, 32, (64, 32))
    eng = _engine(dims, 64, 2, "fp32")          # max_batch = 64: no workspace of the > 64-row kernels
    eng.load_numpy(P)
    mb = to_dev(lang)
    eng.zero_grads()
    l = eng.forward_loss(mb, True, 1.0, CLIP_BETA, step=0)
    dls_fwd = eng.views(eng.flat_grads)["logit_scale"].detach().cpu().numpy().reshape(-1).copy()          # the CLIP kernel adds d logit_scale in the forward
    eng.backward()
    g = eng.flat_grads.clone()
    img = eng.get_tensor("clip_img", 64 * 32).reshape(64, 32)
    txt = eng.get_tensor("clip_txt", 64 * 32).reshape(64, 32)
    k = _clip_call("hulc_k_clip_loss_fp32", img, txt, np.float32(P["logit_scale"]), CLIP_BETA)
    assert np.float32(l["clip"]).tobytes() == k["loss"][0].tobytes(), (l["clip"], k["loss"][0])          # the same kernel on the same inputs: the same bits
    assert dls_fwd.tobytes() == k["dls"].tobytes(), (dls_fwd, k["dls"])                                   # and of d logit_scale (dimg / dtxt are not exposed by the engine)
    # more flagged rows than windows: an error, and the gradients accumulated so far stay as they are
    bad = dict(mb, aux_rows=np.arange(65, dtype=np.int32))
    with pytest.raises(RuntimeError, match="aux rows n=65 unsupported"):
        eng.forward_loss(bad, True, 1.0, CLIP_BETA, step=0)
    assert torch.equal(eng.flat_grads, g)
    with pytest.raises(RuntimeError):
        eng.backward()                                   # no forward kept
    with pytest.raises(RuntimeError, match="aux rows n=65 unsupported"):
        eng.validate(dict(bad), True)
    # the context still works, and computes what it computed before
    eng.zero_grads()
    l2 = eng.forward_loss(mb, True, 1.0, CLIP_BETA, step=0)
    eng.backward()
    assert l2["clip"] == l["clip"] and l2["action"] == l["action"]
    eng.close()
    # the MIA route at 64 rows: the engine's loss slot and the kernel entry's, on the engine's own projections, bit for bit
    d3 = spec.ModelDims(kind="hulc", max_window=32, use_clip=True, use_mia=True)
    P3 = spec.init_all(d3, seed=64, ln_jitter=True)
    e3 = _engine(d3, 64, 2, "fp32")
    e3.load_numpy(P3)
    e3.zero_grads()
    l3 = e3.forward_loss(mb, True, 1.0, CLIP_BETA, step=0)
    e3.backward()
    img, txt = e3.get_tensor("clip_img", 64 * 32).reshape(64, 32), e3.get_tensor("clip_txt", 64 * 32).reshape(64, 32)
    e3.close()
    prm = [P3[f"mia_lang_discriminator.mlp.{i}.{k}"] for i in (0, 3) for k in ("weight", "bias")]
    km = _mia_call(img, txt, prm, 1.0, False)
    assert np.float32(l3["mia"]).tobytes() == km["loss"][0].tobytes(), (l3["mia"], km["loss"][0])
