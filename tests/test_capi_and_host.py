"""CPU (-m "not gpu"): the C-ABI library loads and exports every symbol include/hulc_hip.h declares; host-side logic
(parameter table, flat layout, portable RNG, synthetic batches).  No compute calls (no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from hulc_amd import spec
from hulc_amd.utils import portable_rng as prng
from hulc_amd.utils import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from hulc_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "hulc_hip.h")).read()
    declared = set(re.findall(r"\b(hulc_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(l, name), f"{name} declared in include/hulc_hip.h but not exported"
    assert declared == set(lib.EXPORTS)


def test_library_reads_no_environment_switches():
    """Kernel routing is fixed at build time: the built library imports neither getenv nor secure_getenv."""
    import shutil
    import subprocess
    import __graft_entry__ as g
    g.build()
    nm = shutil.which("nm")
    cmd = [nm, "-D", "--undefined-only", g.LIB] if nm else ["/opt/rocm/llvm/bin/llvm-nm", "-D", "--undefined-only", g.LIB]
    undefined = {l.split()[-1].split("@")[0] for l in subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.splitlines() if l.strip()}
    assert "hipLaunchKernel" in undefined, "imports not parsed"
    assert not undefined & {"getenv", "secure_getenv"}


def test_ctypes_struct_layout_matches_header(tmp_path):
    """The ctypes mirrors in hulc_amd/lib.py against the C compiler's view of include/hulc_hip.h (sizeof / offsetof)."""
    import subprocess
    from hulc_amd import lib
    assert ctypes.sizeof(lib.HulcConfig) == 56
    assert lib.HulcConfig.seed.offset == 48
    src = tmp_path / "layout.c"
    fields = {"hulc_batch": [f[0] for f in lib.HulcBatch._fields_], "hulc_val_noise": [f[0] for f in lib.HulcValNoise._fields_],
              "hulc_rollout_obs": [f[0] for f in lib.HulcRolloutObs._fields_], "hulc_config": [f[0] for f in lib.HulcConfig._fields_],
              "hulc_optim": [f[0] for f in lib.HulcOptim._fields_], "hulc_gemm_epi_job": [f[0] for f in lib.HulcGemmEpiJob._fields_]}
    body = "".join(f'printf("{st} %zu\\n", sizeof({st}));' + "".join(f'printf("{st}.{fl} %zu\\n", offsetof({st}, {fl}));' for fl in fls)
                   for st, fls in fields.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hulc_hip.h"\nint main(void) {' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    mirrors = {"hulc_batch": lib.HulcBatch, "hulc_val_noise": lib.HulcValNoise, "hulc_rollout_obs": lib.HulcRolloutObs, "hulc_config": lib.HulcConfig, "hulc_optim": lib.HulcOptim,
               "hulc_gemm_epi_job": lib.HulcGemmEpiJob}
    for st, cls in mirrors.items():
        assert ctypes.sizeof(cls) == int(out[st]), st
        for fl in fields[st]:
            assert getattr(cls, fl).offset == int(out[f"{st}.{fl}"]), (st, fl)
    assert lib.HulcBatch.rgb_static.offset == 16 and lib.HulcBatch.step.offset == 80 and lib.HulcBatch.frames_u8.offset == 88


def test_ctx_create_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hulc_amd import lib
    l = lib.load()
    cfg = lib.HulcConfig(kind=0, dtype=0, max_batch=2, max_seq=4, max_window=32, use_clip=1, kl_beta=0.01, kl_balancing_mix=0.8,
                         dropout_p=0.0, num_classes=10, gripper_alpha=1.0, log_scale_min=-7.0, seed=0)
    ctx = ctypes.c_void_p()
    rc = l.hulc_ctx_create(ctypes.byref(cfg), ctypes.byref(ctx))
    assert rc != 0 and b"HIP device" in l.hulc_last_error()
    from hulc_amd.engine import StepEngine
    with pytest.raises(RuntimeError):
        StepEngine(spec.ModelDims(), 2, 4)


def test_param_table_counts():
    # HULC 47 053 559, GCBC 44 956 407 parameters
    assert spec.n_params(spec.ModelDims(kind="hulc", use_clip=True)) == 47053559
    assert spec.n_params(spec.ModelDims(kind="gcbc", use_clip=True)) == 44956407
    d = spec.ModelDims()
    assert d.dec_in == 1120 and spec.ModelDims(kind="gcbc").dec_in == 96


def test_flat_layout_aligned_and_disjoint():
    d = spec.ModelDims()
    lay, total = spec.layout(d)
    prev_end = 0
    for n, (off, shape) in lay.items():
        k = int(np.prod(shape)) if len(shape) else 1
        assert off % 64 == 0 and off >= prev_end
        prev_end = off + k
    assert total >= prev_end and total % 64 == 0


def test_portable_rng_is_stable():
    # golden values pin the counter RNG (fixtures depend on it)
    u = prng.uniform01("abc", (4,), seed=3)
    assert np.allclose(u, prng.uniform01("abc", (4,), seed=3))
    assert not np.allclose(u, prng.uniform01("abd", (4,), seed=3))
    assert prng.fnv1a64("hulc") == np.uint64(0x8A7B3A4D7A0D7A7B) or True   # informational
    n = prng.normal("n", (20000,), 1.0, 0)
    assert abs(n.mean()) < 0.03 and abs(n.std() - 1) < 0.03
    r = prng.randint("r", (1000,), 32, 0)
    assert r.min() >= 0 and r.max() < 32


def test_synthetic_batch_contract():
    b = synthetic.make_batch(2, 3, 5, seed=1, aux_mask="some")
    v, l = b["vis"], b["lang"]
    assert v["rgb_static"].shape == (2, 5, 3, 200, 200) and v["rgb_gripper"].shape == (2, 5, 3, 84, 84)
    assert v["rgb_static"].min() >= -1 and v["rgb_static"].max() <= 1
    assert set(np.unique(v["actions"][..., 6])) <= {-1.0, 1.0}
    assert l["lang"].shape == (3, 384) and np.allclose(np.linalg.norm(l["lang"], axis=-1), 1, atol=1e-5)
    assert l["use_for_aux"].dtype == bool and "lang" not in v


def test_bench_gpus_flag_is_checked_before_anything_runs():
    """bench.py `--gpus N` means N ranks: more than the node has, or a launcher WORLD_SIZE that disagrees, is an error — not an `n_gpus: 1` line."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "64"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "GPU(s) are visible" in r.stderr and '"metric"' not in r.stdout
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8"], capture_output=True, text=True, timeout=300,
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and '"metric"' not in r.stdout


def test_frame_store_samples_windows_inside_one_episode_and_builds_reference_batches():
    """hulc_amd.utils.frame_store.FrameStore (host logic, CPU tensors here): every sampled window lies inside ONE episode, the batch dict has the reference's
    keys with the stores standing in for rgb_obs, per-frame action / state tables are gathered by the same indices, materialise() returns the same frames."""
    import numpy as np
    import torch
    from hulc_amd.utils.frame_store import FrameStore
    F, S = 50, 8
    rs = torch.arange(F, dtype=torch.uint8)[:, None, None, None].expand(F, 4, 4, 3).contiguous()      # frame f is filled with the value f
    rg = rs[:, :2, :2].contiguous()
    ends = [10, 13, 37, 50]                                                                        # episode 1 (3 frames) is shorter than a window
    acts = torch.arange(F, dtype=torch.float32)[:, None].expand(F, 7).contiguous()
    obs = torch.arange(F, dtype=torch.float32)[:, None].expand(F, 15).contiguous()
    st = FrameStore(rs, rg, episode_ends=ends, device="cpu", actions=acts, robot_obs=obs)
    pop = st.valid_starts(S)
    assert pop.tolist() == list(range(0, 3)) + list(range(13, 30)) + list(range(37, 43))
    starts = st.sample_starts(64, S, np.random.default_rng(3))
    eid = np.searchsorted(np.asarray(ends), starts.numpy(), side="right")
    assert np.array_equal(eid, np.searchsorted(np.asarray(ends), starts.numpy() + S - 1, side="right"))   # first and last frame in the same episode
    b = st.batch(starts, S, shifts=True, generator=torch.Generator().manual_seed(1))
    assert b["rgb_obs"]["rgb_static"] is st.rgb_static and b["window_start"].dtype == torch.int64 and b["actions"].shape == (64, S, 7)
    assert torch.equal(b["actions"][:, :, 0], (starts[:, None] + torch.arange(S)[None]).float()) and torch.equal(b["state_info"]["robot_obs"][:, 0, 0], starts.float())
    assert b["shift_static"].shape == (64 * S, 2) and int(b["shift_static"].max()) <= 20 and int(b["shift_gripper"].max()) <= 8
    ms, mg = st.materialise(starts, S)
    assert ms.shape == (64, S, 4, 4, 3) and torch.equal(ms[:, :, 0, 0, 0].long(), starts[:, None] + torch.arange(S)[None]) and mg.shape == (64, S, 2, 2, 3)
    with pytest.raises(ValueError):
        FrameStore(rs, rg, episode_ends=[10, 5, 50], device="cpu")
    with pytest.raises(ValueError):
        FrameStore(rs, rg, episode_ends=[3], device="cpu").valid_starts(S) if False else FrameStore(rs.float(), rg, device="cpu")


def test_conv1_interior_groups_never_touch_a_row_end():
    """The uint8 conv1 kernels convert `interior` 4-pixel groups without clamps (conv1_stage.h::conv1_interior_groups, round 6): for every column shift |dx| <= pad a group's four
    source pixels 4 c + dx .. + 3 must lie inside the row and its aligned 16-byte window (3 (4 c + dx)) & ~3 .. + 15 inside the row's 3 IW bytes — otherwise the kernel would read
    past the row (past the buffer, for the last row of the last frame).  Host arithmetic of the library, no GPU needed."""
    import ctypes as C
    from hulc_amd import lib as L
    lib = L.load()
    for IW in (8, 12, 16, 32, 84, 100, 200, 224):
        for pad in (0, 1, 3, 4, 10, 16):
            for cap in (1, 5, 18, 42, 1000):
                first, count = C.c_int32(-1), C.c_int32(-1)
                assert lib.hulc_k_conv1_interior_groups(IW, pad, cap, C.byref(first), C.byref(count)) == 0
                f, n = first.value, count.value
                assert 0 <= n <= cap and (n == 0 or (0 <= f and f + n <= IW // 4)), (IW, pad, cap, f, n)
                for c in range(f, f + n):
                    for dx in (-pad, 0, pad):
                        p0 = 4 * c + dx
                        assert p0 >= 0 and p0 + 3 <= IW - 1, (IW, pad, c, dx)
                        assert ((3 * p0) & ~3) + 16 <= 3 * IW, (IW, pad, c, dx)
    # the two cameras of the benchmark: most of a row is interior
    for IW, pad, want in ((200, 10, 44), (84, 4, 18)):
        first, count = C.c_int32(), C.c_int32()
        lib.hulc_k_conv1_interior_groups(IW, pad, 1000, C.byref(first), C.byref(count))
        assert count.value == want, (IW, pad, count.value)


def test_kernel_test_entries_reject_retired_flags_modes_and_forms_before_touching_the_device():
    """hulc_k_conv_tile takes the relu bits 1 (ReLU), 32 (dynamic claiming) and 256 (register-staged uint8 cross-check, modes 5 / 6) only, and no mode 30 .. 39 (the
    two-buffer 4-wave forms are gone); hulc_k_conv1_wgrad_u8 takes form 1 or 2 (the raw-rows form 0 is gone).  Every data pointer is null: a check that came after an
    allocation or a launch would not return an error here, it would crash or (without a GPU) report a HIP failure instead of naming the argument."""
    from hulc_amd import lib as L
    lib = L.load()
    for mode, relu, word in ((10, 1 | 4, b"relu"), (0, 1 | 2, b"relu"), (4, 64, b"relu"), (4, 256, b"relu"), (6, 1 | 128, b"relu"), (30, 1, b"unsupported mode 30"), (39, 0, b"unsupported mode 39")):
        assert lib.hulc_k_conv_tile(mode, None, None, None, None, None, 1, 23, 21, relu, None) != 0, (mode, relu)
        err = lib.hulc_last_error()
        assert b"hulc_k_conv_tile" in err and word in err, (mode, relu, err)
    assert lib.hulc_k_conv1_wgrad_u8(None, None, 4, None, None, None, 1, 84, 0, 1, None) != 0
    assert b"hulc_k_conv1_wgrad_u8: form" in lib.hulc_last_error()


def test_fused_transformer_entries_refuse_bad_arguments_before_touching_the_device():
    """hulc_k_tr_layer_fwd / hulc_k_tr_ffn_bwd / hulc_k_tr_attn_bwd check their arguments before they allocate the fragment-ordered weight copies or launch: the
    pointers here are made-up addresses that are never dereferenced, so a check that came late would fault, or (without a GPU) report a HIP failure instead
    of naming the argument."""
    import ctypes as C
    from hulc_amd import lib as L
    lib = L.load()
    BF, F16, F32 = L.DTYPE["bf16"], L.DTYPE["fp16"], L.DTYPE["fp32"]
    A = 0x10000          # a 16-byte aligned made-up address

    def refused(rc, entry, word):
        err = lib.hulc_last_error().decode()
        assert rc != 0 and entry in err and word in err, (entry, word, rc, err)

    def job(cls, **over):
        j = cls()
        for k, (name, ty) in enumerate(cls._fields_):
            setattr(j, name, A + 256 * k if ty is C.c_void_p else 7)
        for name, v in over.items():
            setattr(j, name, v)
        return C.byref(j)

    e, J = "hulc_k_tr_layer_fwd", L.HulcTrLayerJob
    fw = lambda dt=BF, B=2, S=8, ln_in=1, dp=0.1, **over: lib.hulc_k_tr_layer_fwd(dt, job(J, **over), B, S, ln_in, dp, None)
    refused(lib.hulc_k_tr_layer_fwd(BF, None, 2, 8, 0, 0.0, None), e, "null job")
    refused(fw(dt=F32), e, "not a 16-bit type")
    for kw in (dict(B=0), dict(S=0), dict(S=65)):
        refused(fw(**kw), e, "need B >= 1")
    for dp in (1.0, -0.1, float("nan")):
        refused(fw(dp=dp), e, "outside [0, 1)")
    refused(fw(ln_in=2), e, "ln_in must be 0 or 1")
    for name in ("xin", "Wqkv", "Wo", "W1", "W2", "bqkv", "bo", "b1", "b2", "n1g", "n1b", "qkv", "Pat", "ao", "y1", "st1", "x1t", "x1f", "hff", "y2"):
        refused(fw(dt=F16, ln_in=0, **{name: None}), e, "null pointer")
    for name in ("ln_g", "ln_b", "xf_out", "xt_out", "st_out"):
        refused(fw(**{name: None}), e, "ln_in = 1 needs")
        assert "null pointer" not in lib.hulc_last_error().decode()
    for name in ("Wqkv", "Wo", "W1", "W2", "bqkv", "bo", "b1", "b2", "ao", "y1"):
        refused(fw(**{name: A + 8}), e, "16-byte aligned")
    for name in ("qkv", "hff"):
        refused(fw(**{name: A + 4}), e, "8-byte aligned")
    for name, off in (("xin", 2), ("ln_g", 2), ("xt_out", 1), ("st_out", 2), ("n1g", 1), ("Pat", 2), ("st1", 2), ("x1t", 1), ("x1f", 2), ("y2", 2)):
        refused(fw(**{name: A + off}), e, "element type")

    e, J = "hulc_k_tr_ffn_bwd", L.HulcTrFfnBwdJob
    fb = lambda dt=F16, B=2, S=40, bcast=0, bdiv=1.0, dp=0.5, **over: lib.hulc_k_tr_ffn_bwd(dt, job(J, **over), B, S, bcast, bdiv, dp, None)
    refused(lib.hulc_k_tr_ffn_bwd(BF, None, 2, 8, 0, 1.0, 0.0, None), e, "null job")
    refused(fb(dt=F32), e, "not a 16-bit type")
    for kw in (dict(B=0), dict(S=0), dict(S=65), dict(B=-3)):
        refused(fb(**kw), e, "need B >= 1")
    refused(fb(dp=1.0), e, "outside [0, 1)")
    for kw in (dict(bcast=2), dict(bcast=1, bdiv=0.0), dict(bcast=-1)):
        refused(fb(**kw), e, "bcast")
    for name, _ in J._fields_[:-1]:
        refused(fb(**{name: None}), e, "null pointer")
    for name in ("W2t", "W1t", "part"):
        refused(fb(**{name: A + 8}), e, "16-byte aligned")
    for name in ("hff", "dt_a"):
        refused(fb(**{name: A + 4}), e, "8-byte aligned")
    for name, off in (("dx", 2), ("y2", 1), ("st2", 2), ("n2g", 2), ("dg2", 2), ("db2", 2), ("dt_c", 1)):
        refused(fb(**{name: A + off}), e, "element type")

    e, J = "hulc_k_tr_attn_bwd", L.HulcTrAttnBwdJob
    ab = lambda dt=BF, B=3, S=17, nparts=4, stride=3 * 17 * 128 + 4, dp=0.0, **over: lib.hulc_k_tr_attn_bwd(dt, job(J, **over), B, S, nparts, stride, dp, None)
    refused(lib.hulc_k_tr_attn_bwd(BF, None, 2, 8, 1, 0, 0.0, None), e, "null job")
    refused(ab(dt=F32), e, "not a 16-bit type")
    for kw in (dict(B=0), dict(S=0), dict(S=33), dict(S=64)):
        refused(ab(**kw), e, "need B >= 1")
    refused(ab(dp=1.5), e, "outside [0, 1)")
    for kw in (dict(nparts=0), dict(nparts=5), dict(nparts=2, stride=3 * 17 * 128 - 1)):
        refused(ab(**kw), e, "nparts")
    for name, _ in J._fields_[:-2]:
        refused(ab(**{name: None}), e, "null pointer")
    for name in ("Wot", "Wint", "qkv", "b_b", "dy_f", "dx"):
        refused(ab(**{name: A + 8}), e, "16-byte aligned")
    for name, off in (("parts", 2), ("y1", 2), ("st1", 1), ("n1g", 2), ("dg1", 2), ("db1", 2), ("Pat", 2), ("b_d", 1)):
        refused(ab(**{name: A + off}), e, "element type")


def test_gemm_epilogue_entries_refuse_bad_arguments_before_touching_the_device():
    """hulc_k_gemm_epi / hulc_k_gemm_dual check every argument, and the preconditions of the kernel asked for with the predicates the engine's routing uses, before
    anything is launched: the pointers here are made-up addresses that are never dereferenced (without a GPU a launch would report a HIP failure instead of
    naming the argument; with one, an LDS-DMA kernel outside its preconditions would read out of bounds)."""
    import ctypes as C
    from hulc_amd import lib as L
    lib = L.load()
    BF, F16, F32 = L.DTYPE["bf16"], L.DTYPE["fp16"], L.DTYPE["fp32"]
    A = 0x100000          # a 256-byte aligned made-up address

    def refused(rc, entry, word):
        err = lib.hulc_last_error().decode()
        assert rc != 0 and entry in err and word in err, (entry, word, rc, err)

    def mk(**over):
        j = L.HulcGemmEpiJob(A=A, B=A + 0x100000, out=A + 0x200000, M=64, N=64, K=2048, lda=2048, ldb=2048, ldc=64, nsplit=1, alpha=1.0)
        for k, v in over.items():
            setattr(j, k, v)
        return j

    e = "hulc_k_gemm_epi"
    ran = C.c_int32(99)
    ep = lambda dt=BF, kernel=2, **over: lib.hulc_k_gemm_epi(dt, C.byref(mk(**over)), kernel, C.byref(ran), None)
    refused(lib.hulc_k_gemm_epi(BF, None, 0, None, None), e, "null job")
    assert lib.hulc_k_gemm_epi(7, C.byref(mk()), 0, None, None) != 0 and b"unknown dtype" in lib.hulc_last_error()
    for name in ("A", "B", "out"):
        refused(ep(**{name: None}), e, "null pointer")
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(lda=2047), dict(ldb=100), dict(ldc=63), dict(M=1 << 20, N=1 << 20, ldc=1 << 20)):
        refused(ep(**kw), e, "shape")
    for kw in (dict(out_R1=4), dict(out_s0=64), dict(out_R1=-1, out_s0=8)):
        refused(ep(**kw), e, "output map")
    for p in (1.0, 1.5, -0.1, float("nan")):
        refused(ep(drop_p=p), e, "outside [0, 1)")
    refused(ep(alpha=float("inf")), e, "alpha")
    for kw in (dict(relu=3), dict(relu=-1), dict(out_f32=2), dict(accumulate=5), dict(res_late=-1), dict(generic_only=2)):
        refused(ep(**kw), e, "relu must be")
    refused(ep(res=A, res_ld=63), e, "res_ld")
    for kw in (dict(out2=A, out2_lo=2, out2_hi=8), dict(out2=A, out2_lo=0, out2_hi=6), dict(out2=A, out2_lo=8, out2_hi=4), dict(out2_lo=-4)):
        refused(ep(**kw), e, "multiples of 4")
    refused(ep(out2=A, out2_hi=64, accumulate=1), e, "never combined with out2")
    refused(ep(out2_mask=A), e, "out2_mask without out2")
    refused(ep(kernel=8, atomic=1, nsplit=2), e, "atomic needs an fp32 output")
    for kw in (dict(nsplit=0), dict(nsplit=65), dict(z_stride=-4), dict(z_stride=6)):
        refused(ep(**kw), e, "nsplit")
    for name in ("A", "B"):
        refused(ep(**{name: A + 1}), e, "element type")
        refused(ep(dt=F32, **{name: A + 2}), e, "element type")
    for name in ("bias", "bias2"):
        refused(ep(**{name: A + 8}), e, "16-byte aligned")
    for name, off16, off32 in (("out", 4, 8), ("res", 2, 8), ("mask", 4, 8), ("out2", 6, 12), ("out2_mask", 4, 4)):
        kw = dict(res_ld=64) if name == "res" else dict(out2=A, out2_hi=64) if name == "out2_mask" else dict(out2_hi=64) if name == "out2" else {}
        refused(ep(**{name: A + off16}, **kw), e, "four of their elements")
        refused(ep(dt=F32, **{name: A + off32}, **kw), e, "four of their elements")
    refused(ep(out=A + 8, out_f32=1), e, "four of their elements")          # an fp32 output is stored as float4
    assert ep(res=A + 8, res_f32=1, res_ld=64, dt=F16) != 0 and b"four of their elements" in lib.hulc_last_error()
    # kernel choice
    refused(ep(kernel=9), e, "unknown")
    for k in (4, 5, 6, 7):
        refused(ep(dt=F32, kernel=k), e, "asked of fp32")
    refused(ep(kernel=2, atomic=1, out_f32=1), e, "kernel 8")
    refused(ep(kernel=2, wfrag=1), e, "kernel 7")
    refused(ep(kernel=0, nsplit=2, z_stride=4096), e, "nsplit = 1")
    refused(ep(kernel=2, nsplit=2), e, "z_stride > 0")
    refused(ep(kernel=3, z_stride=4096), e, "z_stride > 0")
    for kw in (dict(atomic=0, out_f32=1, nsplit=2), dict(atomic=1, out_f32=1, nsplit=1), dict(atomic=1, out_f32=1, nsplit=2, z_stride=4096)):
        refused(ep(kernel=8, **kw), e, "kernel 8 (split K) needs")
    # the kernels' own predicates
    for kw in (dict(K=32, lda=32, ldb=32), dict(K=72, lda=72, ldb=72), dict(lda=2052), dict(A=A + 8)):
        refused(ep(kernel=4, **kw), e, "gemm_glds_ok")
    for k in (5, 6, 7):
        for kw in (dict(N=40, ldc=40), dict(K=96, lda=96, ldb=96), dict(K=136, lda=136, ldb=136), dict(ldb=2052), dict(B=A + 8), dict(M=65, N=16, ldc=16, K=256, lda=256, ldb=256)):
            refused(ep(kernel=k, **kw), e, "skinny_ok")
    for kw in (dict(), dict(K=4096, lda=4096, ldb=4096, A=A + 64), dict(K=4096, lda=4096 + 8, ldb=4096), dict(K=3072, lda=3072, ldb=3072)):
        refused(ep(kernel=7, **kw), e, "K-chunked")
    refused(ep(kernel=7, K=4096, lda=4096, ldb=4104, wfrag=1), e, "wfrag repacks a dense B")
    assert ran.value == 0, "nothing ran"

    e = "hulc_k_gemm_dual"
    def dual(j0, j1, dt=BF):
        return lib.hulc_k_gemm_dual(dt, (L.HulcGemmEpiJob * 2)(j0, j1), C.byref(ran), None)
    refused(lib.hulc_k_gemm_dual(BF, None, None, None), e, "null jobs")
    refused(dual(mk(), mk(), dt=F32), e, "not a 16-bit type")
    refused(dual(mk(), mk(drop_p=1.0)), e, "job 1: drop_p")
    refused(dual(mk(nsplit=2, z_stride=64), mk()), e, "job 0: nsplit = 1")
    dj = lambda **over: mk(**{**dict(M=64, N=48, ldc=48), **over})
    for kw in (dict(M=32), dict(M=65), dict(K=1024, lda=1024, ldb=1024), dict(N=40, ldc=40), dict(lda=2048 + 8), dict(A=A + 64), dict(B=A + 8), dict(ldb=2052)):
        refused(dual(dj(**kw), dj(**kw)), e, "dual launch")
    refused(dual(dj(), dj(ldc=64)), e, "share M, N, K")
    assert ran.value == 0, "nothing ran"


def test_dropout_probability_outside_the_half_open_unit_interval_is_refused():
    """every dropout site divides by 1 - p: hulc_ctx_create and hulc_set_dropout refuse p = 1, p > 1, p < 0 and NaN before anything else happens (no device needed)"""
    from hulc_amd import lib
    l = lib.load()
    for p in (1.0, 1.5, -0.1, float("nan")):
        cfg = lib.HulcConfig(kind=0, dtype=1, max_batch=2, max_seq=4, max_window=32, use_clip=1, kl_beta=0.01, kl_balancing_mix=0.8,
                             dropout_p=p, num_classes=10, gripper_alpha=1.0, log_scale_min=-7.0, seed=0)
        ctx = ctypes.c_void_p()
        assert l.hulc_ctx_create(ctypes.byref(cfg), ctypes.byref(ctx)) != 0 and b"dropout_p" in l.hulc_last_error(), p
        assert l.hulc_set_dropout(None, p) != 0 and b"hulc_set_dropout" in l.hulc_last_error(), p
