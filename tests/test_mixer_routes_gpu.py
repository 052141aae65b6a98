"""Launch-trace table of the Mamba mixer's host path (dimsum_amd/ops/selective_scan_interface.py: _MambaInner behind the four
mamba_inner_fn* wrappers, _BiMambaInner behind bimamba_inner_fn): for every route the host code can take, WHICH library entry points
go out, in which order, with which flags and with operands of which (shape, stride, dtype) -- at the smallest shape every route accepts
(batch 1, L 256, d_inner 128, d_model 256, dstate 16, dt_rank 4, d_conv 4, float32, DIMSUM_SPLIT3_MIN_ROWS=256; the scaled-fp16 training
carrier wants d_inner % 256 == 0 and runs at d_inner 256). Unforced, this launch runs on a state-split scan kernel; the cases of the
64-channel kernel force it with native.scan_fwd_variant(1), for which the library's query returns 1 at this batch.

A pass-through spy (the style of _LaunchSpy in test_model_gpu.py) sits on the attributes of `native` and `gemm` the mixer calls through.
Per case the ordered trace is asserted twice: name and flags against EXPECT below (the readable table), and name, flags and every tensor
argument's (shape, stride, dtype) against tests/golden/mixer_routes_trace.json (one line per launch; running this file as a script on the GPU
records it anew after an intended route change). The result of every case is
also checked against a float64 composition of the same steps in plain torch on the CPU (conv, x_proj, dt_proj, the recurrence, the gate,
out_proj; autograd for the gradients), at the bounds the existing mixer tests use: exact fp32 2e-4 |ref| + 2e-5 max|ref| for the output,
5e-4 / 5e-5 for dxz, 1e-3 / 2e-4 for parameter gradients (test_mamba_inner_fn_fwd_bwd_gpu); 5 x the first two under allow_tf32
(test_bimamba_gpu.py::test_golden); 1e-3 / 1e-3 under policy "f16s" (the block tests of test_model_gpu.py / test_f16s_train_gpu.py);
3e-2 / 5e-2 under bf16 autocast (test_half_dtypes_vs_fp32_oracle)."""
import contextlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, assert_close

pytestmark = pytest.mark.gpu

NATIVE = ("causal_conv1d_fwd", "causal_conv1d_fwd_cond", "causal_conv1d_bwd", "selective_scan_fwd", "selective_scan_bwd",
          "selective_scan_general_fwd", "selective_scan_general_bwd", "selective_scan_bidir_fwd", "selective_scan_bidir_bwd",
          "rows_block_f16s", "rows_f16s", "gemm_tn", "gemm_nt", "gemm_nn")
GEMM = ("linear", "mm_nn_rows", "mm_nt_rows")
RECOMPUTE_AT = {"selective_scan_bwd": 13, "selective_scan_bidir_bwd": 15}       # recompute_out_z is passed by position
ENV = ("DIMSUM_SCAN_DT_PROJ", "DIMSUM_XDBL_T_TRAIN", "DIMSUM_SCAN_INFER_STORES", "DIMSUM_RECOMPUTE_OUT_Z", "DIMSUM_MAMBA_CHECKPOINT_LVL",
       "DIMSUM_OUT_PROJ_PLANES", "DIMSUM_OUT_PROJ_F16", "DIMSUM_SPLIT3", "DIMSUM_SPLIT3_MIN_ROWS", "DIMSUM_GEMM_NT", "DIMSUM_SPLIT3_TRAIN",
       "DIMSUM_F16S_TRAIN")


def _sig(v):
    if isinstance(v, torch.Tensor):
        return [list(v.shape), list(v.stride()), str(v.dtype).replace("torch.", "")]
    if isinstance(v, (tuple, list)):
        return [_sig(t) for t in v]
    return v if v is None or isinstance(v, (bool, int, float, str)) else type(v).__name__


def _flag(k, v):
    if isinstance(v, bool):
        return f"{k}={int(v)}"
    if isinstance(v, int):
        return f"{k}={v}"
    if isinstance(v, (tuple, list)):
        return f"{k}[rank{v[0].dim()}]"
    return k


class _Spy:
    """pass-through recorders: one [name + flags, argument signatures] entry per call, in call order"""

    def __init__(self, monkeypatch):
        from dimsum_amd import gemm, native
        self.trace = []
        for mod, prefix, names in ((native, "", NATIVE), (gemm, "gemm.", GEMM)):
            for name in names:
                monkeypatch.setattr(mod, name, self._wrap(prefix + name, getattr(mod, name)))

    def _wrap(self, name, real):
        def spy(*a, **kw):
            flags = [_flag(k, kw[k]) for k in sorted(kw) if kw[k] is not None]
            if name in RECOMPUTE_AT:
                flags.append(f"recompute_out_z={int(bool(a[RECOMPUTE_AT[name]]))}")
            self.trace.append([" ".join([name] + flags), [_sig(v) for v in a] + [[k, _sig(kw[k])] for k in sorted(kw)]])
            return real(*a, **kw)
        return spy


def _case(fn="plain", policy="default", tf32=True, env=None, variant=0, grad=False, out_bias=False, last_state=False, conv_done=False, init=None,
          B_bias=False, C_bias=False, N=16, d_inner=128, force_general=False, autocast=False):
    return dict(locals())


K1 = dict(variant=1)       # the 64-channel scan kernel, forced
CASES = {
    # ---- inference (torch.no_grad) ----
    "inf_default_split": _case(),
    "inf_default_k1": _case(**K1),
    "inf_default_k1_planes_always": _case(**K1, env={"DIMSUM_OUT_PROJ_PLANES": "1"}),
    "inf_default_k1_no_dt_fusion": _case(**K1, env={"DIMSUM_SCAN_DT_PROJ": "0"}),
    "inf_f16s_k1": _case(**K1, policy="f16s"),
    "inf_f16s_split": _case(policy="f16s", variant=4),
    "inf_f16s_split_f16_off": _case(policy="f16s", variant=4, env={"DIMSUM_OUT_PROJ_F16": "0"}),
    "inf_tf32_off_split": _case(tf32=False),
    "inf_tf32_off_k1": _case(**K1, tf32=False),
    "inf_out_bias_k1": _case(**K1, out_bias=True),
    "inf_out_bias_split": _case(out_bias=True),
    "inf_last_state_default_split": _case(fn="cond", last_state=True),
    "inf_last_state_default_k1": _case(**K1, fn="cond", last_state=True),
    "inf_last_state_f16s_k1": _case(**K1, fn="cond", policy="f16s", last_state=True),
    "inf_last_state_f16s_split": _case(fn="cond", policy="f16s", variant=4, last_state=True),
    "inf_infer_stores_f16s_k1": _case(**K1, policy="f16s", env={"DIMSUM_SCAN_INFER_STORES": "1"}),
    "inf_infer_stores_default_split": _case(env={"DIMSUM_SCAN_INFER_STORES": "1"}),
    "inf_conv_done_f16s_k1": _case(**K1, fn="cond", policy="f16s", conv_done=True),
    "inf_init_full": _case(**K1, fn="cond", init="full"),
    "inf_init_vec": _case(**K1, fn="cond", init="vec"),
    "inf_B_bias_k1": _case(**K1, B_bias=True),
    "inf_B_bias_split": _case(B_bias=True),
    "inf_dstate24": _case(N=24),
    "inf_force_general_f16s": _case(policy="f16s", force_general=True),
    "inf_no_out_proj": _case(**K1, fn="no_out_proj"),
    "inf_no_out_proj_cond": _case(fn="no_out_proj_cond", init="full"),
    "inf_autocast_bf16": _case(**K1, autocast=True),
    # ---- training: forward + backward ----
    "train_default": _case(grad=True),
    "train_default_k1": _case(**K1, grad=True),
    "train_tf32_off": _case(grad=True, tf32=False),
    "train_xdbl_t_off": _case(grad=True, env={"DIMSUM_XDBL_T_TRAIN": "0"}),
    "train_checkpoint_lvl1": _case(grad=True, env={"DIMSUM_MAMBA_CHECKPOINT_LVL": "1"}),
    "train_recompute_out_z": _case(grad=True, env={"DIMSUM_RECOMPUTE_OUT_Z": "1"}),
    "train_out_bias": _case(grad=True, out_bias=True),
    "train_no_out_proj": _case(grad=True, fn="no_out_proj"),
    "train_f16s": _case(grad=True, policy="f16s", d_inner=256),
    "train_f16s_BC_bias": _case(grad=True, policy="f16s", d_inner=256, B_bias=True, C_bias=True),
    "train_dstate24": _case(grad=True, N=24),
    "bi_default": _case(fn="bi", grad=True),
    "bi_inference": _case(fn="bi"),
    "bi_checkpoint_lvl1": _case(fn="bi", grad=True, env={"DIMSUM_MAMBA_CHECKPOINT_LVL": "1"}),
    "bi_recompute_out_z": _case(fn="bi", grad=True, env={"DIMSUM_RECOMPUTE_OUT_Z": "1"}),
    "bi_biases": _case(fn="bi", grad=True, out_bias=True, B_bias=True, C_bias=True),
}
BSZ, L, D_MODEL, R, W = 1, 256, 256, 4, 4


def _operands(c):
    """xz, the parameters and dout on the CPU (float32; xz as bf16 values under autocast)"""
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g)
    d, N = c["d_inner"], c["N"]
    p = dict(conv_w=rn(d, 1, W) * 0.5, conv_b=rn(d) * 0.1, x_proj_w=rn(R + 2 * N, d) / d ** 0.5, dt_proj_w=rn(d, R) / R ** 0.5,
             A=-torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(d, 1) + 0.1 * rn(d, N)), Dv=1 + 0.1 * rn(d), dt_bias=rn(d) * 0.5 - 4.0)
    if c["fn"] == "bi":
        p["A_b"] = -torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(d, 1) + 0.1 * rn(d, N))
    if not c["fn"].startswith("no_out_proj"):
        p["out_proj_w"] = rn(D_MODEL, d) / d ** 0.5
        if c["out_bias"]:
            p["out_proj_b"] = 0.1 * rn(D_MODEL)
    if c["B_bias"]:
        p["B_proj_b"] = 0.1 * rn(N)
    if c["C_bias"]:
        p["C_proj_b"] = 0.1 * rn(N)
    if c["init"] is not None:
        p["init"] = rn(BSZ, d, L) if c["init"] == "full" else rn(BSZ, d)
    xz = rn(BSZ, 2 * d, L)
    if c["autocast"]:
        xz = xz.bfloat16().float()
        for k in ("x_proj_w", "dt_proj_w", "out_proj_w"):
            p[k] = p[k].bfloat16().float()
    dout = rn(BSZ, L, D_MODEL) if "out_proj_w" in p else rn(BSZ, d, L)
    return xz, p, dout


def _scan64(u, delta, A, Bm, Cm, Dv):
    """y_t = C_t . h_t + D u_t, h_t = exp(delta_t A) h_{t-1} + delta_t B_t u_t; (b, d, l) operands, B / C (b, n, l) -> y, h_L"""
    h = u.new_zeros(u.shape[0], u.shape[1], A.shape[1])
    ys = []
    for t in range(u.shape[-1]):
        dt = delta[:, :, t, None]
        h = torch.exp(dt * A) * h + dt * Bm[:, None, :, t] * u[:, :, t, None]
        ys.append((h * Cm[:, None, :, t]).sum(-1))
    return torch.stack(ys, -1) + Dv[:, None] * u, h


def _reference(c, xz, p, dout):
    """the mixer in float64 torch on the CPU -> {name: tensor}: out, last_state, and with c["grad"] dxz and every parameter gradient"""
    xz = xz.double().requires_grad_(c["grad"])
    q = {k: v.double().requires_grad_(c["grad"]) for k, v in p.items()}
    d, N = c["d_inner"], c["N"]
    x, z = xz[:, :d], xz[:, d:]
    if not c["conv_done"]:
        x = F.silu(F.conv1d(F.pad(x, (W - 1, 0)), q["conv_w"], q["conv_b"], groups=d))
    x_dbl = torch.einsum("bdl,rd->brl", x, q["x_proj_w"])
    delta = F.softplus(torch.einsum("brl,dr->bdl", x_dbl[:, :R], q["dt_proj_w"]) + q["dt_bias"][:, None])
    Bm = x_dbl[:, R:R + N] + (q["B_proj_b"][:, None] if "B_proj_b" in q else 0)
    Cm = x_dbl[:, R + N:] + (q["C_proj_b"][:, None] if "C_proj_b" in q else 0)
    y, last = _scan64(x, delta, q["A"], Bm, Cm, q["Dv"])
    if c["fn"] == "bi":
        fl = lambda t: t.flip(-1)
        y = y + fl(_scan64(fl(x), fl(delta), q["A_b"], fl(Bm), fl(Cm), q["Dv"])[0])
    out = y * F.silu(z)
    if "out_proj_w" in q:
        out = torch.einsum("bdl,ed->ble", out, q["out_proj_w"]) + (q["out_proj_b"] if "out_proj_b" in q else 0)
    res = {"out": out.detach(), "last_state": last.detach()}
    if c["grad"]:
        out.backward(dout.double())
        res["dxz"] = xz.grad
        res.update({"g_" + k: v.grad for k, v in q.items()})
    return res


def _call(c, xz, p, last_state):
    from dimsum_amd import ops
    head = (xz, p["conv_w"], p["conv_b"], p["x_proj_w"], p["dt_proj_w"])
    tail = dict(D=p["Dv"], delta_bias=p["dt_bias"], B_proj_bias=p.get("B_proj_b"), C_proj_bias=p.get("C_proj_b"), delta_softplus=True)
    if c["fn"] == "bi":
        return ops.bimamba_inner_fn(*head, p["out_proj_w"], p.get("out_proj_b"), p["A"], p["A_b"], None, None, **tail)
    if c["fn"] == "plain":
        return ops.mamba_inner_fn(*head, p["out_proj_w"], p.get("out_proj_b"), p["A"], None, None, **tail)
    if c["fn"] == "cond":
        return ops.mamba_inner_fn_cond(*head, p["out_proj_w"], p.get("out_proj_b"), p["A"], None, None, **tail, init_states=p.get("init"),
                                       conv_done=c["conv_done"], last_state=last_state)
    if c["fn"] == "no_out_proj":
        return ops.mamba_inner_fn_no_out_proj(*head, p["A"], None, None, **tail)
    return ops.mamba_inner_fn_no_out_proj_cond(*head, p["A"], None, None, **tail, init_states=p.get("init"))


def run_case(name, monkeypatch):
    """-> (trace, {name: GPU tensor}, (xz, parameters, dout) on the CPU): one mixer call (and its backward) of CASES[name] under the spy"""
    from dimsum_amd import gemm, native
    c = CASES[name]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DIMSUM_SPLIT3_MIN_ROWS", "256")
    for k, v in (c["env"] or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", c["tf32"])
    xz, p, dout = _operands(c)
    xc = (xz.bfloat16() if c["autocast"] else xz).cuda().requires_grad_(c["grad"])
    pc = {k: v.cuda().requires_grad_(c["grad"]) for k, v in p.items()}
    last = torch.full((BSZ, c["d_inner"], c["N"]), float("nan"), device="cuda") if c["last_state"] else None
    old_policy = gemm.get_policy()
    gemm.set_policy(c["policy"])
    try:
        with contextlib.ExitStack() as stack:
            stack.enter_context(native.scan_fwd_variant(c["variant"]))
            if c["force_general"]:
                stack.enter_context(native.scan_force_general())
            if c["autocast"]:
                stack.enter_context(torch.autocast("cuda", dtype=torch.bfloat16))
            if not c["grad"]:
                stack.enter_context(torch.no_grad())
            if c["N"] == 16 and c["fn"] != "bi":
                assert (native.scan_fwd_kernel_for(BSZ, c["d_inner"], L, 16) == 1) == (c["variant"] == 1)
            spy = _Spy(monkeypatch)
            out = _call(c, xc, pc, last)
            if c["grad"]:
                out.backward(dout.cuda())
            torch.cuda.synchronize()
    finally:
        gemm.set_policy(old_policy)
    got = {"out": out.detach()}
    if last is not None:
        got["last_state"] = last
    if c["grad"]:
        got["dxz"] = xc.grad
        got.update({"g_" + k: v.grad for k, v in pc.items()})
    return spy.trace, got, (xz, p, dout)


def _bounds(c):
    """(rtol, max-relative atol) of out, dxz, parameter gradients (module docstring)"""
    if c["autocast"]:
        return (3e-2, 5e-2), (6e-2, 1e-1), (3e-2, 5e-2)
    if c["policy"] == "f16s":
        return ((1e-3, 1e-3),) * 3
    s = 5.0 if c["tf32"] else 1.0
    return (2e-4 * s, 2e-5 * s), (5e-4 * s, 5e-5 * s), (1e-3, 2e-4)


# name + flags of every launch, in order (the tensor signatures are in tests/golden/mixer_routes_trace.json)
CONV, CONV_COND, CONV_DMAJOR, CONV_BWD = "causal_conv1d_fwd", "causal_conv1d_fwd_cond", "causal_conv1d_fwd out", "causal_conv1d_bwd"
INF, KEEP, TRAIN = "need_ckpt=0 need_out=0 need_x=0", "need_ckpt=0 need_out=1 need_x=1", "need_ckpt=1 need_out=1 need_x=1"
SCAN, SCAN_DT = "selective_scan_fwd ", "selective_scan_fwd dt_proj[rank2] "
LINEAR, NN_ROWS, NT_ROWS = "gemm.linear", "gemm.mm_nn_rows", "gemm.mm_nt_rows"
PLANES_GEMM = "gemm_tn alias_rows=128"                              # gemm.out_proj_planes
F16_GEMM = ["rows_f16s want_l1=1", "gemm_tn scales[rank2]"]         # gemm.out_proj_f16: the weight image, the TN product over the block table
TAIL_T = [NT_ROWS, NT_ROWS, CONV_BWD]                               # the transposed-x_dbl backward tail: d dt_proj.weight, d x_proj.weight, conv
TAIL_ROWS = [NN_ROWS, NN_ROWS, CONV_BWD]                            # the row-major one
TRAIN_FWD = [CONV, SCAN + TRAIN, LINEAR]
BWD_T, BWD_ROWS = "selective_scan_bwd ckpt dB dC recompute_out_z=0", "selective_scan_bwd ckpt recompute_out_z=0"
F16S_TRAIN_FWD = [CONV, SCAN + TRAIN, "rows_f16s", "rows_f16s", "gemm_tn row_invs[rank1]"]        # images of out_z and W_out^T, their TN product
F16S_TRAIN_DOUT = ["rows_f16s", "gemm_nt scales[rank1]"]                                          # the image of dout, W_out^T dout^T
BI_FWD = [CONV_DMAJOR, "selective_scan_bidir_fwd need_ckpt=1 need_out=1"]
BI_BWD = "selective_scan_bidir_bwd dB dC dz recompute_out_z=0"
EXPECT = {
    "inf_default_split": [CONV, SCAN + INF + " out_z_planes=1", PLANES_GEMM],
    "inf_default_k1": [CONV, SCAN_DT + INF, LINEAR],
    "inf_default_k1_planes_always": [CONV, SCAN_DT + INF + " out_z_planes=1", PLANES_GEMM],
    "inf_default_k1_no_dt_fusion": [CONV, SCAN + INF, LINEAR],
    "inf_f16s_k1": [CONV, SCAN_DT + INF + " out_z_f16=1"] + F16_GEMM,
    "inf_f16s_split": [CONV, SCAN + INF, "rows_block_f16s"] + F16_GEMM,
    "inf_f16s_split_f16_off": [CONV, SCAN + INF + " out_z_planes=1", PLANES_GEMM],
    "inf_tf32_off_split": [CONV, SCAN + INF, LINEAR],
    "inf_tf32_off_k1": [CONV, SCAN + INF, LINEAR],
    "inf_out_bias_k1": [CONV, SCAN_DT + INF],                       # (out_proj with a bias: F.linear)
    "inf_out_bias_split": [CONV, SCAN + INF],
    "inf_last_state_default_split": [CONV, SCAN + KEEP + " out_z_planes=1", PLANES_GEMM],          # the planes are gated on training only
    "inf_last_state_default_k1": [CONV, SCAN + KEEP, LINEAR],
    "inf_last_state_f16s_k1": [CONV, SCAN + KEEP, LINEAR],
    "inf_last_state_f16s_split": [CONV, SCAN + KEEP + " out_z_planes=1", PLANES_GEMM],
    "inf_infer_stores_f16s_k1": [CONV, SCAN + KEEP, LINEAR],
    "inf_infer_stores_default_split": [CONV, SCAN + KEEP + " out_z_planes=1", PLANES_GEMM],
    "inf_conv_done_f16s_k1": [SCAN_DT + INF + " out_z_f16=1"] + F16_GEMM,
    "inf_init_full": [CONV_COND, CONV_DMAJOR, SCAN_DT + INF, LINEAR],                               # (the cond entry calls the plain one with out=)
    "inf_init_vec": [CONV, SCAN_DT + INF, LINEAR],
    "inf_B_bias_k1": [CONV, SCAN + INF, LINEAR],                    # (row-major x_dbl: no dt_proj fusion)
    "inf_B_bias_split": [CONV, SCAN + INF + " out_z_planes=1", PLANES_GEMM],
    "inf_dstate24": [CONV, "selective_scan_general_fwd need_out=0 need_x=0", LINEAR],
    "inf_force_general_f16s": [CONV, "selective_scan_general_fwd need_out=0 need_x=0", LINEAR],
    "inf_no_out_proj": [CONV, SCAN_DT + INF],
    "inf_no_out_proj_cond": [CONV_COND, CONV_DMAJOR, SCAN + INF],
    "inf_autocast_bf16": [CONV, SCAN + INF, LINEAR],
    "train_default": TRAIN_FWD + [BWD_T, NN_ROWS] + TAIL_T,
    "train_default_k1": TRAIN_FWD + [BWD_T, NN_ROWS] + TAIL_T,
    "train_tf32_off": TRAIN_FWD + [BWD_T, NN_ROWS] + TAIL_T,
    "train_xdbl_t_off": TRAIN_FWD + [BWD_ROWS, NN_ROWS] + TAIL_ROWS,
    "train_checkpoint_lvl1": TRAIN_FWD + [CONV, BWD_T, NN_ROWS] + TAIL_T,
    "train_recompute_out_z": TRAIN_FWD + ["selective_scan_bwd ckpt dB dC recompute_out_z=1", NN_ROWS] + TAIL_T,
    "train_out_bias": [CONV, SCAN + TRAIN, BWD_T, NN_ROWS] + TAIL_T,
    "train_no_out_proj": [CONV, SCAN + TRAIN, BWD_T] + TAIL_T,
    "train_f16s": F16S_TRAIN_FWD + F16S_TRAIN_DOUT + [BWD_T, "gemm_nn"] + TAIL_T,
    "train_f16s_BC_bias": F16S_TRAIN_FWD + F16S_TRAIN_DOUT + [BWD_ROWS, "gemm_nn"] + TAIL_ROWS,
    "train_dstate24": [CONV, "selective_scan_general_fwd need_out=1 need_x=1", LINEAR, "selective_scan_general_bwd dB dC", NN_ROWS] + TAIL_T,
    "bi_default": BI_FWD + [LINEAR, BI_BWD, NN_ROWS] + TAIL_T,
    "bi_inference": [CONV_DMAJOR, "selective_scan_bidir_fwd need_ckpt=0 need_out=0", LINEAR],
    "bi_checkpoint_lvl1": BI_FWD + [LINEAR, CONV, BI_BWD, NN_ROWS] + TAIL_T,
    "bi_recompute_out_z": BI_FWD + [LINEAR, "selective_scan_bidir_bwd dB dC dz recompute_out_z=1", NN_ROWS] + TAIL_T,
    "bi_biases": BI_FWD + [BI_BWD, NN_ROWS] + TAIL_T,
}


RECORDED = os.path.join(GOLDEN, "mixer_routes_trace.json")


def write_recorded(traces, path=RECORDED):
    """{case: [[name + flags, argument signatures], ..]} as JSON with one line per launch, so that a route change shows as a line diff"""
    cases = (json.dumps(n) + ": [\n" + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in tr) + "\n]" for n, tr in traces.items())
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(cases) + "\n}\n")


if __name__ == "__main__":      # python tests/test_mixer_routes_gpu.py (on the GPU): records the traces of all cases anew, after an intended route change
    new = {}
    for case in CASES:
        with pytest.MonkeyPatch.context() as mp:
            new[case] = run_case(case, mp)[0]
    write_recorded(new)


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_route(name, monkeypatch, recorded):
    c = CASES[name]
    trace, got, (xz, p, dout) = run_case(name, monkeypatch)
    assert [e[0] for e in trace] == EXPECT[name]
    assert json.loads(json.dumps(trace)) == recorded[name]
    ref = _reference(c, xz, p, dout)
    assert set(got) <= set(ref)
    b_out, b_dxz, b_par = _bounds(c)
    for k, v in got.items():
        if v is None:
            assert k == "g_init", k            # init_states only lends its buffer / keeps the autograd edge: dcond = None
            continue
        rtol, satol = b_out if k in ("out", "last_state") else b_dxz if k == "dxz" else b_par
        err = (v.double().cpu() - ref[k]).abs().max().item() / max(ref[k].abs().max().item(), 1e-300)
        print(f"{name} {k}: max |err| / max |ref| = {err:.2e} (bound {rtol:g} |ref| + {satol:g} max|ref|)")
        assert_close(v.double().cpu().numpy(), ref[k].numpy(), rtol, 0, f"{name} {k}", scale_atol=satol)
