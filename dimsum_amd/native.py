"""Tensor-level entry points with the SAME signatures as the reference's native modules
(`selective_scan_cuda`, `causal_conv1d_cuda`, and the Triton `_layer_norm_fwd/_bwd`), implemented on top of the C ABI
of libdimsum_hip.so.  This is the seam the reference's Python would bind: INTEGRATION.md shows the two-line shim.

Conventions kept from the reference host wrappers:
  * argument checks raise RuntimeError where the reference has TORCH_CHECK (selective_scan.cpp:235-305,
    causal_conv1d.cpp:226-262),
  * outputs are allocated here with torch's caching allocator (`out = empty_like(delta)`, selective_scan.cpp:311),
  * launches go to torch's CURRENT stream of the input's device, no synchronisation.
There is no CPU path: a non-GPU tensor or a missing library is an error.
"""
import contextlib

import os

import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


class _ZeroArena:
    """Zero-filled fp32 scratch for the small accumulators the backward kernels ADD into (conv / norm / scan weight-gradient sums, the token
    passes' (3, B, C) reductions, bias-gradient sums): one fill launch per 16-MB chunk instead of one per accumulator -- ~300 fills of a few KB
    .. 800 KB per DiM-L/2 training step. A slice is handed out once and never again; a chunk lives as long as any of its slices (a parameter
    gradient that is such a slice keeps its chunk until the next zero_grad). Per (device, stream); bypassed under stream capture."""
    CHUNK = 1 << 22          # floats

    def __init__(self):
        import threading
        self._lock, self._cur = threading.Lock(), {}

    def take(self, n, device):
        n = int(n)
        if n <= 0 or n > self.CHUNK // 4 or torch.cuda.is_current_stream_capturing() or os.environ.get("DIMSUM_ZERO_ARENA", "1") == "0":
            return torch.zeros(max(n, 0), device=device, dtype=torch.float32)
        pad = (n + 63) // 64 * 64                          # 256-byte slices: vectorised consumers (fused optimizers) stay on their fast path
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        with self._lock:
            buf, used = self._cur.get(key, (None, 0))
            if buf is None or used + pad > self.CHUNK:
                buf, used = torch.zeros(self.CHUNK, device=device, dtype=torch.float32), 0
            self._cur[key] = (buf, used + pad)
        return buf[used:used + n]


_zero_arena = _ZeroArena()


def _zeros(n, device):
    """n zero floats (a fresh slice of the zero arena)"""
    return _zero_arena.take(n, device)


def _check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _gpu(*ts):
    for t in ts:
        if t is not None:
            _check(t.is_cuda, "dimsum_amd.native: expected a GPU tensor (there is no CPU fallback; the CPU oracle "
                              "lives under oracle/ and is test infrastructure only)")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# selective_scan_cuda.fwd / .bwd   (mamba/csrc/selective_scan/selective_scan.cpp:226-492)
# ---------------------------------------------------------------------------------------------------------------------
# the producers' image modes (dimsum_*_params_t.y_split3 / out_split3): True = three pieces [hi | hi | lo], "f16s" = scaled fp16, "pair" = [hi | lo]
_SPLIT_MODE = {"f16s": 2, "pair": 3}
_scan_fwd_variant = 0     # dimsum_ssm_params_t.kernel_variant of the calls made from here: 0 = the library's own choice


@contextlib.contextmanager
def scan_fwd_variant(v):
    """tests / tuning: ask for one forward scan kernel (lanes per channel: 1, 2, 4, 16; 0 = automatic) for the calls made inside.
    A per-call field of the C ABI -- the library keeps no state; this host-side setting is not thread-safe."""
    global _scan_fwd_variant
    old, _scan_fwd_variant = _scan_fwd_variant, int(v)
    try:
        yield
    finally:
        _scan_fwd_variant = old


def scan_fwd_kernel_for(batch, dim, seqlen, dstate, n_groups=1):
    """which forward scan kernel the library runs for this launch shape, as lanes per channel (dimsum_ssm_scan_fwd_variant): 1 = the
    64-channel kernel (a full chip), 2 / 4 / 16 = the state-split kernels of underfilled launches"""
    P = _lib.SsmParams()
    _fill_ssm_shape(P, batch, dim, seqlen, dstate, n_groups)
    return int(_lib.load().dimsum_ssm_scan_fwd_variant(P))


def _fill_ssm_shape(P, batch, dim, seqlen, dstate, n_groups):
    """the launch shape of a dispatch query (no operands) into the dimsum_ssm_params_t P, with the kernel asked for by scan_fwd_variant"""
    P.batch, P.dim, P.seqlen, P.dstate, P.n_groups, P.n_chunks = batch, dim, seqlen, dstate, n_groups, (seqlen + 2047) // 2048
    if _scan_fwd_variant:
        _lib.attach_ext(P, _lib.SsmExt).kernel_variant = _scan_fwd_variant


def _fill_ssm(P, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, x, out_z, ckpt=None):
    """fills the reference-shaped struct P (dimsum_ssm_params_t) and links a zeroed dimsum_ssm_ext_t to it -> the extension (the caller sets
    what it uses beyond the reference interface: saved states, the inference fusions, timing events)"""
    E = _lib.attach_ext(P, _lib.SsmExt)
    E.kernel_variant, E.ckpt_ptr = _scan_fwd_variant, _ptr(ckpt)
    batch, dim, seqlen = u.shape
    P.batch, P.dim, P.seqlen, P.dstate = batch, dim, seqlen, A.shape[1]
    P.n_groups, P.n_chunks = B.shape[1], (seqlen + 2047) // 2048
    P.delta_softplus, P.dtype = int(bool(delta_softplus)), _DT[u.dtype]
    P.A_d_stride, P.A_dstate_stride = A.stride(0), A.stride(1)
    P.B_batch_stride, P.B_group_stride, P.B_dstate_stride = B.stride(0), B.stride(1), B.stride(2)
    P.C_batch_stride, P.C_group_stride, P.C_dstate_stride = C.stride(0), C.stride(1), C.stride(2)
    P.u_batch_stride, P.u_d_stride = u.stride(0), u.stride(1)
    P.delta_batch_stride, P.delta_d_stride = delta.stride(0), delta.stride(1)
    if z is not None:
        P.z_batch_stride, P.z_d_stride = z.stride(0), z.stride(1)
    if out is not None:
        P.out_batch_stride, P.out_d_stride = out.stride(0), out.stride(1)
    if out_z is not None:
        P.out_z_batch_stride, P.out_z_d_stride = out_z.stride(0), out_z.stride(1)
    P.A_ptr, P.B_ptr, P.C_ptr, P.D_ptr = _ptr(A), _ptr(B), _ptr(C), _ptr(D)
    P.u_ptr, P.delta_ptr, P.delta_bias_ptr, P.z_ptr = _ptr(u), _ptr(delta), _ptr(delta_bias), _ptr(z)
    P.out_ptr, P.x_ptr, P.out_z_ptr = _ptr(out), _ptr(x), _ptr(out_z)
    return E


def _check_ssm(u, delta, A, B, C, D, z, delta_bias):
    _gpu(u, delta, A, B, C, D, z, delta_bias)
    _check(u.dtype in _DT, "selective_scan: input must be float32, float16 or bfloat16")
    _check(A.dtype == torch.float32, "selective_scan: complex A is out of scope of this build (DiMSUM uses real A, "
                                     "mamba_simple.py:586); A must be float32")
    _check(B.dim() == 4 and C.dim() == 4, "selective_scan: only input-dependent B and C of shape (batch, groups, "
                                          "dstate, seqlen) are supported (constant B/C is unused by DiMSUM)")
    _check(delta.dtype == u.dtype and B.dtype == u.dtype and C.dtype == u.dtype, "selective_scan: dtype mismatch")
    batch, dim, seqlen = u.shape
    dstate, groups = A.shape[1], B.shape[1]
    _check(dstate <= 256, "selective_scan only supports state dimension <= 256")
    _check(tuple(delta.shape) == (batch, dim, seqlen), "selective_scan: delta must have shape (batch, dim, seqlen)")
    _check(tuple(A.shape) == (dim, dstate), "selective_scan: A must have shape (dim, dstate)")
    _check(tuple(B.shape) == (batch, groups, dstate, seqlen) and tuple(C.shape) == (batch, groups, dstate, seqlen),
           "selective_scan: B and C must have shape (batch, groups, dstate, seqlen)")
    for t, name in ((u, "u"), (delta, "delta"), (B, "B"), (C, "C"), (z, "z")):
        if t is not None:
            _check(t.stride(-1) == 1 or t.shape[-1] == 1, f"selective_scan: {name}.stride(-1) must be 1")
    if D is not None:
        _check(D.dtype == torch.float32 and tuple(D.shape) == (dim,) and D.stride(-1) == 1, "selective_scan: bad D")
    if delta_bias is not None:
        _check(delta_bias.dtype == torch.float32 and tuple(delta_bias.shape) == (dim,) and delta_bias.stride(-1) == 1,
               "selective_scan: bad delta_bias")
    if z is not None:
        _check(z.dtype == u.dtype and tuple(z.shape) == (batch, dim, seqlen), "selective_scan: bad z")


def scan_ckpt_shape(batch, dim, seqlen, dstate):
    """states kept for the backward: h before every 8th step, (batch, ceil(L/8), dstate, dim) fp32"""
    return (batch, (seqlen + 7) // 8, dstate, dim)


def scan_dt_proj_supported(u, z, A, dt_w, dt_xt, n_groups=1):
    """whether selective_scan_fwd(dt_proj=(dt_w, dt_xt)) is served (csrc/ssm_scan_fwd_kernel.hpp, kDt): the 64-channels-per-wave kernel on
    its full fp32 vector path -- float32, dstate 16, dim / n_groups % 64 == 0, seqlen % 4 == 0, 16-byte aligned rows, dt_rank % 4 == 0 and
    <= 32, dt_xt (dt_rank, batch seqlen) r-major -- and only where that kernel is the one a launch of this shape gets"""
    batch, dim, seqlen = u.shape
    R = dt_w.shape[1]
    return (u.is_cuda and u.dtype == torch.float32 and z is not None and A.shape[1] == 16 and (dim // n_groups) % 64 == 0 and seqlen % 4 == 0
            and dt_w.dtype == torch.float32 and dt_xt.dtype == torch.float32 and dt_w.dim() == 2 and dt_w.shape[0] == dim and R % 4 == 0 and 0 < R <= 32
            and dt_w.stride(1) == 1 and dt_w.stride(0) % 4 == 0 and dt_w.data_ptr() % 16 == 0
            and dt_xt.dim() == 2 and dt_xt.shape == (R, batch * seqlen) and dt_xt.stride(1) == 1 and 32 * dt_xt.stride(0) < 2 ** 31
            and u.stride(2) == 1 and z.stride(2) == 1 and all(st % 4 == 0 for st in (*u.stride()[:2], *z.stride()[:2])) and u.data_ptr() % 16 == 0
            and z.data_ptr() % 16 == 0 and scan_fwd_kernel_for(batch, dim, seqlen, A.shape[1], n_groups) == 1)


def scan_out_z_f16_supported(u, z, A, n_groups):
    """whether selective_scan_fwd(out_z_f16=True) is served: the 64-channel kernel's full fp32 inference path on whole 32-step tiles"""
    return (z is not None and u.dtype == torch.float32 and z.dtype == torch.float32 and A.shape[1] == 16 and not A.is_complex() and n_groups == 1
            and u.shape[1] % 64 == 0 and u.shape[2] % 32 == 0 and u.numel() > 0)


def selective_scan_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, need_out=True, need_x=True, need_ckpt=False, out_z_planes=False, dt_proj=None, out_z_f16=False):
    """-> [out, x, (out_z)]   exactly like selective_scan_cuda.fwd.
    `need_out=False` / `need_x=False` are inference extras: the corresponding store is skipped and None returned.
    `need_ckpt=True` (training extra) appends the tile-boundary states the backward kernel consumes.
    `out_z_planes=True` (inference extra, float32): out_z comes back as its split-bf16 pair of d-major planes, a (2 dim, batch seqlen)
    bfloat16 matrix [hi; lo] -- the operand image of out_proj's GEMM (gemm_tn(..., alias_rows=dim)), the same 4 bytes per element.
    `out_z_f16=True` (inference extra, see scan_out_z_f16_supported): out_z comes back as (image, inv): a (dim, batch seqlen) float16 matrix of
    block-scaled values and the (batch seqlen / 32, dim / 64) float32 table of the blocks' inverse scales (include/dimsum_hip.h, out_z_f16)."""
    if dt_proj is not None:
        # fused dt_proj (inference extra): delta = dt_w @ dt_xt is formed inside the scan (scan_dt_proj_supported); `delta` only lends its layout
        dt_w, dt_xt = dt_proj
        _gpu(dt_w, dt_xt)
        _check(delta is None and not need_ckpt and not need_out and scan_dt_proj_supported(u, z, A, dt_w, dt_xt, B.shape[1]),
               "selective_scan_fwd: dt_proj = (dt_w, dt_xt) needs delta = None, no saved states, no `out` and a shape scan_dt_proj_supported takes")
        delta = u                  # (argument checks and the out_z layout below; the kernel never reads it)
    _check_ssm(u, delta, A, B, C, D, z, delta_bias)
    batch, dim, seqlen = u.shape
    dstate = A.shape[1]
    n_chunks = (seqlen + 2047) // 2048
    out = torch.empty_like(delta) if need_out else None          # HBL layout like delta (selective_scan.cpp:310-311)
    x = torch.empty((batch, dim, n_chunks, dstate * 2), device=u.device, dtype=torch.float32) if need_x else None
    planes = z16 = None
    if out_z_f16:
        _check(not out_z_planes and not need_ckpt and not need_out and scan_out_z_f16_supported(u, z, A, B.shape[1]),
               "selective_scan_fwd: out_z_f16 needs no saved states, no `out`, no planes and a shape scan_out_z_f16_supported takes")
        z16 = (torch.empty((dim, batch * seqlen), device=u.device, dtype=torch.float16), torch.empty((batch * seqlen // 32, dim // 64), device=u.device, dtype=torch.float32))
        out_z = z16[0].view(dim, batch, seqlen).permute(1, 0, 2)
    elif out_z_planes:
        _check(z is not None and u.dtype == torch.float32 and seqlen % 8 == 0, "selective_scan_fwd: out_z_planes needs z, float32 I/O and seqlen % 8 == 0")
        planes = torch.empty((2 * dim, batch * seqlen), device=u.device, dtype=torch.bfloat16)
        out_z = planes[:dim].view(dim, batch, seqlen).permute(1, 0, 2)           # the hi plane as a (batch, dim, seqlen) view
    else:
        out_z = torch.empty_like(z) if z is not None else None
    ckpt = torch.empty(scan_ckpt_shape(batch, dim, seqlen, dstate), device=u.device, dtype=torch.float32) if need_ckpt else None
    if u.numel() > 0:
        P = _lib.SsmParams()
        E = _fill_ssm(P, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, x, out_z, ckpt)
        if planes is not None:
            E.out_z_lo_offset = dim * batch * seqlen
        if z16 is not None:
            E.out_z_f16, E.out_z_scale_ptr, E.out_z_scale_ld = 1, _ptr(z16[1]), z16[1].stride(0)
        if dt_proj is not None:
            P.delta_ptr = None
            E.dt_w_ptr, E.dt_x_ptr, E.dt_w_row_stride, E.dt_x_row_stride, E.dt_rank = _ptr(dt_w), _ptr(dt_xt), dt_w.stride(0), dt_xt.stride(0), dt_w.shape[1]
        with torch.cuda.device(u.device):
            _lib.check(_lib.load().dimsum_ssm_scan_fwd(P, _stream(u)), "selective_scan_fwd")
    res = [out, x]
    if z is not None:
        res.append(z16 if z16 is not None else out_z if planes is None else planes)
    if need_ckpt:
        res.append(ckpt)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# causal_conv1d_cuda.*   (causal-conv1d/csrc/causal_conv1d.cpp:221-577)
# One forward and one backward take every variant as a keyword (packed rows: seq_idx; per-segment states: end_slots + conv_state), with one
# operand check, one out / dx allocate-or-check, one fp32 conversion, one branch per parameter struct and one launch (_conv_launch), in
# _conv_fwd / _conv_bwd; the named variants are wrappers that insist on their arguments. A new variant is a keyword here, a struct branch,
# and a template flag in csrc/causal_conv1d.hip.
# ---------------------------------------------------------------------------------------------------------------------
def _check_conv(x, weight, bias):
    """the checks of both layouts -> True when x is channel-last and goes to the (batch, seqlen, dim) kernels. A tensor the
    seqlen-contiguous kernels serve stays with them (causal_conv1d.cpp:242-247 picks the layout the same way)"""
    _gpu(x, weight, bias)
    _check(x.dim() == 3, "causal_conv1d: x must be (batch, dim, seqlen)")
    _check(x.dtype in _DT, "causal_conv1d: input must be float32, float16 or bfloat16")
    channel_last = not (x.stride(2) == 1 or x.shape[2] == 1)
    _check(not channel_last or x.stride(1) == 1 or x.shape[1] == 1,
           "causal_conv1d: only seqlen-contiguous (batch, dim, seqlen) inputs are "
           "supported here (DiMSUM never feeds channel-last)")
    dim, width = weight.shape
    _check(dim == x.shape[1], "causal_conv1d: weight must be (dim, width)")
    _check(2 <= width <= 4, "causal_conv1d only supports width between 2 and 4")
    if bias is not None:
        _check(tuple(bias.shape) == (dim,) and bias.stride(-1) == 1, "causal_conv1d: bias must be (dim,)")
    return channel_last


def _check_token_ids(t, name, batch, seqlen, who):
    """a per-token int32 operand (seq_idx; end_slots: where it is >= 0 the state after that position goes into that slot of a pool): (batch,
    seqlen), contiguous. Dtype, rank, shape and contiguity here, the device by the caller, last. The VALUES stay on the device: seq_idx is only
    ever compared; that the non-negative end_slots are below num_slots and that none appears twice in one launch is the caller's contract
    (include/dimsum_hip.h)."""
    _check(torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (batch, seqlen) and t.is_contiguous(),
           f"{who}: {name} must be a contiguous int32 (batch, seqlen) = ({batch}, {seqlen}) tensor")


def _check_seq_idx(seq_idx, batch, seqlen, who):
    _check_token_ids(seq_idx, "seq_idx", batch, seqlen, who)


def _check_end_slots(end_slots, batch, seqlen, who):
    _check_token_ids(end_slots, "end_slots", batch, seqlen, who)


def _check_start_slots(start_slots, batch, seqlen, who):
    """start_slots: where it is >= 0 -- only at a segment's first position -- the segment continues that row of `initial_states`"""
    _check_token_ids(start_slots, "start_slots", batch, seqlen, who)


def _is_channel_last(t):
    """(batch, dim, seqlen) with channel stride 1: what the channel-last kernels address"""
    return t.stride(1) == 1 or t.shape[1] == 1


def _new_channel_last(x):
    """an uninitialised (batch, dim, seqlen) tensor like x whose memory is (batch, seqlen, dim)"""
    batch, dim, seqlen = x.shape
    return x.new_empty(batch, seqlen, dim).transpose(1, 2)


def _conv_f32(weight, bias):
    """the kernels read weights and bias as fp32, the bias densely: -> (weight, bias) so (fp32 operands are not copied)"""
    return weight.float(), bias.float().contiguous() if bias is not None else None


def _conv_launch(entry, P, x, who):
    """the conv section's launch: library entry point `entry` on the current stream of x's device"""
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.load(), entry)(P, _stream(x)), who)


def _fill_conv(P, x, weight, bias, silu, out):
    P.batch, P.dim, P.seqlen = x.shape
    P.width, P.silu_activation, P.dtype = weight.shape[1], int(bool(silu)), _DT[x.dtype]
    P.x_batch_stride, P.x_c_stride = x.stride(0), x.stride(1)
    P.weight_c_stride, P.weight_width_stride = weight.stride(0), weight.stride(1)
    P.x_ptr, P.weight_ptr, P.bias_ptr = _ptr(x), _ptr(weight), _ptr(bias)
    if out is not None:
        P.out_batch_stride, P.out_c_stride, P.out_ptr = out.stride(0), out.stride(1), _ptr(out)


def _fill_conv_cl(P, x, weight, bias, silu, out):
    """dimsum_conv_cl_params_t from (batch, dim, seqlen) VIEWS with channel stride 1: the token stride is the view's stride(2)"""
    P.batch, P.dim, P.seqlen = x.shape
    P.width, P.silu_activation, P.dtype = weight.shape[1], int(bool(silu)), _DT[x.dtype]
    P.x_batch_stride, P.x_l_stride = x.stride(0), x.stride(2)
    P.weight_c_stride, P.weight_width_stride = weight.stride(0), weight.stride(1)
    P.x_ptr, P.weight_ptr, P.bias_ptr = _ptr(x), _ptr(weight), _ptr(bias)
    if out is not None:
        P.out_batch_stride, P.out_l_stride, P.out_ptr = out.stride(0), out.stride(2), _ptr(out)


def _fill_conv_bwd(Q, dout, dx, dweight, dbias, channel_last):
    """what dimsum_conv_bwd_params_t / dimsum_conv_cl_bwd_params_t hold beyond their forward struct"""
    if channel_last:
        Q.dout_batch_stride, Q.dout_l_stride = dout.stride(0), dout.stride(2)
        Q.dx_batch_stride, Q.dx_l_stride = dx.stride(0), dx.stride(2)
    else:
        Q.dout_batch_stride, Q.dout_c_stride = dout.stride(0), dout.stride(1)
        Q.dx_batch_stride, Q.dx_c_stride = dx.stride(0), dx.stride(1)
    Q.dweight_c_stride, Q.dweight_width_stride = dweight.stride(0), dweight.stride(1)
    Q.dout_ptr, Q.dx_ptr, Q.dweight_ptr, Q.dbias_ptr = _ptr(dout), _ptr(dx), _ptr(dweight), _ptr(dbias)


CONV_CL_CHUNK = 64        # DIMSUM_CONV_CL_CHUNK: tokens one wave of the channel-last kernels walks; the next chunk re-reads width - 1 halo rows


def causal_conv1d_fwd(x, weight, bias, silu_activation, out=None, *, seq_idx=None, end_slots=None, conv_state=None):
    """-> out (batch, dim, seqlen), like causal_conv1d_cuda.causal_conv1d_fwd. Weights are used in fp32. A channel-last x (channel stride 1,
    e.g. the transpose of a (batch, seqlen, dim) activation or of one half of a (batch, seqlen, 2 dim) buffer) is read as it is and out
    is channel-last too.
    seq_idx: causal_conv1d_varlen_fwd's (packed rows); end_slots / conv_state: causal_conv1d_varlen_states_fwd's. Both need a
    seqlen-contiguous x."""
    who = ("causal_conv1d_varlen_states_fwd" if end_slots is not None or conv_state is not None else
           "causal_conv1d_varlen_fwd" if seq_idx is not None else "causal_conv1d_fwd")
    return _conv_fwd(who, x, weight, bias, silu_activation, out, seq_idx, end_slots, conv_state)


def _conv_fwd(who, x, weight, bias, silu_activation, out, seq_idx=None, end_slots=None, conv_state=None, start_slots=None, initial_states=None):
    """every forward of the (batch, dim, seqlen) conv; `who` names the variant: causal_conv1d_fwd (plain or channel-last), _varlen_fwd
    (seq_idx), _varlen_states_fwd (+ end_slots, conv_state), _varlen_resume_fwd (+ start_slots, initial_states). The shape, dtype and stride
    refusals of the packed-row operands come first (they need no GPU)."""
    resume = who == "causal_conv1d_varlen_resume_fwd"
    states, packed = resume or who == "causal_conv1d_varlen_states_fwd", who != "causal_conv1d_fwd"
    if packed:
        _check(x.dim() == 3, "causal_conv1d: x must be (batch, dim, seqlen)")
        _check_token_ids(seq_idx, "seq_idx", x.shape[0], x.shape[2], who)
    if states:
        _check_token_ids(end_slots, "end_slots", x.shape[0], x.shape[2], who)
        _check(torch.is_tensor(conv_state) and conv_state.dim() == 3 and conv_state.shape[0] >= 1 and tuple(conv_state.shape[1:]) == (x.shape[1], weight.shape[-1]),
               f"{who}: conv_state must be a pool (num_slots >= 1, dim, width)")
        _check(conv_state.dtype == x.dtype, f"{who}: conv_state must have x's dtype {x.dtype}, got {conv_state.dtype} (the state is x's elements, moved, not converted)")
    if resume:
        _check_start_slots(start_slots, x.shape[0], x.shape[2], who)
        _check(torch.is_tensor(initial_states) and initial_states.dim() == 3 and initial_states.shape[0] >= 1
               and tuple(initial_states.shape[1:]) == (x.shape[1], weight.shape[-1]), f"{who}: initial_states must be (n_init >= 1, dim, width)")
        _check(initial_states.dtype == x.dtype, f"{who}: initial_states must have x's dtype {x.dtype}, got {initial_states.dtype} (the carried "
                                                "inputs are x's elements, moved, not converted)")
    channel_last = _check_conv(x, weight, bias)
    if packed:
        if channel_last:
            raise RuntimeError(f"{who}: seq_idx needs a seqlen-contiguous x (the channel-last kernels take none)")
        _gpu(seq_idx, end_slots, conv_state, start_slots, initial_states)
    weight, bias = _conv_f32(weight, bias)
    if out is None:
        out = _new_channel_last(x) if channel_last else torch.empty_like(x)   # x's layout like the reference (causal_conv1d.cpp:262): d-major in Mamba
    elif channel_last:
        _gpu(out)
        _check(out.shape == x.shape and out.dtype == x.dtype and _is_channel_last(out), "causal_conv1d_fwd: out must be channel-last like x")
    elif packed:
        _gpu(out)
        _check(out.shape == x.shape and out.dtype == x.dtype and out.stride(2) == 1, f"{who}: bad out")
    if x.numel() == 0:
        return out
    if channel_last:
        P = _lib.ConvClParams()
        _fill_conv_cl(P, x, weight, bias, silu_activation, out)
        _conv_launch("dimsum_causal_conv1d_cl_fwd", P, x, who)
    elif states:
        R = _lib.ConvVarlenResumeParams() if resume else None
        P = R.states if resume else _lib.ConvVarlenStatesParams()
        _fill_conv(P.varlen.conv, x, weight, bias, silu_activation, out)
        P.varlen.seq_idx_ptr, P.varlen.seq_idx_batch_stride = _ptr(seq_idx), seq_idx.stride(0)
        P.num_slots, P.end_slots_ptr, P.end_slots_batch_stride = conv_state.shape[0], _ptr(end_slots), end_slots.stride(0)
        P.state_ptr, P.state_dtype = _ptr(conv_state), _DT[conv_state.dtype]
        P.state_slot_stride, P.state_c_stride, P.state_w_stride = conv_state.stride()
        if resume:
            R.n_init, R.start_slots_ptr, R.start_slots_batch_stride = initial_states.shape[0], _ptr(start_slots), start_slots.stride(0)
            R.init_ptr, R.init_dtype = _ptr(initial_states), _DT[initial_states.dtype]
            R.init_slot_stride, R.init_c_stride, R.init_w_stride = initial_states.stride()
        _conv_launch("dimsum_" + who, R if resume else P, x, who)
    elif packed:
        P = _lib.ConvVarlenParams()
        _fill_conv(P.conv, x, weight, bias, silu_activation, out)
        P.seq_idx_ptr, P.seq_idx_batch_stride = _ptr(seq_idx), seq_idx.stride(0)
        _conv_launch("dimsum_causal_conv1d_varlen_fwd", P, x, who)
    else:
        P = _lib.ConvParams()
        _fill_conv(P, x, weight, bias, silu_activation, out)
        _conv_launch("dimsum_causal_conv1d_fwd", P, x, who)
    return out


def causal_conv1d_fwd_cond(x, weight, bias, silu_activation, init_x):
    """causal_conv1d_cuda.causal_conv1d_fwd_cond: the result is written INTO init_x and returned; the values of init_x
    never enter the computation (causal_conv1d.cpp:326-329, SURVEY finding 1)."""
    _check(init_x.shape == x.shape and init_x.dtype == x.dtype and init_x.stride(-1) == 1, "causal_conv1d_fwd_cond: bad init_x")
    return causal_conv1d_fwd(x, weight, bias, silu_activation, out=init_x)


def causal_conv1d_varlen_fwd(x, weight, bias, silu_activation, seq_idx, out=None):
    """causal_conv1d_fwd on packed rows -> out (batch, dim, seqlen): tap j of position t counts iff no boundary (a change of seq_idx) lies
    in (t - j, t]. x (batch, dim, seqlen) with unit stride along seqlen and free batch / channel strides (a half of xz, a d-major view);
    a channel-last x is refused: those kernels take no seq_idx."""
    return _conv_fwd("causal_conv1d_varlen_fwd", x, weight, bias, silu_activation, out, seq_idx)


def causal_conv1d_varlen_states_fwd(x, weight, bias, silu_activation, seq_idx, end_slots, conv_state, out=None):
    """causal_conv1d_varlen_fwd that also stores per-segment conv states -> out: where end_slots[b, t] = s >= 0, conv_state[s, :, :] becomes
    the last `width` inputs of the segment ending at t (zero-padded on the left when the segment is shorter), x[b, :, t] last -- the window
    causal_conv1d_update shifts. conv_state: a pool (num_slots, dim, width) of x's dtype with free strides; slots nobody names are not
    touched. Inference only. The slots' values are the caller's contract (_check_token_ids)."""
    return _conv_fwd("causal_conv1d_varlen_states_fwd", x, weight, bias, silu_activation, out, seq_idx, end_slots, conv_state)


def causal_conv1d_varlen_resume_fwd(x, weight, bias, silu_activation, seq_idx, end_slots, conv_state, start_slots, initial_states, out=None):
    """causal_conv1d_varlen_states_fwd whose segments may CONTINUE a carried conv state -> out: where start_slots[b, t] = s >= 0 (allowed only
    at a segment's first position) the taps of that segment that reach before t read initial_states[s, :, :] -- the last `width` inputs of
    the earlier piece, newest last -- instead of zeros, and the state stored through end_slots is the last `width` values of
    concat(initial_states[s], the segment). initial_states: (n_init, dim, width) of x's dtype with free strides; it must not overlap a slot
    of conv_state that this launch stores (different lanes read and write one slot: the operator checks the storage ranges). Negative
    entries are what causal_conv1d_varlen_states_fwd does. Inference only. The values of both rows are the caller's contract."""
    return _conv_fwd("causal_conv1d_varlen_resume_fwd", x, weight, bias, silu_activation, out, seq_idx, end_slots, conv_state, start_slots,
                     initial_states)


def causal_conv1d_bwd(x, weight, bias, dout, dx, silu_activation, *, seq_idx=None):
    """-> [dx, dweight, dbias] like causal_conv1d_cuda.causal_conv1d_bwd (dx may be a caller-provided view). With a channel-last x, dx is
    channel-last and a dout of any other layout is brought there once (causal_conv1d.cpp:379).
    seq_idx: causal_conv1d_varlen_bwd's (packed rows, a seqlen-contiguous x)."""
    return _conv_bwd("causal_conv1d_varlen_bwd" if seq_idx is not None else "causal_conv1d_bwd", x, weight, bias, dout, dx, silu_activation, seq_idx)


def _conv_bwd(who, x, weight, bias, dout, dx, silu_activation, seq_idx=None):
    """every backward of the (batch, dim, seqlen) conv; `who` names the variant: causal_conv1d_bwd (plain or channel-last) or _varlen_bwd (seq_idx)"""
    packed = who == "causal_conv1d_varlen_bwd"
    if packed:
        _check(x.dim() == 3, "causal_conv1d: x must be (batch, dim, seqlen)")
        _check_token_ids(seq_idx, "seq_idx", x.shape[0], x.shape[2], who)
    channel_last = _check_conv(x, weight, bias)
    _check(not (packed and channel_last), f"{who}: seq_idx needs a seqlen-contiguous x (the channel-last kernels take none)")
    _gpu(dout, dx, seq_idx)
    _check(dout.shape == x.shape and dout.dtype == x.dtype and (channel_last or dout.stride(2) == 1 or dout.shape[2] == 1), f"{who}: bad dout")
    if channel_last and not _is_channel_last(dout):
        dout = dout.transpose(1, 2).contiguous().transpose(1, 2)
    if dx is None:
        dx = _new_channel_last(x) if channel_last else torch.empty(x.shape, device=x.device, dtype=x.dtype)
    else:
        _check(dx.shape == x.shape and dx.dtype == x.dtype and (_is_channel_last(dx) if channel_last else dx.stride(2) == 1), f"{who}: bad dx")
    w32, b32 = _conv_f32(weight, bias)
    # fp32 accumulate, then cast (cpp:405-425); ONE zero-filled buffer for both accumulators (one fill launch instead of two)
    acc = _zeros(weight.numel() + (weight.shape[0] if bias is not None else 0), x.device)
    dweight = acc[:weight.numel()].view(weight.shape)
    dbias = acc[weight.numel():] if bias is not None else None
    if x.numel() > 0:
        if packed:
            P = _lib.ConvVarlenBwdParams()
            Q, entry = P.conv, "dimsum_causal_conv1d_varlen_bwd"
            P.seq_idx_ptr, P.seq_idx_batch_stride = _ptr(seq_idx), seq_idx.stride(0)
        elif channel_last:
            P = Q = _lib.ConvClBwdParams()
            entry = "dimsum_causal_conv1d_cl_bwd"
        else:
            P = Q = _lib.ConvBwdParams()
            entry = "dimsum_causal_conv1d_bwd"
        (_fill_conv_cl if channel_last else _fill_conv)(Q.fwd, x, w32, b32, silu_activation, None)
        _fill_conv_bwd(Q, dout, dx, dweight, dbias, channel_last)
        _conv_launch(entry, P, x, who)
    return [dx, dweight.to(weight.dtype), dbias.to(bias.dtype) if bias is not None else None]


def causal_conv1d_varlen_bwd(x, weight, bias, dout, dx, silu_activation, seq_idx):
    """-> [dx, dweight, dbias] of causal_conv1d_varlen_fwd: dx[t] collects from the later positions of its own segment only; dweight sums
    the unmasked (tap, position) pairs, dbias every position"""
    return _conv_bwd("causal_conv1d_varlen_bwd", x, weight, bias, dout, dx, silu_activation, seq_idx)


# ---------------------------------------------------------------------------------------------------------------------
# the recurrent form: causal_conv1d_cuda.causal_conv1d_update (causal_conv1d.cpp:512-569) and the Triton
# selective_state_update (ops/triton/selective_state_update.py:115-190). Both update their state IN PLACE; every operand
# may be a strided view (csrc/mixer_step.hip addresses with one element stride per dim).
# ---------------------------------------------------------------------------------------------------------------------
def _check_state_indices(state_indices, x, who):
    """state_indices: int32 (batch,) -- row b of the call works on state[state_indices[b]] of a pool (num_slots, ...), a negative entry is a
    padding row (no state touched, zero output). Dtype, rank and length first (they need no GPU), the device last. The VALUES stay on the
    device: that they are below num_slots and that no slot is named twice is the caller's contract (include/dimsum_hip.h)."""
    _check(x.dim() == 2, f"{who}: x must be (batch, dim)")
    _check(torch.is_tensor(state_indices) and state_indices.dtype == torch.int32, f"{who}: state_indices must be an int32 tensor")
    _check(state_indices.dim() == 1, f"{who}: state_indices must be 1-D, one slot per batch row")
    _check(state_indices.shape[0] == x.shape[0], f"{who}: state_indices must have batch = {x.shape[0]} entries, got {state_indices.shape[0]}")
    _check(state_indices.is_cuda and state_indices.device == x.device, f"{who}: state_indices must be a GPU tensor on x's device")


def _fill_slots(S, state_indices, pool):
    S.slots_ptr, S.slots_stride, S.num_slots = _ptr(state_indices), state_indices.stride(0), pool.shape[0]


def _check_conv_carried(who, x, conv_state, weight, bias, pool=False):
    """weight, width, state and bias of the carried-state pair (causal_conv1d_update / _chunk), in this order; x is (batch, dim[, seqlen]).
    On the serving path: a message is only put together when its refusal fires."""
    batch, dim = x.shape[0], x.shape[1]
    if not (weight.dim() == 2 and weight.shape[0] == dim):
        raise RuntimeError(f"{who}: weight must be (dim, width)")
    width = weight.shape[1]
    if not 2 <= width <= 4:
        raise RuntimeError(f"{who} only supports width between 2 and 4")
    if pool:
        if not (conv_state.dim() == 3 and conv_state.shape[0] >= 1 and tuple(conv_state.shape[1:]) == (dim, width) and conv_state.dtype == x.dtype):
            raise RuntimeError(f"{who}: with state_indices conv_state must be a pool (num_slots >= 1, dim, width) of x's dtype")
    elif not (conv_state.dim() == 3 and tuple(conv_state.shape) == (batch, dim, width) and conv_state.dtype == x.dtype):
        raise RuntimeError(f"{who}: conv_state must be (batch, dim, width) of x's dtype")
    if bias is not None and tuple(bias.shape) != (dim,):
        raise RuntimeError(f"{who}: bias must be (dim,)")


def _fill_conv_carried(P, x, conv_state, weight, bias, silu, out):
    """what dimsum_conv_update_params_t and dimsum_conv_chunk_params_t share (the chunk's seqlen is its own); weight and bias as _conv_f32 made them"""
    P.batch, P.dim, P.width, P.silu_activation, P.dtype = x.shape[0], x.shape[1], weight.shape[1], int(bool(silu)), _DT[x.dtype]
    P.x_batch_stride, P.x_c_stride = x.stride(0), x.stride(1)
    P.state_batch_stride, P.state_c_stride, P.state_w_stride = conv_state.stride()
    P.weight_c_stride, P.weight_width_stride = weight.stride()
    P.out_batch_stride, P.out_c_stride = out.stride(0), out.stride(1)
    P.x_ptr, P.weight_ptr, P.bias_ptr, P.conv_state_ptr, P.out_ptr = _ptr(x), _ptr(weight), _ptr(bias), _ptr(conv_state), _ptr(out)


def causal_conv1d_update(x, conv_state, weight, bias, silu_activation, state_indices=None):
    """-> out (batch, dim), like causal_conv1d_cuda.causal_conv1d_update: conv_state (batch, dim, width) is shifted left by one and x
    appended, in place; out = act(sum_w conv_state * weight + bias). Weights are used in fp32.
    state_indices (batch,) int32 (upstream Mamba's conv_state_indices): conv_state is a pool (num_slots, dim, width) and row b works on
    conv_state[state_indices[b]]; a negative entry touches no state and gives a zero row. None: the call it always was."""
    if state_indices is not None:
        _check_state_indices(state_indices, x, "causal_conv1d_update")
    _gpu(x, conv_state, weight, bias)
    _check(x.dim() == 2 and x.dtype in _DT, "causal_conv1d_update: x must be (batch, dim) in float32, float16 or bfloat16")
    _check_conv_carried("causal_conv1d_update", x, conv_state, weight, bias, pool=state_indices is not None)
    weight, bias = _conv_f32(weight, bias)
    out = torch.empty_like(x)
    if x.numel() > 0:
        S = None if state_indices is None else _lib.ConvUpdateSlotsParams()
        P = _lib.ConvUpdateParams() if S is None else S.conv
        _fill_conv_carried(P, x, conv_state, weight, bias, silu_activation, out)
        if S is None:
            _conv_launch("dimsum_causal_conv1d_update", P, x, "causal_conv1d_update")
        else:
            _fill_slots(S, state_indices, conv_state)
            _conv_launch("dimsum_causal_conv1d_update_slots", S, x, "causal_conv1d_update (state_indices)")
    return out


def causal_conv1d_chunk(x, conv_state, weight, bias, silu_activation):
    """-> out (batch, dim, seqlen) in x's layout: causal_conv1d_update for any number of tokens (no reference counterpart). The conv sees
    conv_state[.., 1:] to the left of x; conv_state (batch, dim, width) becomes the last `width` values of concat(conv_state, x), in place.
    x needs stride(-1) == 1; its batch and channel strides and all of conv_state's are free. Weights are used in fp32.
    Shape, dtype and stride refusals first (they need no GPU), the device last."""
    _check(x.dim() == 3 and x.dtype in _DT, "causal_conv1d_chunk: x must be (batch, dim, seqlen) in float32, float16 or bfloat16")
    batch, dim, seqlen = x.shape
    _check(batch >= 1 and dim >= 1 and seqlen >= 1, "causal_conv1d_chunk: x must not be empty")
    _check_conv_carried("causal_conv1d_chunk", x, conv_state, weight, bias)
    _check(x.stride(2) == 1 or seqlen == 1, "causal_conv1d_chunk: x.stride(-1) must be 1")
    _gpu(x, conv_state, weight, bias)
    weight, bias = _conv_f32(weight, bias)
    out = torch.empty_like(x)           # x's layout: d-major in the mixer
    if out.stride(2) != 1 and seqlen > 1:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    P = _lib.ConvChunkParams()
    P.seqlen = seqlen
    _fill_conv_carried(P, x, conv_state, weight, bias, silu_activation, out)
    _conv_launch("dimsum_causal_conv1d_chunk", P, x, "causal_conv1d_chunk")
    return out


def selective_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, dt_proj=None, state_indices=None):
    """-> out (batch, dim), like the reference's selective_state_update: state (batch, dim, dstate) <- state exp(dt' A) + dt' B x in place,
    dt' = [softplus](dt + dt_bias); out = sum_n state C + D x, times silu(z). fp32 arithmetic; x, dt, z share one dtype, state and B / C
    are float32 or that dtype.
    `dt_proj=(dt_w (dim, R) float32, dt_x (batch, R))` (no reference counterpart): dt = dt_x @ dt_w^T is formed inside the kernel and `dt`
    must be None -- one GEMV launch less per step.
    state_indices (batch,) int32 (upstream Mamba's state_batch_indices): state is a pool (num_slots, dim, dstate) and row b works on
    state[state_indices[b]]; a negative entry touches no state and gives a zero row. None: the call it always was."""
    if state_indices is not None:
        _check_state_indices(state_indices, x, "selective_state_update")
    _gpu(state, x, dt, A, B, C, D, z, dt_bias)
    _check(x.dim() == 2 and x.dtype in _DT, "selective_state_update: x must be (batch, dim) in float32, float16 or bfloat16")
    batch, dim = x.shape
    if state_indices is None:
        _check(state.dim() == 3 and tuple(state.shape[:2]) == (batch, dim), "selective_state_update: state must be (batch, dim, dstate)")
    else:
        _check(state.dim() == 3 and state.shape[0] >= 1 and state.shape[1] == dim,
               "selective_state_update: with state_indices state must be a pool (num_slots >= 1, dim, dstate)")
    dstate = state.shape[2]
    _check(1 <= dstate <= 256 or state.numel() == 0, "selective_state_update only supports state dimension between 1 and 256")
    _check(state.dtype in (torch.float32, x.dtype), "selective_state_update: state must be float32 or of x's dtype")
    _check(A.dtype == torch.float32 and tuple(A.shape) == (dim, dstate), "selective_state_update: A must be float32 (dim, dstate)")
    _check(tuple(B.shape) == (batch, dstate) and tuple(C.shape) == (batch, dstate) and B.dtype == C.dtype and B.dtype in (torch.float32, x.dtype),
           "selective_state_update: B and C must be (batch, dstate), both float32 or both of x's dtype")
    if dt_proj is None:
        _check(dt is not None and dt.shape == x.shape and dt.dtype == x.dtype, "selective_state_update: dt must be (batch, dim) of x's dtype")
    else:
        dt_w, dt_x = dt_proj
        _gpu(dt_w, dt_x)
        _check(dt is None, "selective_state_update: dt_proj = (dt_w, dt_x) replaces dt, which must be None")
        _check(dt_w.dim() == 2 and dt_w.shape[0] == dim and dt_w.shape[1] >= 1 and dt_w.dtype == torch.float32
               and tuple(dt_x.shape) == (batch, dt_w.shape[1]) and dt_x.dtype == x.dtype,
               "selective_state_update: dt_proj must be (dt_w (dim, R) float32, dt_x (batch, R) of x's dtype), R >= 1")
    for t, name in ((D, "D"), (dt_bias, "dt_bias")):
        if t is not None:
            _check(tuple(t.shape) == (dim,), f"selective_state_update: {name} must be (dim,)")
    D = D.float().contiguous() if D is not None else None
    dt_bias = dt_bias.float().contiguous() if dt_bias is not None else None
    if z is not None:
        _check(z.shape == x.shape and z.dtype == x.dtype, "selective_state_update: z must be (batch, dim) of x's dtype")
    out = torch.empty_like(x)
    if state.numel() > 0 and x.numel() > 0:
        S = None if state_indices is None else _lib.StateUpdateSlotsParams()
        P = _lib.StateUpdateParams() if S is None else S.update
        P.batch, P.dim, P.dstate, P.dt_softplus = batch, dim, dstate, int(bool(dt_softplus))
        P.dtype, P.state_dtype, P.bc_dtype = _DT[x.dtype], _DT[state.dtype], _DT[B.dtype]
        P.state_batch_stride, P.state_d_stride, P.state_n_stride = state.stride()
        P.x_batch_stride, P.x_d_stride = x.stride()
        P.A_d_stride, P.A_n_stride = A.stride()
        P.B_batch_stride, P.B_n_stride = B.stride()
        P.C_batch_stride, P.C_n_stride = C.stride()
        P.out_batch_stride, P.out_d_stride = out.stride()
        if z is not None:
            P.z_batch_stride, P.z_d_stride = z.stride()
        if dt_proj is None:
            P.dt_batch_stride, P.dt_d_stride = dt.stride()
        else:
            E = _lib.attach_ext(P, _lib.StateUpdateExt)
            E.dt_rank, E.dt_w_ptr, E.dt_x_ptr = dt_w.shape[1], _ptr(dt_w), _ptr(dt_x)
            E.dt_w_d_stride, E.dt_w_r_stride = dt_w.stride()
            E.dt_x_batch_stride, E.dt_x_r_stride = dt_x.stride()
        P.state_ptr, P.x_ptr, P.dt_ptr, P.A_ptr, P.B_ptr, P.C_ptr = _ptr(state), _ptr(x), _ptr(dt), _ptr(A), _ptr(B), _ptr(C)
        P.D_ptr, P.z_ptr, P.dt_bias_ptr, P.out_ptr = _ptr(D), _ptr(z), _ptr(dt_bias), _ptr(out)
        with torch.cuda.device(x.device):
            if S is None:
                _lib.check(_lib.load().dimsum_selective_state_update(P, _stream(x)), "selective_state_update")
            else:
                _fill_slots(S, state_indices, state)
                _lib.check(_lib.load().dimsum_selective_state_update_slots(S, _stream(x)), "selective_state_update (state_indices)")
    return out


def decode_linear_serves(x, weight, *others):
    """whether dimsum_decode_linear takes this call: (batch <= 16, K) rows of one 16/32-bit float dtype shared by every other operand"""
    return (x.dim() == 2 and 1 <= x.shape[0] <= _lib.DECODE_MAX_BATCH and x.dtype in _DT and weight.dtype == x.dtype
            and all(t is None or t.dtype == x.dtype for t in others))


def decode_linear(x, weight, bias=None, norm=None, residual=None, residual_out=None, conv=None, state_indices=None):
    """-> y (batch, N), or (y, residual_out) when `residual_out` is asked for: y = x' @ weight^T (+ bias) on csrc/decode_step.hip, batch <= 16;
    x (batch, K), weight (N, K), bias (N) share one dtype T.
    norm = (norm_weight (K), norm_bias (K) or None, eps, is_rms_norm): x' = norm(x (+ residual)) * norm_weight (+ norm_bias) in the same launch;
    residual (batch, K) is float32 or T. residual_out: None, or the dtype (float32 or T, == residual's when one is given) in which
    x (+ residual) is also returned -- a fresh buffer, never a view of x or residual. Without `norm`, x' = x.
    conv = (conv_state (batch, D, W) of T, conv_weight (D, W), conv_bias (D) or None, silu): the outputs n < D go through one in-place
    step of the causal conv1d (causal_conv1d_update) before they are stored; y[:, :D] is the conv output, y[:, D:] the plain outputs.
    state_indices (batch,) int32, with `conv` only: conv_state is a pool (num_slots, D, W) and row b's epilogue works on
    conv_state[state_indices[b]]; a negative entry touches no state and leaves zeros in y[b, :D] (y[b, D:] is written as ever)."""
    if state_indices is not None:
        _check(conv is not None, "decode_linear: state_indices address the conv epilogue's states and need `conv`")
        _check_state_indices(state_indices, x, "decode_linear")
    _check(x.dim() == 2 and x.dtype in _DT and x.stride(1) == 1, "decode_linear: x must be (batch, K) with unit row stride in float32, float16 or bfloat16")
    batch, K = x.shape
    _check(1 <= batch <= _lib.DECODE_MAX_BATCH, f"decode_linear: batch must be 1..{_lib.DECODE_MAX_BATCH}")
    _check(weight.dim() == 2 and weight.shape[1] == K and weight.dtype == x.dtype and weight.stride(1) == 1 and K >= 1 and weight.shape[0] >= 1,
           "decode_linear: weight must be (N, K) of x's dtype with unit row stride")
    N = weight.shape[0]
    if bias is not None:
        _check(tuple(bias.shape) == (N,) and bias.dtype == x.dtype, "decode_linear: bias must be (N,) of x's dtype")
        bias = bias.contiguous()
    _check(norm is not None or (residual is None and residual_out is None), "decode_linear: residual / residual_out belong to the norm prologue")
    S = None if state_indices is None else _lib.DecodeLinearSlotsParams()
    P = _lib.DecodeLinearParams() if S is None else S.linear
    P.batch, P.n, P.k, P.dtype, P.residual_dtype = batch, N, K, _DT[x.dtype], _DT[x.dtype]
    keep = []
    res_out = None
    if norm is not None:
        nw, nb, eps, is_rms = norm
        _check(tuple(nw.shape) == (K,) and nw.dtype == x.dtype and (nb is None or (tuple(nb.shape) == (K,) and nb.dtype == x.dtype)),
               "decode_linear: norm weight / bias must be (K,) of x's dtype")
        nw, nb = nw.contiguous(), None if nb is None else nb.contiguous()
        keep += [nw, nb]
        P.norm, P.eps = (_lib.DECODE_NORM_RMS if is_rms else _lib.DECODE_NORM_LAYER), float(eps)
        P.norm_weight_ptr, P.norm_bias_ptr = _ptr(nw), _ptr(nb)
        res_dtype = residual.dtype if residual is not None else residual_out
        if res_dtype is not None:
            _check(res_dtype in (torch.float32, x.dtype), "decode_linear: the residual stream must be float32 or of x's dtype")
            P.residual_dtype = _DT[res_dtype]
        if residual is not None:
            _check(residual.shape == x.shape and residual.stride(1) == 1, "decode_linear: residual must be (batch, K) with unit row stride")
            _check(residual_out in (None, residual.dtype), "decode_linear: residual_out must have the residual's dtype")
            P.residual_ptr, P.residual_row_stride = _ptr(residual), residual.stride(0)
        if residual_out is not None:
            res_out = torch.empty((batch, K), device=x.device, dtype=res_dtype)
            P.residual_out_ptr, P.residual_out_row_stride = _ptr(res_out), res_out.stride(0)
    y = torch.empty((batch, N), device=x.device, dtype=x.dtype)
    if conv is not None:
        state, cw, cb, silu = conv
        _check(cw.dim() == 2 and 1 <= cw.shape[0] <= N and cw.dtype == x.dtype, "decode_linear: conv weight must be (D <= N, width) of x's dtype")
        D, W = cw.shape
        _check(2 <= W <= 4, "decode_linear: the conv epilogue only supports width between 2 and 4")
        if state_indices is None:
            _check(tuple(state.shape) == (batch, D, W) and state.dtype == x.dtype, "decode_linear: conv_state must be (batch, D, width) of x's dtype")
        else:
            _check(state.dim() == 3 and state.shape[0] >= 1 and tuple(state.shape[1:]) == (D, W) and state.dtype == x.dtype,
                   "decode_linear: with state_indices conv_state must be a pool (num_slots >= 1, D, width) of x's dtype")
        if cb is not None:
            _check(tuple(cb.shape) == (D,) and cb.dtype == x.dtype, "decode_linear: conv bias must be (D,) of x's dtype")
            cb = cb.contiguous()
            keep.append(cb)
        P.conv_dim, P.conv_width, P.silu_activation = D, W, int(bool(silu))
        P.state_batch_stride, P.state_c_stride, P.state_w_stride = state.stride()
        P.conv_weight_c_stride, P.conv_weight_width_stride = cw.stride()
        P.conv_weight_ptr, P.conv_bias_ptr, P.conv_state_ptr = _ptr(cw), _ptr(cb), _ptr(state)
    _gpu(x, weight, bias, residual, *(norm[:2] if norm is not None else ()), *(conv[:3] if conv is not None else ()))     # the device last
    P.x_row_stride, P.w_row_stride, P.y_row_stride = x.stride(0), weight.stride(0), y.stride(0)
    P.x_ptr, P.w_ptr, P.bias_ptr, P.y_ptr = _ptr(x), _ptr(weight), _ptr(bias), _ptr(y)
    with torch.cuda.device(x.device):
        if S is None:
            _lib.check(_lib.load().dimsum_decode_linear(P, _stream(x)), "decode_linear")
        else:
            _fill_slots(S, state_indices, conv[0])
            _lib.check(_lib.load().dimsum_decode_linear_slots(S, _stream(x)), "decode_linear (state_indices)")
    return y if residual_out is None else (y, res_out)


# ---------------------------------------------------------------------------------------------------------------------
# duplicating slots of a state pool: every layer's conv_state and ssm_state in one launch (csrc/state_copy.hip; no reference counterpart;
# dimsum_amd/utils/serving.py is the user)
# ---------------------------------------------------------------------------------------------------------------------
class StatePoolTable:
    """what state_copy_slots needs to know about a pool, built once and kept: `tensors` (the pool's tensors in layer order: they stay alive
    with the table), `num_slots`, `device`, `max_row_bytes`, and `table`, the device int64 (n_tensors, 3) of {base pointer, slot stride in
    bytes, row bytes} the kernel reads (None on the torch stand-in)"""

    def __init__(self, tensors, num_slots, table=None):
        self.tensors, self.num_slots, self.table = tensors, num_slots, table
        self.device = tensors[0].device
        self.max_row_bytes = max(t[0].numel() * t.element_size() for t in tensors)


def state_pool_tensors(pool, who="state_pool_table"):
    """the checks of a pool that need no GPU -> (its tensors in layer order, num_slots). pool: a key_value_memory_dict, {layer: (conv_state,
    ssm_state)} with every tensor (num_slots, ...), each slot's row contiguous (the slot stride is free: a view of a larger buffer is fine)"""
    _check(isinstance(pool, dict) and len(pool) > 0, f"{who}: the pool is a non-empty dict {{layer: (conv_state, ssm_state)}}")
    tensors = [t for key in sorted(pool) for t in pool[key]]
    _check(all(torch.is_tensor(t) and t.dim() >= 2 and t.shape[0] >= 1 and t[0].numel() >= 1 for t in tensors),
           f"{who}: every state of the pool must be a tensor (num_slots >= 1, ...) with non-empty rows")
    slots = sorted({t.shape[0] for t in tensors})
    _check(len(slots) == 1, f"{who}: every tensor of the pool must have the same num_slots, got {slots}")
    _check(all(t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= t[0].numel()) for t in tensors),
           f"{who}: every slot's row must be contiguous and the slots must not overlap")
    devices = sorted({str(t.device) for t in tensors})
    _check(len(devices) == 1, f"{who}: the pool must live on one device, got {devices}")
    return tensors, slots[0]


def state_pool_table(pool):
    """-> StatePoolTable of a key_value_memory_dict (see state_pool_tensors). The table's values travel as kernel arguments on the current
    stream (optim_write_ptrs): no staging buffer, no synchronisation."""
    tensors, num_slots = state_pool_tensors(pool)
    _gpu(*tensors)
    table = torch.empty((len(tensors), 3), dtype=torch.int64, device=tensors[0].device)
    rows = [v for t in tensors for v in (t.data_ptr(), t.stride(0) * t.element_size(), t[0].numel() * t.element_size())]
    optim_write_ptrs(table.view(-1), 0, rows)
    return StatePoolTable(tensors, num_slots, table)


def state_copy_pairs(pairs, num_slots, who="state_copy_slots"):
    """a host list of (src, dst) pairs checked -> int32 (n_pairs, 2) on the host. A pair with a negative index is padding. Refused: an index
    >= num_slots; a dst named twice; a dst that is also a src (the copy would read a row another pair writes)."""
    pairs = [(int(s), int(d)) for s, d in pairs]
    _check(all(s < num_slots and d < num_slots for s, d in pairs), f"{who}: a slot index is out of range for num_slots = {num_slots}: {pairs}")
    live = [(s, d) for s, d in pairs if s >= 0 and d >= 0]
    dsts = [d for _, d in live]
    _check(len(set(dsts)) == len(dsts), f"{who}: a dst slot is named twice: {pairs}")
    _check(not set(dsts) & {s for s, _ in live}, f"{who}: a dst slot is also a src: {pairs}")
    return torch.tensor(pairs, dtype=torch.int32).view(-1, 2)


def state_copy_slots(table, pairs):
    """for every pair (src, dst): slot dst of EVERY tensor of the pool := slot src, bit for bit, in ONE launch on the current stream.
    table: state_pool_table(pool). pairs: a host list of pairs (checked by state_copy_pairs, then uploaded), or a device int32 (n_pairs, 2)
    tensor taken as is -- the kernel reads it, skips pairs with a negative or out-of-range index, and under graph capture copies what the
    buffer holds at replay. The result is defined when no dst is another pair's src or dst."""
    _check(isinstance(table, StatePoolTable) and table.table is not None, "state_copy_slots: table must come from state_pool_table")
    if not torch.is_tensor(pairs):
        pairs = state_copy_pairs(pairs, table.num_slots)
        if pairs.shape[0] == 0:
            return
        pairs = pairs.to(table.device, non_blocking=True)
    _check(pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.stride(1) == 1
           and (pairs.shape[0] <= 1 or pairs.stride(0) >= 2), "state_copy_slots: pairs must be an int32 (n_pairs, 2) tensor with unit stride along a pair")
    _check(pairs.is_cuda and pairs.device == table.device, "state_copy_slots: pairs must be a GPU tensor on the pool's device")
    if pairs.shape[0] == 0:
        return
    P = _lib.StateCopyParams()
    P.num_slots, P.n_tensors, P.n_pairs = table.num_slots, len(table.tensors), pairs.shape[0]
    P.table_ptr, P.pairs_ptr, P.pairs_stride, P.max_row_bytes = _ptr(table.table), _ptr(pairs), max(pairs.stride(0), 2), table.max_row_bytes
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().dimsum_state_copy_slots(P, _stream(pairs)), "state_copy_slots")


# ---------------------------------------------------------------------------------------------------------------------
# the LM loss over rows of logits  (csrc/cross_entropy.hip; the reference's training recipes use a fused cross-entropy here)
# ---------------------------------------------------------------------------------------------------------------------
def _cross_entropy_params(logits, labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, what):
    _check(logits.dim() == 2 and logits.dtype in _DT and logits.shape[0] >= 1 and logits.shape[1] >= 1,
           f"{what}: logits must be (rows >= 1, vocab >= 1) in float32, float16 or bfloat16")
    M, V = logits.shape
    _check(logits.stride(1) == 1 and (M == 1 or logits.stride(0) >= V),
           f"{what}: logits must have unit column stride and a row stride >= vocab (a [..., :vocab] view of a padded buffer is fine)")
    _check(tuple(labels.shape) == (M,) and labels.dtype == torch.int64, f"{what}: labels must be (rows,) int64")
    _check(0.0 <= float(label_smoothing) < 1.0, f"{what}: label_smoothing must be in [0, 1)")
    P = _lib.CrossEntropyParams()
    P.dtype, P.rows, P.vocab, P.logits_row_stride = _DT[logits.dtype], M, V, max(logits.stride(0), V)
    P.ignore_index, P.label_smoothing, P.logit_scale, P.lse_square_scale = int(ignore_index), float(label_smoothing), float(logit_scale), float(lse_square_scale)
    return P


def cross_entropy_fwd(logits, labels, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """-> (loss, lse, z_loss), each (rows,); loss and z_loss float32, lse float64 (what the backward needs to form exp(s - lse) to fp32 accuracy
    under any row offset): with s = logit_scale * logits[m, :], lse = logsumexp(s), z_loss = lse_square_scale * lse^2,
    loss = lse - (1 - label_smoothing) s[label] - (label_smoothing / vocab) sum(s) + z_loss, in ONE read of the logits.
    logits (rows, vocab) float32 / float16 / bfloat16, unit column stride, any row stride >= vocab; labels (rows,) int64.
    label == ignore_index: loss = z_loss = 0; another label outside [0, vocab): loss = NaN."""
    P = _cross_entropy_params(logits, labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, "cross_entropy_fwd")
    _gpu(logits, labels)
    labels = labels.contiguous()
    loss, z_loss = (torch.empty(logits.shape[0], device=logits.device, dtype=torch.float32) for _ in range(2))
    lse = torch.empty(logits.shape[0], device=logits.device, dtype=torch.float64)
    P.logits_ptr, P.labels_ptr, P.loss_ptr, P.lse_ptr, P.z_loss_ptr = _ptr(logits), _ptr(labels), _ptr(loss), _ptr(lse), _ptr(z_loss)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.load().dimsum_cross_entropy_fwd(P, _stream(logits)), "cross_entropy_fwd")
    return loss, lse, z_loss


def cross_entropy_bwd(dloss, logits, lse, labels, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100, inplace=False):
    """-> dlogits (rows, vocab) of the logits' dtype: dloss[m] * logit_scale * ((1 + 2 lse_square_scale lse) softmax(s) - (1 - label_smoothing)
    onehot(label) - label_smoothing / vocab), one read and one write of the logits from the forward's lse. dloss (rows,) float32 with any
    stride >= 0 (an expanded scalar is read in place). inplace: the gradient replaces the logits and the returned tensor IS `logits`.
    A row with label == ignore_index is zeros; with another label outside [0, vocab) it is NaN."""
    P = _cross_entropy_params(logits, labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, "cross_entropy_bwd")
    M, V = logits.shape
    _check(tuple(dloss.shape) == (M,) and dloss.dtype == torch.float32 and dloss.stride(0) >= 0, "cross_entropy_bwd: dloss must be (rows,) float32")
    _check(tuple(lse.shape) == (M,) and lse.dtype == torch.float64, "cross_entropy_bwd: lse must be (rows,) float64, as cross_entropy_fwd returns it")
    _gpu(dloss, logits, lse, labels)
    labels, lse = labels.contiguous(), lse.contiguous()
    dlogits = logits if inplace else torch.empty((M, V), device=logits.device, dtype=logits.dtype)
    P.dlogits_row_stride, P.dloss_stride = max(dlogits.stride(0), V), dloss.stride(0)
    P.logits_ptr, P.labels_ptr, P.lse_ptr, P.dloss_ptr, P.dlogits_ptr = _ptr(logits), _ptr(labels), _ptr(lse), _ptr(dloss), _ptr(dlogits)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.load().dimsum_cross_entropy_bwd(P, _stream(logits)), "cross_entropy_bwd")
    return dlogits


# ---------------------------------------------------------------------------------------------------------------------
# the token sampler of the decode loop   (csrc/sample_logits.hip; the reference's sample(), utils/generation.py:55-80, in one launch)
# ---------------------------------------------------------------------------------------------------------------------
def sample_logits(logits, u, top_k=1, top_p=0.0, temperature=1.0, out=None, row_index=None, out_table=None):
    """-> tokens (rows,) int64 (`out` when given): one token per row of logits (rows, vocab) float32 / float16 / bfloat16, unit column stride,
    any row stride >= vocab. top_k == 1: argmax (the lowest index among equal maxima; u may be None). Otherwise among the top_k highest
    ranks (top_k <= 0 or >= vocab: all; equal logits rank by ascending index), then without the tokens whose higher-ranked mass is
    >= top_p (0 < top_p < 1), p ~ exp((l - max) / temperature), by the inverse CDF in ascending index at the row's uniform: u[r], u (rows,)
    float32 -- or, with row_index (a one-element int64 DEVICE tensor holding a step number), u[step, r] of u (steps, rows); out_table
    (steps, rows) int64 then also receives the token at [step, r]. The kernel draws no random numbers; every value written is in [0, vocab)."""
    _check(logits.dim() == 2 and logits.dtype in _DT and logits.shape[0] >= 1 and logits.shape[1] >= 1,
           "sample_logits: logits must be (rows >= 1, vocab >= 1) in float32, float16 or bfloat16")
    M, V = logits.shape
    _check(logits.stride(1) == 1 and (M == 1 or logits.stride(0) >= V),
           "sample_logits: logits must have unit column stride and a row stride >= vocab (a [..., :vocab] view of a padded buffer is fine)")
    temperature = float(temperature)
    _check(temperature > 0.0 and temperature != float("inf"), "sample_logits: temperature must be finite and > 0")
    top_k = int(top_k)
    _check(-2 ** 31 <= top_k < 2 ** 31, "sample_logits: top_k must fit 32 bits")
    steps = 0
    if row_index is not None:
        _check(row_index.dtype == torch.int64 and row_index.numel() == 1, "sample_logits: row_index must be one int64 on the device")
        _check(u is not None and u.dim() == 2, "sample_logits: with row_index, u must be (steps, rows)")
        steps = u.shape[0]
    else:
        _check(out_table is None, "sample_logits: out_table needs row_index")
    if u is not None:
        _check(u.dtype == torch.float32 and u.is_contiguous() and tuple(u.shape) == ((steps, M) if row_index is not None else (M,)),
               "sample_logits: u must be contiguous float32, (rows,) or with row_index (steps, rows)")
    else:
        _check(top_k == 1, "sample_logits: only top_k == 1 draws nothing: u is required")
    if out_table is not None:
        _check(out_table.dtype == torch.int64 and out_table.is_contiguous() and tuple(out_table.shape) == (steps, M),
               "sample_logits: out_table must be contiguous int64 (steps, rows), as u")
    if out is None:
        out = torch.empty(M, device=logits.device, dtype=torch.int64)
    else:
        _check(out.dtype == torch.int64 and out.numel() == M and out.is_contiguous(), "sample_logits: out must be contiguous int64 with one element per row")
    _gpu(logits, u, out, row_index, out_table)
    P = _lib.SampleLogitsParams()
    P.dtype, P.rows, P.vocab, P.logits_row_stride = _DT[logits.dtype], M, V, max(logits.stride(0), V)
    P.top_k, P.top_p, P.temperature, P.table_steps = top_k, float(top_p), temperature, steps
    P.logits_ptr, P.u_ptr, P.out_ptr, P.row_index_ptr, P.out_table_ptr = _ptr(logits), _ptr(u), _ptr(out), _ptr(row_index), _ptr(out_table)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.load().dimsum_sample_logits(P, _stream(logits)), "sample_logits")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fused add + RMSNorm / LayerNorm  (Triton _layer_norm_fwd / _layer_norm_bwd, ops/triton/layernorm.py:120-364)
# ---------------------------------------------------------------------------------------------------------------------
def layer_norm_fwd(x, weight, bias, eps, residual=None, out_dtype=None, residual_dtype=None, is_rms_norm=False,
                   x_bias=None, mod_scale=None, mod_shift=None, rows_per_batch=0, split3=False):
    """x: (M, N) -> (y, mean, rstd, residual_out), like _layer_norm_fwd (layernorm.py:120-187).
    residual_out is x itself when no residual is added and no dtype change is requested.
    Extras: `x_bias` (N) is added to x first (the bias of the Linear that produced x); `mod_scale/mod_shift`
    ((M / rows_per_batch, N), sharing a row stride) apply y * (1 + scale) + shift per batch element after the norm;
    `split3`: y is returned as the split-bf16 left operand image (M, 3N) bfloat16 of the Linear that consumes it (split3_rows);
    `split3="f16s"`: as a scaled-fp16 image (F16Image, rows_f16s)."""
    _gpu(x, weight, bias, residual)
    _check(x.dim() == 2 and x.stride(-1) == 1, "layer_norm_fwd: x must be (M, N) with contiguous rows")
    M, N = x.shape
    _check(tuple(weight.shape) == (N,), "layer_norm_fwd: weight must be (N,)")
    if residual is not None:
        _check(residual.shape == x.shape and residual.stride(-1) == 1, "layer_norm_fwd: bad residual")
        residual_dtype = residual.dtype
    y_inv = None
    if split3 == "f16s":
        _check(N % 4 == 0, "layer_norm_fwd: the f16s image needs N % 4 == 0")
        y = torch.empty((M, N), device=x.device, dtype=torch.float16)
        y_inv = torch.empty((M,), device=x.device, dtype=torch.float32)
    elif split3:
        _check(N % 4 == 0 and out_dtype in (None, torch.bfloat16), "layer_norm_fwd: split3 needs N % 4 == 0 (bfloat16 output)")
        y = torch.empty((M, (2 if split3 == "pair" else 3) * N), device=x.device, dtype=torch.bfloat16)
    else:
        y = torch.empty((M, N), device=x.device, dtype=x.dtype if out_dtype is None else out_dtype)
    need_res_out = residual is not None or x_bias is not None or (residual_dtype is not None and residual_dtype != x.dtype)
    if residual_dtype is None:
        residual_dtype = x.dtype
    residual_out = torch.empty((M, N), device=x.device, dtype=residual_dtype) if need_res_out else None
    mean = torch.empty((M,), device=x.device, dtype=torch.float32) if not is_rms_norm else None
    rstd = torch.empty((M,), device=x.device, dtype=torch.float32)
    if M > 0:
        P = _lib.NormParams()
        P.rows, P.cols, P.is_rms_norm, P.eps = M, N, int(is_rms_norm), float(eps)
        P.x_dtype, P.out_dtype, P.y_split3 = _DT[x.dtype], _DT[y.dtype], _SPLIT_MODE.get(split3, int(bool(split3)))
        P.y_inv_scale_ptr = _ptr(y_inv)
        P.residual_dtype = _DT[residual_out.dtype] if residual_out is not None else _DT[x.dtype]
        P.x_row_stride, P.y_row_stride = x.stride(0), y.stride(0)
        if residual is not None:
            P.residual_row_stride = residual.stride(0)
        if residual_out is not None:
            P.residual_out_row_stride = residual_out.stride(0)
        w32 = weight.float().contiguous()
        b32 = bias.float().contiguous() if bias is not None else None
        P.x_ptr, P.residual_ptr, P.weight_ptr, P.bias_ptr = _ptr(x), _ptr(residual), _ptr(w32), _ptr(b32)
        P.y_ptr, P.residual_out_ptr, P.mean_ptr, P.rstd_ptr = _ptr(y), _ptr(residual_out), _ptr(mean), _ptr(rstd)
        if x_bias is not None:
            xb32 = x_bias.float().contiguous()
            _check(tuple(xb32.shape) == (N,), "layer_norm_fwd: x_bias must be (N,)")
            P.xbias_ptr = _ptr(xb32)
        if mod_scale is not None:
            _gpu(mod_scale, mod_shift)
            _check(mod_shift is not None and rows_per_batch > 0 and M % rows_per_batch == 0, "layer_norm_fwd: bad modulation arguments")
            nb = M // rows_per_batch
            _check(tuple(mod_scale.shape) == (nb, N) and tuple(mod_shift.shape) == (nb, N) and mod_scale.dtype == torch.float32
                   and mod_shift.dtype == torch.float32 and mod_scale.stride(1) == 1 and mod_shift.stride(1) == 1
                   and mod_scale.stride(0) == mod_shift.stride(0), "layer_norm_fwd: mod_scale / mod_shift must be (M / rows_per_batch, N) float32 sharing a row stride")
            P.mod_scale_ptr, P.mod_shift_ptr, P.mod_row_stride, P.rows_per_batch = _ptr(mod_scale), _ptr(mod_shift), mod_scale.stride(0), rows_per_batch
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dimsum_norm_fwd(P, _stream(x)), "layer_norm_fwd")
    if y_inv is not None:
        y = F16Image(y, y_inv)
    elif split3 == "pair":
        y = PairImage(y)
    return y, mean, rstd, residual_out if residual_out is not None else x


def layer_norm_bwd(dy, x, weight, bias, eps, mean, rstd, dresidual=None, has_residual=False, is_rms_norm=False, x_dtype=None):
    """-> (dx, dw, db, dresidual_in), like _layer_norm_bwd (layernorm.py:288-364). `x` is the saved residual_out."""
    _gpu(dy, x, weight, rstd, dresidual)
    M, N = x.shape
    xf = x if x.dtype == torch.float32 else x.float()
    dyf = dy if dy.dtype == torch.float32 else dy.float()
    drf = None if dresidual is None else (dresidual if dresidual.dtype == torch.float32 else dresidual.float())
    dx32 = torch.empty((M, N), device=x.device, dtype=torch.float32)
    acc = _zeros(2 * N if bias is not None else N, x.device)        # (both accumulators out of the zero arena)
    dw = acc[:N]
    db = acc[N:] if bias is not None else None
    if M > 0:
        P = _lib.NormBwdParams()
        P.rows, P.cols, P.is_rms_norm, P.eps = M, N, int(is_rms_norm), float(eps)
        P.r_row_stride, P.dy_row_stride, P.dx_row_stride = xf.stride(0), dyf.stride(0), dx32.stride(0)
        if drf is not None:
            P.dres_row_stride = drf.stride(0)
        w32 = weight.float().contiguous()
        P.r_ptr, P.weight_ptr, P.mean_ptr, P.rstd_ptr = _ptr(xf), _ptr(w32), _ptr(mean), _ptr(rstd)
        P.dy_ptr, P.dres_ptr, P.dx_ptr, P.dweight_ptr, P.dbias_ptr = _ptr(dyf), _ptr(drf), _ptr(dx32), _ptr(dw), _ptr(db)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dimsum_norm_bwd(P, _stream(x)), "layer_norm_bwd")
    x_dtype = x_dtype or x.dtype
    dx = dx32 if x_dtype == torch.float32 else dx32.to(x_dtype)
    dresidual_in = None
    if has_residual:
        dresidual_in = dx if dx.dtype == x.dtype else dx32.to(x.dtype)
    return dx, dw.to(weight.dtype), db.to(bias.dtype) if bias is not None else None, dresidual_in


def _prep_ssm_bwd(who, u, delta, A, B, C, D, z, delta_bias, dout, dz, dB, dC, n_dirs, also=()):
    """what the two backward calls share before their struct is filled: the checks of dout / dz / dB / dC (`also`: the caller's own (condition,
    message) checks, made between those of dout and dz; messages carry the caller's name `who`) and the allocations
    -> du, ddelta, [dA per direction], dB, dC, dD, ddelta_bias, dz"""
    batch, dim, seqlen = u.shape
    _check(tuple(dout.shape) == (batch, dim, seqlen) and dout.dtype == u.dtype and (dout.stride(-1) == 1 or seqlen == 1), f"{who}: bad dout")
    for cond, msg in also:
        _check(cond, msg)
    if z is not None:
        if dz is None:
            dz = torch.empty_like(z)
        else:
            _check(dz.shape == z.shape and dz.dtype == z.dtype and dz.stride(-1) == 1, f"{who}: bad dz")
    du = torch.empty_like(u)
    ddelta = torch.empty_like(delta)
    # the zero-filled fp32 accumulators (selective_scan.cpp:458-466) out of ONE buffer: one fill launch instead of three
    nA, nD = A.numel(), (dim if D is not None else 0)
    acc = _zeros(n_dirs * nA + nD + (dim if delta_bias is not None else 0), u.device)
    dAs = [acc[i * nA:(i + 1) * nA].view(A.shape) for i in range(n_dirs)]
    # dB / dC: fp32 then cast (cpp:461-462,488); a caller may hand in fp32 views of B's / C's shape (unit stride along l) to have them written in place
    for t, like in ((dB, B), (dC, C)):
        _check(t is None or (t.shape == like.shape and t.dtype == torch.float32 and t.is_cuda and t.stride(-1) == 1), f"{who}: bad dB / dC buffer")
    dB = torch.empty(B.shape, device=u.device, dtype=torch.float32) if dB is None else dB
    dC = torch.empty(C.shape, device=u.device, dtype=torch.float32) if dC is None else dC
    dD = acc[n_dirs * nA:n_dirs * nA + nD] if D is not None else None
    ddelta_bias = acc[n_dirs * nA + nD:] if delta_bias is not None else None
    return du, ddelta, dAs, dB, dC, dD, ddelta_bias, dz


def _fill_ssm_bwd(Q, dout, du, ddelta, dA, dB, dC, dD, ddelta_bias, dz, ckpt):
    """the gradient half of Q (dimsum_ssm_bwd_params_t; _fill_ssm has filled Q.fwd) and a fresh workspace for the partial dB / dC (+ the
    states when no `ckpt` is given) -> the workspace, to be kept until the call is made"""
    Q.dout_batch_stride, Q.dout_d_stride = dout.stride(0), dout.stride(1)
    Q.dA_d_stride, Q.dA_dstate_stride = dA.stride(0), dA.stride(1)
    Q.dB_batch_stride, Q.dB_group_stride, Q.dB_dstate_stride = dB.stride(0), dB.stride(1), dB.stride(2)
    Q.dC_batch_stride, Q.dC_group_stride, Q.dC_dstate_stride = dC.stride(0), dC.stride(1), dC.stride(2)
    Q.du_batch_stride, Q.du_d_stride = du.stride(0), du.stride(1)
    Q.ddelta_batch_stride, Q.ddelta_d_stride = ddelta.stride(0), ddelta.stride(1)
    if dz is not None:
        Q.dz_batch_stride, Q.dz_d_stride = dz.stride(0), dz.stride(1)
    Q.dout_ptr, Q.dA_ptr, Q.dB_ptr, Q.dC_ptr, Q.dD_ptr = _ptr(dout), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dD)
    Q.du_ptr, Q.dz_ptr, Q.ddelta_ptr, Q.ddelta_bias_ptr = _ptr(du), _ptr(dz), _ptr(ddelta), _ptr(ddelta_bias)
    F = Q.fwd
    nbytes = _lib.load().dimsum_ssm_scan_bwd_workspace_bytes(F.batch, F.dim, F.seqlen, F.dstate, F.n_groups)
    if ckpt is not None:
        nbytes -= ckpt.numel() * 4          # the states part is only needed when they must be rebuilt
    ws = torch.empty((nbytes + 3) // 4, device=du.device, dtype=torch.float32)       # per-wave partial dB / dC (+ states)
    Q.workspace_ptr, Q.workspace_bytes = _ptr(ws), nbytes
    return ws


def _fill_ssm_reversed(P, A_b, out_b, ckpt_b):
    """the reversed direction's A / out / saved states into a dimsum_ssm_bidir_params_t or dimsum_ssm_bidir_bwd_params_t"""
    P.A_b_ptr, P.A_b_d_stride, P.A_b_dstate_stride = _ptr(A_b), A_b.stride(0), A_b.stride(1)
    if out_b is not None:
        P.out_b_ptr, P.out_b_batch_stride, P.out_b_d_stride = _ptr(out_b), out_b.stride(0), out_b.stride(1)
    P.ckpt_b_ptr = _ptr(ckpt_b)


def selective_scan_bwd(u, delta, A, B, C, D, z, delta_bias, dout, x, out, dz, delta_softplus, recompute_out_z, ckpt=None, dB=None, dC=None):
    """-> [du, ddelta, dA, dB, dC, dD, ddelta_bias, (dz), (out_z)] exactly like selective_scan_cuda.bwd
    (selective_scan.cpp:338-492). dz may be a caller-provided view (fused chunk backward, :433-441).
    `ckpt` (extra): the tile-boundary states of selective_scan_fwd(need_ckpt=True); without it they are rebuilt by one
    state-only sweep into a scratch buffer."""
    _check_ssm(u, delta, A, B, C, D, z, delta_bias)
    _gpu(dout, x, out, dz)
    batch, dim, seqlen = u.shape
    has_z = z is not None
    also = [(out is not None and out.shape == u.shape and out.stride(-1) == 1, "selective_scan_bwd: `out` of the forward is required with z")] if has_z else []
    du, ddelta, (dA,), dB, dC, dD, ddelta_bias, dz = _prep_ssm_bwd("selective_scan_bwd", u, delta, A, B, C, D, z, delta_bias, dout, dz, dB, dC, 1, also)
    out_z = torch.empty_like(out) if (has_z and recompute_out_z) else None
    if u.numel() > 0:
        Q = _lib.SsmBwdParams()
        if ckpt is not None:
            _gpu(ckpt)
            _check(tuple(ckpt.shape) == scan_ckpt_shape(batch, dim, seqlen, A.shape[1]) and ckpt.dtype == torch.float32
                   and ckpt.is_contiguous(), "selective_scan_bwd: bad ckpt")
        _fill_ssm(Q.fwd, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, x, out_z, ckpt)
        ws = _fill_ssm_bwd(Q, dout, du, ddelta, dA, dB, dC, dD, ddelta_bias, dz, ckpt)
        with torch.cuda.device(u.device):
            _lib.check(_lib.load().dimsum_ssm_scan_bwd(Q, _stream(u)), "selective_scan_bwd")
        del ws
    res = [du, ddelta, dA, dB.to(B.dtype), dC.to(C.dtype), dD, ddelta_bias]
    if has_z:
        res.append(dz)
    if out_z is not None:
        res.append(out_z)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the general selective scan (csrc/ssm_scan_general.hip): any dstate in 1..256, constant B / C, complex A
# ---------------------------------------------------------------------------------------------------------------------
SCAN_TUNED_DSTATES = (4, 8, 16, 32)      # what ssm_dispatch (csrc/ssm_scan_host.hpp) instantiates the tuned kernels for
_scan_force_general = False


@contextlib.contextmanager
def scan_force_general(on=True):
    """tests / measurement: the calls made inside take the general kernels even where a tuned kernel serves them (host-side, not thread-safe)"""
    global _scan_force_general
    old, _scan_force_general = _scan_force_general, bool(on)
    try:
        yield
    finally:
        _scan_force_general = old


def scan_general_forced():
    """the scan_force_general setting"""
    return _scan_force_general


def scan_takes_general_path(dstate, is_complex=False, is_variable_B=True, is_variable_C=True, force=False):
    """THE routing rule of selective_scan_fn / mamba_inner_fn, a pure function of its arguments (callers pass force=scan_general_forced()):
    the general kernels serve what the tuned ones are not built for -- complex A, constant B or C, a dstate outside SCAN_TUNED_DSTATES.
    Every call the tuned kernels serve keeps going to them."""
    return bool(force) or bool(is_complex) or not is_variable_B or not is_variable_C or int(dstate) not in SCAN_TUNED_DSTATES


def _check_ssm_general(u, delta, A, B, C, D, z, delta_bias):
    """-> (is_complex, is_variable_B, is_variable_C, n_groups). Dtypes, shapes and strides first (no GPU needed to be refused), the device last."""
    _check(u.dim() == 3 and u.dtype in _DT, "selective_scan_general: u must be (batch, dim, seqlen) float32, float16 or bfloat16")
    batch, dim, seqlen = u.shape
    cplx = A.is_complex()
    wdt = torch.complex64 if cplx else torch.float32
    _check(A.dim() == 2 and A.dtype == wdt, "selective_scan_general: A must be a float32 or complex64 (dim, dstate) matrix")
    dstate = A.shape[1]
    _check(1 <= dstate <= 256, "selective_scan only supports state dimension <= 256")
    _check(A.shape[0] == dim, "selective_scan_general: A must have shape (dim, dstate)")
    _check(delta.dtype == u.dtype and tuple(delta.shape) == (batch, dim, seqlen), "selective_scan_general: delta must be like u")
    var, groups = [], 1
    for t, name in ((B, "B"), (C, "C")):
        v = t.dim() >= 3
        var.append(v)
        if v:
            _check(t.dim() == 4 and t.dtype == u.dtype and t.shape[0] == batch and t.shape[2] == dstate and t.shape[3] == seqlen * (2 if cplx else 1),
                   f"selective_scan_general: input-dependent {name} must be (batch, groups, dstate, seqlen) of u's dtype (2 * seqlen with complex A)")
            _check(t.stride(-1) == 1 or t.shape[-1] == 1, f"selective_scan_general: {name}.stride(-1) must be 1")
        else:
            _check(t.dtype == wdt and tuple(t.shape) == (dim, dstate), f"selective_scan_general: constant {name} must be (dim, dstate) of A's dtype")
    if var[0] and var[1]:
        _check(B.shape[1] == C.shape[1], "selective_scan_general: B and C must have the same number of groups")
    if var[0] or var[1]:
        groups = (B if var[0] else C).shape[1]
        _check(groups >= 1 and dim % groups == 0, "selective_scan_general: dim must be a multiple of the number of groups")
    for t, name in ((u, "u"), (delta, "delta"), (z, "z")):
        if t is not None:
            _check(t.stride(-1) == 1 or t.shape[-1] == 1, f"selective_scan_general: {name}.stride(-1) must be 1")
    if z is not None:
        _check(z.dtype == u.dtype and tuple(z.shape) == (batch, dim, seqlen), "selective_scan_general: bad z")
    for t, name in ((D, "D"), (delta_bias, "delta_bias")):
        if t is not None:
            _check(t.dtype == torch.float32 and tuple(t.shape) == (dim,) and t.stride(-1) == 1, f"selective_scan_general: bad {name}")
    _check(batch <= 65535, "selective_scan_general: batch <= 65535")
    _gpu(u, delta, A, B, C, D, z, delta_bias)
    return cplx, var[0], var[1], groups


def _fill_bc_strides(P, name, t, var):
    """the stride fields of B / C / dB / dC: input-dependent (batch, groups, dstate, seqlen) -> batch / group / dstate, constant (dim, dstate) -> d / dstate"""
    for axis, stride in zip(("batch", "group", "dstate") if var else ("d", "dstate"), t.stride()):
        setattr(P, f"{name}_{axis}_stride", stride)


def _scan_launch(entry, P, u):
    """the general scan's launch: the library's dimsum_ssm_scan_<entry> on the current stream of u's device"""
    with torch.cuda.device(u.device):
        _lib.check(getattr(_lib.load(), "dimsum_ssm_scan_" + entry)(P, _stream(u)), "selective_scan_" + entry)


def _fill_ssm_general(P, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, x, out_z, flags):
    cplx, var_B, var_C, groups = flags
    batch, dim, seqlen = u.shape
    P.batch, P.dim, P.seqlen, P.dstate, P.n_groups, P.n_chunks = batch, dim, seqlen, A.shape[1], groups, (seqlen + 2047) // 2048
    P.delta_softplus, P.dtype = int(bool(delta_softplus)), _DT[u.dtype]
    P.is_variable_B, P.is_variable_C, P.is_complex = int(var_B), int(var_C), int(cplx)
    P.A_d_stride, P.A_dstate_stride = A.stride(0), A.stride(1)
    _fill_bc_strides(P, "B", B, var_B), _fill_bc_strides(P, "C", C, var_C)
    P.u_batch_stride, P.u_d_stride = u.stride(0), u.stride(1)
    P.delta_batch_stride, P.delta_d_stride = delta.stride(0), delta.stride(1)
    if z is not None:
        P.z_batch_stride, P.z_d_stride = z.stride(0), z.stride(1)
    if out is not None:
        P.out_batch_stride, P.out_d_stride = out.stride(0), out.stride(1)
    if out_z is not None:
        P.out_z_batch_stride, P.out_z_d_stride = out_z.stride(0), out_z.stride(1)
    P.A_ptr, P.B_ptr, P.C_ptr, P.D_ptr = _ptr(A), _ptr(B), _ptr(C), _ptr(D)
    P.u_ptr, P.delta_ptr, P.delta_bias_ptr, P.z_ptr = _ptr(u), _ptr(delta), _ptr(delta_bias), _ptr(z)
    P.out_ptr, P.x_ptr, P.out_z_ptr = _ptr(out), _ptr(x), _ptr(out_z)


def _check_scan_seq_idx(seq_idx, u, flags, who):
    """packed rows, behind the general checks: the ids, then what the packed kernels are not built for"""
    _check_seq_idx(seq_idx, u.shape[0], u.shape[2], who)
    cplx, var_B, var_C, _ = flags
    _check(not cplx, f"{who}: seq_idx with a complex A is not built (the packed-row kernels are instantiated for real A with input-dependent B and C)")
    _check(var_B and var_C, f"{who}: seq_idx with a constant B or C is not built (the packed-row kernels are instantiated for real A with "
                            "input-dependent B and C)")
    _gpu(seq_idx)


def selective_scan_varlen_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, seq_idx, need_out=True, need_x=True):
    """selective_scan_general_fwd on packed rows: seq_idx (batch, seqlen) int32, the state restarts at every position whose id differs from
    the one before it. x[:, :, -1, 1::2] is the state of the row's last segment. Real A, input-dependent B / C, any dstate in 1..256."""
    _check(seq_idx is not None, "selective_scan_varlen_fwd: seq_idx is required")
    return _scan_general_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, need_out, need_x, seq_idx=seq_idx)


def selective_scan_varlen_states_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, seq_idx, end_slots, ssm_state, need_out=True, need_x=True):
    """selective_scan_varlen_fwd that also stores per-segment states -> [out, x, (out_z)], exactly that function's: where end_slots[b, t] =
    s >= 0, ssm_state[s, :, :] becomes h_t, the state after position t (what step t + 1 would read). ssm_state: a pool (num_slots, dim,
    dstate), float32 or of u's dtype, with free strides; slots nobody names are not touched. Inference only. The slots' values are the
    caller's contract (_check_end_slots)."""
    who = "selective_scan_varlen_states_fwd"
    _check(seq_idx is not None, f"{who}: seq_idx is required")
    _check(torch.is_tensor(u) and u.dim() == 3, "selective_scan_general: u must be (batch, dim, seqlen) float32, float16 or bfloat16")
    _check_end_slots(end_slots, u.shape[0], u.shape[2], who)
    _check(torch.is_tensor(ssm_state) and ssm_state.dim() == 3 and ssm_state.shape[0] >= 1 and tuple(ssm_state.shape[1:]) == (u.shape[1], A.shape[1]),
           f"{who}: ssm_state must be a pool (num_slots >= 1, dim, dstate)")
    _check(ssm_state.dtype in (torch.float32, u.dtype), f"{who}: ssm_state must be float32 or of u's dtype {u.dtype}, got {ssm_state.dtype}")
    return _scan_general_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, need_out, need_x, seq_idx=seq_idx, end_slots=end_slots, ssm_state=ssm_state)


def selective_scan_varlen_resume_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, seq_idx, end_slots, ssm_state, start_slots, initial_states,
                                     need_out=True, need_x=True):
    """selective_scan_varlen_states_fwd whose segments may CONTINUE a carried state -> [out, x, (out_z)]: where start_slots[b, t] = s >= 0
    (allowed only at a segment's first position) the state entering position t is initial_states[s, :, :] instead of zeros. initial_states:
    (n_init, dim, dstate), float32 or of u's dtype, with free strides. It MAY be ssm_state itself: one lane owns each (channel, state), loads
    it at the segment's first step and stores it at the segment's end in its own program order -- provided a slot stored in this launch is
    read only by the segment that stores it. Inference only. The values of both rows are the caller's contract."""
    who = "selective_scan_varlen_resume_fwd"
    _check(seq_idx is not None, f"{who}: seq_idx is required")
    _check(torch.is_tensor(u) and u.dim() == 3, "selective_scan_general: u must be (batch, dim, seqlen) float32, float16 or bfloat16")
    _check_end_slots(end_slots, u.shape[0], u.shape[2], who)
    _check(torch.is_tensor(ssm_state) and ssm_state.dim() == 3 and ssm_state.shape[0] >= 1 and tuple(ssm_state.shape[1:]) == (u.shape[1], A.shape[1]),
           f"{who}: ssm_state must be a pool (num_slots >= 1, dim, dstate)")
    _check(ssm_state.dtype in (torch.float32, u.dtype), f"{who}: ssm_state must be float32 or of u's dtype {u.dtype}, got {ssm_state.dtype}")
    _check_start_slots(start_slots, u.shape[0], u.shape[2], who)
    _check(torch.is_tensor(initial_states) and initial_states.dim() == 3 and initial_states.shape[0] >= 1
           and tuple(initial_states.shape[1:]) == (u.shape[1], A.shape[1]), f"{who}: initial_states must be (n_init >= 1, dim, dstate)")
    _check(initial_states.dtype in (torch.float32, u.dtype),
           f"{who}: initial_states must be float32 or of u's dtype {u.dtype}, got {initial_states.dtype}")
    return _scan_general_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, need_out, need_x, seq_idx=seq_idx, end_slots=end_slots, ssm_state=ssm_state,
                             start_slots=start_slots, initial_states=initial_states)


def selective_scan_varlen_bwd(u, delta, A, B, C, D, z, delta_bias, dout, out, dz, delta_softplus, seq_idx, dB=None, dC=None):
    """selective_scan_general_bwd on packed rows: the adjoint state is not handed across a boundary and the terms through a_t h_{t-1} vanish there"""
    _check(seq_idx is not None, "selective_scan_varlen_bwd: seq_idx is required")
    return _scan_general_bwd(u, delta, A, B, C, D, z, delta_bias, dout, out, dz, delta_softplus, dB, dC, seq_idx=seq_idx)


def selective_scan_general_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, need_out=True, need_x=True, *, seq_idx=None, end_slots=None,
                               ssm_state=None, start_slots=None, initial_states=None):
    """-> [out, x, (out_z)] like selective_scan_cuda.fwd, on the general kernels: A float32 or complex64 (dim, dstate), dstate 1..256; B / C
    input-dependent (batch, groups, dstate, seqlen) -- (.., 2 seqlen) reals with complex A -- or constant (dim, dstate) of A's dtype.
    x is (batch, dim, n_chunks, 2 dstate) of A's dtype. None of the inference extras of selective_scan_fwd.
    seq_idx: selective_scan_varlen_fwd's (packed rows); end_slots / ssm_state: selective_scan_varlen_states_fwd's, which checks them;
    start_slots / initial_states on top of those: selective_scan_varlen_resume_fwd's, which checks them.
    One struct per variant, each holding the one before it; _fill_ssm_general fills the innermost."""
    flags = _check_ssm_general(u, delta, A, B, C, D, z, delta_bias)
    if seq_idx is not None:
        _check_scan_seq_idx(seq_idx, u, flags, "selective_scan_varlen_fwd")
    _check(end_slots is None or seq_idx is not None, "selective_scan_general_fwd: end_slots belong to packed rows (seq_idx)")
    _check(start_slots is None or end_slots is not None, "selective_scan_general_fwd: start_slots ride on the per-segment-states entry (end_slots)")
    if end_slots is not None:
        _gpu(end_slots, ssm_state, start_slots, initial_states)
    batch, dim, seqlen = u.shape
    dstate = A.shape[1]
    out = torch.empty_like(delta) if need_out else None
    x = torch.empty((batch, dim, (seqlen + 2047) // 2048, dstate * 2), device=u.device, dtype=A.dtype) if need_x else None
    out_z = torch.empty_like(z) if z is not None else None
    if u.numel() > 0:
        top = None                                                # the outermost struct, where it is not P
        if end_slots is not None:
            entry, P = "varlen_states_fwd", _lib.SsmVarlenStatesParams()
            if start_slots is not None:
                entry, top = "varlen_resume_fwd", _lib.SsmVarlenResumeParams()
                P = top.states
                top.n_init, top.start_slots_ptr, top.start_slots_batch_stride = initial_states.shape[0], _ptr(start_slots), start_slots.stride(0)
                top.init_ptr, top.init_f32 = _ptr(initial_states), int(initial_states.dtype == torch.float32)
                top.init_slot_stride, top.init_d_stride, top.init_dstate_stride = initial_states.stride()
            P.num_slots, P.end_slots_ptr, P.end_slots_batch_stride = ssm_state.shape[0], _ptr(end_slots), end_slots.stride(0)
            P.state_ptr, P.state_f32 = _ptr(ssm_state), int(ssm_state.dtype == torch.float32)
            P.state_slot_stride, P.state_d_stride, P.state_dstate_stride = ssm_state.stride()
        else:
            entry, P = ("varlen_fwd", _lib.SsmVarlenParams()) if seq_idx is not None else ("general_fwd", _lib.SsmGeneralParams())
        V = P.varlen if end_slots is not None else P              # with packed rows: the struct that holds the ids and the scan
        if seq_idx is not None:
            V.seq_idx_ptr, V.seq_idx_batch_stride = _ptr(seq_idx), seq_idx.stride(0)
        _fill_ssm_general(V.scan if seq_idx is not None else P, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, x, out_z, flags)
        _scan_launch(entry, P if top is None else top, u)
    return [out, x] + ([out_z] if z is not None else [])


def _check_carried_state(t, name, u, A):
    batch, dim, _ = u.shape
    want = torch.complex64 if A.is_complex() else None
    _check(t.dim() == 3 and tuple(t.shape) == (batch, dim, A.shape[1]), f"selective_scan_carry: {name} must be (batch, dim, dstate)")
    _check(t.dtype == want if want is not None else t.dtype in (torch.float32, u.dtype),
           f"selective_scan_carry: {name} must be float32 or of u's dtype (complex64 with complex A)")


def selective_scan_carry_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, initial_state, final_state):
    """-> out (batch, dim, seqlen), gated by silu(z) where z is given: the general forward (selective_scan_general_fwd's operands) entered
    with the carried state `initial_state` (batch, dim, dstate) instead of zeros -- None means zeros -- and leaving the state after the last
    step in `final_state` -- None means not wanted. Both are float32 or of u's dtype (complex64 with complex A), with free strides, and
    may be the SAME tensor: a cache, or a strided slice of one, updated in place. Inference only: there is no backward.
    Shape, dtype and stride refusals first (they need no GPU), the device last."""
    for t, name in ((initial_state, "initial_state"), (final_state, "final_state")):
        if t is not None:
            _check_carried_state(t, name, u, A)
    if initial_state is not None and final_state is not None:
        _check(initial_state.dtype == final_state.dtype, "selective_scan_carry: initial_state and final_state must share one dtype")
        _check(initial_state.data_ptr() != final_state.data_ptr() or initial_state.stride() == final_state.stride(),
               "selective_scan_carry: an in-place update needs final_state to be initial_state (same strides)")
    flags = _check_ssm_general(u, delta, A, B, C, D, z, delta_bias)
    _gpu(initial_state, final_state)
    _check(u.numel() > 0, "selective_scan_carry: u must not be empty")
    out = torch.empty_like(delta) if z is None else None       # with z only the gated output is stored
    out_z = torch.empty_like(z) if z is not None else None
    P = _lib.SsmCarryParams()
    _fill_ssm_general(P.scan, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, None, out_z, flags)
    state = initial_state if initial_state is not None else final_state
    if state is not None:
        P.state_dtype = _lib.F32 if state.dtype in (torch.float32, torch.complex64) else _DT[state.dtype]
    if initial_state is not None:
        P.h0_batch_stride, P.h0_d_stride, P.h0_dstate_stride = initial_state.stride()
    if final_state is not None:
        P.hT_batch_stride, P.hT_d_stride, P.hT_dstate_stride = final_state.stride()
    P.h0_ptr, P.hT_ptr = _ptr(initial_state), _ptr(final_state)
    _scan_launch("carry_fwd", P, u)
    return out_z if z is not None else out


def selective_scan_general_bwd(u, delta, A, B, C, D, z, delta_bias, dout, out, dz, delta_softplus, dB=None, dC=None, *, seq_idx=None):
    """-> [du, ddelta, dA, dB, dC, dD, ddelta_bias, (dz)] like selective_scan_cuda.bwd (without recompute_out_z), on the general kernels.
    dA / constant dB / dC come back in A's dtype, input-dependent dB / dC in B's / C's; a caller may hand in fp32 buffers of B's / C's shape
    (unit stride along the sequence) for input-dependent dB / dC: they are zero-filled here (the kernel adds into them) and returned as they are.
    seq_idx: selective_scan_varlen_bwd's (packed rows), whose struct holds the plain one."""
    flags = _check_ssm_general(u, delta, A, B, C, D, z, delta_bias)
    cplx, var_B, var_C, groups = flags
    if seq_idx is not None:
        _check_scan_seq_idx(seq_idx, u, flags, "selective_scan_varlen_bwd")
    _gpu(dout, out, dz)
    batch, dim, seqlen = u.shape
    dstate = A.shape[1]
    _check(tuple(dout.shape) == (batch, dim, seqlen) and dout.dtype == u.dtype and (dout.stride(-1) == 1 or seqlen == 1), "selective_scan_general_bwd: bad dout")
    if z is not None:
        _check(out is not None and out.shape == u.shape and out.dtype == u.dtype and out.stride(-1) == 1,
               "selective_scan_general_bwd: `out` of the forward is required with z")
        if dz is None:
            dz = torch.empty_like(z)
        else:
            _check(dz.shape == z.shape and dz.dtype == z.dtype and dz.stride(-1) == 1, "selective_scan_general_bwd: bad dz")
    du, ddelta = torch.empty_like(u), torch.empty_like(delta)
    dA = torch.zeros_like(A)
    own = []
    for t, like, var in ((dB, B, var_B), (dC, C, var_C)):
        if t is not None:
            _check(var and t.shape == like.shape and t.dtype == torch.float32 and t.is_cuda and t.stride(-1) == 1, "selective_scan_general_bwd: bad dB / dC buffer")
            t.zero_()
        own.append(t is None)
    dB = torch.zeros(B.shape, device=u.device, dtype=torch.float32 if var_B else A.dtype) if dB is None else dB
    dC = torch.zeros(C.shape, device=u.device, dtype=torch.float32 if var_C else A.dtype) if dC is None else dC
    dD = torch.zeros_like(D) if D is not None else None
    ddelta_bias = torch.zeros_like(delta_bias) if delta_bias is not None else None
    if u.numel() > 0:
        entry, P = ("varlen_bwd", _lib.SsmVarlenBwdParams()) if seq_idx is not None else ("general_bwd", _lib.SsmGeneralBwdParams())
        Q = P.bwd if seq_idx is not None else P
        if seq_idx is not None:
            P.seq_idx_ptr, P.seq_idx_batch_stride = _ptr(seq_idx), seq_idx.stride(0)
        _fill_ssm_general(Q.fwd, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out if z is not None else None, None, None, flags)
        Q.dout_batch_stride, Q.dout_d_stride = dout.stride(0), dout.stride(1)
        Q.dA_d_stride, Q.dA_dstate_stride = dA.stride(0), dA.stride(1)
        _fill_bc_strides(Q, "dB", dB, var_B), _fill_bc_strides(Q, "dC", dC, var_C)
        Q.du_batch_stride, Q.du_d_stride = du.stride(0), du.stride(1)
        Q.ddelta_batch_stride, Q.ddelta_d_stride = ddelta.stride(0), ddelta.stride(1)
        if dz is not None:
            Q.dz_batch_stride, Q.dz_d_stride = dz.stride(0), dz.stride(1)
        Q.dout_ptr, Q.dA_ptr, Q.dB_ptr, Q.dC_ptr, Q.dD_ptr = _ptr(dout), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dD)
        Q.du_ptr, Q.dz_ptr, Q.ddelta_ptr, Q.ddelta_bias_ptr = _ptr(du), _ptr(dz if z is not None else None), _ptr(ddelta), _ptr(ddelta_bias)
        nbytes = _lib.load().dimsum_ssm_scan_general_bwd_workspace_bytes(batch, dim, seqlen, dstate, groups, int(cplx))
        ws = torch.empty((nbytes + 3) // 4, device=u.device, dtype=torch.float32)
        Q.workspace_ptr, Q.workspace_bytes = _ptr(ws), nbytes
        _scan_launch(entry, P, u)
        del ws
    res = [du, ddelta, dA, dB.to(B.dtype) if var_B and own[0] else dB, dC.to(C.dtype) if var_C and own[1] else dC, dD, ddelta_bias]
    if z is not None:
        res.append(dz)
    return res


# what the named wrappers enter: the two bodies themselves, so that a stand-in for a public name never reroutes another public function
_scan_general_fwd, _scan_general_bwd = selective_scan_general_fwd, selective_scan_general_bwd


# ---------------------------------------------------------------------------------------------------------------------
# bidirectional selective scan: the two selective_scan_cuda calls of BiMambaInnerFn (mamba/mamba_ssm/ops/selective_scan_interface.py:1010-1388,
# the second one on .flip(-1) copies) as ONE pair of launches that reads the forward layouts backwards (csrc/ssm_scan_fwd_kernel.hpp, kRev)
# ---------------------------------------------------------------------------------------------------------------------
def scan_bidir_fwd_kernel_for(batch, dim, seqlen, dstate, n_groups=1):
    """which forward scan kernel serves both directions of selective_scan_bidir_fwd (dimsum_ssm_scan_bidir_fwd_variant): 16 = one lane per
    state where the library picks it for the shape (dstate 16, far too few channels to fill the chip), else 1 = the 64-channel kernel (the
    state-split kernels have no reversed form); -1 = not served (dstate other than 4, 8, 16, 32)"""
    P = _lib.SsmBidirParams()
    _fill_ssm_shape(P.fwd, batch, dim, seqlen, dstate, n_groups)
    return int(_lib.load().dimsum_ssm_scan_bidir_fwd_variant(P))


def _check_bidir(A, A_b, z):
    _gpu(A_b)
    _check(z is not None, "selective_scan_bidir: z is required")
    _check(A_b.dtype == torch.float32 and tuple(A_b.shape) == tuple(A.shape), "selective_scan_bidir: A_b must be float32 of A's shape")


def selective_scan_bidir_fwd(u, delta, A, A_b, B, C, D, z, delta_bias, delta_softplus, need_out=True, need_ckpt=False):
    """-> [out, out_b, out_z, (ckpt, ckpt_b)]: out = the forward-time scan with A, out_b = the reversed-time scan with A_b (both ungated, in
    forward time order; None unless need_out), out_z = (out + out_b) * silu(z) as out * silu(z) + out_b * silu(z). `need_ckpt` appends both
    directions' saved states (the reversed one's indexed in reversed time), which selective_scan_bidir_bwd consumes."""
    _check_ssm(u, delta, A, B, C, D, z, delta_bias)
    _check_bidir(A, A_b, z)
    batch, dim, seqlen = u.shape
    dstate = A.shape[1]
    _check(dstate in (4, 8, 16, 32), "selective_scan_bidir: dstate must be 4, 8, 16 or 32")
    out = torch.empty_like(delta) if need_out else None
    out_b = torch.empty_like(delta) if need_out else None
    out_z = torch.empty_like(z)
    ckpt = torch.empty(scan_ckpt_shape(batch, dim, seqlen, dstate), device=u.device, dtype=torch.float32) if need_ckpt else None
    ckpt_b = torch.empty_like(ckpt) if need_ckpt else None
    if u.numel() > 0:
        P = _lib.SsmBidirParams()
        _fill_ssm(P.fwd, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, None, out_z, ckpt)
        _fill_ssm_reversed(P, A_b, out_b, ckpt_b)
        with torch.cuda.device(u.device):
            _lib.check(_lib.load().dimsum_ssm_scan_bidir_fwd(P, _stream(u)), "selective_scan_bidir_fwd")
    res = [out, out_b, out_z]
    if need_ckpt:
        res += [ckpt, ckpt_b]
    return res


def selective_scan_bidir_bwd(u, delta, A, A_b, B, C, D, z, delta_bias, dout, out, out_b, ckpt, ckpt_b, delta_softplus, recompute_out_z,
                             dz=None, dB=None, dC=None):
    """-> [du, ddelta, dA, dA_b, dB, dC, dD, ddelta_bias, dz, (out_z)]: the gradients of selective_scan_bidir_fwd's out_z, both directions
    summed (dA / dA_b apart). `out`, `out_b`, `ckpt`, `ckpt_b` are what the forward returned with need_out / need_ckpt. dz may be a
    caller-provided view (dxz's z half); dB / dC fp32 views of B's / C's shape to be written in place (as in selective_scan_bwd)."""
    _check_ssm(u, delta, A, B, C, D, z, delta_bias)
    _check_bidir(A, A_b, z)
    _gpu(dout, out, out_b, ckpt, ckpt_b, dz)
    batch, dim, seqlen = u.shape
    also = [(t is not None and t.shape == u.shape and t.dtype == u.dtype and t.stride(-1) == 1,
             "selective_scan_bidir_bwd: `out` and `out_b` of the forward are required") for t in (out, out_b)]
    also += [(t is not None and tuple(t.shape) == scan_ckpt_shape(batch, dim, seqlen, A.shape[1]) and t.dtype == torch.float32 and t.is_contiguous(),
              "selective_scan_bidir_bwd: both directions' saved states (need_ckpt=True) are required") for t in (ckpt, ckpt_b)]
    du, ddelta, (dA, dA_b), dB, dC, dD, ddelta_bias, dz = _prep_ssm_bwd("selective_scan_bidir_bwd", u, delta, A, B, C, D, z, delta_bias, dout, dz, dB, dC, 2, also)
    out_z = torch.empty_like(out) if recompute_out_z else None
    if u.numel() > 0:
        P = _lib.SsmBidirBwdParams()
        _fill_ssm(P.bwd.fwd, u, delta, A, B, C, D, z, delta_bias, delta_softplus, out, None, out_z, ckpt)
        ws = _fill_ssm_bwd(P.bwd, dout, du, ddelta, dA, dB, dC, dD, ddelta_bias, dz, ckpt)
        _fill_ssm_reversed(P, A_b, out_b, ckpt_b)
        P.dA_b_ptr, P.dA_b_d_stride, P.dA_b_dstate_stride = _ptr(dA_b), dA_b.stride(0), dA_b.stride(1)
        with torch.cuda.device(u.device):
            _lib.check(_lib.load().dimsum_ssm_scan_bidir_bwd(P, _stream(u)), "selective_scan_bidir_bwd")
        del ws
    res = [du, ddelta, dA, dA_b, dB.to(B.dtype), dC.to(C.dtype), dD, ddelta_bias, dz]
    if out_z is not None:
        res.append(out_z)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# fused token-space transform (csrc/token_transform.hip)
# ---------------------------------------------------------------------------------------------------------------------
_TT_KIND = {("none", True): 0, ("none", False): 0, ("haar", True): 1, ("haar", False): 2, ("dct", True): 3, ("dct", False): 4}


def token_transform(x, kind, forward, in_index=None, out_index=None, gate=None, scale=None, shift=None, residual=None,
                    w=None, want_y=True, want_wsum=False, want_tsum=False, split3=False):
    """y[b, out_index[s], c] = T(x[b, in_index[s], c] * gate[b, c])[s] * (1 + scale[b, c]) + shift[b, c] + residual[b, out_index[s], c]
    x: (B, L, C) fp32 with unit channel stride (may be a channel slice of a wider tensor); index tables int32 (L,).
    With a weight tensor `w` (indexed like y) the same pass also reduces, per (batch, channel),
        wdot = sum_s T(.)[s, c] * w[b, out_index[s], c]     and (want_wsum)  wsum = sum_s w[b, out_index[s], c]
    and returns (y or None, wdot, wsum or None) -- the adaLN-modulation gradients of the block backward.
    `want_tsum` appends tsum = sum_s T(.)[s, c] (the plain token sum) to the returned tuple.
    `split3`: y is returned as the split-bf16 left operand image (B, L, 3C) bfloat16 of the Linear that consumes it (split3_rows);
    `split3="f16s"`: as a scaled-fp16 image (F16Image: data (B, L, C) float16, inv (B, L); C <= 1024)."""
    _gpu(x, in_index, out_index, gate, scale, shift, residual, w)
    _check(x.dim() == 3 and x.dtype == torch.float32 and x.stride(2) == 1, "token_transform: x must be (B, L, C) float32, channel-contiguous")
    B, L, C = x.shape
    grid = int(round(L ** 0.5))
    if kind != "none":
        _check(grid * grid == L and grid % 4 == 0, "token_transform: the token grid must be square with side % 4 == 0")
    _check(want_y or w is not None or want_tsum, "token_transform: nothing to compute")
    y_inv = None
    if split3 == "f16s":
        _check(want_y and C % 4 == 0 and C <= (2048 if kind == "none" else 1024) and w is None and not want_tsum,
               "token_transform: the f16s image needs channels % 4 == 0, <= 1024 (2048 without a transform), no reductions")
        y = torch.empty((B, L, C), device=x.device, dtype=torch.float16)
        y_inv = torch.empty((B, L), device=x.device, dtype=torch.float32)
    elif split3:
        _check(want_y and C % 4 == 0, "token_transform: split3 needs an output and channels % 4 == 0")
        y = torch.empty((B, L, (2 if split3 == "pair" else 3) * C), device=x.device, dtype=torch.bfloat16)
    else:
        y = torch.empty((B, L, C), device=x.device, dtype=torch.float32) if want_y else None
    mods = [m for m in (gate, scale, shift) if m is not None]
    mstride = 0
    for m in mods:
        _check(m.dtype == torch.float32 and tuple(m.shape) == (B, C) and m.stride(1) == 1, "token_transform: gate/scale/shift must be (B, C) float32")
        _check(mstride in (0, m.stride(0)), "token_transform: gate/scale/shift must share one row stride")
        mstride = m.stride(0)
    for t in (in_index, out_index):
        if t is not None:
            _check(t.dtype == torch.int32 and t.numel() == L and t.is_contiguous(), "token_transform: index tables must be int32 (L,)")
    if residual is not None:
        _check(residual.shape == x.shape and residual.dtype == torch.float32 and residual.stride(2) == 1, "token_transform: bad residual")
    wdot = wsum = tsum = None
    if w is not None:
        _check(w.shape == x.shape and w.dtype == torch.float32 and w.stride(2) == 1, "token_transform: bad w")
    if w is not None or want_tsum:
        red = _zeros(3 * B * C, x.device).view(3, B, C)
        wdot, wsum = (red[0] if w is not None else None), (red[1] if (w is not None and want_wsum) else None)
        tsum = red[2] if want_tsum else None
    if B > 0:
        P = _lib.TtParams()
        P.batch, P.tokens, P.channels, P.grid, P.kind = B, L, C, grid, _TT_KIND[(kind, bool(forward))]
        P.y_split3 = _SPLIT_MODE.get(split3, int(bool(split3)))
        P.y_inv_scale_ptr = _ptr(y_inv)
        P.x_batch_stride, P.x_token_stride = x.stride(0), x.stride(1)
        if y is not None:
            P.y_batch_stride, P.y_token_stride = y.stride(0), y.stride(1)
        if residual is not None:
            P.res_batch_stride, P.res_token_stride = residual.stride(0), residual.stride(1)
        P.red_batch_stride = C
        if w is not None:
            P.w_batch_stride, P.w_token_stride = w.stride(0), w.stride(1)
        P.mod_batch_stride = mstride
        P.x_ptr, P.in_index_ptr, P.out_index_ptr = _ptr(x), _ptr(in_index), _ptr(out_index)
        P.gate_ptr, P.scale_ptr, P.shift_ptr, P.residual_ptr, P.y_ptr = _ptr(gate), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(y)
        P.w_ptr, P.wdot_ptr, P.wsum_ptr, P.tsum_ptr = _ptr(w), _ptr(wdot), _ptr(wsum), _ptr(tsum)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dimsum_token_transform(P, _stream(x)), "token_transform")
    if y_inv is not None:
        return F16Image(y, y_inv)
    if split3 == "pair":
        y = PairImage(y)
    if want_tsum:
        return (y, wdot, wsum, tsum)
    return y if w is None else (y, wdot, wsum)


# ---- bias + GELU between two GEMMs as a row pass (csrc/act_rows.hip): GatedMLP, the plain Mlp; the experts' form is moe_act_* below ----
def _act_out(lead, H, split3, device, n_dbias=0):
    """what an activation row pass (csrc/act_rows.hip) writes for rows of H columns over the leading shape `lead` -> (out, inv, dbias):
    split3 False: (..., H) float32; True: the split-bf16 image (..., 3H) bfloat16; "pair": (..., 2H) bfloat16; "f16s": (..., H) float16 with
    inv (...) float32 (else None). dbias: n_dbias zeros for the kernel's atomics, or None"""
    inv = None
    if split3 == "f16s":
        out = torch.empty(lead + (H,), device=device, dtype=torch.float16)
        inv = torch.empty(lead, device=device, dtype=torch.float32)
    elif split3:
        out = torch.empty(lead + ((2 if split3 == "pair" else 3) * H,), device=device, dtype=torch.bfloat16)
    else:
        out = torch.empty(lead + (H,), device=device, dtype=torch.float32)
    return out, inv, (_zeros(n_dbias, device) if n_dbias else None)


def _act_image(out, inv, split3):
    return F16Image(out, inv) if split3 == "f16s" else PairImage(out) if split3 == "pair" else out


def gated_gelu_fwd(x12, bias=None, split3=False):
    """x12: (..., 2H) fp32 contiguous (w12 GEMM output WITHOUT bias), bias (2H) or None
    -> gelu_tanh(x12[..., :H] + bias[:H]) * (x12[..., H:] + bias[H:])   (mlp.py:66-70)
    split3: the result as the split-bf16 left operand image (..., 3H) bfloat16 of the w3 GEMM (split3_rows)"""
    _gpu(x12, bias)
    _check(x12.dtype == torch.float32 and x12.is_contiguous() and x12.shape[-1] % 8 == 0, "gated_gelu: x12 must be contiguous float32 with 2H % 8 == 0")
    H = x12.shape[-1] // 2
    if bias is not None:
        _check(bias.dtype == torch.float32 and tuple(bias.shape) == (2 * H,) and bias.is_contiguous(), "gated_gelu: bias must be (2H,) float32")
    h = _act_out(x12.shape[:-1], H, bool(split3), x12.device)[0]
    rows = x12.numel() // (2 * H)
    fn = _lib.load().dimsum_gated_gelu_fwd_split3 if split3 else _lib.load().dimsum_gated_gelu_fwd
    with torch.cuda.device(x12.device):
        _lib.check(fn(_ptr(x12), _ptr(bias), _ptr(h), rows, H, _stream(x12)), "gated_gelu_fwd")
    return h


def gated_gelu_bwd(x12, bias, dh, need_dbias=True, split3=False):
    """-> (dx12, dbias or None).  split3: dx12 as a split-bf16 operand image in weight order, (..., 3 * 2H) bfloat16 [hi | lo | hi];
    split3="pair": (..., 2 * 2H) bfloat16 [hi | lo] (PairImage);
    split3="f16s": as a scaled-fp16 image (F16Image: (..., 2H) float16 + one inverse scale per row, the exact row maximum; H <= 5120)"""
    _gpu(x12, bias, dh)
    dh = dh.contiguous()
    H = x12.shape[-1] // 2
    split3 = split3 if split3 in ("pair", "f16s") else bool(split3)
    f16s = split3 == "f16s"
    _check(not f16s or (x12.is_contiguous() and x12.dtype == torch.float32 and dh.dtype == torch.float32 and H % 4 == 0 and H <= 5120), "gated_gelu_bwd: the f16s image needs contiguous float32 rows, H % 4 == 0, H <= 5120")
    dx12, inv, dbias = _act_out(x12.shape[:-1], 2 * H, split3, x12.device, 2 * H if (bias is not None and need_dbias) else 0)
    lib = _lib.load()
    fn = {False: lib.dimsum_gated_gelu_bwd, True: lib.dimsum_gated_gelu_bwd_split3, "pair": lib.dimsum_gated_gelu_bwd_pair, "f16s": lib.dimsum_gated_gelu_bwd_f16s}[split3]
    with torch.cuda.device(x12.device):
        _lib.check(fn(_ptr(x12), _ptr(bias), _ptr(dh), _ptr(dx12), *((_ptr(inv),) if f16s else ()), _ptr(dbias), x12.numel() // (2 * H), H, _stream(x12)), "gated_gelu_bwd")
    return _act_image(dx12, inv, split3), dbias


_GELU_OUT = {False: _lib.GELU_OUT_F32, True: _lib.GELU_OUT_SPLIT3, "pair": _lib.GELU_OUT_PAIR, "f16s": _lib.GELU_OUT_F16S}


def _gelu_call(fn, what, x, bias, dh, split3, need_dbias, scales):
    """one launch of dimsum_gelu_fwd / _bwd: the output tensor (or image) of the asked mode, the struct, the call"""
    H = x.shape[-1]
    rows = x.numel() // H
    out, inv, dbias = _act_out(x.shape[:-1], H, split3, x.device, H if need_dbias else 0)
    P = _lib.GeluParams()
    P.out_image, P.rows, P.hidden = _GELU_OUT[split3], rows, H
    P.x_ptr, P.bias_ptr, P.dh_ptr, P.out_ptr, P.inv_scale_ptr, P.dbias_ptr = _ptr(x), _ptr(bias), _ptr(dh), _ptr(out), _ptr(inv), _ptr(dbias)
    if scales is not None:
        E = _lib.attach_ext(P, _lib.GeluExt)
        E.row_inv_ptr, E.bound_ptr = _ptr(scales[0]), _ptr(scales[1])
    with torch.cuda.device(x.device):
        _lib.check(fn(P, _stream(x)), what)
    return _act_image(out, inv, split3), dbias


def gelu_fwd(x, bias=None, split3=False, scales=None):
    """x: (..., H) fp32 contiguous (fc1 GEMM output WITHOUT bias), bias (H) or None -> gelu_tanh(x + bias)   (timm Mlp's act, models_dit.py:124)
    split3: the result as the left operand image of the fc2 GEMM -- True: split-bf16 (..., 3H) bfloat16 [hi | hi | lo]; "pair": PairImage
    [hi | lo]; "f16s": F16Image (H <= 5120) with the exact row maximum's scale, or -- scales = (row_inv (rows,), bound (2,) {wl1, bmax}), the
    fc1 GEMM's left-image scales and weight bound -- the bound-derived scale of gemm_nt(epilogue="gelu_f16")"""
    _gpu(x, bias)
    _check(x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 4 == 0, "gelu: x must be contiguous float32 with H % 4 == 0")
    H = x.shape[-1]
    if bias is not None:
        _check(bias.dtype == torch.float32 and tuple(bias.shape) == (H,) and bias.is_contiguous(), "gelu: bias must be (H,) float32")
    _check(split3 in (False, True, "pair", "f16s"), "gelu: split3 is False, True, 'pair' or 'f16s'")
    _check(split3 != "f16s" or H <= 5120, "gelu: the f16s image needs H <= 5120")
    if scales is not None:
        _gpu(*scales)
        _check(split3 == "f16s" and scales[0].dtype == torch.float32 and scales[0].is_contiguous() and scales[0].numel() == x.numel() // H
               and scales[1].dtype == torch.float32 and scales[1].is_contiguous() and scales[1].numel() == 2,
               "gelu: scales = (row_inv (rows,), bound (2,)) float32 go with the f16s image")
    return _gelu_call(_lib.load().dimsum_gelu_fwd, "gelu_fwd", x, bias, None, split3, False, scales)[0]


def gelu_bwd(x, bias, dh, need_dbias=True, split3=False):
    """-> (dx, dbias or None), dx = dh * gelu_tanh'(x + bias).  split3: dx as the operand image of fc1's two gradient GEMMs -- True: split-bf16 in
    weight order (..., 3H) bfloat16 [hi | lo | hi]; "pair": PairImage [hi | lo]; "f16s": F16Image (exact row maxima; H <= 5120)"""
    _gpu(x, bias, dh)
    dh = dh.contiguous()
    H = x.shape[-1]
    _check(x.dtype == torch.float32 and x.is_contiguous() and H % 4 == 0 and dh.dtype == torch.float32 and dh.shape == x.shape,
           "gelu_bwd: x and dh must be contiguous float32 of one shape with H % 4 == 0")
    if bias is not None:
        _check(bias.dtype == torch.float32 and tuple(bias.shape) == (H,) and bias.is_contiguous(), "gelu_bwd: bias must be (H,) float32")
    _check(split3 in (False, True, "pair", "f16s"), "gelu_bwd: split3 is False, True, 'pair' or 'f16s'")
    _check(split3 != "f16s" or H <= 5120, "gelu_bwd: the f16s image needs H <= 5120")
    return _gelu_call(_lib.load().dimsum_gelu_bwd, "gelu_bwd", x, bias, dh, split3, bias is not None and need_dbias, None)


# ---------------------------------------------------------------------------------------------------------------------
# the top-1 mixture-of-experts layer's row passes (csrc/moe.hip, the experts' activation: csrc/act_rows.hip; SwitchMLP, dimsum/switch_mlp.py:69-99)
# ---------------------------------------------------------------------------------------------------------------------
MOE_MAX_EXPERTS = 64
_MOE_MODE = {"softmax": _lib.MOE_ROUTE_SOFTMAX, "sigmoid": _lib.MOE_ROUTE_SIGMOID}


def _moe_rows(t, what, name="x"):
    _check(t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] % 4 == 0 and t.shape[1] > 0,
           f"{what}: {name} must be contiguous float32 (rows, H) with H % 4 == 0")


def _moe_index(t, n, what, name):
    _check(t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (n,), f"{what}: {name} must be contiguous int32 ({n},)")


def _moe_route_check(x, w, b, mode, what):
    _moe_rows(x, what)
    _check(mode in _MOE_MODE, f"{what}: mode is 'softmax' or 'sigmoid'")
    _check(w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.shape[1] == x.shape[1] and 1 <= w.shape[0] <= MOE_MAX_EXPERTS,
           f"{what}: the router weight must be contiguous float32 (E, H) with 1 <= E <= {MOE_MAX_EXPERTS}")
    _check(b is None or (b.dtype == torch.float32 and b.is_contiguous() and tuple(b.shape) == (w.shape[0],)), f"{what}: the router bias must be float32 (E,)")


def moe_route_fwd(x, w, b, mode):
    """x (T, H), router weight (E, H) and bias (E) or None, mode 'softmax' | 'sigmoid' -> prob (T), expert (T) int32 = max(route, 1) (first maximum),
    logits (T, E), and the stable counting sort of the tokens by expert: offsets (E + 1), perm (T), inv (T), row_expert (T), all int32.
    Three launches, no host synchronisation."""
    _gpu(x, w, b)
    _moe_route_check(x, w, b, mode, "moe_route_fwd")
    T, H = x.shape
    E = w.shape[0]
    dev = x.device
    lib = _lib.load()
    prob = torch.empty(T, device=dev, dtype=torch.float32)
    logits = torch.empty(T, E, device=dev, dtype=torch.float32)
    expert, perm, inv, row_expert = (torch.empty(T, device=dev, dtype=torch.int32) for _ in range(4))
    offsets = torch.empty(E + 1, device=dev, dtype=torch.int32)
    nbytes = int(lib.dimsum_moe_route_work_bytes(T, E))
    work = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.int32)
    P = _lib.MoeRouteParams()
    P.mode, P.num_experts, P.tokens, P.hidden = _MOE_MODE[mode], E, T, H
    P.x_ptr, P.w_ptr, P.b_ptr, P.prob_ptr, P.expert_ptr, P.logits_ptr = _ptr(x), _ptr(w), _ptr(b), _ptr(prob), _ptr(expert), _ptr(logits)
    P.offsets_ptr, P.perm_ptr, P.inv_ptr, P.row_expert_ptr, P.work_ptr, P.work_bytes = _ptr(offsets), _ptr(perm), _ptr(inv), _ptr(row_expert), _ptr(work), nbytes
    with torch.cuda.device(dev):
        _lib.check(lib.dimsum_moe_route_fwd(P, _stream(x)), "moe_route_fwd")
    return prob, expert, logits, offsets, perm, inv, row_expert


def moe_route_bwd(x, w, logits, prob, expert, inv, dprob, dxp, mode):
    """the router's adjoint -> (dx (T, H) = dxp[inv] + dlogit w, dw (E, H), db (E)); dlogit is formed in the kernel from the saved logits"""
    _gpu(x, w, logits, prob, expert, inv, dprob, dxp)
    _moe_route_check(x, w, None, mode, "moe_route_bwd")
    T, H = x.shape
    E = w.shape[0]
    _moe_rows(dxp, "moe_route_bwd", "dxp")
    _check(dxp.shape == x.shape and logits.dtype == torch.float32 and logits.is_contiguous() and tuple(logits.shape) == (T, E),
           "moe_route_bwd: dxp (T, H) and logits (T, E) float32")
    for t, n in ((prob, "prob"), (dprob, "dprob")):
        _check(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (T,), f"moe_route_bwd: {n} must be contiguous float32 (T,)")
    _moe_index(expert, T, "moe_route_bwd", "expert")
    _moe_index(inv, T, "moe_route_bwd", "inv")
    dx = torch.empty_like(x)
    acc = _zeros(E * H + E, x.device)
    dw, db = acc[:E * H].view(E, H), acc[E * H:]
    P = _lib.MoeRouteParams()
    P.mode, P.num_experts, P.tokens, P.hidden = _MOE_MODE[mode], E, T, H
    P.x_ptr, P.w_ptr, P.prob_ptr, P.expert_ptr, P.logits_ptr, P.inv_ptr = _ptr(x), _ptr(w), _ptr(prob), _ptr(expert), _ptr(logits), _ptr(inv)
    P.dprob_ptr, P.dxp_ptr, P.dx_ptr, P.dw_ptr, P.db_ptr = _ptr(dprob), _ptr(dxp), _ptr(dx), _ptr(dw), _ptr(db)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dimsum_moe_route_bwd(P, _stream(x)), "moe_route_bwd")
    return dx, dw, db


def _moe_rows_call(fn, what, src, perm, prob=None, y=None, want_dprob=False):
    _gpu(src, perm, prob, y)
    _moe_rows(src, what, "the rows")
    T, H = src.shape
    _moe_index(perm, T, what, "perm")
    _check(prob is None or (prob.dtype == torch.float32 and prob.is_contiguous() and tuple(prob.shape) == (T,)), f"{what}: prob must be contiguous float32 (T,)")
    _check(y is None or (y.dtype == torch.float32 and y.is_contiguous() and y.shape == src.shape), f"{what}: y must be contiguous float32 like the rows")
    dst = torch.empty_like(src)
    dprob = torch.empty(T, device=src.device, dtype=torch.float32) if want_dprob else None
    P = _lib.MoeRowsParams()
    P.rows, P.hidden = T, H
    P.src_ptr, P.perm_ptr, P.prob_ptr, P.y_ptr, P.dst_ptr, P.dprob_ptr = _ptr(src), _ptr(perm), _ptr(prob), _ptr(y), _ptr(dst), _ptr(dprob)
    with torch.cuda.device(src.device):
        _lib.check(fn(P, _stream(src)), what)
    return dst, dprob


def moe_permute(x, perm, split3=False):
    """xp[j, :] = x[perm[j], :]  (perm: int32, entries in [0, T))
    split3="f16s": xp as the scaled-fp16 image (F16Image, exact row maxima) moe_gemm_f16s reads -- rows_f16s(moe_permute(x, perm)) bit for bit, in
    one pass that writes 2 bytes per element instead of 4 + (4 + 2)"""
    _check(split3 in (False, "f16s"), "moe_permute: split3 is False or 'f16s'")
    if not split3:
        return _moe_rows_call(_lib.load().dimsum_moe_permute, "moe_permute", x, perm)[0]
    _gpu(x, perm)
    _moe_rows(x, "moe_permute", "the rows")
    T, H = x.shape
    _moe_index(perm, T, "moe_permute", "perm")
    out, inv, _ = _act_out((T,), H, "f16s", x.device)
    P = _lib.MoePermuteF16sParams()
    P.rows, P.hidden = T, H
    P.src_ptr, P.perm_ptr, P.dst_ptr, P.inv_scale_ptr = _ptr(x), _ptr(perm), _ptr(out), _ptr(inv)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dimsum_moe_permute_f16s(P, _stream(x)), "moe_permute")
    return F16Image(out, inv)


def moe_combine_fwd(y, perm, prob):
    """out[perm[j], :] = prob[perm[j]] * y[j, :]: perm is a permutation, every token's row is written exactly once"""
    _check(prob is not None, "moe_combine_fwd: prob is required")
    return _moe_rows_call(_lib.load().dimsum_moe_combine_fwd, "moe_combine_fwd", y, perm, prob=prob)[0]


def moe_combine_bwd(dout, y, perm, prob):
    """-> (dy (sorted order) = prob[t] dout[t], dprob (T) = <dout[t], y[j]>), t = perm[j], in one pass over (dout, y)"""
    _check(prob is not None and y is not None, "moe_combine_bwd: prob and y are required")
    return _moe_rows_call(_lib.load().dimsum_moe_combine_bwd, "moe_combine_bwd", dout, perm, prob=prob, y=y, want_dprob=True)


MOE_ACT_F16S_MAX_WIDTH = 5120      # kF16sMaxHidden of csrc/act_rows.hip: the widest row the image-writing activation pass holds in registers


def _moe_act_call(fn, what, x, bias, row_expert, dh, gated, need_dbias, f16s=False):
    _gpu(x, bias, row_expert, dh)
    _moe_rows(x, what)
    rows, S = x.shape
    _check(not gated or S % 8 == 0, f"{what}: the gated input is (rows, 2 W) with W % 4 == 0")
    W = S // 2 if gated else S
    E = 1
    if bias is not None:
        _check(bias.dtype == torch.float32 and bias.is_contiguous() and bias.dim() == 2 and bias.shape[1] == S and 1 <= bias.shape[0] <= MOE_MAX_EXPERTS,
               f"{what}: bias must be contiguous float32 (E, {S}) with 1 <= E <= {MOE_MAX_EXPERTS}")
        E = bias.shape[0]
    if row_expert is not None:
        _moe_index(row_expert, rows, what, "row_expert")
    _check(row_expert is not None or bias is None or bias.shape[0] == 1, f"{what}: a bias with more than one row needs row_expert")
    if dh is not None:
        _check(dh.dtype == torch.float32 and dh.is_contiguous() and tuple(dh.shape) == (rows, W), f"{what}: dh must be contiguous float32 (rows, W)")
    if f16s:
        out, inv, _ = _act_out((rows,), W, "f16s", x.device)
        P = _lib.MoeActF16sParams()
        P.gated, P.num_experts, P.rows, P.width = int(bool(gated)), E, rows, W
        P.x_ptr, P.bias_ptr, P.row_expert_ptr, P.out_ptr, P.inv_scale_ptr = _ptr(x), _ptr(bias), _ptr(row_expert), _ptr(out), _ptr(inv)
        with torch.cuda.device(x.device):
            _lib.check(fn(P, _stream(x)), what)
        return F16Image(out, inv), None
    out, _, dbias = _act_out((rows,), S if dh is not None else W, False, x.device, bias.numel() if (need_dbias and bias is not None) else 0)
    dbias = dbias.view(bias.shape) if dbias is not None else None
    P = _lib.MoeActParams()
    P.gated, P.num_experts, P.rows, P.width = int(bool(gated)), E, rows, W
    P.x_ptr, P.bias_ptr, P.row_expert_ptr, P.dh_ptr, P.out_ptr, P.dbias_ptr = _ptr(x), _ptr(bias), _ptr(row_expert), _ptr(dh), _ptr(out), _ptr(dbias)
    with torch.cuda.device(x.device):
        _lib.check(fn(P, _stream(x)), what)
    return out, dbias


def moe_act_fwd(x, bias=None, row_expert=None, gated=True, split3=False):
    """x (rows, 2 W | W) = fc1's output WITHOUT bias, bias (E, 2 W | W) or None picked per row by row_expert (int32; None: row 0) ->
    gelu_erf(a + b_a) * (g + b_g) (gated) or gelu_erf(x + b): the exact GELU of the reference's expert MLP (dimsum/mlp.py:30-38)
    split3="f16s": h as the scaled-fp16 image (F16Image, exact row maxima) of the fc2 grouped GEMM -- rows_f16s(moe_act_fwd(...)) bit for bit; the
    pass writes it itself up to W = 5120, wider rows are converted from the fp32 result by rows_f16s"""
    _check(split3 in (False, "f16s"), "moe_act_fwd: split3 is False or 'f16s'")
    W = x.shape[-1] // 2 if gated else x.shape[-1]
    if split3 and W <= MOE_ACT_F16S_MAX_WIDTH:
        return _moe_act_call(_lib.load().dimsum_moe_act_fwd_f16s, "moe_act_fwd", x, bias, row_expert, None, gated, False, f16s=True)[0]
    h = _moe_act_call(_lib.load().dimsum_moe_act_fwd, "moe_act_fwd", x, bias, row_expert, None, gated, False)[0]
    return rows_f16s(h) if split3 else h


def moe_act_bwd(x, bias, row_expert, dh, gated=True, need_dbias=True):
    """-> (dx like x, dbias (E, 2 W | W) or None): the adjoint of moe_act_fwd with the bias gradient summed per expert"""
    _check(dh is not None, "moe_act_bwd: dh is required")
    return _moe_act_call(_lib.load().dimsum_moe_act_bwd, "moe_act_bwd", x, bias, row_expert, dh.contiguous() if dh is not None else None, gated, need_dbias)


def split3_rows(x, left):
    """(R, K) float32 rows (stride(1) == 1) -> (R, 3K) bfloat16 split operand image: x = hi + lo, hi = bf16(x), lo = bf16(x - hi);
    left: [hi | hi | lo] (activations), else [hi | lo | hi] (weights), so that  left_image @ weight_image.T  accumulates
    hi.hi + hi.lo + lo.hi -- the three products of hipBLASLt's fp32-under-allow_tf32 path -- in ONE bf16 GEMM (csrc/operand_split.hip)."""
    _gpu(x)
    _check(x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] % 4 == 0 and x.stride(0) % 4 == 0,
           "split3_rows: x must be (R, K) float32 with contiguous rows, K % 4 == 0 and a row stride % 4 == 0")
    R, K = x.shape
    pair = isinstance(left, str) and left == "pair"          # the pair [hi | lo] (PairImage): the consumer chooses the reading order
    out = torch.empty((R, (2 if pair else 3) * K), device=x.device, dtype=torch.bfloat16)
    if R > 0:
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dimsum_split3(_ptr(x), R, K, x.stride(0), _ptr(out), 2 if pair else int(bool(left)), _stream(x)), "split3_rows")
    return PairImage(out) if pair else out


def split3_rows_t(w):
    """weight (N, K) float32 (rows contiguous) -> (3 K, N) bfloat16: the row stack [hi; lo; hi] of w^T (csrc/operand_split.hip), the right
    operand of gemm_tn(planes, ., alias_rows=K)"""
    _gpu(w)
    _check(w.dim() == 2 and w.dtype == torch.float32 and w.stride(1) == 1 and w.shape[0] % 2 == 0, "split3_rows_t: w must be (N, K) float32 rows, N even")
    N, K = w.shape
    out = torch.empty((3 * K, N), device=w.device, dtype=torch.bfloat16)
    with torch.cuda.device(w.device):
        _lib.check(_lib.load().dimsum_split3_t(_ptr(w), N, K, w.stride(0), _ptr(out), _stream(w)), "split3_rows_t")
    return out


class PairImage:
    """split-bf16 left operand image stored as the PAIR [hi | lo]: data (M, 2K) bfloat16. The GEMM kernel reads it as [hi | hi | lo]
    (a_alias_rows = K: K tiles past the first piece re-read the tiles one piece earlier) -- a third less image traffic than the three-piece
    form the library GEMM needs; .image3() expands it for a consumer without the kernel."""
    __slots__ = ("data",)

    def __init__(self, data):
        self.data = data

    @property
    def k(self):
        return self.data.shape[-1] // 2

    def image3(self):
        K = self.k
        return torch.cat([self.data[..., :K], self.data[..., :K], self.data[..., K:]], dim=-1)

    @property
    def shape(self):
        return self.data.shape

    def reshape(self, *shape):
        return PairImage(self.data.reshape(*shape))

    view = reshape

    def record_stream(self, stream):
        self.data.record_stream(stream)


class F16Image:
    """scaled-fp16 operand image (csrc/common.hpp, f16s): data (..., K) float16 = fp16(x * 2^s), one s per row, inv (...) float32 = 2^-s.
    Quacks like the tensor it replaces where the host layer only reshapes it and hands it to the next GEMM."""
    __slots__ = ("data", "inv")

    def __init__(self, data, inv):
        self.data, self.inv = data, inv

    @property
    def shape(self):
        return self.data.shape

    def reshape(self, *shape):
        d = self.data.reshape(*shape)
        return F16Image(d, self.inv.reshape(d.shape[:-1]))

    view = reshape

    def record_stream(self, stream):
        self.data.record_stream(stream)
        self.inv.record_stream(stream)

    def float(self):
        return self.data.float() * self.inv.unsqueeze(-1)


def rows_f16s(x, want_l1=False):
    """(R, K) float32 rows (stride(1) == 1) -> F16Image [, l1max]: row r = fp16(x_r * 2^s_r) with 2^s_r max|x_r| in [2^14, 2^15) and
    inv[r] = 2^-s_r (csrc/operand_split.hip). want_l1: also max_r sum_k |x_rk| as a 1-element float32 tensor (weights: the bound of
    the gated GEMM epilogue)."""
    _gpu(x)
    _check(x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] % 4 == 0 and x.stride(0) % 4 == 0,
           "rows_f16s: x must be (R, K) float32 with contiguous rows, K % 4 == 0 and a row stride % 4 == 0")
    R, K = x.shape
    out = torch.empty((R, K), device=x.device, dtype=torch.float16)
    inv = torch.empty((R,), device=x.device, dtype=torch.float32)
    l1 = torch.zeros((1,), device=x.device, dtype=torch.float32) if want_l1 else None
    if R > 0:
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dimsum_rows_f16s(_ptr(x), R, K, x.stride(0), _ptr(out), K, _ptr(inv), _ptr(l1), _stream(x)), "rows_f16s")
    img = F16Image(out, inv)
    return (img, l1) if want_l1 else img


def rows_block_f16s(x):
    """(D, M) float32 rows (a d-major activation: channels x tokens; D % 64 == 0, M % 256 == 0) -> (image (D, M) float16, table (M / 32, D / 64) float32):
    every 64 x 32 block as fp16(x 2^s) with 2^-s in the table -- the layout selective_scan_fwd(out_z_f16=True) returns, for launches the state-split scan
    kernels serve (csrc/operand_split.hip, rows_block_f16s_kernel)"""
    _gpu(x)
    _check(x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[0] % 64 == 0 and x.shape[1] % 256 == 0 and x.stride(0) % 4 == 0
           and x.data_ptr() % 16 == 0, "rows_block_f16s: x must be (D % 64, M % 256) float32 rows, 16-byte aligned")
    D, M = x.shape
    img = torch.empty((D, M), device=x.device, dtype=torch.float16)
    table = torch.empty((M // 32, D // 64), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dimsum_rows_block_f16s(_ptr(x), D, M, x.stride(0), _ptr(img), M, _ptr(table), table.stride(0), _stream(x)), "rows_block_f16s")
    return img, table


def rows_f16s_multi(jobs, n_slots=None):
    """ONE launch per 24 jobs (csrc/operand_split.hip, dimsum_rows_f16s_multi). jobs: list of (x, image, l1_slot, absmax_slot, l1_factor):
    x (R, K) float32 rows (or a (K,) vector: one row); image: build the F16Image; l1_slot / absmax_slot: index into the returned float32
    scalar buffer that receives l1_factor * max_r sum_k |x_rk| / max |x| (None: not wanted; several jobs may NOT share a slot's meaning but
    may share a slot: the maximum over them lands there); an optional 6th element (data (R, K) float16, inv (R,) float32) makes the job
    write its image there (e.g. slices of one buffer). -> ([F16Image or None per job], scalars)"""
    if not jobs:
        return [], None
    dev = jobs[0][0].device
    used = 1 + max([-1] + [s_ for j in jobs for s_ in j[2:4] if s_ is not None])
    n_slots = used if n_slots is None else max(int(n_slots), used)        # (a caller that slices the scalars by its own slot layout passes its total)
    scal = torch.zeros(max(n_slots, 1), device=dev, dtype=torch.float32)
    arr = (_lib.F16sJob * len(jobs))()
    images, keep = [], []
    for q, job in zip(arr, jobs):
        x, image, l1_slot, abs_slot, factor = job[:5]
        _gpu(x)
        x2 = x if x.dim() == 2 else x.reshape(1, -1)
        _check(x2.dtype == torch.float32 and x2.dim() == 2 and x2.stride(1) == 1 and x2.shape[1] % 4 == 0 and (x2.shape[0] == 1 or x2.stride(0) % 4 == 0),
               "rows_f16s_multi: operands must be float32 rows with K % 4 == 0 and a row stride % 4 == 0")
        R, K = x2.shape
        q.src, q.rows, q.cols, q.src_row_stride = _ptr(x2), R, K, (x2.stride(0) if R > 1 else K)
        if image:
            if len(job) > 5:
                out, inv = job[5]
                _check(out.shape == (R, K) and out.dtype == torch.float16 and out.is_contiguous() and inv.shape == (R,) and inv.dtype == torch.float32 and inv.is_contiguous(),
                       "rows_f16s_multi: a job's own destination must be a contiguous (R, K) float16 / (R,) float32 pair")
            else:
                out, inv = torch.empty((R, K), device=dev, dtype=torch.float16), torch.empty((R,), device=dev, dtype=torch.float32)
            q.dst, q.inv_scale_ptr, q.dst_row_stride = _ptr(out), _ptr(inv), K
            images.append(F16Image(out, inv))
        else:
            images.append(None)
        if l1_slot is not None:
            q.l1max_ptr = scal.data_ptr() + 4 * l1_slot
        if abs_slot is not None:
            q.absmax_ptr = scal.data_ptr() + 4 * abs_slot
        q.l1_factor = float(factor)
        keep.append(x2)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dimsum_rows_f16s_multi(arr, len(jobs), _stream(jobs[0][0])), "rows_f16s_multi")
    return images, scal


def _gemm_operands_ok(a, b):
    """what every GEMM entry point asks of its two operands: 2-D, the same 16-bit type, rows of unit column stride whose stride is a multiple of
    8 elements, 16-byte aligned"""
    return (a.is_cuda and a.dim() == 2 and b.dim() == 2 and a.dtype == b.dtype and a.dtype in (torch.bfloat16, torch.float16)
            and a.stride(1) == 1 and b.stride(1) == 1 and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0
            and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def _fill_gemm(G, a, b, out, m, n, k, epilogue=_lib.GEMM_EPI_F32, out_scale=1.0, bias=None, scales=(None, None), events=None, **ext):
    """the shape, operand type, epilogue, leading dimensions and pointers of one launch into G (out: rows of the last dimension); scales = the
    (a, b) inverse scales, events = (start, stop) raw hipEvent_t handles, ext = further fields of dimsum_gemm_ext_t -> the attached GemmExt"""
    G.m, G.n, G.k = m, n, k
    G.operand_dtype, G.epilogue, G.out_scale = _DT[a.dtype], epilogue, float(out_scale)
    G.lda, G.ldb, G.ldc = a.stride(0), b.stride(0), out.stride(-2)
    G.a_ptr, G.b_ptr, G.bias_ptr, G.c_ptr = _ptr(a), _ptr(b), _ptr(bias), _ptr(out)
    G.a_inv_scale_ptr, G.b_inv_scale_ptr = _ptr(scales[0]), _ptr(scales[1])
    X = _lib.attach_ext(G, _lib.GemmExt)            # fused-epilogue operands, image read modes, timing, tuning (dimsum_gemm_ext_t)
    if events is not None:
        X.timing_start_event, X.timing_stop_event = events
    for field, value in ext.items():
        setattr(X, field, value)
    return X


def gemm_nt_supported(a, b, gated=False, pair=False, pair_b=False):
    """shapes the hand-written NT GEMM takes (csrc/gemm_nt_kernel.hpp): 256-row panels of 16-bit rows, 64-deep K tiles.
    pair / pair_b (or a PairImage operand): that operand is the [hi | lo] pair (rows of 2C) of a split-bf16 image over K = 3C (C % 64 == 0)"""
    if isinstance(a, PairImage):
        a, pair = a.data, True
    if isinstance(b, PairImage):
        b, pair_b = b.data, True
    if not _gemm_operands_ok(a, b):
        return False
    M, K = a.shape
    N, Kb = b.shape
    if pair:
        if K % 128 != 0 or a.dtype != torch.bfloat16:
            return False
        K = K // 2 * 3
    if pair_b:
        if pair or gated or Kb % 128 != 0 or b.dtype != torch.bfloat16:
            return False
        Kb = Kb // 2 * 3
    return (Kb == K and M > 0 and M % 256 == 0 and K % 64 == 0 and K >= 128 and N % (16 if gated else 4) == 0
            and 512 * max(a.stride(0), b.stride(0)) < 2 ** 31)


def gemm_tn_supported(a, b):
    """shapes the TN variant takes (csrc/gemm_nt_kernel.hpp, kVarTN): a (R, P), b (R, Q) 16-bit rows over the reduction index R, whole
    256 x 256 output tiles, 64-row reduction tiles"""
    if not _gemm_operands_ok(a, b):
        return False
    R, P = a.shape
    Q = b.shape[1]
    # (Q % 256 != 0: b must be a column slice of rows ZERO-PADDED to whole 256-column tiles -- its row stride says so; gemm.weight_f16s_t pads)
    q_ok = Q % 256 == 0 or (Q % 4 == 0 and b.stride(0) >= (Q + 255) // 256 * 256)
    return (b.shape[0] == R and R % 64 == 0 and R >= 128 and P % 256 == 0 and q_ok and P > 0 and Q > 0
            and 128 * max(a.stride(0), b.stride(0)) + 512 < 2 ** 31)


def gemm_tn_splits(R, P, Q, second_round=True):
    """reduction ranges of a TN launch: enough workgroups to fill the 256 CUs when the output has few tiles (a weight gradient (8192, 1024)
    is 128 tiles, (1536, 512) is 12), ranges of whole 64-row tiles, at least 2048 rows each. second_round=False (the single-product fp16
    launches: a third of the three-product kernel's time per range, so the partial results' write + sum weigh three times as much): one
    round of workgroups -- tools/scratch/tn_splits.py: d w12 at 16384 rows 335 -> 297 us, d w3 180 -> 144"""
    tiles = (P // 256) * (Q // 256)
    s = 1
    ok = lambda s2: R % (s2 * 64) == 0 and R // s2 >= 2048
    while tiles * s < 192 and ok(2 * s):         # three quarters of the 256 CUs at least ...
        s *= 2
    if second_round and tiles >= 64 and tiles * s < 512 and ok(2 * s):       # ... and a second round where the partial results are few (tools/scratch/tn_perf.py)
        s *= 2
    return s


def _rowfac_splits(R, P, Q):
    """reduction ranges of a launch with per-reduction-row factors (gemm_tn with row_scales / row_invs, gemm_nn): one round of workgroups, then
    doubled while a range exceeds 16384 rows (the factors of one range live in 32 KB of LDS)"""
    splits = gemm_tn_splits(R, P, Q, second_round=False)
    while R // splits > 16384 and R % (2 * splits * 64) == 0:
        splits *= 2
    return splits


def gemm_tn_pairs(a, b, splits=None):
    """a, b PairImages (M, 2P) / (M, 2Q): dW = a^T b with a read in weight order [hi | lo | hi] and b in left order [hi | hi | lo] (the three
    products of the split-bf16 policy) -> (P, Q) float32. The reduction runs over 3 pieces x `splits` row ranges of M."""
    ad, bd = a.data, b.data
    _gpu(ad, bd)
    M, P2 = ad.shape
    P, Q = P2 // 2, bd.shape[1] // 2
    _check(bd.shape[0] == M and gemm_tn_supported(ad[:, :P], bd[:, :Q]), "gemm_tn_pairs: unsupported operands")
    if splits is None:
        tiles = (P // 256) * (Q // 256)
        # whole rounds of the 256 CUs: 3 x splits x tiles workgroups of equal length (128 tiles x 3 = 384 would be one and a half)
        splits = 1
        while (tiles * 3 * splits) % 256 != 0 and tiles * 3 * splits < 1024 and M % (2 * splits * 64) == 0 and M // (2 * splits) >= 2048:
            splits *= 2
    _check(M % (splits * 64) == 0 and M // splits >= 128, "gemm_tn_pairs: splits must cut M into ranges of whole 64-row tiles")
    out = torch.empty((3 * splits, P, Q), device=ad.device, dtype=torch.float32)
    G = _lib.GemmParams()
    _fill_gemm(G, ad, bd, out, P, Q, M, tn_pair_a_cols=P, tn_pair_b_cols=Q)
    with torch.cuda.device(ad.device):
        _lib.check(_lib.load().dimsum_gemm_tn(G, 3 * splits, P * Q, _stream(ad)), "gemm_tn_pairs")
    return out.sum(0)


def row_factors(a_inv, b_inv=None):
    """(R,) float32 inverse row scales of two scaled-fp16 images whose ROWS are the reduction index of a product a^T b -> (k_fac (R,) float16,
    c_scale (1,) float32): term r carries a_inv[r] b_inv[r]; k_fac = that / its maximum (powers of two <= 1; below 2^-24: 0), c_scale = the
    maximum (include/dimsum_hip.h, dimsum_gemm_ext_t.k_scale_ptr). b_inv None = 1. One small launch (csrc/operand_split.hip)."""
    _gpu(a_inv, b_inv)
    a_inv = a_inv.reshape(-1)
    _check(a_inv.dtype == torch.float32 and a_inv.is_contiguous() and (b_inv is None or (b_inv.dtype == torch.float32 and b_inv.numel() == a_inv.numel())),
           "row_factors: (R,) float32 inverse scales")
    if b_inv is not None:
        b_inv = b_inv.reshape(-1).contiguous()
    fac = torch.empty(a_inv.numel(), device=a_inv.device, dtype=torch.float16)
    top = torch.empty(1, device=a_inv.device, dtype=torch.float32)
    with torch.cuda.device(a_inv.device):
        _lib.check(_lib.load().dimsum_row_factors(_ptr(a_inv), _ptr(b_inv), a_inv.numel(), _ptr(fac), _ptr(top), _stream(a_inv)), "row_factors")
    return fac, top


def gemm_tn(a, b, splits=None, events=None, alias_rows=0, scales=None, row_scales=None, row_invs=None):
    """a (R, P)^T @ b (R, Q) -> (P, Q) float32 on the hand-written MFMA kernel's TN variant: the weight-gradient product of a Linear
    (reduction over the rows). The reduction is cut into `splits` ranges whose partial results are added in a fixed order.
    alias_rows = D: a is a (2 D, P) pair of planes [hi; lo] read as the row stack [hi; hi; lo] (b: (3 D, Q)); one range.
    scales = (a_inv, b_inv (Q,)): float16 operands carrying power-of-two scales (one range): a_inv (P,) -> the result is multiplied by
    a_inv[p] b_inv[q]; a_inv (P / 32, R / 64) -> block-scaled a (the scan's fp16 out_z with its table, selective_scan_fwd(out_z_f16=True)):
    the values of tokens [32 g, 32 g + 32) x reduction rows [64 t, 64 t + 64) stand for value * a_inv[g][t]; R <= 4096 (out_proj of a
    Mamba mixer as ONE fp16 product per element).
    row_scales = (k_fac (R,) float16, c_scale (1,) float32) from row_factors(a_inv, b_inv): both operands are scaled-fp16 images with one scale
    per ROW and the rows are the reduction index (the weight gradient dW = dy^T x of a Linear under the scaled-fp16 policy): a's row r is
    multiplied by k_fac[r] as it is read, the result by c_scale; ranges of at most 16384 rows.
    row_invs = (a_inv (R,), b_inv (R,) or None) float32: the same product with the factors formed INSIDE the kernel from the two images' row scales
    (every workgroup normalises by the maximum of its own range): no row_factors launch in front of the GEMM."""
    _gpu(a, b)
    blocks = None
    if row_invs is not None:
        ia, ib = row_invs
        _gpu(ia, ib)
        _check(row_scales is None and scales is None and not alias_rows and a.dtype == torch.float16 and ia.dtype == torch.float32 and ia.numel() == a.shape[0]
               and ia.is_contiguous() and (ib is None or (ib.dtype == torch.float32 and ib.numel() == a.shape[0] and ib.is_contiguous())),
               "gemm_tn: row_invs = (a_inv (R,), b_inv (R,) or None) float32 with float16 operands")
        if os.environ.get("DIMSUM_ROW_FACTORS_KERNEL", "0") == "1":        # (A / B: the factor table from its own launch, as before)
            row_scales, row_invs = row_factors(ia, ib), None
    if row_scales is not None:
        kf, cs = row_scales
        _gpu(kf, cs)
        _check(scales is None and not alias_rows and a.dtype == torch.float16 and kf.dtype == torch.float16 and kf.numel() == a.shape[0] and kf.is_contiguous()
               and cs.dtype == torch.float32 and cs.numel() == 1, "gemm_tn: row_scales = (k_fac (R,) float16, c_scale (1,) float32) with float16 operands")
    if scales is not None:
        _gpu(*scales)
        sa, sb = scales
        _check(a.dtype == torch.float16 and not alias_rows and sa.dtype == torch.float32 and sb.dtype == torch.float32 and sb.numel() == b.shape[1] and sb.is_contiguous(),
               "gemm_tn: scales = (a_inv, b_inv (Q,)) float32 with float16 operands")
        if sa.dim() == 2:
            _check(sa.shape[0] == a.shape[1] // 32 and sa.shape[1] >= a.shape[0] // 64 and sa.stride(1) == 1 and a.shape[0] <= 4096 and a.shape[1] % 32 == 0,
                   "gemm_tn: a block table must be (P / 32, R / 64) float32, R <= 4096")
            blocks = sa
        else:
            _check(sa.numel() == a.shape[1] and sa.is_contiguous(), "gemm_tn: a_inv must be (P,)")
        splits = 1
    if alias_rows:
        _check(a.dim() == 2 and a.shape[0] == 2 * alias_rows and b.shape[0] == 3 * alias_rows and alias_rows % 64 == 0 and gemm_tn_supported(a[:alias_rows], b[:alias_rows]),
               "gemm_tn: alias_rows = D takes a (2 D, P) plane pair and a (3 D, Q) row stack, D % 64 == 0")
        R, P = 3 * alias_rows, a.shape[1]
        splits = 1
    else:
        _check(gemm_tn_supported(a, b), "gemm_tn: unsupported operands (R % 64, P % 256, Q % 256, 16-bit rows, 16-byte aligned)")
        R, P = a.shape
    Q = b.shape[1]
    rowfac = row_scales is not None or row_invs is not None
    if splits is None:
        splits = _rowfac_splits(R, P, Q) if rowfac else gemm_tn_splits(R, P, Q)
    if rowfac:
        _check(R // splits <= 16384, "gemm_tn: row factors need ranges of at most 16384 reduction rows")
    _check(splits >= 1 and R % (splits * 64) == 0 and R // splits >= 128, "gemm_tn: splits must cut R into ranges of whole 64-row tiles (>= 2)")
    out = torch.empty((splits, P, Q), device=a.device, dtype=torch.float32)
    ext = dict(a_alias_rows=alias_rows)
    if blocks is not None:
        ext.update(a_block_inv_ptr=_ptr(blocks), a_block_inv_ld=blocks.stride(0))
        scales = (None, scales[1])
    if row_scales is not None:
        ext.update(k_scale_ptr=_ptr(row_scales[0]), c_scale_ptr=_ptr(row_scales[1]))
    if row_invs is not None:
        ext.update(k_inv_a_ptr=_ptr(row_invs[0]), k_inv_b_ptr=_ptr(row_invs[1]))
    G = _lib.GemmParams()
    _fill_gemm(G, a, b, out, P, Q, R, scales=scales or (None, None), events=events, **ext)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().dimsum_gemm_tn(G, splits, P * Q, _stream(a)), "gemm_tn")
    return out[0] if splits == 1 else out.sum(0)


_gemm_kernel_log = None      # a list while gemm_kernel_log() is open: (epilogue, dimsum_gemm_nt_kernel_for) of every gemm_nt call


@contextlib.contextmanager
def gemm_kernel_log():
    """tests / measurement: records, for every gemm_nt call made inside, which kernel family the library launches (_lib.GEMM_NT_KERNELS:
    0 = 256-row tiles, 1 = 128-row tiles, 2 = the persistent K-tile stream). Host-side, not thread-safe."""
    global _gemm_kernel_log
    old, _gemm_kernel_log = _gemm_kernel_log, []
    try:
        yield _gemm_kernel_log
    finally:
        _gemm_kernel_log = old


def gemm_nn_supported(a, b):
    """shapes dimsum_gemm_nn takes: a (P, R) float16 rows contiguous along the reduction, b (R, Q) float16 rows over it; whole 256 x 256 output
    tiles, whole 64-row reduction tiles"""
    if not (_gemm_operands_ok(a, b) and a.dtype == torch.float16):
        return False
    P, R = a.shape
    Q = b.shape[1]
    return (b.shape[0] == R and R % 64 == 0 and R >= 128 and P % 256 == 0 and Q % 256 == 0
            and 256 * a.stride(0) * 2 < 2 ** 31 and 64 * b.stride(0) * 2 + 512 < 2 ** 31)


def gemm_nn(a, a_inv, b, b_inv, splits=None):
    """a (P, R) @ b (R, Q) -> (P, Q) float32 from two scaled-fp16 images: a = fp16 rows with one scale per row (a_inv (P,): its rows are OUTPUT rows --
    a d-major activation, channels x tokens), b = fp16 rows with one scale per row (b_inv (R,): its rows are the REDUCTION index -- a token-major
    activation): the weight gradients of the Mamba projections (d in_proj.weight = dxz x, d out_proj.weight^T = out_z dout) as ONE fp16 product
    per element. b's scales travel as per-reduction-row factors (row_factors with a constant partner)."""
    _gpu(a, a_inv, b, b_inv)
    _check(gemm_nn_supported(a, b) and a_inv.dtype == torch.float32 and a_inv.numel() == a.shape[0] and a_inv.is_contiguous()
           and b_inv.dtype == torch.float32 and b_inv.numel() == b.shape[0], "gemm_nn: unsupported operands")
    P, R = a.shape
    Q = b.shape[1]
    if splits is None:
        splits = _rowfac_splits(R, P, Q)
    _check(splits >= 1 and R % (splits * 64) == 0 and 128 <= R // splits <= 16384, "gemm_nn: splits must cut R into ranges of 2 .. 256 whole 64-row tiles")
    in_kernel = os.environ.get("DIMSUM_ROW_FACTORS_KERNEL", "0") != "1" and b_inv.is_contiguous()       # factors formed inside the GEMM (no launch in front)
    fac, top = (None, None) if in_kernel else row_factors(b_inv)
    out = torch.empty((splits, P, Q), device=a.device, dtype=torch.float32)
    G = _lib.GemmParams()
    _fill_gemm(G, a, b, out, P, Q, R, scales=(a_inv, None), **(dict(k_inv_a_ptr=_ptr(b_inv)) if in_kernel else dict(k_scale_ptr=_ptr(fac), c_scale_ptr=_ptr(top))))
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().dimsum_gemm_nn(G, splits, P * Q, _stream(a)), "gemm_nn")
    return out[0] if splits == 1 else out.sum(0)


def gemm_nt(a, b, bias=None, epilogue="f32", out=None, out_scale=1.0, events=None, tune=None, scales=None, gate_bound=None, residual=None,
            gate=None, rows_per_batch=None, keep_x12=False, pair_out=False, weight_order=False, q_cols=None, conv=None):
    """a (M, K) @ b (N, K)^T on the hand-written MFMA kernel, 16-bit operands (bfloat16: split-bf16 images over 3 K; float16: scaled rows),
    fp32 accumulation.
      epilogue "f32"          -> (M, N) float32 (+ bias[N])
               "gated_split3" -> b = the (2F, K) w12 weight image, bias (2F) or None: the LEFT split-bf16 image (M, 3F) bfloat16 of
                                 gelu_tanh(x1 + b1) * (x2 + b2)   (mlp.py:66-70; the fp32 (M, 2F) x12 never exists)
                                 keep_x12 (training forward): the bias-free float32 (M, 2F) [x1 | x2] is stored too -> (image, x12)
               "gated_f16"    -> same, (M, F) float16 of h * out_scale
               "gelu_f16"     -> F16Image (M, N) of gelu_tanh(a b^T + bias): fc1 of the plain MLP over scaled-fp16 operands (scales and gate_bound
                                 = {wl1, bmax} required: the row scale is derived from the bound); bfloat16 operands are refused by the library
    residual (M, N) float32 [, gate (M / rows_per_batch, N) float32]: epilogue "f32" becomes residual + gate[row // rows_per_batch] * (a b^T + bias)
    -- the residual tail of a block in the epilogue of its last Linear (rows_per_batch % 256 == 0).
    scales: (a_inv (M,), b_inv (N,)) float32 inverse scales of scaled-fp16 operand images (F16Image): C[m, n] *= a_inv[m] * b_inv[n].
    gate_bound ("gated_f16" over scaled operands): 2-element float32 device tensor {max_n sum_k |w_nk|, max |bias|}: the h image gets a
    per-row power-of-two scale derived from it and the call returns (h16, h_inv).
    events: optional (start, stop) raw hipEvent_t handles recorded at the kernel's dispatch boundaries (bench.py)."""
    pair_in = isinstance(a, PairImage)         # a: the pair [hi | lo] of a left image, read as [hi | hi | lo]
    pair_b = isinstance(b, PairImage)          # b: the same on the right (in_proj: weight image x activation pair -> d-major output)
    if pair_in:
        a = a.data
    if pair_b:
        b = b.data
    _gpu(a, b, bias)
    gated = epilogue in ("gated_split3", "gated_f16")
    _check(not (pair_in and pair_b) and not (pair_b and (gated or residual is not None or bias is not None)), "gemm_nt: a right-hand pair goes with the plain fp32 epilogue")
    _check(gemm_nt_supported(a, b, gated, pair=pair_in, pair_b=pair_b), "gemm_nt: unsupported operands (M % 256, K % 64, K >= 128, 16-bit K-contiguous rows, 16-byte aligned)")
    M, K = a.shape[0], (a.shape[1] if pair_b else b.shape[1])
    N = b.shape[0]
    ext = {}                                        # fields of dimsum_gemm_ext_t beyond the zeros
    if pair_in:
        ext.update(a_alias_rows=K // 3, a_alias_weight_order=int(bool(weight_order)))      # weight order: the pair read as [hi | lo | hi] (a gradient image x a left-order weight image)
    if pair_b:
        ext.update(b_alias_rows=K // 3)
    if bias is not None:
        _check(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N, "gemm_nt: bias must be (N,) float32")
    if epilogue == "f32":
        epi = _lib.GEMM_EPI_F32 if bias is None else _lib.GEMM_EPI_F32_BIAS
        if out is None:
            out = torch.empty((M, N), device=a.device, dtype=torch.float32)
        _check(out.dtype == torch.float32 and out.shape == (M, N) and out.stride(1) == 1, "gemm_nt: out must be (M, N) float32 rows")
        if conv is not None:
            # conv = (weight (rows, width) f32, bias (rows) f32 or None, seq): rows [0, rows) of the d-major product get the causal conv1d + SiLU
            # along their columns (sequences of `seq` columns) in the epilogue -- in_proj + causal_conv1d_fn of a Mamba mixer in one kernel
            cw, cb, seq = conv
            _gpu(cw, cb)
            _check(bias is None and residual is None and cw.dtype == torch.float32 and cw.dim() == 2 and cw.stride(1) == 1 and cw.shape[0] % 256 == 0
                   and cw.shape[0] <= M and 2 <= cw.shape[1] <= 4 and 256 % seq == 0 and seq % 4 == 0 and N % seq == 0
                   and (cb is None or (cb.dtype == torch.float32 and cb.is_contiguous() and cb.numel() == cw.shape[0])),
                   "gemm_nt: conv = (weight (rows % 256 == 0, width 2..4) f32, bias or None, seq with 256 % seq == 0)")
            epi = _lib.GEMM_EPI_F32_CONV
            ext.update(conv_weight_ptr=_ptr(cw), conv_bias_ptr=_ptr(cb), conv_rows=cw.shape[0], conv_width=cw.shape[1], conv_seq=seq, conv_weight_ld=cw.stride(0))
        if residual is not None:
            _gpu(residual, gate)
            _check(residual.dtype == torch.float32 and residual.shape == (M, N) and residual.stride(1) == 1, "gemm_nt: residual must be (M, N) float32 rows")
            epi = _lib.GEMM_EPI_F32_GATE_RESIDUAL
            ext.update(residual_ptr=_ptr(residual), residual_ld=residual.stride(0))
            if gate is not None:
                _check(rows_per_batch and rows_per_batch % 256 == 0 and M % rows_per_batch == 0 and gate.dtype == torch.float32
                       and gate.shape == (M // rows_per_batch, N) and gate.stride(1) == 1, "gemm_nt: gate must be (M / rows_per_batch, N) float32, rows_per_batch % 256 == 0")
                ext.update(gate_ptr=_ptr(gate), gate_ld=gate.stride(0), rows_per_batch=rows_per_batch)
    elif epilogue == "gated_split3":
        epi = _lib.GEMM_EPI_GATED_GELU_SPLIT3
        pieces = 2 if pair_out else 3
        ext.update(c_image_pieces=pieces)
        if out is None:
            out = torch.empty((M, pieces * (N // 2)), device=a.device, dtype=torch.bfloat16)
        _check(out.dtype == torch.bfloat16 and out.shape == (M, pieces * (N // 2)) and out.stride(1) == 1, "gemm_nt: out must be (M, 3F) / (M, 2F) bfloat16 rows")
    elif epilogue == "f16_qkv":
        # the qkv Linear of the attention fusion as scaled fp16 (include/dimsum_hip.h, DIMSUM_GEMM_EPI_F16_QKV): q_cols = the width of q
        epi = _lib.GEMM_EPI_F16_QKV
        _check(scales is not None and gate_bound is not None and rows_per_batch and rows_per_batch % 256 == 0 and M % rows_per_batch == 0
               and q_cols and q_cols % 16 == 0 and N % 8 == 0, "gemm_nt: f16_qkv needs scales, gate_bound = {wl1, bmax}, rows_per_batch % 256 == 0, q_cols % 16 == 0")
        ext.update(rows_per_batch=rows_per_batch, qkv_q_cols=q_cols)
        if out is None:
            out = torch.empty((M, N), device=a.device, dtype=torch.float16)
        _check(out.dtype == torch.float16 and out.shape == (M, N) and out.stride(1) == 1, "gemm_nt: out must be (M, N) float16 rows")
    elif epilogue == "gelu_f16":
        epi = _lib.GEMM_EPI_GELU_F16
        _check(scales is not None and gate_bound is not None and N % 8 == 0, "gemm_nt: gelu_f16 needs scales, gate_bound = {wl1, bmax} and N % 8 == 0")
        if out is None:
            out = torch.empty((M, N), device=a.device, dtype=torch.float16)
        _check(out.dtype == torch.float16 and out.shape == (M, N) and out.stride(1) == 1, "gemm_nt: out must be (M, N) float16 rows")
    elif epilogue == "gated_f16":
        epi = _lib.GEMM_EPI_GATED_GELU_F16
        if out is None:
            out = torch.empty((M, N // 2), device=a.device, dtype=torch.float16)
        _check(out.dtype == torch.float16 and out.shape == (M, N // 2) and out.stride(1) == 1, "gemm_nt: out must be (M, F) float16 rows")
    else:
        raise ValueError(f"gemm_nt: unknown epilogue {epilogue!r}")
    h_inv = None
    if scales is not None:
        sa, sb = scales
        _gpu(sa, sb)
        _check(sa.dtype == torch.float32 and sb.dtype == torch.float32 and sa.is_contiguous() and sb.is_contiguous() and sa.numel() == M
               and sb.numel() == N, "gemm_nt: scales must be contiguous float32 (M,) and (N,)")
        if gate_bound is not None:
            _gpu(gate_bound)
            _check(epilogue in ("gated_f16", "f16_qkv", "gelu_f16") and gate_bound.dtype == torch.float32 and gate_bound.numel() == 2 and gate_bound.is_contiguous(),
                   "gemm_nt: gate_bound is a 2-element float32 tensor for the gated_f16 / f16_qkv / gelu_f16 epilogues")
            ext.update(gate_bound_ptr=_ptr(gate_bound))
            if epilogue in ("gated_f16", "gelu_f16"):
                h_inv = torch.empty((M,), device=a.device, dtype=torch.float32)
                ext.update(h_inv_scale_ptr=_ptr(h_inv))
    x12 = None
    if keep_x12:
        _check((epilogue == "gated_split3" and a.dtype == torch.bfloat16 and scales is None) or (epilogue == "gated_f16" and a.dtype == torch.float16 and h_inv is not None),
               "gemm_nt: keep_x12 goes with the gated_split3 epilogue over bf16 images or the gated_f16 epilogue over scaled-fp16 operands with gate_bound")
        x12 = torch.empty((M, N), device=a.device, dtype=torch.float32)
        ext.update(x12_ptr=_ptr(x12), x12_ld=N)
    if tune is not None:
        ext.update(tune_variant=tune[0], tune_group_m=tune[1], tune_reserved=tune[2] if len(tune) > 2 else 0)
    elif epilogue == "gated_f16" and os.environ.get("DIMSUM_GEMM_PERSIST", "1") == "0":
        ext.update(tune_variant=513)  # A / B switch: the gated GEMM one workgroup per tile instead of the persistent stream (csrc/gemm_nt_kernel.hpp, kVarPersist)
    P = _lib.GemmParams()
    _fill_gemm(P, a, b, out, M, N, K, epi, out_scale, bias=bias, scales=scales or (None, None), events=events, **ext)
    with torch.cuda.device(a.device):
        if _gemm_kernel_log is not None:            # tests / bench: which kernel family the library picks for this call
            _gemm_kernel_log.append((epilogue if conv is None else "f32_conv", int(_lib.load().dimsum_gemm_nt_kernel_for(P))))
        _lib.check(_lib.load().dimsum_gemm_nt(P, _stream(a)), "gemm_nt")
    if x12 is not None:
        if h_inv is not None:
            return F16Image(out, h_inv), x12
        return (PairImage(out) if pair_out else out), x12
    if pair_out:
        return PairImage(out)
    return out if h_inv is None else F16Image(out, h_inv)


# ---------------------------------------------------------------------------------------------------------------------
# cross-attention fusion core (csrc/xattn_fusion.hip)
# ---------------------------------------------------------------------------------------------------------------------
def xattn_supported(qkv, head_dim):
    """the MFMA kernel is instantiated for the head sizes of the DiM zoo: 24 (S/2), 48 (B/2), 64 (L/*), 72 (XL/2), and 32"""
    return qkv.is_cuda and qkv.dtype == torch.float32 and qkv.stride(-1) == 1 and head_dim in (24, 32, 48, 64, 72)


def xattn_fusion_fwd(qkv1, qkv2, heads, need_lse=False, bias1=None, bias2=None, split_bf16=None, split3=False, f16s=None):
    """qkv*: (B, L, 3*heads*hd) -> (B, L, 2*heads*hd) = cat(softmax(q1 k2^T/sqrt(hd)) v2, softmax(q2 k1^T/sqrt(hd)) v1).
    qkv2 = None: plain self-attention softmax(q1 k1^T/sqrt(hd)) v1 -> (B, L, heads*hd).
    bias1/bias2 (3*heads*hd): the qkv Linear biases when qkv* are bias-free GEMM outputs (added inside the kernel).
    split_bf16: None follows torch.backends.cuda.matmul.allow_tf32 (the reference's GEMM policy, train.py:20-21: the
    QK^T / PV contractions then run as split-bf16 MFMA like the library GEMMs do); False = exact fp32 MFMA.
    split3 (split-bf16 kernel only): the result as the split-bf16 left operand image (B, L, 3 * width) bfloat16 of the proj Linear.
    f16s = (x1_inv, x2_inv or None, kv_bound): the single-product fp16 kernel (csrc/xattn_fusion_f16.hip, the "f16s" GEMM policy):
    x*_inv (B, L) are the inverse row scales of the scaled-fp16 images the qkv GEMMs consumed, kv_bound a 4-element float32 tensor
    {max_n sum_c |W1_nc|, max|bias1|, the same for qkv2}; with split3="f16s" the result is the scaled-fp16 image (F16Image) of proj."""
    self_attn = qkv2 is None
    if split_bf16 is None:
        split_bf16 = bool(torch.backends.cuda.matmul.allow_tf32)
    _gpu(qkv1, qkv2, bias1, bias2)
    _check(self_attn or (bias1 is None) == (bias2 is None), "xattn_fusion: pass both biases or none")
    for bb in (bias1, bias2):
        if bb is not None:
            _check(bb.dtype == torch.float32 and bb.numel() == qkv1.shape[2] and bb.is_contiguous(), "xattn_fusion: bad bias")
    B, L, W = qkv1.shape
    hd = W // (3 * heads)
    qkv_f16 = qkv1.dtype == torch.float16          # the F16_QKV epilogue's output (gemm_nt(epilogue="f16_qkv")): the fp16 kernel's own scaling
    _check((qkv1.dtype == torch.float32 or (qkv_f16 and f16s is not None and bias1 is None and bias2 is None)) and qkv1.stride(2) == 1, "xattn_fusion: bad qkv")
    if not self_attn:
        _check(qkv1.shape == qkv2.shape and qkv2.dtype == qkv1.dtype and qkv1.stride() == qkv2.stride(), "xattn_fusion: qkv1/qkv2 must share shape, dtype and strides")
    nd = 1 if self_attn else 2
    out_inv = None
    if f16s is not None:
        x1_inv, x2_inv, kv_bound = f16s
        _gpu(x1_inv, x2_inv, kv_bound)
        _check(x1_inv.dtype == torch.float32 and x1_inv.numel() == B * L and x1_inv.is_contiguous()
               and (self_attn or (x2_inv is not None and x2_inv.dtype == torch.float32 and x2_inv.numel() == B * L and x2_inv.is_contiguous()))
               and kv_bound.dtype == torch.float32 and kv_bound.numel() == 4 and kv_bound.is_contiguous(), "xattn_fusion: bad f16s arguments")
        _check(split3 in (False, "f16s"), "xattn_fusion: the fp16 kernel writes fp32 or the scaled-fp16 image")
    if split3 == "f16s":
        _check(f16s is not None and (heads * hd) % 8 == 0, "xattn_fusion: the scaled-fp16 image needs the fp16 kernel")
        out = torch.empty((B, L, nd * heads * hd), device=qkv1.device, dtype=torch.float16)
        out_inv = torch.empty((B, L), device=qkv1.device, dtype=torch.float32)
    elif split3:
        _check(split_bf16, "xattn_fusion: the operand image output exists for the split-bf16 kernel only")
        out = torch.empty((B, L, (2 if split3 == "pair" else 3) * nd * heads * hd), device=qkv1.device, dtype=torch.bfloat16)
    else:
        out = torch.empty((B, L, nd * heads * hd), device=qkv1.device, dtype=torch.float32)
    lse = torch.empty((B, nd, heads, L), device=qkv1.device, dtype=torch.float32) if need_lse else None
    if B > 0:
        P = _lib.XattnParams()
        P.batch, P.seqlen, P.heads, P.head_dim, P.scale, P.n_dirs = B, L, heads, hd, hd ** -0.5, nd
        P.qkv_batch_stride, P.qkv_token_stride = qkv1.stride(0), qkv1.stride(1)
        P.out_batch_stride, P.out_token_stride = out.stride(0), out.stride(1)
        P.qkv1_ptr, P.qkv2_ptr, P.out_ptr, P.lse_ptr = _ptr(qkv1), _ptr(qkv2), _ptr(out), _ptr(lse)
        P.bias1_ptr, P.bias2_ptr = _ptr(bias1), _ptr(bias2)
        P.precision = 1 if split_bf16 else 0
        P.out_split3 = _SPLIT_MODE.get(split3, int(bool(split3)))
        if f16s is not None:
            P.precision = 2
            P.qkv_f16 = int(qkv_f16)
            P.x1_inv_ptr, P.x2_inv_ptr, P.kv_bound_ptr, P.out_inv_ptr = _ptr(x1_inv), _ptr(x2_inv), _ptr(kv_bound), _ptr(out_inv)
        with torch.cuda.device(qkv1.device):
            _lib.check(_lib.load().dimsum_xattn_fusion_fwd(P, _stream(qkv1)), "xattn_fusion_fwd")
    if out_inv is not None:
        out = F16Image(out, out_inv)
    elif split3 == "pair":
        out = PairImage(out)
    return (out, lse) if need_lse else out


def xattn_fusion_bwd(qkv1, qkv2, out, lse, dout, heads, bias1=None, bias2=None, split_bf16=None, f16=False):
    """backward of xattn_fusion_fwd -> (dqkv1, dqkv2), each (B, L, 3*heads*hd); `out`, `lse` are the forward's results.
    qkv2 = None (self-attention): -> (dqkv1, None).
    f16: ONE fp16 MFMA product per element (precision 2: the TF32-equivalent carrier of the "f16s" policy; dout rows scaled by exact powers of
    two inside the kernels, csrc/xattn_fusion_bwd.hip) instead of the three split-bf16 products."""
    self_attn = qkv2 is None
    _gpu(qkv1, qkv2, out, lse, dout, bias1, bias2)
    B, L, W = qkv1.shape
    hd = W // (3 * heads)
    nd = 1 if self_attn else 2
    _check(qkv1.dtype == torch.float32 and qkv1.stride(2) == 1, "xattn_fusion_bwd: bad qkv")
    if not self_attn:
        _check(qkv1.shape == qkv2.shape and qkv1.stride() == qkv2.stride(), "xattn_fusion_bwd: bad qkv2")
    _check(tuple(out.shape) == (B, L, nd * heads * hd) and out.stride(2) == 1 and tuple(lse.shape) == (B, nd, heads, L) and lse.is_contiguous(), "xattn_fusion_bwd: bad out / lse")
    if dout.stride() != out.stride():
        dout, out = dout.contiguous(), out.contiguous()
    _check(self_attn or (bias1 is None) == (bias2 is None), "xattn_fusion_bwd: pass both biases or none")
    dqkv1 = torch.empty((B, L, W), device=qkv1.device, dtype=torch.float32)
    dqkv2 = None if self_attn else torch.empty((B, L, W), device=qkv1.device, dtype=torch.float32)
    delta = torch.empty((2 if f16 else 1, B, nd, heads, L), device=qkv1.device, dtype=torch.float32)      # D rows (+ the dout row scales, f16)
    if B > 0:
        Q = _lib.XattnBwdParams()
        P = Q.fwd
        P.batch, P.seqlen, P.heads, P.head_dim, P.scale, P.n_dirs = B, L, heads, hd, hd ** -0.5, nd
        P.qkv_batch_stride, P.qkv_token_stride = qkv1.stride(0), qkv1.stride(1)
        P.out_batch_stride, P.out_token_stride = out.stride(0), out.stride(1)
        P.qkv1_ptr, P.qkv2_ptr, P.out_ptr, P.lse_ptr = _ptr(qkv1), _ptr(qkv2), _ptr(out), _ptr(lse)
        P.bias1_ptr, P.bias2_ptr = _ptr(bias1), _ptr(bias2)
        if split_bf16 is None:                    # same policy switch as the forward and the library GEMMs
            split_bf16 = bool(torch.backends.cuda.matmul.allow_tf32)
        P.precision = 2 if f16 else (1 if split_bf16 else 0)
        Q.dqkv_batch_stride, Q.dqkv_token_stride = dqkv1.stride(0), dqkv1.stride(1)
        Q.dout_ptr, Q.dqkv1_ptr, Q.dqkv2_ptr, Q.delta_ptr = _ptr(dout), _ptr(dqkv1), _ptr(dqkv2), _ptr(delta)
        with torch.cuda.device(qkv1.device):
            _lib.check(_lib.load().dimsum_xattn_fusion_bwd(Q, _stream(qkv1)), "xattn_fusion_bwd")
    return dqkv1, dqkv2


# ---------------------------------------------------------------------------------------------------------------------
# the tail of a training step: clip_grad_norm_ + AdamW.step + update_ema over a tensor list (dimsum_optim_*; dimsum_amd/optim.py is the user)
# ---------------------------------------------------------------------------------------------------------------------
def optim_tables(numels, device):
    """the part of the device tables that depends on the tensor sizes only -> (numel int64 (n), chunk table int32 (n_chunks, 2)): one row
    (tensor, chunk number within the tensor) per DIMSUM_OPTIM_CHUNK elements, in list order"""
    _check(len(numels) > 0 and all(int(n) > 0 for n in numels), "optim_tables: a non-empty list of non-empty tensors is required")
    n = torch.tensor([int(v) for v in numels], dtype=torch.int64)
    per = (n + _lib.OPTIM_CHUNK - 1) // _lib.OPTIM_CHUNK
    _check(int(per.sum()) < 2 ** 31 and int(per.max()) < 2 ** 31, "optim_tables: too many chunks for int32 indices")
    tensor = torch.repeat_interleave(torch.arange(len(numels), dtype=torch.int64), per)
    first = torch.cumsum(per, 0) - per
    chunk = torch.arange(int(per.sum()), dtype=torch.int64) - first[tensor]
    return n.to(device), torch.stack([tensor, chunk], 1).to(torch.int32).contiguous().to(device)


def optim_write_ptrs(table, first, ptrs):
    """table[first + i] = ptrs[i] (device int64 tensor <- host integers), ordered on the current stream: the values travel as kernel arguments, so
    there is no staging buffer to overwrite too early and no synchronisation"""
    _gpu(table)
    _check(table.dtype == torch.int64 and table.is_contiguous() and 0 <= first and first + len(ptrs) <= table.numel(),
           "optim_write_ptrs: the table is a contiguous int64 tensor that holds [first, first + len(ptrs))")
    if not ptrs:
        return
    lib = _lib.load()
    arr = (_lib.vp * len(ptrs))(*ptrs)
    with torch.cuda.device(table.device):
        _lib.check(lib.dimsum_optim_write_ptrs(table.data_ptr(), first, arr, len(ptrs), _stream(table)), "dimsum_optim_write_ptrs")


def optim_grad_sumsq(P, device):
    """dimsum_optim_grad_sumsq on the current stream of `device`; P: a filled _lib.OptimParams"""
    with torch.cuda.device(device):
        _lib.check(_lib.load().dimsum_optim_grad_sumsq(P, torch.cuda.current_stream(device).cuda_stream), "dimsum_optim_grad_sumsq")


def optim_adamw_ema_step(P, device):
    """dimsum_optim_adamw_ema_step on the current stream of `device`"""
    with torch.cuda.device(device):
        _lib.check(_lib.load().dimsum_optim_adamw_ema_step(P, torch.cuda.current_stream(device).cuda_stream), "dimsum_optim_adamw_ema_step")


# ---------------------------------------------------------------------------------------------------------------------
# the head of a training step: x_t / u_t of the interpolation plan (optionally with the DCT blur of x1) and the per-sample loss with its
# gradient (dimsum_fm_*; dimsum_amd/transport is the user)
# ---------------------------------------------------------------------------------------------------------------------
FM_PATCHES = (2, 4, 8)        # the tile sizes fm_plan's blur has an instantiation for


def _fm_f32(what, *ts):
    for t in ts:
        if t is not None:
            _check(t.dtype == torch.float32 and t.is_contiguous(), f"{what}: contiguous float32 tensors are required")


def fm_plan(x1, x0, coef, patch=0, min_scale=1e-3, need_ut=True):
    """-> (xt, ut): xt = alpha_b B(x1) + sigma_b x0, ut = d_alpha_b x1 + d_sigma_b x0 in ONE launch. coef: (5, B) rows alpha, sigma, d_alpha,
    d_sigma, blur_t = blur_sigma^2 / 2. patch 0: B is the identity; patch in FM_PATCHES: the per-tile DCT blur (ut still takes the unblurred x1).
    x1: (B, C, H, W), its three inner dimensions contiguous (a batch-strided view is read in place). x0 None: the sigma terms are left out.
    need_ut False: -> (xt, None)."""
    _gpu(x1, x0, coef)
    _check(x1.dim() == 4 and x1.dtype == torch.float32, "fm_plan: x1 is a float32 (B, C, H, W) tensor")
    B, C, H, W = x1.shape
    _check(patch == 0 or patch in FM_PATCHES, f"fm_plan: no kernel for patch size {patch} (the blur is instantiated for {FM_PATCHES}; 0 = no blur)")
    _check(B > 0 and C * H * W > 0, "fm_plan: empty tensors are not supported")
    align = 0 if patch == 0 else 8 if patch == 2 else 16      # the blur reads whole rows of a tile as one vector; without blur any address works
    if x1.stride()[1:] != (H * W, W, 1) or (align and (x1.data_ptr() % align or (B > 1 and x1.stride(0) * 4 % align))):
        x1 = x1.clone(memory_format=torch.contiguous_format)
    _fm_f32("fm_plan", x0, coef)
    _check(x0 is None or x0.shape == x1.shape, "fm_plan: x0 has the shape of x1")
    _check(tuple(coef.shape) == (5, B), "fm_plan: the coefficient table is (5, B)")
    xt = torch.empty((B, C, H, W), dtype=torch.float32, device=x1.device)
    ut = torch.empty_like(xt) if need_ut else None
    P = _lib.FmPlanParams()
    P.batch, P.channels, P.height, P.width, P.patch, P.min_scale = B, C, H, W, patch, min_scale
    P.x1_batch_stride = x1.stride(0) if B > 1 else C * H * W
    P.x1, P.x0, P.coef, P.xt, P.ut = x1.data_ptr(), _ptr(x0), coef.data_ptr(), xt.data_ptr(), _ptr(ut)
    with torch.cuda.device(x1.device):
        _lib.check(_lib.load().dimsum_fm_plan(P, _stream(x1)), "dimsum_fm_plan")
    return xt, ut


def _fm_loss_params(what, out, tgt, w, c, sign):
    _gpu(out, tgt, w, c)
    _fm_f32(what, out, tgt, w, c)
    B = out.shape[0]
    _check(out.dim() >= 2 and out.shape == tgt.shape and out.numel() > 0, f"{what}: out and tgt are (B, ...) tensors of one shape")
    _check(all(v is None or tuple(v.shape) == (B,) for v in (w, c)), f"{what}: w and c are (B,) tensors (or None = 1)")
    _check(sign in (1, -1), f"{what}: sign is +1 or -1")
    P = _lib.FmLossParams()
    P.batch, P.n, P.sign = B, out.numel() // B, sign
    P.out, P.tgt, P.w, P.c = out.data_ptr(), tgt.data_ptr(), _ptr(w), _ptr(c)
    return P


def fm_loss_fwd(out, tgt, w=None, c=None, sign=-1):
    """-> loss (B,): loss_b = w_b mean_i (c_b out_i + sign tgt_i)^2, one fixed summation order (two launches on equal inputs are bit-equal)"""
    P = _fm_loss_params("fm_loss_fwd", out, tgt, w, c, sign)
    loss = torch.empty(out.shape[0], dtype=torch.float32, device=out.device)
    P.loss = loss.data_ptr()
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().dimsum_fm_loss_fwd(P, _stream(out)), "dimsum_fm_loss_fwd")
    return loss


def fm_loss_bwd(gloss, out, tgt, w=None, c=None, sign=-1):
    """-> d loss / d out (shape of out): gloss_b 2 w_b c_b (c_b out + sign tgt) / n"""
    P = _fm_loss_params("fm_loss_bwd", out, tgt, w, c, sign)
    _gpu(gloss)
    _fm_f32("fm_loss_bwd", gloss)
    _check(tuple(gloss.shape) == (out.shape[0],), "fm_loss_bwd: gloss is (B,)")
    dout = torch.empty_like(out)
    P.gloss, P.dout = gloss.data_ptr(), dout.data_ptr()
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().dimsum_fm_loss_bwd(P, _stream(out)), "dimsum_fm_loss_bwd")
    return dout


# ---------------------------------------------------------------------------------------------------------------------
# the rope and cpe positional encodings of the embed pass (dimsum_pos_*; dimsum_amd/ops/pos_embed.py is the user)
# ---------------------------------------------------------------------------------------------------------------------
CPE_MAX_CHANNELS = 2048       # one lane per 4 channels, workgroups of up to 512 lanes


def _pos_tokens(what, x):
    """x as the (B, L, C) float32 tensor the positional passes read: channels contiguous, 16-byte aligned rows"""
    _check(x.dim() == 3 and x.dtype == torch.float32, f"{what}: x is a float32 (B, L, C) tensor")
    B, L, C = x.shape
    _check(B > 0 and L > 0, f"{what}: empty tensors are not supported")
    _check(C >= 4 and C % 4 == 0, f"{what}: the channel count must be a multiple of 4 (got {C})")
    _gpu(x)
    if x.stride(2) != 1 or x.stride(0) % 4 or x.stride(1) % 4 or x.stride(1) < C or x.data_ptr() % 16:
        x = x.contiguous()
    return x


def _square_grid(what, L, grid):
    _check(grid >= 1 and grid * grid == L, f"{what}: the tokens must form a square grid (L = {L}, grid = {grid}); other grids are out of scope")


def pos_rope(x, sin, cos, inverse=False):
    """-> y (B, L, C): x cos + rotate_half(x) sin, rotate_half(x)[2i] = -x[2i+1], rotate_half(x)[2i+1] = x[2i], in ONE launch. sin, cos: (L, C)
    float32 tables. inverse: the transpose of that map -- the backward of the forward, and for rotary tables (equal within a channel pair,
    sin^2 + cos^2 = 1) its inverse."""
    x = _pos_tokens("pos_rope", x)
    B, L, C = x.shape
    _gpu(sin, cos)
    for t in (sin, cos):
        _check(t.dtype == torch.float32 and tuple(t.shape) == (L, C) and t.is_contiguous() and t.data_ptr() % 16 == 0,
               f"pos_rope: sin and cos are contiguous float32 (L, C) = ({L}, {C}) tables")
    y = torch.empty((B, L, C), dtype=torch.float32, device=x.device)
    P = _lib.PosRopeParams()
    P.batch, P.tokens, P.channels, P.inverse = B, L, C, int(bool(inverse))
    P.x_batch_stride, P.x_token_stride, P.y_batch_stride, P.y_token_stride = x.stride(0), x.stride(1), L * C, C
    P.x, P.sin, P.cos, P.y = x.data_ptr(), sin.data_ptr(), cos.data_ptr(), y.data_ptr()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dimsum_pos_rope(P, _stream(x)), "dimsum_pos_rope")
    return y


def _pos_cpe_params(what, x, weight, bias, gamma, beta, shift, scale, grid, eps):
    """-> (x as read, the dimsum_pos_cpe_params_t with everything but the outputs, the tensors it points to)"""
    x = _pos_tokens(what, x)
    B, L, C = x.shape
    _square_grid(what, L, grid)
    _check(C <= CPE_MAX_CHANNELS, f"{what}: at most {CPE_MAX_CHANNELS} channels (got {C})")
    _gpu(weight, bias, gamma, beta, shift, scale)
    _check(weight.numel() == 9 * C and tuple(weight.shape[-2:]) == (3, 3), f"{what}: weight is the (C, 1, 3, 3) kernel of a depthwise 3x3 convolution")
    for t in (bias, gamma, beta):
        _check(tuple(t.shape) == (C,), f"{what}: the convolution's bias and the LayerNorm's weight and bias are (C,) tensors")
    weight, bias, gamma, beta = (t.detach().float().contiguous() for t in (weight, bias, gamma, beta))
    for t in (shift, scale):
        _check(tuple(t.shape) == (B, C) and t.dtype == torch.float32, f"{what}: shift and scale are float32 (B, C) tensors")
    if not (shift.stride(1) == 1 and scale.stride(1) == 1 and (B == 1 or shift.stride(0) == scale.stride(0)) and shift.stride(0) % 4 == 0
            and shift.data_ptr() % 16 == 0 and scale.data_ptr() % 16 == 0):
        shift, scale = shift.contiguous(), scale.contiguous()
    P = _lib.PosCpeParams()
    P.batch, P.grid, P.channels, P.eps = B, grid, C, eps
    P.x_batch_stride, P.x_token_stride, P.mod_batch_stride = x.stride(0), x.stride(1), shift.stride(0) if B > 1 else C
    P.x, P.weight, P.conv_bias, P.gamma, P.beta, P.shift, P.scale = (t.data_ptr() for t in (x, weight, bias, gamma, beta, shift, scale))
    return x, P, (x, weight, bias, gamma, beta, shift, scale)


def pos_cpe_fwd(x, weight, bias, gamma, beta, shift, scale, grid, eps=1e-5, need_stats=False, need_v=False):
    """-> (y, mean, rstd, v): v = x + bias + depthwise 3x3 conv(x) on the (grid, grid) token grid (zero padding 1, token l = h * grid + w),
    y = (LayerNorm(v) gamma + beta) (1 + scale[b]) + shift[b], in ONE launch. x: (B, grid^2, C); weight (C, 1, 3, 3); bias, gamma, beta (C,);
    shift, scale (B, C) (the two halves of an adaLN head's output are read in place). need_stats: mean, rstd (B * L,) for the backward, else None.
    need_v (tests): v itself, else None -- the backward rebuilds it from x."""
    x, P, keep = _pos_cpe_params("pos_cpe_fwd", x, weight, bias, gamma, beta, shift, scale, grid, eps)
    B, L, C = x.shape
    y = torch.empty((B, L, C), dtype=torch.float32, device=x.device)
    mean, rstd = (torch.empty(B * L, dtype=torch.float32, device=x.device) for _ in range(2)) if need_stats else (None, None)
    v = torch.empty_like(y) if need_v else None
    P.y_batch_stride, P.y_token_stride = L * C, C
    P.y, P.mean, P.rstd, P.v = y.data_ptr(), _ptr(mean), _ptr(rstd), _ptr(v)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dimsum_pos_cpe_fwd(P, _stream(x)), "dimsum_pos_cpe_fwd")
    return y, mean, rstd, v


def pos_cpe_bwd(dy, x, weight, bias, gamma, beta, shift, scale, mean, rstd, grid, eps=1e-5):
    """-> (dx, dweight, dbias, dgamma, dbeta, dmod) of pos_cpe_fwd in TWO launches: the row pass (v again from x, the modulation and LayerNorm
    backward, every parameter gradient) and dx = dv + conv^T(dv). dweight has weight's shape; dmod (B, 2 C) = [dshift | dscale], the gradient of
    the adaLN head's output. Every parameter gradient is a tensor of its own (fp32, accumulated by atomic adds of per-workgroup sums)."""
    x, P0, keep = _pos_cpe_params("pos_cpe_bwd", x, weight, bias, gamma, beta, shift, scale, grid, eps)
    B, L, C = x.shape
    dy = _pos_tokens("pos_cpe_bwd", dy)
    _check(dy.shape == x.shape, "pos_cpe_bwd: dy has the shape of x")
    _gpu(mean, rstd)
    for t in (mean, rstd):
        _check(t.dtype == torch.float32 and t.numel() == B * L and t.is_contiguous(), "pos_cpe_bwd: mean and rstd are the forward's float32 (B * L,) tensors")
    dev = x.device
    dv, dx = torch.empty((B, L, C), dtype=torch.float32, device=dev), torch.empty((B, L, C), dtype=torch.float32, device=dev)
    dweight = torch.zeros(weight.shape, dtype=torch.float32, device=dev)
    dbias, dgamma, dbeta = (torch.zeros(C, dtype=torch.float32, device=dev) for _ in range(3))
    dmod = torch.zeros((B, 2 * C), dtype=torch.float32, device=dev)
    P = _lib.PosCpeBwdParams()
    P.fwd = P0
    P.fwd.mean, P.fwd.rstd = mean.data_ptr(), rstd.data_ptr()
    P.dy_batch_stride, P.dy_token_stride, P.dmod_batch_stride = dy.stride(0), dy.stride(1), 2 * C
    P.dy, P.dv, P.dx = dy.data_ptr(), dv.data_ptr(), dx.data_ptr()
    P.dweight, P.dconv_bias, P.dgamma, P.dbeta = dweight.data_ptr(), dbias.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
    P.dshift, P.dscale = dmod.data_ptr(), dmod.data_ptr() + 4 * C
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dimsum_pos_cpe_bwd(P, _stream(x)), "dimsum_pos_cpe_bwd")
    return dx, dweight, dbias, dgamma, dbeta, dmod


# ---------------------------------------------------------------------------------------------------------------------
# the spectral branch of block type "combined_einfft" (dimsum_einfft_*; dimsum_amd/ops/einfft.py is the user)
# ---------------------------------------------------------------------------------------------------------------------
EINFFT_MIN_TOKENS, EINFFT_MAX_TOKENS = 16, 1024       # the N-point part is an FFT in LDS
EINFFT_CHANNEL_GRANULE = 32                           # 4 channel blocks of a multiple of 8 columns
EINFFT_MAX_CHANNELS = 1024                            # the MLP keeps two (2 bs, 32) operand tiles in LDS: bs <= 256


def einfft_check_shape(what, N, C):
    """the limits of the einfft passes, checked before any launch: N a power of two in [16, 1024], C % 32 == 0, C <= 1024"""
    _check(EINFFT_MIN_TOKENS <= N <= EINFFT_MAX_TOKENS and N & (N - 1) == 0,
           f"{what}: the token count must be a power of two in [{EINFFT_MIN_TOKENS}, {EINFFT_MAX_TOKENS}] (got {N})")
    _check(C >= EINFFT_CHANNEL_GRANULE and C % EINFFT_CHANNEL_GRANULE == 0 and C <= EINFFT_MAX_CHANNELS,
           f"{what}: the channel count must be a multiple of {EINFFT_CHANNEL_GRANULE}, at most {EINFFT_MAX_CHANNELS} (got {C})")


def _einfft_planes(what, B, N, C, *ts):
    for t in ts:
        _check(t.dtype == torch.float32 and tuple(t.shape) == (B, N, C) and t.is_contiguous(),
               f"{what}: the spectrum planes are contiguous float32 (B, N, C) = ({B}, {N}, {C}) tensors")
    _gpu(*ts)


def _einfft_dft_params(x, re, im):
    B, N, C = x.shape
    P = _lib.EinfftDftParams()
    P.batch, P.tokens, P.channels = B, N, C
    P.x_batch_stride, P.x_token_stride = x.stride(0), x.stride(1)
    P.x, P.re, P.im = x.data_ptr(), re.data_ptr(), im.data_ptr()
    return P


def _einfft_real(what, x):
    _check(x.dim() == 3 and x.dtype == torch.float32, f"{what}: x is a float32 (B, N, C) tensor (got {tuple(x.shape)}, {x.dtype})")
    B, N, C = x.shape
    _check(B > 0, f"{what}: empty tensors are not supported")
    einfft_check_shape(what, N, C)
    _gpu(x)
    return x.stride(2) == 1 and x.stride(1) >= C and (B == 1 or x.stride(0) >= (N - 1) * x.stride(1) + C)


def einfft_dft(x):
    """-> (re, im), contiguous (B, N, C) each: the ortho-normalised 2-D DFT of the real x over (the N tokens, the 4 channel blocks
    {j, j + C/4, j + 2 C/4, j + 3 C/4}), in ONE launch. A channel-half view of a wider tensor is read in place."""
    if not _einfft_real("einfft_dft", x):
        x = x.contiguous()
    B, N, C = x.shape
    re, im = (torch.empty((B, N, C), dtype=torch.float32, device=x.device) for _ in range(2))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dimsum_einfft_dft(_einfft_dft_params(x, re, im), _stream(x)), "dimsum_einfft_dft")
    return re, im


def einfft_idft_real(re, im, out=None):
    """-> y (B, N, C): the real part of the inverse of einfft_dft (its transpose), in ONE launch. out: written in place when given (any row
    stride, e.g. a channel-half view)."""
    _check(re.dim() == 3 and re.dtype == torch.float32, f"einfft_idft_real: re, im are float32 (B, N, C) tensors (got {tuple(re.shape)}, {re.dtype})")
    B, N, C = re.shape
    einfft_check_shape("einfft_idft_real", N, C)
    _einfft_planes("einfft_idft_real", B, N, C, re, im)
    if out is None:
        out = torch.empty((B, N, C), dtype=torch.float32, device=re.device)
    _check(tuple(out.shape) == (B, N, C) and _einfft_real("einfft_idft_real", out), "einfft_idft_real: out is a float32 (B, N, C) tensor with contiguous channels and rows that do not overlap")
    with torch.cuda.device(re.device):
        _lib.check(_lib.load().dimsum_einfft_idft_real(_einfft_dft_params(out, re, im), _stream(re)), "dimsum_einfft_idft_real")
    return out


def _einfft_mlp_params(what, re, im, w1, b1, w2, b2, lam):
    _check(re.dim() == 3 and re.dtype == torch.float32, f"{what}: re, im are float32 (B, N, C) tensors (got {tuple(re.shape)}, {re.dtype})")
    B, N, C = re.shape
    _check(C >= EINFFT_CHANNEL_GRANULE and C % EINFFT_CHANNEL_GRANULE == 0 and C <= EINFFT_MAX_CHANNELS,
           f"{what}: the channel count must be a multiple of {EINFFT_CHANNEL_GRANULE}, at most {EINFFT_MAX_CHANNELS} (got {C})")
    _check(B * N > 0, f"{what}: empty tensors are not supported")
    _einfft_planes(what, B, N, C, re, im)
    bs = C // 4
    _gpu(w1, b1, w2, b2)
    for w, b in ((w1, b1), (w2, b2)):
        _check(w.dtype == torch.float32 and tuple(w.shape) == (2, 4, bs, bs) and b.dtype == torch.float32 and tuple(b.shape) == (2, 4, bs),
               f"{what}: the weights are float32 (2, 4, {bs}, {bs}) tensors, the biases (2, 4, {bs})")
    keep = tuple(t.detach().contiguous() for t in (w1, b1, w2, b2))
    P = _lib.EinfftMlpParams()
    P.channels, P.rows, P.lam = C, B * N, float(lam)
    P.xr, P.xi = re.data_ptr(), im.data_ptr()
    P.w1, P.b1, P.w2, P.b2 = (t.data_ptr() for t in keep)
    return P, keep


def einfft_mlp_fwd(re, im, w1, b1, w2, b2, lam):
    """-> (zr, zi): per row and channel block the complex two-layer MLP h = relu(x W1 + b1) (both parts), z = softshrink(h W2 + b2, lam) (both
    parts), in ONE launch; h stays on the chip. re, im: (B, N, C) planes; w: (2, 4, bs, bs) = [re | im][block][in][out]; b: (2, 4, bs)."""
    P, keep = _einfft_mlp_params("einfft_mlp_fwd", re, im, w1, b1, w2, b2, lam)
    zr, zi = torch.empty_like(re), torch.empty_like(im)
    P.zr, P.zi = zr.data_ptr(), zi.data_ptr()
    with torch.cuda.device(re.device):
        _lib.check(_lib.load().dimsum_einfft_mlp_fwd(P, _stream(re)), "dimsum_einfft_mlp_fwd")
    return zr, zi


def einfft_mlp_bwd(dzr, dzi, re, im, zr, zi, w1, b1, w2, b2, lam):
    """-> (dxr, dxi, (h1r, h1i), (dz2r, dz2i), (dp1r, dp1i)) in ONE launch: the gradient of the spectrum planes and the three plane pairs whose
    products are the parameter gradients (layer 1's output again, the gradient behind the softshrink mask z != 0, the gradient behind the ReLU
    mask). zr, zi: the forward's output."""
    P0, keep = _einfft_mlp_params("einfft_mlp_bwd", re, im, w1, b1, w2, b2, lam)
    B, N, C = re.shape
    _einfft_planes("einfft_mlp_bwd", B, N, C, dzr, dzi, zr, zi)
    w1t, w2t = (w.transpose(-1, -2).contiguous() for w in (keep[0], keep[2]))
    outs = [torch.empty_like(re) for _ in range(8)]
    P = _lib.EinfftMlpBwdParams()
    P.fwd = P0
    P.fwd.zr, P.fwd.zi = zr.data_ptr(), zi.data_ptr()
    P.w1t, P.w2t, P.dzr, P.dzi = w1t.data_ptr(), w2t.data_ptr(), dzr.data_ptr(), dzi.data_ptr()
    P.dxr, P.dxi, P.h1r, P.h1i, P.dz2r, P.dz2i, P.dp1r, P.dp1i = (t.data_ptr() for t in outs)
    with torch.cuda.device(re.device):
        _lib.check(_lib.load().dimsum_einfft_mlp_bwd(P, _stream(re)), "dimsum_einfft_mlp_bwd")
    return outs[0], outs[1], (outs[2], outs[3]), (outs[4], outs[5]), (outs[6], outs[7])


MOE_GEMM_BM, MOE_GEMM_BN = _lib.MOE_GEMM_BM, _lib.MOE_GEMM_BN      # the output tile of moe_gemm (rows, columns)


def moe_gemm_serves(k, n, num_experts):
    """whether moe_gemm has a kernel for (rows, k) x num_experts (n, k) matrices"""
    return k > 0 and n > 0 and k % 32 == 0 and n % 32 == 0 and 1 <= num_experts <= MOE_MAX_EXPERTS


# ---- what the four wrappers of the grouped expert GEMM share. Every check names the wrapper it refuses for; the ORDER of the checks is each
# wrapper's own (moe_gemm asks for the device first, the other three refuse dtypes, shapes and widths without a GPU and ask for the device last)
def _moe_gemm_experts(name, E):
    _check(1 <= E <= MOE_MAX_EXPERTS, f"{name}: 1 <= experts <= {MOE_MAX_EXPERTS}")
    return E


def _moe_gemm_rows(name, t, what, T=None):
    _check(t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and (T is None or t.shape[0] == T), f"{name}: {what} must be contiguous float32 ({'T' if T is None else T}, width)")


def _moe_gemm_weights(name, weights, N, K, device, f16=False):
    """the E (N, K) matrices of the experts: float32 tensors, or (f16) F16Images -> (matrices, their (N,) inverse scales or [])"""
    mats, invs = ([w.data for w in weights], [w.inv for w in weights]) if f16 else (list(weights), [])
    ok = lambda t, dtype, shape: t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape and t.device == device
    _check(all(ok(m, torch.float16 if f16 else torch.float32, (N, K)) for m in mats) and all(ok(i, torch.float32, (N,)) for i in invs),
           f"{name}: every weight image must be contiguous float16 ({N}, {K}) with float32 ({N},) inverse scales on the rows' device" if f16
           else f"{name}: every weight must be contiguous float32 ({N}, {K}) on the rows' device")
    return mats, invs


def _moe_gemm_offsets(name, offsets, E, device, K, N, rule="the widths must be multiples of 32"):
    """the served widths, then the offset table"""
    _check(moe_gemm_serves(K, N, E), f"{name}: {rule} (got K {K}, N {N}); there is no other kernel and no fallback")
    _check(offsets.dtype == torch.int32 and offsets.is_contiguous() and tuple(offsets.shape) == (E + 1,) and offsets.device == device,
           f"{name}: offsets must be contiguous int32 ({E + 1},) on the rows' device")


def _moe_gemm_out(name, out, T, W, device, bias=None, E=0):
    """the (E, W) bias where the entry takes one, then the output view (allocated unless given) -> out"""
    _check(bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (E, W)), f"{name}: bias must be contiguous float32 ({E}, {W})")
    if out is None:
        out = torch.empty(T, W, device=device, dtype=torch.float32)
    _check(out.dtype == torch.float32 and tuple(out.shape) == (T, W) and out.device == device and (T == 0 or (out.stride(1) == 1 and out.stride(0) >= W)),
           f"{name}: out must be a float32 ({T}, {W}) view with unit column stride and row stride >= {W}")
    return out


def _moe_gemm_launch(name, P, shape, tables, **ptrs):
    """dimsum_<name>(P) on the device and stream of the first tensor of ptrs; an empty call launches nothing. shape: (E, T, K, N); ptrs: field =
    tensor or None; tables: field -> the E tensors whose addresses the kernel takes by value"""
    if shape[1] == 0:
        return
    P.num_experts, P.tokens, P.k, P.n = shape
    for field, t in ptrs.items():
        setattr(P, field, _ptr(t))
    for field, ts in tables.items():
        setattr(P, field, (_lib.vp * len(ts))(*[t.data_ptr() for t in ts]))      # (P holds on to the array)
    rows = next(iter(ptrs.values()))
    with torch.cuda.device(rows.device):
        _lib.check(getattr(_lib.load(), "dimsum_" + name)(P, _stream(rows)), name)


def moe_gemm(xp, offsets, weights, bias=None, out=None):
    """xp (T, K) rows sorted by expert, offsets (E + 1) int32 ON THE DEVICE (moe_route_fwd's: non-decreasing in [0, T]; another table is clamped to [0, T] and its ranges are cut where they overlap an earlier one), weights: E
    (N, K) matrices, bias (E, N) or None -> out (T, N): out[j] = xp[j] W_e^T (+ bias[e]) for offsets[e] <= j < offsets[e + 1]. One launch, no host
    read of the offsets; fp32 as three bf16 MFMA products (hi hi + hi lo + lo hi), bit-reproducible. out: a (T, N) float32 view with unit column
    stride (its row stride may exceed N); rows outside every range keep what they held."""
    _gpu(xp, offsets, bias, out, *weights)
    E = _moe_gemm_experts("moe_gemm", len(weights))
    _check(xp.dtype == torch.float32 and xp.dim() == 2 and xp.is_contiguous(), "moe_gemm: xp must be contiguous float32 (T, K)")
    T, K = xp.shape
    N = weights[0].shape[0]
    _moe_gemm_weights("moe_gemm", weights, N, K, xp.device)
    _moe_gemm_offsets("moe_gemm", offsets, E, xp.device, K, N, "K % 32 == 0 and N % 32 == 0")
    out = _moe_gemm_out("moe_gemm", out, T, N, xp.device, bias, E)
    _moe_gemm_launch("moe_gemm", _lib.MoeGemmParams(ldc=out.stride(0)), (E, T, K, N), dict(w_ptrs=weights), x_ptr=xp, offsets_ptr=offsets, bias_ptr=bias, out_ptr=out)
    return out


def moe_gemm_f16s(x16, offsets, weight_images, bias=None, out=None):
    """moe_gemm on scaled-fp16 operand images (csrc/moe_gemm_f16.hip): x16 an F16Image of the (T, K) rows sorted by expert (moe_permute / moe_act_fwd
    with split3="f16s", rows_f16s), weight_images: E F16Images of the (N, K) matrices (rows_f16s, gemm.weight_f16s), offsets (E + 1) int32 ON THE
    DEVICE (read, clamped and cut as moe_gemm does), bias (E, N) float32 or None -> out (T, N) float32:
    out[j, n] = x_inv[j] w_inv_e[n] sum_k x16[j, k] w16_e[n, k] (+ bias[e, n]) for offsets[e] <= j < offsets[e + 1]. One launch, ONE fp16 MFMA product
    per element with fp32 accumulation, no host read of the offsets, bit-reproducible. out: a (T, N) float32 view with unit column stride (its row
    stride may exceed N); rows outside every range keep what they held."""
    E = _moe_gemm_experts("moe_gemm_f16s", len(weight_images))
    _check(isinstance(x16, F16Image) and all(isinstance(w, F16Image) for w in weight_images), "moe_gemm_f16s: the operands must be F16Images (float16 rows + float32 inverse scales)")
    xd, xi = x16.data, x16.inv
    _check(xd.dtype == torch.float16 and xd.dim() == 2 and xd.is_contiguous() and xi.dtype == torch.float32 and xi.is_contiguous() and tuple(xi.shape) == (xd.shape[0],)
           and xi.device == xd.device, "moe_gemm_f16s: x16 must be contiguous float16 (T, K) with float32 (T,) inverse scales")
    T, K = xd.shape
    w0 = weight_images[0].data
    N = w0.shape[0] if w0.dim() == 2 else -1
    mats, invs = _moe_gemm_weights("moe_gemm_f16s", weight_images, N, K, xd.device, f16=True)
    _moe_gemm_offsets("moe_gemm_f16s", offsets, E, xd.device, K, N, "K % 32 == 0 and N % 32 == 0")
    out = _moe_gemm_out("moe_gemm_f16s", out, T, N, xd.device, bias, E)
    _gpu(xd, xi, offsets, bias, out, *[t for pair in zip(mats, invs) for t in pair])
    _moe_gemm_launch("moe_gemm_f16s", _lib.MoeGemmF16sParams(ldc=out.stride(0)), (E, T, K, N), dict(w_ptrs=mats, w_inv_ptrs=invs),
                     x_ptr=xd, x_inv_ptr=xi, offsets_ptr=offsets, bias_ptr=bias, out_ptr=out)
    return out


def moe_gemm_dgrad(dy, offsets, weights, out=None):
    """the data gradient of moe_gemm: dy (T, N) rows sorted by expert, offsets (E + 1) int32 ON THE DEVICE (read, clamped and cut as moe_gemm does),
    weights: the forward's E (N, K) matrices -> dx (T, K): dx[j] = dy[j] W_e for offsets[e] <= j < offsets[e + 1]. One launch, no host read of the
    offsets, no W^T in memory; the forward's three bf16 products, bit-reproducible. out: a (T, K) float32 view with unit column stride; rows outside
    every range keep what they held."""
    E = _moe_gemm_experts("moe_gemm_dgrad", len(weights))
    _moe_gemm_rows("moe_gemm_dgrad", dy, "dy")
    T, N = dy.shape
    K = weights[0].shape[1] if weights[0].dim() == 2 else -1
    _moe_gemm_weights("moe_gemm_dgrad", weights, N, K, dy.device)
    _moe_gemm_offsets("moe_gemm_dgrad", offsets, E, dy.device, K, N)
    out = _moe_gemm_out("moe_gemm_dgrad", out, T, K, dy.device)
    _gpu(dy, offsets, out, *weights)
    _moe_gemm_launch("moe_gemm_dgrad", _lib.MoeGemmDgradParams(ldc=out.stride(0)), (E, T, K, N), dict(w_ptrs=weights), dy_ptr=dy, offsets_ptr=offsets, dx_ptr=out)
    return out


def moe_gemm_wgrad(dy, x, offsets, num_experts, need_dbias=False):
    """the weight gradient of moe_gemm: dy (T, N), x (T, K) rows sorted by expert, offsets (E + 1) int32 ON THE DEVICE -> (E tensors (N, K), db (E, N)
    or None): dW_e = dy[o_e:o_e+1]^T x[o_e:o_e+1], db[e] = dy[o_e:o_e+1].sum(0). One launch writes every element -- zeros for an expert without rows,
    decided on the device; no atomics, bit-reproducible."""
    E = _moe_gemm_experts("moe_gemm_wgrad", int(num_experts))
    _moe_gemm_rows("moe_gemm_wgrad", dy, "dy")
    T, N = dy.shape
    _moe_gemm_rows("moe_gemm_wgrad", x, "x", T)
    _check(x.device == dy.device, "moe_gemm_wgrad: dy and x must be on one device")
    K = x.shape[1]
    _moe_gemm_offsets("moe_gemm_wgrad", offsets, E, dy.device, K, N)
    _gpu(dy, x, offsets)
    new = torch.empty if T > 0 else torch.zeros          # (an empty call launches nothing: its zeros are made here)
    dw = new(E, N, K, device=dy.device, dtype=torch.float32)              # (N K % 1024 == 0: every slice is 16-byte aligned)
    db = new(E, N, device=dy.device, dtype=torch.float32) if need_dbias else None
    dws = list(dw.unbind(0))
    _moe_gemm_launch("moe_gemm_wgrad", _lib.MoeGemmWgradParams(), (E, T, K, N), dict(dw_ptrs=dws), dy_ptr=dy, x_ptr=x, offsets_ptr=offsets, db_ptr=db)
    return dws, db


