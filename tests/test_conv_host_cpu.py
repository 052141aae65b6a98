"""Characterisation of the causal conv1d's host layer, in two parts.

1. The C side (csrc/causal_conv1d.hip): the status code of every refusal the six seqlen-contiguous entry points give before a kernel is
launched, plus the `batch == 0 -> DIMSUM_OK` early return of the five that have it, and a handful of two-fault cases that pin the ORDER each
entry checks in. The codes were recorded from the library BEFORE the host layer was refactored and are kept verbatim: a refactor of that
layer has to reproduce them. Every pointer is a made-up, 16-byte aligned address that is never read: no case reaches a launch. (The
channel-last pair is pinned by test_conv_cl_cpu.py::test_library_refusals_without_a_device.)

`return DIMSUM_ERR_*` lines of these entry points that cannot be reached without a launch, and so have no case here: none in
causal_conv1d.hip itself -- the only one is launch_status()'s DIMSUM_ERR_LAUNCH (common.hpp), after a kernel went out.

2. The Python side (dimsum_amd/native.py, conv section): each of the nine native.causal_conv1d_* functions on CPU tensors with awkward
strides, through a stand-in for the library that records the entry reached and every field of the struct passed, nested structs included;
which operands were copied on the way (.float() / .contiguous()); and the order in which the refusals fire. Recorded before the refactor
as well."""
import contextlib
import ctypes as C

import pytest
import torch

from dimsum_amd import _lib

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)

B, D, L, W = 2, 8, 8, 4                              # the base call of part 1: fp32, contiguous (batch, dim, seqlen) operands


def _addr(i):
    return 0x10000000 + 0x1000 * i                   # 4-KB aligned, distinct, never dereferenced


def _fill_conv(P):
    P.batch, P.dim, P.seqlen, P.width, P.silu_activation, P.dtype = B, D, L, W, 1, _lib.F32
    P.x_batch_stride, P.x_c_stride, P.weight_c_stride, P.weight_width_stride, P.out_batch_stride, P.out_c_stride = D * L, L, W, 1, D * L, L
    P.x_ptr, P.weight_ptr, P.bias_ptr, P.out_ptr = _addr(0), _addr(1), _addr(2), _addr(3)


def _fill_bwd(Q):
    _fill_conv(Q.fwd)
    Q.fwd.out_ptr = None                             # the backward takes no out
    Q.dout_batch_stride, Q.dout_c_stride, Q.dx_batch_stride, Q.dx_c_stride, Q.dweight_c_stride, Q.dweight_width_stride = D * L, L, D * L, L, W, 1
    Q.dout_ptr, Q.dx_ptr, Q.dweight_ptr, Q.dbias_ptr = _addr(4), _addr(5), _addr(6), _addr(7)


def _fill_ids(V):
    V.seq_idx_ptr, V.seq_idx_batch_stride = _addr(8), L


def _make(entry, lib):
    """-> (C function, top struct, {prefix: struct}) of the base call of `entry`. Mutation keys are `prefix.field`: top = the struct the
    entry point takes, conv = its dimsum_conv_params_t (chunk: the chunk struct), bwd = its dimsum_conv_bwd_params_t, ids = the struct
    that holds seq_idx"""
    if entry == "fwd":
        P = _lib.ConvParams()
        _fill_conv(P)
        return lib.dimsum_causal_conv1d_fwd, P, {"top": P, "conv": P}
    if entry == "bwd":
        Q = _lib.ConvBwdParams()
        _fill_bwd(Q)
        return lib.dimsum_causal_conv1d_bwd, Q, {"top": Q, "conv": Q.fwd, "bwd": Q}
    if entry == "varlen_fwd":
        V = _lib.ConvVarlenParams()
        _fill_conv(V.conv), _fill_ids(V)
        return lib.dimsum_causal_conv1d_varlen_fwd, V, {"top": V, "conv": V.conv, "ids": V}
    if entry == "varlen_bwd":
        V = _lib.ConvVarlenBwdParams()
        _fill_bwd(V.conv), _fill_ids(V)
        return lib.dimsum_causal_conv1d_varlen_bwd, V, {"top": V, "conv": V.conv.fwd, "bwd": V.conv, "ids": V}
    if entry == "states":
        E = _lib.ConvVarlenStatesParams()
        _fill_conv(E.varlen.conv), _fill_ids(E.varlen)
        E.num_slots, E.end_slots_ptr, E.end_slots_batch_stride, E.state_ptr, E.state_dtype = 4, _addr(9), L, _addr(10), _lib.F32
        E.state_slot_stride, E.state_c_stride, E.state_w_stride = D * W, W, 1
        return lib.dimsum_causal_conv1d_varlen_states_fwd, E, {"top": E, "conv": E.varlen.conv, "ids": E.varlen}
    assert entry == "chunk"
    P = _lib.ConvChunkParams()
    P.batch, P.dim, P.seqlen, P.width, P.silu_activation, P.dtype = B, D, L, W, 1, _lib.F32
    P.x_batch_stride, P.x_c_stride, P.state_batch_stride, P.state_c_stride, P.state_w_stride = D * L, L, D * W, W, 1
    P.weight_c_stride, P.weight_width_stride, P.out_batch_stride, P.out_c_stride = W, 1, D * L, L
    P.x_ptr, P.weight_ptr, P.bias_ptr, P.conv_state_ptr, P.out_ptr = _addr(0), _addr(1), _addr(2), _addr(11), _addr(3)
    return lib.dimsum_causal_conv1d_chunk, P, {"top": P, "conv": P}


def _status(entry, mut):
    lib = _lib.load()
    fn, P, parts = _make(entry, lib)
    for key, val in mut.items():
        if key == "null":                            # the NULL struct itself
            return fn(None, None)
        prefix, field = key.split(".")
        if field == "struct_size" and val:           # a size relative to the right one
            val += getattr(parts[prefix], field)
        setattr(parts[prefix], field, val)
    return fn(P, None)


_STRUCT = [({"null": 1}, NULL), ({"top.struct_size": 0}, ABI), ({"top.struct_size": 8}, ABI), ({"top.struct_size": -8}, ABI)]
_SHAPE = [({"conv.width": 1}, SHAPE), ({"conv.width": 5}, SHAPE), ({"conv.batch": -1}, SHAPE), ({"conv.dim": 0}, SHAPE), ({"conv.seqlen": 0}, SHAPE)]
_DTYPE = [({"conv.dtype": -1}, DTYPE), ({"conv.dtype": 3}, DTYPE)]
_FWD_NULL = [({"conv." + t + "_ptr": None}, NULL) for t in ("x", "weight", "out")]
_BWD_NULL = [({"conv." + t + "_ptr": None}, NULL) for t in ("x", "weight")] + [({"bwd." + t + "_ptr": None}, NULL) for t in ("dout", "dx", "dweight")]
_IDS = [({"ids.seq_idx_ptr": None}, NULL), ({"ids.seq_idx_batch_stride": -1}, STRIDE), ({"ids.seq_idx_batch_stride": L - 1}, STRIDE),
        ({"ids.seq_idx_batch_stride": -1, "conv.batch": 0}, STRIDE),                     # the ids are checked before the empty batch returns
        ({"conv.dtype": 3, "ids.seq_idx_ptr": None}, DTYPE)]                             # ... and after the plain checks
_EMPTY = [({"conv.batch": 0}, OK)]
_CHUNK_STRIDES = ("x_batch_stride", "x_c_stride", "state_batch_stride", "state_c_stride", "state_w_stride", "weight_c_stride", "weight_width_stride",
                  "out_batch_stride", "out_c_stride")

# (entry, what the base call is changed in, status)
CASES = (
    [("fwd", m, s) for m, s in _STRUCT + _FWD_NULL + _SHAPE + _DTYPE + _EMPTY]
    + [("fwd", m, s) for m, s in [
        ({"conv.out_ptr": None, "conv.width": 5}, NULL),                                 # out, then the plain checks
        ({"conv.x_ptr": None, "conv.width": 5}, NULL), ({"conv.width": 5, "conv.dtype": 3}, SHAPE), ({"conv.dtype": 3, "conv.batch": 0}, DTYPE),
        ({"conv.out_ptr": None, "top.struct_size": 8}, ABI),
    ]]
    + [("bwd", m, s) for m, s in _STRUCT + _BWD_NULL + _SHAPE + _DTYPE + _EMPTY]
    + [("bwd", m, s) for m, s in [
        ({"bwd.dx_ptr": None, "conv.width": 5}, NULL), ({"conv.weight_ptr": None, "conv.seqlen": 0}, NULL), ({"conv.dtype": 3, "conv.batch": 0}, DTYPE),
        ({"bwd.dbias_ptr": None, "conv.bias_ptr": None, "conv.batch": 0}, OK),           # both are optional
    ]]
    + [("varlen_fwd", m, s) for m, s in _STRUCT + _FWD_NULL + _SHAPE + _DTYPE + _IDS + _EMPTY]
    + [("varlen_fwd", m, s) for m, s in [
        ({"conv.width": 5, "ids.seq_idx_ptr": None}, SHAPE),                             # the plain checks, then the ids
        ({"conv.out_ptr": None, "ids.seq_idx_batch_stride": -1}, NULL),
    ]]
    + [("varlen_bwd", m, s) for m, s in _STRUCT + _BWD_NULL + _SHAPE + _DTYPE + _IDS + _EMPTY]
    + [("varlen_bwd", m, s) for m, s in [
        ({"conv.width": 5, "ids.seq_idx_ptr": None}, SHAPE), ({"bwd.dout_ptr": None, "ids.seq_idx_ptr": None, "conv.width": 5}, NULL),
    ]]
    + [("states", m, s) for m, s in _STRUCT + _FWD_NULL + _SHAPE + _DTYPE + _IDS + _EMPTY]
    + [("states", m, s) for m, s in [
        ({"top.num_slots": 0}, SHAPE), ({"top.num_slots": -1}, SHAPE), ({"top.end_slots_ptr": None}, NULL), ({"top.state_ptr": None}, NULL),
        ({"top.state_slot_stride": -1}, STRIDE), ({"top.state_c_stride": -1}, STRIDE), ({"top.state_w_stride": -1}, STRIDE),
        ({"top.end_slots_batch_stride": -1}, STRIDE), ({"top.end_slots_batch_stride": L - 1}, STRIDE),
        ({"top.state_dtype": _lib.F16}, UNSUPPORTED), ({"top.state_dtype": _lib.F16, "conv.dtype": _lib.BF16}, UNSUPPORTED),
        # the entry's own fields come first, in the header's order, then the shared sequence, then the state's dtype
        ({"top.num_slots": 0, "top.struct_size": 8}, ABI), ({"top.end_slots_ptr": None, "conv.width": 5}, NULL),
        ({"top.state_dtype": _lib.F16, "ids.seq_idx_ptr": None}, NULL), ({"top.state_slot_stride": -1, "conv.out_ptr": None}, STRIDE),
        ({"top.num_slots": 0, "top.end_slots_ptr": None}, SHAPE), ({"top.state_ptr": None, "top.end_slots_batch_stride": -1}, NULL),
        ({"top.end_slots_batch_stride": -1, "conv.x_ptr": None}, STRIDE), ({"top.state_dtype": _lib.F16, "conv.batch": 0}, UNSUPPORTED),
        ({"top.state_dtype": _lib.F16, "conv.dtype": 3}, DTYPE), ({"top.state_w_stride": -1, "conv.batch": 0}, STRIDE),
    ]]
    + [("chunk", m, s) for m, s in _STRUCT + _FWD_NULL + _SHAPE + _DTYPE]
    + [("chunk", {"conv." + n: -1}, STRIDE) for n in _CHUNK_STRIDES]
    + [("chunk", m, s) for m, s in [
        ({"conv.batch": 0}, SHAPE),                                                      # refused here, not OK
        ({"conv.conv_state_ptr": None}, NULL), ({"conv.width": 5, "conv.dtype": 3}, SHAPE), ({"conv.conv_state_ptr": None, "conv.width": 5}, NULL),
        ({"conv.dtype": 3, "conv.x_c_stride": -1}, DTYPE), ({"conv.batch": 0, "conv.out_c_stride": -1}, SHAPE),
    ]]
)


def _case_id(case):
    entry, mut, _ = case
    return entry + ":" + ",".join(f"{k}={v}" for k, v in mut.items())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_refused_inputs_keep_their_status(case):
    entry, mut, want = case
    assert want != LAUNCH and (want != OK or mut.get("conv.batch") == 0)       # a refusal, or the empty batch: nothing is launched
    assert _status(entry, mut) == want


# ---------------------------------------------------------------------------------------------------------------------
# part 2: what dimsum_amd.native hands the library
# ---------------------------------------------------------------------------------------------------------------------
def _snapshot(P):
    """every field of a parameter struct as plain Python values, nested structs (fwd, conv, varlen, ...) as nested dicts"""
    out = {}
    for f, _ in P._fields_:
        v = getattr(P, f)
        out[f] = _snapshot(v) if isinstance(v, C.Structure) else list(v) if isinstance(v, C.Array) else v
    return out


class _RecordingLib:
    """stands in for the loaded library: every dimsum_* call records (name, the fields of its struct) and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dimsum_"):
            raise AttributeError(name)
        return lambda P, stream: self.calls.append((name, _snapshot(P))) or 0


@pytest.fixture
def routed(monkeypatch):
    """dimsum_amd.native on CPU tensors with the device-facing pieces replaced: -> (the recording library, the list of the
    (shape, stride) of every non-contiguous 3-D tensor .contiguous() copied)"""
    from dimsum_amd import native
    lib, copies = _RecordingLib(), []
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(native, "_gpu", lambda *ts: None)
    monkeypatch.setattr(native, "_stream", lambda t: None)
    monkeypatch.setattr(native, "_zeros", lambda n, device: torch.zeros(n))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    plain = torch.Tensor.contiguous

    def counting(self, *a, **k):
        if self.dim() == 3 and not self.is_contiguous():
            copies.append((tuple(self.shape), self.stride()))
        return plain(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "contiguous", counting)
    return lib, copies


class _Copies:
    """the .float() / .contiguous() calls that made a new tensor, in order, each kept alive so that its address stays its own"""

    def __init__(self):
        self.made = []                               # (op, source, result)

    def of(self, t):
        """-> ([ops applied to t and to what they made of it], the tensor at the end of that chain)"""
        ops = []
        for op, src, res in self.made:
            if src is t:
                ops.append(op)
                t = res
        return ops, t


@pytest.fixture
def filled(routed, monkeypatch):
    """`routed` + a record of every copy: -> (the recording library, _Copies)"""
    lib, _ = routed
    rec = _Copies()
    for op in ("float", "contiguous"):
        def wrapped(self, *a, _op=op, _plain=getattr(torch.Tensor, op), **k):
            res = _plain(self, *a, **k)
            if res is not self:
                rec.made.append((_op, self, res))
            return res
        monkeypatch.setattr(torch.Tensor, op, wrapped)
    return lib, rec


class _OnGpu(torch.Tensor):
    """a CPU tensor that says it is on the GPU: state_indices, whose device native checks itself (not through _gpu)"""
    is_cuda = property(lambda self: True)


FB, FD, FL, FW = 2, 8, 5, 3                          # the calls of part 2
DTYPES = [torch.float32, torch.float16]
_CODE = {torch.float32: _lib.F32, torch.float16: _lib.F16}


def _half_x(dtype):
    """x = the second half of a (batch, 2 dim, seqlen) buffer: strides (2 dim seqlen, seqlen, 1)"""
    return torch.randn(FB, 2 * FD, FL).to(dtype)[:, FD:]


def _wb(dtype):
    return torch.randn(FD, FW).to(dtype), torch.randn(FD).to(dtype)


def _ids():
    return torch.tensor([[0, 0, 1, 1, 1], [0, 1, 1, 2, 2]], dtype=torch.int32)


def _conv_fields(x, w_used, b_used, silu, out, dtype):
    """dimsum_conv_params_t as _fill_conv fills it"""
    return {"struct_size": 0, "batch": FB, "dim": FD, "seqlen": FL, "width": FW, "silu_activation": int(silu), "dtype": _CODE[dtype], "reserved": 0,
            "x_batch_stride": x.stride(0), "x_c_stride": x.stride(1), "weight_c_stride": FW, "weight_width_stride": 1,
            "out_batch_stride": out.stride(0) if out is not None else 0, "out_c_stride": out.stride(1) if out is not None else 0,
            "x_ptr": x.data_ptr(), "weight_ptr": w_used.data_ptr(), "bias_ptr": b_used.data_ptr() if b_used is not None else None,
            "out_ptr": out.data_ptr() if out is not None else None}


def _operands(rec, w, b, dtype):
    """the copies every entry makes of its weights and bias: fp32 operands are used as they are (no copy at all), others through .float();
    -> (the weights, the bias the struct must name)"""
    (w_ops, w_used), (b_ops, b_used) = rec.of(w), rec.of(b) if b is not None else ([], None)
    want = [] if dtype == torch.float32 else ["float"]
    assert w_ops == want and (b is None or b_ops == want)
    assert w_used.dtype == torch.float32 and (b is None or (b_used.dtype == torch.float32 and b_used.is_contiguous()))
    return w_used, b_used


def _top(P, size_of):
    """a top-level struct's own struct_size is its sizeof; nested ones are not constructed and stay 0"""
    assert P["struct_size"] == C.sizeof(size_of)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("given", [False, True], ids=["out_omitted", "out_given"])
def test_fwd_fill(filled, dtype, given):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, b) = _half_x(dtype), _wb(dtype)
    out = torch.empty(FB, 2 * FD, FL, dtype=dtype)[:, :FD] if given else None
    got = native.causal_conv1d_fwd(x, w, b, True, out) if given else native.causal_conv1d_fwd(x, w, b, True)
    (name, P), = lib.calls
    assert name == "dimsum_causal_conv1d_fwd" and (got is out if given else got.stride() == (FD * FL, FL, 1))
    assert got.shape == x.shape and got.dtype == dtype
    w_used, b_used = _operands(rec, w, b, dtype)
    assert P == {**_conv_fields(x, w_used, b_used, True, got, dtype), "struct_size": C.sizeof(_lib.ConvParams)}
    assert rec.of(x) == ([], x)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fwd_cond_fill(filled, dtype):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, _) = _half_x(dtype), _wb(dtype)
    init = torch.empty(FB, FD, FL, dtype=dtype)
    got = native.causal_conv1d_fwd_cond(x, w, None, False, init)
    (name, P), = lib.calls
    w_used, _ = _operands(rec, w, None, dtype)
    assert name == "dimsum_causal_conv1d_fwd" and got is init
    assert P == {**_conv_fields(x, w_used, None, False, init, dtype), "struct_size": C.sizeof(_lib.ConvParams)}
    with pytest.raises(RuntimeError, match="causal_conv1d_fwd_cond: bad init_x"):
        native.causal_conv1d_fwd_cond(x, w, None, False, torch.empty(FB, FL, FD, dtype=dtype).transpose(1, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("given", [False, True], ids=["out_omitted", "out_given"])
def test_channel_last_fwd_fill(filled, dtype, given):
    from dimsum_amd import native
    lib, rec = filled
    w, b = _wb(dtype)
    x = torch.randn(FB, FL, 2 * FD).to(dtype)[..., FD:].transpose(1, 2)         # a half of a (batch, seqlen, 2 dim) buffer
    out = torch.empty(FB, FL, 3 * FD, dtype=dtype)[..., FD:2 * FD].transpose(1, 2) if given else None
    got = native.causal_conv1d_fwd(x, w, b, False, out)
    (name, P), = lib.calls
    w_used, b_used = _operands(rec, w, b, dtype)
    assert name == "dimsum_causal_conv1d_cl_fwd" and (got is out if given else got.stride() == (FL * FD, 1, FD))
    assert P == {"struct_size": C.sizeof(_lib.ConvClParams), "reserved": 0, "batch": FB, "dim": FD, "seqlen": FL, "width": FW, "silu_activation": 0,
                 "dtype": _CODE[dtype], "x_batch_stride": 2 * FD * FL, "x_l_stride": 2 * FD, "weight_c_stride": FW, "weight_width_stride": 1,
                 "out_batch_stride": got.stride(0), "out_l_stride": 3 * FD if given else FD, "x_ptr": x.data_ptr(), "weight_ptr": w_used.data_ptr(),
                 "bias_ptr": b_used.data_ptr(), "out_ptr": got.data_ptr()}
    assert rec.of(x) == ([], x)
    with pytest.raises(RuntimeError, match="causal_conv1d_fwd: out must be channel-last like x"):
        native.causal_conv1d_fwd(x, w, b, False, torch.empty(FB, FD, FL, dtype=dtype))


def _bwd_fields(dout, dx, dw_ptr, db_ptr):
    return {"dout_batch_stride": dout.stride(0), "dout_c_stride": dout.stride(1), "dx_batch_stride": dx.stride(0), "dx_c_stride": dx.stride(1),
            "dweight_c_stride": FW, "dweight_width_stride": 1, "dout_ptr": dout.data_ptr(), "dx_ptr": dx.data_ptr(), "dweight_ptr": dw_ptr, "dbias_ptr": db_ptr}


def _check_grads(res, dx_given, w, b, dtype):
    dx, dw, db = res
    assert (dx is dx_given if dx_given is not None else dx.is_contiguous()) and dx.shape == (FB, FD, FL) and dx.dtype == dtype
    assert dw.shape == w.shape and dw.dtype == dtype and (db is None if b is None else db.shape == b.shape and db.dtype == dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("given", [False, True], ids=["dx_omitted", "dx_given"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
def test_bwd_fill(filled, dtype, given, bias):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, b) = _half_x(dtype), _wb(dtype)
    b = b if bias else None
    dout = torch.randn(FB, 3 * FD, FL).to(dtype)[:, FD:2 * FD]
    dx_given = torch.empty(FB, 2 * FD, FL, dtype=dtype)[:, :FD] if given else None
    res = native.causal_conv1d_bwd(x, w, b, dout, dx_given, True)
    (name, Q), = lib.calls
    w_used, b_used = _operands(rec, w, b, dtype)
    _check_grads(res, dx_given, w, b, dtype)
    assert name == "dimsum_causal_conv1d_bwd" and Q["struct_size"] == C.sizeof(_lib.ConvBwdParams) and Q["reserved"] == 0
    assert Q["fwd"] == _conv_fields(x, w_used, b_used, True, None, dtype)
    # ONE accumulator buffer: dweight first, dbias right behind it
    assert Q["dweight_ptr"] and Q["dbias_ptr"] == (Q["dweight_ptr"] + 4 * FD * FW if bias else None)
    assert {k: v for k, v in Q.items() if k not in ("struct_size", "reserved", "fwd")} == _bwd_fields(dout, res[0], Q["dweight_ptr"], Q["dbias_ptr"])
    assert rec.of(x) == ([], x) and rec.of(dout) == ([], dout)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_channel_last_bwd_fill(filled, dtype):
    from dimsum_amd import native
    lib, rec = filled
    w, b = _wb(dtype)
    x = torch.randn(FB, FL, 2 * FD).to(dtype)[..., FD:].transpose(1, 2)
    dout = torch.randn(FB, FL, FD).to(dtype).transpose(1, 2)
    dx, dw, db = native.causal_conv1d_bwd(x, w, b, dout, None, False)
    (name, Q), = lib.calls
    w_used, b_used = _operands(rec, w, b, dtype)
    assert name == "dimsum_causal_conv1d_cl_bwd" and Q["struct_size"] == C.sizeof(_lib.ConvClBwdParams) and Q["reserved"] == 0
    assert Q["fwd"] == {"struct_size": 0, "reserved": 0, "batch": FB, "dim": FD, "seqlen": FL, "width": FW, "silu_activation": 0, "dtype": _CODE[dtype],
                        "x_batch_stride": 2 * FD * FL, "x_l_stride": 2 * FD, "weight_c_stride": FW, "weight_width_stride": 1, "out_batch_stride": 0,
                        "out_l_stride": 0, "x_ptr": x.data_ptr(), "weight_ptr": w_used.data_ptr(), "bias_ptr": b_used.data_ptr(), "out_ptr": None}
    assert (Q["dout_batch_stride"], Q["dout_l_stride"], Q["dx_batch_stride"], Q["dx_l_stride"], Q["dweight_c_stride"], Q["dweight_width_stride"]) == (
        FL * FD, FD, FL * FD, FD, FW, 1)
    assert (Q["dout_ptr"], Q["dx_ptr"], Q["dbias_ptr"]) == (dout.data_ptr(), dx.data_ptr(), Q["dweight_ptr"] + 4 * FD * FW)
    assert dx.stride() == (FL * FD, 1, FD) and rec.of(dout) == ([], dout) and dw.dtype == dtype and db.dtype == dtype


def _ids_fields(seq_idx):
    return {"seq_idx_ptr": seq_idx.data_ptr(), "seq_idx_batch_stride": FL}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("given", [False, True], ids=["out_omitted", "out_given"])
def test_varlen_fwd_fill(filled, dtype, given):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, b), seq = _half_x(dtype), _wb(dtype), _ids()
    out = torch.empty(FB, 2 * FD, FL, dtype=dtype)[:, :FD] if given else None
    got = native.causal_conv1d_varlen_fwd(x, w, b, True, seq, out)
    (name, V), = lib.calls
    w_used, b_used = _operands(rec, w, b, dtype)
    assert name == "dimsum_causal_conv1d_varlen_fwd" and (got is out if given else got.shape == x.shape and got.dtype == dtype)
    assert V == {"struct_size": C.sizeof(_lib.ConvVarlenParams), "reserved": 0, "conv": _conv_fields(x, w_used, b_used, True, got, dtype), **_ids_fields(seq)}
    assert rec.of(x) == ([], x) and rec.of(seq) == ([], seq)


def _pool(dtype, slots=5):
    """a non-contiguous (slots, dim, width) slice of a larger pool: strides (2 dim (width + 1), width + 1, 1)"""
    return torch.zeros(2 * slots, FD, FW + 1, dtype=dtype)[1::2, :, 1:]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("given", [False, True], ids=["out_omitted", "out_given"])
def test_varlen_states_fwd_fill(filled, dtype, given):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, b), seq = _half_x(dtype), _wb(dtype), _ids()
    ends = torch.tensor([[-1, 3, -1, -1, 0], [1, -1, 4, -1, 2]], dtype=torch.int32)
    pool = _pool(dtype)
    out = torch.empty(FB, 2 * FD, FL, dtype=dtype)[:, :FD] if given else None
    got = native.causal_conv1d_varlen_states_fwd(x, w, b, False, seq, ends, pool, out)
    (name, E), = lib.calls
    w_used, b_used = _operands(rec, w, b, dtype)
    assert name == "dimsum_causal_conv1d_varlen_states_fwd" and (got is out if given else got.shape == x.shape and got.dtype == dtype)
    assert E == {"struct_size": C.sizeof(_lib.ConvVarlenStatesParams), "num_slots": 5,
                 "varlen": {"struct_size": 0, "reserved": 0, "conv": _conv_fields(x, w_used, b_used, False, got, dtype), **_ids_fields(seq)},
                 "end_slots_ptr": ends.data_ptr(), "end_slots_batch_stride": FL, "state_ptr": pool.data_ptr(),
                 "state_slot_stride": 2 * FD * (FW + 1), "state_c_stride": FW + 1, "state_w_stride": 1, "state_dtype": _CODE[dtype], "reserved": 0}
    assert rec.of(pool) == ([], pool) and rec.of(x) == ([], x)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("given", [False, True], ids=["dx_omitted", "dx_given"])
def test_varlen_bwd_fill(filled, dtype, given):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, b), seq = _half_x(dtype), _wb(dtype), _ids()
    dout = torch.randn(FB, 3 * FD, FL).to(dtype)[:, FD:2 * FD]
    dx_given = torch.empty(FB, 2 * FD, FL, dtype=dtype)[:, :FD] if given else None
    res = native.causal_conv1d_varlen_bwd(x, w, b, dout, dx_given, False, seq)
    (name, V), = lib.calls
    w_used, b_used = _operands(rec, w, b, dtype)
    _check_grads(res, dx_given, w, b, dtype)
    Q = V["conv"]
    assert name == "dimsum_causal_conv1d_varlen_bwd" and V["struct_size"] == C.sizeof(_lib.ConvVarlenBwdParams) and V["reserved"] == 0
    assert {k: V[k] for k in ("seq_idx_ptr", "seq_idx_batch_stride")} == _ids_fields(seq) and set(V) == {"struct_size", "reserved", "conv", "seq_idx_ptr", "seq_idx_batch_stride"}
    assert Q["struct_size"] == 0 and Q["reserved"] == 0 and Q["fwd"] == _conv_fields(x, w_used, b_used, False, None, dtype)
    assert Q["dweight_ptr"] and Q["dbias_ptr"] == Q["dweight_ptr"] + 4 * FD * FW
    assert {k: v for k, v in Q.items() if k not in ("struct_size", "reserved", "fwd")} == _bwd_fields(dout, res[0], Q["dweight_ptr"], Q["dbias_ptr"])


def _state_fields(x, state, w_used, b_used, out, silu, dtype, seqlen):
    """the fields dimsum_conv_update_params_t and dimsum_conv_chunk_params_t share"""
    return {"batch": FB, "dim": FD, "width": FW, "silu_activation": int(silu), "dtype": _CODE[dtype], **({} if seqlen is None else {"seqlen": seqlen}),
            "x_batch_stride": x.stride(0), "x_c_stride": x.stride(1), "state_batch_stride": state.stride(0), "state_c_stride": state.stride(1),
            "state_w_stride": state.stride(2), "weight_c_stride": FW, "weight_width_stride": 1, "out_batch_stride": out.stride(0), "out_c_stride": out.stride(1),
            "x_ptr": x.data_ptr(), "weight_ptr": w_used.data_ptr(), "bias_ptr": b_used.data_ptr() if b_used is not None else None,
            "conv_state_ptr": state.data_ptr(), "out_ptr": out.data_ptr()}


def _strided_bias(dtype):
    """update and chunk take a bias of any stride: every other element of a longer vector"""
    return torch.randn(2 * FD).to(dtype)[::2]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("slots", [False, True], ids=["rows", "state_indices"])
def test_update_fill(filled, dtype, slots):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, _), b = torch.randn(FB, 2 * FD).to(dtype)[:, FD:], _wb(dtype), _strided_bias(dtype)
    state = _pool(dtype, 5 if slots else FB)
    idx = torch.tensor([3, -1], dtype=torch.int32).as_subclass(_OnGpu) if slots else None
    out = native.causal_conv1d_update(x, state, w, b, True, state_indices=idx) if slots else native.causal_conv1d_update(x, state, w, b, True)
    (name, S), = lib.calls
    # the strided bias is made fp32 AND contiguous: one copy for float16 (.float() packs it), .contiguous() for float32
    (w_ops, w_used), (b_ops, b_used) = rec.of(w), rec.of(b)
    assert w_ops == ([] if dtype == torch.float32 else ["float"]) and b_ops == (["contiguous"] if dtype == torch.float32 else ["float"])
    assert b_used.dtype == torch.float32 and b_used.is_contiguous() and w_used.dtype == torch.float32
    assert out.shape == x.shape and out.dtype == dtype and out.is_contiguous() and rec.of(state) == ([], state) and rec.of(x) == ([], x)
    want = {"struct_size": C.sizeof(_lib.ConvUpdateParams), "reserved": [0, 0], **_state_fields(x, state, w_used, b_used, out, True, dtype, None)}
    if slots:
        assert name == "dimsum_causal_conv1d_update_slots"
        assert S == {"struct_size": C.sizeof(_lib.ConvUpdateSlotsParams), "num_slots": 5, "conv": {**want, "struct_size": 0}, "slots_ptr": idx.data_ptr(), "slots_stride": 1}
    else:
        assert name == "dimsum_causal_conv1d_update" and S == want


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_chunk_fill(filled, dtype):
    from dimsum_amd import native
    lib, rec = filled
    x, (w, _), b = _half_x(dtype), _wb(dtype), _strided_bias(dtype)
    state = _pool(dtype, FB)
    out = native.causal_conv1d_chunk(x, state, w, b, False)
    (name, P), = lib.calls
    (w_ops, w_used), (b_ops, b_used) = rec.of(w), rec.of(b)
    assert w_ops == ([] if dtype == torch.float32 else ["float"]) and b_ops == (["contiguous"] if dtype == torch.float32 else ["float"])
    assert out.shape == x.shape and out.dtype == dtype and out.stride(2) == 1 and rec.of(state) == ([], state) and rec.of(x) == ([], x)
    assert name == "dimsum_causal_conv1d_chunk"
    assert P == {"struct_size": C.sizeof(_lib.ConvChunkParams), "reserved": 0, **_state_fields(x, state, w_used, b_used, out, False, dtype, FL)}
    # a d-major x (the mixer's layout) keeps its layout in out
    xd = torch.randn(FD, FB, FL).to(dtype).permute(1, 0, 2)
    out = native.causal_conv1d_chunk(xd, state, w, None, True)
    name, P = lib.calls[-1]
    assert out.stride() == xd.stride() and (P["out_batch_stride"], P["out_c_stride"], P["bias_ptr"], P["silu_activation"]) == (FL, FB * FL, None, 1)


def test_empty_inputs_launch_nothing(filled):
    from dimsum_amd import native
    lib, _ = filled
    w, b = _wb(torch.float32)
    seq, ends = torch.zeros(0, FL, dtype=torch.int32), torch.zeros(0, FL, dtype=torch.int32)
    x = torch.randn(0, FD, FL)
    assert native.causal_conv1d_fwd(x, w, b, True).shape == (0, FD, FL)
    assert native.causal_conv1d_varlen_fwd(x, w, b, True, seq).shape == (0, FD, FL)
    assert native.causal_conv1d_varlen_states_fwd(x, w, b, True, seq, ends, _pool(torch.float32)).shape == (0, FD, FL)
    for res in (native.causal_conv1d_bwd(x, w, b, x, None, True), native.causal_conv1d_varlen_bwd(x, w, b, x, None, True, seq)):
        assert res[0].shape == (0, FD, FL) and res[1].shape == w.shape and res[2].shape == b.shape and not res[1].any() and not res[2].any()
    assert native.causal_conv1d_update(torch.randn(0, FD), torch.zeros(0, FD, FW), w, b, True).shape == (0, FD)
    assert not lib.calls


def test_refusals_fire_in_their_order():
    """on plain CPU tensors, nothing replaced: shape, dtype and stride refusals come before the device is looked at, in this order"""
    from dimsum_amd import native
    f32 = torch.float32
    x, (w, b), seq = _half_x(f32), _wb(f32), _ids()
    xcl = torch.randn(FB, FL, FD).transpose(1, 2)
    ends, pool = torch.full((FB, FL), -1, dtype=torch.int32), _pool(f32)
    cpu = "no CPU fallback"

    def refused(msg, fn, *a, **k):
        with pytest.raises(RuntimeError) as e:
            fn(*a, **k)
        assert msg in str(e.value), str(e.value)

    # the plain pair: the device first (the reference's order), then the shapes
    refused(cpu, native.causal_conv1d_fwd, x[0], w, b, True)
    refused(cpu, native.causal_conv1d_bwd, x, w[:, :1], b, x, None, True)
    # packed rows: rank, ids, then the plain checks (device first among them), the layout after those
    refused("causal_conv1d: x must be (batch, dim, seqlen)", native.causal_conv1d_varlen_fwd, x[0], w, b, True, seq.long())
    refused(f"causal_conv1d_varlen_fwd: seq_idx must be a contiguous int32 (batch, seqlen) = ({FB}, {FL}) tensor", native.causal_conv1d_varlen_fwd, xcl, w[:, :1], b, True, seq.long())
    refused(f"causal_conv1d_varlen_bwd: seq_idx must be a contiguous int32 (batch, seqlen) = ({FB}, {FL}) tensor", native.causal_conv1d_varlen_bwd, xcl, w, b, x, None, True, seq[:, :4])
    refused(cpu, native.causal_conv1d_varlen_fwd, xcl, w, b, True, seq)
    refused(cpu, native.causal_conv1d_varlen_bwd, xcl, w, b, x, None, True, seq)
    # ... with states: seq_idx, end_slots, the pool's shape, its dtype, then the plain checks
    who = "causal_conv1d_varlen_states_fwd"
    refused(f"{who}: seq_idx must be a contiguous int32", native.causal_conv1d_varlen_states_fwd, x, w, b, True, None, ends.long(), pool[0])
    refused(f"{who}: end_slots must be a contiguous int32 (batch, seqlen) = ({FB}, {FL}) tensor", native.causal_conv1d_varlen_states_fwd, x, w, b, True, seq, ends.long(), pool[0])
    refused(f"{who}: conv_state must be a pool (num_slots >= 1, dim, width)", native.causal_conv1d_varlen_states_fwd, x, w, b, True, seq, ends, pool.half()[:, :, :2])
    refused(f"{who}: conv_state must have x's dtype torch.float32, got torch.float16", native.causal_conv1d_varlen_states_fwd, xcl, w, b, True, seq, ends, pool.half())
    refused(cpu, native.causal_conv1d_varlen_states_fwd, xcl, w, b, True, seq, ends, pool)
    # the update: state_indices (down to its device) before anything else, then the device
    idx = torch.tensor([3, -1], dtype=torch.int32)
    refused("causal_conv1d_update: state_indices must be an int32 tensor", native.causal_conv1d_update, x[:, :, 0], pool, w[:, :1], b, True, idx.long())
    refused("causal_conv1d_update: state_indices must have batch = 2 entries, got 1", native.causal_conv1d_update, x[:, :, 0], pool, w, b, True, idx[:1])
    refused("causal_conv1d_update: state_indices must be a GPU tensor on x's device", native.causal_conv1d_update, x[:, :, 0], pool, w[:, :1], b, True, idx)
    refused(cpu, native.causal_conv1d_update, x, pool[:FB], w[:, :1], b, True)
    # the chunk: every shape, dtype and stride refusal before the device
    st = pool[:FB]
    refused("causal_conv1d_chunk: x must be (batch, dim, seqlen) in float32", native.causal_conv1d_chunk, x[0], st, w[:, :1], b, True)
    refused("causal_conv1d_chunk: x must not be empty", native.causal_conv1d_chunk, x[:0], st, w[:, :1], b, True)
    refused("causal_conv1d_chunk: weight must be (dim, width)", native.causal_conv1d_chunk, x, st, w[:4, :1], b, True)
    refused("causal_conv1d_chunk only supports width between 2 and 4", native.causal_conv1d_chunk, x, st.half(), w[:, :1], b, True)
    refused("causal_conv1d_chunk: conv_state must be (batch, dim, width) of x's dtype", native.causal_conv1d_chunk, x, st.half(), w, b[:4], True)
    refused("causal_conv1d_chunk: bias must be (dim,)", native.causal_conv1d_chunk, xcl, st, w, b[:4], True)
    refused("causal_conv1d_chunk: x.stride(-1) must be 1", native.causal_conv1d_chunk, xcl, st, w, b, True)
    refused(cpu, native.causal_conv1d_chunk, x, st, w, b, True)


def test_routed_refusals_keep_their_sentences(filled):
    """past the device: the refusals of the plain checks and of out / dout / dx, each with its entry's name"""
    from dimsum_amd import native
    lib, _ = filled
    f32 = torch.float32
    x, (w, b), seq = _half_x(f32), _wb(f32), _ids()
    xcl = torch.randn(FB, FL, FD).transpose(1, 2)
    ends, pool = torch.full((FB, FL), -1, dtype=torch.int32), _pool(f32)
    bad = torch.empty(FB, FL, FD).transpose(1, 2)                   # right shape, not seqlen-contiguous

    def refused(msg, fn, *a, **k):
        with pytest.raises(RuntimeError) as e:
            fn(*a, **k)
        assert msg in str(e.value), str(e.value)

    refused("causal_conv1d: x must be (batch, dim, seqlen)", native.causal_conv1d_fwd, x[0], w, b, True)
    refused("causal_conv1d: input must be float32, float16 or bfloat16", native.causal_conv1d_fwd, x.double(), w, b, True)
    refused("only seqlen-contiguous", native.causal_conv1d_fwd, torch.randn(FB, 2 * FD, 2 * FL)[:, ::2, ::2], w, b, True)
    refused("causal_conv1d: weight must be (dim, width)", native.causal_conv1d_fwd, x, w[:4], b, True)
    refused("causal_conv1d only supports width between 2 and 4", native.causal_conv1d_fwd, x, w[:, :1], b[:4], True)
    refused("causal_conv1d: bias must be (dim,)", native.causal_conv1d_fwd, x, w, b[:4], True)
    for fn, args in ((native.causal_conv1d_varlen_fwd, (seq,)), (native.causal_conv1d_varlen_states_fwd, (seq, ends, pool))):
        refused(f"{fn.__name__}: seq_idx needs a seqlen-contiguous x (the channel-last kernels take none)", fn, xcl, w, b, True, *args)
        refused(f"{fn.__name__}: bad out", fn, x, w, b, True, *args, bad)
        refused(f"{fn.__name__}: bad out", fn, x, w, b, True, *args, torch.empty(FB, FD, FL, dtype=torch.float16))
    refused("causal_conv1d_varlen_bwd: seq_idx needs a seqlen-contiguous x (the channel-last kernels take none)", native.causal_conv1d_varlen_bwd, xcl, w, b, x, None, True, seq)
    for who, extra in (("causal_conv1d_bwd", ()), ("causal_conv1d_varlen_bwd", (seq,))):
        fn = getattr(native, who)
        refused(f"{who}: bad dout", fn, x, w, b, bad, None, True, *extra)
        refused(f"{who}: bad dout", fn, x, w, b, x[:, :4], None, True, *extra)
        refused(f"{who}: bad dx", fn, x, w, b, x, bad, True, *extra)
    refused("causal_conv1d_bwd: bad dout", native.causal_conv1d_bwd, xcl, w, b, x.half(), None, True)
    refused("causal_conv1d_bwd: bad dx", native.causal_conv1d_bwd, xcl, w, b, x, torch.empty(FB, FD, FL), True)
    st = pool[:FB]
    refused("causal_conv1d_update: x must be (batch, dim) in float32, float16 or bfloat16", native.causal_conv1d_update, x, st, w, b, True)
    refused("causal_conv1d_update: weight must be (dim, width)", native.causal_conv1d_update, x[:, :, 0], st, w[:4, :1], b, True)
    refused("causal_conv1d_update only supports width between 2 and 4", native.causal_conv1d_update, x[:, :, 0], st.half(), w[:, :1], b, True)
    refused("causal_conv1d_update: conv_state must be (batch, dim, width) of x's dtype", native.causal_conv1d_update, x[:, :, 0], pool, w, b[:4], True)
    refused("causal_conv1d_update: with state_indices conv_state must be a pool (num_slots >= 1, dim, width) of x's dtype", native.causal_conv1d_update,
            x[:, :, 0], pool.half(), w, b[:4], True, state_indices=torch.tensor([0, 1], dtype=torch.int32).as_subclass(_OnGpu))
    refused("causal_conv1d_update: bias must be (dim,)", native.causal_conv1d_update, x[:, :, 0], st, w, b[:4], True)
    assert not lib.calls
