"""The channel-last causal conv1d without a GPU: the two entries in the header, the loader and the built library, the layout of their
parameter structs, the library's host-side refusals (they return before any launch), and the layout routing of dimsum_amd.native and
causal_conv1d_fn, observed through stand-ins for the library calls that record the struct they are given."""
import ctypes

import pytest
import torch

from test_conv_host_cpu import routed  # noqa: F401  (the recording library: a fixture both files use)
from test_host_logic import _header_layout

OK, ERR_NULL, ERR_DTYPE, ERR_SHAPE, ERR_STRIDE, ERR_ABI = 0, 1, 2, 3, 4, 7
ENTRIES = (("dimsum_causal_conv1d_cl_fwd", "ConvClParams"), ("dimsum_causal_conv1d_cl_bwd", "ConvClBwdParams"))
OLD_MESSAGE = "only seqlen-contiguous"


def test_entries_are_declared_exported_and_built():
    from dimsum_amd import _lib, native
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    for name, mirror in ENTRIES:
        assert f"int {name}(" in header and name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes[0]._type_ is getattr(_lib, mirror)
    assert f"#define DIMSUM_CONV_CL_CHUNK {native.CONV_CL_CHUNK}\n" in header


def test_struct_layouts_match_the_header():
    from dimsum_amd import _lib
    pairs = [("dimsum_conv_cl_params_t", _lib.ConvClParams), ("dimsum_conv_cl_bwd_params_t", _lib.ConvClBwdParams),
             ("dimsum_conv_params_t", _lib.ConvParams), ("dimsum_conv_bwd_params_t", _lib.ConvBwdParams)]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offs = layout[cname]
        assert size == ctypes.sizeof(mirror), cname
        assert offs == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}, cname
        assert mirror._fields_[0][0] == "struct_size" and mirror().struct_size == size, cname
    assert [f for f, _ in _lib.ConvClParams._fields_[:2]] == ["struct_size", "reserved"]
    assert layout["dimsum_conv_params_t"][0] == 112 and layout["dimsum_conv_bwd_params_t"][0] == 200    # the existing structs as they were


def _filled(bwd):
    """a struct of valid sizes whose pointers all point at host memory nobody dereferences: the checks return before a launch"""
    from dimsum_amd import _lib
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    Q = _lib.ConvClBwdParams() if bwd else _lib.ConvClParams()
    P = Q.fwd if bwd else Q
    P.batch, P.dim, P.seqlen, P.width, P.dtype = 1, 4, 4, 4, 0
    P.x_ptr = P.weight_ptr = P.bias_ptr = P.out_ptr = addr
    P.x_batch_stride, P.x_l_stride, P.weight_c_stride, P.weight_width_stride, P.out_batch_stride, P.out_l_stride = 16, 4, 4, 1, 16, 4
    if bwd:
        Q.dout_ptr = Q.dx_ptr = Q.dweight_ptr = Q.dbias_ptr = addr
        Q.dout_batch_stride, Q.dout_l_stride, Q.dx_batch_stride, Q.dx_l_stride, Q.dweight_c_stride, Q.dweight_width_stride = 16, 4, 16, 4, 4, 1
    return Q, P, buf


@pytest.mark.parametrize("bwd", [False, True])
def test_library_refusals_without_a_device(bwd):
    from dimsum_amd import _lib
    lib = _lib.load()
    fn = lib.dimsum_causal_conv1d_cl_bwd if bwd else lib.dimsum_causal_conv1d_cl_fwd
    assert fn(None, None) == ERR_NULL
    # a wrong struct_size is refused before any pointer is looked at: every pointer is NULL here
    for size in (0, -8, 8):
        Q = (_lib.ConvClBwdParams if bwd else _lib.ConvClParams)()
        Q.struct_size = size if size == 0 else Q.struct_size + size
        assert fn(Q, None) == ERR_ABI, size
    required = ("x_ptr", "weight_ptr") + (("dout_ptr", "dx_ptr", "dweight_ptr") if bwd else ("out_ptr",))
    for name in required:
        Q, P, buf = _filled(bwd)
        P.width = 7                                                 # a NULL pointer is reported before the bad width
        setattr(P if hasattr(type(P), name) else Q, name, None)
        assert fn(Q, None) == ERR_NULL, name
    for field, value in (("width", 1), ("width", 5), ("dim", 0), ("seqlen", 0), ("batch", -1)):
        Q, P, buf = _filled(bwd)
        P.dtype = 3                                                 # a bad size is reported before the bad dtype
        setattr(P, field, value)
        assert fn(Q, None) == ERR_SHAPE, (field, value)
    Q, P, buf = _filled(bwd)
    P.dtype = 3
    P.x_l_stride = -4                                               # a bad dtype is reported before the bad stride
    assert fn(Q, None) == ERR_DTYPE
    strides =[("fwd", n) for n in ("x_batch_stride", "x_l_stride", "weight_c_stride", "weight_width_stride")]
    strides += [("bwd", n) for n in ("dout_batch_stride", "dout_l_stride", "dx_batch_stride", "dx_l_stride", "dweight_c_stride",
                                     "dweight_width_stride")] if bwd else [("fwd", "out_batch_stride"), ("fwd", "out_l_stride")]
    for where, name in strides:
        Q, P, buf = _filled(bwd)
        P.batch = 0                                                 # a negative stride is reported even when nothing would be launched
        setattr(P if where == "fwd" else Q, name, -1)
        assert fn(Q, None) == ERR_STRIDE, name
    Q, P, buf = _filled(bwd)
    P.batch = 0
    assert fn(Q, None) == OK                                        # an empty batch launches nothing


def test_cpu_tensors_are_refused():
    from dimsum_amd import native
    w, b = torch.randn(8, 4), torch.randn(8)
    x = torch.randn(2, 5, 8).transpose(1, 2)
    for t in (x, x.contiguous()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            native.causal_conv1d_fwd(t, w, b, True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            native.causal_conv1d_bwd(t, w, b, t, None, True)


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
B, D, L, W = 2, 8, 5, 4


def _wb():
    return torch.randn(D, W), torch.randn(D)


def test_channel_last_reaches_the_new_entry_without_a_copy(routed):
    from dimsum_amd import native
    lib, copies = routed
    w, b = _wb()
    x = torch.randn(B, L, D).transpose(1, 2)
    out = native.causal_conv1d_fwd(x, w, b, True)
    (name, P), = lib.calls
    assert name == "dimsum_causal_conv1d_cl_fwd" and P["x_ptr"] == x.data_ptr() and not copies
    assert (P["batch"], P["dim"], P["seqlen"], P["width"], P["silu_activation"], P["dtype"]) == (B, D, L, W, 1, 0)
    assert (P["x_batch_stride"], P["x_l_stride"], P["out_batch_stride"], P["out_l_stride"]) == (L * D, D, L * D, D)
    assert out.shape == x.shape and out.stride() == (L * D, 1, D) and P["out_ptr"] == out.data_ptr()
    assert (P["weight_c_stride"], P["weight_width_stride"]) == (W, 1) and P["bias_ptr"]


def test_half_of_a_wider_buffer_is_a_view(routed):
    from dimsum_amd import native
    lib, copies = routed
    w, b = _wb()
    xz = torch.randn(B, L, 2 * D)
    for lo in (0, D):
        x = xz[..., lo:lo + D].transpose(1, 2)
        native.causal_conv1d_fwd(x, w, None, False)
        name, P = lib.calls[-1]
        assert name == "dimsum_causal_conv1d_cl_fwd" and not copies
        assert P["x_ptr"] == xz.data_ptr() + 4 * lo and P["x_l_stride"] == 2 * D and P["x_batch_stride"] == 2 * D * L
        assert P["out_l_stride"] == D and P["bias_ptr"] is None and P["silu_activation"] == 0


def test_seqlen_contiguous_inputs_stay_with_the_old_entry(routed):
    from dimsum_amd import native
    lib, copies = routed
    w, b = _wb()
    x = torch.randn(B, D, L)
    one = torch.randn(B, 1, D).transpose(1, 2)                      # shape[2] == 1 with channel stride 1: still the old kernel's
    assert one.shape == (B, D, 1) and one.stride(1) == 1
    for t in (x, one):
        out = native.causal_conv1d_fwd(t, w, b, True)
        name, P = lib.calls[-1]
        assert name == "dimsum_causal_conv1d_fwd" and P["x_ptr"] == t.data_ptr()
        assert (P["x_batch_stride"], P["x_c_stride"]) == (t.stride(0), t.stride(1)) and out.stride() == t.stride()
        dx, dw, db = native.causal_conv1d_bwd(t, w, b, t, None, True)
        name, Q = lib.calls[-1]
        assert name == "dimsum_causal_conv1d_bwd" and Q["fwd"]["x_ptr"] == t.data_ptr() and dx.is_contiguous()
    assert not copies


def test_neither_layout_is_refused_by_native_and_copied_once_by_the_function(routed):
    from dimsum_amd import native
    from dimsum_amd.ops.causal_conv1d_interface import causal_conv1d_fn
    lib, copies = routed
    w, b = _wb()
    x = torch.randn(B, 2 * D, 2 * L)[:, ::2, ::2]
    assert x.shape == (B, D, L) and x.stride(1) != 1 and x.stride(2) != 1
    with pytest.raises(RuntimeError, match=OLD_MESSAGE):
        native.causal_conv1d_fwd(x, w, b, True)
    with pytest.raises(RuntimeError, match=OLD_MESSAGE):
        native.causal_conv1d_bwd(x, w, b, x, None, True)
    assert not lib.calls and not copies
    out = causal_conv1d_fn(x, w, b, "silu")
    (name, P), = lib.calls
    assert name == "dimsum_causal_conv1d_fwd" and P["x_ptr"] != x.data_ptr() and (P["x_batch_stride"], P["x_c_stride"]) == (D * L, L)
    assert copies == [((B, D, L), x.stride())] and out.shape == x.shape


def test_function_keeps_channel_last_through_forward_and_backward(routed):
    from dimsum_amd.ops.causal_conv1d_interface import causal_conv1d_fn
    lib, copies = routed
    w, b = (t.requires_grad_() for t in _wb())
    leaf = torch.randn(B, L, D, requires_grad=True)
    x = leaf.transpose(1, 2)
    out = causal_conv1d_fn(x, w, b, "silu")
    assert out.stride() == (L * D, 1, D) and not copies
    out.backward(torch.randn(B, L, D).transpose(1, 2))             # a channel-last dout is passed as it is
    (n1, P), (n2, Q) = lib.calls
    assert (n1, n2) == ("dimsum_causal_conv1d_cl_fwd", "dimsum_causal_conv1d_cl_bwd") and not copies
    assert Q["fwd"]["x_ptr"] == P["x_ptr"] == leaf.data_ptr()       # the backward runs on the tensor the forward ran on
    assert (Q["dout_l_stride"], Q["dx_l_stride"], Q["dx_batch_stride"]) == (D, D, L * D)
    assert leaf.grad.shape == leaf.shape and w.grad.shape == w.shape and b.grad.shape == b.shape


def test_other_dout_is_converted_once_and_dx_is_channel_last(routed):
    from dimsum_amd import native
    lib, copies = routed
    w, b = _wb()
    x = torch.randn(B, L, D).transpose(1, 2)
    dout = torch.randn(B, D, L)
    dx, dw, db = native.causal_conv1d_bwd(x, w, b, dout, None, True)
    (name, Q), = lib.calls
    assert name == "dimsum_causal_conv1d_cl_bwd" and Q["fwd"]["x_ptr"] == x.data_ptr()
    assert copies == [((B, L, D), (D * L, 1, L))]                    # dout.transpose(1, 2).contiguous(): the one conversion
    assert Q["dout_ptr"] != dout.data_ptr() and (Q["dout_batch_stride"], Q["dout_l_stride"]) == (L * D, D)
    assert dx.stride() == (L * D, 1, D) and Q["dx_ptr"] == dx.data_ptr() and Q["dx_l_stride"] == D
    assert (Q["dweight_c_stride"], Q["dweight_width_stride"]) == (W, 1) and Q["dweight_ptr"] and Q["dbias_ptr"]
    assert dw.shape == w.shape and db.shape == b.shape
    given = torch.empty(B, L, 2 * D)[..., D:].transpose(1, 2)       # dx= as a view of a wider buffer
    dx2, _, _ = native.causal_conv1d_bwd(x, w, None, dout.transpose(1, 2).contiguous().transpose(1, 2), given, False)
    name, Q = lib.calls[-1]
    assert dx2 is given and Q["dx_ptr"] == given.data_ptr() and Q["dx_l_stride"] == 2 * D and Q["dbias_ptr"] is None
    with pytest.raises(RuntimeError, match="bad dx"):
        native.causal_conv1d_bwd(x, w, b, dout, torch.empty(B, D, L), True)
