"""bimamba_inner_fn without a GPU: the reference's signature, the out-of-scope inputs, no CPU fallback, and the C ABI of the bidirectional
scan (struct layouts against include/dimsum_hip.h, struct_size checked before anything is read). Nothing here launches a kernel."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mamba/mamba_ssm/ops/selective_scan_interface.py:1351-1388, in order
REF_PARAMS = ["xz", "conv1d_weight", "conv1d_bias", "x_proj_weight", "delta_proj_weight", "out_proj_weight", "out_proj_bias", "A", "A_b",
              "B", "C", "D", "delta_bias", "B_proj_bias", "C_proj_bias", "delta_softplus"]
REF_DEFAULTS = {"B": None, "C": None, "D": None, "delta_bias": None, "B_proj_bias": None, "C_proj_bias": None, "delta_softplus": True}


def test_signature_is_the_references():
    from dimsum_amd.ops import bimamba_inner_fn
    sig = inspect.signature(bimamba_inner_fn)
    assert list(sig.parameters) == REF_PARAMS
    for name, p in sig.parameters.items():
        if name in REF_DEFAULTS:
            assert p.default is REF_DEFAULTS[name] or p.default == REF_DEFAULTS[name], name
        else:
            assert p.default is inspect.Parameter.empty, name


def _args(B=1, Dm=8, L=16, N=4, R=2, W=4, dtype=torch.float32):
    D = 2 * Dm
    return dict(xz=torch.randn(B, 2 * D, L, dtype=dtype), conv1d_weight=torch.randn(D, 1, W), conv1d_bias=torch.randn(D),
                x_proj_weight=torch.randn(R + 2 * N, D), delta_proj_weight=torch.randn(D, R), out_proj_weight=torch.randn(Dm, D),
                out_proj_bias=None, A=-torch.rand(D, N), A_b=-torch.rand(D, N), D=torch.randn(D), delta_bias=torch.rand(D))


def test_out_of_scope_inputs_raise():
    from dimsum_amd.ops import bimamba_inner_fn
    a = _args()
    with pytest.raises(NotImplementedError, match="complex A is outside this build's scope"):
        bimamba_inner_fn(**{**a, "A": torch.complex(a["A"], a["A"])})
    with pytest.raises(NotImplementedError, match="complex A is outside this build's scope"):
        bimamba_inner_fn(**{**a, "A_b": torch.complex(a["A_b"], a["A_b"])})
    D, N = a["A"].shape
    with pytest.raises(NotImplementedError, match="constant B/C is outside this build's scope"):
        bimamba_inner_fn(**a, B=torch.randn(D, N))
    with pytest.raises(NotImplementedError, match="constant B/C is outside this build's scope"):
        bimamba_inner_fn(**a, C=torch.randn(D, N))


@pytest.mark.parametrize("grad", [False, True])
def test_no_cpu_fallback(grad):
    from dimsum_amd.ops import bimamba_inner_fn
    a = _args()
    if grad:
        a["xz"].requires_grad_()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bimamba_inner_fn(**a)
    from dimsum_amd import native
    u = torch.randn(1, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.selective_scan_bidir_fwd(u, u, -torch.rand(4, 4), -torch.rand(4, 4), torch.randn(1, 1, 4, 8), torch.randn(1, 1, 4, 8),
                                        None, u, None, True)


def _header_layout(pairs):
    body = ""
    for cname, mirror in pairs:
        body += f'printf("{cname} %zu", sizeof({cname}));'
        body += "".join(f'printf(" {f}=%zu", offsetof({cname}, {f}));' for f, _ in mirror._fields_)
        body += 'printf("\\n");'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dimsum_hip.h"\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout
    layout = {}
    for line in out.strip().splitlines():
        name, size, *fields = line.split()
        layout[name] = (int(size), {f.split("=")[0]: int(f.split("=")[1]) for f in fields})
    return layout


def test_bidir_structs_match_header():
    from dimsum_amd import _lib
    pairs = [("dimsum_ssm_bidir_params_t", _lib.SsmBidirParams), ("dimsum_ssm_bidir_bwd_params_t", _lib.SsmBidirBwdParams)]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offs = layout[cname]
        assert size == ctypes.sizeof(mirror), cname
        assert offs == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}, cname
        assert mirror._fields_[0][0] == "struct_size" and mirror().struct_size == size, cname


def test_abi_version_and_exports():
    from dimsum_amd import _lib
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18
    for name in ("dimsum_ssm_scan_bidir_fwd", "dimsum_ssm_scan_bidir_bwd", "dimsum_ssm_scan_bidir_fwd_variant"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "dimsum_hip.h")).read()
    assert "#define DIMSUM_ABI_VERSION 18" in text


def test_wrong_struct_size_is_refused_before_anything_is_read():
    """DIMSUM_ERR_ABI (7) for a stale or foreign struct_size; the right size gets past the check and fails on its NULL pointers (no launch)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    for fn, mirror in ((lib.dimsum_ssm_scan_bidir_fwd, _lib.SsmBidirParams), (lib.dimsum_ssm_scan_bidir_bwd, _lib.SsmBidirBwdParams)):
        P = mirror()
        assert fn(P, None) == 1, mirror                                       # DIMSUM_ERR_NULL
        for bad in (0, ctypes.sizeof(mirror) - 8, ctypes.sizeof(mirror) + 8, ctypes.sizeof(_lib.SsmParams)):
            P.struct_size = bad
            assert fn(P, None) == 7, (mirror, bad)
    assert lib.dimsum_ssm_scan_bidir_fwd(None, None) == 1


def test_kernel_query():
    """every shape the scan takes is served in both directions: by the 64-channel kernel, or by one lane per state where the library picks
    that kernel (dstate 16, a launch far from filling the chip); invalid parameters -> -1"""
    from dimsum_amd import _lib, native
    for shape, v in (((256, 1024, 256, 16), 1), ((1, 80, 333, 8), 1), ((2, 64, 4096, 4), 1), ((3, 96, 7, 32), 1), ((1, 1, 1, 16), 16),
                     ((4, 256, 512, 16), 16), ((64, 1152, 1024, 16), 1)):
        assert native.scan_bidir_fwd_kernel_for(*shape) == v, shape
        assert v == 1 or native.scan_fwd_kernel_for(*shape) == v, shape
    with native.scan_fwd_variant(1):
        assert native.scan_bidir_fwd_kernel_for(4, 256, 512, 16) == 1
    assert native.scan_bidir_fwd_kernel_for(2, 64, 256, 12) == -1           # dstate the kernels are not built for
    assert native.scan_bidir_fwd_kernel_for(2, 64, 256, 16, n_groups=3) == -1
    P = _lib.SsmBidirParams()
    P.fwd.batch, P.fwd.dim, P.fwd.seqlen, P.fwd.dstate, P.fwd.n_groups, P.fwd.n_chunks = 256, 1024, 256, 16, 1, 1
    assert _lib.load().dimsum_ssm_scan_bidir_fwd_variant(P) == 1
    P.struct_size = 8
    assert _lib.load().dimsum_ssm_scan_bidir_fwd_variant(P) == -1
