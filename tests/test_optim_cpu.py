"""The fused training-step tail without a GPU: the C ABI of dimsum_optim_* (exports, struct layout against include/dimsum_hip.h, struct_size
checked before anything is read), the scope errors of FusedAdamWEMA, the chunk table, and the default of build_training. Nothing here
launches a kernel."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dimsum_optim_grad_sumsq", "dimsum_optim_adamw_ema_step", "dimsum_optim_write_ptrs")


def _header_layout(pairs):
    """{c struct: (sizeof, {field: offset})} from a C program compiled against include/dimsum_hip.h; pairs: [(c struct, ctypes mirror)]"""
    body = ""
    for cname, mirror in pairs:
        body += f'printf("{cname} %zu", sizeof({cname}));'
        body += "".join(f'printf(" {f}=%zu", offsetof({cname}, {f}));' for f, _ in mirror._fields_)
        body += 'printf("\\n");'
    body += 'printf("CHUNK %d\\nMAX_PARTIALS %d\\n", DIMSUM_OPTIM_CHUNK, DIMSUM_OPTIM_MAX_PARTIALS);'
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


def test_symbols_are_exported_under_abi_18():
    from dimsum_amd import _lib
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18
    header = open(os.path.join(ROOT, "include", "dimsum_hip.h")).read()
    assert "#define DIMSUM_ABI_VERSION 18" in header
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name


def test_struct_matches_header():
    from dimsum_amd import _lib
    layout = _header_layout([("dimsum_optim_params_t", _lib.OptimParams)])
    size, offs = layout["dimsum_optim_params_t"]
    assert size == ctypes.sizeof(_lib.OptimParams)
    assert offs == {f: getattr(_lib.OptimParams, f).offset for f, _ in _lib.OptimParams._fields_}
    assert _lib.OptimParams._fields_[0][0] == "struct_size" and _lib.OptimParams().struct_size == size
    assert layout["CHUNK"][0] == _lib.OPTIM_CHUNK and layout["MAX_PARTIALS"][0] == _lib.OPTIM_MAX_PARTIALS


def test_wrong_struct_size_is_refused_before_anything_is_read():
    """DIMSUM_ERR_NULL (1) for NULL; DIMSUM_ERR_ABI (7) for a stale or foreign struct_size; the right size gets past that check and fails on
    the struct's NULL tables (no launch)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    size = ctypes.sizeof(_lib.OptimParams)
    for fn in (lib.dimsum_optim_grad_sumsq, lib.dimsum_optim_adamw_ema_step):
        assert fn(None, None) == 1
        P = _lib.OptimParams()
        P.n_tensors, P.n_chunks = 1, 1
        assert fn(P, None) == 1                                               # past the size check: the tables are NULL
        for bad in (0, size - 8, size + 8):
            P.struct_size = bad
            assert fn(P, None) == 7, bad
    assert lib.dimsum_optim_write_ptrs(None, 0, None, 0, None) == 1


def test_chunk_table():
    """one row (tensor, chunk within the tensor) per 4096 elements, in list order"""
    from dimsum_amd import _lib, native
    C = _lib.OPTIM_CHUNK
    numel, chunks = native.optim_tables([1, C, C + 1, 3 * C - 1], "cpu")
    assert numel.tolist() == [1, C, C + 1, 3 * C - 1] and numel.dtype == torch.int64
    assert chunks.dtype == torch.int32 and chunks.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [3, 0], [3, 1], [3, 2]]
    with pytest.raises(RuntimeError):
        native.optim_tables([], "cpu")
    with pytest.raises(RuntimeError):
        native.optim_tables([4, 0], "cpu")


def test_cpu_parameters_are_refused():
    from dimsum_amd.optim import FusedAdamWEMA
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAdamWEMA([torch.nn.Parameter(torch.zeros(4))], lr=1e-4)


def test_out_of_scope_options_are_refused():
    from dimsum_amd.optim import FusedAdamWEMA
    p = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(fused=False)):
        with pytest.raises(ValueError):
            FusedAdamWEMA(p, **kw)
    assert issubclass(FusedAdamWEMA, torch.optim.AdamW)


def test_build_training_default_is_torch_adamw(monkeypatch):
    from dimsum_amd import train
    from dimsum_amd.optim import FusedAdamWEMA
    monkeypatch.delenv("DIMSUM_FUSED_STEP", raising=False)
    model, ema, opt = train.build_training(torch.nn.Linear(4, 4), "cpu")
    assert type(opt) is torch.optim.AdamW and not hasattr(opt, "step_fused")
    assert "fused_step" in train.build_training.__code__.co_varnames
    monkeypatch.setenv("DIMSUM_FUSED_STEP", "1")                             # on: the fused optimizer, which has no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.build_training(torch.nn.Linear(4, 4), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.build_training(torch.nn.Linear(4, 4), "cpu", fused_step=True)
    monkeypatch.setenv("DIMSUM_FUSED_STEP", "0")
    assert type(train.build_training(torch.nn.Linear(4, 4), "cpu")[2]) is torch.optim.AdamW
    assert FusedAdamWEMA.step_fused is not None
