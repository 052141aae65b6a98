"""The DCT-blurred path and the fused head without a GPU: dct_blur (the matrix-form torch expression) and training_losses with
path_args use_blurring=True against fixtures captured from the REFERENCE's own FFT-based code (tests/golden/transport_blur.npz,
tools/gen_golden.py:gen_transport_blur), what blurring must leave alone (u_t, the unblurred plan), the shape errors, train.py's flags, and
the C ABI of dimsum_fm_* (exports, struct layouts against include/dimsum_hip.h, struct_size checked first). Nothing here launches a kernel.
Tolerances are the transport's own (tests/test_transport_golden.py): the reference's FFT blur sits within 4.8e-7 of a float64 evaluation of
the matrix form at data scale 3.1, an fp32 matrix form within 4.4e-7, against a bound of 2e-6 x scale."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from procedural import seeded, toy_denoiser

from dimsum_amd.transport import create_transport
from dimsum_amd.transport.blurring import dct_blur, dct_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = dict(train_eps=1e-3, sample_eps=2e-3)
TOL = dict(rtol=2e-5, atol=0.0, scale_atol=2e-6)
LOSS_TOL = dict(rtol=1e-4, atol=0.0, scale_atol=1e-5)
SYMBOLS = ("dimsum_fm_plan", "dimsum_fm_loss_fwd", "dimsum_fm_loss_bwd")


def blur_case(g, tag):
    """-> (x, p, sigmas, expected) of one DCTBlur case of the fixture"""
    x = torch.from_numpy(seeded(tuple(int(v) for v in g[f"blur_{tag}_shape"]), int(g[f"blur_{tag}_x_seed"])))
    return x, int(g[f"blur_{tag}_p"]), torch.from_numpy(g[f"blur_{tag}_sigmas"]), g[f"blur_{tag}_out"]


def blur_path_args(g):
    return dict(use_blurring=True, blur_sigma_max=int(g["blur_sigma_max"]), blur_upscale=int(g["blur_upscale"]))


def check_blur_losses(dev, fused_head):
    """training_losses with blurring on against the fixture: t, x_t, the prediction and the loss of all five cases"""
    g = golden("transport_blur")
    x1, y = torch.from_numpy(g["loss_x1"]).to(dev), torch.from_numpy(g["y"]).to(dev)
    cases = [eval(c) for c in g["loss_cases"]]          # tuples of literals written by the generator
    assert len(cases) == 5
    for pt, pred, lw in cases:
        tag = f"loss_{pt}_{pred}_{lw}"
        tr = create_transport(pt, pred, lw, **EPS, path_args=blur_path_args(g), fused_head=fused_head)
        seen = {}

        def model(xt, t, y=None):
            seen["xt"], seen["t"] = xt, t
            return toy_denoiser(xt, t, y)

        torch.manual_seed(int(g[tag + "_seed"]))
        terms = tr.training_losses(model, x1, dict(y=y))
        assert_close(seen["t"].cpu(), g[tag + "_t"], what=tag + " t", **TOL)
        assert_close(seen["xt"].cpu(), g[tag + "_xt"], what=tag + " xt", **TOL)
        assert_close(terms["pred"].cpu(), g[tag + "_pred"], what=tag + " pred", **TOL)
        assert_close(terms["loss"].cpu(), g[tag + "_loss"], what=tag + " loss", **LOSS_TOL)


def test_dct_matrix_is_orthonormal():
    for p in (2, 4, 8, 16):
        c = dct_matrix(p, torch.float64)
        assert torch.allclose(c @ c.t(), torch.eye(p, dtype=torch.float64), atol=1e-14)


def test_dct_blur_matches_every_reference_fixture():
    g = golden("transport_blur")
    assert list(g["blur_cases"]) == ["p4", "p8", "p2", "p4_32"]
    for tag in g["blur_cases"]:
        x, p, sigmas, want = blur_case(g, tag)
        assert float(sigmas[0]) == 0.0 and float(sigmas[-1]) == float(g["blur_sigma_max"])      # both ends of the path, exactly
        assert_close(dct_blur(x, p, sigmas), want, what=f"dct_blur {tag}", **TOL)
        assert_close(dct_blur(x, p, sigmas.view(-1, 1, 1, 1)), want, what=f"dct_blur {tag}, sigmas as the path passes them", **TOL)


def test_training_losses_with_blurring_match_reference_fixture():
    check_blur_losses("cpu", False)


def test_blurring_changes_xt_and_leaves_ut_bitwise():
    g = golden("transport_blur")
    x1 = torch.from_numpy(g["loss_x1"])
    x0, t = torch.from_numpy(seeded(tuple(x1.shape), 7)), torch.tensor([0.0, 0.2, 0.5, 0.9, 1.0])
    for pt in ("GVP", "Linear", "VP"):
        plain = create_transport(pt, "velocity", fused_head=False).path_sampler
        blurred = create_transport(pt, "velocity", path_args=blur_path_args(g), fused_head=False).path_sampler
        assert blurred.use_blurring and not plain.use_blurring
        _, xt_p, ut_p = plain.plan(t, x0, x1)
        _, xt_b, ut_b = blurred.plan(t, x0, x1)
        assert torch.equal(ut_p, ut_b), pt
        assert not torch.allclose(xt_p[:3], xt_b[:3], atol=1e-3), pt                             # sigma_t > 0: a visible blur
        assert_close(xt_b[4], xt_p[4], what=f"{pt}: no blur at the data end", **TOL)


def test_zero_sigmas_return_x():
    x = torch.from_numpy(seeded((3, 2, 8, 8), 11))
    for p in (2, 4, 8):
        assert_close(dct_blur(x, p, torch.zeros(3)), x.numpy(), what=f"p={p}", **TOL)
        assert_close(dct_blur(x, p, 0.0), x.numpy(), what=f"p={p}, one sigma for the batch", **TOL)


def test_bad_shapes_raise_value_error():
    for shape, p in (((2, 3, 8, 12), 4), ((2, 3, 12, 8), 4), ((2, 3, 6, 6), 4), ((2, 3, 2, 2), 4), ((3, 8, 8), 4)):
        with pytest.raises(ValueError):
            dct_blur(torch.zeros(shape), p, torch.zeros(shape[0]))
    with pytest.raises(ValueError):
        dct_blur(torch.zeros(3, 2, 8, 8), 4, torch.zeros(2))                                     # neither one sigma nor one per sample
    tr = create_transport("GVP", "velocity", path_args=dict(use_blurring=True))
    with pytest.raises(ValueError):
        tr.training_losses(toy_denoiser, torch.zeros(2, 3, 6, 6))


def test_train_flags_reach_the_path_sampler(monkeypatch):
    from dimsum_amd import train
    monkeypatch.delenv("DIMSUM_FUSED_HEAD", raising=False)
    ps = train.transport_from_args(train.build_parser().parse_args([])).path_sampler
    assert (ps.use_blurring, ps.blur_sigma_max, ps.blur_upscale) == (False, 3, 4)
    args = train.build_parser().parse_args(["--use-blurring", "--blur-sigma-max", "5", "--blur-upscale", "8"])
    assert args.fused_head is None
    tr = train.transport_from_args(args)
    ps = tr.path_sampler
    assert (ps.use_blurring, ps.blur_sigma_max, ps.blur_upscale) == (True, 5, 8) and not tr.fused_head and not ps.fused_head
    assert train.transport_from_args(train.build_parser().parse_args(["--fused-head"])).fused_head is True
    monkeypatch.setenv("DIMSUM_FUSED_HEAD", "1")
    assert train.transport_from_args(train.build_parser().parse_args([])).path_sampler.fused_head is True
    assert train.transport_from_args(train.build_parser().parse_args(["--no-fused-head"])).fused_head is False


def test_reference_path_args_are_not_swallowed():
    """the call the reference's driver makes: every option it passes is kept on the plan"""
    tr = create_transport("Linear", "velocity", path_args={"diffusion_form": "sigma", "use_blurring": True, "blur_sigma_max": 2, "blur_upscale": 2})
    ps = tr.path_sampler
    assert (ps.diffusion_form, ps.use_blurring, ps.blur_sigma_max, ps.blur_upscale) == ("sigma", True, 2, 2)


def test_plan_without_blurring_is_bitwise_what_it_was(monkeypatch):
    monkeypatch.delenv("DIMSUM_FUSED_HEAD", raising=False)
    x1, x0 = torch.from_numpy(seeded((5, 3, 8, 8), 21)), torch.from_numpy(seeded((5, 3, 8, 8), 22))
    t = torch.tensor([0.0, 0.13, 0.5, 0.77, 1.0])
    for pt in ("GVP", "Linear", "VP"):
        tr = create_transport(pt, "velocity")
        ps = tr.path_sampler
        assert not tr.fused_head and not ps.use_blurring
        te = t.view(-1, 1, 1, 1)
        (a, da), (s, ds) = ps.compute_alpha_t(te), ps.compute_sigma_t(te)
        t_out, xt, ut = ps.plan(t, x0, x1)
        assert t_out is t and torch.equal(xt, a * x1 + s * x0) and torch.equal(ut, da * x1 + ds * x0), pt
        assert torch.equal(ps.compute_mu_t(t, x0, x1), a * x1 + s * x0), pt


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _header_layout(pairs):
    """{c struct: (sizeof, {field: offset})} from a C program compiled against include/dimsum_hip.h; pairs: [(c struct, ctypes mirror)]"""
    import subprocess
    import tempfile
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


def test_symbols_are_exported_and_structs_match_the_header():
    from dimsum_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dimsum_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    pairs = [("dimsum_fm_plan_params_t", _lib.FmPlanParams), ("dimsum_fm_loss_params_t", _lib.FmLossParams)]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offs = layout[cname]
        assert size == ctypes.sizeof(mirror), cname
        assert offs == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}, cname
        assert mirror._fields_[0][0] == "struct_size" and mirror().struct_size == size, cname


def test_wrong_struct_size_is_refused_before_anything_is_read():
    """DIMSUM_ERR_NULL (1) for NULL; DIMSUM_ERR_ABI (7) for a stale or foreign struct_size; the right size gets past that check and fails on
    the struct's NULL pointers (no launch)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    for fn, ptype in ((lib.dimsum_fm_plan, _lib.FmPlanParams), (lib.dimsum_fm_loss_fwd, _lib.FmLossParams), (lib.dimsum_fm_loss_bwd, _lib.FmLossParams)):
        assert fn(None, None) == 1
        P = ptype()
        assert fn(P, None) == 1
        size = ctypes.sizeof(ptype)
        for bad in (0, size - 8, size + 8):
            P.struct_size = bad
            assert fn(P, None) == 7, bad


def test_native_wrappers_refuse_cpu_tensors():
    from dimsum_amd import native
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.fm_plan(x, x, torch.zeros(5, 2), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.fm_loss_fwd(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.fm_loss_bwd(torch.zeros(2), x, x)
