"""Exact-integer tests of the GEMM leaves the suite held to a tolerance or did not launch (csrc/gemm_nt.hip, csrc/gemm_nt_kernel.hpp). The inputs
come from tests/gemm_exact_inputs.py, whose preconditions tests/test_gemm_exact_cpu.py asserts: integers times powers of two, every partial
sum an fp32 number in any order of summation -- so the kernels' results must EQUAL the float64 references (torch.equal), and a factor taken
from the wrong row, a range normalised by another range's maximum, a gate row of the wrong batch element or a tile the walk visits twice
shows as a wrong element, not as a rounding difference.
  part 1: gemm_tn_rowfac_kernel (dimsum_gemm_tn with k_scale_ptr / k_inv_a_ptr) and gemm_nn_rowfac_kernel (dimsum_gemm_nn)
  part 2: launch<kOpBf16, kEpiGatedF16> and launch<kOpF16, kEpiGatedSplit3> (not exact: the GeLU; the sibling leaves' bars)
  part 3: tune_group_m does not change a bit of the result (256-row, 128-row and persistent kernels)
  part 4: kEpiF32GateRes on the three kernel families, bit for bit
No case is skipped at run time: every test records the cases it finished, and the last test of the file counts them."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gemm_exact_inputs as X

_RAN = {"tn": set(), "nn": set(), "leaves": set(), "walk": set(), "persist_walk": set(), "gateres": set()}
PERSIST_ID = "65 x 4 tiles"


def _dev(t):
    return None if t is None else t.cuda()


def _same(got, ref):
    """bit for bit the float64 reference; on failure: where and by how much"""
    g = got.double()
    if not torch.equal(g, ref):
        bad = (g != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{bad.shape[0]} of {ref.numel()} elements differ, first at {i}: got {g[i].item()!r}, want {ref[i].item()!r}")


# ---- part 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,P,Q,splits", X.TN_CASES)
def test_tn_row_factor_routes_are_exact(R, P, Q, splits, monkeypatch):
    """gemm_tn_rowfac_kernel<kOpF16, kEpiF32> (gemm_nt.hip, dimsum_gemm_tn): the factor table of row_factors (k_scale_ptr / c_scale_ptr: normalised
    by the tensor's maximum) and the factors formed inside the kernel (k_inv_a_ptr / k_inv_b_ptr: every range by its own maximum) both equal the
    float64 product of the decoded operands and each other, bit for bit; K / 64 = 2, 3, 5, 8 per range, 2 and 3 ranges, and a Q of 392 through
    the zero-padded rows gemm_tn asks for (the second column tile is partial). Repeated launches are identical."""
    from dimsum_amd import native
    monkeypatch.delenv("DIMSUM_ROW_FACTORS_KERNEL", raising=False)
    c = X.tn_case(R, P, Q, splits)
    a, b, ia, ib, ref = c.a16.cuda(), c.b_buf.cuda()[:, :Q], c.a_inv.cuda(), c.b_inv.cuda(), c.ref.cuda()
    assert native.gemm_tn_supported(a, b)
    fac, top = native.row_factors(ia, ib)
    assert torch.equal(fac.double().cpu(), c.fac) and top.item() == c.top
    table = native.gemm_tn(a, b, splits=splits, row_scales=(fac, top))
    inside = native.gemm_tn(a, b, splits=splits, row_invs=(ia, ib))
    assert table.shape == (P, Q) and table.dtype == torch.float32
    _same(table, ref)
    _same(inside, ref)
    assert torch.equal(table, inside)
    assert torch.equal(native.gemm_tn(a, b, splits=splits, row_scales=(fac, top)), table)
    assert torch.equal(native.gemm_tn(a, b, splits=splits, row_invs=(ia, ib)), inside)
    _RAN["tn"].add((R, P, Q, splits))


@pytest.mark.parametrize("P,R,Q,splits", X.NN_CASES)
def test_nn_row_factor_routes_are_exact(P, R, Q, splits, monkeypatch):
    """gemm_nn_rowfac_kernel<kOpF16, kEpiF32> (gemm_nt.hip, dimsum_gemm_nn) through native.gemm_nn: a's rows are output rows with their own scales,
    b's rows the reduction index whose scales become the factors a's columns are multiplied by -- formed inside the kernel (the default) and
    from the row_factors table (DIMSUM_ROW_FACTORS_KERNEL=1): both equal the float64 product of the decoded operands bit for bit"""
    from dimsum_amd import native
    c = X.nn_case(P, R, Q, splits)
    a, b, ia, ib, ref = c.a16.cuda(), c.b_buf.cuda(), c.a_inv.cuda(), c.b_inv.cuda(), c.ref.cuda()
    assert native.gemm_nn_supported(a, b)
    monkeypatch.delenv("DIMSUM_ROW_FACTORS_KERNEL", raising=False)
    inside = native.gemm_nn(a, ia, b, ib, splits=splits)
    again = native.gemm_nn(a, ia, b, ib, splits=splits)
    monkeypatch.setenv("DIMSUM_ROW_FACTORS_KERNEL", "1")
    table = native.gemm_nn(a, ia, b, ib, splits=splits)
    assert inside.shape == (P, Q) and inside.dtype == torch.float32
    _same(inside, ref)
    _same(table, ref)
    assert torch.equal(inside, again) and torch.equal(inside, table)
    _RAN["nn"].add((P, R, Q, splits))


@pytest.mark.parametrize("P,R,Q,splits", X.NN_REFUSED)
def test_nn_refuses_ranges_of_less_than_two_k_tiles(P, R, Q, splits):
    """dimsum_gemm_nn's ranges_ok: two ranges of R = 128 (one K tile each) or of R = 320 (two and a half) are refused before anything is launched"""
    from dimsum_amd import native
    c = X.nn_case(P, R, Q, None)
    with pytest.raises(RuntimeError):
        native.gemm_nn(c.a16.cuda(), c.a_inv.cuda(), c.b_buf.cuda(), c.b_inv.cuda(), splits=splits)


# ---- part 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,F,H,with_bias", [(256, 136, 192, True), (256, 136, 192, False), (512, 256, 128, True), (512, 256, 128, False)])
def test_gated_gelu_leaves_no_other_test_launches(M, F, H, with_bias):
    """launch<kOpF16, kEpiGatedSplit3> (gemm_nt.hip: gated_split3 over UNSCALED fp16 operands) and launch<kOpBf16, kEpiGatedF16> (gated_f16 over
    bf16 operands, constant out_scale), both on the 256-row tiles. The bars of their sibling leaves (test_gemm_gpu.py::test_gated_gelu_epilogues):
    the split image decodes to the float64 expression of the same 16-bit operands within 2e-5 of max |h|, both hi copies identical, no worse
    than 1.5 x the unfused pair (library GEMM + gated GeLU pass) + 1e-6; the fp16 output / out_scale within 1e-3 of max |h|"""
    from dimsum_amd import native
    g = torch.Generator(device="cuda").manual_seed(4 + M)
    x = torch.randn((M, H), device="cuda", generator=g)
    w12 = torch.randn((2 * F, H), device="cuda", generator=g) * H ** -0.5
    bias = torch.randn((2 * F,), device="cuda", generator=g) * 0.1 if with_bias else None

    def expression(xo, wo):
        x12 = xo.double() @ wo.double().t() + (0 if bias is None else bias.double())
        return torch.nn.functional.gelu(x12[:, :F], approximate="tanh") * x12[:, F:]

    x16, w16 = x.half(), w12.half()
    with native.gemm_kernel_log() as log:
        got = native.gemm_nt(x16, w16, bias=bias, epilogue="gated_split3")
    assert log == [("gated_split3", 0)], log
    assert got.shape == (M, 3 * F) and got.dtype == torch.bfloat16
    ref = expression(x16, w16)
    hi, hi2, lo = got[:, :F], got[:, F:2 * F], got[:, 2 * F:]
    assert torch.equal(hi, hi2)
    scale = ref.abs().max().item()
    err = ((hi.double() + lo.double()) - ref).abs().max().item() / scale
    unf = native.gated_gelu_fwd(torch.mm(x16, w16.t(), out_dtype=torch.float32), bias, split3=True)
    uerr = ((unf[:, :F].double() + unf[:, 2 * F:].double()) - ref).abs().max().item() / scale
    print(f"gated_split3 over fp16 ({M}, {F}, {H}, bias {with_bias}): fused {err:.2e}, unfused {uerr:.2e}")
    assert err < 2e-5 and err < 1.5 * uerr + 1e-6, (err, uerr)
    assert torch.equal(native.gemm_nt(x16, w16, bias=bias, epilogue="gated_split3"), got)

    xb, wb = x.bfloat16(), w12.bfloat16()
    with native.gemm_kernel_log() as log:
        g16 = native.gemm_nt(xb, wb, bias=bias, epilogue="gated_f16", out_scale=8.0)
    assert log == [("gated_f16", 0)], log
    assert g16.shape == (M, F) and g16.dtype == torch.float16
    refb = expression(xb, wb)
    errb = (g16.double() / 8.0 - refb).abs().max().item() / refb.abs().max().item()
    print(f"gated_f16 over bf16 ({M}, {F}, {H}, bias {with_bias}): {errb:.2e}")
    assert errb < 1e-3, errb
    assert torch.equal(native.gemm_nt(xb, wb, bias=bias, epilogue="gated_f16", out_scale=8.0), g16)
    _RAN["leaves"].add((M, F, H, with_bias))


# ---- part 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tune,family", X.WALK_CASES)
def test_tile_walk_does_not_change_a_bit(dtype, tune, family):
    """launch<kOpBf16, kEpiF32>, launch<kOpF16, kEpiF32> (tune 513) and launch_m128<kOpF16, kEpiF32> (tune 512) of gemm_nt.hip with tune_group_m =
    0 (automatic), 1, 2, 3 and tiles_m: which workgroup owns which tile changes, no element does -- every result equals the float64 product of
    the exact-integer operands. 5 row tiles of 256: the last group is partial at group_m 2, 3 (and 4, the automatic walk's for more than 16 row
    tiles); on the 128-row tiles the host layer walks whole tile columns up to 32 row tiles, whatever group_m asks for. tune_reserved stays 0
    (include/dimsum_hip.h documents it for tuning builds)."""
    from dimsum_amd import native
    M, N, K = X.WALK_SHAPE
    c = X.nt_case(dtype, M, N, K)
    a, b, ref = c.a.cuda(), c.b.cuda(), c.ref.cuda()
    kw = dict(scales=(c.sa.cuda(), c.sb.cuda())) if c.sa is not None else {}
    tiles_m = M // (128 if family == 1 else 256)
    first = None
    for group_m in X.walk_groups(tiles_m) + (4,):
        with native.gemm_kernel_log() as log:
            got = native.gemm_nt(a, b, tune=(tune, group_m, 0), **kw)
        assert log == [("f32", family)], log
        _same(got, ref)
        first = got if first is None else first
        assert torch.equal(got, first)
    _RAN["walk"].add((dtype, tune))


def test_tile_walk_of_the_persistent_stream(monkeypatch):
    """launch_persist<kOpF16, kEpiGatedF16> (gemm_nt.hip; tune None: the heuristics' own choice, and 514) against launch<kOpF16, kEpiGatedF16> (513)
    at tune_group_m = 0, 1, 2, 3, 65: 65 x 4 = 260 tiles on 256 workgroups (four of them walk a second tile), 4 K tiles. The GeLU is not exact, so the
    results are compared with each other, bit for bit (images and row scales), and once with float64 at
    test_persistent_stream_is_the_one_tile_per_workgroup_kernel_bit_for_bit's 2e-3 of the row maximum"""
    from dimsum_amd import native
    monkeypatch.delenv("DIMSUM_GEMM_PERSIST", raising=False)           # (tune None must be the heuristics' choice, not the A / B switch's)
    M, F, K = X.PERSIST_WALK_SHAPE
    c = X.persist_walk_case()
    x, xi, w, wi, b12 = c.x16.cuda(), c.x_inv.cuda(), c.w16.cuda(), c.w_inv.cuda(), c.b12.cuda()
    kw = dict(bias=b12, epilogue="gated_f16", scales=(xi, wi), gate_bound=c.bound.cuda())

    def run(tune, family):
        with native.gemm_kernel_log() as log:
            h = native.gemm_nt(x, w, tune=tune, **kw)
        assert log == [("gated_f16", family)], log
        return h

    def same(h, g):
        return torch.equal(h.data.view(torch.int16), g.data.view(torch.int16)) and torch.equal(h.inv, g.inv)

    plain = run((513, 0, 0), 0)
    assert same(run(None, 2), plain)
    for group_m in X.walk_groups(M // 256):
        assert same(run((513, group_m, 0), 0), plain), group_m
        assert same(run((514, group_m, 0), 2), plain), group_m
    x12 = (x.double() * xi.double()[:, None]) @ (w.double() * wi.double()[:, None]).t() + b12.double()
    href = torch.nn.functional.gelu(x12[:, :F], approximate="tanh") * x12[:, F:]
    err = ((plain.float().double() - href).abs() / href.abs().amax(-1, keepdim=True)).max().item()
    print(f"persistent walk: gated f16 image vs float64 {err:.2e} of the row maximum")
    assert err < 2e-3, err
    _RAN["persist_walk"].add(PERSIST_ID)


# ---- part 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,tune,family,M,N,K,rows_per_batch,with_gate", X.GATERES_CASES, ids=[c[0] for c in X.GATERES_CASES])
def test_gate_residual_epilogue_is_exact(name, dtype, tune, family, M, N, K, rows_per_batch, with_gate):
    """kEpiF32GateRes of gemm_nt.hip: launch<kOpBf16, ..> / launch<kOpF16, ..> (tune 513), launch_m128<kOpF16, ..> (512) and launch_persist<kOpF16, ..>
    (514; 65 x 4 tiles, 4 K tiles). out = residual + gate[row // rows_per_batch] (a b^T + bias) equals float64 bit for bit: one and two row tiles
    per batch element (five on the persistent build), ragged N = 392, power-of-two gates that differ per batch element and per column, for fp16
    power-of-two row and column scales; residual and output are column ranges of wider buffers, the gate the middle chunk of a (B, 3 N) tensor,
    and the guard columns of the output keep their sentinel"""
    from dimsum_amd import native
    c = X.gateres_case(dtype, M, N, K, rows_per_batch, with_gate)
    a, b, ref = c.a.cuda(), c.b.cuda(), c.ref.cuda()
    lo, hi = X.GATERES_OUT_PAD
    out_buf = torch.full((M, lo + N + hi), X.SENTINEL, device="cuda", dtype=torch.float32)
    out = out_buf[:, lo:lo + N]
    res = c.res_buf.cuda()[:, X.GATERES_RES_PAD[0]:X.GATERES_RES_PAD[0] + N]
    gate = c.gate_buf.cuda()[:, N:2 * N] if with_gate else None
    kw = dict(bias=c.bias.cuda(), residual=res, gate=gate, rows_per_batch=rows_per_batch if with_gate else None)
    if c.sa is not None:
        kw["scales"] = (c.sa.cuda(), c.sb.cuda())
    with native.gemm_kernel_log() as log:
        got = native.gemm_nt(a, b, out=out, tune=(tune, 0, 0), **kw)
    assert log == [("f32", family)], log
    assert got.data_ptr() == out.data_ptr()
    _same(out, ref)
    assert (out_buf[:, :lo] == X.SENTINEL).all() and (out_buf[:, lo + N:] == X.SENTINEL).all()
    again = torch.full_like(out_buf, X.SENTINEL)
    native.gemm_nt(a, b, out=again[:, lo:lo + N], tune=(tune, 0, 0), **kw)
    assert torch.equal(again, out_buf)
    _RAN["gateres"].add(name)


def test_every_case_ran(request):
    """no case of this file is dropped or skipped at run time: when the whole file was selected, every parametrised case above has finished
    (a failed case is missing here too); the counts are the issue's"""
    assert len(X.TN_CASES) == 8 and len(X.NN_CASES) == 4 and len(X.WALK_CASES) == 3 and len(X.GATERES_CASES) == 8
    mine = [i for i in request.session.items if i.module is request.module]
    if len(mine) != 8 + 4 + 2 + 4 + 3 + 1 + 8 + 1:
        return          # (a selection of this file's tests was asked for)
    assert _RAN["tn"] == set(X.TN_CASES) and _RAN["nn"] == set(X.NN_CASES) and len(_RAN["leaves"]) == 4
    assert _RAN["walk"] == {(d, t) for d, t, _ in X.WALK_CASES} and _RAN["persist_walk"] == {PERSIST_ID}
    assert _RAN["gateres"] == {c[0] for c in X.GATERES_CASES}
