"""The preconditions of the exact-integer GEMM tests (tests/gemm_exact_inputs.py), asserted on the float64 references without a GPU: if one of
them failed, torch.equal against float64 in tests/test_gemm_exact_gpu.py would ask for more than fp32 accumulation can give (or less than
it seems to). For every parametrised case of the row-factor, tile-walk and gate + residual tests:
  * sum |a| |b| / lsb < 2^24 for every output element (the whole expression for gate + residual), and operands, scales and reference on the
    lsb grid: every partial sum, in any order, is an fp32 number;
  * every scale (and gate magnitude) is a power of two;
  * every operand element times the factor the kernel multiplies it by in fp16 is zero or a normal fp16 number;
and the inputs discriminate: neighbouring reduction rows and K tiles carry different factors, the ranges' maxima differ."""
import pytest

torch = pytest.importorskip("torch")

import gemm_exact_inputs as X


def _exact(c, mass):
    assert mass.max().item() / c.lsb < X.EXACT, (mass.max().item() / c.lsb, X.EXACT)
    assert X.on_lsb_grid(c.ref, c.lsb)
    assert (c.ref.abs() <= mass).all()


def _rowfac_preconditions(c, R):
    _exact(c, c.mass)
    assert X.is_pow2(c.a_inv) and X.is_pow2(c.b_inv) and X.is_pow2(c.fac)
    assert c.fac.max().item() == 1.0 and c.fac.min().item() >= X.F16_MIN_NORMAL
    live = c.a_times_fac[c.a_times_fac != 0]
    assert live.min().item() >= X.F16_MIN_NORMAL and live.max().item() < 65504.0
    assert torch.equal(c.a_times_fac.half().double(), c.a_times_fac)               # (and exactly an fp16 number)
    # a factor read from a neighbouring row or K tile is another factor
    r = torch.arange(R)
    assert (c.fac != c.fac[r ^ 1]).all()
    assert (c.fac[64:] != c.fac[:-64]).all()
    # the ranges' maxima differ (range 0 holds the tensor's)
    tops = c.fac.view(c.ranges, -1).amax(1)
    assert tops[0].item() == 1.0 and len(set(tops.tolist())) == c.ranges


@pytest.mark.parametrize("R,P,Q,splits", X.TN_CASES)
def test_tn_row_factor_inputs_are_exact(R, P, Q, splits):
    c = X.tn_case(R, P, Q, splits)
    assert c.a16.shape == (R, P) and c.ref.shape == (P, Q) and c.b_buf.shape[1] % 256 == 0
    assert not c.b_buf[:, Q:].any()
    assert R % (splits * 64) == 0 and R // splits >= 128                             # whole K tiles, two per range at least
    _rowfac_preconditions(c, R)


@pytest.mark.parametrize("P,R,Q,splits", X.NN_CASES)
def test_nn_row_factor_inputs_are_exact(P, R, Q, splits):
    c = X.nn_case(P, R, Q, splits)
    assert c.a16.shape == (P, R) and c.ref.shape == (P, Q)
    assert R % ((splits or 1) * 64) == 0 and R // (splits or 1) >= 128
    _rowfac_preconditions(c, R)


@pytest.mark.parametrize("P,R,Q,splits", X.NN_REFUSED)
def test_nn_refused_cases_have_no_valid_ranges(P, R, Q, splits):
    assert R % (splits * 64) != 0 or R // splits < 128


@pytest.mark.parametrize("dtype,tune,family", X.WALK_CASES)
def test_tile_walk_inputs_are_exact(dtype, tune, family):
    M, N, K = X.WALK_SHAPE
    c = X.nt_case(dtype, M, N, K)
    _exact(c, c.mass)
    tiles_m = M // (128 if family == 1 else 256)
    assert tiles_m == (10 if family == 1 else 5) and {tiles_m % g for g in (2, 3, 4)} != {0}          # a partial last group
    if dtype == "float16":
        assert X.is_pow2(c.sa) and X.is_pow2(c.sb)
        assert (c.sa[:-256] != c.sa[256:]).all()                                     # the same row of the next tile has another scale
    else:
        assert c.sa is None and torch.equal(c.a.double().to(torch.bfloat16).double(), c.a.double())


def test_persistent_walk_inputs():
    M, F, K = X.PERSIST_WALK_SHAPE
    c = X.persist_walk_case()
    assert (M // 256) * (F // 128) == 260 and K // 64 == 4
    assert X.is_pow2(c.x_inv) and X.is_pow2(c.w_inv)
    for t in (c.x16, c.w16):
        live = t.double().abs()[t != 0]
        assert live.min().item() >= X.F16_MIN_NORMAL and live.max().item() < 2.0 ** 15
    l1 = (c.w16.double().abs().sum(1) * c.w_inv.double()).max().item()
    assert c.bound[0].item() >= l1 and c.bound[1].item() == c.b12.abs().max().item()


@pytest.mark.parametrize("name,dtype,tune,family,M,N,K,rows_per_batch,with_gate", X.GATERES_CASES, ids=[c[0] for c in X.GATERES_CASES])
def test_gate_residual_inputs_are_exact(name, dtype, tune, family, M, N, K, rows_per_batch, with_gate):
    c = X.gateres_case(dtype, M, N, K, rows_per_batch, with_gate)
    _exact(c, X.gateres_mass(c))
    assert rows_per_batch % 256 == 0 and M % rows_per_batch == 0 and c.B == M // rows_per_batch
    if dtype == "float16":
        assert X.is_pow2(c.sa) and X.is_pow2(c.sb)
    lo = X.GATERES_RES_PAD[0]
    assert (c.res_buf[:, :lo] == X.SENTINEL).all() and (c.res_buf[:, lo + N:] == X.SENTINEL).all()
    if with_gate:
        gate = c.gate_buf[:, N:2 * N]
        assert X.is_pow2(gate.abs()) and (c.gate_buf[:, :N] == X.SENTINEL).all() and (c.gate_buf[:, 2 * N:] == X.SENTINEL).all()
        assert (gate[0::2][:c.B // 2] != gate[1::2]).all()                           # batch elements e and e ^ 1 differ in every column
        assert (gate[:, :-1] != gate[:, 1:]).all()                                   # and neighbouring columns differ
    else:
        assert c.gate_buf is None


def test_case_counts():
    """the cases the issue names: nothing dropped"""
    assert len(X.TN_CASES) == 8 and len(X.NN_CASES) == 4 and len(X.NN_REFUSED) == 2 and len(X.WALK_CASES) == 3 and len(X.GATERES_CASES) == 8
    assert {(R, s) for R, _, _, s in X.TN_CASES} == {(128, 1), (192, 1), (320, 1), (512, 1), (256, 2), (384, 2), (384, 3)}
    assert any(Q % 256 != 0 for _, _, Q, _ in X.TN_CASES)
    assert {c[3] for c in X.GATERES_CASES} == {0, 1, 2} and sum(not c[8] for c in X.GATERES_CASES) == 1
