"""What tests/test_scan_general_leaves_gpu.py relies on, pinned without a GPU, so that a wrong reference cannot hide a wrong kernel:
`selective_scan_varlen_torch` with two groups and with each optional operand absent against per-segment `scan_restated` on the cut pieces;
the float64 restatement at L = 1, 2, 3 against a recurrence written out by hand; and the two helpers of the 16-bit rule, `round_T`
(round to nearest, ties to even, into bf16 / fp16) and `ulp_T` (the spacing of that format at a value), which live here: they are exact on
hand-written values incl. ties and fp16 subnormals and agree with torch's own conversion."""
import pytest
import torch

from scan_general_ref import make_case, scan_restated
from test_varlen_cpu import BATCHES, ROWS, segments

# (explicit mantissa bits, exponent of the smallest normal)
FORMATS = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def ulp_T(v, T):
    """the spacing of format T at |v| (float64 in, float64 out): 2^(max(floor(log2 |v|), emin) - mantissa bits); below the smallest normal
    and at 0 the subnormal spacing"""
    bits, emin = FORMATS[T]
    v = torch.as_tensor(v, dtype=torch.float64)
    _, e = torch.frexp(v.abs())                                                 # |v| = m 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1
    e = torch.where(v == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v), e - bits)


def round_T(x, T):
    """x (float64 holding fp32 values, finite, inside T's range) rounded to the nearest value of T, ties to even, as float64: x is an exact
    multiple of a power of two far below the spacing, x / spacing is exact, and torch.round rounds halves to even"""
    x = torch.as_tensor(x, dtype=torch.float64)
    q = ulp_T(x, T)
    return torch.round(x / q) * q


# ---- the helpers -------------------------------------------------------------------------------------------------------------------------------------
P = lambda k: 2.0 ** k
ROUNDED = {
    torch.bfloat16: [(1.0, 1.0), (1 + P(-8), 1.0), (1 + 3 * P(-8), 1 + P(-6)), (1 + P(-8) + P(-20), 1 + P(-7)), (1 + P(-8) - P(-20), 1.0),
                     (-(1 + P(-8)), -1.0), (-(1 + 3 * P(-8)), -(1 + P(-6))), (2 - P(-8), 2.0), (2 - P(-8) - P(-22), 2 - P(-7)),
                     (0.0, 0.0), (3.0, 3.0), (255 + 0.5, 256.0), (P(-30) * (1 + P(-8)), P(-30))],
    torch.float16: [(1.0, 1.0), (1 + P(-11), 1.0), (1 + 3 * P(-11), 1 + P(-9)), (1 + P(-11) + P(-23), 1 + P(-10)), (-(1 + P(-11)), -1.0),
                    (2 - P(-11), 2.0), (2048.0 + 1.0, 2048.0), (2048.0 + 3.0, 2052.0), (0.0, 0.0),
                    # subnormals: spacing 2^-24 below 2^-14
                    (P(-24), P(-24)), (P(-25), 0.0), (3 * P(-25), P(-23)), (P(-25) + P(-40), P(-24)), (-P(-25), -0.0), (P(-15), P(-15)),
                    (P(-14) - P(-24), P(-14) - P(-24)), (P(-14) - P(-25), P(-14)), (5 * P(-25), P(-23)), (P(-14) + P(-25), P(-14)),
                    (P(-14) + 3 * P(-25), P(-14) + P(-23))],
}
SPACING = {
    torch.bfloat16: [(1.0, P(-7)), (1.5, P(-7)), (-3.0, P(-6)), (2 - P(-7), P(-7)), (2.0, P(-6)), (0.0, P(-133)), (P(-126), P(-133)), (P(-130), P(-133)),
                     (0.75, P(-8))],
    torch.float16: [(1.0, P(-10)), (1024.0, 1.0), (-1.75, P(-10)), (0.0, P(-24)), (P(-14), P(-24)), (P(-15), P(-24)), (P(-24), P(-24)), (P(-13), P(-23)),
                    (65504.0, 32.0)],
}


@pytest.mark.parametrize("T", list(FORMATS), ids=str)
def test_round_and_ulp_helpers_are_exact(T):
    for x, want in ROUNDED[T]:
        assert float(torch.tensor(x, dtype=torch.float32)) == x, x                  # the list holds fp32 values: what the kernels round
        got = float(round_T(x, T))
        assert got == want, (x, got, want)
        assert float(torch.tensor(x, dtype=torch.float32).to(T)) == want, x         # and torch's conversion rounds the same way
    for v, want in SPACING[T]:
        assert float(ulp_T(v, T)) == want, (v, float(ulp_T(v, T)), want)
    # the neighbours of a value of T are one spacing away (going up; going down too unless the value is a power of two)
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g), 1e-5 * torch.randn(4096, generator=g), 60.0 * torch.randn(4096, generator=g),
                   torch.tensor([x for x, _ in ROUNDED[T]])]).float()
    want = x.to(T).double()
    assert torch.equal(round_T(x.double(), T), want)
    assert bool(((want - x.double()).abs() <= 0.5 * ulp_T(want, T)).all())
    assert torch.equal(round_T(want + ulp_T(want, T) * torch.sign(want), T), want + ulp_T(want, T) * torch.sign(want))


# ---- the packed-row restatement with groups and without the optional operands --------------------------------------------------------------------
OPTIONS = [dict(groups=2), dict(has_z=False), dict(has_D=False), dict(has_bias=False), dict(softplus=False),
           dict(groups=2, has_z=False, has_D=False, has_bias=False, softplus=False)]


@pytest.mark.parametrize("names", [BATCHES[0], BATCHES[2]], ids=["+".join(BATCHES[0]), "+".join(BATCHES[2])])
@pytest.mark.parametrize("opt", OPTIONS, ids=["-".join(o) for o in OPTIONS])
def test_varlen_restatement_with_options_is_the_per_segment_restatement(opt, names):
    from dimsum_amd.ops import selective_scan_varlen_torch
    opt = dict(opt)
    softplus = opt.pop("softplus", True)
    seq = torch.stack([ROWS[n] for n in names])
    L = seq.shape[1]
    c = make_case(batch=2, dim=6, L=L, N=5, cplx=False, var_B=True, var_C=True, seed=4, dtype=torch.float64, **opt)
    keys = [k for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias") if c[k] is not None]
    y, last = selective_scan_varlen_torch(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"], softplus, return_last_state=True,
                                          seq_idx=seq)
    got = torch.autograd.grad(y, [c[k] for k in keys], c["dout"])
    want_y, want_last = torch.zeros_like(y), torch.zeros_like(last)
    for r in range(2):
        for s, e in segments(seq[r]):
            piece = lambda t: None if t is None else t[r:r + 1, ..., s:e]
            res, _, h, _ = scan_restated(piece(c["u"]), piece(c["delta"]), c["A"], piece(c["B"]), piece(c["C"]), c["D"], piece(c["z"]), c["delta_bias"],
                                         softplus)
            want_y[r, :, s:e] = res[0]
            want_last[r] = h[0]                                 # the last one written is the row's last segment
    want = torch.autograd.grad(want_y, [c[k] for k in keys], c["dout"])
    torch.testing.assert_close(y, want_y, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(last, want_last, rtol=1e-12, atol=1e-12)
    for k, a, b in zip(keys, got, want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12, msg=lambda s, k=k: f"d{k}: {s}")
    if "groups" in opt:
        assert c["B"].shape[1] == 2 and got[keys.index("B")].shape == c["B"].shape and bool((got[keys.index("B")][:, 1] != 0).all())


# ---- the restatement shorter than a tile, against the recurrence written out ----------------------------------------------------------------------
@pytest.mark.parametrize("var_B,var_C", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_restatement_at_one_two_three_steps_is_the_unrolled_recurrence(L, cplx, var_B, var_C):
    c = make_case(batch=2, dim=3, L=L, N=4, cplx=cplx, var_B=var_B, var_C=var_C, seed=L, dtype=torch.float64)
    with torch.no_grad():
        res, out, last, ends = scan_restated(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"], True)
        u, A, D, z = c["u"], c["A"], c["D"], c["z"]
        dt = torch.log1p(torch.exp(c["delta"] + c["delta_bias"][None, :, None]))             # softplus, far below its threshold

        def at(M, t):                                           # B_t or C_t as (batch, dim, dstate)
            if M.dim() == 2:
                return M[None]
            return torch.complex(M[:, 0, :, 2 * t], M[:, 0, :, 2 * t + 1])[:, None] if cplx else M[:, 0, :, t][:, None]

        a = lambda t: torch.exp(dt[:, :, t, None] * A[None])
        x = lambda t: (dt[:, :, t] * u[:, :, t])[:, :, None] * at(c["B"], t)
        h = [x(0)]
        if L >= 2:
            h.append(a(1) * x(0) + x(1))
        if L >= 3:
            h.append(a(2) * a(1) * x(0) + a(2) * x(1) + x(2))
        for t in range(L):
            y = (at(c["C"], t) * h[t]).sum(-1)
            y = 2 * y.real if cplx else y
            want = (y + D[None] * u[:, :, t]) * z[:, :, t] / (1 + torch.exp(-z[:, :, t]))
            torch.testing.assert_close(res[:, :, t], want, rtol=1e-13, atol=1e-13)
            torch.testing.assert_close(out[:, :, t], y + D[None] * u[:, :, t], rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(last, h[-1].expand_as(last), rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(ends[:, :, 0], last, rtol=0, atol=0)
