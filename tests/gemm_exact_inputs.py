"""Exact-integer inputs of the GEMM tests (tests/test_gemm_exact_cpu.py asserts the preconditions, tests/test_gemm_exact_gpu.py launches the
kernels). Nothing here touches a GPU: every tensor is built on the CPU, the references are float64 products of the decoded operands.

The technique: operand elements are small integers times ONE fixed power of two, every scale, row factor and gate a power of two, every bias
and residual a small integer. Every product and every partial sum of a result is then a multiple of one power of two (`lsb`) and, as long as

    sum_r |a| |b| / lsb < 2^24      (for the gate + residual cases: |res| + |gate| (sum |a| |b| + |bias|), the whole expression)

holds for every output element, exactly representable in fp32 in ANY order of summation: the kernel's result must EQUAL the float64 reference.
The other two preconditions: every scale is a power of two (frexp mantissa 0.5, what rows_f16s produces), and every operand element times
the factor the kernel multiplies it by in fp16 stays in fp16's normal range (>= 2^-14 in magnitude, or exactly zero) -- the spread of the
per-row inverse scales is at most 2^-8 and the integers are scaled UP by a fixed power of two.

Every reduction row of the row-factor cases has its own scale, a function of its residue mod 64 and of its K tile (row_exponents): rows r and
r ^ 1 differ, rows r and r +- 64 differ, and with several reduction ranges range s sits s binades below range 0, so that the ranges' maxima
differ (the in-kernel route normalises a range by its own maximum, the table route by the tensor's)."""
import functools
from types import SimpleNamespace

import torch

EXACT = 2.0 ** 24
F16_MIN_NORMAL = 2.0 ** -14
SENTINEL = -77777.0          # what the guard columns of the gate + residual buffers hold

# ---- part 1: the row-factor kernels ------------------------------------------------------------------------------------------------------
# TN: (R, P, Q, splits); K / 64 per range = 2, 3, 5, 8, then 2 and 3 with two ranges, 2 with three, and a Q that is no multiple of 256
TN_CASES = [(128, 256, 256, 1), (192, 256, 256, 1), (320, 512, 256, 1), (512, 256, 512, 1), (256, 256, 256, 2), (384, 256, 256, 2), (384, 256, 256, 3),
            (192, 256, 392, 1)]
# NN: (P, R, Q, splits); two ranges only where a range keeps two whole K tiles
NN_CASES = [(256, 128, 256, None), (256, 320, 256, None), (512, 256, 512, None), (512, 256, 512, 2)]
NN_REFUSED = [(256, 128, 256, 2), (256, 320, 256, 2)]


def _ints(seed, shape, top):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-top, top + 1, shape, generator=g).double()


def _pow2(e):
    return torch.exp2(torch.as_tensor(e, dtype=torch.float64))


def row_exponents(R, splits):
    """-> (ea, eb): the binades below the top of the two images' scales of reduction row r. ea + eb differs between r and r ^ 1 (steps of +3 / -2
    against +1 / -2 never cancel) and between r and r +- 64 (ea repeats, eb moves); every K tile holds a row with ea + eb = 0, so range s
    (one binade lower per range) has the maximum 2^-s"""
    r = torch.arange(R)
    res, tile = r % 64, r // 64
    rng = r // (R // (splits or 1))
    return (res * 3) % 5 + rng, (tile + res) % 3


def _pad_cols(t, to=256):
    """(R, Q) -> the (R, Q rounded up to whole `to`-column tiles) zero-padded buffer gemm_tn asks for when Q % 256 != 0: b = buffer[:, :Q]"""
    R, Q = t.shape
    buf = torch.zeros((R, (Q + to - 1) // to * to), dtype=t.dtype)
    buf[:, :Q] = t
    return buf


@functools.lru_cache(maxsize=None)
def tn_case(R, P, Q, splits):
    """C (P, Q) = sum_r a[r, p] a_inv[r] b[r, q] b_inv[r]: a16 (R, P) = integers x 2^4, b (R, Q) = integers x 2^-2 (b_buf: zero-padded to whole
    256-column tiles), a_inv = 2^(-3 - ea), b_inv = 2^(1 - eb). fac = a_inv b_inv / top: the table the kernel multiplies a's rows by"""
    ea, eb = row_exponents(R, splits)
    a16, b16 = (_ints(11 * R + P, (R, P), 7) * 2.0 ** 4).half(), (_ints(13 * R + Q, (R, Q), 7) * 2.0 ** -2).half()
    a_inv, b_inv = _pow2(-3 - ea).float(), _pow2(1 - eb).float()
    a_dec, b_dec = a16.double() * a_inv.double()[:, None], b16.double() * b_inv.double()[:, None]
    prod = a_inv.double() * b_inv.double()
    return SimpleNamespace(a16=a16, b_buf=_pad_cols(b16), Q=Q, a_inv=a_inv, b_inv=b_inv, ref=a_dec.t() @ b_dec, mass=a_dec.abs().t() @ b_dec.abs(),
                           lsb=2.0 ** 4 * 2.0 ** -2 * prod.min().item(), fac=prod / prod.max(), top=prod.max().item(),
                           a_times_fac=a16.double().abs() * (prod / prod.max())[:, None], ranges=splits or 1)


@functools.lru_cache(maxsize=None)
def nn_case(P, R, Q, splits):
    """C (P, Q) = a_inv[p] sum_r a[p, r] b[r, q] b_inv[r]: a16 (P, R) = integers x 2^3 with one scale per OUTPUT row, a_inv = 2^(-2 - p % 4);
    b16 (R, Q) = integers x 2^-1 with one scale per REDUCTION row, b_inv = 2^(2 - ea - eb); fac = b_inv / top multiplies a's columns"""
    ea, eb = row_exponents(R, splits)
    a16, b16 = (_ints(17 * R + P, (P, R), 7) * 2.0 ** 3).half(), (_ints(19 * R + Q, (R, Q), 7) * 2.0 ** -1).half()
    a_inv, b_inv = _pow2(-2 - torch.arange(P) % 4).float(), _pow2(2 - ea - eb).float()
    a_dec, b_dec = a16.double() * a_inv.double()[:, None], b16.double() * b_inv.double()[:, None]
    prod = b_inv.double()
    return SimpleNamespace(a16=a16, b_buf=b16, Q=Q, a_inv=a_inv, b_inv=b_inv, ref=a_dec @ b_dec, mass=a_dec.abs() @ b_dec.abs(),
                           lsb=2.0 ** 3 * 2.0 ** -1 * a_inv.double().min().item() * prod.min().item(), fac=prod / prod.max(), top=prod.max().item(),
                           a_times_fac=a16.double().abs() * (prod / prod.max())[None, :], ranges=splits or 1)


# ---- part 3: the tile walk -------------------------------------------------------------------------------------------------------------------
WALK_SHAPE = (5 * 256, 384, 192)                       # (M, N, K): 5 row tiles of 256 (10 of 128): the last group is partial at group_m 2, 3, 4
WALK_CASES = [("bfloat16", 513, 0), ("float16", 513, 0), ("float16", 512, 1)]        # (operand type, tune_variant, kernel family)
PERSIST_WALK_SHAPE = (65 * 256, 512, 256)              # (M, F, K): 65 x 4 = 260 tiles of the gated epilogue, 4 K tiles


def walk_groups(tiles_m):
    return (0, 1, 2, 3, tiles_m)


@functools.lru_cache(maxsize=None)
def nt_case(dtype, M, N, K):
    """C = (a sa) (b sb)^T: a (M, K) = integers x 2^2, b (N, K) = integers x 2^1; float16: sa = 2^(-2 - m % 5), sb = 2^(-1 - n % 3) (a row's scale
    differs from that of the same row of the next tile: 256 % 5 = 1), bfloat16: no scales"""
    dt = getattr(torch, dtype)
    a, b = (_ints(23 * M + K, (M, K), 7) * 4.0).to(dt), (_ints(29 * N + K, (N, K), 7) * 2.0).to(dt)
    f16 = dtype == "float16"
    sa = _pow2(-2 - torch.arange(M) % 5).float() if f16 else None
    sb = _pow2(-1 - torch.arange(N) % 3).float() if f16 else None
    a_dec = a.double() * (sa.double()[:, None] if f16 else 1.0)
    b_dec = b.double() * (sb.double()[:, None] if f16 else 1.0)
    lsb = 4.0 * 2.0 * (sa.min().item() * sb.min().item() if f16 else 1.0)
    return SimpleNamespace(a=a, b=b, sa=sa, sb=sb, ref=a_dec @ b_dec.t(), mass=a_dec.abs() @ b_dec.abs().t(), lsb=lsb)


@functools.lru_cache(maxsize=None)
def persist_walk_case():
    """the gated f16 epilogue over scaled-fp16 operands with gate_bound: x (M, K) = integers x 2^11 with x_inv = 2^(-14 - m % 3) (true values: integers
    / 8 .. / 32), w12 (2 F, K) = integers x 2^11 with w_inv = 2^(-17 - n % 2), bias = integers / 16; x1, x2 are O(1). The bound is the float64
    l1 norm of the true weight rows (the kernel's bound assumes |x16| <= 2^15, which integers <= 7 x 2^11 meet). Not exact (GeLU)."""
    M, F, K = PERSIST_WALK_SHAPE
    x16, w16 = (_ints(31, (M, K), 7) * 2.0 ** 11).half(), (_ints(37, (2 * F, K), 7) * 2.0 ** 11).half()
    x_inv, w_inv = _pow2(-14 - torch.arange(M) % 3).float(), _pow2(-17 - torch.arange(2 * F) % 2).float()
    b12 = (_ints(41, (2 * F,), 8) / 16.0).float()
    l1 = (w16.double().abs().sum(1) * w_inv.double()).max().item()
    bound = torch.tensor([l1 * (1.0 + 2.0 ** -10), b12.abs().max().item()], dtype=torch.float32)
    return SimpleNamespace(x16=x16, x_inv=x_inv, w16=w16, w_inv=w_inv, b12=b12, bound=bound)


# ---- part 4: gate + residual -----------------------------------------------------------------------------------------------------------------
# (name, operand type, tune_variant, kernel family, M, N, K, rows_per_batch, with_gate)
GATERES_CASES = [
    ("bf16-m256-1tile", "bfloat16", 513, 0, 1024, 392, 192, 256, True),
    ("bf16-m256-2tiles", "bfloat16", 513, 0, 1024, 392, 192, 512, True),
    ("f16-m256-1tile", "float16", 513, 0, 1024, 392, 192, 256, True),
    ("f16-m256-2tiles", "float16", 513, 0, 1024, 392, 192, 512, True),
    ("f16-m128-1tile", "float16", 512, 1, 1024, 392, 192, 256, True),
    ("f16-m128-2tiles", "float16", 512, 1, 1024, 392, 192, 512, True),
    ("f16-persistent", "float16", 514, 2, 65 * 256, 1024, 256, 5 * 256, True),
    ("bf16-m256-nogate", "bfloat16", 513, 0, 1024, 392, 192, 256, False),
]
GATERES_OUT_PAD, GATERES_RES_PAD = (8, 8), (4, 20)     # guard columns left and right of the output / the residual inside their buffers


@functools.lru_cache(maxsize=None)
def gateres_case(dtype, M, N, K, rows_per_batch, with_gate):
    """out = res + gate[row // rows_per_batch] (sa sb a b^T + bias): a, b integers (float16: x 2^2 / x 2^1 with sa = 2^(-2 - m % 3), sb = 2^(-1 - n % 2)),
    bias integers <= 8, residual integers <= 64, gate[e, n] = +-2^(-(3 e + n) % 4) (negative where n % 3 == 0): differs per batch element and per
    column. The residual is a column range of res_buf, the gate the middle chunk of a (B, 3 N) tensor; the guard columns hold SENTINEL"""
    dt = getattr(torch, dtype)
    f16 = dtype == "float16"
    a, b = (_ints(43 * M + K, (M, K), 7) * (4.0 if f16 else 1.0)).to(dt), (_ints(47 * N + K, (N, K), 7) * (2.0 if f16 else 1.0)).to(dt)
    sa = _pow2(-2 - torch.arange(M) % 3).float() if f16 else None
    sb = _pow2(-1 - torch.arange(N) % 2).float() if f16 else None
    bias, res = _ints(53, (N,), 8).float(), _ints(59, (M, N), 64).float()
    B = M // rows_per_batch
    gate_buf = None
    rows = torch.ones((M, N), dtype=torch.float64)
    if with_gate:
        e, n = torch.arange(B)[:, None], torch.arange(N)[None, :]
        gate = (_pow2(-((3 * e + n) % 4)) * torch.where(n % 3 == 0, -1.0, 1.0)).float()
        gate_buf = torch.full((B, 3 * N), SENTINEL, dtype=torch.float32)
        gate_buf[:, N:2 * N] = gate
        rows = gate.double().repeat_interleave(rows_per_batch, 0)
    res_buf = torch.full((M, GATERES_RES_PAD[0] + N + GATERES_RES_PAD[1]), SENTINEL, dtype=torch.float32)
    res_buf[:, GATERES_RES_PAD[0]:GATERES_RES_PAD[0] + N] = res
    a_dec = a.double() * (sa.double()[:, None] if f16 else 1.0)
    b_dec = b.double() * (sb.double()[:, None] if f16 else 1.0)
    ref = res.double() + rows * (a_dec @ b_dec.t() + bias.double())
    lsb = (2.0 ** -3 if f16 else 1.0) * (2.0 ** -3 if with_gate else 1.0)        # (sa sb a b: 4 x 2 x 2^-4 x 2^-2 = 2^-3; the gate: 2^-3)
    return SimpleNamespace(a=a, b=b, sa=sa, sb=sb, bias=bias, res_buf=res_buf, gate_buf=gate_buf, gate_rows=rows, a_dec=a_dec, b_dec=b_dec, ref=ref, lsb=lsb, N=N, B=B)


def gateres_mass(c):
    """|res| + |gate| (sum |a| |b| + |bias|): what bounds every partial result of the expression"""
    lo = GATERES_RES_PAD[0]
    return c.res_buf[:, lo:lo + c.N].double().abs() + c.gate_rows.abs() * (c.a_dec.abs() @ c.b_dec.abs().t() + c.bias.double().abs())


def is_pow2(t):
    """every element a (positive) power of two: frexp mantissa 0.5"""
    return bool((torch.frexp(t.double())[0] == 0.5).all())


def on_lsb_grid(t, lsb):
    """every element a whole multiple of lsb"""
    q = t.double() / lsb
    return bool((q == q.round()).all())
