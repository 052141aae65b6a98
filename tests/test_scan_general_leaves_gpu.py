"""The general selective scan (csrc/ssm_scan_general.hip) on the kernel builds and launch shapes the other GPU files do not reach: one source
compiles into 114 kernels (DESIGN.md section 3.14 has the census) and a spill or a wrong lane map in one of them touches no other.

References and bounds, none of them taken from the kernels under test:
  * float64 / complex128 on the same rounded inputs: scan_general_ref.scan_restated, and selective_scan_varlen_torch for packed rows (both
    pinned by test_scan_general_cpu.py, test_varlen_cpu.py and test_scan_general_leaves_cpu.py), under test_scan_gpu.py's tol(L) /
    _bwd_tol(L) / _bwd_tol(L, True) for fp32 I/O and test_scan_general_gpu.py::test_half_dtypes' per-dtype pairs for 16-bit I/O
    (bf16 3e-2 / 5e-2, fp16 3e-3 / 5e-3, atol x 5 for the sums over batch and time);
  * the 16-bit rule: the 16-bit builds compute out (with z: out_z), du and ddelta in the fp32 build's own arithmetic and round once, so
    against the fp32-I/O build on the same operands upcast (which the fp32 tests pin to float64)
        |got - round_T(fp32 result)| <= 1 ulp of T at that value
    (round_T / ulp_T: test_scan_general_leaves_cpu.py). dz reads the rounded `out` in 16 bits and keeps to the float64 rule alone. Whether
    the two were bit-identical is printed;
  * packed rows: test_varlen_gpu.py's rule (`held`): packed error <= 2 x the error of the per-segment runs of the non-packed general kernel
    + one fp32 ulp, for everything written in a fixed order; the atomically summed gradients against float64.
Base shape: batch 2, dim 72 (lanes 8..63 of the second channel block masked), L = 37 (a partial last tile); N = 12 is one partly filled
wave, N = 72 five waves with a half-empty last one on the 1024-work-item builds."""
import pytest
import torch

from conftest import assert_close
from scan_general_ref import make_case
from test_scan_general_gpu import COMBOS, _case, _check_all, _gpu_leaves, _np, _run_fn
from test_scan_general_leaves_cpu import round_T, ulp_T
from test_scan_gpu import _bwd_tol, tol
from test_varlen_cpu import BATCHES, ROWS, segments
from test_varlen_gpu import ORDER, all_segments, cut, held

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = 37
HALF = {torch.bfloat16: (3e-2, 5e-2), torch.float16: (3e-3, 5e-3)}       # test_half_dtypes' (rtol, atol)
HALF_IDS = ["bf16", "fp16"]


def half_tols(dtype):
    rtol, atol = HALF[dtype]
    f = dict(rtol=rtol, atol=atol)
    return f, f, dict(rtol=rtol, atol=5 * atol)


def fp32_tols(Ln):
    return tol(Ln), _bwd_tol(Ln), _bwd_tol(Ln, True)


def sharp(name, got, fp32, T, report):
    """the 16-bit rule of the module docstring for one tensor -> ok"""
    want = round_T(fp32.detach().double().cpu(), T)
    err = (got.detach().double().cpu() - want).abs() / ulp_T(want, T)
    bit = torch.equal(got.detach(), fp32.detach().to(T))
    report.append(f"{name}: max |got - round_T(fp32 build)| = {err.max().item():.2f} ulp (bound 1), bit-identical {bit}")
    return bool((err <= 1.0).all())


# ---- a. 16-bit I/O on every build -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [12, 72])
@pytest.mark.parametrize("cplx,vB,vC", COMBOS)
@pytest.mark.parametrize("dtype", list(HALF), ids=HALF_IDS)
def test_half_io_on_every_build(dtype, cplx, vB, vC, N):
    """{bf16, fp16} x the 8 (complex, varB, varC) cases x N in {12, 72}: forward, last_state and every gradient through selective_scan_fn
    against float64 at the per-dtype tolerances, then out_z, du and ddelta against the fp32-I/O build under the 16-bit rule"""
    c, ref = _case(("leaf16", dtype, cplx, vB, vC, N), batch=2, dim=72, L=L, N=N, cplx=cplx, var_B=vB, var_C=vC, seed=N + 1, dtype=dtype)
    g = _gpu_leaves(c, dtype)
    res, last = _run_fn(g)
    assert res.dtype == dtype
    _check_all(c, ref, g, res, last, L, *half_tols(dtype))
    g32 = _gpu_leaves(c)                                                   # the same rounded operands, upcast
    res32, _ = _run_fn(g32)
    report = []
    oks = [sharp("out_z", res, res32, dtype, report), sharp("du", g["u"].grad, g32["u"].grad, dtype, report),
           sharp("ddelta", g["delta"].grad, g32["delta"].grad, dtype, report)]
    print("\n".join(report))
    assert all(oks), "\n".join(report)


# ---- packed rows: one case, its float64 answer, the launches, the checks -------------------------------------------------------------------------
_PACKED = {}


def packed_case(key, seq, dim, N, seed, dtype=torch.float32, softplus=True, **opt):
    """make_case's operands for a batch of packed rows (real A, input-dependent B / C; opt: groups, has_z, has_D, has_bias) and what float64
    gives on them: -> (c, dict(y, last, grads)), computed once per key"""
    if key not in _PACKED:
        from dimsum_amd.ops import selective_scan_varlen_torch
        c = make_case(batch=seq.shape[0], dim=dim, L=seq.shape[1], N=N, cplx=False, var_B=True, var_C=True, seed=seed, dtype=dtype, **opt)
        keys = [k for k in ORDER if c[k] is not None]
        y, last = selective_scan_varlen_torch(*(c[k] for k in ORDER), softplus, return_last_state=True, seq_idx=seq)
        grads = dict(zip(keys, torch.autograd.grad(y, [c[k] for k in keys], c["dout"])))
        _PACKED[key] = (c, dict(y=y.detach(), last=last.detach(), grads=grads))
    return _PACKED[key]


def run_packed(g, sq, softplus=True):
    """the packed launch pair through selective_scan_fn with autograd -> (y, last_state, {operand: gradient})"""
    from dimsum_amd.ops import selective_scan_fn
    y, last = selective_scan_fn(*(g[k] for k in ORDER), delta_softplus=softplus, return_last_state=True, seq_idx=sq)
    keys = [k for k in ORDER if g[k] is not None]
    grads = dict(zip(keys, torch.autograd.grad(y, [g[k] for k in keys], g["dout"])))
    torch.cuda.synchronize()
    return y.detach(), last.detach(), grads


def run_alone(g, segs, softplus=True):
    """every segment as a row of its own through the non-packed general kernels -> per-segment lists of what is written in a fixed order"""
    from dimsum_amd import native
    alone = {k: [] for k in ("out", "last", "u", "delta", "z")}
    with torch.no_grad():
        for r, s, e in segs:
            a = [None if g[k] is None else (g[k].detach()[r:r + 1, ..., s:e] if g[k].dim() >= 3 else g[k].detach()) for k in ORDER]
            out, x, *rest = native.selective_scan_general_fwd(*a, softplus)
            du, ddelta, _, _, _, _, _, *dz = native.selective_scan_general_bwd(*a, g["dout"][r:r + 1, :, s:e], out, None, softplus)
            for k, v in (("out", rest[0] if rest else out), ("last", x[:, :, -1, 1::2]), ("u", du), ("delta", ddelta), ("z", dz[0] if dz else None)):
                alone[k].append(v)
    torch.cuda.synchronize()
    return alone


def check_packed(tag, c, want, g, got, seq, softplus, tols, report):
    """the 2x rule against the per-segment runs for out, du, ddelta, dz and last_state; everything against float64 under `tols` = (forward,
    gradient, sums over batch and time) -> ok of the 2x rule (the float64 rule asserts)"""
    y, last, grads = got
    Bt = seq.shape[0]
    segs = all_segments(seq)
    alone = run_alone(g, segs, softplus)
    oks = [held(f"{tag} out", cut(y, segs), alone["out"], cut(want["y"], segs), report)[0]]
    for k in ("u", "delta", "z"):
        if c[k] is not None:
            oks.append(held(f"{tag} d{k}", cut(grads[k], segs), alone[k], cut(want["grads"][k], segs), report)[0])
    last_segs = [(r, *segments(seq[r])[-1]) for r in range(Bt)]
    oks.append(held(f"{tag} last_state", [last[r:r + 1] for r in range(Bt)], [alone["last"][segs.index(t)] for t in last_segs],
                    [want["last"][r:r + 1] for r in range(Bt)], report)[0])
    fwd_tol, grad_tol, wgrad_tol = tols
    assert y.dtype == g["u"].dtype and last.dtype == torch.float32
    assert_close(_np(y), _np(want["y"]), what=f"{tag} out", **fwd_tol)
    assert_close(_np(last), _np(want["last"]), what=f"{tag} last_state", **fwd_tol)
    for k, v in grads.items():
        assert v.dtype == g[k].dtype and v.shape == g[k].shape, k
        assert_close(_np(v), _np(want["grads"][k]), what=f"{tag} d{k}", **(wgrad_tol if k in ("A", "D", "delta_bias") else grad_tol))
    return all(oks)


def rows_of(names):
    return torch.stack([ROWS[n] for n in names])


BATCH_IDS = ["+".join(b) for b in BATCHES]


# ---- b. the packed-row backward at five waves and in 16 bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", BATCHES, ids=BATCH_IDS)
def test_packed_rows_five_waves(names):
    """fp32, dim 72, N = 72: the 1024-work-item packed forward and backward with a half-empty last wave, every segmentation of ROWS"""
    seq = rows_of(names)
    c, want = packed_case(("w5", names), seq, 72, 72, seed=BATCHES.index(names))
    g = _gpu_leaves(c)
    report = []
    ok = check_packed("scan N72 dim72", c, want, g, run_packed(g, seq.to(DEV)), seq, True, fp32_tols(L), report)
    print("\n".join(report))
    assert ok, "\n".join(report)


@pytest.mark.parametrize("N", [16, 72])
@pytest.mark.parametrize("dtype", list(HALF), ids=HALF_IDS)
def test_packed_rows_half_io(dtype, N):
    """bf16 / fp16 packed rows on both launch-bound classes: forward and every gradient against float64 at the per-dtype tolerances and
    against the per-segment 16-bit runs (2x rule), then out_z, du and ddelta against the fp32 packed run under the 16-bit rule"""
    seq = rows_of(BATCHES[0])
    c, want = packed_case(("half", dtype, N), seq, 72, N, seed=N, dtype=dtype)
    g = _gpu_leaves(c, dtype)
    got = run_packed(g, seq.to(DEV))
    report = []
    ok = check_packed(f"scan N{N} {dtype}", c, want, g, got, seq, True, half_tols(dtype), report)
    g32 = _gpu_leaves(c)
    y32, _, grads32 = run_packed(g32, seq.to(DEV))
    oks = [ok, sharp("out_z", got[0], y32, dtype, report), sharp("du", got[2]["u"], grads32["u"], dtype, report),
           sharp("ddelta", got[2]["delta"], grads32["delta"], dtype, report)]
    print("\n".join(report))
    assert all(oks), "\n".join(report)


# ---- c. packed rows with the options off -----------------------------------------------------------------------------------------------------------
OPTIONS = [dict(groups=2), dict(has_z=False), dict(has_D=False), dict(has_bias=False), dict(softplus=False),
           dict(groups=2, has_z=False, has_D=False, has_bias=False, softplus=False)]


@pytest.mark.parametrize("names", [BATCHES[0], BATCHES[2]], ids=[BATCH_IDS[0], BATCH_IDS[2]])
@pytest.mark.parametrize("N", [16, 72])
@pytest.mark.parametrize("opt", OPTIONS, ids=["-".join(o) for o in OPTIONS])
def test_packed_rows_options_off(opt, N, names):
    """fp32 packed rows with two groups (dim 144: two channel blocks per group, the second masked, q.d != blockIdx.x * 64 + lane) and with
    z / D / delta_bias / softplus absent, each alone (dim 72) and all together (dim 144, two groups)"""
    opt = dict(opt)
    softplus = opt.pop("softplus", True)
    dim = 144 if "groups" in opt else 72
    seq = rows_of(names)
    c, want = packed_case(("opt", tuple(sorted(opt.items())), softplus, N, names), seq, dim, N, seed=N + 3, softplus=softplus, **opt)
    g = _gpu_leaves(c)
    got = run_packed(g, seq.to(DEV), softplus)
    if "groups" in opt:
        assert got[2]["B"].shape == (2, 2, N, L) and got[2]["C"].shape == (2, 2, N, L)
    report = []
    ok = check_packed(f"scan N{N} dim{dim}", c, want, g, got, seq, softplus, fp32_tols(L), report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ---- d. row-strided ids ----------------------------------------------------------------------------------------------------------------------------
def _ids_shape_only(t, name, batch, seqlen, who):
    """native._check_token_ids without the contiguity it insists on: what the C ABI itself asks of a row operand (gen_row_stride_bad)"""
    assert torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (batch, seqlen) and t.stride(1) == 1 and t.stride(0) >= seqlen, name


def strided_rows(rows, pad):
    """rows (batch, L) as buf[:, 3:3 + L] of an int32 buffer (batch, L + 8) on the GPU whose other columns hold `pad` (batch, 8)"""
    Bt, Ln = rows.shape
    buf = torch.cat([pad[:, :3], rows, pad[:, 3:]], dim=1).to(torch.int32).to(DEV)
    view = buf[:, 3:3 + Ln]
    assert view.stride() == (Ln + 8, 1) and not view.is_contiguous() and torch.equal(view.cpu(), rows)
    return buf, view


@pytest.mark.parametrize("N", [16, 72])
def test_row_strided_ids_through_the_c_abi(N, monkeypatch):
    """seq_idx (and end_slots) as a view into a wider buffer. Every Python wrapper insists on contiguous ids (native._check_token_ids, pinned
    here), so the batch stride the kernels take and gen_row_stride_bad admits is host-reachable only through the C ABI: with that one Python
    check relaxed inside this test, native's own struct fill hands the view's pointer and stride to dimsum_ssm_scan_varlen_fwd / _bwd /
    _varlen_states_fwd. Everything must be bit-identical to the contiguous call and the buffer's padding untouched. The seq_idx padding
    holds ids that differ from every neighbour (read, they would create boundaries; read in place of a boundary's id they would move it);
    the end_slots padding names a spare slot that nobody else names, so a read of it shows up in the pool (and stays inside it)."""
    from dimsum_amd import native
    from dimsum_amd.ops import selective_scan_fn
    seq = rows_of(BATCHES[0])
    c, _ = packed_case(("w5", BATCHES[0]) if N == 72 else ("strided", N), seq, 72, N, seed=0)
    g = _gpu_leaves(c)
    y0, last0, grads0 = run_packed(g, seq.to(DEV))
    pad = 1000 + torch.arange(16, dtype=torch.int32).view(2, 8)
    buf, view = strided_rows(seq, pad)
    first = buf.clone()
    # the per-segment states: every segment's end stores into a slot of its own
    ends_at = [(r, e - 1) for r in range(2) for _, e in segments(seq[r])]
    num_slots = len(ends_at) + 2
    spare = num_slots - 1
    ends = torch.full((2, L), -1, dtype=torch.int32)
    for k, (r, t) in enumerate(ends_at):
        ends[r, t] = k
    ebuf, eview = strided_rows(ends, torch.full((2, 8), spare, dtype=torch.int32))
    efirst = ebuf.clone()
    ops = [g[k].detach() for k in ORDER]
    for call in (lambda: selective_scan_fn(*ops, delta_softplus=True, seq_idx=view),
                 lambda: native.selective_scan_varlen_fwd(*ops, True, view),
                 lambda: native.selective_scan_varlen_bwd(*ops, g["dout"], y0, None, True, view),
                 lambda: native.selective_scan_varlen_states_fwd(*ops, True, view, ends.to(DEV), torch.zeros(num_slots, 72, N, device=DEV)),
                 lambda: native.selective_scan_varlen_states_fwd(*ops, True, seq.to(DEV), eview, torch.zeros(num_slots, 72, N, device=DEV))):
        with pytest.raises(RuntimeError, match="must be a contiguous int32"):
            call()
    monkeypatch.setattr(native, "_check_token_ids", _ids_shape_only)
    y1, last1, grads1 = run_packed(g, view)
    assert torch.equal(y1, y0) and torch.equal(last1, last0)
    for k in ("u", "delta", "z"):
        assert torch.equal(grads1[k], grads0[k]), k
    for k in ("B", "C"):
        assert_close(_np(grads1[k]), _np(grads0[k]), what="d" + k, **_bwd_tol(L))
    for k in ("A", "D", "delta_bias"):
        assert_close(_np(grads1[k]), _np(grads0[k]), what="d" + k, **_bwd_tol(L, True))
    pools = []
    for sq, en in ((seq.to(DEV), ends.to(DEV)), (view, eview)):
        pool = torch.full((num_slots, 72, N), 7.0, device=DEV)
        out, x, out_z = native.selective_scan_varlen_states_fwd(*ops, True, sq, en, pool)
        torch.cuda.synchronize()
        pools.append((pool, out, x, out_z))
    for a, b in zip(*pools):
        assert torch.equal(a, b)
    assert torch.equal(pools[1][3], y0) and bool((pools[1][0][spare] == 7.0).all()) and bool((pools[1][0][spare - 1] == 7.0).all())
    assert not bool((pools[1][0][:len(ends_at)] == 7.0).any())
    assert torch.equal(pools[1][0][len(ends_at) - 1], last0[1])           # the last entry: the end of row 1
    assert torch.equal(buf, first) and torch.equal(ebuf, efirst)


# ---- e. groups with masked lanes, non-packed -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [12, 72])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_two_groups_with_masked_lanes(cplx, N):
    """(2, 144, 37) with n_groups = 2: 72 channels per group, two channel blocks per group with the second one masked, so the channel of a
    lane is not blockIdx.x * 64 + lane; dB / dC are (batch, 2, N, L) (complex: 2 L)"""
    c, ref = _case(("grp-masked", cplx, N), batch=2, dim=144, L=L, N=N, cplx=cplx, var_B=True, var_C=True, groups=2, seed=N + 2)
    g = _gpu_leaves(c)
    res, last = _run_fn(g)
    assert g["B"].grad.shape == (2, 2, N, L * (2 if cplx else 1))
    _check_all(c, ref, g, res, last, L, *fp32_tols(L))


# ---- f. shorter than a tile ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vB,vC", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("N", [3, 72])
@pytest.mark.parametrize("Ln", [1, 2, 3, 5])
def test_shorter_than_a_tile(Ln, N, cplx, vB, vC):
    """L in {1, 2, 3} (one tile, real: 4 steps, complex: 2) and 5: one checkpoint, a zero-filled B / C tile, fp32, forward, last_state and
    every gradient against float64"""
    c, ref = _case(("short", Ln, N, cplx, vB, vC), batch=2, dim=72, L=Ln, N=N, cplx=cplx, var_B=vB, var_C=vC, seed=10 * Ln + N)
    g = _gpu_leaves(c)
    res, last = _run_fn(g)
    _check_all(c, ref, g, res, last, Ln, *fp32_tols(Ln))


SHORT_ROWS = {"L3": torch.tensor([[0, 1, 1], [5, 5, 5]], dtype=torch.int32), "L1": torch.tensor([[0], [7]], dtype=torch.int32)}


@pytest.mark.parametrize("N", [3, 72])
@pytest.mark.parametrize("which", list(SHORT_ROWS))
def test_packed_rows_shorter_than_a_tile(which, N):
    """packed rows of 3 positions (ids [0, 1, 1] and [5, 5, 5]) and of one: the reset mask clamps every read to the row's last id"""
    seq = SHORT_ROWS[which]
    Ln = seq.shape[1]
    c, want = packed_case(("short", which, N), seq, 72, N, seed=N + Ln)
    g = _gpu_leaves(c)
    report = []
    ok = check_packed(f"scan N{N} {which}", c, want, g, run_packed(g, seq.to(DEV)), seq, True, fp32_tols(Ln), report)
    print("\n".join(report))
    assert ok, "\n".join(report)


# ---- the carried state at five waves ---------------------------------------------------------------------------------------------------------------
def carry_case(N, dim, n, cplx, vB, vC, dtype):
    """test_prefill_chunks_gpu.scan_case with B and C constant or input-dependent independently of each other"""
    from dimsum_amd.ops import selective_scan_carry_torch
    key = ("carry", N, dim, n, cplx, vB, vC, dtype)
    if key not in _PACKED:
        c = make_case(2, dim, n, N, cplx, vB, vC, seed=N + n, dtype=dtype)
        c = {k: v.detach() for k, v in c.items()}
        with torch.no_grad():
            want = selective_scan_carry_torch(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"], True)
        g = {k: v.detach() for k, v in _gpu_leaves(c, dtype).items()}
        g["float64"] = c
        _PACKED[key] = (g, want)
    return _PACKED[key]


@pytest.mark.parametrize("N", [12, 72])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_carried_state_on_every_forward_build(cplx, N):
    """dimsum_ssm_scan_carry_fwd launches the 48 forward builds with a state loaded before the walk and stored after it;
    test_prefill_chunks_gpu.py runs it up to 64 states, with B and C both input-dependent or (fp32) both constant. Here: every (varB, varC)
    case x every I/O type x N in {12, 72} at dim 72 (masked lanes; at 72 the 1024-work-item builds, a half-empty fifth wave), 5 steps, every
    split, under that file's check_split and its bounds; the state float32 (complex: complex64), and of the I/O dtype where B and C are
    input-dependent and A real (what its state_rounding_bound is written for)"""
    from test_prefill_chunks_gpu import check_split
    n, dim = 5, 72
    for (vB, vC), dtype in ((bc, t) for bc in ((True, True), (True, False), (False, True), (False, False)) for t in (torch.float32, torch.float16, torch.bfloat16)):
        g, want = carry_case(N, dim, n, cplx, vB, vC, dtype)
        states = (torch.complex64,) if cplx else (torch.float32, dtype) if vB and vC and dtype != torch.float32 else (torch.float32,)
        for state_dtype in states:
            for s in range(n):
                check_split(g, want, n, s, cplx, dtype, state_dtype, f"N{N} D{dim} L{n} s{s} {dtype} state {state_dtype} varB={vB} varC={vC}")


# ---- g. two launches ---------------------------------------------------------------------------------------------------------------------------------
def test_two_packed_launches():
    """packed rows at N = 72: what is written in a fixed order is bit-equal between two launches, the atomically added sums agree within
    the gradient tolerances (test_scan_general_gpu.py::test_two_launches, for the packed builds)"""
    seq = rows_of(BATCHES[0])
    c, _ = packed_case(("w5", BATCHES[0]), seq, 72, 72, seed=0)
    (y0, l0, g0), (y1, l1, g1) = (run_packed(_gpu_leaves(c), seq.to(DEV)) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(l0, l1)
    for k in ("u", "delta", "z"):
        assert torch.equal(g0[k], g1[k]), k
    for k in ("B", "C"):
        assert_close(_np(g1[k]), _np(g0[k]), what="d" + k, **_bwd_tol(L))
    for k in ("A", "D", "delta_bias"):
        assert_close(_np(g1[k]), _np(g0[k]), what="d" + k, **_bwd_tol(L, True))
