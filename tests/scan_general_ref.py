"""The selective scan restated from its formula in plain torch, in whatever precision its operands have (float64 / complex128 in the tests):

    dt = softplus(delta + delta_bias)        h_t = exp(dt A) h_{t-1} + dt B_t u_t        y_t = sum_n C_t h_t,  complex A: 2 Re sum_n C_t h_t
    out = (y + D u) silu(z)

B / C: input-dependent (batch, groups, dstate, seqlen) -- with complex A (batch, groups, dstate, 2 seqlen) reals, (re, im) interleaved -- or
constant (dim, dstate) of A's dtype. Differentiable: torch.autograd gives the gradients the kernels are held to (for complex leaves
PyTorch's convention). Shared by test_scan_general_cpu.py (which pins it to fixtures of the reference's selective_scan_ref) and
test_scan_general_gpu.py."""
import torch
import torch.nn.functional as F


def scan_restated(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, chunk=2048):
    """-> (out_z or out, out before the gate, last state (batch, dim, dstate), chunk-end states (batch, dim, n_chunks, dstate))"""
    batch, dim, L = u.shape
    N = A.shape[1]
    cplx = A.is_complex()
    dt = delta if delta_bias is None else delta + delta_bias[None, :, None]
    if delta_softplus:
        dt = F.softplus(dt, threshold=20.0)

    def per_channel(M):      # -> (batch, dim, dstate, seqlen) or (1, dim, dstate, 1)
        if M.dim() == 2:
            return M[None, :, :, None]
        if cplx:
            M = torch.view_as_complex(M.reshape(*M.shape[:-1], L, 2).contiguous())
        return M.repeat_interleave(dim // M.shape[1], dim=1)

    Bf, Cf = per_channel(B), per_channel(C)
    a = torch.exp(dt[:, :, None, :] * A[None, :, :, None])                    # (batch, dim, dstate, seqlen)
    bu = (dt * u)[:, :, None, :] * Bf
    h = torch.zeros(batch, dim, N, dtype=a.dtype)
    ys, ends = [], []
    for t in range(L):
        h = a[..., t] * h + bu[..., t]
        y = (h * Cf[..., t if Cf.shape[-1] > 1 else 0]).sum(-1)
        ys.append(2 * y.real if cplx else y)
        if (t + 1) % chunk == 0 or t == L - 1:
            ends.append(h)
    out = torch.stack(ys, dim=-1)
    if D is not None:
        out = out + D[None, :, None] * u
    res = out if z is None else out * F.silu(z)
    return res, out, h, torch.stack(ends, dim=2)


def make_case(batch, dim, L, N, cplx, var_B, var_C, groups=1, has_D=True, has_z=True, has_bias=True, seed=0, dtype=torch.float32):
    """operands in the distributions of mamba/tests/ops/test_selective_scan.py:62-95, rounded to `dtype` (weights: float32), as float64 /
    complex128 leaves that require grad"""
    g = torch.Generator().manual_seed(seed)
    f8 = torch.float64
    rnd = lambda *s: torch.randn(*s, generator=g)
    io = lambda t: t.to(dtype).to(f8)
    A = -0.5 * torch.rand(dim, N, generator=g)
    if cplx:
        A = torch.complex(A, rnd(dim, N))
    wt = lambda: torch.complex(rnd(dim, N), rnd(dim, N)) if cplx else rnd(dim, N)
    k = 2 if cplx else 1
    c = dict(A=A.to(torch.complex128 if cplx else f8),
             B=io(rnd(batch, groups, N, L * k)) if var_B else wt().to(torch.complex128 if cplx else f8),
             C=io(rnd(batch, groups, N, L * k)) if var_C else wt().to(torch.complex128 if cplx else f8),
             D=rnd(dim).to(f8) if has_D else None, z=io(rnd(batch, dim, L)) if has_z else None,
             delta_bias=(0.5 * torch.rand(dim, generator=g)).to(f8) if has_bias else None,
             u=io(rnd(batch, dim, L)), delta=io(0.5 * torch.rand(batch, dim, L, generator=g)), dout=io(rnd(batch, dim, L)))
    for k_, v in c.items():
        if v is not None and k_ != "dout":
            v.requires_grad_()
    return c
