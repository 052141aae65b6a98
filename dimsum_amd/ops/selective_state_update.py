"""selective_state_update -- same API as mamba/mamba_ssm/ops/triton/selective_state_update.py:115-190 (Triton there), on the HIP kernel
of csrc/mixer_step.hip: one token of the selective scan on a carried state."""
import torch

from .. import native


def selective_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False):
    """state: (batch, dim, dstate), updated IN PLACE; x, dt: (batch, dim); A: (dim, dstate); B, C: (batch, dstate); D, dt_bias: (dim,);
    z: (batch, dim) -> out (batch, dim). fp32 arithmetic; state and B / C may be float32 next to 16-bit x. Operands may be strided views."""
    return native.selective_state_update(state, x, dt, A.float(), B, C, D, z, dt_bias, dt_softplus)


def selective_state_update_torch(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False):
    """One step of the discretised state-space recurrence written out in plain torch, in the precision of its inputs (float64 inputs give
    the float64 answer), per batch row b, channel d and state n:
        step[b, d] = dt (+ dt_bias), through softplus if asked (torch's threshold of 20)
        h[b, d, n] <- h[b, d, n] exp(step[b, d] A[d, n]) + step[b, d] x[b, d] B[b, n]
        y[b, d]     = sum_n h[b, d, n] C[b, n] (+ D[d] x[b, d]), times z sigmoid(z) if z is given
    `state` receives h. What the tests compare the kernel with; never a fallback: nothing in the package calls it."""
    step = dt if dt_bias is None else dt + dt_bias.unsqueeze(0)
    if dt_softplus:
        step = torch.where(step > 20, step, torch.log1p(torch.exp(step.clamp(max=20))))
    work = torch.promote_types(step.dtype, torch.promote_types(A.dtype, B.dtype))
    step, xw = step.to(work).unsqueeze(-1), x.to(work).unsqueeze(-1)                     # (batch, dim, 1)
    decay = (step * A.to(work).unsqueeze(0)).exp()                                      # (batch, dim, dstate)
    drive = (step * xw) * B.to(work).unsqueeze(1)
    h = state.to(work) * decay + drive
    assert h.shape == state.shape and C.shape == B.shape == (state.shape[0], state.shape[2])
    y = (h * C.to(work).unsqueeze(1)).sum(-1)
    if D is not None:
        y = y + D.to(work).unsqueeze(0) * xw.squeeze(-1)
    if z is not None:
        zw = z.to(work)
        y = y * zw * torch.sigmoid(zw)
    state.copy_(h)
    return y.to(x.dtype)
