"""selective_state_update -- same API as mamba/mamba_ssm/ops/triton/selective_state_update.py:115-190 (Triton there), on the HIP kernel
of csrc/mixer_step.hip: one token of the selective scan on a carried state. Next to its plain-torch restatement, the restatement of the
scan entered with a carried state for any number of tokens (selective_scan_fn(initial_state=...), csrc/ssm_scan_general.hip)."""
import torch

from .. import native


def selective_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, state_indices=None):
    """state: (batch, dim, dstate), updated IN PLACE; x, dt: (batch, dim); A: (dim, dstate); B, C: (batch, dstate); D, dt_bias: (dim,);
    z: (batch, dim) -> out (batch, dim). fp32 arithmetic; state and B / C may be float32 next to 16-bit x. Operands may be strided views.
    state_indices (batch,) int32 (upstream Mamba's state_batch_indices): state is a pool (num_slots, dim, dstate), row b works on
    state[state_indices[b]], a negative entry is a padding row (no state touched, zero output). Entries must be < num_slots and no slot may
    be named twice: neither is checked (it would take a device read)."""
    if state_indices is None:
        return native.selective_state_update(state, x, dt, A.float(), B, C, D, z, dt_bias, dt_softplus)
    return native.selective_state_update(state, x, dt, A.float(), B, C, D, z, dt_bias, dt_softplus, state_indices=state_indices)


def selective_state_update_torch(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, state_indices=None):
    """One step of the discretised state-space recurrence written out in plain torch, in the precision of its inputs (float64 inputs give
    the float64 answer), per batch row b, channel d and state n:
        step[b, d] = dt (+ dt_bias), through softplus if asked (torch's threshold of 20)
        h[b, d, n] <- h[b, d, n] exp(step[b, d] A[d, n]) + step[b, d] x[b, d] B[b, n]
        y[b, d]     = sum_n h[b, d, n] C[b, n] (+ D[d] x[b, d]), times z sigmoid(z) if z is given
    `state` receives h. What the tests compare the kernel with; never a fallback: nothing in the package calls it.
    state_indices (batch,) int32: state is a pool and row b works on state[state_indices[b]]; rows with a negative entry are skipped -- no
    slot is read or written -- and give zeros."""
    if state_indices is not None:
        from .causal_conv1d_interface import _slot_rows
        live, slots = _slot_rows(state_indices, x.shape[0])
        out = torch.zeros_like(x)
        if live:
            rows = state[slots]                                                         # a gathered copy
            out[live] = selective_state_update_torch(rows, x[live], dt[live], A, B[live], C[live], D, None if z is None else z[live], dt_bias,
                                                     dt_softplus)
            state[slots] = rows
        return out
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


def selective_scan_carry_torch(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, initial_state=None):
    """The selective scan entered with a carried state, written out in plain torch, in the precision of its inputs (float64 / complex128
    inputs give that answer), per batch row b, channel d, state n and step t:
        dt[b, d, t]  = delta (+ delta_bias), through softplus if asked (torch's threshold of 20)
        h[b, d, n]  <- h[b, d, n] exp(dt A[d, n]) + dt u[b, d, t] B[.., n, t],   h before the first step = initial_state (zeros if None)
        y[b, d, t]   = sum_n h[b, d, n] C[.., n, t]   (complex A: twice its real part)   (+ D[d] u[b, d, t]), times z sigmoid(z) if z is given
    B / C: input-dependent (batch, dstate, seqlen) or (batch, groups, dstate, seqlen) -- with complex A a real last axis of 2 seqlen, (re, im)
    interleaved, or complex -- or constant (dim, dstate). -> (out (batch, dim, seqlen) of u's dtype, the state after the last step (batch, dim,
    dstate)); initial_state is left as it is. What the tests compare the kernel with; never a fallback: nothing in the package calls it."""
    batch, dim, L = u.shape
    cplx = A.is_complex()
    work = torch.promote_types(u.dtype, A.real.dtype if cplx else A.dtype)
    cwork = torch.promote_types(work, A.dtype)
    dt = delta.to(work) if delta_bias is None else delta.to(work) + delta_bias.to(work)[None, :, None]
    if delta_softplus:
        dt = torch.where(dt > 20, dt, torch.log1p(torch.exp(dt.clamp(max=20))))
    uw = u.to(work)

    def per_channel(M):      # -> (batch or 1, dim, dstate, seqlen or 1)
        if M.dim() == 2:
            return M.to(cwork)[None, :, :, None]
        if M.dim() == 3:
            M = M.unsqueeze(1)
        if cplx and not M.is_complex():
            M = torch.view_as_complex(M.to(work).reshape(*M.shape[:-1], L, 2).contiguous())
        return M.to(cwork).repeat_interleave(dim // M.shape[1], dim=1)

    Bf, Cf = per_channel(B), per_channel(C)
    Aw = A.to(cwork)
    h = torch.zeros(batch, dim, A.shape[1], dtype=cwork, device=u.device) if initial_state is None else initial_state.to(cwork).clone()
    ys = []
    for t in range(L):
        step = dt[:, :, t, None]
        h = h * torch.exp(step * Aw[None]) + (step * uw[:, :, t, None]) * Bf[..., t if Bf.shape[-1] > 1 else 0]
        y = (h * Cf[..., t if Cf.shape[-1] > 1 else 0]).sum(-1)
        ys.append(2 * y.real if cplx else y)
    out = torch.stack(ys, dim=-1)
    if D is not None:
        out = out + D.to(work)[None, :, None] * uw
    if z is not None:
        zw = z.to(work)
        out = out * zw * torch.sigmoid(zw)
    return out.to(u.dtype), h
