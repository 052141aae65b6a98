"""The top-1 mixture-of-experts layer as ONE autograd function over the HIP row passes of csrc/moe.hip (the experts' activation: csrc/act_rows.hip) and per-expert GEMMs on contiguous row
slices (SwitchMLP.forward, dimsum/switch_mlp.py:69-99; the expert, dimsum/mlp.py:42-46):

    forward : route (router dot products, sigmoid / softmax, first-argmax, stable counting sort by expert)  ->  ONE host read of the E + 1 offsets
              xp = x[perm]  ->  per expert e over rows [o_e, o_e+1): h1 = xp W1_e^T  ->  h = gelu_erf(h1a + b) (h1g + b)  [one pass, bias by row]
              ->  y = h W2_e^T + b2_e  ->  out[perm[j]] = prob y[j]
    backward: (dy, dprob) from (dout, y) in one pass  ->  per expert dW2, db2, dh  ->  the activation's adjoint (dbias per expert)  ->  per expert
              dW1, dxp  ->  dx = dxp[inv] + dlogit W_r, dW_r, db_r in one pass (dlogit from the saved logits)
An expert without tokens gets zero gradients (the reference calls every expert, with zero rows). The reference's forward runs E nonzero() host
synchronisations, E indexed gathers and E indexed scatters into a zero-filled buffer instead.

A layer built with grouped=True serves calls that do not train from switch_mlp_grouped_fwd instead: the same passes around ONE grouped GEMM launch per
projection (native.moe_gemm, csrc/moe_gemm.hip) that reads the offsets on the device -- no host read, so the layer can sit inside a captured hipGraph.

Under the "f16s" policy with allow_tf32 (gemm.moe_f16s_enabled: from DIMSUM_SPLIT3_MIN_ROWS tokens on; DIMSUM_MOE_F16S=0 switches it off) that forward runs on scaled-fp16 images instead:
the permute and the activation write the images, native.moe_gemm_f16s (csrc/moe_gemm_f16.hip) multiplies them with ONE fp16 product per element.
Still six launches and no host read; calls that train, grouped_train and the "fp16" policy are untouched.

A layer built with grouped_train=True sends the calls that TRAIN through _SwitchMlpGroupedFn: the grouped forward's launches, and a backward of
    combine_bwd -> wgrad(dy, h) (+ db2) -> dgrad(dy, W2) -> the activation's adjoint -> wgrad(dh1, xp) -> dgrad(dh1, W1) -> route_bwd
on the grouped GEMM's data and weight gradients (native.moe_gemm_dgrad / moe_gemm_wgrad, csrc/moe_gemm_bwd.hip). The offsets stay a device tensor from
the routing pass to the last gradient: no host read in a training step, 4 GEMM launches backward instead of 4 E, and an expert without tokens gets
the zeros the wgrad kernel stores for an empty range. Opt-in and independent of `grouped`.

`switch_mlp_torch` / `moe_act_torch`: float64 restatements of the reference's expressions -- checkers, not product paths."""
import torch
import torch.nn.functional as F

from .. import gemm, native


def route_kind(routing_mode):
    """the reference applies a sigmoid for routing_mode == 'sinkhorn' and a softmax for every other value (switch_mlp.py:75-80)"""
    return "sigmoid" if routing_mode == "sinkhorn" else "softmax"


def _mm_nt(a, w, out, bias=None, fp16=False):
    """out (a view of the layer's buffer) = a w^T (+ bias); fp16: the "fp16" inference policy's operands (decided by the caller OUTSIDE the
    autograd function: inside its forward grad mode is off and the policy's training guard could not fire)"""
    if fp16:
        y = gemm.linear(a, w)
        out.copy_(y if bias is None else y + bias)
    elif bias is None:
        torch.mm(a, w.t(), out=out)
    else:
        torch.addmm(bias, a, w.t(), out=out)


class _MoeActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, gated):
        x = x.contiguous()
        ctx.save_for_backward(x, bias)
        ctx.gated = gated
        return native.moe_act_fwd(x, bias, None, gated)

    @staticmethod
    def backward(ctx, dh):
        x, bias = ctx.saved_tensors
        dx, dbias = native.moe_act_bwd(x, bias, None, dh.contiguous(), ctx.gated, need_dbias=bias is not None and ctx.needs_input_grad[1])
        return dx, dbias, None


def moe_act(x, bias=None, gated=True):
    """x (rows, 2 W | W), bias (2 W | W) or None -> gelu_erf(a + b) (g + b) or gelu_erf(x + b): the expert MLP's activation outside a SwitchMLP
    (the pass of the mixture with one expert)"""
    return _MoeActFn.apply(x, None if bias is None else bias.float().reshape(1, -1), gated)


class _SwitchMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rw, rb, kind, gated, n_exp, has_bias, fp16, *ws):
        E = n_exp
        w1, w2 = ws[:E], ws[E:2 * E]
        b1 = torch.stack(ws[2 * E:3 * E]).contiguous() if has_bias else None
        b2 = ws[3 * E:4 * E] if has_bias else None
        H = x.shape[-1]
        x2 = x.reshape(-1, H).contiguous()
        T = x2.shape[0]
        prob, expert, logits, offsets, perm, inv, row_expert = native.moe_route_fwd(x2, rw.contiguous(), rb, kind)
        off = offsets.tolist()                          # the layer's one device-to-host copy: E + 1 ints
        xp = native.moe_permute(x2, perm)
        h1 = x2.new_empty(T, w1[0].shape[0])
        for e in range(E):
            if off[e + 1] > off[e]:
                _mm_nt(xp[off[e]:off[e + 1]], w1[e], h1[off[e]:off[e + 1]], fp16=fp16)
        h = native.moe_act_fwd(h1, b1, row_expert, gated)
        y = x2.new_empty(T, H)
        for e in range(E):
            if off[e + 1] > off[e]:
                _mm_nt(h[off[e]:off[e + 1]], w2[e], y[off[e]:off[e + 1]], None if b2 is None else b2[e], fp16=fp16)
        out = native.moe_combine_fwd(y, perm, prob)
        ctx.save_for_backward(x2, rw, logits, prob, expert, perm, inv, row_expert, xp, h1, h, y, b1, *w1, *w2)
        ctx.off, ctx.kind, ctx.gated, ctx.E, ctx.has_bias = off, kind, gated, E, has_bias
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        x2, rw, logits, prob, expert, perm, inv, row_expert, xp, h1, h, y, b1 = ctx.saved_tensors[:13]
        E, off = ctx.E, ctx.off
        w1, w2 = ctx.saved_tensors[13:13 + E], ctx.saved_tensors[13 + E:13 + 2 * E]
        T, H = x2.shape
        dy, dprob = native.moe_combine_bwd(dout.reshape(T, H).contiguous(), y, perm, prob)
        dh = torch.empty_like(h)
        dw1, dw2, db2 = [], [], []
        for e in range(E):
            o0, o1 = off[e], off[e + 1]
            if o1 == o0:
                dw2.append(torch.zeros_like(w2[e]))
                db2.append(torch.zeros(H, device=dy.device, dtype=dy.dtype))
                continue
            dw2.append(gemm.mm_tn(dy[o0:o1], h[o0:o1]))
            if ctx.has_bias:
                db2.append(dy[o0:o1].sum(0))
            torch.mm(dy[o0:o1], w2[e], out=dh[o0:o1])
        dh1, db1 = native.moe_act_bwd(h1, b1, row_expert, dh, ctx.gated, need_dbias=ctx.has_bias)
        dxp = torch.empty_like(xp)
        for e in range(E):
            o0, o1 = off[e], off[e + 1]
            if o1 == o0:
                dw1.append(torch.zeros_like(w1[e]))
                continue
            dw1.append(gemm.mm_tn(dh1[o0:o1], xp[o0:o1]))
            torch.mm(dh1[o0:o1], w1[e], out=dxp[o0:o1])
        dx, drw, drb = native.moe_route_bwd(x2, rw.contiguous(), logits, prob, expert, inv, dprob, dxp, ctx.kind)
        grads = dw1 + dw2 + ((list(db1.unbind(0)) + db2) if ctx.has_bias else [])
        return (dx.view(dout.shape), drw, drb if ctx.needs_input_grad[2] else None, None, None, None, None, None, *grads)


class _SwitchMlpGroupedFn(torch.autograd.Function):
    """the layer that TRAINS on the grouped expert GEMM: switch_mlp_grouped_fwd's launches forward (so its output is the grouped inference forward's,
    bit for bit), and a backward on the grouped GEMM's two gradients (native.moe_gemm_dgrad / moe_gemm_wgrad, csrc/moe_gemm_bwd.hip). The offsets
    are saved as the device tensor they are: no host read in either direction, one launch per product whatever the number of experts, and the
    zero gradients of an expert without tokens are written by the wgrad kernel."""

    @staticmethod
    def forward(ctx, x, rw, rb, kind, gated, n_exp, has_bias, *ws):
        E = n_exp
        w1, w2 = ws[:E], ws[E:2 * E]
        b1 = torch.stack(ws[2 * E:3 * E]).contiguous() if has_bias else None
        b2 = torch.stack(ws[3 * E:4 * E]).contiguous() if has_bias else None
        H = x.shape[-1]
        x2 = x.reshape(-1, H).contiguous()
        rw = rw.contiguous()
        prob, expert, logits, offsets, perm, inv, row_expert = native.moe_route_fwd(x2, rw, rb, kind)
        xp = native.moe_permute(x2, perm)
        h1 = native.moe_gemm(xp, offsets, list(w1))
        h = native.moe_act_fwd(h1, b1, row_expert, gated)
        y = native.moe_gemm(h, offsets, list(w2), bias=b2)
        out = native.moe_combine_fwd(y, perm, prob)
        ctx.save_for_backward(x2, rw, logits, prob, expert, perm, inv, row_expert, offsets, xp, h1, h, y, b1, *w1, *w2)
        ctx.kind, ctx.gated, ctx.E, ctx.has_bias = kind, gated, E, has_bias
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):
        x2, rw, logits, prob, expert, perm, inv, row_expert, offsets, xp, h1, h, y, b1 = ctx.saved_tensors[:14]
        E, need = ctx.E, ctx.needs_input_grad
        w1, w2 = list(ctx.saved_tensors[14:14 + E]), list(ctx.saved_tensors[14 + E:14 + 2 * E])
        T, H = x2.shape
        need_w1, need_w2 = any(need[7:7 + E]), any(need[7 + E:7 + 2 * E])
        need_b1, need_b2 = ctx.has_bias and any(need[7 + 2 * E:7 + 3 * E]), ctx.has_bias and any(need[7 + 3 * E:7 + 4 * E])
        need_route = any(need[:3])                          # x or the router: the last dgrad and the router's adjoint
        dy, dprob = native.moe_combine_bwd(dout.reshape(T, H).contiguous(), y, perm, prob)
        none = [None] * E
        dw1, dw2, db1, db2 = none, none, none, none
        if need_w2 or need_b2:                              # frozen experts: no launch
            dw2, db = native.moe_gemm_wgrad(dy, h, offsets, E, need_dbias=need_b2)
            db2 = none if db is None else list(db.unbind(0))
        dx = drw = drb = None
        if need_w1 or need_b1 or need_route:
            dh = native.moe_gemm_dgrad(dy, offsets, w2)
            dh1, db = native.moe_act_bwd(h1, b1, row_expert, dh, ctx.gated, need_dbias=need_b1)
            db1 = none if db is None else list(db.unbind(0))
            if need_w1:
                dw1, _ = native.moe_gemm_wgrad(dh1, xp, offsets, E)
            if need_route:
                dxp = native.moe_gemm_dgrad(dh1, offsets, w1)
                dx, drw, drb = native.moe_route_bwd(x2, rw, logits, prob, expert, inv, dprob, dxp, ctx.kind)
                dx = dx.view(dout.shape)
        grads = dw1 + dw2 + ((db1 + db2) if ctx.has_bias else [])
        return (dx, drw, drb if need[2] else None, None, None, None, None, *[g if n else None for g, n in zip(grads, need[7:])])


def switch_mlp_grouped_fwd(x, router_weight, router_bias, fc1_weights, fc2_weights, fc1_biases, fc2_biases, kind, gated):
    """the inference forward on the grouped expert GEMM (native.moe_gemm, csrc/moe_gemm.hip): route -> permute -> fc1 -> activation -> fc2 (+ bias) ->
    combine, the expert offsets never leaving the device. No host synchronisation anywhere: the whole layer can be captured into a hipGraph. No
    autograd: the caller sends a call that trains to _SwitchMlpFn."""
    H = x.shape[-1]
    x2 = x.detach().reshape(-1, H).contiguous()
    prob, _, _, offsets, perm, _, row_expert = native.moe_route_fwd(x2, router_weight.detach().contiguous(), None if router_bias is None else router_bias.detach(), kind)
    if gemm.moe_f16s_enabled(x2, fc1_weights, fc2_weights):
        # policy "f16s": the same six launches on scaled-fp16 images -- the permute and the activation write the left operands of the two grouped
        # GEMMs themselves (csrc/moe_gemm_f16.hip: one fp16 product). The router and the routing pass above are the fp32 path's: the same experts.
        E = len(fc1_weights)
        images = gemm.expert_images_f16s([w.detach() for w in (*fc1_weights, *fc2_weights)])
        xp = native.moe_permute(x2, perm, split3="f16s")
        h1 = native.moe_gemm_f16s(xp, offsets, images[:E])
        b1 = None if fc1_biases is None else torch.stack([b.detach() for b in fc1_biases]).contiguous()
        h = native.moe_act_fwd(h1, b1, row_expert, gated, split3="f16s")
        b2 = None if fc2_biases is None else torch.stack([b.detach() for b in fc2_biases]).contiguous()
        y = native.moe_gemm_f16s(h, offsets, images[E:], bias=b2)
        return native.moe_combine_fwd(y, perm, prob).view(x.shape)
    xp = native.moe_permute(x2, perm)
    h1 = native.moe_gemm(xp, offsets, [w.detach() for w in fc1_weights])
    b1 = None if fc1_biases is None else torch.stack([b.detach() for b in fc1_biases]).contiguous()
    h = native.moe_act_fwd(h1, b1, row_expert, gated)
    b2 = None if fc2_biases is None else torch.stack([b.detach() for b in fc2_biases]).contiguous()
    y = native.moe_gemm(h, offsets, [w.detach() for w in fc2_weights], bias=b2)
    return native.moe_combine_fwd(y, perm, prob).view(x.shape)


def switch_mlp_fn(x, router_weight, router_bias, fc1_weights, fc2_weights, fc1_biases=None, fc2_biases=None, routing_mode="top1", gated=True,
                  grouped=False, grouped_train=False):
    """x (..., H) float32 on the GPU -> prob * expert_e(x) per token, e = the first maximum of sigmoid / softmax of the router logits.
    grouped: a call that does not train (grad mode off, or nothing requires grad) runs on the grouped expert GEMM with no host read of the expert
    offsets (switch_mlp_grouped_fwd); a call that trains takes _SwitchMlpFn whatever `grouped` says.
    grouped_train: a call that trains takes _SwitchMlpGroupedFn (the grouped GEMM and its two gradients: no host read forward or backward); it
    changes nothing for a call that does not train."""
    if x.dtype != torch.float32 or any(w.dtype != torch.float32 for w in (router_weight, *fc1_weights, *fc2_weights)):
        raise RuntimeError("switch_mlp: float32 tokens and parameters only (there is no other kernel and no fallback)")
    E = len(fc1_weights)
    has_bias = fc1_biases is not None
    ws = list(fc1_weights) + list(fc2_weights) + ((list(fc1_biases) + list(fc2_biases)) if has_bias else [])
    # decided here, OUTSIDE the autograd function (inside its forward grad mode is always off), like fp16 below
    trains = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, router_weight, router_bias, *ws))
    if grouped and not trains:
        return switch_mlp_grouped_fwd(x, router_weight, router_bias, fc1_weights, fc2_weights, fc1_biases, fc2_biases, route_kind(routing_mode), bool(gated))
    if grouped_train and trains:
        return _SwitchMlpGroupedFn.apply(x, router_weight, router_bias, route_kind(routing_mode), bool(gated), E, has_bias, *ws)
    # the "fp16" policy serves inference only (gemm._use_fp16): asked here, where grad mode and requires_grad still say whether this call trains
    fp16 = all(gemm._use_fp16(x, w) for w in (router_weight, *ws))
    return _SwitchMlpFn.apply(x, router_weight, router_bias, route_kind(routing_mode), bool(gated), E, has_bias, fp16, *ws)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements (checkers)
# ---------------------------------------------------------------------------------------------------------------------
def moe_act_torch(x, bias=None, row_expert=None, gated=True):
    """float64: gelu_erf(a + b_a) * (g + b_g) over the halves of x (gated) or gelu_erf(x + b); bias (E, S) rows picked by row_expert (None: row 0)"""
    x = x.double()
    if bias is not None:
        b = bias.double()
        x = x + (b[row_expert.long()] if row_expert is not None else b.reshape(-1, x.shape[-1])[0])
    if gated:
        a, g = x.chunk(2, dim=-1)
        return F.gelu(a) * g
    return F.gelu(x)


def switch_mlp_torch(x, router_weight, router_bias, fc1_weights, fc2_weights, fc1_biases=None, fc2_biases=None, routing_mode="top1", gated=True):
    """float64, differentiable -> (out like x, expert (T) int64): SwitchMLP.forward as the reference writes it (switch_mlp.py:69-99) with the
    indexed scatter as an index_copy"""
    H = x.shape[-1]
    x2 = x.double().reshape(-1, H)
    logits = x2 @ router_weight.double().t()
    if router_bias is not None:
        logits = logits + router_bias.double()
    route = torch.sigmoid(logits) if routing_mode == "sinkhorn" else torch.softmax(logits, dim=1)
    p, e = torch.max(route, dim=1)
    out = torch.zeros_like(x2)
    for i in range(len(fc1_weights)):
        idx = (e == i).nonzero().squeeze(1)
        h1 = x2[idx] @ fc1_weights[i].double().t()
        h = moe_act_torch(h1, None if fc1_biases is None else fc1_biases[i].double().reshape(1, -1), None, gated)
        y = h @ fc2_weights[i].double().t()
        if fc2_biases is not None:
            y = y + fc2_biases[i].double()
        out = out.index_copy(0, idx, y)
    return (out * p.unsqueeze(1)).view(x.shape), e
