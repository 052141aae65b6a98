"""The tail of a training step -- clip_grad_norm_ -> AdamW.step -> update_ema (dimsum/train.py:55-64, 317-321) -- on the library's own two
launches (include/dimsum_hip.h, dimsum_optim_*): one read of the gradients for the global norm, then one pass that reads g, p, m, v, ema and
writes p, m, v, ema. 10 full-size fp32 streams instead of the 15 of the three torch operations.

`FusedAdamWEMA` is a torch.optim.AdamW: the same constructor, param_groups and per-parameter state ("step" as a float32 device scalar,
"exp_avg", "exp_avg_sq": the layout of torch's fused AdamW), so state_dict() / load_state_dict() interchange with torch.optim.AdamW in both
directions, the reference's non-fused checkpoints (CPU "step" tensors) included. Hyper-parameters are read from param_groups at every step.

One documented difference: the gradients are only READ. After step_fused(max_grad_norm) `.grad` still holds the unclipped gradient, where
clip_grad_norm_ scales it in place. There is no CPU path."""
import torch

from . import _lib, native


class _Plan:
    """everything that depends on the tensor list only, built once and kept on the device: the pointer tables (row G is rewritten every step),
    sizes, the chunk table, the partial sums; + the host-side objects whose identity says that the tables still describe the optimizer"""
    P, M, V, E, S, G = range(6)


class FusedAdamWEMA(torch.optim.AdamW):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        for name, flag in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable),
                           ("foreach", foreach)):
            if flag:
                raise ValueError(f"FusedAdamWEMA: {name}=True is out of scope of the fused kernel")
        if fused is not None and not fused:
            raise ValueError("FusedAdamWEMA is the fused step: fused=False is not available")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdamWEMA: lr must be a float (a tensor lr would need a host synchronisation every step)")
        self._ema, self._ema_extra, self._ema_decay = {}, [], None
        self._plan, self._call, self._last_norm = None, None, None
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, fused=True)

    # ---- construction / state ----------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if not p.is_cuda:
                raise RuntimeError("dimsum_amd.optim.FusedAdamWEMA: expected GPU parameters (there is no CPU fallback)")
            if p.dtype != torch.float32:
                raise TypeError(f"FusedAdamWEMA: float32 parameters only, got {p.dtype}")
            if not p.is_contiguous():
                raise RuntimeError("FusedAdamWEMA: parameters must be contiguous")
        self._plan = None

    def __setstate__(self, state):
        """load_state_dict() and unpickling end here: bring a foreign state (torch.optim.AdamW fused or not; "step" on the CPU or a number)
        into this class's layout"""
        unpickled = "_ema" in state              # a copy's parameters are new objects: the EMA pairing (by identity) has to be attached again
        super().__setstate__(state)
        if unpickled:
            self._ema, self._ema_extra = {}, []
        for g in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if g.get(name):
                    raise ValueError(f"FusedAdamWEMA: the loaded state asks for {name}=True, which the fused kernel does not do")
            g["fused"], g["foreach"] = True, None
            for p in g["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())
                    for k in ("exp_avg", "exp_avg_sq"):
                        st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        self.__dict__.setdefault("_ema", {})
        self.__dict__.setdefault("_ema_extra", [])
        self.__dict__.setdefault("_ema_decay", None)
        self._plan, self._call, self._last_norm = None, None, None

    def attach_ema(self, model, ema_model, decay=None):
        """pair the parameters of `model` (a DistributedDataParallel wrapper is looked through) with those of `ema_model` BY NAME, as update_ema
        does. `decay`: the blend of plain step() calls (None: step() leaves the EMA alone; step_fused(ema_decay=...) names its own)."""
        net = model.module if hasattr(model, "module") else model
        ema_params = dict(ema_model.named_parameters())
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        self._ema, self._ema_extra = {}, []
        for name, p in net.named_parameters():
            e = ema_params[name]
            if not (e.is_cuda and p.is_cuda and e.device == p.device):
                raise RuntimeError("FusedAdamWEMA.attach_ema: expected GPU parameters on one device (there is no CPU fallback)")
            if e.dtype != torch.float32 or p.dtype != torch.float32:
                raise TypeError("FusedAdamWEMA.attach_ema: float32 parameters only")
            if e.shape != p.shape or not e.is_contiguous() or not p.is_contiguous():
                raise RuntimeError(f"FusedAdamWEMA.attach_ema: {name} must be contiguous and of one shape in both models")
            self._ema[id(p)] = e
            if id(p) not in mine:                      # not optimised: no gradient is ever applied, the EMA still follows
                self._ema_extra.append(p)
        self._ema_decay = decay
        self._plan = None

    # ---- the step ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step_fused(self, max_grad_norm=None, ema_decay=None):
        """clip to `max_grad_norm` (None: no clipping) -> AdamW -> EMA with `ema_decay` (None: attach_ema's decay; no EMA without one) ->
        the total gradient norm as a 0-dim device tensor (what clip_grad_norm_ returns). No host synchronisation."""
        self._call = (max_grad_norm, ema_decay)
        try:
            self.step()              # through torch's step wrapper: hooks and LR schedulers see an ordinary step
        finally:
            self._call = None
        norm, self._last_norm = self._last_norm, None
        return norm

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._call is None:
            self._run(None, None, False)
        else:
            self._last_norm = self._run(self._call[0], self._call[1], True)
        return loss

    def _tensors(self):
        """[(parameter, group index)] in table order: the groups' parameters, then the EMA-only ones (group -1)"""
        return [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]] + [(p, -1) for p in self._ema_extra]

    def _build_plan(self, entries, ms, vs, ss, es):
        plan = _Plan()
        device = entries[0][0].device
        n = len(entries)
        plan.device, plan.n = device, n
        plan.params, plan.p_ptrs = [p for p, _ in entries], [p.data_ptr() for p, _ in entries]
        plan.m, plan.v, plan.s, plan.e = ms, vs, ss, es
        plan.numel, plan.chunks = native.optim_tables([p.numel() for p, _ in entries], device)
        plan.table = torch.empty(6, n, dtype=torch.int64, device=device)
        ptr = lambda t: 0 if t is None else t.data_ptr()                                           # noqa: E731
        native.optim_write_ptrs(plan.table, 0, plan.p_ptrs + [ptr(t) for row in (ms, vs, es, ss) for t in row])
        per = [(p.numel() + _lib.OPTIM_CHUNK - 1) // _lib.OPTIM_CHUNK for p, _ in entries]
        # chunk range of every group (table order = group order); the EMA-only tensors ride with the last group
        plan.ranges, c = [], 0
        for gi in range(len(self.param_groups)):
            c0 = c
            c += sum(k for k, (_, g) in zip(per, entries) if g == gi)
            plan.ranges.append([c0, c])
        if plan.ranges:
            plan.ranges[-1][1] = plan.chunks.shape[0]
        plan.n_partials = min(plan.chunks.shape[0], _lib.OPTIM_MAX_PARTIALS)
        plan.partials = torch.empty(plan.n_partials, dtype=torch.float32, device=device)
        return plan

    def _run(self, max_grad_norm, ema_decay, want_norm):
        entries = self._tensors()
        if not entries:
            return None
        device = entries[0][0].device
        if ema_decay is None:
            ema_decay = self._ema_decay
        use_ema = ema_decay is not None and bool(self._ema)
        plan = self._plan
        ok = plan is not None and plan.n == len(entries)
        g_ptrs, keep, ms, vs, ss, es = [], [], [], [], [], []
        for i, (p, gi) in enumerate(entries):
            if p.device != device:
                raise RuntimeError("FusedAdamWEMA: all parameters must live on one GPU")
            g = p.grad if gi >= 0 else None
            st = self.state[p] if (g is not None or p in self.state) else None
            if g is not None:
                if g.is_sparse:
                    raise RuntimeError("FusedAdamWEMA does not support sparse gradients")
                if g.dtype != torch.float32:
                    raise TypeError(f"FusedAdamWEMA: float32 gradients only, got {g.dtype}")
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                if len(st) == 0:           # first gradient of this parameter: torch's fused AdamW state
                    st["step"] = torch.zeros((), dtype=torch.float32, device=device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g_ptrs.append(g.data_ptr())
            else:
                g_ptrs.append(0)
            m, v, s = (st["exp_avg"], st["exp_avg_sq"], st["step"]) if st else (None, None, None)
            e = self._ema.get(id(p))
            ms.append(m), vs.append(v), ss.append(s), es.append(e)
            ok = ok and plan.m[i] is m and plan.v[i] is v and plan.s[i] is s and plan.e[i] is e and plan.p_ptrs[i] == p.data_ptr()
        if not ok:
            plan = self._plan = self._build_plan(entries, ms, vs, ss, es)
        # the gradients are new allocations every step (zero_grad(set_to_none=True)): their row of the table is rewritten every step
        native.optim_write_ptrs(plan.table, _Plan.G * plan.n, g_ptrs)

        row = lambda r: plan.table[r].data_ptr()                                                    # noqa: E731
        total_norm = torch.empty((), dtype=torch.float32, device=device) if want_norm else None

        def params(group, c0, c1):
            P = _lib.OptimParams()
            P.n_tensors, P.n_chunks, P.n_partials = plan.n, c1 - c0, plan.n_partials
            P.p_ptrs, P.g_ptrs, P.m_ptrs, P.v_ptrs, P.step_ptrs = row(_Plan.P), row(_Plan.G), row(_Plan.M), row(_Plan.V), row(_Plan.S)
            P.ema_ptrs = row(_Plan.E) if use_ema else None
            P.numel, P.chunk_table = plan.numel.data_ptr(), plan.chunks.data_ptr() + 8 * c0
            P.partials = plan.partials.data_ptr() if want_norm else None
            P.total_norm = total_norm.data_ptr() if want_norm else None
            if isinstance(group["lr"], torch.Tensor):
                raise ValueError("FusedAdamWEMA: lr must be a float")
            P.lr, (P.beta1, P.beta2), P.eps, P.weight_decay = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            P.max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
            P.ema_decay = float(ema_decay) if use_ema else 0.0
            return P

        native.optim_grad_sumsq(params(self.param_groups[0], 0, plan.chunks.shape[0]), device)
        for group, (c0, c1) in zip(self.param_groups, plan.ranges):
            if c1 > c0:
                native.optim_adamw_ema_step(params(group, c0, c1), device)
        del keep
        return total_norm
