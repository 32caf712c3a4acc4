"""FusedAdamW: torch.optim.AdamW whose step - together with the gradient's sum of squares, clip_grad_value_ and update_ema of the
training loop (human_diffusion/improved_diffusion/train_util.py optimize_normal) - is one HIP launch (csrc/hl_optim.hip).

    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.0)
    opt.attach_ema([ema_params_0999, ema_params_09999], [0.999, 0.9999])
    ...backward...
    opt.step(clip_value=0.5)          # norm of the UNCLIPPED gradient, clip, AdamW, EMA; no host synchronisation
    opt.grad_sqsum                    # () float64 device tensor: sum of g*g over every gradient of the last step

state_dict() / load_state_dict() have torch.optim.AdamW's layout (per parameter `step`, `exp_avg`, `exp_avg_sq`; AdamW's param_group
keys), so a checkpoint written by either optimizer loads into the other.  Differences from AdamW + clip_grad_value_ on purpose:
  - .grad is left UNCLIPPED (the kernel clamps a register copy; writing the clipped values back would add 2 bytes per 4 of traffic
    and nothing of the training loop reads them);
  - fp32 parameters on one HIP device only; amsgrad / maximize / capturable / differentiable are refused.
There is no eager fallback: a missing library or a bad argument raises.
"""
import ctypes as C

import torch

from . import _lib

MAX_EMA = 4


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad or maximize or capturable or differentiable or fused:
            raise NotImplementedError("FusedAdamW: amsgrad, maximize, capturable, differentiable and fused are not supported")
        # AdamW's own param_group keys, so that the two optimizers' state_dicts are interchangeable
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=foreach,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._ema = []                     # [(rate, [target tensor per parameter, in param_groups order])]
        self._plans = None                 # cached launch plans, see _plan()
        self._key = None
        self.grad_sqsum = None

    # ---- EMA targets ----------------------------------------------------------------------------------------------------------
    def attach_ema(self, param_lists, rates):
        """Register EMA targets: param_lists[k][i] follows parameter i (param_groups order) at rates[k] after every step."""
        params = self._params()
        rates = [float(r) for r in rates]
        if len(param_lists) != len(rates) or len(rates) > MAX_EMA:
            raise ValueError(f"attach_ema: one list per rate, at most {MAX_EMA} rates")
        ema = []
        for rate, lst in zip(rates, param_lists):
            lst = list(lst)
            if len(lst) != len(params):
                raise ValueError(f"attach_ema: {len(lst)} targets for {len(params)} parameters")
            for e, p in zip(lst, params):
                if e.shape != p.shape or e.dtype != p.dtype or e.device != p.device or not e.is_contiguous():
                    raise ValueError("attach_ema: every target must be a contiguous tensor of its parameter's shape, dtype and device")
            ema.append((rate, lst))
        self._ema = ema
        self._plans = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = None                 # new moment tensors: the table is packed again

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    # ---- the table --------------------------------------------------------------------------------------------------------------
    def _state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)   # (on the host, as AdamW keeps it when not capturable)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _plan(self):
        """One launch per (param group, step count) among the parameters with a gradient - one in a training loop, where every
        parameter steps together; parameters without a gradient ride along in the first launch for their EMA.  The tables are packed
        on the host and copied to the device when a parameter or gradient pointer changes (or a gradient appears or goes), otherwise
        reused as they are: the check costs two data_ptr() per parameter."""
        params = self._params()
        grads = [p.grad for p in params]
        key = tuple((p.data_ptr(), 0 if g is None else g.data_ptr()) for p, g in zip(params, grads))
        if self._plans is not None and self._key == key:
            return self._plans
        if not params:
            raise RuntimeError("FusedAdamW: no parameters")
        dev = params[0].device
        for p, g in zip(params, grads):
            if p.device != dev or not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("FusedAdamW: every parameter must be a contiguous float32 tensor on one HIP device")
            if g is not None and (g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev):
                raise RuntimeError("FusedAdamW: every gradient must be a dense contiguous float32 tensor on the parameter's device")
        buckets, nograd, fi = {}, [], 0
        for gi, grp in enumerate(self.param_groups):
            for p in grp["params"]:
                if p.grad is None:
                    nograd.append((fi, p, False))
                else:
                    buckets.setdefault((gi, float(self._state(p)["step"])), []).append((fi, p, True))
                fi += 1
        order = sorted(buckets) or [None]                     # None: no gradient anywhere - nothing to step, the EMA alone
        L = _lib.lib()
        plans = []
        for bi, bk in enumerate(order):
            its = (buckets[bk] if bk is not None else []) + (nograd if bi == 0 else [])
            n = len(its)
            numel = (C.c_int64 * n)(*[p.numel() for _, p, _ in its])
            ptrs = (C.c_void_p * (8 * n))()
            for j, (i, p, has_grad) in enumerate(its):
                ptrs[8 * j] = p.data_ptr()
                if has_grad:
                    st = self.state[p]
                    ptrs[8 * j + 1] = p.grad.data_ptr()
                    ptrs[8 * j + 2] = st["exp_avg"].data_ptr()
                    ptrs[8 * j + 3] = st["exp_avg_sq"].data_ptr()
                for k, (_, lst) in enumerate(self._ema):
                    ptrs[8 * j + 4 + k] = lst[i].data_ptr()
            nchunks = int(L.hl_adamw_chunks(numel, n))
            if nchunks <= 0:
                raise RuntimeError("FusedAdamW: empty parameter tensor")
            tb = int(L.hl_adamw_table_bytes(n, nchunks))
            host = torch.empty(tb, dtype=torch.uint8, pin_memory=True)
            _lib.check(L.hl_adamw_table_pack(n, numel, ptrs, len(self._ema), C.c_void_p(host.data_ptr()), tb), "hl_adamw_table_pack")
            table = host.to(dev, non_blocking=True)             # (the caching host allocator keeps `host` until the copy is done)
            stepped = [p for _, p, hg in its if hg]
            plans.append(dict(group=None if bk is None else bk[0], n=n, nchunks=nchunks, table=table, stepped=stepped,
                              steps=[self.state[p]["step"] for p in stepped]))
        total = sum(pl["nchunks"] for pl in plans)
        scratch = torch.empty(total, dtype=torch.float64, device=dev)
        off = 0
        for pl in plans:
            pl["scratch"] = scratch[off:off + pl["nchunks"]]
            off += pl["nchunks"]
        self._plans = dict(plans=plans, scratch=scratch, sqsum=torch.zeros((), dtype=torch.float64, device=dev), device=dev)
        self._key = key
        return self._plans

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, clip_value=None):
        """One fused launch: grad sum of squares (unclipped), clamp to [-clip_value, clip_value] when given, AdamW, EMA.
        Returns the closure's loss like torch's optimizers.  Enqueue-only: the host is not synchronised."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        P = self._plan()
        L = _lib.lib()
        dev = P["device"]
        rates = (C.c_float * (2 * MAX_EMA))()
        for k, (r, _) in enumerate(self._ema):
            rates[2 * k] = r                                   # (float)r, (float)(1 - r): the mul_ and add_ scalars of update_ema
            rates[2 * k + 1] = 1.0 - r
        clip = float(clip_value) if clip_value is not None else 0.0
        if clip_value is not None and not clip > 0:
            raise ValueError("clip_value must be positive")
        with _lib.on(dev):
            stream = _lib.stream_ptr(dev)
            for pl in P["plans"]:
                if pl["group"] is None:                         # EMA only (no parameter has a gradient)
                    a = (1.0, 0.9, 0.999, 1.0, 1e-8, 0.0)
                else:
                    grp = self.param_groups[pl["group"]]
                    lr, (b1, b2), eps, wd = float(grp["lr"]), grp["betas"], grp["eps"], grp["weight_decay"]
                    torch._foreach_add_(pl["steps"], 1)        # (host tensors: no device work)
                    step = float(pl["steps"][0])
                    # the scalars in double on the host, as torch computes them, handed to the kernel as floats
                    bc1 = 1.0 - b1 ** step
                    bc2 = 1.0 - b2 ** step
                    a = (1.0 - lr * wd if wd != 0 else 1.0, b1, b2, bc2 ** 0.5, eps, -(lr / bc1))
                wd_scale, b1, b2, bc2s, eps, neg_step = a
                _lib.check(L.hl_adamw_step(C.c_void_p(pl["table"].data_ptr()), pl["n"], pl["nchunks"], len(self._ema), rates, clip,
                                           wd_scale, 1.0 - b1, b2, 1.0 - b2, bc2s, eps, neg_step, C.c_void_p(pl["scratch"].data_ptr()),
                                           pl["scratch"].numel() * 8, stream), "hl_adamw_step")
            _lib.check(L.hl_adamw_sum_partials(C.c_void_p(P["scratch"].data_ptr()), P["scratch"].numel(),
                                               C.c_void_p(P["sqsum"].data_ptr()), stream), "hl_adamw_sum_partials")
        self.grad_sqsum = P["sqsum"]
        return loss
