"""Adam and AdamW whose step is one hand-written multi-tensor HIP launch per parameter group (csrc/optim.hip).

    from gridnext_amd import optim
    opt = optim.Adam(model.parameters(), lr=1e-3)

Drop-in for `torch.optim.Adam` / `torch.optim.AdamW` in the loops of `training.py` (which accept any optimizer): both subclass
`torch.optim.Optimizer`, so `param_groups`, `zero_grad`, learning-rate schedulers and checkpointing work unchanged, and the
per-parameter state `{'step': 0-dim float32 tensor on the parameter's device, 'exp_avg', 'exp_avg_sq'}` is torch's own
layout: `state_dict()` loads into the torch classes and theirs loads into these.

`step()` walks no tensor on the host beyond collecting addresses: the pointers of every parameter that has a gradient go to
`gnx_adam_step` as one table, the step counts advance on the device, nothing is read back and nothing synchronises, so the
call can be captured into a hipGraph (a replay is valid while the parameters, their `.grad` tensors and the state keep their
addresses - the table travels in the kernel arguments).  After the launch every updated parameter's version counter is
bumped: the kernel writes through raw pointers, and the DenseNet's derived-weight cache, its tape guard and the frozen MLP's
composed stages are all keyed on `_version`.  The bump is host code: it runs when `step()` is called or captured, NOT when a
captured step is replayed.  Whoever replays such a graph must call `functional.bump_versions(*params)` on the updated
parameters after every replay (as the graph steppers of `graphs.py` do for BatchNorm buffers), or those caches go stale.

fp32 parameters on a HIP device only; there is no CPU path.  amsgrad, maximize, sparse gradients and a tensor `lr` are
refused by name.
"""
import ctypes

import torch
from torch.optim import Optimizer

from . import _lib as L
from .functional import bump_versions

__all__ = ['Adam', 'AdamW', 'chunk_elements', 'table_tensors']


def chunk_elements():
    """Elements one block of the step kernel updates (tensors are cut into chunks of this many)."""
    return int(L.query('gnx_adam_chunk'))


def table_tensors():
    """Tensors one launch holds; a longer parameter group takes ceil(n / this) launch pairs."""
    return int(L.query('gnx_adam_table_tensors'))


def _dense(t):
    return t.is_contiguous() or t.is_non_overlapping_and_dense()


class _Plan:
    """What one group's launch needs, kept while the addresses stand: the pointer table as ctypes arrays, the coefficient
    workspace, the parameters to bump and the gradients that must be copied to the parameter's layout first."""
    __slots__ = ('key', 'n', 'arrays', 'coef', 'params', 'staged', 'device')


class Adam(Optimizer):
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise TypeError("gridnext_amd.optim: lr as a tensor is not supported; pass a Python number")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: %r" % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: %r" % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        self._plans = {}
        # (torch's key names, so that a state dict of ours configures a torch.optim.Adam/AdamW alike and the reverse)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        decoupled_weight_decay=self._decoupled)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------ refusals
    @staticmethod
    def _refuse_group(group):
        if group.get('amsgrad', False):
            raise NotImplementedError("gridnext_amd.optim: amsgrad=True is not implemented by the HIP Adam step")
        if group.get('maximize', False):
            raise NotImplementedError("gridnext_amd.optim: maximize=True is not implemented by the HIP Adam step")
        if isinstance(group['lr'], torch.Tensor):
            raise TypeError("gridnext_amd.optim: lr as a tensor is not supported; pass a Python number")

    @staticmethod
    def _refuse_dtype(p):
        if p.dtype != torch.float32:
            raise TypeError("gridnext_amd.optim: the HIP Adam step updates float32 parameters only, got a %s parameter of "
                            "shape %s" % (p.dtype, tuple(p.shape)))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._refuse_group(group)
            for p in group['params']:
                self._refuse_dtype(p)
        except Exception:
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__['_plans'] = {}
        for group in self.param_groups:
            group.setdefault('amsgrad', False)
            group.setdefault('maximize', False)
            group['decoupled_weight_decay'] = self._decoupled or bool(group.get('decoupled_weight_decay', False))

    def load_state_dict(self, state_dict):
        for group in state_dict['param_groups']:
            self._refuse_group(group)
        super().load_state_dict(state_dict)
        # torch keeps a non-capturable optimizer's `step` on the CPU, and old checkpoints hold Python numbers: ours lives
        # where the parameter does, as float32
        for group in self.param_groups:
            for p in group['params']:
                st = self.state.get(p)
                if st and 'step' in st:
                    step = st['step']
                    if not torch.is_tensor(step):
                        step = torch.tensor(float(step), dtype=torch.float32)
                    st['step'] = step.detach().to(device=p.device, dtype=torch.float32).reshape(())
        self._plans = {}

    # ------------------------------------------------------------------ the step
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._step_group(gi, group)
        return loss

    def _init_state(self, p, st):
        with torch.no_grad():
            st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _check_param(self, p):
        if not p.is_cuda:
            raise RuntimeError("gridnext_amd.optim: the Adam step is a HIP kernel and needs parameters on a HIP device "
                               "(got %s); there is no CPU path" % p.device)
        self._refuse_dtype(p)
        if not _dense(p):
            raise RuntimeError("gridnext_amd.optim: a parameter that is a strided view with gaps (shape %s, stride %s) is not "
                               "supported by the HIP Adam step" % (tuple(p.shape), p.stride()))

    def _step_group(self, gi, group):
        self._refuse_group(group)
        state = self.state
        live, key = [], []
        for p in group['params']:
            g = p.grad
            if g is None:
                continue                                  # torch's rule: no gradient, no update, no step count
            if g.layout is not torch.strided:
                raise RuntimeError("gridnext_amd.optim: sparse gradients are not supported by the HIP Adam step "
                                   "(parameter of shape %s)" % (tuple(p.shape),))
            st = state.get(p)
            if not st:
                self._check_param(p)                      # (before the state gets an entry: a refused step leaves none)
                st = state[p]
                self._init_state(p, st)
            live.append(p)
            key += (p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['step'].data_ptr())
        if not live:
            return
        plan = self._plans.get(gi)
        if plan is None or plan.key != key:
            plan = self._plans[gi] = self._build_plan(live, key)
        for p, staging in plan.staged:                    # a gradient laid out unlike its parameter: slow but correct
            with torch.no_grad():
                staging.copy_(p.grad)
        beta1, beta2 = group['betas']
        L.call('gnx_adam_step', *plan.arrays, plan.n, plan.coef.data_ptr(), float(group['lr']), float(beta1), float(beta2),
               float(group['eps']), float(group['weight_decay']), 1 if group.get('decoupled_weight_decay', False) else 0,
               torch.cuda.current_stream(plan.device).cuda_stream)
        # the kernel wrote through raw pointers: tell torch, or every cache keyed on `_version` goes stale.  (Host side only:
        # a REPLAY of a captured step runs no Python - whoever replays it bumps the versions, see the module docstring)
        bump_versions(*plan.params)

    def _build_plan(self, live, key):
        """Full checks and the pointer table; runs on the first step and whenever an address changed (`zero_grad()` drops the
        gradients and the next backward allocates new ones)."""
        n = len(live)
        device = live[0].device
        ptrs = [[], [], [], [], []]
        staged = []
        for p in live:
            self._check_param(p)
            if p.device != device:
                raise RuntimeError("gridnext_amd.optim: one parameter group spans %s and %s; use one group per device"
                                   % (device, p.device))
            st = self.state[p]
            g = p.grad
            if g.dtype != torch.float32:
                raise TypeError("gridnext_amd.optim: expected a float32 gradient, got %s" % g.dtype)
            if g.device != p.device:
                raise RuntimeError("gridnext_amd.optim: a gradient on %s for a parameter on %s" % (g.device, p.device))
            for name in ('exp_avg', 'exp_avg_sq'):        # (a loaded state keeps the layout it was saved with)
                if st[name].stride() != p.stride() or st[name].dtype != torch.float32 or st[name].device != p.device:
                    with torch.no_grad():
                        st[name] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(st[name])
            if st['step'].dtype != torch.float32 or st['step'].device != p.device:
                st['step'] = st['step'].detach().to(device=p.device, dtype=torch.float32).reshape(())
            if p.numel() > 0 and g.stride() != p.stride():
                with torch.no_grad():
                    g = torch.empty_like(p, memory_format=torch.preserve_format)
                staged.append((p, g))
            for col, t in zip(ptrs, (p, g, st['exp_avg'], st['exp_avg_sq'], st['step'])):
                col.append(t.data_ptr() or None)
        plan = _Plan()
        plan.key = key if not staged else None            # (a staged plan is rebuilt every step: its state may have moved)
        plan.n = n
        plan.arrays = tuple((ctypes.c_void_p * n)(*col) for col in ptrs) + ((ctypes.c_long * n)(*[p.numel() for p in live]),)
        plan.coef = torch.empty(2 * n, dtype=torch.float32, device=device)
        plan.params = tuple(live)
        plan.staged = staged
        plan.device = device
        return plan


class AdamW(Adam):
    """Adam with decoupled weight decay: the same kernel, `p *= 1 - lr * weight_decay` in front of the moment updates."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
