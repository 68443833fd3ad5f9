"""The optimizer side of ``SCFlowRefiner.train_step``: the reference's one training recipe
(configs/refine_models/scflow.py:117-131) on the multi-tensor kernels of csrc/optim.hip.

* ``AdamW``: ``torch.optim.AdamW(amsgrad=False)`` with ``clip_grad_norm_`` folded into the step; one parameter group,
  decay on every tensor.  ``step(grads)`` takes the gradients as a dict (there is no autograd and no ``.grad``), enqueues
  at most three launches and returns the gradient norm as a 0-dim GPU tensor without synchronising.
* ``OneCycle``: torch's ``OneCycleLR(three_phase=False, cycle_momentum=False)`` as a function of the iteration.  mmcv's
  ``OneCycleLrUpdaterHook`` (what ``lr_config=dict(policy='OneCycle')`` selects in the reference's runner) is, to our
  knowledge, a restatement of torch's scheduler; mmcv was not available to check against, so that equivalence is
  UNVERIFIED -- only the one with torch is tested.
* ``build_optimizer``: the three dicts of a reference config file, unchanged.

How the gradient pointers reach the kernel: the parameter and moment pointers are uploaded once, the gradients' once per
step, from a pinned staging tensor (torch's pinned allocator keeps the block alive until the copy has run) and only when a
pointer differs from the previous step's.  The alternative -- ``param_grads=`` views of one flat buffer threaded through
the backward -- would touch every stage of the backward chain for the sake of a 936-byte copy.

The update writes the parameters through raw pointers: their ``_version`` does not move, so the kernel-layout copies
(Winograd and K-packed weights, the GRU's context packs, BatchNorm folds) would go stale.  ``step()`` therefore calls
``model.invalidate_packed()`` when it was given the model; the next forward re-packs every layer (DESIGN.md 4.16 states
the cost).  hipGraphs captured before a step (``GraphedRefiner``) replay the OLD packs and must be re-captured.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import ops

Tensor = torch.Tensor

__all__ = ['AdamW', 'OneCycle', 'build_optimizer']


class OneCycle:
    """``lr(it)`` for the 0-based iteration ``it``: torch.optim.lr_scheduler.OneCycleLR with ``three_phase=False`` and
    ``cycle_momentum=False`` -- from ``max_lr / div_factor`` up to ``max_lr`` over ``pct_start * total_steps - 1`` steps,
    then down to ``max_lr / div_factor / final_div_factor`` at step ``total_steps - 1``."""

    def __init__(self, max_lr: float, total_steps: int, pct_start: float = 0.3, anneal_strategy: str = 'cos',
                 div_factor: float = 25., final_div_factor: float = 1e4) -> None:
        if not isinstance(total_steps, int) or total_steps <= 0:
            raise ValueError(f'Expected positive integer total_steps, but got {total_steps}')
        if not isinstance(pct_start, float) or pct_start < 0 or pct_start > 1:
            raise ValueError(f'Expected float between 0 and 1 pct_start, but got {pct_start}')
        if anneal_strategy not in ('cos', 'linear'):
            raise ValueError(f"anneal_strategy must be one of 'cos' or 'linear', instead got {anneal_strategy}")
        self.max_lr, self.total_steps, self.anneal_strategy = float(max_lr), total_steps, anneal_strategy
        self.initial_lr = self.max_lr / div_factor
        self.min_lr = self.initial_lr / final_div_factor
        self._phases = ((float(pct_start * total_steps) - 1, self.initial_lr, self.max_lr),
                        (total_steps - 1, self.max_lr, self.min_lr))

    def _anneal(self, start: float, end: float, pct: float) -> float:
        if self.anneal_strategy == 'cos':
            return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)
        return (end - start) * pct + start

    def __call__(self, it: int) -> float:
        if it < 0 or it >= self.total_steps:
            raise ValueError(f'Tried to step {it + 1} times. The specified number of total steps is {self.total_steps}')
        start_step = 0.0
        for i, (end_step, start, end) in enumerate(self._phases):
            if it <= end_step or i == len(self._phases) - 1:
                return self._anneal(start, end, (it - start_step) / (end_step - start_step))
            start_step = end_step
        raise AssertionError('unreachable')


class AdamW:
    """``AdamW(named_params, lr, betas, eps, weight_decay, max_norm=None)``: clip + AdamW over ``named_params`` (an iterable
    of (name, fp32 GPU tensor), e.g. ``model.trainable_parameters()``) in csrc/optim.hip.  It owns the moments ``m`` / ``v``
    (views of one flat buffer each), the chunk and pointer tables and the step count.

    ``step(grads)`` -> the total L2 gradient norm (0-dim GPU tensor; ``None`` without ``max_norm``, where the norm pass is
    skipped).  The clipped gradient is not written back: ``grads`` is left as it came (the reference clips ``.grad`` in
    place, and nothing reads it afterwards).  ``lr`` may be changed between steps (``optimizer.lr = schedule(it)``), or
    give ``schedule=`` and it is ``schedule(steps taken so far)`` at every step.

    ``model``: the ``HipModule`` the parameters belong to; its kernel-layout weight copies are dropped after every step."""

    def __init__(self, named_params: Iterable[Tuple[str, Tensor]], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: Optional[float] = None, amsgrad: bool = False,
                 model=None, schedule=None) -> None:
        if amsgrad:
            raise NotImplementedError('AdamW(amsgrad=True) is not implemented (the reference trains with amsgrad=False)')
        self.names: List[str] = []
        self.params: List[Tensor] = []
        for name, p in named_params:
            # any device here (the state dict can be inspected and exchanged without a GPU); step() runs on the GPU only
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f'parameter {name} must be a contiguous float32 tensor')
            self.names.append(name)
            self.params.append(p)
        if not self.params:
            raise ValueError('AdamW: no parameters')
        if len(set(self.names)) != len(self.names):
            raise ValueError('AdamW: duplicate parameter names')
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError(f'AdamW: lr, eps and weight_decay must not be negative, got {lr}, {eps}, {weight_decay}')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'AdamW: betas must lie in [0, 1), got {betas}')
        if max_norm is not None and not max_norm > 0:
            raise ValueError(f'AdamW: max_norm must be positive or None, got {max_norm}')
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.model, self.schedule, self.step_count = model, schedule, 0
        # what the schedule is asked for: training iterations, which is the step count unless an iteration has several cycles.
        # It is not part of torch's optimizer state; a runner that resumes sets it (load_state_dict assumes one cycle).
        self.iteration = 0
        dev = self.device = self.params[0].device
        if any(p.device != dev for p in self.params):
            raise ValueError('AdamW: the parameters live on more than one device')
        sizes = [p.numel() for p in self.params]
        # every tensor's moments start on a 16-byte boundary of the flat buffers, whatever its size
        starts, total = [], 0
        for s in sizes:
            starts.append(total)
            total += (s + 3) // 4 * 4
        self._m_flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v_flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = [self._m_flat[a:a + s].view(p.shape) for a, s, p in zip(starts, sizes, self.params)]
        self.exp_avg_sq = [self._v_flat[a:a + s].view(p.shape) for a, s, p in zip(starts, sizes, self.params)]
        self._chunks = ops.AdamwChunks(sizes, dev)          # built and uploaded once
        self.num_chunks = self._chunks.nchunks
        ptr_table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).to(dev)    # noqa: E731
        self._p_ptrs, self._m_ptrs, self._v_ptrs = ptr_table(self.params), ptr_table(self.exp_avg), ptr_table(self.exp_avg_sq)
        self._g_ptrs = torch.zeros(len(sizes), dtype=torch.int64, device=dev)
        self._p_last = tuple(p.data_ptr() for p in self.params)
        self._g_last: Optional[Tuple[int, ...]] = None
        self._partial = torch.zeros(max(self.num_chunks, 1), dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------------------------------------------ the step
    def _check_grads(self, grads: Dict[str, Tensor]) -> List[Tensor]:
        if not isinstance(grads, dict):
            raise TypeError(f'AdamW.step: grads must be a dict of name -> gradient, got {type(grads).__name__}')
        if len(grads) != len(self.names) or any(n not in grads for n in self.names):
            missing = [n for n in self.names if n not in grads]
            extra = [n for n in grads if n not in set(self.names)]
            raise KeyError(f'AdamW.step: the gradients do not match the parameters: missing {missing[:4]}, unexpected {extra[:4]}')
        out = []
        for name, p in zip(self.names, self.params):
            g = grads[name]
            if not isinstance(g, torch.Tensor) or g.dtype != torch.float32:
                raise TypeError(f'AdamW.step: gradient {name} must be a float32 tensor')
            if g.device != p.device:
                raise ValueError(f'AdamW.step: gradient {name} lives on {g.device}, its parameter on {p.device}')
            if g.shape != p.shape:
                raise ValueError(f'AdamW.step: gradient {name} has shape {tuple(g.shape)}, its parameter {tuple(p.shape)}')
            if not g.is_contiguous():
                raise ValueError(f'AdamW.step: gradient {name} is not contiguous')
            out.append(g)
        return out

    def step(self, grads: Dict[str, Tensor], end_of_iteration: bool = True) -> Optional[Tensor]:
        """``end_of_iteration=False``: a step between the cycles of one training iteration (``train_cfg['cycles'] > 1``);
        the schedule's iteration count does not advance, as the reference's runner advances it once per iteration."""
        ops._dev(self.params[0], f'parameter {self.names[0]}')       # on the GPU, or raise: there is no CPU fallback
        gs = self._check_grads(grads)
        if self.schedule is not None:
            self.lr = float(self.schedule(self.iteration))
        if end_of_iteration:
            self.iteration += 1
        where = tuple(p.data_ptr() for p in self.params)
        if where != self._p_last:               # the storage moved under the same Parameter objects (model.to(), .data = ...)
            if any(p.device != self.device for p in self.params):
                raise ValueError(f'AdamW.step: the parameters left {self.device}; build a new optimizer and load the state')
            self._p_ptrs.copy_(torch.tensor(where, dtype=torch.int64))
            self._p_last = where
        ptrs = tuple(g.data_ptr() for g in gs)
        if ptrs != self._g_last:
            staged = torch.empty(len(ptrs), dtype=torch.int64, pin_memory=True)
            staged.copy_(torch.tensor(ptrs, dtype=torch.int64))
            self._g_ptrs.copy_(staged, non_blocking=True)
            self._g_last = ptrs
        norm = None
        if self.max_norm is not None:
            norm = ops.grad_sqnorm(self._chunks, self._g_ptrs, self._partial,
                                   torch.empty((), dtype=torch.float32, device=self.device))
        self.step_count += 1
        ops.adamw_step(self._chunks, self._p_ptrs, self._g_ptrs, self._m_ptrs, self._v_ptrs, norm,
                       self.max_norm or 0.0, self.lr, self.weight_decay, self.betas[0], self.betas[1], self.eps,
                       self.step_count)
        if self.model is not None:
            self.model.invalidate_packed()
        return norm

    # ----------------------------------------------------------------------------------------------------- the state
    def state_dict(self) -> dict:
        """torch.optim.AdamW's layout: ``state[i] = dict(step, exp_avg, exp_avg_sq)`` for parameter i (absent before the
        first step, as in torch) and one entry of ``param_groups``; a ``torch.optim.AdamW`` over the same parameters in
        the same order loads it, and ``load_state_dict`` takes torch's.  ``max_norm`` is not part of it (it is the
        runner's ``grad_clip`` in the reference, not the optimizer's)."""
        state = {}
        if self.step_count:
            for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq)):
                state[i] = dict(step=torch.tensor(float(self.step_count)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        group = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, amsgrad=False,
                     maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                     decoupled_weight_decay=True, params=list(range(len(self.params))))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd: dict) -> None:
        groups = sd['param_groups']
        if len(groups) != 1 or list(groups[0]['params']) != list(range(len(self.params))):
            raise ValueError(f'AdamW.load_state_dict: expected one parameter group over {len(self.params)} parameters')
        g = groups[0]
        if g.get('amsgrad', False) or g.get('maximize', False):
            raise NotImplementedError('AdamW.load_state_dict: amsgrad / maximize are not implemented')
        state = {int(k): v for k, v in sd['state'].items()}
        if state and sorted(state) != list(range(len(self.params))):
            raise ValueError('AdamW.load_state_dict: state for some parameters only')
        steps = {int(float(s['step'])) for s in state.values()}
        if len(steps) > 1:
            raise ValueError(f'AdamW.load_state_dict: the parameters are at different steps {sorted(steps)}')
        for i, s in state.items():
            for name in ('exp_avg', 'exp_avg_sq'):
                if tuple(s[name].shape) != tuple(self.params[i].shape):
                    raise ValueError(f'AdamW.load_state_dict: state[{i}][{name!r}] has shape {tuple(s[name].shape)}, '
                                     f'parameter {self.names[i]} {tuple(self.params[i].shape)}')
        self.lr, self.eps, self.weight_decay = float(g['lr']), float(g['eps']), float(g['weight_decay'])
        self.betas = (float(g['betas'][0]), float(g['betas'][1]))
        self.step_count = self.iteration = steps.pop() if steps else 0
        if not state:
            self._m_flat.zero_()
            self._v_flat.zero_()
        for i, s in state.items():
            self.exp_avg[i].copy_(s['exp_avg'])
            self.exp_avg_sq[i].copy_(s['exp_avg_sq'])


def build_optimizer(model, optimizer_cfg: dict, optimizer_config: Optional[dict] = None, lr_config: Optional[dict] = None,
                    network: bool = False) -> AdamW:
    """the ``optimizer``, ``optimizer_config`` and ``lr_config`` dicts of a reference config file -> ``AdamW`` over
    ``model.trainable_parameters()``, clipping at ``optimizer_config['grad_clip']['max_norm']`` and following the
    ``OneCycle`` schedule of ``lr_config``.  Any other optimizer type or policy is refused by name.
    ``network=True``: over ``model.network_parameters()``, for ``SCFlowRefiner.train_step_network``."""
    cfg = dict(optimizer_cfg)
    kind = cfg.pop('type', None)
    if kind != 'AdamW':
        raise NotImplementedError(f"optimizer type {kind!r} is not implemented: only 'AdamW' is")
    unknown = set(cfg) - {'lr', 'betas', 'eps', 'weight_decay', 'amsgrad'}
    if unknown:
        raise NotImplementedError(f'AdamW options {sorted(unknown)} are not implemented')
    max_norm = None
    clip = (optimizer_config or {}).get('grad_clip')
    if clip is not None:
        if clip.get('norm_type', 2) not in (2, 2.0):
            raise NotImplementedError(f"grad_clip norm_type {clip['norm_type']!r} is not implemented: only the L2 norm is")
        unknown = set(clip) - {'max_norm', 'norm_type'}
        if unknown:
            raise NotImplementedError(f'grad_clip options {sorted(unknown)} are not implemented')
        max_norm = clip['max_norm']
    unknown = set(optimizer_config or {}) - {'grad_clip'}
    if unknown:
        raise NotImplementedError(f'optimizer_config options {sorted(unknown)} are not implemented')
    schedule = None
    if lr_config is not None:
        lr_cfg = dict(lr_config)
        policy = lr_cfg.pop('policy', None)
        if policy != 'OneCycle':
            raise NotImplementedError(f"lr_config policy {policy!r} is not implemented: only 'OneCycle' is")
        unknown = set(lr_cfg) - {'max_lr', 'total_steps', 'pct_start', 'anneal_strategy', 'div_factor', 'final_div_factor'}
        if unknown:
            raise NotImplementedError(f'OneCycle options {sorted(unknown)} are not implemented')
        schedule = OneCycle(**lr_cfg)
    params = model.network_parameters() if network else model.trainable_parameters()
    return AdamW(params, max_norm=max_norm, model=model, schedule=schedule, **cfg)
