"""CPU: the optimizer step of csrc/optim.hip (gradient norm, clip coefficient, AdamW update) restated in float64 with a
per-element bound for any fp32 evaluation in the kernel's operation order (the `EV` running-error arithmetic of
tests/test_stream_ops_host.py), the tensor lists tests/test_gpu_optim.py feeds the kernels, the proof that the bounds are
neither unreachable (torch's fp32 clip_grad_norm_ + AdamW on the CPU stays inside) nor vacuous (seven planted defects fall
outside, each at its own launch), the OneCycle schedule against torch's, the state-dict layout, the chunk-table builder, the
C-ABI wiring and the refusals.

The norm.  The kernel adds g^2 in a fixed order; an element passes through at most `norm_depth(nchunks)` additions:
per lane CHUNK / THREADS vector elements plus one head and one tail element, log2(64) lane steps, THREADS / 64 - 1 wave
steps, and once more the same three stages in the one-block finish over ceil(nchunks / THREADS) partials per lane.  All
terms are nonnegative, so the computed sum of squares is within gamma_{d+1} of the exact one, relatively (the +1: the
square's own rounding); the root halves that (bounded here by the whole) and rounds once.

The update.  Constants derived on the host in float64 (1 - lr wd, 1 - beta, lr / bc1, sqrt(bc2)) are rounded to fp32 once:
relative U each.  Every operation of the kernel is replayed once on `EV`s.  What that comes to is asserted
(`test_update_bound_is_a_handful_of_u`): the bound on p stays below HANDFUL U (|p| + step_size (|m| + |g'|) / denom), with
HANDFUL = 2 (d + 1) + 24 -- the norm's gamma_{d+1} reaches the update once through m and once through sqrt(v) (twice in
g'^2, halved by the root), and 24 U cover the roundings of the straight-line part (counted in `adamw_ref`).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import ops, optim
from test_stream_ops_host import EV, U, f64, measured, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'scflow_hip.h')).read()
SRC = open(os.path.join(ROOT, 'scflow_amd', 'csrc', 'optim.hip')).read()
SYMBOLS = ['scf_adamw_chunks', 'scf_grad_sqnorm', 'scf_adamw_step']

CHUNK, THREADS = ops.ADAMW_CHUNK, ops.ADAMW_NORM_THREADS
f32 = np.float32

# the tensor list of the kernel tests: below one vector, one wave, around one chunk, several chunks with a ragged end
SIZES = [1, 2, 3, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
TABLE_SIZES = [0, 1, 2, 3, 63, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]

# the reference's recipe (configs/refine_models/scflow.py:117-131), copied as data
REF_OPTIMIZER = dict(type='AdamW', lr=0.0004, betas=(0.9, 0.999), eps=1e-08, weight_decay=0.0001, amsgrad=False)
REF_OPTIMIZER_CONFIG = dict(grad_clip=dict(max_norm=10.))
REF_LR_CONFIG = dict(policy='OneCycle', max_lr=0.0004, total_steps=100100, pct_start=0.05, anneal_strategy='linear')

HP_REF = dict(lr=4e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-4, max_norm=10.)
# lr wd = 4e-8 of the reference is below U: one step of its decay cannot be told from none.  The defects are planted where
# every term of the update is far above the rounding.
HP_LOUD = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, wd=0.1, max_norm=10.)
LRS = [1.0, 0.5, 2.0, 0.25, 1.5]               # multiplies hp['lr'] at steps 1..5: a changing rate
SCALES = [1.0, 0.01, 3.0, 0.003, 0.5]          # gradient scale at steps 1..5: |g| ~ 157 s, clipping active / idle / ...


def chunks_of(sizes):
    return sum(-(-s // CHUNK) for s in sizes)


def gamma(n):
    return n * U / (1 - n * U)


def norm_depth(nchunks):
    per_block = lambda terms: terms + int(math.log2(64)) + (THREADS // 64 - 1)      # noqa: E731
    return per_block(CHUNK // THREADS + 2) + per_block(-(-nchunks // THREADS))


def norm_ref(grads, nchunks=None):
    """float64 L2 norm of the list and the bound on |fp32 norm in the kernel's order - it|, as an EV"""
    s = sum(float((f64(g) ** 2).sum()) for g in grads)
    d = norm_depth(chunks_of([np.asarray(g).size for g in grads]) if nchunks is None else nchunks)
    return EV(s, gamma(d + 1) * s).sqrt()


def cst(x):
    """a float64 constant rounded to fp32 once"""
    return EV(x, U * abs(x))


def coef_ref(norm, max_norm):
    """c = min(max_norm / (norm + 1e-6), 1): exactly 1 where the quotient is above 1 beyond its own error"""
    if norm is None:
        return EV(1.0)
    x = cst(max_norm) / (norm + cst(1e-6))
    if x.v - x.e > 1:
        return EV(1.0)
    return EV(min(float(x.v), 1.0), x.e)


def adamw_ref(p, g, m, v, c, hp, t, lr):
    """one step in float64 on fp32 state (p, g, m, v as stored): EVs of the new p, m, v, and the magnitude the bound on p is
    measured against.  Roundings of the straight-line part, relative to their own terms: g' 1, decay 2, m 3 (+ g''s),
    v 3 (+ twice g''s), root 1, quotient by sqrt(bc2) 2, + eps 2, m / denom 1, times step_size 2, the last subtraction 1."""
    b1, b2 = hp['betas']
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p, g, m, v = EV(f64(p)), EV(f64(g)), EV(f64(m)), EV(f64(v))
    gp = g * c
    p1 = p * cst(1 - lr * hp['wd'])
    m1 = m + (gp - m) * cst(1 - b1)
    v1 = v * cst(b2) + cst(1 - b2) * (gp * gp)
    denom = v1.sqrt() / cst(math.sqrt(bc2)) + cst(hp['eps'])
    q = cst(lr / bc1) * (m1 / denom)
    p2 = p1 - q
    with np.errstate(all='ignore'):
        size = np.abs(p.v) + (lr / bc1) * (np.abs(m.v) + np.abs(gp.v)) / denom.v
    return dict(p=p2, m=m1, v=v1, size=size)


def adamw_fp32(ps, gs, ms, vs, hp, t, lr, defect=None, prev_lr=None):
    """numpy fp32 in the kernel's operation order -> (norm, [p], [m], [v]); `defect` plants one of DEFECTS"""
    b1, b2 = hp['betas']
    if defect == 'betas_swapped':
        b1, b2 = b2, b1
    if defect == 'previous_lr':
        lr = prev_lr
    bc1, bc2 = (1.0, 1.0) if defect == 'no_bias_correction' else (1 - b1 ** t, 1 - b2 ** t)
    norm, c = None, f32(1)
    if hp['max_norm'] is not None:
        over = gs[:1] if defect == 'norm_of_one_tensor' else gs
        norm = np.sqrt(np.sum([np.sum(g * g, dtype=f32) for g in over], dtype=f32))
        x = f32(hp['max_norm']) / (norm + f32(1e-6))
        c = f32(1) if x > 1 else x
    decay, omb1, fb2, omb2 = f32(1 - lr * hp['wd']), f32(1 - b1), f32(b2), f32(1 - b2)
    step, bc2s, eps = f32(lr / bc1), f32(math.sqrt(bc2)), f32(hp['eps'])
    out = ([], [], [])
    for p, g, m, v in zip(ps, gs, ms, vs):
        gc = g * c
        gm = g if defect == 'moments_of_unclipped' else gc
        if defect == 'l2_decay':
            gm = gm + f32(hp['wd']) * p
            p1 = p
        else:
            p1 = p * decay
        m1 = m + (gm - m) * omb1
        v1 = v * fb2 + omb2 * (gm * gm)
        denom = np.sqrt(v1 / (bc2s * bc2s) + eps) if defect == 'eps_under_root' else np.sqrt(v1) / bc2s + eps
        out[0].append(p1 - step * (m1 / denom))
        out[1].append(m1)
        out[2].append(v1)
    return (norm,) + out


DEFECTS = ['l2_decay', 'no_bias_correction', 'eps_under_root', 'moments_of_unclipped', 'betas_swapped', 'previous_lr',
           'norm_of_one_tensor']


def make_state(seed=0, sizes=SIZES):
    rng = np.random.RandomState(seed)
    ps = [(rng.randn(s) * 0.1).astype(f32) for s in sizes]
    return ps, [np.zeros(s, f32) for s in sizes], [np.zeros(s, f32) for s in sizes]


def make_grads(step, scale, seed=0, sizes=SIZES):
    rng = np.random.RandomState(1000 * seed + step)
    return [(rng.randn(s) * scale).astype(f32) for s in sizes]


def step_ratios(before, grads, after, norm, hp, t, lr, given_norm=None):
    """worst |after - float64 step from `before`| / bound over p, m, v (and the norm); `given_norm`: an fp32 norm taken as
    given (exact), the way the update kernel takes the norm pass's"""
    ref_norm = None if hp['max_norm'] is None else norm_ref(grads)
    c = coef_ref(EV(float(given_norm)) if given_norm is not None else ref_norm, hp['max_norm']) if hp['max_norm'] is not None \
        else coef_ref(None, None)
    out = dict(p=0.0, m=0.0, v=0.0)
    for i in range(len(grads)):
        ref = adamw_ref(before[0][i], grads[i], before[1][i], before[2][i], c, hp, t, lr)
        for k, name in enumerate('pmv'):
            out[name] = max(out[name], worst_ratio(after[k][i], ref[name].v, ref[name].e))
    if norm is not None and ref_norm is not None:
        out['norm'] = worst_ratio(norm, ref_norm.v, ref_norm.e)
    return out


# ------------------------------------------------------------------------------------------------------------- bounds
def test_norm_depth_is_counted_from_the_kernel_constants():
    assert re.search(rf'#define SCF_ADAMW_CHUNK {CHUNK}\b', HEADER) and re.search(rf'#define SCF_ADAMW_NORM_THREADS {THREADS}\b', HEADER)
    assert re.search(r'#define ADAMW_THREADS 256\b', SRC) and THREADS == 256 and CHUNK & (CHUNK - 1) == 0
    assert norm_depth(1) == (CHUNK // THREADS + 2 + 6 + 3) + (1 + 6 + 3)
    assert norm_depth(1819) == (CHUNK // THREADS + 2 + 6 + 3) + (8 + 6 + 3)     # the model's 117 tensors: 1,819 chunks
    assert 'atomic' not in re.sub(r'//.*', '', SRC)                            # fixed order: no atomics, no done counter


@pytest.mark.parametrize('hp', [HP_REF, HP_LOUD], ids=['reference', 'loud'])
def test_update_bound_is_a_handful_of_u(hp):
    ps, ms, vs = make_state()
    handful = 2 * (norm_depth(chunks_of(SIZES)) + 1) + 24
    worst = 0.0
    for t in range(1, 6):
        gs, lr = make_grads(t, SCALES[t - 1]), hp['lr'] * LRS[t - 1]
        c = coef_ref(norm_ref(gs), hp['max_norm'])
        for i in range(len(ps)):
            ref = adamw_ref(ps[i], gs[i], ms[i], vs[i], c, hp, t, lr)
            worst = max(worst, float((ref['p'].e / (U * ref['size'])).max()))
        _, ps, ms, vs = adamw_fp32(ps, gs, ms, vs, hp, t, lr)
    measured(f'bound on p / (U (|p| + step (|m| + |g\'|) / denom)), handful = {handful}', worst)
    assert worst <= handful


@pytest.mark.parametrize('hp', [HP_REF, HP_LOUD, dict(HP_REF, max_norm=None), dict(HP_LOUD, wd=0.0)],
                         ids=['reference', 'loud', 'no_clip', 'no_decay'])
def test_kernel_order_fp32_falls_inside(hp):
    ps, ms, vs = make_state()
    active = []
    for t in range(1, 6):
        gs, lr = make_grads(t, SCALES[t - 1]), hp['lr'] * LRS[t - 1]
        norm, p2, m2, v2 = adamw_fp32(ps, gs, ms, vs, hp, t, lr)
        r = step_ratios((ps, ms, vs), gs, (p2, m2, v2), norm, hp, t, lr)
        assert max(r.values()) <= 1.0, (t, r)
        r = step_ratios((ps, ms, vs), gs, (p2, m2, v2), None, hp, t, lr, given_norm=norm)
        assert max(r.values()) <= 1.0, (t, r)
        active.append(norm is not None and norm > hp['max_norm'])
        ps, ms, vs = p2, m2, v2
    if hp['max_norm'] is not None:
        assert any(active) and not all(active)       # clipping active in some steps, idle in others


@pytest.mark.parametrize('hp', [HP_REF, HP_LOUD], ids=['reference', 'loud'])
def test_torch_fp32_clip_and_adamw_fall_inside(hp):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=False) on the CPU, five steps, every step from torch's own
    previous state"""
    ps, ms, vs = make_state()
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.AdamW(params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['wd'], foreach=False)
    worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0)
    for t in range(1, 6):
        gs, lr = make_grads(t, SCALES[t - 1]), hp['lr'] * LRS[t - 1]
        opt.param_groups[0]['lr'] = lr
        for q, g in zip(params, gs):
            q.grad = torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_(params, hp['max_norm'], foreach=False)
        opt.step()
        after = ([q.detach().numpy().copy() for q in params], [opt.state[q]['exp_avg'].numpy().copy() for q in params],
                 [opt.state[q]['exp_avg_sq'].numpy().copy() for q in params])
        r = step_ratios((ps, ms, vs), gs, after, float(norm), hp, t, lr)
        for k in r:
            worst[k] = max(worst[k], r[k])
        ps, ms, vs = after
    for k, x in worst.items():
        measured(f'torch fp32 on the CPU, {k}: error / bound', x)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_defects_fall_outside(defect):
    hp = HP_LOUD
    ps, ms, vs = make_state()
    outside = []
    prev_lr = None
    for t in range(1, 4):
        gs, lr = make_grads(t, SCALES[t - 1]), hp['lr'] * LRS[t - 1]
        good = adamw_fp32(ps, gs, ms, vs, hp, t, lr)
        if prev_lr is not None or defect != 'previous_lr':
            bad = adamw_fp32(ps, gs, ms, vs, hp, t, lr, defect=defect, prev_lr=prev_lr)
            r = step_ratios((ps, ms, vs), gs, bad[1:], bad[0], hp, t, lr)
            outside.append(max(r.values()))
        assert max(step_ratios((ps, ms, vs), gs, good[1:], good[0], hp, t, lr).values()) <= 1.0
        ps, ms, vs = good[1:]
        prev_lr = lr
    measured(f'defect {defect}: worst error / bound per step', max(outside))
    # each at its own launch: a defect of the clip path shows in the steps that clip (1 and 3), the others in every step
    clip_only = defect in ('moments_of_unclipped', 'norm_of_one_tensor')
    shown = [x for x, s in zip(outside, SCALES if defect != 'previous_lr' else SCALES[1:]) if not clip_only or 157 * s > hp['max_norm']]
    assert shown and min(shown) > 10.0, outside


# -------------------------------------------------------------------------------------------------- schedule and state
@pytest.mark.parametrize('strategy', ['linear', 'cos'])
@pytest.mark.parametrize('total', [50, 100100])
def test_one_cycle_equals_torch(strategy, total):
    import warnings
    from torch.optim.lr_scheduler import OneCycleLR
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    sched = OneCycleLR(opt, max_lr=4e-4, total_steps=total, pct_start=0.05, anneal_strategy=strategy, cycle_momentum=False)
    ours = optim.OneCycle(4e-4, total, pct_start=0.05, anneal_strategy=strategy)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for it in range(total):
            want, got = opt.param_groups[0]['lr'], ours(it)
            assert got == want or abs(got - want) <= math.ulp(want), (it, got, want)
            if it < total - 1:
                opt.step()
                sched.step()
    assert ours(0) == pytest.approx(4e-4 / 25, rel=1e-12) and ours(total - 1) == pytest.approx(4e-4 / 25 / 1e4, rel=1e-9)
    with pytest.raises(ValueError):
        ours(total)
    with pytest.raises(ValueError):
        optim.OneCycle(4e-4, total, anneal_strategy='exp')


def test_chunk_table_covers_every_element_once():
    table = ops.adamw_chunk_table(TABLE_SIZES)
    rows = ops.adamw_chunk_rows(table)
    assert len(rows) == chunks_of(TABLE_SIZES) == table.shape[0]
    seen = [np.zeros(s, dtype=np.int64) for s in TABLE_SIZES]
    for tensor, off, length in rows:
        assert 1 <= length <= CHUNK and off % CHUNK == 0 and off + length <= TABLE_SIZES[tensor]
        seen[tensor][off:off + length] += 1
    assert all((s == 1).all() for s in seen)
    assert rows == sorted(rows)                                  # tensor by tensor, front to back
    assert ops.adamw_chunk_table([]).shape == (0, 2) and ops.adamw_chunk_table([0, 0]).shape == (0, 2)
    with pytest.raises(ValueError):
        ops.adamw_chunk_table([3, -1])
    # the C entry refuses a table that is too small instead of writing past it
    import ctypes as C
    from scflow_amd import _lib
    lib = _lib.load()
    sizes = (C.c_int64 * 2)(CHUNK + 1, 5)
    out = (_lib.AdamwChunk * 2)()
    assert lib.scf_adamw_chunks(sizes, 2, None, 0) == 3
    assert lib.scf_adamw_chunks(sizes, 2, out, 2) < 0
    assert lib.scf_adamw_chunks(None, 2, None, 0) < 0


def test_symbols_are_declared_exported_and_bound():
    from scflow_amd import _lib
    from scflow_amd.csrc import build
    assert 'optim.hip' in build.SOURCES
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf'\b{name}\(', HEADER), f'{name} is not declared in scflow_hip.h'
        assert re.search(rf'extern "C" \w+ {name}\(', SRC), f'{name} is not defined in optim.hip'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        proto = re.search(rf'^int(?:64_t)? {name}\(([^;]*)\);', HEADER, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(proto.split(',')), f'{name}: argument count'
    import ctypes as C
    assert C.sizeof(_lib.AdamwChunk) == 16
    assert 'the presence of scf_adamw_step marks' in re.sub(r'\s*\n \* ', ' ', HEADER)
    assert re.search(r'#define SCF_VERSION \(SCF_ABI_MAJOR \* 100 \+ 3\)', HEADER)          # no bump
    assert {'AdamW', 'OneCycle', 'build_optimizer'} <= set(dir(scflow_amd))


# ------------------------------------------------------------------------------------------------------------ refusals
def _frozen_model(**over):
    cfg = scflow_amd.scflow_model_cfg(iters=2)
    cfg.update(dict(freeze_encoder=True, freeze_bn=True), **over)
    return scflow_amd.build_refiner(cfg)


def test_trainable_parameters_are_the_decoder_and_the_context_encoder():
    m = _frozen_model()
    named = m.trainable_parameters()
    assert len(named) == 117 and sum(p.numel() for _, p in named) == 7111358
    assert all(n.startswith(('decoder.', 'context.')) for n, _ in named)
    order = [n for n, _ in m.named_parameters() if n.startswith(('decoder.', 'context.'))]
    assert [n for n, _ in named] == order
    buffers = {id(b) for b in m.buffers()}
    assert all(isinstance(p, torch.nn.Parameter) and id(p) not in buffers for _, p in named)
    assert m.freeze_encoder is True and m.freeze_bn is True
    m2 = scflow_amd.build_refiner(scflow_amd.scflow_model_cfg(iters=2))
    assert m2.freeze_encoder is False and m2.freeze_bn is False


def test_wrappers_refuse():
    from scflow_amd._lib import ScflowHipError
    cpu = torch.zeros(4)
    with pytest.raises(NotImplementedError, match='amsgrad'):
        optim.AdamW([('w', cpu)], amsgrad=True)
    opt = optim.AdamW([('w', cpu), ('b', torch.zeros(2, 3))])
    with pytest.raises(ScflowHipError):                          # CPU parameters: the step is HIP only, no fallback
        opt.step({'w': cpu, 'b': torch.zeros(2, 3)})
    with pytest.raises(TypeError):                               # what step() checks next, on the CPU as well
        opt._check_grads([cpu, cpu])
    with pytest.raises(KeyError):
        opt._check_grads({'w': cpu})
    with pytest.raises(KeyError):
        opt._check_grads({'w': cpu, 'c': torch.zeros(2, 3)})
    with pytest.raises(ValueError, match='shape'):
        opt._check_grads({'w': cpu, 'b': torch.zeros(3, 2)})
    with pytest.raises(TypeError, match='float32'):
        opt._check_grads({'w': cpu.double(), 'b': torch.zeros(2, 3)})
    with pytest.raises(ValueError, match='contiguous'):
        opt._check_grads({'w': cpu, 'b': torch.zeros(3, 2).t()})
    with pytest.raises(ValueError):
        optim.AdamW([])
    with pytest.raises(ValueError):
        optim.AdamW([('w', cpu), ('w', cpu)])
    with pytest.raises(ValueError):
        optim.AdamW([('w', cpu.double())])
    with pytest.raises(ValueError):
        optim.AdamW([('w', cpu)], max_norm=0.)
    with pytest.raises(ScflowHipError):
        ops.grad_sqnorm(ops.AdamwChunks([4], 'cpu'), torch.zeros(1, dtype=torch.int64), cpu, cpu)
    with pytest.raises(ScflowHipError):
        ops.adamw_step(ops.AdamwChunks([4], 'cpu'), *[torch.zeros(1, dtype=torch.int64)] * 4, None, 0., 1e-3, 0., 0.9, 0.999, 1e-8, 1)
    with pytest.raises(ScflowHipError):
        ops.grad_sqnorm(torch.zeros((1, 2), dtype=torch.int64), torch.zeros(1, dtype=torch.int64), cpu, cpu)


def test_build_optimizer_refuses_by_name():
    m = _frozen_model()
    for bad, kw in ((dict(REF_OPTIMIZER, type='SGD'), {}), (REF_OPTIMIZER, dict(lr_config=dict(REF_LR_CONFIG, policy='step'))),
                    (dict(REF_OPTIMIZER, amsgrad=True), {}), (dict(REF_OPTIMIZER, fused=True), {}),
                    (REF_OPTIMIZER, dict(optimizer_config=dict(grad_clip=dict(max_norm=1., norm_type=1))))):
        with pytest.raises(NotImplementedError) as e:
            optim.build_optimizer(m, bad, **kw)
        assert any(w in str(e.value) for w in ('SGD', 'step', 'amsgrad', 'fused', 'norm_type'))
    # the three dicts of the reference's scflow.py, unchanged
    opt = optim.build_optimizer(m, REF_OPTIMIZER, REF_OPTIMIZER_CONFIG, REF_LR_CONFIG)
    assert isinstance(opt, optim.AdamW) and len(opt.params) == 117 and opt.model is m and opt.max_norm == 10.
    assert all(a is b for a, (_, b) in zip(opt.params, m.trainable_parameters()))
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (4e-4, (0.9, 0.999), 1e-8, 1e-4)
    assert opt.num_chunks == chunks_of([p.numel() for p in opt.params]) == 1819 and opt.step_count == 0 and opt.iteration == 0
    sched = opt.schedule
    assert isinstance(sched, optim.OneCycle) and sched.total_steps == 100100 and sched.anneal_strategy == 'linear'
    assert sched(0) == 4e-4 / 25 and sched(5004) == 4e-4
    plain = optim.build_optimizer(m, REF_OPTIMIZER)
    assert plain.max_norm is None and plain.schedule is None


def test_state_dict_round_trips_through_torch():
    """ours -> torch.optim.AdamW -> ours over the same parameters in the same order (the layout of the reference's checkpoints)"""
    rng = np.random.RandomState(3)
    shapes = [(5,), (2, 3), (1,), (4, 1, 3, 3)]
    params = [torch.nn.Parameter(torch.from_numpy(rng.randn(*s).astype(f32))) for s in shapes]
    ours = optim.AdamW([(f'p{i}', p) for i, p in enumerate(params)], lr=3e-4, betas=(0.85, 0.98), eps=1e-7, weight_decay=0.02)
    assert ours.state_dict()['state'] == {}                      # torch's: no state before the first step
    torch.optim.AdamW(params).load_state_dict(ours.state_dict())
    for m, v in zip(ours.exp_avg, ours.exp_avg_sq):
        m.copy_(torch.from_numpy(rng.randn(*m.shape).astype(f32)))
        v.copy_(torch.from_numpy(rng.rand(*v.shape).astype(f32)))
    ours.step_count = ours.iteration = 7
    sd = ours.state_dict()
    assert sorted(sd) == ['param_groups', 'state'] and sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step']
    th = torch.optim.AdamW(params)
    th.load_state_dict(sd)
    g = th.param_groups[0]
    assert (g['lr'], tuple(g['betas']), g['eps'], g['weight_decay'], g['amsgrad']) == (3e-4, (0.85, 0.98), 1e-7, 0.02, False)
    assert all(float(th.state[p]['step']) == 7 and torch.equal(th.state[p]['exp_avg'], m)
               for p, m in zip(params, ours.exp_avg))
    back = optim.AdamW([(f'p{i}', p) for i, p in enumerate(params)])
    back.load_state_dict(th.state_dict())
    assert back.step_count == 7 and back.iteration == 7
    assert (back.lr, back.betas, back.eps, back.weight_decay) == (3e-4, (0.85, 0.98), 1e-7, 0.02)
    for a, b in zip(back.exp_avg + back.exp_avg_sq, ours.exp_avg + ours.exp_avg_sq):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        optim.AdamW([('p0', params[0])]).load_state_dict(sd)
    bad = th.state_dict()
    bad['param_groups'][0]['amsgrad'] = True
    with pytest.raises(NotImplementedError):
        back.load_state_dict(bad)


def test_train_step_refuses():
    opt = optim.AdamW([('w', torch.zeros(3))])                    # another model's: never reached past the checks
    with pytest.raises(NotImplementedError, match='feature-encoder and correlation-build backward'):
        _frozen_model(freeze_encoder=False).train_step(None, opt, data={})
    with pytest.raises(NotImplementedError, match='BatchNorm on batch statistics'):
        _frozen_model(freeze_bn=False).train_step(None, opt, data={})
    m = _frozen_model()
    with pytest.raises(TypeError, match='scflow_amd.optim.AdamW'):
        m.train_step(None, torch.optim.AdamW(m.parameters()), data={})
    with pytest.raises(ValueError, match='trainable_parameters'):
        m.train_step(None, opt, data={})
    with pytest.raises(NotImplementedError, match='train_step and the backward'):
        m.forward({}, return_loss=True)                           # unchanged
    assert not hasattr(scflow_amd.RAFTRefinerFlow, 'train_step') and not hasattr(scflow_amd.RAFTRefinerFlowMask, 'train_step')
