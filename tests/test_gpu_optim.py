"""GPU: csrc/optim.hip (scf_grad_sqnorm, scf_adamw_step) and scflow_amd.optim.AdamW against the float64 restatement and the
bounds of tests/test_optim_host.py, against torch's fp32 optimizer on the CPU, and at the regimes where an optimizer goes
wrong quietly.  The norm's bits depend on the chunking and on each gradient's address modulo 16 (the order of the
additions does): reproducibility is claimed, and asserted, for the same pointers only -- NOT across arrangements."""
import numpy as np
import pytest
import torch

from scflow_amd import ops, optim
from scflow_amd._lib import ScflowHipError
import test_optim_host as H
from test_optim_host import CHUNK, HP_LOUD, HP_REF, LRS, SCALES, SIZES, U, f32
from test_stream_ops_host import EV, measured, same_bits, worst_ratio

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 12345.0

# the list of tests/test_optim_host.py plus two views into larger buffers at offsets that are 4-byte aligned only, the
# second with guard values on both sides; (size, offset of the parameter view, offset of the gradient view)
VIEWS = [(1001, 1, 2), (CHUNK + 2, 3, 3)]
ALL_SIZES = SIZES + [s for s, _, _ in VIEWS]


def view_in(buf_size, off, size, fill):
    buf = torch.full((buf_size,), fill, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + size]
    assert v.data_ptr() % 16 == 4 * off % 16 != 0
    return buf, v


class Case:
    """parameters (the last two are misaligned views), an AdamW over them, and per-step gradients of the same layout"""

    def __init__(self, hp, seed=0):
        ps, _, _ = H.make_state(seed, ALL_SIZES)
        self.params, self.p_bufs = [torch.from_numpy(p).to(DEV) for p in ps[:len(SIZES)]], []
        for (size, off, _), p in zip(VIEWS, ps[len(SIZES):]):
            buf, v = view_in(size + 8, off, size, GUARD)
            v.copy_(torch.from_numpy(p))
            self.p_bufs.append((buf, off, size))
            self.params.append(v)
        self.names = [f't{i}' for i in range(len(self.params))]
        self.hp = hp
        self.opt = optim.AdamW(list(zip(self.names, self.params)), lr=hp['lr'], betas=hp['betas'], eps=hp['eps'],
                               weight_decay=hp['wd'], max_norm=hp['max_norm'])

    def grads(self, step, scale, seed=0, edit=None):
        gs = H.make_grads(step, scale, seed, ALL_SIZES)
        if edit is not None:
            edit(gs)
        out, bufs = [torch.from_numpy(g).to(DEV) for g in gs[:len(SIZES)]], []
        for (size, _, off), g in zip(VIEWS, gs[len(SIZES):]):
            buf, v = view_in(size + 8, off, size, GUARD)
            v.copy_(torch.from_numpy(g))
            bufs.append((buf, off, size))
            out.append(v)
        return gs, dict(zip(self.names, out)), bufs

    def state(self):
        cpu = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]      # noqa: E731
        return cpu(self.params), cpu(self.opt.exp_avg), cpu(self.opt.exp_avg_sq)

    def guards_intact(self, bufs):
        for buf, off, size in bufs:
            b = buf.cpu()
            if not (bool((b[:off] == GUARD).all()) and bool((b[off + size:] == GUARD).all())):
                return False
        return True


def torch_step(before, gs, hp, t, lr):
    """one step of torch's fp32 clip_grad_norm_ + AdamW(foreach=False) on the CPU from the state `before`"""
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in before[0]]
    opt = torch.optim.AdamW(params, lr=lr, betas=hp['betas'], eps=hp['eps'], weight_decay=hp['wd'], foreach=False)
    for q, m, v, g in zip(params, before[1], before[2], gs):
        opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
        q.grad = torch.from_numpy(g.copy())
    norm = None
    if hp['max_norm'] is not None:
        norm = float(torch.nn.utils.clip_grad_norm_(params, hp['max_norm'], foreach=False))
    opt.step()
    return norm, ([q.detach().numpy() for q in params], [opt.state[q]['exp_avg'].numpy() for q in params],
                  [opt.state[q]['exp_avg_sq'].numpy() for q in params])


def within_twice(got, other, before, gs, hp, t, lr):
    """max |got - other| / (2 bound), the bound of the float64 step with the norm's own error in it"""
    c = H.coef_ref(H.norm_ref(gs), hp['max_norm']) if hp['max_norm'] is not None else H.coef_ref(None, None)
    worst = 0.0
    for i in range(len(gs)):
        ref = H.adamw_ref(before[0][i], gs[i], before[1][i], before[2][i], c, hp, t, lr)
        for k, name in enumerate('pmv'):
            worst = max(worst, worst_ratio(got[k][i], other[k][i], 2 * ref[name].e))
    return worst


# ------------------------------------------------------------------------------------------------------------ the norm
def test_norm_against_float64_and_bit_identical_over_runs():
    case = Case(HP_REF)
    gs, grads, bufs = case.grads(1, 1.0)
    opt = case.opt
    opt._g_ptrs.copy_(torch.tensor([grads[n].data_ptr() for n in case.names], dtype=torch.int64))
    runs = [ops.grad_sqnorm(opt._chunks, opt._g_ptrs, opt._partial, torch.empty((), device=DEV)).clone() for _ in range(3)]
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])
    ref = H.norm_ref(gs)
    r = worst_ratio(runs[0], ref.v, ref.e)
    measured('norm of the test list, error / bound', r)
    assert r <= 1.0 and opt.num_chunks == H.chunks_of(ALL_SIZES)
    assert case.guards_intact(bufs) and all(same_bits(grads[n], torch.from_numpy(g)) for n, g in zip(case.names, gs))
    # one tensor, one element; and nothing but zeros
    one = optim.AdamW([('w', torch.zeros(1, device=DEV))], max_norm=1.0)
    assert float(one.step({'w': torch.full((1,), -3.0, device=DEV)})) == 3.0
    assert float(one.step({'w': torch.zeros(1, device=DEV)})) == 0.0


# ---------------------------------------------------------------------------------------------------------- the update
@pytest.mark.parametrize('hp', [HP_REF, HP_LOUD, dict(HP_LOUD, wd=0.0)], ids=['reference', 'loud', 'no_decay'])
def test_five_steps_against_float64_and_torch(hp):
    case = Case(hp)
    worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0, torch=0.0)
    active = []
    for t in range(1, 6):
        lr = hp['lr'] * LRS[t - 1]
        gs, grads, bufs = case.grads(t, SCALES[t - 1])
        before = case.state()
        case.opt.lr = lr
        norm = case.opt.step(grads)
        after = case.state()
        assert case.opt.step_count == t and norm.shape == () and norm.is_cuda
        r = H.step_ratios(before, gs, after, None, hp, t, lr, given_norm=float(norm))       # given the GPU's own norm
        ref_norm = H.norm_ref(gs)
        r['norm'] = worst_ratio(norm, ref_norm.v, ref_norm.e)
        tnorm, tafter = torch_step(before, gs, hp, t, lr)
        r['torch'] = within_twice(after, tafter, before, gs, hp, t, lr)
        for k in r:
            worst[k] = max(worst[k], r[k])
        active.append(float(norm) > hp['max_norm'])
        # the gradients are left as they came (the clipped gradient is not written back), the guards around the views too
        assert all(same_bits(grads[n], torch.from_numpy(g)) for n, g in zip(case.names, gs))
        assert case.guards_intact(bufs) and case.guards_intact(case.p_bufs)
    for k, x in worst.items():
        measured(f'five steps, {k}: error / bound', x)
    assert max(worst.values()) <= 1.0, worst
    assert any(active) and not all(active)


def test_vector_path_with_a_scalar_head_keeps_the_guards():
    """all four roles at the SAME 4-byte-only phase: scalar head, 16-byte body, scalar tail (AdamW's own moments are
    16-byte aligned, so only a caller of the C entry reaches this path)"""
    hp, t, lr = HP_LOUD, 3, HP_LOUD['lr']
    rng = np.random.RandomState(5)
    for off in (1, 2, 3):
        size = 2 * CHUNK + 7
        host = [(rng.randn(size) * s).astype(f32) for s in (0.1, 1.0, 0.05)] + [(rng.rand(size) * 0.01).astype(f32)]
        bufs, views = [], []
        for h in host:
            buf, v = view_in(size + 9, off, size, GUARD)
            v.copy_(torch.from_numpy(h))
            bufs.append((buf, off, size))
            views.append(v)
        chunks = ops.AdamwChunks([size], DEV)
        ptr = [torch.tensor([v.data_ptr()], dtype=torch.int64, device=DEV) for v in views]
        norm = ops.grad_sqnorm(chunks, ptr[1], torch.empty(3, device=DEV), torch.empty((), device=DEV))
        ops.adamw_step(chunks, ptr[0], ptr[1], ptr[2], ptr[3], norm, hp['max_norm'], lr, hp['wd'], *hp['betas'], hp['eps'], t)
        after = [[views[k].cpu().numpy()] for k in (0, 2, 3)]
        r = H.step_ratios(([host[0]], [host[2]], [host[3]]), [host[1]], after, None, hp, t, lr, given_norm=float(norm))
        ref_norm = H.norm_ref([host[1]])
        assert max(r.values()) <= 1.0 and worst_ratio(norm, ref_norm.v, ref_norm.e) <= 1.0, (off, r)
        for buf, o, s in bufs:
            b = buf.cpu()
            assert bool((b[:o] == GUARD).all()) and bool((b[o + s:] == GUARD).all()), off
        assert same_bits(views[1], torch.from_numpy(host[1]))


# -------------------------------------------------------------------------------------------------------------- regimes
def test_zero_gradient_and_zero_moments_decay_only():
    hp = HP_LOUD
    case = Case(hp)
    before = case.state()
    _, grads, _ = case.grads(1, 0.0)
    norm = case.opt.step(grads)
    after = case.state()
    assert float(norm) == 0.0
    decay = f32(1 - hp['lr'] * hp['wd'])
    for p0, p1, m1, v1 in zip(before[0], *after):
        assert np.array_equal(p1, p0 * decay) and not m1.any() and not v1.any()


def test_gradients_far_below_eps():
    hp = dict(HP_REF, max_norm=None)
    case = Case(hp)
    for t in (1, 2):
        # |g| ~ 1e-10 << eps = 1e-8: sqrt(v) << eps, the update is ~ lr g / eps, not lr sign(g).  Not smaller: the bounds
        # model no fp32 underflow (tests/test_stream_ops_host.py), and (1 - beta2) g^2 must stay a normal number for the
        # smallest of the ~3e4 draws -- asserted, so that the inputs are inside the model by construction
        gs, grads, _ = case.grads(t, 1e-10)
        assert min(float((1e-3 * g.astype(np.float64) ** 2).min()) for g in gs) >= 2.0 ** -126
        assert max(float(np.abs(g).max()) for g in gs) < 1e-9
        before = case.state()
        assert case.opt.step(grads) is None
        r = H.step_ratios(before, gs, case.state(), None, hp, t, hp['lr'])
        assert max(r.values()) <= 1.0, r
    assert max(float(np.abs(m).max()) for m in case.state()[1]) > 0


def test_without_max_norm_the_norm_pass_is_skipped():
    hp = dict(HP_LOUD, max_norm=None)
    case = Case(hp)
    case.opt._partial.fill_(float('nan'))                        # what the norm pass would have written
    gs, grads, _ = case.grads(1, 3.0)
    before = case.state()
    assert case.opt.step(grads) is None
    assert bool(torch.isnan(case.opt._partial).all())
    r = H.step_ratios(before, gs, case.state(), None, hp, 1, hp['lr'])
    assert max(r.values()) <= 1.0, r


def _plant(value, tensor=4, index=7):
    def edit(gs):
        gs[tensor][index] = value
    return edit


def test_nan_gradient_makes_every_parameter_nan_as_with_torch():
    """pinned, not approved of: one NaN in one tensor's gradient -> norm NaN -> c NaN -> every element of p, m, v"""
    hp = HP_REF
    case = Case(hp)
    gs, grads, _ = case.grads(1, 1.0, edit=_plant(float('nan')))
    before = case.state()
    norm = case.opt.step(grads)
    after = case.state()
    _, tafter = torch_step(before, gs, hp, 1, hp['lr'])
    assert bool(torch.isnan(norm))
    for k in range(3):
        for a, b in zip(after[k], tafter[k]):
            assert np.isnan(a).all() and np.isnan(b).all()


def test_inf_gradient_equals_torch():
    """norm = inf -> c = 0 -> g' = 0 except at the inf itself (0 inf = NaN): from zero moments every other element is
    p (1 - lr wd) exactly, in the kernel and in torch alike.  Both accumulate the norm in fp32, so there is no difference
    from a wider accumulator to document: a sum of squares that overflows fp32 gives inf in both."""
    hp = HP_LOUD
    for value in (float('inf'), 3e30):                           # an inf, and a finite value whose square overflows fp32
        case = Case(hp)
        gs, grads, _ = case.grads(1, 1.0, edit=_plant(value))
        before = case.state()
        norm = case.opt.step(grads)
        after = case.state()
        tnorm, tafter = torch_step(before, gs, hp, 1, hp['lr'])
        assert float(norm) == float('inf') == tnorm
        for k in range(3):
            for a, b in zip(after[k], tafter[k]):
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
        assert sum(int(np.isnan(a).sum()) for a in after[0]) == (1 if value == float('inf') else 0)


# -------------------------------------------------------------------------------------------------------------- interop
def test_state_dict_continues_in_torch():
    hp = HP_LOUD
    case = Case(hp)
    for t in (1, 2):
        case.opt.lr = hp['lr'] * LRS[t - 1]
        case.opt.step(case.grads(t, SCALES[t - 1])[1])
    before = case.state()
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in before[0]]
    th = torch.optim.AdamW(params, foreach=False)
    th.load_state_dict(case.opt.state_dict())
    t, lr = 3, hp['lr'] * LRS[2]
    gs, grads, _ = case.grads(t, SCALES[2])
    th.param_groups[0]['lr'] = lr
    for q, g in zip(params, gs):
        q.grad = torch.from_numpy(g.copy())
    tnorm = float(torch.nn.utils.clip_grad_norm_(params, hp['max_norm'], foreach=False))
    th.step()
    tafter = ([q.detach().numpy() for q in params], [th.state[q]['exp_avg'].numpy() for q in params],
              [th.state[q]['exp_avg_sq'].numpy() for q in params])
    assert all(float(th.state[q]['step']) == 3 for q in params)
    case.opt.lr = lr
    case.opt.step(grads)
    r = within_twice(case.state(), tafter, before, gs, hp, t, lr)
    measured('step 3 in torch from our state dict against ours, difference / twice the bound', r)
    assert r <= 1.0 and max(H.step_ratios(before, gs, tafter, tnorm, hp, t, lr).values()) <= 1.0


def test_resume_is_bit_identical():
    hp = HP_LOUD
    whole, first = Case(hp), Case(hp)
    for t in range(1, 5):
        whole.opt.lr = hp['lr'] * LRS[t - 1]
        whole.opt.step(whole.grads(t, SCALES[t - 1])[1])
    for t in (1, 2):
        first.opt.lr = hp['lr'] * LRS[t - 1]
        first.opt.step(first.grads(t, SCALES[t - 1])[1])
    second = Case(hp, seed=9)                                    # other values: everything comes from the saved state
    for p, q in zip(second.params, first.params):
        p.copy_(q)
    second.opt.load_state_dict(first.opt.state_dict())
    assert second.opt.step_count == 2
    for t in (3, 4):
        second.opt.lr = hp['lr'] * LRS[t - 1]
        second.opt.step(second.grads(t, SCALES[t - 1])[1])
    for a, b in zip(whole.state(), second.state()):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_step_refuses_gradients_that_do_not_match():
    case = Case(HP_REF)
    _, grads, _ = case.grads(1, 1.0)
    before = case.state()
    with pytest.raises(KeyError):
        case.opt.step({k: v for k, v in grads.items() if k != 't3'})
    with pytest.raises(KeyError):
        case.opt.step(dict(grads, extra=grads['t0']))
    with pytest.raises(ValueError, match='shape'):
        case.opt.step(dict(grads, t3=grads['t4']))
    with pytest.raises(ValueError, match='lives on'):
        case.opt.step(dict(grads, t3=grads['t3'].cpu()))
    with pytest.raises(ScflowHipError):
        ops.grad_sqnorm(case.opt._chunks, case.opt._g_ptrs[:3], case.opt._partial, torch.empty((), device=DEV))
    with pytest.raises(ScflowHipError):
        ops.grad_sqnorm(case.opt._chunks, case.opt._g_ptrs, case.opt._partial[:3], torch.empty((), device=DEV))
    assert case.opt.step_count == 0
    for a, b in zip(before, case.state()):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
