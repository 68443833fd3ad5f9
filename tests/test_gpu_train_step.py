"""GPU: ``SCFlowRefiner.train_step`` -- the gradients of ``loss_and_context_grads()`` applied by ``scflow_amd.optim.AdamW``
on the small random-weight refiner of the loss tests (256 x 256, three samples, three iterations): the step against the
float64 restatement of tests/test_optim_host.py, what must stay frozen, that the next forward reads the new weights (no
stale pack, fold or context cache), reproducibility, the multi-cycle loop and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import optim
import test_loss_host as HL
import test_optim_host as H
from test_stream_ops_host import measured, same_bits
from test_gpu_gru_grad import scflow_model  # noqa: F401  (the small random-weight refiner, a module-scoped fixture)
from test_gpu_render import scene  # noqa: F401  (three small meshes, a renderer and a batch of four, module-scoped)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HP = dict(lr=4e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-4, max_norm=10.)       # the reference's recipe


def build(case, sd, cycles=1, **over):
    """a new refiner with the fixture's configuration (its pose loss is a RAFTLoss on flow_from_pose) and the weights `sd`"""
    cfg = scflow_amd.scflow_model_cfg(iters=HL.REFINER_ITERS)
    cfg.update(HL.refiner_loss_cfgs(case))
    cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.7, loss_func_cfg=dict(type='RAFTLoss', loss_weight=0.3, max_flow=400.))
    cfg.update(dict(freeze_encoder=True, freeze_bn=True, train_cfg=dict(cycles=cycles)), **over)
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def optimizer(m, hp=HP, **kw):
    return optim.AdamW(m.trainable_parameters(), lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['wd'],
                       max_norm=hp['max_norm'], model=m, **kw)


def same(a, b):
    """bit for bit; the state dict also holds BatchNorm's integer num_batches_tracked"""
    return same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


def snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def same_outputs(a, b, data):
    la, lb = a.loss(None, data=data), b.loss(None, data=data)
    if not same_bits(la[0], lb[0]) or list(la[2].items()) != list(lb[2].items()):
        return False
    pa = a.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                    data['rendered_depths'], data['internel_k'], data['labels'])
    pb = b.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],
                    data['rendered_depths'], data['internel_k'], data['labels'])
    return all(same_bits(x, y) for sa, sb in zip(pa, pb) for x, y in zip(sa, sb))


@pytest.fixture(scope='module')
def start(scflow_model):
    m, case = scflow_model
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, case


def test_one_step(start):
    """the gradients used are the bits of loss_and_context_grads(); all 117 tensors land inside the float64 bound; nothing
    else moves; the next forward reads the new weights"""
    sd, case = start
    data = HL.refiner_data(case, DEV)
    m = build(case, sd)
    want = m.loss_and_context_grads(None, data=data)
    before = snapshot(m)
    opt = optimizer(m, schedule=optim.OneCycle(4e-4, 100100, pct_start=0.05, anneal_strategy='linear'))
    used = {}
    real_step = opt.step

    def spy(grads, **kw):
        used.update({k: v.clone() for k, v in grads.items()})
        return real_step(grads, **kw)
    opt.step = spy
    out = m.train_step(None, opt, data=data)
    assert sorted(out) == ['log_imgs', 'log_vars', 'loss', 'num_samples'] and out['log_imgs'] is None
    assert out['num_samples'] == HL.REFINER_N and same_bits(out['loss'], want[0])
    log = out['log_vars']
    assert list(log)[:-2] == list(want[2]) and list(log)[-2:] == ['grad_norm', 'lr']
    assert all(log[k] == want[2][k] for k in want[2]) and log['lr'] == 4e-4 / 25 == opt.lr
    names = [n for n, _ in m.trainable_parameters()]
    assert sorted(used) == sorted(want[5]['params']) == sorted(names) and len(names) == 117
    assert all(same_bits(used[n], want[5]['params'][n]) for n in names)
    # the step against float64, given the GPU's own norm (log_vars carries its fp32 value exactly)
    after = snapshot(m)
    cpu = lambda ts: [t.cpu().numpy().reshape(-1) for t in ts]      # noqa: E731
    gs = cpu([used[n] for n in names])
    zeros = [np.zeros_like(g) for g in gs]
    r = H.step_ratios((cpu([before[n] for n in names]), zeros, zeros), gs,
                      (cpu([after[n] for n in names]), cpu(opt.exp_avg), cpu(opt.exp_avg_sq)), None, HP, 1, opt.lr,
                      given_norm=log['grad_norm'])
    ref_norm = H.norm_ref(gs, nchunks=opt.num_chunks)
    r['norm'] = abs(log['grad_norm'] - float(ref_norm.v)) / float(ref_norm.e)
    for k, x in r.items():
        measured(f'train_step, {k} of the 117 tensors: error / bound', x)
    assert max(r.values()) <= 1.0, r
    assert sum(int(not same_bits(before[n], after[n])) for n in names) >= 100      # it did step
    # frozen: the feature encoders and every buffer, BatchNorm's running statistics included
    frozen = [k for k in before if k not in set(names)]
    assert len(frozen) > 20 and any('running_mean' in k for k in frozen) and any(k.startswith('render_encoder.') for k in frozen)
    assert all(same(before[k], after[k]) for k in frozen)
    # fresh weights: a model built from the stepped state dict computes the same bits
    assert same_outputs(m, build(case, {k: v.cpu() for k, v in after.items()}), data)
    assert not same_bits(m.loss(None, data=data)[0], want[0])


def test_three_steps_reproduce_and_leave_no_stale_copy(start):
    sd, case = start
    batches = [HL.refiner_data(HL.refiner_loss_case(7 + i, 5 + i), DEV) for i in range(3)]
    models = [build(case, sd) for _ in range(2)]
    logs = []
    for m in models:
        opt = optimizer(m)
        m.get_pose(*[batches[0][k] for k in ('rendered_images', 'real_images', 'ref_rotations', 'ref_translations',
                                             'rendered_depths', 'internel_k', 'labels')])       # packs exist before the steps
        logs.append([m.train_step(None, opt, data=b)['log_vars'] for b in batches])
        assert opt.step_count == 3 and opt.iteration == 3
    assert logs[0] == logs[1]
    a, b = snapshot(models[0]), snapshot(models[1])
    assert all(same(a[k], b[k]) for k in a)
    assert logs[0][0]['loss'] != logs[0][1]['loss']
    assert same_outputs(models[0], build(case, {k: v.cpu() for k, v in a.items()}), batches[0])


def _train_batch(scene):
    renderer, batch, (R, t, K, labels) = scene
    shift = torch.tensor([2.0, -3.0, 8.0], device=DEV)
    annots = dict(batch['annots'], gt_rotations=[R[:2], R[2:]], gt_translations=[t[:2] + shift, t[2:] + shift])
    annots['gt_masks'] = [g.bool() for g in annots['gt_masks']]
    return renderer, dict(batch, annots=annots)


def test_two_cycles_equal_two_steps_with_update_data(start, scene):
    sd, case = start
    renderer, batch = _train_batch(scene)
    two = build(case, sd, cycles=2).attach_renderer(renderer)
    out = two.train_step(batch, optimizer(two))
    one = build(case, sd).attach_renderer(renderer)
    opt = optimizer(one)
    data = one.format_data_train_sup(batch)
    first = one.loss_and_context_grads(batch, data=dict(data))
    s1 = one.train_step(batch, opt, data=data)
    data2 = one.update_data(first[3][-1], first[4][-1], dict(data))
    s2 = one.train_step(batch, opt, data=data2)
    a, b = snapshot(two), snapshot(one)
    assert all(same(a[k], b[k]) for k in a)
    assert opt.step_count == 2
    log = out['log_vars']
    keys = list(s1['log_vars'])
    assert list(log) == keys[:-1] + ['iter_0_loss', 'lr'] and out['num_samples'] == 2 and keys[-2:] == ['grad_norm', 'lr']
    assert log['iter_0_loss'] == s1['log_vars']['loss'] and same_bits(out['loss'], s2['loss'])
    for k in keys[:-1]:
        assert log[k] == (s1['log_vars'][k] + s2['log_vars'][k]) / 2, k
    assert s1['log_vars']['loss'] != s2['log_vars']['loss']
    bare = build(case, sd, cycles=2)
    with pytest.raises(RuntimeError, match='attach a renderer'):
        bare.train_step(batch, optimizer(bare))


def test_refusals(start):
    sd, case = start
    data = HL.refiner_data(case, DEV)
    for over, what in ((dict(freeze_encoder=False), 'feature-encoder and correlation-build backward'),
                       (dict(freeze_bn=False), 'BatchNorm on batch statistics')):
        m = build(case, sd, **over)
        before = snapshot(m)
        with pytest.raises(NotImplementedError, match=what):
            m.train_step(None, optimizer(m), data=data)
        assert all(same(v, before[k]) for k, v in m.state_dict().items())
    m = build(case, sd)
    with pytest.raises(TypeError, match='scflow_amd.optim.AdamW'):
        m.train_step(None, torch.optim.AdamW(m.parameters(), lr=4e-4), data=data)
    with pytest.raises(ValueError, match='trainable_parameters'):
        m.train_step(None, optimizer(build(case, sd)), data=data)
    opt = optimizer(m)
    m.decoder.detach_flow = False
    try:
        with pytest.raises(NotImplementedError, match='detach_flow=False'):
            m.train_step(None, opt, data=data)
    finally:
        m.decoder.detach_flow = True
    assert opt.step_count == 0
    with pytest.raises(NotImplementedError, match='train_step and the backward'):
        m.forward(data, return_loss=True)
