"""Benchmark of the training step (``SCFlowRefiner.train_step``, scflow_amd/optim.py, csrc/optim.hip) on the model's own
117 trainable tensors (7,111,358 floats) at batch 32, 256 x 256 images, 8 iterations.
    python tools/bench_train_step.py [N] [T]   -> one JSON line
Device events bracket a window of calls; every column is warmed up first; the columns alternate inside one run; every
figure is the median of ``REPS`` >= 20 windows, with the minimum and the 10 % .. 90 % spread next to it.

* ``optimizer_us``: ``AdamW.step`` alone (norm pass, finish, update: three launches) on fixed random gradients, and
  ``optimizer_noclip_us`` without the norm pass (one launch).  ``floor_fraction``: 32 B (28 B) per parameter at the
  6.29 TB/s float4-copy rate of DESIGN.md 4.11 over the median.  The events bracket the Python call, so the figures include
  the binding's host path (117 ``data_ptr()`` calls, the argument checks).
* ``torch_us``: the same tensors through ``torch.nn.utils.clip_grad_norm_(foreach=True)`` + ``torch.optim.AdamW(fused=True)``
  in the same process, alternating with ours.  ``not_slower_than_torch``: ours <= torch's + the larger of the two spreads.
* ``repack_us``: ``get_pose`` right after ``invalidate_packed()`` minus a warm ``get_pose``: what re-packing every
  kernel-layout weight copy costs the forward after a step.
* ``train_step_us``: one step as it runs in a training loop, entered with the packs dropped by the step before; and
  ``train_step_packed_us``, entered with the packs in place.  Its parts, all entered with the packs in place: ``loss()``
  (forward and loss values), ``loss_and_context_grads()`` (forward, loss, backward), the optimizer step above;
  ``backward_us`` is the difference of the first two.

The pose loss is a ``RAFTLoss`` on ``flow_from_pose`` (as in the GPU tests): the point-matching losses need the dataset's
meshes.  Ground truth: the reference poses perturbed by a few degrees and millimetres."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import optim  # noqa: E402

dev = 'cuda:0'
COPY_RATE = 6.29e12
REPS = 25
HP = dict(lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


def window(fn, inner):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    return s, e


def alternate(columns, n=REPS):
    """columns: name -> (fn, inner[, setup]); every repetition times each column once, in turn; ``setup`` runs before the
    window, untimed, and puts the model into the state the column is about"""
    columns = {k: (v + (None,))[:3] for k, v in columns.items()}
    for fn, _, setup in columns.values():
        for _ in range(3):
            if setup:
                setup()
            fn()
    evs = {k: [] for k in columns}
    for _ in range(n):
        for k, (fn, inner, setup) in columns.items():
            if setup:
                setup()
            evs[k].append((window(fn, inner), inner))
    torch.cuda.synchronize()
    out = {}
    for k, lst in evs.items():
        ts = sorted(s.elapsed_time(e) / inner * 1e3 for (s, e), inner in lst)
        out[k] = dict(median=round(ts[len(ts) // 2], 1), min=round(ts[0], 1),
                      spread=round(ts[int(0.9 * (len(ts) - 1))] - ts[int(0.1 * (len(ts) - 1))], 1), windows=len(ts),
                      calls_per_window=lst[0][1])
    return out


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T = int(sys.argv[2]) if len(sys.argv) > 2 else 8
H = W = 256
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
shapes = json.load(open(os.path.join(root, 'tests', 'golden', 'state_dict_keys.json')))['shapes']
cfg = scflow_amd.scflow_model_cfg(iters=T)
cfg.update(scflow_amd.scflow_loss_cfgs(mesh_path='not/used'))
cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='RAFTLoss', loss_weight=1.0, max_flow=400.))
cfg.update(freeze_encoder=True, freeze_bn=True)
model = scflow_amd.build_refiner(cfg)
model.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
model = model.to(dev)
named = model.trainable_parameters()
count = sum(p.numel() for _, p in named)

# ---- the optimizer step alone, ours and torch's, on the same values
torch.manual_seed(0)
grads = {k: torch.randn_like(p) * 0.01 for k, p in named}
mine = [(k, p.detach().clone()) for k, p in named]
ours = optim.AdamW(mine, max_norm=10., **HP)
ours_noclip = optim.AdamW([(k, p.detach().clone()) for k, p in named], max_norm=None, **HP)
theirs = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
for q, (k, _) in zip(theirs, named):
    q.grad = grads[k].clone()
topt = torch.optim.AdamW(theirs, fused=True, amsgrad=False, **HP)


def torch_pair():
    torch.nn.utils.clip_grad_norm_(theirs, 10., foreach=True)
    topt.step()


res = alternate({'optimizer': (lambda: ours.step(grads), 20), 'torch': (torch_pair, 20),
                 'optimizer_noclip': (lambda: ours_noclip.step(grads), 20)})
out = dict(batch=n, image=[H, W], iters=T, tensors=len(named), parameters=count, chunks=ours.num_chunks,
           optimizer_us=res['optimizer'], optimizer_noclip_us=res['optimizer_noclip'], torch_us=res['torch'])
out['floor_us'] = dict(clip=round(32 * count / COPY_RATE * 1e6, 1), noclip=round(28 * count / COPY_RATE * 1e6, 1))
out['floor_fraction'] = dict(clip=round(out['floor_us']['clip'] / res['optimizer']['median'], 3),
                             noclip=round(out['floor_us']['noclip'] / res['optimizer_noclip']['median'], 3))
margin = max(res['optimizer']['spread'], res['torch']['spread'])
out['not_slower_than_torch'] = bool(res['optimizer']['median'] <= res['torch']['median'] + margin)
# one step from equal state: the two must agree to rounding (plausibility; tests/test_gpu_optim.py holds the bounds)
a = optim.AdamW([(k, p.detach().clone()) for k, p in named], max_norm=10., **HP)
b = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
for q, (k, _) in zip(b, named):
    q.grad = grads[k].clone()
bopt = torch.optim.AdamW(b, fused=True, **HP)
a.step(grads)
torch.nn.utils.clip_grad_norm_(b, 10., foreach=True)
bopt.step()
out['worst_difference_to_torch'] = max(float((x - y.detach()).abs().max()) for x, y in zip(a.params, b))

# ---- the whole step and its parts
inp = {k: v.to(dev) for k, v in scflow_amd.make_inputs(n, H, W, seed=1).items()}
g = torch.Generator().manual_seed(2)
ang = torch.randn(n, generator=g) * 0.03
rz = torch.eye(3).repeat(n, 1, 1)
rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1] = ang.cos(), -ang.sin(), ang.sin(), ang.cos()
data = dict(ref_rotations=inp['ref_rotation'], ref_translations=inp['ref_translation'],
            gt_rotations=rz.to(dev) @ inp['ref_rotation'],
            gt_translations=inp['ref_translation'] + (torch.randn(n, 3, generator=g) * torch.tensor([3., 3., 12.])).to(dev),
            labels=inp['label'], internel_k=inp['internel_k'], rendered_images=inp['render_images'],
            real_images=inp['real_images'], rendered_masks=(inp['depth'] > 0).float(), rendered_depths=inp['depth'],
            gt_masks=inp['depth'] > 0)
opt = optim.build_optimizer(model, dict(type='AdamW', amsgrad=False, **HP), dict(grad_clip=dict(max_norm=10.)),
                            dict(policy='OneCycle', max_lr=4e-4, total_steps=100100, pct_start=0.05, anneal_strategy='linear'))
pose = lambda: model.get_pose(data['rendered_images'], data['real_images'], data['ref_rotations'], data['ref_translations'],   # noqa: E731
                              data['rendered_depths'], data['internel_k'], data['labels'])


first = model.train_step(None, opt, data=data)['log_vars']
res = alternate({'train_step': (lambda: model.train_step(None, opt, data=data), 1, model.invalidate_packed),
                 'train_step_packed': (lambda: model.train_step(None, opt, data=data), 1, pose),
                 'loss': (lambda: model.loss(None, data=data), 1, pose),
                 'loss_and_context_grads': (lambda: model.loss_and_context_grads(None, data=data), 1, pose),
                 'get_pose': (pose, 1, pose), 'get_pose_after_invalidate': (pose, 1, model.invalidate_packed)})
last = model.train_step(None, opt, data=data)['log_vars']
out.update(train_step_us=res['train_step'], train_step_packed_us=res['train_step_packed'], loss_us=res['loss'],
           loss_and_context_grads_us=res['loss_and_context_grads'],
           backward_us=round(res['loss_and_context_grads']['median'] - res['loss']['median'], 1),
           get_pose_us=res['get_pose'], get_pose_after_invalidate_us=res['get_pose_after_invalidate'],
           repack_us=round(res['get_pose_after_invalidate']['median'] - res['get_pose']['median'], 1),
           optimizer_share_of_train_step=round(out['optimizer_us']['median'] / res['train_step']['median'], 5),
           steps_taken=opt.step_count, loss_first=first['loss'], loss_last=last['loss'],
           grad_norm_first=first['grad_norm'], finite=bool(math.isfinite(last['loss'])))
print(json.dumps(out))
