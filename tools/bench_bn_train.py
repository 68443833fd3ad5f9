"""Micro-benchmark of BatchNorm on batch statistics (``scf_batch_norm_train`` / ``scf_batch_norm_train_grad``) and of the
context encoder's backward on them (``RAFTEncoder.bn_backward``) at the workload's sizes: N = 32 images of 3 x 256 x 256,
whose planes are (64, 128^2), (96, 64^2) and (128, 32^2).  Device events bracket a window of calls; every column is warmed
up first; the columns alternate inside one process, and each figure is the median of the windows with their 10 % and 90 %
points.
    python tools/bench_bn_train.py [N]   -> one JSON line
``ops_us``: per form and size, ``forward`` and ``backward`` are one call each (two launches; the events bracket the Python
calls, so they include the binding's host path and its allocations), ``first_launch`` the device time of the call's first
launch alone (the statistics pass of ``u``, the backward's reduce pass) from the launch's own timestamps, median of 7.
``floor_fraction``: the mid form's byte floor -- forward 12 bytes an element (u read twice, y written once), backward
24 -- at the 6.29 TB/s float4-copy rate of DESIGN.md 4.11, over the measured median; what the launches really move is
more in the tail forms (the residual, the kept y, g') and 20 bytes in the backward's mid form, so the fractions of the tail
forms understate them.
``hip_us`` is ``bn_backward`` from what a forward under ``batch_stats()`` + ``keeping()`` keeps; ``hip_forward_us`` that
forward, ``eval_forward_us`` the folded eval forward next to it.  ``torch_us`` is torch autograd on the same GPU of the same
encoder built from ``torch.nn.functional`` (``conv2d``, ``batch_norm(training=True)``, ``relu``) on the same tensors,
forward + backward; ``torch_backward_us`` its ``backward()`` alone.  The gradients of the two are compared at the end,
relative to the largest entry (a plausibility figure; the kernels are held to float64 by tests/test_gpu_bn_train.py)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.modules import RAFTEncoder  # noqa: E402

dev = 'cuda:0'
COPY_RATE = 6.29e12
EPS, MOMENTUM = 1e-5, 0.1


def window(fn, inner, args=()):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn(*args)
    e.record()
    return s, e


def alternate(columns, n=11):
    """columns: name -> (fn, inner, setup or None); every repetition times each column once, in turn"""
    for fn, _, setup in columns.values():
        for _ in range(2):
            fn(*(setup() if setup else ()))
    evs = {k: [] for k in columns}
    for _ in range(n):
        for k, (fn, inner, setup) in columns.items():
            evs[k].append((window(fn, inner, setup() if setup else ()), inner))
    torch.cuda.synchronize()
    out = {}
    for k, lst in evs.items():
        ts = sorted(s.elapsed_time(e) / inner for (s, e), inner in lst)
        out[k] = dict(median=round(ts[len(ts) // 2] * 1e3, 1), p10=round(ts[n // 10] * 1e3, 1), p90=round(ts[n - 1 - n // 10] * 1e3, 1))
    return out


def first_launch(fn, n=7):
    fn()
    ts = sorted(ops.time_first_kernel(fn) for _ in range(n))
    return round(ts[n // 2], 1)


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
H = W = 256
torch.manual_seed(0)

# ---- the operators, per form and size
cols, firsts, elems = {}, {}, {}
for c, hw in ((64, 128), (96, 64), (128, 32)):
    shape = (n, c, hw, hw)
    u, r, g = (torch.randn(shape, device=dev) for _ in range(3))
    vec = lambda: (torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev), torch.zeros(c, device=dev), torch.ones(c, device=dev))  # noqa: E731
    pa, pb = vec(), vec()
    ws = torch.empty(ops.batch_norm_train_workspace(n, c, hw * hw), device=dev)
    y = torch.empty(shape, device=dev)
    outs = [torch.empty(shape, device=dev) for _ in range(2)]
    for form in ('mid', 'tail', 'tail_ds'):
        kw = dict(mid={}, tail=dict(res=r), tail_ds=dict(res=r, res_bn=pb))[form]
        fwd = lambda kw=kw, u=u, pa=pa, y=y, ws=ws: ops.batch_norm_train(u, *pa, MOMENTUM, EPS, relu=True, out=y, workspace=ws, **kw)  # noqa: E731
        res = fwd()
        yk, saved = res[0].clone(), res[1]
        gm = torch.where(yk > 0, g, torch.zeros((), device=dev))
        if form == 'mid':
            bwd = lambda u=u, gm=gm, saved=saved, pa=pa, outs=outs, ws=ws: ops.batch_norm_train_grad(  # noqa: E731
                gm, u, saved, pa[0], out=[outs[0], None, None], workspace=ws)
        elif form == 'tail':
            bwd = lambda u=u, g=g, saved=saved, pa=pa, yk=yk, outs=outs, ws=ws: ops.batch_norm_train_grad(  # noqa: E731
                g, u, saved, pa[0], y=yk, out=outs + [None, None], workspace=ws)
        else:
            bwd = lambda u=u, g=g, r=r, saved=saved, sr=res[2], pa=pa, pb=pb, yk=yk, outs=outs, ws=ws: ops.batch_norm_train_grad(  # noqa: E731
                g, u, saved, pa[0], y=yk, r=r, saved_r=sr, gamma_r=pb[0], out=outs + [None] * 4, workspace=ws)
        name = f'{form} {c}@{hw}'
        cols[f'{name} forward'], cols[f'{name} backward'] = (fwd, 10, None), (bwd, 10, None)
        firsts[name] = dict(forward=first_launch(fwd), backward=first_launch(bwd))
        elems[name] = u.numel()
ops_res = alternate(cols)
ops_us, floor = {}, {}
for name, e in elems.items():
    f, b = ops_res[f'{name} forward'], ops_res[f'{name} backward']
    ops_us[name] = dict(forward=f, backward=b, first_launch=firsts[name])
    floor[name] = dict(forward=round(e * 12 / COPY_RATE * 1e6 / f['median'], 3), backward=round(e * 24 / COPY_RATE * 1e6 / b['median'], 3))
del cols, u, r, g, y, outs, yk, gm, ws

# ---- the encoder's stage against torch autograd on the same tensors
enc = RAFTEncoder(3, 256, norm_cfg=dict(type='BN'))
with torch.no_grad():
    for name, p in enc.named_parameters():
        p.copy_(torch.randn_like(p) * (0.05 if p.dim() > 1 else 0.1) + (1.0 if p.dim() == 1 and 'bn' in name and name.endswith('weight') else 0.0))
enc = enc.to(dev)
x = torch.randn(n, 3, H, W, device=dev)
g = torch.randn(n, 256, H // 8, W // 8, device=dev)


def hip_forward():
    with enc.batch_stats(), enc.keeping():
        enc(x)
    return enc.kept


saved = hip_forward()
grads = enc.bn_backward(saved, g)
torch.cuda.synchronize()
P = {k: v.detach().clone().requires_grad_(True) for k, v in enc.named_parameters()}


def t_layer(v, ckey, bkey, stride, pad):
    u = F.conv2d(v, P[f'{ckey}.weight'], P[f'{ckey}.bias'], stride=stride, padding=pad)
    return F.batch_norm(u, None, None, P[f'{bkey}.weight'], P[f'{bkey}.bias'], True, MOMENTUM, EPS)


def t_forward():
    v = torch.relu(t_layer(x, 'conv1', 'bn1', 2, 3))
    for li, stride in enumerate((1, 2, 2), start=1):
        for j in range(2):
            key, s = f'res_layer{li}.{j}', (stride if j == 0 else 1)
            t = torch.relu(t_layer(v, f'{key}.conv1', f'{key}.bn1', s, 1))
            idt = t_layer(v, f'{key}.downsample.0', f'{key}.downsample.1', s, 0) if f'{key}.downsample.0.weight' in P else v
            v = torch.relu(t_layer(t, f'{key}.conv2', f'{key}.bn2', 1, 1) + idt)
    return F.conv2d(v, P['conv2.weight'], P['conv2.bias'])


leaves = list(P.values())


def t_both():
    return torch.autograd.grad((t_forward() * g).sum(), leaves)


res = alternate({'hip': (lambda: enc.bn_backward(saved, g), 2, None), 'hip_forward': (hip_forward, 2, None),
                 'eval_forward': (lambda: enc(x), 2, None), 'torch': (t_both, 2, None),
                 'torch_backward': (lambda loss: torch.autograd.grad(loss, leaves), 1, lambda: ((t_forward() * g).sum(),))})
saved = hip_forward()
grads = enc.bn_backward(saved, g)
tg = dict(zip(P, t_both()))
zero = [k for k in grads if k.endswith('.bias') and '.conv' in '.' + k and k != 'conv2.bias' or 'downsample.0.bias' in k]
worst = max(float((grads[k] - tg[k]).abs().max() / tg[k].abs().max()) for k in grads if k not in zero)
del saved, grads, tg, P, leaves, enc

# ---- the training step: train_step (freeze_encoder=True, freeze_bn=True) next to train_step_network on the shipped flags,
#      8 iterations, each entered with the packs dropped by the step before, as in a training loop (tools/bench_train_step.py)
import scflow_amd  # noqa: E402
from scflow_amd import optim  # noqa: E402

T = 8
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
shapes = json.load(open(os.path.join(root, 'tests', 'golden', 'state_dict_keys.json')))['shapes']
HP = dict(type='AdamW', lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


def refiner(**flags):
    cfg = scflow_amd.scflow_model_cfg(iters=T)
    cfg.update(scflow_amd.scflow_loss_cfgs(mesh_path='not/used'))
    cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='RAFTLoss', loss_weight=1.0, max_flow=400.))
    cfg.update(flags)
    m = scflow_amd.build_refiner(cfg)
    m.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
    return m.to(dev)


inp = {k: v.to(dev) for k, v in scflow_amd.make_inputs(n, H, W, seed=1).items()}
gen = torch.Generator().manual_seed(2)
ang = torch.randn(n, generator=gen) * 0.03
rz = torch.eye(3).repeat(n, 1, 1)
rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1] = ang.cos(), -ang.sin(), ang.sin(), ang.cos()
data = dict(ref_rotations=inp['ref_rotation'], ref_translations=inp['ref_translation'],
            gt_rotations=rz.to(dev) @ inp['ref_rotation'],
            gt_translations=inp['ref_translation'] + (torch.randn(n, 3, generator=gen) * torch.tensor([3., 3., 12.])).to(dev),
            labels=inp['label'], internel_k=inp['internel_k'], rendered_images=inp['render_images'],
            real_images=inp['real_images'], rendered_masks=(inp['depth'] > 0).float(), rendered_depths=inp['depth'],
            gt_masks=inp['depth'] > 0)
clip = dict(grad_clip=dict(max_norm=10.))
frozen, shipped = refiner(freeze_encoder=True, freeze_bn=True), refiner()
opt_f, opt_s = optim.build_optimizer(frozen, HP, clip), optim.build_optimizer(shipped, HP, clip, network=True)
drop = lambda m: (lambda: (m.invalidate_packed(), ())[1])      # noqa: E731
steps = alternate({'train_step': (lambda: frozen.train_step(None, opt_f, data=data), 1, drop(frozen)),
                   'train_step_network': (lambda: shipped.train_step_network(None, opt_s, data=data), 1, drop(shipped))})
last = shipped.train_step_network(None, opt_s, data=data)['log_vars']['loss']
print(json.dumps(dict(batch=n, image=[H, W], iters=T, train_step_us=steps['train_step'],
                      train_step_network_us=steps['train_step_network'], loss_finite=bool(last == last and abs(last) < 1e30),
                      ops_us=ops_us, floor_fraction=floor, hip_us=res['hip'],
                      hip_forward_us=res['hip_forward'], eval_forward_us=res['eval_forward'], torch_us=res['torch'],
                      torch_backward_us=res['torch_backward'], worst_gradient_difference_to_torch=worst)))
