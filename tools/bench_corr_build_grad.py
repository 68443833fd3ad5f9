"""Micro-benchmark of the correlation-build backward (``ops.corr_build_grad``: ``scf_corr_build_grad``, two launches) at the
bench workload N = 32, C = 256, 32 x 32 maps, random operands, and of the rung it completes.  Device events bracket a
window of calls; every column is warmed up first; the columns alternate inside one process, and each figure is the median
of the windows with their 10 % and 90 % points.
    python tools/bench_corr_build_grad.py [N]   -> one JSON line
``both_us`` is one ``ops.corr_build_grad`` call into preallocated outputs: the two launches back to back.  ``g_feat1_us``
is the FIRST launch alone, from a launch-bound timer of the library (``scf_timer_*``); ``g_feat2_us`` is the difference of
the two medians.  ``mfma_peak_fraction``: executed flops (2 x 128 x 128 x the padded contraction per block) over time over
the 157.3 TFLOP/s fp32 MFMA peak of DESIGN.md.  ``torch_us`` is the same two gradients by torch autograd of ``einsum`` on
the same GPU (forward + backward, what they cost a user of torch), ``torch_bmm_us`` the two ``bmm`` calls that ARE the
adjoint, with the scale.  ``network_us`` / ``context_us``: ``loss_and_network_grads()`` next to ``loss_and_context_grads()``
on the refiner of tools/bench_train_step.py: N samples of 256 x 256, 8 iterations, seeded weights, RAFTLoss pose loss.
The events bracket the Python calls, so every HIP figure includes the binding's host path.  The gradients of the two
implementations are compared at the end, relative to the largest entry (a plausibility figure; the kernel is held to
float64 by tests/test_gpu_corr_grad.py)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import scflow_amd  # noqa: E402
from scflow_amd import _lib, ops  # noqa: E402

dev = 'cuda:0'
PEAK = 157.3e12


def window(fn, inner, args=()):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn(*args)
    e.record()
    return s, e


def alternate(columns, n=11):
    """columns: name -> (fn, inner); every repetition times each column once, in turn"""
    for fn, _ in columns.values():
        for _ in range(2):
            fn()
    evs = {k: [] for k in columns}
    for _ in range(n):
        for k, (fn, inner) in columns.items():
            evs[k].append((window(fn, inner), inner))
    torch.cuda.synchronize()
    return {k: stats([s.elapsed_time(e) / inner * 1e3 for (s, e), inner in lst]) for k, lst in evs.items()}


def stats(us):
    ts, n = sorted(us), len(us)
    return dict(median=round(ts[n // 2], 1), p10=round(ts[n // 10], 1), p90=round(ts[n - 1 - n // 10], 1))


n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
c, h, w = 256, 32, 32
hw = h * w
torch.manual_seed(0)
g_vol = torch.randn(n * hw, h, w, device=dev)
f1, f2 = torch.randn(n, c, h, w, device=dev), torch.randn(n, c, h, w, device=dev)
both = torch.empty(2 * n, c, h, w, device=dev)
out = (both[:n], both[n:])
scale = 1.0 / c ** 0.5


def hip():
    return ops.corr_build_grad(g_vol, f1, f2, out=out)


def torch_autograd():
    a, b = f1.view(n, c, hw).requires_grad_(), f2.view(n, c, hw).requires_grad_()
    lvl0 = torch.einsum('nci,ncj->nij', a, b) * scale
    return torch.autograd.grad(lvl0, (a, b), g_vol.view(n, hw, hw))


def torch_bmm():
    G = g_vol.view(n, hw, hw)
    return torch.bmm(f2.view(n, c, hw), G.transpose(1, 2)) * scale, torch.bmm(f1.view(n, c, hw), G) * scale


# ---- the first launch alone: a launch-bound timer per call
lib = _lib.load()
pool = ops._TimerPool(16)
for i in range(13):
    tm = pool.take()
    lib.scf_timer_arm(tm)
    hip()
    lib.scf_timer_arm(None)
torch.cuda.synchronize()
first = stats(pool.read()[2:])
pool.destroy()

# ---- the rung on the refiner
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
shapes = json.load(open(os.path.join(root, 'tests', 'golden', 'state_dict_keys.json')))['shapes']
cfg = scflow_amd.scflow_model_cfg(iters=8)
cfg.update(scflow_amd.scflow_loss_cfgs(mesh_path='not/used'))
cfg['pose_loss_cfg'] = dict(type='SequenceLoss', gamma=0.8, loss_func_cfg=dict(type='RAFTLoss', loss_weight=1.0, max_flow=400.))
model = scflow_amd.build_refiner(cfg)
model.load_state_dict(scflow_amd.fill_state_dict(shapes, seed=0), strict=True)
model = model.to(dev)
inp = {k: v.to(dev) for k, v in scflow_amd.make_inputs(n, 256, 256, seed=1).items()}
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

cols = {'both': (hip, 4), 'torch': (torch_autograd, 4), 'torch_bmm': (torch_bmm, 4),
        'network': (lambda: model.loss_and_network_grads(None, data=data), 1),
        'context': (lambda: model.loss_and_context_grads(None, data=data), 1)}
res = alternate(cols)
mine, theirs = hip(), torch_autograd()
worst = max(float((a.view(n, c, hw) - b).abs().max() / b.abs().max()) for a, b in zip(mine, theirs))
flops = 2.0 * n * (-(-c // 128) * 128) * (-(-hw // 128) * 128) * (-(-hw // 32) * 32)        # executed, one product
second = round(res['both']['median'] - first['median'], 1)
print(json.dumps(dict(
    batch=n, channels=c, map=[h, w], both_us=res['both'], g_feat1_us=first, g_feat2_us_by_difference=second,
    mfma_peak_fraction=dict(both=round(2 * flops / (res['both']['median'] * 1e-6) / PEAK, 3),
                            g_feat1=round(flops / (first['median'] * 1e-6) / PEAK, 3),
                            g_feat2=round(flops / (second * 1e-6) / PEAK, 3)),
    torch_us=res['torch'], torch_bmm_us=res['torch_bmm'], network_us=res['network'], context_us=res['context'],
    worst_gradient_difference_to_torch=worst)))
