"""Generate ``bn_train_grads.npz``: the reference's own backward through its whole network with BatchNorm on the
statistics of the batch -- ``.backward()`` on the total its own ``SCFlowRefiner.loss`` returns, executed unmodified from the
reference checkout on the CPU under the import shim and the ``knn_points`` stand-in of ``make_golden_loss.py``, the model
in ``train()`` mode as the shipped recipe trains it (``freeze_bn=False``).

    python tests/golden/make_golden_bn_train.py

The case, the seeds and everything that is not the reference's are ``make_golden_network_grad.py``'s (``refiner_loss.npz``'s
case: N = 3, 256 x 256, T = 3, ``fill_state_dict`` weights, the shared InstanceNorm feature encoder), with the pose loss of
the gradient tests' models (``RAFT_POSE_LOSS`` of tests/test_chain_grad_host.py).

Stored as float32: the loss total, the 62 ``context.*`` and the 32 ``render_encoder.*`` gradients thinned by
``golden_pick`` of tests/test_context_grad_host.py, and the 15 x 2 running statistics after the forward.  The same graph is
then run once more in float64 (``model.double()``, the inputs in float64), and ``distance.<group>``, the largest
|fp32 - float64| / largest |float64| entry over the tensors of a group (``context``, ``render_encoder``, ``running``, and
``loss`` relative to itself), is stored next to them with every tensor's ``scale.<name>`` (its largest float64 entry): the GPU test allows three times that distance.  It is measured here,
on the CPU, between the reference's two evaluations, never against the code under test.  Inputs and weights are
regenerated from the seeds by the test.  The file holds recorded results only."""
import os
import runpy
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_loss as G  # noqa: E402  (installs the shim and the knn_points stand-in)

import test_chain_grad_host as CH  # noqa: E402
import test_context_grad_host as XH  # noqa: E402

H = G.H


def run(dtype, case, weight_seed):
    """``case``: H.refiner_loss_case(...), made by the caller under the default dtype its generators were written for"""
    cfg = dict(runpy.run_path(G._refshim.REFERENCE_ROOT + '/configs/refine_models/scflow.py')['model'])
    cfg['renderer'] = None
    assert not cfg['freeze_bn'] and not cfg.get('freeze_encoder') and not cfg.get('seperate_encoder')
    cfg['pose_loss_cfg'] = dict(CH.RAFT_POSE_LOSS)
    model = G.build_from_cfg(cfg, G.REFINERS)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(G.fill_state_dict(shapes, seed=weight_seed), strict=True)
    if dtype == torch.float64:
        model.double()
    model.train()                                                    # BatchNorm takes the statistics of the batch
    assert model.context.training and model.real_encoder is model.render_encoder
    model.decoder.iters = H.REFINER_ITERS
    data = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in H.refiner_data(case).items()}
    model.format_data_train_sup = lambda data_batch: data
    model.add_vis_images = lambda **kw: None
    data_batch = dict(img_metas=[dict(scale_factor=np.repeat(case['scale'][:, None], 4, axis=1))])
    loss = model.loss(data_batch)[0]
    loss.backward()
    out = {'loss': loss.detach().double().numpy()}
    for group in ('context', 'render_encoder'):
        for k, v in getattr(model, group).named_parameters():
            out[f'{group}.{k}'] = v.grad.double().numpy()
    for k, v in model.context.state_dict().items():
        if 'running_' in k:
            out[f'running.{k}'] = v.double().numpy()
        elif k.endswith('num_batches_tracked'):
            assert int(v) == 1
    return out


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    seeds = CH.FIXTURE_SEEDS
    case = H.refiner_loss_case(seeds['input_seed'], seeds['case_seed'])
    f32 = run(torch.float32, case, seeds['weight_seed'])
    # the reference pins fp32 in places (``.float()`` on the lookup's grid and output, default-dtype constants): for the
    # float64 evaluation of the same graph those calls are made to keep float64, here, in this process only
    to_float, new_zeros = torch.Tensor.float, torch.Tensor.new_zeros
    wide = lambda k: dict(k, dtype=torch.float64) if k.get('dtype') == torch.float32 else k      # noqa: E731
    torch.set_default_dtype(torch.float64)
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.Tensor.new_zeros = lambda self, *a, **k: new_zeros(self, *a, **wide(k))
    try:
        f64 = run(torch.float64, case, seeds['weight_seed'])
    finally:
        torch.Tensor.float, torch.Tensor.new_zeros = to_float, new_zeros
        torch.set_default_dtype(torch.float32)
    assert sorted(f32) == sorted(f64)
    assert sum(k.startswith('context.') for k in f32) == 62 and sum(k.startswith('running.') for k in f32) == 30
    arrays = dict(iters=np.int32(H.REFINER_ITERS), **{k: np.int32(v) for k, v in seeds.items()})
    dist = {}
    for k, v in f32.items():
        group = k.split('.', 1)[0]
        scale = np.abs(f64[k]).max()
        # the biases in front of a norm have gradient 0 in exact arithmetic: no relative distance; the test leaves them out
        if scale > 1e-6 * max(np.abs(f64[q]).max() for q in f64 if q.startswith(group)):
            dist[group] = max(dist.get(group, 0.0), float(np.abs(v - f64[k]).max() / scale))
        arrays[k] = np.ascontiguousarray(XH.golden_pick(k, v)).astype(np.float32)
        arrays[f'scale.{k}'] = np.float64(scale)                    # the largest float64 entry of the whole tensor
    for group, d in dist.items():
        print(f'  distance.{group}: {d:.3g}')
        arrays[f'distance.{group}'] = np.float64(d)
    G.save('bn_train_grads.npz', arrays)
