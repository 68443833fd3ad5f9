"""Generate ``network_grads.npz``: the reference's own backward through its WHOLE network -- ``.backward()`` on the total its
own ``SCFlowRefiner.loss`` (models/refiner/scflow_refiner.py:184-258) returns, executed unmodified from the reference
checkout on the CPU under the import shim and the ``knn_points`` stand-in of ``make_golden_loss.py`` -- recorded where
``make_golden_chain_grad.py`` stops: behind the correlation volume.

    python tests/golden/make_golden_network_grad.py

The case, the weights, the two loss variants and everything that is not the reference's are ``make_golden_chain_grad.py``'s
(``refiner_loss.npz``'s case: N = 3, 256 x 256, T = 3, ``fill_state_dict`` weights, shipped decoder flags; the shared
InstanceNorm feature encoder, ``freeze_encoder=False`` as configs/refine_models/scflow.py has it, ``eval()`` so the context
encoder's BatchNorm runs on its running statistics).

No reference source is edited or copied.  A forward pre-hook on the decoder calls ``retain_grad()`` on the two feature
maps the refiner hands it (``feat_render``, ``feat_real``); the encoder's parameter gradients are its ``.grad`` after the
backward: with the shared encoder the sum over both image sets.

Stored per variant as float32: the loss total, the two feature-map cotangents thinned by ``feature_pick`` of
tests/test_corr_grad_host.py and the 32 ``render_encoder.*`` gradients thinned by ``golden_pick`` of
tests/test_feature_grad_host.py.  Inputs and weights are regenerated from the seeds by the test.  The file holds
recorded results only."""
import os
import runpy
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_loss as G  # noqa: E402  (installs the shim and the knn_points stand-in)

import test_chain_grad_host as CH  # noqa: E402
import test_corr_grad_host as KH  # noqa: E402
import test_feature_grad_host as FH  # noqa: E402

H = G.H


def network_grads(variant, input_seed, case_seed, weight_seed):
    case = H.refiner_loss_case(input_seed, case_seed)
    cfg = dict(runpy.run_path(G._refshim.REFERENCE_ROOT + '/configs/refine_models/scflow.py')['model'])
    cfg['renderer'] = None
    assert not cfg.get('freeze_encoder') and not cfg.get('seperate_encoder')
    if variant == 'raft':
        cfg['pose_loss_cfg'] = dict(CH.RAFT_POSE_LOSS)
    else:
        cfg['pose_loss_cfg'] = dict(cfg['pose_loss_cfg'])
        cfg['pose_loss_cfg']['loss_func_cfg'] = dict(cfg['pose_loss_cfg']['loss_func_cfg'], mesh_path=tempfile.mkdtemp(),
                                                     symmetry_types=case['symmetry_types'], mesh_diameter=case['diameter'])
    model = G.build_from_cfg(cfg, G.REFINERS).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(G.fill_state_dict(shapes, seed=weight_seed), strict=True)
    assert model.real_encoder is model.render_encoder
    dec = model.decoder
    dec.iters = H.REFINER_ITERS
    if variant != 'raft':
        model.pose_loss_func.loss_func.meshes = [torch.from_numpy(v) for v in case['verts']]
    data = H.refiner_data(case)
    model.format_data_train_sup = lambda data_batch: data
    model.add_vis_images = lambda **kw: None
    data_batch = dict(img_metas=[dict(scale_factor=np.repeat(case['scale'][:, None], 4, axis=1))])
    kept = {}

    def decoder_inputs(module, args):
        args[0].retain_grad()
        args[1].retain_grad()
        kept['render'], kept['real'] = args[0], args[1]

    dec.register_forward_pre_hook(decoder_inputs)
    loss = model.loss(data_batch)[0]
    loss.backward()
    out = {f'{variant}.features.{k}': np.ascontiguousarray(KH.feature_pick(kept[k].grad.numpy())).astype(np.float32)
           for k in ('render', 'real')}
    params = dict(model.render_encoder.named_parameters())
    assert sorted(params) == sorted(FH.PARAM_NAMES)
    for k, v in params.items():
        out[f'{variant}.render_encoder.{k}'] = np.ascontiguousarray(FH.golden_pick(k, v.grad.numpy())).astype(np.float32)
    assert all(np.abs(v).max() > 0 for v in out.values()), [k for k, v in out.items() if not np.abs(v).max() > 0]
    out[f'{variant}.loss'] = np.float32(loss.item())
    return out


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    seeds = CH.FIXTURE_SEEDS
    arrays = dict(iters=np.int32(H.REFINER_ITERS), **{k: np.int32(v) for k, v in seeds.items()})
    for variant in CH.VARIANTS:
        arrays.update(network_grads(variant, **seeds))
    for group in ('features', 'render_encoder'):
        size = sum(v.nbytes for k, v in arrays.items() if k.split('.', 1)[-1].startswith(group))
        print(f'  {group}*: {size / 1024:.1f} KiB before compression')
    G.save('network_grads.npz', arrays)
