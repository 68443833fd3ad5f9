"""Generate ``chain_grads.npz``: the reference's own backward through its whole decoder and loss -- ``.backward()`` on the
total its own ``SCFlowRefiner.loss`` (models/refiner/scflow_refiner.py:184-258) returns, executed unmodified from the
reference checkout on the CPU under the import shim and the ``knn_points`` stand-in of ``make_golden_loss.py`` (see
there for what is not the reference's: the stand-in, the mesh stub, ``format_data_train_sup`` replaced by the seeded
``refiner_loss_case``, ``add_vis_images`` replaced by a no-op).

    python tests/golden/make_golden_chain_grad.py

The case is ``refiner_loss.npz``'s: N = 3, 256 x 256, T = 3, ``fill_state_dict`` weights, the shipped decoder flags of
configs/refine_models/scflow.py.  Two loss variants (``VARIANTS`` of tests/test_chain_grad_host.py): 'shipped', the
config's disentangled point-matching pose loss with the first sample's class symmetric, and 'raft', the ``RAFTLoss`` pose
loss the gradient tests' ``scflow_model`` fixtures use.

No reference source is edited or copied.  The cotangents inside the graph come from hooks: a forward pre-hook on the
decoder calls ``retain_grad()`` on the hidden state and the context the refiner hands it, forward hooks on the decoder's
``corr_block``, ``encoder``, ``gru``, ``flow_pred``, ``mask_pred`` and ``pose_pred`` call it on level 0 of the pyramid (the
pooled levels' adjoints arrive folded in) and on every iteration's output of those modules.  The neighbour indices are
what the ``knn_points`` stand-in returned ((T, N, Vmax), -1 where a sample's class is not symmetric).

Stored per variant, through ``golden_pick`` of tests/test_chain_grad_host.py, as float32: the loss total, every decoder
parameter gradient (thinned), channel picks of the cotangents at h0 and the context, every 768th query map of the volume
cotangent, picks of the per-iteration cotangents at the motion features, the hidden state (complete: own heads plus the
carry), the delta flow, the mask logit and the pose head's outputs.  Inputs and weights are regenerated from the seeds
by the test.  The file holds recorded results only."""
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

H = G.H
_calls = []


def _recording_knn(p1, p2, K=1):
    out = G.knn_points(p1, p2, K)
    _calls.append(out.idx[0, :, 0].numpy().copy())
    return out


G._pm.knn_points = _recording_knn


def chain_grads(variant, input_seed, case_seed, weight_seed):
    case = H.refiner_loss_case(input_seed, case_seed)
    cfg = dict(runpy.run_path(G._refshim.REFERENCE_ROOT + '/configs/refine_models/scflow.py')['model'])
    cfg['renderer'] = None
    if variant == 'raft':
        cfg['pose_loss_cfg'] = dict(CH.RAFT_POSE_LOSS)
    else:
        cfg['pose_loss_cfg'] = dict(cfg['pose_loss_cfg'])
        cfg['pose_loss_cfg']['loss_func_cfg'] = dict(cfg['pose_loss_cfg']['loss_func_cfg'], mesh_path=tempfile.mkdtemp(),
                                                     symmetry_types=case['symmetry_types'], mesh_diameter=case['diameter'])
    model = G.build_from_cfg(cfg, G.REFINERS).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(G.fill_state_dict(shapes, seed=weight_seed), strict=True)
    dec = model.decoder
    dec.iters = T = H.REFINER_ITERS
    flags = CH.shipped_flags()
    assert all(getattr(dec, k) == flags[k] for k in ('detach_flow', 'detach_mask', 'detach_pose', 'detach_depth_for_xy',
                                                     'mask_flow', 'mask_corr'))
    if variant != 'raft':
        model.pose_loss_func.loss_func.meshes = [torch.from_numpy(v) for v in case['verts']]
    data = H.refiner_data(case)
    model.format_data_train_sup = lambda data_batch: data
    model.add_vis_images = lambda **kw: None
    data_batch = dict(img_metas=[dict(scale_factor=np.repeat(case['scale'][:, None], 4, axis=1))])

    kept = dict(x=[], hv=[], d_flow=[], logit=[], d_rot=[], d_trans=[])

    def keep(*names):
        def hook(module, args, out):
            for name, o in zip(names, out if isinstance(out, (tuple, list)) else (out,)):
                o.retain_grad()
                kept[name].append(o)
        return hook

    def decoder_inputs(module, args):
        args[2].retain_grad()
        args[3].retain_grad()
        kept['h0'], kept['context'] = args[2], args[3]

    def pyramid(module, args, out):
        out[0].retain_grad()
        kept['pyramid0'] = out[0]

    dec.register_forward_pre_hook(decoder_inputs)
    dec.corr_block.register_forward_hook(pyramid)
    dec.encoder.register_forward_hook(keep('x'))
    dec.gru.register_forward_hook(keep('hv'))
    dec.flow_pred.register_forward_hook(keep('d_flow'))
    dec.mask_pred.register_forward_hook(keep('logit'))
    dec.pose_pred.register_forward_hook(keep('d_rot', 'd_trans'))
    _calls.clear()
    loss = model.loss(data_batch)[0]
    loss.backward()
    assert all(len(kept[k]) == T for k in ('x', 'hv', 'd_flow', 'logit', 'd_rot', 'd_trans'))
    got = {'decoder.' + k: v.grad.numpy() for k, v in dec.named_parameters()}
    got['initial_hidden'], got['context'] = kept['h0'].grad.numpy(), kept['context'].grad.numpy()
    h, w = kept['pyramid0'].shape[-2:]
    got['correlation'] = kept['pyramid0'].grad.numpy().reshape(-1, h, w)
    for key, name in (('motion_features', 'x'), ('hidden_total', 'hv'), ('delta_flow_preds', 'd_flow'), ('mask_logits', 'logit'),
                      ('delta_rotation_preds', 'd_rot'), ('delta_translation_preds', 'd_trans')):
        for t in range(T):
            got[f'{key}.{t}'] = kept[name][t].grad.numpy()
    out = {f'{variant}.{k}': np.ascontiguousarray(CH.golden_pick(k, v)).astype(np.float32) for k, v in got.items()}
    assert all(np.abs(v).max() > 0 for v in out.values()), [k for k, v in out.items() if not np.abs(v).max() > 0]
    out[f'{variant}.loss'] = np.float32(loss.item())
    if variant != 'raft':
        nn = np.full((T, H.REFINER_N, max(len(v) for v in case['verts'])), -1, dtype=np.int32)
        calls = iter(_calls)
        for t in range(T):
            for n, c in enumerate(case['labels']):
                if f'cls_{int(c) + 1}' in case['symmetry_types']:
                    idx = next(calls)
                    nn[t, n, :len(idx)] = idx
        assert next(calls, None) is None
        out[f'{variant}.nn'] = nn
    return out


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(8)
    seeds = CH.FIXTURE_SEEDS
    arrays = dict(iters=np.int32(H.REFINER_ITERS), **{k: np.int32(v) for k, v in seeds.items()})
    for variant in CH.VARIANTS:
        arrays.update(chain_grads(variant, **seeds))
    for group in ('decoder.', 'initial', 'context', 'correlation', 'motion', 'hidden', 'delta', 'mask'):
        size = sum(v.nbytes for k, v in arrays.items() if k.split('.', 1)[-1].startswith(group))
        print(f'  {group}*: {size / 1024:.1f} KiB before compression')
    G.save('chain_grads.npz', arrays)
