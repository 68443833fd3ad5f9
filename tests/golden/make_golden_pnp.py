"""Generate ``corr_2d3d.npz``: the reference's own ``get_2d_3d_corr_by_fw_flow`` (models/utils/pose.py:182-200, with
``cal_3d_2d_corr`` and ``lift_2d_to_3d``), executed unmodified from the reference checkout on CPU through the same
import shim as ``make_golden.py`` (pure torch; only import-only stubs are involved).

    python tests/golden/make_golden_pnp.py

Cases (each stored with and without an occlusion mask, mask = occlusion > 0.5 as in
BaseFlowRefiner.solve_pose, base_flow_refiner.py:107-111):
* ``a``: two samples at 256 x 256 (``make_inputs`` disc depth); the second sample's occlusion map is all zero,
  so its masked correspondence set is empty;
* ``b``: one ragged 37 x 53 sample.
Flow and occlusion are quantised and stored as integers (``flow16`` = 16 * flow, ``occ8`` = 8 * occlusion, both
exact) so that the file stays small.  Per case and mask variant the file holds the per-sample counts, the source
pixel (x, y) of every correspondence (the full order) and, for every ``*_row_step``-th row (every row with the mask, every
4th row without it), the target point (x + flow) and the object-frame point.
"""
import os
import sys

os.environ.setdefault('MKL_CBWR', 'COMPATIBLE')

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

_refshim.install()

from scflow_amd.synthetic import make_inputs  # noqa: E402

from models.utils.pose import get_2d_3d_corr_by_fw_flow  # noqa: E402

STUBS = 'reference source, import stubs only'


def case(n, h, w, seed, empty_last):
    inp = make_inputs(n, h, w, seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    flow = torch.round(torch.randn((n, 2, h, w), generator=g) * 3 * 16) / 16
    flow = flow * (inp['depth'] > 0)[:, None]              # only foreground flow is read: zeros compress
    occ = torch.round(torch.rand((n, h, w), generator=g) * 8) / 8
    if empty_last:
        occ[-1] = 0.
    out = dict(flow16=(flow * 16).to(torch.int16), depth=inp['depth'], k=inp['internel_k'],
               rot=inp['ref_rotation'], trans=inp['ref_translation'], occ8=(occ * 8).to(torch.uint8))
    for tag, mask in (('nomask', None), ('mask', occ > 0.5)):
        corr = get_2d_3d_corr_by_fw_flow(flow, inp['depth'], inp['ref_rotation'], inp['ref_translation'],
                                         inp['internel_k'], mask)
        out[f'{tag}_count'] = torch.tensor([len(c[0]) for c in corr], dtype=torch.int32)
        out[f'{tag}_src'] = torch.cat([c[0] for c in corr]).to(torch.int16)       # integer pixel coordinates
        src = torch.cat([c[0] for c in corr])
        rows = torch.arange(0, len(src), 1 if mask is not None else 4)
        out[f'{tag}_row_step'] = torch.tensor(1 if mask is not None else 4)
        out[f'{tag}_pts2d'] = torch.cat([c[1] for c in corr])[rows]
        out[f'{tag}_pts3d'] = torch.cat([c[2] for c in corr])[rows]
    return out


@torch.no_grad()
def main():
    torch.set_num_threads(8)
    arrays = {}
    for name, (n, h, w, seed, empty) in {'a': (2, 256, 256, 41, True), 'b': (1, 37, 53, 42, False)}.items():
        for k, v in case(n, h, w, seed, empty).items():
            arrays[f'{name}_{k}'] = v.numpy()
    arrays['pinned_under'] = np.asarray(STUBS)
    path = os.path.join(HERE, 'corr_2d3d.npz')
    np.savez_compressed(path, **arrays)
    print(f'corr_2d3d.npz: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
