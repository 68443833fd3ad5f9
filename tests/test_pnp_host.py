"""CPU: the pose step of the pose-free RAFT refiners (batched RANSAC-EPnP, scflow_amd/csrc/pnp.hip) -- the
correspondence fixture against an in-test torch restatement, mode selection, parameter validation and the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import scflow_amd
from scflow_amd import _lib, ops


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'corr_2d3d.npz'))


def _corr_restated(flow, depth, k, rot, trans, mask=None):
    """get_2d_3d_corr_by_fw_flow (models/utils/pose.py:182-200) restated in torch: per sample the pixels with
    depth > 0 (& mask), row-major, -> (source pixels, target points, object-frame points)."""
    out = []
    for i in range(len(flow)):
        m = depth[i] > 0
        if mask is not None:
            m = m & mask[i]
        ys, xs = torch.nonzero(m, as_tuple=True)
        d = depth[i][m]
        src = torch.stack([xs, ys], dim=-1).float()
        homo = torch.stack([src[:, 0], src[:, 1], torch.ones_like(src[:, 0])], dim=-1) * d[:, None]
        cam = torch.mm(torch.inverse(k[i]), homo.t()).t()
        obj = torch.mm(torch.inverse(rot[i]), (cam - trans[i][None]).t()).t()
        tgt = src + flow[i][:, ys, xs].t()
        out.append((src, tgt, obj))
    return out


@pytest.mark.parametrize('case', ['a', 'b'])
@pytest.mark.parametrize('tag', ['nomask', 'mask'])
def test_corr_restatement_matches_fixture(golden_dir, case, tag):
    g = _fixture(golden_dir)
    f = lambda k: torch.from_numpy(g[f'{case}_{k}'])      # noqa: E731
    flow = f('flow16').float() / 16
    occ = f('occ8').float() / 8
    corr = _corr_restated(flow, f('depth'), f('k'), f('rot'), f('trans'), occ > 0.5 if tag == 'mask' else None)
    assert [len(c[0]) for c in corr] == g[f'{case}_{tag}_count'].tolist()
    src = torch.cat([c[0] for c in corr])
    assert torch.equal(src, f(f'{tag}_src').float())
    step = int(g[f'{case}_{tag}_row_step'])
    torch.testing.assert_close(torch.cat([c[1] for c in corr])[::step], f(f'{tag}_pts2d'), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(torch.cat([c[2] for c in corr])[::step], f(f'{tag}_pts3d'), rtol=1e-5, atol=1e-3)
    if case == 'a' and tag == 'mask':
        assert int(g['a_mask_count'][-1]) == 0               # the empty-mask sample


def _raft(test_cfg):
    cfg = scflow_amd.raft_model_cfg(iters=2)
    cfg['test_cfg'] = dict(iters=2, **test_cfg)
    return scflow_amd.build_refiner(cfg)


def test_hip_mode_builds_and_cv2_modes_raise():
    m = _raft(dict(solve_pose_mode='hip_ransac_epnp', solve_pose_param=dict(iterationscount=50, reprojectionerror=2.0),
                   sample_points=dict(num=500, mode='topk')))
    assert type(m).__name__ == 'RAFTRefinerFlowMask'
    kw = m._pnp_kwargs()
    assert kw == dict(iterations=50, reproj_error=2.0, seed=0, sample_mode='topk', sample_num=500)
    for mode in ('ransacpnp', None, 'progressive-x', 'magic'):
        m = _raft({} if mode is None else dict(solve_pose_mode=mode))
        with pytest.raises(NotImplementedError, match='hip_ransac_epnp'):
            m.solve_pose()
    f = scflow_amd.build_refiner(dict(scflow_amd.raft_model_cfg(iters=2), type='RAFTRefinerFlow',
                                      decoder=dict(scflow_amd.raft_model_cfg()['decoder'], type='RAFTDecoder')))
    with pytest.raises(NotImplementedError):
        f.solve_pose()


def test_remap_modes():
    m = _raft(dict(solve_pose_mode='hip_ransac_epnp'))
    r, t = [torch.eye(3)[None]], [torch.zeros((1, 3))]
    assert m._remap_pose(r, t, None) == (r, t)
    assert m._remap_pose(r, t, [dict(geometry_transform_mode='adapt_intrinsic')]) == (r, t)
    with pytest.raises(NotImplementedError):
        m._remap_pose(r, t, [dict(geometry_transform_mode='target_intrinsic')])


@pytest.mark.parametrize('bad', [dict(iterations=0), dict(iterations=-3), dict(iterations=2.5),
                                 dict(reproj_error=-1.0), dict(reproj_error=float('nan')),
                                 dict(reproj_error=float('inf')), dict(sample_mode='first'),
                                 dict(sample_mode='topk', sample_num=0), dict(seed=-1)])
def test_bad_parameters_rejected(bad):
    with pytest.raises(_lib.ScflowHipError):
        ops.pnp_params(**bad)


def test_bad_parameters_rejected_by_solve_pose_before_any_launch():
    for prm in (dict(iterationscount=0), dict(reprojectionerror=-0.5)):
        m = _raft(dict(solve_pose_mode='hip_ransac_epnp', solve_pose_param=prm))
        with pytest.raises(_lib.ScflowHipError):
            m.solve_pose()


def test_cabi_symbols_version_and_host_validation():
    lib = _lib.load()
    for name in ('scf_flow_corr_2d3d', 'scf_pnp_ransac', 'scf_pnp_workspace_bytes'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.scf_version() % 100 == 3
    assert C.sizeof(_lib.PnpParams) == 24
    ok = _lib.PnpParams(100, 3.0, _lib.PNP_SAMPLE_ALL, 0, 0)
    assert lib.scf_pnp_workspace_bytes(4, 1000, C.byref(ok)) == 0
    topk = _lib.PnpParams(100, 3.0, _lib.PNP_SAMPLE_TOPK, 10, 0)
    assert lib.scf_pnp_workspace_bytes(4, 1000, C.byref(topk)) >= 4 * 1000 * 4 + 4 * 4
    for bad in (_lib.PnpParams(0, 3.0, 0, 0, 0), _lib.PnpParams(10, -1.0, 0, 0, 0),
                _lib.PnpParams(10, 3.0, 7, 0, 0), _lib.PnpParams(10, 3.0, _lib.PNP_SAMPLE_RANDOM, 0, 0)):
        assert lib.scf_pnp_workspace_bytes(4, 1000, C.byref(bad)) == -1
    # argument checks return before any launch: no device needed
    assert lib.scf_pnp_ransac(None, None, None, None, 1, 1, None, None, None, C.byref(ok),
                              None, None, None, None, None, None) == -1
    assert lib.scf_flow_corr_2d3d(None, None, None, 0.5, None, None, None, 1, 1, 1, None, None, None, None, None) == -1
