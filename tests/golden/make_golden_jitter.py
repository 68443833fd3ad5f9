"""DEV-ONLY: writes tests/golden/pose_jitter.npz from the reference's own PoseJitter (datasets/pipelines/jitter.py),
imported unmodified through _refshim.  The class's constructor is bypassed (it cannot run with add_limit set:
``mesh_vertices`` is read before assignment, jitter.py:45) and ``np.random.normal`` is patched to replay the draws of the
restatement (tests/test_patches_train_host.py: hash(seed, sample id, JITTER, 8 try + i)), so that the real class pins the
Euler order, the limits, the first-accepted-try rule and the swapped error names.  The four distributions are chosen
distinct so that a replayed call is recognised by its (loc, scale).

    python tests/golden/make_golden_jitter.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refshim  # noqa: E402

_refshim.install()
for _name in ('datasets', 'datasets.pipelines'):
    _pkg = types.ModuleType(_name)
    _pkg.__path__ = [_refshim.REFERENCE_ROOT + '/' + _name.replace('.', '/')]
    sys.modules[_name] = _pkg

from datasets.pipelines.jitter import PoseJitter  # noqa: E402
from scipy.spatial.transform import Rotation  # noqa: E402

import test_patches_train_host as H  # noqa: E402
from scflow_amd.mesh import icosphere  # noqa: E402

SEED = 17
CFG = dict(jitter_angle_dis=(0.5, 15.), jitter_x_dis=(1., 14.), jitter_y_dis=(-2., 13.), jitter_z_dis=(3., 50.),
           angle_limit=25., translation_limit=70., add_limit=0.6)


class Replay:
    """np.random.normal(loc, scale) -> loc + scale * z of the restatement's current try."""

    def __init__(self, sample_id):
        self.sample_id, self.t, self.angles, self.last = sample_id, -1, 3, 'z'
        self.kinds = {tuple(CFG['jitter_angle_dis']): 'a', tuple(CFG['jitter_x_dis']): 'x', tuple(CFG['jitter_y_dis']): 'y',
                      tuple(CFG['jitter_z_dis']): 'z'}

    def __call__(self, loc=0.0, scale=1.0, size=None):
        assert size is None
        kind = self.kinds[(float(loc), float(scale))]
        if kind == 'a':
            if self.angles == 3 or self.last != 'a':
                self.t, self.angles = self.t + 1, 0
            i = self.angles
            self.angles += 1
        else:
            i = 3 + 'xyz'.index(kind)
        self.last = kind
        return loc + scale * float(H.rng_normal64(SEED, self.sample_id, H.JITTER, self.t * 8 + i))


def main():
    n = 8
    g = np.random.default_rng(5)
    R = Rotation.random(n, random_state=6).as_matrix().astype(np.float32)
    t = np.stack([g.uniform(-80, 80, n), g.uniform(-60, 60, n), g.uniform(300, 900, n)], 1).astype(np.float32)
    labels = np.array([0, 1, 0, 1, 1, 0, 0, 1])
    verts = [icosphere(2, 40.0)[0].astype(np.float32), icosphere(1, 25.0)[0].astype(np.float32)]
    diam = [80.0, 50.0]
    ids = np.array([1, 2, 3, 50, 2 ** 35, 7, 8, 9], np.int64)

    inst = object.__new__(PoseJitter)                          # the constructor cannot run with add_limit set
    inst.jitter_angle_dis, inst.jitter_x_dis = CFG['jitter_angle_dis'], CFG['jitter_x_dis']
    inst.jitter_y_dis, inst.jitter_z_dis = CFG['jitter_y_dis'], CFG['jitter_z_dis']
    inst.jitter_pose_field = ['gt_rotations', 'gt_translations']
    inst.jittered_pose_field = ['ref_rotations', 'ref_translations']
    inst.angle_limit, inst.translation_limit, inst.add_limit = CFG['angle_limit'], CFG['translation_limit'], CFG['add_limit']
    inst.mesh_vertices, inst.mesh_diameters = verts, diam

    tries, state = [], dict(i=0)
    real_jitter = PoseJitter.jitter
    real_normal = np.random.normal

    def jitter(rotation, translation, label):
        replay = Replay(ids[state['i']])
        np.random.normal = replay
        try:
            out = real_jitter(inst, rotation, translation, label)
        finally:
            np.random.normal = real_normal
        tries.append(replay.t + 1)
        state['i'] += 1
        return out

    inst.jitter = jitter
    results = inst(dict(gt_rotations=R, gt_translations=t, labels=labels, k=np.eye(3, dtype=np.float32)))
    out = dict(R=R, t=t, labels=labels, verts0=verts[0], verts1=verts[1], diam=np.array(diam), ids=ids, seed=np.int64(SEED),
               tries=np.array(tries), ref_rotations=np.asarray(results['ref_rotations']),
               ref_translations=np.asarray(results['ref_translations']),
               init_add_error=np.asarray(results['init_add_error'], np.float64),
               init_rot_error=np.asarray(results['init_rot_error'], np.float64),
               init_trans_error=np.asarray(results['init_trans_error'], np.float64))
    for k, v in CFG.items():
        out['cfg_' + k] = np.asarray(v, np.float64)
    np.savez_compressed(os.path.join(HERE, 'pose_jitter.npz'), **out)
    print('tries', tries, 'rot_error (= |noise|)', out['init_rot_error'])


if __name__ == '__main__':
    main()
