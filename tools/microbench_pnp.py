"""Micro-benchmark of the batched RANSAC-EPnP solve (``scf_pnp_ransac``, HIP-event timed) at batch 1 / 8 / 32 with
~20 k exact correspondences per sample (the synthetic disc at 256 x 256), 100 hypotheses, 3 px threshold; the
correspondence extraction (``scf_flow_corr_2d3d``) is timed on the same inputs.
    python tools/microbench_pnp.py [N ...]      -> one JSON line per batch size (median / min microseconds)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from scflow_amd import ops  # noqa: E402
from scflow_amd.synthetic import make_inputs  # noqa: E402

dev = 'cuda:0'


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    evs = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3


for n in [int(a) for a in sys.argv[1:]] or [1, 8, 32]:
    inp = make_inputs(n, 256, 256, seed=3)
    d = {k: inp[k].to(dev) for k in ('depth', 'internel_k', 'ref_rotation', 'ref_translation')}
    tr = d['ref_translation'].clone()
    tr[:, 0] += 5.
    flow = ops.reproject_flow(d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation'],
                              d['ref_rotation'], tr)
    args = (flow, d['depth'], d['internel_k'], d['ref_rotation'], d['ref_translation'])
    pts2d, pts3d, conf, count = ops.flow_corr_2d3d(*args)
    corr_us = timeit(lambda: ops.flow_corr_2d3d(*args))
    ransac_us = timeit(lambda: ops.pnp_ransac(pts2d, pts3d, count, d['internel_k'], d['ref_rotation'],
                                              d['ref_translation']))
    _, _, ok, inl = ops.pnp_ransac(pts2d, pts3d, count, d['internel_k'], d['ref_rotation'], d['ref_translation'])
    print(json.dumps(dict(batch=n, points_per_sample=int(count.float().mean()), hypotheses=100,
                          pnp_ransac_us=dict(median=round(ransac_us[0], 1), min=round(ransac_us[1], 1)),
                          flow_corr_2d3d_us=dict(median=round(corr_us[0], 1), min=round(corr_us[1], 1)),
                          ok=int(ok.sum()), inliers_min=int(inl.min()))))
