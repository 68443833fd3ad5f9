"""bench.py --gpus N must start N ranks itself.  CPU check: the same launcher,
process group, barrier / max-over-ranks timing and pose gather, with a CPU stand-in step over gloo
(``--standin``); the JSON line must report n_gpus == 2 and one entry per rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=180):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_self_launches_two_ranks():
    r = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '4', '--standin',
              '--min-seconds', '0.2', '--min-warmup-seconds', '0.05'])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout          # rank 0 prints exactly one JSON line
    out = json.loads(lines[0])
    assert out['standin'] is True and 'SELF-TEST' in out['metric']
    assert out['n_gpus'] == 2 and out['collective_world_size'] == 2
    assert [e['rank'] for e in out['ranks']] == [0, 1]
    assert len({e['pid'] for e in out['ranks']}) == 2          # two processes
    assert out['steps'] == 2 and out['config']['global_batch'] == 8
    assert out['timing']['blocks'] >= 1 and out['timing']['timed_seconds'] >= 0.2
    assert out['scaling'] == 'weak' and out['value'] > 0


def test_bench_refuses_mismatched_world():
    # a torchrun-style environment whose WORLD_SIZE disagrees with --gpus must not produce a line
    r = _run(['--gpus', '2', '--standin', '--steps', '1', '--warmup', '0'],
             env_extra={'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode == 2
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith('{')]


def test_bench_refuses_without_gpus():
    # no GPU in the CPU container: --gpus 2 (real step) must refuse instead of running 1 rank
    import torch
    if torch.cuda.device_count() >= 2:
        return
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0'])
    assert r.returncode == 2 and 'refusing' in r.stderr


def test_secondary_measurements_are_opt_in():
    """a plain run does only what its headline needs; batch1 / config4 / cpu_baseline / roofline_conv come with --full,
    and --alt (whose loops always ran beside those) implies it."""
    sys.path.insert(0, ROOT)
    import bench
    plain = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not plain.full and not plain.alt
    assert bench.parse_args(['--full']).full and not bench.parse_args(['--full']).alt
    assert bench.parse_args(['--alt']).full


def test_counter_summaries_are_bound_to_the_kernel_sources():
    """bench.py attaches profiles/lookup_pmc.json / *_mfma_pmc.json (separate rocprofv3 --pmc passes) only when they
    record the hashes of today's kernel sources: no hashes -> stale; one changed file -> stale, named."""
    sys.path.insert(0, ROOT)
    import bench
    now = bench.kernel_source_hashes(bench.LOOKUP_SOURCES)
    assert set(now) == set(bench.LOOKUP_SOURCES) and all(v and len(v) == 16 for v in now.values())
    assert bench._fresh({'kernel_source_hashes': dict(now)}, bench.LOOKUP_SOURCES) == (True, None)
    ok, why = bench._fresh({'traffic_bytes_per_launch': 1}, bench.LOOKUP_SOURCES)
    assert not ok and 'no kernel_source_hashes' in why
    other = dict(now, **{'corr_lookup.hip': '0' * 16})
    ok, why = bench._fresh({'kernel_source_hashes': other}, bench.LOOKUP_SOURCES)
    assert not ok and 'corr_lookup.hip' in why
    # whatever is committed under profiles/ is either fresh or refused -- never silently attached
    p = os.path.join(ROOT, 'profiles', 'lookup_pmc.json')
    if os.path.exists(p):
        d = json.load(open(p))
        ok, why = bench._fresh(d, bench.LOOKUP_SOURCES)
        assert ok or why


def test_bench_times_exactly_steps_and_dumps_outputs(tmp_path):
    """--steps K is the number of timed steps (one block by default); --dump-outputs writes the last timed step's
    outputs as float32 .npy, and the same arguments give the same files."""
    import numpy as np
    dumps = []
    for run in range(2):
        d = os.path.join(tmp_path, f'run{run}')
        r = _run(['--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4', '--standin',
                  '--min-warmup-seconds', '0', '--dump-outputs', d])
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
        assert out['steps'] == 3 and out['timing']['blocks'] == 1 and out['timing']['timed_steps'] == 3
        assert out['timing']['warmup_steps_run'] == 1
        assert set(out['dumped_outputs']['arrays']) == {'rotation', 'translation'}
        dumps.append({n: np.load(os.path.join(d, n + '.npy')) for n in ('rotation', 'translation')})
    assert dumps[0]['rotation'].shape == (4, 3, 3) and dumps[0]['translation'].shape == (4, 3)
    for n, a in dumps[0].items():
        assert a.dtype == np.float32 and np.array_equal(a, dumps[1][n])


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_step(tmp_path):
    """the dumped arrays are get_pose's outputs on bench.py's seeded batch (rank 0: seed 1000), bit for bit."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    d = os.path.join(tmp_path, 'dump')
    r = _run(['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '4', '--min-warmup-seconds', '0',
              '--no-batch1', '--no-config4', '--no-cpu-baseline', '--dump-outputs', d], timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert out['timing']['timed_steps'] == 2
    arrays = out['dumped_outputs']['arrays']
    assert set(arrays) == set(bench.GET_POSE_OUTPUTS)
    model, _ = bench.build_model(8, 'cuda:0')
    outs = bench.run_step(model, bench.make_batch(4, 1000, 'cuda:0'))
    total = 0
    for name, val in zip(bench.GET_POSE_OUTPUTS, outs):
        want = torch.stack([v for v in val]).float().cpu().numpy()
        got = np.load(os.path.join(d, name + '.npy'))
        total += got.nbytes
        assert got.dtype == np.float32 and list(want.shape) == arrays[name]['shape']
        if 'sample' in arrays[name]:
            pos = np.sort(np.random.default_rng(0).choice(want.size, bench.DUMP_MAX_ELEMS, replace=False))
            want = want.reshape(-1)[pos]
        assert np.array_equal(got, want), name
    assert total <= 64e6
