"""bench.py's N > 1 path without a GPU: the self-spawn command line, the process-group default, the build stamp."""
import argparse
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spawn_ranks_builds_the_torchrun_command(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen['cmd'], seen['env'] = cmd, env
        return 7
    monkeypatch.setattr('subprocess.call', fake_call)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '20', '--warmup', '5', '--same-device'])
    rc = bench.spawn_ranks(argparse.Namespace(gpus=2))
    cmd = seen['cmd']
    assert rc == 7                                                   # the parent exits with the children's code
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nnodes=1' in cmd and '--nproc-per-node=2' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'        # the container hostname may not resolve
    assert int(cmd[cmd.index('--master-port') + 1]) > 0
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:] == ['--gpus', '2', '--steps', '20', '--warmup', '5', '--same-device']     # the ranks get the same arguments
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0' and seen['env']['MASTER_ADDR'] == '127.0.0.1'


def test_only_rank_zero_prints_and_gloo_is_the_default():
    """The one JSON line is printed under `if rank == 0:` and the process group defaults to gloo (north_star: no RCCL on this
    path; the group carries a barrier and two scalar reductions)."""
    src = open(os.path.join(ROOT, 'bench.py')).read()
    assert src.count('print(json.dumps(out))') == 1
    head, tail = src.split('print(json.dumps(out))')
    guard = head.rstrip().splitlines()
    assert any(l.strip() == 'if rank == 0:' for l in guard)
    assert "add_argument('--dist-backend', default='gloo'" in src
    assert 'GRAFT_REPO_ROOT' not in src                              # no driver-detecting switch in the measurement script


def test_usable_cores_and_build_id():
    sys.path.insert(0, ROOT)
    import bench
    from farms_mujoco_amd import _lib
    n = bench.usable_cores()
    assert 1 <= n <= (os.cpu_count() or 1)
    b = _lib.build_id()
    assert len(b) == 16 and b == _lib.build_id()


def _fake_sim(n_envs, nq, buffer_size, sim_iteration, seed):
    """The fields dump_outputs reads, as CPU tensors: physics.data, the task's counters and its ring of sensor rows."""
    import torch
    from types import SimpleNamespace as NS
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    data = NS(qpos=r(n_envs, nq), qvel=r(n_envs, nq - 1), qacc=r(n_envs, nq - 1), ctrl=r(n_envs, 3), time=r(n_envs),
              xpos=r(n_envs, 5, 3), xquat=r(n_envs, 5, 4), xipos=r(n_envs, 5, 3), sensordata=r(n_envs, 7))
    sensors = NS(links=NS(names=['a', 'b'], array=r(buffer_size, n_envs, 2, 20)), joints=NS(names=['j'], array=r(buffer_size, n_envs, 1, 12)),
                 xfrc=NS(names=['a', 'b'], array=r(buffer_size, n_envs, 2, 6)), contacts=NS(names=[], array=r(buffer_size, n_envs, 0, 12)))
    task = NS(sim_iteration=sim_iteration, substeps=1, buffer_size=buffer_size, data=NS(sensors=sensors))
    return NS(physics=NS(data=data, n_envs=n_envs), task=task)


def test_dump_outputs_writes_the_last_step(tmp_path):
    """--dump-outputs: physics.data and the ring row of the launch's last iteration, float32, one .npy per field and bucket."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    sims = [_fake_sim(6, 4, 10, 23, 0), _fake_sim(5, 3, 10, 23, 1)]
    bench.dump_outputs(sims, str(tmp_path))
    for i, s in enumerate(sims):
        q = np.load(tmp_path/f'bucket{i}_qpos.npy')
        assert q.dtype == np.float32 and np.array_equal(q, s.physics.data.qpos.numpy())
        assert np.array_equal(np.load(tmp_path/f'bucket{i}_links.npy'), s.task.data.sensors.links.array[2].numpy())     # iteration 22 -> row 2
        assert not (tmp_path/f'bucket{i}_contacts.npy').exists() and not (tmp_path/f'bucket{i}_env_index.npy').exists()


def test_dump_outputs_samples_envs_over_the_limit(tmp_path):
    """Over the size limit every array keeps the same seeded sample of envs, the same from run to run, and stays within it."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    limit = 20000
    sim = _fake_sim(64, 4, 3, 3, 0)
    for d in ('a', 'b'):
        bench.dump_outputs([sim], str(tmp_path/d), limit=limit)
    files = sorted(os.listdir(tmp_path/'a'))
    assert files == sorted(os.listdir(tmp_path/'b')) and 'env_index.npy' in files
    idx = np.load(tmp_path/'a'/'env_index.npy').astype(int)
    assert 1 <= idx.size < 64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path/'a'/'xquat.npy'), sim.physics.data.xquat.numpy()[idx])
    assert np.array_equal(np.load(tmp_path/'a'/'xfrc.npy'), sim.task.data.sensors.xfrc.array[2].numpy()[idx])
    assert sum(np.load(tmp_path/'a'/f).nbytes for f in files) <= limit
    for f in files:
        assert np.array_equal(np.load(tmp_path/'a'/f), np.load(tmp_path/'b'/f))
