"""torch.nn.SyncBatchNorm on K19's synchronised form across real ranks, as far as a one-GPU box allows: tests/syncbn_rank_worker.py is
started as child ranks that share cuda:0 over gloo (two and three ranks), and once as a single rank in an RCCL group with the exchange
forced.  The children are subprocesses started with far_amd.parallel.launch_command (never an exec); the worker bounds every
collective (init_process_group timeout) and this side bounds the run, so a rank that dies cannot leave its partner waiting."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'syncbn_rank_worker.py')
pytestmark = pytest.mark.gpu


def _launch(n_ranks, mode):
    from far_amd import parallel
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run(parallel.launch_command(n_ranks, [WORKER, '--mode', mode]), capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    print('\n'.join(ln for ln in r.stdout.splitlines() if '[deviation]' in ln))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_sharing_one_gpu_match_batchnorm_over_the_concatenated_batch(world):
    """(a) ops.bn_act_train on an nn.SyncBatchNorm, unequal shards, against float64 BatchNorm2d over the concatenated shards at K19's
    bars, running statistics bit-identical on every rank; (b) a converted ResNetFPN_8_2, one image per rank, against the plain-BatchNorm
    model on the concatenated batch: maps, summed weight gradients (1e-3 of each tensor's largest entry), the running statistics of
    all 17 layers, num_batches_tracked."""
    out = _launch(world, 'ranks')
    for part in ('operator', 'backbone'):                      # every rank ran both parts (the worker's exit code carries its assertions)
        assert sorted(re.findall(rf'\[deviation\] sync_bn ranks W={world} rank (\d+) {part}:', out)) == [str(r) for r in range(world)], out[-2000:]


def test_forced_exchange_over_rccl_at_world_size_1_returns_the_plain_bits():
    out = _launch(1, 'rccl1')
    assert out.count('[deviation] sync_bn rccl world 1: forced exchange over nccl') == 1, out[-2000:]
