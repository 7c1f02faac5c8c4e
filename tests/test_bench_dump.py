"""bench.py --dump-outputs (CPU): which entries of a step's batch are written, in which dtype, how a large array is sampled, and the
limit on the files together."""
import json
import os

import numpy as np
import torch

import bench


def test_dump_writes_outputs_only_in_wide_dtypes_and_samples_large_arrays(tmp_path):
    inputs = {'image0': torch.zeros(1, 1, 8, 8)}
    big = torch.randn(3, 1000, 700)                                          # 8.4 MB as float32: above DUMP_WHOLE_BYTES
    batch = dict(inputs, b_ids=torch.arange(5), mask=torch.tensor([True, False]), conf=torch.rand(4, dtype=torch.float16),
                 rt=torch.randn(2, 3, 4, dtype=torch.float64), prior=np.ones((2, 3), np.float32), featmap=big,
                 hw=torch.Size([8, 8]), names=['mp3d'], none=None, _private=torch.ones(2))
    man = bench.dump_outputs(batch, inputs, str(tmp_path))
    assert sorted(man) == ['b_ids', 'conf', 'featmap', 'mask', 'prior', 'rt']
    assert sorted(os.listdir(tmp_path)) == sorted([k + '.npy' for k in man] + ['manifest.json'])
    assert json.load(open(tmp_path / 'manifest.json')) == man
    for key, dt in (('b_ids', np.float64), ('mask', np.float64), ('rt', np.float64), ('conf', np.float32), ('prior', np.float32)):
        a = np.load(tmp_path / f'{key}.npy')
        ref = batch[key] if isinstance(batch[key], np.ndarray) else batch[key].to(torch.float64).numpy()
        assert a.dtype == dt and a.shape == tuple(batch[key].shape) and np.array_equal(a, ref.astype(dt)), key
    idx = np.sort(np.random.default_rng(0).choice(big.numel(), bench.DUMP_SAMPLE, replace=False))
    assert man['featmap']['shape'] == [3, 1000, 700] and man['featmap']['sampled']['elements'] == bench.DUMP_SAMPLE
    assert np.array_equal(np.load(tmp_path / 'featmap.npy'), big.reshape(-1).numpy()[idx])


def test_dump_stays_within_its_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_WHOLE_BYTES', 4096)
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 512)
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 16 << 10)
    batch = {f'a{i:02d}': torch.randn(2000) for i in range(12)}             # 12 x 2 KiB sampled = 24 KiB > 16 KiB
    bench.dump_outputs(batch, {}, str(tmp_path))
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= 16 << 10 and len([f for f in os.listdir(tmp_path) if f.endswith('.npy')]) == 12
