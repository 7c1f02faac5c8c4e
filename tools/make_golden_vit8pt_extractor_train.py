"""Container-only: golden G27 -- one training step's worth of results of the 8-Point-ViT extractor's final block, produced by the
reference's own class:

    interiornetStreetlearn_8ptVit/src/modules/extractor.py: ResidualBlock(128, 192, 'batch', kernel_size=5), unmodified, in .train()
    (the block model.py:60 builds and train.py fine-tunes), fp32, under torch autograd

Weights, the (4, 128, 9, 11) input and the output gradient come from the seeded CPU generator of tests/vit8pt_extractor_train_ref.py
(block_fill, block_case); the fixture holds recorded results only: the output, the input gradient, the BatchNorm and bias gradients,
the updated running statistics and a fixed strided slice of every weight gradient.  The float64 restatement's distance is printed.
Usage: python tools/make_golden_vit8pt_extractor_train.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')


def reference_block():
    from tools.make_golden_vit8pt_extractor import REF            # where the container keeps the reference's sources
    sys.path.insert(0, REF)
    from src.modules.extractor import ResidualBlock
    return ResidualBlock(128, 192, 'batch', kernel_size=5)


def main():
    from tests import vit8pt_extractor_ref as er
    from tests import vit8pt_extractor_train_ref as etr
    ref = reference_block()
    x, gy = etr.block_case(etr.block_fill(ref))
    mine = er.FinalConv()
    assert [k for k, _ in etr.block_entries(mine)] == [k for k, _ in etr.block_entries(ref)]
    mine.load_state_dict(ref.state_dict(), strict=True)              # before the run: the running statistics of the fill
    got = etr.block_run(ref, x, gy)
    assert int(ref.norm1.num_batches_tracked) == 1
    r64 = etr.block_run(mine.double(), x, gy)
    print(f'output: positive share {float((got["y"] > 0).double().mean()):.3f}  max |.| {float(got["y"].abs().max()):.2f}')
    for k in sorted(got):
        sc = float(r64[k].abs().max())
        print(f'{k:28s} reference fp32 vs float64 restatement {float((got[k] - r64[k]).abs().max()):.3e}  (max |.| {sc:.3e})')
    path = os.path.join(OUT, 'g27_vit8pt_final_block_train.npz')
    np.savez_compressed(path, seed=etr.SEED, **{k: v.float().numpy() for k, v in got.items()},
                        note="reference: interiornetStreetlearn_8ptVit src/modules/extractor.py ResidualBlock(128, 192, 'batch', kernel_size=5) "
                             'in .train(), fp32 autograd, input (4, 128, 9, 11); weight gradients: [::4, ::8] of (Cout, Cin, k, k)')
    print(f'g27_vit8pt_final_block_train: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
