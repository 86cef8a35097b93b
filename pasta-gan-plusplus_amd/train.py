"""Train on a dataset directory: the command line of the reference's train.py, the options this package supports.

    python train.py --data /path/to/train_data --outdir runs/full --batch 32 --batch-gpu 4 --gamma 10 --aug ada --target 0.6 \
        --kimg 25000 --tick 4 --snap 50 [--resume network-snapshot-000100.pt | reference.pkl] [--workers 8] [--metrics l1,psnr,ssim[,parsing]] \
        [--metric-regions upper,lower,skin]

Writes stats.jsonl and network-snapshot-*.pt into --outdir (training/training_loop.py)."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from training.training_loop import main  # noqa: E402

if __name__ == '__main__':
    main()
