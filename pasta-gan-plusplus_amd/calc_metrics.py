"""Put numbers on the try-on driver's result images: the command line of the reference's calc_metrics.py, for the metrics that need no detector network.

    python calc_metrics.py --results test_results/upper [--metrics l1,psnr,ssim] [--pairs self|all] [--per-file per_image.jsonl] [--device cuda]
        [--dataroot /path/to/test_data --regions upper,lower,skin]

Reads the ``<person>___<clothes>.png`` triptychs tryon.py wrote (clothes | person | result), compares the person panel with the result panel and prints
one JSON line: {"l1": ..., "psnr": ..., "ssim": ..., "count": n, "pairs": "self"} (training/metrics.py).  With ``--regions`` (out of upper, lower,
garment, skin, other; labels from ``<dataroot>/parsing/<person>.png``) the line goes on with ``<metric>_<region>`` and ``count_<region>``."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from training.metrics import main  # noqa: E402

if __name__ == '__main__':
    main()
