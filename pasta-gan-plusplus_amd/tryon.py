"""Try garments on people with a network snapshot: the command line of the reference's test.py / test.sh.

    python tryon.py --dataroot test_datas --testtxt test_pairs.txt --network network-snapshot-004408.pkl \
        --outdir test_results/upper --batchsize 1 --testpart upper --use-sleeve-mask [--device cuda] [--workers 4]

Writes one PNG per pair: clothes | person | result (training/tryon.py).  ``--testpart outfit`` (not one of the reference's) takes the top of one clothes
image and the trousers or skirt of another: pairs-file lines of ``<upper> <lower> <person>``, PNGs of upper clothes | lower clothes | person | result."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from training.tryon import main  # noqa: E402

if __name__ == '__main__':
    main()
