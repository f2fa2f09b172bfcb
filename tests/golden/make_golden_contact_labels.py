"""Writes tests/golden/contact_labels.npz: the fp64 oracle records of the real-size contact-label case (tests/contact_labels_oracle.py
``torus_case``: 84 x 82 torus + 2 unreferenced vertices = 6890 vertices / 13776 faces, N = 2 poses, P = 2048 points).

    python tests/golden/make_golden_contact_labels.py

RECORDED FROM THE RESTATEMENT (tests/contact_labels_oracle.py), NOT from igl.signed_distance: igl, trimesh and psbody are not available, and the
restatement defines the contract.  The inputs are not stored -- the test rebuilds them from ``torus_case`` and recomputes a
slice of the records to prove that file and fixture belong together.
    d, w            float64 [2,2048]  distance and winding number per point
    human, human_lo, human_hi   packed bits [2,862]: body labels at thres, and the two bracketing runs of the comparison rule"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
from tests import contact_labels_oracle as co                 # noqa: E402


def main():
    recs = co.case_oracle(co.torus_case())
    pack = lambda k: np.stack([np.packbits(r[k]) for r in recs])
    out = os.path.join(HERE, 'contact_labels.npz')
    np.savez_compressed(out, d=np.stack([r['d'] for r in recs]), w=np.stack([r['w'] for r in recs]), human=pack('human'), human_lo=pack('human_lo'),
                        human_hi=pack('human_hi'))
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
