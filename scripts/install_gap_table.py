"""Write the finger-gap table where ``vpho_amd.physics_labels.gap_table`` looks for it:

    python scripts/install_gap_table.py ASSET_ROOT        # -> ASSET_ROOT/ours/finger_gap_links.npz

The arrays are those of tests/golden/golden_hand_surface.npz: ``links`` (302, 2) and ``alpha`` (302,), recovered there by running the
reference's own ``fill_finger_gaps_in_mano`` on a one-hot input (tests/golden/make_golden_hand_surface.py).  Without the file the
labeler runs on a seeded synthetic table and says so."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    if len(argv) != 1:
        raise SystemExit(__doc__)
    from vpho_amd.physics_labels import GAP_FILE
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_hand_surface.npz'), allow_pickle=False) as z:
        links, alpha = z['links'], z['alpha']
    path = os.path.join(argv[0], GAP_FILE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, links=links.astype(np.int32), alpha=alpha.astype(np.float64))
    print(f'{path}: {len(links)} links, {778 + len(links)} filled rows')


if __name__ == '__main__':
    main(sys.argv[1:])
