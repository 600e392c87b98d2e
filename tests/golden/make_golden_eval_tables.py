"""Golden tables of evaluate.summarize / evaluate.hand_bench_table as they stood BEFORE the row layout became a declared table
(vpho_amd/eval_layout.py): run once at that commit, ``python tests/golden/make_golden_eval_tables.py``.  Pure fp64 torch arithmetic on
the CPU, so tests/test_eval_layout_cpu.py asks the later code for EQUAL tables, not close ones.

Writes golden_eval_tables.json: {'summarize': {width: table} for the 13 widths that summarize told apart by width, 'hand_bench_table':
{16 | 40: table}}.  The input rows are ``make_rows(width)`` / ``make_hand_bench(width)`` below, which the test calls again: 6 images of
a seeded generator, both hand sides, integer cell counts with zeros among them, one NaN planted in the volume block's pred_cells column
and one in the physics block's pred n_inside column where the width has those blocks.  The block positions are written out per width,
as literal numbers: this file knows nothing of the layout code it pins.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'golden_eval_tables.json')
# width -> (first column of the physics block, first column of the volume block); None: the width has no such block
WIDTHS = {28: (None, None), 32: (None, 28), 36: (28, None), 40: (28, 36), 88: (None, None), 92: (None, 88), 96: (88, None), 98: (None, 94),
          100: (88, 96), 106: (88, 102), 108: (88, None), 112: (88, 108), 118: (88, 114)}
HAND_BENCH_WIDTHS = (16, 40)


def make_rows(width):
    phys, vol = WIDTHS[width]
    g = torch.Generator().manual_seed(1000 + width)
    rows = torch.rand((6, width), generator=g)
    rows[:, 0] = torch.arange(6.0)
    rows[:, 7] = torch.tensor([1.0, 0, 1, 1, 0, 1])
    if vol is not None:
        first = vol - 6 if width in (98, 106, 118) else vol        # the six columns of every hypothesis' volume lie before the four
        for c in range(first + 1, width, 2):                        # IV | cells pairs: whole cell counts, zeros among them
            rows[:, c] = torch.floor(rows[:, c] * 3.0)
        rows[2, vol + 1] = float('nan')
    if phys is not None:
        rows[:, phys + 1] = torch.floor(rows[:, phys + 1] * 4.0)
        rows[4, phys + 1] = float('nan')
    return rows


def make_hand_bench(width):
    g = torch.Generator().manual_seed(2000 + width)
    blk = torch.rand((6, width), generator=g)
    blk[1, 2] = float('nan')
    return blk


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.argv = sys.argv[:1]
    from vpho_amd import evaluate as E
    res = {'summarize': {str(w): E.summarize(make_rows(w)) for w in WIDTHS},
           'hand_bench_table': {str(w): E.hand_bench_table(make_hand_bench(w)) for w in HAND_BENCH_WIDTHS}}
    with open(OUT, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=False)
        f.write('\n')
    print(OUT, {w: sorted(t) for w, t in res['summarize'].items()})


if __name__ == '__main__':
    main()
