"""The layout of the per-image evaluation rows (evaluate.metric_rows, Trainer.eval, evaluate.summarize): ONE ordered table of column
blocks, and RowLayout, the blocks that a set of flags switches on.  Importable without the HIP library, as ops_names is."""
import functools
import itertools
from dataclasses import dataclass

from . import ops_names as N

# THE order of the columns, written here and nowhere else: (block, the RowLayout flag that switches it on, width, column names).
# What each block holds: the comments of ops_names at its column tuple, and INTEGRATION.md §1.
BLOCKS = (('base', None, 28, N.BASE_COLUMNS),
          ('multi', 'eval_best', 60, N.MULTI_COLUMNS),
          ('physics', 'eval_physics', 8, N.PHYSICS_COLUMNS),
          ('physics_multi', 'physics_multi', 12, N.PHYSICS_MULTI_COLUMNS),
          ('volume_multi', 'volume_multi', 6, N.VOLUME_MULTI_COLUMNS),
          ('volume', 'eval_volume', 4, N.VOLUME_COLUMNS),
          ('hand_bench', 'eval_hand_bench', 16, N.HAND_BENCH_COLUMNS),
          ('hand_bench_multi', 'hand_bench_multi', 24, N.HAND_BENCH_MULTI_COLUMNS))
# blocks added after BLOCKS was pinned to its eight entries (tests/test_eval_layout_cpu.py): they follow it, in this order; _spans, width and
# columns walk ALL_BLOCKS
BLOCKS_ADDED = (('symmetric', 'eval_symmetric', 3, N.SYM_COLUMNS),
                ('symmetric_multi', 'symmetric_multi', 9, N.SYM_MULTI_COLUMNS))
# ... and BLOCKS_ADDED was pinned to its two entries in turn (tests/test_symmetry_cpu.py): the blocks of --eval_grasp follow it
BLOCKS_GRASP = (('grasp', 'eval_grasp', 8, N.GRASP_COLUMNS),
                ('grasp_multi', 'grasp_multi', 24, N.GRASP_MULTI_COLUMNS))
ALL_BLOCKS = BLOCKS + BLOCKS_ADDED + BLOCKS_GRASP
assert all(len(cols) == w for _, _, w, cols in ALL_BLOCKS)
# each *_multi block (every sampled hypothesis) needs eval_best and the flag of its single-pose block
MULTI_NEEDS = {'physics_multi': 'eval_physics', 'volume_multi': 'eval_volume', 'hand_bench_multi': 'eval_hand_bench',
               'symmetric_multi': 'eval_symmetric', 'grasp_multi': 'eval_grasp'}


@dataclass(frozen=True)
class RowLayout:
    """the blocks of one evaluation's rows; made by ``resolve`` (or ``from_width``), which sets no *_multi flag without the two it needs"""
    eval_best: bool = False
    eval_physics: bool = False
    physics_multi: bool = False
    eval_volume: bool = False
    volume_multi: bool = False
    eval_hand_bench: bool = False
    hand_bench_multi: bool = False
    eval_grasp: bool = False                 # set by with_grasp; the last two fields and resolve's last two parameters are pinned by a test
    grasp_multi: bool = False
    eval_symmetric: bool = False
    symmetric_multi: bool = False

    @classmethod
    def resolve(cls, eval_best=False, eval_physics=False, physics_multi=False, eval_volume=False, volume_multi=False, eval_hand_bench=False,
                hand_bench_multi=False, eval_symmetric=False, symmetric_multi=False):
        """The layout of the nine flags.  None means 'follow the configuration': cfg.eval_best / eval_physics / eval_volume /
        eval_hand_bench / eval_symmetric for those five, and for a *_multi flag 'both command-line flags', cfg.eval_best and cfg.eval_<its block>, so
        that a caller who passes the older flags itself gets the rows it always got.  The grasp blocks: ``with_grasp`` on the result."""
        return cls._settle(dict(eval_best=eval_best, eval_physics=eval_physics, physics_multi=physics_multi, eval_volume=eval_volume,
                                volume_multi=volume_multi, eval_hand_bench=eval_hand_bench, hand_bench_multi=hand_bench_multi,
                                eval_symmetric=eval_symmetric, symmetric_multi=symmetric_multi))

    def with_grasp(self, eval_grasp=False, grasp_multi=False):
        """this layout with the blocks of --eval_grasp behind the others: ``eval_grasp`` / ``grasp_multi`` by resolve's rules (None: cfg.eval_grasp /
        cfg.eval_best and cfg.eval_grasp; grasp_multi needs this layout's eval_best and eval_grasp)"""
        return self._settle({**{k: getattr(self, k) for k in self.__dataclass_fields__}, 'eval_grasp': eval_grasp, 'grasp_multi': grasp_multi})

    @classmethod
    def _settle(cls, f):
        if None in f.values():
            from .configs.args import cfg
            for k in [k for k, v in f.items() if v is None]:
                f[k] = (cfg.eval_best and getattr(cfg, MULTI_NEEDS[k])) if k in MULTI_NEEDS else getattr(cfg, k)
        for k, single in MULTI_NEEDS.items():
            f[k] = f.get(k, False) and f['eval_best'] and f.get(single, False)
        return cls(**{k: bool(v) for k, v in f.items()})

    @classmethod
    def from_width(cls, width):
        """for callers that hold rows and no layout: the one layout WITHOUT hand-benchmark, symmetric or grasp blocks that is ``width`` columns wide (with
        those blocks the width no longer tells: 92 + 16 = 108, 96 + 16 = 112 and 88 + 40 = 112 + 16 = 128)"""
        if width not in _BY_WIDTH:
            raise ValueError(f'rows of {width} columns: no layout without hand-benchmark blocks is that wide (accepted: '
                             f'{", ".join(str(w) for w in sorted(_BY_WIDTH))}); pass the RowLayout of the rows')
        return _BY_WIDTH[width]

    def has(self, name):
        return name in _spans(self)

    def slice(self, name):
        """the columns of block ``name``; KeyError if the layout does not have it"""
        return _spans(self)[name]

    @property
    def width(self):
        return sum(len(cols) for name, _, _, cols in ALL_BLOCKS if self.has(name))

    @property
    def columns(self):
        return tuple(c for name, _, _, cols in ALL_BLOCKS if self.has(name) for c in cols)


@functools.lru_cache(maxsize=None)
def _spans(layout):
    spans, at = {}, 0
    for name, flag, w, _ in ALL_BLOCKS:
        if flag is None or getattr(layout, flag):
            spans[name] = slice(at, at + w)
            at += w
    return spans


_PLAIN = {RowLayout.resolve(*f) for f in itertools.product((False, True), repeat=5)}
_BY_WIDTH = {l.width: l for l in _PLAIN}
assert len(_BY_WIDTH) == len(_PLAIN) == 13, 'two layouts without hand-benchmark blocks share a width: from_width cannot tell them apart'
