"""The layout of the per-image evaluation rows (evaluate.metric_rows, Trainer.eval, evaluate.summarize): ONE ordered table of column
blocks, and RowLayout, the blocks that a set of flags switches on.  Importable without the HIP library, as ops_names is."""
import functools
import itertools
from dataclasses import dataclass
from typing import NamedTuple, Optional

from . import ops_names as N


class Block(NamedTuple):
    name: str
    flag: Optional[str]                      # the RowLayout flag that switches it on (None: always there)
    width: int
    columns: tuple
    needs: Optional[str] = None              # a *_multi block (every sampled hypothesis): the flag of its single-pose block; it needs eval_best too


# THE order of the columns, written here and nowhere else.  What each block holds: the comments of ops_names at its column tuple, and
# INTEGRATION.md §1.  A new block goes at the end, with a field of its flag's name in RowLayout.
BLOCKS = (Block('base', None, 28, N.BASE_COLUMNS),
          Block('multi', 'eval_best', 60, N.MULTI_COLUMNS),
          Block('physics', 'eval_physics', 8, N.PHYSICS_COLUMNS),
          Block('physics_multi', 'physics_multi', 12, N.PHYSICS_MULTI_COLUMNS, 'eval_physics'),
          Block('volume_multi', 'volume_multi', 6, N.VOLUME_MULTI_COLUMNS, 'eval_volume'),
          Block('volume', 'eval_volume', 4, N.VOLUME_COLUMNS),
          Block('hand_bench', 'eval_hand_bench', 16, N.HAND_BENCH_COLUMNS),
          Block('hand_bench_multi', 'hand_bench_multi', 24, N.HAND_BENCH_MULTI_COLUMNS, 'eval_hand_bench'),
          Block('symmetric', 'eval_symmetric', 3, N.SYM_COLUMNS),
          Block('symmetric_multi', 'symmetric_multi', 9, N.SYM_MULTI_COLUMNS, 'eval_symmetric'),
          Block('grasp', 'eval_grasp', 8, N.GRASP_COLUMNS),
          Block('grasp_multi', 'grasp_multi', 24, N.GRASP_MULTI_COLUMNS, 'eval_grasp'))
assert all(len(b.columns) == b.width for b in BLOCKS)


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
    eval_symmetric: bool = False
    symmetric_multi: bool = False
    eval_grasp: bool = False
    grasp_multi: bool = False

    @classmethod
    def resolve(cls, **flags):
        """The layout of the eleven flags, by keyword; one that is not named is off.  None means 'follow the configuration': cfg.<flag> for
        the six command-line flags, and for a *_multi flag 'both command-line flags', cfg.eval_best and cfg.eval_<its block>, so that a caller
        who passes the older flags itself gets the rows it always got.  A *_multi flag is kept only with eval_best and its single-pose flag."""
        unknown = [k for k in flags if k not in cls.__dataclass_fields__]
        if unknown:
            raise TypeError(f'RowLayout.resolve: no flag named {", ".join(map(repr, unknown))} (the flags: {", ".join(cls.__dataclass_fields__)})')
        f = {k: flags.get(k, False) for k in cls.__dataclass_fields__}
        if None in f.values():
            from .configs.args import cfg
            for b in BLOCKS[1:]:
                if f[b.flag] is None:
                    f[b.flag] = (cfg.eval_best and getattr(cfg, b.needs)) if b.needs else getattr(cfg, b.flag)
        for b in BLOCKS:
            if b.needs:
                f[b.flag] = f[b.flag] and f['eval_best'] and f[b.needs]
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
        return sum(b.width for b in BLOCKS if self.has(b.name))

    @property
    def columns(self):
        return tuple(c for b in BLOCKS if self.has(b.name) for c in b.columns)


@functools.lru_cache(maxsize=None)
def _spans(layout):
    spans, at = {}, 0
    for b in BLOCKS:
        if b.flag is None or getattr(layout, b.flag):
            spans[b.name] = slice(at, at + b.width)
            at += b.width
    return spans


_PLAIN = {RowLayout.resolve(**dict(zip(('eval_best', 'eval_physics', 'physics_multi', 'eval_volume', 'volume_multi'), f)))
          for f in itertools.product((False, True), repeat=5)}
_BY_WIDTH = {l.width: l for l in _PLAIN}
assert len(_BY_WIDTH) == len(_PLAIN) == 13, 'two layouts without hand-benchmark blocks share a width: from_width cannot tell them apart'
