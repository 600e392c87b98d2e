"""The declared layout of the evaluation rows (vpho_amd/eval_layout.py): every flag combination against the width arithmetic it
replaced, written out here as literal numbers; from_width; and summarize / hand_bench_table against the tables the code returned before
the layout was declared (tests/golden/golden_eval_tables.json, made by tests/golden/make_golden_eval_tables.py at that commit).  Needs no
HIP library."""
import importlib.util
import itertools
import json
import math
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
# the 13 widths without hand-benchmark blocks, by (eval_best, eval_physics, physics_multi, eval_volume, volume_multi) after normalisation
PLAIN = {(0, 0, 0, 0, 0): 28, (0, 0, 0, 1, 0): 32, (0, 1, 0, 0, 0): 36, (0, 1, 0, 1, 0): 40, (1, 0, 0, 0, 0): 88, (1, 0, 0, 1, 0): 92,
         (1, 1, 0, 0, 0): 96, (1, 0, 0, 1, 1): 98, (1, 1, 0, 1, 0): 100, (1, 1, 0, 1, 1): 106, (1, 1, 1, 0, 0): 108, (1, 1, 1, 1, 0): 112,
         (1, 1, 1, 1, 1): 118}
BLOCK_WIDTH = dict(base=28, multi=60, physics=8, physics_multi=12, volume_multi=6, volume=4, hand_bench=16, hand_bench_multi=24)
FIVE = ('eval_best', 'eval_physics', 'physics_multi', 'eval_volume', 'volume_multi')                # the flags PLAIN is keyed by, in its order
SEVEN = FIVE + ('eval_hand_bench', 'hand_bench_multi')
# the whole table, in its order: (block, the flag that switches it on, width); a *_multi block also needs eval_best and the flag in NEEDS
TABLE = (('base', None, 28), ('multi', 'eval_best', 60), ('physics', 'eval_physics', 8), ('physics_multi', 'physics_multi', 12),
         ('volume_multi', 'volume_multi', 6), ('volume', 'eval_volume', 4), ('hand_bench', 'eval_hand_bench', 16),
         ('hand_bench_multi', 'hand_bench_multi', 24), ('symmetric', 'eval_symmetric', 3), ('symmetric_multi', 'symmetric_multi', 9),
         ('grasp', 'eval_grasp', 8), ('grasp_multi', 'grasp_multi', 24))
NEEDS = dict(physics_multi='eval_physics', volume_multi='eval_volume', hand_bench_multi='eval_hand_bench', symmetric_multi='eval_symmetric',
             grasp_multi='eval_grasp')
ELEVEN = ('eval_best', 'eval_physics', 'physics_multi', 'eval_volume', 'volume_multi', 'eval_hand_bench', 'hand_bench_multi', 'eval_symmetric',
          'symmetric_multi', 'eval_grasp', 'grasp_multi')


def _golden_module():
    spec = importlib.util.spec_from_file_location('make_golden_eval_tables', os.path.join(HERE, 'golden', 'make_golden_eval_tables.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_flag_combination():
    from vpho_amd.eval_layout import BLOCKS, RowLayout
    assert [(b.name, b.width) for b in BLOCKS[:8]] == list(BLOCK_WIDTH.items())
    for best, phys, pm, vol, vm, hb, hbm in itertools.product((False, True), repeat=7):
        lay = RowLayout.resolve(eval_best=best, eval_physics=phys, physics_multi=pm, eval_volume=vol, volume_multi=vm, eval_hand_bench=hb,
                                hand_bench_multi=hbm)
        # a *_multi block needs eval_best and the flag of its single-pose block
        pm_, vm_, hbm_ = pm and best and phys, vm and best and vol, hbm and best and hb
        assert (lay.eval_best, lay.eval_physics, lay.physics_multi, lay.eval_volume, lay.volume_multi, lay.eval_hand_bench, lay.hand_bench_multi) == \
            (best, phys, pm_, vol, vm_, hb, hbm_)
        want = PLAIN[int(best), int(phys), int(pm_), int(vol), int(vm_)] + (40 if hbm_ else 16 if hb else 0)
        assert lay.width == want
        assert len(lay.columns) == len(set(lay.columns)) == want
        have = [n for n in BLOCK_WIDTH if lay.has(n)]
        assert have == [n for n, on in zip(BLOCK_WIDTH, (True, best, phys, pm_, vm_, vol, hb, hbm_)) if on]
        at = 0
        for n in have:                                          # the blocks tile the row in the order of the table
            assert lay.slice(n) == slice(at, at + BLOCK_WIDTH[n])
            at += BLOCK_WIDTH[n]
        assert at == want
        if vol and not hb:
            assert lay.slice('volume') == slice(want - 4, want)                      # rows[:, -4:] is the volume block
        if vm_:
            assert lay.slice('volume_multi').stop == lay.slice('volume').start       # immediately before it
        if hbm_:
            assert lay.slice('hand_bench_multi').stop == want and lay.slice('hand_bench').stop == want - 24
        for n in BLOCK_WIDTH:
            if not lay.has(n):
                with pytest.raises(KeyError):
                    lay.slice(n)


def test_wrappers_and_constants_keep_their_values():
    """the width constants, and the widths the two width wrappers of evaluate gave, now read off the layout"""
    from vpho_amd import evaluate as E
    from vpho_amd.eval_layout import RowLayout
    assert (E.ROW, E.OBJ_COL, E.MULTI, E.ROW_BEST, E.PHYS, E.PHYS_MULTI, E.VOL, E.VOL_MULTI, E.HAND_BENCH, E.HAND_BENCH_MULTI) == \
        (28, 12, 60, 88, 8, 12, 4, 6, 16, 24)
    for (b, p, m, v, vm), w in PLAIN.items():
        assert RowLayout.resolve(eval_best=bool(b), eval_physics=bool(p), physics_multi=bool(m), volume_multi=bool(vm), eval_volume=bool(v)).width == w
    assert RowLayout.resolve(eval_hand_bench=True).width - 28 == 16
    assert RowLayout.resolve(eval_best=True, eval_hand_bench=True, hand_bench_multi=True).width - 88 == 40


def test_column_names():
    from vpho_amd import ops_names as N
    from vpho_amd.eval_layout import RowLayout
    assert len(N.BASE_COLUMNS) == 28 and N.BASE_COLUMNS[0] == 'image_index' and N.BASE_COLUMNS[7] == 'is_right'
    assert N.BASE_COLUMNS[12:] == tuple(f'object/{k}' for k in N.OBJ_METRIC_NAMES)
    cols = RowLayout.resolve(**dict.fromkeys(SEVEN, True)).columns
    assert cols == N.BASE_COLUMNS + N.MULTI_COLUMNS + N.PHYSICS_COLUMNS + N.PHYSICS_MULTI_COLUMNS + N.VOLUME_MULTI_COLUMNS + N.VOLUME_COLUMNS + \
        N.HAND_BENCH_COLUMNS + N.HAND_BENCH_MULTI_COLUMNS


def test_none_follows_the_configuration():
    from vpho_amd.configs.args import cfg
    from vpho_amd.eval_layout import RowLayout
    keys = ('eval_best', 'eval_physics', 'eval_volume', 'eval_hand_bench', 'eval_symmetric', 'eval_grasp')
    saved = {k: getattr(cfg, k) for k in keys}
    try:
        for flags in itertools.product((False, True), repeat=6):
            for k, v in zip(keys, flags):
                setattr(cfg, k, v)
            b, p, v, h, s, g = flags
            assert RowLayout.resolve(**dict.fromkeys(SEVEN)) == RowLayout.resolve(
                eval_best=b, eval_physics=p, physics_multi=b and p, eval_volume=v, volume_multi=b and v, eval_hand_bench=h, hand_bench_multi=b and h)
            # a caller that passes the older flags itself gets the block of every hypothesis only with both command-line flags
            assert RowLayout.resolve(eval_best=True, eval_physics=True, physics_multi=None, eval_volume=True, volume_multi=None, eval_hand_bench=True,
                                     hand_bench_multi=None) == RowLayout.resolve(
                eval_best=True, eval_physics=True, physics_multi=b and p, eval_volume=True, volume_multi=b and v, eval_hand_bench=True,
                hand_bench_multi=b and h)
            # the same rule for the symmetric and the grasp flags, and for all eleven at once
            assert RowLayout.resolve(eval_symmetric=None, symmetric_multi=None, eval_grasp=None, grasp_multi=None) == \
                RowLayout.resolve(eval_symmetric=s, eval_grasp=g)                    # eval_best is not named: off, so no *_multi block
            assert RowLayout.resolve(eval_best=True, eval_symmetric=True, symmetric_multi=None, eval_grasp=True, grasp_multi=None) == \
                RowLayout.resolve(eval_best=True, eval_symmetric=True, symmetric_multi=b and s, eval_grasp=True, grasp_multi=b and g)
            assert RowLayout.resolve(**dict.fromkeys(ELEVEN)) == RowLayout.resolve(
                eval_best=b, eval_physics=p, physics_multi=b and p, eval_volume=v, volume_multi=b and v, eval_hand_bench=h, hand_bench_multi=b and h,
                eval_symmetric=s, symmetric_multi=b and s, eval_grasp=g, grasp_multi=b and g)
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def test_from_width():
    from vpho_amd.eval_layout import RowLayout
    for flags, w in PLAIN.items():
        lay = RowLayout.from_width(w)
        assert lay == RowLayout.resolve(**{k: bool(f) for k, f in zip(FIVE, flags)}) and lay.width == w and not lay.has('hand_bench')
    # with the hand-benchmark blocks a width no longer names one layout: 92 + 16 = 108 and 96 + 16 = 112 are plain widths too, and
    # 88 + 40 = 112 + 16 = 128 -- so from_width knows none of those layouts, and refuses every width it does not know
    assert RowLayout.resolve(eval_best=True, eval_volume=True, eval_hand_bench=True).width == 108 == \
        RowLayout.resolve(eval_best=True, eval_physics=True, physics_multi=True).width
    assert RowLayout.resolve(eval_best=True, eval_physics=True, eval_hand_bench=True).width == 112 == \
        RowLayout.resolve(eval_best=True, eval_physics=True, physics_multi=True, eval_volume=True).width
    assert RowLayout.resolve(eval_best=True, eval_hand_bench=True, hand_bench_multi=True).width == 128 == \
        RowLayout.resolve(eval_best=True, eval_physics=True, physics_multi=True, eval_volume=True, eval_hand_bench=True).width
    for w in (44, 104, 128, 158):
        with pytest.raises(ValueError, match='28, 32, 36, 40, 88, 92, 96, 98, 100, 106, 108, 112, 118'):
            RowLayout.from_width(w)


def _same(a, b, path=''):
    """equal tables: the same keys in the same order, floats by ==, a NaN equal to a NaN"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (path, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            _same(a[k], b[k], f'{path}/{k}')
    elif isinstance(a, float) and math.isnan(a):
        assert isinstance(b, float) and math.isnan(b), (path, a, b)
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


def test_tables_equal_those_of_the_code_before_the_layout():
    import torch
    from vpho_amd import evaluate as E
    from vpho_amd.eval_layout import RowLayout
    G = _golden_module()
    with open(G.OUT) as f:
        gold = json.load(f)
    assert sorted(int(w) for w in gold['summarize']) == sorted(PLAIN.values()) == sorted(G.WIDTHS)
    nans = 0
    for flags, w in PLAIN.items():
        rows, want = G.make_rows(w), gold['summarize'][str(w)]
        assert rows.shape == (6, w) and 0 < int((rows[:, 7] > 0.5).sum()) < 6
        lay = RowLayout.resolve(**{k: bool(f) for k, f in zip(FIVE, flags)})
        _same(E.summarize(rows), want, str(w))
        _same(E.summarize(rows, lay), want, str(w))
        _same(E.summarize(rows, layout=lay), json.loads(json.dumps(E.summarize(rows))), str(w))      # and it survives the EVAL_JSON line
        nans += int(torch.isnan(rows).sum())
        if lay.has('volume'):
            assert math.isnan(want['volume']['pred']['intersecting_pct']) and not math.isnan(want['volume']['gt']['intersecting_pct'])
        if lay.has('physics'):
            assert math.isnan(want['physics']['pred']['penetration_rate_pct']) and not math.isnan(want['physics']['gt']['penetration_rate_pct'])
    assert nans == 8 + 8                                          # one per volume block, one per physics block
    for w in G.HAND_BENCH_WIDTHS:
        blk, want = G.make_hand_bench(w), gold['hand_bench_table'][str(w)]
        _same(E.hand_bench_table(blk[:, :16], blk[:, 16:] if w == 40 else None), want, f'hand_bench {w}')
        # through summarize: the block behind the widest plain row, read by name
        lay = RowLayout.resolve(**dict.fromkeys(FIVE, True), eval_hand_bench=True, hand_bench_multi=w == 40)
        full = E.summarize(torch.cat([G.make_rows(118), blk], 1), lay)
        _same(full['hand_bench'], want, f'summarize hand_bench {w}')
        _same({k: v for k, v in full.items() if k != 'hand_bench'}, gold['summarize']['118'], f'summarize 118 + {w}')
        assert list(full)[-1] == 'hand_bench'
    with pytest.raises(ValueError):
        E.summarize(torch.zeros((2, 44)))
    with pytest.raises(ValueError):
        E.summarize(torch.zeros((2, 44)), RowLayout.resolve(eval_best=True))


def test_the_whole_contract():
    """What callers may rely on, in literals.  The twelve blocks of TABLE in that order; the all-on layout; which parameters of metric_rows
    are positional; that flags go by keyword.  Then the layout rule restated from TABLE and NEEDS alone -- a block is there iff its flag is
    set and, for a *_multi block, eval_best and the flag it needs are set too -- against resolve at every one of the 2^11 flag settings."""
    import inspect
    from vpho_amd import evaluate as E
    from vpho_amd import ops_names as N
    from vpho_amd.eval_layout import BLOCKS, RowLayout
    from vpho_amd.trainer import Trainer
    assert [(b.name, b.flag, b.width) for b in BLOCKS] == list(TABLE) and len(TABLE) == 12
    assert {b.flag: b.needs for b in BLOCKS if b.needs} == NEEDS
    assert sorted(RowLayout.__dataclass_fields__) == sorted(ELEVEN) == sorted(flag for _, flag, _ in TABLE[1:])
    everything = RowLayout.resolve(**dict.fromkeys(ELEVEN, True))
    assert everything.width == 202 == sum(w for _, _, w in TABLE)
    names = (N.BASE_COLUMNS, N.MULTI_COLUMNS, N.PHYSICS_COLUMNS, N.PHYSICS_MULTI_COLUMNS, N.VOLUME_MULTI_COLUMNS, N.VOLUME_COLUMNS, N.HAND_BENCH_COLUMNS,
             N.HAND_BENCH_MULTI_COLUMNS, N.SYM_COLUMNS, N.SYM_MULTI_COLUMNS, N.GRASP_COLUMNS, N.GRASP_MULTI_COLUMNS)
    assert everything.columns == sum(names, ()) and len(set(everything.columns)) == 202
    assert [len(c) for c in names] == [w for _, _, w in TABLE]
    assert hash(everything) == hash(RowLayout(**dict.fromkeys(ELEVEN, True))) and RowLayout() == RowLayout.resolve()
    with pytest.raises(Exception):                                # frozen
        everything.eval_best = False
    # bench.py calls metric_rows(out, data, gt_joint, gt_vert, first_index, assets): those six by position, everything else by keyword
    p = list(inspect.signature(E.metric_rows).parameters.values())
    assert [q.name for q in p[:6]] == ['out', 'data', 'gt_joint', 'gt_vert', 'first_index', 'assets'] and p[5].default is None
    assert all(q.kind is q.POSITIONAL_OR_KEYWORD for q in p[:6]) and all(q.kind in (q.KEYWORD_ONLY, q.VAR_KEYWORD) for q in p[6:])
    assert 'layout' in [q.name for q in p[6:]] and inspect.signature(E.metric_rows).parameters['layout'].default is None
    # flags by keyword only, a flag that does not exist named in the refusal
    with pytest.raises(TypeError):
        RowLayout.resolve(True)
    with pytest.raises(TypeError, match='eval_bset'):
        RowLayout.resolve(eval_bset=True)
    q = list(inspect.signature(Trainer.eval).parameters.values())
    assert [x.name for x in q[:2]] == ['self', 'loader'] and q[1].default is None
    assert all(x.kind in (x.KEYWORD_ONLY, x.VAR_KEYWORD) for x in q[2:]) and 'layout' in [x.name for x in q[2:]]
    with pytest.raises(TypeError):
        Trainer.eval(object(), None, True)                        # refused when the arguments are bound: nothing of the trainer is touched
    with pytest.raises(TypeError, match='layout'):
        Trainer.eval(object(), layout=everything, eval_best=True)
    with pytest.raises(TypeError, match='eval_bset'):
        Trainer.eval(object(), eval_bset=True)
    # the rule, restated, at every flag setting
    seen = set()
    for values in itertools.product((False, True), repeat=11):
        f = dict(zip(ELEVEN, values))
        lay = RowLayout.resolve(**f)
        spans, cols, at = {}, (), 0
        for (name, flag, w), c in zip(TABLE, names):
            if flag is None or (f[flag] and (flag not in NEEDS or (f['eval_best'] and f[NEEDS[flag]]))):
                spans[name] = slice(at, at + w)
                cols += c
                at += w
        assert [n for n, _, _ in TABLE if lay.has(n)] == list(spans) and all(lay.slice(n) == s for n, s in spans.items())
        assert lay.width == at == len(cols) and lay.columns == cols
        assert all(getattr(lay, flag) == (name in spans) for name, flag, _ in TABLE[1:])
        seen.add(lay)
    assert len(seen) == 275 and sum(not l.eval_best for l in seen) == 32 and sum(l.eval_best for l in seen) == 243
