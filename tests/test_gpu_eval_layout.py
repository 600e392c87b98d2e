"""The declared row layout (vpho_amd/eval_layout.py) end to end on the device: one Trainer, three evaluations of the same images from
the same prior draws -- every block (158 columns), every block but the hand benchmark's (118), the hand benchmark's alone (44).  A block
holds the same bits whichever other blocks the row has, every block read by name has its width, and the EVAL_JSON table is
summarize(rows, layout).  Two batches of two images: the smallest run in which every block is filled by more than one batch and both
hand sides occur."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu
EVAL_ARGS = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=2, num_batches=2, random_seed=7)
BLOCK_WIDTH = dict(base=28, multi=60, physics=8, physics_multi=12, volume_multi=6, volume=4, hand_bench=16, hand_bench_multi=24)


def _by_image(rows):
    idx = rows[:, 0]
    assert len(set(idx.tolist())) == rows.shape[0]
    return rows[idx.argsort()]


def test_three_layouts_of_the_same_images(capsys):
    from vpho_amd import evaluate as E
    from vpho_amd.configs.args import cfg
    from vpho_amd.eval_layout import RowLayout
    from vpho_amd.trainer import Trainer
    keys = tuple(EVAL_ARGS) + ('checkpoint', 'eval_best', 'eval_physics', 'eval_volume', 'eval_hand_bench', 'physics_voxel_pitch')
    saved = {k: getattr(cfg, k) for k in keys}
    for k, v in EVAL_ARGS.items():
        setattr(cfg, k, v)
    cfg.checkpoint, cfg.eval_best, cfg.eval_physics, cfg.eval_volume, cfg.eval_hand_bench, cfg.physics_voxel_pitch = None, False, False, False, False, 0.005
    plain = dict(eval_best=True, eval_physics=True, physics_multi=True, eval_volume=True, volume_multi=True)
    try:
        t = Trainer(cfg)
        rng_state = torch.get_rng_state()                  # behind the model's construction: where the prior draws of an evaluation start
        capsys.readouterr()
        rows158 = t.eval(eval_hand_bench=True, hand_bench_multi=True, **plain)
        text = capsys.readouterr().out
        torch.set_rng_state(rng_state)
        rows118 = t.eval(**plain)
        torch.set_rng_state(rng_state)
        rows44 = t.eval(eval_hand_bench=True)
        capsys.readouterr()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    n = EVAL_ARGS['eval_batch_size'] * EVAL_ARGS['num_batches']
    assert rows158.shape == (n, 158) and rows118.shape == (n, 118) and rows44.shape == (n, 44)
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, text[-2000:]
    layout = RowLayout.resolve(eval_hand_bench=True, hand_bench_multi=True, **plain)
    # as text: key order and a NaN compare too, and a float's text gives the float back
    assert json.dumps(json.loads(line[0][len('EVAL_JSON '):])['table']) == json.dumps(E.summarize(rows158.cpu(), layout))
    rows158, rows118, rows44 = (_by_image(r) for r in (rows158, rows118, rows44))
    assert 0 < int((rows158[:, 7] > 0.5).sum()) < n                                # both hand sides
    i32 = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(i32(rows158[:, :118]), i32(rows118))
    assert torch.equal(i32(rows158[:, layout.slice('hand_bench')]), i32(rows44[:, 28:]))
    assert torch.equal(i32(rows158[:, layout.slice('base')]), i32(rows44[:, :28]))
    at = 0
    for name, w in BLOCK_WIDTH.items():
        blk = rows158[:, layout.slice(name)]
        assert blk.shape == (n, w) and layout.slice(name).start == at, name
        at += w
        assert torch.isfinite(blk).all(), name                                     # torch.empty rows: every block was written
    assert at == 158
