"""Entry-point glue that mirrors the reference's ``Trainer`` surface for the inference path
(lib/engine/base_trainer.py:18-96, lib/engine/train_diff_hand_obj.py:27-357): ``Trainer(cfg).eval()`` builds
``vpho_net``, optionally loads a checkpoint with the reference's key layout, runs ``evaluate`` over per-rank batches and
prints the MJE/MVE tables after ONE all-gather of fixed-layout metric rows.  One process per GPU: launch with
``python -m torch.distributed.run --nproc-per-node N main.py --mode eval ...`` (or ``accelerate launch``, which sets the
same RANK/LOCAL_RANK/WORLD_SIZE variables).  There is no dataset in this build: batches are synthetic (vpho_amd.synth).
``run`` (``--mode train``): ``--train_scope full`` (default) runs the end-to-end training step (train_step.DiffusionTrainStep:
backbone, heat-map heads, encoders, MANO head and score networks are all updated); ``--train_scope score`` trains the two score
networks on frozen features (``ScoreTrainer.step``: the reference's ``repeat_num`` DSM draws, backward, data-parallel gradient
average and AdamW per denoiser).
``fit`` (``--mode train --max_epochs N``): the reference's epoch loop around that step -- LR schedule, gradient clipping and accumulation,
a checkpoint in accelerate's format after every epoch, resume (vpho_amd/checkpoint.py).
``infer`` (``--mode infer``): the same batches through the same pipeline, predictions written to files (vpho_amd/infer.py).
"""
import os
import time

import torch
import torch.distributed as dist

from . import evaluate as E
from .assets import load_assets
from .synth import synth_state_dict, synth_batch


def load_checkpoint_state_dict(path):
    """The state_dict of a checkpoint written by the reference: ``accel.save_state(<save_dir>/checkpoint/epoch_N.state)`` --
    a DIRECTORY holding ``model.safetensors`` (accelerate's default) or ``pytorch_model.bin`` next to optimizer / scheduler /
    RNG files (base_trainer.py:81-89) -- or ``final_model.pt`` / any plain ``state_dict`` file (base_trainer.py:91-96).
    Keys of a DistributedDataParallel wrapper (``module.`` prefix) are accepted."""
    if os.path.isdir(path):
        cand = [os.path.join(path, f) for f in ('model.safetensors', 'pytorch_model.bin', 'model.bin', 'pytorch_model.safetensors')]
        found = [c for c in cand if os.path.exists(c)]
        if not found:
            raise FileNotFoundError(f'{path} is a directory but holds no model file of an accelerate state (looked for: '
                                    + ', '.join(os.path.basename(c) for c in cand) + f'); it contains: {sorted(os.listdir(path))[:20]}')
        path = found[0]
    elif not os.path.exists(path):
        raise FileNotFoundError(f'checkpoint {path} does not exist')
    if path.endswith('.safetensors'):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location='cpu', weights_only=True)
    if isinstance(sd, dict) and 'state_dict' in sd and not any(torch.is_tensor(v) for v in sd.values()):
        sd = sd['state_dict']
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    return sd, path


def ema_state_dict(checkpoint, state_dict, param_names):
    """``--use_ema``: the state_dict of ``--checkpoint`` with its trained tensors replaced by their moving averages.  The averages live in
    the state DIRECTORY a run with ``--ema_rate`` wrote (``custom_checkpoint_0.pkl``, shadow i = parameter i of
    ``vpho_net(...).named_parameters()``); ``final_model_ema.pt`` already IS the averaged model and is passed as it stands."""
    from . import checkpoint as CK
    from .ema import CUSTOM_INDEX, overlay
    name = CK.custom_file(CUSTOM_INDEX)
    if not checkpoint:
        raise ValueError(f'--use_ema needs --checkpoint <save_dir>/checkpoint/epoch_N.state (a state directory holding {name})')
    if not os.path.isdir(checkpoint):
        raise ValueError(f'--use_ema reads the moving average from a state directory ({name}), but --checkpoint {checkpoint} is a plain '
                         f'state_dict file: pass final_model_ema.pt itself as --checkpoint, without --use_ema')
    path = os.path.join(checkpoint, name)
    if not os.path.exists(path):
        raise FileNotFoundError(f'--use_ema: {checkpoint} holds no {name} (written by a run with --ema_rate > 0); it contains: '
                                f'{sorted(os.listdir(checkpoint))[:20]}')
    return overlay(state_dict, torch.load(path, map_location='cpu', weights_only=True), param_names), path


def synthetic_mano_targets(mano, gt_rot6d, gt_shape, is_right):
    """ground-truth vertices / joints of a synthetic hand pose: the MANO forward of the training kernel with zero loss weights"""
    bs = gt_rot6d.shape[0]
    z = lambda *s: torch.zeros(s, device=gt_rot6d.device)
    _, _, _, gv, gj = mano.train(gt_rot6d.contiguous(), gt_shape.contiguous(), z(bs, 778, 3), z(bs, 21, 3), gt_rot6d.contiguous(), gt_shape.contiguous(),
                                 is_right.to(torch.uint8).contiguous(), (0.0, 0.0, 0.0, 0.0), want_outputs=True)
    return dict(gt_hand_vert_flip=gv, gt_hand_jt3d_flip=gj, gt_mano=torch.cat([z(bs, 48), gt_shape], 1))


def loader_indices_are_consecutive(index):
    """a collated ``index`` column (dexycb6.py:472) can serve as the row's image index only if the batch is a run"""
    i = index.reshape(-1).long()
    return bool((i[1:] - i[:-1] == 1).all()) if i.numel() > 1 else True


def train_entry(cfg):
    """which Trainer method ``main.py --mode train`` runs: 'fit' (epochs, scheduler, checkpoints) when --max_epochs is given, else 'run'"""
    return 'fit' if getattr(cfg, 'max_epochs', None) is not None else 'run'


class Trainer:
    def __init__(self, cfg):
        self.cfg = cfg
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.rank = int(os.environ.get('RANK', '0'))
        self.local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        self.device = torch.device('cuda', self.local_rank)
        torch.cuda.set_device(self.device)
        if self.world > 1 and not dist.is_initialized():
            from .launch import init_process_group
            init_process_group(self.device)                # loud on failure: bounded timeout, expected vs observed world
        self.setup_seed()
        self.assets = load_assets(cfg.asset_root)
        self.model = self.get_model()

    def setup_seed(self):
        """base_trainer.py:39-50: seed = random_seed + rank * 1e8."""
        torch.manual_seed(int(self.cfg.random_seed + self.rank * 1e8))

    def get_model(self):
        from .model.VPHO import vpho_net
        model = vpho_net(self.assets)
        use_ema = bool(getattr(self.cfg, 'use_ema', False))
        if use_ema and not self.cfg.checkpoint:
            ema_state_dict(self.cfg.checkpoint, None, None)        # raises: nothing to take an average from
        if self.cfg.checkpoint:
            sd, path = load_checkpoint_state_dict(self.cfg.checkpoint)
            if use_ema:                                            # the averaged weights over the live ones, by parameter order
                sd, path = ema_state_dict(self.cfg.checkpoint, sd, [k for k, p in model.named_parameters() if p.requires_grad])
            missing, unexpected = model.load_state_dict(sd, strict=False)      # base_trainer.py:81-83 (strict=False)
            if self.rank == 0:
                print(f'loaded {path}: {len(missing)} missing, {len(unexpected)} unexpected keys')
        else:
            model.load_state_dict(synth_state_dict(model, seed=1))
        return model.to(self.device).eval()

    def _synthetic_targets(self, bs, i):
        g = torch.Generator().manual_seed(int(self.cfg.random_seed + 7919 * i + self.rank))
        rot = torch.linalg.qr(torch.randn(bs, 17, 3, 3, generator=g))[0]                   # synthetic ground truth: random rotations
        gt_hand = rot[:, :16, :2, :].reshape(bs, 96).to(self.device)                       # 16 x rot6d (mano_aa_to_6D(...)[..., :-10])
        gt_obj = torch.cat([rot[:, 16, :2, :].reshape(bs, 6), torch.randn(bs, 3, generator=g) * 0.05], -1).to(self.device)
        return gt_hand, gt_obj, g

    def _train_batches(self, loader, n_batches, mano, start=0):
        """``start``: number of the first synthetic batch (Trainer.fit numbers them through the epochs).  yields (batch on the device, gt_hand (bs,96) rot6d, gt_obj (bs,9)).  ``loader`` None: synthetic batches with synthetic targets.
        Otherwise any iterable of collated Appendix-A batch dicts with the training keys of lib/dataset/dexycb6.py:471-509 (hm_hand,
        hm_obj, gt_mano, gt_obj, gt_hand_vert_flip, gt_hand_jt3d_flip, force_local, ...): the targets are derived as the reference's
        forward does, gt_hand = mano_aa_to_6D(gt_mano)[..., :96] (VPHO.py:190, head_mano.py:10-18), gt_obj as it stands."""
        cfg, bs = self.cfg, self.cfg.batch_size
        if loader is not None:
            from .model.VPHO import _aa_to_rot6d
            for i, b in enumerate(loader):
                if n_batches is not None and i >= n_batches:
                    return
                b = self._to_device(b)
                missing = [k for k in ('gt_mano', 'gt_obj', 'hm_hand', 'hm_obj') if k not in b]
                if missing:
                    raise KeyError(f'training batch lacks {missing} (lib/dataset/dexycb6.py:471-509)')
                yield b, _aa_to_rot6d(b['gt_mano'][:, :48].float()), b['gt_obj'].float().contiguous()
            return
        for i in range(start, start + (cfg.num_batches if n_batches is None else n_batches)):
            batch = self._to_device(synth_batch(bs, self.assets, seed=cfg.random_seed + i, rank=self.rank))
            gt_hand, gt_obj, g = self._synthetic_targets(bs, i)
            batch['hm_hand'] = (torch.rand(bs, 21, cfg.heatmap_size, cfg.heatmap_size, generator=g) * 0.2).to(self.device)
            batch['hm_obj'] = (torch.rand(bs, 27, cfg.heatmap_size, cfg.heatmap_size, generator=g) * 0.2).to(self.device)
            batch.update(synthetic_mano_targets(mano, gt_hand, (torch.randn(bs, 10, generator=g) * 0.5).to(self.device), batch['is_right']))
            batch['force_local'] = (torch.randn(bs, 32, 3, generator=g) * 0.1).to(self.device)      # pseudo-force labels (force_optim.py's output)
            yield batch, gt_hand, gt_obj

    def run_full(self, n_batches=None, loader=None):
        """End-to-end training (train_diff_hand_obj.py:169-199) with all 13 losses of VPHO.py:190-212 (train_step.DiffusionTrainStep):
        backbone, heat-map heads, encoders, score networks, head_mano, both cross modules and head_physics are updated.  Batches:
        ``_train_batches`` (synthetic by default, or any iterable of Appendix-A dicts).  Returns the per-batch loss dicts (floats)."""
        from .train_step import DiffusionTrainStep
        cfg = self.cfg
        step = DiffusionTrainStep(self.model.state_dict(), self.device, assets=self.assets)
        hist = []
        for i, (batch, gt_hand, gt_obj) in enumerate(self._train_batches(loader, n_batches, step.mano_head.mano)):
            L = step.step(batch, gt_hand, gt_obj)
            hist.append({k: float(v) for k, v in L.items()})
            if self.rank == 0 and i % 10 == 0:
                print(f'[{i:04d}] ' + '  '.join(f'{k.replace("_loss", "")} {v:.3e}' for k, v in hist[-1].items()))
        self.model.load_state_dict(step.state_dict(), strict=False)
        return hist

    def train(self):
        """``--mode train``: the epoch loop ``fit`` when ``--max_epochs`` is given, else one pass ``run`` (nothing written)"""
        return getattr(self, train_entry(self.cfg))()

    def fit(self, loader=None, epochs=None, save_dir=None, eval_loader=None):
        """The reference's training loop (train_diff_hand_obj.py:126-199, base_trainer.py:81-96): ``epochs`` (default cfg.max_epochs)
        epochs of ``steps_per_epoch`` batches (``len(loader)``; synthetic: cfg.num_batches, numbered through the epochs so that a
        resumed run draws the batches a straight run would), each through the fused training step with cfg.gradient_clip,
        cfg.gradient_accumulation_steps and the scheduler's learning rate; after every epoch the scheduler step, the weights written back
        into ``self.model``, ``<save_dir>/checkpoint/epoch_<e+1>.state`` (vpho_amd/checkpoint.py: what ``accel.save_state`` writes) and, with
        ``eval_loader``, ``self.eval(eval_loader)``; after the last epoch ``<save_dir>/final_model.pt``.  ``cfg.checkpoint`` naming such a
        state directory resumes it: optimiser, scheduler and generators restored, first epoch = the N of ``epoch_N.state``.
        ``save_dir`` defaults to ``<output_dir>/<timestamp>_<mark>_train_<model>`` (base_trainer.py:52-55).  Returns a dict
        (save_dir, start_epoch, epochs, per epoch the learning rate it ran at and its last loss line as floats).
        ``cfg.ema_rate`` > 0 keeps the reference's moving average of the weights (lib/model/ema.py; vpho_amd/ema.py): every state directory
        gets ``custom_checkpoint_0.pkl`` (accelerate's file of a registered object) beside the live ``model.safetensors``, a resume restores
        it (a state directory without one starts the average from the restored weights with 0 updates), ``eval_loader`` is evaluated with
        the AVERAGED weights, ``<save_dir>/final_model_ema.pt`` is written next to ``final_model.pt`` and the dict says ``ema=True``."""
        from . import checkpoint as CK
        from .ema import CUSTOM_INDEX
        from .train_step import DiffusionTrainStep
        cfg = self.cfg
        if getattr(cfg, 'train_scope', 'full') != 'full':
            raise ValueError("Trainer.fit (--max_epochs) trains end to end: it needs --train_scope full; --train_scope score has no "
                             "epochs, schedulers or checkpoints (use Trainer.run)")
        epochs = cfg.max_epochs if epochs is None else epochs
        if epochs is None or epochs < 1:
            raise ValueError(f'Trainer.fit needs epochs >= 1 (--max_epochs), got {epochs}')
        steps_per_epoch = cfg.num_batches if loader is None else len(loader)
        A = max(1, int(getattr(cfg, 'gradient_accumulation_steps', 1)))
        print_freq = max(1, int(getattr(cfg, 'print_freq', 500)))
        if save_dir is None:
            names = [os.path.join(cfg.output_dir, f"{time.strftime('%Y%m%d_%H%M%S', time.localtime())}_{cfg.mark}_train_{cfg.model}")]
            if self.world > 1:
                dist.broadcast_object_list(names, src=0)           # one directory for all ranks (base_trainer.py:53-54)
            save_dir = names[0]
        if getattr(cfg, 'use_ema', False):
            raise ValueError('--use_ema loads the averaged weights for --mode eval / infer; training keeps its average with --ema_rate')
        ema_rate = float(getattr(cfg, 'ema_rate', 0.0) or 0.0)
        ema = ema_rate > 0                                         # --ema_rate 0: nothing allocated, launched or written
        step = DiffusionTrainStep(self.model.state_dict(), self.device, assets=self.assets, optimizer=getattr(cfg, 'optimizer', 'adamw'),
                                  ema=ema_rate if ema else None)
        sched = CK.make_scheduler(getattr(cfg, 'scheduler', 'exp'), cfg.base_learning_rate, self.world, getattr(cfg, 'gamma', 0.96),
                                  getattr(cfg, 'lr_step', 5), epochs, steps_per_epoch)
        start_epoch, seen = 0, 0
        if CK.is_training_state(cfg.checkpoint):                   # the weights and running statistics came in through get_model
            st = CK.load_state(cfg.checkpoint, self.rank)          # ... this restores the generators too
            step.load_optimizer_state(st['optimizer'])
            sched.load_state_dict(st['scheduler'])
            sched.load_group(st['optimizer']['param_groups'][0])
            start_epoch, seen = CK.epoch_of(cfg.checkpoint), st['step']
            if self.rank == 0:
                print(f'resumed {cfg.checkpoint}: epoch {start_epoch}, optimiser step {step.steps}, lr {sched.lr:.3e}')
            if ema and len(st['custom']) > CUSTOM_INDEX:
                step.load_ema_state(st['custom'][CUSTOM_INDEX])   # decay and num_updates come with it (ema.py:89-92)
                if self.rank == 0:
                    print(f'resumed the moving average: decay {step.ema.decay}, {step.ema.num_updates} updates')
            elif ema and self.rank == 0:                           # a checkpoint of the reference, or of a run without --ema_rate
                print(f'{cfg.checkpoint} holds no {CK.custom_file(CUSTOM_INDEX)}: the moving average starts from the restored weights, 0 updates')
        out = dict(save_dir=save_dir, start_epoch=start_epoch, epochs=epochs, lr=[], losses=[])
        if ema:
            out['ema'] = True
        for epoch in range(start_epoch, epochs):
            if self.rank == 0:
                print(f'Epoch: {epoch}/{epochs} | Learning Rate: {sched.lr:.3e}')
            out['lr'].append(sched.lr)
            step.hyper['beta1'] = sched.beta1
            L = None
            for i, (batch, gt_hand, gt_obj) in enumerate(self._train_batches(loader, steps_per_epoch, step.mano_head.mano, start=epoch * steps_per_epoch)):
                L = step.step(batch, gt_hand, gt_obj, lr=sched.lr, gradient_clip=cfg.gradient_clip, fused=True,
                              accumulation=(i % A, A, i == steps_per_epoch - 1) if A > 1 else None)
                if self.rank == 0 and i % print_freq == 0:
                    print(f'[{i:04d}/{steps_per_epoch}]| Loss ' + ' '.join(f'{k.replace("_loss", "")}:{float(v):.2e}' for k, v in L.items()))
            out['losses'].append({k: float(v) for k, v in L.items()} if L is not None else {})
            sched.step_epoch()
            seen = step.steps
            self.model.load_state_dict(step.state_dict(), strict=False)
            opt = step.optimizer_state()
            for g in opt['param_groups']:                          # the group as the reference's optimiser holds it after scheduler.step()
                g.update(lr=sched.lr, betas=(sched.beta1, g['betas'][1]), **sched.group_extras())
            CK.save_state(os.path.join(save_dir, 'checkpoint', f'epoch_{epoch + 1}.state'), self.model.state_dict(), opt, sched.state_dict(),
                          self.rank, self.world, step=seen, custom=[step.ema_state()] if ema else None)
            if eval_loader is not None:
                if ema:
                    # the averaged weights are the ones evaluated.  The step's masters may BE the module's tensors (a packed 1x1 weight
                    # is a view of the parameter it was built from), so the live values are copied out first and put back right after
                    live = step.state_dict()
                    self.model.load_state_dict(step.state_dict(ema=True), strict=False)
                self.eval(eval_loader)
                if ema:
                    self.model.load_state_dict(live, strict=False)
        self.model.load_state_dict(step.state_dict(), strict=False)
        if ema:                                                    # the module's state_dict with the averages in place of the trained tensors
            averaged = dict(self.model.state_dict())
            averaged.update({k: v.reshape(averaged[k].shape) for k, v in step.state_dict(ema=True).items()})
            CK.save_model(os.path.join(save_dir, 'final_model_ema.pt'), averaged, self.rank)
        CK.save_model(os.path.join(save_dir, 'final_model.pt'), self.model.state_dict(), self.rank)
        if self.rank == 0:
            print(f'trained epochs {start_epoch}..{epochs} of {steps_per_epoch} batches: {save_dir}')
        return out

    def run(self, n_batches=None, loader=None):
        """``Trainer.run`` (train_diff_hand_obj.py:126-153).  ``loader``: an iterable of Appendix-A batch dicts; default synthetic."""
        if getattr(self.cfg, 'train_scope', 'full') == 'full':
            return self.run_full(n_batches, loader)
        if loader is not None:
            raise NotImplementedError("--train_scope score trains on frozen features of synthetic batches only; use --train_scope full with a loader")
        return self.run_score(n_batches)

    def run_score(self, n_batches=None):
        from .model.engine import Engine
        from .train_score import ScoreTrainer
        cfg, bs = self.cfg, self.cfg.eval_batch_size
        n_batches = cfg.num_batches if n_batches is None else n_batches
        eng = Engine(self.model)
        sd = self.model.state_dict()
        hand, obj = ScoreTrainer(sd, 'denoiser_hand', self.device), ScoreTrainer(sd, 'denoiser_obj', self.device)
        losses = []
        for i in range(n_batches):
            batch = {k: (v.to(self.device) if torch.is_tensor(v) else v)
                     for k, v in synth_batch(bs, self.assets, seed=cfg.random_seed + i, rank=self.rank).items()}
            with torch.no_grad():
                f = eng.features(batch)
            gt_hand, gt_obj, _ = self._synthetic_targets(bs, i)
            lh, _ = hand.step(f['encoding_hand'], gt_hand, repeat_num=getattr(cfg, 'repeat_num', 20))
            lo, _ = obj.step(f['encoding_obj'], gt_obj, repeat_num=getattr(cfg, 'repeat_num', 20))
            losses.append((float(lh), float(lo)))
            if self.rank == 0 and i % 10 == 0:
                print(f'[{i:04d}/{n_batches}] diff_hand_loss {losses[-1][0]:.3e}  diff_obj_loss {losses[-1][1]:.3e}')
        self.model.load_state_dict({**hand.state_dict(), **obj.state_dict()}, strict=False)
        return losses

    def _to_device(self, batch):
        return {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def _eval_batches(self, loader, need_gt=True):
        """yields (batch on the device, (gt_joint, gt_vert), index of its first image).  ``loader`` None: ``cfg.num_batches`` synthetic
        batches whose ground truth is batch 0's own regression output (there is no data set in this build).  Otherwise ANY iterable of
        collated Appendix-A batch dicts (lib/dataset/dexycb6.py:471-509; what ``accel.prepare`` hands each rank,
        train_diff_hand_obj.py:211-217): ground truth = ``gt_joint`` / ``gt_hand_vert`` in the camera frame (:237-238), the object's
        ``gt_obj_rt`` or, like the reference's postprocess of the batch (:578-597), ``gt_obj`` (9-D) + root joint.
        ``need_gt=False`` (``infer``): batches without hand ground truth are taken as they are, their ground truth is None."""
        cfg, bs = self.cfg, self.cfg.eval_batch_size
        if loader is None:
            gt = None
            for i in range(cfg.num_batches):
                b = self._to_device(synth_batch(bs, self.assets, seed=cfg.random_seed + i, rank=self.rank))
                gt = yield b, gt, (self.rank * cfg.num_batches + i) * bs
            return
        seen = 0
        for b in loader:
            # column 0 of the metric rows, decided on the HOST batch (a device tensor here would cost two syncs per batch inside the
            # three-deep pipeline): the data set's own indices (one arange when the batch is a run of them, else the index tensor itself); batches WITHOUT an `index` key get rank-unique NEGATIVE ids
            # -(rank + world * running count) - 1 per image -- they can collide neither with another rank's fallback nor with a real data-set index
            idx = b.get('index')
            first = ids = None
            if torch.is_tensor(idx) and idx.numel():
                hidx = (idx.cpu() if idx.is_cuda else idx).reshape(-1)
                if loader_indices_are_consecutive(hidx):
                    first = int(hidx[0])
                else:
                    ids = hidx.clone()            # a shuffled loader / DistributedSampler: the data set's own indices, image by image
            b = self._to_device(b)
            missing = [k for k in ('gt_joint', 'gt_hand_vert') if k not in b]
            if missing and need_gt:
                raise KeyError(f'evaluation batch lacks {missing}: Trainer.eval(loader) needs the ground truth of lib/dataset/dexycb6.py:471-509')
            if 'gt_obj_rt' not in b and 'gt_obj' in b:
                from . import ops
                b['gt_obj_rt'] = ops.obj_9d_to_rt(b['gt_obj'].double().contiguous(), b['root_joint'].float().contiguous()).float()
            n = b['rgb'].shape[0]
            yield b, (None if missing else (b['gt_joint'].float(), b['gt_hand_vert'].float())), (first if first is not None else ids if ids is not None else -(self.rank + self.world * (seen + torch.arange(n))) - 1)
            seen += n

    @torch.no_grad()
    def eval(self, loader=None, *, layout=None, **flags):
        """``evaluate(testing_dataloader)`` (train_diff_hand_obj.py:202-357).  ``loader``: see ``_eval_batches``; default synthetic.
        ``flags``: the eleven flags of eval_layout.RowLayout, by keyword; they choose the column blocks of the returned rows and the tables
        printed from them (eval_layout.BLOCKS has the blocks and their order, INTEGRATION.md §1 what they hold): ``eval_best`` (the
        reference's is_eval_best) scores every sampled hypothesis (tables one_candidate, best_of_S, mean_of_S), ``eval_physics`` reports
        hand-object penetration and contact (``physics``), ``eval_volume`` the intersection volume at cfg.physics_voxel_pitch (``volume``),
        ``eval_hand_bench`` the hand F-scores and PCK AUC of the HO3D / FreiHAND leaderboards (``hand_bench``), ``eval_symmetric`` the
        symmetry-aware object errors (``symmetric``), ``eval_grasp`` the contact-map and grasp agreement (``grasp``); the ``*_multi`` flag
        of a table adds every sampled hypothesis to it and needs eval_best and the table's own flag.  A flag that is None or not named
        follows the configuration (RowLayout.resolve): cfg.<flag>, and for a *_multi flag cfg.eval_best and cfg.eval_<its table>, i.e. both
        command-line flags: a caller that passes eval_best / eval_physics / ... itself gets the rows it always got unless it asks for the
        newer block too.  ``layout``: a RowLayout instead of flags; both together are a TypeError."""
        from .configs.args import cfg
        if layout is not None and flags:
            raise TypeError(f'Trainer.eval: a layout and flags ({", ".join(flags)}) together; pass one of the two')
        if layout is None:
            layout = E.RowLayout.resolve(**{**dict.fromkeys(E.RowLayout.__dataclass_fields__), **flags})
        batch_rows = lambda out, batch, gt, first: E.metric_rows(out, batch, gt[0], gt[1], first, self.assets, layout=layout)
        E.build_meters(layout, self.assets, self.device)            # once, before the timed loop
        rows = []
        t0 = time.perf_counter()
        # three batches in flight (independent images; see evaluate.PipelinedPredictor)
        pipe = E.PipelinedPredictor(self.model, depth=3)
        futs = []
        gen = self._eval_batches(loader)
        try:
            item = next(gen)
            while True:
                b, gt, first = item
                if gt is None:
                    # synthetic run: batch 0 provides the ground truth (its own regression output), so it is evaluated first
                    out0 = pipe.submit(b).result()
                    gt = (out0['reg_hand_joint'] + b['root_joint'][:, None], out0['reg_hand_vert'] + b['root_joint'][:, None])
                    rows.append(batch_rows(out0, b, gt, first))
                else:
                    futs.append(pipe.submit(b, lambda out, batch, eng, first=first, gt=gt: batch_rows(out, batch, gt, first)))
                item = gen.send(gt)
        except StopIteration:
            pass
        rows += [f.result() for f in futs]
        pipe.close()
        # a rank whose shard is empty still takes part in the collective (with zero rows: the ragged gather carries the counts first);
        # raising here would leave the other ranks blocked in their all-gather.  Only an evaluation without ANY image is an error
        mine = torch.cat(rows, 0) if rows else torch.zeros((0, layout.width), device=self.device, dtype=torch.float32)
        rows = E.gather_rows(mine)
        if rows.shape[0] == 0:
            raise ValueError('Trainer.eval: the loader yielded no batch on any rank')
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if self.rank == 0:
            what = 'synthetic images' if loader is None else 'images'
            print(f'evaluated {rows.shape[0]} {what} on {self.world} GPU(s) in {dt:.2f} s ({rows.shape[0] / dt:.1f} images/s)')
            print(f'aggregation_mode_hand {cfg.aggregation_mode_hand}  aggregation_mode_obj {cfg.aggregation_mode_obj}')
            table = E.summarize(rows.cpu(), layout)
            for name, r in table.items():
                if name not in ('object', 'physics', 'volume', 'hand_bench', 'symmetric', 'grasp') + E.MULTI_TABLES:
                    print(f'{name:>5s}: n={r["n"]:5d}  MJE reg {r["MJE_reg"]:.2f}  first {r["MJE_first"]:.2f}  agg {r["MJE_agg"]:.2f}  MVE agg {r["MVE_agg"]:.2f}  (mm)')
            print('object (aggregated pose): ' + '  '.join(f'{k} {v:.2f}' for k, v in table['object'].items()))
            for name in E.MULTI_TABLES:
                if name in table:
                    print(f'{name} hand (mm): ' + '  '.join(f'{k} {v:.2f}' for k, v in table[name]['hand'].items()))
                    print(f'{name} object: ' + '  '.join(f'{k} {v:.2f}' for k, v in table[name]['object'].items()))
            for name, note, fmt in (('physics', '', '.2f'), ('volume', f' (pitch {cfg.physics_voxel_pitch * 1000.0:g} mm)', '.3f'), ('hand_bench', '', '.4f'),
                                    ('symmetric', ' (m, m, share)', '.5f'), ('grasp', '', '.4f')):
                for src, r in table.get(name, {}).items():
                    print(f'{name} {src}{note}: ' + '  '.join(f'{k} {v:{fmt}}' for k, v in r.items()))
            import json
            print('EVAL_JSON ' + json.dumps({'images': int(rows.shape[0]), 'world': self.world, 'aggregation_mode_hand': cfg.aggregation_mode_hand,
                                             'aggregation_mode_obj': cfg.aggregation_mode_obj, 'table': table}))
        if self.world > 1:
            dist.barrier()
        return rows

    @torch.no_grad()
    def infer(self, loader=None, save_dir=None):
        """``Trainer.infer`` (train_diff_hand_obj.py:359-444): predictions to files.  ``loader``: see ``_eval_batches`` (hand ground truth is
        not needed); default ``cfg.num_batches`` synthetic batches.  Per batch ONE kernel turns the predict outputs into per-image records
        and ONE asynchronous copy lands them in pinned host memory (ops.InferPacker), inside the three-deep pipeline; a host thread takes
        them out.  Every rank writes a shard, rank 0 merges and writes under ``save_dir`` (default
        ``<output_dir>/<timestamp>_<mark>_infer_<model>``, base_trainer.py:52-63) ``submit/hand_reg.zip``, ``submit/hand_diff.zip`` and
        ``my-prediction_align-<clean_data_mode>.pkl`` (vpho_amd/infer.py), prints the object table of the aggregated
        pose when the batches carry its ground truth, and one ``INFER_JSON`` line.  Returns that line's dict on rank 0, None elsewhere.
        With ``cfg.infer_render`` = N > 0 each rank also renders the first N images it sees to ``<save_dir>/render/<index:08d>.png``
        (vpho_amd/render.py, csrc/raster.hip) and the line gains ``render: {dir, images}``; at 0 nothing of that is imported or run."""
        import json
        import queue
        import threading
        import numpy as np
        from . import infer as INF
        from . import ops
        from .configs.args import cfg
        if save_dir is None:
            names = [os.path.join(cfg.output_dir, f"{time.strftime('%Y%m%d_%H%M%S', time.localtime())}_{cfg.mark}_infer_{cfg.model}")]
            if self.world > 1:
                dist.broadcast_object_list(names, src=0)           # one directory for all ranks (base_trainer.py:53)
            save_dir = names[0]
        t0 = time.perf_counter()
        pipe = E.PipelinedPredictor(self.model, depth=3)
        packer = ops.InferPacker(self.device, max_batch=cfg.eval_batch_size, slots=pipe.depth)
        free = [threading.Semaphore(1) for _ in range(pipe.depth)]       # a slot's pinned buffer is refilled only after the host took its records
        todo, recs, objs, errors = queue.Queue(), [], [], []
        # --infer_render N: this rank's first N images as overlays (vpho_amd/render.py, imported only here).  Per batch two raster launches,
        # one overlay launch and one asynchronous copy into the slot's pinned buffer, all on the slot's stream inside `post`; the host thread
        # below encodes the PNGs once the slot's event (recorded behind them by packer.pack) has passed
        n_render = max(int(getattr(cfg, 'infer_render', 0) or 0), 0)
        render_dir, rendered, render_skipped, render_host = os.path.join(save_dir, 'render'), [0, 0], [0], [None] * pipe.depth
        if n_render:
            from . import render as RND
            renderer = RND.MeshRenderer(self.assets, self.device, getattr(cfg, 'asset_root', 'asset'))
            os.makedirs(render_dir, exist_ok=True)

        def consume():
            while True:
                item = todo.get()
                if item is None:
                    return
                fut, slot, shots = item
                try:
                    obj = fut.result()
                    recs.append(packer.collect(slot).copy())
                    objs.append(obj)
                    for i, image_index in enumerate(shots):
                        RND.write_png(os.path.join(render_dir, f'{int(image_index):08d}.png'), render_host[slot][i].numpy())
                        rendered[1] += 1
                except BaseException as e:          # noqa: B036  (kept for the submitting thread; the slot is released either way)
                    errors.append(e)
                finally:
                    free[slot].release()

        host = threading.Thread(target=consume, name='vpho-infer-collect')
        host.start()
        ident = []                                   # per batch, decided on the HOST batch: (data-set indices or None, paths or None)

        def tap(batches):
            for b in batches:
                idx = b.get('index')
                idx = (idx.cpu() if idx.is_cuda else idx).reshape(-1).long().numpy().copy() if torch.is_tensor(idx) and idx.numel() else None
                ident.append((idx, b.get('rgb_path')))
                yield b

        index, paths, sizes, seen, any_index, skipped_obj = [], [], [], 0, loader is None, 0
        gen = self._eval_batches(None if loader is None else tap(loader), need_gt=False)
        try:
            item = next(gen)
            while not errors:
                b, _, first = item
                n = b['rgb'].shape[0]
                if n > packer.max_batch:
                    raise ops.VphoError(f'Trainer.infer: a batch of {n} images with --eval_batch_size {packer.max_batch}: the prediction records '
                                        f'are staged in buffers of eval_batch_size images')
                idx, rp = ident[-1] if loader is not None else (np.arange(first, first + n, dtype=np.int64), None)
                any_index = any_index or idx is not None
                index.append(np.arange(seen, seen + n, dtype=np.int64) if idx is None else idx)
                if (idx is None) != (not any_index):
                    raise KeyError("Trainer.infer: some batches carry 'index' and some do not")
                paths += [''] * n if rp is None else [str(p) for p in rp]
                sizes.append(n)
                seen += n
                want_obj = all(k in b for k in ('gt_obj_rt', 'cam_intr', 'obj_name'))
                skipped_obj += 0 if want_obj else 1
                slot = pipe.n % pipe.depth
                free[slot].acquire()
                take = min(n, n_render - rendered[0]) if n_render else 0
                if take > 0 and not all(k in b for k in ('cam_intr_crop_flip', 'obj_name')):
                    render_skipped[0] += 1
                    take = 0
                shots = [int(i) for i in index[-1][:take]]
                rendered[0] += take
                if take > 0 and (render_host[slot] is None or tuple(render_host[slot].shape[1:3]) != tuple(b['rgb'].shape[2:])):
                    render_host[slot] = torch.empty((packer.max_batch,) + tuple(b['rgb'].shape[2:]) + (3,), dtype=torch.uint8, pin_memory=True)

                def post(out, batch, eng, slot=slot, want_obj=want_obj, take=take):
                    if take > 0:
                        cut = lambda v: v[:take] if torch.is_tensor(v) or isinstance(v, (list, tuple)) else v
                        img = renderer.overlay({k: cut(v) for k, v in batch.items()}, {k: cut(out[k]) for k in ('agg_hand_vert', 'agg_obj_6d')})
                        render_host[slot][:take].copy_(img, non_blocking=True)
                    packer.pack(out, batch, slot=slot)                      # on the slot's stream: kernel + copy + event
                    return E.object_metric_block(out, batch, self.assets).float() if want_obj else None

                todo.put((pipe.submit(b, post), slot, shots))
                item = gen.send(None)
        except StopIteration:
            pass
        finally:
            todo.put(None)
            host.join()
            pipe.close()
        if errors:
            raise errors[0]
        t_collected = time.perf_counter() - t0           # every record of this rank is in host memory; no file has been touched yet
        dt = recs[0].dtype if recs else ops.infer_record_dtype()
        rec = np.concatenate(recs) if recs else np.zeros(0, dt)
        mine = dict(index=np.concatenate(index) if index else np.zeros(0, np.int64), path=paths, batch_sizes=sizes, has_index=any_index,
                    **{k: rec[k] for k in INF.RECORD_FIELDS})
        # object table of the aggregated pose: (n,16) per batch -> rows of the evaluation layout, one small all-gather (rank order = merge order)
        rows = torch.zeros((seen, E.ROW), device=self.device, dtype=torch.float32)
        with_obj = bool(objs) and all(o is not None for o in objs)
        if with_obj:
            rows[:, E.OBJ_COL:E.OBJ_COL + 16] = torch.cat(objs, 0)
        if self.world > 1:
            INF.write_shard(save_dir, self.rank, mine, mine['index'], paths, sizes, any_index)
            flags = [None] * self.world
            dist.all_gather_object(flags, (with_obj, seen, rendered[1], render_skipped[0]))
            with_obj = all(f[0] or f[1] == 0 for f in flags)
            rendered[1], render_skipped[0] = sum(f[2] for f in flags), sum(f[3] for f in flags)
            rows = E.gather_rows(rows)
            dist.barrier()                               # every shard is complete on disk
        res = None
        if self.rank == 0:
            shards = [mine] if self.world == 1 else [INF.shard_path(save_dir, r) for r in range(self.world)]
            rec, idx_all, path_all, size_all, order, gaps = INF.merge_shards(shards)
            if order.size == 0:
                raise ValueError('Trainer.infer: the loader yielded no batch on any rank')
            files = INF.write_outputs(save_dir, cfg.clean_data_mode, rec, idx_all, path_all, size_all, order)
            t_files = time.perf_counter() - t0
            N = int(order.size)
            what = 'synthetic images' if loader is None else 'images'
            print(f'inferred {N} {what} on {self.world} GPU(s): records collected in {t_collected:.2f} s ({N / t_collected:.1f} images/s), '
                  f'files written after {t_files:.2f} s ({N / t_files:.1f} images/s)')
            for k, v in files.items():
                print(f'  {k}: {v}')
            table = None
            if with_obj:
                table = E.summarize(rows.cpu()[torch.from_numpy(order)])['object']
                print('Object Evaluation: \nMean Pose: \n' + '  '.join(f'{k} {v:.2f}' for k, v in table.items()))
            else:
                print("Object Evaluation: skipped (the batches carry no 'gt_obj_rt' / 'gt_obj', 'cam_intr', 'obj_name')")
            res = {'images': N, 'world': self.world, 'files': files, 'object': table, 'images_per_s': N / t_collected,
                   'images_per_s_with_files': N / t_files, 'missing_indices': int(gaps.size), 'save_dir': save_dir}
            if n_render:
                if render_skipped[0]:
                    print(f"Render: {render_skipped[0]} batch(es) skipped (they carry no 'cam_intr_crop_flip' / 'obj_name')")
                print(f'  render: {rendered[1]} overlay(s) under {render_dir}')
                res['render'] = {'dir': render_dir, 'images': int(rendered[1])}
            print('INFER_JSON ' + json.dumps(res))
        if self.world > 1:
            dist.barrier()
        return res
