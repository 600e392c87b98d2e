"""Same entry point as the reference's main.py:8-24: ``main.py --mode {train,eval,infer} --model vpho_net ...``."""
from vpho_amd.configs.args import cfg
from vpho_amd.trainer import Trainer, train_entry


def main():
    trainer = Trainer(cfg)
    if cfg.mode not in ('train', 'eval', 'infer'):
        raise ValueError(f'Unknown mode: {cfg.mode}')
    if getattr(cfg, 'frame_source', 'none') != 'none':
        # frames in: crops, augmentation and heat-map targets on the device (vpho_amd/frames.py), handed to the same Trainer methods
        from vpho_amd.frames import make_loader
        loader = make_loader(cfg, trainer.assets, trainer.device, train=cfg.mode == 'train')
        if cfg.mode == 'train':
            getattr(trainer, train_entry(cfg))(loader=loader)
        else:
            getattr(trainer, cfg.mode)(loader)
    elif cfg.mode == 'train':
        trainer.train()
    elif cfg.mode == 'eval':
        trainer.eval()
    else:
        trainer.infer()


if __name__ == '__main__':
    main()
