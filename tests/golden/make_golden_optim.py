"""Parameter order and optimiser groups of the reference, for the checkpoint exchange (vpho_amd/checkpoint.py): the names, shapes and
``requires_grad`` of the reference's own ``vpho_net().named_parameters()`` (lib/model/VPHO.py) -- ``optimizer.bin`` of an
``accel.save_state`` directory indexes its state by the position in that list -- and the ``param_groups`` of the two optimisers its
trainer builds (lib/engine/train_diff_hand_obj.py:49-54), tensors left out (``params`` are the positions).  Written to
tests/golden/golden_param_order.json.  Run in the build container only.
"""
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def main():
    from vpho_amd.assets import synthetic_assets
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_optim_')
    MG.write_assets(tmp, assets)
    os.chdir(tmp)
    sys.argv = ['main.py', '--mode', 'train']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(assets)
    import torch.utils.model_zoo as zoo
    import lib.model.backbone_FPN_HFL as ref_fpn
    zoo.load_url = lambda url, **kw: ref_fpn.ResNet(ref_fpn.Bottleneck, [3, 4, 6, 3]).state_dict()
    import lib.model.VPHO as ref_vpho
    from lib.configs.args import cfg as ref_cfg
    torch.manual_seed(0)
    ref = ref_vpho.vpho_net()
    params = [dict(name=k, shape=list(p.shape), requires_grad=bool(p.requires_grad)) for k, p in ref.named_parameters()]
    # the two optimisers exactly as get_optimizer builds them (train_diff_hand_obj.py:49-54)
    adamw = torch.optim.AdamW(ref.parameters(), betas=(0.9, 0.999), eps=1e-8, lr=ref_cfg.base_learning_rate)
    adam = torch.optim.Adam(ref.parameters(), lr=ref_cfg.base_learning_rate, weight_decay=0.0005)

    def groups(opt):
        out = []
        for g in opt.state_dict()['param_groups']:
            out.append({k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in g.items()})
        return out

    out = dict(torch=torch.__version__.split('+')[0], params=params, param_groups=dict(adamw=groups(adamw), adam=groups(adam)),
               flags={k: getattr(ref_cfg, k) for k in ('max_epochs', 'optimizer', 'scheduler', 'gamma', 'lr_step', 'gradient_accumulation_steps',
                                                       'print_freq', 'base_learning_rate', 'gradient_clip')})
    path = os.path.join(HERE, 'golden_param_order.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print(path, len(params), 'parameters,', sum(not p['requires_grad'] for p in params), 'frozen')


if __name__ == '__main__':
    main()
