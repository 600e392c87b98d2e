"""Run configuration: the module-global ``cfg`` the model reads at call time.

Mirrors the behaviour of the reference's lib/configs/args.py:4-260 for the flags the inference path and the
``main.py`` entry point use (same names, same defaults, same "argparse at import" semantics), except that unknown
flags are tolerated (``parse_known_args``) so that importing the package under pytest / torchrun does not abort.
"""
import argparse
import sys


# lib/configs/args.py:235-245 (the object side offers no `2D_pt_joint`)
AGGREGATION_MODES_HAND = ('heatmap_cascade', 'heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random')
AGGREGATION_MODES_OBJ = ('heatmap_cascade', 'heatmap', '2D_pt_pose', 'average_all', 'random')
# lib/configs/args.py:151-155: names the data split; --mode infer puts it into the name of its prediction pickle
CLEAN_DATA_MODES = ('2023_CVPR_HFL', '2022_CVPR_ArtiBoost', '2023_WACV_DMA', 'stable_grasping', '2023_NIPS_DeepSimHO')


class Config:
    def __init__(self):
        self.mode = 'train'
        self.eval_full = False
        self.eval_best = False        # also score every sampled hypothesis: one-candidate, best-of-S and mean-of-S tables (is_eval_best)
        self.eval_physics = False     # also report hand-object penetration and contact
        self.physics_contact_thresh = 0.005   # contact distance (m): the reference's contact_vertical_distance_thresh
        self.eval_volume = False      # also report the hand-object intersection volume; independent of eval_physics
        self.physics_voxel_pitch = 0.005      # its voxel pitch (m): the 0.5 cm of the ObMan / GraspTTA evaluations
        self.eval_hand_bench = False  # also report the hand F@5 / F@15 and PCK AUC of the HO3D / FreiHAND leaderboards
        self.eval_symmetric = False   # also report the symmetry-aware object errors SMCE / MSSD / MSSD01d
        self.max_sym_disc_step = 0.01         # discretisation of a continuous symmetry: the reference's constant (test.py:205)
        self.eval_grasp = False       # also report the contact-map and grasp agreement with the annotation; gates: contact_*
        self.mark = ''
        self.random_seed = 0
        self.output_dir = 'output'
        self.checkpoint = ''
        self.pretrain = ''
        self.remove_pretrained_keys = []
        self.dataset_name = 'dexycb'
        self.clean_data_mode = '2023_CVPR_HFL'
        self.patch_size = 256
        self.batch_size = 64
        self.eval_batch_size = 32
        self.num_batches = 4          # synthetic batches / synthetic frames (--frame_source synthetic); a frame directory has its own length
        self.model = 'vpho_net'
        self.sde_mode = 've'
        self.repeat_num = 20
        self.sampler = 'ode'
        self.sampling_steps = 500
        self.heatmap_size = 64
        self.roi_size = 32
        self.sample_T0 = 0.65
        self.sample_num = 50
        self.topk_hand = 15
        self.topk_obj = 5
        # how the S hypotheses become one answer: the visual-physical cascade, or one of the reference's ablation baselines
        self.aggregation_mode_hand = 'heatmap_cascade'
        self.aggregation_mode_obj = 'heatmap_cascade'
        self.do_weighted_average = True   # is_weight of the hand's `heatmap` mode only (the cascade is always weighted)
        self.asset_root = 'asset'
        self.base_learning_rate = 2e-4
        self.gradient_clip = -1.0
        self.train_scope = 'full'     # 'full': backbone + heads + encoders + score networks; 'score': score networks on frozen features
        self.weight_diff_hand_loss = 1.0
        self.weight_diff_obj_loss = 1.0
        self.weight_hm_hand_loss = 1.0
        self.weight_hm_obj_loss = 1.0
        self.weight_vert_loss = 1.0
        self.weight_joint_loss = 1.0
        self.weight_mano_pose_loss = 1.0
        self.weight_mano_shape_loss = 1.0
        self.weight_force_loss = 1.0
        self.weight_gravity_loss = 1.0
        self.weight_torque_loss = 1.0
        self.weight_supervised_loss = 1.0
        self.weight_CoM_loss = 1.0
        # the training loop of Trainer.fit (lib/configs/args.py:131-144; max_epochs None = one pass of Trainer.run, nothing written)
        self.max_epochs = None
        self.optimizer = 'adamw'
        self.scheduler = 'exp'
        self.gamma = 0.96
        self.lr_step = 5
        self.gradient_accumulation_steps = 1
        self.print_freq = 500
        self.ema_rate = 0.0           # decay of a moving average of the weights kept by Trainer.fit (lib/model/ema.py); 0 = none
        self.use_ema = False          # --mode eval / infer: the averaged weights of a --checkpoint state directory (custom_checkpoint_0.pkl)
        # frames in (vpho_amd/frames.py; lib/configs/args.py:156-199): 'none' = the synthetic batch dicts, nothing of the front end is imported
        self.frame_source = 'none'    # none | synthetic | a FrameDirectory path
        self.bbox_scale_factor = 1.2
        self.center_jittering = 0.2
        self.scale_factor = 0.2
        self.max_rot = 30.0
        self.rot_prob = 1.0
        self.RGB_shift_prob = 0.5
        self.shift_limit = (-20.0, 20.0)
        self.color_jitter_prob = 0.5
        self.brightness = (0.6, 1.3)
        self.saturation = (0.6, 1.3)
        self.random_erasing_prob = 0.5
        self.random_erasing_min_area = 0.02
        self.random_erasing_max_area = 0.2
        self.random_erasing_max_count = 1
        self.heatmap_hand_sigma = 2.0
        self.heatmap_obj_sigma = 2.0
        # photometric augmentation on the device (vpho_amd/photo.py; base.py:349-397): every gate is off by default, the reference's values
        # are PHOTO_REFERENCE below (--photo_aug reference).  Contrast and hue ride under color_jitter_prob, like brightness and saturation
        self.photo_aug = 'none'       # none | reference: the five switches below at the reference's values; explicit flags win
        self.clahe_p = 0.0
        self.clahe_clip_limit = (1.0, 4.0)
        self.jitter_contrast = (1.0, 1.0)
        self.jitter_hue = (0.0, 0.0)
        self.blur_p = 0.0
        self.blur_limit = (3, 7)
        self.sigma_limit = (0.2, 2.0)
        self.motion_blur_p = 0.0
        self.motion_blur_limit = (3, 7)
        # physics labels from annotations (vpho_amd/physics_labels.py): the gates of get_hand_contact (lib/configs/args.py:44-45)
        self.contact_normal_distance_thresh = (-0.01, 0.01)
        self.contact_vertical_distance_thresh = 0.005
        self.frame_contact = False    # FramePipeline also emits hand_contact / force_contact and takes is_grasped from them
        self.infer_render = 0         # --mode infer: each rank also renders its first N images to <save_dir>/render/<index>.png (vpho_amd/render.py)
        self.cross_dropout = 0.1      # the reference's nn.TransformerEncoderLayer / PositionalEncoding default (cross_module.py:64,104-107)


# what --photo_aug reference stands for: A.CLAHE(p=0.5), A.ColorJitter(contrast=(0.6, 1.3), hue=(-0.15, 0.15)), A.AdvancedBlur(p=0.5),
# A.MotionBlur(p=0.5) of base.py:349-397
PHOTO_REFERENCE = dict(clahe_p=0.5, jitter_contrast=(0.6, 1.3), jitter_hue=(-0.15, 0.15), blur_p=0.5, motion_blur_p=0.5)


class _Explicit(argparse.Action):
    """stores the value and notes that the flag was given, so that --photo_aug leaves it alone"""
    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace._explicit = getattr(namespace, '_explicit', ()) + (self.dest,)


class _Parser(argparse.ArgumentParser):
    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        explicit = ns.__dict__.pop('_explicit', ())
        if getattr(ns, 'photo_aug', 'none') == 'reference':
            for k, v in PHOTO_REFERENCE.items():
                if k not in explicit:
                    setattr(ns, k, v)
        return ns, rest


def _parser():
    p = _Parser(description='Hand-Object Pose Estimation (MI355X hot path)')
    p.add_argument('--mode', type=str, default='train', choices=['train', 'eval', 'infer'])
    p.add_argument('--eval_full', action='store_true')
    p.add_argument('--eval_best', action='store_true')
    p.add_argument('--eval_physics', action='store_true')
    p.add_argument('--physics_contact_thresh', type=float, default=0.005)
    p.add_argument('--eval_volume', action='store_true')
    p.add_argument('--physics_voxel_pitch', type=float, default=0.005)
    p.add_argument('--eval_hand_bench', action='store_true')
    p.add_argument('--eval_symmetric', action='store_true')
    p.add_argument('--max_sym_disc_step', type=float, default=0.01)
    p.add_argument('--eval_grasp', action='store_true')
    p.add_argument('--mark', type=str, default='')
    p.add_argument('--random_seed', type=int, default=0)
    p.add_argument('--output_dir', type=str, default='output')
    p.add_argument('--checkpoint', type=str, default='')
    p.add_argument('--pretrain', type=str, default='')
    p.add_argument('--remove_pretrained_keys', nargs='+', default=[])
    p.add_argument('--dataset_name', type=str, default='dexycb', choices=['dexycb', 'ho3d'])
    p.add_argument('--clean_data_mode', type=str, default='2023_CVPR_HFL', choices=list(CLEAN_DATA_MODES))
    p.add_argument('--patch_size', type=int, default=256)
    p.add_argument('--batch_size', type=int, default=64)
    p.add_argument('--eval_batch_size', type=int, default=32)
    p.add_argument('--num_batches', type=int, default=4)
    p.add_argument('--model', type=str, default='vpho_net', choices=['vpho_net'])
    p.add_argument('--sde_mode', type=str, choices=['ve'], default='ve')
    p.add_argument('--repeat_num', type=int, default=20)
    p.add_argument('--sampler', type=str, choices=['ode'], default='ode')
    p.add_argument('--sampling_steps', type=int, default=500)
    p.add_argument('--heatmap_size', type=int, default=64)
    p.add_argument('--roi_size', type=int, default=32)
    p.add_argument('--sample_T0', type=float, default=0.65)
    p.add_argument('--sample_num', type=int, default=50)
    p.add_argument('--topk_hand', type=int, default=15)
    p.add_argument('--topk_obj', type=int, default=5)
    p.add_argument('--do_weighted_average', action='store_false')          # the reference's spelling (args.py:233): the flag turns it OFF
    p.add_argument('--aggregation_mode_hand', type=str, default='heatmap_cascade', choices=list(AGGREGATION_MODES_HAND))
    p.add_argument('--aggregation_mode_obj', type=str, default='heatmap_cascade', choices=list(AGGREGATION_MODES_OBJ))
    p.add_argument('--asset_root', type=str, default='asset')
    p.add_argument('--base_learning_rate', type=float, default=2e-4)
    p.add_argument('--gradient_clip', type=float, default=-1.)
    p.add_argument('--train_scope', type=str, default='full', choices=['full', 'score'])
    p.add_argument('--weight_diff_hand_loss', type=float, default=1.0)
    p.add_argument('--weight_diff_obj_loss', type=float, default=1.0)
    p.add_argument('--weight_hm_hand_loss', type=float, default=1e3)
    p.add_argument('--weight_hm_obj_loss', type=float, default=1e3)
    p.add_argument('--weight_vert_loss', type=float, default=1e4)
    p.add_argument('--weight_joint_loss', type=float, default=1e4)
    p.add_argument('--weight_mano_pose_loss', type=float, default=10)
    p.add_argument('--weight_mano_shape_loss', type=float, default=1.0)
    p.add_argument('--weight_force_loss', type=float, default=1.0)
    p.add_argument('--weight_gravity_loss', type=float, default=1.0)
    p.add_argument('--weight_torque_loss', type=float, default=30.0)
    p.add_argument('--weight_supervised_loss', type=float, default=10)
    p.add_argument('--weight_CoM_loss', type=float, default=1e2)
    p.add_argument('--cross_dropout', type=float, default=0.1)
    p.add_argument('--max_epochs', type=int, default=None)
    p.add_argument('--optimizer', type=str, default='adamw', choices=['adamw', 'adam'])
    p.add_argument('--scheduler', type=str, default='exp', choices=['exp', 'cosine', 'step'])
    p.add_argument('--gamma', type=float, default=0.96)
    p.add_argument('--lr_step', type=int, default=5)
    p.add_argument('--gradient_accumulation_steps', type=int, default=1)
    p.add_argument('--print_freq', type=int, default=500)
    p.add_argument('--ema_rate', type=float, default=0.0)
    p.add_argument('--use_ema', action='store_true')
    p.add_argument('--frame_source', type=str, default='none')
    p.add_argument('--bbox_scale_factor', type=float, default=1.2)
    p.add_argument('--center_jittering', type=float, default=0.2)
    p.add_argument('--scale_factor', type=float, default=0.2)
    p.add_argument('--max_rot', type=float, default=30.0)
    p.add_argument('--rot_prob', type=float, default=1.0)
    p.add_argument('--RGB_shift_prob', type=float, default=0.5)
    p.add_argument('--shift_limit', type=float, nargs=2, default=(-20.0, 20.0))          # the reference's default pair, settable as two numbers
    p.add_argument('--color_jitter_prob', type=float, default=0.5)
    p.add_argument('--brightness', type=float, nargs=2, default=(0.6, 1.3))
    p.add_argument('--saturation', type=float, nargs=2, default=(0.6, 1.3))
    p.add_argument('--random_erasing_prob', type=float, default=0.5)
    p.add_argument('--random_erasing_min_area', type=float, default=0.02)
    p.add_argument('--random_erasing_max_area', type=float, default=0.2)
    p.add_argument('--random_erasing_max_count', type=int, default=1)
    p.add_argument('--heatmap_hand_sigma', type=float, default=2.0)
    p.add_argument('--heatmap_obj_sigma', type=float, default=2.0)
    p.add_argument('--photo_aug', type=str, default='none', choices=['none', 'reference'])
    p.add_argument('--clahe_p', type=float, default=0.0, action=_Explicit)
    p.add_argument('--clahe_clip_limit', type=float, nargs=2, default=(1.0, 4.0))
    p.add_argument('--jitter_contrast', type=float, nargs=2, default=(1.0, 1.0), action=_Explicit)
    p.add_argument('--jitter_hue', type=float, nargs=2, default=(0.0, 0.0), action=_Explicit)
    p.add_argument('--blur_p', type=float, default=0.0, action=_Explicit)
    p.add_argument('--blur_limit', type=int, nargs=2, default=(3, 7))
    p.add_argument('--sigma_limit', type=float, nargs=2, default=(0.2, 2.0))
    p.add_argument('--motion_blur_p', type=float, default=0.0, action=_Explicit)
    p.add_argument('--motion_blur_limit', type=int, nargs=2, default=(3, 7))
    p.add_argument('--contact_normal_distance_thresh', type=float, nargs=2, default=(-0.01, 0.01))
    p.add_argument('--contact_vertical_distance_thresh', type=float, default=0.005)
    p.add_argument('--frame_contact', action='store_true')
    p.add_argument('--infer_render', type=int, default=0)
    return p


cfg = Config()
_args, _unknown = _parser().parse_known_args(sys.argv[1:])
for _k, _v in vars(_args).items():
    if hasattr(cfg, _k):
        setattr(cfg, _k, _v)
    else:
        raise ValueError(f"Invalid config key: {_k}")
