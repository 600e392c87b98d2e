"""Inputs of the physics-branch training golden (tests/golden/golden_physics_train.npz), shared by tests/test_gpu_train_physics.py and the
CPU check of the physics-loss reference in tests/test_leaf_fp64_cpu.py.  numpy / torch on the CPU only."""
import numpy as np
import torch

BS = 6
W = dict(force_loss=1.0, gravity_loss=1.0, torque_loss=30.0, supervised_loss=10.0, CoM_loss=100.0)


def inputs(assets):
    """the generator's inputs (tests/golden/make_golden_physics_train.py::inputs)"""
    g = np.random.default_rng(123)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    grav = g.normal(size=(BS, 1, 3))
    grav /= np.linalg.norm(grav, axis=-1, keepdims=True)
    vert = np.asarray(assets['mano']['v_template'])[None] + g.normal(size=(BS, 778, 3)) * 0.002 + np.array([0.02, -0.01, 0.7])
    return dict(st_h=f32(g.normal(size=(BS, 256, 8, 8)) * 0.2), st_o=f32(g.normal(size=(BS, 256, 8, 8)) * 0.2), gravity=f32(grav),
                gt_vert=f32(vert), gt_CoM=f32(np.array([0.05, 0.0, 0.7]) + g.normal(size=(BS, 1, 3)) * 0.02),
                gt_force_local=f32(g.normal(size=(BS, 32, 3)) * 0.1), is_grasped=torch.from_numpy(g.random(BS) < 0.7))
