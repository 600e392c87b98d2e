"""Column names shared by the device metric kernels and the host-side tables (importable without the HIP library)."""
OBJ_METRIC_NAMES = ('MCE', 'OCE', 'MCE2', 'ADD', 'ADDS', 'ADD01d', 'ADDS01d', 'REP', 'REP5', 'CD',
                    'FSCORE@2mm', 'FSCORE@5mm', 'FSCORE@10mm', 'FSCORE@2cm', 'FSCORE@5cm', 'FSCORE@10cm')
HAND_METRIC_NAMES = ('MJE', 'PA_MJE', 'MVE', 'PA_MVE')
# Column blocks of the per-image evaluation rows (evaluate.metric_rows); WHERE each block lies is eval_layout.BLOCKS' business alone.
# the block every row has: global image index, MJE (mm) of the regression hand / the first hypothesis / the aggregated hand, MVE of the
# aggregated hand, |agg - regression| mean joint distance (mm), object translation norm (m), is_right, PA-MJE (regression), PA-MJE
# (aggregated), PA-MVE (aggregated), 0, then the 16 object metrics of the aggregated pose (TesterObject, test.py:240-503)
BASE_COLUMNS = ('image_index', 'MJE_reg', 'MJE_first', 'MJE_agg', 'MVE_agg', 'agg_reg_joint_dist_mm', 'obj_translation_norm_m', 'is_right',
                'PA_MJE_reg', 'PA_MJE_agg', 'PA_MVE_agg', 'zero') + tuple(f'object/{k}' for k in OBJ_METRIC_NAMES)
# the block of eval_best: three hand tables (mm), then three object tables
# (OBJ_METRIC_NAMES units: metres / pixels / {0,1} / [0,1]); one_candidate = hypothesis 0, best_of_S = per-image min over the S
# hypotheses (max for the hit rates and F-scores, TesterObject.postprocess), mean_of_S = per-image mean over the S hypotheses
MULTI_TABLES = ('one_candidate', 'best_of_S', 'mean_of_S')
MULTI_COLUMNS = tuple(f'{t}/hand/{k}' for t in MULTI_TABLES for k in HAND_METRIC_NAMES) + \
    tuple(f'{t}/object/{k}' for t in MULTI_TABLES for k in OBJ_METRIC_NAMES)
# the block of eval_physics: penetration and
# contact (physics_eval) of the aggregated hand vertices with the aggregated object pose ('pred'), then of the
# ground-truth hand vertices with the ground-truth object pose ('gt', NaN without object ground truth); per image PD (m), the number of
# hand vertices inside the object, the smallest signed distance (m) and contact (min sd <= cfg.physics_contact_thresh)
PHYSICS_SOURCES = ('pred', 'gt')
PHYSICS_METRIC_NAMES = ('PD', 'n_inside', 'min_sd', 'contact')
PHYSICS_COLUMNS = tuple(f'physics/{s}/{k}' for s in PHYSICS_SOURCES for k in PHYSICS_METRIC_NAMES)
# the summarize / EVAL_JSON table 'physics', per source: mean PD (mm), largest PD (mm), share of images with a vertex inside (%), mean
# number of inside vertices, share of images in contact (%)
PHYSICS_TABLE = ('PD_mm', 'PD_max_mm', 'penetration_rate_pct', 'inside_verts', 'contact_rate_pct')
# the block of eval_best AND eval_physics (physics_multi): the same four values for every sampled hypothesis (hand
# candidate s against object candidate s), per image reduced to hypothesis 0, best-of-S (min PD, min n_inside, MAX min_sd: the least
# penetrating hypothesis, max contact) and mean-of-S (contact becomes the fraction of hypotheses in contact); the 'physics' table gains
# the three MULTI_TABLES entries beside 'pred' and 'gt', each with the PHYSICS_TABLE keys
PHYSICS_MULTI_COLUMNS = tuple(f'physics/{t}/{k}' for t in MULTI_TABLES for k in PHYSICS_METRIC_NAMES)
# the block of eval_volume: the hand-object intersection volume of the
# aggregated hand mesh with the aggregated object pose ('pred'), then of the ground-truth pair ('gt', NaN without object ground truth);
# per image IV (m^3) and the number of solid cells of the object inside the hand (IV = cells * cfg.physics_voxel_pitch^3)
VOLUME_COLUMNS = ('pred_IV_m3', 'pred_cells', 'gt_IV_m3', 'gt_cells')
# the summarize / EVAL_JSON table 'volume', per source: mean IV (cm^3), largest IV (cm^3), share of images with a cell inside (%)
VOLUME_TABLE = ('IV_cm3', 'IV_max_cm3', 'intersecting_pct')
# the block of eval_best AND eval_volume (volume_multi): the
# intersection volume of every sampled hypothesis (hand candidate s against object candidate s), per image reduced to hypothesis 0,
# best-of-S (the minima) and mean-of-S (mean_cells = integer sum / S, mean_IV = pitch^3 * mean_cells); the 'volume' table gains the three
# MULTI_TABLES entries beside 'pred' and 'gt', each with the VOLUME_TABLE keys
VOLUME_MULTI_COLUMNS = ('one_IV_m3', 'one_cells', 'best_IV_m3', 'best_cells', 'mean_IV_m3', 'mean_cells')
# the hand benchmark block (--eval_hand_bench): the HO3D / FreiHAND leaderboard values of a (hand, ground truth) pair, all
# in [0, 1]: the AUC of the PCK curve over HAND_BENCH_AUC = np.linspace(lo, hi, n) metres for joints and vertices and the vertex F-score at
# the HAND_BENCH_F_THRESH distances (metres), each raw and after the similarity alignment ('PA')
HAND_BENCH_NAMES = ('AUC_J', 'PA_AUC_J', 'AUC_V', 'PA_AUC_V', 'F@5', 'F@15', 'PA_F@5', 'PA_F@15')
HAND_BENCH_F_THRESH = (0.005, 0.015)
HAND_BENCH_AUC = (0.0, 0.05, 100)
# evaluate.hand_bench_block: the eight values of the aggregated hand, then of the regression hand (16 columns)
HAND_BENCH_SOURCES = ('agg', 'reg')
HAND_BENCH_COLUMNS = tuple(f'hand_bench/{s}/{k}' for s in HAND_BENCH_SOURCES for k in HAND_BENCH_NAMES)
# evaluate.hand_bench_multi_block (eval_best AND eval_hand_bench): every sampled hypothesis, per image reduced to hypothesis 0, best-of-S
# (the MAXIMUM of each value on its own) and mean-of-S (24 columns)
HAND_BENCH_MULTI_COLUMNS = tuple(f'hand_bench/{t}/{k}' for t in MULTI_TABLES for k in HAND_BENCH_NAMES)
# the keys of every source of the summarize-level / EVAL_JSON table 'hand_bench': means over the images
HAND_BENCH_TABLE = HAND_BENCH_NAMES
# the symmetry-aware object errors (--eval_symmetric) of a (pose, ground truth) pair over the object's padded symmetry
# table: SMCE (m; TesterObject.criterion_SMCE, test.py:377-398), MSSD (m; min over the symmetries of the largest vertex distance) and
# MSSD < 0.1 * diameter ({0, 1}; as ADD01d is to ADD)
SYM_METRIC_NAMES = ('SMCE', 'MSSD', 'MSSD01d')
# evaluate.symmetric_block: the three values of the aggregated object pose (NaN without object ground truth)
SYM_COLUMNS = tuple(f'sym/pred/{k}' for k in SYM_METRIC_NAMES)
# evaluate.symmetric_multi_block (eval_best AND eval_symmetric): every sampled object hypothesis, per image reduced to hypothesis 0,
# best-of-S (min SMCE, min MSSD, max hit: TesterObject.postprocess) and mean-of-S (9 columns)
SYM_MULTI_COLUMNS = tuple(f'sym/{t}/{k}' for t in MULTI_TABLES for k in SYM_METRIC_NAMES)
# the contact-map and grasp agreement (--eval_grasp) of a (hand, object pose) pair with the annotated pair, both hand
# contact maps made by the same kernel: with c = (weight > 0) and g = (annotation's weight > 0) over the filled hand vertices IoU,
# precision, recall and F1 of c against g (NaN where the denominator is 0), MAE = mean |weight - annotation's weight|, anchor_agree = the
# share of the 32 anchors with equal pooled contact state, grasped = the pair's own is_grasped, grasp_agree = (is_grasped == annotation's)
GRASP_METRIC_NAMES = ('IoU', 'precision', 'recall', 'F1', 'MAE', 'anchor_agree', 'grasped', 'grasp_agree')
# evaluate.grasp_block: the eight values of the aggregated hand with the aggregated object pose (NaN without object ground truth)
GRASP_COLUMNS = tuple(f'grasp/pred/{k}' for k in GRASP_METRIC_NAMES)
# evaluate.grasp_multi_block (eval_best AND eval_grasp): every sampled hypothesis (hand candidate s with object candidate s), per image
# reduced to hypothesis 0, best-of-S (each value's maximum on its own, MAE's minimum) and mean-of-S, NaN hypotheses left out (24 columns)
GRASP_MULTI_COLUMNS = tuple(f'grasp/{t}/{k}' for t in MULTI_TABLES for k in GRASP_METRIC_NAMES)
# the keys of every source of the summarize-level / EVAL_JSON table 'grasp': each value's mean over the images where it is defined (NaN
# where it never is), then the share of images where IoU is defined
GRASP_TABLE = GRASP_METRIC_NAMES + ('IoU_defined',)
