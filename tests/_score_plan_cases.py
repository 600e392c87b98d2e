"""The plans of vpho_amd/csrc/score_plan.h that the suite relies on, as literals: id -> (case, plan), both in the words of
tests/_score_plan_probe.cpp (its header explains the case line; `slots` defaults to 512 = two workgroups on each of 256 CUs).

tests/test_score_plan_cpu.py compares every entry with what the header plans, without a device.  The plans were recorded when the plan
functions were split from `eval_net` and were checked against that function as it stood before (docs/LOG.md, "Sampler plans"); a
threshold that moves shows up here as a changed literal -- and then the GPU test named in the id needs a new shape for its kernel.

  a_*  shapes of tests/test_gpu_sampler.py and tests/test_gpu_head_epilogue.py whose docstrings name a kernel or a tile split
  b_*  one case per pose-encoder kernel (rows x n1), per head family, and per outcome of the tail-tile rule
  c_*  every switch value, and the slot counts of other devices
  d_*  refusals, with their text
  e_*  workspace bytes; every slice starts on a multiple of 256 bytes
  f_*  the Dormand-Prince tableau, the six stage combinations, the t_eval stamps
"""

CASES = {
    'a_pe_readme_64x100_hand': (
        'pe R=6400 D=96 Dp=96',
        'rc=0 rows=32 n1=3 grid=200 lds=35328 flops=1153433600 name=pose_encoder_reg_kernel'),
    'a_pe_readme_64x100_obj': (
        'pe R=6400 D=9 Dp=12',
        'rc=0 rows=32 n1=1 grid=200 lds=35328 flops=943718400 name=pose_encoder_reg_kernel'),
    'a_pe_3x50_hand': (
        'pe R=150 D=96 Dp=96',
        'rc=0 rows=32 n1=3 grid=5 lds=35328 flops=27033600 name=pose_encoder_reg_kernel'),
    'a_pe_3x50_obj': (
        'pe R=150 D=9 Dp=12',
        'rc=0 rows=32 n1=1 grid=5 lds=35328 flops=22118400 name=pose_encoder_reg_kernel'),
    'a_pe_3x700_hand': (
        'pe R=2100 D=96 Dp=96',
        'rc=0 rows=32 n1=3 grid=66 lds=35328 flops=378470400 name=pose_encoder_reg_kernel'),
    'a_pe_3x2129_hand': (
        'pe R=6387 D=96 Dp=96',
        'rc=0 rows=32 n1=3 grid=200 lds=35328 flops=1151090688 name=pose_encoder_reg_kernel'),
    'a_pe_64x256_hand_64_rows_by_default': (
        'pe R=16384 D=96 Dp=96',
        'rc=0 rows=64 n1=3 grid=256 lds=68608 flops=2952790016 name=pose_encoder_reg64_kernel'),
    'a_pe_64x256_obj_64_rows_by_default': (
        'pe R=16384 D=9 Dp=12',
        'rc=0 rows=64 n1=1 grid=256 lds=68608 flops=2415919104 name=pose_encoder_reg64_kernel'),
    'a_head_readme_64x100_hand': (
        'head R=6400 S=100 nheads=32',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'a_head_readme_64x100_obj': (
        'head R=6400 S=100 nheads=3',
        'rc=0 family=plain cb=1 full=50 tail=0 grid=150 lds=57344 flops=2546073600 name=score_head_kernel'),
    'a_head_tail_tiles_3x2129_hand': (
        'head R=6387 S=2129 nheads=32',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27102953472 name=score_head_kernel'),
    'a_head_3x50_hand': (
        'head R=150 S=50 nheads=32',
        'rc=0 family=plain cb=0 full=2 tail=0 grid=64 lds=57344 flops=636518400 name=score_head_kernel'),
    'a_head_3x50_obj': (
        'head R=150 S=50 nheads=3',
        'rc=0 family=plain cb=0 full=2 tail=0 grid=6 lds=57344 flops=59673600 name=score_head_kernel'),
    'a_head_3x700_hand_17_tiles_one_past_a_round': (
        'head R=2100 S=700 nheads=32',
        'rc=0 family=plain cb=1 full=16 tail=2 grid=576 lds=57344 flops=8911257600 name=score_head_kernel'),
    'a_head_64x256_hand': (
        'head R=16384 S=256 nheads=32',
        'rc=0 family=plain cb=1 full=128 tail=0 grid=4096 lds=57344 flops=69524783104 name=score_head_kernel'),
    'a_head_250x2_ordinary_tiles_only': (
        'head R=500 S=250 nheads=32',
        'rc=0 family=plain cb=1 full=4 tail=0 grid=128 lds=57344 flops=2121728000 name=score_head_kernel'),
    'b_pe_8192_last_32_row_launch': (
        'pe R=8192 D=96 Dp=96',
        'rc=0 rows=32 n1=3 grid=256 lds=35328 flops=1476395008 name=pose_encoder_reg_kernel'),
    'b_pe_8193_first_64_row_launch': (
        'pe R=8193 D=96 Dp=96',
        'rc=0 rows=64 n1=3 grid=129 lds=68608 flops=1476575232 name=pose_encoder_reg64_kernel'),
    'b_pe_32_rows_n1_2': (
        'pe R=6400 D=63 Dp=64',
        'rc=0 rows=32 n1=2 grid=200 lds=35328 flops=1048576000 name=pose_encoder_reg_kernel'),
    'b_pe_32_rows_n1_4': (
        'pe R=6400 D=126 Dp=128',
        'rc=0 rows=32 n1=4 grid=200 lds=35328 flops=1258291200 name=pose_encoder_reg_kernel'),
    'b_pe_64_rows_n1_1': (
        'pe R=8193 D=9 Dp=12',
        'rc=0 rows=64 n1=1 grid=129 lds=68608 flops=1208107008 name=pose_encoder_reg64_kernel'),
    'b_pe_64_rows_n1_2': (
        'pe R=8193 D=63 Dp=64',
        'rc=0 rows=64 n1=2 grid=129 lds=68608 flops=1342341120 name=pose_encoder_reg64_kernel'),
    'b_pe_64_rows_n1_4': (
        'pe R=8193 D=126 Dp=128',
        'rc=0 rows=64 n1=4 grid=129 lds=68608 flops=1610809344 name=pose_encoder_reg64_kernel'),
    'b_pe_one_row': (
        'pe R=1 D=96 Dp=96',
        'rc=0 rows=32 n1=3 grid=1 lds=35328 flops=180224 name=pose_encoder_reg_kernel'),
    'b_head_25600_obj_tail_tiles': (
        'head R=25600 S=100 nheads=3',
        'rc=0 family=plain cb=1 full=170 tail=120 grid=870 lds=57344 flops=10184294400 name=score_head_kernel'),
    'b_head_1600_tiles_half_round_keeps_ordinary_tiles': (
        'head R=7168 S=100 nheads=32',
        'rc=0 family=plain cb=1 full=56 tail=0 grid=1792 lds=57344 flops=30417092608 name=score_head_kernel'),
    'b_head_just_below_half_round': (
        'head R=7040 S=100 nheads=32',
        'rc=0 family=plain cb=1 full=48 tail=28 grid=2432 lds=57344 flops=29873930240 name=score_head_kernel'),
    'b_head_exact_rounds': (
        'head R=8192 S=128 nheads=32',
        'rc=0 family=plain cb=1 full=64 tail=0 grid=2048 lds=57344 flops=34762391552 name=score_head_kernel'),
    'b_head_one_row': (
        'head R=1 S=1 nheads=32',
        'rc=0 family=plain cb=0 full=1 tail=0 grid=32 lds=57344 flops=4243456 name=score_head_kernel'),
    'b_head_split6': (
        'head R=6400 S=100 nheads=32 split_terms=6 planes=1',
        'rc=0 family=split6 cb=0 full=48 tail=8 grid=1792 lds=73728 flops=27158118400 name=score_head_split_kernel'),
    'b_head_split9': (
        'head R=6400 S=100 nheads=32 split_terms=9 planes=1',
        'rc=0 family=split9 cb=0 full=48 tail=8 grid=1792 lds=73728 flops=27158118400 name=score_head_split_kernel'),
    'b_head_split9_small': (
        'head R=150 S=50 nheads=3 split_terms=9 planes=1',
        'rc=0 family=split9 cb=0 full=2 tail=0 grid=6 lds=73728 flops=59673600 name=score_head_split_kernel'),
    'b_head_split6_without_planes_is_plain': (
        'head R=6400 S=100 nheads=32 split_terms=6 planes=0',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'b_head_split7_is_plain': (
        'head R=6400 S=100 nheads=32 split_terms=7 planes=1',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'b_head_cb_on_at_64': (
        'head R=320 S=64 nheads=32',
        'rc=0 family=plain cb=1 full=3 tail=0 grid=96 lds=57344 flops=1357905920 name=score_head_kernel'),
    'b_head_cb_off_at_63': (
        'head R=315 S=63 nheads=32',
        'rc=0 family=plain cb=0 full=3 tail=0 grid=96 lds=57344 flops=1336688640 name=score_head_kernel'),
    'c_pe_rows64_forced_at_6387': (
        'pe R=6387 D=96 Dp=96 pe_rows=64',
        'rc=0 rows=64 n1=3 grid=100 lds=68608 flops=1151090688 name=pose_encoder_reg64_kernel'),
    'c_pe_rows32_forced_at_16384': (
        'pe R=16384 D=96 Dp=96 pe_rows=32',
        'rc=0 rows=32 n1=3 grid=512 lds=35328 flops=2952790016 name=pose_encoder_reg_kernel'),
    'c_pe_rows48_is_the_32_row_kernel': (
        'pe R=16384 D=96 Dp=96 pe_rows=48',
        'rc=0 rows=32 n1=3 grid=512 lds=35328 flops=2952790016 name=pose_encoder_reg_kernel'),
    'c_pe_rows64_forced_obj': (
        'pe R=150 D=9 Dp=12 pe_rows=64',
        'rc=0 rows=64 n1=1 grid=3 lds=68608 flops=22118400 name=pose_encoder_reg64_kernel'),
    'c_head_cb0': (
        'head R=6400 S=100 nheads=32 head_cb=0',
        'rc=0 family=plain cb=0 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_cb1': (
        'head R=6400 S=100 nheads=32 head_cb=1',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_epi0_cb_on': (
        'head R=6400 S=100 nheads=32 head_epi=0',
        'rc=0 family=epi0 cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_epi0_cb_off': (
        'head R=150 S=50 nheads=32 head_epi=0',
        'rc=0 family=epi0 cb=0 full=2 tail=0 grid=64 lds=57344 flops=636518400 name=score_head_kernel'),
    'c_head_epi0_cb0': (
        'head R=6400 S=100 nheads=32 head_epi=0 head_cb=0',
        'rc=0 family=epi0 cb=0 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_epi1': (
        'head R=6400 S=100 nheads=32 head_epi=1',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_epi0_leaves_the_split_kernel': (
        'head R=6400 S=100 nheads=32 split_terms=6 planes=1 head_epi=0 head_cb=0',
        'rc=0 family=split6 cb=0 full=48 tail=8 grid=1792 lds=73728 flops=27158118400 name=score_head_split_kernel'),
    'c_head_tail0': (
        'head R=6400 S=100 nheads=32 head_tail=0',
        'rc=0 family=plain cb=1 full=50 tail=0 grid=1600 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_tail1': (
        'head R=6400 S=100 nheads=32 head_tail=1',
        'rc=0 family=plain cb=1 full=48 tail=8 grid=1792 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_tail0_split': (
        'head R=6400 S=100 nheads=32 split_terms=9 planes=1 head_tail=0',
        'rc=0 family=split9 cb=0 full=50 tail=0 grid=1600 lds=73728 flops=27158118400 name=score_head_split_kernel'),
    'c_head_slots_208': (
        'head R=6400 S=100 nheads=32 slots=208',
        'rc=0 family=plain cb=1 full=50 tail=0 grid=1600 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_slots_608': (
        'head R=6400 S=100 nheads=32 slots=608',
        'rc=0 family=plain cb=1 full=50 tail=0 grid=1600 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_slots_16': (
        'head R=6400 S=100 nheads=32 slots=16',
        'rc=0 family=plain cb=1 full=50 tail=0 grid=1600 lds=57344 flops=27158118400 name=score_head_kernel'),
    'c_head_slots_208_tail_tiles': (
        'head R=7000 S=100 nheads=32 slots=208',
        'rc=0 family=plain cb=1 full=52 tail=11 grid=2016 lds=57344 flops=29704192000 name=score_head_kernel'),
    'c_head_slots_unknown': (
        'head R=6400 S=100 nheads=32 slots=-1',
        'rc=1 need_slots=1 error='),
    'c_head_slots_unknown_split': (
        'head R=6400 S=100 nheads=32 split_terms=6 planes=1 slots=-1',
        'rc=1 need_slots=1 error='),
    'd_pe_dp_132': (
        'pe R=6400 D=130 Dp=132',
        'rc=1 error=pose encoder: input dimension 130 (padded 132) not supported (<= 128, multiple of 4)'),
    'd_pe_dp_98': (
        'pe R=6400 D=96 Dp=98',
        'rc=1 error=pose encoder: input dimension 96 (padded 98) not supported (<= 128, multiple of 4)'),
    'd_head_32_bit_offsets': (
        'head R=3906250 S=100 nheads=32',
        'rc=1 need_slots=0 error=score head: 3906250 hypothesis rows exceed the 32-bit buffer offsets'),
    'd_head_32_bit_offsets_last_accepted': (
        'head R=3906249 S=100 nheads=3',
        'rc=0 family=plain cb=1 full=30518 tail=0 grid=91554 lds=57344 flops=1553999602176 name=score_head_kernel'),
    'd_head_32_bit_offsets_before_the_slots': (
        'head R=3906250 S=100 nheads=32 slots=-1',
        'rc=1 need_slots=0 error=score head: 3906250 hypothesis rows exceed the 32-bit buffer offsets'),
    'e_ws_hand_64x100': (
        'ws D=96 Dp=96 nheads=32 bs=64 S=100',
        'bytes=47481856 sizing=47481856 slices=16 aligned=1 ascending=1 first=0 last=47465472'),
    'e_ws_obj_64x100': (
        'ws D=9 Dp=12 nheads=3 bs=64 S=100',
        'bytes=16466944 sizing=16466944 slices=16 aligned=1 ascending=1 first=0 last=16450560'),
    'e_ws_hand_1x1': (
        'ws D=96 Dp=96 nheads=32 bs=1 S=1',
        'bytes=368896 sizing=368896 slices=16 aligned=1 ascending=1 first=0 last=352512'),
    'e_ws_hand_3x2129': (
        'ws D=96 Dp=96 nheads=32 bs=3 S=2129',
        'bytes=45391872 sizing=45391872 slices=16 aligned=1 ascending=1 first=0 last=45375488'),
    'f_tableau': (
        'tableau',
        'a_rows_sum_to_c=1 b_sums_to_1=1 e_sums_to_0=1 p_at_1_is_b=1 rkctl_bytes=320 max_steps=1024 log_cap=512'),
    'f_comb_stage_1': (
        'comb s=1',
        'n=1 h=0 c=0.20000000000000001,0,0,0,0,0,0 at=0.20000000000000001'),
    'f_comb_stage_2': (
        'comb s=2',
        'n=2 h=0 c=0.074999999999999997,0.22500000000000001,0,0,0,0,0 at=0.29999999999999999'),
    'f_comb_stage_3': (
        'comb s=3',
        'n=3 h=0 c=0.97777777777777775,-3.7333333333333334,3.5555555555555554,0,0,0,0 at=0.80000000000000004'),
    'f_comb_stage_4': (
        'comb s=4',
        'n=4 h=0 c=2.9525986892242035,-11.595793324188385,9.8228928516994358,-0.29080932784636487,0,0,0 at=0.88888888888888884'),
    'f_comb_stage_5': (
        'comb s=5',
        'n=5 h=0 c=2.8462752525252526,-10.757575757575758,8.9064227177434727,0.27840909090909088,-0.2735313036020583,0,0 at=1'),
    'f_comb_stage_6': (
        'comb s=6',
        'n=6 h=0 c=0.091145833333333329,0,0.44923629829290207,0.65104166666666663,-0.322376179245283,0.13095238095238096,0 at=1'),
    'f_teval_one_stamp': (
        'teval T0=0.65 eps=1e-05 n=1',
        'n=1 te=0.65000000000000002'),
    'f_teval_two_stamps': (
        'teval T0=0.65 eps=1e-05 n=2',
        'n=2 te=0.65000000000000002,1.0000000000000001e-05'),
    'f_teval_five_stamps_end_point_exact': (
        'teval T0=0.65 eps=1e-05 n=5',
        'n=5 te=0.65000000000000002,0.48750250000000001,0.32500499999999999,0.16250749999999997,1.0000000000000001e-05'),
    'f_teval_twelve_stamps': (
        'teval T0=1 eps=1e-05 n=12',
        'n=12 te=1,0.90909181818181817,0.81818363636363634,0.7272754545454545,0.63636727272727267,0.54545909090909084,0.45455090909090912,0.36364272727272728,0.27273454545454545,0.18182636363636362,0.090918181818181787,1.0000000000000001e-05'),
}

# tests/test_gpu_sampler.py::test_score_launches_are_the_ones_the_plan_table_names scores these on the device under profiling:
# (network, images, hypotheses per image, pose-encoder case, head case); one launch of each per evaluation, with the table's flops
GPU_CASES = [('hand', 3, 50, 'a_pe_3x50_hand', 'a_head_3x50_hand'),
             ('hand', 3, 700, 'a_pe_3x700_hand', 'a_head_3x700_hand_17_tiles_one_past_a_round'),
             ('obj', 3, 50, 'a_pe_3x50_obj', 'a_head_3x50_obj')]
