"""The launch plans of vpho_amd/csrc/conv_plan.h that the suite relies on, as literals: id -> (descriptor, plan), both in the words of
tests/_conv_plan_probe.cpp (its header explains the descriptor line; `slots` defaults to 512 = two workgroups on each of 256 CUs).

tests/test_conv_plan_cpu.py compares every entry with what the header plans, without a device.  The plans were recorded when the plan
functions were split from the launchers and were checked against the launchers as they stood before (docs/LOG.md, "Convolution plans");
a threshold that moves shows up here as a changed literal -- and then the GPU test named in the id needs a new shape for its class.

  a_*  shapes of tests/test_gpu_conv.py, test_gpu_bn_fuse.py and test_gpu_bn_stats_fp64.py whose docstrings name a kernel or a tile class
  b_*  one small shape per kernel family and tile, operand form and BatchNorm-epilogue outcome
  c_*  every switch value that changes a plan
  d_*  refusals, with their text
  e_*  weight gradient: tile, pixel slices, the order of the slice sum, workspace bytes = splits * Cout * K * 4
  f_*  Winograd: input staging mode, BatchNorm kernels, block count
"""

CASES = {
    'a_prologue_16_32_256_256': (
        'conv N=16 H=32 Cin=256 Cout=256 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=glds_pre tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_prologue_9_31_128_64': (
        'conv N=9 H=31 Cin=128 Cout=64 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=glds_pre tile=64x64 threads=256 grid=136x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=128 tiles=136x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_prologue_3_17_512_128': (
        'conv N=3 H=17 Cin=512 Cout=128 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=glds_pre tile=64x64 threads=256 grid=32x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=512 tiles=14x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_prologue_2_8_544_64': (
        'conv N=2 H=8 Cin=544 Cout=64 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=reg tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=544 tiles=2x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_16_32_64_256': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 res=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_16_32_32_256': (
        'conv N=16 H=32 Cin=32 Cout=256 bias=1 res=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=32 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_8_16_128_512': (
        'conv N=8 H=16 Cin=128 Cout=512 bias=1 res=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=256x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=128 tiles=32x8 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_5_13_96_192': (
        'conv N=5 H=13 Cin=96 Cout=192 bias=1 res=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=48x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=96 tiles=14x3 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_3_9_256_64': (
        'conv N=3 H=9 Cin=256 Cout=64 bias=1 res=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=4x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_64_8_512_2048': (
        'conv N=64 H=8 Cin=512 Cout=2048 bias=1 res=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=512 tiles=32x16 uni=1 vec=1 lin=11 dbg=0'),
    'a_residual_16_32_64_256_dbg8': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 res=1 dbg=8',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=8'),
    'a_bn_fuse_64_32_32_64_256': (
        'conv N=64 H=32 W=32 Cin=64 Cout=256 bias=1 stats=1 stats_rows=1 stats_cap=1024',
        'rc=0 family=pers_bn tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=512 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=512x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_fuse_16_16_16_256_64': (
        'conv N=16 H=16 W=16 Cin=256 Cout=64 bias=1 stats=1 stats_rows=1 stats_cap=64',
        'rc=0 family=glds tile=64x64 threads=256 grid=64x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=64 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=64x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_fuse_2_9_7_32_40': (
        'conv N=2 H=9 W=7 Cin=32 Cout=40 bias=1 stats=1 stats_rows=1 stats_cap=2',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=2 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=32 tiles=2x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_fuse_3_8_8_36_132': (
        'conv N=3 H=8 W=8 Cin=36 Cout=132 bias=1 stats=1 stats_rows=1 stats_cap=3',
        'rc=0 family=glds tile=64x64 threads=256 grid=16x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=3 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=36 tiles=3x3 uni=0 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_61_33_33_64_256_1': (
        'conv N=61 H=33 W=33 Cin=64 Cout=256 K=1 pad=0 bias=1 stats=1 stats_rows=1 stats_cap=1038 pers=0',
        'rc=0 family=glds tile=128x128 threads=512 grid=1040x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=519 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=519x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_64_16_16_128_128_3': (
        'conv N=64 H=16 W=16 Cin=128 Cout=128 K=3 pad=1 bias=1 stats=1 stats_rows=1 stats_cap=256 pers=0',
        'rc=0 family=glds tile=128x64 threads=512 grid=256x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=128 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1152 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_63_16_17_128_128_3': (
        'conv N=63 H=16 W=17 Cin=128 Cout=128 K=3 pad=1 bias=1 stats=1 stats_rows=1 stats_cap=268 pers=0',
        'rc=0 family=glds tile=128x64 threads=512 grid=272x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=134 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1152 tiles=134x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_16_16_16_256_64_1': (
        'conv N=16 H=16 W=16 Cin=256 Cout=64 K=1 pad=0 bias=1 stats=1 stats_rows=1 stats_cap=64 pers=0',
        'rc=0 family=glds tile=64x64 threads=256 grid=64x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=64 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=64x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_2_9_7_32_40_1': (
        'conv N=2 H=9 W=7 Cin=32 Cout=40 K=1 pad=0 bias=1 stats=1 stats_rows=1 stats_cap=2 pers=0',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=2 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=32 tiles=2x1 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_3_8_8_36_132_1': (
        'conv N=3 H=8 W=8 Cin=36 Cout=132 K=1 pad=0 bias=1 stats=1 stats_rows=1 stats_cap=3 pers=0',
        'rc=0 family=glds tile=64x64 threads=256 grid=16x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=3 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=36 tiles=3x3 uni=0 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_2_10_6_16_64_3': (
        'conv N=2 H=10 W=6 Cin=16 Cout=64 K=3 pad=1 bias=1 stats=1 stats_rows=1 stats_cap=2 pers=0',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=2 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=144 tiles=2x1 uni=0 vec=1 lin=11 dbg=0'),
    'a_bn_stats_direct_3_12_12_64_128_3': (
        'conv N=3 H=12 W=12 Cin=64 Cout=128 K=3 pad=1 bias=1 stats=1 stats_rows=1 stats_cap=7 pers=0',
        'rc=0 family=glds tile=64x64 threads=256 grid=16x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=7 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=576 tiles=7x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_persistent_64_32': (
        'conv N=64 H=32 Cin=64 Cout=256 bias=1 stats=1 stats_rows=1 stats_cap=1024 pers=2',
        'rc=0 family=pers_bn tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=512 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=512x2 uni=1 vec=1 lin=11 dbg=0'),
    'a_bn_stats_persistent_61_33': (
        'conv N=61 H=33 Cin=64 Cout=256 bias=1 stats=1 stats_rows=1 stats_cap=1038 pers=2',
        'rc=0 family=pers_bn tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=519 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=519x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_glds_128x128': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_pers': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1',
        'rc=0 family=pers tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'b_glds_128x64': (
        'conv N=16 H=32 Cin=64 Cout=192 bias=1',
        'rc=0 family=glds tile=128x64 threads=512 grid=384x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x3 uni=1 vec=1 lin=11 dbg=0'),
    'b_glds_64x64': (
        'conv N=3 H=9 Cin=256 Cout=64 bias=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=4x1 uni=1 vec=1 lin=11 dbg=0'),
    'b_glds_64x64_generic_taps_cin_not_32': (
        'conv N=5 H=9 Cin=280 Cout=256 bias=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=32x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=280 tiles=7x4 uni=0 vec=1 lin=11 dbg=0'),
    'b_glds_64x64_stem_7x7': (
        'conv N=1 H=32 Cin=4 Cout=64 K=7 stride=2 pad=3 bias=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=196 tiles=4x1 uni=0 vec=1 lin=11 dbg=0'),
    'b_glds_64x64_scalar_epilogue': (
        'conv N=3 H=17 W=13 Cin=32 Cout=21 K=3 stride=2 pad=1 bias=1',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=288 tiles=3x1 uni=1 vec=0 lin=11 dbg=0'),
    'b_glds_pre_128x64': (
        'conv N=16 H=32 Cin=128 Cout=192 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=glds_pre tile=128x64 threads=512 grid=384x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=128 tiles=128x3 uni=1 vec=1 lin=11 dbg=0'),
    'b_reg_128x128_prologue_3x3': (
        'conv N=16 H=32 Cin=128 Cout=256 K=3 pad=1 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=reg tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1152 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_reg_128x64_prologue_3x3': (
        'conv N=16 H=32 Cin=128 Cout=192 K=3 pad=1 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=reg tile=128x64 threads=512 grid=384x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1152 tiles=128x3 uni=1 vec=1 lin=11 dbg=0'),
    'b_reg_64x64_prologue_table_exceeded': (
        'conv N=2 H=8 Cin=544 Cout=64 bias=1 in_scale=1 in_shift=1',
        'rc=0 family=reg tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=544 tiles=2x1 uni=1 vec=1 lin=11 dbg=0'),
    'b_split6_128x128': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=6',
        'rc=0 family=split6 tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_split9_128x64': (
        'conv N=16 H=32 Cin=64 Cout=192 bias=1 w_planes=1 plane_terms=9',
        'rc=0 family=split9 tile=128x64 threads=512 grid=384x1 prof=conv_igemm_128x64 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x3 uni=1 vec=1 lin=11 dbg=0'),
    'b_split9_64x64': (
        'conv N=3 H=9 Cin=48 Cout=64 w_planes=1 plane_terms=9',
        'rc=0 family=split9 tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=48 tiles=4x1 uni=0 vec=1 lin=11 dbg=0'),
    'b_split_refused_terms_falls_to_fp32': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=3',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_grouped_128x128': (
        'conv N=8 H=32 Cin=64 Cout=256 bias=1 groups=2 x_group=524288 w_group=16384 y_group=2097152 bias_group=256',
        'rc=0 family=glds tile=128x128 threads=512 grid=128x2 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=64x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_grouped_pers_shares_slots': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 groups=2 x_group=1048576 w_group=40960 y_group=10485760 bias_group=640',
        'rc=0 family=pers tile=128x128 threads=512 grid=256x2 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'b_grouped_shared_input_64x64': (
        'conv N=3 H=9 Cin=256 Cout=64 bias=1 groups=2 x_group=0 w_group=16384 y_group=15552 bias_group=64',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x2 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=4x1 uni=1 vec=1 lin=11 dbg=0'),
    'b_pixel_list_compact': (
        'conv N=16 H=32 Cin=128 Cout=128 K=3 pad=1 bias=1 row_map=1 row_count=1 rows_hint=4000',
        'rc=0 family=glds tile=128x64 threads=512 grid=256x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1152 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_pixel_list_scatter': (
        'conv N=16 H=32 Cin=128 Cout=128 K=3 pad=1 bias=1 row_map=1 row_count=1 rows_scatter=1',
        'rc=0 family=glds tile=128x64 threads=512 grid=256x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1152 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_splits_partial_sums': (
        'conv N=1 H=1 Cin=4096 Cout=256 splits=4 w_ld=16384 x_split=4096 w_split=4096 y_split=65536',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x4 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=4096 tiles=1x4 uni=1 vec=1 lin=11 dbg=0'),
    'b_x2_pers': (
        'conv N=64 H=64 Cin=64 Cout=256 bias=1 x2=1 Cin2=64 stride2=1 H2=64 W2=64',
        'rc=0 family=pers tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=128 tiles=2048x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_x2_stride2_64x64': (
        'conv N=5 H=9 Cin=96 Cout=192 bias=1 x2=1 Cin2=64 stride2=2 H2=18 W2=18',
        'rc=0 family=glds tile=64x64 threads=256 grid=24x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=160 tiles=7x3 uni=1 vec=1 lin=11 dbg=0'),
    'b_res_up_128x128': (
        'conv N=64 H=16 Cin=1024 Cout=256 bias=1 res_up=1 ru_H=8 ru_W=8 ru_ld=256',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1024 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_res_up_64x64': (
        'conv N=2 H=6 Cin=96 Cout=64 bias=1 res_up=1 ru_H=3 ru_W=3 ru_ld=64',
        'rc=0 family=glds tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=96 tiles=2x1 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_forward_on': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=128 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_forward_off_cap_too_small': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 stats=1 stats_rows=1 stats_cap=127',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=0 bn_on=0 drop_gate=0 drop_stats=1 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_forward_generic_taps_on': (
        'conv N=5 H=9 Cin=280 Cout=256 bias=1 stats=1 stats_rows=1 stats_cap=7',
        'rc=0 family=glds tile=64x64 threads=256 grid=32x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=7 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=280 tiles=7x4 uni=0 vec=1 lin=11 dbg=0'),
    'b_bn_forward_pers_on': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=pers_bn tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=128 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_forward_pers_off_cap': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 stats=1 stats_rows=1 stats_cap=100',
        'rc=0 family=pers tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=0 bn_on=0 drop_gate=0 drop_stats=1 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_backward_gate_recomputed': (
        'conv N=16 H=32 Cin=64 Cout=256 gate=1 bn_gamma=1 bn_beta=1 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=128 bn_on=1 drop_gate=1 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_backward_no_stored_gate': (
        'conv N=16 H=32 Cin=64 Cout=256 bn_gamma=1 bn_beta=1 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=128 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_backward_stored_gate_kept': (
        'conv N=16 H=32 Cin=64 Cout=256 gate=1 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=128 bn_on=1 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_backward_off_falls_back_to_gate': (
        'conv N=16 H=32 Cin=64 Cout=256 gate=1 bn_gamma=1 bn_beta=1 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=100',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=0 bn_on=0 drop_gate=0 drop_stats=1 drop_bn_x=1 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'b_bn_backward_off_no_gate_refused': (
        'conv N=16 H=32 Cin=64 Cout=256 bn_gamma=1 bn_beta=1 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=100',
        'rc=1 stats_rows=0 need_slots=0 error=vpho_conv2d_nhwc_f32: bn_x: the launch needs 128 partial rows (stats_cap 100) or runs a kernel without the BatchNorm epilogue (tile 1288)'),
    'c_pers0_more_tiles_than_slots': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 pers=0',
        'rc=0 family=glds tile=128x128 threads=512 grid=640x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'c_pers0_one_round': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 pers=0',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_pers1_more_tiles_than_slots': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 pers=1',
        'rc=0 family=pers tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'c_pers1_one_round': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 pers=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_pers2_more_tiles_than_slots': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 pers=2',
        'rc=0 family=pers tile=128x128 threads=512 grid=512x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=1 vec=1 lin=11 dbg=0'),
    'c_pers2_one_round': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 pers=2',
        'rc=0 family=pers tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile128': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 tile=128',
        'rc=0 family=reg tile=128x128 threads=256 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile128_split6': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=6 tile=128',
        'rc=0 family=split6 tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile1288': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 tile=1288',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile1288_split6': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=6 tile=1288',
        'rc=0 family=split6 tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile12864': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 tile=12864',
        'rc=0 family=glds tile=128x64 threads=512 grid=512x1 prof=conv_igemm_128x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x4 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile12864_split6': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=6 tile=12864',
        'rc=0 family=split6 tile=128x64 threads=512 grid=512x1 prof=conv_igemm_128x64 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x4 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile64': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 tile=64',
        'rc=0 family=glds tile=64x64 threads=256 grid=1024x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=256x4 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile64_split6': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=6 tile=64',
        'rc=0 family=split6 tile=64x64 threads=256 grid=1024x1 prof=conv_igemm_64x64 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=256x4 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile1288_ragged_cout': (
        'conv N=16 H=32 Cin=64 Cout=192 bias=1 tile=1288',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile128_bn_forward_off': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 tile=128 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=reg tile=128x128 threads=256 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=0 bn_on=0 drop_gate=0 drop_stats=1 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile128_bn_backward_falls_back_to_gate': (
        'conv N=16 H=32 Cin=64 Cout=256 gate=1 bn_gamma=1 bn_beta=1 tile=128 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=reg tile=128x128 threads=256 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=0 bn_on=0 drop_gate=0 drop_stats=1 drop_bn_x=1 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_tile128_bn_x_without_gate_refused': (
        'conv N=16 H=32 Cin=64 Cout=256 bn_gamma=1 bn_beta=1 tile=128 bn_x=1 bn_mean=1 bn_invstd=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=1 stats_rows=0 need_slots=0 error=vpho_conv2d_nhwc_f32: bn_x: the launch needs 128 partial rows (stats_cap 256) or runs a kernel without the BatchNorm epilogue (tile 128)'),
    'c_tile128_x2_refused': (
        'conv N=64 H=64 Cin=64 Cout=256 bias=1 x2=1 Cin2=64 stride2=1 H2=64 W2=64 tile=128',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: x2 is served by the direct-to-LDS kernels with wave-uniform taps only'),
    'c_tile128_res_up_refused': (
        'conv N=64 H=16 Cin=1024 Cout=256 bias=1 res_up=1 ru_H=8 ru_W=8 ru_ld=256 tile=128',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: res_up is not served by the forced register-staged tile'),
    'c_no_glds': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 no_glds=1',
        'rc=0 family=reg tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_no_glds_64x64': (
        'conv N=3 H=9 Cin=256 Cout=64 bias=1 no_glds=1',
        'rc=0 family=reg tile=64x64 threads=256 grid=8x1 prof=conv_igemm_64x64 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=4x1 uni=1 vec=1 lin=11 dbg=0'),
    'c_no_glds_res_up_keeps_glds': (
        'conv N=64 H=16 Cin=1024 Cout=256 bias=1 res_up=1 ru_H=8 ru_W=8 ru_ld=256 no_glds=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=1024 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_no_glds_bn_forward_off': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 no_glds=1 stats=1 stats_rows=1 stats_cap=256',
        'rc=0 family=reg tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=0 bn_on=0 drop_gate=0 drop_stats=1 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_no_uni': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 no_uni=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=0 vec=1 lin=11 dbg=0'),
    'c_no_uni_pers_off': (
        'conv N=16 H=32 Cin=64 Cout=640 bias=1 no_uni=1',
        'rc=0 family=glds tile=128x128 threads=512 grid=640x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x5 uni=0 vec=1 lin=11 dbg=0'),
    'c_no_uni_prologue_to_reg': (
        'conv N=16 H=32 Cin=256 Cout=256 bias=1 in_scale=1 in_shift=1 no_uni=1',
        'rc=0 family=reg tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=256 tiles=128x2 uni=0 vec=1 lin=11 dbg=0'),
    'c_no_uni_x2_refused': (
        'conv N=64 H=64 Cin=64 Cout=256 bias=1 x2=1 Cin2=64 stride2=1 H2=64 W2=64 no_uni=1',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: x2 is served by the direct-to-LDS kernels with wave-uniform taps only'),
    'c_dbg8': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 res=1 dbg=8',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=8'),
    'c_dbg16': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 dbg=16',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=16'),
    'c_dbg_other_bits_masked': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 dbg=31',
        'rc=0 family=glds tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=24'),
    'c_slots_unknown_split_needs_none': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 w_planes=1 plane_terms=6 slots=-1',
        'rc=0 family=split6 tile=128x128 threads=512 grid=256x1 prof=conv_igemm_128x128 name=conv_igemm_split_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'c_slots_unknown': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 slots=-1',
        'rc=1 stats_rows=-1 need_slots=1 error='),
    'c_slots_208_pers': (
        'conv N=16 H=32 Cin=64 Cout=256 bias=1 slots=208',
        'rc=0 family=pers tile=128x128 threads=512 grid=208x1 prof=conv_igemm_128x128 name=conv_igemm_pers_kernel stats_rows=-1 bn_on=0 drop_gate=0 drop_stats=0 drop_bn_x=0 K=64 tiles=128x2 uni=1 vec=1 lin=11 dbg=0'),
    'd_null_descriptor': (
        'conv null_desc=1',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: null descriptor'),
    'd_null_tensor': (
        'conv N=16 H=32 Cin=64 Cout=256 y=0',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: null tensor'),
    'd_non_positive': (
        'conv N=0 H=32 Cin=64 Cout=256',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: non-positive dimension'),
    'd_cin_not_4': (
        'conv N=16 H=32 Cin=62 Cout=256',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: Cin=62 x_ld=62 must be multiples of 4, x_ld>=Cin'),
    'd_misaligned_x': (
        'conv N=16 H=32 Cin=64 Cout=256 x=2',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: x/w must be 16-byte aligned'),
    'd_scale_without_shift': (
        'conv N=16 H=32 Cin=64 Cout=256 in_scale=1',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: in_scale/in_shift must come together'),
    'd_output_too_large': (
        'conv N=16 H=32 Cin=64 Cout=256 OH=33',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: output larger than input allows'),
    'd_too_many_pixels': (
        'conv N=4096 H=1024 Cin=4 Cout=4',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: too many output pixels'),
    'd_grouped_with_gate': (
        'conv N=8 H=32 Cin=64 Cout=256 gate=1 groups=2 x_group=524288 w_group=16384 y_group=2097152 bias_group=256',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: grouped launches take no splits / pixel list / gate / bf16 planes'),
    'd_w_ld_below_K': (
        'conv N=16 H=32 Cin=64 Cout=256 w_ld=32',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: w_ld / split strides must be multiples of 4, w_ld >= K'),
    'd_splits_with_bias': (
        'conv N=1 H=1 Cin=4096 Cout=256 bias=1 splits=4 w_ld=16384 x_split=4096 w_split=4096 y_split=65536',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: split launches produce plain partial sums (no bias / residual / prologue / gate)'),
    'd_row_map_without_count': (
        'conv N=16 H=32 Cin=64 Cout=256 row_map=1',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: row_map / row_count must come together'),
    'd_x2_needs_1x1': (
        'conv N=16 H=32 Cin=64 Cout=256 K=3 pad=1 x2=1 Cin2=64 stride2=1 H2=32 W2=32',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: x2 needs a 1x1 unpadded convolution, Cin and Cin2 multiples of 32, no pixel list / prologue / splits / planes'),
    'd_x2_does_not_cover': (
        'conv N=16 H=32 Cin=64 Cout=256 x2=1 Cin2=64 stride2=2 H2=32 W2=32',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: x2 of 32 x 32 pixels read at stride 2 does not cover the 32 x 32 output (or exceeds 3.9 GB)'),
    'd_res_up_with_res': (
        'conv N=64 H=16 Cin=1024 Cout=256 res=1 res_up=1 ru_H=8 ru_W=8 ru_ld=256',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: res_up needs no res / gate / splits, a (N, ru_H, ru_W, ru_ld >= Cout) map with ru_ld % 4 == 0, 16-byte aligned'),
    'd_bn_x_without_stats': (
        'conv N=16 H=32 Cin=64 Cout=256 gate=1 bn_x=1 bn_mean=1 bn_invstd=1',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: bn_x needs stats, stats_rows, mean / invstd and -- without a stored gate -- gamma / beta'),
    'd_stats_without_rows': (
        'conv N=16 H=32 Cin=64 Cout=256 stats=1 stats_cap=256',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: stats needs stats_rows (host) and stats_cap'),
    'd_input_beyond_3_9_gb': (
        'conv N=512 H=256 Cin=64 Cout=64',
        'rc=1 stats_rows=-1 need_slots=0 error=vpho_conv2d_nhwc_f32: input (8.59 GB) and weights (0.00 GB) must each stay below 3.9 GB'),
    'e_wgrad_64x64': (
        'wgrad N=2 OH=16 Cin=64 Cout=64 K=3',
        'tile=64x64 tiles=1x9 splits=2 m_chunk=256 threads=256 grid=32 prof=conv_wgrad_64x64 reduce_groups=1 workspace=294912'),
    'e_wgrad_128x64': (
        'wgrad N=4 OH=16 Cin=256 Cout=512 K=3',
        'tile=128x64 tiles=4x36 splits=4 m_chunk=256 threads=512 grid=576 prof=conv_wgrad_128x128 reduce_groups=1 workspace=18874368'),
    'e_wgrad_128x128_1x1': (
        'wgrad N=64 OH=16 Cin=1024 Cout=256 K=1',
        'tile=128x128 tiles=2x8 splits=32 m_chunk=512 threads=512 grid=512 prof=conv_wgrad_128x128 reduce_groups=4 workspace=33554432'),
    'e_wgrad_128x128_largest': (
        'wgrad N=64 OH=64 Cin=256 Cout=256 K=3',
        'tile=128x128 tiles=2x18 splits=32 m_chunk=8192 threads=512 grid=1152 prof=conv_wgrad_128x128 reduce_groups=4 workspace=75497472'),
    'e_wgrad_one_slice': (
        'wgrad N=1 OH=8 Cin=64 Cout=64 K=1',
        'tile=64x64 tiles=1x1 splits=1 m_chunk=64 threads=256 grid=8 prof=conv_wgrad_64x64 reduce_groups=0 workspace=0'),
    'e_wgrad_8_slices': (
        'wgrad N=2 OH=32 Cin=256 Cout=256 K=3',
        'tile=128x64 tiles=2x36 splits=8 m_chunk=256 threads=512 grid=576 prof=conv_wgrad_128x128 reduce_groups=4 workspace=18874368'),
    'e_wgrad_slices_multiple_of_8': (
        'wgrad N=64 OH=64 Cin=64 Cout=256 K=1',
        'tile=128x64 tiles=2x1 splits=256 m_chunk=1024 threads=512 grid=512 prof=conv_wgrad_128x128 reduce_groups=16 workspace=16777216'),
    'e_wgrad_reduce_plain_few_slices': (
        'wgrad N=1 OH=32 Cin=64 Cout=64 K=3',
        'tile=64x64 tiles=1x9 splits=4 m_chunk=256 threads=256 grid=64 prof=conv_wgrad_64x64 reduce_groups=1 workspace=589824'),
    'e_wgrad_reduce_4': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=1',
        'tile=64x64 tiles=4x4 splits=16 m_chunk=256 threads=256 grid=256 prof=conv_wgrad_64x64 reduce_groups=4 workspace=4194304'),
    'e_wgrad_reduce_16': (
        'wgrad N=64 OH=64 Cin=64 Cout=256 K=1',
        'tile=128x64 tiles=2x1 splits=256 m_chunk=1024 threads=512 grid=512 prof=conv_wgrad_128x128 reduce_groups=16 workspace=16777216'),
    'e_wgrad_reduce_plain_large_dw': (
        'wgrad N=64 OH=16 Cin=512 Cout=512 K=3',
        'tile=128x64 tiles=4x72 splits=4 m_chunk=4096 threads=512 grid=1152 prof=conv_wgrad_128x128 reduce_groups=1 workspace=37748736'),
    'e_wgrad_stem': (
        'wgrad N=64 OH=128 Cin=4 Cout=64 K=7',
        'tile=64x64 tiles=1x4 splits=256 m_chunk=4096 threads=256 grid=1024 prof=conv_wgrad_64x64 reduce_groups=16 workspace=12845056'),
    'e_wgrad_tile64': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=3 tile=64',
        'tile=64x64 tiles=4x36 splits=16 m_chunk=256 threads=256 grid=2304 prof=conv_wgrad_64x64 reduce_groups=4 workspace=37748736'),
    'e_wgrad_tile128': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=3 tile=128',
        'tile=128x128 tiles=2x18 splits=16 m_chunk=256 threads=512 grid=576 prof=conv_wgrad_128x128 reduce_groups=4 workspace=37748736'),
    'e_wgrad_tile12864': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=3 tile=12864',
        'tile=128x64 tiles=2x36 splits=16 m_chunk=256 threads=512 grid=1152 prof=conv_wgrad_128x128 reduce_groups=4 workspace=37748736'),
    'e_wgrad_tile12864_narrow': (
        'wgrad N=16 OH=16 Cin=256 Cout=64 K=3 tile=12864',
        'tile=64x64 tiles=1x36 splits=16 m_chunk=256 threads=256 grid=576 prof=conv_wgrad_64x64 reduce_groups=4 workspace=9437184'),
    'e_wgrad_big_min': (
        'wgrad N=64 OH=16 Cin=1024 Cout=256 K=1 big_min=5e10',
        'tile=128x64 tiles=2x16 splits=32 m_chunk=512 threads=512 grid=1024 prof=conv_wgrad_128x128 reduce_groups=4 workspace=33554432'),
    'e_wgrad_want': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=3 want=512',
        'tile=128x64 tiles=2x36 splits=16 m_chunk=256 threads=512 grid=1152 prof=conv_wgrad_128x128 reduce_groups=4 workspace=37748736'),
    'e_wgrad_stages': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=3 stages=4',
        'tile=128x64 tiles=2x36 splits=32 m_chunk=128 threads=512 grid=2304 prof=conv_wgrad_128x128 reduce_groups=4 workspace=75497472'),
    'e_wgrad_reduce_groups_forced_1': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=1 reduce_groups=1',
        'tile=64x64 tiles=4x4 splits=16 m_chunk=256 threads=256 grid=256 prof=conv_wgrad_64x64 reduce_groups=1 workspace=4194304'),
    'e_wgrad_reduce_groups_forced_4': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=1 reduce_groups=4',
        'tile=64x64 tiles=4x4 splits=16 m_chunk=256 threads=256 grid=256 prof=conv_wgrad_64x64 reduce_groups=4 workspace=4194304'),
    'e_wgrad_reduce_groups_forced_16': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=1 reduce_groups=16',
        'tile=64x64 tiles=4x4 splits=16 m_chunk=256 threads=256 grid=256 prof=conv_wgrad_64x64 reduce_groups=16 workspace=4194304'),
    'e_wgrad_reduce_groups_forced_2': (
        'wgrad N=16 OH=16 Cin=256 Cout=256 K=1 reduce_groups=2',
        'tile=64x64 tiles=4x4 splits=16 m_chunk=256 threads=256 grid=256 prof=conv_wgrad_64x64 reduce_groups=4 workspace=4194304'),
    'f_wino_mode1': (
        'wino Cin=64 N=4 H=32 Cout=128',
        'epilogue=plain mode=1 staged_ok=1 tbs=16 blocks=32 lds=161792'),
    'f_wino_mode0_switch': (
        'wino Cin=64 N=4 H=32 Cout=128 staged=0',
        'epilogue=plain mode=0 staged_ok=1 tbs=16 blocks=32 lds=131072'),
    'f_wino_mode2_windows': (
        'wino Cin=64 N=4 H=32 Cout=128 wins=1',
        'epilogue=plain mode=2 staged_ok=1 tbs=16 blocks=32 lds=161792'),
    'f_wino_mode0_windows_switch': (
        'wino Cin=64 N=4 H=32 Cout=128 wins=1 staged=0',
        'epilogue=plain mode=0 staged_ok=1 tbs=16 blocks=32 lds=131072'),
    'f_wino_staged_not_ok_w6': (
        'wino Cin=64 N=2 H=4 W=6 Cout=64',
        'epilogue=plain mode=0 staged_ok=0 tbs=1 blocks=8 lds=131072'),
    'f_wino_staged_not_ok_w12': (
        'wino Cin=64 N=3 H=12 Cout=128',
        'epilogue=plain mode=0 staged_ok=0 tbs=2 blocks=8 lds=131072'),
    'f_wino_several_images_per_block': (
        'wino Cin=64 N=130 H=8 Cout=64',
        'epilogue=plain mode=1 staged_ok=1 tbs=33 blocks=40 lds=161792'),
    'f_wino_three_channel_blocks': (
        'wino Cin=64 N=2 H=16 Cout=192',
        'epilogue=plain mode=1 staged_ok=1 tbs=2 blocks=6 lds=161792'),
    'f_wino_sixteen_channel_blocks': (
        'wino Cin=64 N=2 H=16 Cout=1024',
        'epilogue=plain mode=1 staged_ok=1 tbs=2 blocks=32 lds=161792'),
    'f_wino_bn_fwd_staged': (
        'wino Cin=64 N=4 H=32 Cout=64 bn=1',
        'epilogue=bn_fwd mode=1 staged_ok=1 tbs=16 blocks=16 lds=161792'),
    'f_wino_bn_fwd_unstaged_switch': (
        'wino Cin=64 N=4 H=32 Cout=64 bn=1 staged=0',
        'epilogue=bn_fwd mode=0 staged_ok=1 tbs=16 blocks=16 lds=131072'),
    'f_wino_bn_fwd_staged_not_ok': (
        'wino Cin=64 N=3 H=12 Cout=128 bn=1',
        'epilogue=bn_fwd mode=0 staged_ok=0 tbs=2 blocks=8 lds=131072'),
    'f_wino_bn_bwd_staged': (
        'wino Cin=64 N=4 H=32 Cout=64 bn=1 bn_x=1',
        'epilogue=bn_bwd mode=1 staged_ok=1 tbs=16 blocks=16 lds=161792'),
    'f_wino_bn_bwd_unstaged_switch': (
        'wino Cin=64 N=4 H=32 Cout=64 bn=1 bn_x=1 staged=0',
        'epilogue=bn_bwd mode=0 staged_ok=1 tbs=16 blocks=16 lds=131072'),
    'f_wino_bn_bwd_staged_not_ok': (
        'wino Cin=64 N=3 H=12 Cout=128 bn=1 bn_x=1',
        'epilogue=bn_bwd mode=0 staged_ok=0 tbs=2 blocks=8 lds=131072'),
}

# tests/test_gpu_conv.py::test_launches_reach_the_kernel_class_the_plan_table_names runs these on the device and watches the profiling
# counter of the class in `prof=` move (the Winograd launcher has one class: conv_winograd)
GPU_CASES = ['b_glds_128x128', 'b_pers', 'b_glds_128x64', 'b_glds_64x64', 'f_wino_mode1', 'e_wgrad_64x64', 'e_wgrad_128x64', 'e_wgrad_128x128_1x1']
