// Which kernel a convolution launch reaches, on what grid, and what becomes of its BatchNorm epilogue: the ONE place where kernel choice
// lives, for the forward implicit GEMM (conv_igemm.hip), the weight gradient (conv_wgrad.hip) and the Winograd launcher
// (conv_winograd.hip).  Every plan is a pure function of sizes, operand presence / alignment and a switches struct; the environment is
// read by the switch readers at the end of each section and nowhere else.
//
// Host only: the C ABI header and the standard library, no HIP -- `g++ -std=c++17 -Wall` compiles it, and tests/test_conv_plan_cpu.py pins
// the plans of the shapes the GPU tests rely on (tests/_conv_plan_cases.py) on a machine without a device.
//
// Everything sits in an unnamed namespace, as it did while it lived in the three .hip files: each of them is the only translation unit
// that sees its copy, and the kernels' symbols (which carry the type of their `Geo` parameter) keep their names.
#ifndef VPHO_CONV_PLAN_H
#define VPHO_CONV_PLAN_H
#include "../../include/vpho_hip.h"
#include "plan_common.h"                       // PLAN_ERR, plan_fail, PLAN_REQUIRE, env_int
#include <algorithm>
#include <cstdint>

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------------------------------
// Forward convolution (vpho_conv2d_nhwc_f32)

constexpr int BK = 32;                // k extent of a stage, forward convolution and weight gradient alike
constexpr int SBK = 16;               // ... of the split-bf16 kernel
constexpr int GLDS_PRE_MAX = 512;     // most input channels of a pre-activation 1x1 convolution on the direct-to-LDS kernel

// the kernels' parameter
struct Geo {
    vpho_conv_desc d;
    int M, K, tiles_m, tiles_n, ntiles;
    int w_ld;                       // floats between consecutive weight rows (K unless the launch reduces a K-slice)
    long long x_zs, w_zs, y_zs;     // per blockIdx.y advance of x / w / y (split reductions, groups; 0 for ordinary launches)
    long long b_zs, r_zs, x2_zs, pre_zs, ru_zs;   // ... and of bias / res / x2 / in_scale + in_shift / res_up (groups only)
    int y_linear, r_linear, vec_epilogue;
    int uni;   // Cin % 32 == 0: wave-uniform taps (direct-to-LDS kernel)
    int dbg;   // A/B switches whose results are bit-identical (VPHO_CONV_DBG, read per call): 8 = residual tile requested in the epilogue
               // (round 3) instead of in front of the last k stage, 16 = second stage requested after the first has landed (round 3).
               // The timing ablations that produce WRONG results (skip global loads / barriers / LDS stores) are compile-time only:
               // -DCONV_ABLATE=<mask> in a diagnostic build (scripts/kernel_ablate.sh), never in the product library
};
static_assert(sizeof(vpho_conv_desc) == 440 && sizeof(Geo) == 552, "Geo is the kernels' parameter: its layout does not move with the plan code");

struct ConvSwitches {
    int dbg;          // VPHO_CONV_DBG, per call: bits 8 | 16 reach Geo::dbg
    int pers;         // VPHO_CONV_PERS, per call: 0 = never the persistent kernel (A/B aid -- same bits), 1 = default, 2 = also launches of at most one round
    int force_tile;   // VPHO_CONV_TILE, once: 128 (register-staged, 4 waves) / 1288 / 12864 / any other non-zero value = 64x64; 0 = the rule
    int no_glds;      // VPHO_CONV_NO_GLDS, once: register-staged kernels wherever they can serve the launch
    int no_uni;       // VPHO_CONV_NO_UNI, once: no wave-uniform taps
};

enum ConvFamily { CONV_REG = 0, CONV_GLDS, CONV_GLDS_PRE, CONV_SPLIT6, CONV_SPLIT9, CONV_PERS, CONV_PERS_BN, CONV_NFAMILY };
// TILE_128_W4: the forced VPHO_CONV_TILE=128, conv_igemm_kernel<128,128,2,2,1>; the split kernels serve it with their TILE_128 instance
enum ConvTile { TILE_128 = 0, TILE_128x64, TILE_64, TILE_128_W4, CONV_NTILE };
// profiling classes as vpho_prof_enable numbers them (conv_igemm.hip asserts that common.h agrees)
enum { PLAN_PROF_CONV128 = 0, PLAN_PROF_CONV64 = 1, PLAN_PROF_CONV128x64 = 3, PLAN_PROF_WGRAD64 = 10, PLAN_PROF_WGRAD128 = 11 };

struct ConvPlan {
    int family, tile;               // ConvFamily, ConvTile: the launch table's key
    int bm, bn, threads;
    unsigned grid_x, grid_y;
    int prof_class;
    const char* name;               // what check_launch reports
    double flops, bytes;            // of the launch, for the profiling counters
    // the BatchNorm epilogue (vpho_conv_desc.stats / bn_x): bn_on = the kernel takes the reductions.  stats_rows = what the caller stores
    // in *desc.stats_rows, also when the plan fails; -1 = the plan failed before the counter is touched.  The drop_* flags say what
    // plan_conv took out of geo->d: the stored gate (recomputed from bn_x instead), the partial rows, bn_x (the stored gate serves)
    int bn_on, stats_rows, drop_gate, drop_stats, drop_bn_x;
    int need_slots;                 // the plan stopped at the persistent decision and `slots` was not known (< 0): the caller reports its own error
    char error[PLAN_ERR];
};

// Every check and decision of a launch, in the order in which a caller can observe them: the first failing check wins.  Returns 0 and a
// complete geo / plan, or 1 with plan->error (or plan->need_slots) set.  slots = workgroups the device holds at two per CU.
inline int plan_conv(const vpho_conv_desc* dp, int slots, const ConvSwitches& sw, Geo* gp, ConvPlan* p) {
    char* err = p->error;
    err[0] = 0;
    p->stats_rows = -1; p->need_slots = 0;
    p->bn_on = p->drop_gate = p->drop_stats = p->drop_bn_x = 0;
    PLAN_REQUIRE(err, dp != nullptr, "vpho_conv2d_nhwc_f32: null descriptor");
    const vpho_conv_desc& d = *dp;
    Geo& g = *gp;
    PLAN_REQUIRE(err, d.x && d.w && d.y, "vpho_conv2d_nhwc_f32: null tensor");
    PLAN_REQUIRE(err, d.N > 0 && d.H > 0 && d.W > 0 && d.Cin > 0 && d.Cout > 0 && d.KH > 0 && d.KW > 0 && d.stride > 0,
                 "vpho_conv2d_nhwc_f32: non-positive dimension");
    PLAN_REQUIRE(err, d.Cin % 4 == 0 && d.x_ld % 4 == 0 && d.x_ld >= d.Cin, "vpho_conv2d_nhwc_f32: Cin=%d x_ld=%d must be multiples of 4, x_ld>=Cin", d.Cin, d.x_ld);
    PLAN_REQUIRE(err, al16(d.x) && al16(d.w), "vpho_conv2d_nhwc_f32: x/w must be 16-byte aligned");
    PLAN_REQUIRE(err, (d.in_scale == nullptr) == (d.in_shift == nullptr), "vpho_conv2d_nhwc_f32: in_scale/in_shift must come together");
    PLAN_REQUIRE(err, d.in_scale == nullptr || (al16(d.in_scale) && al16(d.in_shift)), "vpho_conv2d_nhwc_f32: in_scale/in_shift alignment");
    PLAN_REQUIRE(err, d.OH > 0 && d.OW > 0, "vpho_conv2d_nhwc_f32: empty output");
    // the last tap of the last output pixel may not start beyond the padded input by more than the pad
    PLAN_REQUIRE(err, (d.OH - 1) * d.stride - d.pad_y < d.H && (d.OW - 1) * d.stride - d.pad_x < d.W, "vpho_conv2d_nhwc_f32: output larger than input allows");
    const long long M = (long long)d.N * d.OH * d.OW;
    PLAN_REQUIRE(err, M < (1ll << 31), "vpho_conv2d_nhwc_f32: too many output pixels");
    g.d = d;
    g.M = (int)M;
    g.K = d.KH * d.KW * d.Cin + (d.x2 ? d.Cin2 : 0);
    const int splits = d.splits > 1 ? d.splits : 1;
    g.w_ld = d.w_ld > 0 ? d.w_ld : g.K;
    g.x_zs = splits > 1 ? d.x_split : 0; g.w_zs = splits > 1 ? d.w_split : 0; g.y_zs = splits > 1 ? d.y_split : 0;
    g.b_zs = g.r_zs = g.x2_zs = g.pre_zs = g.ru_zs = 0;
    // grouped launch (ABI 11): blockIdx.y = group; the twin hand / object branches of the feature path (same shapes, different weights,
    // backbone_FPN_HFL.py:79-109) as ONE launch -- twice the tiles, half the launches, every output's k order unchanged
    const int groups = d.groups > 1 ? d.groups : 1;
    if (groups > 1) {
        PLAN_REQUIRE(err, splits == 1 && !d.row_map && !d.gate && !d.w_planes, "vpho_conv2d_nhwc_f32: grouped launches take no splits / pixel list / gate / bf16 planes");
        PLAN_REQUIRE(err, d.x_group >= 0 && d.w_group > 0 && d.y_group > 0 && d.x_group % 4 == 0 && d.w_group % 4 == 0 && d.y_group % 4 == 0 && d.bias_group % 4 == 0 &&
                     d.res_group % 4 == 0 && d.x2_group % 4 == 0 && d.pre_group % 4 == 0 && d.ru_group % 4 == 0,
                     "vpho_conv2d_nhwc_f32: group strides must be non-negative multiples of 4 floats (x_group may be 0: a shared input)");
        g.x_zs = d.x_group; g.w_zs = d.w_group; g.y_zs = d.y_group; g.b_zs = d.bias_group; g.r_zs = d.res_group; g.x2_zs = d.x2_group;
        g.pre_zs = d.pre_group; g.ru_zs = d.ru_group;
    }
    const int ny = splits * groups;                               // grid.y (at most one of the two is > 1)
    PLAN_REQUIRE(err, g.w_ld >= g.K && g.w_ld % 4 == 0 && g.x_zs % 4 == 0 && g.w_zs % 4 == 0, "vpho_conv2d_nhwc_f32: w_ld / split strides must be multiples of 4, w_ld >= K");
    PLAN_REQUIRE(err, splits == 1 || (!d.res && !d.bias && !d.in_scale && !d.gate), "vpho_conv2d_nhwc_f32: split launches produce plain partial sums (no bias / residual / prologue / gate)");
    g.y_linear = (d.y_sy == d.y_sx * d.OW && d.y_sn == d.y_sy * d.OH) ? 1 : 0;
    g.r_linear = (d.res == nullptr) || (d.r_sy == d.r_sx * d.OW && d.r_sn == d.r_sy * d.OH) ? 1 : 0;
    PLAN_REQUIRE(err, (d.row_map == nullptr) == (d.row_count == nullptr), "vpho_conv2d_nhwc_f32: row_map / row_count must come together");
    if (d.row_map) {
        PLAN_REQUIRE(err, splits == 1 && !d.gate, "vpho_conv2d_nhwc_f32: pixel-list launches take no splits / gate");
        if (!d.rows_scatter) g.y_linear = g.r_linear = 1;   // compact output: row r of y (and res) is the r-th listed pixel
    }
    // 16-byte epilogue when every output pixel's channel run (and the residual's) is 16-byte addressable
    g.vec_epilogue = (d.Cout % 4 == 0 && al16(d.y) && d.y_sx % 4 == 0 && d.y_sy % 4 == 0 && d.y_sn % 4 == 0 &&
                      (!d.bias || al16(d.bias)) &&
                      (!d.gate || al16(d.gate)) &&
                      (!d.res || (al16(d.res) && d.r_sx % 4 == 0 && d.r_sy % 4 == 0 && d.r_sn % 4 == 0))) ? 1 : 0;
    // (round 5: the direct-to-LDS kernel's own ablations on the one-round layers, scripts/conv_oneround.py, 3.36 ms per step over nine shapes: stage
    // fills 6 %, stage barrier 1.5 %, epilogue 8.6 %, matrix instructions + launch shape the rest; 4-byte stores straight from the accumulators
    // instead of this 16-byte epilogue: +2.5 %)
    g.dbg = sw.dbg & (8 | 16);                                 // only the bit-identical A/B orders exist at run time
    if (d.x2) {
        // second input concatenated along the channels (projection shortcut merged into conv3): direct-to-LDS kernels, wave-uniform taps
        PLAN_REQUIRE(err, d.KH == 1 && d.KW == 1 && d.pad_y == 0 && d.pad_x == 0 && d.Cin % BK == 0 && d.Cin2 > 0 && d.Cin2 % BK == 0 && d.x2_ld % 4 == 0 &&
                     d.x2_ld >= d.Cin2 && d.stride2 > 0 && al16(d.x2) && !d.row_map && !d.in_scale && splits == 1 && !d.w_planes,
                     "vpho_conv2d_nhwc_f32: x2 needs a 1x1 unpadded convolution, Cin and Cin2 multiples of 32, no pixel list / prologue / splits / planes");
        PLAN_REQUIRE(err, (d.OH - 1) * d.stride2 < d.H2 && (d.OW - 1) * d.stride2 < d.W2 && 4.0 * d.N * d.H2 * d.W2 * (double)d.x2_ld < 3.9e9,
                     "vpho_conv2d_nhwc_f32: x2 of %d x %d pixels read at stride %d does not cover the %d x %d output (or exceeds 3.9 GB)", d.H2, d.W2, d.stride2, d.OH, d.OW);
    }
    if (d.res_up) {
        // up-sampled residual (the FPN's top-down add): served by the direct-to-LDS kernels' 16-byte epilogue only
        PLAN_REQUIRE(err, !d.res && !d.gate && splits == 1 && d.ru_H > 0 && d.ru_W > 0 && d.ru_ld >= d.Cout && d.ru_ld % 4 == 0 && al16(d.res_up),
                     "vpho_conv2d_nhwc_f32: res_up needs no res / gate / splits, a (N, ru_H, ru_W, ru_ld >= Cout) map with ru_ld %% 4 == 0, 16-byte aligned");
        PLAN_REQUIRE(err, g.vec_epilogue && d.in_scale == nullptr && !d.w_planes && (!d.row_map || d.rows_scatter),
                     "vpho_conv2d_nhwc_f32: res_up needs 16-byte addressable output rows, no prologue affine, no split-bf16 planes, scattered pixel lists");
        PLAN_REQUIRE(err, 4.0 * d.N * d.ru_H * d.ru_W * (double)d.ru_ld < 3.9e9, "vpho_conv2d_nhwc_f32: res_up map too large");
    }
    // BatchNorm reductions in the epilogue (ABI 13): the direct-to-LDS kernels' 16-byte epilogue, one partial row per M-tile
    if (d.stats_rows) p->stats_rows = 0;
    const bool stats_shape = g.vec_epilogue && splits == 1 && groups == 1 && !d.row_map && !d.w_planes && (d.in_scale == nullptr);
    if (d.bn_x) {
        PLAN_REQUIRE(err, d.stats && d.stats_rows && d.bn_mean && d.bn_invstd && (d.gate || (d.bn_gamma && d.bn_beta)),
                     "vpho_conv2d_nhwc_f32: bn_x needs stats, stats_rows, mean / invstd and -- without a stored gate -- gamma / beta");
        PLAN_REQUIRE(err, (stats_shape || d.gate) && al16(d.bn_x) && al16(d.bn_mean) && al16(d.bn_invstd) && (!d.bn_gamma || (al16(d.bn_gamma) && al16(d.bn_beta))),
                     "vpho_conv2d_nhwc_f32: bn_x without a stored gate is served by the direct-to-LDS 16-byte epilogue only (Cout %% 4 == 0, aligned, no splits / groups / pixel list / prologue / planes)");
    }
    PLAN_REQUIRE(err, !d.stats || (d.stats_rows && d.stats_cap > 0 && al16(d.stats)), "vpho_conv2d_nhwc_f32: stats needs stats_rows (host) and stats_cap");
    const long long big_tiles = ((M + 127) / 128) * ((d.Cout + 127) / 128) * ny;
    const double m_acc = (d.row_map && d.rows_hint > 0) ? (double)d.rows_hint : (double)M;   // rows the launch really computes
    p->flops = 2.0 * m_acc * d.Cout * g.K * ny;
    // algorithmic HBM bytes: input, packed weights and output once each (+ residual, + bias)
    p->bytes = groups * 4.0 * ((double)d.N * d.H * d.W * d.Cin + (d.x2 ? (double)d.N * d.OH * d.OW * d.Cin2 : 0.0) + (double)d.Cout * g.K + m_acc * d.Cout * (d.res ? 2 : 1) + d.Cout + (d.res_up ? (double)d.N * d.ru_H * d.ru_W * d.Cout : 0.0));
    // tile choice (measured on MI355X, scripts/conv_tune.py): 8-wave 128x128 when it still gives >= 2 tiles per CU,
    // 8-wave 128x64 when that gives >= 1 tile per CU, else the 4-wave 64x64 tile (small feature maps, narrow heads)
    const long long tiles_12864 = ((M + 127) / 128) * ((d.Cout + 63) / 64) * ny;
    int variant = 64;
    if (big_tiles >= 256 && d.Cout % 128 == 0) variant = 1288;
    else if (tiles_12864 >= 256 && d.Cout >= 48) variant = 12864;
    if (sw.force_tile) variant = sw.force_tile;
    // the direct-to-LDS kernels address x and w by 32-bit byte offsets: both extents (all splits included) must stay below 4 GB
    // (the largest activation of the reference's configurations is 0.27 GB)
    const double x_extent = 4.0 * (((double)d.N * d.H * d.W - 1) * d.x_ld + d.Cin + (double)(ny - 1) * (double)g.x_zs);
    const double w_extent = 4.0 * (((double)d.Cout - 1) * g.w_ld + g.K + (double)(ny - 1) * (double)g.w_zs);
    PLAN_REQUIRE(err, x_extent < 3.9e9 && w_extent < 3.9e9 && g.x_zs >= 0 && g.w_zs >= 0,
                 "vpho_conv2d_nhwc_f32: input (%.2f GB) and weights (%.2f GB) must each stay below 3.9 GB", x_extent * 1e-9, w_extent * 1e-9);
    g.uni = (d.Cin % BK == 0 && d.pad_y >= 0 && d.pad_x >= 0 && !sw.no_uni) ? 1 : 0;
    // a pre-activation prologue rides on the direct-to-LDS kernel when the fragment's k is a plain channel index (1x1, unpadded,
    // Cin a multiple of 32 and within the LDS table); everything else with a prologue takes the register-staged kernel
    const bool simple = d.KH == 1 && d.KW == 1 && d.pad_y == 0 && d.pad_x == 0;
    const bool pre_on_read = d.in_scale != nullptr && g.uni && simple && d.Cin <= GLDS_PRE_MAX;
    const bool glds = (d.in_scale == nullptr || pre_on_read) && (!sw.no_glds || d.res_up != nullptr || d.x2 != nullptr || d.bn_x != nullptr);
    PLAN_REQUIRE(err, !d.x2 || (g.uni && variant != 128), "vpho_conv2d_nhwc_f32: x2 is served by the direct-to-LDS kernels with wave-uniform taps only");
    PLAN_REQUIRE(err, !d.res_up || variant != 128, "vpho_conv2d_nhwc_f32: res_up is not served by the forced register-staged tile");

    // ---- family
    // opt-in split-bf16 products (never the default): shapes the split kernel takes, everything else stays on the fp32 kernels
    const bool split_ok = d.w_planes != nullptr && (d.plane_terms == 6 || d.plane_terms == 9) && d.in_scale == nullptr && splits == 1 && !d.gate &&
                          d.Cin % SBK == 0 && g.vec_epilogue && d.pad_y >= 0 && d.pad_x >= 0 && g.w_ld == g.K &&
                          al16(d.w_planes) && 6.0 * d.Cout * g.K < 3.9e9;
    p->name = "conv_igemm_kernel";
    p->family = !glds ? CONV_REG : pre_on_read ? CONV_GLDS_PRE : CONV_GLDS;
    if (variant == 128) p->family = CONV_REG;
    bool pers = false;
    if (split_ok) {
        p->family = d.plane_terms == 9 ? CONV_SPLIT9 : CONV_SPLIT6;
        p->name = "conv_igemm_split_kernel";
    } else {
        // persistent multi-tile kernel (round 5): 1x1 launches of the 128x128 class with more tiles than workgroup slots (two 80-KB workgroups
        // per CU).  VPHO_CONV_PERS: 0 = never (round 4's kernel, A/B aid -- same bits), 1 = default, 2 = also launches of at most one round
        if (slots < 0) { p->need_slots = 1; return 1; }
        const double y_extent = 4.0 * ((double)(d.N - 1) * d.y_sn + (double)(d.OH - 1) * d.y_sy + (double)(d.OW - 1) * d.y_sx + d.Cout);
        const double r_extent = d.res ? 4.0 * ((double)(d.N - 1) * d.r_sn + (double)(d.OH - 1) * d.r_sy + (double)(d.OW - 1) * d.r_sx + d.Cout) : 0.0;
        const bool ok = sw.pers && variant == 1288 && glds && !pre_on_read && d.in_scale == nullptr && g.uni && simple && g.vec_epilogue && !d.row_map && !d.res_up &&
                        !d.gate && !d.bn_x && splits == 1 && y_extent < 3.9e9 && r_extent < 3.9e9 && d.y_sn >= 0 && d.y_sy >= 0 && d.y_sx >= 0 &&
                        (!d.x2 || 4.0 * d.N * d.H2 * d.W2 * (double)d.x2_ld < 3.9e9);
        pers = ok && (big_tiles > slots || sw.pers >= 2);
        if (pers) p->name = "conv_igemm_pers_kernel";
    }

    // ---- tile, threads, grid
    p->tile = variant == 1288 ? TILE_128 : variant == 12864 ? TILE_128x64 : variant == 128 ? (split_ok ? TILE_128 : TILE_128_W4) : TILE_64;
    p->bm = p->tile == TILE_64 ? 64 : 128;
    p->bn = p->tile == TILE_128 || p->tile == TILE_128_W4 ? 128 : 64;
    p->threads = p->tile == TILE_64 || p->tile == TILE_128_W4 ? 256 : 512;
    p->prof_class = p->tile == TILE_64 ? PLAN_PROF_CONV64 : p->tile == TILE_128x64 ? PLAN_PROF_CONV128x64 : PLAN_PROF_CONV128;
    g.tiles_m = (int)((M + p->bm - 1) / p->bm); g.tiles_n = (d.Cout + p->bn - 1) / p->bn;
    g.ntiles = g.tiles_m * g.tiles_n;
    p->grid_x = (unsigned)((g.ntiles + 7) / 8 * 8); p->grid_y = (unsigned)ny;
    if (pers) {                                                    // a walk over the tiles by as many workgroups as the device holds; the groups share the slots
        p->grid_x = (unsigned)std::min<long long>(p->grid_x, std::max(8, slots / groups / 8 * 8));
        p->grid_y = (unsigned)groups;
    }

    // ---- the BatchNorm epilogue: taken by the direct-to-LDS kernels (the persistent one among them) where the shape has 16-byte rows and the
    // caller's table holds one partial row per M-tile
    if (d.stats) {
        p->bn_on = (p->family == CONV_GLDS || p->family == CONV_GLDS_PRE) && stats_shape && g.tiles_m <= d.stats_cap;
        if (p->bn_on) {
            p->stats_rows = g.tiles_m;
            if (d.bn_x && d.bn_gamma) { p->drop_gate = d.gate != nullptr; g.d.gate = nullptr; }   // the gate recomputed from bn_x; the stored one was the fall-back
        } else {
            // no BatchNorm epilogue: the stored gate as is, no partial rows (the caller runs the stand-alone reduction); without a
            // stored gate to fall back to the call fails -- never drop the gate silently
            p->drop_stats = 1; g.d.stats = nullptr;
            if (d.bn_x) {
                PLAN_REQUIRE(err, d.gate, "vpho_conv2d_nhwc_f32: bn_x: the launch needs %d partial rows (stats_cap %d) or runs a kernel without the BatchNorm epilogue (tile %d)",
                             g.tiles_m, d.stats_cap, variant);
                p->drop_bn_x = 1; g.d.bn_x = nullptr;
            }
        }
    }
    if (pers) p->family = p->bn_on ? CONV_PERS_BN : CONV_PERS;
    return 0;
}

inline ConvSwitches read_conv_switches() {
    static const int force_tile = env_int("VPHO_CONV_TILE", 0), no_glds = env_int("VPHO_CONV_NO_GLDS", 0), no_uni = env_int("VPHO_CONV_NO_UNI", 0);   // tuning aids, read once
    return ConvSwitches{env_int("VPHO_CONV_DBG", 0), env_int("VPHO_CONV_PERS", 1), force_tile, no_glds, no_uni};
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Weight gradient (vpho_conv2d_wgrad_nhwc_f32, vpho_conv2d_wgrad_workspace_bytes: both plan with the same switches, so they agree)

struct WgSwitches {      // tuning aids, all read once
    int tile;            // VPHO_WGRAD_TILE: 64 / 128 / 12864
    double big_min;      // VPHO_WGRAD_BIG_MIN: smallest M K Cout of the 128 x 128 tile on 1x1 layers (4e9; round 4's rule: 5e10)
    int want, stages;    // VPHO_WGRAD_WANT / VPHO_WGRAD_STAGES: workgroups aimed at, shortest slice in stages of 32 pixels
    int reduce_groups;   // VPHO_WGRAD_REDUCE_GROUPS: 1 / 4 / 16
};

// reduce_groups: how the slice sum is ordered (0 = one slice, no sum): 1 = wgrad_reduce_kernel, 4 / 16 = wgrad_reduce_grouped_kernel
struct WgPlan { int bm, bn, tiles_m, tiles_n, splits, m_chunk, threads, prof_class, reduce_groups; unsigned grid; };

// threads per quad: 1 (the plain kernel) while it already fills the chip or the slices are few
inline int wgrad_reduce_groups(int splits, long long n4) {
    if (splits < 8 || n4 >= 256ll * 1024) return 1;
    return splits >= 32 && n4 < 64ll * 1024 ? 16 : 4;
}

// M, Cin, Cout, taps > 0: the entry points refuse anything else before they plan
inline WgPlan plan_wgrad(long long M, int Cin, int Cout, int taps, const WgSwitches& sw) {
    WgPlan p;
    const int K = Cin * taps;
    // 128x128 tiles pay off only for the largest products (measured: 3x3 256->256 on 64x64x64 pixels 100 vs 87 TF/s); everywhere else
    // the 64x64 tile wins or ties (3x3 128->128: 79 vs 53 TF/s) -- more tiles, hence fewer, longer pixel slices and less partial-sum traffic
    // (round 5, re-swept per shape with the grouped slice sum, scripts/wgrad_layers.py under VPHO_WGRAD_TILE=64 / 128: the 128 x 128 tile now
    // wins or ties from M K Cout ~ 4e9 on -- 1x1 1024 -> 256 on 16 x 16 maps 101 -> 92 us, 3x3 128 -> 128 on 32 x 32 217 -> 206 -- and loses below
    // (3x3 128 -> 128 on 16 x 16: 74 against 88): 19.6 -> 18.7 ms of weight gradients per training step)
    const bool big = sw.tile ? sw.tile == 128 : (K >= 128 && Cout >= 128 && (double)M * K * Cout >= sw.big_min);
    p.bm = p.bn = big ? 128 : 64;
    // Three tiles (re-swept per shape, round 5, scripts/wgrad_layers.py under VPHO_WGRAD_TILE = 64 / 128 / 12864: 19.6 / 20.8 / 18.5 ms of weight
    // gradients per training step, this rule 18.4, the best tile per shape 18.3): 128 output channels x 64 columns of the (tap, ci) axis --
    // 0.047 bytes of LDS fill per flop against 0.0625 for 64 x 64, three workgroups per CU -- wherever Cout >= 128 and the product is not tiny
    // (it also serves K = 64: 64 -> 256 on 64 x 64 maps 93 -> 88 us; 3x3 256 -> 256 on 16 x 16 202 -> 190); 128 x 128 for the 1x1 layers with
    // K a multiple of 128 from M K Cout = 4e9 on (1024 -> 256 on 16 x 16: 101 -> 92) and for the largest products; 64 x 64 for the rest.
    if (!sw.tile) {
        const double prod = (double)M * K * Cout;
        const bool big128 = K >= 128 && Cout >= 128 && ((taps == 1 && K % 128 == 0 && prod >= sw.big_min) || prod >= 5e10);
        if (big128) p.bm = p.bn = 128;
        else if (Cout >= 128 && K >= 64 && prod >= 1e9) { p.bm = 128; p.bn = 64; }
        else p.bm = p.bn = 64;
    } else if (sw.tile == 12864 && Cout >= 128) { p.bm = 128; p.bn = 64; }
    p.tiles_m = (Cout + p.bm - 1) / p.bm;
    p.tiles_n = (K + p.bn - 1) / p.bn;
    const long long tiles = (long long)p.tiles_m * p.tiles_n;
    // Workgroups for 256 CUs (2 x 128x128 or 4 x 64x64 tiles fit a CU's LDS): about two rounds of them, but no slices shorter than
    // 16 stages of 32 pixels (8 on the smallest maps, where nothing else fills the chip) -- a slice pays its prologue, its 16 KB
    // (64 KB) of partial sums and their reduction whatever its length.  Swept over the training step's 47 shapes
    // (scripts/r04_wgrad_want.sh, r04_wgrad_stages.sh): the 3x3 layers want ~2 000 workgroups, the 1x1 layers on 32 x 32 maps ~500
    // (8 tiles x 64 slices of 1 024 pixels); a fixed target of 1 536 with 8-stage slices cost 1.5 ms per step more.
    const long long want = sw.want > 0 ? (big ? sw.want : 2 * sw.want) : (big ? 1024 : 2048);
    const long long min_stages = sw.stages > 0 ? sw.stages : (M < 8192 ? 8 : 16);
    long long splits = std::max<long long>(1, (want + tiles - 1) / tiles);
    splits = std::min<long long>(splits, std::max<long long>(1, M / (min_stages * BK)));
    splits = std::min<long long>(splits, 256);
    if (splits >= 8) splits = std::max<long long>(8, (splits + 4) / 8 * 8);          // slices go to the 8 XCDs round-robin (see the kernel)
    long long chunk = (M + splits - 1) / splits;
    chunk = (chunk + BK - 1) / BK * BK;
    p.m_chunk = (int)chunk;
    p.splits = (int)((M + chunk - 1) / chunk);
    p.threads = p.bm == 128 ? 512 : 256;
    p.prof_class = p.bm == 128 ? PLAN_PROF_WGRAD128 : PLAN_PROF_WGRAD64;
    // see the kernel: XCD = blockIdx.x & 7
    const unsigned ntiles = (unsigned)tiles;
    p.grid = p.splits >= 8 ? 8u * ntiles * (unsigned)((p.splits + 7) / 8) : (unsigned)((ntiles + 7) / 8 * 8) * (unsigned)p.splits;
    const int forced = sw.reduce_groups;
    p.reduce_groups = p.splits <= 1 ? 0 : (forced == 1 || forced == 4 || forced == 16) ? forced : wgrad_reduce_groups(p.splits, (long long)Cout * K / 4);
    return p;
}

inline const WgSwitches& read_wgrad_switches() {
    static const WgSwitches sw = {env_int("VPHO_WGRAD_TILE", 0), getenv("VPHO_WGRAD_BIG_MIN") ? atof(getenv("VPHO_WGRAD_BIG_MIN")) : 4e9,
                                  env_int("VPHO_WGRAD_WANT", 0), env_int("VPHO_WGRAD_STAGES", 0), env_int("VPHO_WGRAD_REDUCE_GROUPS", 0)};
    return sw;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) launcher (conv_winograd.hip)

constexpr int WK = 8;                          // input channels per stage
constexpr int W_TB = 64, W_CB = 64;            // tiles / output channels per workgroup
constexpr int W_STAGE = 2 * 16 * 64 * WK;      // floats per stage: V | U
constexpr int W_IN_PIXELS = 480;               // STAGED kernel: pixels (64 bytes each) of the input region IN behind the two stages: 128 + 30 KB of the 160
// STAGED geometry: a 64-tile block = whole tile rows (TW | 64) of one image (NR = 64 / TW <= TH, TH % NR == 0) or all rows of NR / TH
// images (TH | NR), and the region's pixels fit IN
inline bool wino_staged_ok(int TH, int TW, int W) {
    if (TW < 4 || TW > 32 || (W_TB % TW) != 0) return false;
    const int NR = W_TB / TW;
    if (NR <= TH ? (TH % NR) != 0 : (NR % TH) != 0) return false;
    const int rpp = NR < TH ? NR : TH, ipb = NR / rpp;
    return ipb * (2 * rpp + 2) * (W + 2) <= W_IN_PIXELS;
}

enum WinoEpilogue { WINO_PLAIN = 0, WINO_BN_FWD, WINO_BN_BWD };    // conv_winograd_kernel / _bn_kernel (sums of y) / _bnb_kernel (bn_x given)
// mode: the kernels' template argument: 0 = input patches through registers, 1 = through LDS (whole tile rows of full maps), 2 = through
// LDS on window tiles (plain kernel only).  tbs = 64-tile blocks = the partial rows of a BatchNorm epilogue
struct WinoPlan { int epilogue, mode, tbs; unsigned blocks; size_t lds; };

// staged: VPHO_WINO_STAGED (read per call; 0 = registers everywhere: A/B aid, bit-identity test).  N > 0, even H and W, Cout a positive
// multiple of 64: the launcher refuses anything else before it plans
inline WinoPlan plan_wino(int N, int H, int W, int Cout, bool wins, bool bn, bool bn_x, bool staged) {
    WinoPlan p;
    const int TH = H / 2, TW = W / 2;
    p.tbs = (N * TH * TW + W_TB - 1) / W_TB;
    const int ncb = Cout / W_CB;
    p.blocks = (unsigned)(p.tbs * ncb);
    if (ncb <= 8 && (8 % ncb) == 0) { const int G = 8 / ncb; p.blocks = (unsigned)((p.tbs + G - 1) / G) * 8u; }
    p.epilogue = !bn ? WINO_PLAIN : bn_x ? WINO_BN_BWD : WINO_BN_FWD;
    // input patches through LDS where the blocks are whole tile rows of full maps (see the kernel)
    p.mode = !staged ? 0 : (wins && !bn) ? 2 : wino_staged_ok(TH, TW, W) ? 1 : 0;
    p.lds = (size_t)2 * W_STAGE * sizeof(float) + (p.mode ? (size_t)W_IN_PIXELS * 64 : 0);
    return p;
}

inline bool read_wino_staged() { return env_int("VPHO_WINO_STAGED", 1) != 0; }

}  // namespace
#endif
