// Which kernels one evaluation of the score network launches (score_ode.hip), on what grids, and what the sampler's host side knows
// without a device: the workspace layout, the Dormand-Prince tableau, the stage combinations and the t_eval stamps.  Every plan is a
// pure function of sizes and a switches struct; the environment is read by read_score_switches() and nowhere else.
//
// Host only: the C ABI header and the standard library, no HIP -- `g++ -std=c++17 -Wall` compiles it, and tests/test_score_plan_cpu.py pins
// the plans of the shapes the GPU tests rely on (tests/_score_plan_cases.py) on a machine without a device.
//
// Everything sits in an unnamed namespace, as it did while it lived in score_ode.hip: that file is the only translation unit that sees
// its copy, and the kernels' symbols (which carry `LinComb`) keep their names.
#ifndef VPHO_SCORE_PLAN_H
#define VPHO_SCORE_PLAN_H
#include "../../include/vpho_hip.h"
#include "plan_common.h"                       // PLAN_ERR, plan_fail, PLAN_REQUIRE, env_int
#include <cstring>

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------
// Switches (A/B aids: either side of each computes the same bits)

struct ScoreSwitches {
    int pe_rows;      // VPHO_PE_ROWS, per call: 0 = unset (the rule), 64 = the 64-row pose encoder at every size, anything else = the 32-row one
    int head_tail;    // VPHO_HEAD_TAIL, once: 0 = ordinary 128-row tiles only
    int head_cb;      // VPHO_HEAD_CB, per call: 0 = per-image epilogue terms by global loads whatever sample_num
    int head_epi;     // VPHO_HEAD_EPI, per call: 0 = the reference epilogue, score_head_epi0_kernel
};

inline ScoreSwitches read_score_switches() {
    static const int head_tail = env_int("VPHO_HEAD_TAIL", 1);
    const int rows = env_int("VPHO_PE_ROWS", 0);
    return ScoreSwitches{getenv("VPHO_PE_ROWS") ? (rows == 64 ? 64 : 32) : 0, head_tail, env_int("VPHO_HEAD_CB", 1), env_int("VPHO_HEAD_EPI", 1)};
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Pose encoder (pose_encoder_reg_kernel<N1> / pose_encoder_reg64_kernel<N1>)

constexpr int PE_ROWS = 32, PE_H_LD = 260;    // hypotheses of a row tile; floats between rows of the 32 x 256 intermediate in LDS

struct PePlan {
    int rows, n1;                   // 32 or 64 hypotheses per workgroup; 32-wide chunks of the first layer's k (1..4): the launch table's keys
    unsigned grid;
    size_t lds;
    double flops;
    const char* name;               // what check_launch reports
    char error[PLAN_ERR];
};

// R rows of D values, zero-padded to Dp.  Returns 0 and a complete plan, or 1 with p->error set.
inline int plan_pose_encoder(long long R, int D, int Dp, const ScoreSwitches& sw, PePlan* p) {
    p->error[0] = 0;
    const int K1 = (Dp + 31) / 32 * 32;
    PLAN_REQUIRE(p->error, K1 <= 128 && (Dp & 3) == 0, "pose encoder: input dimension %d (padded %d) not supported (<= 128, multiple of 4)", D, Dp);
    // 64-row workgroups above 8 192 rows, i.e. as soon as 32-row workgroups would be more than one per CU (measured, isolated launches, hand /
    // object network: 12 800 rows 35.4 / 33.1 -> 30.4 / 27.9 us, 16 384 rows 35.8 / 32.6 -> 30.7 / 26.8, 32 768 rows -- BASELINE cfg4 -- 67.7 / 58.7 ->
    // 57.8 / 47.8; at the README config's 6 400 rows the 32-row kernel wins, 18.7 against 28.9: 200 workgroups against 100 on 256 CUs).
    // VPHO_PE_ROWS=32 / 64 forces either (the two are bit-identical)
    p->rows = (sw.pe_rows ? sw.pe_rows == 64 : R > 8192) ? 2 * PE_ROWS : PE_ROWS;
    p->n1 = K1 / 32;
    p->grid = (unsigned)((R + p->rows - 1) / p->rows);
    p->lds = (size_t)(p->rows * PE_H_LD + 512) * sizeof(float);        // 35 328 B / 68 608 B
    p->flops = 2.0 * (double)R * 256.0 * (K1 + 256.0);
    p->name = p->rows == 64 ? "pose_encoder_reg64_kernel" : "pose_encoder_reg_kernel";
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Score head (score_head_kernel<CB> / score_head_epi0_kernel<CB> / score_head_split_kernel<TERMS>)

constexpr int HB_K = 16;                      // k per LDS stage of the fp32 head
constexpr int SP_K = 16;                      // ... of the split-bf16 head = one 32x32x16 MFMA step

enum HeadFamily { HEAD_PLAIN = 0, HEAD_EPI0, HEAD_SPLIT6, HEAD_SPLIT9, HEAD_NFAMILY };

struct HeadPlan {
    int family, cb;                 // HeadFamily; per-image epilogue terms from an LDS copy (fp32 kernels only): the launch table's keys
    int full_tiles, tail_tiles;     // per head: 128-row tiles, then 32-row tail tiles
    unsigned grid;
    size_t lds;
    double flops;
    const char* name;               // what check_launch reports
    int need_slots;                 // `slots` was not known (< 0): the caller reports its own error
    char error[PLAN_ERR];
};

// Tile plan of R rows on `nheads` heads: 128-row tiles; when the last round of the launch would be less than half full, the rows beyond
// the last full round become 32-row tail tiles that all CUs share (see head_tile).  slots = workgroups the device holds at two per CU
inline void head_tiles(long long R, int nheads, int slots, bool tail_on, int* full_tiles, int* tail_tiles) {
    const int tiles = (int)((R + 127) / 128);
    *full_tiles = tiles; *tail_tiles = 0;
    const long long total = (long long)tiles * nheads;
    if (tail_on && total > slots && total % slots != 0 && (total % slots) * 2 < slots) {
        const int fp = (int)(total / slots * slots / nheads);
        if (fp >= 1 && fp < tiles) { *full_tiles = fp; *tail_tiles = (int)((R - 128ll * fp + 31) / 32); }
    }
}

// R = bs * S rows, S hypotheses per image.  has_planes: the weights carry bf16 planes of w1_p (with split_terms 6 or 9: the split kernels).
// Returns 0 and a complete plan, or 1 with p->error (or p->need_slots) set.
inline int plan_head(long long R, int S, int nheads, int split_terms, bool has_planes, int slots, const ScoreSwitches& sw, HeadPlan* p) {
    p->error[0] = 0;
    p->need_slots = 0;
    PLAN_REQUIRE(p->error, (double)R * 256.0 * 4.0 < 4.0e9, "score head: %lld hypothesis rows exceed the 32-bit buffer offsets", R);
    if (slots < 0) { p->need_slots = 1; return 1; }
    head_tiles(R, nheads, slots, sw.head_tail != 0, &p->full_tiles, &p->tail_tiles);
    p->grid = (unsigned)(nheads * (p->full_tiles + p->tail_tiles));
    p->flops = (double)R * nheads * (2.0 * 256 * 256 + 2.0 * 256 * 3);
    if (has_planes && (split_terms == 6 || split_terms == 9)) {
        p->family = split_terms == 6 ? HEAD_SPLIT6 : HEAD_SPLIT9;
        p->cb = 0;
        // [2] stages of three bf16 weight planes and the fp32 rows | epilogue table | per-image terms: 73 728 B
        p->lds = (size_t)(2 * (3 * 256 * SP_K / 2 + 128 * SP_K) + 256 * 4 + 2 * 128 * 4) * sizeof(float);
        p->name = "score_head_split_kernel";
        return 0;
    }
    p->family = sw.head_epi == 0 ? HEAD_EPI0 : HEAD_PLAIN;
    // per-image epilogue terms from an LDS copy when a 128-row tile spans at most 3 images (sample_num >= 64)
    p->cb = S >= 64 && sw.head_cb ? 1 : 0;
    // [2] stages | [256][4] epilogue table | per-image terms (3 x 257 of 1024 floats): 57 344 B, two workgroups per CU
    p->lds = (size_t)(2 * (256 + 128) * HB_K + 256 * 4 + 2 * 128 * 4) * sizeof(float);
    p->name = "score_head_kernel";
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Workspace (vpho_score_workspace_bytes, vpho_score_eval, vpho_ode_sample)

struct RkCtl;                                 // the device-resident controller block: score_ode.hip, which asserts its size
constexpr int RKCTL_BYTES = 320;
constexpr int CTL_MAX_STEPS = 1024, CTL_LOG_CAP = 512;

struct Workspace {
    float *cimg, *ct, *X, *P1, *P2, *K, *tmp;
    double *y, *ynew, *partial, *result;
    int* nan_count;
    RkCtl* ctl; double *te, *dense_p, *log;
    long long bytes;
};

inline long long align_up(long long v) { return (v + 255) / 256 * 256; }

// base == nullptr: only `bytes` means anything
inline Workspace carve(const vpho_score_weights& w, int bs, int S, char* base) {
    const long long R = (long long)bs * S, NH = (long long)w.nheads * 256;
    long long off = 0;
    Workspace ws;
    auto take = [&](long long b) { char* p = base ? base + off : nullptr; off += align_up(b); return p; };
    ws.cimg = (float*)take(bs * NH * 4);
    ws.ct = (float*)take(8 * NH * 4);
    ws.X = (float*)take(R * w.Dp * 4);
    ws.P1 = (float*)take(R * 256 * 4);
    ws.P2 = (float*)take(R * 256 * 4);
    ws.K = (float*)take(7 * R * w.D * 4);
    ws.tmp = (float*)take(R * w.D * 4);
    ws.y = (double*)take(R * w.D * 8);
    ws.ynew = (double*)take(R * w.D * 8);
    ws.partial = (double*)take(1024 * 8);
    ws.result = (double*)take(64);
    ws.nan_count = (int*)take(64);
    ws.ctl = (RkCtl*)take(RKCTL_BYTES);
    ws.te = (double*)take(CTL_MAX_STEPS * 8);
    ws.dense_p = (double*)take(CTL_MAX_STEPS * 4 * 8);
    ws.log = (double*)take(CTL_LOG_CAP * 4 * 8);
    ws.bytes = off;
    return ws;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Dormand-Prince RK45 (scipy.integrate.RK45's tableau and dense-output polynomial)

const double RK_C[6] = {0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1};
const double RK_A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
const double RK_B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
const double RK_E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
const double RK_P[7][4] = {
    {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0, 0, 0, 0},
    {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};

// x = y + h * sum_{j < n} c_j K_j: the input rows of a stage, formed in the pose encoder (a kernel parameter: the layout stays)
struct LinComb { double c[7]; int n; double h; };

// stage s of an attempt: 1..5 from RK_A (evaluated at t + RK_C[s] h), 6 = the new state y_new from RK_B (at t + h).  h = 0: the caller's
inline LinComb stage_comb(int s) {
    LinComb lc;
    memset(&lc, 0, sizeof(lc));
    lc.n = s;
    for (int j = 0; j < s; ++j) lc.c[j] = s < 6 ? RK_A[s][j] : RK_B[j];
    return lc;
}

// te[0 .. num_steps) = np.linspace(T0, eps, num_steps): i * step + T0, and the end point exactly
inline void t_eval_linspace(double T0, double eps, int num_steps, double* te) {
    const int div = num_steps > 1 ? num_steps - 1 : 1;
    const double step = (eps - T0) / div;
    for (int i = 0; i < num_steps; ++i) te[i] = (double)i * step + T0;
    if (num_steps > 1) te[num_steps - 1] = eps;
}

}  // namespace
#endif
