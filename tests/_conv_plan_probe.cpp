// Prints the launch plans of vpho_amd/csrc/conv_plan.h for descriptors read from stdin, one per line: the stand-alone program behind
// tests/test_conv_plan_cpu.py (which compiles it with the host compiler; no HIP, no device).
//
//   conv  key=value ...   every int field of vpho_conv_desc by its name; K = KH = KW, pad = pad_y = pad_x; OH / OW and the strides of y and res
//                         default to the dense NHWC output.  Operands by name: 0 = absent, 1 = present (a fake, 16-byte aligned
//                         address; nothing is dereferenced), 2 = present and misaligned.  x, w, y default to 1.
//                         Switches: dbg, pers (default 1), tile, no_glds, no_uni; slots (default 512, -1 = unknown).
//   wgrad N= OH= OW= Cin= Cout= K=  [tile= big_min= want= stages= reduce_groups=]
//   wino  N= H= W= Cout=  [wins= bn= bn_x= staged=]
#include "../vpho_amd/csrc/conv_plan.h"
#include <cstring>
#include <map>
#include <string>

namespace {

using Fields = std::map<std::string, double>;

Fields parse_fields(char* line, std::string* kind) {
    Fields f;
    for (char* tok = strtok(line, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
        char* eq = strchr(tok, '=');
        if (!eq) { *kind = tok; continue; }
        *eq = 0;
        f[tok] = atof(eq + 1);
    }
    return f;
}

struct ConvCase { vpho_conv_desc d; ConvSwitches sw; int slots; int stats_rows_host; };

// `c` is filled in place: d.stats_rows points into it
void conv_case(const Fields& f, ConvCase* c) {
    memset(c, 0, sizeof(*c));
    uintptr_t next = 0x10000000;
    auto get = [&](const char* k, double unset) { auto it = f.find(k); return it == f.end() ? unset : it->second; };
    auto geti = [&](const char* k, int unset) { return (int)get(k, unset); };
    auto ptr = [&](const char* k, int unset) -> uintptr_t {
        const int v = geti(k, unset);
        next += 0x100000;
        return v == 0 ? 0 : next + (v == 2 ? 4 : 0);
    };
    vpho_conv_desc& d = c->d;
    d.x = (const float*)ptr("x", 1); d.w = (const float*)ptr("w", 1); d.y = (float*)ptr("y", 1);
    d.bias = (const float*)ptr("bias", 0); d.in_scale = (const float*)ptr("in_scale", 0); d.in_shift = (const float*)ptr("in_shift", 0);
    d.res = (const float*)ptr("res", 0); d.gate = (const float*)ptr("gate", 0);
    d.row_map = (const int*)ptr("row_map", 0); d.row_count = (const int*)ptr("row_count", 0);
    d.w_planes = (const void*)ptr("w_planes", 0); d.res_up = (const float*)ptr("res_up", 0); d.x2 = (const float*)ptr("x2", 0);
    d.stats = (float*)ptr("stats", 0);
    d.bn_x = (const float*)ptr("bn_x", 0); d.bn_mean = (const float*)ptr("bn_mean", 0); d.bn_invstd = (const float*)ptr("bn_invstd", 0);
    d.bn_gamma = (const float*)ptr("bn_gamma", 0); d.bn_beta = (const float*)ptr("bn_beta", 0);
    c->stats_rows_host = -7;                                       // a plan that leaves the counter alone leaves this
    d.stats_rows = geti("stats_rows", 0) ? &c->stats_rows_host : nullptr;
    d.N = geti("N", 1); d.H = geti("H", 1); d.W = geti("W", d.H); d.Cin = geti("Cin", 4); d.x_ld = geti("x_ld", d.Cin);
    d.Cout = geti("Cout", 4); d.KH = geti("KH", geti("K", 1)); d.KW = geti("KW", geti("K", 1)); d.stride = geti("stride", 1);
    d.pad_y = geti("pad_y", geti("pad", 0)); d.pad_x = geti("pad_x", geti("pad", 0));
    d.OH = geti("OH", d.stride > 0 ? (d.H + 2 * d.pad_y - d.KH) / d.stride + 1 : 0);
    d.OW = geti("OW", d.stride > 0 ? (d.W + 2 * d.pad_x - d.KW) / d.stride + 1 : 0);
    d.y_sx = (long long)get("y_sx", d.Cout); d.y_sy = (long long)get("y_sy", (double)d.y_sx * d.OW); d.y_sn = (long long)get("y_sn", (double)d.y_sy * d.OH);
    d.r_sx = (long long)get("r_sx", d.Cout); d.r_sy = (long long)get("r_sy", (double)d.r_sx * d.OW); d.r_sn = (long long)get("r_sn", (double)d.r_sy * d.OH);
    d.in_slope = (float)get("in_slope", 0.1); d.out_slope = (float)get("out_slope", 1.0); d.gate_slope = (float)get("gate_slope", 0.1);
    d.w_ld = geti("w_ld", 0); d.splits = geti("splits", 0);
    d.x_split = (long long)get("x_split", 0); d.w_split = (long long)get("w_split", 0); d.y_split = (long long)get("y_split", 0);
    d.rows_hint = geti("rows_hint", 0); d.rows_scatter = geti("rows_scatter", 0);
    d.plane_terms = geti("plane_terms", 0);
    d.ru_H = geti("ru_H", 0); d.ru_W = geti("ru_W", 0); d.ru_ld = geti("ru_ld", 0);
    d.Cin2 = geti("Cin2", 0); d.x2_ld = geti("x2_ld", d.Cin2); d.stride2 = geti("stride2", 0); d.H2 = geti("H2", 0); d.W2 = geti("W2", 0);
    d.groups = geti("groups", 0);
    d.x_group = (long long)get("x_group", 0); d.w_group = (long long)get("w_group", 0); d.bias_group = (long long)get("bias_group", 0);
    d.y_group = (long long)get("y_group", 0); d.res_group = (long long)get("res_group", 0); d.x2_group = (long long)get("x2_group", 0);
    d.pre_group = (long long)get("pre_group", 0); d.ru_group = (long long)get("ru_group", 0);
    d.stats_cap = geti("stats_cap", 0);
    c->sw = ConvSwitches{geti("dbg", 0), geti("pers", 1), geti("tile", 0), geti("no_glds", 0), geti("no_uni", 0)};
    c->slots = geti("slots", 512);
}

const char* const FAMILY[CONV_NFAMILY] = {"reg", "glds", "glds_pre", "split6", "split9", "pers", "pers_bn"};
const char* prof_name(int cls) {
    switch (cls) {
        case PLAN_PROF_CONV128: return "conv_igemm_128x128";
        case PLAN_PROF_CONV64: return "conv_igemm_64x64";
        case PLAN_PROF_CONV128x64: return "conv_igemm_128x64";
        case PLAN_PROF_WGRAD64: return "conv_wgrad_64x64";
        case PLAN_PROF_WGRAD128: return "conv_wgrad_128x128";
    }
    return "?";
}

void print_conv(const Fields& f) {
    static ConvCase c;
    static Geo g;
    static ConvPlan p;
    conv_case(f, &c);
    const int rc = plan_conv(f.count("null_desc") ? nullptr : &c.d, c.slots, c.sw, &g, &p);
    if (rc) { printf("rc=1 stats_rows=%d need_slots=%d error=%s\n", p.stats_rows, p.need_slots, p.error); return; }
    printf("rc=0 family=%s tile=%dx%d threads=%d grid=%ux%u prof=%s name=%s stats_rows=%d bn_on=%d drop_gate=%d drop_stats=%d drop_bn_x=%d "
           "K=%d tiles=%dx%d uni=%d vec=%d lin=%d%d dbg=%d\n",
           FAMILY[p.family], p.bm, p.bn, p.threads, p.grid_x, p.grid_y, prof_name(p.prof_class), p.name, p.stats_rows, p.bn_on, p.drop_gate,
           p.drop_stats, p.drop_bn_x, g.K, g.tiles_m, g.tiles_n, g.uni, g.vec_epilogue, g.y_linear, g.r_linear, g.dbg);
}

void print_wgrad(const Fields& f) {
    auto get = [&](const char* k, double unset) { auto it = f.find(k); return it == f.end() ? unset : it->second; };
    const int N = (int)get("N", 1), OH = (int)get("OH", 1), OW = (int)get("OW", OH), Cin = (int)get("Cin", 4), Cout = (int)get("Cout", 4), K = (int)get("K", 1);
    if (N <= 0 || OH <= 0 || OW <= 0 || Cin <= 0 || Cout <= 0 || K <= 0) { printf("not planned: the entry points refuse non-positive sizes first\n"); return; }
    const WgSwitches sw = {(int)get("tile", 0), get("big_min", 4e9), (int)get("want", 0), (int)get("stages", 0), (int)get("reduce_groups", 0)};
    const WgPlan p = plan_wgrad((long long)N * OH * OW, Cin, Cout, K * K, sw);
    printf("tile=%dx%d tiles=%dx%d splits=%d m_chunk=%d threads=%d grid=%u prof=%s reduce_groups=%d workspace=%lld\n", p.bm, p.bn, p.tiles_m, p.tiles_n,
           p.splits, p.m_chunk, p.threads, p.grid, prof_name(p.prof_class), p.reduce_groups, p.splits > 1 ? (long long)p.splits * Cout * K * K * Cin * 4 : 0ll);
}

void print_wino(const Fields& f) {
    auto geti = [&](const char* k, int unset) { auto it = f.find(k); return it == f.end() ? unset : (int)it->second; };
    const int H = geti("H", 2), W = geti("W", H);
    if (geti("N", 1) <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || geti("Cout", 64) <= 0 || geti("Cout", 64) % W_CB) {
        printf("not planned: the launcher refuses odd maps and Cout %% 64 != 0 first\n");
        return;
    }
    const WinoPlan p = plan_wino(geti("N", 1), H, W, geti("Cout", 64), geti("wins", 0) != 0, geti("bn", 0) != 0, geti("bn_x", 0) != 0, geti("staged", 1) != 0);
    static const char* const EPI[3] = {"plain", "bn_fwd", "bn_bwd"};
    printf("epilogue=%s mode=%d staged_ok=%d tbs=%d blocks=%u lds=%zu\n", EPI[p.epilogue], p.mode, (int)wino_staged_ok(H / 2, W / 2, W), p.tbs, p.blocks, p.lds);
}

}  // namespace

#ifndef CONV_PLAN_PROBE_NO_MAIN
int main() {
    static char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        std::string kind;
        const Fields f = parse_fields(line, &kind);
        if (kind == "conv") print_conv(f);
        else if (kind == "wgrad") print_wgrad(f);
        else if (kind == "wino") print_wino(f);
        else { printf("unknown kind '%s'\n", kind.c_str()); return 2; }
    }
    return 0;
}
#endif
