// Prints the plans of vpho_amd/csrc/score_plan.h for cases read from stdin, one per line: the stand-alone program behind
// tests/test_score_plan_cpu.py (which compiles it with the host compiler; no HIP, no device).
//
//   pe    R= D= Dp=                           switch: pe_rows (0 = unset)
//   head  R= S= nheads=  [split_terms= planes=]  slots (default 512, -1 = unknown); switches: head_tail, head_cb, head_epi (default 1)
//   ws    D= Dp= nheads= bs= S=                 the workspace carved at a fake base address: bytes, and whether every slice starts on 256 bytes
//   comb  s=                                    the stage combination: n and the coefficients
//   teval T0= eps= n=                           the t_eval stamps
//   tableau                                     consistency sums of the Dormand-Prince constants
#include "../vpho_amd/csrc/score_plan.h"
#include <cmath>
#include <cstdint>
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

double get(const Fields& f, const char* k, double unset) { auto it = f.find(k); return it == f.end() ? unset : it->second; }
int geti(const Fields& f, const char* k, int unset) { return (int)get(f, k, unset); }

ScoreSwitches switches(const Fields& f) { return ScoreSwitches{geti(f, "pe_rows", 0), geti(f, "head_tail", 1), geti(f, "head_cb", 1), geti(f, "head_epi", 1)}; }

void print_pe(const Fields& f) {
    static PePlan p;
    if (plan_pose_encoder((long long)get(f, "R", 1), geti(f, "D", 96), geti(f, "Dp", 96), switches(f), &p)) { printf("rc=1 error=%s\n", p.error); return; }
    printf("rc=0 rows=%d n1=%d grid=%u lds=%zu flops=%.0f name=%s\n", p.rows, p.n1, p.grid, p.lds, p.flops, p.name);
}

void print_head(const Fields& f) {
    static HeadPlan p;
    static const char* const FAMILY[HEAD_NFAMILY] = {"plain", "epi0", "split6", "split9"};
    if (plan_head((long long)get(f, "R", 1), geti(f, "S", 100), geti(f, "nheads", 32), geti(f, "split_terms", 0), geti(f, "planes", 0) != 0, geti(f, "slots", 512),
                  switches(f), &p)) {
        printf("rc=1 need_slots=%d error=%s\n", p.need_slots, p.error);
        return;
    }
    printf("rc=0 family=%s cb=%d full=%d tail=%d grid=%u lds=%zu flops=%.0f name=%s\n", FAMILY[p.family], p.cb, p.full_tiles, p.tail_tiles, p.grid, p.lds, p.flops, p.name);
}

void print_ws(const Fields& f) {
    vpho_score_weights w;
    memset(&w, 0, sizeof(w));
    w.D = geti(f, "D", 96); w.Dp = geti(f, "Dp", w.D); w.nheads = geti(f, "nheads", w.D / 3);
    const int bs = geti(f, "bs", 1), S = geti(f, "S", 1);
    char* const base = (char*)(uintptr_t)0x10000000;
    const Workspace ws = carve(w, bs, S, base);
    const void* const slices[] = {ws.cimg, ws.ct, ws.X, ws.P1, ws.P2, ws.K, ws.tmp, ws.y, ws.ynew, ws.partial, ws.result, ws.nan_count, ws.ctl, ws.te, ws.dense_p, ws.log};
    int aligned = 1, ascending = 1;
    uintptr_t prev = 0;
    for (const void* s : slices) {
        const uintptr_t a = (uintptr_t)s;
        aligned &= a % 256 == 0;
        ascending &= a > prev;
        prev = a;
    }
    printf("bytes=%lld sizing=%lld slices=%zu aligned=%d ascending=%d first=%lld last=%lld\n", ws.bytes, carve(w, bs, S, nullptr).bytes, sizeof(slices) / sizeof(slices[0]),
           aligned, ascending, (long long)((char*)ws.cimg - base), (long long)((char*)ws.log - base));
}

void print_comb(const Fields& f) {
    if (geti(f, "s", 1) < 1 || geti(f, "s", 1) > 6) { printf("not planned: an attempt has stages 1..6\n"); return; }
    const LinComb lc = stage_comb(geti(f, "s", 1));
    printf("n=%d h=%g c=", lc.n, lc.h);
    for (int j = 0; j < 7; ++j) printf("%s%.17g", j ? "," : "", lc.c[j]);
    printf(" at=%.17g\n", lc.n < 6 ? RK_C[lc.n] : 1.0);
}

void print_teval(const Fields& f) {
    static double te[CTL_MAX_STEPS];
    const int n = geti(f, "n", 1);
    if (n < 1 || n > CTL_MAX_STEPS) { printf("not planned: 1 <= n <= %d\n", CTL_MAX_STEPS); return; }
    t_eval_linspace(get(f, "T0", 1.0), get(f, "eps", 1e-5), n, te);
    printf("n=%d te=", n);
    for (int i = 0; i < n; ++i) printf("%s%.17g", i ? "," : "", te[i]);
    printf("\n");
}

// each row of A sums to its C, B sums to 1, E = (B, 0) - the fourth-order weights sums to 0, the dense polynomial at x = 1 is B
void print_tableau() {
    double worst = 0, b = 0, e = 0;
    for (int s = 0; s < 6; ++s) {
        double a = 0;
        for (int j = 0; j < 5; ++j) a += RK_A[s][j];
        worst = std::fmax(worst, std::fabs(a - RK_C[s]));
        b += RK_B[s];
    }
    for (int j = 0; j < 7; ++j) e += RK_E[j];
    double p1 = 0;
    for (int j = 0; j < 7; ++j) {
        const double pj = RK_P[j][0] + RK_P[j][1] + RK_P[j][2] + RK_P[j][3];
        p1 = std::fmax(p1, std::fabs(pj - (j < 6 ? RK_B[j] : 0.0)));
    }
    printf("a_rows_sum_to_c=%d b_sums_to_1=%d e_sums_to_0=%d p_at_1_is_b=%d rkctl_bytes=%d max_steps=%d log_cap=%d\n", worst < 1e-15, std::fabs(b - 1) < 1e-15,
           std::fabs(e) < 1e-15, p1 < 1e-14, RKCTL_BYTES, CTL_MAX_STEPS, CTL_LOG_CAP);
}

}  // namespace

int main() {
    static char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        std::string kind;
        const Fields f = parse_fields(line, &kind);
        if (kind == "pe") print_pe(f);
        else if (kind == "head") print_head(f);
        else if (kind == "ws") print_ws(f);
        else if (kind == "comb") print_comb(f);
        else if (kind == "teval") print_teval(f);
        else if (kind == "tableau") print_tableau();
        else { printf("unknown kind '%s'\n", kind.c_str()); return 2; }
    }
    return 0;
}
