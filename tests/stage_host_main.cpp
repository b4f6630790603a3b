// stage_host_main.cpp — the host-only parts of csrc/td_stage.h and csrc/td_sim_layout.h without the HIP runtime: the layouts
// of both world handles over a grid of sizes, and the ragged-offset check.  tests/test_stage_cpu.py compiles this with the
// host compiler and -fsanitize=address,undefined and runs it; it prints "ok" and exits 0, or says what failed and exits 1.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

struct Take {
    size_t off, bytes, align;
};
static std::vector<Take> g_takes;
#define TD_CARVE_TRACE(off, bytes, align) g_takes.push_back(Take{(off), (bytes), (align)})
#define TD_STAGE_HOST_ONLY 1
#include "td_sim_layout.h"

using td::Carve;
using namespace tdsim;

static int g_failed = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAILED %s: ", #cond);         \
            printf(__VA_ARGS__);                  \
            printf("\n");                         \
            g_failed++;                           \
        }                                         \
    } while (0)

// runs `layout` on a null base and on an allocation of exactly the size the first pass gave: the second pass ends there, the
// arrays ascend without overlap, 8-byte types are 8-byte aligned, and every array can be written from end to end (the
// sanitizer sees a byte past the allocation) and keeps what was written into it
template <class L>
static void check_layout(const char *what, L layout)
{
    g_takes.clear();
    Carve size;
    layout(size);
    const std::vector<Take> first = g_takes;
    size_t end = 0;
    for (const Take &t : first) {
        CHECK(t.off >= end, "%s: an array at %zu begins before the end %zu of the one in front", what, t.off, end);
        CHECK(t.off % t.align == 0, "%s: an array at %zu is not aligned to %zu", what, t.off, t.align);
        CHECK(t.off - end < t.align, "%s: a gap of %zu bytes, more than alignment asks for", what, t.off - end);
        end = t.off + t.bytes;
    }
    CHECK(end == size.at, "%s: the first pass ends at %zu, its arrays at %zu", what, size.at, end);
    char *mem = (char *)malloc(size.at ? size.at : 1);
    g_takes.clear();
    Carve c(mem);
    layout(c);
    CHECK(c.at == size.at, "%s: the second pass ends at %zu, the first at %zu", what, c.at, size.at);
    CHECK(g_takes.size() == first.size(), "%s: the passes differ in their arrays", what);
    for (size_t i = 0; i < g_takes.size() && i < first.size(); i++) {
        CHECK(g_takes[i].off == first[i].off && g_takes[i].bytes == first[i].bytes, "%s: array %zu moved between the passes", what, i);
        memset(mem + g_takes[i].off, (int)(i % 251) + 1, g_takes[i].bytes);
    }
    for (size_t i = 0; i < g_takes.size(); i++)
        for (size_t q = 0; q < g_takes[i].bytes; q++)
            if (mem[g_takes[i].off + q] != (char)((i % 251) + 1)) {
                CHECK(false, "%s: array %zu was overwritten by another", what, i);
                break;
            }
    free(mem);
}

static void layouts()
{
    const int cabs[] = {1, 2, 255, 256, 257}, reqs[] = {0, 1, 2, 257}, stands[] = {1, 31, 32, 33}, worlds[] = {1, 2, 3};
    for (int n_cabs : cabs)
        for (int n_req : reqs)
            for (int n_stands : stands)
                for (int B : worlds)
                    for (int dist = 0; dist < 2; dist++) {
                        char what[96];
                        snprintf(what, sizeof(what), "cabs %d requests %d stands %d worlds %d table %d", n_cabs, n_req, n_stands, B, dist);
                        const size_t words = (size_t)(n_stands + 31) / 32, ns = (size_t)n_stands;
                        {   // td_sim: one world (sim_create's sizes)
                            const size_t nr = (size_t)std::max(n_req, 1), nc = (size_t)n_cabs, cap = std::max(nr, nc);
                            const SimDims d{nc, nr, cap, words, (cap + 1023) / 1024, ns, dist != 0};
                            SimDev s;
                            SimPin p;
                            check_layout(what, [&](Carve &c) { sim_layout(c, d, s); });
                            check_layout(what, [&](Carve &c) { sim_pin_layout(c, d, p); });
                            // the cab and request bits are one array, the near bitsets lie behind them
                            if (dist) CHECK(s.near == s.bits + 2 * words, "%s: td_sim's near bitsets are not behind its bits", what);
                            CHECK((char *)p.h_rows == p.h_head + SIM_PIN_HEAD, "%s: td_sim's pinned results do not follow the head", what);
                        }
                        {   // td_simb: B worlds of these sizes (simb_create's sizes)
                            const size_t nb = (size_t)B, nc = nb * n_cabs, nr = std::max<size_t>(nb * n_req, 1);
                            const size_t big = (size_t)std::max(n_cabs, n_req), ncap = std::max<size_t>(1, std::min<size_t>(2048, big));
                            const size_t hcap = std::max<size_t>(1, std::min<size_t>(2048, n_req) / 2);
                            const SimbDims d{nb, nc, nr, words, ns, nb * std::max<size_t>(1, (big + 1023) / 1024), std::max(nb * hcap, nr / 2 + 1),
                                             nb * std::max<size_t>(big, 1), nb * ncap, (size_t)std::max(n_cabs, 1), dist != 0};
                            SimbDev s;
                            SimbPin p;
                            check_layout(what, [&](Carve &c) { simb_layout(c, d, s); });
                            check_layout(what, [&](Carve &c) { simb_pin_layout(c, d, p); });
                            for (const void *a : {(void *)s.p_total, (void *)s.tk_total, (void *)s.ctl_blk})
                                CHECK((uintptr_t)a % 8 == 0, "%s: a 64-bit array of td_simb is not 8-byte aligned", what);
                            // create zeroes the 64-bit arrays and the head with one memset from the block's start
                            CHECK((int32_t *)s.tk_total == (int32_t *)s.p_total + 2 * nb &&
                                      (int32_t *)s.ctl_blk == (int32_t *)s.p_total + 4 * nb && s.gerr == (int32_t *)s.ctl_blk + 16 * nb &&
                                      s.dem_off == s.gerr + 16,
                                  "%s: td_simb's front block is not p_total, tk_total, Ctl[B], the error word, the offsets", what);
                            // the seven offset arrays and the four per-world arrays: cleared by one memset, read back with the head
                            int32_t *const blk[] = {s.dem_off, s.sup_off, s.pl_off, s.d2_off, s.tk_off, s.ks_off, s.kd_off, s.n_pools, s.tk_np, s.tk_lm, s.tk_rest};
                            for (int q = 0; q < 11; q++)
                                CHECK(blk[q] == s.dem_off + (q < 7 ? q * (nb + 1) : 7 * (nb + 1) + (q - 7) * nb), "%s: array %d of td_simb's per-tick block is not in its place", what, q);
                            CHECK(s.tk_rest + nb == (int32_t *)s.ctl_blk + d.head_ints(), "%s: td_simb's head is not head_ints long", what);
                            // uploaded by one copy
                            CHECK(s.in_r2c_off == s.in_pair_off + nb + 1 && s.in_solved == s.in_r2c_off + nb + 1, "%s: in_pair_off / in_r2c_off / in_solved are not adjacent", what);
                            if (dist) CHECK(s.near != nullptr && s.dist != nullptr, "%s: a table batch without its table", what);
                            CHECK(p.h_stage == p.h_head + d.head_ints(), "%s: td_simb's pinned stage does not follow the head's mirror", what);
                        }
                    }
}

// ragged_check's reporter: keeps the text as td::fail does
static char g_err[512];
static int report(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static void offsets()
{
    struct Case {
        std::vector<int32_t> h;
        int rc, longest, total;
        const char *text;
    };
    const Case cases[] = {
        {{0, 2, 2, 4}, TD_OK, 2, 4, ""},
        {{1, 2, 3, 4}, TD_EINVAL, 0, 0, "fn: x[0] = 1, not 0"},
        {{0, 3, 2, 4}, TD_EINVAL, 0, 0, "fn: x decreases at world 1 (3 -> 2)"},
        {{0, 5, 5, 5}, TD_EINVAL, 0, 0, "fn: world 0 has 5, more than 4"},   // the caller's refusal, in the caller's words
        {{0}, TD_OK, 0, 0, ""},                                              // an empty batch
        {{0, 0}, TD_OK, 0, 0, ""},                                           // one empty model
        {{0, 4}, TD_OK, 4, 4, ""},                                           // one model
    };
    for (const Case &c : cases) {
        const int count = (int)c.h.size() - 1;
        td::Ragged r;
        g_err[0] = 0;
        const int rc = td::ragged_check(report, "fn", "x", "world", c.h.data(), count, &r,
                                        [&](int b, int m) { return m > 4 ? report(TD_EINVAL, "fn: world %d has %d, more than 4", b, m) : 0; });
        CHECK(rc == c.rc && std::string(g_err) == c.text, "offsets of %d segments: rc %d, \"%s\"", count, rc, g_err);
        if (rc == TD_OK) CHECK(r.longest == c.longest && r.total == c.total, "offsets of %d segments: longest %d, total %d", count, r.longest, r.total);
    }
    // without a caller's rule a long segment is fine
    const int32_t h[] = {0, 5, 5, 5};
    td::Ragged r;
    CHECK(td::ragged_check(report, "fn", "x", "model", h, 3, &r) == TD_OK && r.longest == 5 && r.total == 5, "the check without a caller's rule");
}

int main()
{
    layouts();
    offsets();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}
