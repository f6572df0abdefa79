// Sweeps the window's span rule (rs-pathplanning_amd/csrc/pp_window_fill.h) on the host: window
// sizes Kw, iteration counts on both sides of Kw and 2 Kw, and patterns of draws in an obstacle.
// Every case is cut into consecutive windows, each checked against a one-draw-at-a-time count
// written here.  Prints one JSON line; exits 1 with the first violated property on stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pp_window_fill.h"

using namespace ppamd;

static std::string g_case;

#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s Kw=%d N=%d start=%d: ", g_case.c_str(), Kw, N, start); \
            std::fprintf(stderr, __VA_ARGS__);                                    \
            std::fprintf(stderr, " (%s)\n", #cond);                               \
            return false;                                                         \
        }                                                                         \
    } while (0)

static long g_windows = 0, g_cases = 0, g_max_draws4096 = 0;

// the iterations [0, N) with blocked[i], cut into windows of Kw samples drawn in rounds of
// (first, later): every window against the rule counted one draw at a time
static bool run_case(int Kw, const std::vector<char>& blocked, bool pretest, int first, int later) {
    const int N = (int)blocked.size();
    std::vector<int> off((size_t)Kw + 1, -7);
    std::vector<int> live_its;  // what the windows' samples must be, in order
    for (int i = 0; i < N; ++i)
        if (!pretest || !blocked[i]) live_its.push_back(i);
    size_t next_live = 0;
    int start = 0;
    ++g_cases;
    while (start < N) {
        const int64_t rem = N - start;
        off.assign((size_t)Kw + 1, -7);
        int drawn = -1;
        const WindowFill f = window_fill_seq(
            Kw, rem, pretest, first, later, [&](int i) { return blocked[(size_t)(start + i)] != 0; },
            off.data(), &drawn);
        ++g_windows;
        const int C = (int)std::min<int64_t>(pretest ? 2 * (int64_t)Kw : Kw, rem);
        CHECK(C == window_fill_cap(Kw, rem, pretest), "cap %d", C);
        CHECK(f.W >= 0 && f.W <= Kw, "W %d", f.W);
        CHECK(f.span >= 1 && f.span <= C, "span %d of %d", f.span, C);
        CHECK(off[(size_t)Kw] == -7, "iter_off written past Kw entries");
        // the rule, one draw at a time: the span ends before the (Kw + 1)-th live draw
        int live = 0, want = C;
        for (int i = 0; i < C; ++i) {
            if (pretest && blocked[(size_t)(start + i)]) continue;
            if (live == Kw) {
                want = i;
                break;
            }
            ++live;
        }
        CHECK(f.span == want, "span %d, counted %d", f.span, want);
        int inside = 0;
        for (int i = 0; i < f.span; ++i) inside += !(pretest && blocked[(size_t)(start + i)]);
        CHECK(f.W == inside, "W %d, live draws inside the span %d", f.W, inside);
        // maximal: draw `span` is live and would be sample Kw, or the cap stopped the window
        CHECK(f.span == C || (f.W == Kw && !(pretest && blocked[(size_t)(start + f.span)])),
              "span %d is not maximal", f.span);
        for (int id = 0; id < f.W; ++id) {
            CHECK(off[(size_t)id] >= 0 && off[(size_t)id] < f.span, "iter_off[%d] = %d", id, off[(size_t)id]);
            CHECK(id == 0 || off[(size_t)id] > off[(size_t)id - 1], "iter_off[%d] not increasing", id);
            CHECK(next_live < live_its.size() && live_its[next_live] == start + off[(size_t)id],
                  "sample %d is iteration %d", id, start + off[(size_t)id]);
            ++next_live;
        }
        // the draws made: enough to decide the span, never past the cap, whole rounds
        CHECK(drawn <= C && drawn >= f.span + (f.span < C ? 1 : 0), "drawn %d", drawn);
        CHECK(drawn == C || drawn == first || (drawn > first && (drawn - first) % later == 0),
              "drawn %d is no whole round", drawn);
        if (!pretest) CHECK(f.span == f.W && f.W == C, "no pre-test: W %d span %d", f.W, f.span);
        if (Kw == 4096 && drawn > g_max_draws4096) g_max_draws4096 = drawn;
        start += f.span;  // the next window: no gap, no overlap
    }
    {
        const int start = N;
        CHECK(next_live == live_its.size(), "%zu of %zu live iterations sampled", next_live, live_its.size());
        const WindowFill f = window_fill_seq(Kw, 0, pretest, first, later, [](int) { return false; }, off.data());
        CHECK(f.W == 0 && f.span == 0, "a window at the target is empty");
    }
    return true;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

int main() {
    const int kws[] = {1, 2, 7, 64, 4096};
    // (the first: samples_role's)
    const int rounds[][2] = {{4096, 2048}, {64, 32}, {3, 2}};
    for (int Kw : kws) {
        const int ns[] = {Kw - 1, Kw, Kw + 1, 2 * Kw - 1, 2 * Kw, 2 * Kw + 1, 5 * Kw + 3};
        for (int N : ns) {
            if (N < 1) continue;
            std::vector<std::pair<std::string, std::vector<char>>> pats;
            auto add = [&](const std::string& name, std::vector<char> v) { pats.emplace_back(name, std::move(v)); };
            add("none", std::vector<char>((size_t)N, 0));
            add("all", std::vector<char>((size_t)N, 1));
            {
                std::vector<char> a((size_t)N), b((size_t)N);
                for (int i = 0; i < N; ++i) {
                    a[(size_t)i] = i & 1;
                    b[(size_t)i] = !(i & 1);
                }
                add("alt0", a);
                add("alt1", b);
            }
            for (int L : {Kw - 1, Kw, Kw + 1}) {  // one blocked run at the start, middle, end
                if (L < 1 || L > N) continue;
                for (int where = 0; where < 3; ++where) {
                    const int a = where == 0 ? 0 : where == 1 ? (N - L) / 2 : N - L;
                    std::vector<char> v((size_t)N, 0);
                    for (int i = a; i < a + L; ++i) v[(size_t)i] = 1;
                    add("run" + std::to_string(L) + "@" + std::to_string(a), v);
                }
            }
            if (N >= 2 * Kw) {
                // the (Kw + 1)-th live draw is the last drawable one (draw 2 Kw - 1) ...
                std::vector<char> v((size_t)N, 0);
                for (int i = Kw; i < 2 * Kw - 1; ++i) v[(size_t)i] = 1;
                add("next_last", v);
                // ... and one past it (the cap stops the window, the draw opens the next)
                std::vector<char> w((size_t)N, 0);
                for (int i = Kw; i < 2 * Kw && i < N; ++i) w[(size_t)i] = 1;
                add("next_past", w);
                // a blocked run straddling the cap
                std::vector<char> s((size_t)N, 0);
                for (int i = 2 * Kw - (Kw + 1) / 2; i < N && i < 2 * Kw + (Kw + 1) / 2; ++i) s[(size_t)i] = 1;
                add("straddle", s);
            }
            for (int pct : {10, 32, 50, 90}) {
                std::vector<char> v((size_t)N);
                for (int i = 0; i < N; ++i) v[(size_t)i] = rnd() * 100.0 < pct;
                add("rand" + std::to_string(pct), v);
            }
            for (auto& p : pats)
                for (auto& r : rounds) {
                    g_case = p.first + " rounds " + std::to_string(r[0]) + "/" + std::to_string(r[1]);
                    if (!run_case(Kw, p.second, true, r[0], r[1])) return 1;
                    g_case += " no pre-test";
                    if (!run_case(Kw, p.second, false, r[0], r[1])) return 1;
                }
        }
    }
    std::printf("{\"cases\": %ld, \"windows\": %ld, \"max_draws4096\": %ld}\n", g_cases, g_windows,
                g_max_draws4096);
    return 0;
}
