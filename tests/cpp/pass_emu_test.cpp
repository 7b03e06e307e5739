// pass_emu_test.cpp -- the FFT pass kernels themselves (tile_fft_kernel, row_fft_kernel, r2c_last_pass_kernel, c2r_first_pass_kernel,
// wave_fft_kernel, quad_fft_kernel), run on the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_pass_emulator.py
// builds and runs it; tests/emu/block_shim.hpp runs a workgroup as fibers that meet at __syncthreads() and, wave by wave, at the
// cross-lane swaps, wave_barrier and readfirstlane).  One translation unit per product unit (PASS_PART = 1..15, the .hip file #included
// as it stands) and one for main (PASS_PART = 0); argv[1] names the part, argv[2] may narrow a tile part to one shape "LR,LC,LP".
//
// The other host tests of these passes run emulate_tile_pass, emulate_row_fft, emulate_wave_pass ...: second, hand-written schedules
// of the same phase functions, without the kernels' barriers, LDS carve-up, table staging, persistent loop, prefetch and uniformity
// claims.  Here every pass is launched through the product's own launcher (its LDS size, its block size) and runs once through the
// KERNEL on the shim and once through the matching emulate_* function on the same arguments; the outputs -- the whole heap blocks,
// batch gaps and padding included -- must have EQUAL BITS: both sides run the same phase functions in the same order of roundings
// with the host's arithmetic (one translation unit, one set of flags, no FMA contraction on x86-64 without -mfma).  No kernel path
// here is a different sequence of roundings from its emulator's, so no tolerance appears anywhere in this file.
//
// Every table, input plane, scratch plane and output plane is a heap block of exactly the elements the planner allocates
// (plan.hpp: host_twr / host_twq / host_tw3, scratch_elems), so a staging loop or a prefetch that reads one entry too far is an
// AddressSanitizer report, as is an LDS offset past the launch's dynamic LDS.  Everything runs in ascending and in descending thread
// order.  The shapes come from the product's macros (PHAST_TILE_SHAPES, PHAST_TILE_SHAPES_F32, PHAST_ROW_SHAPES) and its plan
// enumerator (enumerate_plans): for a tile shape the shortest transform that has a plan with that pass in that position.
#ifndef PASS_PART
#error "compile with -DPASS_PART=0 (main) .. 15"
#endif

#if PASS_PART == 0
// ------------------------------------------------------------------------------------------------------------ main
#include <cstdio>
#include <cstring>

#include "sanitizer_exit.hpp"

int pass_tile_f64_a(const char *);
int pass_tile_f64_bc(const char *);
int pass_tile_f32_a(const char *);
int pass_tile_f32_bc(const char *);
int pass_tile_f64_r2c(const char *);
int pass_tile_f32_r2c(const char *);
int pass_tile_f64_c2r(const char *);
int pass_tile_f32_c2r(const char *);
int pass_wave_f64(const char *);
int pass_wave_f32(const char *);
int pass_quad_f64(const char *);
int pass_quad_f32(const char *);
int pass_small_fft(const char *);
// the two units that hold ONE instantiation each (tile_dispatch.hpp) are reached through the dispatcher of the pre-twiddle unit
static int pass_tile_f64_bc_wide(const char *) { return pass_tile_f64_bc("10,4,5"); }
static int pass_tile_f32_bc_wide(const char *) { return pass_tile_f32_bc("10,5,5"); }

int main(int argc, char **argv) {
    struct Part {
        const char *name;
        int (*run)(const char *);
    };
    const Part parts[] = {{"tile_f64_a", pass_tile_f64_a},     {"tile_f64_bc", pass_tile_f64_bc},   {"tile_f64_bc_wide", pass_tile_f64_bc_wide},
                          {"tile_f32_a", pass_tile_f32_a},     {"tile_f32_bc", pass_tile_f32_bc},   {"tile_f32_bc_wide", pass_tile_f32_bc_wide},
                          {"tile_f64_r2c", pass_tile_f64_r2c}, {"tile_f32_r2c", pass_tile_f32_r2c}, {"tile_f64_c2r", pass_tile_f64_c2r},
                          {"tile_f32_c2r", pass_tile_f32_c2r}, {"wave_f64", pass_wave_f64},         {"wave_f32", pass_wave_f32},
                          {"quad_f64", pass_quad_f64},         {"quad_f32", pass_quad_f32},         {"small_fft", pass_small_fft}};
    int fails = 0, ran = 0;
    for (const Part &p : parts) {
        if (argc < 2 || std::strcmp(argv[1], p.name) != 0) continue;
        ++ran;
        const int f = p.run(argc > 2 ? argv[2] : "");
        std::printf("%s: %s (%d failures)\n", p.name, f ? "FAILED" : "ok", f);
        fails += f;
    }
    if (!ran) {
        std::printf("usage: %s <part> [LR,LC,LP]; parts:", argv[0]);
        for (const Part &p : parts) std::printf(" %s", p.name);
        std::printf("\n");
        phast_test_exit(2);
    }
    phast_test_exit(fails ? 1 : 0);
}

#else
// ------------------------------------------------------------------------------------------------------------ a part
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#if PASS_PART == 1
#include "tile_f64_a.hip"
#elif PASS_PART == 2
#include "tile_f64_bc.hip"
#elif PASS_PART == 3
#include "tile_f64_bc_wide.hip"
#elif PASS_PART == 4
#include "tile_f32_a.hip"
#elif PASS_PART == 5
#include "tile_f32_bc.hip"
#elif PASS_PART == 6
#include "tile_f32_bc_wide.hip"
#elif PASS_PART == 7
#include "tile_f64_r2c.hip"
#elif PASS_PART == 8
#include "tile_f32_r2c.hip"
#elif PASS_PART == 9
#include "tile_f64_c2r.hip"
#elif PASS_PART == 10
#include "tile_f32_c2r.hip"
#elif PASS_PART == 11
#include "wave_f64.hip"
#elif PASS_PART == 12
#include "wave_f32.hip"
#elif PASS_PART == 13
#include "quad_f64.hip"
#elif PASS_PART == 14
#include "quad_f32.hip"
#elif PASS_PART == 15
#include "small_fft.hip"
#include "plan.hpp"
#endif

#if PASS_PART != 3 && PASS_PART != 6  // (those two are an explicit instantiation and nothing else)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {
using namespace phast;
using u64 = unsigned long long;
using u32 = unsigned;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = u64;
    static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    static const char *name() { return "f64"; }
    static const char *type() { return "double"; }
};
template <> struct Fp<float> {
    using bits = u32;
    static constexpr bits sentinel = 0x7fc5eed1u;
    static const char *name() { return "f32"; }
    static const char *type() { return "float"; }
};

char g_case[400] = "";
int g_fails = 0, g_printed = 0;
void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
// FAIL <kernel instantiation> [case]: ...; the first few are printed, the count is in the summary line
void fail(const std::string &kernel, const char *fmt, ...) {
    ++g_fails;
    if (++g_printed > 40) return;
    std::printf("FAIL %s [%s]: ", kernel.c_str(), g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}
const char *order_name() { return block_shim::order == block_shim::kAscending ? "ascending" : "descending"; }
void set_order(int ord) { block_shim::order = ord ? block_shim::kDescending : block_shim::kAscending; }

// the kernel-only branches a part has run (what the emulate_* functions have no counterpart of); told from the launch itself:
// the grid against the tile count, the kernel's own constants against the arguments
struct Branches {
    bool prog_lds = false, tw_global = false, second_iteration = false, guard_false = false, early_waves = false;
} g_br;
void note_loop(unsigned grid, unsigned tiles) {
    if (grid < tiles) g_br.second_iteration = true;  // workgroup 0 walks tiles 0, grid, ..
    if (tiles > 0 && grid <= tiles) g_br.guard_false = true;  // ... and leaves when t >= tiles_total: the prefetch is not issued
}
int finish(const char *prefix, std::vector<std::string> must, bool need_prog, bool need_loop, bool need_early) {
    set_case("coverage");
    std::sort(must.begin(), must.end());
    must.erase(std::unique(must.begin(), must.end()), must.end());
    for (int ord = 0; ord < 2; ++ord)
        for (const std::string &k : must) {
            bool found = false;
            for (const auto &kv : block_shim::ran_in[ord]) found |= kv.first.find(k) != std::string::npos;
            if (!found) fail(k, "this instantiation was never launched in %s order: the cases no longer reach it", ord ? "descending" : "ascending");
        }
    size_t mine = 0;
    for (const auto &kv : block_shim::ran)
        if (kv.first.find(prefix) != std::string::npos || kv.first.find("one_point_kernel") == 0) {
            ++mine;
            std::printf("  ran %-150s %6llu launches\n", kv.first.c_str(), kv.second);
        }
    std::printf("  instantiations of %s launched: %zu (required: %zu, each in both orders)\n", prefix, mine, must.size());
    std::printf("  branch PROG with the table in LDS: %s\n", g_br.prog_lds ? "ran" : "did not run");
    std::printf("  branch tw_global: %s\n", g_br.tw_global ? "ran" : "did not run (needs the three-level tables of a 2^28-point transform)");
    std::printf("  branch second loop iteration: %s\n", g_br.second_iteration ? "ran" : "did not run");
    std::printf("  branch prefetch guard false: %s\n", g_br.guard_false ? "ran" : "did not run");
    std::printf("  branch early-returning waves: %s\n", g_br.early_waves ? "ran" : "did not run");
    if (need_prog && !g_br.prog_lds) fail("branches", "PROG with the table in LDS did not run");
    if (need_loop && !g_br.second_iteration) fail("branches", "no workgroup ran a second loop iteration");
    if (need_loop && !g_br.guard_false) fail("branches", "the prefetch guard was never false");
    if (need_early && !g_br.early_waves) fail("branches", "no wave returned early");
    block_shim::print_counters();
    return g_fails;
}

template <typename T> void fill_sentinel(std::vector<T> &v) {
    for (T &x : v) std::memcpy(&x, &Fp<T>::sentinel, sizeof(T));
}
template <typename T> void fill_pm1(std::vector<T> &v, u64 id) {
    for (size_t i = 0; i < v.size(); ++i) v[i] = (T)uniform_pm1(0x5eedull, id, i);
}
// index of the first element whose bits differ, or -1
template <typename T> long long first_diff(const std::vector<T> &a, const std::vector<T> &b) {
    if (a.size() != b.size()) return 0;
    if (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T))) return -1;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(&a[i], &b[i], sizeof(T))) return (long long)i;
    return -1;
}
template <typename T> u64 bits_of(T x) {
    typename Fp<T>::bits b;
    std::memcpy(&b, &x, sizeof(T));
    return (u64)b;
}

// the grid exec.hpp gives a pass on a chip with more compute units than these shapes have tiles
unsigned own_grid(unsigned tiles, bool always_round = false) {
    unsigned g = tiles;
    if (g >= 8 && (always_round || (tiles & 7u) == 0u)) g &= ~7u;
    return g;
}

#if PASS_PART != 15
// ---- a plan on host memory: planes, scratch and tables as Planner::exec_in / emu_exec (tests/emu/emu.hip) set them up ----
template <typename T> hipError_t launch_any(const PassGeom &p, unsigned grid, const TileArgs &ta) {
    if constexpr (sizeof(T) == 8) {
        return p.wave        ? launch_wave_f64(p.transpose, nullptr, ta, false, nullptr, nullptr)
               : p.quad      ? launch_quad_f64(grid, nullptr, ta, false, nullptr, nullptr)
               : p.transpose ? launch_tile_f64_a((int)p.lr, (int)p.lc, (int)p.lp, grid, nullptr, ta, false, nullptr, nullptr)
                             : launch_tile_f64_bc((int)p.lr, (int)p.lc, (int)p.lp, grid, nullptr, ta, false, nullptr, nullptr);
    } else {
        return p.wave        ? launch_wave_f32(p.transpose, nullptr, ta, false, nullptr, nullptr)
               : p.quad      ? launch_quad_f32(grid, nullptr, ta, false, nullptr, nullptr)
               : p.transpose ? launch_tile_f32_a((int)p.lr, (int)p.lc, (int)p.lp, grid, nullptr, ta, false, nullptr, nullptr)
                             : launch_tile_f32_bc((int)p.lr, (int)p.lc, (int)p.lp, grid, nullptr, ta, false, nullptr, nullptr);
    }
}

template <typename T> struct State {
    std::vector<T> s_re, s_im, out_re, out_im;
};
// in_kind / out_kind: 0 = planar complex of n points, 1 = the R2C side (in: n (even, odd) pairs in ONE array; out: planar n + 1),
// 2 = the C2R side (in: planar n + 1)
template <typename T> struct Plan {
    unsigned L;
    size_t n, batch, in_dist, out_dist, sd;
    std::vector<PassGeom> ps;
    std::vector<T> in_re, in_im;
    State<T> st;
    std::vector<std::vector<cx_t<T>>> twr, tw3;
    int in_kind, out_kind;
    bool ok;
    Plan(unsigned L_, const PlanSpec &s, size_t batch_, int in_kind_ = 0, int out_kind_ = 0)
        : L(L_), n((size_t)1 << L_), batch(batch_), in_kind(in_kind_), out_kind(out_kind_) {
        ok = make_passes(L, s.lrs(), s.tls(), ps, s.lp, sizeof(T));
        if (!ok) return;
        const size_t in_n = in_kind == 2 ? n + 1 : n, out_n = out_kind == 1 ? n + 1 : n;
        in_dist = batch == 1 ? in_n : in_n + 5;  // a batch of 3 at a distance above n
        out_dist = batch == 1 ? out_n : out_n + 3;
        sd = (size_t)scratch_elems(ps, L);
        in_re.resize(((batch - 1) * in_dist + in_n) * (in_kind == 1 ? 2 : 1));
        in_im.resize(in_kind == 1 ? 0 : in_re.size());
        st.s_re.resize(sd * batch);
        st.s_im.resize(sd * batch);
        st.out_re.resize((batch - 1) * out_dist + out_n);
        st.out_im.resize(st.out_re.size());
        for (const PassGeom &p : ps) {
            twr.push_back(p.quad ? host_twq<T>() : host_twr<T>(1u << p.lr));
            tw3.push_back(p.pre_tw ? host_tw3<T>(p.log_mod(), p.tw_bits) : std::vector<cx_t<T>>());
        }
        fill_pm1(in_re, 1);
        fill_pm1(in_im, 2);
        fill_sentinel(st.s_re);
        fill_sentinel(st.s_im);
        fill_sentinel(st.out_re);
        fill_sentinel(st.out_im);
    }
    TileArgs args(size_t i) {
        const PassGeom &p = ps[i];
        TileArgs ta{};
        const bool first = i == 0, last = i + 1 == ps.size();
        ta.in_re = first ? (const void *)in_re.data() : (const void *)st.s_re.data();
        ta.in_im = first ? (in_kind == 1 ? nullptr : (const void *)in_im.data()) : (const void *)st.s_im.data();
        ta.in_dist = first ? in_dist : sd;
        ta.in_interleaved = first && in_kind == 1 ? 1 : 0;
        ta.out_re = last ? st.out_re.data() : st.s_re.data();
        ta.out_im = last ? st.out_im.data() : st.s_im.data();
        ta.out_dist = last ? out_dist : sd;
        ta.out_interleaved = 0;
        ta.scale = 1.0;
        ta.tw3 = tw3[i].data();
        ta.twr = twr[i].data();
        geom_to_args(p, L, batch, ta);
        return ta;
    }
    // the passes before `pos`, through the product's launchers in the grid the planner gives them
    bool run_before(size_t pos) {
        set_order(0);
        for (size_t i = 0; i < pos; ++i) {
            const TileArgs ta = args(i);
            if (launch_any<T>(ps[i], own_grid(ta.tiles_total), ta) != hipSuccess) return false;
        }
        return true;
    }
};
template <typename T> void compare(const State<T> &got, const State<T> &want, bool last, const Plan<T> &pl) {
    const std::vector<T> *g[4] = {&got.s_re, &got.s_im, &got.out_re, &got.out_im}, *w[4] = {&want.s_re, &want.s_im, &want.out_re, &want.out_im};
    const char *names[4] = {"scratch re", "scratch im", "out re", "out im"};
    for (int k = 0; k < 4; ++k) {
        const long long at = first_diff(*g[k], *w[k]);
        if (at >= 0)
            fail(block_shim::last_kernel, "%s[%lld]: the kernel gives bits %llx, %s %llx", names[k], at, bits_of((*g[k])[(size_t)at]),
                 "the emulator", bits_of((*w[k])[(size_t)at]));
    }
    if (last && pl.batch > 1) {  // the gaps between the transforms of the caller's planes
        const size_t out_n = pl.out_kind == 1 ? pl.n + 1 : pl.n;
        for (size_t b = 0; b + 1 < pl.batch; ++b)
            for (size_t i = b * pl.out_dist + out_n; i < (b + 1) * pl.out_dist; ++i)
                if (bits_of(got.out_re[i]) != (u64)Fp<T>::sentinel || bits_of(got.out_im[i]) != (u64)Fp<T>::sentinel)
                    fail(block_shim::last_kernel, "the gap element %zu of the output was written", i);
    }
}

// every plan of a length, once (tile sizes 2^10 .. 2^15: every shape of the macros)
template <typename T> const std::vector<PlanSpec> &plans_of(unsigned L) {
    static std::map<unsigned, std::vector<PlanSpec>> cache;
    auto it = cache.find(L);
    if (it == cache.end()) {
        it = cache.emplace(L, std::vector<PlanSpec>()).first;
        enumerate_plans(L, sizeof(T), 1, 10, 15, it->second);
    }
    return it->second;
}
// the shortest transform with a plan (of the fewest passes) whose pass `which` (0 = first, 1 = any later, 2 = last) is the generic
// tile kernel of this shape; `extra` may refuse a pass (the fused forms' conditions)
template <typename T, typename Extra>
bool find_plan(int lr, int lc, int lp, int which, unsigned &L_out, PlanSpec &spec, size_t &pos, Extra extra) {
    std::vector<PassGeom> geo;
    for (unsigned L = kTwinMinLog; L <= 24; ++L) {
        unsigned best_np = 9;
        for (const PlanSpec &s : plans_of<T>(L)) {
            if (s.np >= best_np || !make_passes(L, s.lrs(), s.tls(), geo, s.lp, sizeof(T))) continue;
            for (size_t i = 0; i < geo.size(); ++i) {
                const PassGeom &p = geo[i];
                if (which == 0 ? i != 0 : which == 2 ? i + 1 != geo.size() || i == 0 : i == 0) continue;
                if (p.wave || p.quad || (int)p.lr != lr || (int)p.lc != lc || (int)p.lp != lp || p.transpose != (which == 0)) continue;
                if (!extra(geo, i)) continue;
                best_np = s.np;
                spec = s;
                pos = i;
                L_out = L;
                break;
            }
        }
        if (best_np < 9) return true;
    }
    return false;
}
bool shape_wanted(const char *only, int lr, int lc, int lp) {
    char s[32];
    std::snprintf(s, sizeof s, "%d,%d,%d", lr, lc, lp);
    return !*only || !std::strcmp(only, s);
}
#endif  // PASS_PART != 15

}  // namespace

// ============================================================================================================ tile_fft_kernel
#if PASS_PART == 1 || PASS_PART == 2 || PASS_PART == 4 || PASS_PART == 5
namespace {
#if PASS_PART == 1 || PASS_PART == 2
using TT = double;
#else
using TT = float;
#endif
#if PASS_PART == 1 || PASS_PART == 4
constexpr bool kPreTw = false;
#else
constexpr bool kPreTw = true;
#endif

bool emu_this(const PassGeom &p, const TileArgs &a) {
#define PASS_EMU(LR_, LC_, LP_)                                                          \
    if (p.lr == LR_ && p.lc == LC_ && p.lp == LP_) {                                     \
        using Body = TileBody<TT, LR_, LC_, LP_, kPreTw, !kPreTw, plane_seq_v<TT, LP_>>; \
        if (Body::PROG && !Body::tw3_global(a.tw_bits)) g_br.prog_lds = true;            \
        if (Body::PROG && Body::tw3_global(a.tw_bits)) g_br.tw_global = true;            \
        emulate_tile_pass<TT, LR_, LC_, LP_, kPreTw, !kPreTw, plane_seq_v<TT, LP_>>(a);  \
        return true;                                                                     \
    }
    PHAST_TILE_SHAPES(PASS_EMU)
    if constexpr (sizeof(TT) == 4) {
        PHAST_TILE_SHAPES_F32(PASS_EMU)
    }
#undef PASS_EMU
    return false;
}

void tile_shape(int lr, int lc, int lp) {
    unsigned L = 0;
    PlanSpec spec;
    size_t pos = 0;
    set_case("%s %s %dx%d p%d", Fp<TT>::name(), kPreTw ? "PRE_TW" : "TRANSPOSE", 1 << lr, 1 << lc, 1 << lp);
    if (!find_plan<TT>(lr, lc, lp, kPreTw ? 1 : 0, L, spec, pos, [](const std::vector<PassGeom> &, size_t) { return true; })) {
        fail("tile_fft_kernel", "no plan of enumerate_plans up to 2^24 points has this pass in this position");
        return;
    }
    std::printf("  %s %4d x %-3d p%-2d %s: pass %zu of plan %s, 2^%u points\n", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp,
                kPreTw ? "PRE_TW" : "TRANSPOSE", pos, spec_to_string(spec).c_str(), L);
    for (size_t batch : {(size_t)1, (size_t)3}) {
        Plan<TT> pl(L, spec, batch);
        if (!pl.ok || !pl.run_before(pos)) {
            fail("tile_fft_kernel", "the plan %s could not be set up", spec_to_string(spec).c_str());
            return;
        }
        const State<TT> before = pl.st;
        const TileArgs ta = pl.args(pos);
        const bool last = pos + 1 == pl.ps.size();
        if (!emu_this(pl.ps[pos], ta)) {
            fail("emulate_tile_pass", "no emulator for this shape");
            return;
        }
        const State<TT> want = pl.st;
        const unsigned grids[3] = {own_grid(ta.tiles_total), 1u, 3u};
        for (int ord = 0; ord < 2; ++ord)
            for (unsigned grid : grids) {
                pl.st = before;
                set_order(ord);
                set_case("%s %s %dx%d p%d plan %s (2^%u) pass %zu batch %zu tiles %u grid=%u %s", Fp<TT>::name(), kPreTw ? "PRE_TW" : "TRANSPOSE", 1 << lr,
                         1 << lc, 1 << lp, spec_to_string(spec).c_str(), L, pos, batch, ta.tiles_total, grid, order_name());
                if (launch_any<TT>(pl.ps[pos], grid, pl.args(pos)) != hipSuccess) {
                    fail("tile_fft_kernel", "the launcher refused the pass");
                    continue;
                }
                note_loop(grid, ta.tiles_total);
                compare(pl.st, want, last, pl);
            }
    }
}

int run_part(const char *only) {
    std::vector<std::string> must;
    char key[160];
#define PASS_RUN(LR_, LC_, LP_)                                                                                                              \
    if (shape_wanted(only, LR_, LC_, LP_)) {                                                                                                 \
        tile_shape(LR_, LC_, LP_);                                                                                                           \
        std::snprintf(key, sizeof key, "[T = %s, LR = %d, LC = %d, LP = %d, PRE_TW = %s, TRANSPOSE = %s,", Fp<TT>::type(), LR_, LC_, LP_, \
                      kPreTw ? "true" : "false", kPreTw ? "false" : "true");                                                                 \
        must.push_back(key);                                                                                                                 \
    }
    PHAST_TILE_SHAPES(PASS_RUN)
    if constexpr (sizeof(TT) == 4) {
        PHAST_TILE_SHAPES_F32(PASS_RUN)
    }
#undef PASS_RUN
    if (must.empty()) fail("tile_fft_kernel", "no shape %s", only);
    // the progression form exists in every f32 shape, in f64 from 512 rows x 32 points per thread on: a filtered run may have none
    const bool need_prog = kPreTw && (!*only || sizeof(TT) == 4);
    return finish("launch_tile_inst", must, need_prog, true, false);
}
}  // namespace
#if PASS_PART == 1
int pass_tile_f64_a(const char *only) { return run_part(only); }
#elif PASS_PART == 2
int pass_tile_f64_bc(const char *only) { return run_part(only); }
#elif PASS_PART == 4
int pass_tile_f32_a(const char *only) { return run_part(only); }
#else
int pass_tile_f32_bc(const char *only) { return run_part(only); }
#endif
#endif

// ============================================================================================================ r2c_last_pass_kernel
#if PASS_PART == 7 || PASS_PART == 8
namespace {
#if PASS_PART == 7
using TT = double;
#else
using TT = float;
#endif
bool emu_this(const PassGeom &p, const TileArgs &a, const R2cFuseArgs &f) {
#define PASS_EMU(LR_, LC_, LP_)                                                   \
    if constexpr (r2c_shape_fits(LR_, LC_, LP_, sizeof(TT))) {                    \
        if (p.lr == LR_ && p.lc == LC_ && p.lp == LP_) {                          \
            emulate_r2c_last_pass<TT, LR_, LC_, LP_, plane_seq_v<TT, LP_>>(a, f); \
            return true;                                                          \
        }                                                                         \
    }
    PHAST_TILE_SHAPES(PASS_EMU)
#undef PASS_EMU
    return false;
}
// a real transform of 2^(L + 1) points: the inner 2^L-point transform's passes, the last one with the untangle in it
void r2c_shape(int lr, int lc, int lp) {
    unsigned L = 0;
    PlanSpec spec;
    size_t pos = 0;
    set_case("%s r2c %dx%d p%d", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp);
    if (!find_plan<TT>(lr, lc, lp, 2, L, spec, pos, [](const std::vector<PassGeom> &g, size_t i) { return g[i].pre_tw && g[i].log_s_in >= g[i].lc + 1; })) {
        fail("r2c_last_pass_kernel", "no plan of enumerate_plans up to 2^24 points has this pass last");
        return;
    }
    const unsigned log_n = L + 1, nb = tw3_bits_for(log_n);
    std::printf("  %s %4d x %-3d p%-2d fused: pass %zu of plan %s, 2^%u real points\n", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp, pos,
                spec_to_string(spec).c_str(), log_n);
    const std::vector<cx_t<TT>> tw3n = host_tw3<TT>(log_n, nb);
    std::vector<cx_t<TT>> twu((size_t)1 << lr);
    for (size_t k = 0; k < twu.size(); ++k) twu[k] = twiddle_t<TT>(k, 2ull << lr);
    for (size_t batch : {(size_t)1, (size_t)3}) {
        Plan<TT> pl(L, spec, batch, 1, 1);
        if (!pl.ok || !pl.run_before(pos)) {
            fail("r2c_last_pass_kernel", "the plan %s could not be set up", spec_to_string(spec).c_str());
            return;
        }
        const State<TT> before = pl.st;
        const TileArgs ta = pl.args(pos);
        const PassGeom &p = pl.ps[pos];
        R2cFuseArgs fa{};  // as Planner::exec_in
        fa.tw3n = tw3n.data();
        fa.twn_bits = nb;
        fa.twu = twu.data();
        fa.tiles_per_xform = (1u << (p.log_s_in - p.lc - 1)) + 1u;
        fa.tiles_total = (unsigned)(batch * fa.tiles_per_xform);
        fa.pair_tiles = (unsigned)(batch * (fa.tiles_per_xform - 1u));
        if (!emu_this(p, ta, fa)) {
            fail("emulate_r2c_last_pass", "no emulator for this shape");
            return;
        }
        const State<TT> want = pl.st;
        const unsigned grids[3] = {own_grid(fa.tiles_total, true), 1u, 3u};
        for (int ord = 0; ord < 2; ++ord)
            for (unsigned grid : grids) {
                pl.st = before;
                set_order(ord);
                set_case("%s r2c %dx%d p%d plan %s (2^%u real) batch %zu tiles %u grid=%u %s", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp,
                         spec_to_string(spec).c_str(), log_n, batch, fa.tiles_total, grid, order_name());
                if (launch_r2c_last<TT>(lr, lc, lp, grid, nullptr, pl.args(pos), fa, false, nullptr) != hipSuccess) {
                    fail("r2c_last_pass_kernel", "the launcher refused the pass");
                    continue;
                }
                note_loop(grid, fa.tiles_total);
                compare(pl.st, want, true, pl);
            }
    }
}
int run_part(const char *only) {
    std::vector<std::string> must;
    char key[160];
#define PASS_RUN(LR_, LC_, LP_)                                                                                        \
    if (r2c_shape_ok(LR_, LC_, LP_, sizeof(TT)) && shape_wanted(only, LR_, LC_, LP_)) {                                \
        r2c_shape(LR_, LC_, LP_);                                                                                      \
        std::snprintf(key, sizeof key, "[T = %s, LR = %d, LC = %d, LP = %d, SEQ = ", Fp<TT>::type(), LR_, LC_, LP_); \
        must.push_back(key);                                                                                           \
    }
    PHAST_TILE_SHAPES(PASS_RUN)
#undef PASS_RUN
    if (must.empty()) fail("r2c_last_pass_kernel", "no shape %s", only);
    return finish("launch_r2c_last_inst", must, false, true, false);
}
}  // namespace
#if PASS_PART == 7
int pass_tile_f64_r2c(const char *only) { return run_part(only); }
#else
int pass_tile_f32_r2c(const char *only) { return run_part(only); }
#endif
#endif

// ============================================================================================================ c2r_first_pass_kernel
#if PASS_PART == 9 || PASS_PART == 10
namespace {
#if PASS_PART == 9
using TT = double;
#else
using TT = float;
#endif
bool emu_this(const PassGeom &p, const TileArgs &a, const C2rFuseArgs &f) {
#define PASS_EMU(LR_, LC_, LP_)                                                    \
    if constexpr (c2r_shape_fits(LR_, LC_, LP_, sizeof(TT))) {                     \
        if (p.lr == LR_ && p.lc == LC_ && p.lp == LP_) {                           \
            emulate_c2r_first_pass<TT, LR_, LC_, LP_, plane_seq_v<TT, LP_>>(a, f); \
            return true;                                                           \
        }                                                                          \
    }
    PHAST_TILE_SHAPES(PASS_EMU)
    if constexpr (sizeof(TT) == 4) {
        PHAST_TILE_SHAPES_F32(PASS_EMU)
    }
#undef PASS_EMU
    return false;
}
// an inverse real transform of 2^(L + 1) points: the first pass of the inner transform forms z from the half-spectrum on load
void c2r_shape(int lr, int lc, int lp) {
    unsigned L = 0;
    PlanSpec spec;
    size_t pos = 0;
    set_case("%s c2r %dx%d p%d", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp);
    if (!find_plan<TT>(lr, lc, lp, 0, L, spec, pos, [](const std::vector<PassGeom> &g, size_t i) { return g.size() >= 2 && g[i].log_s_in >= g[i].lc + 1; })) {
        fail("c2r_first_pass_kernel", "no plan of enumerate_plans up to 2^24 points has this pass first");
        return;
    }
    const unsigned log_n = L + 1, nb = tw3_bits_for(log_n);
    std::printf("  %s %4d x %-3d p%-2d fused: pass %zu of plan %s, 2^%u real points\n", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp, pos,
                spec_to_string(spec).c_str(), log_n);
    const std::vector<cx_t<TT>> tw3n = host_tw3<TT>(log_n, nb);
    std::vector<cx_t<TT>> twu((size_t)1 << lr);
    for (size_t k = 0; k < twu.size(); ++k) twu[k] = twiddle_t<TT>(k, 2ull << lr);
    for (size_t batch : {(size_t)1, (size_t)3}) {
        Plan<TT> pl(L, spec, batch, 2, 0);
        if (!pl.ok) {
            fail("c2r_first_pass_kernel", "the plan %s could not be set up", spec_to_string(spec).c_str());
            return;
        }
        const State<TT> before = pl.st;
        const TileArgs ta = pl.args(0);
        C2rFuseArgs fa{};
        fa.tw3n = tw3n.data();
        fa.twn_bits = nb;
        fa.twu = twu.data();
        if (!emu_this(pl.ps[0], ta, fa)) {
            fail("emulate_c2r_first_pass", "no emulator for this shape");
            return;
        }
        const State<TT> want = pl.st;
        const unsigned grids[3] = {own_grid(ta.tiles_total), 1u, 3u};
        for (int ord = 0; ord < 2; ++ord)
            for (unsigned grid : grids) {
                pl.st = before;
                set_order(ord);
                set_case("%s c2r %dx%d p%d plan %s (2^%u real) batch %zu tiles %u grid=%u %s", Fp<TT>::name(), 1 << lr, 1 << lc, 1 << lp,
                         spec_to_string(spec).c_str(), log_n, batch, ta.tiles_total, grid, order_name());
                if (launch_c2r_first<TT>(lr, lc, lp, grid, nullptr, pl.args(0), fa, false, nullptr) != hipSuccess) {
                    fail("c2r_first_pass_kernel", "the launcher refused the pass");
                    continue;
                }
                note_loop(grid, ta.tiles_total);
                compare(pl.st, want, false, pl);
            }
    }
}
int run_part(const char *only) {
    std::vector<std::string> must;
    char key[160];
#define PASS_RUN(LR_, LC_, LP_)                                                                                        \
    if (c2r_shape_ok(LR_, LC_, LP_, sizeof(TT)) && shape_wanted(only, LR_, LC_, LP_)) {                                \
        c2r_shape(LR_, LC_, LP_);                                                                                      \
        std::snprintf(key, sizeof key, "[T = %s, LR = %d, LC = %d, LP = %d, SEQ = ", Fp<TT>::type(), LR_, LC_, LP_); \
        must.push_back(key);                                                                                           \
    }
    PHAST_TILE_SHAPES(PASS_RUN)
    if constexpr (sizeof(TT) == 4) {
        PHAST_TILE_SHAPES_F32(PASS_RUN)
    }
#undef PASS_RUN
    if (must.empty()) fail("c2r_first_pass_kernel", "no shape %s", only);
    return finish("launch_c2r_first_inst", must, false, true, false);
}
}  // namespace
#if PASS_PART == 9
int pass_tile_f64_c2r(const char *only) { return run_part(only); }
#else
int pass_tile_f32_c2r(const char *only) { return run_part(only); }
#endif
#endif

// ============================================================================================================ wave_fft_kernel
#if PASS_PART == 11 || PASS_PART == 12
namespace {
#if PASS_PART == 11
using TT = double;
#else
using TT = float;
#endif
// the 64 x 64 plan on wave tiles, three transforms; tiles_total cut to 1, to WAVES and to 2 WAVES + 1 tiles (the trailing waves of
// the last workgroup return at once), and whole.  The stagger is the launcher's: PHAST_WAVE_STAGGER=0,0 in the environment
// (tests/test_pass_emulator.py runs the part both ways) makes it 0.
int run_part(const char *) {
    constexpr unsigned WAVES = (unsigned)WaveBody<TT, false, true>::WAVES;
    const unsigned L = 12, tl = sizeof(TT) == 8 ? 10u : 11u;
    PlanSpec spec;
    spec.np = 2;
    spec.lr[0] = spec.lr[1] = 6;
    spec.tl[0] = spec.tl[1] = tl;
    spec.lp = 4 | kWaveTiles;
    bool listed = false;
    for (const PlanSpec &s : plans_of<TT>(L)) listed |= s == spec;
    set_case("%s wave", Fp<TT>::name());
    if (!listed) fail("wave_fft_kernel", "enumerate_plans no longer lists %s", spec_to_string(spec).c_str());
    std::printf("  stagger setting %#x\n", wave_stagger_setting());
    // ... and eight transforms, whole: the workgroup count is a multiple of 8 (locate's remap for XCD affinity) with several
    // transforms behind it -- what a composite planner's engine gives the kernel (tests/test_gpu_engine_batches.py)
    for (size_t run = 0; run < 4; ++run) {
        const size_t pos = run & 1;
        const bool eight = run >= 2;
        Plan<TT> pl(L, spec, eight ? 8 : 3);
        if (!pl.ok || !pl.ps[pos].wave || !pl.run_before(pos)) {
            fail("wave_fft_kernel", "the plan %s could not be set up", spec_to_string(spec).c_str());
            continue;
        }
        const State<TT> before = pl.st;
        const unsigned all = pl.args(pos).tiles_total;
        if (eight && (all % (8 * WAVES) || all / WAVES < 8)) fail("wave_fft_kernel", "eight transforms: %u tiles are no multiple of 8 workgroups", all);
        for (unsigned tiles : {1u, WAVES, 2 * WAVES + 1, all}) {
            if (eight && tiles != all) continue;
            if (tiles > all) {
                fail("wave_fft_kernel", "%u tiles wanted, the batch has %u", tiles, all);
                continue;
            }
            pl.st = before;
            TileArgs ta = pl.args(pos);
            ta.tiles_total = tiles;
            if (pos == 0) emulate_wave_pass<TT, false, true>(ta);
            else emulate_wave_pass<TT, true, false>(ta);
            const State<TT> want = pl.st;
            for (int ord = 0; ord < 2; ++ord) {
                pl.st = before;
                set_order(ord);
                set_case("%s wave %s plan %s tiles_total %u of %u %s", Fp<TT>::name(), pos ? "PRE_TW" : "TRANSPOSE", spec_to_string(spec).c_str(), tiles,
                         all, order_name());
                const hipError_t e = sizeof(TT) == 8 ? launch_wave_f64(pos == 0, nullptr, ta, false, nullptr, nullptr)
                                                     : launch_wave_f32(pos == 0, nullptr, ta, false, nullptr, nullptr);
                if (e != hipSuccess) {
                    fail("wave_fft_kernel", "the launcher refused the pass");
                    continue;
                }
                if (tiles % WAVES) g_br.early_waves = true;
                compare(pl.st, want, false, pl);
            }
        }
    }
    char k0[96], k1[96];
    std::snprintf(k0, sizeof k0, "[T = %s, PRE_TW = false, TRANSPOSE = true]", Fp<TT>::type());
    std::snprintf(k1, sizeof k1, "[T = %s, PRE_TW = true, TRANSPOSE = false]", Fp<TT>::type());
    return finish("launch_wave_inst", {k0, k1}, false, false, true);
}
}  // namespace
#if PASS_PART == 11
int pass_wave_f64(const char *only) { return run_part(only); }
#else
int pass_wave_f32(const char *only) { return run_part(only); }
#endif
#endif

// ============================================================================================================ quad_fft_kernel
#if PASS_PART == 13 || PASS_PART == 14
namespace {
#if PASS_PART == 13
using TT = double;
#else
using TT = float;
#endif
// the shortest plan with a four-wave pass: 64 x 256 on wave tiles and the 256-row kernel; grid = tiles is the ONE instantiation
int run_part(const char *) {
    const unsigned L = 14;
    PlanSpec spec;
    spec.np = 2;
    spec.lr[0] = 6;
    spec.lr[1] = 8;
    spec.tl[0] = sizeof(TT) == 8 ? 10u : 11u;
    spec.tl[1] = sizeof(TT) == 8 ? 12u : 13u;
    spec.lp = 4 | kWaveTiles;
    bool listed = false;
    for (const PlanSpec &s : plans_of<TT>(L)) listed |= s == spec;
    set_case("%s quad", Fp<TT>::name());
    if (!listed) fail("quad_fft_kernel", "enumerate_plans no longer lists %s", spec_to_string(spec).c_str());
    // (eight transforms: a tile count that is a multiple of 8 -- locate's remap for XCD affinity -- with several transforms in it,
    //  as a composite planner's engine runs the pass: tests/test_gpu_engine_batches.py)
    for (size_t batch : {(size_t)1, (size_t)3, (size_t)8}) {
        Plan<TT> pl(L, spec, batch);
        if (!pl.ok || !pl.ps[1].quad || !pl.run_before(1)) {
            fail("quad_fft_kernel", "the plan %s could not be set up", spec_to_string(spec).c_str());
            continue;
        }
        const State<TT> before = pl.st;
        const TileArgs ta = pl.args(1);
        emulate_quad_pass<TT>(ta);
        const State<TT> want = pl.st;
        const unsigned grids[3] = {own_grid(ta.tiles_total), 1u, 3u};
        for (int ord = 0; ord < 2; ++ord)
            for (unsigned grid : grids) {
                pl.st = before;
                set_order(ord);
                set_case("%s quad plan %s batch %zu tiles %u grid=%u (%s) %s", Fp<TT>::name(), spec_to_string(spec).c_str(), batch, ta.tiles_total, grid,
                         grid == ta.tiles_total ? "ONE" : "looped", order_name());
                const hipError_t e = sizeof(TT) == 8 ? launch_quad_f64(grid, nullptr, pl.args(1), false, nullptr, nullptr)
                                                     : launch_quad_f32(grid, nullptr, pl.args(1), false, nullptr, nullptr);
                if (e != hipSuccess) {
                    fail("quad_fft_kernel", "the launcher refused the pass");
                    continue;
                }
                if (grid != ta.tiles_total) note_loop(grid, ta.tiles_total);
                compare(pl.st, want, true, pl);
            }
    }
    // launch_quad_inst launches through a function pointer variable: the shim names the first function it held (ONE: the grid of
    // one workgroup per tile comes first above) by the launcher alone and marks the second (the looped kernel) with #1
    char k0[96], k1[96];
    std::snprintf(k0, sizeof k0, "kern in hipError_t phast::launch_quad_inst");
    std::snprintf(k1, sizeof k1, "kern#1 in hipError_t phast::launch_quad_inst");
    return finish("launch_quad_inst", {k0, k1}, false, true, false);
}
}  // namespace
#if PASS_PART == 13
int pass_quad_f64(const char *only) { return run_part(only); }
#else
int pass_quad_f32(const char *only) { return run_part(only); }
#endif
#endif

// ============================================================================================================ row_fft_kernel
#if PASS_PART == 15
namespace {
template <typename T> bool emu_row(unsigned log_n, const RowArgs &r) {
    if (log_n == 5 && r.real_mode) {  // as launch_small_fft
        emulate_row_fft<T, 5, 7, kRealRow5LP>(r);
        return true;
    }
#define PASS_EMU(LR_, LC_, LP_)               \
    if (log_n == LR_) {                       \
        emulate_row_fft<T, LR_, LC_, LP_>(r); \
        return true;                          \
    }
    PHAST_ROW_SHAPES(PASS_EMU)
#undef PASS_EMU
    return false;
}
// mode 0: planar complex in and out; 1: R2C (n (even, odd) pairs in, planar n + 1 out); 2: C2R (planar n + 1 in, n (im, re) pairs out)
template <typename T> void row_case(unsigned log_n, unsigned mode, size_t batch, unsigned forced) {
    const size_t n = (size_t)1 << log_n;
    const size_t in_n = mode == 2 ? n + 1 : n, out_n = mode == 1 ? n + 1 : n;
    const size_t in_dist = batch == 1 ? in_n : in_n + 3, out_dist = batch == 1 ? out_n : out_n + 2;
    std::vector<T> in_re(((batch - 1) * in_dist + in_n) * (mode == 1 ? 2 : 1)), in_im(mode == 1 ? 0 : in_re.size());
    std::vector<T> out_re(((batch - 1) * out_dist + out_n) * (mode == 2 ? 2 : 1)), out_im(mode == 2 ? 0 : out_re.size());
    fill_pm1(in_re, 3);
    fill_pm1(in_im, 4);
    const std::vector<cx_t<T>> tw = host_twr<T>(1u << log_n);
    const unsigned rbits = tw3_bits_for(log_n + 1);
    const std::vector<cx_t<T>> rtw = host_tw3<T>(log_n + 1, rbits);
    SmallArgs sa{};
    sa.in_re = in_re.data();
    sa.in_im = mode == 1 ? nullptr : in_im.data();
    sa.out_re = out_re.data();
    sa.out_im = mode == 2 ? nullptr : out_im.data();
    sa.tw = tw.data();
    sa.in_dist = in_dist;
    sa.out_dist = out_dist;
    sa.log_n = log_n;
    sa.batch = (unsigned)batch;
    sa.in_interleaved = mode == 1 ? 1 : 0;
    sa.out_interleaved = mode == 2 ? 2 : 0;
    sa.scale = mode == 2 ? 1.0 / (double)n : 1.0;
    sa.real_mode = mode;
    sa.rtw_bits = mode ? rbits : 0;
    sa.rtw3 = mode ? rtw.data() : nullptr;
    RowArgs r{};  // as launch_small_fft fills it
    r.in_re = sa.in_re;
    r.in_im = sa.in_im;
    r.out_re = sa.out_re;
    r.out_im = sa.out_im;
    r.twr = sa.tw;
    r.in_dist = sa.in_dist;
    r.out_dist = sa.out_dist;
    r.batch = sa.batch;
    r.in_interleaved = sa.in_interleaved;
    r.out_interleaved = sa.out_interleaved;
    r.scale = sa.scale;
    r.real_mode = sa.real_mode;
    r.rtw_bits = sa.rtw_bits;
    r.rtw3 = sa.rtw3;
    const unsigned lc = row_tile_cols_log(log_n);
    r.tiles_total = (unsigned)((batch + ((1ull << lc) - 1)) >> lc);
    fill_sentinel(out_re);
    fill_sentinel(out_im);
    set_case("%s row 2^%u mode %u batch %zu", Fp<T>::name(), log_n, mode, batch);
    if (!emu_row<T>(log_n, r)) {
        fail("emulate_row_fft", "no emulator for this length");
        return;
    }
    const std::vector<T> want_re = out_re, want_im = out_im;
    for (int ord = 0; ord < 2; ++ord) {
        fill_sentinel(out_re);
        fill_sentinel(out_im);
        set_order(ord);
        set_case("%s row 2^%u mode %u batch %zu tiles %u grid=%u %s", Fp<T>::name(), log_n, mode, batch, r.tiles_total, forced ? forced : r.tiles_total,
                 order_name());
        block_shim::force_grid = forced;  // the launcher sizes the grid itself: one workgroup per tile at these sizes
        const hipError_t e = launch_small_fft<T>(sa, nullptr);
        block_shim::force_grid = 0;
        if (e != hipSuccess) {
            fail("row_fft_kernel", "the launcher refused the transform");
            continue;
        }
        note_loop(forced ? forced : r.tiles_total, r.tiles_total);
        long long at = first_diff(out_re, want_re);
        if (at >= 0) fail(block_shim::last_kernel, "out re[%lld]: the kernel gives bits %llx, the emulator %llx", at, bits_of(out_re[(size_t)at]), bits_of(want_re[(size_t)at]));
        at = first_diff(out_im, want_im);
        if (at >= 0) fail(block_shim::last_kernel, "out im[%lld]: the kernel gives bits %llx, the emulator %llx", at, bits_of(out_im[(size_t)at]), bits_of(want_im[(size_t)at]));
        const size_t w = mode == 2 ? 2 : 1;
        for (size_t b = 0; b + 1 < batch; ++b)
            for (size_t i = (b * out_dist + out_n) * w; i < (b + 1) * out_dist * w; ++i)
                if (bits_of(out_re[i]) != (u64)Fp<T>::sentinel) fail(block_shim::last_kernel, "the gap element %zu of the output was written", i);
    }
}
// a single point: a scaled copy
template <typename T> void one_point() {
    const size_t batch = 300;
    std::vector<T> in_re(batch), in_im(batch), out_re(batch), out_im(batch);
    fill_pm1(in_re, 5);
    fill_pm1(in_im, 6);
    SmallArgs sa{};
    sa.in_re = in_re.data();
    sa.in_im = in_im.data();
    sa.out_re = out_re.data();
    sa.out_im = out_im.data();
    sa.in_dist = sa.out_dist = 1;
    sa.batch = (unsigned)batch;
    sa.scale = 0.5;
    for (int ord = 0; ord < 2; ++ord) {
        fill_sentinel(out_re);
        fill_sentinel(out_im);
        set_order(ord);
        set_case("%s one point %s", Fp<T>::name(), order_name());
        if (launch_small_fft<T>(sa, nullptr) != hipSuccess) fail("one_point_kernel", "the launcher refused");
        for (size_t i = 0; i < batch; ++i)
            if (bits_of(out_re[i]) != bits_of(in_re[i] * (T)0.5) || bits_of(out_im[i]) != bits_of(in_im[i] * (T)0.5)) {
                fail(block_shim::last_kernel, "element %zu is not the scaled input", i);
                break;
            }
    }
}
template <typename T> void rows_of(std::vector<std::string> &must) {
    char key[160];
    one_point<T>();
    std::snprintf(key, sizeof key, "one_point_kernel<%s>", Fp<T>::type());
    must.push_back(key);
#define PASS_RUN(LR_, LC_, LP_)                                                                                                       \
    for (unsigned mode = 0; mode < 3; ++mode) {                                                                                       \
        const size_t tile = (size_t)1 << ((LR_ == 5 && mode) ? 7 : LC_);                                                              \
        row_case<T>(LR_, mode, 1, 0);                                                                                                 \
        if (tile > 2) row_case<T>(LR_, mode, tile - 1, 0);                                                                            \
        row_case<T>(LR_, mode, 2 * tile + 1, 0);                                                                                      \
        row_case<T>(LR_, mode, 2 * tile + 1, 1); /* the persistent loop: one workgroup walks the three tiles */                        \
        row_case<T>(LR_, mode, 2 * tile + 1, 2);                                                                                      \
        std::snprintf(key, sizeof key, "[T = %s, LR = %d, LC = %d, LP = %d, REAL = %s]", Fp<T>::type(), LR_, (LR_ == 5 && mode) ? 7 : LC_, \
                      (LR_ == 5 && mode) ? kRealRow5LP : LP_, mode ? "true" : "false");                                               \
        must.push_back(key);                                                                                                          \
    }
    PHAST_ROW_SHAPES(PASS_RUN)
#undef PASS_RUN
}
}  // namespace
int pass_small_fft(const char *only) {
    std::vector<std::string> must;
    if (!*only || !std::strcmp(only, "f64")) rows_of<double>(must);
    if (!*only || !std::strcmp(only, "f32")) rows_of<float>(must);
    return finish("launch_row_inst", must, false, true, false);
}
#endif
#endif  // not an instantiation-only part
#endif
