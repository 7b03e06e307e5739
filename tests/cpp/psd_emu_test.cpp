// psd_emu_test.cpp -- the sweeps of Welch spectral estimation (csrc/psd.hip, #included as it stands), run on the host under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_psd_emulator.py builds and runs it; tests/emu/block_shim.hpp
// runs a workgroup as fibers that meet at __syncthreads(): the mean sweep reduces through LDS).  A stand-alone program: no
// GPU, no HIP runtime.
//
// All kernels are driven through launch_psd with arguments built as PsdPlanner::run builds them, per chunk: whole
// (workspace_len(batch, cross)) and in chunks of one frame (workspace_min(cross)), aligned and one element off, on heap
// blocks of exactly the contract's elements (one element too far is an AddressSanitizer report).  Signals and the stand-ins
// for the spectra hold small integers and the window is all ones, so every value is exact in float and in double and is
// compared bit for bit:
//     mean    against the exact sum of the differences, divided by P as the kernel divides; in both thread orders
//     frame   against ((x - x[f H]) - mean) with the mean the workspace holds; the row's padding must be exactly +0
//     accum   the partial rows against the running sums of the definition, chunk after chunk
//     final   against the partial rows the workspace holds, in ascending slab order, times scale c_k
//     point   against the definition
// so that a wrong kernel is blamed alone.  The real transform between the frame sweep and the spectra is the engine's own
// (tests/cpp/pass_emu_test.cpp, tests/cpp/sweep_emu_test.cpp): here integer planes stand in for its output, with NaN in the
// rows' padding, which must not reach an output.  Outputs and the workspace start as a NaN bit pattern: an element the contract
// names must have lost it, every other one (lead-ins, the stand-in for the real planner's workspace) must have kept its bits.
#include <hip/hip_runtime.h>

#include "block_shim.hpp"

#include <cmath>
// any_len.hpp's chirp() (on psd.hpp's include path, never called by these kernels) names the device's sincospi: a host
// overload so that the header compiles here
inline void sincospi(double t, double *s, double *c) {
    *s = std::sin(3.141592653589793238462643383279502884 * t);
    *c = std::cos(3.141592653589793238462643383279502884 * t);
}

#include "psd.hip"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sanitizer_exit.hpp"

using namespace phast;

namespace {

using ld = long double;
using u64 = unsigned long long;

template <typename T> struct Fp;
template <> struct Fp<double> {
    using bits = unsigned long long;
    static constexpr bits sentinel = 0x7ff8dead5eed0001ull;  // a quiet NaN no kernel produces
    static constexpr size_t V = 2;
    static const char *name() { return "f64"; }
};
template <> struct Fp<float> {
    using bits = unsigned;
    static constexpr bits sentinel = 0x7fc5eed1u;
    static constexpr size_t V = 4;
    static const char *name() { return "f32"; }
};

int g_fails = 0;
u64 g_compared = 0;
char g_case[320] = "";

void set_case(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}
void fail(const char *kernel, const char *fmt, ...) {
    if (++g_fails > 12) return;
    std::printf("FAIL %s [%s]: ", kernel, g_case);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}

// an allocation of exactly n elements of T behind `off` elements of lead-in (off = 1: an element-aligned pointer)
template <typename T> struct Buf {
    using bits = typename Fp<T>::bits;
    T *base = nullptr, *p = nullptr;
    size_t n, off;
    Buf(size_t n_, size_t off_ = 0) : n(n_), off(off_) {
        void *q = nullptr;
        const size_t bytes = (n + off) * sizeof(T);
        if (posix_memalign(&q, 16, bytes ? bytes : 1)) std::abort();
        base = (T *)q;
        p = base + off;
        for (size_t i = 0; i < n + off; ++i) std::memcpy(base + i, &Fp<T>::sentinel, sizeof(T));
    }
    ~Buf() { std::free(base); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    bool is_sentinel(long long i) const {  // i >= -off
        bits b;
        std::memcpy(&b, p + i, sizeof(T));
        return b == Fp<T>::sentinel;
    }
};
template <typename T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

u64 mix(u64 seed, u64 i) {
    u64 x = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
int small_int(u64 seed, u64 i, int amp) {  // in [-amp, amp], never 0: a zero fill cannot pass for data
    const int v = (int)(mix(seed, i) % (unsigned)(2 * amp)) - amp;
    return v >= 0 ? v + 1 : v;
}

// the geometry of PsdPlanner<T> for (L, P, H, F); `rw` elements per row stand in for the real planner's workspace
template <typename T> struct Plan {
    static constexpr size_t V = Fp<T>::V, D = sizeof(double) / sizeof(T);
    size_t len, p, h, f, frames, bins, fd, bd, q, slabs, rw;
    Plan(size_t len_, size_t p_, size_t h_, size_t f_)
        : len(len_), p(p_), h(h_), f(f_), frames((size_t)psd_segments(len_, p_, h_)), bins((size_t)psd_bins(f_)),
          fd((f_ + V - 1) / V * V), bd((bins + V - 1) / V * V), q((size_t)psd_slab_len(frames, bins)),
          slabs((size_t)psd_slabs(frames, q)), rw((f_ & (f_ - 1)) ? 2 * V : 0) {}
    size_t per() const { return fd + 2 * bd + rw; }
    size_t slots_of(size_t c, size_t batch) const {
        const size_t s = 1 + (c + frames - 2) / frames;
        return s < batch ? s : batch;
    }
    size_t need(size_t c, size_t slots, bool cross) const {
        const size_t x = cross ? 2 : 1;
        return x * c * per() + (x * c + 1) / 2 * 2 * D + slots * (cross ? 4 : 1) * slabs * bd * D + (V - 1);
    }
    size_t chunk_of(T *d_work, size_t work_len, size_t batch, bool cross, T **w) const {
        const size_t skip = ((16 - (reinterpret_cast<uintptr_t>(d_work) & 15u)) & 15u) / sizeof(T);
        *w = d_work + skip;
        const size_t avail = work_len - skip + (V - 1), total = batch * frames;
        size_t lo = 1, hi = total;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (need(mid, slots_of(mid, batch), cross) <= avail) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }
};

struct Opt {
    size_t batch, off;
    int chunked;  // 0: all frames in one chunk; 1: chunks of one frame; 2: chunks of two (the last one may hold one)
    bool cross, detrend, average, autos;
};

template <typename T> void run_case(size_t len, size_t p, size_t h, size_t f, const Opt &o) {
    constexpr size_t V = Fp<T>::V;
    set_case("%s L=%zu P=%zu H=%zu F=%zu batch=%zu off=%zu %s %s detrend=%d average=%d autos=%d", Fp<T>::name(), len, p, h, f, o.batch,
             o.off, o.chunked == 0 ? "whole" : o.chunked == 1 ? "chunks of 1" : "chunks of 2", o.cross ? "cross" : "auto", (int)o.detrend, (int)o.average, (int)o.autos);
    if (psd_bad_args(len, p, h, f, o.detrend, kPsdDensity, 2.5, (unsigned)V)) {
        fail("psd_bad_args", "rejects a shape of the table");
        return;
    }
    const Plan<T> pl(len, p, h, f);
    const size_t frames = pl.frames, bins = pl.bins, fd = pl.fd, bd = pl.bd, total = o.batch * frames, nx = o.cross ? 2 : 1;
    const int planes = o.cross ? 4 : 1;
    std::vector<double> ones(p, 1.0);
    double sigma = 0;
    if (psd_sigma(ones.data(), p, kPsdDensity, 2.5, &sigma)) fail("psd_sigma", "rejects a window of ones");
    Buf<double> win(fd);
    for (size_t j = 0; j < fd; ++j) win.p[j] = j < p ? 1.0 : 0.0;
    const size_t sd = o.batch == 1 ? len : len + 3;
    Buf<T> x((o.batch - 1) * sd + len, o.off), y((o.batch - 1) * sd + len, o.off);
    auto xv = [&](int which, size_t b, size_t i) { return (T)small_int(7 * p + 31 * which + b, i, 8); };
    for (size_t b = 0; b < o.batch; ++b)
        for (size_t i = 0; i < len; ++i) {
            x.p[b * sd + i] = xv(0, b, i);
            y.p[b * sd + i] = xv(1, b, i);
        }
    // the stand-in spectra: bin k of the flattened frame q of x (which = 0) or y (1)
    auto zr = [&](int which, size_t q, size_t k) { return (double)small_int(11 * f + which, q * bins + k, 6); };
    auto zi = [&](int which, size_t q, size_t k) { return (double)small_int(13 * f + which, q * bins + k, 6); };
    auto term = [&](int plane, size_t q, size_t k) {
        const double ar = zr(0, q, k), ai = zi(0, q, k), br = zr(1, q, k), bi = zi(1, q, k);
        if (!o.cross || plane == 2) return ar * ar + ai * ai;
        return plane == 0 ? ar * br + ai * bi : plane == 1 ? ar * bi - ai * br : br * br + bi * bi;
    };
    const size_t pts = o.average ? bins : frames * bins;
    Buf<T> out0(o.batch * pts, o.off), out1(o.batch * pts, o.off), out2(o.batch * pts, o.off), out3(o.batch * pts, o.off);
    Buf<T> *outs[4] = {&out0, &out1, &out2, &out3};
    T *outp[4] = {out0.p, o.cross ? out1.p : nullptr, o.cross && o.autos ? out2.p : nullptr, o.cross && o.autos ? out3.p : nullptr};
    const size_t want_chunk = o.chunked == 0 || (size_t)o.chunked > total ? total : (size_t)o.chunked;
    const size_t work_len = pl.need(want_chunk, pl.slots_of(want_chunk, o.batch), o.cross);
    Buf<T> work(work_len, o.off);
    T *w = nullptr;
    const size_t chunk = pl.chunk_of(work.p, work_len, o.batch, o.cross, &w);
    if (chunk != want_chunk) fail("chunk_of", "a chunk of %zu frames in a workspace of %zu elements", chunk, work_len);
    const size_t slots = pl.slots_of(chunk, o.batch);
    std::vector<double> expect(o.batch * planes * pl.slabs * bins, 0.0);  // the running sums of the definition
    auto ex = [&](size_t b, int plane, size_t slab) { return expect.data() + ((b * planes + plane) * pl.slabs + slab) * bins; };

    for (size_t q0 = 0; q0 < total; q0 += chunk) {
        const size_t c = total - q0 < chunk ? total - q0 : chunk, nr = nx * c, cap = nx * chunk;
        T *rows = w, *re = rows + cap * fd, *im = re + cap * bd, *iw = im + cap * bd;
        double *mean = reinterpret_cast<double *>(iw + cap * pl.rw), *acc = mean + (cap + 1) / 2 * 2;
        PsdArgs a{};  // PsdPlanner::args and ::run
        a.win = win.p;
        a.p = p;
        a.h = h;
        a.frames = frames;
        a.fd = fd;
        a.bd = bd;
        a.bins = bins;
        a.nfft = f;
        a.q = pl.q;
        a.slabs = pl.slabs;
        a.tpr = psd_mean_threads(p);
        a.planes = planes;
        a.x = x.p;
        a.y = o.cross ? y.p : nullptr;
        a.sig_dist = sd;
        a.rows = rows;
        a.re = re;
        a.im = im;
        a.acc = acc;
        a.slots = slots;
        a.q0 = q0;
        a.c = c;
        for (int i = 0; i < planes; ++i) a.out[i] = outp[i];
        auto seg = [&](size_t r) {  // the first sample of row r's segment
            const size_t qq = q0 + (r >= c ? r - c : r), b = qq / frames, fr = qq % frames;
            return (r >= c ? y.p : x.p) + b * sd + fr * h;
        };
        if (o.detrend) {
            a.mean = mean;
            a.groups = nr * a.tpr;
            for (int order = 0; order < 2; ++order) {
                block_shim::order = order ? block_shim::kDescending : block_shim::kAscending;
                for (size_t r = 0; r < nr; ++r) std::memset(mean + r, 0xff, sizeof(double));
                if (launch_psd<T>(kPsdMean, a, nullptr) != hipSuccess) fail("psd_mean_kernel", "the launcher failed");
                for (size_t r = 0; r < nr; ++r) {
                    const T *s = seg(r);
                    double sum = 0;  // exact: small integers
                    for (size_t j = 0; j < p; ++j) sum += (double)s[j] - (double)s[0];
                    ++g_compared;
                    if (!same_bits(mean[r], sum / (double)p))
                        fail("psd_mean_kernel", "mean of row %zu = %.17g, must be exactly %.17g (thread order %d)", r, mean[r], sum / (double)p, order);
                }
            }
            block_shim::order = block_shim::kAscending;
        }
        a.gpt = (unsigned)(fd / V);
        a.groups = nr * a.gpt;
        if (launch_psd<T>(kPsdFrame, a, nullptr) != hipSuccess) fail("psd_frame_kernel", "the launcher failed");
        for (size_t r = 0; r < nr; ++r) {
            const T *s = seg(r);
            for (size_t j = 0; j < fd; ++j) {
                const T got = rows[r * fd + j];
                ++g_compared;
                if (j >= p) {
                    if (!same_bits(got, T(0))) fail("psd_frame_kernel", "row %zu padding element %zu = %.9Lg, must be exactly +0", r, j, (ld)got);
                    continue;
                }
                const T want = o.detrend ? (T)((((double)s[j] - (double)s[0]) - mean[r]) * 1.0) : (T)((double)s[j] * 1.0);
                if (!same_bits(got, want)) fail("psd_frame_kernel", "row %zu element %zu = %.9Lg, must be exactly %.9Lg", r, j, (ld)got, (ld)want);
            }
        }
        // the spectra: small integers, NaN in the padding of every row
        for (size_t r = 0; r < nr; ++r)
            for (size_t k = 0; k < bd; ++k) {
                const int which = r >= c ? 1 : 0;
                const size_t qq = q0 + (which ? r - c : r);
                if (k < bins) {
                    re[r * bd + k] = (T)zr(which, qq, k);
                    im[r * bd + k] = (T)zi(which, qq, k);
                } else {
                    std::memcpy(re + r * bd + k, &Fp<T>::sentinel, sizeof(T));
                    std::memcpy(im + r * bd + k, &Fp<T>::sentinel, sizeof(T));
                }
            }
        if (!o.average) {
            a.scale = sigma;
            a.count = c * bins;
            a.groups = (a.count + V - 1) / V;
            if (launch_psd<T>(kPsdPoint, a, nullptr) != hipSuccess) fail("psd_point_kernel", "the launcher failed");
            for (int i = 0; i < planes; ++i) {
                if (!outp[i]) continue;
                for (size_t r = 0; r < c; ++r)
                    for (size_t k = 0; k < bins; ++k) {
                        const T got = outp[i][(q0 + r) * bins + k], want = (T)(term(i, q0 + r, k) * (sigma * psd_onesided(k, f)));
                        ++g_compared;
                        if (!same_bits(got, want))
                            fail("psd_point_kernel", "output %d frame %zu bin %zu = %.9Lg, must be exactly %.9Lg", i, q0 + r, k, (ld)got, (ld)want);
                    }
            }
            continue;
        }
        const size_t b_lo = q0 / frames, nb = (q0 + c - 1) / frames - b_lo + 1;
        a.b0 = b_lo;
        a.s0 = 0;
        a.ns = pl.slabs;
        if (nb == 1) {
            const size_t f_lo = q0 - b_lo * frames;
            a.s0 = f_lo / pl.q;
            a.ns = (f_lo + c - 1) / pl.q - a.s0 + 1;
        }
        a.gpt = (unsigned)(bd / V);
        a.groups = nb * a.ns * a.gpt;
        if (launch_psd<T>(kPsdAccum, a, nullptr) != hipSuccess) fail("psd_accum_kernel", "the launcher failed");
        for (size_t qq = q0; qq < q0 + c; ++qq) {  // the definition: frame by frame into its slab's running sum
            const size_t b = qq / frames, slab = (qq % frames) / pl.q;
            for (int i = 0; i < planes; ++i)
                for (size_t k = 0; k < bins; ++k) ex(b, i, slab)[k] += term(i, qq, k);
        }
        for (size_t b = b_lo; b < b_lo + nb; ++b) {
            const size_t first = b * frames, lo = (q0 > first ? q0 : first) - first, hi = (q0 + c < first + frames ? q0 + c : first + frames) - first;
            for (size_t slab = lo / pl.q; slab <= (hi - 1) / pl.q; ++slab)
                for (int i = 0; i < planes; ++i) {
                    const double *row = acc + (((b % slots) * planes + i) * pl.slabs + slab) * bd;
                    for (size_t k = 0; k < bins; ++k) {
                        ++g_compared;
                        if (!same_bits(row[k], ex(b, i, slab)[k]))
                            fail("psd_accum_kernel", "partial row of signal %zu plane %d slab %zu bin %zu = %.17g, must be exactly %.17g after frame %zu",
                                 b, i, slab, k, row[k], ex(b, i, slab)[k], hi - 1);
                    }
                }
        }
        const size_t done = (q0 + c) / frames - b_lo;
        if (!done) continue;
        std::vector<double> want(done * planes * bins);  // from the partial rows the workspace holds
        for (size_t d = 0; d < done; ++d)
            for (int i = 0; i < planes; ++i)
                for (size_t k = 0; k < bins; ++k) {
                    double s = 0;
                    for (size_t slab = 0; slab < pl.slabs; ++slab) s += acc[((((b_lo + d) % slots) * planes + i) * pl.slabs + slab) * bd + k];
                    want[(d * planes + i) * bins + k] = s * (sigma / (double)frames * psd_onesided(k, f));
                    double all = 0;  // the definition: a partial row must have survived the chunks since its slab was summed
                    for (size_t slab = 0; slab < pl.slabs; ++slab) all += ex(b_lo + d, i, slab)[k];
                    ++g_compared;
                    if (!same_bits(s, all))
                        fail("psd_schedule", "the partial rows of signal %zu plane %d bin %zu sum to %.17g, the definition to %.17g", b_lo + d, i, k, s, all);
                }
        a.scale = sigma / (double)frames;
        a.count = done * bins;
        a.groups = (a.count + V - 1) / V;
        if (launch_psd<T>(kPsdFinal, a, nullptr) != hipSuccess) fail("psd_final_kernel", "the launcher failed");
        for (size_t d = 0; d < done; ++d)
            for (int i = 0; i < planes; ++i) {
                if (!outp[i]) continue;
                for (size_t k = 0; k < bins; ++k) {
                    const T got = outp[i][(b_lo + d) * bins + k], wv = (T)want[(d * planes + i) * bins + k];
                    ++g_compared;
                    if (!same_bits(got, wv))
                        fail("psd_final_kernel", "output %d signal %zu bin %zu = %.9Lg, must be exactly %.9Lg", i, b_lo + d, k, (ld)got, (ld)wv);
                }
            }
    }
    // what the contract names has been written, nothing else has
    for (int i = 0; i < 4; ++i) {
        const char *kernel = o.average ? "psd_final_kernel" : "psd_point_kernel";
        for (size_t e = 0; e < o.batch * pts; ++e)
            if (outs[i]->is_sentinel((long long)e) != (outp[i] == nullptr)) {
                fail(kernel, "element %zu of output %d was %s", e, i, outp[i] ? "not written" : "written");
                break;
            }
        for (size_t e = 1; e <= o.off; ++e)
            if (!outs[i]->is_sentinel(-(long long)e)) fail(kernel, "the element in front of output %d was written", i);
    }
    for (size_t b = 0; b < o.batch; ++b)
        for (size_t i = 0; i < len; ++i)
            if (!same_bits(x.p[b * sd + i], xv(0, b, i)) || !same_bits(y.p[b * sd + i], xv(1, b, i))) {
                fail("psd", "sample %zu of signal %zu was written", i, b);
                break;
            }
    {
        const size_t nr = nx * chunk;  // the stand-in for the real planner's workspace
        const T *iw = w + nr * (fd + 2 * bd);
        for (size_t e = 0; e < nr * pl.rw; ++e)
            if (!work.is_sentinel((long long)(iw - work.p + e))) {
                fail("psd", "the real planner's part of the workspace was written at element %zu", e);
                break;
            }
    }
    for (size_t e = 1; e <= o.off; ++e)
        if (!work.is_sentinel(-(long long)e)) fail("psd", "the element in front of the workspace was written");
}

}  // namespace

int main() {
    struct Shape {
        size_t len, p, h, f;
        bool big;
    };
    const Shape shapes[] = {{1000, 100, 63, 128, false}, {1000, 100, 100, 100, false}, {37, 37, 1, 37, false}, {513, 64, 32, 64, false},
                            {300, 7, 3, 9, false},       {64, 1, 1, 1, false},         {50, 2, 1, 2, false},   {1000, 30, 23, 30, false},
                            {120, 8, 8, 8, false},       {128, 8, 8, 8, false},        {136, 8, 8, 8, false},  {264, 8, 8, 8, false},
                            {4096, 8, 1, 8, true}};
    for (const Shape &s : shapes)
        for (size_t batch = 1; batch <= 2; ++batch)
            for (size_t off = 0; off < 2; ++off)
                for (int chunked = 0; chunked < 3; ++chunked)
                    for (int cross = 0; cross < 2; ++cross)
                        for (int mode = 0; mode < 3; ++mode) {  // (detrend, average): (1, 1), (0, 1), (1, 0)
                            if (s.big && (mode != 0 || cross || batch != 1 || chunked > 1 || off != (size_t)chunked)) continue;  // 4089 frames: two runs
                            const Opt o{batch, off, chunked, cross != 0, mode != 1, mode != 2, (batch + off) % 2 == 0};
                            run_case<double>(s.len, s.p, s.h, s.f, o);
                            run_case<float>(s.len, s.p, s.h, s.f, o);
                        }
    std::printf("psd: ");
    block_shim::print_counters();
    std::printf("psd: elements %llu checked\n", g_compared);
    std::printf("psd: %s (%d failures)\n", g_fails ? "FAILED" : "ok", g_fails);
    phast_test_exit(g_fails ? 1 : 0);
}
