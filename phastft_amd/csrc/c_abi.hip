// c_abi.hip -- the C ABI of include/phastft_hip.h over the host side of libphastft_hip.so (planner.hpp, exec.hpp, host_api.hpp).
// Mirrors PhastFT's public surface (lib.rs:143-226, planner.rs, options.rs,
// algorithms/r2c.rs:521-895, algorithms/bravo.rs:303-324); see DESIGN.md for the mapping.
//
// There is NO CPU fallback in this library: without a gfx950 device every compute entry point returns
// PHAST_ERR_NO_DEVICE / PHAST_ERR_HIP.
#include "host_util.hpp"
#include "workspace.hpp"
#include "planner.hpp"
#include "planner_pool.hpp"
#include "planner_plans.hpp"
#include "exec.hpp"
#include "planner_r2c.hpp"
#include "entry.hpp"
#include "host_api.hpp"
#include "tune.hpp"
#include "planner_any.hpp"
#include "planner_any_real.hpp"
#include "planner_dct.hpp"
#include "planner_mdct.hpp"
#include "planner_psd.hpp"
#include "planner_lomb.hpp"
#include "planner_channelizer.hpp"
#include "planner_synthesizer.hpp"
#include "planner_cwt.hpp"
#include "planner_dwt.hpp"
#include "planner_resample.hpp"
#include "planner_stft.hpp"
#include "planner_conv.hpp"
#include "planner_convnd.hpp"
#include "planner_czt.hpp"
#include "planner_nufft.hpp"
#include "planner_nd.hpp"
#include "planner_nufft_nd.hpp"
#include "planner_nufft_t3.hpp"

// ================================================================================================
// C ABI
// ================================================================================================
using namespace phast;

struct phast_planner_dit64 : Planner<double> {};
struct phast_planner_dit32 : Planner<float> {};
struct phast_planner_r2c64 : PlannerR2c<double> {};
struct phast_planner_r2c32 : PlannerR2c<float> {};
struct phast_planner_any64 : AnyPlanner<double> {};
struct phast_planner_any32 : AnyPlanner<float> {};
struct phast_planner_r2c_any64 : AnyRealPlanner<double> {};
struct phast_planner_r2c_any32 : AnyRealPlanner<float> {};
struct phast_planner_dct64 : DctPlanner<double> {};
struct phast_planner_dct32 : DctPlanner<float> {};
struct phast_planner_stft64 : StftPlanner<double> {};
struct phast_planner_stft32 : StftPlanner<float> {};
struct phast_planner_mdct64 : MdctPlanner<double> {};
struct phast_planner_mdct32 : MdctPlanner<float> {};
struct phast_planner_psd64 : PsdPlanner<double> {};
struct phast_planner_psd32 : PsdPlanner<float> {};
struct phast_planner_lomb64 : LombPlanner<double> {};
struct phast_planner_lomb32 : LombPlanner<float> {};
struct phast_planner_upfirdn64 : UpfirdnPlanner<double> {};
struct phast_planner_upfirdn32 : UpfirdnPlanner<float> {};
struct phast_planner_dwt64 : DwtPlanner<double> {};
struct phast_planner_dwt32 : DwtPlanner<float> {};
struct phast_planner_resample64 : ResamplePlanner<double> {};
struct phast_planner_resample32 : ResamplePlanner<float> {};
struct phast_planner_channelizer64 : ChannelizerPlanner<double> {};
struct phast_planner_channelizer32 : ChannelizerPlanner<float> {};
struct phast_planner_synthesizer64 : SynthesizerPlanner<double> {};
struct phast_planner_synthesizer32 : SynthesizerPlanner<float> {};
struct phast_planner_cwt64 : CwtPlanner<double> {};
struct phast_planner_cwt32 : CwtPlanner<float> {};
struct phast_planner_conv64 : ConvPlanner<double> {};
struct phast_planner_conv32 : ConvPlanner<float> {};
struct phast_planner_convnd64 : ConvNdPlanner<double> {};
struct phast_planner_convnd32 : ConvNdPlanner<float> {};
struct phast_planner_czt64 : CztPlanner<double> {};
struct phast_planner_czt32 : CztPlanner<float> {};
struct phast_planner_nufft64 : NufftPlanner<double> {};
struct phast_planner_nufft32 : NufftPlanner<float> {};
struct phast_planner_nufft2d64 : NufftNdPlanner<double, 2> {};
struct phast_planner_nufft2d32 : NufftNdPlanner<float, 2> {};
struct phast_planner_nufft3d64 : NufftNdPlanner<double, 3> {};
struct phast_planner_nufft3d32 : NufftNdPlanner<float, 3> {};
struct phast_planner_nufft_t3_64 : NufftT3Planner<double> {};
struct phast_planner_nufft_t3_32 : NufftT3Planner<float> {};
struct phast_planner_nd64 : NdPlanner<double> {};
struct phast_planner_nd32 : NdPlanner<float> {};
struct phast_planner_r2c_nd64 : RealNdPlanner<double> {};
struct phast_planner_r2c_nd32 : RealNdPlanner<float> {};

// W_N^(r*c) tables of a four-step split (twiddle.hip)
template <typename T> struct TwiddleGrid {
    unsigned log_n = 0, tw_bits = 1;
    int device = -1;
    void *d_tw3 = nullptr;
    ~TwiddleGrid() {
        DeviceGuard on(device);
        if (d_tw3) hipFree(d_tw3);
    }
    int init(size_t n) {
        int rc = ensure_device(&device);
        if (rc) return rc;
        log_n = ilog2(n);
        if (log_n > 32) return PHAST_ERR_INVALID_ARG;  // exponents are reduced to 32 bits
        tw_bits = tw3_bits_for(log_n);
        if (((size_t)3 << tw_bits) * sizeof(cx_t<T>) > (size_t)160 * 1024) return PHAST_ERR_INVALID_ARG;  // tables must fit one CU's LDS
        return upload<T>(host_tw3<T>(log_n, tw_bits), &d_tw3);
    }
    int apply(T *d_re, T *d_im, size_t rows, size_t cols, size_t row_pitch, size_t row0, size_t col0, hipStream_t s) const {
        if ((!d_re || !d_im) && rows * cols) return PHAST_ERR_INVALID_ARG;
        if (row_pitch < cols) return PHAST_ERR_INVALID_ARG;
        PHAST_ON_DEVICE(device);
        TwiddleGridArgs a{};
        a.re = d_re;
        a.im = d_im;
        a.tw3 = d_tw3;
        a.rows = rows;
        a.cols = cols;
        a.row_pitch = row_pitch;
        a.row0 = row0;
        a.col0 = col0;
        a.log_n = log_n;
        a.tw_bits = tw_bits;
        PHAST_HIP(launch_twiddle_grid<T>(a, s));
        return PHAST_OK;
    }
};
struct phast_twiddle_grid64 : TwiddleGrid<double> {};
struct phast_twiddle_grid32 : TwiddleGrid<float> {};

// PlannerMode::Tune at construction: one transform per call (the reference's only case) -- unless wisdom already holds a
// measurement for this type, length, kind and device
template <typename P> static int tune_new(P *p, int kind) {
    const size_t eb = sizeof(typename P::value_type);
    if (WisdomStore::instance().lookup(eb, kind, p->wisdom_log_n(), 0, cus_of(p->device_of()), arch_of(p->device_of()), nullptr)) return PHAST_OK;
    return p->tune(kind, 1, nullptr);
}
template <typename R> static void report_to_c(const R &r, phast_tune_report *rep) {
    if (!rep) return;
    rep->adopted = r.adopted;
    rep->candidates = r.candidates;
    rep->us_heuristic = r.us_heuristic;
    rep->us_best = r.us_best;
    rep->seconds = r.seconds;
    std::snprintf(rep->plan, sizeof rep->plan, "%s", r.plan.c_str());
}

// No C++ exception leaves the library: the callers are C, Rust (unwinding across `extern "C"` is undefined there), ctypes.
// Host memory exhaustion (std::bad_alloc, std::length_error) becomes PHAST_ERR_ALLOC; anything else PHAST_ERR_HIP with the
// exception's text in phast_last_hip_error().
static int cxx_exception_rc() noexcept {
    try {
        throw;
    } catch (const std::bad_alloc &) {
        return PHAST_ERR_ALLOC;
    } catch (const std::length_error &) {
        return PHAST_ERR_ALLOC;
    } catch (const std::exception &e) {
        std::snprintf(g_hip_err, sizeof g_hip_err, "C++ exception in the host library: %s", e.what());
        return PHAST_ERR_HIP;
    } catch (...) {
        std::snprintf(g_hip_err, sizeof g_hip_err, "unknown C++ exception in the host library");
        return PHAST_ERR_HIP;
    }
}
#define PHAST_CATCH_RC catch (...) { return cxx_exception_rc(); }
#define PHAST_CATCH_ZERO catch (...) { return 0; }
#define PHAST_CATCH_VOID catch (...) {}

extern "C" {

int phast_wisdom_export(char *buf, size_t buf_len, size_t *needed) try {
    const std::string text = WisdomStore::instance().export_text();
    if (needed) *needed = text.size() + 1;
    if (!buf || buf_len == 0) return needed ? PHAST_OK : PHAST_ERR_INVALID_ARG;
    if (buf_len < text.size() + 1) return PHAST_ERR_INVALID_ARG;
    std::memcpy(buf, text.c_str(), text.size() + 1);
    return PHAST_OK;
} PHAST_CATCH_RC
int phast_wisdom_import(const char *text) try {
    if (!text) return PHAST_ERR_INVALID_ARG;
    return WisdomStore::instance().import_text(text, 2) == 0 ? PHAST_OK : PHAST_ERR_INVALID_ARG;
} PHAST_CATCH_RC
void phast_wisdom_forget(void) try { WisdomStore::instance().forget(); } PHAST_CATCH_VOID
int phast_wisdom_builtin(int enable) try { return WisdomStore::instance().set_builtin(enable != 0) ? 1 : 0; } PHAST_CATCH_ZERO
size_t phast_wisdom_count(int layer) try { return WisdomStore::instance().count(layer); } PHAST_CATCH_ZERO
int phast_debug_wisdom_lookup(size_t elem_bytes, int kind, unsigned log_n, unsigned bucket, int cus, int arch, char *buf,
                              size_t buf_len) try {
    if ((elem_bytes != 4 && elem_bytes != 8) || kind < 0 || kind >= kNumKinds) return -1;
    // through lookup_all, the call a planner makes (Planner::apply_wisdom)
    const std::map<unsigned, WisdomEntry> all = WisdomStore::instance().lookup_all(elem_bytes, kind, log_n, cus, arch);
    const auto it = all.find(bucket);
    if (it == all.end()) return -1;
    if (buf && buf_len) std::snprintf(buf, buf_len, "%s", it->second.heuristic ? "heuristic" : spec_to_string(it->second.spec).c_str());
    return it->second.layer;
} catch (...) { return -1; }

const char *phast_strerror(int code) {
    switch (code) {
    case PHAST_OK: return "ok";
    case PHAST_ERR_NOT_POW2: return "assertion failed: num_points > 0 && num_points.is_power_of_two()";
    case PHAST_ERR_LEN_MISMATCH: return "assertion `left == right` failed: reals.len() == imags.len()";
    case PHAST_ERR_PLANNER_SIZE: return "assertion `left == right` failed: log_n == planner.log_n";
    case PHAST_ERR_R2C_N: return "n must be a power of 2 >= 4";
    case PHAST_ERR_R2C_INPUT_LEN: return "input length must match planner size";
    case PHAST_ERR_R2C_OUT_RE_LEN: return "output_re must have length N/2 + 1";
    case PHAST_ERR_R2C_OUT_IM_LEN: return "output_im must have length N/2 + 1";
    case PHAST_ERR_C2R_OUTPUT_LEN: return "output length must match planner size";
    case PHAST_ERR_C2R_IN_RE_LEN: return "input_re must have length N/2 + 1";
    case PHAST_ERR_C2R_IN_IM_LEN: return "input_im must have length N/2 + 1";
    case PHAST_ERR_C2R_SCRATCH_RE: return "scratch_re must have length N/2";
    case PHAST_ERR_C2R_SCRATCH_IM: return "scratch_im must have length N/2";
    case PHAST_ERR_ALLOC: return "host allocation failed";
    case PHAST_ERR_HIP: return "HIP runtime error (see phast_last_hip_error)";
    case PHAST_ERR_NO_DEVICE: return "no HIP device visible: libphastft_hip has no CPU fallback";
    case PHAST_ERR_INVALID_ARG: return "invalid argument";
    default: return "unknown error";
    }
}

const char *phast_last_hip_error(void) { return g_hip_err; }

int phast_hip_graph_upload(void *graph_exec, void *stream) try {
    if (!graph_exec) return PHAST_ERR_INVALID_ARG;
    PHAST_HIP(hipGraphUpload(static_cast<hipGraphExec_t>(graph_exec), static_cast<hipStream_t>(stream)));
    return PHAST_OK;
} PHAST_CATCH_RC

int phast_stream_probe_dev(const void *d_a, void *d_b, size_t bytes, int reps, double *out_gbps, void *stream) try {
    if (!d_a || !d_b || !out_gbps || reps < 1 || bytes < ((size_t)1 << 20) || (bytes & 15)) return PHAST_ERR_INVALID_ARG;
    int dev = 0;
    int rc = ensure_device(&dev);
    if (rc) return rc;
    PHAST_HIP(stream_probe(d_a, d_b, bytes, reps, cus_of(dev), out_gbps, static_cast<hipStream_t>(stream)));
    return PHAST_OK;
} PHAST_CATCH_RC

int phast_debug_throw(int what) try {
    if (what == 1) throw std::bad_alloc();
    if (what == 2) throw std::runtime_error("phast_debug_throw");
    if (what == 3) throw 3;
    return PHAST_OK;
} PHAST_CATCH_RC

void phast_debug_set_guard_bytes(size_t bytes) try { g_guard_bytes = (bytes + 255) & ~(size_t)255; } PHAST_CATCH_VOID

void phast_debug_set_wg_per_cu(int wg_per_cu) try { g_wg_per_cu_override = wg_per_cu; } PHAST_CATCH_VOID
void phast_debug_set_trace(unsigned long long *d_trace) try { g_trace = d_trace; } PHAST_CATCH_VOID

int phast_device_info(char *name, size_t name_len, int *compute_units, size_t *lds_per_block,
                      size_t *global_mem_bytes) try {
    int rc = ensure_device();
    if (rc) return rc;
    int dev = 0;
    PHAST_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    PHAST_HIP(hipGetDeviceProperties(&prop, dev));
    if (name && name_len) std::snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (lds_per_block) *lds_per_block = prop.sharedMemPerBlock;
    if (global_mem_bytes) *global_mem_bytes = prop.totalGlobalMem;
    return PHAST_OK;
} PHAST_CATCH_RC

void phast_options_default(phast_options *out) try {
    if (!out) return;
    out->multithreaded_bit_reversal = 0;
    out->smallest_parallel_chunk_size = 16384;
} PHAST_CATCH_VOID

int phast_options_guess(size_t input_size, phast_options *out) try {
    if (!out) return PHAST_ERR_INVALID_ARG;
    if (input_size == 0) return PHAST_ERR_NOT_POW2;  // usize::ilog2(0) panics (options.rs:40)
    phast_options_default(out);
    out->multithreaded_bit_reversal = ilog2(input_size) >= 16;
    return PHAST_OK;
} PHAST_CATCH_RC

#define PHAST_PLANNER_API(SFX, T)                                                                                       \
    int phast_planner_dit##SFX##_new(size_t n, phast_planner_dit##SFX **out) try {                                      \
        return planner_new(n, out);                                                                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dit##SFX##_with_mode(size_t n, int mode, phast_planner_dit##SFX **out) try {                      \
        if (mode != PHAST_MODE_HEURISTIC && mode != PHAST_MODE_TUNE) return PHAST_ERR_INVALID_ARG;                      \
        int rc = planner_new(n, out);                                                                                   \
        if (rc == PHAST_OK && mode == PHAST_MODE_TUNE) rc = tune_new(*out, kC2C);                                       \
        if (rc != PHAST_OK && out && *out) {                                                                            \
            delete *out;                                                                                                \
            *out = nullptr;                                                                                             \
        }                                                                                                               \
        return rc;                                                                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dit##SFX##_tune(phast_planner_dit##SFX *p, size_t batch, int kind, phast_tune_report *rep) try {  \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        Planner<T>::TuneReport r;                                                                                       \
        int rc = p->tune(kind, batch, &r);                                                                              \
        if (rc == PHAST_OK) report_to_c(r, rep);                                                                        \
        return rc;                                                                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    void phast_planner_dit##SFX##_free(phast_planner_dit##SFX *p) try { delete p; } PHAST_CATCH_VOID                    \
    size_t phast_planner_dit##SFX##_device_bytes(const phast_planner_dit##SFX *p) try {                                 \
        return p ? p->device_bytes() : 0;                                                                               \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_dit##SFX##_debug_check_guards(const phast_planner_dit##SFX *p, size_t *bad_bytes) try {           \
        if (!p || !bad_bytes) return PHAST_ERR_INVALID_ARG;                                                             \
        return p->check_guards(bad_bytes);                                                                              \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dit##SFX##_describe(const phast_planner_dit##SFX *p, char *buf, size_t len) try {                 \
        return describe_to<T>(p, buf, len);                                                                             \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dit##SFX##_describe_call(const phast_planner_dit##SFX *p, size_t batch, int kind, char *buf,      \
                                               size_t len) try {                                                        \
        if (!p || !buf || !len || (kind != kC2C && kind != kC2CI)) return PHAST_ERR_INVALID_ARG;                        \
        std::snprintf(buf, len, "%s", p->describe_call(kind, batch).c_str());                                           \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_describe_call(const phast_planner_r2c##SFX *p, size_t batch, int kind, char *buf,      \
                                               size_t len) try {                                                        \
        if (!p || !buf || !len || (kind != kR2C && kind != kC2R)) return PHAST_ERR_INVALID_ARG;                         \
        const PlannerR2c<T> *q = p->route_small(kind == kC2R, batch);                                                   \
        std::snprintf(buf, len, "%s", q->dit.passes.empty() ? "one-pass" : q->dit.describe_call(kind, batch).c_str());  \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_debug_check_guards(const phast_planner_r2c##SFX *p, size_t *bad_bytes) try {           \
        if (!p || !bad_bytes) return PHAST_ERR_INVALID_ARG;                                                             \
        /* the real transforms run on the inner planner's workspace pool -- and on the multi-pass twin's */             \
        int rc = p->dit.check_guards(bad_bytes);                                                                        \
        size_t bad_twin = 0;                                                                                            \
        if (rc == PHAST_OK && p->twin) rc = p->twin->dit.check_guards(&bad_twin);                                       \
        *bad_bytes += bad_twin;                                                                                         \
        return rc;                                                                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dit##SFX##_reserve_batch(phast_planner_dit##SFX *p, size_t max_batch) try {                       \
        if (!p || max_batch == 0) return PHAST_ERR_INVALID_ARG;                                                         \
        return p->reserve_batch(max_batch);                                                                             \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_dit##SFX##_release_graph_workspaces(phast_planner_dit##SFX *p) try {                           \
        return p ? p->release_graph_workspaces() : 0;                                                                   \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_dit##SFX##_set_plan(phast_planner_dit##SFX *p, const unsigned *lr, const unsigned *tl,            \
                                          size_t np, unsigned points_log) try {                                         \
        return set_plan_c<T>(p, lr, tl, np, points_log);                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dit##SFX##_time_passes(const phast_planner_dit##SFX *p, T *d_re, T *d_im, size_t batch,           \
                                             size_t dist, int reps, float *pass_ms, int *n_passes, void *stream) try {  \
        return time_passes<T>(p, d_re, d_im, batch, dist, reps, pass_ms, n_passes,                                      \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_new(size_t n, phast_planner_r2c##SFX **out) try {                                      \
        return r2c_planner_new(n, out);                                                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    void phast_planner_r2c##SFX##_free(phast_planner_r2c##SFX *p) try { delete p; } PHAST_CATCH_VOID                    \
    int phast_planner_r2c##SFX##_with_mode(size_t n, int mode, phast_planner_r2c##SFX **out) try {                      \
        if (mode != PHAST_MODE_HEURISTIC && mode != PHAST_MODE_TUNE) return PHAST_ERR_INVALID_ARG;                      \
        int rc = r2c_planner_new(n, out);                                                                               \
        if (rc == PHAST_OK && mode == PHAST_MODE_TUNE) rc = tune_new(*out, kR2C);                                       \
        if (rc == PHAST_OK && mode == PHAST_MODE_TUNE) rc = tune_new(*out, kC2R);                                       \
        if (rc != PHAST_OK && out && *out) {                                                                            \
            delete *out;                                                                                                \
            *out = nullptr;                                                                                             \
        }                                                                                                               \
        return rc;                                                                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_tune(phast_planner_r2c##SFX *p, size_t batch, int kind, phast_tune_report *rep) try {  \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        Planner<T>::TuneReport r;                                                                                       \
        int rc = p->tune(kind, batch, &r);                                                                              \
        if (rc == PHAST_OK) report_to_c(r, rep);                                                                        \
        return rc;                                                                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_time_passes(const phast_planner_r2c##SFX *p, const T *d_in, T *d_ore, T *d_oim,        \
                                             size_t batch, size_t in_dist, size_t out_dist, int reps,                   \
                                             float *pass_ms, int *n_passes, void *stream) try {                         \
        return time_passes_r2c<T>(p, d_in, d_ore, d_oim, batch, in_dist, out_dist, reps, pass_ms, n_passes,             \
                                  static_cast<hipStream_t>(stream));                                                    \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_time_c2r_passes(const phast_planner_r2c##SFX *p, const T *d_ire, const T *d_iim,       \
                                                 T *d_out, size_t batch, size_t in_dist, size_t out_dist, int reps,     \
                                                 float *pass_ms, int *n_passes, void *stream) try {                     \
        return time_passes_c2r<T>(p, d_ire, d_iim, d_out, batch, in_dist, out_dist, reps, pass_ms, n_passes,            \
                                  static_cast<hipStream_t>(stream));                                                    \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_set_inner_plan(phast_planner_r2c##SFX *p, const unsigned *lr, const unsigned *tl,      \
                                                size_t np, unsigned points_log) try {                                   \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        PlannerR2c<T> *q = (p->dit.passes.empty() && p->twin) ? p->twin.get() : p;                                      \
        int rc = set_plan_c<T>(&q->dit, lr, tl, np, points_log);                                                        \
        if (rc == PHAST_OK && np == 0 && !q->dit.passes.empty()) rc = q->dit.make_c2r_plans();                          \
        return rc;                                                                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c##SFX##_describe(const phast_planner_r2c##SFX *p, char *buf, size_t len) try {                 \
        if (!p || !buf || !len) return PHAST_ERR_INVALID_ARG;                                                           \
        std::string s = p->dit.describe();                                                                              \
        if (p->twin)                                                                                                    \
            s += std::string(p->route_small(false) != p ? " | one transform: " : " | one c2r transform: ") +            \
                 p->twin->dit.describe();                                                                               \
        std::snprintf(buf, len, "%s", s.c_str());                                                                       \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC

PHAST_PLANNER_API(64, double)
PHAST_PLANNER_API(32, float)

#define PHAST_FFT_API(SFX, FS, T)                                                                                       \
    int phast_fft_##SFX##_dit(T *re, size_t re_len, T *im, size_t im_len, int direction) try {                          \
        return fft_host_noplanner<T>(re, re_len, im, im_len, direction);                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_dit_with_planner(T *re, size_t re_len, T *im, size_t im_len, int direction,                   \
                                           const phast_planner_dit##SFX *pl) try {                                      \
        return fft_host<T>(re, re_len, im, im_len, direction, pl);                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_dit_with_planner_and_opts(T *re, size_t re_len, T *im, size_t im_len, int direction,          \
                                                    const phast_planner_dit##SFX *pl, const phast_options *opts) try {  \
        if (!opts) return PHAST_ERR_INVALID_ARG;                                                                        \
        return fft_host<T>(re, re_len, im, im_len, direction, pl);                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_dit_dev(T *d_re, T *d_im, size_t n, size_t batch, size_t dist, int direction,                 \
                                  const phast_planner_dit##SFX *pl, void *stream) try {                                 \
        return fft_dev<T>(d_re, d_im, n, batch, dist, direction, pl, static_cast<hipStream_t>(stream));                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_dit_many_dev(T *const *d_re, T *const *d_im, size_t count, size_t n, int direction,           \
                                       const phast_planner_dit##SFX *pl, void *stream) try {                            \
        return fft_dev_many<T>(d_re, d_im, count, n, direction, pl, static_cast<hipStream_t>(stream));                  \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_dit_strided_dev(T *d_re, T *d_im, size_t n, size_t batch, size_t dist, size_t stride,         \
                                          int direction, const phast_planner_dit##SFX *pl, void *stream) try {          \
        return fft_strided_dev<T>(d_re, d_im, n, batch, dist, stride, direction, pl,                                    \
                                  static_cast<hipStream_t>(stream));                                                    \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_dit_strided_tw_dev(T *d_re, T *d_im, size_t n, size_t batch, size_t dist, size_t stride,      \
                                             int direction, const phast_planner_dit##SFX *pl, size_t tw_n,              \
                                             size_t tw_col0, void *stream) try {                                        \
        if (tw_n == 0) return PHAST_ERR_INVALID_ARG;                                                                    \
        return fft_strided_dev<T>(d_re, d_im, n, batch, dist, stride, direction, pl,                                    \
                                  static_cast<hipStream_t>(stream), tw_n, tw_col0);                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_interleaved(T *signal, size_t n, int direction) try {                                         \
        std::shared_ptr<Planner<T>> pl; /* lib.rs:121: a planner per call -- kept, see PlannerCache */                  \
        int rc = PlannerCache<Planner<T>>::instance().get(                                                              \
            n, sizeof(T), [](size_t m, Planner<T> **o) { return planner_new(m, o); }, &pl);                             \
        if (rc) return rc;                                                                                              \
        return fft_interleaved_host<T>(signal, n, direction, pl.get());                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_interleaved_with_planner(T *signal, size_t n, int direction,                                  \
                                                   const phast_planner_dit##SFX *pl) try {                              \
        return fft_interleaved_host<T>(signal, n, direction, pl);                                                       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_interleaved_with_planner_and_opts(T *signal, size_t n, int direction,                         \
                                                            const phast_planner_dit##SFX *pl,                           \
                                                            const phast_options *opts) try {                            \
        if (!opts) return PHAST_ERR_INVALID_ARG;                                                                        \
        return fft_interleaved_host<T>(signal, n, direction, pl);                                                       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_interleaved_dev(T *d_signal, size_t n, size_t batch, size_t dist, int direction,              \
                                          const phast_planner_dit##SFX *pl, void *stream) try {                         \
        return fft_interleaved_dev<T>(d_signal, n, batch, dist, direction, pl, static_cast<hipStream_t>(stream));       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_bit_rev_##FS(T *data, size_t len, unsigned log_n) try { return bitrev_host<T>(data, len, log_n); } PHAST_CATCH_RC \
    int phast_bit_rev_##FS##_dev(T *d, unsigned log_n, size_t batch, size_t dist, void *stream) try {                   \
        if (!d || log_n > 31 || (batch > 1 && dist < ((size_t)1 << log_n))) return PHAST_ERR_INVALID_ARG;               \
        int rc = ensure_device();                                                                                       \
        if (rc) return rc;                                                                                              \
        PHAST_HIP(launch_bitrev<T>(d, log_n, batch, dist, static_cast<hipStream_t>(stream)));                           \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_deinterleave_##FS(const T *in, size_t len, T *a, size_t a_len, T *b, size_t b_len) try {                  \
        return deinterleave_host<T>(in, len, a, a_len, b, b_len);                                                       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_deinterleave_##FS##_dev(const T *d_in, size_t len, T *d_a, T *d_b, void *stream) try {                    \
        if (len < 2) return PHAST_OK; /* chunks_exact(2) of fewer than two elements: nothing */                         \
        if (!d_in || !d_a || !d_b) return PHAST_ERR_INVALID_ARG;                                                        \
        int rc = ensure_device();                                                                                       \
        if (rc) return rc;                                                                                              \
        PHAST_HIP(launch_deinterleave<T>(d_in, d_a, d_b, len / 2, static_cast<hipStream_t>(stream)));                   \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_combine_re_im_##FS(const T *re, size_t re_len, const T *im, size_t im_len, T *out, size_t out_len) try {  \
        return combine_host<T>(re, re_len, im, im_len, out, out_len);                                                   \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_combine_re_im_##FS##_dev(const T *d_re, const T *d_im, size_t n, T *d_out, void *stream) try {            \
        if (n == 0) return PHAST_OK;                                                                                    \
        if (!d_re || !d_im || !d_out) return PHAST_ERR_INVALID_ARG;                                                     \
        int rc = ensure_device();                                                                                       \
        if (rc) return rc;                                                                                              \
        PHAST_HIP(launch_combine<T>(d_re, d_im, d_out, n, static_cast<hipStream_t>(stream)));                           \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS(const T *in, size_t in_len, T *ore, size_t ore_len, T *oim, size_t oim_len) try {            \
        std::shared_ptr<PlannerR2c<T>> pl; /* r2c.rs:522: planner from input_re.len() */                                \
        int rc = PlannerCache<PlannerR2c<T>>::instance().get(                                                           \
            in_len, sizeof(T), [](size_t m, PlannerR2c<T> **o) { return r2c_planner_new(m, o); }, &pl);                 \
        if (rc) return rc;                                                                                              \
        return r2c_host<T>(in, in_len, ore, ore_len, oim, oim_len, pl.get());                                           \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_with_planner(const T *in, size_t in_len, T *ore, size_t ore_len, T *oim,                   \
                                          size_t oim_len, const phast_planner_r2c##SFX *pl) try {                       \
        return r2c_host<T>(in, in_len, ore, ore_len, oim, oim_len, pl);                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_dev(const T *d_in, T *d_ore, T *d_oim, size_t batch, size_t in_dist, size_t out_dist,      \
                                 const phast_planner_r2c##SFX *pl, void *stream) try {                                  \
        if (!pl || !d_in || !d_ore || !d_oim) return PHAST_ERR_INVALID_ARG;                                             \
        if (batch > 1 && (in_dist < pl->n || out_dist < pl->n / 2 + 1)) return PHAST_ERR_INVALID_ARG;                   \
        return pl->r2c(d_in, d_ore, d_oim, batch, in_dist, out_dist, static_cast<hipStream_t>(stream));                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *out, size_t out_len) try {    \
        std::shared_ptr<PlannerR2c<T>> pl; /* r2c.rs:696: planner from output.len() */                                  \
        int rc = PlannerCache<PlannerR2c<T>>::instance().get(                                                           \
            out_len, sizeof(T), [](size_t m, PlannerR2c<T> **o) { return r2c_planner_new(m, o); }, &pl);                \
        if (rc) return rc;                                                                                              \
        return c2r_host<T>(ire, ire_len, iim, iim_len, out, out_len, pl.get(), false, 0, 0);                            \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_with_planner(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *out,           \
                                          size_t out_len, const phast_planner_r2c##SFX *pl) try {                       \
        return c2r_host<T>(ire, ire_len, iim, iim_len, out, out_len, pl, false, 0, 0);                                  \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_with_planner_and_scratch(const T *ire, size_t ire_len, const T *iim, size_t iim_len,       \
                                                      T *out, size_t out_len, const phast_planner_r2c##SFX *pl,         \
                                                      T *sre, size_t sre_len, T *sim, size_t sim_len) try {             \
        (void)sre;                                                                                                      \
        (void)sim;                                                                                                      \
        return c2r_host<T>(ire, ire_len, iim, iim_len, out, out_len, pl, true, sre_len, sim_len);                       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_dev(const T *d_ire, const T *d_iim, T *d_out, size_t batch, size_t in_dist,                \
                                 size_t out_dist, const phast_planner_r2c##SFX *pl, void *stream) try {                 \
        if (!pl || !d_ire || !d_iim || !d_out) return PHAST_ERR_INVALID_ARG;                                            \
        if (batch > 1 && (in_dist < pl->n / 2 + 1 || out_dist < pl->n)) return PHAST_ERR_INVALID_ARG;                   \
        return pl->c2r(d_ire, d_iim, d_out, batch, in_dist, out_dist, static_cast<hipStream_t>(stream));                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fill_##FS##_dev(T *d_re, T *d_im, size_t n, size_t batch, size_t dist, unsigned long long seed,           \
                              unsigned long long first_id, void *stream) try {                                          \
        if (!d_re) return PHAST_ERR_INVALID_ARG;                                                                        \
        int rc = ensure_device();                                                                                       \
        if (rc) return rc;                                                                                              \
        PHAST_HIP(launch_fill<T>(d_re, d_im, n, batch, dist, seed, first_id, static_cast<hipStream_t>(stream)));        \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_digest_##FS##_dev(const T *d_re, const T *d_im, size_t n, size_t batch, size_t dist, size_t probe,        \
                                double *d_digest, void *stream) try {                                                   \
        if (!d_re || !d_im || !d_digest) return PHAST_ERR_INVALID_ARG;                                                  \
        int rc = ensure_device();                                                                                       \
        if (rc) return rc;                                                                                              \
        PHAST_HIP(launch_digest<T>(d_re, d_im, n, batch, dist, probe, d_digest, static_cast<hipStream_t>(stream)));     \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC

PHAST_FFT_API(64, f64, double)
PHAST_FFT_API(32, f32, float)

#define PHAST_TWIDDLE_API(SFX, T)                                                                                       \
    int phast_twiddle_grid##SFX##_new(size_t n, phast_twiddle_grid##SFX **out) try {                                    \
        return planner_new(n, out);                                                                                     \
    } PHAST_CATCH_RC                                                                                                    \
    void phast_twiddle_grid##SFX##_free(phast_twiddle_grid##SFX *g) try { delete g; } PHAST_CATCH_VOID                  \
    int phast_twiddle_grid##SFX##_apply_dev(const phast_twiddle_grid##SFX *g, T *d_re, T *d_im, size_t rows,            \
                                            size_t cols, size_t row_pitch, size_t row0, size_t col0, void *stream) try { \
        if (!g) return PHAST_ERR_INVALID_ARG;                                                                           \
        return g->apply(d_re, d_im, rows, cols, row_pitch, row0, col0, static_cast<hipStream_t>(stream));               \
    } PHAST_CATCH_RC
PHAST_TWIDDLE_API(64, double)
PHAST_TWIDDLE_API(32, float)

// What every planner behind an opaque handle has in common, whatever it plans: _free, _describe, _device_bytes and
// _workspace_len of phast_planner_<NAME>.  (The dit and r2c planners differ -- describe_to, twin plans, no workspace length --
// and spell theirs out above; every family's _new and calls follow below.)
#define PHAST_HANDLE_API(NAME)                                                                                          \
    void phast_planner_##NAME##_free(phast_planner_##NAME *p) try { delete p; } PHAST_CATCH_VOID                        \
    int phast_planner_##NAME##_describe(const phast_planner_##NAME *p, char *buf, size_t len) try {                     \
        if (!p || !buf || !len) return PHAST_ERR_INVALID_ARG;                                                           \
        std::snprintf(buf, len, "%s", p->describe().c_str());                                                           \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_##NAME##_device_bytes(const phast_planner_##NAME *p) try {                                     \
        return p ? p->device_bytes() : 0;                                                                               \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_##NAME##_workspace_len(const phast_planner_##NAME *p, size_t batch) try {                      \
        return p ? p->workspace_len(batch) : 0;                                                                         \
    } PHAST_CATCH_ZERO
PHAST_HANDLE_API(any64) PHAST_HANDLE_API(any32) PHAST_HANDLE_API(r2c_any64) PHAST_HANDLE_API(r2c_any32)
PHAST_HANDLE_API(dct64) PHAST_HANDLE_API(dct32) PHAST_HANDLE_API(stft64) PHAST_HANDLE_API(stft32)
PHAST_HANDLE_API(conv64) PHAST_HANDLE_API(conv32) PHAST_HANDLE_API(czt64) PHAST_HANDLE_API(czt32)
PHAST_HANDLE_API(nufft64) PHAST_HANDLE_API(nufft32) PHAST_HANDLE_API(nufft2d64) PHAST_HANDLE_API(nufft2d32)
PHAST_HANDLE_API(nufft3d64) PHAST_HANDLE_API(nufft3d32) PHAST_HANDLE_API(nufft_t3_64) PHAST_HANDLE_API(nufft_t3_32)
PHAST_HANDLE_API(nd64) PHAST_HANDLE_API(nd32) PHAST_HANDLE_API(r2c_nd64) PHAST_HANDLE_API(r2c_nd32)
PHAST_HANDLE_API(convnd64) PHAST_HANDLE_API(convnd32) PHAST_HANDLE_API(mdct64) PHAST_HANDLE_API(mdct32)
PHAST_HANDLE_API(lomb64) PHAST_HANDLE_API(lomb32) PHAST_HANDLE_API(upfirdn64) PHAST_HANDLE_API(upfirdn32)
PHAST_HANDLE_API(resample64) PHAST_HANDLE_API(resample32) PHAST_HANDLE_API(channelizer64) PHAST_HANDLE_API(channelizer32)
PHAST_HANDLE_API(synthesizer64) PHAST_HANDLE_API(synthesizer32) PHAST_HANDLE_API(cwt64) PHAST_HANDLE_API(cwt32)
PHAST_HANDLE_API(dwt64) PHAST_HANDLE_API(dwt32)

// Arbitrary lengths (Bluestein, planner_any.hpp): arguments are checked before the device is touched
#define PHAST_ANY_API(SFX, T)                                                                                           \
    int phast_planner_any##SFX##_new(size_t n, phast_planner_any##SFX **out) try {                                      \
        return any_planner_new(n, out);                                                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_any##SFX##_time_stages(const phast_planner_any##SFX *p, T *d_re, T *d_im, size_t batch,           \
                                             size_t dist, T *d_work, size_t work_len, int reps, float *stage_ms,        \
                                             void *stream) try {                                                        \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_re, d_im, batch, dist, d_work, work_len, reps, stage_ms,                                \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_any(T *re, size_t re_len, T *im, size_t im_len, int direction) try {                          \
        if ((!re && re_len) || (!im && im_len)) return PHAST_ERR_INVALID_ARG;                                           \
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;                     \
        if (re_len != im_len) return PHAST_ERR_LEN_MISMATCH;                                                            \
        std::shared_ptr<AnyPlanner<T>> pl; /* the planner from reals.len(), kept as fft_*_dit keeps its own */          \
        int rc = PlannerCache<AnyPlanner<T>>::instance().get(                                                           \
            re_len, sizeof(T), [](size_t m, AnyPlanner<T> **o) { return any_planner_new(m, o); }, &pl);                 \
        if (rc) return rc;                                                                                              \
        return pl->fft_host_any(re, re_len, im, im_len, direction);                                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_any_with_planner(T *re, size_t re_len, T *im, size_t im_len, int direction,                   \
                                           const phast_planner_any##SFX *p) try {                                       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->fft_host_any(re, re_len, im, im_len, direction);                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_any_dev(T *d_re, T *d_im, size_t n, size_t batch, size_t dist, int direction,                 \
                                  const phast_planner_any##SFX *p, T *d_work, size_t work_len, void *stream) try {      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->fft_dev_any(d_re, d_im, n, batch, dist, direction, d_work, work_len, static_cast<hipStream_t>(stream)); \
    } PHAST_CATCH_RC
PHAST_ANY_API(64, double)
PHAST_ANY_API(32, float)

// Real transforms of arbitrary lengths (planner_any_real.hpp): arguments are checked before the device is touched
#define PHAST_ANY_REAL_API(SFX, FS, T)                                                                                  \
    int phast_planner_r2c_any##SFX##_new(size_t n, phast_planner_r2c_any##SFX **out) try {                              \
        return any_planner_new(n, out);                                                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c_any##SFX##_time_stages(const phast_planner_r2c_any##SFX *p, const T *d_in, T *d_out_re,       \
                                                 T *d_out_im, size_t batch, T *d_work, size_t work_len, int reps,       \
                                                 float *stage_ms, void *stream) try {                                   \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(false, d_in, nullptr, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,        \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_r2c_any##SFX##_time_c2r_stages(const phast_planner_r2c_any##SFX *p, const T *d_in_re,             \
                                                     const T *d_in_im, T *d_out, size_t batch, T *d_work,               \
                                                     size_t work_len, int reps, float *stage_ms, void *stream) try {    \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(true, d_in_re, d_in_im, d_out, nullptr, batch, d_work, work_len, reps, stage_ms,          \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_any(const T *in, size_t in_len, T *ore, size_t ore_len, T *oim, size_t oim_len) try {      \
        if (!in || !ore || !oim || in_len == 0 || in_len > kAnyMaxN) return PHAST_ERR_INVALID_ARG;                      \
        if (ore_len != in_len / 2 + 1) return PHAST_ERR_R2C_OUT_RE_LEN; /* before the device is touched */             \
        if (oim_len != in_len / 2 + 1) return PHAST_ERR_R2C_OUT_IM_LEN;                                                 \
        std::shared_ptr<AnyRealPlanner<T>> pl; /* the planner from input.len(), as r2c_fft_* */                        \
        int rc = PlannerCache<AnyRealPlanner<T>>::instance().get(                                                       \
            in_len, sizeof(T), [](size_t m, AnyRealPlanner<T> **o) { return any_planner_new(m, o); }, &pl);             \
        if (rc) return rc;                                                                                              \
        return pl->host(false, in, in_len, nullptr, 0, ore, ore_len, oim, oim_len);                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_any_with_planner(const T *in, size_t in_len, T *ore, size_t ore_len, T *oim,               \
                                              size_t oim_len, const phast_planner_r2c_any##SFX *p) try {                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(false, in, in_len, nullptr, 0, ore, ore_len, oim, oim_len);                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_any_dev(const T *d_in, T *d_ore, T *d_oim, size_t n, size_t batch, size_t in_dist,         \
                                     size_t out_dist, const phast_planner_r2c_any##SFX *p, T *d_work, size_t work_len,  \
                                     void *stream) try {                                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(false, d_in, nullptr, d_ore, d_oim, n, batch, in_dist, out_dist, d_work, work_len,                \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_any(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *out, size_t out_len) try { \
        if (!ire || !iim || !out || out_len == 0 || out_len > kAnyMaxN) return PHAST_ERR_INVALID_ARG;                   \
        if (ire_len != out_len / 2 + 1) return PHAST_ERR_C2R_IN_RE_LEN; /* before the device is touched */             \
        if (iim_len != out_len / 2 + 1) return PHAST_ERR_C2R_IN_IM_LEN;                                                 \
        std::shared_ptr<AnyRealPlanner<T>> pl; /* the planner from output.len(), as c2r_fft_* */                       \
        int rc = PlannerCache<AnyRealPlanner<T>>::instance().get(                                                       \
            out_len, sizeof(T), [](size_t m, AnyRealPlanner<T> **o) { return any_planner_new(m, o); }, &pl);            \
        if (rc) return rc;                                                                                              \
        return pl->host(true, ire, ire_len, iim, iim_len, out, out_len, nullptr, 0);                                    \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_any_with_planner(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *out,       \
                                              size_t out_len, const phast_planner_r2c_any##SFX *p) try {                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(true, ire, ire_len, iim, iim_len, out, out_len, nullptr, 0);                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_any_dev(const T *d_ire, const T *d_iim, T *d_out, size_t n, size_t batch, size_t in_dist,  \
                                     size_t out_dist, const phast_planner_r2c_any##SFX *p, T *d_work, size_t work_len,  \
                                     void *stream) try {                                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(true, d_ire, d_iim, d_out, nullptr, n, batch, in_dist, out_dist, d_work, work_len,                \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_ANY_REAL_API(64, f64, double)
PHAST_ANY_REAL_API(32, f32, float)

// DCT / DST of types II and III (planner_dct.hpp): type, norm and every length are checked before the device is touched
#define PHAST_DCT_API(SFX, FS, T)                                                                                       \
    int phast_planner_dct##SFX##_new(size_t n, phast_planner_dct##SFX **out) try {                                      \
        return any_planner_new(n, out);                                                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_dct##SFX##_time_stages(const phast_planner_dct##SFX *p, int dst, int type, int norm,              \
                                             const T *d_in, T *d_out, size_t batch, T *d_work, size_t work_len,         \
                                             int reps, float *stage_ms, void *stream) try {                             \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(type, dst != 0, norm, d_in, d_out, batch, d_work, work_len, reps, stage_ms,               \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    PHAST_DCT_CALLS(SFX, FS, T, dct, false)                                                                             \
    PHAST_DCT_CALLS(SFX, FS, T, dst, true)
#define PHAST_DCT_CALLS(SFX, FS, T, KIND, DST)                                                                          \
    int phast_##KIND##_##FS(const T *in, size_t in_len, T *out, size_t out_len, int type, int norm) try {               \
        if (!in || !out || !DctPlanner<T>::valid(type, norm)) return PHAST_ERR_INVALID_ARG;                             \
        if (in_len == 0 || in_len > kAnyMaxN) return PHAST_ERR_INVALID_ARG;                                             \
        if (in_len != out_len) return PHAST_ERR_LEN_MISMATCH; /* before the device is touched */                       \
        std::shared_ptr<DctPlanner<T>> pl; /* the planner from in_len, as r2c_fft_*_any */                             \
        int rc = PlannerCache<DctPlanner<T>>::instance().get(                                                           \
            in_len, sizeof(T), [](size_t m, DctPlanner<T> **o) { return any_planner_new(m, o); }, &pl);                 \
        if (rc) return rc;                                                                                              \
        return pl->host(type, DST, in, in_len, out, out_len, norm);                                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_##KIND##_##FS##_with_planner(const T *in, size_t in_len, T *out, size_t out_len, int type, int norm,      \
                                           const phast_planner_dct##SFX *p) try {                                       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(type, DST, in, in_len, out, out_len, norm);                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_##KIND##_##FS##_dev(const T *d_in, T *d_out, size_t n, size_t batch, size_t in_dist, size_t out_dist,     \
                                  int type, int norm, const phast_planner_dct##SFX *p, T *d_work, size_t work_len,      \
                                  void *stream) try {                                                                   \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(type, DST, d_in, d_out, n, batch, in_dist, out_dist, norm, d_work, work_len,                      \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_DCT_API(64, f64, double)
PHAST_DCT_API(32, f32, float)

// The short-time Fourier transform and its inverse (planner_stft.hpp): every argument rule, a wrong length and a window that
// does not overlap-add to nonzero (the inverse) come back before the device is touched
#define PHAST_STFT_API(SFX, FS, T)                                                                                      \
    int phast_planner_stft##SFX##_new(size_t signal_len, size_t n_fft, size_t hop, const T *window, int center,         \
                                      int pad_mode, phast_planner_stft##SFX **out) try {                                \
        return stft_planner_new<T>(signal_len, n_fft, hop, window, center, pad_mode, out);                              \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_stft##SFX##_frames(const phast_planner_stft##SFX *p) try {                                     \
        return p ? p->frames : 0;                                                                                       \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_stft##SFX##_bins(const phast_planner_stft##SFX *p) try {                                       \
        return p ? p->bins : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_stft##SFX##_workspace_min(const phast_planner_stft##SFX *p, int inverse) try {                 \
        return p ? p->workspace_min(inverse != 0) : 0;                                                                  \
    } PHAST_CATCH_ZERO                                                                                                  \
    double phast_planner_stft##SFX##_envelope_min(const phast_planner_stft##SFX *p) try {                               \
        return p ? p->env_min : 0.0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_stft##SFX##_time_stages(const phast_planner_stft##SFX *p, int inverse, T *d_signal, T *d_re,      \
                                              T *d_im, size_t batch, T *d_work, size_t work_len, int reps,              \
                                              float *stage_ms, void *stream) try {                                      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(inverse != 0, d_signal, d_re, d_im, batch, d_work, work_len, reps, stage_ms,              \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_stft_##FS##_with_planner(const T *signal, size_t signal_len, T *ore, size_t ore_len, T *oim,              \
                                       size_t oim_len, const phast_planner_stft##SFX *p) try {                          \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(false, signal, signal_len, nullptr, 0, ore, ore_len, oim, oim_len);                              \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_istft_##FS##_with_planner(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *signal,          \
                                        size_t signal_len, const phast_planner_stft##SFX *p) try {                      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(true, ire, ire_len, iim, iim_len, signal, signal_len, nullptr, 0);                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_stft_##FS##_dev(const T *d_signal, T *d_re, T *d_im, size_t signal_len, size_t batch, size_t sig_dist,    \
                              const phast_planner_stft##SFX *p, T *d_work, size_t work_len, void *stream) try {         \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->stft_dev(d_signal, d_re, d_im, signal_len, batch, sig_dist, d_work, work_len,                         \
                           static_cast<hipStream_t>(stream));                                                           \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_istft_##FS##_dev(const T *d_re, const T *d_im, T *d_signal, size_t signal_len, size_t batch,              \
                               size_t sig_dist, const phast_planner_stft##SFX *p, T *d_work, size_t work_len,           \
                               void *stream) try {                                                                      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->istft_dev(d_re, d_im, d_signal, signal_len, batch, sig_dist, d_work, work_len,                        \
                            static_cast<hipStream_t>(stream));                                                          \
    } PHAST_CATCH_RC
PHAST_STFT_API(64, f64, double)
PHAST_STFT_API(32, f32, float)

// The MDCT and its inverse (planner_mdct.hpp): every argument rule and a wrong length come back before the device is touched
#define PHAST_MDCT_API(SFX, FS, T)                                                                                      \
    int phast_planner_mdct##SFX##_new(size_t signal_len, size_t n, const T *window, int padded,                         \
                                      phast_planner_mdct##SFX **out) try {                                              \
        return mdct_planner_new<T>(signal_len, n, window, padded, out);                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_mdct##SFX##_frames(const phast_planner_mdct##SFX *p) try {                                     \
        return p ? p->frames : 0;                                                                                       \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_mdct##SFX##_workspace_min(const phast_planner_mdct##SFX *p, int inverse) try {                 \
        return p ? p->workspace_min(inverse != 0) : 0;                                                                  \
    } PHAST_CATCH_ZERO                                                                                                  \
    double phast_planner_mdct##SFX##_tdac_defect(const phast_planner_mdct##SFX *p) try {                                \
        return p ? p->tdac_defect : 0.0;                                                                                \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_mdct##SFX##_time_stages(const phast_planner_mdct##SFX *p, int inverse, T *d_signal, T *d_coefs,   \
                                              size_t batch, T *d_work, size_t work_len, int reps, float *stage_ms,      \
                                              void *stream) try {                                                       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(inverse != 0, d_signal, d_coefs, batch, d_work, work_len, reps, stage_ms,                 \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_mdct_##FS##_with_planner(const T *signal, size_t signal_len, T *coefs, size_t coefs_len,                  \
                                       const phast_planner_mdct##SFX *p) try {                                          \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(false, signal, signal_len, coefs, coefs_len);                                                    \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_imdct_##FS##_with_planner(const T *coefs, size_t coefs_len, T *signal, size_t signal_len,                 \
                                        const phast_planner_mdct##SFX *p) try {                                         \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(true, coefs, coefs_len, signal, signal_len);                                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_mdct_##FS##_dev(const T *d_signal, T *d_coefs, size_t signal_len, size_t batch, size_t sig_dist,          \
                              const phast_planner_mdct##SFX *p, T *d_work, size_t work_len, void *stream) try {         \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->mdct_dev(d_signal, d_coefs, signal_len, batch, sig_dist, d_work, work_len,                            \
                           static_cast<hipStream_t>(stream));                                                           \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_imdct_##FS##_dev(const T *d_coefs, T *d_signal, size_t signal_len, size_t batch, size_t sig_dist,         \
                               const phast_planner_mdct##SFX *p, T *d_work, size_t work_len, void *stream) try {        \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->imdct_dev(d_coefs, d_signal, signal_len, batch, sig_dist, d_work, work_len,                           \
                            static_cast<hipStream_t>(stream));                                                          \
    } PHAST_CATCH_RC
PHAST_MDCT_API(64, f64, double)
PHAST_MDCT_API(32, f32, float)

// Welch spectral estimation (planner_psd.hpp): every argument rule and a wrong length come back before the device is touched
#define PHAST_PSD_API(SFX, FS, T)                                                                                       \
    int phast_planner_psd##SFX##_new(size_t signal_len, size_t nperseg, size_t hop, size_t nfft, const double *window,  \
                                     int detrend, int scaling, double fs, phast_planner_psd##SFX **out) try {           \
        return psd_planner_new<T>(signal_len, nperseg, hop, nfft, window, detrend, scaling, fs, out);                   \
    } PHAST_CATCH_RC                                                                                                    \
    void phast_planner_psd##SFX##_free(phast_planner_psd##SFX *p) try { delete p; } PHAST_CATCH_VOID                    \
    int phast_planner_psd##SFX##_describe(const phast_planner_psd##SFX *p, char *buf, size_t len) try {                 \
        if (!p || !buf || !len) return PHAST_ERR_INVALID_ARG;                                                           \
        std::snprintf(buf, len, "%s", p->describe().c_str());                                                           \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_psd##SFX##_device_bytes(const phast_planner_psd##SFX *p) try {                                 \
        return p ? p->device_bytes() : 0;                                                                               \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_psd##SFX##_segments(const phast_planner_psd##SFX *p) try {                                     \
        return p ? p->frames : 0;                                                                                       \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_psd##SFX##_bins(const phast_planner_psd##SFX *p) try {                                         \
        return p ? p->bins : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_psd##SFX##_slab(const phast_planner_psd##SFX *p) try {                                         \
        return p ? p->q : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_psd##SFX##_workspace_len(const phast_planner_psd##SFX *p, size_t batch, int cross) try {       \
        return p ? p->workspace_len(batch, cross != 0) : 0;                                                             \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_psd##SFX##_workspace_min(const phast_planner_psd##SFX *p, int cross) try {                     \
        return p ? p->workspace_min(cross != 0) : 0;                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_psd##SFX##_time_stages(const phast_planner_psd##SFX *p, T *d_signal, T *d_out, size_t batch,      \
                                             int average, size_t slab, T *d_work, size_t work_len, int reps,            \
                                             float *stage_ms, void *stream) try {                                       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_signal, d_out, batch, average, slab, d_work, work_len, reps, stage_ms,                  \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_psd_##FS##_with_planner(const T *signal, size_t signal_len, T *out, size_t out_len, int average,          \
                                      const phast_planner_psd##SFX *p) try {                                            \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        T *o[4] = {out, nullptr, nullptr, nullptr};                                                                     \
        const size_t n[4] = {out_len, 0, 0, 0};                                                                         \
        return p->host(signal, signal_len, nullptr, 0, o, n, average);                                                  \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_csd_##FS##_with_planner(const T *x, size_t x_len, const T *y, size_t y_len, T *out_re, size_t re_len,     \
                                      T *out_im, size_t im_len, T *pxx, size_t pxx_len, T *pyy, size_t pyy_len,         \
                                      int average, const phast_planner_psd##SFX *p) try {                               \
        if (!p || !y) return PHAST_ERR_INVALID_ARG;                                                                     \
        T *o[4] = {out_re, out_im, pxx, pyy};                                                                           \
        const size_t n[4] = {re_len, im_len, pxx_len, pyy_len};                                                         \
        return p->host(x, x_len, y, y_len, o, n, average);                                                              \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_psd_##FS##_dev(const T *d_x, T *d_out, size_t signal_len, size_t batch, size_t sig_dist, int average,     \
                             const phast_planner_psd##SFX *p, T *d_work, size_t work_len, void *stream) try {           \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        T *o[4] = {d_out, nullptr, nullptr, nullptr};                                                                   \
        return p->run(d_x, nullptr, o, signal_len, batch, sig_dist, average, d_work, work_len,                          \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_csd_##FS##_dev(const T *d_x, const T *d_y, T *d_out_re, T *d_out_im, T *d_pxx, T *d_pyy,                  \
                             size_t signal_len, size_t batch, size_t sig_dist, int average,                             \
                             const phast_planner_psd##SFX *p, T *d_work, size_t work_len, void *stream) try {           \
        if (!p || !d_y) return PHAST_ERR_INVALID_ARG;                                                                   \
        T *o[4] = {d_out_re, d_out_im, d_pxx, d_pyy};                                                                   \
        return p->run(d_x, d_y, o, signal_len, batch, sig_dist, average, d_work, work_len,                              \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_PSD_API(64, f64, double)
PHAST_PSD_API(32, f32, float)

// The Lomb-Scargle periodogram (planner_lomb.hpp): the counts, the values, eps and both type-3 grids are checked before the
// device is touched; the one-shot form builds a planner of its own for the call.
#define PHAST_LOMB_API(SFX, FS, T)                                                                                      \
    int phast_planner_lomb##SFX##_new(const double *t, size_t m, const double *freqs, size_t k, const double *weights,  \
                                      int floating_mean, double eps, phast_planner_lomb##SFX **out) try {               \
        return lomb_planner_new<T>(t, m, freqs, k, weights, floating_mean, eps, out);                                   \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_lomb##SFX##_workspace_min(const phast_planner_lomb##SFX *p) try {                              \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_lomb##SFX##_slab(const phast_planner_lomb##SFX *p) try {                                       \
        return p ? p->q : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_lomb##SFX##_grid_len(const phast_planner_lomb##SFX *p) try {                                   \
        return p ? (size_t)p->t3.grid.nf : 0;                                                                           \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_lomb##SFX##_time_stages(const phast_planner_lomb##SFX *p, const T *d_y, T *d_out_re, T *d_out_im, \
                                              size_t batch, int normalize, T *d_work, size_t work_len, int reps,        \
                                              float *stage_ms, void *stream) try {                                      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_y, d_out_re, d_out_im, batch, normalize, d_work, work_len, reps, stage_ms,              \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_lombscargle_##FS(const double *t, size_t m, const double *freqs, size_t k, const double *weights,         \
                               int floating_mean, double eps, const T *y, T *out_re, T *out_im, int normalize) try {    \
        phast_planner_lomb##SFX *p = nullptr;                                                                           \
        int rc = lomb_planner_new<T>(t, m, freqs, k, weights, floating_mean, eps, &p);                                  \
        if (rc) return rc;                                                                                              \
        std::unique_ptr<phast_planner_lomb##SFX> own(p);                                                                \
        return p->host(y, m, out_re, k, out_im, k, normalize);                                                          \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_lombscargle_##FS##_with_planner(const T *y, size_t m, T *out_re, size_t re_len, T *out_im, size_t im_len, \
                                              int normalize, const phast_planner_lomb##SFX *p) try {                    \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(y, m, out_re, re_len, out_im, im_len, normalize);                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_lombscargle_##FS##_dev(const T *d_y, T *d_out_re, T *d_out_im, size_t m, size_t batch, size_t sig_dist,   \
                                     size_t out_dist, int normalize, const phast_planner_lomb##SFX *p, T *d_work,       \
                                     size_t work_len, void *stream) try {                                               \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->run(d_y, d_out_re, d_out_im, m, batch, sig_dist, out_dist, normalize, d_work, work_len,               \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_LOMB_API(64, f64, double)
PHAST_LOMB_API(32, f32, float)

// Sample-rate conversion (planner_resample.hpp): the polyphase FIR and the Fourier method; every argument rule and a wrong
// length come back before the device is touched
#define PHAST_RESAMPLE_API(SFX, FS, T)                                                                                  \
    int phast_planner_upfirdn##SFX##_new(size_t signal_len, const T *taps, size_t num_taps, size_t up, size_t down,     \
                                         size_t first, size_t out_len, phast_planner_upfirdn##SFX **out) try {          \
        return upfirdn_planner_new<T>(signal_len, taps, num_taps, up, down, first, out_len, out);                       \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_upfirdn##SFX##_out_len(const phast_planner_upfirdn##SFX *p) try {                              \
        return p ? p->out_len : 0;                                                                                      \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_upfirdn##SFX##_full_len(const phast_planner_upfirdn##SFX *p) try {                             \
        return p ? p->full_len : 0;                                                                                     \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_upfirdn##SFX##_tile(const phast_planner_upfirdn##SFX *p) try {                                 \
        return p ? p->geom.tile : 0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_upfirdn##SFX##_chunk(const phast_planner_upfirdn##SFX *p) try {                                \
        return p ? p->geom.jc : 0;                                                                                      \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_upfirdn##SFX##_time_stages(const phast_planner_upfirdn##SFX *p, const T *d_signal, T *d_out,      \
                                                 size_t batch, int reps, float *stage_ms, void *stream) try {           \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_signal, d_out, batch, reps, stage_ms, static_cast<hipStream_t>(stream));                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_upfirdn_##FS##_with_planner(const T *signal, size_t signal_len, T *out, size_t out_len,                   \
                                          const phast_planner_upfirdn##SFX *p) try {                                    \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(signal, signal_len, out, out_len);                                                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_upfirdn_##FS##_dev(const T *d_signal, T *d_out, size_t signal_len, size_t batch, size_t sig_dist,         \
                                 size_t out_dist, const phast_planner_upfirdn##SFX *p, T *, size_t, void *stream) try { \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_signal, d_out, signal_len, batch, sig_dist, out_dist, static_cast<hipStream_t>(stream));        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_resample##SFX##_new(size_t signal_len, size_t num, phast_planner_resample##SFX **out) try {       \
        return resample_planner_new<T>(signal_len, num, out);                                                           \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_resample##SFX##_workspace_min(const phast_planner_resample##SFX *p) try {                      \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_resample##SFX##_time_stages(const phast_planner_resample##SFX *p, const T *d_signal, T *d_out,    \
                                                  size_t batch, T *d_work, size_t work_len, int reps, float *stage_ms,  \
                                                  void *stream) try {                                                   \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_signal, d_out, batch, d_work, work_len, reps, stage_ms,                                 \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_resample_##FS##_with_planner(const T *signal, size_t signal_len, T *out, size_t out_len,                  \
                                           const phast_planner_resample##SFX *p) try {                                  \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(signal, signal_len, out, out_len);                                                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_resample_##FS##_dev(const T *d_signal, T *d_out, size_t signal_len, size_t batch, size_t sig_dist,        \
                                  size_t out_dist, const phast_planner_resample##SFX *p, T *d_work, size_t work_len,    \
                                  void *stream) try {                                                                   \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_signal, d_out, signal_len, batch, sig_dist, out_dist, d_work, work_len,                         \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_RESAMPLE_API(64, f64, double)
PHAST_RESAMPLE_API(32, f32, float)

// The discrete wavelet transform (planner_dwt.hpp): every argument rule, a wrong length, a short distance or workspace come
// back before the device is touched
#define PHAST_DWT_API(SFX, FS, T)                                                                                       \
    int phast_planner_dwt##SFX##_new(size_t signal_len, const T *dec_lo, const T *dec_hi, const T *rec_lo,              \
                                     const T *rec_hi, size_t filter_len, size_t level, int mode,                        \
                                     phast_planner_dwt##SFX **out) try {                                                \
        return dwt_planner_new<T>(signal_len, dec_lo, dec_hi, rec_lo, rec_hi, filter_len, level, mode, out);            \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_dwt##SFX##_workspace_min(const phast_planner_dwt##SFX *p) try {                                \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_dwt##SFX##_coeff_len(const phast_planner_dwt##SFX *p) try {                                    \
        return p ? p->coeff_len() : 0;                                                                                  \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_dwt##SFX##_level_len(const phast_planner_dwt##SFX *p, size_t level) try {                      \
        return p ? p->level_len(level) : 0;                                                                             \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_dwt##SFX##_level_offset(const phast_planner_dwt##SFX *p, size_t level) try {                   \
        return p ? p->level_offset(level) : 0;                                                                          \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_dwt##SFX##_tile(const phast_planner_dwt##SFX *p) try {                                         \
        return p ? p->geom.tile : 0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_dwt##SFX##_time_stages(const phast_planner_dwt##SFX *p, T *d_signal, T *d_coeffs, size_t batch,   \
                                             T *d_work, size_t work_len, int reps, float *stage_ms, void *stream) try { \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_signal, d_coeffs, batch, d_work, work_len, reps, stage_ms,                              \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_wavedec_##FS##_with_planner(const T *signal, size_t signal_len, T *coeffs, size_t coeff_len,              \
                                          const phast_planner_dwt##SFX *p) try {                                        \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(false, signal, signal_len, coeffs, coeff_len);                                                   \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_waverec_##FS##_with_planner(const T *coeffs, size_t coeff_len, T *signal, size_t signal_len,              \
                                          const phast_planner_dwt##SFX *p) try {                                        \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(true, coeffs, coeff_len, signal, signal_len);                                                    \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_wavedec_##FS##_dev(const T *d_signal, T *d_coeffs, size_t signal_len, size_t batch, size_t sig_dist,      \
                                 size_t coeff_dist, const phast_planner_dwt##SFX *p, T *d_work, size_t work_len,        \
                                 void *stream) try {                                                                    \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(false, const_cast<T *>(d_signal), d_coeffs, signal_len, batch, sig_dist, coeff_dist, d_work,      \
                      work_len, static_cast<hipStream_t>(stream));                                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_waverec_##FS##_dev(const T *d_coeffs, T *d_signal, size_t signal_len, size_t batch, size_t coeff_dist,    \
                                 size_t sig_dist, const phast_planner_dwt##SFX *p, T *d_work, size_t work_len,          \
                                 void *stream) try {                                                                    \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(true, d_signal, const_cast<T *>(d_coeffs), signal_len, batch, sig_dist, coeff_dist, d_work,       \
                      work_len, static_cast<hipStream_t>(stream));                                                      \
    } PHAST_CATCH_RC
PHAST_DWT_API(64, f64, double)
PHAST_DWT_API(32, f32, float)

// The polyphase filter-bank channelizer (planner_channelizer.hpp): every argument rule, a wrong length and a signal whose
// planes do not match the planner come back before the device is touched
#define PHAST_CHANNELIZER_API(SFX, FS, T)                                                                               \
    int phast_planner_channelizer##SFX##_new(size_t signal_len, const T *taps, size_t num_taps, size_t channels,        \
                                             size_t hop, size_t first_frame, size_t out_frames, int complex_input,      \
                                             phast_planner_channelizer##SFX **out) try {                                \
        return channelizer_planner_new<T>(signal_len, taps, num_taps, channels, hop, first_frame, out_frames,           \
                                          complex_input, out);                                                          \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_channelizer##SFX##_workspace_min(const phast_planner_channelizer##SFX *p) try {                \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_out_frames(const phast_planner_channelizer##SFX *p) try {                   \
        return p ? p->out_frames : 0;                                                                                   \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_full_frames(const phast_planner_channelizer##SFX *p) try {                  \
        return p ? p->full_frames : 0;                                                                                  \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_bins(const phast_planner_channelizer##SFX *p) try {                         \
        return p ? p->bins : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_tile_frames(const phast_planner_channelizer##SFX *p) try {                  \
        return p ? p->geom.frames : 0;                                                                                  \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_tile_cols(const phast_planner_channelizer##SFX *p) try {                    \
        return p ? p->geom.cols : 0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_chunk(const phast_planner_channelizer##SFX *p) try {                        \
        return p ? p->geom.jc : 0;                                                                                      \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_channelizer##SFX##_periods(const phast_planner_channelizer##SFX *p) try {                      \
        return p ? p->geom.rows : 0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_channelizer##SFX##_time_stages(const phast_planner_channelizer##SFX *p, const T *d_sig_re,        \
                                                     const T *d_sig_im, T *d_out_re, T *d_out_im, size_t batch,         \
                                                     T *d_work, size_t work_len, int reps, float *stage_ms,             \
                                                     void *stream) try {                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_sig_re, d_sig_im, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,          \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_channelize_##FS##_with_planner(const T *sig_re, const T *sig_im, size_t signal_len, T *out_re, T *out_im, \
                                             size_t out_len, const phast_planner_channelizer##SFX *p) try {             \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(sig_re, sig_im, signal_len, out_re, out_im, out_len);                                            \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_channelize_##FS##_dev(const T *d_sig_re, const T *d_sig_im, T *d_out_re, T *d_out_im, size_t signal_len,  \
                                    size_t batch, size_t sig_dist, const phast_planner_channelizer##SFX *p, T *d_work,  \
                                    size_t work_len, void *stream) try {                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_sig_re, d_sig_im, d_out_re, d_out_im, signal_len, batch, sig_dist, d_work, work_len,            \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_CHANNELIZER_API(64, f64, double)
PHAST_CHANNELIZER_API(32, f32, float)

// The polyphase synthesis filter bank (planner_synthesizer.hpp): every argument rule, a wrong length and an output whose
// planes do not match the planner come back before the device is touched
#define PHAST_SYNTHESIZER_API(SFX, FS, T)                                                                               \
    int phast_planner_synthesizer##SFX##_new(size_t frames, const T *taps, size_t num_taps, size_t channels, size_t hop, \
                                             size_t first, size_t out_len, int complex_output,                          \
                                             phast_planner_synthesizer##SFX **out) try {                                \
        return synthesizer_planner_new<T>(frames, taps, num_taps, channels, hop, first, out_len, complex_output, out);  \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_synthesizer##SFX##_workspace_min(const phast_planner_synthesizer##SFX *p) try {                \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_synthesizer##SFX##_out_len(const phast_planner_synthesizer##SFX *p) try {                      \
        return p ? p->out_len : 0;                                                                                      \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_synthesizer##SFX##_full_len(const phast_planner_synthesizer##SFX *p) try {                     \
        return p ? p->full_len : 0;                                                                                     \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_synthesizer##SFX##_bins(const phast_planner_synthesizer##SFX *p) try {                         \
        return p ? p->bins : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_synthesizer##SFX##_tile_samples(const phast_planner_synthesizer##SFX *p) try {                 \
        return p ? p->geom.tile : 0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_synthesizer##SFX##_per_thread(const phast_planner_synthesizer##SFX *p) try {                   \
        return p ? p->geom.per : 0;                                                                                     \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_synthesizer##SFX##_max_terms(const phast_planner_synthesizer##SFX *p) try {                    \
        return p ? p->geom.terms : 0;                                                                                   \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_synthesizer##SFX##_time_stages(const phast_planner_synthesizer##SFX *p, const T *d_in_re,         \
                                                     const T *d_in_im, T *d_out_re, T *d_out_im, size_t batch,          \
                                                     T *d_work, size_t work_len, int reps, float *stage_ms,             \
                                                     void *stream) try {                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_in_re, d_in_im, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,            \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_synthesize_##FS##_with_planner(const T *in_re, const T *in_im, size_t in_len, T *out_re, T *out_im,       \
                                             size_t out_len, const phast_planner_synthesizer##SFX *p) try {             \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(in_re, in_im, in_len, out_re, out_im, out_len);                                                  \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_synthesize_##FS##_dev(const T *d_in_re, const T *d_in_im, T *d_out_re, T *d_out_im, size_t frames,        \
                                    size_t batch, size_t out_dist, const phast_planner_synthesizer##SFX *p, T *d_work,  \
                                    size_t work_len, void *stream) try {                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_in_re, d_in_im, d_out_re, d_out_im, frames, batch, out_dist, d_work, work_len,                  \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_SYNTHESIZER_API(64, f64, double)
PHAST_SYNTHESIZER_API(32, f32, float)

// The continuous wavelet transform (planner_cwt.hpp): every argument rule, a wrong length and planes that do not match the
// planner come back before the device is touched
#define PHAST_CWT_API(SFX, T)                                                                                           \
    int phast_planner_cwt##SFX##_new(size_t signal_len, size_t pad_len, const double *scales, size_t num_scales,        \
                                     int family, double param, int norm, int real_input,                                \
                                     phast_planner_cwt##SFX **out) try {                                                \
        return cwt_planner_new<T>(signal_len, pad_len, scales, num_scales, family, param, norm, real_input, out);       \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_cwt##SFX##_workspace_min(const phast_planner_cwt##SFX *p) try {                                \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_cwt##SFX##_pad_len(const phast_planner_cwt##SFX *p) try {                                      \
        return p ? p->p : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_cwt##SFX##_num_scales(const phast_planner_cwt##SFX *p) try {                                   \
        return p ? p->s : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_cwt##SFX##_tile_bins(const phast_planner_cwt##SFX *p) try {                                    \
        return p ? p->geom.tile : 0;                                                                                    \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_cwt##SFX##_scale_group(const phast_planner_cwt##SFX *p) try {                                  \
        return p ? p->geom.group : 0;                                                                                   \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_cwt##SFX##_time_stages(const phast_planner_cwt##SFX *p, const T *d_x_re, const T *d_x_im,         \
                                             T *d_out_re, T *d_out_im, size_t batch, T *d_work, size_t work_len,        \
                                             int reps, float *stage_ms, void *stream) try {                             \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_x_re, d_x_im, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,              \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_cwt_##SFX##_with_planner(const T *x_re, const T *x_im, size_t x_len, T *out_re, T *out_im,                \
                                       size_t out_len, const phast_planner_cwt##SFX *p) try {                           \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(x_re, x_im, x_len, out_re, out_im, out_len);                                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_cwt_##SFX##_dev(const T *d_x_re, const T *d_x_im, T *d_out_re, T *d_out_im, size_t signal_len,            \
                              size_t batch, size_t sig_dist, size_t out_dist, const phast_planner_cwt##SFX *p,          \
                              T *d_work, size_t work_len, void *stream) try {                                           \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_x_re, d_x_im, d_out_re, d_out_im, signal_len, batch, sig_dist, out_dist, d_work, work_len,      \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_CWT_API(64, double)
PHAST_CWT_API(32, float)

// Overlap-save convolution and correlation of real signals (planner_conv.hpp): every argument rule and a wrong length come
// back before the device is touched
#define PHAST_CONV_API(SFX, FS, T)                                                                                      \
    int phast_planner_conv##SFX##_new(size_t signal_len, const T *taps, size_t num_taps, int mode, int flip,            \
                                      size_t block, phast_planner_conv##SFX **out) try {                                \
        return conv_planner_new<T>(signal_len, taps, num_taps, mode, flip, block, out);                                 \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_conv##SFX##_out_len(const phast_planner_conv##SFX *p) try {                                    \
        return p ? p->out_len : 0;                                                                                      \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_conv##SFX##_block(const phast_planner_conv##SFX *p) try {                                      \
        return p ? p->b : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_conv##SFX##_segments(const phast_planner_conv##SFX *p) try {                                   \
        return p ? p->segs : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_conv##SFX##_workspace_min(const phast_planner_conv##SFX *p) try {                              \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_conv##SFX##_time_stages(const phast_planner_conv##SFX *p, const T *d_signal, T *d_out,            \
                                              size_t batch, T *d_work, size_t work_len, int reps, float *stage_ms,      \
                                              void *stream) try {                                                       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_signal, d_out, batch, d_work, work_len, reps, stage_ms,                                 \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_conv_##FS##_with_planner(const T *signal, size_t signal_len, T *out, size_t out_len,                      \
                                       const phast_planner_conv##SFX *p) try {                                          \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(signal, signal_len, out, out_len);                                                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_conv_##FS##_dev(const T *d_signal, T *d_out, size_t signal_len, size_t batch, size_t sig_dist,            \
                              size_t out_dist, const phast_planner_conv##SFX *p, T *d_work, size_t work_len,            \
                              void *stream) try {                                                                       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_signal, d_out, signal_len, batch, sig_dist, out_dist, d_work, work_len,                         \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_CONV_API(64, f64, double)
PHAST_CONV_API(32, f32, float)

// Overlap-save convolution and correlation of real arrays of rank 1 .. 3 (planner_convnd.hpp): every argument rule and a wrong
// length come back before the device is touched
#define PHAST_CONVND_API(SFX, FS, T)                                                                                    \
    int phast_planner_convnd##SFX##_new(const size_t *signal_dims, const size_t *tap_dims, size_t rank, const T *taps,  \
                                        int mode, int flip, const size_t *block, phast_planner_convnd##SFX **out) try { \
        return convnd_planner_new<T>(signal_dims, tap_dims, rank, taps, mode, flip, block, out);                        \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_convnd##SFX##_out_len(const phast_planner_convnd##SFX *p) try {                                \
        return p ? p->out_pts : 0;                                                                                      \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_convnd##SFX##_out_dims(const phast_planner_convnd##SFX *p, size_t *dims, size_t rank) try {       \
        if (!p || !dims || rank != p->rank) return PHAST_ERR_INVALID_ARG;                                               \
        p->out_dims(dims);                                                                                              \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_convnd##SFX##_block(const phast_planner_convnd##SFX *p, size_t *dims, size_t rank) try {          \
        if (!p || !dims || rank != p->rank) return PHAST_ERR_INVALID_ARG;                                               \
        p->block(dims);                                                                                                 \
        return PHAST_OK;                                                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_convnd##SFX##_tiles(const phast_planner_convnd##SFX *p) try {                                  \
        return p ? p->tiles : 0;                                                                                        \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_convnd##SFX##_workspace_min(const phast_planner_convnd##SFX *p) try {                          \
        return p ? p->workspace_min() : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_convnd##SFX##_time_stages(const phast_planner_convnd##SFX *p, const T *d_signal, T *d_out,        \
                                                size_t batch, T *d_work, size_t work_len, int reps, float *stage_ms,    \
                                                void *stream) try {                                                     \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_signal, d_out, batch, d_work, work_len, reps, stage_ms,                                 \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_convnd_##FS##_with_planner(const T *signal, size_t signal_len, T *out, size_t out_len,                    \
                                         const phast_planner_convnd##SFX *p) try {                                      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(signal, signal_len, out, out_len);                                                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_convnd_##FS##_dev(const T *d_signal, T *d_out, size_t signal_len, size_t batch, size_t sig_dist,          \
                                size_t out_dist, const phast_planner_convnd##SFX *p, T *d_work, size_t work_len,        \
                                void *stream) try {                                                                     \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(d_signal, d_out, signal_len, batch, sig_dist, out_dist, d_work, work_len,                         \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_CONVND_API(64, f64, double)
PHAST_CONVND_API(32, f32, float)

// The chirp-Z transform on the unit circle (planner_czt.hpp): the lengths and the two doubles are checked before the device
// is touched; the one-shot form builds a planner of its own for the call
#define PHAST_CZT_API(SFX, T)                                                                                           \
    int phast_planner_czt##SFX##_new(size_t n, size_t m, double step, double start, phast_planner_czt##SFX **out) try { \
        return czt_planner_new(n, m, step, start, out);                                                                 \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_czt##SFX##_conv_len(const phast_planner_czt##SFX *p) try {                                     \
        return p ? p->m : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_czt##SFX##_time_stages(const phast_planner_czt##SFX *p, const T *d_in_re, const T *d_in_im,       \
                                             T *d_out_re, T *d_out_im, size_t batch, T *d_work, size_t work_len,        \
                                             int reps, float *stage_ms, void *stream) try {                             \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_in_re, d_in_im, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,            \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_czt_##SFX(const T *in_re, const T *in_im, size_t n, T *out_re, T *out_im, size_t m, double step,          \
                        double start) try {                                                                             \
        if (!in_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;                                                 \
        phast_planner_czt##SFX *p = nullptr;                                                                            \
        int rc = czt_planner_new(n, m, step, start, &p);                                                                \
        if (rc) return rc;                                                                                              \
        std::unique_ptr<phast_planner_czt##SFX> own(p);                                                                 \
        return p->czt_host(in_re, in_im, n, out_re, out_im, m);                                                         \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_czt_##SFX##_with_planner(const T *in_re, const T *in_im, size_t n, T *out_re, T *out_im, size_t m,        \
                                       const phast_planner_czt##SFX *p) try {                                           \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->czt_host(in_re, in_im, n, out_re, out_im, m);                                                         \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_czt_##SFX##_dev(const T *d_in_re, const T *d_in_im, size_t in_dist, T *d_out_re, T *d_out_im,             \
                              size_t out_dist, size_t batch, const phast_planner_czt##SFX *p, T *d_work,                \
                              size_t work_len, void *stream) try {                                                      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->czt_dev(d_in_re, d_in_im, p->n, in_dist, d_out_re, d_out_im, p->bins, out_dist, batch, d_work,        \
                          work_len, static_cast<hipStream_t>(stream));                                                  \
    } PHAST_CATCH_RC
PHAST_CZT_API(64, double)
PHAST_CZT_API(32, float)

// Non-uniform FFTs of types 1 and 2 (planner_nufft.hpp, planner_nufft_nd.hpp): the lengths, eps and the points are checked before
// the device is touched; the one-shot forms build a planner of their own for the call.  TYPE 1: points -> modes, 2: modes ->
// points.  What lists neither coordinates nor mode counts is the same for every rank: H = nufft, nufft2d, nufft3d
#define PHAST_NUFFT_RANK_CALLS(H, SFX, T, TYPE)                                                                         \
    int phast_##H##TYPE##_##SFX##_with_planner(const T *in_re, const T *in_im, size_t in_len, T *out_re, T *out_im,     \
                                               size_t out_len, int direction, const phast_planner_##H##SFX *p) try {    \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->nufft_host(TYPE, direction, in_re, in_im, in_len, out_re, out_im, out_len);                           \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_##H##TYPE##_##SFX##_dev(const T *d_in_re, const T *d_in_im, size_t in_dist, T *d_out_re, T *d_out_im,     \
                                      size_t out_dist, size_t batch, int direction, const phast_planner_##H##SFX *p,    \
                                      T *d_work, size_t work_len, void *stream) try {                                   \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->nufft_dev(TYPE, direction, d_in_re, d_in_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work,    \
                            work_len, static_cast<hipStream_t>(stream));                                                \
    } PHAST_CATCH_RC
#define PHAST_NUFFT_RANK_API(H, SFX, T)                                                                                 \
    size_t phast_planner_##H##SFX##_grid_len(const phast_planner_##H##SFX *p) try {                                     \
        return p ? p->grid_len() : 0;                                                                                   \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_##H##SFX##_width(const phast_planner_##H##SFX *p) try {                                           \
        return p ? p->w : 0;                                                                                            \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_##H##SFX##_time_stages(const phast_planner_##H##SFX *p, const T *d_in_re, const T *d_in_im,       \
                                             T *d_out_re, T *d_out_im, int type, size_t batch, T *d_work,               \
                                             size_t work_len, int reps, float *stage_ms, void *stream) try {            \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(type, d_in_re, d_in_im, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,      \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    PHAST_NUFFT_RANK_CALLS(H, SFX, T, 1)                                                                                \
    PHAST_NUFFT_RANK_CALLS(H, SFX, T, 2)
// the body of every rank's one-shot form: NEW builds the planner p
#define PHAST_NUFFT_ONE_SHOT(H, SFX, TYPE, NEW)                                                                         \
    if (!in_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;                                                     \
    phast_planner_##H##SFX *p = nullptr;                                                                                \
    int rc = NEW;                                                                                                       \
    if (rc) return rc;                                                                                                  \
    std::unique_ptr<phast_planner_##H##SFX> own(p);                                                                     \
    return p->nufft_host(TYPE, direction, in_re, in_im, p->in_len(TYPE), out_re, out_im, p->out_len(TYPE));

// one dimension
#define PHAST_NUFFT_CALLS(SFX, T, TYPE)                                                                                 \
    int phast_nufft##TYPE##_##SFX(const double *x_turns, size_t m_points, const T *in_re, const T *in_im, T *out_re,    \
                                  T *out_im, size_t n_modes, double eps, int direction) try {                           \
        PHAST_NUFFT_ONE_SHOT(nufft, SFX, TYPE, nufft_planner_new(n_modes, x_turns, m_points, eps, sizeof(T) == 4, &p))  \
    } PHAST_CATCH_RC
#define PHAST_NUFFT_API(SFX, T)                                                                                         \
    int phast_planner_nufft##SFX##_new(size_t n_modes, const double *x_turns, size_t m_points, double eps,              \
                                       phast_planner_nufft##SFX **out) try {                                            \
        return nufft_planner_new(n_modes, x_turns, m_points, eps, sizeof(T) == 4, out);                                 \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft##SFX##_new_dev(size_t n_modes, const double *d_x_turns, size_t m_points, double eps,        \
                                           void *stream, phast_planner_nufft##SFX **out) try {                          \
        return nufft_planner_new_dev(n_modes, d_x_turns, m_points, eps, sizeof(T) == 4,                                 \
                                     static_cast<hipStream_t>(stream), out);                                            \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft##SFX##_set_points_dev(phast_planner_nufft##SFX *p, const double *d_x_turns,                 \
                                                  size_t m_points, void *stream) try {                                  \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->set_points_dev(d_x_turns, m_points, static_cast<hipStream_t>(stream));                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft##SFX##_time_set_points(phast_planner_nufft##SFX *p, const double *d_x_turns,                \
                                                   size_t m_points, float *stage_ms, void *stream) try {                \
        if (!p || !stage_ms) return PHAST_ERR_INVALID_ARG;                                                              \
        return p->set_points_dev(d_x_turns, m_points, static_cast<hipStream_t>(stream), stage_ms);                      \
    } PHAST_CATCH_RC                                                                                                    \
    PHAST_NUFFT_RANK_API(nufft, SFX, T)                                                                                 \
    PHAST_NUFFT_CALLS(SFX, T, 1)                                                                                        \
    PHAST_NUFFT_CALLS(SFX, T, 2)
PHAST_NUFFT_API(64, double)
PHAST_NUFFT_API(32, float)

// two dimensions: the same rules, (n1, n2) where the 1-D forms have n_modes and (x, y) where they have x
#define PHAST_NUFFT2D_CALLS(SFX, T, TYPE)                                                                               \
    int phast_nufft2d##TYPE##_##SFX(const double *x_turns, const double *y_turns, size_t m_points, const T *in_re,      \
                                    const T *in_im, T *out_re, T *out_im, size_t n1, size_t n2, double eps,             \
                                    int direction) try {                                                                \
        PHAST_NUFFT_ONE_SHOT(nufft2d, SFX, TYPE,                                                                        \
                             nufft_nd_planner_new({n1, n2}, {x_turns, y_turns}, m_points, eps, sizeof(T) == 4, &p))     \
    } PHAST_CATCH_RC
#define PHAST_NUFFT2D_API(SFX, T)                                                                                       \
    int phast_planner_nufft2d##SFX##_new(size_t n1, size_t n2, const double *x_turns, const double *y_turns,            \
                                         size_t m_points, double eps, phast_planner_nufft2d##SFX **out) try {           \
        return nufft_nd_planner_new({n1, n2}, {x_turns, y_turns}, m_points, eps, sizeof(T) == 4, out);                  \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft2d##SFX##_new_dev(size_t n1, size_t n2, const double *d_x_turns, const double *d_y_turns,    \
                                             size_t m_points, double eps, void *stream,                                 \
                                             phast_planner_nufft2d##SFX **out) try {                                    \
        return nufft_nd_planner_new_dev({n1, n2}, {d_x_turns, d_y_turns}, m_points, eps, sizeof(T) == 4,                \
                                        static_cast<hipStream_t>(stream), out);                                         \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft2d##SFX##_set_points_dev(phast_planner_nufft2d##SFX *p, const double *d_x_turns,             \
                                                    const double *d_y_turns, size_t m_points, void *stream) try {       \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->set_points_dev({d_x_turns, d_y_turns}, m_points, static_cast<hipStream_t>(stream));                   \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft2d##SFX##_time_set_points(phast_planner_nufft2d##SFX *p, const double *d_x_turns,            \
                                                     const double *d_y_turns, size_t m_points, float *stage_ms,         \
                                                     void *stream) try {                                                \
        if (!p || !stage_ms) return PHAST_ERR_INVALID_ARG;                                                              \
        return p->set_points_dev({d_x_turns, d_y_turns}, m_points, static_cast<hipStream_t>(stream), stage_ms);         \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_nufft2d##SFX##_grid_rows(const phast_planner_nufft2d##SFX *p) try {                            \
        return p ? p->g[0] : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    size_t phast_planner_nufft2d##SFX##_grid_cols(const phast_planner_nufft2d##SFX *p) try {                            \
        return p ? p->g[1] : 0;                                                                                         \
    } PHAST_CATCH_ZERO                                                                                                  \
    PHAST_NUFFT_RANK_API(nufft2d, SFX, T)                                                                               \
    PHAST_NUFFT2D_CALLS(SFX, T, 1)                                                                                      \
    PHAST_NUFFT2D_CALLS(SFX, T, 2)
PHAST_NUFFT2D_API(64, double)
PHAST_NUFFT2D_API(32, float)

// three dimensions: (n1, n2, n3) and (x, y, z)
#define PHAST_NUFFT3D_CALLS(SFX, T, TYPE)                                                                               \
    int phast_nufft3d##TYPE##_##SFX(const double *x_turns, const double *y_turns, const double *z_turns,                \
                                    size_t m_points, const T *in_re, const T *in_im, T *out_re, T *out_im, size_t n1,   \
                                    size_t n2, size_t n3, double eps, int direction) try {                              \
        PHAST_NUFFT_ONE_SHOT(nufft3d, SFX, TYPE,                                                                        \
                             nufft_nd_planner_new({n1, n2, n3}, {x_turns, y_turns, z_turns}, m_points, eps,             \
                                                  sizeof(T) == 4, &p))                                                  \
    } PHAST_CATCH_RC
#define PHAST_NUFFT3D_API(SFX, T)                                                                                       \
    int phast_planner_nufft3d##SFX##_new(size_t n1, size_t n2, size_t n3, const double *x_turns, const double *y_turns, \
                                         const double *z_turns, size_t m_points, double eps,                            \
                                         phast_planner_nufft3d##SFX **out) try {                                        \
        return nufft_nd_planner_new({n1, n2, n3}, {x_turns, y_turns, z_turns}, m_points, eps, sizeof(T) == 4, out);     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft3d##SFX##_new_dev(size_t n1, size_t n2, size_t n3, const double *d_x_turns,                  \
                                             const double *d_y_turns, const double *d_z_turns, size_t m_points,         \
                                             double eps, void *stream, phast_planner_nufft3d##SFX **out) try {          \
        return nufft_nd_planner_new_dev({n1, n2, n3}, {d_x_turns, d_y_turns, d_z_turns}, m_points, eps, sizeof(T) == 4, \
                                        static_cast<hipStream_t>(stream), out);                                         \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft3d##SFX##_set_points_dev(phast_planner_nufft3d##SFX *p, const double *d_x_turns,             \
                                                    const double *d_y_turns, const double *d_z_turns, size_t m_points,  \
                                                    void *stream) try {                                                 \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->set_points_dev({d_x_turns, d_y_turns, d_z_turns}, m_points, static_cast<hipStream_t>(stream));        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_planner_nufft3d##SFX##_time_set_points(phast_planner_nufft3d##SFX *p, const double *d_x_turns,            \
                                                     const double *d_y_turns, const double *d_z_turns, size_t m_points, \
                                                     float *stage_ms, void *stream) try {                               \
        if (!p || !stage_ms) return PHAST_ERR_INVALID_ARG;                                                              \
        return p->set_points_dev({d_x_turns, d_y_turns, d_z_turns}, m_points, static_cast<hipStream_t>(stream),         \
                                 stage_ms);                                                                             \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_nufft3d##SFX##_grid_dim(const phast_planner_nufft3d##SFX *p, int axis) try {                   \
        return p && axis >= 0 && axis < 3 ? p->g[axis] : 0;                                                             \
    } PHAST_CATCH_ZERO                                                                                                  \
    PHAST_NUFFT_RANK_API(nufft3d, SFX, T)                                                                               \
    PHAST_NUFFT3D_CALLS(SFX, T, 1)                                                                                      \
    PHAST_NUFFT3D_CALLS(SFX, T, 2)
PHAST_NUFFT3D_API(64, double)
PHAST_NUFFT3D_API(32, float)

// The non-uniform FFT of type 3 (planner_nufft_t3.hpp): M sources x, K target frequencies s, s x in turns.  The counts, eps,
// the points and the size of the fine grid are checked before the device is touched; the one-shot form builds a planner of
// its own for the call.
#define PHAST_NUFFT_T3_API(SFX, T)                                                                                      \
    int phast_planner_nufft_t3_##SFX##_new(const double *x, size_t m_points, const double *s, size_t k_targets,         \
                                           double eps, phast_planner_nufft_t3_##SFX **out) try {                        \
        return nufft_t3_planner_new(x, m_points, s, k_targets, eps, sizeof(T) == 4, out);                               \
    } PHAST_CATCH_RC                                                                                                    \
    size_t phast_planner_nufft_t3_##SFX##_grid_len(const phast_planner_nufft_t3_##SFX *p) try {                         \
        return p ? (size_t)p->grid.nf : 0;                                                                              \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_nufft_t3_##SFX##_width(const phast_planner_nufft_t3_##SFX *p) try {                               \
        return p ? p->grid.w : 0;                                                                                       \
    } PHAST_CATCH_ZERO                                                                                                  \
    int phast_planner_nufft_t3_##SFX##_time_stages(const phast_planner_nufft_t3_##SFX *p, const T *d_in_re,             \
                                                   const T *d_in_im, T *d_out_re, T *d_out_im, size_t batch, T *d_work, \
                                                   size_t work_len, int reps, float *stage_ms, void *stream) try {      \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_stages(d_in_re, d_in_im, d_out_re, d_out_im, batch, d_work, work_len, reps, stage_ms,            \
                              static_cast<hipStream_t>(stream));                                                        \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_nufft3_##SFX(const double *x, size_t m_points, const double *s, size_t k_targets, const T *c_re,          \
                           const T *c_im, T *out_re, T *out_im, double eps, int direction) try {                        \
        if (!c_re || !out_re || !out_im) return PHAST_ERR_INVALID_ARG;                                                  \
        phast_planner_nufft_t3_##SFX *p = nullptr;                                                                      \
        int rc = nufft_t3_planner_new(x, m_points, s, k_targets, eps, sizeof(T) == 4, &p);                              \
        if (rc) return rc;                                                                                              \
        std::unique_ptr<phast_planner_nufft_t3_##SFX> own(p);                                                           \
        return p->nufft_host(direction, c_re, c_im, m_points, out_re, out_im, k_targets);                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_nufft3_##SFX##_with_planner(const T *c_re, const T *c_im, size_t m_points, T *out_re, T *out_im,          \
                                          size_t k_targets, int direction, const phast_planner_nufft_t3_##SFX *p) try { \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->nufft_host(direction, c_re, c_im, m_points, out_re, out_im, k_targets);                               \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_nufft3_##SFX##_dev(const T *d_c_re, const T *d_c_im, size_t in_dist, T *d_out_re, T *d_out_im,            \
                                 size_t out_dist, size_t batch, int direction, const phast_planner_nufft_t3_##SFX *p,   \
                                 T *d_work, size_t work_len, void *stream) try {                                        \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->nufft_dev(direction, d_c_re, d_c_im, in_dist, d_out_re, d_out_im, out_dist, batch, d_work, work_len,  \
                            static_cast<hipStream_t>(stream));                                                          \
    } PHAST_CATCH_RC
PHAST_NUFFT_T3_API(64, double)
PHAST_NUFFT_T3_API(32, float)

// Multi-dimensional transforms (planner_nd.hpp): the shape and the lengths are checked before the device is touched
#define PHAST_ND_PLANNER_API(NAME, KIND)                                                                                \
    int phast_planner_##NAME##_new(const size_t *dims, size_t rank, phast_planner_##NAME **out) try {                   \
        return nd_planner_new(dims, rank, KIND, out);                                                                   \
    } PHAST_CATCH_RC
#define PHAST_ND_TIME_API(SFX, T)                                                                                       \
    int phast_planner_nd##SFX##_time_steps(const phast_planner_nd##SFX *p, T *d_re, T *d_im, size_t batch, size_t dist, \
                                           T *d_work, size_t work_len, int reps, float *step_ms, size_t *n_steps,       \
                                           void *stream) try {                                                          \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->time_steps(d_re, d_im, batch, dist, d_work, work_len, reps, step_ms, n_steps,                         \
                             static_cast<hipStream_t>(stream));                                                         \
    } PHAST_CATCH_RC
PHAST_ND_TIME_API(64, double)
PHAST_ND_TIME_API(32, float)
PHAST_ND_PLANNER_API(nd64, kNdC2C)
PHAST_ND_PLANNER_API(nd32, kNdC2C)
PHAST_ND_PLANNER_API(r2c_nd64, kNdR2C)
PHAST_ND_PLANNER_API(r2c_nd32, kNdR2C)

// the product of a legal shape and the half-spectrum points of its real form (0: an illegal shape)
static unsigned long long nd_points(const size_t *dims, size_t rank, unsigned long long *half_points) {
    size_t sq[kNdMaxRank];
    unsigned long long total = 0;
    int bad = 1;
    (void)nd_squeeze(dims, rank, kNdC2C, sq, &total, &bad);
    if (bad) return 0;
    if (half_points) *half_points = total / dims[rank - 1] * (dims[rank - 1] / 2 + 1);
    return total;
}

#define PHAST_ND_API(SFX, T)                                                                                            \
    int phast_fft_##SFX##_nd(T *re, size_t re_len, T *im, size_t im_len, const size_t *dims, size_t rank,                \
                             int direction) try {                                                                       \
        if ((!re && re_len) || (!im && im_len)) return PHAST_ERR_INVALID_ARG;                                           \
        if (direction != PHAST_FORWARD && direction != PHAST_REVERSE) return PHAST_ERR_INVALID_ARG;                     \
        const unsigned long long total = nd_points(dims, rank, nullptr);                                                \
        if (!total) return PHAST_ERR_INVALID_ARG;                                                                       \
        if (re_len != im_len) return PHAST_ERR_LEN_MISMATCH;                                                            \
        if (re_len != total) return PHAST_ERR_PLANNER_SIZE;                                                             \
        NdPlanner<T> *p = nullptr; /* a planner of the call's own */                                                   \
        int rc = nd_planner_new(dims, rank, kNdC2C, &p);                                                                \
        if (rc) return rc;                                                                                              \
        std::unique_ptr<NdPlanner<T>> own(p);                                                                           \
        return p->fft_host_nd(re, re_len, im, im_len, direction);                                                       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_nd_with_planner(T *re, size_t re_len, T *im, size_t im_len, int direction,                    \
                                          const phast_planner_nd##SFX *p) try {                                         \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->fft_host_nd(re, re_len, im, im_len, direction);                                                       \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_fft_##SFX##_nd_dev(T *d_re, T *d_im, size_t n_total, size_t batch, size_t dist, int direction,            \
                                 const phast_planner_nd##SFX *p, T *d_work, size_t work_len, void *stream) try {        \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->fft_dev_nd(d_re, d_im, n_total, batch, dist, direction, d_work, work_len,                             \
                             static_cast<hipStream_t>(stream));                                                         \
    } PHAST_CATCH_RC
PHAST_ND_API(64, double)
PHAST_ND_API(32, float)

#define PHAST_ND_REAL_API(SFX, FS, T)                                                                                   \
    int phast_r2c_fft_##FS##_nd(const T *in, size_t in_len, T *ore, size_t ore_len, T *oim, size_t oim_len,             \
                                const size_t *dims, size_t rank) try {                                                  \
        if (!in || !ore || !oim) return PHAST_ERR_INVALID_ARG;                                                          \
        unsigned long long hp = 0;                                                                                      \
        const unsigned long long total = nd_points(dims, rank, &hp);                                                    \
        if (!total) return PHAST_ERR_INVALID_ARG;                                                                       \
        if (in_len != total) return PHAST_ERR_R2C_INPUT_LEN; /* before the device is touched */                        \
        if (ore_len != hp) return PHAST_ERR_R2C_OUT_RE_LEN;                                                             \
        if (oim_len != hp) return PHAST_ERR_R2C_OUT_IM_LEN;                                                             \
        RealNdPlanner<T> *p = nullptr;                                                                                  \
        int rc = nd_planner_new(dims, rank, kNdR2C, &p);                                                                \
        if (rc) return rc;                                                                                              \
        std::unique_ptr<RealNdPlanner<T>> own(p);                                                                       \
        return p->host(false, in, in_len, nullptr, 0, ore, ore_len, oim, oim_len);                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_nd_with_planner(const T *in, size_t in_len, T *ore, size_t ore_len, T *oim,                \
                                             size_t oim_len, const phast_planner_r2c_nd##SFX *p) try {                  \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(false, in, in_len, nullptr, 0, ore, ore_len, oim, oim_len);                                      \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_r2c_fft_##FS##_nd_dev(const T *d_in, T *d_ore, T *d_oim, size_t n_total, size_t batch, size_t in_dist,    \
                                    size_t out_dist, const phast_planner_r2c_nd##SFX *p, T *d_work, size_t work_len,    \
                                    void *stream) try {                                                                 \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(false, d_in, nullptr, d_ore, d_oim, n_total, batch, in_dist, out_dist, d_work, work_len,          \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_nd(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *out, size_t out_len,     \
                                const size_t *dims, size_t rank) try {                                                  \
        if (!ire || !iim || !out) return PHAST_ERR_INVALID_ARG;                                                         \
        unsigned long long hp = 0;                                                                                      \
        const unsigned long long total = nd_points(dims, rank, &hp);                                                    \
        if (!total) return PHAST_ERR_INVALID_ARG;                                                                       \
        if (out_len != total) return PHAST_ERR_C2R_OUTPUT_LEN; /* before the device is touched */                      \
        if (ire_len != hp) return PHAST_ERR_C2R_IN_RE_LEN;                                                              \
        if (iim_len != hp) return PHAST_ERR_C2R_IN_IM_LEN;                                                              \
        RealNdPlanner<T> *p = nullptr;                                                                                  \
        int rc = nd_planner_new(dims, rank, kNdR2C, &p);                                                                \
        if (rc) return rc;                                                                                              \
        std::unique_ptr<RealNdPlanner<T>> own(p);                                                                       \
        return p->host(true, ire, ire_len, iim, iim_len, out, out_len, nullptr, 0);                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_nd_with_planner(const T *ire, size_t ire_len, const T *iim, size_t iim_len, T *out,        \
                                             size_t out_len, const phast_planner_r2c_nd##SFX *p) try {                  \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->host(true, ire, ire_len, iim, iim_len, out, out_len, nullptr, 0);                                     \
    } PHAST_CATCH_RC                                                                                                    \
    int phast_c2r_fft_##FS##_nd_dev(const T *d_ire, const T *d_iim, T *d_out, size_t n_total, size_t batch,             \
                                    size_t in_dist, size_t out_dist, const phast_planner_r2c_nd##SFX *p, T *d_work,     \
                                    size_t work_len, void *stream) try {                                                \
        if (!p) return PHAST_ERR_INVALID_ARG;                                                                           \
        return p->dev(true, d_ire, d_iim, d_out, nullptr, n_total, batch, in_dist, out_dist, d_work, work_len,          \
                      static_cast<hipStream_t>(stream));                                                                \
    } PHAST_CATCH_RC
PHAST_ND_REAL_API(64, f64, double)
PHAST_ND_REAL_API(32, f32, float)

}  // extern "C"
