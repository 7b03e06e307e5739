/*
 * phastft_hip.h -- C ABI of libphastft_hip.so, the MI355X (gfx950) drop-in for PhastFT's planar
 * power-of-two FFT path.
 *
 * The reference (QuState/PhastFT 0.3.0, /root/reference) has no FFI layer: its boundary is the
 * crate's public Rust API.  Every entry point below is named after, and
 * cites, the Rust item it replaces; a Rust shim crate binds them 1:1.
 *
 *   - plain pointers + explicit lengths (so the library re-validates what the Rust `assert!`s check)
 *   - `int direction`: +1 = Direction::Forward, -1 = Direction::Reverse  (planner.rs:10-16)
 *   - return value: PHAST_OK or one status per reference assert; phast_strerror() returns the
 *     reference's panic text so a shim can `panic!` with it (r2c.rs:1392-1540 tests the strings)
 *   - host-slice calls (no suffix) take HOST pointers, stage H2D/D2H internally and return with the
 *     result visible in the caller's slices -- the drop-in semantics of the Rust API
 *   - `_dev` calls take DEVICE pointers + a hipStream_t (as void*) and are asynchronous on that
 *     stream; they are what bench.py measures.  `batch` independent transforms, transform b at
 *     pointer + b*dist elements.
 *
 * Planners may be shared by concurrent host threads AND streams (planner.rs:38-39: the reference's planner is an
 * immutable value borrowed by `&`).  What a call mutates -- the inter-pass scratch, the staging buffer and pinned mirror of
 * the host-slice calls -- lives in a WORKSPACE, and a planner keeps a small pool of them (up to PHAST_MAX_WORKSPACES = 8,
 * made on demand): a call checks one out while it enqueues (a blocking host-slice call: for the whole call, on the
 * workspace's own non-blocking stream, never the NULL stream), calls on one stream come back to the same workspace, calls
 * on other streams get another one, and only when the pool is exhausted does a stream wait -- on the device, behind an
 * event -- for another stream's work.  N threads x N streams on one planner run side by side.
 * Graphs: a workspace used under stream capture belongs to the captured graph(s) until the planner is freed -- eager
 * calls never touch it again and none of its buffers is ever released early, so replays stay valid whatever the planner
 * is used for afterwards.  Replays of several graphs captured from ONE planner on ONE capture stream share that workspace:
 * order them among themselves (or capture them on different streams).
 *
 * Devices: a planner belongs to the HIP device that is current when it is created (its tables and scratch live
 * there).  One process may hold planners on several devices (one host thread per GPU, or one thread switching):
 * every call on a planner runs on the planner's device whatever the calling thread's current device is, and the
 * caller's current device is restored before the call returns.  Data pointers and the stream of a _dev call must
 * belong to (or be accessible from) the planner's device.
 *
 * Memory: scratch and staging buffers grow on demand (geometrically); an outgrown buffer is released as soon as the
 * work that used it has completed, never under stream capture.  When the device is out of memory a batched call
 * falls back to smaller chunks before it reports PHAST_ERR_HIP.
 */
#ifndef PHASTFT_HIP_H
#define PHASTFT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- planner.rs:10-32 ---- */
#define PHAST_FORWARD 1  /* Direction::Forward */
#define PHAST_REVERSE (-1) /* Direction::Reverse */
#define PHAST_MODE_HEURISTIC 0 /* PlannerMode::Heuristic */
#define PHAST_MODE_TUNE 1      /* PlannerMode::Tune: the planner measures its plans on the device at plan time (below) */

/* ---- status codes: one per reference assert ---- */
#define PHAST_OK 0
#define PHAST_ERR_NOT_POW2 1        /* planner.rs:66, algorithms/dit.rs:285,359 */
#define PHAST_ERR_LEN_MISMATCH 2    /* algorithms/dit.rs:284,358 */
#define PHAST_ERR_PLANNER_SIZE 3    /* algorithms/dit.rs:289,363 */
#define PHAST_ERR_R2C_N 4           /* planner.rs:195 */
#define PHAST_ERR_R2C_INPUT_LEN 5   /* algorithms/r2c.rs:543,615 */
#define PHAST_ERR_R2C_OUT_RE_LEN 6  /* algorithms/r2c.rs:544-548,616-620 */
#define PHAST_ERR_R2C_OUT_IM_LEN 7  /* algorithms/r2c.rs:549-553,621-625 */
#define PHAST_ERR_C2R_OUTPUT_LEN 8  /* algorithms/r2c.rs:750,846 */
#define PHAST_ERR_C2R_IN_RE_LEN 9   /* algorithms/r2c.rs:751-755,847-851 */
#define PHAST_ERR_C2R_IN_IM_LEN 10  /* algorithms/r2c.rs:756-760,852-856 */
#define PHAST_ERR_C2R_SCRATCH_RE 11 /* algorithms/r2c.rs:761,857 */
#define PHAST_ERR_C2R_SCRATCH_IM 12 /* algorithms/r2c.rs:762,858 */
#define PHAST_ERR_ALLOC 13          /* host allocation failed (incl. std::bad_alloc inside the library) */
#define PHAST_ERR_HIP 14            /* a HIP runtime call failed; see phast_last_hip_error() */
#define PHAST_ERR_NO_DEVICE 15      /* no gfx950 device visible: the library never falls back to CPU */
#define PHAST_ERR_INVALID_ARG 16    /* null pointer / bad direction / bit-reversal length != 2^n (bravo.rs:228) */

/* exact panic text of the reference for the code (or a description for the HIP-side codes) */
const char *phast_strerror(int code);
/* hipGetErrorString of the last failing HIP call on this thread ("" if none) */
const char *phast_last_hip_error(void);
/* library / device identification: returns PHAST_OK and fills what it can */
int phast_device_info(char *name, size_t name_len, int *compute_units, size_t *lds_per_block,
                      size_t *global_mem_bytes);

/* ---- options.rs:8-43 ---- */
typedef struct phast_options {
    int multithreaded_bit_reversal;      /* options.rs:17; CPU threading hint -- ignored on the GPU */
    size_t smallest_parallel_chunk_size; /* options.rs:24; ignored on the GPU */
} phast_options;
void phast_options_default(phast_options *out);               /* options.rs:26-33 */
int phast_options_guess(size_t input_size, phast_options *out); /* options.rs:38-43 */

/* ---- planner.rs:34-114 ----
 * num_points: a power of two (else PHAST_ERR_NOT_POW2, the reference's assert) up to 2^30 for f64 and 2^31 for
 * f32; larger sizes return PHAST_ERR_INVALID_ARG (the reference is bounded by host memory only). */
typedef struct phast_planner_dit64 phast_planner_dit64; /* PlannerDit64 */
typedef struct phast_planner_dit32 phast_planner_dit32; /* PlannerDit32 */
int phast_planner_dit64_new(size_t num_points, phast_planner_dit64 **out);                 /* planner.rs:55 */
int phast_planner_dit64_with_mode(size_t num_points, int mode, phast_planner_dit64 **out); /* planner.rs:65 */
void phast_planner_dit64_free(phast_planner_dit64 *p);
int phast_planner_dit32_new(size_t num_points, phast_planner_dit32 **out);
int phast_planner_dit32_with_mode(size_t num_points, int mode, phast_planner_dit32 **out);
void phast_planner_dit32_free(phast_planner_dit32 *p);
/* device footprint of a planner (twiddle tables + scratch), and its pass plan as text */
size_t phast_planner_dit64_device_bytes(const phast_planner_dit64 *p);
size_t phast_planner_dit32_device_bytes(const phast_planner_dit32 *p);
int phast_planner_dit64_describe(const phast_planner_dit64 *p, char *buf, size_t buf_len);
int phast_planner_dit32_describe(const phast_planner_dit32 *p, char *buf, size_t buf_len);
/* the plan a call of `kind` (PHAST_TUNE_*) with `batch` transforms runs, as text: "<which> [rows x cols ...]..." */
int phast_planner_dit64_describe_call(const phast_planner_dit64 *p, size_t batch, int kind, char *buf, size_t buf_len);
int phast_planner_dit32_describe_call(const phast_planner_dit32 *p, size_t batch, int kind, char *buf, size_t buf_len);
/* optional: size the scratch for `max_batch` transforms in flight (default 1); realloc on demand otherwise */
int phast_planner_dit64_reserve_batch(phast_planner_dit64 *p, size_t max_batch);
int phast_planner_dit32_reserve_batch(phast_planner_dit32 *p, size_t max_batch);
/* HIP graphs: the workspaces that captured calls work in are kept until the planner is freed (the library cannot know when a
 * graph dies).  A long-lived planner that is captured again and again may hand them back -- the caller promises that every
 * graph captured on this planner so far is gone.  Returns the device bytes released. */
size_t phast_planner_dit64_release_graph_workspaces(phast_planner_dit64 *p);
size_t phast_planner_dit32_release_graph_workspaces(phast_planner_dit32 *p);

/* ---- PlannerMode::Tune (planner.rs:18-32: "benchmarks both paths at plan time and picks whichever is faster, at the cost of
 * additional planning time") ----
 * The reference chooses between two codelet paths; here the choice is the PLAN -- how N = 2^L is cut into 2 or 3 passes, the
 * tile size of every pass, points per thread, wave / quad tiles, and for r2c whether the untangle rides in the last pass.
 * PHAST_MODE_HEURISTIC: static rules ranked on an MI355X (plus built-in / imported wisdom, below), zero planning overhead.
 * PHAST_MODE_TUNE (`_with_mode`): as the reference's -- the planner times every plan that exists for its length on the
 * current device, for ONE transform per call (the reference's only case), and keeps the fastest if it beats the static rule
 * by more than 3 %.  Costs 0.1 .. 3 s (under 1 s at N = 2^20).  Nothing to measure for N <= 4096 (one kernel).
 * `_tune` does the same for another batch size or call kind on an existing planner: a result covers batches in
 * (2^(b-1), 2^b] around `batch_hint`.  Tuning is synchronous, allocates a ring of input sets (up to 1.25 GiB, or three sets)
 * and must not run under stream capture.  Results are bit-identical for a given plan; which plan runs changes the last bits
 * (same tolerance: every plan is tested against the oracle). */
#define PHAST_TUNE_C2C 0             /* fft_*_dit* on planar arrays */
#define PHAST_TUNE_C2C_INTERLEAVED 1 /* the Complex<T> forms (lib.rs:41-140) */
#define PHAST_TUNE_R2C 2             /* r2c_fft_*   (PlannerR2c* only) */
#define PHAST_TUNE_C2R 3             /* c2r_fft_*   (PlannerR2c* only) */
typedef struct phast_tune_report {
    int adopted;             /* 1: a measured plan replaced the static rule's for this (kind, batch bucket) */
    unsigned candidates;     /* plans timed */
    float us_heuristic;      /* per call, static rule's plan (median of the interleaved rounds) */
    float us_best;           /* per call, the plan now in force */
    double seconds;          /* what the tuning run took */
    char plan[96];           /* "a,b[,c]@ta,tb[,tc]:p<points>[w][ fused]" or "heuristic" / "one pass" */
} phast_tune_report;
int phast_planner_dit64_tune(phast_planner_dit64 *p, size_t batch_hint, int kind, phast_tune_report *report /* or NULL */);
int phast_planner_dit32_tune(phast_planner_dit32 *p, size_t batch_hint, int kind, phast_tune_report *report);
/* Wisdom: what tuning runs found, as text (one line per type / kind / log2 length / batch bucket, csrc/wisdom.hpp).  Planners
 * created after an import start with the plans it names (entries measured on a device with another CU count or gfx architecture, or by another generation of the library's kernels -- the header line's cus= / arch= / lib= -- are kept but not applied).
 * PHAST_WISDOM=<path>: read at first use, rewritten after every tuning run.  The library also carries built-in wisdom measured
 * on an MI355X (PHAST_BUILTIN_WISDOM=0 turns it off).  No device needed for these three calls. */
int phast_wisdom_export(char *buf, size_t buf_len, size_t *needed /* bytes incl. NUL, or NULL */); /* without the built-in layer */
int phast_wisdom_import(const char *text); /* PHAST_ERR_INVALID_ARG: not a wisdom text (nothing of it is kept); lines that do not parse are skipped */
void phast_wisdom_forget(void);            /* everything but the built-in layer */
int phast_wisdom_builtin(int enable);      /* the built-in layer off / on again at run time (planners made afterwards); returns what it was (1 on, 0 off) so a caller can put it back */
size_t phast_wisdom_count(int layer);      /* entries of a layer: 0 built-in, 1 PHAST_WISDOM file, 2 imported, 3 measured here; -1 all */

/* ---- planner.rs:164-212 ---- */
typedef struct phast_planner_r2c64 phast_planner_r2c64; /* PlannerR2c64 */
typedef struct phast_planner_r2c32 phast_planner_r2c32; /* PlannerR2c32 */
int phast_planner_r2c64_new(size_t n, phast_planner_r2c64 **out); /* planner.rs:194 */
void phast_planner_r2c64_free(phast_planner_r2c64 *p);
int phast_planner_r2c32_new(size_t n, phast_planner_r2c32 **out);
void phast_planner_r2c32_free(phast_planner_r2c32 *p);
/* (no reference counterpart: PlannerR2c*::new has no mode -- the same switch as PlannerDit*::with_mode, for r2c_fft and c2r_fft
 * of one transform per call; `_tune`: kind = PHAST_TUNE_R2C or PHAST_TUNE_C2R) */
int phast_planner_r2c64_with_mode(size_t n, int mode, phast_planner_r2c64 **out);
int phast_planner_r2c32_with_mode(size_t n, int mode, phast_planner_r2c32 **out);
int phast_planner_r2c64_describe_call(const phast_planner_r2c64 *p, size_t batch, int kind, char *buf, size_t buf_len);
int phast_planner_r2c32_describe_call(const phast_planner_r2c32 *p, size_t batch, int kind, char *buf, size_t buf_len);
int phast_planner_r2c64_tune(phast_planner_r2c64 *p, size_t batch_hint, int kind, phast_tune_report *report);
int phast_planner_r2c32_tune(phast_planner_r2c32 *p, size_t batch_hint, int kind, phast_tune_report *report);

/* ---- C2C, host slices: lib.rs:143-226, algorithms/dit.rs:263,338 ----
 * The forms without a planner argument make one per call in the reference (lib.rs:181,224).  Here a planner owns device
 * memory, so the library keeps the few most recently used ones (per type, size, device; planes up to 64 MiB) and the
 * second call of a size costs what the _with_planner form costs.  Same results, same errors; PHAST_PLANNER_CACHE=0 turns
 * it off.  The same holds for the real-transform and interleaved forms below. */
int phast_fft_64_dit(double *reals, size_t reals_len, double *imags, size_t imags_len, int direction); /* lib.rs:180 */
int phast_fft_32_dit(float *reals, size_t reals_len, float *imags, size_t imags_len, int direction);   /* lib.rs:223 */
int phast_fft_64_dit_with_planner(double *reals, size_t reals_len, double *imags, size_t imags_len,
                                  int direction, const phast_planner_dit64 *planner); /* lib.rs:143 */
int phast_fft_32_dit_with_planner(float *reals, size_t reals_len, float *imags, size_t imags_len, int direction,
                                  const phast_planner_dit32 *planner); /* lib.rs:186 */
int phast_fft_64_dit_with_planner_and_opts(double *reals, size_t reals_len, double *imags, size_t imags_len,
                                           int direction, const phast_planner_dit64 *planner,
                                           const phast_options *opts); /* algorithms/dit.rs:263 */
int phast_fft_32_dit_with_planner_and_opts(float *reals, size_t reals_len, float *imags, size_t imags_len,
                                           int direction, const phast_planner_dit32 *planner,
                                           const phast_options *opts); /* algorithms/dit.rs:338 */

/* ---- C2C, device-resident, batched, asynchronous on `stream` (hipStream_t) ---- */
int phast_fft_64_dit_dev(double *d_reals, double *d_imags, size_t n, size_t batch, size_t dist, int direction,
                         const phast_planner_dit64 *planner, void *stream);
int phast_fft_32_dit_dev(float *d_reals, float *d_imags, size_t n, size_t batch, size_t dist, int direction,
                         const phast_planner_dit32 *planner, void *stream);
/* `count` independent transforms of n points at arbitrary device addresses (HOST arrays of device pointers), each run
 * exactly as a single-transform call, enqueued back to back by ONE host call -- a caller with many separate signals
 * (the Rust API takes one pair of slices per call, lib.rs:143) pays its FFI / interpreter overhead once. */
int phast_fft_64_dit_many_dev(double *const *d_reals, double *const *d_imags, size_t count, size_t n, int direction,
                              const phast_planner_dit64 *planner, void *stream);
int phast_fft_32_dit_many_dev(float *const *d_reals, float *const *d_imags, size_t count, size_t n, int direction,
                              const phast_planner_dit32 *planner, void *stream);
/* Strided batches (no reference counterpart): transform b occupies elements b*dist + j*stride, j < n.
 * stride == 1 is the call above.  dist == 1 with stride, batch powers of two, batch <= stride, n >= 64 are the
 * "column FFTs" of a row-major [n][stride] array (first `batch` columns), in place, natural order in and out -- what
 * a four-step split (phastft_amd/distributed.py) and multi-dimensional transforms need.  The planner's scratch grows
 * to n*stride elements per plane.  The kernels work on tiles of adjacent columns: batch >= 16 is always served,
 * batch == 8 for every n except 2^6, 2^12 and 2^13, batch == 4 only for n = 2^10 and 2^20, narrower batches never --
 * those (and anything else outside the description above) return PHAST_ERR_INVALID_ARG and nothing has run: transpose
 * and use the contiguous batch (phastft_amd/distributed.py does, and falls back on THAT code only). */
int phast_fft_64_dit_strided_dev(double *d_reals, double *d_imags, size_t n, size_t batch, size_t dist, size_t stride,
                                 int direction, const phast_planner_dit64 *planner, void *stream);
int phast_fft_32_dit_strided_dev(float *d_reals, float *d_imags, size_t n, size_t batch, size_t dist, size_t stride,
                                 int direction, const phast_planner_dit32 *planner, void *stream);
/* The same column FFTs with an INPUT twiddle fused into the first pass's load: element j of transform b is multiplied by
 * W_{tw_n}^(j * (tw_col0 + b)) before it is transformed -- the inter-factor twiddle of a four-step split (N = N1 N2 = tw_n,
 * this call = the second factor's transforms on rank-local columns tw_col0 ...), which otherwise is a sweep of its own
 * (phast_twiddle_grid*_apply_dev).  tw_n a power of two, n <= tw_n <= 2^32; dist == 1 only. */
int phast_fft_64_dit_strided_tw_dev(double *d_reals, double *d_imags, size_t n, size_t batch, size_t dist, size_t stride,
                                    int direction, const phast_planner_dit64 *planner, size_t tw_n, size_t tw_col0,
                                    void *stream);
int phast_fft_32_dit_strided_tw_dev(float *d_reals, float *d_imags, size_t n, size_t batch, size_t dist, size_t stride,
                                    int direction, const phast_planner_dit32 *planner, size_t tw_n, size_t tw_col0,
                                    void *stream);

/* ---- C2C on interleaved Complex<T> signals: lib.rs:41-140 (feature `complex-nums`) ----
 * `signal` holds n complex numbers as (re, im) pairs, transformed in place.  The reference copies into two planar
 * Vecs, runs the planar path and copies back (lib.rs:56-58); here the (de)interleave is fused into the first
 * pass's load and the last pass's store.  `dist` of the _dev form counts complex elements. */
int phast_fft_64_interleaved(double *signal, size_t n, int direction);                               /* lib.rs:120 */
int phast_fft_32_interleaved(float *signal, size_t n, int direction);
int phast_fft_64_interleaved_with_planner(double *signal, size_t n, int direction,
                                          const phast_planner_dit64 *planner);                       /* lib.rs:87 */
int phast_fft_32_interleaved_with_planner(float *signal, size_t n, int direction, const phast_planner_dit32 *planner);
int phast_fft_64_interleaved_with_planner_and_opts(double *signal, size_t n, int direction,
                                                   const phast_planner_dit64 *planner,
                                                   const phast_options *opts);                        /* lib.rs:50 */
int phast_fft_32_interleaved_with_planner_and_opts(float *signal, size_t n, int direction,
                                                   const phast_planner_dit32 *planner, const phast_options *opts);
int phast_fft_64_interleaved_dev(double *d_signal, size_t n, size_t batch, size_t dist, int direction,
                                 const phast_planner_dit64 *planner, void *stream);
int phast_fft_32_interleaved_dev(float *d_signal, size_t n, size_t batch, size_t dist, int direction,
                                 const phast_planner_dit32 *planner, void *stream);

/* ---- complex transforms of ANY length N >= 1 (no reference counterpart: the reference takes powers of two only; its README
 * names other lengths as its first planned feature).  Bluestein's algorithm: the length-N DFT as a cyclic convolution of
 * M = 2^ceil(log2(2N - 1)) points on the power-of-two engine ("Arbitrary lengths").  N <= 2^29 for both types
 * (N = 0 or more: PHAST_ERR_INVALID_ARG).  A power-of-two N calls the phast_fft_*_dit path itself: same bits, no workspace.
 * Forward is unnormalised, the inverse scales by 1/N, as above.  A planner belongs to the device current at creation and
 * is immutable after _new (its table is ready on any stream); share it between threads and streams freely.
 *
 * _dev calls take a caller-provided device workspace of work_len elements of T: phast_planner_any*_workspace_len(p, batch)
 * = 2 M batch (0 for a power of two).  Any work_len >= 2 M is legal: the batch then runs in chunks of floor(work_len / 2M)
 * transforms.  The planner holds no per-call state, so graph capture and concurrent streams are safe as long as no two
 * calls in flight share a workspace.  The bits of a transform do not depend on the batch, the chunking or the form of the
 * call.  Host-slice calls stage through the device (they block). */
typedef struct phast_planner_any64 phast_planner_any64; /* PlannerAny64 */
typedef struct phast_planner_any32 phast_planner_any32; /* PlannerAny32 */
int phast_planner_any64_new(size_t n, phast_planner_any64 **out);
int phast_planner_any32_new(size_t n, phast_planner_any32 **out);
void phast_planner_any64_free(phast_planner_any64 *p);
void phast_planner_any32_free(phast_planner_any32 *p);
int phast_planner_any64_describe(const phast_planner_any64 *p, char *buf, size_t buf_len);
int phast_planner_any32_describe(const phast_planner_any32 *p, char *buf, size_t buf_len);
size_t phast_planner_any64_device_bytes(const phast_planner_any64 *p);
size_t phast_planner_any32_device_bytes(const phast_planner_any32 *p);
size_t phast_planner_any64_workspace_len(const phast_planner_any64 *p, size_t batch);
size_t phast_planner_any32_workspace_len(const phast_planner_any32 *p, size_t batch);
int phast_fft_64_any(double *reals, size_t reals_len, double *imags, size_t imags_len, int direction);
int phast_fft_32_any(float *reals, size_t reals_len, float *imags, size_t imags_len, int direction);
int phast_fft_64_any_with_planner(double *reals, size_t reals_len, double *imags, size_t imags_len, int direction,
                                  const phast_planner_any64 *planner);
int phast_fft_32_any_with_planner(float *reals, size_t reals_len, float *imags, size_t imags_len, int direction,
                                  const phast_planner_any32 *planner);
int phast_fft_64_any_dev(double *d_reals, double *d_imags, size_t n, size_t batch, size_t dist, int direction,
                         const phast_planner_any64 *planner, double *d_work, size_t work_len, void *stream);
int phast_fft_32_any_dev(float *d_reals, float *d_imags, size_t n, size_t batch, size_t dist, int direction,
                         const phast_planner_any32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/any_len_rate.py): stage_ms[5] = average milliseconds of the chirp-pad sweep, the forward M-point
 * engine call, the spectrum sweep, the inverse engine call and the chirp-post sweep over `reps` forward calls of the batch
 * in ONE chunk (work_len >= 2 M batch); not for powers of two.  Blocks until done. */
int phast_planner_any64_time_stages(const phast_planner_any64 *p, double *d_reals, double *d_imags, size_t batch, size_t dist,
                                    double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
int phast_planner_any32_time_stages(const phast_planner_any32 *p, float *d_reals, float *d_imags, size_t batch, size_t dist,
                                    float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- real transforms (R2C / C2R) of ANY length N >= 1 (no reference counterpart: r2c.rs takes powers of two >= 4).  NumPy
 * rfft / irfft semantics with this library's conventions: R2C writes the half spectrum X[k], k = 0 .. floor(N/2), to two
 * planes of floor(N/2) + 1 points (unnormalised; Im X[0] = 0 exactly, and Im X[N/2] = 0 exactly for even N); C2R reads them
 * and writes the real signal of N points, scaled by 1/N (for a Hermitian spectrum, irfft(X, N)).  The length codes 5-10 of
 * the power-of-two calls apply, with floor(N/2).  N <= 2^29 for both types (N = 0 or more: PHAST_ERR_INVALID_ARG, before the
 * device is touched).  Algorithms: a power of two N >= 4 calls phast_r2c_fft_*_dev / phast_c2r_fft_*_dev
 * itself (same bits, no workspace); an even N packs x[2n] + i x[2n+1] into an N/2-point Bluestein transform (the
 * phast_planner_any* engine, table and spectrum sweep) and untangles -- C2R runs the power-of-two path's preprocess formula,
 * so a non-Hermitian input gives what that formula gives; an odd N runs an N-point Bluestein transform on real data (C2R:
 * Im X[0] is ignored, as irfft ignores it); N = 1 and 2 are direct (C2R: the imaginary parts are ignored).  R2C never writes
 * its input, C2R never its input planes.
 *
 * _dev calls: asynchronous on `stream`; `batch` transforms, the real side `in_dist` (R2C) / `out_dist` (C2R) >= N elements
 * apart, the complex side >= floor(N/2) + 1 apart; pointers need element alignment only.  One limit: a power of two N >= 4
 * runs phast_r2c_fft_*_dev / phast_c2r_fft_*_dev, which read and write the real side as (even, odd) pairs, so there a batch
 * needs an EVEN real-side distance (R2C in_dist, C2R out_dist); an odd one is PHAST_ERR_INVALID_ARG.  The caller's device workspace holds
 * phast_planner_r2c_any*_workspace_len(p, batch) = 2 M batch elements of T (M: the inner convolution length; 0 for N a
 * power of two, 1 or 2); any work_len >= 2 M runs the batch in chunks.  A null pointer, a short dist or a null / short
 * workspace is PHAST_ERR_INVALID_ARG; an `n` that is not the planner's, PHAST_ERR_PLANNER_SIZE.  The planner is immutable
 * and holds no per-call state (graph capture, threads and streams as for phast_planner_any*), and the bits of a transform
 * do not depend on the batch, the chunking, the stream or the form of the call.  Host-slice calls stage through the device
 * (they block). */
typedef struct phast_planner_r2c_any64 phast_planner_r2c_any64; /* PlannerR2cAny64 */
typedef struct phast_planner_r2c_any32 phast_planner_r2c_any32; /* PlannerR2cAny32 */
int phast_planner_r2c_any64_new(size_t n, phast_planner_r2c_any64 **out);
int phast_planner_r2c_any32_new(size_t n, phast_planner_r2c_any32 **out);
void phast_planner_r2c_any64_free(phast_planner_r2c_any64 *p);
void phast_planner_r2c_any32_free(phast_planner_r2c_any32 *p);
int phast_planner_r2c_any64_describe(const phast_planner_r2c_any64 *p, char *buf, size_t buf_len);
int phast_planner_r2c_any32_describe(const phast_planner_r2c_any32 *p, char *buf, size_t buf_len);
size_t phast_planner_r2c_any64_device_bytes(const phast_planner_r2c_any64 *p);
size_t phast_planner_r2c_any32_device_bytes(const phast_planner_r2c_any32 *p);
size_t phast_planner_r2c_any64_workspace_len(const phast_planner_r2c_any64 *p, size_t batch);
size_t phast_planner_r2c_any32_workspace_len(const phast_planner_r2c_any32 *p, size_t batch);
int phast_r2c_fft_f64_any(const double *input, size_t input_len, double *output_re, size_t output_re_len, double *output_im,
                          size_t output_im_len);
int phast_r2c_fft_f32_any(const float *input, size_t input_len, float *output_re, size_t output_re_len, float *output_im,
                          size_t output_im_len);
int phast_r2c_fft_f64_any_with_planner(const double *input, size_t input_len, double *output_re, size_t output_re_len,
                                       double *output_im, size_t output_im_len, const phast_planner_r2c_any64 *planner);
int phast_r2c_fft_f32_any_with_planner(const float *input, size_t input_len, float *output_re, size_t output_re_len,
                                       float *output_im, size_t output_im_len, const phast_planner_r2c_any32 *planner);
int phast_r2c_fft_f64_any_dev(const double *d_input, double *d_output_re, double *d_output_im, size_t n, size_t batch,
                              size_t in_dist, size_t out_dist, const phast_planner_r2c_any64 *planner, double *d_work,
                              size_t work_len, void *stream);
int phast_r2c_fft_f32_any_dev(const float *d_input, float *d_output_re, float *d_output_im, size_t n, size_t batch,
                              size_t in_dist, size_t out_dist, const phast_planner_r2c_any32 *planner, float *d_work,
                              size_t work_len, void *stream);
int phast_c2r_fft_f64_any(const double *input_re, size_t input_re_len, const double *input_im, size_t input_im_len,
                          double *output, size_t output_len);
int phast_c2r_fft_f32_any(const float *input_re, size_t input_re_len, const float *input_im, size_t input_im_len,
                          float *output, size_t output_len);
int phast_c2r_fft_f64_any_with_planner(const double *input_re, size_t input_re_len, const double *input_im,
                                       size_t input_im_len, double *output, size_t output_len,
                                       const phast_planner_r2c_any64 *planner);
int phast_c2r_fft_f32_any_with_planner(const float *input_re, size_t input_re_len, const float *input_im,
                                       size_t input_im_len, float *output, size_t output_len,
                                       const phast_planner_r2c_any32 *planner);
int phast_c2r_fft_f64_any_dev(const double *d_input_re, const double *d_input_im, double *d_output, size_t n, size_t batch,
                              size_t in_dist, size_t out_dist, const phast_planner_r2c_any64 *planner, double *d_work,
                              size_t work_len, void *stream);
int phast_c2r_fft_f32_any_dev(const float *d_input_re, const float *d_input_im, float *d_output, size_t n, size_t batch,
                              size_t in_dist, size_t out_dist, const phast_planner_r2c_any32 *planner, float *d_work,
                              size_t work_len, void *stream);
/* measurement hooks (tools/any_real_rate.py): stage_ms[5] = average milliseconds of the pad sweep, the forward M-point engine
 * call, the spectrum sweep, the inverse engine call and the post sweep over `reps` calls of the batch at the natural
 * distances in ONE chunk (work_len >= 2 M batch); not for N a power of two, 1 or 2.  Block until done. */
int phast_planner_r2c_any64_time_stages(const phast_planner_r2c_any64 *p, const double *d_input, double *d_output_re,
                                        double *d_output_im, size_t batch, double *d_work, size_t work_len, int reps,
                                        float *stage_ms, void *stream);
int phast_planner_r2c_any32_time_stages(const phast_planner_r2c_any32 *p, const float *d_input, float *d_output_re,
                                        float *d_output_im, size_t batch, float *d_work, size_t work_len, int reps,
                                        float *stage_ms, void *stream);
int phast_planner_r2c_any64_time_c2r_stages(const phast_planner_r2c_any64 *p, const double *d_input_re,
                                            const double *d_input_im, double *d_output, size_t batch, double *d_work,
                                            size_t work_len, int reps, float *stage_ms, void *stream);
int phast_planner_r2c_any32_time_c2r_stages(const phast_planner_r2c_any32 *p, const float *d_input_re,
                                            const float *d_input_im, float *d_output, size_t batch, float *d_work,
                                            size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- DCT and DST of types II and III, any length 1 <= N <= 2^29 (no reference counterpart; scipy.fft.dct / dst with
 * orthogonalize=True, FFTW REDFT10 / REDFT01 / RODFT10 / RODFT01).  With norm = PHAST_NORM_BACKWARD (scipy's default):
 *     DCT-II   y[k] = 2 sum_{n<N} x[n] cos(pi k (2n+1) / (2N))
 *     DCT-III  y[k] = x[0] + 2 sum_{1<=n<N} x[n] cos(pi n (2k+1) / (2N))
 *     DST-II   y[k] = 2 sum_{n<N} x[n] sin(pi (k+1) (2n+1) / (2N))
 *     DST-III  y[k] = (-1)^k x[N-1] + 2 sum_{n<N-1} x[n] sin(pi (n+1) (2k+1) / (2N))
 * PHAST_NORM_FORWARD scales the result by 1/(2N); PHAST_NORM_ORTHO by 1/sqrt(2N), and in addition DCT-II divides y[0] and
 * DST-II y[N-1] by sqrt 2, DCT-III multiplies x[0] and DST-III x[N-1] by sqrt 2 first.  The inverse of type t with norm
 * backward / ortho / forward is type 5 - t with norm forward / ortho / backward (scipy's idct / idst).  `type` is 2 or 3
 * (types I and IV are reserved); any other type or norm is PHAST_ERR_INVALID_ARG.
 *
 * Algorithm: Makhoul's -- one real transform of the same N (the phast_planner_r2c_any* engine, called
 * unchanged: R2C for type II, C2R for type III) between two O(N) sweeps.  The caller's device workspace holds
 * phast_planner_dct*_workspace_len(p, batch) elements of T; any work_len >= phast_planner_dct*_workspace_len(p, 1) runs the
 * batch in chunks, a null or shorter one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous on `stream`; `batch` transforms,
 * in_dist and out_dist >= N (no parity rule); pointers need element alignment only.  In place (d_out == d_in with in_dist ==
 * out_dist) is allowed; any other overlap of input and output is undefined.  Out of place, the input is never written.  A
 * null pointer, a bad type or norm or a short dist is PHAST_ERR_INVALID_ARG, an `n` that is not the planner's
 * PHAST_ERR_PLANNER_SIZE, host slices of unequal lengths PHAST_ERR_LEN_MISMATCH -- all before the device is touched.  The
 * planner is immutable and holds no per-call state; the bits of a transform do not depend on the batch, the chunking, the
 * stream, graph replay, the form of the call (host slice or _dev), in place or out of place, or pointer alignment.
 * Host-slice calls stage through the device (they block). */
#define PHAST_NORM_BACKWARD 0
#define PHAST_NORM_ORTHO 1
#define PHAST_NORM_FORWARD 2
typedef struct phast_planner_dct64 phast_planner_dct64; /* PlannerDct64 */
typedef struct phast_planner_dct32 phast_planner_dct32; /* PlannerDct32 */
int phast_planner_dct64_new(size_t n, phast_planner_dct64 **out);
int phast_planner_dct32_new(size_t n, phast_planner_dct32 **out);
void phast_planner_dct64_free(phast_planner_dct64 *p);
void phast_planner_dct32_free(phast_planner_dct32 *p);
int phast_planner_dct64_describe(const phast_planner_dct64 *p, char *buf, size_t buf_len);
int phast_planner_dct32_describe(const phast_planner_dct32 *p, char *buf, size_t buf_len);
size_t phast_planner_dct64_device_bytes(const phast_planner_dct64 *p);
size_t phast_planner_dct32_device_bytes(const phast_planner_dct32 *p);
size_t phast_planner_dct64_workspace_len(const phast_planner_dct64 *p, size_t batch);
size_t phast_planner_dct32_workspace_len(const phast_planner_dct32 *p, size_t batch);
int phast_dct_f64(const double *input, size_t input_len, double *output, size_t output_len, int type, int norm);
int phast_dct_f32(const float *input, size_t input_len, float *output, size_t output_len, int type, int norm);
int phast_dst_f64(const double *input, size_t input_len, double *output, size_t output_len, int type, int norm);
int phast_dst_f32(const float *input, size_t input_len, float *output, size_t output_len, int type, int norm);
int phast_dct_f64_with_planner(const double *input, size_t input_len, double *output, size_t output_len, int type, int norm,
                               const phast_planner_dct64 *planner);
int phast_dct_f32_with_planner(const float *input, size_t input_len, float *output, size_t output_len, int type, int norm,
                               const phast_planner_dct32 *planner);
int phast_dst_f64_with_planner(const double *input, size_t input_len, double *output, size_t output_len, int type, int norm,
                               const phast_planner_dct64 *planner);
int phast_dst_f32_with_planner(const float *input, size_t input_len, float *output, size_t output_len, int type, int norm,
                               const phast_planner_dct32 *planner);
int phast_dct_f64_dev(const double *d_input, double *d_output, size_t n, size_t batch, size_t in_dist, size_t out_dist, int type,
                      int norm, const phast_planner_dct64 *planner, double *d_work, size_t work_len, void *stream);
int phast_dct_f32_dev(const float *d_input, float *d_output, size_t n, size_t batch, size_t in_dist, size_t out_dist, int type,
                      int norm, const phast_planner_dct32 *planner, float *d_work, size_t work_len, void *stream);
int phast_dst_f64_dev(const double *d_input, double *d_output, size_t n, size_t batch, size_t in_dist, size_t out_dist, int type,
                      int norm, const phast_planner_dct64 *planner, double *d_work, size_t work_len, void *stream);
int phast_dst_f32_dev(const float *d_input, float *d_output, size_t n, size_t batch, size_t in_dist, size_t out_dist, int type,
                      int norm, const phast_planner_dct32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/dct_rate.py): stage_ms[3] = average milliseconds of the pre sweep, the real transform and the post
 * sweep of a DCT (dst = 0) or DST (dst = 1) of `type` over `reps` calls of `batch` transforms at distance N in ONE chunk
 * (work_len >= phast_planner_dct*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_dct64_time_stages(const phast_planner_dct64 *p, int dst, int type, int norm, const double *d_input,
                                    double *d_output, size_t batch, double *d_work, size_t work_len, int reps, float *stage_ms,
                                    void *stream);
int phast_planner_dct32_time_stages(const phast_planner_dct32 *p, int dst, int type, int norm, const float *d_input,
                                    float *d_output, size_t batch, float *d_work, size_t work_len, int reps, float *stage_ms,
                                    void *stream);

/* ---- the short-time Fourier transform and its inverse (no reference counterpart; torch.stft / torch.istft(length = L) with
 * win_length = n_fft and normalized = False).  Signal length L, frame length F = n_fft, hop H, window w[0..F),
 * p = F / 2 (floor) with `center`, else 0; frames = 1 + (L + 2p - F) / H (floor), bins = F / 2 + 1.
 *     forward  S[f] = rfft_F(w[j] x~[f H - p + j]), x~ = x inside [0, L); outside, PHAST_PAD_REFLECT mirrors (x[-i], x[2(L-1) - i])
 *              and PHAST_PAD_ZERO gives 0.  Two dense planes (re, im): signal b, frame f, bin k at (b frames + f) bins + k
 *              (torch's result transposed).
 *     inverse  y[f] = irfft_F(S[f]); out[t] = sum_f w[u - f H] y[f][u - f H] / sum_f w^2[u - f H], u = t + p, over the frames
 *              that hold u in ascending f; a sample no frame holds is written as 0.
 * _new takes 1 <= H <= F <= 2^29, 1 <= L <= 2^29, p < L with center and reflect, L >= F without center (pad_mode is then
 * ignored), frames F <= 2^30, `window` a host pointer to F values or NULL for all ones: anything else is
 * PHAST_ERR_INVALID_ARG before the device is touched.  _envelope_min is the minimum of sum_f w^2 over the samples some frame
 * holds, computed once on the host in double; the inverse through a planner where it is <= 1e-11 is PHAST_ERR_INVALID_ARG
 * (torch's NOLA rule and threshold).
 *
 * One real transform of F (the phast_planner_r2c_any* engine, called unchanged) and one O(frames F) sweep per direction.
 * The caller's device workspace holds phast_planner_stft*_workspace_len(p, batch) elements of T.  The forward call runs any
 * work_len >= _workspace_min(p, 0) (one frame) in chunks of whole frames, the inverse any work_len >= _workspace_min(p, 1)
 * (one signal's frames) in chunks of whole signals; a null or shorter one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous
 * on `stream`; `batch` signals at sig_dist >= L (any parity), pointers need element alignment only; the signal is never
 * written by the forward call, the planes never by the inverse.  A signal_len that is not the planner's is
 * PHAST_ERR_PLANNER_SIZE, host planes that are not frames * bins long PHAST_ERR_LEN_MISMATCH.  The planner is immutable and
 * holds no per-call state.  The overlap-add is a gather without atomics: the bits of a signal do not depend on the batch, the
 * chunking, the stream or graph replay wherever the real transform's do not (every F that is not a power of two, and powers
 * of two up to 4096).  Host-slice calls take one signal, stage through the device and block. */
#define PHAST_PAD_REFLECT 0
#define PHAST_PAD_ZERO 1
typedef struct phast_planner_stft64 phast_planner_stft64; /* PlannerStft64 */
int phast_planner_stft64_new(size_t signal_len, size_t n_fft, size_t hop, const double *window, int center, int pad_mode,
                             phast_planner_stft64 **out);
void phast_planner_stft64_free(phast_planner_stft64 *p);
int phast_planner_stft64_describe(const phast_planner_stft64 *p, char *buf, size_t buf_len);
size_t phast_planner_stft64_device_bytes(const phast_planner_stft64 *p);
size_t phast_planner_stft64_frames(const phast_planner_stft64 *p);
size_t phast_planner_stft64_bins(const phast_planner_stft64 *p);
size_t phast_planner_stft64_workspace_len(const phast_planner_stft64 *p, size_t batch);
size_t phast_planner_stft64_workspace_min(const phast_planner_stft64 *p, int inverse);
double phast_planner_stft64_envelope_min(const phast_planner_stft64 *p);
int phast_stft_f64_with_planner(const double *signal, size_t signal_len, double *output_re, size_t output_re_len, double *output_im,
                                size_t output_im_len, const phast_planner_stft64 *planner);
int phast_istft_f64_with_planner(const double *input_re, size_t input_re_len, const double *input_im, size_t input_im_len, double *signal,
                                 size_t signal_len, const phast_planner_stft64 *planner);
int phast_stft_f64_dev(const double *d_signal, double *d_re, double *d_im, size_t signal_len, size_t batch, size_t sig_dist,
                       const phast_planner_stft64 *planner, double *d_work, size_t work_len, void *stream);
int phast_istft_f64_dev(const double *d_re, const double *d_im, double *d_signal, size_t signal_len, size_t batch, size_t sig_dist,
                        const phast_planner_stft64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/stft_rate.py): stage_ms[2] = average milliseconds of the sweep and of the real transform of the
 * forward (inverse = 0) or inverse call over `reps` calls of `batch` signals at distance L in ONE chunk (work_len >=
 * phast_planner_stft*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_stft64_time_stages(const phast_planner_stft64 *p, int inverse, double *d_signal, double *d_re, double *d_im, size_t batch,
                                     double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_stft32 phast_planner_stft32; /* PlannerStft32 */
int phast_planner_stft32_new(size_t signal_len, size_t n_fft, size_t hop, const float *window, int center, int pad_mode,
                             phast_planner_stft32 **out);
void phast_planner_stft32_free(phast_planner_stft32 *p);
int phast_planner_stft32_describe(const phast_planner_stft32 *p, char *buf, size_t buf_len);
size_t phast_planner_stft32_device_bytes(const phast_planner_stft32 *p);
size_t phast_planner_stft32_frames(const phast_planner_stft32 *p);
size_t phast_planner_stft32_bins(const phast_planner_stft32 *p);
size_t phast_planner_stft32_workspace_len(const phast_planner_stft32 *p, size_t batch);
size_t phast_planner_stft32_workspace_min(const phast_planner_stft32 *p, int inverse);
double phast_planner_stft32_envelope_min(const phast_planner_stft32 *p);
int phast_stft_f32_with_planner(const float *signal, size_t signal_len, float *output_re, size_t output_re_len, float *output_im,
                                size_t output_im_len, const phast_planner_stft32 *planner);
int phast_istft_f32_with_planner(const float *input_re, size_t input_re_len, const float *input_im, size_t input_im_len, float *signal,
                                 size_t signal_len, const phast_planner_stft32 *planner);
int phast_stft_f32_dev(const float *d_signal, float *d_re, float *d_im, size_t signal_len, size_t batch, size_t sig_dist,
                       const phast_planner_stft32 *planner, float *d_work, size_t work_len, void *stream);
int phast_istft_f32_dev(const float *d_re, const float *d_im, float *d_signal, size_t signal_len, size_t batch, size_t sig_dist,
                        const phast_planner_stft32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/stft_rate.py): stage_ms[2] = average milliseconds of the sweep and of the real transform of the
 * forward (inverse = 0) or inverse call over `reps` calls of `batch` signals at distance L in ONE chunk (work_len >=
 * phast_planner_stft*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_stft32_time_stages(const phast_planner_stft32 *p, int inverse, float *d_signal, float *d_re, float *d_im, size_t batch,
                                     float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- the modified discrete cosine transform and its inverse (no reference counterpart, and none in torch or scipy; DESIGN.md
 * §24).  N coefficients per frame, N even, 2 <= N <= 2^29 (an odd N is PHAST_ERR_INVALID_ARG: no codec uses one, and it would
 * need a 2N-point inner transform); frame length 2N, hop N; window w[0..2N): host doubles (64) or floats (32) given at _new
 * and held as T on the device, NULL for the sine window sin(pi (n + 1/2) / (2N)).  h = N / 2.
 *     forward  For frame t of a signal x[0..L), zero outside [0, L), with s_t = (t - padded) N:
 *                  X_t[k] = sum_{n=0}^{2N-1} w[n] x[s_t + n] cos(pi/N (n + 1/2 + N/2)(k + 1/2)),  k = 0 .. N-1
 *              There is no scale on the forward transform.
 *     frames   padded = 1: F = ceil(L / N) + 1 and L >= 1; every sample lies in exactly two frames.
 *              padded = 0: F = floor(L / N) - 1, L >= 2N is required, and the tail beyond (F + 1) N is not read.
 *              The coefficients are [batch][F][N], row-major and packed, as the STFT's planes are.
 *     inverse  With y_t[n] = (2/N) w[n] sum_k X_t[k] cos(pi/N (n + 1/2 + N/2)(k + 1/2)), out[s] = sum_t y_t[s - s_t] for
 *              0 <= s < L.  There is no division by an envelope (an MDCT cannot be normalised after the fact).  Every output
 *              sample has at most two source frames; a sample with one (padded = 0: s < N or s >= F N) gets that one term,
 *              a sample with none is written as 0.
 * Perfect reconstruction: if w[n]^2 + w[n+N]^2 = 1 and w[2N-1-n] = w[n], then imdct(mdct(x)) = x on all of [0, L) for
 * padded = 1 and on [N, F N) for padded = 0.  _tdac_defect is max(max_n |w[n]^2 + w[n+N]^2 - 1|, max_n |w[n] - w[2N-1-n]|),
 * computed once at _new in double from the values given (for NULL: from the sine window before it is rounded to T).  The
 * planner never refuses a window: an analysis-only caller may pass any.
 * _new takes 1 <= L <= 2^29, frames N <= 2^30 and padded in {0, 1}; anything else is PHAST_ERR_INVALID_ARG before the device
 * is touched.
 *
 * One complex transform of h points per frame (the phast_planner_any* engine, called unchanged) between two O(frames N)
 * sweeps: the fold of 2N windowed samples to N and a DCT-IV of N, whose two twiddle sets are device tables built at _new.
 * The caller's device workspace holds phast_planner_mdct*_workspace_len(p, batch) elements of T.  The forward call runs any
 * work_len >= _workspace_min(p, 0) (one frame) in chunks of whole frames, the inverse any work_len >= _workspace_min(p, 1)
 * (one signal's frames) in chunks of whole signals; a null or shorter one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous
 * on `stream`; `batch` signals at sig_dist >= L, coefficients packed, pointers need element alignment only; the inputs of
 * both calls are never written, and in place is not offered (the shapes differ).  A signal_len that is not the planner's is
 * PHAST_ERR_PLANNER_SIZE, host coefficients that are not frames * N long PHAST_ERR_LEN_MISMATCH.  The planner is immutable and
 * holds no per-call state.  The overlap-add is a gather without atomics.  Host-slice calls take one signal, stage through the
 * device and block. */
typedef struct phast_planner_mdct64 phast_planner_mdct64; /* PlannerMdct64 */
int phast_planner_mdct64_new(size_t signal_len, size_t n, const double *window, int padded, phast_planner_mdct64 **out);
void phast_planner_mdct64_free(phast_planner_mdct64 *p);
int phast_planner_mdct64_describe(const phast_planner_mdct64 *p, char *buf, size_t buf_len);
size_t phast_planner_mdct64_device_bytes(const phast_planner_mdct64 *p);
size_t phast_planner_mdct64_frames(const phast_planner_mdct64 *p);
size_t phast_planner_mdct64_workspace_len(const phast_planner_mdct64 *p, size_t batch);
size_t phast_planner_mdct64_workspace_min(const phast_planner_mdct64 *p, int inverse);
double phast_planner_mdct64_tdac_defect(const phast_planner_mdct64 *p);
int phast_mdct_f64_with_planner(const double *signal, size_t signal_len, double *coefs, size_t coefs_len, const phast_planner_mdct64 *planner);
int phast_imdct_f64_with_planner(const double *coefs, size_t coefs_len, double *signal, size_t signal_len, const phast_planner_mdct64 *planner);
int phast_mdct_f64_dev(const double *d_signal, double *d_coefs, size_t signal_len, size_t batch, size_t sig_dist,
                       const phast_planner_mdct64 *planner, double *d_work, size_t work_len, void *stream);
int phast_imdct_f64_dev(const double *d_coefs, double *d_signal, size_t signal_len, size_t batch, size_t sig_dist,
                        const phast_planner_mdct64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/mdct_rate.py): stage_ms[3] = average milliseconds of the pre sweep, of the complex transform and of
 * the post sweep (inverse = 1: the post and the overlap-add sweeps together) over `reps` calls of `batch` signals at distance
 * L in ONE chunk (work_len >= phast_planner_mdct*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_mdct64_time_stages(const phast_planner_mdct64 *p, int inverse, double *d_signal, double *d_coefs, size_t batch, double *d_work, size_t work_len,
                                     int reps, float *stage_ms, void *stream);
typedef struct phast_planner_mdct32 phast_planner_mdct32; /* PlannerMdct32 */
int phast_planner_mdct32_new(size_t signal_len, size_t n, const float *window, int padded, phast_planner_mdct32 **out);
void phast_planner_mdct32_free(phast_planner_mdct32 *p);
int phast_planner_mdct32_describe(const phast_planner_mdct32 *p, char *buf, size_t buf_len);
size_t phast_planner_mdct32_device_bytes(const phast_planner_mdct32 *p);
size_t phast_planner_mdct32_frames(const phast_planner_mdct32 *p);
size_t phast_planner_mdct32_workspace_len(const phast_planner_mdct32 *p, size_t batch);
size_t phast_planner_mdct32_workspace_min(const phast_planner_mdct32 *p, int inverse);
double phast_planner_mdct32_tdac_defect(const phast_planner_mdct32 *p);
int phast_mdct_f32_with_planner(const float *signal, size_t signal_len, float *coefs, size_t coefs_len, const phast_planner_mdct32 *planner);
int phast_imdct_f32_with_planner(const float *coefs, size_t coefs_len, float *signal, size_t signal_len, const phast_planner_mdct32 *planner);
int phast_mdct_f32_dev(const float *d_signal, float *d_coefs, size_t signal_len, size_t batch, size_t sig_dist,
                       const phast_planner_mdct32 *planner, float *d_work, size_t work_len, void *stream);
int phast_imdct_f32_dev(const float *d_coefs, float *d_signal, size_t signal_len, size_t batch, size_t sig_dist,
                        const phast_planner_mdct32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/mdct_rate.py): stage_ms[3] = average milliseconds of the pre sweep, of the complex transform and of
 * the post sweep (inverse = 1: the post and the overlap-add sweeps together) over `reps` calls of `batch` signals at distance
 * L in ONE chunk (work_len >= phast_planner_mdct*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_mdct32_time_stages(const phast_planner_mdct32 *p, int inverse, float *d_signal, float *d_coefs, size_t batch, float *d_work, size_t work_len,
                                     int reps, float *stage_ms, void *stream);

/* ---- Welch spectral estimation: welch, csd, spectrogram (no reference counterpart; scipy.signal.welch / csd / spectrogram
 * with return_onesided = True, mode = "psd", boundary = None, padded = False).
 *     sizes     L samples per signal, P = nperseg, H = hop = nperseg - noverlap, F = nfft; 1 <= H <= P <= F <= 2^29,
 *               P <= L <= 2^29.  Segments S = 1 + floor((L - P) / H); the tail beyond the last segment is not read.
 *               bins = floor(F / 2) + 1.  fd = F rounded up to 16 bytes; S fd <= 2^30.
 *     window    P host values (double for both types); NULL: Hann, scipy.signal.get_window("hann", P), the periodic form,
 *               built on the host in long double.
 *     segment   r_f[j] = w[j] (x[f H + j] - m_f) for j < P, and 0 for P <= j < F.  m_f is the mean of the P samples of the
 *               segment for detrend = PHAST_DETREND_CONSTANT (scipy's default) and 0 for PHAST_DETREND_NONE.  X_f = rfft_F(r_f).
 *     scale     PHAST_PSD_DENSITY: sigma = 1 / (fs sum w^2).  PHAST_PSD_SPECTRUM: sigma = 1 / (sum w)^2.  sigma is computed at
 *               _new in double from the values given; a window whose sum w^2 (density) or sum w (spectrum) is 0, and
 *               fs <= 0, are PHAST_ERR_INVALID_ARG.
 *     one side  c_k = 2 for every bin, but c_0 = 1 and c_{F/2} = 1 when F is even.
 *     auto      P_xx[k] = sigma c_k (1/S) sum_f |X_f[k]|^2
 *     cross     P_xy[k] = sigma c_k (1/S) sum_f conj(X_f[k]) Y_f[k] (scipy's csd convention), two planes: re and im.  The cross
 *               call also returns P_xx and P_yy from the same pass where d_pxx / d_pyy are not NULL (coherence needs all three).
 *     average   1: the outputs are [batch][bins], packed.  0 (spectrogram): no sum over f and no 1/S; the outputs are
 *               frame-major, [batch][S][bins], laid out as the STFT's planes (scipy.signal.spectrogram returns the transpose).
 * Numerics: m_f is accumulated and kept in double for both types -- as the segment's first sample and the double mean of the
 * differences from it, so that an offset of the signal costs nothing --, x - m_f is formed in double, multiplied by w and
 * then rounded to T.  The sums over frames are formed and carried in double, partial sums in the workspace included, and rounded
 * to T once, at the final store: the f32 error does not grow with S.  The frames of a signal are summed in slabs of
 * _slab(p) frames (a function of S and bins alone), every sum in ascending frame order, without atomics: the result's bits
 * do not depend on the batch, on work_len, on the stream or on a graph replay wherever the real transform's do not (F not a
 * power of two; powers of two up to 4096).
 * Out of scope: linear detrend, average = "median", two-sided output, complex input, scipy's boundary / padded extension,
 * modes other than psd, one window per signal of a batch.
 * The caller's device workspace holds phast_planner_psd*_workspace_len(p, batch, cross) elements of T (cross = 1: for the
 * phast_csd_* calls): all frames of the batch in one chunk, their spectrum planes, the means, the partial rows and the real
 * planner's own workspace.  Any work_len >= _workspace_min(p, cross) runs the flattened (signal, frame) index in chunks of
 * whole frames.  Signal b starts at d_x + b sig_dist (sig_dist >= L; batch 1 ignores it).  The inputs are not written.
 * Every argument rule is checked before the device is touched; the codes are the STFT's.  The *_with_planner forms take host
 * slices of one signal (out_len = bins, or S bins for average = 0), stage through a device buffer of their own and block. */
#define PHAST_DETREND_NONE 0
#define PHAST_DETREND_CONSTANT 1
#define PHAST_PSD_DENSITY 0
#define PHAST_PSD_SPECTRUM 1
typedef struct phast_planner_psd64 phast_planner_psd64; /* PlannerPsd64 */
int phast_planner_psd64_new(size_t signal_len, size_t nperseg, size_t hop, size_t nfft, const double *window, int detrend, int scaling, double fs,
                             phast_planner_psd64 **out);
void phast_planner_psd64_free(phast_planner_psd64 *p);
int phast_planner_psd64_describe(const phast_planner_psd64 *p, char *buf, size_t buf_len);
size_t phast_planner_psd64_device_bytes(const phast_planner_psd64 *p);
size_t phast_planner_psd64_segments(const phast_planner_psd64 *p);
size_t phast_planner_psd64_bins(const phast_planner_psd64 *p);
size_t phast_planner_psd64_slab(const phast_planner_psd64 *p); /* Q: the frames per slab of the sum over frames */
size_t phast_planner_psd64_workspace_len(const phast_planner_psd64 *p, size_t batch, int cross);
size_t phast_planner_psd64_workspace_min(const phast_planner_psd64 *p, int cross);
int phast_psd_f64_with_planner(const double *signal, size_t signal_len, double *out, size_t out_len, int average, const phast_planner_psd64 *planner);
int phast_csd_f64_with_planner(const double *x, size_t x_len, const double *y, size_t y_len, double *out_re, size_t re_len, double *out_im, size_t im_len,
                              double *pxx, size_t pxx_len, double *pyy, size_t pyy_len, int average, const phast_planner_psd64 *planner);
int phast_psd_f64_dev(const double *d_x, double *d_out, size_t signal_len, size_t batch, size_t sig_dist, int average,
                     const phast_planner_psd64 *planner, double *d_work, size_t work_len, void *stream);
int phast_csd_f64_dev(const double *d_x, const double *d_y, double *d_out_re, double *d_out_im, double *d_pxx, double *d_pyy, size_t signal_len, size_t batch,
                     size_t sig_dist, int average, const phast_planner_psd64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/psd_rate.py): stage_ms[3] = average milliseconds of the mean and frame sweeps, of the real transform
 * and of the accumulate and final sweeps (average = 0: the point sweep) over `reps` auto-spectrum calls of `batch` signals at
 * distance L in ONE chunk (work_len >= phast_planner_psd*_workspace_len(p, batch, 0)).  slab: 0, or the frames per slab to sum
 * with instead of _slab(p) (not less than it; slab = segments is one slab: what the slab rule buys).  Blocks until done. */
int phast_planner_psd64_time_stages(const phast_planner_psd64 *p, double *d_signal, double *d_out, size_t batch, int average, size_t slab, double *d_work, size_t work_len,
                                     int reps, float *stage_ms, void *stream);
typedef struct phast_planner_psd32 phast_planner_psd32; /* PlannerPsd32 */
int phast_planner_psd32_new(size_t signal_len, size_t nperseg, size_t hop, size_t nfft, const double *window, int detrend, int scaling, double fs,
                             phast_planner_psd32 **out);
void phast_planner_psd32_free(phast_planner_psd32 *p);
int phast_planner_psd32_describe(const phast_planner_psd32 *p, char *buf, size_t buf_len);
size_t phast_planner_psd32_device_bytes(const phast_planner_psd32 *p);
size_t phast_planner_psd32_segments(const phast_planner_psd32 *p);
size_t phast_planner_psd32_bins(const phast_planner_psd32 *p);
size_t phast_planner_psd32_slab(const phast_planner_psd32 *p); /* Q: the frames per slab of the sum over frames */
size_t phast_planner_psd32_workspace_len(const phast_planner_psd32 *p, size_t batch, int cross);
size_t phast_planner_psd32_workspace_min(const phast_planner_psd32 *p, int cross);
int phast_psd_f32_with_planner(const float *signal, size_t signal_len, float *out, size_t out_len, int average, const phast_planner_psd32 *planner);
int phast_csd_f32_with_planner(const float *x, size_t x_len, const float *y, size_t y_len, float *out_re, size_t re_len, float *out_im, size_t im_len,
                              float *pxx, size_t pxx_len, float *pyy, size_t pyy_len, int average, const phast_planner_psd32 *planner);
int phast_psd_f32_dev(const float *d_x, float *d_out, size_t signal_len, size_t batch, size_t sig_dist, int average,
                     const phast_planner_psd32 *planner, float *d_work, size_t work_len, void *stream);
int phast_csd_f32_dev(const float *d_x, const float *d_y, float *d_out_re, float *d_out_im, float *d_pxx, float *d_pyy, size_t signal_len, size_t batch,
                     size_t sig_dist, int average, const phast_planner_psd32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/psd_rate.py): stage_ms[3] = average milliseconds of the mean and frame sweeps, of the real transform
 * and of the accumulate and final sweeps (average = 0: the point sweep) over `reps` auto-spectrum calls of `batch` signals at
 * distance L in ONE chunk (work_len >= phast_planner_psd*_workspace_len(p, batch, 0)).  slab: 0, or the frames per slab to sum
 * with instead of _slab(p) (not less than it; slab = segments is one slab: what the slab rule buys).  Blocks until done. */
int phast_planner_psd32_time_stages(const phast_planner_psd32 *p, float *d_signal, float *d_out, size_t batch, int average, size_t slab, float *d_work, size_t work_len,
                                     int reps, float *stage_ms, void *stream);

/* ---- the generalised Lomb-Scargle periodogram of unevenly spaced samples (no reference counterpart;
 * scipy.signal.lombscargle, 1.15).  M times t_j and K frequencies f_k (host doubles, f in cycles per unit of t:
 * scipy's angular freqs over 2 pi), optional weights w_j >= 0 with sum w > 0 (normalised to sum 1; NULL: 1 / M),
 * floating_mean (0 / 1), fixed at _new; the values y_j per call.  With phi = 2 pi f_k t_j:
 *     tables    A0 = sum w e^{i phi} = C + i S, A2 = sum w e^{2 i phi} = C2 + i S2; CC = (1 + C2) / 2, SS = (1 - C2) / 2,
 *               CS = S2 / 2; floating mean: CC -= C^2, SS -= S^2, CS -= C S; tau = atan2(2 CS, CC - SS) / 2;
 *               CCt = (1 + C2 cos 2 tau + S2 sin 2 tau) / 2, SSt = 1 - CCt; floating mean: CCt -= (C cos tau + S sin tau)^2,
 *               SSt -= (S cos tau - C sin tau)^2; both clamped from below at finfo(T).epsneg, as scipy does
 *     signal    Y = sum w y (floating mean; else 0), A1 = sum w (y - Y) e^{i phi}; YC = Re A1 cos tau + Im A1 sin tau,
 *               YS = Im A1 cos tau - Re A1 sin tau, a = YC / CCt, b = YS / SSt, P = 2 (a YC + b YS)
 *     PHAST_LOMB_POWER: P M / 4.  PHAST_LOMB_NORMALIZE: P / (2 YY), YY = sum w (y - Y)^2.  PHAST_LOMB_AMPLITUDE: the complex
 *               (a + i b) e^{i tau} into out_re and out_im; out_im is required for amplitude only and not written otherwise.
 * A call is one type-3 transform (Reverse, eps) of the real strengths T(w (y - Y)) between new sweeps; the tables are built at
 * _new in double for both types by temporary f64 type-3 transforms of the weights at f and at 2 f, and rounded to T.
 * Numerics: Y is accumulated and kept in double for both types -- as the signal's first value plus the weighted mean of the
 * differences from it -- and taken off BEFORE the transform, so that an offset of the signal costs nothing; YY likewise.  The
 * points of a signal are summed in slabs of _slab(p) points (a function of M alone), every sum in a fixed order, without
 * atomics: the result's bits do not depend on the batch, on work_len, on alignment, on the stream or on a graph replay.
 * _new refuses with PHAST_ERR_INVALID_ARG, before the device is touched: NULL t or freqs, M or K outside 1 .. 2^30, a
 * non-finite t, f or w, a negative w, sum w <= 0, eps outside the type-3 planner's range for the type, and a type-3 grid --
 * of (t, f) or of (t, 2 f) -- above that planner's limit.
 * Out of scope: times in device memory, a fast path for times on a grid, multi-term models, false-alarm probabilities.
 * The caller's device workspace holds phast_planner_lomb*_workspace_len(p, batch) elements of T: the strengths, A1's planes,
 * the type-3 workspace and the doubles of the reductions of all signals in one chunk.  Any work_len >= _workspace_min(p) runs
 * the batch in chunks of whole signals.  Signal b starts at d_y + b sig_dist (>= M), its results at d_out + b out_dist (>= K);
 * batch 1 ignores both.  The inputs are not written.  The *_with_planner forms take host slices of one signal and block. */
#define PHAST_LOMB_POWER 0
#define PHAST_LOMB_NORMALIZE 1
#define PHAST_LOMB_AMPLITUDE 2
typedef struct phast_planner_lomb64 phast_planner_lomb64; /* PlannerLomb64 */
int phast_planner_lomb64_new(const double *t, size_t m, const double *freqs, size_t k, const double *weights_or_null, int floating_mean, double eps,
                              phast_planner_lomb64 **out);
void phast_planner_lomb64_free(phast_planner_lomb64 *p);
int phast_planner_lomb64_describe(const phast_planner_lomb64 *p, char *buf, size_t buf_len);
size_t phast_planner_lomb64_device_bytes(const phast_planner_lomb64 *p);
size_t phast_planner_lomb64_slab(const phast_planner_lomb64 *p); /* Q: the points per slab of the two reductions */
size_t phast_planner_lomb64_grid_len(const phast_planner_lomb64 *p); /* n_f of the inner type-3 planner */
size_t phast_planner_lomb64_workspace_len(const phast_planner_lomb64 *p, size_t batch);
size_t phast_planner_lomb64_workspace_min(const phast_planner_lomb64 *p);
int phast_lombscargle_f64(const double *t, size_t m, const double *freqs, size_t k, const double *weights_or_null, int floating_mean, double eps,
                         const double *y, double *out_re, double *out_im, int normalize);
int phast_lombscargle_f64_with_planner(const double *y, size_t m, double *out_re, size_t re_len, double *out_im, size_t im_len, int normalize,
                                      const phast_planner_lomb64 *planner);
int phast_lombscargle_f64_dev(const double *d_y, double *d_out_re, double *d_out_im, size_t m, size_t batch, size_t sig_dist, size_t out_dist, int normalize,
                             const phast_planner_lomb64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/lomb_rate.py): stage_ms[3] = average milliseconds of the sweeps in front of the transform (partial,
 * final, strength, final), of the type-3 call and of the post sweep over `reps` calls of `batch` signals at the natural
 * distances in ONE chunk (work_len >= phast_planner_lomb*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_lomb64_time_stages(const phast_planner_lomb64 *p, const double *d_y, double *d_out_re, double *d_out_im, size_t batch, int normalize, double *d_work, size_t work_len,
                                      int reps, float *stage_ms, void *stream);
typedef struct phast_planner_lomb32 phast_planner_lomb32; /* PlannerLomb32 */
int phast_planner_lomb32_new(const double *t, size_t m, const double *freqs, size_t k, const double *weights_or_null, int floating_mean, double eps,
                              phast_planner_lomb32 **out);
void phast_planner_lomb32_free(phast_planner_lomb32 *p);
int phast_planner_lomb32_describe(const phast_planner_lomb32 *p, char *buf, size_t buf_len);
size_t phast_planner_lomb32_device_bytes(const phast_planner_lomb32 *p);
size_t phast_planner_lomb32_slab(const phast_planner_lomb32 *p); /* Q: the points per slab of the two reductions */
size_t phast_planner_lomb32_grid_len(const phast_planner_lomb32 *p); /* n_f of the inner type-3 planner */
size_t phast_planner_lomb32_workspace_len(const phast_planner_lomb32 *p, size_t batch);
size_t phast_planner_lomb32_workspace_min(const phast_planner_lomb32 *p);
int phast_lombscargle_f32(const double *t, size_t m, const double *freqs, size_t k, const double *weights_or_null, int floating_mean, double eps,
                         const float *y, float *out_re, float *out_im, int normalize);
int phast_lombscargle_f32_with_planner(const float *y, size_t m, float *out_re, size_t re_len, float *out_im, size_t im_len, int normalize,
                                      const phast_planner_lomb32 *planner);
int phast_lombscargle_f32_dev(const float *d_y, float *d_out_re, float *d_out_im, size_t m, size_t batch, size_t sig_dist, size_t out_dist, int normalize,
                             const phast_planner_lomb32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/lomb_rate.py): stage_ms[3] = average milliseconds of the sweeps in front of the transform (partial,
 * final, strength, final), of the type-3 call and of the post sweep over `reps` calls of `batch` signals at the natural
 * distances in ONE chunk (work_len >= phast_planner_lomb*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_lomb32_time_stages(const phast_planner_lomb32 *p, const float *d_y, float *d_out_re, float *d_out_im, size_t batch, int normalize, float *d_work, size_t work_len,
                                      int reps, float *stage_ms, void *stream);

/* ---- sample-rate conversion of real signals (no reference counterpart; scipy.signal.upfirdn / resample_poly / decimate and
 * scipy.signal.resample, 1.15).
 *
 * Polyphase FIR: phast_planner_upfirdn*.  Signal x of L samples, K taps h (host values of T), up, down >= 1, used as given (not
 * reduced by their gcd, as scipy.signal.upfirdn does not reduce them):
 *     full[m] = sum_n h[m down - n up] x[n],  0 <= m < full_len = ((L - 1) up + K - 1) / down + 1;  full[m] = 0 above
 *     out[i]  = full[first + i],              0 <= i < out_len     (out_len = 0 at _new: full_len - first)
 * This is upfirdn(h, x, up, down) with mode "constant", windowed by (first, out_len); first + out_len may pass full_len (zeros).
 * One direct kernel, no transform: the taps are kept phase-major on the device (up rows of Kp = ceil(K / up), zero-padded), a
 * 256-thread workgroup owns a tile of consecutive outputs of one signal and walks the rows in tap chunks that share LDS with
 * the run of the signal they meet.  An output is acc = fma(h[p + j up], x[q - j], acc) for j = 0 .. Kp - 1 ascending from 0
 * (p = (m down) mod up, q = (m down) div up), in T: the result's bits depend on the values alone -- not on the batch, the
 * distances, pointer alignment, the workspace, the stream or a graph replay.  No workspace is needed: _workspace_len is 0, and
 * d_work / work_len of the _dev call are not read (NULL and 0 are fine).
 * _new refuses with PHAST_ERR_INVALID_ARG, before the device is touched: NULL taps, L, K or the resulting out_len outside
 * 1 .. 2^29, up or down outside 1 .. 2^20, first > full_len.  _dev: signal b at d_signal + b sig_dist (>= L), its out_len
 * outputs at d_out + b out_dist (>= out_len); batch 1 ignores both; pointers need element alignment only; the signal is never
 * written and nothing is written outside the out_len outputs of a signal.  A null pointer or a short dist is
 * PHAST_ERR_INVALID_ARG, a signal_len that is not the planner's PHAST_ERR_PLANNER_SIZE, a wrong out_len of the host-slice form
 * PHAST_ERR_LEN_MISMATCH -- all before the device is touched.  The *_with_planner forms take host slices of one signal and block. */
typedef struct phast_planner_upfirdn64 phast_planner_upfirdn64; /* PlannerUpfirdn64 */
int phast_planner_upfirdn64_new(size_t signal_len, const double *taps, size_t num_taps, size_t up, size_t down, size_t first, size_t out_len,
                                 phast_planner_upfirdn64 **out);
void phast_planner_upfirdn64_free(phast_planner_upfirdn64 *p);
int phast_planner_upfirdn64_describe(const phast_planner_upfirdn64 *p, char *buf, size_t buf_len);
size_t phast_planner_upfirdn64_device_bytes(const phast_planner_upfirdn64 *p);
size_t phast_planner_upfirdn64_workspace_len(const phast_planner_upfirdn64 *p, size_t batch); /* 0 */
size_t phast_planner_upfirdn64_out_len(const phast_planner_upfirdn64 *p);
size_t phast_planner_upfirdn64_full_len(const phast_planner_upfirdn64 *p);
size_t phast_planner_upfirdn64_tile(const phast_planner_upfirdn64 *p);  /* outputs per workgroup */
size_t phast_planner_upfirdn64_chunk(const phast_planner_upfirdn64 *p); /* taps of a phase per LDS chunk */
int phast_upfirdn_f64_with_planner(const double *signal, size_t signal_len, double *out, size_t out_len, const phast_planner_upfirdn64 *planner);
int phast_upfirdn_f64_dev(const double *d_signal, double *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                         const phast_planner_upfirdn64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/resample_rate.py): stage_ms[1] = average milliseconds of the kernel over `reps` calls of `batch`
 * signals at the natural distances.  Blocks until done. */
int phast_planner_upfirdn64_time_stages(const phast_planner_upfirdn64 *p, const double *d_signal, double *d_out, size_t batch, int reps, float *stage_ms,
                                         void *stream);
typedef struct phast_planner_upfirdn32 phast_planner_upfirdn32; /* PlannerUpfirdn32 */
int phast_planner_upfirdn32_new(size_t signal_len, const float *taps, size_t num_taps, size_t up, size_t down, size_t first, size_t out_len,
                                 phast_planner_upfirdn32 **out);
void phast_planner_upfirdn32_free(phast_planner_upfirdn32 *p);
int phast_planner_upfirdn32_describe(const phast_planner_upfirdn32 *p, char *buf, size_t buf_len);
size_t phast_planner_upfirdn32_device_bytes(const phast_planner_upfirdn32 *p);
size_t phast_planner_upfirdn32_workspace_len(const phast_planner_upfirdn32 *p, size_t batch); /* 0 */
size_t phast_planner_upfirdn32_out_len(const phast_planner_upfirdn32 *p);
size_t phast_planner_upfirdn32_full_len(const phast_planner_upfirdn32 *p);
size_t phast_planner_upfirdn32_tile(const phast_planner_upfirdn32 *p);  /* outputs per workgroup */
size_t phast_planner_upfirdn32_chunk(const phast_planner_upfirdn32 *p); /* taps of a phase per LDS chunk */
int phast_upfirdn_f32_with_planner(const float *signal, size_t signal_len, float *out, size_t out_len, const phast_planner_upfirdn32 *planner);
int phast_upfirdn_f32_dev(const float *d_signal, float *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                         const phast_planner_upfirdn32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/resample_rate.py): stage_ms[1] = average milliseconds of the kernel over `reps` calls of `batch`
 * signals at the natural distances.  Blocks until done. */
int phast_planner_upfirdn32_time_stages(const phast_planner_upfirdn32 *p, const float *d_signal, float *d_out, size_t batch, int reps, float *stage_ms,
                                         void *stream);
/* Fourier method: phast_planner_resample*.  scipy.signal.resample(x, num) of a real signal of L samples (window None, domain
 * "time"), 1 <= L, num <= 2^29:
 *     X = rfft_L(x); N = min(L, num); Y[k] = X[k] for k <= N / 2, 0 for the other k <= num / 2;
 *     N even and num < L: Y[N / 2] *= 2; N even and num > L: Y[N / 2] *= 1/2;  y = irfft_num(Y) num / L
 * One R2C of L and one C2R of num on the any-length real path (phast_planner_r2c_any*; one planner serves both when
 * num = L) around one new sweep, which copies, zero-fills and scales the two planes: num / L, the Nyquist factor, and the
 * imaginary parts of Y[0] and (num even) Y[num / 2] set to 0, as irfft defines them.  The caller's device workspace holds
 * _workspace_len(p, batch) elements of T: the planes of X and Y of all signals and the real planners' workspace in one chunk;
 * any work_len >= _workspace_min(p) runs the batch in chunks of whole signals, to the same bits.  Signal b at d_signal +
 * b sig_dist (>= L), its num outputs at d_out + b out_dist (>= num); batch 1 ignores both; pointers need element alignment
 * only; as for phast_r2c_fft_*_any_dev, a power-of-two L >= 4 needs an even sig_dist in a batch and a power-of-two num >= 4 an
 * even out_dist.  PHAST_ERR_INVALID_ARG (lengths out of range, null pointers, short dists, a null or short workspace),
 * PHAST_ERR_PLANNER_SIZE (signal_len) and PHAST_ERR_LEN_MISMATCH (out_len of the host-slice form) come back before the device
 * is touched.  Out of scope: complex signals, the window argument, automatic dispatch between the two methods. */
typedef struct phast_planner_resample64 phast_planner_resample64; /* PlannerResample64 */
int phast_planner_resample64_new(size_t signal_len, size_t num, phast_planner_resample64 **out);
void phast_planner_resample64_free(phast_planner_resample64 *p);
int phast_planner_resample64_describe(const phast_planner_resample64 *p, char *buf, size_t buf_len);
size_t phast_planner_resample64_device_bytes(const phast_planner_resample64 *p);
size_t phast_planner_resample64_workspace_len(const phast_planner_resample64 *p, size_t batch);
size_t phast_planner_resample64_workspace_min(const phast_planner_resample64 *p);
int phast_resample_f64_with_planner(const double *signal, size_t signal_len, double *out, size_t out_len, const phast_planner_resample64 *planner);
int phast_resample_f64_dev(const double *d_signal, double *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                          const phast_planner_resample64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/resample_rate.py): stage_ms[3] = average milliseconds of the R2C, the spectrum sweep and the C2R over
 * `reps` calls of `batch` signals at the natural distances in ONE chunk (work_len >= _workspace_len(p, batch)).  Blocks. */
int phast_planner_resample64_time_stages(const phast_planner_resample64 *p, const double *d_signal, double *d_out, size_t batch, double *d_work, size_t work_len,
                                          int reps, float *stage_ms, void *stream);
typedef struct phast_planner_resample32 phast_planner_resample32; /* PlannerResample32 */
int phast_planner_resample32_new(size_t signal_len, size_t num, phast_planner_resample32 **out);
void phast_planner_resample32_free(phast_planner_resample32 *p);
int phast_planner_resample32_describe(const phast_planner_resample32 *p, char *buf, size_t buf_len);
size_t phast_planner_resample32_device_bytes(const phast_planner_resample32 *p);
size_t phast_planner_resample32_workspace_len(const phast_planner_resample32 *p, size_t batch);
size_t phast_planner_resample32_workspace_min(const phast_planner_resample32 *p);
int phast_resample_f32_with_planner(const float *signal, size_t signal_len, float *out, size_t out_len, const phast_planner_resample32 *planner);
int phast_resample_f32_dev(const float *d_signal, float *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                          const phast_planner_resample32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/resample_rate.py): stage_ms[3] = average milliseconds of the R2C, the spectrum sweep and the C2R over
 * `reps` calls of `batch` signals at the natural distances in ONE chunk (work_len >= _workspace_len(p, batch)).  Blocks. */
int phast_planner_resample32_time_stages(const phast_planner_resample32 *p, const float *d_signal, float *d_out, size_t batch, float *d_work, size_t work_len,
                                          int reps, float *stage_ms, void *stream);

/* ---- polyphase filter-bank channelizer: the analysis side of a uniform DFT filter bank (no reference counterpart; cuSignal's
 * channelize_poly).  Signal x of L samples -- real: one plane; complex: planes re and im --, K real taps h (host
 * values of T), M channels, hop D, zero extension as phast_planner_upfirdn*:
 *     full_frames = (L + K - 2) / D + 1
 *     y[m][k] = sum_n h[m D - n] x[n] exp(-2 pi i k n / M),  0 <= m < full_frames, 0 <= k < M;  y[m] = 0 above
 *     out[i]  = y[first_frame + i],                          0 <= i < out_frames   (out_frames = 0 at _new: full_frames - first_frame)
 * Channel k is upfirdn(h, x exp(-2 pi i k n / M), 1, D): the phase is referred to absolute sample time, so the channels are
 * baseband streams for any D (D = M: critically sampled; D < M: oversampled; D > M is legal).  first_frame + out_frames may pass
 * full_frames (zeros).  Output planes, dense and frame-major: element (b out_frames + i) bins + k, bins = M for a complex signal
 * and M / 2 + 1 for a real one (y[m][M - k] = conj y[m][k]).
 * Method: one fold kernel, u[m][p] = sum_{j < T} h[r0 + j M] x[m D - r0 - j M] with r0 = (m D - p) mod M and T = ceil(K / M), then
 * one M-point transform per frame on the any-length path (phast_planner_any* / phast_planner_r2c_any*).  An element of the fold is
 * acc = fma(h[r0 + j M], x[m D - r0 - j M], acc) for j = 0 .. T - 1 ascending from 0 in T, so the result's bits depend on the
 * values alone -- not on the batch, the distances, pointer alignment, the workspace, the stream or a graph replay.
 * Complex signals: the fold writes the caller's output planes and the transform runs in place; the workspace
 * (_workspace_len(p, batch) elements of T) is the transform's alone, 0 for a power-of-two M.  Real signals: the fold goes into
 * workspace rows and the R2C from there into the output; any work_len >= _workspace_min(p) (one frame) runs the frames in chunks,
 * to the same bits.  Where _workspace_min is 0, d_work may be NULL.
 * _new refuses with PHAST_ERR_INVALID_ARG, before the device is touched: NULL taps; L, K, M or D outside 1 .. 2^29; first_frame >
 * full_frames; out_frames (resolved) < 1 or out_frames M > 2^30.  _dev: signal b at d_sig_re (d_sig_im) + b sig_dist (>= L; batch 1
 * ignores it); d_sig_im must be NULL for a real planner and non-NULL for a complex one; pointers need element alignment only;
 * the signal is never written; input and output must not overlap (identical pointers are refused).  A null pointer, the wrong
 * d_sig_im, a short dist, a null or short workspace: PHAST_ERR_INVALID_ARG; a signal_len that is not the planner's:
 * PHAST_ERR_PLANNER_SIZE; an out_len of the host-slice form that is not out_frames bins: PHAST_ERR_LEN_MISMATCH -- all before the
 * device is touched.  The *_with_planner forms take host slices of one signal (sig_im NULL for a real planner) and block.
 * The synthesis bank (the inverse) is phast_planner_synthesizer* below.  Out of scope: complex taps, subsets of the channels,
 * any choice of method by size. */
typedef struct phast_planner_channelizer64 phast_planner_channelizer64; /* PlannerChannelizer64 */
int phast_planner_channelizer64_new(size_t signal_len, const double *taps, size_t num_taps, size_t channels, size_t hop, size_t first_frame, size_t out_frames,
                                     int complex_input, phast_planner_channelizer64 **out);
void phast_planner_channelizer64_free(phast_planner_channelizer64 *p);
int phast_planner_channelizer64_describe(const phast_planner_channelizer64 *p, char *buf, size_t buf_len);
size_t phast_planner_channelizer64_device_bytes(const phast_planner_channelizer64 *p);
size_t phast_planner_channelizer64_workspace_len(const phast_planner_channelizer64 *p, size_t batch);
size_t phast_planner_channelizer64_workspace_min(const phast_planner_channelizer64 *p);
size_t phast_planner_channelizer64_out_frames(const phast_planner_channelizer64 *p);
size_t phast_planner_channelizer64_full_frames(const phast_planner_channelizer64 *p);
size_t phast_planner_channelizer64_bins(const phast_planner_channelizer64 *p);
size_t phast_planner_channelizer64_tile_frames(const phast_planner_channelizer64 *p); /* frames per workgroup */
size_t phast_planner_channelizer64_tile_cols(const phast_planner_channelizer64 *p);   /* columns per workgroup */
size_t phast_planner_channelizer64_chunk(const phast_planner_channelizer64 *p);       /* tap rows per LDS chunk */
size_t phast_planner_channelizer64_periods(const phast_planner_channelizer64 *p);     /* periods of the signal in LDS */
int phast_channelize_f64_with_planner(const double *sig_re, const double *sig_im, size_t signal_len, double *out_re, double *out_im, size_t out_len,
                                       const phast_planner_channelizer64 *planner);
int phast_channelize_f64_dev(const double *d_sig_re, const double *d_sig_im, double *d_out_re, double *d_out_im, size_t signal_len, size_t batch, size_t sig_dist,
                              const phast_planner_channelizer64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/channelizer_rate.py): stage_ms[2] = average milliseconds of the fold and of the transform over `reps`
 * calls of `batch` signals at distance L in ONE chunk (work_len >= _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_channelizer64_time_stages(const phast_planner_channelizer64 *p, const double *d_sig_re, const double *d_sig_im, double *d_out_re, double *d_out_im, size_t batch, double *d_work, size_t work_len,
                                             int reps, float *stage_ms, void *stream);
typedef struct phast_planner_channelizer32 phast_planner_channelizer32; /* PlannerChannelizer32 */
int phast_planner_channelizer32_new(size_t signal_len, const float *taps, size_t num_taps, size_t channels, size_t hop, size_t first_frame, size_t out_frames,
                                     int complex_input, phast_planner_channelizer32 **out);
void phast_planner_channelizer32_free(phast_planner_channelizer32 *p);
int phast_planner_channelizer32_describe(const phast_planner_channelizer32 *p, char *buf, size_t buf_len);
size_t phast_planner_channelizer32_device_bytes(const phast_planner_channelizer32 *p);
size_t phast_planner_channelizer32_workspace_len(const phast_planner_channelizer32 *p, size_t batch);
size_t phast_planner_channelizer32_workspace_min(const phast_planner_channelizer32 *p);
size_t phast_planner_channelizer32_out_frames(const phast_planner_channelizer32 *p);
size_t phast_planner_channelizer32_full_frames(const phast_planner_channelizer32 *p);
size_t phast_planner_channelizer32_bins(const phast_planner_channelizer32 *p);
size_t phast_planner_channelizer32_tile_frames(const phast_planner_channelizer32 *p); /* frames per workgroup */
size_t phast_planner_channelizer32_tile_cols(const phast_planner_channelizer32 *p);   /* columns per workgroup */
size_t phast_planner_channelizer32_chunk(const phast_planner_channelizer32 *p);       /* tap rows per LDS chunk */
size_t phast_planner_channelizer32_periods(const phast_planner_channelizer32 *p);     /* periods of the signal in LDS */
int phast_channelize_f32_with_planner(const float *sig_re, const float *sig_im, size_t signal_len, float *out_re, float *out_im, size_t out_len,
                                       const phast_planner_channelizer32 *planner);
int phast_channelize_f32_dev(const float *d_sig_re, const float *d_sig_im, float *d_out_re, float *d_out_im, size_t signal_len, size_t batch, size_t sig_dist,
                              const phast_planner_channelizer32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/channelizer_rate.py): stage_ms[2] = average milliseconds of the fold and of the transform over `reps`
 * calls of `batch` signals at distance L in ONE chunk (work_len >= _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_channelizer32_time_stages(const phast_planner_channelizer32 *p, const float *d_sig_re, const float *d_sig_im, float *d_out_re, float *d_out_im, size_t batch, float *d_work, size_t work_len,
                                             int reps, float *stage_ms, void *stream);

/* ---- polyphase synthesis filter bank: the inverse side of the channelizer above (no reference counterpart).
 * Channel data Y[m][k] of F frames by M channels, K real taps g (host values of T), hop D, zero extension as
 * phast_planner_upfirdn*:
 *     full_len = (F - 1) D + K
 *     s[n]   = sum_m g[n - m D] sum_k Y[m][k] exp(+2 pi i k n / M),  0 <= n < full_len;  s[n] = 0 above
 *     out[i] = s[first + i],                                         0 <= i < out_len   (out_len = 0 at _new: full_len - first)
 * so s = sum_k exp(2 pi i k n / M) upfirdn(g, Y[:, k], D, 1): the phase is referred to absolute sample time, as on the analysis
 * side, and the sum over k is unnormalised.  first + out_len may pass full_len (zeros).  Input planes, dense and frame-major as
 * the channelizer writes them: element (b F + m) bins + k.  complex_output: bins = M and the signal is two planes; otherwise
 * bins = M / 2 + 1, the Hermitian half, read by irfft's rules (the imaginary parts of bin 0 and, for even M, of bin M / 2 are
 * ignored), and the signal is one plane.  Signal b lies at d_out_re (d_out_im) + b out_dist.
 * Because the phases are in absolute time, the delay of an analysis / synthesis pair must be a multiple of M for the columns
 * to line up: with analysis taps h of K = M T points, g = (0, h[K - 1], ..., h[0]) of K + 1 points gives the adjoint of the
 * channelizer delayed by K, and with h[j] = sin(pi (j + 1/2) / M), K = M, D = M / 2 and that g divided by M the pair
 * reconstructs the signal delayed by M.
 * Method: one M-point inverse transform per frame on the any-length path (phast_planner_any* / phast_planner_c2r_any*) into
 * workspace rows, v[m][p], then one gather kernel, the unfold: s[n] = sum_m tab[n - m D] v[m][n mod M] over the frames
 * max(0, ceil((n - K + 1) / D)) .. min(F - 1, n / D).  (Complex output goes through a copy of both planes into those rows; real
 * output of an even M >= 4 through a copy of the imaginary plane with bin 0 and bin M / 2 set to 0, which the engine's C2R
 * would otherwise use.)  The transform carries 1 / M, so the planner keeps tab[j] = M g[j], the
 * product in double, rounded once to T.  An output is acc = fma(tab[n - m D], v[m][n mod M], acc) for m ascending from 0 in T,
 * so the result's bits depend on the values alone -- not on the batch, the distances, pointer alignment, the workspace, the
 * stream or a graph replay.
 * Workspace: _workspace_len(p, batch) elements of T hold every frame of the batch; any work_len >= _workspace_min(p) (one
 * signal's frames: an output sample needs all of them) runs whole signals in chunks, to the same bits.  Complex output of one
 * channel needs none, and d_work may then be NULL.
 * _new refuses with PHAST_ERR_INVALID_ARG, before the device is touched: NULL taps; F, K, M or D outside 1 .. 2^29; F M > 2^30;
 * first > full_len; out_len (resolved) < 1 or > 2^30.  _dev: d_out_im must be NULL for a real planner and non-NULL for a complex
 * one; out_dist >= out_len (batch 1 ignores it); pointers need element alignment only; the input is never written; input and
 * output must not overlap (identical pointers are refused).  A null pointer, the wrong d_out_im, a short dist, a null or short
 * workspace: PHAST_ERR_INVALID_ARG; a `frames` that is not the planner's (host form: an in_len that is not F bins):
 * PHAST_ERR_PLANNER_SIZE; an out_len of the host-slice form that is not the planner's: PHAST_ERR_LEN_MISMATCH -- all before the
 * device is touched.  The *_with_planner forms take host slices of one signal's frames (out_im NULL for a real planner) and block.
 * Out of scope: complex taps, subsets of the channels, fusing the unfold behind the transform's last pass. */
typedef struct phast_planner_synthesizer64 phast_planner_synthesizer64; /* PlannerSynthesizer64 */
int phast_planner_synthesizer64_new(size_t frames, const double *taps, size_t num_taps, size_t channels, size_t hop, size_t first, size_t out_len,
                                     int complex_output, phast_planner_synthesizer64 **out);
void phast_planner_synthesizer64_free(phast_planner_synthesizer64 *p);
int phast_planner_synthesizer64_describe(const phast_planner_synthesizer64 *p, char *buf, size_t buf_len);
size_t phast_planner_synthesizer64_device_bytes(const phast_planner_synthesizer64 *p);
size_t phast_planner_synthesizer64_workspace_len(const phast_planner_synthesizer64 *p, size_t batch);
size_t phast_planner_synthesizer64_workspace_min(const phast_planner_synthesizer64 *p);
size_t phast_planner_synthesizer64_out_len(const phast_planner_synthesizer64 *p);
size_t phast_planner_synthesizer64_full_len(const phast_planner_synthesizer64 *p);
size_t phast_planner_synthesizer64_bins(const phast_planner_synthesizer64 *p);
size_t phast_planner_synthesizer64_tile_samples(const phast_planner_synthesizer64 *p); /* output samples per workgroup */
size_t phast_planner_synthesizer64_per_thread(const phast_planner_synthesizer64 *p);   /* output samples per thread */
size_t phast_planner_synthesizer64_max_terms(const phast_planner_synthesizer64 *p);    /* terms of an output at most: ceil(K / D) */
int phast_synthesize_f64_with_planner(const double *in_re, const double *in_im, size_t in_len, double *out_re, double *out_im, size_t out_len,
                                       const phast_planner_synthesizer64 *planner);
int phast_synthesize_f64_dev(const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, size_t frames, size_t batch, size_t out_dist,
                              const phast_planner_synthesizer64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/synthesizer_rate.py): stage_ms[2] = average milliseconds of the transform (with the copy sweep of
 * complex output) and of the unfold over `reps` calls of `batch` signals at distance out_len in ONE chunk (work_len >=
 * _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_synthesizer64_time_stages(const phast_planner_synthesizer64 *p, const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, size_t batch, double *d_work, size_t work_len,
                                             int reps, float *stage_ms, void *stream);
typedef struct phast_planner_synthesizer32 phast_planner_synthesizer32; /* PlannerSynthesizer32 */
int phast_planner_synthesizer32_new(size_t frames, const float *taps, size_t num_taps, size_t channels, size_t hop, size_t first, size_t out_len,
                                     int complex_output, phast_planner_synthesizer32 **out);
void phast_planner_synthesizer32_free(phast_planner_synthesizer32 *p);
int phast_planner_synthesizer32_describe(const phast_planner_synthesizer32 *p, char *buf, size_t buf_len);
size_t phast_planner_synthesizer32_device_bytes(const phast_planner_synthesizer32 *p);
size_t phast_planner_synthesizer32_workspace_len(const phast_planner_synthesizer32 *p, size_t batch);
size_t phast_planner_synthesizer32_workspace_min(const phast_planner_synthesizer32 *p);
size_t phast_planner_synthesizer32_out_len(const phast_planner_synthesizer32 *p);
size_t phast_planner_synthesizer32_full_len(const phast_planner_synthesizer32 *p);
size_t phast_planner_synthesizer32_bins(const phast_planner_synthesizer32 *p);
size_t phast_planner_synthesizer32_tile_samples(const phast_planner_synthesizer32 *p); /* output samples per workgroup */
size_t phast_planner_synthesizer32_per_thread(const phast_planner_synthesizer32 *p);   /* output samples per thread */
size_t phast_planner_synthesizer32_max_terms(const phast_planner_synthesizer32 *p);    /* terms of an output at most: ceil(K / D) */
int phast_synthesize_f32_with_planner(const float *in_re, const float *in_im, size_t in_len, float *out_re, float *out_im, size_t out_len,
                                       const phast_planner_synthesizer32 *planner);
int phast_synthesize_f32_dev(const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, size_t frames, size_t batch, size_t out_dist,
                              const phast_planner_synthesizer32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/synthesizer_rate.py): stage_ms[2] = average milliseconds of the transform (with the copy sweep of
 * complex output) and of the unfold over `reps` calls of `batch` signals at distance out_len in ONE chunk (work_len >=
 * _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_synthesizer32_time_stages(const phast_planner_synthesizer32 *p, const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, size_t batch, float *d_work, size_t work_len,
                                             int reps, float *stage_ms, void *stream);

/* ---- continuous wavelet transform and analytic signal (no reference counterpart; Torrence & Compo 1998, scipy.signal.hilbert;
 * DESIGN.md §30).  Samples at unit spacing, scales in samples (a caller with a sampling interval dt passes s / dt).  A real or
 * complex signal x of L points is zero-extended to P points, L <= P <= 2^29 (pad_len = 0 at _new: P = L); padding is how a
 * caller pushes the wrap-around of the periodic convolution out of the window.  With X = fft_P(x) (numpy's convention) and
 * w_k = 2 pi k / P for k <= P div 2, 2 pi (k - P) / P above (for even P the bin P / 2 counts as positive), for S scales s_j
 * (finite doubles > 0, any order, repeats allowed, at most 2^20):
 *     W[j][n] = ifft_P( X[k] conj( c_j psi0^(s_j w_k) ) )[n],  n < L
 * in two planes: row (b, j) lies at d_out_re (d_out_im) + b out_dist + j L.  Families (Torrence & Compo's table 1 by its
 * frequency-domain column; H(x) = 1 for x > 0, else 0); `param` is w0 or m:
 *     PHAST_CWT_MORLET (w0 > 0, customarily 6)    pi^(-1/4) H(x) exp(-(x - w0)^2 / 2)
 *     PHAST_CWT_PAUL (integer m, 1 .. 85)         2^m / sqrt(m (2m - 1)!) H(x) x^m exp(-x)
 *     PHAST_CWT_DOG (integer m, 1 .. 170)         -(i^m) / sqrt(Gamma(m + 1/2)) x^m exp(-x^2 / 2)     (m = 2: the Mexican hat)
 *     PHAST_CWT_STEP                              1 at k = 0 and at k = P / 2 (even P), 2 for 0 < k < P / 2, 0 above
 * (the caps on m: where (2m - 1)! and Gamma(m + 1/2) stay finite in double).  The transform is defined by these
 * frequency-domain formulas; for odd m of DOG the paper's time-domain column differs by a sign.  STEP does not depend on the
 * scale and ignores `norm` and `param`: with one scale it is the analytic signal, scipy.signal.hilbert(x, N=P)[:L].  Norms:
 *     PHAST_CWT_L2     c_j = sqrt(2 pi s_j)          (Torrence & Compo eq. 6 at dt = 1: unit energy)
 *     PHAST_CWT_PEAK   c_j = 2 / max_x |psi0^(x)|    (a unit sinusoid at the centre frequency has |W| = 1 for Morlet and Paul)
 * Method: one forward transform of P per signal on the any-length path (R2C for a real planner) into workspace planes, one
 * bank kernel that evaluates the filters in registers and writes the S rows, one batched inverse transform in place in the
 * rows.  When P = L the rows are the output planes; when P > L they live in the workspace and a crop copies the first L of
 * each.  s_j w_k, the exponent and the exponential are formed in double in both types, the filter value rounded once to T; the gains
 * c_j are built at _new in double.  Every element of a row is a function of its signal's spectrum, its scale and P alone, so
 * the result's bits do not depend on the batch, the distances, pointer alignment, the workspace, the stream or a graph replay.
 * Workspace: _workspace_len(p, batch) elements of T hold the whole call; any work_len >= _workspace_min(p) (one signal's
 * spectrum and one row) runs chunks of whole rows, to the same bits.
 * _new refuses with PHAST_ERR_INVALID_ARG, before the device is touched: NULL scales; L < 1; P < L or P > 2^29; S < 1 or
 * S > 2^20; a scale that is not finite or is <= 0; an unknown family or norm; a param outside the family's range or not an
 * integer where m is one.  _dev: d_x_im must be NULL for a real planner (real_input != 0 at _new) and non-NULL for a complex
 * one; sig_dist >= L and out_dist >= S L (batch 1 ignores both); pointers need element alignment only; the signal is never
 * written; signal and output must not overlap (identical pointers are refused).  The engine's distance rules are inherited:
 * a real planner with P = L a power of two >= 4 and batch > 1 needs an even sig_dist.  A null pointer, the wrong d_x_im, a
 * short or refused dist, a null or short workspace: PHAST_ERR_INVALID_ARG; a signal_len that is not the planner's:
 * PHAST_ERR_PLANNER_SIZE; an out_len of the host-slice form that is not S L: PHAST_ERR_LEN_MISMATCH -- all before the device
 * is touched.  The *_with_planner forms take host slices of one signal (x_im NULL for a real planner) and block.
 * Out of scope: the inverse transform, real output by C2R for real wavelets of real signals, a fused |W|^2, pruning rows of
 * narrow support, other families, padding other than zeros. */
#define PHAST_CWT_MORLET 0
#define PHAST_CWT_PAUL 1
#define PHAST_CWT_DOG 2
#define PHAST_CWT_STEP 3
#define PHAST_CWT_L2 0
#define PHAST_CWT_PEAK 1
typedef struct phast_planner_cwt64 phast_planner_cwt64; /* PlannerCwt64 */
int phast_planner_cwt64_new(size_t signal_len, size_t pad_len, const double *scales, size_t num_scales, int family, double param, int norm,
                             int real_input, phast_planner_cwt64 **out);
void phast_planner_cwt64_free(phast_planner_cwt64 *p);
int phast_planner_cwt64_describe(const phast_planner_cwt64 *p, char *buf, size_t buf_len);
size_t phast_planner_cwt64_device_bytes(const phast_planner_cwt64 *p);
size_t phast_planner_cwt64_workspace_len(const phast_planner_cwt64 *p, size_t batch);
size_t phast_planner_cwt64_workspace_min(const phast_planner_cwt64 *p);
size_t phast_planner_cwt64_pad_len(const phast_planner_cwt64 *p);     /* P */
size_t phast_planner_cwt64_num_scales(const phast_planner_cwt64 *p);  /* S */
size_t phast_planner_cwt64_tile_bins(const phast_planner_cwt64 *p);   /* bins per workgroup of the bank */
size_t phast_planner_cwt64_scale_group(const phast_planner_cwt64 *p); /* scales per workgroup of the bank at most */
int phast_cwt_64_with_planner(const double *x_re, const double *x_im, size_t x_len, double *out_re, double *out_im, size_t out_len,
                               const phast_planner_cwt64 *planner);
int phast_cwt_64_dev(const double *d_x_re, const double *d_x_im, double *d_out_re, double *d_out_im, size_t signal_len, size_t batch, size_t sig_dist,
                      size_t out_dist, const phast_planner_cwt64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/cwt_rate.py): stage_ms[4] = average milliseconds of the forward transform (with its copy), the bank,
 * the inverse transform and the crop over `reps` calls of `batch` signals at distances L and S L in ONE chunk (work_len >=
 * _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_cwt64_time_stages(const phast_planner_cwt64 *p, const double *d_x_re, const double *d_x_im, double *d_out_re, double *d_out_im, size_t batch, double *d_work, size_t work_len,
                                     int reps, float *stage_ms, void *stream);
typedef struct phast_planner_cwt32 phast_planner_cwt32; /* PlannerCwt32 */
int phast_planner_cwt32_new(size_t signal_len, size_t pad_len, const double *scales, size_t num_scales, int family, double param, int norm,
                             int real_input, phast_planner_cwt32 **out);
void phast_planner_cwt32_free(phast_planner_cwt32 *p);
int phast_planner_cwt32_describe(const phast_planner_cwt32 *p, char *buf, size_t buf_len);
size_t phast_planner_cwt32_device_bytes(const phast_planner_cwt32 *p);
size_t phast_planner_cwt32_workspace_len(const phast_planner_cwt32 *p, size_t batch);
size_t phast_planner_cwt32_workspace_min(const phast_planner_cwt32 *p);
size_t phast_planner_cwt32_pad_len(const phast_planner_cwt32 *p);     /* P */
size_t phast_planner_cwt32_num_scales(const phast_planner_cwt32 *p);  /* S */
size_t phast_planner_cwt32_tile_bins(const phast_planner_cwt32 *p);   /* bins per workgroup of the bank */
size_t phast_planner_cwt32_scale_group(const phast_planner_cwt32 *p); /* scales per workgroup of the bank at most */
int phast_cwt_32_with_planner(const float *x_re, const float *x_im, size_t x_len, float *out_re, float *out_im, size_t out_len,
                               const phast_planner_cwt32 *planner);
int phast_cwt_32_dev(const float *d_x_re, const float *d_x_im, float *d_out_re, float *d_out_im, size_t signal_len, size_t batch, size_t sig_dist,
                      size_t out_dist, const phast_planner_cwt32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/cwt_rate.py): stage_ms[4] = average milliseconds of the forward transform (with its copy), the bank,
 * the inverse transform and the crop over `reps` calls of `batch` signals at distances L and S L in ONE chunk (work_len >=
 * _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_cwt32_time_stages(const phast_planner_cwt32 *p, const float *d_x_re, const float *d_x_im, float *d_out_re, float *d_out_im, size_t batch, float *d_work, size_t work_len,
                                     int reps, float *stage_ms, void *stream);

/* ---- discrete wavelet transform and its inverse (no reference counterpart; pywt.dwt / idwt / wavedec / waverec; DESIGN.md
 * §31).  PyWavelets' definitions; the formulas here are the authority.  Real signals of L samples, 1 <= L <= 2^29, batches.
 * Filter bank: four real filters of one even length F, 2 <= F <= 256 -- dec_lo, dec_hi, rec_lo, rec_hi --, host values of T used
 * as given (pad an odd-length biorthogonal filter with a zero).  Extension ext(x, t) of a signal of n samples, any integer t:
 *     PHAST_DWT_ZERO            0 outside [0, n)
 *     PHAST_DWT_CONSTANT        x[clamp(t, 0, n - 1)]
 *     PHAST_DWT_SYMMETRIC       u = t mod 2n;        x[u] if u < n, else x[2n - 1 - u]
 *     PHAST_DWT_REFLECT         u = t mod (2n - 2);  x[u] if u < n, else x[2n - 2 - u];  n = 1: x[0]
 *     PHAST_DWT_PERIODIC        x[t mod n]
 *     PHAST_DWT_PERIODIZATION   below
 * (the modulus makes F > n legal: the extension wraps more than once).  One analysis level on n samples:
 *     the five extension modes: m = (n + F - 1) div 2,  cA[i] = sum_{j=0}^{F-1} dec_lo[j] ext(x, 2i + 1 - j),  0 <= i < m
 *     periodization:            n' = n + (n mod 2), x[n] := x[n - 1] for odd n, m = n' / 2,
 *                               cA[i] = sum_j dec_lo[j] x[(2i + F/2 - j) mod n']
 * and cD the same with dec_hi.  One synthesis level from m coefficients of each band:
 *     extension modes:          N = 2m - F + 2,  y[r] = sum_k rec_lo[r + F - 2 - 2k] cA[k] + rec_hi[r + F - 2 - 2k] cD[k] over the k
 *                               whose tap index lies in [0, F)
 *     periodization:            N = 2m,  the tap indices are all t in [0, F) with t = (r + F/2 - 1 - 2k) mod N (more than one
 *                               t per k when F > N)
 * Multi-level, `level` = J, 1 <= J <= 32 (J above floor(log2(L / (F - 1))), pywt.dwt_max_level, is legal): n_0 = L, n_l the m
 * of n_{l-1}.  The packed result of one signal is [cA_J | cD_J | cD_{J-1} | ... | cD_1], _coeff_len = n_J + sum_l n_l elements:
 * pywt.wavedec's list, concatenated; _level_len(p, l) = n_l for 0 <= l <= J, _level_offset(p, l) = where cD_l starts for
 * 1 <= l <= J (cA_J starts at 0).  waverec undoes the levels from J down and keeps, at each, the first n_{l-1} of the N
 * reconstructed samples (N is n_{l-1} or n_{l-1} + 1; PyWavelets drops the extra sample, too).
 * Method: one launch per level.  A 256-thread workgroup owns _tile consecutive coefficient indices (analysis) or output pairs
 * (synthesis) of one signal, stages the run of the input it meets through the extension map into LDS (split by parity, so
 * that lanes read consecutive elements; no padded signal exists in memory and a batch neighbour is never read) and feeds every
 * staged value to both bands.  One order per sum, in T: analysis acc = fma(dec[j], ext(x, 2i + 1 - j), acc), j ascending from
 * 0, one chain per band; synthesis tap index descending (k ascending), per tap acc = fma(rec_lo[t], cA[k], acc), then
 * acc = fma(rec_hi[t], cD[k], acc).  The bits depend on the filters, the mode and the values alone: not on the batch, the
 * distances, pointer alignment (element alignment is all that is needed), the workspace's chunks, the stream or a graph replay.
 * Workspace: two ping-pong rows per signal for the approximations between the levels, n_1 + n_2 elements (the longest of the
 * later levels where a signal shorter than the filter grows); _workspace_len(p, batch) holds the batch in one chunk, any
 * work_len >= _workspace_min(p) (one signal's) runs chunks of whole signals.  For J = 1 both are 0 and d_work is not read.
 * _new refuses with PHAST_ERR_INVALID_ARG, before the device is touched: a NULL filter; L < 1 or L > 2^29; F odd, < 2 or > 256;
 * level < 1 or > 32; an unknown mode (PyWavelets' smooth, antisymmetric and antireflect are out of scope).  _dev: asynchronous
 * on `stream`; signal b at d_signal + b sig_dist, its packed row at d_coeffs + b coeff_dist; sig_dist >= L and coeff_dist >=
 * _coeff_len (batch 1 ignores both); the input is never written; signal and coefficients must not overlap (identical pointers
 * are refused).  A null pointer, a short dist, a null or short workspace where one is needed: PHAST_ERR_INVALID_ARG; a
 * signal_len that is not the planner's: PHAST_ERR_PLANNER_SIZE; a coeff_len of the host-slice form that is not _coeff_len:
 * PHAST_ERR_LEN_MISMATCH -- all before any launch.  The *_with_planner forms take host slices of one signal and block.
 * Out of scope, refused rather than approximated: complex signals, a missing band in the inverse, the stationary transform,
 * wavelet packets, 2-D transforms, an axis argument. */
typedef enum {
    PHAST_DWT_ZERO = 0,
    PHAST_DWT_CONSTANT = 1,
    PHAST_DWT_SYMMETRIC = 2,
    PHAST_DWT_REFLECT = 3,
    PHAST_DWT_PERIODIC = 4,
    PHAST_DWT_PERIODIZATION = 5
} phast_dwt_mode;
typedef struct phast_planner_dwt64 phast_planner_dwt64; /* PlannerDwt64 */
int phast_planner_dwt64_new(size_t signal_len, const double *dec_lo, const double *dec_hi, const double *rec_lo, const double *rec_hi, size_t filter_len, size_t level, int mode,
                             phast_planner_dwt64 **out);
void phast_planner_dwt64_free(phast_planner_dwt64 *p);
int phast_planner_dwt64_describe(const phast_planner_dwt64 *p, char *buf, size_t buf_len);
size_t phast_planner_dwt64_device_bytes(const phast_planner_dwt64 *p);
size_t phast_planner_dwt64_workspace_len(const phast_planner_dwt64 *p, size_t batch);
size_t phast_planner_dwt64_workspace_min(const phast_planner_dwt64 *p);
size_t phast_planner_dwt64_coeff_len(const phast_planner_dwt64 *p);                  /* elements of a packed row */
size_t phast_planner_dwt64_level_len(const phast_planner_dwt64 *p, size_t level);    /* n_level, 0 <= level <= J */
size_t phast_planner_dwt64_level_offset(const phast_planner_dwt64 *p, size_t level); /* where cD_level starts in the packed row, 1 <= level <= J */
size_t phast_planner_dwt64_tile(const phast_planner_dwt64 *p);                       /* coefficient indices / output pairs per workgroup */
int phast_wavedec_f64_with_planner(const double *signal, size_t signal_len, double *coeffs, size_t coeff_len, const phast_planner_dwt64 *planner);
int phast_waverec_f64_with_planner(const double *coeffs, size_t coeff_len, double *signal, size_t signal_len, const phast_planner_dwt64 *planner);
int phast_wavedec_f64_dev(const double *d_signal, double *d_coeffs, size_t signal_len, size_t batch, size_t sig_dist, size_t coeff_dist,
                         const phast_planner_dwt64 *planner, double *d_work, size_t work_len, void *stream);
int phast_waverec_f64_dev(const double *d_coeffs, double *d_signal, size_t signal_len, size_t batch, size_t coeff_dist, size_t sig_dist,
                         const phast_planner_dwt64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/dwt_rate.py): stage_ms[2] = average milliseconds of wavedec of the signals into the packed rows and of
 * waverec of the packed rows back into the signals (which it overwrites with their reconstruction) over `reps` calls of `batch`
 * signals at distances L and _coeff_len in ONE chunk (work_len >= _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_dwt64_time_stages(const phast_planner_dwt64 *p, double *d_signal, double *d_coeffs, size_t batch, double *d_work, size_t work_len, int reps, float *stage_ms,
                                     void *stream);
typedef struct phast_planner_dwt32 phast_planner_dwt32; /* PlannerDwt32 */
int phast_planner_dwt32_new(size_t signal_len, const float *dec_lo, const float *dec_hi, const float *rec_lo, const float *rec_hi, size_t filter_len, size_t level, int mode,
                             phast_planner_dwt32 **out);
void phast_planner_dwt32_free(phast_planner_dwt32 *p);
int phast_planner_dwt32_describe(const phast_planner_dwt32 *p, char *buf, size_t buf_len);
size_t phast_planner_dwt32_device_bytes(const phast_planner_dwt32 *p);
size_t phast_planner_dwt32_workspace_len(const phast_planner_dwt32 *p, size_t batch);
size_t phast_planner_dwt32_workspace_min(const phast_planner_dwt32 *p);
size_t phast_planner_dwt32_coeff_len(const phast_planner_dwt32 *p);                  /* elements of a packed row */
size_t phast_planner_dwt32_level_len(const phast_planner_dwt32 *p, size_t level);    /* n_level, 0 <= level <= J */
size_t phast_planner_dwt32_level_offset(const phast_planner_dwt32 *p, size_t level); /* where cD_level starts in the packed row, 1 <= level <= J */
size_t phast_planner_dwt32_tile(const phast_planner_dwt32 *p);                       /* coefficient indices / output pairs per workgroup */
int phast_wavedec_f32_with_planner(const float *signal, size_t signal_len, float *coeffs, size_t coeff_len, const phast_planner_dwt32 *planner);
int phast_waverec_f32_with_planner(const float *coeffs, size_t coeff_len, float *signal, size_t signal_len, const phast_planner_dwt32 *planner);
int phast_wavedec_f32_dev(const float *d_signal, float *d_coeffs, size_t signal_len, size_t batch, size_t sig_dist, size_t coeff_dist,
                         const phast_planner_dwt32 *planner, float *d_work, size_t work_len, void *stream);
int phast_waverec_f32_dev(const float *d_coeffs, float *d_signal, size_t signal_len, size_t batch, size_t coeff_dist, size_t sig_dist,
                         const phast_planner_dwt32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/dwt_rate.py): stage_ms[2] = average milliseconds of wavedec of the signals into the packed rows and of
 * waverec of the packed rows back into the signals (which it overwrites with their reconstruction) over `reps` calls of `batch`
 * signals at distances L and _coeff_len in ONE chunk (work_len >= _workspace_len(p, batch)).  Blocks until done. */
int phast_planner_dwt32_time_stages(const phast_planner_dwt32 *p, float *d_signal, float *d_coeffs, size_t batch, float *d_work, size_t work_len, int reps, float *stage_ms,
                                     void *stream);

/* ---- overlap-save FIR convolution and correlation of real signals (no reference counterpart; scipy.signal.convolve /
 * correlate(x, h, mode, method="direct")).  Signal x of L samples, K taps h, both real:
 *     full[t] = sum_j g[j] x[t - j], t in [0, L + K - 1); g = h (flip = 0: convolution) or g[j] = h[K - 1 - j] (flip = 1:
 *     correlation); out[i] = full[t0 + i], i < out_len, with
 *         PHAST_CONV_FULL   t0 = 0            out_len = L + K - 1
 *         PHAST_CONV_SAME   t0 = (K - 1) / 2  out_len = L
 *         PHAST_CONV_VALID  t0 = K - 1        out_len = L - K + 1   (L >= K)
 * The signal is cut into segments of `block` = B >= K samples that overlap by K - 1; a segment is one R2C of B, a multiply by
 * the filter's spectrum (built once in double by _new) and one C2R of B on the phast_planner_r2c_any* engine, called
 * unchanged, and yields S = B - K + 1 output samples; _segments is ceil(out_len / S).  block = 0 picks B: the smallest power
 * of two >= 4 (K - 1), at least 1024, or the smallest power of two >= L + K - 1 where that is smaller (_block tells).  Any
 * other block needs K <= B <= 2^29; one that is not a power of two runs the Bluestein real path.
 * _new takes 1 <= L, K <= 2^29, out_len <= 2^29, segments x (B rounded up to 16 bytes) <= 2^30, `taps` a host pointer to K
 * values, flip 0 or 1: anything else is PHAST_ERR_INVALID_ARG before the device is touched.
 *
 * The caller's device workspace holds phast_planner_conv*_workspace_len(p, batch) elements of T; any work_len >=
 * _workspace_min(p) (one segment) runs the call in chunks of whole segments, a null or shorter one is PHAST_ERR_INVALID_ARG.
 * _dev calls: asynchronous on `stream`; `batch` signals at sig_dist >= L, their outputs at out_dist >= out_len (any parity),
 * all through the planner's one filter; pointers need element alignment only; the signal is never written and nothing is
 * written past out_len of an output.  A signal_len that is not the planner's is PHAST_ERR_PLANNER_SIZE, a host output that is
 * not out_len long PHAST_ERR_LEN_MISMATCH.  The planner is immutable and holds no per-call state.  An output sample comes from
 * exactly one segment: the bits of a signal do not depend on the batch, the chunking, the stream or graph replay wherever the
 * real transform's do not (every B that is not a power of two, and powers of two up to 4096).  Host-slice calls take one
 * signal, stage through the device and block. */
#define PHAST_CONV_FULL 0
#define PHAST_CONV_SAME 1
#define PHAST_CONV_VALID 2
typedef struct phast_planner_conv64 phast_planner_conv64; /* PlannerConv64 */
int phast_planner_conv64_new(size_t signal_len, const double *taps, size_t num_taps, int mode, int flip, size_t block,
                             phast_planner_conv64 **out);
void phast_planner_conv64_free(phast_planner_conv64 *p);
int phast_planner_conv64_describe(const phast_planner_conv64 *p, char *buf, size_t buf_len);
size_t phast_planner_conv64_device_bytes(const phast_planner_conv64 *p);
size_t phast_planner_conv64_out_len(const phast_planner_conv64 *p);
size_t phast_planner_conv64_block(const phast_planner_conv64 *p);
size_t phast_planner_conv64_segments(const phast_planner_conv64 *p);
size_t phast_planner_conv64_workspace_len(const phast_planner_conv64 *p, size_t batch);
size_t phast_planner_conv64_workspace_min(const phast_planner_conv64 *p);
int phast_conv_f64_with_planner(const double *signal, size_t signal_len, double *output, size_t output_len,
                                const phast_planner_conv64 *planner);
int phast_conv_f64_dev(const double *d_signal, double *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                       const phast_planner_conv64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/conv_rate.py): stage_ms[5] = average milliseconds of the segment sweep, the R2C, the spectrum sweep,
 * the C2R and the save sweep over `reps` calls of `batch` signals at distances L and out_len in ONE chunk (work_len >=
 * phast_planner_conv*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_conv64_time_stages(const phast_planner_conv64 *p, const double *d_signal, double *d_out, size_t batch, double *d_work,
                                     size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_conv32 phast_planner_conv32; /* PlannerConv32 */
int phast_planner_conv32_new(size_t signal_len, const float *taps, size_t num_taps, int mode, int flip, size_t block,
                             phast_planner_conv32 **out);
void phast_planner_conv32_free(phast_planner_conv32 *p);
int phast_planner_conv32_describe(const phast_planner_conv32 *p, char *buf, size_t buf_len);
size_t phast_planner_conv32_device_bytes(const phast_planner_conv32 *p);
size_t phast_planner_conv32_out_len(const phast_planner_conv32 *p);
size_t phast_planner_conv32_block(const phast_planner_conv32 *p);
size_t phast_planner_conv32_segments(const phast_planner_conv32 *p);
size_t phast_planner_conv32_workspace_len(const phast_planner_conv32 *p, size_t batch);
size_t phast_planner_conv32_workspace_min(const phast_planner_conv32 *p);
int phast_conv_f32_with_planner(const float *signal, size_t signal_len, float *output, size_t output_len,
                                const phast_planner_conv32 *planner);
int phast_conv_f32_dev(const float *d_signal, float *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                       const phast_planner_conv32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/conv_rate.py): stage_ms[5] = average milliseconds of the segment sweep, the R2C, the spectrum sweep,
 * the C2R and the save sweep over `reps` calls of `batch` signals at distances L and out_len in ONE chunk (work_len >=
 * phast_planner_conv*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_conv32_time_stages(const phast_planner_conv32 *p, const float *d_signal, float *d_out, size_t batch, float *d_work,
                                     size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- overlap-save convolution and correlation of real ARRAYS of rank 1 .. 3 (no reference counterpart; scipy.signal.convolve /
 * correlate(x, h, mode, method="direct") of N-d arrays).  x is a row-major array [L_0 .. L_{r-1}], h one of the
 * same rank [K_0 .. K_{r-1}], both real:
 *     full[t] = sum_j g[j] x[t - j], t_i in [0, L_i + K_i - 1); g = h (flip = 0) or h reversed along every axis (flip = 1:
 *     correlation); out[i] = full[t0 + i], with t0_i and out_i per axis by the PHAST_CONV_* rules above (VALID needs
 *     L_i >= K_i on every axis; K_i > L_i is legal in FULL and SAME).
 * The array is cut into tiles of block[i] = B_i >= K_i points per axis that overlap by K_i - 1; a tile is one R2C of the tile
 * shape on the phast_planner_r2c_nd* engine, called unchanged, a multiply by the filter's spectrum (built once in double by
 * _new) and one C2R, and yields S_i = B_i - K_i + 1 output samples per axis; _tiles is prod ceil(out_i / S_i).  `block` null,
 * or block[i] = 0, picks B_i: the smallest power of two >= max(4 (K_i - 1), floor), floor = 1024 where one axis counts and 64
 * where two or three do, or the smallest power of two >= out_i + K_i - 1 where that is smaller (_block tells).  An axis with
 * L_i = K_i = 1 does not count: it is dropped (the last one stays if nothing else does) and its block is 1.
 * _new takes rank 1 .. 3, 1 <= L_i, K_i <= 2^29, K_i <= B_i <= 2^29, prod L <= 2^30, prod out <= 2^30, prod B <= 2^28, `taps` a
 * host pointer to prod K values (row-major), flip 0 or 1: anything else is PHAST_ERR_INVALID_ARG before the device is touched.
 * _out_len is prod out; _out_dims and _block fill `rank` values (the planner's rank, or PHAST_ERR_INVALID_ARG).
 *
 * The caller's device workspace holds phast_planner_convnd*_workspace_len(p, batch) elements of T; any work_len >=
 * _workspace_min(p) (one tile) runs the call in chunks of whole tiles, a null or shorter one is PHAST_ERR_INVALID_ARG.
 * _dev calls: asynchronous on `stream`; `batch` arrays at sig_dist >= prod L, their outputs at out_dist >= prod out, all through
 * the planner's one filter; pointers need element alignment only; the arrays are never written and nothing is written outside
 * the prod out elements of an output.  A signal_len that is not prod L is PHAST_ERR_PLANNER_SIZE, a host output that is not
 * prod out long PHAST_ERR_LEN_MISMATCH.  The planner is immutable and holds no per-call state.  An output sample comes from
 * exactly one tile: the bits of an array do not depend on the batch, the chunking, the pointer alignment, the stream or graph
 * replay wherever the tile transform's do not (two or more tile axes longer than 1; or one that is not a power of two, or a
 * power of two up to 4096).  Host-slice calls take one array, stage through the device and block. */
typedef struct phast_planner_convnd64 phast_planner_convnd64; /* PlannerConvNd64 */
int phast_planner_convnd64_new(const size_t *signal_dims, const size_t *tap_dims, size_t rank, const double *taps, int mode, int flip,
                               const size_t *block, phast_planner_convnd64 **out);
void phast_planner_convnd64_free(phast_planner_convnd64 *p);
int phast_planner_convnd64_describe(const phast_planner_convnd64 *p, char *buf, size_t buf_len);
size_t phast_planner_convnd64_device_bytes(const phast_planner_convnd64 *p);
size_t phast_planner_convnd64_out_len(const phast_planner_convnd64 *p);
int phast_planner_convnd64_out_dims(const phast_planner_convnd64 *p, size_t *dims, size_t rank);
int phast_planner_convnd64_block(const phast_planner_convnd64 *p, size_t *dims, size_t rank);
size_t phast_planner_convnd64_tiles(const phast_planner_convnd64 *p);
size_t phast_planner_convnd64_workspace_len(const phast_planner_convnd64 *p, size_t batch);
size_t phast_planner_convnd64_workspace_min(const phast_planner_convnd64 *p);
int phast_convnd_f64_with_planner(const double *signal, size_t signal_len, double *output, size_t output_len,
                                  const phast_planner_convnd64 *planner);
int phast_convnd_f64_dev(const double *d_signal, double *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                         const phast_planner_convnd64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/convnd_rate.py): stage_ms[5] = average milliseconds of the tile sweep, the R2C, the spectrum sweep,
 * the C2R and the save sweep over `reps` calls of `batch` arrays at distances prod L and prod out in ONE chunk (work_len >=
 * phast_planner_convnd*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_convnd64_time_stages(const phast_planner_convnd64 *p, const double *d_signal, double *d_out, size_t batch,
                                       double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_convnd32 phast_planner_convnd32; /* PlannerConvNd32 */
int phast_planner_convnd32_new(const size_t *signal_dims, const size_t *tap_dims, size_t rank, const float *taps, int mode, int flip,
                               const size_t *block, phast_planner_convnd32 **out);
void phast_planner_convnd32_free(phast_planner_convnd32 *p);
int phast_planner_convnd32_describe(const phast_planner_convnd32 *p, char *buf, size_t buf_len);
size_t phast_planner_convnd32_device_bytes(const phast_planner_convnd32 *p);
size_t phast_planner_convnd32_out_len(const phast_planner_convnd32 *p);
int phast_planner_convnd32_out_dims(const phast_planner_convnd32 *p, size_t *dims, size_t rank);
int phast_planner_convnd32_block(const phast_planner_convnd32 *p, size_t *dims, size_t rank);
size_t phast_planner_convnd32_tiles(const phast_planner_convnd32 *p);
size_t phast_planner_convnd32_workspace_len(const phast_planner_convnd32 *p, size_t batch);
size_t phast_planner_convnd32_workspace_min(const phast_planner_convnd32 *p);
int phast_convnd_f32_with_planner(const float *signal, size_t signal_len, float *output, size_t output_len,
                                  const phast_planner_convnd32 *planner);
int phast_convnd_f32_dev(const float *d_signal, float *d_out, size_t signal_len, size_t batch, size_t sig_dist, size_t out_dist,
                         const phast_planner_convnd32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook: as phast_planner_convnd64_time_stages */
int phast_planner_convnd32_time_stages(const phast_planner_convnd32 *p, const float *d_signal, float *d_out, size_t batch,
                                       float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- the chirp-Z transform on the unit circle and the zoom FFT (no reference counterpart; scipy.signal.czt / zoom_fft;
 * DESIGN.md §17).  N input points x, M output points, `start` and `step` finite doubles in turns (cycles per sample):
 *     X[k] = sum_{n < N} x[n] exp(-2 pi i n (start + k step)),  k < M
 * = scipy.signal.czt(x, M, w, a) with w = exp(-2 pi i step), a = exp(2 pi i start), and scipy.signal.zoom_fft(x, [f1, f2], M,
 * fs = fs, endpoint = e) with start = f1 / fs, step = (f2 - f1) / (fs (M - 1 if e else M)); start = 0, step = 1 / N, M = N is
 * the forward DFT.  The parameters are turns, never complex numbers: a complex w has lost the bits that matter at large N.
 * Every angle is formed exactly mod 1 turn in 128-bit fixed point from the two doubles.  Bluestein's schedule in
 * L = _conv_len = the smallest power of two >= N + M - 1 (at least 8): two L-point transforms between three sweeps.
 * _new takes 1 <= N, 1 <= M, N + M - 1 <= 2^30 and finite step and start: anything else is PHAST_ERR_INVALID_ARG before the
 * device is touched.  Points off the unit circle, an inverse and a real-output form are not offered.
 *
 * The caller's device workspace holds phast_planner_czt*_workspace_len(p, batch) = 2 L batch elements of T; any work_len >= 2 L
 * runs the batch in chunks, a null or shorter one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous on `stream`; `batch`
 * inputs at in_dist >= N, their outputs at out_dist >= M; pointers need element alignment only; d_in_im (in_im) may be NULL:
 * a real signal, of which one plane is read.  The input is never written, nothing is written past M of an output, and the
 * output must not overlap the input, the workspace or its other plane (PHAST_ERR_INVALID_ARG).  A host call whose n or m is not the
 * planner's is PHAST_ERR_PLANNER_SIZE.  The planner is immutable and holds no per-call state; the bits of a transform do not
 * depend on the batch, the chunking, the alignment, the stream or graph replay.  Host-slice calls take one signal, stage
 * through the device and block; phast_czt_64 / _32 build a planner for the one call. */
typedef struct phast_planner_czt64 phast_planner_czt64; /* PlannerCzt64 */
int phast_planner_czt64_new(size_t n, size_t m, double step, double start, phast_planner_czt64 **out);
void phast_planner_czt64_free(phast_planner_czt64 *p);
int phast_planner_czt64_describe(const phast_planner_czt64 *p, char *buf, size_t buf_len);
size_t phast_planner_czt64_device_bytes(const phast_planner_czt64 *p);
size_t phast_planner_czt64_conv_len(const phast_planner_czt64 *p);
size_t phast_planner_czt64_workspace_len(const phast_planner_czt64 *p, size_t batch);
int phast_czt_64(const double *in_re, const double *in_im, size_t n, double *out_re, double *out_im, size_t m, double step, double start);
int phast_czt_64_with_planner(const double *in_re, const double *in_im, size_t n, double *out_re, double *out_im, size_t m,
                               const phast_planner_czt64 *planner);
int phast_czt_64_dev(const double *d_in_re, const double *d_in_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist,
                      size_t batch, const phast_planner_czt64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/czt_rate.py): stage_ms[5] = average milliseconds of the pre sweep, the forward L-point transform, the
 * spectrum sweep, the inverse L-point transform and the post sweep over `reps` calls of `batch` transforms at distances N and M in
 * ONE chunk (work_len >= phast_planner_czt*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_czt64_time_stages(const phast_planner_czt64 *p, const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, size_t batch,
                                    double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_czt32 phast_planner_czt32; /* PlannerCzt32 */
int phast_planner_czt32_new(size_t n, size_t m, double step, double start, phast_planner_czt32 **out);
void phast_planner_czt32_free(phast_planner_czt32 *p);
int phast_planner_czt32_describe(const phast_planner_czt32 *p, char *buf, size_t buf_len);
size_t phast_planner_czt32_device_bytes(const phast_planner_czt32 *p);
size_t phast_planner_czt32_conv_len(const phast_planner_czt32 *p);
size_t phast_planner_czt32_workspace_len(const phast_planner_czt32 *p, size_t batch);
int phast_czt_32(const float *in_re, const float *in_im, size_t n, float *out_re, float *out_im, size_t m, double step, double start);
int phast_czt_32_with_planner(const float *in_re, const float *in_im, size_t n, float *out_re, float *out_im, size_t m,
                               const phast_planner_czt32 *planner);
int phast_czt_32_dev(const float *d_in_re, const float *d_in_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist,
                      size_t batch, const phast_planner_czt32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/czt_rate.py): stage_ms[5] = average milliseconds of the pre sweep, the forward L-point transform, the
 * spectrum sweep, the inverse L-point transform and the post sweep over `reps` calls of `batch` transforms at distances N and M in
 * ONE chunk (work_len >= phast_planner_czt*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_czt32_time_stages(const phast_planner_czt32 *p, const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, size_t batch,
                                    float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- non-uniform FFTs of types 1 and 2 in one dimension (no reference counterpart).  The planner holds M points
 * x_j, finite doubles in turns (reduced mod 1; doubles for the f32 planner too), and N modes in numpy fftfreq order: index m holds
 * the frequency k(m) = m for m < ceil(N / 2) and m - N otherwise.
 *     type 1 (points -> modes)   F[m] = sum_j c_j exp(-+2 pi i k(m) x_j)
 *     type 2 (modes -> points)   c_j  = sum_m F[m] exp(-+2 pi i k(m) x_j)
 * with - for PHAST_FORWARD and + for PHAST_REVERSE, no scaling in either: type 2 Reverse is the adjoint of type 1 Forward, and
 * x_j = j / N, M = N makes type 1 Forward the DFT.  `eps` asks for that relative accuracy: the spreading kernel is
 * w = clamp(ceil(log10(1 / eps)) + 1, 2, 16) cells wide on a fine grid of n_g = the smallest power of two >= max(2N, 2w, 8).
 * 1 <= N <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32), every x_j finite: anything else is
 * PHAST_ERR_INVALID_ARG before the device is touched.  `x_turns` is host memory and is sorted by grid cell once, in _new.
 *
 * The caller's device workspace holds phast_planner_nufft*_workspace_len(p, batch) = 2 n_g batch elements of T; any work_len >=
 * 2 n_g runs the batch in chunks, a null or shorter one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous on `stream`; `batch`
 * inputs at in_dist and outputs at out_dist, each at least the row; pointers need element alignment only; the imaginary input
 * plane may be NULL: real data.  The outputs must not overlap the inputs, the workspace or each other, nor the workspace the
 * inputs (PHAST_ERR_INVALID_ARG).  The planner is immutable and holds no per-call state; no floating-point atomics are used: the
 * bits of a transform do not depend on the batch, the chunking, the alignment, the stream or graph replay.  Host-slice calls take
 * one vector, stage through the device and block (a length that is not the planner's is PHAST_ERR_PLANNER_SIZE);
 * phast_nufft1_64 / phast_nufft2_64 / _32 build a planner for the one call.
 *
 * Points in DEVICE memory: _new_dev is _new with `d_x_turns` a device pointer; the points are sorted on the device
 * by a deterministic stable radix sort, into the very tables _new builds on the host, so a transform gives the same bits through
 * either.  _set_points_dev gives an existing planner (built by either) new points, THE SAME M of them (another m_points is
 * PHAST_ERR_PLANNER_SIZE): the tables are rewritten in place, at the same addresses, so a HIP graph captured through the planner
 * stays valid and, replayed, transforms at the new points; nothing else of the planner changes.  Both order themselves after the
 * earlier work of `stream`, allocate their temporary device memory (16 M bytes and a little) inside the call, free it, and BLOCK
 * until the tables are written.  A point that is not finite, a null pointer or a stream that is capturing is
 * PHAST_ERR_INVALID_ARG: _new_dev then builds no planner, and _set_points_dev leaves the planner as it was (the new points are
 * checked and sorted in temporaries first).  _set_points_dev orders itself after the earlier work of `stream` ONLY: as with _free,
 * the caller must have finished the work on other streams that uses the planner, and no other thread may use the planner during
 * the call. */
typedef struct phast_planner_nufft64 phast_planner_nufft64; /* PlannerNufft64 */
int phast_planner_nufft64_new(size_t n_modes, const double *x_turns, size_t m_points, double eps, phast_planner_nufft64 **out);
int phast_planner_nufft64_new_dev(size_t n_modes, const double *d_x_turns, size_t m_points, double eps, void *stream, phast_planner_nufft64 **out);
int phast_planner_nufft64_set_points_dev(phast_planner_nufft64 *p, const double *d_x_turns, size_t m_points, void *stream);
/* measurement hook (tools/nufft_sort_rate.py): one _set_points_dev; stage_ms[0..2] = the milliseconds of its keys, sort and tables stages */
int phast_planner_nufft64_time_set_points(phast_planner_nufft64 *p, const double *d_x_turns, size_t m_points, float *stage_ms, void *stream);
void phast_planner_nufft64_free(phast_planner_nufft64 *p);
int phast_planner_nufft64_describe(const phast_planner_nufft64 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft64_device_bytes(const phast_planner_nufft64 *p);
size_t phast_planner_nufft64_grid_len(const phast_planner_nufft64 *p);
int phast_planner_nufft64_width(const phast_planner_nufft64 *p);
size_t phast_planner_nufft64_workspace_len(const phast_planner_nufft64 *p, size_t batch);
int phast_nufft1_64(const double *x_turns, size_t m_points, const double *c_re, const double *c_im, double *out_re, double *out_im, size_t n_modes, double eps,
                    int direction);
int phast_nufft1_64_with_planner(const double *c_re, const double *c_im, size_t m_points, double *out_re, double *out_im, size_t n_modes, int direction,
                                 const phast_planner_nufft64 *planner);
int phast_nufft1_64_dev(const double *d_c_re, const double *d_c_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                        int direction, const phast_planner_nufft64 *planner, double *d_work, size_t work_len, void *stream);
int phast_nufft2_64(const double *x_turns, size_t m_points, const double *f_re, const double *f_im, double *out_re, double *out_im, size_t n_modes, double eps,
                    int direction);
int phast_nufft2_64_with_planner(const double *f_re, const double *f_im, size_t n_modes, double *out_re, double *out_im, size_t m_points, int direction,
                                 const phast_planner_nufft64 *planner);
int phast_nufft2_64_dev(const double *d_f_re, const double *d_f_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                        int direction, const phast_planner_nufft64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nufft_rate.py): stage_ms[0..2] = average milliseconds of stage a (spread or pre), the n_g-point transform
 * and stage c (deconvolve or interpolate) over `reps` Forward calls of type `type` (1 or 2) of `batch` transforms at the natural
 * distances in ONE chunk (work_len >= phast_planner_nufft*_workspace_len(p, batch)); stage_ms[3] and [4] are 0.  Blocks until done. */
int phast_planner_nufft64_time_stages(const phast_planner_nufft64 *p, const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, int type,
                                      size_t batch, double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_nufft32 phast_planner_nufft32; /* PlannerNufft32 */
int phast_planner_nufft32_new(size_t n_modes, const double *x_turns, size_t m_points, double eps, phast_planner_nufft32 **out);
int phast_planner_nufft32_new_dev(size_t n_modes, const double *d_x_turns, size_t m_points, double eps, void *stream, phast_planner_nufft32 **out);
int phast_planner_nufft32_set_points_dev(phast_planner_nufft32 *p, const double *d_x_turns, size_t m_points, void *stream);
/* measurement hook (tools/nufft_sort_rate.py): one _set_points_dev; stage_ms[0..2] = the milliseconds of its keys, sort and tables stages */
int phast_planner_nufft32_time_set_points(phast_planner_nufft32 *p, const double *d_x_turns, size_t m_points, float *stage_ms, void *stream);
void phast_planner_nufft32_free(phast_planner_nufft32 *p);
int phast_planner_nufft32_describe(const phast_planner_nufft32 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft32_device_bytes(const phast_planner_nufft32 *p);
size_t phast_planner_nufft32_grid_len(const phast_planner_nufft32 *p);
int phast_planner_nufft32_width(const phast_planner_nufft32 *p);
size_t phast_planner_nufft32_workspace_len(const phast_planner_nufft32 *p, size_t batch);
int phast_nufft1_32(const double *x_turns, size_t m_points, const float *c_re, const float *c_im, float *out_re, float *out_im, size_t n_modes, double eps,
                    int direction);
int phast_nufft1_32_with_planner(const float *c_re, const float *c_im, size_t m_points, float *out_re, float *out_im, size_t n_modes, int direction,
                                 const phast_planner_nufft32 *planner);
int phast_nufft1_32_dev(const float *d_c_re, const float *d_c_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                        int direction, const phast_planner_nufft32 *planner, float *d_work, size_t work_len, void *stream);
int phast_nufft2_32(const double *x_turns, size_t m_points, const float *f_re, const float *f_im, float *out_re, float *out_im, size_t n_modes, double eps,
                    int direction);
int phast_nufft2_32_with_planner(const float *f_re, const float *f_im, size_t n_modes, float *out_re, float *out_im, size_t m_points, int direction,
                                 const phast_planner_nufft32 *planner);
int phast_nufft2_32_dev(const float *d_f_re, const float *d_f_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                        int direction, const phast_planner_nufft32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nufft_rate.py): stage_ms[0..2] = average milliseconds of stage a (spread or pre), the n_g-point transform
 * and stage c (deconvolve or interpolate) over `reps` Forward calls of type `type` (1 or 2) of `batch` transforms at the natural
 * distances in ONE chunk (work_len >= phast_planner_nufft*_workspace_len(p, batch)); stage_ms[3] and [4] are 0.  Blocks until done. */
int phast_planner_nufft32_time_stages(const phast_planner_nufft32 *p, const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, int type,
                                      size_t batch, float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- non-uniform FFTs of types 1 and 2 in two dimensions (no reference counterpart).  The planner holds M points
 * (x_j, y_j), finite doubles in turns (reduced mod 1 per coordinate; doubles for the f32 planner too), and N1 x N2 modes, row-major
 * (index m1 N2 + m2), each axis in numpy fftfreq order; k1 pairs with x, k2 with y:
 *     type 1 (points -> modes)   F[m1, m2] = sum_j c_j exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j))
 *     type 2 (modes -> points)   c_j = sum_{m1, m2} F[m1, m2] exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j))
 * with - for PHAST_FORWARD and + for PHAST_REVERSE, no scaling in either: type 2 Reverse is the adjoint of type 1 Forward, and the
 * points (j1 / N1, j2 / N2), M = N1 N2, make type 1 Forward the 2-D DFT.  `eps`, the width w and the per-axis fine grids
 * g_i = the smallest power of two >= max(2 N_i, 2w, 8) are those of the one-dimensional planner; G = g1 g2 (_grid_len; _grid_rows
 * is g1, _grid_cols g2).  N1, N2 >= 1, G <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32), both point
 * arrays non-null and every coordinate finite: anything else is PHAST_ERR_INVALID_ARG before the device is touched.  `x_turns` and
 * `y_turns` are host memory and are sorted by grid cell once, in _new.
 *
 * The caller's device workspace holds phast_planner_nufft2d*_workspace_len(p, batch) = 4 G batch elements of T; any work_len >= 4 G
 * runs the batch in chunks, a null or shorter one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous on `stream`, no allocation,
 * no synchronisation; `batch` inputs at in_dist and outputs at out_dist, each at least the row (M or N1 N2); pointers need element
 * alignment only; the imaginary input plane may be NULL: real data.  The overlap rules, the return codes and the bit-for-bit
 * guarantees are those of the one-dimensional calls.  Host-slice calls take one vector, stage through a device buffer of their own
 * and block (a length that is not the planner's is PHAST_ERR_PLANNER_SIZE); phast_nufft2d1_64 / phast_nufft2d2_64 / _32 build a
 * planner for the one call. */
typedef struct phast_planner_nufft2d64 phast_planner_nufft2d64; /* PlannerNufft2d64 */
int phast_planner_nufft2d64_new(size_t n1, size_t n2, const double *x_turns, const double *y_turns, size_t m_points, double eps, phast_planner_nufft2d64 **out);
/* points in device memory: _new_dev, _set_points_dev and the hook as the one-dimensional planner's (d_x and d_y: M doubles each) */
int phast_planner_nufft2d64_new_dev(size_t n1, size_t n2, const double *d_x_turns, const double *d_y_turns, size_t m_points, double eps, void *stream,
                                    phast_planner_nufft2d64 **out);
int phast_planner_nufft2d64_set_points_dev(phast_planner_nufft2d64 *p, const double *d_x_turns, const double *d_y_turns, size_t m_points, void *stream);
int phast_planner_nufft2d64_time_set_points(phast_planner_nufft2d64 *p, const double *d_x_turns, const double *d_y_turns, size_t m_points, float *stage_ms,
                                            void *stream);
void phast_planner_nufft2d64_free(phast_planner_nufft2d64 *p);
int phast_planner_nufft2d64_describe(const phast_planner_nufft2d64 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft2d64_device_bytes(const phast_planner_nufft2d64 *p);
size_t phast_planner_nufft2d64_grid_len(const phast_planner_nufft2d64 *p);
size_t phast_planner_nufft2d64_grid_rows(const phast_planner_nufft2d64 *p);
size_t phast_planner_nufft2d64_grid_cols(const phast_planner_nufft2d64 *p);
int phast_planner_nufft2d64_width(const phast_planner_nufft2d64 *p);
size_t phast_planner_nufft2d64_workspace_len(const phast_planner_nufft2d64 *p, size_t batch);
int phast_nufft2d1_64(const double *x_turns, const double *y_turns, size_t m_points, const double *c_re, const double *c_im, double *out_re, double *out_im, size_t n1,
                      size_t n2, double eps, int direction);
int phast_nufft2d1_64_with_planner(const double *c_re, const double *c_im, size_t m_points, double *out_re, double *out_im, size_t n_modes, int direction,
                                   const phast_planner_nufft2d64 *planner);
int phast_nufft2d1_64_dev(const double *d_c_re, const double *d_c_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft2d64 *planner, double *d_work, size_t work_len, void *stream);
int phast_nufft2d2_64(const double *x_turns, const double *y_turns, size_t m_points, const double *f_re, const double *f_im, double *out_re, double *out_im, size_t n1,
                      size_t n2, double eps, int direction);
int phast_nufft2d2_64_with_planner(const double *f_re, const double *f_im, size_t n_modes, double *out_re, double *out_im, size_t m_points, int direction,
                                   const phast_planner_nufft2d64 *planner);
int phast_nufft2d2_64_dev(const double *d_f_re, const double *d_f_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft2d64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nufft2d_rate.py): stage_ms[0..2] = average milliseconds of stage a (spread or pre), the 2-D transform of
 * the grid and stage c (deconvolve or interpolate) over `reps` Forward calls of type `type` (1 or 2) of `batch` transforms at the natural
 * distances in ONE chunk (work_len >= phast_planner_nufft2d*_workspace_len(p, batch)); stage_ms[3] and [4] are 0.  Blocks until done. */
int phast_planner_nufft2d64_time_stages(const phast_planner_nufft2d64 *p, const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, int type,
                    size_t batch, double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_nufft2d32 phast_planner_nufft2d32; /* PlannerNufft2d32 */
int phast_planner_nufft2d32_new(size_t n1, size_t n2, const double *x_turns, const double *y_turns, size_t m_points, double eps, phast_planner_nufft2d32 **out);
int phast_planner_nufft2d32_new_dev(size_t n1, size_t n2, const double *d_x_turns, const double *d_y_turns, size_t m_points, double eps, void *stream,
                                    phast_planner_nufft2d32 **out);
int phast_planner_nufft2d32_set_points_dev(phast_planner_nufft2d32 *p, const double *d_x_turns, const double *d_y_turns, size_t m_points, void *stream);
int phast_planner_nufft2d32_time_set_points(phast_planner_nufft2d32 *p, const double *d_x_turns, const double *d_y_turns, size_t m_points, float *stage_ms,
                                            void *stream);
void phast_planner_nufft2d32_free(phast_planner_nufft2d32 *p);
int phast_planner_nufft2d32_describe(const phast_planner_nufft2d32 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft2d32_device_bytes(const phast_planner_nufft2d32 *p);
size_t phast_planner_nufft2d32_grid_len(const phast_planner_nufft2d32 *p);
size_t phast_planner_nufft2d32_grid_rows(const phast_planner_nufft2d32 *p);
size_t phast_planner_nufft2d32_grid_cols(const phast_planner_nufft2d32 *p);
int phast_planner_nufft2d32_width(const phast_planner_nufft2d32 *p);
size_t phast_planner_nufft2d32_workspace_len(const phast_planner_nufft2d32 *p, size_t batch);
int phast_nufft2d1_32(const double *x_turns, const double *y_turns, size_t m_points, const float *c_re, const float *c_im, float *out_re, float *out_im, size_t n1,
                      size_t n2, double eps, int direction);
int phast_nufft2d1_32_with_planner(const float *c_re, const float *c_im, size_t m_points, float *out_re, float *out_im, size_t n_modes, int direction,
                                   const phast_planner_nufft2d32 *planner);
int phast_nufft2d1_32_dev(const float *d_c_re, const float *d_c_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft2d32 *planner, float *d_work, size_t work_len, void *stream);
int phast_nufft2d2_32(const double *x_turns, const double *y_turns, size_t m_points, const float *f_re, const float *f_im, float *out_re, float *out_im, size_t n1,
                      size_t n2, double eps, int direction);
int phast_nufft2d2_32_with_planner(const float *f_re, const float *f_im, size_t n_modes, float *out_re, float *out_im, size_t m_points, int direction,
                                   const phast_planner_nufft2d32 *planner);
int phast_nufft2d2_32_dev(const float *d_f_re, const float *d_f_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft2d32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nufft2d_rate.py): stage_ms[0..2] = average milliseconds of stage a (spread or pre), the 2-D transform of
 * the grid and stage c (deconvolve or interpolate) over `reps` Forward calls of type `type` (1 or 2) of `batch` transforms at the natural
 * distances in ONE chunk (work_len >= phast_planner_nufft2d*_workspace_len(p, batch)); stage_ms[3] and [4] are 0.  Blocks until done. */
int phast_planner_nufft2d32_time_stages(const phast_planner_nufft2d32 *p, const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, int type,
                    size_t batch, float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- non-uniform FFTs of types 1 and 2 in three dimensions (no reference counterpart).  The planner holds M points
 * (x_j, y_j, z_j), finite doubles in turns (reduced mod 1 per coordinate; doubles for the f32 planner too), and N1 x N2 x N3 modes,
 * row-major (index (m1 N2 + m2) N3 + m3), each axis in numpy fftfreq order; k1 pairs with x, k2 with y, k3 with z:
 *     type 1 (points -> modes)   F[m1, m2, m3] = sum_j c_j exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j + k3(m3) z_j))
 *     type 2 (modes -> points)   c_j = sum_m F[m1, m2, m3] exp(-+2 pi i (k1(m1) x_j + k2(m2) y_j + k3(m3) z_j))
 * with - for PHAST_FORWARD and + for PHAST_REVERSE, no scaling in either: type 2 Reverse is the adjoint of type 1 Forward, and the
 * points (j1 / N1, j2 / N2, j3 / N3), M = N1 N2 N3, make type 1 Forward the 3-D DFT.  `eps`, the width w and the per-axis fine grids
 * g_i = the smallest power of two >= max(2 N_i, 2w, 8) are those of the one-dimensional planner; G = g1 g2 g3 (_grid_len;
 * _grid_dim(p, axis) is g1, g2, g3 for axis 0, 1, 2 and 0 for any other).  N_i >= 1, G <= 2^28, 1 <= M <= 2^30, eps in [1e-14, 1e-1]
 * (f64) or [1e-6, 1e-1] (f32), the three point arrays non-null and every coordinate finite: anything else is PHAST_ERR_INVALID_ARG
 * before the device is touched.  The point arrays are host memory and are sorted by grid cell once, in _new.
 *
 * The caller's device workspace holds phast_planner_nufft3d*_workspace_len(p, batch) = 4 G batch elements of T (two grid planes and
 * what the 3-D transform of the grid works in); any work_len >= that of one transform runs the batch in chunks, a null or shorter
 * one is PHAST_ERR_INVALID_ARG.  _dev calls: asynchronous on `stream`, no allocation, no synchronisation; `batch` inputs at in_dist
 * and outputs at out_dist, each at least the row (M or N1 N2 N3); pointers need element alignment only; the imaginary input plane
 * may be NULL: real data.  The overlap rules, the return codes and the bit-for-bit guarantees are those of the one-dimensional
 * calls.  Host-slice calls take one vector, stage through a device buffer of their own and block (a length that is not the
 * planner's is PHAST_ERR_PLANNER_SIZE); phast_nufft3d1_64 / phast_nufft3d2_64 / _32 build a planner for the one call. */
typedef struct phast_planner_nufft3d64 phast_planner_nufft3d64; /* PlannerNufft3d64 */
int phast_planner_nufft3d64_new(size_t n1, size_t n2, size_t n3, const double *x_turns, const double *y_turns, const double *z_turns, size_t m_points, double eps, phast_planner_nufft3d64 **out);
/* points in device memory: _new_dev, _set_points_dev and the hook as the one-dimensional planner's (d_x, d_y and d_z: M doubles each) */
int phast_planner_nufft3d64_new_dev(size_t n1, size_t n2, size_t n3, const double *d_x_turns, const double *d_y_turns, const double *d_z_turns, size_t m_points,
                                    double eps, void *stream, phast_planner_nufft3d64 **out);
int phast_planner_nufft3d64_set_points_dev(phast_planner_nufft3d64 *p, const double *d_x_turns, const double *d_y_turns, const double *d_z_turns, size_t m_points,
                                           void *stream);
int phast_planner_nufft3d64_time_set_points(phast_planner_nufft3d64 *p, const double *d_x_turns, const double *d_y_turns, const double *d_z_turns,
                                            size_t m_points, float *stage_ms, void *stream);
void phast_planner_nufft3d64_free(phast_planner_nufft3d64 *p);
int phast_planner_nufft3d64_describe(const phast_planner_nufft3d64 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft3d64_device_bytes(const phast_planner_nufft3d64 *p);
size_t phast_planner_nufft3d64_grid_len(const phast_planner_nufft3d64 *p);
size_t phast_planner_nufft3d64_grid_dim(const phast_planner_nufft3d64 *p, int axis);
int phast_planner_nufft3d64_width(const phast_planner_nufft3d64 *p);
size_t phast_planner_nufft3d64_workspace_len(const phast_planner_nufft3d64 *p, size_t batch);
int phast_nufft3d1_64(const double *x_turns, const double *y_turns, const double *z_turns, size_t m_points, const double *c_re, const double *c_im, double *out_re, double *out_im, size_t n1,
                      size_t n2, size_t n3, double eps, int direction);
int phast_nufft3d1_64_with_planner(const double *c_re, const double *c_im, size_t m_points, double *out_re, double *out_im, size_t n_modes, int direction,
                                   const phast_planner_nufft3d64 *planner);
int phast_nufft3d1_64_dev(const double *d_c_re, const double *d_c_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft3d64 *planner, double *d_work, size_t work_len, void *stream);
int phast_nufft3d2_64(const double *x_turns, const double *y_turns, const double *z_turns, size_t m_points, const double *f_re, const double *f_im, double *out_re, double *out_im, size_t n1,
                      size_t n2, size_t n3, double eps, int direction);
int phast_nufft3d2_64_with_planner(const double *f_re, const double *f_im, size_t n_modes, double *out_re, double *out_im, size_t m_points, int direction,
                                   const phast_planner_nufft3d64 *planner);
int phast_nufft3d2_64_dev(const double *d_f_re, const double *d_f_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft3d64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nufft3d_rate.py): stage_ms[0..2] = average milliseconds of stage a (spread or pre), the 3-D transform of
 * the grid and stage c (deconvolve or interpolate) over `reps` Forward calls of type `type` (1 or 2) of `batch` transforms at the natural
 * distances in ONE chunk (work_len >= phast_planner_nufft3d*_workspace_len(p, batch)); stage_ms[3] and [4] are 0.  Blocks until done. */
int phast_planner_nufft3d64_time_stages(const phast_planner_nufft3d64 *p, const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, int type,
                    size_t batch, double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_nufft3d32 phast_planner_nufft3d32; /* PlannerNufft3d32 */
int phast_planner_nufft3d32_new(size_t n1, size_t n2, size_t n3, const double *x_turns, const double *y_turns, const double *z_turns, size_t m_points, double eps, phast_planner_nufft3d32 **out);
int phast_planner_nufft3d32_new_dev(size_t n1, size_t n2, size_t n3, const double *d_x_turns, const double *d_y_turns, const double *d_z_turns, size_t m_points,
                                    double eps, void *stream, phast_planner_nufft3d32 **out);
int phast_planner_nufft3d32_set_points_dev(phast_planner_nufft3d32 *p, const double *d_x_turns, const double *d_y_turns, const double *d_z_turns, size_t m_points,
                                           void *stream);
int phast_planner_nufft3d32_time_set_points(phast_planner_nufft3d32 *p, const double *d_x_turns, const double *d_y_turns, const double *d_z_turns,
                                            size_t m_points, float *stage_ms, void *stream);
void phast_planner_nufft3d32_free(phast_planner_nufft3d32 *p);
int phast_planner_nufft3d32_describe(const phast_planner_nufft3d32 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft3d32_device_bytes(const phast_planner_nufft3d32 *p);
size_t phast_planner_nufft3d32_grid_len(const phast_planner_nufft3d32 *p);
size_t phast_planner_nufft3d32_grid_dim(const phast_planner_nufft3d32 *p, int axis);
int phast_planner_nufft3d32_width(const phast_planner_nufft3d32 *p);
size_t phast_planner_nufft3d32_workspace_len(const phast_planner_nufft3d32 *p, size_t batch);
int phast_nufft3d1_32(const double *x_turns, const double *y_turns, const double *z_turns, size_t m_points, const float *c_re, const float *c_im, float *out_re, float *out_im, size_t n1,
                      size_t n2, size_t n3, double eps, int direction);
int phast_nufft3d1_32_with_planner(const float *c_re, const float *c_im, size_t m_points, float *out_re, float *out_im, size_t n_modes, int direction,
                                   const phast_planner_nufft3d32 *planner);
int phast_nufft3d1_32_dev(const float *d_c_re, const float *d_c_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft3d32 *planner, float *d_work, size_t work_len, void *stream);
int phast_nufft3d2_32(const double *x_turns, const double *y_turns, const double *z_turns, size_t m_points, const float *f_re, const float *f_im, float *out_re, float *out_im, size_t n1,
                      size_t n2, size_t n3, double eps, int direction);
int phast_nufft3d2_32_with_planner(const float *f_re, const float *f_im, size_t n_modes, float *out_re, float *out_im, size_t m_points, int direction,
                                   const phast_planner_nufft3d32 *planner);
int phast_nufft3d2_32_dev(const float *d_f_re, const float *d_f_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                          int direction, const phast_planner_nufft3d32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nufft3d_rate.py): stage_ms[0..2] = average milliseconds of stage a (spread or pre), the 3-D transform of
 * the grid and stage c (deconvolve or interpolate) over `reps` Forward calls of type `type` (1 or 2) of `batch` transforms at the natural
 * distances in ONE chunk (work_len >= phast_planner_nufft3d*_workspace_len(p, batch)); stage_ms[3] and [4] are 0.  Blocks until done. */
int phast_planner_nufft3d32_time_stages(const phast_planner_nufft3d32 *p, const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, int type,
                    size_t batch, float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- the non-uniform FFT of type 3 in one dimension (no reference counterpart; FINUFFT's type 3) ----
 * M sources x_j (host doubles, any finite values, in a unit U) and K target frequencies s_k (host doubles, any finite values,
 * in 1 / U); the product s_k x_j is in TURNS:
 *
 *     f[k] = sum_j c[j] exp(-+2 pi i s[k] x[j]),   j < M, k < K       (- PHAST_FORWARD, + PHAST_REVERSE; no scaling)
 *
 * to the relative accuracy eps in [1e-14, 1e-1] (f64) or [1e-6, 1e-1] (f32).  1 <= M <= 2^30, 1 <= K <= 2^30, and the fine grid
 * n_f = the smallest power of two >= max(8 S X + w, 2 w, 8) -- X and S the half-widths of the two point sets about their centres,
 * w the kernel width of eps -- is at most 2^28 (phast_planner_nufft_t3_*_grid_len); anything else is PHAST_ERR_INVALID_ARG before
 * the device is touched.  Both point sets are fixed at _new.  The error grows with the conditioning of the problem,
 * 2 pi (|C_s| + S) X 2^-53, and with nothing else that depends on the centres C_x, C_s.
 *
 * Data are planar (re, im); a null imaginary INPUT plane means real data.  _dev: `batch` transforms share the planner, transform b
 * at b * in_dist (>= M) and b * out_dist (>= K); asynchronous on `stream`.  The caller's device workspace holds
 * phast_planner_nufft_t3_*_workspace_len(p, batch) = 4 n_f batch elements of T; any work_len >= _workspace_len(p, 1) runs the
 * batch in chunks.  The output may not overlap the input or the workspace, nor the workspace the input.  The host-slice forms
 * block (a length that is not the planner's is PHAST_ERR_PLANNER_SIZE); phast_nufft3_64 / _32 build a planner for the one call. */
typedef struct phast_planner_nufft_t3_64 phast_planner_nufft_t3_64; /* PlannerNufftT3_64 */
int phast_planner_nufft_t3_64_new(const double *x, size_t m_points, const double *s, size_t k_targets, double eps, phast_planner_nufft_t3_64 **out);
void phast_planner_nufft_t3_64_free(phast_planner_nufft_t3_64 *p);
int phast_planner_nufft_t3_64_describe(const phast_planner_nufft_t3_64 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft_t3_64_device_bytes(const phast_planner_nufft_t3_64 *p);
size_t phast_planner_nufft_t3_64_grid_len(const phast_planner_nufft_t3_64 *p);
int phast_planner_nufft_t3_64_width(const phast_planner_nufft_t3_64 *p);
size_t phast_planner_nufft_t3_64_workspace_len(const phast_planner_nufft_t3_64 *p, size_t batch);
int phast_nufft3_64(const double *x, size_t m_points, const double *s, size_t k_targets, const double *c_re, const double *c_im, double *out_re, double *out_im, double eps,
                    int direction);
int phast_nufft3_64_with_planner(const double *c_re, const double *c_im, size_t m_points, double *out_re, double *out_im, size_t k_targets, int direction,
                                 const phast_planner_nufft_t3_64 *planner);
int phast_nufft3_64_dev(const double *d_c_re, const double *d_c_im, size_t in_dist, double *d_out_re, double *d_out_im, size_t out_dist, size_t batch,
                        int direction, const phast_planner_nufft_t3_64 *planner, double *d_work, size_t work_len, void *stream);
/* measurement hook: stage_ms[0..3] = average HIP-event milliseconds of (spread, the n_g-point transform, interpolate, post) over `reps` Forward calls at the
 * natural distances in ONE chunk (work_len >= phast_planner_nufft_t3_*_workspace_len(p, batch)); stage_ms[4] is 0.  Blocks until done. */
int phast_planner_nufft_t3_64_time_stages(const phast_planner_nufft_t3_64 *p, const double *d_in_re, const double *d_in_im, double *d_out_re, double *d_out_im, size_t batch,
                    double *d_work, size_t work_len, int reps, float *stage_ms, void *stream);
typedef struct phast_planner_nufft_t3_32 phast_planner_nufft_t3_32; /* PlannerNufftT3_32 */
int phast_planner_nufft_t3_32_new(const double *x, size_t m_points, const double *s, size_t k_targets, double eps, phast_planner_nufft_t3_32 **out);
void phast_planner_nufft_t3_32_free(phast_planner_nufft_t3_32 *p);
int phast_planner_nufft_t3_32_describe(const phast_planner_nufft_t3_32 *p, char *buf, size_t buf_len);
size_t phast_planner_nufft_t3_32_device_bytes(const phast_planner_nufft_t3_32 *p);
size_t phast_planner_nufft_t3_32_grid_len(const phast_planner_nufft_t3_32 *p);
int phast_planner_nufft_t3_32_width(const phast_planner_nufft_t3_32 *p);
size_t phast_planner_nufft_t3_32_workspace_len(const phast_planner_nufft_t3_32 *p, size_t batch);
int phast_nufft3_32(const double *x, size_t m_points, const double *s, size_t k_targets, const float *c_re, const float *c_im, float *out_re, float *out_im, double eps,
                    int direction);
int phast_nufft3_32_with_planner(const float *c_re, const float *c_im, size_t m_points, float *out_re, float *out_im, size_t k_targets, int direction,
                                 const phast_planner_nufft_t3_32 *planner);
int phast_nufft3_32_dev(const float *d_c_re, const float *d_c_im, size_t in_dist, float *d_out_re, float *d_out_im, size_t out_dist, size_t batch,
                        int direction, const phast_planner_nufft_t3_32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook: stage_ms[0..3] = average HIP-event milliseconds of (spread, the n_g-point transform, interpolate, post) over `reps` Forward calls at the
 * natural distances in ONE chunk (work_len >= phast_planner_nufft_t3_*_workspace_len(p, batch)); stage_ms[4] is 0.  Blocks until done. */
int phast_planner_nufft_t3_32_time_stages(const phast_planner_nufft_t3_32 *p, const float *d_in_re, const float *d_in_im, float *d_out_re, float *d_out_im, size_t batch,
                    float *d_work, size_t work_len, int reps, float *stage_ms, void *stream);

/* ---- multi-dimensional transforms over every axis of a row-major array (no reference counterpart; numpy fftn / ifftn /
 * rfftn / irfftn with this library's conventions).  dims[0 .. rank-1]: rank 1 .. 8, every axis 1 .. 2^29,
 * their product <= 2^30 (else PHAST_ERR_INVALID_ARG, before the device is touched).  Every axis is transformed; leading
 * batch axes are `batch` / `dist` of the _dev calls.  Each axis runs the any-length path of its length (phast_planner_any*:
 * a power of two on the engine, else Bluestein), rotated to the contiguous end by a batched planar transpose: r transposes
 * for rank r.  Axes of length 1 are dropped at _new (the real last axis stays); a shape with one axis left runs the one-axis
 * call itself (phast_fft_*_any_dev / phast_r2c_fft_*_any_dev ...): same bits, same batch rules.
 *
 * Complex: two planes of prod n_i points, in place for the caller; forward unnormalised, the inverse scales by 1 / prod n_i.
 * R2C: the real array [n_0 .. n_{r-1}] -> two planes [n_0 .. n_{r-2}][n_{r-1} / 2 + 1] (floor); C2R the inverse, scaled by
 * 1 / prod n_i: the leading axes first, the last axis by the any-length C2R (its rules for a non-Hermitian input and for
 * Im X[0] carry over).  R2C never writes its input, C2R never its input planes.  The length codes of the one-axis calls
 * apply with these counts (a wrong count of a complex host call: PHAST_ERR_PLANNER_SIZE; n_total of a _dev call that is not
 * the planner's prod n_i: PHAST_ERR_PLANNER_SIZE).
 *
 * _dev calls: asynchronous on `stream`; arrays `dist` (complex), `in_dist` / `out_dist` (real: the real side >= prod n_i,
 * the complex side >= the half-spectrum points) elements apart; element alignment suffices.  Workspace (elements of T):
 * *_workspace_len(p, batch) runs the batch at full speed (the transposed copies of the batch -- two for the real planner,
 * whose C2R ping-pongs between them -- plus the largest Bluestein workspace a step needs); *_workspace_len(p, 1) serves
 * any batch, in chunks.  The smallest legal work_len is the copies of one array plus 2 M of the largest Bluestein axis
 * (M: its convolution length); below it (or null) is PHAST_ERR_INVALID_ARG.  The real planner's lengths count C2R's two
 * copies; R2C uses one and needs 2 x the half-spectrum points per array less.  For a
 * shape with one axis left the workspace is that axis planner's.  Planners are immutable after _new and hold no per-call
 * state: graph capture and concurrent streams need one workspace per call in flight.  With two or more axes left, each
 * axis runs one engine plan fixed at _new, so the bits of a transform do not depend on the batch, the chunking, the
 * stream, graph replay or the form of the call.  Host-slice calls stage through the device (they block); the calls
 * without a planner build one per call. */
typedef struct phast_planner_nd64 phast_planner_nd64;         /* PlannerNd64 */
typedef struct phast_planner_nd32 phast_planner_nd32;         /* PlannerNd32 */
typedef struct phast_planner_r2c_nd64 phast_planner_r2c_nd64; /* PlannerR2cNd64 */
typedef struct phast_planner_r2c_nd32 phast_planner_r2c_nd32; /* PlannerR2cNd32 */
int phast_planner_nd64_new(const size_t *dims, size_t rank, phast_planner_nd64 **out);
int phast_planner_nd32_new(const size_t *dims, size_t rank, phast_planner_nd32 **out);
void phast_planner_nd64_free(phast_planner_nd64 *p);
void phast_planner_nd32_free(phast_planner_nd32 *p);
int phast_planner_nd64_describe(const phast_planner_nd64 *p, char *buf, size_t buf_len);
int phast_planner_nd32_describe(const phast_planner_nd32 *p, char *buf, size_t buf_len);
size_t phast_planner_nd64_device_bytes(const phast_planner_nd64 *p);
size_t phast_planner_nd32_device_bytes(const phast_planner_nd32 *p);
size_t phast_planner_nd64_workspace_len(const phast_planner_nd64 *p, size_t batch);
size_t phast_planner_nd32_workspace_len(const phast_planner_nd32 *p, size_t batch);
int phast_fft_64_nd(double *reals, size_t reals_len, double *imags, size_t imags_len, const size_t *dims, size_t rank,
                    int direction);
int phast_fft_32_nd(float *reals, size_t reals_len, float *imags, size_t imags_len, const size_t *dims, size_t rank,
                    int direction);
int phast_fft_64_nd_with_planner(double *reals, size_t reals_len, double *imags, size_t imags_len, int direction,
                                 const phast_planner_nd64 *planner);
int phast_fft_32_nd_with_planner(float *reals, size_t reals_len, float *imags, size_t imags_len, int direction,
                                 const phast_planner_nd32 *planner);
int phast_fft_64_nd_dev(double *d_reals, double *d_imags, size_t n_total, size_t batch, size_t dist, int direction,
                        const phast_planner_nd64 *planner, double *d_work, size_t work_len, void *stream);
int phast_fft_32_nd_dev(float *d_reals, float *d_imags, size_t n_total, size_t batch, size_t dist, int direction,
                        const phast_planner_nd32 *planner, float *d_work, size_t work_len, void *stream);
/* measurement hook (tools/nd_rate.py): step_ms[i] = average milliseconds of step i of the schedule (describe() lists them;
 * at most 17), *n_steps = their count, over `reps` forward calls of the batch in ONE chunk (two or more axes left,
 * work_len >= phast_planner_nd*_workspace_len(p, batch)).  Blocks until done. */
int phast_planner_nd64_time_steps(const phast_planner_nd64 *p, double *d_reals, double *d_imags, size_t batch, size_t dist,
                                  double *d_work, size_t work_len, int reps, float *step_ms, size_t *n_steps, void *stream);
int phast_planner_nd32_time_steps(const phast_planner_nd32 *p, float *d_reals, float *d_imags, size_t batch, size_t dist,
                                  float *d_work, size_t work_len, int reps, float *step_ms, size_t *n_steps, void *stream);
int phast_planner_r2c_nd64_new(const size_t *dims, size_t rank, phast_planner_r2c_nd64 **out);
int phast_planner_r2c_nd32_new(const size_t *dims, size_t rank, phast_planner_r2c_nd32 **out);
void phast_planner_r2c_nd64_free(phast_planner_r2c_nd64 *p);
void phast_planner_r2c_nd32_free(phast_planner_r2c_nd32 *p);
int phast_planner_r2c_nd64_describe(const phast_planner_r2c_nd64 *p, char *buf, size_t buf_len);
int phast_planner_r2c_nd32_describe(const phast_planner_r2c_nd32 *p, char *buf, size_t buf_len);
size_t phast_planner_r2c_nd64_device_bytes(const phast_planner_r2c_nd64 *p);
size_t phast_planner_r2c_nd32_device_bytes(const phast_planner_r2c_nd32 *p);
size_t phast_planner_r2c_nd64_workspace_len(const phast_planner_r2c_nd64 *p, size_t batch);
size_t phast_planner_r2c_nd32_workspace_len(const phast_planner_r2c_nd32 *p, size_t batch);
int phast_r2c_fft_f64_nd(const double *input, size_t input_len, double *output_re, size_t output_re_len, double *output_im,
                         size_t output_im_len, const size_t *dims, size_t rank);
int phast_r2c_fft_f32_nd(const float *input, size_t input_len, float *output_re, size_t output_re_len, float *output_im,
                         size_t output_im_len, const size_t *dims, size_t rank);
int phast_r2c_fft_f64_nd_with_planner(const double *input, size_t input_len, double *output_re, size_t output_re_len,
                                      double *output_im, size_t output_im_len, const phast_planner_r2c_nd64 *planner);
int phast_r2c_fft_f32_nd_with_planner(const float *input, size_t input_len, float *output_re, size_t output_re_len,
                                      float *output_im, size_t output_im_len, const phast_planner_r2c_nd32 *planner);
int phast_r2c_fft_f64_nd_dev(const double *d_input, double *d_output_re, double *d_output_im, size_t n_total, size_t batch,
                             size_t in_dist, size_t out_dist, const phast_planner_r2c_nd64 *planner, double *d_work,
                             size_t work_len, void *stream);
int phast_r2c_fft_f32_nd_dev(const float *d_input, float *d_output_re, float *d_output_im, size_t n_total, size_t batch,
                             size_t in_dist, size_t out_dist, const phast_planner_r2c_nd32 *planner, float *d_work,
                             size_t work_len, void *stream);
int phast_c2r_fft_f64_nd(const double *input_re, size_t input_re_len, const double *input_im, size_t input_im_len,
                         double *output, size_t output_len, const size_t *dims, size_t rank);
int phast_c2r_fft_f32_nd(const float *input_re, size_t input_re_len, const float *input_im, size_t input_im_len,
                         float *output, size_t output_len, const size_t *dims, size_t rank);
int phast_c2r_fft_f64_nd_with_planner(const double *input_re, size_t input_re_len, const double *input_im,
                                      size_t input_im_len, double *output, size_t output_len,
                                      const phast_planner_r2c_nd64 *planner);
int phast_c2r_fft_f32_nd_with_planner(const float *input_re, size_t input_re_len, const float *input_im,
                                      size_t input_im_len, float *output, size_t output_len,
                                      const phast_planner_r2c_nd32 *planner);
int phast_c2r_fft_f64_nd_dev(const double *d_input_re, const double *d_input_im, double *d_output, size_t n_total,
                             size_t batch, size_t in_dist, size_t out_dist, const phast_planner_r2c_nd64 *planner,
                             double *d_work, size_t work_len, void *stream);
int phast_c2r_fft_f32_nd_dev(const float *d_input_re, const float *d_input_im, float *d_output, size_t n_total,
                             size_t batch, size_t in_dist, size_t out_dist, const phast_planner_r2c_nd32 *planner,
                             float *d_work, size_t work_len, void *stream);

/* ---- bit reversal: algorithms/bravo.rs:303,317 (public with feature bench-internals, lib.rs:20-23) ---- */
int phast_bit_rev_f64(double *data, size_t len, unsigned log_n); /* host slice */
int phast_bit_rev_f32(float *data, size_t len, unsigned log_n);
int phast_bit_rev_f64_dev(double *d_data, unsigned log_n, size_t batch, size_t dist, void *stream);
int phast_bit_rev_f32_dev(float *d_data, unsigned log_n, size_t batch, size_t dist, void *stream);

/* ---- Complex<T> <-> planes: complex_nums.rs (public with feature bench-internals, like the bit reversal) ----
 * deinterleave: [1, 2, 3, 4] -> ([1, 3], [2, 4]) for any length; `chunks_exact(2)` drops an odd last element
 * (complex_nums.rs:11-17).  deinterleave_complex64 / _complex32 (:25-39) are this on the cast slice: pass the n Complex<T>
 * as 2 n scalars.  combine_re_im (:47-56): `assert_eq!(reals.len(), imags.len())` -> PHAST_ERR_LEN_MISMATCH.  The reference
 * returns new Vecs; a C caller brings the outputs, and the host-slice forms check their lengths (len / 2 each; 2 n). */
int phast_deinterleave_f64(const double *input, size_t len, double *out_a, size_t a_len, double *out_b, size_t b_len);
int phast_deinterleave_f32(const float *input, size_t len, float *out_a, size_t a_len, float *out_b, size_t b_len);
int phast_deinterleave_f64_dev(const double *d_input, size_t len, double *d_out_a, double *d_out_b, void *stream);
int phast_deinterleave_f32_dev(const float *d_input, size_t len, float *d_out_a, float *d_out_b, void *stream);
int phast_combine_re_im_f64(const double *reals, size_t reals_len, const double *imags, size_t imags_len, double *out, size_t out_len);
int phast_combine_re_im_f32(const float *reals, size_t reals_len, const float *imags, size_t imags_len, float *out, size_t out_len);
int phast_combine_re_im_f64_dev(const double *d_reals, const double *d_imags, size_t n, double *d_out, void *stream);
int phast_combine_re_im_f32_dev(const float *d_reals, const float *d_imags, size_t n, float *d_out, void *stream);

/* ---- R2C: algorithms/r2c.rs:521-662 ---- */
int phast_r2c_fft_f64(const double *input_re, size_t input_len, double *output_re, size_t output_re_len,
                      double *output_im, size_t output_im_len); /* r2c.rs:521 */
int phast_r2c_fft_f32(const float *input_re, size_t input_len, float *output_re, size_t output_re_len,
                      float *output_im, size_t output_im_len); /* r2c.rs:598 */
int phast_r2c_fft_f64_with_planner(const double *input_re, size_t input_len, double *output_re,
                                   size_t output_re_len, double *output_im, size_t output_im_len,
                                   const phast_planner_r2c64 *planner); /* r2c.rs:535 */
int phast_r2c_fft_f32_with_planner(const float *input_re, size_t input_len, float *output_re, size_t output_re_len,
                                   float *output_im, size_t output_im_len,
                                   const phast_planner_r2c32 *planner); /* r2c.rs:607 */
/* device-resident: input N reals, outputs N/2+1 each; batch b at +b*in_dist / +b*out_dist elements */
int phast_r2c_fft_f64_dev(const double *d_input, double *d_output_re, double *d_output_im, size_t batch,
                          size_t in_dist, size_t out_dist, const phast_planner_r2c64 *planner, void *stream);
int phast_r2c_fft_f32_dev(const float *d_input, float *d_output_re, float *d_output_im, size_t batch,
                          size_t in_dist, size_t out_dist, const phast_planner_r2c32 *planner, void *stream);

/* ---- C2R: algorithms/r2c.rs:695-895 ---- */
int phast_c2r_fft_f64(const double *input_re, size_t input_re_len, const double *input_im, size_t input_im_len,
                      double *output, size_t output_len); /* r2c.rs:695 */
int phast_c2r_fft_f32(const float *input_re, size_t input_re_len, const float *input_im, size_t input_im_len,
                      float *output, size_t output_len); /* r2c.rs:804 */
int phast_c2r_fft_f64_with_planner(const double *input_re, size_t input_re_len, const double *input_im,
                                   size_t input_im_len, double *output, size_t output_len,
                                   const phast_planner_r2c64 *planner); /* r2c.rs:710 */
int phast_c2r_fft_f32_with_planner(const float *input_re, size_t input_re_len, const float *input_im,
                                   size_t input_im_len, float *output, size_t output_len,
                                   const phast_planner_r2c32 *planner); /* r2c.rs:813 */
/* the scratch slices are validated for length exactly as the reference does and otherwise unused:
 * the device path keeps its workspace in the planner (r2c.rs:740,836) */
int phast_c2r_fft_f64_with_planner_and_scratch(const double *input_re, size_t input_re_len, const double *input_im,
                                               size_t input_im_len, double *output, size_t output_len,
                                               const phast_planner_r2c64 *planner, double *scratch_re,
                                               size_t scratch_re_len, double *scratch_im, size_t scratch_im_len);
int phast_c2r_fft_f32_with_planner_and_scratch(const float *input_re, size_t input_re_len, const float *input_im,
                                               size_t input_im_len, float *output, size_t output_len,
                                               const phast_planner_r2c32 *planner, float *scratch_re,
                                               size_t scratch_re_len, float *scratch_im, size_t scratch_im_len);
int phast_c2r_fft_f64_dev(const double *d_input_re, const double *d_input_im, double *d_output, size_t batch,
                          size_t in_dist, size_t out_dist, const phast_planner_r2c64 *planner, void *stream);
int phast_c2r_fft_f32_dev(const float *d_input_re, const float *d_input_im, float *d_output, size_t batch,
                          size_t in_dist, size_t out_dist, const phast_planner_r2c32 *planner, void *stream);

/* ---- harness support: deterministic on-device inputs and digests ---- */
/* value(i) = uniform [-1,1) from splitmix64(seed ^ (transform_id << 40) ^ (2*i + is_imag)); transform b of the
 * batch uses transform_id = first_id + b.  Same generator as oracle/pho_fill_*. */
int phast_fill_f64_dev(double *d_reals, double *d_imags, size_t n, size_t batch, size_t dist,
                       unsigned long long seed, unsigned long long first_id, void *stream);
int phast_fill_f32_dev(float *d_reals, float *d_imags, size_t n, size_t batch, size_t dist,
                       unsigned long long seed, unsigned long long first_id, void *stream);
/* per-transform digest {sum re, sum im, sum re^2+im^2, re[probe]} in f64, 4 doubles per transform */
int phast_digest_f64_dev(const double *d_reals, const double *d_imags, size_t n, size_t batch, size_t dist,
                         size_t probe, double *d_digest, void *stream);
int phast_digest_f32_dev(const float *d_reals, const float *d_imags, size_t n, size_t batch, size_t dist,
                         size_t probe, double *d_digest, void *stream);

/* harness: the streaming ceilings of the current device, measured with hand-written grid-stride kernels (probe.hip):
 * d_a (read) and d_b (written) are device buffers of `bytes` each (a multiple of 16, >= 1 MiB; use >= 1 GiB so that
 * the 256 MiB Infinity Cache does not help); out_gbps[3] = {read-only, write-only, 1:1 copy with read + write counted}
 * in GB/s, each the best of several access widths / grid sizes over `reps` back-to-back launches.  Blocks until done.
 * bench.py reports them as roofline.stream_probe: the copy figure is what a pass that reads and writes every byte once
 * can reach on this box. */
int phast_stream_probe_dev(const void *d_a, void *d_b, size_t bytes, int reps, double *out_gbps, void *stream);

/* The _dev entry points are stream-capture safe (no allocation, no synchronisation in the steady state), so a
 * launch-bound sequence of transforms is captured into a HIP graph with the plain HIP API around them.  This helper is
 * hipGraphUpload for hosts that hold a hipGraphExec_t but cannot call HIP themselves (bench.py: the exec handle of a
 * torch CUDAGraph): the first launch of an instantiated graph otherwise pays the upload inside the timed region. */
int phast_hip_graph_upload(void *graph_exec, void *stream);

/* ---- one transform spread over several GPUs (no reference counterpart: the reference's
 * recursion, algorithms/dit.rs:33-164, never leaves one address space).  A four-step split N = N1*N2 needs, between
 * its two local FFT stages, every element (r, c) of a rank's row-major slab multiplied by W_N^((row0 + r)*(col0 + c));
 * a twiddle grid owns the device tables of W_N (three-level, as the planners').  The exchanges themselves are the
 * host side's (phastft_amd/distributed.py: RCCL all-to-all through torch.distributed). ---- */
typedef struct phast_twiddle_grid64 phast_twiddle_grid64;
typedef struct phast_twiddle_grid32 phast_twiddle_grid32;
int phast_twiddle_grid64_new(size_t n, phast_twiddle_grid64 **out);   /* n = N, a power of two <= 2^32 */
int phast_twiddle_grid32_new(size_t n, phast_twiddle_grid32 **out);
void phast_twiddle_grid64_free(phast_twiddle_grid64 *g);
void phast_twiddle_grid32_free(phast_twiddle_grid32 *g);
int phast_twiddle_grid64_apply_dev(const phast_twiddle_grid64 *g, double *d_re, double *d_im, size_t rows, size_t cols,
                                   size_t row_pitch, size_t row0, size_t col0, void *stream);
int phast_twiddle_grid32_apply_dev(const phast_twiddle_grid32 *g, float *d_re, float *d_im, size_t rows, size_t cols,
                                   size_t row_pitch, size_t row0, size_t col0, void *stream);

/* ---- tuning hook used by tools/ and tests to force a pass plan (n_passes = 0 restores the heuristic) ----
 * log_rows[i] = log2 of pass i's tile FFT length, tile_logs[i] = log2 of the points per tile of pass i
 * (12, 13 or 14), points_log = log2 of the complex points each thread holds (4, or 3 for the 4096-point
 * latency tiles).  The forced plan serves every batch size.  Returns PHAST_ERR_INVALID_ARG when the
 * factorisation is not realisable with the compiled tile shapes. */
int phast_planner_dit64_set_plan(phast_planner_dit64 *p, const unsigned *log_rows, const unsigned *tile_logs,
                                 size_t n_passes, unsigned points_log);
int phast_planner_dit32_set_plan(phast_planner_dit32 *p, const unsigned *log_rows, const unsigned *tile_logs,
                                 size_t n_passes, unsigned points_log);

/* tuning hook: force the number of resident workgroups per CU the tile passes are launched with (0 = planner's own
 * residency estimate).  Process-wide; for sweeps in tools/ only. */
void phast_debug_set_wg_per_cu(int wg_per_cu);
/* debug hooks for the sanitizer pass (the boxes run with xnack off, so device-side ASan is not
 * available): scratch buffers allocated AFTER phast_debug_set_guard_bytes(b) carry a b-byte guard band filled with 0xA5
 * on either side; ..._debug_check_guards blocks until the device is idle and counts the band bytes a kernel overwrote */
void phast_debug_set_guard_bytes(size_t bytes);
int phast_planner_dit64_debug_check_guards(const phast_planner_dit64 *p, size_t *bad_bytes);
int phast_planner_dit32_debug_check_guards(const phast_planner_dit32 *p, size_t *bad_bytes);
/* ... and of a real planner: the scratches of its inner N/2-point planner, which the real transforms run in */
int phast_planner_r2c64_debug_check_guards(const phast_planner_r2c64 *p, size_t *bad_bytes);
int phast_planner_r2c32_debug_check_guards(const phast_planner_r2c32 *p, size_t *bad_bytes);

/* No C++ exception leaves the library (every entry point is a function-try-block, csrc/c_abi.hip): host memory exhaustion
 * comes back as PHAST_ERR_ALLOC, any other exception as PHAST_ERR_HIP with its text in phast_last_hip_error().  Test hook:
 * throws std::bad_alloc (1), std::runtime_error (2) or an int (3) INSIDE the library and returns what the caller would see. */
int phast_debug_throw(int what);

/* debug hook (no device needed): the wisdom entry a planner on a device with `cus` compute units of architecture `arch` (the
 * gfx number read as hex digits, gfx950 -> 0x950; 0 = unknown, matches anything) applies for (element size in bytes,
 * PHAST_TUNE_* kind, log2 of the caller's length, batch bucket).  Returns the layer it came from (0 built-in, 1 PHAST_WISDOM
 * file, 2 imported, 3 measured here) and writes its plan ("heuristic" or the plan text) to buf; -1 when no entry applies. */
int phast_debug_wisdom_lookup(size_t elem_bytes, int kind, unsigned log_n, unsigned bucket, int cus, int arch, char *buf,
                              size_t buf_len);

/* debug hook: device buffer of [3 passes][4096 workgroups][16] s_memtime stamps written by the tile kernels while
 * set (NULL = off; adds drains, so never leave it on while measuring).  tools/trace_tile.py decodes it. */
void phast_debug_set_trace(unsigned long long *d_trace);

/* ---- measurement hook (bench.py "roofline"): runs `reps` batched forward transforms in place on the given
 * buffers with hipEvents recorded on `stream` around every pass kernel; pass_ms[i] = average duration of pass i
 * in milliseconds (sum over batch chunks), *n_passes = number of passes (<= 3).  Blocks until done. ---- */
int phast_planner_dit64_time_passes(const phast_planner_dit64 *p, double *d_reals, double *d_imags, size_t batch,
                                    size_t dist, int reps, float *pass_ms, int *n_passes, void *stream);
int phast_planner_dit32_time_passes(const phast_planner_dit32 *p, float *d_reals, float *d_imags, size_t batch,
                                    size_t dist, int reps, float *pass_ms, int *n_passes, void *stream);

/* the same for a real transform: slots 0..n-2 = the passes of the inner N/2-point complex transform, slot n-1 = the
 * untangle sweep (r2c.rs:150-242); a transform whose inner N/2 <= 8192 runs as ONE kernel (*n_passes = 1, slot 0 not
 * timed per kernel -- use stream events around the call).  pass_ms must hold 4 floats. */
int phast_planner_r2c64_time_passes(const phast_planner_r2c64 *p, const double *d_input, double *d_output_re,
                                    double *d_output_im, size_t batch, size_t in_dist, size_t out_dist, int reps,
                                    float *pass_ms, int *n_passes, void *stream);
int phast_planner_r2c32_time_passes(const phast_planner_r2c32 *p, const float *d_input, float *d_output_re,
                                    float *d_output_im, size_t batch, size_t in_dist, size_t out_dist, int reps,
                                    float *pass_ms, int *n_passes, void *stream);
/* ... and for the inverse real transform (r2c.rs:740-895): slots 0..np-1 = the passes of the inner transform -- the first
 * of them forms z from the half-spectrum on load wherever its fused form exists (every multi-pass plan whose first pass
 * is a generic tile; csrc/c2r_fused.hpp), slot np = the preprocess sweep (r2c.rs:263-433) otherwise. */
int phast_planner_r2c64_time_c2r_passes(const phast_planner_r2c64 *p, const double *d_input_re, const double *d_input_im,
                                        double *d_output, size_t batch, size_t in_dist, size_t out_dist, int reps,
                                        float *pass_ms, int *n_passes, void *stream);
int phast_planner_r2c32_time_c2r_passes(const phast_planner_r2c32 *p, const float *d_input_re, const float *d_input_im,
                                        float *d_output, size_t batch, size_t in_dist, size_t out_dist, int reps,
                                        float *pass_ms, int *n_passes, void *stream);
/* tuning hook, as phast_planner_dit*_set_plan but for the inner N/2-point transform of a real-transform planner (R2C and
 * C2R then run that plan for every batch size; np = 0 restores the library's own plans).  tools/sweep_real.py */
int phast_planner_r2c64_set_inner_plan(phast_planner_r2c64 *p, const unsigned *log_rows, const unsigned *tile_logs,
                                       size_t n_passes, unsigned points_log);
int phast_planner_r2c32_set_inner_plan(phast_planner_r2c32 *p, const unsigned *log_rows, const unsigned *tile_logs,
                                       size_t n_passes, unsigned points_log);

/* plan of the inner N/2-point complex transform, as phast_planner_dit*_describe */
int phast_planner_r2c64_describe(const phast_planner_r2c64 *p, char *buf, size_t buf_len);
int phast_planner_r2c32_describe(const phast_planner_r2c32 *p, char *buf, size_t buf_len);

#ifdef __cplusplus
}
#endif
#endif
