// oxhip_host.hpp -- host-side helpers shared by the C-ABI translation units (oxhip_api.hip: RRT /
// RRTConnect batches and primitives; oxhip_prm_api.hip: PRM).  Not installed.
//
// What oxhip_api.hip builds from them: the table of spaces (kSpaces, one row per oxhip_space); the RRT batch handle in parts (Trees,
// Goals, Obstacles, Cells, Shadow, Solve, Paths, Reval, Star with Star::Wiring), each a set of DevBufs with a bind(DevParams&), a
// PooledStream for the handle and one for the wiring, a PhaseClock per timed service (Solve's made with the handle, Paths' and
// Reval's by their first call); create() in its steps -- validate_config (pure host code: space_resolution, se_space_resolution,
// so3_space_resolution and so2_space_resolution below), fill_params, alloc_common (alloc_star at its place, then the binds), the
// kernel kind, alloc_cells, alloc_shadow --; the filters of refresh_filter (connect_sphere_grid, midpoint_filter, star_edge_filter)
// and pair_params over the pure threshold functions below; and the entry points' shared openings (setup_done / in_range / ready),
// rules (drop_derived, reset_tree_caches, upload_radii) and bodies (copy_tree, op_batch with a PooledStream).  oxhip_prm_api.hip takes
// the same resolution helpers for validate_prm_config, DevBuf for its workspaces and its roadmap, prm_bfs_path, the graph search of
// Planner::solve, and a PhaseClock per service for its phase times.  Both take the shortcut's shape, rounds and matrix expansion
// (shortcut_shape, shortcut_rounds, shortcut_matrix_bytes); shortcut_shape is the one piece the kernels of shortcut_core.hip call too.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <deque>
#include <limits>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/oxmpl_hip.h"

namespace oxhip {

inline thread_local std::string g_last_error;

inline int32_t fail(int32_t code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return ::oxhip::fail(OXHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define OX_TRY(expr) do { int32_t s_ = (expr); if (s_ != OXHIP_OK) return s_; } while (0)

inline int32_t select_device(int32_t device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(OXHIP_ERR_NO_DEVICE, "no HIP device visible (liboxmpl_hip has no CPU fallback)");
    if (device < 0 || device >= count) return fail(OXHIP_ERR_BAD_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return OXHIP_OK;
}

// largest x with sqrt(x) <= r under correctly rounded binary64 sqrt, so that
//   sqrt(d2) >  r  <=>  d2 >  T      (sphere validity, strict)
//   sqrt(d2) <= r  <=>  d2 <= T      (ball goal)
// hold exactly and the kernels need no sqrt per obstacle.  r < 0 -> -1, NaN -> NaN.
inline double sqrt_le_threshold(double r) {
    if (std::isnan(r)) return r;
    if (r < 0.0) return -1.0;
    if (std::isinf(r)) return r;
    double x = r * r;
    if (std::isinf(x)) x = std::numeric_limits<double>::max();
    while (std::sqrt(x) > r) x = std::nextafter(x, -1.0);
    for (;;) {
        double y = std::nextafter(x, std::numeric_limits<double>::infinity());
        if (std::isinf(y) || std::sqrt(y) > r) break;
        x = y;
    }
    return x;
}

// largest x with sqrt(x) < r:  sqrt(d2) < r  <=>  d2 <= T  (PRM's strict connection radius, prm.rs:134).
// r <= 0 or NaN -> -1 (no d2 >= 0 qualifies); +inf -> DBL_MAX (every finite d2 qualifies).
inline double sqrt_lt_threshold(double r) {
    if (std::isnan(r) || r <= 0.0) return -1.0;
    if (std::isinf(r)) return std::numeric_limits<double>::max();
    return sqrt_le_threshold(std::nextafter(r, 0.0));
}

// rand 0.9 Bernoulli::new
inline uint64_t bernoulli_p_int(double p) {
    if (p == 1.0) return ~0ull;
    double v = p * 18446744073709551616.0;
    if (!(v > 0.0)) return 0;
    if (v >= 18446744073709551616.0) return ~0ull;
    return (uint64_t)v;
}

constexpr double kMaxMagnitude = 1e150;  // keeps every squared difference finite

// ---- the RRT batch's obstacle filters (oxhip_api.hip: refresh_filter, pair_params): pure arithmetic, tests/cpp/test_rrt_filter_host.cpp
// rrt_connect.hip's sphere grid lists sphere j in a cell when the squared distance centre - cell box is <= this: the sphere's own
// validity threshold (valid iff d2 > t) with a relative 1e-9 of slack.  A sphere that is not listed contains no state of the cell.
inline double connect_grid_threshold(double r) {
    const double t = sqrt_le_threshold(r);
    return std::isfinite(t) ? (t > 0.0 ? t * (1.0 + 1e-9) : t) : t;
}
// Conservative midpoint filter of a motion check.  Every state the check interpolates lies within h of the segment's midpoint --
// h = half the motion's length with a relative 1e-6, plus an absolute 1e-9 * (largest coordinate magnitude in play), orders of
// magnitude above the few-ulp rounding of the interpolation -- so d2(centre, mid) > (r + h)^2 proves sphere (centre, r) valid for
// the whole motion.  The filter never decides a motion invalid.  A negative radius is never hit (-1: no d2 is below it).
inline double midpoint_threshold(double r, double h) {
    if (std::isnan(r) || std::isinf(r)) return r < 0.0 ? -1.0 : std::numeric_limits<double>::infinity();
    if (r < 0.0) return -1.0;                      // distance > negative radius always holds
    return (r + h) * (r + h) * (1.0 + 1e-9);
}
// RRT*'s edge kernel keeps sphere j when d2(centre, mid) <= (r_j + h)^2 (1 + 1e-9) with h anywhere in [h_lo, h_hi] (motions up to
// search_radius long): its grid is built for the largest such ball (either end of h's range when r_j < 0).
inline double star_edge_threshold(double r, double h_lo, double h_hi) {
    const double a = (r + h_lo) * (r + h_lo), c = (r + h_hi) * (r + h_hi);
    return (std::isnan(r) || std::isinf(r)) ? std::numeric_limits<double>::infinity() : std::fmax(a, c) * (1.0 + 1e-9) * (1.0 + 1e-12);
}
// The largest coordinate magnitude the midpoint filter's absolute margin (1e-9 of it) has to cover, at least 1: the bounds, the
// sphere centres and, where given, the starts.  A planner's launch passes the starts: its thresholds are fixed before the launch
// and a start may lie outside the bounds, whereas every other tree node lies inside them.  The kernels that check motions between
// states a caller may have planted (shortcut_core.hip, rrt_revalidate.hip) pass null: they widen this base per motion by both of
// its ends (SeqSpace::motion_margin, seq_space.hpp), so the starts are in play there without being named here.
inline double filter_maxabs(const oxhip_rrt_config& cfg, const std::vector<double>& centres, const std::vector<double>* starts) {
    double maxabs = 1.0;
    for (uint32_t k = 0; k < 2 * cfg.dim; ++k) maxabs = std::fmax(maxabs, std::fabs(cfg.bounds[k]));
    if (starts) for (double v : *starts) maxabs = std::fmax(maxabs, std::fabs(v));
    for (double v : centres) maxabs = std::fmax(maxabs, std::fabs(v));
    return maxabs;
}

// ---- the shortcut of a path (shortcut_core.hip, DESIGN.md sections 18 and 25): its shape, a batch's rounds and the bit matrix as
// bytes.  Pure arithmetic, tests/cpp/test_shortcut_host.cpp.  A path of L original states with every edge in m parts:
struct ShortcutShape {
    uint64_t rows;     // M = (L - 1) m + 1 rows q_0 .. q_{M-1}, q_{k m} = p_k; 0 for no path
    uint64_t window;   // W = span * m, span = max_span original edges (0 or beyond L - 1: all L - 1); pairs (u, v) with v - u <= W
    uint64_t words;    // 64-bit words of the bit matrix: bit (d - 2) * M + u is check_motion(q_u, q_{u + d}), 2 <= d <= W
    uint64_t checks;   // pairs of the window that are not on one original edge: the motion checks evaluated
};
__host__ __device__ inline ShortcutShape shortcut_shape(uint32_t L, uint32_t m, uint32_t max_span) {
    if (L == 0) return ShortcutShape{0, 0, 0, 0};
    const uint32_t full = L - 1u;
    ShortcutShape s;
    s.rows = (uint64_t)full * m + 1u;
    s.window = (uint64_t)(max_span == 0u || max_span > full ? full : max_span) * m;
    s.words = s.window < 2u ? 0u : ((s.window - 1u) * s.rows + 63u) / 64u;
    // pairs with 1 <= d <= W: sum of (M - d); of them on one edge: m (m + 1) / 2 per original edge
    s.checks = s.window * s.rows - s.window * (s.window + 1u) / 2u - (uint64_t)full * ((uint64_t)m * (m + 1ull) / 2ull);
    return s;
}

constexpr uint64_t kShortcutMatrixBytes = 1ull << 30;   // a round's bit matrices stay within this
constexpr uint64_t kShortcutRowsMax = 0x7FFFFFFFull;    // of one path: the kernels index its rows with 32 bits (an RRT path is shorter:
                                                        // two chains of at most 2^30 nodes, less the shared connection point)

// whether a round can hold this path at all
inline bool shortcut_fits(const ShortcutShape& s, uint64_t budget_bytes) { return s.rows <= kShortcutRowsMax && s.words <= budget_bytes / 8u; }

// The rounds of a batch of n paths: paths are taken in order while their matrices stay within budget_bytes together and, with
// max_paths given (not 0), while the round holds fewer than that many; a round holds at least one path.  first = the first path of
// every round, then n (empty for n = 0).  False, with `refused` the first such path, when a path does not fit a round of its own.
inline bool shortcut_rounds(const uint32_t* len, uint32_t n, uint32_t m, uint32_t max_span, uint64_t budget_bytes, uint32_t max_paths,
                            std::vector<uint32_t>& first, uint32_t& refused) {
    first.clear();
    uint64_t words = 0;
    for (uint32_t q = 0; q < n; ++q) {
        const ShortcutShape s = shortcut_shape(len[q], m, max_span);
        if (!shortcut_fits(s, budget_bytes)) { refused = q; return false; }
        if (q == 0 || (words + s.words) * 8u > budget_bytes || (max_paths != 0 && q - first.back() >= max_paths)) {
            first.push_back(q);
            words = 0;
        }
        words += s.words;
    }
    if (n) first.push_back(n);
    return true;
}

// The bit matrix of one path as the M x M byte matrix of the test hooks: out[u * M + v] for u < v <= u + W is 1 on one original
// edge and the pair's bit otherwise; every other byte is 0.
inline void shortcut_matrix_bytes(const uint64_t* bits, uint32_t L, uint32_t m, uint32_t max_span, uint8_t* out) {
    const ShortcutShape s = shortcut_shape(L, m, max_span);
    const uint64_t M = s.rows;
    std::fill(out, out + M * M, (uint8_t)0);
    for (uint64_t u = 0; u + 1 < M; ++u)
        for (uint64_t v = u + 1; v < M && v - u <= s.window; ++v) {
            const uint64_t slot = (v - u - 2) * M + u;   // (read for pairs that are not on one edge only: those have d >= 2)
            out[u * M + v] = u / m == (v - 1) / m ? 1 : (uint8_t)((bits[slot >> 6] >> (slot & 63u)) & 1ull);
        }
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        if (p) { (void)hipFree(p); p = nullptr; }
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc((void**)&p, count * sizeof(T));
    }
    hipError_t reserve(size_t count) { return n < count ? alloc(count) : hipSuccess; }   // grow to at least `count`; contents not preserved
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
};

// The clock of one service of a handle: n events, made with their owner (which create(), or the service's first call, builds once
// the device is current) and destroyed with it: like DevBuf, after destroy() has made the device current.  The owner names its
// marks with an enum.  mark(i) records mark i on the stream; once the stream is synchronised, ms(i, j) is the GPU time from mark i
// to mark j (0 where the runtime refuses).  A service reads only marks that it recorded itself, in the same call.  `made` is the
// first error of making the events, for the owner's create() to refuse with; event(i) is for a launcher that records a mark itself.
struct PhaseClock {
    std::vector<hipEvent_t> ev;
    hipError_t made = hipSuccess;
    explicit PhaseClock(int n) : ev(n, nullptr) {
        for (hipEvent_t& e : ev) {
            const hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) { e = nullptr; if (made == hipSuccess) made = r; }
        }
    }
    PhaseClock(const PhaseClock&) = delete;
    ~PhaseClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t mark(int i, hipStream_t s) { return hipEventRecord(ev[i], s); }
    hipEvent_t event(int i) const { return ev[i]; }
    double ms(int i, int j) const { float t = 0.f; return hipEventElapsedTime(&t, ev[i], ev[j]) == hipSuccess ? (double)t : 0.0; }
};

// what create() answers when one of its device allocations failed
inline int32_t alloc_failed(hipError_t e) { return fail(OXHIP_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(e)); }

// Streams are recycled.  On this stack hipStreamCreate takes 1.5 ms and hipStreamDestroy 1.7 ms (rocprofv3 --hip-trace of
// tools/bench_single.py, profiles/r3_single/hip_api_stats.csv) -- more than every other call of a one-problem Planner::solve together,
// kernel included -- so a destroyed planner's stream (drained) goes to a small per-device pool and the next create takes it from
// there.  Pooled streams live until the process ends.
hipError_t oxhip_stream_acquire(int device, hipStream_t* out);   // non-blocking streams; `device` is the current device
void oxhip_stream_release(int device, hipStream_t s);            // synchronises s first

struct PooledStream {   // a pooled stream, held by one call of a stand-alone primitive or by a handle, and given back with its holder
    hipStream_t s = nullptr;
    int device = 0;
    PooledStream() = default;
    PooledStream(const PooledStream&) = delete;
    ~PooledStream() { close(); }
    void close() { if (s) oxhip_stream_release(device, s); s = nullptr; }
    operator hipStream_t() const { return s; }
    hipError_t take(int dev) { device = dev; return oxhip_stream_acquire(dev, &s); }   // `dev` is the current device
    int32_t acquire(int dev) {
        hipError_t e = take(dev);
        if (e != hipSuccess) return fail(OXHIP_ERR_HIP, std::string("oxhip_stream_acquire(device, &ts.s): ") + hipGetErrorString(e));
        return OXHIP_OK;
    }
};
template <typename T>
int32_t to_device(DevBuf<T>& buf, const T* host, size_t n, hipStream_t s) {
    HIP_TRY(buf.alloc(n));
    if (n) HIP_TRY(hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    return OXHIP_OK;
}
template <typename T>
int32_t to_host(T* host, const DevBuf<T>& buf, size_t n, hipStream_t s) {
    if (n) HIP_TRY(hipMemcpyAsync(host, buf.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return OXHIP_OK;
}
inline int32_t upload(DevBuf<double>& buf, const std::vector<double>& host, hipStream_t s) {
    HIP_TRY(buf.alloc(host.size()));
    if (!host.empty()) {
        HIP_TRY(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return OXHIP_OK;
}

// RealVectorStateSpace::new + get_maximum_extent + get_longest_valid_segment_length for a config's bounds:
// validates what the reference rejects (real_vector_state_space.rs:69-93,239-244), clamps the fraction
// (rvss.rs:121-129) and returns res = lvsl * 0.1 (rrt.rs:97, prm.rs:168).
inline int32_t space_resolution(uint32_t dim, const double* bounds, double& fraction, double& res) {
    if (dim == 0 || dim > OXHIP_MAX_DIM) return fail(OXHIP_ERR_BAD_ARG, "dim must be in 1..8");
    for (uint32_t k = 0; k < dim; ++k) {
        double lo = bounds[2 * k], hi = bounds[2 * k + 1];
        if (!std::isfinite(lo) || !std::isfinite(hi))  // real_vector_state_space.rs:239-241
            return fail(OXHIP_ERR_UNBOUNDED, "dimension " + std::to_string(k) + " is unbounded");
        if (lo >= hi) return fail(OXHIP_ERR_ZERO_VOLUME, "lower bound >= upper bound");  // rvss.rs:78-83,242-244
        if (std::fabs(lo) > kMaxMagnitude || std::fabs(hi) > kMaxMagnitude)
            return fail(OXHIP_ERR_BAD_ARG, "bounds beyond 1e150 would overflow squared distances");
    }
    // set_longest_valid_segment_fraction clamp (rvss.rs:121-129)
    if (fraction > 0.0 && fraction <= 1.0) {} else if (fraction <= 0.0) fraction = 0.0; else fraction = 1.0;
    // get_maximum_extent (rvss.rs:103-118): sequential sum of squared widths, sqrt
    double acc = 0.0;
    for (uint32_t k = 0; k < dim; ++k) {
        double w = bounds[2 * k + 1] - bounds[2 * k];
        double sq = w * w;
        acc = acc + sq;
    }
    double extent = std::sqrt(acc);
    double lvsl = extent * fraction;  // rvss.rs:251-253
    res = lvsl * 0.1;                 // rrt.rs:97
    if (!(res > 0.0)) return fail(OXHIP_ERR_BAD_ARG, "longest valid segment length is 0: check_motion would never terminate");
    return OXHIP_OK;
}

// SE(2) / SE(3): the first n bounds pairs are (x, y[, z]), validated as RealVectorStateSpace::new(n, ..) (which also clamps the
// fraction); extent = extent_xy[z] + 0.5 * PI (so2_state_space.rs:78-80; the rotation's extent likewise), lvsl = extent * fraction,
// res = lvsl * 0.1.  Sequential sum of squared widths, one sqrt, one add, two multiplies.
inline int32_t se_space_resolution(uint32_t n, const double* bounds, double& fraction, double& res) {
    OX_TRY(space_resolution(n, bounds, fraction, res));
    double acc = 0.0;
    for (uint32_t k = 0; k < n; ++k) { double w = bounds[2 * k + 1] - bounds[2 * k]; double sq = w * w; acc = acc + sq; }
    const double extent = std::sqrt(acc) + 0.5 * 3.14159265358979323846;
    const double lvsl = extent * fraction;
    res = lvsl * 0.1;
    return OXHIP_OK;
}

// SO3StateSpace::new + get_longest_valid_segment_length for a config whose bounds carry (cx, cy, cz, cw, max_angle)
// (include/oxmpl_hip.h, OXHIP_SPACE_SO3): validates the centre and max_angle as so3_state_space.rs:57-76 does (a negative
// max_angle is StateSpaceError::InvalidAngularDistance; max_angle.min(PI), NaN giving PI as f64::min does), clamps the fraction
// (:234-236) and returns res = 0.5 * PI * fraction * 0.1 (extent 0.5 * PI, :81-84; rrt.rs:97, prm.rs:168).  No SO(3) distance
// exceeds 0.5 * PI, which bounds the step count of every motion.
// (the centre / max_angle part, shared with SE(3), whose bounds carry the same five values behind the (x, y, z) bounds)
inline int32_t so3_rotation_bounds(const double* bounds, double& max_angle) {
    for (uint32_t k = 0; k < 4; ++k)
        if (!(std::fabs(bounds[k]) <= kMaxMagnitude)) return fail(OXHIP_ERR_BAD_ARG, "SO(3) centre not finite or beyond 1e150");
    const double pi = 3.14159265358979323846;
    max_angle = bounds[4];
    if (max_angle < 0.0) return fail(OXHIP_ERR_ZERO_VOLUME, "SO(3): max_angle must not be negative");
    max_angle = std::isnan(max_angle) ? pi : std::fmin(max_angle, pi);
    return OXHIP_OK;
}
inline int32_t so3_space_resolution(uint32_t dim, const double* bounds, double& fraction, double& res, double& max_angle) {
    if (dim != 4) return fail(OXHIP_ERR_BAD_ARG, "SO(3) states are quaternions (x, y, z, w): dim must be 4");
    const double pi = 3.14159265358979323846;
    OX_TRY(so3_rotation_bounds(bounds, max_angle));
    if (fraction > 0.0 && fraction <= 1.0) {} else if (fraction <= 0.0) fraction = 0.0; else fraction = 1.0;
    const double lvsl = 0.5 * pi * fraction;
    res = lvsl * 0.1;
    if (!(res > 0.0)) return fail(OXHIP_ERR_BAD_ARG, "longest valid segment length is 0: check_motion would never terminate");
    if (0.5 * pi / res > 1e6) return fail(OXHIP_ERR_BAD_ARG, "more than 1e6 validity checks per edge");
    return OXHIP_OK;
}

// SO2StateSpace::new + get_longest_valid_segment_length for a config whose bounds[0..1] are (lo, hi) (include/oxmpl_hip.h,
// OXHIP_SPACE_SO2): lo >= hi is StateSpaceError::InvalidBound (so2_state_space.rs:57-74; written !(lo < hi), which refuses a NaN
// bound too), the bounds are clamped to [-PI, PI], the fraction is clamped (:83-91) and res = PI * fraction * 0.1 (extent PI,
// :78-80; rrt.rs:97).  No SO(2) distance exceeds PI, which bounds the step count of every motion.
inline int32_t so2_space_resolution(const double* bounds, double& fraction, double& res, double& lo, double& hi) {
    const double pi = 3.14159265358979323846;
    if (!(bounds[0] < bounds[1])) return fail(OXHIP_ERR_ZERO_VOLUME, "SO(2): lower bound >= upper bound");
    lo = bounds[0] > -pi ? bounds[0] : -pi;   // f64::max / f64::min
    hi = bounds[1] < pi ? bounds[1] : pi;
    if (fraction > 0.0 && fraction <= 1.0) {} else if (fraction <= 0.0) fraction = 0.0; else fraction = 1.0;
    const double lvsl = pi * fraction;
    res = lvsl * 0.1;
    if (!(res > 0.0)) return fail(OXHIP_ERR_BAD_ARG, "longest valid segment length is 0: check_motion would never terminate");
    if (pi / res > 1e6) return fail(OXHIP_ERR_BAD_ARG, "more than 1e6 validity checks per edge");
    return OXHIP_OK;
}

// PRM's Planner::solve from the query sets on (prm.rs:266-304) and reconstruct_path (prm.rs:189-208), on the CSR roadmap (every
// row ascending): pure host code.  flags[i] & 2 marks a goal milestone; start_conn are the start connections, enqueued twice, as
// the reference does.  The clock starts here and is read at every pop (prm.rs:285-287); timeout_s = +inf: no limit, and no clock read.
// found: out_chain = goal milestone ... root connection (the path's states in reverse).  Starts on a 64-byte line: the same
// instructions ran 10 % slower on SO(3) roadmaps where the linker happened to start them at 16 mod 64 -- the figure to check again
// is tools/bench_prm_queries.py's SO(3) loop.host_bfs_ms_sum (profiles/prm_handle_parts/README.md, section 1).
enum class PrmBfs { found, unreachable, timed_out, empty_set };
__attribute__((aligned(64))) inline PrmBfs prm_bfs_path(const std::vector<uint32_t>& offsets, const std::vector<uint32_t>& nbrs, const std::vector<uint8_t>& flags,
                           const std::vector<uint32_t>& start_conn, double timeout_s, std::vector<uint32_t>& out_chain) {
    const auto t0 = std::chrono::steady_clock::now();
    out_chain.clear();
    bool any_goal = false;
    for (uint8_t f : flags) any_goal = any_goal || (f & 2);
    if (start_conn.empty() || !any_goal) return PrmBfs::empty_set;   // prm.rs:266-268
    std::deque<uint32_t> queue(start_conn.begin(), start_conn.end());
    std::vector<int64_t> parent(flags.size(), -2);   // parent_map: -2 absent, -1 = Some(None)
    std::vector<uint8_t> visited(flags.size(), 0);
    for (uint32_t s : start_conn) { queue.push_back(s); parent[s] = -1; visited[s] = 1; }
    while (!queue.empty()) {
        const uint32_t cur = queue.front();
        queue.pop_front();
        if (std::isfinite(timeout_s) && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return PrmBfs::timed_out;
        if (flags[cur] & 2) {   // goal_indices.contains(&current_idx)
            for (int64_t c = cur; c >= 0; c = parent[(size_t)c]) out_chain.push_back((uint32_t)c);
            return PrmBfs::found;
        }
        for (uint32_t e = offsets[cur]; e < offsets[cur + 1]; ++e) {
            const uint32_t nb = nbrs[e];
            if (!visited[nb]) { visited[nb] = 1; parent[nb] = (int64_t)cur; queue.push_back(nb); }
        }
    }
    return PrmBfs::unreachable;   // prm.rs:304
}

}  // namespace oxhip
