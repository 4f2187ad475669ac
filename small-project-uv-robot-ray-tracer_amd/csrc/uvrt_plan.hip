// uvrt_plan.hip -- duration planning (include/uvrt.h "duration planning"): capture of the per-position exposure
// E[p][t] from the folded planes of traced batches, the covering LP over it and its f64 repair and certificate.
//
// The LP in row-normalised form: A[i][p] = E[p][t_i] * r_i with r_i = s / (den_t * m') over the required rows t_i,
//     minimise 1.d  subject to  A d >= 1, d >= 0.
// It has few columns (P <= 256 positions) and many rows (every required triangle), and only about P rows are tight at
// the optimum.  Solver: cutting planes.  The GPU evaluates A_i d for every row in f64 (k_plan_rowcheck); the host reads
// the values back and picks the most violated rows, which the GPU gathers (k_plan_gather); the host solves the LP
// restricted to the rows gathered so far (uvrt_plan_lp.h: warm-started simplex on its dual) and repeats until the
// certified gap is <= rel_gap or a cap is reached.  The restricted dual y (zero on the other rows) is feasible for the
// full dual once divided by max_p (A^T y)_p, so LB = sum y / max_p (A^T y)_p is a certified lower bound at every round.
// Every result is bit-reproducible: no float atomics, fixed reduction orders, no dependence on the CU count.
//
// Bounded solve (uvrt_plan_solve_bounded): d_p >= lower[p], fixed columns d_p = lower[p].  With x = lower + e and
// base_t = (sum_p E[p][t] lower[p]) r_t the residual problem  min 1.e  s.t.  sum_{free p} E[p][t] r_t e_p >= rho_t = 1 - base_t
// on the ACTIVE rows (base_t < 1 and a free column reaches t) is the same homogeneous LP with the row scale r_t / rho_t and
// without the fixed columns: the <true> instantiations of the row kernels, the same host loop.
//
// Two kinds of plan, fixed at its begin: E holds uint32 photon counts (uvrt_plan_begin, uvrt_plan_capture_batch) or f64
// expected counts of the direct gather (uvrt_plan_begin_expected, uvrt_plan_capture_expected).  The row kernels and the
// host loop take the element type ET as a template argument and do the same arithmetic on (double)E[p][t]; only the row
// sums that class a triangle differ: exact uint64 for counts, f64 in ascending p for expected values.
//
// An expected plan may carry V, the variance of every element of E (uvrt_plan_begin_expected_variance: the capture adds the
// gather's variance plane beside its expected plane).  uvrt_plan_lower_confidence then replaces E by max(0, E - z sqrt(V)),
// once, and everything above plans for that bound: one solver, no solver kernel knows about V.
#include "uvrt_ctx.h"
#include "uvrt_plan_lp.h"

#include <algorithm>
#include <limits>

using namespace uvrt;
using namespace uvrt_impl;

namespace {

constexpr double PLAN_RHO_MIN = 1e-9; // floor of a bounded solve's rho_t = 1 - base_t (what it costs)
constexpr int PLAN_MAX_P = 256;      // positions (uvrt_plan_begin; LDS copy of the durations in the row kernels): the
                                     // restricted simplex is measured to solve within a second up to here

struct CaptureParams {
    uint32_t* E;
    uint32_t* overflow;      // raised when a sum leaves uint32 (the global counts of a reduced batch included)
    const int32_t* folded;
    int32_t T, count;
    int32_t row[MAX_BATCH], plane[MAX_BATCH];
};

// E[row_k][t] += folded plane of launch k (planes in physical order; several launches may share a row)
__global__ __launch_bounds__(256) void k_plan_capture(CaptureParams p)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.T) return;
    for (int k = 0; k < p.count; ++k) {
        const int32_t v = p.folded[(int64_t)p.plane[k] * p.T + t];
        uint32_t* e = p.E + (int64_t)p.row[k] * p.T + t;
        const uint64_t sum = (uint64_t)*e + (uint32_t)v;
        if (sum > 0xFFFFFFFFull) atomicOr(p.overflow, 1u);
        *e = (uint32_t)sum;
    }
}

// X[t] += expected[t] on one row of an expected plan (X points at the row); a sum that is not finite or is negative raises
// `bad`, the analogue of the uint32 overflow flag
__global__ __launch_bounds__(256) void k_plan_capture_expected(double* __restrict__ X, const double* __restrict__ expected,
                                                              int32_t T, uint32_t* __restrict__ bad)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const double sum = X[t] + expected[t];
    if (!(sum >= 0.0) || sum == std::numeric_limits<double>::infinity()) atomicOr(bad, 1u);
    X[t] = sum;
}

// uvrt_plan_lower_confidence: X = max(0, X - z * sqrt(V)) over all P x T elements, one rounding per operator (this file is
// built without contraction).  z = 0 leaves X as it is: X - 0 * sqrt(V) = X for the finite, non-negative sums a plan holds.
__global__ __launch_bounds__(256) void k_plan_lower_confidence(double* __restrict__ X, const double* __restrict__ V, int64_t n,
                                                              double z)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double lo = X[i] - z * sqrt(V[i]);
    X[i] = lo > 0.0 ? lo : 0.0;
}

// the type a row of E is summed in when k_plan_classify classes it
template <typename ET> struct RowSum { using type = uint64_t; };
template <> struct RowSum<double> { using type = double; };

// what a bounded solve adds to the row kernels: the lower bounds (as f64), the fixed columns and the row scale's terms
struct BoundsDev {
    const double* lower;     // f64[P]
    const uint8_t* fixed;    // uint8[P]
    float s, Nf;
    double mprime;
    int32_t all_met;         // min_dose <= 0: every row that would be class 0, 4 or 5 is class 4
};

// class of every triangle (0 required, 1 unreachable, 2 unresolved, 3 masked out), per block: counts and areas per class.
// B (bounded solve): a row of class 0 splits into 4 (met by the bounds: base_t >= 1), 5 (short: no free column reaches it)
// and 0 (active), whose rho_t = max(1 - base_t, PLAN_RHO_MIN) goes to rho[t]; base_t in f64, columns in ascending order.
template <bool B, typename ET>
__global__ __launch_bounds__(256) void k_plan_classify(const ET* __restrict__ E, int32_t P, int32_t T,
                                                      const uint8_t* __restrict__ mask, const float* __restrict__ area,
                                                      uint32_t min_photons, uint8_t* __restrict__ cls,
                                                      int32_t* __restrict__ blk_cnt, double* __restrict__ blk_area,
                                                      BoundsDev bd, double* __restrict__ rho)
{
    constexpr int NC = B ? 6 : 4;
    __shared__ int32_t s_cnt[4][NC];
    __shared__ double s_area[256];
    __shared__ double s_low[B ? PLAN_MAX_P : 1];
    __shared__ uint8_t s_fix[B ? PLAN_MAX_P : 1];
    if (B) {
        for (int j = threadIdx.x; j < P; j += 256) { s_low[j] = bd.lower[j]; s_fix[j] = bd.fixed[j]; }
        __syncthreads();
    }
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int k = -1;
    double a = 0;
    if (t < T) {
        typename RowSum<ET>::type sum = 0, fre = 0;
        double base = 0.0;
        for (int p = 0; p < P; ++p) {
            const ET e = E[(int64_t)p * T + t];
            sum += e;
            if (B) {
                if (!s_fix[p]) fre += e;
                base += (double)e * s_low[p];
            }
        }
        const float at = area[t];
        a = at;
        if (mask && !mask[t]) k = 3;
        else if (sum == 0 || !(at > 0.0f)) k = 1;      // no photon (or no area: no dose is defined)
        else if (sum < min_photons) k = 2;
        else if (!B) k = 0;
        else if (bd.all_met) k = 4;
        else {
            const float den = at * bd.Nf;                             // computeDosage's f32 denominator
            const double r = (double)bd.s / ((double)den * bd.mprime);
            const double b = base * r;
            if (b >= 1.0) k = 4;
            else if (fre == 0) k = 5;
            else { k = 0; rho[t] = fmax(1.0 - b, PLAN_RHO_MIN); }
        }
        cls[t] = (uint8_t)k;
    }
    for (int q = 0; q < NC; ++q) {
        const uint64_t b = __builtin_amdgcn_ballot_w64(k == q);
        if (lane == 0) s_cnt[w][q] = __popcll(b);
    }
    for (int q = 0; q < NC; ++q) {
        s_area[threadIdx.x] = k == q ? a : 0.0;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) s_area[threadIdx.x] += s_area[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            blk_area[blockIdx.x * NC + q] = s_area[0];
            blk_cnt[blockIdx.x * NC + q] = s_cnt[0][q] + s_cnt[1][q] + s_cnt[2][q] + s_cnt[3][q];
        }
        __syncthreads();
    }
}

// the required (B: the active) rows in ascending triangle order (ballot + block offsets) and their scale r (B: r / rho);
// E is not read, so one kernel serves both element types
template <bool B>
__global__ __launch_bounds__(256) void k_plan_compact(const uint32_t* __restrict__ E, int32_t P, int32_t T,
                                                     const uint8_t* __restrict__ cls, const float* __restrict__ area,
                                                     const int32_t* __restrict__ blk_off, float s, float Nf, double mprime,
                                                     int32_t* __restrict__ rows, double* __restrict__ rd,
                                                     const double* __restrict__ rho)
{
    __shared__ int32_t s_w[4];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool req = t < T && cls[t] == 0;
    const uint64_t b = __builtin_amdgcn_ballot_w64(req);
    if (lane == 0) s_w[w] = __popcll(b);
    __syncthreads();
    if (!req) return;
    int off = blk_off[blockIdx.x];
    for (int j = 0; j < w; ++j) off += s_w[j];
    off += __popcll(b & ((1ull << lane) - 1ull));
    const float den = area[t] * Nf;                               // computeDosage's f32 denominator
    const double r = (double)s / ((double)den * mprime);
    rows[off] = t;
    rd[off] = B ? r / rho[t] : r;
}

// row j of the gathered block: A[sel_j][p] = E[p][rows[sel_j]] * r_{sel_j} in f64; B: P counts the free columns only
// and cols[p] is the p-th of them (the fixed columns never reach the simplex)
template <bool B, typename ET>
__global__ __launch_bounds__(256) void k_plan_gather(const ET* __restrict__ E, int32_t T, int32_t P,
                                                    const int32_t* __restrict__ rows, const double* __restrict__ rd,
                                                    const int64_t* __restrict__ sel, int32_t nsel, double* __restrict__ out,
                                                    const int32_t* __restrict__ cols)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)nsel * P) return;
    const int64_t j = k / P, p = B ? (int64_t)cols[k % P] : k % P, i = sel[j];
    out[k] = (double)E[p * T + rows[i]] * rd[i];
}

// f64 check of durations d over the required rows: per block min_i A_i d (and A_i d per row); rows with A_i d = 0 raise
// their best position (largest E, lowest index) to what covers the row alone (integer max of positive f64 bits:
// order independent).  B: the fixed columns are left out of the sum and of the choice of the best position.
template <bool B, typename ET>
__global__ __launch_bounds__(256) void k_plan_rowcheck(const ET* __restrict__ E, int32_t T, int32_t P, int64_t NR,
                                                      const int32_t* __restrict__ rows, const double* __restrict__ rd,
                                                      const double* __restrict__ d, double* __restrict__ blk_min,
                                                      unsigned long long* __restrict__ raise, int32_t* __restrict__ zero_rows,
                                                      double* __restrict__ ratio, const uint8_t* __restrict__ fixed)
{
    __shared__ double s_d[PLAN_MAX_P];
    __shared__ double s_min[256];
    __shared__ uint8_t s_fix[B ? PLAN_MAX_P : 1];
    for (int j = threadIdx.x; j < P; j += 256) {
        s_d[j] = d[j];
        if (B) s_fix[j] = fixed[j];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double mn = std::numeric_limits<double>::infinity();
    if (i < NR) {
        const int64_t t = rows[i];
        double ad = 0.0;
        ET best = 0;
        int bp = 0;
        for (int q = 0; q < P; ++q) {
            if (B && s_fix[q]) continue;
            const ET e = E[(int64_t)q * T + t];
            ad += (double)e * s_d[q];
            if (e > best) { best = e; bp = q; }
        }
        ad *= rd[i];
        mn = ad;
        if (ratio) ratio[i] = ad;
        if (ad == 0.0 && raise) {
            const double need = 1.0 / ((double)best * rd[i]);
            atomicMax(&raise[bp], (unsigned long long)__double_as_longlong(need));
            atomicAdd(zero_rows, 1);
        }
    }
    s_min[threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blk_min[blockIdx.x] = s_min[0];
}

// the bounded solve's final check, in x-space: per block the minimum over the required rows (classes 0 and 4) of
// (sum_p E[p][t] x_p) * r_t, every column in ascending order, in f64
template <typename ET>
__global__ __launch_bounds__(256) void k_plan_xcheck(const ET* __restrict__ E, int32_t T, int32_t P,
                                                    const uint8_t* __restrict__ cls, const float* __restrict__ area,
                                                    float s, float Nf, double mprime, const double* __restrict__ x,
                                                    double* __restrict__ blk_min)
{
    __shared__ double s_x[PLAN_MAX_P];
    __shared__ double s_min[256];
    for (int j = threadIdx.x; j < P; j += 256) s_x[j] = x[j];
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    double mn = std::numeric_limits<double>::infinity();
    if (t < T && (cls[t] == 0 || cls[t] == 4)) {
        double acc = 0.0;
        for (int q = 0; q < P; ++q) acc += (double)E[(int64_t)q * T + t] * s_x[q];
        const float den = area[t] * Nf;
        mn = acc * ((double)s / ((double)den * mprime));
    }
    s_min[threadIdx.x] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blk_min[blockIdx.x] = s_min[0];
}

// D_t(d) = (float)(s * sum_p E[p][t] d_p / den_t), f64 sum in position order, computeDosage's f32 denominator
template <typename ET>
__global__ __launch_bounds__(256) void k_plan_model_dose(const ET* __restrict__ E, int32_t T, int32_t P,
                                                        const double* __restrict__ d, const float* __restrict__ area,
                                                        float Nf, float s, float* __restrict__ out, int32_t first, int32_t count)
{
    __shared__ double s_d[PLAN_MAX_P];
    for (int j = threadIdx.x; j < P; j += 256) s_d[j] = d[j];
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int64_t t = (int64_t)first + j;
    double acc = 0.0;
    for (int q = 0; q < P; ++q) acc += (double)E[(int64_t)q * T + t] * s_d[q];
    const double num = (double)s * acc;
    const float den = area[t] * Nf;
    out[j] = (float)(num / (double)den);
}

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

struct PlanState {
    int32_t P = 0;
    bool expected = false;               // E holds f64 expected counts (uvrt_plan_begin_expected), not uint32 photon counts
    DevBuf E;
    bool with_variance = false;          // an expected plan with V, the variance of every element of E, beside it (uvrt_plan_begin_expected_variance)
    DevBuf V;                            // f64[P][T]
    bool lowered = false;                // uvrt_plan_lower_confidence has turned E into its lower confidence bound: no more captures
    std::vector<uint64_t> rays;         // rays of this context's launches captured per position (uint32 overflow guard)
    int64_t captures = 0;
    bool solved = false;
    float s = 0, Nf = 0;                 // of the last solve (uvrt_plan_model_dose)
    DevBuf overflow;                     // uint32 flag of k_plan_capture / k_plan_capture_expected
    DevBuf cls, mask, blk_cnt, blk_area, blk_off, rows, rd, dd, blk_min, raise, zrows, outf, ratio, sel, gath;
    DevBuf lowd, fixd, rho, cols, xmin;  // bounded solve: lower as f64[P], fixed uint8[P], rho f64[T], the free columns, k_plan_xcheck
};

namespace uvrt_impl {
void plan_drop(uvrt_ctx* c)
{
    if (!c || !c->plan) return;
    (void)hipStreamSynchronize(c->stream);
    delete c->plan;
    c->plan = nullptr;
}
}  // namespace uvrt_impl

namespace {

struct RowCheck { double min_ratio; int32_t zero_rows; };

// the minimum over the per-block minima of a row kernel
double min_of(const std::vector<double>& blk)
{
    double mn = std::numeric_limits<double>::infinity();
    for (double v : blk) mn = std::min(mn, v);
    return mn;
}

// the smallest f32 >= x that survives SaveRoute / LoadRoute
float round_up_f32(double x)
{
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, INFINITY);
    return uvrt_plan_round_trip_up(f);
}

// the element type of the plan's exposure matrix: f(ET()) with ET = double (expected counts) or uint32_t (photon counts)
template <class F>
int with_element_type(const PlanState& S, F&& f)
{
    return S.expected ? f(double()) : f(uint32_t());
}

// k_plan_rowcheck of host durations d64; with `raise` the raise values come back in raise_out, with ratio_out A_i d per row
// (bounded: the fixed columns of S.fixd are left out)
template <typename ET>
int row_check(uvrt_ctx* c, PlanState& S, bool bounded, int64_t NR, const std::vector<double>& d64, bool raise,
              RowCheck* out, std::vector<double>* raise_out, std::vector<double>* ratio_out = nullptr)
{
    const unsigned nbr = nblocks(NR, 256);
    HIP_TRY(hipMemcpyAsync(S.dd.p, d64.data(), (size_t)S.P * 8, hipMemcpyHostToDevice, c->stream));
    if (raise) {
        HIP_TRY(hipMemsetAsync(S.raise.p, 0, (size_t)S.P * 8, c->stream));
        HIP_TRY(hipMemsetAsync(S.zrows.p, 0, 4, c->stream));
    }
    hipLaunchKernelGGL((bounded ? k_plan_rowcheck<true, ET> : k_plan_rowcheck<false, ET>), dim3(nbr), dim3(256), 0, c->stream,
                       (const ET*)S.E.as<ET>(), c->T, S.P, NR,
                       (const int32_t*)S.rows.as<int32_t>(), (const double*)S.rd.as<double>(), (const double*)S.dd.as<double>(),
                       S.blk_min.as<double>(), raise ? S.raise.as<unsigned long long>() : nullptr,
                       S.zrows.as<int32_t>(), ratio_out ? S.ratio.as<double>() : nullptr,
                       bounded ? (const uint8_t*)S.fixd.as<uint8_t>() : nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<double> mn(nbr);
    if (ratio_out) {
        ratio_out->resize((size_t)NR);
        HIP_TRY(hipMemcpyAsync(ratio_out->data(), S.ratio.p, (size_t)NR * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(mn.data(), S.blk_min.p, (size_t)nbr * 8, hipMemcpyDeviceToHost, c->stream));
    int32_t z = 0;
    std::vector<unsigned long long> rb;
    if (raise) {
        rb.resize(S.P);
        HIP_TRY(hipMemcpyAsync(&z, S.zrows.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rb.data(), S.raise.p, (size_t)S.P * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->min_ratio = min_of(mn);
    out->zero_rows = z;
    if (raise_out) {
        raise_out->assign(S.P, 0.0);
        for (int p = 0; p < S.P && raise; ++p) { double v; memcpy(&v, &rb[p], 8); (*raise_out)[p] = v; }
    }
    return UVRT_OK;
}

// k_plan_xcheck of host durations x (every column): the minimum over the required rows of D_t(x) / m'
template <typename ET>
int x_check(uvrt_ctx* c, PlanState& S, double mprime, const std::vector<double>& x, double* min_ratio)
{
    const unsigned nbt = nblocks(c->T, 256);
    if (int rc = S.xmin.ensure((size_t)nbt * 8, false, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(S.dd.p, x.data(), (size_t)S.P * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_plan_xcheck<ET>, dim3(nbt), dim3(256), 0, c->stream, (const ET*)S.E.as<ET>(), c->T, S.P,
                       (const uint8_t*)S.cls.as<uint8_t>(), (const float*)c->area.as<float>(), S.s, S.Nf, mprime,
                       (const double*)S.dd.as<double>(), S.xmin.as<double>());
    HIP_TRY(hipGetLastError());
    std::vector<double> mn(nbt);
    HIP_TRY(hipMemcpyAsync(mn.data(), S.xmin.p, (size_t)nbt * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *min_ratio = min_of(mn);
    return UVRT_OK;
}

template <typename ET>
int plan_solve_t(uvrt_ctx* c, const char* who, const uvrt_plan_params* prm, const uvrt_plan_bounds* bounds, float* out,
                 uvrt_plan_report* rep, uvrt_plan_bounds_report* brep);

int plan_solve(uvrt_ctx* c, const char* who, const uvrt_plan_params* prm, const uvrt_plan_bounds* bounds, float* out,
               uvrt_plan_report* rep, uvrt_plan_bounds_report* brep)
{
    if (!c || !c->plan) return fail(UVRT_ERR_INVALID, "%s: no plan (uvrt_plan_begin)", who);
    return with_element_type(*c->plan, [&](auto et) { return plan_solve_t<decltype(et)>(c, who, prm, bounds, out, rep, brep); });
}

// uvrt_plan_begin (uint32 counts) and uvrt_plan_begin_expected (f64 expected counts)
int plan_begin(uvrt_ctx* c, const char* who, int32_t positions, bool expected, bool with_variance = false)
{
    if (!c || !c->have_scene) return fail(UVRT_ERR_INVALID, "%s: null context or no scene", who);
    if (positions < 1 || positions > PLAN_MAX_P)
        return fail(UVRT_ERR_INVALID, "%s: positions %d outside [1,%d]", who, positions, PLAN_MAX_P);
    if ((uint64_t)positions * (uint64_t)c->T >= ((uint64_t)1 << 32))
        return fail(UVRT_ERR_INVALID, "%s: %d positions x %d triangles exceed 2^32 counters", who, positions, c->T);
    if (int rc = set_device(c)) return rc;
    plan_drop(c);
    c->plan = new PlanState();
    c->plan->P = positions;
    c->plan->expected = expected;
    c->plan->rays.assign(positions, 0);
    c->plan->with_variance = with_variance;
    if (int rc = c->plan->E.ensure((size_t)positions * (size_t)c->T * (expected ? 8 : 4), true, c->stream)) { plan_drop(c); return rc; }
    if (with_variance)
        if (int rc = c->plan->V.ensure((size_t)positions * (size_t)c->T * 8, true, c->stream)) { plan_drop(c); return rc; }
    if (int rc = c->plan->overflow.ensure(4, true, c->stream)) { plan_drop(c); return rc; }
    return UVRT_OK;
}

}  // namespace

extern "C" {

// smallest float >= v that "%.8g" (SaveRoute) prints back to itself through strtof (LoadRoute's sscanf "%f")
float uvrt_plan_round_trip_up(float v)
{
    if (!std::isfinite(v)) return v;
    for (int k = 0; k < 256; ++k) {
        char b[64];
        snprintf(b, sizeof b, "%.8g", (double)v);
        if (strtof(b, nullptr) == v) return v;
        v = nextafterf(v, INFINITY);
    }
    return v;
}

int uvrt_plan_begin(uvrt_ctx* c, int32_t positions) { return plan_begin(c, "uvrt_plan_begin", positions, false); }

int uvrt_plan_begin_expected(uvrt_ctx* c, int32_t positions) { return plan_begin(c, "uvrt_plan_begin_expected", positions, true); }

int uvrt_plan_begin_expected_variance(uvrt_ctx* c, int32_t positions)
{
    return plan_begin(c, "uvrt_plan_begin_expected_variance", positions, true, true);
}

int uvrt_plan_end(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_plan_end: null context");
    if (int rc = set_device(c)) return rc;
    plan_drop(c);
    return UVRT_OK;
}

int uvrt_plan_capture_batch(uvrt_ctx* c, const int32_t* pos, int32_t count)
{
    if (!c || !c->plan) return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_batch: no plan (uvrt_plan_begin)");
    if (c->plan->expected) return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_batch: the plan holds expected values (uvrt_plan_capture_expected)");
    if (c->b_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_batch: no traced batch");
    if (!pos || count != c->b_count)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_batch: %d positions for a batch of %d launches", count, c->b_count);
    PlanState& S = *c->plan;
    std::vector<uint64_t> rays = S.rays;
    for (int k = 0; k < count; ++k) {
        if (pos[k] < 0 || pos[k] >= S.P)
            return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_batch: position %d of launch %d outside [0,%d)", pos[k], k, S.P);
        rays[pos[k]] += (uint64_t)c->b_n;
        if (rays[pos[k]] > 0xFFFFFFFFull)
            return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_batch: the photons of position %d would overflow the uint32 counts", pos[k]);
        // (this context's rays only: after a reduce the global counts are checked by k_plan_capture itself)
    }
    if (int rc = uvrt_fold_batch(c)) return rc;          // set_device + join_all; a no-op after a reduce
    CaptureParams p;
    memset(&p, 0, sizeof p);
    p.E = S.E.as<uint32_t>();
    p.overflow = S.overflow.as<uint32_t>();
    p.folded = c->bs[c->b_set].folded.as<int32_t>();
    p.T = c->T;
    p.count = count;
    for (int k = 0; k < count; ++k) { p.row[k] = pos[k]; p.plane[k] = c->b_phys[k]; }
    hipLaunchKernelGGL(k_plan_capture, dim3(nblocks(c->T, 256)), dim3(256), 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    S.rays = rays;
    ++S.captures;
    return UVRT_OK;
}

int uvrt_plan_capture_expected(uvrt_ctx* c, int32_t position)
{
    if (!c || !c->plan || !c->plan->expected)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_expected: no plan of expected values (uvrt_plan_begin_expected)");
    PlanState& S = *c->plan;
    if (position < 0 || position >= S.P)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_expected: position %d outside [0,%d)", position, S.P);
    if (S.lowered)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_capture_expected: the plan holds its lower confidence bound (uvrt_plan_lower_confidence): no more captures");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    if (S.with_variance)
        if (int rc = ensure_variance(c)) return rc;
    hipLaunchKernelGGL(k_plan_capture_expected, dim3(nblocks(c->T, 256)), dim3(256), 0, c->stream,
                       S.E.as<double>() + (size_t)position * c->T, (const double*)c->derived.expected.as<double>(), c->T,
                       S.overflow.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (S.with_variance) {      // V[position][t] += variance[t]: the same sum, the same flag
        hipLaunchKernelGGL(k_plan_capture_expected, dim3(nblocks(c->T, 256)), dim3(256), 0, c->stream,
                           S.V.as<double>() + (size_t)position * c->T, (const double*)c->derived.variance.as<double>(), c->T,
                           S.overflow.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    ++S.captures;
    return UVRT_OK;
}

int uvrt_plan_solve(uvrt_ctx* c, const uvrt_plan_params* prm, float* out, uvrt_plan_report* rep)
{
    return plan_solve(c, "uvrt_plan_solve", prm, nullptr, out, rep, nullptr);
}

int uvrt_plan_solve_bounded(uvrt_ctx* c, const uvrt_plan_params* prm, const uvrt_plan_bounds* bounds, float* out,
                            uvrt_plan_report* rep, uvrt_plan_bounds_report* brep)
{
    return plan_solve(c, "uvrt_plan_solve_bounded", prm, bounds, out, rep, brep);
}

int uvrt_plan_model_dose(uvrt_ctx* c, const float* durations, float* out, int32_t first, int32_t count)
{
    if (!c || !c->plan || !c->plan->solved) return fail(UVRT_ERR_INVALID, "uvrt_plan_model_dose: no solved plan");
    if (!durations || !out || first < 0 || count < 0 || (int64_t)first + count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_model_dose: bad range");
    if (count == 0) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    PlanState& S = *c->plan;
    int rc;
    if ((rc = S.dd.ensure((size_t)S.P * 8, false, c->stream))) return rc;
    if ((rc = S.outf.ensure((size_t)c->T * 4, false, c->stream))) return rc;
    std::vector<double> d(S.P);
    for (int p = 0; p < S.P; ++p) d[p] = durations[p];
    HIP_TRY(hipMemcpyAsync(S.dd.p, d.data(), (size_t)S.P * 8, hipMemcpyHostToDevice, c->stream));
    with_element_type(S, [&](auto et) {
        using ET = decltype(et);
        hipLaunchKernelGGL(k_plan_model_dose<ET>, dim3(nblocks(count, 256)), dim3(256), 0, c->stream, (const ET*)S.E.as<ET>(),
                           c->T, S.P, (const double*)S.dd.as<double>(), (const float*)c->area.as<float>(), S.Nf, S.s, S.outf.as<float>(),
                           first, count);
        return UVRT_OK;
    });
    HIP_TRY(hipGetLastError());
    return copy_sync(c, out, S.outf.p, (size_t)count * 4, hipMemcpyDeviceToHost);
}

int uvrt_plan_read_exposure(uvrt_ctx* c, int32_t position, uint32_t* out, int32_t first, int32_t count)
{
    if (!c || !c->plan) return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure: no plan");
    if (c->plan->expected) return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure: the plan holds expected values (uvrt_plan_read_exposure_expected)");
    if (position < 0 || position >= c->plan->P)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure: position %d outside [0,%d)", position, c->plan->P);
    if (!range_ok(out, first, count, c->T)) return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure: bad range");
    return range_copy(c, c->plan->E.as<uint32_t>() + (size_t)position * c->T, 4, out, first, count, hipMemcpyDeviceToHost);
}

// test hook: host values into E[position][first .. first + count) of a counts plan.  It counts as a capture; the rays per
// position and the overflow flag stay as they are (they describe traced batches, and a test writes what no trace gives).
int uvrt_plan_write_exposure(uvrt_ctx* c, int32_t position, const uint32_t* in, int32_t first, int32_t count)
{
    if (!c || !c->plan) return fail(UVRT_ERR_INVALID, "uvrt_plan_write_exposure: no plan");
    if (c->plan->expected) return fail(UVRT_ERR_INVALID, "uvrt_plan_write_exposure: the plan holds expected values (uvrt_write_expected, uvrt_plan_capture_expected)");
    if (position < 0 || position >= c->plan->P)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_write_exposure: position %d outside [0,%d)", position, c->plan->P);
    if (!range_ok(in, first, count, c->T)) return fail(UVRT_ERR_INVALID, "uvrt_plan_write_exposure: bad range");
    if (int rc = range_copy(c, c->plan->E.as<uint32_t>() + (size_t)position * c->T, 4, const_cast<uint32_t*>(in), first, count,
                            hipMemcpyHostToDevice))
        return rc;
    ++c->plan->captures;
    return UVRT_OK;
}

int uvrt_plan_read_exposure_expected(uvrt_ctx* c, int32_t position, double* out, int32_t first, int32_t count)
{
    if (!c || !c->plan || !c->plan->expected)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure_expected: no plan of expected values (uvrt_plan_begin_expected)");
    if (position < 0 || position >= c->plan->P)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure_expected: position %d outside [0,%d)", position, c->plan->P);
    if (!range_ok(out, first, count, c->T)) return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure_expected: bad range");
    return range_copy(c, c->plan->E.as<double>() + (size_t)position * c->T, 8, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_plan_read_exposure_variance(uvrt_ctx* c, int32_t position, double* out, int32_t first, int32_t count)
{
    if (!c || !c->plan || !c->plan->with_variance)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure_variance: no plan with a variance (uvrt_plan_begin_expected_variance)");
    if (position < 0 || position >= c->plan->P)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure_variance: position %d outside [0,%d)", position, c->plan->P);
    if (!range_ok(out, first, count, c->T)) return fail(UVRT_ERR_INVALID, "uvrt_plan_read_exposure_variance: bad range");
    return range_copy(c, c->plan->V.as<double>() + (size_t)position * c->T, 8, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_plan_lower_confidence(uvrt_ctx* c, double z)
{
    if (!c || !c->plan || !c->plan->with_variance)
        return fail(UVRT_ERR_INVALID, "uvrt_plan_lower_confidence: no plan with a variance (uvrt_plan_begin_expected_variance)");
    PlanState& S = *c->plan;
    if (S.lowered) return fail(UVRT_ERR_INVALID, "uvrt_plan_lower_confidence: the plan already holds its lower confidence bound");
    if (!std::isfinite(z) || !(z >= 0.0)) return fail(UVRT_ERR_INVALID, "uvrt_plan_lower_confidence: z must be finite and >= 0");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    const int64_t n = (int64_t)S.P * c->T;
    if (z != 0.0) {             // (z = 0: X - 0 * sqrt(V) is X; not launched, so that every bit stays whatever X holds)
        hipLaunchKernelGGL(k_plan_lower_confidence, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, S.E.as<double>(),
                           (const double*)S.V.as<double>(), n, z);
        HIP_TRY(hipGetLastError());
    }
    S.lowered = true;
    return UVRT_OK;
}

// a range of the last solve's row classes
static int read_classes(uvrt_ctx* c, const char* who, uint8_t* out, int32_t first, int32_t count)
{
    if (!c || !c->plan || !c->plan->solved) return fail(UVRT_ERR_INVALID, "%s: no solved plan", who);
    if (!range_ok(out, first, count, c->T)) return fail(UVRT_ERR_INVALID, "%s: bad range", who);
    return range_copy(c, c->plan->cls.p, 1, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_plan_read_required(uvrt_ctx* c, uint8_t* out, int32_t first, int32_t count)
{
    if (int rc = read_classes(c, "uvrt_plan_read_required", out, first, count)) return rc;
    for (int32_t i = 0; i < count; ++i) out[i] = out[i] == 0 || out[i] == 4 ? 1 : 0;     // a bounded solve: active or met by the bounds
    return UVRT_OK;
}

int uvrt_plan_read_classes(uvrt_ctx* c, uint8_t* out, int32_t first, int32_t count)
{
    return read_classes(c, "uvrt_plan_read_classes", out, first, count);
}

}  // extern "C"

namespace {

// uvrt_plan_solve (bounds == nullptr) and uvrt_plan_solve_bounded, in stages; what one stage leaves for the next is a member.
// Bounds that bind nothing (all-zero lower, no fixed column) take the unbounded instantiations of every kernel: the same
// arithmetic, bit for bit.
struct Solve {
    uvrt_ctx* c; const char* who; const uvrt_plan_params* prm; const uvrt_plan_bounds* bounds;      // the call's arguments
    float* out; uvrt_plan_report* rep; uvrt_plan_bounds_report* brep;
    PlanState& S = *c->plan;
    const int32_t T = c->T, P = S.P;
    const unsigned nbt = nblocks(T, 256);
    // the bounds: lower as f64, the fixed flags, the free columns in ascending order
    std::vector<double> low = std::vector<double>(P, 0.0);
    std::vector<uint8_t> fix = std::vector<uint8_t>(P, 0);
    std::vector<int32_t> cols;
    int32_t PF = 0;                       // the columns the simplex sees (P when unbounded)
    bool bounded = false;
    double lower_total = 0.0;
    double m = 0.0, mprime = 0.0;         // the minimum dose, and with the margin
    int64_t NR = 0;                       // the rows of the LP: the required ones (bounded: the active ones)
    bool done = false;                    // classify_rows left nothing for the LP to decide: out and the report are final
    std::vector<double> d64 = std::vector<double>(P, 0.0);   // a duration per column (bounded: the excess over lower)
    double best_lb = 0.0;
    int it = 0;                           // rounds of cutting planes

    int check_arguments();
    template <typename ET> int classify_rows();
    template <typename ET> int cutting_planes();
    template <typename ET> int repair();
    template <typename ET> int round_to_f32();
};

// the arguments, the bounds, the captures' overflow flag; clears the reports
int Solve::check_arguments()
{
    if (c->plan->captures == 0) return fail(UVRT_ERR_INVALID, "%s: nothing captured (uvrt_plan_capture_batch)", who);
    if (!prm || !out || !rep) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (prm->photons_per_position < 1 || prm->photons_per_position > (int64_t)0xFFFFFFFFll)
        return fail(UVRT_ERR_INVALID, "%s: %lld photons per position overflow the uint32 counts", who,
                    (long long)prm->photons_per_position);
    if (!(prm->scaled_power > 0.0f) || !std::isfinite(prm->scaled_power) || !std::isfinite(prm->min_dose) ||
        !(prm->margin >= 0.0) || !(prm->rel_gap > 0.0))
        return fail(UVRT_ERR_INVALID, "%s: scaled_power > 0, finite min_dose, margin >= 0 and rel_gap > 0 required", who);
    for (int p = 0; p < P && bounds; ++p) {
        if (bounds->lower) {
            const float l = bounds->lower[p];
            if (!std::isfinite(l) || !(l >= 0.0f))
                return fail(UVRT_ERR_INVALID, "%s: lower[%d] must be finite and >= 0", who, p);
            low[p] = l;
            lower_total += l;
            bounded = bounded || l != 0.0f;
        }
        if (bounds->fixed && bounds->fixed[p]) { fix[p] = 1; bounded = true; }
    }
    for (int p = 0; p < P; ++p)
        if (!fix[p]) cols.push_back(p);
    PF = (int32_t)cols.size();
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    {
        uint32_t of = 0;
        HIP_TRY(hipMemcpyAsync(&of, S.overflow.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (of && c->plan->expected) return fail(UVRT_ERR_INVALID, "%s: a captured expected value is not finite or is negative", who);
        if (of) return fail(UVRT_ERR_INVALID, "%s: a captured count overflowed uint32 (over 2^32 - 1 photons of one position)", who);
    }
    memset(rep, 0, sizeof *rep);
    rep->positions = P;
    if (brep) {
        memset(brep, 0, sizeof *brep);
        brep->fixed_columns = P - PF;
        brep->free_columns = PF;
        brep->lower_total = lower_total;
    }
    return UVRT_OK;
}

// classes, exclusion statistics, the required rows compacted
template <typename ET>
int Solve::classify_rows()
{
    int rc;
    const int NC = bounded ? 6 : 4;
    m = prm->min_dose;
    mprime = m * (1.0 + prm->margin);
    if ((rc = S.cls.ensure((size_t)T, false, c->stream))) return rc;
    if ((rc = S.blk_cnt.ensure((size_t)nbt * NC * 4, false, c->stream))) return rc;
    if ((rc = S.blk_area.ensure((size_t)nbt * NC * 8, false, c->stream))) return rc;
    if ((rc = S.blk_off.ensure((size_t)nbt * 4, false, c->stream))) return rc;
    const uint8_t* dmask = nullptr;
    if (prm->mask) {
        if ((rc = S.mask.ensure((size_t)T, false, c->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(S.mask.p, prm->mask, (size_t)T, hipMemcpyHostToDevice, c->stream));
        dmask = S.mask.as<uint8_t>();
    }
    BoundsDev bd;
    memset(&bd, 0, sizeof bd);
    if (bounded) {
        if ((rc = S.lowd.ensure((size_t)P * 8, false, c->stream))) return rc;
        if ((rc = S.fixd.ensure((size_t)P, false, c->stream))) return rc;
        if ((rc = S.cols.ensure((size_t)std::max(PF, 1) * 4, false, c->stream))) return rc;
        if ((rc = S.rho.ensure((size_t)T * 8, false, c->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(S.lowd.p, low.data(), (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(S.fixd.p, fix.data(), (size_t)P, hipMemcpyHostToDevice, c->stream));
        if (PF > 0) HIP_TRY(hipMemcpyAsync(S.cols.p, cols.data(), (size_t)PF * 4, hipMemcpyHostToDevice, c->stream));
        bd.lower = S.lowd.as<double>();
        bd.fixed = S.fixd.as<uint8_t>();
        bd.s = prm->scaled_power;
        bd.Nf = (float)prm->photons_per_position;
        bd.mprime = mprime;
        bd.all_met = !(m > 0.0);
    }
    const uint32_t min_ph = (uint32_t)std::max(1, prm->min_photons);
    hipLaunchKernelGGL((bounded ? k_plan_classify<true, ET> : k_plan_classify<false, ET>), dim3(nbt), dim3(256), 0, c->stream,
                       (const ET*)S.E.as<ET>(), P, T, dmask, (const float*)c->area.as<float>(), min_ph,
                       S.cls.as<uint8_t>(), S.blk_cnt.as<int32_t>(), S.blk_area.as<double>(), bd,
                       bounded ? S.rho.as<double>() : nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> bc((size_t)nbt * NC), boff(nbt);
    std::vector<double> ba((size_t)nbt * NC);
    HIP_TRY(hipMemcpyAsync(bc.data(), S.blk_cnt.p, bc.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ba.data(), S.blk_area.p, ba.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t cnt[6] = {0, 0, 0, 0, 0, 0};
    double area[6] = {0, 0, 0, 0, 0, 0};
    for (unsigned b = 0; b < nbt; ++b) {
        boff[b] = (int32_t)cnt[0];
        for (int q = 0; q < NC; ++q) { cnt[q] += bc[b * NC + q]; area[q] += ba[b * NC + q]; }
    }
    rep->required = (int32_t)(cnt[0] + cnt[4]); rep->unreachable = (int32_t)cnt[1];
    rep->unresolved = (int32_t)cnt[2]; rep->masked_out = (int32_t)cnt[3];
    rep->area_required = bounded ? area[0] + area[4] : area[0]; rep->area_unreachable = area[1];
    rep->area_unresolved = area[2]; rep->area_masked_out = area[3];
    if (brep) {
        brep->met_by_lower = (int32_t)cnt[4]; brep->short_rows = (int32_t)cnt[5];
        brep->area_met_by_lower = area[4]; brep->area_short = area[5];
    }
    NR = cnt[0];
    S.s = prm->scaled_power;
    S.Nf = (float)prm->photons_per_position;
    S.solved = true;
    if (NR == 0 || !(m > 0.0)) {
        done = true;
        if (!bounded) {
            for (int p = 0; p < P; ++p) out[p] = 0.0f;
            rep->status = UVRT_PLAN_CONVERGED;
            rep->min_dose_ratio = std::numeric_limits<double>::infinity();
            return UVRT_OK;
        }
        // the bounds meet every required row (or there is none): out = lower
        double total = 0, minx = std::numeric_limits<double>::infinity();
        int used = 0;
        for (int p = 0; p < P; ++p) { out[p] = (float)low[p]; total += low[p]; used += low[p] > 0.0; }
        if (m > 0.0 && cnt[4] > 0) {
            if ((rc = S.dd.ensure((size_t)P * 8, false, c->stream))) return rc;
            if ((rc = x_check<ET>(c, S, mprime, low, &minx))) return rc;
        }
        rep->used_positions = used;
        rep->total_duration = total;
        rep->lower_bound = total;
        rep->status = UVRT_PLAN_CONVERGED;
        rep->min_dose_ratio = m > 0.0 ? minx * (mprime / m) : minx;
        return UVRT_OK;
    }
    const unsigned nbr = nblocks(NR, 256);
    if ((rc = S.rows.ensure((size_t)NR * 4, false, c->stream))) return rc;
    if ((rc = S.rd.ensure((size_t)NR * 8, false, c->stream))) return rc;
    if ((rc = S.ratio.ensure((size_t)NR * 8, false, c->stream))) return rc;
    for (DevBuf* b : {&S.dd, &S.raise})
        if ((rc = b->ensure((size_t)P * 8, false, c->stream))) return rc;
    if ((rc = S.blk_min.ensure((size_t)nbr * 8, false, c->stream))) return rc;
    if ((rc = S.zrows.ensure(4, false, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(S.blk_off.p, boff.data(), (size_t)nbt * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bounded ? k_plan_compact<true> : k_plan_compact<false>, dim3(nbt), dim3(256), 0, c->stream,
                       (const uint32_t*)S.E.as<uint32_t>(), P, T,
                       (const uint8_t*)S.cls.as<uint8_t>(), (const float*)c->area.as<float>(), (const int32_t*)S.blk_off.as<int32_t>(),
                       S.s, S.Nf, mprime, S.rows.as<int32_t>(), S.rd.as<double>(),
                       bounded ? (const double*)S.rho.as<double>() : nullptr);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

// Cutting planes from the uniform plan: rows W gathered so far (AW: |W| x PF, f64), exact LP over W, repeat.
// d64 holds every column (a fixed one stays 0: the row kernels skip it); the simplex sees the PF free ones.
template <typename ET>
int Solve::cutting_planes()
{
    int rc;
    const int max_rounds = prm->max_iterations > 0 ? prm->max_iterations : 200;
    const int per_round = std::max(64, 2 * PF);
    std::vector<double> dlp, ratio, AW, best_d;
    std::vector<int64_t> W;
    std::vector<uint8_t> inW((size_t)NR, 0);
    uvrt_plan_lp::RestrictedLP lp(PF);
    int64_t pivots = 0;
    double best_ub = std::numeric_limits<double>::infinity();
    auto offer = [&](double min_ratio) {      // d64, scaled to cover its least covered row, is the plan to beat
        double sd = 0;
        for (double v : d64) sd += v;
        if (min_ratio > 0.0 && sd / min_ratio < best_ub) {
            best_ub = sd / min_ratio;
            best_d = d64;
            for (double& v : best_d) v /= min_ratio;
        }
    };
    {
        std::vector<double> ones(P, 1.0);
        RowCheck r1;
        if ((rc = row_check<ET>(c, S, bounded, NR, ones, false, &r1, nullptr))) return rc;
        for (int p : cols) d64[p] = r1.min_ratio > 0.0 ? 1.0 / r1.min_ratio : 1.0;
    }
    for (;;) {
        RowCheck rck;
        if ((rc = row_check<ET>(c, S, bounded, NR, d64, false, &rck, nullptr, &ratio))) return rc;
        offer(rck.min_ratio);
        if (std::isfinite(best_ub) && (best_ub - best_lb) <= prm->rel_gap * best_ub) break;
        if (it >= max_rounds) break;
        // the most violated rows not yet in W (round 0: the least covered ones under the uniform plan)
        std::vector<int64_t> cand;
        for (int64_t i = 0; i < NR; ++i)
            if (!inW[i] && (it == 0 || ratio[i] < 1.0)) cand.push_back(i);
        if (cand.empty()) break;          // d covers every row: the restricted optimum is global
        const size_t take = std::min(cand.size(), (size_t)per_round);
        std::partial_sort(cand.begin(), cand.begin() + take, cand.end(), [&](int64_t a, int64_t b) {
            return ratio[a] < ratio[b] || (ratio[a] == ratio[b] && a < b);
        });
        cand.resize(take);
        std::sort(cand.begin(), cand.end());
        if ((rc = S.sel.ensure(take * 8, false, c->stream))) return rc;
        if ((rc = S.gath.ensure(take * (size_t)PF * 8, false, c->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(S.sel.p, cand.data(), take * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL((bounded ? k_plan_gather<true, ET> : k_plan_gather<false, ET>), dim3(nblocks((int64_t)take * PF, 256)), dim3(256), 0,
                           c->stream, (const ET*)S.E.as<ET>(), T, PF, (const int32_t*)S.rows.as<int32_t>(),
                           (const double*)S.rd.as<double>(), (const int64_t*)S.sel.as<int64_t>(), (int32_t)take, S.gath.as<double>(),
                           bounded ? (const int32_t*)S.cols.as<int32_t>() : nullptr);
        HIP_TRY(hipGetLastError());
        const size_t old = AW.size();
        AW.resize(old + take * (size_t)PF);
        HIP_TRY(hipMemcpyAsync(AW.data() + old, S.gath.p, take * (size_t)PF * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int64_t i : cand) { inW[i] = 1; W.push_back(i); }
        lp.add_rows(AW.data() + old, (int64_t)take);
        const bool solved = lp.solve(50 * (lp.rows() + PF) + 1000, &pivots);
        std::vector<double> yW;
        lp.solution(&yW, &dlp);                 // an interrupted solve still leaves a feasible basis: a certificate
        for (int f = 0; f < PF; ++f) d64[cols[f]] = dlp[f];
        // certificate of the restricted dual (zero on the rows outside W): LB = sum y / max_p (A^T y)_p, in f64
        std::vector<double> g(PF, 0.0);
        double sy = 0;
        for (size_t j = 0; j < W.size(); ++j) {
            if (yW[j] == 0.0) continue;
            sy += yW[j];
            for (int p = 0; p < PF; ++p) g[p] += AW[j * PF + p] * yW[j];
        }
        const double gmax = *std::max_element(g.begin(), g.end());
        if (gmax > 0.0) best_lb = std::max(best_lb, sy / gmax);
        ++it;
        if (!solved) {                          // pivot cap: keep what is certified, report the gap
            RowCheck rlast;
            if ((rc = row_check<ET>(c, S, bounded, NR, d64, false, &rlast, nullptr))) return rc;
            offer(rlast.min_ratio);
            break;
        }
    }
    if (std::isfinite(best_ub)) d64 = best_d;
    return UVRT_OK;
}

// repair (f64): cover rows without coverage by their best position, drop positions the plan does not need, scale
template <typename ET>
int Solve::repair()
{
    int rc;
    {
        double dmax = 0;
        for (double v : d64) dmax = std::max(dmax, v);
        for (double& v : d64) if (v <= 1e-7 * dmax) v = 0.0;
    }
    RowCheck rck{};
    std::vector<double> raise;
    for (int round = 0; round < 4; ++round) {
        if ((rc = row_check<ET>(c, S, bounded, NR, d64, true, &rck, &raise))) return rc;
        if (rck.zero_rows == 0) break;
        for (int p = 0; p < P; ++p) d64[p] = std::max(d64[p], raise[p]);
    }
    if (rck.zero_rows != 0 || !(rck.min_ratio > 0.0)) return fail(UVRT_ERR_INVALID, "%s: repair left rows uncovered", who);
    for (double& v : d64) v /= rck.min_ratio;
    return UVRT_OK;
}

// f32 durations, rounded up to values that survive SaveRoute / LoadRoute and re-checked in f64; the report
template <typename ET>
int Solve::round_to_f32()
{
    int rc;
    std::vector<double> dh(P);
    std::vector<float> d32(P);
    RowCheck rck{};
    double min_ratio = 0.0;
    if (!bounded) {
        for (int round = 0; round < 8; ++round) {
            for (int p = 0; p < P; ++p) dh[p] = d32[p] = d64[p] > 0.0 ? round_up_f32(d64[p]) : 0.0f;
            if ((rc = row_check<ET>(c, S, false, NR, dh, false, &rck, nullptr))) return rc;
            if (rck.min_ratio >= 1.0) break;
            for (double& v : d64) v *= (1.0 / rck.min_ratio) * (1.0 + 1e-12);
        }
        if (!(rck.min_ratio >= 1.0)) return fail(UVRT_ERR_INVALID, "%s: the f32 durations do not reach the minimum", who);
        min_ratio = rck.min_ratio;
    } else {
        // x = lower + e in f32: lower itself where e is 0, else rounded up as above; checked in x-space over the required
        // rows, every column counted.  A miss rescales the excess the f32 values carry by what the active rows lack.
        for (int round = 0; round < 8; ++round) {
            for (int p = 0; p < P; ++p) dh[p] = d32[p] = d64[p] > 0.0 ? round_up_f32(low[p] + d64[p]) : (float)low[p];
            if ((rc = x_check<ET>(c, S, mprime, dh, &min_ratio))) return rc;
            if (min_ratio >= 1.0) break;
            for (int p = 0; p < P; ++p) dh[p] = fix[p] ? 0.0 : dh[p] - low[p];
            if ((rc = row_check<ET>(c, S, true, NR, dh, false, &rck, nullptr))) return rc;
            const double up = (rck.min_ratio > 0.0 && rck.min_ratio < 1.0 ? 1.0 / rck.min_ratio : 1.0) * (1.0 + 1e-9);
            for (int p = 0; p < P; ++p) d64[p] = std::max(d64[p], dh[p]) * up;
        }
        if (!(min_ratio >= 1.0)) return fail(UVRT_ERR_INVALID, "%s: the f32 durations do not reach the minimum", who);
    }
    double total = 0;
    int used = 0;
    for (int p = 0; p < P; ++p) { out[p] = d32[p]; total += d32[p]; used += d32[p] > 0.0f; }
    rep->iterations = it;
    rep->used_positions = used;
    rep->total_duration = total;
    if (!bounded) {
        rep->lower_bound = std::min(best_lb, total);
        rep->gap = total > 0.0 ? (total - rep->lower_bound) / total : 0.0;
    } else {
        const double excess = total - lower_total;       // what the residual LP decides
        rep->lower_bound = lower_total + std::min(best_lb, excess);
        rep->gap = excess > 0.0 ? (total - rep->lower_bound) / excess : 0.0;
    }
    rep->status = rep->gap <= prm->rel_gap ? UVRT_PLAN_CONVERGED : UVRT_PLAN_ITERATION_CAP;
    rep->min_dose_ratio = min_ratio * (mprime / m);
    return UVRT_OK;
}

template <typename ET>
int plan_solve_t(uvrt_ctx* c, const char* who, const uvrt_plan_params* prm, const uvrt_plan_bounds* bounds, float* out,
                 uvrt_plan_report* rep, uvrt_plan_bounds_report* brep)
{
    Solve v{c, who, prm, bounds, out, rep, brep};
    if (int rc = v.check_arguments()) return rc;
    if (int rc = v.template classify_rows<ET>()) return rc;
    if (v.done) return UVRT_OK;
    if (int rc = v.template cutting_planes<ET>()) return rc;
    if (int rc = v.template repair<ET>()) return rc;
    return v.template round_to_f32<ET>();
}

}  // namespace
