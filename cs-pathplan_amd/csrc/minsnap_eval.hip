// minsnap_eval.hip -- position and its derivatives of a batch of piecewise polynomials at arbitrary query times, and the
// reverse mode of that evaluation (csp_minsnap_eval_batch, csp_minsnap_eval_batch_vjp; contract in include/csp_minsnap.h,
// design in DESIGN.md section 19).  Workspace-free, no atomics: every sum has one owner and a fixed order.
//
// A workgroup owns a tile of consecutive trajectories (minsnap_eval_plan.h).  Their segment times are staged into LDS and
// one lane per trajectory turns them into prefix sums in place, left to right, one rounding per addition: that loop IS
// rule 1 of the contract, and every query of the trajectory searches the same row.
//   forward: one lane per (trajectory, query): binary search of the row, one record load in 2-element vectors, one table
//            of powers of the local time, D x 3 outputs.
//   reverse: the same first phase also forms g_tau = sum g * x^(d+1) and leaves (segment key, tau, g_tau) in LDS; then
//            one lane per (segment, axis) walks its trajectory's keys in ascending q (an LDS broadcast read each) and
//            accumulates its record in registers, so the record is written whole, zeros included.  The lane of axis 0
//            also forms the segment's g_tau sum; one lane per trajectory turns those into grad_times by a suffix sum.
//            More than 85 segments in a tile are taken in blocks of 85, more queries than LDS holds in tiles.
#include "minsnap_eval.h"

#include <climits>
#include <cmath>

namespace csp {
namespace {

using namespace evalk;

constexpr int TRAJ_NONFINITE_BIT = 1, TRAJ_SKIPPED_BIT = 4;   // CSP_TRAJ_NONFINITE, CSP_TRAJ_SKIPPED
constexpr int KEY_HIGH = 1 << 30;                            // the query was clamped to the end of the trajectory

template <typename T> struct Vec2;
template <> struct Vec2<double> { using type = double2; };
template <> struct Vec2<float> { using type = float2; };

// p (p-1) ... (p-d+1); zero for p < d
__host__ __device__ constexpr double falling(int p, int d) {
    double r = 1.0;
    for (int i = 0; i < d; ++i) r *= (double)(p - i > 0 ? p - i : 0);
    return r;
}

__device__ __forceinline__ bool finite_(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

struct Lds {
    double *cum;
    long long *base;
    int *nseg, *bad, *stat;
    double *seg_sum, *hi_sum, *tau, *gt;
    int *key;
};

// the layout of eval_lds_common / plan_eval_vjp (minsnap_eval_plan.h)
__device__ __forceinline__ Lds carve(unsigned char *p, int tb, int smax, int qt) {
    Lds L;
    L.cum = (double *)p;
    p += (size_t)tb * (smax + 1) * 8;
    L.base = (long long *)p;
    p += (size_t)tb * 8;
    L.nseg = (int *)p;
    L.bad = L.nseg + tb;
    L.stat = L.bad + tb;
    p += (size_t)((3 * tb + 1) / 2 * 2) * 4;
    L.seg_sum = (double *)p;
    L.hi_sum = L.seg_sum + (size_t)tb * smax;
    L.tau = L.hi_sum + tb;
    L.gt = L.tau + (size_t)tb * qt;
    L.key = (int *)(L.gt + (size_t)tb * qt);
    return L;
}

// Shapes of the tile's trajectories, then their prefix sums: cum[0] = 0, cum[j+1] = cum[j] + T[j] in fp64.  A
// trajectory with a time that is negative, inf or NaN is marked bad.
template <typename T> __device__ __forceinline__ void stage_cum(const EvalArgs &a, const Lds &L, int64_t b0, int tb_n) {
    const int tid = threadIdx.x, stride = a.Smax + 1;
    for (int tl = tid; tl < tb_n; tl += EVAL_THREADS) {
        const int64_t b = b0 + tl;
        int64_t base, n;
        int st = 0;
        if (a.seg_off) {
            base = a.seg_off[b];
            n = a.seg_off[b + 1] - base;
            if (n < 0 || n > a.Smax) { n = 0; st = TRAJ_SKIPPED_BIT; }
        } else {
            base = b * (int64_t)a.S;
            n = a.S;
        }
        L.base[tl] = base;
        L.nseg[tl] = (int)n;
        L.stat[tl] = st;
    }
    __syncthreads();
    const T *tm = (const T *)a.times;
    for (int i = tid; i < tb_n * a.Smax; i += EVAL_THREADS) {
        const int tl = i / a.Smax, j = i - tl * a.Smax;
        if (j < L.nseg[tl]) L.cum[tl * stride + j + 1] = (double)tm[L.base[tl] + j];
    }
    __syncthreads();
    for (int tl = tid; tl < tb_n; tl += EVAL_THREADS) {
        double *row = L.cum + tl * stride;
        const int n = L.nseg[tl];
        double c = 0.0;
        int bad = 0;
        row[0] = 0.0;
        for (int j = 0; j < n; ++j) {
            const double t = row[j + 1];
            if (!(t >= 0.0 && t <= 1.7976931348623157e308)) bad = 1;
            c += t;
            row[j + 1] = c;
        }
        L.bad[tl] = bad;
        if (bad) L.stat[tl] = TRAJ_NONFINITE_BIT;
    }
    __syncthreads();
}

// largest j in 0..n-1 with cum[j] <= tc (cum is non-decreasing and cum[0] = 0 <= tc)
__device__ __forceinline__ int find_segment(const double *row, int n, double tc) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row[mid] <= tc) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T, int M> __device__ __forceinline__ void load_record(const void *coeffs, int64_t rec, double *c) {
    using V = typename Vec2<T>::type;
    const V *p = (const V *)coeffs + rec * (3 * M / 2);
#pragma unroll
    for (int i = 0; i < 3 * M / 2; ++i) {
        const V v = p[i];
        c[2 * i] = (double)v.x;
        c[2 * i + 1] = (double)v.y;
    }
}

template <int M> __device__ __forceinline__ void powers(double tau, double *pw) {
    pw[0] = 1.0;
#pragma unroll
    for (int i = 1; i < M; ++i) pw[i] = pw[i - 1] * tau;
}

// d-th derivative of sum_k c[k] tau^(M-1-k).  At tau = 0 it is the one term that does not vanish, bit for bit.
template <int M> __device__ __forceinline__ double deriv(const double *c, const double *pw, double tau, int d) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const int p = M - 1 - k;
        if (p >= d) acc += c[k] * (falling(p, d) * pw[p - d]);
    }
    const double at0 = d < M ? c[d < M ? M - 1 - d : 0] * falling(d, d) : 0.0;
    return tau == 0.0 ? at0 : acc;
}

template <typename T, int O>
__global__ void __launch_bounds__(EVAL_THREADS) minsnap_eval_kernel(EvalArgs a, int tb) {
    constexpr int M = 2 * O;
    extern __shared__ __align__(16) unsigned char eval_lds[];
    const Lds L = carve(eval_lds, tb, a.Smax, 0);
    const int tid = threadIdx.x, stride = a.Smax + 1;
    const int64_t b0 = (int64_t)blockIdx.x * tb;
    const int tb_n = (int)(a.B - b0 < tb ? a.B - b0 : tb);
    stage_cum<T>(a, L, b0, tb_n);

    const T *query = (const T *)a.query;
    T *out = (T *)a.out;
    const int64_t nq = (int64_t)tb_n * a.Q;
    const bool small = nq <= INT_MAX;
    const double nan = __builtin_nan("");
    for (int64_t i = tid; i < nq; i += EVAL_THREADS) {
        const int tl = small ? (int)i / (int)a.Q : (int)(i / a.Q);
        const int64_t q = i - (int64_t)tl * a.Q, b = b0 + tl, qi = b * a.Q + q;
        const int n = L.nseg[tl];
        const double t = (double)query[qi];
        T *o = out + qi * (a.D * 3);
        int seg = -1;
        if (n == 0 || L.bad[tl] || !finite_(t)) {
            for (int e = 0; e < a.D * 3; ++e) o[e] = (T)nan;
        } else {
            const double *row = L.cum + tl * stride;
            const double tc = t < 0.0 ? 0.0 : (t > row[n] ? row[n] : t);
            seg = find_segment(row, n, tc);
            const double tau = tc - row[seg];
            double c[3 * M], pw[M];
            load_record<T, M>(a.coeffs, L.base[tl] + seg, c);
            powers<M>(tau, pw);
            bool nonfinite = false;
#pragma unroll
            for (int d = 0; d < EVAL_MAX_DERIVS; ++d) {
                if (d < a.D) {
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const T v = (T)deriv<M>(c + ax * M, pw, tau, d);
                        o[d * 3 + ax] = v;
                        nonfinite |= !finite_((double)v);
                    }
                }
            }
            if (nonfinite) L.stat[tl] = TRAJ_NONFINITE_BIT;   // every writer stores the same value
        }
        if (a.seg_index) a.seg_index[qi] = seg;
    }
    __syncthreads();
    if (a.status)
        for (int tl = tid; tl < tb_n; tl += EVAL_THREADS) a.status[b0 + tl] = L.stat[tl];
}

template <typename T, int O>
__global__ void __launch_bounds__(EVAL_THREADS) minsnap_eval_vjp_kernel(EvalArgs a, int tb, int qt, int blocks) {
    constexpr int M = 2 * O;
    using V = typename Vec2<T>::type;
    extern __shared__ __align__(16) unsigned char eval_lds[];
    const Lds L = carve(eval_lds, tb, a.Smax, qt);
    const int tid = threadIdx.x, stride = a.Smax + 1;
    const int64_t b0 = (int64_t)blockIdx.x * tb;
    const int tb_n = (int)(a.B - b0 < tb ? a.B - b0 : tb);
    stage_cum<T>(a, L, b0, tb_n);

    const T *query = (const T *)a.query, *gout = (const T *)a.grad_out;
    T *gq = (T *)a.grad_query;
    const bool want_c = a.grad_coeffs != nullptr, want_t = a.grad_times != nullptr, scan = want_c || want_t;
    const int64_t ntile = qt > 0 ? (a.Q + qt - 1) / qt : 0;
    const double nan = __builtin_nan("");
    const int sl = tid / 3, ax = tid - sl * 3;

    for (int kb = 0; kb < (scan ? blocks : 1); ++kb) {
        const int f0 = kb * EVAL_BLOCK_SEGS;
        // the record this lane owns in this block: segment sj of the tile's trajectory stl, axis ax
        const int f = f0 + sl;
        bool own = scan && sl < EVAL_BLOCK_SEGS && f < tb_n * a.Smax;
        const int stl = own ? f / a.Smax : 0, sj = f - stl * a.Smax;
        own = own && sj < L.nseg[stl];
        double acc[M];
#pragma unroll
        for (int k = 0; k < M; ++k) acc[k] = 0.0;
        double ssum = 0.0, hsum = 0.0;

        for (int64_t tile = 0; tile < ntile; ++tile) {
            const int64_t q0 = tile * qt;
            const int nqt = (int)(a.Q - q0 < qt ? a.Q - q0 : qt);
            __syncthreads();   // the previous tile's walk is over
            for (int i = tid; i < tb_n * nqt; i += EVAL_THREADS) {
                const int tl = i / nqt, ql = i - tl * nqt, slot = tl * qt + ql;
                const int64_t qi = (b0 + tl) * a.Q + q0 + ql;
                const int n = L.nseg[tl];
                const double t = (double)query[qi];
                int key = -1;
                if (n == 0 || L.bad[tl] || !finite_(t)) {
                    if (kb == 0 && gq) gq[qi] = n == 0 ? (T)0.0 : (T)nan;
                } else {
                    const double *row = L.cum + tl * stride;
                    const bool low = t < 0.0, high = t > row[n];
                    const double tc = low ? 0.0 : (high ? row[n] : t);
                    const int j = find_segment(row, n, tc);
                    const int fq = tl * a.Smax + j - f0;
                    if (!scan || (fq >= 0 && fq < EVAL_BLOCK_SEGS)) {
                        const double tau = tc - row[j];
                        double c[3 * M], pw[M];
                        load_record<T, M>(a.coeffs, L.base[tl] + j, c);
                        powers<M>(tau, pw);
                        const T *g = gout + qi * (a.D * 3);
                        double gtau = 0.0;
#pragma unroll
                        for (int d = 0; d < EVAL_MAX_DERIVS; ++d) {
                            if (d < a.D) {
#pragma unroll
                                for (int x = 0; x < 3; ++x) gtau += (double)g[d * 3 + x] * deriv<M>(c + x * M, pw, tau, d + 1);
                            }
                        }
                        if (gq) {
                            const T v = (low || high) ? (T)0.0 : (T)gtau;
                            gq[qi] = v;
                            if (!finite_((double)v)) L.stat[tl] = TRAJ_NONFINITE_BIT;
                        }
                        key = fq | (high ? KEY_HIGH : 0);
                        L.tau[slot] = tau;
                        L.gt[slot] = low ? 0.0 : gtau;   // a query clamped to the start depends on no time
                    }
                }
                L.key[slot] = key;
            }
            __syncthreads();
            if (own) {
                const int *kp = L.key + stl * qt;
                for (int ql = 0; ql < nqt; ++ql) {
                    const int key = kp[ql];
                    if (key < 0 || (key & (KEY_HIGH - 1)) != sl) continue;
                    const int slot = stl * qt + ql;
                    if (ax == 0) {
                        const double g = L.gt[slot];
                        if (key & KEY_HIGH) hsum += g;   // tau = T[S-1] there: the last segment's time alone
                        else ssum += g;
                    }
                    if (want_c) {
                        double pw[M];
                        powers<M>(L.tau[slot], pw);
                        const T *g = gout + ((b0 + stl) * a.Q + q0 + ql) * (a.D * 3) + ax;
#pragma unroll
                        for (int d = 0; d < EVAL_MAX_DERIVS; ++d) {
                            if (d < a.D) {
                                const double gv = (double)g[d * 3];
#pragma unroll
                                for (int k = 0; k < M; ++k) {
                                    const int p = M - 1 - k;
                                    if (p >= d) acc[k] += gv * (falling(p, d) * pw[p - d]);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (own) {
            const bool bad = L.bad[stl] != 0;
            if (want_c) {
                V *rec = (V *)a.grad_coeffs + ((L.base[stl] + sj) * 3 + ax) * (M / 2);
                bool nonfinite = false;
#pragma unroll
                for (int i = 0; i < M / 2; ++i) {
                    V v;
                    v.x = bad ? (T)nan : (T)acc[2 * i];
                    v.y = bad ? (T)nan : (T)acc[2 * i + 1];
                    rec[i] = v;
                    nonfinite |= !finite_((double)v.x) || !finite_((double)v.y);
                }
                if (nonfinite && !bad) L.stat[stl] = TRAJ_NONFINITE_BIT;
            }
            if (ax == 0) {
                L.seg_sum[stl * a.Smax + sj] = ssum;
                if (sj == L.nseg[stl] - 1) L.hi_sum[stl] = hsum;
            }
        }
    }
    __syncthreads();
    // grad_times[i] = -(sum of the later segments' in-range sums), plus the clamped-high queries' sum for the last segment
    if (want_t) {
        for (int tl = tid; tl < tb_n; tl += EVAL_THREADS) {
            const int n = L.nseg[tl];
            const bool bad = L.bad[tl] != 0;
            T *gt = (T *)a.grad_times + L.base[tl];
            const double *ss = L.seg_sum + tl * a.Smax;
            double suf = 0.0;
            bool nonfinite = false;
            for (int i = n - 1; i >= 0; --i) {
                const T v = bad ? (T)nan : (T)(i == n - 1 ? L.hi_sum[tl] : 0.0 - suf);
                gt[i] = v;
                nonfinite |= !finite_((double)v);
                suf += ss[i];
            }
            if (nonfinite && !bad) L.stat[tl] = TRAJ_NONFINITE_BIT;
        }
        __syncthreads();
    }
    if (a.status)
        for (int tl = tid; tl < tb_n; tl += EVAL_THREADS) a.status[b0 + tl] = L.stat[tl];
}

template <typename T, int O> hipError_t launch_fwd_o(const EvalArgs &a, hipStream_t st) {
    const EvalPlan p = plan_eval_forward(a.Smax, a.B);
    if (p.lds_bytes > 65536 || p.grid > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL((minsnap_eval_kernel<T, O>), dim3((unsigned)p.grid), dim3(EVAL_THREADS), p.lds_bytes, st, a, p.tb);
    return hipGetLastError();
}

template <typename T, int O> hipError_t launch_vjp_o(const EvalArgs &a, hipStream_t st) {
    const EvalPlan p = plan_eval_vjp(a.Smax, a.Q, a.B);
    if (p.lds_bytes > 65536 || p.grid > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL((minsnap_eval_vjp_kernel<T, O>), dim3((unsigned)p.grid), dim3(EVAL_THREADS), p.lds_bytes, st, a, p.tb,
                       p.qt, p.blocks);
    return hipGetLastError();
}

template <typename T> hipError_t launch_io(const EvalArgs &a, bool vjp, hipStream_t st) {
    switch (a.order) {
        case 2: return vjp ? launch_vjp_o<T, 2>(a, st) : launch_fwd_o<T, 2>(a, st);
        case 3: return vjp ? launch_vjp_o<T, 3>(a, st) : launch_fwd_o<T, 3>(a, st);
        case 4: return vjp ? launch_vjp_o<T, 4>(a, st) : launch_fwd_o<T, 4>(a, st);
        case 5: return vjp ? launch_vjp_o<T, 5>(a, st) : launch_fwd_o<T, 5>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_eval(const EvalArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0 || a.Q == 0) return hipSuccess;
    if (!eval_supported(a.order, a.Smax)) return hipErrorInvalidValue;
    return f32 ? launch_io<float>(a, false, st) : launch_io<double>(a, false, st);
}

hipError_t launch_eval_vjp(const EvalArgs &a, bool f32, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    if (!eval_supported(a.order, a.Smax)) return hipErrorInvalidValue;
    return f32 ? launch_io<float>(a, true, st) : launch_io<double>(a, true, st);
}

}  // namespace csp
